// go2nn_sensor.h — the evaluator's sensor model: noise, bias, latency and dropped frames between the simulator's observation and the policy (include/go2nn.h:
// go2nn_sensor_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp after go2nn_maneuver.h (FAIL, HIPCHK are the former's helpers; EVAL_FN, eval_f go2nn_eval.h's; the cursor kernel go2nn_trace.h's).
//
// go2nn_sensor_apply: one launch per env step, one lane per OUTPUT float: lane i handles column c = i % D of env e = i / D, so the row-major [N, D] observation, the ring
// slot, `held` and the output are all read and written densely, 256 bytes per wave instruction.  A lane touches only its own (e, c) entries of the ring and of `held`: no
// LDS, no atomics, no cross-lane traffic, and a lane that reads a delayed value reads what the SAME lane stored in an earlier launch.  The spec (32 bytes, at most 64 of
// them), scale[c] and kind[c] stay in L2 / the vector cache; the ring of 1024 x 45 x 5 floats is 0.9 MB and stays in L2.  Launch-bound at evaluation sizes (46080 lanes
// = 180 workgroups).  The step is the cursor, read from device memory (every lane reads the same address: one broadcast load) and advanced by a second, one-lane launch
// on the same stream — the recorder's pattern (go2nn_trace.h) —, so no host argument changes between steps and a captured pair advances on every replay.
// The host build runs the same element function in plain loops.
//
// THE UNIFORMS.  u = (x >> 8) * 2^-24 in [0, 1) with x = word 0 of philox4x32_10 (go2_math.h) under
//   key     = (seed, tag)            tag: 1 noise, 2 bias, 3 drop
//   counter = (env, column, step, 0) the bias has no step (0): one draw per (env, column) for the whole evaluation;  the drop has no column (0): one draw per (env, step)
// with env, column and step as uint32.  2 u - 1 is exact in fp32 (a multiple of 2^-23 of magnitude <= 1).
#ifndef GO2NN_SENSOR_H
#define GO2NN_SENSOR_H

#include "go2_math.h"

#define SENSOR_THREADS 256
#define SENSOR_TAG_NOISE 1u
#define SENSOR_TAG_BIAS 2u
#define SENSOR_TAG_DROP 3u
#define SENSOR_RING (GO2NN_SENSOR_MAX_DELAY + 1)
#define SENSOR_HEADER_BYTES 256          // the cursor's own cache lines: the ring starts 256-byte aligned

EVAL_FN int sensor_slot(int s) { return ((s % SENSOR_RING) + SENSOR_RING) % SENSOR_RING; }

// column c of env e at step s: the rule of include/go2nn.h -> the delivered value (also left in held)
EVAL_FN float sensor_lane(const Go2nnSensorIn& in, const Go2nnSensorSpec* specs, const int32_t* sensor_of_env, float* ring, float* held, int N, int s, int e, int c) {
  const long long i = (long long)e * in.D + c, slot = (long long)N * in.D;
  const float x = eval_f(in.obs, e, c);
  const bool fresh = s == 0 || in.dones[e] != 0;
  if (fresh) {
    for (int r = 0; r < SENSOR_RING; ++r) ring[r * slot + i] = x;
  } else {
    ring[sensor_slot(s) * slot + i] = x;
  }
  const int p = sensor_of_env[e];
  if (p < 0 || p >= in.num_specs) return held[i] = x;
  const Go2nnSensorSpec sp = specs[p];
  const int kind = in.kind[c];
  float src = x;
  if (kind != GO2NN_SENSOR_PASS && !fresh) {
    const int d = sp.delay < 0 ? 0 : (sp.delay > GO2NN_SENSOR_MAX_DELAY ? GO2NN_SENSOR_MAX_DELAY : sp.delay);          // (the host check's duty; never outside the ring)
    if (d > 0) src = ring[sensor_slot(s - d) * slot + i];
    if (sp.drop > 0.f && philox_u01((uint32_t)e, 0u, (uint32_t)s, 0u, in.seed, SENSOR_TAG_DROP, 0) < sp.drop) return held[i];          // held stays what it is
  }
  const float mag = kind == GO2NN_SENSOR_GYRO ? sp.gyro_bias : (kind == GO2NN_SENSOR_GRAVITY ? sp.gravity_bias : (kind == GO2NN_SENSOR_JOINT_POS ? sp.joint_offset : 0.f));
  const float k = in.scale[c] * sp.noise_mul;          // one rounded product, a constant of (spec, column)
  if (mag == 0.f && k == 0.f) return held[i] = src;    // nothing to add: the bits go through (no add of zero, no clamp)
  float v = src;
  if (mag != 0.f) v += (2.f * philox_u01((uint32_t)e, (uint32_t)c, 0u, 0u, in.seed, SENSOR_TAG_BIAS, 0) - 1.f) * mag;
  if (k != 0.f) v += (2.f * philox_u01((uint32_t)e, (uint32_t)c, (uint32_t)s, 0u, in.seed, SENSOR_TAG_NOISE, 0) - 1.f) * k;
  return held[i] = fminf(fmaxf(v, -in.clip), in.clip);
}

// where the three parts of the state allocation are (host and device code both ask)
#ifdef GO2_EMU
#define SENSOR_HD static inline
#else
#define SENSOR_HD __host__ __device__ __forceinline__
#endif
SENSOR_HD int32_t* sensor_cursor(void* state) { return (int32_t*)state; }
SENSOR_HD float* sensor_ring(void* state) { return (float*)((char*)state + SENSOR_HEADER_BYTES); }
SENSOR_HD float* sensor_held(void* state, int N, int D) { return sensor_ring(state) + (long long)SENSOR_RING * N * D; }

#ifndef GO2_EMU
__global__ void __launch_bounds__(SENSOR_THREADS) go2nn_sensor_apply_kernel(const Go2nnSensorIn in, const Go2nnSensorSpec* specs, const int32_t* sensor_of_env, void* state,
                                                                            float* out, int N) {
  const int i = blockIdx.x * SENSOR_THREADS + threadIdx.x;
  if (i >= N * in.D) return;
  out[i] = sensor_lane(in, specs, sensor_of_env, sensor_ring(state), sensor_held(state, N, in.D), N, *sensor_cursor(state), i / in.D, i % in.D);
}
#endif

static const char* sensor_in_bad(const Go2nnSensorIn* in, int N) {
  if (!in->obs.p || !in->dones || !in->scale || !in->kind) return "a null buffer pointer";
  if (in->obs.env_stride < 1 || in->obs.comp_stride < 1) return "an observation field with an env stride or a component stride < 1";
  if (in->D < 1 || in->D > GO2NN_SENSOR_MAX_WIDTH) return "D outside [1, 64]";
  if (in->num_specs < 1 || in->num_specs > GO2NN_SENSOR_MAX_SPECS) return "num_specs outside [1, 64]";
  if (!(in->clip > 0.f)) return "clip <= 0 (or NaN)";
  if ((long long)N * in->D * (SENSOR_RING + 1) > 0x7fffffffLL / 4) return "N * D too large";
  return nullptr;
}

extern "C" {

int go2nn_sensor_check_specs(const Go2nnSensorSpec* specs, int32_t P, const int32_t* kind, const float* scale, int32_t D) {
  if (!specs || !kind || !scale) FAIL(GO2NN_EINVAL, "sensor specs: null pointer");
  if (P < 1 || P > GO2NN_SENSOR_MAX_SPECS) FAIL(GO2NN_EINVAL, "sensor specs: P = %d conditions (1 .. %d)", P, GO2NN_SENSOR_MAX_SPECS);
  if (D < 1 || D > GO2NN_SENSOR_MAX_WIDTH) FAIL(GO2NN_EINVAL, "sensor specs: D = %d observation columns (1 .. %d)", D, GO2NN_SENSOR_MAX_WIDTH);
  for (int c = 0; c < D; ++c) {
    if (kind[c] < GO2NN_SENSOR_PASS || kind[c] > GO2NN_SENSOR_JOINT_VEL) FAIL(GO2NN_EINVAL, "sensor layout: kind[%d] = %d (0 .. 4)", c, kind[c]);
    if (!(scale[c] >= 0.f && scale[c] <= 3.0e38f)) FAIL(GO2NN_EINVAL, "sensor layout: scale[%d] = %g (finite, >= 0)", c, (double)scale[c]);
  }
  for (int p = 0; p < P; ++p) {
    const Go2nnSensorSpec& s = specs[p];
    if (s.delay < 0 || s.delay > GO2NN_SENSOR_MAX_DELAY) FAIL(GO2NN_EINVAL, "sensor spec %d: delay = %d steps (0 .. %d)", p, s.delay, GO2NN_SENSOR_MAX_DELAY);
    if (!(s.drop >= 0.f && s.drop < 1.f)) FAIL(GO2NN_EINVAL, "sensor spec %d: drop = %g (a probability in [0, 1))", p, (double)s.drop);
    const float mags[] = {s.noise_mul, s.gyro_bias, s.gravity_bias, s.joint_offset};
    for (float m : mags)
      if (!(m >= 0.f && m <= 3.0e38f))
        FAIL(GO2NN_EINVAL, "sensor spec %d: magnitude %g (noise_mul, gyro_bias, gravity_bias, joint_offset: finite, >= 0)", p, (double)m);
  }
  return 0;
}

int64_t go2nn_sensor_state_bytes(int32_t N, int32_t D) {
  if (N < 1 || D < 1 || D > GO2NN_SENSOR_MAX_WIDTH) return 0;
  return SENSOR_HEADER_BYTES + (int64_t)(SENSOR_RING + 1) * N * D * (int64_t)sizeof(float);
}

int go2nn_sensor_begin(void* state, void* stream) {
  if (!state) FAIL(GO2NN_EINVAL, "sensor begin: null state");
#ifdef GO2_EMU
  (void)stream;
  *sensor_cursor(state) = 0;
#else
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sensor_cursor(state), -1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_sensor_apply(const Go2nnSensorIn* in, const Go2nnSensorSpec* specs, const int32_t* sensor_of_env, void* state, float* out, int32_t N, void* stream) {
  if (!in || !specs || !sensor_of_env || !state || !out || N < 1) FAIL(GO2NN_EINVAL, "sensor apply: null argument or N < 1");
  if (const char* bad = sensor_in_bad(in, N)) FAIL(GO2NN_EINVAL, "sensor apply: %s", bad);
  const int n = N * in->D;
#ifdef GO2_EMU
  (void)stream;
  const int s = *sensor_cursor(state);
  for (int i = 0; i < n; ++i) out[i] = sensor_lane(*in, specs, sensor_of_env, sensor_ring(state), sensor_held(state, N, in->D), N, s, i / in->D, i % in->D);
  *sensor_cursor(state) = s + 1;
#else
  hipLaunchKernelGGL(go2nn_sensor_apply_kernel, dim3((unsigned)((n + SENSOR_THREADS - 1) / SENSOR_THREADS)), dim3(SENSOR_THREADS), 0, (hipStream_t)stream, *in, specs,
                     sensor_of_env, state, out, N);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sensor_cursor(state), 1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_SENSOR_H
