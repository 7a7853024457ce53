// go2nn_sensor_rand.h — TRAINING under randomised sensor latency, dropped frames and constant offsets (include/go2nn.h: go2nn_sensor_rand_*, added within ABI 7;
// go2_rl_gym_amd/envs/base/legged_robot.py, domain_rand.randomize_sensors).
// Included at the end of go2nn_impl.cpp after go2nn_sensor.h, whose ring, cursor header, slot function and launch shape it shares.
//
// The evaluator's kernel gives every robot one fixed condition out of a table for a whole run; this one redraws the condition per robot and per EPISODE from continuous
// ranges, keyed by the cursor value at which the episode began.  go2nn_sensor_rand_apply: one launch per env step, one lane per OUTPUT float: lane i handles column
// c = i % D of env e = i / D; the observation, the ring slot, `held`, `start` and the output are read and written densely.  A lane touches only its own (e, c) entries
// of the ring, of `held` and of `start` — an env's 45 lanes straddle waves, so a per-env entry written by one of them and read by the others in the same launch would be a
// race; a per-lane entry is not: no LDS, no atomics, no cross-lane traffic.  The episode's draws are not cached: a lane that is not PASS recomputes them from `start`
// (two Philox blocks, ~100 integer instructions) and one more block for the drop decision, which is nothing next to the launch itself: at 4096 x 45 lanes the kernel moves
// 5 MB and is launch-bound on the rollout's dependent chain.  The Go2nnSensorRand (32 bytes) travels by value in the kernel arguments.
// The step is the cursor, read from device memory and advanced by the one-lane cursor kernel (go2nn_trace.h) as a second launch on the same stream, so a captured pair
// advances on every replay of the rollout graph.  The host build runs the same element function in plain loops.
//
// THE UNIFORMS.  u = (x >> 8) * 2^-24 in [0, 1) with x a word of philox4x32_10 (go2_math.h), g = env_offset + e the env's GLOBAL id, s0 the episode's first cursor value:
//   key (seed, 4)  counter (g, 0, s0, 0)   word 0: the episode's delay, word 1: the episode's drop probability
//   key (seed, 5)  counter (g, c, s0, 0)   word 0: the episode's offset of column c
//   key (seed, 6)  counter (g, 0, s,  0)   word 0: is the frame of step s lost
// Tags 4 .. 6 keep these streams apart from the evaluator's 1 .. 3.
#ifndef GO2NN_SENSOR_RAND_H
#define GO2NN_SENSOR_RAND_H

#include "go2nn_sensor.h"

#define SENSOR_TAG_EPISODE 4u
#define SENSOR_TAG_EPISODE_BIAS 5u
#define SENSOR_TAG_EPISODE_DROP 6u

// column c of env e at step s: the rule of include/go2nn.h -> the delivered value (also left in held)
EVAL_FN float sensor_rand_lane(const Go2nnSensorIn& in, const Go2nnSensorRand& r, const uint8_t* also_fresh, float* ring, float* held, int32_t* start, int N, int s, int e, int c) {
  const long long i = (long long)e * in.D + c, slot = (long long)N * in.D;
  const float x = eval_f(in.obs, e, c);
  const bool fresh = s == 0 || in.dones[e] != 0 || (also_fresh != nullptr && also_fresh[e] != 0);
  int s0 = s;
  if (fresh) {
    for (int k = 0; k < SENSOR_RING; ++k) ring[k * slot + i] = x;
    start[i] = s;
  } else {
    ring[sensor_slot(s) * slot + i] = x;
    s0 = start[i];
  }
  const int kind = in.kind[c];
  if (kind == GO2NN_SENSOR_PASS) return held[i] = x;
  const uint32_t g = r.env_offset + (uint32_t)e;
  uint32_t w[4];
  philox4x32_10(g, 0u, (uint32_t)s0, 0u, in.seed, SENSOR_TAG_EPISODE, w);
  const int span = r.delay_hi - r.delay_lo;
  const int k = (int)(u01_from_bits(w[0]) * (float)(span + 1));
  int delay = r.delay_lo + (k < span ? k : span);
  delay = delay < 0 ? 0 : (delay > GO2NN_SENSOR_MAX_DELAY ? GO2NN_SENSOR_MAX_DELAY : delay);          // (the host check's duty; never outside the ring)
  const float p = r.drop_lo + u01_from_bits(w[1]) * (r.drop_hi - r.drop_lo);
  if (!fresh && p > 0.f && philox_u01(g, 0u, (uint32_t)s, 0u, in.seed, SENSOR_TAG_EPISODE_DROP, 0) < p) return held[i];          // held stays what it is
  const float src = (fresh || delay == 0) ? x : ring[sensor_slot(s - delay) * slot + i];
  const float mag = kind == GO2NN_SENSOR_GYRO ? r.gyro_bias : (kind == GO2NN_SENSOR_GRAVITY ? r.gravity_bias : (kind == GO2NN_SENSOR_JOINT_POS ? r.joint_offset : 0.f));
  if (mag == 0.f) return held[i] = src;          // nothing to add: the bits go through (no add of zero, no clamp)
  const float v = src + (2.f * philox_u01(g, (uint32_t)c, (uint32_t)s0, 0u, in.seed, SENSOR_TAG_EPISODE_BIAS, 0) - 1.f) * mag;
  return held[i] = fminf(fmaxf(v, -in.clip), in.clip);
}

// the state allocation: go2nn_sensor.h's header, ring and held, then start [N][D] int32
SENSOR_HD int32_t* sensor_rand_start(void* state, int N, int D) { return (int32_t*)(sensor_held(state, N, D) + (long long)N * D); }

#ifndef GO2_EMU
__global__ void __launch_bounds__(SENSOR_THREADS) go2nn_sensor_rand_apply_kernel(const Go2nnSensorIn in, const Go2nnSensorRand r, const uint8_t* also_fresh, void* state,
                                                                                 float* out, int N) {
  const int i = blockIdx.x * SENSOR_THREADS + threadIdx.x;
  if (i >= N * in.D) return;
  out[i] = sensor_rand_lane(in, r, also_fresh, sensor_ring(state), sensor_held(state, N, in.D), sensor_rand_start(state, N, in.D), N, *sensor_cursor(state), i / in.D,
                            i % in.D);
}
#endif

static const char* sensor_rand_bad(const Go2nnSensorRand* r) {
  if (r->delay_lo < 0) return "delay_lo < 0";
  if (r->delay_hi > GO2NN_SENSOR_MAX_DELAY) return "delay_hi above GO2NN_SENSOR_MAX_DELAY";
  if (r->delay_lo > r->delay_hi) return "delay_lo > delay_hi";
  if (!(r->drop_lo >= 0.f)) return "drop_lo negative (or NaN)";
  if (!(r->drop_hi < 1.f)) return "drop_hi not below 1 (or NaN)";
  if (!(r->drop_lo <= r->drop_hi)) return "drop_lo > drop_hi";
  if (!(r->gyro_bias >= 0.f && r->gyro_bias <= 3.0e38f)) return "gyro_bias negative or not finite";
  if (!(r->gravity_bias >= 0.f && r->gravity_bias <= 3.0e38f)) return "gravity_bias negative or not finite";
  if (!(r->joint_offset >= 0.f && r->joint_offset <= 3.0e38f)) return "joint_offset negative or not finite";
  return nullptr;
}

extern "C" {

int go2nn_sensor_rand_check(const Go2nnSensorRand* r, const int32_t* kind, int32_t D) {
  if (!r || !kind) FAIL(GO2NN_EINVAL, "sensor randomisation: null pointer");
  if (D < 1 || D > GO2NN_SENSOR_MAX_WIDTH) FAIL(GO2NN_EINVAL, "sensor randomisation: D = %d observation columns (1 .. %d)", D, GO2NN_SENSOR_MAX_WIDTH);
  for (int c = 0; c < D; ++c)
    if (kind[c] < GO2NN_SENSOR_PASS || kind[c] > GO2NN_SENSOR_JOINT_VEL) FAIL(GO2NN_EINVAL, "sensor randomisation: kind[%d] = %d (0 .. 4)", c, kind[c]);
  if (const char* bad = sensor_rand_bad(r))
    FAIL(GO2NN_EINVAL, "sensor randomisation: %s (delay %d .. %d, drop %g .. %g, gyro_bias %g, gravity_bias %g, joint_offset %g)", bad, r->delay_lo, r->delay_hi,
         (double)r->drop_lo, (double)r->drop_hi, (double)r->gyro_bias, (double)r->gravity_bias, (double)r->joint_offset);
  return 0;
}

int64_t go2nn_sensor_rand_state_bytes(int32_t N, int32_t D) {
  if (N < 1 || D < 1 || D > GO2NN_SENSOR_MAX_WIDTH) return 0;
  return SENSOR_HEADER_BYTES + (int64_t)(SENSOR_RING + 2) * N * D * (int64_t)sizeof(float);
}

int go2nn_sensor_rand_begin(void* state, void* stream) {
  if (!state) FAIL(GO2NN_EINVAL, "sensor randomisation begin: null state");
#ifdef GO2_EMU
  (void)stream;
  *sensor_cursor(state) = 0;
#else
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sensor_cursor(state), -1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_sensor_rand_apply(const Go2nnSensorIn* in, const Go2nnSensorRand* r, const uint8_t* also_fresh, void* state, float* out, int32_t N, void* stream) {
  if (!in || !r || !state || !out || N < 1) FAIL(GO2NN_EINVAL, "sensor randomisation apply: null argument or N < 1");
  if (!in->obs.p || !in->dones || !in->kind) FAIL(GO2NN_EINVAL, "sensor randomisation apply: a null buffer pointer");
  if (in->obs.env_stride < 1 || in->obs.comp_stride < 1) FAIL(GO2NN_EINVAL, "sensor randomisation apply: an observation field with an env stride or a component stride < 1");
  if (in->D < 1 || in->D > GO2NN_SENSOR_MAX_WIDTH) FAIL(GO2NN_EINVAL, "sensor randomisation apply: D outside [1, 64]");
  if (!(in->clip > 0.f)) FAIL(GO2NN_EINVAL, "sensor randomisation apply: clip <= 0 (or NaN)");
  if ((long long)N * in->D * (SENSOR_RING + 2) > 0x7fffffffLL / 4) FAIL(GO2NN_EINVAL, "sensor randomisation apply: N * D too large");
  if (const char* bad = sensor_rand_bad(r)) FAIL(GO2NN_EINVAL, "sensor randomisation apply: %s", bad);
  const int n = N * in->D;
#ifdef GO2_EMU
  (void)stream;
  const int s = *sensor_cursor(state);
  for (int i = 0; i < n; ++i)
    out[i] = sensor_rand_lane(*in, *r, also_fresh, sensor_ring(state), sensor_held(state, N, in->D), sensor_rand_start(state, N, in->D), N, s, i / in->D, i % in->D);
  *sensor_cursor(state) = s + 1;
#else
  hipLaunchKernelGGL(go2nn_sensor_rand_apply_kernel, dim3((unsigned)((n + SENSOR_THREADS - 1) / SENSOR_THREADS)), dim3(SENSOR_THREADS), 0, (hipStream_t)stream, *in, *r,
                     also_fresh, state, out, N);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sensor_cursor(state), 1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_SENSOR_RAND_H
