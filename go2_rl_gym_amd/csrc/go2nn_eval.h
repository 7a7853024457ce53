// go2nn_eval.h — the policy evaluator's metric kernels (include/go2nn.h: go2nn_eval_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp (FAIL, HIPCHK are its helpers).
//
// go2nn_eval_accumulate: one launch per env step, one lane per env.  A lane reads its env's ~75 input values through (env stride, component stride) pairs — with the
// HIP simulator's field-major buffers consecutive lanes read consecutive addresses of every component, i.e. each load instruction of a wave is one dense 256-byte line —
// and read-modify-writes its column of the metric-major accumulator [GO2NN_EVAL_NUM, N] (dense again).  No LDS, no atomics, no cross-lane traffic: a streaming kernel of
// ~0.4 KB per env.  go2nn_eval_reduce: one workgroup per (group, output column): lane t adds the envs t, t + 256, ... of the group in fp64, then a fixed LDS tree over the
// 256 partials — the order is a function of (N, G) only.  The host build runs the same element function and the same summation order in plain loops.
#ifndef GO2NN_EVAL_H
#define GO2NN_EVAL_H

#ifdef GO2_EMU
#define EVAL_FN static inline
#define EVAL_MEMBER inline
#else
#define EVAL_FN __device__ __forceinline__
#define EVAL_MEMBER __device__ __forceinline__
#endif
#define EVAL_THREADS 256

EVAL_FN float eval_f(const Go2nnEvalField& f, int e, int c) { return ((const float*)f.p)[(long long)e * f.env_stride + (long long)c * f.comp_stride]; }
EVAL_FN uint8_t eval_b(const Go2nnEvalField& f, int e) { return ((const uint8_t*)f.p)[(long long)e * f.env_stride]; }

// the ten terms of env e for one step (the table of include/go2nn.h), added to acc[m * N + e]
EVAL_FN void eval_accumulate_env(const Go2nnEvalIn& in, float* acc, int N, int e) {
  const float cx = eval_f(in.commands, e, 0), cy = eval_f(in.commands, e, 1), cw = eval_f(in.commands, e, 2);
  const float vx = eval_f(in.base_lin_vel, e, 0), vy = eval_f(in.base_lin_vel, e, 1);
  const float dx = cx - vx, dy = cy - vy;
  const float cn = sqrtf(cx * cx + cy * cy);
  const float gx = eval_f(in.projected_gravity, e, 0), gy = eval_f(in.projected_gravity, e, 1);
  float power = 0.f, tsq = 0.f, rate = 0.f;
  bool out = false;
  for (int j = 0; j < 12; ++j) {
    const long long q_at = (long long)e * in.dof_state.env_stride + (long long)j * in.dof_state.comp_stride;
    const float q = ((const float*)in.dof_state.p)[q_at], qd = ((const float*)in.dof_state.p)[q_at + in.dof_vel_offset];
    const float tau = eval_f(in.torques, e, j);
    const float da = eval_f(in.actions, e, j) - eval_f(in.last_actions, e, j);
    power += fabsf(tau * qd);
    tsq += tau * tau;
    rate += da * da;
    out = out || q < in.dof_limits[2 * j] || q > in.dof_limits[2 * j + 1];
  }
  const bool fall = eval_b(in.reset_buf, e) != 0 && eval_b(in.time_out_buf, e) == 0;
  float t[GO2NN_EVAL_NUM];
  t[GO2NN_EVAL_STEPS] = 1.f;
  t[GO2NN_EVAL_LIN_VEL_ERR] = sqrtf(dx * dx + dy * dy);
  t[GO2NN_EVAL_ANG_VEL_ERR] = fabsf(cw - eval_f(in.base_ang_vel, e, 2));
  t[GO2NN_EVAL_SPEED_ALONG_CMD] = cn < 1e-6f ? 0.f : (vx * cx + vy * cy) / cn;
  t[GO2NN_EVAL_TILT] = sqrtf(gx * gx + gy * gy);
  t[GO2NN_EVAL_POWER] = power;
  t[GO2NN_EVAL_TORQUE_SQ] = tsq;
  t[GO2NN_EVAL_ACTION_RATE_SQ] = rate;
  t[GO2NN_EVAL_DOF_LIMIT_STEPS] = out ? 1.f : 0.f;
  t[GO2NN_EVAL_FALLS] = fall ? 1.f : 0.f;
  for (int m = 0; m < GO2NN_EVAL_NUM; ++m) acc[(long long)m * N + e] += t[m];
}

// what env e contributes to output column c of its group: the ten accumulators, 1 (the group's size), 1 if the env never fell
EVAL_FN double eval_reduce_term(const float* acc, int N, int e, int c) {
  if (c < GO2NN_EVAL_NUM) return (double)acc[(long long)c * N + e];
  if (c == GO2NN_EVAL_NUM) return 1.0;
  return acc[(long long)GO2NN_EVAL_FALLS * N + e] == 0.f ? 1.0 : 0.0;
}

struct EvalTerm {
  const float* acc; int N, c;
  EVAL_MEMBER double operator()(int e) const { return eval_reduce_term(acc, N, e, c); }
};

// The sum of term(e) over the envs e of group g, in an order that depends on N only: partial t adds the envs t, t + 256, ... in fp64, then a fixed tree over the 256
// partials.  Device: called by every thread of a 256-thread workgroup, the sum is valid in thread 0.  Shared by go2nn_eval_reduce and go2nn_robust_reduce (go2nn_robust.h).
#ifdef GO2_EMU
template <class Term> static inline double eval_group_sum(const int32_t* group, int N, int g, Term term) {
  double part[EVAL_THREADS];
  for (int t = 0; t < EVAL_THREADS; ++t) {
    double s = 0.0;
    for (int e = t; e < N; e += EVAL_THREADS)
      if (group[e] == g) s += term(e);
    part[t] = s;
  }
  for (int w = EVAL_THREADS / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) part[t] += part[t + w];
  return part[0];
}
#else
template <class Term> __device__ __forceinline__ double eval_group_sum(const int32_t* group, int N, int g, Term term) {
  __shared__ double part[EVAL_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int e = t; e < N; e += EVAL_THREADS)
    if (group[e] == g) s += term(e);
  part[t] = s;
  __syncthreads();
  for (int w = EVAL_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  return part[0];
}
#endif

#ifndef GO2_EMU
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_eval_accumulate_kernel(const Go2nnEvalIn in, float* acc, int N) {
  const int e = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (e < N) eval_accumulate_env(in, acc, N, e);
}
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_eval_clear_kernel(float* acc, long long n) {
  const long long k = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (k < n) acc[k] = 0.f;
}
// grid = (G, GO2NN_EVAL_NUM + 2)
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_eval_reduce_kernel(const float* acc, const int32_t* group, int N, double* out) {
  const int g = blockIdx.x, c = blockIdx.y;
  const double s = eval_group_sum(group, N, g, EvalTerm{acc, N, c});
  if (threadIdx.x == 0) out[(long long)g * (GO2NN_EVAL_NUM + 2) + c] = s;
}
#endif

static int eval_in_ok(const Go2nnEvalIn* in) {
  const Go2nnEvalField* f[] = {&in->commands, &in->base_lin_vel, &in->base_ang_vel, &in->projected_gravity, &in->dof_state, &in->torques, &in->actions, &in->last_actions,
                               &in->reset_buf, &in->time_out_buf};
  for (const Go2nnEvalField* x : f)
    if (!x->p || x->env_stride < 1 || x->comp_stride < 0) return 0;
  return in->dof_limits != nullptr && in->dof_vel_offset >= 1;
}

extern "C" {

int go2nn_eval_clear(float* acc, int32_t N, void* stream) {
  if (!acc || N < 1) FAIL(GO2NN_EINVAL, "eval clear: bad argument");
  const long long n = (long long)GO2NN_EVAL_NUM * N;
#ifdef GO2_EMU
  (void)stream;
  for (long long k = 0; k < n; ++k) acc[k] = 0.f;
#else
  hipLaunchKernelGGL(go2nn_eval_clear_kernel, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, acc, n);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_eval_accumulate(const Go2nnEvalIn* in, float* acc, int32_t N, void* stream) {
  if (!in || !acc || N < 1 || !eval_in_ok(in)) FAIL(GO2NN_EINVAL, "eval accumulate: bad argument (every field needs a pointer, an env stride >= 1 and a component stride >= 0)");
#ifdef GO2_EMU
  (void)stream;
  for (int e = 0; e < N; ++e) eval_accumulate_env(*in, acc, N, e);
#else
  hipLaunchKernelGGL(go2nn_eval_accumulate_kernel, dim3((unsigned)((N + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, *in, acc, N);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_eval_reduce(const float* acc, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!acc || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "eval reduce: bad argument (1 <= G <= 65535)");
#ifdef GO2_EMU
  (void)stream;
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < GO2NN_EVAL_NUM + 2; ++c) out[(long long)g * (GO2NN_EVAL_NUM + 2) + c] = eval_group_sum(group, N, g, EvalTerm{acc, N, c});
#else
  hipLaunchKernelGGL(go2nn_eval_reduce_kernel, dim3((unsigned)G, GO2NN_EVAL_NUM + 2), dim3(EVAL_THREADS), 0, (hipStream_t)stream, acc, group, N, out);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_EVAL_H
