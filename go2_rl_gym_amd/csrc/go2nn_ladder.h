// go2nn_ladder.h — the evaluator's terrain-difficulty ladder (include/go2nn.h: go2nn_ladder_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp after go2nn_robust.h (FAIL, HIPCHK are the former's helpers; EVAL_FN, eval_f, eval_b, eval_group_sum go2nn_eval.h's).
//
// One launch per env step, one lane per env, no LDS, no atomics, no cross-lane traffic.  go2nn_ladder_accumulate (after the step) reads two root-state floats and two flags
// and read-modify-writes the env's column of the table [GO2NN_LADDER_NUM, N]: with the HIP simulator's field-major buffers (env stride 1) consecutive lanes touch consecutive
// addresses of every component and of every table row, i.e. each load / store instruction of a wave is one dense 256-byte line.  8 B + 2 B read and 24 B read-modify-written
// per env: launch-bound at evaluation sizes (1024 lanes = 16 waves).  Distances are compared squared: there is no sqrt in the per-step kernel (the reduce takes one per env,
// in fp64).  The step counter is the table's STEP row, advanced by the kernel itself: no host argument changes between steps, so a captured launch advances on every replay.
// The host build runs the same element functions in plain loops.
#ifndef GO2NN_LADDER_H
#define GO2NN_LADDER_H

EVAL_FN void ladder_accumulate_env(const Go2nnLadderIn& in, float* table, int N, int e) {
  float* col = table + e;
#define ROW(r) col[(long long)GO2NN_LADDER_##r * N]
  const float s = ROW(STEP);
  if (s >= 0.f) {
    const float x = eval_f(in.root_states, e, 0), y = eval_f(in.root_states, e, 1);
    if (s == 0.f) {          // the first counted step: where the robot stands now is where its distance is measured from
      ROW(X0) = x;
      ROW(Y0) = y;
      ROW(MAX_D2) = 0.f;
      ROW(STATE) = (float)GO2NN_LADDER_RUNNING;
    }
    if (ROW(STATE) == (float)GO2NN_LADDER_RUNNING) {
      if (eval_b(in.reset_buf, e) != 0) {          // the root state is already the post-reset pose: the flags come BEFORE the position
        ROW(STATE) = eval_b(in.time_out_buf, e) != 0 ? (float)GO2NN_LADDER_TIMED_OUT : (float)GO2NN_LADDER_FELL;
      } else {
        const float dx = x - ROW(X0), dy = y - ROW(Y0);
        const float d2 = dx * dx + dy * dy;
        ROW(MAX_D2) = fmaxf(ROW(MAX_D2), d2);
        if (d2 > in.dist2_thr) {
          ROW(STATE) = (float)GO2NN_LADDER_CLEARED;
          ROW(CLEAR_STEP) = s + 1.f;
        }
      }
    }
  }
  ROW(STEP) = s + 1.f;
#undef ROW
}

// column c of go2nn_ladder_reduce's output for env e: 1 (the group's size), the three latched states, CLEAR_STEP of a cleared env, the progress
struct LadderTerm {
  const float* table; int N, c; double dist2_thr;
  EVAL_MEMBER double operator()(int e) const {
    if (c == GO2NN_LADDER_OUT_N) return 1.0;
    const float state = table[(long long)GO2NN_LADDER_STATE * N + e];
    if (c == GO2NN_LADDER_OUT_CLEARED) return state == (float)GO2NN_LADDER_CLEARED ? 1.0 : 0.0;
    if (c == GO2NN_LADDER_OUT_FELL) return state == (float)GO2NN_LADDER_FELL ? 1.0 : 0.0;
    if (c == GO2NN_LADDER_OUT_TIMED_OUT) return state == (float)GO2NN_LADDER_TIMED_OUT ? 1.0 : 0.0;
    if (c == GO2NN_LADDER_OUT_CLEAR_STEPS) return state == (float)GO2NN_LADDER_CLEARED ? (double)table[(long long)GO2NN_LADDER_CLEAR_STEP * N + e] : 0.0;
    const double p = sqrt((double)table[(long long)GO2NN_LADDER_MAX_D2 * N + e] / dist2_thr);
    return p < 1.0 ? p : 1.0;
  }
};

#ifndef GO2_EMU
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_ladder_begin_kernel(float* table, int N, float start) {
  const long long k = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  static_assert(GO2NN_LADDER_STEP == 0, "the STEP row is the table's first N floats");
  if (k < (long long)GO2NN_LADDER_NUM * N) table[k] = k < N ? start : 0.f;
}
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_ladder_accumulate_kernel(const Go2nnLadderIn in, float* table, int N) {
  const int e = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (e < N) ladder_accumulate_env(in, table, N, e);
}
// grid = (G, GO2NN_LADDER_OUT_NUM)
__global__ void __launch_bounds__(EVAL_THREADS) go2nn_ladder_reduce_kernel(const float* table, const int32_t* group, int N, double dist2_thr, double* out) {
  const int g = blockIdx.x, c = blockIdx.y;
  const double s = eval_group_sum(group, N, g, LadderTerm{table, N, c, dist2_thr});
  if (threadIdx.x == 0) out[(long long)g * GO2NN_LADDER_OUT_NUM + c] = s;
}
#endif

static const char* ladder_in_bad(const Go2nnLadderIn* in) {
  if (!in->root_states.p || !in->reset_buf.p || !in->time_out_buf.p) return "a null buffer pointer";
  if (in->root_states.env_stride < 1 || in->root_states.comp_stride < 1) return "root_states with an env stride or a component stride < 1";
  if (in->reset_buf.env_stride < 1 || in->time_out_buf.env_stride < 1 || in->reset_buf.comp_stride < 0 || in->time_out_buf.comp_stride < 0) return "a flag field with an env stride < 1";
  if (!(in->dist2_thr > 0.f)) return "dist2_thr <= 0";
  return nullptr;
}

extern "C" {

int go2nn_ladder_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "ladder begin: bad argument (a table and N >= 1)");
  const long long n = (long long)GO2NN_LADDER_NUM * N;
#ifdef GO2_EMU
  (void)stream;
  for (long long k = 0; k < n; ++k) table[k] = 0.f;
  for (int e = 0; e < N; ++e) table[(long long)GO2NN_LADDER_STEP * N + e] = (float)start;
#else
  hipLaunchKernelGGL(go2nn_ladder_begin_kernel, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, table, N, (float)start);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_ladder_accumulate(const Go2nnLadderIn* in, float* table, int32_t N, void* stream) {
  if (!in || !table || N < 1) FAIL(GO2NN_EINVAL, "ladder accumulate: null argument or N < 1");
  if (const char* bad = ladder_in_bad(in)) FAIL(GO2NN_EINVAL, "ladder accumulate: %s", bad);
#ifdef GO2_EMU
  (void)stream;
  for (int e = 0; e < N; ++e) ladder_accumulate_env(*in, table, N, e);
#else
  hipLaunchKernelGGL(go2nn_ladder_accumulate_kernel, dim3((unsigned)((N + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, *in, table, N);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_ladder_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, float dist2_thr, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "ladder reduce: bad argument (1 <= G <= 65535)");
  if (!(dist2_thr > 0.f)) FAIL(GO2NN_EINVAL, "ladder reduce: dist2_thr <= 0");
#ifdef GO2_EMU
  (void)stream;
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < GO2NN_LADDER_OUT_NUM; ++c) out[(long long)g * GO2NN_LADDER_OUT_NUM + c] = eval_group_sum(group, N, g, LadderTerm{table, N, c, (double)dist2_thr});
#else
  hipLaunchKernelGGL(go2nn_ladder_reduce_kernel, dim3((unsigned)G, GO2NN_LADDER_OUT_NUM), dim3(EVAL_THREADS), 0, (hipStream_t)stream, table, group, N, (double)dist2_thr, out);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_LADDER_H
