// go2nn_eval.h — the policy evaluator's metric kernels (include/go2nn.h: go2nn_eval_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py) and the launch scaffold that
// every scoring family shares (go2nn_robust.h, go2nn_ladder.h, go2nn_maneuver.h, go2nn_gait.h, go2nn_asym.h).  Included at the end of go2nn_impl.cpp (FAIL, HIPCHK are its helpers).
//
// go2nn_eval_accumulate: one launch per env step, one lane per env.  A lane reads its env's ~75 input values through (env stride, component stride) pairs — with the
// HIP simulator's field-major buffers consecutive lanes read consecutive addresses of every component, i.e. each load instruction of a wave is one dense 256-byte line —
// and read-modify-writes its column of the metric-major accumulator [GO2NN_EVAL_NUM, N] (dense again).  No LDS, no atomics, no cross-lane traffic: a streaming kernel of
// ~0.4 KB per env.  go2nn_eval_reduce: one workgroup per (group, output column): lane t adds the envs t, t + 256, ... of the group in fp64, then a fixed LDS tree over the
// 256 partials — the order is a function of (N, G) only.  The host build runs the same element function and the same summation order in plain loops.
//
// THE SCAFFOLD.  A family writes one element function per env and one Term functor per reduce; the three launch shapes around them live here, once, with their host loops:
//   eval_per_env(f, N)                       grid = ceil(N / 256), lane e calls f(e): eval_per_env_kernel<EvalAccumulate>, <LadderAccumulate>, ... in a kernel trace
//   eval_table_begin(table, rows, N, start)  grid = ceil(rows N / 256), one float per lane: row 0 (a family's STEP row) = start, every other row = 0
//   eval_reduce(term, group, N, G, cols)     grid = (G, cols), workgroup (g, c) writes out[g cols + c] = eval_group_sum of the Term at column c (eval_group_max for MAX_COL)
//   eval_bootstrap<COLS, CHUNK, MAX_COL>(term, cell_start, cell_envs, G, B, seed)   grid = (G, ceil(B / 256), COLS / CHUNK), lane (g, b, z) writes window z of replicate
//                                            b of cell g: the Term's columns summed (MAX_COL: the max) over the cell's members redrawn with replacement
//                                            (go2nn_bootstrap.h instantiates it for every family's Term)
// eval_field_fault is the one statement of what a Go2nnEvalField must satisfy; each family words its own messages around it.
#ifndef GO2NN_EVAL_H
#define GO2NN_EVAL_H

#include "go2_math.h"          // philox4x32_10: eval_bootstrap's draws

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

struct EvalAccumulate {
  Go2nnEvalIn in; float* acc; int N;
  EVAL_MEMBER void operator()(int e) const { eval_accumulate_env(in, acc, N, e); }
};

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

// What is wrong with a field, in the order it is looked at: no pointer, an env stride < 1, a component stride < min_comp (1 for a vector field; 0 for a per-env field, which
// has no second component to step to).
enum { EVAL_FIELD_OK = 0, EVAL_FIELD_NULL, EVAL_FIELD_ENV_STRIDE, EVAL_FIELD_COMP_STRIDE };
static int eval_field_fault(const Go2nnEvalField& f, int min_comp) {
  return !f.p ? EVAL_FIELD_NULL : f.env_stride < 1 ? EVAL_FIELD_ENV_STRIDE : f.comp_stride < min_comp ? EVAL_FIELD_COMP_STRIDE : EVAL_FIELD_OK;
}

// f(e) for every env e < N, one lane per env (host: in env order).  F holds by value what the lane needs — the family's In struct, its pointers, N — and is a named type at
// namespace scope, so that the instantiation has a readable name.
#ifndef GO2_EMU
template <class F> __global__ void __launch_bounds__(EVAL_THREADS) eval_per_env_kernel(const F f, int N) {
  const int e = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (e < N) f(e);
}
#endif
template <class F> static int eval_per_env(const F& f, int N, void* stream) {
#ifdef GO2_EMU
  (void)stream;
  for (int e = 0; e < N; ++e) f(e);
#else
  hipLaunchKernelGGL(eval_per_env_kernel<F>, dim3((unsigned)((N + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, f, N);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

// table [rows, N]: row 0 = start, every other row = 0
#ifndef GO2_EMU
__global__ void __launch_bounds__(EVAL_THREADS) eval_table_begin_kernel(float* table, long long n, int N, float start) {
  const long long k = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (k < n) table[k] = k < N ? start : 0.f;
}
#endif
static int eval_table_begin(float* table, int rows, int N, float start, void* stream) {
  const long long n = (long long)rows * N;
#ifdef GO2_EMU
  (void)stream;
  for (long long k = 0; k < n; ++k) table[k] = k < N ? start : 0.f;
#else
  hipLaunchKernelGGL(eval_table_begin_kernel, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, (hipStream_t)stream, table, n, N, start);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

// The sum of term(e) over the envs e of group g, in an order that depends on N only: partial t adds the envs t, t + 256, ... in fp64, then a fixed tree over the 256
// partials.  Device: called by every thread of a 256-thread workgroup, the sum is valid in thread 0.  Every family's reduce goes through it (eval_reduce below).
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

// The largest term(e) over the envs e of group g (0 for an empty group: the terms are >= 0), eval_group_sum's scheme with max in place of +: any order gives the same bits.
#ifdef GO2_EMU
template <class Term> static inline double eval_group_max(const int32_t* group, int N, int g, Term term) {
  double m = 0.0;
  for (int e = 0; e < N; ++e)
    if (group[e] == g) m = fmax(m, term(e));
  return m;
}
#else
template <class Term> __device__ __forceinline__ double eval_group_max(const int32_t* group, int N, int g, Term term) {
  __shared__ double part[EVAL_THREADS];
  const int t = threadIdx.x;
  double m = 0.0;
  for (int e = t; e < N; e += EVAL_THREADS)
    if (group[e] == g) m = fmax(m, term(e));
  part[t] = m;
  __syncthreads();
  for (int w = EVAL_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) part[t] = fmax(part[t], part[t + w]);
    __syncthreads();
  }
  return part[0];
}
#endif

// out[g * cols + c] for every group g < G and column c < cols: the group's sum of the Term at column c (a Term has a member `c`, set here), or its max where c == MAX_COL.
// MAX_COL = -1 (no such column) instantiates no max tree, so no second LDS array; with one, the branch is uniform over the workgroup.
template <int MAX_COL, class Term> EVAL_FN double eval_group_value(const int32_t* group, int N, int g, const Term& term) {
  if constexpr (MAX_COL >= 0)
    if (term.c == MAX_COL) return eval_group_max(group, N, g, term);
  return eval_group_sum(group, N, g, term);
}
#ifndef GO2_EMU
template <int MAX_COL, class Term> __global__ void __launch_bounds__(EVAL_THREADS) eval_reduce_kernel(Term term, const int32_t* group, int N, int cols, double* out) {
  const int g = blockIdx.x;
  term.c = blockIdx.y;
  const double s = eval_group_value<MAX_COL>(group, N, g, term);
  if (threadIdx.x == 0) out[(long long)g * cols + term.c] = s;
}
#endif
template <int MAX_COL = -1, class Term> static int eval_reduce(Term term, const int32_t* group, int N, int G, int cols, double* out, void* stream) {
#ifdef GO2_EMU
  (void)stream;
  for (int g = 0; g < G; ++g)
    for (term.c = 0; term.c < cols; ++term.c) out[(long long)g * cols + term.c] = eval_group_value<MAX_COL>(group, N, g, term);
#else
  hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_reduce_kernel<MAX_COL, Term>), dim3((unsigned)G, (unsigned)cols), dim3(EVAL_THREADS), 0, (hipStream_t)stream, term, group, N, cols, out);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

// out[(b G + g) COLS + c] for every replicate b < B, cell g < G and column c < COLS: the sum of the Term at column c over n = cell_start[g + 1] - cell_start[g] members of the
// cell drawn WITH replacement (a stratified bootstrap: every cell keeps its size), in fp64 in the order of the draws; at c == MAX_COL (eval_reduce's: -1 = no such column) the
// largest of the drawn members' terms instead (0 for an empty cell: the terms are >= 0).  Draw k of (b, g) is member (x n) >> 32 of the cell's list
// cell_envs[cell_start[g] ...], x = word (k & 3) of philox4x32_10(b, g, k >> 2, 0, seed, EVAL_TAG_BOOTSTRAP): integers only, so the host loops, the lanes and a restatement in
// Python integers pick the same members, and a replicate depends on (b, g, seed) but not on B, COLS or the Term: replicate (b, g) of EVERY family's table redraws the same robots.
// grid = (G, ceil(B / 256), COLS / CHUNK), lane (g, b, z) walks its cell's draws — one Philox block per four, the words picked by the unrolled loop's constant index, never
// by a dynamic one (that array would live in scratch) — and keeps the sums of ITS column window [z CHUNK, z CHUNK + CHUNK) in registers, which is why COLS and CHUNK are template
// arguments and not ones of the call; every z-slice recomputes the same draws.  No LDS, no atomics.  n is uniform over a workgroup; the member loads are gathers from a table
// that fits the caches.  CHUNK == COLS (EvalTerm's twelve columns) is one window with constant column indices: the code and the bits of the launch before it had a window.
//
// THE WINDOW'S WIDTH.  Read from the gfx950 code object's notes (build.py kernel_resources; scratch 0 and LDS 0 in every row) and timed on an MI355X: device events around
// 200 back-to-back launches, 1024 robots, B = 1000, at 6 / 42 / 294 cells (profiles/bootstrap_all_bench.json):
//   Term, COLS      CHUNK  windows  VGPRs  SGPRs   us per launch at 6 / 42 / 294 cells
//   EvalTerm 12        12        1     64     41   131 /  22 /  17     (64 / 41 before the launch had a window: the same code)
//   RobustTerm 7        7        1     32     38    70 /  13 /  13
//   ManeuverTerm 9      9        1     36     38    94 /  16 /  16
//   LadderTerm 6        6        1     40     46    68 /  12 /  10
//   GaitTerm 55        55        1    130     45   934 / 143 /  94
//   GaitTerm 55        28        2     74    106   561 /  92 /  87
//   GaitTerm 55        19        3     56     91   401 /  67 /  77
//   GaitTerm 55        11        5     56     69   132 /  74 /  68     kept: a lane's serial walk is what a launch at few cells waits for, and five windows cut it to a fifth
//   AsymTerm 25        25        1    108     38   180 /  35 /  33     kept
//   AsymTerm 25        13        2     81    106   573 /  89 /  48
//   AsymTerm 25         9        3     73    106   380 /  63 /  44
//   AsymTerm 25         5        5     57    106   176 /  46 /  42
// (The widths 28, 19, 13 and 9 do not divide their column counts; they were timed with a guarded, narrower last window, a path the launch no longer has: CHUNK divides COLS.)
// A window makes the column a run-time value: GaitTerm only turns it into a row index, AsymTerm branches on it into two fp64 divisions per imbalance column, which every
// lane of a windowed launch then pays for on every column — so the 25 columns stay in one window (108 VGPRs, still 4 waves per SIMD) and the 55 are split.
#define EVAL_TAG_BOOTSTRAP 7u          // the key's second word; 1 .. 6 are the sensor kernels' (go2nn_sensor.h, go2nn_sensor_rand.h)
template <int COLS, int CHUNK, int MAX_COL, class Term>
EVAL_FN void eval_bootstrap_replicate(Term term, const int32_t* cell_start, const int32_t* cell_envs, int G, int g, int b, int z, uint32_t seed, double* out) {
  static_assert(CHUNK >= 1 && COLS % CHUNK == 0, "the windows are equally wide: CHUNK divides COLS");
  const int s0 = cell_start[g], n = cell_start[g + 1] - s0;
  const int c0 = CHUNK == COLS ? 0 : z * CHUNK;          // (one window: the column indices below are constants)
  double sum[CHUNK];
#pragma unroll
  for (int j = 0; j < CHUNK; ++j) sum[j] = 0.0;
  for (int k0 = 0; k0 < n; k0 += 4) {
    uint32_t w[4];
    philox4x32_10((uint32_t)b, (uint32_t)g, (uint32_t)(k0 >> 2), 0u, seed, EVAL_TAG_BOOTSTRAP, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (k0 + q < n) {
        const int e = cell_envs[s0 + (int)(((uint64_t)w[q] * (uint64_t)(uint32_t)n) >> 32)];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
          term.c = c0 + j;
          const double v = term(e);
          if (MAX_COL >= 0 && term.c == MAX_COL) sum[j] = fmax(sum[j], v);
          else sum[j] += v;
        }
      }
    }
  }
  double* row = out + ((long long)b * G + g) * COLS;
#pragma unroll
  for (int j = 0; j < CHUNK; ++j) row[c0 + j] = sum[j];
}
#ifndef GO2_EMU
template <int COLS, int CHUNK, int MAX_COL, class Term>
__global__ void __launch_bounds__(EVAL_THREADS) eval_bootstrap_kernel(const Term term, const int32_t* cell_start, const int32_t* cell_envs, int G, int B, uint32_t seed, double* out) {
  const int b = blockIdx.y * EVAL_THREADS + threadIdx.x;
  if (b < B) eval_bootstrap_replicate<COLS, CHUNK, MAX_COL>(term, cell_start, cell_envs, G, (int)blockIdx.x, b, (int)blockIdx.z, seed, out);
}
#endif
template <int COLS, int CHUNK = COLS, int MAX_COL = -1, class Term>
static int eval_bootstrap(const Term& term, const int32_t* cell_start, const int32_t* cell_envs, int G, int B, uint32_t seed, double* out, void* stream) {
  constexpr int Z = COLS / CHUNK;
#ifdef GO2_EMU
  (void)stream;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g)
      for (int z = 0; z < Z; ++z) eval_bootstrap_replicate<COLS, CHUNK, MAX_COL>(term, cell_start, cell_envs, G, g, b, z, seed, out);
#else
  hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_bootstrap_kernel<COLS, CHUNK, MAX_COL, Term>), dim3((unsigned)G, (unsigned)((B + EVAL_THREADS - 1) / EVAL_THREADS), (unsigned)Z), dim3(EVAL_THREADS), 0,
                     (hipStream_t)stream, term, cell_start, cell_envs, G, B, seed, out);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

static int eval_in_ok(const Go2nnEvalIn* in) {
  const Go2nnEvalField* f[] = {&in->commands, &in->base_lin_vel, &in->base_ang_vel, &in->projected_gravity, &in->dof_state, &in->torques, &in->actions, &in->last_actions,
                               &in->reset_buf, &in->time_out_buf};
  for (const Go2nnEvalField* x : f)
    if (eval_field_fault(*x, 0)) return 0;
  return in->dof_limits != nullptr && in->dof_vel_offset >= 1;
}

extern "C" {

int go2nn_eval_clear(float* acc, int32_t N, void* stream) {
  if (!acc || N < 1) FAIL(GO2NN_EINVAL, "eval clear: bad argument");
  return eval_table_begin(acc, GO2NN_EVAL_NUM, N, 0.f, stream);
}

int go2nn_eval_accumulate(const Go2nnEvalIn* in, float* acc, int32_t N, void* stream) {
  if (!in || !acc || N < 1 || !eval_in_ok(in)) FAIL(GO2NN_EINVAL, "eval accumulate: bad argument (every field needs a pointer, an env stride >= 1 and a component stride >= 0)");
  return eval_per_env(EvalAccumulate{*in, acc, N}, N, stream);
}

int go2nn_eval_reduce(const float* acc, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!acc || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "eval reduce: bad argument (1 <= G <= 65535)");
  return eval_reduce(EvalTerm{acc, N, 0}, group, N, G, GO2NN_EVAL_NUM + 2, out, stream);
}

}  // extern "C"

#endif  // GO2NN_EVAL_H
