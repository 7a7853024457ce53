// go2nn_bootstrap.h — bootstrap replicates of the policy evaluator's reduce table (include/go2nn.h: go2nn_eval_bootstrap*, added within ABI 7;
// go2_rl_gym_amd/utils/evaluator.py, `evaluation.bootstrap`).  Included at the end of go2nn_impl.cpp, after go2nn_eval.h (FAIL is go2nn_impl.cpp's; EvalTerm and the launch
// eval_bootstrap — its rule, its grid and its host loop — are go2nn_eval.h's).
//
// One launch after go2nn_eval_reduce, on the same accumulator table: replicate b of cell g is go2nn_eval_reduce's row of the cell with its robots redrawn with replacement,
// so whatever the evaluator makes of a reduce row (a per-step mean, a fall rate) it can make of B resampled ones, and a quantile of those is the figure's interval.  The
// members of a cell come as a CSR list built once on the host; the launch cannot read it back, so go2nn_eval_bootstrap_check looks at the host copy before the upload.
//
// go2nn_<family>_bootstrap (`evaluation.bootstrap_all`) is the same launch on a scoring family's per-robot table with the family's reduce Term: replicate b of cell g is the
// family's reduce row of the SAME redrawn robots (the draws depend on (b, g, k, seed) only), so a replicate's rows across the tables are one resampled population.  The gait
// table is split into column windows (eval_bootstrap's CHUNK): 55 fp64 sums per lane take 130 VGPRs and a lane walks 55 gathers per draw.  The widths were chosen from the
// code object's resource notes and from timings at 6, 42 and 294 cells (go2nn_eval.h's table, README).
#ifndef GO2NN_BOOTSTRAP_H
#define GO2NN_BOOTSTRAP_H

#define BOOTSTRAP_MAX_REPLICATES (1 << 20)
#ifndef BOOTSTRAP_GAIT_CHUNK
#define BOOTSTRAP_GAIT_CHUNK 11          // 55 columns in 5 windows (a width divides the column count: eval_bootstrap asserts it)
#endif
#ifndef BOOTSTRAP_ASYM_CHUNK
#define BOOTSTRAP_ASYM_CHUNK 25          // one window: AsymTerm's branches on a run-time column cost more than the shorter walk gains (go2nn_eval.h's table)
#endif

// what every bootstrap entry point refuses before it launches (go2nn_eval_bootstrap's rule, with the family's column count); the host build also looks at the list (host
// memory there).  go2nn_eval_bootstrap_check is defined below.
extern "C" int go2nn_eval_bootstrap_check(const int32_t* host_cell_start, const int32_t* host_cell_envs, int32_t N, int32_t G);
static int bootstrap_refuse(const char* what, const void* table, const int32_t* cell_start, const int32_t* cell_envs, const void* out, int N, int G, int B, int cols) {
  if (!table || !cell_start || !cell_envs || !out || N < 1 || G < 1 || G > 65535 || B < 1 || B > BOOTSTRAP_MAX_REPLICATES)
    FAIL(GO2NN_EINVAL, "%s bootstrap: bad argument (pointers, N >= 1, 1 <= G <= 65535, 1 <= B <= 2^20)", what);
  if ((long long)B * G * cols >= (1ll << 31)) FAIL(GO2NN_EINVAL, "%s bootstrap: B G %d = %lld output values, 2^31 or more", what, cols, (long long)B * G * cols);
#ifdef GO2_EMU
  if (go2nn_eval_bootstrap_check(cell_start, cell_envs, N, G) != 0) return GO2NN_EINVAL;
#endif
  return 0;
}

extern "C" {

int go2nn_eval_bootstrap_check(const int32_t* host_cell_start, const int32_t* host_cell_envs, int32_t N, int32_t G) {
  if (!host_cell_start || !host_cell_envs || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "eval bootstrap check: bad argument (pointers, N >= 1, 1 <= G <= 65535)");
  if (host_cell_start[0] != 0) FAIL(GO2NN_EINVAL, "eval bootstrap check: cell_start[0] = %d, the first cell's list starts at 0", (int)host_cell_start[0]);
  for (int g = 0; g < G; ++g)
    if (host_cell_start[g + 1] < host_cell_start[g])
      FAIL(GO2NN_EINVAL, "eval bootstrap check: cell_start[%d] = %d is below cell_start[%d] = %d", g + 1, (int)host_cell_start[g + 1], g, (int)host_cell_start[g]);
  if (host_cell_start[G] > N) FAIL(GO2NN_EINVAL, "eval bootstrap check: cell_start[%d] = %d members, more than the %d envs", (int)G, (int)host_cell_start[G], (int)N);
  for (int i = 0; i < host_cell_start[G]; ++i)
    if (host_cell_envs[i] < 0 || host_cell_envs[i] >= N) FAIL(GO2NN_EINVAL, "eval bootstrap check: cell_envs[%d] = %d is outside [0, %d)", i, (int)host_cell_envs[i], (int)N);
  return 0;
}

int go2nn_eval_bootstrap(const float* acc, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("eval", acc, cell_start, cell_envs, out, N, G, B, GO2NN_EVAL_NUM + 2)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_EVAL_NUM + 2>(EvalTerm{acc, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

int go2nn_robust_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("robust", table, cell_start, cell_envs, out, N, G, B, GO2NN_ROBUST_ACC_NUM + 1)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_ROBUST_ACC_NUM + 1>(RobustTerm{table, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

int go2nn_maneuver_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("maneuver", table, cell_start, cell_envs, out, N, G, B, GO2NN_MANEUVER_ACC_NUM + 1)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_MANEUVER_ACC_NUM + 1>(ManeuverTerm{table, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

int go2nn_ladder_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, float dist2_thr, double* out,
                           void* stream) {
  if (bootstrap_refuse("ladder", table, cell_start, cell_envs, out, N, G, B, GO2NN_LADDER_OUT_NUM)) return GO2NN_EINVAL;
  if (!(dist2_thr > 0.f)) FAIL(GO2NN_EINVAL, "ladder bootstrap: dist2_thr <= 0");
  return eval_bootstrap<GO2NN_LADDER_OUT_NUM>(LadderTerm{table, N, 0, (double)dist2_thr}, cell_start, cell_envs, G, B, seed, out, stream);
}

int go2nn_gait_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("gait", table, cell_start, cell_envs, out, N, G, B, GO2NN_GAIT_OUT_NUM)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_GAIT_OUT_NUM, BOOTSTRAP_GAIT_CHUNK>(GaitTerm{table, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

int go2nn_asym_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("asym", table, cell_start, cell_envs, out, N, G, B, GO2NN_ASYM_OUT_NUM)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_ASYM_OUT_NUM, BOOTSTRAP_ASYM_CHUNK, ASYM_OUT_EQ_MAX>(AsymTerm{table, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);          // EQ_MAX: the max over the drawn members
}

}  // extern "C"

#endif  // GO2NN_BOOTSTRAP_H
