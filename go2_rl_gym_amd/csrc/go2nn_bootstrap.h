// go2nn_bootstrap.h — bootstrap replicates of the policy evaluator's reduce table (include/go2nn.h: go2nn_eval_bootstrap*, added within ABI 7;
// go2_rl_gym_amd/utils/evaluator.py, `evaluation.bootstrap`).  Included at the end of go2nn_impl.cpp, after go2nn_eval.h (FAIL is go2nn_impl.cpp's; EvalTerm and the launch
// eval_bootstrap — its rule, its grid and its host loop — are go2nn_eval.h's).
//
// One launch after go2nn_eval_reduce, on the same accumulator table: replicate b of cell g is go2nn_eval_reduce's row of the cell with its robots redrawn with replacement,
// so whatever the evaluator makes of a reduce row (a per-step mean, a fall rate) it can make of B resampled ones, and a quantile of those is the figure's interval.  The
// members of a cell come as a CSR list built once on the host; the launch cannot read it back, so go2nn_eval_bootstrap_check looks at the host copy before the upload.
#ifndef GO2NN_BOOTSTRAP_H
#define GO2NN_BOOTSTRAP_H

#define BOOTSTRAP_MAX_REPLICATES (1 << 20)

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
  if (!acc || !cell_start || !cell_envs || !out || N < 1 || G < 1 || G > 65535 || B < 1 || B > BOOTSTRAP_MAX_REPLICATES)
    FAIL(GO2NN_EINVAL, "eval bootstrap: bad argument (pointers, N >= 1, 1 <= G <= 65535, 1 <= B <= 2^20)");
  if ((long long)B * G * (GO2NN_EVAL_NUM + 2) >= (1ll << 31)) FAIL(GO2NN_EINVAL, "eval bootstrap: B G %d = %lld output values, 2^31 or more", GO2NN_EVAL_NUM + 2, (long long)B * G * (GO2NN_EVAL_NUM + 2));
#ifdef GO2_EMU
  if (go2nn_eval_bootstrap_check(cell_start, cell_envs, N, G) != 0) return GO2NN_EINVAL;          // (host memory: the list can be looked at here too)
#endif
  return eval_bootstrap<GO2NN_EVAL_NUM + 2>(EvalTerm{acc, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

}  // extern "C"

#endif  // GO2NN_BOOTSTRAP_H
