// go2nn_ladder.h — the evaluator's terrain-difficulty ladder (include/go2nn.h: go2nn_ladder_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp after go2nn_robust.h (FAIL is the former's helper; EVAL_FN, EVAL_MEMBER, eval_f, eval_b, eval_field_fault and the launch scaffold —
// eval_table_begin, eval_per_env, eval_reduce over eval_group_sum — go2nn_eval.h's).
//
// One launch per env step (eval_per_env_kernel<LadderAccumulate>), one lane per env, no LDS, no atomics, no cross-lane traffic.  go2nn_ladder_accumulate (after the step) reads two root-state floats and two flags
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

struct LadderAccumulate {
  Go2nnLadderIn in; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { ladder_accumulate_env(in, table, N, e); }
};

static const char* ladder_in_bad(const Go2nnLadderIn* in) {
  const int root = eval_field_fault(in->root_states, 1), reset = eval_field_fault(in->reset_buf, 0), tout = eval_field_fault(in->time_out_buf, 0);
  if (root == EVAL_FIELD_NULL || reset == EVAL_FIELD_NULL || tout == EVAL_FIELD_NULL) return "a null buffer pointer";
  if (root) return "root_states with an env stride or a component stride < 1";
  if (reset || tout) return "a flag field with an env stride < 1";
  if (!(in->dist2_thr > 0.f)) return "dist2_thr <= 0";
  return nullptr;
}

extern "C" {

int go2nn_ladder_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "ladder begin: bad argument (a table and N >= 1)");
  static_assert(GO2NN_LADDER_STEP == 0, "the STEP row is the table's first N floats");
  return eval_table_begin(table, GO2NN_LADDER_NUM, N, (float)start, stream);
}

int go2nn_ladder_accumulate(const Go2nnLadderIn* in, float* table, int32_t N, void* stream) {
  if (!in || !table || N < 1) FAIL(GO2NN_EINVAL, "ladder accumulate: null argument or N < 1");
  if (const char* bad = ladder_in_bad(in)) FAIL(GO2NN_EINVAL, "ladder accumulate: %s", bad);
  return eval_per_env(LadderAccumulate{*in, table, N}, N, stream);
}

int go2nn_ladder_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, float dist2_thr, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "ladder reduce: bad argument (1 <= G <= 65535)");
  if (!(dist2_thr > 0.f)) FAIL(GO2NN_EINVAL, "ladder reduce: dist2_thr <= 0");
  return eval_reduce(LadderTerm{table, N, 0, (double)dist2_thr}, group, N, G, GO2NN_LADDER_OUT_NUM, out, stream);
}

}  // extern "C"

#endif  // GO2NN_LADDER_H
