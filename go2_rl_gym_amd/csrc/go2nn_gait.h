// go2nn_gait.h — the evaluator's gait scores (include/go2nn.h: go2nn_gait_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py, `evaluation.gait`).
// Included at the end of go2nn_impl.cpp after go2nn_trace.h (FAIL is the former's helper; EVAL_FN, EVAL_MEMBER, eval_b, eval_field_fault and the launch scaffold —
// eval_table_begin, eval_per_env, eval_reduce over eval_group_sum — go2nn_eval.h's).
//
// One launch per env step (eval_per_env_kernel<GaitAccumulate>), one lane per env, the four feet unrolled inside the lane; no LDS, no atomics, no cross-lane traffic.  go2nn_gait_accumulate (after the step) reads
// per foot four floats (force z; world z, vx, vy of the foot body) and one flag, and read-modify-writes the env's column of the table [GO2NN_GAIT_NUM, N]: with the HIP
// simulator's field-major buffers (env stride 1) consecutive lanes touch consecutive addresses of every component and of every table row, i.e. each load / store instruction
// of a wave is one dense 256-byte line, like ladder_accumulate_env.  Most rows move only on a touchdown or a lift-off; a plain frame touches the foot's PREV and one of
// LIFT_Z / SWING_MAX, CONTACT and SLIP_SUM, and three per-env rows: launch-bound at evaluation sizes (1024 lanes = 16 waves).  The step counter is the table's STEP row,
// advanced by the kernel itself: no host argument changes between steps, so a captured launch advances on every replay.  The host build runs the same element functions in
// plain loops.
//
// The per-foot rule, restated once (utils/recorder.py gait_summary is the same rule on a recorded trace; keep the two in step): a foot is in contact on a frame when its
// vertical contact force is > contact_threshold, strictly.  A frame with reset_buf set is not used and ends the SEGMENT: previous contact state, phase start, last touchdown
// and running swing maximum start afresh after it, as they do at the first counted step.  Inside a segment: `used` and `contact` count frames; slip_sum adds the horizontal
// speed of the foot body over contact frames; a touchdown is a swing -> contact transition (a contact run that opens a segment is not one); strides are the step differences
// between consecutive touchdowns; a stance or a swing counts only when both of its ends were seen; height_sum adds each complete swing's largest world z, clearance_sum that
// maximum minus the foot's world z on the last contact frame before the swing.
#ifndef GO2NN_GAIT_H
#define GO2NN_GAIT_H

#define GAIT_NONE 0.f
#define GAIT_SWING 1.f
#define GAIT_CONTACT 2.f

EVAL_FN void gait_accumulate_env(const Go2nnGaitIn& in, float* table, int N, int e) {
  float* col = table + e;
#define ROW(r) col[(long long)(r) * N]
  const float s = ROW(GO2NN_GAIT_STEP);
  ROW(GO2NN_GAIT_STEP) = s + 1.f;
  if (s < 0.f) return;
  const bool reset = eval_b(in.reset_buf, e) != 0;
  const float now = s + 1.f;          // phase starts and touchdowns are kept as step + 1: 0 is "none"
  int mask = 0, feet = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#define FROW(r) ROW(GO2NN_GAIT_FOOT0 + f * GO2NN_GAIT_FOOT_ROWS + GO2NN_GAIT_F_##r)
    if (reset) {          // the frame shows the post-reset pose: not used, and nothing is followed across it
      FROW(PREV) = GAIT_NONE;
      FROW(PHASE_START) = 0.f;
      FROW(LAST_TD) = 0.f;
      continue;
    }
    const Go2nnEvalField &rb = in.rigid_body_states, &cf = in.contact_forces;
    const float* body = (const float*)rb.p + (long long)e * rb.env_stride + (long long)in.foot_body[f] * in.rigid_body_stride;
    const float fz = ((const float*)cf.p)[(long long)e * cf.env_stride + (long long)in.foot_body[f] * in.contact_body_stride + 2LL * cf.comp_stride];
    const float z = body[2LL * rb.comp_stride];
    const bool contact = fz > in.contact_threshold;
    const float prev = FROW(PREV);
    if (contact) {
      const float vx = body[7LL * rb.comp_stride], vy = body[8LL * rb.comp_stride];
      FROW(CONTACT) += 1.f;
      FROW(SLIP_SUM) += sqrtf(vx * vx + vy * vy);
      mask |= 1 << f;
      ++feet;
    }
    if (prev == GAIT_NONE) {
      FROW(PHASE_START) = 0.f;
      if (contact) FROW(LIFT_Z) = z; else FROW(SWING_MAX) = z;
    } else if (contact && prev == GAIT_SWING) {          // touchdown
      FROW(TOUCHDOWNS) += 1.f;
      const float last = FROW(LAST_TD), start = FROW(PHASE_START);
      if (last > 0.f) {
        FROW(STRIDE_STEPS) += now - last;
        FROW(STRIDES) += 1.f;
      }
      if (start > 0.f) {
        const float top = FROW(SWING_MAX);
        FROW(SWING_STEPS) += now - start;
        FROW(SWINGS) += 1.f;
        FROW(HEIGHT_SUM) += top;
        FROW(CLEARANCE_SUM) += top - FROW(LIFT_Z);
      }
      FROW(LAST_TD) = now;
      FROW(PHASE_START) = now;
      FROW(LIFT_Z) = z;
    } else if (!contact && prev == GAIT_CONTACT) {       // lift-off
      const float start = FROW(PHASE_START);
      if (start > 0.f) {
        FROW(STANCE_STEPS) += now - start;
        FROW(STANCES) += 1.f;
      }
      FROW(PHASE_START) = now;
      FROW(SWING_MAX) = z;
    } else if (contact) {
      FROW(LIFT_Z) = z;
    } else {
      FROW(SWING_MAX) = fmaxf(FROW(SWING_MAX), z);
    }
    FROW(PREV) = contact ? GAIT_CONTACT : GAIT_SWING;
#undef FROW
  }
  if (reset) return;
  ROW(GO2NN_GAIT_USED) += 1.f;
  ROW(GO2NN_GAIT_SUPPORT0 + feet) += 1.f;
  if (mask == in.diagonal_mask[0] || mask == in.diagonal_mask[1]) ROW(GO2NN_GAIT_DIAGONAL) += 1.f;
#undef ROW
}

// column c of go2nn_gait_reduce's output for env e: 1 (the group's size), the foot columns (USED is the env's row, repeated per foot), SUPPORT0 .. 4, DIAGONAL
struct GaitTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const {
    if (c == GO2NN_GAIT_OUT_N) return 1.0;
    int row;
    if (c >= GO2NN_GAIT_OUT_SUPPORT0) {
      row = GO2NN_GAIT_SUPPORT0 + (c - GO2NN_GAIT_OUT_SUPPORT0);          // (DIAGONAL follows SUPPORT4 in both enums)
    } else {
      const int f = (c - GO2NN_GAIT_OUT_FOOT0) / GO2NN_GAIT_OUT_FOOT_COLS, k = (c - GO2NN_GAIT_OUT_FOOT0) % GO2NN_GAIT_OUT_FOOT_COLS;
      row = k == GO2NN_GAIT_O_USED ? GO2NN_GAIT_USED : GO2NN_GAIT_FOOT0 + f * GO2NN_GAIT_FOOT_ROWS + GO2NN_GAIT_F_ACC_FIRST + (k - 1);
    }
    return (double)table[(long long)row * N + e];
  }
};
static_assert(GO2NN_GAIT_DIAGONAL == GO2NN_GAIT_SUPPORT0 + 5 && GO2NN_GAIT_OUT_DIAGONAL == GO2NN_GAIT_OUT_SUPPORT0 + 5, "DIAGONAL follows SUPPORT4 in the table and in the output");
static_assert(GO2NN_GAIT_FOOT_ROWS - GO2NN_GAIT_F_ACC_FIRST == GO2NN_GAIT_OUT_FOOT_COLS - 1, "the foot's accumulator rows are the output's foot columns after USED, in order");

struct GaitAccumulate {
  Go2nnGaitIn in; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { gait_accumulate_env(in, table, N, e); }
};

static const char* gait_in_bad(const Go2nnGaitIn* in) {
  const int rb = eval_field_fault(in->rigid_body_states, 1), cf = eval_field_fault(in->contact_forces, 1), reset = eval_field_fault(in->reset_buf, 0);
  if (rb == EVAL_FIELD_NULL || cf == EVAL_FIELD_NULL || reset == EVAL_FIELD_NULL) return "a null buffer pointer";
  if (rb == EVAL_FIELD_ENV_STRIDE || cf == EVAL_FIELD_ENV_STRIDE || reset == EVAL_FIELD_ENV_STRIDE) return "a field with an env stride < 1";
  if (rb || cf || reset) return "a vector field with a component stride < 1";
  if (in->rigid_body_stride < 1 || in->contact_body_stride < 1) return "a body stride < 1";
  for (int f = 0; f < 4; ++f)
    if (in->foot_body[f] < 0) return "foot_body < 0";
  if (!(in->contact_threshold >= 0.f) || !(in->contact_threshold <= 3.0e38f)) return "contact_threshold negative or not finite";
  const int a = in->diagonal_mask[0], b = in->diagonal_mask[1];
  if (a < 0 || b < 0 || (a | b) != 15 || (a & b) != 0 || __builtin_popcount(a) != 2) return "diagonal_mask: two disjoint pairs of the four feet (bit f = foot f of foot_body)";
  return nullptr;
}

extern "C" {

int go2nn_gait_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "gait begin: bad argument (a table and N >= 1)");
  static_assert(GO2NN_GAIT_STEP == 0, "the STEP row is the table's first N floats");
  return eval_table_begin(table, GO2NN_GAIT_NUM, N, (float)start, stream);
}

int go2nn_gait_accumulate(const Go2nnGaitIn* in, float* table, int32_t N, void* stream) {
  if (!in || !table || N < 1) FAIL(GO2NN_EINVAL, "gait accumulate: null argument or N < 1");
  if (const char* bad = gait_in_bad(in)) FAIL(GO2NN_EINVAL, "gait accumulate: %s", bad);
  return eval_per_env(GaitAccumulate{*in, table, N}, N, stream);
}

int go2nn_gait_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "gait reduce: bad argument (1 <= G <= 65535)");
  return eval_reduce(GaitTerm{table, N, 0}, group, N, G, GO2NN_GAIT_OUT_NUM, out, stream);
}

}  // extern "C"

#endif  // GO2NN_GAIT_H
