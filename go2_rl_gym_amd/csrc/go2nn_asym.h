// go2nn_asym.h — the evaluator's left-right asymmetry scores (include/go2nn.h: go2nn_asym_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py, `evaluation.asymmetry`).
// Included at the end of go2nn_impl.cpp after go2nn_gait.h (FAIL is the former's helper; EVAL_FN, EVAL_MEMBER, eval_f, eval_b, eval_field_fault and the launch scaffold —
// eval_table_begin, eval_per_env, eval_reduce over eval_group_sum and, for the EQ_MAX column, eval_group_max — go2nn_eval.h's).
//
// One launch per env step (eval_per_env_kernel<AsymAccumulate>), one lane per env, the twelve joints and the four feet unrolled inside the lane; no LDS, no atomics, no cross-lane traffic.  go2nn_asym_accumulate
// (after the step) reads per env the action and the action of the mirrored observation (2 x 12 floats, row-major: a lane's 48 bytes are three 16-byte pieces of lines its
// neighbours share), three command components, twelve torques and joint velocities, four vertical contact forces and one flag, and read-modify-writes the env's column of
// the table [GO2NN_ASYM_NUM, N]: with the HIP simulator's field-major buffers (env stride 1) consecutive lanes touch consecutive addresses of every component and of every
// table row, like gait_accumulate_env.  ~0.3 KB per env: launch-bound at evaluation sizes (1024 lanes = 16 waves).  The mirror table of the action (twelve entries) comes by
// value in the struct; the sums over a kind or a side add `cond ? x : 0.f` (exact) instead of indexing a local array, so nothing lives in scratch.  The step counter is the
// table's STEP row, advanced by the kernel itself: no host argument changes between steps, so a captured launch advances on every replay.  The host build runs the same
// element functions in plain loops.
#ifndef GO2NN_ASYM_H
#define GO2NN_ASYM_H

EVAL_FN void asym_accumulate_env(const Go2nnAsymIn& in, const float* actions, const float* mirrored, float* table, int N, int e) {
  float* col = table + e;
#define ROW(r) col[(long long)(r) * N]
  const float s = ROW(GO2NN_ASYM_STEP);
  ROW(GO2NN_ASYM_STEP) = s + 1.f;
  if (s < 0.f) return;
  const float *a = actions + (long long)e * 12, *am = mirrored + (long long)e * 12;
  const bool sym = eval_b(in.reset_buf, e) == 0 && eval_f(in.commands, e, 1) == 0.f && eval_f(in.commands, e, 2) == 0.f;
  float sq = 0.f, hip = 0.f, thigh = 0.f, calf = 0.f, asq = 0.f, emax = 0.f;
  float al = 0.f, ar = 0.f, tl = 0.f, tr = 0.f, pl = 0.f, pr = 0.f;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const float aj = a[j];
    const float ej = aj - in.action_sign[j] * am[in.action_perm[j]];          // (the product by +-1 is exact: one rounding, contracted or not)
    const float e2 = ej * ej, a2 = aj * aj;
    const int kind = in.joint_kind[j];
    sq += e2;
    hip += kind == 0 ? e2 : 0.f;
    thigh += kind == 1 ? e2 : 0.f;
    calf += kind == 2 ? e2 : 0.f;
    asq += a2;
    emax = fmaxf(emax, fabsf(ej));
    if (sym) {
      const long long q_at = (long long)e * in.dof_state.env_stride + (long long)j * in.dof_state.comp_stride;
      const float qd = ((const float*)in.dof_state.p)[q_at + in.dof_vel_offset];
      const float tau = eval_f(in.torques, e, j);
      const float t2 = tau * tau, pw = fabsf(tau * qd);
      const bool left = in.joint_side[j] > 0;
      al += left ? a2 : 0.f;  ar += left ? 0.f : a2;
      tl += left ? t2 : 0.f;  tr += left ? 0.f : t2;
      pl += left ? pw : 0.f;  pr += left ? 0.f : pw;
    }
  }
  ROW(GO2NN_ASYM_EQ_STEPS) += 1.f;
  ROW(GO2NN_ASYM_EQ_SQ) += sq;
  ROW(GO2NN_ASYM_EQ_SQ_HIP) += hip;
  ROW(GO2NN_ASYM_EQ_SQ_THIGH) += thigh;
  ROW(GO2NN_ASYM_EQ_SQ_CALF) += calf;
  ROW(GO2NN_ASYM_ACT_SQ) += asq;
  ROW(GO2NN_ASYM_EQ_MAX) = fmaxf(ROW(GO2NN_ASYM_EQ_MAX), emax);
  if (!sym) return;
  float cl = 0.f, cr = 0.f;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const Go2nnEvalField& cf = in.contact_forces;
    const float fz = ((const float*)cf.p)[(long long)e * cf.env_stride + (long long)in.foot_body[f] * in.contact_body_stride + 2LL * cf.comp_stride];
    const float down = fz > in.contact_threshold ? 1.f : 0.f;
    cl += in.foot_side[f] > 0 ? down : 0.f;
    cr += in.foot_side[f] > 0 ? 0.f : down;
  }
  ROW(GO2NN_ASYM_SYM_STEPS) += 1.f;
  ROW(GO2NN_ASYM_ACT_SQ_L) += al;
  ROW(GO2NN_ASYM_ACT_SQ_R) += ar;
  ROW(GO2NN_ASYM_TORQUE_SQ_L) += tl;
  ROW(GO2NN_ASYM_TORQUE_SQ_R) += tr;
  ROW(GO2NN_ASYM_POWER_L) += pl;
  ROW(GO2NN_ASYM_POWER_R) += pr;
  ROW(GO2NN_ASYM_CONTACT_L) += cl;
  ROW(GO2NN_ASYM_CONTACT_R) += cr;
#undef ROW
}

// column c of go2nn_asym_reduce's output for env e: 1 (the group's size), the table's rows after STEP (EQ_MAX: the value the group's MAX is taken over), then per (L, R)
// pair the robot's own |L - R| / (L + R) and whether it has one
struct AsymTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const {
    if (c == GO2NN_ASYM_OUT_N) return 1.0;
    if (c < GO2NN_ASYM_OUT_IMB0) return (double)table[(long long)(c - GO2NN_ASYM_OUT_ROW0 + 1) * N + e];
    const int p = (c - GO2NN_ASYM_OUT_IMB0) >> 1;
    const double l = (double)table[(long long)(GO2NN_ASYM_PAIR0 + 2 * p) * N + e], r = (double)table[(long long)(GO2NN_ASYM_PAIR0 + 2 * p + 1) * N + e];
    const bool has = l + r > 0.0;
    if ((c - GO2NN_ASYM_OUT_IMB0) & 1) return has ? 1.0 : 0.0;
    return has ? fabs(l - r) / (l + r) : 0.0;
  }
};
static_assert(GO2NN_ASYM_STEP == 0 && GO2NN_ASYM_NUM == GO2NN_ASYM_PAIR0 + 8, "STEP is the first row; the four (L, R) pairs are the last eight");
#define ASYM_OUT_EQ_MAX (GO2NN_ASYM_OUT_ROW0 + GO2NN_ASYM_EQ_MAX - 1)

struct AsymAccumulate {
  Go2nnAsymIn in; const float *actions, *mirrored; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { asym_accumulate_env(in, actions, mirrored, table, N, e); }
};

static const char* asym_in_bad(const Go2nnAsymIn* in) {
  const Go2nnEvalField* f[] = {&in->commands, &in->dof_state, &in->torques, &in->contact_forces, &in->reset_buf};          // (reset_buf, the per-env field, comes last)
  for (const Go2nnEvalField* x : f)
    switch (eval_field_fault(*x, x == &in->reset_buf ? 0 : 1)) {
      case EVAL_FIELD_NULL: return "a null buffer pointer";
      case EVAL_FIELD_ENV_STRIDE: return "a field with an env stride < 1";
      case EVAL_FIELD_COMP_STRIDE: return "a vector field with a component stride < 1";
    }
  if (in->dof_vel_offset < 1) return "dof_vel_offset < 1";
  if (in->contact_body_stride < 1) return "a body stride < 1";
  for (int k = 0; k < 4; ++k) {
    if (in->foot_body[k] < 0) return "foot_body < 0";
    if (in->foot_side[k] != 1 && in->foot_side[k] != -1) return "foot_side: +1 (left) or -1 (right)";
  }
  for (int j = 0; j < 12; ++j) {
    if (in->action_perm[j] < 0 || in->action_perm[j] >= 12) return "action_perm outside [0, 12)";
    if (in->action_sign[j] != 1.0f && in->action_sign[j] != -1.0f) return "action_sign: +1 or -1";
    if (in->joint_side[j] != 1 && in->joint_side[j] != -1) return "joint_side: +1 (left) or -1 (right)";
    if (in->joint_kind[j] < 0 || in->joint_kind[j] > 2) return "joint_kind: 0 hip, 1 thigh, 2 calf";
  }
  if (!(in->contact_threshold >= 0.f) || !(in->contact_threshold <= 3.0e38f)) return "contact_threshold negative or not finite";
  return nullptr;
}

extern "C" {

int go2nn_asym_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "asym begin: bad argument (a table and N >= 1)");
  return eval_table_begin(table, GO2NN_ASYM_NUM, N, (float)start, stream);          // (STEP is the table's first row: the static_assert above)
}

int go2nn_asym_accumulate(const Go2nnAsymIn* in, const float* actions, const float* mirrored_actions, float* table, int32_t N, void* stream) {
  if (!in || !actions || !mirrored_actions || !table || N < 1) FAIL(GO2NN_EINVAL, "asym accumulate: null argument or N < 1");
  if (const char* bad = asym_in_bad(in)) FAIL(GO2NN_EINVAL, "asym accumulate: %s", bad);
  return eval_per_env(AsymAccumulate{*in, actions, mirrored_actions, table, N}, N, stream);
}

int go2nn_asym_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "asym reduce: bad argument (1 <= G <= 65535)");
#ifdef GO2_EMU
  for (int e = 0; e < N; ++e)          // the host build can read the ids (the device build ignores those outside [0, G))
    if (group[e] < 0 || group[e] >= G) FAIL(GO2NN_EINVAL, "asym reduce: group[%d] = %d outside [0, %d)", e, group[e], G);
#endif
  return eval_reduce<ASYM_OUT_EQ_MAX>(AsymTerm{table, N, 0}, group, N, G, GO2NN_ASYM_OUT_NUM, out, stream);          // EQ_MAX: the group's max (eval_group_max), every other column its sum
}

}  // extern "C"

#endif  // GO2NN_ASYM_H
