// go2nn_actuator.h — the evaluator's per-joint actuator loads (include/go2nn.h: go2nn_actuator_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py, `evaluation.actuators`).
// Included at the end of go2nn_impl.cpp after go2nn_bootstrap.h (FAIL is the former's helper, bootstrap_refuse the latter's; EVAL_FN, EVAL_MEMBER, eval_b, eval_field_fault and
// the launch scaffold — eval_table_begin, eval_per_env, eval_reduce, eval_bootstrap — go2nn_eval.h's).
//
// One launch per env step (eval_per_env_kernel<ActuatorAccumulate>), one lane per robot, the twelve joints and four feet unrolled inside the lane; no LDS, no atomics, no
// cross-lane traffic.  A lane reads per joint three floats (torque, position, velocity), per foot one (force z), the root's planar velocity and one flag, and read-modify-writes
// its column of the table [GO2NN_ACTUATOR_NUM, N]: with the HIP simulator's field-major buffers (env stride 1) every load and every table access of a wave is one dense
// 256-byte line.  The by-value limit arrays are indexed by the unrolled loops' constants only, so they stay in the kernel's argument registers: no scratch.  The step counter
// is the table's STEP row, advanced by the kernel itself: no host argument changes between steps, so a captured launch advances on every replay.  The host build runs the same
// element functions in plain loops.  The rule is stated once, in include/go2nn.h.
//
// THE LANE'S SHAPE.  Read from the gfx950 code object's notes (build.py kernel_resources; scratch 0 and LDS 0 in every row) and timed on an MI355X in one session: device
// events around 200 back-to-back launches on the buffers of a go2_flat evaluation, 1024 robots, every call a counted step, next to go2nn_gait_accumulate (4.3 - 5.1 us) and
// go2nn_asym_accumulate (6.8 - 7.0 us) timed the same way in the same process (profiles/actuators_bench.json, "variants").  Every form writes the same bits.
//   form                                                              VGPRs  SGPRs   us per launch
//   one lane per robot, a joint's rows loaded, updated, stored in turn    41     78   6.37
//   one lane per (joint, robot)                                           43     94   4.23 - 4.45   a hand-written kernel: workgroups of 12 waves = 12 joints x 64 robots, the
//                                                                                                   robot's STEP, USED and reset flag read in front of a barrier, joint 0's lane
//                                                                                                   writing them behind it; the per-robot rows to joint 0's lane, foot f to joint f's
//   one lane per robot, every load in front of the first store           378     74   5.14 - 5.87   kept
// The table and the simulator's buffers come as plain pointers that may alias for all the compiler knows, so a load behind a store waits for it: joint by joint in place a
// lane is a chain of dependent memory round trips, and putting its 40 input loads and 110 row loads in front of its first store takes 1.2 us off the launch at the price
// of registers nobody else wants (256 VGPRs + 122 AGPRs, one wave per SIMD: 1024 robots are 16 waves on 256 compute units; tests/test_actuator_host.py
// test_no_kernel_has_scratch holds every build to 0 bytes of scratch, so a compiler that starts to spill this lane is seen).  Twelve times the lanes gain another 0.7 - 0.9
// us, but all three forms lie between the gait launch and the asymmetry launch, which are launch-bound at this size: the scaffold form is not clearly slower than those
// two, so it stays, and the hand-written kernel with its barrier was not kept.
//
// THE BOOTSTRAP'S WINDOW.  go2nn_actuator_bootstrap is eval_bootstrap<112, CHUNK> (go2nn_eval.h) with the reduce's Term; the widths tried, timed as go2nn_eval.h's table was
// (200 back-to-back launches, 1024 robots, B = 1000) next to go2nn_gait_bootstrap in the same session (132 / 75 / 69 us):
//   CHUNK  windows  VGPRs  SGPRs   us per launch at 6 / 42 / 294 cells
//     112        1    255     41   1034 / 191 / 150
//      56        2    178    106    607 / 173 / 146
//      28        4    113     99    318 / 129 / 135
//      16        7     76     75    217 / 146 / 132
//      14        8     68     71    196 / 146 / 132
//       8       14     48     59    174 / 134 / 129     kept: the shortest serial walk that still pays for itself at few cells, and the fastest at 294
//       7       16     48     55    220 / 128 / 190
// ActuatorTerm only turns a run-time column into a row index, as GaitTerm does, so narrow windows cost nothing but the draws every window recomputes.
#ifndef GO2NN_ACTUATOR_H
#define GO2NN_ACTUATOR_H

#define ACT_ROW(r) table[(long long)(r) * N + e]

// joint j on a used frame: its GO2NN_ACTUATOR_JOINT_ROWS rows r, in registers;  first: no frame of this robot has been used yet
EVAL_FN void actuator_joint(const Go2nnActuatorIn& in, int j, bool first, float tau, float q, float qd, float* r) {
  const float at = fabsf(tau), av = fabsf(qd), p = tau * qd;
  const float m = fminf(q - in.pos_lo[j], in.pos_hi[j] - q);
  r[GO2NN_ACTUATOR_J_TAU_SQ] += tau * tau;
  r[GO2NN_ACTUATOR_J_TAU_PEAK] = fmaxf(r[GO2NN_ACTUATOR_J_TAU_PEAK], at);
  r[GO2NN_ACTUATOR_J_TAU_SAT] += at >= in.tau_sat_thr[j] ? 1.f : 0.f;
  r[GO2NN_ACTUATOR_J_VEL_PEAK] = fmaxf(r[GO2NN_ACTUATOR_J_VEL_PEAK], av);
  r[GO2NN_ACTUATOR_J_VEL_SAT] += av >= in.vel_sat_thr[j] ? 1.f : 0.f;
  r[GO2NN_ACTUATOR_J_WORK_POS] += fmaxf(p, 0.f);
  r[GO2NN_ACTUATOR_J_WORK_NEG] += fmaxf(-p, 0.f);
  r[GO2NN_ACTUATOR_J_MARGIN_MIN] = first ? m : fminf(r[GO2NN_ACTUATOR_J_MARGIN_MIN], m);
}

// a foot on a used frame: its GO2NN_ACTUATOR_FOOT_ROWS rows r, in registers
EVAL_FN void actuator_foot(const Go2nnActuatorIn& in, float fz, float* r) {
  r[GO2NN_ACTUATOR_F_FZ_PEAK] = fmaxf(r[GO2NN_ACTUATOR_F_FZ_PEAK], fz);
  if (fz > in.contact_threshold) {
    r[GO2NN_ACTUATOR_F_FZ_SUM] += fz;
    r[GO2NN_ACTUATOR_F_FZ_FRAMES] += 1.f;
  }
}

EVAL_FN void actuator_joint_in(const Go2nnActuatorIn& in, int e, int j, float& tau, float& q, float& qd) {
  const long long q_at = (long long)e * in.dof_state.env_stride + (long long)j * in.dof_state.comp_stride;
  q = ((const float*)in.dof_state.p)[q_at];
  qd = ((const float*)in.dof_state.p)[q_at + in.dof_vel_offset];
  tau = eval_f(in.torques, e, j);
}

EVAL_FN float actuator_foot_in(const Go2nnActuatorIn& in, int e, int f) {
  const Go2nnEvalField& cf = in.contact_forces;
  return ((const float*)cf.p)[(long long)e * cf.env_stride + (long long)in.foot_body[f] * in.contact_body_stride + 2LL * cf.comp_stride];
}

// Robot e for one step.  Every input and every table row of the lane is loaded before the first row is stored (THE LANE'S SHAPE above)
EVAL_FN void actuator_accumulate_env(const Go2nnActuatorIn& in, float* table, int N, int e) {
  const float s = ACT_ROW(GO2NN_ACTUATOR_STEP);
  const bool reset = eval_b(in.reset_buf, e) != 0;
  float tau[12], q[12], qd[12], fz[4], r[GO2NN_ACTUATOR_NUM];
#pragma unroll
  for (int j = 0; j < 12; ++j) actuator_joint_in(in, e, j, tau[j], q[j], qd[j]);
#pragma unroll
  for (int f = 0; f < 4; ++f) fz[f] = actuator_foot_in(in, e, f);
  const float vx = eval_f(in.root_states, e, 7), vy = eval_f(in.root_states, e, 8);
#pragma unroll
  for (int k = 1; k < GO2NN_ACTUATOR_NUM; ++k) r[k] = ACT_ROW(k);
  ACT_ROW(GO2NN_ACTUATOR_STEP) = s + 1.f;
  if (s < 0.f || reset) return;          // warm-up; or the frame shows the post-reset pose
  const bool first = r[GO2NN_ACTUATOR_USED] == 0.f;
  r[GO2NN_ACTUATOR_USED] += 1.f;
  r[GO2NN_ACTUATOR_DIST] += sqrtf(vx * vx + vy * vy);
#pragma unroll
  for (int j = 0; j < 12; ++j) actuator_joint(in, j, first, tau[j], q[j], qd[j], r + GO2NN_ACTUATOR_JOINT0 + j * GO2NN_ACTUATOR_JOINT_ROWS);
#pragma unroll
  for (int f = 0; f < 4; ++f) actuator_foot(in, fz[f], r + GO2NN_ACTUATOR_FOOT0 + f * GO2NN_ACTUATOR_FOOT_ROWS);
#pragma unroll
  for (int k = 1; k < GO2NN_ACTUATOR_NUM; ++k) ACT_ROW(k) = r[k];
}

// column c of go2nn_actuator_reduce's output for robot e: 1 (the group's size), 1 if the robot has a used frame, then table row c - 1 (USED, DIST, the joint and foot rows)
struct ActuatorTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const {
    if (c == GO2NN_ACTUATOR_OUT_N) return 1.0;
    if (c == GO2NN_ACTUATOR_OUT_N_USED) return table[(long long)GO2NN_ACTUATOR_USED * N + e] > 0.f ? 1.0 : 0.0;
    return (double)table[(long long)(c - GO2NN_ACTUATOR_OUT_ROW0 + 1) * N + e];
  }
};
static_assert(GO2NN_ACTUATOR_STEP == 0 && GO2NN_ACTUATOR_OUT_NUM == GO2NN_ACTUATOR_NUM + 1, "every table row but STEP is an output column, behind N and N_USED");

struct ActuatorAccumulate {
  Go2nnActuatorIn in; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { actuator_accumulate_env(in, table, N, e); }
};

#undef ACT_ROW

#ifndef BOOTSTRAP_ACTUATOR_CHUNK
#define BOOTSTRAP_ACTUATOR_CHUNK 8          // 112 columns in 14 windows (the table above; a width divides the column count: eval_bootstrap asserts it)
#endif

static const char* actuator_in_bad(const Go2nnActuatorIn* in) {
  const Go2nnEvalField* vec[] = {&in->dof_state, &in->torques, &in->contact_forces, &in->root_states};
  int worst = eval_field_fault(in->reset_buf, 0);
  for (const Go2nnEvalField* f : vec) {
    const int fault = eval_field_fault(*f, 1);
    if (fault && (!worst || fault < worst)) worst = fault;
  }
  if (worst == EVAL_FIELD_NULL) return "a null buffer pointer";
  if (worst == EVAL_FIELD_ENV_STRIDE) return "a field with an env stride < 1";
  if (worst) return "a vector field with a component stride < 1";
  if (in->dof_vel_offset < 1) return "dof_vel_offset < 1";
  if (in->contact_body_stride < 1) return "a body stride < 1";
  for (int f = 0; f < 4; ++f)
    if (in->foot_body[f] < 0) return "foot_body < 0";
  const auto finite = [](float x) { return x - x == 0.f; };          // (neither NaN nor an infinity: every finite fp32 passes)
  for (int j = 0; j < 12; ++j) {
    if (!finite(in->pos_lo[j]) || !finite(in->pos_hi[j]) || in->pos_lo[j] > in->pos_hi[j]) return "pos_lo / pos_hi: finite limits with pos_lo <= pos_hi";
    if (!(in->tau_sat_thr[j] > 0.f) || !finite(in->tau_sat_thr[j])) return "tau_sat_thr: a finite torque > 0";
    if (!(in->vel_sat_thr[j] > 0.f) || !finite(in->vel_sat_thr[j])) return "vel_sat_thr: a finite speed > 0";
  }
  if (!(in->contact_threshold >= 0.f) || !finite(in->contact_threshold)) return "contact_threshold negative or not finite";
  return nullptr;
}

extern "C" {

int go2nn_actuator_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "actuator begin: bad argument (a table and N >= 1)");
  return eval_table_begin(table, GO2NN_ACTUATOR_NUM, N, (float)start, stream);
}

int go2nn_actuator_accumulate(const Go2nnActuatorIn* in, float* table, int32_t N, void* stream) {
  if (!in || !table || N < 1) FAIL(GO2NN_EINVAL, "actuator accumulate: null argument or N < 1");
  if (const char* bad = actuator_in_bad(in)) FAIL(GO2NN_EINVAL, "actuator accumulate: %s", bad);
  return eval_per_env(ActuatorAccumulate{*in, table, N}, N, stream);
}

int go2nn_actuator_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "actuator reduce: bad argument (1 <= G <= 65535)");
  return eval_reduce(ActuatorTerm{table, N, 0}, group, N, G, GO2NN_ACTUATOR_OUT_NUM, out, stream);
}

int go2nn_actuator_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream) {
  if (bootstrap_refuse("actuator", table, cell_start, cell_envs, out, N, G, B, GO2NN_ACTUATOR_OUT_NUM)) return GO2NN_EINVAL;
  return eval_bootstrap<GO2NN_ACTUATOR_OUT_NUM, BOOTSTRAP_ACTUATOR_CHUNK>(ActuatorTerm{table, N, 0}, cell_start, cell_envs, G, B, seed, out, stream);
}

}  // extern "C"

#endif  // GO2NN_ACTUATOR_H
