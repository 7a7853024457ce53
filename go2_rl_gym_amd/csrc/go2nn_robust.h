// go2nn_robust.h — the evaluator's perturbation kernels (include/go2nn.h: go2nn_robust_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp after go2nn_trace.h (FAIL is the former's helper; EVAL_FN, EVAL_MEMBER, eval_f, eval_b, eval_field_fault and the launch scaffold —
// eval_table_begin, eval_per_env, eval_reduce over eval_group_sum — go2nn_eval.h's).
//
// Two launches per env step (eval_per_env_kernel<RobustApply>, <RobustAccumulate>), one lane per env, no LDS, no atomics, no cross-lane traffic.  go2nn_robust_apply (before the step) writes the env's masked dynamics rows —
// up to 38 floats — and, on a scheduled step, adds the rotated impulse to three root-state floats; go2nn_robust_accumulate (after it) reads 7 floats and two flags and
// read-modify-writes the env's column of the table [GO2NN_ROBUST_NUM, N].  With the HIP simulator's field-major buffers (env stride 1) consecutive lanes touch consecutive
// addresses of every component and of every table row: each load / store instruction of a wave is one dense 256-byte line.  The spec is read through pert_of_env — at most 64
// specs of 64 bytes, resident in L2 / the vector cache after the first wave.  Both kernels are launch-bound at evaluation sizes (1024 lanes = 16 waves).
// The step counter is the table's STEP row, advanced by the accumulate kernel: no host argument changes between steps, so a captured pair advances on every replay.
// The host build runs the same element functions in plain loops.
#ifndef GO2NN_ROBUST_H
#define GO2NN_ROBUST_H

EVAL_FN float* robust_w(const Go2nnEvalField& f, int e, int c) { return (float*)f.p + ((long long)e * f.env_stride + (long long)c * f.comp_stride); }

// does a push fire at step s?  (period >= 1 is the host check's duty; a bad spec that got here never fires instead of dividing by zero)
EVAL_FN bool robust_fires(const Go2nnRobustSpec& sp, int s) {
  if (sp.count <= 0 || sp.period < 1 || s < sp.first) return false;
  const int d = s - sp.first;
  return d % sp.period == 0 && d / sp.period < sp.count;
}

EVAL_FN void robust_apply_env(const Go2nnRobustIn& in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int N, int e) {
  const int p = pert_of_env[e];
  if (p < 0 || p >= in.num_specs) return;
  const Go2nnRobustSpec sp = specs[p];
  if (sp.mask & GO2NN_ROBUST_MASK_STRENGTH)
    for (int j = 0; j < 12; ++j) *robust_w(in.motor_strengths, e, j) = sp.strength;
  if (sp.mask & GO2NN_ROBUST_MASK_KP)
    for (int j = 0; j < 12; ++j) *robust_w(in.p_gains_multiplier, e, j) = sp.kp_mul;
  if (sp.mask & GO2NN_ROBUST_MASK_KD)
    for (int j = 0; j < 12; ++j) *robust_w(in.d_gains_multiplier, e, j) = sp.kd_mul;
  if (sp.mask & GO2NN_ROBUST_MASK_ADDED_MASS) *robust_w(in.added_base_mass, e, 0) = sp.added_mass;
  if (sp.mask & GO2NN_ROBUST_MASK_FRICTION) *robust_w(in.friction_coeffs, e, 0) = sp.friction;
  float* col = table + e;
  if (!robust_fires(sp, (int)col[(long long)GO2NN_ROBUST_STEP * N])) return;
  const float qx = eval_f(in.root_states, e, 3), qy = eval_f(in.root_states, e, 4), qz = eval_f(in.root_states, e, 5), qw = eval_f(in.root_states, e, 6);
  float c = 1.f - 2.f * (qy * qy + qz * qz), s = 2.f * (qx * qy + qw * qz);
  const float n = sqrtf(c * c + s * s);
  if (n < 1e-6f) { c = 1.f; s = 0.f; } else { c /= n; s /= n; }
  *robust_w(in.root_states, e, 7) += c * sp.dv[0] - s * sp.dv[1];
  *robust_w(in.root_states, e, 8) += s * sp.dv[0] + c * sp.dv[1];
  *robust_w(in.root_states, e, 9) += sp.dv[2];
  col[(long long)GO2NN_ROBUST_OPEN * N] = 1.f;
  col[(long long)GO2NN_ROBUST_PEAK_ERR * N] = 0.f;
  col[(long long)GO2NN_ROBUST_PEAK_TILT * N] = 0.f;
  col[(long long)GO2NN_ROBUST_OK_RUN * N] = 0.f;
  col[(long long)GO2NN_ROBUST_DONE * N] = 0.f;
  col[(long long)GO2NN_ROBUST_PUSHES * N] += 1.f;
}

EVAL_FN void robust_accumulate_env(const Go2nnRobustIn& in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int N, int e) {
  float* col = table + e;
#define ROW(r) col[(long long)GO2NN_ROBUST_##r * N]
  const int p = pert_of_env[e];
  const float open = ROW(OPEN);
  if (p >= 0 && p < in.num_specs && open > 0.f) {
    const Go2nnRobustSpec sp = specs[p];
    if (ROW(DONE) == 0.f) {
      const float dx = eval_f(in.commands, e, 0) - eval_f(in.base_lin_vel, e, 0), dy = eval_f(in.commands, e, 1) - eval_f(in.base_lin_vel, e, 1);
      const float gx = eval_f(in.projected_gravity, e, 0), gy = eval_f(in.projected_gravity, e, 1);
      const float err = sqrtf(dx * dx + dy * dy), tilt = sqrtf(gx * gx + gy * gy);
      const bool fall = eval_b(in.reset_buf, e) != 0 && eval_b(in.time_out_buf, e) == 0;
      ROW(PEAK_ERR) = fmaxf(ROW(PEAK_ERR), err);
      ROW(PEAK_TILT) = fmaxf(ROW(PEAK_TILT), tilt);
      if (fall) {
        ROW(PUSH_FALLS) += 1.f;
        ROW(DONE) = 1.f;
      } else if (err < sp.thr) {
        const float run = ROW(OK_RUN) + 1.f;
        ROW(OK_RUN) = run;
        if (run == (float)sp.hold) {
          ROW(RECOVERED) += 1.f;
          ROW(RECOVERY_STEPS) += open;
          ROW(DONE) = 1.f;
        }
      } else {
        ROW(OK_RUN) = 0.f;
      }
    }
    if (open >= (float)sp.window) {
      ROW(PEAK_ERR_SUM) += ROW(PEAK_ERR);
      ROW(PEAK_TILT_SUM) += ROW(PEAK_TILT);
      ROW(OPEN) = 0.f;
    } else {
      ROW(OPEN) = open + 1.f;
    }
  }
  ROW(STEP) += 1.f;
#undef ROW
}

// column c of go2nn_robust_reduce's output: the accumulator rows, then 1 (the group's size)
struct RobustTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const { return c < GO2NN_ROBUST_ACC_NUM ? (double)table[(long long)(GO2NN_ROBUST_ACC_FIRST + c) * N + e] : 1.0; }
};

struct RobustApply {
  Go2nnRobustIn in; const Go2nnRobustSpec* specs; const int32_t* pert_of_env; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { robust_apply_env(in, specs, pert_of_env, table, N, e); }
};
struct RobustAccumulate {
  Go2nnRobustIn in; const Go2nnRobustSpec* specs; const int32_t* pert_of_env; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { robust_accumulate_env(in, specs, pert_of_env, table, N, e); }
};

static const char* robust_in_bad(const Go2nnRobustIn* in) {
  const Go2nnEvalField* vec[] = {&in->root_states, &in->commands, &in->base_lin_vel, &in->projected_gravity, &in->motor_strengths, &in->p_gains_multiplier,
                                 &in->d_gains_multiplier};
  const Go2nnEvalField* scalar[] = {&in->reset_buf, &in->time_out_buf, &in->added_base_mass, &in->friction_coeffs};
  for (const Go2nnEvalField* x : vec)
    if (const int bad = eval_field_fault(*x, 1)) return bad == EVAL_FIELD_NULL ? "a null buffer pointer" : "a vector field with an env stride or a component stride < 1";
  for (const Go2nnEvalField* x : scalar)
    if (const int bad = eval_field_fault(*x, 0)) return bad == EVAL_FIELD_NULL ? "a null buffer pointer" : "a per-env field with an env stride < 1";
  if (in->num_specs < 1 || in->num_specs > GO2NN_ROBUST_MAX_SPECS) return "num_specs outside [1, 64]";
  return nullptr;
}

extern "C" {

int go2nn_robust_check_specs(const Go2nnRobustSpec* specs, int32_t P) {
  if (!specs) FAIL(GO2NN_EINVAL, "robust specs: null pointer");
  if (P < 1 || P > GO2NN_ROBUST_MAX_SPECS) FAIL(GO2NN_EINVAL, "robust specs: P = %d perturbations (1 .. %d)", P, GO2NN_ROBUST_MAX_SPECS);
  for (int p = 0; p < P; ++p) {
    const Go2nnRobustSpec& s = specs[p];
    if (s.hold < 1) FAIL(GO2NN_EINVAL, "robust spec %d: hold = %d steps (>= 1)", p, s.hold);
    if (s.first < 0 || s.count < 0) FAIL(GO2NN_EINVAL, "robust spec %d: first = %d, count = %d (both >= 0)", p, s.first, s.count);
    if (s.count > 0 && s.period < 1) FAIL(GO2NN_EINVAL, "robust spec %d: period = %d steps (>= 1 when count > 0)", p, s.period);
    if (s.count > 0 && (s.window < 1 || s.window > s.period))
      FAIL(GO2NN_EINVAL, "robust spec %d: window = %d steps (1 .. period = %d when count > 0: windows do not overlap)", p, s.window, s.period);
  }
  return 0;
}

int go2nn_robust_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "robust begin: bad argument (a table and N >= 1)");
  static_assert(GO2NN_ROBUST_STEP == 0, "the STEP row is the table's first N floats");
  return eval_table_begin(table, GO2NN_ROBUST_NUM, N, (float)start, stream);
}

int go2nn_robust_apply(const Go2nnRobustIn* in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int32_t N, void* stream) {
  if (!in || !specs || !pert_of_env || !table || N < 1) FAIL(GO2NN_EINVAL, "robust apply: null argument or N < 1");
  if (const char* bad = robust_in_bad(in)) FAIL(GO2NN_EINVAL, "robust apply: %s", bad);
  return eval_per_env(RobustApply{*in, specs, pert_of_env, table, N}, N, stream);
}

int go2nn_robust_accumulate(const Go2nnRobustIn* in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int32_t N, void* stream) {
  if (!in || !specs || !pert_of_env || !table || N < 1) FAIL(GO2NN_EINVAL, "robust accumulate: null argument or N < 1");
  if (const char* bad = robust_in_bad(in)) FAIL(GO2NN_EINVAL, "robust accumulate: %s", bad);
  return eval_per_env(RobustAccumulate{*in, specs, pert_of_env, table, N}, N, stream);
}

int go2nn_robust_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "robust reduce: bad argument (1 <= G <= 65535)");
  return eval_reduce(RobustTerm{table, N, 0}, group, N, G, GO2NN_ROBUST_ACC_NUM + 1, out, stream);
}

}  // extern "C"

#endif  // GO2NN_ROBUST_H
