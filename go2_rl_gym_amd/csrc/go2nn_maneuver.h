// go2nn_maneuver.h — the evaluator's scripted command maneuvers (include/go2nn.h: go2nn_maneuver_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py).
// Included at the end of go2nn_impl.cpp after go2nn_ladder.h (FAIL is the former's helper; EVAL_FN, EVAL_MEMBER, eval_f, eval_b, eval_field_fault and the launch scaffold —
// eval_table_begin, eval_per_env, eval_reduce over eval_group_sum — go2nn_eval.h's; robust_w go2nn_robust.h's).
//
// Two launches per env step (eval_per_env_kernel<ManeuverApply>, <ManeuverAccumulate>), one lane per env, no LDS, no atomics, no cross-lane traffic.  go2nn_maneuver_apply (before the step) reads the env's step counter and writes its
// command row — 3 floats of the schedule and zeros in every further column —; go2nn_maneuver_accumulate (after it) writes the same row again (the step may have reset the robot
// and drawn a command), reads 7 floats and two flags and read-modify-writes the env's column of the table [GO2NN_MANEUVER_NUM, N].  With the HIP simulator's field-major buffers
// (env stride 1) consecutive lanes touch consecutive addresses of every component and of every table row: each load / store instruction of a wave is one dense 256-byte line.
// The spec is read through man_of_env — at most 64 specs of 148 bytes, resident in L2 / the vector cache after the first wave.  Both kernels are launch-bound at evaluation
// sizes (1024 lanes = 16 waves).  The step counter is the table's STEP row, advanced by the accumulate kernel: no host argument changes between steps, so a captured pair
// switches on the right step of every replay.  The host build runs the same element functions in plain loops.
//
// THE CONVENTION: the switch at counted step s takes effect in the apply call BEFORE that step's go2sim_step.  The step's physics runs on an action chosen from an observation
// that still carries the old command; the observation the step produces, and the metrics of step s, carry the new one.  This is the simulator's own resampling order
// (_post_physics_step_callback runs before the rewards and the observations).
#ifndef GO2NN_MANEUVER_H
#define GO2NN_MANEUVER_H

// the segment in force at step s: the one with the largest start <= max(s, 0) (segment 0 also covers the warm-up; count >= 1 and increasing starts are the host check's duty)
EVAL_FN int maneuver_segment(const Go2nnManeuverSpec& sp, int s) {
  int k = 0;
  for (int j = 1; j < GO2NN_MANEUVER_MAX_SEGS; ++j)
    if (j < sp.count && sp.start[j] <= s) k = j;
  return k;
}

EVAL_FN void maneuver_write_command(const Go2nnManeuverIn& in, const Go2nnManeuverSpec& sp, int k, int e) {
  for (int c = 0; c < 3; ++c) *robust_w(in.commands, e, c) = sp.cmd[k][c];
  for (int c = 3; c < in.num_commands; ++c) *robust_w(in.commands, e, c) = 0.f;
}

EVAL_FN void maneuver_apply_env(const Go2nnManeuverIn& in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, const float* table, int N, int e) {
  const int m = man_of_env[e];
  if (m < 0 || m >= in.num_specs) return;
  const Go2nnManeuverSpec& sp = specs[m];
  maneuver_write_command(in, sp, maneuver_segment(sp, (int)table[(long long)GO2NN_MANEUVER_STEP * N + e]), e);
}

EVAL_FN void maneuver_accumulate_env(const Go2nnManeuverIn& in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, float* table, int N, int e) {
  float* col = table + e;
#define ROW(r) col[(long long)GO2NN_MANEUVER_##r * N]
  const float sf = ROW(STEP);
  const int m = man_of_env[e];
  if (m >= 0 && m < in.num_specs) {
    const Go2nnManeuverSpec& sp = specs[m];
    const int s = (int)sf, k = maneuver_segment(sp, s);
    maneuver_write_command(in, sp, k, e);
    if (k >= 1 && sp.start[k] == s) {
      ROW(OPEN) = 1.f;
      ROW(OK_RUN) = 0.f;
      ROW(IS_SETTLED) = 0.f;
      ROW(IS_FELL) = 0.f;
      ROW(PEAK_TILT) = 0.f;
      ROW(SWITCHES) += 1.f;
    }
    const float open = ROW(OPEN);
    if (open > 0.f) {
      if (ROW(IS_FELL) == 0.f) {
        if (eval_b(in.reset_buf, e) != 0 && eval_b(in.time_out_buf, e) == 0) {          // the buffers already hold the post-reset state: the flags come first
          ROW(SWITCH_FALLS) += 1.f;
          ROW(IS_FELL) = 1.f;
        } else {
          const float dx = sp.cmd[k][0] - eval_f(in.base_lin_vel, e, 0), dy = sp.cmd[k][1] - eval_f(in.base_lin_vel, e, 1);
          const float gx = eval_f(in.projected_gravity, e, 0), gy = eval_f(in.projected_gravity, e, 1);
          const float err_lin = sqrtf(dx * dx + dy * dy), err_ang = fabsf(sp.cmd[k][2] - eval_f(in.base_ang_vel, e, 2)), tilt = sqrtf(gx * gx + gy * gy);
          ROW(WIN_STEPS) += 1.f;
          ROW(WIN_LIN_ERR) += err_lin;
          ROW(WIN_ANG_ERR) += err_ang;
          ROW(PEAK_TILT) = fmaxf(ROW(PEAK_TILT), tilt);
          if (ROW(IS_SETTLED) == 0.f) {
            if (err_lin < sp.thr_lin && err_ang < sp.thr_ang) {
              const float run = ROW(OK_RUN) + 1.f;
              ROW(OK_RUN) = run;
              if (run == (float)sp.hold) {
                ROW(SETTLED) += 1.f;
                ROW(SETTLE_STEPS) += open;
                ROW(IS_SETTLED) = 1.f;
              }
            } else {
              ROW(OK_RUN) = 0.f;
            }
          }
        }
      }
      if (open == (float)sp.window) {
        ROW(PEAK_TILT_SUM) += ROW(PEAK_TILT);
        ROW(OPEN) = 0.f;
      } else {
        ROW(OPEN) = open + 1.f;
      }
    }
  }
  ROW(STEP) = sf + 1.f;
#undef ROW
}

// column c of go2nn_maneuver_reduce's output: the accumulator rows, then 1 (the group's size)
struct ManeuverTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const { return c < GO2NN_MANEUVER_ACC_NUM ? (double)table[(long long)(GO2NN_MANEUVER_ACC_FIRST + c) * N + e] : 1.0; }
};

struct ManeuverApply {
  Go2nnManeuverIn in; const Go2nnManeuverSpec* specs; const int32_t* man_of_env; const float* table; int N;
  EVAL_MEMBER void operator()(int e) const { maneuver_apply_env(in, specs, man_of_env, table, N, e); }
};
struct ManeuverAccumulate {
  Go2nnManeuverIn in; const Go2nnManeuverSpec* specs; const int32_t* man_of_env; float* table; int N;
  EVAL_MEMBER void operator()(int e) const { maneuver_accumulate_env(in, specs, man_of_env, table, N, e); }
};

static const char* maneuver_in_bad(const Go2nnManeuverIn* in) {
  const Go2nnEvalField* vec[] = {&in->commands, &in->base_lin_vel, &in->base_ang_vel, &in->projected_gravity};
  const Go2nnEvalField* flag[] = {&in->reset_buf, &in->time_out_buf};
  for (const Go2nnEvalField* x : vec)
    if (const int bad = eval_field_fault(*x, 1)) return bad == EVAL_FIELD_NULL ? "a null buffer pointer" : "a vector field with an env stride or a component stride < 1";
  for (const Go2nnEvalField* x : flag)
    if (const int bad = eval_field_fault(*x, 0)) return bad == EVAL_FIELD_NULL ? "a null buffer pointer" : "a flag field with an env stride < 1";
  if (in->num_specs < 1 || in->num_specs > GO2NN_MANEUVER_MAX_SPECS) return "num_specs outside [1, 64]";
  if (in->num_commands < 3) return "num_commands < 3";
  return nullptr;
}

extern "C" {

int go2nn_maneuver_check_specs(const Go2nnManeuverSpec* specs, int32_t M) {
  if (!specs) FAIL(GO2NN_EINVAL, "maneuver specs: null pointer");
  if (M < 1 || M > GO2NN_MANEUVER_MAX_SPECS) FAIL(GO2NN_EINVAL, "maneuver specs: M = %d maneuvers (1 .. %d)", M, GO2NN_MANEUVER_MAX_SPECS);
  for (int m = 0; m < M; ++m) {
    const Go2nnManeuverSpec& s = specs[m];
    if (s.count < 1 || s.count > GO2NN_MANEUVER_MAX_SEGS) FAIL(GO2NN_EINVAL, "maneuver spec %d: count = %d segments (1 .. %d)", m, s.count, GO2NN_MANEUVER_MAX_SEGS);
    if (s.start[0] != 0) FAIL(GO2NN_EINVAL, "maneuver spec %d: start[0] = %d (segment 0 starts at step 0)", m, s.start[0]);
    if (s.hold < 1 || s.window < s.hold) FAIL(GO2NN_EINVAL, "maneuver spec %d: hold = %d, window = %d steps (1 <= hold <= window)", m, s.hold, s.window);
    if (!(s.thr_lin > 0.f) || !(s.thr_ang > 0.f)) FAIL(GO2NN_EINVAL, "maneuver spec %d: thr_lin = %g, thr_ang = %g (both > 0)", m, (double)s.thr_lin, (double)s.thr_ang);
    for (int k = 1; k < s.count; ++k) {
      if (s.start[k] <= s.start[k - 1]) FAIL(GO2NN_EINVAL, "maneuver spec %d: start[%d] = %d after start[%d] = %d (strictly increasing)", m, k, s.start[k], k - 1, s.start[k - 1]);
      if (k >= 2 && s.window > s.start[k] - s.start[k - 1])
        FAIL(GO2NN_EINVAL, "maneuver spec %d: window = %d steps, but the switches %d and %d are %d steps apart (windows do not overlap)", m, s.window, k - 1, k,
             s.start[k] - s.start[k - 1]);
    }
  }
  return 0;
}

int go2nn_maneuver_begin(float* table, int32_t N, int32_t start, void* stream) {
  if (!table || N < 1) FAIL(GO2NN_EINVAL, "maneuver begin: bad argument (a table and N >= 1)");
  static_assert(GO2NN_MANEUVER_STEP == 0, "the STEP row is the table's first N floats");
  return eval_table_begin(table, GO2NN_MANEUVER_NUM, N, (float)start, stream);
}

int go2nn_maneuver_apply(const Go2nnManeuverIn* in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, const float* table, int32_t N, void* stream) {
  if (!in || !specs || !man_of_env || !table || N < 1) FAIL(GO2NN_EINVAL, "maneuver apply: null argument or N < 1");
  if (const char* bad = maneuver_in_bad(in)) FAIL(GO2NN_EINVAL, "maneuver apply: %s", bad);
  return eval_per_env(ManeuverApply{*in, specs, man_of_env, table, N}, N, stream);
}

int go2nn_maneuver_accumulate(const Go2nnManeuverIn* in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, float* table, int32_t N, void* stream) {
  if (!in || !specs || !man_of_env || !table || N < 1) FAIL(GO2NN_EINVAL, "maneuver accumulate: null argument or N < 1");
  if (const char* bad = maneuver_in_bad(in)) FAIL(GO2NN_EINVAL, "maneuver accumulate: %s", bad);
  return eval_per_env(ManeuverAccumulate{*in, specs, man_of_env, table, N}, N, stream);
}

int go2nn_maneuver_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "maneuver reduce: bad argument (1 <= G <= 65535)");
  return eval_reduce(ManeuverTerm{table, N, 0}, group, N, G, GO2NN_MANEUVER_ACC_NUM + 1, out, stream);
}

}  // extern "C"

#endif  // GO2NN_MANEUVER_H
