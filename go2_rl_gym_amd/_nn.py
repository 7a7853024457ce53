"""ctypes binding of include/go2nn.h (the policy-side MFMA kernels) and the small host object the algorithms use.

`load_nn()` loads go2_rl_gym_amd/libgo2nn_hip.so and raises if it is missing — like _lib.load_hip there is no CPU fallback in the product;
tests hand `PolicyKernel` the host build (tests/emu/libgo2nn_emu.so) explicitly."""
import ctypes as C
import os

import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
NN_LIB = os.path.join(_HERE, "libgo2nn_hip.so")
GO2NN_MAX_LAYERS, GO2NN_MAX_WIDTH, GO2NN_ABI_VERSION, GO2NN_MAX_GROUP = 6, 512, 7, 2
GO2NN_RNN_LSTM, GO2NN_RNN_GRU, GO2NN_RNN_MAX_STATES = 0, 1, 4
GO2NN_TM_MAX_FORWARD, GO2NN_TM_MAX_INPUT_GRAD = 3, 2
GO2NN_WGRAD_F32_64x64, GO2NN_WGRAD_F32_64x128, GO2NN_WGRAD_SPLIT_128x128 = 1, 2, 3
# the evaluator's accumulators, in the order of the enum GO2NN_EVAL_* of include/go2nn.h (where the formulas are)
EVAL_METRICS = ("steps", "lin_vel_err", "ang_vel_err", "speed_along_cmd", "tilt", "power", "torque_sq", "action_rate_sq", "dof_limit_steps", "falls")
GO2NN_EVAL_NUM = len(EVAL_METRICS)
EVAL_FIELDS = ("commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "dof_state", "torques", "actions", "last_actions", "reset_buf", "time_out_buf")
# the trajectory recorder's frame: (block, floats) in the order of the enum GO2NN_TRACE_* of include/go2nn.h (the one specification; tests/test_trace_host.py holds this
# table to it), and the source buffers of Go2nnTraceIn in the struct's order
TRACE_BLOCKS = (("root_pos", 3), ("root_quat", 4), ("root_lin_vel", 3), ("root_ang_vel", 3), ("dof_pos", 12), ("dof_vel", 12), ("torques", 12), ("actions", 12),
                ("commands", 3), ("base_lin_vel", 3), ("base_ang_vel", 3), ("projected_gravity", 3), ("foot_pos", 12), ("foot_vel", 12), ("foot_force", 12),
                ("reward", 1), ("reset", 1), ("time_out", 1))
GO2NN_TRACE_WIDTH = sum(w for _, w in TRACE_BLOCKS)
TRACE_OFFSET = {name: sum(w for _, w in TRACE_BLOCKS[:i]) for i, (name, _) in enumerate(TRACE_BLOCKS)}
TRACE_FIELDS = ("root_states", "dof_state", "torques", "actions", "commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "rigid_body_states", "contact_forces",
                "rew_buf", "reset_buf", "time_out_buf")
# the black box (utils/recorder.py FallRecorder): the per-robot rows of its int32 state block [GO2NN_BLACKBOX_NUM * N + 1] in the order of the enum GO2NN_BLACKBOX_* of
# include/go2nn.h; the one step counter is the block's last int
BLACKBOX_ROWS = ("written", "frozen", "fall_step")
GO2NN_BLACKBOX_NUM = len(BLACKBOX_ROWS)
# the evaluator's perturbations: the rows of the table [GO2NN_ROBUST_NUM, N] in the order of the enum GO2NN_ROBUST_* of include/go2nn.h (per-env state first, then the
# accumulators go2nn_robust_reduce sums), the buffers of Go2nnRobustIn in the struct's order, and the mask bit of each writable dynamics row
ROBUST_ROWS = ("step", "open", "peak_err", "peak_tilt", "ok_run", "done", "pushes", "push_falls", "recovered", "recovery_steps", "peak_err_sum", "peak_tilt_sum")
GO2NN_ROBUST_NUM, GO2NN_ROBUST_ACC_FIRST, GO2NN_ROBUST_MAX_SPECS = len(ROBUST_ROWS), ROBUST_ROWS.index("pushes"), 64
GO2NN_ROBUST_ACC_NUM = GO2NN_ROBUST_NUM - GO2NN_ROBUST_ACC_FIRST
ROBUST_FIELDS = ("root_states", "commands", "base_lin_vel", "projected_gravity", "reset_buf", "time_out_buf", "motor_strengths", "p_gains_multiplier", "d_gains_multiplier",
                 "added_base_mass", "friction_coeffs")
ROBUST_MASK = {"strength": 1, "kp_mul": 2, "kd_mul": 4, "added_mass": 8, "friction": 16}
# the evaluator's terrain ladder: the rows of the table [GO2NN_LADDER_NUM, N], the columns of go2nn_ladder_reduce's output and the values of the STATE row, each in the
# order of its enum GO2NN_LADDER_* of include/go2nn.h, and the buffers of Go2nnLadderIn in the struct's order
LADDER_ROWS = ("step", "state", "x0", "y0", "max_d2", "clear_step")
LADDER_OUT = ("n", "cleared", "fell", "timed_out", "clear_steps", "progress")
LADDER_STATES = ("running", "cleared", "fell", "timed_out")
GO2NN_LADDER_NUM, GO2NN_LADDER_OUT_NUM = len(LADDER_ROWS), len(LADDER_OUT)
LADDER_FIELDS = ("root_states", "reset_buf", "time_out_buf")
# the evaluator's gait scores: the per-env rows of the table [GO2NN_GAIT_NUM, N], the rows of one foot (state first, then the accumulators go2nn_gait_reduce sums) and the
# per-foot columns of the reduce's output, each in the order of its enum GO2NN_GAIT_* of include/go2nn.h; the table is the env rows, then GAIT_FOOT_ROWS per foot; the output
# is "n", then GAIT_OUT_FOOT per foot, then support0 .. support4 and diagonal; and the buffers of Go2nnGaitIn in the struct's order
GAIT_ENV_ROWS = ("step", "used", "support0", "support1", "support2", "support3", "support4", "diagonal")
GAIT_FOOT_ROWS = ("prev", "phase_start", "last_td", "swing_max", "lift_z", "contact", "slip_sum", "touchdowns", "stride_steps", "strides", "stance_steps", "stances",
                  "swing_steps", "swings", "height_sum", "clearance_sum")
GAIT_OUT_FOOT = ("used",) + GAIT_FOOT_ROWS[GAIT_FOOT_ROWS.index("contact"):]
GO2NN_GAIT_FOOT0, GO2NN_GAIT_NUM = len(GAIT_ENV_ROWS), len(GAIT_ENV_ROWS) + 4 * len(GAIT_FOOT_ROWS)
GO2NN_GAIT_OUT_SUPPORT0 = 1 + 4 * len(GAIT_OUT_FOOT)
GO2NN_GAIT_OUT_DIAGONAL, GO2NN_GAIT_OUT_NUM = GO2NN_GAIT_OUT_SUPPORT0 + 5, GO2NN_GAIT_OUT_SUPPORT0 + 6
GAIT_FIELDS = ("rigid_body_states", "contact_forces", "reset_buf")
# the evaluator's asymmetry scores: the rows of the table [GO2NN_ASYM_NUM, N] in the order of the enum GO2NN_ASYM_* of include/go2nn.h (the last eight are the four
# (left, right) pairs ASYM_PAIRS); go2nn_asym_reduce's output is "n", every row but "step" (eq_max as the group's max), then per pair its imbalance sum and env count; and
# the buffers of Go2nnAsymIn in the struct's order
ASYM_ROWS = ("step", "eq_steps", "eq_sq", "eq_sq_hip", "eq_sq_thigh", "eq_sq_calf", "act_sq", "eq_max", "sym_steps", "act_sq_l", "act_sq_r", "torque_sq_l", "torque_sq_r",
             "power_l", "power_r", "contact_l", "contact_r")
ASYM_PAIRS = ("act_sq", "torque_sq", "power", "contact")
GO2NN_ASYM_NUM, GO2NN_ASYM_PAIR0 = len(ASYM_ROWS), ASYM_ROWS.index("act_sq_l")
ASYM_OUT = ("n",) + ASYM_ROWS[1:] + tuple("%s_%s" % (p, k) for p in ASYM_PAIRS for k in ("imb", "imb_n"))
GO2NN_ASYM_OUT_IMB0, GO2NN_ASYM_OUT_NUM = GO2NN_ASYM_NUM, len(ASYM_OUT)
ASYM_FIELDS = ("commands", "dof_state", "torques", "contact_forces", "reset_buf")
# the evaluator's action and torque spectra (GO2NN_SPECTRUM_* of include/go2nn.h): the trace [1 + 25 T, N] — the step row, then per counted step the actions and the torques
# of the 12 slots (joints in kind order) and the reset flag —, the table [2 + 12 K, N], K = W / 2 + 1 — used, skipped, then sum P and sum M per (signal, kind, bin) —, the
# reduce's output "n" + the table's rows; and the buffers of Go2nnSpectrumIn in the struct's order
SPECTRUM_FIELDS = ("actions", "torques", "reset_buf")
SPECTRUM_SIGNALS, SPECTRUM_KINDS = ("action", "torque"), ("hip", "thigh", "calf")
GO2NN_SPECTRUM_MIN_WINDOW, GO2NN_SPECTRUM_MAX_WINDOW, GO2NN_SPECTRUM_MAX_STEPS = 8, 256, 1 << 20
GO2NN_SPECTRUM_CHANNELS, GO2NN_SPECTRUM_CH_ACTION0, GO2NN_SPECTRUM_CH_TORQUE0, GO2NN_SPECTRUM_CH_RESET = 25, 0, 12, 24
GO2NN_SPECTRUM_USED, GO2NN_SPECTRUM_SKIPPED, GO2NN_SPECTRUM_BIN0 = 0, 1, 2
# the evaluator's actuator loads (GO2NN_ACTUATOR_* of include/go2nn.h): the per-robot rows of the table [GO2NN_ACTUATOR_NUM, N], the rows of one joint and of one foot, each in
# the order of its enum; the table is the robot rows, then ACTUATOR_JOINT_ROWS per joint, then ACTUATOR_FOOT_ROWS per foot; go2nn_actuator_reduce's output is "n", "n_used",
# then every table row but "step"; and the buffers of Go2nnActuatorIn in the struct's order
ACTUATOR_ENV_ROWS = ("step", "used", "dist")
ACTUATOR_JOINT_ROWS = ("tau_sq", "tau_peak", "tau_sat", "vel_peak", "vel_sat", "work_pos", "work_neg", "margin_min")
ACTUATOR_FOOT_ROWS = ("fz_peak", "fz_sum", "fz_frames")
GO2NN_ACTUATOR_JOINT0 = len(ACTUATOR_ENV_ROWS)
GO2NN_ACTUATOR_FOOT0 = GO2NN_ACTUATOR_JOINT0 + 12 * len(ACTUATOR_JOINT_ROWS)
GO2NN_ACTUATOR_NUM = GO2NN_ACTUATOR_FOOT0 + 4 * len(ACTUATOR_FOOT_ROWS)
GO2NN_ACTUATOR_OUT_N, GO2NN_ACTUATOR_OUT_N_USED, GO2NN_ACTUATOR_OUT_ROW0, GO2NN_ACTUATOR_OUT_NUM = 0, 1, 2, GO2NN_ACTUATOR_NUM + 1
ACTUATOR_FIELDS = ("dof_state", "torques", "contact_forces", "root_states", "reset_buf")


def actuator_row(name, index=None):
    """the table row of `name`: of ACTUATOR_ENV_ROWS, or of ACTUATOR_JOINT_ROWS for joint `index` (DOF order), or of ACTUATOR_FOOT_ROWS for foot `index` (foot_body order)"""
    if name in ACTUATOR_ENV_ROWS:
        return ACTUATOR_ENV_ROWS.index(name)
    if name in ACTUATOR_JOINT_ROWS:
        return GO2NN_ACTUATOR_JOINT0 + index * len(ACTUATOR_JOINT_ROWS) + ACTUATOR_JOINT_ROWS.index(name)
    return GO2NN_ACTUATOR_FOOT0 + index * len(ACTUATOR_FOOT_ROWS) + ACTUATOR_FOOT_ROWS.index(name)


def actuator_out_col(name, index=None):
    """the column of `name` in go2nn_actuator_reduce's output: "n", "n_used", or a table row's (actuator_row's arguments)"""
    return {"n": GO2NN_ACTUATOR_OUT_N, "n_used": GO2NN_ACTUATOR_OUT_N_USED}[name] if name in ("n", "n_used") else GO2NN_ACTUATOR_OUT_ROW0 + actuator_row(name, index) - 1


def spectrum_bins(W):
    return W // 2 + 1


def spectrum_trace_rows(T):
    return 1 + GO2NN_SPECTRUM_CHANNELS * T


def spectrum_rows(W):
    """the rows of the per-robot table; go2nn_spectrum_reduce's output has one more column in front (the group's robots)"""
    return GO2NN_SPECTRUM_BIN0 + 12 * spectrum_bins(W)


def spectrum_row(W, what, signal, kind, k=0):
    """the table row of bin k of `what` ("P" or "M") of SPECTRUM_SIGNALS[signal] x SPECTRUM_KINDS[kind]"""
    K = spectrum_bins(W)
    return GO2NN_SPECTRUM_BIN0 + (6 * K if what == "M" else 0) + (signal * 3 + kind) * K + k


def spectrum_twiddle(W):
    """float64 [W, 2]: (cos, sin)(2 pi n / W), what go2nn_spectrum_welch reads its rotations and its Hann weights from"""
    import numpy as np
    a = 2.0 * np.pi * np.arange(W, dtype=np.float64) / float(W)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], 1))
# the evaluator's command maneuvers: the rows of the table [GO2NN_MANEUVER_NUM, N] in the order of the enum GO2NN_MANEUVER_* of include/go2nn.h (per-env state first, then
# the accumulators go2nn_maneuver_reduce sums; its output columns are those plus "n"), and the buffers of Go2nnManeuverIn in the struct's order
MANEUVER_ROWS = ("step", "open", "ok_run", "is_settled", "is_fell", "peak_tilt", "switches", "switch_falls", "settled", "settle_steps", "win_steps", "win_lin_err",
                 "win_ang_err", "peak_tilt_sum")
GO2NN_MANEUVER_NUM, GO2NN_MANEUVER_ACC_FIRST, GO2NN_MANEUVER_MAX_SPECS, GO2NN_MANEUVER_MAX_SEGS = len(MANEUVER_ROWS), MANEUVER_ROWS.index("switches"), 64, 8
GO2NN_MANEUVER_ACC_NUM = GO2NN_MANEUVER_NUM - GO2NN_MANEUVER_ACC_FIRST
MANEUVER_OUT = MANEUVER_ROWS[GO2NN_MANEUVER_ACC_FIRST:] + ("n",)
MANEUVER_FIELDS = ("commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "reset_buf", "time_out_buf")
# the evaluator's sensor model: the values of Go2nnSensorIn.kind in the order of the enum GO2NN_SENSOR_* of include/go2nn.h (PASS: commands, previous actions — never delayed,
# dropped or biased), the fields of Go2nnSensorSpec in the struct's order, and the limits of the ring, the observation width and the number of conditions
SENSOR_KINDS = ("pass", "gyro", "gravity", "joint_pos", "joint_vel")
SENSOR_SPEC_FIELDS = ("noise_mul", "gyro_bias", "gravity_bias", "joint_offset", "delay", "drop")
GO2NN_SENSOR_MAX_DELAY, GO2NN_SENSOR_MAX_WIDTH, GO2NN_SENSOR_MAX_SPECS = 4, 64, 64
# the Go2 tasks' 45 observation columns (envs/go2/go2_env.py): angular velocity, projected gravity, commands, joint positions, joint velocities, previous actions — what the
# evaluator's sensor model and the training-time sensor randomisation (Go2nnSensorRand, fields in the struct's order below) both use as Go2nnSensorIn.kind
GO2_OBS_KINDS = ["gyro"] * 3 + ["gravity"] * 3 + ["pass"] * 3 + ["joint_pos"] * 12 + ["joint_vel"] * 12 + ["pass"] * 12
SENSOR_RAND_FIELDS = ("delay_lo", "delay_hi", "drop_lo", "drop_hi", "gyro_bias", "gravity_bias", "joint_offset", "env_offset")
_cached = None


class Go2nnSumJob(C.Structure):
    _fields_ = [("part", C.c_void_p), ("out", C.c_void_p), ("nrows", C.c_int32), ("ncols", C.c_int32), ("acc", C.c_void_p), ("nacc", C.c_int32), ("pad_", C.c_int32),
                ("out_w", C.c_int32), ("out_ld", C.c_int32)]          # ABI 6: out_w > 0: the sums go out as rows of out_w floats with pitch out_ld


class Go2nnFwdJob(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("M", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("act", C.c_int32),
                ("w_split", C.c_void_p)]          # ABI 4: the weight's split image (go2nn_split_weights) selects the 3 x bf16 kernel; None = fp32 MFMA.  ABI 5: act 1 = no activation


class Go2nnBwdInJob(C.Structure):
    _fields_ = [("gz", C.c_void_p), ("w", C.c_void_p), ("y_prev", C.c_void_p), ("gz_prev", C.c_void_p), ("workspace", C.c_void_p),
                ("M", C.c_int32), ("C", C.c_int32), ("Kin", C.c_int32), ("plain", C.c_int32), ("w_split", C.c_void_p), ("ld", C.c_int32),          # ABI 5: plain 1 = gz W only; ld = pitch of y_prev / gz_prev (0: Kin)
                ("Kx", C.c_int32), ("x_in", C.c_void_p), ("dw_workspace", C.c_void_p), ("ldx", C.c_int32)]          # ABI 6: x_in [M, Kx] = input of the layer below: its weight gradient's partials -> dw_workspace; gz_prev may be None


class Go2nnBwdWJob(C.Structure):
    _fields_ = [("gz", C.c_void_p), ("x", C.c_void_p), ("workspace", C.c_void_p), ("M", C.c_int32), ("C", C.c_int32), ("Kin", C.c_int32), ("split", C.c_int32), ("ldx", C.c_int32)]          # ABI 6: ldx = pitch of x (0: Kin)


class Go2nnSplitJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("image", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32)]


class Go2nnPpoHeads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("y_a", "y_c", "w_mu", "b_mu", "w_v", "b_v", "std", "actions", "old_mu", "old_sigma", "old_logp", "adv", "old_values", "returns",
                                          "gz_a", "gz_c", "partials")] + [(k, C.c_int32) for k in ("B", "A", "K", "use_clipped_value_loss")] + \
               [(k, C.c_float) for k in ("clip", "value_loss_coef", "entropy_coef")] + [("surrogate_split", C.c_int32)]          # ABI 5: CTS' teacher rows (0: plain PPO)


class Go2nnMlpIO(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x2", C.c_void_p), ("rows", C.c_void_p), ("y", C.c_void_p)] + [(k, C.c_int32) for k in ("ldx", "ldx2", "kx", "nrows", "ldy", "normalize")]


class Go2nnMlp(C.Structure):
    _fields_ = [("num_layers", C.c_int32), ("dims", C.c_int32 * (GO2NN_MAX_LAYERS + 1)),
                ("weight", C.c_void_p * GO2NN_MAX_LAYERS), ("bias", C.c_void_p * GO2NN_MAX_LAYERS)]


class Go2nnRnnCellJob(C.Structure):          # ABI 7
    _fields_ = [(k, C.c_void_p) for k in ("gi", "gh", "h_prev", "c_prev", "h", "c", "gates", "save_h", "save_c", "done", "sub_h", "sub_c", "next_h", "next_c")] + \
               [(k, C.c_int32) for k in ("B", "H", "type", "pad_")]


class Go2nnRnnCellBwdJob(C.Structure):       # ABI 7
    _fields_ = [(k, C.c_void_p) for k in ("gates", "c", "c_prev", "h_prev", "dy", "dh_rec", "dh_carry", "dc", "done", "dgi", "dgh")] + \
               [(k, C.c_int32) for k in ("B", "H", "type", "pad_")]


class Go2nnEvalField(C.Structure):          # (within ABI 7) strides in elements
    _fields_ = [("p", C.c_void_p), ("env_stride", C.c_int32), ("comp_stride", C.c_int32)]


class Go2nnEvalIn(C.Structure):
    _fields_ = [(k, Go2nnEvalField) for k in EVAL_FIELDS] + [("dof_limits", C.c_void_p), ("dof_vel_offset", C.c_int32), ("dt", C.c_float)]


class Go2nnTraceIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in TRACE_FIELDS] + [("dof_vel_offset", C.c_int32), ("rigid_body_stride", C.c_int32), ("contact_body_stride", C.c_int32),
                                                              ("foot_body", C.c_int32 * 4), ("pad_", C.c_int32)]


class Go2nnRobustSpec(C.Structure):          # (within ABI 7)
    _fields_ = [("dv", C.c_float * 3), ("first", C.c_int32), ("period", C.c_int32), ("count", C.c_int32), ("window", C.c_int32), ("hold", C.c_int32), ("thr", C.c_float),
                ("strength", C.c_float), ("kp_mul", C.c_float), ("kd_mul", C.c_float), ("added_mass", C.c_float), ("friction", C.c_float), ("mask", C.c_int32), ("pad_", C.c_int32)]


class Go2nnRobustIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in ROBUST_FIELDS] + [("num_specs", C.c_int32), ("pad_", C.c_int32)]


class Go2nnLadderIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in LADDER_FIELDS] + [("dist2_thr", C.c_float), ("pad_", C.c_int32)]


class Go2nnGaitIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in GAIT_FIELDS] + [("rigid_body_stride", C.c_int32), ("contact_body_stride", C.c_int32), ("foot_body", C.c_int32 * 4),
                                                             ("contact_threshold", C.c_float), ("diagonal_mask", C.c_int32 * 2), ("pad_", C.c_int32)]


class Go2nnAsymIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in ASYM_FIELDS] + [("dof_vel_offset", C.c_int32), ("contact_body_stride", C.c_int32), ("foot_body", C.c_int32 * 4),
                                                             ("foot_side", C.c_int32 * 4), ("joint_side", C.c_int32 * 12), ("joint_kind", C.c_int32 * 12),
                                                             ("action_perm", C.c_int16 * 12), ("action_sign", C.c_float * 12), ("contact_threshold", C.c_float),
                                                             ("pad_", C.c_int32)]


class Go2nnSpectrumIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in SPECTRUM_FIELDS] + [("joint_of_slot", C.c_int32 * 12)]


class Go2nnActuatorIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in ACTUATOR_FIELDS] + [("dof_vel_offset", C.c_int32), ("contact_body_stride", C.c_int32), ("foot_body", C.c_int32 * 4),
                                                                 ("pos_lo", C.c_float * 12), ("pos_hi", C.c_float * 12), ("tau_sat_thr", C.c_float * 12),
                                                                 ("vel_sat_thr", C.c_float * 12), ("contact_threshold", C.c_float), ("pad_", C.c_int32)]


def gait_row(foot, name):
    """the table row of `name` (GAIT_FOOT_ROWS) of foot `foot` (in foot_body order)"""
    return GO2NN_GAIT_FOOT0 + foot * len(GAIT_FOOT_ROWS) + GAIT_FOOT_ROWS.index(name)


def gait_out_col(foot, name):
    """the column of `name` (GAIT_OUT_FOOT) of foot `foot` in go2nn_gait_reduce's output"""
    return 1 + foot * len(GAIT_OUT_FOOT) + GAIT_OUT_FOOT.index(name)


class Go2nnManeuverSpec(C.Structure):          # (within ABI 7)
    _fields_ = [("count", C.c_int32), ("window", C.c_int32), ("hold", C.c_int32), ("thr_lin", C.c_float), ("thr_ang", C.c_float),
                ("start", C.c_int32 * GO2NN_MANEUVER_MAX_SEGS), ("cmd", (C.c_float * 3) * GO2NN_MANEUVER_MAX_SEGS)]


class Go2nnManeuverIn(C.Structure):          # (within ABI 7)
    _fields_ = [(k, Go2nnEvalField) for k in MANEUVER_FIELDS] + [("num_specs", C.c_int32), ("num_commands", C.c_int32)]


class Go2nnSensorSpec(C.Structure):          # (within ABI 7)
    _fields_ = [("noise_mul", C.c_float), ("gyro_bias", C.c_float), ("gravity_bias", C.c_float), ("joint_offset", C.c_float), ("delay", C.c_int32), ("drop", C.c_float),
                ("pad_", C.c_int32 * 2)]


class Go2nnSensorIn(C.Structure):          # (within ABI 7)
    _fields_ = [("obs", Go2nnEvalField), ("dones", C.c_void_p), ("scale", C.c_void_p), ("kind", C.c_void_p), ("D", C.c_int32), ("num_specs", C.c_int32), ("clip", C.c_float),
                ("seed", C.c_uint32)]


class Go2nnSensorRand(C.Structure):          # (within ABI 7)
    _fields_ = [("delay_lo", C.c_int32), ("delay_hi", C.c_int32), ("drop_lo", C.c_float), ("drop_hi", C.c_float), ("gyro_bias", C.c_float), ("gravity_bias", C.c_float),
                ("joint_offset", C.c_float), ("env_offset", C.c_uint32)]


class Go2nnMirrorJob(C.Structure):          # (within ABI 7) perm and sign None: both halves of dst are copies
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int32), ("perm", C.c_void_p), ("sign", C.c_void_p)]


GO2NN_MIRROR_MAX_JOBS = 16


class Go2nnMirrorLoss(C.Structure):          # (within ABI 7) perm and sign None: the identity table
    _fields_ = [("y_a", C.c_void_p), ("w_mu", C.c_void_p), ("b_mu", C.c_void_p), ("perm", C.c_void_p), ("sign", C.c_void_p), ("gz_a", C.c_void_p), ("partials", C.c_void_p),
                ("B", C.c_int32), ("A", C.c_int32), ("K", C.c_int32), ("coef", C.c_float)]


class Go2nnSmoothLoss(C.Structure):          # (within ABI 7) rows in block layout: r = b T n + t n + j
    _fields_ = [("y_a", C.c_void_p), ("w_mu", C.c_void_p), ("b_mu", C.c_void_p), ("w", C.c_void_p), ("gz_a", C.c_void_p), ("partials", C.c_void_p),
                ("blocks", C.c_int32), ("T", C.c_int32), ("n", C.c_int32), ("A", C.c_int32), ("K", C.c_int32), ("coef", C.c_float)]


# the update's diagnostics: the columns of a table row in the order of the enum GO2NN_DIAG_* of include/go2nn.h (where the definitions are)
DIAG_COLS = ("rows", "ratio_clipped", "ratio_sum", "logratio_sum", "k3_sum", "kl_sum", "kl_max", "adv_sum", "adv_sq", "adv_pos", "verr_sum", "verr_sq", "verr_abs_max",
             "ret_sum", "ret_sq", "value_clipped", "ratio_max", "ratio_min")
GO2NN_DIAG_NUM = len(DIAG_COLS)
DIAG_MAX_COLS, DIAG_MIN_COLS = ("kl_max", "verr_abs_max", "ratio_max"), ("ratio_min",)          # every other column is a sum
GO2NN_GRAD_SQNORM_MAX = 48


class Go2nnPpoDiag(C.Structure):          # (within ABI 7) the inputs of Go2nnPpoHeads, read only
    _fields_ = [(k, C.c_void_p) for k in ("y_a", "y_c", "w_mu", "b_mu", "w_v", "b_v", "std", "actions", "old_mu", "old_sigma", "old_logp", "adv", "old_values", "returns",
                                          "partials", "table", "cursor")] + [(k, C.c_int32) for k in ("B", "A", "K", "surrogate_split", "slots")] + [("clip", C.c_float)]


def mirror_loss_table_tensors(lib, table, device):
    """The action table of the mirror loss — an involution with sign[perm[j]] == sign[j] —, checked on the host (go2nn_mirror_loss_check_table) and uploaded
    -> (int16 tensor [A], float32 tensor [A]) on `device`"""
    import numpy as np
    perm, sign = np.ascontiguousarray(table[0], np.int16), np.ascontiguousarray(table[1], np.float32)
    if perm.ndim != 1 or perm.shape != sign.shape:
        raise ValueError("a mirror table is a pair of 1-d arrays of one length, got shapes %s and %s" % (perm.shape, sign.shape))
    if lib.go2nn_mirror_loss_check_table(perm.ctypes.data, sign.ctypes.data, perm.shape[0]) != 0:
        raise ValueError(lib.go2nn_last_error().decode())
    return torch.from_numpy(perm).to(device), torch.from_numpy(sign).to(device)


def mirror_table_tensors(lib, table, device):
    """A (perm, sign) table of utils/symmetry.py, checked on the host (go2nn_mirror_check_table: the launch cannot report a bad index) and uploaded
    -> (int16 tensor [W], float32 tensor [W]) on `device`"""
    import numpy as np
    perm, sign = np.ascontiguousarray(table[0], np.int16), np.ascontiguousarray(table[1], np.float32)
    if perm.ndim != 1 or perm.shape != sign.shape:
        raise ValueError("a mirror table is a pair of 1-d arrays of one length, got shapes %s and %s" % (perm.shape, sign.shape))
    if lib.go2nn_mirror_check_table(perm.ctypes.data, sign.ctypes.data, perm.shape[0]) != 0:
        raise ValueError(lib.go2nn_last_error().decode())
    return torch.from_numpy(perm).to(device), torch.from_numpy(sign).to(device)


def mirror_jobs(pairs):
    """pairs: (src [chunks * chunk_rows, ...], dst [chunks, 2 * chunk_rows, ...], (perm tensor, sign tensor) or None) -> the ctypes job array of go2nn_mirror_rows"""
    jobs = []
    for src, dst, tab in pairs:
        width = int(src[0].numel()) if src.dim() > 1 else 1
        for t in (src, dst) + (tuple(tab) if tab is not None else ()):
            assert t.is_contiguous() and t.device == src.device, "contiguous tensors on one device"
        assert src.dtype == dst.dtype == torch.float32 and dst.numel() == 2 * src.numel() and src.data_ptr() != dst.data_ptr()
        assert tab is None or (tab[0].dtype == torch.int16 and tab[1].dtype == torch.float32 and tab[0].numel() == tab[1].numel() == width), "a table of the rows' width"
        jobs.append(Go2nnMirrorJob(src.data_ptr(), dst.data_ptr(), width, tab[0].data_ptr() if tab is not None else None, tab[1].data_ptr() if tab is not None else None))
    return (Go2nnMirrorJob * len(jobs))(*jobs)


def mirror_rows(lib, jobs, chunks, chunk_rows, stream=None):
    if lib.go2nn_mirror_rows(jobs, len(jobs), int(chunks), int(chunk_rows), stream) != 0:
        raise RuntimeError("go2nn_mirror_rows failed: %s" % lib.go2nn_last_error().decode())


class Go2nnObsNormJob(C.Structure):          # (within ABI 7) y may be x; partials None: normalise only
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("inv", C.c_void_p), ("partials", C.c_void_p), ("D", C.c_int32), ("clip", C.c_float)]


GO2NN_OBS_NORM_MAX_JOBS = 4


def obs_norm_jobs(items):
    """items: (x [N, D], y [N, D] (may be x), mean32 [D], inv32 [D], partials fp64 [partial_rows(N), D, 2] or None, clip) -> the ctypes job array of go2nn_obs_norm_apply"""
    jobs = []
    for x, y, mean, inv, partials, clip in items:
        D = int(x.shape[-1])
        for t in (x, y, mean, inv):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == x.device, "contiguous fp32 tensors on one device"
        assert x.dim() == 2 and y.shape == x.shape and mean.numel() == inv.numel() == D, "x and y [N, D], mean and inv [D]"
        if partials is not None:
            assert partials.is_contiguous() and partials.dtype == torch.float64 and partials.device == x.device and partials.numel() == -(-x.shape[0] // 64) * D * 2, \
                "partials: fp64 [partial_rows(N), D, 2]"
        jobs.append(Go2nnObsNormJob(x.data_ptr(), y.data_ptr(), mean.data_ptr(), inv.data_ptr(), partials.data_ptr() if partials is not None else None, D, float(clip)))
    return (Go2nnObsNormJob * len(jobs))(*jobs)


def obs_norm_apply(lib, jobs, N, stream=None):
    if lib.go2nn_obs_norm_apply(jobs, len(jobs), int(N), stream) != 0:
        raise RuntimeError("go2nn_obs_norm_apply failed: %s" % lib.go2nn_last_error().decode())


def obs_norm_update(lib, table, state, n, eps, mean32, inv32, stream=None):
    """table fp64 [steps, rows, D, 2], state fp64 [1 + 2 D]: the iteration's moments merged into the state, mean32 / inv32 rewritten (go2nn_obs_norm_update)"""
    steps, rows, D = (int(v) for v in table.shape[:3])
    assert table.is_contiguous() and table.dtype == state.dtype == torch.float64 and state.numel() == 1 + 2 * D and mean32.numel() == inv32.numel() == D
    if lib.go2nn_obs_norm_update(table.data_ptr(), steps, rows, D, state.data_ptr(), float(n), float(eps), mean32.data_ptr(), inv32.data_ptr(), stream) != 0:
        raise RuntimeError("go2nn_obs_norm_update failed: %s" % lib.go2nn_last_error().decode())


GO2NN_VALUE_NORM_ROWS = 1024          # include/go2nn.h: elements per block of go2nn_value_norm_apply = per row of its partial table


def value_norm_apply(lib, values, returns, stat32, partials=None, stream=None):
    """values, returns: fp32 views of n contiguous floats each, normalised in place by stat32 = mean32 | std32 | inv32; partials fp64 [partial_rows(n), 2] or None
    (go2nn_value_norm_apply)"""
    n = int(values.numel())
    for t in (values, returns, stat32):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.device == values.device, "contiguous fp32 tensors on one device"
    assert returns.numel() == n and stat32.numel() == 3
    if partials is not None:
        assert partials.is_contiguous() and partials.dtype == torch.float64 and partials.device == values.device and partials.numel() == -(-n // GO2NN_VALUE_NORM_ROWS) * 2, \
            "partials: fp64 [partial_rows(n), 2]"
    if lib.go2nn_value_norm_apply(values.data_ptr(), returns.data_ptr(), n, stat32.data_ptr(), partials.data_ptr() if partials is not None else None, stream) != 0:
        raise RuntimeError("go2nn_value_norm_apply failed: %s" % lib.go2nn_last_error().decode())


def value_norm_update(lib, partials, state, n, eps, stat32, w_last=None, b_last=None, stream=None):
    """partials fp64 [rows, 2] merged into state fp64 [3] = count | mean | M2, stat32 rewritten; w_last [1, K] / b_last [1] (the critic's last layer): output preservation
    (go2nn_value_norm_update)"""
    assert partials.is_contiguous() and partials.dtype == state.dtype == torch.float64 and state.numel() == 3 and stat32.numel() == 3 and stat32.dtype == torch.float32
    K = 0
    if w_last is not None:
        assert w_last.is_contiguous() and b_last.is_contiguous() and w_last.dtype == b_last.dtype == torch.float32 and b_last.numel() == 1 and w_last.shape[0] == 1
        K = int(w_last.numel())
    if lib.go2nn_value_norm_update(partials.data_ptr(), int(partials.numel() // 2), state.data_ptr(), float(n), float(eps), stat32.data_ptr(),
                                   w_last.data_ptr() if w_last is not None else None, b_last.data_ptr() if w_last is not None else None, K, stream) != 0:
        raise RuntimeError("go2nn_value_norm_update failed: %s" % lib.go2nn_last_error().decode())


def value_head_fold(lib, w, b, stat32, w_out, b_out, stream=None):
    """(w [1, K], b [1]) of a critic's last layer -> (w std32, b std32 + mean32) in the scratch pair (go2nn_value_head_fold)"""
    K = int(w.numel())
    for t in (w, b, stat32, w_out, b_out):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.device == w.device
    assert b.numel() == 1 and w_out.numel() == K and b_out.numel() == 1 and stat32.numel() == 3
    if lib.go2nn_value_head_fold(w.data_ptr(), b.data_ptr(), K, stat32.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), stream) != 0:
        raise RuntimeError("go2nn_value_head_fold failed: %s" % lib.go2nn_last_error().decode())


def trace_env_ids(env_ids, num_envs):
    """the tracked robots of go2nn_trace_record as the kernel needs them -> int32 numpy [K], strictly increasing, each in [0, num_envs).  The kernel cannot report a bad
    index (it would read outside the buffers), so anything else raises here."""
    import numpy as np
    ids = env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else np.asarray(env_ids)
    if ids.ndim != 1 or ids.size < 1 or ids.dtype.kind not in "iu":
        raise ValueError("env_ids: a non-empty 1-d sequence of integers is needed, got %r" % (env_ids,))
    ids = ids.astype(np.int64)
    if ids.min() < 0 or ids.max() >= int(num_envs):
        raise ValueError("env_ids outside [0, %d): %s" % (num_envs, ids.tolist()))
    if (np.diff(ids) <= 0).any():
        raise ValueError("env_ids must be strictly increasing: %s" % ids.tolist())
    return np.ascontiguousarray(ids, np.int32)


def bind(path):
    lib = C.CDLL(path)
    lib.go2nn_last_error.restype = C.c_char_p
    lib.go2nn_packed_floats.restype = C.c_int64
    lib.go2nn_packed_floats.argtypes = [C.POINTER(Go2nnMlp)]
    lib.go2nn_pack.argtypes = [C.POINTER(Go2nnMlp), C.c_void_p, C.c_void_p]
    lib.go2nn_mlp_arith.argtypes = [C.POINTER(Go2nnMlp)]
    lib.go2nn_mlp_forward.argtypes = [C.POINTER(Go2nnMlp), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_policy_act.argtypes = [C.POINTER(Go2nnMlp), C.c_void_p, C.POINTER(Go2nnMlp), C.c_void_p] + [C.c_void_p] * 10 + [C.c_int32, C.c_void_p]
    lib.go2nn_mlp_forward_rows.argtypes = [C.POINTER(C.POINTER(Go2nnMlp)), C.POINTER(C.c_void_p), C.POINTER(Go2nnMlpIO), C.c_int32, C.c_void_p]
    lib.go2nn_policy_act_latent.argtypes = [C.POINTER(Go2nnMlp), C.c_void_p, C.POINTER(Go2nnMlp), C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 10 + [C.c_int32, C.c_void_p]
    lib.go2nn_head_backward_workspace.restype = C.c_int64
    lib.go2nn_head_backward_workspace.argtypes = [C.c_int32] * 3
    lib.go2nn_head_backward.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p]
    lib.go2nn_linear_elu_forward.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]
    lib.go2nn_linear_backward_workspace.restype = C.c_int64
    lib.go2nn_linear_backward_workspace.argtypes = [C.c_int32] * 3
    lib.go2nn_linear_backward_input.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p]
    lib.go2nn_linear_backward_weight.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]
    lib.go2nn_sum_rows.argtypes = [C.POINTER(Go2nnSumJob), C.c_int32, C.c_void_p]
    lib.go2nn_head_backward_rows.argtypes = [C.c_int32] * 3
    lib.go2nn_linear_backward_input_rows.argtypes = [C.c_int32] * 3
    lib.go2nn_linear_elu_forward_group.argtypes = [C.POINTER(Go2nnFwdJob), C.c_int32, C.c_void_p]
    lib.go2nn_linear_backward_input_group_rows.argtypes = [C.c_int32] * 3
    lib.go2nn_linear_backward_input_group.argtypes = [C.POINTER(Go2nnBwdInJob), C.c_int32, C.c_void_p]
    lib.go2nn_linear_backward_input_fused_rows.argtypes = [C.c_int32]
    lib.go2nn_linear_backward_weight_group_rows.argtypes = [C.POINTER(Go2nnBwdWJob), C.c_int32]
    lib.go2nn_linear_backward_weight_group.argtypes = [C.POINTER(Go2nnBwdWJob), C.c_int32, C.c_void_p]
    lib.go2nn_linear_group_tile_rows.argtypes = [C.c_int32] * 4          # (within ABI 7) which kernel a shape gets: 64 / 128 / 192 rows per tile; 0 on the host build
    lib.go2nn_linear_backward_weight_group_kernel.argtypes = [C.POINTER(Go2nnBwdWJob), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]          # -> GO2NN_WGRAD_*
    lib.go2nn_split_weights_bytes.restype = C.c_int64
    lib.go2nn_split_weights_bytes.argtypes = [C.c_int32] * 2
    lib.go2nn_split_weights.argtypes = [C.POINTER(Go2nnSplitJob), C.c_int32, C.c_void_p]
    lib.go2nn_ppo_heads_rows.argtypes = [C.c_int32] * 3
    lib.go2nn_ppo_heads_cols.argtypes = [C.c_int32] * 2
    lib.go2nn_ppo_heads.argtypes = [C.POINTER(Go2nnPpoHeads), C.c_void_p]
    lib.go2nn_l2norm_backward_rows.argtypes = [C.c_int32]
    lib.go2nn_latent_concat.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_l2norm_backward.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_latent_mse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    lib.go2nn_moe_usage.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_moe_mix_loss.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.go2nn_moe_mix_forward.argtypes = [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p]
    lib.go2nn_rnn_cell_forward.argtypes = [C.POINTER(Go2nnRnnCellJob), C.c_int32, C.c_void_p]
    lib.go2nn_rnn_cell_backward.argtypes = [C.POINTER(Go2nnRnnCellBwdJob), C.c_int32, C.c_void_p]
    lib.go2nn_rnn_reset.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_eval_clear.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_eval_accumulate.argtypes = [C.POINTER(Go2nnEvalIn), C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_eval_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_trace_record.argtypes = [C.POINTER(Go2nnTraceIn), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_trace_clear.argtypes = [C.c_void_p, C.c_void_p]
    lib.go2nn_blackbox_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_blackbox_record.argtypes = [C.POINTER(Go2nnTraceIn), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_robust_check_specs.argtypes = [C.c_void_p, C.c_int32]
    lib.go2nn_robust_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_robust_apply.argtypes = [C.POINTER(Go2nnRobustIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_robust_accumulate.argtypes = [C.POINTER(Go2nnRobustIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_robust_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_ladder_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_ladder_accumulate.argtypes = [C.POINTER(Go2nnLadderIn), C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_ladder_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.go2nn_gait_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_gait_accumulate.argtypes = [C.POINTER(Go2nnGaitIn), C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_gait_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_asym_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_asym_accumulate.argtypes = [C.POINTER(Go2nnAsymIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_asym_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_spectrum_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]          # (within ABI 7) the evaluator's action and torque spectra
    lib.go2nn_spectrum_record.argtypes = [C.POINTER(Go2nnSpectrumIn), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_spectrum_welch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.go2nn_spectrum_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_eval_bootstrap_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]          # (within ABI 7) the cells' member lists, in host memory
    lib.go2nn_eval_bootstrap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.go2nn_actuator_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]          # (within ABI 7) the evaluator's actuator loads
    lib.go2nn_actuator_accumulate.argtypes = [C.POINTER(Go2nnActuatorIn), C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_actuator_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    for fam in ("robust", "maneuver", "gait", "asym", "actuator"):          # (within ABI 7) the same replicates of every scoring family's reduce table
        getattr(lib, "go2nn_%s_bootstrap" % fam).argtypes = lib.go2nn_eval_bootstrap.argtypes
    lib.go2nn_ladder_bootstrap.argtypes = lib.go2nn_eval_bootstrap.argtypes[:7] + [C.c_float, C.c_void_p, C.c_void_p]
    lib.go2nn_maneuver_check_specs.argtypes = [C.c_void_p, C.c_int32]
    lib.go2nn_maneuver_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_maneuver_apply.argtypes = [C.POINTER(Go2nnManeuverIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_maneuver_accumulate.argtypes = [C.POINTER(Go2nnManeuverIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_maneuver_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_sensor_check_specs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    lib.go2nn_sensor_state_bytes.restype = C.c_int64
    lib.go2nn_sensor_state_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.go2nn_sensor_begin.argtypes = [C.c_void_p, C.c_void_p]
    lib.go2nn_sensor_apply.argtypes = [C.POINTER(Go2nnSensorIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_sensor_rand_check.argtypes = [C.POINTER(Go2nnSensorRand), C.c_void_p, C.c_int32]
    lib.go2nn_sensor_rand_state_bytes.restype = C.c_int64
    lib.go2nn_sensor_rand_state_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.go2nn_sensor_rand_begin.argtypes = [C.c_void_p, C.c_void_p]
    lib.go2nn_sensor_rand_apply.argtypes = [C.POINTER(Go2nnSensorIn), C.POINTER(Go2nnSensorRand), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_mirror_check_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.go2nn_mirror_rows.argtypes = [C.POINTER(Go2nnMirrorJob), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_mirror_loss_rows.argtypes = [C.c_int32] * 3
    lib.go2nn_mirror_loss_cols.argtypes = [C.c_int32] * 2
    lib.go2nn_mirror_loss_check_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.go2nn_mirror_loss.argtypes = [C.POINTER(Go2nnMirrorLoss), C.c_void_p]
    lib.go2nn_smooth_loss_rows.argtypes = [C.c_int32] * 5          # (within ABI 7) the temporal action-smoothness loss on env-block mini-batches
    lib.go2nn_smooth_loss_cols.argtypes = [C.c_int32] * 2
    lib.go2nn_smooth_loss_set_segments.argtypes = [C.c_int32]
    lib.go2nn_smooth_loss.argtypes = [C.POINTER(Go2nnSmoothLoss), C.c_void_p]
    lib.go2nn_smooth_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.go2nn_ppo_diag_rows.argtypes = [C.c_int32] * 3          # (within ABI 7) the update's diagnostics
    lib.go2nn_ppo_diag.argtypes = [C.POINTER(Go2nnPpoDiag), C.c_void_p]
    lib.go2nn_grad_sqnorm_rows.argtypes = [C.c_void_p, C.c_int32]
    lib.go2nn_grad_sqnorm.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_obs_norm_partial_rows.argtypes = [C.c_int32]          # (within ABI 7) empirical observation normalisation
    lib.go2nn_obs_norm_apply.argtypes = [C.POINTER(Go2nnObsNormJob), C.c_int32, C.c_int32, C.c_void_p]
    lib.go2nn_obs_norm_update.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.go2nn_value_norm_partial_rows.argtypes = [C.c_int32]          # (within ABI 7) value normalisation
    lib.go2nn_value_norm_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.go2nn_value_norm_update.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.go2nn_value_head_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if lib.go2nn_abi_version() != GO2NN_ABI_VERSION:
        raise RuntimeError("%s: ABI version %d, expected %d" % (path, lib.go2nn_abi_version(), GO2NN_ABI_VERSION))
    return lib


def load_nn():
    global _cached
    if _cached is None:
        if not os.path.exists(NN_LIB):
            raise RuntimeError("%s is missing: build it with `python -m go2_rl_gym_amd.build` (hipcc --offload-arch=gfx950). There is no CPU fallback." % NN_LIB)
        torch.cuda.is_available()            # torch's HIP runtime first (see _lib.py)
        lib = bind(NN_LIB)
        if lib.go2nn_is_device_library() != 1:
            raise RuntimeError("%s is not the HIP device library" % NN_LIB)
        _cached = lib
    return _cached


def mlp_layers(seq):
    """[(weight, bias)] of an nn.Sequential that is Linear, ELU(alpha=1), ..., Linear (rsl_rl/modules/actor_critic.py:_mlp), else None."""
    mods = list(seq)
    if len(mods) % 2 != 1:
        return None
    out = []
    for k, m in enumerate(mods):
        if k % 2 == 0:
            if not isinstance(m, nn.Linear) or m.bias is None or m.weight.dtype != torch.float32:
                return None
            out.append((m.weight, m.bias))
        elif not (isinstance(m, nn.ELU) and m.alpha == 1.0):
            return None
    dims = [out[0][0].shape[1]] + [w.shape[0] for w, _ in out]
    if len(out) > GO2NN_MAX_LAYERS or max(dims) > GO2NN_MAX_WIDTH:
        return None
    return out


class PackedMlp:
    """One MLP's parameters as the kernels read them: the Go2nnMlp descriptor (pointers to the LIVE parameter tensors) and the packed operand
    buffer, refreshed by pack() — one small launch — whenever the parameters have changed (once per rollout: they only change in update())."""

    def __init__(self, lib, seq, linears=None, fold=None):
        """seq: an nn.Sequential of Linear / ELU; or linears: the Linear modules of such a stack (wherever they live: nested containers, a normaliser behind them).
        fold: the fp32 [3] stat32 of a ValueNormalization (modules/normalizer.py) — the scalar last layer is read from a scratch pair (W std32, b std32 + mean32) that
        pack() refills from the live parameters and stat32 with ONE go2nn_value_head_fold launch in front of go2nn_pack: the kernels answer in raw units"""
        layers = mlp_layers(seq) if linears is None else [(m.weight, m.bias) for m in linears]
        if layers is not None and (len(layers) > GO2NN_MAX_LAYERS or max([layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]) > GO2NN_MAX_WIDTH):
            layers = None
        if layers is None:
            raise ValueError("not a Linear/ELU MLP the kernel supports")
        self.lib, self.layers = lib, layers
        self.desc = Go2nnMlp()
        self.desc.num_layers = len(layers)
        self.desc.dims[0] = layers[0][0].shape[1]
        for l, (w, b) in enumerate(layers):
            assert w.is_contiguous() and b.is_contiguous()
            self.desc.dims[l + 1] = w.shape[0]
            self.desc.weight[l], self.desc.bias[l] = w.data_ptr(), b.data_ptr()
        self._live = [(w.data_ptr(), b.data_ptr()) for w, b in layers]
        self.fold = None
        if fold is not None:
            w, b = layers[-1]
            if w.shape[0] != 1 or fold.numel() != 3 or fold.dtype != torch.float32 or fold.device != w.device:
                raise ValueError("a folded last layer: a scalar output and an fp32 [3] stat32 on the parameters' device")
            self.fold = (fold, torch.zeros_like(w), torch.zeros_like(b))
            self.desc.weight[len(layers) - 1], self.desc.bias[len(layers) - 1] = self.fold[1].data_ptr(), self.fold[2].data_ptr()
        n = lib.go2nn_packed_floats(C.byref(self.desc))
        if n <= 0:
            raise ValueError(lib.go2nn_last_error().decode())
        self.packed = torch.zeros(int(n), dtype=torch.float32, device=layers[0][0].device)
        self.in_dim, self.out_dim = int(self.desc.dims[0]), int(self.desc.dims[len(layers)])
        self.arith = int(lib.go2nn_mlp_arith(C.byref(self.desc)))          # 3: split-operand kernel, 1: fp32-MFMA kernel, 0: the host test build (include/go2nn.h)

    def _stream(self):
        d = self.packed.device
        return C.c_void_p(torch.cuda.current_stream(d).cuda_stream) if d.type == "cuda" else None

    def still_valid(self):
        return all(self._live[l] == (w.data_ptr(), b.data_ptr()) for l, (w, b) in enumerate(self.layers))          # (the LIVE parameters, also of a folded last layer)

    def pack(self):
        if not self.still_valid():
            raise RuntimeError("the MLP's parameter tensors were re-allocated after the policy kernel was built (rebuild PolicyKernel)")
        if self.fold is not None:
            w, b = self.layers[-1]
            value_head_fold(self.lib, w.detach(), b.detach(), self.fold[0], self.fold[1], self.fold[2], self._stream())
        rc = self.lib.go2nn_pack(C.byref(self.desc), C.c_void_p(self.packed.data_ptr()), self._stream())
        if rc != 0:
            raise RuntimeError("go2nn_pack failed: %s" % self.lib.go2nn_last_error().decode())

    def forward(self, x):
        x = x.detach().contiguous().float()
        y = torch.empty(x.shape[0], self.out_dim, dtype=torch.float32, device=x.device)
        rc = self.lib.go2nn_mlp_forward(C.byref(self.desc), C.c_void_p(self.packed.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), x.shape[0], self._stream())
        if rc != 0:
            raise RuntimeError("go2nn_mlp_forward failed: %s" % self.lib.go2nn_last_error().decode())
        return y


class PolicyKernel:
    """PPO.act (rsl_rl/algorithms/ppo.py:90-102) for an ActorCritic of two Linear/ELU MLPs and a state-independent std, as one launch."""

    def __init__(self, lib, actor_critic, value_fold=None):
        """value_fold: stat32 of the value normaliser — the critic's packed weights answer in raw units (PackedMlp(fold=...))"""
        self.lib, self.ac = lib, actor_critic
        self.actor, self.critic = PackedMlp(lib, actor_critic.actor), PackedMlp(lib, actor_critic.critic, fold=value_fold)
        if self.actor.out_dim > 32 or self.critic.out_dim != 1:
            raise ValueError("head: up to 32 actions and a scalar value")

    @staticmethod
    def supports(actor_critic):
        if not (hasattr(actor_critic, "actor") and hasattr(actor_critic, "critic") and hasattr(actor_critic, "std") and actor_critic.std.dim() == 1):
            return False
        la, lc = mlp_layers(actor_critic.actor), mlp_layers(actor_critic.critic)
        # the head of go2nn_policy_act: up to 32 actions, a scalar value (the loss head go2sim_ppo_loss takes up to 16 actions; every go2 task has 12)
        return la is not None and lc is not None and la[-1][0].shape[0] <= 32 and lc[-1][0].shape[0] == 1 and actor_critic.std.shape[0] == la[-1][0].shape[0]

    def pack(self):
        self.actor.pack(); self.critic.pack()

    def act(self, obs, critic_obs, eps, a_st=None, mu_st=None, sig_st=None, lp_st=None, v_st=None):
        """-> actions [N, A]; the *_st tensors (storage rows of this step) are filled in place"""
        N, A = obs.shape[0], self.actor.out_dim
        actions = torch.empty(N, A, dtype=torch.float32, device=obs.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for t in (obs, critic_obs, eps, a_st, mu_st, sig_st, lp_st, v_st):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32), "contiguous float32 tensors"
        rc = self.lib.go2nn_policy_act(C.byref(self.actor.desc), p(self.actor.packed), C.byref(self.critic.desc), p(self.critic.packed), p(obs), p(critic_obs),
                                       p(self.ac.std.detach()), p(eps), p(actions), p(a_st), p(mu_st), p(sig_st), p(lp_st), p(v_st), N, self.actor._stream())
        if rc != 0:
            raise RuntimeError("go2nn_policy_act failed: %s" % self.lib.go2nn_last_error().decode())
        return actions


class PolicyKernelCTS:
    """CTS.act of one rollout step (rsl_rl/rsl_rl/algorithms/cts.py:112-149 over modules/actor_critic_cts.py:146-176) as TWO launches:
    both encoders on their env subsets -> the env-ordered normalised latent (go2nn_mlp_forward_rows), then actor([latent | obs]) + critic([latent | privileged obs]) +
    the sampling head (go2nn_policy_act_latent).  plan: modules/fused_cts.py:CtsPlan (which Linear modules make up the four networks); a model whose student encoder
    is not a plain MLP (the MoE variants) leaves the student rows of the latent to the caller."""

    def __init__(self, lib, model, plan, teacher_idx, student_idx, value_fold=None):
        self.lib, self.model, self.L = lib, model, plan.L
        self.enc_t = PackedMlp(lib, None, linears=plan.teacher)
        self.enc_s = PackedMlp(lib, None, linears=plan.student) if plan.student is not None else None
        self.actor, self.critic = PackedMlp(lib, None, linears=plan.actor), PackedMlp(lib, None, linears=plan.critic, fold=value_fold)          # (value_fold: as PolicyKernel)
        if self.actor.out_dim > 32 or self.critic.out_dim != 1:
            raise ValueError("head: up to 32 actions and a scalar value")
        self.ti, self.si = teacher_idx.to(torch.int32).contiguous(), student_idx.to(torch.int32).contiguous()
        self._nets = [self.enc_t] + ([self.enc_s] if self.enc_s is not None else [])

    def pack(self):
        for m in self._nets + [self.actor, self.critic]:
            m.pack()

    def _rows(self, nets, ios):
        n = len(nets)
        descs = (C.POINTER(Go2nnMlp) * n)(*[C.pointer(m.desc) for m in nets])
        packed = (C.c_void_p * n)(*[m.packed.data_ptr() for m in nets])
        rc = self.lib.go2nn_mlp_forward_rows(descs, packed, (Go2nnMlpIO * n)(*ios), n, nets[0]._stream())
        if rc != 0:
            raise RuntimeError("go2nn_mlp_forward_rows failed: %s" % self.lib.go2nn_last_error().decode())

    def latents(self, privileged_obs, history, latent):
        """latent [N, L] (env order) <- L2Norm(teacher_encoder(privileged_obs[teacher envs])), L2Norm(student_encoder(history[student envs])) — one launch
        (the student rows only when the student encoder is a plain MLP)"""
        for t in (privileged_obs, history, latent):
            assert t.is_contiguous() and t.dtype == torch.float32
        L = self.L
        ios = [Go2nnMlpIO(privileged_obs.data_ptr(), None, self.ti.data_ptr(), latent.data_ptr(), privileged_obs.shape[1], 0, privileged_obs.shape[1], self.ti.numel(), L, 1)]
        if self.enc_s is not None:
            ios.append(Go2nnMlpIO(history.data_ptr(), None, self.si.data_ptr(), latent.data_ptr(), history.shape[1], 0, history.shape[1], self.si.numel(), L, 1))
        self._rows(self._nets, ios)

    def moe_mix_ok(self, model):
        """the student encoder is a soft mixture whose tail go2nn_moe_mix_forward covers: E <= 16 experts, an L2 normaliser, the latent width the CTS kernels take"""
        enc = getattr(model, "student_moe_encoder", None)
        from .rsl_rl.modules.actor_critic_moe_cts import ActorCriticMoECTS
        from .rsl_rl.modules.utils import L2Norm
        return (enc is not None and getattr(type(model), "student_moe_parts", None) is ActorCriticMoECTS.student_moe_parts and hasattr(enc, "moe") and isinstance(getattr(enc, "norm_layer", None), L2Norm) and enc.moe.experts.expert_num <= 16
                and enc.moe.experts.output_dim == self.L)

    def moe_mix(self, logits, outs, bias, latent, rows=True):
        """latent[student envs] <- normalise(sum_e softmax(logits)_e (outs[e] + bias[e])): logits [n, E], outs [E, n, L] (expert-major, no bias), bias [E * L].
        rows False: latent is [n, L], row r <- source row r (the update's student rows)"""
        E, n, L = outs.shape
        for t in (logits, outs, bias, latent):
            assert t.is_contiguous() and t.dtype == torch.float32
        assert logits.shape == (n, E) and L == self.L and (n == self.si.numel() if rows else latent.shape[0] == n)
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.go2nn_moe_mix_forward(p(logits), p(outs), p(bias.detach()), p(self.si) if rows else None, p(latent), latent.shape[1], n, E, L, 1, self.enc_t._stream())
        if rc != 0:
            raise RuntimeError("go2nn_moe_mix_forward failed: %s" % self.lib.go2nn_last_error().decode())

    def value(self, latent, privileged_obs):
        """critic([latent | privileged obs]) -> [N, 1] (the bootstrap value of compute_returns), one launch on the packed weights"""
        N = latent.shape[0]
        v = torch.empty(N, 1, dtype=torch.float32, device=latent.device)
        self._rows([self.critic], [Go2nnMlpIO(latent.data_ptr(), privileged_obs.data_ptr(), None, v.data_ptr(), self.L, privileged_obs.shape[1], self.L, N, 1, 0)])
        return v

    def act(self, latent, obs, privileged_obs, eps, a_st=None, mu_st=None, sig_st=None, lp_st=None, v_st=None):
        N, A = obs.shape[0], self.actor.out_dim
        actions = torch.empty(N, A, dtype=torch.float32, device=obs.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for t in (latent, obs, privileged_obs, eps, a_st, mu_st, sig_st, lp_st, v_st):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32), "contiguous float32 tensors"
        rc = self.lib.go2nn_policy_act_latent(C.byref(self.actor.desc), p(self.actor.packed), C.byref(self.critic.desc), p(self.critic.packed), p(latent), self.L, p(obs), p(privileged_obs),
                                              p(self.model.std.detach()), p(eps), p(actions), p(a_st), p(mu_st), p(sig_st), p(lp_st), p(v_st), N, self.actor._stream())
        if rc != 0:
            raise RuntimeError("go2nn_policy_act_latent failed: %s" % self.lib.go2nn_last_error().decode())
        return actions
