"""PolicyEvaluator — on-device evaluation of a policy on a fixed, noise-free scenario set, with per-terrain, per-command scores.

It takes the slot the reference fills with RoboGauge (rsl_rl/rsl_rl/runners/on_policy_runner.py:103-111,243-295: every `interval` iterations and for the last model the
checkpoint is scored, the scores go to TensorBoard and to a results yaml).  RoboGauge itself (an HTTP service in front of MuJoCo) stays out of scope;
the numbers here are measured in THIS project's physics and are not comparable to the reference's RoboGauge table.

One evaluation = a simulator of its own (never the training env), reset, `warmup_s` of uncounted steps, `seconds` of counted steps of
    { write the commands, policy (deterministic mean), go2sim_step, go2nn_eval_accumulate }
then ONE go2nn_eval_reduce and ONE device -> host copy of its [groups, 12] fp64 table — the only synchronisation.  The metric formulas are in include/go2nn.h.

Reproducible: the simulator's random stream is indexed by a step count that the go2sim ABI does not rewind, so every evaluate() builds a FRESH simulator from the same
config and seed (the generated terrain is kept on the host, which makes that cheap): the same weights give bit-identical numbers.  For the same reason a captured HIP graph
belongs to one evaluation.  With `evaluation.replay` the first evaluate() of an evaluator runs eagerly and later ones capture ONE chunk of steps on their fresh simulator
and replay it for the whole horizon, bit-identical to the eager run; GO2_STRICT_GRAPHS=1 makes a failed capture raise, as elsewhere.  It is OFF by default because it
measured slower: capture + instantiation per evaluation cost more than the ~500 eager enqueues they replace (profiles/eval_bench.json).

Looking at the motion: with `evaluation.record = r > 0` a TrajectoryRecorder (utils/recorder.py) keeps the per-step frames of the first r robots of every group over the
counted steps — one more kernel call per step, after the accumulate call and inside the captured chunk —, evaluate() returns them as res["trace"] and write_results puts
them next to the yaml as trace_<it>.npz.  The scores do not depend on it (the recorder only reads); with record = 0 no recorder exists.

Beyond ideal conditions: with `evaluation.perturbations` (a list of [name, {field: value}]; DEFAULT_PERTURBATIONS is what --robust selects) every robot also belongs to one
perturbation — a velocity impulse `dv` [m/s, heading frame] on a fixed schedule, and / or changed dynamics: `strength` (motor strength), `kp_mul`, `kd_mul`, `added_mass` [kg],
`friction` (the robot's shape coefficient; the contact uses the mean of it and the terrain's).  Within a terrain kind the robots take the (scenario, perturbation) cells in
turn.  Every perturbation carries the push schedule (`dv` defaults to 0: a sham push), so every cell has the same windows and `nominal` gives their baseline.  A step is then
    { policy, go2nn_robust_apply, go2sim_step, write the commands, go2nn_eval_accumulate, go2nn_robust_accumulate }
— two more launches (csrc/go2nn_robust.h; the formulas and the recovery rule are in include/go2nn.h), inside the captured chunk — and one more reduce at the end.  Per push:
`push_falls` (share of pushes after which the robot fell inside the window), `recovered` (share after which the velocity error stayed below `recover_thr` for
`recover_hold_s`), `recovery_time_s` (push -> end of that hold, mean over the recovered pushes), `peak_lin_vel_err` / `peak_tilt` (largest value inside the window, mean
over pushes).  With `perturbations = None` nothing of this is allocated or launched.

How far up the terrain: with `evaluation.ladder` (--ladder; heightfield / trimesh tasks) the robots do not stand on ONE row of the terrain grid but on every row of
`ladder_levels`, under the commands `ladder_scenarios`: within a terrain kind they take the (level, scenario) cells in turn, cell index = (terrain * L + level) * S +
scenario — what every reduce kernel groups by —, and every fresh simulator gets `terrain_levels` / `env_origins` written per env.  A step is then
    { policy, go2sim_step, write the commands, go2nn_eval_accumulate, go2nn_ladder_accumulate }
— one more launch (csrc/go2nn_ladder.h; the rule is in include/go2nn.h), inside the captured chunk — and one more reduce at the end.  A robot has CLEARED its level when it
has been further than `ladder_distance` (default: half a tile, the simulator's own promotion rule) from where it stood at the first counted step; the record is latched per
robot on the device, so it survives the simulator's reset of a fallen robot.  Per cell: `cleared`, `fell`, `timed_out` (shares: what happened FIRST), `time_to_clear_s`,
`progress` (largest distance reached / `ladder_distance`, capped at 1); per terrain kind `level_cleared` (the highest level up to which every level has cleared >=
`ladder_pass_share`) and `mean_level_cleared` (the sum of `cleared` over the levels).  With `ladder = False` nothing of this is allocated or launched.

Commands that change: with `evaluation.maneuvers` (--maneuvers selects DEFAULT_MANEUVERS; a list of [name, [[seconds, vx, vy, yaw rate], ...]]) the maneuvers take the
scenarios' place: within a terrain kind the robots take the maneuvers in turn, cell index = terrain * M + maneuver.  The schedule of every maneuver lives on the device
(at most 8 segments in counted steps, the first at step 0 — it also covers the warm-up —, the last to the horizon's end), and a step is
    { policy, go2nn_maneuver_apply, go2sim_step, go2nn_maneuver_accumulate, go2nn_eval_accumulate }
— two more launches (csrc/go2nn_maneuver.h; the rule and the switch convention are in include/go2nn.h), inside the captured chunk, both writing the command row, so the
copy of the commands is not issued — and one more reduce at the end.  Per command switch, over the `maneuver_window_s` after it: `switch_falls` (share of switches after
which the robot fell inside the window), `settled` (share after which both velocity errors stayed below `maneuver_thr_lin` / `maneuver_thr_ang` for `maneuver_hold_s`),
`settle_time_s` (switch -> end of that hold, mean over the settled switches), `window_lin_vel_err` / `window_ang_vel_err` (means over the window's steps), `peak_tilt`
(largest value inside the window, mean over switches).  With `maneuvers = None` nothing of this is allocated or launched.

What the policy sees: with `evaluation.sensors` (--sensors selects DEFAULT_SENSORS; a list of [name, {field: value}]) every robot also belongs to one sensor condition
— `noise` (multiple of the task's own observation noise), `gyro_bias` [rad/s], `gravity_bias`, `joint_offset` [rad] (a constant offset per robot and column, uniform within
+- the value), `delay` (policy steps, at most 4: the proprioceptive columns are that old) and `drop` (probability that a frame is lost and the previous one repeats) —, split
like the perturbations: cell index = (terrain * S + scenario) * P + condition.  The observation no longer goes from the simulator straight into the policy: a step is
    { policy(delivered), go2sim_step, write the commands, go2nn_sensor_apply(obs_buf -> delivered), go2nn_eval_accumulate }
— two more launches (csrc/go2nn_sensor.h; the rule and the random streams are in include/go2nn.h), inside the captured chunk —, the CTS history and the recurrent state are
fed the delivered frames too, and the metrics still read the simulator's true state.  No reduce of its own: go2nn_eval_reduce over the cells gives RESULT_KEYS per condition.
With `sensors = None` nothing of this is allocated or launched.

How the robot walks: with `evaluation.gait` (--gait) every robot's feet are followed too — an add-on like `record`, not an axis: it splits nothing and works in the plain
evaluation and next to perturbations, ladder, maneuvers and sensors.  A step gains ONE launch after go2nn_eval_accumulate, inside the captured chunk,
    { ..., go2sim_step, ..., go2nn_eval_accumulate, ..., go2nn_gait_accumulate }
(csrc/go2nn_gait.h; the per-foot rule — utils/recorder.py gait_summary's, on the vertical contact force > `gait_contact_threshold` — is in include/go2nn.h) and the end one
go2nn_gait_reduce over the finest cells the mode has.  The cells' rows are summed on the host in fp64 for every partition the mode reports, and the figures GAIT_KEYS are
POOLED RATIOS over a partition's robots (sums of counts / sums of counts), not means of per-robot means, NaN where the denominator is 0: `duty_factor` (contact / used
frames), `stride_frequency` [Hz], `stance_time`, `swing_time` [s] (complete phases only), `slip_speed` [m/s] (horizontal foot speed in contact), `swing_height` [m, world z],
`swing_clearance` [m] (a swing's highest point above the foot's last contact frame), `touchdowns_per_s`, each per foot (`<key>/FL` ...) and over the four feet, and the
support pattern: `trot_share` (frames on exactly one diagonal pair), `flight_share` (no foot down), `mean_feet_in_contact`.  With `gait = False` nothing of this is loaded,
allocated or launched.

Why a robot fell: with `evaluation.blackbox = n > 0` (--blackbox [n]) a FallRecorder (utils/recorder.py; csrc/go2nn_blackbox.h) keeps for EVERY robot a ring of the last
`blackbox_seconds` of frames — the trajectory recorder's 112-float frame — that stops when the robot falls on a counted step and stays stopped while the simulator resets
the robot and carries on.  An add-on like `gait` and `record`, not an axis: one more kernel call per step (two small launches), after the recorder's slot and inside the
captured chunk; it starts with the warm-up and is NOT cleared at the warm-up boundary, so a fall right after it still has its history.  At the end the small state block
is read, and of every cell of the finest partition the mode reports the rings of the `n` fallen robots with the lowest env indices are gathered on the device and copied:
res["falls"], written next to the yaml as falls_<it>.npz (utils/recorder.py read_falls, fall_summary).  Memory: num_envs x steps x 448 bytes (1024 x 100: 46 MB), refused
above `blackbox_max_bytes`.  Only a robot's first counted fall is kept.  The scores do not depend on it; with blackbox = 0 nothing is allocated, loaded or launched.

How even the policy and the robot are, left against right: with `evaluation.asymmetry` (--asymmetry) every step also runs the policy on the mirror image of the observation
it has just read, and one more launch after the simulator's step scores both — an add-on like `gait`: it splits nothing and works next to every mode,
    { a = policy(o), go2nn_mirror_rows(o [, the CTS history ring]), a_m = policy(M_o o), ..., go2sim_step(a), ..., go2nn_asym_accumulate(a, a_m) }
(csrc/go2nn_asym.h; the rule is in include/go2nn.h; the tables are utils/symmetry.py's), all inside the captured chunk, and at the end one go2nn_asym_reduce over the
finest cells the mode has.  With e = a - M_a a_m, on every counted step: `equivariance_rmse` (over the 12 joints; `/hip`, `/thigh`, `/calf` over the 4 of a kind),
`equivariance_rel` (|e| / |a|), `equivariance_max`.  On the counted steps without a reset whose command has vy == 0 and yaw == 0 exactly (`sym_steps_share` of all): for x in
action (a^2), torque (tau^2), power (|tau qd|), contact (feet with force z > `gait_contact_threshold`) `left_share/<x>` = L / (L + R) and `imbalance/<x>` = the mean over
the robots of each robot's own |L - R| / (L + R).  ASYM_KEYS are pooled ratios of the cells' sums (the max of their maxima), NaN where nothing was counted; they live in
res["asymmetry"] only — res["overall"] and every other result are those of the flag-off run.  The mirrored forward shares the weights and nothing else with act(); a
recurrent policy is refused (its mirrored stream needs a twin hidden state).  With `asymmetry = False` nothing of this is loaded, allocated or launched.

How fast the joints are driven: with `evaluation.spectrum` (--spectrum) every robot's 12 actions and 12 torques after the step, and its reset flag, are kept for the counted
steps — one more plain launch per step, behind the recorders' slot and inside the captured chunk, into a device trace with its own step counter,
    { ..., go2sim_step, ..., go2nn_eval_accumulate, ..., go2nn_spectrum_record }
(csrc/go2nn_spectrum.h; steps x num_envs x 25 floats, refused above `spectrum_max_bytes`) — and after the last step ONE go2nn_spectrum_welch, outside any capture, makes every
robot's Welch spectra of them (the estimator is in include/go2nn.h: windows of `spectrum_window` steps, hop W / 2, a window with a reset frame skipped, mean removed, periodic
Hann, density scaling; the joints pooled by kind) and one go2nn_spectrum_reduce sums the table over the finest cells the mode has.  An add-on like `gait`: it splits
nothing and works next to every mode.  SPECTRUM_KEYS, per signal and (`/hip`, `/thigh`, `/calf`) per joint kind, over the bins k >= 1 at f_k = k fs / W: `hf_share` = the
power at f_k >= `spectrum_cutoff_hz` over the power, `centroid_hz` = sum f_k P_k / sum P_k, `smoothness` = CAPS's 2 / (n fs) sum f_k M_k on the mean amplitude spectrum
(n = W / 2), `power` = (fs / W) sum of the mean P_k: the mean non-DC variance per joint; `spectrum_windows` and `spectrum_skipped_share` next to them.  Pooled ratios of the
cells' sums, NaN where nothing was counted; res["overall"] gains the eight pooled figures.  They have no bootstrap replicates (`bootstrap_all` leaves the family out).
With `spectrum = False` nothing of this is loaded, allocated or launched.

What the policy does to the motors and the legs: with `evaluation.actuators` (--actuators) every robot's joints and feet are followed too — an add-on like `gait`: it splits
nothing and works in the plain evaluation and next to every mode and add-on.  A step gains ONE launch behind the gait scorer's slot, inside the captured chunk,
    { ..., go2sim_step, ..., go2nn_eval_accumulate, ..., go2nn_actuator_accumulate }
(csrc/go2nn_actuator.h; the rule is in include/go2nn.h: frames with reset_buf set are not used, as in gait) and the end one go2nn_actuator_reduce over the finest cells the
mode has.  The limits are the simulator's nominal `torque_limits` and `dof_vel_limits` and the soft position limits the reward uses; a sample counts as saturated at or above
`actuators_saturation` x the limit (an exact fp32 comparison against a threshold formed once on the host); a foot is in contact above `gait_contact_threshold`.  ACTUATOR_KEYS
are pooled over a partition's robots — over all joints, per joint kind (`<key>/hip`, `/thigh`, `/calf`) and per joint (`<key>/FL_hip` ...), NaN where nothing was counted:
`torque_rms` [N m] (what motor heating goes with), `torque_rms_share` (each joint's tau^2 in units of its limit^2), `torque_peak` and `joint_speed_peak` (the mean over the
robots of each robot's own largest sample), `torque_saturation` and `joint_speed_saturation` (share of samples), `positive_power` and `negative_power` [W] (mean of
max(+-tau qd, 0) per step, summed over the pool's joints), `limit_margin` [rad] (the mean over robots of each robot's own smallest distance to a position limit; negative past
it; higher is better); per foot (`<key>/FL` ...) and over the feet `grf_peak` [N] (mean over robots, and feet, of each one's largest vertical force) and `grf_stance_mean`
(mean force over the contact frames); per partition `energy_per_m` [J/m] (positive mechanical work / distance the root travelled in the plane; NaN below 1 mm per used
robot, as for `stand`).  ACTUATOR_EXTREME_KEYS — `torque_peak_max`, `joint_speed_peak_max`, `grf_peak_max`, `limit_margin_min`, with the same pools — are the exact max / min
over a partition's robots, from one more device -> host copy of the table's USED, peak and margin rows; they get no bootstrap interval.  The figures live in
res["actuators"] only: res["overall"] and every other result are those of the flag-off run.  With `actuators = False` nothing of this is loaded, allocated or launched.

How sure a figure is: with `evaluation.bootstrap = B > 0` (--ci [B]) ONE more launch after go2nn_eval_reduce, on the same accumulators and the same cells, redraws every
cell's robots with replacement B times (go2nn_eval_bootstrap: csrc/go2nn_bootstrap.h, the rule in include/go2nn.h; Philox seed `bootstrap_seed`) and one more device ->
host copy brings the [B, cells, 12] fp64 table of resampled reduce rows: res["bootstrap"] = {"replicates", "seed", "confidence", "table", "overall" ([B, 12]: the overall
row per replicate)}.  A partition's replicate rows are the sums of its cells' (_cell_views: the reshapes and sums of _results, with the replicate axis in front), a figure's replicates are _row() of them, and every leaf
dict _row() makes — "overall", "groups", "cells", "perturbations", "sensors", "maneuvers", the ladder's per-level leaves — gains "ci": {metric: [lo, hi]} for CI_KEYS, the
(1 - confidence) / 2 and (1 + confidence) / 2 quantiles ([nan, nan] where every replicate is NaN).  The cells are strata: every replicate keeps the design's robots per
cell.  An evaluation is deterministic per robot index, so the same replicates of two checkpoints' evaluations are PAIRED: compare() below.  The modes' own figures
(push_falls, settle_time_s, cleared, ...) and the gait and asymmetry sections get NO interval unless `evaluation.bootstrap_all` (--ci_all) is on: then one more launch per
active scoring family (go2nn_<family>_bootstrap, after the family's reduce, outside any captured graph) redraws the SAME robots — the draws depend on (b, g, k, seed) only —
on the family's table, res["bootstrap"] gains "tables": {family: [B, cells, cols]} and "metrics": {figure: float64 [B]} (the overall replicates of every figure that has an
interval, the asymmetry's among them), and every leaf that reports a family's figures gains them in its "ci" — the leaves of res["gait"] and res["asymmetry"] too, the gait's
with the per-foot keys, the actuators' with every pool's keys but the extremes; res["ladder_summary"][t] gains "ci" for level_cleared and mean_level_cleared from the replicate `cleared` curves.  The replicate figures are the row
functions' vectorised twins (robust_replicates, ... below: the same IEEE operations on every replicate row and leaf at once); integer counts (pushes, switches, n_envs) and
equivariance_max (a bootstrap of a maximum is not one) get no interval; `bootstrap_max_bytes` then caps the sum of all tables.  An add-on like `gait`: it reads only the accumulators and the cell
assignment and works next to every mode; the table is refused above `bootstrap_max_bytes`; with bootstrap = 0 nothing is loaded, allocated or launched.

Isolated: nothing of the training env, the model, the optimizer or torch's generators is written; policy state the evaluation needs (the CTS observation history, the
recurrent memory's hidden state) lives in buffers of the evaluator."""
import copy
import ctypes as C
import math
import os
import types

import numpy as np
import torch

from .. import _abi
from .._nn import (EVAL_FIELDS, EVAL_METRICS, GO2NN_EVAL_NUM, GO2NN_RNN_GRU, GO2NN_RNN_LSTM, GO2NN_ROBUST_ACC_NUM, GO2NN_ROBUST_MAX_SPECS, GO2NN_ROBUST_NUM, ROBUST_FIELDS, ROBUST_MASK,
                   GO2NN_LADDER_NUM, GO2NN_LADDER_OUT_NUM, LADDER_FIELDS, LADDER_OUT, GO2NN_MANEUVER_ACC_NUM, GO2NN_MANEUVER_MAX_SEGS, GO2NN_MANEUVER_MAX_SPECS, GO2NN_MANEUVER_NUM,
                   MANEUVER_FIELDS, MANEUVER_OUT, Go2nnEvalIn, Go2nnFwdJob, Go2nnLadderIn, Go2nnManeuverIn, Go2nnManeuverSpec, Go2nnMlpIO, Go2nnRnnCellJob, Go2nnRobustIn,
                   Go2nnRobustSpec, PackedMlp, GAIT_FIELDS, GAIT_OUT_FOOT, GO2NN_GAIT_NUM, GO2NN_GAIT_OUT_DIAGONAL, GO2NN_GAIT_OUT_NUM, GO2NN_GAIT_OUT_SUPPORT0, Go2nnGaitIn,
                   gait_out_col, ASYM_FIELDS, ASYM_OUT, ASYM_PAIRS, GO2NN_ASYM_NUM, GO2NN_ASYM_OUT_NUM, Go2nnAsymIn, GO2NN_SENSOR_MAX_DELAY, GO2NN_SENSOR_MAX_SPECS, GO2_OBS_KINDS, SENSOR_KINDS, Go2nnSensorIn, Go2nnSensorSpec)
from .._nn import (GO2NN_SPECTRUM_MAX_STEPS, GO2NN_SPECTRUM_MAX_WINDOW, GO2NN_SPECTRUM_MIN_WINDOW, GO2NN_SPECTRUM_SKIPPED, GO2NN_SPECTRUM_USED, SPECTRUM_FIELDS, SPECTRUM_KINDS,
                   SPECTRUM_SIGNALS, Go2nnSpectrumIn, spectrum_bins, spectrum_row, spectrum_rows, spectrum_trace_rows, spectrum_twiddle)
from .._nn import (ACTUATOR_FIELDS, ACTUATOR_FOOT_ROWS, ACTUATOR_JOINT_ROWS, GO2NN_ACTUATOR_NUM, GO2NN_ACTUATOR_OUT_NUM, Go2nnActuatorIn, actuator_out_col, actuator_row)
from .._nn import mirror_rows
from .helpers import class_to_dict

DEFAULT_SCENARIOS = [["forward_1.0", 1.0, 0.0, 0.0], ["forward_2.0", 2.0, 0.0, 0.0], ["backward_1.0", -1.0, 0.0, 0.0], ["lateral_0.5", 0.0, 0.5, 0.0],
                     ["turn_1.0", 0.0, 0.0, 1.0], ["stand", 0.0, 0.0, 0.0]]
MEAN_METRICS = EVAL_METRICS[1:9]          # reported as per-step means; `falls` per robot, `survival`, `n_envs` next to them
RESULT_KEYS = MEAN_METRICS + ("falls", "survival", "n_envs")
CI_KEYS = MEAN_METRICS + ("falls", "survival")          # what `evaluation.bootstrap` puts an interval on: the figures _row() makes of ONE reduce row
# name, {field: value}; fields: dv [m/s: forward, left, up in the heading frame] and the dynamics values of ROBUST_MASK.  `nominal` is the sham push: the same windows, dv = 0
DEFAULT_PERTURBATIONS = [["nominal", {}], ["push_front_1.0", {"dv": [1.0, 0.0, 0.0]}], ["push_side_1.0", {"dv": [0.0, 1.0, 0.0]}], ["payload_3kg", {"added_mass": 3.0}],
                         ["motor_0.8", {"strength": 0.8}], ["kp_0.8", {"kp_mul": 0.8}], ["friction_0.3", {"friction": 0.3}]]
ROBUST_KEYS = ("pushes", "push_falls", "recovered", "recovery_time_s", "peak_lin_vel_err", "peak_tilt")
DEFAULT_LADDER_SCENARIOS = [["forward_1.0", 1.0, 0.0, 0.0]]
LADDER_KEYS = ("cleared", "fell", "timed_out", "time_to_clear_s", "progress")
LADDER_SUMMARY_KEYS = ("level_cleared", "mean_level_cleared")
# name, [[seconds, vx, vy, yaw rate], ...]: segment k holds from its time (counted; the first is 0 and also covers the warm-up) to the next one's; for the 10 s horizon
DEFAULT_MANEUVERS = [["start_1.0", [[0.0, 0.0, 0.0, 0.0], [5.0, 1.0, 0.0, 0.0]]], ["brake_1.0", [[0.0, 1.0, 0.0, 0.0], [5.0, 0.0, 0.0, 0.0]]],
                     ["brake_2.0", [[0.0, 2.0, 0.0, 0.0], [5.0, 0.0, 0.0, 0.0]]], ["reverse_1.0", [[0.0, 1.0, 0.0, 0.0], [5.0, -1.0, 0.0, 0.0]]],
                     ["sidestep_flip_0.5", [[0.0, 0.0, 0.5, 0.0], [5.0, 0.0, -0.5, 0.0]]], ["turn_flip_1.0", [[0.0, 0.0, 0.0, 1.0], [5.0, 0.0, 0.0, -1.0]]],
                     ["walk_into_turn_1.0", [[0.0, 1.0, 0.0, 0.0], [5.0, 1.0, 0.0, 1.0]]]]
MANEUVER_KEYS = ("switches", "switch_falls", "settled", "settle_time_s", "window_lin_vel_err", "window_ang_vel_err", "peak_tilt")
# name, {field: value}; fields: noise (x the task's own noise vector), gyro_bias [rad/s], gravity_bias, joint_offset [rad], delay [policy steps], drop [probability]
DEFAULT_SENSORS = [["nominal", {}], ["noise_1.0", {"noise": 1.0}], ["noise_3.0", {"noise": 3.0}], ["gyro_bias_0.1", {"gyro_bias": 0.1}],
                   ["joint_offset_0.05", {"joint_offset": 0.05}], ["delay_1", {"delay": 1}], ["delay_2", {"delay": 2}], ["drop_0.2", {"drop": 0.2}]]
SENSOR_FIELDS = ("noise", "gyro_bias", "gravity_bias", "joint_offset", "delay", "drop")
# pooled over a partition's robots: per foot ("<key>/<foot>") and over the four feet, then the support pattern
GAIT_FOOT_KEYS = ("duty_factor", "stride_frequency", "stance_time", "swing_time", "slip_speed", "swing_height", "swing_clearance", "touchdowns_per_s")
GAIT_PATTERN_KEYS = ("trot_share", "flight_share", "mean_feet_in_contact")
GAIT_KEYS = GAIT_FOOT_KEYS + GAIT_PATTERN_KEYS
DIAGONAL_PAIRS = (("FL", "RR"), ("FR", "RL"))
# pooled over a partition's robots: the equivariance error of the policy on the visited states, then per load x its left share and the per-robot mean imbalance
ASYM_LOADS = ("action", "torque", "power", "contact")          # in the order of ASYM_PAIRS (act_sq, torque_sq, power, contact)
ASYM_EQ_KEYS = ("equivariance_rmse", "equivariance_rmse/hip", "equivariance_rmse/thigh", "equivariance_rmse/calf", "equivariance_rel", "equivariance_max")
ASYM_KEYS = ASYM_EQ_KEYS + ("sym_steps_share",) + tuple("left_share/" + x for x in ASYM_LOADS) + tuple("imbalance/" + x for x in ASYM_LOADS)
# pooled over a partition's robots, per signal ("action_<key>", "torque_<key>") and per joint kind ("<signal>_<key>/<kind>"): the share of the power at and above the
# cut-off, the power's centroid, CAPS's frequency-weighted mean amplitude, the mean non-DC variance per joint; then the windows analysed and the share skipped for a reset
SPECTRUM_FIGURES = ("hf_share", "centroid_hz", "smoothness", "power")
SPECTRUM_KEYS = tuple("%s_%s" % (s, k) for s in SPECTRUM_SIGNALS for k in SPECTRUM_FIGURES)
SPECTRUM_COUNT_KEYS = ("spectrum_windows", "spectrum_skipped_share")
# pooled over a partition's robots, over all joints, per joint kind ("<key>/hip", "/thigh", "/calf") and per joint ("<key>/FL_hip" ...): RMS torque [N m] and the same in units
# of each joint's limit, the mean over robots of each robot's own peak torque / speed, the share of samples at or above `actuators_saturation` x the limit, the mean positive
# and negative mechanical power [W] summed over the pool's joints, the mean over robots of each robot's own smallest distance to a soft position limit [rad]; per foot
# ("<key>/FL" ...) and over the feet the mean of each robot's own largest vertical foot force [N] and the mean force over the contact frames; per partition the positive
# mechanical work per metre travelled [J/m]; and the extremes over a partition's robots, which are exact maxima / minima and have no bootstrap interval
ACTUATOR_JOINT_KEYS = ("torque_rms", "torque_rms_share", "torque_peak", "torque_saturation", "joint_speed_peak", "joint_speed_saturation", "positive_power", "negative_power",
                       "limit_margin")
ACTUATOR_FOOT_KEYS = ("grf_peak", "grf_stance_mean")
ACTUATOR_KEYS = ACTUATOR_JOINT_KEYS + ACTUATOR_FOOT_KEYS + ("energy_per_m",)
ACTUATOR_EXTREME_KEYS = ("torque_peak_max", "joint_speed_peak_max", "grf_peak_max", "limit_margin_min")
ACTUATOR_KINDS = ("hip", "thigh", "calf")
# the rows of the per-robot table behind the extremes, as one device -> host copy brings them: USED (a robot without a used frame has none), then the maxima, then the minima
ACTUATOR_MAX_ROWS = [actuator_row(k, j) for k in ("tau_peak", "vel_peak") for j in range(12)] + [actuator_row("fz_peak", f) for f in range(4)]
ACTUATOR_MIN_ROWS = [actuator_row("margin_min", j) for j in range(12)]
# with `bootstrap_all`: what the printed table's interval block shows of each family
BOOTSTRAP_HEADLINES = (("robust", ("push_falls", "recovered", "recovery_time_s")), ("maneuver", ("switch_falls", "settled", "settle_time_s")),
                       ("ladder", ("cleared", "mean_level_cleared")), ("gait", ("slip_speed", "trot_share", "swing_clearance")), ("asym", ("equivariance_rmse", "imbalance/torque")),
                       ("actuator", ("torque_rms_share", "torque_saturation", "energy_per_m")))
MAX_CHUNK = 50
# The accumulate kernel runs AFTER the env step, when the simulator has already rolled its action history (last_actions = this step's actions): the previous step's
# actions — the kernel's `last_actions` input — are then in the simulator's last_last_actions buffer.
EVAL_SOURCE = {"last_actions": "last_last_actions"}


def _get(section, key, default=None):
    return section.get(key, default) if isinstance(section, dict) else getattr(section, key, default)


def _field_views(a, buf, names, source=None, last=False):
    """fill the (pointer, env stride, component stride) triples `names` of the ctypes input struct `a` from the simulator's buffers `buf`, in elements from the torch views'
    own strides -> a.  source: field name -> buffer name where they differ;  last: the component stride is that of the LAST dimension (per-body fields, whose body stride
    the struct carries separately), not of dimension 1"""
    for name in names:
        t, f = buf[(source or {}).get(name, name)], getattr(a, name)
        f.p, f.env_stride, f.comp_stride = t.data_ptr(), t.stride(0), (t.stride(t.dim() - 1 if last else 1) if t.dim() > 1 else 0)
    return a


class _ScoreTable:
    """One per-env score table `table` [rows, N]: begun once per evaluation (go2nn_<name>_begin), advanced once per step (go2nn_<name>_accumulate; robust and maneuver also
    go2nn_<name>_apply before the simulator steps) and reduced once into `out` [cells, cols] (go2nn_<name>_reduce).  make_in: -> the kernels' input struct on the current
    simulator;  args: the tensors a step's launches take between the input and the table (the specs and the env -> spec map);  reduce_args: what the reduce takes in front
    of `out`.  The spectrum's step is go2nn_spectrum_record into a trace and its table is made by one go2nn_spectrum_welch after the last step: `state` is what
    go2nn_<name>_begin starts (the table itself, or that trace, which carries the step counter), begin_args what it takes behind the start step, and resampled says whether
    the family has a go2nn_<name>_bootstrap (`bootstrap_all`).  The evaluator's attributes stay the owners of every tensor"""

    def __init__(self, name, make_in, table, out, args=(), reduce_args=(), state=None, begin_args=(), resampled=True):
        self.name, self.make_in, self.table, self.out, self.reduce_args = name, make_in, table, out, tuple(reduce_args)
        self.args = tuple(C.c_void_p(t.data_ptr()) for t in args)
        self.state, self.begin_args, self.resampled = (table if state is None else state), tuple(begin_args), bool(resampled)


def replicate_metrics(rows):
    """rows: float64 [B, GO2NN_EVAL_NUM + 2], one reduce row per bootstrap replicate -> {metric: float64 [B]} for CI_KEYS: PolicyEvaluator._row's arithmetic on every row
    at once (one IEEE division each: the same bits), NaN where _row reports NaN"""
    rows = np.asarray(rows, np.float64)
    n, steps = rows[:, GO2NN_EVAL_NUM], rows[:, 0]
    per = lambda x, d: np.divide(x, d, out=np.full(x.shape, np.nan), where=d > 0)
    out = {m: per(rows[:, 1 + i], steps) for i, m in enumerate(MEAN_METRICS)}
    out["falls"], out["survival"] = per(rows[:, EVAL_METRICS.index("falls")], n), per(rows[:, GO2NN_EVAL_NUM + 1], n)
    return out


def interval(replicates, confidence):
    """the percentile interval of a figure's replicates -> [lo, hi] (plain floats); [nan, nan] where every replicate is NaN"""
    x = np.asarray(replicates, np.float64)
    if x.size == 0 or np.isnan(x).all():
        return [float("nan"), float("nan")]
    lo, hi = np.nanquantile(x, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
    return [float(lo), float(hi)]


def intervals(rows, confidence):
    """rows: float64 [B, 12], a leaf's reduce row per replicate -> its "ci" entry {metric: [lo, hi]} for CI_KEYS: interval() of every figure's replicates — taken in one
    call where no replicate is NaN (the quantile of numbers is nanquantile's), figure by figure otherwise"""
    reps = replicate_metrics(rows)
    mat = np.stack([reps[m] for m in CI_KEYS], 1)
    if np.isnan(mat).any():
        return {m: interval(reps[m], confidence) for m in CI_KEYS}
    q = np.quantile(mat, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0], axis=0)
    return {m: [float(q[0, i]), float(q[1, i])] for i, m in enumerate(CI_KEYS)}


# ---- `evaluation.bootstrap_all`: the row functions' twins.  rows: float64 [..., cols], a family's reduce row per replicate (and per leaf) -> {key: float64 [...]}: the
# arithmetic of PolicyEvaluator._<family>_row on every row at once — the same IEEE operations in the same order, so replicate b's figure is the row function of replicate
# row b bit for bit —, NaN where the row function reports NaN.  Integer counts (pushes, switches, n_envs) and equivariance_max (a bootstrap of a maximum is not one) get none.
def _per(x, d):
    """x / d where d > 0, NaN elsewhere: the row functions' `x / n if n > 0 else nan`"""
    x, d = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(d, np.float64))
    return np.divide(x, d, out=np.full(x.shape, np.nan), where=d > 0)


def robust_replicates(rows, dt):
    r = np.asarray(rows, np.float64)
    pushes, rec = r[..., 0], r[..., 2]
    return {"push_falls": _per(r[..., 1], pushes), "recovered": _per(r[..., 2], pushes), "recovery_time_s": _per(r[..., 3], rec) * dt,
            "peak_lin_vel_err": _per(r[..., 4], pushes), "peak_tilt": _per(r[..., 5], pushes)}


def maneuver_replicates(rows, dt):
    r = np.asarray(rows, np.float64)
    v = {k: r[..., i] for i, k in enumerate(MANEUVER_OUT)}
    sw, settled, steps = v["switches"], v["settled"], v["win_steps"]
    return {"switch_falls": _per(v["switch_falls"], sw), "settled": _per(settled, sw), "settle_time_s": _per(v["settle_steps"], settled) * dt,
            "window_lin_vel_err": _per(v["win_lin_err"], steps), "window_ang_vel_err": _per(v["win_ang_err"], steps), "peak_tilt": _per(v["peak_tilt_sum"], sw)}


def ladder_replicates(rows, dt):
    r = np.asarray(rows, np.float64)
    v = {k: r[..., i] for i, k in enumerate(LADDER_OUT)}
    return {"cleared": _per(v["cleared"], v["n"]), "fell": _per(v["fell"], v["n"]), "timed_out": _per(v["timed_out"], v["n"]),
            "time_to_clear_s": _per(v["clear_steps"], v["cleared"]) * dt, "progress": _per(v["progress"], v["n"])}


def gait_replicates(rows, dt, foot_names):
    r = np.asarray(rows, np.float64)
    K, first = len(GAIT_OUT_FOOT), gait_out_col(0, GAIT_OUT_FOOT[0])
    feet = [r[..., first + f * K:first + (f + 1) * K] for f in range(4)]
    d = {}
    for name, row in [("", ((feet[0] + feet[1]) + feet[2]) + feet[3])] + [("/" + n, feet[f]) for f, n in enumerate(foot_names)]:          # (feet.sum(0): in the feet's order)
        v = {k: row[..., i] for i, k in enumerate(GAIT_OUT_FOOT)}
        d["duty_factor" + name] = _per(v["contact"], v["used"])
        d["stride_frequency" + name] = _per(v["strides"], v["stride_steps"] * dt)
        d["stance_time" + name] = _per(v["stance_steps"] * dt, v["stances"])
        d["swing_time" + name] = _per(v["swing_steps"] * dt, v["swings"])
        d["slip_speed" + name] = _per(v["slip_sum"], v["contact"])
        d["swing_height" + name] = _per(v["height_sum"], v["swings"])
        d["swing_clearance" + name] = _per(v["clearance_sum"], v["swings"])
        d["touchdowns_per_s" + name] = _per(v["touchdowns"], v["used"] * dt)
    frames, support = feet[0][..., 0], r[..., GO2NN_GAIT_OUT_SUPPORT0:GO2NN_GAIT_OUT_SUPPORT0 + 5]
    d["trot_share"], d["flight_share"] = _per(r[..., GO2NN_GAIT_OUT_DIAGONAL], frames), _per(support[..., 0], frames)
    weighted = np.zeros(frames.shape)          # np.dot(arange(5), support): whole numbers far below 2^53, exact in any order
    for k in range(5):
        weighted = weighted + float(k) * support[..., k]
    d["mean_feet_in_contact"] = _per(weighted, frames)
    return d


def asym_replicates(rows):
    r = np.asarray(rows, np.float64)
    v = {k: r[..., i] for i, k in enumerate(ASYM_OUT)}
    steps = v["eq_steps"]
    d = {"equivariance_rmse": np.sqrt(_per(v["eq_sq"], 12.0 * steps))}
    for kind in ("hip", "thigh", "calf"):
        d["equivariance_rmse/" + kind] = np.sqrt(_per(v["eq_sq_" + kind], 4.0 * steps))
    d["equivariance_rel"] = np.sqrt(_per(v["eq_sq"], v["act_sq"]))
    d["sym_steps_share"] = _per(v["sym_steps"], steps)
    for x, p in zip(ASYM_LOADS, ASYM_PAIRS):
        d["left_share/" + x] = _per(v[p + "_l"], v[p + "_l"] + v[p + "_r"])
    for x, p in zip(ASYM_LOADS, ASYM_PAIRS):
        d["imbalance/" + x] = _per(v[p + "_imb"], v[p + "_imb_n"])
    return d


def actuator_figures(rows, dt, joint_names, foot_names, torque_limits):
    """rows: float64 [..., GO2NN_ACTUATOR_OUT_NUM (+ the extremes)], go2nn_actuator_reduce's row per leaf (and per replicate) -> {key: float64 [...]} for ACTUATOR_KEYS
    over every pool; NaN where nothing was counted.  The ONE statement of the figures: PolicyEvaluator._actuator_row is this on a single row, so replicate b's figure is
    the row function of replicate row b bit for bit.  A pool's sums run over its joints (feet) in DOF (foot_body) order"""
    r = np.asarray(rows, np.float64)
    col = lambda name, i=None: r[..., actuator_out_col(name, i)]
    n_used, used, dist = col("n_used"), col("used"), col("dist")

    def total(name, members, scale=None):
        acc = np.zeros(used.shape)
        for i in members:
            acc = acc + (col(name, i) if scale is None else col(name, i) / scale[i])
        return acc
    kind_of = [next((k for k in ACTUATOR_KINDS if k in n), None) for n in joint_names]
    pools = [("", list(range(12)))] + [("/" + k, [j for j in range(12) if kind_of[j] == k]) for k in ACTUATOR_KINDS] + [("/" + n, [j]) for j, n in enumerate(joint_names)]
    limit_sq = [float(t) * float(t) for t in torque_limits]
    d = {}
    for name, js in pools:
        nj = float(len(js))
        d["torque_rms" + name] = np.sqrt(_per(total("tau_sq", js), nj * used))
        d["torque_rms_share" + name] = np.sqrt(_per(total("tau_sq", js, limit_sq), nj * used))
        d["torque_peak" + name] = _per(total("tau_peak", js), nj * n_used)
        d["torque_saturation" + name] = _per(total("tau_sat", js), nj * used)
        d["joint_speed_peak" + name] = _per(total("vel_peak", js), nj * n_used)
        d["joint_speed_saturation" + name] = _per(total("vel_sat", js), nj * used)
        d["positive_power" + name] = _per(total("work_pos", js), used)
        d["negative_power" + name] = _per(total("work_neg", js), used)
        d["limit_margin" + name] = _per(total("margin_min", js), nj * n_used)
    for name, fs in [("", list(range(4)))] + [("/" + n, [f]) for f, n in enumerate(foot_names)]:
        d["grf_peak" + name] = _per(total("fz_peak", fs), float(len(fs)) * n_used)
        d["grf_stance_mean" + name] = _per(total("fz_sum", fs), total("fz_frames", fs))
    moved = dist * dt >= 1e-3 * n_used          # below a millimetre per used robot (`stand`) a cost per metre says nothing
    d["energy_per_m"] = _per(total("work_pos", list(range(12))), np.where(moved, dist, 0.0))          # (dt cancels: joules per metre)
    return d


def actuator_replicates(rows, dt, joint_names, foot_names, torque_limits):
    """the bootstrappable actuator figures of replicate rows [B, leaves, cols]: all but the extremes (a bootstrap of an extreme is not one)"""
    return actuator_figures(rows, dt, joint_names, foot_names, torque_limits)


def interval_columns(mat, confidence):
    """mat: float64 [B, M], M figures' replicates -> (lo [M], hi [M]): interval() of every column — the columns without a NaN in one quantile call, the others one by one"""
    mat = np.asarray(mat, np.float64)
    lo, hi = np.full(mat.shape[1], np.nan), np.full(mat.shape[1], np.nan)
    clean = ~np.isnan(mat).any(0)
    if clean.any() and mat.shape[0] > 0:
        lo[clean], hi[clean] = np.quantile(mat[:, clean], [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0], axis=0)
    for j in np.nonzero(~clean)[0]:
        lo[j], hi[j] = interval(mat[:, j], confidence)
    return lo, hi


def compare(reps_a, reps_b, confidence=0.95):
    """The paired comparison of two evaluations of ONE evaluator (same robots, same `bootstrap_seed`): replicate b of both redrew the same robots, so d_b = a_b - b_b
    is a replicate of the difference — common random numbers, far tighter than two marginal intervals side by side.
    -> {"diff_ci": [lo, hi] of d, "tied": lo <= 0 <= hi}; a difference that does not exist (every d_b NaN) is [nan, nan] and not tied: nothing can be said of it"""
    a, b = np.asarray(reps_a, np.float64), np.asarray(reps_b, np.float64)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("compare: two replicate vectors of one length are needed, got shapes %s and %s" % (a.shape, b.shape))
    lo, hi = interval(a - b, confidence)
    return {"diff_ci": [lo, hi], "tied": bool(lo <= 0.0 <= hi)}


def evaluation_env_cfg(env_cfg, ev):
    """The task's env config as the evaluation runs it: scripts/play.py's edits (noise, pushes and every domain randomisation off, no terrain curriculum, env.test) plus
    commands that hold — no resampling inside the horizon, no heading controller, no command curricula — and the evaluation's own seed and size."""
    cfg = copy.deepcopy(env_cfg)
    horizon = float(_get(ev, "warmup_s", 1.0)) + float(_get(ev, "seconds", 10.0))
    cfg.env.num_envs = int(_get(ev, "num_envs", 1024))
    cfg.env.test = True
    cfg.env.episode_length_s = max(float(cfg.env.episode_length_s), horizon + 1.0)          # no time-out resets inside the horizon
    cfg.seed = int(_get(ev, "seed", 12345))
    cfg.noise.add_noise = False
    cfg.terrain.curriculum = False
    dr = cfg.domain_rand
    for k in dir(dr):
        if k.startswith("randomize_"):
            setattr(dr, k, False)
    dr.push_robots = False
    cm = cfg.commands
    cm.resampling_time = 10.0 * horizon + 1000.0
    cm.heading_command = False
    cm.curriculum = False
    cm.dynamic_resample_commands = False
    cm.command_range_curriculum = []
    cm.zero_command_curriculum = None
    if any("strength" in (p[1] or {}) for p in (_get(ev, "perturbations") or [])):
        # the simulator applies motor_strengths only when it was created with the randomisation on: on, with the range [1, 1] — a reset draws exactly 1, a product with 1 is exact
        dr.randomize_motor_strength, dr.motor_strength_range = True, [1.0, 1.0]
    return cfg


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# The policy side: the deterministic action mean of the three model families, on the go2nn kernels, with every piece of recurrent state owned here.
class _Policy:
    def __init__(self, ev, model):
        self.ev, self.model = ev, model
        self._stream, self._check = ev._stream, ev._check          # the evaluator's own: one stream, one way to fail

    def begin(self, obs):
        """once per evaluation, after the reset: read the CURRENT weights (packed images are rebuilt here, so an evaluation after an update never sees stale ones)"""

    def act(self, obs):
        raise NotImplementedError

    def act_mirrored(self, obs_m, hist_m=None):
        """the action mean of the MIRRORED observation (`evaluation.asymmetry`): the same weights and kernels as act(), on buffers of its own; no state of act() moves"""
        raise NotImplementedError

    def after_step(self, obs, dones_u8):
        pass


class _MlpPolicy(_Policy):
    """ActorCritic: actions = actor(obs), one launch (go2nn_mlp_forward on the packed weights)"""

    def __init__(self, ev, model):
        super().__init__(ev, model)
        self.actor = PackedMlp(ev.nn, model.actor)
        # empirical observation normalisation (rsl_rl/modules/normalizer.py): a model that has the child gets one go2nn_obs_norm_apply launch (no partial table: the
        # statistics never change during an evaluation) into a scratch buffer in front of the forward kernel — of the raw observation's mirror image too, and of the
        # frame the sensor model delivered.  No child: nothing is allocated or launched.
        self.norm, self._norm_stats, self._norm_out = None, None, {}

    def begin(self, obs):
        self.actor.pack()
        self.norm = getattr(self.model, "obs_normalizer", None)
        if self.norm is not None:          # the CURRENT statistics, on the evaluator's device
            self._norm_stats = (self.norm.mean32.detach().to(obs.device, copy=True), self.norm.inv32.detach().to(obs.device, copy=True), float(self.norm.clip))

    def _normalised(self, obs, key):
        if self.norm is None:
            return obs
        from .._nn import obs_norm_apply, obs_norm_jobs
        mean32, inv32, clip = self._norm_stats
        obs = obs if (obs.is_contiguous() and obs.dtype == torch.float32) else obs.contiguous().float()
        out = self._norm_out.get(key)
        if out is None or out[0].shape != obs.shape:
            out = self._norm_out[key] = [torch.empty_like(obs), None]
        out[1] = obs_norm_jobs([(obs, out[0], mean32, inv32, None, clip)])          # (kept alive with the buffer)
        obs_norm_apply(self.ev.nn, out[1], obs.shape[0], self._stream())
        return out[0]

    def act(self, obs):
        return self.actor.forward(self._normalised(obs, "obs"))

    def act_mirrored(self, obs_m, hist_m=None):
        return self.actor.forward(self._normalised(obs_m, "mirror"))


class _CtsPolicy(_Policy):
    """The CTS family's deployment path (modules/actor_critic_cts.py act_inference): student encoder on the observation history -> normalised latent -> actor([latent | obs]).
    The history ring is the evaluator's (go2sim_history_push, as the CTS runner keeps its own).  A plain Linear / ELU student encoder with an L2 normaliser and the base class's
    actor run as two go2nn_mlp_forward_rows launches; the other members of the family (mixture encoders, mixture actors) run their modules' own inference formulation."""

    def __init__(self, ev, model):
        super().__init__(ev, model)
        from ..rsl_rl.modules.actor_critic_cts import ActorCriticCTS
        from ..rsl_rl.modules.fused_cts import mlp_linears
        N, dev = ev.num_envs, ev.device
        self.H, self.D = model.history_length, model.num_actor_obs
        self.history = torch.zeros(N, self.H, self.D, device=dev)
        t = type(model)
        enc = mlp_linears(model.student_encoder, norm=True) if (t.student_latent is ActorCriticCTS.student_latent and hasattr(model, "student_encoder")) else None
        act = mlp_linears(model.actor) if (t.policy_mean is ActorCriticCTS.policy_mean and hasattr(model, "actor")) else None
        self.kernels = enc is not None and act is not None and act[0].in_features == enc[-1].out_features + self.D
        if self.kernels:
            self.enc, self.actor = PackedMlp(ev.nn, None, linears=enc), PackedMlp(ev.nn, None, linears=act)
            self.L = enc[-1].out_features
            self.latent = torch.zeros(N, self.L, device=dev)
            self.latent_m = torch.zeros(N, self.L, device=dev) if ev.asymmetry else None

    def _push(self, obs, dones_u8):
        lib = self.ev.env.lib
        rc = lib.go2sim_history_push(C.c_void_p(self.history.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(dones_u8.data_ptr()) if dones_u8 is not None else None,
                                     self.ev.num_envs, self.H, self.D, self._stream())
        if rc != 0:
            raise RuntimeError("go2sim_history_push failed: %s" % lib.go2sim_last_error().decode())

    def begin(self, obs):
        self.history.zero_()
        self._push(obs, None)
        if self.kernels:
            self.enc.pack(); self.actor.pack()

    def _rows(self, net, io):
        descs = (C.POINTER(type(net.desc)) * 1)(C.pointer(net.desc))
        packed = (C.c_void_p * 1)(net.packed.data_ptr())
        self._check(self.ev.nn.go2nn_mlp_forward_rows(descs, packed, (Go2nnMlpIO * 1)(io), 1, self._stream()), "go2nn_mlp_forward_rows")

    def act(self, obs):
        N = self.ev.num_envs
        hist = self.history.view(N, self.H * self.D)
        if not self.kernels:
            return self.model.policy_mean(self.model.student_latent(hist)[0], obs).contiguous()
        A = self.actor.out_dim
        actions = torch.empty(N, A, device=obs.device)
        self._rows(self.enc, Go2nnMlpIO(hist.data_ptr(), None, None, self.latent.data_ptr(), self.H * self.D, 0, self.H * self.D, N, self.L, 1))
        self._rows(self.actor, Go2nnMlpIO(self.latent.data_ptr(), obs.data_ptr(), None, actions.data_ptr(), self.L, obs.shape[1], self.L, N, A, 0))
        return actions

    def act_mirrored(self, obs_m, hist_m=None):
        """hist_m [N, H * D]: the mirror image of the history ring act() has just read (the evaluator's mirror launch makes it next to obs_m)"""
        N = self.ev.num_envs
        if not self.kernels:
            return self.model.policy_mean(self.model.student_latent(hist_m)[0], obs_m).contiguous()
        A = self.actor.out_dim
        actions = torch.empty(N, A, device=obs_m.device)
        self._rows(self.enc, Go2nnMlpIO(hist_m.data_ptr(), None, None, self.latent_m.data_ptr(), self.H * self.D, 0, self.H * self.D, N, self.L, 1))
        self._rows(self.actor, Go2nnMlpIO(self.latent_m.data_ptr(), obs_m.data_ptr(), None, actions.data_ptr(), self.L, obs_m.shape[1], self.L, N, A, 0))
        return actions

    def after_step(self, obs, dones_u8):
        self._push(obs, dones_u8)


class _RecurrentPolicy(_Policy):
    """ActorCriticRecurrent: the actor's memory (LSTM / GRU) on the library's cell kernels with a hidden state of the evaluator's own — zero at the start, zeroed on dones —,
    then the actor MLP.  Per layer: gi and gh as one grouped product launch (fp32-MFMA kernels: no split image to keep in step with the weights), one cell launch."""

    def __init__(self, ev, model):
        super().__init__(ev, model)
        from ..rsl_rl.modules.fused_rnn import _layers, check_shape
        mem = model.memory_a
        check_shape(mem)
        self.lstm, self.layers = mem.is_lstm, _layers(mem)
        L, H = mem.rnn.num_layers, mem.rnn.hidden_size
        self.h = torch.zeros(L, ev.num_envs, H, device=ev.device)
        self.c = torch.zeros_like(self.h) if self.lstm else None
        self.actor = PackedMlp(ev.nn, model.actor)

    def begin(self, obs):
        self.h.zero_()
        if self.c is not None:
            self.c.zero_()
        self.actor.pack()

    def act(self, obs):
        nn_, N = self.ev.nn, self.ev.num_envs
        G = 4 if self.lstm else 3
        x = obs
        for l, (ih, hh) in enumerate(self.layers):
            H = self.h.shape[2]
            gi, gh = torch.empty(N, G * H, device=obs.device), torch.empty(N, G * H, device=obs.device)
            for xin, lin, out in ((x, ih, gi), (self.h[l], hh, gh)):
                job = Go2nnFwdJob(xin.data_ptr(), lin.weight.data_ptr(), lin.bias.data_ptr(), out.data_ptr(), N, lin.in_features, lin.out_features, 1, None)
                self._check(nn_.go2nn_linear_elu_forward_group((Go2nnFwdJob * 1)(job), 1, self._stream()), "go2nn_linear_elu_forward_group")
            h, c = self.h[l], (self.c[l] if self.lstm else None)
            p = lambda t: t.data_ptr() if t is not None else None
            job = Go2nnRnnCellJob(p(gi), p(gh), p(h), p(c), p(h), p(c), None, None, None, None, None, None, None, None, N, H, GO2NN_RNN_LSTM if self.lstm else GO2NN_RNN_GRU, 0)
            self._check(nn_.go2nn_rnn_cell_forward((Go2nnRnnCellJob * 1)(job), 1, self._stream()), "go2nn_rnn_cell_forward")
            x = h
        return self.actor.forward(x)

    def act_mirrored(self, obs_m, hist_m=None):
        raise NotImplementedError("evaluation.asymmetry with a recurrent policy: the mirrored observation stream needs a twin hidden state of its own (zeroed on the same "
                                  "dones as act()'s), which the evaluator does not keep yet")

    def after_step(self, obs, dones_u8):
        sts = [self.h] + ([self.c] if self.lstm else [])
        L, N, H = self.h.shape
        arr = (C.c_void_p * len(sts))(*[s.data_ptr() for s in sts])
        self._check(self.ev.nn.go2nn_rnn_reset(arr, len(sts), L, N, H, C.c_void_p(dones_u8.data_ptr()), self._stream()), "go2nn_rnn_reset")


def _make_policy(ev, model):
    from ..rsl_rl.modules import ActorCritic, ActorCriticRecurrent
    from ..rsl_rl.modules.actor_critic_cts import ActorCriticCTS
    if isinstance(model, ActorCriticRecurrent):
        return _RecurrentPolicy(ev, model)
    if isinstance(model, ActorCriticCTS):
        return _CtsPolicy(ev, model)
    if isinstance(model, ActorCritic):
        return _MlpPolicy(ev, model)
    raise TypeError("PolicyEvaluator: no evaluation path for %s (ActorCritic, ActorCriticRecurrent and the ActorCriticCTS family are covered)" % type(model).__name__)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class PolicyEvaluator:
    def __init__(self, env_cfg, evaluation, task_class=None, sim_params=None, device="cuda:0", lib=None, nn_lib=None, step_callback=None, apply_callback=None):
        """env_cfg: the task's env config (copied, never modified);  evaluation: the train config's `evaluation` section (class or dict).
        lib / nn_lib: the go2sim / go2nn libraries — tests hand in the CPU oracle and the host build; the product passes neither and runs on the HIP libraries or not at all.
        step_callback(evaluator, step, counted): called after every eager step with the buffers the accumulate kernel has just read (tests record them).
        apply_callback(evaluator, step, counted): with perturbations / maneuvers, called in every eager step right after go2nn_robust_apply / go2nn_maneuver_apply, before the
        simulator steps."""
        from ..envs.base.legged_robot import LeggedRobot
        self.ev = evaluation
        self.cfg = evaluation_env_cfg(env_cfg, evaluation)
        self.task_class = task_class or LeggedRobot
        self.sim_params = sim_params
        self._lib, self.device_arg = lib, device
        self.step_callback, self.apply_callback = step_callback, apply_callback
        perts = _get(evaluation, "perturbations")
        self.perturbations = [[str(p[0]), dict(p[1] or {})] for p in perts] if perts else None
        self.ladder = bool(_get(evaluation, "ladder", False))
        mans = _get(evaluation, "maneuvers")
        self.maneuvers = [[str(m[0]), [[float(x) for x in seg] for seg in m[1]]] for m in mans] if mans else None
        if self.maneuvers is not None and (self.ladder or self.perturbations is not None):
            raise ValueError("evaluation.maneuvers cannot be combined with evaluation.ladder or evaluation.perturbations: one evaluation splits the robots along ONE extra axis")
        sens = _get(evaluation, "sensors")
        self.sensors = [[str(c[0]), dict(c[1] or {})] for c in sens] if sens else None
        if self.sensors is not None:
            if self.maneuvers is not None or self.ladder or self.perturbations is not None:
                raise ValueError("evaluation.sensors cannot be combined with evaluation.perturbations, evaluation.ladder or evaluation.maneuvers: one evaluation splits the "
                                 "robots along ONE extra axis")
            self._noise_cfg = copy.deepcopy(env_cfg.noise)          # the task's own noise scales, from the config as the task trains with it
            self._noise_cfg.noise_level = 1.0
        if self.ladder:
            self._init_ladder()
        elif self.maneuvers is not None:          # the maneuvers take the scenarios' place: a "scenario" per maneuver, its command that of the first segment
            self._init_maneuvers()
        else:
            self.scenarios = [list(s) for s in (_get(evaluation, "scenarios") or DEFAULT_SCENARIOS)]
        self.terrain_level = int(_get(evaluation, "terrain_level", 5))
        self.num_envs = self.cfg.env.num_envs
        self.env = self._terrain = self.level_of_env = None
        self._make_env()
        self.device = self.env.device
        self.on_device = self.env.lib.go2sim_is_device_library() == 1
        if nn_lib is None:
            if not self.on_device:
                raise RuntimeError("PolicyEvaluator on a host simulator library needs the go2nn host build passed as nn_lib (tests only)")
            from .._nn import load_nn
            nn_lib = load_nn()
        self.nn = nn_lib
        self.dt = float(self.env.dt)
        self.warmup_steps = int(round(float(_get(evaluation, "warmup_s", 1.0)) / self.dt))
        self.steps = max(1, int(round(float(_get(evaluation, "seconds", 10.0)) / self.dt)))
        g = math.gcd(self.warmup_steps, self.steps)
        self.chunk = max(d for d in range(1, min(g, MAX_CHUNK) + 1) if g % d == 0)
        self._build_groups()
        if self.ladder:
            self._place_on_levels()
        N = self.num_envs
        self.acc = torch.zeros(GO2NN_EVAL_NUM, N, device=self.device)
        self.out = torch.zeros(self.num_cells, GO2NN_EVAL_NUM + 2, dtype=torch.float64, device=self.device)
        self.tables = []          # the active _ScoreTable records in begin / reduce order: robust, ladder, maneuver, gait, asym, spectrum, actuator
        if self.perturbations is not None:
            self._build_robust()
        if self.sensors is not None:
            self._build_sensors()
        if self.ladder:
            self._build_ladder()
        if self.maneuvers is not None:
            self._build_maneuvers()
        self.gait = bool(_get(evaluation, "gait", False))
        if self.gait:
            self._build_gait()
        self.actuators = bool(_get(evaluation, "actuators", False))
        if self.axis_key is not None or self.gait or self.actuators:
            self._warn_small_cells()
        self.asymmetry = bool(_get(evaluation, "asymmetry", False))
        if self.asymmetry:
            self._build_asymmetry()
        self.spectrum = bool(_get(evaluation, "spectrum", False))
        if self.spectrum:
            self._build_spectrum()
        self.dof_limits = self.env.dof_pos_limits.contiguous().clone()
        if self.actuators:
            self._build_actuators()
        self._policy, self._policy_of = None, None
        self.recorder = None
        per_group = int(_get(evaluation, "record", 0) or 0)
        if per_group > 0:          # the first `record` env indices of every group, for the counted steps
            from .recorder import TrajectoryRecorder
            ids = np.sort(np.concatenate([np.nonzero(self.cell_host == g)[0][:per_group] for g in range(self.num_cells)]))          # (a cell is a group without perturbations)
            self.recorder = TrajectoryRecorder(self.env, ids, self.steps, nn_lib=self.nn)
        self.blackbox, self.fall_recorder = int(_get(evaluation, "blackbox", 0) or 0), None
        if self.blackbox < 0:
            raise ValueError("evaluation.blackbox: robots kept per cell, >= 0 (0 = off), got %r" % (_get(evaluation, "blackbox"),))
        if self.blackbox > 0:
            self._build_blackbox()
        self.bootstrap = int(_get(evaluation, "bootstrap", 0) or 0)
        if self.bootstrap < 0:
            raise ValueError("evaluation.bootstrap: replicates, >= 0 (0 = off), got %r" % (_get(evaluation, "bootstrap"),))
        if self.bootstrap > 0:
            self._build_bootstrap()
        self.evaluations = 0
        self.last_mode = None          # "eager" / "graph": how the latest evaluation's steps ran

    # ------------------------------------------------------------------ the simulator of one evaluation
    def _make_env(self):
        """a fresh simulator in the evaluation's initial state: same config, same seed, same (host-resident) terrain"""
        if self.env is not None:
            self.env.close()
        if self.cfg.terrain.mesh_type != "plane" and self._terrain is None:
            from .terrain import Terrain
            state = np.random.get_state()          # the terrain generators draw from numpy's global stream: seed it for the evaluation, hand it back untouched
            np.random.seed(self.cfg.seed)
            tcfg = copy.deepcopy(self.cfg.terrain)
            tcfg.curriculum = True                 # the LAYOUT by terrain kind (columns by terrain_proportions, rows by difficulty); nothing moves between levels (below)
            self._terrain = Terrain(tcfg, self.num_envs)
            np.random.set_state(state)
        sp = self.sim_params
        if sp is None:
            from .helpers import SimParams
            sim = class_to_dict(self.cfg.sim)
            sp = SimParams(dt=sim.get("dt", 0.005), substeps=sim.get("substeps", 1), gravity=sim.get("gravity", (0.0, 0.0, -9.81)))
        cls = type("_Eval" + self.task_class.__name__, (self.task_class,), {"_terrain_prebuilt": self._terrain})
        kw = {} if self._lib is None else {"lib": self._lib}
        self.env = cls(cfg=self.cfg, sim_params=sp, physics_engine=1, sim_device=self.device_arg, headless=True, **kw)
        env = self.env
        if self.ladder:                 # every env on its cell's level (known once the groups are built: __init__ places the first simulator's robots itself)
            if self.level_of_env is not None:
                self._place_on_levels()
        elif env.custom_origins:        # every env at the evaluation's terrain level, in the column the simulator gave it
            lv = min(max(self.terrain_level, 0), self.cfg.terrain.num_rows - 1)
            env.terrain_levels.fill_(lv)
            env.env_origins.copy_(env.terrain_origins[lv, env.terrain_types])

    def _init_ladder(self):
        """the ladder's own settings, checked before anything is built: scenarios, levels, clearing distance, pass share"""
        ev, t = self.ev, self.cfg.terrain
        if t.mesh_type not in ("heightfield", "trimesh"):
            raise ValueError("evaluation.ladder needs a task with terrain levels (terrain.mesh_type heightfield / trimesh), got mesh_type = %r" % (t.mesh_type,))
        if self.perturbations is not None:
            raise ValueError("evaluation.ladder and evaluation.perturbations cannot be combined: one evaluation splits the robots along ONE extra axis")
        self.scenarios = [list(s) for s in (_get(ev, "ladder_scenarios") or DEFAULT_LADDER_SCENARIOS)]
        levels = _get(ev, "ladder_levels")
        self.levels = [int(l) for l in (range(int(t.num_rows)) if levels is None else levels)]
        if not self.levels or sorted(set(self.levels)) != self.levels or self.levels[0] < 0 or self.levels[-1] >= int(t.num_rows):
            raise ValueError("evaluation.ladder_levels: increasing rows of the terrain grid inside 0 .. %d, got %r" % (int(t.num_rows) - 1, levels))
        dist = _get(ev, "ladder_distance")
        self.ladder_distance = float(t.terrain_length) * 0.5 if dist is None else float(dist)
        self.ladder_pass_share = float(_get(ev, "ladder_pass_share", 0.5))
        if not self.ladder_distance > 0.0:
            raise ValueError("evaluation.ladder_distance: a distance > 0 [m], got %r" % (dist,))
        seconds = float(_get(ev, "seconds", 10.0))
        for s in self.scenarios:
            reach = math.hypot(float(s[1]), float(s[2])) * seconds
            if reach <= self.ladder_distance:
                print("[go2_rl_gym_amd] evaluation: ladder scenario %r covers at most %.2f m in %.1f s at its command and cannot clear the %.2f m of evaluation.ladder_distance; "
                      "raise evaluation.seconds" % (s[0], reach, seconds, self.ladder_distance))

    def _init_maneuvers(self):
        """the maneuvers' shape, checked before anything is built (the schedule in steps needs the simulator's dt: _build_maneuvers)"""
        mans = self.maneuvers
        names = [m[0] for m in mans]
        if len(mans) > GO2NN_MANEUVER_MAX_SPECS:
            raise ValueError("evaluation.maneuvers: at most %d maneuvers, got %d" % (GO2NN_MANEUVER_MAX_SPECS, len(mans)))
        if len(set(names)) != len(names):
            raise ValueError("evaluation.maneuvers: the maneuvers need distinct names, got %r" % (names,))
        for name, segs in mans:
            if not 1 <= len(segs) <= GO2NN_MANEUVER_MAX_SEGS or any(len(seg) != 4 for seg in segs):
                raise ValueError("maneuver %r: 1 .. %d segments [seconds, vx, vy, yaw rate], got %r" % (name, GO2NN_MANEUVER_MAX_SEGS, segs))
            if segs[0][0] != 0.0:
                raise ValueError("maneuver %r: the first segment starts at 0 s, got %r" % (name, segs[0][0]))
        self.scenarios = [[name] + segs[0][1:4] for name, segs in mans]

    def _build_maneuvers(self):
        """the maneuvers as the kernels read them: M specs and the env -> maneuver map in device memory, the per-env table and the reduce output"""
        ev, mans, M = self.ev, self.maneuvers, len(self.maneuvers)
        steps_of = lambda seconds: int(round(float(seconds) / self.dt))
        window, hold = max(1, steps_of(_get(ev, "maneuver_window_s", 3.0))), max(1, steps_of(_get(ev, "maneuver_hold_s", 0.3)))
        thr_lin, thr_ang = float(_get(ev, "maneuver_thr_lin", 0.3)), float(_get(ev, "maneuver_thr_ang", 0.3))
        if window < hold or not (thr_lin > 0.0 and thr_ang > 0.0):
            raise ValueError("evaluation: maneuver_window_s (%d steps) must not be shorter than maneuver_hold_s (%d steps), and maneuver_thr_lin = %r, maneuver_thr_ang = %r "
                             "must be > 0" % (window, hold, thr_lin, thr_ang))
        specs = (Go2nnManeuverSpec * M)()
        self.switch_steps = {}
        for sp, (name, segs) in zip(specs, mans):
            starts = [steps_of(seg[0]) for seg in segs]
            if any(b <= a for a, b in zip(starts, starts[1:])):
                raise ValueError("maneuver %r: the segments' times must increase by at least one step of %.3f s, got %r" % (name, self.dt, [seg[0] for seg in segs]))
            # the window of the switch at step s ends with the accumulate call of step s + window - 1: inside its segment and inside the horizon
            for k in range(1, len(starts)):
                end = starts[k + 1] if k + 1 < len(starts) else self.steps
                if starts[k] + window > end:
                    raise ValueError("maneuver %r: the %.2f s window of the switch at %.2f s does not close before %s at %.2f s; shorten evaluation.maneuver_window_s, move the "
                                     "switch or raise evaluation.seconds" % (name, window * self.dt, segs[k][0], "the next switch" if k + 1 < len(starts) else "the horizon's end",
                                                                             end * self.dt))
            sp.count, sp.window, sp.hold, sp.thr_lin, sp.thr_ang = len(segs), window, hold, thr_lin, thr_ang
            for k, seg in enumerate(segs):
                sp.start[k] = starts[k]
                sp.cmd[k][:] = seg[1:4]
            self.switch_steps[name] = starts[1:]
        self._check(self.nn.go2nn_maneuver_check_specs(C.cast(specs, C.c_void_p), M), "go2nn_maneuver_check_specs")
        self.maneuver_window, self.maneuver_hold, self.maneuver_thr = window, hold, (thr_lin, thr_ang)
        self.mspecs_host = specs
        self.mspecs = torch.from_numpy(np.frombuffer(bytes(specs), np.uint8).copy()).to(self.device)
        self.man_host = (self.group_host % M).astype(np.int32)
        self.man = torch.from_numpy(self.man_host).to(self.device)
        self.mtable = torch.zeros(GO2NN_MANEUVER_NUM, self.num_envs, device=self.device)
        self.mout = torch.zeros(self.num_cells, GO2NN_MANEUVER_ACC_NUM + 1, dtype=torch.float64, device=self.device)
        self.tables.append(_ScoreTable("maneuver", self._maneuver_in, self.mtable, self.mout, args=(self.mspecs, self.man)))

    def _place_on_levels(self):
        """the ladder's env placement on the current simulator: every env on its cell's row of the terrain grid, in the column the simulator gave it"""
        env = self.env
        lv = torch.from_numpy(self.level_of_env).to(env.terrain_levels.device)
        env.terrain_levels.copy_(lv.to(env.terrain_levels.dtype))
        env.env_origins.copy_(env.terrain_origins[lv.long(), env.terrain_types.long()])

    def _build_ladder(self):
        """the ladder's device side: the per-env table, the reduce output, the squared clearing distance as the kernel compares it"""
        self.dist2_thr = float(np.float32(self.ladder_distance) * np.float32(self.ladder_distance))
        self.ltable = torch.zeros(GO2NN_LADDER_NUM, self.num_envs, device=self.device)
        self.lout = torch.zeros(self.num_cells, GO2NN_LADDER_OUT_NUM, dtype=torch.float64, device=self.device)
        self.tables.append(_ScoreTable("ladder", self._ladder_in, self.ltable, self.lout, reduce_args=(self.dist2_thr,)))

    def _build_groups(self):
        """env -> (terrain kind x scenario) group, built once on the host: the kinds are those of the columns the envs stand in (one kind, 'plane', without a terrain mesh);
        within a kind the envs take the scenarios in turn, so the groups of a kind differ by at most one env.  With P perturbations (or P sensor conditions) they take the (scenario, perturbation)
        CELLS in turn; cell index = (terrain * S + scenario) * P + perturbation — the kernels' group —, and a group is the union of its P cells (P = 1 without).
        With the ladder's L levels they take the (level, scenario) cells in turn; cell index = (terrain * L + level) * S + scenario, a group is the union of its L cells.
        The layout is kept for everything that reshapes a cell table or names a cell: T, S, P, L, the extra axis's result key `axis_key`, its values' names `axis_names`
        and `cell_axes`, what a cell is"""
        from .terrain import KIND_NAMES
        N, S, P = self.num_envs, len(self.scenarios), len(self.perturbations or self.sensors or [None])
        L = len(self.levels) if self.ladder else 1
        if self.ladder:
            self.axis_key, self.axis_names, self.cell_axes = "ladder", list(self.levels), ["terrain", "level", "scenario"]
        elif self.maneuvers is not None:          # (a "scenario" is a maneuver there)
            self.axis_key, self.axis_names, self.cell_axes = "maneuvers", [m[0] for m in self.maneuvers], ["terrain", "maneuver"]
        elif self.perturbations is not None or self.sensors is not None:
            self.axis_key, self.cell_axes = ("perturbations", ["terrain", "scenario", "perturbation"]) if self.perturbations is not None else ("sensors", ["terrain", "scenario", "sensor"])
            self.axis_names = [p[0] for p in (self.perturbations or self.sensors)]
        else:
            self.axis_key, self.axis_names, self.cell_axes = None, [], ["terrain", "scenario"]
        if self.env.custom_origins:
            kind_of_env = self.env.terrain_cols2id.cpu().numpy()[self.env.terrain_types.cpu().numpy()]
            kinds = [int(k) for k in sorted(set(kind_of_env.tolist()))]
            self.terrain_names = [KIND_NAMES[k] if 0 <= k < len(KIND_NAMES) else "kind_%d" % k for k in kinds]
        else:
            kind_of_env, kinds, self.terrain_names = np.zeros(N, np.int64), [0], ["plane"]
        group = np.zeros(N, np.int32)
        scen, pert, level = np.zeros(N, np.int64), np.zeros(N, np.int32), np.zeros(N, np.int64)
        for ki, k in enumerate(kinds):
            ids = np.nonzero(kind_of_env == k)[0]
            if self.ladder:
                turn = np.arange(len(ids)) % (L * S)
                level[ids], scen[ids] = turn // S, turn % S
            else:
                turn = np.arange(len(ids)) % (S * P)
                scen[ids], pert[ids] = turn // P, turn % P
            group[ids] = ki * S + scen[ids]
        self.groups = [(t, s[0]) for t in self.terrain_names for s in self.scenarios]
        self.T, self.S, self.P, self.L = len(self.terrain_names), S, P, L
        self.group_host, self.pert_host = group, pert
        self.cell_host, self.num_cells = group * P + pert, len(self.groups) * P
        if self.ladder:          # level_index_host: index into self.levels;  level_of_env: the row of the terrain grid itself
            self.level_index_host, self.level_of_env = level, np.asarray(self.levels, np.int64)[level]
            self.cell_host, self.num_cells = (((group // S) * L + level) * S + scen).astype(np.int32), len(self.groups) * L
        self.group = torch.from_numpy(self.cell_host).to(self.device)          # what the reduce kernels group by
        cmd = np.zeros((N, 4), np.float32)
        cmd[:, :3] = np.asarray([s[1:4] for s in self.scenarios], np.float32)[scen]
        self.commands_host = cmd
        self.commands = torch.from_numpy(cmd).to(self.device)

    def _warn_small_cells(self):
        """said once per evaluator, of the finest cells the mode has — or, without a mode, of the groups the gait figures are pooled over"""
        sizes = np.bincount(self.cell_host, minlength=self.num_cells)
        if sizes.min() < 4:
            axes = " x ".join(self.cell_axes) + (" condition" if self.axis_key == "sensors" else "")
            pooled = " and ".join(n for n, on in (("gait", self.gait), ("actuator", self.actuators)) if on)
            what = "cells have fewer than 4 robots (smallest: %d)" if self.axis_key is not None else "groups have fewer than 4 robots (smallest: %d) for the " + pooled + " figures"
            print("[go2_rl_gym_amd] evaluation: %d of %d (%s) %s; raise evaluation.num_envs" % (int((sizes < 4).sum()), self.num_cells, axes, what % int(sizes.min())))

    def _cell_views(self, cells, pool=np.sum):
        """cells [..., num_cells, cols]: a reduce table per cell (the bootstrap's with its replicate axis in front);  pool(a, axis): stacked rows -> the row of their union
        -> (the per-group table [..., T * S, cols]: the cells pooled over the extra axis, the per-cell view: [..., T, L, S, cols] with the ladder, [..., T * S, P, cols] without)"""
        lead = cells.shape[:-2]
        if self.ladder:
            view = cells.reshape(lead + (self.T, self.L, self.S, -1))
            return pool(view, len(lead) + 1).reshape(lead + (self.T * self.S, -1)), view
        view = cells.reshape(lead + (self.T * self.S, self.P, -1))          # P = 1: the cells' rows themselves
        return pool(view, len(lead) + 1), view

    def _build_robust(self):
        """the perturbations as the kernels read them: P specs and the env -> perturbation map in device memory, the per-env table and the reduce output"""
        ev, perts, P = self.ev, self.perturbations, len(self.perturbations)
        if P > GO2NN_ROBUST_MAX_SPECS or len({p[0] for p in perts}) != P:
            raise ValueError("evaluation.perturbations: 1 .. %d perturbations with distinct names, got %r" % (GO2NN_ROBUST_MAX_SPECS, [p[0] for p in perts]))
        steps_of = lambda key, default: int(round(float(_get(ev, key, default)) / self.dt))
        first, period, window = steps_of("push_first_s", 1.0), max(1, steps_of("push_period_s", 2.5)), max(1, steps_of("push_window_s", 2.0))
        hold, thr = max(1, steps_of("recover_hold_s", 0.2)), float(_get(ev, "recover_thr", 0.3))
        # every window closes inside the horizon: the window of the push at step s ends with the accumulate call of step s + window - 1
        count = (self.steps - first - window) // period + 1 if self.steps - first - window >= 0 else 0
        self.push_first, self.push_period, self.push_window, self.push_hold, self.push_count = first, period, window, hold, count
        self.push_steps = np.asarray([first + k * period for k in range(count)], np.int64)
        specs = (Go2nnRobustSpec * P)()
        for sp, (name, fields) in zip(specs, perts):
            unknown = set(fields) - {"dv"} - set(ROBUST_MASK)
            if unknown:
                raise ValueError("perturbation %r: unknown field(s) %s (dv, %s)" % (name, sorted(unknown), ", ".join(ROBUST_MASK)))
            sp.dv[:] = [float(x) for x in fields.get("dv", (0.0, 0.0, 0.0))]
            sp.first, sp.period, sp.count, sp.window, sp.hold, sp.thr = first, period, count, window, hold, thr
            sp.strength, sp.kp_mul, sp.kd_mul, sp.added_mass, sp.friction = 1.0, 1.0, 1.0, 0.0, 1.0
            for k, bit in ROBUST_MASK.items():
                if k in fields:
                    setattr(sp, k, float(fields[k]))
                    sp.mask |= bit
        self._check(self.nn.go2nn_robust_check_specs(C.cast(specs, C.c_void_p), P), "go2nn_robust_check_specs")
        self.specs_host = specs
        self.specs = torch.from_numpy(np.frombuffer(bytes(specs), np.uint8).copy()).to(self.device)
        self.pert = torch.from_numpy(self.pert_host).to(self.device)
        self.rtable = torch.zeros(GO2NN_ROBUST_NUM, self.num_envs, device=self.device)
        self.rout = torch.zeros(self.num_cells, GO2NN_ROBUST_ACC_NUM + 1, dtype=torch.float64, device=self.device)
        self.tables.append(_ScoreTable("robust", self._robust_in, self.rtable, self.rout, args=(self.specs, self.pert)))

    def _build_sensors(self):
        """the sensor conditions as the kernel reads them: P specs (observation scales folded in), the env -> condition map, the observation's layout (kind, the task's noise
        vector at noise_level 1), the state allocation and the delivered frame [N, D] — a fixed address, so a captured policy launch keeps reading it"""
        conds, P, env = self.sensors, len(self.sensors), self.env
        if P > GO2NN_SENSOR_MAX_SPECS or len({c[0] for c in conds}) != P:
            raise ValueError("evaluation.sensors: 1 .. %d conditions with distinct names, got %r" % (GO2NN_SENSOR_MAX_SPECS, [c[0] for c in conds]))
        D = int(env.num_obs)
        if D != len(GO2_OBS_KINDS) or not hasattr(env, "_get_noise_scale_vec"):
            raise ValueError("evaluation.sensors: no observation layout for %s with %d observation columns (the Go2 layout of envs/go2/go2_env.py is covered)"
                             % (type(env).__name__, D))
        scale = env._get_noise_scale_vec(types.SimpleNamespace(noise=self._noise_cfg)).detach().cpu().numpy().astype(np.float32)
        kind = np.asarray([SENSOR_KINDS.index(k) for k in GO2_OBS_KINDS], np.int32)
        o = self.cfg.normalization.obs_scales
        specs = (Go2nnSensorSpec * P)()
        for sp, (name, fields) in zip(specs, conds):
            unknown = set(fields) - set(SENSOR_FIELDS)
            if unknown:
                raise ValueError("sensor condition %r: unknown field(s) %s (%s)" % (name, sorted(unknown), ", ".join(SENSOR_FIELDS)))
            delay = fields.get("delay", 0)
            if int(delay) != delay:
                raise ValueError("sensor condition %r: delay = %r (whole policy steps, 0 .. %d)" % (name, delay, GO2NN_SENSOR_MAX_DELAY))
            sp.noise_mul, sp.gravity_bias, sp.delay, sp.drop = float(fields.get("noise", 0.0)), float(fields.get("gravity_bias", 0.0)), int(delay), float(fields.get("drop", 0.0))
            sp.gyro_bias, sp.joint_offset = float(fields.get("gyro_bias", 0.0)) * float(o.ang_vel), float(fields.get("joint_offset", 0.0)) * float(o.dof_pos)
        self._check(self.nn.go2nn_sensor_check_specs(C.cast(specs, C.c_void_p), P, C.c_void_p(kind.ctypes.data), C.c_void_p(scale.ctypes.data), D), "go2nn_sensor_check_specs")
        self.sspecs_host, self.sensor_kind_host, self.sensor_scale_host = specs, kind, scale
        self.sspecs = torch.from_numpy(np.frombuffer(bytes(specs), np.uint8).copy()).to(self.device)
        self.sensor_kind, self.sensor_scale = torch.from_numpy(kind).to(self.device), torch.from_numpy(scale).to(self.device)
        self.sensor_host = self.pert_host          # the condition of every env (the cells' last axis)
        self.sensor_of_env = torch.from_numpy(self.sensor_host).to(self.device)
        self.sstate = torch.zeros(int(self.nn.go2nn_sensor_state_bytes(self.num_envs, D)), dtype=torch.uint8, device=self.device)
        self.delivered = torch.zeros(self.num_envs, D, device=self.device)
        self.sensor_clip, self.sensor_seed = float(self.cfg.normalization.clip_observations), int(_get(self.ev, "seed", 12345)) & 0xFFFFFFFF

    def _build_gait(self):
        """the gait scorer's device side: the per-env table, the reduce output per cell, the feet in foot_body order and the two diagonal pairs among them by NAME"""
        env = self.env
        self.gait_threshold = float(_get(self.ev, "gait_contact_threshold", 1.0))
        if not (math.isfinite(self.gait_threshold) and self.gait_threshold >= 0.0):
            raise ValueError("evaluation.gait_contact_threshold: a finite force >= 0 [N], got %r" % (_get(self.ev, "gait_contact_threshold"),))
        self.gait_feet = [int(i) for i in env.feet_indices.tolist()]
        self.foot_names = [str(env.body_names[i]).replace("_foot", "") for i in self.gait_feet]
        masks = []
        for pair in DIAGONAL_PAIRS:
            at = [[f for f, n in enumerate(self.foot_names) if n.upper().startswith(leg)] for leg in pair]
            if len(self.gait_feet) != 4 or any(len(a) != 1 for a in at):
                raise ValueError("evaluation.gait: the feet %r do not name one FL, FR, RL and RR foot each" % (self.foot_names,))
            masks.append((1 << at[0][0]) | (1 << at[1][0]))
        self.gait_diagonal = masks
        self.gtable = torch.zeros(GO2NN_GAIT_NUM, self.num_envs, device=self.device)
        self.gout = torch.zeros(self.num_cells, GO2NN_GAIT_OUT_NUM, dtype=torch.float64, device=self.device)
        self.tables.append(_ScoreTable("gait", self._gait_in, self.gtable, self.gout))

    def _build_asymmetry(self):
        """the asymmetry scorer's device side: the mirror tables of the task's layout (any other layout raises mirror_tables' ValueError), the sides of the feet by NAME,
        the per-env table, the reduce output per cell and the buffer the mirror launch writes the observation and its mirror image to"""
        from .symmetry import joint_kinds, joint_sides, leg_side, mirror_tables
        from .._nn import mirror_table_tensors
        env, N = self.env, self.num_envs
        self.asym_tables = mirror_tables(self.cfg)
        perm, sign = self.asym_tables.action
        if len(perm) != 12:
            raise ValueError("evaluation.asymmetry: the kernel scores 12 joints, the action table has %d" % len(perm))
        self.asym_feet = [int(i) for i in env.feet_indices.tolist()]
        names = [str(env.body_names[i]) for i in self.asym_feet]
        if len(names) != 4:
            raise ValueError("evaluation.asymmetry: four feet are needed, got %r" % (names,))
        self.asym_foot_side = [leg_side(n) for n in names]
        if sum(self.asym_foot_side) != 0:
            raise ValueError("evaluation.asymmetry: the feet %r are not two left and two right ones" % (names,))
        self.asym_joint_side, self.asym_joint_kind = joint_sides().tolist(), joint_kinds().tolist()
        self.asym_threshold = float(_get(self.ev, "gait_contact_threshold", 1.0))
        if not (math.isfinite(self.asym_threshold) and self.asym_threshold >= 0.0):
            raise ValueError("evaluation.gait_contact_threshold: a finite force >= 0 [N], got %r" % (_get(self.ev, "gait_contact_threshold"),))
        self.asym_obs_table = mirror_table_tensors(self.nn, self.asym_tables.obs, self.device)
        self.atable = torch.zeros(GO2NN_ASYM_NUM, N, device=self.device)
        self.aout = torch.zeros(self.num_cells, GO2NN_ASYM_OUT_NUM, dtype=torch.float64, device=self.device)
        self.asym_obs = torch.zeros(2, N, len(self.asym_tables.obs[0]), device=self.device)          # [0]: the copy half of go2nn_mirror_rows, [1]: the mirror image
        self.asym_hist = self.asym_hist_table = self.asym_last = None
        self.tables.append(_ScoreTable("asym", self._asym_in, self.atable, self.aout))

    def _asym_in(self):
        """the asymmetry kernel's view of the simulator's buffers (as _gait_in) and its small tables, by value"""
        b = self.env._buf
        a, d = _field_views(Go2nnAsymIn(), b, ASYM_FIELDS, last=True), b["dof_state"]
        a.dof_state.comp_stride, a.dof_vel_offset, a.contact_body_stride = d.stride(1), d.stride(2), b["contact_forces"].stride(1)
        a.foot_body[:], a.foot_side[:], a.joint_side[:], a.joint_kind[:] = self.asym_feet, self.asym_foot_side, self.asym_joint_side, self.asym_joint_kind
        a.action_perm[:], a.action_sign[:] = [int(p) for p in self.asym_tables.action[0]], [float(s) for s in self.asym_tables.action[1]]
        a.contact_threshold = self.asym_threshold
        return a

    def _asym_jobs(self, pol, obs):
        """the one mirror launch of a step: the observation the policy reads and, for a policy with a history ring (CTS), the ring -> the go2nn_mirror_rows job array"""
        from .symmetry import history_table
        from .._nn import mirror_jobs, mirror_table_tensors
        pairs = [(obs, self.asym_obs, self.asym_obs_table)]
        hist = getattr(pol, "history", None)
        if hist is not None:
            N, H, D = hist.shape
            if self.asym_hist is None or tuple(self.asym_hist.shape) != (2, N, H * D):
                self.asym_hist = torch.zeros(2, N, H * D, device=self.device)
                self.asym_hist_table = mirror_table_tensors(self.nn, history_table(self.asym_tables.obs, H), self.device)
            pairs.append((hist.view(N, H * D), self.asym_hist, self.asym_hist_table))
        return mirror_jobs(pairs), (self.asym_hist[1] if hist is not None else None)

    def _build_blackbox(self):
        """the black box's device side: a ring of `blackbox_seconds` for every robot (utils/recorder.py FallRecorder), refused before anything is allocated when it is too
        short to show a fall or larger than `blackbox_max_bytes`; and what a cell is called in the falls table"""
        from .recorder import FallRecorder
        from .._nn import GO2NN_TRACE_WIDTH
        seconds, cap = float(_get(self.ev, "blackbox_seconds", 2.0)), int(_get(self.ev, "blackbox_max_bytes", 512 * 1024 * 1024))
        T = int(round(seconds / self.dt))
        if T < 2:
            raise ValueError("evaluation.blackbox_seconds = %r is %d steps of %.4f s: the ring needs at least 2 (the fall frame and one frame before it)" % (seconds, T, self.dt))
        need = self.num_envs * T * GO2NN_TRACE_WIDTH * 4
        if need > cap:
            raise ValueError("evaluation.blackbox: %d robots x %d steps x %d bytes per frame = %d bytes, more than evaluation.blackbox_max_bytes = %d; shorten "
                             "evaluation.blackbox_seconds or lower evaluation.num_envs" % (self.num_envs, T, GO2NN_TRACE_WIDTH * 4, need, cap))
        self.fall_recorder = FallRecorder(self.env, T, nn_lib=self.nn)
        self.cell_names = self._cell_names()

    def _cell_names(self):
        """what a cell of the finest partition is called, in cell order"""
        if self.ladder:
            names = ["%s/level_%d/%s" % (t, lv, s[0]) for t in self.terrain_names for lv in self.levels for s in self.scenarios]
        else:
            axis = self.axis_names if self.axis_key in ("perturbations", "sensors") else [None]          # (a maneuver is the cell's scenario itself)
            names = ["%s/%s" % (t, s[0]) + ("/" + p if p is not None else "") for t in self.terrain_names for s in self.scenarios for p in axis]
        assert len(names) == self.num_cells == self.T * self.S * self.L * self.P
        return names

    def _build_bootstrap(self):
        """the bootstrap's device side: the cells' member lists (CSR, env indices ascending within a cell; checked on the host, the launch cannot report a bad index) and
        the [B, cells, 12] fp64 table, refused before anything is allocated when it is larger than `bootstrap_max_bytes`"""
        B, cols = self.bootstrap, GO2NN_EVAL_NUM + 2
        self.confidence = float(_get(self.ev, "confidence", 0.95))
        if not 0.0 < self.confidence < 1.0:
            raise ValueError("evaluation.confidence: an interval level inside (0, 1), got %r" % (_get(self.ev, "confidence"),))
        self.bootstrap_seed = int(_get(self.ev, "bootstrap_seed", 2718)) & 0xFFFFFFFF
        need, cap = B * self.num_cells * cols * 8, int(_get(self.ev, "bootstrap_max_bytes", 256 << 20))
        self.bootstrap_all = bool(_get(self.ev, "bootstrap_all", False))
        if self.bootstrap_all:          # the cap holds the SUM of all tables; the refusal names each table's share, before anything is allocated
            share = [("eval", cols)] + [(t.name, int(t.out.shape[1])) for t in self.tables if t.resampled]
            total = sum(B * self.num_cells * c * 8 for _, c in share)
            if total > cap or any(B * self.num_cells * c >= 2 ** 31 for _, c in share):
                raise ValueError("evaluation.bootstrap_all: %d replicates x %d cells x 8 bytes x (%s) = %d bytes, more than evaluation.bootstrap_max_bytes = %d (or a table "
                                 "of 2^31 values); lower evaluation.bootstrap" % (B, self.num_cells, " + ".join("%s: %d columns = %d bytes" % (n, c, B * self.num_cells * c * 8)
                                                                                                               for n, c in share), total, cap))
        if need > cap or B * self.num_cells * cols >= 2 ** 31:
            raise ValueError("evaluation.bootstrap: %d replicates x %d cells x %d columns x 8 bytes = %d bytes, more than evaluation.bootstrap_max_bytes = %d (or 2^31 values); "
                             "lower evaluation.bootstrap" % (B, self.num_cells, cols, need, cap))
        sizes = np.bincount(self.cell_host, minlength=self.num_cells)
        self.cell_start_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.cell_envs_host = np.argsort(self.cell_host, kind="stable").astype(np.int32)
        self._check(self.nn.go2nn_eval_bootstrap_check(C.c_void_p(self.cell_start_host.ctypes.data), C.c_void_p(self.cell_envs_host.ctypes.data), self.num_envs, self.num_cells),
                    "go2nn_eval_bootstrap_check")
        self.cell_start, self.cell_envs = torch.from_numpy(self.cell_start_host).to(self.device), torch.from_numpy(self.cell_envs_host).to(self.device)
        self.boot_out = torch.zeros(B, self.num_cells, cols, dtype=torch.float64, device=self.device)
        if self.bootstrap_all:          # one more [B, cells, cols] table per active scoring family, in the families' reduce order
            self.boot_outs = {t.name: torch.zeros(B, self.num_cells, int(t.out.shape[1]), dtype=torch.float64, device=self.device) for t in self.tables if t.resampled}

    def _build_spectrum(self):
        """the spectrum scorer's device side: the trace of the counted steps (refused before it is allocated when larger than `spectrum_max_bytes`), the twiddle table, the
        per-robot table and the reduce output per cell"""
        from .symmetry import joint_kinds
        ev = self.ev
        W = _get(ev, "spectrum_window", 64)
        if isinstance(W, bool) or not isinstance(W, (int, np.integer)) or W % 2 or not GO2NN_SPECTRUM_MIN_WINDOW <= W <= GO2NN_SPECTRUM_MAX_WINDOW:
            raise ValueError("evaluation.spectrum_window: an even number of policy steps in [%d, %d], got %r" % (GO2NN_SPECTRUM_MIN_WINDOW, GO2NN_SPECTRUM_MAX_WINDOW, W))
        self.spectrum_window, self.spectrum_fs = int(W), 1.0 / self.dt
        try:
            cutoff = float(_get(ev, "spectrum_cutoff_hz", 10.0))
        except (TypeError, ValueError):
            cutoff = float("nan")
        if not (math.isfinite(cutoff) and 0.0 < cutoff <= 0.5 * self.spectrum_fs):
            raise ValueError("evaluation.spectrum_cutoff_hz: a frequency in (0, fs / 2 = %g] Hz, got %r" % (0.5 * self.spectrum_fs, _get(ev, "spectrum_cutoff_hz")))
        self.spectrum_cutoff = cutoff
        cap = _get(ev, "spectrum_max_bytes", 512 << 20)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 1:
            raise ValueError("evaluation.spectrum_max_bytes: a number of bytes >= 1, got %r" % (cap,))
        N, T = self.num_envs, self.steps
        need = spectrum_trace_rows(T) * N * 4
        if need > int(cap) or T > GO2NN_SPECTRUM_MAX_STEPS:
            raise ValueError("evaluation.spectrum: the trace of %d counted steps x %d robots x 25 floats = %d bytes, more than evaluation.spectrum_max_bytes = %d (or more than "
                             "2^20 steps); lower evaluation.num_envs or evaluation.seconds" % (T, N, need, int(cap)))
        kinds = [int(k) for k in joint_kinds()]
        self.spectrum_slots = [j for kind in range(len(SPECTRUM_KINDS)) for j in range(12) if kinds[j] == kind]          # hips, thighs, calves: four joints each
        if len(self.spectrum_slots) != 12 or any(kinds.count(k) != 4 for k in range(3)) or self.env.num_actions != 12:
            raise ValueError("evaluation.spectrum: 12 joints, four of each kind (utils/symmetry.py joint_kinds), got %r" % (kinds,))
        self.strace = torch.zeros(spectrum_trace_rows(T), N, device=self.device)
        self.stwiddle = torch.from_numpy(spectrum_twiddle(self.spectrum_window)).to(self.device)
        self.stable = torch.zeros(spectrum_rows(self.spectrum_window), N, device=self.device)
        self.sout = torch.zeros(self.num_cells, 1 + spectrum_rows(self.spectrum_window), dtype=torch.float64, device=self.device)
        self.tables.append(_ScoreTable("spectrum", self._spectrum_in, self.stable, self.sout, reduce_args=(self.spectrum_window,), state=self.strace, begin_args=(T,),
                                       resampled=False))

    def _build_actuators(self):
        """the actuator scorer's device side: the per-robot table, the reduce output per cell, the limits and the two saturation thresholds as the kernel compares them
        (fp32 products formed once, here), the joints and feet by NAME, and the rows the extremes are read from"""
        env, ev = self.env, self.ev
        raw = _get(ev, "actuators_saturation", 0.95)
        try:
            sat = float(raw)
        except (TypeError, ValueError):
            sat = float("nan")
        if isinstance(raw, bool) or not (math.isfinite(sat) and 0.0 < sat <= 1.0):
            raise ValueError("evaluation.actuators_saturation: the share of a joint's torque / speed limit from which a sample counts as saturated, finite and in (0, 1], got %r" % (raw,))
        self.act_saturation = sat
        self.act_threshold = float(_get(ev, "gait_contact_threshold", 1.0))
        if not (math.isfinite(self.act_threshold) and self.act_threshold >= 0.0):
            raise ValueError("evaluation.gait_contact_threshold: a finite force >= 0 [N], got %r" % (_get(ev, "gait_contact_threshold"),))
        host = lambda t: t.detach().cpu().numpy().astype(np.float32)
        self.act_torque_limits, self.act_vel_limits, pos = host(env.torque_limits), host(env.dof_vel_limits), host(self.dof_limits)
        if self.act_torque_limits.shape != (12,) or self.act_vel_limits.shape != (12,) or pos.shape != (12, 2) or env.num_actions != 12:
            raise ValueError("evaluation.actuators: the kernel scores 12 joints, got torque limits %s, speed limits %s, position limits %s"
                             % (self.act_torque_limits.shape, self.act_vel_limits.shape, pos.shape))
        self.act_pos_lo, self.act_pos_hi = pos[:, 0].copy(), pos[:, 1].copy()
        self.act_tau_thr, self.act_vel_thr = np.float32(sat) * self.act_torque_limits, np.float32(sat) * self.act_vel_limits
        self.joint_names = [str(n).replace("_joint", "") for n in env.dof_names]
        if len(self.joint_names) != 12 or any(sum(k in n for k in ACTUATOR_KINDS) != 1 for n in self.joint_names) or len(set(self.joint_names)) != 12:
            raise ValueError("evaluation.actuators: the joints %r do not name one hip, thigh or calf each" % (self.joint_names,))
        self.act_feet = [int(i) for i in env.feet_indices.tolist()]
        if len(self.act_feet) != 4:
            raise ValueError("evaluation.actuators: four feet are needed, got bodies %r" % (self.act_feet,))
        self.act_foot_names = [str(env.body_names[i]).replace("_foot", "") for i in self.act_feet]
        self.act_table = torch.zeros(GO2NN_ACTUATOR_NUM, self.num_envs, device=self.device)
        self.act_out = torch.zeros(self.num_cells, GO2NN_ACTUATOR_OUT_NUM, dtype=torch.float64, device=self.device)
        self.act_extreme_rows = torch.tensor([actuator_row("used")] + ACTUATOR_MAX_ROWS + ACTUATOR_MIN_ROWS, dtype=torch.long, device=self.device)
        self.tables.append(_ScoreTable("actuator", self._actuator_in, self.act_table, self.act_out))

    def _actuator_in(self):
        """the actuator kernel's view of the simulator's buffers (as _asym_in) and its limits, by value"""
        b = self.env._buf
        a, d = _field_views(Go2nnActuatorIn(), b, ACTUATOR_FIELDS, last=True), b["dof_state"]
        a.dof_state.comp_stride, a.dof_vel_offset, a.contact_body_stride = d.stride(1), d.stride(2), b["contact_forces"].stride(1)
        a.foot_body[:], a.contact_threshold = self.act_feet, self.act_threshold
        a.pos_lo[:], a.pos_hi[:], a.tau_sat_thr[:], a.vel_sat_thr[:] = self.act_pos_lo.tolist(), self.act_pos_hi.tolist(), self.act_tau_thr.tolist(), self.act_vel_thr.tolist()
        return a

    def _spectrum_in(self):
        """the record kernel's view of the simulator's buffers (as _eval_in) and the joints in slot order"""
        a = _field_views(Go2nnSpectrumIn(), self.env._buf, SPECTRUM_FIELDS)
        a.joint_of_slot[:] = self.spectrum_slots
        return a

    def _spectrum_welch(self):
        """the per-robot table from the trace of the counted steps: one launch, after the last step and outside any capture"""
        self._check(self.nn.go2nn_spectrum_welch(C.c_void_p(self.strace.data_ptr()), self.num_envs, self.steps, self.spectrum_window, self.spectrum_fs,
                                                 C.c_void_p(self.stwiddle.data_ptr()), C.c_void_p(self.stable.data_ptr()), self._stream()), "go2nn_spectrum_welch")

    def _keep_fallen(self, fell):
        """of the fallen robots, per cell of the finest partition the mode reports, the `blackbox` lowest env indices"""
        cells = self.cell_host[fell]
        return np.sort(np.concatenate([fell[cells == c][:self.blackbox] for c in np.unique(cells)])) if len(fell) else fell

    def _label(self, d, ids):
        """what a trace and a falls dict say about their robots `ids`: group, and with the mode's extra axis its value per robot and its schedule"""
        d.update(group_of_robot=self.group_host[ids].copy(), terrain_names=list(self.terrain_names), scenarios=[s[0] for s in self.scenarios])
        key, names = self.axis_key, list(self.axis_names)
        if key == "ladder":
            d.update(levels=names, level_of_robot=self.level_of_env[ids].copy())
        elif key == "perturbations":          # push_steps: the counted steps (= frame indices) whose go2nn_robust_apply pushed; the frame holds the state AFTER that step
            d.update(perturbations=names, pert_of_robot=self.pert_host[ids].copy(), push_steps=self.push_steps.copy())
        elif key == "sensors":
            d.update(sensors=names, sensor_of_robot=self.sensor_host[ids].copy())
        elif key == "maneuvers":
            # switch_steps [M, GO2NN_MANEUVER_MAX_SEGS - 1] int32: per maneuver the counted steps (= frame indices) at which a new segment begins — that frame carries the
            # new command —, padded with -1 (a rectangular array: maneuvers differ in their number of switches, and the trace goes to an .npz)
            steps = np.full((len(self.maneuvers), GO2NN_MANEUVER_MAX_SEGS - 1), -1, np.int32)
            for mi, m in enumerate(self.maneuvers):
                steps[mi, :len(self.switch_steps[m[0]])] = self.switch_steps[m[0]]
            d.update(maneuvers=names, maneuver_of_robot=self.man_host[ids].copy(), switch_steps=steps)

    def _gait_in(self):
        """the gait kernel's view of the simulator's buffers (as TrajectoryRecorder.bind: component and body strides of the two per-body fields)"""
        b = self.env._buf
        a = _field_views(Go2nnGaitIn(), b, GAIT_FIELDS, last=True)
        a.rigid_body_stride, a.contact_body_stride = b["rigid_body_states"].stride(1), b["contact_forces"].stride(1)
        a.foot_body[:], a.diagonal_mask[:], a.contact_threshold = self.gait_feet, self.gait_diagonal, self.gait_threshold
        return a

    def _sensor_in(self):
        """the sensor kernel's view of the current simulator: its observation and reset flags, and the evaluator's own layout tensors"""
        t = self.env.obs_buf
        a = _field_views(Go2nnSensorIn(), {"obs": t}, ("obs",))
        a.dones, a.scale, a.kind = self.env._buf["reset_buf"].data_ptr(), self.sensor_scale.data_ptr(), self.sensor_kind.data_ptr()
        a.D, a.num_specs, a.clip, a.seed = t.shape[1], len(self.sensors), self.sensor_clip, self.sensor_seed
        return a

    def _sensor_apply(self, sin):
        self._check(self.nn.go2nn_sensor_apply(C.byref(sin), C.c_void_p(self.sspecs.data_ptr()), C.c_void_p(self.sensor_of_env.data_ptr()), C.c_void_p(self.sstate.data_ptr()),
                                               C.c_void_p(self.delivered.data_ptr()), self.num_envs, self._stream()), "go2nn_sensor_apply")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.on_device else None

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self.nn.go2nn_last_error().decode()))

    def _robust_in(self):
        """the perturbation kernels' view of the simulator's buffers (as _eval_in)"""
        a = _field_views(Go2nnRobustIn(), self.env._buf, ROBUST_FIELDS)
        a.num_specs = len(self.perturbations)
        return a

    def _ladder_in(self):
        """the ladder kernel's view of the simulator's buffers (as _eval_in)"""
        a = _field_views(Go2nnLadderIn(), self.env._buf, LADDER_FIELDS)
        a.dist2_thr = self.dist2_thr
        return a

    def _maneuver_in(self):
        """the maneuver kernels' view of the simulator's buffers (as _eval_in)"""
        a = _field_views(Go2nnManeuverIn(), self.env._buf, MANEUVER_FIELDS)
        a.num_specs, a.num_commands = len(self.maneuvers), self.env._buf["commands"].shape[1]
        return a

    def _eval_in(self):
        """the accumulate kernel's view of the simulator's buffers (_field_views; its `last_actions` is EVAL_SOURCE's buffer)"""
        a = _field_views(Go2nnEvalIn(), self.env._buf, EVAL_FIELDS, source=EVAL_SOURCE)
        a.dof_vel_offset = self.env._buf["dof_state"].stride(2)
        a.dof_limits, a.dt = self.dof_limits.data_ptr(), self.dt
        return a

    def _table_launch(self, what, t, tin, *extra):
        """one launch of a score table's step: go2nn_<name>_<what>(input, the table's own arguments, [extra,] table, N, stream), `what` being "apply" or "accumulate" """
        name = "go2nn_%s_%s" % (t.name, what)
        self._check(getattr(self.nn, name)(C.byref(tin), *t.args, *extra, C.c_void_p(t.table.data_ptr()), self.num_envs, self._stream()), name)

    # ------------------------------------------------------------------ one env step of the evaluation (pure enqueue)
    def _step(self, pol, run, k=None):
        """run: what evaluate() made for this evaluation — `ein`, `sin` (the eval and sensor kernels' inputs; sin None without sensors: the policy then reads the simulator's
        observation itself), the active score tables as (record, input) pairs: `applied` (maneuver or robust: the one that acts before the simulator steps), `maneuver`,
        `scored` (robust, ladder, gait), `asym` (each None / empty when off), and for the asymmetry `jobs` (the mirror launch's) and `hist_m` (the mirrored history or None);
        k: the step's index in an eager run (None inside a capture: no callback there)"""
        env = self.env
        obs = env.obs_buf if run.sin is None else self.delivered
        actions = pol.act(obs)
        if run.asym is not None:          # the mirror image of what act() has just read, and the same weights on it; nothing act() owns moves
            mirror_rows(self.nn, run.jobs, 1, self.num_envs, self._stream())
            mirrored = pol.act_mirrored(self.asym_obs[1], run.hist_m)
        if run.applied is not None:
            self._table_launch("apply", *run.applied)
            if k is not None and self.apply_callback is not None:
                self.apply_callback(self, k, k >= self.warmup_steps)
        _abi.check(env.lib, env.lib.go2sim_step(env.handle, C.c_void_p(actions.data_ptr()), self._stream()), "go2sim_step")
        if run.maneuver is not None:          # (it rewrites the command row itself: the maneuver's command at this step)
            self._table_launch("accumulate", *run.maneuver)
        else:
            env.commands.copy_(self.commands)          # a robot that fell was reset by the step and drew a new command: the scenario's command holds
        if run.sin is not None:          # the frame the policy gets NEXT step, and what its history / memory is fed below
            self._sensor_apply(run.sin)
        self._check(self.nn.go2nn_eval_accumulate(C.byref(run.ein), C.c_void_p(self.acc.data_ptr()), self.num_envs, self._stream()), "go2nn_eval_accumulate")
        for pair in run.scored:
            self._table_launch("accumulate", *pair)
        if run.asym is not None:
            self._table_launch("accumulate", *run.asym, C.c_void_p(actions.data_ptr()), C.c_void_p(mirrored.data_ptr()))
            self.asym_last = (actions, mirrored)          # (what a step_callback of a test reads next to asym_obs)
        if run.spectrum is not None:          # this step's actions, torques and reset flags into the trace, behind the trace's own step counter
            self._check(self.nn.go2nn_spectrum_record(C.byref(run.spectrum[1]), C.c_void_p(self.strace.data_ptr()), self.num_envs, self.steps, self._stream()), "go2nn_spectrum_record")
        if self.recorder is not None:
            self.recorder.record()
        if self.fall_recorder is not None:
            self.fall_recorder.record()
        pol.after_step(obs, env._buf["reset_buf"])

    def _clear(self):
        self._check(self.nn.go2nn_eval_clear(C.c_void_p(self.acc.data_ptr()), self.num_envs, self._stream()), "go2nn_eval_clear")
        if self.recorder is not None:
            self.recorder.clear()

    def _run_eager(self, pol, run):
        for k in range(self.warmup_steps + self.steps):
            if k == self.warmup_steps:
                self._clear()
            self._step(pol, run, k)
            if self.step_callback is not None:
                self.step_callback(self, k, k >= self.warmup_steps)

    def _run_graph(self, pol, run):
        """capture `chunk` steps on this evaluation's simulator, replay them for the whole horizon -> False if the capture failed (nothing has run then)"""
        from ..rsl_rl.algorithms._graph import no_gc, strict_graphs
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        try:
            with no_gc(), torch.cuda.graph(g):
                for _ in range(self.chunk):
                    self._step(pol, run)
        except Exception as e:      # noqa: BLE001
            if strict_graphs():
                raise RuntimeError("HIP-graph capture of the evaluation failed (%s: %s)" % (type(e).__name__, e)) from e
            print("[go2_rl_gym_amd] HIP-graph capture of the evaluation failed (%s: %s); evaluating eagerly" % (type(e).__name__, e))
            torch.cuda.synchronize(self.device)
            return False
        for k in range(0, self.warmup_steps + self.steps, self.chunk):
            if k == self.warmup_steps:
                self._clear()
            g.replay()
            self.env.lib.go2sim_notify_replayed(self.env.handle, self.chunk)
        self._graph = g          # alive until the results have been read
        return True

    # ------------------------------------------------------------------ the public call
    def evaluate(self, actor_critic, use_graph=None):
        """-> {"overall": {...}, "groups": {terrain: {scenario: {...}}}, "terrain_names", "scenarios", "steps", "dt", "mode"}; every leaf dict has RESULT_KEYS.
        With `evaluation.ladder` also "ladder": {terrain: {level: {scenario: {RESULT_KEYS + LADDER_KEYS}}}}, "ladder_summary": {terrain: {LADDER_SUMMARY_KEYS}}, "levels",
        "ladder_table" (go2nn_ladder_reduce's raw output per cell) and "ladder_distance"; "overall" gains `cleared` and `mean_level_cleared`.
        With `evaluation.maneuvers` every leaf of "groups" (a "scenario" being a maneuver) and "overall" gain MANEUVER_KEYS; also "maneuvers": {name: {RESULT_KEYS +
        MANEUVER_KEYS}} over the terrains, "maneuver_table" (go2nn_maneuver_reduce's raw output per cell) "switch_steps": {name: [counted steps]}, "maneuver_schedule": {name: [[step, vx, vy, yaw rate], ...]} and "maneuver_rule" (window and hold in steps, the thresholds).
        A trace gains "maneuvers", "maneuver_of_robot" and "switch_steps" (int32 [M, 7], padded with -1).
        With `evaluation.sensors` also "cells": {terrain: {scenario: {condition: {RESULT_KEYS}}}}, "sensors": {condition: {RESULT_KEYS}} over the terrains and scenarios,
        "sensor_names", "sensor_specs": {condition: {SENSOR_FIELDS}} and "cell_table" (go2nn_eval_reduce's raw output per cell).  A trace gains "sensors" and "sensor_of_robot".
        With `evaluation.gait` also "gait": {"overall": {...}, "groups": {terrain: {scenario: {...}}}} and, under the mode's own keys, "perturbations" / "sensors" /
        "maneuvers": {name: {...}}, "cells": {terrain: {scenario: {name: {...}}}}, "ladder": {terrain: {level: {scenario: {...}}}}; every leaf has GAIT_KEYS, "<key>/<foot>"
        for GAIT_FOOT_KEYS and "n_envs"; "gait_table" (go2nn_gait_reduce's raw output per cell), "gait_cells" (what a cell is: its axes' names), "foot_names"; "overall"
        gains GAIT_KEYS.
        With `evaluation.asymmetry` also "asymmetry": the same tree as "gait" ("overall", "groups" and the mode's own keys), every leaf with ASYM_KEYS and "n_envs";
        "asymmetry_table" (go2nn_asym_reduce's raw output per cell), "asymmetry_cells" and "asymmetry_contact_threshold".  "overall" gains nothing.
        With `evaluation.spectrum` also "spectrum": the same tree as "gait", every leaf with SPECTRUM_KEYS, "<key>/<kind>" for the three joint kinds, SPECTRUM_COUNT_KEYS and
        "n_envs"; "spectrum_table" (go2nn_spectrum_reduce's raw output per cell), "spectrum_cells", "spectrum_settings" {"window", "cutoff_hz", "fs"} and "spectrum_psd"
        (what eval_results/spectrum_<it>.npz holds: "freqs" [K], the mean power spectrum "psd" [cells, 2, 3, K], the cell, signal and kind names); "overall" gains SPECTRUM_KEYS.
        With `evaluation.actuators` also "actuators": the same tree as "gait", every leaf with ACTUATOR_KEYS and ACTUATOR_EXTREME_KEYS over all joints / feet, per joint kind,
        per joint and per foot, and "n_envs"; "actuator_table" (go2nn_actuator_reduce's raw output per cell), "actuator_extremes" (per cell the 28 maxima and 12 minima
        behind the extremes; -inf / +inf for a cell without a used robot), "actuator_cells" and "actuator_settings" (the limits, the thresholds, the names).  "overall" gains nothing.
        With `evaluation.record` also "trace": TrajectoryRecorder.fetch() of the counted steps plus "group_of_robot" (index into terrain_names x scenarios, terrain-major,
        per tracked robot), "terrain_names" and "scenarios".
        With `evaluation.blackbox` also "falls": FallRecorder.fetch() of the kept fallen robots plus the labels a trace gets, "cell_names", "cell_of_robot",
        "fell_per_cell" (robots that fell per cell, kept or not) and "kept_per_cell".
        With `evaluation.bootstrap` also "bootstrap": {"replicates", "seed", "confidence", "table" (go2nn_eval_bootstrap's raw output, float64 [B, cells, 12]), "overall"
        (float64 [B, 12]: the overall row of every replicate; replicate_metrics() turns it into the figures' replicates)}, and every leaf dict with RESULT_KEYS gains
        "ci": {metric: [lo, hi]} for CI_KEYS.
        With `evaluation.bootstrap_all` too "bootstrap" gains "tables": {family: go2nn_<family>_bootstrap's raw output, float64 [B, cells, cols]} and "metrics": {figure:
        float64 [B]}, the "ci" of every leaf that reports a family's figures gains them, every leaf of "gait" and "asymmetry" gains a "ci", and every entry of
        "ladder_summary" gains "ci": {"level_cleared", "mean_level_cleared"}.
        use_graph: None = eager, or with `evaluation.replay` eager the first time and a captured chunk afterwards (on the GPU); True / False force it."""
        with torch.inference_mode():
            if self.evaluations > 0:
                self._make_env()
            if self._policy_of is not actor_critic:
                self._policy, self._policy_of = _make_policy(self, actor_critic), actor_critic
            pol, env = self._policy, self.env
            if self.asymmetry and isinstance(pol, _RecurrentPolicy):          # refused before anything runs
                pol.act_mirrored(None)
            _abi.check(env.lib, env.lib.go2sim_reset_all(env.handle, self._stream()), "go2sim_reset_all")
            env.commands.copy_(self.commands)
            zero = torch.zeros(self.num_envs, env.num_actions, device=self.device)
            _abi.check(env.lib, env.lib.go2sim_step(env.handle, C.c_void_p(zero.data_ptr()), self._stream()), "go2sim_step")          # BaseTask.reset: the first observations
            env.commands.copy_(self.commands)
            sin = None
            if self.sensors is not None:          # the policy's first observation and the CTS history's first frame are sensor frames: step 0 of the sensor's own cursor
                sin = self._sensor_in()
                self._check(self.nn.go2nn_sensor_begin(C.c_void_p(self.sstate.data_ptr()), self._stream()), "go2nn_sensor_begin")
                self._sensor_apply(sin)
            pol.begin(env.obs_buf if sin is None else self.delivered)
            if self.recorder is not None:
                self.recorder.bind(env)
            self._clear()
            # every score table's step counter starts at -warmup_steps and its kernels advance it: nothing is pushed, switched or counted before step 0 (the ladder takes the
            # distance's origin there, the gait opens every foot's first segment there), and no table is cleared at the boundary
            pairs = [(t, t.make_in()) for t in self.tables]
            by = {t.name: (t, tin) for t, tin in pairs}
            run = types.SimpleNamespace(ein=self._eval_in(), sin=sin, tables=pairs, maneuver=by.get("maneuver"), applied=by.get("maneuver") or by.get("robust"),
                                        scored=[by[n] for n in ("robust", "ladder", "gait", "actuator") if n in by], asym=by.get("asym"), spectrum=by.get("spectrum"), jobs=None, hist_m=None)
            if run.asym is not None:
                run.jobs, run.hist_m = self._asym_jobs(pol, env.obs_buf if sin is None else self.delivered)
            for t, _ in pairs:
                self._check(getattr(self.nn, "go2nn_%s_begin" % t.name)(C.c_void_p(t.state.data_ptr()), self.num_envs, -self.warmup_steps, *t.begin_args, self._stream()), "go2nn_%s_begin" % t.name)
            if self.fall_recorder is not None:          # as above; NOT cleared at the warm-up boundary: a ring's history runs through it
                self.fall_recorder.bind(env)
                self.fall_recorder.begin(-self.warmup_steps)
            replay = bool(_get(self.ev, "replay", False))
            graph = (replay and self.on_device and self.evaluations > 0 and self.step_callback is None) if use_graph is None else bool(use_graph and self.on_device)
            done = graph and self._run_graph(pol, run)
            if not done:
                self._run_eager(pol, run)
            self.last_mode = "graph" if done else "eager"
            self._check(self.nn.go2nn_eval_reduce(C.c_void_p(self.acc.data_ptr()), C.c_void_p(self.group.data_ptr()), self.num_envs, self.num_cells,
                                                  C.c_void_p(self.out.data_ptr()), self._stream()), "go2nn_eval_reduce")
            if self.bootstrap > 0:          # the same accumulators, the same cells: B resampled reduce tables (after the replayed chunks, never inside a capture)
                self._check(self.nn.go2nn_eval_bootstrap(C.c_void_p(self.acc.data_ptr()), C.c_void_p(self.cell_start.data_ptr()), C.c_void_p(self.cell_envs.data_ptr()),
                                                         self.num_envs, self.num_cells, self.bootstrap, self.bootstrap_seed, C.c_void_p(self.boot_out.data_ptr()), self._stream()),
                            "go2nn_eval_bootstrap")
            host, bhost = {}, {}
            boot_all = self.bootstrap > 0 and self.bootstrap_all
            if run.spectrum is not None:
                self._spectrum_welch()
            for t, _ in pairs:
                self._check(getattr(self.nn, "go2nn_%s_reduce" % t.name)(C.c_void_p(t.table.data_ptr()), C.c_void_p(self.group.data_ptr()), self.num_envs, self.num_cells,
                                                                         *t.reduce_args, C.c_void_p(t.out.data_ptr()), self._stream()), "go2nn_%s_reduce" % t.name)
                if boot_all and t.resampled:          # the family's reduce rows of the SAME redrawn robots (outside any capture, as go2nn_eval_bootstrap above)
                    self._check(getattr(self.nn, "go2nn_%s_bootstrap" % t.name)(C.c_void_p(t.table.data_ptr()), C.c_void_p(self.cell_start.data_ptr()), C.c_void_p(self.cell_envs.data_ptr()),
                                                                                self.num_envs, self.num_cells, self.bootstrap, self.bootstrap_seed, *t.reduce_args,
                                                                                C.c_void_p(self.boot_outs[t.name].data_ptr()), self._stream()), "go2nn_%s_bootstrap" % t.name)
                host[t.name] = t.out.cpu().numpy().copy()
                if boot_all and t.resampled:
                    bhost[t.name] = self.boot_outs[t.name].cpu().numpy().copy()
            if run.asym is not None:
                self.asym_last = None
            # the actuators' extremes: ONE more device -> host copy, of the USED row and the 28 + 12 peak and margin rows of every robot
            extremes = self.act_table.index_select(0, self.act_extreme_rows).cpu().numpy() if "actuator" in by else None
            table = self.out.cpu().numpy().copy()          # the device -> host copy (and synchronisation) of an evaluation
            btable = self.boot_out.cpu().numpy().copy() if self.bootstrap > 0 else None
            trace = self.recorder.fetch() if self.recorder is not None else None
            falls = self.fall_recorder.fetch(self._keep_fallen) if self.fall_recorder is not None else None
            self._graph = None
            self.evaluations += 1
        res = self._results(table, host.get("robust"), host.get("ladder"), host.get("maneuver"))
        if btable is not None:
            self._bootstrap_results(res, btable)
        if "gait" in host:
            self._gait_results(res, host["gait"])
        if "asym" in host:
            self._asym_results(res, host["asym"])
        if "spectrum" in host:
            self._spectrum_results(res, host["spectrum"])
        if "actuator" in host:
            self._actuator_results(res, host["actuator"], extremes)
        if btable is not None and self.bootstrap_all:
            self._bootstrap_all_results(res, btable, bhost)
        if trace is not None:
            self._label(trace, trace["env_ids"])
            res["trace"] = trace
        if falls is not None:          # the kept robots' labels, and per cell how many robots fell (kept or not)
            self._label(falls, falls["env_ids"])
            falls.update(cell_names=list(self.cell_names), cell_of_robot=self.cell_host[falls["env_ids"]].copy(),
                         fell_per_cell=np.bincount(self.cell_host[falls["fell_env_ids"]], minlength=self.num_cells).astype(np.int64), kept_per_cell=self.blackbox)
            res["falls"] = falls
        return res

    @staticmethod
    def _row(r):
        """one row of the reduce table (sums of the ten accumulators, envs, envs without a fall) -> the reported figures; an empty group reports NaN (as episode_info does)"""
        n, steps = float(r[GO2NN_EVAL_NUM]), float(r[0])
        d = {m: (float(r[1 + i]) / steps if steps > 0 else float("nan")) for i, m in enumerate(MEAN_METRICS)}
        d["falls"] = float(r[EVAL_METRICS.index("falls")]) / n if n > 0 else float("nan")
        d["survival"] = float(r[GO2NN_EVAL_NUM + 1]) / n if n > 0 else float("nan")
        d["n_envs"] = int(n)
        return d

    def _robust_row(self, r):
        """one row of go2nn_robust_reduce (sums of the six accumulators, envs) -> the per-push figures; without a push (a recovered push) they are NaN"""
        pushes, rec = float(r[0]), float(r[2])
        per_push = lambda x: float(x) / pushes if pushes > 0 else float("nan")
        return {"pushes": int(pushes), "push_falls": per_push(r[1]), "recovered": per_push(r[2]), "recovery_time_s": float(r[3]) / rec * self.dt if rec > 0 else float("nan"),
                "peak_lin_vel_err": per_push(r[4]), "peak_tilt": per_push(r[5])}

    def _maneuver_row(self, r):
        """one row of go2nn_maneuver_reduce (MANEUVER_OUT) -> the per-switch figures; NaN without a switch, without a settled switch (settle_time_s), without a window step"""
        v = {k: float(r[i]) for i, k in enumerate(MANEUVER_OUT)}
        sw, settled, steps = v["switches"], v["settled"], v["win_steps"]
        per = lambda x, n: x / n if n > 0 else float("nan")
        return {"switches": int(sw), "switch_falls": per(v["switch_falls"], sw), "settled": per(settled, sw), "settle_time_s": per(v["settle_steps"], settled) * self.dt,
                "window_lin_vel_err": per(v["win_lin_err"], steps), "window_ang_vel_err": per(v["win_ang_err"], steps), "peak_tilt": per(v["peak_tilt_sum"], sw)}

    def _ladder_row(self, r):
        """one row of go2nn_ladder_reduce (LADDER_OUT) -> the cell's shares; an empty cell reports NaN, and so does time_to_clear_s without a cleared robot"""
        n, cleared = float(r[LADDER_OUT.index("n")]), float(r[LADDER_OUT.index("cleared")])
        share = lambda k: float(r[LADDER_OUT.index(k)]) / n if n > 0 else float("nan")
        return {"cleared": share("cleared"), "fell": share("fell"), "timed_out": share("timed_out"),
                "time_to_clear_s": float(r[LADDER_OUT.index("clear_steps")]) / cleared * self.dt if cleared > 0 else float("nan"), "progress": share("progress")}

    def _ladder_results(self, res, cells, lcells):
        """cells / lcells: the eval / ladder reduce tables per (terrain, level, scenario) cell -> the ladder's entries of the result"""
        c4, l4 = self._cell_views(cells)[1], self._cell_views(lcells)[1]
        res["ladder"] = {t: {lv: {s[0]: dict(self._row(c4[ti, li, si]), **self._ladder_row(l4[ti, li, si])) for si, s in enumerate(self.scenarios)}
                             for li, lv in enumerate(self.levels)} for ti, t in enumerate(self.terrain_names)}
        first = self.scenarios[0][0]
        summary = {}
        for t in self.terrain_names:          # over the FIRST ladder scenario; an empty cell (cleared = NaN) has cleared nothing
            curve = [res["ladder"][t][lv][first]["cleared"] for lv in self.levels]
            curve = [0.0 if math.isnan(c) else c for c in curve]
            top = -1
            for lv, c in zip(self.levels, curve):
                if c < self.ladder_pass_share:
                    break
                top = lv
            summary[t] = {"level_cleared": int(top), "mean_level_cleared": float(sum(curve))}
        res["ladder_summary"] = summary
        whole = lcells.sum(0)
        res["overall"].update(cleared=self._ladder_row(whole)["cleared"], mean_level_cleared=float(np.mean([v["mean_level_cleared"] for v in summary.values()])))
        res.update(levels=list(self.levels), ladder_table=lcells, ladder_cell_table=cells, ladder_distance=self.ladder_distance, ladder_pass_share=self.ladder_pass_share)

    def _gait_row(self, r):
        """one row of go2nn_gait_reduce, or a sum of rows -> the pooled figures: GAIT_FOOT_KEYS per foot ("<key>/<foot>") and over the four feet, GAIT_PATTERN_KEYS, n_envs;
        NaN where the denominator is 0"""
        r = np.asarray(r, np.float64)
        per = lambda x, n: float(x) / float(n) if n > 0 else float("nan")
        feet = np.stack([r[gait_out_col(f, GAIT_OUT_FOOT[0]):gait_out_col(f, GAIT_OUT_FOOT[0]) + len(GAIT_OUT_FOOT)] for f in range(4)])
        d = {}
        for name, row in [("", feet.sum(0))] + [("/" + n, feet[f]) for f, n in enumerate(self.foot_names)]:
            v = dict(zip(GAIT_OUT_FOOT, row))
            d["duty_factor" + name] = per(v["contact"], v["used"])
            d["stride_frequency" + name] = per(v["strides"], v["stride_steps"] * self.dt)
            d["stance_time" + name] = per(v["stance_steps"] * self.dt, v["stances"])
            d["swing_time" + name] = per(v["swing_steps"] * self.dt, v["swings"])
            d["slip_speed" + name] = per(v["slip_sum"], v["contact"])
            d["swing_height" + name] = per(v["height_sum"], v["swings"])
            d["swing_clearance" + name] = per(v["clearance_sum"], v["swings"])
            d["touchdowns_per_s" + name] = per(v["touchdowns"], v["used"] * self.dt)
        frames, support = feet[0, 0], r[GO2NN_GAIT_OUT_SUPPORT0:GO2NN_GAIT_OUT_SUPPORT0 + 5]          # (used is the env's own count, the same under every foot)
        d["trot_share"], d["flight_share"] = per(r[GO2NN_GAIT_OUT_DIAGONAL], frames), per(support[0], frames)
        d["mean_feet_in_contact"] = per(float(np.dot(np.arange(5.0), support)), frames)
        d["n_envs"] = int(r[0])
        return d

    def _addon_tree(self, cells, row, pool=np.sum):
        """cells: an add-on's reduce table per cell of the active mode;  pool(a, axis): stacked rows -> the row of their union (a sum in fp64);  row: such a row -> its figures.
        -> ({"overall", "groups" and the mode's own keys: `row` of every partition the mode reports}, what a cell is: its axes' names)"""
        T, S, key, names = self.T, self.S, self.axis_key, self.axis_names
        table, view = self._cell_views(cells, pool)
        tree = {"overall": row(pool(table, 0)), "groups": {t: {s[0]: row(table[ti * S + si]) for si, s in enumerate(self.scenarios)} for ti, t in enumerate(self.terrain_names)}}
        if key in ("perturbations", "sensors"):
            tree["cells"] = {t: {s[0]: {n: row(view[ti * S + si, pi]) for pi, n in enumerate(names)} for si, s in enumerate(self.scenarios)} for ti, t in enumerate(self.terrain_names)}
            tree[key] = {n: row(pool(view[:, pi], 0)) for pi, n in enumerate(names)}
        elif key == "ladder":
            tree["ladder"] = {t: {lv: {s[0]: row(view[ti, li, si]) for si, s in enumerate(self.scenarios)} for li, lv in enumerate(names)} for ti, t in enumerate(self.terrain_names)}
        elif key == "maneuvers":          # (a "scenario" is a maneuver there)
            tree["maneuvers"] = {n: row(pool(table.reshape(T, S, -1)[:, si], 0)) for si, n in enumerate(names)}
        return tree, list(self.cell_axes)

    def _gait_results(self, res, gcells):
        """gcells: go2nn_gait_reduce's table per cell of the active mode -> res["gait"]: the cells' rows summed in fp64 for every partition the mode reports"""
        gait, axes = self._addon_tree(gcells, self._gait_row)
        res["overall"].update({k: gait["overall"][k] for k in GAIT_KEYS})
        res.update(gait=gait, gait_table=gcells, gait_cells=axes, foot_names=list(self.foot_names), gait_contact_threshold=self.gait_threshold)

    @staticmethod
    def _asym_pool(rows, axis=0):
        """stacked rows of go2nn_asym_reduce -> the row of their union along `axis` (not the last): every column a sum, eq_max the max"""
        rows = np.asarray(rows, np.float64)
        out, c = rows.sum(axis), ASYM_OUT.index("eq_max")
        out[..., c] = rows[..., c].max(axis)
        return out

    @staticmethod
    def _asym_row(r):
        """one row of go2nn_asym_reduce, or a pooled one (_asym_pool) -> ASYM_KEYS and n_envs: pooled ratios of the sums, NaN where nothing was counted"""
        v = dict(zip(ASYM_OUT, (float(x) for x in r)))
        per = lambda x, n: x / n if n > 0 else float("nan")
        root = lambda x: math.sqrt(x) if x == x else x
        steps = v["eq_steps"]
        d = {"equivariance_rmse": root(per(v["eq_sq"], 12.0 * steps))}
        for kind in ("hip", "thigh", "calf"):
            d["equivariance_rmse/" + kind] = root(per(v["eq_sq_" + kind], 4.0 * steps))
        d["equivariance_rel"] = root(per(v["eq_sq"], v["act_sq"]))
        d["equivariance_max"] = v["eq_max"] if steps > 0 else float("nan")
        d["sym_steps_share"] = per(v["sym_steps"], steps)
        for x, p in zip(ASYM_LOADS, ASYM_PAIRS):
            d["left_share/" + x] = per(v[p + "_l"], v[p + "_l"] + v[p + "_r"])
        for x, p in zip(ASYM_LOADS, ASYM_PAIRS):
            d["imbalance/" + x] = per(v[p + "_imb"], v[p + "_imb_n"])
        d["n_envs"] = int(v["n"])
        return d

    def _asym_results(self, res, acells):
        """acells: go2nn_asym_reduce's table per cell of the active mode -> res["asymmetry"]: the cells' rows pooled for every partition the mode reports.
        res["overall"] is left as it is: with the flag on every other result is that of the flag-off run"""
        asym, axes = self._addon_tree(acells, self._asym_row, self._asym_pool)
        res.update(asymmetry=asym, asymmetry_table=acells, asymmetry_cells=axes, asymmetry_contact_threshold=self.asym_threshold)

    def _spectrum_row(self, r):
        """one row of go2nn_spectrum_reduce, or a sum of rows -> SPECTRUM_KEYS pooled over the three joint kinds and per kind ("<key>/<kind>"), SPECTRUM_COUNT_KEYS and
        n_envs: ratios of the sums, NaN where nothing was counted (no used window, or no power to take a share of).  Bins k >= 1 only: the DC bin holds what the Hann
        window leaves of the removed mean"""
        r = np.asarray(r, np.float64)
        W, fs, K = self.spectrum_window, self.spectrum_fs, spectrum_bins(self.spectrum_window)
        per = lambda x, n: float(x) / float(n) if n > 0 else float("nan")
        f = np.arange(1, K, dtype=np.float64) * (fs / W)
        high = f >= self.spectrum_cutoff
        used, skipped = r[1 + GO2NN_SPECTRUM_USED], r[1 + GO2NN_SPECTRUM_SKIPPED]
        d = {}
        for si, sig in enumerate(SPECTRUM_SIGNALS):
            P = np.stack([r[1 + spectrum_row(W, "P", si, ki, 1):1 + spectrum_row(W, "P", si, ki, 0) + K] for ki in range(len(SPECTRUM_KINDS))])
            M = np.stack([r[1 + spectrum_row(W, "M", si, ki, 1):1 + spectrum_row(W, "M", si, ki, 0) + K] for ki in range(len(SPECTRUM_KINDS))])
            for name, p, m, joints in [("", P.sum(0), M.sum(0), 12.0)] + [("/" + kind, P[ki], M[ki], 4.0) for ki, kind in enumerate(SPECTRUM_KINDS)]:
                total, n = float(p.sum()), joints * used          # n: the (window, joint) pairs the sums run over
                d["%s_hf_share%s" % (sig, name)] = per(p[high].sum(), total)
                d["%s_centroid_hz%s" % (sig, name)] = per(float(np.dot(f, p)), total)
                d["%s_smoothness%s" % (sig, name)] = per(2.0 / ((W // 2) * fs) * float(np.dot(f, m)), n)
                d["%s_power%s" % (sig, name)] = per((fs / W) * total, n)
        d["spectrum_windows"] = int(used)
        d["spectrum_skipped_share"] = per(skipped, used + skipped)
        d["n_envs"] = int(r[0])
        return d

    def _spectrum_results(self, res, scells):
        """scells: go2nn_spectrum_reduce's table per cell of the active mode -> res["spectrum"]: the cells' rows summed in fp64 for every partition the mode reports;
        res["overall"] gains the pooled figures SPECTRUM_KEYS"""
        spec, axes = self._addon_tree(scells, self._spectrum_row)
        res["overall"].update({k: spec["overall"][k] for k in SPECTRUM_KEYS})
        W, K = self.spectrum_window, spectrum_bins(self.spectrum_window)
        used = scells[:, 1 + GO2NN_SPECTRUM_USED][:, None, None, None]
        first = 1 + spectrum_row(W, "P", 0, 0)
        psd = scells[:, first:first + 6 * K].reshape(-1, len(SPECTRUM_SIGNALS), len(SPECTRUM_KINDS), K)
        psd = np.divide(psd, 4.0 * used, out=np.full(psd.shape, np.nan), where=used > 0)          # the mean over the used windows and a kind's 4 joints
        settings = {"window": W, "cutoff_hz": self.spectrum_cutoff, "fs": self.spectrum_fs}
        res.update(spectrum=spec, spectrum_table=scells, spectrum_cells=axes, spectrum_settings=settings,
                   spectrum_psd=dict(settings, freqs=np.arange(K, dtype=np.float64) * (self.spectrum_fs / W), psd=psd, cell_names=self._cell_names(),
                                     signals=list(SPECTRUM_SIGNALS), kinds=list(SPECTRUM_KINDS)))

    @staticmethod
    def _actuator_pool(rows, axis=0):
        """stacked actuator rows [reduce columns | maxima | minima] -> the row of their union along `axis` (not the last): sums, the max of the maxima, the min of the minima"""
        rows = np.asarray(rows, np.float64)
        out, a, b = rows.sum(axis), GO2NN_ACTUATOR_OUT_NUM, GO2NN_ACTUATOR_OUT_NUM + len(ACTUATOR_MAX_ROWS)
        out[..., a:b] = rows[..., a:b].max(axis)
        out[..., b:] = rows[..., b:].min(axis)
        return out

    def _actuator_rows(self, rows):
        """rows [L, cols]: L rows of go2nn_actuator_reduce, or pooled ones -> L dicts: ACTUATOR_KEYS over all joints / feet, per joint kind, per joint and per foot, and
        n_envs — actuator_figures of all rows at once (numpy's elementwise IEEE operations: a row's figures do not depend on its neighbours); rows that carry the extremes
        behind the reduce columns (_actuator_pool) also give ACTUATOR_EXTREME_KEYS, NaN without a used robot"""
        rows = np.asarray(rows, np.float64)
        d = actuator_figures(rows[:, :GO2NN_ACTUATOR_OUT_NUM], self.dt, self.joint_names, self.act_foot_names, self.act_torque_limits)
        if rows.shape[1] > GO2NN_ACTUATOR_OUT_NUM:
            x = rows[:, GO2NN_ACTUATOR_OUT_NUM:]
            x = np.where(np.isfinite(x), x, np.nan)          # (-inf / +inf: no robot of the partition has a used frame — then none of its entries is finite)
            tau, vel, fz, margin = x[:, 0:12], x[:, 12:24], x[:, 24:28], x[:, 28:40]
            kind_of = [next(k for k in ACTUATOR_KINDS if k in n) for n in self.joint_names]
            pools = [("", list(range(12)))] + [("/" + k, [j for j in range(12) if kind_of[j] == k]) for k in ACTUATOR_KINDS] + [("/" + n, [j]) for j, n in enumerate(self.joint_names)]
            for name, js in pools:
                d["torque_peak_max" + name], d["joint_speed_peak_max" + name], d["limit_margin_min" + name] = tau[:, js].max(1), vel[:, js].max(1), margin[:, js].min(1)
            for name, fs in [("", list(range(4)))] + [("/" + n, [f]) for f, n in enumerate(self.act_foot_names)]:
                d["grf_peak_max" + name] = fz[:, fs].max(1)
        keys, cols = list(d), [v.tolist() for v in d.values()]
        return [dict(zip(keys, vals), n_envs=int(n)) for vals, n in zip(zip(*cols), rows[:, 0])]

    def _actuator_row(self, r):
        """one row of go2nn_actuator_reduce, or a pooled one -> its figures (_actuator_rows)"""
        return self._actuator_rows(np.asarray(r, np.float64)[None])[0]

    def _actuator_results(self, res, acells, extremes):
        """acells: go2nn_actuator_reduce's table per cell of the active mode;  extremes [1 + 28 + 12, N]: the USED, peak and margin rows of every robot -> res["actuators"]:
        the cells' rows pooled for every partition the mode reports — sums in fp64, the extremes as the exact max / min over the partition's robots that have a used frame.
        res["overall"] is left as it is: with the flag on every other result is that of the flag-off run"""
        n_max = len(ACTUATOR_MAX_ROWS)
        ext = np.concatenate([np.full((self.num_cells, n_max), -np.inf), np.full((self.num_cells, len(ACTUATOR_MIN_ROWS)), np.inf)], 1)
        used = extremes[0] > 0
        for c in range(self.num_cells):
            ids = np.nonzero((self.cell_host == c) & used)[0]
            if len(ids):
                ext[c, :n_max], ext[c, n_max:] = extremes[1:1 + n_max][:, ids].max(1), extremes[1 + n_max:][:, ids].min(1)
        # the pooled row of every leaf first, then the figures of all leaves in one vectorised pass (a leaf has some 200 of them)
        tree, axes = self._addon_tree(np.concatenate([acells, ext], 1), lambda r: np.array(r, np.float64), self._actuator_pool)
        leaves = []

        def walk(node, visit):
            return {k: walk(v, visit) for k, v in node.items()} if isinstance(node, dict) else visit(node)
        walk(tree, leaves.append)
        figures = iter(self._actuator_rows(np.stack(leaves)))
        tree = walk(tree, lambda _: next(figures))
        settings = {"saturation": self.act_saturation, "contact_threshold": self.act_threshold, "joint_names": list(self.joint_names), "foot_names": list(self.act_foot_names),
                    "torque_limits": [float(x) for x in self.act_torque_limits], "joint_speed_limits": [float(x) for x in self.act_vel_limits],
                    "position_limits": [[float(a), float(b)] for a, b in zip(self.act_pos_lo, self.act_pos_hi)],
                    "torque_saturation_thresholds": [float(x) for x in self.act_tau_thr], "joint_speed_saturation_thresholds": [float(x) for x in self.act_vel_thr]}
        res.update(actuators=tree, actuator_table=acells, actuator_extremes=ext, actuator_cells=axes, actuator_settings=settings)

    def _bootstrap_results(self, res, bcells):
        """bcells: go2nn_eval_bootstrap's table [B, cells, 12] -> "ci" in every leaf dict _row() made, and res["bootstrap"].  A partition's replicate rows are the sums of
        its cells' replicate rows: _cell_views, which gives _results its reshapes and sums, one axis further in"""
        B, conf = bcells.shape[0], self.confidence
        T, S, key, names = self.T, self.S, self.axis_key, self.axis_names
        ci = lambda rows: intervals(rows, conf)
        table, view = self._cell_views(bcells)
        overall = table.sum(1)
        res["overall"]["ci"] = ci(overall)
        for ti, t in enumerate(self.terrain_names):
            for si, s in enumerate(self.scenarios):
                res["groups"][t][s[0]]["ci"] = ci(table[:, ti * S + si])
        if key in ("perturbations", "sensors"):
            for pi, n in enumerate(names):
                res[key][n]["ci"] = ci(view[:, :, pi].sum(1))
                for ti, t in enumerate(self.terrain_names):
                    for si, s in enumerate(self.scenarios):
                        res["cells"][t][s[0]][n]["ci"] = ci(view[:, ti * S + si, pi])
        elif key == "ladder":
            for ti, t in enumerate(self.terrain_names):
                for li, lv in enumerate(names):
                    for si, s in enumerate(self.scenarios):
                        res["ladder"][t][lv][s[0]]["ci"] = ci(view[:, ti, li, si])
        elif key == "maneuvers":          # (a "scenario" is a maneuver there)
            t3 = table.reshape(B, T, S, -1)
            for mi, n in enumerate(names):
                res["maneuvers"][n]["ci"] = ci(t3[:, :, mi].sum(1))
        res["bootstrap"] = {"replicates": B, "seed": self.bootstrap_seed, "confidence": conf, "table": bcells, "overall": overall}

    def _addon_replicates(self, bcells, pool=np.sum):
        """bcells [B, cells, cols]: an add-on's bootstrap table -> [(path into the add-on's tree, replicate rows [B, cols])] for every leaf _addon_tree makes: its pooling,
        one axis further in"""
        B, T, S, key, names = bcells.shape[0], self.T, self.S, self.axis_key, self.axis_names
        table, view = self._cell_views(bcells, pool)
        out = [(("overall",), pool(table, 1))]
        out += [(("groups", t, s[0]), table[:, ti * S + si]) for ti, t in enumerate(self.terrain_names) for si, s in enumerate(self.scenarios)]
        if key in ("perturbations", "sensors"):
            out += [(("cells", t, s[0], n), view[:, ti * S + si, pi]) for ti, t in enumerate(self.terrain_names) for si, s in enumerate(self.scenarios) for pi, n in enumerate(names)]
            out += [((key, n), pool(view[:, :, pi], 1)) for pi, n in enumerate(names)]
        elif key == "ladder":
            out += [(("ladder", t, lv, s[0]), view[:, ti, li, si]) for ti, t in enumerate(self.terrain_names) for li, lv in enumerate(names) for si, s in enumerate(self.scenarios)]
        elif key == "maneuvers":
            out += [(("maneuvers", n), pool(table.reshape(B, T, S, -1)[:, :, si], 1)) for si, n in enumerate(names)]
        return out

    def _mode_replicates(self, res, name, bcells):
        """bcells [B, cells, cols]: the bootstrap table of a mode's own family -> [(path into res, replicate rows [B, cols])] for every leaf that reports the family's
        figures: the pooling of _results / _ladder_results, one axis further in"""
        B, T, S, names = bcells.shape[0], self.T, self.S, self.axis_names
        out = [(("overall",), bcells.sum(1))]
        if name == "robust":
            r3 = self._cell_views(bcells)[1]
            out += [(("cells", t, s[0], n), r3[:, ti * S + si, pi]) for ti, t in enumerate(self.terrain_names) for si, s in enumerate(self.scenarios) for pi, n in enumerate(names)]
            out += [(("perturbations", n), r3[:, :, pi].sum(1)) for pi, n in enumerate(names)]
        elif name == "maneuver":
            out += [(("groups", t, n), bcells[:, ti * S + mi]) for ti, t in enumerate(self.terrain_names) for mi, n in enumerate(names)]
            out += [(("maneuvers", n), bcells.reshape(B, T, S, -1)[:, :, mi].sum(1)) for mi, n in enumerate(names)]
        elif name == "ladder":
            l4 = self._cell_views(bcells)[1]
            out += [(("ladder", t, lv, s[0]), l4[:, ti, li, si]) for ti, t in enumerate(self.terrain_names) for li, lv in enumerate(self.levels) for si, s in enumerate(self.scenarios)]
        return out

    def _ladder_summary_replicates(self, cleared):
        """cleared: float64 [B, levels], a terrain's replicate `cleared` curve under the first ladder scenario -> (level_cleared [B], mean_level_cleared [B]) by
        _ladder_results' loop rule: an empty cell (NaN) has cleared nothing; the highest level of the unbroken run of levels at or above the pass share (-1: none); the
        curve's sum from the lowest level up"""
        curve = np.where(np.isnan(cleared), 0.0, cleared)
        run = np.logical_and.accumulate(~(curve < self.ladder_pass_share), axis=1).sum(1)
        top = np.where(run > 0, np.asarray(self.levels, np.float64)[np.maximum(run, 1) - 1], -1.0)
        mean = np.zeros(curve.shape[0])
        for li in range(curve.shape[1]):
            mean = mean + curve[:, li]
        return top, mean

    def _bootstrap_all_results(self, res, bcells, bhost):
        """bhost: {family: its bootstrap table [B, cells, cols]} -> the families' figures in the "ci" of every leaf that reports them (the leaves of res["gait"] and
        res["asymmetry"] gain a "ci"), the ladder summary's intervals, and res["bootstrap"]["tables"] / ["metrics"].  Per family ONE vectorised pass over (replicates x
        leaves): the row function's twin on the stacked replicate rows, one quantile call over every figure of every leaf"""
        conf, bs, dt = self.confidence, res["bootstrap"], self.dt
        metrics = dict(replicate_metrics(bs["overall"]))
        twins = {"robust": lambda r: robust_replicates(r, dt), "maneuver": lambda r: maneuver_replicates(r, dt), "ladder": lambda r: ladder_replicates(r, dt),
                 "gait": lambda r: gait_replicates(r, dt, self.foot_names), "asym": asym_replicates,
                 "actuator": lambda r: actuator_replicates(r, dt, self.joint_names, self.act_foot_names, self.act_torque_limits)}
        for name, table in bhost.items():
            if name in ("gait", "asym", "actuator"):
                root = res[{"gait": "gait", "asym": "asymmetry", "actuator": "actuators"}[name]]
                leaves = self._addon_replicates(table, self._asym_pool if name == "asym" else np.sum)
            else:
                root, leaves = res, self._mode_replicates(res, name, table)
            reps = twins[name](np.stack([rows for _, rows in leaves], 1))          # {key: [B, leaves]}
            keys = list(reps)
            lo, hi = interval_columns(np.concatenate([reps[k] for k in keys], 1), conf)
            L = len(leaves)
            for li, (path, _) in enumerate(leaves):
                node = root
                for step in path:
                    node = node[step]
                if name == "ladder" and path == ("overall",):          # the overall row reports `cleared` alone (and mean_level_cleared, below)
                    node["ci"]["cleared"] = [float(lo[keys.index("cleared") * L + li]), float(hi[keys.index("cleared") * L + li])]
                    continue
                node.setdefault("ci", {}).update({k: [float(lo[ki * L + li]), float(hi[ki * L + li])] for ki, k in enumerate(keys)})
            overall = {k: np.ascontiguousarray(v[:, 0]) for k, v in reps.items()}          # (leaf 0 is "overall")
            if name == "ladder":          # per terrain the summary's two figures from the replicate curves, and the overall mean over the terrains
                overall = {"cleared": overall["cleared"]}
                first, per_t = self.scenarios[0][0], []
                at = {path: li for li, (path, _) in enumerate(leaves)}
                for t in self.terrain_names:
                    curve = np.stack([reps["cleared"][:, at[("ladder", t, lv, first)]] for lv in self.levels], 1)
                    top, mean = self._ladder_summary_replicates(curve)
                    res["ladder_summary"][t]["ci"] = {"level_cleared": interval(top, conf), "mean_level_cleared": interval(mean, conf)}
                    per_t.append(mean)
                per_t = np.stack(per_t, 1)
                overall["mean_level_cleared"] = np.asarray([float(np.mean(per_t[b])) for b in range(per_t.shape[0])])
                res["overall"]["ci"]["mean_level_cleared"] = interval(overall["mean_level_cleared"], conf)
            if name == "gait":          # res["overall"] reports the pooled gait figures
                res["overall"]["ci"].update({k: root["overall"]["ci"][k] for k in GAIT_KEYS})
            metrics.update(overall)
        bs["tables"], bs["metrics"] = dict(bhost), metrics

    def _results(self, cells, rcells=None, lcells=None, mcells=None):
        """cells: the eval reduce table per (terrain, scenario, perturbation) cell; rcells: the robust one (None without perturbations: a cell is a group then);
        lcells: the ladder's (None without the ladder), cells being per (terrain, level, scenario) then;  mcells: the maneuvers' (None without maneuvers), per
        (terrain, maneuver) cell = group"""
        S = self.S
        table, c3 = self._cell_views(cells)          # (c3: the per-cell view [groups, P, cols] of the modes without a ladder)
        groups = {t: {s[0]: self._row(table[ti * S + si]) for si, s in enumerate(self.scenarios)} for ti, t in enumerate(self.terrain_names)}
        res = {"overall": self._row(table.sum(0)), "groups": groups, "terrain_names": list(self.terrain_names), "scenarios": [s[0] for s in self.scenarios],
               "steps": self.steps, "dt": self.dt, "mode": self.last_mode, "table": table}
        if rcells is not None:
            both = lambda e, r: dict(self._row(e), **self._robust_row(r))
            names, r3 = list(self.axis_names), self._cell_views(rcells)[1]
            res["cells"] = {t: {s[0]: {n: both(c3[ti * S + si, pi], r3[ti * S + si, pi]) for pi, n in enumerate(names)} for si, s in enumerate(self.scenarios)}
                            for ti, t in enumerate(self.terrain_names)}
            res["perturbations"] = {n: both(c3[:, pi].sum(0), r3[:, pi].sum(0)) for pi, n in enumerate(names)}
            res["overall"].update(self._robust_row(rcells.sum(0)))
            res.update(perturbation_names=names, cell_table=cells, robust_table=rcells, push_steps=self.push_steps.tolist(),
                       push={"first": self.push_first, "period": self.push_period, "window": self.push_window, "hold": self.push_hold, "count": self.push_count})
        if self.sensors is not None:
            names = list(self.axis_names)
            res["cells"] = {t: {s[0]: {n: self._row(c3[ti * S + si, pi]) for pi, n in enumerate(names)} for si, s in enumerate(self.scenarios)}
                            for ti, t in enumerate(self.terrain_names)}
            res["sensors"] = {n: self._row(c3[:, pi].sum(0)) for pi, n in enumerate(names)}
            res.update(sensor_names=names, cell_table=cells,
                       sensor_specs={n: {k: (int(f.get(k, 0)) if k == "delay" else float(f.get(k, 0.0))) for k in SENSOR_FIELDS} for n, f in self.sensors})
        if lcells is not None:
            self._ladder_results(res, cells, lcells)
        if mcells is not None:
            T, M, names = self.T, self.S, self.axis_names
            for ti, t in enumerate(self.terrain_names):
                for mi, n in enumerate(names):
                    groups[t][n].update(self._maneuver_row(mcells[ti * M + mi]))
            c3, m3 = table.reshape(T, M, -1), mcells.reshape(T, M, -1)
            res["maneuvers"] = {n: dict(self._row(c3[:, mi].sum(0)), **self._maneuver_row(m3[:, mi].sum(0))) for mi, n in enumerate(names)}
            res["overall"].update(self._maneuver_row(mcells.sum(0)))
            res.update(maneuver_table=mcells, switch_steps={n: list(self.switch_steps[n]) for n in names},
                       maneuver_rule={"window": self.maneuver_window, "hold": self.maneuver_hold, "thr_lin": self.maneuver_thr[0], "thr_ang": self.maneuver_thr[1]},
                       maneuver_schedule={n: [[int(s)] + [float(x) for x in seg[1:4]] for s, seg in zip([0] + list(self.switch_steps[n]), segs)] for n, segs in self.maneuvers})
        return res

    def close(self):
        if self.env is not None:
            self.env.close()
            self.env = None


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def scalars(res):
    """[(tag, value)]: with gait 'Eval/gait/<key>' and 'Eval/gait/<terrain>/<scenario>/<key>'; with asymmetry 'Eval/asymmetry/<key>' and 'Eval/asymmetry/<terrain>/<scenario>/<key>'; 'Eval/<metric>' for the overall figures, 'Eval/<terrain>/<scenario>/<metric>' per group, with perturbations 'Eval/robust/<name>/<metric>', with
    maneuvers 'Eval/maneuver/<name>/<metric>', with sensor conditions 'Eval/sensors/<name>/<metric>' and, with the ladder, 'Eval/ladder/<terrain>/{level_cleared,mean_level_cleared}' and 'Eval/ladder/mean_level_cleared'; with the black box 'Eval/falls/robots_fell'; with the bootstrap 'Eval/ci_low/<metric>' and 'Eval/ci_high/<metric>' (overall only; with `bootstrap_all` also the families' overall figures and 'Eval/asymmetry/ci_low|high/<key>')"""
    out = [("Eval/" + k, res["overall"][k]) for k in RESULT_KEYS]
    for t, per in res["groups"].items():
        for s, d in per.items():
            out += [("Eval/%s/%s/%s" % (t, s, k), d[k]) for k in RESULT_KEYS]
    for n, d in (res.get("perturbations") or {}).items():
        out += [("Eval/robust/%s/%s" % (n, k), d[k]) for k in RESULT_KEYS + ROBUST_KEYS]
    for n, d in (res.get("maneuvers") or {}).items():
        out += [("Eval/maneuver/%s/%s" % (n, k), d[k]) for k in RESULT_KEYS + MANEUVER_KEYS]
    for n, d in (res.get("sensors") or {}).items():
        out += [("Eval/sensors/%s/%s" % (n, k), d[k]) for k in RESULT_KEYS]
    if res.get("ladder_summary") is not None:
        for t, d in res["ladder_summary"].items():
            out += [("Eval/ladder/%s/%s" % (t, k), d[k]) for k in LADDER_SUMMARY_KEYS]
        out.append(("Eval/ladder/mean_level_cleared", res["overall"]["mean_level_cleared"]))
    if res.get("gait") is not None:          # overall: pooled and per foot; per group: pooled
        out += [("Eval/gait/" + k, v) for k, v in res["gait"]["overall"].items() if k not in ("n_envs", "ci")]
        for t, per in res["gait"]["groups"].items():
            for s, d in per.items():
                out += [("Eval/gait/%s/%s/%s" % (t, s, k), d[k]) for k in GAIT_KEYS]
    if res.get("asymmetry") is not None:          # 'Eval/asymmetry/<key>' overall and 'Eval/asymmetry/<terrain>/<scenario>/<key>' per group
        out += [("Eval/asymmetry/" + k, res["asymmetry"]["overall"][k]) for k in ASYM_KEYS]
        for t, per in res["asymmetry"]["groups"].items():
            for s, d in per.items():
                out += [("Eval/asymmetry/%s/%s/%s" % (t, s, k), d[k]) for k in ASYM_KEYS]
    if res.get("spectrum") is not None:          # 'Eval/spectrum/<key>' overall (pooled and per joint kind) and 'Eval/spectrum/<terrain>/<scenario>/<key>' per group
        out += [("Eval/spectrum/" + k, v) for k, v in res["spectrum"]["overall"].items() if k not in ("n_envs", "ci")]
        for t, per in res["spectrum"]["groups"].items():
            for s, d in per.items():
                out += [("Eval/spectrum/%s/%s/%s" % (t, s, k), d[k]) for k in SPECTRUM_KEYS]
    if res.get("actuators") is not None:          # 'Eval/actuators/<key>' overall (every pool) and 'Eval/actuators/<terrain>/<scenario>/<key>' per group (over all joints / feet)
        out += [("Eval/actuators/" + k, v) for k, v in res["actuators"]["overall"].items() if k not in ("n_envs", "ci")]
        for t, per in res["actuators"]["groups"].items():
            for s, d in per.items():
                out += [("Eval/actuators/%s/%s/%s" % (t, s, k), d[k]) for k in ACTUATOR_KEYS + ACTUATOR_EXTREME_KEYS]
    if res.get("falls") is not None:          # with the black box: how many robots fell on a counted step
        out.append(("Eval/falls/robots_fell", res["falls"]["fell_total"]))
    if res.get("bootstrap") is not None:          # with the bootstrap: 'Eval/ci_low/<metric>' and 'Eval/ci_high/<metric>', the overall figures only
        for k in CI_KEYS:
            out += [("Eval/ci_low/" + k, res["overall"]["ci"][k][0]), ("Eval/ci_high/" + k, res["overall"]["ci"][k][1])]
        if "tables" in res["bootstrap"]:          # with `bootstrap_all`: the families' overall figures, and the asymmetry section's
            for k, (lo, hi) in res["overall"]["ci"].items():
                if k not in CI_KEYS:
                    out += [("Eval/ci_low/" + k, lo), ("Eval/ci_high/" + k, hi)]
            for k, (lo, hi) in ((res.get("asymmetry") or {}).get("overall", {}).get("ci") or {}).items():
                out += [("Eval/asymmetry/ci_low/" + k, lo), ("Eval/asymmetry/ci_high/" + k, hi)]
            for k, (lo, hi) in ((res.get("actuators") or {}).get("overall", {}).get("ci") or {}).items():
                out += [("Eval/actuators/ci_low/" + k, lo), ("Eval/actuators/ci_high/" + k, hi)]
    return out


def results_dict(res, it=None):
    """what eval_results/results_{it}.yaml holds (plain Python numbers)"""
    d = {"iteration": it, "steps": res["steps"], "dt": res["dt"], "overall": dict(res["overall"]), "groups": {t: {s: dict(v) for s, v in per.items()} for t, per in res["groups"].items()}}
    if res.get("perturbations") is not None:
        d["perturbations"] = {n: dict(v) for n, v in res["perturbations"].items()}
        d["push"] = dict(res["push"])
    if res.get("maneuvers") is not None:          # per maneuver over the terrains, the settling rule and the schedule [counted step, vx, vy, yaw rate] per segment
        d["maneuvers"] = {n: dict(v) for n, v in res["maneuvers"].items()}
        d["maneuver_rule"] = dict(res["maneuver_rule"])
        d["maneuver_schedule"] = {n: [list(seg) for seg in segs] for n, segs in res["maneuver_schedule"].items()}
    if res.get("sensors") is not None:          # per condition over the terrains and scenarios, next to the condition's own spec
        d["sensors"] = {n: dict(v, spec=dict(res["sensor_specs"][n])) for n, v in res["sensors"].items()}
    if res.get("ladder") is not None:          # the full curve, and what it comes to per terrain kind
        d["ladder"] = {t: {int(lv): {s: dict(v) for s, v in per.items()} for lv, per in levels.items()} for t, levels in res["ladder"].items()}
        d["ladder_summary"] = {t: dict(v) for t, v in res["ladder_summary"].items()}
        d["ladder_levels"], d["ladder_distance"], d["ladder_pass_share"] = [int(l) for l in res["levels"]], float(res["ladder_distance"]), float(res["ladder_pass_share"])
    plain = lambda v: {(int(k) if isinstance(k, (int, np.integer)) else k): plain(x) for k, x in v.items()} if isinstance(v, dict) else v
    if res.get("gait") is not None:          # every partition the mode reports, pooled figures per leaf; level keys as plain ints
        d["gait"] = plain(res["gait"])
        d["gait_contact_threshold"], d["foot_names"] = float(res["gait_contact_threshold"]), list(res["foot_names"])
    if res.get("asymmetry") is not None:          # as the gait section: every partition the mode reports
        d["asymmetry"] = plain(res["asymmetry"])
        d["asymmetry_contact_threshold"] = float(res["asymmetry_contact_threshold"])
    if res.get("spectrum") is not None:          # as the gait section; the estimator's settings next to the tree
        d["spectrum"] = dict(plain(res["spectrum"]), **{k: (int(v) if k == "window" else float(v)) for k, v in res["spectrum_settings"].items()})
    if res.get("actuators") is not None:          # as the gait section; the limits and the saturation share next to the tree
        d["actuators"] = dict(plain(res["actuators"]), settings=dict(res["actuator_settings"]))
    if res.get("bootstrap") is not None:          # how the "ci" entries of the leaves above were made
        d["bootstrap"] = {k: res["bootstrap"][k] for k in ("replicates", "seed", "confidence")}
    return d


def format_table(res):
    cols = ("lin_vel_err", "ang_vel_err", "speed_along_cmd", "tilt", "power", "falls", "survival", "n_envs")
    lines = ["%-16s %-14s " % ("terrain", "scenario") + " ".join("%15s" % c for c in cols)]
    rows = [(t, s, d) for t, per in res["groups"].items() for s, d in per.items()] + [("all", "all", res["overall"])]
    for t, s, d in rows:
        lines.append("%-16s %-14s " % (t, s) + " ".join("%15.4f" % d[c] if c != "n_envs" else "%15d" % d[c] for c in cols))
    if res.get("perturbations") is not None:          # the second block: one line per perturbation, over every terrain and scenario
        cols = ("lin_vel_err", "torque_sq", "falls", "survival") + ROBUST_KEYS + ("n_envs",)
        whole = ("pushes", "n_envs")
        lines += ["", "%-20s " % "perturbation" + " ".join("%16s" % c for c in cols)]
        for n, d in list(res["perturbations"].items()) + [("all", res["overall"])]:
            lines.append("%-20s " % n + " ".join("%16d" % d[c] if c in whole else "%16.4f" % d[c] for c in cols))
    if res.get("ladder") is not None:          # the third block: one line per terrain kind, the share of robots that cleared each level under the first ladder scenario
        first = res["scenarios"][0]
        lines += ["", "%-16s %-14s " % ("terrain", "cleared @ level") + " ".join("%6d" % lv for lv in res["levels"]) + " %14s %19s" % LADDER_SUMMARY_KEYS]
        for t, levels in res["ladder"].items():
            sm = res["ladder_summary"][t]
            lines.append("%-16s %-14s " % (t, first) + " ".join("%6.2f" % levels[lv][first]["cleared"] for lv in res["levels"])
                         + " %14d %19.3f" % (sm["level_cleared"], sm["mean_level_cleared"]))
        lines.append("%-16s %-14s " % ("all", first) + " ".join("%6s" % "" for _ in res["levels"]) + " %14s %19.3f" % ("", res["overall"]["mean_level_cleared"]))
    if res.get("maneuvers") is not None:          # the fourth block: one line per maneuver, over every terrain
        cols = ("lin_vel_err", "ang_vel_err", "falls", "survival") + MANEUVER_KEYS + ("n_envs",)
        whole = ("switches", "n_envs")
        lines += ["", "%-20s " % "maneuver" + " ".join("%18s" % c for c in cols)]
        for n, d in list(res["maneuvers"].items()) + [("all", res["overall"])]:
            lines.append("%-20s " % n + " ".join("%18d" % d[c] if c in whole else "%18.4f" % d[c] for c in cols))
    if res.get("sensors") is not None:          # one more block: one line per sensor condition, over every terrain and scenario
        cols = ("lin_vel_err", "ang_vel_err", "tilt", "action_rate_sq", "torque_sq", "falls", "survival", "n_envs")
        lines += ["", "%-20s " % "sensors" + " ".join("%16s" % c for c in cols)]
        for n, d in list(res["sensors"].items()) + [("all", res["overall"])]:
            lines.append("%-20s " % n + " ".join("%16d" % d[c] if c == "n_envs" else "%16.4f" % d[c] for c in cols))
    if res.get("gait") is not None:          # one more block: the pooled gait figures per group
        lines += ["", "%-16s %-14s " % ("terrain", "gait") + " ".join("%20s" % c for c in GAIT_KEYS)]
        rows = [(t, s, d) for t, per in res["gait"]["groups"].items() for s, d in per.items()] + [("all", "all", res["gait"]["overall"])]
        for t, s, d in rows:
            lines.append("%-16s %-14s " % (t, s) + " ".join("%20.4f" % d[c] for c in GAIT_KEYS))
    if res.get("asymmetry") is not None:          # one more block: the policy's equivariance error and the left / right load per group
        cols = ("equivariance_rmse", "equivariance_rel", "equivariance_max", "sym_steps_share") + tuple("left_share/" + x for x in ASYM_LOADS) + tuple("imbalance/" + x for x in ASYM_LOADS)
        lines += ["", "%-16s %-14s " % ("terrain", "asymmetry") + " ".join("%18s" % c for c in cols)]
        rows = [(t, s, d) for t, per in res["asymmetry"]["groups"].items() for s, d in per.items()] + [("all", "all", res["asymmetry"]["overall"])]
        for t, s, d in rows:
            lines.append("%-16s %-14s " % (t, s) + " ".join("%18.3e" % d[c] if c.startswith("equivariance") else "%18.4f" % d[c] for c in cols))
    if res.get("spectrum") is not None:          # one more block: the pooled spectrum figures per group
        cols = SPECTRUM_KEYS + SPECTRUM_COUNT_KEYS
        lines += ["", "%-16s %-14s " % ("terrain", "spectrum") + " ".join("%22s" % c for c in cols)]
        rows = [(t, s, d) for t, per in res["spectrum"]["groups"].items() for s, d in per.items()] + [("all", "all", res["spectrum"]["overall"])]
        for t, s, d in rows:
            lines.append("%-16s %-14s " % (t, s) + " ".join("%22.4g" % d[c] for c in cols))
    if res.get("actuators") is not None:          # one more block: per joint kind the torque, speed and margin figures, then the foot forces and the work per metre
        cols = tuple("%s/%s" % (k, kind) for kind in ACTUATOR_KINDS for k in ("torque_rms", "torque_peak", "torque_saturation", "joint_speed_peak", "limit_margin")) + ("grf_peak", "energy_per_m")
        lines += ["", "%-16s %-14s " % ("terrain", "actuators") + " ".join("%23s" % c for c in cols)]
        rows = [(t, s, d) for t, per in res["actuators"]["groups"].items() for s, d in per.items()] + [("all", "all", res["actuators"]["overall"])]
        for t, s, d in rows:
            lines.append("%-16s %-14s " % (t, s) + " ".join("%23.4f" % d[c] for c in cols))
    if res.get("falls") is not None:          # one more block: per cell with falls, how many robots fell and the medians over the kept ones (NaN: no frame before the fall)
        from .recorder import fall_summary
        falls = res["falls"]
        sm = fall_summary(falls, contact_threshold=float(res.get("gait_contact_threshold", 1.0)))
        cols = ("robots_fell", "kept", "time_s", "tilt_before", "feet_down_before")
        lines += ["", "%-44s " % "falls (first counted fall per robot)" + " ".join("%17s" % c for c in cols)]
        median = lambda v: float(np.nanmedian(v)) if np.isfinite(v).any() else float("nan")
        for c in np.nonzero(falls["fell_per_cell"])[0]:
            k = np.asarray(falls["cell_of_robot"]) == c
            lines.append("%-44s " % falls["cell_names"][c] + "%17d %17d " % (falls["fell_per_cell"][c], int(k.sum()))
                         + " ".join("%17.4f" % median(sm[key][k]) for key in ("time_s", "tilt", "feet_in_contact")))
        lines.append("%-44s " % "all" + "%17d %17d" % (falls["fell_total"], len(falls["env_ids"])))
    if res.get("bootstrap") is not None:          # one more block: the overall row again, every figure with its interval
        bs, cols = res["bootstrap"], ("lin_vel_err", "ang_vel_err", "speed_along_cmd", "tilt", "power", "falls", "survival")
        head = "%g %% interval, %d replicates" % (100.0 * bs["confidence"], bs["replicates"])
        lines += ["", "%-36s " % head + " ".join("%34s" % c for c in cols)]
        lines.append("%-36s " % "all" + " ".join("%34s" % ("%.4f [%.4f, %.4f]" % ((res["overall"][c],) + tuple(res["overall"]["ci"][c]))) for c in cols))
        if "tables" in bs:          # with `bootstrap_all`: the active families' headline figures
            cells = [(c, res["overall"]) for fam, cs in BOOTSTRAP_HEADLINES for c in cs if fam in bs["tables"] and fam not in ("asym", "actuator")]
            cells += [(c, res["asymmetry"]["overall"]) for fam, cs in BOOTSTRAP_HEADLINES for c in cs if fam == "asym" and fam in bs["tables"]]
            cells += [(c, res["actuators"]["overall"]) for fam, cs in BOOTSTRAP_HEADLINES for c in cs if fam == "actuator" and fam in bs["tables"]]
            if cells:
                lines += ["%-36s " % "" + " ".join("%34s" % c for c, _ in cells)]
                lines.append("%-36s " % "all" + " ".join("%34s" % ("%.4g [%.4g, %.4g]" % ((d[c],) + tuple(d["ci"][c]))) for c, d in cells))
    return "\n".join(lines)


def write_results(log_dir, it, res):
    import yaml
    path = os.path.join(log_dir, "eval_results")
    os.makedirs(path, exist_ok=True)
    out = os.path.join(path, "results_%s.yaml" % it)
    with open(out, "w") as f:
        yaml.safe_dump(results_dict(res, it), f)
    if res.get("trace") is not None:
        from .recorder import write_trace
        write_trace(os.path.join(path, "trace_%s.npz" % it), res["trace"])
    if res.get("falls") is not None:
        from .recorder import write_falls
        write_falls(os.path.join(path, "falls_%s.npz" % it), res["falls"])
    if res.get("spectrum_psd") is not None:
        from .recorder import write_spectrum
        write_spectrum(os.path.join(path, "spectrum_%s.npz" % it), res["spectrum_psd"])
    return out
