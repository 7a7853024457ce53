"""python -m go2_rl_gym_amd.scripts.evaluate --task go2_flat [--load_run RUN --checkpoint N] [--all_checkpoints --metric lin_vel_err]

Loads a checkpoint of the task's experiment through the runner (like scripts/play.py), scores it with the native policy evaluator (utils/evaluator.py; the train
config's `evaluation` section sets robots, horizon and scenarios), prints the per-terrain, per-command table and one JSON line.  --all_checkpoints walks every
model_*.pt of the run and names the best one by --metric (lower is better for the error / effort metrics, higher for survival and speed_along_cmd).
--robust also scores the default perturbations (pushes, payload, weak motors, soft gains, low friction: utils/evaluator.py DEFAULT_PERTURBATIONS); --metric then also
takes push_falls, recovered, recovery_time_s, peak_lin_vel_err and peak_tilt.
--ladder (terrain tasks) places the robots on every terrain level and adds the per-terrain table of the share that cleared each level; --metric then also takes
mean_level_cleared and cleared (higher is better), so --all_checkpoints --ladder --metric mean_level_cleared names the checkpoint that gets furthest.  The whole curve goes to eval_results/ladder_<checkpoint number>.yaml
in the run's directory.
--maneuvers scores scripted command changes (start, brake, reverse, turn: utils/evaluator.py DEFAULT_MANEUVERS) in the scenarios' place; --metric then also takes
switch_falls, settle_time_s, window_lin_vel_err, window_ang_vel_err (lower is better) and settled (higher is better).
--sensors scores the default sensor conditions (noise, gyro bias, joint offset, one and two steps of latency, dropped frames: utils/evaluator.py DEFAULT_SENSORS) next to
the scenarios; the overall figures are then means over the conditions' robots, so --all_checkpoints --sensors --metric lin_vel_err names the checkpoint that tracks best
across all of them.
--gait also scores how the robots walk (utils/evaluator.py GAIT_KEYS), next to any of the modes above; --metric then also takes the pooled gait figures: slip_speed and
touchdowns_per_s count as lower is better, trot_share and swing_clearance as higher is better (a per-foot figure, slip_speed/FL, ranks as its pooled one), so --all_checkpoints --gait --metric slip_speed names the checkpoint whose
feet drag least.
--asymmetry also scores left-right asymmetry (utils/evaluator.py ASYM_KEYS), next to any of the modes above; --metric then also takes equivariance_rmse (and /hip, /thigh,
/calf), equivariance_rel, equivariance_max and imbalance/action, /torque, /power, /contact — all lower is better —, so --all_checkpoints --asymmetry --metric
equivariance_rmse compares a --symmetry run with a plain one.  left_share/* says WHICH side carries more and has no better direction: it is refused as a metric.
--spectrum also scores how fast the joints are driven (utils/evaluator.py SPECTRUM_KEYS: Welch spectra of every robot's actions and torques), next to any of the modes
above; --metric then also takes action_hf_share, action_centroid_hz, action_smoothness, action_power and their torque_ twins (and a per-kind figure, action_hf_share/calf) —
all lower is better —, so --all_checkpoints --spectrum --metric action_hf_share compares a --smooth_loss run with a plain one.  The figures have no bootstrap replicates:
--ci next to --spectrum leaves every interval as it is, and --ci --metric <a spectrum figure> is refused before anything runs.  The mean power spectra per cell go to
eval_results/spectrum_<checkpoint number>.npz (utils/recorder.py read_spectrum).
--actuators also scores what the policy does to the motors and the legs (utils/evaluator.py ACTUATOR_KEYS), next to any of the modes above; --metric then also takes
torque_rms, torque_rms_share, torque_peak, torque_saturation, joint_speed_peak, joint_speed_saturation, positive_power, negative_power, grf_peak, grf_stance_mean and
energy_per_m — all lower is better — and limit_margin (higher is better), each also per joint kind and per joint (torque_saturation/calf, torque_rms/FL_thigh; a foot figure
per foot, grf_peak/RR), ranked in its pooled figure's direction, so --all_checkpoints --actuators --metric torque_saturation names the checkpoint that leans least on the
torque limit.  The extremes torque_peak_max, joint_speed_peak_max, grf_peak_max (lower is better) and limit_margin_min (higher) rank without --ci and are refused with it: a
bootstrap of an extreme is not one.  A key given without --actuators is refused before anything runs.
--record N also records N robots of every (terrain x scenario) group and writes eval_results/trace_<checkpoint number>.npz into the run's directory.
--blackbox [N] also keeps the last seconds before every robot's first fall (utils/recorder.py FallRecorder), prints per cell with falls how many robots fell and when,
and writes those of N fallen robots per cell (default 2) to eval_results/falls_<checkpoint number>.npz; read_falls and fall_summary read it back.
--ci [B] also gives every figure a bootstrap confidence interval (utils/evaluator.py CI_KEYS; B resamplings of the robots within their cells, default 1000), next to any of
the modes above; --metric must then be one of CI_KEYS.  After the best checkpoint is named as without it, every checkpoint is compared with the best one ON THE SAME
RESAMPLINGS — an evaluation is deterministic per robot index, so the difference of the two metrics per resampling is a paired comparison —: the JSON line gains
"comparison" (per checkpoint its value and interval, the difference to the best and that difference's interval) and "tied_with_best", the checkpoints whose paired interval
contains 0; the same goes to eval_results/comparison_<metric>.yaml in the run's directory (a "/" in the metric's name written as "_").
--ci_all (with --ci [B]; alone it means --ci 1000) also resamples the modes' own figures and the gait and asymmetry sections, on the same draws; --metric may then be any
figure that has replicates (res["bootstrap"]["metrics"]: push_falls, settle_time_s, mean_level_cleared, slip_speed, equivariance_rmse, imbalance/torque, ...), so
--all_checkpoints --asymmetry --ci --ci_all --metric equivariance_rmse says whether two checkpoints' equivariance errors can be told apart.  Refused before anything runs:
left_share/* (no better direction), equivariance_max (a bootstrap of a maximum is not one), the integer counts pushes, switches and n_envs, and a figure whose flag is
not on (push_falls without --robust)."""
import json
import math
import os
import sys
from pathlib import Path

from go2_rl_gym_amd.envs import *  # noqa: F401,F403
from go2_rl_gym_amd.utils import get_args
from go2_rl_gym_amd.utils.evaluator import (ACTUATOR_EXTREME_KEYS, ACTUATOR_FOOT_KEYS, ACTUATOR_KEYS, ACTUATOR_KINDS, ASYM_KEYS, CI_KEYS, DIAGONAL_PAIRS, GAIT_FOOT_KEYS, GAIT_KEYS, MANEUVER_KEYS, ROBUST_KEYS, SPECTRUM_COUNT_KEYS, SPECTRUM_KEYS, PolicyEvaluator,
                                            compare, format_table, interval, replicate_metrics, results_dict)
from go2_rl_gym_amd._nn import SPECTRUM_KINDS
from go2_rl_gym_amd.utils.helpers import _checkpoint_number, get_load_path
from go2_rl_gym_amd.utils.task_registry import ROOT_DIR, task_registry

HIGHER_IS_BETTER = ("survival", "speed_along_cmd", "recovered", "mean_level_cleared", "cleared", "settled", "trot_share", "swing_clearance", "limit_margin", "limit_margin_min")
LEGS = ("FL", "FR", "RL", "RR")
ACTUATOR_JOINTS = tuple("%s_%s" % (leg, kind) for leg in LEGS for kind in ACTUATOR_KINDS)          # what the actuator scorer names its per-joint keys after ("<key>/<joint>")
FEET = tuple(leg for pair in DIAGONAL_PAIRS for leg in pair)          # the feet the gait scorer names its per-foot keys after ("<key>/<foot>")


def higher_is_better(metric):
    """a per-foot gait figure ("swing_clearance/FL") has the direction of its pooled figure"""
    return metric in HIGHER_IS_BETTER or ((is_foot_metric(metric) or is_actuator_metric(metric)) and metric.split("/", 1)[0] in HIGHER_IS_BETTER)


def is_foot_metric(metric):
    return "/" in metric and metric.split("/", 1)[0] in GAIT_FOOT_KEYS and metric.split("/", 1)[1] in FEET


def is_spectrum_metric(metric):
    """a pooled spectrum figure, or one of a joint kind ("torque_centroid_hz/calf")"""
    return metric in SPECTRUM_KEYS or ("/" in metric and metric.split("/", 1)[0] in SPECTRUM_KEYS and metric.split("/", 1)[1] in SPECTRUM_KINDS)


def is_actuator_metric(metric):
    """an actuator figure or extreme: over all joints / feet, of a joint kind or a joint ("torque_rms/FL_hip"), of a foot ("grf_peak/RR"); energy_per_m has no pools.
    The joints and feet are the Go2's (LEGS x ACTUATOR_KINDS), known here before a simulator exists so that a key can be refused before anything runs; the evaluator names
    its keys after env.dof_names and env.body_names, and for a robot named otherwise the pooled and per-kind keys rank and a per-joint key is refused here"""
    key, _, pool = metric.partition("/")
    if key not in ACTUATOR_KEYS + ACTUATOR_EXTREME_KEYS:
        return False
    if not pool:
        return "/" not in metric
    if key == "energy_per_m":
        return False
    return pool in LEGS if key in ACTUATOR_FOOT_KEYS + ("grf_peak_max",) else pool in ACTUATOR_KINDS + ACTUATOR_JOINTS


def _own_flags(argv):
    """--all_checkpoints / --metric / --eval_envs belong to this script; the rest is the common CLI"""
    own = {"all_checkpoints": False, "metric": "lin_vel_err", "eval_envs": None}
    rest, k = [], 0
    while k < len(argv):
        a = argv[k]
        if a == "--all_checkpoints":
            own["all_checkpoints"] = True
        elif a in ("--metric", "--eval_envs"):
            own[a[2:]] = argv[k + 1] if a == "--metric" else int(argv[k + 1])
            k += 1
        else:
            rest.append(a)
        k += 1
    return own, rest


def check_metric(metric):
    if metric.startswith("left_share/"):
        raise ValueError("--metric %s: a left share says which side carries more (0.5 is balanced) and has no better direction; rank by imbalance/%s instead"
                         % (metric, metric.split("/", 1)[1]))
    if metric in SPECTRUM_COUNT_KEYS:
        raise ValueError("--metric %s: how many windows the spectra were taken over (and the share skipped for a reset) says how much was analysed, not how the policy moves; "
                         "rank by one of %s" % (metric, ", ".join(SPECTRUM_KEYS)))


def check_flag_metric(metric, args):
    """a figure whose flag is not on is refused before anything runs"""
    if is_actuator_metric(metric) and not getattr(args, "actuators", False):
        raise ValueError("--metric %s: the figure is scored under --actuators, which is not on" % metric)


def check_ci_metric(metric, args):
    """--ci [--ci_all] --metric: refused before anything runs unless the metric will have replicates — with a message that says why"""
    if metric in CI_KEYS:
        return
    if is_actuator_metric(metric) and metric.split("/", 1)[0] in ACTUATOR_EXTREME_KEYS:
        raise ValueError("--ci --metric %s: an extreme over the robots has no bootstrap interval — a bootstrap of an extreme is not one (a resampling can only lose the "
                         "largest value); rank by it without --ci, or by %s" % (metric, metric.replace("_max", "").replace("_min", "")))
    if is_spectrum_metric(metric):
        raise ValueError("--ci --metric %s: the spectrum figures have no replicates (a robot's table is made by one Welch pass after the run and is not resampled, with or "
                         "without --ci_all); rank by it without --ci" % metric)
    if not getattr(args, "ci_all", False):
        raise ValueError("--ci --metric %s: the bootstrap resamples the figures %s; the modes' own figures, the gait and the asymmetry sections have no replicates "
                         "without --ci_all" % (metric, ", ".join(CI_KEYS)))
    if metric in ("pushes", "switches", "n_envs"):
        raise ValueError("--ci_all --metric %s: an integer count of the design, the same in every resampling of a cell's robots up to which robots were drawn; it gets no "
                         "interval and ranks nothing" % metric)
    if is_actuator_metric(metric):          # (every one that is left has replicates under --ci_all)
        if not getattr(args, "actuators", False):
            raise ValueError("--ci_all --metric %s: the figure is scored under --actuators, which is not on" % metric)
        return
    if metric == "equivariance_max":
        raise ValueError("--ci_all --metric equivariance_max: a maximum over the robots has no bootstrap interval (a resampling can only lose the largest value); rank by "
                         "equivariance_rmse")
    flags = [f for f, keys in (("robust", ROBUST_KEYS), ("maneuvers", MANEUVER_KEYS), ("ladder", ("cleared", "mean_level_cleared")), ("gait", GAIT_KEYS), ("asymmetry", ASYM_KEYS))
             if metric in keys or (f == "gait" and is_foot_metric(metric))]
    if not flags:
        raise ValueError("--ci_all --metric %s: not a figure the evaluator resamples (utils/evaluator.py CI_KEYS, ROBUST_KEYS, MANEUVER_KEYS, cleared, mean_level_cleared, "
                         "GAIT_KEYS and <GAIT_FOOT_KEYS>/<%s>, ASYM_KEYS)" % (metric, "|".join(FEET)))
    if not any(getattr(args, f, False) for f in flags):
        raise ValueError("--ci_all --metric %s: the figure is scored under %s, which is not on" % (metric, " or ".join("--" + f for f in flags)))


def metric_value(row, metric):
    """a checkpoint row's overall `metric`: the scores' own; with --gait a per-foot gait figure (the pooled ones are in `overall`, the per-foot ones in the gait section's);
    with --asymmetry one of the asymmetry figures (kept in their own section: they leave `overall` alone)"""
    for section in ("gait", "asymmetry", "spectrum", "actuators"):
        if metric not in row["overall"] and metric in row.get(section, {}).get("overall", {}):
            return row[section]["overall"][metric]
    return row["overall"][metric]


def best_checkpoint(rows, metric):
    """the row with the best overall `metric`.  A figure that does not exist (NaN: settle_time_s without a settled switch, recovery_time_s without a recovered push) ranks
    last, whatever the order of the rows"""
    check_metric(metric)
    higher = higher_is_better(metric)
    worst = float("-inf") if higher else float("inf")
    value = lambda r: metric_value(r, metric)
    rank = lambda r: worst if isinstance(value(r), float) and math.isnan(value(r)) else value(r)
    return (max if higher else min)(rows, key=rank)


def comparison(rows, reps, best, metric, confidence):
    """rows: the checkpoint rows;  reps: {checkpoint: the [B] replicates of its overall `metric`};  best: the best row -> the "comparison" block: every checkpoint against
    the best one on the same replicates (utils/evaluator.py compare), and the names of those that cannot be told from it"""
    out, tied = [], []
    for r in rows:
        name, value = r["checkpoint"], metric_value(r, metric)
        c = compare(reps[name], reps[best["checkpoint"]], confidence)
        out.append({"checkpoint": name, "value": value, "ci": interval(reps[name], confidence), "diff_to_best": value - metric_value(best, metric), "diff_ci": c["diff_ci"],
                    "tied_with_best": c["tied"]})
        if c["tied"]:
            tied.append(name)
    return {"metric": metric, "confidence": confidence, "replicates": int(len(reps[best["checkpoint"]])), "rows": out}, tied


def format_comparison(comp):
    lines = ["%-20s %12s %26s %14s %26s %6s" % ("checkpoint", comp["metric"][:12], "%g %% interval" % (100.0 * comp["confidence"]), "diff to best", "paired interval", "tied")]
    for r in comp["rows"]:
        lines.append("%-20s %12.4f %26s %14.4f %26s %6s" % (r["checkpoint"], r["value"], "[%.4f, %.4f]" % tuple(r["ci"]), r["diff_to_best"], "[%.4f, %.4f]" % tuple(r["diff_ci"]),
                                                            "yes" if r["tied_with_best"] else "no"))
    return "\n".join(lines)


def evaluate(argv=None, log_root="default", env_kwargs=None, evaluator_kwargs=None):
    """env_kwargs / evaluator_kwargs: extra arguments of the env / of PolicyEvaluator (tests hand in host libraries, as through runner.evaluator_kwargs)"""
    own, rest = _own_flags(list(sys.argv[1:] if argv is None else argv))
    check_metric(own["metric"])
    args = get_args(rest)
    check_flag_metric(own["metric"], args)
    if args.ci is not None:          # refused before anything runs: the comparison needs the metric's replicates
        check_ci_metric(own["metric"], args)
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.env.num_envs = min(env_cfg.env.num_envs, 64)          # the runner's own env only carries the model's shapes here; the evaluator brings its own simulator
    env_cfg.env.test = True
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg, **(env_kwargs or {}))
    train_cfg.runner.resume = True
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=log_root)
    root = os.path.join(ROOT_DIR, "logs", train_cfg.runner.experiment_name) if log_root == "default" else log_root
    first = get_load_path(root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
    paths = sorted(Path(first).parent.glob("model_*.pt"), key=_checkpoint_number) if own["all_checkpoints"] else [Path(first)]
    ev_cfg = dict(runner.eval_cfg)
    if own["eval_envs"] is not None:
        ev_cfg["num_envs"] = own["eval_envs"]
    kw = dict(runner.evaluator_kwargs, **(evaluator_kwargs or {}))
    if env.lib.go2sim_is_device_library() != 1:
        kw.setdefault("lib", env.lib)
    ev = PolicyEvaluator(env.cfg, ev_cfg, task_class=type(env), sim_params=env.sim_params, device=env.sim_device, **kw)
    rows, reps = [], {}
    for p in paths:
        runner.load(str(p), load_optimizer=False)
        res = ev.evaluate(runner.alg.actor_critic)
        print("== %s (%s)\n%s" % (p.name, res["mode"], format_table(res)))
        rows.append({"checkpoint": p.name, "overall": res["overall"], "groups": res["groups"]})
        if res.get("bootstrap") is not None and own["metric"] in CI_KEYS:          # the [B] replicates of the overall metric: what the paired comparison below reads
            reps[p.name] = replicate_metrics(res["bootstrap"]["overall"])[own["metric"]]
        elif res.get("bootstrap") is not None and "metrics" in res["bootstrap"]:          # (--ci_all: a family's figure; check_ci_metric let only those through)
            reps[p.name] = res["bootstrap"]["metrics"][own["metric"]]
        if res.get("perturbations") is not None:
            rows[-1]["perturbations"] = res["perturbations"]
        if res.get("maneuvers") is not None:
            rows[-1]["maneuvers"] = res["maneuvers"]
        if res.get("sensors") is not None:
            rows[-1]["sensors"] = res["sensors"]
        if res.get("gait") is not None:
            rows[-1]["gait"] = {"overall": res["gait"]["overall"], "groups": res["gait"]["groups"]}
        if res.get("asymmetry") is not None:
            rows[-1]["asymmetry"] = {"overall": res["asymmetry"]["overall"], "groups": res["asymmetry"]["groups"]}
        if res.get("actuators") is not None:
            rows[-1]["actuators"] = {"overall": res["actuators"]["overall"], "groups": res["actuators"]["groups"]}
        if res.get("spectrum") is not None:
            from go2_rl_gym_amd.utils.recorder import write_spectrum
            rows[-1]["spectrum"] = {"overall": res["spectrum"]["overall"], "groups": res["spectrum"]["groups"]}
            print("spectrum: %s" % write_spectrum(os.path.join(str(p.parent), "eval_results", "spectrum_%s.npz" % _checkpoint_number(p)), res["spectrum_psd"]))
        if res.get("ladder_summary") is not None:
            rows[-1]["ladder_summary"] = res["ladder_summary"]
            import yaml
            path = os.path.join(str(p.parent), "eval_results", "ladder_%s.yaml" % _checkpoint_number(p))
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                yaml.safe_dump(results_dict(res, _checkpoint_number(p)), f)
            print("ladder: %s" % path)
        if res.get("trace") is not None:
            from go2_rl_gym_amd.utils.recorder import write_trace
            print("trace: %s" % write_trace(os.path.join(str(p.parent), "eval_results", "trace_%s.npz" % _checkpoint_number(p)), res["trace"]))
        if res.get("falls") is not None:
            from go2_rl_gym_amd.utils.recorder import write_falls
            rows[-1]["robots_fell"] = res["falls"]["fell_total"]
            print("falls: %s" % write_falls(os.path.join(str(p.parent), "eval_results", "falls_%s.npz" % _checkpoint_number(p)), res["falls"]))
    metric = own["metric"]
    key = lambda r: metric_value(r, metric)
    best = best_checkpoint(rows, metric)
    out = {"task": args.task, "metric": metric, "best": best["checkpoint"], "best_value": key(best), "checkpoints": rows}
    if reps:          # every checkpoint against the best one, on the same replicates
        import yaml
        out["comparison"], out["tied_with_best"] = comparison(rows, reps, best, metric, ev.confidence)
        print(format_comparison(out["comparison"]))
        path = os.path.join(str(paths[0].parent), "eval_results", "comparison_%s.yaml" % metric.replace("/", "_"))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            yaml.safe_dump({"best": best["checkpoint"], "comparison": out["comparison"], "tied_with_best": out["tied_with_best"]}, f)
        print("comparison: %s" % path)
    print(json.dumps(out))
    ev.close()
    env.close()
    return out


if __name__ == "__main__":
    evaluate()
