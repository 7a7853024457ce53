"""CLI / config helpers with the reference's surface (legged_gym/utils/helpers.py): class_to_dict :12-27,
set_seed :38-48, parse_sim_params :50-72, get_load_path :74-97, update_cfg_from_args :99-126, get_args :128-157
(including the flags Isaac Gym's gymutil.parse_arguments adds: --sim_device --pipeline --graphics_device_id
--physx/--flex --num_threads --subscenes --slices)."""
import argparse
import os
import random
from pathlib import Path

import numpy as np
import torch


def _public_attrs(obj):
    return ((k, getattr(obj, k)) for k in dir(obj) if not k.startswith("_"))


def class_to_dict(obj) -> dict:
    """Nested config classes -> plain nested dicts (what the runner dumps to config.yaml).  Leaves (anything without a __dict__) pass
    through; lists are converted element-wise.  Reference surface: legged_gym/utils/helpers.py class_to_dict."""
    if not hasattr(obj, "__dict__"):
        return obj
    conv = lambda v: list(map(class_to_dict, v)) if isinstance(v, list) else class_to_dict(v)
    return {k: conv(v) for k, v in _public_attrs(obj)}


def update_class_from_dict(obj, d):
    """Inverse direction: write the entries of a (nested) dict into the matching (nested) config classes."""
    for key, val in d.items():
        target = getattr(obj, key, None)
        if isinstance(target, type):
            update_class_from_dict(target, val)
            continue
        setattr(obj, key, val)


def set_seed(seed):
    """Seed every generator a run touches (python, numpy, torch CPU + all GPUs); -1 draws one.  -> the seed used."""
    seed = int(np.random.randint(0, 10000)) if seed == -1 else seed
    print(f"Setting seed: {seed}")
    os.environ["PYTHONHASHSEED"] = str(seed)
    for seeder in (random.seed, np.random.seed, torch.manual_seed):
        seeder(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


class SimParams:
    """What the reference passes around as gymapi.SimParams: only dt / substeps / gravity / pipeline flag matter here."""

    def __init__(self, dt=0.005, substeps=1, use_gpu_pipeline=True, gravity=(0.0, 0.0, -9.81)):
        self.dt, self.substeps, self.use_gpu_pipeline, self.gravity = dt, substeps, use_gpu_pipeline, list(gravity)


def parse_sim_params(args, cfg):
    sp = SimParams(use_gpu_pipeline=getattr(args, "use_gpu_pipeline", True))
    sim = cfg.get("sim", {})
    sp.dt = sim.get("dt", sp.dt)
    sp.substeps = sim.get("substeps", sp.substeps)
    sp.gravity = list(sim.get("gravity", sp.gravity))
    return sp


def _checkpoint_number(path):
    stem = path.stem.split("_", 1)[-1]
    return int(stem) if stem.isdigit() else -1


def get_load_path(root, load_run=-1, checkpoint=-1):
    """logs/<experiment>/<run>/model_<it>.pt to resume from: the last run directory (by name) that holds checkpoints unless `load_run`
    names one, and its highest-numbered checkpoint unless `checkpoint` names one (legged_gym/utils/helpers.py get_load_path)."""
    root = Path(root) if root is not None else None
    if load_run == -1:
        runs = sorted(d.name for d in root.iterdir() if d.is_dir() and d.name != "exported" and any(d.glob("model_*.pt"))) if root is not None and root.is_dir() else []
        if not runs:
            raise ValueError("No runs in this directory: %s" % (root,))
        run_dir = root / runs[-1]
    else:
        run_dir = root / load_run
    if checkpoint != -1:
        return str(run_dir / ("model_%s.pt" % checkpoint))
    saved = sorted(run_dir.glob("model*"), key=lambda f: (_checkpoint_number(f), f.name))
    if not saved:
        raise ValueError("No checkpoints in %s" % (run_dir,))
    return str(saved[-1])


# command-line argument -> attribute of train_cfg.runner it overrides when given
_RUNNER_OVERRIDES = ("max_iterations", "experiment_name", "run_name", "load_run", "checkpoint")


def update_cfg_from_args(env_cfg, cfg_train, args):
    """Command-line overrides onto the config objects (legged_gym/utils/helpers.py update_cfg_from_args): --num_envs onto the env config;
    --seed, --resume and the runner fields above onto the train config; the RoboGauge switches when the train config has that section (parsed and ignored: the service is
    out of scope), --symmetry onto algorithm.symmetry, --diagnostics onto algorithm.diagnostics, --normalize_obs onto runner.empirical_normalization, --normalize_value onto algorithm.normalize_value, and next to them --evaluate / --eval_interval / --record / --robust / --ladder / --maneuvers / --sensors / --gait / --spectrum / --actuators / --blackbox / --asymmetry / --ci / --ci_all onto the `evaluation` section."""
    if env_cfg is not None and args.num_envs is not None:
        env_cfg.env.num_envs = args.num_envs
    if cfg_train is None:
        return env_cfg, cfg_train
    if args.seed is not None:
        cfg_train.seed = args.seed
    if args.resume:
        cfg_train.runner.resume = True
    for name in _RUNNER_OVERRIDES:
        given = getattr(args, name)
        if given is not None:
            setattr(cfg_train.runner, name, given)
    gauge = getattr(cfg_train, "robogauge", None)
    if gauge is not None:
        for arg_name, field in (("robogauge", "enabled"), ("robogauge_port", "port")):
            given = getattr(args, arg_name, None)
            if given is not None:
                setattr(gauge, field, given)
    if getattr(args, "symmetry", False):
        cfg_train.algorithm.symmetry = True          # (a CTS task's algorithm then refuses at construction: feed-forward PPO only)
    if getattr(args, "diagnostics", False):
        cfg_train.algorithm.diagnostics = True          # (a recurrent policy or MCP-CTS then refuses at construction)
    if getattr(args, "smooth_loss", None) is not None:
        cfg_train.algorithm.smooth_loss_coef = args.smooth_loss
    if getattr(args, "mirror_loss", None) is not None:          # the mirror loss is a term on the augmented mini-batches: the flag switches augmentation on too
        cfg_train.algorithm.mirror_loss_coef = args.mirror_loss
        cfg_train.algorithm.symmetry = True
    if getattr(args, "normalize_value", False):
        cfg_train.algorithm.normalize_value = True          # (a recurrent policy or more than one rank then refuses at construction)
    if getattr(args, "normalize_obs", False):
        cfg_train.runner.empirical_normalization = True          # (a CTS or recurrent task, or --symmetry next to it, then refuses at construction: feed-forward PPO only)
    ev = getattr(cfg_train, "evaluation", None)
    if ev is not None:
        if getattr(args, "evaluate", False):
            ev.enabled = True
        if getattr(args, "eval_interval", None) is not None:
            ev.interval = args.eval_interval
        if getattr(args, "record", None) is not None:
            ev.record = args.record
        if getattr(args, "robust", False):
            from .evaluator import DEFAULT_PERTURBATIONS
            ev.perturbations = [[n, dict(f)] for n, f in DEFAULT_PERTURBATIONS]
        if getattr(args, "ladder", False):
            ev.ladder = True
        if getattr(args, "maneuvers", False):
            from .evaluator import DEFAULT_MANEUVERS
            ev.maneuvers = [[n, [list(seg) for seg in segs]] for n, segs in DEFAULT_MANEUVERS]
        if getattr(args, "sensors", False):
            from .evaluator import DEFAULT_SENSORS
            ev.sensors = [[n, dict(f)] for n, f in DEFAULT_SENSORS]
        if getattr(args, "gait", False):
            ev.gait = True
        if getattr(args, "spectrum", False):
            ev.spectrum = True
        if getattr(args, "actuators", False):
            ev.actuators = True
        if getattr(args, "blackbox", None) is not None:
            ev.blackbox = args.blackbox
        if getattr(args, "asymmetry", False):
            ev.asymmetry = True
        if getattr(args, "ci", None) is not None:
            ev.bootstrap = args.ci
        if getattr(args, "ci_all", False):
            ev.bootstrap_all = True
    return env_cfg, cfg_train


def get_args(argv=None):
    p = argparse.ArgumentParser(description="RL Policy")
    p.add_argument("--task", type=str, default="go2_flat")
    p.add_argument("--resume", action="store_true", default=False)
    p.add_argument("--experiment_name", type=str)
    p.add_argument("--run_name", type=str)
    p.add_argument("--load_run", type=str)
    p.add_argument("--checkpoint", type=int)
    p.add_argument("--headless", action="store_true", default=False)
    p.add_argument("--horovod", action="store_true", default=False, help="accepted and ignored, as in the reference")
    p.add_argument("--rl_device", type=str, default="cuda:0")
    p.add_argument("--num_envs", type=int)
    p.add_argument("--seed", type=int)
    p.add_argument("--max_iterations", type=int)
    p.add_argument("--robogauge", action="store_true", default=False)
    p.add_argument("--robogauge_port", type=int, default=9973)
    p.add_argument("--evaluate", action="store_true", default=False, help="score the checkpoints with the native policy evaluator (train config section `evaluation`)")
    p.add_argument("--eval_interval", type=int, help="iterations between two evaluations")
    p.add_argument("--record", type=int, help="record per-step trajectories on the device: robots per evaluation group (train.py --evaluate, evaluate.py), first N envs (play.py)")
    p.add_argument("--robust", action="store_true", default=False, help="evaluate under the default perturbations too (pushes, payload, weak motors, soft gains, low friction): "
                   "evaluation.perturbations = utils/evaluator.py DEFAULT_PERTURBATIONS")
    p.add_argument("--ladder", action="store_true", default=False, help="evaluate on every terrain level and report the difficulty the policy gets through "
                   "(terrain tasks): evaluation.ladder = True")
    p.add_argument("--maneuvers", action="store_true", default=False, help="evaluate scripted command changes (start, brake, reverse, turn) instead of commands that hold: "
                   "evaluation.maneuvers = utils/evaluator.py DEFAULT_MANEUVERS")
    p.add_argument("--sensors", action="store_true", default=False, help="evaluate under sensor noise, bias, latency and dropped frames too (what the policy sees, not what the "
                   "robot does): evaluation.sensors = utils/evaluator.py DEFAULT_SENSORS")
    p.add_argument("--gait", action="store_true", default=False, help="score how the robots walk too (duty factor, stride frequency, slip, swing clearance, support pattern; works "
                   "next to every mode above): evaluation.gait = True")
    p.add_argument("--spectrum", action="store_true", default=False, help="score how fast the joints are driven too: Welch spectra of every robot's actions and torques (high-"
                   "frequency share, centroid, CAPS smoothness, power; works next to every mode above): evaluation.spectrum = True")
    p.add_argument("--actuators", action="store_true", default=False, help="score what the policy does to the motors and the legs too: per-joint RMS and peak torque, the "
                   "share of samples at the torque / speed limit, mechanical power, margin to the joint stops, foot forces, energy per metre (works next to every mode "
                   "above): evaluation.actuators = True")
    p.add_argument("--blackbox", type=int, nargs="?", const=2, help="keep the last seconds before every evaluated robot's first fall and write, per reported cell, those of N "
                   "fallen robots (default 2) to eval_results/falls_<it>.npz (works next to every mode above): evaluation.blackbox = N")
    p.add_argument("--asymmetry", action="store_true", default=False, help="score left-right asymmetry too: how far the policy is from mirror-equivariant on the states it "
                   "visits, and how unequally the robot loads its left and right legs under mirror-symmetric commands (works next to every mode above; not for recurrent "
                   "policies): evaluation.asymmetry = True")
    p.add_argument("--ci", type=int, nargs="?", const=1000, help="give every evaluated figure a bootstrap confidence interval from B resamplings of the robots within their "
                   "cells (default 1000; works next to every mode above), and let evaluate.py --all_checkpoints compare every checkpoint with the best one on the same "
                   "resamplings: evaluation.bootstrap = B")
    p.add_argument("--ci_all", action="store_true", default=False, help="with --ci [B] (given alone: --ci 1000) also give the modes' own figures (push_falls, settle_time_s, "
                   "cleared, ...) and the gait and asymmetry sections their intervals, from the same resamplings, and let evaluate.py --metric rank by them: "
                   "evaluation.bootstrap_all = True")
    p.add_argument("--symmetry", action="store_true", default=False, help="train every PPO mini-batch on its left-right mirror image too (feed-forward PPO only): "
                   "algorithm.symmetry = True")
    p.add_argument("--diagnostics", action="store_true", default=False, help="log the update's diagnostics as Diag/*: clip fraction, approximate and analytic KL, explained "
                   "variance, ratio and advantage statistics, gradient norm and clipped share, with their first- and last-epoch values; computed on the device inside the "
                   "update, training is bit for bit unchanged (feed-forward PPO and the CTS family): algorithm.diagnostics = True")
    p.add_argument("--smooth_loss", type=float, default=None, metavar="COEF", help="add COEF x the mean squared gap between the policy's action means at successive steps of an "
                   "episode to the PPO loss; the update's mini-batches become blocks of whole environments (feed-forward PPO only): algorithm.smooth_loss_coef = COEF")
    p.add_argument("--mirror_loss", type=float, default=None, metavar="COEF", help="add COEF x the mean squared gap between the policy's answer to an observation and the "
                   "mirrored answer to its mirror image to the PPO loss (feed-forward PPO only; switches --symmetry on): algorithm.mirror_loss_coef = COEF")
    p.add_argument("--normalize_obs", action="store_true", default=False, help="normalise both observation streams by their running mean and standard deviation "
                   "(feed-forward PPO only; the statistics travel in the checkpoint): runner.empirical_normalization = True")
    p.add_argument("--normalize_value", action="store_true", default=False, help="let the critic predict returns normalised by their running mean and standard deviation "
                   "(feed-forward PPO and the CTS family, one rank; the statistics travel in the checkpoint): algorithm.normalize_value = True")
    p.add_argument("--record_steps", type=int, default=500, help="play.py --record: the last S steps of the rollout are kept")
    # flags contributed by isaacgym.gymutil.parse_arguments in the reference
    p.add_argument("--sim_device", type=str, default="cuda:0")
    p.add_argument("--pipeline", type=str, default="gpu")
    p.add_argument("--graphics_device_id", type=int, default=0)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--flex", action="store_true")
    g.add_argument("--physx", action="store_true")
    p.add_argument("--num_threads", type=int, default=0)
    p.add_argument("--subscenes", type=int, default=0)
    p.add_argument("--slices", type=int, default=0)
    args = p.parse_args(argv)
    if args.ci_all and args.ci is None:          # --ci_all alone: --ci with its default
        args.ci = 1000
    dev = args.sim_device
    args.sim_device_type = dev.split(":")[0]
    args.compute_device_id = int(dev.split(":")[1]) if ":" in dev else 0
    args.use_gpu = args.sim_device_type == "cuda"
    args.use_gpu_pipeline = args.pipeline in ("gpu", "cuda") and args.use_gpu
    args.physics_engine = 1                      # SIM_PHYSX in the reference; this build has one engine
    args.sim_device_id = args.compute_device_id  # name alignment (:153-156)
    args.sim_device = args.sim_device_type + (f":{args.sim_device_id}" if args.sim_device_type == "cuda" else "")
    return args
