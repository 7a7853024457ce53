"""What one policy evaluation costs (utils/evaluator.py), and what the metric kernel saves over torch expressions.

    python tools/eval_bench.py [--task go2_flat] [--reps 3] [--robust] [--ladder] [--maneuvers] [--sensors] [--blackbox] [--asymmetry] [--ci] [--ci_all] [--spectrum] [--actuators] [--out profiles/eval_bench.json]

Measures, on cuda:0, with the task's default `evaluation` section (1024 robots, 1 s + 10 s):
  * wall time of evaluate() run eagerly and with the captured chunk of steps replayed (simulator re-creation, capture and the final host copy included: it is what
    the training loop waits for), best and median of --reps;
  * go2nn_eval_accumulate per launch, from device events around 200 back-to-back launches on the evaluator's own buffers (for the kernel's own duration run this tool
    under `rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --kernel_only` and read eval_per_env_kernel<EvalAccumulate>);
  * the same ten per-step terms written as torch expressions on the same (strided) buffers, per step, eager and replayed from a HIP graph.
--robust: the same with the default perturbations on (evaluation.perturbations = DEFAULT_PERTURBATIONS), plus go2nn_robust_apply + go2nn_robust_accumulate per pair of
back-to-back launches; the torch-expression comparison is left out.
--ladder (a terrain task, e.g. --task go2): the same with evaluation.ladder on, plus go2nn_ladder_accumulate per back-to-back launch; again without the torch expressions.
--maneuvers: the same with the default maneuvers in the scenarios' place (evaluation.maneuvers = DEFAULT_MANEUVERS), plus go2nn_maneuver_apply + go2nn_maneuver_accumulate per
pair of back-to-back launches; again without the torch expressions.
--sensors: a measurement of its own, ADDED to the JSON file under the key "sensors" (the file's other keys stay as they are): evaluate() run eagerly without and with the
default sensor conditions (evaluation.sensors = DEFAULT_SENSORS), alternating, in this one session, best and median of --reps, and go2nn_sensor_apply (the frame kernel
and its one-lane cursor launch) per back-to-back call on the evaluator's own buffers, by the method of the go2nn_eval_accumulate figure.
--blackbox: a measurement of its own, written to profiles/blackbox_bench.json: evaluate() run eagerly with evaluation.blackbox off and on (2 robots kept per cell),
alternating, at least three runs each in this one session — best, median, spread and every run —, and go2nn_blackbox_record (the frame kernel and the state kernel) per
back-to-back call with no robot frozen, by the same method.
--asymmetry: a measurement of its own, ADDED to profiles/asymmetry_bench.json under the task's name: evaluate() run eagerly with evaluation.asymmetry off and on,
alternating, --reps runs each (at least five) in this one session — best, median, spread and every run —, and per back-to-back call on the evaluator's own buffers the
three extra pieces of a step: the mirror launch, the policy's second forward and go2nn_asym_accumulate.
--ci_all: a measurement of its own, written to profiles/bootstrap_all_bench.json: evaluate() with --robust --gait --asymmetry --ci run eagerly without and with
evaluation.bootstrap_all, alternating, the difference split into launches, copies and the host's quantiles, and every family's launch alone at 6, 42 and 294 cells.
--ci: a measurement of its own, written to profiles/bootstrap_bench.json: evaluate() run eagerly with evaluation.bootstrap off and at 1000 replicates, alternating, --reps
runs each (at least five) in this one session — best, median, spread, every run and the difference of the medians —, and go2nn_eval_bootstrap alone per back-to-back call
on the evaluation's own accumulators at the plain cells, at --robust's cells and at seven times as many (--robust on a terrain task), each next to the same resampling
written in numpy on the host with the copy of the accumulators it would need.
--spectrum: a measurement of its own, written to profiles/spectrum_bench.json: evaluate() run eagerly with evaluation.spectrum off and on, alternating, --reps runs each
(at least five) in this one session — best, median, spread, every run and the difference of the medians —, go2nn_spectrum_record per back-to-back call, go2nn_spectrum_welch
per back-to-back launch on the evaluation's own trace, a device-to-device copy of the trace's bytes for scale, and the Welch kernel's registers, LDS and scratch from the
code object's notes.
--actuators: a measurement of its own, written to profiles/actuators_bench.json: evaluate() run eagerly with evaluation.actuators off and on, alternating, --reps runs each
(at least five) in this one session — best, median, spread, every run and the difference of the medians —, go2nn_actuator_accumulate per back-to-back call next to
go2nn_gait_accumulate and go2nn_asym_accumulate timed the same way in the same process on the same simulator's buffers, go2nn_actuator_bootstrap next to go2nn_gait_bootstrap
at 6, 42 and 294 cells (B = 1000), the reduce, the copy of the rows the extremes are read from, and the kernels' registers and scratch from the code object's notes.
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils.evaluator import DEFAULT_MANEUVERS, DEFAULT_PERTURBATIONS, DEFAULT_SENSORS, EVAL_SOURCE, PolicyEvaluator  # noqa: E402
from go2_rl_gym_amd.utils.helpers import class_to_dict  # noqa: E402


def torch_metrics(b, lim, acc):
    """the table of include/go2nn.h as torch expressions on the simulator's buffer views, accumulated into acc [10, N]"""
    c, v = b["commands"], b["base_lin_vel"]
    cn = torch.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2)
    q, qd, tau = b["dof_state"][:, :, 0], b["dof_state"][:, :, 1], b["torques"]
    acc[0] += 1.0
    acc[1] += torch.sqrt((c[:, 0] - v[:, 0]) ** 2 + (c[:, 1] - v[:, 1]) ** 2)
    acc[2] += (c[:, 2] - b["base_ang_vel"][:, 2]).abs()
    acc[3] += torch.where(cn < 1e-6, torch.zeros_like(cn), (v[:, 0] * c[:, 0] + v[:, 1] * c[:, 1]) / cn.clamp_min(1e-6))
    acc[4] += torch.sqrt(b["projected_gravity"][:, 0] ** 2 + b["projected_gravity"][:, 1] ** 2)
    acc[5] += (tau * qd).abs().sum(1)
    acc[6] += (tau * tau).sum(1)
    acc[7] += ((b["actions"] - b[EVAL_SOURCE["last_actions"]]) ** 2).sum(1)
    acc[8] += ((q < lim[:, 0]) | (q > lim[:, 1])).any(1).float()
    acc[9] += (b["reset_buf"].bool() & ~b["time_out_buf"].bool()).float()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, (time.perf_counter() - t0) * 1e6 / n          # device us, wall us per call


def sensors_main(a):
    """--sensors: the cost of the sensor model, next to the plain evaluation in the same session -> the "sensors" entry of the JSON file"""
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda sensors: PolicyEvaluator(env_cfg, dict(ev_cfg, sensors=sensors), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"plain": make(None), "sensors": make([[n, dict(f)] for n, f in DEFAULT_SENSORS])}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    for ev in evs.values():
        ev.evaluate(ac, use_graph=False)
    ev = evs["sensors"]
    sin = ev._sensor_in()
    fn = lambda: ev._sensor_apply(sin)
    timed(fn, 20)
    dev_us, wall_us = timed(fn, 200)
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": ev.num_envs, "steps": ev.warmup_steps + ev.steps, "conditions": [c[0] for c in ev.sensors],
             "sensor_apply": {"device_us_per_call_back_to_back": dev_us, "host_us_per_call": wall_us, "launches_per_call": 2}}
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(a.reps):
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w)} for k, w in walls.items()}
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out["sensors"] = entry
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"sensors": entry}))
    for e in evs.values():
        e.close()


def blackbox_main(a):
    """--blackbox: what the black box costs one evaluation, next to the plain evaluation of the same commit in the same session -> profiles/blackbox_bench.json"""
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda n: PolicyEvaluator(env_cfg, dict(ev_cfg, blackbox=n), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"off": make(0), "on": make(2)}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["on"]["table"].tobytes() == res["off"]["table"].tobytes() and "falls" not in res["off"]
    ev = evs["on"]
    rec = ev.fall_recorder
    rec.begin(0)          # nobody frozen: every back-to-back call writes every robot's frame
    timed(rec.record, 20)
    dev_us, wall_us = timed(rec.record, 200)
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": ev.num_envs, "steps": ev.warmup_steps + ev.steps, "ring_steps": rec.T,
             "ring_bytes": rec.frames.numel() * 4, "robots_fell": res["on"]["falls"]["fell_total"], "robots_kept": len(res["on"]["falls"]["env_ids"]),
             "blackbox_record": {"device_us_per_call_back_to_back": dev_us, "host_us_per_call": wall_us, "launches_per_call": 2, "frame_bytes_per_call": ev.num_envs * 448}}
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 3)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(entry, f, indent=1)
    print(json.dumps(entry))
    for e in evs.values():
        e.close()


def asymmetry_main(a):
    """--asymmetry: what the asymmetry scores cost one evaluation, next to the plain evaluation of the same commit in the same session -> profiles/asymmetry_bench.json"""
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda on: PolicyEvaluator(env_cfg, dict(ev_cfg, asymmetry=on), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"off": make(False), "on": make(True)}
    torch.manual_seed(0)
    pol = class_to_dict(train_cfg.policy)
    if "history_length" in class_to_dict(train_cfg):          # the CTS family
        from go2_rl_gym_amd.rsl_rl.modules.actor_critic_cts import ActorCriticCTS
        ac = ActorCriticCTS(45, 263, 12, evs["on"].num_envs, int(train_cfg.history_length), **pol).to("cuda:0")
    else:
        from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
        ac = ActorCritic(45, 263, 12, **{k: v for k, v in pol.items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["on"]["table"].tobytes() == res["off"]["table"].tobytes() and "asymmetry" not in res["off"]
    ev = evs["on"]
    pol_, st, N = ev._policy, ev._stream(), ev.num_envs
    from go2_rl_gym_amd._nn import mirror_rows
    with torch.inference_mode():
        jobs, hist_m = ev._asym_jobs(pol_, ev.env.obs_buf)
        ain = ev._asym_in()
        act = pol_.act(ev.env.obs_buf)
        pieces = {"mirror_rows": lambda: mirror_rows(ev.nn, jobs, 1, N, st), "act_mirrored": lambda: pol_.act_mirrored(ev.asym_obs[1], hist_m),
                  "asym_accumulate": lambda: ev.nn.go2nn_asym_accumulate(C.byref(ain), C.c_void_p(act.data_ptr()), C.c_void_p(act.data_ptr()), C.c_void_p(ev.atable.data_ptr()), N, st)}
        cost = {}
        for name, fn in pieces.items():
            timed(fn, 20)
            dev_us, wall_us = timed(fn, 200)
            cost[name] = {"device_us_per_call_back_to_back": dev_us, "host_us_per_call": wall_us}
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": N, "steps": ev.warmup_steps + ev.steps, "policy": type(ac).__name__,
             "overall": {k: v for k, v in res["on"]["asymmetry"]["overall"].items()}, "per_step": cost}
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 5)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out[a.task] = entry
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({a.task: entry}))
    for e in evs.values():
        e.close()


def numpy_bootstrap(acc, start, envs, B, seed):
    """go2nn_eval_bootstrap's resampling on the host: the same Philox words and index rule (include/go2nn.h) on uint64 arrays, the gathered terms summed by numpy (pairwise:
    the same replicates to the last bits, not the same bits) -> [B, G, 12]"""
    import numpy as np
    from go2_rl_gym_amd._nn import EVAL_METRICS
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    N, G = acc.shape[1], len(start) - 1
    terms = np.concatenate([acc.astype(np.float64), np.ones((1, N)), (acc[EVAL_METRICS.index("falls")] == 0).astype(np.float64)[None]]).T.copy()          # [N, 12]
    out = np.zeros((B, G, terms.shape[1]))
    for g in range(G):
        s0, n = int(start[g]), int(start[g + 1] - start[g])
        if n == 0:
            continue
        blocks = (n + 3) // 4
        c0, c2 = np.broadcast_arrays(np.arange(B, dtype=np.uint64)[:, None], np.arange(blocks, dtype=np.uint64)[None, :])
        c1, c3, k0, k1 = np.full_like(c0, g), np.zeros_like(c0), np.uint64(seed), np.uint64(7)
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
            c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        x = np.stack([c0, c1, c2, c3], 2).reshape(B, blocks * 4)[:, :n]
        j = ((x * np.uint64(n)) >> s32).astype(np.int64)
        out[:, g] = terms[envs[s0 + j]].sum(1)
    return out


def bootstrap_main(a):
    """--ci: what the bootstrap costs one evaluation, next to the option-off evaluation of the same commit in the same session, and the launch alone next to the same
    resampling in numpy on the host -> profiles/bootstrap_bench.json"""
    import numpy as np
    B = 1000
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda **over: PolicyEvaluator(env_cfg, dict(ev_cfg, **over), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"off": make(bootstrap=0), "on": make(bootstrap=B)}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["on"]["table"].tobytes() == res["off"]["table"].tobytes() and "bootstrap" not in res["off"]
    ev = evs["on"]
    N, st, p = ev.num_envs, ev._stream(), lambda t: C.c_void_p(t.data_ptr())
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": N, "steps": ev.warmup_steps + ev.steps, "replicates": B, "confidence": ev.confidence,
             "overall": {k: [res["on"]["overall"][k]] + res["on"]["overall"]["ci"][k] for k in res["on"]["overall"]["ci"]}, "launch": {}}
    # the launch alone, on the evaluation's own accumulators: the plain cells, --robust's cells of this task, and as many cells as --robust has on the terrain task (7 kinds)
    robust = make(perturbations=[[n, dict(f)] for n, f in DEFAULT_PERTURBATIONS])
    layouts = {"plain": ev.cell_host, "robust": robust.cell_host, "robust_7_terrain_kinds": (np.arange(N) % (7 * robust.num_cells)).astype(np.int32)}
    robust.close()
    acc_host = ev.acc.cpu().numpy()
    for name, cell in layouts.items():
        G = int(cell.max()) + 1
        start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=G))]).astype(np.int32)
        envs = np.argsort(cell, kind="stable").astype(np.int32)
        assert ev.nn.go2nn_eval_bootstrap_check(C.c_void_p(start.ctypes.data), C.c_void_p(envs.ctypes.data), N, G) == 0
        s_d, e_d = torch.from_numpy(start).to("cuda:0"), torch.from_numpy(envs).to("cuda:0")
        out = torch.zeros(B, G, 12, dtype=torch.float64, device="cuda:0")
        fn = lambda: ev.nn.go2nn_eval_bootstrap(p(ev.acc), p(s_d), p(e_d), N, G, B, ev.bootstrap_seed, p(out), st)
        assert fn() == 0
        timed(fn, 20)
        dev_us, wall_us = timed(fn, 200)
        host = []
        for _ in range(3):          # the same resampling on the host, with the copies it would need: the accumulators down, nothing up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = numpy_bootstrap(ev.acc.cpu().numpy(), start, envs, B, ev.bootstrap_seed)
            host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        got = out.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        scale = np.abs(ref).max((0, 1))
        entry["launch"][name] = {"cells": G, "robots_per_cell": [int(np.diff(start).min()), int(np.diff(start).max())], "device_us_per_call_back_to_back": dev_us,
                                 "host_us_per_call": wall_us, "table_bytes": got.nbytes, "table_copy_ms": copy_ms, "numpy_on_host_ms": {"best": min(host), "all": host},
                                 "largest_gap_to_numpy_over_column_max": float((np.abs(got - ref).max((0, 1)) / np.maximum(scale, 1e-300)).max())}
        assert np.array_equal(got[:, :, 10], ref[:, :, 10]) and np.array_equal(acc_host, ev.acc.cpu().numpy())
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 5)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        entry["evaluate_wall_ms_eager"]["on_minus_off_median"] = statistics.median(walls["on"]) - statistics.median(walls["off"])
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(entry, f, indent=1)
    print(json.dumps(entry))
    for e in evs.values():
        e.close()


def bootstrap_all_main(a):
    """--ci_all: what `evaluation.bootstrap_all` costs one evaluation with --robust --gait --asymmetry --ci, next to the same evaluation without it in the same session
    (alternating runs), the difference split into launches, copies and the host's replicate figures and quantiles, and every bootstrap launch alone (the five families' and go2nn_eval_bootstrap) at 6, 42 and 294 cells
    next to the same resampling in vectorised numpy -> profiles/bootstrap_all_bench.json"""
    import numpy as np
    from go2_rl_gym_amd import build
    B = 1000
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = dict(class_to_dict(train_cfg.evaluation), perturbations=[[n, dict(f)] for n, f in DEFAULT_PERTURBATIONS], gait=True, asymmetry=True, bootstrap=B)
    make = lambda **over: PolicyEvaluator(env_cfg, dict(ev_cfg, **over), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"ci": make(), "ci_all": make(bootstrap_all=True)}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["ci"]["bootstrap"]["table"].tobytes() == res["ci_all"]["bootstrap"]["table"].tobytes() and "tables" not in res["ci"]["bootstrap"]
    ev = evs["ci_all"]
    N, st, p = ev.num_envs, ev._stream(), lambda t: C.c_void_p(t.data_ptr())
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": N, "steps": ev.warmup_steps + ev.steps, "cells": ev.num_cells, "replicates": B,
             "families": {t.name: int(t.out.shape[1]) for t in ev.tables}, "table_bytes": {n: int(t.numel() * 8) for n, t in ev.boot_outs.items()}}
    match = {"eval": 12, "robust": 7, "maneuver": 9, "ladder": 6, "gait": 55, "asym": 25}
    entry["registers"] = {f: {k: r[k] for k in ("kernel", "vgpr_count", "sgpr_count", "scratch_bytes_per_lane", "lds_bytes_per_workgroup")}
                          for f, r in ((f, build.kernel_resources(build.NN_OUT, match="eval_bootstrap_kernelILi%dELi" % c)) for f, c in match.items()) if r}
    # the split: the families' launches on the evaluation's own tables (device events), the copies of their tables, the host's pass over them
    launch = lambda t, s_d, e_d, G, out: getattr(ev.nn, "go2nn_%s_bootstrap" % t.name)(p(t.table), p(s_d), p(e_d), N, G, B, ev.bootstrap_seed, *t.reduce_args, p(out), st)
    split = {"launch_us": {}, "copy_ms": {}}
    for t in ev.tables:
        fn = lambda: launch(t, ev.cell_start, ev.cell_envs, ev.num_cells, ev.boot_outs[t.name])
        assert fn() == 0
        timed(fn, 20)
        split["launch_us"][t.name] = timed(fn, 200)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.boot_outs[t.name].cpu().numpy().copy()
        split["copy_ms"][t.name] = (time.perf_counter() - t0) * 1e3
    host = []
    for _ in range(3):
        r = ev.evaluate(ac, use_graph=False)
        tables = r["bootstrap"].pop("tables")
        r["bootstrap"].pop("metrics")
        t0 = time.perf_counter()
        ev._bootstrap_all_results(r, r["bootstrap"]["table"], tables)
        host.append((time.perf_counter() - t0) * 1e3)
    split["host_replicates_and_quantiles_ms"] = {"best": min(host), "all": host}
    split["launches_ms_total"], split["copies_ms_total"] = sum(split["launch_us"].values()) / 1e3, sum(split["copy_ms"].values())
    entry["split_of_one_evaluation"] = split
    # every family's launch alone at 6, 42 and 294 cells of these robots, next to the same resampling in vectorised numpy (random indices, a gather and a sum per cell)
    entry["launch"] = {}
    maneuver = make(perturbations=None, maneuvers=[[n, [list(seg) for seg in segs]] for n, segs in DEFAULT_MANEUVERS], gait=False, asymmetry=False, bootstrap_all=True)
    maneuver.evaluate(ac, use_graph=False)
    # the two launches this evaluation does not make: go2nn_eval_bootstrap on its own accumulators, and the ladder's (a terrain-task mode) on a table of these robots with
    # random states and distances — the launch's work does not depend on the values
    from go2_rl_gym_amd._nn import GO2NN_EVAL_NUM, GO2NN_LADDER_NUM, GO2NN_LADDER_OUT_NUM, LADDER_ROWS, LADDER_STATES
    ltable = torch.rand(GO2NN_LADDER_NUM, N, device="cuda:0")
    ltable[LADDER_ROWS.index("state")] = torch.randint(0, len(LADDER_STATES), (N,), device="cuda:0").float()
    alone = types.SimpleNamespace
    extra = [alone(name="eval", table=ev.acc, out=torch.zeros(1, GO2NN_EVAL_NUM + 2), reduce_args=()),
             alone(name="ladder", table=ltable, out=torch.zeros(1, GO2NN_LADDER_OUT_NUM), reduce_args=(0.25,))]
    for e, t in [(ev, t) for t in ev.tables] + [(maneuver, t) for t in maneuver.tables] + [(ev, t) for t in extra]:
        terms = np.ascontiguousarray(np.resize(t.table.cpu().numpy().astype(np.float64), (int(t.out.shape[1]), N)).T)          # [N, cols]: the yardstick's gather width
        for G in (6, 42, 294):
            cell = (np.arange(N) % G).astype(np.int32)
            start, envs = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=G))]).astype(np.int32), np.argsort(cell, kind="stable").astype(np.int32)
            s_d, e_d = torch.from_numpy(start).to("cuda:0"), torch.from_numpy(envs).to("cuda:0")
            out = torch.zeros(B, G, int(t.out.shape[1]), dtype=torch.float64, device="cuda:0")
            fn = lambda: launch(t, s_d, e_d, G, out)
            assert fn() == 0
            timed(fn, 20)
            dev_us, wall_us = timed(fn, 200)
            host = []
            for _ in range(3):
                rng, t0 = np.random.default_rng(1), time.perf_counter()
                ref = np.zeros((B, G, terms.shape[1]))
                for g in range(G):
                    mem = envs[start[g]:start[g + 1]]
                    ref[:, g] = terms[mem[rng.integers(0, len(mem), (B, len(mem)))]].sum(1)
                host.append((time.perf_counter() - t0) * 1e3)
            entry["launch"]["%s/%d" % (t.name, G)] = {"device_us_per_call_back_to_back": dev_us, "host_us_per_call": wall_us, "numpy_on_host_ms": min(host)}
    maneuver.close()
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 5)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        entry["evaluate_wall_ms_eager"]["ci_all_minus_ci_median"] = statistics.median(walls["ci_all"]) - statistics.median(walls["ci"])
        if os.path.exists(a.out):          # sections of the file this tool does not measure (merged by hand; their "about" says from what) stay
            with open(a.out) as f:
                entry.update({k: v for k, v in json.load(f).items() if k in ("chunk_widths", "bench_py_env_steps_per_s")})
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(entry, f, indent=1)
    print(json.dumps(entry))
    for e in evs.values():
        e.close()


def spectrum_main(a):
    """--spectrum: what `evaluation.spectrum` costs one evaluation, next to the same evaluation without it in the same session (alternating runs), and its launches alone
    -> profiles/spectrum_bench.json"""
    from go2_rl_gym_amd import build
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda on: PolicyEvaluator(env_cfg, dict(ev_cfg, spectrum=on), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"off": make(False), "on": make(True)}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["off"]["table"].tobytes() == res["on"]["table"].tobytes() and "spectrum" not in res["off"]
    ev = evs["on"]
    N, T, W, st = ev.num_envs, ev.steps, ev.spectrum_window, ev._stream()
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": N, "steps": ev.warmup_steps + T, "counted_steps": T, "window": W, "fs": ev.spectrum_fs,
             "trace_bytes": int(ev.strace.numel() * 4), "table_bytes": int(ev.stable.numel() * 4), "cells": ev.num_cells,
             "overall": {k: v for k, v in res["on"]["spectrum"]["overall"].items() if "/" not in k}}
    entry["registers"] = {name: {k: r[k] for k in ("kernel", "vgpr_count", "sgpr_count", "scratch_bytes_per_lane", "lds_bytes_per_workgroup")}
                          for name, r in (("welch", build.kernel_resources(build.NN_OUT, match="spectrum_welch_kernel")),
                                          ("record", build.kernel_resources(build.NN_OUT, match="SpectrumRecord"))) if r}
    entry["welch_dynamic_lds_bytes"] = 8 * (2 * W + 24 * W + 24)
    # the per-step launch: 200 back-to-back calls on the evaluation's own buffers (the trace's counter is past T: the launch's early return is NOT what is timed — begin first)
    sin = ev._spectrum_in()
    begin = lambda: ev.nn.go2nn_spectrum_begin(C.c_void_p(ev.strace.data_ptr()), N, 0, T, st)
    rec = lambda: ev.nn.go2nn_spectrum_record(C.byref(sin), C.c_void_p(ev.strace.data_ptr()), N, T, st)
    keep = ev.strace.clone()
    assert begin() == 0 and rec() == 0
    timed(rec, 20)
    assert begin() == 0
    dev_us, wall_us = timed(rec, 200)          # steps 0 .. 199 < T: every call writes its 25 rows
    entry["record"] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    begin_us = timed(begin, 20)[0]
    entry["begin"] = {"device_us_per_launch_back_to_back": begin_us}
    ev.strace.copy_(keep)
    # the Welch launch on the evaluation's own trace, and a device-to-device copy of the trace's bytes for scale
    timed(ev._spectrum_welch, 3)
    dev_us, wall_us = timed(ev._spectrum_welch, 20)
    entry["welch"] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    other = torch.empty_like(ev.strace)
    copy = lambda: other.copy_(ev.strace)
    timed(copy, 3)
    entry["trace_copy_device_to_device"] = {"device_us_per_copy": timed(copy, 20)[0]}
    group = C.c_void_p(ev.group.data_ptr())
    red = lambda: ev.nn.go2nn_spectrum_reduce(C.c_void_p(ev.stable.data_ptr()), group, N, ev.num_cells, W, C.c_void_p(ev.sout.data_ptr()), st)
    timed(red, 3)
    entry["reduce"] = {"device_us_per_launch_back_to_back": timed(red, 20)[0]}
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 5)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        entry["evaluate_wall_ms_eager"]["on_minus_off_median"] = statistics.median(walls["on"]) - statistics.median(walls["off"])
        if os.path.exists(a.out):          # sections of the file this tool does not measure (merged by hand; their "about" says from what) stay
            with open(a.out) as f:
                entry.update({k: v for k, v in json.load(f).items() if k in ("bench_py_env_steps_per_s",)})
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(entry, f, indent=1)
    print(json.dumps(entry))
    for e in evs.values():
        e.close()


def actuator_launches(ev):
    """ev: an evaluator with actuators, gait and asymmetry on, after an evaluation -> device and host us per back-to-back go2nn_<family>_accumulate call on its own buffers:
    begin at step 0, 20 calls to warm up, begin again, 200 timed calls — every one a counted step"""
    N, st, out = ev.num_envs, ev._stream(), {}
    actions = torch.zeros(N, 12, device=ev.device)
    for t in ev.tables:
        if t.name not in ("actuator", "gait", "asym"):
            continue
        tin, extra = t.make_in(), ((C.c_void_p(actions.data_ptr()), C.c_void_p(actions.data_ptr())) if t.name == "asym" else ())
        begin = lambda: getattr(ev.nn, "go2nn_%s_begin" % t.name)(C.c_void_p(t.table.data_ptr()), N, 0, st)
        acc = lambda: getattr(ev.nn, "go2nn_%s_accumulate" % t.name)(C.byref(tin), *extra, C.c_void_p(t.table.data_ptr()), N, st)
        keep = t.table.clone()
        assert begin() == 0 and acc() == 0, ev.nn.go2nn_last_error()
        timed(acc, 20)
        assert begin() == 0
        dev_us, wall_us = timed(acc, 200)
        t.table.copy_(keep)
        out[t.name] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    return out


def actuator_bootstraps(ev, B=1000):
    """-> device us per back-to-back go2nn_actuator_bootstrap and go2nn_gait_bootstrap launch on the evaluator's own tables at 6, 42 and 294 cells of its robots"""
    import numpy as np
    N, st, out, p = ev.num_envs, ev._stream(), {}, lambda t: C.c_void_p(t.data_ptr())
    for t in ev.tables:
        if t.name not in ("actuator", "gait"):
            continue
        for G in (6, 42, 294):
            cell = (np.arange(N) % G).astype(np.int32)
            start, envs = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=G))]).astype(np.int32), np.argsort(cell, kind="stable").astype(np.int32)
            s_d, e_d = torch.from_numpy(start).to(ev.device), torch.from_numpy(envs).to(ev.device)
            res = torch.zeros(B, G, int(t.out.shape[1]), dtype=torch.float64, device=ev.device)
            fn = lambda: getattr(ev.nn, "go2nn_%s_bootstrap" % t.name)(p(t.table), p(s_d), p(e_d), N, G, B, 2718, p(res), st)
            assert fn() == 0, ev.nn.go2nn_last_error()
            timed(fn, 20)
            out["%s/%d" % (t.name, G)] = {"device_us_per_launch_back_to_back": timed(fn, 200)[0]}
    return out


def actuators_main(a):
    """--actuators: what `evaluation.actuators` costs one evaluation, next to the same evaluation without it in the same session (alternating runs), and its launches alone
    next to the gait and asymmetry scorers' -> profiles/actuators_bench.json"""
    from go2_rl_gym_amd import build
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    make = lambda **over: PolicyEvaluator(env_cfg, dict(ev_cfg, **over), task_class=task_registry.get_task_class(a.task), device="cuda:0")
    evs = {"off": make(actuators=False), "on": make(actuators=True)}
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    res = {k: ev.evaluate(ac, use_graph=False) for k, ev in evs.items()}
    assert res["off"]["table"].tobytes() == res["on"]["table"].tobytes() and "actuators" not in res["off"]
    ev = evs["on"]
    N, st = ev.num_envs, ev._stream()
    entry = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": N, "steps": ev.warmup_steps + ev.steps, "counted_steps": ev.steps, "cells": ev.num_cells,
             "table_bytes": int(ev.act_table.numel() * 4), "overall": {k: v for k, v in res["on"]["actuators"]["overall"].items() if "/" not in k}}
    entry["registers"] = {name: {k: r[k] for k in ("kernel", "vgpr_count", "sgpr_count", "scratch_bytes_per_lane", "lds_bytes_per_workgroup")}
                          for name, r in (("accumulate", build.kernel_resources(build.NN_OUT, match="ActuatorAccumulate")),
                                          ("reduce", build.kernel_resources(build.NN_OUT, match="eval_reduce_kernelILin1E12ActuatorTerm")),
                                          ("bootstrap", build.kernel_resources(build.NN_OUT, match="eval_bootstrap_kernelILi112E"))) if r}
    # the per-step launch next to gait's and the asymmetry's: one evaluator with all three on, so that the three are timed in one process on one simulator's buffers
    three = make(actuators=True, gait=True, asymmetry=True)
    three.evaluate(ac, use_graph=False)
    entry["accumulate"] = actuator_launches(three)
    entry["bootstrap_B1000"] = actuator_bootstraps(three)
    three.close()
    group = C.c_void_p(ev.group.data_ptr())
    red = lambda: ev.nn.go2nn_actuator_reduce(C.c_void_p(ev.act_table.data_ptr()), group, N, ev.num_cells, C.c_void_p(ev.act_out.data_ptr()), st)
    timed(red, 3)
    entry["reduce"] = {"device_us_per_launch_back_to_back": timed(red, 20)[0]}
    rows = lambda: ev.act_table.index_select(0, ev.act_extreme_rows).cpu()
    timed(rows, 3)
    entry["extremes_copy"] = {"rows": int(ev.act_extreme_rows.numel()), "host_us_per_copy": timed(rows, 20)[1]}
    if not a.kernel_only:
        walls = {k: [] for k in evs}
        for _ in range(max(a.reps, 5)):          # alternating, in this one session
            for k, e in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.evaluate(ac, use_graph=False)
                walls[k].append((time.perf_counter() - t0) * 1e3)
        entry["evaluate_wall_ms_eager"] = {k: {"best": min(w), "median": statistics.median(w), "spread": max(w) - min(w), "all": w} for k, w in walls.items()}
        entry["evaluate_wall_ms_eager"]["on_minus_off_median"] = statistics.median(walls["on"]) - statistics.median(walls["off"])
        if os.path.exists(a.out):          # sections of the file this tool does not measure (merged by hand; their "about" says from what) stay
            with open(a.out) as f:
                entry.update({k: v for k, v in json.load(f).items() if k in ("variants", "bench_py_env_steps_per_s")})
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(entry, f, indent=1)
    print(json.dumps(entry))
    for e in evs.values():
        e.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--task", default="go2_flat")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--kernel_only", action="store_true")
    p.add_argument("--robust", action="store_true")
    p.add_argument("--ladder", action="store_true")
    p.add_argument("--maneuvers", action="store_true")
    p.add_argument("--sensors", action="store_true")
    p.add_argument("--blackbox", action="store_true")
    p.add_argument("--asymmetry", action="store_true")
    p.add_argument("--ci", action="store_true")
    p.add_argument("--ci_all", action="store_true")
    p.add_argument("--spectrum", action="store_true")
    p.add_argument("--actuators", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "actuators_bench.json" if a.actuators else "spectrum_bench.json" if a.spectrum else "bootstrap_all_bench.json" if a.ci_all else "bootstrap_bench.json" if a.ci else "asymmetry_bench.json" if a.asymmetry else "blackbox_bench.json" if a.blackbox else "eval_bench.json")
    if a.actuators:
        return actuators_main(a)
    if a.spectrum:
        return spectrum_main(a)
    if a.ci_all:
        return bootstrap_all_main(a)
    if a.ci:
        return bootstrap_main(a)
    if a.asymmetry:
        return asymmetry_main(a)
    if a.blackbox:
        return blackbox_main(a)
    if a.sensors:
        return sensors_main(a)
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    if a.robust:
        ev_cfg["perturbations"] = [[n, dict(f)] for n, f in DEFAULT_PERTURBATIONS]
    if a.ladder:
        ev_cfg["ladder"] = True
    if a.maneuvers:
        ev_cfg["maneuvers"] = [[n, [list(seg) for seg in segs]] for n, segs in DEFAULT_MANEUVERS]
    ev = PolicyEvaluator(env_cfg, ev_cfg, task_class=task_registry.get_task_class(a.task), device="cuda:0")
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    out = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": ev.num_envs, "steps": ev.warmup_steps + ev.steps, "chunk": ev.chunk,
           "perturbations": [n for n, _ in ev.perturbations] if ev.perturbations else None, "ladder_levels": list(ev.levels) if ev.ladder else None,
           "maneuvers": [m[0] for m in ev.maneuvers] if ev.maneuvers else None}
    ev.evaluate(ac, use_graph=False)
    ein, st = ev._eval_in(), ev._stream()
    acc_fn = lambda: ev.nn.go2nn_eval_accumulate(C.byref(ein), C.c_void_p(ev.acc.data_ptr()), ev.num_envs, st)
    timed(acc_fn, 20)
    dev_us, wall_us = timed(acc_fn, 200)
    out["accumulate_kernel"] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    if a.robust:
        robust, rin = next(t for t in ev.tables if t.name == "robust"), ev._robust_in()

        def pair():
            ev._table_launch("apply", robust, rin)
            ev._table_launch("accumulate", robust, rin)
        timed(pair, 20)
        dev_us, wall_us = timed(pair, 200)
        out["robust_apply_plus_accumulate"] = {"device_us_per_pair_back_to_back": dev_us, "host_us_per_pair": wall_us}
    if a.ladder:
        lin = ev._ladder_in()
        lad_fn = lambda: ev.nn.go2nn_ladder_accumulate(C.byref(lin), C.c_void_p(ev.ltable.data_ptr()), ev.num_envs, st)
        timed(lad_fn, 20)
        dev_us, wall_us = timed(lad_fn, 200)
        out["ladder_accumulate_kernel"] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    if a.maneuvers:
        maneuver, min_ = next(t for t in ev.tables if t.name == "maneuver"), ev._maneuver_in()

        def man_pair():
            ev._table_launch("apply", maneuver, min_)
            ev._table_launch("accumulate", maneuver, min_)
        timed(man_pair, 20)
        dev_us, wall_us = timed(man_pair, 200)
        out["maneuver_apply_plus_accumulate"] = {"device_us_per_pair_back_to_back": dev_us, "host_us_per_pair": wall_us}
    if not a.kernel_only:
        walls = {"eager": [], "replayed": []}
        for _ in range(a.reps):
            for mode, g in (("eager", False), ("replayed", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ev.evaluate(ac, use_graph=g)
                walls[mode].append((time.perf_counter() - t0) * 1e3)
                assert res["mode"] == ("graph" if g else "eager")
        out["evaluate_wall_ms"] = {m: {"best": min(w), "median": statistics.median(w)} for m, w in walls.items()}
    if not a.kernel_only and not a.robust and not a.ladder and not a.maneuvers:
        b, lim, acc = ev.env._buf, ev.dof_limits, torch.zeros_like(ev.acc)
        tm = lambda: torch_metrics(b, lim, acc)
        timed(tm, 5)
        d_e, w_e = timed(tm, 50)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tm()
        timed(g.replay, 5)
        d_g, w_g = timed(g.replay, 50)
        out["torch_expressions_per_step"] = {"eager_device_us": d_e, "eager_host_us": w_e, "replayed_device_us": d_g, "replayed_host_us": w_g}
    if not a.kernel_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    ev.close()


if __name__ == "__main__":
    main()
