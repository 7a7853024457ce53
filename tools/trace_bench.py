"""What the trajectory recorder costs (utils/recorder.py): one go2nn_trace_record call next to one go2nn_eval_accumulate call, and whole evaluations with and without it.

    python tools/trace_bench.py [--task go2_flat] [--reps 5] [--baseline_tree DIR] [--out profiles/trace_bench.json]

Measures, on cuda:0, with the task's default `evaluation` section (1024 robots, 1 s + 10 s):
  * go2nn_trace_record per call (its frame launch + its one-lane cursor launch) for the tracked robots of record = 1 and record = 4, and go2nn_eval_accumulate per launch,
    each from device events around 300 back-to-back calls on the evaluator's own buffers;
  * wall time of an eager evaluate() with evaluation.record = 0, 1 and 4 (simulator re-creation and the final host copies included), best and median of --reps, the
    three settings interleaved;
  * with --baseline_tree DIR (a built checkout of another revision, e.g. the parent commit): the accumulate launch and the record = 0 evaluation of THAT tree, measured by
    this script in a fresh process in the same session (--tree DIR --baseline_leg).
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

p = argparse.ArgumentParser()
p.add_argument("--task", default="go2_flat")
p.add_argument("--reps", type=int, default=5)
p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
p.add_argument("--baseline_tree", default=None)
p.add_argument("--baseline_leg", action="store_true", help="only what every revision with an evaluator has: the accumulate launch and the plain evaluation; prints, writes nothing")
p.add_argument("--out", default=None)
ARGS = p.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from go2_rl_gym_amd.envs import task_registry  # noqa: E402
from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator  # noqa: E402
from go2_rl_gym_amd.utils.helpers import class_to_dict  # noqa: E402


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


def per_call(fn):
    timed(fn, 30)
    runs = [timed(fn, 300) for _ in range(3)]
    return {"device_us_per_call_back_to_back": min(r[0] for r in runs), "host_us_per_call": min(r[1] for r in runs)}


def main():
    a = ARGS
    env_cfg, train_cfg = task_registry.get_cfgs(a.task)
    section = class_to_dict(train_cfg.evaluation)
    make = lambda record: PolicyEvaluator(env_cfg, dict(section, record=record), task_class=task_registry.get_task_class(a.task), device="cuda:0")          # noqa: E731
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    settings = (0,) if a.baseline_leg else (0, 1, 4)
    evs = {r: make(r) for r in settings}
    out = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": evs[0].num_envs, "steps": evs[0].warmup_steps + evs[0].steps, "reps": a.reps}
    tables = {r: ev.evaluate(ac, use_graph=False)["table"].tobytes() for r, ev in evs.items()}          # warm-up; every later evaluate() recreates its simulator
    assert len(set(tables.values())) == 1, "the scores depend on evaluation.record"
    ev = evs[0]
    ein, st = ev._eval_in(), ev._stream()
    out["accumulate_launch"] = per_call(lambda: ev.nn.go2nn_eval_accumulate(C.byref(ein), C.c_void_p(ev.acc.data_ptr()), ev.num_envs, st))
    for r in settings[1:]:
        rec = evs[r].recorder
        out["record_call_%d_per_group" % r] = dict(per_call(rec.record), tracked_robots=rec.K, bytes_written_per_call=rec.K * 112 * 4)
    walls = {r: [] for r in settings}
    for _ in range(a.reps):
        for r in settings:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evs[r].evaluate(ac, use_graph=False)
            walls[r].append((time.perf_counter() - t0) * 1e3)
            assert res["table"].tobytes() == tables[0]
    out["evaluate_wall_ms"] = {"record_%d" % r: {"best": min(w), "median": statistics.median(w), "worst": max(w)} for r, w in walls.items()}
    for e in evs.values():
        e.close()
    if a.baseline_tree:
        tree = os.path.abspath(a.baseline_tree)
        leg = subprocess.run([sys.executable, os.path.abspath(__file__), "--task", a.task, "--reps", str(a.reps), "--tree", tree, "--baseline_leg"], capture_output=True, text=True, cwd=tree)
        if leg.returncode != 0:
            raise RuntimeError("the baseline leg failed:\n" + leg.stderr[-2000:])
        out["baseline_tree"] = json.loads([l for l in leg.stdout.splitlines() if l.startswith("{")][-1])
    if not a.baseline_leg:
        path = a.out or os.path.join(os.path.abspath(a.tree), "profiles", "trace_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
