"""What the gait scores cost one policy evaluation (utils/evaluator.py, `evaluation.gait`; csrc/go2nn_gait.h).

    python tools/gait_bench.py [--task go2_flat] [--reps 5] [--parent DIR] [--out profiles/gait_bench.json]

Measures, on cuda:0, with the task's default `evaluation` section (1024 robots, 1 s + 10 s = 550 steps), eagerly:
  * wall time of evaluate() without and with gait, alternating in this one process, best and median of --reps (simulator re-creation and the final host copies included:
    it is what the training loop waits for);
  * go2nn_gait_accumulate per launch, from device events around 200 back-to-back launches on the evaluator's own buffers, next to go2nn_eval_accumulate by the same method;
  * with --parent DIR (a built checkout of the parent commit): the plain evaluation of THAT tree and of this one, each in a child process of its own started from here, in
    turn — the same session, the same method, so the flag-off cost of this change is a difference of two like figures.
Writes one JSON file and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, (time.perf_counter() - t0) * 1e6 / n          # device us, wall us per call


def setup(tree, task, variants):
    """the package of `tree`, one evaluator per variant {name: overrides of the evaluation section}, a fresh actor-critic -> (evaluators, model); each evaluated once"""
    sys.path.insert(0, tree)
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    ev_cfg = class_to_dict(train_cfg.evaluation)
    evs = {k: PolicyEvaluator(env_cfg, dict(ev_cfg, **over), task_class=task_registry.get_task_class(task), device="cuda:0") for k, over in variants.items()}
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, **{k: v for k, v in class_to_dict(train_cfg.policy).items() if k in ("actor_hidden_dims", "critic_hidden_dims", "activation", "init_noise_std")}).to("cuda:0")
    for ev in evs.values():
        ev.evaluate(ac, use_graph=False)
    return evs, ac


def walls(evs, ac, reps):
    import torch
    w = {k: [] for k in evs}
    for _ in range(reps):
        for k, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate(ac, use_graph=False)
            w[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"best": min(v), "median": statistics.median(v), "all": v} for k, v in w.items()}


def worker(a):
    """a child process: the plain evaluation of the tree at --tree -> one JSON line"""
    evs, ac = setup(a.tree, a.task, {"plain": {}})
    print(json.dumps(walls(evs, ac, a.reps)["plain"]))
    evs["plain"].close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--task", default="go2_flat")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    p.add_argument("--worker", action="store_true")
    p.add_argument("--tree", default=ROOT)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "gait_bench.json"))
    a = p.parse_args()
    if a.worker:
        return worker(a)
    import torch
    evs, ac = setup(ROOT, a.task, {"plain": {}, "gait": {"gait": True}})
    ev = evs["gait"]
    out = {"task": a.task, "device": torch.cuda.get_device_name(0), "num_envs": ev.num_envs, "steps": ev.warmup_steps + ev.steps, "reps": a.reps}
    out["evaluate_wall_ms_eager"] = walls(evs, ac, a.reps)
    gin, ein, st = ev._gait_in(), ev._eval_in(), ev._stream()
    for name, fn in (("gait_accumulate_kernel", lambda: ev.nn.go2nn_gait_accumulate(C.byref(gin), C.c_void_p(ev.gtable.data_ptr()), ev.num_envs, st)),
                     ("eval_accumulate_kernel", lambda: ev.nn.go2nn_eval_accumulate(C.byref(ein), C.c_void_p(ev.acc.data_ptr()), ev.num_envs, st))):
        timed(fn, 20)
        dev_us, wall_us = timed(fn, 200)
        out[name] = {"device_us_per_launch_back_to_back": dev_us, "host_us_per_call": wall_us}
    for e in evs.values():
        e.close()
    if a.parent:          # one process holds the GPU at a time; parent and this tree in turn, twice
        trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
        runs = {k: [] for k in trees}
        for _ in range(2):
            for k, tree in trees.items():
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--task", a.task, "--reps", str(a.reps)], capture_output=True, text=True,
                                   cwd=tree, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("the %s tree's evaluation failed:\n%s" % (k, r.stderr[-2000:]))
                runs[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out["plain_evaluate_wall_ms_eager_by_tree"] = {k: {"median_of_medians": statistics.median(x["median"] for x in v), "runs": v} for k, v in runs.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
