"""Time task go2_flat_rnn (ActorCriticRecurrent: LSTM, 256 units) per PPO iteration on one GPU, rollout and update apart, for the library's kernels (the memory on
include/go2nn.h ABI 7, the whole update one HIP graph) and for the reference formulation (GO2_FUSED_MLP=0: torch nn.LSTM — MIOpen — over the split / pad
generator) on the same box.  Each formulation runs in a fresh child process.  Prints ONE JSON line.
    python tools/rnn_bench.py [--envs 4096] [--iters 10] [--warmup 4]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(envs, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat_rnn", "--num_envs", str(envs), "--headless", "--seed", "1"])
    env, _ = task_registry.make_env("go2_flat_rnn", args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat_rnn", args, log_root=None)
    runner.learn(warmup)
    coll, learn = [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        runner.learn(1)
        coll.append(runner.last_collection_time)
        learn.append(runner.last_learn_time)
    total = time.time() - t0
    w = torch.cat([p.detach().reshape(-1) for p in runner.alg.actor_critic.parameters()])
    return {"ms_per_iter": 1e3 * total / iters, "rollout_ms": 1e3 * sum(coll) / iters, "update_ms": 1e3 * sum(learn) / iters,
            "graphs": runner.graphs_captured(), "finite": bool(torch.isfinite(w).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RNN_BENCH_CHILD " + json.dumps(child(a.envs, a.iters, a.warmup)))
        return
    out = {"task": "go2_flat_rnn", "envs": a.envs, "iters": a.iters}
    for name, extra in (("hip", {}), ("reference_fused_mlp_0", {"GO2_FUSED_MLP": "0"})):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup)],
                           env=dict(os.environ, **extra), capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("RNN_BENCH_CHILD ")]
        if r.returncode != 0 or not line:
            out[name] = {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
            continue
        out[name] = json.loads(line[-1].split(" ", 1)[1])
    if "ms_per_iter" in out.get("hip", {}) and "ms_per_iter" in out.get("reference_fused_mlp_0", {}):
        out["speedup"] = out["reference_fused_mlp_0"]["ms_per_iter"] / out["hip"]["ms_per_iter"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
