"""Time a full go2_flat PPO iteration (rollout + update, graph mode) on one GPU with runner.empirical_normalization off and on: the switch adds one launch per policy
step to the rollout's dependent chain (go2nn_obs_norm_apply, both observation streams), one to compute_returns and two plain launches behind the captured update
(go2nn_obs_norm_update per stream).  Each setting runs in a fresh child process, --repeats times, alternating, so the figure can be read against the run-to-run spread of
the same session.  A third kind of child times the launches alone: the apply launch at envs x (45 + 263) floats, in place, with partial tables, and the update launch
over 24 steps' tables, device events around --calls back-to-back calls, next to a device-to-device copy of the bytes the apply launch reads in the same process.
Prints ONE JSON line and writes it to profiles/obs_norm_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures of the same session).
    python tools/obs_norm_bench.py [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3] [--calls 200]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(envs, iters, warmup, on):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("GO2_STRICT_GRAPHS", "1")          # no figure from a rollout that silently degraded to eager
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(envs), "--headless", "--seed", "1"] + (["--normalize_obs"] if on else []))
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    assert hasattr(runner.alg.actor_critic, "obs_normalizer") == bool(on)
    runner.learn(warmup, init_at_random_ep_len=True)
    coll, learn = [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        runner.learn(1)
        coll.append(runner.last_collection_time)
        learn.append(runner.last_learn_time)
    total = time.time() - t0
    w = torch.cat([p.detach().reshape(-1) for p in runner.alg.actor_critic.parameters()])
    out = {"ms_per_iter": 1e3 * total / iters, "rollout_ms": 1e3 * sum(coll) / iters, "update_ms": 1e3 * sum(learn) / iters,
           "graphs": runner.graphs_captured(), "finite": bool(torch.isfinite(w).all())}
    if on:
        out["count"] = float(runner.alg.actor_critic.obs_normalizer.count)
    return out


def kernels(envs, calls):
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    lib, dev, T = _nn.load_nn(), "cuda:0", 24
    torch.manual_seed(0)
    rows = int(lib.go2nn_obs_norm_partial_rows(envs))
    xs = [torch.randn(envs, D, device=dev) for D in (45, 263)]
    stats = [(torch.randn(D, device=dev) * 0.1, torch.rand(D, device=dev) + 0.5) for D in (45, 263)]
    tables = [torch.zeros(T, rows, D, 2, dtype=torch.float64, device=dev) for D in (45, 263)]
    states = [torch.zeros(1 + 2 * D, dtype=torch.float64, device=dev) for D in (45, 263)]
    jobs = _nn.obs_norm_jobs([(x, x, m, i, t[0], 10.0) for x, (m, i), t in zip(xs, stats, tables)])
    src, dst = torch.randn(envs * (45 + 263), device=dev), torch.empty(envs * (45 + 263), device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best.append(1e3 * e0.elapsed_time(e1) / calls)
        return {"us_per_call_median": sorted(best)[2], "us_per_call_min": min(best), "us_per_call_max": max(best)}

    def update():
        for t, s, (m, i) in zip(tables, states, stats):
            _nn.obs_norm_update(lib, t, s, envs * T, 1e-2, m, i, stream)
    nbytes = 4 * envs * (45 + 263)
    out = {"envs": envs, "calls": calls, "apply_bytes_read": nbytes, "apply_bytes_written": nbytes + 16 * rows * (45 + 263),
           "apply_in_place_with_partials": timed(lambda: _nn.obs_norm_apply(lib, jobs, envs, stream)),
           "device_to_device_copy_same_bytes": timed(lambda: dst.copy_(src)),
           "update_both_streams_24_steps": timed(update), "device": torch.cuda.get_device_name(0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm_bench.json"))
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "on", "kernels"])
    a = ap.parse_args()
    if a.child:
        print("OBS_NORM_BENCH_CHILD " + json.dumps(kernels(a.envs, a.calls) if a.child == "kernels" else child(a.envs, a.iters, a.warmup, a.child == "on")))
        return

    def run(name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup),
                            "--calls", str(a.calls)], capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("OBS_NORM_BENCH_CHILD ")]
        return json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
    out = {"task": "go2_flat", "envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "off": [], "on": []}
    for _ in range(a.repeats):
        for name in ("off", "on"):
            out[name].append(run(name))
    out["launches"] = run("kernels")
    ok = {k: [x for x in out[k] if "ms_per_iter" in x] for k in ("off", "on")}
    if ok["off"] and ok["on"]:
        med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
        for key in ("ms_per_iter", "rollout_ms", "update_ms"):
            off, on = med(ok["off"], key), med(ok["on"], key)
            out["median_" + key] = {"off": off, "on": on, "cost_ms": on - off, "cost_pct": 100.0 * (on - off) / off,
                                    "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
        out["rollout_share_of_cost"] = out["median_rollout_ms"]["cost_ms"] / out["median_ms_per_iter"]["cost_ms"] if out["median_ms_per_iter"]["cost_ms"] else None
        out["cost_us_per_policy_step"] = 1e3 * out["median_rollout_ms"]["cost_ms"] / 24
    for note in a.note:
        k, _, v = note.partition("=")
        try:
            out[k] = json.loads(v)
        except ValueError:
            out[k] = v
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
