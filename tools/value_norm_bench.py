"""Time a full iteration (rollout + update, graph mode) of go2_flat and go2_flat_cts on one GPU with algorithm.normalize_value off and on: the switch adds one launch
to the rollout's first step (go2nn_value_head_fold in front of go2nn_pack), one to compute_returns (go2nn_value_norm_apply) and one plain launch behind the captured
update (go2nn_value_norm_update).  Each setting runs in a fresh child process, --repeats times, alternating, so the figure can be read against the run-to-run spread of
the same session.  A third kind of child times the three launches alone: device events around --calls back-to-back calls at envs x 24 values and returns, next to a
device-to-device copy of the bytes the apply launch reads in the same process.  At 4096 x 24 = 98 304 floats all of this is launch latency, not bandwidth.
Prints ONE JSON line and writes it to profiles/value_norm_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures of the same session).
    python tools/value_norm_bench.py [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3] [--calls 200] [--tasks go2_flat,go2_flat_cts]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(task, envs, iters, warmup, on):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("GO2_STRICT_GRAPHS", "1")          # no figure from a rollout that silently degraded to eager
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(envs), "--headless", "--seed", "1"] + (["--normalize_value"] if on else []))
    env, _ = task_registry.make_env(task, args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
    assert hasattr(runner.alg.actor_critic, "value_normalizer") == bool(on)
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
           "graphs": runner.graphs_captured(), "returns_graph": bool(runner._returns_graph is not None and runner._returns_graph.graph is not None),
           "finite": bool(torch.isfinite(w).all())}
    if on:
        vn = runner.alg.actor_critic.value_normalizer
        out["count"], out["return_mean_std"] = float(vn.count), runner.alg.return_stats
    return out


def kernels(envs, calls):
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    lib, dev, n = _nn.load_nn(), "cuda:0", envs * 24
    torch.manual_seed(0)
    rows = int(lib.go2nn_value_norm_partial_rows(n))
    values, returns = torch.randn(n, device=dev) + 20.0, torch.randn(n, device=dev) + 20.0
    stat = torch.tensor([20.0, 1.01, 1.0 / 1.01], device=dev)          # (in place over and over: the data drift towards 0, the work does not change)
    partials = torch.zeros(rows, 2, dtype=torch.float64, device=dev)
    state = torch.zeros(3, dtype=torch.float64, device=dev)
    w, b, wo, bo = torch.randn(1, 128, device=dev), torch.randn(1, device=dev), torch.empty(1, 128, device=dev), torch.empty(1, device=dev)
    src, dst = torch.randn(2 * n, device=dev), torch.empty(2 * n, device=dev)
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

    stat_u = stat.clone()
    return {"envs": envs, "floats": n, "calls": calls, "apply_bytes_read": 8 * n, "apply_bytes_written": 8 * n + 16 * rows,
            "apply_in_place_with_partials": timed(lambda: _nn.value_norm_apply(lib, values, returns, stat, partials, stream)),
            "apply_in_place_without_partials": timed(lambda: _nn.value_norm_apply(lib, values, returns, stat, None, stream)),
            "device_to_device_copy_same_bytes": timed(lambda: dst.copy_(src)),
            "update_%d_rows" % rows: timed(lambda: _nn.value_norm_update(lib, partials, state, n, 1e-2, stat_u, stream=stream)),
            "update_with_preservation_K128": timed(lambda: _nn.value_norm_update(lib, partials, state, n, 1e-2, stat_u, w, b, stream)),
            "fold_K128": timed(lambda: _nn.value_head_fold(lib, w, b, stat, wo, bo, stream)), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--tasks", default="go2_flat,go2_flat_cts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "value_norm_bench.json"))
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "on", "kernels"])
    ap.add_argument("--task", default="go2_flat")
    a = ap.parse_args()
    if a.child:
        print("VALUE_NORM_BENCH_CHILD " + json.dumps(kernels(a.envs, a.calls) if a.child == "kernels" else child(a.task, a.envs, a.iters, a.warmup, a.child == "on")))
        return

    def run(name, task="go2_flat"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--task", task, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup),
                            "--calls", str(a.calls)], capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("VALUE_NORM_BENCH_CHILD ")]
        return json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
    out = {"envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "tasks": {}}
    for task in [t for t in a.tasks.split(",") if t]:
        res = {"off": [], "on": []}
        for _ in range(a.repeats):
            for name in ("off", "on"):
                res[name].append(run(name, task))
        ok = {k: [x for x in res[k] if "ms_per_iter" in x] for k in ("off", "on")}
        if ok["off"] and ok["on"]:
            med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
            for key in ("ms_per_iter", "rollout_ms", "update_ms"):
                off, on = med(ok["off"], key), med(ok["on"], key)
                res["median_" + key] = {"off": off, "on": on, "cost_ms": on - off, "cost_pct": 100.0 * (on - off) / off,
                                        "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
        out["tasks"][task] = res
    out["launches"] = run("kernels")
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
