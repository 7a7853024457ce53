"""Time a full training iteration (rollout + update, graph mode) of go2_flat (PPO) and go2_flat_cts (CTS) on one GPU with algorithm.diagnostics off and on: the key adds
per mini-batch step two launches behind go2nn_ppo_heads (go2nn_ppo_diag: the pass and its one-block finish) and two in front of every clip + Adam call
(go2nn_grad_sqnorm), all inside the captured update, plus one fill in front of the update and one device -> host copy behind it.  Each setting runs in a fresh child
process, --repeats times, alternating, so the figure can be read against the run-to-run spread of the key-off runs of the same session.  A third kind of child times the
launches alone at the update's shape (24576 rows, 12 actions, 128 hidden units; the gradient tensors of the go2_flat actor-critic): device events around --calls
back-to-back calls, next to a device-to-device copy of the bytes the pass reads (y_a, y_c) in the same process.
Prints ONE JSON line and writes it to profiles/update_diag_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures of the same session).
    python tools/update_diag_bench.py [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3] [--calls 50]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ("go2_flat", "go2_flat_cts")


def child(task, envs, iters, warmup, on):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("GO2_STRICT_GRAPHS", "1")          # no figure from an update that silently degraded to eager
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(envs), "--headless", "--seed", "1"] + (["--diagnostics"] if on else []))
    env, _ = task_registry.make_env(task, args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
    assert (runner.alg.diagnostics_table is not None or runner.alg._diag is not None) == bool(on)
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
           "graphs": runner.graphs_captured(), "finite": bool(torch.isfinite(w).all()), "steps_per_update": runner.alg.num_learning_epochs * runner.alg.num_mini_batches}
    if on:
        d = runner.alg.diagnostics
        d = d["all"] if "all" in d else d
        out["figures"] = {k: d[k] for k in ("clip_fraction", "approx_kl", "kl", "explained_variance", "grad_norm", "grad_clipped_share")}
    return out


def kernels(calls, B=24576, A=12, K=128):
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    lib, dev = _nn.load_nn(), "cuda:0"
    torch.manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev)
    t = dict(y_a=torch.nn.functional.elu(r(B, K)), y_c=torch.nn.functional.elu(r(B, K)), w_mu=r(A, K) / K ** 0.5, b_mu=0.1 * r(A), w_v=r(1, K) / K ** 0.5, b_v=0.1 * r(1),
             std=0.5 + torch.rand(A, device=dev), actions=r(B, A), old_mu=r(B, A), old_sigma=0.5 + torch.rand(B, A, device=dev), old_logp=-10.0 + r(B), adv=r(B),
             old_values=r(B), returns=r(B))
    keys = ("y_a", "y_c", "w_mu", "b_mu", "w_v", "b_v", "std", "actions", "old_mu", "old_sigma", "old_logp", "adv", "old_values", "returns")
    slots = 1 << 20
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"rows": B, "actions": A, "hidden": K, "calls": calls, "device": torch.cuda.get_device_name(0), "pass_bytes_read": 4 * (2 * B * K + 3 * B * A + 4 * B)}

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(1e3 * e0.elapsed_time(e1) / calls)
        return {"us_per_call_median": sorted(runs)[2], "us_per_call_min": min(runs), "us_per_call_max": max(runs)}
    for split in (0, 18432):
        segs = 2 if split else 1
        part = torch.zeros(lib.go2nn_ppo_diag_rows(B, A, K) * segs * _nn.GO2NN_DIAG_NUM, dtype=torch.float64, device=dev)
        table = torch.zeros(4096 * segs * _nn.GO2NN_DIAG_NUM, dtype=torch.float64, device=dev)
        cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _nn.Go2nnPpoDiag(*[t[k].data_ptr() for k in keys], part.data_ptr(), table.data_ptr(), cursor.data_ptr(), B, A, K, split, 4096, 0.2)

        def call(d=d, cursor=cursor):          # (4096 slots: the cursor stays inside the table for every timed call, so the finish does its full work)
            assert lib.go2nn_ppo_diag(C.byref(d), stream) == 0
        res["ppo_diag_pass_and_finish_%d_segment%s" % (segs, "s" if segs > 1 else "")] = timed(call)
    # the gradient tensors of the go2_flat actor-critic: actor 45-512-256-128-12, critic 263-512-256-128-1, std
    sizes = [a * b for dims in ((45, 512, 256, 128, 12), (263, 512, 256, 128, 1)) for a, b in zip(dims[:-1], dims[1:])] + \
            [b for dims in ((45, 512, 256, 128, 12), (263, 512, 256, 128, 1)) for b in dims[1:]] + [12]
    grads = [r(n) for n in sizes]
    ptrs = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    numel = (C.c_int32 * len(grads))(*[g.numel() for g in grads])
    gpart = torch.zeros(lib.go2nn_grad_sqnorm_rows(numel, len(grads)), dtype=torch.float64, device=dev)
    gout, gcur = torch.zeros(slots, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def gcall():
        assert lib.go2nn_grad_sqnorm(ptrs, numel, len(grads), gpart.data_ptr(), gout.data_ptr(), gcur.data_ptr(), slots, stream) == 0
    res["grad_sqnorm"] = dict(timed(gcall), tensors=len(grads), floats=sum(sizes))
    src, dst = torch.randn(2 * B * K, device=dev), torch.empty(2 * B * K, device=dev)
    res["device_to_device_copy_of_y_a_y_c"] = dict(timed(lambda: dst.copy_(src)), bytes=8 * B * K)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_diag_bench.json"))
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "on", "kernels"])
    ap.add_argument("--task", default="go2_flat")
    ap.add_argument("--child_timeout", type=int, default=180, help="seconds a child process may take")
    a = ap.parse_args()
    if a.child:
        print("UPDATE_DIAG_BENCH_CHILD " + json.dumps(kernels(a.calls) if a.child == "kernels" else child(a.task, a.envs, a.iters, a.warmup, a.child == "on")))
        return

    def run(name, task="go2_flat"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--task", task, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup),
                                "--calls", str(a.calls)], capture_output=True, text=True, cwd=ROOT, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:          # (the child is killed; the session ends as after any failed child)
            return {"error": "no result within %d s" % a.child_timeout}
        line = [l for l in r.stdout.splitlines() if l.startswith("UPDATE_DIAG_BENCH_CHILD ")]
        return json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
    out = {"envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "tasks": {}}
    failed = False          # a child that failed ends the session: nothing more is started on the GPU behind it
    for task in [t for t in a.tasks.split(",") if t]:
        res = {"off": [], "on": []}
        for _ in range(a.repeats):
            for name in ("off", "on"):
                if not failed:
                    res[name].append(run(name, task))
                    failed = "error" in res[name][-1]
        ok = {k: [x for x in res[k] if "ms_per_iter" in x] for k in ("off", "on")}
        if ok["off"] and ok["on"]:
            med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
            for key in ("ms_per_iter", "rollout_ms", "update_ms"):
                off, on = med(ok["off"], key), med(ok["on"], key)
                res["median_" + key] = {"off": off, "on": on, "cost_ms": on - off, "cost_pct": 100.0 * (on - off) / off,
                                        "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
            res["cost_us_per_mini_batch_step"] = 1e3 * res["median_update_ms"]["cost_ms"] / ok["on"][0]["steps_per_update"]
        out["tasks"][task] = res
    if not failed:
        out["launches"] = run("kernels")
        failed = "error" in out["launches"]
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
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
