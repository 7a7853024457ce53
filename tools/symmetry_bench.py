"""What `algorithm.symmetry` costs on one GPU (go2_flat, graph mode):
  * a full PPO iteration (rollout + update) with the flag off and on — the update runs on twice the rows, so roughly the update doubles; each setting in a fresh child
    process, --repeats times, alternating, so the figure can be read against the run-to-run spread of the same session;
  * the go2nn_mirror_rows launch alone at the update's shapes (the nine tensors of the rollout, num_mini_batches chunks): device events around --launches back-to-back
    launches, the bytes it moves (every source float read once, written twice) and GB/s, next to a device-to-device copy moving the same bytes in the same process.
Prints ONE JSON line and writes it to profiles/symmetry_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures of the same session).
    python tools/symmetry_bench.py [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3] [--launches 50]
With --mirror_loss COEF the same harness measures what `algorithm.mirror_loss_coef` costs instead: both settings run with symmetry on, "off" with the coefficient 0 and
"on" with COEF, and the launch timed alone is go2nn_mirror_loss at the update's shape (envs x 24 / 4 pairs, 12 actions, 128 hidden units: it reads y_a once and reads and
writes gz_a) next to a device-to-device copy of the same bytes; the result goes to profiles/mirror_loss_bench.json.
    python tools/symmetry_bench.py --mirror_loss 0.5"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_iteration(envs, iters, warmup, on, mirror_loss=None):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("GO2_STRICT_GRAPHS", "1")          # no figure from an update that silently degraded to eager
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(envs), "--headless", "--seed", "1"] + (["--symmetry"] if on or mirror_loss is not None else []) +
                    (["--mirror_loss", str(mirror_loss)] if on and mirror_loss is not None else []))
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    assert (runner.alg._sym is not None) == bool(on or mirror_loss is not None) and runner.alg.mirror_loss_coef == (mirror_loss if on and mirror_loss is not None else 0.0)
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
    return {"ms_per_iter": 1e3 * total / iters, "rollout_ms": 1e3 * sum(coll) / iters, "update_ms": 1e3 * sum(learn) / iters,
            "graphs": runner.graphs_captured(), "finite": bool(torch.isfinite(w).all())}


def child_launch(envs, launches, steps=24, nmb=4):
    """the mirror launch alone, at the shapes PPO._sym_setup gives it"""
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg
    from go2_rl_gym_amd.utils.symmetry import mirror_tables
    lib, dev, t = _nn.load_nn(), "cuda:0", mirror_tables(GO2Cfg())
    rows = envs * steps
    mb = rows // nmb
    tabs = {k: _nn.mirror_table_tensors(lib, v, dev) for k, v in (("obs", t.obs), ("cobs", t.privileged_obs), ("act", t.action), ("mu", t.action), ("sig", t.action_std))}
    widths = (("obs", 45), ("cobs", 263), ("act", 12), ("val", 1), ("adv", 1), ("ret", 1), ("logp", 1), ("mu", 12), ("sig", 12))
    src = {k: torch.randn(nmb * mb, w, device=dev) for k, w in widths}
    dst = {k: torch.empty(nmb, 2 * mb, w, device=dev) for k, w in widths}
    jobs = _nn.mirror_jobs([(src[k], dst[k], tabs.get(k)) for k, _ in widths])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    moved = 3 * 4 * nmb * mb * sum(w for _, w in widths)          # bytes: every source float read once, written twice (the gathered re-read stays inside the row)
    a = torch.empty(moved // 8, dtype=torch.float32, device=dev)          # a copy that reads moved / 2 bytes and writes moved / 2
    b = torch.empty_like(a)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches          # ms
    out = {"rows": nmb * mb, "floats_per_row": sum(w for _, w in widths), "bytes_moved": moved, "launches": launches}
    for name, fn in (("mirror", lambda: _nn.mirror_rows(lib, jobs, nmb, mb, stream)), ("copy", lambda: b.copy_(a)), ("mirror_again", lambda: _nn.mirror_rows(lib, jobs, nmb, mb, stream)),
                     ("copy_again", lambda: b.copy_(a))):
        ms = timed(fn)
        out[name] = {"us": 1e3 * ms, "GB_per_s": moved / (ms * 1e-3) / 1e9}
    return out


def child_mirror_loss_launch(envs, launches, steps=24, nmb=4, A=12, K=128):
    """go2nn_mirror_loss alone at the shape fused.pair_grads gives it: one augmented mini-batch of 2 x (envs x steps / nmb) rows"""
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg
    from go2_rl_gym_amd.utils.symmetry import mirror_tables
    lib, dev = _nn.load_nn(), "cuda:0"
    B = envs * steps // nmb
    perm, sign = _nn.mirror_loss_table_tensors(lib, mirror_tables(GO2Cfg()).action, dev)
    y, gz = torch.nn.functional.elu(torch.randn(2 * B, K, device=dev)), 1e-3 * torch.randn(2 * B, K, device=dev)
    w, b = torch.randn(A, K, device=dev) / K ** 0.5, torch.randn(A, device=dev)
    rows, cols = lib.go2nn_mirror_loss_rows(B, A, K), lib.go2nn_mirror_loss_cols(A, K)
    part = torch.empty(rows * cols, device=dev)
    m = _nn.Go2nnMirrorLoss(y.data_ptr(), w.data_ptr(), b.data_ptr(), perm.data_ptr(), sign.data_ptr(), gz.data_ptr(), part.data_ptr(), B, A, K, 0.5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    moved = 3 * 4 * 2 * B * K          # bytes: y_a read, gz_a read and written
    a = torch.empty(moved // 8, dtype=torch.float32, device=dev)          # a copy that reads moved / 2 bytes and writes moved / 2
    c = torch.empty_like(a)

    def launch():
        assert lib.go2nn_mirror_loss(C.byref(m), stream) == 0, lib.go2nn_last_error()

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches          # ms
    out = {"pairs": B, "A": A, "K": K, "workgroups": rows, "bytes_moved": moved, "launches": launches}
    for name, fn in (("mirror_loss", launch), ("copy", lambda: c.copy_(a)), ("mirror_loss_again", launch), ("copy_again", lambda: c.copy_(a))):
        ms = timed(fn)
        out[name] = {"us": 1e3 * ms, "GB_per_s": moved / (ms * 1e-3) / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--mirror_loss", type=float, default=None, metavar="COEF", help="measure the mirror loss instead: symmetry on in both settings, coefficient 0 against COEF")
    ap.add_argument("--out", default=None, help="default: profiles/symmetry_bench.json, with --mirror_loss profiles/mirror_loss_bench.json")
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "on", "launch"])
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mirror_loss_bench.json" if a.mirror_loss is not None else "symmetry_bench.json")
    if a.child:
        if a.child == "launch":
            res = child_launch(a.envs, a.launches) if a.mirror_loss is None else child_mirror_loss_launch(a.envs, a.launches)
        else:
            res = child_iteration(a.envs, a.iters, a.warmup, a.child == "on", a.mirror_loss)
        print("SYMMETRY_BENCH_CHILD " + json.dumps(res))
        return

    def run(name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup),
                            "--launches", str(a.launches)] + (["--mirror_loss", str(a.mirror_loss)] if a.mirror_loss is not None else []), capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("SYMMETRY_BENCH_CHILD ")]
        print("[symmetry_bench] %s: %s" % (name, line[-1][21:] if line else "exit %d" % r.returncode), file=sys.stderr, flush=True)
        return json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
    out = {"task": "go2_flat", "envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "off": [], "on": []}
    if a.mirror_loss is not None:
        out["settings"] = {"off": "symmetry on, mirror_loss_coef 0", "on": "symmetry on, mirror_loss_coef %g" % a.mirror_loss}
    for _ in range(a.repeats):
        for name in ("off", "on"):
            out[name].append(run(name))
    out["mirror_launch" if a.mirror_loss is None else "mirror_loss_launch"] = run("launch")
    ok = {k: [x for x in out[k] if "ms_per_iter" in x] for k in ("off", "on")}
    if ok["off"] and ok["on"]:
        med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
        for key in ("ms_per_iter", "update_ms", "rollout_ms"):
            off, on = med(ok["off"], key), med(ok["on"], key)
            out["median_" + key] = {"off": off, "on": on, "cost_ms": on - off, "ratio": on / off,
                                    "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
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
