"""What `algorithm.smooth_loss_coef` costs on one GPU (go2_flat, graph mode):
  * a full PPO iteration (rollout + update) with the coefficient 0 ("off": random-row mini-batches, none of the new launches), tiny ("tiny", 1e-12: env-block
    mini-batches and both new launches, a term too small to move a weight — what the layout and the launches cost by themselves) and COEF ("on"); each setting in a
    fresh child process, --repeats times, alternating, so the figures can be read against the run-to-run spread of the coefficient-0 runs of the same session;
  * the launches alone at the update's shape (one block of 24 steps x envs / 4 environments, 12 actions, 128 hidden units): device events around --launches back-to-back
    calls of go2nn_smooth_loss at every time-segment count of --segments (0: the launch's own choice), of go2nn_smooth_indices, of go2nn_mirror_loss at the same number of
    rows and of a device-to-device copy of the bytes the loss pass moves (y_a read, gz_a read and written), all in one process.
Prints ONE JSON line and writes it to profiles/smooth_loss_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures of the same session).
    python tools/smooth_loss_bench.py [--smooth_loss 0.5] [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3] [--launches 50] [--segments 0,1,2,3,4,6,8,12]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 1e-12


def child_iteration(envs, iters, warmup, coef):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("GO2_STRICT_GRAPHS", "1")          # no figure from an update that silently degraded to eager
    import torch
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    args = get_args(["--task", "go2_flat", "--num_envs", str(envs), "--headless", "--seed", "1"] + (["--smooth_loss", repr(coef)] if coef > 0 else []))
    env, _ = task_registry.make_env("go2_flat", args)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    assert runner.alg.smooth_loss_coef == coef
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
    return {"ms_per_iter": 1e3 * total / iters, "rollout_ms": 1e3 * sum(coll) / iters, "update_ms": 1e3 * sum(learn) / iters, "graphs": runner.graphs_captured(),
            "finite": bool(torch.isfinite(w).all()), "smooth_loss": runner.alg.smooth_loss}


def child_launch(envs, launches, segments, steps=24, nmb=4, A=12, K=128):
    """go2nn_smooth_loss and go2nn_smooth_indices alone at the shapes the update gives them, next to go2nn_mirror_loss on as many rows and a copy of the same bytes"""
    sys.path.insert(0, ROOT)
    import torch
    from go2_rl_gym_amd import _nn
    from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg
    from go2_rl_gym_amd.utils.symmetry import mirror_tables
    lib, dev = _nn.load_nn(), "cuda:0"
    n = envs // nmb
    R = steps * n
    y, gz = torch.nn.functional.elu(torch.randn(R, K, device=dev)), 1e-3 * torch.randn(R, K, device=dev)
    w, b = torch.randn(A, K, device=dev) / K ** 0.5, torch.randn(A, device=dev)
    pw = (torch.rand(steps, n, device=dev) >= 0.02).to(torch.uint8)
    pw[steps - 1] = 0
    cols = lib.go2nn_smooth_loss_cols(A, K)
    part = torch.empty((R // 2 + 1) * cols, device=dev)          # (room for every segment count: at most one workgroup per two rows)
    m = _nn.Go2nnSmoothLoss(y.data_ptr(), w.data_ptr(), b.data_ptr(), pw.data_ptr(), gz.data_ptr(), part.data_ptr(), 1, steps, n, A, K, 0.5)
    perm, sign = _nn.mirror_loss_table_tensors(lib, mirror_tables(GO2Cfg()).action, dev)
    mrows = lib.go2nn_mirror_loss_rows(R // 2, A, K)
    mpart = torch.empty(mrows * lib.go2nn_mirror_loss_cols(A, K), device=dev)
    mm = _nn.Go2nnMirrorLoss(y.data_ptr(), w.data_ptr(), b.data_ptr(), perm.data_ptr(), sign.data_ptr(), gz.data_ptr(), mpart.data_ptr(), R // 2, A, K, 0.5)
    idx, iw = torch.empty(steps * envs, dtype=torch.int64, device=dev), torch.empty(steps * envs, dtype=torch.uint8, device=dev)
    dones, key = (torch.rand(steps * envs, device=dev) < 0.02).to(torch.uint8), torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    moved = 3 * 4 * R * K          # bytes: y_a read, gz_a read and written
    a = torch.empty(moved // 8, dtype=torch.float32, device=dev)          # a copy that reads moved / 2 bytes and writes moved / 2
    c = torch.empty_like(a)

    def smooth():
        assert lib.go2nn_smooth_loss(C.byref(m), stream) == 0, lib.go2nn_last_error()

    def mirror():
        assert lib.go2nn_mirror_loss(C.byref(mm), stream) == 0, lib.go2nn_last_error()

    def indices():
        assert lib.go2nn_smooth_indices(idx.data_ptr(), iw.data_ptr(), dones.data_ptr(), nmb, steps, envs, key.data_ptr(), stream) == 0, lib.go2nn_last_error()

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
    out = {"rows": R, "T": steps, "n": n, "A": A, "K": K, "bytes_moved": moved, "launches": launches, "smooth_loss": {}}
    rate = lambda ms: {"us": 1e3 * ms, "GB_per_s": moved / (ms * 1e-3) / 1e9}
    for rep in ("", "_again"):
        for S in segments:
            assert lib.go2nn_smooth_loss_set_segments(S) == 0
            out["smooth_loss"]["segments_%d%s" % (S, rep)] = dict(rate(timed(smooth)), workgroups=lib.go2nn_smooth_loss_rows(1, steps, n, A, K))
        lib.go2nn_smooth_loss_set_segments(0)
        out["mirror_loss" + rep] = dict(rate(timed(mirror)), pairs=R // 2, workgroups=mrows)
        out["copy" + rep] = rate(timed(lambda: c.copy_(a)))
        out["smooth_indices" + rep] = {"us": 1e3 * timed(indices), "rows": steps * envs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smooth_loss", type=float, default=0.5, metavar="COEF")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--segments", default="0,1,2,3,4,6,8,12", help="the time-segment counts of go2nn_smooth_loss to time (0: the launch's own choice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_loss_bench.json"))
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "tiny", "on", "launch"])
    a = ap.parse_args()
    coefs = {"off": 0.0, "tiny": TINY, "on": a.smooth_loss}
    if a.child:
        res = child_launch(a.envs, a.launches, [int(s) for s in a.segments.split(",")]) if a.child == "launch" else child_iteration(a.envs, a.iters, a.warmup, coefs[a.child])
        print("SMOOTH_BENCH_CHILD " + json.dumps(res))
        return

    def run(name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup),
                            "--launches", str(a.launches), "--segments", a.segments, "--smooth_loss", repr(a.smooth_loss)], capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("SMOOTH_BENCH_CHILD ")]
        print("[smooth_loss_bench] %s: %s" % (name, line[-1][19:] if line else "exit %d" % r.returncode), file=sys.stderr, flush=True)
        return json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])}
    out = {"task": "go2_flat", "envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "settings": {"off": "smooth_loss_coef 0 (random-row mini-batches)", "tiny": "smooth_loss_coef %g (env-block mini-batches, both launches, no effect on the weights)" % TINY,
                        "on": "smooth_loss_coef %g" % a.smooth_loss}, "off": [], "tiny": [], "on": []}
    out["launches_alone"] = run("launch")
    for _ in range(a.repeats):
        for name in ("off", "tiny", "on"):
            out[name].append(run(name))
    ok = {k: [x for x in out[k] if "ms_per_iter" in x] for k in ("off", "tiny", "on")}
    if all(ok.values()):
        med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
        for key in ("ms_per_iter", "update_ms", "rollout_ms"):
            off = med(ok["off"], key)
            out["median_" + key] = {"off": off, "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
            for k in ("tiny", "on"):
                v = med(ok[k], key)
                out["median_" + key][k] = {"value": v, "cost_ms": v - off, "ratio": v / off}
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
