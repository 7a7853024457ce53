"""Time a full go2_flat PPO iteration (rollout + update, graph mode) on one GPU with domain_rand.randomize_sensors off and on: the flag adds two launches per policy
step to the rollout's dependent chain (go2nn_sensor_rand_apply: the frame kernel and the cursor launch) and takes one redirected write out of the step kernel.  Each
setting runs in a fresh child process, --repeats times, alternating, so the figure can be read against the run-to-run spread of the same session.  Prints ONE JSON line
and writes it to profiles/sensor_rand_bench.json (--out; keys given with --note KEY=VALUE are merged in, e.g. bench.py figures taken in the same session).
    python tools/sensor_rand_bench.py [--envs 4096] [--iters 20] [--warmup 6] [--repeats 3]"""
import argparse
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
    args = get_args(["--task", "go2_flat", "--num_envs", str(envs), "--headless", "--seed", "1"])
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    env_cfg.domain_rand.randomize_sensors = bool(on)
    env, _ = task_registry.make_env("go2_flat", args, env_cfg=env_cfg)
    torch.manual_seed(1)
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
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
            "rollout_graph": runner._rollout_graph is not None, "finite": bool(torch.isfinite(w).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_rand_bench.json"))
    ap.add_argument("--note", action="append", default=[], help="KEY=VALUE (VALUE read as JSON when it parses) merged into the result")
    ap.add_argument("--child", choices=["off", "on"])
    a = ap.parse_args()
    if a.child:
        print("SENSOR_RAND_BENCH_CHILD " + json.dumps(child(a.envs, a.iters, a.warmup, a.child == "on")))
        return
    out = {"task": "go2_flat", "envs": a.envs, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "off": [], "on": []}
    for _ in range(a.repeats):
        for name in ("off", "on"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, cwd=ROOT)
            line = [l for l in r.stdout.splitlines() if l.startswith("SENSOR_RAND_BENCH_CHILD ")]
            out[name].append(json.loads(line[-1].split(" ", 1)[1]) if r.returncode == 0 and line else {"error": "exit %d: %s" % (r.returncode, r.stderr[-600:])})
    ok = {k: [x for x in out[k] if "ms_per_iter" in x] for k in ("off", "on")}
    if ok["off"] and ok["on"]:
        med = lambda xs, key: sorted(x[key] for x in xs)[len(xs) // 2]
        for key in ("ms_per_iter", "rollout_ms"):
            off, on = med(ok["off"], key), med(ok["on"], key)
            out["median_" + key] = {"off": off, "on": on, "cost_ms": on - off, "cost_pct": 100.0 * (on - off) / off,
                                    "off_spread_pct": 100.0 * (max(x[key] for x in ok["off"]) - min(x[key] for x in ok["off"])) / off}
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
