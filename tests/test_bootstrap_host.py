"""The evaluator's bootstrap on the CPU: the host build of go2nn_eval_bootstrap (include/go2nn.h) against a restatement in Python integers and numpy float64 written here
— bit for bit: the draws are integer arithmetic and the sums run in the draws' order —, its refusals, what the replicates say statistically, PolicyEvaluator with
`evaluation.bootstrap` off and on, the paired comparison and the CLI.  tests/test_gpu_bootstrap.py runs the same cases on the device."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import yaml

from helpers import load_nn_emu, load_oracle
from test_eval_host import EVAL, make_evaluator, small_actor_critic
from test_sensor_host import philox_int
from go2_rl_gym_amd._nn import EVAL_METRICS, GO2NN_EVAL_NUM

COLS = GO2NN_EVAL_NUM + 2
EINVAL = -22
TAG = 7
FALLS = EVAL_METRICS.index("falls")
# N: the cells' sizes.  37: an empty cell, one robot, five (a Philox block of four draws and a ragged one), 31;  300: cells of 3 and 4 (the block boundary) and one wider
# than a workgroup.  Every env belongs to a cell, as in the evaluator.
CASES = {37: (0, 1, 5, 31), 300: (3, 4, 293)}
BS = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


def p(a):
    return C.c_void_p(a.ctypes.data)


def case(N, seed=11):
    """-> (acc fp32 [NUM, N] of both signs over many decades with exact zeros, the falls row whole numbers with zeros; cell_start [G + 1]; cell_envs [N], ascending within a
    cell, the cells interleaved over the env indices)"""
    rng = np.random.default_rng(seed + N)
    acc = (rng.normal(0, 1, (GO2NN_EVAL_NUM, N)) * np.exp(rng.normal(0, 6, (GO2NN_EVAL_NUM, N)))).astype(np.float32)
    acc[rng.random(acc.shape) < 0.1] = 0.0
    acc[1, 0], acc[2, N - 1] = 3.0e37, -3.0e37
    acc[0] = 50.0
    acc[FALLS] = (rng.random(N) < 0.4) * rng.integers(1, 4, N)
    sizes = np.asarray(CASES[N])
    cell = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    assert len(cell) == N
    return acc, *csr(cell, len(sizes))


def csr(cell, G):
    start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=G))]).astype(np.int32)
    return start, np.argsort(cell, kind="stable").astype(np.int32)


def terms(acc):
    """go2nn_eval_reduce's term of every env and column, float64 [COLS, N]"""
    N = acc.shape[1]
    return np.concatenate([acc.astype(np.float64), np.ones((1, N)), (acc[FALLS] == 0).astype(np.float64)[None]])


def restatement(acc, start, envs, B, seed):
    """the rule of include/go2nn.h: draw k of (b, g) is member (x n) >> 32 with x = word (k & 3) of philox4x32_10((b, g, k >> 2, 0), (seed, 7)), in Python integers; the
    twelve sums in float64, one add per draw in the draws' order -> [B, G, COLS]"""
    t, G = terms(acc), len(start) - 1
    out = np.zeros((B, G, COLS))
    for b in range(B):
        for g in range(G):
            s0, n = int(start[g]), int(start[g + 1] - start[g])
            s = np.zeros(COLS)
            for k in range(n):
                if k % 4 == 0:
                    w = philox_int((b, g, k >> 2, 0), (seed, TAG))
                s = s + t[:, envs[s0 + ((w[k & 3] * n) >> 32)]]
            out[b, g] = s
    return out


@functools.lru_cache(maxsize=None)
def reference(N, seed=2718):
    """the case at `N` and its restatement at the largest B (a replicate does not depend on B: smaller calls are compared with its first rows) -> shared, never written"""
    acc, start, envs = case(N)
    ref = restatement(acc, start, envs, max(BS), seed)
    for a in (acc, start, envs, ref):
        a.setflags(write=False)
    return acc, start, envs, ref


def host_call(emu):
    def call(acc, start, envs, B, seed):
        out = np.full((B, len(start) - 1, COLS), -7.0)
        rc = emu.go2nn_eval_bootstrap(p(acc), p(start), p(envs), acc.shape[1], len(start) - 1, B, seed, p(out), None)
        assert rc == 0, emu.go2nn_last_error()
        return out
    return call


def check_kernel_case(call, N, B):
    """call(acc, start, envs, B, seed) -> [B, G, COLS] of a library: the restatement's bits, the cells' sizes in the count column, zeros for the empty cell"""
    acc, start, envs, ref = reference(N)
    out = call(acc, start, envs, B, 2718)
    assert out.shape == ref[:B].shape and out.tobytes() == ref[:B].tobytes(), np.abs(out - ref[:B]).max()
    sizes = np.diff(start)
    assert (out[:, :, GO2NN_EVAL_NUM] == sizes[None]).all() and (out[:, :, 0] == 50.0 * sizes[None]).all()
    for g in np.nonzero(sizes == 0)[0]:
        assert not out[:, g].any()
    assert np.isfinite(out).all() and (out[:, sizes > 0, GO2NN_EVAL_NUM + 1] <= sizes[sizes > 0]).all()
    assert B < 255 or np.abs(out).max() > 1e37          # the large magnitudes are drawn


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", sorted(CASES))
def test_kernel_equals_the_restatement_bit_for_bit(emu, N, B):
    check_kernel_case(host_call(emu), N, B)


def check_prefix_and_seed(call):
    acc, start, envs, _ = reference(300)
    big, small = call(acc, start, envs, 256, 5), call(acc, start, envs, 64, 5)
    assert big[:64].tobytes() == small.tobytes()
    other = call(acc, start, envs, 64, 6)
    assert other.tobytes() != small.tobytes() and (other[:, :, GO2NN_EVAL_NUM] == small[:, :, GO2NN_EVAL_NUM]).all()
    # replicates differ from each other, and each differs from the plain reduce row (a cell of 293 redrawn 293 times is not itself)
    assert len({big[b, 2].tobytes() for b in range(256)}) == 256


def test_prefix_property_and_seed(emu):
    check_prefix_and_seed(host_call(emu))


def check_constant_cell(call, reduce):
    """a cell whose robots all hold the same small-integer rows: whichever members are drawn, every replicate is go2nn_eval_reduce's row of the cell (exact sums)"""
    N, rng = 90, np.random.default_rng(4)
    cell = (np.arange(N) % 3).astype(np.int32)
    acc = rng.integers(-50, 50, (GO2NN_EVAL_NUM, N)).astype(np.float32)
    acc[:, cell == 1] = np.asarray([50, 3, 0, -7, 2, 11, 40, 5, 1, 2], np.float32)[:, None]
    start, envs = csr(cell, 3)
    out, red = call(acc, start, envs, 33, 9), reduce(acc, cell, 3)
    assert (out[:, 1] == red[1][None]).all() and red[1, GO2NN_EVAL_NUM] == 30 and red[1, GO2NN_EVAL_NUM + 1] == 0
    assert (out[:, 0] != red[0][None]).any()


def test_constant_cell_gives_the_reduce_row(emu):
    def reduce(acc, cell, G):
        out = np.zeros((G, COLS))
        assert emu.go2nn_eval_reduce(p(acc), p(cell), acc.shape[1], G, p(out), None) == 0
        return out
    check_constant_cell(host_call(emu), reduce)


def refusal_cases(N, G, B):
    """(what, the arguments' overrides) of every GO2NN_EINVAL case of go2nn_eval_bootstrap"""
    return [("acc", dict(acc=None)), ("cell_start", dict(start=None)), ("cell_envs", dict(envs=None)), ("out", dict(out=None)), ("N = 0", dict(N=0)), ("G = 0", dict(G=0)),
            ("G = 65536", dict(G=65536)), ("B = 0", dict(B=0)), ("B > 2^20", dict(B=(1 << 20) + 1)), ("B G 12 >= 2^31", dict(B=1 << 20, G=171))]


def test_refusals(emu):
    acc, start, envs, _ = reference(37)
    N, G = 37, len(start) - 1
    out = np.full((4, G, COLS), -3.0)
    base = dict(acc=p(acc), start=p(start), envs=p(envs), N=N, G=G, B=4, out=p(out))
    for what, over in refusal_cases(N, G, 4):
        a = dict(base, **over)
        rc = emu.go2nn_eval_bootstrap(a["acc"], a["start"], a["envs"], a["N"], a["G"], a["B"], 1, a["out"], None)
        assert rc == EINVAL and emu.go2nn_last_error() and (out == -3.0).all(), what
    assert (1 << 20) * 171 * COLS >= 2 ** 31 > (1 << 20) * 170 * COLS
    check = lambda s, e, n=N, g=G: emu.go2nn_eval_bootstrap_check(p(s) if s is not None else None, p(e) if e is not None else None, n, g)
    assert check(start, envs) == 0
    for s, e, n, g in ((None, envs, N, G), (start, None, N, G), (start, envs, 0, G), (start, envs, N, 0), (start, envs, N, 65536)):
        assert check(s, e, n, g) == EINVAL
    bad = start.copy(); bad[0] = 1
    assert check(bad, envs) == EINVAL and b"starts at 0" in emu.go2nn_last_error()
    bad = start.copy(); bad[2] = bad[1] - 1
    assert check(bad, envs) == EINVAL and b"below" in emu.go2nn_last_error()
    bad = start.copy(); bad[G] = N + 1
    assert check(bad, np.concatenate([envs, [0]]).astype(np.int32)) == EINVAL and b"more than" in emu.go2nn_last_error()
    for v in (-1, N):
        bad = envs.copy(); bad[5] = v
        assert check(start, bad) == EINVAL and b"outside" in emu.go2nn_last_error()
        # the host build looks at the list in the launch call too (host memory), and writes nothing
        assert emu.go2nn_eval_bootstrap(p(acc), p(start), p(bad), N, G, 4, 1, p(out), None) == EINVAL and (out == -3.0).all()
    assert check(start[:2].copy(), envs, N, 1) == 0          # cell_start[G] < N: envs that belong to no cell are allowed


def check_statistics(call):
    """one cell of 64 lognormal values, 4096 replicates: the standard deviation of the replicate means against the closed form std(x, ddof=0) / sqrt(n) of drawing n of n
    with replacement.  10 %: the estimate from 4096 replicates has a relative error of about 1 / sqrt(2 * 4096) = 1.1 % (a numpy trial of the same rule over 20 seeds stayed
    within 3.1 %), while a wrong index rule — always member 0, or n - 1 members — moves the ratio by far more"""
    n, B = 64, 4096
    x = np.random.default_rng(123).lognormal(0.0, 1.0, n).astype(np.float32)
    acc = np.zeros((GO2NN_EVAL_NUM, n), np.float32)
    acc[0], acc[1] = 1.0, x
    start, envs = np.asarray([0, n], np.int32), np.arange(n, dtype=np.int32)
    out = call(acc, start, envs, B, 2718)
    means = out[:, 0, 1] / out[:, 0, 0]
    got, want = means.std(), x.astype(np.float64).std() / np.sqrt(n)
    print("bootstrap std of the mean %.5f, closed form %.5f, ratio %.4f; mean of the means %.5f, sample mean %.5f" % (got, want, got / want, means.mean(), x.mean()))
    assert abs(got / want - 1.0) <= 0.10
    assert abs(means.mean() - x.astype(np.float64).mean()) <= 4.0 * want / np.sqrt(B) * 1.10          # the replicate means centre on the sample mean (4 sigma of their mean)


def test_statistics_of_the_replicates(emu):
    check_statistics(host_call(emu))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
SENSORS = [["nominal", {}], ["noise_3.0", {"noise": 3.0}], ["delay_2", {"delay": 2}]]


def leaves(res):
    """every leaf dict _row() made, with its path"""
    out = [("overall", res["overall"])] + [("groups/%s/%s" % (t, s), d) for t, per in res["groups"].items() for s, d in per.items()]
    out += [("%s/%s" % (k, n), d) for k in ("perturbations", "sensors", "maneuvers") for n, d in (res.get(k) or {}).items()]
    out += [("cells/%s/%s/%s" % (t, s, n), d) for t, per in (res.get("cells") or {}).items() for s, cs in per.items() for n, d in cs.items()]
    return out


def same_value(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def without_ci(v):
    return {k: without_ci(x) for k, x in v.items() if k != "ci"} if isinstance(v, dict) else v


def check_on_against_off(ev_on, on, off, acc_host):
    """on / off: the results of the same weights with and without `evaluation.bootstrap`;  acc_host: the option-on evaluator's accumulators on the host"""
    from go2_rl_gym_amd.utils.evaluator import CI_KEYS, replicate_metrics, interval
    assert "bootstrap" not in off and not any("ci" in d for _, d in leaves(off))
    assert set(on) == set(off) | {"bootstrap"}
    for k in off:
        assert same_value(without_ci(on[k]), off[k]), k
    bs = on["bootstrap"]
    B, cells = ev_on.bootstrap, ev_on.num_cells
    assert bs["replicates"] == B and bs["seed"] == ev_on.bootstrap_seed and bs["confidence"] == ev_on.confidence and bs["table"].shape == (B, cells, COLS)
    start, envs = csr(ev_on.cell_host.astype(np.int32), cells)
    assert (start == ev_on.cell_start_host).all() and (envs == ev_on.cell_envs_host).all()
    assert bs["table"].tobytes() == restatement(acc_host, start, envs, B, bs["seed"]).tobytes()
    # the overall row of a replicate is the sum of its cells' rows: whole numbers exactly, the sums to the rounding of a handful of fp64 adds
    total = bs["table"].sum(1)
    assert bs["overall"].shape == (B, COLS) and (bs["overall"][:, [0, FALLS, GO2NN_EVAL_NUM, GO2NN_EVAL_NUM + 1]] == total[:, [0, FALLS, GO2NN_EVAL_NUM, GO2NN_EVAL_NUM + 1]]).all()
    assert (bs["overall"][:, GO2NN_EVAL_NUM] == ev_on.num_envs).all() and (np.abs(bs["overall"] - total) <= cells * 2.0 ** -52 * np.abs(bs["table"]).sum(1)).all()
    reps = replicate_metrics(bs["overall"])
    for path, d in leaves(on):
        assert set(d["ci"]) == set(CI_KEYS), path
        for m, (lo, hi) in d["ci"].items():
            assert lo <= hi or (np.isnan(lo) and np.isnan(hi)), (path, m)
    for m in CI_KEYS:
        assert on["overall"]["ci"][m] == interval(reps[m], bs["confidence"])
        # a replicate figure is _row() of the replicate row
        assert reps[m][3] == ev_on._row(bs["overall"][3])[m]
    lo, hi = on["overall"]["ci"]["lin_vel_err"]
    assert lo < on["overall"]["lin_vel_err"] < hi and hi - lo > 0


@pytest.mark.parametrize("axis", ["plain", "sensors"])
def test_evaluator_option_off_and_on(emu, axis):
    from go2_rl_gym_amd.utils.evaluator import CI_KEYS, format_table, results_dict, scalars
    over = dict(sensors=SENSORS) if axis == "sensors" else {}
    ac = small_actor_critic()
    ev_plain = make_evaluator(emu, **over)                                                                   # an evaluator built without the keys
    ev_off = make_evaluator(emu, bootstrap=0, bootstrap_seed=5, confidence=0.9, bootstrap_max_bytes=1, **over)
    ev_on = make_evaluator(emu, bootstrap=48, confidence=0.9, **over)
    plain, off, on = ev_plain.evaluate(ac), ev_off.evaluate(ac), ev_on.evaluate(ac)
    assert not hasattr(ev_off, "boot_out") and not hasattr(ev_off, "cell_start") and ev_off.bootstrap == 0
    assert same_value(off, plain) and results_dict(off, 3) == results_dict(plain, 3) and format_table(off) == format_table(plain)
    assert [(t, np.float64(v).tobytes()) for t, v in scalars(off)] == [(t, np.float64(v).tobytes()) for t, v in scalars(plain)]
    assert ev_on.num_cells == (4 * len(SENSORS) if axis == "sensors" else 4)
    check_on_against_off(ev_on, on, off, ev_on.acc.numpy().copy())
    # the yaml, the scalars and the table carry the intervals
    d = yaml.safe_load(yaml.safe_dump(results_dict(on, 3)))
    assert d["bootstrap"] == {"replicates": 48, "seed": 2718, "confidence": 0.9} and set(d["overall"]["ci"]) == set(CI_KEYS)
    assert d["groups"]["plane"]["stand"]["ci"]["tilt"] == on["groups"]["plane"]["stand"]["ci"]["tilt"]
    assert without_ci({k: v for k, v in d.items() if k != "bootstrap"}) == yaml.safe_load(yaml.safe_dump(results_dict(off, 3)))
    tags = dict(scalars(on))
    assert set(tags) - set(dict(scalars(off))) == {"Eval/ci_%s/%s" % (side, m) for side in ("low", "high") for m in CI_KEYS}
    assert [tags["Eval/ci_low/tilt"], tags["Eval/ci_high/tilt"]] == on["overall"]["ci"]["tilt"]
    text = format_table(on)
    assert text.startswith(format_table(off)) and "90 % interval, 48 replicates" in text[len(format_table(off)):]
    assert "%.4f [%.4f, %.4f]" % ((on["overall"]["tilt"],) + tuple(on["overall"]["ci"]["tilt"])) in text
    # the same weights again: the same replicates
    assert ev_on.evaluate(ac)["bootstrap"]["table"].tobytes() == on["bootstrap"]["table"].tobytes()
    for e in (ev_plain, ev_off, ev_on):
        e.close()


def test_evaluator_refuses_what_it_cannot_hold(emu):
    with pytest.raises(ValueError, match="bootstrap_max_bytes"):
        make_evaluator(emu, bootstrap=48, bootstrap_max_bytes=48 * 4 * COLS * 8 - 1)
    make_evaluator(emu, bootstrap=48, bootstrap_max_bytes=48 * 4 * COLS * 8).close()
    with pytest.raises(ValueError, match="bootstrap"):
        make_evaluator(emu, bootstrap=-1)
    with pytest.raises(ValueError, match="confidence"):
        make_evaluator(emu, bootstrap=8, confidence=1.0)


def test_compare_is_paired(emu):
    from go2_rl_gym_amd.utils.evaluator import compare, interval, replicate_metrics
    # two evaluations of the same weights: every difference exactly 0, tied
    ev = make_evaluator(emu, bootstrap=32)
    ac = small_actor_critic()
    a, b = (replicate_metrics(ev.evaluate(ac)["bootstrap"]["overall"]) for _ in range(2))
    ev.close()
    for m in a:
        assert (a[m] - b[m] == 0).all()
        assert compare(a[m], b[m], 0.95) == {"diff_ci": [0.0, 0.0], "tied": True}
    # a and a + 0.01 with std(a) = 0.1: the marginal intervals overlap almost entirely, the paired interval has no width at 0.01 and excludes 0
    x = np.random.default_rng(0).normal(0.0, 1.0, 1000)
    x = 0.5 + 0.1 * (x - x.mean()) / x.std()
    y = x + 0.01
    c = compare(y, x, 0.95)
    (alo, ahi), (blo, bhi) = interval(x, 0.95), interval(y, 0.95)
    assert blo < ahi and alo < bhi and ahi - alo > 0.3                 # overlapping marginals
    assert c["tied"] is False and abs(c["diff_ci"][0] - 0.01) < 1e-12 and c["diff_ci"][1] - c["diff_ci"][0] < 1e-12
    assert compare(x, y, 0.95)["diff_ci"][1] < 0 and compare(x, x, 0.95)["tied"] is True
    nan = np.full(8, np.nan)
    assert compare(nan, nan)["tied"] is False and all(np.isnan(compare(nan, nan)["diff_ci"]))
    with pytest.raises(ValueError):
        compare(x, x[:5])


def test_cli_flag(tmp_path):
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    base = ["--task", "go2_flat", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"]
    for argv, want in (([], 0), (["--ci"], 1000), (["--ci", "200"], 200)):
        args = get_args(base + argv)
        _, train_cfg = update_cfg_from_args(None, copy.deepcopy(task_registry.train_cfgs["go2_flat"]), args)
        assert train_cfg.evaluation.bootstrap == want and (args.ci is None) == (want == 0)
    e = task_registry.train_cfgs["go2_flat"].evaluation
    assert (e.bootstrap, e.bootstrap_seed, e.confidence, e.bootstrap_max_bytes) == (0, 2718, 0.95, 256 << 20)
    with pytest.raises(ValueError, match="push_falls"):          # refused before anything is loaded
        evaluate(base + ["--robust", "--ci", "--metric", "push_falls"], log_root=str(tmp_path))


def test_cli_compares_every_checkpoint_with_the_best(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints with and without --ci 64"""
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import CI_KEYS
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s = 24, 0.2, 0.1
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    base = ["--task", "go2_flat", "--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    run_dir = runner.log_dir
    env.close()
    kw = dict(log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    plain = evaluate(base + ["--all_checkpoints", "--metric", "tilt"], **kw)
    assert set(plain) == {"task", "metric", "best", "best_value", "checkpoints"} and not os.path.exists(os.path.join(run_dir, "eval_results", "comparison_tilt.yaml"))
    assert all("ci" not in r["overall"] for r in plain["checkpoints"])
    capsys.readouterr()
    out = evaluate(base + ["--all_checkpoints", "--metric", "tilt", "--ci", "64"], **kw)
    assert set(out) == set(plain) | {"comparison", "tied_with_best"} and (out["best"], out["best_value"]) == (plain["best"], plain["best_value"])
    comp = out["comparison"]
    assert (comp["metric"], comp["confidence"], comp["replicates"]) == ("tilt", 0.95, 64) and [r["checkpoint"] for r in comp["rows"]] == ["model_0.pt", "model_1.pt"]
    for r, row in zip(comp["rows"], out["checkpoints"]):
        assert set(r) == {"checkpoint", "value", "ci", "diff_to_best", "diff_ci", "tied_with_best"}
        assert r["value"] == row["overall"]["tilt"] and r["ci"] == row["overall"]["ci"]["tilt"] and set(row["overall"]["ci"]) == set(CI_KEYS)
        assert r["diff_to_best"] == r["value"] - out["best_value"] >= 0 and r["diff_ci"][0] <= r["diff_ci"][1]
        assert r["tied_with_best"] == (r["diff_ci"][0] <= 0 <= r["diff_ci"][1]) and (r["checkpoint"] in out["tied_with_best"]) == r["tied_with_best"]
        if r["checkpoint"] == out["best"]:
            assert r["diff_to_best"] == 0 and r["diff_ci"] == [0.0, 0.0] and r["tied_with_best"]
    text = capsys.readouterr().out
    line = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
    assert line["tied_with_best"] == out["tied_with_best"] and line["comparison"]["rows"][1]["diff_ci"] == comp["rows"][1]["diff_ci"]
    assert "paired interval" in text and "64 replicates" in text
    d = yaml.safe_load(open(os.path.join(run_dir, "eval_results", "comparison_tilt.yaml")))
    assert d["best"] == out["best"] and d["tied_with_best"] == out["tied_with_best"] and d["comparison"]["rows"][0]["ci"] == comp["rows"][0]["ci"]
