"""The bootstrap of the modes' and add-ons' figures (`evaluation.bootstrap_all`) on the CPU: the host build of go2nn_{robust,maneuver,ladder,gait,asym}_bootstrap
(include/go2nn.h) against the draws restated in Python integers and the fp64 sum of the library's OWN per-robot terms (its reduce with singleton groups: a singleton's fixed
tree adds zeros, so the term is exact) — bit for bit —, the refusals, the code object's resources, PolicyEvaluator with the key off and on, and the CLI.
tests/test_gpu_bootstrap_modes.py runs the same cases on the device."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import yaml

from helpers import load_nn_emu, load_oracle
import test_bootstrap_host as tb
from test_eval_host import make_evaluator, small_actor_critic
from test_sensor_host import philox_int
from go2_rl_gym_amd import _nn

EINVAL = -22
DIST2_THR = 2.25
SEED = 2718


class Family:
    """one scoring family: its table's rows, its reduce's width, where its count column is, which rows hold whole numbers, its max column"""
    def __init__(self, name, rows, cols, n_col, whole, max_col=-1, extra=()):
        self.name, self.rows, self.cols, self.n_col, self.whole, self.max_col, self.extra = name, tuple(rows), cols, n_col, tuple(whole), max_col, tuple(extra)

    def args(self, table, start, envs, N, G, B, seed, out, stream=None):
        """the argument list of go2nn_<family>_bootstrap (the ladder's has dist2_thr before the output)"""
        return [table, start, envs, N, G, B, seed] + list(self.extra) + [out, stream]


GAIT_ROWS = _nn.GAIT_ENV_ROWS + tuple("%s/%d" % (r, f) for f in range(4) for r in _nn.GAIT_FOOT_ROWS)
GAIT_WHOLE = tuple(r for r in GAIT_ROWS if r.split("/")[0] in ("used", "support0", "support1", "support2", "support3", "support4", "diagonal", "contact", "touchdowns",
                                                               "stride_steps", "strides", "stance_steps", "stances", "swing_steps", "swings"))
FAMILIES = {f.name: f for f in (
    Family("robust", _nn.ROBUST_ROWS, _nn.GO2NN_ROBUST_ACC_NUM + 1, _nn.GO2NN_ROBUST_ACC_NUM, ("pushes", "push_falls", "recovered", "recovery_steps")),
    Family("maneuver", _nn.MANEUVER_ROWS, _nn.GO2NN_MANEUVER_ACC_NUM + 1, _nn.GO2NN_MANEUVER_ACC_NUM, ("switches", "switch_falls", "settled", "settle_steps", "win_steps")),
    Family("ladder", _nn.LADDER_ROWS, _nn.GO2NN_LADDER_OUT_NUM, 0, ("clear_step",), extra=(C.c_float(DIST2_THR),)),
    Family("gait", GAIT_ROWS, _nn.GO2NN_GAIT_OUT_NUM, 0, GAIT_WHOLE),
    Family("asym", _nn.ASYM_ROWS, _nn.GO2NN_ASYM_OUT_NUM, 0, ("eq_steps", "sym_steps", "contact_l", "contact_r"), max_col=_nn.ASYM_OUT.index("eq_max")))}
assert len(GAIT_ROWS) == _nn.GO2NN_GAIT_NUM and FAMILIES["gait"].cols == 55 and FAMILIES["asym"].cols == 25


def make_table(fam, N, seed=11):
    """fp32 [rows, N]: both signs over many decades with exact zeros and two huge entries; whole numbers in the rows that are counts; the ladder's states from their enum;
    asym pairs with L + R = 0 (both zero, and L = -R)"""
    rng = np.random.default_rng(seed + 1000 * sorted(FAMILIES).index(fam.name) + N)
    R = len(fam.rows)
    t = (rng.normal(0, 1, (R, N)) * np.exp(rng.normal(0, 6, (R, N)))).astype(np.float32)
    t[rng.random(t.shape) < 0.1] = 0.0
    for r in fam.whole:
        t[fam.rows.index(r)] = (rng.random(N) < 0.7) * rng.integers(1, 40, N)
    if fam.name == "ladder":
        t[fam.rows.index("state")] = rng.integers(0, len(_nn.LADDER_STATES), N)
    if fam.name == "asym":
        for p in _nn.ASYM_PAIRS:
            l, r = fam.rows.index(p + "_l"), fam.rows.index(p + "_r")
            t[l, 1::7], t[r, 1::7] = 0.0, 0.0
            t[r, 2::7] = -t[l, 2::7]
    big = {"robust": ("peak_err_sum", "peak_tilt_sum"), "maneuver": ("win_lin_err", "peak_tilt_sum"), "ladder": ("clear_step", "max_d2"), "gait": ("slip_sum/0", "height_sum/3"),
           "asym": ("eq_sq", "act_sq")}[fam.name]
    t[fam.rows.index(big[0]), 0], t[fam.rows.index(big[1]), N - 1] = 3.0e37, -3.0e37          # two huge entries in rows the reduce reads
    if fam.name == "ladder":
        t[fam.rows.index("state"), 0] = _nn.LADDER_STATES.index("cleared")
    return t


class HostBackend:
    """how the checks below reach a library: numpy arrays in host memory"""
    name = "host"

    def __init__(self, lib):
        self.lib = lib

    up = staticmethod(lambda a: np.ascontiguousarray(a).copy())
    ptr = staticmethod(lambda a: None if a is None else C.c_void_p(a.ctypes.data))
    down = staticmethod(lambda a: a)
    stream = staticmethod(lambda: None)
    full = staticmethod(lambda shape, v: np.full(shape, v, np.float64))


def bootstrap(be, fam, table, start, envs, B, seed):
    """go2nn_<family>_bootstrap of the backend's library -> float64 [B, G, cols]"""
    G = len(start) - 1
    t, s, e, out = be.up(table), be.up(start), be.up(envs), be.full((B, G, fam.cols), -7.0)
    assert be.lib.go2nn_eval_bootstrap_check(tb.p(start), tb.p(envs), table.shape[1], G) == 0, be.lib.go2nn_last_error()
    rc = getattr(be.lib, "go2nn_%s_bootstrap" % fam.name)(*fam.args(be.ptr(t), be.ptr(s), be.ptr(e), table.shape[1], G, B, seed, be.ptr(out), be.stream()))
    assert rc == 0, be.lib.go2nn_last_error()
    return np.array(be.down(out))


def reduce(be, fam, table, group, G):
    """go2nn_<family>_reduce of the backend's library -> float64 [G, cols]"""
    t, g, out = be.up(table), be.up(np.asarray(group, np.int32)), be.full((G, fam.cols), -7.0)
    rc = getattr(be.lib, "go2nn_%s_reduce" % fam.name)(be.ptr(t), be.ptr(g), table.shape[1], G, *fam.extra, be.ptr(out), be.stream())
    assert rc == 0, be.lib.go2nn_last_error()
    return np.array(be.down(out))


def own_terms(be, fam, table):
    """the library's own term of every robot and column: its reduce with singleton groups -> float64 [N, cols]"""
    N = table.shape[1]
    return reduce(be, fam, table, np.arange(N), N)


@functools.lru_cache(maxsize=None)
def draws(N, seed=SEED, B=max(tb.BS), sizes=None):
    """the rule of include/go2nn.h in Python integers, once per case and shared by every family: -> (cell_start, cell_envs, [per cell: int [B, n] env of draw k of replicate b])"""
    sizes = np.asarray(tb.CASES[N] if sizes is None else sizes)
    cell = np.random.default_rng(seed + N).permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    start, envs = tb.csr(cell, len(sizes))
    return (start, envs) + (drawn(start, envs, B, seed),)


def drawn(start, envs, B, seed):
    per_cell = []
    for g in range(len(start) - 1):
        s0, n = int(start[g]), int(start[g + 1] - start[g])
        idx = np.zeros((B, n), np.int64)
        for b in range(B):
            for k in range(n):
                if k % 4 == 0:
                    w = philox_int((b, g, k >> 2, 0), (seed, tb.TAG))
                idx[b, k] = envs[s0 + ((w[k & 3] * n) >> 32)]
        idx.setflags(write=False)
        per_cell.append(idx)
    for a in (start, envs):
        a.setflags(write=False)
    return per_cell


def restate(terms, per_cell, max_col=-1):
    """terms float64 [N, cols], the draws -> [B, G, cols]: one fp64 add per draw in the draws' order (the max column: the max, from 0)"""
    B, cols = per_cell[0].shape[0], terms.shape[1]
    out = np.zeros((B, len(per_cell), cols))
    for g, idx in enumerate(per_cell):
        s = np.zeros((B, cols))
        for k in range(idx.shape[1]):
            v = terms[idx[:, k]]
            nxt = s + v
            if max_col >= 0:
                nxt[:, max_col] = np.fmax(s[:, max_col], v[:, max_col])
            s = nxt
        out[:, g] = s
    return out


_REF = {}


def reference(be, fam, N):
    """the family's table at `N` and the restatement at the largest B, from the backend's own terms -> shared, never written"""
    key = (be.name, fam.name, N)
    if key not in _REF:
        table = make_table(fam, N)
        start, envs, per_cell = draws(N)
        ref = restate(own_terms(be, fam, table), per_cell, fam.max_col)
        for a in (table, ref):
            a.setflags(write=False)
        _REF[key] = (table, start, envs, ref)
    return _REF[key]


def check_kernel_case(be, fam, N, B):
    """the restatement's bits; the cells' sizes in the count column (common draws); zeros for the empty cell"""
    table, start, envs, ref = reference(be, fam, N)
    out = bootstrap(be, fam, table, start, envs, B, SEED)
    assert out.shape == ref[:B].shape and out.tobytes() == ref[:B].tobytes(), (fam.name, np.nanmax(np.abs(out - ref[:B])))
    sizes = np.diff(start)
    assert (out[:, :, fam.n_col] == sizes[None]).all()
    for g in np.nonzero(sizes == 0)[0]:
        assert not out[:, g].any()
    assert B < 255 or np.nanmax(np.abs(out)) > 1e37          # the large magnitudes are drawn


def check_same_robots(be, fam, N=300):
    """every row of the table holds the env index (the ladder: every robot CLEARED, so that CLEAR_STEPS is the index): every summed column of every column window is the sum
    of cell_envs over the restated draws — a window that drew differently shows"""
    start, envs, per_cell = draws(N)
    table = np.tile(np.arange(N, dtype=np.float32), (len(fam.rows), 1))
    if fam.name == "ladder":
        table[fam.rows.index("state")] = _nn.LADDER_STATES.index("cleared")
    B = 33
    out = bootstrap(be, fam, table, start, envs, B, SEED)
    want = np.stack([idx[:B].sum(1) for idx in per_cell], 1).astype(np.float64)          # [B, G] (whole numbers below 2^53: any order)
    index_cols = {"robust": range(fam.cols - 1), "maneuver": range(fam.cols - 1), "ladder": [_nn.LADDER_OUT.index("clear_steps")], "gait": range(1, fam.cols),
                  "asym": [c for c in range(1, _nn.GO2NN_ASYM_OUT_IMB0) if c != fam.max_col]}[fam.name]
    for c in index_cols:
        assert (out[:, :, c] == want).all(), (fam.name, c)
    assert len(index_cols) >= fam.cols - 10 or fam.name == "ladder"
    if fam.max_col >= 0:
        assert (out[:, :, fam.max_col] == np.stack([idx[:B].max(1) for idx in per_cell], 1)).all()
        imb = out[:, :, _nn.GO2NN_ASYM_OUT_IMB0:].reshape(B, len(per_cell), 4, 2)          # L = R = e: no imbalance, and a pair unless e = 0
        has = np.stack([(idx[:B] > 0).sum(1) for idx in per_cell], 1)
        assert not imb[..., 0].any() and (imb[..., 1] == has[:, :, None]).all()
    assert (out[:, :, fam.n_col] == np.diff(start)[None]).all()


def check_prefix_and_seed(be, fam):
    table, start, envs, _ = reference(be, fam, 300)
    big, small = bootstrap(be, fam, table, start, envs, 256, 5), bootstrap(be, fam, table, start, envs, 64, 5)
    assert big[:64].tobytes() == small.tobytes()
    other = bootstrap(be, fam, table, start, envs, 64, 6)
    assert other.tobytes() != small.tobytes() and (other[:, :, fam.n_col] == small[:, :, fam.n_col]).all()
    assert len({big[b, 2].tobytes() for b in range(256)}) == 256


def check_constant_cell(be, fam):
    """a cell whose robots all hold the same small-integer rows: every replicate is the family's reduce row of the cell, whichever members are drawn (exact sums; the
    ladder's progress is sqrt(0.5625 / 2.25) = 0.5, the asym imbalances |3 - 1| / 4 = 0.5)"""
    N, rng = 90, np.random.default_rng(4)
    cell = (np.arange(N) % 3).astype(np.int32)
    table = rng.integers(0, 50, (len(fam.rows), N)).astype(np.float32)
    const = (np.arange(len(fam.rows)) % 7 + 1).astype(np.float32)
    if fam.name == "ladder":
        table[fam.rows.index("state")] = rng.integers(0, 4, N)
        const[fam.rows.index("state")], const[fam.rows.index("max_d2")] = _nn.LADDER_STATES.index("cleared"), 0.5625
    if fam.name == "asym":
        for pr in _nn.ASYM_PAIRS:
            const[fam.rows.index(pr + "_l")], const[fam.rows.index(pr + "_r")] = 3.0, 1.0
    table[:, cell == 1] = const[:, None]
    start, envs = tb.csr(cell, 3)
    out, red = bootstrap(be, fam, table, start, envs, 33, 9), reduce(be, fam, table, cell, 3)
    assert (out[:, 1] == red[1][None]).all() and red[1, fam.n_col] == 30 and np.abs(red[1]).sum() > 30
    assert (out[:, 0] != red[0][None]).any()


def refusal_cases(fam):
    G_big = -(-(1 << 11) // fam.cols)          # the smallest G with 2^20 G cols >= 2^31
    assert (1 << 20) * G_big * fam.cols >= 2 ** 31 > (1 << 20) * (G_big - 1) * fam.cols
    cases = [("table", dict(table=None)), ("cell_start", dict(start=None)), ("cell_envs", dict(envs=None)), ("out", dict(out=None)), ("N = 0", dict(N=0)), ("G = 0", dict(G=0)),
             ("G = 65536", dict(G=65536)), ("B = 0", dict(B=0)), ("B > 2^20", dict(B=(1 << 20) + 1)), ("B G cols >= 2^31", dict(B=1 << 20, G=G_big))]
    if fam.name == "ladder":
        cases += [("dist2_thr = 0", dict(thr=0.0)), ("dist2_thr < 0", dict(thr=-1.0)), ("dist2_thr NaN", dict(thr=float("nan")))]
    return cases


def check_refusals(be, fam, sync=lambda: None):
    """every GO2NN_EINVAL case, with the output buffer left untouched"""
    table, start, envs, _ = reference(be, fam, 37)
    N, G = 37, len(start) - 1
    t, s, e, out = be.up(table), be.up(start), be.up(envs), be.full((4, G, fam.cols), -3.0)
    base = dict(table=be.ptr(t), start=be.ptr(s), envs=be.ptr(e), N=N, G=G, B=4, out=be.ptr(out), thr=DIST2_THR)
    fn = getattr(be.lib, "go2nn_%s_bootstrap" % fam.name)
    for what, over in refusal_cases(fam):
        a = dict(base, **over)
        extra = [C.c_float(a["thr"])] if fam.name == "ladder" else []
        rc = fn(*([a["table"], a["start"], a["envs"], a["N"], a["G"], a["B"], 1] + extra + [a["out"], be.stream()]))
        assert rc == EINVAL and be.lib.go2nn_last_error(), (fam.name, what)
    sync()
    assert (np.array(be.down(out)) == -3.0).all()
    return t, s, e, out


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.fixture(scope="module")
def host(emu):
    return HostBackend(emu)


FAMS = sorted(FAMILIES)


@pytest.mark.parametrize("B", tb.BS)
@pytest.mark.parametrize("N", sorted(tb.CASES))
@pytest.mark.parametrize("fam", FAMS)
def test_kernel_equals_the_restatement_bit_for_bit(host, fam, N, B):
    check_kernel_case(host, FAMILIES[fam], N, B)


def test_the_shared_draws_are_those_of_the_eval_bootstrap(emu):
    """the draw indices every family's restatement uses, checked against test_bootstrap_host's own restatement through go2nn_eval_bootstrap: a table whose first row is the
    env index"""
    start, envs, per_cell = draws(37)
    acc = np.zeros((_nn.GO2NN_EVAL_NUM, 37), np.float32)
    acc[0] = np.arange(37)
    out = tb.host_call(emu)(acc, start, envs, 64, SEED)
    assert (out[:, :, 0] == np.stack([idx[:64].sum(1) for idx in per_cell], 1)).all()
    assert out.tobytes() == tb.restatement(acc, start, envs, 64, SEED).tobytes()


@pytest.mark.parametrize("fam", FAMS)
def test_same_robots_in_every_family_and_column_window(host, fam):
    check_same_robots(host, FAMILIES[fam])


@pytest.mark.parametrize("fam", FAMS)
def test_prefix_seed_and_constant_cell(host, fam):
    check_prefix_and_seed(host, FAMILIES[fam])
    check_constant_cell(host, FAMILIES[fam])


@pytest.mark.parametrize("fam", FAMS)
def test_refusals(host, fam):
    f = FAMILIES[fam]
    t, s, e, out = check_refusals(host, f)
    _, start, envs, _ = reference(host, f, 37)
    for v in (-1, 37):          # the host build looks at the list in the launch call too (host memory), and writes nothing
        bad = envs.copy(); bad[5] = v
        rc = getattr(host.lib, "go2nn_%s_bootstrap" % fam)(*f.args(host.ptr(t), host.ptr(s), tb.p(bad), 37, len(start) - 1, 4, 1, host.ptr(out)))
        assert rc == EINVAL and b"outside" in host.lib.go2nn_last_error() and (out == -3.0).all()


@pytest.mark.parametrize("fam", FAMS + ["eval"])
def test_no_instantiation_has_scratch(fam):
    """the gfx950 code object of the built library: every bootstrap instantiation keeps its window's sums in registers (no scratch), and uses no LDS"""
    from go2_rl_gym_amd import build
    cols = tb.COLS if fam == "eval" else FAMILIES[fam].cols
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(build.NN_OUT) and os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("no built device library, or no LLVM tools to read its code object")
    res = build.kernel_resources(build.NN_OUT, match="eval_bootstrap_kernelILi%dELi" % cols)
    print(fam, res)
    assert res is not None, "the library has no bootstrap kernel of %d columns" % cols
    assert res["scratch_bytes_per_lane"] == 0 and res["lds_bytes_per_workgroup"] == 0 and res["vgpr_count"] <= 128


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# PolicyEvaluator with `evaluation.bootstrap_all`: one evaluation per mode on the oracle and the host build, shared by the tests below
PERTURBATIONS = [["nominal", {}], ["push_front_1.0", {"dv": [1.0, 0.0, 0.0]}], ["payload_3kg", {"added_mass": 3.0}]]
MANEUVERS = [["brake", [[0.0, 1.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]]], ["zigzag", [[0.0, 0.0, 0.5, 0.0], [0.1, 0.0, -0.5, 0.5], [0.22, 0.5, 0.0, -1.0]]]]
MODES = {"robust": dict(num_envs=48, seconds=0.4, perturbations=PERTURBATIONS, push_first_s=0.04, push_period_s=0.16, push_window_s=0.12, push_hold_s=0.02, gait=True, asymmetry=True),
         "maneuvers": dict(num_envs=40, seconds=0.4, maneuvers=MANEUVERS, maneuver_window_s=0.1, maneuver_hold_s=0.02),
         "sensors": dict(num_envs=48, seconds=0.3, sensors=tb.SENSORS, gait=True),
         "ladder": dict(task="go2", num_envs=48, seconds=0.4, warmup_s=0.1, ladder=True, ladder_levels=[0, 1, 2], ladder_scenarios=[["forward_1.0", 1.0, 0.0, 0.0]], ladder_distance=0.05)}
B, CONF = 48, 0.9
_RUNS = {}


def run(emu, mode):
    """-> (the option-on evaluator, its result, the result of `bootstrap` alone) of the same weights"""
    if mode not in _RUNS:
        cfg = dict(MODES[mode], bootstrap=B, confidence=CONF)
        ac = small_actor_critic()
        ev_ci, ev_on = make_evaluator(emu, **cfg), make_evaluator(emu, bootstrap_all=True, **cfg)
        _RUNS[mode] = (ev_on, ev_on.evaluate(ac), ev_ci.evaluate(ac), ac, cfg)
        ev_ci.close()
    return _RUNS[mode]


def strip(v):
    """a result without what `bootstrap_all` adds: every "ci", and the bootstrap's "tables" and "metrics" """
    return {k: strip(x) for k, x in v.items() if k not in ("ci", "tables", "metrics")} if isinstance(v, dict) else v


def tree_leaves(d, path=()):
    """every dict with "n_envs" below `d`, with its path"""
    if isinstance(d, dict):
        if "n_envs" in d:
            yield path, d
        else:
            for k, x in d.items():
                yield from tree_leaves(x, path + (k,))


def all_ci(res):
    """every "ci" dict of a result, with a name"""
    out = [(p, d["ci"]) for p, d in tb.leaves(res)]
    out += [("ladder/" + "/".join(map(str, p)), d["ci"]) for p, d in tree_leaves(res.get("ladder") or {})]
    out += [("summary/" + t, d["ci"]) for t, d in (res.get("ladder_summary") or {}).items()]
    for sec in ("gait", "asymmetry"):
        out += [(sec + "/" + "/".join(map(str, p)), d["ci"]) for p, d in tree_leaves(res.get(sec) or {})]
    return out


def same_scalars(a, b):
    return [(t, np.float64(v).tobytes()) for t, v in a] == [(t, np.float64(v).tobytes()) for t, v in b]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluator_key_off_is_ci_alone(emu, mode):
    """`bootstrap_all = False` next to `bootstrap`, and the key on next to `bootstrap = 0`: the evaluator without the key"""
    from go2_rl_gym_amd.utils.evaluator import format_table, results_dict, scalars
    _, _, ci, ac, cfg = run(emu, mode)
    ev_off = make_evaluator(emu, bootstrap_all=False, **cfg)
    off = ev_off.evaluate(ac)
    assert not hasattr(ev_off, "boot_outs") and tb.same_value(off, ci) and tb.same_value(results_dict(off, 3), results_dict(ci, 3)) and format_table(off) == format_table(ci)
    assert same_scalars(scalars(off), scalars(ci)) and "tables" not in ci["bootstrap"] and "metrics" not in ci["bootstrap"]
    ev_off.close()
    ev_zero, ev_none = make_evaluator(emu, **dict(cfg, bootstrap=0, bootstrap_all=True)), make_evaluator(emu, **dict(cfg, bootstrap=0))
    zero, none = ev_zero.evaluate(ac), ev_none.evaluate(ac)
    assert not hasattr(ev_zero, "boot_outs") and not hasattr(ev_zero, "boot_out") and "bootstrap" not in zero and tb.same_value(zero, none)
    ev_zero.close(); ev_none.close()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluator_key_on_changes_nothing_else_and_repeats(emu, mode):
    ev_on, on, ci, ac, cfg = run(emu, mode)
    # on against off: every value other than "ci", the tables and the metrics
    assert set(on) == set(ci) and tb.same_value(strip(on), strip(ci))
    for (p, d_on), (q, d_ci) in zip(tb.leaves(on), tb.leaves(ci)):          # what `bootstrap` alone puts there stays as it is
        assert p == q and all(tb.same_value(d_on["ci"][k], d_ci["ci"][k]) for k in d_ci["ci"])
    # the same weights again: the same bytes
    again = ev_on.evaluate(ac)
    assert list(again["bootstrap"]["tables"]) == list(on["bootstrap"]["tables"]) and tb.same_value(again["bootstrap"], on["bootstrap"]) and str(all_ci(again)) == str(all_ci(on))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluator_key_sets_and_order_of_every_interval(emu, mode):
    from go2_rl_gym_amd.utils.evaluator import ASYM_KEYS, CI_KEYS, GAIT_KEYS, LADDER_KEYS, LADDER_SUMMARY_KEYS, MANEUVER_KEYS, ROBUST_KEYS
    ev_on, on, _, _, cfg = run(emu, mode)
    robust, maneuver, gait = set(ROBUST_KEYS) - {"pushes"}, set(MANEUVER_KEYS) - {"switches"}, set(GAIT_KEYS)
    fams = {"robust": ["robust", "gait", "asym"], "maneuvers": ["maneuver"], "sensors": ["gait"], "ladder": ["ladder"]}[mode]
    assert list(on["bootstrap"]["tables"]) == fams
    for f in fams:
        assert on["bootstrap"]["tables"][f].shape == (B, ev_on.num_cells, FAMILIES[f].cols) and (on["bootstrap"]["tables"][f][:, :, FAMILIES[f].n_col] == np.bincount(ev_on.cell_host)[None]).all()
    want_overall = set(CI_KEYS) | {"robust": robust | gait, "maneuvers": maneuver, "sensors": gait, "ladder": {"cleared", "mean_level_cleared"}}[mode]
    for path, d in tb.leaves(on):
        kind = path.split("/")[0]
        want = set(CI_KEYS)
        if kind == "overall":
            want = want_overall
        elif mode == "robust" and kind in ("cells", "perturbations"):
            want |= robust
        elif mode == "maneuvers" and kind in ("groups", "maneuvers"):
            want |= maneuver
        assert set(d["ci"]) == want, (path, set(d["ci"]) ^ want)
        assert not {"pushes", "switches", "n_envs", "equivariance_max"} & set(d["ci"])
    if mode == "ladder":
        for p, d in tree_leaves(on["ladder"]):
            assert set(d["ci"]) == set(CI_KEYS) | set(LADDER_KEYS), p
        assert all(set(d["ci"]) == set(LADDER_SUMMARY_KEYS) for d in on["ladder_summary"].values())
    if "gait" in fams:
        n = 0
        for p, d in tree_leaves(on["gait"]):
            assert set(d["ci"]) == set(d) - {"n_envs", "ci"} and "slip_speed/%s" % ev_on.foot_names[0] in d["ci"], p
            n += 1
        assert n == len(list(tree_leaves(strip(on["gait"])))) > 4
    if "asym" in fams:
        for p, d in tree_leaves(on["asymmetry"]):
            assert set(d["ci"]) == set(ASYM_KEYS) - {"equivariance_max"} and "left_share/torque" in d["ci"], p
    for name, c in all_ci(on):
        for k, (lo, hi) in c.items():
            assert lo <= hi or (np.isnan(lo) and np.isnan(hi)), (name, k)
    want_metrics = set(want_overall) | (set(on["asymmetry"]["overall"]["ci"]) if "asym" in fams else set()) | (set(on["gait"]["overall"]["ci"]) if "gait" in fams else set())
    assert set(on["bootstrap"]["metrics"]) == want_metrics and all(v.shape == (B,) and v.dtype == np.float64 for v in on["bootstrap"]["metrics"].values())


def check_leaf(ev, leaf, rows, rowfn, twin, keys):
    """rows [B, cols]: a leaf's replicate rows pooled by the test -> the twin's replicates are the row function's figures bit for bit (three replicates), and the leaf's
    intervals are interval() of the row function's figures"""
    from go2_rl_gym_amd.utils.evaluator import interval
    reps, figures = twin(rows), [rowfn(rows[b]) for b in range(B)]
    for b in (0, 17, B - 1):
        for k in keys:
            assert np.float64(figures[b][k]).tobytes() == np.float64(reps[k][b]).tobytes(), (k, b, figures[b][k], reps[k][b])
    for k in keys:
        want = interval(np.asarray([d[k] for d in figures]), CONF)
        assert tb.same_value(leaf["ci"][k], want), (k, leaf["ci"][k], want)


def check_leaves(ev, on, emu_mode):
    """a few leaves of every kind the mode reports, pooled here with _cell_views / _asym_pool one axis further in"""
    from go2_rl_gym_amd.utils import evaluator as E
    tabs, S, T, t0, dt = on["bootstrap"]["tables"], ev.S, ev.T, ev.terrain_names[0], ev.dt
    s = [x[0] for x in ev.scenarios]
    names = list(ev.axis_names) if ev.axis_names is not None else []
    met = on["bootstrap"]["metrics"]
    if "robust" in tabs:
        twin, keys = (lambda r: E.robust_replicates(r, dt)), [k for k in E.ROBUST_KEYS if k != "pushes"]
        r3 = ev._cell_views(tabs["robust"])[1]
        check_leaf(ev, on["overall"], tabs["robust"].sum(1), ev._robust_row, twin, keys)
        check_leaf(ev, on["cells"][t0][s[1]][names[2]], r3[:, 1, 2], ev._robust_row, twin, keys)
        check_leaf(ev, on["perturbations"][names[1]], r3[:, :, 1].sum(1), ev._robust_row, twin, keys)
        assert all(met[k].tobytes() == twin(tabs["robust"].sum(1))[k].tobytes() for k in keys)
    if "maneuver" in tabs:
        twin, keys = (lambda r: E.maneuver_replicates(r, dt)), [k for k in E.MANEUVER_KEYS if k != "switches"]
        m = tabs["maneuver"]
        check_leaf(ev, on["overall"], m.sum(1), ev._maneuver_row, twin, keys)
        check_leaf(ev, on["groups"][t0][names[1]], m[:, 1], ev._maneuver_row, twin, keys)
        check_leaf(ev, on["maneuvers"][names[0]], m.reshape(B, T, S, -1)[:, :, 0].sum(1), ev._maneuver_row, twin, keys)
        assert all(met[k].tobytes() == twin(m.sum(1))[k].tobytes() for k in keys)
    if "ladder" in tabs:
        twin, keys = (lambda r: E.ladder_replicates(r, dt)), list(E.LADDER_KEYS)
        l4 = ev._cell_views(tabs["ladder"])[1]
        for ti, li in ((0, 0), (T - 1, 1), (1, 2)):
            check_leaf(ev, on["ladder"][ev.terrain_names[ti]][ev.levels[li]][s[0]], l4[:, ti, li, 0], ev._ladder_row, twin, keys)
        check_leaf(ev, on["overall"], tabs["ladder"].sum(1), ev._ladder_row, twin, ["cleared"])
    if "gait" in tabs:
        twin = lambda r: E.gait_replicates(r, dt, ev.foot_names)
        keys = [k for k in on["gait"]["overall"] if k not in ("n_envs", "ci")]
        assert len(keys) == 8 * 5 + 3
        table, view = ev._cell_views(tabs["gait"])
        check_leaf(ev, on["gait"]["overall"], table.sum(1), ev._gait_row, twin, keys)
        check_leaf(ev, on["gait"]["groups"][t0][s[2]], table[:, 2], ev._gait_row, twin, keys)
        check_leaf(ev, on["gait"]["cells"][t0][s[1]][names[1]], view[:, 1, 1], ev._gait_row, twin, keys)
        check_leaf(ev, on["gait"][ev.axis_key][names[2]], view[:, :, 2].sum(1), ev._gait_row, twin, keys)
        assert all(on["overall"]["ci"][k] == on["gait"]["overall"]["ci"][k] or np.isnan(on["overall"]["ci"][k]).all() for k in E.GAIT_KEYS)
    if "asym" in tabs:
        keys = [k for k in E.ASYM_KEYS if k != "equivariance_max"]
        pool = ev._asym_pool
        table, view = ev._cell_views(tabs["asym"], pool)
        check_leaf(ev, on["asymmetry"]["overall"], pool(table, 1), ev._asym_row, E.asym_replicates, keys)
        check_leaf(ev, on["asymmetry"]["groups"][t0][s[3]], table[:, 3], ev._asym_row, E.asym_replicates, keys)
        check_leaf(ev, on["asymmetry"]["cells"][t0][s[0]][names[1]], view[:, 0, 1], ev._asym_row, E.asym_replicates, keys)
        check_leaf(ev, on["asymmetry"]["perturbations"][names[0]], pool(view[:, :, 0], 1), ev._asym_row, E.asym_replicates, keys)
        assert all(met[k].tobytes() == E.asym_replicates(pool(table, 1))[k].tobytes() for k in keys)
        # the max column of a replicate table is the max over the drawn members: never above the cell's own
        c = _nn.ASYM_OUT.index("eq_max")
        assert (tabs["asym"][:, :, c] <= on["asymmetry_table"][None, :, c]).all() and (tabs["asym"][:, :, c] == on["asymmetry_table"][None, :, c]).any()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluator_replicates_are_the_row_functions_of_the_replicate_rows(emu, mode):
    ev_on, on, _, _, _ = run(emu, mode)
    check_leaves(ev_on, on, mode)


def check_ladder_summary(ev, on):
    """the summary's replicates by the loop rule of _ladder_results on every replicate's `cleared` curve"""
    from go2_rl_gym_amd.utils.evaluator import interval
    l4 = ev._cell_views(on["bootstrap"]["tables"]["ladder"])[1]
    means = []
    for ti, t in enumerate(ev.terrain_names):
        tops, sums = [], []
        for b in range(B):
            curve = [ev._ladder_row(l4[b, ti, li, 0])["cleared"] for li in range(len(ev.levels))]
            curve = [0.0 if np.isnan(c) else c for c in curve]
            top = -1
            for lv, c in zip(ev.levels, curve):
                if c < ev.ladder_pass_share:
                    break
                top = lv
            tops.append(float(top)); sums.append(float(sum(curve)))
        assert tb.same_value(on["ladder_summary"][t]["ci"], {"level_cleared": interval(tops, CONF), "mean_level_cleared": interval(sums, CONF)}), t
        means.append(sums)
    overall = np.asarray([float(np.mean([m[b] for m in means])) for b in range(B)])
    assert on["bootstrap"]["metrics"]["mean_level_cleared"].tobytes() == overall.tobytes()
    assert tb.same_value(on["overall"]["ci"]["mean_level_cleared"], interval(overall, CONF))
    lo, hi = on["overall"]["ci"]["mean_level_cleared"]
    assert lo <= on["overall"]["mean_level_cleared"] <= hi or lo == hi


def test_ladder_summary_replicates_follow_the_loop_rule(emu):
    ev_on, on, _, _, _ = run(emu, "ladder")
    check_ladder_summary(ev_on, on)
    curve = np.asarray([[1.0, 0.6, 0.2], [0.4, 1.0, 1.0], [np.nan, 1.0, 1.0], [0.5, 0.5, 0.5]])          # pass share 0.5: levels 0 and 1; none; none (empty = 0); all three
    top, mean = ev_on._ladder_summary_replicates(curve)
    assert top.tolist() == [float(ev_on.levels[1]), -1.0, -1.0, float(ev_on.levels[2])] and mean.tolist() == [1.0 + 0.6 + 0.2, 2.4, 2.0, 1.5]


def test_outputs_carry_the_new_intervals(emu):
    from go2_rl_gym_amd.utils.evaluator import CI_KEYS, format_table, results_dict, scalars
    ev_on, on, ci, _, _ = run(emu, "robust")
    d = yaml.safe_load(yaml.safe_dump(results_dict(on, 3)))
    assert d["bootstrap"] == {"replicates": B, "seed": 2718, "confidence": CONF}
    assert d["overall"]["ci"]["push_falls"] == on["overall"]["ci"]["push_falls"] or np.isnan(on["overall"]["ci"]["push_falls"]).all()
    assert d["gait"]["groups"]["plane"]["stand"]["ci"]["duty_factor"] == on["gait"]["groups"]["plane"]["stand"]["ci"]["duty_factor"]
    assert d["asymmetry"]["overall"]["ci"]["imbalance/torque"] == on["asymmetry"]["overall"]["ci"]["imbalance/torque"]
    tags, before = dict(scalars(on)), dict(scalars(ci))
    new = [k for k in on["overall"]["ci"] if k not in CI_KEYS]
    assert set(tags) - set(before) == ({"Eval/ci_%s/%s" % (side, k) for side in ("low", "high") for k in new}
                                       | {"Eval/asymmetry/ci_%s/%s" % (side, k) for side in ("low", "high") for k in on["asymmetry"]["overall"]["ci"]})
    assert all(np.float64(tags[t]).tobytes() == np.float64(v).tobytes() for t, v in before.items()) and all(isinstance(v, float) for v in tags.values() if not isinstance(v, int))
    assert [tags["Eval/asymmetry/ci_low/equivariance_rmse"], tags["Eval/asymmetry/ci_high/equivariance_rmse"]] == on["asymmetry"]["overall"]["ci"]["equivariance_rmse"]
    text = format_table(on)
    assert text.startswith(format_table(ci)) and all(c in text[len(format_table(ci)):] for c in ("push_falls", "slip_speed", "equivariance_rmse", "imbalance/torque"))
    assert "%.4g [%.4g, %.4g]" % ((on["asymmetry"]["overall"]["equivariance_rmse"],) + tuple(on["asymmetry"]["overall"]["ci"]["equivariance_rmse"])) in text


def test_the_cap_holds_the_sum_of_all_tables(emu):
    cfg = dict(MODES["robust"], bootstrap=B, bootstrap_all=True)
    cells = 4 * len(PERTURBATIONS)
    total = B * cells * 8 * (tb.COLS + FAMILIES["robust"].cols + FAMILIES["gait"].cols + FAMILIES["asym"].cols)
    with pytest.raises(ValueError, match="bootstrap_max_bytes") as e:
        make_evaluator(emu, bootstrap_max_bytes=total - 1, **cfg)
    assert all("%s: %d columns = %d bytes" % (n, c, B * cells * c * 8) in str(e.value) for n, c in (("eval", 12), ("robust", 7), ("gait", 55), ("asym", 25))) and str(total) in str(e.value)
    make_evaluator(emu, bootstrap_max_bytes=total, **cfg).close()
    make_evaluator(emu, bootstrap_max_bytes=B * cells * 8 * tb.COLS, **dict(cfg, bootstrap_all=False)).close()          # (the key off: the one table, as before)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
BASE = ["--task", "go2_flat", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"]


def test_cli_flag_and_config_key():
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    for argv, want in (([], (0, False)), (["--ci"], (1000, False)), (["--ci_all"], (1000, True)), (["--ci", "200", "--ci_all"], (200, True)), (["--ci_all", "--ci", "64"], (64, True))):
        args = get_args(BASE + argv)
        _, train_cfg = update_cfg_from_args(None, copy.deepcopy(task_registry.train_cfgs["go2_flat"]), args)
        assert (train_cfg.evaluation.bootstrap, train_cfg.evaluation.bootstrap_all) == want, argv
    for task in ("go2_flat", "go2"):
        assert task_registry.train_cfgs[task].evaluation.bootstrap_all is False


@pytest.mark.parametrize("argv, says", [
    (["--robust", "--ci", "--metric", "push_falls"], ["push_falls", "--ci_all"]),                                    # --ci alone: as before, and the way out is named
    (["--asymmetry", "--ci", "--metric", "equivariance_rmse"], ["equivariance_rmse", "--ci_all"]),
    (["--asymmetry", "--ci_all", "--metric", "left_share/torque"], ["left_share/torque", "no better direction"]),
    (["--asymmetry", "--ci_all", "--metric", "equivariance_max"], ["equivariance_max", "maximum"]),
    (["--robust", "--ci_all", "--metric", "pushes"], ["pushes", "count"]),
    (["--maneuvers", "--ci_all", "--metric", "switches"], ["switches", "count"]),
    (["--ci_all", "--metric", "n_envs"], ["n_envs", "count"]),
    (["--ci", "64", "--ci_all", "--metric", "push_falls"], ["push_falls", "--robust", "not on"]),
    (["--robust", "--ci_all", "--metric", "settle_time_s"], ["settle_time_s", "--maneuvers", "not on"]),
    (["--gait", "--ci_all", "--metric", "imbalance/torque"], ["imbalance/torque", "--asymmetry", "not on"]),
    (["--ci_all", "--metric", "slip_speed/FL"], ["slip_speed/FL", "--gait", "not on"]),
    (["--gait", "--ci_all", "--metric", "slip_speed/XX"], ["slip_speed/XX", "not a figure", "FL|RR|FR|RL"]),          # a foot the scorer does not name: no replicates
    (["--gait", "--ci_all", "--metric", "trot_share/FL"], ["trot_share/FL", "not a figure"]),                       # a pattern figure has no per-foot form
    (["--ci_all", "--metric", "mean_level_cleared"], ["mean_level_cleared", "--ladder", "not on"]),
    (["--ci_all", "--metric", "no_such_figure"], ["no_such_figure", "not a figure"])])
def test_cli_refusals_before_anything_is_loaded(tmp_path, monkeypatch, argv, says):
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate

    def loaded(*a, **k):
        raise AssertionError("an environment was made before the refusal")
    monkeypatch.setattr(task_registry, "make_env", loaded)
    with pytest.raises(ValueError) as e:
        evaluate(BASE + argv, log_root=str(tmp_path))
    assert all(w in str(e.value) for w in says), str(e.value)


def test_cli_compares_checkpoints_by_the_families_figures(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints --ci 64 --ci_all ranked by a robust and two asymmetry figures"""
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s = 28, 0.4, 0.1
    e.push_first_s, e.push_period_s, e.push_window_s, e.push_hold_s = 0.04, 0.16, 0.12, 0.02
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    base = ["--task", "go2_flat", "--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    run_dir = runner.log_dir
    env.close()
    kw = dict(log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    for flag, metric in (("--robust", "push_falls"), ("--asymmetry", "equivariance_rmse"), ("--asymmetry", "imbalance/torque"), ("--gait", "duty_factor/FL"),
                         ("--gait", "swing_clearance/RR")):
        out = evaluate(base + ["--all_checkpoints", flag, "--ci", "64", "--ci_all", "--metric", metric], **kw)
        comp = out["comparison"]
        if flag == "--gait":          # a per-foot figure: read from the gait section, ranked in its pooled figure's direction
            values = [r["gait"]["overall"][metric] for r in out["checkpoints"]]
            assert [r["value"] for r in comp["rows"]] == values or all(np.isnan(v) for v in values)
            finite = [v for v in values if not np.isnan(v)]
            assert not finite or out["best_value"] == (max(finite) if metric.startswith("swing_clearance") else min(finite))
        assert (comp["metric"], comp["replicates"]) == (metric, 64) and [r["checkpoint"] for r in comp["rows"]] == ["model_0.pt", "model_1.pt"] and "tied_with_best" in out
        for r in comp["rows"]:
            assert set(r) == {"checkpoint", "value", "ci", "diff_to_best", "diff_ci", "tied_with_best"}
            assert (r["checkpoint"] in out["tied_with_best"]) == r["tied_with_best"]
            if r["checkpoint"] == out["best"]:
                assert r["diff_ci"] == [0.0, 0.0] and r["tied_with_best"] and r["value"] == out["best_value"]
        files = os.listdir(os.path.join(run_dir, "eval_results"))
        name = "comparison_%s.yaml" % metric.replace("/", "_")
        assert name in files and "/" not in name and not os.path.isdir(os.path.join(run_dir, "eval_results", "comparison_imbalance"))
        d = yaml.safe_load(open(os.path.join(run_dir, "eval_results", name)))
        assert d["best"] == out["best"] and d["comparison"]["metric"] == metric
    assert "paired interval" in capsys.readouterr().out
