"""The evaluator's left-right asymmetry scores on the CPU: the host build of the go2nn_asym_* kernels (include/go2nn.h) against a float64 restatement written here — over
the whole scripted record at once, not step by step as the kernel works —, the reduce against math.fsum and max, the argument checks, the struct layout, and PolicyEvaluator
with `asymmetry` on the oracle + the host build: two policies whose equivariance error is known, the add-on discipline (nothing else moves with the flag on, nothing is
called with it off), every mode next to it, the CTS family and the writers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, load_nn_emu, reduce_groups, reduce_twice
import test_eval_host as th
from test_gait_host import MODES, store3
from test_robust_host import HostMemory
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import ASYM_FIELDS, ASYM_OUT, ASYM_PAIRS, ASYM_ROWS, GO2NN_ASYM_NUM, GO2NN_ASYM_OUT_IMB0, GO2NN_ASYM_OUT_NUM, GO2NN_ASYM_PAIR0, Go2nnAsymIn
from go2_rl_gym_amd.utils import symmetry as sym

EINVAL = -22
START, STEPS = -3, 36          # three warm-up calls, then the counted steps
CALLS = STEPS - START
THR = 2.5                      # [N] not the default: the kernel must read it.  Exact in fp32, so a force EQUAL to it can be scripted
BODIES = 19
FOOT_BODY = (10, 6, 18, 14)    # FR, FL, RR, RL: not the simulator's order — the kernel may not assume one
FOOT_SIDE = (-1, 1, -1, 1)
ACT_PERM, ACT_SIGN = sym.layout_table(sym.ACTION_BLOCKS)
JOINT_SIDE, JOINT_KIND = sym.joint_sides(), sym.joint_kinds()
COUNT_ROWS = ("eq_steps", "sym_steps", "contact_l", "contact_r")
FLOAT_ROWS = tuple(r for r in ASYM_ROWS[1:] if r not in COUNT_ROWS + ("eq_max",))
# A float row is a running fp32 sum of `steps` terms, each term the sum of up to twelve fp32 squares (or |products|) formed in a local first.  Against the exact value from
# the same fp32 inputs: e_j rounds once (2^-24 relative, 2^-23 on its square), the square or product once, the up to eleven local additions once each, at most 2^-24 of the
# step's term: 14 * 2^-24 of sum |term|; every addition to the row rounds once, 2^-24 of a partial sum that is at most sum |term|: steps * 2^-24 more.  (steps / 2 + 7) * 2^-23
# is below the bound stated here for steps >= 14 (tests/test_gait_host.py FLOAT_BOUND is the same statement for its sums).
FLOAT_BOUND = lambda steps, mag: steps * 2.0 ** -23 * mag
assert STEPS >= 14
CASES = ("reset_first", "reset_middle", "reset_last", "vy_negative_zero", "vy_tiny", "yaw_nonzero", "force_equals_threshold", "warmup_ignored")
CASES_MANY = CASES + ("never_symmetric", "zero_action")


def script(N, seed=0):
    """-> per call: actions, mirrored [CALLS, N, 12], commands [CALLS, N, 4], qd, tau [CALLS, N, 12], force [CALLS, N, 4, 3] fp32, reset [CALLS, N] bool.  Env e plays role
    e % 6 (random commands and resets from the twelfth env on): 0 resets on the first, a middle and the last counted frame, vy = -0.0, one step of vy = 1e-30, one of yaw != 0,
    a force equal to the threshold;  1 a plain forward walk;  2 vy = -0.0 throughout;  3 a command that is never symmetric;  4 a == 0;  5 a lateral command with symmetric gaps"""
    rng = np.random.default_rng(seed + N)
    d = {"actions": rng.normal(0, 1.0, (CALLS, N, 12)), "mirrored": rng.normal(0, 1.0, (CALLS, N, 12)), "qd": rng.normal(0, 5.0, (CALLS, N, 12)),
         "tau": rng.normal(0, 8.0, (CALLS, N, 12)), "force": rng.uniform(-1.0, 60.0, (CALLS, N, 4, 3))}
    d = {k: v.astype(np.float32) for k, v in d.items()}
    cmd = np.zeros((CALLS, N, 4), np.float32)
    cmd[..., 0], cmd[..., 3] = rng.uniform(-1, 2, (CALLS, N)), 7.0          # (the heading column is not the kernel's business)
    reset = np.zeros((CALLS, N), bool)
    w = -START
    for e in range(N):
        role = e % 6
        if e >= 12:
            cmd[:, e, 1] = rng.choice(np.asarray([0.0, -0.0, 1e-30, 0.5], np.float32), CALLS)
            cmd[:, e, 2] = rng.choice(np.asarray([0.0, 0.0, -0.0, -1.0], np.float32), CALLS)
            reset[w:, e] = rng.random(STEPS) < 0.15
        elif role == 0:
            reset[[w, w + 17, CALLS - 1], e] = True
            cmd[:, e, 1] = -0.0
            cmd[w + 5, e, 1], cmd[w + 9, e, 2] = 1e-30, 0.25
            d["force"][w + 3, e, 1, 2] = d["force"][w + 11, e, 2, 2] = THR
        elif role == 2:
            cmd[:, e, 1], cmd[:, e, 2] = -0.0, -0.0
        elif role == 3:
            cmd[:, e, 2] = 1.0
        elif role == 4:
            d["actions"][:, e] = 0.0
        elif role == 5:
            cmd[:, e, 1] = 0.5
            cmd[w + 4:w + 20, e, 1] = 0.0
    d["commands"], d["reset"] = cmd, reset
    return d


class Reference:
    """the rule in float64 over the whole record at once.  Inputs are the COUNTED frames: actions, mirrored, qd, tau [S, N, 12], commands [S, N, >= 3], fz [S, N, 4]
    (vertical force per foot of FOOT order), reset [S, N] -> rows[name] [N] for every table row but step, mag[name] (sum |term|) for FLOAT_ROWS, seen"""

    def __init__(self, actions, mirrored, commands, qd, tau, fz, reset, thr, foot_side=FOOT_SIDE, perm=ACT_PERM, sign=ACT_SIGN):
        a32, m32 = np.asarray(actions, np.float32), np.asarray(mirrored, np.float32)
        a, m, qd, tau = (np.asarray(x, np.float64) for x in (a32, m32, qd, tau))
        perm, sign = np.asarray(perm, np.int64), np.asarray(sign, np.float64)
        reset, commands = np.asarray(reset, bool), np.asarray(commands, np.float32)
        S, N = reset.shape
        e = a - sign * m[..., perm]
        e32 = a32 - sign.astype(np.float32) * m32[..., perm]          # one fp32 rounding: the product by +-1 is exact
        symm = ~reset & (commands[..., 1] == 0) & (commands[..., 2] == 0)          # (-0.0 == 0 in IEEE, 1e-30 is not)
        left, side = JOINT_SIDE > 0, np.asarray(foot_side) > 0
        r = {"eq_steps": np.full(N, float(S)), "eq_sq": (e ** 2).sum((0, 2)), "act_sq": (a ** 2).sum((0, 2)), "eq_max": np.abs(e32).max((0, 2)) if S else np.zeros(N, np.float32),
             "sym_steps": symm.sum(0).astype(np.float64)}
        for k, name in enumerate(("hip", "thigh", "calf")):
            r["eq_sq_" + name] = (e[..., JOINT_KIND == k] ** 2).sum((0, 2))
        down = (np.asarray(fz, np.float64) > thr) & symm[..., None]
        for name, term in (("act_sq", a ** 2), ("torque_sq", tau ** 2), ("power", np.abs(tau * qd))):
            term = term * symm[..., None]
            r[name + "_l"], r[name + "_r"] = term[..., left].sum((0, 2)), term[..., ~left].sum((0, 2))
        r["contact_l"], r["contact_r"] = down[..., side].sum((0, 2)).astype(np.float64), down[..., ~side].sum((0, 2)).astype(np.float64)
        self.rows, self.mag = r, {k: r[k] for k in FLOAT_ROWS}          # (every term is >= 0: sum |term| is the sum)
        self.seen = set()
        if S:
            for k, at in (("reset_first", 0), ("reset_last", S - 1)):
                if reset[at].any():
                    self.seen.add(k)
            if reset[1:-1].any():
                self.seen.add("reset_middle")
            vy, yaw = commands[..., 1], commands[..., 2]
            if ((vy == 0) & np.signbit(vy) & ~reset & (yaw == 0)).any():
                self.seen.add("vy_negative_zero")
            if ((vy != 0) & (np.abs(vy) < 1e-20)).any():
                self.seen.add("vy_tiny")
            if (yaw != 0).any():
                self.seen.add("yaw_nonzero")
            if ((np.asarray(fz) == thr) & symm[..., None]).any():
                self.seen.add("force_equals_threshold")
            if (r["sym_steps"] == 0).any():
                self.seen.add("never_symmetric")
            if (r["act_sq"] == 0).any() and (r["eq_sq"][r["act_sq"] == 0] > 0).all():
                self.seen.add("zero_action")


def store2(a, layout):
    """a logical [N, w] array as the libraries store it -> (flat storage, env stride, component stride)"""
    N, w = a.shape
    return (np.ascontiguousarray(a.T), 1, N) if layout == 1 else (np.ascontiguousarray(a), w, 1)


def buffers_at(d, call, N):
    """the simulator's buffers after the script's call `call`: every body that is no foot holds values the kernel must not read into the result"""
    cf = np.full((N, BODIES, 3), 1e6, np.float32)
    for f, b in enumerate(FOOT_BODY):
        cf[:, b] = d["force"][call, :, f]
    ds = np.stack([np.full((N, 12), 1e6, np.float32), d["qd"][call]], 2)          # [N, 12, (position, velocity)]
    return {"commands": d["commands"][call], "dof_state": ds, "torques": d["tau"][call], "contact_forces": cf, "reset_buf": d["reset"][call].astype(np.uint8)}


def stored(bufs, layout):
    """-> {field: (flat, env stride, component stride, extra)}: extra is the velocity offset of dof_state, the body stride of contact_forces"""
    out = {}
    for k in ("commands", "torques"):
        out[k] = store2(bufs[k], layout) + (0,)
    flat, es, bs, cs = store3(bufs["dof_state"], layout)          # [N, 12, 2]: the "bodies" are the joints, the "components" position and velocity
    out["dof_state"] = (flat, es, bs, cs)
    flat, es, bs, cs = store3(bufs["contact_forces"], layout)
    out["contact_forces"] = (flat, es, cs, bs)
    out["reset_buf"] = (bufs["reset_buf"], 1, 0, 0)
    return out


def asym_in(mem, h, st, thr=THR):
    a = Go2nnAsymIn()
    for k in ASYM_FIELDS:
        f = getattr(a, k)
        f.p, f.env_stride, f.comp_stride = mem.ptr(h[k]), st[k][1], st[k][2]
    a.dof_vel_offset, a.contact_body_stride = st["dof_state"][3], st["contact_forces"][3]
    a.foot_body[:], a.foot_side[:], a.joint_side[:], a.joint_kind[:] = FOOT_BODY, FOOT_SIDE, JOINT_SIDE.tolist(), JOINT_KIND.tolist()
    a.action_perm[:], a.action_sign[:], a.contact_threshold = ACT_PERM.tolist(), ACT_SIGN.tolist(), thr
    return a


def run_script(lib, mem, N, layout, seed=0):
    """the scripted sequence on `lib` with its buffers in `mem` -> (table fp32 [NUM, N], Reference, the script)"""
    d = script(N, seed)
    st = stored(buffers_at(d, 0, N), layout)
    h = {k: mem.put(v[0]) for k, v in st.items()}
    act, mir = mem.put(d["actions"][0]), mem.put(d["mirrored"][0])
    a = asym_in(mem, h, st)
    table = mem.put(np.full((GO2NN_ASYM_NUM, N), 7.0, np.float32))
    assert lib.go2nn_asym_begin(C.c_void_p(mem.ptr(table)), N, START, mem.stream) == 0, lib.go2nn_last_error()
    got = mem.get(table).reshape(GO2NN_ASYM_NUM, N)
    assert (got[0] == START).all() and not got[1:].any()
    for call in range(CALLS):
        for k, v in stored(buffers_at(d, call, N), layout).items():
            mem.set(h[k], v[0])
        mem.set(act, d["actions"][call])
        mem.set(mir, d["mirrored"][call])
        rc = lib.go2nn_asym_accumulate(C.byref(a), C.c_void_p(mem.ptr(act)), C.c_void_p(mem.ptr(mir)), C.c_void_p(mem.ptr(table)), N, mem.stream)
        assert rc == 0, lib.go2nn_last_error()
        if call == -START - 1:          # the warm-up is over: nothing but the counter has moved
            got = mem.get(table).reshape(GO2NN_ASYM_NUM, N)
            assert (got[0] == 0).all() and not got[1:].any()
    w = -START
    ref = Reference(d["actions"][w:], d["mirrored"][w:], d["commands"][w:], d["qd"][w:], d["tau"][w:], d["force"][w:, :, :, 2], d["reset"][w:], THR)
    if np.abs(d["actions"][:w]).sum() > 0 and (d["force"][:w, :, :, 2] > THR).any():
        ref.seen.add("warmup_ignored")
    return mem.get(table).reshape(GO2NN_ASYM_NUM, N), ref, d


def check_rows(rows, ref, steps, ids=None):
    """table rows {name: [K]} against a Reference of the same robots: counts exactly, eq_max to the bits, the float sums within FLOAT_BOUND -> largest gap / bound"""
    pick = (lambda v: v) if ids is None else (lambda v: v[ids])
    for k in COUNT_ROWS:
        np.testing.assert_array_equal(rows[k], pick(ref.rows[k]), err_msg=k)
    assert np.asarray(rows["eq_max"], np.float32).tobytes() == np.asarray(pick(ref.rows["eq_max"]), np.float32).tobytes()
    worst = 0.0
    for k in FLOAT_ROWS:
        gap, bound = np.abs(rows[k] - pick(ref.rows[k])), FLOAT_BOUND(steps, pick(ref.mag[k]))
        worst = max(worst, float((gap / np.maximum(bound, 1e-300)).max()))
        assert (gap <= bound).all(), (k, gap.max(), bound)
    return worst


def table_rows(table):
    return {k: table[i].astype(np.float64) if k != "eq_max" else table[i] for i, k in enumerate(ASYM_ROWS)}


def check_table(table, ref, N, what):
    cases = CASES_MANY if N >= 5 else CASES
    assert ref.seen >= set(cases), set(cases) - ref.seen          # the script met every edge it was written for
    assert (table[0] == STEPS).all()
    worst = check_rows(table_rows(table), ref, STEPS)
    print("%s: %d symmetric steps of %d; largest float-sum gap / bound (%d * 2^-23 * sum|term|) %.4f" % (what, ref.rows["sym_steps"].sum(), N * STEPS, STEPS, worst))
    assert 0 < ref.rows["sym_steps"].sum() < N * STEPS


def emu_reduce(emu, table, group, G):
    N = table.shape[1]
    out = np.full((G, GO2NN_ASYM_OUT_NUM), -1.0)
    assert emu.go2nn_asym_reduce(C.c_void_p(table.ctypes.data), C.c_void_p(group.ctypes.data), N, G, C.c_void_p(out.ctypes.data), None) == 0, emu.go2nn_last_error()
    return out


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_against_float64(emu, N, layout):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    table, ref, _ = run_script(emu, HostMemory(), N, layout)
    check_table(table, ref, N, "host N=%d layout=%d" % (N, layout))
    if N == 65:          # the figures of single robots: one group per env
        out = emu_reduce(emu, np.ascontiguousarray(table), np.arange(N, dtype=np.int32), N)
        never, zero, plain = (PolicyEvaluator._asym_row(out[e]) for e in (3, 4, 1))
        assert never["sym_steps_share"] == 0.0 and all(math.isnan(never[k]) for k in never if k.startswith(("left_share", "imbalance"))) and never["equivariance_rmse"] > 0
        assert math.isnan(zero["equivariance_rel"]) and zero["equivariance_rmse"] > 0 and zero["left_share/action"] != zero["left_share/action"] and zero["left_share/torque"] > 0
        assert plain["sym_steps_share"] == 1.0 and all(math.isfinite(v) for v in plain.values())
        r = {k: float(table[i, 1]) for i, k in enumerate(ASYM_ROWS)}
        assert plain["imbalance/power"] == abs(r["power_l"] - r["power_r"]) / (r["power_l"] + r["power_r"]) and plain["left_share/power"] == r["power_l"] / (r["power_l"] + r["power_r"])
        assert plain["equivariance_rmse"] == math.sqrt(r["eq_sq"] / (12.0 * STEPS)) and plain["equivariance_max"] == r["eq_max"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def reduce_case(N, G, seed=5):
    rng = np.random.default_rng(seed + N)
    table = rng.uniform(0, 500, (GO2NN_ASYM_NUM, N)).astype(np.float32)
    for r in COUNT_ROWS:
        table[ASYM_ROWS.index(r)] = rng.integers(0, 40, N)
    for p in range(4):          # robots without a left or a right term, without either, and balanced ones
        kind = rng.integers(0, 6, N)
        l, r_ = table[GO2NN_ASYM_PAIR0 + 2 * p], table[GO2NN_ASYM_PAIR0 + 2 * p + 1]
        l[kind == 0], r_[kind == 1] = 0.0, 0.0
        l[kind == 2] = r_[kind == 2] = 0.0
        r_[kind == 3] = l[kind == 3]
    return table, reduce_groups(rng, N, G, outside=0)          # (the host build refuses ids outside [0, G))


def check_reduce(out, table, group, G, N, what):
    """the group sizes, the counts of robots with an imbalance and the max exactly; every fp64 sum to N roundings of the running sum"""
    worst = 0.0
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        assert out[g, 0] == len(ids)
        for c in range(1, GO2NN_ASYM_OUT_NUM):
            if c < GO2NN_ASYM_OUT_IMB0:
                terms = [float(x) for x in table[c, ids]]
            else:
                p, odd = divmod(c - GO2NN_ASYM_OUT_IMB0, 2)
                pairs = [(float(table[GO2NN_ASYM_PAIR0 + 2 * p, e]), float(table[GO2NN_ASYM_PAIR0 + 2 * p + 1, e])) for e in ids]
                terms = [(1.0 if odd else abs(l - r) / (l + r)) for l, r in pairs if l + r > 0]
            if ASYM_OUT[c] == "eq_max":
                assert out[g, c] == max(terms, default=0.0), (g, c)
                continue
            gap, bound = abs(out[g, c] - math.fsum(terms)), N * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
            assert gap <= bound, (g, ASYM_OUT[c], gap, bound)
            worst = max(worst, gap / max(bound, 1e-300))
    print("%s: largest reduce gap / bound %.3f" % (what, worst))


@pytest.mark.parametrize("N,G", [(1, 3), (17, 3), (300, 5), (4096, 7)])
def test_reduce_against_fsum_and_max(emu, N, G):
    from go2_rl_gym_amd.utils.evaluator import ASYM_KEYS, PolicyEvaluator
    table, group = reduce_case(N, G)
    out = reduce_twice(lambda *a: emu.go2nn_asym_reduce(*a, None), table, group, G, GO2NN_ASYM_OUT_NUM)
    check_reduce(out, table, group, G, N, "host N=%d" % N)
    if N >= 17:
        assert (out[1] == 0).all() and (group == 1).sum() == 0 and len(set(np.bincount(group, minlength=G).tolist())) > 2
        n_imb = out[:, GO2NN_ASYM_OUT_IMB0 + 1::2]
        assert (n_imb.sum(0) < (group != 1).sum()).all() and (n_imb.sum(0) > 0).all()          # some robots have no imbalance figure, some do
    # the empty group: zeros, and figures that do not exist rather than an exception; pooling rows: sums, and the max of the max
    row = PolicyEvaluator._asym_row(out[1])
    assert row["n_envs"] == 0 and all(math.isnan(v) for k, v in row.items() if k != "n_envs") and set(row) == set(ASYM_KEYS) | {"n_envs"}
    pooled = PolicyEvaluator._asym_pool(out)
    c = ASYM_OUT.index("eq_max")
    assert pooled[c] == out[:, c].max() and (np.delete(pooled, c) == np.delete(out.sum(0), c)).all() and ASYM_OUT[GO2NN_ASYM_OUT_IMB0] == "act_sq_imb"


def test_argument_checks(emu):
    N, PAD = 4, 3
    bufs = {"commands": np.zeros((N, 4), np.float32), "dof_state": np.zeros((N, 12, 2), np.float32), "torques": np.zeros((N, 12), np.float32),
            "contact_forces": np.zeros((N, BODIES, 3), np.float32), "reset_buf": np.zeros(N, np.uint8)}
    st = stored(bufs, 0)
    mem = HostMemory()
    h = {k: v[0] for k, v in st.items()}
    act, mir = np.ones((N, 12), np.float32), np.ones((N, 12), np.float32)
    store = np.full(GO2NN_ASYM_NUM * N + 2 * PAD, 9.0, np.float32)          # the table between two runs of sentinel values
    table = store[PAD:-PAD]
    group, out = np.zeros(N, np.int32), np.full((2, GO2NN_ASYM_OUT_NUM), -3.0)
    p = lambda x: C.c_void_p(x.ctypes.data)
    untouched = lambda: (store == 9.0).all()
    padding_ok = lambda: (store[:PAD] == 9.0).all() and (store[-PAD:] == 9.0).all()

    def broken(edit):
        a = asym_in(mem, h, st)
        edit(a)
        return emu.go2nn_asym_accumulate(C.byref(a), p(act), p(mir), p(table), N, None)

    def set_item(name, i, v):
        def edit(a):
            getattr(a, name)[i] = v
        return edit
    good = asym_in(mem, h, st)
    assert emu.go2nn_asym_accumulate(None, p(act), p(mir), p(table), N, None) == EINVAL and emu.go2nn_last_error()
    for args in ((None, p(mir), p(table), N), (p(act), None, p(table), N), (p(act), p(mir), None, N), (p(act), p(mir), p(table), 0), (p(act), p(mir), p(table), -1)):
        assert emu.go2nn_asym_accumulate(C.byref(good), *args, None) == EINVAL and untouched(), args[3]
    for field in ASYM_FIELDS:
        assert broken(lambda a: setattr(getattr(a, field), "p", None)) == EINVAL and b"null" in emu.go2nn_last_error(), field
        assert broken(lambda a: setattr(getattr(a, field), "env_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
    for field in ASYM_FIELDS[:-1]:
        assert broken(lambda a: setattr(getattr(a, field), "comp_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
    for field in ("dof_vel_offset", "contact_body_stride"):
        assert broken(lambda a: setattr(a, field, 0)) == EINVAL, field
    for j in (0, 5, 11):
        for name, bad, word in (("action_perm", -1, b"action_perm"), ("action_perm", 12, b"action_perm"), ("action_sign", 0.5, b"action_sign"), ("action_sign", 0.0, b"action_sign"),
                                ("joint_side", 0, b"joint_side"), ("joint_side", 2, b"joint_side"), ("joint_kind", -1, b"joint_kind"), ("joint_kind", 3, b"joint_kind")):
            assert broken(set_item(name, j, bad)) == EINVAL and word in emu.go2nn_last_error(), (name, j, bad)
    for f in range(4):
        assert broken(set_item("foot_body", f, -1)) == EINVAL and b"foot_body" in emu.go2nn_last_error()
        assert broken(set_item("foot_side", f, 0)) == EINVAL and b"foot_side" in emu.go2nn_last_error()
    for thr in (-1.0, float("nan"), float("inf")):
        assert broken(lambda a: setattr(a, "contact_threshold", thr)) == EINVAL and b"contact_threshold" in emu.go2nn_last_error(), thr
    assert untouched()          # not one refused call has written
    assert emu.go2nn_asym_begin(None, N, 0, None) == EINVAL and emu.go2nn_asym_begin(p(table), 0, 0, None) == EINVAL and emu.go2nn_last_error() and untouched()
    assert emu.go2nn_asym_begin(p(table), N, -2, None) == 0 and padding_ok() and (table[:N] == -2).all() and not table[N:].any()
    assert broken(lambda a: None) == 0 and padding_ok() and (table[:N] == -1).all()
    for args in ((None, p(group), N, 2, p(out)), (p(table), None, N, 2, p(out)), (p(table), p(group), N, 2, None), (p(table), p(group), 0, 2, p(out)),
                 (p(table), p(group), N, 0, p(out)), (p(table), p(group), N, 65536, p(out))):
        assert emu.go2nn_asym_reduce(*args, None) == EINVAL and emu.go2nn_last_error() and (out == -3.0).all(), args[2:4]
    for bad in (-1, 2):          # the host build reads the ids
        g = group.copy()
        g[2] = bad
        assert emu.go2nn_asym_reduce(p(table), p(g), N, 2, p(out), None) == EINVAL and b"group" in emu.go2nn_last_error() and (out == -3.0).all()
    assert emu.go2nn_asym_reduce(p(table), p(group), N, 2, p(out), None) == 0 and out[0, 0] == N and padding_ok()


def test_asym_symbols_and_struct_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7 and _nn.GO2NN_ABI_VERSION == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_asym_begin", "go2nn_asym_accumulate", "go2nn_asym_reduce"):
            assert (" T " + f + "\n") in syms, (path, f)
    names = [n for n, _ in Go2nnAsymIn._fields_]
    consts = ("GO2NN_ASYM_NUM", "GO2NN_ASYM_OUT_NUM", "GO2NN_ASYM_PAIR0", "GO2NN_ASYM_OUT_IMB0", "GO2NN_ASYM_OUT_N", "GO2NN_ASYM_OUT_ROW0")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu", sizeof(Go2nnAsymIn));\n'
                   + "".join('printf(" %%d", (int)%s);\n' % c for c in consts) + "".join('printf(" %%zu", offsetof(Go2nnAsymIn, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(Go2nnAsymIn)
    assert got[1:1 + len(consts)] == [GO2NN_ASYM_NUM, GO2NN_ASYM_OUT_NUM, GO2NN_ASYM_PAIR0, GO2NN_ASYM_OUT_IMB0, 0, 1]
    assert got[1 + len(consts):] == [getattr(Go2nnAsymIn, n).offset for n in names]
    assert names[:5] == list(ASYM_FIELDS) and len(ASYM_OUT) == GO2NN_ASYM_OUT_NUM == GO2NN_ASYM_NUM + 8
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    enum = hdr[hdr.index("GO2NN_ASYM_STEP = 0"):hdr.index("GO2NN_ASYM_NUM\n}")]
    assert [e.strip().split(" ")[0].replace("GO2NN_ASYM_", "").lower() for e in enum.split(",") if e.strip()] == list(ASYM_ROWS)
    assert ASYM_ROWS[GO2NN_ASYM_PAIR0:] == tuple("%s_%s" % (p, s) for p in ASYM_PAIRS for s in "lr")


def test_tables_of_the_symmetry_module():
    """joint sides and kinds follow LEGS and JOINTS; the history table is the actor table per frame; a foot's side comes from its name"""
    assert sym.joint_sides().tolist() == [1, 1, 1, -1, -1, -1, 1, 1, 1, -1, -1, -1] and sym.joint_kinds().tolist() == [0, 1, 2] * 4
    perm = ACT_PERM.astype(np.int64)
    assert (sym.joint_sides()[perm] == -sym.joint_sides()).all() and (sym.joint_kinds()[perm] == sym.joint_kinds()).all()          # the mirror swaps sides, keeps kinds
    assert (ACT_SIGN == np.where(sym.joint_kinds() == 0, -1.0, 1.0)).all()
    obs = sym.layout_table(sym.ACTOR_BLOCKS)
    H = 5
    hp, hs = sym.history_table(obs, H)
    assert hp.dtype == np.int16 and hs.dtype == np.float32 and hp.shape == hs.shape == (H * 45,)
    x = np.random.default_rng(0).normal(size=(7, H, 45)).astype(np.float32)
    np.testing.assert_array_equal(sym.mirror_rows(x.reshape(7, -1), (hp, hs)).reshape(7, H, 45), sym.mirror_rows(x, obs))
    with pytest.raises(ValueError):
        sym.history_table(obs, 0)
    assert [sym.leg_side(n) for n in ("FL_foot", "FR_foot", "RL_foot", "RR_foot", "rl")] == [1, -1, 1, -1, 1]
    with pytest.raises(ValueError, match="legs"):
        sym.leg_side("base")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# PolicyEvaluator with `asymmetry`.  A step_callback keeps what the kernels of a step read: the observation (the copy half of the mirror launch: the bits the policy
# read), its mirror image, both actions and the buffers of ASYM_FIELDS after the step.
ASYM = dict(num_envs=64, seconds=1.0, warmup_s=0.1)
OBS_TABLE = sym.layout_table(sym.ACTOR_BLOCKS)


def keeper(frames):
    def cb(ev, k, counted):
        b = ev.env._buf
        f = {"counted": counted, "obs": ev.asym_obs[0].detach().clone().cpu().numpy(), "obs_m": ev.asym_obs[1].detach().clone().cpu().numpy(),
             "a": ev.asym_last[0].detach().clone().cpu().numpy(), "a_m": ev.asym_last[1].detach().clone().cpu().numpy(),
             "next_obs": (ev.env.obs_buf if ev.sensors is None else ev.delivered).detach().clone().cpu().numpy()}
        if ev.asym_hist is not None:
            f["hist"], f["hist_m"] = ev.asym_hist[0].detach().clone().cpu().numpy(), ev.asym_hist[1].detach().clone().cpu().numpy()
        for name in ASYM_FIELDS:
            f[name] = b[name].detach().clone().cpu().numpy()
        frames.append(f)
    return cb


def reference_of(ev, frames, actions=None, mirrored=None):
    """the Reference of the counted frames of an evaluation (the kept actions, or others in their place)"""
    fr = [f for f in frames if f["counted"]]
    st = lambda k: np.stack([f[k] for f in fr])
    feet = [int(i) for i in ev.env.feet_indices.tolist()]
    side = [sym.leg_side(ev.env.body_names[i]) for i in feet]
    return Reference(st("a") if actions is None else actions, st("a_m") if mirrored is None else mirrored, st("commands"), st("dof_state")[..., 1], st("torques"),
                     st("contact_forces")[:, :, feet, 2], st("reset_buf") != 0, ev.asym_threshold, foot_side=side)


def check_frames(frames):
    """every kept observation is the frame the policy was handed (the previous step's delivered frame or observation), its mirror image is mirror_rows of it, bit for bit"""
    for k, f in enumerate(frames):
        assert f["obs_m"].tobytes() == sym.mirror_rows(f["obs"], OBS_TABLE).astype(np.float32).tobytes(), k
        if k > 0:
            assert f["obs"].tobytes() == frames[k - 1]["next_obs"].tobytes(), k


def check_result(ev, res, ref, what):
    """res["asymmetry"] against a Reference per env: the per-cell table column by column (counts and max exactly, sums within the accumulate bound of every robot plus the
    reduce's), the per-robot imbalance columns from the device table, then every reported partition as _asym_row of the
    pooled rows of ITS robots' cells — found from the per-env axis arrays, not from the evaluator's cell arithmetic"""
    from go2_rl_gym_amd.utils.evaluator import ASYM_KEYS, PolicyEvaluator
    at, N = res["asymmetry_table"], ev.num_envs
    assert at.shape == (ev.num_cells, GO2NN_ASYM_OUT_NUM)
    worst = 0.0
    for c in range(ev.num_cells):
        ids = np.nonzero(ev.cell_host == c)[0]
        assert at[c, 0] == len(ids)
        for col, name in enumerate(ASYM_OUT):
            if name in COUNT_ROWS:
                assert at[c, col] == ref.rows[name][ids].sum(), (c, name)
            elif name == "eq_max":
                assert at[c, col] == (ref.rows[name][ids].max() if len(ids) else 0.0), (c, name)
            elif name in FLOAT_ROWS:
                want, mag = math.fsum(ref.rows[name][ids]), math.fsum(ref.mag[name][ids])
                bound = FLOAT_BOUND(ev.steps, mag) + N * 2.0 ** -53 * mag
                worst = max(worst, abs(at[c, col] - want) / max(bound, 1e-300))
                assert abs(at[c, col] - want) <= bound, (c, name, at[c, col], want, bound)
    t = ev.atable.cpu().numpy().astype(np.float64)          # the per-robot imbalance, from the device table itself
    for c in range(ev.num_cells):
        ids = np.nonzero(ev.cell_host == c)[0]
        for p in range(4):
            l, r = t[GO2NN_ASYM_PAIR0 + 2 * p, ids], t[GO2NN_ASYM_PAIR0 + 2 * p + 1, ids]
            has = l + r > 0
            want = math.fsum(np.abs(l - r)[has] / (l + r)[has])
            assert at[c, GO2NN_ASYM_OUT_IMB0 + 2 * p + 1] == has.sum() and abs(at[c, GO2NN_ASYM_OUT_IMB0 + 2 * p] - want) <= N * 2.0 ** -53 * want
    row = lambda ids: PolicyEvaluator._asym_row(PolicyEvaluator._asym_pool(at[np.unique(ev.cell_host[ids])]))
    asym = res["asymmetry"]
    S = len(ev.scenarios)
    families = {"overall": [((), np.arange(N))],
                "groups": [((t_, s[0]), np.nonzero(ev.group_host == ti * S + si)[0]) for ti, t_ in enumerate(ev.terrain_names) for si, s in enumerate(ev.scenarios)]}
    for key, axis, host in (("perturbations", ev.perturbations, getattr(ev, "pert_host", None)), ("sensors", ev.sensors, getattr(ev, "pert_host", None))):
        if axis is not None:
            families[key] = [((n[0],), np.nonzero(host == pi)[0]) for pi, n in enumerate(axis)]
            families["cells"] = [((t_, s[0], n[0]), np.nonzero((ev.group_host == ti * S + si) & (host == pi))[0]) for ti, t_ in enumerate(ev.terrain_names)
                                 for si, s in enumerate(ev.scenarios) for pi, n in enumerate(axis)]
    if ev.maneuvers is not None:
        families["maneuvers"] = [((m[0],), np.nonzero(ev.man_host == mi)[0]) for mi, m in enumerate(ev.maneuvers)]
    if ev.ladder:
        families["ladder"] = [((t_, lv, s[0]), np.nonzero((ev.group_host == ti * S + si) & (ev.level_of_env == lv))[0]) for ti, t_ in enumerate(ev.terrain_names)
                              for lv in ev.levels for si, s in enumerate(ev.scenarios)]
    assert set(asym) == set(families), (set(asym), set(families))
    for fam, parts in families.items():
        total = 0
        for path, ids in parts:
            leaf = asym[fam]
            for k in path:
                leaf = leaf[k]
            assert set(leaf) == set(ASYM_KEYS) | {"n_envs"}
            if len(ids):
                want = row(ids)
                for k in want:          # (the evaluator pools cells -> groups -> the whole, this pools the cells at once: fp64 sums in another order)
                    assert (math.isnan(leaf[k]) and math.isnan(want[k])) or abs(leaf[k] - want[k]) <= 1e-12 * abs(want[k]), (fam, path, k, leaf[k], want[k])
            else:
                assert leaf["n_envs"] == 0 and math.isnan(leaf["equivariance_rmse"])
            total += leaf["n_envs"]
        assert total == N, (fam, total)
    print("%s: %d cells, largest sum gap / bound %.4f, overall %s" % (what, ev.num_cells, worst, {k: float("%.4g" % v) for k, v in asym["overall"].items()}))
    return worst


def mirror_matrix(table):
    """M with M x = the mirror image of x"""
    perm, sign = table
    M = np.zeros((len(perm), len(perm)))
    M[np.arange(len(perm)), perm.astype(np.int64)] = sign
    return M


def one_hidden_actor_critic(h, seed=0):
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(seed)
    return ActorCritic(45, 263, 12, actor_hidden_dims=[2 * h], critic_hidden_dims=[16], activation="elu", init_noise_std=1.0)


def equivariant_actor_critic(h=16, seed=0):
    """hidden width 2 h: first layer rows [A ; A M_o] (bias [b ; b]), last layer [B , M_a B] (bias c with M_a c = c).  With u = elu(A o + b), v = elu(A M_o o + b) the mean
    is B u + M_a B v + c; the mirrored observation swaps u and v (M_o M_o = 1), and M_a (B u + M_a B v + c) = M_a B u + B v + c: the same.  The products by +-1 are exact,
    so the fp32 weights have the structure exactly; what is left is the rounding of two sums of the same terms in different orders"""
    ac = one_hidden_actor_critic(h, seed)
    Mo, Ma = mirror_matrix(OBS_TABLE), mirror_matrix((ACT_PERM, ACT_SIGN))
    with torch.no_grad():
        first, last = ac.actor[0], ac.actor[2]
        A, b = first.weight[:h].double().numpy().copy(), first.bias[:h].clone()
        B, c = last.weight[:, :h].double().numpy().copy(), last.bias.double().numpy().copy()
        first.weight.copy_(torch.from_numpy(np.concatenate([A, A @ Mo])).float())
        first.bias.copy_(torch.cat([b, b]))
        last.weight.copy_(torch.from_numpy(np.concatenate([B, Ma @ B], 1)).float())
        last.bias.copy_(torch.from_numpy(np.where(ACT_SIGN < 0, 0.0, c + c[ACT_PERM.astype(np.int64)])).float())
    assert first.weight.detach().double().numpy().tobytes() == np.concatenate([A, A @ Mo]).tobytes() and len(list(ac.actor)) == 3
    return ac


def forward64(ac, x):
    with torch.no_grad():
        return ac.actor.cpu().double()(torch.from_numpy(np.asarray(x, np.float64))).numpy()


def run_kept(emu, ac, make=None, **over):
    """make: another way to an evaluator (tests/test_gpu_asymmetry.py: the HIP libraries)"""
    frames = []
    ev = (make or th.make_evaluator)(emu, cb=keeper(frames), asymmetry=True, **dict(ASYM, **over))
    res = ev.evaluate(ac)
    return ev, res, frames


def constant_policy_case(emu, make=None, dev="cpu"):
    """first layer = 0: a = a_m = c whatever the observation, so e_j = c_j - sign_j c_perm(j) on every step of every robot"""
    ac = th.small_actor_critic()
    with torch.no_grad():
        ac.actor[0].weight.zero_()
    ev, res, frames = run_kept(emu, ac.to(dev), make)
    assert ev.warmup_steps == 5 and ev.steps == 50 and len(frames) == 55
    check_frames(frames)
    c = frames[0]["a"][0]
    for f in frames:
        assert (f["a"] == c).all() and (f["a_m"] == c).all()
    e = c.astype(np.float64) - ACT_SIGN * c.astype(np.float64)[ACT_PERM.astype(np.int64)]
    o, tol = res["asymmetry"]["overall"], FLOAT_BOUND(ev.steps, 1.0)          # relative: the sums' own bound (a square root halves it)
    assert abs(o["equivariance_rmse"] - math.sqrt((e ** 2).mean())) <= tol * math.sqrt((e ** 2).mean()) and o["equivariance_rmse"] > 0.01
    for k, name in enumerate(("hip", "thigh", "calf")):
        want = math.sqrt((e[JOINT_KIND == k] ** 2).mean())
        assert abs(o["equivariance_rmse/" + name] - want) <= tol * want, name
    assert o["equivariance_max"] == np.abs(c - ACT_SIGN * c[ACT_PERM.astype(np.int64)]).max()
    assert abs(o["equivariance_rel"] - math.sqrt((e ** 2).sum() / (c.astype(np.float64) ** 2).sum())) <= tol * o["equivariance_rel"]
    check_result(ev, res, reference_of(ev, frames), "constant policy")
    delta, a64, am64 = delta_of(ac, frames)
    check_against_float64(ev, res, a64, am64, delta, "constant policy")
    ev.close()


def equivariant_policy_case(emu, make=None, dev="cpu"):
    ac = equivariant_actor_critic().to(dev)
    ev, res, frames = run_kept(emu, ac, make)
    check_frames(frames)
    delta, a64, am64 = delta_of(ac, frames, both=False)
    rmse = res["asymmetry"]["overall"]["equivariance_rmse"]
    # in float64 the construction is equivariant to float64 rounding: the yardstick is sound
    e64 = a64 - ACT_SIGN * am64[..., ACT_PERM.astype(np.int64)]
    assert np.abs(e64).max() < 1e-12 and np.abs(a64).max() > 0.1
    print("equivariant by construction: equivariance_rmse %.3e, max %.3e, delta %.3e (bound 4 delta = %.3e)" % (rmse, res["asymmetry"]["overall"]["equivariance_max"], delta, 4 * delta))
    assert 0 < delta < 1e-4 and rmse <= 4 * delta
    check_result(ev, res, reference_of(ev, frames), "equivariant policy")
    check_against_float64(ev, res, a64, am64, delta_of(ac, frames)[0], "equivariant policy")
    ev.close()
    other = one_hidden_actor_critic(16, seed=1).to(dev)
    ev2, res2, frames2 = run_kept(emu, other, make)
    rmse2 = res2["asymmetry"]["overall"]["equivariance_rmse"]
    print("random weights of the same shape: equivariance_rmse %.3e = %.0f x the bound" % (rmse2, rmse2 / (4 * delta)))
    assert rmse2 >= 100 * 4 * delta
    check_result(ev2, res2, reference_of(ev2, frames2), "random policy")
    d2, b64, bm64 = delta_of(other, frames2)
    check_against_float64(ev2, res2, b64, bm64, d2, "random policy")
    ev2.close()


def delta_of(ac, frames, both=True):
    """delta: the largest gap between the forward kernel's actions and a float64 forward of the same weights on the kept observations.  both: over the mirrored forward of
    every step too — the comparison with the float64 restatement argues "e is the difference of two forwards, each within delta", which needs delta to bound both; the
    4 delta bound on the equivariant policy takes the plain forward's alone"""
    import copy
    ac64 = copy.deepcopy(ac)
    st = lambda k: np.stack([f[k] for f in frames if f["counted"]])
    a64, am64 = forward64(ac64, st("obs")), forward64(ac64, st("obs_m"))
    plain, mirrored = np.abs(a64 - st("a")).max(), np.abs(am64 - st("a_m")).max()
    return (max(plain, mirrored) if both else plain), a64, am64


def test_constant_policy_has_its_closed_form(emu):
    constant_policy_case(emu)


def check_against_float64(ev, res, a64, am64, delta, what):
    """the equivariance figures of the whole evaluation and of every group against the float64 forward of the kept observations [S, N, 12]: e is a difference of two
    forwards, each within delta of the kernel's, so every e_j is within 2 delta and so are a root mean square and a maximum of them; on top the sums' own bound (relative
    FLOAT_BOUND and the reduce's, halved by the square root).  equivariance_rel = |e| / |a|: |e| moves by at most 2 delta sqrt(n), |a| by delta sqrt(n)"""
    e64 = a64 - ACT_SIGN * am64[..., ACT_PERM.astype(np.int64)]
    S = len(ev.scenarios)
    parts = [(res["asymmetry"]["overall"], np.arange(ev.num_envs))]
    parts += [(res["asymmetry"]["groups"][t][s[0]], np.nonzero(ev.group_host == ti * S + si)[0]) for ti, t in enumerate(ev.terrain_names) for si, s in enumerate(ev.scenarios)]
    rel_sum, worst = FLOAT_BOUND(ev.steps, 1.0) + ev.num_envs * 2.0 ** -53, 0.0
    for got, ids in parts:
        e, a = e64[:, ids], a64[:, ids]
        want = {"equivariance_rmse": math.sqrt((e ** 2).mean()), "equivariance_max": np.abs(e).max()}
        for k, name in enumerate(("hip", "thigh", "calf")):
            want["equivariance_rmse/" + name] = math.sqrt((e[..., JOINT_KIND == k] ** 2).mean())
        for key, w in want.items():
            tol = 2 * delta + rel_sum * w
            worst = max(worst, abs(got[key] - w) / tol)
            assert abs(got[key] - w) <= tol, (what, key, got[key], w, tol)
        E, A, n = math.sqrt((e ** 2).sum()), math.sqrt((a ** 2).sum()), e.size
        tol = (2 * delta * math.sqrt(n) / (A - delta * math.sqrt(n))) * (1 + E / A) + rel_sum * E / A
        assert abs(got["equivariance_rel"] - E / A) <= tol, (what, got["equivariance_rel"], E / A, tol)
    print("%s: the figures against the float64 forward: largest gap / (2 delta + sum bound) %.4f, delta %.3e" % (what, worst, delta))


def test_equivariant_policy_reads_zero_and_a_random_one_does_not(emu):
    """an MLP made equivariant by construction reads at most 4 delta, delta being the forward kernel's own gap to float64 measured in the same run; random weights of the
    same shape read at least 100 times that bound"""
    equivariant_policy_case(emu)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Counting:
    """the host library with every call of a go2nn_asym_* function counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("go2nn_asym_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_flag_off_calls_nothing_and_flag_on_moves_nothing_else(emu):
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import results_dict
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    ac = th.small_actor_critic()
    over = dict(ASYM, gait=True, record=1, blackbox=1, blackbox_seconds=0.2)
    lib = Counting(emu)
    runs = {}
    for name, extra in (("never", {}), ("off", dict(asymmetry=False)), ("on", dict(asymmetry=True))):
        ev = th.make_evaluator(lib, **dict(over, **extra))
        runs[name] = (ev, ev.evaluate(ac))
        if name == "off":
            assert lib.calls == {} and ev.asymmetry is False and not any(hasattr(ev, k) for k in ("atable", "aout", "asym_obs", "asym_tables"))
    (ev, res), (_, res0), (_, res1) = runs["on"], runs["never"], runs["off"]
    assert lib.calls == {"go2nn_asym_begin": 1, "go2nn_asym_accumulate": ev.warmup_steps + ev.steps, "go2nn_asym_reduce": 1}
    assert not any("asym" in k for k in res1) and set(res1) == set(res0) and str(results_dict(res1)) == str(results_dict(res0))
    assert set(res) - set(res0) == {"asymmetry", "asymmetry_table", "asymmetry_cells", "asymmetry_contact_threshold"} and res["asymmetry_cells"] == ["terrain", "scenario"]
    for other in (res0, res1):
        assert res["table"].tobytes() == other["table"].tobytes() and res["gait_table"].tobytes() == other["gait_table"].tobytes()
        assert str(res["overall"]) == str(other["overall"]) and str(res["groups"]) == str(other["groups"]) and str(res["gait"]) == str(other["gait"])
        assert res["trace"]["frames"].tobytes() == other["trace"]["frames"].tobytes()
        assert set(res["falls"]) == set(other["falls"])
        for k, v in res["falls"].items():
            assert (v.tobytes() == other["falls"][k].tobytes()) if isinstance(v, np.ndarray) else (str(v) == str(other["falls"][k])), k
    again = ev.evaluate(ac)          # the same weights twice
    assert again["asymmetry_table"].tobytes() == res["asymmetry_table"].tobytes() and str(again["asymmetry"]) == str(res["asymmetry"])
    for e, _ in runs.values():
        e.close()
    for task in ("go2_flat", "go2_cts"):
        assert task_registry.get_cfgs(task)[1].evaluation.asymmetry is False
    assert get_args(["--asymmetry"]).asymmetry is True and get_args([]).asymmetry is False
    _, cfg = update_cfg_from_args(None, task_registry.get_cfgs("go2_flat")[1], get_args(["--asymmetry", "--gait"]))
    assert cfg.evaluation.asymmetry is True and cfg.evaluation.gait is True and task_registry.get_cfgs("go2_flat")[1].evaluation.asymmetry is False


@pytest.mark.parametrize("mode", sorted(set(MODES) - {"ladder"}))          # (the ladder's partitions go through the tree tests/test_gait_host.py walks on a terrain task)
def test_asymmetry_next_to_every_mode(emu, mode):
    """next to each extra axis the mode's own results are those of the run without the flag, byte for byte; the kept frames give the table; every partition the mode
    reports is the pool of its cells; under sensors the DELIVERED frame is what is mirrored; under maneuvers the command of the step decides what counts as symmetric"""
    over = dict(ASYM, **MODES[mode])
    task = over.pop("task")
    ac = th.small_actor_critic()
    base = th.make_evaluator(emu, task=task, **over)
    res0 = base.evaluate(ac)
    base.close()
    frames = []
    ev = th.make_evaluator(emu, task=task, cb=keeper(frames), asymmetry=True, **over)
    res = ev.evaluate(ac)
    own = {"perturbations": "robust_table", "sensors": "cell_table", "maneuvers": "maneuver_table", "ladder": "ladder_table"}[mode]
    assert res["table"].tobytes() == res0["table"].tobytes() and res[own].tobytes() == res0[own].tobytes() and str(res["overall"]) == str(res0["overall"])
    check_frames(frames)          # (under sensors: the DELIVERED frame of the step before)
    ref = reference_of(ev, frames)
    check_result(ev, res, ref, mode)
    assert mode in res["asymmetry"] and ("cells" in res["asymmetry"]) == (mode in ("perturbations", "sensors"))
    if mode == "maneuvers":          # start_1.0: symmetric throughout; turn_flip: never
        m = res["asymmetry"]["maneuvers"]
        assert m["start_1.0"]["sym_steps_share"] == 1.0 and m["turn_flip"]["sym_steps_share"] == 0.0 and math.isnan(m["turn_flip"]["imbalance/torque"])
    ev.close()


def test_cts_family_and_recurrent(emu):
    """the CTS student on go2_flat_cts: the history the encoder is fed is mirror_rows(history, history_table) bit for bit, the figures are those of the kept frames; a
    mixture model runs through its module's own formulation; a recurrent policy is refused before anything runs"""
    from test_sensor_host import small_models
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_moe_cts import ActorCriticMoECTS
    models = small_models()
    frames = []
    ev = th.make_evaluator(emu, task="go2_flat_cts", cb=keeper(frames), asymmetry=True, **ASYM)
    base = th.make_evaluator(emu, task="go2_flat_cts", **ASYM)
    res, res0 = ev.evaluate(models["cts"]), base.evaluate(models["cts"])
    assert ev._policy.kernels and res["table"].tobytes() == res0["table"].tobytes()
    base.close()
    H = models["cts"].history_length
    htab = sym.history_table(OBS_TABLE, H)
    check_frames(frames)
    for k, f in enumerate(frames):
        assert f["hist"].shape == (64, H * 45) and f["hist_m"].tobytes() == sym.mirror_rows(f["hist"], htab).astype(np.float32).tobytes(), k
        assert f["hist"].reshape(64, H, 45)[:, -1].tobytes() == f["obs"].tobytes() or f["hist"].reshape(64, H, 45)[:, 0].tobytes() == f["obs"].tobytes()          # the ring holds the frame
    check_result(ev, res, reference_of(ev, frames), "cts")
    # against a float64 forward of the module's own formulation on the kept frames
    import copy
    m64 = copy.deepcopy(models["cts"]).double()
    fr = [f for f in frames if f["counted"]]
    with torch.no_grad():
        fwd = lambda h, o: m64.policy_mean(m64.student_latent(torch.from_numpy(h.astype(np.float64)))[0], torch.from_numpy(o.astype(np.float64))).numpy()
        a64, am64 = np.stack([fwd(f["hist"], f["obs"]) for f in fr]), np.stack([fwd(f["hist_m"], f["obs_m"]) for f in fr])
    delta = max(np.abs(a64 - np.stack([f["a"] for f in fr])).max(), np.abs(am64 - np.stack([f["a_m"] for f in fr])).max())
    assert 0 < delta < 1e-4
    check_against_float64(ev, res, a64, am64, delta, "cts")
    torch.manual_seed(5)
    moe = ActorCriticMoECTS(45, 263, 12, 24, 5, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], teacher_encoder_hidden_dims=[32], student_encoder_hidden_dims=[32])
    frames.clear()
    res_moe = ev.evaluate(moe)
    assert not ev._policy.kernels and res_moe["asymmetry"]["overall"]["equivariance_rmse"] > 0
    check_result(ev, res_moe, reference_of(ev, frames), "moe cts")
    ev.close()
    rec = th.make_evaluator(emu, asymmetry=True, **ASYM)
    with pytest.raises(NotImplementedError, match="twin hidden state"):
        rec.evaluate(models["lstm"])
    rec.close()
    from go2_rl_gym_amd.envs import task_registry
    cfg = copy.deepcopy(task_registry.get_cfgs("go2_flat")[0])          # any layout but the Go2 tasks': the tables' own ValueError, which _build_asymmetry lets through
    cfg.env.num_observations = 48
    with pytest.raises(ValueError, match="mirror table"):
        sym.mirror_tables(cfg)


def test_writers_cli_and_metric(emu, tmp_path):
    import yaml
    from go2_rl_gym_amd.scripts.evaluate import HIGHER_IS_BETTER, best_checkpoint, check_metric, metric_value
    from go2_rl_gym_amd.utils.evaluator import ASYM_KEYS, format_table, scalars, write_results
    ev = th.make_evaluator(emu, asymmetry=True, **ASYM)
    res = ev.evaluate(th.small_actor_critic())
    ev.close()
    plain = th.make_evaluator(emu, **ASYM)
    res0 = plain.evaluate(th.small_actor_critic())
    plain.close()
    tags = dict(scalars(res))
    o = res["asymmetry"]["overall"]
    assert all(tags["Eval/asymmetry/" + k] == o[k] for k in ASYM_KEYS) and tags["Eval/asymmetry/plane/forward_1.0/imbalance/torque"] == res["asymmetry"]["groups"]["plane"]["forward_1.0"]["imbalance/torque"]
    assert math.isnan(tags["Eval/asymmetry/plane/turn_1.0/left_share/power"]) and not any("asymmetry" in t for t, _ in scalars(res0))
    assert {t: v for t, v in scalars(res) if "asymmetry" not in t} == dict(scalars(res0))
    path = write_results(str(tmp_path), 7, res)
    back = yaml.safe_load(open(path))
    assert set(back["asymmetry"]) == {"overall", "groups"} and back["asymmetry"]["overall"]["equivariance_rmse"] == o["equivariance_rmse"]
    assert back["asymmetry"]["groups"]["plane"]["stand"]["n_envs"] == 16 and back["asymmetry"]["groups"]["plane"]["stand"]["sym_steps_share"] == 1.0
    assert "asymmetry" not in yaml.safe_load(open(write_results(str(tmp_path), 8, res0)))
    text, text0 = format_table(res), format_table(res0)
    assert text.startswith(text0) and "equivariance_rmse" in text and "imbalance/torque" in text and len(text.splitlines()) == len(text0.splitlines()) + 1 + 1 + 4 + 1
    rows = [{"checkpoint": "a", "overall": {"lin_vel_err": 0.1}, "asymmetry": {"overall": {"equivariance_rmse": 0.3, "imbalance/torque": float("nan"), "left_share/torque": 0.5}}},
            {"checkpoint": "b", "overall": {"lin_vel_err": 0.2}, "asymmetry": {"overall": {"equivariance_rmse": 0.02, "imbalance/torque": 0.4, "left_share/torque": 0.4}}}]
    assert best_checkpoint(rows, "equivariance_rmse")["checkpoint"] == "b" and best_checkpoint(rows[::-1], "equivariance_rmse")["checkpoint"] == "b"
    assert best_checkpoint(rows, "imbalance/torque")["checkpoint"] == "b" and best_checkpoint(rows, "lin_vel_err")["checkpoint"] == "a" and metric_value(rows[0], "equivariance_rmse") == 0.3
    assert not any(k.startswith(("equivariance", "imbalance")) for k in HIGHER_IS_BETTER)
    with pytest.raises(ValueError, match="no better direction"):
        best_checkpoint(rows, "left_share/torque")
    with pytest.raises(ValueError, match="imbalance/torque"):
        check_metric("left_share/torque")
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    with pytest.raises(ValueError, match="left_share"):          # refused before anything is loaded
        evaluate(["--task", "go2_flat", "--asymmetry", "--metric", "left_share/torque"], log_root=str(tmp_path))


def test_cli_names_the_most_equivariant_checkpoint(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints --asymmetry --metric equivariance_rmse: lower is better, and the
    figure comes from the rows' own asymmetry section"""
    import copy
    import json
    from helpers import load_oracle
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import ASYM_KEYS
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
    env.close()
    capsys.readouterr()
    out = evaluate(base + ["--asymmetry", "--all_checkpoints", "--metric", "equivariance_rmse"], log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    names = [r["checkpoint"] for r in out["checkpoints"]]
    assert names == ["model_0.pt", "model_1.pt"] and out["metric"] == "equivariance_rmse" and out["best"] in names
    assert out["best_value"] == min(r["asymmetry"]["overall"]["equivariance_rmse"] for r in out["checkpoints"]) and out["best_value"] > 0
    for r in out["checkpoints"]:
        assert set(ASYM_KEYS) < set(r["asymmetry"]["overall"]) and set(r["asymmetry"]["groups"]) == set(r["groups"]) and not set(ASYM_KEYS) & set(r["overall"])
    text = capsys.readouterr().out
    assert "equivariance_rmse" in text and json.loads([l for l in text.splitlines() if l.startswith("{")][-1])["best"] == out["best"]
