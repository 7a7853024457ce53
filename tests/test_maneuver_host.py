"""The evaluator's scripted command maneuvers on the CPU: the host build of the go2nn_maneuver_* kernels (include/go2nn.h) against a float64 restatement written here over a
scripted sequence in which the envs meet every branch, the reduce against math.fsum, the spec and argument checks, the struct layout, and PolicyEvaluator with `maneuvers`
on the oracle + the host build: the whole table recomputed from the recorded buffers, the exact equivalences (one-segment maneuvers = scenarios, maneuvers off = nothing),
reproducibility, the results' shape, and the CLI.

The bounds.  u = 2^-24.  The kernel's err_lin differs from the float64 value of the same fp32 inputs by at most 3 u relative (a difference u, its square and the sum of two
squares u each — halved by the square root —, the root u), err_ang by u, tilt by 2 u.  A sum of n such addends in fp32 adds (n - 1) u (the first addition, to 0, is exact):
(n + 2) u <= n 2^-23 for n >= 2, which is the bound asserted, n being the env's own number of addends (WIN_STEPS for the window sums, the closed windows for PEAK_TILT_SUM,
1 for PEAK_TILT).  The scripted sequence has no env with exactly one window step.  Every decision (err < thr) is taken at least MARGIN away from its threshold, asserted
on the float64 reference; MARGIN = 1e-5 is 50 times the 3 u above, so no decision can flip on rounding and flags, counts and step rows must be EQUAL."""
import contextlib
import copy
import ctypes as C
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from helpers import ROOT, load_nn_emu, load_oracle, lognormal_table, reduce_groups, reduce_twice
import test_eval_host as th
from test_robust_host import HostMemory, logical, store
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import (GO2NN_MANEUVER_ACC_FIRST, GO2NN_MANEUVER_ACC_NUM, GO2NN_MANEUVER_MAX_SEGS, GO2NN_MANEUVER_NUM, MANEUVER_FIELDS, MANEUVER_OUT, MANEUVER_ROWS,
                                Go2nnManeuverIn, Go2nnManeuverSpec)
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.utils import get_args

R = {n: i for i, n in enumerate(MANEUVER_ROWS)}
O = {n: i for i, n in enumerate(MANEUVER_OUT)}
EXACT_ROWS = ("step", "open", "ok_run", "is_settled", "is_fell", "switches", "switch_falls", "settled", "settle_steps", "win_steps")
SUM_ROWS = {"win_lin_err": "win_steps", "win_ang_err": "win_steps", "peak_tilt_sum": "closed"}          # fp32 sum row -> what counts its addends
MARGIN = 1e-5
EINVAL = -22
WIDTH = {"commands": 4, "base_lin_vel": 3, "base_ang_vel": 3, "projected_gravity": 3, "reset_buf": 0, "time_out_buf": 0}
START, CALLS = -3, 47          # counted steps -3 .. 43: the last windows of maneuvers 1 and 2 close on the last step
# M = 3 maneuvers of 1, 2 and 8 segments
SPECS = [dict(window=5, hold=2, thr_lin=0.3, thr_ang=0.3, segs=[(0, 0.5, 0.0, 0.0)]),
         dict(window=10, hold=4, thr_lin=0.3, thr_ang=0.25, segs=[(0, 1.0, 0.0, 0.0), (34, -1.0, 0.25, 0.5)]),
         dict(window=6, hold=3, thr_lin=0.2, thr_ang=0.4, segs=[(0, 0.0, 0.0, 0.0), (2, 1.0, 0.0, 0.0), (8, 0.0, 0.5, 0.0), (14, 0.0, 0.0, 1.0), (20, 2.0, 0.0, 0.0),
                                                                 (26, 0.0, 0.0, 0.0), (32, -1.0, 0.0, -1.0), (38, 0.5, -0.5, 0.5)])]
PATTERNS = 7


def make_specs(dicts):
    specs = (Go2nnManeuverSpec * len(dicts))()
    for sp, d in zip(specs, dicts):
        sp.count, sp.window, sp.hold, sp.thr_lin, sp.thr_ang = d.get("count", len(d["segs"])), d["window"], d["hold"], d["thr_lin"], d["thr_ang"]
        for k, seg in enumerate(d["segs"]):
            sp.start[k] = seg[0]
            sp.cmd[k][:] = seg[1:4]
    return specs


def man_of(N):
    """env -> maneuver: 1, 2, 0 in turn (so env 0 of N = 1 switches); the last env (N > 1) and env 5 (N > 20) carry ids outside [0, M) and are left alone"""
    man = np.asarray([(1, 2, 0)[e % 3] for e in range(N)], np.int32)
    if N > 1:
        man[N - 1] = 7
    if N > 20:
        man[5] = -1
    return man


def segment(d, s):
    """index of the segment of spec dict d in force at step s"""
    return max(k for k, seg in enumerate(d["segs"]) if seg[0] <= max(s, 0))


def schedule(dicts, man, s, width=4):
    """-> (commands [N, width] fp32 as the kernels must write them at step s, mask of the envs that have a maneuver)"""
    has = (man >= 0) & (man < len(dicts))
    cmd = np.zeros((len(man), width), np.float32)
    for e in np.nonzero(has)[0]:
        d = dicts[man[e]]
        cmd[e, :3] = d["segs"][segment(d, s)][1:4]
    return cmd, has


def scripted_step(rng, N, s, man, phi):
    """what the simulator shows after step s, by the env's pattern e % 7 and the window step j = 1 .. W its maneuver is in (0: no window open):
    0 settles at exactly H;  1 breaks its run at j = H (after H - 1 good steps) and settles at 2 H;  2 falls at j = 3 (two window steps before);  3 falls on the switch step
    itself;  4 is reset by a time-out at j = 2 — not a fall — and settles at H;  5 settles at H and falls at j = H + 1;  6 never settles (one error low, the other high,
    alternating).  Outside the windows everything is random, falls included.  -> {field: array}"""
    d = {"base_lin_vel": rng.normal(0, 1, (N, 3)), "base_ang_vel": rng.normal(0, 1, (N, 3)), "projected_gravity": rng.uniform(-0.3, 0.3, (N, 3)),
         "reset_buf": (rng.random(N) < 0.2), "time_out_buf": (rng.random(N) < 0.1)}
    for e in range(N):
        if not 0 <= man[e] < len(SPECS):
            continue
        sp = SPECS[man[e]]
        k = segment(sp, s)
        j = s - sp["segs"][k][0] + 1 if (k >= 1 and s - sp["segs"][k][0] < sp["window"]) else 0
        if j == 0:
            continue
        p, H = e % PATTERNS, sp["hold"]
        low = (p in (0, 4, 5)) or (p == 1 and j != H) or (p == 2)
        f_lin, f_ang = (0.5, 0.5) if low else (2.0, 2.0)
        if p == 6:
            f_lin, f_ang = (0.5, 2.0) if (k + j) % 2 else (2.0, 0.5)
        f_lin, f_ang = f_lin * rng.uniform(0.9, 1.1), f_ang * rng.uniform(0.9, 1.1)
        cmd = sp["segs"][k][1:4]
        d["base_lin_vel"][e, 0] = cmd[0] - f_lin * sp["thr_lin"] * math.cos(phi[e])
        d["base_lin_vel"][e, 1] = cmd[1] - f_lin * sp["thr_lin"] * math.sin(phi[e])
        d["base_ang_vel"][e, 2] = cmd[2] + f_ang * sp["thr_ang"] * (1 if e % 2 else -1)
        fall = (p == 2 and j == 3) or (p == 3 and j == 1) or (p == 5 and j == H + 1)
        timeout = p == 4 and j == 2
        d["reset_buf"][e], d["time_out_buf"][e] = fall or timeout, timeout
    return {k: v.astype(np.uint8 if k.endswith("_buf") else np.float32) for k, v in d.items()}


class Reference:
    """the rule of include/go2nn.h in float64, one env at a time.  `closest`: the smallest |err - thr| / thr of any decision; `closed`: the windows closed per env"""

    def __init__(self, N, start, dicts, man):
        self.N, self.dicts, self.man = N, dicts, man
        self.t = np.zeros((GO2NN_MANEUVER_NUM, N))
        self.t[R["step"]] = start
        self.closed = np.zeros(N)
        self.closest = float("inf")

    def accumulate(self, d):
        lin, ang, grav = (np.asarray(d[k], np.float64) for k in ("base_lin_vel", "base_ang_vel", "projected_gravity"))
        for e in range(self.N):
            t = self.t[:, e]
            s = int(t[R["step"]])
            if 0 <= self.man[e] < len(self.dicts):
                sp = self.dicts[self.man[e]]
                k = segment(sp, s)
                cmd = [float(np.float32(x)) for x in sp["segs"][k][1:4]]
                if k >= 1 and sp["segs"][k][0] == s:
                    t[R["open"]], t[R["ok_run"]], t[R["is_settled"]], t[R["is_fell"]], t[R["peak_tilt"]] = 1, 0, 0, 0, 0
                    t[R["switches"]] += 1
                if t[R["open"]] > 0:
                    fall = bool(d["reset_buf"][e]) and not bool(d["time_out_buf"][e])
                    if not t[R["is_fell"]]:
                        if fall:
                            t[R["switch_falls"]] += 1
                            t[R["is_fell"]] = 1
                        else:
                            err_lin, err_ang = math.hypot(cmd[0] - lin[e, 0], cmd[1] - lin[e, 1]), abs(cmd[2] - ang[e, 2])
                            t[R["win_steps"]] += 1
                            t[R["win_lin_err"]] += err_lin
                            t[R["win_ang_err"]] += err_ang
                            t[R["peak_tilt"]] = max(t[R["peak_tilt"]], math.hypot(grav[e, 0], grav[e, 1]))
                            if not t[R["is_settled"]]:
                                thr_lin, thr_ang = float(np.float32(sp["thr_lin"])), float(np.float32(sp["thr_ang"]))
                                self.closest = min(self.closest, abs(err_lin - thr_lin) / thr_lin, abs(err_ang - thr_ang) / thr_ang)
                                if err_lin < thr_lin and err_ang < thr_ang:
                                    t[R["ok_run"]] += 1
                                    if t[R["ok_run"]] == sp["hold"]:
                                        t[R["settled"]] += 1
                                        t[R["settle_steps"]] += t[R["open"]]
                                        t[R["is_settled"]] = 1
                                else:
                                    t[R["ok_run"]] = 0
                    if t[R["open"]] == sp["window"]:
                        t[R["peak_tilt_sum"]] += t[R["peak_tilt"]]
                        t[R["open"]] = 0
                        self.closed[e] += 1
                    else:
                        t[R["open"]] += 1
            t[R["step"]] = s + 1

    def addends(self, row):
        return self.t[R["win_steps"]] if SUM_ROWS[row] == "win_steps" else self.closed


def compare_tables(table, ref, what):
    """the exact rows equal, the fp32 sums within n 2^-23 relative (n = the env's addends), PEAK_TILT within 2^-23 -> the largest gap / bound"""
    assert ref.closest >= MARGIN, ref.closest          # the condition under which the rows below must be EXACTLY equal
    t, r = table.astype(np.float64), ref.t
    for row in EXACT_ROWS:
        np.testing.assert_array_equal(t[R[row]], r[R[row]], err_msg=row)
    worst = {}
    for row in tuple(SUM_ROWS) + ("peak_tilt",):
        n = np.ones(ref.N) if row == "peak_tilt" else ref.addends(row)
        gap, bound = np.abs(t[R[row]] - r[R[row]]), n * 2.0 ** -23 * np.abs(r[R[row]])
        assert (gap <= bound).all(), (row, gap.max(), np.argmax(gap - bound))
        worst[row] = float((gap / np.maximum(bound, 1e-300)).max())
    print("%s: closest |err - thr| / thr %.2e, largest |table - ref| / bound: %s" % (what, ref.closest, ", ".join("%s %.3f" % kv for kv in worst.items())))


def maneuver_in(mem, handles, strides, M, width=4):
    a = Go2nnManeuverIn()
    for k in MANEUVER_FIELDS:
        f = getattr(a, k)
        f.p, (f.env_stride, f.comp_stride) = mem.ptr(handles[k]), strides[k]
    a.num_specs, a.num_commands = M, width
    return a


def run_script(lib, mem, N, layout, seed=0):
    """the scripted sequence on `lib` with its buffers in `mem`; the command row is checked bit for bit after every apply and every accumulate -> (table, Reference, man)"""
    rng = np.random.default_rng(seed + N)
    man, specs, M = man_of(N), make_specs(SPECS), len(SPECS)
    assert lib.go2nn_maneuver_check_specs(C.cast(specs, C.c_void_p), M) == 0, lib.go2nn_last_error()
    phi = rng.uniform(-np.pi, np.pi, N)
    ref = Reference(N, START, SPECS, man)
    shapes = {k: ((N, w) if w else (N,)) for k, w in WIDTH.items()}
    h, strides = {}, {}
    for k in MANEUVER_FIELDS:
        flat, es, cs = store(np.zeros(shapes[k], np.uint8 if k.endswith("_buf") else np.float32), layout)
        h[k], strides[k] = mem.put(flat), (es, cs)
    a = maneuver_in(mem, h, strides, M)
    table = mem.put(np.full((GO2NN_MANEUVER_NUM, N), 7.0, np.float32))
    specs_h, man_h = mem.put(np.frombuffer(bytes(specs), np.uint8)), mem.put(man)
    args = (C.byref(a), C.c_void_p(mem.ptr(specs_h)), C.c_void_p(mem.ptr(man_h)), C.c_void_p(mem.ptr(table)), N, mem.stream)
    assert lib.go2nn_maneuver_begin(C.c_void_p(mem.ptr(table)), N, START, mem.stream) == 0, lib.go2nn_last_error()
    got = mem.get(table).reshape(GO2NN_MANEUVER_NUM, N)
    assert (got[0] == START).all() and not got[1:].any()

    def commands_hold(s, junk, what):          # the schedule's command, the further column zeroed, bit for bit; an env without a maneuver keeps what it had
        want, has = schedule(SPECS, man, s)
        cmd = logical(mem.get(h["commands"]), shapes["commands"], layout)
        assert cmd[has].tobytes() == want[has].tobytes() and cmd[~has].tobytes() == junk[~has].tobytes(), (what, s)
    for call in range(CALLS):
        s = START + call
        junk = rng.normal(0, 1, shapes["commands"]).astype(np.float32)
        mem.set(h["commands"], store(junk, layout)[0])
        before = mem.get(table).tobytes()
        for _ in range(2 if call % 5 == 0 else 1):          # idempotent, and the table is not written
            assert lib.go2nn_maneuver_apply(*args) == 0, lib.go2nn_last_error()
            commands_hold(s, junk, "apply")
        assert mem.get(table).tobytes() == before
        d = scripted_step(rng, N, s, man, phi)
        junk = rng.normal(0, 1, shapes["commands"]).astype(np.float32)          # "the step" has reset robots and drawn commands
        mem.set(h["commands"], store(junk, layout)[0])
        for k in MANEUVER_FIELDS[1:]:
            mem.set(h[k], store(d[k], layout)[0])
        ref.accumulate(d)
        assert lib.go2nn_maneuver_accumulate(*args) == 0, lib.go2nn_last_error()
        commands_hold(s, junk, "accumulate")
    return mem.get(table).reshape(GO2NN_MANEUVER_NUM, N), ref, man


def check_table(table, ref, man, N, what):
    compare_tables(table, ref, what)
    r, e = ref.t, np.arange(N)
    assert (r[R["step"]] == START + CALLS).all() and (r[R["open"]] == 0).all()          # ... the last windows closed on the last step
    assert START + CALLS - 1 == SPECS[1]["segs"][-1][0] + SPECS[1]["window"] - 1 == SPECS[2]["segs"][-1][0] + SPECS[2]["window"] - 1
    alone = ~((man >= 0) & (man < len(SPECS)))
    assert (N == 1 or alone.sum() >= 1) and not table[1:, alone].any() and not table[1:, man == 0].any()          # left alone / no switch: only the step counter ran
    steps = ref.addends("win_lin_err")
    assert ((steps == 0) | (steps >= 2)).all()          # (the derivation of the bound)
    for m in (1, 2):          # every branch occurred, with the scripted outcome
        sw, W, H = len(SPECS[m]["segs"]) - 1, SPECS[m]["window"], SPECS[m]["hold"]
        of = lambda p: (man == m) & (e % PATTERNS == p)
        rows = lambda ids, *names: [r[R[n], ids] for n in names]
        assert (r[R["switches"], man == m] == sw).all() and (ref.closed[man == m] == sw).all()
        for p, (settled, steps_, falls, win) in {0: (sw, H * sw, 0, W * sw), 1: (sw, 2 * H * sw, 0, W * sw), 2: (0, 0, sw, 2 * sw), 3: (0, 0, sw, 0), 4: (sw, H * sw, 0, W * sw),
                                                 5: (sw, H * sw, sw, H * sw), 6: (0, 0, 0, W * sw)}.items():
            assert N < 63 or of(p).sum() >= 2, (m, p)          # from 63 envs on every (maneuver, pattern) pair has robots: none of the asserts below is vacuous
            for got, want in zip(rows(of(p), "settled", "settle_steps", "switch_falls", "win_steps"), (settled, steps_, falls, win)):
                assert (got == want).all(), (m, p, got, want)
    if N >= 17:
        seen = {int(p) for p in e[(man == 1) | (man == 2)] % PATTERNS}
        assert seen == set(range(PATTERNS)), seen


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 17, 300])
def test_apply_and_accumulate_against_float64(emu, N, layout):
    table, ref, man = run_script(emu, HostMemory(), N, layout)
    check_table(table, ref, man, N, "host N=%d layout=%d" % (N, layout))


def reduce_case(N, G, seed=9):
    rng = np.random.default_rng(seed + N)
    return lognormal_table(rng, GO2NN_MANEUVER_NUM, N), reduce_groups(rng, N, G)


def reduce_reference(table, group, G):
    out = np.zeros((G, GO2NN_MANEUVER_ACC_NUM + 1))
    mag = np.zeros_like(out)
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        out[g, GO2NN_MANEUVER_ACC_NUM] = mag[g, GO2NN_MANEUVER_ACC_NUM] = len(ids)
        for c in range(GO2NN_MANEUVER_ACC_NUM):
            row = table[GO2NN_MANEUVER_ACC_FIRST + c, ids]
            out[g, c], mag[g, c] = math.fsum(float(x) for x in row), math.fsum(abs(float(x)) for x in row)
    return out, mag


def check_reduce(out, table, group, G, N, what):
    """the group sizes exactly; every fp64 sum to N roundings of the running sum"""
    want, mag = reduce_reference(table, group, G)
    np.testing.assert_array_equal(out[:, GO2NN_MANEUVER_ACC_NUM], want[:, GO2NN_MANEUVER_ACC_NUM])
    gap, bound = np.abs(out - want), N * 2.0 ** -53 * mag
    assert (gap <= bound).all(), (gap.max(), bound.max())
    assert (out[1] == 0).all() and (group == 1).sum() == 0
    print("%s: largest reduce gap / bound %.3f" % (what, float((gap / np.maximum(bound, 1e-300)).max())))


@pytest.mark.parametrize("N,G", [(1, 3), (17, 3), (300, 5), (4096, 7)])
def test_reduce_against_fsum(emu, N, G):
    table, group = reduce_case(N, G)
    out = reduce_twice(lambda *a: emu.go2nn_maneuver_reduce(*a, None), table, group, G, GO2NN_MANEUVER_ACC_NUM + 1)
    check_reduce(out, table, group, G, N, "host N=%d" % N)


def test_check_specs(emu):
    good = dict(window=5, hold=2, thr_lin=0.3, thr_ang=0.3, segs=[(0, 1, 0, 0), (4, 0, 0, 0), (9, 0, 0, 1)])
    check = lambda dicts, M=None: emu.go2nn_maneuver_check_specs(C.cast(make_specs(dicts), C.c_void_p), len(dicts) if M is None else M)
    full = dict(good, window=1, hold=1, segs=[(k, 0, 0, 0) for k in range(GO2NN_MANEUVER_MAX_SEGS)])
    assert check([good]) == 0 and check([dict(good, segs=good["segs"][:1], window=1000)]) == 0 and check([full]) == 0 and check([good] * 64) == 0
    assert check([dict(good, segs=[(0, 1, 0, 0), (1, 0, 0, 0), (6, 0, 0, 1)])]) == 0          # the gap before the FIRST switch may be shorter than the window
    bad = {"count": [dict(good, count=0), dict(good, count=9), dict(good, count=-1)],
           "start[0]": [dict(good, segs=[(1, 1, 0, 0), (4, 0, 0, 0)]), dict(good, segs=[(-1, 1, 0, 0), (4, 0, 0, 0)])],
           "increasing": [dict(good, segs=[(0, 1, 0, 0), (4, 0, 0, 0), (4, 0, 0, 1)]), dict(good, segs=[(0, 1, 0, 0), (9, 0, 0, 0), (4, 0, 0, 1)]), dict(good, segs=[(0, 1, 0, 0), (0, 0, 0, 0)])],
           "hold": [dict(good, hold=0), dict(good, hold=-2), dict(good, window=1, hold=2), dict(good, window=0, hold=1)],
           "overlap": [dict(good, window=6), dict(good, segs=[(0, 1, 0, 0), (4, 0, 0, 0), (8, 0, 0, 1)])],
           "thr": [dict(good, thr_lin=0.0), dict(good, thr_ang=0.0), dict(good, thr_lin=-0.3), dict(good, thr_ang=float("nan")), dict(good, thr_lin=float("nan"))]}
    for word, cases in bad.items():
        for d in cases:
            assert check([good, d]) == EINVAL and b"maneuver spec 1" in emu.go2nn_last_error() and word.encode() in emu.go2nn_last_error(), (word, d, emu.go2nn_last_error())
    for M in (0, 65, -1):
        assert check([good], M) == EINVAL and b"M = " in emu.go2nn_last_error()
    assert emu.go2nn_maneuver_check_specs(None, 1) == EINVAL and emu.go2nn_last_error()


def test_argument_checks(emu):
    N = 4
    bufs = {k: np.zeros((N, max(w, 1)), np.uint8 if k.endswith("_buf") else np.float32) for k, w in WIDTH.items()}

    def make_in():
        a = Go2nnManeuverIn()
        for k in MANEUVER_FIELDS:
            f = getattr(a, k)
            f.p, f.env_stride, f.comp_stride = bufs[k].ctypes.data, max(WIDTH[k], 1), 1 if WIDTH[k] else 0
        a.num_specs, a.num_commands = 1, 4
        return a
    specs = make_specs([dict(window=5, hold=2, thr_lin=0.3, thr_ang=0.3, segs=[(0, 1, 0, 0)])])
    man, table, out = np.zeros(N, np.int32), np.zeros((GO2NN_MANEUVER_NUM, N), np.float32), np.zeros((2, GO2NN_MANEUVER_ACC_NUM + 1))
    p, sp = (lambda x: C.c_void_p(x.ctypes.data)), C.cast(specs, C.c_void_p)
    for fn in (emu.go2nn_maneuver_apply, emu.go2nn_maneuver_accumulate):
        assert fn(C.byref(make_in()), sp, p(man), p(table), N, None) == 0, emu.go2nn_last_error()
        for args in ((None, sp, p(man), p(table), N), (C.byref(make_in()), None, p(man), p(table), N), (C.byref(make_in()), sp, None, p(table), N),
                     (C.byref(make_in()), sp, p(man), None, N), (C.byref(make_in()), sp, p(man), p(table), 0), (C.byref(make_in()), sp, p(man), p(table), -1)):
            assert fn(*args, None) == EINVAL and emu.go2nn_last_error()

        def broken(edit):
            a = make_in()
            edit(a)
            return fn(C.byref(a), sp, p(man), p(table), N, None)
        for M in (0, 65, -1):
            assert broken(lambda a: setattr(a, "num_specs", M)) == EINVAL and b"num_specs" in emu.go2nn_last_error()
        assert broken(lambda a: setattr(a, "num_commands", 2)) == EINVAL and b"num_commands" in emu.go2nn_last_error()
        for field in MANEUVER_FIELDS:
            assert broken(lambda a: setattr(getattr(a, field), "p", None)) == EINVAL and b"null" in emu.go2nn_last_error(), field
            assert broken(lambda a: setattr(getattr(a, field), "env_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
            if WIDTH[field]:
                assert broken(lambda a: setattr(getattr(a, field), "comp_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
        assert broken(lambda a: setattr(a.reset_buf, "comp_stride", -1)) == EINVAL and b"stride" in emu.go2nn_last_error()
    assert emu.go2nn_maneuver_begin(None, N, 0, None) == EINVAL and emu.go2nn_maneuver_begin(p(table), 0, 0, None) == EINVAL and emu.go2nn_last_error()
    assert emu.go2nn_maneuver_begin(p(table), N, -2, None) == 0 and (table[0] == -2).all()
    assert emu.go2nn_maneuver_reduce(p(table), p(man), N, 2, p(out), None) == 0
    for args in ((None, p(man), N, 2, p(out)), (p(table), None, N, 2, p(out)), (p(table), p(man), N, 2, None), (p(table), p(man), 0, 2, p(out)),
                 (p(table), p(man), N, 0, p(out)), (p(table), p(man), N, 65536, p(out))):
        assert emu.go2nn_maneuver_reduce(*args, None) == EINVAL and emu.go2nn_last_error(), args[2:4]


def test_maneuver_symbols_and_structs_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7 and _nn.GO2NN_ABI_VERSION == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_maneuver_check_specs", "go2nn_maneuver_begin", "go2nn_maneuver_apply", "go2nn_maneuver_accumulate", "go2nn_maneuver_reduce"):
            assert (" T " + f + "\n") in syms, (path, f)
    spec_names, in_names = [n for n, _ in Go2nnManeuverSpec._fields_], [n for n, _ in Go2nnManeuverIn._fields_]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu %zu %d %d %d %d %d", sizeof(Go2nnManeuverSpec), sizeof(Go2nnManeuverIn), '
                   'GO2NN_MANEUVER_NUM, GO2NN_MANEUVER_ACC_FIRST, GO2NN_MANEUVER_ACC_NUM, GO2NN_MANEUVER_MAX_SPECS, GO2NN_MANEUVER_MAX_SEGS);\n'
                   + "".join('printf(" %%zu", offsetof(Go2nnManeuverSpec, %s));\n' % n for n in spec_names)
                   + "".join('printf(" %%zu", offsetof(Go2nnManeuverIn, %s));\n' % n for n in in_names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:7] == [C.sizeof(Go2nnManeuverSpec), C.sizeof(Go2nnManeuverIn), len(MANEUVER_ROWS), GO2NN_MANEUVER_ACC_FIRST, GO2NN_MANEUVER_ACC_NUM, _nn.GO2NN_MANEUVER_MAX_SPECS,
                       GO2NN_MANEUVER_MAX_SEGS] and got[5:7] == [64, 8]
    assert got[7:7 + len(spec_names)] == [getattr(Go2nnManeuverSpec, n).offset for n in spec_names]
    assert got[7 + len(spec_names):] == [getattr(Go2nnManeuverIn, n).offset for n in in_names]
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    enum = hdr[hdr.index("GO2NN_MANEUVER_STEP = 0"):hdr.index("GO2NN_MANEUVER_NUM\n")]
    assert [e.strip().split(" ")[0].replace("GO2NN_MANEUVER_", "").lower() for e in enum.split(",") if e.strip()] == list(MANEUVER_ROWS)
    assert MANEUVER_OUT == MANEUVER_ROWS[GO2NN_MANEUVER_ACC_FIRST:] + ("n",) and MANEUVER_ROWS[GO2NN_MANEUVER_ACC_FIRST] == "switches"
    assert "ADDED WITHIN ABI 7: five new entry points" in hdr[hdr.index("scripted command maneuvers"):]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# dt = 0.02 s: switches at counted steps 3 / 4 and 17 / 6, windows of 10 steps, a hold of 3; the horizon is 30 counted steps after 5 of warm-up
MANEUVERS = [["brake", [[0.0, 1.0, 0.0, 0.0], [0.06, 0.0, 0.0, 0.0]]], ["zigzag", [[0.0, 0.0, 0.5, 0.0], [0.08, 0.0, -0.5, 0.5], [0.34, 0.5, 0.0, -1.0]]],
             ["start", [[0.0, 0.0, 0.0, 0.0], [0.12, 1.0, 0.0, 0.0]]]]
SWITCH_STEPS = {"brake": [3], "zigzag": [4, 17], "start": [6]}
# (thr_lin [m/s], thr_ang [rad/s]): the fixed list the evaluator tests take their thresholds from: the first pair every recorded window error is at least MARGIN away from
THRESHOLDS = ((0.3, 0.3), (0.4, 0.4), (0.5, 0.6), (0.25, 0.35), (0.6, 0.8), (0.2, 0.2), (0.8, 1.0))
MAN = dict(num_envs=96, seconds=0.6, warmup_s=0.1, maneuvers=MANEUVERS, maneuver_window_s=0.2, maneuver_hold_s=0.06)
REC = ("commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "reset_buf", "time_out_buf")


def spec_dicts(thr, dt=0.02, window=10, hold=3):
    return [dict(window=window, hold=hold, thr_lin=thr[0], thr_ang=thr[1], segs=[(int(round(seg[0] / dt)),) + tuple(seg[1:4]) for seg in segs]) for _, segs in MANEUVERS]


def recompute(rec, ev, thr):
    """the whole maneuver table from the recorded buffers, in float64 -> Reference"""
    ref = Reference(ev.num_envs, -ev.warmup_steps, spec_dicts(thr), ev.man_host)
    for d in rec:
        ref.accumulate(d)
    return ref


def recorded_run(emu, ac, thr):
    rec, seen, text = [], [], io.StringIO()

    def cb(ev, k, counted):
        b = ev.env._buf
        rec.append({n: b[n].detach().clone().numpy() for n in REC})

    def applied(ev, k, counted):          # between go2nn_maneuver_apply and the step
        seen.append(ev.env._buf["commands"].detach().clone().numpy())
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    with contextlib.redirect_stdout(text):
        ev = PolicyEvaluator(env_cfg, dict(th.EVAL, maneuver_thr_lin=thr[0], maneuver_thr_ang=thr[1], **MAN), task_class=task_registry.get_task_class("go2_flat"), device="cpu",
                             lib=load_oracle(), nn_lib=emu, step_callback=cb, apply_callback=applied)
    res = ev.evaluate(ac)
    return dict(ev=ev, res=res, rec=rec, applied=seen, thr=thr, printed=text.getvalue(), mtable=ev.mtable.clone().numpy())


@pytest.fixture(scope="module")
def maneuver_run(emu):
    """ONE evaluation of go2_flat under MANEUVERS with the per-step buffers recorded.  The robots' motion does not depend on the thresholds (they only decide what is counted),
    so the pair is chosen on the first run's recording, by the float64 reference alone; a second evaluator is built only if that is not the list's first entry"""
    ac = th.small_actor_critic()
    run = recorded_run(emu, ac, THRESHOLDS[0])
    tried = [(thr, recompute(run["rec"], run["ev"], thr).closest) for thr in THRESHOLDS]
    chosen = [thr for thr, closest in tried if closest >= MARGIN][:1]
    if chosen and chosen[0] != THRESHOLDS[0]:
        run["ev"].close()
        run = recorded_run(emu, ac, chosen[0])
    run.update(ac=ac, tried=tried, chosen=chosen, ref=recompute(run["rec"], run["ev"], run["thr"]))
    yield run
    run["ev"].close()


def test_thresholds_away_from_every_recorded_error_were_found(maneuver_run):
    print("threshold candidates ((thr_lin, thr_ang), closest |err - thr| / thr): %s -> %s" % (["%s: %.2e" % t for t in maneuver_run["tried"]], maneuver_run["chosen"]))
    assert maneuver_run["chosen"] == [maneuver_run["thr"]] and maneuver_run["ref"].closest >= MARGIN, maneuver_run["tried"]


def test_evaluator_writes_the_schedule(maneuver_run):
    ev, rec, res = maneuver_run["ev"], maneuver_run["rec"], maneuver_run["res"]
    M, N = len(MANEUVERS), ev.num_envs
    assert ev.warmup_steps == 5 and ev.steps == 30 and len(rec) == 35 == len(maneuver_run["applied"]) and res["mode"] == "eager"
    assert res["terrain_names"] == ["plane"] and res["scenarios"] == [m[0] for m in MANEUVERS] == list(res["maneuvers"]) and ev.num_cells == M
    np.testing.assert_array_equal(ev.man_host, np.arange(N) % M)          # within a terrain kind the maneuvers are taken in turn: cell = terrain * M + maneuver
    np.testing.assert_array_equal(ev.cell_host, ev.man_host)
    assert res["switch_steps"] == SWITCH_STEPS and ev.maneuver_window == 10 and ev.maneuver_hold == 3
    dicts = spec_dicts(maneuver_run["thr"])
    changed = 0
    for k, (d, before) in enumerate(zip(rec, maneuver_run["applied"])):          # the command of step s holds from the apply before the step to the buffers the metrics read
        want, has = schedule(dicts, ev.man_host, k - ev.warmup_steps, d["commands"].shape[1])
        assert has.all() and d["commands"].tobytes() == want.tobytes() == before.tobytes(), k
        changed += k > 0 and want.tobytes() != schedule(dicts, ev.man_host, k - 1 - ev.warmup_steps, d["commands"].shape[1])[0].tobytes()
    assert changed == 4          # steps 3, 4, 6 and 17


def test_evaluator_maneuver_table_against_float64(maneuver_run):
    from go2_rl_gym_amd.utils.evaluator import MANEUVER_KEYS, RESULT_KEYS
    ev, res, ref = maneuver_run["ev"], maneuver_run["res"], maneuver_run["ref"]
    N, G, M = ev.num_envs, ev.num_cells, len(MANEUVERS)
    compare_tables(maneuver_run["mtable"], ref, "evaluator thr=%s" % (maneuver_run["thr"],))
    t = ref.t
    sw = np.asarray([len(SWITCH_STEPS[m[0]]) for m in MANEUVERS])[ev.man_host]
    assert (t[R["switches"]] == sw).all() and (ref.closed == sw).all() and (t[R["open"]] == 0).all() and (t[R["step"]] == ev.steps).all()
    print("settled %d of %d switches, %d switch falls, settle steps %s" % (t[R["settled"]].sum(), sw.sum(), t[R["switch_falls"]].sum(), sorted(set(t[R["settle_steps"]].tolist()))[:8]))
    # the reduce of the device table: counts exactly, the sums to the per-env bound carried through (n 2^-23 of every env's magnitude) plus the fp64 sum's N roundings
    want, mag = reduce_reference(t, ev.cell_host, G)
    got = res["maneuver_table"]
    assert got.shape == (G, GO2NN_MANEUVER_ACC_NUM + 1) and got[:, O["n"]].sum() == N
    for k in ("switches", "switch_falls", "settled", "settle_steps", "win_steps", "n"):
        np.testing.assert_array_equal(got[:, O[k]], want[:, O[k]], err_msg=k)
    for k in SUM_ROWS:
        n = ref.addends(k)
        per_env = n * 2.0 ** -23 * np.abs(t[R[k]])
        bound = np.asarray([per_env[ev.cell_host == g].sum() for g in range(G)]) + N * 2.0 ** -53 * mag[:, O[k]]
        assert (np.abs(got[:, O[k]] - want[:, O[k]]) <= bound).all(), k
    # the reported figures are those sums
    for mi, (name, _) in enumerate(MANEUVERS):
        cell, w = res["groups"]["plane"][name], got[mi]
        assert set(cell) == set(RESULT_KEYS) | set(MANEUVER_KEYS) and cell["n_envs"] == w[O["n"]] == N // M and cell["switches"] == w[O["switches"]] == len(SWITCH_STEPS[name]) * N // M
        assert cell["switch_falls"] == w[O["switch_falls"]] / w[O["switches"]] and cell["settled"] == w[O["settled"]] / w[O["switches"]]
        assert cell["settle_time_s"] == w[O["settle_steps"]] / w[O["settled"]] * ev.dt if w[O["settled"]] > 0 else math.isnan(cell["settle_time_s"])
        assert cell["window_lin_vel_err"] == w[O["win_lin_err"]] / w[O["win_steps"]] and cell["window_ang_vel_err"] == w[O["win_ang_err"]] / w[O["win_steps"]]
        assert cell["peak_tilt"] == w[O["peak_tilt_sum"]] / w[O["switches"]] and 0 <= cell["peak_tilt"] <= 1
        assert str(res["maneuvers"][name]) == str(cell)          # (one terrain kind: the maneuver over the terrains is its one cell)
    whole = got.sum(0)
    assert res["overall"]["switches"] == whole[O["switches"]] == sw.sum() and res["overall"]["settled"] == whole[O["settled"]] / whole[O["switches"]]
    assert res["overall"]["n_envs"] == N and set(res["overall"]) == set(RESULT_KEYS) | set(MANEUVER_KEYS)
    row = ev._maneuver_row(np.zeros(GO2NN_MANEUVER_ACC_NUM + 1))          # no switch at all: NaN, not a division by zero
    assert row["switches"] == 0 and all(math.isnan(row[k]) for k in MANEUVER_KEYS if k != "switches")


def test_evaluator_warnings_and_outputs(emu, maneuver_run, capsys):
    from go2_rl_gym_amd.utils.evaluator import MANEUVER_KEYS, RESULT_KEYS, format_table, results_dict, scalars
    ev, res = maneuver_run["ev"], maneuver_run["res"]
    assert "fewer than 4 robots" not in maneuver_run["printed"]          # 32 robots per cell
    capsys.readouterr()
    small = th.make_evaluator(emu, **dict(MAN, num_envs=8))
    assert "(terrain x maneuver) cells have fewer than 4 robots (smallest: 2)" in capsys.readouterr().out
    small.close()
    tags = dict(scalars(res))
    for name, _ in MANEUVERS:
        for k in RESULT_KEYS + MANEUVER_KEYS:
            got, want = tags["Eval/maneuver/%s/%s" % (name, k)], res["maneuvers"][name][k]
            assert got == want or (math.isnan(got) and math.isnan(want)), (name, k)
    assert "Eval/lin_vel_err" in tags and "Eval/plane/brake/tilt" in tags
    rd = yaml.safe_load(yaml.safe_dump(results_dict(res, 3)))
    assert set(rd["maneuvers"]) == {m[0] for m in MANEUVERS} and set(rd["maneuvers"]["brake"]) == set(RESULT_KEYS) | set(MANEUVER_KEYS) == set(rd["groups"]["plane"]["brake"])
    assert rd["maneuver_schedule"] == {"brake": [[0, 1.0, 0.0, 0.0], [3, 0.0, 0.0, 0.0]], "zigzag": [[0, 0.0, 0.5, 0.0], [4, 0.0, -0.5, 0.5], [17, 0.5, 0.0, -1.0]],
                                       "start": [[0, 0.0, 0.0, 0.0], [6, 1.0, 0.0, 0.0]]}
    assert rd["maneuver_rule"] == {"window": 10, "hold": 3, "thr_lin": maneuver_run["thr"][0], "thr_ang": maneuver_run["thr"][1]} and rd["iteration"] == 3
    text = format_table(res)
    print(text)
    block = text.split("\n\n")[-1].splitlines()
    assert len(text.split("\n\n")) == 2 and block[0].split() == ["maneuver", "lin_vel_err", "ang_vel_err", "falls", "survival"] + list(MANEUVER_KEYS) + ["n_envs"]
    assert [l.split()[0] for l in block[1:]] == [m[0] for m in MANEUVERS] + ["all"]


def test_recorded_trace_carries_the_schedule(emu):
    ev = th.make_evaluator(emu, record=2, **MAN)
    trace = ev.evaluate(th.small_actor_critic())["trace"]
    pad = lambda steps: steps + [-1] * (GO2NN_MANEUVER_MAX_SEGS - 1 - len(steps))
    assert trace["maneuvers"] == [m[0] for m in MANEUVERS] and trace["switch_steps"].dtype == np.int32
    assert trace["switch_steps"].tolist() == [pad(SWITCH_STEPS[m[0]]) for m in MANEUVERS] == [pad([3]), pad([4, 17]), pad([6])]          # unequal switch counts
    np.testing.assert_array_equal(trace["maneuver_of_robot"], ev.man_host[trace["env_ids"]])
    assert sorted(trace["maneuver_of_robot"].tolist()) == [0, 0, 1, 1, 2, 2]
    cmd = trace["frames"][:, :, _nn.TRACE_OFFSET["commands"]:_nn.TRACE_OFFSET["commands"] + 3]          # the frame of a switch step carries the new command
    dicts = spec_dicts((0.3, 0.3))
    for s in range(ev.steps):
        np.testing.assert_array_equal(cmd[s], schedule(dicts, trace["maneuver_of_robot"], s)[0][:, :3])
    ev.close()


def test_a_trace_with_unequal_switch_counts_goes_through_the_file(emu, tmp_path):
    """write_results (what the training loop and scripts/evaluate.py --record call) and read_trace: the schedule comes back as it went in"""
    from go2_rl_gym_amd.utils.evaluator import write_results
    from go2_rl_gym_amd.utils.recorder import read_trace
    ev = th.make_evaluator(emu, record=1, **MAN)
    res = ev.evaluate(th.small_actor_critic())
    ev.close()
    out = write_results(str(tmp_path), 7, res)
    assert yaml.safe_load(open(out))["maneuver_schedule"]["zigzag"][2] == [17, 0.5, 0.0, -1.0]
    back = read_trace(os.path.join(str(tmp_path), "eval_results", "trace_7.npz"))
    trace = res["trace"]
    assert back["maneuvers"] == [m[0] for m in MANEUVERS] and back["switch_steps"].dtype == np.int32 and back["switch_steps"].shape == (3, GO2NN_MANEUVER_MAX_SEGS - 1)
    np.testing.assert_array_equal(back["switch_steps"], trace["switch_steps"])
    np.testing.assert_array_equal(back["maneuver_of_robot"], trace["maneuver_of_robot"])
    np.testing.assert_array_equal(back["frames"], trace["frames"])
    assert [[s for s in row if s >= 0] for row in back["switch_steps"].tolist()] == [[3], [4, 17], [6]]


def test_a_metric_that_does_not_exist_ranks_last():
    from go2_rl_gym_amd.scripts.evaluate import best_checkpoint
    nan = float("nan")
    rows = [{"checkpoint": c, "overall": {"settle_time_s": t, "settled": s}} for c, t, s in (("a", nan, 0.0), ("b", 0.8, 0.5), ("c", 0.6, nan), ("d", nan, 0.7))]
    for order in (rows, rows[::-1], rows[1:] + rows[:1]):
        assert best_checkpoint(order, "settle_time_s")["checkpoint"] == "c" and best_checkpoint(order, "settled")["checkpoint"] == "d"


def test_evaluator_is_reproducible(maneuver_run):
    """(after the tests that look at the first evaluation's simulator) the same weights: byte-identical tables; other weights: another result"""
    ev, res, ac = maneuver_run["ev"], maneuver_run["res"], maneuver_run["ac"]
    again = ev.evaluate(ac)
    assert again["table"].tobytes() == res["table"].tobytes() and again["maneuver_table"].tobytes() == res["maneuver_table"].tobytes()
    assert str(again["groups"]) == str(res["groups"]) and str(again["maneuvers"]) == str(res["maneuvers"]) and ev.mtable.numpy().tobytes() == maneuver_run["mtable"].tobytes()
    other = ev.evaluate(th.small_actor_critic(1))
    assert other["table"].tobytes() != res["table"].tobytes() and other["maneuver_table"].tobytes() != res["maneuver_table"].tobytes()
    assert other["maneuver_table"][:, O["switches"]].tobytes() == res["maneuver_table"][:, O["switches"]].tobytes()          # (the schedule does not depend on the weights)


def test_one_segment_maneuvers_are_the_scenarios(emu):
    """a maneuver of one segment per scenario: the command never changes, and the evaluation is the plain one, byte for byte — the two kernels write what the copy wrote"""
    ac = th.small_actor_critic()
    plain = th.make_evaluator(emu)
    res0 = plain.evaluate(ac)
    plain.close()
    one = th.make_evaluator(emu, maneuvers=[[s[0], [[0.0] + list(s[1:4])]] for s in th.EVAL["scenarios"]])
    res1 = one.evaluate(ac)
    assert res1["table"].tobytes() == res0["table"].tobytes() and res1["scenarios"] == res0["scenarios"]
    assert not res1["maneuver_table"][:, :GO2NN_MANEUVER_ACC_NUM].any() and res1["overall"]["switches"] == 0 and math.isnan(res1["overall"]["settled"])
    for s in th.EVAL["scenarios"]:
        assert {k: res1["groups"]["plane"][s[0]][k] for k in res0["groups"]["plane"][s[0]]} == res0["groups"]["plane"][s[0]]
    one.close()


def test_maneuvers_off_change_nothing(emu):
    """maneuvers = None: no maneuver key in the result, nothing allocated, and the table of an evaluator whose config never heard of maneuvers, byte for byte"""
    ac = th.small_actor_critic()
    plain = th.make_evaluator(emu)
    assert not any(k.startswith("maneuver") for k in th.EVAL)
    res0 = plain.evaluate(ac)
    plain.close()
    off = th.make_evaluator(emu, maneuvers=None, maneuver_window_s=0.1, maneuver_hold_s=0.04, maneuver_thr_lin=0.1, maneuver_thr_ang=0.1)
    res1 = off.evaluate(ac)
    assert res1["table"].tobytes() == res0["table"].tobytes() and str(res1["groups"]) == str(res0["groups"]) and str(res1["overall"]) == str(res0["overall"])
    assert set(res1) == set(res0) and not any("maneuver" in k or "switch" in k for k in res1) and "switches" not in res1["overall"]
    assert off.maneuvers is None and not any(hasattr(off, k) for k in ("mtable", "mout", "mspecs", "man", "man_host"))
    off.close()
    for task in ("go2_cts", "go2"):
        _, fresh = task_registry.get_cfgs(task)
        e = fresh.evaluation
        assert (e.maneuvers, e.maneuver_window_s, e.maneuver_hold_s, e.maneuver_thr_lin, e.maneuver_thr_ang) == (None, 3.0, 0.3, 0.3, 0.3)


def test_maneuver_configuration_errors(emu):
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_MANEUVERS
    two = [[0.0, 1.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0]]
    with pytest.raises(ValueError, match="cannot be combined"):
        th.make_evaluator(emu, maneuvers=MANEUVERS, perturbations=[["nominal", {}]])
    with pytest.raises(ValueError, match="cannot be combined"):
        th.make_evaluator(emu, task="go2", maneuvers=MANEUVERS, ladder=True)
    with pytest.raises(ValueError, match="distinct names"):
        th.make_evaluator(emu, maneuvers=[["a", two], ["a", two]])
    with pytest.raises(ValueError, match="at most 64 maneuvers, got 65"):
        th.make_evaluator(emu, maneuvers=[["m%d" % k, two] for k in range(65)])
    with pytest.raises(ValueError, match="segments"):
        th.make_evaluator(emu, maneuvers=[["long", [[0.02 * k, 0.0, 0.0, 0.0] for k in range(9)]]])
    with pytest.raises(ValueError, match="first segment"):
        th.make_evaluator(emu, maneuvers=[["late", [[0.1, 1.0, 0.0, 0.0]]]])
    with pytest.raises(ValueError, match="must increase"):
        th.make_evaluator(emu, maneuvers=[["back", [[0.0, 1.0, 0.0, 0.0], [0.4, 0.0, 0.0, 0.0], [0.4, 1.0, 0.0, 0.0]]]], maneuver_window_s=0.1, maneuver_hold_s=0.04)
    for over in (dict(maneuver_window_s=0.2), dict(maneuver_window_s=0.2, maneuver_hold_s=0.1, maneuver_thr_lin=0.0), dict(maneuver_window_s=0.2, maneuver_hold_s=0.1, maneuver_thr_ang=-1.0)):
        with pytest.raises(ValueError, match="maneuver_window_s"):          # (the default hold of 0.3 s is longer than that window)
            th.make_evaluator(emu, maneuvers=[["a", two]], **over)
    short = dict(maneuver_window_s=0.2, maneuver_hold_s=0.1)
    # th.EVAL: 1 s = 50 counted steps.  The window of a switch closes inside its segment and inside the horizon, or the configuration is refused
    ok = th.make_evaluator(emu, maneuvers=[["a", [[0.0, 1.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0], [0.8, 0.0, 0.0, 1.0]]]], **short)          # 40 + 10 = 50: on the last step
    assert ok.switch_steps == {"a": [10, 40]} and ok.maneuver_window == 10
    ok.close()
    with pytest.raises(ValueError, match="horizon's end"):
        th.make_evaluator(emu, maneuvers=[["a", [[0.0, 1.0, 0.0, 0.0], [0.82, 0.0, 0.0, 0.0]]]], **short)
    with pytest.raises(ValueError, match="the next switch"):
        th.make_evaluator(emu, maneuvers=[["a", [[0.0, 1.0, 0.0, 0.0], [0.2, 0.0, 0.0, 0.0], [0.3, 0.0, 0.0, 1.0]]]], **short)
    with pytest.raises(ValueError, match="horizon's end"):          # the defaults are made for the default 10 s horizon, not for th.EVAL's 1 s
        th.make_evaluator(emu, maneuvers=DEFAULT_MANEUVERS)
    args = get_args(["--task", "go2", "--maneuvers"])
    assert args.maneuvers is True and get_args(["--task", "go2"]).maneuvers is False
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), get_args(["--task", "go2_flat", "--maneuvers"]))
    assert cfg.evaluation.maneuvers == DEFAULT_MANEUVERS and cfg.evaluation.maneuvers is not DEFAULT_MANEUVERS and train_cfg.evaluation.maneuvers is None
    assert [m[0] for m in DEFAULT_MANEUVERS] == ["start_1.0", "brake_1.0", "brake_2.0", "reverse_1.0", "sidestep_flip_0.5", "turn_flip_1.0", "walk_into_turn_1.0"]
    assert all(len(segs) == 2 and segs[0][0] == 0.0 and segs[1][0] == 5.0 for _, segs in DEFAULT_MANEUVERS)


def test_cli_names_the_checkpoint_that_falls_least(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints --maneuvers --metric switch_falls (lower is better)"""
    from go2_rl_gym_amd.scripts.evaluate import HIGHER_IS_BETTER, evaluate
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_MANEUVERS, MANEUVER_KEYS
    assert "settled" in HIGHER_IS_BETTER and "switch_falls" not in HIGHER_IS_BETTER and "settle_time_s" not in HIGHER_IS_BETTER
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s, e.maneuver_window_s, e.maneuver_hold_s = 28, 0.4, 0.1, 0.1, 0.04
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    short = [[n, [[0.0] + segs[0][1:], [0.2] + segs[1][1:]]] for n, segs in DEFAULT_MANEUVERS]          # the default maneuvers, switching at 0.2 s of the 0.4 s horizon
    from go2_rl_gym_amd.utils import evaluator as E
    monkeypatch.setattr(E, "DEFAULT_MANEUVERS", short)
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    capsys.readouterr()
    out = evaluate(base + ["--maneuvers", "--all_checkpoints", "--metric", "switch_falls"], log_root=str(tmp_path), env_kwargs={"lib": load_oracle()},
                   evaluator_kwargs={"nn_lib": emu})
    names = [r["checkpoint"] for r in out["checkpoints"]]
    assert names == ["model_0.pt", "model_1.pt"] and out["metric"] == "switch_falls" and out["best"] in names
    assert out["best_value"] == min(r["overall"]["switch_falls"] for r in out["checkpoints"]) and 0 <= out["best_value"] <= 1
    for r in out["checkpoints"]:
        assert list(r["maneuvers"]) == [m[0] for m in DEFAULT_MANEUVERS] and all(set(MANEUVER_KEYS) <= set(v) for v in r["maneuvers"].values())
        assert r["overall"]["switches"] == 28 and all(v["switches"] == 4 for v in r["maneuvers"].values())
    text = capsys.readouterr().out
    assert "maneuver " in text and "settle_time_s" in text and json.loads([l for l in text.splitlines() if l.startswith("{")][-1])["best"] == out["best"]
