"""The evaluator's perturbations on the CPU: the host build of the go2nn_robust_* kernels (include/go2nn.h) against a float64 restatement written here over a scripted
sequence in which the envs meet every branch, the reduce against math.fsum, the argument checks, the struct layouts, and PolicyEvaluator with `perturbations` on the oracle +
the host build: the push itself, the dynamics rows after a reset, reproducibility, the results' shape, and its isolation from a training run."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, load_nn_emu, load_oracle, lognormal_table, reduce_groups, reduce_twice
import test_eval_host as th
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import GO2NN_ROBUST_ACC_FIRST, GO2NN_ROBUST_ACC_NUM, GO2NN_ROBUST_NUM, ROBUST_FIELDS, ROBUST_MASK, ROBUST_ROWS, Go2nnRobustIn, Go2nnRobustSpec
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.utils import get_args

U = 2.0 ** -24
R = {n: i for i, n in enumerate(ROBUST_ROWS)}
WIDTH = {"root_states": 13, "commands": 4, "base_lin_vel": 3, "projected_gravity": 3, "reset_buf": 0, "time_out_buf": 0, "motor_strengths": 12, "p_gains_multiplier": 12,
         "d_gains_multiplier": 12, "added_base_mass": 0, "friction_coeffs": 0}
DYN = {"strength": "motor_strengths", "kp_mul": "p_gains_multiplier", "kd_mul": "d_gains_multiplier", "added_mass": "added_base_mass", "friction": "friction_coeffs"}
COUNTER_ROWS = ("step", "open", "ok_run", "done", "pushes", "push_falls", "recovered", "recovery_steps")
FLOAT_ROWS = ("peak_err", "peak_tilt", "peak_err_sum", "peak_tilt_sum")
START, CALLS = -9, 40
# spec 0: pushes at 3 and 15 (a third one would come at 27: count exhausted), windows 3..12 and 15..24; spec 1: pushes at 0 and 9 — the first call has STEP = -9, where
# (s - first) % period == 0 in C's arithmetic: only s >= first keeps it from firing; spec 2: never pushes, writes nothing
SPECS = [dict(dv=(0.5, -0.25, 0.1), first=3, period=12, count=2, window=10, hold=3, thr=0.3, strength=0.8, added_mass=3.0),
         dict(dv=(0.0, 1.0, 0.0), first=0, period=9, count=2, window=9, hold=2, thr=0.5, kp_mul=0.9, kd_mul=1.25, friction=0.3),
         dict(dv=(1.0, 1.0, 1.0), first=0, period=5, count=0, window=5, hold=1, thr=0.3)]


def make_specs(dicts):
    specs = (Go2nnRobustSpec * len(dicts))()
    for sp, d in zip(specs, dicts):
        sp.dv[:] = d["dv"]
        sp.first, sp.period, sp.count, sp.window, sp.hold, sp.thr = d["first"], d["period"], d["count"], d["window"], d["hold"], d["thr"]
        sp.strength, sp.kp_mul, sp.kd_mul, sp.added_mass, sp.friction = 1.0, 1.0, 1.0, 0.0, 1.0
        for k, bit in ROBUST_MASK.items():
            if k in d:
                setattr(sp, k, d[k])
                sp.mask |= bit
    return specs


def pert_of(N):
    p = (np.arange(N) % 3).astype(np.int32)
    p[np.arange(N) % 17 == 15] = -1          # outside [0, P) on either side: the env is left alone
    p[np.arange(N) % 17 == 16] = 5
    return p


def scripted_step(rng, N, s):
    """what the simulator shows after step s, by the env's pattern e % 5 (crossed with the perturbation e % 3):  0 tracks at once (recovers after `hold` steps);  1 never
    tracks (the window ends unrecovered);  2 never tracks and FALLS at s % 12 == 7, inside the windows, with a time-out reset (not a fall) at s % 12 == 5;  3 dips below
    thr for 2 steps (hold - 1 of spec 0), rises for 3, then tracks (a late recovery);  4 random, 0.05 away from either thr, random falls.  -> {field: array}"""
    e = np.arange(N)
    k, m = e % 5, s % 12
    err = np.where(k == 0, 0.05, 0.9)
    err = np.where((k == 3) & np.isin(m, (4, 5, 9, 10, 11)), 0.1, err)
    lo = rng.random(N) < 0.5
    err = np.where(k == 4, np.where(lo, rng.uniform(0.0, 0.25, N), rng.uniform(0.55, 1.5, N)), err)
    phi = rng.uniform(-np.pi, np.pi, N)
    d = {"commands": rng.normal(0, 1, (N, 4)).astype(np.float32), "projected_gravity": rng.normal(0, 0.3, (N, 3)).astype(np.float32)}
    v = rng.normal(0, 1, (N, 3))
    v[:, 0], v[:, 1] = d["commands"][:, 0] - err * np.cos(phi), d["commands"][:, 1] - err * np.sin(phi)
    d["base_lin_vel"] = v.astype(np.float32)
    reset = ((k == 2) & ((m == 7) | (m == 5))) | ((k == 4) & (rng.random(N) < 0.05))
    d["reset_buf"] = reset.astype(np.uint8)
    d["time_out_buf"] = ((k == 2) & (m == 5)).astype(np.uint8)
    root = rng.normal(0, 1, (N, 13))
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    root[e % 11 == 4, 3:7] = (0.0, math.sqrt(0.5), 0.0, math.sqrt(0.5))          # nose straight up: the heading is undefined -> (1, 0)
    d["root_states"] = root.astype(np.float32)
    return d


class Reference:
    """the table of include/go2nn.h in float64, one env at a time"""

    def __init__(self, N, start, specs, pert):
        self.N, self.specs, self.pert = N, specs, pert
        self.t = np.zeros((GO2NN_ROBUST_NUM, N))
        self.t[R["step"]] = start

    def apply(self, bufs):
        """bufs: {field: logical fp32 array}, modified in place -> {env: |terms| of the three velocity sums} for the pushed envs"""
        pushed = {}
        for e in range(self.N):
            p = self.pert[e]
            if not 0 <= p < len(self.specs):
                continue
            sp = self.specs[p]
            for k, f in DYN.items():
                if k in sp:
                    bufs[f][e] = np.float32(sp[k])
            s = int(self.t[R["step"], e])
            if not (sp["count"] > 0 and s >= sp["first"] and (s - sp["first"]) % sp["period"] == 0 and (s - sp["first"]) // sp["period"] < sp["count"]):
                continue
            x, y, z, w = (float(q) for q in bufs["root_states"][e, 3:7])
            c, sn = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z)
            n = math.hypot(c, sn)
            c, sn = (1.0, 0.0) if n < 1e-6 else (c / n, sn / n)
            dv = [float(np.float32(a)) for a in sp["dv"]]
            v = bufs["root_states"][e, 7:10].astype(np.float64)
            add = np.array([c * dv[0] - sn * dv[1], sn * dv[0] + c * dv[1], dv[2]])
            pushed[e] = (v + add, np.abs(v) + np.array([abs(c * dv[0]) + abs(sn * dv[1]), abs(sn * dv[0]) + abs(c * dv[1]), abs(dv[2])]))
            t = self.t[:, e]
            t[R["open"]], t[R["peak_err"]], t[R["peak_tilt"]], t[R["ok_run"]], t[R["done"]] = 1, 0, 0, 0, 0
            t[R["pushes"]] += 1
        return pushed

    def accumulate(self, d):
        f = {k: np.asarray(v, np.float64) for k, v in d.items()}
        for e in range(self.N):
            t, p = self.t[:, e], self.pert[e]
            if 0 <= p < len(self.specs) and t[R["open"]] > 0:
                sp = self.specs[p]
                if t[R["done"]] == 0:
                    err = math.hypot(f["commands"][e, 0] - f["base_lin_vel"][e, 0], f["commands"][e, 1] - f["base_lin_vel"][e, 1])
                    assert abs(err - float(np.float32(sp["thr"]))) > 0.01          # the script keeps every comparison with thr away from rounding
                    t[R["peak_err"]] = max(t[R["peak_err"]], err)
                    t[R["peak_tilt"]] = max(t[R["peak_tilt"]], math.hypot(f["projected_gravity"][e, 0], f["projected_gravity"][e, 1]))
                    if d["reset_buf"][e] and not d["time_out_buf"][e]:
                        t[R["push_falls"]] += 1
                        t[R["done"]] = 1
                    elif err < sp["thr"]:
                        t[R["ok_run"]] += 1
                        if t[R["ok_run"]] == sp["hold"]:
                            t[R["recovered"]] += 1
                            t[R["recovery_steps"]] += t[R["open"]]
                            t[R["done"]] = 1
                    else:
                        t[R["ok_run"]] = 0
                if t[R["open"]] == sp["window"]:
                    t[R["peak_err_sum"]] += t[R["peak_err"]]
                    t[R["peak_tilt_sum"]] += t[R["peak_tilt"]]
                    t[R["open"]] = 0
                else:
                    t[R["open"]] += 1
            t[R["step"]] += 1


def store(a, layout):
    """a logical [N, w] (or [N]) array as the libraries store it -> (flat storage, env stride, component stride)"""
    if a.ndim == 1:
        return np.ascontiguousarray(a), 1, 0
    if layout == 1:
        return np.ascontiguousarray(a.T), 1, a.shape[0]
    return np.ascontiguousarray(a), a.shape[1], 1


def logical(flat, shape, layout):
    return flat.reshape(shape[::-1]).T if (layout == 1 and len(shape) > 1) else flat.reshape(shape)


class HostMemory:
    """where the kernels' buffers live: numpy here, torch device tensors in tests/test_gpu_robust.py"""
    stream = None

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return np.array(h, copy=True)

    def set(self, h, a):
        h.reshape(-1)[:] = np.ascontiguousarray(a).reshape(-1)


def run_script(lib, mem, N, layout, seed=0):
    """the scripted sequence on `lib` with its buffers in `mem`, checked call by call against the Reference -> (table fp32 [NUM, N], reference table)"""
    rng = np.random.default_rng(seed + N)
    pert, specs = pert_of(N), make_specs(SPECS)
    assert lib.go2nn_robust_check_specs(C.cast(specs, C.c_void_p), len(SPECS)) == 0, lib.go2nn_last_error()
    ref = Reference(N, START, SPECS, pert)
    shapes = {k: ((N, w) if w else (N,)) for k, w in WIDTH.items()}
    dyn0 = {f: rng.uniform(0.5, 1.5, shapes[f]).astype(np.float32) for f in DYN.values()}
    bufs = {k: (np.zeros(shapes[k], np.uint8) if k.endswith("_buf") else dyn0[k].copy() if k in dyn0 else np.zeros(shapes[k], np.float32)) for k in ROBUST_FIELDS}
    a, h = Go2nnRobustIn(), {}
    for k in ROBUST_FIELDS:
        flat, es, cs = store(bufs[k], layout)
        h[k] = mem.put(flat)
        f = getattr(a, k)
        f.p, f.env_stride, f.comp_stride = mem.ptr(h[k]), es, cs
    a.num_specs = len(SPECS)
    table = mem.put(np.full((GO2NN_ROBUST_NUM, N), 7.0, np.float32))
    specs_h = mem.put(np.frombuffer(bytes(specs), np.uint8))
    pert_h = mem.put(pert)
    args = (C.byref(a), C.c_void_p(mem.ptr(specs_h)), C.c_void_p(mem.ptr(pert_h)), C.c_void_p(mem.ptr(table)), N, mem.stream)
    assert lib.go2nn_robust_begin(C.c_void_p(mem.ptr(table)), N, START, mem.stream) == 0, lib.go2nn_last_error()
    pushes_seen, worst = 0, 0.0
    for call in range(CALLS):
        s = START + call
        d = scripted_step(rng, N, s)
        bufs["root_states"] = d["root_states"].copy()          # "the simulator" has moved the robot since the last call
        if call == 20:          # ... and a reset has redrawn some envs' dynamics rows
            for f in DYN.values():
                bufs[f][::4] = np.float32(1.0)
        for k in ["root_states"] + list(DYN.values()):
            mem.set(h[k], store(bufs[k], layout)[0])
        before = {k: bufs[k].copy() for k in DYN.values()}
        pushed = ref.apply(bufs)
        assert lib.go2nn_robust_apply(*args) == 0, lib.go2nn_last_error()
        for f in DYN.values():          # the masked rows hold the spec's values, every other row is bit-for-bit what it was
            got = logical(mem.get(h[f]), shapes[f], layout)
            np.testing.assert_array_equal(got, bufs[f], err_msg="%s at step %d" % (f, s))
        spec_of_row = {f: k for k, f in DYN.items()}
        for f in DYN.values():
            for e in range(N):
                if not (0 <= pert[e] < len(SPECS) and spec_of_row[f] in SPECS[pert[e]]):
                    assert np.array_equal(bufs[f][e], before[f][e])
        got = logical(mem.get(h["root_states"]), shapes["root_states"], layout).astype(np.float64)
        want = d["root_states"].astype(np.float64)
        for e, (v, mag) in pushed.items():
            gap, bound = np.abs(got[e, 7:10] - v), th.accumulate_bound(32, mag)
            worst = max(worst, float((gap / bound).max()))
            assert (gap <= bound).all(), (s, e, got[e, 7:10], v)
            want[e, 7:10] = got[e, 7:10]
        np.testing.assert_array_equal(got, want)          # nothing but the pushed envs' velocity has moved
        pushes_seen += len(pushed)
        for k in ("commands", "base_lin_vel", "projected_gravity", "reset_buf", "time_out_buf"):
            mem.set(h[k], store(d[k], layout)[0])
        ref.accumulate(d)
        assert lib.go2nn_robust_accumulate(*args) == 0, lib.go2nn_last_error()
    print("N=%d layout=%d: %d pushes, largest push gap / bound %.3f" % (N, layout, pushes_seen, worst))
    return mem.get(table).reshape(GO2NN_ROBUST_NUM, N), ref.t, pert


def check_table(table, ref, pert, N, what):
    t = table.astype(np.float64)
    for r in COUNTER_ROWS:
        np.testing.assert_array_equal(t[R[r]], ref[R[r]], err_msg=r)
    assert (ref[R["step"]] == START + CALLS).all()
    alone = ~((pert >= 0) & (pert < len(SPECS)))
    assert alone.sum() >= 2 and not t[1:, alone].any() and not t[1:, pert == 2].any()          # left alone / never pushed: only the step counter ran
    e = np.arange(N)
    p0, p1 = (pert == 0), (pert == 1)
    assert (ref[R["pushes"], p0 | p1] == 2).all()
    # every branch occurred: recovered at once (OPEN = hold), late after a dip of hold - 1 steps (spec 0: at the 9th step), unrecovered windows, falls inside a window
    assert (ref[R["recovery_steps"], p0 & (e % 5 == 0)] == 2 * 3).all() and (ref[R["recovery_steps"], p1 & (e % 5 == 0)] == 2 * 2).all()
    if (p0 & (e % 5 == 3)).any():
        assert (ref[R["recovered"], p0 & (e % 5 == 3)] >= 1).all() and (ref[R["recovery_steps"], p0 & (e % 5 == 3)] >= 9).all()
    assert (ref[R["recovered"], (p0 | p1) & (e % 5 == 1)] == 0).all() and (ref[R["push_falls"], (p0 | p1) & (e % 5 == 1)] == 0).all()
    assert (ref[R["push_falls"], p0 & (e % 5 == 2)] == 2).all() and (ref[R["push_falls"], p1 & (e % 5 == 2)] >= 1).all()
    assert (ref[R["open"]] == 0).all() and (ref[R["peak_err_sum"], p0 | p1] > 0).all()
    ratio = {r: np.abs(t[R[r]] - ref[R[r]]) / np.maximum(th.accumulate_bound(32, np.abs(ref[R[r]])), 1e-300) for r in FLOAT_ROWS}
    print("%s: largest |table - ref| / bound: %s" % (what, ", ".join("%s %.3f" % (r, v.max()) for r, v in ratio.items())))
    for r, v in ratio.items():
        assert (v <= 1.0).all(), (r, float(v.max()))


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [17, 300])
def test_apply_and_accumulate_against_float64(emu, N, layout):
    table, ref, pert = run_script(emu, HostMemory(), N, layout)
    check_table(table, ref, pert, N, "host N=%d layout=%d" % (N, layout))


def reduce_case(N, G, seed=5):
    rng = np.random.default_rng(seed + N)
    return lognormal_table(rng, GO2NN_ROBUST_NUM, N), reduce_groups(rng, N, G)


def check_reduce(out, table, group, G, N, what):
    worst = 0.0
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        assert out[g, GO2NN_ROBUST_ACC_NUM] == len(ids)
        for c in range(GO2NN_ROBUST_ACC_NUM):
            row = table[GO2NN_ROBUST_ACC_FIRST + c, ids]
            want, mag = math.fsum(float(x) for x in row), math.fsum(abs(float(x)) for x in row)
            assert abs(out[g, c] - want) <= N * 2.0 ** -53 * mag, (g, c, out[g, c], want)
            worst = max(worst, abs(out[g, c] - want) / max(N * 2.0 ** -53 * mag, 1e-300))
    assert (out[1] == 0).all() and (group == 1).sum() == 0
    print("%s: largest reduce gap / bound %.3f" % (what, worst))


@pytest.mark.parametrize("N,G", [(17, 3), (300, 5), (4096, 7)])
def test_reduce_against_fsum(emu, N, G):
    table, group = reduce_case(N, G)
    out = reduce_twice(lambda *a: emu.go2nn_robust_reduce(*a, None), table, group, G, GO2NN_ROBUST_ACC_NUM + 1)
    check_reduce(out, table, group, G, N, "host N=%d" % N)


def test_argument_checks(emu):
    good = dict(dv=(0, 0, 0), first=0, period=10, count=2, window=5, hold=2, thr=0.3)
    check = lambda dicts, P=None: emu.go2nn_robust_check_specs(C.cast(make_specs(dicts), C.c_void_p), len(dicts) if P is None else P)
    assert check([good]) == 0 and check([dict(good, count=0, window=0, period=0)]) == 0          # without pushes window and period are not looked at
    for bad in (dict(good, window=0), dict(good, window=11), dict(good, hold=0), dict(good, period=0), dict(good, first=-1), dict(good, count=-1)):
        assert check([good, bad]) != 0 and b"robust spec 1" in emu.go2nn_last_error(), bad
    for P in (0, 65, -1):
        assert check([good], P) != 0 and b"P = " in emu.go2nn_last_error()
    assert emu.go2nn_robust_check_specs(None, 1) != 0 and emu.go2nn_last_error()
    N = 4
    bufs = {k: np.zeros((N, max(w, 1)), np.uint8 if k.endswith("_buf") else np.float32) for k, w in WIDTH.items()}

    def make_in():
        a = Go2nnRobustIn()
        for k in ROBUST_FIELDS:
            f = getattr(a, k)
            f.p, f.env_stride, f.comp_stride = bufs[k].ctypes.data, max(WIDTH[k], 1), 1 if WIDTH[k] else 0
        a.num_specs = 1
        return a
    specs, pert, table = make_specs([good]), np.zeros(N, np.int32), np.zeros((GO2NN_ROBUST_NUM, N), np.float32)
    p = lambda x: C.c_void_p(x.ctypes.data)
    for fn in (emu.go2nn_robust_apply, emu.go2nn_robust_accumulate):
        assert fn(C.byref(make_in()), C.cast(specs, C.c_void_p), p(pert), p(table), N, None) == 0, emu.go2nn_last_error()
        for args in ((None, C.cast(specs, C.c_void_p), p(pert), p(table), N), (C.byref(make_in()), None, p(pert), p(table), N), (C.byref(make_in()), C.cast(specs, C.c_void_p), None, p(table), N),
                     (C.byref(make_in()), C.cast(specs, C.c_void_p), p(pert), None, N), (C.byref(make_in()), C.cast(specs, C.c_void_p), p(pert), p(table), 0)):
            assert fn(*args, None) != 0 and emu.go2nn_last_error()

        def broken(edit):
            a = make_in()
            edit(a)
            return fn(C.byref(a), C.cast(specs, C.c_void_p), p(pert), p(table), N, None)
        for P in (0, 65):
            assert broken(lambda a: setattr(a, "num_specs", P)) != 0 and b"num_specs" in emu.go2nn_last_error()
        assert broken(lambda a: setattr(a.root_states, "env_stride", 0)) != 0 and b"stride" in emu.go2nn_last_error()
        assert broken(lambda a: setattr(a.motor_strengths, "comp_stride", 0)) != 0 and b"stride" in emu.go2nn_last_error()
        assert broken(lambda a: setattr(a.friction_coeffs, "env_stride", 0)) != 0 and b"stride" in emu.go2nn_last_error()
        assert broken(lambda a: setattr(a.added_base_mass, "p", None)) != 0 and b"null" in emu.go2nn_last_error()
    assert emu.go2nn_robust_begin(None, N, 0, None) != 0 and emu.go2nn_robust_begin(p(table), 0, 0, None) != 0 and emu.go2nn_last_error()
    assert emu.go2nn_robust_reduce(None, p(pert), N, 1, p(table), None) != 0


def test_robust_symbols_and_structs_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_robust_check_specs", "go2nn_robust_begin", "go2nn_robust_apply", "go2nn_robust_accumulate", "go2nn_robust_reduce"):
            assert (" T " + f + "\n") in syms, (path, f)
    spec_names = [n for n, _ in Go2nnRobustSpec._fields_]
    in_names = [n for n, _ in Go2nnRobustIn._fields_]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu %zu %d %d %d %d", sizeof(Go2nnRobustSpec), sizeof(Go2nnRobustIn), '
                   'GO2NN_ROBUST_NUM, GO2NN_ROBUST_ACC_FIRST, GO2NN_ROBUST_ACC_NUM, GO2NN_ROBUST_MAX_SPECS);\n'
                   + "".join('printf(" %%zu", offsetof(Go2nnRobustSpec, %s));\n' % n for n in spec_names)
                   + "".join('printf(" %%zu", offsetof(Go2nnRobustIn, %s));\n' % n for n in in_names)
                   + 'printf(" %d %d %d %d %d", GO2NN_ROBUST_MASK_STRENGTH, GO2NN_ROBUST_MASK_KP, GO2NN_ROBUST_MASK_KD, GO2NN_ROBUST_MASK_ADDED_MASS, GO2NN_ROBUST_MASK_FRICTION);\n'
                   + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [C.sizeof(Go2nnRobustSpec), C.sizeof(Go2nnRobustIn), len(ROBUST_ROWS), GO2NN_ROBUST_ACC_FIRST, GO2NN_ROBUST_ACC_NUM, _nn.GO2NN_ROBUST_MAX_SPECS]
    assert got[6:6 + len(spec_names)] == [getattr(Go2nnRobustSpec, n).offset for n in spec_names]
    assert got[6 + len(spec_names):-5] == [getattr(Go2nnRobustIn, n).offset for n in in_names]
    assert got[-5:] == [ROBUST_MASK[k] for k in ("strength", "kp_mul", "kd_mul", "added_mass", "friction")]
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    enum = hdr[hdr.index("GO2NN_ROBUST_STEP = 0"):hdr.index("GO2NN_ROBUST_NUM\n")]
    assert [e.strip().split(" ")[0].replace("GO2NN_ROBUST_", "").lower() for e in enum.split(",") if e.strip()] == list(ROBUST_ROWS)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
PUSH = dict(push_first_s=0.2, push_period_s=0.4, push_window_s=0.3, recover_thr=0.3, recover_hold_s=0.1)
PERTS = [["nominal", {}], ["shove", {"dv": [0.3, 1.0, 0.2]}], ["weak", {"strength": 0.8, "kp_mul": 0.9}]]


def heading(q):
    """float64 (c, s) of the quaternions q [n, 4] (xyzw), the kernel's rule"""
    x, y, z, w = (q[:, i].astype(np.float64) for i in range(4))
    c, s = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z)
    n = np.hypot(c, s)
    return np.where(n < 1e-6, 1.0, c / np.maximum(n, 1e-300)), np.where(n < 1e-6, 0.0, s / np.maximum(n, 1e-300))


def check_push(v_before, quat, v_after, dv, what=""):
    """v_after == v_before + dv rotated about z by the heading of quat, to the accumulate bound (64 eps of the summed magnitudes)"""
    c, s = heading(quat)
    dv = np.asarray(dv, np.float32).astype(np.float64)
    want = v_before.astype(np.float64) + np.stack([c * dv[0] - s * dv[1], s * dv[0] + c * dv[1], np.full_like(c, dv[2])], 1)
    mag = np.abs(v_before.astype(np.float64)) + np.stack([abs(c * dv[0]) + abs(s * dv[1]), abs(s * dv[0]) + abs(c * dv[1]), np.full_like(c, abs(dv[2]))], 1)
    gap, bound = np.abs(v_after.astype(np.float64) - want), th.accumulate_bound(32, mag)
    assert (gap <= bound).all(), (what, float((gap / bound).max()))
    return float((gap / bound).max())


def test_nominal_alone_changes_nothing(emu):
    """one sham perturbation: the same robots in the same groups, no row written, no velocity moved -> the groups table is byte-identical to perturbations = None"""
    ac = th.small_actor_critic()
    plain = th.make_evaluator(emu, **PUSH)
    res0 = plain.evaluate(ac)
    assert "cells" not in res0 and "perturbations" not in res0 and not hasattr(plain, "rtable")
    plain.close()
    sham = th.make_evaluator(emu, perturbations=[["nominal", {}]], **PUSH)
    res1 = sham.evaluate(ac)
    assert res1["table"].tobytes() == res0["table"].tobytes() and str(res1["groups"]) == str(res0["groups"])
    assert res1["perturbations"]["nominal"]["pushes"] == 2 * 38 == res1["overall"]["pushes"] and res1["push_steps"] == [10, 30]
    sham.close()


def test_evaluator_with_perturbations_on_host_libraries(emu):
    from go2_rl_gym_amd.utils.evaluator import RESULT_KEYS, ROBUST_KEYS, format_table, results_dict, scalars
    after_step, after_apply, rows = {}, {}, {}
    victim = []

    def step_cb(ev, k, counted):
        after_step[k] = ev.env._buf["root_states"].detach().clone().numpy()
        if k == 20:          # a reset between two steps: the simulator redraws the env's motor strengths (1.0: the evaluation's range is [1, 1])
            ids = np.asarray(victim, np.int32)
            assert ev.env.lib.go2sim_reset_idx(ev.env.handle, ids.ctypes.data, 1, None) == 0
            assert (ev.env._buf["motor_strengths"][victim[0]] == 1.0).all()
            ev.env._buf["p_gains_multiplier"][victim[0]] = 1.0

    def apply_cb(ev, k, counted):
        after_apply[k] = ev.env._buf["root_states"].detach().clone().numpy()
        rows[k] = {f: ev.env._buf[f].detach().clone().numpy() for f in ("motor_strengths", "p_gains_multiplier", "d_gains_multiplier", "added_base_mass", "friction_coeffs")}
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    env_cfg, _ = task_registry.get_cfgs("go2_flat")
    ev = PolicyEvaluator(env_cfg, dict(th.EVAL, num_envs=76, perturbations=PERTS, **PUSH), task_class=task_registry.get_task_class("go2_flat"), device="cpu", lib=load_oracle(),
                         nn_lib=emu, step_callback=step_cb, apply_callback=apply_cb)
    S, P, N = 4, 3, 76
    assert (ev.push_first, ev.push_period, ev.push_window, ev.push_hold, ev.push_count) == (10, 20, 15, 5, 2) and ev.push_steps.tolist() == [10, 30]
    sizes = np.bincount(ev.cell_host, minlength=S * P)
    assert ev.num_cells == S * P and sizes.min() >= 4 and sizes.max() - sizes.min() <= 1 and (ev.cell_host == ev.group_host * P + ev.pert_host).all()
    weak = np.nonzero(ev.pert_host == 2)[0]
    victim.append(int(weak[1]))
    ac = th.small_actor_critic()
    res = ev.evaluate(ac)
    W = ev.warmup_steps
    assert len(after_apply) == len(after_step) == W + ev.steps
    # the push: at counted steps 10 and 30 the `shove` robots' velocity is what the previous step left plus the rotated impulse; nothing else of any root state ever moves
    worst = 0.0
    for k in range(1, W + ev.steps):
        prev, now = after_step[k - 1], after_apply[k]
        if k == 21:
            prev = prev.copy(); prev[victim[0]] = now[victim[0]]          # (the callback's reset moved this robot)
        pushed = (ev.pert_host == 1) if (k - W) in (10, 30) else np.zeros(N, bool)
        np.testing.assert_array_equal(now[~pushed], prev[~pushed])
        if pushed.any():
            np.testing.assert_array_equal(now[pushed][:, :7], prev[pushed][:, :7])
            np.testing.assert_array_equal(now[pushed][:, 10:], prev[pushed][:, 10:])
            worst = max(worst, check_push(prev[pushed][:, 7:10], prev[pushed][:, 3:7], now[pushed][:, 7:10], PERTS[1][1]["dv"], "step %d" % k))
            assert np.abs(now[pushed][:, 7:10] - prev[pushed][:, 7:10]).max() > 0.2
    print("push vs float64: largest gap / bound %.3f" % worst)
    # the dynamics rows: the `weak` robots' at the spec's values at every step — the step after the reset included —, everybody else's untouched
    for k, r in rows.items():
        assert (r["motor_strengths"][weak] == np.float32(0.8)).all() and (r["p_gains_multiplier"][weak] == np.float32(0.9)).all(), k
        assert (r["motor_strengths"][ev.pert_host != 2] == 1.0).all() and (r["p_gains_multiplier"][ev.pert_host != 2] == 1.0).all()
        assert (r["d_gains_multiplier"] == 1.0).all() and (r["added_base_mass"] == 0.0).all() and (r["friction_coeffs"] == rows[0]["friction_coeffs"]).all()
    # the results' shape
    names = [p[0] for p in PERTS]
    assert res["perturbation_names"] == names and list(res["perturbations"]) == names and set(res["cells"]["plane"]) == {s[0] for s in th.EVAL["scenarios"]}
    for d in [res["overall"]] + list(res["perturbations"].values()) + [c for per in res["cells"]["plane"].values() for c in per.values()]:
        assert set(d) == set(RESULT_KEYS) | set(ROBUST_KEYS)
    for si, s in enumerate(th.EVAL["scenarios"]):
        assert set(res["groups"]["plane"][s[0]]) == set(RESULT_KEYS)
        for pi, n in enumerate(names):
            cell = res["cells"]["plane"][s[0]][n]
            assert cell["n_envs"] == sizes[si * P + pi] and cell["pushes"] == 2 * cell["n_envs"]
            assert 0 <= cell["push_falls"] <= 1 and 0 <= cell["recovered"] <= 1 and cell["push_falls"] + cell["recovered"] <= 1 and cell["peak_lin_vel_err"] > 0
        assert res["groups"]["plane"][s[0]]["n_envs"] == sum(res["cells"]["plane"][s[0]][n]["n_envs"] for n in names)
    assert res["overall"]["pushes"] == 2 * N and res["table"].shape == (S, 12) and res["cell_table"].shape == (S * P, 12) and res["robust_table"].shape == (S * P, 7)
    tags = dict(scalars(res))
    assert "Eval/robust/shove/push_falls" in tags and "Eval/robust/nominal/lin_vel_err" in tags and "Eval/plane/stand/tilt" in tags
    rd = results_dict(res, 3)
    assert set(rd["perturbations"]) == set(names) and rd["push"]["count"] == 2
    import yaml
    assert set(yaml.safe_load(yaml.safe_dump(rd))["perturbations"]["weak"]) == set(RESULT_KEYS) | set(ROBUST_KEYS)
    text = format_table(res)
    print(text)
    assert "perturbation" in text and "shove" in text and "recovery_time_s" in text
    ev.close()
    # the same weights twice: byte-equal cells (no callbacks, so no reset in the middle)
    ev = th.make_evaluator(emu, num_envs=76, perturbations=PERTS, record=1, **PUSH)
    a, b = ev.evaluate(ac), ev.evaluate(ac)
    assert a["cell_table"].tobytes() == b["cell_table"].tobytes() and a["robust_table"].tobytes() == b["robust_table"].tobytes() and str(a["cells"]) == str(b["cells"])
    assert a["robust_table"][:, 0].sum() == 2 * N
    tr = a["trace"]
    assert tr["perturbations"] == names and tr["push_steps"].tolist() == [10, 30] and len(tr["env_ids"]) == S * P
    assert (tr["pert_of_robot"] == ev.pert_host[tr["env_ids"]]).all() and sorted(tr["pert_of_robot"].tolist()) == sorted(list(range(P)) * S) and tr["frames"].shape[0] == ev.steps
    ev.close()
    with pytest.raises(RuntimeError, match="window"):
        th.make_evaluator(emu, perturbations=PERTS, **dict(PUSH, push_window_s=0.5))
    with pytest.raises(ValueError, match="unknown field"):
        th.make_evaluator(emu, perturbations=[["x", {"mass": 1.0}]], **PUSH)


def test_robust_evaluation_leaves_the_training_run_untouched(emu):
    from go2_rl_gym_amd.utils.evaluator import DEFAULT_PERTURBATIONS
    args = get_args(["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5", "--evaluate", "--robust"])
    assert args.robust is True and get_args(["--task", "go2_flat"]).robust is False
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, train_cfg = task_registry.make_alg_runner(env, "go2_flat", args, log_root=None)
    assert train_cfg.evaluation.perturbations == DEFAULT_PERTURBATIONS and [p[0] for p in runner.eval_cfg["perturbations"]][:3] == ["nominal", "push_front_1.0", "push_side_1.0"]
    _, fresh = task_registry.get_cfgs("go2_flat")
    assert fresh.evaluation.perturbations is None and fresh.evaluation.push_first_s == 1.0 and fresh.evaluation.push_period_s == 2.5 and fresh.evaluation.push_window_s == 2.0
    assert fresh.evaluation.recover_thr == 0.3 and fresh.evaluation.recover_hold_s == 0.2
    runner.learn(1, init_at_random_ep_len=True)
    runner.eval_cfg = dict(runner.eval_cfg, num_envs=84, seconds=0.4, warmup_s=0.1, push_first_s=0.1, push_period_s=0.2, push_window_s=0.1, recover_hold_s=0.04)
    runner.evaluator_kwargs = {"nn_lib": emu}
    before = th._snapshot(env, runner)
    res = runner.update_evaluation(0, False)
    assert res is not None and runner.evaluator.env is not env and res["overall"]["pushes"] == 2 * 84 and set(res["perturbations"]) == {p[0] for p in DEFAULT_PERTURBATIONS}
    th.assert_same_snapshot(before, th._snapshot(env, runner))
    runner.learn(1)
    env.close()
