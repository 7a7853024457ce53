"""The evaluator's action and torque spectra on the CPU: the host build of the go2nn_spectrum_* kernels (include/go2nn.h) against a float64 restatement written here with
np.fft.rfft — the same Hann window, detrend, window positions and skip rule, but none of the kernel's summation order —, the closed forms of a sinusoid on a bin and of a
constant, the reset rule, the record kernel through both buffer layouts, the reduce against math.fsum, the argument checks, the struct layout, and PolicyEvaluator with
`spectrum` on the oracle + the host build: nothing changes with the flag off, the scores do not move with it on, the per-robot table is what the restatement makes of the
recorded buffers, and every partition of every mode is the sum of its cells."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import ROOT, load_nn_emu, reduce_groups, reduce_twice
import test_eval_host as th
from test_robust_host import HostMemory
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import (GO2NN_SPECTRUM_BIN0, GO2NN_SPECTRUM_CH_ACTION0, GO2NN_SPECTRUM_CH_RESET, GO2NN_SPECTRUM_CH_TORQUE0, GO2NN_SPECTRUM_CHANNELS,
                                GO2NN_SPECTRUM_SKIPPED, GO2NN_SPECTRUM_USED, SPECTRUM_FIELDS, SPECTRUM_KINDS, SPECTRUM_SIGNALS, Go2nnSpectrumIn, spectrum_bins, spectrum_row,
                                spectrum_rows, spectrum_trace_rows, spectrum_twiddle)
from go2_rl_gym_amd.utils.symmetry import joint_kinds

EINVAL = -22
FS = 50.0
KINDS = np.asarray(joint_kinds())
SLOTS = [j for kind in range(3) for j in range(12) if KINDS[j] == kind]          # the joints in slot order: hips, thighs, calves
WARMUP = 3          # record calls in front of the counted steps


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def reference(actions, torques, reset, W, fs=FS):
    """the estimator in float64.  actions, torques [T, N, 12] (joint order) and reset [T, N] are the COUNTED frames
    -> {"P", "M": [N, 2, 3, K] sums over the used windows and a kind's 4 joints, "used", "skipped": [N], "windows": positions}"""
    x = np.stack([np.asarray(actions, np.float64), np.asarray(torques, np.float64)], 2)          # [T, N, 2, 12]
    reset = np.asarray(reset, bool)
    T, N = reset.shape
    K = W // 2 + 1
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
    c = np.full(K, 2.0)
    c[0] = c[-1] = 1.0
    out = {"P": np.zeros((N, 2, 3, K)), "M": np.zeros((N, 2, 3, K)), "used": np.zeros(N), "skipped": np.zeros(N), "windows": []}
    f0 = 0
    while f0 + W <= T:
        out["windows"].append(f0)
        seg = x[f0:f0 + W]
        X = np.fft.rfft((seg - seg.mean(0)) * hann[:, None, None, None], axis=0)          # [K, N, 2, 12]
        mag = np.abs(X)
        P = np.moveaxis(c[:, None, None, None] * mag ** 2 / (fs * (hann ** 2).sum()), 0, -1)          # [N, 2, 12, K]
        M = np.moveaxis(c[:, None, None, None] * mag / hann.sum(), 0, -1)
        skip = reset[f0:f0 + W].any(0)
        for kind in range(3):
            out["P"][~skip, :, kind] += P[~skip][:, :, KINDS == kind].sum(2)
            out["M"][~skip, :, kind] += M[~skip][:, :, KINDS == kind].sum(2)
        out["used"] += ~skip
        out["skipped"] += skip
        f0 += W // 2
    return out


def table_parts(table, W):
    """the per-robot table [rows, N] -> (P, M [N, 2, 3, K] float64, used, skipped [N])"""
    K, t = spectrum_bins(W), np.asarray(table, np.float64)
    cut = lambda what: t[spectrum_row(W, what, 0, 0):spectrum_row(W, what, 0, 0) + 6 * K].reshape(2, 3, K, -1).transpose(3, 0, 1, 2)
    return cut("P"), cut("M"), t[GO2NN_SPECTRUM_USED], t[GO2NN_SPECTRUM_SKIPPED]


def check_table(table, ref, W, what):
    """whole numbers exactly; every P and M entry within (windows + 2) 2^-24 of itself — one fp32 rounding per window, the fp32 running sum of non-negative terms — plus
    1e-12 of its spectrum's total for the fp64 DFT -> largest gap / bound"""
    P, M, used, skipped = table_parts(table, W)
    np.testing.assert_array_equal(used, ref["used"])
    np.testing.assert_array_equal(skipped, ref["skipped"])
    worst = 0.0
    for name, got in (("P", P), ("M", M)):
        want = ref[name]
        bound = (ref["used"][:, None, None, None] + 2) * 2.0 ** -24 * want + 1e-12 * want.sum(-1, keepdims=True)
        gap = np.abs(got - want)
        print("%s %s: largest |gap| %.3e, largest gap / bound %.4f" % (what, name, gap.max() if gap.size else 0.0, (gap / np.maximum(bound, 1e-300)).max() if gap.size else 0.0))
        assert (gap <= bound).all(), (name, float(gap.max()), float((gap / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((gap / np.maximum(bound, 1e-300)).max()) if gap.size else 0.0)
    return worst


def random_trace(N, T, seed=0, resets=True):
    """-> actions, torques [WARMUP + T, N, 12] fp32 with a different scale, offset and colour per joint, reset [WARMUP + T, N] (a few flags; all set during the warm-up)"""
    rng = np.random.default_rng(seed + 1000 * N + T)
    S = WARMUP + T
    scale, offset = np.exp(rng.normal(0, 1.5, (2, 1, N, 12))), rng.normal(0, 3, (2, 1, N, 12))
    white = rng.normal(0, 1, (2, S, N, 12))
    x = (offset + scale * (white + np.cumsum(white, 1) * rng.uniform(0, 0.5, (2, 1, N, 12)))).astype(np.float32)
    reset = rng.random((S, N)) < (0.02 if resets else 0.0)
    reset[:WARMUP] = True
    return x[0], x[1], reset


def store2(a, layout):
    """a logical [N, 12] array as the libraries store it -> (flat storage, env stride, component stride): env-major, or field-major as the HIP simulator keeps it"""
    N, w = a.shape
    return (np.ascontiguousarray(a.T), 1, N) if layout == 1 else (np.ascontiguousarray(a), w, 1)


def spectrum_in(mem, h, strides, slots=SLOTS):
    a = Go2nnSpectrumIn()
    for k in ("actions", "torques"):
        f = getattr(a, k)
        f.p, f.env_stride, f.comp_stride = mem.ptr(h[k]), strides[k][0], strides[k][1]
    a.reset_buf.p, a.reset_buf.env_stride, a.reset_buf.comp_stride = mem.ptr(h["reset_buf"]), 1, 0
    a.joint_of_slot[:] = slots
    return a


def record(lib, mem, actions, torques, reset, T, layout):
    """every call of the scripted sequence through go2nn_spectrum_record -> the trace's handle; the warm-up calls write nothing but the counter"""
    S, N = reset.shape
    h, strides = {}, {}
    for k, a in (("actions", actions[0]), ("torques", torques[0])):
        flat, *strides[k] = store2(a, layout)
        h[k] = mem.put(flat)
    h["reset_buf"] = mem.put(reset[0].astype(np.uint8))
    a = spectrum_in(mem, h, strides)
    trace = mem.put(np.full((spectrum_trace_rows(T), N), 7.0, np.float32))
    assert lib.go2nn_spectrum_begin(C.c_void_p(mem.ptr(trace)), N, -WARMUP, T, mem.stream) == 0, lib.go2nn_last_error()
    got = mem.get(trace).reshape(-1, N)
    assert (got[0] == -WARMUP).all() and not got[1:].any()
    for call in range(S):
        mem.set(h["actions"], store2(actions[call], layout)[0])
        mem.set(h["torques"], store2(torques[call], layout)[0])
        mem.set(h["reset_buf"], reset[call].astype(np.uint8))
        assert lib.go2nn_spectrum_record(C.byref(a), C.c_void_p(mem.ptr(trace)), N, T, mem.stream) == 0, lib.go2nn_last_error()
        if call == WARMUP - 1:
            got = mem.get(trace).reshape(-1, N)
            assert (got[0] == 0).all() and not got[1:].any()
    return trace


def welch(lib, mem, trace, N, T, W, fs=FS, fill=7.0):
    tw = mem.put(spectrum_twiddle(W))
    table = mem.put(np.full((spectrum_rows(W), N), fill, np.float32))
    assert lib.go2nn_spectrum_welch(C.c_void_p(mem.ptr(trace)), N, T, W, fs, C.c_void_p(mem.ptr(tw)), C.c_void_p(mem.ptr(table)), mem.stream) == 0, lib.go2nn_last_error()
    return mem.get(table).reshape(spectrum_rows(W), N)


def run_trace(lib, mem, actions, torques, reset, W, layout=1):
    """record + Welch of a scripted sequence [WARMUP + T, ...] on `lib` -> (table fp32 [rows, N], the trace fp32 [1 + 25 T, N])"""
    S, N = reset.shape
    T = S - WARMUP
    trace = record(lib, mem, actions, torques, reset, T, layout)
    return welch(lib, mem, trace, N, T, W), mem.get(trace).reshape(-1, N)


def check_trace(trace, actions, torques, reset, T):
    """the trace holds bit-exact copies of the counted frames, the joints in slot order"""
    N = reset.shape[1]
    t = trace.reshape(-1, N)
    assert (t[0] == T).all()
    frames = t[1:].reshape(T, GO2NN_SPECTRUM_CHANNELS, N)
    assert frames[:, GO2NN_SPECTRUM_CH_ACTION0:GO2NN_SPECTRUM_CH_ACTION0 + 12].tobytes() == np.ascontiguousarray(actions[WARMUP:][:, :, SLOTS].transpose(0, 2, 1)).tobytes()
    assert frames[:, GO2NN_SPECTRUM_CH_TORQUE0:GO2NN_SPECTRUM_CH_TORQUE0 + 12].tobytes() == np.ascontiguousarray(torques[WARMUP:][:, :, SLOTS].transpose(0, 2, 1)).tobytes()
    np.testing.assert_array_equal(frames[:, GO2NN_SPECTRUM_CH_RESET], reset[WARMUP:].astype(np.float32))


def figures(row, W, fs=FS, cutoff=10.0):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    return PolicyEvaluator._spectrum_row(types.SimpleNamespace(spectrum_window=W, spectrum_fs=fs, spectrum_cutoff=cutoff), row)


def robot_row(table, e):
    """robot e's column of the per-robot table as a reduce row of a group of one"""
    return np.concatenate([[1.0], np.asarray(table, np.float64)[:, e]])


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_of", ["W-1", "W", "2W+3"])
@pytest.mark.parametrize("W", [8, 64])
@pytest.mark.parametrize("N", [1, 63, 65])
def test_welch_against_float64(emu, N, W, T_of):
    """no window, one window, three windows and a dropped tail"""
    T = {"W-1": W - 1, "W": W, "2W+3": 2 * W + 3}[T_of]
    actions, torques, reset = random_trace(N, T)
    table, trace = run_trace(emu, HostMemory(), actions, torques, reset, W)
    check_trace(trace, actions, torques, reset, T)
    ref = reference(actions[WARMUP:], torques[WARMUP:], reset[WARMUP:], W)
    assert len(ref["windows"]) == {"W-1": 0, "W": 1, "2W+3": 3}[T_of]
    check_table(table, ref, W, "host N=%d W=%d T=%d" % (N, W, T))
    if T < W:
        assert not table.any()
    elif N > 1:
        assert ref["used"].sum() > 0 and (ref["P"].sum(-1)[ref["used"] > 0] > 0).all()
    if T_of == "2W+3" and N == 65:
        assert ref["skipped"].sum() > 0


def test_restatement_against_scipy():
    """where scipy is importable: the yardstick itself is scipy.signal.welch's estimate (density scaling, constant detrend, periodic Hann, half overlap)"""
    signal = pytest.importorskip("scipy.signal")
    W, T, N = 64, 2 * 64 + 3, 5
    actions, torques, reset = random_trace(N, T, resets=False)
    ref = reference(actions[WARMUP:], torques[WARMUP:], reset[WARMUP:], W)
    for si, x in enumerate((actions, torques)):
        _, pxx = signal.welch(x[WARMUP:].astype(np.float64), fs=FS, window="hann", nperseg=W, noverlap=W // 2, detrend="constant", scaling="density", axis=0, average="mean")
        for kind in range(3):
            want = pxx[:, :, KINDS == kind].sum(2).T * len(ref["windows"])          # scipy averages the windows; the table sums them
            np.testing.assert_allclose(ref["P"][:, si, kind], want, rtol=1e-10, atol=1e-12 * want.max())


@pytest.mark.parametrize("k0", [3, 20])
def test_sinusoid_on_a_bin(emu, k0):
    """amplitude A exactly on bin k0 of the hip joints' actions at W = 64: power in k0 - 1, k0, k0 + 1 as 1/4 : 1 : 1/4, amplitude A on the bin, the centroid on f_k0, the
    high-frequency share 0 or 1 by the cut-off; the fp32 samples leave a noise floor of 2^-24 A per sample, far below 1e-9 of the peak's power"""
    W, N, A = 64, 3, 0.75
    T = 2 * W
    n = np.arange(WARMUP + T)[:, None, None]
    actions = np.zeros((WARMUP + T, N, 12), np.float32)
    actions[:, :, KINDS == 0] = (A * np.cos(2.0 * np.pi * k0 * n / W + np.asarray([0.3, 1.1, 2.0, 4.0]))).astype(np.float32)
    torques = np.full_like(actions, 2.5)          # a constant: power 0
    reset = np.zeros((WARMUP + T, N), bool)
    table, _ = run_trace(emu, HostMemory(), actions, torques, reset, W)
    P, M, used, _ = table_parts(table, W)
    assert (used == 3).all() and not P[:, 1].any() and not M[:, 1].any() and not P[:, 0, 1:].any()
    hip = P[:, 0, 0]
    peak = hip[:, k0]
    np.testing.assert_allclose(hip[:, k0 - 1] / peak, 0.25, rtol=1e-6)
    np.testing.assert_allclose(hip[:, k0 + 1] / peak, 0.25, rtol=1e-6)
    others = np.delete(hip, [k0 - 1, k0, k0 + 1], axis=1)
    assert (others <= 1e-9 * peak[:, None]).all()
    np.testing.assert_allclose(M[:, 0, 0, k0] / (4 * 3), A, rtol=1e-6)          # 4 joints x 3 windows
    np.testing.assert_allclose(peak, 4 * 3 * A * A * W / (3.0 * FS), rtol=1e-6)          # 2 |A W / 4|^2 / (fs 3 W / 8) per joint and window
    f = k0 * FS / W
    for cutoff, share in (((k0 - 1) * FS / W, 1.0), ((k0 + 1) * FS / W + 1e-9, 0.0)):
        d = figures(robot_row(table, 0), W, cutoff=cutoff)
        assert abs(d["action_hf_share/hip"] - share) <= 1e-9 and abs(d["action_hf_share"] - share) <= 1e-9
        assert abs(d["action_centroid_hz/hip"] - f) <= 1e-6 * f and abs(d["action_centroid_hz"] - f) <= 1e-6 * f
        for kind in ("thigh", "calf"):
            assert d["action_power/" + kind] == 0.0 and all(math.isnan(d["action_%s/%s" % (k, kind)]) for k in ("hf_share", "centroid_hz"))
            assert d["action_smoothness/" + kind] == 0.0
        assert d["torque_power"] == 0.0 and math.isnan(d["torque_hf_share"]) and math.isnan(d["torque_centroid_hz"])
        np.testing.assert_allclose(d["action_power/hip"], 0.5 * A * A, rtol=1e-6)          # (fs / W) (1/4 + 1 + 1/4) A^2 W / (3 fs): the sinusoid's variance
        # CAPS: 2 / (n fs) sum f_k M_k, n = W / 2, with M = A / 2, A, A / 2 around k0
        np.testing.assert_allclose(d["action_smoothness/hip"], 2.0 / ((W // 2) * FS) * A * ((f - FS / W) / 2 + f + (f + FS / W) / 2), rtol=1e-6)
        assert d["spectrum_windows"] == 3 and d["spectrum_skipped_share"] == 0.0 and d["n_envs"] == 1


@pytest.mark.parametrize("W", [8, 64])
def test_constant_signal_has_no_power(emu, W):
    N, T = 2, 3 * W
    actions = np.broadcast_to(np.linspace(-3, 3, 12, dtype=np.float32), (WARMUP + T, N, 12)).copy()
    torques = np.full_like(actions, -17.25)
    table, _ = run_trace(emu, HostMemory(), actions, torques, np.zeros((WARMUP + T, N), bool), W, layout=0)
    assert (table[GO2NN_SPECTRUM_USED] == 5).all() and not table[GO2NN_SPECTRUM_SKIPPED].any() and not table[GO2NN_SPECTRUM_BIN0:].any()


def test_resets_skip_exactly_their_windows(emu):
    """T = 4 W: seven windows.  Robot 0: a flag in [0, W / 2) lies in window 0 alone; robot 1: a flag in [W / 2, W) lies in windows 0 and 1; robot 2: none; robot 3: every
    window hit.  Values of frames that lie only in skipped windows do not matter"""
    W, N = 16, 4
    T = 4 * W
    actions, torques, reset = random_trace(N, T, seed=3, resets=False)
    reset[WARMUP + 5, 0] = True
    reset[WARMUP + W // 2 + 3, 1] = True
    reset[WARMUP + W // 2 - 1::W // 2, 3] = True          # frames 7, 15, 23, ...: every window holds one
    mem = HostMemory()
    table, _ = run_trace(emu, mem, actions, torques, reset, W)
    ref = reference(actions[WARMUP:], torques[WARMUP:], reset[WARMUP:], W)
    assert len(ref["windows"]) == 7 and ref["skipped"].tolist() == [1, 2, 0, 7] and ref["used"].tolist() == [6, 5, 7, 0]
    check_table(table, ref, W, "resets")
    assert not table[GO2NN_SPECTRUM_BIN0:, 3].any()
    rows = np.stack([robot_row(table, e) for e in range(N)])
    shares = [figures(r, W)["spectrum_skipped_share"] for r in rows]
    assert shares == [1 / 7, 2 / 7, 0.0, 1.0]
    pooled = figures(rows.sum(0), W)
    assert pooled["spectrum_windows"] == 18 and pooled["spectrum_skipped_share"] == 10 / 28 and pooled["n_envs"] == 4
    dead = figures(rows[3], W)          # a cell of robots without a used window: every figure NaN
    assert dead["spectrum_windows"] == 0 and all(math.isnan(v) for k, v in dead.items() if k not in ("spectrum_windows", "spectrum_skipped_share", "n_envs"))
    # robot 3 adds nothing to a pool: the figures of robots 0 .. 2 alone, apart from the counts
    a, b = figures(rows[:3].sum(0), W), pooled
    assert all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a if k not in ("spectrum_skipped_share", "n_envs"))
    # frames 0 .. W / 2 - 1 of robot 0 and 0 .. W / 2 - 1 of robot 1 lie in skipped windows only
    a2, t2 = actions.copy(), torques.copy()
    a2[WARMUP:WARMUP + W // 2, :2] += 100.0
    t2[WARMUP:WARMUP + W // 2, :2] *= -3.0
    again, _ = run_trace(emu, HostMemory(), a2, t2, reset, W)
    assert again.tobytes() == table.tobytes()
    a2[WARMUP + W // 2, 0] += 1.0          # ... and the next frame of robot 0 does matter
    moved, _ = run_trace(emu, HostMemory(), a2, t2, reset, W)
    assert moved[:, 1:].tobytes() == table[:, 1:].tobytes() and moved[:, 0].tobytes() != table[:, 0].tobytes()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 5])
def test_record_is_a_bit_exact_copy(emu, N, layout):
    """env-major test tensors and the HIP simulator's field-major buffers; the warm-up calls write nothing (checked inside record); calls past T write nothing either"""
    T = 9
    actions, torques, reset = random_trace(N, T + 2, seed=1)
    mem = HostMemory()
    trace = record(emu, mem, actions, torques, reset, T, layout)
    got = mem.get(trace).reshape(-1, N)
    assert (got[0] == T + 2).all()
    got[0] = T
    check_trace(got, actions[:WARMUP + T], torques[:WARMUP + T], reset[:WARMUP + T], T)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def reduce_case(N, G, W, seed=5):
    rng = np.random.default_rng(seed + N)
    table = np.abs(rng.normal(0, 1, (spectrum_rows(W), N)) * np.exp(rng.normal(0, 3, (spectrum_rows(W), N)))).astype(np.float32)
    table[:GO2NN_SPECTRUM_BIN0] = rng.integers(0, 20, (GO2NN_SPECTRUM_BIN0, N))
    return table, reduce_groups(rng, N, G)


def check_reduce(out, table, group, G, N, what):
    """the group sizes exactly; every fp64 sum to N roundings of the running sum"""
    worst = 0.0
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        assert out[g, 0] == len(ids)
        for r in range(table.shape[0]):
            terms = [float(x) for x in table[r, ids]]
            gap, bound = abs(out[g, 1 + r] - math.fsum(terms)), N * 2.0 ** -53 * math.fsum(abs(x) for x in terms)
            assert gap <= bound, (g, r, gap, bound)
            worst = max(worst, gap / max(bound, 1e-300))
    assert (out[1] == 0).all() and (group == 1).sum() == 0
    print("%s: largest reduce gap / bound %.3f" % (what, worst))


def emu_reduce(emu, table, group, G, W):
    out = np.full((G, 1 + spectrum_rows(W)), -1.0)
    assert emu.go2nn_spectrum_reduce(C.c_void_p(table.ctypes.data), C.c_void_p(group.ctypes.data), table.shape[1], G, W, C.c_void_p(out.ctypes.data), None) == 0, emu.go2nn_last_error()
    return out


@pytest.mark.parametrize("N,G,W", [(1, 3, 8), (17, 3, 8), (300, 5, 16), (4096, 7, 8)])
def test_reduce_against_fsum(emu, N, G, W):
    table, group = reduce_case(N, G, W)
    out = reduce_twice(lambda t, g, n, G_, o: emu.go2nn_spectrum_reduce(t, g, n, G_, W, o, None), table, group, G, 1 + spectrum_rows(W))
    if N >= 17:
        check_reduce(out, table, group, G, N, "host N=%d" % N)
    row = figures(out[1], W)          # the empty group: zeros, and figures that do not exist rather than an exception
    assert not out[1].any() and row["n_envs"] == 0 and row["spectrum_windows"] == 0
    assert all(math.isnan(v) for k, v in row.items() if k not in ("n_envs", "spectrum_windows")) and len(row) == 2 * 4 * 4 + 3


def test_argument_checks(emu):
    N, T, W = 4, 20, 8
    actions, torques, rs = np.zeros((N, 12), np.float32), np.zeros((N, 12), np.float32), np.zeros(N, np.uint8)
    trace, tw = np.full((spectrum_trace_rows(T), N), 3.0, np.float32), spectrum_twiddle(W)
    table, group, out = np.full((spectrum_rows(W), N), 3.0, np.float32), np.zeros(N, np.int32), np.full((2, 1 + spectrum_rows(W)), 3.0)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    mem = HostMemory()
    make_in = lambda: spectrum_in(mem, {"actions": actions, "torques": torques, "reset_buf": rs}, {"actions": (12, 1), "torques": (12, 1)})
    untouched = lambda: (trace == 3.0).all() and (table == 3.0).all() and (out == 3.0).all()

    def broken(edit):
        a = make_in()
        edit(a)
        return emu.go2nn_spectrum_record(C.byref(a), p(trace), N, T, None)

    for args in ((None, N, 0, T), (trace, 0, 0, T), (trace, N, 0, 0), (trace, N, 0, (1 << 20) + 1)):
        assert emu.go2nn_spectrum_begin(p(args[0]), *args[1:], None) == EINVAL and emu.go2nn_last_error() and untouched()
    assert emu.go2nn_spectrum_record(None, p(trace), N, T, None) == EINVAL and emu.go2nn_last_error()
    assert emu.go2nn_spectrum_record(C.byref(make_in()), None, N, T, None) == EINVAL
    for n, t in ((0, T), (-1, T), (N, 0)):
        assert emu.go2nn_spectrum_record(C.byref(make_in()), p(trace), n, t, None) == EINVAL
    for field in SPECTRUM_FIELDS:
        assert broken(lambda a: setattr(getattr(a, field), "p", None)) == EINVAL and b"null" in emu.go2nn_last_error(), field
        assert broken(lambda a: setattr(getattr(a, field), "env_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
    for field in ("actions", "torques"):
        assert broken(lambda a: setattr(getattr(a, field), "comp_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error(), field
    for slots in ([0] * 12, list(range(11)) + [12], [-1] + list(range(1, 12))):
        def edit(a):
            a.joint_of_slot[:] = slots
        assert broken(edit) == EINVAL and b"joint_of_slot" in emu.go2nn_last_error(), slots
    assert untouched()
    good = (trace, N, T, W, FS, tw, table)
    for i, v in ((0, None), (5, None), (6, None), (1, 0), (2, 0), (3, 7), (3, 6), (3, 258), (3, 0), (4, 0.0), (4, -50.0), (4, float("nan")), (4, float("inf"))):
        args = list(good)
        args[i] = v
        args = [p(x) if isinstance(x, np.ndarray) or x is None else x for x in args]
        assert emu.go2nn_spectrum_welch(*args, None) == EINVAL and emu.go2nn_last_error() and untouched(), (i, v)
    for args in ((None, group, N, 2, W, out), (table, None, N, 2, W, out), (table, group, N, 2, W, None), (table, group, 0, 2, W, out), (table, group, N, 0, W, out),
                 (table, group, N, 65536, W, out), (table, group, N, 2, 9, out), (table, group, N, 2, 4, out)):
        args = [p(x) if isinstance(x, np.ndarray) or x is None else x for x in args]
        assert emu.go2nn_spectrum_reduce(*args, None) == EINVAL and emu.go2nn_last_error() and untouched()
    # and the good calls go through
    assert emu.go2nn_spectrum_begin(p(trace), N, -2, T, None) == 0 and emu.go2nn_spectrum_record(C.byref(make_in()), p(trace), N, T, None) == 0
    assert emu.go2nn_spectrum_welch(p(trace), N, T, W, FS, p(tw), p(table), None) == 0 and emu.go2nn_spectrum_reduce(p(table), p(group), N, 2, W, p(out), None) == 0


def test_spectrum_symbols_and_struct_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7 and _nn.GO2NN_ABI_VERSION == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_spectrum_begin", "go2nn_spectrum_record", "go2nn_spectrum_welch", "go2nn_spectrum_reduce"):
            assert (" T " + f + "\n") in syms, (path, f)
    names = [n for n, _ in Go2nnSpectrumIn._fields_]
    W = 64
    consts = ("GO2NN_SPECTRUM_MIN_WINDOW", "GO2NN_SPECTRUM_MAX_WINDOW", "GO2NN_SPECTRUM_MAX_STEPS", "GO2NN_SPECTRUM_CHANNELS", "GO2NN_SPECTRUM_CH_ACTION0", "GO2NN_SPECTRUM_CH_TORQUE0",
              "GO2NN_SPECTRUM_CH_RESET", "GO2NN_SPECTRUM_USED", "GO2NN_SPECTRUM_SKIPPED", "GO2NN_SPECTRUM_BIN0", "GO2NN_SPECTRUM_TRACE_ROWS(500)", "GO2NN_SPECTRUM_BINS(64)",
              "GO2NN_SPECTRUM_ROWS(64)", "GO2NN_SPECTRUM_OUT_NUM(64)", "GO2NN_SPECTRUM_OUT_N", "GO2NN_SPECTRUM_OUT_ROW0", "GO2NN_SPECTRUM_TRACE_STEP")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu", sizeof(Go2nnSpectrumIn));\n'
                   + "".join('printf(" %%d", (int)%s);\n' % c for c in consts) + "".join('printf(" %%zu", offsetof(Go2nnSpectrumIn, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(Go2nnSpectrumIn)
    assert got[1:1 + len(consts)] == [_nn.GO2NN_SPECTRUM_MIN_WINDOW, _nn.GO2NN_SPECTRUM_MAX_WINDOW, _nn.GO2NN_SPECTRUM_MAX_STEPS, GO2NN_SPECTRUM_CHANNELS, GO2NN_SPECTRUM_CH_ACTION0,
                                      GO2NN_SPECTRUM_CH_TORQUE0, GO2NN_SPECTRUM_CH_RESET, GO2NN_SPECTRUM_USED, GO2NN_SPECTRUM_SKIPPED, GO2NN_SPECTRUM_BIN0, spectrum_trace_rows(500),
                                      spectrum_bins(W), spectrum_rows(W), 1 + spectrum_rows(W), 0, 1, 0]
    assert got[1 + len(consts):] == [getattr(Go2nnSpectrumIn, n).offset for n in names] and names[:3] == list(SPECTRUM_FIELDS)
    assert spectrum_row(W, "P", 0, 0) == GO2NN_SPECTRUM_BIN0 and spectrum_row(W, "M", 1, 2, 32) == spectrum_rows(W) - 1 and SLOTS == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8, 11]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
SPEC = dict(num_envs=64, seconds=1.0, warmup_s=0.1, spectrum_window=16)          # 50 counted steps: windows at 0, 8, 16, 24, 32 — and a tail of two frames


def same(a, b):
    """two leaves of res["spectrum"]: equal, NaN where the other is NaN"""
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def check_spectrum_result(ev, res, what):
    """everything the result says, recomputed from the per-robot table: the cells' rows, and every partition of every family as the sum of the rows of ITS robots' cells —
    found from the per-env axis arrays, not from the cell index arithmetic of the evaluator"""
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_COUNT_KEYS, SPECTRUM_KEYS
    W = ev.spectrum_window
    t = ev.stable.cpu().numpy().astype(np.float64)
    st, N = res["spectrum_table"], ev.num_envs
    assert st.shape == (ev.num_cells, 1 + spectrum_rows(W)) and (ev.strace[0].cpu().numpy() == ev.steps).all()
    for c in range(ev.num_cells):
        ids = np.nonzero(ev.cell_host == c)[0]
        assert st[c, 0] == len(ids)
        for r in range(t.shape[0]):
            assert abs(st[c, 1 + r] - math.fsum(t[r, ids])) <= N * 2.0 ** -53 * math.fsum(t[r, ids]), (c, r)
    windows = (ev.steps - W) // (W // 2) + 1
    np.testing.assert_array_equal(st[:, 1 + GO2NN_SPECTRUM_USED] + st[:, 1 + GO2NN_SPECTRUM_SKIPPED], windows * st[:, 0])
    row = lambda ids: ev._spectrum_row(st[np.unique(ev.cell_host[ids])].sum(0))
    spec = res["spectrum"]
    same(spec["overall"], ev._spectrum_row(st.sum(0)))
    assert spec["overall"]["n_envs"] == N and all(res["overall"][k] == spec["overall"][k] or math.isnan(spec["overall"][k]) for k in SPECTRUM_KEYS)
    assert set(spec["overall"]) == set(SPECTRUM_KEYS) | {"%s/%s" % (k, n) for k in SPECTRUM_KEYS for n in SPECTRUM_KINDS} | set(SPECTRUM_COUNT_KEYS) | {"n_envs"}
    S = len(ev.scenarios)
    families = {"groups": [((t_, s[0]), np.nonzero(ev.group_host == ti * S + si)[0]) for ti, t_ in enumerate(ev.terrain_names) for si, s in enumerate(ev.scenarios)]}
    for key, axis, host in (("perturbations", ev.perturbations, ev.pert_host), ("sensors", ev.sensors, ev.pert_host)):
        if axis is not None:
            families[key] = [((n[0],), np.nonzero(host == pi)[0]) for pi, n in enumerate(axis)]
            families["cells"] = [((t_, s[0], n[0]), np.nonzero((ev.group_host == ti * S + si) & (host == pi))[0]) for ti, t_ in enumerate(ev.terrain_names)
                                 for si, s in enumerate(ev.scenarios) for pi, n in enumerate(axis)]
    if ev.maneuvers is not None:
        families["maneuvers"] = [((m[0],), np.nonzero(ev.man_host == mi)[0]) for mi, m in enumerate(ev.maneuvers)]
    if ev.ladder:
        families["ladder"] = [((t_, lv, s[0]), np.nonzero((ev.group_host == ti * S + si) & (ev.level_of_env == lv))[0]) for ti, t_ in enumerate(ev.terrain_names)
                              for lv in ev.levels for si, s in enumerate(ev.scenarios)]
    assert set(spec) == set(families) | {"overall"}, (set(spec), set(families))
    for fam, parts in families.items():
        total = 0
        for path, ids in parts:
            leaf = spec[fam]
            for k in path:
                leaf = leaf[k]
            if len(ids):
                same(leaf, row(ids))
            total += leaf["n_envs"]
        assert total == N, (fam, total)
    # what the figures are: shares in [0, 1], centroids inside (0, fs / 2], nothing negative
    leaves = [spec["overall"]] + [d for per in spec["groups"].values() for d in per.values()]
    for d in leaves:
        for k, v in d.items():
            if "hf_share" in k or k == "spectrum_skipped_share":
                assert math.isnan(v) or 0.0 <= v <= 1.0, (k, v)
            if "centroid_hz" in k:
                assert math.isnan(v) or 0.0 < v <= 0.5 * ev.spectrum_fs, (k, v)
            if "power" in k or "smoothness" in k:
                assert math.isnan(v) or v >= 0.0, (k, v)
    print("%s: %d cells, overall %s" % (what, ev.num_cells, {k: round(spec["overall"][k], 4) for k in SPECTRUM_KEYS + SPECTRUM_COUNT_KEYS}))


@pytest.fixture(scope="module")
def plain_runs(emu):
    """the plain evaluation on the same weights: an evaluator that never heard of the spectrum, spectrum = False, and spectrum = True with its buffers recorded step by step"""
    ac = th.small_actor_critic()
    out = {"ac": ac, "frames": []}

    def cb(ev, k, counted):
        if counted:
            b = ev.env._buf
            out["frames"].append(tuple(b[n].detach().clone().numpy() for n in SPECTRUM_FIELDS))
    for name, over, call in (("never", {}, None), ("off", dict(spectrum=False, spectrum_window=7, spectrum_cutoff_hz=-1.0), None), ("on", dict(spectrum=True), cb)):
        ev = th.make_evaluator(emu, cb=call, **dict({k: v for k, v in SPEC.items() if name == "on" or k != "spectrum_window"}, **over))
        out[name] = (ev, ev.evaluate(ac))
    yield out
    for name in ("never", "off", "on"):
        out[name][0].close()


def test_spectrum_off_changes_nothing(plain_runs):
    from go2_rl_gym_amd.utils.evaluator import format_table, results_dict, scalars
    (ev0, res0), (ev1, res1) = plain_runs["never"], plain_runs["off"]
    assert "spectrum" not in th.EVAL and ev1.spectrum is False and not hasattr(ev1, "strace") and not hasattr(ev1, "stable") and [t.name for t in ev1.tables] == []
    assert set(res1) == set(res0) and not any("spectrum" in k for k in res1) and "action_hf_share" not in res1["overall"]
    assert res1["table"].tobytes() == res0["table"].tobytes() and str(results_dict(res1)) == str(results_dict(res0))
    assert format_table(res1) == format_table(res0) and str(scalars(res1)) == str(scalars(res0))
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    for task in ("go2_flat", "go2_cts"):
        e = task_registry.get_cfgs(task)[1].evaluation
        assert (e.spectrum, e.spectrum_window, e.spectrum_cutoff_hz, e.spectrum_max_bytes) == (False, 64, 10.0, 512 << 20)
    assert get_args(["--spectrum"]).spectrum is True and get_args([]).spectrum is False
    _, cfg = update_cfg_from_args(None, task_registry.get_cfgs("go2_flat")[1], get_args(["--spectrum", "--robust"]))
    assert cfg.evaluation.spectrum is True and cfg.evaluation.perturbations and task_registry.get_cfgs("go2_flat")[1].evaluation.spectrum is False


def test_spectrum_on_leaves_scores_alone_and_matches_the_recorded_buffers(plain_runs):
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_KEYS
    (_, res0), (ev, res) = plain_runs["never"], plain_runs["on"]
    assert res["table"].tobytes() == res0["table"].tobytes() and ev.spectrum is True and [t.name for t in ev.tables] == ["spectrum"]
    assert {k: v for k, v in res["overall"].items() if k in res0["overall"]} == res0["overall"] and set(res["overall"]) - set(res0["overall"]) == set(SPECTRUM_KEYS)
    assert {k: res[k] for k in ("groups", "steps", "dt", "mode", "scenarios", "terrain_names")} == {k: res0[k] for k in ("groups", "steps", "dt", "mode", "scenarios", "terrain_names")}
    assert set(res) - set(res0) == {"spectrum", "spectrum_table", "spectrum_cells", "spectrum_settings", "spectrum_psd"}
    frames = plain_runs["frames"]
    assert len(frames) == ev.steps == 50 and ev.spectrum_fs == 50.0 and res["spectrum_settings"] == {"window": 16, "cutoff_hz": 10.0, "fs": 50.0}
    actions, torques, reset = (np.stack([f[i] for f in frames]) for i in range(3))
    ref = reference(actions, torques, reset != 0, 16, fs=ev.spectrum_fs)
    assert len(ref["windows"]) == 5
    check_table(ev.stable.cpu().numpy(), ref, 16, "evaluator")
    trace = ev.strace.cpu().numpy()
    check_trace(trace, np.concatenate([actions[:WARMUP], actions]), np.concatenate([torques[:WARMUP], torques]), np.concatenate([reset[:WARMUP], reset]) != 0, ev.steps)
    assert ref["used"].sum() > 0 and np.isfinite(res["overall"]["action_hf_share"]) and res["overall"]["action_power"] > 0


def test_spectrum_partitions_and_outputs(plain_runs, tmp_path):
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_COUNT_KEYS, SPECTRUM_KEYS, format_table, results_dict, scalars, write_results
    from go2_rl_gym_amd.utils.recorder import read_spectrum
    ev, res = plain_runs["on"]
    check_spectrum_result(ev, res, "plain evaluation")
    assert res["spectrum_cells"] == ["terrain", "scenario"] and set(res["spectrum"]) == {"overall", "groups"}
    tags = dict(scalars(res))
    assert all(tags["Eval/spectrum/" + k] == res["spectrum"]["overall"][k] or math.isnan(tags["Eval/spectrum/" + k]) for k in SPECTRUM_KEYS + SPECTRUM_COUNT_KEYS)
    assert "Eval/spectrum/torque_hf_share/calf" in tags and "Eval/lin_vel_err" in tags
    assert tags["Eval/spectrum/plane/forward_1.0/action_power"] == res["spectrum"]["groups"]["plane"]["forward_1.0"]["action_power"]
    import yaml
    path = write_results(str(tmp_path), 3, res)
    back = yaml.safe_load(open(path))
    assert set(back["spectrum"]) == {"overall", "groups", "window", "cutoff_hz", "fs"} and (back["spectrum"]["window"], back["spectrum"]["cutoff_hz"], back["spectrum"]["fs"]) == (16, 10.0, 50.0)
    assert back["spectrum"]["groups"]["plane"]["stand"]["n_envs"] == 16 and back["spectrum"]["overall"]["spectrum_windows"] == res["spectrum"]["overall"]["spectrum_windows"]
    assert results_dict(res, 3)["spectrum"]["overall"]["action_centroid_hz"] == res["spectrum"]["overall"]["action_centroid_hz"]
    z = read_spectrum(os.path.join(str(tmp_path), "eval_results", "spectrum_3.npz"))
    K = spectrum_bins(16)
    assert z["psd"].shape == (ev.num_cells, 2, 3, K) and z["signals"] == list(SPECTRUM_SIGNALS) and z["kinds"] == list(SPECTRUM_KINDS) and len(z["cell_names"]) == ev.num_cells
    assert (z["window"], z["cutoff_hz"], z["fs"]) == (16, 10.0, 50.0) and z["cell_names"][0] == "plane/forward_1.0"
    np.testing.assert_array_equal(z["freqs"], np.arange(K) * 50.0 / 16)
    st = res["spectrum_table"]
    np.testing.assert_array_equal(z["psd"][2, 1, 0], st[2, 1 + spectrum_row(16, "P", 1, 0):1 + spectrum_row(16, "P", 1, 0) + K] / (4.0 * st[2, 1 + GO2NN_SPECTRUM_USED]))
    text = format_table(res)
    assert "action_hf_share" in text and "torque_smoothness" in text and len(text.splitlines()) == 2 * (1 + len(ev.groups) + 1) + 1


@pytest.mark.parametrize("key,value", [("spectrum_window", 15), ("spectrum_window", 6), ("spectrum_window", 258), ("spectrum_window", 16.0), ("spectrum_cutoff_hz", 0.0),
                                       ("spectrum_cutoff_hz", 25.5), ("spectrum_cutoff_hz", float("nan")), ("spectrum_max_bytes", 0), ("spectrum_max_bytes", 1000)])
def test_bad_settings_name_their_key(emu, key, value):
    with pytest.raises(ValueError, match=key):
        th.make_evaluator(emu, num_envs=12, seconds=0.4, warmup_s=0.0, spectrum=True, **{key: value})


MODES = {
    "perturbations": dict(perturbations=[["nominal", {}], ["push_front_0.5", {"dv": [0.5, 0.0, 0.0]}], ["payload_2kg", {"added_mass": 2.0}]],
                          push_first_s=0.2, push_period_s=0.4, push_window_s=0.3),
    "maneuvers+gait": dict(maneuvers=[["start_1.0", [[0.0, 0.0, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0]]], ["turn_flip", [[0.0, 0.0, 0.0, 1.0], [0.4, 0.0, 0.0, -1.0]]]],
                           maneuver_window_s=0.3, maneuver_hold_s=0.1, gait=True),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_spectrum_next_to_a_mode(emu, mode):
    """an add-on: next to an extra axis (and next to the gait scorer) the mode's own results are those of the run without it, byte for byte, and every partition the mode
    reports is the sum of its cells"""
    over = dict(SPEC, **MODES[mode])
    ac = th.small_actor_critic()
    base = th.make_evaluator(emu, **over)
    res0 = base.evaluate(ac)
    base.close()
    ev = th.make_evaluator(emu, spectrum=True, **over)
    res = ev.evaluate(ac)
    own = ["robust_table"] if mode == "perturbations" else ["maneuver_table", "gait_table"]
    assert res["table"].tobytes() == res0["table"].tobytes() and all(res[k].tobytes() == res0[k].tobytes() for k in own)
    check_spectrum_result(ev, res, mode)
    assert mode.split("+")[0] in res["spectrum"] and ("cells" in res["spectrum"]) == (mode == "perturbations")
    again = ev.evaluate(ac)
    assert again["spectrum_table"].tobytes() == res["spectrum_table"].tobytes()
    ev.close()


def test_intervals_run_next_to_the_spectrum_and_do_not_move(emu):
    """--ci and --ci_all next to --spectrum: every existing interval is that of the run without it; the spectrum figures get none"""
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_KEYS
    over = dict(SPEC, gait=True, bootstrap=40, bootstrap_all=True)
    ac = th.small_actor_critic()
    base = th.make_evaluator(emu, **over)
    res0 = base.evaluate(ac)
    base.close()
    ev = th.make_evaluator(emu, spectrum=True, **over)
    res = ev.evaluate(ac)
    assert str(res["overall"]["ci"]) == str(res0["overall"]["ci"]) and str(res["gait"]) == str(res0["gait"]) and set(res["bootstrap"]["tables"]) == {"gait"}
    assert res["bootstrap"]["table"].tobytes() == res0["bootstrap"]["table"].tobytes() and not hasattr(ev, "sboot") and "spectrum" not in ev.boot_outs
    assert "ci" not in res["spectrum"]["overall"] and not set(SPECTRUM_KEYS) & set(res["bootstrap"]["metrics"])
    ev.close()


def test_metric_acceptance_and_ci_refusal():
    from go2_rl_gym_amd.scripts.evaluate import HIGHER_IS_BETTER, best_checkpoint, check_ci_metric, check_metric, evaluate, higher_is_better, metric_value
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_KEYS
    assert not set(SPECTRUM_KEYS) & set(HIGHER_IS_BETTER) and not any(higher_is_better(k) for k in SPECTRUM_KEYS + ("action_hf_share/calf",))
    rows = [{"checkpoint": "a", "overall": {"action_hf_share": 0.3, "torque_power": float("nan")}, "spectrum": {"overall": {"action_hf_share": 0.3, "action_hf_share/calf": 0.5}}},
            {"checkpoint": "b", "overall": {"action_hf_share": 0.1, "torque_power": 2.0}, "spectrum": {"overall": {"action_hf_share": 0.1, "action_hf_share/calf": 0.7}}}]
    assert best_checkpoint(rows, "action_hf_share")["checkpoint"] == "b" and best_checkpoint(rows, "torque_power")["checkpoint"] == "b"
    assert best_checkpoint(rows, "action_hf_share/calf")["checkpoint"] == "a" and metric_value(rows[1], "action_hf_share/calf") == 0.7
    for k in SPECTRUM_KEYS:
        check_metric(k)
    for k in ("spectrum_windows", "spectrum_skipped_share"):
        with pytest.raises(ValueError, match=k):
            check_metric(k)
    for ci_all in (False, True):
        for k in ("action_hf_share", "torque_centroid_hz/thigh"):
            with pytest.raises(ValueError, match="no replicates"):
                check_ci_metric(k, types.SimpleNamespace(ci=100, ci_all=ci_all, spectrum=True))
    check_ci_metric("lin_vel_err", types.SimpleNamespace(ci=100, ci_all=False, spectrum=True))
    # the script refuses before anything runs: no run directory exists here
    with pytest.raises(ValueError, match="no replicates"):
        evaluate(["--task", "go2_flat", "--spectrum", "--ci", "--all_checkpoints", "--metric", "action_hf_share", "--sim_device", "cpu", "--rl_device", "cpu", "--headless"],
                 log_root="/nonexistent")


def test_cli_ranks_checkpoints_by_a_spectrum_figure(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints --spectrum --metric action_hf_share: lower is better"""
    import copy
    import json
    from helpers import load_oracle
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import SPECTRUM_KEYS
    from go2_rl_gym_amd.utils.recorder import read_spectrum
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s, e.spectrum_window = 48, 0.6, 0.1, 8
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    capsys.readouterr()
    out = evaluate(base + ["--spectrum", "--all_checkpoints", "--metric", "action_hf_share"], log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    names = [r["checkpoint"] for r in out["checkpoints"]]
    assert names == ["model_0.pt", "model_1.pt"] and out["metric"] == "action_hf_share" and out["best"] in names
    assert out["best_value"] == min(r["overall"]["action_hf_share"] for r in out["checkpoints"]) and 0.0 <= out["best_value"] <= 1.0
    for r in out["checkpoints"]:
        assert set(SPECTRUM_KEYS) < set(r["overall"]) and set(r["spectrum"]) == {"overall", "groups"} and set(r["spectrum"]["groups"]) == set(r["groups"])
    text = capsys.readouterr().out
    assert "torque_centroid_hz" in text and json.loads([l for l in text.splitlines() if l.startswith("{")][-1])["best"] == out["best"]
    files = [l.split(": ", 1)[1] for l in text.splitlines() if l.startswith("spectrum: ")]
    assert len(files) == 2 and read_spectrum(files[1])["psd"].shape[1:] == (2, 3, 5)
