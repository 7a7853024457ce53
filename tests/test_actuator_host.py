"""The evaluator's actuator loads on the CPU: the host build of the go2nn_actuator_* kernels (include/go2nn.h) against a float64 restatement written here — over the whole
record of a robot at once, not step by step as the kernel works — on a scripted sequence that meets every edge of the rule, the reduce against math.fsum, the bootstrap
against the Python-integer restatement of the draws, the argument checks, the struct layout, and PolicyEvaluator with `actuators` on the oracle + the host build: nothing
changes with the flag off, nothing else moves with it on, the table of every recorded robot is the rule applied to its trace, every partition of every mode is the pool
of its cells, and scripts/evaluate.py ranks by the new figures."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, load_nn_emu, reduce_groups, reduce_twice
import test_bootstrap_host as tb
import test_bootstrap_modes_host as tm
import test_eval_host as th
from test_gait_host import store3
from test_robust_host import HostMemory
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd._nn import (ACTUATOR_ENV_ROWS, ACTUATOR_FIELDS, ACTUATOR_FOOT_ROWS, ACTUATOR_JOINT_ROWS, GO2NN_ACTUATOR_FOOT0, GO2NN_ACTUATOR_JOINT0, GO2NN_ACTUATOR_NUM,
                                GO2NN_ACTUATOR_OUT_NUM, Go2nnActuatorIn, actuator_out_col, actuator_row)

EINVAL = -22
START, STEPS = -3, 37          # three warm-up calls, then the counted steps: 40 calls
CALLS = STEPS - START
BODIES = 19
FOOT_BODY = (10, 6, 18, 14)    # FR, FL, RR, RL: not the simulator's order — the kernel may not assume one
THR = 2.5                      # [N] contact threshold, not the default and exact in fp32: a force EQUAL to it can be scripted
# limits and a saturation share that are not the Go2's and whose products are exact in fp32: the kernel must read them, and a sample EQUAL to a threshold can be scripted
SAT = 0.75
TAU_LIM = np.asarray([16.0, 24.0, 32.0] * 4, np.float32)
VEL_LIM = np.asarray([20.0, 28.0, 12.0] * 4, np.float32)
TAU_THR, VEL_THR = np.float32(SAT) * TAU_LIM, np.float32(SAT) * VEL_LIM          # 12 / 18 / 24 N m, 15 / 21 / 9 rad/s
POS_LO = np.asarray([-1.0, -1.5, -2.75] * 4, np.float32)
POS_HI = np.asarray([1.0, 3.5, -0.75] * 4, np.float32)
COUNT_ROWS = ("tau_sat", "vel_sat", "fz_frames")
EXACT_ROWS = ("tau_peak", "vel_peak", "margin_min", "fz_peak")
SUM_ROWS = ("tau_sq", "work_pos", "work_neg", "fz_sum")
# A float sum is a running fp32 sum of at most STEPS terms: every addition rounds once, 2^-24 relative to a partial sum that is at most sum |term|, and every term carries
# its own rounding (a product: one; the planar speed — two products, a sum, a square root —: 2.5) relative to itself: (STEPS + 2.5) 2^-24 sum |term| in all, below the bound
# of tests/test_gait_host.py stated here for STEPS >= 3.
FLOAT_BOUND = lambda steps, mag: steps * 2.0 ** -23 * mag
CASES = ("torque_equals_threshold", "torque_one_ulp_below", "speed_equals_threshold", "speed_one_ulp_below", "peak_on_warmup_frame", "peak_on_reset_frame",
         "reset_on_first_counted_frame", "every_counted_frame_a_reset", "joint_past_a_limit", "margin_minimum_on_first_used_frame", "margin_minimum_on_last_used_frame",
         "only_negative_work", "foot_never_in_contact", "force_equals_contact_threshold", "never_moves")
ENV0_CASES = CASES[:6]         # what a single robot (N = 1) shows


def below(x):
    return np.nextafter(np.float32(x), np.float32(0.0))


def script(N, seed=0):
    """-> {"tau", "q", "qd" [CALLS, N, 12], "fz" [CALLS, N, 4], "vxy" [CALLS, N, 2] fp32, "reset" [CALLS, N] bool}, and the CASES it was written to meet.  Robot e < 8 follows
    the pattern written for it below; from the ninth on everything is random, resets and saturated samples included"""
    rng = np.random.default_rng(seed + N)
    tau = rng.uniform(-10.0, 10.0, (CALLS, N, 12)).astype(np.float32)          # below every torque threshold
    qd = rng.uniform(-8.0, 8.0, (CALLS, N, 12)).astype(np.float32)             # below every speed threshold
    q = (POS_LO + 0.1 + rng.random((CALLS, N, 12)) * (POS_HI - POS_LO - 0.2)).astype(np.float32)
    fz = np.where(rng.random((CALLS, N, 4)) < 0.5, rng.uniform(3.0, 80.0, (CALLS, N, 4)), rng.uniform(-0.5, 2.4, (CALLS, N, 4))).astype(np.float32)
    vxy = rng.normal(0.0, 1.0, (CALLS, N, 2)).astype(np.float32)
    reset = np.zeros((CALLS, N), bool)
    at = lambda step: step - START          # the call of a counted step
    wrote = set()
    for e in range(N):
        if e >= 8:
            reset[at(0):, e] = rng.random(STEPS) < 0.15
            hot = rng.random((STEPS, 12)) < 0.1
            tau[at(0):, e][hot] = (rng.choice([-1.0, 1.0], hot.sum()) * rng.uniform(0.7, 1.0, hot.sum()) * np.broadcast_to(TAU_LIM, hot.shape)[hot]).astype(np.float32)
            fast = rng.random((STEPS, 12)) < 0.1
            qd[at(0):, e][fast] = (rng.choice([-1.0, 1.0], fast.sum()) * rng.uniform(0.7, 1.0, fast.sum()) * np.broadcast_to(VEL_LIM, fast.shape)[fast]).astype(np.float32)
            continue
        k = e % 8
        if k == 0:
            tau[at(5), e, 0], tau[at(6), e, 0] = -TAU_THR[0], below(TAU_THR[0])          # at the threshold (negative: |tau| counts), one ulp below it
            qd[at(7), e, 1], qd[at(8), e, 1] = VEL_THR[1], -below(VEL_THR[1])
            tau[1, e, 2], qd[1, e, 2], fz[1, e, 3] = 31.0, 11.5, 900.0                    # a warm-up call: larger than anything counted
            reset[at(10), e] = True
            tau[at(10), e, 2], qd[at(10), e, 2], fz[at(10), e, 3], q[at(10), e, 2] = -30.0, -11.0, 800.0, POS_HI[2] + 1.0          # the post-reset frame: not taken
            wrote |= set(ENV0_CASES)
        elif k == 1:
            reset[at(0), e] = True
            q[at(0), e, :] = POS_LO + 0.001          # (would be every joint's smallest margin)
            q[at(1), e, 3] = POS_LO[3] + 0.01        # the first USED frame holds joint 3's minimum
            q[at(STEPS - 1), e, 4] = POS_HI[4] - 0.005
            wrote |= {"reset_on_first_counted_frame", "margin_minimum_on_first_used_frame", "margin_minimum_on_last_used_frame"}
        elif k == 2:
            reset[at(0):, e] = True
            wrote.add("every_counted_frame_a_reset")
        elif k == 3:
            q[at(12), e, 5] = POS_HI[5] + 0.125
            tau[:, e, 6], qd[:, e, 6] = np.abs(tau[:, e, 6]) + 0.5, -np.abs(qd[:, e, 6]) - 0.5
            wrote |= {"joint_past_a_limit", "only_negative_work"}
        elif k == 4:
            fz[:, e, 2] = rng.uniform(-0.5, 2.0, CALLS)
            fz[at(9), e, 1] = THR
            wrote |= {"foot_never_in_contact", "force_equals_contact_threshold"}
        elif k == 5:
            vxy[:, e] = 0.0
            wrote.add("never_moves")
    return {"tau": tau, "q": q, "qd": qd, "fz": fz, "vxy": vxy, "reset": reset}, wrote


class Reference:
    """the rule of include/go2nn.h in float64, over the whole COUNTED record of every robot at once: tau, q, qd [S, N, 12], fz [S, N, 4], vxy [S, N, 2], reset [S, N].
    -> rows[name] ([N], [N, 12] or [N, 4]), mag[name] (sum |term|) for the float sums, seen (the CASES the record meets).  |tau|, |qd|, q - lo and hi - q are formed in
    np.float32, as the kernel forms them: the counting rows, the peaks and the margin are exact"""

    def __init__(self, tau, q, qd, fz, vxy, reset, tau_thr=TAU_THR, vel_thr=VEL_THR, lo=POS_LO, hi=POS_HI, thr=THR):
        f32 = lambda a: np.asarray(a, np.float32)
        tau, q, qd, fz, vxy, reset = f32(tau), f32(q), f32(qd), f32(fz), f32(vxy), np.asarray(reset, bool)
        S, N = reset.shape
        use = ~reset
        self.rows, self.mag, self.seen = {}, {}, set()
        self.rows["used"] = use.sum(0).astype(np.float64)
        speed = np.hypot(vxy[..., 0].astype(np.float64), vxy[..., 1].astype(np.float64))
        fsum = lambda x, w: np.asarray([[math.fsum(x[w[:, e], e, j]) for j in range(x.shape[2])] for e in range(N)])
        self.rows["dist"] = self.mag["dist"] = fsum(speed[..., None], use)[:, 0]
        at, av = np.abs(tau), np.abs(qd)
        margin = np.minimum(q - f32(lo), f32(hi) - q)          # fp32 differences, as the kernel's
        assert margin.dtype == np.float32 and at.dtype == np.float32
        u3 = use[:, :, None]
        live = use.any(0)[:, None]          # a robot without a used frame keeps the zeros go2nn_actuator_begin wrote
        self.rows["tau_peak"] = np.where(live, np.where(u3, at, -np.inf).astype(np.float64).max(0), 0.0)
        self.rows["vel_peak"] = np.where(live, np.where(u3, av, -np.inf).astype(np.float64).max(0), 0.0)
        self.rows["margin_min"] = np.where(live, np.where(u3, margin, np.inf).astype(np.float64).min(0), 0.0)
        self.rows["tau_sat"], self.rows["vel_sat"] = ((at >= f32(tau_thr)) & u3).sum(0).astype(np.float64), ((av >= f32(vel_thr)) & u3).sum(0).astype(np.float64)
        t64, p = tau.astype(np.float64), tau.astype(np.float64) * qd.astype(np.float64)
        for name, term in (("tau_sq", t64 * t64), ("work_pos", np.maximum(p, 0.0)), ("work_neg", np.maximum(-p, 0.0))):
            self.rows[name] = self.mag[name] = fsum(term, use)
        self.rows["fz_peak"] = np.maximum(np.where(u3, fz, -np.inf).astype(np.float64).max(0), 0.0)          # (the row starts at 0: a foot that only ever pulls reports 0)
        down = (fz > np.float32(thr)) & u3
        self.rows["fz_frames"] = down.sum(0).astype(np.float64)
        self.rows["fz_sum"] = self.mag["fz_sum"] = np.asarray([[math.fsum(fz[down[:, e, f], e, f].astype(np.float64)) for f in range(4)] for e in range(N)])
        # which edges of the rule the record meets
        for name, a, thr_ in (("torque", at, f32(tau_thr)), ("speed", av, f32(vel_thr))):
            if ((a == thr_) & u3).any():
                self.seen.add(name + "_equals_threshold")
            if ((a == np.nextafter(thr_, np.float32(0))) & u3).any():
                self.seen.add(name + "_one_ulp_below")
        if (reset & (at.max(2) > np.where(u3, at, 0).max((0, 2))[None])).any():
            self.seen.add("peak_on_reset_frame")
        if reset[0].any():
            self.seen.add("reset_on_first_counted_frame")
        if reset.all(0).any():
            self.seen.add("every_counted_frame_a_reset")
        if (self.rows["margin_min"] < 0).any():
            self.seen.add("joint_past_a_limit")
        first, last = use.argmax(0), S - 1 - use[::-1].argmax(0)          # the first and the last used frame of every robot
        for e in np.nonzero(use.any(0))[0]:
            for name, frame in (("first", first[e]), ("last", last[e])):
                rest = use[:, e].copy()
                rest[frame] = False
                if rest.any() and (margin[frame, e] < margin[rest, e].min(0)).any():
                    self.seen.add("margin_minimum_on_%s_used_frame" % name)
        if ((self.rows["work_pos"] == 0) & (self.rows["work_neg"] > 0)).any():
            self.seen.add("only_negative_work")
        if ((self.rows["fz_frames"] == 0) & (self.rows["used"] > 0)[:, None]).any():
            self.seen.add("foot_never_in_contact")
        if ((fz == np.float32(thr)) & u3).any():
            self.seen.add("force_equals_contact_threshold")
        if ((self.rows["dist"] == 0) & (self.rows["used"] > 0)).any():
            self.seen.add("never_moves")


def table_rows(table):
    """the table [NUM, N] as the Reference names it -> {name: [N], [N, 12] or [N, 4]} (float64)"""
    t = np.asarray(table, np.float64)
    d = {k: t[actuator_row(k)] for k in ACTUATOR_ENV_ROWS}
    d.update({k: np.stack([t[actuator_row(k, j)] for j in range(12)], 1) for k in ACTUATOR_JOINT_ROWS})
    d.update({k: np.stack([t[actuator_row(k, f)] for f in range(4)], 1) for k in ACTUATOR_FOOT_ROWS})
    return d


def check_rows(got, ref, steps, what):
    """the table's rows of some robots against a Reference of the same robots: counts, peaks and margins exactly, the float sums within FLOAT_BOUND -> largest gap / bound"""
    for k in ("used",) + COUNT_ROWS + EXACT_ROWS:
        np.testing.assert_array_equal(got[k], ref.rows[k], err_msg="%s: %s" % (what, k))
    worst = 0.0
    for k in ("dist",) + SUM_ROWS:
        gap, bound = np.abs(got[k] - ref.rows[k]), FLOAT_BOUND(steps, ref.mag[k])
        worst = max(worst, float((gap / np.maximum(bound, 1e-300)).max()))
        assert (gap <= bound).all(), (what, k, gap.max(), bound.max())
    idle = ref.rows["used"] == 0          # a robot without a used frame holds zeros in every row
    for k, v in got.items():
        assert k == "step" or not v[idle].any(), (what, k)
    return worst


def buffers_at(d, call, N):
    """the simulator's buffers after the script's call `call`: every body that is no foot, and every force component but z, holds values the kernel must not read"""
    ds = np.stack([d["q"][call], d["qd"][call]], 2)
    cf, rs = np.full((N, BODIES, 3), 1e6, np.float32), np.full((N, 13), 1e6, np.float32)
    for f, b in enumerate(FOOT_BODY):
        cf[:, b, 2] = d["fz"][call, :, f]
    rs[:, 7:9] = d["vxy"][call]
    return {"dof_state": ds, "torques": d["tau"][call], "contact_forces": cf, "root_states": rs, "reset_buf": d["reset"][call].astype(np.uint8)}


def store(a, layout):
    """a logical [N, ...] array as the libraries store it -> (flat storage, its strides in elements, in the logical axes' order): row-major as the oracle keeps it, or
    field-major as the HIP simulator does (the whole shape reversed: env stride 1)"""
    if a.ndim == 3:
        return store3(a, layout)
    if a.ndim == 1:
        return np.ascontiguousarray(a), 1
    return (np.ascontiguousarray(a.T), 1, a.shape[0]) if layout == 1 else (np.ascontiguousarray(a), a.shape[1], 1)


def actuator_in(mem, h, strides, tau_thr=TAU_THR, vel_thr=VEL_THR, thr=THR):
    a = Go2nnActuatorIn()
    for k in ACTUATOR_FIELDS:
        f = getattr(a, k)
        f.p, f.env_stride, f.comp_stride = mem.ptr(h[k]), strides[k][0], (strides[k][-1] if len(strides[k]) > 1 else 0)
    a.dof_state.comp_stride, a.dof_vel_offset, a.contact_body_stride = strides["dof_state"][1], strides["dof_state"][2], strides["contact_forces"][1]
    a.foot_body[:], a.contact_threshold = FOOT_BODY, thr
    a.pos_lo[:], a.pos_hi[:], a.tau_sat_thr[:], a.vel_sat_thr[:] = POS_LO.tolist(), POS_HI.tolist(), np.asarray(tau_thr).tolist(), np.asarray(vel_thr).tolist()
    return a


def run_script(lib, mem, N, layout, seed=0):
    """the scripted sequence on `lib` with its buffers in `mem` -> (table fp32 [NUM, N], Reference, the script's own CASES)"""
    d, wrote = script(N, seed)
    h, strides = {}, {}
    for k, a in buffers_at(d, 0, N).items():
        flat, *strides[k] = store(a, layout)
        h[k] = mem.put(flat)
    a = actuator_in(mem, h, strides)
    table = mem.put(np.full((GO2NN_ACTUATOR_NUM, N), 7.0, np.float32))
    assert lib.go2nn_actuator_begin(C.c_void_p(mem.ptr(table)), N, START, mem.stream) == 0, lib.go2nn_last_error()
    got = mem.get(table).reshape(GO2NN_ACTUATOR_NUM, N)
    assert (got[0] == START).all() and not got[1:].any()
    for call in range(CALLS):
        for k, v in buffers_at(d, call, N).items():
            mem.set(h[k], store(v, layout)[0])
        assert lib.go2nn_actuator_accumulate(C.byref(a), C.c_void_p(mem.ptr(table)), N, mem.stream) == 0, lib.go2nn_last_error()
        if call == -START - 1:          # the warm-up is over: nothing but the counter has moved
            got = mem.get(table).reshape(GO2NN_ACTUATOR_NUM, N)
            assert (got[0] == 0).all() and not got[1:].any()
    c = slice(-START, None)
    ref = Reference(d["tau"][c], d["q"][c], d["qd"][c], d["fz"][c], d["vxy"][c], d["reset"][c])
    if (np.abs(d["tau"][:-START]).max((0, 2)) > ref.rows["tau_peak"].max(1)).any():
        ref.seen.add("peak_on_warmup_frame")
    return mem.get(table).reshape(GO2NN_ACTUATOR_NUM, N), ref, wrote


def check_table(table, ref, wrote, N, what):
    want = set(CASES) if N >= 8 else set(ENV0_CASES)
    assert wrote >= want and ref.seen >= want, want - ref.seen          # the script holds every edge it was written for, and the record shows it
    got = table_rows(table)
    assert (got["step"] == STEPS).all()
    worst = check_rows(got, ref, STEPS, what)
    print("%s: %d used frames, %d saturated torque samples, %d robots without a used frame; largest float-sum gap / bound (%d * 2^-23 * sum|term|) %.4f"
          % (what, ref.rows["used"].sum(), ref.rows["tau_sat"].sum(), (ref.rows["used"] == 0).sum(), STEPS, worst))
    assert ref.rows["tau_sat"].sum() > 0 and ref.rows["vel_sat"].sum() > 0 and ref.rows["fz_frames"].sum() > 0 and (ref.rows["margin_min"] > 0).any()


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_accumulate_against_float64(emu, N, layout):
    table, ref, wrote = run_script(emu, HostMemory(), N, layout)
    check_table(table, ref, wrote, N, "host N=%d layout=%d" % (N, layout))
    got = table_rows(table)
    # the hand-written figures of robot 0: the sample AT the threshold counts and the one an ulp below does not; neither the warm-up's nor the reset frame's peak is taken
    assert got["tau_sat"][0, 0] == 1 and got["vel_sat"][0, 1] == 1 and got["used"][0] == STEPS - 1 and got["tau_peak"][0, 2] <= 10.0 and got["fz_peak"][0, 3] <= 80.0
    if N >= 8:
        assert got["used"][1] == STEPS - 1 and abs(got["margin_min"][1, 3] - 0.01) < 1e-6 and abs(got["margin_min"][1, 4] - 0.005) < 1e-6
        assert got["used"][2] == 0 and got["margin_min"][3, 5] == -0.125 and got["work_pos"][3, 6] == 0 and got["work_neg"][3, 6] > 0
        assert got["fz_frames"][4, 2] == 0 and got["fz_sum"][4, 2] == 0 and got["dist"][5] == 0 and got["used"][5] == STEPS


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def reduce_case(N, G, seed=5):
    """a table of both signs (a margin can be negative) whose USED row holds zeros, and group ids of which some lie outside [0, G)"""
    rng = np.random.default_rng(seed + N)
    table = rng.normal(0, 30, (GO2NN_ACTUATOR_NUM, N)).astype(np.float32)
    table[actuator_row("used")] = (rng.random(N) < 0.7) * rng.integers(1, 500, N)
    group = reduce_groups(rng, N, G)
    if N == 1:          # the one robot: with a used frame, inside the only group for G = 1 and outside every group for G = 5
        table[actuator_row("used")], group[:] = 7.0, (0 if G == 1 else G + 1)
    return table, group


def terms(table):
    """go2nn_actuator_reduce's term of every robot and column, float64 [N, OUT_NUM]: 1, USED > 0, then every row but STEP"""
    t = np.asarray(table, np.float64)
    return np.concatenate([np.ones((1, t.shape[1])), (t[actuator_row("used")] > 0)[None].astype(np.float64), t[1:]]).T.copy()


def check_reduce(out, table, group, G, N, what):
    """the counts exactly; every fp64 sum to N roundings of the running sum"""
    t, worst = terms(table), 0.0
    assert actuator_out_col("n") == 0 and actuator_out_col("n_used") == 1 and actuator_out_col("used") == 2 and actuator_out_col("fz_frames", 3) == GO2NN_ACTUATOR_OUT_NUM - 1
    for g in range(G):
        ids = np.nonzero(group == g)[0]
        assert out[g, 0] == len(ids) and out[g, 1] == (table[actuator_row("used"), ids] > 0).sum()
        for c in range(2, GO2NN_ACTUATOR_OUT_NUM):
            x = [float(v) for v in t[ids, c]]
            gap, bound = abs(out[g, c] - math.fsum(x)), N * 2.0 ** -53 * math.fsum(abs(v) for v in x)
            assert gap <= bound, (g, c, gap, bound)
            worst = max(worst, gap / max(bound, 1e-300))
    assert N == 1 or (((group < 0) | (group >= G)).any() and (G == 1 or ((group == 1).sum() == 0 and not out[1].any())))
    print("%s: largest reduce gap / bound %.3f" % (what, worst))


def emu_reduce(emu, table, group, G):
    out = np.full((G, GO2NN_ACTUATOR_OUT_NUM), -1.0)
    assert emu.go2nn_actuator_reduce(C.c_void_p(table.ctypes.data), C.c_void_p(group.ctypes.data), table.shape[1], G, C.c_void_p(out.ctypes.data), None) == 0, emu.go2nn_last_error()
    return out


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_reduce_against_fsum(emu, N, G):
    table, group = reduce_case(N, G)
    out = reduce_twice(lambda *a: emu.go2nn_actuator_reduce(*a, None), table, group, G, GO2NN_ACTUATOR_OUT_NUM)
    check_reduce(out, table, group, G, N, "host N=%d G=%d" % (N, G))
    if N == 1:          # the robot's own row in its group, nothing in a group it is not in
        assert (out[0] == terms(table)[0]).all() and out[0, 0] == out[0, 1] == 1 if G == 1 else not out.any()


FAMILY = tm.Family("actuator", ACTUATOR_ENV_ROWS + tuple("%s/%d" % (r, j) for j in range(12) for r in ACTUATOR_JOINT_ROWS)
                   + tuple("%s/%d" % (r, f) for f in range(4) for r in ACTUATOR_FOOT_ROWS), GO2NN_ACTUATOR_OUT_NUM, 0, ())
BOOT_BS = (1, 255, 257)
_BOOT = {}


def bootstrap_case(N):
    """the table at `N` (tests/test_bootstrap_host.py's cell sizes: an empty cell, one robot, ragged Philox blocks, a cell wider than a workgroup), its cells and the
    restatement of the largest B from the Python-integer draws -> shared, never written"""
    if N not in _BOOT:
        table = reduce_case(N, 1, seed=23)[0]
        table[actuator_row("dist"), 0], table[actuator_row("fz_sum", 2), N - 1] = 3.0e37, -3.0e37
        start, envs, per_cell = tm.draws(N)
        ref = tm.restate(terms(table), per_cell)
        for a in (table, ref):
            a.setflags(write=False)
        _BOOT[N] = (table, start, envs, ref)
    return _BOOT[N]


def check_bootstrap(be, N, B):
    table, start, envs, ref = bootstrap_case(N)
    assert max(BOOT_BS) <= ref.shape[0] and len(FAMILY.rows) == GO2NN_ACTUATOR_NUM
    out = tm.bootstrap(be, FAMILY, table, start, envs, B, tm.SEED)
    assert out.shape == ref[:B].shape and out.tobytes() == ref[:B].tobytes(), np.nanmax(np.abs(out - ref[:B]))
    sizes = np.diff(start)
    assert (out[:, :, 0] == sizes[None]).all() and (out[:, :, 1] <= sizes[None]).all() and not out[:, sizes == 0].any()


@pytest.mark.parametrize("B", BOOT_BS)
@pytest.mark.parametrize("N", sorted(tb.CASES))
def test_bootstrap_equals_the_restatement_bit_for_bit(emu, N, B):
    check_bootstrap(tm.HostBackend(emu), N, B)


def test_bootstrap_replicate_does_not_depend_on_B_and_refusals(emu):
    be = tm.HostBackend(emu)
    table, start, envs, _ = bootstrap_case(300)
    big, small = tm.bootstrap(be, FAMILY, table, start, envs, 256, 5), tm.bootstrap(be, FAMILY, table, start, envs, 64, 5)
    assert big[:64].tobytes() == small.tobytes() and tm.bootstrap(be, FAMILY, table, start, envs, 64, 6).tobytes() != small.tobytes()
    tm._REF.setdefault((be.name, "actuator", 37), bootstrap_case(37))          # (check_refusals reads its case from there)
    tm.check_refusals(be, FAMILY)


def test_argument_checks(emu):
    N = 4
    bufs = {"dof_state": np.zeros((N, 12, 2), np.float32), "torques": np.zeros((N, 12), np.float32), "contact_forces": np.zeros((N, BODIES, 3), np.float32),
            "root_states": np.zeros((N, 13), np.float32), "reset_buf": np.zeros(N, np.uint8)}
    strides = {"dof_state": (24, 2, 1), "torques": (12, 1), "contact_forces": (BODIES * 3, 3, 1), "root_states": (13, 1), "reset_buf": (1,)}
    table, group, out = np.zeros((GO2NN_ACTUATOR_NUM, N), np.float32), np.zeros(N, np.int32), np.zeros((2, GO2NN_ACTUATOR_OUT_NUM))
    p = lambda x: C.c_void_p(x.ctypes.data)
    mem = HostMemory()
    make_in = lambda: actuator_in(mem, bufs, strides)

    def broken(edit, says):
        a = make_in()
        edit(a)
        before = table.copy()
        rc = emu.go2nn_actuator_accumulate(C.byref(a), p(table), N, None)
        assert (table == before).all()
        return rc == EINVAL and says in emu.go2nn_last_error()

    def item(name, i, v):
        def edit(a):
            getattr(a, name)[i] = v
        return edit
    assert emu.go2nn_actuator_begin(p(table), N, -2, None) == 0
    assert emu.go2nn_actuator_accumulate(C.byref(make_in()), p(table), N, None) == 0, emu.go2nn_last_error()
    assert emu.go2nn_actuator_accumulate(None, p(table), N, None) == EINVAL and emu.go2nn_last_error()
    assert emu.go2nn_actuator_accumulate(C.byref(make_in()), None, N, None) == EINVAL
    for n in (0, -1):
        assert emu.go2nn_actuator_accumulate(C.byref(make_in()), p(table), n, None) == EINVAL
    for field in ACTUATOR_FIELDS:
        assert broken(lambda a: setattr(getattr(a, field), "p", None), b"null"), field
        assert broken(lambda a: setattr(getattr(a, field), "env_stride", 0), b"stride"), field
        if field != "reset_buf":
            assert broken(lambda a: setattr(getattr(a, field), "comp_stride", 0), b"component stride"), field
    assert broken(lambda a: setattr(a, "dof_vel_offset", 0), b"dof_vel_offset") and broken(lambda a: setattr(a, "contact_body_stride", 0), b"body stride")
    for f in range(4):
        assert broken(item("foot_body", f, -1), b"foot_body"), f
    for j in (0, 11):
        for v in (float("nan"), float("inf")):
            assert broken(item("pos_lo", j, v), b"pos_lo") and broken(item("pos_hi", j, v), b"pos_hi"), (j, v)
        assert broken(item("pos_lo", j, float(POS_HI[j]) + 1.0), b"pos_lo <= pos_hi")
        big = float(np.finfo(np.float32).max)          # every finite fp32 is a legal limit
        for name, v in (("pos_lo", -big), ("pos_hi", big), ("tau_sat_thr", big), ("vel_sat_thr", big)):
            a = make_in()
            getattr(a, name)[j] = v
            assert emu.go2nn_actuator_accumulate(C.byref(a), p(table), N, None) == 0, (name, emu.go2nn_last_error())
    a = make_in()
    a.contact_threshold = float(np.finfo(np.float32).max)
    assert emu.go2nn_actuator_accumulate(C.byref(a), p(table), N, None) == 0, emu.go2nn_last_error()
    for j in (0, 11):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert broken(item("tau_sat_thr", j, v), b"tau_sat_thr") and broken(item("vel_sat_thr", j, v), b"vel_sat_thr"), (j, v)
    for thr in (-1.0, float("nan"), float("inf")):
        assert broken(lambda a: setattr(a, "contact_threshold", thr), b"contact_threshold"), thr
    assert emu.go2nn_actuator_begin(None, N, 0, None) == EINVAL and emu.go2nn_actuator_begin(p(table), 0, 0, None) == EINVAL and emu.go2nn_last_error()
    assert emu.go2nn_actuator_reduce(p(table), p(group), N, 2, p(out), None) == 0
    for args in ((None, p(group), N, 2, p(out)), (p(table), None, N, 2, p(out)), (p(table), p(group), N, 2, None), (p(table), p(group), 0, 2, p(out)),
                 (p(table), p(group), N, 0, p(out)), (p(table), p(group), N, 65536, p(out))):
        assert emu.go2nn_actuator_reduce(*args, None) == EINVAL and emu.go2nn_last_error(), args[2:4]


@pytest.mark.parametrize("kernel,vgprs", [("eval_per_env_kernelI18ActuatorAccumulate", 512), ("eval_reduce_kernelILin1E12ActuatorTerm", 128), ("eval_bootstrap_kernelILi112ELi", 128)])
def test_no_kernel_has_scratch(kernel, vgprs):
    """the gfx950 code object of the built library: the accumulate lane keeps its 110 rows and 40 inputs in registers and the bootstrap lane its window's sums — a build
    that spills either to scratch fails here, not in a comment.  The accumulate lane uses no LDS (the reduce's tree does)"""
    from go2_rl_gym_amd import build
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(build.NN_OUT) and os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("no built device library, or no LLVM tools to read its code object")
    res = build.kernel_resources(build.NN_OUT, match=kernel)
    print(kernel, res)
    assert res is not None, "the library has no kernel %s" % kernel
    assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_count"] <= vgprs and ("reduce" in kernel or res["lds_bytes_per_workgroup"] == 0)


def test_actuator_symbols_and_struct_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7 and _nn.GO2NN_ABI_VERSION == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_actuator_begin", "go2nn_actuator_accumulate", "go2nn_actuator_reduce", "go2nn_actuator_bootstrap"):
            assert (" T " + f + "\n") in syms, (path, f)
    names = [n for n, _ in Go2nnActuatorIn._fields_]
    consts = ("GO2NN_ACTUATOR_NUM", "GO2NN_ACTUATOR_OUT_NUM", "GO2NN_ACTUATOR_JOINT0", "GO2NN_ACTUATOR_JOINT_ROWS", "GO2NN_ACTUATOR_FOOT0", "GO2NN_ACTUATOR_FOOT_ROWS",
              "GO2NN_ACTUATOR_OUT_N", "GO2NN_ACTUATOR_OUT_N_USED", "GO2NN_ACTUATOR_OUT_ROW0", "GO2NN_ABI_VERSION")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu", sizeof(Go2nnActuatorIn));\n'
                   + "".join('printf(" %%d", (int)%s);\n' % c for c in consts) + "".join('printf(" %%zu", offsetof(Go2nnActuatorIn, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(Go2nnActuatorIn)
    assert got[1:1 + len(consts)] == [GO2NN_ACTUATOR_NUM, GO2NN_ACTUATOR_OUT_NUM, GO2NN_ACTUATOR_JOINT0, len(ACTUATOR_JOINT_ROWS), GO2NN_ACTUATOR_FOOT0, len(ACTUATOR_FOOT_ROWS),
                                      _nn.GO2NN_ACTUATOR_OUT_N, _nn.GO2NN_ACTUATOR_OUT_N_USED, _nn.GO2NN_ACTUATOR_OUT_ROW0, 7]
    assert (GO2NN_ACTUATOR_NUM, GO2NN_ACTUATOR_OUT_NUM) == (111, 112)
    assert got[1 + len(consts):] == [getattr(Go2nnActuatorIn, n).offset for n in names]
    assert names[:5] == list(ACTUATOR_FIELDS)
    hdr = open(os.path.join(ROOT, "include", "go2nn.h")).read()
    for first, last, prefix, mirror in (("GO2NN_ACTUATOR_STEP = 0", "GO2NN_ACTUATOR_JOINT0 }", "GO2NN_ACTUATOR_", ACTUATOR_ENV_ROWS),
                                        ("GO2NN_ACTUATOR_J_TAU_SQ = 0", "GO2NN_ACTUATOR_JOINT_ROWS\n}", "GO2NN_ACTUATOR_J_", ACTUATOR_JOINT_ROWS),
                                        ("GO2NN_ACTUATOR_F_FZ_PEAK = 0", "GO2NN_ACTUATOR_FOOT_ROWS }", "GO2NN_ACTUATOR_F_", ACTUATOR_FOOT_ROWS)):
        enum = hdr[hdr.index(first):hdr.index(last)]
        assert [e.strip().split(" ")[0].replace(prefix, "").lower() for e in enum.split(",") if e.strip()] == list(mirror)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# The figures, restated from their definitions in plain Python floats: nothing of utils/evaluator.py is used below but the column helper of the reduce's layout.
KINDS = ("hip", "thigh", "calf")
JOINT_NAMES = ["%s_%s" % (leg, kind) for leg in ("FL", "FR", "RL", "RR") for kind in KINDS]
FOOT_NAMES = ["FR", "FL", "RR", "RL"]          # FOOT_BODY's order
DT = 0.02
NAN = float("nan")


def restated_figures(row, dt, joint_names, foot_names, torque_limits, peaks=None):
    """row: one (pooled) row of go2nn_actuator_reduce -> every key of every pool, from the definitions: sums with math.fsum, one division, NaN where the denominator is 0.
    peaks: {"tau", "vel", "margin" [12], "fz" [4]}, the partition's extremes per joint / foot (None entries: no used robot) -> the four extreme keys too"""
    v = lambda name, i=None: float(row[actuator_out_col(name, i)])
    div = lambda a, b: a / b if b > 0 else NAN
    root = lambda x: math.sqrt(x) if x == x else NAN
    n_used, used, dist = v("n_used"), v("used"), v("dist")
    joint_pools = [("", list(range(12)))] + [("/" + k, [j for j, n in enumerate(joint_names) if n.endswith(k)]) for k in KINDS] + [("/" + n, [j]) for j, n in enumerate(joint_names)]
    foot_pools = [("", list(range(4)))] + [("/" + n, [f]) for f, n in enumerate(foot_names)]
    d = {}
    for name, js in joint_pools:
        n = len(js)
        total = lambda key: math.fsum(v(key, j) for j in js)
        d["torque_rms" + name] = root(div(total("tau_sq"), n * used))
        d["torque_rms_share" + name] = root(div(math.fsum(v("tau_sq", j) / float(torque_limits[j]) ** 2 for j in js), n * used))
        d["torque_peak" + name] = div(total("tau_peak"), n * n_used)
        d["torque_saturation" + name] = div(total("tau_sat"), n * used)
        d["joint_speed_peak" + name] = div(total("vel_peak"), n * n_used)
        d["joint_speed_saturation" + name] = div(total("vel_sat"), n * used)
        d["positive_power" + name] = div(total("work_pos"), used)
        d["negative_power" + name] = div(total("work_neg"), used)
        d["limit_margin" + name] = div(total("margin_min"), n * n_used)
        if peaks is not None:
            some = peaks["tau"][js[0]] is not None
            d["torque_peak_max" + name] = max(peaks["tau"][j] for j in js) if some else NAN
            d["joint_speed_peak_max" + name] = max(peaks["vel"][j] for j in js) if some else NAN
            d["limit_margin_min" + name] = min(peaks["margin"][j] for j in js) if some else NAN
    for name, fs in foot_pools:
        d["grf_peak" + name] = div(math.fsum(v("fz_peak", f) for f in fs), len(fs) * n_used)
        d["grf_stance_mean" + name] = div(math.fsum(v("fz_sum", f) for f in fs), math.fsum(v("fz_frames", f) for f in fs))
        if peaks is not None:
            d["grf_peak_max" + name] = max(peaks["fz"][f] for f in fs) if peaks["fz"][fs[0]] is not None else NAN
    work = math.fsum(v("work_pos", j) for j in range(12))
    d["energy_per_m"] = work / dist if (n_used > 0 and dist * dt >= 1e-3 * n_used) else NAN          # J/m: dt cancels; below 1 mm per used robot it says nothing
    d["n_envs"] = int(v("n"))
    return d


def table_peaks(table, ids):
    """the extremes of the robots `ids` that have a used frame, straight from the per-robot table -> restated_figures' `peaks`"""
    t = table_rows(table)
    live = [e for e in ids if t["used"][e] > 0]
    col = lambda key, n, fn: [float(fn(t[key][live, i])) if live else None for i in range(n)]
    return {"tau": col("tau_peak", 12, max), "vel": col("vel_peak", 12, max), "margin": col("margin_min", 12, min), "fz": col("fz_peak", 4, max)}


def close(got, want, what=""):
    """a leaf of figures against its restatement: the same keys, NaN exactly where the restatement has NaN, every number to 1e-12 of itself (the order of a sum)"""
    got = {k: v for k, v in got.items() if k != "ci"}
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-12 * abs(w), (what, k, g, w)


def test_figures_against_their_definitions(emu):
    """the scripted table at 257 robots, reduced with each of the eight scripted robots in a cell of its own and the random ones dealt to three more: every key of every pool of
    every cell, and of the cells pooled, is the issue's definition applied to the reduce row — the figures that do not exist among them"""
    import types
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_EXTREME_KEYS, ACTUATOR_KEYS, ACTUATOR_MAX_ROWS, ACTUATOR_MIN_ROWS, PolicyEvaluator
    N, G = 257, 11
    table, ref, _ = run_script(emu, HostMemory(), N, layout=1)
    group = np.where(np.arange(N) < 8, np.arange(N), 8 + np.arange(N) % 3).astype(np.int32)
    out = emu_reduce(emu, np.ascontiguousarray(table), group, G)
    ns = types.SimpleNamespace(dt=DT, joint_names=JOINT_NAMES, act_foot_names=FOOT_NAMES, act_torque_limits=TAU_LIM)
    t64 = table.astype(np.float64)

    def with_extremes(rows, ids):          # the row as _actuator_results hands it to the row function: the reduce columns, then the 28 maxima and the 12 minima
        live = [e for e in ids if t64[actuator_row("used"), e] > 0]
        ext = np.concatenate([t64[ACTUATOR_MAX_ROWS][:, live].max(1), t64[ACTUATOR_MIN_ROWS][:, live].min(1)]) if live else np.concatenate([np.full(28, -np.inf), np.full(12, np.inf)])
        return np.concatenate([rows, ext])
    parts = [(np.nonzero(group == g)[0], out[g]) for g in range(G)] + [(np.arange(N), out.sum(0))]
    got = PolicyEvaluator._actuator_rows(ns, np.stack([with_extremes(r, ids) for ids, r in parts]))
    for (ids, r), leaf in zip(parts, got):
        want = restated_figures(r, DT, JOINT_NAMES, FOOT_NAMES, TAU_LIM, table_peaks(table, ids))
        close(leaf, want, "cell of robots %s..." % ids[:3])
        assert len(want) == 12 * 16 + 3 * 5 + 2 and set(ACTUATOR_KEYS + ACTUATOR_EXTREME_KEYS) < set(want)
    bare = PolicyEvaluator._actuator_rows(ns, out)          # (a bootstrap replicate's row: no extremes behind the reduce columns)
    for g in range(G):
        close(bare[g], restated_figures(out[g], DT, JOINT_NAMES, FOOT_NAMES, TAU_LIM), "bare row %d" % g)
    number = lambda x: isinstance(x, float) and not math.isnan(x)
    # robot 2: every counted frame a reset — in N, not in N_USED, and no figure exists
    assert got[2]["n_envs"] == 1 and out[2, 1] == 0 and all(math.isnan(v) for k, v in got[2].items() if k != "n_envs")
    # robot 4: foot 2 (RR) never in contact — its stance mean does not exist, the other feet's and the pooled one do; a force AT the threshold is no contact frame
    assert math.isnan(got[4]["grf_stance_mean/RR"]) and all(number(got[4]["grf_stance_mean" + n]) for n in ("", "/FR", "/FL", "/RL")) and number(got[4]["grf_peak/RR"])
    assert out[4, actuator_out_col("fz_frames", 1)] == (ref.rows["fz_frames"][4, 1]) < STEPS
    # robot 5 never moves: no cost per metre, every other figure exists; the robots that move have one, and it is the positive work alone over the distance
    assert math.isnan(got[5]["energy_per_m"]) and all(number(v) for k, v in got[5].items() if k not in ("energy_per_m", "n_envs"))
    for g in (0, 1, 3, 8, 9, 10, G):
        assert number(got[g]["energy_per_m"]) and got[g]["energy_per_m"] > 0, g
    work = math.fsum(ref.rows["work_pos"][3])
    assert abs(got[3]["energy_per_m"] - work / ref.rows["dist"][3]) <= 1e-5 * got[3]["energy_per_m"] and ref.rows["work_neg"][3].sum() > 0
    # robot 3: a joint past its limit and a joint that only brakes; robot 0: one saturated torque sample of 36 on joint 0, in units of joints x frames
    assert got[3]["limit_margin_min/FR_calf"] == -0.125 == got[3]["limit_margin/FR_calf"] and got[3]["positive_power/RL_hip"] == 0 and got[3]["negative_power/RL_hip"] > 0
    assert got[0]["torque_saturation/FL_hip"] == 1 / 36 and got[0]["torque_saturation/hip"] == 1 / (4 * 36) and got[0]["torque_saturation"] == 1 / (12 * 36)
    assert got[0]["joint_speed_saturation/FL_thigh"] == 1 / 36 and got[0]["torque_peak_max/FL_hip"] == 12.0 == got[0]["torque_peak/FL_hip"]
    # a hand-made row: tau^2 sums of 4 x limit^2 over 4 frames of 1 robot -> an RMS of the limit itself and a share of 1, whatever the limit
    row = np.zeros(GO2NN_ACTUATOR_OUT_NUM)
    edge = 1e-3 / DT          # the smallest distance sum [m / dt] of one used robot at which dist x dt reaches a millimetre
    while edge * DT < 1e-3:
        edge = float(np.nextafter(edge, np.inf))
    while float(np.nextafter(edge, 0.0)) * DT >= 1e-3:
        edge = float(np.nextafter(edge, 0.0))
    row[[actuator_out_col("n"), actuator_out_col("n_used")]], row[actuator_out_col("used")], row[actuator_out_col("dist")] = 1.0, 4.0, edge
    for j in range(12):
        row[actuator_out_col("tau_sq", j)], row[actuator_out_col("work_pos", j)], row[actuator_out_col("work_neg", j)] = 4.0 * float(TAU_LIM[j]) ** 2, 2.0, 100.0
    hand = PolicyEvaluator._actuator_rows(ns, row[None])[0]
    assert hand["torque_rms_share"] == 1.0 and hand["torque_rms/calf"] == 32.0 and hand["torque_rms/FL_thigh"] == 24.0 and hand["torque_rms"] == math.sqrt((16.0 ** 2 + 24.0 ** 2 + 32.0 ** 2) / 3)
    assert hand["positive_power"] == 6.0 and hand["positive_power/hip"] == 2.0 and hand["negative_power/FL_hip"] == 25.0
    assert hand["energy_per_m"] == 24.0 / row[actuator_out_col("dist")]          # exactly 1 mm per used robot: at the rule's edge the figure exists; work_neg is not in it
    row[actuator_out_col("dist")] = np.nextafter(row[actuator_out_col("dist")], 0.0)
    assert math.isnan(PolicyEvaluator._actuator_rows(ns, row[None])[0]["energy_per_m"])


ACT = dict(num_envs=64, seconds=1.0, warmup_s=0.1)


def same(a, b):
    """two leaves of res["actuators"]: equal, NaN where the other is NaN"""
    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        if k != "ci":
            assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def leaf_keys(ev):
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_EXTREME_KEYS, ACTUATOR_FOOT_KEYS, ACTUATOR_JOINT_KEYS, ACTUATOR_KINDS
    joint_pools = [""] + ["/" + k for k in ACTUATOR_KINDS] + ["/" + n for n in ev.joint_names]
    foot_pools = [""] + ["/" + n for n in ev.act_foot_names]
    keys = {k + pl for k in ACTUATOR_JOINT_KEYS + ("torque_peak_max", "joint_speed_peak_max", "limit_margin_min") for pl in joint_pools}
    keys |= {k + pl for k in ACTUATOR_FOOT_KEYS + ("grf_peak_max",) for pl in foot_pools} | {"energy_per_m", "n_envs"}
    assert set(ACTUATOR_EXTREME_KEYS) < keys and len(keys) == 12 * 16 + 3 * 5 + 2
    return keys


def check_actuator_result(ev, res, what):
    """everything the result says, recomputed from the per-robot table: the cells' rows, and every partition of every family as the pool of ITS robots — the sums exactly the
    sums of its cells' rows, the extremes the max / min over its robots —, found from the per-env axis arrays, not from the cell index arithmetic of the evaluator"""
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_KEYS
    t = ev.act_table.cpu().numpy().astype(np.float64)
    at, N = res["actuator_table"], ev.num_envs
    assert at.shape == (ev.num_cells, GO2NN_ACTUATOR_OUT_NUM) and (t[0] == ev.steps).all()
    tt = terms(t)
    whole = [actuator_out_col(k) for k in ("n", "n_used", "used")] + [actuator_out_col(k, i) for k in COUNT_ROWS for i in range(4 if k == "fz_frames" else 12)]
    for c in range(ev.num_cells):
        ids = np.nonzero(ev.cell_host == c)[0]
        for col in range(GO2NN_ACTUATOR_OUT_NUM):
            want = math.fsum(tt[ids, col])
            assert at[c, col] == want if col in whole else abs(at[c, col] - want) <= N * 2.0 ** -53 * math.fsum(np.abs(tt[ids, col])), (c, col)
    keys = leaf_keys(ev)

    def row(ids):
        return restated_figures(at[np.unique(ev.cell_host[ids])].sum(0), ev.dt, ev.joint_names, ev.act_foot_names, ev.act_torque_limits, table_peaks(t, ids))
    tree = res["actuators"]
    close(tree["overall"], row(np.arange(N)), "overall")
    assert tree["overall"]["n_envs"] == N and set(tree["overall"]) - {"ci"} == keys and not set(ACTUATOR_KEYS) & set(res["overall"])
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
    assert set(tree) == set(families) | {"overall"}, (set(tree), set(families))
    for fam, parts in families.items():
        total, peaks, margins = 0, [], []
        for path, ids in parts:
            leaf = tree[fam]
            for k in path:
                leaf = leaf[k]
            if len(ids):
                close(leaf, row(ids), (fam, path))
            else:
                assert leaf["n_envs"] == 0 and math.isnan(leaf["torque_rms"]) and math.isnan(leaf["torque_peak_max"])
            total += leaf["n_envs"]
            peaks.append(leaf["torque_peak_max"])
            margins.append(leaf["limit_margin_min"])
        assert total == N, (fam, total)          # the partitions of a family add up to the whole: the extremes as the max / min of the parts
        assert np.nanmax(peaks) == tree["overall"]["torque_peak_max"] and np.nanmin(margins) == tree["overall"]["limit_margin_min"], fam
    o = tree["overall"]
    print("%s: %d cells, overall %s" % (what, ev.num_cells, {k: round(o[k], 4) for k in ACTUATOR_KEYS + ("torque_peak_max", "limit_margin_min")}))
    assert o["torque_peak"] <= o["torque_peak_max"] and o["torque_rms"] <= o["torque_peak_max"] and o["limit_margin"] >= o["limit_margin_min"] and 0 <= o["torque_saturation"] <= 1


def check_recorded_robots(ev, res, what):
    """the table columns of the recorded robots are the rule (Reference, with the evaluator's own limits) applied to their recorded frames, within the table test's bounds"""
    trace = res["trace"]
    ids, S = trace["env_ids"], ev.steps
    assert trace["steps_recorded"] == S and trace["reset"].shape == (S, len(ids))
    ref = Reference(trace["torques"], trace["dof_pos"], trace["dof_vel"], trace["foot_force"][..., 2], trace["root_lin_vel"][..., :2], trace["reset"],
                    tau_thr=ev.act_tau_thr, vel_thr=ev.act_vel_thr, lo=ev.act_pos_lo, hi=ev.act_pos_hi, thr=ev.act_threshold)
    got = {k: v[ids] for k, v in table_rows(ev.act_table.cpu().numpy()).items()}
    worst = check_rows(got, ref, S, what)
    print("%s: %d recorded robots, %d used frames, %d saturated torque samples; largest float-sum gap / bound %.4f" % (what, len(ids), ref.rows["used"].sum(), ref.rows["tau_sat"].sum(), worst))
    return ref


@pytest.fixture(scope="module")
def plain_runs(emu):
    """the plain evaluation on the same weights: an evaluator that never heard of the flag, actuators = False, record = 2 without it, record = 2 with it"""
    ac = th.small_actor_critic()
    out = {"ac": ac}
    for name, over in (("never", {}), ("off", dict(actuators=False, actuators_saturation=0.5)), ("record", dict(record=2)), ("on", dict(actuators=True, record=2))):
        ev = th.make_evaluator(emu, **dict(ACT, **over))
        out[name] = (ev, ev.evaluate(ac))
    yield out
    for name in ("never", "off", "record", "on"):
        out[name][0].close()


def test_actuators_off_changes_nothing(plain_runs):
    from go2_rl_gym_amd.utils.evaluator import format_table, results_dict, scalars
    (ev0, res0), (ev1, res1) = plain_runs["never"], plain_runs["off"]
    assert "actuators" not in th.EVAL and ev1.actuators is False and not hasattr(ev1, "act_table") and not hasattr(ev1, "act_out") and [t.name for t in ev1.tables] == []
    assert set(res1) == set(res0) and not any("actuator" in k for k in res1)
    assert res1["table"].tobytes() == res0["table"].tobytes() and str(results_dict(res1)) == str(results_dict(res0))
    assert format_table(res1) == format_table(res0) and str(scalars(res1)) == str(scalars(res0))
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    for task in ("go2_flat", "go2_cts"):
        e = task_registry.get_cfgs(task)[1].evaluation
        assert (e.actuators, e.actuators_saturation) == (False, 0.95)
    assert get_args(["--actuators"]).actuators is True and get_args([]).actuators is False
    _, cfg = update_cfg_from_args(None, task_registry.get_cfgs("go2_flat")[1], get_args(["--actuators", "--robust"]))
    assert cfg.evaluation.actuators is True and cfg.evaluation.perturbations and task_registry.get_cfgs("go2_flat")[1].evaluation.actuators is False


def test_actuators_on_leaves_scores_and_trace_alone(plain_runs):
    from go2_rl_gym_amd.utils.evaluator import results_dict
    (_, res0), (_, rec), (ev, res) = plain_runs["never"], plain_runs["record"], plain_runs["on"]
    assert res["table"].tobytes() == rec["table"].tobytes() == res0["table"].tobytes()
    assert res["trace"]["frames"].tobytes() == rec["trace"]["frames"].tobytes() and res["trace"]["env_ids"].tolist() == rec["trace"]["env_ids"].tolist()
    assert res["overall"] == rec["overall"] and res["groups"] == rec["groups"] and ev.actuators is True
    rd, rd0 = results_dict(res), results_dict(rec)
    assert str({k: v for k, v in rd.items() if k != "actuators"}) == str(rd0)
    s = res["actuator_settings"]
    assert s["saturation"] == 0.95 and s["contact_threshold"] == 1.0 and s["torque_limits"][:3] == [pytest.approx(23.7), pytest.approx(23.7), pytest.approx(35.55)]
    assert s["torque_saturation_thresholds"][2] == float(np.float32(0.95) * np.float32(35.55)) and s["joint_names"][:3] == ["FL_hip", "FL_thigh", "FL_calf"]


def test_actuator_table_of_the_recorded_robots_is_the_rule_on_their_frames(plain_runs):
    ev, res = plain_runs["on"]
    ref = check_recorded_robots(ev, res, "plain evaluation")
    assert len(res["trace"]["env_ids"]) == 2 * len(ev.groups) and ref.rows["used"].sum() > 0 and ref.rows["work_pos"].sum() > 0


def test_actuator_partitions_and_outputs(plain_runs, capsys):
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_EXTREME_KEYS, ACTUATOR_KEYS, format_table, results_dict, scalars
    ev, res = plain_runs["on"]
    check_actuator_result(ev, res, "plain evaluation")
    assert res["actuator_cells"] == ["terrain", "scenario"] and set(res["actuators"]) == {"overall", "groups"}
    tags = dict(scalars(res))
    eq = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    assert all(eq(tags["Eval/actuators/" + k], res["actuators"]["overall"][k]) for k in ACTUATOR_KEYS + ACTUATOR_EXTREME_KEYS) and "Eval/actuators/torque_rms/FL_calf" in tags
    assert eq(tags["Eval/actuators/plane/forward_1.0/torque_saturation"], res["actuators"]["groups"]["plane"]["forward_1.0"]["torque_saturation"]) and "Eval/lin_vel_err" in tags
    assert math.isnan(res["actuators"]["groups"]["plane"]["stand"]["energy_per_m"]) or res["actuators"]["groups"]["plane"]["stand"]["energy_per_m"] > 0
    import yaml
    back = yaml.safe_load(yaml.safe_dump(results_dict(res, 3)))
    assert set(back["actuators"]) == {"overall", "groups", "settings"} and back["actuators"]["groups"]["plane"]["stand"]["n_envs"] == 16
    assert back["actuators"]["settings"]["saturation"] == 0.95 and len(back["actuators"]["settings"]["torque_limits"]) == 12
    text = format_table(res)
    assert "torque_saturation/calf" in text and "limit_margin/hip" in text and "grf_peak" in text and "energy_per_m" in text
    assert len(text.splitlines()) == 2 * (1 + len(ev.groups) + 1) + 1
    # a group with fewer than 4 robots is said so, once
    small = th.make_evaluator(load_nn_emu(), num_envs=12, seconds=0.1, warmup_s=0.0, actuators=True)
    said = capsys.readouterr().out
    assert "fewer than 4 robots" in said and "actuator figures" in said
    small.close()


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0001, float("nan"), float("inf"), "much", None, True])
def test_bad_saturation_names_the_key(emu, bad):
    with pytest.raises(ValueError, match="actuators_saturation"):
        th.make_evaluator(emu, num_envs=12, actuators=True, actuators_saturation=bad)


def test_saturation_of_one_is_accepted_and_read(emu):
    ev = th.make_evaluator(emu, num_envs=12, seconds=0.1, warmup_s=0.0, actuators=True, actuators_saturation=1.0, gait_contact_threshold=3.0)
    a = ev._actuator_in()
    assert list(a.tau_sat_thr) == [float(x) for x in ev.env.torque_limits.tolist()] and a.contact_threshold == 3.0 and list(a.foot_body) == ev.env.feet_indices.tolist()
    ev.close()
    with pytest.raises(ValueError, match="gait_contact_threshold"):
        th.make_evaluator(emu, num_envs=12, actuators=True, gait_contact_threshold=-1.0)


NEXT_TO = {
    "perturbations": dict(task="go2_flat", own="robust_table", perturbations=[["nominal", {}], ["push_front_0.5", {"dv": [0.5, 0.0, 0.0]}], ["motor_0.8", {"strength": 0.8}]],
                          push_first_s=0.2, push_period_s=0.4, push_window_s=0.3),
    "sensors": dict(task="go2_flat", own="cell_table", sensors=[["nominal", {}], ["delay_1", {"delay": 1}], ["noise_2.0", {"noise": 2.0}]]),
    "maneuvers": dict(task="go2_flat", own="maneuver_table", maneuvers=[["start_1.0", [[0.0, 0.0, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0]]], ["turn_flip", [[0.0, 0.0, 0.0, 1.0], [0.4, 0.0, 0.0, -1.0]]]],
                      maneuver_window_s=0.3, maneuver_hold_s=0.1),
    "ladder": dict(task="go2", own="ladder_table", ladder=True, ladder_levels=[0, 4], ladder_distance=0.1),
    "gait": dict(task="go2_flat", own="gait_table", gait=True),
    "asymmetry": dict(task="go2_flat", own="asymmetry_table", asymmetry=True),
    "spectrum": dict(task="go2_flat", own="spectrum_table", spectrum=True, spectrum_window=16),
}


@pytest.mark.parametrize("other", sorted(NEXT_TO))
def test_actuators_next_to_every_mode_and_add_on(emu, other):
    """an add-on: next to each extra axis and each other add-on the others' results are those of the run without it, byte for byte; the recorded robots follow the rule
    and every partition the mode reports is the pool of its cells"""
    from go2_rl_gym_amd.utils.evaluator import results_dict
    over = dict(ACT, **NEXT_TO[other])
    task, own = over.pop("task"), over.pop("own")
    ac = th.small_actor_critic()
    base = th.make_evaluator(emu, task=task, record=1, **over)
    res0 = base.evaluate(ac)
    base.close()
    ev = th.make_evaluator(emu, task=task, actuators=True, record=1, **over)
    res = ev.evaluate(ac)
    assert res["table"].tobytes() == res0["table"].tobytes() and res[own].tobytes() == res0[own].tobytes() and res["trace"]["frames"].tobytes() == res0["trace"]["frames"].tobytes()
    assert str({k: v for k, v in results_dict(res).items() if k != "actuators"}) == str(results_dict(res0))
    check_actuator_result(ev, res, other)
    check_recorded_robots(ev, res, other)
    assert (other in res["actuators"]) == (other in ("perturbations", "sensors", "maneuvers", "ladder")) and ("cells" in res["actuators"]) == (other in ("perturbations", "sensors"))
    again = ev.evaluate(ac)
    assert again["actuator_table"].tobytes() == res["actuator_table"].tobytes() and again["actuator_extremes"].tobytes() == res["actuator_extremes"].tobytes()
    ev.close()


def test_ci_all_gives_every_leaf_intervals_that_are_the_row_function_of_the_replicate_rows(emu):
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_EXTREME_KEYS, BOOTSTRAP_HEADLINES, actuator_replicates, format_table
    over = dict(ACT, sensors=NEXT_TO["sensors"]["sensors"], bootstrap=200, bootstrap_all=True)
    ac = th.small_actor_critic()
    base = th.make_evaluator(emu, **over)
    res0 = base.evaluate(ac)
    base.close()
    ev = th.make_evaluator(emu, actuators=True, **over)
    res = ev.evaluate(ac)
    bs = res["bootstrap"]
    assert bs["table"].tobytes() == res0["bootstrap"]["table"].tobytes() and str(res["overall"]) == str(res0["overall"]) and set(bs["tables"]) == {"actuator"}
    assert bs["tables"]["actuator"].shape == (200, ev.num_cells, GO2NN_ACTUATOR_OUT_NUM) and ("actuator", ("torque_rms_share", "torque_saturation", "energy_per_m")) in BOOTSTRAP_HEADLINES
    keys = leaf_keys(ev) - {"n_envs"}
    boot = {k for k in keys if k.split("/")[0] not in ACTUATOR_EXTREME_KEYS}
    leaves = ev._addon_replicates(bs["tables"]["actuator"])
    assert {p[0] for p, _ in leaves} == {"overall", "groups", "cells", "sensors"}
    for path, rows in leaves:
        leaf = res["actuators"]
        for k in path:
            leaf = leaf[k]
        assert set(leaf["ci"]) == boot and rows.shape == (200, GO2NN_ACTUATOR_OUT_NUM)
        lo, hi = leaf["ci"]["torque_rms"]
        assert lo <= leaf["torque_rms"] <= hi, (path, lo, leaf["torque_rms"], hi)
    path, rows = leaves[0]
    reps = actuator_replicates(rows, ev.dt, ev.joint_names, ev.act_foot_names, ev.act_torque_limits)
    for b in (0, 17, 199):          # replicate b's figures are the row function of replicate row b, bit for bit
        want = ev._actuator_row(rows[b])
        close(want, restated_figures(rows[b], ev.dt, ev.joint_names, ev.act_foot_names, ev.act_torque_limits), "replicate %d" % b)
        for k in boot:
            assert reps[k][b] == want[k] or (math.isnan(reps[k][b]) and math.isnan(want[k])), (b, k)
            assert bs["metrics"][k][b] == reps[k][b] or math.isnan(want[k])
    text = format_table(res)
    assert "torque_rms_share" in text.splitlines()[-2] and "energy_per_m" in text.splitlines()[-2]
    ev.close()
    with pytest.raises(ValueError, match="actuator: 112 columns"):
        th.make_evaluator(emu, actuators=True, **dict(over, bootstrap_max_bytes=200 * 12 * 8 * 20))


BASE = ["--task", "go2_flat", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"]


def test_metric_acceptance_directions_and_refusals():
    from go2_rl_gym_amd.scripts.evaluate import best_checkpoint, check_ci_metric, check_flag_metric, check_metric, evaluate, higher_is_better, is_actuator_metric
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.evaluator import ACTUATOR_EXTREME_KEYS, ACTUATOR_KEYS
    lower = [k for k in ACTUATOR_KEYS + ACTUATOR_EXTREME_KEYS if not k.startswith("limit_margin")]
    assert all(is_actuator_metric(k) and not higher_is_better(k) for k in lower) and higher_is_better("limit_margin") and higher_is_better("limit_margin_min")
    for k, hi in (("torque_rms/calf", False), ("torque_saturation/FL_thigh", False), ("limit_margin/hip", True), ("limit_margin/RR_calf", True), ("grf_peak/RL", False),
                  ("limit_margin_min/thigh", True), ("grf_peak_max/FR", False)):
        assert is_actuator_metric(k) and higher_is_better(k) is hi, k
        check_metric(k)
    for k in ("torque_rms/FL", "grf_peak/calf", "energy_per_m/hip", "torque_rms/FL_foot", "torque", "torque_rms/calf/x"):
        assert not is_actuator_metric(k), k
    on, off = get_args(BASE + ["--actuators"]), get_args(BASE)
    check_flag_metric("torque_saturation", on)
    check_flag_metric("lin_vel_err", off)
    with pytest.raises(ValueError, match="--actuators, which is not on"):
        check_flag_metric("torque_saturation/calf", off)
    with pytest.raises(ValueError, match="--actuators, which is not on"):          # refused before anything runs: no run directory exists here
        evaluate(BASE + ["--metric", "energy_per_m"], log_root="/nonexistent")
    ci, ci_all = get_args(BASE + ["--actuators", "--ci", "50"]), get_args(BASE + ["--actuators", "--ci", "50", "--ci_all"])
    for k in ("torque_saturation", "torque_rms/calf", "energy_per_m", "limit_margin/FL_hip", "grf_stance_mean/RR"):
        check_ci_metric(k, ci_all)
        with pytest.raises(ValueError, match="without --ci_all"):
            check_ci_metric(k, ci)
    for k in ACTUATOR_EXTREME_KEYS + ("torque_peak_max/calf",):
        for args in (ci, ci_all):
            with pytest.raises(ValueError, match="a bootstrap of an extreme is not one"):
                check_ci_metric(k, args)
    with pytest.raises(ValueError, match="--actuators, which is not on"):
        check_ci_metric("torque_saturation", get_args(BASE + ["--ci", "50", "--ci_all"]))
    rows = [{"checkpoint": "a", "overall": {}, "actuators": {"overall": {"torque_saturation": 0.2, "limit_margin": 0.1, "torque_peak_max": float("nan")}}},
            {"checkpoint": "b", "overall": {}, "actuators": {"overall": {"torque_saturation": 0.1, "limit_margin": 0.3, "torque_peak_max": 30.0}}}]
    assert [best_checkpoint(rows, m)["checkpoint"] for m in ("torque_saturation", "limit_margin", "torque_peak_max")] == ["b", "b", "b"]


def test_cli_names_the_checkpoint_that_leans_least_on_the_torque_limit(emu, tmp_path, capsys, monkeypatch):
    """a tiny go2_flat run on the oracle (two checkpoints), then scripts/evaluate.py --all_checkpoints --actuators --metric torque_saturation: lower is better"""
    import copy
    import json
    from helpers import load_oracle
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.scripts.evaluate import evaluate
    from go2_rl_gym_amd.utils import get_args
    train_cfg = copy.deepcopy(task_registry.train_cfgs["go2_flat"])
    train_cfg.runner.save_interval = 1
    e = train_cfg.evaluation
    e.num_envs, e.seconds, e.warmup_s, e.actuators_saturation = 48, 0.6, 0.1, 0.3          # (a low share: an untrained policy's torques reach it)
    monkeypatch.setitem(task_registry.train_cfgs, "go2_flat", train_cfg)
    base = ["--task", "go2_flat", "--num_envs", "16", "--headless", "--sim_device", "cpu", "--rl_device", "cpu", "--seed", "5"]
    args = get_args(base)
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, log_root=str(tmp_path))
    runner.learn(1)
    env.close()
    capsys.readouterr()
    out = evaluate(base + ["--actuators", "--all_checkpoints", "--metric", "torque_saturation"], log_root=str(tmp_path), env_kwargs={"lib": load_oracle()}, evaluator_kwargs={"nn_lib": emu})
    names = [r["checkpoint"] for r in out["checkpoints"]]
    values = [r["actuators"]["overall"]["torque_saturation"] for r in out["checkpoints"]]
    assert names == ["model_0.pt", "model_1.pt"] and out["metric"] == "torque_saturation" and out["best"] == names[int(np.argmin(values))]
    assert out["best_value"] == min(values) and 0 < max(values) <= 1 and all("torque_saturation" not in r["overall"] for r in out["checkpoints"])
    text = capsys.readouterr().out
    assert "torque_saturation/calf" in text and json.loads([l for l in text.splitlines() if l.startswith("{")][-1])["best"] == out["best"]
