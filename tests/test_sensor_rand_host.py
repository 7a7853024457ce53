"""Training under randomised sensors on the CPU: the host build of go2nn_sensor_rand_apply (include/go2nn.h) over a scripted run of 14 calls — the ring of 5 slots wraps
twice — against a restatement written here (Philox4x32-10 in integers, the arithmetic in float64), the spread of the episode draws, the argument checks, the struct layout,
LeggedRobot with domain_rand.randomize_sensors on the oracle + the host build (plain steps and rollout rows), and two PPO and two CTS iterations restated from the rollout
storage alone.

THE BOUND of a lane that adds an offset.  out = fl(src + fl(t mag)) with t = 2 u - 1 exact, or one fused multiply-add.  With b = t mag exact, M = max(|src|, |b|) and B
the power of two with B / 2 <= M < B, ulp(M) = B 2^-24: the product is within ulp(M) / 2 of b, and the sum, of magnitude below 2 B where the spacing is 2 ulp(M), within
ulp(M) of src + fl(b): |out - (src + b)| <= 1.5 ulp(M).  The fused form has the second rounding only, and the clamp moves two numbers no further apart.  Every test that
uses the bound prints the largest |out - exact| / (1.5 ulp(M)) of its run: 0.98 on the host build (two roundings), 0.67 on the MI355X (fused).

THE DROP DECISION u < p uses an fp32 p = drop_lo + u_p (drop_hi - drop_lo) that may be formed with or without fusion; either is within 2^-23 of the float64 value used
here, so a draw with |u - p| >= 2^-20 is decided alike.  The others are left out (with everything that then depends on the env's held frame) and their share is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, load_nn_emu, load_oracle
import test_eval_host as th
from test_sensor_host import GO2_KIND, K, TOY_KIND, HostMemory, bits, philox_int, ulp32
from go2_rl_gym_amd import _abi, _nn
from go2_rl_gym_amd._nn import GO2NN_SENSOR_MAX_DELAY, GO2NN_SENSOR_MAX_WIDTH, GO2_OBS_KINDS, SENSOR_KINDS, SENSOR_RAND_FIELDS, Go2nnSensorIn, Go2nnSensorRand
from go2_rl_gym_amd.envs import task_registry
from go2_rl_gym_amd.utils import get_args

M32 = 0xFFFFFFFF
TAG_EPISODE, TAG_BIAS, TAG_DROP = 4, 5, 6
R = GO2NN_SENSOR_MAX_DELAY + 1
CALLS = 14
EINVAL = -22
RANGES = dict(delay_lo=0, delay_hi=4, drop_lo=0.1, drop_hi=0.5, gyro_bias=0.05, gravity_bias=0.0, joint_offset=0.03)


def philox_words(c0, c1, c2, seed, tag):
    """Philox4x32-10 on uint64 arrays (every product of two 32-bit numbers fits) for counters (c0, c1, c2, 0), key (seed, tag) -> words 0 and 1"""
    c0, c1, c2 = np.broadcast_arrays(np.asarray(c0, np.uint64), np.asarray(c1, np.uint64), np.asarray(c2, np.uint64))
    c3 = np.zeros_like(c0)
    k0, k1, m, s32 = np.uint64(seed), np.uint64(tag), np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1


def u01(word):
    """u = (x >> 8) 2^-24, exact in float64"""
    return (word >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def test_two_word_philox_restatement():
    rng = np.random.default_rng(2)
    c = rng.integers(0, 2 ** 32, (40, 3), dtype=np.uint64)
    w0, w1 = philox_words(c[:, 0], c[:, 1], c[:, 2], 0xDEADBEEF, TAG_EPISODE)
    want = [philox_int((int(a), int(b), int(d), 0), (0xDEADBEEF, TAG_EPISODE))[:2] for a, b, d in c]
    assert [(int(a), int(b)) for a, b in zip(w0, w1)] == want


def make_rand(env_offset=0, **fields):
    r = Go2nnSensorRand()
    for k, v in dict(RANGES, **fields).items():
        setattr(r, k, v)
    r.env_offset = env_offset
    return r


def episode_draws(r, seed, g, s0):
    """the draws of the episodes that began at cursor s0 (any shape, broadcast against the global env ids g) -> delay (int64), p (float64)"""
    w0, w1 = philox_words(g, 0, np.asarray(s0, np.int64) & M32, seed, TAG_EPISODE)
    span = r.delay_hi - r.delay_lo
    k = (u01(w0).astype(np.float32) * np.float32(span + 1)).astype(np.int64)          # one fp32 product, truncated
    width = np.float32(r.drop_hi) - np.float32(r.drop_lo)
    assert width.dtype == np.float32
    return r.delay_lo + np.minimum(k, span), float(np.float32(r.drop_lo)) + u01(w1) * float(width)


class Restated:
    """the rule of include/go2nn.h for frames x [T, N, D] delivered at cursor values cursor0 .. cursor0 + T - 1, with fresh [T, N] (dones, also_fresh and cursor 0 already
    merged).  known0 False: the episodes that run at row 0 began before it — their lanes are not restated until the env's first fresh row."""

    def __init__(self, x, fresh, kind, r, seed, clip, cursor0=0, known0=True):
        T, N, D = x.shape
        self.x, self.kind = x, kind
        s = cursor0 + np.arange(T, dtype=np.int64)
        fresh = fresh.astype(bool).copy()
        if cursor0 == 0:
            fresh[0] = True
        assert known0 is False or fresh[0].all()
        s0 = np.full((T, N), -1, np.int64)          # the cursor at which the running episode began, -1: before row 0
        for t in range(T):
            s0[t] = np.where(fresh[t], s[t], s0[t - 1] if t else -1)
        known = s0 >= 0
        g = (r.env_offset + np.arange(N, dtype=np.int64)) & M32
        delay, p = episode_draws(r, seed, g[None, :], np.maximum(s0, 0))
        u = u01(philox_words(g[None, :], 0, s[:, None] & M32, seed, TAG_DROP)[0])
        near = known & ~fresh & (p > 0) & (np.abs(u - p) < 2.0 ** -20)
        self.undecided_share = float(near.sum()) / max(int(known.sum()), 1)
        self.dropped = known & ~fresh & (p > 0) & (u < p) & ~near
        self.u_drop, self.p, self.delay, self.s0, self.fresh, self.known = u, p, delay, s0, fresh, known
        bad = np.zeros((T, N), bool)          # the held frame is not known: an undecided draw, until a frame is surely delivered again
        for t in range(T):
            bad[t] = near[t] | (self.dropped[t] & (bad[t - 1] if t else False))
        prop = kind != K["pass"]
        self.src_row = np.where(prop[None, None, :], (np.maximum(s[:, None] - delay, s0) - cursor0)[:, :, None], np.arange(T)[:, None, None])
        self.checked = np.broadcast_to((known & ~bad)[:, :, None], (T, N, D)) | (~prop)[None, None, :]
        self.src = np.take_along_axis(x, np.clip(self.src_row, 0, T - 1), 0)
        assert (self.src_row[self.checked] >= 0).all()
        mag = np.zeros(D, np.float32)
        mag[kind == K["gyro"]], mag[kind == K["gravity"]], mag[kind == K["joint_pos"]] = r.gyro_bias, r.gravity_bias, r.joint_offset
        self.mag = mag
        ub = u01(philox_words(g[None, :, None], np.arange(D)[None, None, :], (np.maximum(s0, 0) & M32)[:, :, None], seed, TAG_BIAS)[0])
        self.bias = (2.0 * ub - 1.0) * mag.astype(np.float64)[None, None, :]
        src64 = self.src.astype(np.float64)
        self.exact = np.clip(src64 + self.bias, -clip, clip)
        self.largest = np.maximum(np.abs(src64), np.abs(self.bias))
        self.held_lane = self.checked & self.dropped[:, :, None] & prop[None, None, :]
        self.pass_lane = np.broadcast_to((~prop)[None, None, :], (T, N, D))
        self.copy_lane = self.checked & ~self.held_lane & ~self.pass_lane & (mag == 0)[None, None, :]
        self.arith_lane = self.checked & ~self.held_lane & ~self.pass_lane & (mag != 0)[None, None, :]
        self.clip = clip

    def check(self, out, what):
        """every checked lane of out [T, N, D] -> the largest |out - exact| / (1.5 ulp(M))"""
        assert self.undecided_share <= 0.01, self.undecided_share
        assert (bits(out)[self.pass_lane] == bits(self.x)[self.pass_lane]).all(), what
        assert (bits(out)[self.copy_lane] == bits(self.src)[self.copy_lane]).all(), what
        assert not self.held_lane[0].any()
        assert (bits(out[1:])[self.held_lane[1:]] == bits(out[:-1])[self.held_lane[1:]]).all(), what
        gap = np.abs(out.astype(np.float64) - self.exact)
        ratio = np.where(self.arith_lane, gap / (1.5 * ulp32(self.largest)), 0.0)
        worst = float(ratio.max())
        print("%s: %d arithmetic lanes, %d copied, %d held, %d passed through, undecided drop draws %.2e; largest |out - exact| / (1.5 ulp(M)) = %.3f"
              % (what, int(self.arith_lane.sum()), int(self.copy_lane.sum()), int(self.held_lane.sum()), int(self.pass_lane.sum()), self.undecided_share, worst))
        assert worst <= 1.0 and (np.abs(out[self.arith_lane]) <= self.clip).all()
        return worst


# ---- the scripted run -------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """14 calls: resets at steps 3, 6 and 11 for interleaved env subsets, one more on a step whose drop draw fires for any p of the range, an also_fresh call at step 8 and
    an all-zero also_fresh at step 9"""

    def __init__(self, N, kind=GO2_KIND, env_offset=0, clip=100.0, x_scale=1.0, **fields):
        self.N, self.D, self.kind, self.clip, self.seed = N, len(kind), kind, clip, 0x5EED0000 + N
        self.r = make_rand(env_offset, **fields)
        rng = np.random.default_rng(200 + N)
        T, D = CALLS, self.D
        x = (rng.normal(0, 1, (T, N, D)) * x_scale).astype(np.float32)
        x[rng.random((T, N, D)) < 0.02] = -0.0                       # bit patterns an add of zero or a clamp round trip would not keep
        x[rng.random((T, N, D)) < 0.02] = np.float32(1e-41)          # (a denormal)
        self.x = x
        ids = np.arange(N)
        dones = np.zeros((T, N), np.uint8)
        dones[3, ids % 7 == 3] = 1
        dones[6, ids % 5 == 2] = 1
        dones[11, ids % 7 == 3] = 1
        dones[0, ids % 4 == 1] = 1          # (step 0 refills anyway)
        self.also = {8: (ids % 6 == 1).astype(np.uint8), 9: np.zeros(N, np.uint8)}
        self.done_on_drop = None
        if self.r.drop_lo > 0:
            g = (env_offset + ids) & M32
            u = u01(philox_words(g[None, :], 0, np.arange(T)[:, None], self.seed, TAG_DROP)[0])
            te = np.argwhere((u[4:13] < float(np.float32(self.r.drop_lo)) - 2.0 ** -20) & (dones[4:13] == 0) & (ids % 6 != 1)[None, :])
            assert len(te) > 0
            self.done_on_drop = (int(te[0][0]) + 4, int(te[0][1]))
            dones[self.done_on_drop] = 1
        self.dones = dones
        fresh = dones != 0
        fresh[8] |= self.also[8] != 0
        self.ref = Restated(x, fresh, kind, self.r, self.seed, clip)
        if self.done_on_drop is not None:          # the draw fires under every p of the range, and the frame is delivered all the same
            t0, e0 = self.done_on_drop
            assert self.ref.u_drop[t0, e0] < self.ref.p[t0, e0] and self.ref.fresh[t0, e0] and not self.ref.dropped[t0, e0]


def run_script(lib, mem, case):
    """the scripted calls on `lib` with every buffer in `mem` -> the delivered frames fp32 [CALLS, N, D]"""
    N, D = case.N, case.D
    assert lib.go2nn_sensor_rand_check(C.byref(case.r), C.c_void_p(case.kind.ctypes.data), D) == 0, lib.go2nn_last_error()
    nbytes = lib.go2nn_sensor_rand_state_bytes(N, D)
    assert nbytes == 256 + (R + 2) * N * D * 4
    state = mem.put(np.full(nbytes, 0xAB, np.uint8))          # garbage: begin and step 0 define everything that is ever read
    h = dict(obs=mem.put(case.x[0]), dones=mem.put(case.dones[0]), kind=mem.put(case.kind), also=mem.put(np.zeros(N, np.uint8)), out=mem.put(np.full((N, D), 7.0, np.float32)))
    a = Go2nnSensorIn()
    a.obs.p, a.obs.env_stride, a.obs.comp_stride = mem.ptr(h["obs"]), D, 1
    a.dones, a.scale, a.kind, a.D, a.num_specs, a.clip, a.seed = mem.ptr(h["dones"]), None, mem.ptr(h["kind"]), D, 0, case.clip, case.seed
    assert lib.go2nn_sensor_rand_begin(C.c_void_p(mem.ptr(state)), mem.stream) == 0, lib.go2nn_last_error()
    out = np.zeros((CALLS, N, D), np.float32)
    for t in range(CALLS):
        mem.set(h["obs"], case.x[t])
        mem.set(h["dones"], case.dones[t])
        also = None
        if t in case.also:
            mem.set(h["also"], case.also[t])
            also = C.c_void_p(mem.ptr(h["also"]))
        assert lib.go2nn_sensor_rand_apply(C.byref(a), C.byref(case.r), also, C.c_void_p(mem.ptr(state)), C.c_void_p(mem.ptr(h["out"])), N, mem.stream) == 0, lib.go2nn_last_error()
        out[t] = np.asarray(mem.get(h["out"])).reshape(N, D)
    st = np.asarray(mem.get(state))
    assert int(st[:4].view(np.int32)[0]) == CALLS          # the cursor
    start = st[256 + (R + 1) * N * D * 4:].view(np.int32).reshape(N, D)
    assert (start == case.ref.s0[-1][:, None]).all()          # every lane's own entry, PASS columns included
    return out


def check_script(case, out, what):
    ref = case.ref
    worst = ref.check(out, what)
    N = case.N
    prop = case.kind != K["pass"]
    if case.r.delay_hi > 0 and N >= 17:          # delayed sources: lanes that deliver an OLDER frame's bits exist, on both sides of a ring wrap
        old = ref.copy_lane & (ref.src_row < np.arange(CALLS)[:, None, None])
        assert old[:R].any() and old[R:2 * R].any() and old[2 * R:].any() and (bits(out)[old] == bits(ref.src)[old]).all()
        after = ref.copy_lane & (ref.src_row == (ref.s0 - 0)[:, :, None]) & ~ref.fresh[:, :, None] & (ref.delay > 0)[:, :, None]
        assert after.any()          # (the refill: a delayed lane right after a reset repeats the reset frame, not the pre-reset past)
    if case.r.drop_hi > 0 and N >= 17:
        assert ref.held_lane.any() and (ref.dropped.sum(0) > 0).mean() > 0.5
        # a delivered frame after a dropped one is the restated source again (held was left alone and then replaced)
        follow = np.zeros_like(ref.dropped)
        follow[1:] = ref.dropped[:-1] & ~ref.dropped[1:]
        assert follow.any()
    special = ((bits(case.x) == 0x80000000) | (bits(case.x) == bits(np.float32(1e-41)))) & (ref.pass_lane | ref.copy_lane)
    assert N < 17 or special.sum() > 10          # -0.0 and denormals go through the lanes that add nothing (bit-exact above)
    if case.done_on_drop is not None:
        t0, e0 = case.done_on_drop
        lanes = (ref.copy_lane | ref.arith_lane)[t0, e0]
        assert lanes[prop].all() and (ref.src_row[t0, e0] == t0).all()
    return worst


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


@pytest.mark.parametrize("N,env_offset", [(1, 0), (17, 0), (300, 0), (300, 0xFFFFFF00)])
def test_scripted_run_against_the_restatement(emu, N, env_offset):
    """(a global id that wraps at 2^32 included: env_offset + e is uint32 arithmetic)"""
    case = Case(N, env_offset=env_offset)
    check_script(case, run_script(emu, HostMemory(), case), "host N=%d D=45 env_offset=%#x" % (N, env_offset))


def test_scripted_run_with_a_toy_layout(emu):
    case = Case(40, kind=TOY_KIND, gravity_bias=0.02)
    check_script(case, run_script(emu, HostMemory(), case), "host N=40 D=7")


def test_env_offset_shifts_the_draws(emu):
    """rank 1 of two ranks with 17 envs each draws what envs 17 .. 33 of one rank with 34 draw"""
    whole, part = Case(34), Case(17, env_offset=17)
    part.seed, part.x, part.dones, part.also = whole.seed, whole.x[:, 17:], whole.dones[:, 17:], {k: v[17:] for k, v in whole.also.items()}
    a, b = run_script(emu, HostMemory(), whole), None
    part.ref = Restated(part.x, (part.dones != 0) | np.stack([part.also.get(t, np.zeros(17, np.uint8)) != 0 for t in range(CALLS)]), part.kind, part.r, part.seed, part.clip)
    b = run_script(emu, HostMemory(), part)
    assert a[:, 17:].tobytes() == b.tobytes() and a[:, :17].tobytes() != b.tobytes()


def test_latency_alone_delivers_old_bits(emu):
    """delay 2 for every episode, no drops, no offsets: every proprioceptive lane is a copy"""
    case = Case(17, delay_lo=2, delay_hi=2, drop_lo=0.0, drop_hi=0.0, gyro_bias=0.0, joint_offset=0.0)
    out = run_script(emu, HostMemory(), case)
    check_script(case, out, "host N=17, delay 2 only")
    assert not case.ref.arith_lane.any() and not case.ref.held_lane.any() and (case.ref.delay == 2).all()


def test_clamp_engages(emu):
    case = Case(17, clip=2.0, x_scale=0.6, gyro_bias=3.0, joint_offset=3.0)
    out = run_script(emu, HostMemory(), case)
    check_script(case, out, "host N=17, offsets 3, clip 2")
    arith = case.ref.arith_lane
    assert (np.abs(out[arith]) == 2.0).sum() > 50 and (np.abs(out[arith]) < 2.0).sum() > 50


def test_episode_draws_are_spread_and_change_across_a_reset():
    """the restated draws at N = 300: every integer delay occurs, the drop probabilities reach within 10 % of the range's ends, and an env's delay, drop probability and
    offsets are new after a reset"""
    case = Case(300)
    ref, r = case.ref, case.r
    first = ref.delay[0], ref.p[0]
    assert sorted(set(first[0].tolist())) == list(range(r.delay_lo, r.delay_hi + 1))
    lo, hi = float(np.float32(r.drop_lo)), float(np.float32(r.drop_hi))
    assert lo <= first[1].min() <= lo + 0.1 * (hi - lo) and hi - 0.1 * (hi - lo) <= first[1].max() < hi
    counts = np.bincount(first[0], minlength=5)
    assert counts.min() > 300 / 5 - 5 * np.sqrt(300 * 0.2 * 0.8), counts          # (5 standard deviations of a fair five-sided draw)
    again = np.nonzero(case.dones[3] != 0)[0]
    assert len(again) > 30
    assert (ref.p[2, again] != ref.p[3, again]).all() and (ref.delay[2, again] != ref.delay[3, again]).mean() > 0.6          # (4 in 5 for independent draws)
    gyro = case.kind == K["gyro"]
    assert (ref.bias[2, again][:, gyro] != ref.bias[3, again][:, gyro]).all() and (ref.bias[1] == ref.bias[2]).all()
    assert (np.abs(ref.bias) <= ref.mag[None, None, :]).all() and len(set(ref.bias[0][:, gyro].ravel().tolist())) == 900


def test_argument_checks(emu):
    kind = GO2_KIND.copy()
    p = lambda a: C.c_void_p(a.ctypes.data)
    check = lambda r, kind_=kind, D=45: emu.go2nn_sensor_rand_check(C.byref(r), p(kind_), D)
    assert check(make_rand()) == 0 and check(make_rand(delay_lo=4, delay_hi=4, drop_lo=0.0, drop_hi=0.0, gyro_bias=0.0)) == 0, emu.go2nn_last_error()
    nan, inf = float("nan"), float("inf")
    for bad, name in ((dict(delay_lo=-1), b"delay_lo"), (dict(delay_hi=GO2NN_SENSOR_MAX_DELAY + 1), b"delay_hi"), (dict(delay_lo=3, delay_hi=2), b"delay_lo > delay_hi"),
                      (dict(drop_lo=-0.1), b"drop_lo"), (dict(drop_lo=nan), b"drop_lo"), (dict(drop_hi=1.0), b"drop_hi"), (dict(drop_hi=nan), b"drop_hi"),
                      (dict(drop_lo=0.4, drop_hi=0.3), b"drop_lo > drop_hi"), (dict(gyro_bias=-1.0), b"gyro_bias"), (dict(gyro_bias=inf), b"gyro_bias"),
                      (dict(gravity_bias=nan), b"gravity_bias"), (dict(gravity_bias=-0.5), b"gravity_bias"), (dict(joint_offset=-0.01), b"joint_offset"),
                      (dict(joint_offset=inf), b"joint_offset")):
        assert check(make_rand(**bad)) == EINVAL and name in emu.go2nn_last_error(), (bad, emu.go2nn_last_error())
    for D in (0, GO2NN_SENSOR_MAX_WIDTH + 1):
        assert check(make_rand(), D=D) == EINVAL and b"D = " in emu.go2nn_last_error()
    for v in (-1, 5):
        k2 = kind.copy(); k2[7] = v
        assert check(make_rand(), kind_=k2) == EINVAL and b"kind[7]" in emu.go2nn_last_error()
    assert emu.go2nn_sensor_rand_check(None, p(kind), 45) == EINVAL and emu.go2nn_sensor_rand_check(C.byref(make_rand()), None, 45) == EINVAL
    assert emu.go2nn_sensor_rand_state_bytes(0, 45) == 0 and emu.go2nn_sensor_rand_state_bytes(4, 65) == 0 and emu.go2nn_sensor_rand_state_bytes(4, 0) == 0
    assert emu.go2nn_sensor_rand_state_bytes(4096, 45) == 256 + 7 * 4096 * 45 * 4
    N, D = 4, 45
    obs, dones, out = np.zeros((N, D), np.float32), np.zeros(N, np.uint8), np.zeros((N, D), np.float32)
    state = np.zeros(emu.go2nn_sensor_rand_state_bytes(N, D), np.uint8)
    r = make_rand()

    def make_in():
        a = Go2nnSensorIn()
        a.obs.p, a.obs.env_stride, a.obs.comp_stride = obs.ctypes.data, D, 1
        a.dones, a.scale, a.kind, a.D, a.num_specs, a.clip, a.seed = dones.ctypes.data, None, kind.ctypes.data, D, 0, 100.0, 1
        return a
    full = lambda a, r_=r, n=N: [C.byref(a), C.byref(r_), None, p(state), p(out), n, None]
    assert emu.go2nn_sensor_rand_begin(p(state), None) == 0 and emu.go2nn_sensor_rand_apply(*full(make_in())) == 0, emu.go2nn_last_error()
    assert emu.go2nn_sensor_rand_begin(None, None) == EINVAL and emu.go2nn_last_error()
    for k in (0, 1, 3, 4):          # each required pointer null in turn (also_fresh, argument 2, may be), then N < 1
        args = full(make_in())
        args[k] = None
        assert emu.go2nn_sensor_rand_apply(*args) == EINVAL and emu.go2nn_last_error()
    assert emu.go2nn_sensor_rand_apply(*full(make_in(), n=0)) == EINVAL

    def broken(edit):
        a = make_in()
        edit(a)
        return emu.go2nn_sensor_rand_apply(*full(a))
    for f in ("dones", "kind"):
        assert broken(lambda a: setattr(a, f, None)) == EINVAL and b"null" in emu.go2nn_last_error()
    assert broken(lambda a: setattr(a.obs, "p", None)) == EINVAL and b"null" in emu.go2nn_last_error()
    assert broken(lambda a: setattr(a.obs, "env_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error()
    assert broken(lambda a: setattr(a.obs, "comp_stride", 0)) == EINVAL and b"stride" in emu.go2nn_last_error()
    for D_ in (0, GO2NN_SENSOR_MAX_WIDTH + 1):
        assert broken(lambda a: setattr(a, "D", D_)) == EINVAL and b"D outside" in emu.go2nn_last_error()
    for clip in (0.0, -1.0, nan):
        assert broken(lambda a: setattr(a, "clip", clip)) == EINVAL and b"clip" in emu.go2nn_last_error()
    assert emu.go2nn_sensor_rand_apply(*full(make_in(), r_=make_rand(delay_hi=9))) == EINVAL and b"delay_hi" in emu.go2nn_last_error()
    too_many = (0x7FFFFFFF // 4) // (45 * (R + 2)) + 1          # refused before anything is touched
    assert emu.go2nn_sensor_rand_apply(*full(make_in(), n=too_many)) == EINVAL and b"too large" in emu.go2nn_last_error()
    assert emu.go2nn_sensor_rand_apply(*full(make_in())) == 0


def test_symbols_and_struct_within_abi_7(emu, tmp_path):
    assert emu.go2nn_abi_version() == 7
    libs = [os.path.join(ROOT, "tests", "emu", "libgo2nn_emu.so")] + [p for p in [_nn.NN_LIB] if os.path.exists(p)]
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for f in ("go2nn_sensor_rand_check", "go2nn_sensor_rand_state_bytes", "go2nn_sensor_rand_begin", "go2nn_sensor_rand_apply"):
            assert (" T " + f + "\n") in syms, (path, f)
    names = [n for n, _ in Go2nnSensorRand._fields_]
    assert tuple(names) == SENSOR_RAND_FIELDS and [SENSOR_KINDS.index(k) for k in GO2_OBS_KINDS] == GO2_KIND.tolist()
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "go2nn.h"\nint main(void) { printf("%zu", sizeof(Go2nnSensorRand));\n'
                   + "".join('printf(" %%zu", offsetof(Go2nnSensorRand, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(Go2nnSensorRand)] + [getattr(Go2nnSensorRand, n).offset for n in names] and got[0] == 32


# ---- the environment ---------------------------------------------------------------------------------------------------------------------------------------------
ENVS = 64


def sensor_cfg(task="go2_flat", on=True, episode_length_s=0.3, add_noise=None):
    env_cfg, _ = task_registry.get_cfgs(task)
    env_cfg.domain_rand.randomize_sensors = on
    env_cfg.env.episode_length_s = episode_length_s
    if add_noise is not None:
        env_cfg.noise.add_noise = add_noise
    return env_cfg


def make_env(lib, nn, env_cfg, task="go2_flat", device="cpu", n=ENVS):
    args = get_args(["--task", task, "--num_envs", str(n), "--headless", "--seed", "7"] + (["--sim_device", "cpu", "--rl_device", "cpu"] if device == "cpu" else []))
    env, _ = task_registry.make_env(task, args, env_cfg=env_cfg, lib=lib, **({"nn": nn} if nn is not None else {}))
    return env, args


def env_rand(env):
    """the ranges as the kernel must have been given them, from the config alone"""
    d, o = env.cfg.domain_rand, env.cfg.normalization.obs_scales
    return make_rand(env._env_offset, delay_lo=d.sensor_delay_range[0], delay_hi=d.sensor_delay_range[1], drop_lo=d.sensor_drop_range[0], drop_hi=d.sensor_drop_range[1],
                     gyro_bias=d.sensor_gyro_bias * o.ang_vel, gravity_bias=d.sensor_gravity_bias, joint_offset=d.sensor_joint_offset * o.dof_pos)


def test_defaults_are_off_and_the_evaluator_switches_it_off():
    from go2_rl_gym_amd.utils.evaluator import evaluation_env_cfg
    for task in ("go2_flat", "go2", "go2_flat_cts"):
        d = task_registry.get_cfgs(task)[0].domain_rand
        assert d.randomize_sensors is False and d.sensor_delay_range == [0, 2] and d.sensor_drop_range == [0.0, 0.2]
        assert (d.sensor_gyro_bias, d.sensor_gravity_bias, d.sensor_joint_offset) == (0.1, 0.0, 0.05)
    env_cfg, train_cfg = task_registry.get_cfgs("go2_flat")
    env_cfg.domain_rand.randomize_sensors = True
    from go2_rl_gym_amd.utils.helpers import class_to_dict
    assert evaluation_env_cfg(env_cfg, dict(class_to_dict(train_cfg.evaluation), **th.EVAL)).domain_rand.randomize_sensors is False


def actions_of(steps, n=ENVS):
    return torch.from_numpy(np.random.default_rng(5).normal(0, 0.6, (steps, n, 12)).astype(np.float32))


def test_flag_off_is_the_plain_simulator(emu):
    """no sensor state, step() returns obs_buf itself, and 30 steps give the bytes of a second handle driven through the C ABI directly"""
    lib = load_oracle()
    env, _ = make_env(lib, emu, sensor_cfg(on=False))
    assert env._sensors is None and not any("sensor" in k for k in vars(env))
    h = C.c_void_p()
    _abi.check(lib, lib.go2sim_create(C.byref(env._c), 0, C.byref(h)), "go2sim_create")
    from helpers import HostSim
    twin = HostSim.__new__(HostSim)
    twin.lib, twin.abi, twin._keep, twin.real = lib, lib.abi, [], np.float32
    twin._wrap(h, ENVS)
    twin.reset_all()
    twin.step(np.zeros((ENVS, 12), np.float32))
    obs, _ = env.reset()
    assert obs is env.obs_buf and env.get_observations() is env.obs_buf
    acts = actions_of(30).to(env.device)
    for a in acts:
        got = env.step(a)
        twin.step(a.cpu().numpy())
        assert got[0] is env.obs_buf and got[0].cpu().numpy().tobytes() == np.ascontiguousarray(twin.obs_buf).tobytes()
    assert np.ascontiguousarray(twin.rew_buf).tobytes() == env.rew_buf.cpu().numpy().tobytes()
    twin.close()
    env.close()


STEPS = 40
OUTSIDE = {17: [3, 20, 21, 50]}          # a reset_idx from outside a step, before step 17


def drive(env, rows):
    """reset, then STEPS steps (plain, or through rollout rows of a [STEPS + 1, N, 45] tensor with the last step left to the delivered buffer) -> the simulator's frames,
    the fresh flags and the frames the policy was handed, [STEPS + 1, N, ...]; row 0 is what reset() left"""
    N, dev = env.num_envs, env.obs_buf.device
    cpu = lambda t: t.detach().cpu().numpy().copy()
    obs, _ = env.reset()
    env.episode_length_buf = torch.from_numpy(np.random.default_rng(6).integers(0, int(env.max_episode_length), N)).to(env.episode_length_buf)          # time-outs out of step
    x, fresh, got = [cpu(env.obs_buf)], [np.ones(N, bool)], [cpu(obs)]
    assert obs is env.get_observations() and obs is not env.obs_buf
    store = torch.zeros(STEPS + 1, N, 45, device=dev)
    priv, val, rew, don = torch.zeros(N, 263, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    for t, a in enumerate(actions_of(STEPS, N).to(dev), start=1):
        outside = np.zeros(N, bool)
        if t in OUTSIDE:
            env.reset_idx(torch.tensor(OUTSIDE[t], device=dev))
            outside[OUTSIDE[t]] = True
        if rows:
            dst = store[t] if t < STEPS else None
            obs, p, _, dones, info = env.step(a, rollout={"obs_out": dst, "priv_out": priv, "values": val, "rewards_out": rew, "dones_out": don, "gamma": 0.99})
            assert info["transition_stored"] and (obs is dst if dst is not None else obs is env.get_observations()) and p is priv
            assert (don.cpu().numpy() != 0).tolist() == cpu(dones).astype(bool).tolist()
        else:
            obs, p, _, dones, _ = env.step(a)
            assert obs is env.get_observations() and p is env.privileged_obs_buf
        x.append(cpu(env.obs_buf)); fresh.append(cpu(dones).astype(bool) | outside); got.append(cpu(obs))
    return np.stack(x), np.stack(fresh), np.stack(got)


def check_env_run(env, x, fresh, got, what):
    ref = Restated(x, fresh, GO2_KIND, env_rand(env), int(env.cfg.seed) & M32, float(env.cfg.normalization.clip_observations))
    ref.check(got, what)
    inner = fresh[1:].sum()
    assert inner > 2 * env.num_envs and ref.held_lane.any() and (ref.delay > 0).any() and fresh[17][OUTSIDE[17]].all()          # time-outs fall inside the run
    assert (bits(got) != bits(x)).any()
    return ref


def test_env_steps_against_the_restatement(emu, capsys):
    lib = load_oracle()
    env, _ = make_env(lib, emu, sensor_cfg())
    assert "randomize_sensors" in capsys.readouterr().out
    x, fresh, got = drive(env, rows=False)
    check_env_run(env, x, fresh, got, "env, 40 plain steps")
    env.close()
    # through rollout rows: the same frames in the rows the caller named, and obs_buf keeps the simulator's own frame
    env2, _ = make_env(lib, emu, sensor_cfg())
    x2, fresh2, got2 = drive(env2, rows=True)
    check_env_run(env2, x2, fresh2, got2, "env, 40 steps through rollout rows")
    assert x2.tobytes() == x.tobytes() and fresh2.tobytes() == fresh.tobytes() and got2.tobytes() == got.tobytes()
    env2.close()


def test_env_refuses_what_it_cannot_randomise(emu):
    lib = load_oracle()
    cfg = sensor_cfg()
    cfg.domain_rand.sensor_delay_range = [0, GO2NN_SENSOR_MAX_DELAY + 1]
    with pytest.raises(ValueError, match="delay_hi"):
        make_env(lib, emu, cfg)
    cfg = sensor_cfg()
    cfg.domain_rand.sensor_delay_range = [0.5, 2]
    with pytest.raises(ValueError, match="whole policy steps"):
        make_env(lib, emu, cfg)
    from go2_rl_gym_amd.envs.base.legged_robot import LeggedRobot
    from go2_rl_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    args = get_args(["--task", "go2_flat", "--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"])
    cfg = sensor_cfg()
    cfg.env.num_envs = 8
    with pytest.raises(ValueError, match="no observation layout"):          # (the base class has no column layout of its own)
        LeggedRobot(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, "cpu", True, lib=lib, nn=emu)


def test_evaluator_ignores_the_flag(emu):
    from go2_rl_gym_amd.utils.evaluator import PolicyEvaluator
    ac = th.small_actor_critic()
    tables = []
    for on in (False, True):
        cfg = sensor_cfg(on=on, episode_length_s=task_registry.get_cfgs("go2_flat")[0].env.episode_length_s)
        ev = PolicyEvaluator(cfg, dict(th.EVAL), task_class=task_registry.get_task_class("go2_flat"), device="cpu", lib=load_oracle(), nn_lib=emu)
        tables.append(ev.evaluate(ac)["table"].tobytes())
        assert ev.env._sensors is None
        ev.close()
    assert tables[0] == tables[1]


# ---- the runners -------------------------------------------------------------------------------------------------------------------------------------------------
def make_runner(lib, nn, task, on, device="cpu", episode_length_s=0.2):
    env, args = make_env(lib, nn if on else None, sensor_cfg(task, on=on, episode_length_s=episode_length_s, add_noise=False), task=task, device=device)
    runner, _ = task_registry.make_alg_runner(env, task, args, log_root=None)
    return env, runner


def check_storage(env, runner, what):
    """restate the last rollout from the storage alone: clean frames privileged_observations[s][:, 3:48], delivered frames observations[s], the dones rows, and the cursor
    read back from the state — every lane of every env from its first reset inside the rollout onwards.  -> the share of (row >= 1, env) pairs so checked"""
    st = runner.alg.storage
    T, N = st.observations.shape[:2]
    clean, got = st.privileged_observations[:, :, 3:48].cpu().numpy().copy(), st.observations.cpu().numpy().copy()
    dones = st.dones.cpu().numpy().reshape(T, N) != 0
    cursor = int(env._sensors["state"][:4].cpu().numpy().view(np.int32)[0])
    fresh = np.zeros((T, N), bool)
    fresh[1:] = dones[:-1]
    ref = Restated(clean, fresh, GO2_KIND, env_rand(env), int(env.cfg.seed) & M32, float(env.cfg.normalization.clip_observations), cursor0=cursor - (T + 1), known0=False)
    assert cursor > T + 1 and not ref.known[0].any()
    ref.check(got, what)
    share = float(ref.known[1:].mean())
    print("%s: cursor %d, %.1f %% of the (row >= 1, env) lanes restated" % (what, cursor, 100 * share))
    assert share >= 0.5 and ref.held_lane.any() and (ref.src_row[ref.copy_lane] < np.broadcast_to(np.arange(T)[:, None, None], ref.copy_lane.shape)[ref.copy_lane]).any()
    # the frame after the rollout's last step: the delivered buffer, from obs_buf and the last dones row
    last = Restated(np.concatenate([clean, env.obs_buf.cpu().numpy()[None]]), np.concatenate([fresh, dones[-1:]]), GO2_KIND, env_rand(env), int(env.cfg.seed) & M32,
                    float(env.cfg.normalization.clip_observations), cursor0=cursor - (T + 1), known0=False)
    last.check(np.concatenate([got, env.get_observations().cpu().numpy()[None]]), what + " + the delivered buffer")
    return share


@pytest.mark.parametrize("task", ["go2_flat", "go2_flat_cts"])
def test_runner_storage_against_the_restatement(emu, monkeypatch, task):
    monkeypatch.setenv("GO2_FUSE_STEP", "1")          # the env step writes the storage rows on the CPU too
    lib = load_oracle()
    env, runner = make_runner(lib, emu, task, on=False)
    runner.learn(1, init_at_random_ep_len=True)
    st = runner.alg.storage
    assert env._sensors is None and bits(st.privileged_observations[:, :, 3:48].numpy()).tobytes() == bits(st.observations.numpy()).tobytes()
    env.close()
    env, runner = make_runner(lib, emu, task, on=True)
    runner.learn(2, init_at_random_ep_len=True)
    check_storage(env, runner, "%s on the host libraries" % task)
    assert all(np.isfinite(p.detach().numpy()).all() for p in runner.alg.actor_critic.parameters()) if hasattr(runner.alg, "actor_critic") else True
    if task.endswith("cts"):          # the student's history was fed the delivered frames
        assert bits(runner.history[:, -1].numpy()).tobytes() == bits(env.get_observations().numpy()).tobytes()
        assert bits(runner.history[:, -1].numpy()).tobytes() != bits(env.obs_buf.numpy()).tobytes()
    env.close()
