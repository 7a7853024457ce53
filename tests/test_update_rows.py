"""The small "row" entry points of include/go2sim.h that sit between the GEMMs of every rollout step and every mini-batch — go2sim_gae / go2sim_normalize_advantages,
go2sim_ppo_loss, go2sim_act_head, go2sim_store_transition, go2sim_history_push, go2sim_adam_clip_step — at the smallest shapes that reach each of their tail paths,
against a float64 numpy restatement of the reference's formulas (rollout_storage.py:123-137, ppo.py:104-114, ppo.py:131-181).

Every checker is check_*(lib, device, case...): here it runs on the two host builds (the oracle and the lane emulation), which is where the restatements, the input
constructions and the bounds are shown to be right; tests/test_gpu_update_rows.py hands the same checkers the HIP library on cuda:0.

The bound of every compared output: with e(x) = max |x - ref64| / max |ref64| and the yardstick the SAME restatement evaluated in float32 numpy (reductions summed
sequentially), e(kernel) <= 4 * e(yardstick) + 2^-23 (one float32 ulp at the output's scale).  Outputs that are exact by construction are compared with ==.
Passive memory checks: every output has PAD sentinel elements behind its end (and in front of it where it starts at an offset), workspaces start as NaN, optional
outputs handed in as NULL have a sentinel-filled stand-in.

Measured on the two host builds (largest e_kernel with the e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound):
  GAE returns / advantages      4.6e-7 (4.6e-7)   0.23   T=24 N=255
  normalize                     1.1e-7 (5.4e-7)   0.19   T=5 N=64, count 320
  loss head gmu/gstd/gval/stats 8.4e-6 (8.4e-6)   0.81   B=65 A=12 split=64 (one student row of weight 1: its ratio's rounding is the whole error)
  act head log-probability      2.2e-7 (2.2e-7)   0.28   N=15 A=12
  Adam param / moments / lr     2.1e-7 (6.5e-6)   0.20   numel 4095
  store transition              0.91 of its two-rounding bound
(the device's figures: tests/test_gpu_update_rows.py)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import load_emu, load_oracle

F32, F64 = np.float32, np.float64
PAD = 64
ULP = 2.0 ** -23
SENT = {torch.float32: -12345.0, torch.float64: -12345.0, torch.uint8: 0xA5}
WHICH = ["oracle", "lane_emulation"]
host_lib = lambda which: load_oracle() if which == "oracle" else load_emu()


class Buf:
    """n elements of device memory with `front` sentinel elements before them and PAD behind"""

    def __init__(self, device, n, init=None, dtype=torch.float32, front=0):
        self.n, self.front, self.sent = n, front, SENT[dtype]
        self.t = torch.full((front + n + PAD,), self.sent, dtype=dtype, device=device)
        if init is not None:
            self.t[front:front + n] = init if np.isscalar(init) else torch.as_tensor(np.ascontiguousarray(init).reshape(-1)).to(device)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.front * self.t.element_size())

    def get(self):
        return self.t[self.front:self.front + self.n].cpu().numpy()

    def intact(self):
        return bool((self.t[self.front + self.n:] == self.sent).all()) and bool((self.t[:self.front] == self.sent).all())

    def untouched(self):
        return bool((self.t == self.sent).all())


def dev_in(x, device):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device)


P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
stream_of = lambda device: C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None


def sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def seqsum(x, dt):
    """sum over axis 0, one addend after the other in `dt`"""
    return np.cumsum(np.asarray(x, dt), axis=0, dtype=dt)[-1]


def nerr(x, ref):
    ref = np.asarray(ref, F64)
    s = float(np.abs(ref).max())
    return float(np.abs(np.asarray(x, F64).reshape(ref.shape) - ref).max()) / (s if s > 0 else 1.0)


def within(tag, got, yard, ref):
    """e_kernel <= 4 e_yardstick + one float32 ulp, both normalised by max |ref|"""
    ek, ey = nerr(got, ref), nerr(yard, ref)
    print("[update_rows] %s: e_kernel %.3e e_yardstick %.3e (of bound: %.2f)" % (tag, ek, ey, ek / (4 * ey + ULP)))
    assert np.isfinite(np.asarray(got)).all(), tag
    assert ek <= 4 * ey + ULP, (tag, ek, ey)


# ---- GAE + advantage normalisation (rollout_storage.py:123-137) -------------------------------------------------------------------------
GAE_SHAPES = [(1, 1), (3, 63), (5, 64), (4, 65), (24, 255), (7, 257), (24, 1000)]
GAE_DONES = ["none", "all", "random", "last"]
GAMMA, LAM = float(F32(0.99)), float(F32(0.95))


def gae_restated(rew, dones, val, last, dt):
    rew, val, last, gamma, lam = rew.astype(dt), val.astype(dt), last.astype(dt), dt(GAMMA), dt(LAM)
    T = rew.shape[0]
    ret, a = np.empty_like(rew), np.zeros_like(last)
    for t in reversed(range(T)):
        nv = last if t == T - 1 else val[t + 1]
        nt = dt(1.0) - dones[t].astype(dt)
        delta = rew[t] + nt * gamma * nv - val[t]
        a = delta + nt * gamma * lam * a
        ret[t] = a + val[t]
    return ret, ret - val


def normalize_restated(a, count, dt):
    """(adv - mean) / (std + 1e-8), unbiased std, statistics over all of `a`; the first `count` elements"""
    a = a.astype(dt).reshape(-1)
    n = dt(a.size)
    if dt is F64:
        mean = dt(math.fsum(a) / a.size)
        sd = dt(math.sqrt(math.fsum((a - mean) ** 2) / (a.size - 1)))
    else:
        mean = seqsum(a, dt) / n
        sd = np.sqrt(seqsum((a - mean) ** 2, dt) / (n - dt(1.0)))
    return (a[:count] - mean) / (sd + dt(1e-8))


def check_gae(lib, device, T, N, pattern):
    rng = np.random.default_rng(1000 * T + N)
    rew, val, last = (0.5 * rng.normal(size=(T, N))).astype(F32), rng.normal(size=(T, N)).astype(F32), rng.normal(size=N).astype(F32)
    u = rng.uniform(size=(T, N))
    dones = {"none": np.zeros((T, N)), "all": np.ones((T, N)), "random": u < 0.1, "last": np.arange(T)[:, None] + np.zeros(N) == T - 1}[pattern].astype(np.uint8)
    st, n = stream_of(device), T * N
    ins = [dev_in(x, device) for x in (rew, dones, val, last)]
    ret, adv, part = Buf(device, n), Buf(device, n), Buf(device, 3, 0.0, torch.float64)
    assert lib.go2sim_gae(*[P(x) for x in ins], ret.ptr, adv.ptr, part.ptr, T, N, GAMMA, LAM, st) == 0, lib.go2sim_last_error()
    sync(device)
    tag = "gae T=%d N=%d dones=%s" % (T, N, pattern)
    r64, a64 = gae_restated(rew, dones, val, last, F64)
    r32, a32 = gae_restated(rew, dones, val, last, F32)
    ak = adv.get()
    within(tag + " returns", ret.get(), r32, r64)
    within(tag + " advantages", ak, a32, a64)
    assert ret.intact() and adv.intact() and part.intact()
    # the block sums against the float64 sums of the kernel's own advantages: n addends, each addition rounds once in float64
    p, x = part.get(), ak.astype(F64).reshape(-1)
    assert p[2] == n
    assert abs(p[0] - math.fsum(x)) <= n * 2.0 ** -53 * math.fsum(np.abs(x)), (tag, p[0], math.fsum(x))
    assert abs(p[1] - math.fsum(x * x)) <= n * 2.0 ** -53 * math.fsum(x * x), (tag, p[1], math.fsum(x * x))
    if n == 1:
        return          # (the reference's std of one sample is NaN as well)
    for count in sorted({N, n}):
        buf = Buf(device, n, ak)
        assert lib.go2sim_normalize_advantages(buf.ptr, part.ptr, count, st) == 0, lib.go2sim_last_error()
        sync(device)
        out = buf.get()
        within(tag + " normalize count=%d" % count, out[:count], normalize_restated(ak, count, F32), normalize_restated(ak, count, F64))
        assert np.array_equal(out[count:], ak.reshape(-1)[count:]) and buf.intact()


def check_normalize_grid_stride(lib, device):
    """count = 2048 * 256 + 1: one element more than the largest grid covers in one trip"""
    count = 2048 * 256 + 1
    x = (2.0 * np.random.default_rng(7).normal(size=count) + 0.5).astype(F32)
    x64 = x.astype(F64)
    part, buf = Buf(device, 3, np.array([x64.sum(), (x64 * x64).sum(), float(count)]), torch.float64), Buf(device, count, x)
    assert lib.go2sim_normalize_advantages(buf.ptr, part.ptr, count, stream_of(device)) == 0, lib.go2sim_last_error()
    sync(device)
    within("normalize count=%d" % count, buf.get(), normalize_restated(x, count, F32), normalize_restated(x, count, F64))
    assert buf.intact() and part.intact()
    assert lib.go2sim_normalize_advantages(buf.ptr, part.ptr, 0, None) < 0 and lib.go2sim_normalize_advantages(None, part.ptr, 4, None) < 0


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("pattern", GAE_DONES)
@pytest.mark.parametrize("T,N", GAE_SHAPES)
def test_gae_and_normalize(which, T, N, pattern):
    check_gae(host_lib(which), "cpu", T, N, pattern)


@pytest.mark.parametrize("which", WHICH)
def test_normalize_grid_stride(which):
    check_normalize_grid_stride(host_lib(which), "cpu")


# ---- the loss head (ppo.py:131-170) --------------------------------------------------------------------------------------------------------
CLIP, VCOEF, ECOEF = float(F32(0.2)), 0.75, float(F32(0.01))


def _loss_cases():
    cases = []
    for B in (65, 4099):          # every value of every axis at a ragged small and a ragged multi-block size
        cases += [(B, 1, 1, 0), (B, 5, 0, 1), (B, 12, 1, B - 1), (B, 16, 0, 37), (B, 12, 0, 0), (B, 16, 1, 1), (B, 1, 0, 37), (B, 5, 1, B - 1)]
    cases += [(1, 12, 1, 0), (1, 1, 0, 0), (15, 5, 0, 1), (15, 16, 1, 14), (63, 16, 1, 37), (63, 1, 0, 62), (64, 12, 1, 37), (64, 5, 0, 0), (64, 16, 0, 63),
              (200, 12, 1, 37), (200, 16, 0, 199), (200, 1, 1, 1), (200, 5, 0, 0)]
    return cases


LOSS_CASES = _loss_cases()          # (B, A, use_clip_v, split)


def loss_restated(ins, B, A, use_clip_v, split, dt):
    """surrogate / value / KL / entropy terms of ppo.py:131-171 and the gradients of `loss` with respect to mu, std and value, written out by hand"""
    mu, std, value, acts, old_mu, old_sig, old_lp, adv, tv, ret = [x.astype(dt) for x in ins]
    clip, vcoef, ecoef, one, half, two = dt(CLIP), dt(VCOEF), dt(ECOEF), dt(1.0), dt(0.5), dt(2.0)
    log2pi = dt(math.log(2.0 * math.pi))
    wr = np.full(B, one / dt(B), dt)
    if 0 < split < B:          # CTS: the surrogate's mean is taken over the teacher rows and the student rows separately
        wr[:split], wr[split:] = one / dt(split), one / dt(B - split)
    d = acts - mu
    lp = seqsum((-(d * d) / (two * std * std) - np.log(std) - half * log2pi).T, dt)
    ent = seqsum((half + half * log2pi + np.log(std))[:, None] + np.zeros((A, B), dt), dt)
    kl = seqsum((np.log(std / old_sig + dt(1e-5)) + (old_sig * old_sig + (old_mu - mu) ** 2) / (two * std * std) - half).T, dt)
    ratio = np.exp(lp - old_lp)
    lo, hi = one - clip, one + clip
    rc, inb = np.clip(ratio, lo, hi), ((ratio >= lo) & (ratio <= hi)).astype(dt)
    s1, s2 = -adv * ratio, -adv * rc
    sur = np.maximum(s1, s2)
    w = np.where(s1 > s2, one, np.where(s1 < s2, inb, half + half * inb))          # torch.max hands a tie half the gradient each; clamp passes it inside [lo, hi]
    g_lp = -adv * w * ratio * wr
    dv = value - tv
    l1 = (value - ret) ** 2
    if use_clip_v:
        vc = tv + np.clip(dv, -clip, clip)
        vin = ((dv >= -clip) & (dv <= clip)).astype(dt)
        l2 = (vc - ret) ** 2
        vl = np.maximum(l1, l2)
        g1, g2 = two * (value - ret), two * (vc - ret) * vin
        gv = np.where(l1 > l2, g1, np.where(l1 < l2, g2, half * g1 + half * g2))
    else:
        l2 = (tv + np.clip(dv, -clip, clip) - ret) ** 2          # (only the input construction looks at it)
        vl, gv = (ret - value) ** 2, two * (value - ret)
    gmu = g_lp[:, None] * d / (std * std)
    gstd = seqsum(g_lp[:, None] * (d * d / (std * std * std) - one / std), dt) - ecoef / std
    gval = vcoef * gv / dt(B)
    s = [seqsum(sur * wr, dt), seqsum(vl, dt) / dt(B), seqsum(kl, dt) / dt(B), seqsum(ent, dt) / dt(B)]
    stats = np.array(s + [s[0] + vcoef * s[1] - ecoef * s[3]], dt)
    return dict(gmu=gmu, gstd=gstd, gval=gval, stats=stats, ratio=ratio, dv=dv, l1=l1, l2=l2)


def loss_inputs(B, A):
    """the inputs of test_fused_ppo_loss_kernel_on_gpu, about 5 % of the advantages exactly 0, and no row within 1e-3 of a discontinuity of the loss (in float64):
    the ratio at 1 +- clip (rows of zero advantage are exempt: their surrogate and its gradient are 0 on either side), |v - tv| at clip, l1 = l2 outside the clip"""
    rng = np.random.default_rng(B * 100 + A)
    f = lambda *s: rng.normal(size=s).astype(F32)
    mu, std, value, acts = f(B, A), (0.6 + 0.3 * rng.uniform(size=A)).astype(F32), f(B), f(B, A)
    old_mu, old_sig = mu + 0.1 * f(B, A), (0.7 + 0.2 * rng.uniform(size=(B, A))).astype(F32)
    lp = (-((acts - mu) ** 2) / (2 * std ** 2) - np.log(std) - 0.9189385).sum(1).astype(F32)
    adv = f(B)
    adv[rng.uniform(size=B) < 0.05] = 0.0
    old_lp, tv, ret = lp + 0.3 * f(B), value + 0.3 * f(B), value + f(B)

    def offenders():
        r = loss_restated([mu, std, value, acts, old_mu, old_sig, old_lp, adv, tv, ret], B, A, 1, 0, F64)
        edge = (np.minimum(np.abs(r["ratio"] - (1 - CLIP)), np.abs(r["ratio"] - (1 + CLIP))) < 1e-3) & (adv != 0)
        edge |= np.abs(np.abs(r["dv"]) - CLIP) < 1e-3
        edge |= (np.abs(r["l1"] - r["l2"]) < 1e-3) & (np.abs(r["dv"]) > CLIP)
        return edge, r

    for _ in range(1000):
        bad, r = offenders()
        if not bad.any():
            break
        k = int(bad.sum())
        old_lp[bad], tv[bad], ret[bad] = lp[bad] + 0.3 * f(k), value[bad] + 0.3 * f(k), value[bad] + f(k)
    bad, r = offenders()
    assert not bad.any()
    if B >= 200:          # every branch of the loss holds at least a tenth of the rows
        share = [r["ratio"] < 1 - CLIP, (r["ratio"] >= 1 - CLIP) & (r["ratio"] <= 1 + CLIP), r["ratio"] > 1 + CLIP, adv > 0, adv < 0,
                 r["dv"] < -CLIP, np.abs(r["dv"]) <= CLIP, r["dv"] > CLIP]
        assert min(float(m.mean()) for m in share) >= 0.1, [float(m.mean()) for m in share]
    return [mu, std, value, acts, old_mu, old_sig, old_lp, adv, tv, ret]


def _run_loss(lib, device, t, B, A, use_clip_v, split, fill=None):
    nb = max(1, (B + 63) // 64)
    out = [Buf(device, max(B, 1) * max(A, 1), fill), Buf(device, max(A, 1), fill), Buf(device, max(B, 1), fill), Buf(device, 5, fill)]          # gmu, gstd, gval, stats
    ws = Buf(device, 24 * nb, float("nan"))
    rc = lib.go2sim_ppo_loss(*[P(x) for x in t], *[o.ptr for o in out], ws.ptr, B, A, CLIP, VCOEF, ECOEF, use_clip_v, split, stream_of(device))
    sync(device)
    return rc, out, ws


def check_ppo_loss(lib, device, B, A, use_clip_v, split):
    ins = loss_inputs(B, A)
    t = [dev_in(x, device) for x in ins]
    rc, out, ws = _run_loss(lib, device, t, B, A, use_clip_v, split)
    assert rc == 0, lib.go2sim_last_error()
    ref, yard = loss_restated(ins, B, A, use_clip_v, split, F64), loss_restated(ins, B, A, use_clip_v, split, F32)
    tag = "ppo_loss B=%d A=%d clip_v=%d split=%d" % (B, A, use_clip_v, split)
    got = dict(zip(("gmu", "gstd", "gval", "stats"), [o.get() for o in out]))
    for k in ("gmu", "gstd", "gval", "stats"):
        within(tag + " " + k, got[k].reshape(ref[k].shape), yard[k], ref[k])
    assert all(o.intact() for o in out) and ws.intact()
    if lib.go2sim_is_device_library():          # the block partials the finish kernel reads: all written (columns >= 4 + A hold nothing that is read back)
        assert np.isfinite(ws.get().reshape(-1, 24)[:, :4 + A]).all()
    rc, again, _ = _run_loss(lib, device, t, B, A, use_clip_v, split)          # a fixed summation order: bit-equal from call to call
    assert rc == 0 and all(np.array_equal(a.get().view(np.uint32), b.get().view(np.uint32)) for a, b in zip(out, again))


def check_ppo_loss_refusals(lib, device):
    ins = loss_inputs(15, 16)
    t = [dev_in(x, device) for x in ins]
    for B, A in ((15, 0), (15, 17), (0, 16)):
        rc, out, ws = _run_loss(lib, device, t, B, A, 1, 0, fill=SENT[torch.float32])
        assert rc < 0 and all(o.untouched() for o in out), (B, A)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("B,A,use_clip_v,split", LOSS_CASES)
def test_ppo_loss(which, B, A, use_clip_v, split):
    check_ppo_loss(host_lib(which), "cpu", B, A, use_clip_v, split)


@pytest.mark.parametrize("which", WHICH)
def test_ppo_loss_refusals(which):
    check_ppo_loss_refusals(host_lib(which), "cpu")


def test_loss_cases_cover_every_axis_value_at_both_ragged_sizes():
    for B in (65, 4099):
        mine = [c for c in LOSS_CASES if c[0] == B]
        assert {c[1] for c in mine} == {1, 5, 12, 16} and {c[2] for c in mine} == {0, 1} and {c[3] for c in mine} == {0, 1, B - 1, 37}
    assert {c[0] for c in LOSS_CASES} == {1, 15, 63, 64, 65, 200, 4099}


# ---- the rollout's sampling head (ppo.py:104-114 with the act() above it) and the transition it stores -----------------------------------------
ACT_CASES = [(N, A) for N in (1, 15, 16, 17, 63, 65, 1000) for A in (1, 12, 16)] + [(N, A) for N in (1, 65, 300) for A in (17, 33)]
ACT_POINTERS = ["all", "lp_only", "none"]


def logp_restated(a, mu, std, dt):
    """Normal(mu, std).log_prob(a).sum(-1)"""
    a, mu, std = a.astype(dt), mu.astype(dt), std.astype(dt)
    d = a - mu
    return seqsum((-(d * d) / (dt(2.0) * std * std) - np.log(std) - dt(0.5 * math.log(2.0 * math.pi))).T, dt)


def check_act_head(lib, device, N, A):
    g = torch.Generator().manual_seed(N * 100 + A)
    mu, eps, value, std = torch.randn(N, A, generator=g), torch.randn(N, A, generator=g), torch.randn(N, generator=g), 0.3 + torch.rand(A, generator=g)
    a = mu + std * eps          # two float32 operations, as the eager formulation has them
    ins = [x.to(device) for x in (mu, std, eps, value)]
    sig = (mu * 0 + std).numpy()
    lp64, lp32 = logp_restated(a.numpy(), mu.numpy(), std.numpy(), F64), logp_restated(a.numpy(), mu.numpy(), std.numpy(), F32)
    for ptrs in ACT_POINTERS:
        a_out, a_st, mu_st, sig_st, lp_st, v_st = [Buf(device, N * A, SENT[torch.float32]) for _ in range(4)] + [Buf(device, N, SENT[torch.float32]) for _ in range(2)]
        given = {"all": [a_st, mu_st, sig_st, lp_st, v_st], "lp_only": [lp_st], "none": []}[ptrs]
        opt = [b.ptr if b in given else None for b in (a_st, mu_st, sig_st, lp_st, v_st)]
        rc = lib.go2sim_act_head(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]) if ptrs != "none" else None, a_out.ptr, *opt, N, A, stream_of(device))
        assert rc == 0, lib.go2sim_last_error()
        sync(device)
        assert np.array_equal(a_out.get().reshape(N, A), a.numpy()) and a_out.intact()
        for b, want in ((a_st, a.numpy()), (mu_st, mu.numpy()), (sig_st, sig), (v_st, value.numpy())):
            if b in given:
                assert np.array_equal(b.get(), want.reshape(-1)) and b.intact()
            else:
                assert b.untouched()
        if lp_st in given:
            within("act_head N=%d A=%d %s lp" % (N, A, ptrs), lp_st.get(), lp32, lp64)
            assert lp_st.intact()
        else:
            assert lp_st.untouched()
    assert lib.go2sim_act_head(P(ins[0]), P(ins[1]), P(ins[2]), None, a_out.ptr, None, None, None, None, v_st.ptr, N, A, None) < 0          # v_st without value


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,A", ACT_CASES)
def test_act_head(which, N, A):
    check_act_head(host_lib(which), "cpu", N, A)


STORE_N = [1, 255, 256, 257]


def check_store_transition(lib, device, N):
    rng = np.random.default_rng(N)
    rew, v = rng.normal(size=N).astype(F32), rng.normal(size=N).astype(F32)
    dones, touts = (rng.uniform(size=N) < 0.3).astype(np.uint8), (rng.uniform(size=N) < 0.5).astype(np.uint8)
    if N > 1:
        touts[:2] = (0, 1)
    t = [dev_in(x, device) for x in (rew, dones, touts, v)]
    for with_touts in (True, False):
        rst, dst = Buf(device, N), Buf(device, N, dtype=torch.uint8)
        rc = lib.go2sim_store_transition(P(t[0]), P(t[1]), P(t[2]) if with_touts else None, P(t[3]) if with_touts else None, rst.ptr, dst.ptr, GAMMA, N, stream_of(device))
        assert rc == 0, lib.go2sim_last_error()
        sync(device)
        assert np.array_equal(dst.get(), dones) and dst.intact() and rst.intact()
        if with_touts:          # rewards + gamma * values * time_outs: one rounding of the product, one of the sum (none of the product where the two are contracted)
            prod = GAMMA * v.astype(F64) * touts
            ref = rew.astype(F64) + prod
            err = np.abs(rst.get().astype(F64) - ref)
            print("[update_rows] store_transition N=%d: max error %.3e of bound %.2f" % (N, err.max(), (err / (2.0 ** -24 * (np.abs(prod) + np.abs(ref)) * (1 + ULP) + 1e-300)).max()))
            assert (err <= 2.0 ** -24 * (np.abs(prod) + np.abs(ref)) * (1 + ULP)).all()
        else:
            assert np.array_equal(rst.get(), rew)
    assert lib.go2sim_store_transition(P(t[0]), P(t[1]), P(t[2]), None, rst.ptr, dst.ptr, GAMMA, N, None) < 0          # time-outs without values


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N", STORE_N)
def test_store_transition(which, N):
    check_store_transition(host_lib(which), "cpu", N)


# ---- the CTS observation-history ring (on_policy_runner_cts.py:155-156) ------------------------------------------------------------------
HISTORY_CASES = [(1, 1, 3), (7, 2, 45), (33, 6, 7), (300, 5, 45)]


def check_history_push(lib, device, N, H, D):
    rng = np.random.default_rng(N * 100 + H)
    want = rng.normal(size=(N, H, D)).astype(F32)
    hist = Buf(device, N * H * D, want)
    for it in range(3):
        obs = rng.normal(size=(N, D)).astype(F32)
        dones = (rng.uniform(size=N) < 0.3).astype(np.uint8) if it else None
        if dones is not None:
            want[dones > 0] = 0.0
        want = np.concatenate([want[:, 1:], obs[:, None]], axis=1)
        do, dd = dev_in(obs, device), (dev_in(dones, device) if dones is not None else None)
        assert lib.go2sim_history_push(hist.ptr, P(do), P(dd), N, H, D, stream_of(device)) == 0, lib.go2sim_last_error()
        sync(device)
        assert np.array_equal(hist.get().reshape(N, H, D), want) and hist.intact()
    assert lib.go2sim_history_push(hist.ptr, P(do), None, N, 0, D, None) < 0


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,H,D", HISTORY_CASES)
def test_history_push(which, N, H, D):
    check_history_push(host_lib(which), "cpu", N, H, D)


# ---- clip_grad_norm_ + adaptive-KL learning rate + Adam (ppo.py:140-155,178-181) ------------------------------------------------------------
# (numel, float offset of param / grad / exp_avg / exp_avg_sq into their buffers): offsets of 4 keep the 16-byte alignment, odd ones break it
ADAM_TENSORS = [(n, (4, 4, 4, 4)) for n in (1, 3, 4, 5, 12, 4095, 4096, 4097, 8195)] + [(4096, (1, 1, 1, 1)), (37, (4, 1, 4, 4)), (2, (1, 1, 1, 1))]
ADAM_STEPS = [(3.0, 0.05), (0.01, None), (1.0, 0.001)]          # (gradient scale, kl_mean): clipped + lr down, not clipped + lr kept, clipped + lr up
DESIRED_KL, MAX_NORM, BETA1, BETA2, EPS = float(F32(0.01)), 1.0, 0.9, 0.999, 1e-8


def adam_restated(params, ms, vs, grads, lr, kl, step, dt):
    """one step: the learning-rate decision of ppo.py:140-151, clip_grad_norm_ over all tensors, torch.optim.Adam (no weight decay, no amsgrad)"""
    lr = dt(lr)
    if kl is not None:
        if dt(kl) > dt(DESIRED_KL) * dt(2.0):
            lr = max(dt(1e-5), lr / dt(1.5))
        elif dt(kl) < dt(DESIRED_KL) / dt(2.0) and kl > 0.0:
            lr = min(dt(1e-2), lr * dt(1.5))
    norm = np.sqrt(seqsum(np.concatenate([g.astype(dt) ** 2 for g in grads]), dt))
    coef = min(dt(MAX_NORM) / (norm + dt(1e-6)), dt(1.0))
    b2 = dt(BETA2)
    bc1, bc2 = dt(1.0 - BETA1 ** step), dt(1.0 - BETA2 ** step)
    out = []
    for p, m, v, g in zip(params, ms, vs, grads):
        g = g.astype(dt) * coef
        m = m + (g - m) * dt(1.0 - BETA1)
        v = b2 * v + dt(1.0 - BETA2) * g * g
        out.append((p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + dt(EPS)), m, v))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], lr


def _adam_struct(lib, bufs, steps, numels):
    t = lib.abi.AdamTensors()
    fp = C.POINTER(lib.abi.real)
    t.count = len(numels)
    for i, n in enumerate(numels[:lib.abi.GO2_ADAM_MAX_TENSORS]):
        t.numel[i] = n
        for name, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), bufs[i]):
            getattr(t, name)[i] = C.cast(b.ptr, fp)
        t.step[i] = C.cast(steps[i].ptr, fp)
    return t


def _adam_run(lib, device, tensors, steps_spec, seed, compare):
    rng = np.random.default_rng(seed)
    numels = [n for n, _ in tensors]
    p0 = [(0.1 * rng.normal(size=n)).astype(F32) for n in numels]
    grads = [[(s * 1e-2 * rng.normal(size=n)).astype(F32) for n in numels] for s, _ in steps_spec]
    bufs = [[Buf(device, n, init, front=off) for init, off in zip((p0[i], 0.0, 0.0, 0.0), offs)] for i, (n, offs) in enumerate(tensors)]
    steps = [Buf(device, 1, 0.0) for _ in numels]
    t = _adam_struct(lib, bufs, steps, numels)
    nws = lib.go2sim_adam_workspace_len(C.byref(t))
    assert nws == sum((n + lib.abi.GO2_ADAM_CHUNK - 1) // lib.abi.GO2_ADAM_CHUNK for n in numels)
    ws, lr = Buf(device, nws, float("nan")), Buf(device, 1, 1e-3)
    state = {dt: ([x.astype(dt) for x in p0], [np.zeros(n, dt) for n in numels], [np.zeros(n, dt) for n in numels], dt(F32(1e-3))) for dt in (F64, F32)}
    trace = []
    for it, (_, kl) in enumerate(steps_spec):
        for i in range(len(numels)):
            bufs[i][1].t[bufs[i][1].front:bufs[i][1].front + numels[i]] = dev_in(grads[it][i], device)
        klt = dev_in(np.array([kl], F32), device) if kl is not None else None
        rc = lib.go2sim_adam_clip_step(C.byref(t), lr.ptr, P(klt), DESIRED_KL, MAX_NORM, BETA1, BETA2, EPS, ws.ptr, stream_of(device))
        assert rc == 0, lib.go2sim_last_error()
        sync(device)
        got = [[b.get() for b in (bufs[i][0], bufs[i][2], bufs[i][3])] for i in range(len(numels))]
        trace.append((got, lr.get().copy()))
        for dt in (F64, F32):
            state[dt] = adam_restated(*state[dt][:3], grads[it], state[dt][3], kl, it + 1, dt)
        if compare:
            for i, n in enumerate(numels):
                for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
                    within("adam step %d tensor %d numel=%d offsets=%s %s" % (it + 1, i, n, tensors[i][1], name), got[i][k], state[F32][k][i], state[F64][k][i])
            within("adam step %d lr" % (it + 1), lr.get(), [state[F32][3]], [state[F64][3]])
        assert all(float(s.get()[0]) == it + 1 and s.intact() for s in steps)
        assert all(b.intact() for row in bufs for b in row) and ws.intact() and lr.intact()
        assert all(np.array_equal(bufs[i][1].get(), grads[it][i]) for i in range(len(numels)))          # the gradients are read, not scaled in place
    return trace, t, bufs, steps, lr, ws


def check_adam(lib, device):
    a = _adam_run(lib, device, ADAM_TENSORS, ADAM_STEPS, 11, True)[0]
    b = _adam_run(lib, device, ADAM_TENSORS, ADAM_STEPS, 11, False)[0]          # a fixed summation order: bit-equal from run to run
    for (ga, la), (gb, lb) in zip(a, b):
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ra, rb in zip(ga, gb) for x, y in zip(ra, rb))


def check_adam_limits(lib, device):
    """count = GO2_ADAM_MAX_TENSORS is served; one tensor more, or an empty tensor, is refused and nothing is written"""
    M = lib.abi.GO2_ADAM_MAX_TENSORS
    _, t, bufs, steps, lr, ws = _adam_run(lib, device, [(7, (4, 4, 4, 4))] * M, ADAM_STEPS[:1], 13, True)
    before = [[b.t.clone() for b in row] for row in bufs]
    for bad in ("count", "numel"):
        if bad == "count":
            t.count = M + 1
        else:
            t.count, t.numel[M // 2] = M, 0
        assert lib.go2sim_adam_workspace_len(C.byref(t)) < 0
        assert lib.go2sim_adam_clip_step(C.byref(t), lr.ptr, None, DESIRED_KL, MAX_NORM, BETA1, BETA2, EPS, ws.ptr, stream_of(device)) < 0
        sync(device)
        assert all(torch.equal(b.t, c) for row, crow in zip(bufs, before) for b, c in zip(row, crow)) and all(float(s.get()[0]) == 1.0 for s in steps)


@pytest.mark.parametrize("which", WHICH)
def test_adam_clip_step(which):
    check_adam(host_lib(which), "cpu")


@pytest.mark.parametrize("which", WHICH)
def test_adam_limits(which):
    check_adam_limits(host_lib(which), "cpu")
