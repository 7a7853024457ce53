"""The update's diagnostics on the CPU (`algorithm.diagnostics`): go2nn_ppo_diag and go2nn_grad_sqnorm (host build) against float64 with the torch fp32 statement as the
yardstick of the error, their bit repeatability and refusals, the slot cursor, training being bit for bit untouched, the figures meaning what they say, graph mode
against the eager mode per slot, the new refusals and the way from the command line to the TensorBoard tags.  tests/test_gpu_update_diag.py runs the kernels' cases on
the device."""
import copy
import ctypes as C
import math
import re
import os

import numpy as np
import pytest
import torch

from helpers import load_nn_emu, load_oracle
from test_cts_own import make_cts
from test_symmetry_host import _ppo, fill_storage
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd.rsl_rl.algorithms import _diag

GO2NN_EINVAL = -22
NUM = _nn.GO2NN_DIAG_NUM
COL = _diag.COL
COUNT_COLS = ("rows", "ratio_clipped", "adv_pos", "value_clipped")
CLIP = 0.2
MARGIN = 1e-3
SENT = -7.25


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


def pass_rows(lib):
    """T, the pass's rows per workgroup: the largest B that go2nn_ppo_diag_rows answers with one partial row"""
    T = 1
    while lib.go2nn_ppo_diag_rows(T + 1, 12, 128) == 1:
        T += 1
    assert lib.go2nn_ppo_diag_rows(T, 12, 128) == 1 and lib.go2nn_ppo_diag_rows(T + 1, 12, 128) == 2
    return T


def shapes(lib):
    """(B, A, K, split): one row, two rows split, one row short of a workgroup, a full one with the largest head and the split at its last row, one row more, two
    workgroups and a ragged third with the split just inside the second, several workgroups with the CTS proportions"""
    T = pass_rows(lib)
    return [(1, 1, 4, 0), (2, 12, 128, 1), (T - 1, 12, 128, 0), (T, 16, 256, T - 1), (T + 1, 12, 128, 1), (2 * T + 3, 12, 64, T + 1), (384, 12, 128, 288)]


# ---- the cases and their references --------------------------------------------------------------------------------------------------------------------------
def _draw_rows(c, rng, rows):
    """the per-row inputs of `rows`: old policy near the new one (ratios on both sides of 1 +- clip), old values near the values"""
    n, A = len(rows), c["A"]
    y_a, y_c = c["y_a"][rows].astype(np.float64), c["y_c"][rows].astype(np.float64)
    mu = y_a @ c["w_mu"].astype(np.float64).T + c["b_mu"]
    v = y_c @ c["w_v"].astype(np.float64).reshape(-1) + c["b_v"][0]
    std = c["std"].astype(np.float64)
    old_mu = (mu + 0.1 * rng.normal(size=(n, A))).astype(np.float32)
    old_sigma = (std * (1.0 + 0.05 * rng.normal(size=(n, A)))).astype(np.float32)
    actions = (old_mu + old_sigma * rng.normal(size=(n, A))).astype(np.float32)
    z = (actions.astype(np.float64) - old_mu) / old_sigma
    c["old_mu"][rows], c["old_sigma"][rows], c["actions"][rows] = old_mu, old_sigma, actions
    c["old_logp"][rows] = (-0.5 * z * z - np.log(old_sigma.astype(np.float64)) - 0.5 * math.log(2.0 * math.pi)).sum(-1).astype(np.float32)
    c["adv"][rows] = rng.normal(size=n).astype(np.float32)
    c["old_values"][rows] = (v + 0.3 * rng.normal(size=n)).astype(np.float32)
    c["returns"][rows] = (c["old_values"][rows] + 0.5 * rng.normal(size=n)).astype(np.float32)


def terms_and_magnitudes64(mu, v, std, act, omu, osg, olp, adv, tv, ret, clip):
    """float64 numpy from mu [B, A] and v [B]: the rows' terms [B, 18] in the enum's order (the issue's section 2), and per term the MAGNITUDE its fp32 evaluation's
    rounding error scales with — the size of the fp32 operands of the operation that forms it, not of its result, which may be what a cancellation leaves:
      lr = lp - old_logp: max(|lp|, |old_logp|, 1);  rho = exp(lr): rho x that (an absolute error of lr is a relative one of rho);  (rho - 1) - lr: both;
      kl: the sum of its addends' absolute values;  err = returns - v: max(|returns|, |v|), its square that squared;  adv, returns and their squares: themselves.
    -> (terms, magnitudes, dict of the rows' rho / dv / adv)"""
    lp = (-(act - mu) ** 2 / (2.0 * std ** 2) - np.log(std) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    kl_a, kl_b = np.log(std / osg + 1.0e-5), (osg ** 2 + (omu - mu) ** 2) / (2.0 * std ** 2)
    kl = (kl_a + kl_b - 0.5).sum(-1)
    lr = lp - olp
    rho, err, dv = np.exp(lr), ret - v, v - tv
    one = np.ones_like(lr)
    terms = np.stack([one, (np.abs(rho - 1.0) > clip) * 1.0, rho, lr, (rho - 1.0) - lr, kl, kl, adv, adv ** 2, (adv > 0) * 1.0, err, err ** 2, np.abs(err), ret, ret ** 2,
                      (np.abs(dv) > clip) * 1.0, rho, rho], axis=1)
    m_lr = np.maximum(np.maximum(np.abs(lp), np.abs(olp)), 1.0)
    m_rho, m_kl, m_err = rho * m_lr, (np.abs(kl_a) + kl_b + 0.5).sum(-1), np.maximum(np.abs(ret), np.abs(v))
    mags = np.stack([one, one, m_rho, m_lr, m_rho + m_lr, m_kl, m_kl, np.abs(adv), adv ** 2, one, m_err, m_err ** 2, m_err, np.abs(ret), ret ** 2, one, m_rho, m_rho], axis=1)
    return terms, mags, dict(rho=rho, dv=dv, adv=adv)


def pool_magnitudes(terms, mags):
    """[rows, 18] x 2 -> [18]: a sum column's magnitude is the sum of its rows' magnitudes, an extremum's that of the row that holds the extremum"""
    pick = np.where(_diag._KIND == 2, terms.argmin(0), terms.argmax(0))
    return np.where(_diag._KIND == 0, mags.sum(0), mags[pick, np.arange(NUM)])


def row_terms64(c):
    """the case in float64: mu and v as float64 products of the fp32 inputs -> terms_and_magnitudes64's result"""
    f = lambda k: c[k].astype(np.float64)
    mu = f("y_a") @ f("w_mu").T + f("b_mu")
    v = f("y_c") @ f("w_v").reshape(-1) + f("b_v")[0]
    return terms_and_magnitudes64(mu, v, f("std"), f("actions"), f("old_mu"), f("old_sigma"), f("old_logp"), f("adv"), f("old_values"), f("returns"), c["clip"])


def make_case(B, A, K, split, seed=0):
    rng = np.random.default_rng(seed + 1000003 * B + 1009 * A + K)
    elu = lambda z: np.where(z > 0, z, np.expm1(z)).astype(np.float32)
    c = dict(B=B, A=A, K=K, split=split, clip=CLIP, y_a=elu(rng.normal(size=(B, K))), y_c=elu(rng.normal(size=(B, K))),
             w_mu=(rng.normal(size=(A, K)) / math.sqrt(K)).astype(np.float32), b_mu=rng.normal(0.0, 0.3, A).astype(np.float32),
             w_v=(rng.normal(size=(1, K)) / math.sqrt(K)).astype(np.float32), b_v=rng.normal(0.0, 0.3, 1).astype(np.float32),
             std=rng.uniform(0.4, 1.0, A).astype(np.float32))
    for k, w in (("old_mu", A), ("old_sigma", A), ("actions", A)):
        c[k] = np.zeros((B, w), np.float32)
    for k in ("old_logp", "adv", "old_values", "returns"):
        c[k] = np.zeros(B, np.float32)
    _draw_rows(c, rng, np.arange(B))
    for _ in range(200):          # redraw the rows whose float64 ratio or value step sits within MARGIN of a count's threshold, until none is left
        bad = np.nonzero(~_clear_of_thresholds(c))[0]
        if len(bad) == 0:
            break
        _draw_rows(c, rng, bad)
    assert _clear_of_thresholds(c).all()          # the cap on excluded rows is zero
    return c


def _clear_of_thresholds(c):
    t = row_terms64(c)[2]
    return (np.abs(np.abs(t["rho"] - 1.0) - c["clip"]) >= MARGIN) & (np.abs(np.abs(t["dv"]) - c["clip"]) >= MARGIN) & (np.abs(t["adv"]) > 0)


def segments_of(c):
    return [(0, c["B"])] if c["split"] <= 0 else [(0, c["split"]), (c["split"], c["B"])]


def reference64(c):
    """-> (table [segments, 18], magnitude [segments, 18]) in float64"""
    terms, mags, _ = row_terms64(c)
    return np.stack([_diag.pool_rows(terms[a:b]) for a, b in segments_of(c)]), np.stack([pool_magnitudes(terms[a:b], mags[a:b]) for a, b in segments_of(c)])


def torch32(c, dev="cpu"):
    """the torch fp32 statement (algorithms/_diag.py:diag_rows_torch, what every formulation that holds mu and value as tensors runs) -> [segments, 18] float64"""
    t = lambda k: torch.from_numpy(c[k]).to(dev)
    mu, v = torch.addmm(t("b_mu"), t("y_a"), t("w_mu").t()), torch.addmm(t("b_v"), t("y_c"), t("w_v").t())
    return _diag.diag_rows_torch(mu, t("std"), v, t("actions"), t("old_mu"), t("old_sigma"), t("old_logp"), t("adv"), t("old_values"), t("returns"), c["clip"],
                                 c["split"]).cpu().numpy()


class DiagCall:
    """the device (or host) buffers of a case and go2nn_ppo_diag calls on them; partials and table carry SENT-filled tails so that a write past the end shows"""
    KEYS = ("y_a", "y_c", "w_mu", "b_mu", "w_v", "b_v", "std", "actions", "old_mu", "old_sigma", "old_logp", "adv", "old_values", "returns")

    def __init__(self, lib, c, dev="cpu", slots=3):
        self.lib, self.c, self.dev, self.slots = lib, c, dev, slots
        self.t = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in self.KEYS}          # (copies: a later copy_ into them leaves the case alone)
        self.segs = 2 if c["split"] > 0 else 1
        self.rows = lib.go2nn_ppo_diag_rows(c["B"], c["A"], c["K"])
        assert self.rows == (c["B"] + pass_rows(lib) - 1) // pass_rows(lib), lib.go2nn_last_error()
        self.partials = torch.full((self.rows * self.segs * NUM + 8,), SENT, dtype=torch.float64, device=dev)
        self.table = torch.full(((slots + 1) * self.segs * NUM,), SENT, dtype=torch.float64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)

    def struct(self):
        c = self.c
        return _nn.Go2nnPpoDiag(*[self.t[k].data_ptr() for k in self.KEYS], self.partials.data_ptr(), self.table.data_ptr(), self.cursor.data_ptr(), c["B"], c["A"], c["K"],
                                c["split"], self.slots, c["clip"])

    def __call__(self, patch=None, stream=None, null_struct=False):
        d = self.struct()
        if patch:
            patch(d)
        return self.lib.go2nn_ppo_diag(None if null_struct else C.byref(d), stream)

    def slot(self, i):
        n = self.segs * NUM
        return self.table[i * n:(i + 1) * n].cpu().numpy().reshape(self.segs, NUM)

    def bits(self):
        return self.partials.cpu().numpy().tobytes() + self.table.cpu().numpy().tobytes() + self.cursor.cpu().numpy().tobytes()


def check_against_float64(got, c, what, dev="cpu"):
    """the rule of the kernel-vs-float64 test: counts exact; every other column at most 4 x as far from float64 as the torch fp32 statement is on the same inputs (a
    different summation order of equal arithmetic), plus 1e-6 x the column's magnitude.  Prints both gaps."""
    ref, mag = reference64(c)
    t32 = torch32(c, dev)
    assert got.shape == ref.shape == t32.shape
    for s in range(ref.shape[0]):
        for k in COUNT_COLS:
            assert got[s, COL[k]] == ref[s, COL[k]], (what, s, k, got[s, COL[k]], ref[s, COL[k]])
        for k, j in COL.items():
            if k in COUNT_COLS:
                continue
            gk, gt = abs(got[s, j] - ref[s, j]), abs(t32[s, j] - ref[s, j])
            print("[update diag, %s] segment %d %-14s float64 % .9e: kernel gap %.2e, torch fp32 gap %.2e, floor %.2e" % (what, s, k, ref[s, j], gk, gt, 1e-6 * mag[s, j]))
            assert np.isfinite(got[s, j]) and gk <= 4.0 * gt + 1e-6 * mag[s, j], (what, s, k, got[s, j], ref[s, j], gk, gt, mag[s, j])


# ---- 1. the kernel against float64 ---------------------------------------------------------------------------------------------------------------------------
def test_enum_of_the_header_is_the_binding_s_column_order():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = re.findall(r"^\s*GO2NN_DIAG_([A-Z0-9_]+)\b", open(os.path.join(root, "include", "go2nn.h")).read(), re.M)
    assert names[-1] == "NUM" and tuple(n.lower() for n in names[:-1]) == _nn.DIAG_COLS and NUM == 18
    assert [k for k, kind in zip(_nn.DIAG_COLS, _diag._KIND) if kind == 1] == list(_nn.DIAG_MAX_COLS) and [k for k, kind in zip(_nn.DIAG_COLS, _diag._KIND) if kind == 2] == ["ratio_min"]


@pytest.mark.parametrize("i", range(7))
def test_kernel_matches_float64(emu, i):
    B, A, K, split = shapes(emu)[i]
    c = make_case(B, A, K, split)
    t = row_terms64(c)[2]
    if B >= 40:          # the counts are not trivial: rows on both sides of every threshold
        for m in (np.abs(t["rho"] - 1.0) > CLIP, np.abs(t["dv"]) > CLIP, t["adv"] > 0):
            assert 0 < m.sum() < B
    call = DiagCall(emu, c)
    assert call() == 0, emu.go2nn_last_error()
    assert int(call.cursor[0]) == 1 and (call.partials[-8:] == SENT).all() and (call.table[call.segs * NUM:] == SENT).all()
    check_against_float64(call.slot(0), c, "host build, B %d A %d K %d split %d" % (B, A, K, split))


# ---- 2. bit repeatability; nothing the heads wrote is touched --------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_heads_outputs_stay(emu):
    B, A, K, split = shapes(emu)[6]
    c = make_case(B, A, K, split)
    a, b = DiagCall(emu, c), DiagCall(emu, c)
    rows, cols = emu.go2nn_ppo_heads_rows(B, A, K), emu.go2nn_ppo_heads_cols(A, K)
    gz_a, gz_c, part = torch.full((B, K), 3.5), torch.full((B, K), -1.25), torch.full((rows * cols,), 9.0)
    h = _nn.Go2nnPpoHeads(*[a.t[k].data_ptr() for k in DiagCall.KEYS], gz_a.data_ptr(), gz_c.data_ptr(), part.data_ptr(), B, A, K, 1, CLIP, 1.0, 0.01, split)
    assert emu.go2nn_ppo_heads(C.byref(h), None) == 0          # (the pattern: what the heads leave)
    before = gz_a.numpy().tobytes() + gz_c.numpy().tobytes() + part.numpy().tobytes()
    inputs = b"".join(a.t[k].numpy().tobytes() for k in DiagCall.KEYS)
    assert a() == 0 and b() == 0
    assert a.bits() == b.bits()
    assert before == gz_a.numpy().tobytes() + gz_c.numpy().tobytes() + part.numpy().tobytes()
    assert inputs == b"".join(a.t[k].numpy().tobytes() for k in DiagCall.KEYS)


# ---- 3. go2nn_grad_sqnorm ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 4095, 4096, 4097, 131073)


def grad_case(count, seed=0):
    """`count` tensors of the sizes above in turn, magnitudes over several decades"""
    rng = np.random.default_rng(seed + count)
    return [(rng.normal(size=SIZES[i % len(SIZES)]) * np.exp(rng.normal(0, 2))).astype(np.float32) for i in range(count)]


def run_grad_sqnorm(lib, arrays, dev="cpu", slots=2, stream=None):
    ts = [torch.from_numpy(a).to(dev) for a in arrays]
    ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    numel = (C.c_int32 * len(ts))(*[t.numel() for t in ts])
    rows = lib.go2nn_grad_sqnorm_rows(numel, len(ts))
    assert rows == sum((t.numel() + 4095) // 4096 for t in ts), lib.go2nn_last_error()
    part = torch.full((rows + 8,), SENT, dtype=torch.float64, device=dev)
    out = torch.full((slots + 1,), SENT, dtype=torch.float64, device=dev)
    cur = torch.zeros(1, dtype=torch.int32, device=dev)
    rcs = [lib.go2nn_grad_sqnorm(ptrs, numel, len(ts), part.data_ptr(), out.data_ptr(), cur.data_ptr(), slots, stream) for _ in range(2)]
    if dev != "cpu":
        torch.cuda.synchronize()
    return rcs, out.cpu().numpy(), part.cpu().numpy(), int(cur.cpu()[0]), ts


@pytest.mark.parametrize("count", [1, 3, 48])
def test_grad_sqnorm_matches_float64(emu, count):
    """Exact squares and at most ~6e5 fp64 additions: N 2^-53 ~ 7e-11 relative, so 1e-9 holds with room; the second call writes the same bits into the next slot"""
    arrays = grad_case(count)
    rcs, out, part, cur, _ = run_grad_sqnorm(emu, arrays)
    want = sum(float((a.astype(np.float64) ** 2).sum()) for a in arrays)
    print("[update diag, grad sqnorm, host build] %d tensors: %.15e against float64 %.15e (relative gap %.2e)" % (count, out[0], want, abs(out[0] - want) / want))
    assert rcs == [0, 0] and cur == 2 and abs(out[0] - want) <= 1e-9 * want
    assert out[0].tobytes() == out[1].tobytes() and out[2] == SENT and (part[-8:] == SENT).all()


def test_grad_sqnorm_refuses(emu):
    arrays = grad_case(3)
    ts = [torch.from_numpy(a) for a in arrays]
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    numel = (C.c_int32 * 3)(*[t.numel() for t in ts])
    bad_numel = (C.c_int32 * 3)(ts[0].numel(), 0, ts[2].numel())
    huge_numel = (C.c_int32 * 3)(ts[0].numel(), 2 ** 31 - 4096, ts[2].numel())          # (its last chunk's int index would pass INT32_MAX; refused before anything is read)
    many = (C.c_void_p * 49)(*([ts[0].data_ptr()] * 49))
    many_n = (C.c_int32 * 49)(*([1] * 49))
    part, out, cur = torch.full((64,), SENT, dtype=torch.float64), torch.full((3,), SENT, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    p, o, c = part.data_ptr(), out.data_ptr(), cur.data_ptr()
    calls = [(None, numel, 3, p, o, c, 2), (ptrs, None, 3, p, o, c, 2), (ptrs, numel, 3, None, o, c, 2), (ptrs, numel, 3, p, None, c, 2), (ptrs, numel, 3, p, o, None, 2),
             (ptrs, numel, 0, p, o, c, 2), (many, many_n, 49, p, o, c, 2), (ptrs, bad_numel, 3, p, o, c, 2), (ptrs, huge_numel, 3, p, o, c, 2), (ptrs, numel, 3, p, o, c, 0)]
    for args in calls:
        assert emu.go2nn_grad_sqnorm(*args, None) == GO2NN_EINVAL and emu.go2nn_last_error(), args
    assert emu.go2nn_grad_sqnorm_rows(bad_numel, 3) == GO2NN_EINVAL and emu.go2nn_grad_sqnorm_rows(huge_numel, 3) == GO2NN_EINVAL and emu.go2nn_grad_sqnorm_rows(many_n, 49) == GO2NN_EINVAL
    assert (part == SENT).all() and (out == SENT).all() and int(cur[0]) == 0
    # a full cursor: nothing is written, the cursor stays
    cur[0] = 2
    assert emu.go2nn_grad_sqnorm(ptrs, numel, 3, p, o, c, 2, None) == 0 and (out == SENT).all() and int(cur[0]) == 2


# ---- 4. the cursor and the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_cursor_fills_the_slots_in_turn_and_refuses_past_the_last(emu):
    B, A, K, split = shapes(emu)[5]
    cases = [make_case(B, A, K, split, seed=s) for s in range(3)]
    call = DiagCall(emu, cases[0], slots=3)
    for i, c in enumerate(cases):
        for k in DiagCall.KEYS:
            call.t[k].copy_(torch.from_numpy(c[k]))
        assert call() == 0 and int(call.cursor[0]) == i + 1
    for i, c in enumerate(cases):
        ref, _ = reference64(c)
        assert np.array_equal(call.slot(i)[:, COL["rows"]], ref[:, COL["rows"]]) and np.allclose(call.slot(i), ref, rtol=1e-4, atol=1e-4)
    assert not np.array_equal(call.slot(0), call.slot(1))
    before = call.table.numpy().tobytes()
    assert call() == 0          # slot 3 of 3: the launch is accepted (the slot is a device-side value), the kernel writes nothing and the cursor stays
    assert call.table.numpy().tobytes() == before and int(call.cursor[0]) == 3 and (call.slot(3) == SENT).all()
    call.cursor[0] = -1
    assert call() == 0 and call.table.numpy().tobytes() == before and int(call.cursor[0]) == -1


def test_every_refusal_writes_nothing(emu):
    B, A, K, split = shapes(emu)[4]
    c = make_case(B, A, K, split)
    call = DiagCall(emu, c)
    clean = call.bits()

    def setter(**kw):
        def patch(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return patch
    patches = [setter(**{k: None}) for k in DiagCall.KEYS + ("partials", "table", "cursor")]
    patches += [setter(B=0), setter(B=-3), setter(A=0), setter(A=17), setter(K=0), setter(K=2), setter(K=126), setter(K=260), setter(surrogate_split=-1),
                setter(surrogate_split=B), setter(slots=0), setter(slots=-1)]
    for patch in patches:
        assert call(patch=patch) == GO2NN_EINVAL and emu.go2nn_last_error()
        assert call.bits() == clean
    assert call(null_struct=True) == GO2NN_EINVAL and call.bits() == clean
    for bad in ((0, 12, 128), (5, 0, 128), (5, 17, 128), (5, 12, 130), (5, 12, 0), (5, 12, 260)):
        assert emu.go2nn_ppo_diag_rows(*bad) == GO2NN_EINVAL
    assert call() == 0 and call.bits() != clean


# ---- 5. training is untouched -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_pair():
    """the go2sim oracle and the go2nn host build as the library pair of modules/fused.py: the no-autograd mini-batches run on the CPU"""
    from go2_rl_gym_amd.rsl_rl.modules import fused
    was = (fused._LIB, fused._NN)
    lib = load_nn_emu()
    fused.set_library(load_oracle())
    fused.set_nn_library(lib)
    yield lib
    fused._LIB, fused._NN = was


def _optimizers(alg):
    return [alg.optimizer] if hasattr(alg, "optimizer") else [alg.optimizer1, alg.optimizer2]


def training_state(alg, out):
    """every parameter, every Adam moment and step, the returned losses and the learning rate, as bytes"""
    b = b"".join(p.detach().numpy().tobytes() for p in alg.actor_critic.parameters()) + np.asarray(out, np.float64).tobytes() + np.float64(alg.learning_rate).tobytes()
    for o in _optimizers(alg):
        for g in o.param_groups:
            for p in g["params"]:
                st = o.state[p]
                b += st["exp_avg"].numpy().tobytes() + st["exp_avg_sq"].numpy().tobytes() + np.float64(float(st["step"])).tobytes()
    return b


def fill_cts_storage(alg, seed, scale=0.3):
    st = alg.storage
    g = torch.Generator().manual_seed(seed)
    r = lambda t, s=1.0: torch.randn(t.shape, generator=g) * s
    for k in ("observations", "privileged_observations", "history"):
        getattr(st, k).copy_(r(getattr(st, k)))
    st.mu.copy_(r(st.mu, 0.5))
    st.sigma.copy_(0.6 + 0.4 * torch.rand(st.sigma.shape, generator=g))
    st.actions.copy_(st.mu + st.sigma * r(st.actions))
    st.actions_log_prob.copy_(torch.distributions.Normal(st.mu, st.sigma).log_prob(st.actions).sum(-1, keepdim=True))
    for k in ("values", "returns", "advantages"):
        getattr(st, k).copy_(r(getattr(st, k), scale))
    st.step = st.num_transitions_per_env


GRAPH = dict(use_graphs="uncaptured", fused_loss=True)          # the graph-mode update, run uncaptured on the host builds


def make_alg(kind, lib, **kw):
    """PPO (the small networks of tests/test_symmetry_host.py) or CTS / MoECTS (those of tests/test_cts_own.py) on 8 envs x 6 steps, 2 epochs x 2 mini-batches, a filled storage"""
    if kind == "PPO":
        alg = _ppo(**kw)
        alg.nn_lib = lib
        fill_storage(alg, 10, scale=0.3)
        return alg
    if kw.get("use_graphs"):
        kw = dict(kw, lib=load_oracle())
    _, alg = make_cts("cpu", kind, num_learning_epochs=2, num_mini_batches=2, **dict(dict(schedule="adaptive"), **kw))
    alg.nn_lib = lib
    alg.init_storage(8, 6, [45], [60], [12])
    fill_cts_storage(alg, 3)
    return alg


@pytest.mark.parametrize("mode", ["eager", "graph", "graph_autograd"])
@pytest.mark.parametrize("kind", ["PPO", "CTS", "MoECTS"])
def test_training_is_bit_identical_with_the_key_on(host_pair, kind, mode):
    kw = {} if mode == "eager" else (GRAPH if mode == "graph" else dict(GRAPH, fused_loss=False))
    states = []
    for key in (False, True):
        alg = make_alg(kind, host_pair, diagnostics=key, **kw)
        torch.manual_seed(20)
        states.append(training_state(alg, alg.update()))
        if key:
            assert alg.diagnostics and alg.diagnostics_table.shape == (4, 1 if kind == "PPO" else 2, NUM) and alg.diagnostics_grad_sq.shape == (4, 1 if kind == "PPO" else 2)
            assert np.isfinite(alg.diagnostics_table).all() and (alg.diagnostics_grad_sq > 0).all()
            if mode == "graph":          # the mini-batch without autograd: the kernel filled the table (its partial rows exist), not the torch statement
                assert alg._diag._partials is not None and all(p is not None for p in alg._diag._gpart)
        else:
            assert alg.diagnostics is None and alg.diagnostics_table is None and alg.diagnostics_grad_sq is None and alg._diag is None
    assert states[0] == states[1]


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("kind", ["MoENGCTS", "ACMoECTS", "DualMoECTS"])
def test_other_cts_variants_take_the_torch_statement(kind, mode, tmp_path, monkeypatch):
    """The three CTS variants next to CTS / MoE-CTS do not refuse: one learn() iteration on the scripted env of tests/test_cts_golden.py, in the eager mode and in graph
    mode run uncaptured on the host builds, with the key off and on — weights, Adam moments and returned losses bit-identical, both segments' rows filled and finite,
    the Diag tags written.  (AC-MoE and Dual-MoE keep the autograd step in graph mode; MoE-NG takes the no-autograd policy step, i.e. the kernel.)"""
    from go2_rl_gym_amd.rsl_rl.modules import fused as fmod
    from go2_rl_gym_amd.rsl_rl.runners import OnPolicyRunnerCTS
    from helpers import ROOT
    from test_cts_golden import ScriptedEnv, _train_cfg
    fixture = {"MoENGCTS": "moe_ng_cts_iteration.npz", "ACMoECTS": "ac_moe_cts_iteration.npz", "DualMoECTS": "dual_moe_cts_iteration.npz"}[kind]
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", fixture)))
    T = g["rew"].shape[0]
    if mode == "graph":
        monkeypatch.setattr(fmod, "_LIB", load_oracle()); monkeypatch.setattr(fmod, "_NN", load_nn_emu())
    states = []
    for key in (False, True):
        cfg = _train_cfg(kind, T)
        if key:
            cfg["algorithm"]["diagnostics"] = True
        os.makedirs(tmp_path / str(key))
        torch.manual_seed(11)
        runner = OnPolicyRunnerCTS(ScriptedEnv(g, load_oracle()), cfg, log_dir=str(tmp_path / str(key)), device="cpu", use_graphs="uncaptured" if mode == "graph" else None)
        alg = runner.alg
        if mode == "graph":
            alg.fused_loss = alg.fused_rollout = True
            alg.nn_lib = load_nn_emu()
        runner.writer = Scalars()
        runner.learn(1, init_at_random_ep_len=False)
        losses = [v for t, v in runner.writer.rows if t.startswith("Loss/")]
        states.append(training_state(alg, losses))
        if key:
            tab = alg.diagnostics_table
            assert tab.shape == (4, 2, NUM) and np.isfinite(tab).all() and (tab[..., COL["rows"]] > 0).all() and (alg.diagnostics_grad_sq > 0).all()
            assert set(alg.diagnostics) == {"teacher", "student", "all"} and any(t == "Diag/all/clip_fraction" for t, _ in runner.writer.rows)
            if mode == "graph":
                assert (alg._diag._partials is not None) == (kind == "MoENGCTS")
        else:
            assert alg.diagnostics is None
    assert states[0] == states[1]


def test_the_key_defaults_to_off():
    assert _ppo()._diag is None and make_cts("cpu")[1]._diag is None


# ---- 6. the figures mean what they say (eager, CPU) ------------------------------------------------------------------------------------------------------------
def coherent_rollout(alg, seed):
    """a storage whose old policy IS the current one: mu, sigma, log-prob and values of the stored rows computed by the algorithm's own networks"""
    fill_storage(alg, seed, scale=0.3)
    st, ac = alg.storage, alg.actor_critic
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        obs, cobs = st.observations.flatten(0, 1), st.privileged_observations.flatten(0, 1)
        mu, sigma = ac.actor(obs), ac.std.expand(obs.shape[0], -1)
        act = mu + sigma * torch.randn(mu.shape, generator=g)
        shape = st.mu.shape
        st.mu.copy_(mu.view(shape)); st.sigma.copy_(sigma.reshape(shape)); st.actions.copy_(act.view(shape))
        st.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1).view(st.actions_log_prob.shape))
        st.values.copy_(ac.critic(cobs).view(st.values.shape))


def test_step_0_reads_the_rollouts_own_policy():
    alg = _ppo(diagnostics=True, schedule="fixed")
    coherent_rollout(alg, 4)
    alg.update()
    d, tab = alg.diagnostics, alg.diagnostics_table
    step0 = _diag.figures(tab[0, 0])
    print("[update diag] step 0: ratio in [%.8f, %.8f], approx_kl %.2e, clip fraction %g; last step: approx_kl %.2e" % (step0["ratio_min"], step0["ratio_max"], step0["approx_kl"],
                                                                                                                    step0["clip_fraction"], _diag.figures(tab[-1, 0])["approx_kl"]))
    assert abs(step0["ratio_max"] - 1.0) <= 1e-5 and abs(step0["ratio_min"] - 1.0) <= 1e-5 and step0["clip_fraction"] == 0 and abs(step0["approx_kl"]) < 1e-8
    assert abs(step0["kl"] - 12 * math.log1p(1e-5)) < 1e-5          # (the heads' expression carries a 1e-5 inside its logarithm: 12 actions x log(1 + 1e-5))
    # the policy has moved by the last step, and the epochs' keys are the pooled rows of their steps
    assert _diag.figures(tab[-1, 0])["approx_kl"] > 1e-7
    assert d["approx_kl/first_epoch"] == _diag.figures(_diag.pool_rows(tab[:2]))["approx_kl"] and d["approx_kl/last_epoch"] == _diag.figures(_diag.pool_rows(tab[2:]))["approx_kl"]
    assert set(k for k in d if "/" not in k) == {"clip_fraction", "approx_kl", "approx_kl_k1", "kl", "kl_max", "ratio_mean", "ratio_max", "ratio_min", "explained_variance",
                                                 "value_err_max", "value_clip_fraction", "adv_mean", "adv_std", "adv_pos_share", "grad_norm", "grad_norm_max", "grad_clipped_share"}
    assert all(k + sfx in d for k in ("clip_fraction", "grad_norm") for sfx in ("/first_epoch", "/last_epoch"))


def test_learning_rate_zero_keeps_every_step_at_step_0():
    alg = _ppo(diagnostics=True, schedule="fixed", learning_rate=0.0)
    coherent_rollout(alg, 5)
    alg.update()
    for row in alg.diagnostics_table[:, 0]:
        f = _diag.figures(row)
        assert abs(f["ratio_max"] - 1.0) <= 1e-5 and abs(f["ratio_min"] - 1.0) <= 1e-5 and f["clip_fraction"] == 0 and abs(f["approx_kl"]) < 1e-8


def test_grad_norm_is_what_the_clip_saw(monkeypatch):
    seen = []
    real = torch.nn.utils.clip_grad_norm_

    def spy(params, max_norm, *a, **k):
        out = real(params, max_norm, *a, **k)
        seen.append(float(out))
        return out
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    alg = _ppo(diagnostics=True, max_grad_norm=0.55)
    fill_storage(alg, 10, scale=0.3)
    alg.update()
    norms = np.sqrt(alg.diagnostics_grad_sq[:, 0])
    assert len(seen) == 4 and np.allclose(norms, seen, rtol=1e-5, atol=0)
    d = alg.diagnostics
    assert abs(d["grad_norm"] - np.mean(seen)) <= 1e-5 * np.mean(seen) and abs(d["grad_norm_max"] - max(seen)) <= 1e-5 * max(seen)
    assert d["grad_clipped_share"] == np.mean(np.asarray(seen) > 0.55) and 0.0 < d["grad_clipped_share"] < 1.0


def test_grad_sqnorm_of_graph_mode_is_what_the_clip_saw(host_pair, monkeypatch):
    """graph mode on the host build: go2nn_grad_sqnorm in front of the clip + Adam call against the gradients that call receives"""
    from go2_rl_gym_amd.rsl_rl.algorithms import _base
    seen = []
    real = _base._RolloutHeads._clip_adam

    def spy(self, optimizer, params, kl_mean=None):
        seen.append(math.sqrt(sum(float(p.grad.double().square().sum()) for p in params if p.grad is not None)))
        return real(self, optimizer, params, kl_mean)
    monkeypatch.setattr(_base._RolloutHeads, "_clip_adam", spy)
    alg = make_alg("PPO", host_pair, diagnostics=True, **GRAPH)
    alg.update()
    assert len(seen) == 4 and np.allclose(np.sqrt(alg.diagnostics_grad_sq[:, 0]), seen, rtol=1e-9, atol=0)


def test_explained_variance_is_one_for_a_perfect_critic_and_zero_for_the_mean():
    g = torch.Generator().manual_seed(2)
    B, A = 500, 12
    r = lambda *s: torch.randn(*s, generator=g)
    mu, sigma, act, old_lp, adv, tv = r(B, A), 0.5 + torch.rand(A, generator=g), r(B, A), r(B), r(B), r(B)
    returns = 1.5 + 2.0 * r(B)
    rows = lambda v: _diag.diag_rows_torch(mu, sigma, v, act, mu, sigma.expand(B, A), old_lp, adv, tv, returns, CLIP)[0].numpy()
    perfect, mean = _diag.figures(rows(returns.clone())), _diag.figures(rows(torch.full((B,), float(returns.double().mean()))))
    print("[update diag] explained variance: perfect critic %.9f, constant mean %.3e" % (perfect["explained_variance"], mean["explained_variance"]))
    assert abs(perfect["explained_variance"] - 1.0) <= 1e-6 and perfect["value_err_max"] == 0.0 and abs(mean["explained_variance"]) <= 1e-6
    assert math.isnan(_diag.figures(_diag.diag_rows_torch(mu, sigma, r(B), act, mu, sigma.expand(B, A), old_lp, adv, tv, torch.full((B,), 0.75), CLIP)[0].numpy())["explained_variance"])
    # and through an update whose critic head is SET so that v == returns on the batch: the head passes hidden unit 0 through (weight e_0, bias 0) and the stored
    # returns are that unit's activations
    alg = _ppo(diagnostics=True, num_learning_epochs=1, num_mini_batches=1, learning_rate=0.0, schedule="fixed")
    fill_storage(alg, 6, scale=0.3)
    critic = alg.actor_critic.critic
    with torch.no_grad():
        critic[-1].weight.zero_(); critic[-1].weight[0, 0] = 1.0; critic[-1].bias.zero_()
        hidden = critic[:-1](alg.storage.privileged_observations.flatten(0, 1))
        alg.storage.returns.copy_(hidden[:, :1].view(alg.storage.returns.shape))
    assert float(hidden[:, 0].var()) > 1e-4
    alg.update()
    assert abs(alg.diagnostics["explained_variance"] - 1.0) <= 1e-6 and alg.diagnostics["value_err_max"] <= 1e-6


def test_cts_segments_add_up():
    _, alg = make_cts("cpu", "CTS", num_learning_epochs=2, num_mini_batches=2, diagnostics=True)
    alg.init_storage(8, 6, [45], [60], [12])
    fill_cts_storage(alg, 3)
    alg.update()
    tab, d = alg.diagnostics_table, alg.diagnostics
    n_t = alg._teacher_rows()
    assert set(d) == {"teacher", "student", "all"} and (tab[:, 0, COL["rows"]] == n_t).all() and (tab[:, 1, COL["rows"]] == 24 - n_t).all()
    sums = [j for k, j in COL.items() if k not in _nn.DIAG_MAX_COLS + _nn.DIAG_MIN_COLS]
    pooled = {s: _diag.pool_rows(tab[:, i]) for i, s in enumerate(("teacher", "student"))}
    both = _diag.pool_rows(tab)
    assert np.array_equal(both[sums], (pooled["teacher"] + pooled["student"])[sums])
    assert both[COL["ratio_max"]] == max(pooled["teacher"][COL["ratio_max"]], pooled["student"][COL["ratio_max"]])
    assert d["all"]["clip_fraction"] == both[COL["ratio_clipped"]] / both[COL["rows"]] and d["teacher"]["kl"] == pooled["teacher"][COL["kl_sum"]] / pooled["teacher"][COL["rows"]]
    assert "grad_norm" in d["all"] and "student_encoder_grad_norm" in d["all"] and "grad_norm" not in d["teacher"]


# ---- 7. graph mode equals the eager mode on the host build, per slot ---------------------------------------------------------------------------------------------
CLIP_OFF = 1.0e6          # (tests/test_gpu_parity.py: the smooth objective)


def to_float64(alg):
    """the eager formulation in float64: networks, optimizer state (none yet) and every floating tensor of the storage"""
    alg.actor_critic.double()
    st = alg.storage
    for k, v in list(vars(st).items()):
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(st, k, v.double())


@pytest.mark.parametrize("kind", ["PPO", "CTS"])
def test_graph_mode_fills_the_slots_the_eager_mode_fills(host_pair, monkeypatch, kind):
    """Three arms from the same weights and storage under ONE fixed permutation, clip_param = CLIP_OFF, a fixed learning rate: the eager mode in float64 (the
    reference), the eager mode in fp32 (the torch statement: the yardstick) and graph mode on the host build (go2nn_ppo_diag).  Slot by slot the counts are equal
    and every other column of graph mode is at most 4 x as far from float64 as the eager fp32 mode is, plus 1e-6 x the column's magnitude: test 1's rule, the
    magnitudes recorded from the reference arm's rows (terms_and_magnitudes64)."""
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(6))
    real_randperm = torch.randperm          # (the CTS storage draws one permutation per group: each fixed by its length)
    monkeypatch.setattr(torch, "randperm", lambda n_, **kw: perm if n_ == 48 else real_randperm(n_, generator=torch.Generator().manual_seed(n_)))
    tabs, mags = {}, []
    real_terms = _diag.diag_terms_torch
    for mode, kw in (("float64", {}), ("eager", {}), ("graph", GRAPH)):
        alg = make_alg(kind, host_pair, diagnostics=True, clip_param=CLIP_OFF, schedule="fixed", **kw)
        if mode == "float64":
            to_float64(alg)
            split = 0 if kind == "PPO" else alg._teacher_rows()

            def recording(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, clip):
                t = real_terms(mu, sigma, value, actions, old_mu, old_sigma, old_logp, adv, old_values, returns, clip)
                assert t.dtype == torch.float64
                n = lambda x, shape: x.detach().double().numpy().reshape(shape)
                B, A = mu.shape
                terms, m, _ = terms_and_magnitudes64(n(mu, (B, A)), n(value, B), np.broadcast_to(n(sigma, (-1, A)), (B, A)), n(actions, (B, A)), n(old_mu, (B, A)),
                                                     n(old_sigma, (B, A)), n(old_logp, B), n(adv, B), n(old_values, B), n(returns, B), clip)
                assert np.allclose(terms, t.numpy(), rtol=1e-12, atol=1e-13)          # (the reference arm's rows ARE the float64 restatement)
                mags.append(np.stack([pool_magnitudes(terms[lo:hi], m[lo:hi]) for lo, hi in ([(0, B)] if not split else [(0, split), (split, B)])]))
                return t
            monkeypatch.setattr(_diag, "diag_terms_torch", recording)
        torch.manual_seed(20)
        alg.update()
        monkeypatch.setattr(_diag, "diag_terms_torch", real_terms)
        tabs[mode] = alg.diagnostics_table
    ref, e, g = tabs["float64"], tabs["eager"], tabs["graph"]
    mag = np.stack(mags)
    assert ref.shape == e.shape == g.shape == mag.shape
    for k in COUNT_COLS:
        assert np.array_equal(e[..., COL[k]], g[..., COL[k]]) and np.array_equal(ref[..., COL[k]], g[..., COL[k]]), k
    for k, j in COL.items():
        if k in COUNT_COLS:
            continue
        gk, gt, floor = np.abs(g[..., j] - ref[..., j]), np.abs(e[..., j] - ref[..., j]), 1e-6 * mag[..., j]
        print("[update diag, graph vs eager, %s] %-14s largest gap to float64: graph mode %.2e, eager fp32 %.2e; smallest slack %.2e" % (kind, k, gk.max(), gt.max(), (4.0 * gt + floor - gk).min()))
        assert (gk <= 4.0 * gt + floor).all(), (k, gk, gt, floor)


# ---- 8. the refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_recurrent_and_state_dependent_std_are_refused():
    from go2_rl_gym_amd.rsl_rl.algorithms import MCPCTS, PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCriticMCPCTS, ActorCriticRecurrent
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], rnn_hidden_size=16)
    with pytest.raises(NotImplementedError, match="recurrent"):
        PPO(ac, diagnostics=True, device="cpu")
    PPO(ac, device="cpu")          # (no existing behaviour changes)
    model = ActorCriticMCPCTS(45, 60, 12, 8, 5, [True] * 6 + [False] * 3 + [True] * 36, student_expert_num=4, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], teacher_encoder_hidden_dims=[32, 16], student_encoder_hidden_dims=[32, 16],
                              latent_dim=8)
    with pytest.raises(NotImplementedError, match="state-dependent std"):
        MCPCTS(model, 8, 5, diagnostics=True, device="cpu")
    MCPCTS(model, 8, 5, device="cpu")


# ---- 9. the flag reaches the algorithm and the log ------------------------------------------------------------------------------------------------------------
def test_flag_reaches_the_algorithm_and_the_tags_are_written():
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    assert train_cfg.algorithm.diagnostics is False and task_registry.get_cfgs("go2_flat_cts")[1].algorithm.diagnostics is False
    common = ["--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"]
    args = get_args(["--task", "go2_flat", *common])
    assert update_cfg_from_args(None, copy.deepcopy(train_cfg), args)[1].algorithm.diagnostics is False
    args = get_args(["--task", "go2_flat", *common, "--diagnostics"])
    _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), args)
    assert cfg.algorithm.diagnostics is True
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=cfg, log_root=None)
    assert runner.alg._diag is not None and runner.alg._diag.steps == cfg.algorithm.num_learning_epochs * cfg.algorithm.num_mini_batches
    args = get_args(["--task", "go2_flat_cts", *common, "--diagnostics"])
    assert update_cfg_from_args(None, copy.deepcopy(task_registry.get_cfgs("go2_flat_cts")[1]), args)[1].algorithm.diagnostics is True


class Scalars:
    """the runner's writer stub: every add_scalar call, in order"""
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value)))


@pytest.mark.parametrize("kind", ["PPO", "CTS"])
def test_runner_writes_the_tags_and_the_report_lines(kind, tmp_path, capsys):
    """one learn() iteration on the scripted env of tests/test_cts_golden.py with the key on: Diag/<key> for PPO, Diag/<segment>/<key> for CTS, the values those of
    alg.diagnostics, and two more lines of the iteration report; with the key off no Diag tag at all"""
    from go2_rl_gym_amd.rsl_rl.runners import OnPolicyRunner, OnPolicyRunnerCTS
    from helpers import ROOT
    from test_cts_golden import ScriptedEnv, _train_cfg
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ppo_runner_log.npz" if kind == "PPO" else "cts_iteration.npz")))
    T = g["rew"].shape[0]
    for key in (False, True):
        if kind == "PPO":
            cfg = {"runner": dict(policy_class_name="ActorCritic", algorithm_class_name="PPO", num_steps_per_env=T, max_iterations=1, save_interval=50, experiment_name="golden", run_name=""),
                   "algorithm": dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=2, num_mini_batches=2,
                                     learning_rate=1e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0),
                   "policy": dict(init_noise_std=1.0, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu")}
        else:
            cfg = _train_cfg("CTS", T)
        if key:
            cfg["algorithm"]["diagnostics"] = True
        os.makedirs(tmp_path / str(key))
        runner = (OnPolicyRunner if kind == "PPO" else OnPolicyRunnerCTS)(ScriptedEnv(g, load_oracle()), cfg, log_dir=str(tmp_path / str(key)), device="cpu")
        runner.writer = Scalars()
        runner.learn(1, init_at_random_ep_len=False)
        diag = {t: v for t, v in runner.writer.rows if t.startswith("Diag/")}
        out = capsys.readouterr().out
        if not key:
            assert not diag and runner.alg.diagnostics is None and "Clip frac" not in out
            continue
        d = runner.alg.diagnostics
        pre = "Diag/" if kind == "PPO" else "Diag/all/"
        assert {pre + k for k in ("clip_fraction", "approx_kl", "kl", "explained_variance", "grad_norm", "grad_clipped_share", "clip_fraction/last_epoch",
                                  "approx_kl/first_epoch")} <= set(diag)
        if kind == "PPO":
            assert diag["Diag/clip_fraction"] == d["clip_fraction"] and len(diag) == len(d)
        else:
            assert diag["Diag/teacher/kl"] == d["teacher"]["kl"] and diag["Diag/student/clip_fraction"] == d["student"]["clip_fraction"]
            assert "Diag/all/student_encoder_grad_norm" in diag and len(diag) == sum(len(v) for v in d.values())
        assert "Clip frac / approx KL / EV:" in out and "Grad norm / clipped share:" in out
