"""The mirror (equivariance) loss of symmetry-augmented PPO on the CPU (`algorithm.mirror_loss_coef`): go2nn_mirror_loss (host build) against a float64 restatement of its
formulas with the torch fp32 formulation as the yardstick of the error, its refusals, the swap invariance, an equivariant network reading zero, the graph-mode update on
the host build against torch, the term lowering what it penalises, the flag-off identity and the way from the command line to the algorithm.
tests/test_gpu_mirror_loss.py runs the same cases on the device."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import load_nn_emu, load_oracle
from test_asymmetry_host import ACT_PERM, ACT_SIGN, OBS_TABLE, equivariant_actor_critic, one_hidden_actor_critic
from test_symmetry_host import _ppo, fill_storage
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd.envs.go2.go2_config import GO2Cfg
from go2_rl_gym_amd.utils.symmetry import mirror_rows, mirror_tables

GO2NN_EINVAL = -22
SENTINEL = 64
FILL = 7.25
QUANTITIES = ("loss", "gz_a", "dW_mu", "gb_a", "db_mu")
# B pairs x (A actions, K hidden units): the Go2's (12, 128) at every B — one pair, fewer pairs than row lanes, a ragged last group, more than one workgroup, many —, the
# other head shapes (one action, a K below one full row of lanes, A and K between the kernel's template sizes, the largest) at a small and a several-workgroup B
SHAPES = [(B, 12, 128) for B in (1, 3, 63, 257, 1000)] + [(B, A, K) for A, K in ((1, 4), (4, 20), (13, 132), (16, 256)) for B in (3, 257)]


@pytest.fixture(scope="module")
def tables():
    return mirror_tables(GO2Cfg())


@pytest.fixture(scope="module")
def emu():
    return load_nn_emu()


# ---- the cases and their references --------------------------------------------------------------------------------------------------------------------------
def involution(A, rng):
    """a random involution of A columns with sign[perm[j]] == sign[j]: swapped pairs of either sign, fixed points of either sign (the first fixed point carries -1)"""
    order = rng.permutation(A)
    perm, sign = np.arange(A, dtype=np.int16), np.ones(A, np.float32)
    n_pairs = A // 3
    for a, b in zip(order[0:2 * n_pairs:2], order[1:2 * n_pairs:2]):
        perm[a], perm[b] = b, a
        sign[a] = sign[b] = rng.choice([-1.0, 1.0])
    for i, j in enumerate(order[2 * n_pairs:]):
        sign[j] = -1.0 if i % 2 == 0 else 1.0
    p = perm.astype(np.int64)
    assert np.array_equal(p[p], np.arange(A)) and np.array_equal(sign[p], sign) and (sign[p == np.arange(A)] == -1.0).any()
    return perm, sign


def make_case(B, A, K, tables, seed=0, coef=0.75):
    """(coef: a value fp32 holds exactly — the struct carries it as a float, the float64 reference reads the same number)"""
    rng = np.random.default_rng(seed + 1000003 * B + 1009 * A + K)
    z = rng.normal(0.0, 1.0, (2 * B, K))
    y = np.where(z > 0, z, np.expm1(z)).astype(np.float32)          # an ELU output: both branches of ELU' occur
    assert (y > 0).any() and (y <= 0).any()
    perm, sign = (np.ascontiguousarray(tables.action[0], np.int16), np.ascontiguousarray(tables.action[1], np.float32)) if A == 12 else involution(A, rng)
    return dict(B=B, A=A, K=K, coef=coef, y=y, w=(rng.normal(0.0, 1.0, (A, K)) / math.sqrt(K)).astype(np.float32), b=rng.normal(0.0, 0.3, A).astype(np.float32),
                gz0=rng.normal(0.0, 1e-3, (2 * B, K)).astype(np.float32), perm=perm, sign=sign)


def reference64(c):
    """the formulas of the issue's section 1 in float64 numpy"""
    B, A, K, coef = c["B"], c["A"], c["K"], c["coef"]
    y, w, b, p, s = c["y"].astype(np.float64), c["w"].astype(np.float64), c["b"].astype(np.float64), c["perm"].astype(np.int64), c["sign"].astype(np.float64)
    mu = y @ w.T + b
    e = mu[:B] - s * mu[B:][:, p]
    g = np.zeros_like(mu)
    g[:B] = 2.0 * coef / (B * A) * e
    g[B:][:, p] = -s * g[:B]
    add = (g @ w) * np.where(y > 0, 1.0, y + 1.0)
    return dict(loss=np.array([coef / (B * A) * (e ** 2).sum()]), gz_a=c["gz0"].astype(np.float64) + add, dW_mu=g.T @ y, gb_a=add.sum(0), db_mu=g.sum(0))


def torch32(c, dev="cpu"):
    """the eager formulation: the same five quantities with torch autograd in fp32 on `dev`"""
    B, coef = c["B"], c["coef"]
    t = lambda k: torch.from_numpy(c[k]).to(dev)
    y, w, b = t("y").requires_grad_(), t("w").requires_grad_(), t("b").requires_grad_()
    perm, sign = torch.from_numpy(c["perm"].astype(np.int64)).to(dev), t("sign")
    mu = torch.addmm(b, y, w.t())
    loss = coef * (mu[:B] - mu[B:][:, perm] * sign).square().mean()
    gy, gw, gb = torch.autograd.grad(loss, [y, w, b])
    with torch.no_grad():
        add = gy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
        out = dict(loss=loss.reshape(1), gz_a=t("gz0") + add, dW_mu=gw, gb_a=add.sum(0), db_mu=gb)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def run_kernel(lib, c, dev="cpu", stream=None, patch=None, shape=None, null_struct=False):
    """one go2nn_mirror_loss call (+ go2nn_sum_rows over its partial rows) on tensors of `dev`; gz_a and the partial rows are followed by SENTINEL floats.
    patch(struct): edits the argument struct; shape: (B, A, K) handed to the call instead of the case's
    -> (rc, the five quantities or None, the gz_a buffer, the partials buffer — both with their sentinels, as numpy)"""
    B, A, K = c["B"], c["A"], c["K"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    y, w, b, perm, sign = t(c["y"]), t(c["w"]), t(c["b"]), t(c["perm"]), t(c["sign"])
    gz = torch.full((2 * B * K + SENTINEL,), FILL, device=dev)
    gz[:2 * B * K] = t(c["gz0"]).reshape(-1)
    rows, cols = lib.go2nn_mirror_loss_rows(B, A, K), lib.go2nn_mirror_loss_cols(A, K)
    assert rows >= 1 and cols == 4 + (A + 1) * K + A, lib.go2nn_last_error()
    part = torch.full((rows * cols + SENTINEL,), FILL, device=dev)
    sB, sA, sK = shape or (B, A, K)
    m = _nn.Go2nnMirrorLoss(y.data_ptr(), w.data_ptr(), b.data_ptr(), perm.data_ptr(), sign.data_ptr(), gz.data_ptr(), part.data_ptr(), sB, sA, sK, c["coef"])
    if patch:
        patch(m)
    rc = lib.go2nn_mirror_loss(None if null_struct else C.byref(m), stream)
    out = None
    if rc == 0:
        tot = torch.empty(cols, device=dev)
        job = _nn.Go2nnSumJob(part.data_ptr(), tot.data_ptr(), rows, cols, None, 0, 0, 0, 0)
        assert lib.go2nn_sum_rows(C.byref(job), 1, stream) == 0, lib.go2nn_last_error()
    if dev != "cpu":
        torch.cuda.synchronize()
    if rc == 0:
        s = tot.cpu().numpy()
        assert (s[1:4] == 0.0).all()
        out = dict(loss=s[:1].copy(), gz_a=gz[:2 * B * K].cpu().numpy().reshape(2 * B, K), dW_mu=s[4:4 + A * K].reshape(A, K), gb_a=s[4 + A * K:4 + (A + 1) * K], db_mu=s[4 + (A + 1) * K:])
    return rc, out, gz.cpu().numpy(), part.cpu().numpy()


def errors(got, ref):
    return {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) for k in QUANTITIES}


def check_entry_point(lib, c, dev="cpu", stream=None, what="host build"):
    """test A on one shape: the kernel's error against float64 is at most 4 x the fp32 torch formulation's, per quantity; sentinels; two launches, one result; coef 0"""
    ref = reference64(c)
    rc, got, gz, part = run_kernel(lib, c, dev, stream)
    assert rc == 0, lib.go2nn_last_error()
    assert (gz[-SENTINEL:] == FILL).all() and (part[-SENTINEL:] == FILL).all()
    ek, et = errors(got, ref), errors(torch32(c, dev), ref)
    print("[mirror loss, %s] B %d A %d K %d: error against float64, kernel / torch fp32: %s" % (what, c["B"], c["A"], c["K"], "  ".join("%s %.2e / %.2e" % (k, ek[k], et[k]) for k in QUANTITIES)))
    for k in QUANTITIES:
        assert np.abs(ref[k]).max() > 0 and ek[k] <= 4.0 * et[k], (k, ek[k], et[k])
    rc2, got2, gz2, part2 = run_kernel(lib, c, dev, stream)
    assert rc2 == 0 and gz2.tobytes() == gz.tobytes() and part2.tobytes() == part.tobytes()
    rc0, got0, gz0, _ = run_kernel(lib, dict(c, coef=0.0), dev, stream)
    assert rc0 == 0 and gz0[:-SENTINEL].tobytes() == c["gz0"].tobytes() and all((got0[k] == 0.0).all() for k in QUANTITIES if k != "gz_a")
    return ek, et


# ---- A. the entry point against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,K", SHAPES)
def test_entry_point_against_float64(emu, tables, B, A, K):
    """The host build's loss, gz_a (prefill + the added term), dW_mu, gb_a and db_mu against the float64 restatement: its largest error per quantity is at most 4 x that
    of torch autograd in fp32 on the same inputs (the factor covers another summation order over up to 1000 pairs).  Measured, host build / torch fp32 on the CPU (every
    shape is printed by the run): at (1000, 12, 128) loss 5.3e-8 / 5.3e-8, gz_a 2.4e-10 / 2.3e-10, dW_mu 1.0e-8 / 1.6e-8, gb_a 1.1e-8 / 5.6e-9, db_mu 2.1e-8 / 2.1e-8;
    at (3, 1, 4) loss 3.6e-8 / 1.6e-7, gz_a 3.5e-8 / 6.9e-8, dW_mu 1.6e-7 / 1.6e-7, gb_a 7.6e-8 / 7.6e-8, db_mu 3.2e-8 / 8.7e-8; the largest ratio over the 13 shapes is
    3.0 (gb_a at (257, 1, 4): 8.9e-8 / 2.9e-8); the loss, summed in fp64 and rounded once, is never further off than torch's."""
    check_entry_point(emu, make_case(B, A, K, tables))


# ---- B. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, tables, dev="cpu", stream=None):
    c = make_case(3, 12, 128, tables)

    def refused(**kw):
        rc, _, gz, part = run_kernel(lib, c, dev, stream, **kw)
        assert rc == GO2NN_EINVAL and lib.go2nn_last_error().decode() != "", kw
        assert gz[:-SENTINEL].tobytes() == c["gz0"].tobytes() and (gz[-SENTINEL:] == FILL).all() and (part == FILL).all(), kw

    refused(null_struct=True)
    for field in ("y_a", "gz_a", "partials", "sign"):          # (sign: perm without sign)
        refused(patch=lambda m, f=field: setattr(m, f, None))
    refused(patch=lambda m: setattr(m, "perm", None))          # sign without perm
    refused(shape=(0, 12, 128))
    refused(shape=(3, 17, 128))
    refused(shape=(3, 12, 6))
    refused(shape=(3, 12, 260))
    assert lib.go2nn_mirror_loss_rows(0, 12, 128) == GO2NN_EINVAL and lib.go2nn_mirror_loss_cols(17, 128) == GO2NN_EINVAL and lib.go2nn_mirror_loss_cols(12, 6) == GO2NN_EINVAL


def check_table_refusals(lib, tables):
    perm, sign = np.ascontiguousarray(tables.action[0], np.int16), np.ascontiguousarray(tables.action[1], np.float32)
    chk = lambda p, s, A=12: lib.go2nn_mirror_loss_check_table(p.ctypes.data, s.ctypes.data, A)
    assert chk(perm, sign) == 0
    for bad in (12, -1):
        p = perm.copy(); p[7] = bad
        assert chk(p, sign) == GO2NN_EINVAL and b"perm" in lib.go2nn_last_error()
    s = sign.copy(); s[2] = 0.5
    assert chk(perm, s) == GO2NN_EINVAL and b"sign" in lib.go2nn_last_error()
    p = np.arange(12, dtype=np.int16); p[[0, 1, 2]] = [1, 2, 0]          # a 3-cycle
    assert chk(p, np.ones(12, np.float32)) == GO2NN_EINVAL and b"involution" in lib.go2nn_last_error()
    p = np.arange(12, dtype=np.int16); p[[4, 5]] = [5, 4]
    s = np.ones(12, np.float32); s[4] = -1.0                           # a swapped pair with opposite signs
    assert chk(p, s) == GO2NN_EINVAL and b"sign" in lib.go2nn_last_error()
    assert lib.go2nn_mirror_loss_check_table(None, sign.ctypes.data, 12) == GO2NN_EINVAL and chk(perm, sign, 0) == GO2NN_EINVAL and chk(perm, sign, 17) == GO2NN_EINVAL
    with pytest.raises(ValueError, match="involution"):
        _nn.mirror_loss_table_tensors(lib, (np.array([1, 2, 0], np.int16), np.ones(3, np.float32)), "cpu")


def test_refusals_write_nothing(emu, tables):
    check_refusals(emu, tables)
    check_table_refusals(emu, tables)
    # the host build can read the table: a bad one is refused by the call itself
    c = make_case(3, 12, 128, tables)
    c["perm"] = c["perm"].copy(); c["perm"][0] = 1          # 0 -> 1 -> 4 ...: not an involution
    rc, _, gz, part = run_kernel(emu, c)
    assert rc == GO2NN_EINVAL and (part == FILL).all() and gz[:-SENTINEL].tobytes() == c["gz0"].tobytes()


def test_constructor_checks(tables):
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO
    from go2_rl_gym_amd.rsl_rl.algorithms.cts import CTS
    from go2_rl_gym_amd.rsl_rl.algorithms.moe_cts import MoECTS
    from go2_rl_gym_amd.rsl_rl.modules.actor_critic_recurrent import ActorCriticRecurrent
    with pytest.raises(ValueError, match="symmetry"):
        _ppo(None, mirror_loss_coef=0.1)
    with pytest.raises(ValueError, match="symmetry"):
        _ppo(None, pass_arg=False, mirror_loss_coef=0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mirror_loss_coef"):
            _ppo(tables, mirror_loss_coef=bad)
    ac = ActorCriticRecurrent(45, 263, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_hidden_size=16)
    with pytest.raises(NotImplementedError, match="recurrent"):
        PPO(ac, device="cpu", lib=load_oracle(), mirror_loss_coef=0.1)
    PPO(ac, device="cpu", lib=load_oracle(), mirror_loss_coef=0.0)
    for cls in (CTS, MoECTS):
        with pytest.raises(NotImplementedError, match="mirror loss"):
            cls(None, 8, 5, mirror_loss_coef=0.1)
        with pytest.raises(NotImplementedError, match="CTS"):          # (what the symmetry flag alone gives: unchanged)
            cls(None, 8, 5, symmetry=tables, mirror_loss_coef=0.1)
    alg = _ppo(tables, mirror_loss_coef=0.25)
    assert alg.mirror_loss_coef == 0.25 and alg._sym is not None and alg.mirror_loss == 0.0


# ---- C. swap invariance --------------------------------------------------------------------------------------------------------------------------------------
def check_swap(lib, tables, dev="cpu", stream=None):
    """rows r <-> B + r of y_a: the same loss, the halves of the added gz_a swapped, the same dW_mu, gb_a, db_mu — exact for an involutive table, here within the bound
    of test A (4 x the fp32 torch formulation's error against float64, per quantity, of the unswapped case)"""
    for B, A, K in ((257, 12, 128), (63, 13, 132), (3, 4, 20)):
        c = make_case(B, A, K, tables, seed=3)
        sw = dict(c, y=np.concatenate([c["y"][B:], c["y"][:B]]), gz0=np.concatenate([c["gz0"][B:], c["gz0"][:B]]))
        ref = reference64(c)
        et = errors(torch32(c, dev), ref)
        (rc, got, _, _), (rc2, got2, _, _) = run_kernel(lib, c, dev, stream), run_kernel(lib, sw, dev, stream)
        assert rc == 0 and rc2 == 0
        got2 = dict(got2, gz_a=np.concatenate([got2["gz_a"][B:], got2["gz_a"][:B]]))
        for k in QUANTITIES:
            # each of the two is within 4 et of float64, where the two are equal
            assert np.abs(got[k].astype(np.float64) - got2[k]).max() <= 2 * 4.0 * et[k], (B, A, K, k)
            assert np.abs(got2[k].astype(np.float64) - ref[k]).max() <= 4.0 * et[k], (B, A, K, k)


def test_swapping_the_halves(emu, tables):
    check_swap(emu, tables)


# ---- D. an equivariant network reads zero ------------------------------------------------------------------------------------------------------------------
def last_hidden_case(ac, obs, dev="cpu", coef=0.5):
    """-> (the entry point's case on the last hidden activations of `ac`'s actor over [obs | mirror(obs)], delta: the RMS gap of the fp32 forward's means to float64)"""
    x = np.concatenate([obs, mirror_rows(obs, OBS_TABLE)]).astype(np.float32)
    actor = copy.deepcopy(ac.actor).to(dev)
    with torch.no_grad():
        xt = torch.from_numpy(x).to(dev)
        y = actor[1](actor[0](xt))
        mu = actor[2](y)
        mu64 = copy.deepcopy(ac.actor).cpu().double()(torch.from_numpy(x.astype(np.float64))).numpy()
    delta = float(np.sqrt(((mu.cpu().numpy().astype(np.float64) - mu64) ** 2).mean()))
    B = obs.shape[0]
    c = dict(B=B, A=12, K=y.shape[1], coef=coef, y=y.cpu().numpy(), w=actor[2].weight.detach().cpu().numpy().copy(), b=actor[2].bias.detach().cpu().numpy().copy(),
             gz0=np.zeros((2 * B, y.shape[1]), np.float32), perm=np.ascontiguousarray(ACT_PERM, np.int16), sign=np.ascontiguousarray(ACT_SIGN, np.float32))
    return c, delta


def check_equivariant_reads_zero(lib, dev="cpu", stream=None, what="host build"):
    obs = np.random.default_rng(11).normal(0.0, 1.0, (256, 45)).astype(np.float32)
    c, delta = last_hidden_case(equivariant_actor_critic(), obs, dev)
    rc, got, _, _ = run_kernel(lib, c, dev, stream)
    assert rc == 0 and 0 < delta < 1e-5
    ms, bound = float(got["loss"][0]) / c["coef"], (4.0 * delta) ** 2
    c2, _ = last_hidden_case(one_hidden_actor_critic(16, seed=1), obs, dev)
    rc2, got2, _, _ = run_kernel(lib, c2, dev, stream)
    ms2 = float(got2["loss"][0]) / c2["coef"]
    print("[mirror loss, %s] equivariant by construction: L / coef %.3e, bound (4 delta)^2 %.3e (delta %.3e); random weights of the same shape: %.3e = %.1e x the bound"
          % (what, ms, bound, delta, ms2, ms2 / bound))
    assert rc2 == 0 and ms <= bound and ms2 >= 1000.0 * bound


def test_equivariant_network_reads_zero(emu):
    """L_mirror / coef of an actor made equivariant by construction (tests/test_asymmetry_host.py), on 256 random observations and their mirror images, is at most
    (4 delta)^2, delta being the fp32 forward's own RMS gap to float64 in the same run; random weights of the same shape read at least 1000 x that bound."""
    check_equivariant_reads_zero(emu)


# ---- E. graph mode on the host build against torch -----------------------------------------------------------------------------------------------------------
class Counting:
    """the host library with the calls of go2nn_mirror_loss counted"""

    def __init__(self, lib):
        self._lib, self.mirror_loss_calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "go2nn_mirror_loss":
            return fn

        def counted(*a):
            self.mirror_loss_calls += 1
            return fn(*a)
        return counted


@pytest.fixture
def host_pair():
    """the go2sim oracle and the go2nn host build as the library pair of modules/fused.py: the no-autograd mini-batch (go2nn_ppo_heads, go2nn_mirror_loss) runs on the CPU"""
    from go2_rl_gym_amd.rsl_rl.modules import fused
    was = (fused._LIB, fused._NN)
    lib = Counting(load_nn_emu())
    fused.set_library(load_oracle())
    fused.set_nn_library(lib)
    yield lib
    fused._LIB, fused._NN = was


ONE_BATCH = dict(num_learning_epochs=1, num_mini_batches=1, learning_rate=0.0, max_grad_norm=1e9, schedule="fixed")


def torch_gradients(alg, batch, double):
    """loss.backward() of the eager formulation on `batch` (already augmented) -> ({parameter name: gradient}, L_mirror / coef); double: in float64 on a copy"""
    if double:
        alg.actor_critic.distribution = None          # (the last forward's: not a leaf, deepcopy refuses it)
        alg = copy.copy(alg)
        alg.actor_critic = copy.deepcopy(alg.actor_critic).double()
        alg._sym_t = None
        batch = tuple(t.double() for t in batch[:9])
    alg.actor_critic.zero_grad()
    loss = alg._losses(*batch[:9])[0]
    loss.backward()
    return {n: p.grad.detach().numpy().astype(np.float64) for n, p in alg.actor_critic.named_parameters()}, (float(alg._ml) if alg.mirror_loss_coef > 0.0 else None)


@pytest.mark.parametrize("branch", ["heads", "loss_kernel", "autograd"])
def test_graph_mode_update_on_the_host_build_equals_torch(tables, host_pair, monkeypatch, branch):
    """One mini-batch at learning rate 0 through the graph-mode update (run eagerly on the CPU) with mirror_loss_coef = 0.5: every parameter's .grad against the float64
    torch restatement of the whole objective is at most 4 x as far as the fp32 eager formulation is (the bound of test A), and alg.mirror_loss agrees to 1e-5 relative.
    The three ways the graph-mode step forms its gradients: the no-autograd mini-batch (go2nn_mirror_loss on the host build), autograd seeded with the loss kernel's
    gradients plus the torch expression of g, and plain autograd."""
    from go2_rl_gym_amd.rsl_rl.modules import fused
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(6))
    monkeypatch.setattr(torch, "randperm", lambda n_, **kw: perm)
    if branch != "heads":
        fused._LIB, fused._NN = None, None
    alg = _ppo(tables, use_graphs="uncaptured", fused_loss=branch != "autograd", mirror_loss_coef=0.5, **ONE_BATCH)
    alg.nn_lib = host_pair
    fill_storage(alg, 7, scale=0.3)
    eager = _ppo(tables, mirror_loss_coef=0.5, **ONE_BATCH)
    fill_storage(eager, 7, scale=0.3)
    batch = eager._sym_batch(next(iter(eager.storage.mini_batch_generator(1, 1))))
    g32, ml32 = torch_gradients(eager, batch, False)
    g64, ml64 = torch_gradients(eager, batch, True)
    w0 = torch.cat([p.detach().reshape(-1) for p in alg.actor_critic.parameters()]).clone()
    alg.update()
    assert torch.equal(w0, torch.cat([p.detach().reshape(-1) for p in alg.actor_critic.parameters()])) and alg._acc.numel() == 3
    assert host_pair.mirror_loss_calls == (1 if branch == "heads" else 0)
    for k, got, want in zip(alg._KEYS, alg._graph_batch(0), batch):
        assert torch.equal(got, want), k
    assert ml64 > 1e-3 and abs(alg.mirror_loss - ml64) <= 1e-5 * ml64 and abs(ml32 - ml64) <= 1e-5 * ml64, (alg.mirror_loss, ml32, ml64)
    for n, p in alg.actor_critic.named_parameters():
        ek, et = float(np.abs(p.grad.numpy() - g64[n]).max()), float(np.abs(g32[n] - g64[n]).max())
        print("[mirror loss, graph mode on the host build, %s] %s: gradient error against float64 %.2e, eager fp32 %.2e" % (branch, n, ek, et))
        assert np.abs(g64[n]).max() > 0 and ek <= 4.0 * et, (n, ek, et)
    # and the term is in those gradients: without it the actor's are others
    plain = _ppo(tables, **ONE_BATCH)
    fill_storage(plain, 7, scale=0.3)
    g0, _ = torch_gradients(plain, batch, True)
    assert np.abs(g0["actor.4.weight"] - g64["actor.4.weight"]).max() > 1e-4 and np.abs(g0["critic.4.weight"] - g64["critic.4.weight"]).max() < 1e-12


# ---- F. the term does what it is for -------------------------------------------------------------------------------------------------------------------------
def mirror_gap_of(alg, obs):
    """mean((pi(o) - M_a pi(M_o o))^2) over the rows `obs` with the algorithm's own tables, in float64 on a copy of the actor"""
    s = alg._sym
    actor = copy.deepcopy(alg.actor_critic.actor).cpu().double()
    o = obs.detach().cpu().numpy().reshape(-1, obs.shape[-1]).astype(np.float64)
    with torch.no_grad():
        a, am = actor(torch.from_numpy(o)).numpy(), actor(torch.from_numpy(mirror_rows(o, s.obs))).numpy()
    return float(((a - mirror_rows(am, s.action)) ** 2).mean())


def check_term_lowers_the_gap(tables, device, lib, what, **kw):
    from go2_rl_gym_amd.rsl_rl.algorithms import PPO
    from go2_rl_gym_amd.rsl_rl.modules import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(45, 263, 12, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], activation="elu", init_noise_std=0.8)
    alg = PPO(ac, num_learning_epochs=5, num_mini_batches=1, clip_param=0.2, value_loss_coef=0.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
              use_clipped_value_loss=True, schedule="fixed", device=device, lib=lib, symmetry=tables, mirror_loss_coef=1.0, **kw)
    alg.init_storage(16, 24, [45], [263], [12])
    fill_storage(alg, 3, scale=0.3)
    alg.storage.advantages.zero_()          # the surrogate's gradient vanishes: only the mirror term moves the actor
    critic0 = [p.detach().clone() for p in ac.critic.parameters()]
    std0 = ac.std.detach().clone()
    obs = alg.storage.observations.clone()
    before = mirror_gap_of(alg, obs)
    alg.update()
    after = mirror_gap_of(alg, obs)
    print("[mirror loss, %s] L_mirror / coef of the fixed batch: %.4e before, %.4e after 5 epochs; alg.mirror_loss %.4e" % (what, before, after, alg.mirror_loss))
    assert after < before and before * 0.5 < alg.mirror_loss < before * 1.0001
    assert all(torch.equal(a, b.detach()) for a, b in zip(critic0, ac.critic.parameters())) and torch.equal(std0, ac.std.detach())
    return alg


def test_term_lowers_what_it_penalises(tables):
    """One mini-batch of 16 x 24 rows, advantages 0, value and entropy coefficients 0, mirror_loss_coef 1, learning rate 1e-3, 5 epochs: the mean squared gap of the fixed
    batch falls and the critic does not move.  A condition, not a measurement; measured with the eager formulation on the CPU: 1.10e-2 before, 7.1e-3 after."""
    check_term_lowers_the_gap(tables, "cpu", load_oracle(), "eager on the CPU")


# ---- G. flag-off identity ------------------------------------------------------------------------------------------------------------------------------------
def _weights_and_returns(alg, out):
    return torch.cat([p.detach().reshape(-1) for p in alg.actor_critic.parameters()]).numpy().tobytes() + np.asarray(out, np.float64).tobytes() + np.float64(alg.learning_rate).tobytes()


def test_coefficient_zero_is_byte_identical_to_no_argument(tables, host_pair, monkeypatch):
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(6))
    monkeypatch.setattr(torch, "randperm", lambda n_, **kw: perm)
    for mode in ({}, {"use_graphs": "uncaptured", "fused_loss": True}):
        res = []
        for kw in ({}, {"mirror_loss_coef": 0.0}):
            alg = _ppo(tables, **mode, **kw)
            alg.nn_lib = host_pair
            fill_storage(alg, 10)
            torch.manual_seed(20)
            res.append(_weights_and_returns(alg, alg.update()))
            assert alg.mirror_loss_coef == 0.0 and alg.mirror_loss == 0.0 and alg._ml_dev is None
            if mode:
                assert alg._acc.numel() == 2 and alg._aug is not None
        assert res[0] == res[1]
    assert host_pair.mirror_loss_calls == 0


# ---- H. the flag reaches the algorithm -----------------------------------------------------------------------------------------------------------------------
def test_flag_reaches_the_algorithm_through_the_cli_and_the_runner():
    from go2_rl_gym_amd.envs import task_registry
    from go2_rl_gym_amd.utils import get_args
    from go2_rl_gym_amd.utils.helpers import update_cfg_from_args
    _, train_cfg = task_registry.get_cfgs("go2_flat")
    assert train_cfg.algorithm.mirror_loss_coef == 0.0 and train_cfg.algorithm.symmetry is False
    common = ["--num_envs", "8", "--headless", "--sim_device", "cpu", "--rl_device", "cpu"]
    args = get_args(["--task", "go2_flat", *common])
    _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), args)
    assert cfg.algorithm.mirror_loss_coef == 0.0 and cfg.algorithm.symmetry is False
    args = get_args(["--task", "go2_flat", *common, "--mirror_loss", "0.25"])
    _, cfg = update_cfg_from_args(None, copy.deepcopy(train_cfg), args)
    assert cfg.algorithm.mirror_loss_coef == 0.25 and cfg.algorithm.symmetry is True
    env, _ = task_registry.make_env("go2_flat", args, lib=load_oracle())
    runner, _ = task_registry.make_alg_runner(env, "go2_flat", args, train_cfg=cfg, log_root=None)
    alg = runner.alg
    assert alg.mirror_loss_coef == 0.25 and alg._sym is not None
    runner.learn(1, init_at_random_ep_len=True)
    assert all(torch.isfinite(p).all() for p in alg.actor_critic.parameters()) and math.isfinite(alg.mirror_loss) and alg.mirror_loss > 0.0
    env.close()
    args = get_args(["--task", "go2_flat_cts", *common, "--mirror_loss", "0.25"])
    env, _ = task_registry.make_env("go2_flat_cts", args, lib=load_oracle())
    try:
        with pytest.raises(NotImplementedError):
            task_registry.make_alg_runner(env, "go2_flat_cts", args, log_root=None)
    finally:
        env.close()
