"""What tests/test_value_norm_host.py (host build) and tests/test_gpu_value_norm.py (device) share: the cases of go2nn_value_norm_apply / go2nn_value_norm_update /
go2nn_value_head_fold, their numpy and float64 restatements, and the derived bound on the moments (obs_norm_cases.moment_bounds for one column: it bounds ANY summation
order of n terms by (n - 1) 2^-53 sum |t_i|, the block tree of this kernel included).  Everything runs on torch tensors of `device` through go2_rl_gym_amd/_nn.py."""
import math

import numpy as np
import torch

import obs_norm_cases as O
from go2_rl_gym_amd import _nn
from go2_rl_gym_amd.rsl_rl.modules.normalizer import ValueNormalization

GO2NN_EINVAL = -22
ROWS = _nn.GO2NN_VALUE_NORM_ROWS          # elements per block (include/go2nn.h)
NS = [1, 63, 64, 65, 255, 256, 257, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 5]
SENTINEL, PAD = 7.25, 64
U = O.U
FWD = dict(atol=2e-6, rtol=2e-6)          # the forward tolerance of tests/test_policy_kernel.py
bits, stream, sync = O.bits, O.stream, O.sync


def np_normalise(x, stat32):
    """the numpy statement: one fp32 subtraction, one fp32 product, no clamp"""
    y = (x.astype(np.float32) - np.float32(stat32[0])) * np.float32(stat32[2])
    assert y.dtype == np.float32
    return y


def stat_of(mean, var, eps=1e-2):
    sd = math.sqrt(var) + eps
    return np.array([mean, sd, 1.0 / sd]).astype(np.float32)


def make_data(rng, n, loc=20.0, spread=0.5):
    """-> (values, returns) fp32 [n]: returns around `loc` with `spread` (a mean far from zero), -0.0 and a denormal among both"""
    v = (loc + spread * rng.normal(size=n) + 0.3).astype(np.float32)
    r = (loc + spread * rng.normal(size=n)).astype(np.float32)
    for a, k in ((v, 0), (r, 1)):
        a[(3 + k) % n] = -0.0
        if n > 8:
            a[(6 + k) % n] = 1e-45
            a[n - 1 - k] = -0.0
    return v, r


def framed(n, offset, dtype, device, fill=None):
    """-> (a view of n elements that starts `offset` elements behind a 16-byte aligned address, the whole buffer: PAD sentinels in front, the view, PAD behind)"""
    buf = torch.full((PAD + offset + n + PAD,), SENTINEL, dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + offset:PAD + offset + n]
    if fill is not None:
        view.copy_(torch.as_tensor(fill))
    return view, buf


def frame_intact(buf, n, offset):
    return bool((buf[:PAD + offset] == SENTINEL).all().item()) and bool((buf[PAD + offset + n:] == SENTINEL).all().item())


def apply_case(lib, device, n, offset, with_partials, seed=0):
    rng = np.random.default_rng(seed + 7 * n)
    v, r = make_data(rng, n)
    stat = stat_of(19.7, 0.3)
    vt, vbuf = framed(n, offset, torch.float32, device, v)
    rt, rbuf = framed(n, offset, torch.float32, device, r)
    rows = -(-n // ROWS)
    tab, tbuf = framed(rows * 2, 0, torch.float64, device)
    st = torch.from_numpy(stat).to(device)
    assert (vt.data_ptr() % 16 == 0) == (offset == 0)
    _nn.value_norm_apply(lib, vt, rt, st, tab if with_partials else None, stream(device))
    sync(device)
    return dict(n=n, offset=offset, v=v, r=r, stat=stat, got_v=vt.cpu().numpy(), got_r=rt.cpu().numpy(), table=tab.cpu().numpy().reshape(rows, 2), tbuf=tbuf,
                frames=[(vbuf, n), (rbuf, n)], stat_after=st.cpu().numpy())


def check_apply_case(c, with_partials):
    n, offset = c["n"], c["offset"]
    assert np.array_equal(bits(c["got_v"]), bits(np_normalise(c["v"], c["stat"]))), ("values differ from numpy", n, offset)
    assert np.array_equal(bits(c["got_r"]), bits(np_normalise(c["r"], c["stat"]))), ("returns differ from numpy", n, offset)
    assert all(frame_intact(b, m, offset) for b, m in c["frames"]), ("a sentinel was overwritten", n, offset)
    assert np.array_equal(bits(c["stat_after"]), bits(c["stat"]))
    if not with_partials:
        assert bool((c["tbuf"] == SENTINEL).all().item()), "partials = NULL wrote a table"
        return
    assert frame_intact(c["tbuf"], c["table"].size, 0)
    d = c["r"].astype(np.float64) - np.float64(c["stat"][0])
    for b in range(c["table"].shape[0]):
        blk = d[ROWS * b:ROWS * (b + 1)]
        for k, t in ((0, blk), (1, blk * blk)):
            # any order of adding n terms errs by at most (n - 1) 2^-53 sum |t_i| to first order; every d * d is itself rounded once (or fused into the sum): one more
            # 2^-53 sum |t_i|; and one more for the higher-order terms and the reference's own rounding: (n + 1) 2^-53 sum |t_i|.  d is exact (two fp32 numbers in fp64)
            want, bound = math.fsum(t), (len(blk) + 1) * U * np.abs(t).sum()
            assert abs(c["table"][b, k] - want) <= bound, ("partial sums", n, offset, b, k)


# ---- the moments ---------------------------------------------------------------------------------------------------------------------------------------------
class Stream:
    """the normaliser's device buffers driven through the library: one apply over the iteration's returns (in place, with partials), then ONE update"""

    def __init__(self, lib, device, eps=1e-2):
        self.lib, self.device, self.eps = lib, device, eps
        self.state = torch.zeros(3, dtype=torch.float64, device=device)
        self.stat32 = torch.tensor([0.0, 1.0 + eps, 1.0 / (1.0 + eps)], dtype=torch.float32, device=device)

    def iteration(self, returns):
        r = torch.from_numpy(returns).to(self.device).contiguous()
        v = r.clone()
        tab = torch.zeros(-(-r.numel() // ROWS), 2, dtype=torch.float64, device=self.device)
        _nn.value_norm_apply(self.lib, v, r, self.stat32, tab, stream(self.device))
        _nn.value_norm_update(self.lib, tab, self.state, r.numel(), self.eps, self.stat32, stream=stream(self.device))
        sync(self.device)
        return r.cpu().numpy()

    def read(self):
        s = self.state.cpu().numpy()
        return s[0], s[1], s[2] / max(s[0], 1.0), self.stat32.cpu().numpy()


def shifted_returns(rng, steps_list=(1, 3, 24), N=65):
    """three iterations of 1, 3 and 24 steps' worth of N rows, a shifted and rescaled distribution each -> [fp32 [steps * N]]"""
    return [(20.0 * k - 5.0 + (0.5 + 2.0 * k) * rng.normal(size=steps * N)).astype(np.float32) for k, steps in enumerate(steps_list)]


def derived_stat(mean, var, eps):
    sd = np.sqrt(np.float64(var)) + eps
    return np.array([np.float32(mean), np.float32(sd), np.float32(1.0 / sd)])


def check_moments(lib, device, label=""):
    """after each iteration: the state against the pooled two-pass float64 statistics of all samples within obs_norm_cases.moment_bounds; stat32 the fp32 roundings of the
    state; the normalised rows numpy's.  -> the final state's bytes"""
    rng = np.random.default_rng(11)
    st, seen, frozen = Stream(lib, device), [], []
    for k, b in enumerate(shifted_returns(rng)):
        before = st.stat32.cpu().numpy().copy()
        frozen.append(before[:1].copy())
        got = st.iteration(b.copy())
        assert np.array_equal(bits(got), bits(np_normalise(b, before)))
        seen.append(b.reshape(-1, 1))
        count, mean, var, stat32 = st.read()
        ref_mean, ref_var = O.two_pass(np.concatenate(seen))
        b_mean, b_var = O.moment_bounds(seen, frozen)
        e_mean, e_var = abs(mean - ref_mean[0]), abs(var - ref_var[0])
        print("[value norm%s] after iteration %d (%d samples): |mean err| %.3e (bound %.3e), |var err| %.3e (bound %.3e)" % (label, k + 1, int(count), e_mean, b_mean[0], e_var, b_var[0]))
        assert count == sum(s.shape[0] for s in seen)
        assert e_mean <= b_mean[0] and e_var <= b_var[0], (k, e_mean / b_mean[0], e_var / b_var[0])
        assert np.array_equal(bits(stat32), bits(derived_stat(mean, var, st.eps)))
    return st.state.cpu().numpy().tobytes() + st.stat32.cpu().numpy().tobytes()


# ---- the folded critic ---------------------------------------------------------------------------------------------------------------------------------------
CRITICS = {1: [5, 1], 37: [19, 23, 37], 128: [263, 512, 256, 128]}          # K -> input width and hidden widths: a one-unit layer, a ragged small one, the project's critic
FOLD_MEAN, FOLD_STD = -2.9, 3.7          # a missing fold is off by O(1), 10^5 tolerances; small enough that the fp32 rounding of v^ std + mean stays under the tolerance


def make_critic(K, device, seed=0):
    torch.manual_seed(seed + K)
    dims = CRITICS[K]
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
    mods.append(torch.nn.Linear(dims[-1], 1))
    return torch.nn.Sequential(*mods).to(device)


def critic64(critic, x):
    """the critic evaluated in float64 on its fp32 parameters"""
    import copy
    with torch.no_grad():
        return copy.deepcopy(critic).double()(x.double())


def check_fold(lib, device, K, n=70):
    critic = make_critic(K, device)
    x = torch.randn(n, CRITICS[K][0], generator=torch.Generator().manual_seed(K)).to(device)
    stat = torch.tensor([FOLD_MEAN, FOLD_STD, 1.0 / FOLD_STD], dtype=torch.float32, device=device)
    pm = _nn.PackedMlp(lib, critic, fold=stat)
    pm.pack()
    raw = pm.forward(x)
    sync(device)
    with torch.no_grad():
        want = critic(x)
    got = (raw.double() - stat[0].double()) / stat[1].double()
    gap = float((got - want.double()).abs().max())
    print("[value norm] fold K = %d: max |(forward - mean32) / std32 - critic| %.3e; unfolded it would be %.3e" % (K, gap, float((raw.double() - want.double()).abs().max())))
    np.testing.assert_allclose(got.cpu().numpy(), want.double().cpu().numpy(), **FWD)
    assert pm.still_valid()
    plain = _nn.PackedMlp(lib, critic)
    plain.pack()
    np.testing.assert_allclose(plain.forward(x).cpu().numpy(), want.cpu().numpy(), **FWD)          # (and without the option it is the critic, as ever)
    assert float((raw - want).abs().min()) > 0.1          # a missing fold fails by orders of magnitude
    # the fold follows the live parameters and stat32 at the next pack()
    with torch.no_grad():
        critic[-1].bias.add_(0.5)
        stat.copy_(torch.tensor([1.5, 0.25, 4.0]))
    pm.pack()
    with torch.no_grad():
        np.testing.assert_allclose(((pm.forward(x).double() - 1.5) / 0.25).cpu().numpy(), critic(x).double().cpu().numpy(), atol=2e-6, rtol=2e-6)


# ---- output preservation -------------------------------------------------------------------------------------------------------------------------------------
def check_preservation(lib, device, K, label=""):
    """go2nn_value_norm_update with w_last: critic'(x) sigma' + mu' against critic(x) sigma + mu in float64, no further off than 4 x the torch fp32 statement of the same
    rewrite (ValueNormalization.merge(last_layer=...)) plus 2e-6, the rule of tests/test_gpu_obs_norm.py"""
    rng = np.random.default_rng(5 + K)
    x = torch.randn(64, CRITICS[K][0], generator=torch.Generator().manual_seed(3)).to(device)
    returns = (31.0 + 4.0 * rng.normal(size=3 * ROWS + 5)).astype(np.float32)
    gaps, states = {}, {}
    for arm in ("kernel", "torch"):
        critic = make_critic(K, device, seed=9)
        vn = ValueNormalization().to(device)
        vn.set_state(5000.0, 18.0, 2.5)
        old = vn.stat32.double().clone()
        before = critic64(critic, x) * old[1] + old[0]
        w, b = critic[-1].weight, critic[-1].bias
        w0 = w.detach().clone()
        r = torch.from_numpy(returns).to(device)
        if arm == "kernel":
            tab = torch.zeros(-(-r.numel() // ROWS), 2, dtype=torch.float64, device=device)
            _nn.value_norm_apply(lib, r.clone(), r.clone(), vn.stat32, tab, stream(device))
            _nn.value_norm_update(lib, tab, vn.state, r.numel(), vn.eps, vn.stat32, w.detach(), b.detach(), stream(device))
            sync(device)
        else:
            vn.merge(r, (w, b))
        new = vn.stat32.double()
        assert float((new - old).abs()[:2].min()) > 0.1 and not torch.equal(w.detach(), w0)          # the statistics moved, the layer was rewritten
        after = critic64(critic, x) * new[1] + new[0]
        gaps[arm] = float((after - before).abs().max())
        states[arm] = vn.state.cpu().numpy().copy()
    print("[value norm%s] preservation K = %d: raw value moved by %.3e (kernel), %.3e (torch fp32 statement); allowed 4 x torch + 2e-6" % (label, K, gaps["kernel"], gaps["torch"]))
    assert gaps["kernel"] <= 4.0 * gaps["torch"] + 2e-6, gaps
    np.testing.assert_allclose(states["kernel"], states["torch"], rtol=1e-12)
    return gaps


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, device):
    n, K = 5, 7
    v, vbuf = framed(n, 0, torch.float32, device)
    r, rbuf = framed(n, 0, torch.float32, device)
    tab, tbuf = framed(2, 0, torch.float64, device)
    state, sbuf = framed(3, 0, torch.float64, device)
    stat, stbuf = framed(3, 0, torch.float32, device)
    w, wbuf = framed(K, 0, torch.float32, device)
    b, bbuf = framed(1, 0, torch.float32, device)
    wo, wobuf = framed(K, 0, torch.float32, device)
    bo, bobuf = framed(1, 0, torch.float32, device)
    p = lambda t: t.data_ptr()
    s = stream(device)

    def refused(rc):
        sync(device)
        assert rc == GO2NN_EINVAL and len(lib.go2nn_last_error()) > 0
        assert all(bool((x == SENTINEL).all().item()) for x in (vbuf, rbuf, tbuf, sbuf, stbuf, wbuf, bbuf, wobuf, bobuf))

    def apply(values=p(v), returns=p(r), n_=n, stat32=p(stat), partials=p(tab)):
        return lib.go2nn_value_norm_apply(values, returns, n_, stat32, partials, s)

    for k in ("values", "returns", "stat32"):
        refused(apply(**{k: None}))
    for bad in (0, -3):
        refused(apply(n_=bad))
    refused(apply(values=p(v) + 2))          # not aligned to a float

    def update(partials=p(tab), rows=1, state_=p(state), n_=5.0, eps=1e-2, stat32=p(stat), w_last=p(w), b_last=p(b), K_=K):
        return lib.go2nn_value_norm_update(partials, rows, state_, n_, eps, stat32, w_last, b_last, K_, s)

    for k in ("partials", "state_", "stat32"):
        refused(update(**{k: None}))
    for bad in (0, -2):
        refused(update(rows=bad))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(update(n_=bad))
    for bad in (0.0, -1e-2, float("nan"), float("inf")):
        refused(update(eps=bad))
    refused(update(b_last=None))
    for bad in (0, -1):
        refused(update(K_=bad))

    def fold(w_=p(w), b_=p(b), K_=K, stat32=p(stat), w_out=p(wo), b_out=p(bo)):
        return lib.go2nn_value_head_fold(w_, b_, K_, stat32, w_out, b_out, s)

    for k in ("w_", "b_", "stat32", "w_out", "b_out"):
        refused(fold(**{k: None}))
    for bad in (0, -1):
        refused(fold(K_=bad))
    assert lib.go2nn_value_norm_partial_rows(0) == 0 and lib.go2nn_value_norm_partial_rows(-4) == 0
    assert [lib.go2nn_value_norm_partial_rows(m) for m in (1, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 5)] == [1, 1, 1, 2, 4]


# ---- the round trip ------------------------------------------------------------------------------------------------------------------------------------------
def round_trip_ulp(vhat, stat32):
    """((v^ std32 + mean32) - mean32) inv32 against v^, in ulp of v^ (fp32 arithmetic, as every formulation states it)"""
    m, sd, iv = (np.float32(s) for s in stat32)
    raw = vhat.astype(np.float32) * sd + m
    back = (raw - m) * iv
    return np.abs(back.astype(np.float64) - vhat.astype(np.float64)) / np.spacing(np.abs(vhat).astype(np.float32)).astype(np.float64)
