"""The three products of a hidden layer — forward y = act(x W^T + b), input gradient gz_prev = (gz W) * elu'(y_prev) with its column partials, weight gradient dW = gz^T x, and
the fused launch that also leaves the weight gradient of the layer below — through every tile path of go2_rl_gym_amd/csrc/go2nn_bx3.h (split-operand bf16 MFMA) and
go2nn_gemm3.h / go2nn_gemm.h (fp32 MFMA), and the plane image go2nn_split_weights writes, against float64 numpy at the smallest ragged shapes that reach each path.

Every checker is check_*(lib, device, case...): here it runs on the lane-emulation host build (plain loops), where the restatements, the input constructions and the bounds
are shown to be right; tests/test_gpu_gemm_paths.py hands the same checkers the HIP library on cuda:0 and asserts, through go2nn_linear_group_tile_rows and
go2nn_linear_backward_weight_group_kernel, that every case reached the instantiation it is meant for.

Two input families per path.
  EXACT     every partial sum is representable in fp32, so any summation order and any rounding mode give the reference: compared with ==.  Operands and biases are integers in
            [-8, 8], y_prev is drawn from {1, -0.5, -0.75} (ELU' = 1, 0.5, 0.25); every sum stays below 2^24 of its granularity (asserted per case).  Forward with act = 0 is
            exact where the pre-activation is >= 0, the negative outputs go to the bound below.  Two plane-exercising variants, on either operand side: one operand holds
            values with all 24 significand bits set at random (2^-20 .. 2^20), the other exactly one nonzero +-2^e per output column (row), so an output is a scaled copy of one
            input element and needs all three planes of it — lo . hi resp. hi . lo included — to be bit-exact.
  ROUNDING  with S = sum_k |a_k| |b_k| (+ |bias|) per output (carried through column sums and the second product of the fused launch) and e(x) = max |x - ref64| / S:
            e(kernel) <= 4 e(yardstick) + 2^-23, the yardstick being the same product in float32 numpy accumulated one k after the other (column sums one row after the
            other).  Factor and ulp term are those of tests/test_update_rows.py.  The ELU of the yardstick is exp(z) - 1 in float32, the form go2nn.h states for the kernels
            (the hardware exponential): for a pre-activation far below 1 its error is an ulp of 1, not of z, in the kernel and in the yardstick alike.
            Data: N(0, 1); N(0, 1) with rows and columns scaled by powers of two (2^-6 .. 2^6 each, 2^-12 .. 2^12 together); and a plane-coherent set, every operand
            h + m + l with positive planes (below), so that each of the six kept terms has the sign of the main term.
The plane-coherent set closes the gap the old bounds left: on the CPU, with planes() of tests/test_split_planes.py, the product formed from the six kept terms is inside the
bound and the product with ANY ONE of the six terms removed is outside it, for every contraction length COHERENT_K the set is used with (asserted in
test_coherent_set_tells_six_terms_from_five).  Longer contractions are left out of this set only: the yardstick's own error grows with sqrt(K) and from K ~ 64 on four
times it exceeds the mid . mid term (2^-18.6 of the product).  The weight gradient contracts over the M >= 70 rows and therefore has no plane-coherent case.

Passive memory checks: every output, partial-sum workspace and split image lives in a Buf (tests/test_update_rows.py) with sentinels behind it, and in front of it where it
starts at an offset; the gap columns of a pitched output are sentinels that must survive; workspaces start as NaN and exactly the rows the go2nn_*_rows queries report are
summed (go2nn_sum_rows) and must be finite; an optional output handed in as NULL has a sentinel stand-in; every case runs twice and the results are bit-equal.

Measured on the lane-emulation host build (largest e_kernel with the e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound):
  forward, every (M, K, N), act 0 / 1             2.8e-7 (2.8e-7)   0.30   gauss M=150 K=20 N=132 act=0 (192-row case: 0.23)
  forward, outputs on the ELU's negative branch   2.2e-7 (1.1e-7)   0.40   scaled M=192 K=33 N=128 (with the scale S + 1: 8.2e-8 (3.9e-8) 0.30)
  input gradient / its column sums                3.0e-7 (1.9e-7)   0.35   gauss M=150 C=144 Kin=128 ld=131 / 1.9e-7 (1.1e-7) 0.33 scaled M=70 C=4 Kin=45
  fused: gz_prev, column sums / dW below          1.2e-7 (7.6e-8)   0.27   gauss M=1 C=7 Kin=45 Kx=64 / 1.6e-7 (1.2e-7) 0.27
  weight gradient                                 7.7e-7 (6.9e-7)   0.27   scaled M=301 C=40 Kin=128
(with and without a split image the host build runs the same loops: one figure per product)
(the device's figures: tests/test_gpu_gemm_paths.py)"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import load_nn_emu
from test_split_planes import planes
from test_update_rows import F32, F64, PAD, ULP, Buf, dev_in, seqsum, stream_of, sync

from go2_rl_gym_amd._nn import (GO2NN_TM_MAX_FORWARD, GO2NN_TM_MAX_INPUT_GRAD, GO2NN_WGRAD_F32_64x64, GO2NN_WGRAD_F32_64x128, GO2NN_WGRAD_SPLIT_128x128, Go2nnBwdInJob,
                                Go2nnBwdWJob, Go2nnFwdJob, Go2nnSplitJob, Go2nnSumJob)

BX3_BK, BX3_TILE_BYTES = 16, 12288          # go2nn_bx3.h: contraction depth of a k-tile, bytes of one 128-row x 16-k tile of three planes
EXACT = ("int", "bits_a", "bits_b")
ROUNDING = ("gauss", "scaled", "coherent")
COHERENT_K = (4, 7, 16, 20, 33, 48)          # contraction lengths the plane-coherent set is used with (the module docstring says why not the longer ones)
WORST = {}                                    # path -> (share of the bound, e_kernel, e_yardstick, case): the module docstrings' tables are printed from it


def is_device(lib):
    return lib.go2nn_is_device_library() == 1


def adr(buf):
    return buf.ptr.value


def untouched(buf):
    """Buf.untouched() through numpy (a byte image of half a megabyte is compared hundreds of times)"""
    return bool((buf.t.cpu().numpy() == buf.sent).all())


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def full_bits(rng, shape):
    """fp32 values with all 24 significand bits random (the lowest one set), magnitudes 2^-20 .. 2^20, either sign"""
    man = rng.integers(0, 1 << 23, size=shape, dtype=np.int64) | 1
    exp = rng.integers(-20, 21, size=shape)
    return (np.ldexp(1.0 + man / float(1 << 23), exp) * rng.choice([-1.0, 1.0], size=shape)).astype(F32)


def one_hot_rows(rng, rows, cols):
    """[rows, cols] with exactly one nonzero +-2^e (e in -6 .. 6) per row"""
    out = np.zeros((rows, cols), F32)
    out[np.arange(rows), rng.integers(0, cols, size=rows)] = np.ldexp(rng.choice([-1.0, 1.0], size=rows), rng.integers(-6, 7, size=rows))
    return out


def coherent(rng, shape):
    """positive fp32 values whose 24 significand bits are [1 x x 0 0 0 0 0 | 0 1 x x x x x x x | 0 1 x x x x x]: hi = 2^e (1 .. 1.375), the bit below each plane is 0 (so
    bf16 rounding goes DOWN and the next plane is positive), mid = 2^(e-9) (1 .. 2), lo = 2^(e-18) (1 .. 2): with u = mid / (hi 2^-9), v = lo / (hi 2^-17): u in (0.72, 2),
    v in (0.36, 1) — the issue's u, v in [0.5, 1) pushed towards the large side, where a missing term is easier to tell from rounding; e in {-1, 0, 1}"""
    hi = (1 << 23) | (rng.integers(0, 4, size=shape, dtype=np.int64) << 20)
    mid = (1 << 14) | (rng.integers(0, 1 << 7, size=shape, dtype=np.int64) << 7)
    lo = (1 << 5) | rng.integers(0, 1 << 5, size=shape, dtype=np.int64)
    return np.ldexp((hi | mid | lo).astype(F64), rng.integers(-1, 2, size=shape) - 23).astype(F32)


def operands(kind, rng, ra, rb, K, lim=8):
    """A [ra, K], B [rb, K] of the product A B^T (contraction along the last axis of both)"""
    if kind == "int":
        return rng.integers(-lim, lim + 1, size=(ra, K)).astype(F32), rng.integers(-lim, lim + 1, size=(rb, K)).astype(F32)
    if kind == "bits_a":
        return full_bits(rng, (ra, K)), one_hot_rows(rng, rb, K)
    if kind == "bits_b":
        return one_hot_rows(rng, ra, K), full_bits(rng, (rb, K))
    if kind == "gauss":
        return rng.normal(size=(ra, K)).astype(F32), rng.normal(size=(rb, K)).astype(F32)
    if kind == "scaled":
        p2 = lambda n: np.ldexp(1.0, rng.integers(-6, 7, size=n))
        return (rng.normal(size=(ra, K)) * p2(ra)[:, None] * p2(K)).astype(F32), (rng.normal(size=(rb, K)) * p2(rb)[:, None] * p2(K)).astype(F32)
    assert kind == "coherent"
    return coherent(rng, (ra, K)), coherent(rng, (rb, K))


def bias_of(kind, rng, n):
    if kind == "int":
        return rng.integers(-8, 9, size=n).astype(F32)
    if kind in ("bits_a", "bits_b"):
        return np.zeros(n, F32)          # (the output is one scaled input element: nothing may be added to it)
    if kind == "coherent":
        return coherent(rng, n)
    return rng.normal(size=n).astype(F32)


def y_prev_of(kind, rng, shape):
    """the ELU outputs whose derivative multiplies the input gradient: exact family {1, -0.5, -0.75} (ELU' = 1, 0.5, 0.25), else ELU of N(0, 1)"""
    if kind in EXACT:
        return rng.choice(np.array([1.0, -0.5, -0.75], F32), size=shape)
    z = rng.normal(size=shape)
    return np.where(z > 0, z, np.expm1(z)).astype(F32)


# ---- references ------------------------------------------------------------------------------------------------------------------------------------------
def product(a, b, dt):
    """a b^T accumulated one k after the other in dt"""
    a, b = a.astype(dt), b.astype(dt)
    if dt is F64:
        return a @ b.T
    acc = np.zeros((a.shape[0], b.shape[0]), dt)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    return acc


def scale_of(a, b):
    return np.abs(a.astype(F64)) @ np.abs(b.astype(F64)).T


def elu_as_stated(z, dt):
    """go2nn.h: ELU through the exponential, exp(z) - 1"""
    z = np.asarray(z, dt)
    with np.errstate(over="ignore"):
        return np.where(z > 0, z, np.exp(np.minimum(z, dt(0))) - dt(1.0)).astype(dt)


def elu_prime(y, dt):
    y = y.astype(dt)
    return np.where(y > 0, dt(1.0), y + dt(1.0))


def within_s(path, tag, got, yard, ref, S):
    """e_kernel <= 4 e_yardstick + 2^-23 with e(x) = max |x - ref| / S componentwise; where S = 0 the output is 0"""
    got, yard, ref, S = (np.asarray(v, F64).reshape(-1) for v in (got, yard, ref, S))
    assert np.isfinite(got).all(), (path, tag)
    nz = S > 0
    assert (got[~nz] == 0).all(), (path, tag)
    if not nz.any():
        return
    ek, ey = float((np.abs(got - ref)[nz] / S[nz]).max()), float((np.abs(yard - ref)[nz] / S[nz]).max())
    share = ek / (4 * ey + ULP)
    print("[gemm_paths] %s | %s: e_kernel %.3e e_yardstick %.3e (of bound: %.2f)" % (path, tag, ek, ey, share))
    if share > WORST.get(path, (-1.0,))[0]:
        WORST[path] = (share, ek, ey, tag)
    assert ek <= 4 * ey + ULP, (path, tag, ek, ey)


def exact(path, tag, got, ref, peak):
    """peak: the largest sum of magnitudes, in units of the data's granularity — below 2^24 every partial sum of every summation order is an fp32 number"""
    assert peak < 2.0 ** 24, (path, tag, peak)
    got, ref = np.asarray(got, F64).reshape(-1), np.asarray(ref, F64).reshape(-1)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (path, tag, "%d of %d differ, first at %d: %r != %r" % (bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]]))


def same_bits(a, b):
    """the outputs of two calls, bit for bit (the sentinels around them are each call's own check)"""
    return all(np.array_equal(x.get().view(np.uint8), y.get().view(np.uint8)) for x, y in zip(a, b))


def expect_tile_rows(lib, M, n0, n1, tm_max, want):
    got = lib.go2nn_linear_group_tile_rows(M, n0, n1, tm_max)
    assert got == (want if is_device(lib) else 0), ("tile rows", M, n0, n1, tm_max, got, want)


def split_image(lib, device, w, N, K):
    """-> Buf holding the split image of w [N, K] (sentinels behind it), filled by go2nn_split_weights"""
    n = lib.go2nn_split_weights_bytes(N, K)
    assert n == image_bytes(N, K) + image_bytes(K, N), lib.go2nn_last_error()
    img = Buf(device, int(n), dtype=torch.uint8)
    sj = (Go2nnSplitJob * 1)(Go2nnSplitJob(w.data_ptr(), adr(img), N, K))
    assert lib.go2nn_split_weights(sj, 1, stream_of(device)) == 0, lib.go2nn_last_error()
    return img


def sum_rows(lib, device, part, out, nrows, ncols):
    job = (Go2nnSumJob * 1)(Go2nnSumJob(adr(part), adr(out), nrows, ncols))
    assert lib.go2nn_sum_rows(job, 1, stream_of(device)) == 0, lib.go2nn_last_error()


def col_sums(x, dt):
    return seqsum(np.asarray(x, dt), dt)


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------------------
FWD_M = {70: 64, 129: 128, 150: 128, 191: 128, 192: 128}          # rows -> rows per workgroup tile of the split-operand launch (bx3_tm's tie at 129 .. 192 rows: 3 / 768 = 2 / 512)
FWD_N = (33, 128, 130, 132)
FWD_K = (4, 7, 16, 20, 33, 48, 64, 70, 80, 144)          # < 16: no pipelined loop; 16: one whole tile; 20 / 33 / 70: ragged last tile; 48 .. 144: both staging depths, past the unroll group


def forward_pairs():
    """every (K, N) of FWD_K x FWD_N once, two to a launch: a launch's jobs differ in K AND in N (the fp32 twin then also meets groups whose jobs pick different tiles)"""
    combos = [(K, N) for i, K in enumerate(FWD_K) for N in FWD_N[i % 4:] + FWD_N[:i % 4]]
    half = len(combos) // 2
    return [(combos[i], combos[half + i]) for i in range(half)]


def run_forward(lib, device, M, data, act, split, y_front, held):
    """held: the device copies of the inputs and the split images, made by the first of a case's two calls"""
    jobs, keep = (Go2nnFwdJob * len(data))(), []
    ys, imgs = [], []
    for k, (x, w, b) in enumerate(data):
        if k not in held:
            t = [dev_in(v, device) for v in (x, w, b)]
            held[k] = (t, split_image(lib, device, t[1], w.shape[0], w.shape[1]) if split else None)
        t, img = held[k]
        y = Buf(device, M * w.shape[0], front=y_front)
        jobs[k] = Go2nnFwdJob(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), adr(y), M, w.shape[1], w.shape[0], act, adr(img) if split else None)
        keep.append(t); ys.append(y); imgs.append(img)
    assert lib.go2nn_linear_elu_forward_group(jobs, len(data), stream_of(device)) == 0, lib.go2nn_last_error()
    sync(device)
    for img in imgs:
        if img is not None:
            assert img.intact() and (is_device(lib) or untouched(img))          # (the host build's products read the fp32 weights: the image is not written)
    return ys


def check_forward(lib, device, M, shapes, act, split, kind, want_rows=None, y_front=0):
    """shapes: (K, N) of the launch's one or two jobs"""
    rng = np.random.default_rng([M, act, EXACT.index(kind) if kind in EXACT else 3 + ROUNDING.index(kind)] + [v for s in shapes for v in s])
    data = []
    for K, N in shapes:
        x, w = operands(kind, rng, M, N, K)
        data.append((x, w, bias_of(kind, rng, N)))
    if split and want_rows is not None:
        expect_tile_rows(lib, M, shapes[0][1], shapes[1][1] if len(shapes) == 2 else 0, GO2NN_TM_MAX_FORWARD, want_rows)
    held = {}
    ys = run_forward(lib, device, M, data, act, split, y_front, held)
    again = run_forward(lib, device, M, data, act, split, y_front, held)
    assert same_bits(ys, again), "not bit-equal from call to call"
    path = "forward %s %s" % ("split" if split else "fp32", "rows/tile %s" % want_rows if split else "")
    for (K, N), (x, w, b), y in zip(shapes, data, ys):
        tag = "%s M=%d K=%d N=%d act=%d front=%d" % (kind, M, K, N, act, y_front)
        assert y.intact(), (tag, "sentinels around y")
        got = y.get().reshape(M, N)
        z64 = product(x, w, F64) + b.astype(F64)
        S = scale_of(x, w) + np.abs(b.astype(F64))
        ref = z64 if act else elu_as_stated(z64, F64)
        neg = (z64 < 0) & (not act)          # the ELU's exponential branch
        if kind in EXACT:
            exact(path, tag, got[~neg], ref[~neg], float(S.max()) if kind == "int" else 0.0)
            yard = elu_as_stated(z64.astype(F32), F32)          # (the pre-activation is exact: the yardstick's error is its exponential's)
        else:
            z32 = product(x, w, F32) + b
            yard = z32 if act else elu_as_stated(z32, F32)
            within_s(path, tag, got[~neg], yard[~neg], ref[~neg], S[~neg])
        if neg.any():
            within_s(path + " ELU < 0", tag, got[neg], yard[neg], ref[neg], S[neg])
            # exp(z) - 1 rounds at the scale of its two terms, not of z: with the 1 counted into the scale like |bias| the same bound also holds outputs whose S is tiny
            within_s(path + " ELU < 0, scale S + 1", tag, got[neg], yard[neg], ref[neg], S[neg] + 1.0)


# ---- input gradient --------------------------------------------------------------------------------------------------------------------------------------
IG_M = {70: 64, 150: 128, 129: 128}
IG_C = (4, 7, 20, 48, 144)
IG_KIN = (33, 45, 128, 130)
IG_PITCHED = [(20, 128, 388, 128), (48, 130, 131, 0), (7, 128, 388, 128), (144, 128, 131, 2)]          # (C, Kin, ld, column offset): a block of a wider matrix; a pitch that is no multiple of 4


def input_grad_pairs():
    combos = [(C_, Kin) for i, C_ in enumerate(IG_C) for Kin in IG_KIN[i % 4:] + IG_KIN[:i % 4]]
    half = len(combos) // 2
    return [((combos[i] + (0, 0)), (combos[half + i] + (0, 0))) for i in range(half)] + [(IG_PITCHED[0], IG_PITCHED[1]), (IG_PITCHED[2], IG_PITCHED[3])]


def fp32_serves(plain, C_, Kin, ld):
    """go2nn_linear_backward_input_group without w_split: a width that is no multiple of 4 goes to the single-network kernels, which know neither `plain` nor a pitch"""
    return Kin % 4 == 0 or (not plain and not ld)


def run_input_grad(lib, device, M, data, plain, split, held):
    jobs, keep, outs = (Go2nnBwdInJob * len(data))(), [], []
    for k, (gz, w, yp, ld, off) in enumerate(data):
        C_, Kin = w.shape
        pitch = ld if ld else Kin
        if k not in held:
            t = [dev_in(gz, device), dev_in(w, device), dev_in(yp, device)]
            held[k] = (t, split_image(lib, device, t[1], C_, Kin) if split else None)
        t, img = held[k]
        gzp = Buf(device, M * pitch)                                    # all sentinels: the gap columns of a pitched job stay that way
        r = lib.go2nn_linear_backward_input_group_rows(M, C_, Kin)
        assert r > 0, lib.go2nn_last_error()
        ws = Buf(device, r * Kin, None if plain else float("nan"))      # plain: not read, not written (a stand-in)
        jobs[k] = Go2nnBwdInJob(t[0].data_ptr(), t[1].data_ptr(), None if plain else t[2].data_ptr() + 4 * off, adr(gzp) + 4 * off, adr(ws), M, C_, Kin, plain,
                                adr(img) if split else None, ld)
        keep.append(t); outs.append([gzp, ws, r, img])
    assert lib.go2nn_linear_backward_input_group(jobs, len(data), stream_of(device)) == 0, lib.go2nn_last_error()
    for (gz, w, yp, ld, off), o in zip(data, outs):
        gb = Buf(device, w.shape[1])
        if not plain:
            sum_rows(lib, device, o[1], gb, o[2], w.shape[1])
        o.append(gb)
    sync(device)
    return outs


def check_input_grad(lib, device, M, shapes, plain, split, kind, want_rows=None):
    """shapes: (C, Kin, ld, column offset) of the launch's one or two jobs"""
    rng = np.random.default_rng([M, plain, 7, EXACT.index(kind) if kind in EXACT else 3 + ROUNDING.index(kind)] + [v for s in shapes for v in s])
    data = []
    for C_, Kin, ld, off in shapes:
        gz, wt = operands(kind, rng, M, Kin, C_)          # gz [M, C], W^T [Kin, C]
        yp = y_prev_of(kind, rng, (M, ld if ld else Kin))
        data.append((gz, np.ascontiguousarray(wt.T), yp, ld, off))
    if split and want_rows is not None:
        expect_tile_rows(lib, M, shapes[0][1], shapes[1][1] if len(shapes) == 2 else 0, GO2NN_TM_MAX_INPUT_GRAD, want_rows)
    held = {}
    outs = run_input_grad(lib, device, M, data, plain, split, held)
    again = run_input_grad(lib, device, M, data, plain, split, held)
    assert same_bits([b for o in outs for b in (o[0], o[4])], [b for o in again for b in (o[0], o[4])]), "not bit-equal from call to call"
    path = "input gradient %s %s" % ("split" if split else "fp32", "rows/tile %s" % want_rows if split else "")
    for (C_, Kin, ld, off), (gz, w, yp, _, _), (gzp, ws, r, img, gb) in zip(shapes, data, outs):
        tag = "%s M=%d C=%d Kin=%d plain=%d ld=%d+%d" % (kind, M, C_, Kin, plain, ld, off)
        pitch = ld if ld else Kin
        full = gzp.get().reshape(M, pitch)
        got, gap = full[:, off:off + Kin], np.delete(full, np.s_[off:off + Kin], axis=1)
        assert gzp.intact() and (gap == gzp.sent).all(), (tag, "sentinels around gz_prev or in the gap columns of its pitch")
        assert ws.intact() and gb.intact() and (img is None or img.intact()), (tag, "sentinels behind the column partials")
        f64 = F64(1.0) if plain else elu_prime(yp[:, off:off + Kin], F64)
        f32 = F32(1.0) if plain else elu_prime(yp[:, off:off + Kin], F32)
        ref, S = product(gz, w.T, F64) * f64, scale_of(gz, w.T) * np.abs(f64)
        if plain:
            assert ws.untouched() and gb.untouched(), tag
        else:
            assert np.isfinite(ws.get()).all(), tag          # exactly the reported rows were written
        if kind in EXACT:
            exact(path, tag, got, ref, 4.0 * float(S.max()) if kind == "int" else 0.0)
            if not plain and kind == "int":
                exact(path + " column sums", tag, gb.get(), ref.sum(0), 4.0 * float(S.sum(0).max()))
            elif not plain:          # (exact elements of any magnitude: their column sums round)
                within_s(path + " column sums", tag, gb.get(), col_sums(ref.astype(F32), F32), ref.sum(0), S.sum(0))
            continue
        yard = product(gz, w.T, F32) * f32
        within_s(path, tag, got, yard, ref, S)
        if not plain:
            within_s(path + " column sums", tag, gb.get(), col_sums(yard, F32), ref.sum(0), S.sum(0))


# ---- the fused launch: input gradient + the weight gradient of the layer below (EPI_DELU_WG) ----------------------------------------------------------------
FUSED_SHAPES = [(70, 96, 40, 45, 48, True), (130, 37, 70, 64, 7, False), (257, 8, 33, 33, 32, True), (128, 64, 128, 1, 45, False),          # tests/test_mlp_tail.py: BELOW_SHAPES
                (129, 20, 130, 33, 64, False), (129, 48, 130, 1, 32, True), (1, 7, 45, 64, 33, True), (1, 16, 128, 32, 1, False)]          # M, C, Kin, Kx of job 0 / 1, gz_prev stored


FUSED_EXACT = ("int", "bits_gp", "bits_x")
FUSED_KINDS = lambda C_: FUSED_EXACT + ("gauss", "scaled") + (("coherent",) if C_ in COHERENT_K else ())


def run_fused(lib, device, M, data, keep_gz, held):
    jobs, keep, outs = (Go2nnBwdInJob * len(data))(), [], []
    rows = lib.go2nn_linear_backward_input_fused_rows(M)
    assert rows > 0, lib.go2nn_last_error()
    for k, (gz, w, yp, xw, x0, kx) in enumerate(data):
        C_, Kin = w.shape
        if k not in held:
            t = [dev_in(v, device) for v in (gz, w, yp, xw)]
            held[k] = (t, split_image(lib, device, t[1], C_, Kin))
        t, img = held[k]
        r = lib.go2nn_linear_backward_input_group_rows(M, C_, Kin)
        gzp = Buf(device, M * Kin)          # keep_gz False: NULL goes to the kernel and this stand-in stays untouched
        ws, dws = Buf(device, r * Kin, float("nan")), Buf(device, rows * Kin * kx, float("nan"))
        jobs[k] = Go2nnBwdInJob(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), adr(gzp) if keep_gz else None, adr(ws), M, C_, Kin, 0, adr(img), 0, kx,
                                t[3].data_ptr() + 4 * x0, adr(dws), xw.shape[1] if xw.shape[1] != kx else 0)
        keep.append(t); outs.append([gzp, ws, dws, img, r])
    assert lib.go2nn_linear_backward_input_group(jobs, len(data), stream_of(device)) == 0, lib.go2nn_last_error()
    for (gz, w, yp, xw, x0, kx), o in zip(data, outs):
        gb, dw = Buf(device, w.shape[1]), Buf(device, w.shape[1] * kx)
        sum_rows(lib, device, o[1], gb, o[4], w.shape[1])
        sum_rows(lib, device, o[2], dw, rows, w.shape[1] * kx)
        o += [gb, dw]
    sync(device)
    return outs


def check_fused(lib, device, M, C_, Kin, kx0, kx1, keep_gz, kind):
    """two jobs; job 1's x_in is columns [3, 3 + Kx) of a matrix 5 columns wider (Go2nnBwdInJob.ldx)"""
    rng = np.random.default_rng([M, C_, Kin, kx0, kx1, (FUSED_EXACT + ROUNDING).index(kind)])
    lim = 4 if kind == "int" else 8          # (two products in a row: 16 C . 8 M . 4 stays below 2^24 at every shape of FUSED_SHAPES)
    data = []
    for k, kx in enumerate((kx0, kx1)):
        wide, x0 = (kx + 5, 3) if k else (kx, 0)
        if kind == "bits_gp":          # gz_prev[m, k] = a scaled copy of one element of gz (24 bits), x_in one nonzero +-2^e per column: dW_below[k, j] = a scaled copy of gz_prev[m_j, k]
            gz, wt = operands("bits_a", rng, M, Kin, C_)
            xw = np.ascontiguousarray(one_hot_rows(rng, wide, M).T)
        elif kind == "bits_x":         # gz_prev = +-2^e in ONE row, x_in with all 24 bits: dW_below[k, j] = a scaled copy of x_in[m0, j]
            gz, wt = np.zeros((M, C_), F32), np.ldexp(rng.choice([-1.0, 1.0], size=(Kin, C_)), rng.integers(-6, 7, size=(Kin, C_))).astype(F32)
            gz[rng.integers(0, M), rng.integers(0, C_)] = 4.0
            xw = full_bits(rng, (M, wide))
        else:
            gz, wt = operands(kind, rng, M, Kin, C_, lim)
            xw = coherent(rng, (M, wide)) if kind == "coherent" else rng.integers(-8, 9, size=(M, wide)).astype(F32) if kind == "int" else rng.normal(size=(M, wide)).astype(F32)
        yp = y_prev_of("int" if kind in FUSED_EXACT else kind, rng, (M, Kin))
        data.append((gz, np.ascontiguousarray(wt.T), yp, xw, x0, kx))
    held = {}
    outs = run_fused(lib, device, M, data, keep_gz, held)
    again = run_fused(lib, device, M, data, keep_gz, held)
    assert same_bits([b for o in outs for b in (o[0], o[5], o[6])], [b for o in again for b in (o[0], o[5], o[6])]), "not bit-equal from call to call"
    path = "fused input gradient + weight gradient below"
    for (gz, w, yp, xw, x0, kx), (gzp, ws, dws, img, r, gb, dw) in zip(data, outs):
        tag = "%s M=%d C=%d Kin=%d Kx=%d ldx=%d gz_prev=%d" % (kind, M, C_, Kin, kx, xw.shape[1], keep_gz)
        assert all(b.intact() for b in (gzp, ws, dws, img, gb, dw)), (tag, "sentinels")
        assert np.isfinite(ws.get()).all() and np.isfinite(dws.get()).all(), tag
        x = xw[:, x0:x0 + kx]
        ref = product(gz, w.T, F64) * elu_prime(yp, F64)
        S = scale_of(gz, w.T) * np.abs(elu_prime(yp, F64))
        rdw, Sdw = ref.T @ x.astype(F64), S.T @ np.abs(x.astype(F64))
        if not keep_gz:
            assert gzp.untouched(), tag
        if kind in FUSED_EXACT:
            peak = (lambda v: 4.0 * float(v.max())) if kind == "int" else (lambda v: 0.0)
            if keep_gz:
                exact(path + " gz_prev", tag, gzp.get(), ref, peak(S))
            if kind != "bits_gp":          # (bits_x: one nonzero per column)
                exact(path + " column sums", tag, gb.get(), ref.sum(0), peak(S.sum(0)))
            exact(path + " dW below", tag, dw.get(), rdw, peak(Sdw))
            continue
        yard = product(gz, w.T, F32) * elu_prime(yp, F32)
        if keep_gz:
            within_s(path + " gz_prev", tag, gzp.get(), yard, ref, S)
        within_s(path + " column sums", tag, gb.get(), col_sums(yard, F32), ref.sum(0), S.sum(0))
        within_s(path + " dW below", tag, dw.get(), product(yard.T, x.T, F32), rdw, Sdw)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------------------------
# (M, [(C, Kin, ldx, float offset of gz, of x)] per job, split asked for, kernel, slices): VECA needs an even C and gz on 8 bytes, VECB Kin a multiple of the lane's piece
# (4 floats for 64 x 128 tiles, 2 for 64 x 64) and x aligned to it — the four variants of either tile shape; the split-operand kernel takes C = 512 (whole 128-row tiles, 16 tiles)
WGRAD_CASES = [
    (70, [(40, 128, 0, 0, 0), (40, 256, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x128, 8),          # VECA VECB; 8 slices of 16 rows, three of them wholly past M
    (301, [(37, 128, 0, 0, 0), (37, 256, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x128, 8),         # odd C: VECB only
    (301, [(40, 128, 0, 0, 1), (40, 256, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x128, 8),         # x 4 bytes past 16: VECA only
    (70, [(37, 256, 0, 1, 1), (37, 128, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x128, 8),          # neither
    (70, [(40, 46, 0, 0, 0), (40, 264, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x64, 8),            # VECA VECB
    (301, [(40, 45, 0, 0, 0), (40, 263, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x64, 8),           # odd Kin: VECA only
    (301, [(37, 46, 0, 0, 0), (37, 264, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x64, 8),           # odd C: VECB only
    (70, [(40, 45, 0, 1, 0), (37, 263, 0, 0, 1)], 0, GO2NN_WGRAD_F32_64x64, 8),            # neither (gz 4 bytes past 8, odd Kin)
    (70, [(512, 130, 0, 0, 0), (512, 250, 0, 0, 0)], 1, GO2NN_WGRAD_SPLIT_128x128, 8),     # 8 slices of 16 rows, three of them wholly past M; columns beyond Kin: the out-of-range buffer offset
    (1000, [(512, 130, 0, 0, 0), (512, 250, 0, 0, 0)], 1, GO2NN_WGRAD_SPLIT_128x128, 8),
    (1001, [(512, 130, 0, 0, 0), (512, 250, 0, 0, 0)], 1, GO2NN_WGRAD_SPLIT_128x128, 8),    # the last slice ends inside a k-tile
    (1001, [(512, 130, 135, 0, 0), (512, 250, 255, 0, 1)], 1, GO2NN_WGRAD_SPLIT_128x128, 8),          # x pitched: ldx = Kin + 5
    (70, [(512, 130, 0, 0, 0), (512, 250, 0, 0, 0)], 0, GO2NN_WGRAD_F32_64x64, 8),         # the same group without the split flag
]


WGRAD_KINDS = lambda M: ("int", "bits_a", "bits_b", "gauss", "scaled") if M < 1000 else ("int", "bits_a", "bits_b", "gauss")


def run_wgrad(lib, device, M, data, split):
    jobs, keep, outs = (Go2nnBwdWJob * len(data))(), [], []
    for k, (gz, xw, Kin, ldx, goff, xoff) in enumerate(data):
        tg, tx = Buf(device, gz.size, gz, front=goff), Buf(device, xw.size, xw, front=xoff)
        jobs[k] = Go2nnBwdWJob(adr(tg), adr(tx), None, M, gz.shape[1], Kin, split, ldx)
        keep += [tg, tx]
    ns, rps = C.c_int32(-1), C.c_int32(-1)
    kern = lib.go2nn_linear_backward_weight_group_kernel(jobs, len(data), C.byref(ns), C.byref(rps))
    rows = lib.go2nn_linear_backward_weight_group_rows(jobs, len(data))
    assert rows > 0 and kern >= 0 and ns.value == rows, lib.go2nn_last_error()
    for k, (gz, xw, Kin, ldx, goff, xoff) in enumerate(data):
        ws = Buf(device, rows * gz.shape[1] * Kin, float("nan"))
        jobs[k].workspace = adr(ws)
        outs.append([ws])
    assert lib.go2nn_linear_backward_weight_group(jobs, len(data), stream_of(device)) == 0, lib.go2nn_last_error()
    for (gz, xw, Kin, ldx, goff, xoff), o in zip(data, outs):
        dw = Buf(device, gz.shape[1] * Kin)
        sum_rows(lib, device, o[0], dw, rows, gz.shape[1] * Kin)
        o.append(dw)
    sync(device)
    return outs, kern, rows, rps.value


def check_wgrad(lib, device, M, shapes, split, want_kernel, want_slices, kind):
    rng = np.random.default_rng([M, split, EXACT.index(kind) if kind in EXACT else 3 + ROUNDING.index(kind)] + [v for s in shapes for v in s])
    data = []
    for C_, Kin, ldx, goff, xoff in shapes:
        gt, xt = operands(kind, rng, C_, ldx if ldx else Kin, M)          # gz^T [C, M], x^T [ldx, M]: the contraction runs over the rows
        data.append((np.ascontiguousarray(gt.T), np.ascontiguousarray(xt.T), Kin, ldx, goff, xoff))
    outs, kern, rows, rps = run_wgrad(lib, device, M, data, split)
    again = run_wgrad(lib, device, M, data, split)[0]
    assert same_bits([o[1] for o in outs], [o[1] for o in again]), "not bit-equal from call to call"
    if is_device(lib):
        assert (kern, rows) == (want_kernel, want_slices) and rows * rps >= M, (kern, rows, rps)
        if (M, want_kernel) in ((70, GO2NN_WGRAD_SPLIT_128x128), (70, GO2NN_WGRAD_F32_64x128)):
            assert rps == 16          # three of the 8 slices start at row 80 or later
    else:
        assert (kern, rows) == (0, 1)
    path = "weight gradient %s" % {GO2NN_WGRAD_SPLIT_128x128: "split 128x128", GO2NN_WGRAD_F32_64x128: "fp32 64x128", GO2NN_WGRAD_F32_64x64: "fp32 64x64"}[want_kernel]
    for (C_, Kin, ldx, goff, xoff), (gz, xw, _, _, _, _), (ws, dw) in zip(shapes, data, outs):
        tag = "%s M=%d C=%d Kin=%d ldx=%d offsets=%d,%d" % (kind, M, C_, Kin, ldx, goff, xoff)
        assert ws.intact() and dw.intact() and np.isfinite(ws.get()).all(), (tag, "sentinels behind the slices' partials, or a partial that was not written")
        x = xw[:, :Kin]
        ref, S = gz.astype(F64).T @ x.astype(F64), scale_of(gz.T, x.T)
        if kind in EXACT:          # bits_a: x has one nonzero +-2^e per column, so dW[c, k] is a scaled copy of one element of gz (all 24 bits); bits_b: the other way round
            exact(path, tag, dw.get(), ref, float(S.max()) if kind == "int" else 0.0)
        else:
            within_s(path, tag, dw.get(), product(gz.T, x.T, F32), ref, S)


# ---- the split image ---------------------------------------------------------------------------------------------------------------------------------------
IMAGE_SHAPES = [(1, 1), (33, 7), (128, 16), (130, 20), (300, 45)]          # (N, K)


def image_bytes(rows, con):
    return ((rows + 127) // 128) * ((con + BX3_BK - 1) // BX3_BK) * BX3_TILE_BYTES


def decode_image(img, rows, con):
    """go2nn_bx3.h: [row tile of 128][k tile of 16][plane][row][chunk ^ ((row >> 3) & 1)][8 bf16] -> three [128 row tiles, 16 k tiles] matrices of bf16 bit patterns"""
    nrt, nkt = (rows + 127) // 128, (con + BX3_BK - 1) // BX3_BK
    a = np.frombuffer(np.ascontiguousarray(img).tobytes(), np.uint16).reshape(nrt, nkt, 3, 128, 2, 8)
    swap = ((np.arange(128) >> 3) & 1) == 1
    a = np.where(swap[None, None, None, :, None, None], a[:, :, :, :, ::-1, :], a)
    return a.transpose(2, 0, 3, 1, 4, 5).reshape(3, nrt * 128, nkt * 16)


def image_values(n):
    """the values of test_three_bf16_planes_hold_every_bit_of_an_fp32_value: N(0, 9), +-2^-60 .. 2^60, ties of the bf16 rounding, +-0"""
    rng = np.random.default_rng(0)
    special = np.array([-(1.0 + 2.0 ** -8 + 2.0 ** -16), 0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0e38, -3.0e38, 2.0 ** -100, 0.1, 255.5, 256.0 - 2.0 ** -15, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], F32)
    x = np.concatenate([special, (rng.standard_normal(n) * 3).astype(F32), (np.exp2(rng.uniform(-60, 60, n)) * rng.choice([-1, 1], n)).astype(F32)])
    return np.concatenate([special, rng.permutation(x[special.size:])])[:n]


def check_split_image(lib, device, shape_a, shape_b):
    """two jobs in one launch"""
    ws, imgs, jobs = [], [], (Go2nnSplitJob * 2)()
    for k, (N, K) in enumerate((shape_a, shape_b)):
        w = image_values(N * K).reshape(N, K)
        n = lib.go2nn_split_weights_bytes(N, K)
        assert n == image_bytes(N, K) + image_bytes(K, N)
        t, img = dev_in(w, device), Buf(device, int(n), dtype=torch.uint8)
        assert img.t.numel() == n + PAD          # the sentinels stand right behind go2nn_split_weights_bytes
        jobs[k] = Go2nnSplitJob(t.data_ptr(), adr(img), N, K)
        ws.append((w, t)); imgs.append(img)
    assert lib.go2nn_split_weights(jobs, 2, stream_of(device)) == 0, lib.go2nn_last_error()
    sync(device)
    for (N, K), (w, _), img in zip((shape_a, shape_b), ws, imgs):
        assert img.intact(), (N, K)
        if not is_device(lib):
            assert untouched(img)          # the host build returns without writing: its products read the fp32 weights
            continue
        raw = img.get()
        for tr, (m, rows, con) in enumerate(((w, N, K), (np.ascontiguousarray(w.T), K, N))):
            got = decode_image(raw[tr * image_bytes(N, K):][:image_bytes(rows, con)], rows, con)
            h, mid, lo, rest = planes(m)
            assert (rest == 0).all()
            want = np.zeros_like(got)
            for p, v in enumerate((h, mid, lo)):
                want[p, :rows, :con] = (bits(v) >> 16).astype(np.uint16)
                assert (bits(v) & 0xffff == 0).all()
            assert np.array_equal(got[:, :rows, :con], want[:, :rows, :con]), ("plane bits", N, K, tr)
            pad = got.copy(); pad[:, :rows, :con] = 0
            assert (pad == 0).all(), ("beyond the matrix", N, K, tr)
            val = (got.astype(np.uint32) << 16).view(F32).astype(F64)
            assert np.array_equal(val[:, :rows, :con].sum(0), m.astype(F64)), ("hi + mid + lo", N, K, tr)


# ---- on the host build -------------------------------------------------------------------------------------------------------------------------------------
KINDS = EXACT + ROUNDING


def kinds_for(K):
    return [k for k in KINDS if k != "coherent" or K in COHERENT_K]


def forward_case(lib, device, M, act, split, want_rows):
    for pair in forward_pairs():
        for kind in KINDS:
            jobs = [s for s in pair if kind in kinds_for(s[0])]
            if jobs:
                check_forward(lib, device, M, jobs, act, split, kind, want_rows)
    if not act and not split:
        check_forward(lib, device, M, [(3, 33), (2, 130)], act, split, "int")          # K < 4 without an image: the single-network kernels
        check_forward(lib, device, M, [(3, 33), (2, 130)], act, split, "gauss")


def input_grad_case(lib, device, M, plain, split, want_rows):
    for pair in input_grad_pairs():
        for kind in KINDS:
            jobs = [s for s in pair if kind in kinds_for(s[0]) and (split or fp32_serves(plain, *s[:3]))]
            # (without an image a group of which one job needs the single-network kernels takes every job there: such widths are launched on their own)
            for launch in ([[s] for s in jobs] if not split and any(s[1] % 4 for s in jobs) else [jobs] if jobs else []):
                check_input_grad(lib, device, M, launch, plain, split, kind, want_rows)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", sorted(FWD_M))
def test_forward(M, act, split):
    forward_case(load_nn_emu(), "cpu", M, act, split, FWD_M[M])


def test_forward_unaligned_output():
    for kind in ("int", "gauss"):
        check_forward(load_nn_emu(), "cpu", 150, [(20, 132), (48, 128)], 0, True, kind, 128, y_front=1)


def test_forward_two_jobs_on_the_xcd_interleave():
    for kind in ("int", "gauss"):
        check_forward(load_nn_emu(), "cpu", 70, [(20, 512), (48, 500)], 0, True, kind, 64)


@pytest.mark.parametrize("K,act", [(20, 0), (7, 1)])
def test_forward_192_row_tiles(K, act):
    for kind in ("int", "gauss"):
        check_forward(load_nn_emu(), "cpu", 1537, [(K, 2500), (K, 2557)], act, True, kind, 192)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("M", sorted(IG_M))
def test_input_gradient(M, plain, split):
    input_grad_case(load_nn_emu(), "cpu", M, plain, split, IG_M[M])


@pytest.mark.parametrize("M,C_,Kin,kx0,kx1,keep_gz", FUSED_SHAPES)
def test_fused_weight_gradient_below(M, C_, Kin, kx0, kx1, keep_gz):
    for kind in FUSED_KINDS(C_):
        check_fused(load_nn_emu(), "cpu", M, C_, Kin, kx0, kx1, keep_gz, kind)


@pytest.mark.parametrize("M,shapes,split,kernel,slices", WGRAD_CASES)
def test_weight_gradient(M, shapes, split, kernel, slices):
    for kind in WGRAD_KINDS(M):
        check_wgrad(load_nn_emu(), "cpu", M, shapes, split, kernel, slices, kind)


@pytest.mark.parametrize("k", range(len(IMAGE_SHAPES)))
def test_split_image_is_left_alone_by_the_host_build(k):
    check_split_image(load_nn_emu(), "cpu", IMAGE_SHAPES[k], IMAGE_SHAPES[(k + 1) % len(IMAGE_SHAPES)])


# ---- the constructions themselves ----------------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_what_they_claim():
    assert sorted({s for p in forward_pairs() for s in p}) == sorted((K, N) for K in FWD_K for N in FWD_N)
    assert all(a[0] != b[0] and a[1] != b[1] for a, b in forward_pairs())
    ig = {s[:2] for p in input_grad_pairs() for s in p if not s[2]}
    assert ig == {(C_, Kin) for C_ in IG_C for Kin in IG_KIN} and {s for p in input_grad_pairs() for s in p if s[2]} == set(IG_PITCHED)
    assert any(s[2] % 4 for s in IG_PITCHED) and any(s[3] for s in IG_PITCHED)
    assert {c[3] for c in WGRAD_CASES} == {GO2NN_WGRAD_F32_64x64, GO2NN_WGRAD_F32_64x128, GO2NN_WGRAD_SPLIT_128x128}
    assert {(m, kx) for m, _, _, a, b, _ in FUSED_SHAPES for kx in (a, b)} >= {(129, 1), (129, 32), (129, 33), (129, 64), (1, 1), (1, 32), (1, 33), (1, 64)}
    assert {g for *_, g in FUSED_SHAPES} == {True, False}


def test_input_constructions():
    rng = np.random.default_rng(3)
    x = full_bits(rng, (64, 33))
    assert (bits(x) & 1 == 1).all() and (np.abs(x) >= 2.0 ** -20).all() and (np.abs(x) < 2.0 ** 21).all()
    assert (planes(x)[1] != 0).mean() > 0.98 and (planes(x)[2] != 0).mean() > 0.98          # all three planes carry bits (but for a few values whose middle bits are all 0)
    o = one_hot_rows(rng, 50, 7)
    assert ((o != 0).sum(1) == 1).all() and (np.abs(np.log2(np.abs(o[o != 0]))) <= 6).all() and (np.log2(np.abs(o[o != 0])) % 1 == 0).all()
    a, b = operands("bits_a", rng, 20, 9, 33)
    assert np.array_equal(product(a, b, F64), product(a, b, F32))          # a scaled copy of one element: exact in fp32
    c = coherent(rng, (300, 40))
    h, m, l, rest = (v.astype(F64) for v in planes(c))
    assert (rest == 0).all() and (h > 0).all() and (m > 0).all() and (l > 0).all() and np.array_equal(h + m + l, c.astype(F64))
    u, v = m / (h * 2.0 ** -9), l / (h * 2.0 ** -17)
    assert u.min() > 0.72 and u.max() < 2 and v.min() > 0.36 and v.max() < 1
    y = y_prev_of("int", rng, (40, 9))
    assert set(np.unique(elu_prime(y, F32))) == {0.25, 0.5, 1.0}
    g, w = operands("scaled", rng, 400, 300, 64)
    assert np.log2(np.abs(g).max() / np.abs(g[g != 0]).min()) > 12          # the scaling spreads the magnitudes over more than the 2^12 the bf16 planes span twice
    assert np.allclose(elu_as_stated(np.array([-1.0, 0.0, 2.0]), F64), [np.expm1(-1.0), 0.0, 2.0])


@pytest.mark.parametrize("K", COHERENT_K)
def test_coherent_set_tells_six_terms_from_five(K):
    """on the plane-coherent set the product formed from the six kept terms is inside the bound of this file, and with any one of the six removed it is outside"""
    rng = np.random.default_rng(K)
    a, b = coherent(rng, (150, K)), coherent(rng, (132, K))
    pa, pb = [v.astype(F64) for v in planes(a)[:3]], [v.astype(F64) for v in planes(b)[:3]]
    terms = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]          # go2nn_bx3.h: hi hi + hi mid + mid hi + mid mid + hi lo + lo hi
    ref, S = product(a, b, F64), scale_of(a, b)
    bound = 4 * float((np.abs(product(a, b, F32) - ref) / S).max()) + ULP
    e = lambda got: float((np.abs(got - ref) / S).max())
    six = sum(pa[i] @ pb[j].T for i, j in terms)
    assert e(six) <= bound, (K, e(six), bound)
    for drop in terms:
        five = sum(pa[i] @ pb[j].T for i, j in terms if (i, j) != drop)
        assert e(five) > bound, (K, drop, e(five), bound)
        assert float((np.abs(five - ref) / S).min()) > bound, (K, drop)          # EVERY output shows it, so a term lost in one tile or one k-tail cannot hide


def test_measured_table_is_printed():
    """(runs last in this file) the largest share of the bound per path over the cases above"""
    for path in sorted(WORST):
        share, ek, ey, tag = WORST[path]
        print("[gemm_paths table] %-48s %.1e (%.1e)   %.2f   %s" % (path, ek, ey, share, tag))
