"""The rollout's policy kernels — go2nn_mlp3_kernel (go2_rl_gym_amd/csrc/go2nn_mlp3.h: split-bf16 planes, weight ring, clamped duplicate tile), go2nn_mlp_kernel with nn_finish
(go2nn_impl.cpp: fp32 MFMA) and go2nn_pack_kernel — through the four entry points they serve (go2nn_mlp_forward, go2nn_mlp_forward_rows, go2nn_policy_act,
go2nn_policy_act_latent), called through the C ABI with ctypes (Go2nnMlp, Go2nnMlpIO: pointers, pitches and NULLs are the test's own), against float64 numpy at the smallest shapes
that reach each ring, tile, staging and head path.

Every checker is check_*(lib, device, case...): here it runs on the host build (helpers.load_nn_emu: the fp32 kernel's order restated in plain loops), where the restatements, the
input constructions and the bounds are shown to be right; tests/test_gpu_policy_paths.py hands the same checkers the HIP library on cuda:0.  describe() of go2nn_impl.cpp is restated
below (NT, KV3, ring, KB3, nn3_pitch, the even / odd LDS regions against 163840 bytes): CLAIMS holds, per network shape, whether it fits the LDS as planes and the (NT, KV3, KB3)
per layer it is meant to reach; the restatement is held against CLAIMS here and against go2nn_packed_floats / go2nn_mlp_arith in every case.

Input families (inputs, helpers and bound are those of tests/test_gemm_paths.py).
  EXACT     compared with == against float64.
            int     one layer: integers in [-8, 8].  Several layers: inputs, hidden weights and hidden biases are non-negative integers (first layer dense, middle layers two ones
                    per row), so every hidden pre-activation is >= 0 and the ELU is the identity; the last layer is signed, its magnitude chosen so that the carried scale S stays
                    below 2^24 (asserted per case).  The first hidden layer exceeds 256: the epilogue's split has a nonzero mid plane.
            int20   the same with half of the first hidden biases in [2^19, 2^20) (20-bit hidden values: a nonzero lo plane in the epilogue's split — round-to-nearest planes
                    hold 17-bit integers in hi + mid), one one per middle-layer row and four nonzeros per last-layer row.
            bits_x  x = positive values with all 24 significand bits, hidden weight rows one-hot +2^e, last layer one-hot +-2^e, no bias: an output is a scaled copy of one input
                    element that went through the staging split and every epilogue split (all three activation planes, lo . hi included).
            bits_w  x one-hot +2^e per row, first layer 24-bit values, later layers one-hot: pins the three weight planes of the packed image and hi . lo.
  ROUNDING  e(kernel) <= 4 e(yardstick) + 2^-23 with e(x) = max |x - ref64| / S; the yardstick is the same network in float32 numpy, one k after the other, ELU as exp(z) - 1;
            S is carried through the layers, S_0 = |x|, S_l = |W_l| S_(l-1) + |b_l| (the ELU is 1-Lipschitz).  Log-probability: S = the sum of the absolute terms of its row;
            normalised output: S / the float64 norm.  Data: gauss (N(0, 1), weights / sqrt(K)); scaled (rows and columns of x and of every W times powers of two, 2^-6 .. 2^6 for
            one layer, 2^-3 .. 2^3 for several: the ELU's own 1 does not scale with S); coherent (one layer, K in COHERENT_K: every operand h + m + l with positive planes —
            test_coherent_set_tells_six_terms_from_five shows the six kept terms inside the bound and every five outside it, in this kernel's form: last layer, bias, no ELU).

Bit-equalities: a_out == a_st == add(mu, mul(std, eps)); sig_st == std; mu_st / v_st == go2nn_mlp_forward of actor / critic; policy_act_latent == policy_act on the concatenated
input; forward_rows(rows = NULL, one segment) == mlp_forward; a permutation in `rows` permutes the output rows; input rows r == r mod 32 at 289 rows give every workgroup the
outputs of workgroup 0 (the rotation of tile ownership changes nothing); a second launch equals the first.
Passive memory checks: every output and the packed image live in a Buf with sentinels behind it; gap columns of pitched inputs are NaN, of pitched outputs sentinels; rows outside
`rows` stay sentinels; an optional output handed in as NULL has a sentinel stand-in; the packed image starts as NaN.

Measured on the host build (largest e_kernel with the e_yardstick of its case; largest share e_kernel / (4 e_yardstick + 2^-23) of the bound):
  forward / forward_rows(NULL), one layer        3.8e-7 (3.1e-7)   0.28   coherent (48, 7) rows=33
  forward / forward_rows(NULL), several layers   9.6e-8 (7.7e-8)   0.23   scaled (64, 288, 1) rows=33
  forward_rows: staging, pitches, out widths     3.4e-7 (3.2e-7)   0.24   scaled (17, 500)
    ... normalised                               8.2e-7 (8.2e-7)   0.24   scaled (17, 512)
    ... two networks / the normalised one        1.1e-8 (1.3e-8)   0.06 / 1.4e-7 (1.4e-7) 0.21   gauss (129, 288, 7) 97 rows / int20 (65, 300, 33) 33 rows
  policy_act mu / value                          1.4e-7 (1.3e-7)   0.22 / 6.0e-8 (6.0e-8) 0.17   scaled, N=257
  policy_act log-probability                     3.9e-4 (3.9e-4)   0.25   scaled A=12 N=257 (|mu| up to 2^9 sigma: the rounding of the sample a = mu + std eps is the whole error,
                                                                          in the kernel and the yardstick alike; with integer mu up to 2^24: 2.9e-3 (2.9e-3) 0.25)
With S carried through several layers the yardstick's own e is far below 2^-23 (gauss, the tasks' networks: 1e-10), so there the ulp term is the bound: the exact families are the
sharp check of the deep networks, the rounding families of the one-layer ones.
(the device's figures: tests/test_gpu_policy_paths.py)"""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import load_nn_emu
from test_gemm_paths import COHERENT_K, WORST, bits, coherent, elu_as_stated, exact, full_bits, is_device, one_hot_rows, product, within_s
from test_split_planes import planes
from test_update_rows import F32, F64, ULP, Buf, dev_in, seqsum, stream_of, sync

from go2_rl_gym_amd._nn import Go2nnMlp, Go2nnMlpIO

GO2NN_EINVAL, MAX_LAYERS, MAX_WIDTH = -22, 6, 512
NN_ROWS, NN_WAVES, NN3_LDS = 32, 8, 163840          # go2nn_impl.cpp: rows per workgroup, waves per workgroup, the planes kernel's LDS
HALF_LOG2PI = F32(0.9189385332046727)
FP32_ONLY = os.environ.get("GO2_GEMM_SPLIT", "1") == "0"          # the library reads it once per process
EXACT = ("int", "int20", "bits_x", "bits_w")
ROUNDING = ("gauss", "scaled", "coherent")


# ---- describe() of go2nn_impl.cpp, restated ------------------------------------------------------------------------------------------------------------------
def nn3_pitch(width):
    return (width + 31) // 32 * 64 + 16


class Desc:
    def __init__(self, dims):
        K, N = list(dims[:-1]), list(dims[1:])
        self.dims, self.nl, self.K, self.N = tuple(dims), len(N), K, N
        self.NT, self.KB, self.KV3 = [(n + 31) // 32 for n in N], [(k + 31) // 32 * 4 for k in K], [(k + 15) // 16 for k in K]
        self.ring = [4 if nt > NN_WAVES else 8 for nt in self.NT]
        self.KB3 = [(kv + r - 1) // r * r for kv, r in zip(self.KV3, self.ring)]
        off, self.woff, self.boff, self.woff3 = 0, [], [], []
        for l in range(self.nl):
            self.woff.append(off); off += self.NT[l] * self.KB[l] * 256
            self.boff.append(off); off += self.NT[l] * 32
        for l in range(self.nl):
            self.woff3.append(off); off += self.NT[l] * self.KB3[l] * 768
        self.total = off
        reg = [0, 0]
        for l in range(self.nl):
            reg[l & 1] = max(reg[l & 1], 3 * NN_ROWS * nn3_pitch(16 * self.KV3[0] if l == 0 else 32 * self.NT[l - 1]))
        reg[self.nl & 1] = max(reg[self.nl & 1], NN_ROWS * (32 * self.NT[-1] + 4) * 4)
        self.lds, self.fits = reg[0] + reg[1], reg[0] + reg[1] <= NN3_LDS
        self.paths = list(zip(self.NT, self.KV3, self.KB3))


# dims -> (LDS bytes or None, fits, per-layer (NT, KV3, KB3) or None): what each case is meant to reach
SIX = (30, 24, 24, 24, 24, 24, 5)
CLAIMS = {
    (512, 320, 12): (162816, True, [(10, 32, 32), (1, 20, 24)]),          # the LDS fit with 1 KB to spare
    (512, 352, 12): (168960, False, None),
    (480, 512): (159744, True, [(16, 30, 32)]),                           # last layer with 16 tiles: NTW = 2 fp32 store
    (496, 512): (165888, False, None),
    (512, 480): (161792, True, None),                                     # widest fitting one-layer shape
    (320, 512, 320, 1): (162816, True, None),
    (129, 288, 7): (None, True, [(9, 9, 12), (1, 18, 24)]),               # NTW = 2, odd NT = 9: 7 waves hold a clamped duplicate tile; three trips, zero blocks
    (64, 288, 1): (None, True, [(9, 4, 4), (1, 18, 24)]),                 # NTW = 2, KV3 == R == 4: only the LAST trip
    (65, 300, 33): (None, True, [(10, 5, 8), (2, 19, 24)]),               # KV3 = R + 1; the second output tile has one live column
    (128, 40, 24, 12): (None, True, [(2, 8, 8), (1, 3, 8), (1, 2, 8)]),   # NTW = 1, KV3 == R, one trip
    (17, 33): (None, True, [(2, 2, 8)]),                                  # one layer: the last-layer fp32 epilogue only
    (1, 1): (None, True, [(1, 1, 8)]),
    SIX: (None, True, [(1, 2, 8)] * 6),                                   # GO2NN_MAX_LAYERS: both regions reused three times
    (45, 512, 256, 128, 12): (None, True, None),                          # the tasks' own networks
    (263, 512, 256, 128, 1): (None, True, None),
    (300, 512, 512, 12): (None, False, None),
    (512, 512): (None, False, None),
}
PLANE_SHAPES = [d for d, c in CLAIMS.items() if c[1]]
FALLBACK_SHAPES = [(512, 352, 12), (496, 512), (300, 512, 512, 12)]
FP32_CHILD_SHAPES = [(17, 33), (129, 288, 7), (65, 300, 33), (128, 40, 24, 12), SIX]


def claim(dims):
    """the restatement against what the case claims; -> Desc"""
    d = Desc(dims)
    if tuple(dims) in CLAIMS:
        lds, fits, paths = CLAIMS[tuple(dims)]
        assert d.fits == fits and (lds is None or d.lds == lds) and (paths is None or d.paths == paths), (dims, d.lds, d.fits, d.paths)
    return d


def want_arith(d):
    return 3 if d.fits and not FP32_ONLY else 1


# ---- a network on the device -----------------------------------------------------------------------------------------------------------------------------------
def mlp_struct(dims, wts, bts, num_layers=None):
    m = Go2nnMlp()
    m.num_layers = len(dims) - 1 if num_layers is None else num_layers
    for i, v in enumerate(dims[:MAX_LAYERS + 1]):
        m.dims[i] = v
    for l, (w, b) in enumerate(zip(wts, bts)):
        m.weight[l], m.bias[l] = w.data_ptr(), b.data_ptr()
    return m


class Net:
    """weights on the device, the Go2nnMlp that points at them, the packed image (NaN before go2nn_pack, sentinels behind it)"""

    def __init__(self, lib, device, Ws, bs):
        self.Ws, self.bs = [np.ascontiguousarray(W, F32) for W in Ws], [np.ascontiguousarray(b, F32) for b in bs]
        self.dims = (self.Ws[0].shape[1],) + tuple(W.shape[0] for W in self.Ws)
        self.d = claim(self.dims)
        self.wt, self.bt = [dev_in(W, device) for W in self.Ws], [dev_in(b, device) for b in self.bs]
        self.m = mlp_struct(self.dims, self.wt, self.bt)
        n = lib.go2nn_packed_floats(C.byref(self.m))
        assert n == self.d.total, (self.dims, n, self.d.total, lib.go2nn_last_error())
        self.packed = Buf(device, int(n), float("nan"))
        assert lib.go2nn_pack(C.byref(self.m), self.packed.ptr, stream_of(device)) == 0, lib.go2nn_last_error()
        sync(device)
        assert self.packed.intact(), (self.dims, "sentinels behind the packed image")
        self.arith = lib.go2nn_mlp_arith(C.byref(self.m))
        assert self.arith == (want_arith(self.d) if is_device(lib) else 0), (self.dims, self.arith)


def launch_name(lib, nets):
    """run() of go2nn_impl.cpp: a launch runs planes only if every network of it reports 3"""
    if not is_device(lib):
        return "host"
    return "planes" if all(n.arith == 3 for n in nets) else "fp32"


def adr(buf):
    return buf.ptr.value if buf is not None else None


def run_forward(lib, device, net, xt, nrows):
    y = Buf(device, nrows * net.dims[-1])
    assert lib.go2nn_mlp_forward(C.byref(net.m), net.packed.ptr, xt.data_ptr(), y.ptr, nrows, stream_of(device)) == 0, lib.go2nn_last_error()
    sync(device)
    assert y.intact(), (net.dims, "sentinels behind y")
    return y


def run_rows(lib, device, nets, ios):
    """ios: per network dict(x, x2, rows, y, ldx, ldx2, kx, nrows, ldy, normalize) of device tensors / Bufs"""
    n = len(nets)
    mp = (C.POINTER(Go2nnMlp) * n)(*[C.pointer(t.m) for t in nets])
    pk = (C.c_void_p * n)(*[adr(t.packed) for t in nets])
    io = (Go2nnMlpIO * n)()
    for k, q in enumerate(ios):
        io[k] = Go2nnMlpIO(q["x"].data_ptr(), q["x2"].data_ptr() if q.get("x2") is not None else None, q["rows"].data_ptr() if q.get("rows") is not None else None, adr(q["y"]),
                           q["ldx"], q.get("ldx2", 0), q["kx"], q["nrows"], q["ldy"], q.get("normalize", 0))
    rc = lib.go2nn_mlp_forward_rows(mp, pk, io, n, stream_of(device))
    sync(device)
    return rc


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------------
def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(F32)


def few(rng, N, K, c, signed_lim=0):
    """[N, K] with min(c, K) nonzeros per row at distinct places: ones, or integers of either sign in 1 .. signed_lim"""
    c = min(c, K)
    idx = rng.random((N, K)).argsort(1)[:, :c]
    v = np.ones((N, c)) if not signed_lim else rng.integers(1, signed_lim + 1, size=(N, c)) * rng.choice([-1.0, 1.0], size=(N, c))
    out = np.zeros((N, K), F32)
    out[np.arange(N)[:, None], idx] = v
    return out


def carried_scale(x, Ws, bs):
    S = np.abs(x.astype(F64))
    for W, b in zip(Ws, bs):
        S = S @ np.abs(W.astype(F64)).T + np.abs(b.astype(F64))
    return S


def make_case(kind, rng, dims, nrows):
    """-> x [nrows, dims[0]], weights, biases"""
    nl = len(dims) - 1
    p2 = lambda n, lim: np.ldexp(1.0, rng.integers(-lim, lim + 1, size=n))
    Ws, bs = [], []
    if kind in ("int", "int20"):
        x = ints(rng, -8, 8, (nrows, dims[0])) if nl == 1 else ints(rng, 0, 8, (nrows, dims[0]))
    elif kind == "bits_x":
        x = np.abs(full_bits(rng, (nrows, dims[0])))
    elif kind == "bits_w":
        x = np.abs(one_hot_rows(rng, nrows, dims[0]))
    elif kind == "coherent":
        x = coherent(rng, (nrows, dims[0]))
    elif kind == "gauss":
        x = (1.5 * rng.normal(size=(nrows, dims[0]))).astype(F32)
    else:
        lim = 6 if nl == 1 else 3
        x = (rng.normal(size=(nrows, dims[0])) * p2(nrows, lim)[:, None] * p2(dims[0], lim)).astype(F32)
    for l in range(nl):
        K, N, first, last = dims[l], dims[l + 1], l == 0, l == nl - 1
        if kind in ("int", "int20"):
            if nl == 1:
                W, b = ints(rng, -8, 8, (N, K)), ints(rng, -8, 8, N)
            elif first:
                W, b = ints(rng, 0, 8 if K <= 128 else 2, (N, K)), ints(rng, 0, 8, N)
                if kind == "int20":
                    b[::2] += ints(rng, 1 << 19, (1 << 20) - 9, b[::2].shape)
            elif not last:
                W, b = few(rng, N, K, 2 if kind == "int" else 1), ints(rng, 0, 8, N)
            else:
                nnz = K if kind == "int" else min(4, K)
                hmax = float(carried_scale(x, Ws, bs).max())
                lim = int(min(8, (2 ** 24 - 9) // (nnz * hmax)))
                assert lim >= 1, (dims, kind, hmax)
                W, b = few(rng, N, K, nnz, lim), ints(rng, -8, 8, N)
        elif kind in ("bits_x", "bits_w"):
            if kind == "bits_w" and first:
                W = full_bits(rng, (N, K)) if last else np.abs(full_bits(rng, (N, K)))
            else:
                W = one_hot_rows(rng, N, K) if last else np.abs(one_hot_rows(rng, N, K))
            b = np.zeros(N, F32)
        elif kind == "coherent":
            W, b = coherent(rng, (N, K)), coherent(rng, N)
        elif kind == "gauss":
            W, b = (rng.normal(size=(N, K)) / np.sqrt(K)).astype(F32), (0.1 * rng.normal(size=N)).astype(F32)
        else:
            lim = 6 if nl == 1 else 3
            W = (rng.normal(size=(N, K)) / np.sqrt(K) * p2(N, lim)[:, None] * p2(K, lim)).astype(F32)
            b = (0.1 * rng.normal(size=N) * p2(N, lim)).astype(F32)
        Ws.append(W); bs.append(b)
    return x, Ws, bs


def kinds_for(dims):
    nl = len(dims) - 1
    return [k for k in EXACT + ROUNDING if (k != "coherent" or (nl == 1 and dims[0] in COHERENT_K)) and (k != "int20" or nl > 1)]


# ---- references --------------------------------------------------------------------------------------------------------------------------------------------------
def reference(x, Ws, bs, yardstick=True):
    """-> the network in float64, in float32 numpy one k after the other (ELU as exp(z) - 1), the carried scale S"""
    h64, h32 = x.astype(F64), x.astype(F32)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        last = l == len(Ws) - 1
        z64 = h64 @ W.astype(F64).T + b.astype(F64)
        h64 = z64 if last else elu_as_stated(z64, F64)
        if yardstick:
            z32 = product(h32, W, F32) + b
            h32 = z32 if last else elu_as_stated(z32, F32)
    return h64, (h32 if yardstick else None), carried_scale(x, Ws, bs)


def normalised(y, S, dt):
    """F.normalize: y / max(|y|, 1e-12) along the last axis; the scale divided by the float64 norm"""
    y = y.astype(dt)
    if dt is F64:
        nrm = np.sqrt((y * y).sum(1))
        return y / np.maximum(nrm, 1e-12)[:, None], np.where(nrm[:, None] > 0, S / np.where(nrm > 0, nrm, 1.0)[:, None], 0.0)
    inv = F32(1.0) / np.maximum(np.sqrt(seqsum((y * y).T, F32)), F32(1e-12))
    return y * inv[:, None], None


def compare(path, tag, kind, got, x, Ws, bs, normalize=0):
    ref, yard, S = reference(x, Ws, bs, kind not in EXACT or normalize)
    if normalize:
        yard = normalised(yard, None, F32)[0]
        ref, S = normalised(ref, S, F64)
        within_s(path + " normalised", tag, got, yard, ref, S)
    elif kind in EXACT:
        exact(path, tag, got, ref, float(S.max()) if kind in ("int", "int20") else 0.0)
    else:
        within_s(path, tag, got, yard, ref, S)


# ---- go2nn_mlp_forward, and go2nn_mlp_forward_rows in its plain form ------------------------------------------------------------------------------------------------
def check_forward(lib, device, dims, kind, nrows):
    rng = np.random.default_rng(list(dims) + [nrows, (EXACT + ROUNDING).index(kind)])
    x, Ws, bs = make_case(kind, rng, dims, nrows)
    net = Net(lib, device, Ws, bs)
    xt = dev_in(x, device)
    y, again = run_forward(lib, device, net, xt, nrows), run_forward(lib, device, net, xt, nrows)
    assert same(y.get(), again.get()), (dims, kind, "not bit-equal from call to call")
    yr = Buf(device, nrows * dims[-1])
    assert run_rows(lib, device, [net], [dict(x=xt, y=yr, ldx=dims[0], kx=dims[0], nrows=nrows, ldy=dims[-1])]) == 0, lib.go2nn_last_error()
    assert yr.intact() and same(y.get(), yr.get()), (dims, kind, "forward_rows(rows = NULL, one segment) != mlp_forward")
    path = "policy forward %s, %s" % (launch_name(lib, [net]), "one layer" if len(dims) == 2 else "several layers")
    compare(path, "%s %s rows=%d" % (kind, dims, nrows), kind, y.get().reshape(nrows, dims[-1]), x, Ws, bs)


def check_same_rows(lib, device, dims, nrows=289):
    """input row r = row r mod 32: every workgroup computes what workgroup 0 does, each with another rotation of the tiles' owners"""
    rng = np.random.default_rng(list(dims) + [nrows])
    x, Ws, bs = make_case("gauss", rng, dims, NN_ROWS)
    net = Net(lib, device, Ws, bs)
    xt = dev_in(x[np.arange(nrows) % NN_ROWS], device)
    y = run_forward(lib, device, net, xt, nrows).get().reshape(nrows, dims[-1])
    assert same(y, y[np.arange(nrows) % NN_ROWS]), (dims, "a workgroup's outputs differ from workgroup 0's")
    compare("policy forward %s, %s" % (launch_name(lib, [net]), "one layer" if len(dims) == 2 else "several layers"), "gauss %s rows r = r mod 32" % (dims,), "gauss", y[:NN_ROWS], x, Ws, bs)


# ---- staging: segments, pitches, row lists --------------------------------------------------------------------------------------------------------------------------
STAGING_IN = (1, 2, 45, 127, 128, 129, 255, 257, 512)          # lane pairs and the four 128-column quads
STAGING_OUT = 33


def kx_options(in_dim):
    """one column, an odd split (a lane's pair straddles the two segments), all but one column, one segment"""
    return sorted({k for k in (1, (in_dim // 2) | 1, in_dim - 1, in_dim) if 1 <= k <= in_dim})


def segments(x, kx, rng, device):
    """x [M, in_dim] as two pitched matrices with NaN in the gap columns -> io fields"""
    M, K = x.shape
    ldx, ldx2 = kx + 3, K - kx + 5
    a = np.full((M, ldx), np.nan, F32); a[:, :kx] = x[:, :kx]
    q = dict(x=dev_in(a, device), ldx=ldx, kx=kx)
    if kx < K:
        b = np.full((M, ldx2), np.nan, F32); b[:, :K - kx] = x[:, kx:]
        q.update(x2=dev_in(b, device), ldx2=ldx2)
    return q


def row_lists(rng, nrows, extra=7):
    """-> (rows or None, number of input rows): NULL, a permutation, a strict subset of a larger input matrix"""
    return [(None, nrows), (rng.permutation(nrows).astype(np.int32), nrows), (rng.permutation(nrows + extra)[:nrows].astype(np.int32), nrows + extra)]


def check_staging(lib, device, in_dim, kind, nrows=37):
    dims = (in_dim, STAGING_OUT)
    rng = np.random.default_rng([in_dim, nrows, EXACT.index(kind)])
    _, Ws, bs = make_case(kind, rng, dims, 1)
    net = Net(lib, device, Ws, bs)
    path = "policy forward_rows %s" % launch_name(lib, [net])
    for kx, (rows, M) in itertools.product(kx_options(in_dim), row_lists(rng, nrows)):
        x = make_case(kind, rng, dims, M)[0]
        ldy = STAGING_OUT + 3
        y = Buf(device, M * ldy)
        q = segments(x, kx, rng, device)
        q.update(y=y, nrows=nrows, ldy=ldy, rows=None if rows is None else dev_in(rows, device))
        assert run_rows(lib, device, [net], [q]) == 0, lib.go2nn_last_error()
        tag = "%s in=%d kx=%d rows=%s of %d" % (kind, in_dim, kx, "NULL" if rows is None else "list", M)
        full = y.get().reshape(M, ldy)
        used = np.arange(nrows) if rows is None else rows
        assert y.intact() and (full[:, STAGING_OUT:] == y.sent).all() and (np.delete(full, used, axis=0) == y.sent).all(), (tag, "sentinels in the gap columns / unused rows")
        compare(path, tag, kind, full[used, :STAGING_OUT], x[used], Ws, bs)


def check_permutation(lib, device, dims, nrows):
    """a permutation in `rows` permutes the output rows and changes no bit"""
    rng = np.random.default_rng(list(dims) + [nrows, 11])
    x, Ws, bs = make_case("gauss", rng, dims, nrows)
    net = Net(lib, device, Ws, bs)
    xt = dev_in(x, device)
    y = run_forward(lib, device, net, xt, nrows).get().reshape(nrows, dims[-1])
    perm = rng.permutation(nrows).astype(np.int32)
    yp = Buf(device, nrows * dims[-1])
    assert run_rows(lib, device, [net], [dict(x=xt, y=yp, ldx=dims[0], kx=dims[0], nrows=nrows, ldy=dims[-1], rows=dev_in(perm, device))]) == 0, lib.go2nn_last_error()
    assert yp.intact() and same(yp.get().reshape(nrows, dims[-1]), y), (dims, nrows)          # row perm[i] is written at row perm[i]: the same matrix
    # and the same input rows in another order: the outputs move with them
    yq = run_forward(lib, device, net, dev_in(x[perm], device), nrows).get().reshape(nrows, dims[-1])
    assert same(yq, y[perm]), (dims, nrows, "a row's output depends on its place in the workgroup")


def check_two_networks(lib, device, dims_a, dims_b, nrows_a, nrows_b, kind):
    """one launch, two networks on row subsets of different sizes: whole workgroups of the smaller one leave; the second one normalises"""
    rng = np.random.default_rng(list(dims_a) + list(dims_b) + [nrows_a, nrows_b, (EXACT + ROUNDING).index(kind)])
    M = max(nrows_a, nrows_b) + 5
    nets, ios, keep = [], [], []
    for dims, nrows, norm in ((dims_a, nrows_a, 0), (dims_b, nrows_b, 1)):
        x, Ws, bs = make_case(kind, rng, dims, M)
        net = Net(lib, device, Ws, bs)
        rows = rng.permutation(M)[:nrows].astype(np.int32)
        y = Buf(device, M * dims[-1])
        q = segments(x, kx_options(dims[0])[1], rng, device)
        q.update(y=y, nrows=nrows, ldy=dims[-1], rows=dev_in(rows, device), normalize=norm)
        nets.append(net); ios.append(q); keep.append((x, Ws, bs, rows, y, norm, dims))
    assert run_rows(lib, device, nets, ios) == 0, lib.go2nn_last_error()
    path = "policy forward_rows %s, two networks" % launch_name(lib, nets)
    for x, Ws, bs, rows, y, norm, dims in keep:
        full = y.get().reshape(M, dims[-1])
        assert y.intact() and (np.delete(full, rows, axis=0) == y.sent).all(), (dims, "rows outside the list")
        compare(path, "%s %s rows=%d" % (kind, dims, len(rows)), kind, full[rows], x[rows], Ws, bs, norm)


NORMALIZE_OUT = (1, 32, 33, 500, 512)          # the row scale is parked at column out_dim of the tile: 512 is its edge


def check_normalize(lib, device, out_dim, normalize, kind, nrows=35, in_dim=17):
    """ldy > out_dim with sentinels in the gap; `int` has no bias and one zero input row: its output is exactly zero and stays zero under normalize"""
    dims = (in_dim, out_dim)
    rng = np.random.default_rng([out_dim, normalize, (EXACT + ROUNDING).index(kind)])
    x, Ws, bs = make_case(kind, rng, dims, nrows)
    if kind == "int":
        bs[0][:] = 0; x[nrows // 2] = 0
    net = Net(lib, device, Ws, bs)
    ldy = out_dim + 3
    y = Buf(device, nrows * ldy)
    assert run_rows(lib, device, [net], [dict(x=dev_in(x, device), y=y, ldx=in_dim, kx=in_dim, nrows=nrows, ldy=ldy, normalize=normalize)]) == 0, lib.go2nn_last_error()
    full = y.get().reshape(nrows, ldy)
    assert y.intact() and (full[:, out_dim:] == y.sent).all(), (dims, "sentinels in the gap columns")
    if kind == "int":
        assert (full[nrows // 2, :out_dim] == 0).all(), (dims, normalize, "a zero row")
    compare("policy forward_rows %s" % launch_name(lib, [net]), "%s %s normalize=%d" % (kind, dims, normalize), kind, full[:, :out_dim], x, Ws, bs, normalize)


# ---- the heads: go2nn_policy_act, go2nn_policy_act_latent -------------------------------------------------------------------------------------------------------------
OPTIONAL = ("a_st", "mu_st", "sig_st", "lp_st", "v_st")


def logp_restated(mu, std, eps, dt):
    """-> log-probability, sum of the absolute terms.  float64: the exact sample mu + std eps; float32: the kernel's two rounded operations, j ascending"""
    std_, eps_ = std.astype(dt), eps.astype(dt)
    if dt is F64:
        d = std_ * eps_
    else:
        d = (mu.astype(F32) + std_ * eps_) - mu.astype(F32)
    t0, t1 = (d * d) / (dt(2.0) * std_ * std_), np.log(std_) + np.zeros_like(d)
    terms = -t0 - t1 - dt(HALF_LOG2PI)
    return seqsum(terms.T, dt), (np.abs(t0) + np.abs(t1) + np.abs(dt(HALF_LOG2PI))).sum(1)


def run_act(lib, device, actor, critic, xa, xc, std_t, eps_t, N, A, nulls, L=None, latent=None):
    """-> the six outputs as Bufs; the ones named in `nulls` go to the library as NULL and must stay untouched"""
    out = {k: Buf(device, N * (A if k in ("a_out", "a_st", "mu_st", "sig_st") else 1)) for k in ("a_out",) + OPTIONAL}
    ptrs = [adr(out["a_out"])] + [None if k in nulls else adr(out[k]) for k in OPTIONAL]
    if L is None:
        rc = lib.go2nn_policy_act(C.byref(actor.m), actor.packed.ptr, C.byref(critic.m), critic.packed.ptr, xa.data_ptr(), xc.data_ptr(), std_t.data_ptr(), eps_t.data_ptr(),
                                  *ptrs, N, stream_of(device))
    else:
        rc = lib.go2nn_policy_act_latent(C.byref(actor.m), actor.packed.ptr, C.byref(critic.m), critic.packed.ptr, latent.data_ptr(), L, xa.data_ptr(), xc.data_ptr(),
                                         std_t.data_ptr(), eps_t.data_ptr(), *ptrs, N, stream_of(device))
    assert rc == 0, lib.go2nn_last_error()
    sync(device)
    for k, b in out.items():
        assert b.intact() and (k not in nulls or b.untouched()), (k, "sentinels behind an output, or an output that was handed in as NULL")
    return out


def check_act(lib, device, adims, cdims, N, kind, nulls=(), L=None):
    A = adims[-1]
    rng = np.random.default_rng(list(adims) + list(cdims) + [N, (EXACT + ROUNDING).index(kind), len(nulls), L or 0] + [OPTIONAL.index(k) for k in nulls])
    xa, Wa, ba = make_case(kind, rng, adims, N)
    xc, Wc, bc = make_case(kind, rng, cdims, N)
    if L:
        xc[:, :L] = xa[:, :L]
    std, eps = rng.uniform(0.5, 1.5, size=A).astype(F32), rng.normal(size=(N, A)).astype(F32)
    actor, critic = Net(lib, device, Wa, ba), Net(lib, device, Wc, bc)
    xat, xct, std_t, eps_t = (dev_in(v, device) for v in (xa, xc, std, eps))
    o = run_act(lib, device, actor, critic, xat, xct, std_t, eps_t, N, A, nulls)
    again = run_act(lib, device, actor, critic, xat, xct, std_t, eps_t, N, A, nulls)
    assert all(same(o[k].get(), again[k].get()) for k in o), "not bit-equal from call to call"
    if L:
        lat = run_act(lib, device, actor, critic, dev_in(xa[:, L:], device), dev_in(xc[:, L:], device), std_t, eps_t, N, A, nulls, L, dev_in(xa[:, :L], device))
        assert all(same(o[k].get(), lat[k].get()) for k in o), "policy_act_latent != policy_act on the concatenated input"
    name = launch_name(lib, [actor, critic])
    tag = "%s %s %s N=%d" % (kind, adims, cdims, N)
    ya, yc = run_forward(lib, device, actor, xat, N).get().reshape(N, A), run_forward(lib, device, critic, xct, N).get().reshape(N, 1)
    alone = lambda net: launch_name(lib, [net]) == name          # (a network that fits as planes runs fp32 when its partner does not: then the single forward is another kernel)
    a_out = o["a_out"].get().reshape(N, A)
    if "mu_st" not in nulls:
        mu = o["mu_st"].get().reshape(N, A)
        assert not alone(actor) or same(mu, ya), (tag, "mu_st != go2nn_mlp_forward of the actor")
        compare("policy act %s mu" % name, tag, kind, mu, xa, Wa, ba)
    else:
        mu = ya
    if alone(actor):
        assert same(a_out, mu + std[None, :] * eps), (tag, "a != add(mu, mul(std, eps))")          # (numpy float32: two rounded operations)
    if "a_st" not in nulls:
        assert same(o["a_st"].get().reshape(N, A), a_out), tag
    if "sig_st" not in nulls:
        assert same(o["sig_st"].get().reshape(N, A), np.broadcast_to(std, (N, A))), tag
    if "v_st" not in nulls:
        v = o["v_st"].get()
        assert not alone(critic) or same(v, yc[:, 0]), (tag, "v_st != column 0 of go2nn_mlp_forward of the critic")
        compare("policy act %s value" % name, tag, kind, v.reshape(N, 1), xc, Wc, bc)
    if "lp_st" not in nulls:
        mu64, mu32, _ = reference(xa, Wa, ba)
        ref, S = logp_restated(mu64, std, eps, F64)
        within_s("policy act %s log-probability%s" % (name, " (integer mu up to 2^24: the sample's rounding is the error)" if kind in EXACT else ""), tag + " A=%d" % A, o["lp_st"].get(), logp_restated(mu32, std, eps, F32)[0], ref, S)


# ---- the packed image ---------------------------------------------------------------------------------------------------------------------------------------------------
IMAGE_SHAPES = sorted({(d[0], d[1]) for d in PLANE_SHAPES} | {(512, 512)})          # each first layer of the plane shapes; (512, 512) is written though the network runs as fp32


def check_image(lib, device, K, N):
    """both layouts restated from the header comments of go2nn_impl.cpp / go2nn_mlp3.h:
    fp32   [t][kb][lane][4]:                 n = 32 t + (lane & 31), k = 8 kb + 4 (lane >> 5) + e
    planes [t][kb of 16][plane][lane][8 bf16]: n = 32 t + (lane & 31), k = 16 kb + 8 (lane >> 5) + e"""
    rng = np.random.default_rng([K, N, 5])
    W, b = full_bits(rng, (N, K)), full_bits(rng, N)
    net = Net(lib, device, [W], [b])          # (asserts the sentinels behind go2nn_packed_floats floats)
    d, raw = net.d, net.packed.get()
    NT, KB, KB3, KV3 = d.NT[0], d.KB[0], d.KB3[0], d.KV3[0]
    w32 = raw[d.woff[0]:d.woff[0] + NT * KB * 256].reshape(NT, KB, 2, 32, 4).transpose(0, 3, 1, 2, 4).reshape(NT * 32, KB * 8)
    want = np.zeros_like(w32); want[:N, :K] = W
    assert same(w32, want), ("fp32 image", K, N)
    wb = np.zeros(NT * 32, F32); wb[:N] = b
    assert same(raw[d.boff[0]:d.boff[0] + NT * 32], wb), ("padded bias", K, N)
    pl = raw[d.woff3[0]:d.woff3[0] + NT * KB3 * 768]
    if not is_device(lib):
        assert np.isnan(pl).all()          # the host build has the fp32 image only
        return
    got = pl.view(np.uint16).reshape(NT, KB3, 3, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5).reshape(3, NT * 32, KB3 * 16)
    h, m, l, rest = planes(W)
    assert (rest == 0).all()
    for p, v in enumerate((h, m, l)):          # each plane is the bf16 rounding of the running remainder
        assert (bits(v) & 0xffff == 0).all()
        assert np.array_equal(got[p, :N, :K], (bits(v) >> 16).astype(np.uint16)), ("plane bits", p, K, N)
    pad = got.copy(); pad[:, :N, :K] = 0
    assert (pad == 0).all() and KB3 >= KV3 and (got[:, :, 16 * KV3:] == 0).all(), ("beyond the matrix: n >= N, k >= K, kb >= KV3", K, N)
    val = (got.astype(np.uint32) << 16).view(F32).astype(F64)
    assert np.array_equal(val[:, :N, :K].sum(0), W.astype(F64)), ("hi + mid + lo", K, N)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, device):
    """GO2NN_EINVAL, and nothing written"""
    st, N = stream_of(device), 5
    rng = np.random.default_rng(9)
    mk = lambda dims: Net(lib, device, *make_case("gauss", rng, dims, 1)[1:])
    wide = dev_in(np.zeros(MAX_WIDTH * MAX_WIDTH, F32), device)          # weights large enough for any shape below: a refusal that failed would still read its own memory
    scratch, y = Buf(device, 4096), Buf(device, N * 64)
    for dims, nl in (((8, 8), 0), ((8,) * 7, 7), ((0, 8), None), ((8, 0), None), ((513, 8), None), ((8, 513, 8), None)):
        m = mlp_struct(dims, [wide] * min(len(dims) - 1, MAX_LAYERS), [wide] * min(len(dims) - 1, MAX_LAYERS), nl)
        assert lib.go2nn_packed_floats(C.byref(m)) == GO2NN_EINVAL and lib.go2nn_mlp_arith(C.byref(m)) == GO2NN_EINVAL, (dims, nl)
        assert lib.go2nn_pack(C.byref(m), scratch.ptr, st) == GO2NN_EINVAL, (dims, nl)
        assert lib.go2nn_mlp_forward(C.byref(m), scratch.ptr, wide.data_ptr(), y.ptr, N, st) == GO2NN_EINVAL, (dims, nl)
    actor, actor33, critic, critic2 = mk((20, 24, 12)), mk((20, 24, 33)), mk((20, 24, 1)), mk((20, 24, 2))
    x, std_t, eps_t = dev_in(np.zeros((N, 64), F32), device), dev_in(np.ones(64, F32), device), dev_in(np.zeros((N, 64), F32), device)
    outs = [Buf(device, N * 64) for _ in range(6)]
    act = lambda a, c: lib.go2nn_policy_act(C.byref(a.m), a.packed.ptr, C.byref(c.m), c.packed.ptr, x.data_ptr(), x.data_ptr(), std_t.data_ptr(), eps_t.data_ptr(),
                                            *[adr(o) for o in outs], N, st)
    lat = lambda a, c, L: lib.go2nn_policy_act_latent(C.byref(a.m), a.packed.ptr, C.byref(c.m), c.packed.ptr, x.data_ptr(), L, x.data_ptr(), x.data_ptr(), std_t.data_ptr(),
                                                      eps_t.data_ptr(), *[adr(o) for o in outs], N, st)
    assert act(actor33, critic) == GO2NN_EINVAL and act(actor, critic2) == GO2NN_EINVAL
    assert lat(actor33, critic, 4) == GO2NN_EINVAL and lat(actor, critic2, 4) == GO2NN_EINVAL
    assert lat(actor, critic, 20) == GO2NN_EINVAL and lat(actor, critic, 21) == GO2NN_EINVAL and lat(actor, critic, 0) == GO2NN_EINVAL
    good = dict(x=x, x2=x, y=y, ldx=64, ldx2=64, kx=7, nrows=N, ldy=64)
    assert run_rows(lib, device, [actor], [good]) == 0 and not y.untouched()          # (the description the refusals below spoil is a valid one)
    y = Buf(device, N * 64)
    for bad in (dict(kx=0), dict(kx=21), dict(ldx=6), dict(x2=None), dict(ldy=11), dict(ldx2=12), dict(nrows=0)):
        assert run_rows(lib, device, [actor], [dict(good, y=y, **bad)]) == GO2NN_EINVAL, bad
    three = (C.POINTER(Go2nnMlp) * 3)(*[C.pointer(actor.m)] * 3)
    io3 = (Go2nnMlpIO * 3)(*[Go2nnMlpIO(x.data_ptr(), x.data_ptr(), None, adr(y), 64, 64, 7, N, 64, 0)] * 3)
    assert lib.go2nn_mlp_forward_rows(three, (C.c_void_p * 3)(*[adr(actor.packed)] * 3), io3, 3, st) == GO2NN_EINVAL
    assert lib.go2nn_mlp_forward_rows(three, (C.c_void_p * 3)(*[adr(actor.packed)] * 3), io3, 0, st) == GO2NN_EINVAL
    sync(device)
    assert scratch.untouched() and y.untouched() and all(o.untouched() for o in outs), "a refused call wrote something"


# ---- the cases, shared with tests/test_gpu_policy_paths.py ----------------------------------------------------------------------------------------------------------------
ROWS = (1, 31, 32, 33, 65, 257)          # 257 rows = 9 workgroups: every value of the tile-ownership rotation, and one again after the wrap
HEAD_NETS = {1: ((128, 40, 24, 1), (64, 288, 1)), 12: ((128, 40, 24, 12), (64, 288, 1)), 32: ((65, 300, 32), (129, 288, 1))}          # A -> actor, critic


COHERENT_SHAPES = [(K, N) for K in COHERENT_K for N in (7, 33, 288)]          # one layer; 288 outputs: NTW = 2 with an odd tile count
FORWARD_CASES = [(d, k) for d in PLANE_SHAPES + FALLBACK_SHAPES for k in kinds_for(d)]          # 33 rows: two workgroups, the second with one row


def rows_case(lib, device, nrows):
    for kind in ("int", "int20", "gauss"):
        check_forward(lib, device, (129, 288, 7), kind, nrows)
    for kind in ("int", "bits_x", "gauss"):
        check_forward(lib, device, (17, 33), kind, nrows)
    check_permutation(lib, device, (129, 288, 7), nrows)


def heads_case(lib, device, A):
    adims, cdims = HEAD_NETS[A]
    for kind in ("int", "gauss", "scaled"):
        for N in (33, 257):
            check_act(lib, device, adims, cdims, N, kind)
    check_act(lib, device, (24 + adims[0],) + adims[1:], (24 + cdims[0],) + cdims[1:], 65, "gauss", L=24)
    check_act(lib, device, (1 + adims[0],) + adims[1:], (1 + cdims[0],) + cdims[1:], 33, "int", L=1)


def null_subsets_case(lib, device):
    adims, cdims = HEAD_NETS[12]
    for r in range(len(OPTIONAL) + 1):
        for nulls in itertools.combinations(OPTIONAL, r):
            check_act(lib, device, adims, cdims, 33, "gauss", nulls)


def fp32_child():
    """the fp32-MFMA kernel at small ragged shapes: GO2_GEMM_SPLIT is read once per process, so tests/test_gpu_policy_paths.py starts this in a fresh one with GO2_GEMM_SPLIT=0"""
    from go2_rl_gym_amd import _nn
    assert FP32_ONLY
    lib = _nn.load_nn()
    for dims in FP32_CHILD_SHAPES:
        for nrows in (33, 257):
            for kind in [k for k in ("int", "int20", "gauss") if k in kinds_for(dims)]:
                check_forward(lib, "cuda:0", dims, kind, nrows)          # (Net asserts go2nn_mlp_arith == 1)
        check_same_rows(lib, "cuda:0", dims)
        check_permutation(lib, "cuda:0", dims, 257)
    for kind in ("int", "gauss"):
        check_act(lib, "cuda:0", (128, 40, 24, 12), (64, 288, 1), 257, kind)
        check_act(lib, "cuda:0", (24 + 128, 40, 24, 12), (24 + 64, 288, 1), 33, kind, L=24)
    print_table()
    print("FP32 CHILD OK")


def run_fp32_child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_policy_paths as p; p.fp32_child()" % (os.path.join(root, "tests"), root)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GO2_GEMM_SPLIT="0"), capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "FP32 CHILD OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


def print_table():
    for path in sorted(p for p in WORST if p.startswith("policy")):
        share, ek, ey, tag = WORST[path]
        print("[policy_paths table] %-52s %.1e (%.1e)   %.2f   %s" % (path, ek, ey, share, tag))


# ---- on the host build -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,kind", FORWARD_CASES, ids=str)
def test_forward(dims, kind):
    check_forward(load_nn_emu(), "cpu", dims, kind, 33)


@pytest.mark.parametrize("dims", COHERENT_SHAPES, ids=str)
def test_forward_on_the_plane_coherent_set(dims):
    check_forward(load_nn_emu(), "cpu", dims, "coherent", 33)


@pytest.mark.parametrize("nrows", ROWS)
def test_rows(nrows):
    rows_case(load_nn_emu(), "cpu", nrows)


@pytest.mark.parametrize("dims", [(129, 288, 7), (65, 300, 33), (480, 512)], ids=str)
def test_every_workgroup_computes_what_workgroup_0_does(dims):
    check_same_rows(load_nn_emu(), "cpu", dims)


@pytest.mark.parametrize("in_dim", STAGING_IN)
def test_staging(in_dim):
    for kind in ("int", "bits_x"):
        check_staging(load_nn_emu(), "cpu", in_dim, kind)


@pytest.mark.parametrize("kind", ["int", "int20", "gauss"])
def test_two_networks_on_row_subsets(kind):
    check_two_networks(load_nn_emu(), "cpu", (129, 288, 7), (65, 300, 33), 97, 33, kind)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("out_dim", NORMALIZE_OUT)
def test_normalize(out_dim, normalize):
    for kind in ("int", "gauss", "scaled"):
        check_normalize(load_nn_emu(), "cpu", out_dim, normalize, kind)


@pytest.mark.parametrize("A", sorted(HEAD_NETS))
def test_heads(A):
    heads_case(load_nn_emu(), "cpu", A)


def test_heads_with_every_subset_of_optional_outputs_null():
    null_subsets_case(load_nn_emu(), "cpu")


def test_heads_of_a_pair_of_which_one_network_does_not_fit():
    check_act(load_nn_emu(), "cpu", (45, 512, 256, 128, 12), (300, 512, 512, 1), 33, "gauss")


@pytest.mark.parametrize("K,N", IMAGE_SHAPES)
def test_packed_image(K, N):
    check_image(load_nn_emu(), "cpu", K, N)


def test_refusals():
    check_refusals(load_nn_emu(), "cpu")


# ---- the constructions themselves ----------------------------------------------------------------------------------------------------------------------------------------------
def test_describe_restated_reaches_what_the_cases_claim():
    for dims in CLAIMS:
        claim(dims)
    assert all(not claim(d).fits for d in FALLBACK_SHAPES) and all(d in CLAIMS for d in FP32_CHILD_SHAPES)
    layers = [(2 if nt > NN_WAVES else 1, nt, kv, ring) for d in map(Desc, PLANE_SHAPES + [(k, STAGING_OUT) for k in STAGING_IN]) for nt, kv, ring in zip(d.NT, d.KV3, d.ring)]
    for ntw in (1, 2):          # on both rings: KV3 == R (only the LAST trip), KV3 == R + 1, several trips, fewer k-blocks than the ring
        assert {"==" if kv == ring else "+1" if kv == ring + 1 else ">" if kv > 2 * ring else "<" if kv < ring else "" for n, nt, kv, ring in layers if n == ntw} >= {"==", "+1", ">"} | ({"<"} if ntw == 1 else set()), ntw
    assert any(n == 2 and nt % 2 == 1 for n, nt, kv, ring in layers) and any(nt == 2 * NN_WAVES for n, nt, kv, ring in layers)          # a clamped duplicate tile; 16 tiles
    assert all(nt <= 2 * NN_WAVES for d in map(Desc, CLAIMS) for nt in d.NT)          # run_layer<4> of the fp32 kernel cannot be reached at GO2NN_MAX_WIDTH 512
    assert {len(d) - 1 for d in PLANE_SHAPES} >= {1, 2, 6} and kx_options(45) == [1, 23, 44, 45] and kx_options(1) == [1] and kx_options(2) == [1, 2]


@pytest.mark.parametrize("dims", [d for d in CLAIMS if len(d) > 2], ids=str)
def test_integer_networks_are_exact_in_fp32(dims):
    """hidden pre-activations >= 0 (the ELU is the identity), the first hidden layer above 256, int20 above 2^19 with a nonzero lo plane, the carried scale below 2^24"""
    for kind in ("int", "int20"):
        x, Ws, bs = make_case(kind, np.random.default_rng(1), dims, 33)
        h = x.astype(F64)
        for l, (W, b) in enumerate(zip(Ws[:-1], bs[:-1])):
            assert (W >= 0).all() and (b >= 0).all() and (h >= 0).all()
            h = h @ W.astype(F64).T + b
            if l == 0:
                assert h.max() > (2 ** 19 if kind == "int20" else 256)
                hi, mid, lo, _ = planes(h.astype(F32))
                assert (mid != 0).any() and (kind == "int" or (lo != 0).any())
        assert carried_scale(x, Ws, bs).max() < 2 ** 24 and (Ws[-1] < 0).any() and np.array_equal(reference(x, Ws, bs)[0], reference(x, Ws, bs)[1].astype(F64))


def test_bit_networks_copy_one_element():
    for dims in ((17, 33), (129, 288, 7), SIX):
        for kind in ("bits_x", "bits_w"):
            x, Ws, bs = make_case(kind, np.random.default_rng(2), dims, 33)
            ref, yard, _ = reference(x, Ws, bs)
            assert np.array_equal(ref, yard.astype(F64)) and (ref != 0).any()
            src = x if kind == "bits_x" else Ws[0]
            assert (bits(src) & 1 == 1).all() and (src > 0).all() == (len(dims) > 2 or kind == "bits_x")
            nz = ref[ref != 0]
            assert ((bits(nz.astype(F32)) & 0x7fffff) != 0).all() and (planes(nz.astype(F32))[2] != 0).mean() > 0.9          # the copies still carry all three planes


@pytest.mark.parametrize("N", [7, 33, 288])
@pytest.mark.parametrize("K", COHERENT_K)
def test_coherent_set_tells_six_terms_from_five(K, N):
    """in this kernel's form (last layer: bias, no ELU): the six kept terms are inside the bound, any five of them outside it at EVERY output"""
    x, Ws, bs = make_case("coherent", np.random.default_rng([K, N]), (K, N), 33)
    W, b = Ws[0], bs[0].astype(F64)
    pa, pb = [v.astype(F64) for v in planes(x)[:3]], [v.astype(F64) for v in planes(W)[:3]]
    terms = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]          # go2nn_mlp3.h: PA, PB
    ref, yard, S = reference(x, Ws, bs)
    bound = 4 * float((np.abs(yard - ref) / S).max()) + ULP
    e = lambda got: np.abs(got - ref) / S
    assert e(sum(pa[i] @ pb[j].T for i, j in terms) + b).max() <= bound
    for drop in terms:
        five = sum(pa[i] @ pb[j].T for i, j in terms if (i, j) != drop) + b
        assert e(five).min() > bound, (K, N, drop, e(five).min(), bound)


def test_measured_table_is_printed():
    """(runs last in this file) the largest share of the bound per path over the cases above"""
    print_table()
