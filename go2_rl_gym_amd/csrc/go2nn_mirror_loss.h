// go2nn_mirror_loss.h — the mirror (equivariance) loss of symmetry-augmented PPO (include/go2nn.h: go2nn_mirror_loss*, added within ABI 7; rsl_rl/algorithms/ppo.py,
// `algorithm.mirror_loss_coef`; the tables: go2_rl_gym_amd/utils/symmetry.py).  Included at the end of go2nn_impl.cpp (FAIL, HIPCHK, HB_MAX_C are its helpers).
//
// An augmented mini-batch is [B originals | B mirror images]: the actor's forward pass has already left pi(o) in row r and pi(M_o o) in row B + r, so the term
//   e[r, j] = mu[r, j] - sign[j] mu[B + r, perm[j]],   L = coef / (B A) sum e^2,   g[r, j] = 2 coef / (B A) e[r, j],   g[B + r, perm[j]] = -sign[j] g[r, j]
// costs no forward pass: ONE streaming pass over the actor's last hidden activations y_a [2B, K], launched right behind go2nn_ppo_heads on the same stream, which
//   1. forms mu of both rows of a pair with go2nn_ppo_heads' fp32 dot products (a lane owns four columns, the QP lanes of a row reduce-scatter the A partial products:
//      lane role c = cq >> SH ends up with mu[c]),
//   2. forms e and both g on the role lanes (mu[B + r, perm[j]] and g[r, perm[j]] come from the partner role's lane by one shuffle each: the table never indexes memory),
//   3. ADDS (g W_mu) * ELU'(y_a) to both rows of gz_a (ELU' from the output, y > 0 ? 1 : y + 1) and keeps dW_mu, the column sums of what it added and db_mu as
//      per-workgroup partial rows [ L (+ 3 zeros) | dW_mu [A, K] | gb_a [K] | db_mu [A] ], finished by go2nn_sum_rows.  L is formed by a one-block launch behind
//      the pass from the workgroups' fp64 sums of e^2 (go2nn_mirror_loss_finish_kernel below: row 0 holds it, rounded once).
// Thread = (k quad cq, pair lane rl) as in go2nn_ppo_heads_kernel; the next pair's four loads fly while this pair is worked on; the row lanes' accumulators meet in LDS
// behind ONE barrier and are added in a fixed order: no atomics, two launches give the same bits.  HBM traffic per pair: 2 K floats of y_a read, 2 K of gz_a read and
// written (75 MB at 24576 pairs x 128).
// Compiled for gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage): <12> (the Go2's 12 actions) 226 VGPRs, 54400 B of LDS, no scratch, no spills, 2 waves per
// SIMD (go2nn_ppo_heads_kernel<12>: 224 VGPRs, 63808 B); <4> 132 VGPRs, 21632 B, 3 waves; <8> 182 VGPRs, 38016 B, 2 waves; <16> 256 VGPRs + 14 AGPRs, 70784 B, 1 wave;
// the one-block loss launch 8 VGPRs, 2048 B; no scratch and no spills in any of them.
// The host build (GO2_EMU) restates the same formulas in plain loops: the dot products in the device's order, one partial row per ML_EMU_PAIRS pairs.
#ifndef GO2NN_MIRROR_LOSS_H
#define GO2NN_MIRROR_LOSS_H

#define ML_NSTAT 4          // the weighted loss and three zeros (the matrices behind it start on a float4 boundary of the row)
#define ML_EMU_PAIRS 64     // the host build: pairs per partial row (sums of a few tens of terms, then go2nn_sum_rows: as short as the device's chains)
// a lane's share of a dot product (what the device compiler's contraction makes of go2nn_ppo_heads' y.x w.x + y.y w.y + y.z w.z + y.w w.w; the host build says it itself)
#define ML_DOT4(a0, a1, a2, a3, b0, b1, b2, b3) fmaf((a3), (b3), fmaf((a2), (b2), fmaf((a1), (b1), (a0) * (b0))))

static inline int mirror_loss_ok(int B, int A, int K) { return B > 0 && A >= 1 && A <= HB_MAX_C && K >= 4 && K <= 256 && (K & 3) == 0; }
PH_HD static inline int mirror_loss_ncols(int A, int K) { return ML_NSTAT + (A + 1) * K + A; }

#ifndef GO2_EMU
struct MirrorLossArgs {
  const float *y_a, *w_mu, *b_mu, *sign; const int16_t* perm;
  float *gz_a, *part;
  int B, A, K; float scale;          // scale = coef / (B A), for the gradients (the reported loss takes it in fp64: go2nn_mirror_loss_finish_kernel)
};

// the head's A dot products of one row, reduce-scattered over the row's QP lanes (go2nn_ppo_heads_kernel's exchange: 8 + 4 + 2 + 1 values, then the lanes of one role)
template <int CP>
__device__ __forceinline__ float ml_head_dot(const float4 y, const float4 (&wq)[CP], int cq, int QP) {
  float pm[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) { const float4 w = wq[c < CP ? c : 0]; pm[c] = c < CP ? ML_DOT4(y.x, y.y, y.z, y.w, w.x, w.y, w.z, w.w) : 0.f; }
  const int d3 = QP >> 1, d2 = QP >> 2, d1 = QP >> 3, d0 = QP >> 4;
  float p8[8], p4[4], p2[2], m;
  { const bool up = cq & d3;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float keep = up ? pm[8 + i] : pm[i], send = up ? pm[i] : pm[8 + i]; p8[i] = keep + __shfl_xor(send, d3); } }
  { const bool up = cq & d2;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float keep = up ? p8[4 + i] : p8[i], send = up ? p8[i] : p8[4 + i]; p4[i] = keep + __shfl_xor(send, d2); } }
  { const bool up = cq & d1;
#pragma unroll
    for (int i = 0; i < 2; ++i) { const float keep = up ? p4[2 + i] : p4[i], send = up ? p4[i] : p4[2 + i]; p2[i] = keep + __shfl_xor(send, d1); } }
  { const bool up = cq & d0; const float keep = up ? p2[1] : p2[0], send = up ? p2[0] : p2[1]; m = keep + __shfl_xor(send, d0); }
  for (int d = d0 >> 1; d >= 1; d >>= 1) m += __shfl_xor(m, d);
  return m;
}

struct MlPair { float4 y0, y1, z0, z1; };          // what a lane loads for one pair: its four columns of both rows of y_a and of gz_a

template <int CP>
__global__ void __launch_bounds__(256, CP > 12 ? 1 : 2) go2nn_mirror_loss_kernel(const MirrorLossArgs a, int qp_log2, int pairs_per_wg) {
  static_assert(CP <= 16, "16 value slots in the reduce-scatter");
  __shared__ float4 sh[CP + 1][256];
  __shared__ float shs[256 / 16][HB_MAX_C];
  __shared__ double shl[256 / 16];
  const int B = a.B, A = a.A, K = a.K;
  const int QP = 1 << qp_log2, RL = 256 >> qp_log2, SH = qp_log2 - 4;          // QP >= 16 lanes per row; lane role c = cq >> SH (2^SH lanes share a role)
  const int cq = threadIdx.x & (QP - 1), rl = threadIdx.x >> qp_log2;
  const bool on = 4 * cq < K;
  const int k0 = on ? 4 * cq : 0;
  const int role = cq >> SH; const bool first = (cq & ((1 << SH) - 1)) == 0, role_on = role < A;
  const int rc = role_on ? role : 0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 wq[CP], dw[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float4 t = *reinterpret_cast<const float4*>(a.w_mu + (size_t)min(c, A - 1) * K + k0);
    wq[c] = (on && c < A) ? t : zero; dw[c] = zero;
  }
  // the role's action dimension: head bias, its mirror partner (clamped: the table was checked on the host, a lane index can do no harm either way) and sign
  const float bm = a.b_mu[rc], sg = a.perm ? a.sign[rc] : 1.f;
  const int pj = a.perm ? min(max((int)a.perm[rc], 0), A - 1) : rc;
  const int src = pj << SH;          // the first lane of the partner role, within the row's QP lanes
  float4 gb = zero;
  float dbm = 0.f;
  double s_e2 = 0.0;          // (the reported loss: one fp64 fma per pair on the role lanes keeps its sum at the rounding of its result)
  const int r0 = blockIdx.x * pairs_per_wg, r1 = min(B, r0 + pairs_per_wg);
  auto fetch = [&](int rb) {
    MlPair x; const size_t r = (size_t)min(rb + rl, r1 - 1);
    x.y0 = *reinterpret_cast<const float4*>(a.y_a + r * K + k0); x.y1 = *reinterpret_cast<const float4*>(a.y_a + ((size_t)B + r) * K + k0);
    x.z0 = *reinterpret_cast<const float4*>(a.gz_a + r * K + k0); x.z1 = *reinterpret_cast<const float4*>(a.gz_a + ((size_t)B + r) * K + k0);
    return x;
  };
  MlPair nx = fetch(r0);
  for (int rb = r0; rb < r1; rb += RL) {          // (uniform trip count: the exchanges need every lane of a row; pairs past the end run on a clamped pair and are dropped)
    const MlPair x = nx;
    nx = fetch(min(rb + RL, r1 - 1));
    const bool live = rb + rl < r1;
    const float m0 = ml_head_dot<CP>(x.y0, wq, cq, QP) + bm, m1 = ml_head_dot<CP>(x.y1, wq, cq, QP) + bm;
    // role j: e = mu[r, j] - sign[j] mu[B + r, perm[j]];  g0 = d L / d mu[r, j];  g1 = d L / d mu[B + r, j] = -sign[j] g0[perm[j]] (an involution with sign[perm[j]] = sign[j])
    const float e = (live && role_on) ? m0 - sg * __shfl(m1, src, QP) : 0.f;
    const float g0 = a.scale * 2.f * e, g1 = -sg * __shfl(g0, src, QP);
    if (first) { s_e2 = fma((double)e, (double)e, s_e2); dbm += g0 + g1; }
    float4 gx0 = zero, gx1 = zero;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float ga = __shfl(g0, c << SH, QP), gm = __shfl(g1, c << SH, QP);
      gx0.x = fmaf(ga, wq[c].x, gx0.x); gx0.y = fmaf(ga, wq[c].y, gx0.y); gx0.z = fmaf(ga, wq[c].z, gx0.z); gx0.w = fmaf(ga, wq[c].w, gx0.w);
      gx1.x = fmaf(gm, wq[c].x, gx1.x); gx1.y = fmaf(gm, wq[c].y, gx1.y); gx1.z = fmaf(gm, wq[c].z, gx1.z); gx1.w = fmaf(gm, wq[c].w, gx1.w);
      dw[c].x = fmaf(ga, x.y0.x, dw[c].x); dw[c].y = fmaf(ga, x.y0.y, dw[c].y); dw[c].z = fmaf(ga, x.y0.z, dw[c].z); dw[c].w = fmaf(ga, x.y0.w, dw[c].w);
      dw[c].x = fmaf(gm, x.y1.x, dw[c].x); dw[c].y = fmaf(gm, x.y1.y, dw[c].y); dw[c].z = fmaf(gm, x.y1.z, dw[c].z); dw[c].w = fmaf(gm, x.y1.w, dw[c].w);
    }
    float4 d0, d1, o0, o1;          // ELU' from the output; o: what is added (its column sums are gb_a); gz += gx * ELU' as ONE fma: a single rounding of the new gz
    d0.x = x.y0.x > 0.f ? 1.f : x.y0.x + 1.f; d0.y = x.y0.y > 0.f ? 1.f : x.y0.y + 1.f; d0.z = x.y0.z > 0.f ? 1.f : x.y0.z + 1.f; d0.w = x.y0.w > 0.f ? 1.f : x.y0.w + 1.f;
    d1.x = x.y1.x > 0.f ? 1.f : x.y1.x + 1.f; d1.y = x.y1.y > 0.f ? 1.f : x.y1.y + 1.f; d1.z = x.y1.z > 0.f ? 1.f : x.y1.z + 1.f; d1.w = x.y1.w > 0.f ? 1.f : x.y1.w + 1.f;
    o0.x = gx0.x * d0.x; o0.y = gx0.y * d0.y; o0.z = gx0.z * d0.z; o0.w = gx0.w * d0.w;
    o1.x = gx1.x * d1.x; o1.y = gx1.y * d1.y; o1.z = gx1.z * d1.z; o1.w = gx1.w * d1.w;
    if (live && on) {
      const size_t r = (size_t)(rb + rl);
      *reinterpret_cast<float4*>(a.gz_a + r * K + k0) = make_float4(fmaf(gx0.x, d0.x, x.z0.x), fmaf(gx0.y, d0.y, x.z0.y), fmaf(gx0.z, d0.z, x.z0.z), fmaf(gx0.w, d0.w, x.z0.w));
      *reinterpret_cast<float4*>(a.gz_a + ((size_t)B + r) * K + k0) = make_float4(fmaf(gx1.x, d1.x, x.z1.x), fmaf(gx1.y, d1.y, x.z1.y), fmaf(gx1.z, d1.z, x.z1.z), fmaf(gx1.w, d1.w, x.z1.w));
    }
    gb.x += o0.x + o1.x; gb.y += o0.y + o1.y; gb.z += o0.z + o1.z; gb.w += o0.w + o1.w;          // (a dropped pair: e = 0, so its o are zeros)
  }
  // the workgroup's partial row; the row lanes of a column quad are added in a fixed order
  float* prow = a.part + (size_t)blockIdx.x * mirror_loss_ncols(A, K);
  float* pa = prow + ML_NSTAT;
#pragma unroll
  for (int c = 0; c < CP + 1; ++c) sh[c][threadIdx.x] = c < CP ? dw[c < CP ? c : 0] : gb;
  // the pair's squared errors sit on the first lane of every role: once round the row, then lane 0 of the row holds the row lane's sum
  for (int d = 1; d < QP; d <<= 1) s_e2 += __shfl_xor(s_e2, d);
  if (cq == 0) shl[rl] = s_e2;
  if (first && role_on) shs[rl][role] = dbm;
  __syncthreads();
  for (int task = threadIdx.x; task < ((CP + 1) << qp_log2); task += 256) {
    const int c = task >> qp_log2, q = task & (QP - 1);
    if ((c < A || c == CP) && 4 * q < K) {
      float4 t4 = sh[c][q];
      for (int j = 1; j < RL; ++j) { const float4 t = sh[c][j * QP + q]; t4.x += t.x; t4.y += t.y; t4.z += t.z; t4.w += t.w; }
      float* o = pa + (size_t)(c < CP ? c : A) * K + 4 * q;          // (a partial row starts wherever the rows before it end: four plain stores, no alignment assumed)
      o[0] = t4.x; o[1] = t4.y; o[2] = t4.z; o[3] = t4.w;
    }
  }
  if ((int)threadIdx.x <= HB_MAX_C) {
    const int t = threadIdx.x;
    if (t == HB_MAX_C) {
      double s = shl[0];
      for (int j = 1; j < RL; ++j) s += shl[j];
      // the workgroup's sum of e^2 as the two halves of its fp64 bits, for go2nn_mirror_loss_finish_kernel (which leaves [L | 0 | 0 | 0] in row 0 and zeros in the others)
      prow[0] = 0.f; prow[1] = 0.f; prow[2] = __int_as_float(__double2hiint(s)); prow[3] = __int_as_float(__double2loint(s));
    } else if (t < A) {
      float s = shs[0][t];
      for (int j = 1; j < RL; ++j) s += shs[j][t];
      pa[(size_t)(A + 1) * K + t] = s;
    }
  }
}

// The reported loss.  A sum of per-workgroup fp32 losses in fp32 ends up to a few roundings of the result away from it, whatever the order; the workgroups' sums of
// e^2 are fp64, so this one-block launch behind the pass adds them in fp64 (a thread's rows in ascending order, then a fixed tree: deterministic, no atomics), scales in
// fp64 and rounds ONCE: row 0 gets the weighted loss, every other row 0, and the two columns that carried the fp64 bits are zeroed — go2nn_sum_rows then adds zeros to it.
__global__ void __launch_bounds__(256) go2nn_mirror_loss_finish_kernel(float* __restrict__ part, int nrows, int ncols, double lscale) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int r = threadIdx.x; r < nrows; r += 256) {
    const float* p = part + (size_t)r * ncols;
    s += __hiloint2double(__float_as_int(p[2]), __float_as_int(p[3]));
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  const float total = (float)(lscale * sh[0]);
  for (int r = threadIdx.x; r < nrows; r += 256) {          // (the rows this thread has read)
    float* p = part + (size_t)r * ncols;
    p[0] = r == 0 ? total : 0.f; p[2] = 0.f; p[3] = 0.f;
  }
}

// ~512 workgroups of whole pair groups, as go2nn_ppo_heads (two per CU cover each other's loads)
static inline void mirror_loss_shape(int B, int K, int* qp_log2, int* pairs_per_wg, int* nwg) {
  int q = 4;
  while ((1 << q) * 4 < K) ++q;
  const int RL = 256 >> q;
  int rows = (B + 511) / 512;
  rows = (rows + RL - 1) / RL * RL;
  *qp_log2 = q; *pairs_per_wg = rows; *nwg = (B + rows - 1) / rows;
}
#endif  // !GO2_EMU

#ifdef GO2_EMU
// the host build: pairs [r0, r1) into the partial row S, plain loops -> their sum of e^2 (fp64)
static double mirror_loss_host_rows(const Go2nnMirrorLoss& m, int r0, int r1, float scale, float* S) {
  const int B = m.B, A = m.A, K = m.K, nc = mirror_loss_ncols(A, K);
  int QP = 16; while (QP * 4 < K) QP *= 2;
  for (int i = 0; i < nc; ++i) S[i] = 0.f;
  float* pa = S + ML_NSTAT;
  double e2 = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float* y[2] = {m.y_a + (size_t)r * K, m.y_a + ((size_t)B + r) * K};
    float* gz[2] = {m.gz_a + (size_t)r * K, m.gz_a + ((size_t)B + r) * K};
    float mu[2][HB_MAX_C], g[2][HB_MAX_C];
    // the dot products in the device kernel's order: four columns per lane, then the row's QP lanes halved log2(QP) times
    for (int h = 0; h < 2; ++h)
      for (int c = 0; c < A; ++c) {
        const float* w = m.w_mu + (size_t)c * K;
        float lane[64];
        for (int q = 0; q < QP; ++q) lane[q] = 4 * q < K ? ML_DOT4(y[h][4 * q], y[h][4 * q + 1], y[h][4 * q + 2], y[h][4 * q + 3], w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]) : 0.f;
        for (int d = QP >> 1; d >= 1; d >>= 1) for (int q = 0; q < d; ++q) lane[q] += lane[q + d];
        mu[h][c] = lane[0] + m.b_mu[c];
      }
    for (int j = 0; j < A; ++j) {
      const int pj = m.perm ? m.perm[j] : j; const float sg = m.perm ? m.sign[j] : 1.f;
      const float e = mu[0][j] - sg * mu[1][pj];
      e2 = fma((double)e, (double)e, e2);
      g[0][j] = scale * 2.f * e; g[1][pj] = -sg * g[0][j];
    }
    for (int c = 0; c < A; ++c) pa[(size_t)(A + 1) * K + c] += g[0][c] + g[1][c];
    for (int k = 0; k < K; ++k) {
      float o[2];
      for (int h = 0; h < 2; ++h) {
        float gx = 0.f; for (int c = 0; c < A; ++c) gx = fmaf(g[h][c], m.w_mu[(size_t)c * K + k], gx);
        const float d = y[h][k] > 0.f ? 1.f : y[h][k] + 1.f;
        o[h] = gx * d;
        gz[h][k] = fmaf(gx, d, gz[h][k]);
      }
      for (int c = 0; c < A; ++c) pa[(size_t)c * K + k] = fmaf(g[1][c], y[1][k], fmaf(g[0][c], y[0][k], pa[(size_t)c * K + k]));
      pa[(size_t)A * K + k] += o[0] + o[1];
    }
  }
  return e2;
}
#endif

extern "C" {

int32_t go2nn_mirror_loss_cols(int32_t A, int32_t K) {
  if (!mirror_loss_ok(1, A, K)) FAIL(GO2NN_EINVAL, "mirror loss: 1 <= A <= %d, K a multiple of 4 up to 256", HB_MAX_C);
  return mirror_loss_ncols(A, K);
}

int32_t go2nn_mirror_loss_rows(int32_t B, int32_t A, int32_t K) {
  if (!mirror_loss_ok(B, A, K)) FAIL(GO2NN_EINVAL, "mirror loss: bad shape (B %d pairs, A %d, K %d)", B, A, K);
#ifdef GO2_EMU
  return (B + ML_EMU_PAIRS - 1) / ML_EMU_PAIRS;
#else
  int q, rows, nwg; mirror_loss_shape(B, K, &q, &rows, &nwg); return nwg;
#endif
}

int go2nn_mirror_loss_check_table(const int16_t* host_perm, const float* host_sign, int32_t A) {
  if (!host_perm || !host_sign) FAIL(GO2NN_EINVAL, "mirror loss table: a null pointer");
  if (A < 1 || A > HB_MAX_C) FAIL(GO2NN_EINVAL, "mirror loss table: %d actions outside [1, %d]", A, HB_MAX_C);
  for (int32_t j = 0; j < A; ++j) {
    if (host_perm[j] < 0 || host_perm[j] >= A) FAIL(GO2NN_EINVAL, "mirror loss table: perm[%d] = %d outside [0, %d)", j, (int)host_perm[j], A);
    if (host_sign[j] != 1.0f && host_sign[j] != -1.0f) FAIL(GO2NN_EINVAL, "mirror loss table: sign[%d] = %g is neither +1 nor -1", j, (double)host_sign[j]);
  }
  for (int32_t j = 0; j < A; ++j) {
    const int32_t p = host_perm[j];
    if (host_perm[p] != j) FAIL(GO2NN_EINVAL, "mirror loss table: perm is not an involution (perm[perm[%d]] = %d)", j, (int)host_perm[p]);
    if (host_sign[p] != host_sign[j]) FAIL(GO2NN_EINVAL, "mirror loss table: sign[perm[%d]] = %g differs from sign[%d] = %g", j, (double)host_sign[p], j, (double)host_sign[j]);
  }
  return 0;
}

int go2nn_mirror_loss(const Go2nnMirrorLoss* m, void* stream) {
  if (!m) FAIL(GO2NN_EINVAL, "mirror loss: a null argument struct");
  if (!mirror_loss_ok(m->B, m->A, m->K)) FAIL(GO2NN_EINVAL, "mirror loss: bad shape (B %d pairs >= 1, 1 <= A %d <= %d, K %d a multiple of 4 up to 256)", m->B, m->A, HB_MAX_C, m->K);
  if (!m->y_a || !m->w_mu || !m->b_mu || !m->gz_a || !m->partials) FAIL(GO2NN_EINVAL, "mirror loss: a null pointer");
  if ((m->perm == nullptr) != (m->sign == nullptr)) FAIL(GO2NN_EINVAL, "mirror loss: perm and sign are given together or not at all");
  if (2LL * m->B * m->K >= (1LL << 31)) FAIL(GO2NN_EINVAL, "mirror loss: 2 x %d x %d elements do not fit 31 bits", m->B, m->K);
  const int B = m->B, A = m->A, K = m->K;
  const float scale = m->coef / ((float)B * (float)A);
  const double lscale = (double)m->coef / ((double)B * (double)A);
#ifdef GO2_EMU
  (void)stream;
  if (m->perm && go2nn_mirror_loss_check_table(m->perm, m->sign, A) != 0) return GO2NN_EINVAL;          // (the host build can read the table)
  double e2 = 0.0;
  for (int r0 = 0; r0 < B; r0 += ML_EMU_PAIRS)          // one partial row per ML_EMU_PAIRS pairs
    e2 += mirror_loss_host_rows(*m, r0, r0 + ML_EMU_PAIRS < B ? r0 + ML_EMU_PAIRS : B, scale, m->partials + (size_t)(r0 / ML_EMU_PAIRS) * mirror_loss_ncols(A, K));
  m->partials[0] = (float)(lscale * e2);          // the reported loss: fp64 to the end, rounded once, in row 0 (the other rows hold 0)
#else
  MirrorLossArgs a;
  a.y_a = m->y_a; a.w_mu = m->w_mu; a.b_mu = m->b_mu; a.perm = m->perm; a.sign = m->sign; a.gz_a = m->gz_a; a.part = m->partials;
  a.B = B; a.A = A; a.K = K; a.scale = scale;
  int q, rows, nwg; mirror_loss_shape(B, K, &q, &rows, &nwg);
  hipStream_t st = (hipStream_t)stream;
  if (A <= 4)       hipLaunchKernelGGL(go2nn_mirror_loss_kernel<4>,  dim3(nwg), dim3(256), 0, st, a, q, rows);
  else if (A <= 8)  hipLaunchKernelGGL(go2nn_mirror_loss_kernel<8>,  dim3(nwg), dim3(256), 0, st, a, q, rows);
  else if (A <= 12) hipLaunchKernelGGL(go2nn_mirror_loss_kernel<12>, dim3(nwg), dim3(256), 0, st, a, q, rows);
  else              hipLaunchKernelGGL(go2nn_mirror_loss_kernel<16>, dim3(nwg), dim3(256), 0, st, a, q, rows);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_mirror_loss_finish_kernel, dim3(1), dim3(256), 0, st, m->partials, nwg, mirror_loss_ncols(A, K), lscale);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_MIRROR_LOSS_H
