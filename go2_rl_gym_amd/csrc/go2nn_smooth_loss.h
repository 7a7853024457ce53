// go2nn_smooth_loss.h — the temporal action-smoothness loss of PPO on env-block mini-batches (include/go2nn.h: go2nn_smooth_*, added within ABI 7;
// rsl_rl/algorithms/ppo.py, `algorithm.smooth_loss_coef`).  Included at the end of go2nn_impl.cpp behind go2nn_mirror_loss.h, whose dot product (ML_DOT4, ml_head_dot),
// partial-row layout (ML_NSTAT, mirror_loss_ncols) and one-block fp64 loss launch (go2nn_mirror_loss_finish_kernel) it shares.
//
// A mini-batch in block layout is blocks x T x n rows, row r = b T n + t n + j: all T steps of n environments (and, under symmetry augmentation, of their mirror
// images: block 1).  Rows (t, j) and (t + 1, j) are both ordinary PPO samples of the mini-batch, so with mu = y_a W_mu^T + b_mu and the pair weights w[t, j] in {0, 1}
//   e[b, t, j, :] = w[t, j] (mu[b, t, j, :] - mu[b, t + 1, j, :])   (t < T - 1),   L = coef / (blocks (T - 1) n A) sum e^2,
//   g[b, t, j, :] = 2 coef / (blocks (T - 1) n A) (e[b, t, j, :] - e[b, t - 1, j, :]),   e[., -1] = e[., T - 1] = 0
// costs no forward pass: ONE streaming pass over the actor's last hidden activations, launched behind go2nn_ppo_heads (and go2nn_mirror_loss) on the same stream.
// The pairs overlap — row t + 1 is the second row of pair t and the first of pair t + 1 —, so a workgroup owns a run of 256 / QP consecutive envs of one block and WALKS
// t over a time segment [t0, t1): row (t + 1, j) lies n rows behind row (t, j), a step of the env lanes is one contiguous 256 / QP x K float span.  A lane keeps y[t],
// gz[t] and y[t + 1], gz[t + 1] in registers while the loads of row t + 2 fly; the role lanes (ml_head_dot: role c ends up with mu[c]) keep mu[t] and e[t - 1]: when
// mu[t + 1] has been formed, g[t] is complete and row t's backward runs — (g W_mu) * ELU'(y_a) (ELU' from the output) ADDED to gz_a with one fma, dW_mu, the column
// sums of what was added and db_mu into the workgroup's partial row [ fp64 sum of e^2 | dW_mu [A, K] | gb_a [K] | db_mu [A] ] behind ONE barrier in a fixed order.
// Every row of y_a and gz_a is read once and every row of gz_a written once by exactly one lane group: no atomics, no race, two launches give the same bits.
//
// TIME SEGMENTS.  At 4096 envs and 4 mini-batches (n = 1024, K = 128: 8 envs per workgroup) one segment is 128 workgroups walking 24 dependent steps on 256 CUs.  T is
// therefore split into S segments [s T / S, (s + 1) T / S) with a one-step halo: a segment also forms mu of the row in front of it (for e[t0 - 1]) and of the row behind it
// (for e[t1 - 1]) — two extra row reads of y_a and two extra dot products per segment, no extra write; the pair (t1 - 1, t1) is counted in the loss by the segment that
// owns row t1 - 1 only.  S = the smallest count that reaches SL_TARGET_WG workgroups, at most T / 2 (a segment owns at least two rows).  Tried on one MI355X at the
// update's shape (24 x 1024 rows, A = 12, K = 128; device events around 50 back-to-back calls of both launches, two rounds; profiles/smooth_loss_bench.json,
// tools/smooth_loss_bench.py --segments forces a count through go2nn_smooth_loss_set_segments): 1 segment 35.1 / 34.3 us, 2: 24.5 / 23.9, 3: 22.1 / 21.8, 4 (512 workgroups,
// the choice): 20.7 / 20.1, 6: 28.3 / 28.3, 8: 28.0 / 27.9, 12: 34.8 / 34.8 — beyond two workgroups per CU the halo's extra reads and dot products cost more than the shorter
// walk saves; go2nn_mirror_loss on as many rows 17.0 us, a device-to-device copy of the same 38 MB 5.4 us.
// Compiled for gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage): <12> (the Go2's 12 actions) 182 VGPRs, 54400 B of LDS, no scratch, no spills, 2 waves per SIMD
// (go2nn_mirror_loss_kernel<12>: 226 VGPRs — only one row's gx is live here); <4> 102 VGPRs, 21632 B, 4 waves; <8> 146 VGPRs, 38016 B, 3 waves; <16> 222 VGPRs, 70784 B,
// 2 waves; the index launch 8 VGPRs, its counter launch 2, no LDS; no scratch and no spills in any of them.  Plain vector loads and stores only.
// The host build (GO2_EMU) restates the same formulas in plain loops: the dot products in the device's order, one partial row per block and SL_EMU_ENVS envs.
#ifndef GO2NN_SMOOTH_LOSS_H
#define GO2NN_SMOOTH_LOSS_H

#ifdef GO2_EMU
#define GO2_SHUFFLE_FN static inline
#else
#define GO2_SHUFFLE_FN static __host__ __device__ inline
#endif
#include "../../include/go2sim_shuffle.h"

#define SL_EMU_ENVS 8        // the host build: envs per partial row (the device's env lanes of a workgroup at K = 128)
#define SL_TARGET_WG 512     // the device: split T until the launch has this many workgroups (two per CU cover each other's loads)

static int g_smooth_segments = 0;          // go2nn_smooth_loss_set_segments: 0 = automatic

static inline int smooth_loss_ok(int blocks, int T, int n, int A, int K) {
  return blocks >= 1 && blocks <= 2 && T >= 2 && n >= 1 && A >= 1 && A <= HB_MAX_C && K >= 4 && K <= 256 && (K & 3) == 0;
}
static inline long long smooth_loss_elems(int blocks, int T, int n, int K) { return (long long)blocks * T * n * K; }

// the launch shape: QP lanes per row, RL envs per workgroup, S time segments -> workgroups = blocks x groups x S, workgroup id = (b groups + grp) S + s
static inline void smooth_loss_shape(int blocks, int T, int n, int K, int* qp_log2, int* groups, int* segs) {
  int q = 4;
  while ((1 << q) * 4 < K) ++q;
  const int RL = 256 >> q, g = (n + RL - 1) / RL;
  int S = g_smooth_segments > 0 ? g_smooth_segments : (SL_TARGET_WG + blocks * g - 1) / (blocks * g);
  const int smax = T / 2 > 1 ? T / 2 : 1;
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  *qp_log2 = q; *groups = g; *segs = S;
}

#ifndef GO2_EMU
struct SmoothLossArgs {
  const float *y_a, *w_mu, *b_mu; const uint8_t* w;
  float *gz_a, *part;
  int blocks, T, n, A, K, groups, segs; float scale;          // scale = coef / (blocks (T - 1) n A), for the gradients (the reported loss takes it in fp64)
};

struct SlRow { float4 y, z; bool wt; };          // what a lane loads for one row: its four columns of y_a and (of a row the segment owns) of gz_a, and the row's pair weight

template <int CP>
__global__ void __launch_bounds__(256, CP > 12 ? 1 : 2) go2nn_smooth_loss_kernel(const SmoothLossArgs a, int qp_log2) {
  static_assert(CP <= 16, "16 value slots in the reduce-scatter");
  __shared__ float4 sh[CP + 1][256];
  __shared__ float shs[256 / 16][HB_MAX_C];
  __shared__ double shl[256 / 16];
  const int T = a.T, n = a.n, A = a.A, K = a.K;
  const int QP = 1 << qp_log2, RL = 256 >> qp_log2, SH = qp_log2 - 4;
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
  const float bm = a.b_mu[rc];
  // this workgroup: block b, envs [j0, j0 + RL) of it, rows [t0, t1) of them
  const int seg = blockIdx.x % a.segs, bg = blockIdx.x / a.segs, grp = bg % a.groups, b = bg / a.groups;
  const int t0 = (int)((long long)seg * T / a.segs), t1 = (int)((long long)(seg + 1) * T / a.segs);
  const int j = grp * RL + rl; const bool live = j < n;
  const int jc = live ? j : n - 1;          // (uniform trip count: the exchanges need every lane of a row; env lanes past the end run on a clamped env and are dropped)
  const size_t base = ((size_t)b * T * n + jc) * K + k0;
  auto fetch = [&](int t) {          // (gz_a of the segment's own rows only — a uniform branch —: a halo row's belongs to the neighbouring segment, which writes it)
    SlRow x; const int tc = min(t, T - 1);
    x.y = *reinterpret_cast<const float4*>(a.y_a + base + (size_t)tc * n * K);
    x.z = (t >= t0 && t < t1) ? *reinterpret_cast<const float4*>(a.gz_a + base + (size_t)tc * n * K) : zero;
    x.wt = t < T - 1 && a.w[(size_t)tc * n + jc] != 0;          // the weight of pair (t, t + 1); row T - 1 begins no pair
    return x;
  };
  float4 gb = zero;
  float dbm = 0.f;
  double s_e2 = 0.0;
  // the halo in front: e[t0 - 1] from mu[t0 - 1] and mu[t0]
  SlRow cur = fetch(t0), nx = fetch(t0 + 1);
  float mu_c = ml_head_dot<CP>(cur.y, wq, cq, QP) + bm, e_prev = 0.f;
  if (t0 > 0) {
    const SlRow h = fetch(t0 - 1);
    const float mu_h = ml_head_dot<CP>(h.y, wq, cq, QP) + bm;
    e_prev = (live && role_on && h.wt) ? mu_h - mu_c : 0.f;
  }
  for (int t = t0; t < t1; ++t) {
    const SlRow nn = fetch(t + 2);          // (clamped to row T - 1 past the end: read, never used)
    const float mu_n = ml_head_dot<CP>(nx.y, wq, cq, QP) + bm;          // row t + 1 (behind the last row: the clamped row, weight 0)
    // role c: e = w (mu[t, c] - mu[t + 1, c]);  g = d L / d mu[t, c] = 2 scale (e[t] - e[t - 1])
    const float e = (live && role_on && cur.wt) ? mu_c - mu_n : 0.f;
    const float g = a.scale * 2.f * (e - e_prev);
    if (first) { s_e2 = fma((double)e, (double)e, s_e2); dbm += g; }
    float4 gx = zero;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float ga = __shfl(g, c << SH, QP);
      gx.x = fmaf(ga, wq[c].x, gx.x); gx.y = fmaf(ga, wq[c].y, gx.y); gx.z = fmaf(ga, wq[c].z, gx.z); gx.w = fmaf(ga, wq[c].w, gx.w);
      dw[c].x = fmaf(ga, cur.y.x, dw[c].x); dw[c].y = fmaf(ga, cur.y.y, dw[c].y); dw[c].z = fmaf(ga, cur.y.z, dw[c].z); dw[c].w = fmaf(ga, cur.y.w, dw[c].w);
    }
    float4 d, o;          // ELU' from the output; o: what is added (its column sums are gb_a); gz += gx * ELU' as ONE fma: a single rounding of the new gz
    d.x = cur.y.x > 0.f ? 1.f : cur.y.x + 1.f; d.y = cur.y.y > 0.f ? 1.f : cur.y.y + 1.f; d.z = cur.y.z > 0.f ? 1.f : cur.y.z + 1.f; d.w = cur.y.w > 0.f ? 1.f : cur.y.w + 1.f;
    o.x = gx.x * d.x; o.y = gx.y * d.y; o.z = gx.z * d.z; o.w = gx.w * d.w;
    if (live && on)
      *reinterpret_cast<float4*>(a.gz_a + base + (size_t)t * n * K) = make_float4(fmaf(gx.x, d.x, cur.z.x), fmaf(gx.y, d.y, cur.z.y), fmaf(gx.z, d.z, cur.z.z), fmaf(gx.w, d.w, cur.z.w));
    gb.x += o.x; gb.y += o.y; gb.z += o.z; gb.w += o.w;          // (a dropped env lane: e = 0 throughout, so its o are zeros)
    e_prev = e; mu_c = mu_n; cur = nx; nx = nn;
  }
  // the workgroup's partial row; the env lanes of a column quad are added in a fixed order (go2nn_mirror_loss_kernel's epilogue)
  float* prow = a.part + (size_t)blockIdx.x * mirror_loss_ncols(A, K);
  float* pa = prow + ML_NSTAT;
#pragma unroll
  for (int c = 0; c < CP + 1; ++c) sh[c][threadIdx.x] = c < CP ? dw[c < CP ? c : 0] : gb;
  for (int dd = 1; dd < QP; dd <<= 1) s_e2 += __shfl_xor(s_e2, dd);
  if (cq == 0) shl[rl] = s_e2;
  if (first && role_on) shs[rl][role] = dbm;
  __syncthreads();
  for (int task = threadIdx.x; task < ((CP + 1) << qp_log2); task += 256) {
    const int c = task >> qp_log2, q = task & (QP - 1);
    if ((c < A || c == CP) && 4 * q < K) {
      float4 t4 = sh[c][q];
      for (int i = 1; i < RL; ++i) { const float4 t = sh[c][i * QP + q]; t4.x += t.x; t4.y += t.y; t4.z += t.z; t4.w += t.w; }
      float* o = pa + (size_t)(c < CP ? c : A) * K + 4 * q;
      o[0] = t4.x; o[1] = t4.y; o[2] = t4.z; o[3] = t4.w;
    }
  }
  if ((int)threadIdx.x <= HB_MAX_C) {
    const int t = threadIdx.x;
    if (t == HB_MAX_C) {
      double s = shl[0];
      for (int i = 1; i < RL; ++i) s += shl[i];
      // the workgroup's sum of e^2 as the two halves of its fp64 bits, for go2nn_mirror_loss_finish_kernel (which leaves [L | 0 | 0 | 0] in row 0 and zeros in the others)
      prow[0] = 0.f; prow[1] = 0.f; prow[2] = __int_as_float(__double2hiint(s)); prow[3] = __int_as_float(__double2loint(s));
    } else if (t < A) {
      float s = shs[0][t];
      for (int i = 1; i < RL; ++i) s += shs[i][t];
      pa[(size_t)(A + 1) * K + t] = s;
    }
  }
}

// out[i T n + t n + j] = t N + pi(i n + j), w in the same order; one lane per output element (pi is ~6 hash rounds: nothing next to the launch)
__global__ void __launch_bounds__(256) go2nn_smooth_indices_kernel(int64_t* __restrict__ out, uint8_t* __restrict__ w, const uint8_t* __restrict__ dones, int nmb, int T, int N, int n, int h,
                                                                  const uint32_t* __restrict__ key) {
  const uint32_t seed = key[0], counter = key[1];          // (the counter moves in the launch behind this one)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= T * N) return;
  const int i = r / (T * n), q = r - i * (T * n), t = q / n, jj = q - t * n;
  const int64_t src = (int64_t)t * N + (int64_t)go2_shuffle_index((uint32_t)(i * n + jj), (uint32_t)N, h, seed, counter);
  out[r] = src;
  w[r] = (t < T - 1 && dones[src] == 0) ? 1 : 0;
}
__global__ void go2nn_smooth_counter_kernel(uint32_t* key) { key[1] += 1u; }
#endif  // !GO2_EMU

#ifdef GO2_EMU
// the host build: envs [j0, j1) of block b, every t, into the partial row S, plain loops -> their sum of e^2 (fp64).  An env's sums over t are formed first and then
// added to the row, env by env: chains as short as the device's (a lane's T steps, then the workgroup's env lanes).
static double smooth_loss_host_envs(const Go2nnSmoothLoss& m, int b, int j0, int j1, float scale, float* S) {
  const int T = m.T, n = m.n, A = m.A, K = m.K, nc = mirror_loss_ncols(A, K);
  int QP = 16; while (QP * 4 < K) QP *= 2;
  for (int i = 0; i < nc; ++i) S[i] = 0.f;
  float* pa = S + ML_NSTAT;
  std::vector<float> env((size_t)(A + 1) * K + A);
  double e2 = 0.0;
  auto head = [&](const float* y, float* mu) {          // the dot products in the device kernel's order (go2nn_mirror_loss.h)
    for (int c = 0; c < A; ++c) {
      const float* w = m.w_mu + (size_t)c * K;
      float lane[64];
      for (int q = 0; q < QP; ++q) lane[q] = 4 * q < K ? ML_DOT4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3], w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]) : 0.f;
      for (int d = QP >> 1; d >= 1; d >>= 1) for (int q = 0; q < d; ++q) lane[q] += lane[q + d];
      mu[c] = lane[0] + m.b_mu[c];
    }
  };
  for (int j = j0; j < j1; ++j) {
    float mu_c[HB_MAX_C], mu_n[HB_MAX_C], e_prev[HB_MAX_C], g[HB_MAX_C];
    for (int c = 0; c < A; ++c) { e_prev[c] = 0.f; mu_n[c] = 0.f; }
    for (size_t i = 0; i < env.size(); ++i) env[i] = 0.f;
    float* ea = env.data();
    head(m.y_a + ((size_t)b * T * n + j) * K, mu_c);
    for (int t = 0; t < T; ++t) {
      const size_t r = (size_t)b * T * n + (size_t)t * n + j;
      const float* y = m.y_a + r * K; float* gz = m.gz_a + r * K;
      const bool wt = t < T - 1 && m.w[(size_t)t * n + j] != 0;
      if (t < T - 1) head(y + (size_t)n * K, mu_n);
      for (int c = 0; c < A; ++c) {
        const float e = wt ? mu_c[c] - mu_n[c] : 0.f;
        e2 = fma((double)e, (double)e, e2);
        g[c] = scale * 2.f * (e - e_prev[c]);
        ea[(size_t)(A + 1) * K + c] += g[c];
        e_prev[c] = e; mu_c[c] = mu_n[c];
      }
      for (int k = 0; k < K; ++k) {
        float gx = 0.f; for (int c = 0; c < A; ++c) gx = fmaf(g[c], m.w_mu[(size_t)c * K + k], gx);
        const float d = y[k] > 0.f ? 1.f : y[k] + 1.f;
        gz[k] = fmaf(gx, d, gz[k]);
        for (int c = 0; c < A; ++c) ea[(size_t)c * K + k] = fmaf(g[c], y[k], ea[(size_t)c * K + k]);
        ea[(size_t)A * K + k] += gx * d;
      }
    }
    for (size_t i = 0; i < env.size(); ++i) pa[i] += ea[i];
  }
  return e2;
}
#endif

extern "C" {

int32_t go2nn_smooth_loss_cols(int32_t A, int32_t K) {
  if (!smooth_loss_ok(1, 2, 1, A, K)) FAIL(GO2NN_EINVAL, "smooth loss: 1 <= A <= %d, K a multiple of 4 up to 256", HB_MAX_C);
  return mirror_loss_ncols(A, K);
}

int32_t go2nn_smooth_loss_rows(int32_t blocks, int32_t T, int32_t n, int32_t A, int32_t K) {
  if (!smooth_loss_ok(blocks, T, n, A, K)) FAIL(GO2NN_EINVAL, "smooth loss: bad shape (blocks %d, T %d, n %d, A %d, K %d)", blocks, T, n, A, K);
#ifdef GO2_EMU
  return blocks * ((n + SL_EMU_ENVS - 1) / SL_EMU_ENVS);
#else
  int q, g, S; smooth_loss_shape(blocks, T, n, K, &q, &g, &S); return blocks * g * S;
#endif
}

int go2nn_smooth_loss_set_segments(int32_t segments) {
  if (segments < 0) FAIL(GO2NN_EINVAL, "smooth loss: a segment count >= 1, or 0 for the automatic choice");
  g_smooth_segments = segments;
  return 0;
}

int go2nn_smooth_loss(const Go2nnSmoothLoss* m, void* stream) {
  if (!m) FAIL(GO2NN_EINVAL, "smooth loss: a null argument struct");
  if (!smooth_loss_ok(m->blocks, m->T, m->n, m->A, m->K))
    FAIL(GO2NN_EINVAL, "smooth loss: bad shape (1 <= blocks %d <= 2, T %d >= 2, n %d >= 1, 1 <= A %d <= %d, K %d a multiple of 4 up to 256)", m->blocks, m->T, m->n, m->A, HB_MAX_C, m->K);
  if (!m->y_a || !m->w_mu || !m->b_mu || !m->w || !m->gz_a || !m->partials) FAIL(GO2NN_EINVAL, "smooth loss: a null pointer");
  if (smooth_loss_elems(m->blocks, m->T, m->n, m->K) >= (1LL << 31)) FAIL(GO2NN_EINVAL, "smooth loss: %d x %d x %d x %d elements do not fit 31 bits", m->blocks, m->T, m->n, m->K);
  if (!(m->coef >= 0.f) || !(m->coef <= 3.0e38f)) FAIL(GO2NN_EINVAL, "smooth loss: a finite coefficient >= 0");
  const int blocks = m->blocks, T = m->T, n = m->n, A = m->A, K = m->K;
  const float scale = m->coef / ((float)blocks * (float)(T - 1) * (float)n * (float)A);
  const double lscale = (double)m->coef / ((double)blocks * (double)(T - 1) * (double)n * (double)A);
#ifdef GO2_EMU
  (void)stream;
  double e2 = 0.0;
  int row = 0;
  for (int b = 0; b < blocks; ++b)
    for (int j0 = 0; j0 < n; j0 += SL_EMU_ENVS, ++row)
      e2 += smooth_loss_host_envs(*m, b, j0, j0 + SL_EMU_ENVS < n ? j0 + SL_EMU_ENVS : n, scale, m->partials + (size_t)row * mirror_loss_ncols(A, K));
  m->partials[0] = (float)(lscale * e2);          // the reported loss: fp64 to the end, rounded once, in row 0 (the other rows hold 0)
#else
  SmoothLossArgs a;
  a.y_a = m->y_a; a.w_mu = m->w_mu; a.b_mu = m->b_mu; a.w = m->w; a.gz_a = m->gz_a; a.part = m->partials;
  a.blocks = blocks; a.T = T; a.n = n; a.A = A; a.K = K; a.scale = scale;
  int q; smooth_loss_shape(blocks, T, n, K, &q, &a.groups, &a.segs);
  const int nwg = blocks * a.groups * a.segs;
  hipStream_t st = (hipStream_t)stream;
  if (A <= 4)       hipLaunchKernelGGL(go2nn_smooth_loss_kernel<4>,  dim3(nwg), dim3(256), 0, st, a, q);
  else if (A <= 8)  hipLaunchKernelGGL(go2nn_smooth_loss_kernel<8>,  dim3(nwg), dim3(256), 0, st, a, q);
  else if (A <= 12) hipLaunchKernelGGL(go2nn_smooth_loss_kernel<12>, dim3(nwg), dim3(256), 0, st, a, q);
  else              hipLaunchKernelGGL(go2nn_smooth_loss_kernel<16>, dim3(nwg), dim3(256), 0, st, a, q);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_mirror_loss_finish_kernel, dim3(1), dim3(256), 0, st, m->partials, nwg, mirror_loss_ncols(A, K), lscale);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_smooth_indices(int64_t* out, uint8_t* w, const uint8_t* dones, int32_t nmb, int32_t T, int32_t N, uint32_t* key_state, void* stream) {
  if (!out || !w || !dones || !key_state) FAIL(GO2NN_EINVAL, "smooth indices: a null pointer");
  if (nmb < 1 || T < 2 || N < 1 || N % nmb != 0) FAIL(GO2NN_EINVAL, "smooth indices: %d envs in %d mini-batches of whole envs, T %d >= 2", N, nmb, T);
  if ((long long)T * N >= (1LL << 31)) FAIL(GO2NN_EINVAL, "smooth indices: %d x %d rows do not fit 31 bits", T, N);
  const int n = N / nmb, h = go2_shuffle_half_bits((uint32_t)N);
#ifdef GO2_EMU
  (void)stream;
  for (int i = 0; i < nmb; ++i) for (int t = 0; t < T; ++t) for (int j = 0; j < n; ++j) {
    const size_t r = ((size_t)i * T + t) * n + j;
    const int64_t src = (int64_t)t * N + (int64_t)go2_shuffle_index((uint32_t)(i * n + j), (uint32_t)N, h, key_state[0], key_state[1]);
    out[r] = src;
    w[r] = (t < T - 1 && dones[src] == 0) ? 1 : 0;
  }
  key_state[1] += 1u;
#else
  hipLaunchKernelGGL(go2nn_smooth_indices_kernel, dim3((T * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, w, dones, nmb, T, N, n, h, key_state);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_smooth_counter_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, key_state);          // a replayed graph draws a new permutation every time
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_SMOOTH_LOSS_H
