// go2nn_diag.h — the update's diagnostics (include/go2nn.h: go2nn_ppo_diag, go2nn_grad_sqnorm, the enum GO2NN_DIAG_*, added within ABI 7;
// rsl_rl/algorithms/_diag.py, `algorithm.diagnostics`).  Included at the end of go2nn_impl.cpp (FAIL, HIPCHK, HB_MAX_C, EVAL_FN are its helpers).
//
// In graph mode the action mean, the log-probability, the ratio and the value of a mini-batch row never exist as tensors: go2nn_ppo_heads forms them in registers.  The
// figures a PPO user reads (clip fraction, KL, explained variance, ...) therefore need a pass of their own: go2nn_ppo_diag, behind the heads on the same stream, READS
// what the heads read — y_a, y_c [B, K] and the row inputs — and writes only its own partial rows and table.  gz_*, the heads' partials and every .grad are not touched.
//   the pass    thread = (k quad cq, row lane rl) as in go2nn_ppo_heads_kernel, the heads' own dot-product expressions and reduce-scatter, so mu and v are the heads'
//               fp32 values; the row's lp and kl go round the row's lanes; then EVERY lane of the row holds the row's 18 fp32 terms (diag_terms below) and lane cq < 16
//               keeps column cq of both segments in two fp64 registers (lanes 0 and 1 also the ratio's maximum and minimum): no per-lane table of 36 doubles, no
//               dynamic register indexing.  A workgroup owns GO2NN_DIAG_PASS_ROWS consecutive rows whatever B is, so a partial row means the same rows on every
//               launch; its row lanes meet in 4.5 KB of LDS behind one barrier and are combined in increasing order.  No atomics.
//   the finish  one block: thread (segment, column) combines the partial rows in increasing order, writes table[*cursor] and lane 0 advances the cursor with a plain
//               vector store (the one-lane counters of go2nn_sensor_rand.h): the slot is a device-side value, so ONE captured launch pair serves every replay.
// go2nn_grad_sqnorm: the squared L2 norm of up to 48 gradient tensors in front of the clip + Adam call (go2sim_adam_clip_step keeps its norm to itself and is not
// touched).  Stage 1: a workgroup per GO2NN_GRAD_SQNORM_CHUNK floats of a tensor (pointers, sizes and first-block indices by value in the kernel arguments), x * x
// formed and added in fp64 (the square of an fp32 value is exact in fp64), the lanes' sums through the wave's xor butterfly and the four waves in order; stage 2: one
// block adds the per-workgroup doubles (a thread's in increasing order, then a fixed tree) and writes out[*cursor].
// Compiled for gfx950 (hipcc -O3; build.py kernel_resources reads the code object's notes): go2nn_ppo_diag_kernel<12> (the Go2's 12 actions) 123 VGPRs, 106 SGPRs,
// 4608 B of LDS, 4 waves per SIMD; <4> 84 VGPRs, 5 waves; <16> 143 VGPRs, 3 waves (<8> lies between); its finish 28 VGPRs, 43 SGPRs, 36864 B of LDS; go2nn_grad_sq_kernel 38
// VGPRs, 23 SGPRs, 32 B of LDS (the pointer table stays in the kernel-argument segment: scalar loads, no copy to the stack); its finish 10 VGPRs, 20 SGPRs, 2048 B.
// Scratch is 0 and nothing spills in any of them.
// What was tried: the first shape kept all 2 x 18 fp64 accumulators on the row's first lane (72 VGPRs of accumulators that idle on the row's other lanes, and a
// dynamically indexed segment would have gone to scratch); spreading the columns over the row's lanes costs 15 selects per row and leaves four fp64 registers per lane.
// The finish is serial over the partial rows (512 at 24576 rows) on purpose — the table promises increasing order.  Measured on one MI355X at 24576 rows x 12
// actions x 128 (a kernel trace of tools/update_diag_bench.py's launch loop: average device time per launch): the pass 16 us; the finish 24 us; the two stages of
// go2nn_grad_sqnorm over the 17 gradient tensors of go2_flat 5 + 2 us; a device-to-device copy of y_a and y_c 8 us.  The finish went through three shapes: (1) one
// wave reading the partial rows straight from memory in the serial loop, one memory latency per row: the call took 175 us; (2) the rows staged in LDS tiles but
// combined through one function that selects sum / max / min per column at run time: 122 us for the finish alone — the select chain and the LDS latency sat on the
// dependent chain of every row; (3) one plain chain per column kind, unrolled by eight: 35 us, the three kinds' chains one after the other in one wave; now each kind
// has a wave of its own: 24 us.  What is left is 512 dependent fp64 operations behind four tile loads and eight barriers.
// The host build (GO2_EMU) runs the same term / combine functions in plain loops: one partial row per GO2NN_DIAG_PASS_ROWS rows, the dot products in the order of the
// host build's go2nn_ppo_heads.
#ifndef GO2NN_DIAG_H
#define GO2NN_DIAG_H

#define DG_NUM GO2NN_DIAG_NUM
#define DG_ROWS GO2NN_DIAG_PASS_ROWS
#define DG_INF __builtin_huge_val()

static inline int ppo_diag_ok(int B, int A, int K) { return B > 0 && A >= 1 && A <= HB_MAX_C && K >= 4 && K <= 256 && (K & 3) == 0; }

// column kinds: 0 a sum, 1 a maximum, 2 a minimum
EVAL_FN int diag_kind(int c) { return (c == GO2NN_DIAG_KL_MAX || c == GO2NN_DIAG_VERR_ABS_MAX || c == GO2NN_DIAG_RATIO_MAX) ? 1 : (c == GO2NN_DIAG_RATIO_MIN ? 2 : 0); }
EVAL_FN double diag_init(int c) { const int k = diag_kind(c); return k == 1 ? -DG_INF : (k == 2 ? DG_INF : 0.0); }
EVAL_FN double diag_combine(int c, double acc, double x) { const int k = diag_kind(c); return k == 1 ? fmax(acc, x) : (k == 2 ? fmin(acc, x) : acc + x); }

// the 18 fp32 terms of one row (include/go2nn.h) from its log-probability, KL, old log-probability, advantage, value, old value and return
EVAL_FN void diag_terms(float lp, float kl, float olp, float ad, float v, float tv, float rt, float clip, float* t) {
  const float lr = lp - olp, ratio = expf(lr), err = rt - v, dv = v - tv;
  t[GO2NN_DIAG_ROWS] = 1.f;
  t[GO2NN_DIAG_RATIO_CLIPPED] = fabsf(ratio - 1.f) > clip ? 1.f : 0.f;
  t[GO2NN_DIAG_RATIO_SUM] = ratio;
  t[GO2NN_DIAG_LOGRATIO_SUM] = lr;
  t[GO2NN_DIAG_K3_SUM] = (ratio - 1.f) - lr;
  t[GO2NN_DIAG_KL_SUM] = kl;
  t[GO2NN_DIAG_KL_MAX] = kl;
  t[GO2NN_DIAG_ADV_SUM] = ad;
  t[GO2NN_DIAG_ADV_SQ] = ad * ad;
  t[GO2NN_DIAG_ADV_POS] = ad > 0.f ? 1.f : 0.f;
  t[GO2NN_DIAG_VERR_SUM] = err;
  t[GO2NN_DIAG_VERR_SQ] = err * err;
  t[GO2NN_DIAG_VERR_ABS_MAX] = fabsf(err);
  t[GO2NN_DIAG_RET_SUM] = rt;
  t[GO2NN_DIAG_RET_SQ] = rt * rt;
  t[GO2NN_DIAG_VALUE_CLIPPED] = fabsf(dv) > clip ? 1.f : 0.f;
  t[GO2NN_DIAG_RATIO_MAX] = ratio;
  t[GO2NN_DIAG_RATIO_MIN] = ratio;
}

#ifndef GO2_EMU
struct PpoDiagArgs {
  const float *y_a, *y_c, *w_mu, *b_mu, *w_v, *b_v, *std_, *actions, *old_mu, *old_sigma, *old_logp, *adv, *old_values, *returns;
  double* part;
  int B, A, K, split, segs; float clip;
};

// what a lane loads for one row (go2nn_ppo_heads_kernel's PhRow)
struct DgRow { float4 ya, yc; float act, omu, osg, olp, ad, tv, rt; };

template <int CP>
__global__ void __launch_bounds__(256) go2nn_ppo_diag_kernel(const PpoDiagArgs a, int qp_log2) {
  static_assert(CP <= 16, "16 value slots in the reduce-scatter");
  static_assert(DG_NUM == 18, "lane cq < 16 keeps column cq, lanes 0 and 1 also columns 16 and 17");
  __shared__ double shd[16][2][DG_NUM];          // (QP >= 16: at most 16 row lanes)
  const int B = a.B, A = a.A, K = a.K;
  const int QP = 1 << qp_log2, RL = 256 >> qp_log2, SH = qp_log2 - 4;          // QP >= 16 lanes per row; lane role c = cq >> SH (2^SH lanes share a role)
  const int cq = threadIdx.x & (QP - 1), rl = threadIdx.x >> qp_log2;
  const bool on = 4 * cq < K;
  const int k0 = on ? 4 * cq : 0;
  const int role = cq >> SH; const bool first = (cq & ((1 << SH) - 1)) == 0, role_on = role < A;
  const int rc = role_on ? role : 0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float LOG2PI = 1.8378770664093453f;
  float4 wq[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float4 t = *reinterpret_cast<const float4*>(a.w_mu + (size_t)min(c, A - 1) * K + k0);
    wq[c] = (on && c < A) ? t : zero;
  }
  const float sg = a.std_[rc], ls = logf(sg), isg2 = 1.f / (sg * sg), bm = a.b_mu[rc];
  const float4 wv = on ? *reinterpret_cast<const float4*>(a.w_v + k0) : zero;
  const float bv = a.b_v[0];
  const int col = cq & 15;
  const bool is_max = diag_kind(col) == 1, odd = cq & 1;
  double a0[2], a1[2];
  a0[0] = a0[1] = is_max ? -DG_INF : 0.0;          // (columns 0 .. 15 hold sums and maxima)
  a1[0] = a1[1] = odd ? DG_INF : -DG_INF;          // lane 0: the ratio's maximum, lane 1: its minimum
  const int r0 = blockIdx.x * DG_ROWS, r1 = min(B, r0 + DG_ROWS);          // (r0 < B: the grid is ceil(B / DG_ROWS))
  auto fetch = [&](int rb) {
    DgRow x; const int r = min(rb + rl, r1 - 1);
    x.ya = *reinterpret_cast<const float4*>(a.y_a + (size_t)r * K + k0); x.yc = *reinterpret_cast<const float4*>(a.y_c + (size_t)r * K + k0);
    const size_t k = (size_t)r * A + rc;
    x.act = a.actions[k]; x.omu = a.old_mu[k]; x.osg = a.old_sigma[k]; x.olp = a.old_logp[r]; x.ad = a.adv[r]; x.tv = a.old_values[r]; x.rt = a.returns[r];
    return x;
  };
  DgRow nx = fetch(r0);
  for (int rb = r0; rb < r1; rb += RL) {          // (uniform trip count: the exchanges need every lane of a row; rows past the end run on a clamped row and are dropped)
    const DgRow x = nx;
    nx = fetch(min(rb + RL, r1 - 1));
    const bool live = rb + rl < r1;
    const float4 ya = x.ya, yc = x.yc;
    // the heads forward, literally go2nn_ppo_heads_kernel's: the same products, the same reduce-scatter, the same order
    float pm[16], pv = yc.x * wv.x + yc.y * wv.y + yc.z * wv.z + yc.w * wv.w;
#pragma unroll
    for (int c = 0; c < 16; ++c) pm[c] = c < CP ? ya.x * wq[c < CP ? c : 0].x + ya.y * wq[c < CP ? c : 0].y + ya.z * wq[c < CP ? c : 0].z + ya.w * wq[c < CP ? c : 0].w : 0.f;
    float mu_r;
    {
      const int d3 = QP >> 1, d2 = QP >> 2, d1 = QP >> 3, d0 = QP >> 4;
      float p8[8], p4[4], p2[2];
      { const bool up = cq & d3;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float keep = up ? pm[8 + i] : pm[i], send = up ? pm[i] : pm[8 + i]; p8[i] = keep + __shfl_xor(send, d3); } }
      { const bool up = cq & d2;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float keep = up ? p8[4 + i] : p8[i], send = up ? p8[i] : p8[4 + i]; p4[i] = keep + __shfl_xor(send, d2); } }
      { const bool up = cq & d1;
#pragma unroll
        for (int i = 0; i < 2; ++i) { const float keep = up ? p4[2 + i] : p4[i], send = up ? p4[i] : p4[2 + i]; p2[i] = keep + __shfl_xor(send, d1); } }
      { const bool up = cq & d0; const float keep = up ? p2[1] : p2[0], send = up ? p2[0] : p2[1]; mu_r = keep + __shfl_xor(send, d0); }
      for (int d = d0 >> 1; d >= 1; d >>= 1) mu_r += __shfl_xor(mu_r, d);
    }
    for (int d = 1; d < QP; d <<= 1) pv += __shfl_xor(pv, d);
    const float v = pv + bv;
    const float m = mu_r + bm, dd = x.act - m, dm = x.omu - m;
    float lp = (role_on && first) ? -dd * dd * (0.5f * isg2) - ls - 0.5f * LOG2PI : 0.f;
    float kl = (role_on && first) ? logf(sg / x.osg + 1e-5f) + (x.osg * x.osg + dm * dm) * (0.5f * isg2) - 0.5f : 0.f;
    for (int d = 1; d < QP; d <<= 1) { lp += __shfl_xor(lp, d); kl += __shfl_xor(kl, d); }
    // every lane of the row now holds the row's scalars: its 18 terms, of which this lane keeps column `col` (and the ratio)
    float t[DG_NUM];
    diag_terms(lp, kl, x.olp, x.ad, v, x.tv, x.rt, a.clip, t);
    float term = t[0];
#pragma unroll
    for (int c = 1; c < 16; ++c) term = col == c ? t[c] : term;
    const double td = (double)term, rd = (double)t[GO2NN_DIAG_RATIO_MAX];
    const int seg = (a.split > 0 && rb + rl >= a.split) ? 1 : 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bool hit = live && seg == s;
      const double n0 = is_max ? fmax(a0[s], td) : a0[s] + td, n1 = odd ? fmin(a1[s], rd) : fmax(a1[s], rd);
      a0[s] = hit ? n0 : a0[s]; a1[s] = hit ? n1 : a1[s];
    }
  }
  // the workgroup's partial rows [segs][18]: the row lanes of a column are combined in increasing order
  if (cq < 16) { shd[rl][0][cq] = a0[0]; shd[rl][1][cq] = a0[1]; }
  if (cq < 2) { shd[rl][0][16 + cq] = a1[0]; shd[rl][1][16 + cq] = a1[1]; }
  __syncthreads();
  if ((int)threadIdx.x < a.segs * DG_NUM) {
    const int s = threadIdx.x / DG_NUM, c = threadIdx.x % DG_NUM;
    double acc = shd[0][s][c];
    for (int j = 1; j < RL; ++j) acc = diag_combine(c, acc, shd[j][s][c]);
    a.part[((size_t)blockIdx.x * a.segs + s) * DG_NUM + c] = acc;
  }
}

// one block: the partial rows come into LDS a tile of DG_FIN_TILE rows at a time — every lane's loads are independent and dense, so they are all in flight at once —
// and one lane per (segment, column) combines the tile's rows in increasing order from LDS; the slot is the device-side cursor
#define DG_FIN_TILE 128
__global__ void __launch_bounds__(256) go2nn_ppo_diag_finish_kernel(const double* __restrict__ part, int nrows, int segs, double* __restrict__ table, int32_t* cursor, int slots) {
  __shared__ double sh[DG_FIN_TILE * 2 * DG_NUM];
  const int slot = *cursor, ncol = segs * DG_NUM, tid = threadIdx.x;
  const bool ok = slot >= 0 && slot < slots;          // (uniform: every lane read the same cursor)
  if (ok) {
    // wave w owns the columns of kind w (0: the sums, 1: the maxima, 2: the minimum), lane l its l-th such column of segment l / (columns of that kind): each wave
    // runs ONE plain dependent chain, the three side by side (in one wave the three kinds' chains ran one after the other: 35 us of the call's 51)
    const int kind = tid >> 6, lane = tid & 63;
    int per = 0;
    for (int c = 0; c < DG_NUM; ++c) per += diag_kind(c) == kind ? 1 : 0;
    const bool mine = kind < 3 && lane < segs * per;
    int j = -1;          // the table column (segment * DG_NUM + column) this lane combines
    if (mine) {
      int want = lane % per, seen = 0;
      for (int c = 0; c < DG_NUM; ++c)
        if (diag_kind(c) == kind) { if (seen == want) j = (lane / per) * DG_NUM + c; ++seen; }
    }
    double acc = kind == 1 ? -DG_INF : (kind == 2 ? DG_INF : 0.0);
    for (int r0 = 0; r0 < nrows; r0 += DG_FIN_TILE) {
      const int nr = min(DG_FIN_TILE, nrows - r0), n = nr * ncol;
      for (int i = tid; i < n; i += 256) sh[i] = part[(size_t)r0 * ncol + i];
      __syncthreads();
      if (mine) {          // (the LDS reads of eight rows are issued ahead of the eight dependent operations)
        const double* col = sh + j;
        if (kind == 0) {
#pragma unroll 8
          for (int r = 0; r < nr; ++r) acc += col[r * ncol];
        } else if (kind == 1) {
#pragma unroll 8
          for (int r = 0; r < nr; ++r) acc = fmax(acc, col[r * ncol]);
        } else {
#pragma unroll 8
          for (int r = 0; r < nr; ++r) acc = fmin(acc, col[r * ncol]);
        }
      }
      __syncthreads();
    }
    if (mine) table[(size_t)slot * ncol + j] = acc;
  }
  __syncthreads();          // (every lane has read the cursor)
  if (ok && tid == 0) *cursor = slot + 1;
}

struct GradSqArgs { const float* g[GO2NN_GRAD_SQNORM_MAX]; int n[GO2NN_GRAD_SQNORM_MAX]; int blk0[GO2NN_GRAD_SQNORM_MAX + 1]; int count; };

// stage 1: workgroup b = chunk (b - blk0[i]) of tensor i
__global__ void __launch_bounds__(256) go2nn_grad_sq_kernel(const GradSqArgs a, double* __restrict__ part) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  int i = 0;
  while (i + 1 < a.count && b >= a.blk0[i + 1]) ++i;
  const float* g = a.g[i];
  const int n = a.n[i], base = (b - a.blk0[i]) * GO2NN_GRAD_SQNORM_CHUNK;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < GO2NN_GRAD_SQNORM_CHUNK / 256; ++j) {
    const int idx = base + j * 256 + (int)threadIdx.x;
    const double x = idx < n ? (double)g[idx] : 0.0;
    s = fma(x, x, s);
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[b] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage 2: one block
__global__ void __launch_bounds__(256) go2nn_grad_sq_finish_kernel(const double* __restrict__ part, int nrows, double* __restrict__ out, int32_t* cursor, int slots) {
  __shared__ double sh[256];
  const int slot = *cursor;
  double s = 0.0;
  for (int r = threadIdx.x; r < nrows; r += 256) s += part[r];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0 && slot >= 0 && slot < slots) { out[slot] = sh[0]; *cursor = slot + 1; }
}
#endif  // !GO2_EMU

// a chunk's element index base + j * 256 + lane is an int: the last chunk of a tensor must not carry it past INT_MAX
#define GSQ_MAX_NUMEL (0x7fffffff - GO2NN_GRAD_SQNORM_CHUNK)
static int grad_sq_blocks(const int32_t* numel, int count, int* blk0) {
  long long b = 0;
  for (int i = 0; i < count; ++i) {
    if (blk0) blk0[i] = (int)b;
    b += ((long long)numel[i] + GO2NN_GRAD_SQNORM_CHUNK - 1) / GO2NN_GRAD_SQNORM_CHUNK;
  }
  if (blk0) blk0[count] = (int)b;
  return b < (1LL << 30) ? (int)b : -1;
}

extern "C" {

int32_t go2nn_ppo_diag_rows(int32_t B, int32_t A, int32_t K) {
  if (!ppo_diag_ok(B, A, K)) FAIL(GO2NN_EINVAL, "ppo diag: bad shape (B %d rows >= 1, 1 <= A %d <= %d, K %d a multiple of 4 up to 256)", B, A, HB_MAX_C, K);
  return (B + DG_ROWS - 1) / DG_ROWS;
}

int go2nn_ppo_diag(const Go2nnPpoDiag* h, void* stream) {
  if (!h) FAIL(GO2NN_EINVAL, "ppo diag: a null argument struct");
  if (!ppo_diag_ok(h->B, h->A, h->K)) FAIL(GO2NN_EINVAL, "ppo diag: bad shape (B %d rows >= 1, 1 <= A %d <= %d, K %d a multiple of 4 up to 256)", h->B, h->A, HB_MAX_C, h->K);
  const void* ptrs[] = {h->y_a, h->y_c, h->w_mu, h->b_mu, h->w_v, h->b_v, h->std, h->actions, h->old_mu, h->old_sigma, h->old_logp, h->adv, h->old_values, h->returns,
                        h->partials, h->table, h->cursor};
  for (const void* q : ptrs) if (!q) FAIL(GO2NN_EINVAL, "ppo diag: a null pointer");
  if (h->surrogate_split < 0 || h->surrogate_split >= h->B) FAIL(GO2NN_EINVAL, "ppo diag: surrogate_split %d outside [0, %d)", h->surrogate_split, h->B);
  if (h->slots < 1) FAIL(GO2NN_EINVAL, "ppo diag: %d slots", h->slots);
  if ((long long)h->B * h->K >= (1LL << 31)) FAIL(GO2NN_EINVAL, "ppo diag: %d x %d elements do not fit 31 bits", h->B, h->K);
  const int B = h->B, A = h->A, K = h->K, split = h->surrogate_split, segs = split > 0 ? 2 : 1, nrows = (B + DG_ROWS - 1) / DG_ROWS;
#ifdef GO2_EMU
  (void)stream;
  const float LOG2PI = 1.8378770664093453f;
  for (int w = 0; w < nrows; ++w) {          // one partial row per DG_ROWS rows
    double* P = h->partials + (size_t)w * segs * DG_NUM;
    for (int s = 0; s < segs; ++s) for (int c = 0; c < DG_NUM; ++c) P[s * DG_NUM + c] = diag_init(c);
    const int r1 = (w + 1) * DG_ROWS < B ? (w + 1) * DG_ROWS : B;
    for (int r = w * DG_ROWS; r < r1; ++r) {
      const float* ya = h->y_a + (size_t)r * K; const float* yc = h->y_c + (size_t)r * K;
      float v = h->b_v[0], lp = 0.f, kl = 0.f;          // (the host build's go2nn_ppo_heads: one fma chain from the bias)
      for (int k = 0; k < K; ++k) v = fmaf(yc[k], h->w_v[k], v);
      for (int c = 0; c < A; ++c) {
        float m = h->b_mu[c]; for (int k = 0; k < K; ++k) m = fmaf(ya[k], h->w_mu[(size_t)c * K + k], m);
        const float sg = h->std[c], d = h->actions[(size_t)r * A + c] - m, so = h->old_sigma[(size_t)r * A + c], dm = h->old_mu[(size_t)r * A + c] - m, isg2 = 1.f / (sg * sg);
        lp += -d * d * (0.5f * isg2) - logf(sg) - 0.5f * LOG2PI; kl += logf(sg / so + 1e-5f) + (so * so + dm * dm) * (0.5f * isg2) - 0.5f;
      }
      float t[DG_NUM];
      diag_terms(lp, kl, h->old_logp[r], h->adv[r], v, h->old_values[r], h->returns[r], h->clip, t);
      double* S = P + ((split > 0 && r >= split) ? DG_NUM : 0);
      for (int c = 0; c < DG_NUM; ++c) S[c] = diag_combine(c, S[c], (double)t[c]);
    }
  }
  const int slot = *h->cursor;
  if (slot >= 0 && slot < h->slots) {
    for (int j = 0; j < segs * DG_NUM; ++j) {
      double acc = diag_init(j % DG_NUM);
      for (int w = 0; w < nrows; ++w) acc = diag_combine(j % DG_NUM, acc, h->partials[(size_t)w * segs * DG_NUM + j]);
      h->table[(size_t)slot * segs * DG_NUM + j] = acc;
    }
    *h->cursor = slot + 1;
  }
#else
  PpoDiagArgs a;
  a.y_a = h->y_a; a.y_c = h->y_c; a.w_mu = h->w_mu; a.b_mu = h->b_mu; a.w_v = h->w_v; a.b_v = h->b_v; a.std_ = h->std; a.actions = h->actions; a.old_mu = h->old_mu;
  a.old_sigma = h->old_sigma; a.old_logp = h->old_logp; a.adv = h->adv; a.old_values = h->old_values; a.returns = h->returns; a.part = h->partials;
  a.B = B; a.A = A; a.K = K; a.split = split; a.segs = segs; a.clip = h->clip;
  int q = 4;
  while ((1 << q) * 4 < K) ++q;          // (QP = 16, 32 or 64 lanes per row: RL = 16, 8 or 4 row lanes, each a divisor of DG_ROWS)
  hipStream_t st = (hipStream_t)stream;
  if (A <= 4)       hipLaunchKernelGGL(go2nn_ppo_diag_kernel<4>,  dim3(nrows), dim3(256), 0, st, a, q);
  else if (A <= 8)  hipLaunchKernelGGL(go2nn_ppo_diag_kernel<8>,  dim3(nrows), dim3(256), 0, st, a, q);
  else if (A <= 12) hipLaunchKernelGGL(go2nn_ppo_diag_kernel<12>, dim3(nrows), dim3(256), 0, st, a, q);
  else              hipLaunchKernelGGL(go2nn_ppo_diag_kernel<16>, dim3(nrows), dim3(256), 0, st, a, q);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_ppo_diag_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)h->partials, nrows, segs, h->table, h->cursor, h->slots);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int32_t go2nn_grad_sqnorm_rows(const int32_t* host_numel, int32_t count) {
  if (!host_numel) FAIL(GO2NN_EINVAL, "grad sqnorm: a null pointer");
  if (count < 1 || count > GO2NN_GRAD_SQNORM_MAX) FAIL(GO2NN_EINVAL, "grad sqnorm: %d tensors outside [1, %d]", count, GO2NN_GRAD_SQNORM_MAX);
  for (int i = 0; i < count; ++i) if (host_numel[i] < 1 || host_numel[i] > GSQ_MAX_NUMEL) FAIL(GO2NN_EINVAL, "grad sqnorm: tensor %d has %d elements (1 .. %d)", i, host_numel[i], GSQ_MAX_NUMEL);
  const int b = grad_sq_blocks(host_numel, count, nullptr);
  if (b < 0) FAIL(GO2NN_EINVAL, "grad sqnorm: too many elements");
  return b;
}

int go2nn_grad_sqnorm(const float* const* host_grads, const int32_t* host_numel, int32_t count, double* partials, double* out, int32_t* cursor, int32_t slots, void* stream) {
  if (!host_grads || !host_numel || !partials || !out || !cursor) FAIL(GO2NN_EINVAL, "grad sqnorm: a null pointer");
  if (count < 1 || count > GO2NN_GRAD_SQNORM_MAX) FAIL(GO2NN_EINVAL, "grad sqnorm: %d tensors outside [1, %d]", count, GO2NN_GRAD_SQNORM_MAX);
  if (slots < 1) FAIL(GO2NN_EINVAL, "grad sqnorm: %d slots", slots);
  for (int i = 0; i < count; ++i) {
    if (host_numel[i] < 1 || host_numel[i] > GSQ_MAX_NUMEL) FAIL(GO2NN_EINVAL, "grad sqnorm: tensor %d has %d elements (1 .. %d)", i, host_numel[i], GSQ_MAX_NUMEL);
    if (!host_grads[i]) FAIL(GO2NN_EINVAL, "grad sqnorm: tensor %d is a null pointer", i);
  }
  int blk0[GO2NN_GRAD_SQNORM_MAX + 1];
  const int nb = grad_sq_blocks(host_numel, count, blk0);
  if (nb < 0) FAIL(GO2NN_EINVAL, "grad sqnorm: too many elements");
#ifdef GO2_EMU
  (void)stream;
  for (int i = 0; i < count; ++i)
    for (int b = blk0[i]; b < blk0[i + 1]; ++b) {          // the device's order: 256 lanes stride the chunk, each wave's xor butterfly, the four waves in order
      const int base = (b - blk0[i]) * GO2NN_GRAD_SQNORM_CHUNK;
      double lane[256], w4[4];
      for (int t = 0; t < 256; ++t) {
        double s = 0.0;
        for (int j = 0; j < GO2NN_GRAD_SQNORM_CHUNK / 256; ++j) { const int idx = base + j * 256 + t; const double x = idx < host_numel[i] ? (double)host_grads[i][idx] : 0.0; s = fma(x, x, s); }
        lane[t] = s;
      }
      for (int w = 0; w < 4; ++w) {
        double* L = lane + 64 * w;
        for (int d = 32; d >= 1; d >>= 1) { double nxt[64]; for (int l = 0; l < 64; ++l) nxt[l] = L[l] + L[l ^ d]; for (int l = 0; l < 64; ++l) L[l] = nxt[l]; }
        w4[w] = L[0];
      }
      partials[b] = ((w4[0] + w4[1]) + w4[2]) + w4[3];
    }
  double sh[256];
  for (int t = 0; t < 256; ++t) { double s = 0.0; for (int r = t; r < nb; r += 256) s += partials[r]; sh[t] = s; }
  for (int d = 128; d >= 1; d >>= 1) for (int t = 0; t < d; ++t) sh[t] += sh[t + d];
  const int slot = *cursor;
  if (slot >= 0 && slot < slots) { out[slot] = sh[0]; *cursor = slot + 1; }
#else
  GradSqArgs a;
  for (int i = 0; i < GO2NN_GRAD_SQNORM_MAX; ++i) { a.g[i] = i < count ? host_grads[i] : nullptr; a.n[i] = i < count ? host_numel[i] : 0; }
  for (int i = 0; i <= GO2NN_GRAD_SQNORM_MAX; ++i) a.blk0[i] = blk0[i < count ? i : count];
  a.count = count;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(go2nn_grad_sq_kernel, dim3(nb), dim3(256), 0, st, a, partials);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_grad_sq_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, nb, out, cursor, slots);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_DIAG_H
