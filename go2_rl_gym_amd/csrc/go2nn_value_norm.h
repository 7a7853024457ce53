// go2nn_value_norm.h — value normalisation: the critic predicts returns normalised by their running mean / std (include/go2nn.h: go2nn_value_norm_*, go2nn_value_head_fold,
// added within ABI 7; go2_rl_gym_amd/rsl_rl/modules/normalizer.py:ValueNormalization, rsl_rl/algorithms/_base.py, `algorithm.normalize_value`).  Included at the end of
// go2nn_impl.cpp (FAIL, HIPCHK are its helpers).
//
// go2nn_value_norm_apply: ONE launch per iteration, behind GAE, over the T x N floats of `values` and of `returns`, in place: x <- (x - mean32) * inv32 — one fp32
// subtraction and one fp32 product, nothing contracts to an FMA, no clamp: the device, the host build, torch and numpy agree bit for bit (this library is built without
// fast-math).  A 256-lane block owns VALUE_NORM_ROWS = 1024 consecutive elements, four per lane.  Where BOTH pointers are 16-byte aligned lane l owns elements 4 l .. 4 l + 3
// of the block's range — one 16-byte load and one 16-byte store per tensor, dense in the lane index (a lane whose four elements straddle n takes them one by one) —, else
// elements l, l + 256, l + 512, l + 768: four 4-byte accesses per tensor, each dense in the lane index.  All of a lane's loads issue before its first store.  With a
// partial table the lane adds d = (double) R - (double) mean32 and d * d of its RAW returns in increasing element order; the 256 pairs meet in LDS and are added in a fixed
// order (lane t < 64 adds t, t + 64, t + 128, t + 192; then the halving tree 32, 16, ..., 1): no atomics, no scratch, two launches give the same bits.  (The device may
// contract d * d into the sum as one fp64 FMA, the host build may not, and the two layouts add in different orders: all agree on values / returns bit for bit and on the
// moments within the rounding of fp64.)
// go2nn_value_norm_update: one block.  Lane 0 reads the OLD stat32, adds the table's rows in increasing order, applies Chan's pooled update to the fp64 state
// (go2nn_obs_norm_update's rule for one column) and rewrites stat32 = mean32 | std32 | inv32; with w_last given (output preservation, PopArt's step) the block then rewrites
// the critic's last layer so that v * std32 + mean32 of every input stays what it was: W <- W sigma / sigma', b <- (sigma b + mu - mu') / sigma', in fp64 from the fp32
// scalars, rounded once.
// go2nn_value_head_fold: K + 1 floats, (W std32, b std32 + mean32) into a scratch pair the critic's packed operand buffer is made from (in front of go2nn_pack, once per
// rollout, inside the replayed rollout graph: no host scalar).
// Code object notes (build.py kernel_resources, gfx950): apply 24 VGPR / 26 SGPR, 0 scratch, 4096 B LDS; update 22 VGPR / 68 SGPR, 0 scratch, 32 B LDS; fold 4 VGPR /
// 21 SGPR, 0 scratch, 0 LDS; 8 waves per SIMD each.  At T x N = 98 304 all three are launch latency, not bandwidth (README: value normalisation).
// The host build runs the same lane functions in plain loops.
#ifndef GO2NN_VALUE_NORM_H
#define GO2NN_VALUE_NORM_H

#define VALUE_NORM_THREADS 256
#define VALUE_NORM_PER_LANE 4
#define VALUE_NORM_ROWS GO2NN_VALUE_NORM_ROWS          // elements per block = elements per row of the partial table
static_assert(VALUE_NORM_ROWS == VALUE_NORM_THREADS * VALUE_NORM_PER_LANE, "a block owns four elements per lane");

#ifndef GO2_EMU
#define VALUE_NORM_FN __device__ __forceinline__
#else
#define VALUE_NORM_FN static inline
#endif

struct alignas(16) ValueNormVec4 {
  float v[4];
};

VALUE_NORM_FN bool value_norm_vector_ok(const float* values, const float* returns) { return (((uintptr_t)values | (uintptr_t)returns) & 15u) == 0; }

// lane l of the block that owns elements [base, base + VALUE_NORM_ROWS) of the n: loads, then stores; -> the lane's sums of d and d * d of the raw returns
VALUE_NORM_FN void value_norm_lane(float* values, float* returns, uint32_t n, uint32_t base, uint32_t l, bool vec, float m, float iv, double* s1, double* s2) {
  float v[VALUE_NORM_PER_LANE], r[VALUE_NORM_PER_LANE];
  uint32_t e[VALUE_NORM_PER_LANE];
  const uint32_t e0 = base + VALUE_NORM_PER_LANE * l;
  const bool whole = vec && e0 + VALUE_NORM_PER_LANE <= n;          // (base + 1024 <= 2^31 + 1023: no wrap in 32 bits)
  if (whole) {
    const ValueNormVec4 a = *reinterpret_cast<const ValueNormVec4*>(values + e0), b = *reinterpret_cast<const ValueNormVec4*>(returns + e0);
#pragma unroll
    for (int k = 0; k < VALUE_NORM_PER_LANE; ++k) {
      e[k] = e0 + k;
      v[k] = a.v[k];
      r[k] = b.v[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < VALUE_NORM_PER_LANE; ++k) {
      e[k] = vec ? e0 + k : base + (uint32_t)k * VALUE_NORM_THREADS + l;
      v[k] = e[k] < n ? values[e[k]] : 0.f;
      r[k] = e[k] < n ? returns[e[k]] : 0.f;
    }
  }
  const double md = (double)m;
  double a1 = 0.0, a2 = 0.0;
  ValueNormVec4 ov, orr;
#pragma unroll
  for (int k = 0; k < VALUE_NORM_PER_LANE; ++k) {
    ov.v[k] = (v[k] - m) * iv;
    orr.v[k] = (r[k] - m) * iv;
    if (e[k] < n) {
      const double d = (double)r[k] - md;
      a1 += d;
      a2 += d * d;
    }
  }
  if (whole) {
    *reinterpret_cast<ValueNormVec4*>(values + e0) = ov;
    *reinterpret_cast<ValueNormVec4*>(returns + e0) = orr;
  } else {
#pragma unroll
    for (int k = 0; k < VALUE_NORM_PER_LANE; ++k)
      if (e[k] < n) {
        values[e[k]] = ov.v[k];
        returns[e[k]] = orr.v[k];
      }
  }
  *s1 = a1;
  *s2 = a2;
}

// the fixed order in which a block's 256 pairs are added: stage 0 (t < 64), then stride = 32, 16, ..., 1 (t < stride)
VALUE_NORM_FN void value_norm_fold4(double (*s)[2], uint32_t t) {
  s[t][0] = ((s[t][0] + s[t + 64][0]) + s[t + 128][0]) + s[t + 192][0];
  s[t][1] = ((s[t][1] + s[t + 64][1]) + s[t + 128][1]) + s[t + 192][1];
}

VALUE_NORM_FN void value_norm_halve(double (*s)[2], uint32_t t, uint32_t stride) {
  s[t][0] += s[t + stride][0];
  s[t][1] += s[t + stride][1];
}

// lane 0 of the update: -> sc = mu | sigma | mu' | sigma' (the fp32 scalars before and after, as doubles); state and stat32 rewritten
VALUE_NORM_FN void value_norm_merge(const double* partials, int32_t rows, double* state, double n, double eps, float* stat32, double* sc) {
  const double mu_old = (double)stat32[0], sd_old = (double)stat32[1];
  double S1 = 0.0, S2 = 0.0;
#pragma unroll 8
  for (int32_t t = 0; t < rows; ++t) {
    S1 += partials[(size_t)t * 2];
    S2 += partials[(size_t)t * 2 + 1];
  }
  const double count = state[0];
  const double mb = mu_old + S1 / n;          // the batch's mean: the sums are centred on the frozen fp32 mean
  double M2b = S2 - S1 * (S1 / n);
  if (M2b < 0.0) M2b = 0.0;
  const double ma = state[1], M2a = count > 0.0 ? state[2] : 0.0;          // (count 0: the initial var = 1 is forgotten)
  const double tot = count + n, delta = mb - ma;
  const double mnew = ma + delta * (n / tot), M2new = M2a + M2b + delta * delta * (count * (n / tot));
  state[0] = tot;
  state[1] = mnew;
  state[2] = M2new;
  const double sd = sqrt(M2new / tot) + eps;
  const float m32 = (float)mnew, s32 = (float)sd;
  stat32[0] = m32;
  stat32[1] = s32;
  stat32[2] = (float)(1.0 / sd);
  sc[0] = mu_old;
  sc[1] = sd_old;
  sc[2] = (double)m32;
  sc[3] = (double)s32;
}

VALUE_NORM_FN float value_norm_keep_w(float w, const double* sc) { return (float)((double)w * (sc[1] / sc[3])); }
VALUE_NORM_FN float value_norm_keep_b(float b, const double* sc) { return (float)((sc[1] * (double)b + sc[0] - sc[2]) / sc[3]); }

#ifndef GO2_EMU
__global__ void __launch_bounds__(VALUE_NORM_THREADS) go2nn_value_norm_apply_kernel(float* values, float* returns, uint32_t n, const float* stat32, double* partials) {
  __shared__ double s[VALUE_NORM_THREADS][2];
  const uint32_t t = threadIdx.x;
  const float m = stat32[0], iv = stat32[2];
  double s1, s2;
  value_norm_lane(values, returns, n, blockIdx.x * (uint32_t)VALUE_NORM_ROWS, t, value_norm_vector_ok(values, returns), m, iv, &s1, &s2);
  if (partials == nullptr) return;          // (uniform over the grid)
  s[t][0] = s1;
  s[t][1] = s2;
  __syncthreads();
  if (t < 64) value_norm_fold4(s, t);
  for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
    __syncthreads();
    if (t < stride) value_norm_halve(s, t, stride);
  }
  if (t == 0) {
    partials[(size_t)blockIdx.x * 2] = s[0][0];
    partials[(size_t)blockIdx.x * 2 + 1] = s[0][1];
  }
}

__global__ void __launch_bounds__(VALUE_NORM_THREADS) go2nn_value_norm_update_kernel(const double* partials, int32_t rows, double* state, double n, double eps, float* stat32,
                                                                                    float* w_last, float* b_last, int32_t K) {
  __shared__ double sc[4];
  if (threadIdx.x == 0) value_norm_merge(partials, rows, state, n, eps, stat32, sc);
  if (w_last == nullptr) return;          // (uniform)
  __syncthreads();
  for (int32_t k = (int32_t)threadIdx.x; k < K; k += VALUE_NORM_THREADS) w_last[k] = value_norm_keep_w(w_last[k], sc);
  if (threadIdx.x == 0) b_last[0] = value_norm_keep_b(b_last[0], sc);
}

__global__ void __launch_bounds__(VALUE_NORM_THREADS) go2nn_value_head_fold_kernel(const float* w, const float* b, int32_t K, const float* stat32, float* w_out, float* b_out) {
  const int32_t k = (int32_t)(blockIdx.x * VALUE_NORM_THREADS + threadIdx.x);
  const float m = stat32[0], sd = stat32[1];
  if (k < K) w_out[k] = w[k] * sd;
  else if (k == K) b_out[0] = b[0] * sd + m;
}
#endif

extern "C" {

int32_t go2nn_value_norm_partial_rows(int32_t n) { return n < 1 ? 0 : (int32_t)(((int64_t)n + VALUE_NORM_ROWS - 1) / VALUE_NORM_ROWS); }

int go2nn_value_norm_apply(float* values, float* returns, int32_t n, const float* stat32, double* partials, void* stream) {
  if (!values || !returns || !stat32) FAIL(GO2NN_EINVAL, "value norm apply: a null values, returns or stat32");
  if (n < 1) FAIL(GO2NN_EINVAL, "value norm apply: n = %d below 1", n);
  if (((uintptr_t)values | (uintptr_t)returns | (uintptr_t)stat32) & 3u) FAIL(GO2NN_EINVAL, "value norm apply: a pointer that is not aligned to a float");
  const uint32_t blocks = (uint32_t)go2nn_value_norm_partial_rows(n);
#ifdef GO2_EMU
  (void)stream;
  static thread_local double s[VALUE_NORM_THREADS][2];
  const float m = stat32[0], iv = stat32[2];
  const bool vec = value_norm_vector_ok(values, returns);
  for (uint32_t b = 0; b < blocks; ++b) {
    for (uint32_t t = 0; t < VALUE_NORM_THREADS; ++t) value_norm_lane(values, returns, (uint32_t)n, b * (uint32_t)VALUE_NORM_ROWS, t, vec, m, iv, &s[t][0], &s[t][1]);
    if (partials == nullptr) continue;
    for (uint32_t t = 0; t < 64; ++t) value_norm_fold4(s, t);
    for (uint32_t stride = 32; stride >= 1; stride >>= 1)
      for (uint32_t t = 0; t < stride; ++t) value_norm_halve(s, t, stride);
    partials[(size_t)b * 2] = s[0][0];
    partials[(size_t)b * 2 + 1] = s[0][1];
  }
#else
  hipLaunchKernelGGL(go2nn_value_norm_apply_kernel, dim3(blocks), dim3(VALUE_NORM_THREADS), 0, (hipStream_t)stream, values, returns, (uint32_t)n, stat32, partials);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_value_norm_update(const double* partials, int32_t rows, double* state, double n, double eps, float* stat32, float* w_last, float* b_last, int32_t K, void* stream) {
  if (!partials || !state || !stat32) FAIL(GO2NN_EINVAL, "value norm update: a null partials, state or stat32");
  if (rows < 1) FAIL(GO2NN_EINVAL, "value norm update: rows = %d below 1", rows);
  if (!(n > 0.0) || !(n - n == 0.0)) FAIL(GO2NN_EINVAL, "value norm update: n = %g new samples (finite, above 0)", n);
  if (!(eps > 0.0) || !(eps - eps == 0.0)) FAIL(GO2NN_EINVAL, "value norm update: eps = %g (finite, above 0)", eps);
  if (w_last && (!b_last || K < 1)) FAIL(GO2NN_EINVAL, "value norm update: output preservation needs b_last and K >= 1 (K = %d)", K);
#ifdef GO2_EMU
  (void)stream;
  double sc[4];
  value_norm_merge(partials, rows, state, n, eps, stat32, sc);
  if (w_last) {
    for (int32_t k = 0; k < K; ++k) w_last[k] = value_norm_keep_w(w_last[k], sc);
    b_last[0] = value_norm_keep_b(b_last[0], sc);
  }
#else
  hipLaunchKernelGGL(go2nn_value_norm_update_kernel, dim3(1), dim3(VALUE_NORM_THREADS), 0, (hipStream_t)stream, partials, rows, state, n, eps, stat32, w_last, b_last, K);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_value_head_fold(const float* w, const float* b, int32_t K, const float* stat32, float* w_out, float* b_out, void* stream) {
  if (!w || !b || !stat32 || !w_out || !b_out) FAIL(GO2NN_EINVAL, "value head fold: a null pointer");
  if (K < 1) FAIL(GO2NN_EINVAL, "value head fold: K = %d below 1", K);
#ifdef GO2_EMU
  (void)stream;
  const float m = stat32[0], sd = stat32[1];
  for (int32_t k = 0; k < K; ++k) w_out[k] = w[k] * sd;
  {
    const float t = b[0] * sd;          // (two roundings, as torch states it; the device may contract the pair into one FMA: the fold is compared within the forward tolerance)
    b_out[0] = t + m;
  }
#else
  hipLaunchKernelGGL(go2nn_value_head_fold_kernel, dim3((unsigned)(((int64_t)K + 1 + VALUE_NORM_THREADS - 1) / VALUE_NORM_THREADS)), dim3(VALUE_NORM_THREADS), 0, (hipStream_t)stream,
                     w, b, K, stat32, w_out, b_out);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_VALUE_NORM_H
