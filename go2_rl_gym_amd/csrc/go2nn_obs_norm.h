// go2nn_obs_norm.h — empirical (running mean / std) normalisation of the observations of feed-forward PPO (include/go2nn.h: go2nn_obs_norm_*, added within ABI 7;
// go2_rl_gym_amd/rsl_rl/modules/normalizer.py, rsl_rl/algorithms/ppo.py, `runner.empirical_normalization`).  Included at the end of go2nn_impl.cpp (FAIL, HIPCHK are its helpers).
//
// go2nn_obs_norm_apply: ONE launch per policy step for both observation streams (up to 4 jobs), inside the replayed rollout like go2nn_sensor_rand_apply.  The job index sits
// in the grid the way go2nn_mirror_rows has it: every job owns a range of blocks (first_block, a prefix sum), a block finds its job by walking that list.  Inside a job a
// block owns a tile of OBS_NORM_ROWS rows x OBS_NORM_COLS columns: wave w of its four takes rows w, w + 4, ... of the tile, lane l column l of the tile — every load and
// store of a wave is dense in the lane index along a row — and writes y = (x - mean) * inv [clamped] where it read x, which is why y may BE x.  One fp32 subtraction and one
// fp32 product: nothing contracts to an FMA, so the device, the host build and numpy agree on y bit for bit (this library is built without fast-math).
// With a partial table the lane also adds d = (double) x - (double) mean and d * d over its rows in increasing row order; the four waves' sums meet in LDS and wave 0
// adds them in the order 0, 1, 2, 3 and writes the tile's row of the table.  No atomics: two launches give the same bits.  (The device may contract d * d into the sum
// as one fp64 FMA, the host build may not: the two builds agree on y bit for bit and on the moments within the rounding of fp64.)
// go2nn_obs_norm_update: one block, one lane per column (columns past OBS_NORM_UPDATE_THREADS: a lane takes several): the table's rows — steps x rows of them, 1536 at 4096
// envs x 24 steps — are added in increasing order, merged into the fp64 state by Chan's pooled update, and the two fp32 values the apply launch reads are rewritten.  One
// block, because every lane reads `count` before lane 0 replaces it (a barrier orders the two) — and so the launch is bound by what ONE compute unit loads: measured on an
// MI355X 135 us for both streams at 4096 envs (7.5 MB of tables: 55 GB/s), once per iteration; 16 lanes per column with an LDS sum in the same block read 181 us, so that
// is not built.  A grid over the column tiles would need `count` replaced by a second launch.
// The host build runs the same lane functions in plain loops.
#ifndef GO2NN_OBS_NORM_H
#define GO2NN_OBS_NORM_H

#define OBS_NORM_COLS 64                 // the column tile: one wave along a row
#define OBS_NORM_WAVES 4
#define OBS_NORM_THREADS (OBS_NORM_COLS * OBS_NORM_WAVES)
#define OBS_NORM_ROWS GO2NN_OBS_NORM_ROWS          // rows per block = rows per row of the partial table
#define OBS_NORM_UPDATE_THREADS 1024
#define OBS_NORM_MAX_D 4096

struct ObsNormArgs {
  Go2nnObsNormJob job[GO2NN_OBS_NORM_MAX_JOBS];
  uint32_t col_tiles[GO2NN_OBS_NORM_MAX_JOBS];
  uint32_t first_block[GO2NN_OBS_NORM_MAX_JOBS + 1];      // job i owns blocks [first_block[i], first_block[i + 1]): row blocks x col_tiles[i]
  int32_t n_jobs, N;
};

#ifndef GO2_EMU
#define OBS_NORM_FN __device__ __forceinline__
#else
#define OBS_NORM_FN static inline
#endif

// which job, row block and column tile block `block` owns
OBS_NORM_FN int obs_norm_locate(const ObsNormArgs& a, uint32_t block, uint32_t* rb, uint32_t* ct) {
  int jb = 0;
  while (jb + 1 < a.n_jobs && block >= a.first_block[jb + 1]) ++jb;
  const uint32_t b = block - a.first_block[jb];
  *rb = b / a.col_tiles[jb];
  *ct = b - *rb * a.col_tiles[jb];
  return jb;
}

// wave w, lane l of the block that owns (rb, ct) of job j: its rows of the tile, in increasing order.  -> the lane's sums
OBS_NORM_FN void obs_norm_lane(const Go2nnObsNormJob& j, int32_t N, uint32_t rb, uint32_t ct, uint32_t w, uint32_t l, double* s1, double* s2) {
  const uint32_t col = ct * OBS_NORM_COLS + l;
  double a1 = 0.0, a2 = 0.0;
  if (col < (uint32_t)j.D) {
    const float m = j.mean[col], iv = j.inv[col], clip = j.clip;
    const double md = (double)m;
    const uint32_t r0 = rb * OBS_NORM_ROWS, r1 = r0 + OBS_NORM_ROWS < (uint32_t)N ? r0 + OBS_NORM_ROWS : (uint32_t)N;
    for (uint32_t r = r0 + w; r < r1; r += OBS_NORM_WAVES) {
      const size_t e = (size_t)r * (uint32_t)j.D + col;
      const float x = j.x[e];
      float y = (x - m) * iv;
      if (clip > 0.f) y = y < -clip ? -clip : (y > clip ? clip : y);
      j.y[e] = y;
      const double d = (double)x - md;
      a1 += d;
      a2 += d * d;
    }
  }
  *s1 = a1;
  *s2 = a2;
}

// the tile's row of the table from the four waves' sums of column tile lane l (sums[w][l][0 / 1])
OBS_NORM_FN void obs_norm_finish(const Go2nnObsNormJob& j, uint32_t rb, uint32_t ct, uint32_t l, const double (*sums)[OBS_NORM_COLS][2]) {
  const uint32_t col = ct * OBS_NORM_COLS + l;
  if (col >= (uint32_t)j.D) return;
  double a1 = sums[0][l][0], a2 = sums[0][l][1];
  for (int w = 1; w < OBS_NORM_WAVES; ++w) {
    a1 += sums[w][l][0];
    a2 += sums[w][l][1];
  }
  double* p = j.partials + ((size_t)rb * (uint32_t)j.D + col) * 2;
  p[0] = a1;
  p[1] = a2;
}

// column c of the update: the table's rows added in increasing order; -> the merged (mean, M2) and the two fp32 values, from the OLD count
OBS_NORM_FN void obs_norm_merge(const double* table, int32_t entries, int32_t D, int32_t c, double count, double* mean, double* M2, double n, double eps, float* mean32,
                                float* inv32) {
  double S1 = 0.0, S2 = 0.0;
  const double* p = table + (size_t)c * 2;
#pragma unroll 8
  for (int32_t t = 0; t < entries; ++t) {
    S1 += p[(size_t)t * D * 2];
    S2 += p[(size_t)t * D * 2 + 1];
  }
  const double mb = (double)mean32[c] + S1 / n;          // the batch's mean: the sums are centred on the frozen fp32 mean
  double M2b = S2 - S1 * (S1 / n);
  if (M2b < 0.0) M2b = 0.0;
  const double ma = mean[c], M2a = count > 0.0 ? M2[c] : 0.0;          // (count 0: the initial var = 1 is forgotten)
  const double tot = count + n, delta = mb - ma;
  const double mnew = ma + delta * (n / tot), M2new = M2a + M2b + delta * delta * (count * (n / tot));
  mean[c] = mnew;
  M2[c] = M2new;
  mean32[c] = (float)mnew;
  inv32[c] = (float)(1.0 / (sqrt(M2new / tot) + eps));
}

#ifndef GO2_EMU
__global__ void __launch_bounds__(OBS_NORM_THREADS) go2nn_obs_norm_apply_kernel(const ObsNormArgs a) {
  __shared__ double sums[OBS_NORM_WAVES][OBS_NORM_COLS][2];
  uint32_t rb, ct;
  const Go2nnObsNormJob& j = a.job[obs_norm_locate(a, blockIdx.x, &rb, &ct)];
  const uint32_t w = threadIdx.x / OBS_NORM_COLS, l = threadIdx.x % OBS_NORM_COLS;
  double s1, s2;
  obs_norm_lane(j, a.N, rb, ct, w, l, &s1, &s2);
  if (j.partials == nullptr) return;          // (uniform over the block)
  sums[w][l][0] = s1;
  sums[w][l][1] = s2;
  __syncthreads();
  if (w == 0) obs_norm_finish(j, rb, ct, l, sums);
}

__global__ void __launch_bounds__(OBS_NORM_UPDATE_THREADS) go2nn_obs_norm_update_kernel(const double* table, int32_t entries, int32_t D, double* state, double n, double eps,
                                                                                        float* mean32, float* inv32) {
  const double count = state[0];
  for (int32_t c = (int32_t)threadIdx.x; c < D; c += OBS_NORM_UPDATE_THREADS) obs_norm_merge(table, entries, D, c, count, state + 1, state + 1 + D, n, eps, mean32, inv32);
  __syncthreads();          // every lane has read the old count
  if (threadIdx.x == 0) state[0] = count + n;
}
#endif

extern "C" {

int32_t go2nn_obs_norm_partial_rows(int32_t N) { return N < 1 ? 0 : (int32_t)(((int64_t)N + OBS_NORM_ROWS - 1) / OBS_NORM_ROWS); }

int go2nn_obs_norm_apply(const Go2nnObsNormJob* jobs, int32_t n_jobs, int32_t N, void* stream) {
  if (!jobs || n_jobs < 1 || n_jobs > GO2NN_OBS_NORM_MAX_JOBS) FAIL(GO2NN_EINVAL, "obs norm apply: jobs null or n_jobs outside [1, %d]", GO2NN_OBS_NORM_MAX_JOBS);
  if (N < 1) FAIL(GO2NN_EINVAL, "obs norm apply: N = %d below 1", N);
  ObsNormArgs a = {};
  a.n_jobs = n_jobs;
  a.N = N;
  const long long row_blocks = go2nn_obs_norm_partial_rows(N);
  long long blocks = 0;
  for (int32_t i = 0; i < n_jobs; ++i) {
    const Go2nnObsNormJob& j = jobs[i];
    if (!j.x || !j.y || !j.mean || !j.inv) FAIL(GO2NN_EINVAL, "obs norm apply: job %d: a null x, y, mean or inv", i);
    if (j.D < 1 || j.D > OBS_NORM_MAX_D) FAIL(GO2NN_EINVAL, "obs norm apply: job %d: D = %d outside [1, %d]", i, j.D, OBS_NORM_MAX_D);
    if (!(j.clip - j.clip == 0.f)) FAIL(GO2NN_EINVAL, "obs norm apply: job %d: clip is not finite", i);
    a.job[i] = j;
    a.col_tiles[i] = (uint32_t)((j.D + OBS_NORM_COLS - 1) / OBS_NORM_COLS);
    a.first_block[i] = (uint32_t)blocks;
    blocks += row_blocks * a.col_tiles[i];
    if (blocks >= (1LL << 31)) FAIL(GO2NN_EINVAL, "obs norm apply: %d rows need too many blocks", N);
  }
  a.first_block[n_jobs] = (uint32_t)blocks;
#ifdef GO2_EMU
  (void)stream;
  static thread_local double sums[OBS_NORM_WAVES][OBS_NORM_COLS][2];
  for (uint32_t b = 0; b < (uint32_t)blocks; ++b) {
    uint32_t rb, ct;
    const Go2nnObsNormJob& j = a.job[obs_norm_locate(a, b, &rb, &ct)];
    for (uint32_t w = 0; w < OBS_NORM_WAVES; ++w)
      for (uint32_t l = 0; l < OBS_NORM_COLS; ++l) obs_norm_lane(j, a.N, rb, ct, w, l, &sums[w][l][0], &sums[w][l][1]);
    if (j.partials == nullptr) continue;
    for (uint32_t l = 0; l < OBS_NORM_COLS; ++l) obs_norm_finish(j, rb, ct, l, sums);
  }
#else
  hipLaunchKernelGGL(go2nn_obs_norm_apply_kernel, dim3((unsigned)blocks), dim3(OBS_NORM_THREADS), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_obs_norm_update(const double* table, int32_t steps, int32_t rows, int32_t D, double* state, double n, double eps, float* mean32, float* inv32, void* stream) {
  if (!table || !state || !mean32 || !inv32) FAIL(GO2NN_EINVAL, "obs norm update: a null pointer");
  if (steps < 1 || rows < 1 || D < 1 || D > OBS_NORM_MAX_D) FAIL(GO2NN_EINVAL, "obs norm update: steps %d or rows %d below 1, or D = %d outside [1, %d]", steps, rows, D, OBS_NORM_MAX_D);
  if (!(n > 0.0) || !(n - n == 0.0)) FAIL(GO2NN_EINVAL, "obs norm update: n = %g new samples (finite, above 0)", n);
  if (!(eps > 0.0) || !(eps - eps == 0.0)) FAIL(GO2NN_EINVAL, "obs norm update: eps = %g (finite, above 0)", eps);
  if ((long long)steps * rows >= (1LL << 31)) FAIL(GO2NN_EINVAL, "obs norm update: %d steps x %d rows do not fit 31 bits", steps, rows);
  const int32_t entries = steps * rows;
#ifdef GO2_EMU
  (void)stream;
  const double count = state[0];
  for (int32_t c = 0; c < D; ++c) obs_norm_merge(table, entries, D, c, count, state + 1, state + 1 + D, n, eps, mean32, inv32);
  state[0] = count + n;
#else
  hipLaunchKernelGGL(go2nn_obs_norm_update_kernel, dim3(1), dim3(OBS_NORM_UPDATE_THREADS), 0, (hipStream_t)stream, table, entries, D, state, n, eps, mean32, inv32);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_OBS_NORM_H
