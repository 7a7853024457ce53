// go2nn_mirror.h — the PPO update's left-right symmetry augmentation (include/go2nn.h: go2nn_mirror_*, added within ABI 7; rsl_rl/algorithms/ppo.py, `algorithm.symmetry`;
// the tables: go2_rl_gym_amd/utils/symmetry.py).  Included at the end of go2nn_impl.cpp (FAIL, HIPCHK are its helpers).
//
// One launch per update, after the rollout's permutation, for all (up to 16) tensors of the mini-batch.  The job index sits in the grid the way go2nn_sum_rows has it: every
// job owns a range of blocks (first_block, a prefix sum), a block finds its job by walking that list.  Inside a job a block owns one TILE of MIRROR_TILE consecutive source
// floats of one chunk — a chunk's source rows and both of its destination halves are contiguous, so a tile is three dense streams —, one lane per source element, 16
// elements per lane at a stride of the block: a lane reads src[e] and writes the copy, reads src[e - col + perm[col]] — inside the row its neighbours have just read, so the
// gather is served by lines already in L1 / L2 — multiplies by sign[col] (+-1.0f: exact, -0.0 and denormals included; this library is built without fast-math) and writes
// the mirror.  Every load and store instruction of a wave is dense in the lane index.  No LDS, no atomics.
// Integer divisions: what is uniform over a block (chunk and tile of the block, the column of the tile's first element) is divided once per block; the per-element column is
// (col0 + offset) mod width through a multiply-high by magic = floor(2^32 / width) + 1, exact while n * width < 2^32 (n < width + MIRROR_TILE, width < 2^15).
// Measured on one MI355X at the update's shapes of 4096 envs (98304 rows x 348 floats: 137 MB read once, written twice; tools/symmetry_bench.py, device events around 50
// back-to-back launches): 135 .. 140 us, 2.9 .. 3.0 TB/s, against 75 us for a device-to-device copy moving the same 410 MB (profiles/symmetry_bench.json).  The first version — one lane per element over a (widest job)
// x (jobs) grid with two 32-bit divisions per lane — took 299 us: most of its 909 k blocks belonged to the narrow jobs and had nothing to do; tiles with one load -> store
// chain per element took 154 us; a lane's loads issued before its stores, the figure above.  The host build runs the same block function in plain loops.
#ifndef GO2NN_MIRROR_H
#define GO2NN_MIRROR_H

#define MIRROR_THREADS 256
#define MIRROR_PER_LANE 16
#define MIRROR_TILE (MIRROR_THREADS * MIRROR_PER_LANE)

struct MirrorArgs {
  Go2nnMirrorJob job[GO2NN_MIRROR_MAX_JOBS];
  uint32_t magic[GO2NN_MIRROR_MAX_JOBS];                // floor(2^32 / width) + 1 (unused for width 1)
  uint32_t tiles[GO2NN_MIRROR_MAX_JOBS];                // tiles per chunk
  uint32_t first_block[GO2NN_MIRROR_MAX_JOBS + 1];      // job i owns blocks [first_block[i], first_block[i + 1]): chunks x tiles[i]
  uint32_t chunk_rows;
  int32_t n_jobs;
};

#ifndef GO2_EMU
#define MIRROR_FN __device__ __forceinline__
#define MIRROR_MULHI(a, b) __umulhi((a), (b))
#else
#define MIRROR_FN static inline
#define MIRROR_MULHI(a, b) ((uint32_t)(((uint64_t)(a) * (uint64_t)(b)) >> 32))
#endif

// lane `tid` of block `block`
MIRROR_FN void mirror_block(const MirrorArgs& a, uint32_t block, uint32_t tid) {
  int jb = 0;
  while (jb + 1 < a.n_jobs && block >= a.first_block[jb + 1]) ++jb;
  const Go2nnMirrorJob& j = a.job[jb];
  const uint32_t w = (uint32_t)j.width, n_c = a.chunk_rows * w, magic = a.magic[jb];          // n_c: source floats of one chunk
  const uint32_t b = block - a.first_block[jb], c = b / a.tiles[jb], e0 = (b - c * a.tiles[jb]) * MIRROR_TILE, col0 = e0 % w;
  const float* s = j.src + (size_t)c * n_c;
  float* d = j.dst + (size_t)c * 2u * n_c;          // dst [chunks, 2, chunk_rows, width]: the chunk's copy half, then its mirror half
  // all of the lane's loads first, then its stores: 2 x MIRROR_PER_LANE loads in flight per lane instead of one load -> store chain per element
  float x[MIRROR_PER_LANE], m[MIRROR_PER_LANE];
#pragma unroll
  for (uint32_t i = 0; i < MIRROR_PER_LANE; ++i) {
    const uint32_t off = i * MIRROR_THREADS + tid, e = e0 + off;
    if (e >= n_c) continue;
    x[i] = m[i] = s[e];
    if (j.perm) {
      const uint32_t n = col0 + off, col = w == 1 ? 0u : n - MIRROR_MULHI(n, magic) * w;
      m[i] = j.sign[col] * s[e - col + (uint32_t)j.perm[col]];
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < MIRROR_PER_LANE; ++i) {
    const uint32_t e = e0 + i * MIRROR_THREADS + tid;
    if (e >= n_c) continue;
    d[e] = x[i];
    d[n_c + e] = m[i];
  }
}

#ifndef GO2_EMU
__global__ void __launch_bounds__(MIRROR_THREADS) go2nn_mirror_rows_kernel(const MirrorArgs a) { mirror_block(a, blockIdx.x, threadIdx.x); }
#endif

extern "C" {

int go2nn_mirror_check_table(const int16_t* host_perm, const float* host_sign, int32_t width) {
  if (!host_perm || !host_sign) FAIL(GO2NN_EINVAL, "mirror table: a null pointer");
  if (width < 1 || width > 32767) FAIL(GO2NN_EINVAL, "mirror table: width %d outside [1, 32767]", width);
  for (int32_t c = 0; c < width; ++c) {
    if (host_perm[c] < 0 || host_perm[c] >= width) FAIL(GO2NN_EINVAL, "mirror table: perm[%d] = %d outside [0, %d)", c, (int)host_perm[c], width);
    if (host_sign[c] != 1.0f && host_sign[c] != -1.0f) FAIL(GO2NN_EINVAL, "mirror table: sign[%d] = %g is neither +1 nor -1", c, (double)host_sign[c]);
  }
  return 0;
}

int go2nn_mirror_rows(const Go2nnMirrorJob* jobs, int32_t n_jobs, int32_t chunks, int32_t chunk_rows, void* stream) {
  if (!jobs || n_jobs < 1 || n_jobs > GO2NN_MIRROR_MAX_JOBS) FAIL(GO2NN_EINVAL, "mirror rows: jobs null or n_jobs outside [1, %d]", GO2NN_MIRROR_MAX_JOBS);
  if (chunks < 1 || chunk_rows < 1) FAIL(GO2NN_EINVAL, "mirror rows: chunks %d or chunk_rows %d below 1", chunks, chunk_rows);
  const long long rows = (long long)chunks * chunk_rows;
  MirrorArgs a = {};
  a.chunk_rows = (uint32_t)chunk_rows;
  a.n_jobs = n_jobs;
  long long blocks = 0;
  for (int32_t i = 0; i < n_jobs; ++i) {
    const Go2nnMirrorJob& j = jobs[i];
    if (!j.src || !j.dst) FAIL(GO2NN_EINVAL, "mirror rows: job %d: a null src or dst", i);
    if (j.width < 1 || j.width > 32767) FAIL(GO2NN_EINVAL, "mirror rows: job %d: width %d outside [1, 32767]", i, j.width);
    if ((j.perm == nullptr) != (j.sign == nullptr)) FAIL(GO2NN_EINVAL, "mirror rows: job %d: perm and sign are given together or not at all", i);
    if (2 * rows * j.width >= (1LL << 31)) FAIL(GO2NN_EINVAL, "mirror rows: job %d: %lld x 2 x %d elements do not fit 31 bits", i, rows, j.width);
#ifdef GO2_EMU
    if (j.perm)          // the host build can read the table (on the device it was checked before the upload: go2nn_mirror_check_table)
      for (int32_t c = 0; c < j.width; ++c)
        if (j.perm[c] < 0 || j.perm[c] >= j.width) FAIL(GO2NN_EINVAL, "mirror rows: job %d: perm[%d] = %d outside [0, %d)", i, c, (int)j.perm[c], j.width);
#endif
    a.job[i] = j;
    a.magic[i] = (uint32_t)((1ULL << 32) / (uint32_t)j.width + 1ULL);          // (width 1: wraps to 1, not used)
    a.tiles[i] = (uint32_t)(((long long)chunk_rows * j.width + MIRROR_TILE - 1) / MIRROR_TILE);
    a.first_block[i] = (uint32_t)blocks;
    blocks += (long long)chunks * a.tiles[i];
    if (blocks * MIRROR_THREADS >= (1LL << 32))          // (the grid's lanes are counted in 32 bits)
      FAIL(GO2NN_EINVAL, "mirror rows: %d chunks of %d rows need too many blocks (chunks this small are not what the kernel is for)", chunks, chunk_rows);
  }
  a.first_block[n_jobs] = (uint32_t)blocks;
#ifdef GO2_EMU
  (void)stream;
  for (uint32_t b = 0; b < (uint32_t)blocks; ++b)
    for (uint32_t t = 0; t < MIRROR_THREADS; ++t) mirror_block(a, b, t);
#else
  hipLaunchKernelGGL(go2nn_mirror_rows_kernel, dim3((unsigned)blocks), dim3(MIRROR_THREADS), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_MIRROR_H
