// go2nn_spectrum.h — the evaluator's action and torque spectra (include/go2nn.h: go2nn_spectrum_*, added within ABI 7; go2_rl_gym_amd/utils/evaluator.py, `evaluation.spectrum`).
// Included at the end of go2nn_impl.cpp after go2nn_eval.h (FAIL, HIPCHK are the former's helpers; EVAL_FN, EVAL_MEMBER, eval_f, eval_b, eval_field_fault and the launch
// scaffold — eval_table_begin, eval_per_env, eval_reduce over eval_group_sum — go2nn_eval.h's).  The estimator (Welch, periodic Hann, half-overlapping windows at fixed
// positions, a window with a reset frame skipped) is stated once, in include/go2nn.h.
//
// THE TRACE AND WHO PAYS ITS STRIDE.  trace is fp32 [1 + 25 T, N], row-major by row, column e = robot e: the STEP row, then per counted step the 25 channel rows — TIME-MAJOR,
// ROBOT INNERMOST.  The per-step writer (eval_per_env_kernel<SpectrumRecord>, one lane per robot, inside the replayed graph: it runs `steps` times per evaluation and is
// launch-bound at 1024 lanes) therefore stores 25 dense lines per wave and reads the simulator's field-major buffers densely, as every other family's step does.  The Welch
// reader runs ONCE per evaluation and pays: a workgroup owns one robot, and its loads of a window (25 W floats) are N floats apart — every 4-byte load its own line.
// Neighbouring workgroups read the neighbouring columns of the same lines at about the same time, so the lines are served from L2; the kernel reads every frame twice
// (the windows overlap by half).  The other layout (robot-major) would make the once-only reader dense and the 500-times writer a 25-way scatter per lane.
//
// go2nn_spectrum_welch: grid = N, 256 lanes, dynamic LDS (2 W + 24 W + 24) doubles (13.5 KB at W = 64, 53.4 KB at W = 256).  Per window: the W flags (one lane each,
// __syncthreads_or: the skip is uniform); the 24 channels staged in LDS as fp64; 24 lanes add their channel in increasing n and keep its mean; every staged sample becomes
// (x - mean) hann[n]; then lane t owns the outputs o = t, t + 256, ... of the 6 (W / 2 + 1) (signal, kind, bin) triples and walks its kind's 4 channels x W samples in
// increasing (channel, n), the twiddle index k n mod W kept by addition — fp64 fma throughout, written as fma() so that hipcc and g++ round at the same places: the device
// and the host build agree bit for bit.  Each window's P and M is rounded once to fp32 and added to the lane's fp32 sums (registers: at most 4 outputs per lane at W = 256,
// constant indices, no scratch), stored once at the end.  No atomics, no cross-workgroup traffic, the order is a function of (T, W) only: two launches give the same bits.
// From the gfx950 code object's notes (build.py kernel_resources): 91 VGPRs, 74 SGPRs, 0 bytes of scratch, 256 B of static LDS next to the dynamic block; the record
// launch 13 VGPRs, 28 SGPRs, no scratch, no LDS.  On an MI355X (profiles/spectrum_bench.json; 1024 robots, 500 counted steps, W = 64): 0.82 ms per Welch launch, 4.4 us
// per record launch, 15 us for a device-to-device copy of the trace's 51 MB — the pass is bound by its LDS operand reads (a (cos, sin) pair per two multiply-adds at a
// lane-dependent address: an estimate from the instruction mix), not by memory.
// The scales 1 / (fs sum hann^2) = 1 / (fs 3 W / 8) and 1 / sum hann = 2 / W (the periodic Hann window's closed forms) and 1 / W are computed on the host in both builds.
#ifndef GO2NN_SPECTRUM_H
#define GO2NN_SPECTRUM_H

#define SPECTRUM_MAX_OUT ((6 * (GO2NN_SPECTRUM_MAX_WINDOW / 2 + 1) + EVAL_THREADS - 1) / EVAL_THREADS)          // outputs per lane at the largest window
#define SPECTRUM_SIGNALS 24                                                                                     // staged channels: all but the reset flag
static_assert(GO2NN_SPECTRUM_CH_RESET == SPECTRUM_SIGNALS && GO2NN_SPECTRUM_CHANNELS == SPECTRUM_SIGNALS + 1, "the flag follows the 24 signals");
static_assert(GO2NN_SPECTRUM_MAX_WINDOW <= EVAL_THREADS, "one lane per flag of a window");

EVAL_FN long long spectrum_trace_at(int N, int frame, int ch, int e) { return (1LL + (long long)frame * GO2NN_SPECTRUM_CHANNELS + ch) * N + e; }

// one counted step of robot e: its 24 floats in slot order (joint_of_slot: hips, thighs, calves) and its reset flag, behind the robot's own step counter
EVAL_FN void spectrum_record_env(const Go2nnSpectrumIn& in, float* trace, int N, int T, int e) {
  const float s = trace[e];
  trace[e] = s + 1.f;
  if (s < 0.f || s >= (float)T) return;
  float* row = trace + spectrum_trace_at(N, (int)s, 0, e);
#pragma unroll
  for (int slot = 0; slot < 12; ++slot) {
    const int j = in.joint_of_slot[slot];
    row[(long long)(GO2NN_SPECTRUM_CH_ACTION0 + slot) * N] = eval_f(in.actions, e, j);
    row[(long long)(GO2NN_SPECTRUM_CH_TORQUE0 + slot) * N] = eval_f(in.torques, e, j);
  }
  row[(long long)GO2NN_SPECTRUM_CH_RESET * N] = eval_b(in.reset_buf, e) != 0 ? 1.f : 0.f;
}

struct SpectrumRecord {
  Go2nnSpectrumIn in; float* trace; int N, T;
  EVAL_MEMBER void operator()(int e) const { spectrum_record_env(in, trace, N, T, e); }
};

// the mean of one staged channel, added in increasing n
EVAL_FN double spectrum_mean(const double* x, int W, double inv_w) {
  double s = 0.0;
  for (int n = 0; n < W; ++n) s += x[n];
  return s * inv_w;
}

// (x - mean) hann[n], hann[n] = 0.5 - 0.5 cos(2 pi n / W) from the twiddle table's cosine
EVAL_FN double spectrum_taper(double x, double mean, double cos_n) { return (x - mean) * fma(-0.5, cos_n, 0.5); }

// bin k of one (signal, kind): x4 = the kind's 4 tapered channels [4, W], tw = [W] (cos, sin) pairs -> the sums over the 4 channels of P_k and M_k
EVAL_FN void spectrum_bin(const double* x4, const double* tw, int W, int k, double scale_p, double scale_m, double* P, double* M) {
  const double ck = (k == 0 || 2 * k == W) ? 1.0 : 2.0;
  double sp = 0.0, sm = 0.0;
  for (int j = 0; j < 4; ++j) {
    const double* x = x4 + j * W;
    double re = 0.0, im = 0.0;
    int at = 0;          // k n mod W
    for (int n = 0; n < W; ++n) {
      re = fma(x[n], tw[2 * at], re);
      im = fma(-x[n], tw[2 * at + 1], im);
      at += k;
      if (at >= W) at -= W;
    }
    const double m2 = fma(re, re, im * im);
    sp = fma(ck * m2, scale_p, sp);
    sm = fma(ck * sqrt(m2), scale_m, sm);
  }
  *P = sp;
  *M = sm;
}

EVAL_FN int spectrum_windows(int T, int W) { return T >= W ? (T - W) / (W / 2) + 1 : 0; }

struct SpectrumWelch {
  const float* trace; const double* twiddle; float* table;
  int N, T, W;
  double inv_w, scale_p, scale_m;
};

#ifdef GO2_EMU
// robot e, the workgroup's program in plain loops: the same element functions in the same order
static void spectrum_welch_robot(const SpectrumWelch& a, int e, double* x, float* acc_p, float* acc_m) {
  const int N = a.N, W = a.W, O = 6 * (W / 2 + 1);
  int used = 0, skipped = 0;
  for (int o = 0; o < O; ++o) acc_p[o] = acc_m[o] = 0.f;
  for (int w = 0; w < spectrum_windows(a.T, W); ++w) {
    const int f0 = w * (W / 2);
    bool reset = false;
    for (int n = 0; n < W; ++n) reset = reset || a.trace[spectrum_trace_at(N, f0 + n, GO2NN_SPECTRUM_CH_RESET, e)] != 0.f;
    if (reset) { ++skipped; continue; }
    for (int c = 0; c < SPECTRUM_SIGNALS; ++c) {
      for (int n = 0; n < W; ++n) x[c * W + n] = (double)a.trace[spectrum_trace_at(N, f0 + n, c, e)];
      const double mean = spectrum_mean(x + c * W, W, a.inv_w);
      for (int n = 0; n < W; ++n) x[c * W + n] = spectrum_taper(x[c * W + n], mean, a.twiddle[2 * n]);
    }
    for (int o = 0; o < O; ++o) {
      double P, M;
      spectrum_bin(x + (o / (W / 2 + 1)) * 4 * W, a.twiddle, W, o % (W / 2 + 1), a.scale_p, a.scale_m, &P, &M);
      acc_p[o] += (float)P;
      acc_m[o] += (float)M;
    }
    ++used;
  }
  a.table[(long long)GO2NN_SPECTRUM_USED * N + e] = (float)used;
  a.table[(long long)GO2NN_SPECTRUM_SKIPPED * N + e] = (float)skipped;
  for (int o = 0; o < O; ++o) {
    a.table[(long long)(GO2NN_SPECTRUM_BIN0 + o) * N + e] = acc_p[o];
    a.table[(long long)(GO2NN_SPECTRUM_BIN0 + O + o) * N + e] = acc_m[o];
  }
}
#else
__global__ void __launch_bounds__(EVAL_THREADS) spectrum_welch_kernel(const SpectrumWelch a) {
  extern __shared__ double spectrum_lds[];
  const int N = a.N, W = a.W, K = W / 2 + 1, O = 6 * K, e = blockIdx.x, t = threadIdx.x;
  double* tw = spectrum_lds;                       // [W] (cos, sin)
  double* x = tw + 2 * W;                          // [24, W]
  double* mean = x + SPECTRUM_SIGNALS * W;         // [24]
  for (int i = t; i < 2 * W; i += EVAL_THREADS) tw[i] = a.twiddle[i];
  float acc_p[SPECTRUM_MAX_OUT], acc_m[SPECTRUM_MAX_OUT];
#pragma unroll
  for (int q = 0; q < SPECTRUM_MAX_OUT; ++q) acc_p[q] = acc_m[q] = 0.f;
  int used = 0, skipped = 0;
  const int windows = spectrum_windows(a.T, W);
  for (int w = 0; w < windows; ++w) {
    const int f0 = w * (W / 2);
    const int flag = t < W ? a.trace[spectrum_trace_at(N, f0 + t, GO2NN_SPECTRUM_CH_RESET, e)] != 0.f : 0;
    if (__syncthreads_or(flag)) {          // (a barrier too: the window before has been read, and tw is in place)
      ++skipped;
      continue;
    }
    for (int i = t; i < SPECTRUM_SIGNALS * W; i += EVAL_THREADS) x[i] = (double)a.trace[spectrum_trace_at(N, f0 + i % W, i / W, e)];
    __syncthreads();
    if (t < SPECTRUM_SIGNALS) mean[t] = spectrum_mean(x + t * W, W, a.inv_w);
    __syncthreads();
    for (int i = t; i < SPECTRUM_SIGNALS * W; i += EVAL_THREADS) x[i] = spectrum_taper(x[i], mean[i / W], tw[2 * (i % W)]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SPECTRUM_MAX_OUT; ++q) {
      const int o = t + q * EVAL_THREADS;
      if (o < O) {
        double P, M;
        spectrum_bin(x + (o / K) * 4 * W, tw, W, o % K, a.scale_p, a.scale_m, &P, &M);
        acc_p[q] += (float)P;
        acc_m[q] += (float)M;
      }
    }
    ++used;
  }
  if (t == 0) {
    a.table[(long long)GO2NN_SPECTRUM_USED * N + e] = (float)used;
    a.table[(long long)GO2NN_SPECTRUM_SKIPPED * N + e] = (float)skipped;
  }
#pragma unroll
  for (int q = 0; q < SPECTRUM_MAX_OUT; ++q) {
    const int o = t + q * EVAL_THREADS;
    if (o < O) {
      a.table[(long long)(GO2NN_SPECTRUM_BIN0 + o) * N + e] = acc_p[q];
      a.table[(long long)(GO2NN_SPECTRUM_BIN0 + O + o) * N + e] = acc_m[q];
    }
  }
}
#endif

// column c of go2nn_spectrum_reduce's output for robot e: 1 (the group's size), then the table's rows in order
struct SpectrumTerm {
  const float* table; int N, c;
  EVAL_MEMBER double operator()(int e) const { return c == GO2NN_SPECTRUM_OUT_N ? 1.0 : (double)table[(long long)(c - GO2NN_SPECTRUM_OUT_ROW0) * N + e]; }
};

static const char* spectrum_window_bad(int W) {
  return (W < GO2NN_SPECTRUM_MIN_WINDOW || W > GO2NN_SPECTRUM_MAX_WINDOW || (W & 1)) ? "W: an even window length in [8, 256]" : nullptr;
}

static const char* spectrum_in_bad(const Go2nnSpectrumIn* in) {
  const int a = eval_field_fault(in->actions, 1), q = eval_field_fault(in->torques, 1), reset = eval_field_fault(in->reset_buf, 0);
  if (a == EVAL_FIELD_NULL || q == EVAL_FIELD_NULL || reset == EVAL_FIELD_NULL) return "a null buffer pointer";
  if (a == EVAL_FIELD_ENV_STRIDE || q == EVAL_FIELD_ENV_STRIDE || reset == EVAL_FIELD_ENV_STRIDE) return "a field with an env stride < 1";
  if (a || q || reset) return "a vector field with a component stride < 1";
  int seen = 0;
  for (int s = 0; s < 12; ++s) {
    if (in->joint_of_slot[s] < 0 || in->joint_of_slot[s] > 11) return "joint_of_slot outside [0, 12)";
    seen |= 1 << in->joint_of_slot[s];
  }
  if (seen != 0xFFF) return "joint_of_slot: every joint once (a permutation of 0 .. 11)";
  return nullptr;
}

extern "C" {

int go2nn_spectrum_begin(float* trace, int32_t N, int32_t start, int32_t T, void* stream) {
  if (!trace || N < 1 || T < 1 || T > GO2NN_SPECTRUM_MAX_STEPS) FAIL(GO2NN_EINVAL, "spectrum begin: bad argument (a trace, N >= 1 and 1 <= T <= 2^20)");
  static_assert(GO2NN_SPECTRUM_TRACE_STEP == 0, "the STEP row is the trace's first N floats");
  return eval_table_begin(trace, 1 + GO2NN_SPECTRUM_CHANNELS * T, N, (float)start, stream);          // a frame that is never recorded reads as zeros
}

int go2nn_spectrum_record(const Go2nnSpectrumIn* in, float* trace, int32_t N, int32_t T, void* stream) {
  if (!in || !trace || N < 1 || T < 1 || T > GO2NN_SPECTRUM_MAX_STEPS) FAIL(GO2NN_EINVAL, "spectrum record: null argument, N < 1 or T outside [1, 2^20]");
  if (const char* bad = spectrum_in_bad(in)) FAIL(GO2NN_EINVAL, "spectrum record: %s", bad);
  return eval_per_env(SpectrumRecord{*in, trace, N, T}, N, stream);
}

int go2nn_spectrum_welch(const float* trace, int32_t N, int32_t T, int32_t W, double fs, const double* twiddle, float* table, void* stream) {
  if (!trace || !twiddle || !table || N < 1 || T < 1 || T > GO2NN_SPECTRUM_MAX_STEPS) FAIL(GO2NN_EINVAL, "spectrum welch: null argument, N < 1 or T outside [1, 2^20]");
  if (const char* bad = spectrum_window_bad(W)) FAIL(GO2NN_EINVAL, "spectrum welch: %s", bad);
  if (!(fs > 0.0) || !(fs <= 1.0e12)) FAIL(GO2NN_EINVAL, "spectrum welch: fs must be a finite sampling rate > 0");
  const SpectrumWelch a{trace, twiddle, table, N, T, W, 1.0 / (double)W, 1.0 / (fs * (0.375 * (double)W)), 2.0 / (double)W};
#ifdef GO2_EMU
  (void)stream;
  std::vector<double> x((size_t)SPECTRUM_SIGNALS * W);
  std::vector<float> acc(2 * 6 * (size_t)(W / 2 + 1));
  for (int e = 0; e < N; ++e) spectrum_welch_robot(a, e, x.data(), acc.data(), acc.data() + 6 * (W / 2 + 1));
#else
  const size_t lds = sizeof(double) * ((size_t)2 * W + (size_t)SPECTRUM_SIGNALS * W + SPECTRUM_SIGNALS);
  hipLaunchKernelGGL(spectrum_welch_kernel, dim3((unsigned)N), dim3(EVAL_THREADS), lds, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_spectrum_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, int32_t W, double* out, void* stream) {
  if (!table || !group || !out || N < 1 || G < 1 || G > 65535) FAIL(GO2NN_EINVAL, "spectrum reduce: bad argument (1 <= G <= 65535)");
  if (const char* bad = spectrum_window_bad(W)) FAIL(GO2NN_EINVAL, "spectrum reduce: %s", bad);
  return eval_reduce(SpectrumTerm{table, N, 0}, group, N, G, GO2NN_SPECTRUM_OUT_NUM(W), out, stream);
}

}  // extern "C"

#endif  // GO2NN_SPECTRUM_H
