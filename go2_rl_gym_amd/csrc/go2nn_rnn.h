// go2nn_rnn.h — the cell steps of the recurrent memory (include/go2nn.h ABI 7; rsl_rl/rsl_rl/modules/actor_critic_recurrent.py Memory = nn.LSTM / nn.GRU).
// Included at the end of go2nn_impl.cpp (FAIL, cdiv, HIPCHK are its helpers).
//
// The matrix products of a step (gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh) run on the split-operand / fp32-MFMA GEMMs of go2nn_gemm3.h / go2nn_gemm.h; what is
// here is the per-(row, hidden unit) part: torch's gate formulas (aten/src/ATen/native/RNN.cpp: LSTMCell, GRUCell) in fp32 on one thread per element, and
// their backward.  One lane owns (r, j) and touches only element (r, j) of every [B, H] tensor and column j of every gate block of row r, so the in-place
// aliases the header allows (h over h_prev, the carried gradients) are race-free.  The host build runs the same element functions in plain loops.
#ifndef GO2NN_RNN_H
#define GO2NN_RNN_H

#ifdef GO2_EMU
#define RNN_FN static inline
#else
#define RNN_FN __device__ __forceinline__
#endif

RNN_FN float rnn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// forward of element (r, j) of one job
RNN_FN void rnn_cell_fwd(const Go2nnRnnCellJob& q, int r, int j) {
  const int H = q.H;
  const size_t e = (size_t)r * H + j;
  const bool lstm = q.type == GO2NN_RNN_LSTM;
  const size_t gr = (size_t)r * (lstm ? 4 : 3) * H, sr = (size_t)r * 4 * H;
  const float hp = q.h_prev[e];
  const float cp = lstm ? q.c_prev[e] : 0.f;
  if (q.save_h) q.save_h[e] = hp;
  if (lstm && q.save_c) q.save_c[e] = cp;
  float h, c = 0.f;
  if (lstm) {
    const float i = rnn_sigmoid(q.gi[gr + j] + q.gh[gr + j]);
    const float f = rnn_sigmoid(q.gi[gr + H + j] + q.gh[gr + H + j]);
    const float g = tanhf(q.gi[gr + 2 * H + j] + q.gh[gr + 2 * H + j]);
    const float o = rnn_sigmoid(q.gi[gr + 3 * H + j] + q.gh[gr + 3 * H + j]);
    c = f * cp + i * g;
    h = o * tanhf(c);
    if (q.gates) { q.gates[sr + j] = i; q.gates[sr + H + j] = f; q.gates[sr + 2 * H + j] = g; q.gates[sr + 3 * H + j] = o; }
    q.c[e] = c;
  } else {
    const float rg = rnn_sigmoid(q.gi[gr + j] + q.gh[gr + j]);
    const float z = rnn_sigmoid(q.gi[gr + H + j] + q.gh[gr + H + j]);
    const float hn = q.gh[gr + 2 * H + j];
    const float n = tanhf(q.gi[gr + 2 * H + j] + rg * hn);
    h = (1.f - z) * n + z * hp;
    if (q.gates) { q.gates[sr + j] = rg; q.gates[sr + H + j] = z; q.gates[sr + 2 * H + j] = n; q.gates[sr + 3 * H + j] = hn; }
  }
  q.h[e] = h;
  if (q.next_h) {
    const bool sub = q.done && q.done[r];
    q.next_h[e] = sub ? q.sub_h[e] : h;
    if (lstm) q.next_c[e] = sub ? q.sub_c[e] : c;
  }
}

// backward of element (r, j) of one job
RNN_FN void rnn_cell_bwd(const Go2nnRnnCellBwdJob& q, int r, int j) {
  const int H = q.H;
  const size_t e = (size_t)r * H + j;
  const bool lstm = q.type == GO2NN_RNN_LSTM;
  const size_t gr = (size_t)r * (lstm ? 4 : 3) * H, sr = (size_t)r * 4 * H;
  const bool carry = q.dh_rec && !(q.done && q.done[r]);          // gradient of step t+1 through the carry t -> t+1
  float dh = q.dy[e];
  if (carry) dh += q.dh_rec[e];
  if (lstm) {
    const float i = q.gates[sr + j], f = q.gates[sr + H + j], g = q.gates[sr + 2 * H + j], o = q.gates[sr + 3 * H + j];
    const float tc = tanhf(q.c[e]);
    float dc = dh * o * (1.f - tc * tc);
    if (carry) dc += q.dc[e];
    const float di = dc * g * i * (1.f - i), df = dc * q.c_prev[e] * f * (1.f - f), dg = dc * i * (1.f - g * g), dout = dh * tc * o * (1.f - o);
    q.dgi[gr + j] = di; q.dgi[gr + H + j] = df; q.dgi[gr + 2 * H + j] = dg; q.dgi[gr + 3 * H + j] = dout;
    q.dgh[gr + j] = di; q.dgh[gr + H + j] = df; q.dgh[gr + 2 * H + j] = dg; q.dgh[gr + 3 * H + j] = dout;
    q.dc[e] = dc * f;
  } else {
    if (carry) dh += q.dh_carry[e];
    const float rg = q.gates[sr + j], z = q.gates[sr + H + j], n = q.gates[sr + 2 * H + j], hn = q.gates[sr + 3 * H + j];
    const float dn = dh * (1.f - z) * (1.f - n * n);
    const float dz = dh * (q.h_prev[e] - n) * z * (1.f - z);
    const float dr = dn * hn * rg * (1.f - rg);
    q.dgi[gr + j] = dr; q.dgi[gr + H + j] = dz; q.dgi[gr + 2 * H + j] = dn;
    q.dgh[gr + j] = dr; q.dgh[gr + H + j] = dz; q.dgh[gr + 2 * H + j] = dn * rg;
    q.dh_carry[e] = dh * z;
  }
}

#ifndef GO2_EMU
struct RnnFwdArgs { Go2nnRnnCellJob job[GO2NN_MAX_GROUP]; };
struct RnnBwdArgs { Go2nnRnnCellBwdJob job[GO2NN_MAX_GROUP]; };
struct RnnResetArgs { float* s[GO2NN_RNN_MAX_STATES]; int n, L, B, H; const uint8_t* done; };

// grid = (ceil(B H / 256), njobs); consecutive lanes walk the hidden units of a row: every load and store is a dense line
__global__ void __launch_bounds__(256) go2nn_rnn_fwd_kernel(const RnnFwdArgs a) {
  const Go2nnRnnCellJob& q = a.job[blockIdx.y];
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < (long long)q.B * q.H) rnn_cell_fwd(q, (int)(k / q.H), (int)(k % q.H));
}
__global__ void __launch_bounds__(256) go2nn_rnn_bwd_kernel(const RnnBwdArgs a) {
  const Go2nnRnnCellBwdJob& q = a.job[blockIdx.y];
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < (long long)q.B * q.H) rnn_cell_bwd(q, (int)(k / q.H), (int)(k % q.H));
}
__global__ void __launch_bounds__(256) go2nn_rnn_reset_kernel(const RnnResetArgs a) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)a.L * a.B * a.H;
  if (k >= per) return;
  const int r = (int)((k / a.H) % a.B);
  if (!a.done[r]) return;
  for (int s = 0; s < a.n; ++s) a.s[s][k] = 0.f;
}
#endif

static int rnn_job_ok(int B, int H, int type) { return B >= 1 && H >= 1 && H <= GO2NN_MAX_WIDTH && (type == GO2NN_RNN_LSTM || type == GO2NN_RNN_GRU); }

extern "C" {

int go2nn_rnn_cell_forward(const Go2nnRnnCellJob* jobs, int32_t njobs, void* stream) {
  if (!jobs || njobs < 1 || njobs > GO2NN_MAX_GROUP) FAIL(GO2NN_EINVAL, "rnn cell forward: 1..%d jobs", GO2NN_MAX_GROUP);
  long long most = 0;
  for (int k = 0; k < njobs; ++k) {
    const Go2nnRnnCellJob& q = jobs[k];
    const bool lstm = q.type == GO2NN_RNN_LSTM;
    if (!rnn_job_ok(q.B, q.H, q.type) || !q.gi || !q.gh || !q.h_prev || !q.h || (lstm && (!q.c_prev || !q.c)) || (lstm && q.save_h && !q.save_c) ||
        (q.next_h && (!q.sub_h || (lstm && (!q.sub_c || !q.next_c)))))
      FAIL(GO2NN_EINVAL, "rnn cell forward: job %d: bad argument (type 0 LSTM / 1 GRU, 1 <= H <= %d, the LSTM's cell-state pointers)", k, GO2NN_MAX_WIDTH);
    most = std::max(most, (long long)q.B * q.H);
  }
#ifdef GO2_EMU
  (void)stream;
  for (int k = 0; k < njobs; ++k)
    for (int r = 0; r < jobs[k].B; ++r)
      for (int j = 0; j < jobs[k].H; ++j) rnn_cell_fwd(jobs[k], r, j);
#else
  RnnFwdArgs a;
  for (int k = 0; k < njobs; ++k) a.job[k] = jobs[k];
  hipLaunchKernelGGL(go2nn_rnn_fwd_kernel, dim3((unsigned)((most + 255) / 256), njobs), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_rnn_cell_backward(const Go2nnRnnCellBwdJob* jobs, int32_t njobs, void* stream) {
  if (!jobs || njobs < 1 || njobs > GO2NN_MAX_GROUP) FAIL(GO2NN_EINVAL, "rnn cell backward: 1..%d jobs", GO2NN_MAX_GROUP);
  long long most = 0;
  for (int k = 0; k < njobs; ++k) {
    const Go2nnRnnCellBwdJob& q = jobs[k];
    const bool lstm = q.type == GO2NN_RNN_LSTM;
    if (!rnn_job_ok(q.B, q.H, q.type) || !q.gates || !q.dy || !q.dgi || !q.dgh || (lstm && (!q.c || !q.c_prev || !q.dc)) || (!lstm && (!q.h_prev || !q.dh_carry)))
      FAIL(GO2NN_EINVAL, "rnn cell backward: job %d: bad argument", k);
    most = std::max(most, (long long)q.B * q.H);
  }
#ifdef GO2_EMU
  (void)stream;
  for (int k = 0; k < njobs; ++k)
    for (int r = 0; r < jobs[k].B; ++r)
      for (int j = 0; j < jobs[k].H; ++j) rnn_cell_bwd(jobs[k], r, j);
#else
  RnnBwdArgs a;
  for (int k = 0; k < njobs; ++k) a.job[k] = jobs[k];
  hipLaunchKernelGGL(go2nn_rnn_bwd_kernel, dim3((unsigned)((most + 255) / 256), njobs), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_rnn_reset(float* const* states, int32_t nstates, int32_t L, int32_t B, int32_t H, const uint8_t* done, void* stream) {
  if (!states || nstates < 1 || nstates > GO2NN_RNN_MAX_STATES || L < 1 || B < 1 || H < 1 || !done) FAIL(GO2NN_EINVAL, "rnn reset: bad argument (1..%d states)", GO2NN_RNN_MAX_STATES);
  for (int s = 0; s < nstates; ++s) if (!states[s]) FAIL(GO2NN_EINVAL, "rnn reset: state %d is NULL", s);
  const long long per = (long long)L * B * H;
#ifdef GO2_EMU
  (void)stream;
  for (int s = 0; s < nstates; ++s)
    for (long long k = 0; k < per; ++k) if (done[(k / H) % B]) states[s][k] = 0.f;
#else
  RnnResetArgs a;
  for (int s = 0; s < nstates; ++s) a.s[s] = states[s];
  a.n = nstates; a.L = L; a.B = B; a.H = H; a.done = done;
  hipLaunchKernelGGL(go2nn_rnn_reset_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_RNN_H
