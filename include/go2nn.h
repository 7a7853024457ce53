/* go2nn.h — C ABI of the policy-side MFMA kernels (libgo2nn_hip.so, gfx950).
 *
 * What it replaces, in the rollout of OnPolicyRunner.learn (rsl_rl/rsl_rl/runners/on_policy_runner.py:135-153): PPO.act
 * (rsl_rl/rsl_rl/algorithms/ppo.py:90-102) = ActorCritic.act + evaluate + get_actions_log_prob
 * (rsl_rl/rsl_rl/modules/actor_critic.py:119-136): two 4-layer MLPs (Linear, ELU, ..., Linear; :50-75), a Gaussian sample
 * a = mu + std * eps, its log-probability, and the rows PPO.act keeps for RolloutStorage.add_transitions
 * (rsl_rl/rsl_rl/storage/rollout_storage.py:88-101).  In PyTorch that is ~30 launches per env step (8 GEMMs, 6 ELUs, the sampling head)
 * at M = 4096 rows — launch-latency-bound; here it is ONE launch: a workgroup carries 32 rows through all layers of one network on the
 * matrix pipe, activations in LDS, weights streamed from L2 in a pre-packed operand order.  Arithmetic: fp32 operands split EXACTLY into
 * three bf16 planes, six v_mfma_f32_32x32x16_bf16 terms per product, fp32 accumulate (csrc/go2nn_mlp3.h; no operand bit is dropped, the
 * results are as close to float64 as an fp32 evaluation's); with GO2_GEMM_SPLIT=0 in the environment, or for networks whose activations
 * do not fit the LDS as planes (two neighbouring 512-wide layers), v_mfma_f32_32x32x2_f32 on the fp32 values (csrc/go2nn_impl.cpp).
 *
 * Plain pointers and sizes, no torch types; asynchronous on the given HIP stream; 0 = ok, negative = error (go2nn_last_error).
 * All pointers are device pointers unless stated. */
#ifndef GO2NN_H
#define GO2NN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO2NN_ABI_VERSION 7      /* 2: + the learner-side kernels (go2nn_head_backward, go2nn_linear_*); 3: + the grouped (actor + critic) layer calls; 4: + split-operand (3 x bf16) products;
                                    5: + the CTS pieces: layers without activation, plain input gradients, the latent normaliser forward / backward, the split surrogate, two-segment policy inputs;
                                    6: + Go2nnBwdInJob.x_in: the weight gradient of the layer below out of the input gradient's epilogue (its gz_prev never goes to HBM);
                                    7: + the recurrent memory's cell steps (LSTM / GRU) and state reset */
#define GO2NN_MAX_LAYERS 6
#define GO2NN_MAX_WIDTH 512      /* widest layer input / output (LDS holds two 32-row activation tiles of this width) */
#define GO2NN_EINVAL (-22)
#define GO2NN_EDEVICE (-5)

/* An MLP as torch.nn.Sequential(Linear, ELU(alpha=1), ..., Linear) holds it: weight[l] is [dims[l+1], dims[l]] row-major (out x in),
 * bias[l] is [dims[l+1]].  Host struct with device pointers. */
typedef struct Go2nnMlp {
  int32_t num_layers;
  int32_t dims[GO2NN_MAX_LAYERS + 1];
  const float* weight[GO2NN_MAX_LAYERS];
  const float* bias[GO2NN_MAX_LAYERS];
} Go2nnMlp;

int go2nn_abi_version(void);
const char* go2nn_last_error(void);

/* Number of floats of the packed operand buffer of `m` (weights in MFMA B-operand order for both arithmetics — fp32 zero-padded to 32 x 8 tiles, the three bf16 planes
 * to 32 x 16 —, + padded biases; the layout is the library's own);
 * negative on an unsupported shape (more than GO2NN_MAX_LAYERS layers, a dimension above GO2NN_MAX_WIDTH). */
int64_t go2nn_packed_floats(const Go2nnMlp* m);
/* Which kernel evaluates `m` in the calls below (a host-side query, no device work): 3 = the split-operand kernel (csrc/go2nn_mlp3.h: three bf16 planes, six bf16-MFMA terms),
 * 1 = the fp32-MFMA kernel (GO2_GEMM_SPLIT=0 in the environment, or activations that do not fit the LDS as planes), 0 = the host test build's loops; negative on an unsupported
 * shape.  bench.py and the GPU tests read it so that a fall-back to the slower kernel cannot go unnoticed. */
int32_t go2nn_mlp_arith(const Go2nnMlp* m);
/* Re-pack the CURRENT weights of `m` into `packed` (call after every optimizer step that the next forward must see; one small launch). */
int go2nn_pack(const Go2nnMlp* m, float* packed, void* stream);

/* y[N, dims[last]] = m(x[N, dims[0]]) — one launch (ActorCritic.act_inference / evaluate, actor_critic.py:131-136). */
int go2nn_mlp_forward(const Go2nnMlp* m, const float* packed, const float* x, float* y, int32_t N, void* stream);

/* PPO.act for one policy step (ppo.py:90-102), one launch:
 *   mu = actor(obs), value = critic(critic_obs), a = mu + std * eps (two separately rounded operations, like the eager formulation),
 *   log_prob = sum_j [-(a_j - mu_j)^2 / (2 std_j^2) - log std_j - log sqrt(2 pi)]   (j ascending)
 * a_out [N,A] receives the actions (the tensor env.step gets); the *_st pointers receive the storage rows of this step and may be NULL:
 * actions [N,A], mu [N,A], sigma [N,A], log-prob [N], value [N].  eps [N,A] are standard-normal draws supplied by the caller. */
int go2nn_policy_act(const Go2nnMlp* actor, const float* actor_packed, const Go2nnMlp* critic, const float* critic_packed,
                     const float* obs, const float* critic_obs, const float* std, const float* eps,
                     float* a_out, float* a_st, float* mu_st, float* sig_st, float* lp_st, float* v_st, int32_t N, void* stream);

/* ---- ABI 5: the same kernel in the rollout of the Concurrent Teacher-Student runner (rsl_rl/rsl_rl/runners/on_policy_runner_cts.py:135-160 -> algorithms/cts.py:112-149 ->
 * modules/actor_critic_cts.py:146-176): per step the reference gathers teacher / student env rows, runs teacher_encoder(privileged obs) resp. student_encoder(history),
 * normalises, cats [latent | obs] and [latent | privileged obs], runs actor and critic, samples — ~45 launches.  Here: TWO launches.
 *   go2nn_mlp_forward_rows   up to two MLPs in one launch, each on its own row subset `rows[0 .. nrows)` of its inputs (the teacher / student envs; NULL: rows 0 .. nrows - 1),
 *                            its input row made of two column segments (x: columns [0, kx), x2: the rest), its output stored at the SAME row index of y (pitch ldy),
 *                            L2-normalised (F.normalize: x / max(|x|, 1e-12)) when `normalize` — both encoders write the env-ordered latent [N, L] directly
 *   go2nn_policy_act_latent  go2nn_policy_act with the actor's input = [latent | obs] and the critic's = [latent | critic_obs] read as two segments (no cat);
 *                            actor->dims[0] = L + obs width, critic->dims[0] = L + critic_obs width */
typedef struct Go2nnMlpIO {
  const float* x; const float* x2;      /* input segments (x2 may be NULL when kx = the network's input width) */
  const int32_t* rows;                  /* device int32 [nrows] or NULL */
  float* y;
  int32_t ldx, ldx2, kx, nrows, ldy, normalize;
} Go2nnMlpIO;
int go2nn_mlp_forward_rows(const Go2nnMlp* const* nets, const float* const* packed, const Go2nnMlpIO* io, int32_t nnets, void* stream);
int go2nn_policy_act_latent(const Go2nnMlp* actor, const float* actor_packed, const Go2nnMlp* critic, const float* critic_packed,
                            const float* latent, int32_t L, const float* obs, const float* critic_obs, const float* std, const float* eps,
                            float* a_out, float* a_st, float* mu_st, float* sig_st, float* lp_st, float* v_st, int32_t N, void* stream);

/* ---- learner side: PPO.update's backward pass (rsl_rl/rsl_rl/algorithms/ppo.py:120-187; autograd over modules/actor_critic.py:50-75) ----
 *
 * Backward of an MLP's tail  h -> Linear -> ELU(alpha=1) -> y [B,K] -> Linear(W [C,K], b [C]) -> out [B,C]  for a NARROW output (C <= 16: the
 * 12-wide action mean, the 1-wide value), given gy = dLoss/d out [B,C], in one streaming pass over y:
 *   gz [B,K]  = (gy W) * (y > 0 ? 1 : y + 1)      the gradient at the hidden layer's PRE-activation (torch: mm + elu_backward(is_result))
 *   sums      = [ dW [C,K] = gy^T y | gb [K] = column sums of gz (the hidden Linear's bias gradient) | db [C] = column sums of gy ]
 * i.e. what autograd computes with two GEMMs of degenerate shape, a split-K fix-up, two column-sum reductions and an element-wise pass.
 * Sums are formed in a fixed order (per-workgroup partials, then a fixed tree): bit-reproducible from run to run.
 * K a multiple of 4, K <= GO2NN_MAX_WIDTH.  workspace: go2nn_head_backward_workspace(B, C, K) floats (negative: unsupported shape). */
/* Second stage of the fixed-order reductions: out[c] = sum_r part[r][c] (part [nrows, ncols] row-major) for up to 16 jobs in ONE launch.
 * go2nn_head_backward (sums == NULL) and go2nn_linear_backward_input (gb_prev == NULL) then leave their per-workgroup partial rows in `workspace` —
 * go2nn_*_rows rows of (C + 1) K + C resp. Kin columns — and the caller finishes all of a backward pass's reductions (and the row splits of its
 * weight gradients) with one go2nn_sum_rows call, off the chain of dependent GEMMs. */
typedef struct Go2nnSumJob { const float* part; float* out; int32_t nrows, ncols; float* acc; int32_t nacc, pad_; int32_t out_w, out_ld; } Go2nnSumJob;      /* ABI 4: acc != NULL: acc[c] += out[c] for c < nacc (a running sum over launches, e.g. the update's mean losses) */
/* ABI 6: out_w > 0: the sums are a [ncols / out_w, out_w] matrix written with row pitch out_ld — a column block of a wider matrix (a weight gradient assembled from
 * two launches' partials: Go2nnBwdInJob.x_in, Go2nnBwdWJob.ldx); 0: dense */
#define GO2NN_MAX_SUM_JOBS 32      /* (ABI 5: was 16 — a CTS policy step finishes 19 reductions in one launch) */
int go2nn_sum_rows(const Go2nnSumJob* jobs, int32_t njobs, void* stream);
int32_t go2nn_head_backward_rows(int32_t B, int32_t C, int32_t K);
int32_t go2nn_linear_backward_input_rows(int32_t M, int32_t C, int32_t Kin);
int64_t go2nn_head_backward_workspace(int32_t B, int32_t C, int32_t K);
int go2nn_head_backward(const float* gy, const float* y, const float* w, float* gz, float* sums, float* workspace, int32_t B, int32_t C, int32_t K, void* stream);

/* The hidden layers  y = elu(x W^T + b)  of the same MLPs, forward and backward, as fp32-MFMA GEMMs whose epilogues do the element-wise work that
 * follows a vendor GEMM as separate passes over the [M, N] activations (torch: addmm + elu_; mm + elu_backward + sum(0); a row-split bmm + sum(0)).
 * x [M,K], W [N,K] (torch.nn.Linear layout), b [N], y [M,N]; all row-major and dense.  Any M, N, K >= 1 (ragged edges are masked; 16-byte loads
 * are used when a row length is a multiple of 4).  ELU through the hardware exponential as in go2nn_policy_act. */
int go2nn_linear_elu_forward(const float* x, const float* w, const float* b, float* y, int32_t M, int32_t K, int32_t N, void* stream);
/* Backward of a layer with C outputs and Kin inputs, given gz [M,C] = the gradient at ITS pre-activation:
 *   go2nn_linear_backward_input:  gz_prev [M,Kin] = (gz W) * (y_prev > 0 ? 1 : y_prev + 1)   where y_prev [M,Kin] = the layer's input = the previous
 *                                 layer's ELU output; gb_prev [Kin] = column sums of gz_prev (the previous layer's bias gradient)
 *   go2nn_linear_backward_weight: dw [C,Kin] = gz^T x                                          (x [M,Kin] = the layer's input)
 * both with fixed-order sums (bit-reproducible).  workspace: go2nn_linear_backward_workspace(M, C, Kin) floats serve either call. */
int64_t go2nn_linear_backward_workspace(int32_t M, int32_t C, int32_t Kin);
int go2nn_linear_backward_input(const float* gz, const float* w, const float* y_prev, float* gz_prev, float* gb_prev, float* workspace,
                                int32_t M, int32_t C, int32_t Kin, void* stream);
int go2nn_linear_backward_weight(const float* gz, const float* x, float* dw, float* workspace, int32_t M, int32_t C, int32_t Kin, void* stream);


/* ---- ABI 3: one layer of SEVERAL independent MLPs per launch (PPO.update evaluates the same layer of the actor and of the critic back to back:
 * ppo.py:131-133 -> actor_critic.py:119-136; as two launches on two HIP streams the pair takes twice one network's time and needs the second stream).
 * A group is 1..GO2NN_MAX_GROUP jobs; the jobs' tiles form one grid.  Same arithmetic and the same fixed summation orders as the single calls.
 *   forward:       y = elu(x W^T + b) per job (M, K may differ between the jobs; the 45- and 263-wide input layers are one group)
 *   input grad:    gz_prev = (gz W) * elu'(y_prev); column partial sums of gz_prev are left in the job's `workspace` as
 *                  go2nn_linear_backward_input_group_rows(M, C, Kin) rows of Kin columns (the caller finishes them with go2nn_sum_rows)
 *   weight grad:   row-slice partials of dW = gz^T x are left in the job's `workspace` as go2nn_linear_backward_weight_group_rows(jobs, njobs) rows of
 *                  C * Kin columns (every job of a group has the same M); operands go from global memory straight into MFMA registers (both are
 *                  contiguous along the output index), the four waves of a workgroup split the rows of one output tile
 * workspace floats per job: rows * Kin resp. rows * C * Kin. */
#define GO2NN_MAX_GROUP 2
/* ABI 5 (what was padding; 0 keeps the ABI 3 / 4 meaning).  Every job of a group carries the same flag.
 *   Go2nnFwdJob.act     0: y = elu(x W^T + b);  1: y = x W^T + b — the LAST Linear of an encoder, whose output goes to a normaliser instead of an ELU
 *                       (rsl_rl/rsl_rl/modules/actor_critic_cts.py:49-80: teacher_encoder / student_encoder = MLP -> L2Norm)
 *   Go2nnBwdInJob.plain 0: gz_prev = (gz W) * elu'(y_prev) + column partials;  1: gz_prev = gz W — the gradient at the INPUT of a network's first layer
 *                       (CTS: d loss / d [latent | obs], actor_critic_cts.py:146-151 -> autograd); y_prev and workspace are not read
 *   Go2nnBwdInJob.ld    row pitch in floats of y_prev and gz_prev, 0 = Kin (dense).  A pitch > Kin addresses a column block of a wider matrix: the E expert heads of
 *                       a MoE encoder (rsl_rl/rsl_rl/modules/utils.py:78-93, Conv1d(groups=E)) read their 128 columns of the shared [M, E * 128] backbone output and
 *                       write the matching block of its gradient, ELU' and bias partials in the epilogue, with no transposing copy in between; the job's
 *                       workspace stays dense (rows x Kin) */
typedef struct Go2nnFwdJob { const float *x, *w, *b; float* y; int32_t M, K, N; int32_t act; const void* w_split; } Go2nnFwdJob;
 /* ABI 6 (appended fields; NULL / 0 keep the ABI 5 meaning).  Every job of a group alike; split-operand kernels only (w_split set), plain 0, ld 0.
 *   Go2nnBwdInJob.x_in  the input x [M, Kx] (dense, 1 <= Kx <= 64) of the layer BELOW — the one whose ELU output is y_prev.  The job then ALSO leaves that layer's weight
 *                       gradient  dW_prev [Kin, Kx] = gz_prev^T x_in  as go2nn_linear_backward_input_fused_rows(M) partial rows of Kin * Kx columns in `dw_workspace`
 *                       (finished by go2nn_sum_rows), formed from the gz_prev tile while it is still in the accumulators: autograd's mm(gz_prev.t(), x) (ppo.py:173
 *                       loss.backward() through the FIRST Linear of actor_critic.py:50-75) without gz_prev's round trip through HBM.  gz_prev may then be NULL (PPO: nothing
 *                       else reads the gradient at the first layer's pre-activation); `workspace` keeps its meaning and its row count.
 *   Go2nnBwdInJob.ldx   row pitch of x_in in floats, 0 = Kx: x_in may be a column block of a wider input — a 263-wide critic input leaves its last 7 columns' weight
 *                       gradient here and its first 256 = two whole 128-column tiles to go2nn_linear_backward_weight_group (Go2nnBwdWJob.ldx), which would otherwise pad
 *                       263 to 384 columns */
typedef struct Go2nnBwdInJob { const float *gz, *w, *y_prev; float *gz_prev, *workspace; int32_t M, C, Kin; int32_t plain; const void* w_split; int32_t ld;
                               int32_t Kx; const float* x_in; float* dw_workspace; int32_t ldx; } Go2nnBwdInJob;
typedef struct Go2nnBwdWJob { const float *gz, *x; float* workspace; int32_t M, C, Kin; int32_t split; int32_t ldx; } Go2nnBwdWJob;      /* ABI 6: ldx = row pitch of x, 0 = Kin (split-operand kernel only) */
int go2nn_linear_elu_forward_group(const Go2nnFwdJob* jobs, int32_t njobs, void* stream);
int32_t go2nn_linear_backward_input_group_rows(int32_t M, int32_t C, int32_t Kin);
int go2nn_linear_backward_input_group(const Go2nnBwdInJob* jobs, int32_t njobs, void* stream);
int32_t go2nn_linear_backward_input_fused_rows(int32_t M);          /* ABI 6: partial rows of dw_workspace */
int32_t go2nn_linear_backward_weight_group_rows(const Go2nnBwdWJob* jobs, int32_t njobs);
int go2nn_linear_backward_weight_group(const Go2nnBwdWJob* jobs, int32_t njobs, void* stream);
/* Which kernel a shape gets (host-side queries, no device work; the host test build returns 0 like go2nn_mlp_arith).  ADDED WITHIN ABI 7: two new entry points, nothing
 * existing changes, GO2NN_ABI_VERSION stays 7.  The GPU tests read them so that a case meant for one tile path cannot drift to another when a selection rule changes.
 *   go2nn_linear_group_tile_rows            rows per workgroup tile (64, 128 or 192) of the split-operand (w_split set) forward or input-gradient group launch of M rows whose
 *                                           jobs are N0 and N1 columns wide (N1 = 0: one job; the input gradient's columns are its Kin); tm_max = GO2NN_TM_MAX_FORWARD resp.
 *                                           GO2NN_TM_MAX_INPUT_GRAD — the launches pass the same constants to the same selection function (the fused x_in launch is always 128)
 *   go2nn_linear_backward_weight_group_kernel   the kernel go2nn_linear_backward_weight_group runs for `jobs` (GO2NN_WGRAD_*), with its number of row slices
 *                                           (= go2nn_linear_backward_weight_group_rows) and the rows of one slice; negative on a group that call would refuse */
#define GO2NN_TM_MAX_FORWARD 3
#define GO2NN_TM_MAX_INPUT_GRAD 2
#define GO2NN_WGRAD_F32_64x64 1        /* fp32 MFMA, 64 x 64 tiles (some Kin is not a multiple of 128) */
#define GO2NN_WGRAD_F32_64x128 2       /* fp32 MFMA, 64 x 128 tiles */
#define GO2NN_WGRAD_SPLIT_128x128 3    /* split-operand (Go2nnBwdWJob.split on every job, C in whole 128-row tiles, enough tiles) */
int32_t go2nn_linear_group_tile_rows(int32_t M, int32_t N0, int32_t N1, int32_t tm_max);
int32_t go2nn_linear_backward_weight_group_kernel(const Go2nnBwdWJob* jobs, int32_t njobs, int32_t* nslices, int32_t* rows_per_slice);

/* ---- ABI 4: the same three products on the bf16 matrix pipe WITHOUT giving up fp32 operands.  Every fp32 value is split exactly into three bf16 planes
 * (8 + 8 + 8 significand bits) and a product is six bf16 MFMA terms accumulated in fp32 — the three terms left out are below 2^-23 of the product, i.e. below
 * the rounding of an fp32 multiply; against float64 the results are as close as the fp32-MFMA kernels' (tools/gemm3_bench.cpp, tests/test_gpu_mlp_tail.py hold both
 * to the same tolerances; rms error 0.8 - 1.2 x).  One measurable difference: the bf16 pipe's accumulation is not round-to-nearest-even, every output carries a bias of
 * about a third of an fp32 ulp towards -inf, which a column sum over 24576 rows turns into ~1.5e-6 of the sum (fp32 kernels: ~4e-7).  v_mfma_f32_32x32x16_bf16 moves 16 k per 32 cycles, v_mfma_f32_32x32x2_f32 2 k per 64: six terms cost 3/8 of the fp32 form.
 *   go2nn_split_weights   a layer's weight [N,K] -> its split image for both orientations (forward: rows n; input gradient: rows k), `go2nn_split_weights_bytes`
 *                         bytes in a caller-owned buffer; run once after every optimizer step (one launch for up to 8 layers)
 *   Go2nnFwdJob.w_split / Go2nnBwdInJob.w_split   that image: non-NULL selects the split-operand kernel for the group (every job of a group alike)
 *   Go2nnBwdWJob.split    1 selects it for the weight gradient (both operands are activations: split in registers, no image)
 * NULL / 0 keep the fp32-MFMA kernels (bit-for-bit the ABI 3 results). */
typedef struct Go2nnSplitJob { const float* w; void* image; int32_t N, K; } Go2nnSplitJob;
#define GO2NN_MAX_SPLIT_JOBS 16      /* (ABI 5: was 8 — teacher encoder + actor + critic of a CTS policy step are 9 hidden layers) */
int64_t go2nn_split_weights_bytes(int32_t N, int32_t K);
int go2nn_split_weights(const Go2nnSplitJob* jobs, int32_t njobs, void* stream);


/* The narrow heads of BOTH networks forward, the PPO loss head (rsl_rl/rsl_rl/algorithms/ppo.py:131-170: Gaussian log-prob, ratio, clipped surrogate, clipped
 * value loss, entropy, KL) with its analytic gradients, and the heads backward, as ONE streaming pass over the last hidden activations y_a, y_c [B,K] of the
 * actor (head W_mu [A,K], b_mu [A]) and the critic (head w_v [1,K], b_v [1]) — in place of two degenerate GEMMs, go2sim_ppo_loss and two go2nn_head_backward
 * launches.  Same arithmetic as go2sim_ppo_loss (torch.max tie splitting, clamp gradient semantics) with every row weighted 1 / B.
 * Out: gz_a, gz_c [B,K] = the gradients at the last hidden layers' pre-activations; `partials` = go2nn_ppo_heads_rows(B, A, K) rows of
 * go2nn_ppo_heads_cols(A, K) columns whose column sums (go2nn_sum_rows) are
 *   [ surrogate, value loss, KL, entropy (means) | d loss/d std [A] | dW_mu [A,K] | gb_a [K] | db_mu [A] | dW_v [K] | gb_c [K] | db_v ]
 * (gb_*: bias gradient of the last hidden layer = column sums of gz_*).  A <= 16, K a multiple of 4 up to 256.  Fixed summation order.
 * ABI 5: surrogate_split = n > 0 gives the CTS surrogate (rsl_rl/rsl_rl/algorithms/cts.py:228-231): mean over rows [0, n) + mean over rows [n, B) — a row's surrogate
 * and its gradient are weighted 1 / n resp. 1 / (B - n) instead of 1 / B (go2sim_ppo_loss's surrogate_split); value loss, KL and entropy keep 1 / B. */
typedef struct Go2nnPpoHeads {
  const float *y_a, *y_c, *w_mu, *b_mu, *w_v, *b_v, *std, *actions, *old_mu, *old_sigma, *old_logp, *adv, *old_values, *returns;
  float *gz_a, *gz_c, *partials;
  int32_t B, A, K, use_clipped_value_loss;
  float clip, value_loss_coef, entropy_coef;
  int32_t surrogate_split;
} Go2nnPpoHeads;
int32_t go2nn_ppo_heads_rows(int32_t B, int32_t A, int32_t K);
int32_t go2nn_ppo_heads_cols(int32_t A, int32_t K);
int go2nn_ppo_heads(const Go2nnPpoHeads* a, void* stream);


/* ---- ABI 5: the latent normaliser of the Concurrent Teacher-Student networks (rsl_rl/rsl_rl/modules/utils.py:24-30 L2Norm = F.normalize(x, p=2, dim=-1): x / max(|x|, 1e-12);
 * rsl_rl/rsl_rl/modules/actor_critic_cts.py:49-80,146-176: latent = L2Norm(encoder MLP), actor input = [latent | obs], critic input = [latent.detach() | privileged obs]).
 * Row-wise streaming kernels over [n, L] (L a multiple of 4, <= 128); fixed summation orders.
 *
 * go2nn_latent_concat: zhat = z / max(|z|, 1e-12) written into columns [0, L) of up to two row-major destinations with their own row pitch (the [latent | obs] and
 *   [latent | privileged obs] input matrices of the actor and the critic: torch.cat + two copies in the reference), inv_norm [n] = 1 / max(|z|, 1e-12) kept for the backward pass
 *   (dst_b, inv_norm may be NULL).
 * go2nn_l2norm_backward: g = d loss / d zhat read from columns [0, L) of a matrix with row pitch ldg (the plain input gradient of the actor's first layer), zhat likewise
 *   (pitch ldz):  dz = (g - zhat (zhat . g)) * inv_norm  -> dz [n, L] dense; column partial sums of dz (the encoder's last bias gradient) as
 *   go2nn_l2norm_backward_rows(n) rows of L columns in `partials` (finished by go2nn_sum_rows).
 * go2nn_latent_mse: the student step of CTS (rsl_rl/rsl_rl/algorithms/cts.py:259-275): shat = normalise(z_s), that = normalise(z_t),
 *   loss = mean((that - shat)^2) over n L elements; dz_s = gradient of the loss at the student encoder's un-normalised output z_s.  `partials` = go2nn_l2norm_backward_rows(n)
 *   rows of 4 + L columns: [ loss, 0, 0, 0 | column sums of dz_s ].  grad_scale multiplies dz_s (1: the plain MSE). */
int32_t go2nn_l2norm_backward_rows(int32_t n);
int go2nn_latent_concat(const float* z, int32_t n, int32_t L, float* dst_a, int32_t lda, float* dst_b, int32_t ldb, float* inv_norm, void* stream);
int go2nn_l2norm_backward(const float* g, int32_t ldg, const float* zhat, int32_t ldz, const float* inv_norm, float* dz, float* partials, int32_t n, int32_t L, void* stream);
int go2nn_latent_mse(const float* z_s, const float* z_t, float* dz_s, float* partials, int32_t n, int32_t L, float grad_scale, void* stream);

/* The loss head of the MoE student step (rsl_rl/rsl_rl/modules/utils.py:96-152: MoE.forward + StudentMoEEncoder's normaliser; rsl_rl/rsl_rl/algorithms/moe_cts.py:203-214):
 *   w = softmax(logits [n, E]);  y = sum_e w_e outs[:, e, :] (outs [n, E, L]);  shat = y / max(|y|, 1e-12);  latent loss = mean((t_hat - shat)^2)   (t_hat [n, L]: the teacher's
 *   NORMALISED latent);  usage = mean over rows of w;  load balance = mean_e((usage_e - 1 / E)^2);  loss = latent + lb_coef * load balance
 * with its analytic gradients — two launches (the load-balance gradient needs the batch mean of the gate first) in place of ~55 element-wise / reduction launches of autograd:
 *   go2nn_moe_usage      partials = go2nn_l2norm_backward_rows(n) rows of E: column partial sums of w (go2nn_sum_rows -> usage_sum [E], sums not means)
 *   go2nn_moe_mix_loss   d_logits [n, E], d_outs [n, E, L] = d loss / d logits, / d outs;  partials = go2nn_l2norm_backward_rows(n) rows of 4: [ latent loss | load balance (row 0) | 0 | 0 ]
 * E <= 16; L as above.  Fixed summation order. */
int go2nn_moe_usage(const float* logits, float* partials, int32_t n, int32_t E, void* stream);
int go2nn_moe_mix_loss(const float* logits, const float* outs, const float* t_hat, const float* usage_sum, float* d_logits, float* d_outs, float* partials,
                       int32_t n, int32_t E, int32_t L, float lb_coef, int32_t expert_major, const float* bias, float* dbias_partials, void* stream);
/* ABI 6: the mixture FORWARD only — the student rows of a rollout step (rsl_rl/rsl_rl/algorithms/cts.py:112-149: CTS.act evaluates the student encoder without gradient):
 *   z[rows ? rows[r] : r][0 .. L) = normalise(sum_e softmax(logits[r])_e (outs[r, e] + bias[e]))     z has row pitch ldz (a multiple of 4, 16-byte aligned rows)
 * one launch in place of softmax, a broadcast product, a sum, the normaliser's four element-wise / reduction kernels and the index_copy into the env-ordered latent. */
int go2nn_moe_mix_forward(const float* logits, const float* outs, const float* bias, const int32_t* rows, float* z, int32_t ldz, int32_t n, int32_t E, int32_t L,
                          int32_t expert_major, void* stream);
/* expert_major 1: outs / d_outs are [E, n, L] (the batched GEMM's own layout: no transposing copies either way).  bias (optional, [E, L]): the expert heads' output bias,
 * added to outs here — autograd then differentiates a plain batched product — with its gradient left as go2nn_l2norm_backward_rows(n) partial rows of E L columns in
 * dbias_partials (a 77 us torch reduction otherwise). */

/* ---- ABI 7: the recurrent memory of ActorCriticRecurrent (rsl_rl/rsl_rl/modules/actor_critic_recurrent.py: Memory = nn.LSTM / nn.GRU, sequence-first, torch's gate
 * order and formulas).  One time step of one layer is two matrix products on the kernels above (go2nn_linear_elu_forward_group, act 1, split images):
 *   gi = x W_ih^T + b_ih,  gh = h_prev W_hh^T + b_hh   [B, G H]  (G = 4: i, f, g, o;  G = 3: r, z, n — GRU keeps W_hn h + b_hn apart: n = tanh(gi_n + r (gh_n)))
 * and ONE cell launch (go2nn_rnn_cell_forward) that applies the non-linearities and the state update for every (row, hidden unit); in the update the input products
 * of all T steps are one GEMM up front.  The backward step (go2nn_rnn_cell_backward) turns the gradient at h_t (from the heads or the layer above, plus the carried
 * gradient of step t+1) into the gradients at gi and gh; dW_ih, dW_hh and the biases are then one weight-gradient GEMM / column sum each over all T B rows, and the
 * carried gradient of step t-1 is dgh W_hh (go2nn_linear_backward_input_group, plain).
 * Done handling (the fixed-shape form of the reference's split / pad / unpad, rsl_rl/rsl_rl/utils/utils.py:33-71): a row with done[r] set carries sub[r] into the
 * next step instead of its new state, and no gradient flows back through that carry.
 * Cell jobs: elementwise, 1..GO2NN_MAX_GROUP jobs (actor and critic memory) per launch, any B >= 1, 1 <= H <= GO2NN_MAX_WIDTH.  Outputs may alias the inputs they
 * replace element for element (h with h_prev, c with c_prev, dh_carry and dc in place). */
#define GO2NN_RNN_LSTM 0
#define GO2NN_RNN_GRU 1
typedef struct Go2nnRnnCellJob {
  const float *gi, *gh;          /* [B, G H] the two products of the step, biases included */
  const float *h_prev, *c_prev;  /* [B, H] the state the step starts from (c: LSTM only) */
  float *h, *c;                  /* [B, H] the new state (c: LSTM only) */
  float* gates;                  /* [B, 4 H] or NULL: what the backward step reads — LSTM: i, f, g, o after the non-linearity; GRU: r, z, n, gh_n */
  float *save_h, *save_c;        /* [B, H] or NULL: h_prev (c_prev) copied here first (the rollout storage slot of the step) */
  const uint8_t* done;           /* [B] or NULL: rows whose carry into the next step is sub_h (sub_c) instead of the new state */
  const float *sub_h, *sub_c;    /* [B, H] */
  float *next_h, *next_c;        /* [B, H] or NULL: the carry = done[r] ? sub[r] : new state (the update's recurrence) */
  int32_t B, H, type, pad_;
} Go2nnRnnCellJob;
typedef struct Go2nnRnnCellBwdJob {
  const float *gates, *c, *c_prev, *h_prev;   /* step t's saved gates, c_t and c_{t-1} (LSTM) / h_{t-1} (GRU), as the forward step left them */
  const float* dy;               /* [B, H] d loss / d h_t from outside the recurrence (the heads, or the layer above) */
  const float* dh_rec;           /* [B, H] or NULL (the last step): dgh_{t+1} W_hh, the gradient at the carry t -> t+1 through the next step's product */
  float* dh_carry;               /* GRU: [B, H] in: dh_{t+1} z_{t+1} (read when dh_rec is set), out: dh_t z_t.  LSTM: NULL */
  float* dc;                     /* LSTM: [B, H] in: dc carried from step t+1 (read when dh_rec is set), out: the carry for step t-1.  GRU: NULL */
  const uint8_t* done;           /* [B] or NULL: done[t] of the forward (rows whose carry t -> t+1 was replaced: dh_rec, dh_carry and dc are not added) */
  float *dgi, *dgh;              /* [B, G H] out: d loss / d gi, d gh (equal but for the GRU's n block: dgh_n = dgi_n r) */
  int32_t B, H, type, pad_;
} Go2nnRnnCellBwdJob;
int go2nn_rnn_cell_forward(const Go2nnRnnCellJob* jobs, int32_t njobs, void* stream);
int go2nn_rnn_cell_backward(const Go2nnRnnCellBwdJob* jobs, int32_t njobs, void* stream);
/* The reset of the rollout (actor_critic_recurrent.py Memory.reset: hidden_state[..., dones, :] = 0): rows r with done[r] != 0 of up to 4 state tensors [L, B, H]
 * set to 0, one launch, no host read of done (capturable). */
#define GO2NN_RNN_MAX_STATES 4
int go2nn_rnn_reset(float* const* states, int32_t nstates, int32_t L, int32_t B, int32_t H, const uint8_t* done, void* stream);

/* ---- the policy evaluator's metrics (go2_rl_gym_amd/utils/evaluator.py; the slot the reference fills with RoboGauge, rsl_rl/rsl_rl/runners/on_policy_runner.py:103-111,243-295).
 * ADDED WITHIN ABI 7: three new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * An evaluation is { policy, go2sim_step, go2nn_eval_accumulate } per env step and one go2nn_eval_reduce at the end; all three calls are plain launches (capturable).
 *
 * go2nn_eval_accumulate adds, per env e and step, to acc[m, e] (acc: fp32 [GO2NN_EVAL_NUM, N], metric-major, read-modify-written in place; one lane per env, no atomics):
 *   STEPS            1
 *   LIN_VEL_ERR      |cmd_xy - v_xy|_2                       v = base_lin_vel (base frame), cmd = commands
 *   ANG_VEL_ERR      |cmd_yaw - w_z|                         w = base_ang_vel, cmd_yaw = commands[2]
 *   SPEED_ALONG_CMD  v_xy . cmd_xy / |cmd_xy|                0 when |cmd_xy| < 1e-6
 *   TILT             sqrt(g_x^2 + g_y^2)                     g = projected_gravity
 *   POWER            sum_j |tau_j qd_j|                      tau = torques, qd = joint velocities (dof_state[..., 1])
 *   TORQUE_SQ        sum_j tau_j^2
 *   ACTION_RATE_SQ   sum_j (a_j - a_j^prev)^2                a = actions, a^prev = last_actions
 *   DOF_LIMIT_STEPS  1 if any joint position q_j < dof_limits[j][0] or > dof_limits[j][1]
 *   FALLS            1 if reset_buf and not time_out_buf
 * Every input is a Go2SimBuffers field described by (pointer, env stride, component stride) in ELEMENTS, so the same kernel reads the HIP simulator's field-major buffers
 * (go2sim_buffer_layout() == 1: env stride 1, component stride N — consecutive lanes read consecutive addresses) and row-major ones (layout 0: env stride = row length,
 * component stride 1).  dof_state [N,12,2]: comp_stride is the stride between JOINTS and dof_vel_offset the distance from a joint's position to its velocity (row-major:
 * 2 and 1; field-major: N and 12 N).  reset_buf / time_out_buf are uint8.  dof_limits: [12,2] floats in the buffers' memory space.  dt (the policy step) is carried for
 * the consumer that turns per-step sums into per-second figures; the accumulators are per-step sums and do not use it. */
enum {
  GO2NN_EVAL_STEPS = 0, GO2NN_EVAL_LIN_VEL_ERR, GO2NN_EVAL_ANG_VEL_ERR, GO2NN_EVAL_SPEED_ALONG_CMD, GO2NN_EVAL_TILT, GO2NN_EVAL_POWER, GO2NN_EVAL_TORQUE_SQ,
  GO2NN_EVAL_ACTION_RATE_SQ, GO2NN_EVAL_DOF_LIMIT_STEPS, GO2NN_EVAL_FALLS, GO2NN_EVAL_NUM
};
typedef struct Go2nnEvalField { const void* p; int32_t env_stride; int32_t comp_stride; } Go2nnEvalField;
typedef struct Go2nnEvalIn {
  Go2nnEvalField commands, base_lin_vel, base_ang_vel, projected_gravity, dof_state, torques, actions, last_actions, reset_buf, time_out_buf;
  const float* dof_limits;
  int32_t dof_vel_offset;
  float dt;
} Go2nnEvalIn;
int go2nn_eval_clear(float* acc, int32_t N, void* stream);          /* acc[GO2NN_EVAL_NUM, N] = 0 */
int go2nn_eval_accumulate(const Go2nnEvalIn* in, float* acc, int32_t N, void* stream);
/* out [G, GO2NN_EVAL_NUM + 2] (fp64): per group g the sums over the envs e with group[e] == g of the ten accumulators, then the number of such envs, then the number of them
 * with acc[FALLS, e] == 0.  Group ids outside [0, G) are ignored; an empty group gives a row of zeros.  Every sum is formed in an order that depends on (N, G) only — 256
 * strided fp64 partials, then a fixed tree; no floating-point atomics —, so equal inputs give bit-equal outputs.  1 <= G <= 65535. */
int go2nn_eval_reduce(const float* acc, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);

/* ---- the trajectory recorder (go2_rl_gym_amd/utils/recorder.py): per-step frames of chosen robots, kept on the device.
 * ADDED WITHIN ABI 7: two new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A FRAME is GO2NN_TRACE_WIDTH floats of one robot after one env step; every column is a plain copy of a simulator buffer (no arithmetic; the uint8 flags become 0.0 / 1.0).
 * This enum is the one specification of the frame: column offset of each block, the block's length being the distance to the next one.
 *   ROOT_POS 3, ROOT_QUAT 4 (xyzw), ROOT_LIN_VEL 3, ROOT_ANG_VEL 3 (world; root_states[0:13])     DOF_POS 12, DOF_VEL 12 (dof_state[..., 0 / 1])     TORQUES 12, ACTIONS 12
 *   COMMANDS 3 (vx, vy, yaw rate)     BASE_LIN_VEL 3, BASE_ANG_VEL 3, PROJECTED_GRAVITY 3 (base frame)
 *   FOOT_POS 4 x 3, FOOT_VEL 4 x 3 (world; rigid_body_states[foot_body[f], 0:3 / 7:10])     FOOT_FORCE 4 x 3 (world; contact_forces[foot_body[f]])
 *   REWARD 1 (rew_buf), RESET 1 (reset_buf), TIME_OUT 1 (time_out_buf) */
enum {
  GO2NN_TRACE_ROOT_POS = 0, GO2NN_TRACE_ROOT_QUAT = 3, GO2NN_TRACE_ROOT_LIN_VEL = 7, GO2NN_TRACE_ROOT_ANG_VEL = 10, GO2NN_TRACE_DOF_POS = 13, GO2NN_TRACE_DOF_VEL = 25,
  GO2NN_TRACE_TORQUES = 37, GO2NN_TRACE_ACTIONS = 49, GO2NN_TRACE_COMMANDS = 61, GO2NN_TRACE_BASE_LIN_VEL = 64, GO2NN_TRACE_BASE_ANG_VEL = 67,
  GO2NN_TRACE_PROJECTED_GRAVITY = 70, GO2NN_TRACE_FOOT_POS = 73, GO2NN_TRACE_FOOT_VEL = 85, GO2NN_TRACE_FOOT_FORCE = 97, GO2NN_TRACE_REWARD = 109, GO2NN_TRACE_RESET = 110,
  GO2NN_TRACE_TIME_OUT = 111, GO2NN_TRACE_WIDTH = 112
};
/* The sources, each as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's, so field-major and row-major buffers are read unchanged.  dof_state: as in
 * Go2nnEvalIn (comp_stride between joints, dof_vel_offset from a position to its velocity).  rigid_body_states [N, bodies, 13] and contact_forces [N, bodies, 3]: comp_stride
 * is the stride between the COMPONENTS of one body and *_body_stride the stride between bodies; foot_body names the four foot bodies.  rew_buf is fp32, reset_buf and
 * time_out_buf are uint8 (comp_stride unused, may be 0). */
typedef struct Go2nnTraceIn {
  Go2nnEvalField root_states, dof_state, torques, actions, commands, base_lin_vel, base_ang_vel, projected_gravity, rigid_body_states, contact_forces, rew_buf, reset_buf,
      time_out_buf;
  int32_t dof_vel_offset;
  int32_t rigid_body_stride;
  int32_t contact_body_stride;
  int32_t foot_body[4];
  int32_t pad_;
} Go2nnTraceIn;
/* frames: fp32 [T, K, GO2NN_TRACE_WIDTH] row-major, a ring of T steps;  env_ids: int32 [K], strictly increasing, each in [0, N) (the caller's duty: the kernel cannot check
 * it);  cursor: ONE int32 in the buffers' memory space = frames recorded since the last clear.  The call writes the frame of every tracked robot to slot (*cursor) % T and
 * then adds 1 to *cursor: the slot is read from the cursor by the kernel, never passed by the host, so a captured launch lands in a new slot on every replay.  Two plain
 * launches on `stream` (the frame kernel, one lane per output float; then one lane that advances the cursor), no atomics.  After c calls the ring holds the steps
 * max(0, c - T) .. c - 1, step s in slot s % T. */
int go2nn_trace_record(const Go2nnTraceIn* in, const int32_t* env_ids, int32_t K, float* frames, int32_t* cursor, int32_t T, void* stream);
int go2nn_trace_clear(int32_t* cursor, void* stream);          /* *cursor = 0; the frames are left as they are */

/* ---- the evaluator's perturbations: scheduled pushes, perturbed dynamics and what happens next (go2_rl_gym_amd/utils/evaluator.py, `evaluation.perturbations`).
 * ADDED WITHIN ABI 7: five new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A perturbed evaluation step is { policy, go2nn_robust_apply, go2sim_step, go2nn_eval_accumulate, go2nn_robust_accumulate }: two more plain launches per step
 * (capturable; one lane per env, no atomics), and one go2nn_robust_reduce at the end.  Every env e belongs to one perturbation pert_of_env[e] in [0, P), P <= 64;
 * an env with pert_of_env[e] outside [0, P) is left alone (only its step counter runs).
 * A perturbation is one Go2nnRobustSpec (an array of P of them in the buffers' memory space):
 *   dv[3]                  velocity impulse [m/s] in the robot's HEADING frame: x forward, y left, z up
 *   first, period, count   the push schedule in counted steps: a push fires at step s when s >= first, (s - first) % period == 0 and (s - first) / period < count;
 *                          count = 0: no pushes
 *   window W, hold H, thr  the recovery rule (below), W and H in steps, thr in m/s
 *   strength, kp_mul, kd_mul, added_mass, friction   the values written to the env's rows of motor_strengths, p_gains_multiplier, d_gains_multiplier (all 12 joints),
 *                          added_base_mass [kg] and friction_coeffs; only the rows named in `mask` are written.  Identity: 1, 1, 1, 0 and the simulator's own friction.
 *                          friction is the robot's SHAPE coefficient: the simulator's contact uses the mean of it and the terrain's (go2sim_impl.cpp lane_load_phys: ph.mu).
 *                          The simulator multiplies torques by motor_strengths only when it was created with randomize_motor_strength set.
 * The table: fp32 [GO2NN_ROBUST_NUM, N], row-major by row of the enum below, column e = env e.
 * go2nn_robust_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps: nothing is pushed while STEP < 0 when first >= 0).
 * go2nn_robust_apply (BEFORE go2sim_step), per env with a perturbation:
 *   the masked dynamics rows are rewritten (every step: idempotent, and a reset inside the step cannot erase them);
 *   if a push fires at s = STEP[e]:  root_states[e, 7:10] += (c dv_x - s dv_y, s dv_x + c dv_y, dv_z) with the heading (c, s) = (1 - 2 (y^2 + z^2), 2 (x y + w z)) of the root
 *   quaternion (x, y, z, w) = root_states[e, 3:7], normalised, (1, 0) if its norm is below 1e-6 (no trigonometric function is evaluated);
 *   OPEN = 1, PEAK_ERR = PEAK_TILT = OK_RUN = DONE = 0, PUSHES += 1.
 * go2nn_robust_accumulate (AFTER the step), per env: err = |cmd_xy - v_xy|_2 (as LIN_VEL_ERR above), tilt = |g_xy|_2, fall = reset_buf and not time_out_buf.
 *   With a perturbation and OPEN > 0 (a window is open, this being its OPEN-th step):
 *     if not DONE:  PEAK_ERR = max(PEAK_ERR, err), PEAK_TILT = max(PEAK_TILT, tilt);
 *                   fall:            PUSH_FALLS += 1, DONE = 1
 *                   else err < thr:  OK_RUN += 1; at OK_RUN == H:  RECOVERED += 1, RECOVERY_STEPS += OPEN, DONE = 1
 *                   else:            OK_RUN = 0
 *     OPEN == W:  PEAK_ERR_SUM += PEAK_ERR, PEAK_TILT_SUM += PEAK_TILT, OPEN = 0 (closed);  otherwise OPEN += 1
 *   Always: STEP += 1 — the step counter lives in the table, so a captured launch advances on every replay.
 * The scores are per PUSH: a robot that falls after its window has closed, or outside any window, counts in the evaluator's FALLS only. */
enum {
  GO2NN_ROBUST_STEP = 0, GO2NN_ROBUST_OPEN, GO2NN_ROBUST_PEAK_ERR, GO2NN_ROBUST_PEAK_TILT, GO2NN_ROBUST_OK_RUN, GO2NN_ROBUST_DONE,
  GO2NN_ROBUST_PUSHES, GO2NN_ROBUST_PUSH_FALLS, GO2NN_ROBUST_RECOVERED, GO2NN_ROBUST_RECOVERY_STEPS, GO2NN_ROBUST_PEAK_ERR_SUM, GO2NN_ROBUST_PEAK_TILT_SUM, GO2NN_ROBUST_NUM
};
#define GO2NN_ROBUST_ACC_FIRST GO2NN_ROBUST_PUSHES                          /* rows below it are per-env state, rows from it on are accumulators */
#define GO2NN_ROBUST_ACC_NUM (GO2NN_ROBUST_NUM - GO2NN_ROBUST_ACC_FIRST)
#define GO2NN_ROBUST_MAX_SPECS 64
#define GO2NN_ROBUST_MASK_STRENGTH 1
#define GO2NN_ROBUST_MASK_KP 2
#define GO2NN_ROBUST_MASK_KD 4
#define GO2NN_ROBUST_MASK_ADDED_MASS 8
#define GO2NN_ROBUST_MASK_FRICTION 16
typedef struct Go2nnRobustSpec {
  float dv[3];
  int32_t first, period, count;
  int32_t window, hold;
  float thr;
  float strength, kp_mul, kd_mul, added_mass, friction;
  int32_t mask;
  int32_t pad_;
} Go2nnRobustSpec;
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's.  root_states [N,13], commands, base_lin_vel, projected_gravity as above;
 * reset_buf / time_out_buf uint8; motor_strengths, p_gains_multiplier, d_gains_multiplier [N,12]; added_base_mass, friction_coeffs [N] (comp_stride unused).
 * The five dynamics buffers and root_states are WRITTEN by go2nn_robust_apply.  num_specs = P. */
typedef struct Go2nnRobustIn {
  Go2nnEvalField root_states, commands, base_lin_vel, projected_gravity, reset_buf, time_out_buf;
  Go2nnEvalField motor_strengths, p_gains_multiplier, d_gains_multiplier, added_base_mass, friction_coeffs;
  int32_t num_specs;
  int32_t pad_;
} Go2nnRobustIn;
/* Host-side check of P specs in HOST memory, before they are copied to the buffers' memory space (the launches cannot read them back): GO2NN_EINVAL with a message for
 * P outside [1, 64], a null pointer, hold < 1, first < 0, count < 0, and — where count > 0 — period < 1, window < 1 or window > period (windows never overlap). */
int go2nn_robust_check_specs(const Go2nnRobustSpec* host_specs, int32_t P);
int go2nn_robust_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, num_specs outside [1, 64], an env stride < 1 or (vector fields) a component stride < 1. */
int go2nn_robust_apply(const Go2nnRobustIn* in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int32_t N, void* stream);
int go2nn_robust_accumulate(const Go2nnRobustIn* in, const Go2nnRobustSpec* specs, const int32_t* pert_of_env, float* table, int32_t N, void* stream);
/* out [G, GO2NN_ROBUST_ACC_NUM + 1] (fp64): per group the sums of the accumulator rows over its envs, then the number of its envs — the summation scheme (and the device
 * function) of go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, group ids outside [0, G) ignored, an empty group gives zeros.  1 <= G <= 65535. */
int go2nn_robust_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);

/* ---- the evaluator's terrain-difficulty ladder: how far does a robot get from where it stood (go2_rl_gym_amd/utils/evaluator.py, `evaluation.ladder`).
 * ADDED WITHIN ABI 7: three new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A ladder evaluation step is { policy, go2sim_step, go2nn_eval_accumulate, go2nn_ladder_accumulate }: one more plain launch per step (capturable; one lane per env, no
 * atomics), and one go2nn_ladder_reduce at the end.  The record of a robot survives the simulator's reset of a fallen robot: it is latched in the table.
 * The table: fp32 [GO2NN_LADDER_NUM, N], row-major by row of the first enum below, column e = env e.
 * go2nn_ladder_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).
 * go2nn_ladder_accumulate (AFTER the step), per env, with s = STEP[e], in this order:
 *   1. s < 0:   nothing but step 4 (a fall before the first counted step leaves no trace);
 *   2. s == 0:  X0, Y0 = root_states[e, 0:2] (bit copies), MAX_D2 = 0, STATE = RUNNING;
 *   3. STATE == RUNNING:  reset_buf and not time_out_buf:  STATE = FELL;     reset_buf and time_out_buf:  STATE = TIMED_OUT;
 *                         otherwise d2 = (x - X0)^2 + (y - Y0)^2,  MAX_D2 = max(MAX_D2, d2),  and if d2 > dist2_thr:  STATE = CLEARED, CLEAR_STEP = s + 1;
 *   4. STEP = s + 1.
 * On a reset root_states already holds the post-reset pose, so the flags are looked at BEFORE the position (a step with a reset never contributes a distance).  A latched
 * state (CLEARED, FELL, TIMED_OUT) is never left: a robot that clears and falls afterwards stays CLEARED, and only the first fall or time-out is seen.  Distances are compared
 * squared; no square root is taken per step.  CLEAR_STEP is the number of counted steps the robot took to clear (1 = at the first counted step's end).
 * go2nn_ladder_reduce: out [G, GO2NN_LADDER_OUT_NUM] (fp64), per group the columns of the second enum: its envs, those CLEARED / FELL / TIMED_OUT, the sum of CLEAR_STEP
 * over the CLEARED ones, and the sum of progress = min(sqrt(MAX_D2 / dist2_thr), 1) (fp64) over all of them — the summation scheme (and the device function) of
 * go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, group ids outside [0, G) ignored, an empty group gives zeros.  It takes dist2_thr as an argument (the
 * table does not hold it): pass the value go2nn_ladder_accumulate ran with. */
enum { GO2NN_LADDER_STEP = 0, GO2NN_LADDER_STATE, GO2NN_LADDER_X0, GO2NN_LADDER_Y0, GO2NN_LADDER_MAX_D2, GO2NN_LADDER_CLEAR_STEP, GO2NN_LADDER_NUM };
enum { GO2NN_LADDER_OUT_N = 0, GO2NN_LADDER_OUT_CLEARED, GO2NN_LADDER_OUT_FELL, GO2NN_LADDER_OUT_TIMED_OUT, GO2NN_LADDER_OUT_CLEAR_STEPS, GO2NN_LADDER_OUT_PROGRESS, GO2NN_LADDER_OUT_NUM };
enum { GO2NN_LADDER_RUNNING = 0, GO2NN_LADDER_CLEARED = 1, GO2NN_LADDER_FELL = 2, GO2NN_LADDER_TIMED_OUT = 3 };          /* the values of the STATE row */
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's: root_states [N,13] (only columns 0 and 1 are read), reset_buf / time_out_buf uint8
 * (comp_stride unused, may be 0).  dist2_thr: the SQUARED clearing distance [m^2], > 0.  Nothing but the table is written. */
typedef struct Go2nnLadderIn {
  Go2nnEvalField root_states, reset_buf, time_out_buf;
  float dist2_thr;
  int32_t pad_;
} Go2nnLadderIn;
int go2nn_ladder_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, an env stride < 1, a component stride of root_states < 1, dist2_thr <= 0 (or NaN). */
int go2nn_ladder_accumulate(const Go2nnLadderIn* in, float* table, int32_t N, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, G outside 1 .. 65535, dist2_thr <= 0 (or NaN). */
int go2nn_ladder_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, float dist2_thr, double* out, void* stream);

/* ---- the evaluator's scripted command maneuvers: start, brake, reverse, turn — and how the robot answers (go2_rl_gym_amd/utils/evaluator.py, `evaluation.maneuvers`).
 * ADDED WITHIN ABI 7: five new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A maneuver evaluation step is { policy, go2nn_maneuver_apply, go2sim_step, go2nn_maneuver_accumulate, go2nn_eval_accumulate }: two more plain launches per step
 * (capturable; one lane per env, no atomics), and one go2nn_maneuver_reduce at the end.  Every env e belongs to one maneuver man_of_env[e] in [0, M), M <= 64; an env with
 * man_of_env[e] outside [0, M) is left alone (only its step counter runs).
 * A maneuver is one Go2nnManeuverSpec (an array of M of them in the buffers' memory space):
 *   count                  1 .. GO2NN_MANEUVER_MAX_SEGS segments
 *   start[k], cmd[k][3]    segment k begins at counted step start[k] (start[0] = 0, strictly increasing) and commands (vx, vy, yaw rate)
 *   window W, hold H       the settling rule (below), in steps;  thr_lin [m/s], thr_ang [rad/s] its thresholds
 * The command in force at step s is a pure function c_m(s): that of the segment with the largest start <= max(s, 0) — segment 0 also covers the warm-up.  A SWITCH is the
 * start of a segment k >= 1.
 * THE CONVENTION: the switch at counted step s takes effect in the go2nn_maneuver_apply BEFORE that step's go2sim_step.  The step's physics runs on an action chosen from an
 * observation that still carries the old command; the observation it produces, and the metrics of step s, carry the new one.  This is the simulator's own resampling order
 * (_post_physics_step_callback runs before the rewards and the observations).
 * The table: fp32 [GO2NN_MANEUVER_NUM, N], row-major by row of the enum below, column e = env e.
 * go2nn_maneuver_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).
 * go2nn_maneuver_apply (BEFORE go2sim_step), per env with a maneuver: commands[e, 0:3] = c_m(STEP[e]), commands[e, 3:num_commands] = 0.  Nothing else is written (the table
 *   is const here); calling it twice is calling it once.
 * go2nn_maneuver_accumulate (AFTER the step, before go2nn_eval_accumulate), per env with a maneuver, with s = STEP[e], in this order:
 *   1. commands[e] = c_m(s) as above (a robot that fell was reset inside the step and drew a command: go2nn_eval_accumulate and the recorder see the maneuver's);
 *   2. s == start[k] for a k >= 1:  OPEN = 1, OK_RUN = IS_SETTLED = IS_FELL = PEAK_TILT = 0, SWITCHES += 1;
 *   3. OPEN > 0 (a window is open, this being its OPEN-th step):  err_lin = |cmd_xy - v_xy|_2, err_ang = |cmd_yaw - w_z|, tilt = |g_xy|_2 (as LIN_VEL_ERR, ANG_VEL_ERR and
 *      TILT above), fall = reset_buf and not time_out_buf.  The flags come first: on a reset the buffers already hold the post-reset state.
 *        not IS_FELL and fall:     SWITCH_FALLS += 1, IS_FELL = 1
 *        not IS_FELL and no fall:  WIN_STEPS += 1, WIN_LIN_ERR += err_lin, WIN_ANG_ERR += err_ang, PEAK_TILT = max(PEAK_TILT, tilt);
 *                                  not IS_SETTLED and err_lin < thr_lin and err_ang < thr_ang:  OK_RUN += 1; at OK_RUN == H:  SETTLED += 1, SETTLE_STEPS += OPEN, IS_SETTLED = 1
 *                                  not IS_SETTLED otherwise:                                    OK_RUN = 0
 *        OPEN == W:  PEAK_TILT_SUM += PEAK_TILT, OPEN = 0 (closed);  otherwise OPEN += 1
 *   4. STEP = s + 1 (every env) — the step counter lives in the table, so a captured launch advances on every replay.
 * The scores are per SWITCH: SETTLE_STEPS counts from the switch to the END of the hold; a robot that falls after its window has closed, or outside any window, counts
 * in the evaluator's FALLS only; a robot that settles and falls later inside the same window counts in SETTLED and in SWITCH_FALLS. */
enum {
  GO2NN_MANEUVER_STEP = 0, GO2NN_MANEUVER_OPEN, GO2NN_MANEUVER_OK_RUN, GO2NN_MANEUVER_IS_SETTLED, GO2NN_MANEUVER_IS_FELL, GO2NN_MANEUVER_PEAK_TILT,
  GO2NN_MANEUVER_SWITCHES, GO2NN_MANEUVER_SWITCH_FALLS, GO2NN_MANEUVER_SETTLED, GO2NN_MANEUVER_SETTLE_STEPS, GO2NN_MANEUVER_WIN_STEPS, GO2NN_MANEUVER_WIN_LIN_ERR,
  GO2NN_MANEUVER_WIN_ANG_ERR, GO2NN_MANEUVER_PEAK_TILT_SUM, GO2NN_MANEUVER_NUM
};
#define GO2NN_MANEUVER_ACC_FIRST GO2NN_MANEUVER_SWITCHES                    /* rows below it are per-env state, rows from it on are accumulators */
#define GO2NN_MANEUVER_ACC_NUM (GO2NN_MANEUVER_NUM - GO2NN_MANEUVER_ACC_FIRST)
#define GO2NN_MANEUVER_MAX_SPECS 64
#define GO2NN_MANEUVER_MAX_SEGS 8
typedef struct Go2nnManeuverSpec {
  int32_t count;
  int32_t window, hold;
  float thr_lin, thr_ang;
  int32_t start[GO2NN_MANEUVER_MAX_SEGS];
  float cmd[GO2NN_MANEUVER_MAX_SEGS][3];
} Go2nnManeuverSpec;
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's.  commands [N, num_commands] (WRITTEN by both calls; num_commands >= 3),
 * base_lin_vel, base_ang_vel, projected_gravity [N,3]; reset_buf / time_out_buf uint8 (comp_stride unused, may be 0).  num_specs = M. */
typedef struct Go2nnManeuverIn {
  Go2nnEvalField commands, base_lin_vel, base_ang_vel, projected_gravity, reset_buf, time_out_buf;
  int32_t num_specs;
  int32_t num_commands;
} Go2nnManeuverIn;
/* Host-side check of M specs in HOST memory, before they are copied to the buffers' memory space (the launches cannot read them back): GO2NN_EINVAL with a message for
 * M outside [1, 64], a null pointer, count outside [1, 8], start[0] != 0, starts not strictly increasing, hold < 1, window < hold, a window longer than the gap between
 * two switches (windows never overlap), a threshold <= 0 (or NaN). */
int go2nn_maneuver_check_specs(const Go2nnManeuverSpec* host_specs, int32_t M);
int go2nn_maneuver_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, num_specs outside [1, 64], num_commands < 3, an env stride < 1 or (vector fields) a component stride < 1. */
int go2nn_maneuver_apply(const Go2nnManeuverIn* in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, const float* table, int32_t N, void* stream);
int go2nn_maneuver_accumulate(const Go2nnManeuverIn* in, const Go2nnManeuverSpec* specs, const int32_t* man_of_env, float* table, int32_t N, void* stream);
/* out [G, GO2NN_MANEUVER_ACC_NUM + 1] (fp64): per group the sums of the accumulator rows over its envs, then the number of its envs — the summation scheme (and the device
 * function) of go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, group ids outside [0, G) ignored, an empty group gives zeros.  1 <= G <= 65535. */
int go2nn_maneuver_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);

/* ---- the evaluator's sensor model: what the policy SEES — noise, bias, latency, dropped frames (go2_rl_gym_amd/utils/evaluator.py, `evaluation.sensors`).
 * ADDED WITHIN ABI 7: four new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A sensor evaluation step is { policy(delivered), go2sim_step, go2nn_sensor_apply(obs_buf -> delivered), go2nn_eval_accumulate }: two more plain launches per step
 * (capturable; one lane per observation float, no atomics), no reduce of its own.  The metrics still read the simulator's true state.  Every env e belongs to one condition
 * sensor_of_env[e] in [0, P), P <= 64; an env with sensor_of_env[e] outside [0, P) gets its observation's bits unchanged.
 * A condition is one Go2nnSensorSpec (an array of P of them in the buffers' memory space):
 *   noise_mul                multiple of the task's own observation noise (1 = what the task trains with)
 *   gyro_bias, gravity_bias, joint_offset   half-width of the constant per-(env, column) offset of the gyro / gravity / joint-position columns, in OBSERVATION units (the
 *                            caller folds the observation scales in: rad/s x obs_scales.ang_vel, rad x obs_scales.dof_pos)
 *   delay                    age of the proprioceptive columns in policy steps, 0 .. GO2NN_SENSOR_MAX_DELAY
 *   drop                     probability in [0, 1) that a whole frame is lost: the proprioceptive columns then repeat what was delivered last
 * The layout (Go2nnSensorIn): D <= GO2NN_SENSOR_MAX_WIDTH columns; scale[D], the task's noise vector at noise_level 1; kind[D], one of the enum below — PASS columns
 * (commands, previous actions) are never delayed, dropped or biased; clip, the observation clip; seed.
 * The state: ONE allocation of go2nn_sensor_state_bytes(N, D) bytes in the buffers' memory space: an int32 cursor (steps since go2nn_sensor_begin) in the first 256 bytes,
 * a ring [R][N][D] of clean observations, R = GO2NN_SENSOR_MAX_DELAY + 1, and held [N][D], the frame last delivered.
 * go2nn_sensor_apply, per (env e, column c), with s = the cursor, x = obs[e, c], fresh = (s == 0 or dones[e]):
 *   1. ring[s % R][e][c] = x; if fresh, every slot of the ring = x (a robot that was just reset never sees its pre-fall past);
 *   2. src = x for a PASS column, otherwise ring[(s - delay) % R][e][c];
 *   3. the frame is DROPPED when drop > 0, not fresh, and u(seed, DROP; e, 0, s) < drop — one draw per env and step —: every column that is not PASS delivers held[e][c];
 *   4. otherwise, with b = (2 u(seed, BIAS; e, c, 0) - 1) mag  (mag: gyro_bias / gravity_bias / joint_offset by the column's kind, 0 for the others; one draw per (e, c) for
 *      the whole evaluation) and k = fl(scale[c] noise_mul) (one rounded fp32 product):
 *        mag == 0 and k == 0:  out = src, the BITS (no add, no clamp: an all-zero spec is the identity, and a delay alone delivers old bits)
 *        otherwise:            out = clamp(src + b + (2 u(seed, NOISE; e, c, s) - 1) k, -clip, clip)
 *   5. held[e][c] = out, and out goes to the output buffer [N, D] (row-major; it must not be the input).
 * Then the cursor is advanced by a second, one-lane launch on the same stream: the step is read from device memory, so a captured pair advances on every replay.
 * The uniforms: u = (x >> 8) 2^-24 with x = word 0 of Philox4x32-10 under key (seed, tag) — tag 1 NOISE, 2 BIAS, 3 DROP — and counter (env, column, step, 0). */
enum { GO2NN_SENSOR_PASS = 0, GO2NN_SENSOR_GYRO, GO2NN_SENSOR_GRAVITY, GO2NN_SENSOR_JOINT_POS, GO2NN_SENSOR_JOINT_VEL };          /* the values of kind[] */
#define GO2NN_SENSOR_MAX_DELAY 4                                            /* policy steps: 80 ms at 50 Hz */
#define GO2NN_SENSOR_MAX_WIDTH 64
#define GO2NN_SENSOR_MAX_SPECS 64
typedef struct Go2nnSensorSpec {
  float noise_mul, gyro_bias, gravity_bias, joint_offset;
  int32_t delay;
  float drop;
  int32_t pad_[2];
} Go2nnSensorSpec;
/* obs: the clean observation as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's fields (row-major [N, D]: D and 1);  dones: uint8 [N];
 * scale: fp32 [D], kind: int32 [D], both in the buffers' memory space;  num_specs = P. */
typedef struct Go2nnSensorIn {
  Go2nnEvalField obs;
  const uint8_t* dones;
  const float* scale;
  const int32_t* kind;
  int32_t D;
  int32_t num_specs;
  float clip;
  uint32_t seed;
} Go2nnSensorIn;
/* Host-side check of P specs and the layout in HOST memory, before they are copied to the buffers' memory space: GO2NN_EINVAL with a message for a null pointer, P outside
 * [1, 64], D outside [1, 64], kind[c] outside 0 .. 4, scale[c] negative or not finite, delay outside [0, GO2NN_SENSOR_MAX_DELAY], drop outside [0, 1) (or NaN), a
 * magnitude (noise_mul, gyro_bias, gravity_bias, joint_offset) negative or not finite. */
int go2nn_sensor_check_specs(const Go2nnSensorSpec* host_specs, int32_t P, const int32_t* host_kind, const float* host_scale, int32_t D);
int64_t go2nn_sensor_state_bytes(int32_t N, int32_t D);          /* 0 for N < 1 or D outside [1, 64] */
int go2nn_sensor_begin(void* state, void* stream);               /* cursor = 0; ring and held are left as they are (step 0 fills them) */
/* GO2NN_EINVAL for null pointers, N < 1, D or num_specs outside [1, 64], a stride < 1, clip <= 0 (or NaN). */
int go2nn_sensor_apply(const Go2nnSensorIn* in, const Go2nnSensorSpec* specs, const int32_t* sensor_of_env, void* state, float* out, int32_t N, void* stream);

/* ---- TRAINING under randomised sensors: latency, dropped frames and constant offsets redrawn per robot and per EPISODE (domain_rand.randomize_sensors,
 * go2_rl_gym_amd/envs/base/legged_robot.py; csrc/go2nn_sensor_rand.h).
 * ADDED WITHIN ABI 7: four new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A training step is { policy(delivered), go2sim_step, go2nn_sensor_rand_apply(obs_buf -> the next storage row) }: two plain launches per step, capturable, one lane per
 * observation float, no atomics.  The privileged observation is not touched.  No white noise is added: the simulator's own noise.add_noise does that.
 * The layout is a Go2nnSensorIn, of which `scale` and `num_specs` are NOT read (scale may be NULL).  The ranges are one Go2nnSensorRand, passed to the kernel by value:
 *   delay_lo, delay_hi       the episode's latency of the proprioceptive columns in policy steps, an integer of [delay_lo, delay_hi] (inclusive)
 *   drop_lo, drop_hi         the episode's probability that a whole frame is lost, uniform in [drop_lo, drop_hi)
 *   gyro_bias, gravity_bias, joint_offset   half-width of the episode's constant per-(env, column) offset, in OBSERVATION units (as in Go2nnSensorSpec)
 *   env_offset               the global id of env 0 of this rank: ranks draw different conditions, and a robot's draws do not depend on how the envs are split
 * The state: ONE allocation of go2nn_sensor_rand_state_bytes(N, D) bytes in the buffers' memory space: the int32 cursor (steps since go2nn_sensor_rand_begin) in the first
 * 256 bytes, the ring [R][N][D] of the simulator's frames, R = GO2NN_SENSOR_MAX_DELAY + 1, held [N][D], the frame last delivered, and start [N][D] (int32), the cursor value
 * at which the lane's episode began.  Nothing of it is read before step 0 has written it.
 * go2nn_sensor_rand_apply, per (env e, column c), with s = the cursor, g = env_offset + e, x = obs[e, c]:
 *   1. fresh = (s == 0 or dones[e] or (also_fresh and also_fresh[e])).  If fresh: every ring slot of the lane = x and start = s; otherwise ring[s % R] = x.  s0 = start.
 *   2. a PASS column: out = held = x, the BITS.
 *   3. the episode's draws, (u_d, u_p) = words (0, 1) under key (seed, 4), counter (g, 0, s0, 0):
 *        delay = delay_lo + min((int)(u_d (delay_hi - delay_lo + 1)), delay_hi - delay_lo)     (one fp32 product, truncated)
 *        p     = drop_lo + u_p (drop_hi - drop_lo)                                             (fp32)
 *   4. the frame is LOST when not fresh, p > 0 and u < p with u = word 0 under key (seed, 6), counter (g, 0, s, 0): out = held, and held stays as it is.
 *   5. src = x if fresh or delay == 0, otherwise ring[(s - delay) % R]: the refill at a reset makes this the frame of step max(s - delay, s0).
 *   6. mag = gyro_bias / gravity_bias / joint_offset by the column's kind, 0 for joint velocities:
 *        mag == 0:   out = held = src, the BITS (no add, no clamp)
 *        otherwise:  out = held = clamp(src + (2 u - 1) mag, -clip, clip) with u = word 0 under key (seed, 5), counter (g, c, s0, 0)
 * `out` [N, D] is row-major and must not be the input.  Then the cursor is advanced by a second, one-lane launch on the same stream, so a captured pair advances on every
 * replay.  The uniforms: u = (x >> 8) 2^-24 with x a word of Philox4x32-10; tags 4 .. 6 keep these streams apart from the evaluator's 1 .. 3. */
typedef struct Go2nnSensorRand {
  int32_t delay_lo, delay_hi;          /* policy steps, inclusive */
  float drop_lo, drop_hi;              /* per-episode drop probability */
  float gyro_bias, gravity_bias, joint_offset;
  uint32_t env_offset;                 /* global id of env 0 on this rank */
} Go2nnSensorRand;
/* Host-side check of the ranges and the layout in HOST memory: GO2NN_EINVAL with a message naming the field for a null pointer, D outside [1, 64], kind[c] outside 0 .. 4,
 * anything but 0 <= delay_lo <= delay_hi <= GO2NN_SENSOR_MAX_DELAY and 0 <= drop_lo <= drop_hi < 1, a magnitude (gyro_bias, gravity_bias, joint_offset) negative or not finite. */
int go2nn_sensor_rand_check(const Go2nnSensorRand* host_r, const int32_t* host_kind, int32_t D);
int64_t go2nn_sensor_rand_state_bytes(int32_t N, int32_t D);          /* 0 for N < 1 or D outside [1, 64] */
int go2nn_sensor_rand_begin(void* state, void* stream);               /* cursor = 0; ring, held and start are left as they are (step 0 fills them) */
/* also_fresh: uint8 [N] in the buffers' memory space or NULL — envs that were reset from outside a step since the last call.  r is read on the host (a HOST pointer) and
 * passed by value.  GO2NN_EINVAL for null pointers (also_fresh aside), N < 1, D outside [1, 64], a stride < 1, clip <= 0 (or NaN), N * D too large, ranges the check refuses. */
int go2nn_sensor_rand_apply(const Go2nnSensorIn* in, const Go2nnSensorRand* r, const uint8_t* also_fresh, void* state, float* out, int32_t N, void* stream);

/* ---- the evaluator's gait scores: how does every evaluated robot walk (go2_rl_gym_amd/utils/evaluator.py, `evaluation.gait`; csrc/go2nn_gait.h).
 * ADDED WITHIN ABI 7: three new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A gait evaluation step is { ..., go2sim_step, go2nn_eval_accumulate, go2nn_gait_accumulate }: one more plain launch per step (capturable; one lane per env, the four
 * feet unrolled inside the lane, no atomics), and one go2nn_gait_reduce at the end.  The per-foot rule is that of utils/recorder.py gait_summary, kept in step with it.
 * The table: fp32 [GO2NN_GAIT_NUM, N], row-major by row, column e = env e: the per-env rows of the first enum below, then GO2NN_GAIT_FOOT_ROWS rows per foot f (row
 * GO2NN_GAIT_FOOT0 + f * GO2NN_GAIT_FOOT_ROWS + the second enum), f in foot_body order.  Counts and step sums are whole numbers held in fp32 (exact below 2^24).
 * go2nn_gait_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).  An all-zero foot state is "no frame of this segment seen yet".
 * go2nn_gait_accumulate (AFTER the step), per env, with s = STEP[e]:
 *   s < 0:  nothing but STEP = s + 1 (contacts of the warm-up leave no trace; the first counted step opens a segment).
 *   reset_buf set:  the frame is not used and ENDS THE SEGMENT: PREV, PHASE_START, LAST_TD = 0 for every foot.  STEP = s + 1.
 *   otherwise the frame is used:  USED += 1;  a foot is in CONTACT when contact_forces[foot, z] > contact_threshold (strictly); z = rigid_body_states[foot, 2] (world),
 *   speed = sqrt(vx^2 + vy^2) of rigid_body_states[foot, 7:9].  Per foot, with PREV in { 0 none, 1 swing, 2 contact }:
 *     contact:  CONTACT += 1, SLIP_SUM += speed.
 *     PREV == none:               the phase that opens a segment has no seen start: PHASE_START = 0;  swing: SWING_MAX = z;  contact: LIFT_Z = z.
 *     swing -> contact (TOUCHDOWN):  TOUCHDOWNS += 1;  if LAST_TD: STRIDE_STEPS += s + 1 - LAST_TD, STRIDES += 1;  LAST_TD = s + 1;
 *                                 if PHASE_START (the swing's lift-off was seen): SWING_STEPS += s + 1 - PHASE_START, SWINGS += 1, HEIGHT_SUM += SWING_MAX,
 *                                 CLEARANCE_SUM += SWING_MAX - LIFT_Z;  PHASE_START = s + 1, LIFT_Z = z.
 *     contact -> swing (LIFT-OFF):   if PHASE_START (the stance's touchdown was seen): STANCE_STEPS += s + 1 - PHASE_START, STANCES += 1;  PHASE_START = s + 1, SWING_MAX = z.
 *     contact -> contact:  LIFT_Z = z (the foot's height on the last contact frame before a swing).     swing -> swing:  SWING_MAX = max(SWING_MAX, z).
 *     PREV = contact ? 2 : 1.
 *   So a contact run that opens a segment is no touchdown, a stance or a swing counts only when both of its ends were seen inside the segment, and strides are the step
 *   differences between consecutive touchdowns of one segment.  PHASE_START and LAST_TD hold step + 1 (0 = none).  HEIGHT_SUM is in world z, which means nothing on
 *   stairs; CLEARANCE_SUM — the rise above the lift-off point — does.
 *   Per env, with k = the number of feet in contact: SUPPORT<k> += 1;  DIAGONAL += 1 when the feet in contact are exactly one of the two pairs diagonal_mask[0..1]
 *   (bit f = foot f of foot_body; the host resolves FL+RR and FR+RL from the foot names — the kernel assumes no order).  STEP = s + 1.
 * go2nn_gait_reduce: out [G, GO2NN_GAIT_OUT_NUM] (fp64), per group: its envs, then per foot the twelve columns of the third enum (USED is the env's, repeated per foot),
 * then SUPPORT0 .. SUPPORT4 and DIAGONAL — the summation scheme (and the device function) of go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, group ids
 * outside [0, G) ignored, an empty group gives zeros. */
enum { GO2NN_GAIT_STEP = 0, GO2NN_GAIT_USED, GO2NN_GAIT_SUPPORT0, GO2NN_GAIT_SUPPORT1, GO2NN_GAIT_SUPPORT2, GO2NN_GAIT_SUPPORT3, GO2NN_GAIT_SUPPORT4, GO2NN_GAIT_DIAGONAL, GO2NN_GAIT_FOOT0 };
enum {
  GO2NN_GAIT_F_PREV = 0, GO2NN_GAIT_F_PHASE_START, GO2NN_GAIT_F_LAST_TD, GO2NN_GAIT_F_SWING_MAX, GO2NN_GAIT_F_LIFT_Z, GO2NN_GAIT_F_CONTACT, GO2NN_GAIT_F_SLIP_SUM,
  GO2NN_GAIT_F_TOUCHDOWNS, GO2NN_GAIT_F_STRIDE_STEPS, GO2NN_GAIT_F_STRIDES, GO2NN_GAIT_F_STANCE_STEPS, GO2NN_GAIT_F_STANCES, GO2NN_GAIT_F_SWING_STEPS, GO2NN_GAIT_F_SWINGS,
  GO2NN_GAIT_F_HEIGHT_SUM, GO2NN_GAIT_F_CLEARANCE_SUM, GO2NN_GAIT_FOOT_ROWS
};
#define GO2NN_GAIT_F_ACC_FIRST GO2NN_GAIT_F_CONTACT                         /* foot rows below it are state, rows from it on are accumulators */
#define GO2NN_GAIT_NUM (GO2NN_GAIT_FOOT0 + 4 * GO2NN_GAIT_FOOT_ROWS)
enum {
  GO2NN_GAIT_O_USED = 0, GO2NN_GAIT_O_CONTACT, GO2NN_GAIT_O_SLIP_SUM, GO2NN_GAIT_O_TOUCHDOWNS, GO2NN_GAIT_O_STRIDE_STEPS, GO2NN_GAIT_O_STRIDES, GO2NN_GAIT_O_STANCE_STEPS,
  GO2NN_GAIT_O_STANCES, GO2NN_GAIT_O_SWING_STEPS, GO2NN_GAIT_O_SWINGS, GO2NN_GAIT_O_HEIGHT_SUM, GO2NN_GAIT_O_CLEARANCE_SUM, GO2NN_GAIT_OUT_FOOT_COLS
};
#define GO2NN_GAIT_OUT_N 0
#define GO2NN_GAIT_OUT_FOOT0 1
#define GO2NN_GAIT_OUT_SUPPORT0 (GO2NN_GAIT_OUT_FOOT0 + 4 * GO2NN_GAIT_OUT_FOOT_COLS)
#define GO2NN_GAIT_OUT_DIAGONAL (GO2NN_GAIT_OUT_SUPPORT0 + 5)
#define GO2NN_GAIT_OUT_NUM (GO2NN_GAIT_OUT_DIAGONAL + 1)
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnTraceIn's: rigid_body_states [N, bodies, 13] and contact_forces [N, bodies, 3] with
 * comp_stride between the components of one body and *_body_stride between bodies; foot_body names the four foot bodies; reset_buf uint8 (comp_stride unused, may be 0).
 * contact_threshold in newtons: finite and >= 0 (the evaluator's default 1.0 is the reference's `> 1 N` rule, legged_robot.py _reward_feet_air_time).  diagonal_mask: two disjoint
 * masks of two feet each.  Nothing but the table is written. */
typedef struct Go2nnGaitIn {
  Go2nnEvalField rigid_body_states, contact_forces, reset_buf;
  int32_t rigid_body_stride;
  int32_t contact_body_stride;
  int32_t foot_body[4];
  float contact_threshold;
  int32_t diagonal_mask[2];
  int32_t pad_;
} Go2nnGaitIn;
int go2nn_gait_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, an env stride < 1, a component stride (vector fields) or a body stride < 1, foot_body < 0, a contact_threshold that is negative
 * or not finite, diagonal masks that are not two disjoint pairs of the four feet. */
int go2nn_gait_accumulate(const Go2nnGaitIn* in, float* table, int32_t N, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, G outside 1 .. 65535. */
int go2nn_gait_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);

/* ---- the evaluator's black box: the last T frames before every robot's FIRST COUNTED FALL (go2_rl_gym_amd/utils/recorder.py FallRecorder, `evaluation.blackbox`;
 * csrc/go2nn_blackbox.h).
 * ADDED WITHIN ABI 7: two new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A frame is the trajectory recorder's (GO2NN_TRACE_*, Go2nnTraceIn above, unchanged): the state AFTER the env step.
 * frames: fp32 [N, T, GO2NN_TRACE_WIDTH] row-major, ROBOT-major: robot e's ring of T slots is contiguous.
 * state:  int32 [GO2NN_BLACKBOX_NUM * N + 1]: the rows of the enum below, row-major by row (row r of robot e at r * N + e), then ONE step counter at
 *         GO2NN_BLACKBOX_NUM * N (GO2NN_BLACKBOX_STATE_INTS(N) ints in all).
 * go2nn_blackbox_begin: every robot WRITTEN = 0, FROZEN = 0, FALL_STEP = -1; the step counter = first_step (the evaluator passes -warmup_steps; steps < 0 are not counted).
 * go2nn_blackbox_record (AFTER the env step), per robot, with s = the step counter before the call:
 *   FROZEN:  the robot is skipped; nothing of its ring or of its state rows changes until the next begin.
 *   otherwise its frame goes to slot WRITTEN % T of its ring, and then
 *     reset_buf && !time_out_buf (a FALL, go2nn_eval_accumulate's rule) and s >= 0:  WRITTEN += 1, FROZEN = 1, FALL_STEP = s.  The ring's newest frame is the fall step's own
 *       frame — the post-reset pose with the reset flag set, the recorder's convention —; the frames before it are the fall.
 *     reset_buf otherwise (a time-out; a fall of the warm-up):  WRITTEN = 0: the ring starts again with the next step, nothing is followed across a reset.
 *     no reset:  WRITTEN += 1.
 *   The step counter becomes s + 1.
 * So a frozen robot's ring holds its last min(WRITTEN, T) frames, the oldest in slot (WRITTEN - min(WRITTEN, T)) % T, the fall frame in slot (WRITTEN - 1) % T; only a
 * robot's first counted fall is kept.  Two plain launches on `stream` (the frame kernel, one lane per output float, which also advances the step counter it does not read;
 * then one lane per robot that updates the robot's state rows from the counter), no atomics, no host argument that changes per step: a captured pair replays correctly.
 * GO2NN_EINVAL for null pointers, N < 1, T < 1, N * GO2NN_TRACE_WIDTH >= 2^31, a bad Go2nnTraceIn (as go2nn_trace_record); a refused call writes nothing. */
enum { GO2NN_BLACKBOX_WRITTEN = 0, GO2NN_BLACKBOX_FROZEN, GO2NN_BLACKBOX_FALL_STEP, GO2NN_BLACKBOX_NUM };
#define GO2NN_BLACKBOX_STATE_INTS(N) (GO2NN_BLACKBOX_NUM * (long long)(N) + 1)
int go2nn_blackbox_begin(int32_t* state, int32_t N, int32_t first_step, void* stream);
int go2nn_blackbox_record(const Go2nnTraceIn* in, int32_t N, float* frames, int32_t* state, int32_t T, void* stream);

/* ---- the PPO update's left-right symmetry augmentation: every mini-batch followed by its mirror image (go2_rl_gym_amd/rsl_rl/algorithms/ppo.py, `algorithm.symmetry`;
 * the tables: go2_rl_gym_amd/utils/symmetry.py; csrc/go2nn_mirror.h).
 * ADDED WITHIN ABI 7: two new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * One plain launch per update (capturable), after the rollout's permutation, for up to GO2NN_MIRROR_MAX_JOBS tensors: the job index sits in the grid, one lane per source
 * element, no LDS, no atomics.  Per job: src fp32 [chunks * chunk_rows, width] row-major; dst fp32 [chunks, 2, chunk_rows, width] row-major, not overlapping src:
 *   dst[c, 0, r, :] = src[c * chunk_rows + r, :]                                  (the BITS)
 *   dst[c, 1, r, j] = sign[j] * src[c * chunk_rows + r, perm[j]]                  (one fp32 product by +-1.0f: exact, -0.0 and denormals included)
 * so chunk c of dst is one contiguous mini-batch of 2 * chunk_rows rows: the originals, then their mirror images.  perm == sign == NULL: both halves are copies.
 * perm (int16 [width]) and sign (fp32 [width]) live in the buffers' memory space and are uploaded once; the launch cannot read them back, so go2nn_mirror_check_table checks
 * them in HOST memory before the upload: GO2NN_EINVAL for a null pointer, width outside [1, 32767], perm[j] outside [0, width), a sign that is neither +1 nor -1.
 * go2nn_mirror_rows: GO2NN_EINVAL, with nothing written, for a null pointer (jobs, src, dst; perm without sign or sign without perm), n_jobs outside
 * [1, GO2NN_MIRROR_MAX_JOBS], chunks or chunk_rows < 1, width outside [1, 32767], a dst of 2^31 elements or more, 2^24 blocks or more (a block covers up to 4096
 * source floats of ONE chunk of one job); the host build also for perm[j] outside [0, width). */
#define GO2NN_MIRROR_MAX_JOBS 16
typedef struct Go2nnMirrorJob {
  const float* src;
  float* dst;
  int32_t width;
  const int16_t* perm;
  const float* sign;
} Go2nnMirrorJob;
int go2nn_mirror_check_table(const int16_t* host_perm, const float* host_sign, int32_t width);
int go2nn_mirror_rows(const Go2nnMirrorJob* jobs, int32_t n_jobs, int32_t chunks, int32_t chunk_rows, void* stream);

/* ---- the mirror (equivariance) loss of symmetry-augmented PPO (go2_rl_gym_amd/rsl_rl/algorithms/ppo.py, `algorithm.mirror_loss_coef`; csrc/go2nn_mirror_loss.h).
 * ADDED WITHIN ABI 7: four new entry points and one struct, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * An augmented mini-batch is [B originals | B mirror images]; with the involutive (perm, sign) table of the action vector, for pair r:
 *   e[r, j] = mu[r, j] - sign[j] mu[B + r, perm[j]]           mu = y_a W_mu^T + b_mu (the fp32 dot products of go2nn_ppo_heads)
 *   L = coef / (B A) sum_r sum_j e[r, j]^2                    (L / coef is the batch's equivariance_rmse^2)
 *   g[r, j] = 2 coef / (B A) e[r, j],   g[B + r, perm[j]] = -sign[j] g[r, j]          (both halves receive gradient)
 * Two plain launches (capturable) behind go2nn_ppo_heads on the same stream — the pass, then one block that adds the workgroups' fp64 sums of e^2 and leaves L,
 * rounded once, in the first partial row —: (g W_mu) * ELU'(y_a) (ELU' from the output: y > 0 ? 1 : y + 1) is ADDED to gz_a, and
 * `partials` receives go2nn_mirror_loss_rows(B, A, K) rows of go2nn_mirror_loss_cols(A, K) columns whose column sums (go2nn_sum_rows) are
 *   [ L, 0, 0, 0 | dW_mu [A, K] | gb_a [K] = the column sums of what was added to gz_a | db_mu [A] ]
 * Fixed summation order, no atomics: two launches give the same bits.  perm == sign == NULL: the identity table.  perm (int16 [A]) and sign (fp32 [A]) live in the
 * buffers' memory space; the launch cannot read them back, so go2nn_mirror_loss_check_table checks them in HOST memory before the upload: GO2NN_EINVAL for a null
 * pointer, A outside [1, 16], perm[j] outside [0, A), a sign that is neither +1 nor -1, perm[perm[j]] != j, sign[perm[j]] != sign[j].
 * go2nn_mirror_loss: GO2NN_EINVAL, with nothing written, for a null struct or pointer (y_a, w_mu, b_mu, gz_a, partials; perm without sign or sign without perm),
 * B < 1, A outside [1, 16], K not a multiple of 4 in [4, 256]; the host build also for a table go2nn_mirror_loss_check_table refuses. */
typedef struct Go2nnMirrorLoss {
  const float* y_a;            /* [2B, K] last hidden activations of the actor: row r and row B + r are a pair */
  const float *w_mu, *b_mu;    /* head [A, K], [A] */
  const int16_t* perm; const float* sign;   /* [A] */
  float* gz_a;                 /* [2B, K]: ADDED to (go2nn_ppo_heads has written it on the same stream) */
  float* partials;             /* go2nn_mirror_loss_rows x go2nn_mirror_loss_cols */
  int32_t B, A, K; float coef;
} Go2nnMirrorLoss;
int32_t go2nn_mirror_loss_rows(int32_t B, int32_t A, int32_t K);
int32_t go2nn_mirror_loss_cols(int32_t A, int32_t K);
int go2nn_mirror_loss_check_table(const int16_t* host_perm, const float* host_sign, int32_t A);
int go2nn_mirror_loss(const Go2nnMirrorLoss* a, void* stream);

/* ---- the update's diagnostics: what a PPO user reads to find out why a run stalls — clip fraction, KL, explained variance, gradient norm — computed on the device
 * inside the captured update (go2_rl_gym_amd/rsl_rl/algorithms/_diag.py, `algorithm.diagnostics`; csrc/go2nn_diag.h).  READ-ONLY: nothing training reads is written.
 * ADDED WITHIN ABI 7: four new entry points, one struct and one enum, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * Per mini-batch step and per SEGMENT of its rows (surrogate_split = 0: one segment, all rows; n > 0: rows [0, n) and rows [n, B), the CTS teacher / student rows) one
 * row of GO2NN_DIAG_NUM fp64 columns.  For row i, with mu = y_a W_mu^T + b_mu and v = y_c w_v + b_v (the fp32 dot products of go2nn_ppo_heads), all in fp32:
 *   lp  = sum_j [-(a_j - mu_j)^2 / (2 std_j^2) - log std_j - log sqrt(2 pi)]        the log-probability of the stored action
 *   lr  = lp - old_logp,   rho = exp(lr)
 *   kl  = sum_j [log(std_j / old_sigma_j + 1e-5) + (old_sigma_j^2 + (old_mu_j - mu_j)^2) / (2 std_j^2) - 1 / 2]      (go2nn_ppo_heads' expression for its mean KL)
 *   err = returns - v
 * and every column is the fp64 sum (or extremum) of the rows' fp32 terms: */
enum {
  GO2NN_DIAG_ROWS = 0,        /* rows of the segment */
  GO2NN_DIAG_RATIO_CLIPPED,   /* rows with |rho - 1| > clip */
  GO2NN_DIAG_RATIO_SUM,       /* sum rho */
  GO2NN_DIAG_LOGRATIO_SUM,    /* sum lr */
  GO2NN_DIAG_K3_SUM,          /* sum (rho - 1) - lr */
  GO2NN_DIAG_KL_SUM,          /* sum kl */
  GO2NN_DIAG_KL_MAX,          /* max kl */
  GO2NN_DIAG_ADV_SUM,         /* sum adv (the advantages as the mini-batch holds them) */
  GO2NN_DIAG_ADV_SQ,          /* sum adv^2 */
  GO2NN_DIAG_ADV_POS,         /* rows with adv > 0 */
  GO2NN_DIAG_VERR_SUM,        /* sum err */
  GO2NN_DIAG_VERR_SQ,         /* sum err^2 */
  GO2NN_DIAG_VERR_ABS_MAX,    /* max |err| */
  GO2NN_DIAG_RET_SUM,         /* sum returns */
  GO2NN_DIAG_RET_SQ,          /* sum returns^2 */
  GO2NN_DIAG_VALUE_CLIPPED,   /* rows with |v - old_values| > clip */
  GO2NN_DIAG_RATIO_MAX,       /* max rho */
  GO2NN_DIAG_RATIO_MIN,       /* min rho */
  GO2NN_DIAG_NUM
};
/* go2nn_ppo_diag: two plain launches (capturable) on the stream of go2nn_ppo_heads, behind it.  The pass streams y_a, y_c [B, K] and the per-row inputs of
 * go2nn_ppo_heads once (GO2NN_DIAG_PASS_ROWS rows per workgroup, loads dense along K) and leaves per-workgroup partial rows in `partials`:
 * go2nn_ppo_diag_rows(B, A, K) x segments x GO2NN_DIAG_NUM doubles, segments = surrogate_split > 0 ? 2 : 1.  The finish, one block, combines them in increasing row
 * order, writes table[*cursor] ([slots][segments][GO2NN_DIAG_NUM]) and advances the device-side cursor by one; a cursor outside [0, slots) writes nothing and stays.
 * The caller zeroes the cursor once per update.  No atomics, fixed order: two launches give the same bits.
 * GO2NN_EINVAL, with nothing written, for a null struct or pointer, B < 1, A outside [1, 16], K not a multiple of 4 in [4, 256], surrogate_split outside [0, B),
 * slots < 1. */
#define GO2NN_DIAG_PASS_ROWS 48
typedef struct Go2nnPpoDiag {
  const float *y_a, *y_c, *w_mu, *b_mu, *w_v, *b_v, *std, *actions, *old_mu, *old_sigma, *old_logp, *adv, *old_values, *returns;      /* as Go2nnPpoHeads */
  double* partials;            /* go2nn_ppo_diag_rows x segments x GO2NN_DIAG_NUM */
  double* table;               /* [slots][segments][GO2NN_DIAG_NUM] */
  int32_t* cursor;             /* one int32 in the buffers' memory space */
  int32_t B, A, K, surrogate_split, slots;
  float clip;
} Go2nnPpoDiag;
int32_t go2nn_ppo_diag_rows(int32_t B, int32_t A, int32_t K);
int go2nn_ppo_diag(const Go2nnPpoDiag* a, void* stream);
/* go2nn_grad_sqnorm: out[*cursor] = sum over `count` tensors (1 .. GO2NN_GRAD_SQNORM_MAX, the limit of go2sim_adam_clip_step) of the squares of their numel[i]
 * floats — the squared L2 norm that clip_grad_norm_ sees, BEFORE clipping — with the squares and every sum in fp64, then the cursor advances by one; a cursor outside
 * [0, slots) writes nothing and stays.  `grads` and `numel` are HOST arrays (of device pointers / of sizes): they travel by value in the kernel arguments.  Two plain
 * launches (capturable), a two-stage fixed-order reduction: `partials` holds go2nn_grad_sqnorm_rows(numel, count) doubles (one per GO2NN_GRAD_SQNORM_CHUNK floats of
 * every tensor).  GO2NN_EINVAL, with nothing written, for a null pointer, count outside [1, GO2NN_GRAD_SQNORM_MAX], a numel < 1 (or above
 * INT32_MAX - GO2NN_GRAD_SQNORM_CHUNK: the kernel's element index is an int), slots < 1. */
#define GO2NN_GRAD_SQNORM_MAX 48
#define GO2NN_GRAD_SQNORM_CHUNK 4096
int32_t go2nn_grad_sqnorm_rows(const int32_t* host_numel, int32_t count);
int go2nn_grad_sqnorm(const float* const* host_grads, const int32_t* host_numel, int32_t count, double* partials, double* out, int32_t* cursor, int32_t slots, void* stream);

/* ---- the evaluator's left-right asymmetry scores: how far is the policy from equivariant on the states it visits, and does the robot load its left and right legs
 * equally (go2_rl_gym_amd/utils/evaluator.py, `evaluation.asymmetry`; the tables: go2_rl_gym_amd/utils/symmetry.py; csrc/go2nn_asym.h).
 * ADDED WITHIN ABI 7: three new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * An asymmetry evaluation step is { a = policy(o), go2nn_mirror_rows(o), a_m = policy(M_o o), go2sim_step(a), ..., go2nn_asym_accumulate(a, a_m) }: one more plain
 * launch per step after the simulator's (capturable; one lane per env, the twelve joints and four feet unrolled inside the lane, no LDS, no atomics, no cross-lane
 * traffic), and one go2nn_asym_reduce at the end.
 * The table: fp32 [GO2NN_ASYM_NUM, N], row-major by row, column e = env e: the rows of the first enum below.  Counts are whole numbers held in fp32 (exact below 2^24).
 * go2nn_asym_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).  It does not see the struct: the struct's small
 * tables are checked on the host by every accumulate call, before its launch.
 * go2nn_asym_accumulate (AFTER the step), per env, with s = STEP[e], a = actions[e, :], a_m = mirrored_actions[e, :] (both fp32 [N, 12] row-major, plain pointers: they
 * are per-step tensors, captured per launch like go2sim_step's action pointer):
 *   s < 0:  nothing but STEP = s + 1.
 *   otherwise, a reset frame included (the action was computed from a valid observation), with e_j = a[j] - action_sign[j] * a_m[action_perm[j]]:
 *     EQ_STEPS += 1;  EQ_SQ += sum_j e_j^2;  EQ_SQ_HIP / _THIGH / _CALF += the same sum over the joints of joint_kind 0 / 1 / 2;  ACT_SQ += sum_j a[j]^2;
 *     EQ_MAX = max(EQ_MAX, max_j |e_j|).
 *   and, only when reset_buf is clear AND commands[e, 1] == 0.f && commands[e, 2] == 0.f (vy and yaw rate; the comparison is exact: -0.0f is zero, 1e-30f is not — the
 *   evaluator rewrites the scenario's or maneuver's command every step, so its zeros are exact):
 *     SYM_STEPS += 1;  per side (joint_side[j] / foot_side[f] = +1 left, -1 right):  ACT_SQ_L/R += sum a[j]^2;  TORQUE_SQ_L/R += sum torques[j]^2;
 *     POWER_L/R += sum |torques[j] * dof_vel[j]|;  CONTACT_L/R += the side's feet with contact_forces[foot, z] > contact_threshold (strictly: the gait rule).
 *   STEP = s + 1.  Sums of one step are formed in a local in joint order 0 .. 11 and added to the row once.
 * go2nn_asym_reduce: out [G, GO2NN_ASYM_OUT_NUM] (fp64), per group g: column 0 its envs; column 1 + r, r = 0 .. GO2NN_ASYM_NUM - 2, the fp64 sum of table row r + 1 (every
 * row but STEP) — except the EQ_MAX column, which is the MAX over the group's envs (0 for an empty group); then for each of the four pairs ACT_SQ, TORQUE_SQ, POWER, CONTACT
 * two columns: the sum over the group's envs with L + R > 0 of the per-robot |L - R| / (L + R) (fp64), and the number of such envs (a pooled |sum L - sum R| would let
 * robots limping on opposite sides cancel).  The summation scheme (and the device function) of go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, an empty
 * group gives zeros.  Group ids outside [0, G) are ignored by the device build, which cannot read them back on the host; the host build refuses them. */
enum {
  GO2NN_ASYM_STEP = 0, GO2NN_ASYM_EQ_STEPS, GO2NN_ASYM_EQ_SQ, GO2NN_ASYM_EQ_SQ_HIP, GO2NN_ASYM_EQ_SQ_THIGH, GO2NN_ASYM_EQ_SQ_CALF, GO2NN_ASYM_ACT_SQ, GO2NN_ASYM_EQ_MAX,
  GO2NN_ASYM_SYM_STEPS, GO2NN_ASYM_ACT_SQ_L, GO2NN_ASYM_ACT_SQ_R, GO2NN_ASYM_TORQUE_SQ_L, GO2NN_ASYM_TORQUE_SQ_R, GO2NN_ASYM_POWER_L, GO2NN_ASYM_POWER_R,
  GO2NN_ASYM_CONTACT_L, GO2NN_ASYM_CONTACT_R, GO2NN_ASYM_NUM
};
#define GO2NN_ASYM_PAIR0 GO2NN_ASYM_ACT_SQ_L                                /* the four (L, R) row pairs start here */
#define GO2NN_ASYM_OUT_N 0
#define GO2NN_ASYM_OUT_ROW0 1                                               /* column GO2NN_ASYM_OUT_ROW0 + r - 1 belongs to table row r >= 1 */
#define GO2NN_ASYM_OUT_IMB0 (GO2NN_ASYM_OUT_ROW0 + GO2NN_ASYM_NUM - 1)      /* then per pair p: the imbalance sum at IMB0 + 2 p, its env count at IMB0 + 2 p + 1 */
#define GO2NN_ASYM_OUT_NUM (GO2NN_ASYM_OUT_IMB0 + 8)
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's: commands [N, >= 3], dof_state [N, 12, 2] (dof_vel_offset elements from a joint's
 * position to its velocity), torques [N, 12], contact_forces [N, bodies, 3] with contact_body_stride between bodies, reset_buf uint8 (comp_stride unused, may be 0).
 * foot_body names the four foot bodies, foot_side / joint_side are +1 (left) or -1 (right), joint_kind 0 hip, 1 thigh, 2 calf; action_perm / action_sign are the action
 * mirror table BY VALUE (twelve entries need no device table).  contact_threshold in newtons, finite and >= 0.  Nothing but the table is written. */
typedef struct Go2nnAsymIn {
  Go2nnEvalField commands, dof_state, torques, contact_forces, reset_buf;
  int32_t dof_vel_offset;
  int32_t contact_body_stride;
  int32_t foot_body[4];
  int32_t foot_side[4];
  int32_t joint_side[12];
  int32_t joint_kind[12];
  int16_t action_perm[12];
  float action_sign[12];
  float contact_threshold;
  int32_t pad_;
} Go2nnAsymIn;
/* GO2NN_EINVAL for a null table or N < 1. */
int go2nn_asym_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL, with nothing written, for null pointers, N < 1, an env stride < 1, a component stride (vector fields) < 1, dof_vel_offset or contact_body_stride < 1,
 * foot_body < 0, action_perm[j] outside [0, 12), an action_sign / foot_side / joint_side that is not +-1, joint_kind outside 0 .. 2, a contact_threshold that is negative
 * or not finite. */
int go2nn_asym_accumulate(const Go2nnAsymIn* in, const float* actions, const float* mirrored_actions, float* table, int32_t N, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, G outside 1 .. 65535; the host build also for a group id outside [0, G). */
int go2nn_asym_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);

/* ---- the evaluator's confidence intervals: bootstrap replicates of go2nn_eval_reduce's table (go2_rl_gym_amd/utils/evaluator.py, `evaluation.bootstrap`;
 * csrc/go2nn_bootstrap.h, the launch in csrc/go2nn_eval.h).
 * ADDED WITHIN ABI 7: two new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * One plain launch (capturable) after go2nn_eval_reduce, on the same acc [GO2NN_EVAL_NUM, N]: a STRATIFIED bootstrap — the robots are redrawn with replacement inside
 * their cells, every cell keeps its size.  The cells' members come as a CSR list: cell_start int32 [G + 1], cell_envs int32 [cell_start[G]], the envs of cell g at
 * cell_envs[cell_start[g] .. cell_start[g + 1]) (the evaluator lists them ascending), both in acc's memory space.  With n = cell_start[g + 1] - cell_start[g]:
 *   out[(b G + g) 12 + c] = sum over k = 0 .. n - 1 of term(cell_envs[cell_start[g] + j(b, g, k)], c)                     out: fp64 [B, G, GO2NN_EVAL_NUM + 2] row-major
 *   j(b, g, k) = ((uint64) x * n) >> 32,   x = word (k & 3) of philox4x32_10(counter (b, g, k >> 2, 0), key (seed, 7))
 * term(e, c) is go2nn_eval_reduce's: acc[c, e] for c < GO2NN_EVAL_NUM, 1 for c = GO2NN_EVAL_NUM, acc[FALLS, e] == 0 for the last column.  The sum runs in fp64 in
 * increasing k and the index is integer arithmetic, so the device, the host build and a restatement in Python integers agree bit for bit; an empty cell gives twelve
 * zeros; replicate b does not depend on B.  Key word 7 is the bootstrap's: 1 .. 6 belong to the sensor kernels.  One lane per (replicate, cell), no LDS, no atomics.
 * go2nn_eval_bootstrap_check looks at the list in HOST memory before the upload (the launch cannot report a bad index): GO2NN_EINVAL for a null pointer, N < 1, G outside
 * [1, 65535], cell_start[0] != 0, a decreasing cell_start, cell_start[G] > N, an env outside [0, N).
 * go2nn_eval_bootstrap: GO2NN_EINVAL, with nothing written, for a null pointer, N < 1, G outside [1, 65535], B outside [1, 2^20], B G 12 >= 2^31; the host build also for
 * what go2nn_eval_bootstrap_check refuses. */
int go2nn_eval_bootstrap_check(const int32_t* host_cell_start, const int32_t* host_cell_envs, int32_t N, int32_t G);
int go2nn_eval_bootstrap(const float* acc, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);

/* ---- the same replicates of every scoring family's reduce table (`evaluation.bootstrap_all`; csrc/go2nn_bootstrap.h).
 * ADDED WITHIN ABI 7: five new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * THE RULE, ONCE: replicate (b, g) of every family draws the same members as go2nn_eval_bootstrap's — j(b, g, k) above depends on (b, g, k, seed) and the cell's size, not on
 * the table — so a replicate's rows across the tables are ONE resampled population (a robot drawn twice brings its pushes, its switches and its strides twice).
 * Each entry point is its family's reduce with the group's envs replaced by the draws: `table` is the family's per-robot table, term(e, c) the family's reduce term, cols its
 * reduce width (robust GO2NN_ROBUST_ACC_NUM + 1, maneuver GO2NN_MANEUVER_ACC_NUM + 1, ladder GO2NN_LADDER_OUT_NUM, gait GO2NN_GAIT_OUT_NUM, asym GO2NN_ASYM_OUT_NUM):
 *   out[(b G + g) cols + c] = sum over k = 0 .. n - 1 of term(cell_envs[cell_start[g] + j(b, g, k)], c)                     out: fp64 [B, G, cols] row-major
 * in fp64 in increasing k; the asym table's EQ_MAX column is the MAX over the drawn members instead (as go2nn_asym_reduce's is the group's max).  An empty cell gives zeros.
 * One lane per (replicate, cell, column window), no LDS, no atomics; the gait table is split into column windows whose lanes recompute the same draws.
 * GO2NN_EINVAL, with nothing written: go2nn_eval_bootstrap's cases with the bound B G cols < 2^31; the ladder also for dist2_thr <= 0 (go2nn_ladder_reduce's argument). */
int go2nn_robust_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);
int go2nn_maneuver_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);
int go2nn_ladder_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, float dist2_thr, double* out,
                           void* stream);
int go2nn_gait_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);
int go2nn_asym_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);

/* ---- empirical (running mean / std) normalisation of the observations of feed-forward PPO (go2_rl_gym_amd/rsl_rl/modules/normalizer.py, rsl_rl/algorithms/ppo.py,
 * `runner.empirical_normalization`; csrc/go2nn_obs_norm.h).
 * ADDED WITHIN ABI 7: three new entry points and one struct, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * go2nn_obs_norm_apply: one plain launch (capturable) per policy step for up to GO2NN_OBS_NORM_MAX_JOBS row-major fp32 [N, D] tensors; the job index sits in the grid.
 *   y[r, c] = (x[r, c] - mean[c]) * inv[c]                 one fp32 subtraction, one fp32 product (no FMA can form): the device, the host build and numpy agree bit for bit
 *   clip > 0:  y = y < -clip ? -clip : (y > clip ? clip : y)
 * y may BE x (in place); otherwise the two must not overlap.  mean, inv: fp32 [D] in the buffers' memory space.  partials == NULL: normalise only.  Otherwise partials is
 * fp64 [go2nn_obs_norm_partial_rows(N), D, 2]: row b receives, per column, the sums of d and of d * d over rows [b * GO2NN_OBS_NORM_ROWS, (b + 1) * GO2NN_OBS_NORM_ROWS)
 * of x, d = (double) x - (double) mean: centred on the frozen mean, so S2 - S1^2 / n does not cancel later.  Fixed summation order (a wave's rows in increasing order, then
 * the four waves in order through LDS), no atomics: two launches give the same bits.
 * GO2NN_EINVAL, with nothing written, for a null pointer (jobs, x, y, mean, inv), n_jobs outside [1, GO2NN_OBS_NORM_MAX_JOBS], N < 1, D outside [1, 4096], a clip that
 * is not finite.
 * go2nn_obs_norm_update: one plain launch (capturable), one block, one lane per column.  table: fp64 [steps, rows, D, 2], the partial tables of the iteration's apply
 * launches; state: fp64 [1 + 2 D] = count | mean [D] | M2 [D] (M2: the sum of squared deviations; var = M2 / count, the population variance; at count 0 M2 is not read —
 * the initial var = 1 is forgotten at the first batch); n: the table's samples.  Per column, reading its old mean32 first: S1, S2 = the table's sums in increasing
 * (step, row) order; batch mean = mean32_old + S1 / n, batch M2 = S2 - S1^2 / n (floored at 0); Chan's pooled update into the state; mean32 = (float) mean,
 * inv32 = (float) (1 / (sqrt(M2 / count) + eps)).
 * GO2NN_EINVAL, with nothing written, for a null pointer, steps, rows or D below 1 (D above 4096), n or eps not finite and above 0. */
#define GO2NN_OBS_NORM_MAX_JOBS 4
#define GO2NN_OBS_NORM_ROWS 64
typedef struct Go2nnObsNormJob {
  const float* x;
  float* y;
  const float* mean;
  const float* inv;
  double* partials;
  int32_t D;
  float clip;
} Go2nnObsNormJob;
int32_t go2nn_obs_norm_partial_rows(int32_t N);          /* ceil(N / GO2NN_OBS_NORM_ROWS); 0 for N < 1 */
int go2nn_obs_norm_apply(const Go2nnObsNormJob* jobs, int32_t n_jobs, int32_t N, void* stream);
int go2nn_obs_norm_update(const double* table, int32_t steps, int32_t rows, int32_t D, double* state, double n, double eps, float* mean32, float* inv32, void* stream);

/* ---- value normalisation: the critic predicts returns normalised by their running mean / std (go2_rl_gym_amd/rsl_rl/modules/normalizer.py:ValueNormalization,
 * rsl_rl/algorithms/_base.py, `algorithm.normalize_value`; csrc/go2nn_value_norm.h).
 * ADDED WITHIN ABI 7: four new entry points, nothing existing changes, GO2NN_ABI_VERSION stays 7.  All three launches are plain and capturable.
 * stat32: fp32 [3] = mean32 | std32 | inv32 in the buffers' memory space, mean32 = (float) mean, std32 = (float) (sqrt(var) + eps), inv32 = (float) (1 / (sqrt(var) + eps)).
 * go2nn_value_norm_apply: in place over the n floats of `values` and of `returns` (they must not overlap)
 *   x <- (x - mean32) * inv32                 one fp32 subtraction, one fp32 product (no FMA can form), no clamp: the device, the host build, torch and numpy agree bit for bit
 * A 256-lane block owns GO2NN_VALUE_NORM_ROWS consecutive elements; 16-byte accesses only where both pointers are 16-byte aligned.  partials == NULL: normalise only.
 * Otherwise partials is fp64 [go2nn_value_norm_partial_rows(n), 2]: row b receives the sums of d and of d * d over elements [b * ROWS, (b + 1) * ROWS) of the RAW
 * returns, d = (double) R - (double) mean32.  Fixed summation order, no atomics: two launches give the same bits.
 * GO2NN_EINVAL, with nothing written, for a null values, returns or stat32, a pointer not aligned to a float, n < 1.
 * go2nn_value_norm_update: one block.  state: fp64 [3] = count | mean | M2 (var = M2 / count; at count 0 M2 is not read: the initial var = 1 is forgotten at the first
 * batch); n: the table's samples.  Reading the old stat32 first: S1, S2 = the rows' sums in increasing order; batch mean = mean32_old + S1 / n, batch M2 = S2 - S1^2 / n
 * (floored at 0); Chan's pooled update into the state; stat32 rewritten.  w_last != NULL (output preservation): the critic's last layer, fp32 [K] and b_last fp32 [1], is
 * rewritten W <- W sigma / sigma', b <- (sigma b + mu - mu') / sigma' with (mu, sigma) the old and (mu', sigma') the new mean32, std32: v * std32 + mean32 of every
 * input stays what it was.  w_last == NULL: no preservation, b_last and K are not read.
 * GO2NN_EINVAL, with nothing written, for a null partials, state or stat32, rows < 1, n or eps not finite and above 0, w_last given with b_last null or K < 1.
 * go2nn_value_head_fold: w_out[k] = w[k] * std32 (k < K), b_out[0] = b[0] * std32 + mean32: the last layer of a critic whose packed operand buffer answers in raw units.
 * GO2NN_EINVAL, with nothing written, for a null pointer or K < 1. */
#define GO2NN_VALUE_NORM_ROWS 1024
int32_t go2nn_value_norm_partial_rows(int32_t n);          /* ceil(n / GO2NN_VALUE_NORM_ROWS); 0 for n < 1 */
int go2nn_value_norm_apply(float* values, float* returns, int32_t n, const float* stat32, double* partials, void* stream);
int go2nn_value_norm_update(const double* partials, int32_t rows, double* state, double n, double eps, float* stat32, float* w_last, float* b_last, int32_t K, void* stream);
int go2nn_value_head_fold(const float* w, const float* b, int32_t K, const float* stat32, float* w_out, float* b_out, void* stream);

/* ---- the temporal action-smoothness loss of PPO on env-block mini-batches (go2_rl_gym_amd/rsl_rl/algorithms/ppo.py, `algorithm.smooth_loss_coef`; csrc/go2nn_smooth_loss.h).
 * ADDED WITHIN ABI 7: five new entry points and one struct, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A mini-batch in block layout is blocks x T x n rows, row r = b T n + t n + j: all T steps of n environments (blocks = 2: followed by their mirror images).  For t < T - 1,
 * with the pair weights w[t, j] in {0, 1} (0: an episode boundary between steps t and t + 1 of env j):
 *   e[b, t, j, :] = w[t, j] (mu[b, t, j, :] - mu[b, t + 1, j, :])           mu = y_a W_mu^T + b_mu (the fp32 dot products of go2nn_ppo_heads)
 *   L = coef / (blocks (T - 1) n A) sum e^2                                 (a fixed denominator: masked pairs add 0)
 *   g[b, t, j, :] = 2 coef / (blocks (T - 1) n A) (e[b, t, j, :] - e[b, t - 1, j, :]),   e[., -1] = e[., T - 1] = 0          (both rows of a pair receive gradient)
 * go2nn_smooth_loss: two plain launches (capturable) behind go2nn_ppo_heads (and go2nn_mirror_loss) on the same stream — the pass, then one block that adds the workgroups'
 * fp64 sums of e^2 and leaves L, rounded once, in the first partial row —: (g W_mu) * ELU'(y_a) (ELU' from the output: y > 0 ? 1 : y + 1) is ADDED to gz_a, and `partials`
 * receives go2nn_smooth_loss_rows(blocks, T, n, A, K) rows of go2nn_smooth_loss_cols(A, K) columns whose column sums (go2nn_sum_rows) are
 *   [ L, 0, 0, 0 | dW_mu [A, K] | gb_a [K] = the column sums of what was added to gz_a | db_mu [A] ]
 * Fixed summation order, no atomics: two launches give the same bits.  GO2NN_EINVAL, with nothing written, for a null struct or pointer, blocks outside [1, 2], T < 2, n < 1,
 * A outside [1, 16], K not a multiple of 4 in [4, 256], blocks T n K >= 2^31, a coefficient that is negative or not finite.
 * go2nn_smooth_loss_set_segments: the number of time segments the device pass splits T into (csrc/go2nn_smooth_loss.h; 0, the default: its own choice); a measurement
 * hook — go2nn_smooth_loss_rows follows it, the results agree to rounding of the partial sums.  The host build accepts and ignores it.
 * go2nn_smooth_indices: the env-block mini-batches.  With pi = go2_shuffle_index(., N, ...) of include/go2sim_shuffle.h under (key_state[0], key_state[1]) and n = N / nmb,
 *   out[i T n + t n + j] = t N + pi(i n + j)          the int64 index list go2sim_shuffle_gather takes as `indices` (rows of the [T, N] rollout)
 *   w  [i T n + t n + j] = t < T - 1 && dones[t N + pi(i n + j)] == 0          (uint8; dones: the storage's [T, N] uint8 tensor, time-outs included)
 * and key_state[1] += 1 by a one-lane second launch, so a replayed graph draws a new permutation every time.  GO2NN_EINVAL, with nothing written, for a null pointer,
 * nmb < 1, T < 2, N < 1, N not a multiple of nmb, T N >= 2^31. */
typedef struct Go2nnSmoothLoss {
  const float* y_a;            /* [blocks*T*n, K] */
  const float *w_mu, *b_mu;    /* [A, K], [A] */
  const uint8_t* w;            /* [T*n] pair weights of this mini-batch (row T-1 is 0) */
  float* gz_a;                 /* [blocks*T*n, K]: ADDED to */
  float* partials;             /* go2nn_smooth_loss_rows x go2nn_smooth_loss_cols: [L,0,0,0 | dW_mu | gb_a | db_mu] */
  int32_t blocks, T, n, A, K; float coef;
} Go2nnSmoothLoss;
int32_t go2nn_smooth_loss_rows(int32_t blocks, int32_t T, int32_t n, int32_t A, int32_t K);
int32_t go2nn_smooth_loss_cols(int32_t A, int32_t K);
int go2nn_smooth_loss_set_segments(int32_t segments);
int go2nn_smooth_loss(const Go2nnSmoothLoss* a, void* stream);
int go2nn_smooth_indices(int64_t* out, uint8_t* w, const uint8_t* dones, int32_t nmb, int32_t T, int32_t N, uint32_t* key_state, void* stream);

/* ---- the evaluator's action and torque spectra: how fast are the joints of every evaluated robot being driven (go2_rl_gym_amd/utils/evaluator.py, `evaluation.spectrum`;
 * csrc/go2nn_spectrum.h).
 * ADDED WITHIN ABI 7: four new entry points and one struct, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * A spectrum evaluation step is { ..., go2sim_step, go2nn_eval_accumulate, ..., go2nn_spectrum_record }: one more plain launch per step (capturable; one lane per robot, no
 * atomics), then ONE go2nn_spectrum_welch after the last step and one go2nn_spectrum_reduce.
 * THE ESTIMATOR, ONCE: Welch's method on the T counted steps, per robot.  24 signals: the 12 entries of the simulator's `actions` and the 12 of `torques` AFTER the step,
 * sampled at the policy rate fs = 1 / (sim dt x decimation).  Windows of W samples (even, 8 <= W <= 256), hop W / 2: window w covers the counted frames
 * [w W / 2, w W / 2 + W); a tail shorter than W is dropped; the positions do not depend on what the robot does.  A window is SKIPPED (and counted as such) when any of its
 * frames has reset_buf set: that frame shows the post-reset pose, and nothing is analysed across an episode boundary.  Per used window and signal x[0 .. W):
 *   y[n] = (x[n] - mean(x)) hann[n],   hann[n] = 0.5 - 0.5 cos(2 pi n / W)   (periodic),   X_k = sum_n y[n] exp(-2 pi i k n / W),   k = 0 .. W / 2
 *   P_k = c_k |X_k|^2 / (fs sum hann^2)        c_k = 2 except c_0 = c_{W/2} = 1          (scipy.signal.welch: window "hann", detrend "constant", scaling "density")
 *   M_k = c_k |X_k| / sum hann                 (the amplitude of a sinusoid on bin k)
 * in fp64 (sum hann = W / 2, sum hann^2 = 3 W / 8).  The 12 joints are pooled by KIND — slots 0 .. 3 the hips, 4 .. 7 the thighs, 8 .. 11 the calves; joint_of_slot names
 * the joint of every slot (utils/symmetry.py joint_kinds()) — and each window's sum over a kind's 4 joints is rounded once to fp32 and added to the robot's table column.
 * The trace: fp32 [GO2NN_SPECTRUM_TRACE_ROWS(T), N], row-major by row, column e = robot e: the STEP row, then per counted step s the GO2NN_SPECTRUM_CHANNELS rows
 * 1 + s 25 + channel — the action of slot 0 .. 11, the torque of slot 0 .. 11, the reset flag as 0.f / 1.f.  T x N x 25 x 4 bytes: the caller caps it.
 * The table: fp32 [GO2NN_SPECTRUM_ROWS(W), N], column e = robot e: USED (windows), SKIPPED (windows), then with K = W / 2 + 1 the row BIN0 + (signal 3 + kind) K + k =
 * sum P_k and the row BIN0 + 6 K + (signal 3 + kind) K + k = sum M_k over the used windows and the kind's 4 joints (signal 0 action, 1 torque; kind 0 hip, 1 thigh, 2 calf).
 * go2nn_spectrum_begin: trace = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).
 * go2nn_spectrum_record (AFTER the step), per robot, with s = STEP[e]: STEP[e] = s + 1; if 0 <= s < T the 25 floats of step s are written — bit-exact copies of the fields.
 * go2nn_spectrum_welch: the table of every robot from its trace, overwritten (not added to).  twiddle: fp64 [W, 2] = (cos, sin)(2 pi n / W) in the trace's memory space.
 *   No atomics, fixed summation order: two launches give the same bits, and the host build gives the device's.
 * go2nn_spectrum_reduce: out [G, GO2NN_SPECTRUM_OUT_NUM(W)] (fp64), per group g: column 0 its robots, column 1 + r the fp64 sum of table row r (go2nn_eval_reduce's order).
 * GO2NN_EINVAL, with nothing written: null pointers, N < 1, T outside [1, GO2NN_SPECTRUM_MAX_STEPS], W odd or outside [8, 256], fs not finite and above 0, an env stride < 1,
 * a component stride (actions, torques) < 1, a joint_of_slot that is no permutation of 0 .. 11, G outside 1 .. 65535. */
#define GO2NN_SPECTRUM_MIN_WINDOW 8
#define GO2NN_SPECTRUM_MAX_WINDOW 256
#define GO2NN_SPECTRUM_MAX_STEPS 1048576
#define GO2NN_SPECTRUM_CHANNELS 25
enum { GO2NN_SPECTRUM_CH_ACTION0 = 0, GO2NN_SPECTRUM_CH_TORQUE0 = 12, GO2NN_SPECTRUM_CH_RESET = 24 };
#define GO2NN_SPECTRUM_TRACE_STEP 0
#define GO2NN_SPECTRUM_TRACE_ROWS(T) (1 + GO2NN_SPECTRUM_CHANNELS * (T))
enum { GO2NN_SPECTRUM_USED = 0, GO2NN_SPECTRUM_SKIPPED, GO2NN_SPECTRUM_BIN0 };
#define GO2NN_SPECTRUM_BINS(W) ((W) / 2 + 1)
#define GO2NN_SPECTRUM_ROWS(W) (GO2NN_SPECTRUM_BIN0 + 12 * GO2NN_SPECTRUM_BINS(W))
#define GO2NN_SPECTRUM_OUT_N 0
#define GO2NN_SPECTRUM_OUT_ROW0 1
#define GO2NN_SPECTRUM_OUT_NUM(W) (GO2NN_SPECTRUM_OUT_ROW0 + GO2NN_SPECTRUM_ROWS(W))
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnEvalIn's: actions and torques [N, 12], reset_buf uint8 (comp_stride unused, may be 0). */
typedef struct Go2nnSpectrumIn {
  Go2nnEvalField actions, torques, reset_buf;
  int32_t joint_of_slot[12];
} Go2nnSpectrumIn;
int go2nn_spectrum_begin(float* trace, int32_t N, int32_t start, int32_t T, void* stream);
int go2nn_spectrum_record(const Go2nnSpectrumIn* in, float* trace, int32_t N, int32_t T, void* stream);
int go2nn_spectrum_welch(const float* trace, int32_t N, int32_t T, int32_t W, double fs, const double* twiddle, float* table, void* stream);
int go2nn_spectrum_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, int32_t W, double* out, void* stream);

/* ---- the evaluator's actuator loads: what does every evaluated robot do to its motors and its legs (go2_rl_gym_amd/utils/evaluator.py, `evaluation.actuators`;
 * csrc/go2nn_actuator.h).
 * ADDED WITHIN ABI 7: four new entry points and one struct, nothing existing changes, GO2NN_ABI_VERSION stays 7.
 * An actuator evaluation step is { ..., go2sim_step, go2nn_eval_accumulate, ..., go2nn_actuator_accumulate }: one more plain launch per step (capturable; one lane per robot,
 * the twelve joints and four feet unrolled inside the lane, no LDS, no atomics), one go2nn_actuator_reduce at the end and, for intervals, one go2nn_actuator_bootstrap.
 * The table: fp32 [GO2NN_ACTUATOR_NUM, N], row-major by row, column e = robot e: the per-robot rows of the first enum below, then GO2NN_ACTUATOR_JOINT_ROWS rows per joint j
 * (row GO2NN_ACTUATOR_JOINT0 + j * GO2NN_ACTUATOR_JOINT_ROWS + the second enum; j in the simulator's DOF order), then GO2NN_ACTUATOR_FOOT_ROWS rows per foot f (row
 * GO2NN_ACTUATOR_FOOT0 + f * GO2NN_ACTUATOR_FOOT_ROWS + the third enum; f in foot_body order).  Counts are whole numbers held in fp32 (exact below 2^24).
 * go2nn_actuator_begin: table = 0, then STEP[e] = start for every e (the evaluator passes -warmup_steps).
 * go2nn_actuator_accumulate (AFTER the step), per robot, with s = STEP[e]:
 *   STEP = s + 1.  s < 0: nothing more.  reset_buf set: the frame is not used (the gait rule: it shows the post-reset pose).
 *   otherwise, with first = (USED == 0):  USED += 1;  DIST += sqrt(vx^2 + vy^2), the root's world planar speed root_states[7:9] (x dt: metres);
 *   per joint j, with tau = torques[j] (the torque APPLIED in the last substep, after the simulator's clip), q = dof_state[j, 0], qd = dof_state[j, 1]:
 *     TAU_SQ += tau^2;  TAU_PEAK = max(TAU_PEAK, |tau|);  TAU_SAT += (|tau| >= tau_sat_thr[j]);  VEL_PEAK = max(VEL_PEAK, |qd|);  VEL_SAT += (|qd| >= vel_sat_thr[j]);
 *     p = tau * qd (one rounded fp32 product):  WORK_POS += max(p, 0);  WORK_NEG += max(-p, 0)          (x dt: joules)
 *     m = min(q - pos_lo[j], pos_hi[j] - q):  MARGIN_MIN = first ? m : min(MARGIN_MIN, m)                (negative past a limit)
 *   per foot f, with fz = contact_forces[foot_body[f], z]:  FZ_PEAK = max(FZ_PEAK, fz);  if fz > contact_threshold (strictly, the gait rule): FZ_SUM += fz, FZ_FRAMES += 1.
 *   The two saturation comparisons are exact fp32 comparisons against thresholds the host forms once (the evaluator: `actuators_saturation` x the nominal limit).
 * go2nn_actuator_reduce: out [G, GO2NN_ACTUATOR_OUT_NUM] (fp64), per group g: column N its robots, N_USED those with USED > 0, then column GO2NN_ACTUATOR_OUT_ROW0 + r - 1
 * the fp64 sum of table row r >= 1 (USED, DIST, the 96 joint rows, the 12 foot rows).  EVERY column is a sum: a peak or margin column is the sum over the robots of each
 * robot's own peak or margin (divide by N_USED for their mean); a robot with USED == 0 holds zeros in every row.  The summation scheme (and the device function) of
 * go2nn_eval_reduce: fixed order, bit-equal outputs for equal inputs, group ids outside [0, G) ignored, an empty group gives zeros.
 * go2nn_actuator_bootstrap: go2nn_gait_bootstrap's rule and refusals on this table and these columns (the same draws: replicate (b, g) of every family redraws the same robots). */
enum { GO2NN_ACTUATOR_STEP = 0, GO2NN_ACTUATOR_USED, GO2NN_ACTUATOR_DIST, GO2NN_ACTUATOR_JOINT0 };
enum {
  GO2NN_ACTUATOR_J_TAU_SQ = 0, GO2NN_ACTUATOR_J_TAU_PEAK, GO2NN_ACTUATOR_J_TAU_SAT, GO2NN_ACTUATOR_J_VEL_PEAK, GO2NN_ACTUATOR_J_VEL_SAT, GO2NN_ACTUATOR_J_WORK_POS,
  GO2NN_ACTUATOR_J_WORK_NEG, GO2NN_ACTUATOR_J_MARGIN_MIN, GO2NN_ACTUATOR_JOINT_ROWS
};
#define GO2NN_ACTUATOR_FOOT0 (GO2NN_ACTUATOR_JOINT0 + 12 * GO2NN_ACTUATOR_JOINT_ROWS)
enum { GO2NN_ACTUATOR_F_FZ_PEAK = 0, GO2NN_ACTUATOR_F_FZ_SUM, GO2NN_ACTUATOR_F_FZ_FRAMES, GO2NN_ACTUATOR_FOOT_ROWS };
#define GO2NN_ACTUATOR_NUM (GO2NN_ACTUATOR_FOOT0 + 4 * GO2NN_ACTUATOR_FOOT_ROWS)          /* 111 */
#define GO2NN_ACTUATOR_OUT_N 0
#define GO2NN_ACTUATOR_OUT_N_USED 1
#define GO2NN_ACTUATOR_OUT_ROW0 2                                           /* column GO2NN_ACTUATOR_OUT_ROW0 + r - 1 belongs to table row r >= 1 */
#define GO2NN_ACTUATOR_OUT_NUM (GO2NN_ACTUATOR_OUT_ROW0 + GO2NN_ACTUATOR_NUM - 1)          /* 112 = 7 x 16 = 8 x 14 = 4 x 28: equal column windows exist */
/* The buffers as (pointer, env stride, component stride) in ELEMENTS like Go2nnAsymIn's: dof_state [N, 12, 2] (dof_vel_offset elements from a joint's position to its
 * velocity), torques [N, 12], contact_forces [N, bodies, 3] with contact_body_stride between bodies, root_states [N, 13], reset_buf uint8 (comp_stride unused, may be 0).
 * foot_body names the four foot bodies.  BY VALUE (twelve entries need no device table): pos_lo / pos_hi [rad], the position limits the margin is taken to; tau_sat_thr
 * [N m] and vel_sat_thr [rad/s], at and above which a sample counts as saturated; contact_threshold in newtons, finite and >= 0.  Nothing but the table is written. */
typedef struct Go2nnActuatorIn {
  Go2nnEvalField dof_state, torques, contact_forces, root_states, reset_buf;
  int32_t dof_vel_offset;
  int32_t contact_body_stride;
  int32_t foot_body[4];
  float pos_lo[12], pos_hi[12];
  float tau_sat_thr[12], vel_sat_thr[12];
  float contact_threshold;
  int32_t pad_;
} Go2nnActuatorIn;
/* GO2NN_EINVAL for a null table or N < 1. */
int go2nn_actuator_begin(float* table, int32_t N, int32_t start, void* stream);
/* GO2NN_EINVAL, with nothing written, for null pointers, N < 1, an env stride < 1, a component stride (vector fields) < 1, dof_vel_offset or contact_body_stride < 1,
 * foot_body < 0, a position limit that is not finite or pos_lo > pos_hi, a saturation threshold that is not finite and above 0, a contact_threshold that is negative or
 * not finite. */
int go2nn_actuator_accumulate(const Go2nnActuatorIn* in, float* table, int32_t N, void* stream);
/* GO2NN_EINVAL for null pointers, N < 1, G outside 1 .. 65535. */
int go2nn_actuator_reduce(const float* table, const int32_t* group, int32_t N, int32_t G, double* out, void* stream);
int go2nn_actuator_bootstrap(const float* table, const int32_t* cell_start, const int32_t* cell_envs, int32_t N, int32_t G, int32_t B, uint32_t seed, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
