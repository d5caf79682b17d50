/*
 * npf_hip.h -- C ABI of the MI355X (gfx950) neural-process hot path.
 *
 * The reference (MarinerQ/npf_GWwaveform) is 100 % Python and has no FFI; the calls below
 * are what a maintainer would bind (ctypes) to replace the torch op
 * sequences of these reference functions (paths relative to the reference root):
 *
 *   npf_chain_run        MLP.forward                      npf/architectures/mlp.py:95-109
 *                        MergeFlatInputs.forward          npf/architectures/encoders.py:175-183
 *                        BaseAttender.forward / DotAttender.score
 *                                                         npf/architectures/attention.py:129-164,204-220
 *                        merge_r_z                        npf/neuralproc/base.py:554-575
 *                        (and the autograd backward of each: dgrad chains)
 *   npf_wgrad_run        autograd of nn.Linear weights/biases on the path (mlp.py:84-91) and
 *                        of torch.bmm / einsum wrt keys/values (attention.py:151,212)
 *   npf_gauss_head_fwd   NeuralProcessFamily.decode tail  npf/neuralproc/base.py:350-365 (+ :116),
 *                        pool_and_replicate_middle        npf/neuralproc/helpers.py:21-32,
 *                        sum_log_prob                     npf/losses.py:18-24
 *   npf_gauss_head_bwd   autograd of the above
 *   npf_masked_gauss_head_fwd/bwd  the same over a batch of padded targets whose per-task sizes are device data
 *   npf_mixture_summary  mean / std / quantiles of the predictive mixture over the latent samples (inference; no reference counterpart)
 *   npf_mixture_score    log density / PIT / CRPS of an observation under that mixture (inference; no reference counterpart)
 *   npf_waveform_match   overlap / match / mismatch of predicted against reference waveforms over a time-shift grid (inference; no
 *                        reference counterpart)
 *   npf_waveform_match_ex/_bwd  the same with the unrounded row scalars kept, and the gradient of the match with respect to the
 *                        predicted amplitude and phase (training on the mismatch; no reference counterpart)
 *   npf_waveform_match_bank  the match of every predicted waveform against every template of one shared bank, the contraction on
 *                        the double-precision matrix instruction (inference; no reference counterpart)
 *   npf_waveform_loglike  matched-filter SNR and log likelihood of complex data under the predicted waveforms, phase and arrival
 *                        time maximised or marginalised, and marginal over the latent samples (inference; no reference counterpart)
 *   npf_waveform_loglike_net  the coherent likelihood of a detector network: per-detector weights, delays and complex responses,
 *                        the complex correlations added before the modulus (inference; no reference counterpart)
 *   npf_waveform_loglike_dist/_net_dist  both likelihoods marginalised over a grid of amplitude scales (luminosity distance) as
 *                        well, with the distance posterior (inference; no reference counterpart)
 *   npf_mc_objective_fwd/bwd  mean / logsumexp / SUMO over the latent samples
 *                                                         npf/losses.py:146,197-200,262-274
 *   npf_mean_agg_fwd/bwd torch.mean(R_cntxt, dim=1)       npf/neuralproc/np.py:95, attnnp.py:181
 *   npf_pack_pt/unpack_pt  layout change at the module boundary (no reference counterpart)
 *   npf_transpose        W -> W^T for the dgrad chains (no reference counterpart)
 *   npf_cast_bf16_weights  bf16 weight images for the bf16 compute mode (no reference counterpart)
 *   npf_prepare_weights    the two above, batched over the layers of a chain (no reference counterpart)
 *   npf_gather_points    CntxtTrgtGetter.select              npf/utils/datasplit.py:246-255
 *   npf_masked_attn_fwd/bwd (and _fwd_nq / _bwd_nq: padded queries too), npf_masked_mean_fwd/bwd  DotAttender.forward / torch.mean(R_cntxt, dim=1) of a padded batch
 *                        whose per-task context sizes are device data (no reference counterpart: the reference cuts the batch)
 *   npf_masked_attn_fwd_loo, npf_loo_mean  the same for every context point over the OTHER points of its task (leave-one-out; inference)
 *   npf_masked_attn_fwd_weighted, npf_weighted_mean  the same for S replicates of one stored context that differ in a weight per key
 *                        (bootstrap multiplicities, fold masks; inference)
 *   npf_masked_attn_fwd_weighted_ex, npf_masked_attn_bwd_weighted, npf_weighted_mean_bwd  training through such weights at one
 *                        replicate: the forward pass with its log-sum-exp, and the gradients, the weights' included
 *   npf_append_points    new context rows behind the rows each task of such a padded batch holds (no reference counterpart)
 *   npf_split_heads/npf_merge_heads  MultiheadAttender._make_multiheaded / _concatenate_multiheads
 *                                                         npf/architectures/attention.py:505-527
 *
 * Conventions: plain device pointers + sizes, caller owns all memory, every call is
 * asynchronous on `stream` (a hipStream_t passed as void*), returns 0 on success and a
 * negative NPF_E* code otherwise (never throws, never allocates, never synchronises).
 * All tensors fp32.
 *
 * "PT32" layout (the on-device layout between kernels): points are grouped in tiles of 32
 * (each task padded to whole tiles); a tile of F features (F % 32 == 0) is stored as
 * [F/4][32 points][4 features], tiles of one task are consecutive, tasks are consecutive:
 *   elem(task, p, f) = (((task*tiles_per_task + p/32) * (F/4) + f/4) * 32 + p%32) * 4 + f%4
 * It is exactly the MFMA 32x32 accumulator layout with the point on the lane, so chain
 * kernels load/store it with fully coalesced 16-byte accesses.
 */
#ifndef NPF_HIP_H
#define NPF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPF_OK 0
#define NPF_EINVAL (-1)   /* bad argument / unsupported size           */
#define NPF_ELAUNCH (-2)  /* hipLaunch failed (hipGetLastError != 0)    */

#define NPF_MAX_OPS 40
#define NPF_MAX_FEATURES 512 /* widest activation a chain keeps in registers, forward and backward (programs that
                                stay <= 256 wide run the 2-workgroups-per-CU variants of the kernel) */

/* ---- chain programs ------------------------------------------------------------- */
enum npf_opcode {
  NPF_OP_END = 0,
  NPF_OP_LOAD_PT = 1,      /* cur <- PT32 tensor p0 (i0 = features F)                          */
  NPF_OP_STORE_PT = 2,     /* PT32 tensor p0 <- cur (i0 = F)                                   */
  NPF_OP_LOAD_ROWS = 3,    /* cur <- row-major p0 [task][pt][i0], i0 <= 32, zero padded        */
  NPF_OP_STORE_ROWS = 4,   /* row-major p0 [task][pt][i0] <- cur features < i0                 */
  NPF_OP_LINEAR = 5,       /* cur <- act(W cur + b [+ PT addend p2]); see npf_op_t fields       */
  NPF_OP_SOFTMAX = 6,      /* cur <- softmax over features < i0 of f0*cur.  i1 = 1: also store the
                              row statistics (max of cur, sum of exp(f0*(cur-max))) to
                              p0[task][pt][2]; i1 = 2: use the statistics stored in p0 instead
                              of the row's own (one block of a softmax over > 512 keys)          */
  NPF_OP_ADD_PT = 7,       /* cur <- cur + PT32 tensor p0 (i0 = F), optional relu (i1)          */
  NPF_OP_MASK_POS = 8,     /* cur <- (PT32 p0 > 0) ? cur : 0 (i0 = F)      [relu backward]      */
  NPF_OP_ADD_TASKVEC = 9,  /* cur <- cur + p0[task][i0 features] (row-major), optional relu (i1)*/
  NPF_OP_ROWDOT_PT = 10,   /* acc0 <- sum_f cur[f] * PT32 p0[f] (i0 = F)   [softmax bwd delta]  */
  NPF_OP_SOFTMAX_BWD = 11, /* cur <- f0 * P * (cur - acc0), P = PT32 p0 (i0 = F)                */
  NPF_OP_RELU = 12,        /* cur <- max(cur, 0)                                                */
  NPF_OP_SCALE = 13,       /* cur <- f0 * cur                                                   */
  NPF_OP_STORE_TR = 14,    /* row-major p0 [task][i0 features][i1 >= 32*tiles points] <- cur: a
                              feature-major copy, i.e. the activations as NPF_W_ROWMAJOR per-task
                              weights W[n = feature][k = point] (s0 = i0*i1, i3 = i1)            */
  NPF_OP_LAYERNORM = 15,   /* cur <- (cur - mean) / sqrt(var + f0) * p0[f] + p1[f] over the i0 <= 256
                              features of the point (nn.LayerNorm of TransformerAttender,
                              npf/architectures/attention.py:552-553,583-586); p0 (gamma), p1
                              (beta): 16-byte aligned, zero-padded to a multiple of 32 floats    */
  NPF_OP_STORE_WB = 18,    /* bf16 mode only: p0 [task][i1 >= 32*tiles rows][roundup(i0, 32)] bf16 <- cur, one row per
                              point, features k-permuted like npf_cast_bf16_weights: the activations as a
                              bf16 weight image W[n = point][k = feature] (per-task NPF_W_ROWMAJOR)         */
  NPF_OP_STORE_TRB = 19,   /* bf16 mode only: p0 [task][i0 features][i1 = 32*tiles columns] bf16 <- cur, the
                              transposed image W[n = feature][k = point], points k-permuted in groups of 32  */
  NPF_OP_LOAD_RM = 17,     /* cur <- row-major p0 [task][pt][i0], i0 % 32 == 0, i0 <= 512 (i4 = modulus)  */
  NPF_OP_STORE_MASK = 20,  /* bf16 mode only: PTM tensor p0 <- (cur > 0) as bits (i0 = F <= 256): the ReLU mask of the
                              backward pass -- one 32-bit word per point, lane group g = (feature / 4) % 4 and 128
                              features, [task][tile][ceil(F/128) words][4 g][32 points]; within a word the 16-feature
                              block bb = (feature / 16) % 8, element e = feature % 4 sits at bit 31 - (4 bb + e)        */
  NPF_OP_MASK_BITS = 21,   /* bf16 mode only: cur <- (bit of PTM tensor p0) ? cur : 0 (i0 = F)   [relu backward]      */
  NPF_OP_LAYERNORM_BWD = 16 /* cur = dy on entry; x = PT32 p0 (the forward input, i0 = F), gamma p1:
                              xhat = (x - mean) rstd;  PT32 p2 <- dy * xhat (for dgamma);
                              cur <- rstd (g - mean(g) - xhat mean(g xhat)),  g = dy * gamma      */
};

enum npf_wmode {
  NPF_W_ROWMAJOR = 0, /* W[n][k] at p0 + task*s0 + n*i3 (nn.Linear layout, i3 = row stride)   */
  NPF_W_PT_ROWS = 1,  /* W[n][k] = PT32 tensor p0 (features = k, points = n) of the WG's task:
                         the weights of q.k^T are the task's keys                              */
  NPF_W_PT_COLS = 2   /* W[n][k] = PT32 tensor p0 (features = n, points = k) of the WG's task:
                         the weights of attn.V are the task's values, transposed              */
};

#define NPF_F_RELU 1u
#define NPF_F_ADD_PT 2u /* add PT32 tensor p2 (same F as the output) before the activation     */
#define NPF_F_MASK_PT 4u /* out = (PT32 tensor p2 > 0) ? out : 0 (fused relu backward); not with ADD_PT */
#define NPF_F_P16 16u     /* bf16 mode only: the op's PT tensor (p0 of LOAD_PT / STORE_PT / ADD_PT / MASK_POS /
                            ROWDOT_PT / SOFTMAX_BWD, p2 of a LINEAR's addend or mask) is a PT16 tensor: bf16 tiles
                            [F/8 rows][32 points][8 features], row 4s+g = features {32s+4g+i}, {32s+16+4g+i}     */
#define NPF_F_MASK_BITS 32u /* bf16 mode only: like MASK_PT with the mask as bits, p2 = PTM tensor (NPF_OP_STORE_MASK)   */
#define NPF_F_ADD_RM 8u  /* like ADD_PT with a row-major addend p2 [task][pt][i1] (i1 % 32 == 0): module-
                            boundary tensors enter without a layout pass (inference paths)            */
#define NPF_F_STORE_IN 64u /* bf16 mode only. LINEAR: PT tensor p3 <- the layer's INPUT (i0 features), exactly what NPF_OP_STORE_PT in
                              front of the layer would store; the pipelined layers spread the stores over their stages
                              instead of bursting them between two layers                                       */
#define NPF_F_STORE_BITS 256u /* bf16 mode only. LINEAR with NPF_F_RELU and no addend / mask: PTM tensor p2 <- (output > 0) as
                                 bits, exactly what NPF_OP_STORE_MASK behind the layer would store (i1 <= 256)             */
#define NPF_F_STORE_P16 128u /* bf16 mode only, with NPF_F_STORE_IN: p3 is a PT16 tensor (see NPF_F_P16)                */

typedef struct npf_op {
  int32_t op;        /* npf_opcode                                                              */
  int32_t i0;        /* LINEAR: K (valid inputs)        others: see opcode                      */
  int32_t i1;        /* LINEAR: N (valid outputs)                                               */
  int32_t i2;        /* LINEAR: npf_wmode                                                       */
  int32_t i3;        /* LINEAR: row stride of W in floats (mode 0); tiles of the PT weight
                        tensor per task (modes 1, 2)                                            */
  uint32_t flags;    /* NPF_F_*                                                                 */
  float f0;          /* SOFTMAX / SOFTMAX_BWD / SCALE: scale                                    */
  int32_t i4;        /* *_PT ops and LINEAR addend: task modulus (0 = none): the tensor's task
                        index is task % i4 (broadcast of X_trgt over n_z samples)               */
  const void *p0;    /* LINEAR: W                        others: tensor                         */
  const void *p1;    /* LINEAR: bias or NULL                                                    */
  const void *p2;    /* LINEAR: PT32 addend or NULL                                             */
  int64_t s0;        /* LINEAR: per-task stride of W in floats (0 = shared)                     */
  int64_t s1;        /* LINEAR: per-task stride of bias in floats (0 = shared)                  */
  void *p3;          /* LINEAR with NPF_F_STORE_IN: destination of the input store              */
} npf_op_t;

typedef struct npf_program {
  int32_t n_ops;
  int32_t n_tasks;        /* tasks in the batch                                                 */
  int32_t pts_per_task;   /* valid points per task                                              */
  int32_t tiles_per_task; /* ceil(pts_per_task / 32)                                            */
  int32_t wg_per_task;    /* 1: every workgroup (4 tiles) stays inside one task (required by
                             per-task weights, modes 1/2); 0: tiles are dealt flat               */
  int32_t reserved[3];
  npf_op_t ops[NPF_MAX_OPS];
} npf_program_t;

/* Runs a chain program: every wavefront keeps the activations of one tile of 32 points in
 * registers (feature-major MFMA accumulator layout) across all ops; weights stream through
 * LDS.  Replaces the reference functions listed at the top of this file. */
int npf_chain_run(const npf_program_t *prog, void *stream);

/* The kernel instance npf_chain_run launches for a program (host code only, nothing is launched):
 * one of the values below, or NPF_EINVAL for a program npf_chain_run rejects. */
#define NPF_CHAIN_BF16 1    /* bf16 weight images (reserved[2] == 1): <16 blocks, 4 waves>, four-slot ring     */
#define NPF_CHAIN_EXTRA 2   /* a LayerNorm op: <16, 4> with the LayerNorm code, generic slab loop only          */
#define NPF_CHAIN_WIDE 3    /* a layer side or PT operand above 256 features: <32, 4>, generic slab loop only   */
#define NPF_CHAIN_PAIRED 4  /* reserved[1] == 2: <16, 8>, 128-point workgroups, three-slot ring, 256 -> 256     */
#define NPF_CHAIN_N128 5    /* more 128 -> 128 than 256 -> 256 layers: <16, 4> with the 128 -> 128 pipeline     */
#define NPF_CHAIN_DEFAULT 6 /* <16, 4> with the 256 -> 256 pipeline                                             */
int npf_chain_instance(const npf_program_t *prog);

/* ---- weight/bias gradients -------------------------------------------------------- */
/* One job: dW[n][k] (+)= sum_p dZ[n][p] * A[k][p] and db[n] (+)= sum_p dZ[n][p], where dZ and
 * A are PT32 tensors with roundup(N,32) / roundup(K,32) features over the same points.
 * per_task == 0: one dW (row-major, row stride ldw) for all points of all tasks, reduced
 *                over the workgroups through `partials` (deterministic, no atomics);
 * per_task == 1: one dW per task, written as a PT32 tensor whose *points* are n and whose
 *                features are k ([task][ceil(N/32) tiles][roundup(K,32)/4][32][4]): this is
 *                the gradient of attention keys / values; db is ignored. */
typedef struct npf_wgrad_job {
  const float *dZ;
  const float *A;
  float *dW;
  float *db;        /* may be NULL */
  int64_t ldw;      /* row stride of dW in floats (per_task == 0) */
  int32_t N, K;
  int32_t per_task;
  int32_t accumulate; /* bit 0: 0 = overwrite dW/db, 1 = add to them; bit 1 (NPF_WGRAD_BF16): round the
                         operands to bf16 at the MFMA input (bf16 compute mode; all jobs of a launch alike) */
  /* A job covers at most 256 x 256 of dW.  Wider layers (up to NPF_MAX_FEATURES = 512 features per side, the
   * reference's MLPs have no limit: npf/architectures/mlp.py:44-93) are run as several jobs on blocks of the
   * operands: dZ / A then point at the block's first feature inside the (wider) tensor and ldz / lda give the
   * features per tile of that tensor (0 = the job's own roundup(N, 32) / roundup(K, 32)); ldo likewise for the
   * PT32 output of a per-task job whose K is a block of a wider tensor. */
  int32_t ldz, lda, ldo;
  int32_t reserved;
} npf_wgrad_job_t;
#define NPF_WGRAD_ACCUMULATE 1
#define NPF_WGRAD_BF16 2
#define NPF_WGRAD_DZ16 4 /* with NPF_WGRAD_BF16: dZ is a PT16 tensor (bf16 tiles, see NPF_F_P16) */
#define NPF_WGRAD_A16 8  /* with NPF_WGRAD_BF16: A is a PT16 tensor */
/* fp32 result on the bf16 matrix pipe (all jobs of a launch alike, not with NPF_WGRAD_BF16): each fp32 operand is split
 * exactly into three bf16 terms and six of the nine cross products are accumulated in fp32 -- the dropped terms are
 * below 2^-26 of a product, i.e. under fp32 rounding; same operands, same result to summation-order noise, 6/16 of
 * the v_mfma_f32_16x16x4_f32 time (csrc/wgrad_kernel.hip, wgrad_x6_kernel). */
#define NPF_WGRAD_F32X6 16
/* with NPF_WGRAD_F32X6: keep wgrad_x6_kernel (every wave splits the fragments it reads) for this launch; default for launches whose
 * jobs are all 256 x 256 is wgrad_h16_kernel (every operand value split once per workgroup).  An A/B switch. */
#define NPF_WGRAD_NO_H16 32

#define NPF_MAX_WGRAD_JOBS 16
/* Runs up to NPF_MAX_WGRAD_JOBS jobs over the same points in ONE launch (+ one reduce). */
int npf_wgrad_run(const npf_wgrad_job_t *jobs, int32_t n_jobs, int32_t n_tasks, int32_t tiles_per_task,
                  float *partials, int64_t partials_bytes, void *stream);
/* Bytes of workspace npf_wgrad_run needs for these jobs (-1 on invalid arguments). */
int64_t npf_wgrad_partials_bytes(const npf_wgrad_job_t *jobs, int32_t n_jobs, int32_t n_tasks,
                                 int32_t tiles_per_task);

/* ---- Gaussian head ------------------------------------------------------------------ */
/* suff: row-major [n_rows][pts][2*dy] raw decoder output.  loc/scale: [n_rows][pts][dy].
 * scale = 0.01 + 0.99 softplus(raw) (base.py:116); homoskedastic != 0 pools scale over the
 * points of each row-task (base.py:356-362).  If Y != NULL (row-major [n_y_rows][pts][dy],
 * row r uses Y[r % n_y_rows]) also writes sum_logp[n_rows] = sum_t sum_dy log N(y|loc,scale)
 * (losses.py:18-24).  loc == scale == NULL: loss-only launch, only sum_logp is written (nothing of size
 * [n_rows][pts][dy] is materialised: the multi-sample objectives below only need sum_logp). */
int npf_gauss_head_fwd(const float *suff, int32_t n_rows, int32_t pts, int32_t dy, int32_t homoskedastic,
                       const float *Y, int32_t n_y_rows, float *loc, float *scale, float *sum_logp,
                       void *stream);
/* d_suff from (d_loc, d_scale, d_sum_logp): any of the three upstream gradients may be NULL.  loc == scale == NULL
 * (after a loss-only forward): they are recomputed from suff; d_loc and d_scale must then be NULL. */
int npf_gauss_head_bwd(const float *suff, const float *loc, const float *scale, int32_t n_rows, int32_t pts,
                       int32_t dy, int32_t homoskedastic, const float *Y, int32_t n_y_rows,
                       const float *d_loc, const float *d_scale, const float *d_sum_logp, float *d_suff,
                       void *stream);

/* Padded targets: row r owns the first n_valid[r % n_tasks] of its pts target rows.  n_valid is a DEVICE int32 [n_tasks] tensor the
 * kernels read (clamped to [0, pts]); n_rows % n_tasks == 0 and, with Y, n_y_rows % n_tasks == 0.  loc / scale / sum_logp and the
 * homoskedastic pooling (divided by the count) cover the rows below the count only and equal npf_gauss_head_fwd of the row cut to
 * them (bit for bit at full counts); rows beyond: loc = 0, scale = 1.  sum_logp of a row without targets is 0.  suff and Y beyond the
 * count are never read.  Otherwise the arguments of npf_gauss_head_fwd. */
int npf_masked_gauss_head_fwd(const float *suff, const int32_t *n_valid, int32_t n_tasks, int32_t n_rows, int32_t pts, int32_t dy,
                              int32_t homoskedastic, const float *Y, int32_t n_y_rows, float *loc, float *scale,
                              float *sum_logp, void *stream);
/* d_suff of the above: every row is written, the rows at and beyond the count as zeros (so nothing upstream -- decoder, attention,
 * x-encoder -- gets a gradient from padding); d_loc / d_scale beyond the count are not read. */
int npf_masked_gauss_head_bwd(const float *suff, const float *loc, const float *scale, const int32_t *n_valid, int32_t n_tasks,
                              int32_t n_rows, int32_t pts, int32_t dy, int32_t homoskedastic, const float *Y, int32_t n_y_rows,
                              const float *d_loc, const float *d_scale, const float *d_sum_logp, float *d_suff, void *stream);

/* Predictive summary (no reference counterpart: the reference leaves it to the caller's torch code).  Per task b, point t and output
 * dimension d the predictive distribution is the equal-weight mixture of the n_z Gaussians N(mu_k, sg_k^2) of the rows k * n_tasks + b
 * of suff ([n_z * n_tasks][pts][2 dy], what the decoder stores), mu / sg by the head's formulas above (homoskedastic: sg_k pooled over
 * the row's points).  One launch writes mean = 1/n_z sum_k mu_k, std = sqrt(1/n_z sum_k (sg_k^2 + (mu_k - mean)^2)) ([n_tasks][pts][dy]
 * each) and, with n_probs > 0, quant[n_probs][n_tasks][pts][dy]: quant[j] = x with 1/n_z sum_k Phi((x - mu_k) / sg_k) = probs[j],
 * solved by Newton steps safeguarded by bisection inside the bracket [min_k, max_k] of mu_k + sg_k z_p[j].  z_p[j] is the standard-
 * normal quantile of probs[j] (both DEVICE float [n_probs], computed by the caller).  Nothing of size [n_z][n_tasks][pts][dy] is
 * written.  1 <= n_z <= 128, dy <= 16, n_tasks <= 65535.  n_valid: NULL or a DEVICE int32 [n_tasks] tensor (clamped to [0, pts]):
 * task b owns its first n_valid[b] points, the pooling covers those, suff beyond is never read and the rows beyond get mean = 0,
 * std = 1, quant[j] = z_p[j] (loc = 0, scale = 1 of npf_masked_gauss_head_fwd); full counts equal the NULL launch bit for bit.
 * n_probs == 0: z_p, probs and quant may be NULL. */
int npf_mixture_summary(const float *suff, const int32_t *n_valid, int32_t n_z, int32_t n_tasks, int32_t pts, int32_t dy,
                        int32_t homoskedastic, const float *z_p, int32_t n_probs, const float *probs, float *mean, float *std,
                        float *quant, void *stream);

/* Scores of observations under the same mixture (the counterpart of npf_mixture_summary evaluated at y; no reference counterpart).
 * suff as above, Y[n_tasks][pts][dy].  With mu_k, sg_k the components of element (b, t, d), u_k = (y - mu_k) / sg_k and K = n_z, one
 * launch writes the outputs whose pointer is not NULL ([n_tasks][pts][dy] each; at least one must be given, a NULL one costs nothing):
 *   log_density = logsumexp_k(-u_k^2 / 2 - log sg_k - log sqrt(2 pi)) - log K   (maximum subtracted; a component at -inf has weight 0)
 *   pit         = 1/K sum_k Phi(u_k)                                             (Phi through erfc, on the side that does not cancel)
 *   crps        = 1/K sum_k A(y - mu_k, sg_k) - 1/(2 K^2) sum_{i,j} A(mu_i - mu_j, sqrt(sg_i^2 + sg_j^2)),
 *                 A(m, s) = 2 s phi(m / s) + m erf(m / (s sqrt 2));  the pair sum is evaluated as K (K - 1) / 2 off-diagonal terms
 *                 plus the diagonal 2 sg_i / sqrt(pi), its terms in fp32, their sum in double.
 * The scores are marginal per output dimension.  1 <= n_z <= 128, dy <= 16, n_tasks <= 65535, pts * dy <= 2^30.  n_valid: NULL or a
 * DEVICE int32 [n_tasks] tensor (clamped to [0, pts]): task b owns its first n_valid[b] points, the homoskedastic pooling covers
 * those, suff and Y beyond are never read and the rows beyond get log_density = 0, crps = 0 (a sum over the points needs no mask)
 * and pit = 0.5 (a PIT histogram must be masked by the counts).  A non-finite Y[b][t][d] reaches the outputs of that element only. */
int npf_mixture_score(const float *suff, const float *Y, const int32_t *n_valid, int32_t n_z, int32_t n_tasks, int32_t pts,
                      int32_t dy, int32_t homoskedastic, float *log_density, float *pit, float *crps, void *stream);

/* ---- Monte-Carlo objectives over the latent samples (npf/losses.py:126-276) ------------ */
/* log_w: row-major [n_z][n_tasks], the log weight of latent sample k for task b: sum_t log p(y_t | z_k), plus
 * log q(z_k | C) - log q(z_k | C, T) when the samples come from q(z | C, T).  out[n_tasks]:
 *   mode 0  mean_k log_w                                  (E_z of ELBOLossLNPF, losses.py:146)
 *   mode 1  logsumexp_k log_w - log n_z                   (NLLLossLNPF, losses.py:197-200)
 *   mode 2  SUMO (SUMOLossLNPF, losses.py:262-274): c_k = logsumexp_{j<=k} log_w_j - log(k+1) (k 0-based),
 *           out = c_{m-1} + sum_{k>=m} inv_weights[k] (c_k - c_{k-1}); inv_weights[n_z] = P(K >= k) of the
 *           number-of-samples distribution (host), m = the smallest number of samples it draws.
 * Running logsumexp per task: no [n_z][n_tasks] temporaries (and, with the loss-only Gaussian head above,
 * nothing of size [n_z][n_tasks][targets][dy]).
 * A sample with log_w = -inf (modes 1 and 2) is a term of weight 0 wherever it stands, the first sample included, and its
 * gradient is exactly 0, as with torch.logsumexp.  A task whose samples are ALL -inf is not covered: its result is unspecified. */
int npf_mc_objective_fwd(const float *log_w, int32_t n_z, int32_t n_tasks, int32_t mode, const float *inv_weights,
                         int32_t m, float *out, void *stream);
/* d_log_w[n_z][n_tasks] from d_out[n_tasks]; workspace: n_z * n_tasks floats (mode 2 only, else may be NULL). */
int npf_mc_objective_bwd(const float *log_w, int32_t n_z, int32_t n_tasks, int32_t mode, const float *inv_weights,
                         int32_t m, const float *d_out, float *d_log_w, float *workspace, void *stream);

/* ---- mean aggregation over the points of a task ------------------------------------- */
/* out[task][F] (row-major) = mean over valid points of PT32 tensor R (np.py:95). */
int npf_mean_agg_fwd(const float *R_pt, int32_t n_tasks, int32_t pts_per_task, int32_t F, float *out,
                     void *stream);
/* dR_pt[task][p][f] = d_out[task][f] / pts_per_task for valid points, 0 for padding. */
int npf_mean_agg_bwd(const float *d_out, int32_t n_tasks, int32_t pts_per_task, int32_t F, float *dR_pt,
                     int32_t accumulate, void *stream);

/* ---- layout ----------------------------------------------------------------------- */
/* rows: row-major [n_tasks][pts_per_task][F_valid]; pt: PT32 with F = roundup(F_valid, 32). */
int npf_pack_pt(const float *rows, int32_t n_tasks, int32_t pts_per_task, int32_t F_valid, float *pt,
                void *stream);
int npf_unpack_pt(const float *pt, int32_t n_tasks, int32_t pts_per_task, int32_t F_valid, float *rows,
                  void *stream);
/* dst[c][r] = src[r][c] for a row-major [rows][cols] matrix. */
int npf_transpose(const float *src, int32_t rows, int32_t cols, float *dst, void *stream);
/* Heads as tasks (MultiheadAttender._make_multiheaded / _concatenate_multiheads,
 * npf/architectures/attention.py:505-527) on PT32 tensors:
 *   split:  dst PT32 [n_heads*n_tasks][pts][F/n_heads]:  dst(h*n_tasks + b, p, f) = src(b, p, h*(F/n_heads) + f)
 *   merge:  the inverse (dst PT32 [n_tasks][pts][F]).  F % n_heads == 0 and (F/n_heads) % 4 == 0. */
int npf_split_heads(const float *src, int32_t n_tasks, int32_t pts_per_task, int32_t F, int32_t n_heads, float *dst,
                    void *stream);
int npf_merge_heads(const float *src, int32_t n_tasks, int32_t pts_per_task, int32_t F, int32_t n_heads, float *dst,
                    void *stream);

/* Multihead scaled-dot attention with 16- or 32-feature heads (D = F / n_heads), straight on the PT32 tensors of the K / Q / V projections
 * (MultiheadAttender.forward between the projections and the concatenation, npf/architectures/attention.py:505-527 with
 * DotAttender :204-220 per head, scale 1 / sqrt(head size)): out(b, q, D h + :) = softmax_k(Q_h K_h^T / sqrt(D)) V_h, X_h = features
 * D h .. D h + D - 1.  q / out: PT32 [n_tasks][n_queries][F], k / v: PT32 [n_tasks][n_keys][F], F = D n_heads (tiles of
 * roundup(F, 32) features), n_keys <= 256 (D = 16) or 128 (D = 32).  lse [n_tasks][n_heads][n_queries] (or NULL at inference): log-sum-exp of the scaled
 * scores, what the backward pass recomputes the probabilities from.  fp32 MFMA, softmax with max subtraction.
 * npf_mha_bwd: d_q / d_k / d_v (PT32, same shapes as q / k / v; points and features outside the valid ranges are not written). */
int npf_mha_fwd(const float *q, const float *k, const float *v, int32_t n_tasks, int32_t n_heads, int32_t n_keys,
                int32_t n_queries, int32_t F, float *out, float *lse, void *stream);
int npf_mha_bwd(const float *q, const float *k, const float *v, const float *out, const float *d_out, const float *lse,
                int32_t n_tasks, int32_t n_heads, int32_t n_keys, int32_t n_queries, int32_t F, float *d_q, float *d_k, float *d_v,
                void *stream);

/* y = LayerNorm(a + b) over the F features of every point (F % 4 == 0, F <= 256), PT32 tensors [n_tasks][pts_per_task][F]:
 * TransformerAttender.forward's layer_norm1(context + queries) (npf/architectures/attention.py:566-575; nn.LayerNorm: biased
 * variance, eps inside the root, gamma / beta [F]).  stats [n_tasks * tiles * 32][2] = (mean, 1 / std) per point, or NULL at inference.
 * npf_add_layernorm_bwd: dx (the gradient of a and of b alike; zero at the padding points) and partials [n_tasks * tiles][2][F] = the
 * tile's sums of dy * xhat and of dy, which the caller adds up over the tiles to dgamma and dbeta.
 * Padding points (p >= pts_per_task inside the last tile of a task): every point is normalised on its own, and in the backward pass
 * nothing read at a padding point -- a, b, stats, dy -- reaches dx, the partials or another point: whatever they hold there, NaN
 * included, has no influence.  (y and stats AT the padding points are whatever the arithmetic makes of a and b there.) */
int npf_add_layernorm_fwd(const float *a, const float *b, const float *gamma, const float *beta, float eps, int32_t n_tasks,
                          int32_t pts_per_task, int32_t F, float *y, float *stats, void *stream);
int npf_add_layernorm_bwd(const float *a, const float *b, const float *gamma, const float *stats, const float *dy, int32_t n_tasks,
                          int32_t pts_per_task, int32_t F, float *dx, float *partials, void *stream);

/* Context / target selection (CntxtTrgtGetter.select, npf/utils/datasplit.py:246-255: torch.gather along
 * the points of X and y with the same indices): out_x[b][i][:] = x[b][idx[b][i]][:], same for y.
 * idx: int64 [n_tasks][n_sel], every entry in [0, n_points) (checked on the host side). */
int npf_gather_points(const float *x, const float *y, const int64_t *idx, int32_t n_tasks, int32_t n_points,
                      int32_t n_sel, int32_t x_dim, int32_t y_dim, float *out_x, float *out_y, void *stream);

/* bf16 compute mode of the chain kernel (prog->reserved[2] == 1): every LINEAR op takes, instead of fp32
 * weights, the bf16 image this function writes -- dst [rows][roundup(cols, 32)] bf16, columns permuted
 * inside each group of 32 (position 8g+i <- column 4g+i, position 8g+4+i <- column 16+4g+i), zero
 * padded -- with p0 = dst, i3 = roundup(K, 32) / 2 (row stride in floats), NPF_W_ROWMAJOR.  Activations
 * are rounded to bf16 at the MFMA input, accumulation / bias / epilogue / HBM tensors stay fp32.
 * transposed != 0: the image of src^T (rows = columns of src), for the dgrad chains. */
int npf_cast_bf16_weights(const float *src, int32_t n_rows, int32_t n_cols, int32_t ld, int32_t transposed, void *dst,
                          void *stream);

/* Batched weight preparation: up to NPF_MAX_WPREP_JOBS of the two functions above in ONE launch (a chain's
 * dgrad needs W^T -- or, in the bf16 mode, an image -- of every layer; one 5 us launch per layer otherwise).
 * kind: 0 = fp32 transpose (as npf_transpose, src row stride ld), 1 = bf16 image, 2 = bf16 image of src^T;
 * 1 / 2 + 16 t, t = 1..3: the same image of term t - 1 of the exact three-term split of src (x0 = bf16(x), x1 = bf16(x - x0),
 * x2 = bf16(x - x0 - x1)) -- the weights of npf_mlp_x6_run;
 * 5 / 6 = kinds 1 / 2 with every image row zero-padded to 256 inputs (a layer with <= 32 real inputs whose remaining
 * input registers are known to be zero then runs as a 256-input layer on the pipelined path). */
typedef struct npf_wprep_job {
  const float *src; /* row-major [n_rows][n_cols], row stride ld floats */
  void *dst;        /* kind 0: float [n_cols][n_rows]; kind 1 / 2: bf16 image, 16-byte aligned */
  int32_t n_rows, n_cols, ld, kind;
} npf_wprep_job_t;
#define NPF_MAX_WPREP_JOBS 32
int npf_prepare_weights(const npf_wprep_job_t *jobs, int32_t n_jobs, void *stream);

/* Library / device info. */
/* ---- hidden layers of the flat MLPs with their fp32 products on the bf16 matrix pipe ----------------------------------
 * Replaces, for stacks of 256 -> 256 layers, what npf_chain_run does with LINEAR ops (npf/architectures/mlp.py:95-109 forward;
 * its autograd backward): cur <- x; per layer: [cur <- mask > 0 ? cur : 0] [store_in <- cur] cur <- W cur + bias [+ addend] [relu]
 * [store_out <- cur]; y <- cur.  x, y, mask, store_in, store_out: PT32 tensors with 256 features over n_tasks x tiles_per_task
 * tiles.  w_img: the layer's weights as THREE bf16 terms, W = W0 + W1 + W2 exactly to 2^-27 (W0 = bf16(W), W1 = bf16(W - W0),
 * W2 = bf16(W - W0 - W1)), each a 256 x 256 k-permuted image as npf_cast_bf16_weights makes it, stored back to back; the kernel
 * splits the layer input the same way in registers and accumulates six of the nine cross products in fp32 (the dropped ones
 * are below 2^-26 of a product): an fp32 result, at 6/16 of the fp32-MFMA time (csrc/mlp_x6_kernel.hip).
 * Forward pass of a stack: bias, relu, store_out (the saved activations) per layer.  Its dgrad: layers in reverse order with
 * w_img = the images of W^T, mask = the layer's saved output, store_in = the dZ buffer the weight gradient reads. */
#define NPF_X6_MAX_LAYERS 8
typedef struct {
  const void *w_img;   /* [3][256][256] bf16 */
  const float *bias;   /* [256] or NULL */
  const float *mask;   /* PT32 or NULL */
  float *store_in;     /* PT32 or NULL */
  float *store_out;    /* PT32 or NULL */
  const float *addend; /* PT32 or NULL: added before the ReLU (MergeFlatInputs: relu(x1 + resizer(x2)), encoders.py:178-179) */
  /* where the layer's output is positive, as bits: one uint64 per lane and half tile ([tiles][2][64], bit 4 b + e = the
   * lane's block b, element e) -- written by a forward layer (store_bits), read by the dgrad of the same layer (mask_bits)
   * in place of `mask`: 8 bytes per 64 values */
  unsigned long long *store_bits;
  const unsigned long long *mask_bits;
  int32_t relu;
  int32_t reserved;
} npf_x6_layer_t;
int npf_mlp_x6_run(const npf_x6_layer_t *layers, int32_t n_layers, const float *x, float *y, int32_t n_tasks,
                   int32_t tiles_per_task, void *stream);
/* The same with a 256 -> 4 layer on either side of the stack (the decoder's output layer, npf/architectures/mlp.py:109), as rows
 * [n_tasks * tiles_per_task * 32][4] row-major and a [4][256] fp32 matrix, in plain fp32 FMAs:
 *  - in front (x == NULL): x[point][f] = sum_n in_rows[point][n] in_w[n][f] -- the dgrad of that layer ahead of the dgrad of
 *    the stack (in_rows = dOut as the Gaussian head's backward leaves it, in_w = W_out): the 256-wide gradient is never
 *    written to or read from HBM;
 *  - behind (out_rows != NULL): out_rows[point][n] = sum_f out_w[n][f] cur[f] + out_b[n] from the registers the last layer
 *    leaves (forward; y may be NULL when the stack's own output is not needed). */
int npf_mlp_x6_run_rows(const npf_x6_layer_t *layers, int32_t n_layers, const float *x, const float *in_rows, const float *in_w,
                        float *y, const float *out_w, const float *out_b, float *out_rows, int32_t n_tasks,
                        int32_t tiles_per_task, void *stream);

/* ---- x6 programs: whole sides of the model as ONE launch on the bf16 matrix pipe, fp32 results -------------------------
 * The generalisation of npf_mlp_x6_run: a straight-line program of up to NPF_X6_MAX_OPS ops on the register-resident activation
 * `cur` of every point (width F = 128 or 256 features, PT32 tensors with exactly F features), every multiply an fp32 product
 * as six bf16 products of exact three-term splits (see above).  Besides the shared-weight layers of the flat MLPs
 * (npf/architectures/mlp.py:95-109) an op can
 *  - take PER-TASK weights (w_task_stride != 0): the task's keys / values as three-term images (npf_x6_task_images) -- the two
 *    contractions of DotAttender (npf/architectures/attention.py:204-220 scores, :151 attn . values) and of its backward;
 *  - apply the softmax of attention.py:158-164 to its result (softmax_n keys, in registers, wavefront shuffles), or the softmax
 *    backward to its input (sbwd_p);
 *  - form its input from [points][4] rows through a [4][in_n] matrix (+ bias, ReLU): the first layer of the x-encoder and of
 *    the XY-encoder's resizer (Linear(1 -> r), Linear(2 -> 32); mlp.py:96) at no HBM traffic, or the dgrad of a 256 -> 4 layer;
 *  - run without a multiply (w_img == NULL): an elementwise step (mask + store: the end of a dgrad chain).
 * Per op, in this order:
 *   input side   cur <- in_pt                           (a new PT32 input; else cur = the previous op's result)
 *                cur <- [relu](in_w^T rows + in_b)      (in_rows; features >= in_n are zero)
 *                cur += pre_add                         (PT32)
 *                cur <- mask > 0 ? cur : 0              (mask: PT32; mask_bits: one uint64 per lane and half tile, see below)
 *                cur <- sbwd_scale * P * (cur - <cur, P>)   (sbwd_p = P, PT32)
 *                store_in <- cur (PT32);  store_in_bits <- (cur > 0)
 *   multiply     cur <- W cur + bias                    (w_img: [3][F][F] bf16 three-term image, + task * w_task_stride BYTES;
 *                                                        bias [F] or NULL, + task * bias_task_stride floats)
 *   output side  cur += addend (PT32);  relu;  softmax over the first softmax_n features of softmax_scale * cur;
 *                store_out <- cur (PT32);  store_bits <- (cur > 0)
 * Bit tensors: [n_tasks * tiles_per_task][2][64] uint64, bit 4 b + e of lane (p, g) = feature 16 b + 4 g + e of point p of
 * the half tile.  Rows tensors: [n_tasks * tiles_per_task * 32][4] (the points of a task fill whole tiles). */
#define NPF_X6_MAX_OPS 12
typedef struct npf_x6_op {
  const float *in_pt;
  const float *in_rows;
  const float *in_w;
  const float *in_b;
  const float *pre_add;
  const float *mask;
  const unsigned long long *mask_bits;
  const float *sbwd_p;
  float *store_in;
  unsigned long long *store_in_bits;
  const void *w_img;
  int64_t w_task_stride;
  const float *bias;
  int64_t bias_task_stride;
  const float *addend;
  float *store_out;
  unsigned long long *store_bits;
  int32_t in_n;        /* outputs of the rows prologue (a multiple of 16, <= F) */
  int32_t in_relu;
  int32_t relu;
  int32_t softmax_n;   /* 0 = no softmax */
  float softmax_scale;
  float sbwd_scale;
  int32_t reserved[2]; /* [0]: op flags (NPF_X6_IN_RM ...); [1]: 0 */
} npf_x6_op_t;
/* op flags (reserved[0]): in_pt / addend are ROW-MAJOR [n_tasks][pts_per_task][F] tensors -- what the reference's decode(X_trgt_enc,
 * R_trgt) is handed (npf/neuralproc/base.py:327) -- read without a layout pass (inference inputs: no gradient flows into them) */
#define NPF_X6_IN_RM 1
#define NPF_X6_ADD_RM 2
/* npf_b16_run only: store_in / store_out take the fp32 value as a PT32 tensor (default there: bf16(value) as a PT16 tensor) */
#define NPF_X6_STORE_IN_F32 4
#define NPF_X6_STORE_OUT_F32 8
/* 256-feature programs, the library's choice of kernel instance (npf_x6_run_ex variant 0): 1 = 16 points per wave, four waves per
 * workgroup, two workgroups per CU; 2 = 32 points per wave (one wave per SIMD, every weight fragment feeds twice the matrix
 * instructions); 3 = 16 points per wave, EIGHT waves per workgroup sharing one slab ring (a CU streams every slab once) */
#define NPF_X6_DEFAULT_VARIANT 3
/* out_rows != NULL: a F -> 4 layer behind the program, out_rows[point][n] = sum_f out_w[n][f] cur[f] + out_b[n] (the decoder's
 * output layer, mlp.py:109).  per_task != 0: every workgroup stays inside one task (required by per-task weights / biases).
 * width: 128 or 256. */
/* npf_x6_run_ex: the same with pts_per_task valid points per task (<= 32 tiles_per_task; row-major operands are indexed with it),
 * width 128, 256 or 512 (512: no ReLU-bit operands -- inference programs, e.g. the r = 512 decoder of base.py:327-367 from
 * row-major inputs), and variant = 0 (library's choice) | 1 | 2 | 3: width 256 see NPF_X6_DEFAULT_VARIANT above; width 512: 1 = a wave
 * holds all 512 features of its 16 points (one wave per SIMD), 0 / 2 = the contraction split over pairs of waves through LDS
 * (two waves per SIMD; programs of plain layers -- inputs, multiply, bias / addend / ReLU, stores -- only; others take 1). */
int npf_x6_run_ex(const npf_x6_op_t *ops, int32_t n_ops, const float *out_w, const float *out_b, float *out_rows,
                  int32_t n_tasks, int32_t tiles_per_task, int32_t pts_per_task, int32_t per_task, int32_t width,
                  int32_t variant, void *stream);
int npf_x6_run(const npf_x6_op_t *ops, int32_t n_ops, const float *out_w, const float *out_b, float *out_rows,
               int32_t n_tasks, int32_t tiles_per_task, int32_t per_task, int32_t width, void *stream);
/* The three-term images of a PT32 tensor src [n_tasks][tiles_per_task][F/4][32][4] taken as per-task weights, F = width:
 *   row_img [n_tasks][3][F][F] bf16: W[n = point][k = feature]   (scores = K q, dP = V dO), points >= pts are zero rows;
 *   tr_img  [n_tasks][3][F][F] bf16: W[n = feature][k = point]   (attn . V, dq = K^T dS), points >= pts are zero columns;
 * both k-permuted like npf_cast_bf16_weights.  pts <= F points per task.  Either destination may be NULL. */
int npf_x6_task_images(const float *src, int32_t n_tasks, int32_t pts, int32_t width, void *row_img, void *tr_img, void *stream);

/* ---- b16 programs: the same programs in the bf16 compute mode (BASELINE config 3) ------------------------------------------
 * npf_x6_op_t programs of width 128 or 256 with ONE bf16 product per multiply, fp32 accumulation: the input of every multiply is
 * rounded to bf16 (nearest even), w_img is a ONE-term image [F][F] bf16 (npf_prepare_weights kinds 1 / 2; npf_b16_task_images for
 * the task's keys / values), bias / addend / ReLU / softmax in fp32 -- the arithmetic of the bf16 chain instance
 * (npf/architectures/mlp.py:95-109, attention.py:129-164 with the rounding points DESIGN.md 4 lists).  Differences to npf_x6_run:
 *   store_in / store_out  <- bf16(cur) as a PT16 tensor [tiles][F/8][32][8] (see NPF_F_P16) -- what only the weight-gradient launch
 *                            reads -- unless NPF_X6_STORE_IN_F32 / NPF_X6_STORE_OUT_F32 asks for the fp32 value as a PT32 tensor;
 *   sbwd_p                =  a PT16 tensor (the saved probabilities are bf16 values);
 *   in_rows prologue / the F -> 4 layer behind the program: fp32 FMAs; the caller hands bf16-ROUNDED rows and matrices, the
 *                            F -> 4 layer rounds its input itself;
 *   mask (PT32), row-major operands: not available.
 * Whole tiles only (pts_per_task = 32 tiles_per_task).  variant: 0 = the library's choice (1), 1 = eight waves per workgroup on one
 * ring of three 64-row slabs (one workgroup per CU), 2 = four waves and three 32-row slabs (two workgroups per CU). */
int npf_b16_run(const npf_x6_op_t *ops, int32_t n_ops, const float *out_w, const float *out_b, float *out_rows, int32_t n_tasks,
                int32_t tiles_per_task, int32_t per_task, int32_t width, int32_t variant, void *stream);
/* npf_x6_task_images with the rounded value alone: row_img / tr_img [n_tasks][F][F] bf16. */
int npf_b16_task_images(const float *src, int32_t n_tasks, int32_t pts, int32_t width, void *row_img, void *tr_img, void *stream);

/* ---- padded contexts: per-task counts as device data (csrc/masked_kernels.hip) -------------------------------------------
 * The batch holds n_keys (attention) / pts_per_task (mean) context rows per task, of which the first n_valid[task] are real:
 * n_valid is a DEVICE int32 [n_tasks] tensor the kernels read (values outside [0, n_keys] are clamped there), the host never
 * does -- the launch can sit in a captured graph and see new counts at every replay.  What the rows beyond the count hold
 * (NaN included) has no influence on any result.
 *
 * Scaled-dot attention of n_queries queries over the first n_valid[task] keys of every task (DotAttender.forward on the batch cut
 * per task, npf/architectures/attention.py:129-164,204-220):
 *   out(b, q, :) = sum_{k < n_valid[b]} softmax_{k < n_valid[b]}(scale <Q(b,q,:), K(b,k,:)>) V(b,k,:),   0 if n_valid[b] == 0.
 * q / out: PT32 [n_tasks][n_queries][d], k / v: PT32 [n_tasks][n_keys][d] (tiles of roundup(d, 32) features), d % 4 == 0, d <= 256, any
 * n_keys: the keys are walked in blocks with an online softmax, blocks wholly beyond the count are skipped.  Multihead attention:
 * the heads as extra tasks (npf_split_heads: task h * n_tasks + b) with n_valid repeated per head.  lse [n_tasks][n_queries] (or NULL at
 * inference): log-sum-exp of the scaled scores over the real keys (0 where there is none), what the backward pass recomputes the
 * probabilities from.  fp32 MFMA.  Every element of out (whole tiles) is written.
 * npf_masked_attn_bwd: d_q / d_k / d_v (PT32, shapes of q / k / v, every element written); rows k >= n_valid[b] of d_k / d_v are exact
 * zeros, and so is d_q where n_valid[b] == 0.
 * Status: NPF_EINVAL (nothing launched) for d % 4 != 0, d > 256 or a negative count of tasks / keys / queries. */
int npf_masked_attn_fwd(const float *q, const float *k, const float *v, const int32_t *n_valid, int32_t n_tasks, int32_t n_keys,
                        int32_t n_queries, int32_t d, float scale, float *out, float *lse, void *stream);
int npf_masked_attn_bwd(const float *q, const float *k, const float *v, const int32_t *n_valid, const float *out, const float *d_out,
                        const float *lse, int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float *d_q,
                        float *d_k, float *d_v, void *stream);
/* The same with a count of real QUERIES per task as well (padded targets): n_q_valid is a DEVICE int32 [n_tasks] tensor, clamped to
 * [0, n_queries]; with heads as extra tasks the caller repeats it per head like n_valid.  Rows q >= n_q_valid[b] of out / d_q are
 * exact zeros (lse = 0) and q / out / d_out / lse beyond the count are never read; workgroups wholly beyond it return before they
 * stage a key, and the walk of the d_k / d_v kernel over the queries ends at the count.  The rows below the counts are bit-identical
 * to npf_masked_attn_fwd / _bwd on the same tensors (with d_out zeroed beyond the query count): same block and summation order. */
int npf_masked_attn_fwd_nq(const float *q, const float *k, const float *v, const int32_t *n_valid, const int32_t *n_q_valid,
                           int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float *out, float *lse,
                           void *stream);
int npf_masked_attn_bwd_nq(const float *q, const float *k, const float *v, const int32_t *n_valid, const int32_t *n_q_valid,
                           const float *out, const float *d_out, const float *lse, int32_t n_tasks, int32_t n_keys, int32_t n_queries,
                           int32_t d, float scale, float *d_q, float *d_k, float *d_v, void *stream);
/* A shared prefix and an own tail (inference only, no backward): n_tasks = S * n_prefix_tasks tasks, task j attends over the first
 * n_prefix[j % n_prefix_tasks] rows of PREFIX task j % n_prefix_tasks (k_pre / v_pre: PT32 [n_prefix_tasks][c_pad][d]) followed by the
 * first n_tail[j] rows of its own tail (k_tail / v_tail: PT32 [n_tasks][m_tail][d]):
 *   out(j, q, :) = softmax(scale <Q(j,q,:), [K_pre(j % P, :n_prefix); K_tail(j, :n_tail)]>) [V_pre; V_tail],   0 if both counts are 0.
 * S function samples of one conditioned context read it from one copy.  n_prefix [n_prefix_tasks] / n_tail [n_tasks]: DEVICE int32,
 * clamped to [0, c_pad] / [0, m_tail], never read by the host.  n_q_valid [n_tasks]: as in npf_masked_attn_fwd_nq, or NULL.  The key
 * blocks of the prefix are walked first, then those of the tail, each segment ending as the single one of npf_masked_attn_fwd does;
 * with every n_tail == 0 and S == 1 the result is bit-identical to npf_masked_attn_fwd on the prefix.  With heads as extra tasks the
 * caller orders them sample-major (task s * (B H) + h * B + b over a prefix split by npf_split_heads).  Every element of out (whole
 * tiles) is written.  Status: NPF_EINVAL (nothing launched) for d % 4 != 0, d > 256, n_prefix_tasks <= 0, n_tasks % n_prefix_tasks != 0
 * or a negative size. */
int npf_masked_attn_fwd_prefix(const float *q, const float *k_pre, const float *v_pre, const int32_t *n_prefix, const float *k_tail,
                               const float *v_tail, const int32_t *n_tail, const int32_t *n_q_valid, int32_t n_tasks,
                               int32_t n_prefix_tasks, int32_t c_pad, int32_t m_tail, int32_t n_queries, int32_t d, float scale,
                               float *out, void *stream);
/* Leave-one-out (inference only, no backward, no lse): npf_masked_attn_fwd_nq in which query row t of a task never meets key row t
 * of that task (row numbers inside the task; q and k / v stay separate tensors):
 *   out(b, t, :) = sum_{k < n_valid[b], k != t} softmax_{k < n_valid[b], k != t}(scale <Q(b,t,:), K(b,k,:)>) V(b,k,:)
 * for t < n_q_valid[b], exact zeros for a query without any such key (n_valid[b] <= 1 with t = 0, n_valid[b] == 0) and beyond the
 * query count.  With q = k = the encoded context points and v = their representations this is, for every context point, the
 * attention of that point over the OTHER points of its task.  v(b, t, :) has no influence on out(b, t, :), whatever it holds (Inf /
 * NaN included: the own row's product is not formed).  n_q_valid: DEVICE int32 [n_tasks] as in npf_masked_attn_fwd_nq, or NULL (all
 * n_queries rows are real).  Same key blocks, fp32 MFMA roles and online softmax as npf_masked_attn_fwd; the results are
 * deterministic.  Every element of out (whole tiles) is written.  Status: as npf_masked_attn_fwd. */
int npf_masked_attn_fwd_loo(const float *q, const float *k, const float *v, const int32_t *n_valid, const int32_t *n_q_valid,
                            int32_t n_tasks, int32_t n_keys, int32_t n_queries, int32_t d, float scale, float *out, void *stream);
/* out[task][F] (row-major) = mean over the first n_valid[task] points of PT32 tensor R (F % 32 == 0), zeros if n_valid[task] == 0
 * (torch.mean(R_cntxt, dim=1) on the batch cut per task, np.py:95, attnnp.py:181); tiles beyond the count are not read. */
int npf_masked_mean_fwd(const float *R_pt, const int32_t *n_valid, int32_t n_tasks, int32_t pts_per_task, int32_t F, float *out,
                        void *stream);
/* dR_pt[task][p][f] (+)= d_out[task][f] / n_valid[task] for p < n_valid[task], 0 beyond (accumulate as npf_mean_agg_bwd). */
int npf_masked_mean_bwd(const float *d_out, const int32_t *n_valid, int32_t n_tasks, int32_t pts_per_task, int32_t F, float *dR_pt,
                        int32_t accumulate, void *stream);
/* Leave-one-out means (inference only): out (PT32 [n_tasks][pts_per_task][F], every element written) row i < n_valid[task] =
 * (sum over the task's first n_valid[task] rows of R_pt - row i) / (n_valid[task] - 1); zeros for i >= n_valid[task] and where
 * n_valid[task] <= 1.  The per-task sum is taken inside the launch in the summation order of npf_masked_mean_fwd; tiles beyond the
 * count are not read. */
int npf_loo_mean(const float *R_pt, const int32_t *n_valid, int32_t n_tasks, int32_t pts_per_task, int32_t F, float *out,
                 void *stream);
/* Reweighted contexts (inference only, no backward, no lse): n_tasks = S * n_ctx_tasks replicates of ONE stored copy of the context.
 * Task j reads the queries (q: PT32 [n_ctx_tasks][n_queries][d], shared by the replicates), keys, values and counts (n_valid /
 * n_q_valid: DEVICE int32 [n_ctx_tasks], n_q_valid may be NULL) of context task j % n_ctx_tasks -- the rule of
 * npf_masked_attn_fwd_prefix -- and row j of w (row-major [n_tasks][n_keys], fp32, on the device): a weight per key.  Key k of task j
 * is admissible iff k < n_valid[j % n_ctx_tasks] and 0 < w[j][k] < +inf (a weight that is 0, negative, NaN or Inf removes the key):
 *   out(j, q, :) = sum_adm w_k exp(scale <Q, K_k>) V_k / sum_adm w_k exp(scale <Q, K_k>),    out: PT32 [n_tasks][n_queries][d],
 * exact zeros for a query without an admissible key and beyond n_q_valid.  An integer weight is "the point appears w times": the
 * result is that of npf_masked_attn_fwd on the context with its rows repeated.  The K / V rows of an inadmissible key never meet a
 * multiply, whatever they hold.  The running maximum is over scale <Q, K_k> + log w_k of the admissible keys of the replicate alone.
 * With every weight 1.0 and S = 1 the result is BIT-IDENTICAL to npf_masked_attn_fwd_nq (npf_masked_attn_fwd with n_q_valid NULL) on
 * the same tensors: the same key blocks, summation order and online softmax.  The host never reads w or the counts: the launch sits in
 * a captured graph and sees new weights at every replay.  Deterministic; every element of out (whole tiles) is written.  With heads
 * as extra tasks the caller orders them replicate-major (task s * (B H) + h * B + b) over keys / values split by npf_split_heads.
 * Status: NPF_EINVAL (nothing launched) for d % 4 != 0, d > 256, n_ctx_tasks <= 0, n_tasks % n_ctx_tasks != 0, a negative size or
 * misaligned pointers. */
int npf_masked_attn_fwd_weighted(const float *q, const float *k, const float *v, const float *w, const int32_t *n_valid,
                                 const int32_t *n_q_valid, int32_t n_tasks, int32_t n_ctx_tasks, int32_t n_keys, int32_t n_queries,
                                 int32_t d, float scale, float *out, void *stream);
/* out[j][F] (row-major, as npf_masked_mean_fwd; F % 32 == 0) = sum_adm w[j][k] R(j % n_ctx_tasks, k, :) / sum_adm w[j][k] over the
 * admissible points (as above) of context task j % n_ctx_tasks of PT32 tensor R_pt [n_ctx_tasks][pts_per_task][F]; zeros where the
 * admissible weights sum to 0.  w: row-major [n_tasks][pts_per_task].  Tiles beyond the count and rows without weight are not read.
 * Sums and the division are held in double in a fixed order: one rounding, and a second launch gives the same bits. */
int npf_weighted_mean(const float *R_pt, const float *w, const int32_t *n_valid, int32_t n_tasks, int32_t n_ctx_tasks,
                      int32_t pts_per_task, int32_t F, float *out, void *stream);

/* ---- training through key weights: the log-sum-exp of the weighted forward pass, and the gradients (csrc/masked_kernels.hip,
 * csrc/layout_kernels.hip) ----------------------------------------------------------------------------------------------------
 * npf_masked_attn_fwd_weighted_ex: the arguments and the result of npf_masked_attn_fwd_weighted (out is bit-identical) plus
 * lse (row-major [n_tasks][n_queries], every element written, must not be NULL):
 *   lse(j, q) = log sum_adm w_k exp(scale <Q_q, K_k>)    (the walk's running maximum + log of its running sum),
 * 0 for a query without an admissible key or at / beyond n_q_valid. */
int npf_masked_attn_fwd_weighted_ex(const float *q, const float *k, const float *v, const float *w, const int32_t *n_valid,
                                    const int32_t *n_q_valid, int32_t n_tasks, int32_t n_ctx_tasks, int32_t n_keys,
                                    int32_t n_queries, int32_t d, float scale, float *out, float *lse, void *stream);
/* The backward pass of npf_masked_attn_fwd_weighted_ex at ONE replicate (n_tasks == n_ctx_tasks: task j reads its own q / k / v /
 * counts and row j of w).  out, lse: what the forward call wrote; d_out: PT32 like out.  With
 *   a_qk = scale <q_q, k_k> + log w_k,   p_qk = exp(a_qk - lse_q),   D_q = <d_out_q, out_q>,   dA_qk = p_qk (<d_out_q, v_k> - D_q)
 * over the admissible keys (k < n_valid[j] and 0 < w_k < +inf) and the queries below n_q_valid[j] (NULL: all):
 *   d_q(q) = scale sum_k dA_qk k_k      d_k(k) = scale sum_q dA_qk q_q      d_v(k) = sum_q p_qk d_out_q
 *   d_w(k) = (sum_q dA_qk) / w_k        (d a_qk / d w_k = 1 / w_k;  d_w: row-major [n_tasks][n_keys])
 * d_q, d_k, d_v: PT32 like q, k, v.  Every element of the four outputs is written (whole tiles): the caller needs no memset.
 * An inadmissible key -- at or beyond the count, or with a weight that is 0, negative, NaN or Inf -- never meets a multiply, whatever
 * its K / V rows and its weight hold, and gets d_k = d_v = d_w = 0 EXACTLY: a removed point is removed, there is no one-sided
 * derivative at w = 0.  Queries at / beyond n_q_valid are never read and get d_q = 0; a query without an admissible key contributes
 * nothing.  At w = 1 everywhere, d_w(k) of a scalar loss is the infinitesimal jackknife: how much the loss changes per unit of
 * extra weight on point k.  No atomics: the sums over keys and queries have a fixed order, a second launch gives the same bits.
 * The host never reads w or the counts.  Status: NPF_EINVAL for d % 4 != 0, d > 256, a negative size, a NULL or misaligned pointer. */
int npf_masked_attn_bwd_weighted(const float *q, const float *k, const float *v, const float *w, const int32_t *n_valid,
                                 const int32_t *n_q_valid, const float *out, const float *d_out, const float *lse, int32_t n_tasks,
                                 int32_t n_keys, int32_t n_queries, int32_t d, float scale, float *d_q, float *d_k, float *d_v,
                                 float *d_w, void *stream);
/* The backward pass of npf_weighted_mean at ONE replicate (n_tasks == n_ctx_tasks).  out: what the forward call wrote, d_out:
 * row-major [n_tasks][F] like out.  With W = the sum of the task's admissible weights:
 *   dR_pt(j, k, :) = (w_k / W) d_out(j, :)          dw(j, k) = <d_out(j, :), R(j, k, :) - out(j, :)> / W
 * for the admissible points; exact zeros for the others and for a task with W = 0 (no one-sided derivative at w = 0).  dR_pt: PT32
 * like R_pt, dw: row-major [n_tasks][pts_per_task]; every element of both is written.  W is summed in the forward pass's order;
 * quotients, products, the scalar product and the division are held in double in a fixed order with one rounding per stored value.
 * The mean in dw is summed again in double and subtracted unrounded (out, rounded to fp32, would cost dw its digits where the
 * points of a task differ by less than 2^-24 of their size); out must still be a valid pointer and is not read.
 * Tiles beyond the count and the rows of inadmissible points are not read.  Status: NPF_EINVAL (nothing launched) for a NULL pointer,
 * n_tasks < 0, pts_per_task <= 0, F <= 0 or F % 32 != 0, R_pt / out / d_out / dR_pt not 16-byte aligned, w / dw not 4-byte aligned,
 * or n_tasks * ceil(pts_per_task / 32) above 2^31 - 1 (task and tile are the grid's x index); n_tasks == 0 launches nothing. */
int npf_weighted_mean_bwd(const float *R_pt, const float *w, const int32_t *n_valid, const float *out, const float *d_out,
                          int32_t n_tasks, int32_t pts_per_task, int32_t F, float *dR_pt, float *dw, void *stream);

/* ---- growing contexts: rows appended at per-task offsets that are device data (csrc/append_kernels.hip) ----------------------
 * For every pair i < n_pairs (<= NPF_APPEND_MAX_PAIRS), task b and j < clamp(n_new[b], 0, n_rows) (n_new == NULL: j < n_rows):
 *   dst_i(b, clamp(n_valid[b], 0, capacity) + j, :) = src_i(b, j, :)    over all F_i features,
 * src_i: PT32 [n_tasks][n_rows][F_i], dst_i: PT32 [n_tasks][capacity][F_i], F_i % 32 == 0.  Rows that would land at or beyond
 * `capacity` are dropped; no other row of dst_i (and nothing outside its `capacity` rows' tiles) is written.  Then, in a second
 * launch in stream order -- after every row of every pair has been placed -- n_valid[b] <- min(n_valid[b] + n_new[b], capacity)
 * (both clamped as above) in place.  n_valid / n_new: DEVICE int32 [n_tasks] tensors the kernels read, the host never does: the
 * call sits in a captured graph and sees new counts at every replay.  `pairs` is read on the host at call time.  n_tasks <= 65535.
 * No reference counterpart (the reference re-encodes the whole context). */
#define NPF_APPEND_MAX_PAIRS 3
typedef struct npf_append_pair {
  const float *src;
  float *dst;
  int32_t F;
  int32_t reserved;
} npf_append_pair_t;
int npf_append_points(const npf_append_pair_t *pairs, int32_t n_pairs, int32_t *n_valid, const int32_t *n_new, int32_t n_tasks,
                      int32_t n_rows, int32_t capacity, void *stream);

/* ---- waveform match over a time-shift grid and its gradient (csrc/waveform_kernels.hip; no reference counterpart) -----------------
 * Row r = k * n_tasks + b (latent sample k, task b) of h holds the predicted waveform h_t = A_t e^{i phi_t}: A = h[r][t][0],
 * phi = h[r][t][1], h_ld >= 2 floats per point (2: a [n_rows][pts][2] tensor; 4: the raw decoder output of a dy = 2 head, whose first
 * two entries are the head's loc).  g[n_tasks][pts][2] holds the reference g_t = A'_t e^{i phi'_t} of every task, wgt the weight
 * w_t of every point (the caller's 4 df / S_n(f); NULL: all ones) and freq its physical frequency f_t, either as one row shared by
 * the tasks (wgt_rows / freq_rows = 1) or one per task (= n_tasks).  Over the uniform grid tau_j = tau0 + j dtau, j < n_tau:
 *   hh  = sum_t w_t A_t^2            gg = sum_t w_t A'_t^2
 *   c_j = sum_t w_t A_t A'_t exp(i (phi_t - phi'_t + 2 pi f_t tau_j))
 *   c_0/ = the same sum without the 2 pi f tau term (no time shift, whatever the grid is)
 *   overlap  = Re c_0/ / sqrt(hh gg)
 *   match    = max_j |c_j| / sqrt(hh gg)        tau_index = the smallest j that attains it
 *   phase    = arg c_{tau_index}
 *   mismatch = 1 - match                        (formed in double, then rounded once)
 * n_tau == 0 (no time maximisation): match = |c_0/| / sqrt(hh gg), phase = arg c_0/, tau_index = 0, and freq is not read (may be
 * NULL).  A point is removed unless 0 < w_t < +inf (the admissibility rule of npf_masked_attn_fwd_weighted): A, phi, A', phi', f of
 * a removed point have no influence, NaN included.  n_valid: NULL or a DEVICE int32 [n_tasks] tensor (clamped to [0, pts]): task b
 * owns its first n_valid[b] points, nothing at or beyond is read.  A row with hh gg == 0 (or no point left) gets overlap = match = 0,
 * mismatch = 1, tau_index = 0, phase = 0 and zeros in corr.
 * Arithmetic: everything -- the phase, its sine and cosine, the products and the sums -- is double, the inputs are fp32 values widened
 * exactly and every output is rounded to fp32 once.  Launch 1: one workgroup per (row, chunk of NPF_WAVEFORM_JC shifts); per point one
 * sincos at the chunk's first shift and one of the step 2 pi f dtau, then a complex rotation per shift (the recurrence restarts at
 * every chunk); sums reduced in a fixed order into `workspace`.  Launch 2: per row the normalisation, maximum and outputs.  No atomics:
 * a second call on the same inputs gives the same bits.  The host reads neither the counts nor the data: the call sits in a captured
 * graph.  Outputs (each may be NULL, at least one must be given; every requested element is written): hh[n_rows], gg[n_tasks],
 * overlap / match / mismatch / tau_index / phase [n_rows], corr[n_rows][max(n_tau, 1)][2] = c_j / sqrt(hh gg) (n_tau == 0: c_0/).
 * workspace: npf_waveform_match_workspace_bytes(n_rows, n_tau) bytes of device memory, 8-byte aligned (NPF_EINVAL (-1) from that
 * function for n_rows <= 0 or n_tau outside [0, 65536]).
 * Status: NPF_EINVAL (nothing launched) for n_rows % n_tasks != 0, h_ld < 2, wgt_rows / freq_rows of a given pointer not in
 * {1, n_tasks}, n_tau < 0, n_tau > 65536, n_tau > 0 with freq == NULL, all outputs NULL, a NULL h, g or workspace, pts <= 0,
 * n_tasks <= 0, n_rows <= 0 or n_rows > 2^24. */
#define NPF_WAVEFORM_JC 16
int64_t npf_waveform_match_workspace_bytes(int32_t n_rows, int32_t n_tau);
int npf_waveform_match(const float *h, int32_t h_ld, const float *g, const float *wgt, int32_t wgt_rows, const float *freq,
                       int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                       double dtau, int32_t n_tau, float *hh, float *gg, float *overlap, float *match, float *mismatch,
                       int32_t *tau_index, float *phase, float *corr, void *workspace, void *stream);
/* npf_waveform_match with one more output for a backward pass: saved[n_rows][4] = (hh, gg, Re c_{j*}, Im c_{j*}), j* = tau_index
 * (n_tau == 0: c_0/), the DOUBLES the finishing launch holds before anything is rounded to fp32; zeros for a degenerate row.  saved
 * may be NULL (and counts as an output when it is not); npf_waveform_match is this call with saved = NULL, and every other output
 * has the same bits with saved given or not. */
int npf_waveform_match_ex(const float *h, int32_t h_ld, const float *g, const float *wgt, int32_t wgt_rows, const float *freq,
                          int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                          double dtau, int32_t n_tau, float *hh, float *gg, float *overlap, float *match, float *mismatch,
                          int32_t *tau_index, float *phase, float *corr, void *workspace, double *saved, void *stream);
/* Gradient of the match with respect to the predicted amplitude and phase, at the maximiser the forward found.  For row r with
 * j* = tau_index[r], tau* = tau0 + j* dtau, theta_t = phi_t - phi'_t + 2 pi f_t tau* (n_tau == 0: no such term, tau_index and freq are
 * not read), c = c_{j*} = (saved[r][2], saved[r][3]), psi = arg c, hh = saved[r][0], gg = saved[r][1], N = sqrt(hh gg), M = |c| / N:
 *   dM/dA_t   = w_t (A'_t cos(theta_t - psi) / N - M A_t / hh)
 *   dM/dphi_t = -w_t A_t A'_t sin(theta_t - psi) / N
 * Where the maximiser over the grid is unique this is the derivative of the maximum (Danskin); at a tie it is the derivative at the
 * smallest index, as the forward reports it: a subgradient.  The mismatch is 1 - M: a caller that differentiates the mismatch hands
 * in the negated incoming gradient.  d_match[n_rows]: the incoming gradient with respect to the match of every row.
 * d_h has n_bcast * n_rows rows of pts * dh_ld floats: row q * n_rows + r, q < n_bcast, receives d_match[r] / n_bcast times the gradient
 * above in entries 0 and 1 of every point and exact zeros in entries 2 .. dh_ld - 1 (dh_ld = 4: d_h is the gradient of the raw decoder
 * output of a dy = 2 head, whose scale entries get none).  n_bcast > 1 serves a match evaluated on the mean over n_bcast latent samples:
 * the mean is linear, every sample receives 1 / n_bcast of the row's gradient, and the n_bcast row blocks are bit-identical.
 * EVERY element of d_h is written, so it needs no memset: a removed point (weight not in (0, inf)), a point at or beyond n_valid[b], and
 * every point of a degenerate row (hh gg == 0, the zeros npf_waveform_match_ex saves; also c == 0, where the phase has no direction)
 * get exact zeros in all entries.  These are selected, never multiplied in: nothing at or beyond n_valid[b] is read, A, phi, A', phi',
 * f of a removed point are not read, and a NaN there (or in d_match of a degenerate row) cannot reach d_h.  There is no gradient with
 * respect to g, wgt or freq.
 * Arithmetic as in the forward: fp32 inputs widened exactly, everything in double -- the two terms of dM/dA cancel as M -> 1, which is
 * why the row scalars arrive unrounded -- one sincos per point, one rounding to fp32 per output.  One launch, one thread per point, no
 * reduction and no atomics: the same inputs give the same bits.  h, g, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts,
 * tau0, dtau, n_tau: as given to the forward; tau_index, saved, n_valid, d_match are DEVICE data the host never reads: the call sits
 * in a captured graph.
 * Status: NPF_EINVAL (nothing launched) for the sizes npf_waveform_match refuses, a NULL h, g, saved, d_match or d_h, n_tau > 0 with
 * freq or tau_index NULL, n_bcast < 1 or dh_ld < 2. */
int npf_waveform_match_bwd(const float *h, int32_t h_ld, const float *g, const float *wgt, int32_t wgt_rows, const float *freq,
                           int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                           double dtau, int32_t n_tau, const int32_t *tau_index, const double *saved, const float *d_match,
                           int32_t n_bcast, float *d_h, int32_t dh_ld, void *stream);

/* ---- bank match: every predicted waveform against every template of one bank (csrc/waveform_bank_kernels.hip; no reference counterpart)
 * h[n_rows][pts][h_ld] as in npf_waveform_match (entries 0 and 1 are A, phi; h_ld >= 2).  bank[n_bank][pts][2] = (A', phi') is ONE
 * bank shared by all rows, so wgt[pts] (NULL: ones) and freq[pts] (NULL only when n_tau == 0) are single rows and there is no
 * n_valid.  A point is removed unless 0 < w_t < +inf: nothing of it is read in h, bank or freq, NaN included; removed points are
 * selected out (the operand panels are built from the live points alone), never multiplied in, so a call with removed points has
 * the bits of the same call with those points cut out.  For row r, template g and tau_j = tau0 + j dtau, j < n_tau:
 *   hh_r = sum_t w_t A_{r,t}^2          gg_g = sum_t w_t A'_{g,t}^2
 *   c_j[r,g] = sum_t w_t A_{r,t} A'_{g,t} exp(i (phi_{r,t} - phi'_{g,t} + 2 pi f_t tau_j))
 *   match[r][g]     = max_j |c_j| / sqrt(hh_r gg_g)       tau_index[r][g] = the smallest j that attains it
 *   phase[r][g]     = arg c_{j*}                          mismatch = 1 - match (formed in double, rounded once)
 *   dot[r][g][2]    = c_{j*} as unrounded DOUBLES
 *   best_index[r]   = the smallest g that attains max_g match[r][g] over the pairs whose match is not NaN, 0 if there is none
 *   best_match[r]   = match[r][best_index[r]]
 * n_tau == 0: the single candidate without the time term.  A pair with hh_r gg_g == 0 gets match = 0, mismatch = 1, tau_index = 0,
 * phase = 0, dot = 0.  A NaN at a live point of row r reaches row r's outputs only, a NaN in template g column g only.
 * Arithmetic: double throughout, from fp32 inputs widened exactly.  Launch 1 writes the operand panels u = w A e^{i phi}, v = A' e^{i
 * phi'}, the per-point step e^{i 2 pi f dtau} and the start e^{i 2 pi f tau_c} of every chunk of NPF_WAVEFORM_JC shifts into
 * `workspace` and reduces hh, gg in a fixed order.  Launch 2: one wavefront per (16 rows, 16 templates); per chunk it rotates its
 * rows once per shift (start, then one complex rotation per further shift: the scheme of npf_waveform_match) and contracts
 * K = 2 pts on v_mfma_f64_16x16x4_f64: Re c takes (Re u, Im u) against (Re v, Im v), Im c against (-Im v, Re v).  The running maximum
 * of |c_j|^2, its first index and c there stay in registers: nothing of size [n_rows][n_bank][n_tau] is written.  Launch 3 (best_*
 * only): one wavefront per row.  No atomics, fixed K and tile order: the same inputs give the same bits.  The host reads no device
 * data: the call sits in a captured graph.  Outputs: each may be NULL, at least one must be given; every requested element is
 * written.  workspace: npf_waveform_match_bank_workspace_bytes(...) bytes of device memory, 8-byte aligned.
 * Status: NPF_EINVAL (nothing launched; -1 from the workspace function for the same sizes) for n_rows, n_bank or pts <= 0,
 * n_rows > 2^24, n_bank > 2^20, h_ld < 2, n_tau outside [0, 65536], n_tau > 0 with freq == NULL, a NULL h, bank or workspace, all
 * outputs NULL. */
int64_t npf_waveform_match_bank_workspace_bytes(int32_t n_rows, int32_t n_bank, int32_t pts, int32_t n_tau);
int npf_waveform_match_bank(const float *h, int32_t h_ld, const float *bank, const float *wgt, const float *freq,
                            int32_t n_rows, int32_t n_bank, int32_t pts, double tau0, double dtau, int32_t n_tau,
                            float *hh, float *gg, float *match, float *mismatch, int32_t *tau_index, float *phase,
                            double *dot, int32_t *best_index, float *best_match, void *workspace, void *stream);

/* ---- matched-filter log likelihood of complex data under the predicted waveforms (csrc/waveform_kernels.hip; no reference counterpart)
 * h, h_ld, wgt, wgt_rows, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau: as in npf_waveform_match; row
 * r = s * n_tasks + b is latent sample s of task b, n_z = n_rows / n_tasks.  d[n_tasks][pts][2] holds the data of every task as
 * (Re d_t, Im d_t): Cartesian, so neither an atan2 nor an fp32 phase of the data enters anywhere.  w_t is the caller's 4 df / S_n(f_t).
 * A point is LIVE if t < n_valid[b] and 0 < w_t < +inf; nothing is read of a point that is not live (NaN included); a NaN in h, d or
 * freq of a LIVE point is the caller's and propagates into the row's outputs and its task's mixtures.  All sums run
 * over the live points, in double, from fp32 inputs widened exactly:
 *   kappa_j  = sum_t w_t A_t e^{i (phi_t + 2 pi f_t tau_j)} conj(d_t)      tau_j = tau0 + j dtau, j < n_tau
 *   kappa_0/ = the same sum without the time term (n_tau == 0: the only candidate, n = 1 below; freq is not read and may be NULL)
 *   hh = sum_t w_t A_t^2          dd = sum_t w_t |d_t|^2
 *   x_j = |kappa_j|               j* = the smallest j that attains max_j x_j
 *   snr      = x_{j*} / sqrt(hh)                  (the optimal SNR is sqrt(hh))
 *   phase    = arg kappa_{j*}
 *   lnl_max  = x_{j*} - hh / 2                    (ln Lambda maximised over the phase and the grid times)
 *   L_j      = ln I0(x_j) - hh / 2                (phase marginalised, uniform prior)
 *   lnl_marg = logsumexp_j L_j - ln n,  n = max(n_tau, 1)      (phase and time marginalised, uniform over the grid)
 *   lnl_mix[b]     = logsumexp_s lnl_marg[s n_tasks + b] - ln n_z      (the latent samples marginalised)
 *   lnl_max_mix[b] = logsumexp_s lnl_max[s n_tasks + b] - ln n_z
 * The time term has the sign of npf_waveform_match: h is shifted by e^{+i 2 pi f tau}.  A degenerate row, hh == 0 (no live point or a
 * zero template), gets snr = 0, phase = 0, tau_index = 0, lnl_max = lnl_marg = 0 (Lambda = 1) and zeros in series; it enters the two
 * mixtures with 0.  The constant -dd / 2 is added to nothing; dd is returned so that the caller can.
 * ln I0(x) in double: below NPF_LOGLIKE_I0_SWITCH, log1p of the power series sum_{k >= 1} (x^2 / 4)^k / (k!)^2; from there on
 * x - ln(2 pi x) / 2 + log1p(S), S the first 16 terms of the series in 1 / (8 x) (truncation 2.7e-16 of I0 at the switch point).  No
 * overflow for any finite x.  Both log-sum-exps are shifted by their maximum, the one over the latent samples as well: rows whose
 * likelihoods lie more than 745 apart give neither -inf nor NaN.
 * Launch 1: geometry, recurrence, reduction order and workspace of npf_waveform_match's first launch (per row [hh, dd, Re kappa_0/,
 * Im kappa_0/, (Re, Im) kappa_j ...]).  Launch 2: one workgroup per task walks its n_z rows in order.  No atomics: a second call on
 * the same inputs gives the same bits; the host reads nothing, so the call sits in a captured graph.
 * Outputs, all DOUBLE but tau_index (each may be NULL, at least one must be given; every requested element is written):
 * hh / snr / lnl_max / lnl_marg / tau_index / phase [n_rows], dd / lnl_mix / lnl_max_mix [n_tasks],
 * series[n_rows][max(n_tau, 1)][2] = (L_j, x_j / sqrt(hh)).
 * workspace: npf_waveform_loglike_workspace_bytes(n_rows, n_tau) bytes of device memory, 8-byte aligned; the function equals
 * npf_waveform_match_workspace_bytes.  Status: NPF_EINVAL (nothing launched) under the rules of npf_waveform_match, d in g's place. */
#define NPF_LOGLIKE_I0_SWITCH 24.0
int64_t npf_waveform_loglike_workspace_bytes(int32_t n_rows, int32_t n_tau);
int npf_waveform_loglike(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                         int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                         double dtau, int32_t n_tau, double *hh, double *dd, double *snr, double *lnl_max, double *lnl_marg,
                         int32_t *tau_index, double *phase, double *series, double *lnl_mix, double *lnl_max_mix, void *workspace,
                         void *stream);

/* ---- coherent matched-filter log likelihood of a detector network (csrc/waveform_net_kernels.hip; no reference counterpart)
 * h, h_ld, freq, freq_rows, n_valid, n_rows, n_tasks, pts, tau0, dtau, n_tau, the rows r = s * n_tasks + b: as in
 * npf_waveform_loglike.  Detector k < n_det = D, 1 <= D <= NPF_NET_MAX_DET, sees the same waveform with its own noise spectrum, its own
 * arrival delay and its own complex response factor (antenna pattern times inclination):
 *   d[n_tasks][D][pts][2]     fp32, the data of every task and detector as (Re, Im)
 *   wgt                       fp32, [D][pts] (wgt_rows == 1) or [n_tasks][D][pts] (wgt_rows == n_tasks), NULL: ones
 *   delay[n_tasks][D]         DOUBLE, DEVICE data: seconds, either sign, not tied to the grid; NULL: zeros
 *   resp[n_tasks][D][2]       DOUBLE, DEVICE data: C_{b,k} = (Re, Im); detector k's template is C_k h shifted by tau_j + delay_k
 * The host reads neither delay nor resp: both may be overwritten in place between the replays of a captured graph.
 * A point is LIVE FOR DETECTOR k if t < n_valid[b] and 0 < w_{k,t} < +inf; nothing is read of a point that is not live, in any of that
 * detector's arrays (NaN included).  freq is shared by the detectors and is read only for points that are live for at least one
 * detector.  All sums run over the live points, in double, from fp32 inputs widened exactly:
 *   kappa_{k,j} = sum_t w_{k,t} A_t e^{i (phi_t + 2 pi f_t (tau_j + delay_k))} conj(d_{k,t})       tau_j = tau0 + j dtau, j < n_tau
 *   hh_k = sum_t w_{k,t} A_t^2          dd_k = sum_t w_{k,t} |d_{k,t}|^2
 *   K_j  = sum_k C_k kappa_{k,j}        HH = sum_k |C_k|^2 hh_k        DD = sum_k dd_k        (k in ascending order)
 *   x_j  = |K_j|                        j* = the smallest j that attains max_j x_j
 *   snr      = x_{j*} / sqrt(HH)        phase = arg K_{j*}             lnl_max = x_{j*} - HH / 2
 *   L_j      = ln I0(x_j) - HH / 2      lnl_marg = logsumexp_j L_j - ln n,  n = max(n_tau, 1)
 *   lnl_mix[b], lnl_max_mix[b]: the log-mean-exp of lnl_marg / lnl_max over the latent samples, as in npf_waveform_loglike
 *   snr_det[r][k] = |kappa_{k,j*}| / sqrt(hh_k)   (0 where hh_k == 0)      hh_det[r][k] = hh_k      dd_det[b][k] = dd_k
 * The complex sums of the detectors are added BEFORE the modulus is taken: one coalescence phase and one geocentric arrival time are
 * shared by the network, which D calls of npf_waveform_loglike cannot give.  n_tau == 0: the one candidate is tau = 0 and the delays
 * still enter, so freq is required whenever delay is given (with neither a grid nor delays freq is not read and may be NULL).  A
 * degenerate row, HH == 0 (no live point, a zero template or no response), gets the zeros npf_waveform_loglike gives, and its
 * snr_det is taken at j* = 0.  A detector with C_k == 0 changes no network output and still reports its snr_det.  ln I0, its switch
 * point and both max-shifted log-sum-exps are those of npf_waveform_loglike.
 * Launch 1: one workgroup per (row, chunk of NPF_WAVEFORM_JC shifts) walks the detectors; per detector the recurrence and the
 * reduction order of npf_waveform_loglike's first launch (one double sincos of phi + 2 pi f (tau_c0 + delay_k) and one of the step per
 * live point, restarted at every chunk), and the reducing threads add C_k kappa_{k,j} to the network sums in ascending k.  The sums a
 * thread keeps do not grow with D.  Launch 2: one workgroup per task walks its n_z rows in order over the network sums and, for
 * snr_det, forms the D sums kappa_{k,j*} once more at the single shift j* (a direct sincos per live point): no per-detector series is
 * kept.  No atomics: a second call on the same inputs gives the same bits; the host reads nothing, so the call sits in a captured graph.
 * Outputs, all DOUBLE but tau_index (each may be NULL, at least one must be given; every requested element is written):
 * hh (= HH) / snr / lnl_max / lnl_marg / tau_index / phase [n_rows], dd (= DD) / lnl_mix / lnl_max_mix [n_tasks],
 * series[n_rows][max(n_tau, 1)][2] = (L_j, x_j / sqrt(HH)), hh_det / snr_det [n_rows][D], dd_det [n_tasks][D].
 * workspace: npf_waveform_loglike_net_workspace_bytes(n_rows, n_det, n_tau) bytes of device memory, 8-byte aligned: per row 2 + 2 D
 * doubles and whole chunks of (Re, Im) (-1 for sizes the call refuses).  Status: NPF_EINVAL (nothing launched) for everything
 * npf_waveform_loglike refuses, n_det outside [1, NPF_NET_MAX_DET], a NULL resp, and delay given with a NULL freq. */
#define NPF_NET_MAX_DET 8
int64_t npf_waveform_loglike_net_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t n_tau);
int npf_waveform_loglike_net(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                             int32_t freq_rows, const int32_t *n_valid, const double *delay, const double *resp, int32_t n_rows,
                             int32_t n_tasks, int32_t n_det, int32_t pts, double tau0, double dtau, int32_t n_tau, double *hh,
                             double *dd, double *snr, double *lnl_max, double *lnl_marg, int32_t *tau_index, double *phase,
                             double *series, double *lnl_mix, double *lnl_max_mix, double *hh_det, double *snr_det, double *dd_det,
                             void *workspace, void *stream);

/* ---- sky-grid network likelihood (csrc/waveform_sky_kernels.hip; no reference counterpart)
 * The coherent likelihood of npf_waveform_loglike_net at every pixel of ONE sky grid shared by the tasks, and its marginal over the
 * pixels.  h, h_ld, d[n_tasks][D][pts][2], wgt ([D][pts] or [n_tasks][D][pts], NULL: ones), wgt_rows, n_valid, n_rows, n_tasks,
 * n_det = D (1 <= D <= NPF_NET_MAX_DET), pts, tau0, dtau, n_tau, the rows r = s * n_tasks + b: as in npf_waveform_loglike_net.  A
 * point is LIVE FOR DETECTOR k exactly as there (t < n_valid[b] and 0 < w_{k,t} < +inf); a point that is not live contributes an exact
 * zero, chosen by a select and not a multiply, and nothing else of it is read in h, d or wgt (NaN included).
 *   freq[pts]               fp32, ONE row shared by all tasks (the pixel operand is shared): required, freq_rows must be 1, read at
 *                           every t < pts.  PRECONDITION: every entry is finite (the host does not read it).
 *   resp[n_pix][D][2]       DOUBLE, DEVICE data: C_{p,k} = (Re, Im), the response of detector k to pixel p
 *   delay[n_pix][D]         DOUBLE, DEVICE data: Delta_{p,k} in seconds, either sign, not tied to the grid; NULL: zeros
 *   log_prior[n_pix]        DOUBLE, DEVICE data: the log prior MASS of every pixel; NULL: uniform, -ln n_pix each
 * with 1 <= n_pix = P <= NPF_SKY_MAX_PIX.  The grid is shared by the tasks.  The host reads none of the three: all may be overwritten
 * in place between the replays of a captured graph.  A pixel is LIVE if its log_prior is finite; a dead pixel gets no mass and -inf /
 * 0 outputs, nothing of its resp or delay is read (NaN included), and nothing of it reaches another pixel.
 * Everything in double, from fp32 inputs widened exactly; n = max(n_tau, 1), n_tau == 0 is the one candidate tau = 0 (the delays
 * still enter):
 *   K_{j,p}[r] = sum_k sum_t [w_{k,t} A_t e^{i phi_t} conj(d_{k,t}) e^{i 2 pi f_t tau_j}] [C_{p,k} e^{i 2 pi f_t Delta_{p,k}}]
 *   hh_k[r]   = sum_t w_{k,t} A_t^2                     HH_p[r] = sum_k |C_{p,k}|^2 hh_k[r]       (k ascending)
 *   x_{j,p}   = |K_{j,p}|                               L_{j,p} = ln I0(x_{j,p}) - HH_p / 2       (ln I0 of npf_waveform_loglike)
 *   u_p       = log_prior_p + logsumexp_j L_{j,p} - ln n                        (-inf for a dead pixel)
 *   lnl_sky[r]   = logsumexp_p u_p                      (no live pixel: -inf)
 *   pix_index[r] = the smallest p attaining max_p u_p   (no live pixel: 0)
 *   tau_index[r] = the smallest j attaining max_j x_{j,p*},  snr[r] = x_{j*,p*} / sqrt(HH_{p*})   (0 where HH_{p*} == 0), p* = pix_index
 *                  (p* dead, which needs every pixel dead: tau_index = 0, snr = 0)
 *   post[r][p]   = u_p - lnl_sky[r]                     (-inf at dead pixels, everywhere when none is live)
 *   snr_map[r][p] = max_j x_{j,p} / sqrt(HH_p)          (0 where HH_p == 0 or the pixel is dead)
 *   lnl_sky_mix[b] = log-mean-exp over the latent samples of lnl_sky
 *   post_mix[b][p] = logmeanexp_s u_p[s, b] - lnl_sky_mix[b]
 * A pixel with HH_p == 0 has Lambda = 1, so u_p = log_prior_p, by the formulas.  The prior is not normalised by the kernel.  The
 * log-sum-exp over j is carried chunk by chunk with a running maximum.  A NaN at a live point of row r reaches row r's outputs and its
 * task's mixtures only.  A NaN in the resp or delay of a LIVE pixel p makes K_{j,p} and HH_p NaN, so snr_map[r][p] and u_p, and with
 * u_p lnl_sky[r] and lnl_sky_mix, are NaN in every row, while snr_map at every other pixel keeps its bits.
 * The work is one complex GEMM with M = rows x n_tau, N = P, K = D x pts: the first bracket depends on (row, j) only, the second on
 * the pixel only, and the detectors fold into the contraction axis, so the sum over k stays inside the modulus.  Launch 1 writes the
 * operand panels in the fragment order of npf_waveform_match_bank (K axis: detector ascending, then point ascending, every detector's
 * points padded to a multiple of 4 and rows / pixels to whole tiles of 16, all with exact zeros), the step e^{i 2 pi f dtau} and the
 * start of every chunk of NPF_SKY_JC shifts once over t, and hh_k in a fixed order.  Launch 2: one wavefront per (16 rows, 16 pixels)
 * on v_mfma_f64_16x16x4_f64; per chunk the 2 NPF_SKY_JC accumulator tiles, ln I0 on them, the running log-sum-exp over j and the
 * running max x with its first j stay in registers: nothing of size [n_rows][n_pix][n_tau] is written.  Launch 3: one workgroup per
 * task over its n_z rows in order; the sum over the pixels is taken in 2^-62 fixed point on integer accumulators, so lnl_sky and post
 * do not depend on the order of the pixels (error <= P 2^-62 of the largest term).  No atomics: a second call on the same inputs gives
 * the same bits, and the value at (row, pixel) does not depend on the tile, wavefront or workgroup that computed it.  The host reads
 * no device data: the call sits in a captured graph.
 * Outputs, all DOUBLE but the two int32 indices (each may be NULL, at least one must be given; every requested element is written):
 * lnl_sky / pix_index / tau_index / snr [n_rows], lnl_sky_mix [n_tasks], post / snr_map [n_rows][n_pix], post_mix [n_tasks][n_pix].
 * workspace: npf_waveform_loglike_sky_workspace_bytes(n_rows, n_det, pts, n_pix, n_tau) bytes of device memory, 8-byte aligned (-1
 * for sizes the call refuses).  NPF_SKY_MAX_PIX = 65536 keeps that count in int64: the largest term, the row panel, is at most 2^24
 * rows x 8 detectors x 2^31 points x 16 bytes = 2^62.
 * Status: NPF_EINVAL (nothing launched) for everything npf_waveform_loglike_net refuses, freq_rows != 1, a NULL freq or resp, n_pix
 * outside [1, NPF_SKY_MAX_PIX], all outputs NULL. */
#define NPF_SKY_JC 8
#define NPF_SKY_MAX_PIX 65536
int64_t npf_waveform_loglike_sky_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t pts, int32_t n_pix, int32_t n_tau);
int npf_waveform_loglike_sky(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                             int32_t freq_rows, const int32_t *n_valid, const double *resp, const double *delay,
                             const double *log_prior, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, int32_t n_pix,
                             double tau0, double dtau, int32_t n_tau, double *lnl_sky, int32_t *pix_index, int32_t *tau_index,
                             double *snr, double *lnl_sky_mix, double *post, double *snr_map, double *post_mix, void *workspace,
                             void *stream);

/* ---- distance-marginalised likelihood (csrc/waveform_dist_kernels.hip; no reference counterpart)
 * The predicted waveform is a template at a reference distance d_ref; at luminosity distance d it is a h with the amplitude scale
 * a = d_ref / d.  npf_waveform_loglike_dist marginalises the likelihood of npf_waveform_loglike over a grid of scales as well,
 * npf_waveform_loglike_net_dist that of npf_waveform_loglike_net.  The arguments up to the parent's last output are the parent's; then
 *   scales[scale_rows][n_a]      DOUBLE, DEVICE data: a_i; scale_rows == 1 (shared by the tasks) or n_tasks
 *   log_prior[prior_rows][n_a]   DOUBLE, DEVICE data: ln pi_i, the log prior MASS of grid point i (quadrature weight included)
 * with 1 <= n_a <= NPF_DIST_MAX_SCALES, then the new outputs, then workspace and stream.  The host reads neither tensor: both may be
 * overwritten in place between the replays of a captured graph.  A scale is LIVE if 0 < a_i < +inf and ln pi_i is finite; nothing else
 * of a dead scale is used (NaN included).  With x_j, HH (hh of the single stream), j* and the rows r = s * n_tasks + b of the parent,
 * n = max(n_tau, 1), all in double:
 *   x*      = x_{j*} = max_j x_j
 *   M_i     = ln pi_i + (ln I0(a_i x*) - a_i^2 HH / 2)                          (live i)
 *   S_i     = sum_j exp(ln I0(a_i x_j) - ln I0(a_i x*))                         (every term <= 1: ln I0 increases)
 *   u_i     = M_i + (ln S_i - ln n)              dead i: u_i = -inf             (the evidence of scale i, phase and time marginalised)
 *   lnl_dist[r]     = logsumexp_i u_i            (shifted by max_i u_i; no live scale: -inf)
 *   post[r][i]      = u_i - lnl_dist[r]          (-inf for dead i, and for every i when no scale is live)
 *   scale_index[r]  = the smallest i that attains max_i u_i   (no live scale: 0)
 *   scale_hat[r]    = x* / HH        lnl_amp_max[r] = x*^2 / (2 HH)             (both 0 for HH == 0)
 *   lnl_dist_mix[b] = logsumexp_s lnl_dist[s n_tasks + b] - ln n_z
 *   post_mix[b][i]  = logsumexp_s u_i[s n_tasks + b] - ln n_z - lnl_dist_mix[b]   (-inf where that is -inf - -inf)
 * The prior is NOT normalised: lnl_dist carries ln sum_i pi_i as given.  A row with HH == 0 is treated as x_j = 0 for every j:
 * Lambda = 1 at every scale, lnl_dist = logsumexp_i ln pi_i and post_i = ln pi_i - lnl_dist (the parent's degenerate-row rule,
 * extended).  With n_a = 1, a = 1, ln pi = 0, u_0 is the expression the parent evaluates for lnl_marg, in its order.  a_i x* and
 * a_i^2 HH must be finite.  post and post_mix are formed as (u_i - max) - ln sum, the difference first, so that sum_i exp(post_i) = 1
 * holds to rounding where u reaches 1e6; the mixture keeps its shift and its sum apart for the same reason.
 * Launches: launch 1 of the parent; the parent's finishing launch only if one of the parent's outputs is requested -- those outputs
 * come from the parent's kernels and match a plain call bit for bit; then, if one of the new outputs is requested, launch A (one
 * workgroup per (row, chunk of NPF_DIST_SC scales): x* by the finishing kernels' reduction, x_j kept in LDS up to 4096 grid times and
 * re-read from the workspace beyond, ln I0(a_i x*) once per scale, S_i strided over j and reduced in a fixed order, u_i into the row's
 * workspace tail) and launch B (one workgroup per task walks its n_z rows in order; post_mix is a second pass over the u_i).  No
 * atomics: a second call gives the same bits; the host reads nothing, so the call sits in a captured graph.
 * New outputs (each may be NULL; with the parent's, at least one must be given; every requested element is written): DOUBLE
 * lnl_dist / scale_hat / lnl_amp_max [n_rows], int32 scale_index [n_rows], lnl_dist_mix [n_tasks], post [n_rows][n_a],
 * post_mix [n_tasks][n_a].
 * workspace: npf_waveform_loglike_dist_workspace_bytes(n_rows, n_det, n_tau, n_a) bytes, 8-byte aligned; n_det == 0: the single
 * stream.  Per row the parent's doubles, then x* and the n_a values u_i (-1 for sizes the calls refuse).
 * Status: NPF_EINVAL (nothing launched) for everything the parent refuses but its "no output" rule, n_a outside
 * [1, NPF_DIST_MAX_SCALES], a NULL scales or log_prior, scale_rows or prior_rows neither 1 nor n_tasks, no output requested at all. */
#define NPF_DIST_SC 16
#define NPF_DIST_MAX_SCALES 4096
int64_t npf_waveform_loglike_dist_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t n_tau, int32_t n_a);
int npf_waveform_loglike_dist(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                              int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                              double dtau, int32_t n_tau, double *hh, double *dd, double *snr, double *lnl_max, double *lnl_marg,
                              int32_t *tau_index, double *phase, double *series, double *lnl_mix, double *lnl_max_mix,
                              const double *scales, int32_t scale_rows, const double *log_prior, int32_t prior_rows, int32_t n_a,
                              double *lnl_dist, int32_t *scale_index, double *scale_hat, double *lnl_amp_max, double *lnl_dist_mix,
                              double *post, double *post_mix, void *workspace, void *stream);
int npf_waveform_loglike_net_dist(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                                  int32_t freq_rows, const int32_t *n_valid, const double *delay, const double *resp, int32_t n_rows,
                                  int32_t n_tasks, int32_t n_det, int32_t pts, double tau0, double dtau, int32_t n_tau, double *hh,
                                  double *dd, double *snr, double *lnl_max, double *lnl_marg, int32_t *tau_index, double *phase,
                                  double *series, double *lnl_mix, double *lnl_max_mix, double *hh_det, double *snr_det, double *dd_det,
                                  const double *scales, int32_t scale_rows, const double *log_prior, int32_t prior_rows, int32_t n_a,
                                  double *lnl_dist, int32_t *scale_index, double *scale_hat, double *lnl_amp_max, double *lnl_dist_mix,
                                  double *post, double *post_mix, void *workspace, void *stream);

/* ---- sky and distance marginalised jointly (csrc/waveform_sky_kernels.hip; no reference counterpart)
 * The likelihood of npf_waveform_loglike_sky at every pixel of the shared sky grid AND every scale of ONE scale grid shared by the
 * tasks.  The arguments up to n_tau are those of npf_waveform_loglike_sky, under its rules (live points, live pixels, freq_rows == 1,
 * the preconditions on freq); then
 *   scales[n_a]            DOUBLE, DEVICE data: a_i
 *   log_prior_scale[n_a]   DOUBLE, DEVICE data: ln pi_i, the log prior MASS of grid point i (quadrature weight included)
 * with 1 <= n_a <= NPF_DIST_MAX_SCALES and the liveness rule of npf_waveform_loglike_dist (0 < a_i < +inf and ln pi_i finite; nothing
 * else of a dead scale is used, NaN included).  The host reads neither.  With x_{p,j} = |K_{j,p}|, HH_p, n = max(n_tau, 1) and lp_p
 * (NULL: -ln n_pix) of the sky call, x*_p = max_j x_{p,j}, all in double:
 *   w_{p,i} = lp_p + ((ln pi_i + (ln I0(a_i x*_p) - a_i^2 HH_p / 2)) + (ln sum_j exp(ln I0(a_i x_{p,j}) - ln I0(a_i x*_p)) - ln n))
 *             (dead p or dead i: -inf; every term of the sum <= 1)
 *   lnl_vol[r]        = logsumexp_{p,i} w_{p,i}                                  (no live pixel or no live scale: -inf)
 *   post_sky[r][p]    = logsumexp_i w_{p,i} - lnl_vol[r]   (= u_sky[p] - lnl_vol)     post_dist[r][i] = logsumexp_p w_{p,i} - lnl_vol[r]
 *   post_joint[r][p][i] = w_{p,i} - lnl_vol[r]
 *   pix_index[r]      = the smallest p attaining max_p u_sky[p]    scale_index[r] = the smallest i attaining max_i u_dist[i]
 *   tau_index[r], snr[r] = what npf_waveform_loglike_sky reports at pixel pix_index;  scale_hat[r] = x* / HH there (0 where HH == 0)
 *   dist_mean[r][p]   = sum_i (1 / a_i) exp(w_{p,i} - u_sky[p])                   (E[d / d_ref | pixel p])
 *   dist_std[r][p]    = sqrt(sum_i (1 / a_i - dist_mean)^2 exp(w_{p,i} - u_sky[p]))   (a second pass about the mean)
 *   lnl[b]            = logsumexp_s lnl_vol[s n_tasks + b] - ln n_z
 *   post_sky_mix[b][p]  = logsumexp_s u_sky[s n_tasks + b][p] - ln n_z - lnl[b]      post_dist_mix[b][i]: the same of u_dist
 * A dead pixel or scale gets -inf in every posterior and 0 in dist_mean / dist_std.  With no live pixel or no live scale lnl_vol is
 * -inf, the indices are 0 and snr = scale_hat = 0.  A pixel with HH_p == 0 is treated as x = 0: w_{p,i} = lp_p + ln pi_i.  The priors
 * are not normalised.  The posteriors are differences first -- with mm_p = max_i w, s_p = sum_i exp(w - mm_p), M = max w and total =
 * sum_p exp(mm_p - M) s_p: post_sky = (mm_p - M) + (ln s_p - ln total), post_joint = (w - M) - ln total, post_dist likewise -- so each
 * sums to one to rounding where w reaches 1e6.  Sums over the pixels (total, and sum_p exp(w_{p,i} - max_p w) of every scale) are
 * taken in the 2^-62 fixed point of npf_waveform_loglike_sky on integer accumulators: they do not depend on the order of the pixels;
 * sums over the scales run in ascending i.  A NaN in the resp or delay of a LIVE pixel makes that pixel's w NaN in every row: lnl_vol,
 * lnl, post_* are NaN, while dist_mean / dist_std at every other pixel keep their bits.
 * Launch 1: the prep launch of npf_waveform_loglike_sky.  Launch 2: its f64 MFMA correlation with an epilogue that stores x_{p,j} to
 * the panel X[n_rows][n][pix_pad] (pix_pad = n_pix rounded up to 16; the 16 lanes of a C/D fragment row store one 128-byte line) and
 * keeps max_j x, its first j and HH_p.  Launch 3: one wavefront per (row, 64 pixels, NPF_SKYD_SC scales), one pass over j, w to the
 * panel W[n_rows][n_a][pix_pad].  Launch 4: one workgroup per task over its n_z rows in order.  No atomics, no host read: a second
 * call gives the same bits and the call sits in a captured graph.
 * Outputs, all DOUBLE but the three int32 indices (each may be NULL, at least one must be given; every requested element is written):
 * lnl_vol / pix_index / scale_index / tau_index / snr / scale_hat [n_rows], lnl [n_tasks], post_sky / dist_mean / dist_std
 * [n_rows][n_pix], post_dist [n_rows][n_a], post_joint [n_rows][n_pix][n_a], post_sky_mix [n_tasks][n_pix], post_dist_mix
 * [n_tasks][n_a].
 * workspace: npf_waveform_loglike_sky_dist_workspace_bytes(n_rows, n_det, pts, n_pix, n_tau, n_a) bytes of device memory, 8-byte
 * aligned (-1 for sizes the call refuses and for a count that does not fit int64).
 * Status: NPF_EINVAL (nothing launched) for everything npf_waveform_loglike_sky refuses, a NULL scales or log_prior_scale, n_a outside
 * [1, NPF_DIST_MAX_SCALES], a workspace count beyond int64, all outputs NULL. */
#define NPF_SKYD_SC 8
int64_t npf_waveform_loglike_sky_dist_workspace_bytes(int32_t n_rows, int32_t n_det, int32_t pts, int32_t n_pix, int32_t n_tau,
                                                      int32_t n_a);
int npf_waveform_loglike_sky_dist(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                                  int32_t freq_rows, const int32_t *n_valid, const double *resp, const double *delay,
                                  const double *log_prior, int32_t n_rows, int32_t n_tasks, int32_t n_det, int32_t pts, int32_t n_pix,
                                  double tau0, double dtau, int32_t n_tau, const double *scales, const double *log_prior_scale,
                                  int32_t n_a, double *lnl_vol, int32_t *pix_index, int32_t *scale_index, int32_t *tau_index,
                                  double *snr, double *scale_hat, double *lnl, double *post_sky, double *post_dist, double *post_joint,
                                  double *dist_mean, double *dist_std, double *post_sky_mix, double *post_dist_mix, void *workspace,
                                  void *stream);

/* ---- gradient of the matched-filter likelihoods with respect to the predicted waveform (csrc/waveform_grad_kernels.hip; no reference
 * counterpart).  npf_waveform_loglike_ex / npf_waveform_loglike_net_ex are npf_waveform_loglike / npf_waveform_loglike_net with one
 * more argument before workspace: every output of the parent comes from the parent's own launches and is BIT-EQUAL to a plain call,
 * and a third launch (one workgroup per row over the workspace row launch 1 left, the maximum and the shifted sum in the finishing
 * launch's order) fills
 *   saved[n_rows][npf_waveform_loglike_saved_doubles(n_tau) = 4 + 2 n]   DOUBLE, n = max(n_tau, 1), the caller's (the workspace may be
 *     reused before the backward runs): [hh (the network: HH), Re conj(u_{j*}), Im conj(u_{j*}), 0, (Re q_j, Im q_j) j < n]
 * with x_j = |kappa_j| (|K_j|), u_j = kappa_j / x_j (0 where x_j == 0), p_j = exp(L_j - logsumexp_j L_j), rho = I1 / I0 and
 *   q_j = p_j rho(x_j) conj(u_j)                                  (|sum_j q_j| <= 1; a row with hh == 0: all zeros)
 * rho(x) in double: below NPF_LOGLIKE_I0_SWITCH (x / 2) S1 / S0 with the power series S0 = sum_k (x^2 / 4)^k / (k!)^2 and
 * S1 = sum_k (x^2 / 4)^k / (k! (k + 1)!); from there on the ratio of the two 16-term series in 1 / (8 x).  rho(0) = 0, no overflow.
 * The parent's "no output" rule does not apply (saved is one); a NULL saved is NPF_EINVAL.
 *
 * npf_waveform_loglike_bwd / npf_waveform_loglike_net_bwd: the gradient of a scalar F of the four likelihoods with respect to (A, phi).
 * Upstream gradients, DOUBLE, DEVICE data, each may be NULL (at least one must be given): d_marg / d_max [n_rows] of lnl_marg /
 * lnl_max, d_mix / d_max_mix [n_tasks] of lnl_mix / lnl_max_mix; lnl_marg, lnl_max, lnl_mix, lnl_max_mix: what the forward returned
 * (read only for a mixture's gradient, which needs both of its tensors).  Per row, with b = r % n_tasks, n_z = n_rows / n_tasks,
 *   g_marg = d_marg[r] + d_mix[b] exp(lnl_marg[r] - lnl_mix[b]) / n_z        g_max likewise from d_max, d_max_mix
 *   G_t    = g_marg sum_j q_j e^{i 2 pi f_t tau_j} + g_max conj(u_{j*}) e^{i 2 pi f_t tau_{j*}}     (n_tau == 0: no time factors)
 *   E_t    = conj(d_t) e^{i phi_t}
 *   dF/dA_t = w_t (Re(E_t G_t) - (g_marg + g_max) A_t)          dF/dphi_t = -w_t A_t Im(E_t G_t)
 * and for the network, over the detectors that are live at t in ascending k, with the one G_t:
 *   E_{k,t} = C_k conj(d_{k,t}) e^{i (phi_t + 2 pi f_t delay_k)}
 *   dA += w_{k,t} (Re(E_{k,t} G_t) - (g_marg + g_max) |C_k|^2 A_t)          dphi -= w_{k,t} A_t Im(E_{k,t} G_t)
 * The lnl_marg term is exact; the lnl_max term is the derivative at j* = tau_index[r], the grid time the forward found (at a tie the
 * smallest index: a subgradient, as in npf_waveform_match_bwd).  d_h, n_bcast, dh_ld: as in npf_waveform_match_bwd -- row
 * q * n_rows + r receives 1 / n_bcast of row r's gradient, entries 2 .. dh_ld - 1 get exact zeros, EVERY element is written.  A point
 * that is not live (the network: for any detector), a point at or beyond n_valid[b] and every point of a row with hh == 0 get exact
 * zeros, SELECTED: nothing of such a point is read, nor the upstream gradients of such a row, and a NaN there cannot reach d_h.
 * (For hh == 0 the zero is the limit of the marginal's gradient: rho(0) = 0.)  No gradient with respect to d, wgt, freq, resp, delay.
 * One launch: grid (n_rows, min(ceil(pts / 256), 1024)), one thread per point with a grid-stride loop; the workgroup stages 256
 * shifts of the row's coefficients in LDS at a time; per point and chunk of NPF_WAVEFORM_JC shifts one double sincos of
 * 2 pi f_t tau_{j0}, one of 2 pi f_t dtau per point, then G += q_j z, z <- z s; one sincos of phi_t per point, for the network one
 * per (point, live detector) where delay is given.  Everything in double, one rounding to fp32 per output; no reduction across
 * threads, no atomics: the same inputs give the same bits.  The host reads nothing: the call sits in a captured graph.
 * Status: NPF_EINVAL (nothing launched) for the sizes the forward refuses, a NULL h, d, saved or d_h, n_tau > 0 with freq or
 * tau_index NULL, no upstream gradient, d_mix without lnl_marg and lnl_mix, d_max_mix without lnl_max and lnl_max_mix, n_bcast < 1,
 * dh_ld < 2; the network: n_det outside [1, NPF_NET_MAX_DET], a NULL resp, delay given with a NULL freq. */
int64_t npf_waveform_loglike_saved_doubles(int32_t n_tau);
int npf_waveform_loglike_ex(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                            int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                            double dtau, int32_t n_tau, double *hh, double *dd, double *snr, double *lnl_max, double *lnl_marg,
                            int32_t *tau_index, double *phase, double *series, double *lnl_mix, double *lnl_max_mix, double *saved,
                            void *workspace, void *stream);
int npf_waveform_loglike_net_ex(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                                int32_t freq_rows, const int32_t *n_valid, const double *delay, const double *resp, int32_t n_rows,
                                int32_t n_tasks, int32_t n_det, int32_t pts, double tau0, double dtau, int32_t n_tau, double *hh,
                                double *dd, double *snr, double *lnl_max, double *lnl_marg, int32_t *tau_index, double *phase,
                                double *series, double *lnl_mix, double *lnl_max_mix, double *hh_det, double *snr_det, double *dd_det,
                                double *saved, void *workspace, void *stream);
int npf_waveform_loglike_bwd(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                             int32_t freq_rows, const int32_t *n_valid, int32_t n_rows, int32_t n_tasks, int32_t pts, double tau0,
                             double dtau, int32_t n_tau, const int32_t *tau_index, const double *saved, const double *lnl_marg,
                             const double *lnl_max, const double *lnl_mix, const double *lnl_max_mix, const double *d_marg,
                             const double *d_max, const double *d_mix, const double *d_max_mix, int32_t n_bcast, float *d_h,
                             int32_t dh_ld, void *stream);
int npf_waveform_loglike_net_bwd(const float *h, int32_t h_ld, const float *d, const float *wgt, int32_t wgt_rows, const float *freq,
                                 int32_t freq_rows, const int32_t *n_valid, const double *delay, const double *resp, int32_t n_rows,
                                 int32_t n_tasks, int32_t n_det, int32_t pts, double tau0, double dtau, int32_t n_tau,
                                 const int32_t *tau_index, const double *saved, const double *lnl_marg, const double *lnl_max,
                                 const double *lnl_mix, const double *lnl_max_mix, const double *d_marg, const double *d_max,
                                 const double *d_mix, const double *d_max_mix, int32_t n_bcast, float *d_h, int32_t dh_ld, void *stream);

int npf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NPF_HIP_H */
