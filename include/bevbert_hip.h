/* libbevbert_hip.so -- C ABI of the MI355X-native BEVBert cross-modal hot path (gfx950 only).
 *
 * The reference (MarSaKi/VLN-BEVBert) has no native/plugin layer: its hot path is Python nn.Modules over ATen,
 * torch_scatter and nn.MultiheadAttention.  This header is the boundary a reference maintainer binds with ctypes
 * (INTEGRATION.md shows the stubs); each entry names the reference code it replaces (paths under /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; the caller owns all memory, nothing is allocated,
 *     retained or freed here.  Process-wide state, all of it: (1) bevbert_gemm's mutex-guarded plan cache (library
 *     handle + per-shape descriptors), (2) the step-salt POINTER registered by bevbert_set_step_salt (one per process:
 *     two training loops in one process share the salt word -- their masks still differ through their seeds) and the slot array
 *     registered by bevbert_set_fold_norm_slots, (3) the environment switches read by capi.hip (A/B knobs).  Entries may be called concurrently from several threads on
 *     different streams; bevbert_set_step_salt must not race with launches;
 *   - `stream` is a hipStream_t (PyTorch-ROCm: torch.cuda.current_stream().cuda_stream); launches are asynchronous;
 *   - return value 0 = ok, <0 = error (-1 invalid argument, -2 launch failure, -3 unsupported); the message is
 *     available from bevbert_last_error() (thread-local);
 *   - dtype codes: 0 = float32, 1 = bfloat16, 2 = float16; parameters (bias, gamma, beta) and statistics are always
 *     float32; arithmetic is float32 everywhere except the MFMA operands of the bf16 attention path and of the float16
 *     attention forward (bevbert_attn_f16_fwd); float16 is taken by that entry, the bevbert_vit_* row kernels and the GEMMs;
 *   - dropout masks are a pure function of (seed, offset, flat element index) -- a 32-bit site key from (seed, offset),
 *     16 random bits per element, two elements per 32-bit mix: backward entries regenerate the forward's mask from
 *     the same (seed, offset) instead of storing it.  Attention indexes its elements as
 *     ((b*nh + h)*Lq + q) * Lk2 + k with Lk2 = Lk rounded up to even.
 */
#ifndef BEVBERT_HIP_H
#define BEVBERT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define BEVBERT_F32 0
#define BEVBERT_BF16 1
#define BEVBERT_F16 2

const char* bevbert_last_error(void);
int bevbert_version(void); /* major*10000 + minor*100 + patch */
/* drain the HIP runtime's sticky last-error slot after a FAILED stream capture (the stale code would otherwise be
 * reported by the next launch check of any library in the process); returns the number of errors dropped. */
int bevbert_hip_error_reset(void);
const char* bevbert_arch(void);
/* name of the kernel the calling thread's last bevbert_attn_fwd (backward = 0) / bevbert_attn_bwd (backward = 1) call was
 * dispatched to ("attn_fwd4", "attn_bwd3", "attn_short_fwd", ...; "" before the first call).  The choice depends on
 * shape, dtype, dropout and the BEVBERT_ATTN_* environment knobs; tests and bench.py use this to prove which path ran. */
const char* bevbert_attn_last_path(int backward);
/* The same choice without a call: the kernel bevbert_attn_fwd (backward = 0) / bevbert_attn_bwd (backward = 1) would take
 * for this shape with suitably aligned operands, under the BEVBERT_ATTN_* knobs the environment holds right now.  has_* /
 * want_dbias say which optional pointers the call would pass; ncu is the CU count the occupancy rule of the persistent
 * forward plans for (<= 0: this device's).  Launches nothing, and with ncu > 0 touches no device; "" for a dtype / impl
 * pair the calls reject. */
const char* bevbert_attn_plan(int B, int nh, int Lq, int Lk, int dtype, int impl, int has_key_mask, int has_bias,
                              float drop_p, int has_bits, int bits_ready, int want_dbias, int ncu, int backward);

/* ---------------------------------------------------------------------------------------------------------------
 * K1  lift + BEV binning + deterministic scatter-mean.
 * Replaces PointCloud.forward (pretrain_src/model/bev_utils.py:349-378), the world->ego transform of
 * GlocalTextPathCMTPreTraining.lift_splat (pretrain_src/model/pretrain_cmt.py:124-137), and
 * PointCloud.project_bev + torch_scatter.scatter_mean (bev_utils.py:381-430; fine-tune twin
 * map_nav_src/models/bev_utils.py:381-417, map_nav_src/r2r/agent.py:143-192).
 *
 * bevbert_bev_lift_bin: depths (B,V,hw,hw) stored /depth_scale, T_c2w (B,V,4,4), T_w2c (B,4,4), S_w2c (B,3),
 *   pix_scale (hw) = ((u + .5 - c)/f) fp32.  Outputs: cell (B,P) int32 (cell id = dim*z + x, -1 = dropped),
 *   order (B,P) int32 (point ids sorted by (cell, id)), cell_start (B, dim*dim+1) int32.  P = V*hw*hw <= 24576.
 * bevbert_bev_bin_points: same outputs from ready-made ego-frame points (B,P,3) + drop mask (B,P) uint8.
 * bevbert_bev_splat_mean: out[b,cell,:] = mean of feat[b,p,:] over the cell's points (0 if empty);
 *   semantics: sem_ids (B,P) uint8 class ids  XOR  sem_dense (B,P,S) float64 one-hot (the reference's format);
 *   out_sem (B,K,S) uint8 {0,1}, out_sem_mask (B,K) uint8; pass out_sem = NULL to skip semantics.
 *   sample_rows (B, rows_per_sample) int32 or NULL: feat / sem_ids are a device-resident store of per-viewpoint grid
 *   features ((N, P/rows_per_sample, C) / (N, P/rows_per_sample); dataset.py:110-118) read in place -- no batch copy:
 *   sample b's points p*P0 .. (p+1)*P0-1 are store row sample_rows[b][p].  rows_per_sample = 1 in pre-training; the
 *   fine-tuning agent splats the current viewpoint together with its visited neighbours (GraphMap.gather_node_pc,
 *   map_nav_src/models/graph_utils.py:129-144; agent.py:282-296), rows_per_sample = the batch maximum, short lists
 *   padded with any valid row whose depths are 0 (those points are dropped by the binning). */
int bevbert_bev_lift_bin(const float* depths, const float* T_c2w, const float* T_w2c, const float* S_w2c,
                         const float* pix_scale, int B, int V, int hw, float depth_scale, int dim, float res,
                         float y_clip, int* cell, int* order, int* cell_start, hipStream_t stream);
int bevbert_bev_bin_points(const float* points, const uint8_t* drop_mask, int B, int P, int dim, float res,
                           float y_clip, int* cell, int* order, int* cell_start, hipStream_t stream);
int bevbert_bev_splat_mean(const void* feat, int feat_dtype, const int* order, const int* cell_start, void* out,
                           int out_dtype, int B, int P, int K, int C, const uint8_t* sem_ids, const double* sem_dense,
                           int S, uint8_t* out_sem, uint8_t* out_sem_mask, const int* sample_rows, int rows_per_sample,
                           hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K2  fused multi-head attention (head_dim 64).
 * Replaces BertSelfAttention.forward (pretrain_src/model/vilmodel.py:103-141), BertOutAttention.forward
 * (vilmodel.py:325-352) and nn.MultiheadAttention inside TransformerEncoderLayer.forward_pre
 * (pretrain_src/model/transformer.py:170-182): softmax(Q K^T * scale + key_mask[b,k] + bias[b,q,k]) V with dropout
 * on the probabilities.  q/k/v/o are (B, L, nh*64) views with row/batch strides (elements):
 *   strides[8] (host) = {ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso}; dq/dk/dv use the q/k/v strides, dout the o strides.
 * key_mask (B,Lk) and bias (B,Lq,Lk) are additive fp32 (NULL = none; -inf allowed); lse (B,nh,Lq) fp32.
 * impl: 0 = auto (bf16 -> MFMA kernels, f32 -> exact fp32 kernels), 1 = exact kernels, 2 = MFMA kernels.
 * bwd: delta_ws is a (B,nh,Lq) fp32 scratch; dbias (B,nh,Lq,Lk) fp32 receives the PER-HEAD bias gradients (written,
 * not accumulated: the bias is shared by the heads and the caller sums dim 1 in a fixed order -- no atomics), NULL to
 * skip. */
int bevbert_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* key_mask,
                     const float* bias, const int64_t* strides, int B, int nh, int Lq, int Lk, int head_dim,
                     float scale, int dtype, int impl, float drop_p, uint64_t seed, uint64_t offset,
                     uint64_t* drop_bits, int bits_ready, hipStream_t stream);
int bevbert_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                     float* delta_ws, void* dq, void* dk, void* dv, float* dbias, const float* key_mask,
                     const float* bias, const int64_t* strides, int B, int nh, int Lq, int Lk, int head_dim,
                     float scale, int dtype, int impl, float drop_p, uint64_t seed, uint64_t offset,
                     const uint64_t* drop_bits, hipStream_t stream);
/* drop_bits (may be NULL): keep-bit workspace of the dropout mask on the attention probabilities (nn.Dropout,
 * vilmodel.py:134), bevbert_attn_drop_bits_words(B, nh, Lq, Lk) 64-bit words: the mask as one bit per score element,
 * once in the lane layout of the forward's accumulators and once in the backward's.  The bf16 kernels read the bits with
 * scalar loads and drop with one select per element instead of hashing per element.  bevbert_attn_drop_bits fills the
 * workspace (any stream, any time before the forward: the mask is a pure function of seed, offset, step salt and
 * element index); bevbert_attn_fwd does that itself first when bits_ready == 0.  NULL: both directions derive the mask
 * from (seed, offset) inline (round-2 kernels) -- same mask, more arithmetic. */
int64_t bevbert_attn_drop_bits_words(int B, int nh, int Lq, int Lk);
int bevbert_attn_drop_bits(uint64_t* drop_bits, int B, int nh, int Lq, int Lk, float drop_p, uint64_t seed,
                           uint64_t offset, hipStream_t stream);
/* 1: fill the workspace of this dropout site ahead of its forward (bevbert_attn_drop_bits, then bits_ready = 1); 0: pass
 * bits_ready = 0 -- the forward hashes inline and leaves the bits behind for the backward (small score matrices). */
int bevbert_attn_bits_ahead(int Lq, int Lk, int has_bias);

/* Float16 attention forward (since 0.5.0; entry point added, ABI otherwise unchanged; csrc/attn_fwd2.hip): the attention of
 * the CLIP image encoder's float16 mode, inference only.  o = softmax(q k^T * scale) v with fp16 q / k / v / o (B, L, nh*64)
 * and the stride block of bevbert_attn_fwd; no key mask, no bias, no dropout, no lse.  Any Lq, Lk >= 1, head_dim 64.
 * Scores, maximum and row sum are fp32; P is rounded to fp16 (nearest even) for the P V product, which accumulates in
 * fp32; the quotient by the row sum is rounded to fp16 once and overflows to inf as IEEE fp16 does.  Pointers 16-byte
 * aligned, strides multiples of 8 elements.  bevbert_attn_fwd / _bwd / bevbert_attn_plan keep rejecting dtype 2. */
int bevbert_attn_f16_fwd(const void* q, const void* k, const void* v, void* o, const int64_t* strides, int B, int nh, int Lq,
                         int Lk, int head_dim, float scale, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K3  y = LayerNorm(dropout(x + bias) + residual).
 * Replaces BertSelfOutput.forward / BertOutput.forward (vilmodel.py:150-154,189-193) and every bare LayerNorm of the
 * path (bias/residual NULL).  z_out (optional) receives the pre-norm sum for the backward; mean/rstd optional.
 * bwd: dz = grad wrt the pre-norm sum (= grad of residual), dx = grad wrt the dense output (dz through the dropout
 * mask; pass NULL when p == 0 and use dz); dgamma/dbeta/dbias (H) fp32 are written or accumulated (accumulate != 0);
 * workspace: bevbert_colsum_workspace_floats(3*H) floats. */
int bevbert_bias_dropout_residual_layernorm_fwd(const void* x, const float* bias, const void* residual,
                                                const float* gamma, const float* beta, void* y, void* z_out,
                                                float* mean, float* rstd, int rows, int H, float eps, int dtype,
                                                float drop_p, uint64_t seed, uint64_t offset, hipStream_t stream);
/* y = LayerNorm(x + bias) + post1 + post2 (post terms optional, same dtype / shape as y, added in that order after the
 * affine): the sums that follow a LayerNorm in the embedding compositions -- ImageEmbeddings (vilmodel.py:494-532:
 * LN(img) + LN(loc) + nav_type ...) and bev_input_embedding (:589-593) -- ride on its store instead of being separate
 * element-wise launches.  Backward: bevbert_layernorm_bwd with dy (the post terms receive dy unchanged). */
int bevbert_layernorm_post_fwd(const void* x, const float* bias, const float* gamma, const float* beta,
                               const void* post1, const void* post2, void* y, void* z_out, float* mean, float* rstd,
                               int rows, int H, float eps, int dtype, hipStream_t stream);
int bevbert_layernorm_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                          void* dz, void* dx, float* dgamma, float* dbeta, float* dbias, float* workspace, int rows,
                          int H, int dtype, float drop_p, uint64_t seed, uint64_t offset, int accumulate,
                          hipStream_t stream);
/* bevbert_layernorm_bwd with an addend: dz (and dx behind the dropout mask) = LayerNorm's input gradient + dz_add, the
 * gradient that reaches z through its second consumer when z is also a module output (pre-norm residual stream of the
 * panorama encoder, pretrain_src/model/transformer.py:170-182). */
int bevbert_layernorm_bwd_add(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                              void* dz, void* dx, const void* dz_add, float* dgamma, float* dbeta, float* dbias,
                              float* workspace, int rows, int H, int dtype, float drop_p, uint64_t seed, uint64_t offset,
                              int accumulate, hipStream_t stream);
/* The LayerNorm pair with an fp32 RESIDUAL STREAM around bf16 matrix operands -- what torch.autocast does to these modules
 * (pretrain_src/train_r2r.py:256-258: LayerNorm outputs and residual sums stay fp32, only GEMM operands are rounded).
 * fwd: x bf16 (dense output), residual fp32 or bf16 (residual_dtype: 0 / 1) or NULL; y16 = bf16(y) for the next GEMMs,
 * y32 = y (fp32) for the next residual add, z32 = the pre-norm sum in fp32 (y32 / z32 / mean / rstd may be NULL).
 * bwd: the output gradient is dy16 (bf16, from the GEMMs that read y16) + dy32 (fp32, from the residual add that read
 * y32), either may be NULL; dz32 (fp32) = gradient w.r.t. the residual, dx16 (bf16) = gradient w.r.t. the dense output
 * (dz through the dropout mask); parameter gradients and workspace as in bevbert_layernorm_bwd. */
int bevbert_layernorm_res32_fwd(const void* x, const float* bias, const void* residual, int residual_dtype,
                                const float* gamma, const float* beta, void* y16, float* y32, float* z32, float* mean,
                                float* rstd, int rows, int H, float eps, float drop_p, uint64_t seed, uint64_t offset,
                                hipStream_t stream);
/* bevbert_layernorm_res32_fwd for a residual that is the fp32 output of the PREVIOUS LayerNorm of the stream, when that
 * call wrote no y32 (since 0.3.0; entry point added, ABI otherwise unchanged): the residual is recomputed as
 * (z_prev - mean_prev) * rstd_prev * gamma_prev + beta_prev from the previous call's z32, mean, rstd (all required, fp32)
 * and its gamma / beta, with the arithmetic that call would have used for its y32 -- bit for bit the same results. */
int bevbert_layernorm_res32_chain_fwd(const void* x, const float* bias, const float* z_prev, const float* mean_prev,
                                      const float* rstd_prev, const float* gamma_prev, const float* beta_prev,
                                      const float* gamma, const float* beta, void* y16, float* y32, float* z32,
                                      float* mean, float* rstd, int rows, int H, float eps, float drop_p, uint64_t seed,
                                      uint64_t offset, hipStream_t stream);
int bevbert_layernorm_res32_bwd(const void* dy16, const float* dy32, const float* z32, const float* mean,
                                const float* rstd, const float* gamma, void* dz, void* dx16, float* dgamma,
                                float* dbeta, float* dbias, float* workspace, int rows, int H, float drop_p, uint64_t seed,
                                uint64_t offset, int accumulate, int dz_dtype,
                                hipStream_t stream);
int64_t bevbert_colsum_workspace_floats(int total_cols);
/* Split form of the parameter-gradient reductions: bevbert_layernorm_bwd / bevbert_bias_gelu_bwd called with NULL
 * dgamma/dbeta/dbias leave per-block partial sums [bevbert_colsum_partial_rows(rows)][nwhich][C] (nwhich = 3 for
 * LayerNorm: dgamma, dbeta, dbias; 1 for GELU) in `workspace`; bevbert_colsum_finalize folds them into the outputs
 * (written, or accumulated when accumulate != 0; NULL outputs are skipped) -- typically on another stream. */
int bevbert_colsum_partial_rows(int rows);
int bevbert_colsum_finalize(const float* partials, int nblocks, int nwhich, int C, float* out0, float* out1,
                            float* out2, int accumulate, hipStream_t stream);
/* Batched second stage.  bevbert_colsum_partials = the first stage of bevbert_colsum alone.  bevbert_multi_finalize runs
 * `ntasks` 64-column finalize tasks in ONE launch; `tasks` is a device array of 40-byte records
 * {u64 partials, u64 out, i32 nblocks, i32 row_stride, i32 col0, i32 ncols, i32 accumulate, i32 pad}:
 * out[c] (+)= sum_b partials[b * row_stride + col0 + c], c < ncols <= 64, fixed summation order (deterministic). */
int bevbert_colsum_partials(const void* dy, float* partials, int rows, int C, int dtype, hipStream_t stream);
int bevbert_multi_finalize(const void* tasks, int ntasks, hipStream_t stream);
/* Batched bevbert_accum_partials: `tasks` = device array of 40-byte records
 * {u64 partials, u64 sink, u64 n4_total, u32 off4, u32 n4, i32 S, i32 dtype}: for the n4 float4 groups starting at
 * off4, sink[i] += sum_{s < S} partials[s * n4_total + off4 + i] (sink already points at the range's first element).
 * The dtype field carries two task flags above the dtype code (bits 0-7); records with them clear behave as above.
 *   bit 8  STORE: the caller guarantees that the sink range is zero (the gradient arena's fill, nothing added since): the
 *          sum starts from 0.f -- ((0 + p0) + p1) + ..., bit for bit what accumulating into zeros gives -- and the sink
 *          is not read.
 *   bit 9  NORM:  the sum of squares of the values the task stores goes to slots[dtype >> 12] of the array registered
 *          with bevbert_set_fold_norm_slots (one writer per slot, fixed order, no atomics); ignored when no array is
 *          registered or the slot lies beyond its capacity. */
int bevbert_multi_accum(const void* tasks, int ntasks, hipStream_t stream);
/* The fused gradient norm.  bevbert_set_fold_norm_slots registers (NULL / 0: clears) a device array of `capacity`
 * floats, process-wide like the step salt; the pointer is read at launch time and passed to the kernels as an argument,
 * so a captured launch keeps the array it was captured with.  bevbert_sumsq_tasks fills the slots of what no NORM fold
 * covers: `tasks` = device array of 16-byte records {u64 ptr, u32 n4, u32 slot}, slots[slot] = sum of squares of the
 * n4 <= 4096 float4 groups at ptr, one workgroup per record. */
int bevbert_set_fold_norm_slots(float* slots, int capacity);
int bevbert_sumsq_tasks(const void* tasks, int ntasks, hipStream_t stream);

/* K5  BertEmbeddings.forward (vilmodel.py:62-77): y = LayerNorm(word[ids] + pos[row % L] + type_row) (+dropout). */
int bevbert_embed_sum_layernorm_fwd(const int64_t* ids, const void* word, const void* pos, const void* type_row,
                                    const float* gamma, const float* beta, void* y, void* z_out, float* mean,
                                    float* rstd, int rows, int L, int H, float eps, int dtype, float drop_p,
                                    uint64_t seed, uint64_t offset, hipStream_t stream);

/* backward of the word-embedding gather of BertEmbeddings (vilmodel.py:50,67): table_grad[t, :] += sum of d[r, :] over
 * the rows with ids[r] == t, rows with ids[r] == padding_idx skipped (nn.Embedding(padding_idx=0); -1: none).  No
 * atomics: the first row of every id sums its id's rows in ascending row order (four waves, one contiguous quarter of
 * the row range each, folded pairwise), so the result is a pure function of the inputs.  H % 4 == 0, H <= 1024. */
int bevbert_embedding_grad(const int64_t* ids, const void* d, float* table_grad, int rows, int H, int padding_idx,
                           int dtype, hipStream_t stream);

/* Feature projections with a tiny inner dimension fused into their LayerNorm (pretrain_src/model/vilmodel.py:507-518
 * loc_layer_norm(loc_linear(loc_fts)), :577-583 bev_pos_embeddings, :589-593 gmap_pos_embeddings):
 *   y = (LayerNorm(feat W^T + bias) + post1) + table[idx]      feat (rows, K) fp32, K <= 16; weight (H, K) fp32 (nn.Linear
 * layout); post1 (rows, H) and table (T, H) of ``dtype`` or NULL; idx (rows) int64 (with table).  mean / rstd (rows) are left
 * for the backward, which RECOMPUTES feat W^T (no z tensor is stored, no dz tensor written): it adds the gradients of
 * weight (H, K), bias, gamma, beta into the given fp32 buffers (NULL: skipped) through per-workgroup partial sums in
 * ``workspace`` (bevbert_smallk_workspace_floats(rows, K, H) floats), folded in a fixed order.  d post1 = d table rows = dy.
 * H in {256, 512, 768, 1024}; (K + 8) * H * 4 bytes must fit 64 KB of LDS. */
int64_t bevbert_smallk_workspace_floats(int rows, int K, int H);
int bevbert_smallk_linear_layernorm_fwd(const float* feat, const float* weight, const float* bias, const float* gamma,
                                        const float* beta, const void* post1, const void* table, const int64_t* idx,
                                        void* y, float* mean, float* rstd, int rows, int K, int H, float eps, int dtype,
                                        hipStream_t stream);
int bevbert_smallk_linear_layernorm_bwd(const void* dy, const float* feat, const float* weight, const float* bias,
                                        const float* mean, const float* rstd, const float* gamma, float* dweight,
                                        float* dbias, float* dgamma, float* dbeta, float* workspace, int rows, int K,
                                        int H, int dtype, hipStream_t stream);

/* column sums for any column count (C % 4 != 0: the 30 522-wide vocabulary bias, the 1-wide prediction heads):
 * out[c] (+)= sum_r dy[r][c], fixed summation order. */
int bevbert_colsum_any(const void* dy, float* out, int rows, int C, int dtype, int accumulate, hipStream_t stream);

/* loss.mean() of the step (pretrain_src/train_r2r.py:263) over a static batch's rows: *out = sum_i w[i] x[i] / denom (w NULL:
 * ones -- zero for the padding rows of a static batch; denom_dev, if given, is read from device memory: the row count of
 * the batch that currently sits in the buffers); bwd: dx[i] = w[i] * *dout / denom. */
int bevbert_weighted_mean_fwd(const float* x, const float* w, const float* denom_dev, float denom, int n, float* out,
                              hipStream_t stream);
int bevbert_weighted_mean_bwd(const float* dout, const float* w, const float* denom_dev, float denom, int n, float* dx,
                              hipStream_t stream);

/* Semantic head's loss (pretrain_src/model/pretrain_cmt.py:391-441).  sem_select: row numbers of the cells with mask1 (and
 * mask2, if given) set, compacted in ascending order into idx (cap entries; padding: row 0), valid[i] = 1 for the real ones,
 * *denom = count x classes -- one workgroup, no host sync for the data-dependent count.  bce_rows_fwd: out[r] = sum over the
 * C classes of binary_cross_entropy_with_logits(logits[r, c], labels[idx[r], c]) (labels uint8 {0, 1}; idx NULL: row r);
 * bce_rows_bwd: dlogits[r, c] = (sigmoid(logits[r, c]) - label) * g[r]. */
int bevbert_sem_select(const uint8_t* mask1, const uint8_t* mask2, int n, int cap, int classes, int64_t* idx, float* valid,
                       float* denom, hipStream_t stream);
int bevbert_bce_rows_fwd(const void* logits, const uint8_t* labels, const int64_t* idx, float* out, int rows, int C, int dtype,
                         hipStream_t stream);
int bevbert_bce_rows_bwd(const void* logits, const uint8_t* labels, const int64_t* idx, const float* g, void* dlogits, int rows,
                         int C, int dtype, hipStream_t stream);

/* Graph-aware attention bias of the global-map encoder (pretrain_src/model/vilmodel.py:543-546,575-577: sprel_linear =
 * nn.Linear(1, 1) over the pairwise node distances).  fwd: out[i] = dists[i] * *w + *b (w, b: the parameters in device
 * memory).  bwd: *dw += sum dbias * dists, *db += sum dbias over the (layers, B, nh, G, G) per-head bias gradients the
 * attention backward leaves for every layer that used the bias (dists: (B, G, G)); two stages, fixed summation order. */
int bevbert_graph_bias_fwd(const float* dists, const float* w, const float* b, float* out, int64_t n, hipStream_t stream);
int bevbert_graph_bias_bwd(const float* dbias, const float* dists, int layers, int B, int nh, int G, float* dw, float* db,
                           float* workspace /* 1024 floats */, hipStream_t stream);

/* Row selection of activations and its backward (the reference indexes with boolean masks / index tensors:
 * pretrain_src/model/pretrain_cmt.py:254-256 masked tokens of the MLM head, :321-326 candidate cells of the SAP head, :403-410
 * supervised cells of the semantic head).  rows_gather: out[i, :] = src[ids[i], :].  rows_scatter: out[t, :] (+)= sum of
 * d[r, :] over the rows with ids[r] == t, for the ids that occur -- the caller zeroes ``out`` first (bevbert_zero);
 * accumulate = 1 adds to what the row holds (a second selection from the same tensor).  Duplicate ids are summed by the
 * first row of the id in ascending row order (no atomics, as bevbert_embedding_grad).  H % 4 == 0, H <= 1024. */
int bevbert_rows_gather(const void* src, const int64_t* ids, void* out, int rows, int H, int dtype, hipStream_t stream);
int bevbert_rows_scatter(const int64_t* ids, const void* d, void* out, int rows, int H, int dtype, int accumulate,
                         hipStream_t stream);

/* backward of nn.Embedding lookups on SMALL tables (vilmodel.py:452 nav_type_embedding, :567 gmap_step_embedding, the
 * token-type row): partials[s][t][:] = sum of d[r, :] over the rows r of slice s (rows_per_slice rows each) with
 * ids[r] == t; ceil(rows / rows_per_slice) slices of table_rows * H floats, folded into the table gradient by the
 * second stage of the column reductions (bevbert_multi_finalize with row_stride = table_rows * H).  No atomics: the
 * summation order is fixed. */
int bevbert_embedding_grad_sliced(const int64_t* ids, const void* d, float* partials, int rows, int H, int table_rows,
                                  int rows_per_slice, int dtype, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K4  y = gelu_erf(x + bias)  -- BertIntermediate.forward + gelu (vilmodel.py:31-37,177-180); F.gelu in the pano
 * encoder (transformer.py:178).  bwd: dx = dy * gelu'(x + bias) (dx may alias dy), dbias (C) written/accumulated. */
int bevbert_bias_gelu_fwd(const void* x, const float* bias, void* y, int rows, int C, int dtype, hipStream_t stream);
int bevbert_bias_gelu_bwd(const void* dy, const void* x, const float* bias, void* dx, float* dbias, float* workspace,
                          int rows, int C, int dtype, int accumulate, hipStream_t stream);
/* the same pair with ReLU: the prediction heads' Linear -> ReLU -> LayerNorm -> Linear (pretrain_src/model/pretrain_cmt.py:34-71;
 * the Linear's bias rides on the activation kernel, its gradient on the activation's backward) */
int bevbert_bias_relu_fwd(const void* x, const float* bias, void* y, int rows, int C, int dtype, hipStream_t stream);
int bevbert_bias_relu_bwd(const void* dy, const void* x, const float* bias, void* dx, float* dbias, float* workspace,
                          int rows, int C, int dtype, int accumulate, hipStream_t stream);
/* out[c] (+)= sum_r dy[r,c]: bias gradients of the projection GEMMs (autograd's grad.sum(0) in the reference). */
int bevbert_colsum(const void* dy, float* out, float* workspace, int rows, int C, int dtype, int accumulate,
                   hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K6  out[r] = sum_e w[e] * src[idx[e]], e in [rowptr[r], rowptr[r+1])  -- GlobalMapEncoder._aggregate_gmap_features
 * (vilmodel.py:632-666) with the visited/unvisited bookkeeping turned into a CSR on the host; the backward is the
 * same call on the transposed CSR. */
int bevbert_segment_wsum(const void* src, const int* rowptr, const int* idx, const float* w, void* out, int out_rows,
                         int H, int dtype, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K7  flat-arena optimiser.  All parameters / gradients / Adam moments live in contiguous fp32 arenas whose tensors
 * start on 1024-element boundaries; chunk_flags[n/1024]: bit0 = weight decay applies, bit1 = tensor has had a grad.
 * bevbert_grad_norm_clip: scalars[0] = ||pre_scale * g||_2, scalars[1] = pre_scale * min(1, max_norm/(norm+1e-6))
 *   (torch.nn.utils.clip_grad_norm_ as called at pretrain_src/train_r2r.py:295-306; pre_scale folds DDP's 1/world).
 *   partials: 1024 floats scratch.  No host sync: adamw_step reads the multiplier from device memory.
 * bevbert_adamw_step: AdamW.step (pretrain_src/optim/adamw.py:53-112): bias-corrected Adam, decoupled decay applied
 *   after the update; optionally refreshes the bf16 shadow copy of the parameters in the same pass.  chunk_steps
 *   (int32 per 1024-element chunk, zero-initialised by the caller) is the reference's per-parameter state["step"]:
 *   it advances only for chunks whose flag bit1 is set, so a parameter first used at step 6 starts at t = 1.
 *   lr_dev (may be NULL): learning rate read from device memory instead of the `lr` argument, so that a step captured
 *   in a hipGraph follows the schedule (optim/sched.py:24-30) without being re-captured. */
int bevbert_grad_norm_clip(const float* grads, int64_t n, float pre_scale, float max_norm, float* partials,
                           float* scalars, hipStream_t stream);
/* bevbert_grad_norm_clip's second half alone, over `n` sums of squares that NORM folds and bevbert_sumsq_tasks left in
 * `slots`: fp64 sum in a fixed order, the same scalars[0..1]. */
int bevbert_clip_from_slots(const float* slots, int n, float pre_scale, float max_norm, float* scalars,
                            hipStream_t stream);
int bevbert_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* params_bf16,
                       const uint8_t* chunk_flags, int* chunk_steps, int64_t n, const float* grad_scale_dev,
                       const float* lr_dev, float lr, float beta1, float beta2, float eps, float weight_decay,
                       hipStream_t stream);
int bevbert_cast_f32(const float* src, void* dst, int64_t n, int dst_dtype, hipStream_t stream);
/* zero ``bytes`` bytes on the stream with a memset command (optimizer.zero_grad() of the flat gradient arena,
 * pretrain_src/train_r2r.py:313; a memset node when the step is captured) */
int bevbert_zero(void* p, int64_t bytes, hipStream_t stream);
/* sink[i] += sum_{s<S} partials[s*n + i]: reduction of the host-side split-K weight-gradient GEMMs (library batched
 * GEMM over S chunks of the token axis), fused with the accumulation into the fp32 gradient arena. */
int bevbert_accum_partials(const void* partials, float* sink, int S, int64_t n, int dtype, hipStream_t stream);

/* ---- library GEMM (hipBLASLt) with cached per-shape plans ---------------------------------------------------------
 * Replaces every nn.Linear matmul of the path (pretrain_src/model/vilmodel.py:92-94,314-316 query/key/value,
 * :146,:171,:185,:247,:261,:281 dense/decoder layers, :469-475,:542,:577-581,:621 input projections;
 * pretrain_cmt.py:38-68 prediction heads) and their two backward GEMMs, which PyTorch dispatches to the same
 * library at ~4x the host cost per call.
 *   C[M x N] = alpha * op(A)[M x K] . op(B)[K x N] (+ bias[N]),  row-major, optionally strided-batched.
 *   opA == 0: A stored M x K with row stride lda;  opA == 1: A stored K x M (row stride lda), used transposed.
 *   opB == 0: B stored K x N with row stride ldb;  opB == 1: B stored N x K (row stride ldb), used transposed.
 * in_dtype in {F32, BF16, F16 (since 0.5.0)}; out_dtype == in_dtype or F32; bias (may be NULL) has dtype bias_dtype (F32 or
 * out_dtype).
 * autotune > 1: on the first call of a problem, time the library's top `autotune` (<= 64) heuristic candidates on the
 * given operands (the product is recomputed, beta == 0) and keep the fastest; a problem listed in an imported tuning
 * table starts with the recorded choice instead.  Returns BB_EUNSUPPORTED (-3) when the
 * library has no kernel for the problem.
 * bevbert_gemm_plan / bevbert_gemm_run split the same call in two so that the per-call path carries 8 arguments:
 * plan returns an id >= 0 (cached by problem; bias_dtype < 0 = no bias; accumulate != 0: C += product, used by the
 * weight-gradient GEMMs that add into the fp32 gradient arena) or a negative error; run executes it (and autotunes
 * on its first call).  `workspace_bytes` at run time must be >= the value the plan was made with. */
int bevbert_gemm(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int opA, int opB,
                 int64_t lda, int64_t ldb, int64_t ldc, int batch, int64_t stride_a, int64_t stride_b,
                 int64_t stride_c, int in_dtype, int out_dtype, int bias_dtype, float alpha, void* workspace,
                 int64_t workspace_bytes, int autotune, hipStream_t stream);
int bevbert_gemm_plan(int M, int N, int K, int opA, int opB, int64_t lda, int64_t ldb, int64_t ldc, int batch,
                      int64_t stride_a, int64_t stride_b, int64_t stride_c, int in_dtype, int out_dtype, int bias_dtype,
                      int accumulate, int64_t workspace_bytes, int autotune);
int bevbert_gemm_run(int plan, const void* A, const void* B, void* C, const void* bias, void* workspace,
                     int64_t workspace_bytes, hipStream_t stream);
/* D = op(A) . op(B) + Cin through an ACCUMULATING plan (beta = 1) with a separate addend of D's layout. */
int bevbert_gemm_run_add(int plan, const void* A, const void* B, const void* Cin, void* D, const void* bias,
                         void* workspace, int64_t workspace_bytes, hipStream_t stream);
int bevbert_gemm_plan_count(void);
/* library algorithms dropped so far because two launches on the same operands left different output bits (split-K /
 * stream-K reductions through atomics): plans only ever use algorithms whose results repeat (BEVBERT_GEMM_DETERMINISTIC=0
 * turns the screening off). */
int bevbert_gemm_rejected_count(void);
/* Tuning table (text): one line "<problem key> <choice> <ncand>" per autotuned plan after a header naming the hipBLASLt
 * version.  export returns the bytes the text needs (incl. the final 0) and fills buf when cap suffices; import makes
 * later plans reuse the recorded choice instead of timing candidates (returns the number of rows; -3 when the table
 * belongs to another library version).  Shipping a table makes runs start tuned and removes run-to-run variation of
 * the picks (and timing candidates under a profiler is unreliable). */
int64_t bevbert_gemm_tuning_export(char* buf, int64_t cap);
int bevbert_gemm_tuning_import(const char* text);

/* y = residual + dropout(x) over n (multiple of 4) elements; residual may be NULL, y may alias x when the dtypes match.
 * Replaces the bare nn.Dropout sites of the path: feature dropout of the loader's fp32 features fused with their cast
 * to the compute dtype (pretrain_cmt.py:102-106 drop_feats; map_nav_src/models/model.py:30-36), the embedding dropout
 * (vilmodel.py:76, :494-496) and the two residual dropouts of TransformerEncoderLayer.forward_pre
 * (transformer.py:170-182).  The backward of x is the same call on dy with residual = NULL. */
int bevbert_dropout_add(const void* x, const void* residual, void* y, int64_t n, int in_dtype, int out_dtype,
                        float drop_p, uint64_t seed, uint64_t offset, hipStream_t stream);

/* Tail of forward_sap (pretrain_src/model/pretrain_cmt.py:225-275) behind the three prediction heads, one launch:
 * fw = sigmoid(fuse_raw) (fuse_raw NULL: 0.5); global logits = global_raw * fw with -inf on visited nodes and beyond
 * gmap_lens; local logits = local_raw * (1 - fw) with -inf where nav_masks[b, cand_idxs[b, k]] == 0; fused logits =
 * global + [local | sum of local over vis_c | 0][src]; loss[b] = CE(global) + CE(local) + CE(fused) (labels:
 * global_labels twice, local_labels).  A label of -100 is ignored as by F.cross_entropy's ignore_index: global -100
 * drops the global and the fused term, local -100 the local term; a dropped term adds 0 to loss[b] and nothing to dG /
 * dL / dF, the other terms are unchanged; other labels outside [0, G) / [0, K) are the caller's error.  dG (B,G) /
 * dL (B,K) / dF (B): fp32 gradients w.r.t. global_raw / local_raw / fuse_raw for dloss[b] = 1.  bool tensors are
 * bytes.  G <= 64, K <= 62.  bevbert_sap_loss_bwd: d_*_raw = d* * dloss[b] in the heads' dtype (d_fuse_raw may be NULL). */
int bevbert_sap_loss_fwd(const void* global_raw, const void* local_raw, const void* fuse_raw, const uint8_t* visited,
                         const int64_t* gmap_lens, const uint8_t* nav_masks, const int64_t* cand_idxs, const int64_t* src,
                         const uint8_t* vis_c, const int64_t* global_labels, const int64_t* local_labels, float* loss,
                         float* dG, float* dL, float* dF, int B, int G, int K, int P, int dtype, hipStream_t stream);
int bevbert_sap_loss_bwd(const float* dG, const float* dL, const float* dF, const float* dloss, void* d_global_raw,
                         void* d_local_raw, void* d_fuse_raw, int B, int G, int K, int dtype, hipStream_t stream);

/* F.cross_entropy(logits.float(), target, reduction="none") on wide rows -- the MLM head (pretrain_cmt.py:262-266,
 * rows = masked tokens, C = vocabulary): logits are read in their own dtype (bf16 / fp32, rows x C contiguous, base
 * 16-byte aligned, any C), statistics in fp32; loss[r] out, and lse (2 x rows floats) = the row maxima m[r] followed by
 * log sum_c exp(logits[r, c] - m[r]), kept apart so that the backward's softmax does not inherit the rounding of their
 * sum at the size of m.  bwd: lse as the forward left it; dlogits = (softmax - onehot) * dloss[r] in the logits' dtype
 * (dlogits may alias logits).  Targets must lie in [0, C): there is no ignore_index here, static batches pad their rows
 * with target 0 and weight 0 (static_step.py:174). */
int bevbert_cross_entropy_fwd(const void* logits, const int64_t* target, float* loss, float* lse, int rows, int C,
                              int dtype, hipStream_t stream);
int bevbert_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* dloss,
                              void* dlogits, int rows, int C, int dtype, hipStream_t stream);

/* F.kl_div(F.log_softmax(logits.float(), -1), t, reduction="none").sum(1) for finite logits and t >= 0 -- the MRC head
 * (pretrain_cmt.py:272-297, rows = masked objects, C = detector classes).  logits (rows, C) bf16 / fp32, contiguous, base
 * 16-byte aligned, any C >= 1; targets (N, C) f32; idx (rows) i64 or NULL: row r reads targets[idx[r]] (NULL: row r;
 * duplicates allowed).  loss[r] = sum_c xlogy(t, t) - t * ((x - m) - ls) in fp32, a term with t == 0 adds exactly 0.
 * stats (3 x rows floats) = the row maxima m, then ls = log sum_c exp(x - m) (apart, as in cross_entropy_fwd), then
 * S = sum_c t.  bwd: stats as the forward left them; dlogits = (exp((x - m) - ls) * S[r] - t) * dloss[r] in the logits'
 * dtype (dlogits may alias logits) -- the factor S because detector probabilities do not sum to 1 exactly.  targets get no
 * gradient.  C <= 1024: one wave per row, else one workgroup per row; no atomics.  rows <= 0 returns 0; a NULL logits /
 * targets / output pointer with rows > 0 is an argument error (idx alone may be NULL). */
int bevbert_soft_ce_fwd(const void* logits, const float* targets, const int64_t* idx, float* loss, float* stats, int rows,
                        int C, int dtype, hipStream_t stream);
int bevbert_soft_ce_bwd(const void* logits, const float* targets, const int64_t* idx, const float* stats, const float* dloss,
                        void* dlogits, int rows, int C, int dtype, hipStream_t stream);

/* Per-step dropout salt.  Every dropout site derives its mask from hash(seed, offset) -- launch arguments, frozen in a
 * captured hipGraph.  After bevbert_set_step_salt(word) (word: 4 bytes of device memory owned by the caller, NULL to
 * clear) every dropout kernel of the library uses hash(site_key ^ *word): the host rewrites the word once per training
 * step and a replayed graph draws fresh masks; forward and backward of one step read the same word, so they agree.
 * Process-wide setting (the one piece of state besides the hipBLASLt plan cache); set it once, before any launch. */
int bevbert_set_step_salt(const void* device_word);

/* test hook: keep-mask (uint8) the kernels derive for n consecutive elements starting at `offset` */
int bevbert_dropout_keep_mask(uint8_t* out, int64_t n, float drop_p, uint64_t seed, uint64_t offset,
                              hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fine-tune rollout bookkeeping on the device: the B topological maps of a rollout as dense
 * device arrays over a node capacity N.  Replaces map_nav_src/models/graph_utils.py:44-94 (FloydGraph.add_edge / update /
 * path lengths), :96-189 (GraphMap.update_graph, get_pos_fts, gather_node_pc's node choice) and the numeric half of
 * map_nav_src/r2r/agent.py:194-276,326-331 (_nav_gmap_variable, the start-viewpoint position features).  The host keeps
 * only the viewpoint-id -> node-index dictionaries and the presentation order of the nodes.
 * All pointers are device pointers except the state block itself (a host struct of device pointers).  f64 add / compare
 * follow the reference's Python floats bit for bit. */
typedef struct bevbert_gm_state {
  double* pos;        /* (B, N, 3)  node positions */
  double* dis;        /* (B, N, N)  shortest known distances, 95959595 = none (graph_utils.py:46) */
  int* point;         /* (B, N, N)  next hop of the shortest path, -1 = direct edge */
  int* hops;          /* (B, N, N)  len(FloydGraph.path(x, y)), written by bevbert_gm_update */
  uint8_t* visited;   /* (B, N) */
  int* step_ids;      /* (B, N)     agent.py:471-474 */
  int* pc_list;       /* (B, N)     visited nodes in first-visit order (GraphMap.node_pc's dict order) */
  int* npc;           /* (B) */
  int* node_row;      /* (B, N)     feature-store row of a visited node */
  float* node_T;      /* (B, N, V, 16) its V camera-to-world matrices */
  int B, N, V, pad;
} bevbert_gm_state;

/* One navigation step of every episode: live_graph[b] -> register the edges cur[b] -- cand[b, 0..ncand[b]) (positions
 * cur_pos (B,3), cand_pos (B,C,3) and edge lengths cand_dist (B,C), f64, computed by the host with the reference's own
 * arithmetic), relax all pairs through cur[b], mark it visited, rebuild the hop counts of the
 * first n_nodes[b] nodes; live_step[b] -> step_ids[b, cur[b]] = step_id (if > 0) and, when row != NULL and row[b] >= 0,
 * remember the node's feature-store row and poses T (B, V*16). */
int bevbert_gm_update(const bevbert_gm_state* st, const uint8_t* live_graph, const uint8_t* live_step, const int* cur,
                      const int* ncand, const int* cand, const double* cur_pos, const double* cand_pos,
                      const double* cand_dist, const int* n_nodes, int C, int step_id, const int* row, const float* T,
                      hipStream_t stream);

/* The tensors of agent.py:194-276 for the node order node (B, G-1) (cnt[b] real entries per sample, chosen by the host:
 * visited nodes first): step_ids (B,G) i64, visited / masks (B,G) bool bytes, pair (B,G,G) f32 = dis / 30, pos_fts
 * (B,G,7) f32 (row 0 = [stop]); gpos (B,7) or NULL: position features of start[b] seen from cur[b]. */
int bevbert_gm_nav_vars(const bevbert_gm_state* st, const int* node, const int* cnt, const int* cur, const int* start,
                        const double* heading, const double* elevation, int G, int enc_full_graph, int act_visited,
                        int64_t* step_ids, uint8_t* visited, uint8_t* masks, float* pair, float* pos_fts, float* gpos,
                        hipStream_t stream);

/* graph_utils.py:129-144: per sample the visited nodes within `order` hops of cur[b], in first-visit order, as
 * feature-store rows (B,R) (padding repeats the first row with live = 0) and their poses T_c2w (B,R,V*16);
 * *overflow = 1 if a sample has more than R such nodes. */
int bevbert_gm_bev_select(const bevbert_gm_state* st, const int* cur, int order, int R, int* rows, uint8_t* live,
                          float* T_c2w, int* overflow, hipStream_t stream);

/* agent.py:150-156,168-176: the stored views of the selected nodes, out[i] = live[i] ? store[rows[i]] : 0 for i < n_out;
 * store / out rows are row_bytes bytes (V x h x w depths of any element type). */
int bevbert_gm_gather_views(const void* store, const int* rows, const uint8_t* live, void* out, int n_out, int64_t row_bytes,
                            hipStream_t stream);

/* agent.py:485-494 without gradients: embed_sum (B,N,H) / embed_cnt (B,N) running sums of the node embeddings (slot = node
 * index): the current viewpoint's slot is rewritten with avg (B,H), every not-yet-visited candidate j < ncand[b] accumulates
 * pano (B,V,H)[b, j].  live (B) bytes; cand (B,C) node indices (-1 = none). */
int bevbert_gm_embed_update(const bevbert_gm_state* st, void* embed_sum, float* embed_cnt, const void* avg, const void* pano,
                            const uint8_t* live, const int* cur, const int* ncand, const int* cand, int C, int V, int H,
                            int dtype, hipStream_t stream);
/* graph_utils.py:146-147 for the listed nodes: out (B,G,H), row 0 = [stop] = 0, row j = sum / count of node[b, j-1]. */
int bevbert_gm_node_embeds(const bevbert_gm_state* st, const void* embed_sum, const float* embed_cnt, const int* node,
                           const int* cnt, int G, int H, int dtype, void* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fine-tune supervision (since 0.1.2; entry points added, ABI otherwise unchanged).  Replaces map_nav_src/r2r/agent.py:371-417
 * (_teacher_action_r4r), :523-534,559-612 (stop scores, feedback modes, stop rule, stop-node pick), agent_base.py:148 (the
 * IL criterion) and r2r/env.py:309-378 + r2r/eval_utils.py (_eval_item, eval_metrics, cal_dtw, cal_cls).
 * Graph tables (vln_bevbert_amd/nav_expert.py ScanGraphs): dist (S,N,N) f64 = networkx all-pairs Dijkstra lengths (inf =
 * unreachable / padding), pred (S,N,N) i16 = predecessor of v on networkx's path from u (-1 = none).  Node ids are scan
 * indices; ids outside [0, N) read as unreachable.  No entry synchronises with the host. */

/* Expert targets (B) i64: policy 0 = imitation (slot of gt[t+1], 0 at the last gt step), 1 = spl (first strict minimum
 * of d[vp][goal] + d[cur][vp]), 2 = ndtw (first strict minimum of -nDTW(traj ++ path(cur, vp)[1:], gt, 3.0)); slots j >= 1
 * of cand (B,C) (-1 = padding) not flagged in visited (B,C) u8 (may be NULL); 0 when cur is the goal; -100 for ended
 * samples and when every slot is excluded.  gt (B,Lg) + gt_len (B); traj (B,Lt) + traj_len (B) (ndtw only,
 * Lt + N <= 1023). */
int bevbert_nav_expert(const double* dist, const int16_t* pred, int N, int S, const int* scan, const int* cur,
                       const int* cand, const uint8_t* visited, const uint8_t* ended, const int* gt, const int* gt_len,
                       int Lg, const int* traj, const int* traj_len, int Lt, int B, int C, int t, int policy, int64_t* out,
                       hipStream_t stream);

/* One navigation step's decision for B samples from logits (B,C) (dtype 0/1, -inf = masked).  feedback 0 = teacher
 * (targets), 1 = argmax, 2 = sample (inverse CDF of a uniform draw), 3 = expl_sample (first max of the logits = of the probabilities; with
 * probability P(u > expl_max_ratio) a uniform pick among masks (B,C) u8).  Draws (since 0.2.3 in a domain of their own):
 * k = salted(hash(site_key(seed, t) ^ BB_STREAM_NAV)), u0 = 24 bits of hash(k ^ 4 b) (sample; explore or not),
 * u1 = 24 bits of hash(k ^ (4 b + 1)) (which mask slot); salted(x) = hash(x ^ step salt), see csrc/common.h.
 * Live samples store p[0] as the stop score of node cur in stop_scores (B,N) (first-insertion order in stop_order (B,N),
 * n_stop (B)).  Stop: teacher / sample at goal[b], else a == 0; also ended, no_vp_left (may be NULL), t == max_len - 1.
 * Outputs: a_t (B) i64, node (B) = cand[b, a], or -1 when the sample does not move (the reference's None action);
 * just_ended (B) u8 = the sample stops this step (stop rule, no_vp_left, last step) and gets a stop-node pick:
 * stop_node (B) = first max of its stop scores (else -1); entropy (B) f32, rand (B) f32 (the uniform draw used).
 * ended[b] is set for every node == -1, as agent.py:615 does -- also for a live sample whose slot has no viewpoint
 * (slot 0 away from the goal in teacher / sample mode), which ends in place without a stop-node pick.  Stops are
 * signalled by just_ended, not by node == -1. */
int bevbert_nav_action(const void* logits, int dtype, int B, int C, int feedback, int t, int max_len,
                       const int64_t* targets, const int* cand, const int* cur, const int* goal, uint8_t* ended,
                       const uint8_t* no_vp_left, const uint8_t* masks, float* stop_scores, int* stop_order, int* n_stop,
                       int N, float expl_max_ratio, uint32_t seed, int64_t* a_t, int* node, uint8_t* just_ended,
                       int* stop_node, float* entropy, float* rand, hipStream_t stream);

/* CrossEntropyLoss(ignore_index = ignore, reduction='sum') of logits (B,C) (dtype 0/1): out (2B+1) f32 = [lse (B) |
 * per-row loss (B) | sum in row order]; targets equal to ignore or outside [0, C) contribute 0.  bwd: dlogits (B,C) =
 * dloss[0] * (softmax - onehot), 0 on ignored rows. */
int bevbert_nav_ce_fwd(const void* logits, const int64_t* target, float* out, int B, int C, int ignore, int dtype,
                       hipStream_t stream);
int bevbert_nav_ce_bwd(const void* logits, const int64_t* target, const float* out, const float* dloss, void* dlogits,
                       int B, int C, int ignore, int dtype, hipStream_t stream);

/* Trajectory record (graph_utils.py:85-93 FloydGraph.path, agent.py:418-434 / :598-599 the appends): for every b with
 * live[b], n_seg[b] += 1 and traj[b, traj_len[b]..] += the nodes of path(from[b], to[b]) after from[b] (none when equal),
 * expanded from the agent map's next-hop table point (B,Nm,Nm) (-1 = direct edge; bevbert_gm_state.point) and written as
 * node_scan[b, node] (B,Nm) scan indices.  A full record or a table that is not a next-hop table sets *overflow (read it
 * once per episode). */
int bevbert_nav_traj_append(const int* point, int Nm, const int* node_scan, const int* from, const int* to,
                            const uint8_t* live, int* traj, int* traj_len, int Lt, int* n_seg, int* overflow, int B,
                            hipStream_t stream);

/* _eval_item of B finished trajectories, f64: path (B,Lp) = sum(pred_path, []) + path_len (B), action_steps (B) =
 * len(pred_path) - 1, gt (B,Lg) + gt_len (B), margin = ERROR_MARGIN (3.0).  items (B,12): nav_error, oracle_error,
 * action_steps, trajectory_steps, trajectory_lengths, success, spl, oracle_success, DTW, nDTW, SDTW, CLS.  avg (11) or
 * NULL: eval_metrics' means (action_steps, steps, lengths, nav_error, oracle_error, sr, oracle_sr, spl, nDTW, SDTW, CLS;
 * the last six x100), summed in sample order.  Lp < 1024.  A scan index outside [0, S) gives a row of NaN. */
int bevbert_nav_metrics(const double* dist, int N, int S, const int* scan, const int* path, const int* path_len, int Lp,
                        const int* action_steps, const int* gt, const int* gt_len, int Lg, int B, double margin,
                        double* items, double* avg, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Object grounding of the REVERIE / SOON fine-tune rollout (since 0.4.0; entry points added, ABI otherwise unchanged;
 * csrc/nav_obj.hip).  Replaces map_nav_src/reverie/agent_obj.py:343-349 (_nav_obj_variable), :384-400 (_teacher_object),
 * :516-526 (the 'og' record of node_stop_scores), :597-604 (pred_objid) and reverie/env.py:360-411 (_eval_item,
 * eval_metrics).  Fixed shapes, lengths read on the device, no atomics, no entry synchronises with the host: every launch
 * can sit inside a captured step. */

/* Object rows of a panorama: obj (B,Op,H) dtype 0/1 with obj[b, j] = pano[b, view_len[b] + j] (pano (B,L,H)) for
 * j < obj_len[b] and 0 otherwise; mask (B,Op) u8 = j < obj_len[b].  view_len, obj_len (B) i64.  H % 4 == 0.  Lengths are
 * clamped to view_len in [0, L], obj_len in [0, min(Op, L - view_len)], so no value addresses outside the tensors.
 * bwd is the adjoint in store form: EVERY row of dpano (B,L,H) is written, dobj[b, l - view_len[b]] inside the object
 * segment and 0 elsewhere (no prior zero fill).  Both are pure copies. */
int bevbert_obj_rows_fwd(const void* pano, const int64_t* view_len, const int64_t* obj_len, void* obj, uint8_t* mask, int B,
                         int L, int Op, int H, int dtype, hipStream_t stream);
int bevbert_obj_rows_bwd(const void* dobj, const int64_t* view_len, const int64_t* obj_len, void* dpano, int B, int L,
                         int Op, int H, int dtype, hipStream_t stream);

/* Object supervision and record of one navigation step; launch BEFORE bevbert_nav_action (it reads the pre-action ended).
 * obj_logits (B,O) dtype 0/1 (-inf = masked), obj_ids (B,O) i32 (the caller's integer ids), obj_len (B) i64 (clamped to
 * [0, O]), gt_obj (B), cur (B) node, end_vps (B,E) + n_end (B): the goal-viewpoint set, ended (B) u8.
 * targets (B) i64 = -100 when ended or cur is not in end_vps[b, :n_end[b]], else the first j < obj_len[b] with
 * obj_ids[b, j] == gt_obj[b] (-100 when there is none).  og_slot (B) i32 = torch.argmax of obj_logits[b, :obj_len[b]] (the
 * first maximum; a NaN beats every number, the first NaN wins), -1 when obj_len[b] == 0.  For samples that are not ended
 * stop_og[b, cur[b]] (B,N) i32 = og_slot >= 0 ? obj_ids[b, og_slot] : -1 (a revisit overwrites; cur outside [0, N) is
 * not recorded). */
int bevbert_nav_obj_step(const void* obj_logits, int dtype, int B, int O, const int* obj_ids, const int64_t* obj_len,
                         const int* gt_obj, const int* cur, const int* end_vps, const int* n_end, int E, const uint8_t* ended,
                         int* stop_og, int N, int64_t* targets, int* og_slot, hipStream_t stream);

/* After bevbert_nav_action: for just_ended[b], pred_obj[b] = stop_node[b] in [0, N) ? stop_og[b, stop_node[b]] : -1; the
 * other rows of pred_obj (B) i32 keep what they hold. */
int bevbert_nav_obj_pick(const uint8_t* just_ended, const int* stop_node, const int* stop_og, int N, int* pred_obj, int B,
                         hipStream_t stream);

/* reverie/env.py _eval_item of B finished trajectories, f64; path / gt / action_steps as in bevbert_nav_metrics (no bound
 * on Lp), goal_vps (B,E) + n_goal (B) the goal-viewpoint set, pred_obj / gt_obj (B) i32.  items (B,8): action_steps,
 * trajectory_steps, trajectory_lengths, success (last path node in the goal set), oracle_success (any), spl, rgs
 * (pred_obj == gt_obj), rgspl.  avg (8) or NULL: eval_metrics' means in the same order, the last five x100, summed in
 * sample order.  Path lengths are summed by the routine bevbert_nav_metrics uses.  A scan outside [0, S): a row of NaN. */
int bevbert_nav_metrics_obj(const double* dist, int N, int S, const int* scan, const int* path, const int* path_len, int Lp,
                            const int* action_steps, const int* gt, const int* gt_len, int Lg, const int* goal_vps,
                            const int* n_goal, int E, const int* pred_obj, const int* gt_obj, int B, double* items,
                            double* avg, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Candidate waypoint prediction of the continuous-environment agent (since 0.2.0; entry points added, ABI otherwise
 * unchanged).  Replaces bevbert_ce/vlnce_baselines/waypoint_pred/transformer/waypoint_bert.py:66-86 (the ring-masked
 * self-attention of BinaryDistPredictor_TRM), models/Policy_ViewSelection_BEV.py:196-321 (mode 'waypoint' after the
 * predictor: softmax, waypoint_pred/utils.py nms, the waypoint_aug draw, candidate features, pooling and re-ordering)
 * and ss_trainer_BEV.py:347-384 (_vp_feature_variable).  Forward only, no atomics, fixed output shapes (K_MAX = 5
 * candidates, L = 17 panorama rows); no entry synchronises with the host, so the stage can sit in a captured step.
 * The reference's behaviour is kept as it executes, quirks included: they are listed in csrc/waypoint.hip. */

/* Self-attention over the ring of 12 views: qkv (B,12,3*nh*64) packed [q | k | v] (dtype 0/1), out (B,12,nh*64).  Query i
 * attends to keys i-1, i, i+1 (mod 12); the reference's additive -10000 on the other nine keys underflows to an exact 0
 * weight in fp32, so this is the same function.  No dropout, no backward (the predictor is frozen, always eval). */
int bevbert_wp_ring_attn(const void* qkv, void* out, int B, int nh, float scale, int dtype, hipStream_t stream);

/* logits (B,12,120) f32: the classifier output BEFORE the predictor's roll by HEATMAP_OFFSET = 5 (row 10*img + k of the
 * (120,12) view is angle 10*img + k - 5).  Per sample: softmax over the 1 440 cells of the rolled map -> heat (B,120,12);
 * one wrap row on either side; 5 rounds of arg-max (first index wins ties) + suppression, sigma = (7, 5); the surviving
 * picks of rows 1..120 in row-major order are the candidates: cand_count (B).  in_train != 0 (waypoint_aug): candidate k
 * is replaced by an inverse-CDF draw over the 120 cells of its image's region, region_probs (B,5,120) (0 for k >=
 * cand_count), with the uniform rand (B,5) = 24 bits of hash(key ^ (8 b + k)), key = salted(hash(site_key(seed, t) ^
 * BB_STREAM_WAYPOINT)) (csrc/common.h; a domain of its own since 0.2.3) -- all five are written, the first cand_count
 * are used.  Outputs, padding -1 / 0: cand_angle_idx, cand_dist_idx, cand_img_idx (counter-clockwise)
 * (B,5) i32; cand_angle_fts (B,5,4) = [sin, cos, 0, 1] of the clockwise angle; cand_angles (B,5) counter-clockwise
 * radians; cand_distances (B,5) = (dist_idx + 1) / 4.  region_probs and rand may be NULL when in_train == 0. */
int bevbert_wp_candidates(const float* logits, int B, int in_train, uint32_t seed, int t, int* cand_count,
                          int* cand_angle_idx, int* cand_dist_idx, int* cand_img_idx, float* cand_angle_fts,
                          float* cand_angles, float* cand_distances, float* region_probs, float* heat, float* rand,
                          hipStream_t stream);

/* rgb_embeds (B*12,512), depth_embeds (B*12,128,4,4) in the predictor's clockwise view order (dtype 0/1, outputs alike);
 * pano_angle_fts (12,4) f32 = the angle features of the counter-clockwise views.  pano_rgb (B,12,512), pano_depth
 * (B,12,128) (4 x 4 mean): counter-clockwise view i = input view (12 - i) % 12.  Panorama-encoder inputs padded to L = 17:
 * rgb_fts (B,17,512), dep_fts (B,17,128), loc_fts (B,17,4) f32, nav_types (B,17) i64, view_lens (B) i64; rows = the
 * candidates in order (view cand_img_idx, own angle feature, type 1), the views no candidate points into in ascending
 * index (type 0), zeros. */
int bevbert_wp_pano_inputs(const void* rgb_embeds, const void* depth_embeds, int dtype, int B, const int* cand_count,
                           const int* cand_img_idx, const float* cand_angle_fts, const float* pano_angle_fts,
                           void* pano_rgb, void* pano_depth, void* rgb_fts, void* dep_fts, float* loc_fts,
                           int64_t* nav_types, int64_t* view_lens, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Ghost-node map of the continuous-environment agent (since 0.2.2; entry points added, ABI otherwise unchanged).
 * Replaces bevbert_ce/vlnce_baselines/models/graph_utils.py:142-372 (GraphMap: identify_node, estimate_cand_pos,
 * update_graph with its two networkx all-pairs Dijkstra runs, front_to_ghost_dist, get_pos_fts, get_neighbors) and
 * ss_trainer_BEV.py:317-345 (_teacher_action_new from given distances), :465-475 (_discretize_polar_relpos), :477-532 (the
 * candidate half of _nav_bev_variable), :534-611 (_nav_gmap_variable), :1083-1084 (stop scores), :1110-1179 (actions).
 * B maps in dense arrays of fixed capacity: node k is the reference's str(k), ghost g its 'g' + str(g); ids in outputs
 * are -1 = [stop] / none, k < N = node k, N + g = ghost g.  N <= 64, 1 + N + Gh <= 512.  No atomics, fixed output shapes,
 * no entry synchronises with the host.  *overflow: 1 = a capacity (nodes, ghosts, positions per ghost, BEV candidates)
 * was exceeded and the item was refused, 2 = an action that names no live ghost.  The reference's behaviours that are
 * kept as they execute are listed in csrc/ce_map.hip.  Per-step host inputs: pose (B,4) f64 = x, y, z, heading;
 * live (B) u8 (0: the map is left alone, its output rows are padding); step_id (1) i32 -- device memory, so a captured
 * step replays with fresh values. */
typedef struct bevbert_ce_state {
  double* node_pos;   /* (B, N, 3) */
  double* edge_w;     /* (B, N, N)  edge weights, < 0 = no edge */
  double* dist;       /* (B, N, N)  shortest_dist[x][y], summed from x; +inf = none */
  int* hops;          /* (B, N, N)  len(shortest_path[x][y]) (both end points), 0 = none */
  int* pred;          /* (B, N, N)  predecessor of y on the path from x, -1 = none */
  int* n_nodes;       /* (B) */
  int* node_step;     /* (B, N) */
  float* stop_score;  /* (B, N) */
  void* node_embeds;  /* (B, N, H)  dtype */
  int* g_cnt;         /* (B)  ghosts ever created: the next ghost id */
  uint8_t* g_alive;   /* (B, Gh) */
  int* g_npos;        /* (B, Gh)  observed positions = fronts = embedding count */
  double* g_pos;      /* (B, Gh, P, 3) */
  double* g_mean;     /* (B, Gh, 3) */
  double* g_aug;      /* (B, Gh, 3)  mean + training noise */
  float* g_sum;       /* (B, Gh, H)  embedding sums */
  int* g_fronts;      /* (B, Gh, P) */
  int* prev_vp;       /* (B)  -1 = none */
  int* cur_vp;        /* (B)  node made by the last update */
  uint8_t* merge;     /* (B)  merge_ghost of each map */
  int* overflow;      /* (1) */
  int B, N, Gh, P, H, dtype;
} bevbert_ce_state;

/* identify_node + estimate_cand_pos + update_graph of every live map: a new node at pose, the prev_vp edge, every
 * candidate j < cand_count[b] (cand_angles / cand_distances (B,C) f32, C <= 16, as bevbert_wp_candidates writes them)
 * localized to a node or created as / merged into a ghost with the j-th row of pano (B,L,H) whose nav_types (B,L) i64 is 1;
 * avg_pano (B,H) becomes the node embedding (dtype of the state).  ghost_aug a > 0: every live ghost's augmented position
 * is redrawn as mean + clip(N(0, (a, 0, a)), +-a), a pure function of (seed, step salt, step_id, b, ghost id): key =
 * salted(hash(hash(seed ^ 0x9e3779b9) ^ BB_STREAM_GHOST)) (csrc/common.h; a domain of its own since 0.2.3), kb =
 * hash(hash(key ^ step_id) ^ b), kg = hash(kb ^ g), u1 = (24 bits of hash(kg ^ 1) + 1) / 2^24, u2 = 24 bits of
 * hash(kg ^ 2) / 2^24, Box-Muller in double.  Then
 * all-pairs Dijkstra.  cand_slot (B,C): the id a candidate went to, -1 = padding / refused (a candidate
 * without a nav_types == 1 row is refused with the overflow flag). */
int bevbert_ce_update(const bevbert_ce_state* st, const double* pose, const uint8_t* live, const int* step_id,
                      const int* cand_count, const float* cand_angles, const float* cand_distances, int C,
                      const void* avg_pano, const void* pano, const int64_t* nav_types, int L, double loc_noise,
                      double ghost_aug, uint32_t seed, int* cand_slot, hipStream_t stream);

/* _nav_gmap_variable padded to G = 1 + N + Gh rows: [stop], the nodes in creation order, the live ghosts in creation
 * order.  gmap_ids (B,G) i64, step_ids (B,G) i64, visited / masks (B,G) u8, img_fts (B,G,H) dtype (row 0 = 0, ghosts =
 * sum / count), pos_fts (B,G,7) f32, pair_dists (B,G,G) f32, no_vp_left (B) u8. */
int bevbert_ce_nav_vars(const bevbert_ce_state* st, const double* pose, const uint8_t* live, int64_t* gmap_ids,
                        int64_t* step_ids, uint8_t* visited, uint8_t* masks, void* img_fts, float* pos_fts,
                        float* pair_dists, uint8_t* no_vp_left, hipStream_t stream);

/* get_neighbors + _discretize_polar_relpos: slot 0 = the current node (centre cell), the 1-hop nodes, the live ghosts
 * with the current node among their fronts; at most K slots.  nav_masks (B,dim*dim) u8, cand_idxs / cand_ids (B,K) i64
 * (padding 0 / -1), cand_n (B), gpos_fts (B,7) f32 = the start node's position features, and the SAP logit fusion's
 * indices computed from the ids: src (B,G) i64 into [local (K) | backtrack | 0], vis_c (B,K) u8. */
int bevbert_ce_bev_cands(const bevbert_ce_state* st, const double* pose, const uint8_t* live, int bev_dim, double bev_res,
                         int K, uint8_t* nav_masks, int64_t* cand_idxs, int64_t* cand_ids, int* cand_n, float* gpos_fts,
                         int64_t* src, uint8_t* vis_c, hipStream_t stream);

/* node_stop_scores[cur_vp] = probs0[b * stride] for every live map. */
int bevbert_ce_stop_scores(const bevbert_ce_state* st, const uint8_t* live, const float* probs0, int stride,
                           hipStream_t stream);

/* _teacher_action_new ('spl') from cur_dist (B) f64 and ghost_dist (B,Gh) f64 by ghost id: 0 when cur_dist < 1.5, -100
 * when no ghost is left (and for maps that are not live), else the row of the first minimal live ghost.  out (B) i64. */
int bevbert_ce_teacher(const bevbert_ce_state* st, const uint8_t* live, const double* cur_dist, const double* ghost_dist,
                       int64_t* out, hipStream_t stream);

/* ss_trainer_BEV.py:1110-1179 for a_t (B) i64 rows of gmap_ids (B,G): rec (B, 11 + 4 N) f64 = [act 0 / 4 (-1: not live or
 * refused), cur, stop_vp / front_vp, ghost id (-1), len(back_path), back_path (N, -1 padded), stop / front position (3),
 * ghost position (3), positions of back_path's nodes (N,3)]; sets prev_vp = front and, with consume_ghost, deletes the ghost. */
int bevbert_ce_act(const bevbert_ce_state* st, const uint8_t* live, const int64_t* a_t, const int64_t* gmap_ids,
                   int last_step, int consume_ghost, double* rec, hipStream_t stream);

/* update_node_pc's store: for every live map, row b of src (B rows of row_bytes bytes, a multiple of 4) is copied into
 * slot b * N + cur_vp[b] of store (B * N rows).  Called once each for the step's grid features, depths and camera matrices. */
int bevbert_ce_remember(const bevbert_ce_state* st, const uint8_t* live, const void* src, void* store, int64_t row_bytes,
                        hipStream_t stream);

/* gather_node_pc(cur, order) as written: order 0 = the current node, else the nodes in creation order with
 * len(shortest_path[cur][node]) <= order (both end points counted: order 1 is still the current node alone).  rows (B,R)
 * store slots, row_live (B,R) u8; padding = the map's slot 0 with row_live 0; more than R nodes set *overflow. */
int bevbert_ce_bev_select(const bevbert_ce_state* st, const uint8_t* live, int order, int R, int* rows, uint8_t* row_live,
                          hipStream_t stream);

/* ---- Training through the ghost-node map (csrc/ce_train.hip, ce_train.py; since 0.2.4) -------------------------------
 * The reference keeps the panorama embeddings as live tensors inside GraphMap (ss_trainer_BEV.py:1060-1066), so the loss of
 * step t reaches the panorama encoder's pass of every step s <= t through _nav_gmap_variable.  The device map keeps them
 * in raw arrays; these entries record what its updates did (the "tape") and run the adjoint of its embedding path.  A tape
 * of T steps: cur (T,B) i32 the node a step made (-1: none), live (T,B) u8, slot / row (T,B,C) i32 the ghost id N + g a
 * candidate went to and the row of pano it brought (-1 / -1: localised to a node, refused, padding), ids (T,B,G) i64 the
 * gmap_ids of a step's listing, cnt (T,B,Gh) i32 the ghosts' g_npos at that listing, and the fp32 accumulators d_avg
 * (T,B,H), d_pano (T,B,L,H).  No atomics, no host synchronisation. */

/* After bevbert_ce_update of one step: fills that step's slices cur_out (B), live_out (B), slot_out / row_out (B,C) from the
 * state's cur_vp (B), the live mask, the update's cand_slot (B,C) and nav_types (B,L) i64 (candidate j brings the j-th row
 * whose type is 1).  last_cur (B) i32 is the tape's own memory of the node recorded last (-1 at the start of an episode):
 * a live map whose cur_vp did not move (update refused at node capacity) is recorded as not live. */
int bevbert_ce_tape_record(const int* cur_vp, const uint8_t* live, const int* cand_slot, const int64_t* nav_types, int B,
                           int N, int C, int L, int* last_cur, int* cur_out, uint8_t* live_out, int* slot_out, int* row_out,
                           hipStream_t stream);

/* Adjoint of gmap_img_fts of tape step t (0 <= t < T) for every step s <= t, one launch: with dG (B,G,H) `dtype` (BB_F32 /
 * BB_BF16) = d gmap_img_fts[t], for every map live at s and at t
 *   d_avg[s][b, :]            += dG[b, 1 + e, :]                 e = cur[s][b], the node step s made;
 *   d_pano[s][b, row, :]      += dG[b, r, :] / cnt[t][b, g]      for each candidate of step s with slot N + g whose ghost is
 *                                                                 listed at row r of ids[t][b] (a consumed ghost is not).
 * One wave per (s, b, avg | candidate): each reads at most one row of dG and adds into its own accumulator row, so the
 * result does not depend on scheduling; a row receives the consumer steps in the order of the calls (backward: t
 * descending).  H is any positive integer (16-byte loads when H % 4 == 0). */
int bevbert_ce_embeds_bwd(const void* dG, int dtype, int t, int T, int B, int N, int Gh, int C, int L, int H, const int* cur,
                          const uint8_t* live, const int* slot, const int* row, const int64_t* ids, const int* cnt,
                          float* d_avg, float* d_pano, hipStream_t stream);

/* The action draw of a training rollout (ss_trainer_BEV.py:1097-1100): a_t (B) i64 = the inverse-CDF sample of
 * softmax(logits (B,C) f32 / bf16, -inf on masked slots) with the rule of bevbert_nav_action's `sample` mode (fp32 softmax,
 * cumulative sum in row order, the first j with u0 < c and p > 0, else the last positive j), replaced by teacher[b] (i64,
 * -100 passes through) where u1 <= sample_ratio.  u0 / u1 (B) f32 = 24 bits of hash(k ^ 4 b) / hash(k ^ (4 b + 1)) / 2^24,
 * k = salted(hash(site_key(seed, t) ^ BB_STREAM_CE_ACTION)) (csrc/common.h). */
int bevbert_ce_sample_action(const void* logits, int dtype, int B, int C, const int64_t* teacher, float sample_ratio,
                             uint32_t seed, int t, int64_t* a_t, float* u0, float* u1, hipStream_t stream);

/* ---- Validation metrics (csrc/val_metrics.hip, validate.py; pretrain_src/train_r2r.py:351-510) ------------------------
 * Accumulated on the device, no atomics: every entry leaves per-row (per-workgroup) records in `scratch` and ONE workgroup
 * folds them in index order, so two runs give the same bits.  `acc` is three 8-byte words {double sum; int64 a; int64 b}
 * that the fold ADDS into (zero them per task).  scratch: 8 bytes per row for val_ce_rows / val_bce_keys, 24 KiB for
 * val_auc; 8-byte aligned; the entries of one accumulator share a stream.
 *
 * val_ce_rows: logits (R, C) f32 / bf16 with row stride ld (elements), target (R) i64, valid (R) f32 or NULL.  One pass
 * per row: running maximum and sum of exponentials in fp32 (-inf entries add nothing), arg-max with the lowest index on a
 * tie, loss = lse - logit[target].  sum += loss, a += (arg-max == target), b += 1.  A row with valid == 0 adds nothing; a
 * row with target < 0 (ignore_index; also target >= C) adds no loss and no hit but counts in b -- what
 * F.cross_entropy(reduction='sum') and len(labels) give.  C <= 1024: one wave per row, else one workgroup per row; 16-byte
 * loads where a row starts on a 16-byte boundary.  NaN logits are not ranked as torch.argmax ranks them. */
int bevbert_val_ce_rows(const void* logits, int64_t ld, const int64_t* target, const float* valid, int R, int C, int dtype,
                        void* acc, void* scratch, hipStream_t stream);

/* val_kl_rows (MRC, train_reverie_obj.py:415-446): logits as in val_ce_rows; targets (N, C) f32 contiguous, row r reads
 * targets[idx[r]] (idx (R) i64 or NULL: row r); valid (R) f32 or NULL.  sum += the row's KL as bevbert_soft_ce_fwd defines
 * it (fp32 statistics m and s; the terms formed and summed per row in fp64, the row's sum rounded to fp32 once for its
 * record, the records added in fp64), a += (arg-max of the logits == arg-max of the target row, the lowest index on
 * a tie on both sides), b += 1.  A row with valid == 0 adds nothing.  Same record layout, fold and scratch (8 bytes per
 * row) as val_ce_rows. */
int bevbert_val_kl_rows(const void* logits, int64_t ld, const float* targets, const int64_t* idx, const float* valid, int R,
                        int C, int dtype, void* acc, void* scratch, hipStream_t stream);

/* val_bce_keys: logits (R, C) f32 / bf16 (row stride ld), labels uint8 rows read through idx (i64, NULL: row r) as in
 * bce_rows_fwd, valid (R) f32 or NULL.  sum += BCE-with-logits over the valid rows' elements, a += valid rows.  Element
 * (r, c) leaves keys[cursor + r C + c] = (monotone_u32(logit) << 1) | (label != 0), monotone_u32 = the sign-flip map of the
 * fp32 bits with -0.0 taken as +0.0 (bf16 is widened exactly); elements of invalid rows leave INT64_MAX.  A position
 * >= capacity is not written and sets *overflow (i64) to 1.  The caller advances its cursor by R C. */
int bevbert_val_bce_keys(const void* logits, int64_t ld, const uint8_t* labels, const int64_t* idx, const float* valid, int R,
                         int C, int dtype, void* acc, void* scratch, int64_t* keys, int64_t cursor, int64_t capacity,
                         int64_t* overflow, hipStream_t stream);

/* val_auc: keys ascending (n < 2^31), INT64_MAX entries skipped.  out[0] = 2U, out[1] = P, out[2] = N (stored, not
 * added): U the Mann-Whitney statistic of the positives with ties (equal key >> 1) at their mid-rank, exact in integers;
 * AUC = out[0] / (2 P N). */
int bevbert_val_auc(const int64_t* sorted_keys, int64_t n, int64_t* out, void* scratch, hipStream_t stream);

/* ---- CLIP vision transformer (csrc/vit.hip, clip_vit.py): forward-only row kernels ------------------------------------
 * Rows are (rows, H) row-major, H in {256, 512, 768, 1024}; the residual stream z32 is fp32 whatever `dtype` (the
 * compute dtype of the GEMM operands: BB_F32 or BB_BF16; since 0.5.0 also BB_F16 for the four bevbert_vit_* entries, whose
 * fp16 results are the fp32 value rounded to nearest even, overflow to inf). */

/* ConvertImageDtype + Normalize + conv1's im2col: images (n_src, R, R, 3) u8 -> out (N * g * g, 3 * P * P) dtype with
 * g = R / P, P in {16, 32}, column order (c, ky, kx); output image i reads input image view_map[i] (NULL: i; an index
 * outside [0, n_src) gives rows of zeros).  value = (float(u8) / 255 - mean_c) / std_c, each operation rounded to nearest;
 * mean_std: six HOST floats, mean[3] then std[3]. */
int bevbert_vit_patchify(const uint8_t* images, const int* view_map, void* out, int N, int n_src, int R, int P,
                         const float* mean_std, int dtype, hipStream_t stream);

/* Token assembly + ln_pre + ln_1 of block 0: row n * L + t is class_embedding + pos[0] for t = 0 and
 * conv_out[n * (L - 1) + t - 1] + pos[t] otherwise (conv_out (N * (L - 1), H) dtype; class_embedding (H), pos (L, H) f32);
 * z32 (N * L, H) f32 = LayerNorm(row; gamma_pre, beta_pre), y (N * L, H) dtype = LayerNorm(z32; gamma1, beta1). */
int bevbert_vit_embed_prenorm(const void* conv_out, const float* class_embedding, const float* pos, const float* gamma_pre,
                              const float* beta_pre, const float* gamma1, const float* beta1, float* z32, void* y, int N,
                              int L, int H, float eps, int dtype, hipStream_t stream);

/* z = z32 + (x + bias) with x (rows, H) dtype.  final_form = 0: z32 <- z in place, y (rows, H) dtype = LayerNorm(z).
 * final_form = 1 (rows = N * L): rows t > 0 of every image go to x_patch (N, L - 1, H) f32 unnormalised, the class rows
 * t = 0 through LayerNorm to y (N, H) dtype; z32 is left as it was. */
int bevbert_vit_bias_residual_prenorm(float* z32, const void* x, const float* bias, const float* gamma, const float* beta,
                                      void* y, float* x_patch, int rows, int L, int H, float eps, int final_form, int dtype,
                                      hipStream_t stream);

/* QuickGELU: t = x + bias, y = t * sigmoid(1.702 t); (rows, C) dtype, C % 4 == 0, bias (C) f32; finite for every finite t;
 * y may be x. */
int bevbert_vit_bias_quickgelu(const void* x, const float* bias, void* y, int rows, int C, int dtype, hipStream_t stream);

/* AdaptiveAvgPool2d((G, G)) of depth (n_src, Hd, Wd) f32 -> out (N, G, G) f32, windows as torch defines them; view_map as
 * in bevbert_vit_patchify. */
int bevbert_depth_grid_pool(const float* depth, const int* view_map, float* out, int N, int n_src, int Hd, int Wd, int G,
                            hipStream_t stream);

/* ---- depth ResNet encoder (csrc/depth_resnet.hip, depth_resnet.py): forward-only kernels around the library GEMMs ------
 * Activations are NHWC; `dtype` is the compute dtype of the GEMM operands (BB_F32 or BB_BF16).  A GroupNorm shape (C, G)
 * is supported when C is a power of two in [4, 1024], G a power of two up to 16 and C / G is 2 or a multiple of 4.  No
 * atomics: two calls on the same input give the same bits. */

/* avg_pool2d(2) + Conv2d(1, 32, 7, stride 2, pad 3, no bias), fp32: depth (n_src, H, W) -> out (N, H / 4, W / 4, 32), raw
 * (not normalised); H and W multiples of 4; weight_t (49, 32): the convolution weight (32, 1, 7, 7) transposed to
 * (ky * 7 + kx, c); view_map as in bevbert_vit_patchify. */
int bevbert_dr_stem(const float* depth, const int* view_map, const float* weight_t, float* out, int N, int n_src, int H, int W,
                    hipStream_t stream);

/* GroupNorm statistics of x (N, HW, C) dtype (BB_F32 is always accepted): mean, rstd (N, G) f32, rstd = 1 / sqrt(var + eps)
 * with the biased variance, computed from squared distances to the mean (never E[x^2] - mean^2).  An image is cut into
 * ceil(HW / (8192 / C)) chunks; with more than one chunk `partial` must hold N * chunks * G * 2 floats. */
int bevbert_dr_gn_stats(const void* x, float* partial, int64_t partial_floats, float* mean, float* rstd, int N, int HW, int C,
                        int G, float eps, int dtype, hipStream_t stream);

/* y = relu(gn(x) [+ second term]) over (N, HW, C) dtype with gn(x) = (x - mean[n, g]) * rstd[n, g] * gamma[c] + beta[c]:
 * mode 0 nothing added; mode 1 + r (N, HW, C) dtype; mode 2 + gn2(r) with mean2, rstd2, gamma2, beta2 (the downsample
 * branch); mode 3 as mode 0 but y is written (N, C, HW).  Unused pointers may be NULL.  y may be x or r except in mode 3. */
int bevbert_dr_gn_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        const void* r, const float* mean2, const float* rstd2, const float* gamma2, const float* beta2, void* y,
                        int N, int HW, int C, int G, int mode, int dtype, hipStream_t stream);

/* The stem's form: x (N, H, W, C) f32 raw -> y (N, ceil(H / 2), ceil(W / 2), C) dtype = relu(MaxPool2d(3, 2, 1)(gn(x))); the
 * maximum is taken over the normalised values. */
int bevbert_dr_gn_relu_maxpool(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                               void* y, int N, int H, int W, int C, int G, int dtype, hipStream_t stream);

/* Rows of a ksize x ksize convolution (ksize 1 or 3, padding (ksize - 1) / 2, stride 1 or 2) on x (N, H, W, C) dtype:
 * out (N * Ho * Wo, ksize * ksize * C) with Ho = (H - 1) / stride + 1, column order (ky, kx, c), zeros outside the image.
 * C * sizeof(dtype) must be a multiple of 16. */
int bevbert_dr_gather_rows(const void* x, void* out, int N, int H, int W, int C, int ksize, int stride, int dtype,
                           hipStream_t stream);

/* ---- R2R pre-training inputs from device-resident tables (csrc/path_data.hip, path_data.py, feature_store.py) ----------
 * The panorama tensors of a batch, gathered from a resident view-feature store and the per-viewpoint PanoTable instead of
 * being collated on the host (pretrain_src/data/dataset.py:580-622 get_traj_pano_fts, tasks.py:126-137 the collates'
 * pad_tensors, loader.py:78-120 the copy).  store (N, n_views, view_stride) f16: only the first D channels of a view are
 * read (the reference slices [:, :image_feat_size] off rows that may carry class probabilities).  PanoTable: view_order
 * (N, Vmax) u8 the store view of token v, n_tokens (N), loc_tab (N, Vmax, L) f32, nav_tab (N, Vmax) u8.  rows (Tp): the
 * batch's panoramas as store / table rows, -1 = a dummy panorama.  Written: img (Tp, Vp, D) f32 (the widening is exact), loc
 * (Tp, Vp, L) f32, nav (Tp, Vp) i64, lens (Tp) i64; everything beyond a panorama's token count is zero; a dummy panorama is
 * all zeros with length 1.  16-byte loads where D, view_stride and the pointers allow, single elements otherwise.  No
 * atomics.  The CALLER checks 0 <= rows < N or -1 and n_tokens <= Vp (device data is not read back here); a row >= N is
 * written as a dummy and tokens beyond Vp are dropped rather than written out of bounds. */
int bevbert_pd_pano_rows(const void* store, int64_t view_stride, int n_views, const uint8_t* view_order, const int* n_tokens,
                         const float* loc_tab, const uint8_t* nav_tab, const int* rows, float* img, float* loc, int64_t* nav,
                         int64_t* lens, int N, int Vmax, int L, int Tp, int Vp, int D, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVBERT_HIP_H */
