/* ase_hip.h — C ABI of libase_hip.so: the MI355X (gfx950) kernels behind the ASE/AMP PPO update.
 *
 * The reference (nv-tlabs/ASE) is pure Python on stock PyTorch ops; it has no FFI.  Each entry
 * point below therefore cites the reference *Python* statement(s) it replaces (paths relative to
 * /root/reference/ase/).  INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add for each.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ASE_E* code otherwise
 *     (ase_hip_last_error() gives the text); nothing allocates, frees or synchronises;
 *     work is enqueued on `stream` (a hipStream_t), so calls are hipGraph-capturable.
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS.
 *   - `dtype` selects the storage type of activations / shadow weights that feed the matrix
 *     cores: ASE_F32 (exact f32 MFMA, parity mode), ASE_BF16 (bf16 MFMA, f32 accumulate) or — for the two GEMM
 *     entry points only — ASE_F32X3 (f32 storage like ASE_F32, each product as three bf16 MFMAs on a hi/lo split) and, for
 *     ase_hip_gemm_nt, ASE_F32H3 (three f16 MFMAs on a hi/lo split of power-of-two scaled operands: ~22 significant bits).
 *     Running statistics are f64, master weights / gradients / Adam state / loss math are f32.
 *   - GEMM operands live in "padded" buffers: K (the contracted, contiguous dimension) is a
 *     multiple of 128 bytes / sizeof(type) and the padding is zero.
 *   - row index maps: a logical minibatch row r reads dataset row p = idx ? idx[r] : r; when
 *     remap_h > 0 the dataset is the time-major experience buffer [H=remap_h, N=remap_n, ...] and
 *     p is the env-major flat index (p = env*H + t, rl_games swap_and_flatten01), i.e. the
 *     physical row is (p % H) * N + p / H.  This is how learning/ase_agent.py:108-113 and
 *     learning/amp_datasets.py:14-27 are applied without materialising copies.
 */
#ifndef ASE_HIP_H
#define ASE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (ase_hip_gemm_nt_ex, ase_hip_gemm_nt_stacked, ase_hip_disc_head_v2, ase_hip_rms_normalize_multi_v2, ase_hip_apply_multi_v2, ase_hip_task_reset, ase_hip_proj_launch, ase_hip_motion_sync, ase_hip_latent_renew, ase_hip_amp_reset_due, ase_hip_amp_demo_fetch, ase_hip_gemm_tn_kernel_id, ase_hip_rollout_store, ase_hip_rollout_head / ase_hip_word_step, ase_hip_hrl_latent / ase_hip_hrl_llc_action / ase_hip_hrl_accum and ase_hip_env_pre_step / ase_hip_env_post_step were added WITHOUT a new version
 *  number: a library built before them passes this check and fails at symbol lookup instead - ase_amd/lib.py resolves every symbol at
 *  load time) */
#define ASE_HIP_ABI_VERSION 9

enum { ASE_F32 = 0, ASE_BF16 = 1, ASE_F32X3 = 2 /* f32 storage, products as 3 bf16 MFMAs on a hi/lo split (GEMMs only) */,
       ASE_F32H3 = 4 /* 4-byte storage, products as 3 f16 MFMAs on hi/lo splits of operands scaled by 2^ea / 2^eb (the exponents ride in
                        bits 8-15 / 16-23 of dtype: ASE_F32H3 | (ea << 8) | (eb << 16)).  ase_hip_gemm_nt: A is plain f32 (split in the
                        kernel), B is the PACKED SPLIT format ase_hip_refresh_shadow(dtype = ASE_F32H3 | eb << 16) writes - per group of
                        8 consecutive k: 8 hi halves, then 8 lo halves, of W * 2^eb (32 bytes, leading dimension as for f32).  Operands
                        must satisfy |x| * 2^e < 65504 (overflow turns the output into NaN); best accuracy for |x| * 2^e >= 2^-2 */,
       ASE_F16 = 3 /* IEEE half storage + v_mfma_f32_32x32x16_f16, f32 accumulate: what the reference's mixed_precision flag
                      (torch.cuda.amp autocast + GradScaler, learning/ase_agent.py:216,271-288) computes in; conversions saturate */ };
/* activations: the names of rl_games' activations_factory (learning/ase_network_builder.py:162); swish = SiLU */
enum { ASE_ACT_NONE = 0, ASE_ACT_RELU = 1, ASE_ACT_TANH = 2, ASE_ACT_SILU = 3, ASE_ACT_ELU = 4, ASE_ACT_GELU = 5,
       ASE_ACT_SIGMOID = 6, ASE_ACT_SELU = 7, ASE_ACT_SOFTPLUS = 8 };
enum { ASE_AUX_NONE = 0, ASE_AUX_RELU_MASK = 1, ASE_AUX_TANH_GRAD = 2, ASE_AUX_RELU_BITS = 3 /* aux = bit matrix written by mask_out */,
       ASE_AUX_PREACT = 4 /* aux = the layer's PRE-activation z (dtype, written by the forward launch as its twin): multiply by
                             act'(z); the activation id rides in bits 8+ of aux_mode: ASE_AUX_PREACT | (ASE_ACT_x << 8) */ };
enum { ASE_OK = 0, ASE_EINVAL = -1, ASE_ELAUNCH = -2, ASE_EUNSUPPORTED = -3 };

int ase_hip_abi_version(void);
const char* ase_hip_last_error(void);

/* Which kernel ase_hip_gemm_nt launches for a shape (host only): 0 = 64 x 64 tile (narrow outputs), 1 = 128 x 128,
 * 2 = phased 256 x 256 (16-bit storage), 3 = lock-step 256 x 256 (4-byte storage), 4 = 64 x 128, 5 = 64 x 64 with
 * 128-byte rows, 6 = phased 192 x 256 (16-bit storage, single rounds of 192-255 tiles; falls back to 2 when the
 * launch needs the LDS-slab epilogue).  bench.py uses it to attribute launch times to the dominant kernel. */
int ase_hip_gemm_nt_kernel_id(int M, int N, int K, int dtype);

/* Kernel-tuning aid (scripts/lab): when buf is a device uint64[4 * workgroups] array, the phased NT kernel stamps
 * {entry, first tile landed, main loop done, stores retired} per workgroup (100 MHz clock); NULL switches it off. */
int ase_hip_debug_nt_profile(void* buf);
/* ... shader_clock != 0: the two main-loop stamps (1, 2) of the phased kernel count SHADER clocks (s_memtime) instead of the
 * 100 MHz clock - two profiled launches of one shape give the clock frequency the chip actually sustains under that kernel
 * (bench.py `roofline.sustained_clock_mhz`: MI355X does not hold its 2.4 GHz boost under dense MFMA load). */
int ase_hip_debug_nt_profile_clock(int shader_clock);

/* ---------------------------------------------------------------------------------------------
 * Dense layers (matrix cores).
 * ------------------------------------------------------------------------------------------- */

/* C[m,n] = mask( act( alpha * sum_k A[m,k] * B[n,k] + bias[n] ) )       "NT" GEMM
 *   A [M,K] dtype, B [N,K] dtype (weights, K contiguous), C [M,N] dtype or f32 (out_f32).
 *   aux [M,N] dtype: ASE_AUX_RELU_MASK multiplies by (aux > 0), ASE_AUX_TANH_GRAD by (1 - aux^2);
 *   rows m >= aux_split (> 0) read aux row m - aux_delta (a stacked block of rows re-using another block's mask:
 *   the gradient-penalty chain rides on the discriminator's data-gradient launches).
 *   colsum (nullable, f32[colsum_n]) += column sums of the stored values for n < colsum_n (atomic):
 *   the bias gradient of the producing layer.
 *   mask_out (nullable) = the layer's TWIN output, what the data-gradient launch of the same activation will read as aux:
 *   act NONE / RELU / TANH: uint32 [M, ldmask], N % 32 == 0: bit n % 32 of word [m, n / 32] = (stored C[m,n] > 0) - read back
 *     with ASE_AUX_RELU_BITS (ldaux in words): 1/16 of the bytes of re-reading the 16-bit activation in the store-bound epilogue;
 *   act >= ASE_ACT_SILU: dtype [M, ldmask] (ldmask in ELEMENTS), the pre-activation z = alpha * A.B^T + bias - read back with
 *     ASE_AUX_PREACT (the derivative of a non-monotonic activation is not a function of its output; tanh keeps
 *     ASE_AUX_TANH_GRAD on the output itself).
 *   alpha_dev (nullable; ABI 6, a RECORD since ABI 7): DEVICE f32[2] scale record {factor, overflow count}.  The launch multiplies
 *   alpha by `factor` when it RUNS - how the factors of the dynamic loss scale (ase_hip_scaler_step's table: S, 1 / S, 1 / S^2, 1) reach
 *   launches recorded once and replayed across scale changes - and ADDS to `count` (by an unspecified positive amount) when an element
 *   it STORED into C / mask_out's pre-activation twin is not finite or sits at the storage type's saturation value (ASE_F16 conversions
 *   saturate at +-65504 where autocast would produce inf): GradScaler's found_inf, detected by the producer instead of a pass that
 *   re-reads every buffer of the step (ase_hip_scaler_check).  The same convention for every `*_dev` argument below; the loss heads
 *   report their stored head gradients, ase_hip_gemm_tn(_grouped) and ase_hip_sqnorm only read the factor.
 *   NON-FINITE values pass through as torch's nn.Linear + activation pass them: a NaN in A, B or bias makes every element of its
 *   row / column NaN (with a mask operand: where the mask keeps the element - ASE_AUX_RELU_MASK / ASE_AUX_RELU_BITS SELECT, so a
 *   masked-out element is 0 even where the product is NaN or inf, unlike torch's grad * mask) and NO activation turns it into a number - ASE_ACT_RELU is torch.relu, max(z, 0) that KEEPS a NaN (so an
 *   ASE_F32H3 operand beyond half's range stays loud behind ReLU too), tanh(+-inf) = +-1, sigmoid(+-inf) = 1 / 0, relu(-inf) = 0, +inf
 *   stays +inf.  ASE_F32, ASE_F32X3, ASE_F32H3, ASE_BF16 and out_f32 store the NaN / inf as such; ASE_F16 saturates: +-inf -> +-65504,
 *   and a NaN is stored as NaN by the launches that convert two outputs at a time (16-bit output, no colsum, act <= RELU, no value
 *   mask operand, N a whole number of wave tiles) and as -65504 by every other launch (the shared conversion, see
 *   ase_hip_gather_rows) - either way a scale record counts it.  mask_out's bit is (stored > 0): 0 for a NaN; a colsum entry is NaN
 *   where a stored value of its column is.  Elements the non-finite inputs do not reach are bitwise what they are without them.
 * Replaces: nn.Linear + activation forward  (learning/ase_network_builder.py:255-259,305-324,
 *   learning/amp_network_builder.py:81-84), and autograd's data-gradient of the same layers
 *   (B = the transposed weight shadow; mask = derivative of the previous activation), and the
 *   transposed-MLP chain of the gradient penalty (learning/amp_agent.py:453-459). */
int ase_hip_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                    const float* bias, const void* aux, int64_t ldaux, int aux_split, int aux_delta,
                    float* colsum, int colsum_n, void* mask_out, int64_t ldmask, int M, int N, int K, int act,
                    int aux_mode, int out_f32, float alpha, float* alpha_dev, int dtype, void* stream);

/* ase_hip_gemm_nt with three more duties in its epilogue, each nullable and each what a launch of its own did around the
 * six launches of the gradient penalty's value path.  dtype ASE_F32H3 only; act NONE / RELU, aux_mode NONE / RELU_BITS, no colsum.
 *   seed_w (f32[seed_n], seed_n <= N), seed_scale: C[m,n] = seed_scale * seed_w[n] * (act(z) > 0 ? 1 : 0) instead of act(z) - the
 *     product ase_hip_gp_seed forms for ReLU, bit for bit; columns n >= seed_n store 0.  mask_out still describes act(z).
 *   twin ([M, ldtwin] of twin_dtype = ASE_F16 / ASE_BF16, ldtwin in elements): the value stored to C once more in 16 bits, by the
 *     conversion ase_hip_gather_multi applies (RNE; f16 saturating).  With a twin, C may be NULL: no f32 store at all.
 *   sq_acc (f64*), sq_scale, sq_dyn (nullable scale record, only its factor is read): *sq_acc += sq_scale * factor * sum of the
 *     squares of the values stored (f32 over 4 consecutive columns, f64 beyond, one atomic per workgroup) - ase_hip_sqnorm.
 * An overflow report (alpha_dev) covers the f32 values; the twin's saturation is left to ase_hip_scaler_check_multi on its buffer. */
int ase_hip_gemm_nt_ex(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                       const float* bias, const void* aux, int64_t ldaux, int aux_split, int aux_delta,
                       float* colsum, int colsum_n, void* mask_out, int64_t ldmask, int M, int N, int K, int act,
                       int aux_mode, int out_f32, float alpha, float* alpha_dev, int dtype,
                       const float* seed_w, int seed_n, float seed_scale, void* twin, int64_t ldtwin, int twin_dtype,
                       double* sq_acc, double sq_scale, const float* sq_dyn, void* stream);

/* ase_hip_gemm_nt over TWO row blocks of one A [M,K] / C [M,N] pair (16-bit or 4-byte storage type, never out_f32) that share B, with
 * an epilogue each - the forward of a discriminator layer over the loss rows and the backward of the gradient-penalty chain through
 * the same weights (dJ/dU_l = m_l * (dJ/dU_{l-1} @ W_l^T) is forward-shaped), stacked as the engine's buffers already are:
 *   rows [0, split):  bias (nullable), act NONE / RELU, mask_out (nullable, only behind ReLU; written for these rows alone),
 *                     alpha, alpha_dev.  No mask operand.
 *   rows [split, M):  no bias, no activation, no mask_out; alpha2, alpha_dev2 (nullable record, as alpha_dev); the optional mask operand
 *                     aux in the ASE_AUX_RELU_BITS format, [M - split, ldaux] words, read at row m - split: pass aux_split = aux_delta =
 *                     split.  The mask SELECTS, as in ase_hip_gemm_nt: a masked-out element is 0 even where the product is inf or NaN.
 * The result is what ase_hip_gemm_nt on rows [0, split) followed by ase_hip_gemm_nt on rows [split, M) stores: bit for bit whenever both
 * forms sum in the same order, always on operands whose products and sums are exact.  One launch of the phased 256 x 256 kernel when
 * that is the kernel of the whole shape (ase_hip_gemm_nt_kernel_id(M, N, K, dtype) == 2, ASE_F16 / ASE_BF16, M < 65536) and split is a
 * multiple of 256 - every workgroup then lies in one block and picks that block's duties at its entry; in every other case the
 * library issues the two plain launches itself, on `stream`.
 * Refused (ASE_EINVAL): split <= 0 or >= M; a mask operand that is not the second block's (aux_mode other than NONE / RELU_BITS, or
 * aux_split / aux_delta != split); mask_out without ReLU; an activation beyond ReLU; colsum or out_f32. */
int ase_hip_gemm_nt_stacked(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                            const float* bias, const void* aux, int64_t ldaux, int aux_split, int aux_delta,
                            float* colsum, int colsum_n, void* mask_out, int64_t ldmask, int M, int N, int K, int act,
                            int aux_mode, int out_f32, float alpha, float* alpha_dev, int split, float alpha2, float* alpha_dev2,
                            int dtype, void* stream);

/* G[n, kmap(k)] += alpha * sum_m A[m,n] * B[m,k]   for n < n_real, kmap(k) valid     "TN" GEMM
 *   A [M,N] dtype (output gradients), B [M,K] dtype (layer inputs), G f32 [n_real, k_real]
 *   (master-layout weight gradient, accumulated with f32 atomics; split over M internally).
 *   kmap undoes the padded-concat layout of the first actor/critic layer: k < split_src -> k;
 *   k >= split_dst -> k - (split_dst - split_src); columns in between are padding.
 *   (layers without a concat pass split_src = split_dst = k_real).
 *   gbias (nullable, f32[n_real]) += alpha * sum_{m < bias_rows} A[m,n] (bias_rows <= 0: all rows): the bias gradient of the same layer, reduced from
 *   the A tiles the kernel stages anyway (a handful of atomics per column instead of one per row tile).
 *   Every column of G needs its column of B: k_real + (split_dst - split_src) <= K, anything else is refused (ASE_EINVAL; the
 *   grouped plan refuses it too).  Columns [n_real, N) of A, [split_src, split_dst) and [k_real + gap, K) of B are padding whose
 *   CONTENT never reaches G or gbias.
 * Replaces: autograd's weight gradient of nn.Linear inside loss.backward()
 *   (learning/ase_agent.py:271). */
int ase_hip_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, float* G, float* gbias,
                    int bias_rows, int M, int N, int K, int n_real, int k_real, int split_src, int split_dst,
                    float alpha, const float* alpha_dev, int dtype, void* stream);

/* Which kernel ase_hip_gemm_tn launches for a problem (host only): 0 = 128 x 128 (register-staged, every storage mode),
 * 1 = phased 256 x 256 (16-bit storage, M and bias_rows whole 64-row K-tiles, M * (256 x 256 tiles) >= 256 * 2048, operands
 * below 2 GiB).  The arguments are exactly what the choice depends on; ase_hip_gemm_tn asks the same function. */
int ase_hip_gemm_tn_kernel_id(int M, int N, int K, int n_real, int bias_rows, int64_t lda, int64_t ldb, int dtype);

/* All weight gradients of one branch of an optimisation step in ONE grouped launch (16-bit storage).  They only depend on
 * buffers the data-gradient chain has already written, and one grid of ~256 long contractions pays the split-M reduction once
 * per step instead of once per layer.
 *   problems: int64[n][16] = {A, lda, B, ldb, G, gbias (or 0), bias_rows (0 = all), M, N, K, n_real, k_real, split_src,
 *             split_dst, alpha (f32 bit pattern), 0}, fields as in ase_hip_gemm_tn, leading dimensions in elements;
 *             M and bias_rows multiples of 64.
 *   ase_hip_gemm_tn_grouped_plan (host only, no GPU needed): validates the HOST copy of the table, fills field 15 (tiles
 *             along k; bit 30: the gradient buffer is shared with another problem of the launch) and writes the work list
 *             int32[n_work][4] = {problem, 256 x 256 output tile, first row, 64-row K-tiles | workspace slab << 16} in LAUNCH
 *             order - positions [x n_work/8, (x+1) n_work/8) run on XCD x: the tiles of one (problem, row range) share their
 *             operand panels through that XCD's L2, so such groups are bin-packed whole into the 8 ranges and the ranges
 *             padded with empty items (K-tiles = 0; n_work is a multiple of 8) - and (red non-null) the reduce list
 *             int32[n_red][4] = {problem, tile, first slab, splits} (split s of a tile: slab first + s * tiles of the problem);
 *             target_wg <= 0: one workgroup per CU.
 *   ase_hip_gemm_tn_grouped: launch with DEVICE copies of the planned tables.  workspace (device f32, 16-byte aligned,
 *             n_work * ASE_TN_SLAB floats, private to the launch until it completes): every work item stores its partial
 *             tile there with plain 16-byte stores and a second kernel adds the sums into G / gbias (deterministic, no
 *             atomics: memory-side f32 atomics run at ~1.4 TB/s on this chip, 64 MB of them per launch).  workspace NULL:
 *             the work items add into G with f32 atomics directly.
 * Replaces: loss.backward()'s weight / bias gradients of every nn.Linear (learning/ase_agent.py:271). */
#define ASE_TN_SLAB (65536 + 256)
int ase_hip_gemm_tn_grouped_plan(int64_t* problems, int n_problems, int target_wg, int32_t* work, int max_work,
                                 int* n_work, int32_t* red, int max_red, int* n_red);
int ase_hip_gemm_tn_grouped(const int64_t* problems, const int32_t* work, int n_work, const int32_t* red, int n_red,
                            float* workspace, const float* alpha_dev, int dtype, void* stream);

/* Shadow copies of one weight matrix for the matrix cores: W_s [n_pad,k_pad] and its transpose
 * Wt_s [k_pad,n_pad] (both dtype, zero padded, concat columns moved to split_dst).  Run after
 * every optimizer step.  (No reference counterpart: the reference multiplies f32 masters.)
 * dtype = ASE_F32H3 | (eb << 16): the packed half-split shadows of W * 2^eb (see ASE_F32H3; buffers sized and strided as f32). */
int ase_hip_refresh_shadow(const float* W, int n_real, int k_real, void* Ws, int64_t ldws,
                           void* Wts, int64_t ldwts, int split_src, int split_dst, int dtype,
                           void* stream);

/* The same for every layer in ONE launch.  desc: DEVICE int64[n_layers][12] =
 * {W, n_real, k_real, Ws, ldws, Wts, ldwts, split_src, split_dst - split_src, bias, bias_shadow, ceil(k_real/32)}
 * (pointers as integers; bias_shadow f32[n_pad] feeds ase_hip_gemm_nt's bias). */
int ase_hip_refresh_shadow_multi(const int64_t* desc, int n_layers, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Running mean/std normaliser (rl_games RunningMeanStd; learning/common_agent.py:49,323-325,
 * learning/amp_agent.py:26,535-538, learning/ase_agent.py:170-181) fused with the minibatch
 * gather (learning/amp_datasets.py:14-27).
 * state: f64[2*D+1] = running_mean[D], running_var[D], count.
 * ------------------------------------------------------------------------------------------- */

/* sums[2*D] (f64, atomic) += { sum_r (x[r,j]-shift[j]), sum_r (x[r,j]-shift[j])^2 }, shift = f32(running_mean) */
int ase_hip_rms_moments(const float* src, int64_t ld_src, int D, const int32_t* idx, int remap_h,
                        int remap_n, int M, const double* state, double* sums, void* stream);

/* The same for up to 4 streams of equal width D and row count M in ONE launch (agent / replay / demo AMP observations,
 * learning/amp_agent.py:280-289): HOST arrays of per-stream sources, index maps and partial-sum buffers. */
int ase_hip_rms_moments_multi(const float* const* srcs, const int64_t* ld_srcs, const int32_t* const* idxs,
                              const int* remap_h, const int* remap_n, double* const* sums, int n_streams, int D, int M,
                              const double* state, void* stream);
int ase_hip_rms_normalize_multi(const float* const* srcs, const int64_t* ld_srcs, const int32_t* const* idxs,
                                const int* remap_h, const int* remap_n, const float* const* means,
                                const float* const* stds, void* const* outs, const int64_t* ld_outs, int n_streams, int D,
                                int M, int dtype, void* stream);
/* ... with a nullable f32 twin per stream (outs32 / ld_outs32, HOST arrays like the others; a NULL entry or a NULL array: none):
 * the normalised, clamped value BEFORE its rounding to dtype, [M, ld] f32 in 16-byte rows - the demo rows' exact input of the
 * gradient penalty's value path out of the launch that normalises them anyway (it was an ase_hip_rms_normalize of its own). */
int ase_hip_rms_normalize_multi_v2(const float* const* srcs, const int64_t* ld_srcs, const int32_t* const* idxs,
                                   const int* remap_h, const int* remap_n, const float* const* means,
                                   const float* const* stds, void* const* outs, const int64_t* ld_outs,
                                   float* const* outs32, const int64_t* ld_outs32, int n_streams, int D, int M, int dtype,
                                   void* stream);

/* Sequentially merge n_streams batches (sums[s][2*D], counts[s] rows each; counts are the GLOBAL
 * row counts) into `state` exactly as RunningMeanStd.forward does in training mode, and after
 * each merge emit mean_f32[s][D] and std_f32[s][D] = sqrt(f32(var)+1e-5).  n_streams == 0 emits
 * one pair from the current state (eval mode). */
int ase_hip_rms_finalize(double* state, int D, const double* sums, const int32_t* counts /* HOST */,
                         int n_streams, float* mean_out, float* std_out, void* stream);

/* out_i[r, col_off_i + j] = clamp((x[map(r), j] - mean[j]) / std[j], -5, 5), i < 3 destinations.  The clamp is torch.clamp's:
 * +-inf -> +-5, a NaN is KEPT (a diverged observation must not reach the policy as a plausible -5).  A normalised value is in
 * [-5, 5] or NaN, so 16-bit outputs (here and in ase_hip_rms_normalize_multi / _v2) are stored with a plain RNE cast: the NaN
 * survives in all three storage types. */
int ase_hip_rms_normalize(const float* src, int64_t ld_src, int D, const int32_t* idx, int remap_h,
                          int remap_n, int M, const float* mean, const float* std,
                          void* out0, int64_t ld0, void* out1, int64_t ld1, void* out2, int64_t ld2,
                          int dtype, void* stream);

/* y = sqrt(f32(var)+1e-5) * clamp(x,-5,5) + f32(mean): RunningMeanStd(..., unnorm=True)
 * (learning/ase_agent.py:140-141,391-392), D == 1.  torch.clamp: a NaN x gives a NaN y. */
int ase_hip_rms_unnormalize(const double* state, const float* x, float* y, int64_t n, void* stream);

/* Generic row gather + cast: dst[r, 0:D] = src[map(r), 0:D]; dst dtype = dst_dtype
 * (learning/amp_datasets.py:21-22 for the small per-row tensors).  The cast is RNE; ASE_F16 saturating: beyond +-65504 and
 * +-inf -> +-65504, and a NaN -> -65504 (the saturating conversion is a median of three with the two bounds, which returns the
 * minimum of its operands when one is a NaN; every producer that stores ASE_F16 through it shares this, the GEMM epilogues
 * included).  ASE_BF16 and ASE_F32 keep inf and NaN. */
int ase_hip_gather_rows(const float* src, int64_t ld_src, int D, const int32_t* idx, int remap_h,
                        int remap_n, int M, void* dst, int64_t ld_dst, int dst_dtype, void* stream);

/* Several fields by ONE launch.  desc: DEVICE int64[n_fields][6] = {src, ld_src, D, dst, ld_dst, dst_dtype}.  idx may be NULL
 * (identity row map): the launch is then a multi-tensor f32 -> storage-type conversion (the exact gradient-penalty chain handed
 * to the 16-bit launches, UpdateEngine._gp_f32). */
int ase_hip_gather_multi(const int64_t* desc, int n_fields, const int32_t* idx, int remap_h, int remap_n,
                         int M, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss heads: forward value + analytic gradient w.r.t. the head inputs, in one pass.
 * `acc` is a device array of f64 partial sums (layout ASE_ACC_* below), zeroed by begin_step.
 * ------------------------------------------------------------------------------------------- */
enum {
    ASE_ACC_MASK_SUM = 0,   /* sum rand_action_mask                         */
    ASE_ACC_A_LOSS,         /* sum mask * ppo surrogate                      */
    ASE_ACC_B_LOSS,         /* sum mask * bound loss                         */
    ASE_ACC_ENTROPY,        /* sum mask * entropy                            */
    ASE_ACC_CLIPPED,        /* sum mask * 1[|ratio-1| > e_clip]              */
    ASE_ACC_C_LOSS,         /* sum (return - value)^2                        */
    ASE_ACC_KL,             /* sum_rows policy_kl                            */
    ASE_ACC_DIV,            /* sum mask * diversity loss                     */
    ASE_ACC_BCE_AGENT,      /* sum softplus(l) over agent+replay rows        */
    ASE_ACC_BCE_DEMO,       /* sum softplus(-l) over demo rows               */
    ASE_ACC_AGENT_ACC,      /* count l < 0 (agent+replay)                    */
    ASE_ACC_DEMO_ACC,       /* count l > 0 (demo)                            */
    ASE_ACC_GP,             /* sum_rows |d logit / d x_demo|^2               */
    ASE_ACC_ENC,            /* sum_rows -<enc, z>                            */
    ASE_ACC_ENC_GP,         /* sum_rows |d enc_err / d x_agent|^2 (enc_grad_penalty); slots up to here are per-row sums
                               (the data-parallel ranks add them), the ones below depend on the weights only */
    ASE_ACC_LOGIT_W2,       /* sum w_logit^2                                 */
    ASE_ACC_DISC_W2,        /* sum over all disc weights^2                   */
    ASE_ACC_ENC_W2,         /* sum over all enc weights^2                    */
    ASE_ACC_GRAD_SQ,        /* sum of all gradients^2 (truncate_grads: global-norm clip) */
    ASE_ACC_COUNT = 24
};

/* acc[slot] += sum_i x[i] (f32 in, f64 atomic out); square != 0 sums x^2. */
int ase_hip_reduce_sum(const float* x, int64_t n, int square, double* acc, int slot, void* stream);

/* PPO actor/critic head for one minibatch (learning/common_agent.py:505-534,456-464,
 * learning/ase_agent.py:228-241,252-258,290-294,445-467; rl_games neglogp / policy_kl).
 *   mu      f32 [rows_mu, ld_mu]   rows [0,M) main pass, rows [M,2M) diversity pass (if div_on)
 *   value   f32 [M, ld_v] (column 0)
 *   mb_*    packed f32 minibatch fields (see ase_hip_gather_rows)
 *   d_mu    dtype [rows_mu, ld_dmu], d_value dtype [M, ld_dv]: d loss / d mu, d loss / d value
 *   db_mu f32[act_dim], db_value f32[1] (nullable): += their column sums (head bias gradients)
 *   masked: 1 -> sum(mask*x)/sum(mask) reductions (AMP/ASE), 0 -> plain means over m_global (PPO)
 *   mu_tanh: 1 -> mu_out = tanh(mu) precedes the losses (HRL high-level policy,
 *            learning/hrl_network_builder.py:26-29)
 *   acc[ASE_ACC_MASK_SUM] must already hold the GLOBAL mask sum.
 *   The diversity loss is weighted like the other masked means: mask / acc[ASE_ACC_MASK_SUM] with masked, 1 / m_global without.
 *   A NaN in mu or value stays NaN wherever the reference's torch.clamp / torch.max keep it: in the surrogate, the bound loss,
 *   the diversity loss and the clipped critic loss, in their accumulators and in the gradients of both row blocks.
 *   grad_scale (all loss heads): the STORED head gradients d_* are multiplied by it (the bias gradients and the loss
 *            scalars are not) - the static loss scale of ASE_F16 storage, whose back-propagated gradients would
 *            otherwise fall into half's subnormal range; the weight-gradient launches undo it through their alpha.
 *            The counterpart of the reference's GradScaler (learning/ase_agent.py:216,271-288).  1 for bf16 / f32.
 *            grad_scale_dev (nullable, ABI 6 / 7): a DEVICE scale record {factor on top - the DYNAMIC loss scale (ase_hip_scaler_step
 *            keeps it), read when the launch runs; overflow count, see ase_hip_gemm_nt's alpha_dev}.
 *   scratch: device f64[ASE_PPO_SCRATCH] workspace, private to one launch at a time: per-workgroup partial sums (loss
 *            scalars, head-bias column sums), folded into acc / db_* by a second one-workgroup kernel of the same call (no
 *            contended atomics; a kernel boundary instead of per-workgroup fences).
 *   ls_mode (ABI 8): the policy's log-std (network space.continuous, rl_games A2CBuilder):
 *            ASE_LS_FROZEN  logstd f32[act_dim], frozen (learn_sigma False): no log-std gradient; ld_ls, d_ls, db_ls unused.
 *            ASE_LS_VECTOR  logstd f32[act_dim], learned (learn_sigma, fixed_sigma True).
 *            ASE_LS_ROWS    logstd f32[rows, ld_ls], one row per state (learn_sigma, fixed_sigma False: the sigma head's output,
 *                           e.g. columns 64.. of the stacked [mu | sigma] head output, ld_ls = ld_mu).
 *            A learned mode adds d loss / d logstd = w (-g ratio (1 - d^2) - entropy_coef) per row and action (g = d a_loss /
 *            d ratio, d = (a - mu) / sigma, w the masked-mean weight; the KL takes sigma detached): d_ls (nullable) dtype
 *            [rows_mu, ld_dls] receives it times grad_scale (diversity rows [M, 2M): zero), db_ls f32[act_dim] (nullable) +=
 *            its column sums (the vector's gradient, or the sigma head's bias gradient).  scratch then holds
 *            ASE_PPO_SCRATCH_LS doubles.  entropy_coef: the loss's -entropy_coef * entropy term (learned modes only). */
#define ASE_PPO_SCRATCH (1024 * 72 + 8)
#define ASE_PPO_SCRATCH_LS (1024 * 136 + 8)
#define ASE_LS_FROZEN 0
#define ASE_LS_VECTOR 1
#define ASE_LS_ROWS 2
int ase_hip_ppo_head(const float* mu, int64_t ld_mu, const float* value, int64_t ld_v,
                     const float* mb_actions, const float* mb_old_mu, const float* mb_old_sigma,
                     const float* mb_old_logp, const float* mb_adv, const float* mb_old_value,
                     const float* mb_return, const float* mb_mask, const float* mb_z,
                     const float* new_z, const float* logstd,
                     void* d_mu, int64_t ld_dmu, void* d_value, int64_t ld_dv,
                     float* db_mu, float* db_value, float* mu_out, double* acc, double* scratch,
                     int M, int m_global, int act_dim, int z_dim, int masked, int div_on, int mu_tanh,
                     int clip_value, float e_clip, float critic_coef, float bounds_coef,
                     float div_coef, float div_tar, float grad_scale, float* grad_scale_dev,
                     int ls_mode, int64_t ld_ls, void* d_ls, int64_t ld_dls, float* db_ls, float entropy_coef,
                     int dtype, void* stream);

/* Discriminator logit losses (learning/amp_agent.py:442-447,481-496): rows [0,2*amb) agent+replay
 * (target 0), rows [2*amb,3*amb) demo (target 1).  d_logit dtype [3*amb, ld_d] column 0. */
int ase_hip_disc_head(const float* logit, int64_t ld_l, void* d_logit, int64_t ld_d, float* db_logit,
                      double* acc, int amb, int amb_global, float disc_coef, float grad_scale, float* grad_scale_dev, int dtype,
                      void* stream);
/* ... with an addend for the gradient penalty's accumulator: gp_add (nullable, DEVICE f64*): acc[ASE_ACC_GP] += *gp_add, once per
 * launch.  The stacked schedule of the penalty (ase_hip_gemm_nt_stacked) forms sum (S s g_0)^2 in a cell of its own BEFORE the step's
 * accumulators are zeroed; this launch, which runs behind that, folds it in.  gp_add = NULL: ase_hip_disc_head. */
int ase_hip_disc_head_v2(const float* logit, int64_t ld_l, void* d_logit, int64_t ld_d, float* db_logit,
                         double* acc, int amb, int amb_global, float disc_coef, float grad_scale, float* grad_scale_dev,
                         const double* gp_add, int dtype, void* stream);

/* Encoder head (learning/ase_network_builder.py:217, learning/ase_agent.py:413-418,469-472):
 * e f32 [amb, ld_e] pre-normalisation output, z f32 [amb, z_dim]; d_e dtype [amb, ld_de].
 * enc_out (nullable) f32 [amb, z_dim] receives normalize(e) (torch.nn.functional.normalize, eps 1e-12: a row with a NaN is
 * NaN in every column). */
int ase_hip_enc_head(const float* e, int64_t ld_e, const float* z, int64_t ld_z, void* d_e,
                     int64_t ld_de, float* db_enc, float* enc_out, double* acc, int amb, int amb_global,
                     int z_dim, float enc_coef, float grad_scale, float* grad_scale_dev, int dtype, void* stream);

/* Encoder gradient penalty (learning/ase_agent.py:431-441: mean_rows |d enc_err / d amp_obs|^2 with enc_err = -<normalize(e), z>),
 * the two per-row pieces around the GEMM chain.  e f32 [rows, ld_e] pre-normalisation encoder output, z f32 [rows, ld_z].
 *   seed: u[r, :] = scale * d enc_err / d e = -scale (z - eh <eh, z>) / |e|          (dtype [rows, ld_u]; eh = e / |e|)
 *   back: d_e[r, :] += grad_scale * J du[r, :],  J = d u / d e (unscaled), du f32 [rows, ld_du] = what the chain's backward
 *         returns at u (d_e carries the gradient scale of ase_hip_enc_head); J = 0 for a row with |e| < 1e-12, where
 *         normalize(e) = e / 1e-12 and u does not depend on e;
 *         db_enc (nullable, f32 [z_dim]) += column sums of the change of the stored d_e. */
int ase_hip_enc_gp_seed(const float* e, int64_t ld_e, const float* z, int64_t ld_z, void* u, int64_t ld_u, int rows,
                        int z_dim, float scale, int dtype, void* stream);
int ase_hip_enc_gp_back(const float* e, int64_t ld_e, const float* z, int64_t ld_z, const float* du, int64_t ld_du,
                        void* d_e, int64_t ld_de, float* db_enc, int rows, int z_dim, float grad_scale, float* grad_scale_dev,
                        int dtype, void* stream);

/* Gradient-penalty seed (learning/amp_agent.py:453-459): g[r,j] = scale * w[j] * act'  (d logit / d pre-activation of the last
 * hidden layer).  h = that layer's TWIN: its output for ReLU (act' = [h > 0]) and tanh (1 - h^2), its pre-activation z for
 * the smooth activations (act >= ASE_ACT_SILU). */
int ase_hip_gp_seed(const void* h, int64_t ld_h, const float* w, void* g, int64_t ld_g, int rows,
                    int width, float scale, int act, int dtype, void* stream);

/* Second-order term of the penalty's double backward for activations with curvature: with g = act'(z) u the chain value at a
 * layer and dg = act'(z) r the (masked) gradient of the penalty w.r.t. u,  dz[r,j] += act''(z) u r = act'' / act'^2 * g * dg
 * - the path through act'(z) that autograd's create_graph=True adds for anything but ReLU.  twin as in ase_hip_gp_seed. */
int ase_hip_gp_second(const void* twin, int64_t ld_t, const void* g, int64_t ld_g, const void* dg, int64_t ld_dg,
                      void* dz, int64_t ld_dz, int rows, int width, int act, int dtype, void* stream);

/* out[j] += scale * sum_r x[r, j] over an f32 matrix [rows, cols] (row pitch ld): the gradient of the logit weights from the
 * gradient penalty = column sums of the last launch of the chain's backward (learning/amp_agent.py:453-459) - a 3 us
 * stream instead of column sums inside that launch's store-bound epilogue. */
int ase_hip_colsum(const float* x, int64_t ld, int rows, int cols, float scale, float* out, void* stream);

/* acc[slot] += scale * sum_{r,j} x[r,j]^2 over a dtype matrix [rows, cols]; scale_dev (nullable): a DEVICE f32 factor on top. */
int ase_hip_sqnorm(const void* x, int64_t ld, int rows, int cols, double* acc, int slot, double scale, const float* scale_dev,
                   int dtype, void* stream);

/* train_result scalars from the accumulators (same keys as learning/ase_agent.py:296-306).
 * out f32[ASE_RES_COUNT].  opt_state_lr (nullable: constant lr): the optimizer state of ase_hip_begin_step - the learning rate
 * opt_state[1] is then adapted from this step's kl as rl_games' AdaptiveScheduler does under the 'legacy' schedule after every
 * minibatch (learning/common_agent.py:204-208; lr_schedule: adaptive, kl_threshold): kl > 2 thr: lr / 1.5 (>= 1e-6),
 * kl < thr / 2: lr * 1.5 (<= 1e-2) - on the device, no .item() per step.  out[ASE_RES_LR] = the learning rate THIS step was
 * taken with (the reference's train_result['last_lr'], learning/common_agent.py:430), 0 with a constant rate (the host
 * knows it).  The masked means (a_loss, b_loss, entropy, clip fraction, diversity loss) divide by acc[ASE_ACC_MASK_SUM] when
 * masked != 0 and by m_global when masked == 0 - ASE_RES_DIV_LOSS uses the denominator that ase_hip_ppo_head used for the
 * diversity gradient.  ABI 3: ASE_RES_COUNT 16 -> 20 (ASE_RES_LR; result vectors are slots of a per-update ring, 80-byte pitch). */
enum {
    ASE_RES_A_LOSS = 0, ASE_RES_C_LOSS, ASE_RES_B_LOSS, ASE_RES_ENTROPY, ASE_RES_CLIP_FRAC, ASE_RES_KL,
    ASE_RES_DISC_LOSS, ASE_RES_DISC_GP, ASE_RES_DISC_LOGIT_LOSS, ASE_RES_DISC_AGENT_ACC,
    ASE_RES_DISC_DEMO_ACC, ASE_RES_ENC_LOSS, ASE_RES_DIV_LOSS, ASE_RES_LOSS, ASE_RES_MASK_SUM, ASE_RES_ENC_GP,
    ASE_RES_LR,
    ASE_RES_COUNT = 20
};
int ase_hip_finalize_scalars(const double* acc, float* out, int m_global, int amb_global, int masked,
                             int has_disc, int has_enc, int has_div, float critic_coef,
                             float entropy_coef, float bounds_coef, float disc_coef, float disc_logit_reg,
                             float disc_grad_penalty, float disc_weight_decay, float enc_coef,
                             float enc_weight_decay, float div_coef, float enc_grad_penalty, double* opt_state_lr,
                             float kl_threshold, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer (torch.optim.Adam(lr, eps=1e-8, weight_decay=0): learning/common_agent.py:45,
 * learning/ase_agent.py:265-269,287).
 * opt_state: DEVICE f64[8] = {step, lr, beta1, beta2, eps, bias_corr1, bias_corr2, _}; step is
 * advanced and the bias corrections recomputed on device by ase_hip_begin_step (graph-replay safe),
 * which also zeroes the n_acc accumulators.
 * ------------------------------------------------------------------------------------------- */
/* Global-norm gradient clipping, torch.nn.utils.clip_grad_norm_(parameters, grad_norm) (learning/ase_agent.py:273-288,
 * truncate_grads): g *= min(1, max_norm / (sqrt(*sqnorm) + 1e-6)); *sqnorm = sum of g^2 over all parameters (device f64,
 * e.g. accumulated by ase_hip_reduce_sum with square = 1).  The min is torch.clamp(coef, max=1.0): a NaN norm is KEPT, the
 * coefficient and with it every gradient become NaN (an infinite norm: coefficient 0). */
int ase_hip_clip_scale(float* g, int64_t n, const double* sqnorm, float max_norm, void* stream);

/* One small launch at the head of every optimisation step: + zeroes a second f64 buffer (the per-step partial statistics the
 * ranks exchange) and advances the Philox stream of the in-step latent draw (ase_hip_sample_latents with advance = 0). */
int ase_hip_begin_step(double* opt_state, double* acc, int n_acc, double* zero2, int n_zero2, uint64_t* rng_bump,
                       void* stream);
int ase_hip_adam(float* w, const float* g, float* m, float* v, int64_t n, const double* opt_state,
                 void* stream);
/* g[i] += c * w[i]  (the weight-only loss terms: learning/amp_agent.py:449-466) */
int ase_hip_axpy(float* g, const float* w, int64_t n, float c, void* stream);

/* Loss scaler of the half-storage engine = torch.cuda.amp.GradScaler around the optimizer step of the reference's mixed_precision
 * path (learning/ase_agent.py:271-288, learning/amp_agent.py:354-371: scaler.scale(loss).backward(); scaler.unscale_; scaler.step;
 * scaler.update - after EVERY optimisation step).  ABI 5; ABI 6: the scale lives on the device.
 *   scaler: DEVICE f64[8] = {found, skipped steps (total), growth tracker = clean steps since the scale last moved, steps (total),
 *           scale, growth_factor, backoff_factor, growth_interval}  (GradScaler's state and constructor arguments; the host writes
 *           slots 4-7 once)
 *   scale_tab: DEVICE f32[8] = four scale records {S, n0}, {1 / S, n1}, {1 / S^2, n2}, {1, n3}: what the `*_dev` arguments of the loss
 *           heads (S), the weight-gradient launches (1 / S), the penalty's norm (1 / S^2) and launches that carry no factor (1) point at
 *           - launches recorded once keep working when the scale moves - and where those launches report an overflow they stored (the
 *           counts n_k, ABI 7).
 * ase_hip_scaler_check = the found_inf test over ONE buffer the scaled backward wrote (dtype ASE_F32 / ASE_BF16 / ASE_F16):
 * scaler[found] += number of workgroups that met an element that is not finite or - ASE_F16, whose conversions saturate instead
 * of producing inf - sits at +-65504.  For buffers whose producers were given no record, and for the f32 gradient.
 * ase_hip_scaler_check_multi (ABI 7): the same over a DEVICE table int64[n_bufs][3] = {pointer, elements, dtype} in one launch,
 * wg_per_buf workgroups per buffer.
 * ase_hip_scaler_fold (ABI 7): scaler[found] += n0 + n1 + n2 + n3, counts = 0 - for a data-parallel step, whose ranks SUM-exchange
 * scaler[found] between this launch and ase_hip_scaler_step (which otherwise reads the counts itself). */
int ase_hip_scaler_check(const void* buf, int64_t n, int dtype, double* scaler, void* stream);
int ase_hip_scaler_check_multi(const int64_t* table, int n_bufs, int wg_per_buf, double* scaler, void* stream);
int ase_hip_scaler_fold(double* scaler, float* scale_tab, void* stream);
/* ase_hip_scaler_step = GradScaler.step + GradScaler.update, between the checks and the optimizer launch (ase_hip_adam reads opt_eff):
 *   found = scaler[found] != 0 or a non-zero count in scale_tab;
 *   found != 0: grads[0..n) = 0, opt_eff = the identity step {lr 0, beta1 = beta2 = 1, bias corrections 1} (w, m, v stay what they
 *               are), opt_state.step -= 1 (a skipped step is no optimizer step), skipped += 1;
 *               scale *= backoff_factor, growth tracker = 0
 *   found == 0: opt_eff = opt_state; growth tracker += 1, and when it reaches growth_interval: scale *= growth_factor, tracker = 0
 * then steps += 1, found = 0 and (scale_tab non-null) scale_tab = {scale, 0, 1 / scale, 0, 1 / scale^2, 0, 1, 0} - exactly
 * torch/amp/grad_scaler.py's _amp_update_scale_, once per optimisation step.  scale_tab NULL (ABI 5 behaviour): the scale is a
 * launch argument the host moves between updates; slots 4-7 are not touched. */
int ase_hip_scaler_step(double* scaler, double* opt_state, double* opt_eff, float* grads, int64_t n, float* scale_tab,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * Once-per-epoch rollout tail.
 * ------------------------------------------------------------------------------------------- */

/* r = -log(max(1 - sigmoid(l), 1e-4)) * scale   (learning/amp_agent.py:570-577) */
int ase_hip_disc_reward(const float* logit, int64_t ld_l, float* r, int64_t n, float scale, void* stream);
/* r = max(<normalize(e), z>, 0) * scale          (learning/ase_agent.py:404-411) */
int ase_hip_enc_reward(const float* e, int64_t ld_e, const float* z, int64_t ld_z, float* r, int64_t n,
                       int z_dim, float scale, void* stream);
/* GAE (learning/common_agent.py:437-449, learning/ase_agent.py:484-490,105-106):
 * rewards = w_task*task + w_disc*disc + w_enc*enc (disc/enc nullable); all [H,N] time-major. */
int ase_hip_gae(const uint8_t* dones, const float* values, const float* next_values,
                const float* r_task, const float* r_disc, const float* r_enc, float w_task, float w_disc,
                float w_enc, double gamma, double tau, float* advs, float* returns, int H, int N, void* stream);
/* advantages = returns - values, masked normalisation (learning/amp_agent.py:551-561 with rl_games
 * normalization_with_masks; mask nullable -> learning/common_agent.py:536-546).
 * Two calls: phase 0 accumulates moments into acc3 (f64[3], zeroed by the caller), phase 1 writes. */
int ase_hip_adv_norm(const float* returns, const float* values, const float* mask, float* adv,
                     double* acc3, int64_t n, int normalize, int phase, void* stream);

/* dst[(head + i) % size, :] = src[map(i), :]  (learning/replay_buffer.py:27-49) */
int ase_hip_ring_store(const float* src, int64_t ld_src, int D, const int32_t* idx, int remap_h,
                       int remap_n, int n, float* dst, int64_t size, int64_t head, void* stream);

/* y[r,:] = x[r,:] / max(|x[r,:]|_2, 1e-12): the latent a high-level action selects
 * (torch.nn.functional.normalize, learning/hrl_agent.py:235; learning/ase_network_builder.py:140-142). */
int ase_hip_normalize_rows(const float* x, int64_t ld_x, float* y, int64_t ld_y, int n, int dim, void* stream);

/* Rollout-time action head: the eval branch of the model wrapper + the eps-greedy mix
 * (learning/amp_models.py:29-36; learning/amp_agent.py:139-169; learning/ase_agent.py:117-148): per row
 * mu' = mu (tanh'ed when mu_tanh, learning/hrl_network_builder.py:26-29), sigma = exp(logstd), a = mu' + sigma N(0,1)
 * (Philox, rng_state as below), neglogp(a), rand_mask = Bernoulli(rand_probs[row]) and actions = rand_mask ? a : mu'.
 * rand_probs / rand_mask nullable (plain PPO: every row stochastic).  mu has leading dimension ld_mu, outputs are dense.
 * logstd: row r reads logstd[r * ld_logstd ..] (ABI 8): ld_logstd 0 - one vector for every row, >= act_dim - a per-state
 * log-std (the sigma head's output rows). */
int ase_hip_sample_actions(const float* mu, int64_t ld_mu, const float* logstd, int64_t ld_logstd, const float* rand_probs,
                           uint64_t* rng_state, float* mu_out, float* sigma_out, float* actions, float* neglogp,
                           float* rand_mask, int n, int act_dim, int mu_tanh, void* stream);

/* z[r,:] = normalize(N(0,I))  (learning/ase_network_builder.py:221-225); counter-based Philox,
 * stream position read from and advanced in rng_state (u64[2] = {seed, offset}).  Row r draws the elements
 * (row_offset + r) * dim .. of the stream: data-parallel ranks pass the global index of their first row, so the R-rank
 * draw equals the 1-rank draw.  advance = 0: the stream position is left alone (ase_hip_begin_step moved it). */
int ase_hip_sample_latents(float* z, int rows, int dim, uint64_t* rng_state, int64_t row_offset, int advance,
                           void* z2 /* nullable: a second copy [rows, ld_z2] in z2_dtype (the GEMM input buffer) */,
                           int64_t ld_z2, int z2_dtype, void* stream);

/* One environment step stored into experience slot n (an addition to ABI 9, nothing else changed): everything
 * play_steps does behind env_step, over n_envs rows, without dones.nonzero() and without a host round trip.  n = slot, or -
 * slot_dev non-NULL (DEVICE int32 [1]) - the word read when the launch runs, IN PLACE of slot (ase_hip_amp_demo_fetch's
 * head_dev idea: a recorded launch follows a slot kept on the device); a word outside [0, n_slots) makes the whole call write
 * nothing: no experience, no accumulators, no meter, no ids.  Every part but dones is optional, each group given whole or
 * left out whole (NULL):
 *   row copies   fields: DEVICE int64[n_fields][6] = {src, ld_src, D, dst_base, ld_dst, slot_stride}, all f32, pitches in
 *                elements (ase_hip_gather_multi's table with a slot stride in place of the dtype), n_fields 0 .. 16, D >= 1,
 *                ld >= D: dst_base[n * slot_stride + e * ld_dst + j] = src[e * ld_src + j] for j < D, bitwise.  Columns
 *                [D, ld_dst) and other slots are not touched.  A field moves 16 bytes per lane when D % 4 == 0, ld_src % 4
 *                == 0, ld_dst % 4 == 0, slot_stride % 4 == 0 and src and dst_base are 16-byte aligned, 4 bytes otherwise -
 *                chosen per field inside the kernel.  The table's content cannot be checked on the host.
 *   rewards      rewards_out[n * rewards_ss + e] = (rewards[e] + shift) * scale, two f32 operations each rounded on its own
 *                (rl_games DefaultRewardsShaper).  rewards f32 [n_envs] is also what the accumulators add: it is required by
 *                either, and refused when neither rewards_out nor the accumulators are given.
 *   dones_out    dones_out[n * dones_ss + e] = (uint8)(dones[e] != 0).  dones [n_envs] has the type dones_kind names:
 *                ASE_KIND_U8, ASE_KIND_I32, ASE_KIND_I64 (Isaac Gym's reset_buf) or ASE_KIND_F32 (HRLAgent.env_step); its
 *                values are expected to be 0 or 1, as in the reference.  d = (float)dones[e] below.
 *   next values  next_values_out[n * next_values_ss + e] = next_values[e] * (1.0f - (float)terminate[e]); terminate
 *                [n_envs] of terminate_kind (the same four codes).
 *   accumulators cur_rewards, cur_lengths f32 [n_envs], in place: r = cur_rewards[e] + rewards[e] (the RAW reward),
 *                l = cur_lengths[e] + 1.0f; a row with dones[e] != 0 enters this call's meter sums with (r, l); then
 *                cur_rewards[e] = r * (1.0f - d), cur_lengths[e] = l * (1.0f - d).
 *                meter: DEVICE f64[4] = {reward_mean, length_mean, current_size, episodes_seen}, max_size = games_to_track.
 *                With k done rows in this call: k == 0 leaves the four words bitwise unchanged; otherwise, in f64, for each
 *                of the two means new = sum / k, size = min(k, max_size), old = min(max_size - size, current_size),
 *                mean = (mean * old + new * size) / (old + size); then current_size = old + size, episodes_seen += k - rl_games
 *                AverageMeter.update word for word.
 *                workspace: DEVICE f64[workspace_doubles], workspace_doubles >= ASE_ROLLOUT_STORE_WS(n_envs), private to
 *                the call until it completes; its content on entry does not matter.  NO floating-point atomics and no
 *                ticket: every block of ASE_ROLLOUT_STORE_ROWS rows stores its partial {sum r, sum l, k} (rows in order) to
 *                its own three words, and a SECOND one-wave kernel of the same call (ase_hip_adv_norm's and
 *                ase_hip_ppo_head's precedent: a kernel boundary instead of a fence) folds them - lane i the blocks i,
 *                i + 64, ... in order, then a butterfly over the lanes - and updates the meter.  Only the order of the f64
 *                sum differs from a sequential sum; two calls on equal inputs give bitwise-equal meters.
 *   id list      done_ids_out int32 [n_envs]: done_ids_out[e] = e for a done row, -1 otherwise, every element written - the
 *                list ase_hip_task_reset, ase_hip_latent_renew and a plan of ase_hip_amp_reset accept (ids outside
 *                [0, n_envs) are skipped), so the next step's resets need no nonzero.
 * The three outputs with a slot stride need rewards_ss / dones_ss / next_values_ss >= n_envs.
 * Refused, on the host, before any launch: NULL dones; a partial group (accumulators; next values; rewards_out without
 * rewards; rewards without a consumer; accumulators without rewards); n_envs <= 0; n_fields outside [0, 16] or fields NULL with
 * n_fields > 0; a kind code outside the four; a slot stride below n_envs; max_size <= 0 with a meter; a workspace below
 * ASE_ROLLOUT_STORE_WS(n_envs); n_slots <= 0 or slot outside [0, n_slots) (checked also when slot_dev is given).
 * Replaces: learning/common_agent.py:267-293 (the stores behind env_step, rewards_shaper, terminated / next_vals,
 *   current_rewards / current_lengths, dones.nonzero, game_rewards.update / game_lengths.update, not_dones), with
 *   learning/amp_agent.py:93-122, learning/ase_agent.py:66-100 and learning/hrl_agent.py:124-151 for the extra fields. */
enum { ASE_KIND_U8 = 0, ASE_KIND_I32 = 1, ASE_KIND_I64 = 2, ASE_KIND_F32 = 3 };
#define ASE_ROLLOUT_STORE_MAX_FIELDS 16
#define ASE_ROLLOUT_STORE_ROWS 8
#define ASE_ROLLOUT_STORE_WS(n_envs) (3 * (((n_envs) + ASE_ROLLOUT_STORE_ROWS - 1) / ASE_ROLLOUT_STORE_ROWS))
int ase_hip_rollout_store(const int64_t* fields, int n_fields, const float* rewards, float shift, float scale,
                          float* rewards_out, int64_t rewards_ss, const void* dones, int dones_kind, uint8_t* dones_out,
                          int64_t dones_ss, const float* next_values, const void* terminate, int terminate_kind,
                          float* next_values_out, int64_t next_values_ss, float* cur_rewards, float* cur_lengths,
                          double* meter, int max_size, double* workspace, int64_t workspace_doubles, int32_t* done_ids_out,
                          int n_envs, int slot, const int32_t* slot_dev, int n_slots, void* stream);

/* The head of one environment step in ONE launch (an addition to ABI 9, nothing else changed), over n rows of a
 * raw f32 observation obs [n, D] read at its own pitch ld_obs, and - optional - the latents z [n, Z] at ld_z.  Every output
 * is nullable, at least one is required; all pitches are in elements.
 *   xa, xc       (x_dtype: ASE_F32 / ASE_BF16 / ASE_F16; the actor's and the critic's input buffer)
 *                x[e * ld + j] = from_f32_plain<T>(y), y = ceil_nan(floor_nan((obs[e, j] - mean[j]) / std[j], -5), 5) for j < D:
 *                an IEEE f32 subtraction, an IEEE f32 division, each rounded on its own, then torch.clamp, under which a NaN
 *                stays NaN, then a plain RNE cast without saturation - rms_normalize_kernel's arithmetic operation by operation
 *                (csrc/rms.hip:197-203 with store_opt, rms.hip:181-183; the 16-byte variant rms.hip:218-232).  mean, std f32
 *                [D] are required with either.  Columns at and beyond D are not touched.
 *   zc, zs       (x_dtype; the critic input's concat block and the style chain's input buffer)
 *                zc[e * ld_zc + k] = zs[e * ld_zs + k] = from_f32<T>(z[e, k]) for k < Z: gather_rows_kernel's SATURATING
 *                conversion (rms.hip:257) - half: clamped to +-65504 by a median of three, under which a NaN is stored as
 *                -65504; bf16: RNE; f32: the bits.
 *   obses_out, z_out  (f32, a row pitch and a slot stride each) the raw rows copied BITWISE into experience slot s:
 *                obses_out[s * obses_slot_stride + e * ld_obses_out + j] = obs[e, j], z_out likewise from z - the
 *                E['obses'][n].copy_(obs) of learning/common_agent.py:253-262 and the latents' store of
 *                learning/ase_agent.py:66-100.  s = slot, or - slot_dev non-NULL (DEVICE int32 [1]) - the word read when the
 *                launch runs, ase_hip_rollout_store's convention: a word outside [0, n_slots) makes the WHOLE call write
 *                nothing, the normalised and converted outputs included.  With neither slot output the slot arguments (slot,
 *                slot_dev, n_slots) are ignored.
 * Each side moves 16 bytes per lane (16-bit outputs: one 8-byte store of four elements) or 4 bytes per lane, chosen on the
 * host; the result is bitwise the same.  Observation side, 16 bytes when: D % 4 == 0, ld_obs % 4 == 0, obs 16-byte aligned,
 * mean and std 16-byte aligned when xa or xc is given, every given xa / xc with ld % 4 == 0 and its base aligned to four
 * elements (16 bytes f32, 8 bytes 16-bit), obses_out (when given) with ld_obses_out % 4 == 0, obses_slot_stride % 4 == 0 and a
 * 16-byte aligned base.  Latent side: the same clauses on Z, ld_z, z, zc / zs and z_out.
 * Refused, on the host, before any launch (ASE_EINVAL): no output at all; n <= 0 or D <= 0; NULL obs; a pitch below its
 * width (ld_obs, ld_xa, ld_xc, ld_obses_out < D; ld_z, ld_zc, ld_zs, ld_z_out < Z); Z < 0 or Z > 0 without z; z_out, zc or zs
 * given with Z == 0; xa or xc without mean and std; an x_dtype outside the three; and, with a slot output: a slot stride below
 * n * pitch, n_slots <= 0, slot outside [0, n_slots) (checked also when slot_dev is given).
 * Replaces, per rollout step: the obses copy, ase_hip_rms_normalize into two outputs, two ase_hip_gather_rows and the latent
 * launch's z2 store. */
int ase_hip_rollout_head(const float* obs, int64_t ld_obs, int D, const float* z, int64_t ld_z, int Z, const float* mean,
                         const float* stdv, void* xa, int64_t ld_xa, void* xc, int64_t ld_xc, void* zc, int64_t ld_zc, void* zs,
                         int64_t ld_zs, int x_dtype, float* obses_out, int64_t ld_obses_out, int64_t obses_slot_stride,
                         float* z_out, int64_t ld_z_out, int64_t z_slot_stride, int n, int slot, const int32_t* slot_dev,
                         int n_slots, void* stream);

/* The step counter of a recorded rollout step: one lane computes *word = (*word + add) mod wrap - the sum in 64 bits, the
 * result in [0, wrap) also for a negative sum; wrap <= 0: no modulo, the low 32 bits of the sum (two's complement) - and
 * writes it with a plain vector store.  word: DEVICE int32 [1], the slot word ase_hip_rollout_store and ase_hip_rollout_head
 * read; a launch program ends its step with this entry.  Refused on the host: NULL word. */
int ase_hip_word_step(int32_t* word, int add, int wrap, void* stream);

/* The glue of the HRL agent's inner loop (additions to ABI 9, nothing else changed): one high-level step wraps
 * llc_steps simulator steps around the frozen low-level controller (learning/hrl_agent.py:45-82).  Three entries, each ONE
 * launch on a grid that depends on n alone, no atomics, no intermediate tensor, recordable in a launch program.  Every f32
 * operation named below is rounded on its own (no a * b + c contraction).
 *
 * ase_hip_hrl_latent, once per high-level step: z[e, :] = normalize(clamp(actions[e, :], -1, 1)) - the high-level
 *   preprocess_actions and F.normalize (learning/hrl_agent.py:89-93,235).  actions f32 [n, ld_a], dim in [1, 128], one wave
 *   per row.  The clamp is torch.clamp's: a NaN stays NaN, -0.0 stays -0.0.  The normalisation is ase_hip_normalize_rows'
 *   arithmetic (x / max(sqrt(sum x^2), 1e-12), the sum in the wave's butterfly order), so z is bitwise
 *   ase_hip_normalize_rows(torch.clamp(actions, -1, 1)).  z f32 [n, ld_z], nullable.  z2 (nullable): a second copy in
 *   z2_dtype (ASE_F32 / ASE_BF16 / ASE_F16; the 16-bit types rounded to nearest even, f16 saturating as ase_hip_gather_rows
 *   stores it) at pitch ld_z2 - the style chain's input buffer; columns [0, dim) only, the pad columns are not touched.
 *   Refused: NULL actions; neither z nor z2; dim outside [1, 128]; a pitch below dim; a z2_dtype outside the three; n < 1.
 *
 * ase_hip_hrl_llc_action, once per inner step: the padded f32 head output mu [n, ld_mu] -> the action the environment gets,
 *   out f32 [n, ld_out] (ASEAgent.preprocess_actions through learning/hrl_agent.py:238; rl_games rescale_actions), one lane per
 *   element, act in [1, 128].  clip != 0:
 *     out[e, j] = clamp(mu[e, j], -1, 1) * ((high[j] - low[j]) / 2) + ((high[j] + low[j]) / 2)
 *   in that order - the two bound terms, the multiply, then the add; the clamp keeps a NaN.  clip == 0: out[e, j] = mu[e, j],
 *   a strided copy; low / high may be NULL.  mu is read at its own pitch: no gather runs in front.
 *   Refused: NULL mu / out; clip without low / high; act outside [1, 128]; a pitch below act; n < 1.
 *
 * ase_hip_hrl_accum, once per inner step, one lane per environment (learning/hrl_agent.py:57-73).  acc: f32 [4, n] at row pitch
 *   acc_stride >= n = {task-reward sum, discriminator-reward sum, done count, terminate count}.  Each row does
 *     acc[k, e] = (first ? 0.0f : acc[k, e]) + x_k[e]
 *   (first != 0: the accumulator's content on entry does not matter and is not read; the 0.0f + turns a first -0.0 into +0.0,
 *   as the reference's 0.0 + tensor does) with x_0 = rewards[e]; x_1 = -log(max(1 - sigmoid(l), 1e-4)) * disc_scale of
 *   l = logit[e * ld_l], the device function of ase_hip_disc_reward; x_2, x_3 = the float values of dones[e] / terminate[e],
 *   typed by dones_kind / terminate_kind (ASE_KIND_*, as in ase_hip_rollout_store).  last != 0: the call also writes the finals,
 *     rewards_out[e] = acc[0, e] / (float)llc_steps, disc_out[e] = acc[1, e] / (float)llc_steps
 *   - an IEEE DIVISION, correctly rounded, NOT a multiplication by the rounded reciprocal (the two differ for llc_steps 3 and
 *   5) - and dones_out[e] = acc[2, e] > 0 ? 1.0f : 0.0f, terminate_out[e] likewise from acc[3, e] (f32; a NaN count gives 0,
 *   as the reference's (count > 0) mask).  last == 0 leaves the four outputs untouched, and they may be NULL.
 *   Optional groups: {terminate, terminate_out} (a player has no terminate: row 3 is not touched), {logit, disc_out} (row 1 is
 *   not touched).
 *   Refused: NULL rewards / dones / acc; a kind code outside the four; terminate_out without terminate or disc_out without logit;
 *   last with terminate but no terminate_out, or with logit but no disc_out; ld_l < 1 with a logit; llc_steps < 1; last without
 *   rewards_out / dones_out; acc_stride < n; n < 1.
 * Replaces, per inner step: F.normalize and the high-level clamp (hoisted to once per high-level step), the LLC's clamp and
 *   rescale_actions, _calc_disc_reward's reward expression, the four running sums, the two divisions and the two masks. */
int ase_hip_hrl_latent(const float* actions, int64_t ld_a, float* z, int64_t ld_z, void* z2, int64_t ld_z2, int z2_dtype,
                       int n, int dim, void* stream);
int ase_hip_hrl_llc_action(const float* mu, int64_t ld_mu, const float* low, const float* high, float* out, int64_t ld_out,
                           int n, int act, int clip, void* stream);
int ase_hip_hrl_accum(const float* rewards, const void* dones, int dones_kind, const void* terminate, int terminate_kind,
                      const float* logit, int64_t ld_l, float disc_scale, float* acc, int64_t acc_stride, int first, int last,
                      int llc_steps, float* rewards_out, float* disc_out, float* dones_out, float* terminate_out, int n,
                      void* stream);

/* One environment step's tensor work, ONE launch per side of the physics step (additions to ABI 9, nothing
 * else changed).  Fixed grids, no atomics, no host decision: both record in a launch program.  Every f32 operation is rounded on
 * its own (no a * b + c contraction); the arithmetic is the device functions ase_hip_humanoid_obs_max, ase_hip_humanoid_reset,
 * ase_hip_task_obs, ase_hip_task_reward and ase_hip_build_amp_obs call, so the outputs are bitwise theirs.
 *
 * State operands.  A per-body or per-dof operand is a base pointer, an environment stride and an element stride, in floats:
 *   element (e, b) sits at base + e * se + b * sb.  A contiguous [n, B, 3] tensor is (p, 3 B, 3); the position window of the
 *   simulator's packed [n, bodies_per_env, 13] rigid-body tensor is (p, 13 bodies_per_env, 13), rotation / velocity / angular
 *   velocity at p + 3 / + 7 / + 10; the two halves of the [n, D, 2] dof state are (p, 2 D, 2) and (p + 1, 2 D, 2).  root_states /
 *   tar_states [.., 13] and tar_contact_forces [.., 3] have one stride (actor e at base + e * stride).  Nothing is copied.
 *
 * ase_hip_env_pre_step, the pre_physics_step chain, one lane per (environment, dof):
 *   x = clamp(actions_in[e * ld_in + j], -clip_actions, clip_actions) (torch.clamp: a NaN stays NaN, -0.0 stays -0.0;
 *   VecTaskPython.step) -> actions[e * ld_actions + j], the environment's own copy;
 *   pd_control != 0: targets = pd_offset[j] + pd_scale[j] * x, the product and the sum each rounded (_action_to_pd_targets);
 *   pd_control == 0: targets = x * motor_efforts[j] * power_scale, left to right (humanoid.py:361-366);
 *   prev_root_pos (nullable) [n, 3] = root_states[e, 0:3] (heading, location, strike: humanoid_heading.py:81-85);
 *   recovery_counter (nullable) int32 [n] = max(recovery_counter - 1, 0) (humanoid_amp_getup.py:131-134).
 *   Refused: NULL actions_in / actions / targets; n_envs or n_dof < 1; a pitch below n_dof; clip_actions < 0 or NaN; PD control
 *   without pd_offset / pd_scale, torque control without motor_efforts; prev_root_pos without root_states at a stride >= 3.
 *
 * ase_hip_env_post_step, Humanoid.post_physics_step + HumanoidAMP.post_physics_step, 16 environments per block:
 *   progress_buf[e] += 1 (int64), and the incremented value is the one the reset test sees;
 *   the 15 n_bodies - 2 columns of compute_humanoid_observations_max at obs + e * ld_obs + col_offset and, with enable_task_obs,
 *   the task's 5 / 2 / 3 / 15 columns at obs + e * ld_obs + task_col_offset, every column clamped to +-clip_obs as torch.clamp
 *   does (a NaN stays NaN; clip_obs = INFINITY stores the value as computed);
 *   reward[e]: the task's reward (task_kind = ASE_TASK_*, operands as in ase_hip_task_reward, the reach body read from body_pos)
 *   or 1.0f with task_kind < 0; prev_root_pos is only read;
 *   reset[e], terminated[e] (int64): compute_humanoid_reset, the strike form with tar_contact_forces + strike_body_ids; then,
 *   with recovery_counter (nullable, int32 [n]), both are 0 while recovery_counter[e] > 0 (humanoid_amp_getup.py:136-142);
 *   hist (nullable) f32 [n, n_steps, F], F = 13 + 6 n_joints + n_dof + 3 n_key: every slot moves one step into the past, then
 *   the new frame takes slot 0 - root state and key bodies are body 0 and key_body_ids of the rigid-body operands.  hist NULL:
 *   the plain Humanoid; the dof operands and tables are then not read.
 *   Refused: a NULL required operand; n_bodies outside [1, 64]; F > 255; an element stride smaller than its element or an
 *   environment stride smaller than its elements; columns that do not fit ld_obs; clip_obs < 0 or NaN; a task operand missing
 *   for its kind or given without use (reward operands, plus the observation's with enable_task_obs); enable_task_obs without a
 *   task; dt <= 0 outside reach; body ids out of range; half a strike form; joints of other than 1 or 3 dofs.
 * Replaces, per step: progress_buf += 1, five contiguous copies and an indexed gather in front of build_amp_obs, the two
 *   launches of ase_hip_build_amp_obs, ase_hip_humanoid_obs_max, ase_hip_task_obs, ase_hip_task_reward, ase_hip_humanoid_reset,
 *   the two masked fills of the recovery mask and torch.clamp of the observation; the action clamp and clone, the PD-target
 *   expression, the prev_root_pos copy and the counter's sub / clamp. */
int ase_hip_env_pre_step(const float* actions_in, int64_t ld_in, float clip_actions, float* actions, int64_t ld_actions,
                         float* targets, int64_t ld_targets, int pd_control, const float* pd_offset, const float* pd_scale,
                         const float* motor_efforts, float power_scale, const float* root_states, int64_t root_stride,
                         float* prev_root_pos, int32_t* recovery_counter, int n_envs, int n_dof, void* stream);
int ase_hip_env_post_step(const float* body_pos, int64_t pos_se, int64_t pos_sb, const float* body_rot, int64_t rot_se,
                          int64_t rot_sb, const float* body_vel, int64_t vel_se, int64_t vel_sb, const float* body_ang_vel,
                          int64_t ang_se, int64_t ang_sb, const float* contact_forces, int64_t cf_se, int64_t cf_sb,
                          const float* dof_pos, int64_t dp_se, int64_t dp_sd, const float* dof_vel, int64_t dv_se, int64_t dv_sd,
                          int n_envs, int n_bodies, int n_dof, int local_root_obs, int root_height_obs, float* obs,
                          int64_t ld_obs, int col_offset, float clip_obs, int task_kind, int enable_task_obs,
                          int task_col_offset, const float* root_states, int64_t root_stride, const float* prev_root_pos,
                          const float* tar_a, const float* tar_b, const float* tar_speed, float tar_speed_scalar,
                          const float* tar_states, int64_t tar_stride, int reach_body_id, float dt, float* reward,
                          int64_t* progress_buf, const float* termination_heights, const int32_t* contact_body_ids,
                          int n_contact, const float* tar_contact_forces, int64_t tar_contact_stride,
                          const int32_t* strike_body_ids, int n_strike, float max_episode_length,
                          int enable_early_termination, const int32_t* recovery_counter, int64_t* reset, int64_t* terminated,
                          float* hist, int n_steps, const int32_t* dof_offsets, int n_joints, const int32_t* key_body_ids,
                          int n_key, void* stream);

/* The whole optimizer step of every dense layer in ONE launch: weight-only gradient terms (g += c * w: discriminator
 * weight decay / logit regulariser / encoder weight decay), their reported sums of squares (pre-update weights, into
 * acc[slot]), torch.optim.Adam, and the refreshed compute-dtype shadows W_s / W_s^T / bias (ase_hip_refresh_shadow_multi's
 * job).  desc: DEVICE int64[n_layers][24] = {W, n_real, k_real, Ws, ldws, Wts, ldwts, split_src, split_dst - split_src,
 * bias, bias_shadow, ceil(k_real/32), gW, mW, vW, gb, mb, vb, coefficient c (f32 bit pattern), acc slot A or -1,
 * acc slot B or -1, 0, 0, 0}.  opt_state NULL: shadows only.
 * Replaces: the weight terms of learning/amp_agent.py:449-466 + optimizer.step() (learning/ase_agent.py:287). */
int ase_hip_apply_multi(const int64_t* desc, int n_layers, const double* opt_state, double* acc, int dtype,
                        void* stream);
/* ... with a SECOND shadow pair per layer: desc2 = device int64 [n_layers, 8], row l = {Ws3, ldws3, Wts3, ldwts3, eb, 0, 0, 0} or all
 * zeros (none).  The tile that sends the fresh weight to the 16-bit shadows also writes the packed half-split shadows of W * 2^eb -
 * exactly what ase_hip_refresh_shadow(dtype = ASE_F32H3 | eb << 16) writes (same split function, same bytes; pitches in f32
 * elements, 32-byte aligned bases) - so the gradient penalty's value path needs no refresh launches of its own.  dtype ASE_F16 only (anything else is
 * refused with ASE_EINVAL: the bf16 instantiation would need more than the 64 registers the small kernels are held to). */
int ase_hip_apply_multi_v2(const int64_t* desc, int n_layers, const int64_t* desc2, const double* opt_state, double* acc,
                           int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Observation side.
 * ------------------------------------------------------------------------------------------- */

/* One frame of the AMP (discriminator) observation per environment from the simulator state, pushed into the history
 * hist [n_envs, n_steps, F], F = 13 + 6 n_joints + n_dof + 3 n_key: {root height, root rotation as tangent + normal
 * (heading-local when local_root_obs), heading-local root velocity and angular velocity, per joint tangent + normal of
 * its rotation (3-dof joints: exponential map; 1-dof: hinge about y), dof velocities, heading-local key body
 * positions}.  shift != 0: slots move one step into the past first; the new frame takes slot 0.  Quaternions xyzw.
 * dof_offsets: HOST int32[n_joints + 1], starting at 0 and ending at n_dof, joints of 1 or 3 dofs, n_joints in 1..32.
 * n_key == 0: no key columns, key_body_pos may be NULL.  F <= 255 (the 64 x (F + 1) float staging tile is 64 KB at F = 255);
 * a wider frame is refused.  n_steps == 1 with shift: nothing but slot 0 changes.
 * Pinned by tests/test_gpu_amp_obs.py (the reference's values, tests/ref_amp_obs.py): column 0, the dof velocity columns
 * and every shifted slot are copies, bit for bit.  An exponential map whose wrapped length is at most 1e-5 - and any map
 * with a NaN or infinite component, or a length that overflows f32 (|e| ~ 1e30: sin(inf) is NaN and NaN > 1e-5 is false)
 * - is the identity rotation (1, 0, 0, 0, 0, 1), not NaN.  A NaN or infinite hinge angle gives NaN in that joint's six
 * columns; in root_rot, NaN in every root and key column but column 0; in root_vel, root_ang_vel or a key position,
 * that vector's three columns and no other: all NaN for a NaN or an infinite x / y component (0 * inf inside the
 * rotation about z), NaN, NaN and an infinity or NaN for an infinite z component.
 * A root rotation whose x axis turns exactly vertical has heading atan2(0, 0) = 0.
 * Replaces: build_amp_observations + _update_hist_amp_obs (env/tasks/humanoid_amp.py:248-266,280-316),
 *   dof_to_obs (env/tasks/humanoid.py:523-552). */
int ase_hip_build_amp_obs(const float* root_pos, const float* root_rot, const float* root_vel,
                          const float* root_ang_vel, const float* dof_pos, const float* dof_vel,
                          const float* key_body_pos, int n_envs, int n_dof, int n_key, const int32_t* dof_offsets,
                          int n_joints, int local_root_obs, int root_height_obs, float* hist, int n_steps, int shift,
                          void* stream);

/* Motion-clip sampler: the reference pose at (motion id, time) for n samples from the concatenated clip tensors
 * (global translations gts [frames, B, 3], global / local rotations grs / lrs [frames, B, 4] xyzw, root velocities
 * grvs / gravs [frames, 3], dof velocities dvs [frames, D]; per motion: lengths [s], num_frames, dt, length_starts):
 * frame pair + blend, linear interpolation of positions, spherical interpolation of rotations, local rotations ->
 * dof positions (3-dof: exponential map, 1-dof: angle about y).  Outputs feed ase_hip_build_amp_obs (demo stream).
 * dof_body_ids / dof_offsets / key_body_ids: HOST int32 arrays; everything else device memory.  dof_offsets start at 0
 * (refused otherwise), joints of 1 or 3 dofs, body ids inside [0, n_bodies); n_key == 0: key_pos and key_body_ids may be
 * NULL.  motion_ids are NOT checked on the device.
 * Times are used as given (pinned by tests/test_gpu_amp_obs.py): outside [0, length] the frame pair clips to the first
 * two frames / the last frame twice while the blend (t - i0 dt) / dt keeps following t, so positions and rotations
 * EXTRAPOLATE below 0 exactly as the reference's do (the demo fetch and the reset history ask for times down to
 * -(n_steps - 1) dt) and stay on the last frame above the length; velocities are copies of frame i0.  slerp: neighbours
 * with a negative dot product are negated first, sin(half angle) < 0.001 gives the midpoint 0.5 q0 + 0.5 q1 whatever
 * the blend, a dot product >= 1 gives q0.  A local rotation with |w| >= 1 (sin_theta <= 1e-5, or NaN from w > 1) gives
 * dof positions 0; w < 0 gives angles past pi, wrapped into (-pi, pi]; a hinge angle is wrapped a second time.
 * Replaces: MotionLib.get_motion_state (utils/motion_lib.py:122-172,263-272,296-325). */
int ase_hip_motion_state(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                         const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames, const float* dt,
                         const int32_t* length_starts, const int32_t* motion_ids, const float* times, int n,
                         const int32_t* dof_body_ids, const int32_t* dof_offsets, int n_joints,
                         const int32_t* key_body_ids, int n_key, float* root_pos, float* root_rot, float* dof_pos,
                         float* root_vel, float* root_ang_vel, float* dof_vel, float* key_pos, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Environment side: the tensor functions a task runs every simulator step on the rigid-body state.
 * Quaternions xyzw, every state tensor contiguous f32 on the device.  The observation entries write rows of a caller's
 * buffer: row e of the output starts at obs + e * ld_obs + col_offset, so the humanoid and the task observation sit side
 * by side in one obs_buf (env/tasks/humanoid_amp_task.py:51-64).  env_ids (DEVICE int32[n_ids], NULL with n_ids = 0: every
 * environment) names the environments to compute; only their rows are written (obs_buf[env_ids] = obs), ids outside
 * [0, n_envs) are skipped.
 * ------------------------------------------------------------------------------------------- */

/* The policy observation of the humanoid, F = 15 n_bodies - 2 columns (253 for 17 bodies): {root height (0 unless
 * root_height_obs), heading-local positions of bodies 1.. relative to the root (the root's own three columns are dropped),
 * tangent + normal of every body's heading-local rotation (6 each), heading-local linear and angular velocities}.  With
 * local_root_obs the root's six rotation columns are the tangent / normal of its RAW rotation, as in the reference.
 * body_pos / body_vel / body_ang_vel [n_envs, n_bodies, 3], body_rot [n_envs, n_bodies, 4]; n_bodies <= 64.
 * Replaces: compute_humanoid_observations_max + _compute_humanoid_obs / _compute_observations
 *   (env/tasks/humanoid.py:385-413,592-636). */
int ase_hip_humanoid_obs_max(const float* body_pos, const float* body_rot, const float* body_vel,
                             const float* body_ang_vel, int n_envs, int n_bodies, int local_root_obs,
                             int root_height_obs, const int32_t* env_ids, int n_ids, float* obs, int64_t ld_obs,
                             int col_offset, void* stream);

/* Termination test: terminated = early termination && progress > 1 && (a body outside contact_body_ids carries a contact force
 * component above 0.1 AND one of them is below its termination height); reset = progress >= max_episode_length - 1 ? 1 :
 * terminated.  Strike form (tar_contact_forces [n_envs, 3] and strike_body_ids both non-NULL): also terminated when the
 * target is touched (|x| or |y| force above 1) while a body that is neither a contact nor a strike body carries a force
 * above 1.  contact_body_ids / strike_body_ids: HOST int32 arrays (turned into body bit masks: n_bodies <= 64);
 * progress_buf / reset / terminated: int64 [n_envs]; contact_forces, body_pos [n_envs, n_bodies, 3];
 * termination_heights [n_bodies].
 * Replaces: compute_humanoid_reset (env/tasks/humanoid.py:645-672) and its strike form
 *   (env/tasks/humanoid_strike.py:255-297). */
int ase_hip_humanoid_reset(const int64_t* progress_buf, const float* contact_forces, const float* body_pos,
                           const float* termination_heights, const int32_t* contact_body_ids, int n_contact,
                           const float* tar_contact_forces, const int32_t* strike_body_ids, int n_strike, int n_envs,
                           int n_bodies, float max_episode_length, int enable_early_termination, int64_t* reset,
                           int64_t* terminated, void* stream);

/* The tasks of the high-level controller.  An operand a kind does not use must be NULL, one it uses must not be. */
enum { ASE_TASK_HEADING = 0, ASE_TASK_LOCATION = 1, ASE_TASK_REACH = 2, ASE_TASK_STRIKE = 3 };

/* Task observation, 5 / 2 / 3 / 15 columns (root_states [n_envs, 13] = position, rotation, velocity, angular velocity):
 *   HEADING : tar_a = target direction [n, 2], tar_b = target facing direction [n, 2], tar_speed [n]
 *             -> {local direction xy, speed, local facing direction xy}
 *   LOCATION: tar_a = target position [n, 2] -> heading-local xy of (target - root)
 *   REACH   : tar_a = target position [n, 3] (already relative) -> heading-local xyz
 *   STRIKE  : tar_states [n, 13] -> heading-local {position (height absolute), rotation tangent + normal, velocity,
 *             angular velocity}
 * Replaces: compute_heading_observations (env/tasks/humanoid_heading.py:231-250), compute_location_observations
 *   (env/tasks/humanoid_location.py:169-183 and env/tasks/humanoid_reach.py:174-182), compute_strike_observations
 *   (env/tasks/humanoid_strike.py:193-219) + the _compute_task_obs of each task. */
int ase_hip_task_obs(int kind, const float* root_states, const float* tar_a, const float* tar_b, const float* tar_speed,
                     const float* tar_states, int n_envs, const int32_t* env_ids, int n_ids, float* obs, int64_t ld_obs,
                     int col_offset, void* stream);

/* Task reward [n_envs] with the reference's literal weights and scales:
 *   HEADING : root_states, prev_root_pos [n, 3], tar_a, tar_b, tar_speed [n], dt
 *   LOCATION: root_states, prev_root_pos, tar_a [n, 2], tar_speed_scalar, dt
 *   REACH   : body_pos [n, n_bodies, 3] (body_id = the reaching body), tar_a [n, 3]
 *   STRIKE  : root_states, prev_root_pos, tar_states [n, 13], dt
 * Non-finite operands: the rewards are the reference's, NaN for NaN.  Its clamps are torch.clamp_min, which keeps a NaN, and so
 * do the clamps here (the heading and location facing terms, the location and strike speed errors, the strike rotation
 * term): a NaN in an operand that reaches a reward's arithmetic gives a NaN reward, never a plausible finite one.  A comparison
 * with a NaN is false, so a NaN speed is not "<= 0", a NaN pos_err not "< 0.5", a NaN tar_rot_err not "< 0.2"; where an override
 * holds (LOCATION: pos_err < 0.5 sets the velocity and facing terms to 1; STRIKE: tar_rot_err < 0.2 sets the reward to 1) it
 * replaces a NaN term as it does in the reference.  REACH has no clamp: exp(-4 |tar - body|^2), NaN for NaN, 0 for an infinity.
 * Replaces: compute_heading_reward (env/tasks/humanoid_heading.py:252-289), compute_location_reward
 *   (env/tasks/humanoid_location.py:185-232), compute_reach_reward (env/tasks/humanoid_reach.py:184-196),
 *   compute_strike_reward (env/tasks/humanoid_strike.py:221-252). */
int ase_hip_task_reward(int kind, const float* root_states, const float* prev_root_pos, const float* tar_a,
                        const float* tar_b, const float* tar_speed, float tar_speed_scalar, const float* tar_states,
                        const float* body_pos, int n_bodies, int body_id, float dt, int n_envs, float* reward,
                        void* stream);

/* Target draws and resets of the four tasks (an addition to ABI 9, nothing else changed): new targets and new
 * change steps for the selected environments, in ONE launch, one lane per row, no intermediate tensor.
 * Which rows:
 *   ids mode: env_ids (DEVICE int32[n_ids], DISTINCT) names them - _reset_task(env_ids) / _reset_target(env_ids); ids
 *             outside [0, n_envs) are skipped.
 *   due mode: env_ids NULL with n_ids = 0: every environment e with progress_buf[e] >= change_steps[e], tested inside the
 *             kernel - _update_task without nonzero, without a host round trip, on a fixed grid.  Refused for STRIKE (it has
 *             no change steps).
 * Where the draws come from - exactly one of u and rng_state is non-NULL:
 *   u         f32 [n_ids, U] uniforms in [0, 1), ids mode only, in the order of the reference's torch.rand calls: HEADING
 *             U = 3 {theta, face theta, speed}, LOCATION 2 {x, y}, REACH 3 {x, y, height}, STRIKE 4 {near test, distance,
 *             theta, rotation theta}; with it steps int64 [n_ids], what torch.randint(low, high) returned (NULL for STRIKE).
 *             Row i of both belongs to env_ids[i].
 *   rng_state u64[2] = {seed, offset} on the device, as in ase_hip_sample_latents; steps must be NULL.  The draws of
 *             environment e depend on (seed, offset, e) only, not on its position in env_ids or on the other rows: uniform
 *             j is (word 2 of Philox4x32-10 at element 4 e + j, same counter / key layout as above) >> 8, times 2^-24; the
 *             change steps are steps_low + (((uint64)w * (uint64)(steps_high - steps_low)) >> 32) with w = word 0 of
 *             element 4 e + 3 - an integer in [steps_low, steps_high), exactly.  advance != 0: the offset moves on by one
 *             behind the launch (also when env_ids is empty: a call is one stream position).
 * What is written, for the selected rows only, f32 operation by operation in the reference's order (2 pi and pi are the f32
 * roundings of the f64 constants; sinf / cosf):
 *   HEADING : theta = 2 pi u0 - pi, face = 2 pi u1 - pi (both 0 unless enable_rand_heading); tar_a [n, 2] = (cos, sin) theta,
 *             tar_b [n, 2] = (cos, sin) face; tar_speed [n] = (float)(tar_speed_max - tar_speed_min) u2 + tar_speed_min
 *   LOCATION: tar_a [n, 2] = root_states[e, 0:2] + tar_dist_max (2 u - 1)
 *   REACH   : tar_a [n, 3] = {tar_dist_max (2 u0 - 1), tar_dist_max (2 u1 - 1), (float)(tar_height_max - tar_height_min) u2 +
 *             tar_height_min}
 *   STRIKE  : d = ((u0 < near_prob ? near_dist : tar_dist_max) - tar_dist_min) u1 + tar_dist_min; target_states[e] =
 *             {d cos(2 pi u2) + root x, d sin(2 pi u2) + root y, 0.9, quat_from_angle_axis(2 pi u3, z) normalised, 0 x 6}.
 *             root_states is read when the launch runs: the reference calls _reset_target after the actor reset wrote the
 *             new root, so this call comes after ase_hip_amp_reset on the stream.
 *   all but STRIKE: change_steps[e] = progress_buf[e] + steps (int64 [n_envs] both).
 * Every other row and column is untouched.  root_states / target_states: row e at base + e * ld (ld_root, ld_target >= 13:
 * views of the simulator's [n_envs, actors, 13] tensor).  An operand a kind does not use must be NULL, one it uses must not
 * be; the range arguments a kind does not use are ignored.  steps_high - steps_low in [1, 2^32 - 1].
 * Replaces: HumanoidHeading._update_task / _reset_task (env/tasks/humanoid_heading.py:147-174), HumanoidLocation
 *   (env/tasks/humanoid_location.py:107-125), HumanoidReach (env/tasks/humanoid_reach.py:111-130),
 *   HumanoidStrike._reset_target (env/tasks/humanoid_strike.py:108-128). */
int ase_hip_task_reset(int kind, const int32_t* env_ids, int n_ids, const float* u, const int64_t* steps,
                       uint64_t* rng_state, int advance, const int64_t* progress_buf, int64_t* change_steps,
                       int64_t steps_low, int64_t steps_high, const float* root_states, int64_t ld_root, float* tar_a,
                       float* tar_b, float* tar_speed, float* target_states, int64_t ld_target, double tar_speed_min,
                       double tar_speed_max, double tar_dist_min, double tar_dist_max, double tar_height_min,
                       double tar_height_max, double near_dist, double near_prob, int enable_rand_heading, int n_envs,
                       void* stream);

/* The projectile launches of the perturbation task (an addition to ABI 9, nothing else changed):
 * HumanoidPerturb._update_proj in ONE launch, one lane per environment (or per id), on a fixed grid, no intermediate tensor.
 * Which slot (projectile) and which rows:
 *   due mode      slot = -1, env_ids NULL: progress_buf (DEVICE int64, element 0 is read - the reference's semantics: the counter
 *                 of environment 0 decides for ALL environments) and timesteps (DEVICE int32 [n_slots], the cumulative sums of the
 *                 objects' step counts, strictly increasing and positive) are read when the launch runs: t = progress_buf[0] mod
 *                 (timesteps[n_slots - 1] + 1), the launched slot is the first k with timesteps[k] == t.  Without such a k
 *                 nothing is written but slot_out = -1 and ids_out[e] = -1.  No host read, no nonzero, no where.
 *   explicit mode 0 <= slot < n_slots from the caller (progress_buf, timesteps NULL), for every environment or for the rows
 *                 env_ids (DEVICE int32 [n_ids], DISTINCT); ids outside [0, n_envs) are skipped and never dereferenced.
 *   n_slots in 1 .. 32.
 * Where the seven draws of a row come from - exactly one source:
 *   u, eps    f32 [rows, 4] uniforms {theta, distance, height, speed} and f32 [rows, 3] normals (the direction noise), both
 *             contiguous; rows = n_ids with env_ids (row i belongs to env_ids[i]), else n_envs.
 *   rng_state u64[2] = {seed, offset} on the device, as in ase_hip_task_reset.  Draw j of environment e comes from element
 *             8 e + j of the stream and depends on (seed, offset, e) only ("uniform": the 24-bit uniform (c[2] >> 8) * 2^-24 of
 *             the element, "normal": its Box-Muller normal from words 0 and 1, as in ase_hip_sample_latents):
 *               j = 0  uniform  theta = (float)(2 pi) u
 *               j = 1  uniform  distance = (float)(dist_max - dist_min) u + dist_min
 *               j = 2  uniform  height = (float)(h_max - h_min) u + h_min
 *               j = 3 .. 5  normal   the noise of the launch direction x, y, z
 *               j = 6  uniform  speed = (float)(speed_max - speed_min) u + speed_min
 *             advance != 0: the offset moves on by one behind the launch, whether or not a launch was due (a call is one
 *             stream position).
 *   draws_out (nullable) f32 [n_envs, 7]: row e receives the draws of a launched environment e in the order j = 0 .. 6.
 * What a launched row writes, f32 operation by operation in the reference's order (range differences taken in double and rounded
 * once; sinf / cosf / sqrtf), into proj_states + e * ld_env + slot * ld_slot (13 floats; ld_env, ld_slot >= 13):
 *   p = {root x + distance cos(theta), root y + (-distance) sin(theta), height}              columns 0:3
 *   columns 3:6 = 0, column 6 = 1, columns 10:13 = 0
 *   d = (target body position - p) + (float)noise * normals; d / max(|d|, 1e-12) (F.normalize: a NaN stays a NaN)
 *   velocity = speed * d, + the target body's velocity in x and y only                             columns 7:10
 * Operands are read in place from the simulator's layout: root_states row e at + e * ld_root (ld_root >= 13); the target body's
 * position at body_pos + e * pos_se + tar_body * pos_sb, its velocity at body_vel + e * vel_se + tar_body * vel_sb (strides in
 * floats, >= 3; tar_body in [0, n_bodies); the reference hard-codes body 1).  Every other slot, actor and row is untouched.
 * Outputs besides the row (nullable): slot_out int32 [1], the launched slot or -1; ids_out int32 [n_envs] (not with env_ids),
 * EVERY element written: e where environment e launched, -1 elsewhere - the full-length id list of ase_hip_rollout_store /
 * ase_hip_amp_reset_due, here for the simulator's indexed root-state set call.
 * Replaces: HumanoidPerturb._update_proj (env/tasks/humanoid_perturb.py:172-213) but its set_actor_root_state_tensor_indexed. */
#define ASE_PROJ_DRAWS 7
#define ASE_PROJ_MAX_SLOTS 32
int ase_hip_proj_launch(const int64_t* progress_buf, const int32_t* timesteps, int n_slots, int slot, const int32_t* env_ids,
                        int n_ids, const float* u, const float* eps, uint64_t* rng_state, int advance, const float* root_states,
                        int64_t ld_root, const float* body_pos, int64_t pos_se, int64_t pos_sb, const float* body_vel,
                        int64_t vel_se, int64_t vel_sb, int n_bodies, int tar_body, float* proj_states, int64_t ld_env,
                        int64_t ld_slot, double dist_min, double dist_max, double h_min, double h_max, double speed_min,
                        double speed_max, double noise, int32_t* slot_out, int32_t* ids_out, float* draws_out, int n_envs,
                        void* stream);

/* The view-motion task (an addition to ABI 9, nothing else changed): the per-step logic of HumanoidViewMotion in
 * ONE launch, one lane per environment on a fixed grid over all n_envs, no host read, no intermediate tensor; recordable.
 * motion_ids (DEVICE int32 [n_envs]), progress_buf, reset_buf, terminate_buf (DEVICE int64 [n_envs]) are the task's buffers.
 * mode ASE_MOTION_SYNC = _compute_reset + _motion_sync, per environment e with m = motion_ids[e]:
 *   t = (float)progress_buf[e] * (float)motion_dt - torch's product of an integer tensor and a Python float: the counter is
 *       rounded to f32 (exact below 2^24), motion_dt (the f64 product controlFrequencyInv * sim dt) is rounded to f32 ONCE, on
 *       the host, and the product is one f32 multiplication
 *   reset_buf[e] = t > lengths[m] (strict), terminate_buf[e] = 0
 *   the pose of (m, t) by the sampler of ase_hip_motion_state (the same device functions, the same bits):
 *   root_states + e * ld_root (ld_root >= 13): position, rotation, then six +0.0 for the two velocities - the humanoid's row of
 *       the packed root tensor, whatever actors lie beside it
 *   dof_pos + e * dp_se + d * dp_sd = the dof positions, dof_vel + e * dv_se + d * dv_sd = +0.0 (strides in floats; Isaac Gym's
 *       interleaved dof state [n, D, 2] is element stride 2)
 *   optional (NULL: skipped) rigid-body outputs at + e * se + b * sb: body_pos [n, B, 3] = body b's global translation of the
 *       frame pair, blended by the key-body expression; body_rot [n, B, 4] = body b's global rotation of the frame pair, blended
 *       by the root rotation's expression (slerp); body 0 is bitwise the root row.  body_vel / body_ang_vel [n, B, 3] = +0.0.
 *       These are the clip's own arrays: no forward kinematics runs.
 *   env_ids, ids_out: NULL.  Every other element of every operand is untouched.
 * mode ASE_MOTION_RESET = _reset_env_tensors, for every e with reset_buf[e] != 0 (env_ids NULL) or for the rows env_ids (DEVICE
 *   int32 [n_ids], DISTINCT, n_ids <= n_envs; -1 and ids outside [0, n_envs) are skipped and never dereferenced):
 *   motion_ids[e] = (motion_ids[e] + n_envs) mod num_motions, progress_buf[e] = reset_buf[e] = terminate_buf[e] = 0.
 *   It writes NO state (every state and clip operand NULL / ignored): the reference's override does not call the base class's
 *   indexed set, so a reset environment shows the old clip's last pose until the next ASE_MOTION_SYNC.
 *   ids_out (nullable, not with env_ids) int32 [n_envs], EVERY element written: e where environment e was reset, -1 elsewhere -
 *   the full-length id list of ase_hip_amp_reset_due.
 * In both modes a row whose motion_ids[e] is outside [0, num_motions) writes nothing to the buffers (ids_out[e] = -1).
 * Host checks: dof_offsets[0] == 0, joints of 1 or 3 dofs on bodies in range, n_bodies <= ASE_MOTION_SYNC_MAX_BODIES,
 * n_joints <= 32, num_motions >= 1, strides that cover the widths.
 * Replaces: HumanoidViewMotion._motion_sync, _compute_reset / compute_view_motion_reset, _reset_env_tensors
 * (env/tasks/humanoid_view_motion.py:44-97) but the two indexed set calls. */
enum { ASE_MOTION_SYNC = 0, ASE_MOTION_RESET = 1 };
#define ASE_MOTION_SYNC_MAX_BODIES 64
int ase_hip_motion_sync(int mode, const float* gts, const float* grs, const float* lrs, int n_bodies, const float* lengths,
                        const int32_t* num_frames, const float* dt, const int32_t* length_starts, int num_motions,
                        const int32_t* dof_body_ids, const int32_t* dof_offsets, int n_joints, int32_t* motion_ids,
                        int64_t* progress_buf, double motion_dt, int64_t* reset_buf, int64_t* terminate_buf,
                        float* root_states, int64_t ld_root, float* dof_pos, int64_t dp_se, int64_t dp_sd, float* dof_vel,
                        int64_t dv_se, int64_t dv_sd, float* body_pos, int64_t bp_se, int64_t bp_sb, float* body_rot,
                        int64_t br_se, int64_t br_sb, float* body_vel, int64_t bv_se, int64_t bv_sb, float* body_ang_vel,
                        int64_t ba_se, int64_t ba_sb, const int32_t* env_ids, int n_ids, int32_t* ids_out, int n_envs,
                        void* stream);

/* Renewals of the ASE agent's per-environment latents (an addition to ABI 9, nothing else changed): new unit
 * latents and new step counts for the selected environments, in ONE launch, one wave per row (lanes j and j + 64 hold the
 * row's elements, dim 1 .. 128), no intermediate tensor.
 * Which rows:
 *   ids mode: env_ids (DEVICE int32[n_ids], DISTINCT) names them - _reset_latents(env_ids) of env_reset and of the player;
 *             ids outside [0, n_envs) are skipped and never dereferenced.
 *   due mode: env_ids NULL with n_ids = 0: every environment e with reset_steps[e] <= progress_buf[e], tested inside the
 *             kernel - _update_latents without any / nonzero, without a host round trip, on a fixed grid.  progress_buf is
 *             int64 [n_envs] when progress_i64 is set, else int32 [n_envs]; it is NULL in ids mode.
 * A renewed row: latents[e, 0:dim] = v / max(|v|, 1e-12) with v the row's dim normals (torch.nn.functional.normalize; a NaN
 * in v makes the row NaN, an all-zero v gives zeros), row e at latents + e * ld_z (ld_z >= dim).  Rows that are not
 * renewed are not written.
 * The step counts, only if reset_steps (int32 [n_envs]) is given: steps_add = 0: reset_steps[e] = s
 * (_reset_latent_step_count); steps_add != 0: reset_steps[e] += s (_update_latents; required in due mode, which also
 * requires reset_steps).  Without reset_steps (the player's resets) no step is drawn and steps must be NULL.
 * Where the draws come from - exactly one of eps and rng_state is non-NULL:
 *   eps       f32 [n_ids, >= dim] normals with row stride ld_eps, ids mode only, and with it steps int32 [n_ids] (what
 *             torch.randint_like returned) whenever reset_steps is given.  Row i of both belongs to env_ids[i].
 *   rng_state u64[2] = {seed, offset} on the device, as in ase_hip_sample_latents; steps must be NULL.  Normal j of
 *             environment e is the normal of element e * dim + j: a renewed row e is row e of
 *             ase_hip_sample_latents(rows = n_envs, dim) at the same stream position, whichever other rows are renewed.  The
 *             step count is steps_low + (((uint64)w * (uint64)(steps_high - steps_low)) >> 32) with w = output word 3 of
 *             element e * dim (words 0 and 1 make that element's normal, word 2 its keep-uniform) - an integer in
 *             [steps_low, steps_high), exactly; steps_high - steps_low in [1, 2^32 - 1] and the range within int32.
 *             advance != 0: the offset moves on by one behind the launch (also when env_ids is empty: a call is one stream
 *             position).
 * z2 (nullable, due mode only): a second output [n_envs, ld_z2 >= dim] in z2_dtype (ASE_F32 / ASE_F16 / ASE_BF16, converted
 * as in ase_hip_sample_latents): row e receives the latent of EVERY environment after the decision, renewed or kept - the
 * copy of all latents into the step's experience slot, folded into the launch.
 * Replaces: ASEAgent.env_reset's latent part, _reset_latent_step_count, _reset_latents, _update_latents
 *   (learning/ase_agent.py:310-379), ASEPlayer._reset_latents (learning/ase_players.py), and the ase_latents copy of
 *   play_steps (learning/ase_agent.py:36-115). */
int ase_hip_latent_renew(const int32_t* env_ids, int n_ids, const float* eps, int64_t ld_eps, const int32_t* steps,
                         uint64_t* rng_state, int advance, const void* progress_buf, int progress_i64, int32_t* reset_steps,
                         int steps_add, int64_t steps_low, int64_t steps_high, float* latents, int64_t ld_z, void* z2,
                         int64_t ld_z2, int z2_dtype, int n_envs, int dim, void* stream);

/* HumanoidAMP / HumanoidAMPGetup resets (ABI 9): for n_ids environments, state initialisation and the refill of
 * their AMP observation history hist [n_envs, n_steps, F] (F as in ase_hip_build_amp_obs), all in ONE launch.
 * Row i of the plan (DEVICE arrays of length n_ids, read when the launch runs - a recorded launch follows their
 * contents; n_ids is fixed when it is recorded) resets environment e = env_ids[i] the way kind[i] says:
 *   ASE_RESET_FRAME : slot 0 of e's history is recomputed, nothing else is touched (_compute_amp_observations(env_ids);
 *                     the recovery episodes of the get-up task)
 *   ASE_RESET_TABLE : root_states / dof_pos / dof_vel of e are copied from row src_rows[i] of the state table
 *                     (tab_root_states [n_tab, 13], tab_dof_pos / tab_dof_vel [n_tab, D]: the initial state with
 *                     src_rows[i] = e for _reset_default, the fall states for _reset_fall_episode), slot 0 is computed and
 *                     copied into slots 1 .. n_steps - 1 (_init_amp_obs_default)
 *   ASE_RESET_MOTION: the pose of motion motion_ids[i] at motion_times[i] (the sampler of ase_hip_motion_state, same clip
 *                     tensors and HOST index arrays) goes to root_states[e, 0:13], dof_pos[e], dof_vel[e]
 *                     (_reset_ref_state_init + _set_env_state); slot 0 is computed, slot k = 1 .. n_steps - 1 is the frame
 *                     of the motion at the f32 time motion_times[i] + (float)(-env_dt) * (float)k, used UNCLAMPED as the
 *                     reference does (_init_amp_obs_ref): before the clip's start the phase clips to frame 0 and the
 *                     blend turns negative, i.e. the interpolation extrapolates.
 * Slot 0 always comes from the simulator tensors body_pos / body_vel / body_ang_vel [n_envs, n_bodies, 3], body_rot
 * [n_envs, n_bodies, 4] (root = body 0, key bodies = key_body_ids) and e's dof_pos / dof_vel as this call leaves them.
 * env_ids MUST BE DISTINCT (two rows of one environment race).  A row whose id lies outside [0, n_envs), whose kind is
 * unknown or not announced in `kinds`, or whose src_rows[i] lies outside the table is skipped; motion_ids must be valid.
 * kinds: HOST mask of the kinds that may occur, ASE_RESET_HAS_TABLE | ASE_RESET_HAS_MOTION; without a bit the operands of
 * that kind (table + src_rows; clip tensors + dof_body_ids + motion_ids + motion_times) may be NULL.
 * root_states: row e at root_states + e * ld_root.  Dof d of environment e: dof_pos[e * ld_dof + d * dof_stride], same
 * for dof_vel; dof_stride = 1: two plain tensors, 2: the simulator's interleaved [n_envs, D, 2] tensor (dof_vel =
 * dof_pos + 1).  n_steps <= 64; n_joints, n_key <= 32.
 * Replaces: HumanoidAMP._reset_actors / _reset_default / _reset_ref_state_init / _set_env_state / _init_amp_obs /
 *   _init_amp_obs_default / _init_amp_obs_ref / _compute_amp_observations(env_ids) (env/tasks/humanoid_amp.py:141-246,
 *   257-275), HumanoidAMPGetup._reset_fall_episode / _init_amp_obs (env/tasks/humanoid_amp_getup.py:109-129). */
enum { ASE_RESET_FRAME = 0, ASE_RESET_TABLE = 1, ASE_RESET_MOTION = 2 };
enum { ASE_RESET_HAS_TABLE = 1, ASE_RESET_HAS_MOTION = 2 };
int ase_hip_amp_reset(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                      const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames, const float* dt,
                      const int32_t* length_starts, const int32_t* dof_body_ids, const int32_t* dof_offsets, int n_joints,
                      const int32_t* key_body_ids, int n_key, const int32_t* env_ids, const int32_t* kind,
                      const int32_t* motion_ids, const float* motion_times, const int32_t* src_rows, int n_ids, int kinds,
                      const float* tab_root_states, const float* tab_dof_pos, const float* tab_dof_vel, int n_tab,
                      float* root_states, int64_t ld_root, float* dof_pos, float* dof_vel, int64_t ld_dof, int dof_stride,
                      const float* body_pos, const float* body_rot, const float* body_vel, const float* body_ang_vel,
                      int n_envs, int local_root_obs, int root_height_obs, float env_dt, float* hist, int n_steps,
                      void* stream);

/* The same resets with the due test and the draws inside the launch (an addition to ABI 9, nothing else
 * changed): ONE launch over all n_envs environments, no plan from the host, no nonzero, no host round trip, a fixed grid.
 * Environment e is reset iff reset_buf[e] != 0 (progress_buf / reset_buf / terminate_buf: DEVICE int64 [n_envs]).  How it is
 * reset follows from draws that depend on (seed, offset, e) only, rng_state = u64[2] {seed, offset} on the device as in
 * ase_hip_task_reset.  Draw j of environment e comes from element 8 e + j of the stream; all six are defined for every
 * environment, whichever branch uses them ("uniform": the 24-bit uniform (c[2] >> 8) * 2^-24 of the element, f32):
 *   j = 0  uniform u0     getup: a recovery episode (ASE_RESET_FRAME) iff u0 < (float)recovery_episode_prob and
 *                         terminate_buf[e] == 1
 *   j = 1  uniform u1     getup, else: a fall episode iff u1 < (float)fall_init_prob
 *   j = 2  output word 0  the fall row: ASE_RESET_TABLE with src = n_envs + (((uint64)word * (uint64)n_fall) >> 32),
 *                         n_fall = n_tab - n_envs (exact, never reaches n_tab)
 *   j = 3  uniform u3     ASE_INIT_HYBRID: a motion row iff u3 < (float)hybrid_init_prob, else the default row
 *   j = 4  v = c[2] >> 8  the 24-bit integer behind the uniform: the clip of a motion row is the first m with v < cdf[m]
 *   j = 5  uniform u5     motion_time = u5 * lengths[clip], one f32 product; ASE_INIT_START: 0
 * Otherwise state_init decides: ASE_INIT_DEFAULT: ASE_RESET_TABLE with src = e; ASE_INIT_START / ASE_INIT_RANDOM:
 * ASE_RESET_MOTION; ASE_INIT_HYBRID: j = 3.  Without getup, j = 0 .. 2 are unused.
 * cdf: DEVICE uint32 [n_clips], non-decreasing, cdf[m] = floor(2^24 * cumsum(w)[m] / sum(w) + 0.5) taken in f64, the last entry
 * 2^24: clip m has probability (cdf[m] - cdf[m - 1]) / 2^24 exactly, a clip of weight zero is never drawn.
 * A reset row is then treated exactly as ase_hip_amp_reset treats a plan row of that (kind, motion_id, motion_time, src_row):
 * the same kernel body.  The state table holds the initial state in rows [0, n_envs) and the fall states behind it.
 * In the same launch, for reset rows only: progress_buf[e] = reset_buf[e] = terminate_buf[e] = 0 (progress_buf and, without
 * getup, terminate_buf may be NULL) and, with getup, recovery_counter[e] (int32 [n_envs]) = recovery_steps for recovery and
 * fall rows, else 0.
 * The plan export (nullable, all five or none; int32 [n_envs], motion_times_out f32 [n_envs]): EVERY element is written -
 * env_ids_out[e] = e for a reset row and -1 otherwise, the other four the row's decision (0 where it has none, and for rows
 * that are not reset).  It is a valid plan of ase_hip_amp_reset and an id list for ase_hip_task_reset / ase_hip_latent_renew,
 * which skip -1.
 * advance != 0: the offset moves on by one behind the launch, also when no row was due (a call is one stream position).
 * Refused: NULL reset_buf / rng_state; a state_init or a fall_init_prob > 0 that needs the table without it, or with n_tab <
 * n_envs (n_tab <= n_envs for falls); ASE_INIT_START / _RANDOM / _HYBRID without the clip tensors or cdf; getup without
 * terminate_buf or recovery_counter; a partial plan export; probabilities outside [0, 1]; the limits of ase_hip_amp_reset.
 * Replaces: HumanoidAMP._reset_envs' draws and _reset_env_tensors (env/tasks/humanoid_amp.py:132-201, humanoid.py:165-167),
 *   HumanoidAMPGetup._reset_actors / _reset_recovery_episode / _reset_fall_episode (env/tasks/humanoid_amp_getup.py:78-114). */
enum { ASE_INIT_DEFAULT = 0, ASE_INIT_START = 1, ASE_INIT_RANDOM = 2, ASE_INIT_HYBRID = 3 };
int ase_hip_amp_reset_due(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                          const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames, const float* dt,
                          const int32_t* length_starts, const int32_t* dof_body_ids, const int32_t* dof_offsets, int n_joints,
                          const int32_t* key_body_ids, int n_key, const uint32_t* cdf, int n_clips,
                          const float* tab_root_states, const float* tab_dof_pos, const float* tab_dof_vel, int n_tab,
                          int state_init, double hybrid_init_prob, int getup, double recovery_episode_prob,
                          double fall_init_prob, int recovery_steps, uint64_t* rng_state, int advance, int64_t* progress_buf,
                          int64_t* reset_buf, int64_t* terminate_buf, int32_t* recovery_counter, int32_t* env_ids_out,
                          int32_t* kind_out, int32_t* motion_ids_out, float* motion_times_out, int32_t* src_rows_out,
                          float* root_states, int64_t ld_root, float* dof_pos, float* dof_vel, int64_t ld_dof, int dof_stride,
                          const float* body_pos, const float* body_rot, const float* body_vel, const float* body_ang_vel,
                          int n_envs, int local_root_obs, int root_height_obs, float env_dt, float* hist, int n_steps,
                          void* stream);

/* The demo fetch (an addition to ABI 9, nothing else changed): n demo observations of n_steps frames each,
 * drawn, sampled, built and stored into the demo ring by ONE launch over the (sample i, slot k) items, no intermediate tensor.
 * Clip tensors, HOST index arrays and the frame layout F = 13 + 6 n_joints + D + 3 n_key as in ase_hip_motion_state /
 * ase_hip_build_amp_obs; lengths / num_frames / dt / length_starts have n_clips entries.  Up to 78 key bodies (F <= 255).
 * Where sample i's clip m and time t0 come from - exactly one pair is non-NULL:
 *   motion_ids (DEVICE int32 [n]), motion_times0 (f32 [n]): passed in, read when the launch runs.  A motion_ids[i] outside
 *             [0, n_clips) leaves sample i's row unwritten and is never dereferenced.
 *   rng_state (u64[2] = {seed, offset} on the device, as in ase_hip_amp_reset_due), cdf (DEVICE uint32 [n_clips], the table of
 *             ase_hip_amp_reset_due): draw j of sample i comes from element 2 i + j of the stream ("uniform": the 24-bit uniform
 *             (c[2] >> 8) * 2^-24 of the element, f32):
 *               j = 0  v = c[2] >> 8  the 24-bit integer behind the uniform: m is the first clip with v < cdf[m]
 *               j = 1  uniform u      t0 = u * (lengths[m] - truncate_time) + truncate_time, three f32 operations each rounded
 *                                     on its own (MotionLib.sample_time(truncate_time) + truncate_time; a clip shorter than
 *                                     truncate_time gives t0 in (length, truncate_time], as the reference does)
 *             advance != 0: the offset moves on by one behind the launch (a call is one stream position).
 * motion_ids_out / motion_times0_out (nullable, both or none; int32 / f32 [n]) receive every sample's (m, t0), in both modes.
 * Slot k of sample i is the frame of clip m at the f32 time t0 + (-step_dt) * (float)k (product and sum rounded on their own),
 * used UNCLAMPED as ase_hip_amp_reset does: what build_amp_obs_demo's motion_times0.unsqueeze(-1) + (-dt * arange(n_steps)),
 * ase_hip_motion_state and ase_hip_build_amp_obs compute, bit for bit - the same device functions.
 * Sample i goes to row (head + i) % ring_rows of out (f32 [ring_rows, ld_out], ld_out >= n_steps * F), slot k at columns
 * [k F, (k + 1) F); columns behind n_steps * F and all other rows are not written.  ring_rows = n, head = 0: a plain
 * [n, n_steps F] output.  head_dev (nullable, DEVICE int32 [1]): read when the launch runs and added to head, so that a
 * recorded launch follows a ring head kept on the device; a value outside [0, ring_rows) leaves every row unwritten.
 * Refused: a NULL operand of the mode; both modes or neither; half an export; n < 1; n_steps outside [1, 64]; n > ring_rows;
 * head outside [0, ring_rows); ld_out < n_steps * F; n_joints outside [1, 32]; a joint of other than 1 or 3 dofs;
 * dof_offsets[0] != 0; key / dof body ids outside [0, n_bodies); F > 255; n_clips < 1; a tile beyond 64 KB (n_steps > 32 of a
 * wide frame).
 * Replaces: HumanoidAMP.fetch_amp_obs_demo / build_amp_obs_demo (env/tasks/humanoid_amp.py:63-105), MotionLib.sample_motions /
 *   sample_time (utils/motion_lib.py:100-119) and the store into the demo ring (learning/amp_agent.py:498-533). */
int ase_hip_amp_demo_fetch(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                           const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames, const float* dt,
                           const int32_t* length_starts, int n_clips, const int32_t* dof_body_ids, const int32_t* dof_offsets,
                           int n_joints, const int32_t* key_body_ids, int n_key, const int32_t* motion_ids,
                           const float* motion_times0, uint64_t* rng_state, const uint32_t* cdf, int advance,
                           int32_t* motion_ids_out, float* motion_times0_out, int n, int n_steps, float truncate_time,
                           float step_dt, int local_root_obs, int root_height_obs, float* out, int64_t ld_out, int ring_rows,
                           int head, const int32_t* head_dev, void* stream);

/* Motion-clip loader: the frame arrays of ase_hip_motion_state / ase_hip_amp_reset from the raw contents of
 * SkeletonMotion clip files, every frame of every clip in ONE launch.  Inputs (DEVICE, all clips concatenated along the
 * frame axis, n_frames rows): rotation [n_frames, n_bodies, 4] f64, the stored LOCAL rotations xyzw; root_translation,
 * root_velocity, root_angular_velocity [n_frames, 3] f64 (body 0 of the stored global velocities); local_translation
 * [n_clips, n_bodies, 3] f32, each clip's skeleton offsets; per clip clip_first (its first row), clip_num_frames (>= 2),
 * clip_fps (f64); frame_clip [n_frames]: the clip of a row.  parent_indices [n_bodies], dof_body_ids [n_joints],
 * dof_offsets [n_joints + 1]: HOST int32 arrays; body 0 is a root, a parent precedes its child, a joint has 1 or 3 dofs.
 * Outputs (f32): gts [n_frames, n_bodies, 3], grs / lrs [n_frames, n_bodies, 4], grvs / gravs [n_frames, 3], dvs
 * [n_frames, D = dof_offsets[n_joints]].
 * Arithmetic: f64, operation by operation as poselib, rounded to f32 at the store.  grs / gts: a root's transform is its
 * local one (stored rotation; body 0's translation is root_translation rounded to f32 first, as poselib's f32
 * local_translation tensor does), a child's is transform_mul(global[parent], local[child]) with the rotation
 * re-normalised (sign flipped when w < 0, divided by max(norm, 1e-9)).  dvs: for frame f < F - 1 of a clip,
 * d = quat_mul_norm(conj(l[f]), l[f + 1]), angle = acos(clamp(2 d.w^2 - 1)), velocity = d.xyz / max(|d.xyz|, 1e-9) *
 * angle / (1.0 / fps); a 3-dof joint takes the vector, a 1-dof joint its y component; the last frame repeats the one
 * before; frames of different clips never pair.  lrs, grvs, gravs: the stored values cast.  Rows whose frame_clip lies
 * outside [0, n_clips) are skipped; n_bodies, n_joints <= 32.
 * Replaces: MotionLib._load_motions / _compute_motion_dof_vels / _local_rotation_to_dof_vel and the concatenation of
 *   MotionLib.__init__ (utils/motion_lib.py:75-80,174-236,279-294,326-355); SkeletonState.global_transformation /
 *   local_translation (poselib/skeleton/skeleton3d.py:403-424,495-510); quat_mul, quat_normalize, quat_rotate,
 *   quat_angle_axis, transform_mul (poselib/core/rotation3d.py:8-49,88-93,201-206,226-235,318-327). */
int ase_hip_clip_frames(const double* rotation, const double* root_translation, const double* root_velocity,
                        const double* root_angular_velocity, const float* local_translation,
                        const int32_t* parent_indices, int n_bodies, const int32_t* clip_first,
                        const int32_t* clip_num_frames, const double* clip_fps, const int32_t* frame_clip, int n_clips,
                        int n_frames, const int32_t* dof_body_ids, const int32_t* dof_offsets, int n_joints, float* gts,
                        float* grs, float* lrs, float* grvs, float* gravs, float* dvs, void* stream);

/* Motion retargeting: a mocap clip on its own skeleton -> a SkeletonMotion on the target skeleton, all frames
 * of all clips of a call in SEVEN launches (six without the hinge stage), whatever the number of clips and frames, with no
 * host read in between.  Arithmetic: f64, operation by operation as poselib; every buffer between two launches is f64 on the
 * device; the four outputs of a clip file are rounded to f32 once, at their store.  Clips are concatenated along the frame
 * axis with the loader's tables (clip_first, clip_num_frames, clip_fps [n_clips], frame_clip [n_frames], DEVICE); no stencil,
 * pairing or reduction crosses a clip boundary.  TRIMMING is table arithmetic: output row t of clip c, frame f = t -
 * clip_first[c], reads source row src_first[c] + f (src_first already holds the clip's first kept frame).
 * All skeleton tables are DEVICE int32 arrays (a source skeleton has up to 64 bodies).  A TREE table is [n, tree_ld]: column 0
 * the depth of node b, columns 1 .. depth + 1 its chain from the root down to b itself; tree_ld <= 65.  The entries cannot
 * read them, so the caller (ase_amd.retarget.Retargeter) checks that a parent precedes its child and that the reduced trees
 * of a mapping have equal sizes; the kernels range-check every index they read from a table and an item whose tables do not
 * describe it writes nothing.  Refused here: null operands, body counts outside 1-64, frames x bodies >= 2^31, clip counts
 * that do not fit the frames, and (ase_hip_retarget_velocity) fewer than 2 frames per clip.
 * params (DEVICE f64 [12]): the rotation to the target skeleton xyzw [0..3], the source T-pose's root translation [4..6], the
 * target T-pose's [7..9], the scale [10], the root height offset [11].
 *
 * ase_hip_retarget_fk: global rotations of a tree, out [n_frames, n_bodies, 4].  mode 0: rotation holds local rotations,
 *   forward kinematics (a root's is its own, a child's quat_mul_norm(global[parent], local[child])); 1: rotation holds
 *   global rotations, copied as stored (SkeletonState._transfer_to of an is_local == False clip); 2: global rotations
 *   taken to local form first (quat_mul_norm(inverse(global[parent]), global[child])), then mode 0 - a T-pose stored in
 *   global form.  A T-pose is a one-frame call.
 * ase_hip_retarget_chain: src_global [n_frames, n_src_bodies, 4] -> out [n_frames, n_mapped, 4], the global rotations on the
 *   REDUCED TARGET tree: reduced-target node k takes the rotation of reduced-source node m = rt_src[k] (source body
 *   rs_body[m]) local to its reduced-source parent rs_parent[m] (-1: none), node 0 is pre-multiplied by params[0..3]
 *   (quat_mul_norm), and the locals are recomposed along rt_tree.  Where the two reduced trees differ in topology this is
 *   not the source's global rotation (SkeletonState._transfer_to, _remapped_to, STEP 2 of retarget_to).
 * ase_hip_retarget_pose: per frame and target body b, g(b) = quat_mul_norm(quat_mul_norm(state_global[i], inverse(
 *   tpose_global[i])), target_global[rt_body[i]]) with i = ancestor[b], the reduced-target node of b or of its nearest mapped
 *   ancestor; local_rotation[b] = g(b) for a root, quat_mul_norm(inverse(g(parent)), g(b)) otherwise.  root_out = params[7..9]
 *   + (rotate(R, root_translation[src row]) - rotate(R, params[4..6])) * scale.  tpose_global [n_mapped, 4]: the source
 *   T-pose through ase_hip_retarget_fk and _chain; target_global [n_bodies, 4]: the target T-pose through _fk.
 * ase_hip_retarget_hinge: project_joints from a table, roles [n_bodies, 6] = (role, upper, lower, end, bend sign, twist
 *   sense): role 0 copies the body, 1 sets it to identity, 3 (lower body of a limb) stores the bend about y by
 *   sign * |theta|, theta the angle at `lower` between the global positions of `upper` and `end`; 2 (upper body) stores
 *   quat_mul(local[upper], twist) with the twist about the offset of `end` that takes the bent direction to the unprojected
 *   one, positive where dir0.y <= 0 (sense -1, arms) or dir0.y >= 0 (sense +1, legs).  All limbs read the unprojected input.
 * ase_hip_retarget_ground: min_z [n_clips], the minimum of global z over all frames and bodies of a clip; one block per clip,
 *   a fixed comparison order, no atomics; a NaN wins.
 * ase_hip_retarget_finish: root z + -min_z[clip] + params[11]; global_rotation / global_translation (f64) of the grounded
 *   motion by forward kinematics on the target tree; rotation_out [n_frames, n_bodies, 4], root_out [n_frames, 3]: f32.
 * ase_hip_retarget_velocity: velocity = gaussian(numpy.gradient(global_translation)) / (1.0 / fps) (central differences,
 *   one-sided at a clip's ends); angular_velocity = gaussian(axis * angle / (1.0 / fps)) of quat_mul_norm(r[f + 1],
 *   inverse(r[f])), zero at a clip's last frame (angle: acos(clamp(2 w^2 - 1)), axis / max(norm, 1e-9)).  gaussian: 17 taps,
 *   sigma 2, indices clamped to the clip, added in the order of scipy's symmetric correlation (centre, then the pairs from
 *   the outermost in).  Both f32 [n_frames, n_bodies, 3].
 * Replaces: SkeletonState.retarget_to / _transfer_to / _remapped_to / local_rotation, SkeletonMotion.retarget_to_by_tpose,
 *   from_skeleton_state, _compute_velocity, _compute_angular_velocity (poselib/skeleton/skeleton3d.py:462-482,706-713,757-784,
 *   786-948,1090-1120,1223-1246,1345-1390); project_joints and main of poselib/retarget_motion.py:24-175,211-243. */
int ase_hip_retarget_fk(const double* rotation, int mode, const int32_t* tree, int tree_ld, int n_bodies,
                        const int32_t* clip_first, const int32_t* clip_num_frames, const int32_t* src_first,
                        const int32_t* frame_clip, int n_clips, int n_frames, int n_src_frames, double* out, void* stream);
int ase_hip_retarget_chain(const double* src_global, int n_src_bodies, const int32_t* rs_body, const int32_t* rs_parent,
                           const int32_t* rt_src, const int32_t* rt_tree, int tree_ld, int n_mapped, const double* params,
                           int n_frames, double* out, void* stream);
int ase_hip_retarget_pose(const double* state_global, const double* tpose_global, const double* target_global,
                          const double* root_translation, const double* params, const int32_t* rt_body,
                          const int32_t* ancestor, const int32_t* parent_indices, int n_mapped, int n_bodies,
                          const int32_t* clip_first, const int32_t* clip_num_frames, const int32_t* src_first,
                          const int32_t* frame_clip, int n_clips, int n_frames, int n_src_frames, double* local_rotation,
                          double* root_out, void* stream);
int ase_hip_retarget_hinge(const double* local_rotation, const double* root_translation, const float* local_translation,
                           const int32_t* tree, int tree_ld, const int32_t* roles, int n_bodies, int n_frames, double* out,
                           void* stream);
int ase_hip_retarget_ground(const double* local_rotation, const double* root_translation, const float* local_translation,
                            const int32_t* tree, int tree_ld, int n_bodies, const int32_t* clip_first,
                            const int32_t* clip_num_frames, int n_clips, int n_frames, double* min_z, void* stream);
int ase_hip_retarget_finish(const double* local_rotation, const double* root_translation, const double* min_z,
                            const double* params, const float* local_translation, const int32_t* tree, int tree_ld,
                            int n_bodies, const int32_t* frame_clip, int n_clips, int n_frames, double* global_rotation,
                            double* global_translation, float* rotation_out, float* root_out, void* stream);
int ase_hip_retarget_velocity(const double* global_rotation, const double* global_translation, int n_bodies,
                              const int32_t* clip_first, const int32_t* clip_num_frames, const double* clip_fps,
                              const int32_t* frame_clip, int n_clips, int n_frames, float* velocity, float* angular_velocity,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Launch programs: record a sequence of the calls above ONCE (nothing is launched while recording), replay it with 4-5 us
 * of host work per launch on the same HIP streams - the optimisation step as one call, with OUR branch -> stream mapping
 * (a captured hipGraph picks its own; eager launches from Python fall behind the GPU).  Recording is per thread.
 * ase_hip_mark / ase_hip_wait are the fork / join points between streams (event record / stream-wait-event); outside a
 * recording they act immediately on a pool of events.  ase_hip_memset / ase_hip_memcpy: recordable fills / device copies.
 * ------------------------------------------------------------------------------------------- */
int ase_hip_prog_create(void** prog);
int ase_hip_prog_destroy(void* prog);
int ase_hip_prog_begin(void* prog);
int ase_hip_prog_end(void* prog);
int ase_hip_prog_size(void* prog);          /* entries recorded (launches + fork / join points); < 0: null program */
int ase_hip_prog_launch(void* prog);
/* A HOST callback at this position of the sequence: called immediately outside a recording, on every replay inside one.
 * This is how the exchange points of the data-parallel update (the RCCL all-reduce of a branch's gradient bucket, issued while
 * the other branches' backward launches are still being replayed - learning/common_agent.py:94-107, the Horovod optimizer's
 * gradient hooks) live inside ONE launch program; fn runs on the replaying thread and must enqueue its work on a stream
 * itself. */
int ase_hip_prog_host(void (*fn)(void*), void* arg);
int ase_hip_mark(void* stream, int* id);
int ase_hip_wait(void* stream, int id);
int ase_hip_memset(void* dst, int value, int64_t bytes, void* stream);
int ase_hip_memcpy(void* dst, const void* src, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASE_HIP_H */
