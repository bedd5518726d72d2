/* kalle_hip.h - C-ABI of libkalle_hip.so: the MI355X (gfx950) kernels behind the kalle-audio DiT /
 * audio-VAE hot path.
 *
 * The reference (18281818221/kalle-audio) has no FFI/operator interface for this path: its seam is
 * Python nn.Module classes that call torch ops.  Each entry point below therefore
 * names the reference call site (file:line under /root/reference) whose torch op it replaces; the
 * Python drop-in modules in kalle_audio_amd/stable_audio_tools bind these with ctypes
 * (INTEGRATION.md shows the binding a maintainer would add on the reference side).
 *
 * Conventions: plain device pointers + sizes, `stream` is a hipStream_t passed as void*, every call
 * is asynchronous on that stream, allocates nothing, and returns 0 on success or a negative KALLE_ERR_* code (never
 * throws).  Process state the library does keep: per-thread caches of GEMM split plans (pure functions of the shape), the
 * calling thread's last plan / last HIP error name (kalle_gemm_last_plan, kalle_gemm_wgrad_group_last_plan, kalle_conv_last_plan, kalle_attn_last_plan, kalle_last_error), a per-kernel per-device flag for
 * the dynamic-LDS attribute.  The library reads no environment variables.  bf16 tensors are raw uint16 storage.
 */
#ifndef KALLE_HIP_H
#define KALLE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KALLE_BF16 0
#define KALLE_F32 1

/* library / device info: returns the ABI version; fills the gfx arch name the code objects target */
int kalle_abi_version(void);
const char* kalle_target_arch(void);
/* name of the HIP error behind the calling thread's most recent KALLE_ERR_LAUNCH ("" if none) */
const char* kalle_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM (bf16 MFMA, fp32 accumulate) with fused epilogue.
 *   C[M,N] = alpha * op(A) @ op(B)  (+bias[n]) (* sigmoid(1-gate[m/rows_per_batch, n])) (+residual[m,n]) (+C)
 *   a_kmajor=0: A stored [M][K] (lda)   | a_kmajor=1: A stored [K][M] (lda)
 *   b_kmajor=0: B stored [N][K] (ldb)   | b_kmajor=1: B stored [K][N] (ldb)
 * forward  y = x @ W^T            : a_kmajor=0, b_kmajor=0  (nn.Linear: transformer.py:216,252,411,414,419,541,774,807)
 * dgrad    dx = dy @ W            : a_kmajor=0, b_kmajor=1
 * wgrad    dW = dy^T @ x          : a_kmajor=1, b_kmajor=1
 * c_dtype: KALLE_BF16 or KALLE_F32.  N, K (and M when a_kmajor) must be multiples of 8; pointers 16-B aligned.
 */
typedef struct kalle_gemm_epilogue {
    const float* bias;      /* [N] fp32 or NULL                                   (transformer.py:207,252 Linear bias) */
    const float* gate;      /* [rows/rows_per_batch][ldg] fp32 or NULL: adaLN gate (transformer.py:667,681)            */
    int64_t ldg;
    int32_t rows_per_batch;
    const float* residual;  /* [M][ldr] fp32 or NULL: residual stream add          (transformer.py:668,682,685-693)    */
    int64_t ldr;
    int32_t accumulate;     /* C += result (fp32 C only): gradient accumulation                                        */
    float alpha;            /* 0 is read as 1                                                                          */
    /* optional output-row remap (0 = off): logical row m is stored at row
     *   (m / c_rows_per_batch) * c_batch_rows + c_row_offset + m % c_rows_per_batch   of C (and of residual):
     * lets project_in write straight behind the prepended tokens of the residual stream (transformer.py:774-781) */
    int32_t c_rows_per_batch;
    int32_t c_batch_rows;
    int32_t c_row_offset;
    const uint8_t* row_mask; /* [M] or NULL: rows with 0 contribute 0 before the residual add
                              * (Attention zeroes padded query rows after to_out, transformer.py:543-545) */
    /* fused SwiGLU (transformer.py:216-219), bf16 C; in the 256x256 kernel (glu_inner % 128 == 0) and, forward only, in the
     * small-tile kernels of the few-row path (M <= 2048, glu_inner % 32 == 0); KALLE_ERR_UNSUPPORTED otherwise - the caller
     * then runs the GEMM and kalle_swiglu_* separately:
     *   glu_mode 1 (forward,  a_kmajor=0,b_kmajor=0, N = 2*glu_inner): C = h = x W^T + b  [M][2*inner]  AND
     *              glu_aux = act [M][inner] bf16 = h[:, j] * silu(h[:, inner + j])
     *   glu_mode 2 (backward, a_kmajor=0,b_kmajor=1, N = glu_inner):   acc = d(act); glu_aux = h [M][2*inner] bf16;
     *              C = dh [M][2*inner] bf16; glu_dbias (fp32 [2*inner], optional) += column sums of dh
     * The fused epilogues take no other field: glu_mode 1 with alpha != 1, a gate, residual, row_mask, output-row remap or
     * accumulate, and glu_mode 2 with a bias or any of those (alpha is applied to d(act) first), return KALLE_ERR_UNSUPPORTED
     * before any kernel runs. */
    int32_t glu_mode;
    int32_t glu_inner;
    void* glu_aux;
    float* glu_dbias;
    /* optional scratch for the few-rows paths (sampling at generation batch sizes, small training batches): with
     * workspace_bytes >= 8 * M * N the dispatcher may cut K into up to workspace_bytes / (4 M N) slices, each writing its
     * partial result as an fp32 [M][N] slab, and sum the slabs in a fixed order + apply the epilogue in a finishing pass
     * (bitwise reproducible).  Used for long K only: with M <= 2048 rows and N % 64 == 0 (N % 128 for a k-major B) the
     * dispatcher first cuts the OUTPUT into 64 x 64 ... 128 x 128 tiles over the whole K (two wave groups per tile, epilogue in
     * the same launch, no scratch), and takes K slices only beyond ~2048 deep.  The library never allocates: no workspace, no
     * sliced path.  Contents are undefined afterwards; one workspace per stream. */
    void* workspace;
    int64_t workspace_bytes;
} kalle_gemm_epilogue;

int kalle_gemm_bf16(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor,
                    void* C, int64_t ldc, int c_dtype, int M, int N, int K,
                    const kalle_gemm_epilogue* ep, void* stream);

/* which kernel the calling thread's most recent kalle_gemm_bf16 launched (unchanged by a call that returned an error before
 * launching): low byte = family: 1 = gemm_bf16_kernel (128x128, register-staged, any shape), 2 = gemm2_kernel (256x128, LDS-DMA
 * 3-stage ring, K % 8 == 0), 3 = gemm3_kernel (256x256, 2 stages), 4 = few-rows K slices (gemm2_kernel into slabs + finishing
 * pass), 5 = small tiles with two wave groups (gemm2_ks2_kernel).  For 2 and 3 bits 8-23 = split-K factor (atomic adds into C
 * when > 1) and bit 24 = mixed split-K (3 only: some tiles are cut into one K slice fewer than bits 8-23 say); 1 reports no
 * factor (0) and 4 always 1 (its slab count is not reported); for 5 bits 8-11 / 12-15 = tile rows / columns in units of 64,
 * bits 16.. = K slices (more than one: slabs + finishing pass).
 * kalle_gemm_plan is the same planner as a pure host query: the arguments of kalle_gemm_bf16 without `stream` (pointers are
 * tested for null and alignment only, never read), the same argument checks and return codes; on success *plan is the word
 * that kalle_gemm_bf16 would leave now on this thread, otherwise *plan is left alone.  It launches nothing, needs no device,
 * does not change kalle_gemm_last_plan and leaves the thread's cache of mixed split-K plans as it found it (kalle_gemm_bf16
 * enters the plans it finds: a weight gradient's plan then serves every K of its 1024-deep bucket on that thread). */
int kalle_gemm_last_plan(void);
int kalle_gemm_plan(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor,
                    void* C, int64_t ldc, int c_dtype, int M, int N, int K,
                    const kalle_gemm_epilogue* ep, int* plan);

/* diagnostics (tools/gemm_stamps.py), never set by the product path: with a non-NULL device buffer of
 * [workgroups][2][8] uint64 the 256x256 kernel's wave 0 / wave 7 leave s_memrealtime stamps (100 MHz) at: 0 entry, 1 first
 * K-tile landed, 2 main loop done, 3 epilogue barrier passed, 4 stores issued, 5 stores acknowledged (an extra wait that only
 * exists while the buffer is set).  NULL switches it off again.  Process-wide. */
int kalle_gemm_debug_stamps(void* buf);
/* the same for the attention kernels (tools/attn_stamps.py): [B * H workgroups][8] stamps of thread 0 - forward: 0 entry, 1 tiles
 * staged, 2 computed, 3 stores issued, 4 stores acknowledged; fused self-attention backward: 0 entry, 1 tiles staged, 2 row
 * statistics ready, 3 dK / dV computed, 4 dK / dV stored, 5 dQ computed, 6 stores issued, 7 acknowledged */
int kalle_attn_debug_stamps(void* buf);
/* diagnostics (tools/cu_hold_probe.py), never called by the product path: `nwg` workgroups of 256 threads with `lds_bytes` of LDS
 * each (<= 64 KiB) that do nothing but stay resident for `microseconds` - a stand-in for a communication kernel that holds some
 * CUs while the GEMMs of the backward pass launch (a 160-KiB-LDS GEMM workgroup cannot share a CU with it) */
int kalle_debug_hold_cus(int nwg, int lds_bytes, int microseconds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (bias-less gamma, eps 1e-5) with optional adaLN modulation - one wavefront per row.
 *   y = ((x-mean)*rstd*gamma + beta) * (1 + scale[b]) + shift[b]        (transformer.py:173-192, 660-665, 677-679)
 * x: [rows][D] fp32 (residual stream) or bf16; y: bf16; mean/rstd: [rows] fp32 saved for backward.
 * beta, scale, shift may be NULL.  D % 8 == 0, D <= 4096.
 */
int kalle_layernorm_fwd(const void* x, int x_dtype, const float* gamma, const float* beta,
                        const float* scale, const float* shift, int64_t ld_mod, int rows_per_batch,
                        void* y, float* mean, float* rstd, int rows, int D, float eps, void* stream);

/* backward of the above w.r.t. x and gamma/beta.
 *   dx_out = dres + dLN/dx(dy)   (dres: incoming residual-stream gradient fp32 or NULL; may alias dx_out)
 *   dx_bf16 (optional): the same values rounded to bf16 - the operand of the next dgrad/wgrad GEMMs, saving a cast pass
 *   dgamma_part/dbeta_part: [nparts][D] fp32 partial sums (nparts = value returned by
 *   kalle_layernorm_bwd_parts(rows)); reduce with kalle_colsum_f32.
 */
int kalle_layernorm_bwd_parts(int rows);
int kalle_layernorm_bwd(const void* dy, const void* x, int x_dtype, const float* gamma,
                        const float* scale, int64_t ld_mod, int rows_per_batch,
                        const float* mean, const float* rstd, const float* dres, float* dx_out, void* dx_bf16,
                        float* dgamma_part, float* dbeta_part, int rows, int D, void* stream);

/* same, with the parameter gradients added ATOMICALLY into [D] accumulators (dgamma_acc, dbeta_acc or NULL) that the
 * caller has initialised - the trainer's flat gradient: no partial rows, no reduction launch */
int kalle_layernorm_bwd_acc(const void* dy, const void* x, int x_dtype, const float* gamma,
                            const float* scale, int64_t ld_mod, int rows_per_batch,
                            const float* mean, const float* rstd, const float* dres, float* dx_out, void* dx_bf16,
                            float* dgamma_acc, float* dbeta_acc, int rows, int D, void* stream);

/* the _acc form with the COLUMN SUMS of the bf16-rounded dx added atomically into dx_colsum_acc [D] (fp32) in place of dbeta:
 * dx of a block's pre_norm is the output gradient of the block below, whose FF-out bias gradient (transformer.py:252,
 * nn.Linear(inner, dim) with bias) is exactly that sum - fused here it saves a pass over the [rows][D] bf16 gradient */
int kalle_layernorm_bwd_colsum(const void* dy, const void* x, int x_dtype, const float* gamma,
                               const float* scale, int64_t ld_mod, int rows_per_batch,
                               const float* mean, const float* rstd, const float* dres, float* dx_out, void* dx_bf16,
                               float* dgamma_acc, float* dx_colsum_acc, int rows, int D, void* stream);

/* adaLN modulation gradients: dscale[b,d] = sum_t dy*ln, dshift[b,d] = sum_t dy   (transformer.py:665,679) */
int kalle_adaln_mod_bwd(const void* dy, const void* x, int x_dtype, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* dscale, float* dshift, int64_t ld_mod,
                        int nbatch, int rows_per_batch, int D, void* stream);

/* RMSNorm  y = x * scale * rsqrt(mean(x^2)+eps)   (blocks.py:268-272, 285-299; AdaRMSNorm 211-221 via scale=[b]) */
int kalle_rmsnorm_fwd(const void* x, int x_dtype, const float* scale, int64_t ld_scale, int rows_per_batch,
                      void* y, int y_dtype, float* rrms, int rows, int D, float eps, void* stream);
/* dx = RMSNorm backward (+ dres, the residual-stream gradient, when given); dx_bf16: optional bf16 copy of dx for the
 * next GEMM (the Llama decoder layers under model_sigmaVAE.py:78-81: input_layernorm / post_attention_layernorm) */
int kalle_rmsnorm_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* scale, int64_t ld_scale,
                      int rows_per_batch, const float* rrms, float* dx, float* dscale_part, const float* dres,
                      void* dx_bf16, int rows, int D, void* stream);

/* same, with dscale added ATOMICALLY into the caller-initialised [D] accumulator dscale_acc (the trainer's flat gradient) */
int kalle_rmsnorm_bwd_acc(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* scale, int64_t ld_scale,
                          int rows_per_batch, const float* rrms, float* dx, float* dscale_acc, const float* dres,
                          void* dx_bf16, int rows, int D, void* stream);

/* Attention(qk_norm=...) (transformer.py:303-307, 422-428): every 64-wide head of q / k is normalised before the rotary
 * embedding (any head width dh in {32, 64, 128}: the _hd forms below).
 * mode 1 "l2": F.normalize = x / max(||x||_2, 1e-12);  mode 2 "ln": LayerNorm(64, eps 1e-6), gamma / beta fp32 [64].
 * x, y: bf16 row-major with leading dimensions ldx / ldy and element offsets (the q or k slice of a projection output, as in
 * kalle_attention_fwd; all multiples of 8); `heads` consecutive heads per row.  stat: fp32 [rows][heads][2], written by the
 * forward (mean | clamp flag, reciprocal std | reciprocal norm) and read by the backward.
 * Backward: g = gradient w.r.t. the normalised values (bf16, as kalle_attention_bwd leaves it), dx may alias g; mode 2 ADDS the
 * column sums into dgamma / dbeta (fp32 [64], atomics; either may be NULL, independently of the other).  mode 1 with
 * ||x|| <= 1e-12 (an all-zero head of a padded token): the clamp is active, y = x * 1e12 (= 0) and dx = g * 1e12, which is what
 * autograd gives for F.normalize. */
int kalle_head_norm_fwd(const void* x, int64_t ldx, int64_t x_off, void* y, int64_t ldy, int64_t y_off, float* stat,
                        const float* gamma, const float* beta, int mode, int64_t rows, int heads, void* stream);
int kalle_head_norm_bwd(const void* x, int64_t ldx, int64_t x_off, const float* stat, const void* g, int64_t ldg,
                        int64_t g_off, void* dx, int64_t lddx, int64_t dx_off, const float* gamma, float* dgamma,
                        float* dbeta, int mode, int64_t rows, int heads, void* stream);
/* the same for heads of width head_dim in {32, 64, 128} (Attention(dim_heads = head_dim, qk_norm=...), transformer.py:303-307:
 * LayerNorm(dim_heads)): head h of a row at column h * head_dim, "ln" statistics over head_dim values, gamma / beta / dgamma /
 * dbeta fp32 [head_dim]; ld* >= heads * head_dim.  Any other head_dim: KALLE_ERR_ARG.  head_dim 64 is exactly
 * kalle_head_norm_fwd / _bwd (which forward here). */
int kalle_head_norm_fwd_hd(const void* x, int64_t ldx, int64_t x_off, void* y, int64_t ldy, int64_t y_off, float* stat,
                           const float* gamma, const float* beta, int mode, int64_t rows, int heads, int head_dim, void* stream);
int kalle_head_norm_bwd_hd(const void* x, int64_t ldx, int64_t x_off, const float* stat, const void* g, int64_t ldg,
                           int64_t g_off, void* dx, int64_t lddx, int64_t dx_off, const float* gamma, float* dgamma,
                           float* dbeta, int mode, int64_t rows, int heads, int head_dim, void* stream);

/* column sums: out[c] (+)= sum_r in[r][c]; in fp32 or bf16 [rows][ld]. Used for bias grads and partial reduces. */
int kalle_colsum(const void* in, int in_dtype, int64_t ld, float* out, int rows, int cols, int accumulate,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise / reductions on the DiT path
 */
/* SwiGLU: out[m, j] = h[m, j] * silu(h[m, inner + j])                     (transformer.py:218-219) */
int kalle_swiglu_fwd(const void* h, void* out, int64_t rows, int inner, void* stream);
/* dh[m, j] = dout*silu(g), dh[m, inner+j] = dout*x*silu'(g);  dbias (optional, fp32 [2*inner]) += column sums of dh
 * (the GLU projection's bias gradient, fused so dh is not re-read; atomically accumulated - zero it for a fresh sum) */
int kalle_swiglu_bwd(const void* dout, const void* h, void* dh, float* dbias, int64_t rows, int inner, void* stream);
/* SiLU on fp32/bf16 vectors (to_cond_embed / to_global_embed / to_scale_shift_gate: dit.py:39-72, transformer.py:641-644) */
int kalle_silu_fwd(const void* x, void* y, int dtype, int64_t n, void* stream);
int kalle_silu_bwd(const void* dy, const void* x, void* dx, int dtype, int64_t n, void* stream);

/* forward noising + target (training/diffusion.py:365-379, inference/sampling.py:8-11)
 *   objective 0 ("v"): a=cos(pi t/2), s=sin(pi t/2); x_t = a x + s n ; target = a n - s x
 *   objective 1 ("rectified_flow"): a=1-t, s=t ;     x_t = a x + s n ; target = n - x
 * x, noise: fp32 [B][per_sample]; t fp32 [B]; x_t, target fp32.
 */
int kalle_diffuse_fwd(const float* x, const float* noise, const float* t, float* x_t, float* target,
                      int nbatch, int64_t per_sample, int objective, void* stream);

/* MSE loss (training/losses/losses.py:53-69): loss = mean((out-target)^2) over the masked elements,
 * dout = dloss * 2 (out-target)/count.  mask: uint8 [B][T] over the last dim (broadcast over C) or NULL.
 * out/target fp32 [B][C][T].  loss_sum[0] += sum of squares, loss_sum[1] += count (both must be zeroed by the caller);
 * call kalle_mse_finish to produce loss and scale dout.
 */
int kalle_mse_fwd(const float* out, const float* target, const uint8_t* mask, float* loss_acc, float* diff,
                  int nbatch, int C, int T, void* stream);
int kalle_mse_finish(float* loss_acc, float* loss, float* diff, int64_t n, float weight, void* stream);

/* batched 2-D transpose with dtype conversion (the "b c t -> b t c" rearranges of dit.py:199,219):
 *   out[b][c][r] = in[b][r][c] for r < R, c < Cn; element (b,r,c) of `in` at b*in_batch_stride + r*in_ld + c,
 *   element (b,c,r) of `out` at b*out_batch_stride + c*out_ld + r.  dtypes fp32 or bf16 independently. */
int kalle_transpose_2d(const void* in, int in_dtype, int64_t in_batch_stride, int64_t in_ld, void* out,
                       int out_dtype, int64_t out_batch_stride, int64_t out_ld, int nbatch, int R, int Cn,
                       void* stream);

/* strided row copy / cast / accumulate: out[b][r][0:cols] (+)= in[b][r][0:cols]  (cols, strides % 4 == 0).
 * Used to splice the prepended conditioning token into the residual stream (transformer.py:776-787) and to
 * gather token rows for GEMM operands. */
int kalle_copy_rows(const void* in, int in_dtype, int64_t in_batch_stride, int64_t in_ld, void* out,
                    int out_dtype, int64_t out_batch_stride, int64_t out_ld, int nbatch, int rows, int cols,
                    int accumulate, void* stream);

/* All weight gradients of a transformer block in ONE launch: dw_i [N_i][K_i] += dy_i^T x_i over `tokens` rows
 * (the autograd backward of the block's nn.Linear layers - transformer.py:216,252,411,414,419,541 - which the reference
 * leaves to torch, one GEMM each).  dy bf16 [tokens][N] (ld lddy), x bf16 [tokens][K] (ld ldx), dw fp32 [N][K] (ld lddw),
 * ACCUMULATED into (the trainer's gradient sink; zero it for a plain gradient).  N, K, lddy, ldx % 8 == 0, 16-byte aligned
 * pointers; tokens % 8 != 0 returns KALLE_ERR_UNSUPPORTED (launch the gradients one by one with kalle_gemm_bf16 then).
 * Most 256 x 256 output tiles run over all tokens (read-add-store), a tail is cut into token slices (atomic adds) so that
 * the last round of workgroups is full. */
#define KALLE_MAX_GROUP 8
typedef struct kalle_wgrad_problem {
    const void* dy;
    int64_t lddy;
    const void* x;
    int64_t ldx;
    float* dw;
    int64_t lddw;
    int32_t N, K, tokens;
} kalle_wgrad_problem;
/* overwrite != 0: dw_i = dy_i^T x_i instead (no clear needed: tiles that run whole store their result, the regions of the
 * tiles that are cut into token slices are cleared by a small launch first) */
int kalle_gemm_wgrad_group(const kalle_wgrad_problem* problems, int nprob, int overwrite, void* stream);
/* What the calling thread's most recent kalle_gemm_wgrad_group launched, as five ints (all 0 when that call returned before
 * launching anything):
 *   plan[0] tiles    256 x 256 output tiles of all problems: sum of ceil(N / 256) * ceil(K / 256)
 *   plan[1] whole    tiles that ran over all tokens in one workgroup (read-add-store, or a plain store under `overwrite`): the
 *                    first `whole` tiles in problem order; either all of them or a multiple of 256
 *   plan[2] slices   token slices (atomic adds) per remaining tile, 2 .. 12; 0 when no tile is sliced.  A slice is
 *                    ceil(ktiles / slices) 64-token K-tiles long, so the last one may be short and trailing ones empty
 *   plan[3] cleared  1 when the clearing launch ran first (`overwrite` with sliced tiles)
 *   plan[4] cached   1 when whole / slices were replayed from the thread's plan cache, which is keyed on every problem's
 *                    (N, K, tokens / 1024): a plan found at one token count serves the others of its 1024-token bucket, with
 *                    slices falling back to 0 (all tiles whole) where the shortest problem has fewer K-tiles than slices
 * kalle_gemm_wgrad_group_plan is the same planner as a pure host query: same arguments (the pointers are only checked, never
 * read), same return codes, `plan` filled as above for the launch that kalle_gemm_wgrad_group would make now on this thread;
 * it launches nothing, needs no device and leaves the plan cache as it found it. */
int kalle_gemm_wgrad_group_last_plan(int* plan);
int kalle_gemm_wgrad_group_plan(const kalle_wgrad_problem* problems, int nprob, int overwrite, int* plan);

/* Chunked VAE encode / decode (AudioAutoencoder.encode_audio / decode_audio, autoencoders.py:429-560) as a batched pipeline:
 * every chunk rides on the batch axis of ONE encoder / decoder pass; this call is the gather in front of it and the paste
 * of the trimmed chunk centres behind it.  For segment s < nseg (<= KALLE_MAX_SEGMENTS), batch item b, row (channel) c:
 *   dst[s*dst_seg_stride + b*dst_batch_stride + c*dst_ld + dst_off[s] + j] =
 *   src[s*src_seg_stride + b*src_batch_stride + c*src_ld + src_off[s] + j]          for j < len[s]
 * offsets / strides in elements; src_off / dst_off / len are HOST arrays (copied into the launch); destinations of
 * different segments must not overlap; src and dst have the same dtype (fp32 or bf16). */
#define KALLE_MAX_SEGMENTS 64
int kalle_segment_copy(const void* src, void* dst, int dtype, int nseg, const int64_t* src_off, const int64_t* dst_off,
                       const int* len, int nbatch, int rows, int64_t src_seg_stride, int64_t src_batch_stride,
                       int64_t src_ld, int64_t dst_seg_stride, int64_t dst_batch_stride, int64_t dst_ld, void* stream);

/* dtype conversion fp32 <-> bf16 (n elements, n % 8 == 0 not required) */
int kalle_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, void* stream);

/* residual-stream gradient -> bf16 GEMM operand, with the adaLN gate backward fused in:
 *   gb[b,t,n]   = bf16( g[b,t,n] * (gate ? sigmoid(1-gate[b,n]) : 1) * (row_mask ? row_mask[b*T+t] : 1) )
 *   dgate[b,n]  = -(1 - sigmoid(1-gate[b,n])) * sum_t g[b,t,n]*row_mask * (x_out[b,t,n] - x_in[b,t,n])     (gate != NULL)
 * (x_out = x_in + branch*sigmoid(1-gate), transformer.py:667-668,681-682; x_out/x_in/dgate unused when gate == NULL).
 * D % 4 == 0, ldg % 4 == 0, 16-byte aligned rows; dgate is cleared and then summed atomically over chunks of rows. */
int kalle_grad_cast(const float* g, const float* x_out, const float* x_in, const float* gate, int64_t ldg,
                    const uint8_t* row_mask, void* gb, float* dgate, int nbatch, int rows_per_batch, int D,
                    void* stream);

/* timestep Fourier features (blocks.py:84-93): out[b, j] = cos(2 pi t[b] w[j]), out[b, F/2+j] = sin(...) ; out bf16 or fp32 */
int kalle_fourier_features(const float* t, const float* w, void* out, int out_dtype, int nbatch, int half,
                           void* stream);

/* dw[j] = sum_b 2 pi t[b] * (dout[b, half+j] cos(f) - dout[b, j] sin(f)),  f = 2 pi t[b] w[j]   (dout fp32 [B][2*half]) */
int kalle_fourier_features_bwd(const float* dout, const float* t, const float* w, float* dw, int nbatch, int half,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention (optional causal mask, optional key mask), LDS-resident K/V tiles, bf16 MFMA, fp32 softmax.
 *   out[b, i, h*64+d] = softmax_j(q_i . k_j / 8 + maskbias_j) v_j              (transformer.py:382-387, 494, 514-530)
 * q/k/v are read in place from the projection outputs (no head transposes):
 *   q: [B][Nq][ldq]  head h at column q_off + h*64 ; k: [B][Nk][ldk] at k_off + (h / (H/Hkv))*64 ; v likewise
 *   (self-attention: q,k,v all point into the fused to_qkv output, ld = 3*D, offsets 0, D, 2D;
 *    cross-attention: q from to_q (ld=D), k/v from to_kv output (ld=2*Dc, offsets 0, Dc); GQA repeat_interleave 337-340)
 * rope_cos/rope_sin: [Npos][rot/2] fp32 tables or NULL - rotary on the first `rot` dims of q and k, applied on the fly:
 *   rot = 32 the DiT's partial rotary (transformer.py:146-170, 430-444), rot = head dim (64, or 128 through the _hd forms)
 *   the Llama decoder's (HF `apply_rotary_pos_emb` over the whole head, partners head_dim / 2 apart; the third-party model
 *   under model_sigmaVAE.py:17-29).
 * causal != 0: query i attends keys j <= i + (Nk - Nq) only (the Llama decoder called at model_sigmaVAE.py:78-81); the
 *   queries are then the LAST Nq positions (rotary position of query row i = i + Nk - Nq), which is what decoding against
 *   a KV cache needs (model_sigmaVAE.py:122-146 re-runs the prefix instead).
 * key_mask: uint8 [B][Nk] (1 = attend) or NULL.  lse: [B][H][Nq] fp32 saved for backward.  Head dim 64 here; the _hd
 * forms below take 32 and 128 too.
 * A masked key has probability exactly 0 wherever its batch row has a live key (masked_fill(-finfo.max), transformer.py:446-462;
 * the kernels fill with -1e30 in raw score units).  A batch row whose mask is all zero: the forward gives every key the same
 * weight, out = mean_j v_j (what the fill gives the reference too; with causal != 0 as well such a row is not defined: -1e30 is
 * also what a causally excluded key gets), and lse =
 * -1e30 / sqrt(dh) from the tiled kernels, -1e30 from the single-query kernel (finite, otherwise meaningless).  The backward
 * treats a masked key as absent: on every path dk and dv of a masked key are written as exact zeros, and in a fully masked
 * batch row dq, dk and dv are all exact zeros (NOT the uniform-weight gradient dv = mean_i dout_i that autograd through the
 * fill would give: such a row carries no signal); delta is written as rowsum(dout * out) there as everywhere.
 */
int kalle_attention_fwd(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                        const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                        const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                        int B, int H, int Hkv, int Nq, int Nk, void* stream);
/* backward: dq/dk/dv written with the same strides/offsets into dq_buf/dk_buf/dv_buf (bf16). For GQA dk/dv are
 * summed over the query heads sharing a kv head; RoPE is un-rotated on dq/dk. delta scratch: [B][H][Nq] fp32. */
int kalle_attention_bwd(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                        const void* v, int64_t ldv, int v_off, const void* out, const void* dout, int64_t ldo,
                        const float* lse, float* delta, void* dq, void* dk, void* dv,
                        const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                        int B, int H, int Hkv, int Nq, int Nk, void* stream);
/* The same two at head dim dh = head_dim in {32, 64, 128} (DiffusionTransformer(embed_dim, num_heads) -> dim_heads =
 * embed_dim // num_heads, dit.py:118; Attention(dim, dim_heads), transformer.py:290-300):
 *   out[b, i, h*dh+d] = softmax_j(q_i . k_j / sqrt(dh) + maskbias_j) v_j      (scale 1/sqrt(dh) in fp32: 0.17678 / 0.125 / 0.088388)
 *   q head h at column q_off + h*dh, k / v head (h / (H/Hkv)) at k_off / v_off + (h / (H/Hkv))*dh; out / dout / dq / dk / dv
 *   likewise with dh-wide heads; lse / delta [B][H][Nq] as above.
 * rot in {0, 32, 64, 128} and rot <= dh: rotary on the first rot dims of every head (RotaryEmbedding(max(dh // 2, 32)),
 * transformer.py:730: the DiT's rot is 32 at dh 32 - the whole head - and 64 at dh 128; rot 128 at dh 128 is a Llama decoder
 * with 128-wide heads, `AutoModelForCausalLM.from_pretrained(config['llm_model_name_or_path'])` at model_sigmaVAE.py:17-29 with a
 * Llama-3.2-3B / 3.1-8B checkpoint: tables [Npos][64]).
 * Anything else returns KALLE_ERR_ARG: a head dim or a rot without an instantiation (attn_head_dim_exists / attn_rot_exists in
 * csrc/attention.hip: head_dim not in {32, 64, 128}, rot not in {0, 32, 64, 128} or > head_dim), the null, size, alignment and
 * table checks of plan_attention there, causal with Nk < Nq.  head_dim 64 is exactly kalle_attention_fwd / _bwd (which forward
 * here); which kernel family a shape gets is the list of predicates next to attn_fold_tail in csrc/attention.hip, reported by
 * kalle_attn_last_plan and, with no device, by the _plan queries below. */
int kalle_attention_fwd_hd(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                           const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                           const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                           int B, int H, int Hkv, int Nq, int Nk, int head_dim, void* stream);
int kalle_attention_bwd_hd(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                           const void* v, int64_t ldv, int v_off, const void* out, const void* dout, int64_t ldo,
                           const float* lse, float* delta, void* dq, void* dk, void* dv,
                           const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                           int B, int H, int Hkv, int Nq, int Nk, int head_dim, void* stream);
/* Decoding against a KV cache: ONE query per batch row, the LAST position (rotary position Nk - 1, sees every key), against Nk
 * cached keys (model_sigmaVAE.py:122-146 re-runs `self.base_model.model(inputs_embeds=...)` over the prefix for every frame; with a
 * cache only this row is new).  q: [B][ldq], out: [B][ldo], lse: [B][H] or NULL, k / v / key_mask / tables as above.
 * It is kalle_attention_fwd_hd with causal = 1 and Nq = 1, and one family more (attn_fwd_decode128 in csrc/attention.hip):
 *   head_dim 64:  exactly that call, bit for bit (attn_decode_kernel<rot, AttnParams>, rot in {0, 32, 64})
 *   head_dim 128: rot = 128 only (attn_decode128_kernel: vector-ALU scoring with two lanes per key, block softmax over the scores
 *                 in LDS, P V with 16 lanes per key row; bf16 rounding of the rotated q / k and of the probabilities as in the tiled
 *                 kernel, so the two agree to the rounding of fp32 sums)
 *   Nk > KALLE_ATTN_DECODE_MAX_KEYS (the scores no longer fit in LDS): the tiled kernel of kalle_attention_fwd_hd at either head dim.
 * Anything else - head_dim 32 or any other, at head_dim 128 a rot other than 128 (at every Nk), and whatever
 * kalle_attention_fwd_hd refuses - returns KALLE_ERR_ARG and launches nothing. */
#define KALLE_ATTN_DECODE_MAX_KEYS 15360      /* keys whose fp32 scores the single-query kernels hold in LDS (60 KiB) */
int kalle_attention_decode_hd(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                              const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                              const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask,
                              int B, int H, int Hkv, int Nk, int head_dim, void* stream);
/* Batched decoding: R sequences (rows) of different lengths share one call.  Row r has ONE query q[r] at rotary position
 * nk[r] - 1 and attends keys 0 .. nk[r] - 1 of ITS OWN cache at k + r * kv_row_stride (elements; v likewise), rows of ldk / ldv
 * inside it; out: [R][ldo], lse: [R][H] or NULL.  nk is a HOST array of R ints, copied into the kernel's parameter block (as the
 * `layers` of kalle_llama_decode_step are read on the host): no device read-back, no copy.  nk[r] <= 0: row r is INACTIVE -
 * nothing of it is read (q, cache, tables) and nothing written (out, lse).  Cache rows >= nk[r] and table rows >= max(nk) are
 * never read.  The kernels are attn_decode_kernel<rot, AttnRowsParams> (head_dim 64, rot 64 or 0) and
 * attn_decode128_kernel<128, AttnRowsParams> (head_dim 128, rot 128): the templates of kalle_attention_decode_hd instantiated for
 * per-row lengths, so the same statements, arithmetic and rounding points; the LDS score array is sized by max(nk).
 * KALLE_ERR_ARG, nothing launched: R outside 1 .. KALLE_DECODE_MAX_ROWS, max(nk) > KALLE_ATTN_DECODE_MAX_KEYS (there is no tiled
 * fallback with per-row lengths), kv_row_stride negative or not a multiple of 8, rot 32 (attn_rot_exists), and whatever
 * kalle_attention_decode_hd refuses at Nk = max(max(nk), 1).  Every row inactive: KALLE_OK, nothing launched (plan word 0) -
 * checked like any other call first. */
#define KALLE_DECODE_MAX_ROWS 16
int kalle_attention_decode_rows(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                                const void* v, int64_t ldv, int v_off, int64_t kv_row_stride, void* out, int64_t ldo,
                                float* lse, const float* rope_cos, const float* rope_sin, int rot, const int32_t* nk,
                                int R, int H, int Hkv, int head_dim, void* stream);
/* Packed ragged batches (training on right-padded batches without the padding; the reference's flash_attention_2 path unpads and
 * calls variable-length attention whenever an attention_mask is given, model_sigmaVAE.py:18-22): nseq sequences share one buffer
 * of total_rows rows.  Sequence b owns the packed rows row0[b] .. row0[b] + len[b] - 1; there is no B / Nq / Nk block structure,
 * the row index of q / k / v / out / dout / dq / dk / dv IS the packed row, everything else (ld, column offset, head h at
 * off + h*dh, GQA as h / (H/Hkv)) is addressed as in kalle_attention_fwd_hd / _bwd_hd.
 *   Per sequence b the result is exactly kalle_attention_fwd_hd / _bwd_hd with B = 1, causal = 1, Nq = Nk = len[b],
 *   key_mask = NULL on that sequence's rows (the same kernel statements on a rebased parameter block: bit for bit);
 *   the rotary position of a row is row - row0[b] (tables [>= max_len][rot/2]).
 *   lse / delta: sequence b's block is [H][len[b]] at float offset H * row0[b]; the whole buffer is H * total_rows floats.
 * Sequences lie in increasing row order and do not overlap; rows between them and after the last one belong to nobody: such
 * rows of q / k / v / dout are never read, such rows of out / lse / delta / dq / dk / dv stay as found.
 * row0 / len are passed twice: as HOST int32 arrays (row0_host / len_host: read by the planner, as nk of
 * kalle_attention_decode_rows is) and as DEVICE int32 arrays (row0_dev / len_dev: read by the kernels).  The library allocates
 * nothing and copies nothing.  The host arrays are checked; THAT THE DEVICE ARRAYS HOLD THE SAME VALUES IS THE CALLER'S
 * CONTRACT (the kernels index the buffers by them).  max_len >= max(len) sizes the grid: forward (ceil(max_len/128), H, nseq),
 * backward that and then (ceil(max_len/128), Hkv, nseq); a workgroup whose block lies past its sequence leaves at once.
 * Supported: head_dim 64 with rot in {0, 64}, head_dim 128 with rot in {0, 64, 128}, GQA.  KALLE_ERR_ARG before any launch:
 * any other head_dim (32 included) or rot, nseq outside 1 .. 65535, a len[b] <= 0, overlapping or unordered sequences,
 * row0[b] + len[b] > total_rows, max_len < max(len), a NULL array, and the null / alignment / table checks of
 * kalle_attention_fwd_hd / _bwd_hd. */
int kalle_attention_fwd_varlen(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                               const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                               const float* rope_cos, const float* rope_sin, int rot,
                               int nseq, const int32_t* row0_host, const int32_t* len_host,
                               const int32_t* row0_dev, const int32_t* len_dev, int total_rows, int max_len,
                               int H, int Hkv, int head_dim, void* stream);
int kalle_attention_bwd_varlen(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                               const void* v, int64_t ldv, int v_off, const void* out, const void* dout, int64_t ldo,
                               const float* lse, float* delta, void* dq, void* dk, void* dv,
                               const float* rope_cos, const float* rope_sin, int rot,
                               int nseq, const int32_t* row0_host, const int32_t* len_host,
                               const int32_t* row0_dev, const int32_t* len_dev, int total_rows, int max_len,
                               int H, int Hkv, int head_dim, void* stream);
/* which kernel family the calling thread's most recent kalle_attention_fwd / _bwd (_hd) / kalle_attention_decode_hd /
 * kalle_attention_decode_rows / kalle_attention_fwd_varlen / _bwd_varlen launched; 0 when that call returned before launching
 * anything.
 *   bits 0-3   family; the condition of each is ONE predicate in csrc/attention.hip (next to attn_fold_tail), named here:
 *              1 fwd_tiled (attn_fwd_kernel: every forward that is neither 2 nor 6), 2 fwd_decode (attn_decode_kernel;
 *              attn_fwd_decode: head dim 64, Nq == 1, Nk <= KALLE_ATTN_DECODE_MAX_KEYS, causal or not), 3 bwd_two_pass
 *              (attn_bwd_kernel, dQ + delta then dK / dV: every backward that is neither 4 nor 5, so all of head dims 32 and 128),
 *              4 bwd_fused (attn_bwd_fused_kernel; attn_bwd_fused: head dim 64, not causal, H == Hkv, Nq, Nk <= 128), 5 bwd_fused_gqa
 *              (attn_bwd_fused_gqa_kernel; attn_bwd_fused_gqa, asked after 4: head dim 64, not causal, rot 0, Nq <= 128,
 *              max(Nk - 128, 0) <= min(16, 128 - Nq)), 6 fwd_decode_128 (attn_decode128_kernel; attn_fwd_decode128:
 *              kalle_attention_decode_hd at head dim 128, Nk <= KALLE_ATTN_DECODE_MAX_KEYS; a forward family: bit 4 is 0),
 *              7 fwd_decode_rows (attn_decode_kernel / attn_decode128_kernel on AttnRowsParams: kalle_attention_decode_rows; a forward
 *              family, head dim and ROT in their fields), 8 fwd_varlen (attn_fwd_kernel<1, dh, VARLEN>: kalle_attention_fwd_varlen),
 *              9 bwd_varlen (attn_bwd_kernel<KV, 1, dh, VARLEN>, dQ + delta then dK / dV: kalle_attention_bwd_varlen; bit 4 is 1):
 *              words 8 | dh << 8 and 9 | 16 | dh << 8
 *   bit 4      direction: 0 forward, 1 backward
 *   bits 8-15  head dim (32 / 64 / 128)
 *   bit 16     family 1: the keys 128 .. Nk - 1 were folded into the first block (Nk in (128, 160], rot 0, not causal)
 *   bits 17-24 families 2, 6 and 7: the ROT instantiation (0 / 32 / 64; 128 for family 6 and for 7 at head dim 128, which is why the field has 8 bits - every
 *              word of families 1-5 keeps the value it had with a 7-bit field) */
int kalle_attn_last_plan(void);
/* The planner of the entry points as pure host queries, one per entry point: its arguments without `stream`, then `plan`.
 * Pointers are tested for null and never read (nk is: a host array by contract); the same checks and return codes as the
 * entry point.  On KALLE_OK plan[0 .. 11] =
 *   [0] the word kalle_attn_last_plan would hold after the call   [1] the number of launches: 0 (kalle_attention_decode_rows with
 *   every row inactive; word 0), 1, or 2 (family 3: dQ + delta, then dK / dV)
 *   [2 .. 6] the first launch: grid x, y, z, block threads, dynamic LDS bytes   [7 .. 11] the second likewise; 0 where there is none
 * otherwise plan is left as found (a NULL plan is KALLE_ERR_ARG).  They launch nothing, need no device and do not change
 * kalle_attn_last_plan. */
int kalle_attention_fwd_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                             const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                             const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                             int B, int H, int Hkv, int Nq, int Nk, int head_dim, int* plan);
int kalle_attention_bwd_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                             const void* v, int64_t ldv, int v_off, const void* out, const void* dout, int64_t ldo,
                             const float* lse, float* delta, void* dq, void* dk, void* dv,
                             const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask, int causal,
                             int B, int H, int Hkv, int Nq, int Nk, int head_dim, int* plan);
int kalle_attention_decode_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                                const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                                const float* rope_cos, const float* rope_sin, int rot, const uint8_t* key_mask,
                                int B, int H, int Hkv, int Nk, int head_dim, int* plan);
int kalle_attention_decode_rows_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                                     const void* v, int64_t ldv, int v_off, int64_t kv_row_stride, void* out, int64_t ldo,
                                     float* lse, const float* rope_cos, const float* rope_sin, int rot, const int32_t* nk,
                                     int R, int H, int Hkv, int head_dim, int* plan);
/* (the varlen entry points likewise: row0_host / len_host are read, row0_dev / len_dev tested for null only; 2 launches for the
 * backward) */
int kalle_attention_fwd_varlen_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                                    const void* v, int64_t ldv, int v_off, void* out, int64_t ldo, float* lse,
                                    const float* rope_cos, const float* rope_sin, int rot,
                                    int nseq, const int32_t* row0_host, const int32_t* len_host,
                                    const int32_t* row0_dev, const int32_t* len_dev, int total_rows, int max_len,
                                    int H, int Hkv, int head_dim, int* plan);
int kalle_attention_bwd_varlen_plan(const void* q, int64_t ldq, int q_off, const void* k, int64_t ldk, int k_off,
                                    const void* v, int64_t ldv, int v_off, const void* out, const void* dout, int64_t ldo,
                                    const float* lse, float* delta, void* dq, void* dk, void* dv,
                                    const float* rope_cos, const float* rope_sin, int rot,
                                    int nseq, const int32_t* row0_host, const int32_t* len_host,
                                    const int32_t* row0_dev, const int32_t* len_dev, int total_rows, int max_len,
                                    int H, int Hkv, int head_dim, int* plan);

/* ------------------------------------------------------------------------------------------------
 * Optimizer: fused Adam / AdamW over a flat fp32 master buffer, also emitting the bf16 compute copy.
 *   (training/utils.py:88-93 torch.optim / FusedAdam; train_offline.py:94-100 AdamW)
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce SUM, loss scaling, ...).
 */
int kalle_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                    int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                    int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-norm clipping and the non-finite skip, decided on the device (torch.nn.utils.clip_grad_norm_,
 * train_offline.py:246; GradScaler's skipped optimizer step, train.py:136,180-190).  Three stages, every one of them
 * readable in device memory:
 *
 *   kalle_grad_sumsq        one streaming pass over grad[0..n): sum of squares in double + "saw +-inf / NaN", written as
 *                           KALLE_GRAD_NORM_PARTIALS per-workgroup partials into region `slot` of the workspace
 *   kalle_grad_norm_finish  one workgroup: sums every region in index order, publishes norm / coef / nonfinite / skip in a
 *                           kalle_opt_ctl and bumps its counters
 *   kalle_adam_step_ctl     kalle_adam_step whose gradient factor is f32(grad_scale * ctl->coef) and which writes nothing
 *                           when ctl->skip is set
 *
 * Workspace (kalle_grad_norm_ws_bytes(nslots) bytes, 16-byte aligned, caller-owned), region s = 0 .. nslots - 1 at byte
 * s * KALLE_GRAD_NORM_SLOT_BYTES:
 *     double  sumsq[KALLE_GRAD_NORM_PARTIALS]     workgroup b's sum of g^2 over the elements it read, each g widened to double
 *                                                 first (exact, no overflow at 1e20, no underflow at 1e-30); 0 if it read none
 *     int32_t bad[KALLE_GRAD_NORM_PARTIALS]       1 if workgroup b read an element whose fp32 exponent bits are all set
 * A launch is always KALLE_GRAD_NORM_PARTIALS workgroups of KALLE_GRAD_NORM_BLOCK lanes; a lane reads KALLE_GRAD_NORM_UNROLL
 * 16-byte vectors per grid sweep (one sweep = PARTIALS * BLOCK * UNROLL * 4 elements), the n % 4 tail belongs to workgroup 0.
 * Which element a workgroup reads, and the order in which its lanes, waves and the partials are added, are functions of
 * (n, slot) alone - no floating-point atomics, no "last arriver" - so the published norm is the same bit pattern whichever
 * bucket or workgroup finishes first, and the same on every rank.
 * kalle_grad_norm_finish does not clear the workspace: the caller writes every slot before every finish.
 *
 * KALLE_ERR_ARG before any launch (so the refusals need no device): a NULL pointer (stream excepted), n <= 0, nslots <= 0,
 * slot outside [0, nslots), grad / ws not 16-byte aligned, ctl not 8-byte aligned, step <= 0.
 */
#define KALLE_GRAD_NORM_PARTIALS 1024
#define KALLE_GRAD_NORM_BLOCK 256
#define KALLE_GRAD_NORM_UNROLL 4
#define KALLE_GRAD_NORM_SLOT_BYTES (KALLE_GRAD_NORM_PARTIALS * 12)
typedef struct kalle_opt_ctl {   /* device memory; written by kalle_grad_norm_finish, read by kalle_adam_step_ctl */
    float   norm;        /* || grad_scale * g ||_2 over every slot: (float)(sqrt(S) * (double)grad_scale) */
    float   coef;        /* multiplies grad_scale in the Adam kernel: 1, or < 1 when clipping:
                          * 0 < max_norm < inf ? (float)min(1.0, max_norm / (norm + 1e-6)) in double from the rounded norm : 1
                          * (a NaN norm gives 1: such a step is either skipped or lost, as under clip_grad_norm_) */
    int32_t nonfinite;   /* 1: some gradient element was +-inf or NaN */
    int32_t skip;        /* 1: nonfinite && skip_nonfinite - the Adam kernel writes nothing */
    int64_t skipped;     /* running counts, incremented by finish: steps with skip set, */
    int64_t clipped;     /* steps with coef < 1 */
} kalle_opt_ctl;
int kalle_grad_norm_ws_bytes(int nslots);                 /* host query; <= 0 slots: KALLE_ERR_ARG */
int kalle_grad_sumsq(const float* grad, int64_t n, void* ws, int slot, int nslots, void* stream);
int kalle_grad_norm_finish(const void* ws, int nslots, float grad_scale, float max_norm, int skip_nonfinite,
                           kalle_opt_ctl* ctl, void* stream);
int kalle_adam_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                        int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                        int step, float grad_scale, const kalle_opt_ctl* ctl, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 1-D convolution stack of the audio VAEs (no MFMA; LDS line buffers, coalesced HBM).
 * Layout (B, C, L) fp32 or bf16 activations, fp32 weights (weight-norm already folded: w = g * v/||v||).
 */
/* fold weight norm and repack to the kernels' weight layout [Cin][K][CoutP] fp32, CoutP = Cout rounded up to a multiple
 * of 8 with the pad columns zeroed (w_packed must hold Cin*K*CoutP floats), so a wave's 8 output-channel weights of a
 * tap are one aligned scalar load (once per forward; weights are frozen in every reference script, factory.py:77-80):
 *   transposed=0 (Conv1d):          v [Cout=d0][Cin=d1][K], g [Cout] -> w[ci][k][co] = g[co] v[co][ci][k] / ||v[co,:,:]||
 *   transposed=1 (ConvTranspose1d): v [Cin=d0][Cout=d1][K], g [Cin]  -> w[ci][k][co] = g[ci] v[ci][co][k] / ||v[ci,:,:]||
 *   g == NULL: repack only (plain nn.Conv1d).   (dac.nn.layers.WNConv1d -> torch weight_norm; autoencoders.py:9)
 *   transposed | 2: additionally store tap k at K-1-k - with transposed=1 on a Conv1d's (v, g) this is the weight of the
 *   convolution that computes the DATA gradient of a stride-1 conv (kalle_conv1d_fwd over dy, padding (K-1)*dil - pad). */
int kalle_weight_norm_fold(const float* v, const float* g, float* w_packed, int d0, int d1, int ksize,
                           int transposed, void* stream);
/* activation descriptor of the conv kernels.  code: 0 none, 1 Snake / SnakeBeta x + sin^2(a x)/(b + 1e-9) with per-channel
 * alpha / beta (exp() applied first when logscale; plain Snake passes alpha as beta too; blocks.py:301-339,
 * backup/flows.py:51-62,113-126), 2 ELU, 3 LeakyReLU(negative_slope = param) (backup/flows.py:177-181,217,230),
 * 4 (input side only) WaveNet gate tanh(x[:, :Cin]) * sigmoid(x[:, Cin:]) - x then has 2*Cin channels
 * (backup/flows.py:614-620). */
typedef struct kalle_act {
    int32_t code;
    int32_t logscale;
    const float* alpha;
    const float* beta;
    float param;
} kalle_act;
/* what the conv kernels fuse into their store:
 *   v = (conv + bias + residual) * out_scale;  if accumulate: v += y (previous contents: sum over the parallel AMP blocks,
 *   backup/flows.py:517-523);  v = post_act(v) (the NEXT layer's input activation, per output channel, applied once here
 *   instead of once per consumer tile);  if tanh: v = tanh(v) (autoencoders.py:185).  residual has y's shape and x's dtype. */
typedef struct kalle_conv_epilogue {
    const void* residual;
    float out_scale;
    int32_t accumulate;
    int32_t tanh;
    kalle_act post_act;
    void* y_raw;   /* optional second output: the value BEFORE post_act / tanh (y's shape and dtype) - a residual unit's output
                      is needed raw by the next unit's skip path and activated by its first conv */
} kalle_conv_epilogue;
/* y = epilogue(conv1d(in_act(x), w, b, stride, padding, dilation)); in_act / epi may be NULL (= none / plain store).
 *   `padding` is the LEFT zero pad; the right pad is implied by Lout (symmetric padding: autoencoders.py:45,76;
 *   causal left-only padding: backup/flows.py:574-575,602-603).  ksize <= 16.
 *   (autoencoders.py:39-62 ResidualUnit, 64-81 EncoderBlock, 116-191 encoder/decoder stems) */
int kalle_conv1d_fwd(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y, int y_dtype, int B,
                     int Cin, int Lin, int Cout, int Lout, int ksize, int stride, int padding, int dilation,
                     const kalle_act* in_act, const kalle_conv_epilogue* epi, void* stream);
/* Few positions, many channels (the C >= 512 top of the VAE; all of a single-clip decode): stride-1 conv with the roles of
 * lanes and registers swapped (lane = 4 output channels, 16 positions in registers, weights as coalesced vector loads, the
 * step's inputs as one scalar load).  Two calls: kalle_conv_pad_act writes act(x) into a zero-padded fp32 copy
 * x_padded [B][C][Lp] (`padding` leading zeros, Lp = kalle_conv_pad_len(...)), kalle_conv1d_cfirst_fwd convolves it (same
 * epilogue struct as kalle_conv1d_fwd; fp32 only).  Strided convs (dilation 1): pass phases = stride and padding =
 * ceil(padding / stride) * stride to kalle_conv_pad_act - the copy is then de-interleaved into `stride` phase rows so that a
 * tap's inputs for consecutive outputs are consecutive.  The caller owns x_padded.  Any B x C (rows ride on grid x). */
int kalle_conv_pad_len(int Lout, int ksize, int stride, int padding, int dilation);
int kalle_conv_pad_act(const float* x, float* x_padded, int B, int C, int Lin, int Lp, int padding, const kalle_act* act,
                       int phases, void* stream);
/* workspace (optional, fp32, kalle_conv_cfirst_ws_floats(...) elements; that count is 0 when it would not be used): lets the
 * launch split the input channels over workgroups too - partial sums land there and a second small kernel applies the
 * epilogue.  For the bottom of a single-clip encode (1024 -> 2048 stride 8 and 2048 -> 128 at 215 positions, the encoder of
 * autoencoders.py:116-147 as twj_dataset.py:239 calls it clip by clip). */
int kalle_conv_cfirst_ws_floats(int B, int Cin, int Cout, int Lout, int ksize);
int kalle_conv1d_cfirst_fwd(const float* x_padded, const float* w_packed, const float* bias, float* y, int B, int Cin,
                            int Lp, int Cout, int Lout, int ksize, int stride, int padding, int dilation,
                            const kalle_conv_epilogue* epi, float* workspace, void* stream);
/* the same for a transposed conv (one pass per output phase): x_padded [B][C][Lp] = kalle_conv_pad_act(x, padding =
 * ceil(ksize / stride) - 1), Lp >= kalle_convT_pad_len(Lout, ksize, stride, padding) */
int kalle_convT_pad_len(int Lout, int ksize, int stride, int padding);
int kalle_conv_transpose1d_cfirst_fwd(const float* x_padded, const float* w_packed, const float* bias, float* y, int B,
                                      int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding,
                                      const kalle_conv_epilogue* epi, void* stream);
/* y = epilogue(conv_transpose1d(in_act(x), w, b, stride, padding))   (autoencoders.py:98-100 DecoderBlock);
 * Lout may be shorter than the full length: the causal variant trims the last `stride` outputs (backup/flows.py:383-384);
 * and up to `padding` longer (outputs the symmetric right trim would drop: the data gradient of a strided conv) */
int kalle_conv_transpose1d_fwd(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                               int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                               int padding, const kalle_act* in_act, const kalle_conv_epilogue* epi, void* stream);
/* Ragged batches: the five forward entry points above with per-row valid lengths.  Row b of x [B][C][Lin] is a tensor of
 * lens_in[b] positions and row b of y [B][Cout][Lout] one of lens_out[b]; the row strides stay Lin and Lout.
 *   - inputs at positions >= lens_in[b] read as ZERO, whatever the memory holds (what zero padding supplies when the row runs
 *     alone); the mask acts on the load, before the input activation, and every input activation maps 0 to 0;
 *   - outputs (y and y_raw) at positions >= lens_out[b] are NOT WRITTEN (the buffers keep their contents there);
 *   - lens_in[b] == 0 makes row b inactive: lens_out[b] must be 0 and nothing of the row is read or written; a workgroup whose
 *     position tile lies at or past lens_out[b] leaves before it stages anything, so the cost follows the live samples;
 *   - every row inactive: KALLE_OK, nothing launched.
 * Each array (int32 [B]) is passed twice, as row0 / len of kalle_attention_fwd_varlen are: ..._host is checked here and read by
 * nobody else, ..._dev is what the kernels read; that the two agree is the caller's contract.  All arrays NULL = the dense
 * entry point (which is that call).  Refused with KALLE_ERR_ARG before any launch: some but not all arrays NULL; a length < 0;
 * lens_in[b] > Lin; lens_out[b] > Lout; lens_out[b] beyond what lens_in[b] inputs yield - conv: (lens_in[b] - 1 + padding) /
 * stride + 1, transposed: (lens_in[b] - 1) * stride - padding + ksize (the bounds the dense calls put on Lout against Lin).
 * The plan does not depend on the lengths: kalle_conv_plan / kalle_conv_transpose_plan answer for (B, Lin, Lout) as for the
 * dense call, and kalle_conv_last_plan after a _lens call that passed its checks is the dense call's word (also when every row
 * was inactive).  Channels-per-lane families: kalle_conv_pad_act_lens applies lens_in (zeros from lens_in[b] on; an inactive
 * row's copy is not made), kalle_conv1d_cfirst_fwd_lens checks lens_out against lens_in (it cannot know Lin) and obeys lens_out,
 * kalle_conv_transpose1d_cfirst_fwd_lens takes lens_out only.  Forward only: no backward kernel takes lengths. */
int kalle_conv1d_fwd_lens(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y, int y_dtype, int B,
                          int Cin, int Lin, int Cout, int Lout, int ksize, int stride, int padding, int dilation,
                          const kalle_act* in_act, const kalle_conv_epilogue* epi, const int32_t* lens_in_host,
                          const int32_t* lens_in_dev, const int32_t* lens_out_host, const int32_t* lens_out_dev, void* stream);
int kalle_conv_transpose1d_fwd_lens(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                                    int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                                    int padding, const kalle_act* in_act, const kalle_conv_epilogue* epi,
                                    const int32_t* lens_in_host, const int32_t* lens_in_dev, const int32_t* lens_out_host,
                                    const int32_t* lens_out_dev, void* stream);
int kalle_conv_pad_act_lens(const float* x, float* x_padded, int B, int C, int Lin, int Lp, int padding, const kalle_act* act,
                            int phases, const int32_t* lens_in_host, const int32_t* lens_in_dev, void* stream);
int kalle_conv1d_cfirst_fwd_lens(const float* x_padded, const float* w_packed, const float* bias, float* y, int B, int Cin,
                                 int Lp, int Cout, int Lout, int ksize, int stride, int padding, int dilation,
                                 const kalle_conv_epilogue* epi, float* workspace, const int32_t* lens_in_host,
                                 const int32_t* lens_in_dev, const int32_t* lens_out_host, const int32_t* lens_out_dev,
                                 void* stream);
int kalle_conv_transpose1d_cfirst_fwd_lens(const float* x_padded, const float* w_packed, const float* bias, float* y, int B,
                                           int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding,
                                           const kalle_conv_epilogue* epi, const int32_t* lens_out_host,
                                           const int32_t* lens_out_dev, void* stream);
/* which kernel the calling thread's most recent kalle_conv1d_fwd / kalle_conv_transpose1d_fwd / kalle_conv1d_cfirst_fwd /
 * kalle_conv_transpose1d_cfirst_fwd / kalle_conv_wgrad launched; 0 when that call returned before launching anything.
 *   bits 0-3 family: 1 conv1d_kernel (fallback), 2 conv1d_v2_kernel, 3 convT1d_kernel (fallback), 4 convT1d_v2_kernel,
 *                    5 conv1d_cfirst_kernel stride 1, 6 the same strided (phase rows), 7 the same transposed,
 *                    8 conv_wgrad_lds_kernel, 9 conv_wgrad_kernel (per-lane loads)
 *   bit 4 / bit 5:   x / y is fp32 (both set for the fp32-only families 5-9)
 *   families 2, 4:   bits 8-12 COW (output channels per wave), 13-16 LPT (positions per lane), 17-20 WCO (waves along the
 *                    channels), 21-24 NW (waves per workgroup), 25-27 log2(CI / 8) (input-channel chunk 8 / 16 / 32),
 *                    28-30 log2(stride) (the de-interleaved stride 2 / 4 / 8 forms of family 2)
 *   families 5-7:    bits 8-11 split (waves that share a position tile's input channels: 1 / 2 / 4), bits 12-16 ks (workgroup-level
 *                    input-channel split; > 1 means cfirst_finish_kernel ran too)
 *   family 8:        bits 8-12 TU, 13-17 KT;    family 9: bits 8-12 TU, 13-17 TV, 18-22 KM */
int kalle_conv_last_plan(void);
/* The dispatch as pure host queries: no device, nothing launched, kalle_conv_last_plan and every other state left alone.
 * kalle_conv_plan / kalle_conv_transpose_plan answer for one conv what kalle_audio_amd/conv_ops.py asks them before every
 * call, so a C caller that follows the answer gets the same dispatch.  Arguments: those of kalle_conv1d_fwd /
 * kalle_conv_transpose1d_fwd without the tensors and the stream (in_act / epi as there, may be NULL; their pointers are tested
 * for null only, never read) plus `prefer`: 0 = auto (the channels-per-lane kernels where their cost rule in csrc/conv1d.hip
 * asks for them), 1 = the channels-per-lane kernels wherever the call is eligible, 2 = never.  Eligible: fp32 in and out, in_act
 * not the gate (4), stride == 1 or dilation == 1; transposed: Lout at most the symmetric (Lin - 1) stride - 2 padding + ksize
 * (trimmed, not extended).  The planner of the chosen entry point then checks the arguments: its return code is the query's,
 * and a refused query leaves `out` alone.  On success out[0..5] =
 *   family (bits 0-3 of the word: 1 / 2 call kalle_conv1d_fwd, 3 / 4 kalle_conv_transpose1d_fwd, 5 / 6 kalle_conv1d_cfirst_fwd,
 *   7 kalle_conv_transpose1d_cfirst_fwd), the word kalle_conv_last_plan holds after that call, and for families 5-7 what the
 *   call needs: Lp (length of x_padded), lead and phases (`padding` and `phases` of kalle_conv_pad_act), workspace floats (0:
 *   pass NULL; the word's ks assumes a workspace of that size is lent).  Families 1-4 leave those four 0.
 * kalle_conv_wgrad_plan: the arguments of kalle_conv_wgrad without tensors and stream; out[0..4] = family (8 / 9), word,
 * grid x, y, z. */
int kalle_conv_plan(int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride, int padding,
                    int dilation, const kalle_act* in_act, const kalle_conv_epilogue* epi, int prefer, int32_t* out);
int kalle_conv_transpose_plan(int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                              int padding, const kalle_act* in_act, const kalle_conv_epilogue* epi, int prefer, int32_t* out);
int kalle_conv_wgrad_plan(int B, int CU, int CV, int MU, int LV, int ksize, int stride, int padding, int dilation, int act_on,
                          const kalle_act* act, int32_t* out);
/* ------------------------------------------------------------------------------------------------
 * Llasa task model head / tail (model_sigmaVAE.py:53-104); the Llama decoder layers in between run on kalle_gemm_bf16,
 * kalle_rmsnorm_*, kalle_attention_* (causal, rot = head_dim = 64 or 128, GQA).
 */
/* out = a x + b y, fp32   (fixed-sigma sampling x = mean + std * randn, model_sigmaVAE.py:150-166) */
int kalle_axpby(const float* x, const float* y, float* out, float a, float b, int64_t n, void* stream);
/* one-row GEMM for decoding against a KV cache: y[n] = sum_k W[n][k] x[k] (+ residual[n]); x bf16 [K], W bf16 [N][ldw],
 * y bf16 or fp32 [N], residual fp32 [N] or NULL; K % 8 == 0, K <= 32768 */
int kalle_gemv_bf16(const void* x, const void* W, int64_t ldw, void* y, int y_dtype, const float* residual, int N, int K,
                    void* stream);
/* One KV-cached decode step of the whole Llama stack (batch 1, one new position t0), sequenced on the C side so that a
 * generated frame costs one host call instead of ~150 Python-level launches (model_sigmaVAE.py:122-146 runs
 * `self.base_model.model(inputs_embeds=...)` over the growing prefix once per frame; with a cache only the new position
 * is computed).  Per layer: [RMSNorm + fused q|k|v GEMV, k|v written straight into cache row t0] -> causal GQA attention
 * over rows 0..t0 -> [o_proj GEMV + residual] -> [RMSNorm + up|gate GEMV] -> [SwiGLU + down GEMV + residual].
 *   layers: HOST array of n_layers descriptors; weights bf16 row-major ([out][in]; wqkv = [q;k;v], wug = [up;gate]),
 *           norm weights fp32 [D], kv_cache bf16 [cache_rows][2*Hkv*64] holding un-rotated k | v of positions < t0
 *   x: fp32 [D] input embedding of position t0; out: fp32 [D] residual stream after the last layer (final norm not applied)
 *   rope_cos / rope_sin: fp32 [>= t0+1][32]; workspace: kalle_llama_decode_ws_bytes(H, Hkv, inner) bytes, 64-byte aligned
 *   H % Hkv == 0, inner % 8 == 0, 0 <= t0 < cache_rows, D = 64 H <= 32768, inner <= 32768 (a GEMV keeps its K-long bf16 operand in
 *   LDS: 64 KiB at the bound); anything else, or a NULL field in the descriptor of ANY layer, returns KALLE_ERR_ARG before the
 *   first launch.  Every launch is checked where it is made: a refused launch returns KALLE_ERR_LAUNCH at once.
 * This step and its head-dim, R-row and e4m3 forms below are argument adapters of one sequencer (decode_step, csrc/llasa.hip):
 * the argument checks, the workspace carve-up and the per-layer sequence exist once.
 * Only row t0 of each cache is written (all 2*Hkv*64 of it); rows above t0 and rope rows above t0 are never read.
 * The workspace is caller-owned and its layout is part of this contract (D = 64 H), in this order:
 *   x2  fp32 [D]                         residual stream after the attention branch: x_in + Wo . ao
 *   x3  fp32 [D]                         output of the layer before the last one = input of the last layer (n_layers >= 2;
 *                                        a one-layer call does not touch it)
 *   lse fp32 [H], padded to a multiple of 64 bytes (the padding is never written)
 *   q   bf16 [D]                         bf16(Wq . bf16(rmsnorm(x_in)))            (un-rotated; k | v of the same GEMV are in cache row t0)
 *   ao  bf16 [D]                         attention output
 *   hf  bf16 [2*inner]                   up | gate = bf16(Wug . bf16(rmsnorm(x2)))
 * After a call every region holds the LAST layer's values (x_in = x for one layer, x3 otherwise), so that each stage of a layer
 * can be checked from that stage's own inputs; out = x2 + Wdown . bf16(up * silu(gate)).  bf16 rounding points of a layer: the
 * two normalised activations, q | k | v, the rotated q and k and the probabilities inside the attention, ao, up | gate, and
 * up * silu(gate); x2, x3 and out stay fp32. */
typedef struct kalle_llama_layer {
    const float* input_norm;
    const void* wqkv;
    const void* wo;
    const float* post_norm;
    const void* wug;
    const void* wdown;
    void* kv_cache;
} kalle_llama_layer;
int kalle_llama_decode_ws_bytes(int H, int Hkv, int inner);
int kalle_llama_decode_step(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int H, int Hkv,
                            int inner, float eps, int t0, int cache_rows, const float* rope_cos, const float* rope_sin,
                            void* workspace, void* stream);
/* The same two for a decoder whose heads are head_dim = 64 or 128 wide (`AutoModelForCausalLM.from_pretrained(
 * config['llm_model_name_or_path'])`, model_sigmaVAE.py:17-29, accepts any Llama checkpoint: Llama-3.2-1B has 64-wide heads,
 * Llama-3.2-3B and Llama-3.1-8B 128-wide ones).  Everything above holds with D = H * head_dim, cache rows of 2 * Hkv * head_dim
 * (k | v), rope tables [>= t0+1][head_dim / 2] and rotary over the whole head; the workspace layout is the one above with that D
 * (kalle_llama_decode_ws_bytes_hd bytes); the limits D <= 32768 and inner <= 32768 are the GEMV's and do not depend on the head.
 * The attention of a layer is kalle_attention_decode_hd.  head_dim = 64 is exactly the two functions above, which forward here;
 * any other head_dim than 64 or 128 returns KALLE_ERR_ARG. */
int kalle_llama_decode_ws_bytes_hd(int H, int Hkv, int inner, int head_dim);
int kalle_llama_decode_step_hd(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int H, int Hkv,
                               int inner, int head_dim, float eps, int t0, int cache_rows,
                               const float* rope_cos, const float* rope_sin, void* workspace, void* stream);
/* ---- batched KV-cached decoding: R = 1 .. KALLE_DECODE_MAX_ROWS sequences (rows) per step ------------------------------------
 * The reference's inference scripts run a list of utterances through `model.infer` one after the other (infer_0828_sigma.py:313);
 * a decode step reads every decoder weight once and does one multiply-add per weight read, so R rows per step share that stream.
 *
 * Skinny GEMM: Y[r][n] = sum_k W[n][k] X[r][k] (+ residual[r][n]) for R rows; W bf16 [N][ldw] is read from HBM once for all rows
 * (gemm_rows_kernel<YF32, TR, 1>: 8 weight rows per workgroup below N = 8192 and 16 from there - as many workgroups as kalle_gemv_bf16 has or
 * more - x 16 batch columns of v_mfma_f32_16x16x32_bf16, the unused columns zero, the four waves splitting K; fp32 accumulation,
 * order unspecified but fixed).  X bf16 [R][ldx], Y bf16 or fp32 [R][ldy], residual
 * fp32 [R][ldres] or NULL.  K % 8 == 0, ldx % 8 == 0, ldw % 8 == 0, K <= 32768 (as kalle_gemv_bf16), 1 <= R <= 16. */
int kalle_gemm_rows_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, int y_dtype,
                         const float* residual, int64_t ldres, int R, int N, int K, void* stream);
/* The form the batched step uses.  On top of the above:
 *   prologue (the three of the one-row kernel, per row, rounded to bf16 at the same points):
 *     KALLE_PRO_BF16   x bf16 [R][ldx] used as is (gamma, eps, xhat unused)
 *     KALLE_PRO_RMS    x fp32 [R][ldx] (ldx % 4 == 0) -> bf16(x * (gamma * rsqrt(mean(x^2) + eps)))
 *     KALLE_PRO_SWIGLU x bf16 [R][ldx] = up [K] | gate [K] per row -> bf16(up * silu(gate))
 *     the last two run as a pre-pass (one launch, a workgroup per row) that writes the operand once into xhat, bf16 [R][K]
 *     caller scratch, instead of once per workgroup of the GEMM;
 *   nsplit / y2 / y2_off: output columns n >= nsplit of row r go to y2 + y2_off[r] + (n - nsplit) (elements of y's dtype; y2_off
 *     a HOST array [R]): k | v of the fused q|k|v projection land in cache row t0[r] of sequence r.  nsplit = N: no second
 *     destination (y2, y2_off may be NULL);
 *   active: HOST int32 [R] or NULL (all rows).  active[r] == 0: nothing of row r is read (x, residual) or written (xhat, y, y2).
 * Both arrays travel in the kernel's parameter block. */
#define KALLE_PRO_BF16 0
#define KALLE_PRO_RMS 1
#define KALLE_PRO_SWIGLU 2
int kalle_gemm_rows_fused(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat, const void* W,
                          int64_t ldw, void* y, int64_t ldy, int y_dtype, void* y2, int nsplit, const int64_t* y2_off,
                          const float* residual, int64_t ldres, const int32_t* active, int R, int N, int K, void* stream);
/* kalle_llama_decode_step_hd on R rows.  x, out: fp32 [R][D]; t0: HOST int32 [R], the new position of each row, NEGATIVE = the
 * row is inactive (finished, or padding): nothing is read or written for it anywhere - not its cache, not its workspace rows,
 * not its out row.  kv_cache of a layer: bf16 [R][cache_rows][2*Hkv*head_dim]; only row t0[r] of sequence r is written.
 * rope tables: [>= max(t0)+1][head_dim/2].  Per layer (8 launches): RMSNorm pre-pass -> q|k|v skinny GEMM (k|v into the caches)
 * -> kalle_attention_decode_rows (nk = t0 + 1) -> o_proj + residual -> RMSNorm pre-pass -> up|gate -> SwiGLU pre-pass -> down +
 * residual.  Limits: those of the _hd step, 1 <= R <= 16, t0[r] < cache_rows, max(t0) < KALLE_ATTN_DECODE_MAX_KEYS; anything else returns
 * KALLE_ERR_ARG before the first launch and leaves no attention plan.  Every launch is checked where it is made.  Every row
 * inactive: KALLE_OK, nothing launched.
 * Workspace (kalle_llama_decode_ws_bytes_rows bytes, 64-byte aligned), the regions of the one-row step, each [R][...] row-major,
 * and one more for the pre-pass operand:
 *   x2  fp32 [R][D] | x3 fp32 [R][D] | lse fp32 [R][H], the region padded to a multiple of 64 bytes | q bf16 [R][D] |
 *   ao bf16 [R][D] | hf bf16 [R][2*inner] | xn bf16 [R][max(D, inner)]: the LAST pre-pass's operand (up * silu(gate), row
 *   stride max(D, inner), the first `inner` of each row) */
int kalle_llama_decode_ws_bytes_rows(int R, int H, int Hkv, int inner, int head_dim);
int kalle_llama_decode_step_rows(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int R, int H,
                                 int Hkv, int inner, int head_dim, float eps, const int32_t* t0, int cache_rows,
                                 const float* rope_cos, const float* rope_sin, void* workspace, void* stream);
/* ---- the wide decode step: up to KALLE_DECODE_WIDE_MAX_ROWS rows share one read of the weights ---------------------------------
 * 16 is the width of one MFMA column block, not an optimum: a batched step is a fixed cost plus very little per row.  The wide
 * forms serve 1 <= R <= 64 rows with the arguments, the meaning and the refusals of the _rows forms above (the bound on R at
 * 64): inactive rows (active[r] == 0 / t0[r] < 0) are neither read nor written, the second destination goes through y2_off,
 * every refusal comes before the first HIP call, every launch is checked where it is made.  Up to 16 rows they forward to
 * the _rows forms.  Above, the projections run in the same gemm_rows_kernel template at NCB = ceil(R / 16) column blocks (one
 * weight-chunk load feeds NCB MFMAs, one per block of 16 batch rows; 16 weight rows per workgroup from N = 3072, 8 below) after the pre-pass, and the step runs
 * kalle_attention_decode_rows once per chunk of 16 rows that has an active row (kalle_attn_last_plan: the last chunk launched).
 * A ROW'S BITS ARE THOSE OF THE 16-ROW PATH: for one (weight row, batch row) pair the accumulation walks K in
 * the order of the NCB = 1 instantiation, so y, the caches and every workspace region of row r equal what the _rows form writes for a group
 * of up to 16 rows that holds r, whatever R, the row's index or the other rows.
 * Workspace: the published _rows layout at that R (kalle_llama_decode_ws_bytes_wide bytes).
 * Not served, KALLE_ERR_ARG: e4m3 layers (there is no _wide_w8 form), R > 64, head dim 32. */
#define KALLE_DECODE_WIDE_MAX_ROWS 64
/* kalle_gemm_rows_fused for 1 <= R <= 64, bf16 weights: same arguments, same meaning */
int kalle_gemm_rows_wide(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat, const void* W,
                         int64_t ldw, void* y, int64_t ldy, int y_dtype, void* y2, int nsplit, const int64_t* y2_off,
                         const float* residual, int64_t ldres, const int32_t* active, int R, int N, int K, void* stream);
int kalle_llama_decode_ws_bytes_wide(int R, int H, int Hkv, int inner, int head_dim);
/* kalle_llama_decode_step_rows for 1 <= R <= 64, bf16 layers */
int kalle_llama_decode_step_wide(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int R, int H,
                                 int Hkv, int inner, int head_dim, float eps, const int32_t* t0, int cache_rows,
                                 const float* rope_cos, const float* rope_sin, void* workspace, void* stream);
/* Packed prefill into a batch cache: after the q|k|v GEMM over the packed rows of several prompts (kalle_attention_fwd_varlen's
 * layout), the un-rotated k|v window of every sequence goes to that sequence's cache row, all sequences in ONE launch.
 *   src   bf16 [total_rows][ld_src], the k|v window at column src_off (kvw = 2*Hkv*head_dim columns)
 *   cache bf16 [R][cache_rows][kvw], row r at cache + r * cache_row_stride (elements)
 * Sequence s < nseq (<= KALLE_DECODE_MAX_ROWS) owns packed rows row0[s] .. row0[s] + len[s] - 1; row j of it is copied, bit for
 * bit, to cache[dst_row[s]][t0[s] + j][0 .. kvw).  Nothing else is written.  row0 / len / dst_row / t0 are HOST arrays [nseq] and
 * travel in the kernel's parameter block.  A workgroup moves KALLE_KV_APPEND_ROWS rows of one sequence, 16 bytes per lane.
 * KALLE_ERR_ARG before any launch (so the refusals need no device): a NULL pointer (stream excepted) or src / cache not 16-byte
 * aligned; nseq outside 1 ..
 * KALLE_DECODE_MAX_ROWS; R outside 1 .. KALLE_DECODE_MAX_ROWS; len <= 0, t0 < 0 or t0 + len > cache_rows; dst_row outside [0, R)
 * or named twice; row0 < 0 or row0 + len > total_rows; sequences overlapping or not in increasing row order; kvw, ld_src,
 * src_off or cache_row_stride <= 0 (src_off: < 0) or not a multiple of 8 elements; src_off + kvw > ld_src; cache_row_stride <
 * cache_rows * kvw. */
#define KALLE_KV_APPEND_ROWS 32
int kalle_kv_append_varlen(const void* src, int64_t ld_src, int src_off, void* cache, int64_t cache_row_stride, int kvw,
                           int nseq, const int32_t* row0_host, const int32_t* len_host, const int32_t* dst_row_host,
                           const int32_t* t0_host, int total_rows, int R, int cache_rows, void* stream);
/* ---- weight-only FP8 decoding: the decoder weights as OCP e4m3 codes with one fp32 scale per output row ------------------------
 * A decode step reads every decoder weight once, so a frame costs the bytes of the weights; this halves them.  Activations,
 * accumulation (fp32) and every bf16 rounding point of the steps above stay where they are.  Opt-in: nothing above changes.
 * Format:
 *   W8    uint8 [N][ldq], OCP `e4m3fn` codes (sign, 4 exponent bits with bias 7, 3 mantissa bits: exponent 0 is man/8 * 2^-6,
 *         otherwise (1 + man/8) * 2^(exp-7); 0x7E = 448 is the largest) - NOT the `e4m3fnuz` codes of MI300.  ldq % 16 == 0 and
 *         K % 16 == 0: a lane's unit is one 16-byte load of 16 weights.
 *   scale fp32 [N]; weight (n, k) stands for scale[n] * e4m3(W8[n][k]).
 *   The codes 0x7F and 0xFF are NaN.  The quantiser never emits them; a GEMM that reads one may produce NaN.
 *
 * Quantiser, reproducible bit for bit: per row n of W (bf16 [N][ldw], ldw % 8 == 0), amax = max_k |W[n][k]| exactly;
 * scale[n] = amax / 448 and t = W[n][k] / scale[n], both correctly rounded fp32 divisions; code = e4m3(clamp(t, -448, 448)),
 * round to nearest even.  An all-zero row gets scale 1 and codes 0.  Writes [N][K] of W8 and [N] of scale, nothing else. */
int kalle_quantize_rows_e4m3(const void* W, int64_t ldw, void* W8, int64_t ldq, float* scale, int N, int K, void* stream);
/* kalle_gemv_bf16 on such weights: y[n] = scale[n] * (fp32 sum over k of e4m3(W8[n][k]) * x[k]) (+ residual[n]); x bf16 [K],
 * y bf16 or fp32 [N], residual fp32 [N] or NULL; K % 16 == 0, ldq % 16 == 0, K <= 32768 (x is kept in LDS as bf16).  The
 * products are exact in fp32 (4 significant bits times 8); the order of the sum is unspecified but fixed. */
int kalle_gemv_e4m3(const void* x, const void* W8, int64_t ldq, const float* scale, void* y, int y_dtype,
                    const float* residual, int N, int K, void* stream);
/* The form the one-row step uses: the prologues of kalle_gemm_rows_fused for one row, built inside the kernel (no scratch) with
 * the expressions of the bf16 step's GEMV - KALLE_PRO_BF16 x bf16 [K]; KALLE_PRO_RMS x fp32 [K], gamma fp32 [K];
 * KALLE_PRO_SWIGLU x bf16 [2K] = up | gate - and a second destination: outputs n >= nsplit go to y2[n - nsplit] (y's dtype;
 * nsplit = N: none, y2 may be NULL).  It has no bf16 counterpart and no Python wrapper: it is the step's internal launcher with
 * argument checks, exported so that the tests can drive each prologue and the second destination of the kernel alone; a caller
 * wants kalle_gemv_e4m3 or the steps below. */
int kalle_gemv_fused_e4m3(const void* x, int prologue, const float* gamma, float eps, const void* W8, int64_t ldq,
                          const float* scale, void* y, int y_dtype, void* y2, int nsplit, const float* residual, int N, int K,
                          void* stream);
/* kalle_gemm_rows_fused with W8, ldq and scale in place of W and ldw: the same kernel structure, the weight fragment widened from
 * e4m3 to bf16 in registers (exact) in front of the same v_mfma_f32_16x16x32_bf16, activations bf16, scale[n] applied where
 * output (r, n) is written.  Prologues, xhat, nsplit / y2 / y2_off, residual and active as there; K % 16 == 0, ldq % 16 == 0,
 * K <= 32768, 1 <= R <= 16. */
int kalle_gemm_rows_fused_e4m3(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat,
                               const void* W8, int64_t ldq, const float* scale, void* y, int64_t ldy, int y_dtype, void* y2,
                               int nsplit, const int64_t* y2_off, const float* residual, int64_t ldres, const int32_t* active,
                               int R, int N, int K, void* stream);
/* kalle_llama_decode_step_hd and kalle_llama_decode_step_rows on e4m3 weights: the arguments, the per-layer sequence, the
 * attention calls, the workspace layout and size (kalle_llama_decode_ws_bytes_hd / kalle_llama_decode_ws_bytes_rows serve both)
 * and the refusals of those two, plus D % 16 != 0 (no supported head dim has it) and inner % 16 != 0.  Weights: uint8 row-major
 * with row stride K ([out][in]; wqkv = [q;k;v], wug = [up;gate]), each with its fp32 scale per output row; norm weights and the
 * KV cache as in kalle_llama_layer.  Every launch is checked where it is made. */
typedef struct kalle_llama_layer_w8 {
    const float* input_norm;
    const void* wqkv;
    const float* sqkv;
    const void* wo;
    const float* so;
    const float* post_norm;
    const void* wug;
    const float* sug;
    const void* wdown;
    const float* sdown;
    void* kv_cache;
} kalle_llama_layer_w8;
int kalle_llama_decode_step_w8(const kalle_llama_layer_w8* layers, int n_layers, const float* x, float* out, int H, int Hkv,
                               int inner, int head_dim, float eps, int t0, int cache_rows, const float* rope_cos,
                               const float* rope_sin, void* workspace, void* stream);
int kalle_llama_decode_step_rows_w8(const kalle_llama_layer_w8* layers, int n_layers, const float* x, float* out, int R, int H,
                                    int Hkv, int inner, int head_dim, float eps, const int32_t* t0, int cache_rows,
                                    const float* rope_cos, const float* rope_sin, void* workspace, void* stream);
/* ---- the per-frame head of KV-cached generation (model_sigmaVAE.py:123-146): everything between two decode steps, one call ----
 * For each active row r of the R rows, from h = the UN-NORMED residual stream (`out` of kalle_llama_decode_step*, or the last
 * position of a prefill before model.norm), fp32 [R][ldh >= D]:
 *   xn     = bf16(rmsnorm(h[r]; norm, eps))                                    (LlamaRMSNorm, the rounding of kalle_rmsnorm_fwd)
 *   h1     = W1 . xn + b1                            fp32 [dl]                 distribution_linear[0]
 *   a      = bf16(gelu(h1))                                                    the exact GELU of kalle_gelu_fwd (one device function)
 *   mean   = W2 . a + b2                             fp32 [R][dl]              distribution_linear[2]
 *   latent = mean + std * noise[r]                   fp32 [R][dl]              sample(), noise fp32 [R][ldn >= dl]
 *   kl[r]  = (1/dl) sum_j [ log(e/std) + (std^2 + (mean_j - 1)^2) / (2 e^2) - 1/2 ]     KL(N(mean, std) || N(1, e)) / dl (:135-139)
 *   x_next = Wa . bf16(latent) + ba                  fp32 [R][D]               audio_linear: the next decode step's input
 * bf16 roundings at exactly the three marked points (those of a host path whose Linear casts its input to bf16); all else fp32.
 * Four launches: the RMSNorm pre-pass and the R-row GEMM of kalle_gemm_rows_fused for W1 (bias = residual at row stride 0), one
 * kernel with a workgroup per active row for GELU, W2, the sample and the KL (its terms summed in a fixed order), the R-row GEMM
 * for Wa.  No atomics, no workgroup waits on another: two calls on the same input give the same bits, and an active row's bits
 * do not depend on which other rows are active.  active: HOST int32 [R], 0 = row r is INACTIVE - nothing of it is read or
 * written, in the outputs or the workspace; NULL = every row active (as in kalle_gemm_rows_fused).  Every row inactive:
 * KALLE_OK, nothing launched.
 * Limits: 1 <= R <= KALLE_DECODE_MAX_ROWS; D % 8 == 0, 8 <= D <= 32768; dl % 8 == 0, 8 <= dl <= 512 (one workgroup streams the
 * dl x dl matrix per row: 512 KiB at the bound); std > 0; ldh % 4 == 0, ldh >= D; ldn >= dl; ldw* % 8 == 0 and not below the
 * row they hold.  Anything else, or a NULL argument or descriptor field other than active / stream, returns KALLE_ERR_ARG
 * before the first HIP call.  Every launch is checked where it is made.
 * Workspace (kalle_llasa_head_ws_bytes(R, D, dl) bytes, 64-byte aligned, caller-owned; KALLE_ERR_ARG outside the limits), in
 * this order, each region padded to a multiple of 64 bytes, rows dense:
 *   xn bf16 [R][D] | h1 fp32 [R][dl] | a bf16 [R][dl] | lat bf16 [R][dl] (= bf16(latent))
 * They are published so that every stage can be checked from its own inputs. */
typedef struct kalle_llasa_head {
    const float* norm;                 /* final RMSNorm weight, fp32 [D] */
    const void* w1; const float* b1;   /* distribution_linear[0]: bf16 [dl][ldw1 >= D], fp32 [dl] */
    const void* w2; const float* b2;   /* distribution_linear[2]: bf16 [dl][ldw2 >= dl], fp32 [dl] */
    const void* wa; const float* ba;   /* audio_linear:           bf16 [D][ldwa >= dl],  fp32 [D]  */
    int64_t ldw1, ldw2, ldwa;
} kalle_llasa_head;
int kalle_llasa_head_ws_bytes(int R, int D, int dl);
int kalle_llasa_frame_head_rows(const kalle_llasa_head* head, const float* h, int64_t ldh, const float* noise, int64_t ldn,
                                float std, float eps, float* mean, float* latent, float* kl, float* x_next,
                                const int32_t* active, int R, int D, int dl, void* workspace, void* stream);
/* ---- the same for the head that predicts its scale (model.py:109-150; infer_0828_sigma.py:319-323): mean || log-scale ----------
 * The descriptor is kalle_llasa_head with d2 = 2 * lat output rows in distribution_linear:
 *   w1 bf16 [d2][ldw1 >= D], b1 fp32 [d2];  w2 bf16 [d2][ldw2 >= d2], b2 fp32 [d2];  wa bf16 [D][ldwa >= lat], ba fp32 [D].
 * For each active row r of the R rows, from h = the UN-NORMED residual stream, fp32 [R][ldh >= D]:
 *   xn     = bf16(rmsnorm(h[r]; norm, eps))                                    (as above)
 *   h1     = W1 . xn + b1                            fp32 [d2]                 distribution_linear[0]
 *   a      = bf16(gelu(h1))                                                    the exact GELU of kalle_gelu_fwd (one device function)
 *   disp   = W2 . a + b2                             fp32 [R][d2]              distribution_linear[2]: mean = disp[:lat],
 *                                                                              logs = disp[lat:] - what `infer` stacks and returns
 *   s      = exp(logs)                               fp32 [R][lat]             (expf of this build)
 *   latent = mean + s * noise[r]                     fp32 [R][lat]             noise fp32 [R][ldn >= lat]
 *   kl[r]  = (1/lat) sum_j [ (1 - logs_j) + (s_j^2 + (mean_j - 1)^2) / (2 e^2) - 1/2 ]   KL(N(mean, s) || N(1, e)) / lat (:133-136)
 *   x_next = Wa . bf16(latent) + ba                  fp32 [R][D]               audio_linear: the next decode step's input
 * bf16 roundings at exactly the three marked points; all else fp32.  There is no std argument.
 * Four launches, as above: the RMSNorm pre-pass and the R-row GEMM for W1, one kernel with a workgroup per active row for GELU,
 * W2, exp, the sample and the KL, the R-row GEMM for Wa.  In the middle kernel rows j and j + lat of the W2 walk are finished
 * by different lanes (at d2 = 512 in different passes), so disp goes through LDS and a second phase after a barrier computes
 * s, latent, bf16(latent) and the KL terms, which one wave sums in a fixed order.  No atomics, no workgroup reads what another
 * writes: two calls on the same input give the same bits, and an active row's bits do not depend on which other rows are
 * active.  active: HOST int32 [R] as above - nothing of an inactive row is read or written, in the outputs or the workspace;
 * NULL = every row active.  Every row inactive: KALLE_OK, nothing launched.
 * Limits: 1 <= R <= KALLE_DECODE_MAX_ROWS; D % 8 == 0, 8 <= D <= 32768; lat % 8 == 0, 8 <= lat <= 256 (d2 <= 512: one workgroup
 * streams the d2 x d2 matrix per row, 512 KiB at the bound); ldh % 4 == 0, ldh >= D; ldn >= lat; ldw* % 8 == 0 and not below
 * the row they hold (D, d2, lat).  Anything else, or a NULL argument or descriptor field other than active / stream, returns
 * KALLE_ERR_ARG before the first HIP call.  Every launch is checked where it is made.
 * Workspace (kalle_llasa_head2_ws_bytes(R, D, lat) bytes, 64-byte aligned, caller-owned; KALLE_ERR_ARG outside the limits), in
 * this order, each region padded to a multiple of 64 bytes, rows dense:
 *   xn bf16 [R][D] | h1 fp32 [R][d2] | a bf16 [R][d2] | s fp32 [R][lat] | lat bf16 [R][lat] (= bf16(latent))
 * They are published so that every stage can be checked from its own inputs. */
int kalle_llasa_head2_ws_bytes(int R, int D, int lat);
int kalle_llasa_frame_head2_rows(const kalle_llasa_head* head, const float* h, int64_t ldh, const float* noise, int64_t ldn,
                                 float eps, float* disp, float* latent, float* kl, float* x_next, const int32_t* active, int R,
                                 int D, int lat, void* workspace, void* stream);
/* waveform -> int16 PCM as the inference scripts write it (infer_0723.py:293): out = int16(clamp(x / max|x|, -1, 1) * 32767);
 * peak: one fp32 of device scratch that receives max|x|; x fp32 or bf16 */
int kalle_peak_normalize_int16(const void* x, int dtype, float* peak, int16_t* out, int64_t n, void* stream);
/* out[r, :] = audio[r, :] * audio_mask[r] + table[ids[r], :] * ids_mask[r]   (embed_tokens + masked mix, :66-73);
 * table fp32 [vocab][D], audio fp32 or bf16 [rows][D], masks fp32 [rows], out fp32.  A row whose ids_mask is 0 contributes
 * exactly 0 from the table and its id is NOT read as an index (padding ids such as -100 lie outside the table); a row whose
 * audio_mask is 0 does not read its audio row (which may hold anything, NaN included).  Ids of rows that are read are clamped
 * to [0, vocab).  D % 4 == 0. */
int kalle_embed_mix_fwd(const int64_t* ids, const float* table, const void* audio, int audio_dtype, const float* ids_mask,
                        const float* audio_mask, float* out, int64_t rows, int D, int64_t vocab, void* stream);
/* daudio = dout * audio_mask (if daudio); dtable[ids[r], :] += dout[r, :] * ids_mask[r] (if dtable; fp32 atomics) */
int kalle_embed_mix_bwd(const float* dout, const int64_t* ids, const float* ids_mask, const float* audio_mask,
                        float* dtable, float* daudio, int64_t rows, int D, int64_t vocab, void* stream);
/* exact (erf) GELU, nn.GELU() default (model_sigmaVAE.py:46) */
int kalle_gelu_fwd(const void* x, void* y, int dtype, int64_t n, void* stream);
int kalle_gelu_bwd(const void* dy, const void* x, void* dx, int dtype, int64_t n, void* stream);
/* masked fixed-sigma Gaussian KL (model_sigmaVAE.py:85-95): kl[r] = sum_c (pred - label)^2 / (2 std^2) / dim;
 * sums4 (zeroed by the caller) += {sum kl*mask_a, sum mask_a, sum kl*mask_b, sum mask_b}; the two losses are
 * sums4[0]/sums4[1] and sums4[2]/sums4[3].  bwd: dpred for upstream gradients grad_a / grad_b (device scalars). */
int kalle_gauss_kl_fwd(const float* pred, const float* label, const float* mask_a, const float* mask_b, float* sums4,
                       float std, int64_t rows, int dim, void* stream);
int kalle_gauss_kl_bwd(const float* pred, const float* label, const float* mask_a, const float* mask_b,
                       const float* sums4, const float* grad_a, const float* grad_b, float* dpred, float std,
                       int64_t rows, int dim, void* stream);

/* masked two-Gaussian KL of the Stable-Audio-VAE task model (model.py:84-100):
 *   kl[r] = sum_c KL( N(m1, s1) || N(m2, exp(l2)) ) / dim,   m2 | l2 = the halves of pred [rows][2 dim] (model.py:89-90)
 * label_mode 0: label_mean / label_std [rows][dim] hold the label statistics (the transform of model.py:84 already applied
 * by the caller); label_mode 1: label_mean is the raw label [rows][2 dim] = mean | scale and std = softplus(scale) + 1e-4
 * (label_std unused).  std is multiplied by std_mult (1.25, model.py:87).  sums4 / grad_a / grad_b as kalle_gauss_kl_*;
 * dpred [rows][2 dim]. */
int kalle_gauss_kl2_fwd(const float* pred, const float* label_mean, const float* label_std, int label_mode, float std_mult,
                        const float* mask_a, const float* mask_b, float* sums4, int64_t rows, int dim, void* stream);
int kalle_gauss_kl2_bwd(const float* pred, const float* label_mean, const float* label_std, int label_mode, float std_mult,
                        const float* mask_a, const float* mask_b, const float* sums4, const float* grad_a,
                        const float* grad_b, float* dpred, int64_t rows, int dim, void* stream);

/* ---- backward of the VAE conv stacks (training the pretransform: `enable_grad`, models/factory.py:77-80; the reference
 * leaves it to torch autograd).  A fused forward unit is y = conv(act(x)) (+ residual) (-> tanh).
 * Data gradient: the forward entry points over dy with weights re-packed by kalle_weight_norm_fold -
 *   stride-1 Conv1d:   kalle_conv1d_fwd(dy, fold(v, g, 1 | 2), K, stride 1, padding (K-1)*dil - pad, dil)
 *   strided Conv1d:    kalle_conv_transpose1d_fwd(dy, fold(v, g, 1), K, stride, padding)
 *   ConvTranspose1d:   kalle_conv1d_fwd(dy, fold(v, g, 0), K, stride, padding)
 * Weight gradient (fp32, position reduction on the vector ALU, added atomically into dW which the caller zeroes):
 *   dW[cu][cv][k] += sum_{b, m} U[b, cu, m] * V[b, cv, m*stride - padding + k*dilation]
 *   Conv1d: U = dy [B][Cout][Lout], V = x [B][Cin][Lin]  -> dW in the module's [Cout][Cin][K] layout (act_on 0)
 *   ConvTranspose1d: U = x [B][Cin][Lin], V = dy [B][Cout][Lout] -> dW [Cin][Cout][K]            (act_on 1)
 *   `act` (code 0 / 1 SnakeBeta / 2 ELU) is the conv's INPUT activation, applied on the fly to x = V (act_on 0) or U (1).
 *   With the activation on V (or none), >= 16 V channels and 1 / 4 / 7 / 8 / 16 taps the LDS-staged kernel runs (the V span of a
 *   position tile staged and activated once, U as scalar operands); a transposed conv's caller passes act(x) as U with act 0. */
int kalle_conv_wgrad(const float* U, const float* V, float* dW, int B, int CU, int CV, int MU, int LV, int ksize, int stride,
                     int padding, int dilation, int act_on, const kalle_act* act, void* stream);
/* dx = g * act'(x) for x, g [B][C][L] fp32; SnakeBeta (blocks.py:301-339) also adds d alpha, d beta [C] atomically
 * (through the exp when logscale); act codes 0 / 1 / 2 */
int kalle_act_bwd(const float* x, const float* g, float* dx, const kalle_act* act, float* dalpha, float* dbeta, int B, int C,
                  int L, void* stream);
/* g = dy * (1 - y^2): the decoder's final tanh (autoencoders.py:185) */
int kalle_tanh_bwd(const float* dy, const float* y, float* g, int64_t n, void* stream);
/* nn.Upsample(scale_factor=scale, mode="nearest") along the last axis (DecoderBlock use_nearest_upsample, autoencoders.py:87-89):
 * backward == 0: x [rows][L] -> y [rows][L*scale], y[r][l] = x[r][l / scale];
 * backward != 0: x = dy [rows][L*scale] -> y = dx [rows][L], dx[r][m] = sum_{j<scale} dy[r][m*scale + j].  fp32, scale 1..64 */
int kalle_upsample_nearest(const float* x, float* y, int64_t rows, int L, int scale, int backward, void* stream);
/* out[c] += sum_{b, l} x[b][c][l]  (bias gradient; out zeroed or accumulated by the caller) */
int kalle_channel_sum(const float* x, float* out, int B, int C, int L, void* stream);
/* torch weight_norm (dim 0) backward: w = g v / ||v|| per slice of dim 0 (n = elements per slice):
 * dg = <dw, v> / ||v||, dv = g / ||v|| (dw - v <dw, v> / ||v||^2); accumulate != 0 adds to dv / dg */
int kalle_weight_norm_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int d0, int n,
                          int accumulate, void* stream);

/* anti-aliased periodic activation (alias-free-torch `Activation1d`, third-party, used by the mel-VAE decoder,
 * backup/flows.py:266-279,452-456): 2x kaiser-sinc FIR upsample (12 taps, replicate pad) -> x + sin^2(x a)/(b+1e-9)
 * -> 2x FIR low-pass downsample.  x, y: (B, C, L) fp32 or bf16; filter12: the 12 fp32 taps.  alpha == beta == NULL: ELU in
 * place of the snake (Oobleck units built with antialias_activation=True and use_snake=False, autoencoders.py:24-37). */
int kalle_act1d_fwd(const void* x, void* y, int dtype, const float* filter12, const float* alpha, const float* beta,
                    int logscale, int B, int C, int L, void* stream);
/* standalone SnakeBeta: y = x + sin^2(x e^alpha) / (e^beta + 1e-9)     (blocks.py:301-339) */
int kalle_snake_beta_fwd(const void* x, void* y, int dtype, const float* alpha, const float* beta, int logscale,
                         int B, int C, int L, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Off-default options of the DiT's transformer (none is set by the configs the reference ships)
 */
/* x[b][i] += table[i], b < nbatch, i < n: the position-embedding add of ContinuousTransformer(use_sinusoidal_emb /
 * use_abs_pos_emb), transformer.py:796-797 (`x = x + self.pos_emb(x)`, one [seq][dim] table for every batch element).
 * fp32, n % 4 == 0, 16-byte aligned; in place on the residual stream */
int kalle_add_rows(float* x, const float* table, int64_t nbatch, int64_t n, void* stream);
/* depthwise convolution along the sequence of token-major activations - ConformerModule.depthwise_conv, transformer.py:564
 * (Conv1d(dim, dim, 17, groups = dim, padding = 8, bias = False) between two rearranges b n d <-> b d n, 576-578):
 *   y[b][n][c] = sum_k w[c][flip ? K-1-k : k] * x[b][n + k - pad][c]        (x = 0 outside 0 <= n + k - pad < N)
 * x: bf16 [B][N][D]; w: fp32 [D][K] (the parameter's [D][1][K]); y: fp32 or bf16 [B][N][D].  flip != 0 with
 * pad = K - 1 - padding is the data gradient (x = dy).  D even, K <= 32, B <= 65535 */
int kalle_dwconv1d_fwd(const void* x, const float* w, void* y, int y_dtype, int B, int N, int D, int K, int pad, int flip,
                       void* stream);
/* its weight gradient: dw[c][k] += sum_{b, n} dy[b][n][c] * x[b][n + k - pad][c]   (dy, x bf16; dw fp32 [D][K], atomically
 * ADDED into: zero it for a fresh sum) */
int kalle_dwconv1d_wgrad(const void* dy, const void* x, float* dw, int B, int N, int D, int K, int pad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KALLE_HIP_H */
