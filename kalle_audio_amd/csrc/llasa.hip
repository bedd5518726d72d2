// Kernels of the Llasa task model's head and tail (model_sigmaVAE.py:53-104) around the Llama decoder layers (which run on
// the shared GEMM / attention / RMSNorm kernels): fixed-sigma latent sampling, token-embedding gather mixed with the
// projected audio latents under the two row masks (+ its scatter-add backward), exact GELU, and the masked fixed-sigma
// Gaussian KL losses.  All HBM-bound: vectorised where rows are long, fp32 math.
#include <type_traits>

#include "common.h"
#include "../../include/kalle_hip.h"

namespace {

inline int grid_for(int64_t work_items, int block) {
    int64_t g = (work_items + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// out = a * x + b * y   (model_sigmaVAE.py:166: x = mean + std * randn_like(mean))
__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                    float* __restrict__ out, float a, float b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = a * x[i] + b * y[i];
}

// single-row GEMM for KV-cached decoding (model_sigmaVAE.py:122-146 with a cache): y[n] = sum_k W[n][k] x[k] (+ residual[n]).
// Pure weight streaming: a wave owns 2 weight rows, its lanes walk K in 16-byte chunks (x staged once per workgroup in
// LDS), shuffle-reduce, lane 0 writes.  8 rows per 256-thread workgroup -> N/8 workgroups keep every HBM channel busy.
// The LDS copy of x can be built on the fly so that the decode step needs no separate norm / activation launches:
//   PRO_RMS:    x fp32 [K] -> bf16(x * (gamma * rsqrt(mean(x^2) + eps)))   (LlamaRMSNorm, same rounding as rms_fwd_kernel)
//   PRO_SWIGLU: x bf16 [2K] = [up | gate] -> bf16(up * silu(gate))         (LlamaMLP, same rounding as swiglu_fwd_kernel)
// Rows >= nsplit go to y2 (the k | v part of the fused qkv projection lands directly in its KV-cache row).
enum { PRO_BF16 = 0, PRO_RMS = 1, PRO_SWIGLU = 2 };

// The bf16 operand row xs[K] of a projection, built by the NT threads of a workgroup from xin (PRO_BF16: a copy).  The one
// routine behind the GEMVs (into LDS) and the R-row pre-pass (into xhat): one set of expressions, so one set of rounding points.
// The caller puts the barrier between these stores and its reads.
template <int PRO, int NT>
__device__ __forceinline__ void x_prologue(const void* __restrict__ xin, const float* __restrict__ gamma, float eps, bf16_t* xs,
                                           int K) {
    if constexpr (PRO == PRO_BF16) {
        const bf16_t* x = static_cast<const bf16_t*>(xin);
        for (int i = threadIdx.x; i < (K >> 3); i += NT)
            reinterpret_cast<i32x4*>(xs)[i] = reinterpret_cast<const i32x4*>(x)[i];
    } else if constexpr (PRO == PRO_RMS) {
        __shared__ float red[NT / 64];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const float* x = static_cast<const float*>(xin);
        float q = 0.f;
        for (int i = threadIdx.x; i < (K >> 2); i += NT) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
            q += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
        q = wave_sum(q);
        if (lane == 0) red[wave] = q;
        __syncthreads();
        float ss = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) ss += red[w];
        const float rr = rsqrtf(ss / (float)K + eps);
        for (int i = threadIdx.x; i < (K >> 2); i += NT) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
            const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[i];
            i32x2 o;
            o[0] = (int)pack_bf16x2(v[0] * (g[0] * rr), v[1] * (g[1] * rr));
            o[1] = (int)pack_bf16x2(v[2] * (g[2] * rr), v[3] * (g[3] * rr));
            reinterpret_cast<i32x2*>(xs)[i] = o;
        }
    } else {
        const bf16_t* h = static_cast<const bf16_t*>(xin);
        for (int i = threadIdx.x; i < (K >> 3); i += NT) {
            const i32x4 xv = reinterpret_cast<const i32x4*>(h)[i];
            const i32x4 gv = reinterpret_cast<const i32x4*>(h + K)[i];
            i32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = (int)pack_bf16x2(bf16lo((uint32_t)xv[j]) * siluf_(bf16lo((uint32_t)gv[j])),
                                        bf16hi((uint32_t)xv[j]) * siluf_(bf16hi((uint32_t)gv[j])));
            reinterpret_cast<i32x4*>(xs)[i] = o;
        }
    }
}

template <bool YF32, int PRO>
__global__ __launch_bounds__(256) void gemv_kernel(const void* __restrict__ xin, const float* __restrict__ gamma, float eps,
                                                   const bf16_t* __restrict__ W, int64_t ldw, void* __restrict__ y,
                                                   void* __restrict__ y2, int nsplit, const float* __restrict__ res,
                                                   int N, int K, int rpw) {
    extern __shared__ __attribute__((aligned(16))) char gsm[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(gsm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the weight stream does not depend on x: the first PF chunks of both rows are in flight while x is being prepared.
    // A wave walks `rpw` row pairs (rows ((blockIdx * rpw + p) * 4 + wave) * 2 + {0, 1}); its work is the flat sequence
    // of (pair, K batch) items, each item's loads issued one item ahead of its FMAs.
    constexpr int PF = 4;
    const int nc = K >> 3;
    const int NB = (nc + 64 * PF - 1) / (64 * PF);
    const int T = rpw * NB;
    auto load = [&](int pr, int bb, i32x4* uu, i32x4* vv) {
        const int n = ((blockIdx.x * rpw + pr) * 4 + wave) * 2;
        const bf16_t* r0 = W + (int64_t)(n < N ? n : N - 1) * ldw;
        const bf16_t* r1 = W + (int64_t)(n + 1 < N ? n + 1 : N - 1) * ldw;
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int c = bb * (64 * PF) + lane + 64 * j;
            const int cc = c < nc ? c : nc - 1;
            uu[j] = *reinterpret_cast<const i32x4*>(r0 + 8 * cc);
            vv[j] = *reinterpret_cast<const i32x4*>(r1 + 8 * cc);
        }
    };
    i32x4 u[PF], v[PF];
    load(0, 0, u, v);
    x_prologue<PRO, 256>(xin, gamma, eps, xs, K);
    __syncthreads();
    float a0 = 0.f, a1 = 0.f;
    int pr = 0, bb = 0;
    for (int t = 0; t < T; ++t) {
        i32x4 un[PF], vn[PF];
        const bool more = t + 1 < T;
        const int npr = bb + 1 == NB ? pr + 1 : pr, nbb = bb + 1 == NB ? 0 : bb + 1;
        if (more) load(npr, nbb, un, vn);
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int c = bb * (64 * PF) + lane + 64 * j;
            if (c < nc) {
                const i32x4 xv = reinterpret_cast<const i32x4*>(xs)[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = bf16lo((uint32_t)xv[e]), x1 = bf16hi((uint32_t)xv[e]);
                    a0 += bf16lo((uint32_t)u[j][e]) * x0 + bf16hi((uint32_t)u[j][e]) * x1;
                    a1 += bf16lo((uint32_t)v[j][e]) * x0 + bf16hi((uint32_t)v[j][e]) * x1;
                }
            }
        }
        if (bb + 1 == NB) {   // row pair done
            const int n0 = ((blockIdx.x * rpw + pr) * 4 + wave) * 2;
            a0 = wave_sum(a0);
            a1 = wave_sum(a1);
            if (lane == 0 && n0 < N) {
                const bool two = n0 + 1 < N;
                if (res) { a0 += res[n0]; if (two) a1 += res[n0 + 1]; }
                // nsplit is even (a multiple of 64 in practice), so a wave's two rows never straddle it
                void* yo = n0 < nsplit ? y : y2;
                const int r0 = n0 < nsplit ? n0 : n0 - nsplit;
                if constexpr (YF32) {
                    static_cast<float*>(yo)[r0] = a0;
                    if (two) static_cast<float*>(yo)[r0 + 1] = a1;
                } else {
                    static_cast<bf16_t*>(yo)[r0] = f32_to_bf16(a0);
                    if (two) static_cast<bf16_t*>(yo)[r0 + 1] = f32_to_bf16(a1);
                }
            }
            a0 = a1 = 0.f;
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < PF; ++j) { u[j] = un[j]; v[j] = vn[j]; }
        }
        pr = npr; bb = nbb;
    }
}

// ---- R-row GEMM for batched decoding: Y[r][n] = sum_k W[n][k] X[r][k] (+ residual[r][n]), 1 <= R <= 64 -------------------------
// Still pure weight streaming: W is read from HBM once for all rows.  A workgroup owns TR weight rows and every row of the batch:
// v_mfma_f32_16x16x32_bf16 with the weight rows on the M side and the batch on the 16-wide N side in NCB = ceil(R / 16) column
// blocks, rows >= R or inactive held at zero.  The dot product over k does not care which k a lane supplies as long as A and B
// agree, so lane (row i, group g) supplies the SAME 16-byte chunk of weight row i (A) and of batch rows i, 16 + i, ... (B, one
// per column block): the weight chunk a lane loaded feeds NCB MFMAs, both operands come straight from global memory in the
// layout the instruction wants, and X needs no LDS at any K (16 rows x 32768 x 2 B would be 1 MiB against the CU's 160 KiB).
// One load instruction covers 64 contiguous bytes of each weight row (the four groups side by side), eight consecutive ones a
// 512-byte run.  X is R x K x 2 bytes out of L2 per workgroup.
// Accumulation, per (weight row, batch row) pair and whatever R, TR, NCB, the row's index or the other rows (an MFMA output
// element depends on its own row of A and column of B only): wave w takes the 256-element K blocks w, w + 4, ..., the eight
// chunks of a block go through one accumulator in order, and the four waves' partial tiles meet in LDS (4 KiB per column
// block) as (p0 + p1) + (p2 + p3) in rows_output.  So a row's bits are the same at every R.
// Schedule: the loads of the next unit are issued before the MFMAs of the current one.  Up to 16 rows (NCB = 1) the unit is a
// whole K block (8 weight + 8 X chunk registers, twice: 202 VGPRs as compiled); above, HALF a block (4 weight + 4 NCB X, twice:
// 136 / 172 - 176 / 212 - 216 VGPRs at NCB = 2 / 3 / 4), where whole blocks double-buffered would need about 320 by count.
// Tile: up to 16 rows TR = 8 for N < 8192 (the upper M half of the tile stays zero: the MFMA is idle anyway) and 16 from there,
// so the grid is N / 8 workgroups where the one-row kernel has N / 8 (every decoder GEMM but up|gate: 256 - 640 workgroups at
// the 1B / 3B shapes on 256 CUs) and N / 16 where it has N / 16 or N / 32; above 16 rows wide_tile_rows below.
// The RMSNorm / SwiGLU prologues cannot be rebuilt per workgroup here the way the one-row kernel does it: each of the N / 8
// or N / 16 workgroups would re-read R x K fp32 from L2 (qkv at the 3B shape: 640 x 192 KiB = 120 MiB against 31 MiB of weights) and redo
// R row norms.  rows_prologue_kernel writes the bf16 operand once per GEMM instead (R x K x 2 bytes, one short launch), through
// x_prologue like the one-row kernels.

// The rows of a batch as the host keeps them: one form for every R.
struct RowSet {
    int64_t y2_off[KALLE_DECODE_WIDE_MAX_ROWS];   // element offset into y2 of row r's second destination
    uint64_t active;                              // bit r: row r takes part
    int R;
};

// ... and as a kernel takes them, by value: MAXR = 16 (136 bytes of kernel arguments, a 32-bit mask) or 64 (528, 64-bit)
template <int MAXR>
struct RowArgs {
    static_assert(MAXR == KALLE_DECODE_MAX_ROWS || MAXR == KALLE_DECODE_WIDE_MAX_ROWS, "the two row bounds of the ABI");
    using Mask = std::conditional_t<(MAXR > 32), uint64_t, unsigned>;
    int64_t y2_off[MAXR];
    Mask active;
    int R;
    explicit RowArgs(const RowSet& s) : active((Mask)s.active), R(s.R) {      // (s.R <= MAXR: proj_launch picks MAXR by s.R)
        for (int r = 0; r < MAXR; ++r) y2_off[r] = s.y2_off[r];
    }
};

template <int PRO, class MaskT>
__global__ __launch_bounds__(256) void rows_prologue_kernel(const void* __restrict__ xall, int64_t ldx,
                                                            const float* __restrict__ gamma, float eps,
                                                            bf16_t* __restrict__ xhat, int64_t ldh, int K, MaskT active) {
    static_assert(PRO == PRO_RMS || PRO == PRO_SWIGLU, "PRO_BF16 has no pre-pass");
    const int r = blockIdx.x;
    if (!(active >> r & 1)) return;
    if constexpr (PRO == PRO_RMS) x_prologue<PRO, 256>(static_cast<const float*>(xall) + r * ldx, gamma, eps, xhat + r * ldh, K);
    else x_prologue<PRO, 256>(static_cast<const bf16_t*>(xall) + r * ldx, gamma, eps, xhat + r * ldh, K);
}

// The output stage of the R-row GEMMs, after the barrier behind the waves' partial tiles (lane (i16, g) of column block b wrote
// weight rows n0 + 4 g + {0 .. 3} of batch row 16 b + i16): thread t owns output (row t / TR, column t % TR), then 256 further.
// The partials summed in the fixed order, times scale[n] (SCALED: the e4m3 weights), plus the residual; columns >= nsplit go to
// y2 at the row's y2_off.
template <bool YF32, int TR, int NCB, bool SCALED, class MaskT>
__device__ __forceinline__ void rows_output(const float (*part)[NCB][64][4], const float* __restrict__ scale, void* __restrict__ y,
                                           int64_t ldy, void* __restrict__ y2, int nsplit, const float* __restrict__ res,
                                           int64_t ldres, int n0, int N, int R, MaskT active, const int64_t* y2_off) {
    auto store = [&](int idx) {
        const int r = idx / TR, j = idx % TR, n = n0 + j;
        if (r < R && (active >> r & 1) && n < N) {
            const int b = r >> 4, src = (j >> 2) * 16 + (r & 15), e = j & 3;
            float s = (part[0][b][src][e] + part[1][b][src][e]) + (part[2][b][src][e] + part[3][b][src][e]);
            if constexpr (SCALED) s *= scale[n];
            if (res) s += res[r * ldres + n];
            const int64_t at = n < nsplit ? r * ldy + n : y2_off[r] + (n - nsplit);
            void* yo = n < nsplit ? y : y2;
            if constexpr (YF32) static_cast<float*>(yo)[at] = s;
            else static_cast<bf16_t*>(yo)[at] = f32_to_bf16(s);
        }
    };
    // (one pass needs no bound on idx: R <= 16 NCB rows)
    if constexpr (16 * NCB * TR <= 256) store(threadIdx.x);
    else
        for (int idx = threadIdx.x; idx < 16 * NCB * TR; idx += 256) store(idx);
}

template <bool YF32, int TR, int NCB>
__global__ __launch_bounds__(256) void gemm_rows_kernel(const bf16_t* __restrict__ X, int64_t ldx, const bf16_t* __restrict__ W,
                                                        int64_t ldw, void* __restrict__ y, int64_t ldy, void* __restrict__ y2,
                                                        int nsplit, const float* __restrict__ res, int64_t ldres, int N, int K,
                                                        RowArgs<(NCB == 1 ? KALLE_DECODE_MAX_ROWS : KALLE_DECODE_WIDE_MAX_ROWS)> a) {
    static_assert(TR == 8 || TR == 16, "weight rows per workgroup");
    static_assert(NCB >= 1 && NCB <= 4, "column blocks of 16 batch rows");
    __shared__ __attribute__((aligned(16))) float part[4][NCB][64][4];
    // 16-byte chunks per lane and K block (a block is 8 x 4 groups x 8 = 256 elements) / per pipelined unit; LU = log2(units per block)
    constexpr int CH = 8, HC = NCB == 1 ? 8 : 4, LU = NCB == 1 ? 0 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * TR;
    const bool wrow = TR == 16 || i16 < TR;                   // (TR = 8: M rows 8 .. 15 of the tile stay zero, nothing loaded)
    const int nc = K >> 3, NB = (nc + 4 * CH - 1) / (4 * CH);
    const int R = a.R;                            // (both read once, here with the other arguments, for the loads and rows_output)
    const auto active = a.active;
    bool live[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) live[b] = 16 * b + i16 < R && (active >> (16 * b + i16) & 1);
    const bf16_t* wr = W + (int64_t)(n0 + i16 < N ? n0 + i16 : N - 1) * ldw;
    const bf16_t* xr[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) xr[b] = X + (live[b] ? 16 * b + i16 : 0) * ldx;      // (not read unless live)
    // unit u of this wave: part (u & (1 << LU) - 1) of K block wave + 4 (u >> LU)
    auto load = [&](int u, i32x4* wq, i32x4 (*xq)[HC]) {
        const int c0 = ((wave + 4 * (u >> LU)) * CH + (u & ((1 << LU) - 1)) * HC) * 4 + g;
#pragma unroll
        for (int j = 0; j < HC; ++j) {
            const int c = c0 + 4 * j;
            const bool in = c < nc;
            const int cc = in ? c : nc - 1;
            wq[j] = i32x4{0, 0, 0, 0};                        // past K: a zero weight chunk against a chunk of x that exists
            if (wrow && in) wq[j] = *reinterpret_cast<const i32x4*>(wr + 8 * cc);
#pragma unroll
            for (int b = 0; b < NCB; ++b) {
                xq[b][j] = i32x4{0, 0, 0, 0};
                if (live[b]) xq[b][j] = *reinterpret_cast<const i32x4*>(xr[b] + 8 * cc);
            }
        }
    };
    f32x4 acc[NCB];
#pragma unroll
    for (int b = 0; b < NCB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int NU = wave < NB ? ((NB - wave + 3) / 4) << LU : 0;
    i32x4 wv[HC], xv[NCB][HC];
    if (NU) load(0, wv, xv);
    for (int u = 0; u < NU; ++u) {
        i32x4 wn[HC], xn[NCB][HC];
        const bool more = u + 1 < NU;
        if (more) load(u + 1, wn, xn);
#pragma unroll
        for (int j = 0; j < HC; ++j)
#pragma unroll
            for (int b = 0; b < NCB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv[j]),
                                                                 __builtin_bit_cast(bf16x8, xv[b][j]), acc[b], 0, 0, 0);
        if (more) {
#pragma unroll
            for (int j = 0; j < HC; ++j) {
                wv[j] = wn[j];
#pragma unroll
                for (int b = 0; b < NCB; ++b) xv[b][j] = xn[b][j];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NCB; ++b) *reinterpret_cast<f32x4*>(part[wave][b][lane]) = acc[b];
    __syncthreads();
    rows_output<YF32, TR, NCB, false>(part, nullptr, y, ldy, y2, nsplit, res, ldres, n0, N, R, active, a.y2_off);
}

// ---- weight-only OCP e4m3 decoding: W8 uint8 [N][ldq] codes, scale fp32 [N]; weight (n, k) = scale[n] * e4m3(W8[n][k]) -----------
// The decode step is weight streaming, so the one thing left to cut per frame is the bytes per weight.  v_cvt_pk_f32_fp8 turns
// two codes into two fp32 values; an e4m3 value (4 significant bits) times a bf16 value (8) is exact in fp32, so the only
// differences from the bf16 kernels above are the weights themselves, the fp32 summation order and one multiply by scale[n].

// a / b correctly rounded (the IEEE sequence the compiler emits for a precise fdiv): the library is built with -ffast-math, where
// `/` - and __fdiv_rn, which is `/` in this HIP - is v_rcp_f32 times the numerator, an ulp or so off
__device__ __forceinline__ float div_rn(float a, float b) {
    bool fd, fn;
    const float d = __builtin_amdgcn_div_scalef(a, b, false, &fd);
    const float n = __builtin_amdgcn_div_scalef(a, b, true, &fn);
    float r = __builtin_amdgcn_rcpf(d);
    r = __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
    float q = n * r;
    q = __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
    return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(__builtin_fmaf(-d, q, n), r, q, fn), b, a);
}

// per row: scale = max|w| / 448 (1 for an all-zero row), code = e4m3_rne(clamp(w / scale, +-448)), both divisions correctly
// rounded.  A wave per row, 4 rows per workgroup; a lane's unit is 16 weights in (two 16-byte loads), 16 codes out (one store).
__global__ __launch_bounds__(256) void quantize_rows_e4m3_kernel(const bf16_t* __restrict__ W, int64_t ldw,
                                                                 uint8_t* __restrict__ W8, int64_t ldq,
                                                                 float* __restrict__ scale, int N, int K) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const bf16_t* w = W + (int64_t)n * ldw;
    const int nc = K >> 4;
    float m = 0.f;
    for (int c = lane; c < nc; c += 64) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const i32x4 v = *reinterpret_cast<const i32x4*>(w + 16 * c + 8 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                m = fmaxf(m, fmaxf(fabsf(bf16lo((uint32_t)v[e])), fabsf(bf16hi((uint32_t)v[e]))));
        }
    }
    m = wave_max(m);
    const float s = m > 0.f ? div_rn(m, 448.f) : 1.f;
    if (lane == 0) scale[n] = s;
    for (int c = lane; c < nc; c += 64) {
        i32x4 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const i32x4 v = *reinterpret_cast<const i32x4*>(w + 16 * c + 8 * h);
            float t[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t[2 * e] = fminf(fmaxf(div_rn(bf16lo((uint32_t)v[e]), s), -448.f), 448.f);
                t[2 * e + 1] = fminf(fmaxf(div_rn(bf16hi((uint32_t)v[e]), s), -448.f), 448.f);
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                int word = __builtin_amdgcn_cvt_pk_fp8_f32(t[4 * p], t[4 * p + 1], 0, false);
                word = __builtin_amdgcn_cvt_pk_fp8_f32(t[4 * p + 2], t[4 * p + 3], word, true);
                o[2 * h + p] = word;
            }
        }
        *reinterpret_cast<i32x4*>(W8 + (int64_t)n * ldq + 16 * c) = o;
    }
}

// gemv_kernel on e4m3 weights: y[n] = scale[n] * sum_k e4m3(W8[n][k]) x[k] (+ residual[n]), the three prologues through
// x_prologue (the operand stays bf16 in LDS).
// Byte budget: a weight row is K bytes now, so 16 bytes of it hold 16 weights and 64 lanes x 16 bytes cover 1024 of them - at
// K = 2048 (every Llama-3.2-1B GEMV but down) a row is two loads per lane.  To keep gemv_kernel's 128 bytes per lane in flight
// (2 rows x 4 x 16 B) a wave owns FOUR rows and issues 2 x 16 B of each per item, one item ahead; a workgroup is two such waves
// (128 threads), so it still owns 8 rpw rows and the grid is gemv_kernel's for every N.  Vector ALU per 16-byte load: 8
// v_cvt_pk_f32_fp8 + 16 FMA (8 packed), and 16 unpacks of x shared by the four rows: 112 instructions per 64 weight bytes and lane
// against gemv_kernel's 40 per 32 - 1.4 x the ALU work per byte on half the bytes.
template <bool YF32, int PRO>
__global__ __launch_bounds__(128) void gemv_e4m3_kernel(const void* __restrict__ xin, const float* __restrict__ gamma, float eps,
                                                        const uint8_t* __restrict__ W8, int64_t ldq,
                                                        const float* __restrict__ scale, void* __restrict__ y,
                                                        void* __restrict__ y2, int nsplit, const float* __restrict__ res,
                                                        int N, int K, int rpw) {
    extern __shared__ __attribute__((aligned(16))) char gsm[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(gsm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PF = 2, RW = 4;                 // 16-byte loads per row and item; rows per wave
    const int nc = K >> 4;
    const int NB = (nc + 64 * PF - 1) / (64 * PF);
    const int T = rpw * NB;
    // a wave walks `rpw` row groups (rows ((blockIdx * rpw + p) * 2 + wave) * 4 + {0 .. 3}) as the flat sequence of (group, K
    // batch) items; rows past N and chunks past K re-read the last one (in bounds) and are not used
    auto load = [&](int pr, int bb, i32x4 (*q)[PF]) {
        const int n = ((blockIdx.x * rpw + pr) * 2 + wave) * RW;
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const uint8_t* r = W8 + (int64_t)(n + i < N ? n + i : N - 1) * ldq;
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int c = bb * (64 * PF) + lane + 64 * j;
                q[i][j] = *reinterpret_cast<const i32x4*>(r + 16 * (c < nc ? c : nc - 1));
            }
        }
    };
    i32x4 u[RW][PF];
    load(0, 0, u);
    x_prologue<PRO, 128>(xin, gamma, eps, xs, K);
    __syncthreads();
    f32x2 a[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) a[i] = f32x2{0.f, 0.f};
    int pr = 0, bb = 0;
    for (int t = 0; t < T; ++t) {
        i32x4 un[RW][PF];
        const bool more = t + 1 < T;
        const int npr = bb + 1 == NB ? pr + 1 : pr, nbb = bb + 1 == NB ? 0 : bb + 1;
        if (more) load(npr, nbb, un);
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int c = bb * (64 * PF) + lane + 64 * j;
            if (c < nc) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {          // 8 of the chunk's 16 operand elements at a time
                    const i32x4 xv = reinterpret_cast<const i32x4*>(xs)[2 * c + h];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const f32x2 x2 = {bf16lo((uint32_t)xv[e]), bf16hi((uint32_t)xv[e])};
#pragma unroll
                        for (int i = 0; i < RW; ++i) {
                            // word 2 h + (e >> 1) of the chunk, its low or high pair of codes
                            const int w = u[i][j][2 * h + (e >> 1)];
                            const f32x2 wf = (e & 1) ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true) : __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
                            a[i] += wf * x2;
                        }
                    }
                }
            }
        }
        if (bb + 1 == NB) {   // row group done
            const int n0 = ((blockIdx.x * rpw + pr) * 2 + wave) * RW;
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const float s = wave_sum(a[i][0] + a[i][1]);
                const int n = n0 + i;
                if (lane == 0 && n < N) {
                    float v = scale[n] * s;
                    if (res) v += res[n];
                    void* yo = n < nsplit ? y : y2;
                    const int at = n < nsplit ? n : n - nsplit;
                    if constexpr (YF32) static_cast<float*>(yo)[at] = v;
                    else static_cast<bf16_t*>(yo)[at] = f32_to_bf16(v);
                }
                a[i] = f32x2{0.f, 0.f};
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int j = 0; j < PF; ++j) u[i][j] = un[i][j];
        }
        pr = npr; bb = nbb;
    }
}

// gemm_rows_kernel on e4m3 weights: the same tile, grid, K split over the waves and LDS meeting point.  Lane (row i, group g)
// takes 16 bytes of weight row i - 16 weights, two of the MFMA's K chunks - widens them to bf16 in registers (exact: 4
// significant bits) and feeds v_mfma_f32_16x16x32_bf16 twice, each time against the 16-byte chunk of batch row i that holds the
// same k.  The activations stay bf16.  A K block is 256 elements as before: 4 weight loads and 8 x loads per lane.  scale[n] is
// applied in rows_output by the thread that owns output (r, n).
template <bool YF32, int TR>
__global__ __launch_bounds__(256) void gemm_rows_e4m3_kernel(const bf16_t* __restrict__ X, int64_t ldx,
                                                             const uint8_t* __restrict__ W8, int64_t ldq,
                                                             const float* __restrict__ scale, void* __restrict__ y, int64_t ldy,
                                                             void* __restrict__ y2, int nsplit, const float* __restrict__ res,
                                                             int64_t ldres, int N, int K, RowArgs<KALLE_DECODE_MAX_ROWS> a) {
    static_assert(TR == 8 || TR == 16, "weight rows per workgroup");
    __shared__ __attribute__((aligned(16))) float part[4][1][64][4];
    constexpr int CH = 4;                         // 16-byte weight loads per lane and K block: 4 x 4 groups x 16 = 256 elements
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * TR;
    const bool wrow = TR == 16 || i16 < TR;
    const int nc = K >> 4, NB = (nc + 4 * CH - 1) / (4 * CH);
    const int R = a.R;
    const unsigned active = a.active;
    const bool live = i16 < R && (active >> i16 & 1);
    const uint8_t* wr = W8 + (int64_t)(n0 + i16 < N ? n0 + i16 : N - 1) * ldq;
    const bf16_t* xr = X + (live ? i16 : 0) * ldx;            // (not read unless live)
    auto load = [&](int kb, i32x4* wq, i32x4* xq) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int c = (kb * CH + j) * 4 + g;
            const bool in = c < nc;
            const int cc = in ? c : nc - 1;
            wq[j] = i32x4{0, 0, 0, 0};                        // past K: zero codes (+0) against a chunk of x that exists
            if (wrow && in) wq[j] = *reinterpret_cast<const i32x4*>(wr + 16 * cc);
            xq[2 * j] = xq[2 * j + 1] = i32x4{0, 0, 0, 0};
            if (live) {
                xq[2 * j] = *reinterpret_cast<const i32x4*>(xr + 16 * cc);
                xq[2 * j + 1] = *reinterpret_cast<const i32x4*>(xr + 16 * cc + 8);
            }
        }
    };
    // codes -> bf16 pairs: v_cvt_pk_f32_fp8, then the (exact) rounding to bf16
    auto widen = [](int lo, int hi) {
        i32x4 o;
        f32x2 p = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
        o[0] = (int)pack_bf16x2(p[0], p[1]);
        p = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
        o[1] = (int)pack_bf16x2(p[0], p[1]);
        p = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
        o[2] = (int)pack_bf16x2(p[0], p[1]);
        p = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
        o[3] = (int)pack_bf16x2(p[0], p[1]);
        return o;
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    i32x4 wv[CH], xv[2 * CH];
    int kb = wave;
    if (kb < NB) load(kb, wv, xv);
    for (; kb < NB; kb += 4) {
        i32x4 wn[CH], xn[2 * CH];
        const bool more = kb + 4 < NB;
        if (more) load(kb + 4, wn, xn);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, widen(wv[j][0], wv[j][1])),
                                                          __builtin_bit_cast(bf16x8, xv[2 * j]), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, widen(wv[j][2], wv[j][3])),
                                                          __builtin_bit_cast(bf16x8, xv[2 * j + 1]), acc, 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < CH; ++j) { wv[j] = wn[j]; xv[2 * j] = xn[2 * j]; xv[2 * j + 1] = xn[2 * j + 1]; }
        }
    }
    *reinterpret_cast<f32x4*>(part[wave][0][lane]) = acc;
    __syncthreads();
    rows_output<YF32, TR, 1, true>(part, scale, y, ldy, y2, nsplit, res, ldres, n0, N, R, active, a.y2_off);
}

// ---- the one projection launcher: every GEMV and R-row GEMM of this file, public or inside the decode step, is launched here ---
struct Proj {
    const void* w;          // [N][ld]: bf16, or e4m3 codes when `scale` is set
    int64_t ld;
    const float* scale;     // fp32 [N] (e4m3) or NULL (bf16)
};

// f(std::bool_constant<flag>, std::integral_constant<int, v>) for the runtime pair; v must be one of Vs
template <int... Vs, class F>
inline void for_instance(bool flag, int v, F&& f) {
    auto on = [&](auto fl) { ((v == Vs ? (f(fl, std::integral_constant<int, Vs>{}), 0) : 0), ...); };
    if (flag) on(std::true_type{});
    else on(std::false_type{});
}

// Weight rows per workgroup of the wide GEMM.  X never goes through LDS, so a workgroup reads all of it from
// L2: 16 NCB x K x 2 bytes, (N / TR) times over - at TR = 8, 64 rows and the 1B down projection (N 2048, K 8192) 256 x 1 MiB
// against 32 MiB of weights from HBM.  16 weight rows halve that and put the MFMA's upper M half to work; what they cost is
// workgroups (N / 16).  Measured with both tiles forced at the eight decoder GEMMs of the 1B and 3B shapes, 32 and 64 rows:
// from N = 3072 (192 workgroups of 16 rows) the 16-row tile wins everywhere, by 1.2 - 1.7 x; at N = 2048 (128 workgroups
// on 256 CUs) the 8-row tile is 5 - 9 % ahead at either K and row count.  One threshold, no dependence on K or NCB.
// -DKALLE_WIDE_TILE_ROWS=8 | 16 forces one tile everywhere: the builds behind that comparison
// (python -m kalle_audio_amd.build --variant tr8 -DKALLE_WIDE_TILE_ROWS=8, run with KALLE_LIB_PATH; never set in the product build)
inline int wide_tile_rows(int N) {
#ifdef KALLE_WIDE_TILE_ROWS
    static_assert(KALLE_WIDE_TILE_ROWS == 8 || KALLE_WIDE_TILE_ROWS == 16, "weight rows per workgroup");
    (void)N;
    return KALLE_WIDE_TILE_ROWS;
#else
    return N >= 3072 ? 16 : 8;
#endif
}

// y (columns n >= nsplit: y2) = W . pro(x) (+ res); returns the first failed launch.
// rows == NULL: one row, the prologue built inside the GEMV (ldx, xhat, ldh, ldy, ldres unused).  Otherwise the R-row GEMM: the
// prologue, if any, as a pre-pass into xhat (row stride ldh), y2 columns of row r at rows->y2_off[r]; up to 16 rows the kernels
// of either weight format at NCB = 1, above the bf16 kernel at NCB = ceil(R / 16).  The row set becomes a kernel argument here.
inline int proj_launch(const Proj& P, const void* x, int64_t ldx, int pro, const float* gamma, float eps, bf16_t* xhat,
                       int64_t ldh, void* y, int64_t ldy, bool yf32, void* y2, int nsplit, const float* res, int64_t ldres,
                       const RowSet* rows, int N, int K, hipStream_t st) {
    const bf16_t* Wb = static_cast<const bf16_t*>(P.w);
    const uint8_t* Wq = static_cast<const uint8_t*>(P.w);
    if (!rows) {
        // several row pairs (e4m3: row groups) per wave once there are enough workgroups: the per-workgroup x preparation is
        // amortised.  A workgroup owns 8 rpw rows in both kernels, so the grid is the same for every N.
        const int rpw = N >= 8 * 4 * 512 ? 4 : N >= 8 * 2 * 512 ? 2 : 1;
        const dim3 grid((N + 8 * rpw - 1) / (8 * rpw));
        const size_t lds = (size_t)K * 2;
        for_instance<PRO_BF16, PRO_RMS, PRO_SWIGLU>(yf32, pro, [&](auto yf, auto p) {
            constexpr bool F = decltype(yf)::value;
            constexpr int PRO = decltype(p)::value;
            if (P.scale)
                KALLE_LAUNCH((gemv_e4m3_kernel<F, PRO>), grid, dim3(128), lds, st, x, gamma, eps, Wq, P.ld, P.scale, y, y2, nsplit,
                             res, N, K, rpw);
            else
                KALLE_LAUNCH((gemv_kernel<F, PRO>), grid, dim3(256), lds, st, x, gamma, eps, Wb, P.ld, y, y2, nsplit, res, N, K, rpw);
        });
        return kalle_check_launch();
    }
    const int R = rows->R;
    const bool wide = R > KALLE_DECODE_MAX_ROWS;
    if (wide && P.scale) return KALLE_ERR_ARG;               // (there is no wide e4m3 kernel)
    const bf16_t* X = static_cast<const bf16_t*>(x);
    if (pro != PRO_BF16) {
        for_instance<PRO_RMS, PRO_SWIGLU>(wide, pro, [&](auto w, auto p) {
            using MaskT = std::conditional_t<decltype(w)::value, uint64_t, unsigned>;
            KALLE_LAUNCH((rows_prologue_kernel<decltype(p)::value, MaskT>), dim3(R), dim3(256), 0, st, x, ldx, gamma, eps, xhat, ldh,
                         K, (MaskT)rows->active);
        });
        const int rc = kalle_check_launch();
        if (rc != KALLE_OK) return rc;
        X = xhat;
        ldx = ldh;
    }
    // up to 16 rows never fewer workgroups streaming weights than the one-row form has for this N: N / 8 below 8192 rows, N / 16
    // from there
    const int tr = wide ? wide_tile_rows(N) : N < 8192 ? 8 : 16;
    const dim3 grid((N + tr - 1) / tr), block(256);
    if (!wide) {
        const RowArgs<KALLE_DECODE_MAX_ROWS> a(*rows);
        for_instance<8, 16>(yf32, tr, [&](auto yf, auto t) {
            constexpr bool F = decltype(yf)::value;
            constexpr int TR = decltype(t)::value;
            if (P.scale)
                KALLE_LAUNCH((gemm_rows_e4m3_kernel<F, TR>), grid, block, 0, st, X, ldx, Wq, P.ld, P.scale, y, ldy, y2, nsplit, res,
                             ldres, N, K, a);
            else
                KALLE_LAUNCH((gemm_rows_kernel<F, TR, 1>), grid, block, 0, st, X, ldx, Wb, P.ld, y, ldy, y2, nsplit, res, ldres, N, K,
                             a);
        });
    } else {
        const RowArgs<KALLE_DECODE_WIDE_MAX_ROWS> a(*rows);
        for_instance<2, 3, 4>(yf32, (R + 15) / 16, [&](auto yf, auto nb) {
            constexpr bool F = decltype(yf)::value;
            constexpr int NCB = decltype(nb)::value;
            if (tr == 16)
                KALLE_LAUNCH((gemm_rows_kernel<F, 16, NCB>), grid, block, 0, st, X, ldx, Wb, P.ld, y, ldy, y2, nsplit, res, ldres,
                             N, K, a);
            else
                KALLE_LAUNCH((gemm_rows_kernel<F, 8, NCB>), grid, block, 0, st, X, ldx, Wb, P.ld, y, ldy, y2, nsplit, res, ldres, N,
                             K, a);
        });
    }
    return kalle_check_launch();
}

// peak normalisation to int16 (infer_0723.py:293: x / max|x| -> clamp(-1, 1) * 32767 -> int16, truncating like .to(int16))
template <bool F32>
__global__ __launch_bounds__(256) void absmax_kernel(const void* __restrict__ x, unsigned* __restrict__ peak_bits, int64_t n) {
    __shared__ float red[4];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(F32 ? static_cast<const float*>(x)[i] : bf16_to_f32(static_cast<const bf16_t*>(x)[i])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)   // non-negative floats order like their bit patterns
        atomicMax(peak_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}
// float quotient with one residual correction.  The library is built with -ffast-math, under which a / b (__fdiv_rn included, and a
// double quotient narrowed back to float too) compiles to a * rcp(b) with a 1-ulp reciprocal: peak / peak can then be 1 - 2^-24 and the
// loudest sample lands on 32766 instead of 32767.  q + (a - q b) / b with the residual in one fma is exact for a == b and within
// half an ulp (+ 2^-46 relative) of a / b otherwise.
__device__ __forceinline__ float div_refined(float a, float b) {
    const float r = __builtin_amdgcn_rcpf(b);
    const float q = a * r;
    return __builtin_fmaf(__builtin_fmaf(-q, b, a), r, q);
}

template <bool F32>
__global__ __launch_bounds__(256) void to_int16_kernel(const void* __restrict__ x, const unsigned* __restrict__ peak_bits,
                                                       int16_t* __restrict__ out, int64_t n) {
    const float peak = __uint_as_float(peak_bits[0]);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v0 = div_refined(F32 ? static_cast<const float*>(x)[i] : bf16_to_f32(static_cast<const bf16_t*>(x)[i]), peak);
        float v = v0;
        v = fminf(fmaxf(v, -1.f), 1.f) * 32767.f;
        out[i] = (int16_t)(int)v;
    }
}

// out[r, :] = audio[r, :] * am[r] + table[ids[r], :] * im[r]     (model_sigmaVAE.py:66, 73)
template <bool AF32>
__global__ __launch_bounds__(256) void embed_mix_fwd_kernel(const int64_t* __restrict__ ids,
                                                            const float* __restrict__ table,
                                                            const void* __restrict__ audio,
                                                            const float* __restrict__ im, const float* __restrict__ am,
                                                            float* __restrict__ out, int64_t rows, int D, int64_t V) {
    const int cpr = D >> 2;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 4;
        const float wi = im[r], wa = am[r];
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (wi != 0.f) {
            int64_t id = ids[r];
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            const f32x4 e = *reinterpret_cast<const f32x4*>(table + id * D + c);
            o = e * wi;
        }
        if (wa != 0.f) {
            f32x4 a;
            if constexpr (AF32) {
                a = *reinterpret_cast<const f32x4*>(static_cast<const float*>(audio) + r * D + c);
            } else {
                const i32x2 v = *reinterpret_cast<const i32x2*>(static_cast<const bf16_t*>(audio) + r * D + c);
                a = f32x4{bf16lo((uint32_t)v[0]), bf16hi((uint32_t)v[0]), bf16lo((uint32_t)v[1]), bf16hi((uint32_t)v[1])};
            }
            o += a * wa;
        }
        *reinterpret_cast<f32x4*>(out + r * D + c) = o;
    }
}

// daudio[r, :] = dout[r, :] * am[r] ;  dtable[ids[r], :] += dout[r, :] * im[r]  (fp32 atomics: tokens repeat)
__global__ __launch_bounds__(256) void embed_mix_bwd_kernel(const float* __restrict__ dout,
                                                            const int64_t* __restrict__ ids,
                                                            const float* __restrict__ im, const float* __restrict__ am,
                                                            float* __restrict__ dtable, float* __restrict__ daudio,
                                                            int64_t rows, int D, int64_t V) {
    const int cpr = D >> 2;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dout + r * D + c);
        if (daudio) *reinterpret_cast<f32x4*>(daudio + r * D + c) = g * am[r];
        const float wi = im[r];
        if (dtable && wi != 0.f) {
            int64_t id = ids[r];
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            float* dst = dtable + id * D + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(dst + e, g[e] * wi);
        }
    }
}

// exact GELU (nn.GELU() default, model_sigmaVAE.py:46): 0.5 x (1 + erf(x / sqrt 2))
__device__ __forceinline__ float gelu_exact(float v) {
    const float h = 0.5f * v;
    return h * (1.f + erff(v * 0.70710678118654752f));
}

template <bool F32>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const void* __restrict__ x, void* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = F32 ? static_cast<const float*>(x)[i] : bf16_to_f32(static_cast<const bf16_t*>(x)[i]);
        const float o = gelu_exact(v);
        if constexpr (F32) static_cast<float*>(y)[i] = o;
        else static_cast<bf16_t*>(y)[i] = f32_to_bf16(o);
    }
}
template <bool F32>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                       void* __restrict__ dx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = F32 ? static_cast<const float*>(x)[i] : bf16_to_f32(static_cast<const bf16_t*>(x)[i]);
        const float g = F32 ? static_cast<const float*>(dy)[i] : bf16_to_f32(static_cast<const bf16_t*>(dy)[i]);
        const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
        const float pdf = 0.39894228040143268f * __expf(-0.5f * v * v);
        const float o = g * (cdf + v * pdf);
        if constexpr (F32) static_cast<float*>(dx)[i] = o;
        else static_cast<bf16_t*>(dx)[i] = f32_to_bf16(o);
    }
}

// ---- the middle of the per-frame head of KV-cached generation (model_sigmaVAE.py:127-146, kalle_llasa_frame_head_rows) ---------
// One workgroup per active row r:  a = bf16(gelu(h1[r])),  mean = W2 . a + b2,  latent = mean + std * noise[r],
// lat = bf16(latent),  kl[r] = (1/dl) sum_j [c0 + (std^2 + (mean_j - 1)^2) c1 - 1/2]  with c0 = log(e / std), c1 = 1 / (2 e^2).
// A weight row is dl / 8 <= 64 chunks of 16 bytes: G lanes (the power of two >= dl / 8) own a row and lane c of the group its
// chunk c, so a lane multiplies every row it meets by the SAME eight activations - they are computed once, into registers, and
// need no LDS.  The 256 / G groups walk the rows 256 / G at a time, PF rows per step, the loads of the next step issued before
// the FMAs of this one.  The KL terms meet in LDS and wave 0 sums them in a fixed order.  No atomics, nothing another
// workgroup writes is read: a row's bits depend on that row alone.
__global__ __launch_bounds__(256) void llasa_head_kernel(const float* __restrict__ h1, const bf16_t* __restrict__ W2, int64_t ldw2,
                                                         const float* __restrict__ b2, const float* __restrict__ noise,
                                                         int64_t ldn, float std, float c0, float c1, bf16_t* __restrict__ a_out,
                                                         float* __restrict__ mean, float* __restrict__ latent,
                                                         bf16_t* __restrict__ lat, float* __restrict__ kl, int dl, int lgG,
                                                         unsigned active) {
    __shared__ float term[512];
    const int r = blockIdx.x;
    if (!(active >> r & 1)) return;
    constexpr int PF = 8;
    const int G = 1 << lgG, ngrp = 256 >> lgG, nc = dl >> 3;
    const int c = threadIdx.x & (G - 1), grp = threadIdx.x >> lgG;
    const bool in = c < nc;
    auto load = [&](int base, i32x4* w) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int j = base + p * ngrp + grp;
            w[p] = i32x4{0, 0, 0, 0};
            if (in) w[p] = *reinterpret_cast<const i32x4*>(W2 + (int64_t)(j < dl ? j : dl - 1) * ldw2 + 8 * c);
        }
    };
    i32x4 w[PF];
    load(0, w);                                   // (the weight stream does not wait for the activations)
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float* hr = h1 + (int64_t)r * dl + 8 * c;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(hr), hi = *reinterpret_cast<const f32x4*>(hr + 4);
        i32x4 o;
        o[0] = (int)pack_bf16x2(gelu_exact(lo[0]), gelu_exact(lo[1]));
        o[1] = (int)pack_bf16x2(gelu_exact(lo[2]), gelu_exact(lo[3]));
        o[2] = (int)pack_bf16x2(gelu_exact(hi[0]), gelu_exact(hi[1]));
        o[3] = (int)pack_bf16x2(gelu_exact(hi[2]), gelu_exact(hi[3]));
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[2 * e] = bf16lo((uint32_t)o[e]); x[2 * e + 1] = bf16hi((uint32_t)o[e]); }
        if (grp == 0) *reinterpret_cast<i32x4*>(a_out + (int64_t)r * dl + 8 * c) = o;
    }
    const float s2 = std * std;
    for (int base = 0; base < dl; base += ngrp * PF) {          // (uniform over the workgroup: every lane takes every shuffle)
        i32x4 wn[PF];
        const bool more = base + ngrp * PF < dl;
        if (more) load(base + ngrp * PF, wn);
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += bf16lo((uint32_t)w[p][e]) * x[2 * e] + bf16hi((uint32_t)w[p][e]) * x[2 * e + 1];
            for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int j = base + p * ngrp + grp;
            if (c == 0 && j < dl) {
                const int64_t at = (int64_t)r * dl + j;
                const float m = s + b2[j];
                const float z = m + std * noise[r * ldn + j];
                mean[at] = m;
                latent[at] = z;
                lat[at] = f32_to_bf16(z);
                const float d = m - 1.f;
                term[j] = c0 + (s2 + d * d) * c1 - 0.5f;
            }
        }
        if (more) {
#pragma unroll
            for (int p = 0; p < PF; ++p) w[p] = wn[p];
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int j = threadIdx.x; j < dl; j += 64) s += term[j];
        s = wave_sum(s);
        if (threadIdx.x == 0) kl[r] = s / (float)dl;
    }
}

// ---- the same stage for the head that predicts its scale (model.py:109-150, kalle_llasa_frame_head2_rows) -------------------------
// One workgroup per active row r, d2 = 2 lat:  a = bf16(gelu(h1[r])),  disp = W2 . a + b2  (mean = disp[:lat], logs = disp[lat:]),
// s = exp(logs),  latent = mean + s * noise[r],  lat = bf16(latent),
// kl[r] = (1/lat) sum_j [(1 - logs_j) + (s_j^2 + (mean_j - 1)^2) c1 - 1/2]  with c1 = 1 / (2 e^2).
// Phase 1 is the W2 walk of llasa_head_kernel over d2 rows (written out again, so that kernel's summation order and bits stay as
// they are): rows j and j + lat are finished by different lane groups and, at d2 = 512, in different passes, so the finished
// row goes to global `disp` and to LDS.  Phase 2, after a barrier: thread j < lat reads mean_j and logs_j from LDS and computes
// everything that needs both; the KL terms meet in LDS and wave 0 sums them in a fixed order.  No atomics, nothing another
// workgroup writes is read: a row's bits depend on that row alone.
__global__ __launch_bounds__(256) void llasa_head2_kernel(const float* __restrict__ h1, const bf16_t* __restrict__ W2, int64_t ldw2,
                                                          const float* __restrict__ b2, const float* __restrict__ noise,
                                                          int64_t ldn, float c1, bf16_t* __restrict__ a_out,
                                                          float* __restrict__ disp, float* __restrict__ s_out,
                                                          float* __restrict__ latent, bf16_t* __restrict__ lat,
                                                          float* __restrict__ kl, int dl, int lgG, unsigned active) {
    __shared__ float dsp[512];
    __shared__ float term[256];
    const int r = blockIdx.x;
    if (!(active >> r & 1)) return;
    constexpr int PF = 8;
    const int d2 = 2 * dl;
    const int G = 1 << lgG, ngrp = 256 >> lgG, nc = d2 >> 3;
    const int c = threadIdx.x & (G - 1), grp = threadIdx.x >> lgG;
    const bool in = c < nc;
    auto load = [&](int base, i32x4* w) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int j = base + p * ngrp + grp;
            w[p] = i32x4{0, 0, 0, 0};
            if (in) w[p] = *reinterpret_cast<const i32x4*>(W2 + (int64_t)(j < d2 ? j : d2 - 1) * ldw2 + 8 * c);
        }
    };
    i32x4 w[PF];
    load(0, w);                                   // (the weight stream does not wait for the activations)
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float* hr = h1 + (int64_t)r * d2 + 8 * c;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(hr), hi = *reinterpret_cast<const f32x4*>(hr + 4);
        i32x4 o;
        o[0] = (int)pack_bf16x2(gelu_exact(lo[0]), gelu_exact(lo[1]));
        o[1] = (int)pack_bf16x2(gelu_exact(lo[2]), gelu_exact(lo[3]));
        o[2] = (int)pack_bf16x2(gelu_exact(hi[0]), gelu_exact(hi[1]));
        o[3] = (int)pack_bf16x2(gelu_exact(hi[2]), gelu_exact(hi[3]));
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[2 * e] = bf16lo((uint32_t)o[e]); x[2 * e + 1] = bf16hi((uint32_t)o[e]); }
        if (grp == 0) *reinterpret_cast<i32x4*>(a_out + (int64_t)r * d2 + 8 * c) = o;
    }
    for (int base = 0; base < d2; base += ngrp * PF) {          // (uniform over the workgroup: every lane takes every shuffle)
        i32x4 wn[PF];
        const bool more = base + ngrp * PF < d2;
        if (more) load(base + ngrp * PF, wn);
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += bf16lo((uint32_t)w[p][e]) * x[2 * e] + bf16hi((uint32_t)w[p][e]) * x[2 * e + 1];
            for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int j = base + p * ngrp + grp;
            if (c == 0 && j < d2) {
                const float v = s + b2[j];
                disp[(int64_t)r * d2 + j] = v;
                dsp[j] = v;
            }
        }
        if (more) {
#pragma unroll
            for (int p = 0; p < PF; ++p) w[p] = wn[p];
        }
    }
    __syncthreads();
    const int j = threadIdx.x;                    // lat <= 256: one thread per latent element
    if (j < dl) {
        const float m = dsp[j], lg = dsp[j + dl];
        const float sc = expf(lg);
        const float z = m + sc * noise[r * ldn + j];
        const int64_t at = (int64_t)r * dl + j;
        s_out[at] = sc;
        latent[at] = z;
        lat[at] = f32_to_bf16(z);
        const float d = m - 1.f;
        term[j] = (1.f - lg) + (sc * sc + d * d) * c1 - 0.5f;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int t = threadIdx.x; t < dl; t += 64) s += term[t];
        s = wave_sum(s);
        if (threadIdx.x == 0) kl[r] = s / (float)dl;
    }
}

// KL( N(pred, s) || N(label, s) ) = (pred - label)^2 / (2 s^2), summed over the latent dim / dim, then the two masked
// sums over rows (model_sigmaVAE.py:85-95).  One wave per row; sums[0..3] += {kl*ma, ma, kl*mb, mb}.
__global__ __launch_bounds__(256) void gauss_kl_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                           const float* __restrict__ ma, const float* __restrict__ mb,
                                                           float* __restrict__ sums, float coef, int64_t rows, int d) {
    __shared__ float red[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        float s = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float t = pred[r * d + c] - label[r * d + c];
            s += t * t;
        }
        s = wave_sum(s) * coef;
        const float a = ma[r], b = mb[r];
        acc[0] += s * a; acc[1] += a; acc[2] += s * b; acc[3] += b;
    }
    if (lane == 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 4) atomicAdd(sums + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                                       red[3][threadIdx.x]);
}
// dpred[r, c] = 2 coef (pred - label) * (ga * ma[r] / sum(ma) + gb * mb[r] / sum(mb)); ga / gb: upstream gradients of the
// two losses (device scalars), sums from the forward
__global__ __launch_bounds__(256) void gauss_kl_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                           const float* __restrict__ ma, const float* __restrict__ mb,
                                                           const float* __restrict__ sums, const float* __restrict__ ga,
                                                           const float* __restrict__ gb, float* __restrict__ dpred,
                                                           float coef, int64_t rows, int d) {
    const float wa = ga[0] / sums[1], wb = gb[0] / sums[3];
    const int64_t total = rows * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / d;
        dpred[i] = 2.f * coef * (pred[i] - label[i]) * (wa * ma[r] + wb * mb[r]);
    }
}

// ---- two-Gaussian KL of model.py:84-100 --------------------------------------------------------------------------------
// KL( N(m1, s1) || N(m2, s2) ) = log(s2 / s1) + (s1^2 + (m1 - m2)^2) / (2 s2^2) - 1/2 per latent element, with
// m2 | log s2 = the two halves of the head's output row [2 dim]; summed over the latent dim / dim; two masked sums over rows.
// Label statistics: MODE 0 - explicit mean / std rows [dim] (a caller-supplied transform already applied);
//                   MODE 1 - one row [2 dim] = mean | scale of the Oobleck encoder, std = softplus(scale) + 1e-4
//                            (stable_audio_tools/models/bottleneck.py:51-54 on the same tensor); both times std_mult (1.25).
template <int MODE>
__device__ __forceinline__ void kl2_label(const float* __restrict__ lmean, const float* __restrict__ lstd, int64_t r, int c,
                                          int d, float std_mult, float& m1, float& s1) {
    if constexpr (MODE == 0) {
        m1 = lmean[r * d + c];
        s1 = lstd[r * d + c] * std_mult;
    } else {
        m1 = lmean[r * 2 * d + c];
        const float sc = lmean[r * 2 * d + d + c];
        s1 = ((sc > 20.f ? sc : log1pf(expf(sc))) + 1e-4f) * std_mult;      // F.softplus (threshold 20)
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void gauss_kl2_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ lmean,
                                                            const float* __restrict__ lstd, const float* __restrict__ ma,
                                                            const float* __restrict__ mb, float* __restrict__ sums,
                                                            float std_mult, int64_t rows, int d) {
    __shared__ float red[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float inv_d = 1.f / (float)d;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        float s = 0.f;
        for (int c = lane; c < d; c += 64) {
            float m1, s1;
            kl2_label<MODE>(lmean, lstd, r, c, d, std_mult, m1, s1);
            const float m2 = pred[r * 2 * d + c], l2 = pred[r * 2 * d + d + c];
            const float dm = m1 - m2;
            s += l2 - logf(s1) + 0.5f * (s1 * s1 + dm * dm) * expf(-2.f * l2) - 0.5f;
        }
        s = wave_sum(s) * inv_d;
        const float a = ma[r], b = mb[r];
        acc[0] += s * a; acc[1] += a; acc[2] += s * b; acc[3] += b;
    }
    if (lane == 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 4) atomicAdd(sums + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                                       red[3][threadIdx.x]);
}

// d kl / d m2 = (m2 - m1) / s2^2 ;  d kl / d log s2 = 1 - (s1^2 + (m1 - m2)^2) / s2^2 ; times the row weight / dim
template <int MODE>
__global__ __launch_bounds__(256) void gauss_kl2_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ lmean,
                                                            const float* __restrict__ lstd, const float* __restrict__ ma,
                                                            const float* __restrict__ mb, const float* __restrict__ sums,
                                                            const float* __restrict__ ga, const float* __restrict__ gb,
                                                            float* __restrict__ dpred, float std_mult, int64_t rows, int d) {
    const float wa = ga[0] / sums[1], wb = gb[0] / sums[3];
    const float inv_d = 1.f / (float)d;
    const int64_t total = rows * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / d;
        const int c = (int)(i - r * d);
        float m1, s1;
        kl2_label<MODE>(lmean, lstd, r, c, d, std_mult, m1, s1);
        const float m2 = pred[r * 2 * d + c], l2 = pred[r * 2 * d + d + c];
        const float w = (wa * ma[r] + wb * mb[r]) * inv_d, e = expf(-2.f * l2), dm = m2 - m1;
        dpred[r * 2 * d + c] = w * dm * e;
        dpred[r * 2 * d + d + c] = w * (1.f - (s1 * s1 + dm * dm) * e);
    }
}

}  // namespace

extern "C" int kalle_axpby(const float* x, const float* y, float* out, float a, float b, int64_t n, void* stream) {
    if (!x || !y || !out || n <= 0) return KALLE_ERR_ARG;
    KALLE_LAUNCH(axpby_kernel, dim3(grid_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, out, a, b, n);
    return kalle_check_launch();
}

extern "C" int kalle_gemv_bf16(const void* x, const void* W, int64_t ldw, void* y, int y_dtype, const float* residual,
                               int N, int K, void* stream) {
    if (!x || !W || !y || N <= 0 || K <= 0 || (K & 7) || (ldw & 7) || K > 32768) return KALLE_ERR_ARG;
    if (y_dtype != KALLE_F32 && y_dtype != KALLE_BF16) return KALLE_ERR_ARG;
    return proj_launch({W, ldw, nullptr}, x, 0, PRO_BF16, nullptr, 0.f, nullptr, 0, y, 0, y_dtype == KALLE_F32, y, N, residual, 0,
                       nullptr, N, K, static_cast<hipStream_t>(stream));
}

// ---- KV-cached decoding: ONE sequencer for bf16 / e4m3 weights and one row / R rows ----------------------------------------------
extern "C" __attribute__((visibility("hidden"))) void kalle_set_attn_plan(int plan);   // (attention.hip)

namespace {

// The workspace the header publishes, carved in its order; the one-row layout is this at R = 1 without the trailing xn.
struct DecodeWs {                // byte offsets
    int64_t x2, x3, lse;         // fp32 [R][D] | [R][D] | [R][H], the lse region padded to a multiple of 64 bytes
    int64_t q, ao, hf, xn;       // bf16 [R][D] | [R][D] | [R][2*inner] | [R][max(D, inner)]
    int64_t end;
};

inline DecodeWs decode_ws(int R, int H, int inner, int head_dim) {
    const int64_t D = (int64_t)H * head_dim, xw = D > inner ? D : inner;
    DecodeWs w;
    w.x2 = 0;
    w.x3 = w.x2 + R * D * 4;
    w.lse = w.x3 + R * D * 4;
    w.q = w.lse + (((int64_t)R * H * 4 + 63) & ~(int64_t)63);
    w.ao = w.q + R * D * 2;
    w.hf = w.ao + R * D * 2;
    w.xn = w.hf + R * 2 * (int64_t)inner * 2;
    w.end = w.xn + R * xw * 2;
    return w;
}

// one decoder layer of either descriptor form
struct LayerView {
    const float* input_norm;
    Proj qkv, o;
    const float* post_norm;
    Proj ug, down;
    void* kv_cache;
    bool complete(bool w8) const {
        return input_norm && qkv.w && o.w && post_norm && ug.w && down.w && kv_cache &&
               (!w8 || (qkv.scale && o.scale && ug.scale && down.scale));
    }
};
inline LayerView layer_view(const kalle_llama_layer& L, int D, int inner) {
    return {L.input_norm, {L.wqkv, D, nullptr}, {L.wo, D, nullptr}, L.post_norm, {L.wug, D, nullptr}, {L.wdown, inner, nullptr},
            L.kv_cache};
}
inline LayerView layer_view(const kalle_llama_layer_w8& L, int D, int inner) {
    return {L.input_norm, {L.wqkv, D, L.sqkv}, {L.wo, D, L.so}, L.post_norm, {L.wug, D, L.sug}, {L.wdown, inner, L.sdown},
            L.kv_cache};
}

// The step behind the exported ones.  Exactly one of lb / l8 is set.  STEP_ROWS: the R-row form (t0[r] < 0 = row r inactive,
// skinny GEMMs, kalle_attention_decode_rows); STEP_WIDE: that with 17 .. 64 rows (bf16 only) - the projections through the wide
// GEMM, the attention once per chunk of 16 rows; STEP_ONE: R = 1, GEMVs and kalle_attention_decode_hd.  Nothing is launched
// unless every argument and every layer passes.
enum StepForm { STEP_ONE, STEP_ROWS, STEP_WIDE };

int decode_step(const kalle_llama_layer* lb, const kalle_llama_layer_w8* l8, int n_layers, const float* x, float* out,
                StepForm form, int R, int H, int Hkv, int inner, int head_dim, float eps, const int32_t* t0, int cache_rows,
                const float* rope_cos, const float* rope_sin, void* workspace, void* stream) {
    const bool batched = form != STEP_ONE, is_wide = form == STEP_WIDE;
    kalle_set_attn_plan(0);      // (a step refused before its first launch leaves no attention plan behind)
    if ((!lb && !l8) || n_layers <= 0 || !x || !out || !workspace || !rope_cos || !rope_sin || !t0) return KALLE_ERR_ARG;
    if (R < 1 || R > (is_wide ? KALLE_DECODE_WIDE_MAX_ROWS : KALLE_DECODE_MAX_ROWS) || (is_wide && !lb)) return KALLE_ERR_ARG;
    // (a lane's unit of a weight row is 16 bytes: 8 bf16 weights, 16 e4m3 codes; D is a multiple of 64)
    if (H <= 0 || Hkv <= 0 || H % Hkv || inner <= 0 || (inner & (l8 ? 15 : 7)) || cache_rows <= 0) return KALLE_ERR_ARG;
    if (head_dim != 64 && head_dim != 128) return KALLE_ERR_ARG;
    if ((int64_t)H * head_dim > 32768 || inner > 32768) return KALLE_ERR_ARG;
    const int D = H * head_dim, kvw = 2 * Hkv * head_dim, xw = D > inner ? D : inner;
    RowSet kvr{};                                            // (second destination: the rows' KV-cache rows)
    kvr.R = R;
    int32_t nk[KALLE_DECODE_WIDE_MAX_ROWS];
    for (int r = 0; r < R; ++r) {
        // (batched: the attention's LDS score array holds nk <= KALLE_ATTN_DECODE_MAX_KEYS keys; the one-row attention falls back to the tiled kernel)
        if (t0[r] >= cache_rows || (batched ? t0[r] >= KALLE_ATTN_DECODE_MAX_KEYS : t0[r] < 0)) return KALLE_ERR_ARG;
        nk[r] = t0[r] < 0 ? 0 : t0[r] + 1;
        if (t0[r] >= 0) kvr.active |= (uint64_t)1 << r;
        kvr.y2_off[r] = t0[r] < 0 ? 0 : ((int64_t)r * cache_rows + t0[r]) * kvw;
    }
    auto layer = [&](int l) { return lb ? layer_view(lb[l], D, inner) : layer_view(l8[l], D, inner); };
    for (int l = 0; l < n_layers; ++l)
        if (!layer(l).complete(l8 != nullptr)) return KALLE_ERR_ARG;
    if (!kvr.active) return KALLE_OK;
    RowSet plain{};                                          // (no second destination)
    plain.active = kvr.active;
    plain.R = R;
    const RowSet* rows_kv = batched ? &kvr : nullptr;
    const RowSet* rows = batched ? &plain : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DecodeWs o = decode_ws(R, H, inner, head_dim);
    char* ws = static_cast<char*>(workspace);
    float* x2 = reinterpret_cast<float*>(ws + o.x2);        // residual stream after the attention branch
    float* x3 = reinterpret_cast<float*>(ws + o.x3);        // layer output (input of the next layer)
    float* lse = reinterpret_cast<float*>(ws + o.lse);
    bf16_t* q = reinterpret_cast<bf16_t*>(ws + o.q);
    bf16_t* ao = reinterpret_cast<bf16_t*>(ws + o.ao);
    bf16_t* hf = reinterpret_cast<bf16_t*>(ws + o.hf);
    bf16_t* xn = batched ? reinterpret_cast<bf16_t*>(ws + o.xn) : nullptr;      // (the one-row workspace ends before it)
    const float* xin = x;
    for (int l = 0; l < n_layers; ++l) {
        const LayerView L = layer(l);
        // q -> scratch, k | v -> cache row t0[r] of sequence r (un-rotated: the attention kernel rotates by row index); the one-row
        // GEMV takes the row's address, the R-row GEMM the cache and y2_off.
        // (every launch is checked where it is made: KALLE_LAUNCH clears the error state, so a refused launch would otherwise be
        // forgotten by the next one and the step would report success over an unwritten buffer)
        // (nsplit = D is a multiple of 64 at either head dim: a wave's rows never straddle it)
        void* kv = batched ? L.kv_cache : static_cast<bf16_t*>(L.kv_cache) + kvr.y2_off[0];
        int rc = proj_launch(L.qkv, xin, D, PRO_RMS, L.input_norm, eps, xn, xw, q, D, false, kv, D, nullptr, 0, rows_kv, D + kvw,
                             D, st);
        if (rc != KALLE_OK) return rc;
        if (is_wide) {
            // the per-row attention in chunks of 16 rows: q / ao, the cache, lse and nk offset by the chunk's first row.  A chunk
            // with no active row launches nothing; the plan word left behind is the last launching chunk's
            const bf16_t* cache = static_cast<const bf16_t*>(L.kv_cache);
            const int64_t kvs = (int64_t)cache_rows * kvw;
            int plan = 0;
            for (int r0 = 0; r0 < R && rc == KALLE_OK; r0 += KALLE_DECODE_MAX_ROWS) {
                const int rn = R - r0 < KALLE_DECODE_MAX_ROWS ? R - r0 : KALLE_DECODE_MAX_ROWS;
                if (!(kvr.active >> r0 & 0xFFFFu)) continue;
                rc = kalle_attention_decode_rows(q + (int64_t)r0 * D, D, 0, cache + r0 * kvs, kvw, 0, cache + r0 * kvs, kvw,
                                                 Hkv * head_dim, kvs, ao + (int64_t)r0 * D, D, lse + (int64_t)r0 * H, rope_cos,
                                                 rope_sin, head_dim, nk + r0, rn, H, Hkv, head_dim, stream);
                plan = kalle_attn_last_plan();
            }
            if (rc == KALLE_OK) kalle_set_attn_plan(plan);
        } else if (batched) {
            rc = kalle_attention_decode_rows(q, D, 0, L.kv_cache, kvw, 0, L.kv_cache, kvw, Hkv * head_dim,
                                             (int64_t)cache_rows * kvw, ao, D, lse, rope_cos, rope_sin, head_dim, nk, R, H, Hkv,
                                             head_dim, stream);
        } else {
            rc = kalle_attention_decode_hd(q, D, 0, L.kv_cache, kvw, 0, L.kv_cache, kvw, Hkv * head_dim, ao, D, lse, rope_cos,
                                           rope_sin, head_dim, nullptr, 1, H, Hkv, nk[0], head_dim, stream);
        }
        if (rc != KALLE_OK) return rc;
        rc = proj_launch(L.o, ao, D, PRO_BF16, nullptr, 0.f, nullptr, 0, x2, D, true, x2, D, xin, D, rows, D, D, st);
        if (rc != KALLE_OK) return rc;
        rc = proj_launch(L.ug, x2, D, PRO_RMS, L.post_norm, eps, xn, xw, hf, 2 * inner, false, hf, 2 * inner, nullptr, 0, rows,
                         2 * inner, D, st);
        if (rc != KALLE_OK) return rc;
        float* xo = l + 1 == n_layers ? out : x3;
        rc = proj_launch(L.down, hf, 2 * inner, PRO_SWIGLU, nullptr, 0.f, xn, xw, xo, D, true, xo, D, x2, D, rows, D, inner, st);
        if (rc != KALLE_OK) return rc;
        xin = xo;
    }
    return KALLE_OK;
}

}  // namespace

extern "C" int kalle_llama_decode_ws_bytes_hd(int H, int Hkv, int inner, int head_dim) {
    if (H <= 0 || Hkv <= 0 || inner <= 0 || (head_dim != 64 && head_dim != 128)) return KALLE_ERR_ARG;
    return (int)decode_ws(1, H, inner, head_dim).xn;         // (one row: no pre-pass, no xn)
}

extern "C" int kalle_llama_decode_ws_bytes_rows(int R, int H, int Hkv, int inner, int head_dim) {
    if (R < 1 || R > KALLE_DECODE_MAX_ROWS || H <= 0 || Hkv <= 0 || inner <= 0 || (head_dim != 64 && head_dim != 128))
        return KALLE_ERR_ARG;
    if ((int64_t)H * head_dim > 32768 || inner > 32768) return KALLE_ERR_ARG;
    return (int)decode_ws(R, H, inner, head_dim).end;
}

// the six exported steps: argument adapters of decode_step
extern "C" int kalle_llama_decode_step_hd(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int H,
                                          int Hkv, int inner, int head_dim, float eps, int t0, int cache_rows,
                                          const float* rope_cos, const float* rope_sin, void* workspace, void* stream) {
    const int32_t t = t0;
    return decode_step(layers, nullptr, n_layers, x, out, STEP_ONE, 1, H, Hkv, inner, head_dim, eps, &t, cache_rows, rope_cos, rope_sin,
                       workspace, stream);
}
extern "C" int kalle_llama_decode_step_w8(const kalle_llama_layer_w8* layers, int n_layers, const float* x, float* out, int H,
                                          int Hkv, int inner, int head_dim, float eps, int t0, int cache_rows,
                                          const float* rope_cos, const float* rope_sin, void* workspace, void* stream) {
    const int32_t t = t0;
    return decode_step(nullptr, layers, n_layers, x, out, STEP_ONE, 1, H, Hkv, inner, head_dim, eps, &t, cache_rows, rope_cos, rope_sin,
                       workspace, stream);
}
extern "C" int kalle_llama_decode_step_rows(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int R,
                                            int H, int Hkv, int inner, int head_dim, float eps, const int32_t* t0,
                                            int cache_rows, const float* rope_cos, const float* rope_sin, void* workspace,
                                            void* stream) {
    return decode_step(layers, nullptr, n_layers, x, out, STEP_ROWS, R, H, Hkv, inner, head_dim, eps, t0, cache_rows, rope_cos, rope_sin,
                       workspace, stream);
}
extern "C" int kalle_llama_decode_step_rows_w8(const kalle_llama_layer_w8* layers, int n_layers, const float* x, float* out,
                                               int R, int H, int Hkv, int inner, int head_dim, float eps, const int32_t* t0,
                                               int cache_rows, const float* rope_cos, const float* rope_sin, void* workspace,
                                               void* stream) {
    return decode_step(nullptr, layers, n_layers, x, out, STEP_ROWS, R, H, Hkv, inner, head_dim, eps, t0, cache_rows, rope_cos, rope_sin,
                       workspace, stream);
}
// the wide forms: up to 16 rows they ARE the _rows forms
extern "C" int kalle_llama_decode_ws_bytes_wide(int R, int H, int Hkv, int inner, int head_dim) {
    if (R < 1 || R > KALLE_DECODE_WIDE_MAX_ROWS || H <= 0 || Hkv <= 0 || inner <= 0 || (head_dim != 64 && head_dim != 128))
        return KALLE_ERR_ARG;
    if ((int64_t)H * head_dim > 32768 || inner > 32768) return KALLE_ERR_ARG;
    return (int)decode_ws(R, H, inner, head_dim).end;
}
extern "C" int kalle_llama_decode_step_wide(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int R,
                                            int H, int Hkv, int inner, int head_dim, float eps, const int32_t* t0,
                                            int cache_rows, const float* rope_cos, const float* rope_sin, void* workspace,
                                            void* stream) {
    return decode_step(layers, nullptr, n_layers, x, out, R <= KALLE_DECODE_MAX_ROWS ? STEP_ROWS : STEP_WIDE, R, H, Hkv, inner,
                       head_dim, eps, t0, cache_rows, rope_cos, rope_sin, workspace, stream);
}
// the head-dim-64 forms of the C ABI: forwarders
extern "C" int kalle_llama_decode_ws_bytes(int H, int Hkv, int inner) { return kalle_llama_decode_ws_bytes_hd(H, Hkv, inner, 64); }
extern "C" int kalle_llama_decode_step(const kalle_llama_layer* layers, int n_layers, const float* x, float* out, int H,
                                       int Hkv, int inner, float eps, int t0, int cache_rows, const float* rope_cos,
                                       const float* rope_sin, void* workspace, void* stream) {
    return kalle_llama_decode_step_hd(layers, n_layers, x, out, H, Hkv, inner, 64, eps, t0, cache_rows, rope_cos, rope_sin,
                                      workspace, stream);
}

// ---- the R-row GEMM entry points -------------------------------------------------------------------------------------------------
// the argument check and the row set of both weight formats, then the launch.  kalign: 8 (bf16) or 16 (e4m3) weights per 16 bytes.
// (everything but the bound on R, which is the caller's)
static int gemm_rows_args_ok(int kalign, const void* x, const void* w, int64_t ldw, const void* y, int64_t ldx, int prologue,
                             const float* gamma, const void* xhat, int64_t ldy, int y_dtype, const void* y2, int nsplit,
                             const int64_t* y2_off, int64_t ldres, int N, int K) {
    if (!x || !w || !y || N <= 0 || K <= 0 || (K & (kalign - 1)) || (ldw & (kalign - 1)) || K > 32768) return KALLE_ERR_ARG;
    if (y_dtype != KALLE_F32 && y_dtype != KALLE_BF16) return KALLE_ERR_ARG;
    if (prologue != PRO_BF16 && prologue != PRO_RMS && prologue != PRO_SWIGLU) return KALLE_ERR_ARG;
    if (prologue == PRO_RMS ? (!gamma || (ldx & 3)) : (ldx & 7)) return KALLE_ERR_ARG;
    if (prologue != PRO_BF16 && !xhat) return KALLE_ERR_ARG;
    if (ldx < (prologue == PRO_SWIGLU ? 2 * (int64_t)K : K) || ldw < K || ldy < 0 || ldres < 0) return KALLE_ERR_ARG;
    if (nsplit < 0 || nsplit > N || (nsplit < N && (!y2 || !y2_off))) return KALLE_ERR_ARG;
    return KALLE_OK;
}

static int gemm_rows_entry(const Proj& P, int kalign, const void* x, int64_t ldx, int prologue, const float* gamma, float eps,
                           void* xhat, void* y, int64_t ldy, int y_dtype, void* y2, int nsplit, const int64_t* y2_off,
                           const float* residual, int64_t ldres, const int32_t* active, int R, int max_rows, int N, int K,
                           void* stream) {
    if (R < 1 || R > max_rows) return KALLE_ERR_ARG;
    const int ok = gemm_rows_args_ok(kalign, x, P.w, P.ld, y, ldx, prologue, gamma, xhat, ldy, y_dtype, y2, nsplit, y2_off, ldres, N, K);
    if (ok != KALLE_OK) return ok;
    RowSet a{};
    a.R = R;
    for (int r = 0; r < R; ++r) {
        if (!active || active[r]) a.active |= (uint64_t)1 << r;
        a.y2_off[r] = nsplit < N ? y2_off[r] : 0;
    }
    if (!a.active) return KALLE_OK;
    return proj_launch(P, x, ldx, prologue, gamma, eps, static_cast<bf16_t*>(xhat), K, y, ldy, y_dtype == KALLE_F32, y2, nsplit,
                       residual, ldres, &a, N, K, static_cast<hipStream_t>(stream));
}

extern "C" int kalle_gemm_rows_fused(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat,
                                     const void* W, int64_t ldw, void* y, int64_t ldy, int y_dtype, void* y2, int nsplit,
                                     const int64_t* y2_off, const float* residual, int64_t ldres, const int32_t* active, int R,
                                     int N, int K, void* stream) {
    return gemm_rows_entry({W, ldw, nullptr}, 8, x, ldx, prologue, gamma, eps, xhat, y, ldy, y_dtype, y2, nsplit, y2_off, residual,
                           ldres, active, R, KALLE_DECODE_MAX_ROWS, N, K, stream);
}

// kalle_gemm_rows_fused with the bound at 64 rows (bf16 weights): up to 16 rows the same launch, above the NCB >= 2 kernels
extern "C" int kalle_gemm_rows_wide(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat,
                                    const void* W, int64_t ldw, void* y, int64_t ldy, int y_dtype, void* y2, int nsplit,
                                    const int64_t* y2_off, const float* residual, int64_t ldres, const int32_t* active, int R,
                                    int N, int K, void* stream) {
    return gemm_rows_entry({W, ldw, nullptr}, 8, x, ldx, prologue, gamma, eps, xhat, y, ldy, y_dtype, y2, nsplit, y2_off, residual,
                           ldres, active, R, KALLE_DECODE_WIDE_MAX_ROWS, N, K, stream);
}

extern "C" int kalle_gemm_rows_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, int y_dtype,
                                    const float* residual, int64_t ldres, int R, int N, int K, void* stream) {
    return kalle_gemm_rows_fused(x, ldx, PRO_BF16, nullptr, 0.f, nullptr, W, ldw, y, ldy, y_dtype, nullptr, N, nullptr, residual,
                                 ldres, nullptr, R, N, K, stream);
}

extern "C" int kalle_gemm_rows_fused_e4m3(const void* x, int64_t ldx, int prologue, const float* gamma, float eps, void* xhat,
                                          const void* W8, int64_t ldq, const float* scale, void* y, int64_t ldy, int y_dtype,
                                          void* y2, int nsplit, const int64_t* y2_off, const float* residual, int64_t ldres,
                                          const int32_t* active, int R, int N, int K, void* stream) {
    if (!scale) return KALLE_ERR_ARG;
    return gemm_rows_entry({W8, ldq, scale}, 16, x, ldx, prologue, gamma, eps, xhat, y, ldy, y_dtype, y2, nsplit, y2_off, residual,
                           ldres, active, R, KALLE_DECODE_MAX_ROWS, N, K, stream);
}

// ---- the per-frame head of KV-cached generation: final norm, distribution_linear, sampling, stop KL, audio_linear ----------------
namespace {

// The workspace the header publishes, carved in its order, each region padded to 64 bytes.
struct HeadWs {                  // byte offsets
    int64_t xn, h1, a, lat;      // bf16 [R][D] | fp32 [R][dl] | bf16 [R][dl] | bf16 [R][dl]
    int64_t end;
};

inline HeadWs head_ws(int R, int D, int dl) {
    auto pad = [](int64_t b) { return (b + 63) & ~(int64_t)63; };
    HeadWs w;
    w.xn = 0;
    w.h1 = w.xn + pad((int64_t)R * D * 2);
    w.a = w.h1 + pad((int64_t)R * dl * 4);
    w.lat = w.a + pad((int64_t)R * dl * 2);
    w.end = w.lat + pad((int64_t)R * dl * 2);
    return w;
}

inline bool head_dims_ok(int R, int D, int dl) {
    return R >= 1 && R <= KALLE_DECODE_MAX_ROWS && D >= 8 && !(D & 7) && D <= 32768 && dl >= 8 && !(dl & 7) && dl <= 512;
}

}  // namespace

extern "C" int kalle_llasa_head_ws_bytes(int R, int D, int dl) {
    if (!head_dims_ok(R, D, dl)) return KALLE_ERR_ARG;
    return (int)head_ws(R, D, dl).end;
}

extern "C" int kalle_llasa_frame_head_rows(const kalle_llasa_head* head, const float* h, int64_t ldh, const float* noise,
                                           int64_t ldn, float std, float eps, float* mean, float* latent, float* kl,
                                           float* x_next, const int32_t* active, int R, int D, int dl, void* workspace,
                                           void* stream) {
    if (!head || !h || !noise || !mean || !latent || !kl || !x_next || !workspace) return KALLE_ERR_ARG;
    if (!head->norm || !head->w1 || !head->b1 || !head->w2 || !head->b2 || !head->wa || !head->ba) return KALLE_ERR_ARG;
    if (!head_dims_ok(R, D, dl) || !(std > 0.f)) return KALLE_ERR_ARG;
    if ((ldh & 3) || ldh < D || ldn < dl) return KALLE_ERR_ARG;
    if ((head->ldw1 & 7) || head->ldw1 < D || (head->ldw2 & 7) || head->ldw2 < dl || (head->ldwa & 7) || head->ldwa < dl)
        return KALLE_ERR_ARG;
    RowSet a{};
    a.R = R;
    for (int r = 0; r < R; ++r)
        if (!active || active[r]) a.active |= (uint64_t)1 << r;
    if (!a.active) return KALLE_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const HeadWs o = head_ws(R, D, dl);
    char* ws = static_cast<char*>(workspace);
    bf16_t* xn = reinterpret_cast<bf16_t*>(ws + o.xn);       // bf16(rmsnorm(h))
    float* h1 = reinterpret_cast<float*>(ws + o.h1);         // W1 . xn + b1
    bf16_t* ga = reinterpret_cast<bf16_t*>(ws + o.a);        // bf16(gelu(h1))
    bf16_t* lat = reinterpret_cast<bf16_t*>(ws + o.lat);     // bf16(latent)
    // (every launch is checked where it is made, as in decode_step; a bias is the residual at row stride 0)
    int rc = proj_launch({head->w1, head->ldw1, nullptr}, h, ldh, PRO_RMS, head->norm, eps, xn, D, h1, dl, true, h1, dl, head->b1, 0,
                         &a, dl, D, st);
    if (rc != KALLE_OK) return rc;
    int lg = 0;
    while ((8 << lg) < dl) ++lg;                             // G = 1 << lg lanes per weight row, the power of two >= dl / 8
    const float c0 = (float)(1.0 - log((double)std));        // log(e / std)
    const float c1 = (float)(0.5 / (M_E * M_E));             // 1 / (2 e^2)
    KALLE_LAUNCH(llasa_head_kernel, dim3(R), dim3(256), 0, st, h1, static_cast<const bf16_t*>(head->w2), head->ldw2, head->b2, noise,
                 ldn, std, c0, c1, ga, mean, latent, lat, kl, dl, lg, (unsigned)a.active);
    rc = kalle_check_launch();
    if (rc != KALLE_OK) return rc;
    return proj_launch({head->wa, head->ldwa, nullptr}, lat, dl, PRO_BF16, nullptr, 0.f, nullptr, 0, x_next, D, true, x_next, D,
                       head->ba, 0, &a, D, dl, st);
}

// ---- the same for the head that predicts mean || log-scale (model.py:109-150) ---------------------------------------------------
namespace {

struct Head2Ws {                    // byte offsets
    int64_t xn, h1, a, s, lat;      // bf16 [R][D] | fp32 [R][d2] | bf16 [R][d2] | fp32 [R][lat] | bf16 [R][lat]
    int64_t end;
};

inline Head2Ws head2_ws(int R, int D, int lat) {
    auto pad = [](int64_t b) { return (b + 63) & ~(int64_t)63; };
    const int64_t d2 = 2 * (int64_t)lat;
    Head2Ws w;
    w.xn = 0;
    w.h1 = w.xn + pad((int64_t)R * D * 2);
    w.a = w.h1 + pad(R * d2 * 4);
    w.s = w.a + pad(R * d2 * 2);
    w.lat = w.s + pad((int64_t)R * lat * 4);
    w.end = w.lat + pad((int64_t)R * lat * 2);
    return w;
}

inline bool head2_dims_ok(int R, int D, int lat) {
    return R >= 1 && R <= KALLE_DECODE_MAX_ROWS && D >= 8 && !(D & 7) && D <= 32768 && lat >= 8 && !(lat & 7) && lat <= 256;
}

}  // namespace

extern "C" int kalle_llasa_head2_ws_bytes(int R, int D, int lat) {
    if (!head2_dims_ok(R, D, lat)) return KALLE_ERR_ARG;
    return (int)head2_ws(R, D, lat).end;
}

extern "C" int kalle_llasa_frame_head2_rows(const kalle_llasa_head* head, const float* h, int64_t ldh, const float* noise,
                                            int64_t ldn, float eps, float* disp, float* latent, float* kl, float* x_next,
                                            const int32_t* active, int R, int D, int lat, void* workspace, void* stream) {
    if (!head || !h || !noise || !disp || !latent || !kl || !x_next || !workspace) return KALLE_ERR_ARG;
    if (!head->norm || !head->w1 || !head->b1 || !head->w2 || !head->b2 || !head->wa || !head->ba) return KALLE_ERR_ARG;
    if (!head2_dims_ok(R, D, lat)) return KALLE_ERR_ARG;
    const int d2 = 2 * lat;
    if ((ldh & 3) || ldh < D || ldn < lat) return KALLE_ERR_ARG;
    if ((head->ldw1 & 7) || head->ldw1 < D || (head->ldw2 & 7) || head->ldw2 < d2 || (head->ldwa & 7) || head->ldwa < lat)
        return KALLE_ERR_ARG;
    RowSet a{};
    a.R = R;
    for (int r = 0; r < R; ++r)
        if (!active || active[r]) a.active |= (uint64_t)1 << r;
    if (!a.active) return KALLE_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Head2Ws o = head2_ws(R, D, lat);
    char* ws = static_cast<char*>(workspace);
    bf16_t* xn = reinterpret_cast<bf16_t*>(ws + o.xn);       // bf16(rmsnorm(h))
    float* h1 = reinterpret_cast<float*>(ws + o.h1);         // W1 . xn + b1
    bf16_t* ga = reinterpret_cast<bf16_t*>(ws + o.a);        // bf16(gelu(h1))
    float* sc = reinterpret_cast<float*>(ws + o.s);          // exp(logs)
    bf16_t* lb = reinterpret_cast<bf16_t*>(ws + o.lat);      // bf16(latent)
    int rc = proj_launch({head->w1, head->ldw1, nullptr}, h, ldh, PRO_RMS, head->norm, eps, xn, D, h1, d2, true, h1, d2, head->b1, 0,
                         &a, d2, D, st);
    if (rc != KALLE_OK) return rc;
    int lg = 0;
    while ((8 << lg) < d2) ++lg;                             // G = 1 << lg lanes per weight row, the power of two >= d2 / 8
    const float c1 = (float)(0.5 / (M_E * M_E));             // 1 / (2 e^2)
    KALLE_LAUNCH(llasa_head2_kernel, dim3(R), dim3(256), 0, st, h1, static_cast<const bf16_t*>(head->w2), head->ldw2, head->b2, noise,
                 ldn, c1, ga, disp, sc, latent, lb, kl, lat, lg, (unsigned)a.active);
    rc = kalle_check_launch();
    if (rc != KALLE_OK) return rc;
    return proj_launch({head->wa, head->ldwa, nullptr}, lb, lat, PRO_BF16, nullptr, 0.f, nullptr, 0, x_next, D, true, x_next, D,
                       head->ba, 0, &a, D, lat, st);
}

// ---- weight-only e4m3 decoding -----------------------------------------------------------------------------------------------
extern "C" int kalle_quantize_rows_e4m3(const void* W, int64_t ldw, void* W8, int64_t ldq, float* scale, int N, int K,
                                        void* stream) {
    if (!W || !W8 || !scale || N <= 0 || K <= 0 || (K & 15) || (ldw & 7) || (ldq & 15) || ldw < K || ldq < K) return KALLE_ERR_ARG;
    KALLE_LAUNCH(quantize_rows_e4m3_kernel, dim3((N + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream),
                 static_cast<const bf16_t*>(W), ldw, static_cast<uint8_t*>(W8), ldq, scale, N, K);
    return kalle_check_launch();
}

extern "C" int kalle_gemv_fused_e4m3(const void* x, int prologue, const float* gamma, float eps, const void* W8, int64_t ldq,
                                     const float* scale, void* y, int y_dtype, void* y2, int nsplit, const float* residual,
                                     int N, int K, void* stream) {
    if (!x || !W8 || !scale || !y || N <= 0 || K <= 0 || (K & 15) || (ldq & 15) || ldq < K || K > 32768) return KALLE_ERR_ARG;
    if (y_dtype != KALLE_F32 && y_dtype != KALLE_BF16) return KALLE_ERR_ARG;
    if (prologue != PRO_BF16 && prologue != PRO_RMS && prologue != PRO_SWIGLU) return KALLE_ERR_ARG;
    if (prologue == PRO_RMS && !gamma) return KALLE_ERR_ARG;
    if (nsplit < 0 || nsplit > N || (nsplit < N && !y2)) return KALLE_ERR_ARG;
    return proj_launch({W8, ldq, scale}, x, 0, prologue, gamma, eps, nullptr, 0, y, 0, y_dtype == KALLE_F32, nsplit == N ? y : y2,
                       nsplit, residual, 0, nullptr, N, K, static_cast<hipStream_t>(stream));
}

extern "C" int kalle_gemv_e4m3(const void* x, const void* W8, int64_t ldq, const float* scale, void* y, int y_dtype,
                               const float* residual, int N, int K, void* stream) {
    return kalle_gemv_fused_e4m3(x, PRO_BF16, nullptr, 0.f, W8, ldq, scale, y, y_dtype, nullptr, N, residual, N, K, stream);
}

extern "C" int kalle_peak_normalize_int16(const void* x, int dtype, float* peak, int16_t* out, int64_t n, void* stream) {
    if (!x || !peak || !out || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(peak, 0, sizeof(float), st) != hipSuccess) return KALLE_ERR_LAUNCH;
    unsigned* pb = reinterpret_cast<unsigned*>(peak);
    if (dtype == KALLE_F32) {
        KALLE_LAUNCH((absmax_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, pb, n);
        KALLE_LAUNCH((to_int16_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, pb, out, n);
    } else {
        KALLE_LAUNCH((absmax_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, pb, n);
        KALLE_LAUNCH((to_int16_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, pb, out, n);
    }
    return kalle_check_launch();
}

extern "C" int kalle_embed_mix_fwd(const int64_t* ids, const float* table, const void* audio, int audio_dtype,
                                   const float* ids_mask, const float* audio_mask, float* out, int64_t rows, int D,
                                   int64_t vocab, void* stream) {
    if (!ids || !table || !audio || !ids_mask || !audio_mask || !out || rows <= 0 || D <= 0 || (D & 3) || vocab <= 0)
        return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(rows * (D >> 2), 256));
    if (audio_dtype == KALLE_F32)
        KALLE_LAUNCH((embed_mix_fwd_kernel<true>), grid, dim3(256), 0, st, ids, table, audio, ids_mask, audio_mask, out, rows,
                     D, vocab);
    else
        KALLE_LAUNCH((embed_mix_fwd_kernel<false>), grid, dim3(256), 0, st, ids, table, audio, ids_mask, audio_mask, out,
                     rows, D, vocab);
    return kalle_check_launch();
}

extern "C" int kalle_embed_mix_bwd(const float* dout, const int64_t* ids, const float* ids_mask, const float* audio_mask,
                                   float* dtable, float* daudio, int64_t rows, int D, int64_t vocab, void* stream) {
    if (!dout || !ids || !ids_mask || !audio_mask || (!dtable && !daudio) || rows <= 0 || D <= 0 || (D & 3) || vocab <= 0)
        return KALLE_ERR_ARG;
    KALLE_LAUNCH(embed_mix_bwd_kernel, dim3(grid_for(rows * (D >> 2), 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                 dout, ids, ids_mask, audio_mask, dtable, daudio, rows, D, vocab);
    return kalle_check_launch();
}

extern "C" int kalle_gelu_fwd(const void* x, void* y, int dtype, int64_t n, void* stream) {
    if (!x || !y || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32) KALLE_LAUNCH((gelu_fwd_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, n);
    else KALLE_LAUNCH((gelu_fwd_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, n);
    return kalle_check_launch();
}

extern "C" int kalle_gelu_bwd(const void* dy, const void* x, void* dx, int dtype, int64_t n, void* stream) {
    if (!dy || !x || !dx || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32) KALLE_LAUNCH((gelu_bwd_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, dy, x, dx, n);
    else KALLE_LAUNCH((gelu_bwd_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, dy, x, dx, n);
    return kalle_check_launch();
}

extern "C" int kalle_gauss_kl_fwd(const float* pred, const float* label, const float* mask_a, const float* mask_b,
                                  float* sums4, float std, int64_t rows, int dim, void* stream) {
    if (!pred || !label || !mask_a || !mask_b || !sums4 || rows <= 0 || dim <= 0 || !(std > 0.f)) return KALLE_ERR_ARG;
    const float coef = 1.f / (2.f * std * std * (float)dim);
    KALLE_LAUNCH(gauss_kl_fwd_kernel, dim3(grid_for((rows + 3) / 4, 1)), dim3(256), 0, static_cast<hipStream_t>(stream), pred,
                 label, mask_a, mask_b, sums4, coef, rows, dim);
    return kalle_check_launch();
}

extern "C" int kalle_gauss_kl_bwd(const float* pred, const float* label, const float* mask_a, const float* mask_b,
                                  const float* sums4, const float* grad_a, const float* grad_b, float* dpred, float std,
                                  int64_t rows, int dim, void* stream) {
    if (!pred || !label || !mask_a || !mask_b || !sums4 || !grad_a || !grad_b || !dpred || rows <= 0 || dim <= 0 ||
        !(std > 0.f))
        return KALLE_ERR_ARG;
    const float coef = 1.f / (2.f * std * std * (float)dim);
    KALLE_LAUNCH(gauss_kl_bwd_kernel, dim3(grid_for(rows * dim, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pred,
                 label, mask_a, mask_b, sums4, grad_a, grad_b, dpred, coef, rows, dim);
    return kalle_check_launch();
}

extern "C" int kalle_gauss_kl2_fwd(const float* pred, const float* label_mean, const float* label_std, int label_mode,
                                   float std_mult, const float* mask_a, const float* mask_b, float* sums4, int64_t rows,
                                   int dim, void* stream) {
    if (!pred || !label_mean || !mask_a || !mask_b || !sums4 || rows <= 0 || dim <= 0 || !(std_mult > 0.f)) return KALLE_ERR_ARG;
    if (label_mode != 0 && label_mode != 1) return KALLE_ERR_ARG;
    if (label_mode == 0 && !label_std) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((rows + 3) / 4, 1)), block(256);
    if (label_mode == 0) KALLE_LAUNCH(gauss_kl2_fwd_kernel<0>, grid, block, 0, st, pred, label_mean, label_std, mask_a, mask_b, sums4, std_mult, rows, dim);
    else KALLE_LAUNCH(gauss_kl2_fwd_kernel<1>, grid, block, 0, st, pred, label_mean, label_std, mask_a, mask_b, sums4, std_mult, rows, dim);
    return kalle_check_launch();
}

extern "C" int kalle_gauss_kl2_bwd(const float* pred, const float* label_mean, const float* label_std, int label_mode,
                                   float std_mult, const float* mask_a, const float* mask_b, const float* sums4,
                                   const float* grad_a, const float* grad_b, float* dpred, int64_t rows, int dim,
                                   void* stream) {
    if (!pred || !label_mean || !mask_a || !mask_b || !sums4 || !grad_a || !grad_b || !dpred || rows <= 0 || dim <= 0 ||
        !(std_mult > 0.f))
        return KALLE_ERR_ARG;
    if (label_mode != 0 && label_mode != 1) return KALLE_ERR_ARG;
    if (label_mode == 0 && !label_std) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(rows * dim, 256)), block(256);
    if (label_mode == 0) KALLE_LAUNCH(gauss_kl2_bwd_kernel<0>, grid, block, 0, st, pred, label_mean, label_std, mask_a, mask_b, sums4, grad_a, grad_b, dpred, std_mult, rows, dim);
    else KALLE_LAUNCH(gauss_kl2_bwd_kernel<1>, grid, block, 0, st, pred, label_mean, label_std, mask_a, mask_b, sums4, grad_a, grad_b, dpred, std_mult, rows, dim);
    return kalle_check_launch();
}

// ---- packed prefill: the k|v windows of several prompts' packed rows into their rows of a batch KV cache, one launch -----------
// blockIdx.y = sequence, blockIdx.x = a chunk of KALLE_KV_APPEND_ROWS of its rows; a lane moves 16 bytes (8 bf16) at a time.
namespace {
struct KvAppendTab {
    int row0[KALLE_DECODE_MAX_ROWS], len[KALLE_DECODE_MAX_ROWS], dst[KALLE_DECODE_MAX_ROWS], t0[KALLE_DECODE_MAX_ROWS];
};
__global__ __launch_bounds__(256) void kv_append_varlen_kernel(const bf16_t* __restrict__ src, int64_t ld_src, int src_off,
                                                               bf16_t* __restrict__ cache, int64_t cache_row_stride, int kvw,
                                                               KvAppendTab tab) {
    const int s = blockIdx.y;
    const int j0 = blockIdx.x * KALLE_KV_APPEND_ROWS;
    const int len = tab.len[s];
    if (j0 >= len) return;
    const int nrows = len - j0 < KALLE_KV_APPEND_ROWS ? len - j0 : KALLE_KV_APPEND_ROWS;
    const int vpr = kvw >> 3;                      // 16-byte units per row
    const bf16_t* sp = src + (int64_t)(tab.row0[s] + j0) * ld_src + src_off;
    bf16_t* dp = cache + (int64_t)tab.dst[s] * cache_row_stride + (int64_t)(tab.t0[s] + j0) * kvw;
    for (int i = threadIdx.x; i < nrows * vpr; i += blockDim.x) {
        const int r = i / vpr, c = (i - r * vpr) << 3;
        *reinterpret_cast<i32x4*>(dp + (int64_t)r * kvw + c) = *reinterpret_cast<const i32x4*>(sp + (int64_t)r * ld_src + c);
    }
}
}  // namespace

extern "C" int kalle_kv_append_varlen(const void* src, int64_t ld_src, int src_off, void* cache, int64_t cache_row_stride,
                                      int kvw, int nseq, const int32_t* row0_host, const int32_t* len_host,
                                      const int32_t* dst_row_host, const int32_t* t0_host, int total_rows, int R, int cache_rows,
                                      void* stream) {
    if (!src || !cache || !row0_host || !len_host || !dst_row_host || !t0_host) return KALLE_ERR_ARG;
    if (nseq < 1 || nseq > KALLE_DECODE_MAX_ROWS || R < 1 || R > KALLE_DECODE_MAX_ROWS || total_rows <= 0 || cache_rows <= 0)
        return KALLE_ERR_ARG;
    if (kvw <= 0 || (kvw & 7) || ld_src <= 0 || (ld_src & 7) || src_off < 0 || (src_off & 7) || cache_row_stride <= 0 ||
        (cache_row_stride & 7))
        return KALLE_ERR_ARG;
    if ((int64_t)src_off + kvw > ld_src || cache_row_stride < (int64_t)cache_rows * kvw) return KALLE_ERR_ARG;
    if ((((uintptr_t)src | (uintptr_t)cache) & 15) != 0) return KALLE_ERR_ARG;      // (16-byte loads and stores)
    KvAppendTab tab{};
    unsigned taken = 0;
    int maxlen = 0;
    int64_t next = 0;                              // the first packed row the next sequence may own
    for (int s = 0; s < nseq; ++s) {
        const int64_t r0 = row0_host[s], n = len_host[s], d = dst_row_host[s], t = t0_host[s];
        if (n <= 0 || t < 0 || t + n > cache_rows) return KALLE_ERR_ARG;
        if (d < 0 || d >= R || (taken >> d & 1u)) return KALLE_ERR_ARG;
        if (r0 < next || r0 + n > total_rows) return KALLE_ERR_ARG;
        taken |= 1u << d;
        next = r0 + n;
        tab.row0[s] = (int)r0; tab.len[s] = (int)n; tab.dst[s] = (int)d; tab.t0[s] = (int)t;
        maxlen = (int)n > maxlen ? (int)n : maxlen;
    }
    const dim3 grid((maxlen + KALLE_KV_APPEND_ROWS - 1) / KALLE_KV_APPEND_ROWS, nseq), block(256);
    KALLE_LAUNCH(kv_append_varlen_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(src),
                 ld_src, src_off, static_cast<bf16_t*>(cache), cache_row_stride, kvw, tab);
    return kalle_check_launch();
}
