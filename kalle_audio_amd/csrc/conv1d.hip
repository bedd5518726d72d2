// 1-D convolution stacks of the audio VAEs (gfx950, vector ALUs only - no MFMA, per the north-star spec):
// weight-norm fold, input activation (SnakeBeta / ELU / LeakyReLU / WaveNet gate) fused into the input staging,
// dilated / strided / causal conv and transposed conv, and (conv + bias + residual) * scale (+= y) -> activation -> tanh
// fused into the store.
// Reference: stable_audio_tools/models/autoencoders.py:39-62 (ResidualUnit), 64-81 (EncoderBlock), 83-114
// (DecoderBlock), 116-191 (Oobleck encoder/decoder); blocks.py:301-339 (SnakeBeta); dac.nn.layers.WNConv1d ->
// torch.nn.utils.weight_norm (w = g * v / ||v||, norm over all dims but 0); backup/flows.py (mel-VAE).
//
// Layout: activations (B, C, L) row-major (L contiguous, as torch), fp32 or bf16; weights are repacked once per
// forward by kalle_weight_norm_fold into [Cin][K][CoutP] fp32 (CoutP = Cout rounded up to 8).
//
// Main kernels ("v2", stride-1 conv and every transposed conv): a wave owns 8 output channels for 64*LPT positions;
// lane l handles positions l, l+64, ... so every LDS read of the input span is lane-consecutive (conflict-free for any
// dilation / alignment); the 8 weights of a (ci, tap) are wave-uniform, so they are fetched with SCALAR loads straight
// from the packed array (scalar cache / L2) and feed v_pk_fma_f32 as SGPR operands - no LDS traffic for weights.  The
// input span is staged through registers (global loads of chunk n+1 in flight while chunk n is computed), activated when
// it is written to LDS, double-buffered, one barrier per 8-channel chunk; the (channel, tap) loop is software-pipelined by
// hand (loads of step t+1 issued right after the wait for step t).  A transposed conv of stride S is S independent
// ceil(K/S)-tap convolutions (one per output phase) run back to back by the same workgroup.
// Fallback kernels ("v1": strided conv, gated input, mixed dtypes): 64 co x 64 positions per workgroup, 4x4 per thread.
#include <cstdlib>
#include <initializer_list>
#include <type_traits>
#include "common.h"
#include "../../include/kalle_hip.h"

namespace {

constexpr int CO_T = 64, L_T = 64, CI_T = 8;
constexpr int MAX_SPAN = 576;   // (L_T-1)*stride + (K-1)*dil + 1 must fit
constexpr int MAX_K = 16;

__device__ __forceinline__ float fast_sin(float x) {   // v_sin_f32 takes revolutions; fract() does the range reduction
    const float r = x * 0.15915494309189535f;
    return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r));
}
// act: 1 snake(-beta) x + sin^2(a x) * inv_b, 2 ELU, 3 LeakyReLU(a)
__device__ __forceinline__ float act_apply(float x, int act, float a, float inv_b) {
    if (act == 1) {
        const float s = fast_sin(x * a);
        return x + inv_b * s * s;
    }
    if (act == 2) return x > 0.f ? x : (__expf(x) - 1.f);
    if (act == 3) return x > 0.f ? x : x * a;
    return x;
}

template <bool F32>
__device__ __forceinline__ float ld1(const void* p, int64_t i) {
    if constexpr (F32) return static_cast<const float*>(p)[i];
    else return bf16_to_f32(static_cast<const bf16_t*>(p)[i]);
}
template <bool F32>
__device__ __forceinline__ void st1(void* p, int64_t i, float v) {
    if constexpr (F32) static_cast<float*>(p)[i] = v;
    else static_cast<bf16_t*>(p)[i] = f32_to_bf16(v);
}

struct ConvParams {
    const void* x; const float* w; const float* bias; const void* res; void* y;
    int B, Cin, Lin, Cout, Lout, K, stride, pad, dil, act, post;   // post bits: 1 tanh, 2 accumulate into y
    const float* aa; const float* ab; int logscale;
    float act_param;
    float out_scale;
    int CoutP;  // row stride of the packed weights = Cout rounded up to 8 (pad columns are zero)
    int xC;     // channels of the x tensor (2*Cin for the gated activation, else Cin)
    int pact; const float* paa; const float* pab; int plogscale; float pparam;   // activation applied to the output
    void* y_raw;               // dual output: the un-activated value also goes here (same shape / dtype as y)
    int nco, ntile, co_fast;   // v2 grid: blockIdx.x enumerates (position tile, channel tile), channel tile fastest if co_fast
};
// Ragged batch: row b is a tensor of lens_in[b] inputs and lens_out[b] outputs inside its [Lin] / [Lout] row - inputs at or past
// lens_in[b] read as zero, outputs at or past lens_out[b] are not stored.  Every kernel is a template on LENS: the dense
// instantiation takes ConvParams and its code knows nothing of lengths (the same instruction stream as before lengths existed),
// the LENS one takes ConvParamsL.  (host side: lens_out == NULL means dense)
struct ConvParamsL : ConvParams { const int* lens_in; const int* lens_out; };
template <bool LENS> using ConvArgs = std::conditional_t<LENS, ConvParamsL, ConvParams>;

// (conv + bias + residual) * out_scale (+= y) -> post activation -> tanh -> store
template <bool XF32, bool YF32, bool RES = true>
__device__ __forceinline__ void conv_store(const ConvParams& p, int co, int64_t oi, float v, float bv, float pa,
                                           float pinv_b) {
    v += bv;
    if (RES && p.res) v += ld1<XF32>(p.res, oi);
    v *= p.out_scale;
    if (p.post & 2) v += ld1<YF32>(p.y, oi);
    if (p.y_raw) st1<YF32>(p.y_raw, oi, v);         // consumers that need the raw value (residual paths)
    if (p.pact) v = act_apply(v, p.pact, pa, pinv_b);
    if (p.post & 1) v = tanhf(v);
    st1<YF32>(p.y, oi, v);
}
__device__ __forceinline__ void post_act_params(const ConvParams& p, int co, float& pa, float& pinv_b) {
    pa = p.pparam;
    pinv_b = 0.f;
    if (p.pact == 1) {
        pa = p.paa[co];
        float bb = p.pab[co];
        if (p.plogscale) { pa = __expf(pa); bb = __expf(bb); }
        pinv_b = 1.f / (bb + 1e-9f);
    }
}

template <bool XF32, bool YF32, bool LENS = false>
__global__ __launch_bounds__(256) void conv1d_kernel(ConvArgs<LENS> p) {
    __shared__ float Xs[CI_T][MAX_SPAN];
    __shared__ __attribute__((aligned(16))) float Ws[CI_T][MAX_K][CO_T];
    const int tid = threadIdx.x;
    const int tc = tid & 15, tl = tid >> 4;           // 16 channel groups x 16 position groups
    const int b = blockIdx.z, co0 = blockIdx.y * CO_T, l0 = blockIdx.x * L_T;
    int lin_b = 0, lout_b = 0;                        // this row's lengths (LENS only)
    if constexpr (LENS) {
        lin_b = p.lens_in[b]; lout_b = p.lens_out[b];
        if (l0 >= lout_b) return;                     // nothing to store: leave before staging anything
    }
    const int span = (L_T - 1) * p.stride + (p.K - 1) * p.dil + 1;
    const int in0 = l0 * p.stride - p.pad;            // input position of span element 0

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int ci0 = 0; ci0 < p.Cin; ci0 += CI_T) {
        __syncthreads();
        // stage activated input span: consecutive threads -> consecutive positions (coalesced)
        for (int idx = tid; idx < CI_T * span; idx += 256) {
            const int c = idx / span, sp = idx - c * span;
            const int ci = ci0 + c, li = in0 + sp;
            float v = 0.f;
            if (ci < p.Cin && li >= 0 && li < (LENS ? lin_b : p.Lin)) {
                const int64_t xi = ((int64_t)b * p.xC + ci) * p.Lin + li;
                v = ld1<XF32>(p.x, xi);
                if (p.act == 1) {
                    float a = p.aa[ci], bb = p.ab[ci];
                    if (p.logscale) { a = __expf(a); bb = __expf(bb); }
                    v = act_apply(v, 1, a, 1.f / (bb + 1e-9f));
                } else if (p.act == 4) {  // WaveNet gate: tanh(x[ci]) * sigmoid(x[Cin + ci])
                    const float gt = ld1<XF32>(p.x, xi + (int64_t)p.Cin * p.Lin);
                    v = tanhf(v) / (1.f + __expf(-gt));
                } else if (p.act >= 2) {
                    v = act_apply(v, p.act, p.act_param, 0.f);
                }
            }
            Xs[c][sp] = v;
        }
        // stage weights [ci][k][co] (contiguous in co)
        for (int idx = tid; idx < CI_T * p.K * CO_T; idx += 256) {
            const int co = idx & (CO_T - 1);
            const int ck = idx >> 6;
            const int c = ck / p.K, k = ck - c * p.K;
            const int ci = ci0 + c;
            float v = 0.f;
            if (ci < p.Cin && co0 + co < p.Cout) v = p.w[((int64_t)ci * p.K + k) * p.CoutP + co0 + co];
            Ws[c][k][co] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < CI_T; ++c) {
            for (int k = 0; k < p.K; ++k) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(&Ws[c][k][4 * tc]);
                const int xb = (4 * tl) * p.stride + k * p.dil;
                float xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = Xs[c][xb + j * p.stride];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(wv[i], xv[j], acc[i][j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + 4 * tc + i;
        if (co >= p.Cout) continue;
        const float bv = p.bias ? p.bias[co] : 0.f;
        float pa, pinv_b;
        post_act_params(p, co, pa, pinv_b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = l0 + 4 * tl + j;
            if (l >= (LENS ? lout_b : p.Lout)) continue;
            conv_store<XF32, YF32>(p, co, ((int64_t)b * p.Cout + co) * p.Lout + l, acc[i][j], bv, pa, pinv_b);
        }
    }
}

// transposed conv: y[b,co,lo] = bias + sum_ci sum_k act(x)[b,ci,li] w[ci,k,co],  lo = li*stride - pad + k
template <bool XF32, bool YF32, bool LENS = false>
__global__ __launch_bounds__(256) void convT1d_kernel(ConvArgs<LENS> p) {
    __shared__ float Xs[CI_T][L_T + 8];
    __shared__ __attribute__((aligned(16))) float Ws[CI_T][MAX_K + 2][CO_T];
    const int tid = threadIdx.x;
    const int tc = tid & 15, tl = tid >> 4;
    const int b = blockIdx.z, co0 = blockIdx.y * CO_T, l0 = blockIdx.x * L_T;
    int lin_b = 0, lout_b = 0;
    if constexpr (LENS) {
        lin_b = p.lens_in[b]; lout_b = p.lens_out[b];
        if (l0 >= lout_b) return;
    }
    // input positions that can reach outputs [l0, l0+L_T): li in [floor((l0+pad-K+1)/s), floor((l0+L_T-1+pad)/s)]
    int li_lo = l0 + p.pad - p.K + 1;
    li_lo = li_lo >= 0 ? li_lo / p.stride : -((-li_lo + p.stride - 1) / p.stride);
    const int li_hi = (l0 + L_T - 1 + p.pad) / p.stride;
    const int nli = li_hi - li_lo + 1;  // <= L_T/stride + K/stride + 2 <= L_T + 8 for stride >= 1, K <= 2*stride+1

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int ci0 = 0; ci0 < p.Cin; ci0 += CI_T) {
        __syncthreads();
        for (int idx = tid; idx < CI_T * nli; idx += 256) {
            const int c = idx / nli, sp = idx - c * nli;
            const int ci = ci0 + c, li = li_lo + sp;
            float v = 0.f;
            if (ci < p.Cin && li >= 0 && li < (LENS ? lin_b : p.Lin)) {
                v = ld1<XF32>(p.x, ((int64_t)b * p.Cin + ci) * p.Lin + li);
                if (p.act == 1) {
                    float a = p.aa[ci], bb = p.ab[ci];
                    if (p.logscale) { a = __expf(a); bb = __expf(bb); }
                    v = act_apply(v, 1, a, 1.f / (bb + 1e-9f));
                } else if (p.act >= 2) {
                    v = act_apply(v, p.act, p.act_param, 0.f);
                }
            }
            Xs[c][sp] = v;
        }
        for (int idx = tid; idx < CI_T * p.K * CO_T; idx += 256) {
            const int co = idx & (CO_T - 1);
            const int ck = idx >> 6;
            const int c = ck / p.K, k = ck - c * p.K;
            const int ci = ci0 + c;
            float v = 0.f;
            if (ci < p.Cin && co0 + co < p.Cout) v = p.w[((int64_t)ci * p.K + k) * p.CoutP + co0 + co];
            Ws[c][k][co] = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lo = l0 + 4 * tl + j;
            const int t = lo + p.pad;
            const int r = t % p.stride;            // first tap
            const int lif = t / p.stride;          // its input position
            for (int k = r, m = 0; k < p.K; k += p.stride, ++m) {
                const int sp = lif - m - li_lo;
                if (sp < 0 || sp >= nli) continue;
#pragma unroll 4
                for (int c = 0; c < CI_T; ++c) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(&Ws[c][k][4 * tc]);
                    const float xv = Xs[c][sp];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = fmaf(wv[i], xv, acc[i][j]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + 4 * tc + i;
        if (co >= p.Cout) continue;
        const float bv = p.bias ? p.bias[co] : 0.f;
        float pa, pinv_b;
        post_act_params(p, co, pa, pinv_b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int l = l0 + 4 * tl + j;
            if (l >= (LENS ? lout_b : p.Lout)) continue;
            conv_store<XF32, YF32>(p, co, ((int64_t)b * p.Cout + co) * p.Lout + l, acc[i][j], bv, pa, pinv_b);
        }
    }
}



// ------------------------------------------------------------------------------------------------ v2 core
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float* cfloat_p;   // constant address space: uniform loads become SMEM

struct ConvPass {        // one pass of the core = one output phase
    int in0;             // x index of span slot 0
    int span;            // slots to stage (<= SPAN)
    int xs0;             // span slot read by tap 0 at local position 0
    int ntaps;           // taps per input channel (K, or the taps of this phase of a transposed conv)
    int S;               // input phases of a strided conv (1 otherwise): x index i is staged at LDS slot
                         // (i - in0) % S * pspan + (i - in0) / S, so a tap reads lane-consecutive slots at any stride
    int lgS, pspan, ph0; // log2(S), slots per phase row, phase of tap 0
    int xtap;            // slot advance per tap inside a phase run (S > 1: pspan = next phase)
    int xtap_wrap;       // slot advance when the phase wraps (S == 1: every tap - the dilation, or -1)
    int64_t w0;          // first weight row of ci = 0, in rows of CoutP
    int64_t wtap, wchan; // weight row advance per tap / from the last tap of ci to the first tap of ci + 1
    int64_t o0;          // output position of local position 0
    int ostride;         // output positions per local position (1, or the stride of a transposed conv)
};

// COW output channels per wave, 64*LPT positions per wave; WCO of the NW waves are spread over output channels, the other
// NW/WCO over positions (tiny-Cout layers: WCO = 1); CI input channels per staged chunk; SPAN = LDS row length.
// NW = 8 (512 threads) stages x once for 128 output channels: half the x traffic and half the staging instructions per
// FMA of the 4-wave tiling - what the HBM-side pointwise (k = 1) convs need.
template <int COW, int LPT, int WCO, int CI, int SPAN, bool XF32, bool YF32, int NW = 4, bool LENS = false>
__device__ __forceinline__ void conv_core(const ConvParams& p, const ConvPass& g, float (*Xs)[SPAN], int b, int co_w,
                                          int lane, int wave, int wave_l, int lin_b = 0, int lout_b = 0) {   // row b's lengths (LENS)
    constexpr int LW = 64 * LPT;
    constexpr int NS = SPAN / 64;                     // span slots per lane
    constexpr int NH = CI / NW;                       // channels of a chunk staged by one wave
    const int nchunks = (p.Cin + CI - 1) / CI;

    f32x2 acc[COW][LPT / 2];                          // packed along positions: (l_2j, l_2j+1) share one v_pk_fma_f32
#pragma unroll
    for (int i = 0; i < COW; ++i)
#pragma unroll
        for (int j = 0; j < LPT / 2; ++j) acc[i][j] = f32x2{0.f, 0.f};
    // the residual is loaded straight into the accumulators up front (all loads in flight together, their latency hidden
    // behind the first chunk) - in the store loop every load would sit behind the previous store (they may alias)
    if (p.res) {                                      // clamped addresses, no branches: invalid lanes are never stored
#pragma unroll
        for (int i = 0; i < COW; ++i) {
            const int64_t rb = ((int64_t)b * p.Cout + min(co_w + i, p.Cout - 1)) * p.Lout;
#pragma unroll
            for (int j = 0; j < LPT / 2; ++j) {
                const int64_t la = g.o0 + (int64_t)(wave_l * LW + lane + 128 * j) * g.ostride;
                const int64_t lb = la + 64 * g.ostride;
                const float ra = ld1<XF32>(p.res, rb + min(max(la, (int64_t)0), (int64_t)p.Lout - 1));
                const float rc = ld1<XF32>(p.res, rb + min(max(lb, (int64_t)0), (int64_t)p.Lout - 1));
                acc[i][j] = f32x2{ra, rc};
            }
        }
    }

    float stg[NH][NS];                                // wave w stages channels w, w+NW, ... of a chunk
    float s_a[NH], s_b[NH];                           // their activation parameters (scalar loads, issued with the data)
    const cfloat_p aa_c = reinterpret_cast<cfloat_p>(reinterpret_cast<uintptr_t>(p.aa));
    const cfloat_p ab_c = reinterpret_cast<cfloat_p>(reinterpret_cast<uintptr_t>(p.ab));
    auto gload = [&](int ci0) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int ci = ci0 + wave + NW * h;
            if (p.act == 1) {
                s_a[h] = aa_c[min(ci, p.Cin - 1)];
                s_b[h] = ab_c[min(ci, p.Cin - 1)];
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int sp = lane + 64 * s, li = g.in0 + sp;
                float v = 0.f;
                if (sp < g.span && ci < p.Cin && li >= 0 && li < (LENS ? lin_b : p.Lin))
                    v = ld1<XF32>(p.x, ((int64_t)b * p.xC + ci) * p.Lin + li);
                stg[h][s] = v;
            }
        }
    };
    auto lstore = [&](int ci0, int buf) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int c = wave + NW * h, ci = ci0 + c;
            float a = p.act_param, inv_b = 0.f;
            if (p.act == 1) {
                a = s_a[h];
                float bb = s_b[h];
                if (p.logscale) { a = __expf(a); bb = __expf(bb); }
                inv_b = 1.f / (bb + 1e-9f);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int sp = lane + 64 * s, li = g.in0 + sp;
                if (sp < g.span) {
                    float v = stg[h][s];
                    if (p.act && ci < p.Cin && li >= 0 && li < (LENS ? lin_b : p.Lin)) v = act_apply(v, p.act, a, inv_b);
                    const int slot = g.S == 1 ? sp : (sp & (g.S - 1)) * g.pspan + (sp >> g.lgS);
                    Xs[buf * CI + c][slot] = v;
                }
            }
        }
    };
    // A wave whose channel group lies wholly beyond the packed row (Cout = 16 under a 32-channel workgroup: waves 2, 3) still
    // runs the loop for the barriers and the staging; its weight reads are redirected to column 0 - read at co_w they would
    // run up to COW floats past the END of the array on the last (ci, tap) row (a fault when the array ends a mapped segment).
    // (A group that is partly valid needs CoutP % COW == 0: pick_tile only offers COW = 16 then.)
    const int co_ld = co_w + COW <= p.CoutP ? co_w : 0;
    const cfloat_p wbase = reinterpret_cast<cfloat_p>(reinterpret_cast<uintptr_t>(p.w)) + co_ld;
    const cfloat_p wlast = wbase + ((int64_t)p.Cin * p.K - 1) * p.CoutP;
    const int nwrap = (g.ph0 + g.ntaps - 1) / g.S;   // phase wraps among the ntaps-1 advances of one channel
    const int xwrap = SPAN - ((g.ntaps - 1 - nwrap) * g.xtap + nwrap * g.xtap_wrap);
    const int64_t wtap = g.wtap * p.CoutP, wchan = g.wchan * p.CoutP;

    // The scalar weight loads only run one step ahead, so they must hit in L2: every thread touches one 64-B line of the
    // NEXT chunk's weight rows with a vector load (same vmcnt batch as the x loads), which pulls the rows of all four
    // waves from HBM / MALL into this XCD's L2 a whole chunk before they are needed.
    constexpr int LPR = WCO * COW * 4 / 64 > 0 ? WCO * COW * 4 / 64 : 1;   // 64-B lines per weight row of this workgroup
    float wt0 = 0.f, wt1 = 0.f;                       // touched values: consumed (= waited for) only at the next lstore
    auto wprefetch = [&](int ci0) {
        const int per_c = g.ntaps * LPR;
        const int total = min(CI, p.Cin - ci0) * per_c;
        const int co_g = co_w - (wave % WCO) * COW;
        auto touch = [&](int idx) {
            idx = idx < total ? idx : 0;              // clamped, branch-free: a redundant touch of the first line
            const int c = idx / per_c, rem = idx - c * per_c;
            const int m = rem / LPR;
            int col = co_g + 16 * (rem - m * LPR);
            col = col < p.CoutP ? col : co_g;
            const int64_t row = min(g.w0 + (int64_t)(ci0 + c) * p.K + (int64_t)m * g.wtap, (int64_t)p.Cin * p.K - 1);
            return p.w[row * p.CoutP + col];
        };
        if (total > 0) {
            wt0 = touch(threadIdx.x);
            wt1 = touch(threadIdx.x + 64 * NW);
        }
    };
    auto consume_touch = [&]() { asm volatile("" ::"v"(wt0), "v"(wt1)); };

    wprefetch(0);
    gload(0);
    consume_touch();
    if (nchunks > 1) wprefetch(CI);
    lstore(0, 0);
    __syncthreads();
    for (int n = 0; n < nchunks; ++n) {
        const int ci0 = n * CI, buf = n & 1;
        if (n + 1 < nchunks) {
            consume_touch();                             // (loads issued a whole chunk ago)
            if (n + 2 < nchunks) wprefetch(ci0 + 2 * CI);
            gload(ci0 + CI);
        }
        const int cmax = min(CI, p.Cin - ci0);
        // flattened (channel, tap) loop, software-pipelined by hand: the loads of step t+1 are issued right after the
        // wait for step t's operands, so LDS + scalar-cache latency hides behind the packed FMAs of step t.
        // (scalar loads return out of order, so any wait on them is lgkmcnt(0): the wait must precede the prefetch.)
        const int T = cmax * g.ntaps;
        cfloat_p wr = wbase + (g.w0 + (int64_t)ci0 * p.K) * p.CoutP;
        if (wr > wlast) wr = wlast;
        const float* xs = &Xs[buf * CI][g.xs0 + wave_l * LW + lane];
        int kk = 0, ph = g.ph0;
        f32x2 w0[COW / 2], w1[COW / 2];
        f32x2 x0[LPT / 2], x1[LPT / 2];
        auto ld = [&](f32x2 (&w)[COW / 2], f32x2 (&x)[LPT / 2]) {
#pragma unroll
            for (int i = 0; i < COW / 2; ++i) w[i] = f32x2{wr[2 * i], wr[2 * i + 1]};
#pragma unroll
            for (int j = 0; j < LPT / 2; ++j) x[j] = f32x2{xs[128 * j], xs[128 * j + 64]};
            if (++kk == g.ntaps) {
                kk = 0; ph = g.ph0; xs += xwrap; wr += wchan;
            } else {
                wr += wtap;
                if (++ph == g.S) { ph = 0; xs += g.xtap_wrap; } else xs += g.xtap;
            }
            if (wr > wlast) wr = wlast;              // the one-step-ahead prefetch never leaves the array
        };
        // acc(l_2j, l_2j+1) += w_i * (x_2j, x_2j+1): the weight is one half of an SGPR pair, broadcast by op_sel (hipcc
        // would copy odd weights into even SGPRs first, which makes it wait on the prefetch it has just issued)
        auto fma = [&](const f32x2 (&w)[COW / 2], const f32x2 (&x)[LPT / 2]) {
#pragma unroll
            for (int j = 0; j < LPT / 2; ++j)
#pragma unroll
                for (int i = 0; i < COW / 2; ++i) {
                    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc[2 * i][j]) : "s"(w[i]), "v"(x[j]));
                    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]"
                        : "+v"(acc[2 * i + 1][j]) : "s"(w[i]), "v"(x[j]));
                }
        };
        auto wait_lgkm = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
            __builtin_amdgcn_sched_barrier(0);
        };
        if (T > 0) {
            ld(w0, x0);
            int t = 0;
            for (; t + 2 <= T; t += 2) {
                wait_lgkm();
                ld(w1, x1);
                fma(w0, x0);
                wait_lgkm();
                ld(w0, x0);                          // step t+2 (may be one past the chunk: unused)
                fma(w1, x1);
            }
            if (t < T) fma(w0, x0);
        }
        if (n + 1 < nchunks) lstore(ci0 + CI, buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < COW; ++i) {
        const int co = co_w + i;
        if (co >= p.Cout) continue;
        const float bv = p.bias ? p.bias[co] : 0.f;
        float pa, pinv_b;
        post_act_params(p, co, pa, pinv_b);
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int64_t l = g.o0 + (int64_t)(wave_l * LW + lane + 64 * j) * g.ostride;
            if (l < 0 || l >= (LENS ? lout_b : p.Lout)) continue;
            conv_store<XF32, YF32, false>(p, co, ((int64_t)b * p.Cout + co) * p.Lout + l, acc[i][j >> 1][j & 1], bv, pa,
                                          pinv_b);
        }
    }
}

template <int COW, int LPT, int WCO, int CI, int SPAN, bool XF32, bool YF32, int NW = 4, bool LENS = false>
__global__ __launch_bounds__(64 * NW) void conv1d_v2_kernel(ConvArgs<LENS> p) {
    constexpr int LT = 64 * LPT * (NW / WCO);
    __shared__ float Xs[2 * CI + 1][SPAN];           // two buffers + one pad row for the one-step-ahead prefetch
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bt = p.co_fast ? blockIdx.x / p.nco : blockIdx.x % p.ntile;
    const int bc = p.co_fast ? blockIdx.x % p.nco : blockIdx.x / p.ntile;
    const int l0 = bt * LT;
    int lin_b = 0, lout_b = 0;
    if constexpr (LENS) {
        lin_b = p.lens_in[blockIdx.z]; lout_b = p.lens_out[blockIdx.z];
        if (l0 >= lout_b) return;                     // the whole position tile is past the row's end (or the row inactive)
    }
    ConvPass g;
    g.ntaps = p.K;
    g.w0 = 0;
    g.wtap = 1;
    g.wchan = 1;
    g.o0 = l0;
    g.ostride = 1;
    if (p.stride == 1) {
        g.S = 1; g.lgS = 0; g.pspan = 0; g.ph0 = 0;
        g.in0 = l0 - p.pad;
        g.span = (LT - 1) + (p.K - 1) * p.dil + 1;
        g.xs0 = 0;
        g.xtap = 0;
        g.xtap_wrap = p.dil;
    } else {                                          // power-of-two stride, dilation 1 (host-checked)
        const int S = p.stride;
        const int padq = (p.pad + S - 1) / S;         // in0 is a multiple of S: tap k of local position l sits at slot l*S + k + d
        const int d = padq * S - p.pad;
        g.S = S; g.lgS = 31 - __builtin_clz(S);
        g.pspan = LT + 64 / S;                        // (pspan mod 64) = 64/S: the de-interleaving LDS writes are conflict-free
        g.ph0 = d;
        g.in0 = (l0 - padq) * S;
        g.span = (LT - 1) * S + p.K + d;
        g.xs0 = d * g.pspan;
        g.xtap = g.pspan;
        g.xtap_wrap = 1 - (S - 1) * g.pspan;
    }
    if constexpr (LENS)
        conv_core<COW, LPT, WCO, CI, SPAN, XF32, YF32, NW, true>(p, g, Xs, blockIdx.z, bc * (WCO * COW) + (wave % WCO) * COW, lane,
                                                                      wave, wave / WCO, lin_b, lout_b);
    else
        conv_core<COW, LPT, WCO, CI, SPAN, XF32, YF32, NW>(p, g, Xs, blockIdx.z, bc * (WCO * COW) + (wave % WCO) * COW, lane,
                                                                wave, wave / WCO);
}

// transposed conv: output lo = q*S + r - pad (phase r < S, input position q):
//   y[q*S + r - pad] = sum_ci sum_m x[q - m] w[ci, r + m*S, co],  m < ceil((K - r)/S)
// i.e. S independent ceil(K/S)-tap convolutions whose outputs interleave.  One workgroup = one phase of one
// (64*LPT*(4/WCO) input positions q) x (channel tile).  Workgroup ids are laid out so that the S phases of a tile differ
// by multiples of 8: the hardware deals consecutive ids round-robin to the 8 XCDs, so all phases of a tile run on the
// SAME XCD within a few ids of each other and their interleaved 4-byte stores merge in that XCD's L2 before write-back.
template <int COW, int LPT, int WCO, int CI, int SPAN, bool XF32, bool YF32, bool LENS = false>
__global__ __launch_bounds__(256) void convT1d_v2_kernel(ConvArgs<LENS> p) {
    constexpr int LT = 64 * LPT * (4 / WCO);
    __shared__ float Xs[2 * CI + 1][SPAN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int S = p.stride;
    const int n = blockIdx.x;
    const int r = (n >> 3) % S;
    const int tile = (n / (8 * S)) * 8 + (n & 7);    // (position tile, channel tile) pair, position tiles fastest
    if (tile >= p.ntile * p.nco) return;
    const int bt = tile % p.ntile, bc = tile / p.ntile;
    const int q0 = bt * LT;
    const int mmax = (p.K + S - 1) / S;
    ConvPass g;
    g.ntaps = r < p.K ? (p.K - r + S - 1) / S : 0;
    g.in0 = q0 - (mmax - 1);
    g.span = LT + mmax - 1;
    g.xs0 = mmax - 1;
    g.S = 1; g.lgS = 0; g.pspan = 0; g.ph0 = 0;
    g.xtap = 0;
    g.xtap_wrap = -1;
    g.w0 = r;
    g.wtap = S;
    g.wchan = p.K - (int64_t)(g.ntaps - 1) * S;
    g.o0 = (int64_t)q0 * S + r - p.pad;
    g.ostride = S;
    if constexpr (LENS) {
        const int lin_b = p.lens_in[blockIdx.z], lout_b = p.lens_out[blockIdx.z];
        if (g.o0 >= lout_b) return;                   // o0 is the lowest output of this (tile, phase)
        conv_core<COW, LPT, WCO, CI, SPAN, XF32, YF32, 4, true>(p, g, Xs, blockIdx.z, bc * (WCO * COW) + (wave % WCO) * COW, lane,
                                                                     wave, wave / WCO, lin_b, lout_b);
    } else {
        conv_core<COW, LPT, WCO, CI, SPAN, XF32, YF32>(p, g, Xs, blockIdx.z, bc * (WCO * COW) + (wave % WCO) * COW, lane,
                                                            wave, wave / WCO);
    }
}

// ------------------------------------------------------------------------------------------------ few positions, many channels
// The top of the VAE (C = 512 .. 2048 at a few hundred to a few thousand positions - all of a single-clip decode) does not
// have enough positions to fill 256 CUs with the position-per-lane tiling above.  Here the roles are swapped: a LANE owns 4
// output channels (a wave 256 of them) and 16 consecutive positions live in its accumulators; the weights of a (ci, tap)
// step are then a coalesced 16-byte-per-lane VECTOR load from the packed [Cin][K][CoutP] array (prefetched 4 steps ahead,
// counted vmcnt), and the 16 input values of the step are wave-uniform: ONE scalar load from a zero-padded, already
// activated copy of x (kalle_conv_pad_act), fed to v_pk_fma_f32 as SGPR pairs.  No LDS, no barriers, waves independent.
// phases > 1 (strided conv): padded index j is stored at (j % phases) * (Lp / phases) + j / phases, so the inputs of a tap
// for consecutive outputs are consecutive
template <bool LENS>
__device__ __forceinline__ void pad_act_body(const float* __restrict__ x, float* __restrict__ xp, int C, int Lin,
                                             int Lp, int pad, int act, const float* __restrict__ aa,
                                             const float* __restrict__ ab, int logscale, float act_param,
                                             int phases, int gx, const int* __restrict__ lens) {
    const int row = blockIdx.x / gx;                // b * C + c (rows on grid x: B * C exceeds grid y's 65535 at 1024 channels x 64 chunks)
    const int bx = blockIdx.x - row * gx;
    const int c = row % C;
    int lin_b = 0;                                  // ragged batch: zeros from lens[b] on; an inactive row's copy is not made
    if constexpr (LENS) {
        lin_b = lens[row / C];
        if (lin_b == 0) return;
    }
    float a = act_param, inv_b = 0.f;
    if (act == 1) {
        a = aa[c];
        float bb = ab[c];
        if (logscale) { a = __expf(a); bb = __expf(bb); }
        inv_b = 1.f / (bb + 1e-9f);
    }
    for (int j = bx * 256 + threadIdx.x; j < Lp; j += gx * 256) {
        const int li = j - pad;
        float v = 0.f;
        if (li >= 0 && li < (LENS ? lin_b : Lin)) {
            v = x[(int64_t)row * Lin + li];
            if (act) v = act_apply(v, act, a, inv_b);
        }
        const int slot = phases == 1 ? j : (j % phases) * (Lp / phases) + j / phases;
        xp[(int64_t)row * Lp + slot] = v;
    }
}
__global__ __launch_bounds__(256) void pad_act_kernel(const float* __restrict__ x, float* __restrict__ xp, int C, int Lin,
                                                      int Lp, int pad, int act, const float* __restrict__ aa,
                                                      const float* __restrict__ ab, int logscale, float act_param,
                                                      int phases, int gx) {
    pad_act_body<false>(x, xp, C, Lin, Lp, pad, act, aa, ab, logscale, act_param, phases, gx, nullptr);
}
__global__ __launch_bounds__(256) void pad_act_lens_kernel(const float* __restrict__ x, float* __restrict__ xp, int C, int Lin,
                                                           int Lp, int pad, int act, const float* __restrict__ aa,
                                                           const float* __restrict__ ab, int logscale, float act_param,
                                                           int phases, int gx, const int* __restrict__ lens) {
    pad_act_body<true>(x, xp, C, Lin, Lp, pad, act, aa, ab, logscale, act_param, phases, gx, lens);
}

struct ConvCParams {
    const float* xp; const float* w; const float* bias; const float* res; float* y; float* y_raw;
    int B, Cin, Lp, Cout, CoutP, Lout, K, dil, post;
    int split;           // 1, 2 or 4 waves of a workgroup share one position tile and split the input channels
    int ks; float* part; // ks > 1: blockIdx.z = b * ks + slice - workgroups split the input channels too; each writes its raw
                         // partial sums to part[slice][b][co][l] and cfirst_finish_kernel applies bias / residual / epilogue
    // geometry of one pass: conv (nphase 1, taps K, weight row k, x offset k * dil, output l) or one phase r of a transposed
    // conv (taps ceil((K - r) / S), weight row r + m * S, x offset -m, output q * S + r - pad)
    int nphase, npos, xtap, ostride, opad, xlead;
    int xS, xLq, xph0;   // strided conv: input phases, phase-row length, phase of tap 0 (xS = 1 otherwise)
    float out_scale;
    int pact; const float* paa; const float* pab; int plogscale; float pparam;
};
struct ConvCParamsL : ConvCParams { const int* lens_out; };   // ragged batch: row b stores its first lens_out[b] outputs only
template <bool LENS> using ConvCArgs = std::conditional_t<LENS, ConvCParamsL, ConvCParams>;

template <bool LENS = false>
__global__ __launch_bounds__(256) void conv1d_cfirst_kernel(ConvCArgs<LENS> p) {
    constexpr int P = 16, D = 4;                    // positions per wave, weight prefetch depth
    __shared__ float red[3 * 64 * 64];              // partial accumulators of the input-channel splits (48 KiB)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.z / p.ks, ksl = blockIdx.z - b * p.ks;   // batch item, workgroup-level input-channel slice
    const int S = p.split;                          // waves per position tile
    const int sp = wave % S;                        // this wave's input-channel slice (within the workgroup's)
    const int ph = blockIdx.x % p.nphase;           // output phase (transposed conv), 0 otherwise
    const int l0 = ((blockIdx.x / p.nphase) * (4 / S) + wave / S) * P;   // first (input-side) position of the tile
    bool live_b = l0 < p.npos;                      // (whole tile groups stay together: sp-waves of a tile share `live`)
    int lout_b = 0;
    if constexpr (LENS) {                           // outputs of position q: q * ostride + ph - opad, rising with q
        lout_b = p.lens_out[b];
        const int64_t shift = p.nphase == 1 ? 0 : ph - p.opad;
        if ((int64_t)(blockIdx.x / p.nphase) * (4 / S) * P * p.ostride + shift >= lout_b) return;   // the workgroup's first tile is past the end
        live_b = live_b && (int64_t)l0 * p.ostride + shift < lout_b;
    }
    const bool live = live_b;
    const int co = blockIdx.y * 256 + 4 * lane;
    const int cw = min(co, p.CoutP - 4);            // clamped weight column (lanes past Cout are never stored)
    const int cper = (p.Cin + S * p.ks - 1) / (S * p.ks);
    const int ci_lo = min((ksl * S + sp) * cper, p.Cin), ci_hi = min(ci_lo + cper, p.Cin);
    const int kt = p.nphase == 1 ? p.K : (ph < p.K ? (p.K - ph + p.nphase - 1) / p.nphase : 0);   // taps of this pass
    const int wstep = p.nphase;                     // weight k advance per tap (1 for a conv)
    const int T = live ? (ci_hi - ci_lo) * kt : 0;
    const int64_t oo = p.nphase == 1 ? 0 : ph - p.opad;   // output index of position q: q * ostride + oo

    f32x2 acc[4][P / 2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < P / 2; ++j) acc[c][j] = f32x2{0.f, 0.f};
    if (p.res && sp == 0 && live && p.ks == 1) {    // residual straight into the accumulators (clamped, branch-free)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float* rp = p.res + ((int64_t)b * p.Cout + min(co + c, p.Cout - 1)) * p.Lout;
#pragma unroll
            for (int j = 0; j < P / 2; ++j) {
                const int64_t la = (int64_t)(l0 + 2 * j) * p.ostride + oo, lb = la + p.ostride;
                acc[c][j] = f32x2{rp[min(max(la, (int64_t)0), (int64_t)p.Lout - 1)],
                                  rp[min(max(lb, (int64_t)0), (int64_t)p.Lout - 1)]};
            }
        }
    }

    // weight row of step t = (ci, m): ci * K + ph + m * wstep;  x row offset: ci * Lp + xlead + m * xtap.  Both are walked
    // with running scalar pointers (adds only - recomputing them from (ci, m) costs ~40 scalar instructions per step)
    const cfloat_p xb = reinterpret_cast<cfloat_p>(reinterpret_cast<uintptr_t>(p.xp)) + (int64_t)b * p.Cin * p.Lp + l0;
    int64_t xoff = (int64_t)ci_lo * p.Lp + p.xlead;
    const int nwr = p.xS > 1 ? (p.xph0 + kt - 1) / p.xS : 0;          // phase wraps among a channel's kt-1 tap advances
    const int64_t xphw = 1 - (int64_t)(p.xS - 1) * p.xLq;
    const int64_t xwrap = (int64_t)p.Lp - (p.xS > 1 ? (int64_t)(kt - 1 - nwr) * p.xLq + nwr * xphw : (int64_t)(kt - 1) * p.xtap);
    int k_n = 0, ph_x = p.xph0;
    auto xoff_next = [&]() {
        const int64_t o = xoff;
        if (++k_n == kt) { k_n = 0; ph_x = p.xph0; xoff += xwrap; }
        else if (p.xS > 1) { if (++ph_x == p.xS) { ph_x = 0; xoff += xphw; } else xoff += p.xLq; }
        else xoff += p.xtap;
        return o;
    };
    const float* wrow = p.w + ((int64_t)ci_lo * p.K + min(ph, p.K - 1)) * p.CoutP;      // uniform
    const float* const wlast = p.w + ((int64_t)p.Cin * p.K - 1) * p.CoutP;
    const int64_t wtap = (int64_t)wstep * p.CoutP, wwrap = ((int64_t)p.K - (int64_t)(kt - 1) * wstep) * p.CoutP;
    int k_w = 0;
    auto wload = [&]() {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + cw);
        if (++k_w >= kt) { k_w = 0; wrow += wwrap; } else wrow += wtap;
        if (wrow > wlast) wrow = wlast;              // prefetch past the last step: clamped, unused
        return v;
    };
    f32x4 wq[D];
#pragma unroll
    for (int d = 0; d < D; ++d) wq[d] = wload();
    f32x2 xa[P / 2], xn[P / 2];
    auto xload = [&](f32x2 (&xv)[P / 2], int64_t off) {
#pragma unroll
        for (int j = 0; j < P / 2; ++j) xv[j] = f32x2{xb[off + 2 * j], xb[off + 2 * j + 1]};
    };
    auto fma = [&](const f32x4& wv, const f32x2 (&xv)[P / 2]) {
        const f32x2 w01 = f32x2{wv[0], wv[1]}, w23 = f32x2{wv[2], wv[3]};
#pragma unroll
        for (int j = 0; j < P / 2; ++j) {
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc[0][j]) : "v"(w01), "s"(xv[j]));
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc[1][j]) : "v"(w01), "s"(xv[j]));
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc[2][j]) : "v"(w23), "s"(xv[j]));
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc[3][j]) : "v"(w23), "s"(xv[j]));
        }
    };
    if (T > 0) xload(xa, xoff_next());
    // steps in groups of D so the prefetch slots are static registers; x double-buffered by name (two steps per pair)
    auto step = [&](int t, int slot, f32x2 (&xc)[P / 2], f32x2 (&xnext)[P / 2]) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xC07F);                     // lgkmcnt(0): x of this step is here
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < T) xload(xnext, xoff_next());
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");        // weights of this step (3 younger loads may fly)
        const f32x4 wv = wq[slot];
        wq[slot] = wload();
        fma(wv, xc);
    };
    int t = 0;
#pragma unroll 1
    for (; t + 4 <= T; t += 4) {
        step(t, 0, xa, xn);
        step(t + 1, 1, xn, xa);
        step(t + 2, 2, xa, xn);
        step(t + 3, 3, xn, xa);
    }
    if (t < T) { step(t, 0, xa, xn); ++t; }
    if (t < T) { step(t, 1, xn, xa); ++t; }
    if (t < T) { step(t, 2, xa, xn); ++t; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (S > 1) {                                    // fold the input-channel slices: slice 0 of each tile collects
        const int tile = wave / S;
        if (sp > 0) {
            float* rp = red + ((tile * (S - 1) + sp - 1) * 64) * 64 + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < P; ++j) rp[(c * P + j) * 64] = acc[c][j >> 1][j & 1];
        }
        __syncthreads();
        if (sp > 0) return;
        for (int q = 0; q < S - 1; ++q) {
            const float* rp = red + ((tile * (S - 1) + q) * 64) * 64 + lane;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < P; ++j) acc[c][j >> 1][j & 1] += rp[(c * P + j) * 64];
        }
    }
    if (!live) return;
    if (p.ks > 1) {                                 // raw partial sums; the epilogue runs in cfirst_finish_kernel
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int cc = co + c;
            if (cc >= p.Cout) continue;
            float* pp = p.part + (((int64_t)ksl * p.B + b) * p.Cout + cc) * p.Lout;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int64_t l = (int64_t)(l0 + j) * p.ostride + oo;
                if (l >= 0 && l < (LENS ? lout_b : p.Lout)) pp[l] = acc[c][j >> 1][j & 1];
            }
        }
        return;
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cc = co + c;
        if (cc >= p.Cout) continue;
        const float bv = p.bias ? p.bias[cc] : 0.f;
        float pa = p.pparam, pinv_b = 0.f;
        if (p.pact == 1) {
            pa = p.paa[cc];
            float bb = p.pab[cc];
            if (p.plogscale) { pa = __expf(pa); bb = __expf(bb); }
            pinv_b = 1.f / (bb + 1e-9f);
        }
        float* yp = p.y + ((int64_t)b * p.Cout + cc) * p.Lout;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int64_t l = (int64_t)(l0 + j) * p.ostride + oo;
            if (l < 0 || l >= (LENS ? lout_b : p.Lout)) continue;
            float v = (acc[c][j >> 1][j & 1] + bv) * p.out_scale;   // (residual already inside acc)
            if (p.post & 2) v += yp[l];
            if (p.y_raw) p.y_raw[((int64_t)b * p.Cout + cc) * p.Lout + l] = v;
            if (p.pact) v = act_apply(v, p.pact, pa, pinv_b);
            if (p.post & 1) v = tanhf(v);
            yp[l] = v;
        }
    }
}

// sums the input-channel slices of a split conv1d_cfirst launch and applies the conv epilogue (same order as above)
template <bool LENS = false>
__global__ __launch_bounds__(256) void cfirst_finish_kernel(ConvCArgs<LENS> p) {
    const int64_t n = (int64_t)p.B * p.Cout * p.Lout;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int cc = (int)((i / p.Lout) % p.Cout);
        if constexpr (LENS) {
            if ((int)(i % p.Lout) >= p.lens_out[i / ((int64_t)p.Cout * p.Lout)]) continue;   // (its partial sums were not written)
        }
        float v = p.res ? p.res[i] : 0.f;
        for (int s = 0; s < p.ks; ++s) v += p.part[(int64_t)s * n + i];
        v = (v + (p.bias ? p.bias[cc] : 0.f)) * p.out_scale;
        if (p.post & 2) v += p.y[i];
        if (p.y_raw) p.y_raw[i] = v;
        if (p.pact) {
            float pa = p.pparam, pinv_b = 0.f;
            if (p.pact == 1) {
                pa = p.paa[cc];
                float bb = p.pab[cc];
                if (p.plogscale) { pa = __expf(pa); bb = __expf(bb); }
                pinv_b = 1.f / (bb + 1e-9f);
            }
            v = act_apply(v, p.pact, pa, pinv_b);
        }
        if (p.post & 1) v = tanhf(v);
        p.y[i] = v;
    }
}

// weight norm fold + repack to [Cin][K][CoutP] (CoutP = Cout rounded up to 8, pad columns zeroed). One workgroup per index of dim 0 of v (the weight_norm dim).
//   conv:  v [Cout][Cin][K], g [Cout]  -> w[ci][k][co] = g[co] v[co][ci][k] / ||v[co]||
//   convT: v [Cin][Cout][K], g [Cin]   -> w[ci][k][co] = g[ci] v[ci][co][k] / ||v[ci]||
__global__ __launch_bounds__(256) void wn_fold_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                      float* __restrict__ w, int d0, int d1, int K, int flags) {
    __shared__ float red[16];
    const int transposed = flags & 1, flip = flags & 2;     // flip: tap k stored at K-1-k (the data gradient of a stride-1 conv)
    const int o = blockIdx.x;
    const int per = d1 * K;
    const int cout = transposed ? d1 : d0, coutp = (cout + 7) & ~7;
    if (!transposed && o >= d0) {       // pad output channel: zero column
        for (int i = threadIdx.x; i < per; i += 256) w[(int64_t)i * coutp + o] = 0.f;   // i = j*K + k
        return;
    }
    const float* vp = v + (int64_t)o * per;
    float scale = 1.f;
    if (g) {
        float s = 0.f;
        for (int i = threadIdx.x; i < per; i += 256) s += vp[i] * vp[i];
        s = block_sum(s, red);
        scale = g[o] / sqrtf(s);
    }
    for (int i = threadIdx.x; i < per; i += 256) {
        const int j = i / K, k0 = i - j * K, k = flip ? K - 1 - k0 : k0;
        if (!transposed) {  // o = co, j = ci ; Cout = d0
            w[((int64_t)j * K + k) * coutp + o] = vp[i] * scale;
        } else {            // o = ci, j = co ; Cout = d1
            w[((int64_t)o * K + k) * coutp + j] = vp[i] * scale;
        }
    }
    if (transposed)
        for (int i = threadIdx.x; i < (coutp - d1) * K; i += 256) {
            const int k = i / (coutp - d1), j = d1 + i - k * (coutp - d1);
            w[((int64_t)o * K + k) * coutp + j] = 0.f;
        }
}

template <bool F32>
__global__ __launch_bounds__(256) void snake_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                    const float* __restrict__ alpha, const float* __restrict__ beta,
                                                    int logscale, int C, int L, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)((i / L) % C);
        float a = alpha[c], b = beta[c];
        if (logscale) { a = __expf(a); b = __expf(b); }
        const float xv = ld1<F32>(x, i);
        const float sn = sinf(xv * a);            // accurate sine: this kernel is HBM-bound anyway
        st1<F32>(y, i, xv + sn * sn / (b + 1e-9f));
    }
}

// anti-aliased activation (alias-free-torch Activation1d, used by backup/flows.py:266-279,300-313,452-456):
//   2x kaiser-sinc FIR upsample (12 taps, replicate padding) -> snake / snake-beta -> 2x FIR low-pass downsample.
// One workgroup = 256 consecutive outputs of one (batch, channel) row; x segment and the activated 2x-rate
// signal live in LDS, so HBM sees one read and one write per element.
constexpr int A1_T = 1024;   // outputs per workgroup: 4 consecutive ones per thread
template <bool F32>
__global__ __launch_bounds__(256) void act1d_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                    const float* __restrict__ filt, const float* __restrict__ alpha,
                                                    const float* __restrict__ beta, int logscale, int C, int L) {
    // xs[j] = x_pad[i0 + j] (replicate padding folded in);  as[j] = act(u[clamp(2 t0 - 5 + j)])
    __shared__ __attribute__((aligned(16))) float xs[A1_T + 16];
    __shared__ __attribute__((aligned(16))) float as[2 * A1_T + 16];
    const int row = blockIdx.x;                     // b * C + c (rows on grid x: B * C may exceed grid y's 65535)
    const int c = row % C;
    const int t0 = blockIdx.y * A1_T;
    const int64_t base = (int64_t)row * L;
    float f[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) f[j] = filt[j];    // uniform: scalar loads
    // u index n = 2 t0 - 5 + j uses x_pad[(n + 5) >> 1 .. + 5]; j = 0 -> x_pad index t0: take i0 = t0 - 1 as slot 0
    const int i0 = t0 - 1;
    for (int j = threadIdx.x; j < A1_T + 16; j += 256) {
        const int xi = min(max(i0 + j - 5, 0), L - 1);   // x_pad[i] = x[clamp(i - 5)]
        xs[j] = ld1<F32>(x, base + xi);
    }
    __syncthreads();
    // alpha == NULL: ELU in place of the snake (Oobleck units with antialias_activation and use_snake=False, autoencoders.py:24-37)
    const bool elu = alpha == nullptr;
    float a = elu ? 0.f : alpha[c], b = elu ? 1.f : beta[c];
    if (logscale && !elu) { a = __expf(a); b = __expf(b); }
    const float inv_b = 1.f / (b + 1e-9f);
    // each thread produces 8 consecutive as[] slots (+ the 12-slot tail by the first threads) from a register window of x
    for (int j0 = 8 * threadIdx.x; j0 < 2 * A1_T + 12; j0 += 8 * 256) {
        // slots j0..j0+7 <-> n = 2 t0 - 5 + j0 + e; x_pad index of tap q: ((n + 5) >> 1) + q = t0 + ((j0 + e) >> 1) + q
        float xw[12];
        const int w0 = (j0 >> 1) + 1;               // slot of x_pad[t0 + (j0 >> 1)] in xs (i0 = t0 - 1)
#pragma unroll
        for (int q = 0; q < 10; ++q) xw[q] = xs[min(w0 + q, A1_T + 15)];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + e;
            if (j >= 2 * A1_T + 12) break;
            const int n = 2 * t0 - 5 + j;
            // tap of x_pad[t0 + (j >> 1) + q] is n + 15 - 2 i = 10 + (j & 1) - 2 q: even slots use taps 10, 8, .., 0 and odd
            // slots 11, 9, .., 1 (e and j have the same parity: j0 is a multiple of 8)
            float u = 0.f;
#pragma unroll
            for (int q = 0; q < 6; ++q) u += xw[(e >> 1) + q] * f[10 + (e & 1) - 2 * q];
            u *= 2.f;
            // replicate padding of the up-sampled signal: slots whose n falls outside [0, 2L) copy the edge value
            const int nc = min(max(n, 0), 2 * L - 1);
            if (nc != n) {
                const int ilo = (nc + 5) >> 1;      // recompute for the clamped index (rare: only at the two ends)
                float uu = 0.f;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const int i = ilo + q, tap = nc + 15 - 2 * i;
                    const int sl = min(max(i - i0, 0), A1_T + 15);
                    uu += xs[sl] * f[tap];
                }
                u = 2.f * uu;
            }
            const float sn = fast_sin(u * a);
            as[j] = elu ? (u > 0.f ? u : __expf(u) - 1.f) : u + inv_b * sn * sn;
        }
    }
    __syncthreads();
    // 4 consecutive outputs per thread: y[t] = sum_j f[j] as[2 (t - t0) + j]  -> 18 consecutive slots, 16-B aligned
    const int tl = 4 * threadIdx.x;
    float w[20];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(&as[2 * tl + 4 * q]);
        w[4 * q] = v[0]; w[4 * q + 1] = v[1]; w[4 * q + 2] = v[2]; w[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int t = t0 + tl + e;
        if (t >= L) break;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j) acc += f[j] * w[2 * e + j];
        st1<F32>(y, base + t, acc);
    }
}

}  // namespace

extern "C" int kalle_act1d_fwd(const void* x, void* y, int dtype, const float* filter12, const float* alpha,
                               const float* beta, int logscale, int B, int C, int L, void* stream) {
    if (!x || !y || !filter12 || ((alpha == nullptr) != (beta == nullptr)) || B <= 0 || C <= 0 || L <= 0 ||
        (int64_t)B * C > 0x7fffffff || (L + A1_T - 1) / A1_T > 65535)
        return KALLE_ERR_ARG;
    dim3 grid(B * C, (L + A1_T - 1) / A1_T), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32) KALLE_LAUNCH((act1d_kernel<true>), grid, block, 0, st, x, y, filter12, alpha, beta, logscale, C, L);
    else KALLE_LAUNCH((act1d_kernel<false>), grid, block, 0, st, x, y, filter12, alpha, beta, logscale, C, L);
    return kalle_check_launch();
}

extern "C" int kalle_weight_norm_fold(const float* v, const float* g, float* w_packed, int d0, int d1, int ksize,
                                      int transposed, void* stream) {
    if (!v || !w_packed || d0 <= 0 || d1 <= 0 || ksize <= 0) return KALLE_ERR_ARG;
    KALLE_LAUNCH(wn_fold_kernel, dim3((transposed & 1) ? d0 : ((d0 + 7) & ~7)), dim3(256), 0, static_cast<hipStream_t>(stream), v, g, w_packed, d0, d1,
                       ksize, transposed);
    return kalle_check_launch();
}


namespace {
struct ActArgs { int code = 0; const float* alpha = nullptr; const float* beta = nullptr; int logscale = 0; float param = 0.f; };
bool read_act(const kalle_act* a, ActArgs& o, bool input_side) {
    if (!a) return true;
    o.code = a->code; o.alpha = a->alpha; o.beta = a->beta; o.logscale = a->logscale; o.param = a->param;
    if (o.code < 0 || o.code > (input_side ? 4 : 3)) return false;
    if (o.code == 1 && (!o.alpha || !o.beta)) return false;
    return true;
}
bool fill_params(ConvParams& p, const kalle_act* in_act, const kalle_conv_epilogue* epi) {
    ActArgs ia, pa;
    if (!read_act(in_act, ia, true)) return false;
    p.act = ia.code; p.aa = ia.alpha; p.ab = ia.beta; p.logscale = ia.logscale; p.act_param = ia.param;
    p.res = nullptr; p.out_scale = 1.f; p.post = 0; p.y_raw = nullptr;
    if (epi) {
        if (!read_act(&epi->post_act, pa, false)) return false;
        p.res = epi->residual;
        p.y_raw = epi->y_raw;
        p.out_scale = epi->out_scale;
        p.post = (epi->tanh ? 1 : 0) | (epi->accumulate ? 2 : 0);
    }
    p.pact = pa.code; p.paa = pa.alpha; p.pab = pa.beta; p.plogscale = pa.logscale; p.pparam = pa.param;
    return true;
}
// v2 tile choice: (channels per wave, positions per lane).  A workgroup's cost is its padded output count times a
// penalty for the shorter (less well pipelined) tiles; workgroups beyond one per CU run in further rounds.
struct TileChoice { int cow, lpt; };
TileChoice pick_tile(int64_t npos, int Cout, int B, int halo, int span, int lpt_only, int64_t wg_mult) {
    const int cows[4] = {16, 8, 8, 8}, lpts[4] = {8, 8, 4, 2};
    const double pen[4] = {1.0, 1.08, 1.2, 1.5};
    TileChoice best{0, 0};
    double best_cost = 0;
    for (int i = 0; i < 4; ++i) {
        const int lt = 64 * lpts[i], cot = 4 * cows[i];
        if (lt + halo > span || (lpt_only && lpts[i] != lpt_only)) continue;
        if (cows[i] == 16 && (Cout < 64 || ((Cout + 7) & ~7) % 16)) continue;   // (16-wide weight reads need CoutP % 16 == 0)
        const int64_t nwg = ((npos + lt - 1) / lt) * ((Cout + cot - 1) / cot) * B * wg_mult;
        // rounds: 2 (COW 16) / 3 (COW 8) workgroups fit a CU; a lone workgroup per CU still costs ~0.6 of a full round
        const int64_t slots = 256 * (cows[i] == 16 ? 2 : 3);
        const double rounds = nwg <= 256 ? 0.6 : (double)((nwg + slots - 1) / slots);
        const double cost = (double)lt * cot * pen[i] * rounds * (cows[i] == 16 ? 2 : 3);
        if (!best.cow || cost < best_cost) { best = TileChoice{cows[i], lpts[i]}; best_cost = cost; }
    }
    return best;
}
constexpr int V2_SPAN = 640;
// kalle_conv_last_plan (encoding: include/kalle_hip.h)
thread_local int g_conv_plan = 0;
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr int plan_dtypes(bool xf, bool yf) { return (xf ? 1 << 4 : 0) | (yf ? 1 << 5 : 0); }
constexpr int plan_v2(int family, int cow, int lpt, int wco, int nw, int ci) {
    return family | cow << 8 | lpt << 13 | wco << 17 | nw << 21 | ilog2(ci / 8) << 25;
}

// What a planner decides about one call.  Filling it makes no HIP call and leaves g_conv_plan alone: the entry points launch
// from it, kalle_conv_plan / kalle_conv_transpose_plan report it.
struct TileForm { int cow, lpt, wco, ci, span, nw; };   // template arguments of the v2 kernels; cow 0: none
struct ConvPlan {
    int family = 0;            // 1-7, as in the plan word
    TileForm form{};           // families 2, 4
    int ntile = 0, nco = 0;    // families 2, 4: position tiles, channel tiles
    dim3 grid, block;
    int split = 0, ks = 0;     // families 5-7
    int Lp = 0, lead = 0, phases = 0, ws_floats = 0;   // families 5-7: the padded copy kalle_conv_pad_act makes, the workspace
    int word = 0;              // kalle_conv_last_plan after the launch
};
// a workgroup of form f covers 64 LPT NW / WCO positions and COW WCO channels
void set_form(ConvPlan& pl, ConvParams& p, const TileForm& f, int npos) {
    const int lt = 64 * f.lpt * (f.nw / f.wco), cot = f.cow * f.wco;
    pl.form = f;
    pl.ntile = p.ntile = (npos + lt - 1) / lt;
    pl.nco = p.nco = (p.Cout + cot - 1) / cot;
    pl.block = dim3(64 * f.nw);
}

// kalle_conv1d_fwd: argument checks, the kernel parameters (the entry point has set the four tensor pointers) and the plan
int plan_conv1d(bool tensors, int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                int padding, int dilation, const kalle_act* in_act, const kalle_conv_epilogue* epi, ConvParams& p, ConvPlan& pl) {
    if (!tensors || B <= 0 || Cin <= 0 || Cout <= 0 || Lin <= 0 || Lout <= 0) return KALLE_ERR_ARG;
    if (ksize <= 0 || ksize > MAX_K || stride <= 0 || dilation <= 0 || padding < 0) return KALLE_ERR_ARG;
    // `padding` is the LEFT pad; the right pad is implied by Lout (symmetric, 'same' or causal alike): taps beyond Lin read 0
    if ((int64_t)(Lout - 1) * stride - padding >= Lin) return KALLE_ERR_ARG;
    if (B > 65535 || (Cout + 7) / 8 > 65535) return KALLE_ERR_ARG;
    if (!fill_params(p, in_act, epi)) return KALLE_ERR_ARG;
    p.B = B; p.Cin = Cin; p.Lin = Lin; p.Cout = Cout; p.Lout = Lout; p.K = ksize; p.stride = stride; p.pad = padding;
    p.dil = dilation; p.CoutP = (Cout + 7) & ~7; p.xC = p.act == 4 ? 2 * Cin : Cin;
    const bool xf = x_dtype == KALLE_F32, yf = y_dtype == KALLE_F32;
    const int halo = (ksize - 1) * dilation;
    // weights small enough to stay in one XCD's L2: run the channel tiles of a position tile back to back (x re-read hits L2)
    p.co_fast = (int64_t)Cin * ksize * p.CoutP * 4 <= (2 << 20);
    const bool v2_stride = stride == 1 || (dilation == 1 && (stride == 2 || stride == 4 || stride == 8) && ksize <= 32);
    TileForm f{};
    if (v2_stride && p.act != 4 && xf == yf) {
        if (stride == 1) {
            const TileChoice tc = pick_tile(Lout, Cout, B, halo, V2_SPAN, 0, 1);
            if (Cout <= 4) {
                if (halo + 512 <= V2_SPAN) f = TileForm{2, 2, 1, 8, 640, 4};
            } else if (tc.cow == 16) {
                // 8 waves share one staged x tile for 128 output channels (pointwise convs: 32-channel chunks to cover
                // the HBM latency; measured +15 % at C >= 256, +8 % on the k = 7 convs at C = 256, neutral at C = 128)
                // pointwise convs: 256 positions x 128 channels per workgroup (64 accumulator registers per wave, 66 KiB of LDS) so
                // that TWO workgroups share a CU - one's residual loads / stores run under the other's FMAs; with 512 positions
                // (128 accumulator registers, 133 KiB) a CU runs one workgroup whose memory phases nothing overlaps
                if (ksize == 1 && Cout > 64) f = TileForm{16, 4, 8, 32, 256, 8};
                // (the same halving for the wide k = 7 convs - 7 x the FMAs per byte - is worth 0.4 % of a decode: not taken)
                else if (ksize != 1 && Cout >= 256 && halo + 512 <= 640) f = TileForm{16, 8, 8, 8, 640, 8};
                else if (ksize == 1) f = TileForm{16, 8, 4, 16, 512, 4};   // pointwise conv: longer chunks cover the HBM latency
                else f = TileForm{16, 8, 4, 8, 640, 4};
            } else if (tc.lpt) {                         // (0: not even the shortest tile fits its halo into the span)
                f = TileForm{8, tc.lpt, 4, 8, 640, 4};
            }
        } else if (Cout > 4) {                           // stride 2 / 4 / 8: de-interleaved staging, 1024/stride positions
            const bool wide = Cout >= 64 && p.CoutP % 16 == 0;
            if (stride == 2) f = TileForm{8, 8, 4, 8, 1088, 4};
            else if (stride == 4) f = wide ? TileForm{16, 4, 4, 8, 1088, 4} : TileForm{8, 4, 4, 8, 1088, 4};
            else if ((int64_t)Lout * B <= 1024) f = TileForm{8, 2, 4, 8, 1088, 4};   // stride 8; longer: fallback is faster
        }
    }
    if (f.cow) {
        set_form(pl, p, f, Lout);
        if ((int64_t)p.ntile * p.nco > 0x7fffffff) return KALLE_ERR_ARG;
        pl.grid = dim3(p.ntile * p.nco, 1, B);
        pl.family = 2;
        pl.word = plan_v2(2, f.cow, f.lpt, f.wco, f.nw, f.ci) | plan_dtypes(xf, yf) | ilog2(stride) << 28;
        return KALLE_OK;
    }
    if ((L_T - 1) * stride + halo + 1 > MAX_SPAN) return KALLE_ERR_UNSUPPORTED;
    pl.grid = dim3((Lout + L_T - 1) / L_T, (Cout + CO_T - 1) / CO_T, B);
    pl.block = dim3(256);
    pl.family = 1;
    pl.word = 1 | plan_dtypes(xf, yf);
    return KALLE_OK;
}

// kalle_conv_transpose1d_fwd
int plan_convT(bool tensors, int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
               int padding, const kalle_act* in_act, const kalle_conv_epilogue* epi, ConvParams& p, ConvPlan& pl) {
    if (!tensors || B <= 0 || Cin <= 0 || Cout <= 0 || Lin <= 0 || Lout <= 0) return KALLE_ERR_ARG;
    if (ksize <= 0 || stride <= 0 || padding < 0) return KALLE_ERR_ARG;
    // shorter than (Lin-1)*stride - 2*padding + K = causal trim of the tail; up to `padding` longer = the outputs the symmetric
    // trim would drop on the right (the data gradient of a strided conv whose input length is not a multiple of the stride)
    if (Lout > (Lin - 1) * stride - padding + ksize) return KALLE_ERR_ARG;
    if (B > 65535 || (Cout + 7) / 8 > 65535) return KALLE_ERR_ARG;
    if (!fill_params(p, in_act, epi)) return KALLE_ERR_ARG;
    if (p.act == 4) return KALLE_ERR_UNSUPPORTED;
    p.B = B; p.Cin = Cin; p.Lin = Lin; p.Cout = Cout; p.Lout = Lout; p.K = ksize; p.stride = stride; p.pad = padding;
    p.dil = 1; p.CoutP = (Cout + 7) & ~7; p.xC = Cin;
    const bool xf = x_dtype == KALLE_F32, yf = y_dtype == KALLE_F32;
    const int mmax = (ksize + stride - 1) / stride;
    TileForm f{};
    const int nq = (Lout - 1 + padding) / stride + 1;      // input positions that reach an output
    if (xf == yf && mmax <= 64) {
        const TileChoice tc = pick_tile(nq, Cout, B, mmax - 1, V2_SPAN, 0, stride);
        if (Cout <= 4) {
            if (mmax - 1 + 512 <= V2_SPAN) f = TileForm{2, 2, 1, 8, 640, 4};
        } else if (tc.cow == 16) {
            f = TileForm{16, 8, 4, 8, 640, 4};
        } else if (tc.lpt) {
            f = TileForm{8, tc.lpt, 4, 8, 640, 4};
        }
    }
    if (f.cow) {
        set_form(pl, p, f, nq);
        const int64_t nwg = (((int64_t)p.ntile * p.nco + 7) / 8) * 8 * stride;      // one pass per output phase
        if (nwg > 0x7fffffff) return KALLE_ERR_ARG;
        pl.grid = dim3((unsigned)nwg, 1, B);
        pl.family = 4;
        pl.word = plan_v2(4, f.cow, f.lpt, f.wco, 4, 8) | plan_dtypes(xf, yf);
        return KALLE_OK;
    }
    if (ksize > MAX_K + 2 || ksize > 2 * stride + 1 || p.res || p.post || p.pact || p.y_raw || p.out_scale != 1.f)
        return KALLE_ERR_UNSUPPORTED;
    pl.grid = dim3((Lout + L_T - 1) / L_T, (Cout + CO_T - 1) / CO_T, B);
    pl.block = dim3(256);
    pl.family = 3;
    pl.word = 3 | plan_dtypes(xf, yf);
    return KALLE_OK;
}

// ---- launchers: the plan's tile form -> the instantiation.  The tables are the whole set of v2 code objects.
constexpr int64_t form_key(int cow, int lpt, int wco, int ci, int span, int nw) {
    return (int64_t)span << 32 | plan_v2(0, cow, lpt, wco, nw, ci);
}
int64_t form_key(const TileForm& f) { return form_key(f.cow, f.lpt, f.wco, f.ci, f.span, f.nw); }

// (every kernel exists twice: the dense instantiation, whose code does not know of lengths, and the LENS one a ragged call gets)
template <int COW, int LPT, int WCO, int CI, int SPAN, int NW>
void launch_v2(const ConvPlan& pl, const ConvParamsL& p, bool f32, hipStream_t st) {
    const ConvParams& d = p;
    if (p.lens_out) {
        if (f32) KALLE_LAUNCH((conv1d_v2_kernel<COW, LPT, WCO, CI, SPAN, true, true, NW, true>), pl.grid, pl.block, 0, st, p);
        else KALLE_LAUNCH((conv1d_v2_kernel<COW, LPT, WCO, CI, SPAN, false, false, NW, true>), pl.grid, pl.block, 0, st, p);
    } else if (f32) KALLE_LAUNCH((conv1d_v2_kernel<COW, LPT, WCO, CI, SPAN, true, true, NW>), pl.grid, pl.block, 0, st, d);
    else KALLE_LAUNCH((conv1d_v2_kernel<COW, LPT, WCO, CI, SPAN, false, false, NW>), pl.grid, pl.block, 0, st, d);
}
template <int COW, int LPT, int WCO>
void launch_tv2(const ConvPlan& pl, const ConvParamsL& p, bool f32, hipStream_t st) {
    const ConvParams& d = p;
    if (p.lens_out) {
        if (f32) KALLE_LAUNCH((convT1d_v2_kernel<COW, LPT, WCO, 8, 640, true, true, true>), pl.grid, pl.block, 0, st, p);
        else KALLE_LAUNCH((convT1d_v2_kernel<COW, LPT, WCO, 8, 640, false, false, true>), pl.grid, pl.block, 0, st, p);
    } else if (f32) KALLE_LAUNCH((convT1d_v2_kernel<COW, LPT, WCO, 8, 640, true, true>), pl.grid, pl.block, 0, st, d);
    else KALLE_LAUNCH((convT1d_v2_kernel<COW, LPT, WCO, 8, 640, false, false>), pl.grid, pl.block, 0, st, d);
}
template <bool LENS>
void launch_v1(const ConvPlan& pl, const ConvArgs<LENS>& p, bool xf, bool yf, hipStream_t st) {
    if (xf && yf) KALLE_LAUNCH((conv1d_kernel<true, true, LENS>), pl.grid, pl.block, 0, st, p);
    else if (xf) KALLE_LAUNCH((conv1d_kernel<true, false, LENS>), pl.grid, pl.block, 0, st, p);
    else if (yf) KALLE_LAUNCH((conv1d_kernel<false, true, LENS>), pl.grid, pl.block, 0, st, p);
    else KALLE_LAUNCH((conv1d_kernel<false, false, LENS>), pl.grid, pl.block, 0, st, p);
}
template <bool LENS>
void launch_tv1(const ConvPlan& pl, const ConvArgs<LENS>& p, bool xf, bool yf, hipStream_t st) {
    if (xf && yf) KALLE_LAUNCH((convT1d_kernel<true, true, LENS>), pl.grid, pl.block, 0, st, p);
    else if (xf) KALLE_LAUNCH((convT1d_kernel<true, false, LENS>), pl.grid, pl.block, 0, st, p);
    else if (yf) KALLE_LAUNCH((convT1d_kernel<false, true, LENS>), pl.grid, pl.block, 0, st, p);
    else KALLE_LAUNCH((convT1d_kernel<false, false, LENS>), pl.grid, pl.block, 0, st, p);
}
// false: the plan names a form that was never compiled (a planner bug; nothing is launched)
bool launch_conv1d(const ConvPlan& pl, const ConvParamsL& p, bool xf, bool yf, hipStream_t st) {
    if (pl.family == 1) {
        if (p.lens_out) launch_v1<true>(pl, p, xf, yf, st);
        else launch_v1<false>(pl, p, xf, yf, st);
        return true;
    }
    switch (form_key(pl.form)) {
#define KALLE_FORM(...) case form_key(__VA_ARGS__): launch_v2<__VA_ARGS__>(pl, p, xf, st); break;
        KALLE_FORM(2, 2, 1, 8, 640, 4)
        KALLE_FORM(8, 2, 4, 8, 640, 4)
        KALLE_FORM(8, 4, 4, 8, 640, 4)
        KALLE_FORM(8, 8, 4, 8, 640, 4)
        KALLE_FORM(16, 8, 4, 8, 640, 4)
        KALLE_FORM(16, 8, 4, 16, 512, 4)
        KALLE_FORM(16, 4, 8, 32, 256, 8)
        KALLE_FORM(16, 8, 8, 8, 640, 8)
        KALLE_FORM(8, 8, 4, 8, 1088, 4)
        KALLE_FORM(8, 4, 4, 8, 1088, 4)
        KALLE_FORM(16, 4, 4, 8, 1088, 4)
        KALLE_FORM(8, 2, 4, 8, 1088, 4)
#undef KALLE_FORM
        default: return false;
    }
    return true;
}
bool launch_convT(const ConvPlan& pl, const ConvParamsL& p, bool xf, bool yf, hipStream_t st) {
    if (pl.family == 3) {
        if (p.lens_out) launch_tv1<true>(pl, p, xf, yf, st);
        else launch_tv1<false>(pl, p, xf, yf, st);
        return true;
    }
    switch (form_key(pl.form)) {
#define KALLE_FORM(COW, LPT, WCO) case form_key(COW, LPT, WCO, 8, 640, 4): launch_tv2<COW, LPT, WCO>(pl, p, xf, st); break;
        KALLE_FORM(2, 2, 1)
        KALLE_FORM(8, 2, 4)
        KALLE_FORM(8, 4, 4)
        KALLE_FORM(8, 8, 4)
        KALLE_FORM(16, 8, 4)
#undef KALLE_FORM
        default: return false;
    }
    return true;
}

// ---- channels-per-lane kernels (families 5-7)
// The padded copy x_padded [B][C][Lp] that kalle_conv_pad_act(..., padding = lead, phases) makes for them.  A conv reads
// 16-position tiles plus the halo.  Strided (dilation 1): the copy is de-interleaved into `stride` phase rows of Lp / stride
// slots behind a left pad of padq * stride: tap k of output l reads phase (k + d) % stride at slot l + (k + d) / stride.
struct PadGeom { int Lp, lead, phases, d; };
PadGeom conv_pad_geom(int Lout, int ksize, int stride, int padding, int dilation) {
    const int l16 = (Lout + 15) & ~15;
    if (stride == 1) return PadGeom{l16 + (ksize - 1) * dilation, padding, 1, 0};
    const int padq = (padding + stride - 1) / stride, d = padq * stride - padding;
    return PadGeom{stride * (l16 + (ksize - 1 + d) / stride + 1), padq * stride, stride, d};
}
// transposed: nq input positions reach an output, each tap m of input position q reads slot q + (mmax - 1) - m
PadGeom convT_pad_geom(int Lout, int ksize, int stride, int padding) {
    const int nq = (Lout - 1 + padding) / stride + 1, mmax = (ksize + stride - 1) / stride;
    return PadGeom{((nq + 15) & ~15) + mmax - 1, mmax - 1, 1, 0};
}
// waves of a workgroup that share one position tile and split its input channels: `waves` counts the tiles; aim for >= 2048
// waves (two per SIMD)
int cfirst_split(int64_t waves) { return waves >= 2048 ? 1 : (waves >= 1024 ? 2 : 4); }
// workgroup-level input-channel split of the channels-per-lane conv: with few positions AND few output channels even 4
// waves per tile leave most SIMDs idle while every wave walks Cin * K dependent prefetch steps (the 1024 -> 2048 stride-8
// and 2048 -> 128 convs at the bottom of a single-clip encode: 112 / 14 position-channel tiles)
int cfirst_ksplit(int B, int Cin, int Cout, int Lout, int ksize) {
    const int64_t waves = (int64_t)((Lout + 15) / 16) * ((Cout + 255) / 256) * B * 4;
    int ks = 1;
    while (ks < 16 && waves * ks < 4096 && (int64_t)Cin * ksize / (8 * ks) >= 64) ks *= 2;
    return ks;
}
// fp32 elements of the workspace that lets a launch use that split; 0: not split (or the slabs would pass 2^31 elements)
int cfirst_ws_floats(int B, int Cin, int Cout, int Lout, int ksize) {
    const int ks = cfirst_ksplit(B, Cin, Cout, Lout, ksize);
    const int64_t n = ks > 1 ? (int64_t)ks * B * Cout * Lout : 0;
    return n > 0x7fffffff ? 0 : (int)n;
}
// what the two forms share: tensors, sizes, the epilogue; false: a bad epilogue
bool cfirst_params(ConvCParams& p, const kalle_conv_epilogue* epi, int B, int Cin, int Lp, int Cout, int Lout, int ksize) {
    ConvParams q{};
    if (!fill_params(q, nullptr, epi)) return false;
    p.res = static_cast<const float*>(q.res); p.y_raw = static_cast<float*>(q.y_raw);
    p.B = B; p.Cin = Cin; p.Lp = Lp; p.Cout = Cout; p.CoutP = (Cout + 7) & ~7; p.Lout = Lout; p.K = ksize;
    p.post = q.post; p.out_scale = q.out_scale;
    p.pact = q.pact; p.paa = q.paa; p.pab = q.pab; p.plogscale = q.plogscale; p.pparam = q.pparam;
    return true;
}
void cfirst_word(ConvPlan& pl, int family, int split, int ks) {
    pl.family = family; pl.split = split; pl.ks = ks;
    pl.block = dim3(256);
    pl.word = family | plan_dtypes(true, true) | split << 8 | ks << 12;
}

// kalle_conv1d_cfirst_fwd (the entry point has set xp, w, bias, y and part); have_ws: the caller lends a workspace
int plan_cfirst(bool tensors, int B, int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding, int dilation,
                const kalle_conv_epilogue* epi, bool have_ws, ConvCParams& p, ConvPlan& pl) {
    if (!tensors || B <= 0 || Cin <= 0 || Cout <= 0 || Lout <= 0 || ksize <= 0 || dilation <= 0 || stride <= 0 || padding < 0)
        return KALLE_ERR_ARG;
    if (stride > 1 && dilation != 1) return KALLE_ERR_UNSUPPORTED;
    const PadGeom g = conv_pad_geom(Lout, ksize, stride, padding, dilation);
    if (Lp < g.Lp || (stride > 1 && Lp % stride) || B > 65535) return KALLE_ERR_ARG;
    if (!cfirst_params(p, epi, B, Cin, Lp, Cout, Lout, ksize)) return KALLE_ERR_ARG;
    const int split = cfirst_split((int64_t)((Lout + 15) / 16) * ((Cout + 255) / 256) * B);
    const int ks = have_ws ? cfirst_ksplit(B, Cin, Cout, Lout, ksize) : 1;   // (the caller sized it with ..._ws_floats)
    const int Lq = stride > 1 ? Lp / stride : 0;
    p.dil = dilation; p.split = split; p.ks = ks;
    p.nphase = 1; p.npos = Lout; p.xtap = dilation; p.ostride = 1; p.opad = 0; p.xlead = g.d * Lq;
    p.xS = stride; p.xLq = Lq; p.xph0 = g.d;
    if (p.CoutP < 4) return KALLE_ERR_UNSUPPORTED;
    const int tiles_per_wg = 4 / split;
    if ((int64_t)B * ks > 65535) return KALLE_ERR_ARG;
    pl.grid = dim3(((Lout + 15) / 16 + tiles_per_wg - 1) / tiles_per_wg, (Cout + 255) / 256, B * ks);
    cfirst_word(pl, stride > 1 ? 6 : 5, split, ks);
    pl.Lp = g.Lp; pl.lead = g.lead; pl.phases = g.phases;
    pl.ws_floats = have_ws ? cfirst_ws_floats(B, Cin, Cout, Lout, ksize) : 0;
    return KALLE_OK;
}

// kalle_conv_transpose1d_cfirst_fwd: one pass per output phase, no workspace
int plan_cfirst_T(bool tensors, int B, int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding,
                  const kalle_conv_epilogue* epi, ConvCParams& p, ConvPlan& pl) {
    if (!tensors || B <= 0 || Cin <= 0 || Cout <= 0 || Lout <= 0 || ksize <= 0 || stride <= 0 || padding < 0) return KALLE_ERR_ARG;
    const PadGeom g = convT_pad_geom(Lout, ksize, stride, padding);
    if (Lp < g.Lp || B > 65535) return KALLE_ERR_ARG;
    if (!cfirst_params(p, epi, B, Cin, Lp, Cout, Lout, ksize)) return KALLE_ERR_ARG;
    const int nq = (Lout - 1 + padding) / stride + 1;
    const int split = cfirst_split((int64_t)((nq + 15) / 16) * ((Cout + 255) / 256) * B * stride);
    p.dil = 1; p.split = split; p.ks = 1;
    p.nphase = stride; p.npos = nq; p.xtap = -1; p.ostride = stride; p.opad = padding; p.xlead = g.lead;
    p.xS = 1; p.xLq = 0; p.xph0 = 0;
    if (p.CoutP < 4) return KALLE_ERR_UNSUPPORTED;
    const int tiles_per_wg = 4 / split;
    const int64_t gx = (int64_t)(((nq + 15) / 16 + tiles_per_wg - 1) / tiles_per_wg) * stride;
    if (gx > 0x7fffffff) return KALLE_ERR_ARG;
    pl.grid = dim3((unsigned)gx, (Cout + 255) / 256, B);
    cfirst_word(pl, 7, split, 1);
    pl.Lp = g.Lp; pl.lead = g.lead; pl.phases = g.phases;
    return KALLE_OK;
}

void launch_cfirst(const ConvPlan& pl, const ConvCParamsL& p, hipStream_t st) {
    const ConvCParams& d = p;
    if (p.lens_out) KALLE_LAUNCH(conv1d_cfirst_kernel<true>, pl.grid, pl.block, 0, st, p);
    else KALLE_LAUNCH(conv1d_cfirst_kernel<false>, pl.grid, pl.block, 0, st, d);
    if (pl.ks > 1) {
        const int64_t n = (int64_t)p.B * p.Cout * p.Lout;
        const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 2048));
        if (p.lens_out) KALLE_LAUNCH(cfirst_finish_kernel<true>, grid, dim3(256), 0, st, p);
        else KALLE_LAUNCH(cfirst_finish_kernel<false>, grid, dim3(256), 0, st, d);
    }
}

// ---- ragged batches: the per-row lengths of the ..._lens entry points (contract: include/kalle_hip.h)
// Each array comes as a host copy (checked here, read by nobody else) and a device copy (read by the kernels).
enum { LENS_DENSE, LENS_LIVE, LENS_IDLE, LENS_BAD };
// h_in may be absent (an entry point that takes output lengths only) and so may h_out; Lin / Lout < 0: that bound is not known
// to the entry point.  max_out(len_in): the most outputs the layer makes of len_in inputs (0 of 0: an inactive row).
template <class F>
int read_lens(int n_given, int n_taken, const int32_t* h_in, const int32_t* h_out, int B, int Lin, int Lout, F max_out) {
    if (n_given == 0) return LENS_DENSE;
    if (n_given != n_taken) return LENS_BAD;        // a host copy without its device copy, lens_in without lens_out, ...
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const int64_t li = h_in ? h_in[b] : -1, lo = h_out ? h_out[b] : -1;
        if (h_in && (li < 0 || (Lin >= 0 && li > Lin))) return LENS_BAD;
        if (h_out && (lo < 0 || (Lout >= 0 && lo > Lout))) return LENS_BAD;
        if (h_in && h_out && lo > (li == 0 ? 0 : max_out(li))) return LENS_BAD;
        any = any || (h_out ? lo > 0 : li > 0);
    }
    return any ? LENS_LIVE : LENS_IDLE;
}
int count_given(std::initializer_list<const void*> ps) {
    int n = 0;
    for (const void* q : ps) n += q != nullptr;
    return n;
}

// ---- which family a call gets (kalle_conv_plan / kalle_conv_transpose_plan; kalle_audio_amd/conv_ops.py asks them)
// Few positions, many channels (the top of the VAE, all of a single-clip decode): the channels-per-lane kernel over a padded,
// pre-activated copy of x, where the position-per-lane tiling would leave most CUs without a workgroup.
bool conv_prefers_cfirst(int B, int Cin, int Cout, int Lout, int ksize, int stride) {
    // strided convs (the encoder's down-samplers): the position-per-lane kernels reach 16-25 TFLOP/s at stride 8 and 38-46 at
    // stride 4, the channels-per-lane kernel 43-57 at every batch size measured (512 -> 1024, k = 16, stride 8, 13760 inputs,
    // B = 4: 5388 against 2379 us; 1024 -> 2048 x 1720, B = 8: 7237 against 2166; 256 -> 512, k = 8, stride 4, B = 8: 5021 against 3876)
    if (stride > 1) return Cout >= 256;
    // The position-per-lane kernel runs these layers in 8-wave workgroups of 128 channels x 512 positions (256 for k = 1): one
    // round of them takes the same time whether 100 or 256 exist, while the channels-per-lane kernel scales with the work
    // (tools/cfirst_vs_v2.sh, 1024 channels x 1720 positions, k = 7: B = 4 -> 128 workgroups 2316 us against 1820; B = 5 -> 160
    // workgroups 2262 against 2560; 512 channels x 13760, k = 1, B = 1 -> 216 workgroups 162 us against 222)
    const int lt = ksize == 1 ? 256 : 512;
    if (Cout >= 256) return (int64_t)((Lout + lt - 1) / lt) * ((Cout + 127) / 128) * B < 160;
    // few output channels: while positions are few too - or the reduction is long and the position-per-lane grid a handful of
    // workgroups that each walk all of it (2048 -> 128, k = 3, 215 positions, B = 16: 1089 against 222 us)
    const int64_t nwg64 = (int64_t)((Lout + 511) / 512) * ((Cout + 63) / 64) * B;
    return Cout >= 64 && nwg64 < 256 && ((int64_t)Lout * B <= 1024 || (Cin >= 1024 && nwg64 <= 64));
}
// (tools/cfirst_vs_v2.sh: at 512+ output channels the channels-per-lane kernel holds 50-70 TFLOP/s where the phase-per-workgroup
// kernel needs far more positions to get there - 2048 -> 1024 x 215, B = 8: 2082 against 3463 us; 1024 -> 512 x 1720, B = 8: 3290
// against 3878; at 256 channels the two cross near 1500: 512 -> 256 x 13760, B = 3: 1465 against 1551, B = 4: 1870 against 1806)
bool convT_prefers_cfirst(int B, int Cout, int Lout, int stride, int padding) {
    const int nq = (Lout - 1 + padding) / stride + 1;
    return (int64_t)((nq + 511) / 512) * ((Cout + 63) / 64) * B * stride < (Cout >= 512 ? 4096 : 1536) && Cout >= 256;
}
enum { PREFER_AUTO = 0, PREFER_CFIRST = 1, PREFER_POSITIONS = 2 };
void report(const ConvPlan& pl, int32_t* out) {
    out[0] = pl.family; out[1] = pl.word; out[2] = pl.Lp; out[3] = pl.lead; out[4] = pl.phases; out[5] = pl.ws_floats;
}
}  // namespace

extern "C" int kalle_conv_last_plan(void) { return g_conv_plan; }
// library-internal (conv1d_bwd.hip records its launches through it): not part of the ABI, not exported
extern "C" __attribute__((visibility("hidden"))) void kalle_set_conv_plan(int plan) { g_conv_plan = plan; }

extern "C" int kalle_conv1d_fwd_lens(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                                     int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                                     int padding, int dilation, const kalle_act* in_act, const kalle_conv_epilogue* epi,
                                     const int32_t* lens_in_host, const int32_t* lens_in_dev, const int32_t* lens_out_host,
                                     const int32_t* lens_out_dev, void* stream) {
    g_conv_plan = 0;
    ConvParamsL p{};
    ConvPlan pl;
    p.x = x; p.w = w_packed; p.bias = bias; p.y = y;
    const int rc = plan_conv1d(x && w_packed && y, x_dtype, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding, dilation,
                               in_act, epi, p, pl);
    if (rc != KALLE_OK) return rc;
    const int lens = read_lens(count_given({lens_in_host, lens_in_dev, lens_out_host, lens_out_dev}), 4, lens_in_host, lens_out_host,
                               B, Lin, Lout, [&](int64_t li) { return (li - 1 + padding) / stride + 1; });
    if (lens == LENS_BAD) return KALLE_ERR_ARG;
    p.lens_in = lens_in_dev; p.lens_out = lens_out_dev;
    if (lens == LENS_IDLE) {                        // every row inactive: nothing to launch; the plan is the dense call's
        g_conv_plan = pl.word;
        return KALLE_OK;
    }
    if (!launch_conv1d(pl, p, x_dtype == KALLE_F32, y_dtype == KALLE_F32, static_cast<hipStream_t>(stream)))
        return KALLE_ERR_UNSUPPORTED;
    g_conv_plan = pl.word;
    return kalle_check_launch();
}
extern "C" int kalle_conv1d_fwd(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                                int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                                int padding, int dilation, const kalle_act* in_act, const kalle_conv_epilogue* epi,
                                void* stream) {
    return kalle_conv1d_fwd_lens(x, x_dtype, w_packed, bias, y, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding, dilation,
                                 in_act, epi, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int kalle_conv_transpose1d_fwd_lens(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                                               int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize,
                                               int stride, int padding, const kalle_act* in_act,
                                               const kalle_conv_epilogue* epi, const int32_t* lens_in_host,
                                               const int32_t* lens_in_dev, const int32_t* lens_out_host,
                                               const int32_t* lens_out_dev, void* stream) {
    g_conv_plan = 0;
    ConvParamsL p{};
    ConvPlan pl;
    p.x = x; p.w = w_packed; p.bias = bias; p.y = y;
    const int rc = plan_convT(x && w_packed && y, x_dtype, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding, in_act, epi,
                              p, pl);
    if (rc != KALLE_OK) return rc;
    const int lens = read_lens(count_given({lens_in_host, lens_in_dev, lens_out_host, lens_out_dev}), 4, lens_in_host, lens_out_host,
                               B, Lin, Lout, [&](int64_t li) { return (li - 1) * stride - padding + ksize; });
    if (lens == LENS_BAD) return KALLE_ERR_ARG;
    p.lens_in = lens_in_dev; p.lens_out = lens_out_dev;
    if (lens == LENS_IDLE) {
        g_conv_plan = pl.word;
        return KALLE_OK;
    }
    if (!launch_convT(pl, p, x_dtype == KALLE_F32, y_dtype == KALLE_F32, static_cast<hipStream_t>(stream)))
        return KALLE_ERR_UNSUPPORTED;
    g_conv_plan = pl.word;
    return kalle_check_launch();
}
extern "C" int kalle_conv_transpose1d_fwd(const void* x, int x_dtype, const float* w_packed, const float* bias, void* y,
                                          int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize,
                                          int stride, int padding, const kalle_act* in_act,
                                          const kalle_conv_epilogue* epi, void* stream) {
    return kalle_conv_transpose1d_fwd_lens(x, x_dtype, w_packed, bias, y, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding,
                                           in_act, epi, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int kalle_conv_pad_len(int Lout, int ksize, int stride, int padding, int dilation) {
    return conv_pad_geom(Lout, ksize, stride, padding, dilation).Lp;
}
extern "C" int kalle_convT_pad_len(int Lout, int ksize, int stride, int padding) {
    return convT_pad_geom(Lout, ksize, stride, padding).Lp;
}

extern "C" int kalle_conv_pad_act_lens(const float* x, float* x_padded, int B, int C, int Lin, int Lp, int padding,
                                       const kalle_act* act, int phases, const int32_t* lens_in_host, const int32_t* lens_in_dev,
                                       void* stream) {
    if (!x || !x_padded || B <= 0 || C <= 0 || Lin <= 0 || Lp <= 0 || padding < 0 || phases <= 0 || Lp % phases)
        return KALLE_ERR_ARG;
    const int gx = (Lp + 255) / 256 > 64 ? 64 : (Lp + 255) / 256;
    if ((int64_t)B * C * gx > 0x7fffffff) return KALLE_ERR_ARG;
    ActArgs a;
    if (!read_act(act, a, false)) return KALLE_ERR_ARG;
    const int lens = read_lens(count_given({lens_in_host, lens_in_dev}), 2, lens_in_host, nullptr, B, Lin, -1, [](int64_t) { return 0; });
    if (lens == LENS_BAD) return KALLE_ERR_ARG;
    if (lens == LENS_IDLE) return KALLE_OK;
    const dim3 grid((unsigned)(B * C * gx));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (lens == LENS_LIVE)
        KALLE_LAUNCH(pad_act_lens_kernel, grid, dim3(256), 0, st, x, x_padded, C, Lin, Lp, padding, a.code, a.alpha, a.beta, a.logscale,
                     a.param, phases, gx, lens_in_dev);
    else
        KALLE_LAUNCH(pad_act_kernel, grid, dim3(256), 0, st, x, x_padded, C, Lin, Lp, padding, a.code, a.alpha, a.beta, a.logscale,
                     a.param, phases, gx);
    return kalle_check_launch();
}
extern "C" int kalle_conv_pad_act(const float* x, float* x_padded, int B, int C, int Lin, int Lp, int padding,
                                  const kalle_act* act, int phases, void* stream) {
    return kalle_conv_pad_act_lens(x, x_padded, B, C, Lin, Lp, padding, act, phases, nullptr, nullptr, stream);
}

extern "C" int kalle_conv_cfirst_ws_floats(int B, int Cin, int Cout, int Lout, int ksize) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Lout <= 0 || ksize <= 0) return KALLE_ERR_ARG;
    return cfirst_ws_floats(B, Cin, Cout, Lout, ksize);
}

extern "C" int kalle_conv1d_cfirst_fwd_lens(const float* x_padded, const float* w_packed, const float* bias, float* y, int B,
                                            int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding,
                                            int dilation, const kalle_conv_epilogue* epi, float* workspace,
                                            const int32_t* lens_in_host, const int32_t* lens_in_dev, const int32_t* lens_out_host,
                                            const int32_t* lens_out_dev, void* stream) {
    g_conv_plan = 0;
    ConvCParamsL p{};
    ConvPlan pl;
    p.xp = x_padded; p.w = w_packed; p.bias = bias; p.y = y; p.part = workspace;
    const int rc = plan_cfirst(x_padded && w_packed && y, B, Cin, Lp, Cout, Lout, ksize, stride, padding, dilation, epi,
                               workspace != nullptr, p, pl);
    if (rc != KALLE_OK) return rc;
    // (the padded copy hides Lin: kalle_conv_pad_act_lens holds the input lengths to it)
    const int lens = read_lens(count_given({lens_in_host, lens_in_dev, lens_out_host, lens_out_dev}), 4, lens_in_host, lens_out_host,
                               B, -1, Lout, [&](int64_t li) { return (li - 1 + padding) / stride + 1; });
    if (lens == LENS_BAD) return KALLE_ERR_ARG;
    p.lens_out = lens_out_dev;                      // (the input lengths acted in kalle_conv_pad_act_lens)
    if (lens != LENS_IDLE) launch_cfirst(pl, p, static_cast<hipStream_t>(stream));
    g_conv_plan = pl.word;
    return lens == LENS_IDLE ? KALLE_OK : kalle_check_launch();
}
extern "C" int kalle_conv1d_cfirst_fwd(const float* x_padded, const float* w_packed, const float* bias, float* y, int B,
                                       int Cin, int Lp, int Cout, int Lout, int ksize, int stride, int padding,
                                       int dilation, const kalle_conv_epilogue* epi, float* workspace, void* stream) {
    return kalle_conv1d_cfirst_fwd_lens(x_padded, w_packed, bias, y, B, Cin, Lp, Cout, Lout, ksize, stride, padding, dilation, epi,
                                        workspace, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int kalle_conv_transpose1d_cfirst_fwd_lens(const float* x_padded, const float* w_packed, const float* bias, float* y,
                                                      int B, int Cin, int Lp, int Cout, int Lout, int ksize, int stride,
                                                      int padding, const kalle_conv_epilogue* epi, const int32_t* lens_out_host,
                                                      const int32_t* lens_out_dev, void* stream) {
    g_conv_plan = 0;
    ConvCParamsL p{};
    ConvPlan pl;
    p.xp = x_padded; p.w = w_packed; p.bias = bias; p.y = y;
    const int rc = plan_cfirst_T(x_padded && w_packed && y, B, Cin, Lp, Cout, Lout, ksize, stride, padding, epi, p, pl);
    if (rc != KALLE_OK) return rc;
    const int lens = read_lens(count_given({lens_out_host, lens_out_dev}), 2, nullptr, lens_out_host, B, -1, Lout, [](int64_t) { return 0; });
    if (lens == LENS_BAD) return KALLE_ERR_ARG;
    p.lens_out = lens_out_dev;
    if (lens != LENS_IDLE) launch_cfirst(pl, p, static_cast<hipStream_t>(stream));
    g_conv_plan = pl.word;
    return lens == LENS_IDLE ? KALLE_OK : kalle_check_launch();
}
extern "C" int kalle_conv_transpose1d_cfirst_fwd(const float* x_padded, const float* w_packed, const float* bias, float* y,
                                                 int B, int Cin, int Lp, int Cout, int Lout, int ksize, int stride,
                                                 int padding, const kalle_conv_epilogue* epi, void* stream) {
    return kalle_conv_transpose1d_cfirst_fwd_lens(x_padded, w_packed, bias, y, B, Cin, Lp, Cout, Lout, ksize, stride, padding, epi,
                                                  nullptr, nullptr, stream);
}

// The two queries: the dispatch of conv_ops.conv1d / conv_transpose1d for any caller, without a device.  The channels-per-lane
// family is taken where the call is eligible (fp32 in and out, no gate, not strided and dilated at once; transposed: not
// extended past the symmetric trim) and `prefer` forces it or, left at auto, the cost rule above asks for it; the planner of
// the family's entry point then checks the arguments and answers.
extern "C" int kalle_conv_plan(int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize, int stride,
                               int padding, int dilation, const kalle_act* in_act, const kalle_conv_epilogue* epi, int prefer,
                               int32_t* out) {
    if (!out || prefer < PREFER_AUTO || prefer > PREFER_POSITIONS) return KALLE_ERR_ARG;
    ConvPlan pl;
    int rc;
    const bool sane = B > 0 && Cin > 0 && Lin > 0 && Cout > 0 && Lout > 0 && ksize > 0 && stride > 0 && dilation > 0 && padding >= 0;
    const bool eligible = sane && (stride == 1 || dilation == 1) && (!in_act || in_act->code != 4) && x_dtype == KALLE_F32 &&
                          y_dtype == KALLE_F32;
    if (eligible && (prefer == PREFER_CFIRST ||
                     (prefer == PREFER_AUTO && conv_prefers_cfirst(B, Cin, Cout, Lout, ksize, stride)))) {
        ActArgs a;
        if (!read_act(in_act, a, false)) return KALLE_ERR_ARG;             // (kalle_conv_pad_act applies it)
        ConvCParams p{};
        const bool ws = cfirst_ws_floats(B, Cin, Cout, Lout, ksize) > 0;
        rc = plan_cfirst(true, B, Cin, conv_pad_geom(Lout, ksize, stride, padding, dilation).Lp, Cout, Lout, ksize, stride,
                         padding, dilation, epi, ws, p, pl);
    } else {
        ConvParams p{};
        rc = plan_conv1d(true, x_dtype, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding, dilation, in_act, epi, p, pl);
    }
    if (rc == KALLE_OK) report(pl, out);
    return rc;
}

extern "C" int kalle_conv_transpose_plan(int x_dtype, int y_dtype, int B, int Cin, int Lin, int Cout, int Lout, int ksize,
                                         int stride, int padding, const kalle_act* in_act, const kalle_conv_epilogue* epi,
                                         int prefer, int32_t* out) {
    if (!out || prefer < PREFER_AUTO || prefer > PREFER_POSITIONS) return KALLE_ERR_ARG;
    ConvPlan pl;
    int rc;
    const bool sane = B > 0 && Cin > 0 && Lin > 0 && Cout > 0 && Lout > 0 && ksize > 0 && stride > 0 && padding >= 0;
    // trimmed (Lout at most the symmetric length) or extended (the data gradient of a strided conv): only the former
    const bool eligible = sane && (int64_t)Lout <= (int64_t)(Lin - 1) * stride - 2 * padding + ksize &&
                          (!in_act || in_act->code != 4) && x_dtype == KALLE_F32 && y_dtype == KALLE_F32;
    if (eligible && (prefer == PREFER_CFIRST || (prefer == PREFER_AUTO && convT_prefers_cfirst(B, Cout, Lout, stride, padding)))) {
        ActArgs a;
        if (!read_act(in_act, a, false)) return KALLE_ERR_ARG;
        ConvCParams p{};
        rc = plan_cfirst_T(true, B, Cin, convT_pad_geom(Lout, ksize, stride, padding).Lp, Cout, Lout, ksize, stride, padding, epi,
                           p, pl);
    } else {
        ConvParams p{};
        rc = plan_convT(true, x_dtype, y_dtype, B, Cin, Lin, Cout, Lout, ksize, stride, padding, in_act, epi, p, pl);
    }
    if (rc == KALLE_OK) report(pl, out);
    return rc;
}

extern "C" int kalle_snake_beta_fwd(const void* x, void* y, int dtype, const float* alpha, const float* beta,
                                    int logscale, int B, int C, int L, void* stream) {
    if (!x || !y || !alpha || !beta || B <= 0 || C <= 0 || L <= 0) return KALLE_ERR_ARG;
    const int64_t total = (int64_t)B * C * L;
    int64_t g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32)
        KALLE_LAUNCH((snake_kernel<true>), dim3((unsigned)g), dim3(256), 0, st, x, y, alpha, beta, logscale, C, L, total);
    else
        KALLE_LAUNCH((snake_kernel<false>), dim3((unsigned)g), dim3(256), 0, st, x, y, alpha, beta, logscale, C, L, total);
    return kalle_check_launch();
}
