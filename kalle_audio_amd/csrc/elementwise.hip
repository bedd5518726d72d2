// HBM-bound elementwise / reduction kernels on the DiT train-step path (gfx950): vectorised 16-B
// accesses, grid-stride loops capped at 2048 blocks, fp32 math on bf16 storage.
// Reference call sites are cited per kernel.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "../../include/kalle_hip.h"

namespace {

inline int grid_for(int64_t work_items, int block) {
    int64_t g = (work_items + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// ---- SwiGLU (transformer.py:218-219: x, gate = proj(x).chunk(2); x * silu(gate)) ---------------
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const bf16_t* __restrict__ h, bf16_t* __restrict__ out,
                                                         int64_t rows, int inner) {
    const int cpr = inner >> 3;  // 8-element chunks per row
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 8;
        const i32x4 xv = *reinterpret_cast<const i32x4*>(h + r * 2 * inner + c);
        const i32x4 gv = *reinterpret_cast<const i32x4*>(h + r * 2 * inner + inner + c);
        i32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x0 = bf16lo((uint32_t)xv[j]), x1 = bf16hi((uint32_t)xv[j]);
            const float g0 = bf16lo((uint32_t)gv[j]), g1 = bf16hi((uint32_t)gv[j]);
            o[j] = (int)pack_bf16x2(x0 * siluf_(g0), x1 * siluf_(g1));
        }
        *reinterpret_cast<i32x4*>(out + r * inner + c) = o;
    }
}

// grid (inner/512, slabs): a thread keeps its 8 columns and walks rows, so the bias-gradient column sums stay in registers
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ h,
                                                         bf16_t* __restrict__ dh, float* __restrict__ dbias,
                                                         int64_t rows, int inner, int rows_per_slab) {
    __shared__ float red[4][64 * 16];
    const int lane = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 8;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t r1 = min(rows, r0 + rows_per_slab);
    float sx[8], sg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sx[e] = 0.f; sg[e] = 0.f; }
    if (c < inner) {
        for (int64_t r = r0 + ty; r < r1; r += 4) {
            const i32x4 xv = *reinterpret_cast<const i32x4*>(h + r * 2 * inner + c);
            const i32x4 gv = *reinterpret_cast<const i32x4*>(h + r * 2 * inner + inner + c);
            const i32x4 dv = *reinterpret_cast<const i32x4*>(dout + r * inner + c);
            i32x4 ox, og;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x[2] = {bf16lo((uint32_t)xv[j]), bf16hi((uint32_t)xv[j])};
                float g[2] = {bf16lo((uint32_t)gv[j]), bf16hi((uint32_t)gv[j])};
                float d[2] = {bf16lo((uint32_t)dv[j]), bf16hi((uint32_t)dv[j])};
                float dx[2], dg[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float sgm = sigmoidf_(g[e]);
                    dx[e] = d[e] * g[e] * sgm;
                    dg[e] = d[e] * x[e] * sgm * (1.f + g[e] * (1.f - sgm));
                }
                ox[j] = (int)pack_bf16x2(dx[0], dx[1]);
                og[j] = (int)pack_bf16x2(dg[0], dg[1]);
                // sum what the wgrad GEMM will see (the bf16-rounded values)
                sx[2 * j] += bf16lo((uint32_t)ox[j]); sx[2 * j + 1] += bf16hi((uint32_t)ox[j]);
                sg[2 * j] += bf16lo((uint32_t)og[j]); sg[2 * j + 1] += bf16hi((uint32_t)og[j]);
            }
            *reinterpret_cast<i32x4*>(dh + r * 2 * inner + c) = ox;
            *reinterpret_cast<i32x4*>(dh + r * 2 * inner + inner + c) = og;
        }
    }
    if (!dbias) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[ty][lane * 16 + e] = sx[e]; red[ty][lane * 16 + 8 + e] = sg[e]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
        const int l = i >> 4, e = i & 15;
        const int col = (blockIdx.x * 64 + l) * 8 + (e & 7);
        if (col < inner) atomicAdd(dbias + (e < 8 ? col : inner + col), red[0][i] + red[1][i] + red[2][i] + red[3][i]);
    }
}

// ---- SiLU --------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void silu_fwd_kernel(const void* __restrict__ x, void* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (F32) {
            static_cast<float*>(y)[i] = siluf_(static_cast<const float*>(x)[i]);
        } else {
            static_cast<bf16_t*>(y)[i] = f32_to_bf16(siluf_(bf16_to_f32(static_cast<const bf16_t*>(x)[i])));
        }
    }
}
template <bool F32>
__global__ __launch_bounds__(256) void silu_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                       void* __restrict__ dx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float xv, d;
        if constexpr (F32) { xv = static_cast<const float*>(x)[i]; d = static_cast<const float*>(dy)[i]; }
        else { xv = bf16_to_f32(static_cast<const bf16_t*>(x)[i]); d = bf16_to_f32(static_cast<const bf16_t*>(dy)[i]); }
        const float s = sigmoidf_(xv);
        const float r = d * s * (1.f + xv * (1.f - s));
        if constexpr (F32) static_cast<float*>(dx)[i] = r; else static_cast<bf16_t*>(dx)[i] = f32_to_bf16(r);
    }
}

// ---- forward noising + target (training/diffusion.py:365-379; sampling.py:8-11) --------------------
__global__ __launch_bounds__(256) void diffuse_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                      const float* __restrict__ t, float* __restrict__ xt,
                                                      float* __restrict__ target, int nbatch, int64_t per, int objective) {
    const int64_t total = (int64_t)nbatch * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / per);
        const float tv = t[b];
        float a, s;
        if (objective == 0) {
            a = cosf(tv * 1.57079632679489662f);
            s = sinf(tv * 1.57079632679489662f);
        } else {
            a = 1.f - tv;
            s = tv;
        }
        const float xv = x[i], nv = noise[i];
        xt[i] = xv * a + nv * s;
        target[i] = objective == 0 ? (nv * a - xv * s) : (nv - xv);
    }
}

// ---- MSE (training/losses/losses.py:53-69) -------------------------------------------------------
__global__ __launch_bounds__(256) void mse_fwd_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                      const uint8_t* __restrict__ mask, float* __restrict__ acc,
                                                      float* __restrict__ diff, int nbatch, int C, int T) {
    __shared__ float red[16];
    const int64_t total = (int64_t)nbatch * C * T;
    float s = 0.f, cnt = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float m = 1.f;
        if (mask) {
            const int64_t bc = i / T;
            const int tt = (int)(i - bc * T);
            const int b = (int)(bc / C);
            m = mask[(int64_t)b * T + tt] ? 1.f : 0.f;
        }
        const float d = (out[i] - target[i]) * m;
        if (diff) diff[i] = d;
        s += d * d;
        cnt += m;
    }
    s = block_sum(s, red);
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0) { atomicAdd(acc, s); atomicAdd(acc + 1, cnt); }
}
__global__ __launch_bounds__(256) void mse_finish_kernel(const float* __restrict__ acc, float* __restrict__ loss,
                                                         float* __restrict__ diff, int64_t n, float weight) {
    const float inv = 1.f / acc[1];
    if (blockIdx.x == 0 && threadIdx.x == 0 && loss) *loss = weight * acc[0] * inv;
    if (!diff) return;
    const float k = 2.f * weight * inv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        diff[i] *= k;
}

// ---- batched 2-D transpose with dtype conversion -------------------------------------------------------
template <bool IF32, bool OF32>
__global__ __launch_bounds__(256) void transpose_kernel(const void* __restrict__ in, void* __restrict__ out, int R,
                                                        int Cn, int64_t in_bs, int64_t out_bs, int64_t in_ld,
                                                        int64_t out_ld) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        float v = 0.f;
        if (r < R && c < Cn) {
            const int64_t idx = (int64_t)b * in_bs + (int64_t)r * in_ld + c;
            if constexpr (IF32) v = static_cast<const float*>(in)[idx];
            else v = bf16_to_f32(static_cast<const bf16_t*>(in)[idx]);
        }
        tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < R && c < Cn) {
            const int64_t idx = (int64_t)b * out_bs + (int64_t)c * out_ld + r;
            const float v = tile[tx][ty + 8 * i];
            if constexpr (OF32) static_cast<float*>(out)[idx] = v;
            else static_cast<bf16_t*>(out)[idx] = f32_to_bf16(v);
        }
    }
}

// ---- segment copy: the gather / paste of chunked VAE encode / decode (autoencoders.py:429-560) in ONE launch --------------
// For segment s, batch item b, channel c:  dst[s*dst_ss + b*dst_bs + c*dst_ld + dst_off[s] + j] = src[s*src_ss + b*src_bs +
// c*src_ld + src_off[s] + j], j < len[s].  Gather: src_ss = 0 (every chunk reads the same signal), dst_ss = one chunk batch;
// paste: the other way round, segments trimmed so that their destinations are disjoint.  Same element type both sides.
struct SegTable {
    int64_t src_off[KALLE_MAX_SEGMENTS], dst_off[KALLE_MAX_SEGMENTS];
    int len[KALLE_MAX_SEGMENTS];
};
template <typename T>
__global__ __launch_bounds__(256) void segment_copy_kernel(const T* __restrict__ src, T* __restrict__ dst, SegTable tab,
                                                           int nbatch, int rows, int64_t src_ss, int64_t src_bs,
                                                           int64_t src_ld, int64_t dst_ss, int64_t dst_bs, int64_t dst_ld) {
    const int row = blockIdx.y;                 // (segment, batch, channel)
    const int s = row / (nbatch * rows);
    const int br = row - s * nbatch * rows;
    const int b = br / rows, c = br - b * rows;
    const T* sp = src + s * src_ss + b * src_bs + c * src_ld + tab.src_off[s];
    T* dp = dst + s * dst_ss + b * dst_bs + c * dst_ld + tab.dst_off[s];
    const int n = tab.len[s];
    constexpr int V = 16 / sizeof(T);
    const bool vec = (((uintptr_t)sp | (uintptr_t)dp) & 15) == 0;
    if (vec) {
        const int nv = n / V;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gridDim.x * blockDim.x)
            reinterpret_cast<i32x4*>(dp)[i] = reinterpret_cast<const i32x4*>(sp)[i];
        for (int i = nv * V + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dp[i] = sp[i];
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dp[i] = sp[i];
    }
}

// ---- strided row copy with dtype conversion: out[b][r][:] = in[b][r][:]  -------------------------
template <bool IF32, bool OF32>
__global__ __launch_bounds__(256) void copy_rows_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                        int nbatch, int rows, int cols, int64_t in_bs, int64_t in_ld,
                                                        int64_t out_bs, int64_t out_ld, int accumulate) {
    const int cpr = cols >> 2;  // 4-element groups
    const int64_t total = (int64_t)nbatch * rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t br = i / cpr;
        const int c = (int)(i - br * cpr) * 4;
        const int b = (int)(br / rows);
        const int r = (int)(br - (int64_t)b * rows);
        const int64_t ii = (int64_t)b * in_bs + (int64_t)r * in_ld + c;
        const int64_t oi = (int64_t)b * out_bs + (int64_t)r * out_ld + c;
        float v[4];
        if constexpr (IF32) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(static_cast<const float*>(in) + ii);
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
        } else {
            const i32x2 a = *reinterpret_cast<const i32x2*>(static_cast<const bf16_t*>(in) + ii);
            v[0] = bf16lo((uint32_t)a[0]); v[1] = bf16hi((uint32_t)a[0]);
            v[2] = bf16lo((uint32_t)a[1]); v[3] = bf16hi((uint32_t)a[1]);
        }
        if constexpr (OF32) {
            float* op = static_cast<float*>(out) + oi;
            if (accumulate) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(op);
                v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
            *reinterpret_cast<f32x4*>(op) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            i32x2 o;
            o[0] = (int)pack_bf16x2(v[0], v[1]);
            o[1] = (int)pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<i32x2*>(static_cast<bf16_t*>(out) + oi) = o;
        }
    }
}

template <bool IF32, bool OF32>
__global__ __launch_bounds__(256) void cast_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v;
        if constexpr (IF32) v = static_cast<const float*>(in)[i];
        else v = bf16_to_f32(static_cast<const bf16_t*>(in)[i]);
        if constexpr (OF32) static_cast<float*>(out)[i] = v;
        else static_cast<bf16_t*>(out)[i] = f32_to_bf16(v);
    }
}

// ---- Fourier features (blocks.py:84-93) ---------------------------------------------------------------
template <bool OF32>
__global__ void fourier_kernel(const float* __restrict__ t, const float* __restrict__ w, void* __restrict__ out,
                               int nbatch, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbatch * half) return;
    const int b = i / half, j = i - b * half;
    const float f = 6.283185307179586f * t[b] * w[j];
    const float c = cosf(f), s = sinf(f);
    if constexpr (OF32) {
        static_cast<float*>(out)[(int64_t)b * 2 * half + j] = c;
        static_cast<float*>(out)[(int64_t)b * 2 * half + half + j] = s;
    } else {
        static_cast<bf16_t*>(out)[(int64_t)b * 2 * half + j] = f32_to_bf16(c);
        static_cast<bf16_t*>(out)[(int64_t)b * 2 * half + half + j] = f32_to_bf16(s);
    }
}

// ---- residual gradient -> bf16 operand (+ adaLN gate backward) -------------------------------------------------------------
// A thread owns 4 columns (16-byte loads of g / x_out / x_in, one 8-byte store) of a chunk of `rpc` rows of one batch element;
// the gate gradient is a sum over the element's rows: per-chunk partial sums are added atomically into the zeroed dgate
// (8 adds per value at 126 rows) - the one-thread-per-column-pair form walked all rows serially with 8-byte loads on 12 waves per
// CU and reached 2.4 TB/s of the 14 bytes per element it moves.
__global__ __launch_bounds__(128) void grad_cast_kernel(const float* __restrict__ g, const float* __restrict__ xo,
                                                        const float* __restrict__ xi, const float* __restrict__ gate,
                                                        int64_t ldg, const uint8_t* __restrict__ rmask,
                                                        bf16_t* __restrict__ gb, float* __restrict__ dgate, int rpb,
                                                        int D, int rpc) {
    const int b = blockIdx.z;
    const int col = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (col >= D) return;
    const int t0 = blockIdx.y * rpc, t1 = min(t0 + rpc, rpb);
    float s[4] = {1.f, 1.f, 1.f, 1.f};
    if (gate) {
        const f32x4 gt = *reinterpret_cast<const f32x4*>(gate + (int64_t)b * ldg + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = sigmoidf_(1.f - gt[j]);
    }
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int t = t0; t < t1; ++t) {
        const int64_t row = (int64_t)b * rpb + t;
        const float m = (rmask && !rmask[row]) ? 0.f : 1.f;
        f32x4 gv = *reinterpret_cast<const f32x4*>(g + row * D + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] *= m;
        if (gate) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(xo + row * D + col);
            const f32x4 i = *reinterpret_cast<const f32x4*>(xi + row * D + col);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += gv[j] * (o[j] - i[j]);
        }
        i32x2 w;
        w[0] = (int)pack_bf16x2(gv[0] * s[0], gv[1] * s[1]);
        w[1] = (int)pack_bf16x2(gv[2] * s[2], gv[3] * s[3]);
        *reinterpret_cast<i32x2*>(gb + row * D + col) = w;
    }
    if (gate && dgate) {
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(dgate + (int64_t)b * ldg + col + j, -(1.f - s[j]) * a[j]);
    }
}

__global__ void fourier_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ t,
                                   const float* __restrict__ w, float* __restrict__ dw, int nbatch, int half) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= half) return;
    float acc = 0.f;
    const float wj = w[j];
    for (int b = 0; b < nbatch; ++b) {
        const float k = 6.283185307179586f * t[b];
        const float f = k * wj;
        acc += k * (dout[(int64_t)b * 2 * half + half + j] * cosf(f) - dout[(int64_t)b * 2 * half + j] * sinf(f));
    }
    dw[j] = acc;
}

// ---- fused Adam / AdamW ------------------------------------------------------------------------------
// (one body for both kernels below: kalle_adam_step_ctl is bit-identical to kalle_adam_step by construction)
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g,
                                          float* __restrict__ m, float* __restrict__ v,
                                          bf16_t* __restrict__ pb, int64_t n, float lr, float b1, float b2,
                                          float eps, float wd, int decoupled, float bc1, float bc2,
                                          float gscale, const int64_t first, const int64_t stride) {
    const int64_t n4 = n >> 2;
    for (int64_t i = first; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float gr = gv[e] * gscale;
            if (decoupled) pv[e] *= (1.f - lr * wd); else gr += wd * pv[e];
            mv[e] = b1 * mv[e] + (1.f - b1) * gr;
            vv[e] = b2 * vv[e] + (1.f - b2) * gr * gr;
            const float denom = sqrtf(vv[e]) / bc2 + eps;   // torch.optim.Adam: sqrt(v)/sqrt(1-b2^t) + eps
            pv[e] -= (lr / bc1) * (mv[e] / denom);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (pb) {
            i32x2 o;
            o[0] = (int)pack_bf16x2(pv[0], pv[1]);
            o[1] = (int)pack_bf16x2(pv[2], pv[3]);
            reinterpret_cast<i32x2*>(pb)[i] = o;
        }
    }
    // tail (n % 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        float pv = p[i], gr = g[i] * gscale, mv = m[i], vv = v[i];
        if (decoupled) pv *= (1.f - lr * wd); else gr += wd * pv;
        mv = b1 * mv + (1.f - b1) * gr;
        vv = b2 * vv + (1.f - b2) * gr * gr;
        pv -= (lr / bc1) * (mv / (sqrtf(vv) / bc2 + eps));
        p[i] = pv; m[i] = mv; v[i] = vv;
        if (pb) pb[i] = f32_to_bf16(pv);
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16_t* __restrict__ pb, int64_t n, float lr, float b1, float b2,
                                                   float eps, float wd, int decoupled, float bc1, float bc2,
                                                   float gscale) {
    adam_body(p, g, m, v, pb, n, lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale,
              (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// the same step under the decision kalle_grad_norm_finish left in device memory: nothing is written on a skipped step, and the
// clip coefficient rides on grad_scale as ONE fp32 product
__global__ __launch_bounds__(256) void adam_ctl_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       bf16_t* __restrict__ pb, int64_t n, float lr, float b1, float b2,
                                                       float eps, float wd, int decoupled, float bc1, float bc2,
                                                       float gscale, const kalle_opt_ctl* __restrict__ ctl) {
    if (ctl->skip) return;
    adam_body(p, g, m, v, pb, n, lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale * ctl->coef,
              (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// ---- gradient norm: per-workgroup partial sums of squares (double) + non-finite flag ---------------------------------
__device__ __forceinline__ void sumsq_acc(const f32x4 x, double& acc, uint32_t& bad) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xe = x[e];      // (a copy: __builtin_bit_cast applied to the vector element itself reads element 0)
        const double d = (double)xe;
        acc += d * d;
        bad |= (uint32_t)((__builtin_bit_cast(uint32_t, xe) & 0x7f800000u) == 0x7f800000u);
    }
}

// grid = KALLE_GRAD_NORM_PARTIALS workgroups of KALLE_GRAD_NORM_BLOCK lanes, always: workgroup b owns partial b of the slot.
// Every address read is below g + n: the vector loops stop at n4 = n / 4 vectors, the tail reads n4 * 4 + lane < n.
__global__ __launch_bounds__(KALLE_GRAD_NORM_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                                           double* __restrict__ part,
                                                                           int32_t* __restrict__ flag) {
    __shared__ double red[KALLE_GRAD_NORM_BLOCK / 64];
    __shared__ uint32_t redbad[KALLE_GRAD_NORM_BLOCK / 64];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * KALLE_GRAD_NORM_BLOCK;
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g);
    double acc = 0.0;
    uint32_t bad = 0;
    int64_t i = (int64_t)blockIdx.x * KALLE_GRAD_NORM_BLOCK + threadIdx.x;
    static_assert(KALLE_GRAD_NORM_UNROLL == 4, "the main loop below issues four loads");
    for (; i + 3 * stride < n4; i += 4 * stride) {      // four 16-byte loads in flight per lane
        const f32x4 x0 = gv[i], x1 = gv[i + stride], x2 = gv[i + 2 * stride], x3 = gv[i + 3 * stride];
        sumsq_acc(x0, acc, bad);
        sumsq_acc(x1, acc, bad);
        sumsq_acc(x2, acc, bad);
        sumsq_acc(x3, acc, bad);
    }
    for (; i < n4; i += stride) sumsq_acc(gv[i], acc, bad);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {     // scalar tail (n % 4)
        const float x = g[(n4 << 2) + threadIdx.x];
        const double d = (double)x;
        acc += d * d;
        bad |= (uint32_t)((__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                  // per wave, a fixed butterfly
        acc += __shfl_xor(acc, o, 64);
        bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[w] = acc; redbad[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {                             // per block through LDS, waves in index order
        double t = 0.0;
        uint32_t b = 0;
        for (int k = 0; k < KALLE_GRAD_NORM_BLOCK / 64; ++k) { t += red[k]; b |= redbad[k]; }
        part[blockIdx.x] = t;
        flag[blockIdx.x] = (int32_t)(b != 0);
    }
}

// one workgroup: lane t adds partials t, t + 256, ... of the regions laid end to end (index order), then a fixed tree over LDS
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const char* __restrict__ ws, int nslots, float grad_scale,
                                                               float max_norm, int skip_nonfinite,
                                                               kalle_opt_ctl* __restrict__ ctl) {
    __shared__ double red[256];
    __shared__ int redbad[256];
    double acc = 0.0;
    int bad = 0;
    const int total = nslots * KALLE_GRAD_NORM_PARTIALS;
    for (int i = threadIdx.x; i < total; i += 256) {
        const char* base = ws + (int64_t)(i / KALLE_GRAD_NORM_PARTIALS) * KALLE_GRAD_NORM_SLOT_BYTES;
        const int j = i % KALLE_GRAD_NORM_PARTIALS;
        acc += reinterpret_cast<const double*>(base)[j];
        bad |= reinterpret_cast<const int32_t*>(base + KALLE_GRAD_NORM_PARTIALS * 8)[j];
    }
    red[threadIdx.x] = acc;
    redbad[threadIdx.x] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[threadIdx.x] += red[threadIdx.x + o];
            redbad[threadIdx.x] |= redbad[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)(sqrt(red[0]) * (double)grad_scale);
        float coef = 1.f;
        if (max_norm > 0.f && max_norm < __builtin_inff()) {
            const double c = (double)max_norm / ((double)norm + 1e-6);
            coef = c < 1.0 ? (float)c : 1.f;
        }
        const int nonfinite = redbad[0] != 0;
        const int skip = nonfinite && skip_nonfinite;
        ctl->norm = norm;
        ctl->coef = coef;
        ctl->nonfinite = nonfinite;
        ctl->skip = skip;
        ctl->skipped += skip;
        ctl->clipped += coef < 1.f;
    }
}

}  // namespace

extern "C" int kalle_swiglu_fwd(const void* h, void* out, int64_t rows, int inner, void* stream) {
    if (!h || !out || rows <= 0 || inner <= 0 || (inner & 7)) return KALLE_ERR_ARG;
    KALLE_LAUNCH(swiglu_fwd_kernel, dim3(grid_for(rows * (inner >> 3), 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(h), static_cast<bf16_t*>(out), rows,
                       inner);
    return kalle_check_launch();
}
extern "C" int kalle_swiglu_bwd(const void* dout, const void* h, void* dh, float* dbias, int64_t rows, int inner,
                                void* stream) {
    if (!dout || !h || !dh || rows <= 0 || inner <= 0 || (inner & 7)) return KALLE_ERR_ARG;
    const int gx = (inner + 511) / 512;
    int slabs = (1536 + gx - 1) / gx;
    if ((int64_t)slabs * 32 > rows) slabs = (int)((rows + 31) / 32);
    if (slabs < 1) slabs = 1;
    const int rps = (int)((rows + slabs - 1) / slabs);
    slabs = (int)((rows + rps - 1) / rps);
    KALLE_LAUNCH(swiglu_bwd_kernel, dim3(gx, slabs), dim3(256), 0, static_cast<hipStream_t>(stream),
                 static_cast<const bf16_t*>(dout), static_cast<const bf16_t*>(h), static_cast<bf16_t*>(dh), dbias, rows,
                 inner, rps);
    return kalle_check_launch();
}
extern "C" int kalle_silu_fwd(const void* x, void* y, int dtype, int64_t n, void* stream) {
    if (!x || !y || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32) KALLE_LAUNCH((silu_fwd_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, n);
    else KALLE_LAUNCH((silu_fwd_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, x, y, n);
    return kalle_check_launch();
}
extern "C" int kalle_silu_bwd(const void* dy, const void* x, void* dx, int dtype, int64_t n, void* stream) {
    if (!dy || !x || !dx || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == KALLE_F32) KALLE_LAUNCH((silu_bwd_kernel<true>), dim3(grid_for(n, 256)), dim3(256), 0, st, dy, x, dx, n);
    else KALLE_LAUNCH((silu_bwd_kernel<false>), dim3(grid_for(n, 256)), dim3(256), 0, st, dy, x, dx, n);
    return kalle_check_launch();
}
extern "C" int kalle_diffuse_fwd(const float* x, const float* noise, const float* t, float* x_t, float* target,
                                 int nbatch, int64_t per_sample, int objective, void* stream) {
    if (!x || !noise || !t || !x_t || !target || nbatch <= 0 || per_sample <= 0 || (objective != 0 && objective != 1))
        return KALLE_ERR_ARG;
    KALLE_LAUNCH(diffuse_kernel, dim3(grid_for((int64_t)nbatch * per_sample, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, noise, t, x_t, target, nbatch, per_sample, objective);
    return kalle_check_launch();
}
extern "C" int kalle_mse_fwd(const float* out, const float* target, const uint8_t* mask, float* loss_acc, float* diff,
                             int nbatch, int C, int T, void* stream) {
    if (!out || !target || !loss_acc || nbatch <= 0 || C <= 0 || T <= 0) return KALLE_ERR_ARG;
    int g = grid_for((int64_t)nbatch * C * T, 256);
    if (g > 1024) g = 1024;
    KALLE_LAUNCH(mse_fwd_kernel, dim3(g), dim3(256), 0, static_cast<hipStream_t>(stream), out, target, mask,
                       loss_acc, diff, nbatch, C, T);
    return kalle_check_launch();
}
extern "C" int kalle_mse_finish(float* loss_acc, float* loss, float* diff, int64_t n, float weight, void* stream) {
    if (!loss_acc || n < 0) return KALLE_ERR_ARG;
    KALLE_LAUNCH(mse_finish_kernel, dim3(diff ? grid_for(n, 256) : 1), dim3(256), 0,
                       static_cast<hipStream_t>(stream), loss_acc, loss, diff, n, weight);
    return kalle_check_launch();
}
extern "C" int kalle_transpose_2d(const void* in, int in_dtype, int64_t in_batch_stride, int64_t in_ld, void* out,
                                  int out_dtype, int64_t out_batch_stride, int64_t out_ld, int nbatch, int R, int Cn,
                                  void* stream) {
    if (!in || !out || nbatch <= 0 || R <= 0 || Cn <= 0 || nbatch > 65535) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((Cn + 31) / 32, (R + 31) / 32, nbatch), block(256);
    const bool i32 = in_dtype == KALLE_F32, o32 = out_dtype == KALLE_F32;
#define TL(I, O) KALLE_LAUNCH((transpose_kernel<I, O>), grid, block, 0, st, in, out, R, Cn, in_batch_stride, \
                                    out_batch_stride, in_ld, out_ld)
    if (i32 && o32) TL(true, true); else if (i32) TL(true, false); else if (o32) TL(false, true); else TL(false, false);
#undef TL
    return kalle_check_launch();
}
extern "C" int kalle_copy_rows(const void* in, int in_dtype, int64_t in_batch_stride, int64_t in_ld, void* out,
                               int out_dtype, int64_t out_batch_stride, int64_t out_ld, int nbatch, int rows, int cols,
                               int accumulate, void* stream) {
    if (!in || !out || nbatch <= 0 || rows <= 0 || cols <= 0 || (cols & 3) || (in_ld & 3) || (out_ld & 3) ||
        (in_batch_stride & 3) || (out_batch_stride & 3))
        return KALLE_ERR_ARG;
    if (accumulate && out_dtype != KALLE_F32) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(grid_for((int64_t)nbatch * rows * (cols >> 2), 256)), block(256);
    const bool i32 = in_dtype == KALLE_F32, o32 = out_dtype == KALLE_F32;
#define CL(I, O) KALLE_LAUNCH((copy_rows_kernel<I, O>), grid, block, 0, st, in, out, nbatch, rows, cols, \
                                    in_batch_stride, in_ld, out_batch_stride, out_ld, accumulate)
    if (i32 && o32) CL(true, true); else if (i32) CL(true, false); else if (o32) CL(false, true); else CL(false, false);
#undef CL
    return kalle_check_launch();
}
extern "C" int kalle_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, void* stream) {
    if (!in || !out || n <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(grid_for(n, 256)), block(256);
    const bool i32 = in_dtype == KALLE_F32, o32 = out_dtype == KALLE_F32;
#define CK(I, O) KALLE_LAUNCH((cast_kernel<I, O>), grid, block, 0, st, in, out, n)
    if (i32 && o32) CK(true, true); else if (i32) CK(true, false); else if (o32) CK(false, true); else CK(false, false);
#undef CK
    return kalle_check_launch();
}
extern "C" int kalle_fourier_features(const float* t, const float* w, void* out, int out_dtype, int nbatch, int half,
                                      void* stream) {
    if (!t || !w || !out || nbatch <= 0 || half <= 0) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((nbatch * half + 255) / 256), block(256);
    if (out_dtype == KALLE_F32) KALLE_LAUNCH((fourier_kernel<true>), grid, block, 0, st, t, w, out, nbatch, half);
    else KALLE_LAUNCH((fourier_kernel<false>), grid, block, 0, st, t, w, out, nbatch, half);
    return kalle_check_launch();
}
extern "C" int kalle_grad_cast(const float* g, const float* x_out, const float* x_in, const float* gate, int64_t ldg,
                               const uint8_t* row_mask, void* gb, float* dgate, int nbatch, int rows_per_batch, int D,
                               void* stream) {
    if (!g || !gb || nbatch <= 0 || rows_per_batch <= 0 || D <= 0 || (D & 3) || nbatch > 65535) return KALLE_ERR_ARG;
    if (gate && (!x_out || !x_in || (ldg & 3))) return KALLE_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (gate && dgate) {        // the kernel adds per-chunk partial sums
        if (hipMemset2DAsync(dgate, sizeof(float) * ldg, 0, sizeof(float) * D, nbatch, st) != hipSuccess) return KALLE_ERR_LAUNCH;
    }
    const int rpc = 16;
    const int chunks = (rows_per_batch + rpc - 1) / rpc;
    if (chunks > 65535) return KALLE_ERR_ARG;
    dim3 block(128), grid((D / 4 + 127) / 128, chunks, nbatch);
    KALLE_LAUNCH(grad_cast_kernel, grid, block, 0, st, g, x_out, x_in, gate, ldg,
                       row_mask, static_cast<bf16_t*>(gb), dgate, rows_per_batch, D, rpc);
    return kalle_check_launch();
}
extern "C" int kalle_fourier_features_bwd(const float* dout, const float* t, const float* w, float* dw, int nbatch,
                                          int half, void* stream) {
    if (!dout || !t || !w || !dw || nbatch <= 0 || half <= 0) return KALLE_ERR_ARG;
    KALLE_LAUNCH(fourier_bwd_kernel, dim3((half + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream),
                       dout, t, w, dw, nbatch, half);
    return kalle_check_launch();
}
extern "C" int kalle_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                               int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int decoupled, int step, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return KALLE_ERR_ARG;
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2 = sqrtf(1.f - powf(beta2, (float)step));
    // 30 B / parameter of pure streaming: 16 k workgroups measured 4 % faster than the 2 k grid-stride default
    const int agrid = (int)std::min<int64_t>(((n >> 2) + 255) / 256 + 1, 16384);
    KALLE_LAUNCH(adam_kernel, dim3(agrid), dim3(256), 0, static_cast<hipStream_t>(stream), param,
                       grad, exp_avg, exp_avg_sq, static_cast<bf16_t*>(param_bf16), n, lr, beta1, beta2, eps,
                       weight_decay, decoupled, bc1, bc2, grad_scale);
    return kalle_check_launch();
}

extern "C" int kalle_adam_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   int decoupled, int step, float grad_scale, const kalle_opt_ctl* ctl, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !ctl || n <= 0 || step <= 0) return KALLE_ERR_ARG;
    if ((uintptr_t)ctl & 7) return KALLE_ERR_ARG;
    const float bc1 = 1.f - powf(beta1, (float)step);       // host-computed from `step`, exactly as kalle_adam_step
    const float bc2 = sqrtf(1.f - powf(beta2, (float)step));
    const int agrid = (int)std::min<int64_t>(((n >> 2) + 255) / 256 + 1, 16384);
    KALLE_LAUNCH(adam_ctl_kernel, dim3(agrid), dim3(256), 0, static_cast<hipStream_t>(stream), param,
                       grad, exp_avg, exp_avg_sq, static_cast<bf16_t*>(param_bf16), n, lr, beta1, beta2, eps,
                       weight_decay, decoupled, bc1, bc2, grad_scale, ctl);
    return kalle_check_launch();
}
extern "C" int kalle_grad_norm_ws_bytes(int nslots) {
    if (nslots <= 0 || nslots > (1 << 16)) return KALLE_ERR_ARG;
    return nslots * KALLE_GRAD_NORM_SLOT_BYTES;
}
extern "C" int kalle_grad_sumsq(const float* grad, int64_t n, void* ws, int slot, int nslots, void* stream) {
    if (!grad || !ws || n <= 0 || nslots <= 0 || nslots > (1 << 16) || slot < 0 || slot >= nslots) return KALLE_ERR_ARG;
    if (((uintptr_t)grad & 15) || ((uintptr_t)ws & 15)) return KALLE_ERR_ARG;
    char* base = static_cast<char*>(ws) + (int64_t)slot * KALLE_GRAD_NORM_SLOT_BYTES;
    KALLE_LAUNCH(grad_sumsq_kernel, dim3(KALLE_GRAD_NORM_PARTIALS), dim3(KALLE_GRAD_NORM_BLOCK), 0,
                 static_cast<hipStream_t>(stream), grad, n, reinterpret_cast<double*>(base),
                 reinterpret_cast<int32_t*>(base + KALLE_GRAD_NORM_PARTIALS * 8));
    return kalle_check_launch();
}
extern "C" int kalle_grad_norm_finish(const void* ws, int nslots, float grad_scale, float max_norm, int skip_nonfinite,
                                      kalle_opt_ctl* ctl, void* stream) {
    if (!ws || !ctl || nslots <= 0 || nslots > (1 << 16)) return KALLE_ERR_ARG;
    if (((uintptr_t)ws & 15) || ((uintptr_t)ctl & 7)) return KALLE_ERR_ARG;
    KALLE_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                 static_cast<const char*>(ws), nslots, grad_scale, max_norm, skip_nonfinite, ctl);
    return kalle_check_launch();
}

static thread_local char g_last_error[128] = "";
extern "C" void kalle_set_last_error(const char* what) {
    snprintf(g_last_error, sizeof(g_last_error), "%s", what ? what : "");
}
extern "C" const char* kalle_last_error(void) { return g_last_error; }
extern "C" int kalle_abi_version(void) { return 2; }   // 2: kalle_gemm_epilogue.workspace, kalle_gemm_wgrad_group, conv backward
extern "C" const char* kalle_target_arch(void) { return "gfx950"; }

extern "C" int kalle_segment_copy(const void* src, void* dst, int dtype, int nseg, const int64_t* src_off,
                                  const int64_t* dst_off, const int* len, int nbatch, int rows, int64_t src_seg_stride,
                                  int64_t src_batch_stride, int64_t src_ld, int64_t dst_seg_stride,
                                  int64_t dst_batch_stride, int64_t dst_ld, void* stream) {
    if (!src || !dst || !src_off || !dst_off || !len || nseg <= 0 || nseg > KALLE_MAX_SEGMENTS || nbatch <= 0 || rows <= 0)
        return KALLE_ERR_ARG;
    if (dtype != KALLE_F32 && dtype != KALLE_BF16) return KALLE_ERR_ARG;
    if ((int64_t)nseg * nbatch * rows > 65535) return KALLE_ERR_ARG;
    SegTable tab{};
    int maxlen = 0;
    for (int i = 0; i < nseg; ++i) {
        if (len[i] < 0 || src_off[i] < 0 || dst_off[i] < 0) return KALLE_ERR_ARG;
        tab.src_off[i] = src_off[i]; tab.dst_off[i] = dst_off[i]; tab.len[i] = len[i];
        maxlen = len[i] > maxlen ? len[i] : maxlen;
    }
    if (maxlen == 0) return KALLE_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per = dtype == KALLE_F32 ? 4 : 8;
    int gx = (maxlen / per + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    dim3 grid(gx, nseg * nbatch * rows), block(256);
    if (dtype == KALLE_F32)
        KALLE_LAUNCH(segment_copy_kernel<float>, grid, block, 0, st, static_cast<const float*>(src), static_cast<float*>(dst), tab,
                     nbatch, rows, src_seg_stride, src_batch_stride, src_ld, dst_seg_stride, dst_batch_stride, dst_ld);
    else
        KALLE_LAUNCH(segment_copy_kernel<bf16_t>, grid, block, 0, st, static_cast<const bf16_t*>(src), static_cast<bf16_t*>(dst),
                     tab, nbatch, rows, src_seg_stride, src_batch_stride, src_ld, dst_seg_stride, dst_batch_stride, dst_ld);
    return kalle_check_launch();
}
