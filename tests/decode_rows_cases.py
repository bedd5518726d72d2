"""Case lists and seeded inputs of the batched decode path (kalle_gemm_rows_bf16 / kalle_gemm_rows_fused,
kalle_attention_decode_rows, kalle_llama_decode_step_rows) shared by tests/test_decode_rows_gpu.py and
tests/test_decode_rows_cpu.py (which asserts the 1 % ambiguity cap on the prologue inputs committed to here).  Inputs are drawn as
tests/decode_cases.py draws them: x and the norm weights on the CPU from the case's seed, weights and caches on the device."""
import torch

import decode_cases as dc
import kernel_refs as kr

EPS = dc.EPS
MAX_ROWS = 16
PRO_BF16, PRO_RMS, PRO_SWIGLU = 0, 1, 2

# ---- skinny GEMM: (N, K, nsplit).  70: N no multiple of the 8-row tile, one K chunk group; 1000: K no multiple of the 256-element
# block of a wave nor of the 1024 of a workgroup; (520, 2056): two blocks per wave + a ragged third, columns >= 256 to a second
# destination per row
GEMM_SHAPES = [(70, 64, 70), (264, 1000, 264), (520, 2056, 256)]
# either side of the row count from which a workgroup takes 16 weight rows instead of 8 (N >= 8192), neither a multiple of 16
GEMM_TILE_SHAPES = [(8184, 64, 8184), (8200, 72, 8200)]
GEMM_ROWS = (1, 2, 3, 8, 16)


def ambiguous(x, gamma, pro):
    """per row: how many elements of the prologue value (float64) lie within the kernel's fast-math window of a bf16 rounding
    boundary (decode_cases.rms_window / swiglu_window)"""
    out = []
    for r in range(x.shape[0]):
        if pro == PRO_RMS:
            xh = kr.decode_rms_prologue(x[r].double(), gamma.double(), EPS)
            out.append(int(kr.bf16_ambiguous(xh, dc.rms_window(xh)).sum()))
        else:
            h = x[r].double()
            out.append(int(kr.bf16_ambiguous(kr.decode_swiglu_prologue(h), dc.swiglu_window(h)).sum()))
    return out


# where the case's own seed draws an input with more ambiguous prologue elements than the cap allows (at K = 64 and 72 the
# 1 % cap allows none, and one draw in a few has one), the case takes a later seed of its sequence: found once on the CPU from
# the float64 reference alone, fixed here, and asserted by tests/test_decode_rows_cpu.py for every case
RESEED = {(70, 64, 8, 2): 1, (70, 64, 16, 2): 1, (8184, 64, 2, 1): 1, (8184, 64, 2, 2): 1, (8184, 64, 3, 1): 1, (8184, 64, 3, 2): 1,
          (8200, 72, 3, 2): 1, (8200, 72, 8, 1): 1, (8200, 72, 8, 2): 1, (8200, 72, 16, 2): 4}


def gemm_inputs(N, K, R, pro):
    """the operand of prologue `pro` for R rows (CPU): PRO_BF16 bf16 [R][K]; PRO_RMS (x fp32 [R][K], gamma fp32 [K]);
    PRO_SWIGLU hf bf16 [R][2K] = up | gate"""
    g = torch.Generator().manual_seed(7000 + 131 * N + 17 * K + R + 1000 * pro + 100000 * RESEED.get((N, K, R, pro), 0))
    if pro == PRO_BF16:
        return torch.randn((R, K), generator=g).to(torch.bfloat16), None
    if pro == PRO_RMS:
        return torch.randn((R, K), generator=g), 1 + 0.1 * torch.randn(K, generator=g)
    return torch.randn((R, 2 * K), generator=g).to(torch.bfloat16), None


# ---- attention rows: H = 4, Hkv = 2, R = 3
ATTN_NK = [(1, 257, 130), (37, 0, 37)]
ATTN_HEADS = [(64, 64), (64, 0), (128, 128)]          # (head dim, rot)


def rope_tables(npos, hd):
    """[npos][hd / 2] fp32 cos / sin of HF's rotary embedding, base 10000"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).double() / hd))
    f = torch.arange(npos).double()[:, None] * inv[None, :]
    return f.cos().float(), f.sin().float()


# ---- the step: decode_cases' smallest H / Hkv / inner at either head dim, R = 3, one inactive row
STEP_CASES = {
    "hd64": dict(hd=64, H=2, Hkv=1, inner=8, t0=(0, 37, -1), rows=40, seed=900),
    "hd128": dict(hd=128, H=2, Hkv=1, inner=8, t0=(0, 37, -1), rows=40, seed=901),
}


def step_inputs(c):
    """x fp32 [R][D], input_norm fp32 [D] (CPU)"""
    g = torch.Generator().manual_seed(c["seed"])
    D = c["hd"] * c["H"]
    return torch.randn((len(c["t0"]), D), generator=g), 1 + 0.1 * torch.randn(D, generator=g)


def ws_bytes(R, H, inner, hd):
    """the published workspace layout: x2 | x3 fp32 [R][D], lse fp32 [R][H] (region padded to 64 bytes), q | ao bf16 [R][D],
    hf bf16 [R][2 inner], xn bf16 [R][max(D, inner)]"""
    D = H * hd
    return 2 * R * D * 4 + ((R * H * 4 + 63) & ~63) + 2 * R * D * 2 + R * 2 * inner * 2 + R * max(D, inner) * 2


def gemm_rows_ref(W, X, residual=None):
    """Y[r][n] = sum_k W[n][k] X[r][k] (+ residual[r][n]), float64"""
    y = torch.einsum("nk,rk->rn", W.double(), X.double())
    return y if residual is None else y + residual.double()
