"""Case lists and seeded inputs of the e4m3 decode path (kalle_quantize_rows_e4m3, kalle_gemv_e4m3 / kalle_gemv_fused_e4m3,
kalle_gemm_rows_fused_e4m3, kalle_llama_decode_step_w8 / _rows_w8) for tests/test_decode_w8_gpu.py.  The cases are those of
tests/decode_cases.py (all 17 of CASES) and tests/decode_rows_cases.py moved to where the format allows them: K a multiple of 16
(a lane's unit is one 16-byte load of 16 weights), so K = 1000 / 2056 / 72 become 1008 / 2064 / 80 and inner = 8 / 2056 become
16 / 2064.  None is left out.  The one-row step takes tests/test_decode_rows_gpu.py's Setup at R = 1, whose x is
decode_rows_cases.step_inputs: at one row that is the draw of decode_cases.stage1_inputs (same seed, same count), times the
case's xscale."""
import torch

import decode_cases as dc
import decode_rows_cases as rc
import fp8_refs as f8

EPS = dc.EPS
PRO_BF16, PRO_RMS, PRO_SWIGLU = rc.PRO_BF16, rc.PRO_RMS, rc.PRO_SWIGLU

# ---- quantiser: (N, K, ldw - K, ldq - K).  The kernel takes 4 rows per workgroup (a wave each), 16 weights per lane and pass.
QUANT_SHAPES = [(1, 16, 0, 0), (7, 208, 8, 16), (9, 1040, 0, 32), (64, 2064, 24, 0)]

# ---- one-row GEMV: (N, K, ldq - K).  gemv_e4m3_kernel: a wave owns 4 rows and issues 2 x 16 bytes of each per item, so one
# full wave batch of loads is 64 lanes x 2 x 16 = 2048 weights of a row; a workgroup (2 waves) owns 8 rows below N = 8192, 16
# from there and 32 from N = 16384.
WAVE_BATCH = 2048
GEMV_SHAPES = [(1, 16, 0), (7, WAVE_BATCH - 16, 16), (9, WAVE_BATCH, 0), (9, WAVE_BATCH + 16, 16), (9, 32768, 0),
               (8188, 64, 0), (8200, 64, 16), (16380, 48, 0), (16392, 80, 0),
               # several row groups per wave TOGETHER with several K batches (the 3B up|gate GEMV, 16384 x 3072, is of this kind):
               # two groups x two batches with a ragged last workgroup, four x two likewise
               (8200, WAVE_BATCH + 16, 0), (16392, WAVE_BATCH + 16, 16)]
# (N, K, nsplit) for the prologues and the second destination; nsplit = 70 splits a wave's four rows
GEMV_FUSED_SHAPES = [(70, 2064, 70), (200, 1008, 70)]

# ---- skinny GEMM: the analogues of decode_rows_cases.GEMM_SHAPES / GEMM_TILE_SHAPES with K % 16 == 0
GEMM_SHAPES = [(70, 64, 70), (264, 1008, 264), (520, 2064, 256)]
GEMM_TILE_SHAPES = [(8184, 64, 8184), (8200, 80, 8200)]
GEMM_ROWS = rc.GEMM_ROWS


def gemm_inputs(N, K, R, pro):
    """decode_rows_cases.gemm_inputs, from the first seed of the case's sequence whose prologue values stay inside the 1 % cap on
    ambiguous elements (decided on the CPU from the float64 reference alone; at K = 64 and 80 the cap allows none and one draw in
    a few has one)"""
    for k in range(64):
        g = torch.Generator().manual_seed(9000 + 131 * N + 17 * K + R + 1000 * pro + 100000 * k)
        if pro == PRO_BF16:
            return torch.randn((R, K), generator=g).to(torch.bfloat16), None
        if pro == PRO_RMS:
            x, gamma = torch.randn((R, K), generator=g), 1 + 0.1 * torch.randn(K, generator=g)
        else:
            x, gamma = torch.randn((R, 2 * K), generator=g).to(torch.bfloat16), None
        if max(rc.ambiguous(x, gamma, pro)) <= 0.01 * K:
            return x, gamma
    raise AssertionError((N, K, R, pro))


def weights(N, K, seed):
    """(codes uint8 [N, K] random non-NaN bytes, scale fp32 [N] random in 2^-12 .. 2^4), CPU"""
    g = torch.Generator().manual_seed(seed)
    return f8.random_codes((N, K), g), (2.0 ** (torch.rand(N, generator=g, dtype=torch.float64) * 16 - 12)).float()


# ---- the steps, as decode_rows_cases.STEP_CASES writes a case (t0 a tuple, one entry per row).  "one": the one-row step
def _one(name):
    c = dc.CASES[name]
    return dict(hd=64, H=c["H"], Hkv=c["Hkv"], inner=(c["inner"] + 15) // 16 * 16, t0=(c["t0"],), rows=c["rows"], seed=c["seed"],
                xscale=c["xscale"], one=True)


# every case of decode_cases.CASES: "small-x" is the one where eps changes a bf16 rounding of xhat (the RMSNorm prologue is this
# kernel's own copy); "limit-D32768" / "limit-inner32768" are PRO_RMS / PRO_SWIGLU with 64 KiB of operand in LDS
ONE_ROW_CASES = {n: _one(n) for n in dc.CASES}
ONE_ROW_CASES["hd128"] = dict(hd=128, H=2, Hkv=1, inner=16, t0=(5,), rows=8, seed=902, one=True)
ONE_ROW_CASES["hd128-gqa2"] = dict(hd=128, H=4, Hkv=2, inner=32, t0=(37,), rows=40, seed=903, one=True)
ROWS_CASES = {n: dict(c, inner=16) for n, c in rc.STEP_CASES.items()}
# (inner = 128: the 1 % cap on ambiguous SwiGLU elements allows none below K = 100, and these are values the kernel produces)
ROWS_CASES["hd64-gqa4"] = dict(hd=64, H=4, Hkv=1, inner=128, t0=(3, -1, 0, 9), rows=12, seed=904)
