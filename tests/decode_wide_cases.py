"""Case lists and seeded inputs of the wide decode path (kalle_gemm_rows_wide, kalle_llama_decode_step_wide: 17 .. 64 rows per
read of the weights) shared by tests/test_decode_wide_gpu.py and tests/test_decode_wide_cpu.py.  Shapes, draws and the 1 % cap on
ambiguous prologue elements are those of tests/decode_rows_cases.py; the cap is a condition of the check, so a case whose draw
misses it takes the first later seed of its sequence that meets it on every row - found on the CPU from the float64 reference
alone, fixed in RESEED and asserted by the CPU test."""
import torch

import decode_rows_cases as rc

EPS = rc.EPS
MAX_ROWS, WIDE_MAX_ROWS = rc.MAX_ROWS, 64
PRO_BF16, PRO_RMS, PRO_SWIGLU = rc.PRO_BF16, rc.PRO_RMS, rc.PRO_SWIGLU

# either side of the threshold of the wide kernel's tile rule (16 weight rows per workgroup from N = 3072, 8 below), N on neither
# side a multiple of the tile; K = 264: a ragged second chunk group
WIDE_TILE_SHAPES = [(3068, 264, 3068), (3076, 264, 3076)]
GEMM_SHAPES = rc.GEMM_SHAPES + rc.GEMM_TILE_SHAPES + WIDE_TILE_SHAPES
# one row in the second column block of 16, full blocks, one row in the third block, three blocks, the bound
GEMM_ROWS = (17, 32, 33, 48, 64)

# (N, K, R, pro) -> k, the first reseed at which every row meets the cap (absent: 0)
RESEED = {
    (70, 64, 32, 1): 1, (70, 64, 32, 2): 5, (70, 64, 33, 1): 2, (70, 64, 33, 2): 13, (70, 64, 64, 1): 6, (70, 64, 64, 2): 26,
    (8184, 64, 17, 1): 1, (8184, 64, 17, 2): 1, (8184, 64, 32, 2): 12, (8184, 64, 33, 2): 4, (8184, 64, 48, 1): 3,
    (8184, 64, 48, 2): 8, (8184, 64, 64, 1): 7, (8184, 64, 64, 2): 17,
    (8200, 72, 17, 1): 1, (8200, 72, 17, 2): 3, (8200, 72, 32, 1): 10, (8200, 72, 32, 2): 2, (8200, 72, 33, 1): 1,
    (8200, 72, 33, 2): 14, (8200, 72, 48, 1): 2, (8200, 72, 48, 2): 11, (8200, 72, 64, 1): 1, (8200, 72, 64, 2): 6,
    (3068, 264, 48, 2): 1,
}


def seed(N, K, R, pro, k):
    return 7000 + 131 * N + 17 * K + R + 1000 * pro + 100000 * k


def draw(N, K, R, pro, k):
    """decode_rows_cases.gemm_inputs' draws at reseed k"""
    g = torch.Generator().manual_seed(seed(N, K, R, pro, k))
    if pro == PRO_BF16:
        return torch.randn((R, K), generator=g).to(torch.bfloat16), None
    if pro == PRO_RMS:
        return torch.randn((R, K), generator=g), 1 + 0.1 * torch.randn(K, generator=g)
    return torch.randn((R, 2 * K), generator=g).to(torch.bfloat16), None


def gemm_inputs(N, K, R, pro):
    return draw(N, K, R, pro, RESEED.get((N, K, R, pro), 0))


def under_cap(x, gamma, pro, K):
    return max(rc.ambiguous(x, gamma, pro)) <= 0.01 * K


# ---- the step: decode_rows_cases.STEP_CASES' models, two layers, 40 cache rows
def _t0_33():
    """0, 37, mid values and -1 mixed; rows 16 .. 31 all inactive"""
    t = [(0, 37, 5, -1, 12, 21, 37, 0)[r % 8] for r in range(33)]
    for r in range(16, 32):
        t[r] = -1
    return tuple(t)


STEP_T0 = {33: _t0_33(), 64: tuple((7 * r) % 38 for r in range(64))}


def step_case(name, R):
    c = dict(rc.STEP_CASES[name])
    c["t0"] = STEP_T0[R]
    c["seed"] = c["seed"] + 10 * R
    return c
