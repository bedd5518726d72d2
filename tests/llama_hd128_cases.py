"""Case lists and seeded inputs of the head-dim-128 Llama path shared by tests/test_llama_hd128_gpu.py and
tests/test_llama_hd128_cpu.py: the tiled forward / two-pass backward at rot = 128, the single-query kernel at head dim 128
(attn_decode128_kernel through kalle_attention_decode_hd) and kalle_llama_decode_step_hd at head_dim = 128.  The attention
cases are the dicts of tests/test_attention_gpu.py (A); the decode-step cases mirror tests/decode_cases.py with D = 128 H."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import golden_util as gu  # noqa: E402
from test_attention_gpu import A, tiled, two_pass  # noqa: E402

HD = 128
KB128 = 128            # keys scored per pass by attn_decode128_kernel (two lanes per key, 256 threads)
PV_GROUPS128 = 16      # key rows its P V pass handles at a time (16 threads per row)
SEED = 140             # of tests/golden/llasa_hd128.npz


def decode128(rot=128):
    """kalle_attn_last_plan: family 6, head dim 128, ROT in bits 17-24"""
    return 6 | 128 << 8 | rot << 17


def decode64(rot):
    return 2 | 64 << 8 | rot << 17


def llasa_config():
    """the config of tests/golden/make_golden_llama_hd128.py: LLASA_WIDE_CONFIG with 2 heads of 128 over 1 kv head"""
    lc = dict(gu.LLASA_WIDE_CONFIG)
    lc["llama"] = dict(lc["llama"], hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                       intermediate_size=512, num_hidden_layers=2)
    return lc


# ------------------------------------------------------------------------------------------------ attention
T128, TP128 = tiled(128), two_pass(128)
K = dict(dh=128, rot=128)
# the folded tail is OFF at (130, 130): rot != 0
TILED_CASES = [
    A(2, 2, T128, TP128, causal=True, layout="fused", **K),
    A(17, 17, T128, TP128, causal=True, H=4, Hkv=1, **K),
    A(128, 128, T128, TP128, causal=True, mask="row", **K),
    A(129, 129, T128, TP128, causal=True, H=4, Hkv=2, layout="fused", **K),
    A(60, 191, T128, TP128, causal=True, **K),
    A(130, 130, T128, TP128, mask="random", **K),
    A(257, 257, T128, TP128, causal=True, **K),
]
WRONG = [
    ("rotate_half_sign", A(128, 128, T128, None, mask="random", layout="fused", **K)),
    ("query_position", A(60, 65, T128, None, causal=True, H=4, Hkv=1, **K)),
    ("dq_not_unrotated", A(17, 17, T128, TP128, mask="random", **K)),
]
# single query, the LAST position: causal in the reference's terms (rotary position Nk - 1).  The issue's lengths, then each side of
# a scoring pass (KB128) and of a P V pass (PV_GROUPS128) and of two of each
DECODE_CASES = [A(1, Nk, decode128(), None, causal=True, H=H, Hkv=Hkv, mask=mask, **K)
                for Nk, (H, Hkv), mask in [
                    (1, (2, 2), "none"), (7, (4, 1), "random"), (8, (4, 1), "none"), (31, (2, 2), "last_only"),
                    (32, (4, 1), "random"), (33, (4, 2), "none"), (255, (4, 1), "first"), (256, (2, 2), "random"),
                    (257, (4, 1), "last_only"), (1025, (4, 1), "random"),
                    (PV_GROUPS128 - 1, (4, 2), "first"), (PV_GROUPS128, (2, 2), "none"), (PV_GROUPS128 + 1, (4, 1), "random"),
                    (KB128 - 1, (4, 2), "random"), (KB128, (4, 1), "none"), (KB128 + 1, (2, 2), "first")]]


# ------------------------------------------------------------------------------------------------ decode step
EPS = 1e-5
# name -> H, Hkv, inner, t0, cache_rows.  D = 128 H; Nk = t0 + 1 keys
STEP_CASES = {
    "base": dict(H=2, Hkv=1, inner=8, t0=3, rows=6),
    "gqa1": dict(H=2, Hkv=2, inner=8, t0=3, rows=6),
    "gqa4": dict(H=4, Hkv=1, inner=16, t0=3, rows=6),
    "t0-0": dict(H=2, Hkv=1, inner=8, t0=0, rows=3),
    "t0-kb-1": dict(H=2, Hkv=1, inner=8, t0=KB128 - 1, rows=KB128 + 4),
    "t0-kb": dict(H=2, Hkv=1, inner=8, t0=KB128, rows=KB128 + 4),
    "t0-kb+1": dict(H=2, Hkv=1, inner=8, t0=KB128 + 1, rows=KB128 + 4),
    "t0-last-row": dict(H=2, Hkv=1, inner=8, t0=6, rows=7),
    "llama-3.2-3b": dict(H=24, Hkv=8, inner=8192, t0=70, rows=72),
    "limit-D32768": dict(H=256, Hkv=1, inner=8, t0=3, rows=6),
}
for _i, _c in enumerate(STEP_CASES.values()):
    _c.setdefault("seed", 300 + _i)
    _c.setdefault("xscale", 1.0)


def rope_tables(npos):
    """[npos][64] fp32 cos / sin of HF's rotary embedding at head dim 128, base 10000"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2).double() / HD))
    f = torch.arange(npos).double()[:, None] * inv[None, :]
    return f.cos().float(), f.sin().float()


def stage1_inputs(c):
    """x fp32 [D], input_norm fp32 [D] (CPU)"""
    g = torch.Generator().manual_seed(c["seed"])
    D = HD * c["H"]
    return torch.randn(D, generator=g) * c["xscale"], 1 + 0.1 * torch.randn(D, generator=g)
