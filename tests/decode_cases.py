"""Case list and seeded inputs of kalle_llama_decode_step shared by tests/test_decode_gpu.py and tests/test_decode_refs_cpu.py
(which asserts the ambiguity cap on the stage-1 inputs).  x and the norm weights are made on the CPU from the case's seed; the
weights and the cache are made on the device (the largest case has 4.3 GB of them)."""
import torch

EPS = 1e-5
U = 2.0 ** -24
RSQRT_U, SIGMOID_U = 10.0, 10.0        # ALLOW["RSQRT"] / ALLOW["SIGMOID"] of tests/test_norm_elementwise_gpu.py (measured there, x 4)
KB = 256                               # keys scored per pass by the single-query attention kernel (attn_decode_kernel: one per thread)
PV_GROUPS = 32                         # key rows its P V pass handles at a time (8 threads per row)

# name -> H, Hkv, inner, t0, cache_rows, seed, xscale.  D = 64 H; the GEMVs have K = D (qkv, o, up|gate) and K = inner (down)
CASES = {
    "base": dict(H=2, Hkv=1, inner=8, t0=3, rows=6),
    "gqa1": dict(H=2, Hkv=2, inner=8, t0=3, rows=6),
    "gqa4": dict(H=4, Hkv=1, inner=16, t0=3, rows=6),
    "t0-0": dict(H=2, Hkv=1, inner=8, t0=0, rows=3),
    "t0-kb-1": dict(H=2, Hkv=1, inner=8, t0=KB - 1, rows=KB + 4),
    "t0-kb": dict(H=2, Hkv=1, inner=8, t0=KB, rows=KB + 4),
    "t0-kb+1": dict(H=2, Hkv=1, inner=8, t0=KB + 1, rows=KB + 4),
    "t0-pv-groups": dict(H=2, Hkv=1, inner=8, t0=PV_GROUPS, rows=PV_GROUPS + 2),             # 33 keys
    "t0-last-row": dict(H=2, Hkv=1, inner=8, t0=6, rows=7),
    "k-batches-D2112": dict(H=33, Hkv=11, inner=8, t0=3, rows=6),          # K = 2112: 264 chunks, the second batch of 256 ragged
    "k-batches-inner2056": dict(H=2, Hkv=1, inner=2056, t0=3, rows=6),     # down: 257 chunks
    "rpw2": dict(H=2, Hkv=1, inner=4096, t0=3, rows=6),                    # up|gate N = 8192: two row pairs per wave
    "rpw4": dict(H=2, Hkv=1, inner=8192, t0=3, rows=6),                    # N = 16384: four
    "llama-3.2-1b": dict(H=32, Hkv=8, inner=8192, t0=70, rows=72),
    "small-x": dict(H=2, Hkv=1, inner=8, t0=3, rows=6, xscale=3e-3),        # mean(x^2) ~ eps: eps matters
    "limit-inner32768": dict(H=2, Hkv=1, inner=32768, t0=3, rows=6),
    "limit-D32768": dict(H=512, Hkv=1, inner=8, t0=3, rows=6),
}
for _i, _c in enumerate(CASES.values()):
    _c.setdefault("seed", 100 + _i)
    _c.setdefault("xscale", 1.0)


def rope_tables(npos):
    """[npos][32] fp32 cos / sin of HF's rotary embedding at head dim 64, base 10000"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2).double() / 64))
    f = torch.arange(npos).double()[:, None] * inv[None, :]
    return f.cos().float(), f.sin().float()


def stage1_inputs(c):
    """x fp32 [D], input_norm fp32 [D] (CPU)"""
    g = torch.Generator().manual_seed(c["seed"])
    D = 64 * c["H"]
    return torch.randn(D, generator=g) * c["xscale"], 1 + 0.1 * torch.randn(D, generator=g)


def rms_window(xh):
    """how far the kernel's fp32 prologue value may lie from the float64 one: rsqrtf (RSQRT_U), the fp32 sum of K squares
    (K / 256 adds per lane + 10 across lanes, halved by the square root), three roundings in x * (gamma * rr)"""
    K = xh.numel()
    return (RSQRT_U + (K / 256 + 10) / 2 + 3) * U * xh.abs()


def swiglu_window(hf):
    """up * silu(gate): silu carries (SIGMOID_U + 3) u |gate| (test_norm_elementwise_gpu.py), one more rounding in the product"""
    inner = hf.numel() // 2
    return (SIGMOID_U + 4) * U * (hf[:inner] * hf[inner:]).abs()
