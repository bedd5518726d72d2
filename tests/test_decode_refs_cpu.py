"""CPU: the float64 references of the Llama decode step in tests/kernel_refs.py against torch / float64 equivalents written
independently (LlamaRMSNorm, F.silu, matmul, attention_ref itself against SDPA is tests/test_attention_refs_cpu.py), at 1e-12;
the bf16 boundary helpers; and the ambiguity cap of tests/test_decode_gpu.py on the exact stage-1 inputs its cases use."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc  # noqa: E402
import kernel_refs as kr  # noqa: E402


def close(a, b, what):
    err = ((a - b).abs() / (1 + b.abs())).max().item()
    assert err < 1e-12, (what, err)


class LlamaRMSNorm(torch.nn.Module):
    """transformers' LlamaRMSNorm, in the dtype of its input"""

    def __init__(self, weight, eps):
        super().__init__()
        self.weight, self.eps = weight, eps

    def forward(self, h):
        var = h.pow(2).mean(-1, keepdim=True)
        return self.weight * (h * torch.rsqrt(var + self.eps))


def _inputs(D=192, inner=40, Hkv=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return r(D), 1 + 0.1 * r(D), r(D + 2 * Hkv * 64, D) / D ** 0.5, r(2 * inner), r(D, inner), r(D)


def test_rms_prologue_and_qkv():
    x, gamma, wqkv, hf, wdown, x2 = _inputs()
    xh = LlamaRMSNorm(gamma, 1e-5)(x)
    close(kr.decode_rms_prologue(x, gamma, 1e-5), xh, "rms")
    q, kv, xh2 = kr.decode_qkv(x, gamma, 1e-5, wqkv, 192)
    y = F.linear(xh.to(torch.bfloat16).double(), wqkv)
    close(torch.cat([q, kv]), y, "qkv")
    close(xh2, xh, "xhat")
    # the wrong variants differ
    assert (kr.decode_rms_prologue(x * 1e-2, gamma, 1e-5, "no_eps") - kr.decode_rms_prologue(x * 1e-2, gamma, 1e-5)).abs().max() > 1e-3
    q2, kv2, _ = kr.decode_qkv(x, gamma, 1e-5, wqkv, 192, "kv_swapped")
    close(kv2, torch.cat([kv[64:], kv[:64]]), "swap")


def test_swiglu_prologue_and_down():
    x, gamma, wqkv, hf, wdown, x2 = _inputs()
    act = hf[:40] * F.silu(hf[40:])
    close(kr.decode_swiglu_prologue(hf), act, "swiglu")
    out, a = kr.decode_mlp_out(x2, hf, wdown)
    close(out, x2 + F.linear(act.to(torch.bfloat16).double(), wdown), "down")
    close(kr.decode_mlp_out(x2, hf, wdown, "residual_x", x)[0], x + F.linear(act.to(torch.bfloat16).double(), wdown), "residual x")
    close(kr.decode_swiglu_prologue(hf, "gate_silu_up"), hf[40:] * F.silu(hf[:40]), "gate silu up")
    close(kr.gemv(wdown, hf[:40], x2), x2 + wdown @ hf[:40], "gemv")


@pytest.mark.parametrize("t0", [0, 5])
def test_decode_attention_is_sdpa_over_the_cache(t0):
    g = torch.Generator().manual_seed(t0)
    H, Hkv = 4, 2
    q = torch.randn(H * 64, generator=g, dtype=torch.float64)
    cache = torch.randn(8, 2 * Hkv * 64, generator=g, dtype=torch.float64)
    cos, sin = dc.rope_tables(8)
    out, lse, p, qh, kh = kr.decode_attention(q, cache, H, Hkv, t0, cos.double(), sin.double())
    k = kr._rotate(cache[:t0 + 1, :Hkv * 64].reshape(-1, Hkv, 64).transpose(0, 1), cos.double(), sin.double(), 64, torch.arange(t0 + 1))
    v = cache[:t0 + 1, Hkv * 64:].reshape(-1, Hkv, 64).transpose(0, 1)
    qr = kr._rotate(q.reshape(H, 1, 64), cos.double(), sin.double(), 64, torch.tensor([t0]))
    ref = F.scaled_dot_product_attention(qr[None], k[None].repeat_interleave(2, 1), v[None].repeat_interleave(2, 1))
    close(out.reshape(H, 64), ref[0, :, 0], "attention")
    assert kr.decode_attention(q, cache, H, Hkv, 5, cos.double(), sin.double(), wrong="t0_rows")[2].shape[-1] == 5


def test_bf16_boundary_helpers():
    v = torch.tensor([1.0, 1.5, -3.0, 0.3, 100.0], dtype=torch.float64)
    assert kr.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9, 0.5]
    # spacing agrees with torch's bf16: the next number up is one ulp away
    nxt = (v.abs().to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).double()
    assert torch.equal(nxt - v.abs().to(torch.bfloat16).double(), kr.bf16_ulp(v))
    mid = 1.0 + 2.0 ** -8                                   # the boundary between 1 and 1 + 2^-7
    w = torch.tensor([mid, mid + 1e-6, mid - 1e-6, 1.0, mid + 1e-4], dtype=torch.float64)
    assert kr.bf16_ambiguous(w, torch.full_like(w, 2e-6)).tolist() == [True, True, True, False, False]
    # an ambiguous element is exactly one whose rounding a perturbation of the window can flip
    g = torch.Generator().manual_seed(1)
    z = torch.randn(20000, generator=g, dtype=torch.float64)
    win = 1e-4 * z.abs()
    flips = (kr.bf16r(z + win) != kr.bf16r(z - win))
    assert torch.equal(flips, kr.bf16_ambiguous(z, win))


@pytest.mark.parametrize("name", list(dc.CASES))
def test_ambiguity_cap_on_the_stage_1_inputs_of_every_gpu_case(name):
    """the condition of the GPU file: at most 1 % of the K elements of a prologue value lie within the prologue's fast-math
    window of a bf16 rounding boundary (the later prologues read the kernel's own x2 and hf: the GPU file asserts the cap on
    those when it runs)"""
    c = dc.CASES[name]
    x, gamma = dc.stage1_inputs(c)
    xh = kr.decode_rms_prologue(x.double(), gamma.double(), dc.EPS)
    amb = kr.bf16_ambiguous(xh, dc.rms_window(xh))
    assert amb.sum().item() <= 0.01 * xh.numel(), (name, amb.sum().item(), xh.numel())
