"""The fp64 attention references (tests/kernel_refs.py, "attention") on the CPU, 1e-12 relative: with round_points=False they
equal torch's scaled_dot_product_attention in float64 and float64 autograd through it (head dims 32 / 64 / 128, rot 0 / 32 / 64,
GQA 4:1 and 4:2, causal with Nk > Nq, a key mask, a fully masked batch row forward only), and the reference project's
attention through the committed golden vectors (fp32 vectors: the tolerance of tests/test_oracle_golden.py).  The last test
asserts from the references alone that every wrong reference of tests/test_attention_gpu.py moves some element of its case by
more than twice the allowance the GPU test grants, on the GPU test's own inputs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import golden_util as gu  # noqa: E402
import kernel_refs as kr  # noqa: E402
import test_attention_gpu as ag  # noqa: E402  (its case constructor, input generator, WRONG list and ALLOW; no GPU is touched)

REL = 1e-12


def _close(a, b, what="", rel=REL):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    mag = max(b.abs().max().item(), 1e-300)
    assert err <= rel * mag, (what, err, mag)


def _torch_rotary(t, cos, sin, pos):
    """transformer.py:146-170 on [B][heads][n][dh]: t cos + rotate_half(t) sin over the first 2 * cos.shape[1] dims"""
    rot = 2 * cos.shape[1]
    c, s = torch.cat([cos[pos], cos[pos]], -1), torch.cat([sin[pos], sin[pos]], -1)
    tr, tu = t[..., :rot], t[..., rot:]
    rh = torch.cat([-tr[..., rot // 2:], tr[..., :rot // 2]], -1)
    return torch.cat([tr * c + rh * s, tu], -1)


def _sdpa(q, k, v, H, Hkv, dh, rot, cos, sin, mask, causal):
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    qh = q.view(B, Nq, H, dh).transpose(1, 2)
    kh = k.view(B, Nk, Hkv, dh).transpose(1, 2)
    vh = v.view(B, Nk, Hkv, dh).transpose(1, 2)
    off = Nk - Nq if causal else 0
    if rot:
        qh = _torch_rotary(qh, cos, sin, torch.arange(Nq) + off)
        kh = _torch_rotary(kh, cos, sin, torch.arange(Nk))
    kh, vh = kh.repeat_interleave(H // Hkv, 1), vh.repeat_interleave(H // Hkv, 1)
    bias = torch.zeros(B, 1, Nq, Nk, dtype=torch.float64)
    if mask is not None:
        bias = bias.masked_fill(~mask[:, None, None, :], -torch.finfo(torch.float64).max)
    if causal:
        bias = bias.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool).triu(off + 1), -float("inf"))
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias)
    return o.transpose(1, 2).reshape(B, Nq, H * dh)


CASES = [
    dict(dh=64, H=2, Hkv=2, Nq=9, Nk=9, rot=32, causal=False, mask="random"),
    dict(dh=64, H=4, Hkv=1, Nq=7, Nk=12, rot=64, causal=True, mask="none"),
    dict(dh=64, H=4, Hkv=2, Nq=5, Nk=11, rot=0, causal=False, mask="row"),
    dict(dh=32, H=4, Hkv=2, Nq=6, Nk=10, rot=32, causal=True, mask="random"),
    dict(dh=32, H=4, Hkv=1, Nq=8, Nk=8, rot=0, causal=False, mask="first"),
    dict(dh=128, H=4, Hkv=1, Nq=5, Nk=9, rot=64, causal=True, mask="none"),
    dict(dh=128, H=2, Hkv=2, Nq=6, Nk=6, rot=32, causal=False, mask="random"),
    dict(dh=128, H=4, Hkv=2, Nq=1, Nk=7, rot=64, causal=True, mask="last_only"),
]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_references_equal_sdpa_and_autograd(c):
    c = ag.A(c["Nq"], c["Nk"], 0, **{k: v for k, v in c.items() if k not in ("Nq", "Nk")})
    x = ag.make_inputs(c)
    dh, H, Hkv, rot, causal = c["dh"], c["H"], c["Hkv"], c["rot"], c["causal"]
    cos, sin = (x["cos"].double(), x["sin"].double()) if rot else (None, None)
    mask = x["mask"]
    q, k, v = (x[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    want = _sdpa(q, k, v, H, Hkv, dh, rot, cos, sin, mask, causal)
    out, lse, p, qh, kh = kr.attention_ref(x["q"], x["k"], x["v"], H, Hkv, dh, rot, cos, sin, mask, causal)
    _close(p.sum(-1), torch.ones_like(lse), "rows of p")
    if mask is not None and not mask.any(1).all():        # fully masked batch row: uniform weights (the fill's own result; torch's
        full = ~mask.any(1)                               # fused CPU softmax does not define such a row), forward only
        _close(out[~full], want.detach()[~full], "out")
        _close(p[full], torch.full_like(p[full], 1.0 / c["Nk"]), "uniform weights")
        _close(out[full], x["v"][full].view(-1, c["Nk"], Hkv, 1, dh).mean(1, keepdim=True).expand(-1, c["Nq"], Hkv, H // Hkv, dh)
               .reshape(-1, c["Nq"], H * dh), "mean of v")
        return
    _close(out, want.detach(), "out")
    want.backward(x["dout"])
    dq, dk, dv, delta, mags = kr.attention_bwd_ref(x["q"], x["k"], x["v"], x["dout"], H, Hkv, dh, rot, cos, sin, mask, causal)
    _close(dq, q.grad, "dq"); _close(dk, k.grad, "dk"); _close(dv, v.grad, "dv")
    _close(delta, (x["dout"] * out).view(2, c["Nq"], H, dh).sum(-1).transpose(1, 2), "delta")
    for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert (mags[n] >= g.abs() * (1 - 1e-12)).all(), (n, "magnitude below the value")
    # masked_rows_zero changes nothing where every batch row has a live key
    z = kr.attention_bwd_ref(x["q"], x["k"], x["v"], x["dout"], H, Hkv, dh, rot, cos, sin, mask, causal, masked_rows_zero=True)
    _close(z[0], dq); _close(z[1], dk); _close(z[2], dv)


def test_masked_rows_zero_contract():
    """the header's backward contract in the reference: a fully masked batch row gives exact zeros, the other row is untouched"""
    c = ag.A(5, 11, 0, H=4, Hkv=2, mask="row")
    x = ag.make_inputs(c)
    a = (x["q"], x["k"], x["v"], x["dout"], 4, 2, 64, 0, None, None)
    dq, dk, dv, _, mags = kr.attention_bwd_ref(*a, x["mask"], False, masked_rows_zero=True)
    assert (dq[1] == 0).all() and (dk[1] == 0).all() and (dv[1] == 0).all() and all((m[1] == 0).all() for m in mags.values())
    one = kr.attention_bwd_ref(*(t[:1] for t in a[:4]), *a[4:], x["mask"][:1], False)
    _close(dq[:1], one[0]); _close(dk[:1], one[1]); _close(dv[:1], one[2])


def test_round_points_round_the_rotated_operands():
    c = ag.A(9, 9, 0, rot=32)
    x = ag.make_inputs(c)
    cos, sin = x["cos"].double(), x["sin"].double()
    _, _, _, qh, kh = kr.attention_ref(x["q"], x["k"], x["v"], 2, 2, 64, 32, cos, sin, None, False, round_points=True)
    _, _, _, q0, k0 = kr.attention_ref(x["q"], x["k"], x["v"], 2, 2, 64, 32, cos, sin, None, False)
    assert torch.equal(qh, kr.bf16r(q0)) and torch.equal(kh, kr.bf16r(k0)) and not torch.equal(qh, q0)


def test_references_equal_the_reference_project_goldens():
    """tests/golden/attention_self.npz / attention_cross.npz (the reference project's Attention.forward, fp32): projections in
    float64 around attention_ref / attention_bwd_ref, inputs regenerated as tests/test_oracle_golden.py does"""
    Bn, N, D, S, DC = 2, 125, 128, 7, 64
    G = os.path.join(HERE, "golden")
    T = lambda a: torch.from_numpy(np.asarray(a)).double()  # noqa: E731
    rel = lambda a, b: ((a - T(b)).norm() / T(b).norm()).item()  # noqa: E731
    dy = T(gu.make_input("dy", (Bn, N, D), 1))
    # ---- self-attention: fused qkv, partial rotary 32, key mask = query mask
    f = np.load(os.path.join(G, "attention_self.npz"))
    x, mask = T(gu.make_input("x", (Bn, N, D), 5)), torch.from_numpy(np.asarray(gu.make_mask("m", (Bn, N), 5))).bool()
    sd = {n: T(w) for n, w in gu.make_state([("to_qkv.weight", (3 * D, D)), ("to_out.weight", (D, D))], 5).items()}
    q, k, v = (x @ sd["to_qkv.weight"].t()).chunk(3, -1)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 32, 2).float() / 32))
    fr = (torch.arange(N).float()[:, None] * inv[None, :]).double()
    cos, sin = fr.cos(), fr.sin()
    o = kr.attention_ref(q, k, v, 2, 2, 64, 32, cos, sin, mask, False)[0]
    y = (o @ sd["to_out.weight"].t()).masked_fill(~mask[:, :, None], 0.0)
    assert rel(y, f["y"]) < 3e-6, rel(y, f["y"])
    do = dy.masked_fill(~mask[:, :, None], 0.0) @ sd["to_out.weight"]
    dq, dk, dv, _, _ = kr.attention_bwd_ref(q, k, v, do, 2, 2, 64, 32, cos, sin, mask, False)
    dx = torch.cat([dq, dk, dv], -1) @ sd["to_qkv.weight"]
    assert rel(dx, f["dx"]) < 3e-6, rel(dx, f["dx"])
    # ---- cross-attention: q | kv, GQA 2:1, context mask, no rotary
    f = np.load(os.path.join(G, "attention_cross.npz"))
    x, ctx = T(gu.make_input("x", (Bn, N, D), 6)), T(gu.make_input("ctx", (Bn, S, DC), 6))
    cm = torch.from_numpy(np.asarray(gu.make_mask("cm", (Bn, S), 6))).bool()
    sd = {n: T(w) for n, w in gu.make_state([("to_q.weight", (D, D)), ("to_kv.weight", (2 * DC, DC)), ("to_out.weight", (D, D))], 6).items()}
    q = x @ sd["to_q.weight"].t()
    k, v = (ctx @ sd["to_kv.weight"].t()).chunk(2, -1)
    o = kr.attention_ref(q, k, v, 2, 1, 64, 0, None, None, cm, False)[0]
    y = o @ sd["to_out.weight"].t()
    assert rel(y, f["y"]) < 3e-6, rel(y, f["y"])
    do = dy @ sd["to_out.weight"]
    dq, dk, dv, _, _ = kr.attention_bwd_ref(q, k, v, do, 2, 1, 64, 0, None, None, cm, False)
    assert rel(dq @ sd["to_q.weight"], f["dx"]) < 3e-6
    assert rel(torch.cat([dk, dv], -1) @ sd["to_kv.weight"], f["dctx"]) < 3e-6


@pytest.mark.parametrize("wrong,c", ag.WRONG, ids=[w[0] for w in ag.WRONG])
def test_every_wrong_reference_clears_the_allowance(wrong, c):
    """|wrong reference - right reference| > 2 x ALLOW x unit somewhere: a kernel within ALLOW x unit of the right one is then
    more than ALLOW x unit from the wrong one"""
    x = ag.make_inputs(c)
    dh, H, Hkv, Nq, Nk, rot, causal = (c[k] for k in ("dh", "H", "Hkv", "Nq", "Nk", "rot", "causal"))
    cos, sin = (x["cos"].double(), x["sin"].double()) if rot else (None, None)
    args = (H, Hkv, dh, rot, cos, sin, x["mask"], causal)
    fill = -1.0e30 * dh ** -0.5
    ref, lse, p, qh, kh = kr.attention_ref(x["q"], x["k"], x["v"], *args, round_points=True, mask_fill=fill)
    cleared = []
    if wrong in ("dk_missing_head", "dq_not_unrotated", "delta_dout_squared"):
        fam = ag.FAMILY[c["bwd"] & 15]
        ob = kr.bf16r(ref)
        good = kr.attention_bwd_ref(x["q"], x["k"], x["v"], x["dout"], *args, round_points=True, out=ob, masked_rows_zero=True)
        bad = kr.attention_bwd_ref(x["q"], x["k"], x["v"], x["dout"], *args, round_points=True, out=ob, masked_rows_zero=True, wrong=wrong)
        for i, n in enumerate(("dq", "dk", "dv")):
            tol = ag.ALLOW[n + "/" + fam] * 2.0 ** -9 * good[4][n]
            cleared.append(bool(((bad[i] - good[i]).abs() > 2 * tol).any()))
    else:
        fam = ag.FAMILY[c["fwd"] & 15]
        bad = kr.attention_ref(x["q"], x["k"], x["v"], *args, round_points=True, mask_fill=fill, wrong=ag.wrong_kw(wrong, c))
        u_out, u_lse = kr.attention_fwd_units(p, qh, kh, x["v"], ref, lse, H, Hkv, dh)
        cleared.append(bool(((bad[0] - ref).abs() > 2 * ag.ALLOW["out/" + fam] * 2.0 ** -9 * u_out).any()))
    assert any(cleared), (wrong, "does not clear the allowance")
