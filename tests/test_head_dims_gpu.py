"""-m gpu: attention and qk_norm at head dims 32 and 128 (Attention(dim_heads=...), DiffusionTransformer(embed_dim, num_heads)
with dim_heads = embed_dim // num_heads, dit.py:118).

  * kernel level: kalle_attention_fwd_hd / _bwd_hd against an fp64 torch product - self and cross layouts read in place with
    leading dimensions and column offsets, GQA groups 1 / 2 / 4, rotary 0 / 32 / 64, key mask with a fully masked batch row,
    causal with Nq <= Nk, Nq = 1 (decoding), any Nk (multi-block online softmax); forward output, lse, dQ / dK / dV;
  * the _hd entry points at head dim 64 are bit-identical to the original ones;
  * kalle_head_norm_*_hd ("l2" / "ln") against torch;
  * the modules (Attention, TransformerBlock, DiffusionTransformer) against the CPU oracle, a DataParallelTrainer step, and
    generate_diffusion_cond with HIP-graph replay against the eager launches.
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import golden_util as gu  # noqa: E402
import kalle_oracle as ko  # noqa: E402

DIT_ROT = {32: 32, 64: 32, 128: 64}       # RotaryEmbedding(max(dh // 2, 32)) (transformer.py:730)


def rel_l2(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _mk(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops(dev):
    from kalle_audio_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ kernel level
def _tables(n, rot, dev):
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2).double() / rot))
    f = torch.arange(n).double()[:, None] * inv[None, :]
    return f.cos().float().contiguous().to(dev), f.sin().float().contiguous().to(dev)


def _rotate(t, cos, sin, pos, rot):
    """t [B, H, N, dh] fp64; rotary on the first `rot` dims at positions `pos` (rotate_half, transformer.py:146-170)"""
    if rot == 0:
        return t
    c = torch.cat([cos, cos], -1)[pos].double()[None, None]
    s = torch.cat([sin, sin], -1)[pos].double()[None, None]
    r, u = t[..., :rot], t[..., rot:]
    x1, x2 = r[..., :rot // 2], r[..., rot // 2:]
    return torch.cat([r * c + torch.cat([-x2, x1], -1) * s, u], -1)


def _ref(q, k, v, H, Hkv, dh, rot, tabs, mask, causal):
    """fp64: q [B, Nq, H*dh], k / v [B, Nk, Hkv*dh] -> (out [B, Nq, H*dh], lse [B, H, Nq])"""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    off = Nk - Nq if causal else 0
    qh = q.view(B, Nq, H, dh).transpose(1, 2)
    kh = k.view(B, Nk, Hkv, dh).transpose(1, 2)
    vh = v.view(B, Nk, Hkv, dh).transpose(1, 2)
    if rot:
        cos, sin = (t.cpu() for t in tabs)
        qh = _rotate(qh, cos, sin, torch.arange(Nq) + off, rot)
        kh = _rotate(kh, cos, sin, torch.arange(Nk), rot)
    kh = kh.repeat_interleave(H // Hkv, 1)
    vh = vh.repeat_interleave(H // Hkv, 1)
    dots = qh @ kh.transpose(-1, -2) * dh ** -0.5
    if mask is not None:
        dots = dots.masked_fill(~mask.cpu()[:, None, None, :], -torch.finfo(dots.dtype).max)
    if causal:
        allowed = torch.arange(Nk)[None, :] <= torch.arange(Nq)[:, None] + off
        dots = dots.masked_fill(~allowed, -math.inf)
    lse = torch.logsumexp(dots, -1)
    o = dots.softmax(-1) @ vh
    return o.transpose(1, 2).reshape(B, Nq, H * dh), lse


# (Nq, Nk, H, Hkv, rot, mask, causal, layout): layout "fused" = one [B, N, ld] buffer holding q | k | v (Nq == Nk),
# "split" = q and k | v in two padded buffers (column offsets != 0)
def _cases(dh):
    r = DIT_ROT[dh]
    return [(37, 37, 2, 2, r, False, False, "fused"), (126, 126, 3, 3, r, True, False, "fused"),
            (128, 128, 2, 2, 0, True, False, "fused"), (130, 130, 2, 2, r, False, False, "fused"),
            (200, 200, 4, 2, r, True, False, "fused"), (300, 300, 2, 2, r, True, True, "fused"),
            (126, 126, 2, 2, 32, False, True, "fused"),
            (126, 130, 4, 1, 0, True, False, "split"), (126, 130, 4, 4, 0, False, False, "split"),
            (37, 200, 4, 2, r, True, True, "split"), (128, 300, 2, 1, 0, True, False, "split"),
            (1, 1, 2, 2, r, False, False, "split"), (1, 37, 4, 1, 0, True, False, "split"),
            (1, 300, 4, 2, r, True, True, "split"), (1, 126, 2, 2, 0, False, False, "split"),
            (126, 7, 4, 4, 0, True, False, "split"), (300, 130, 4, 2, 0, False, False, "split")]


def _run_case(ops, dev, dh, Nq, Nk, H, Hkv, rot, use_mask, causal, layout, seed):
    B = 2
    if layout == "fused":
        assert Nq == Nk
        ld = (H + 2 * Hkv) * dh + 8
        buf = (_mk((B, Nq, ld), seed) * 0.8).bfloat16()
        qo, ko_, vo = 0, H * dh, (H + Hkv) * dh
        qb = kb = buf
        ldq = ldk = ld
        q = buf[..., qo:qo + H * dh]
        k, v = buf[..., ko_:ko_ + Hkv * dh], buf[..., vo:vo + Hkv * dh]
    else:
        ldq, ldk = H * dh + 16, 2 * Hkv * dh + 24
        qb = (_mk((B, Nq, ldq), seed) * 0.8).bfloat16()
        kb = (_mk((B, Nk, ldk), seed + 1) * 0.8).bfloat16()
        qo, ko_, vo = 8, 16, 16 + Hkv * dh
        q = qb[..., qo:qo + H * dh]
        k, v = kb[..., ko_:ko_ + Hkv * dh], kb[..., vo:vo + Hkv * dh]
    dout = _mk((B, Nq, H * dh), seed + 2).bfloat16()
    mask = None
    if use_mask:
        mask = torch.rand(B, Nk, generator=torch.Generator().manual_seed(seed + 3)) > 0.3
        mask[0, 0] = True
        if not causal:
            # a fully masked batch row: uniform weights over all keys in the forward, as the reference's masked_fill(-max)
            # and the head-dim-64 kernel give (its backward, like the head-dim-64 one, treats every key as masked: checked on
            # batch element 0 only)
            mask[1, :] = False
    tabs = _tables(max(Nq, Nk), rot, dev) if rot else None

    qr = q.double().requires_grad_(True)
    kr = k.double().requires_grad_(True)
    vr = v.double().requires_grad_(True)
    ref, lse_ref = _ref(qr, kr, vr, H, Hkv, dh, rot, tabs, mask, causal)
    ref.backward(dout.double())

    d = lambda t: t.to(dev)  # noqa: E731
    qb_d, kb_d = d(qb), d(kb)
    m_d = d(mask) if mask is not None else None
    out, lse = ops.attention_fwd(qb_d, kb_d, kb_d, ldq=ldq, q_off=qo, ldk=ldk, k_off=ko_, ldv=ldk, v_off=vo, B=B, H=H,
                                 Hkv=Hkv, Nq=Nq, Nk=Nk, rope=tabs, key_mask=m_d, causal=causal, dh=dh)
    torch.cuda.synchronize()
    e = rel_l2(out, ref)
    assert e < 1e-2, ("out", e)
    live = torch.ones(B, dtype=torch.bool) if mask is None else mask.any(-1)     # (a fully masked row's lse is not the fp64 one)
    lr = lse_ref[live]
    assert (lse.cpu().double()[live] - lr).abs().max().item() < 1e-2 * (1 + lr.abs().max().item())
    if Nq == 1:
        return                                # (the backward of a decoding step is not a training shape)
    dqb = torch.zeros_like(qb_d)
    dkb = torch.zeros_like(kb_d)
    dkb = dqb if layout == "fused" else dkb
    ops.attention_bwd(qb_d, kb_d, kb_d, out, d(dout), lse, dqb, dkb, dkb, ldq=ldq, q_off=qo, ldk=ldk, k_off=ko_, ldv=ldk,
                      v_off=vo, B=B, H=H, Hkv=Hkv, Nq=Nq, Nk=Nk, rope=tabs, key_mask=m_d, causal=causal, dh=dh)
    torch.cuda.synchronize()
    if layout == "fused":
        dq, dk, dv = dqb[..., qo:qo + H * dh], dqb[..., ko_:ko_ + Hkv * dh], dqb[..., vo:vo + Hkv * dh]
    else:
        dq, dk, dv = dqb[..., qo:qo + H * dh], dkb[..., ko_:ko_ + Hkv * dh], dkb[..., vo:vo + Hkv * dh]
        # columns outside the heads are never written
        assert dqb[..., :qo].abs().max().item() == 0 and dkb[..., :ko_].abs().max().item() == 0
    bs = slice(0, 1) if (mask is not None and not mask[1].any()) else slice(0, B)
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        e = rel_l2(got[bs], want[bs])
        assert e < 2e-2, (name, e)


@pytest.mark.parametrize("dh", [32, 64, 128])        # (64: the same product through the original kernels, a control)
@pytest.mark.parametrize("case", range(17))
def test_attention_hd_kernels_vs_fp64(ops, dev, dh, case):
    Nq, Nk, H, Hkv, rot, use_mask, causal, layout = _cases(dh)[case]
    _run_case(ops, dev, dh, Nq, Nk, H, Hkv, rot, use_mask, causal, layout, seed=1000 + 31 * case + dh)


def test_attention_hd_rejects_bad_arguments(ops, dev):
    from kalle_audio_amd import _lib
    lib = _lib.load()
    x = torch.zeros((1, 4, 3 * 128), device=dev, dtype=torch.bfloat16)
    lse = torch.zeros((1, 1, 4), device=dev)
    cos = torch.zeros((4, 32), device=dev)
    P = ops._p
    for dh, rot in ((48, 0), (256, 0), (0, 0), (32, 64), (128, 16)):
        r = lib.kalle_attention_fwd_hd(P(x), 3 * 128, 0, P(x), 3 * 128, 128, P(x), 3 * 128, 256, P(x), 128, P(lse),
                                       P(cos), P(cos), rot, None, 0, 1, 1, 1, 4, 4, dh, ops._stream())
        assert r != 0, (dh, rot)


# ------------------------------------------------------------------------------------------------ head dim 64 bit for bit
@pytest.mark.parametrize("Nq,Nk,H,Hkv,rot,causal", [(126, 126, 4, 4, 32, False), (126, 130, 4, 2, 0, False),
                                                   (300, 300, 2, 2, 64, True), (1, 200, 4, 1, 64, True)])
def test_hd64_entry_points_bit_identical(ops, dev, Nq, Nk, H, Hkv, rot, causal):
    from kalle_audio_amd import _lib
    lib = _lib.load()
    P, st = ops._p, ops._stream()
    B, dh = 2, 64
    q = (_mk((B, Nq, H * dh), 5) * 0.8).bfloat16().to(dev)
    kv = (_mk((B, Nk, 2 * Hkv * dh), 6) * 0.8).bfloat16().to(dev)
    dout = _mk((B, Nq, H * dh), 7).bfloat16().to(dev)
    mask = (torch.rand(B, Nk, generator=torch.Generator().manual_seed(8)) > 0.2).to(dev)
    mask[:, -1] = True
    m8 = mask.to(torch.uint8).contiguous()
    cos, sin = _tables(Nk, rot, dev) if rot else (None, None)
    outs = []
    for hd in (False, True):
        out = torch.empty((B, Nq, H * dh), device=dev, dtype=torch.bfloat16)
        lse = torch.empty((B, H, Nq), device=dev)
        a = (P(q), H * dh, 0, P(kv), 2 * Hkv * dh, 0, P(kv), 2 * Hkv * dh, Hkv * dh, P(out), H * dh, P(lse), P(cos), P(sin), rot,
             P(m8), int(causal), B, H, Hkv, Nq, Nk)
        assert (lib.kalle_attention_fwd_hd(*a, 64, st) if hd else lib.kalle_attention_fwd(*a, st)) == 0
        res = [out, lse]
        if Nq > 1:
            delta = torch.empty((B, H, Nq), device=dev)
            dq, dkv = torch.zeros_like(q), torch.zeros_like(kv)
            a = (P(q), H * dh, 0, P(kv), 2 * Hkv * dh, 0, P(kv), 2 * Hkv * dh, Hkv * dh, P(out), P(dout), H * dh, P(lse),
                 P(delta), P(dq), P(dkv), P(dkv), P(cos), P(sin), rot, P(m8), int(causal), B, H, Hkv, Nq, Nk)
            assert (lib.kalle_attention_bwd_hd(*a, 64, st) if hd else lib.kalle_attention_bwd(*a, st)) == 0
            res += [dq, dkv]
        torch.cuda.synchronize()
        outs.append(res)
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    # the head norms
    rows, heads = 300, 5
    x = (_mk((rows, 3 * heads * dh), 9)).bfloat16().to(dev)
    gam = (1 + 0.2 * _mk((dh,), 10)).to(dev)
    bet = (0.1 * _mk((dh,), 11)).to(dev)
    g = _mk((rows, heads * dh), 12).bfloat16().to(dev)
    for mode in (1, 2):
        res = []
        for hd in (False, True):
            y = torch.empty((rows, heads * dh), device=dev, dtype=torch.bfloat16)
            stat = torch.empty((rows, heads, 2), device=dev)
            dx = torch.zeros_like(x)
            dga, dbe = torch.zeros(dh, device=dev), torch.zeros(dh, device=dev)
            a = (P(x), 3 * heads * dh, heads * dh, P(y), heads * dh, 0, P(stat), P(gam), P(bet), mode, rows, heads)
            assert (lib.kalle_head_norm_fwd_hd(*a, 64, st) if hd else lib.kalle_head_norm_fwd(*a, st)) == 0
            a = (P(x), 3 * heads * dh, heads * dh, P(stat), P(g), heads * dh, 0, P(dx), 3 * heads * dh, heads * dh, P(gam),
                 P(dga), P(dbe), mode, rows, heads)
            assert (lib.kalle_head_norm_bwd_hd(*a, 64, st) if hd else lib.kalle_head_norm_bwd(*a, st)) == 0
            torch.cuda.synchronize()
            res.append((y, stat, dx, dga, dbe))
        for a_, b_ in zip(*res):
            assert torch.equal(a_, b_) or (mode == 2 and a_.dtype == torch.float32 and a_.dim() == 1 and
                                           torch.allclose(a_, b_, rtol=1e-5, atol=1e-5))   # (atomic column sums)


# ------------------------------------------------------------------------------------------------ head norm
@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("mode", [1, 2])
def test_head_norm_hd(ops, dev, dh, mode):
    rows, heads = 257, 3
    ld = 3 * heads * dh
    x = (_mk((rows, ld), 20 + dh) * 1.3 + 0.2).bfloat16()
    g = _mk((rows, heads * dh), 21 + dh).bfloat16()
    gam = (1 + 0.2 * _mk((dh,), 22)).requires_grad_(True)
    bet = (0.1 * _mk((dh,), 23)).requires_grad_(True)
    xs = x[:, heads * dh:2 * heads * dh].double().requires_grad_(True)
    xh = xs.view(rows, heads, dh)
    if mode == 1:
        ref = xh / xh.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    else:
        ref = torch.nn.functional.layer_norm(xh, (dh,), gam.double(), bet.double(), 1e-6)
    ref.reshape(rows, heads * dh).backward(g.double())
    xd = x.to(dev)
    gm_d = gam.detach().to(dev) if mode == 2 else None
    bt_d = bet.detach().to(dev) if mode == 2 else None
    y, stat = ops.head_norm_fwd(xd, ld, heads * dh, rows, heads, mode, gm_d, bt_d, dh=dh)
    assert rel_l2(y, ref.reshape(rows, heads * dh)) < 5e-3
    dx = torch.zeros_like(xd)
    dga = torch.zeros(dh, device=dev) if mode == 2 else None
    dbe = torch.zeros(dh, device=dev) if mode == 2 else None
    ops.head_norm_bwd(xd, ld, heads * dh, stat, g.to(dev), dx, ld, heads * dh, rows, heads, mode, gm_d, dga, dbe, dh=dh)
    torch.cuda.synchronize()
    assert rel_l2(dx[:, heads * dh:2 * heads * dh], xs.grad) < 1e-2
    assert dx[:, :heads * dh].abs().max().item() == 0 and dx[:, 2 * heads * dh:].abs().max().item() == 0
    if mode == 2:
        gsum = (g.double().view(rows, heads, dh))
        xhat = (ref.detach() - bet.double()) / gam.double()
        assert rel_l2(dga, (gsum * xhat).sum((0, 1))) < 1e-2
        assert rel_l2(dbe, gsum.sum((0, 1))) < 1e-2


# ------------------------------------------------------------------------------------------------ modules vs the CPU oracle
B, N, S = 2, 125, 9


def _seeded(module, seed, dev):
    st = gu.make_state([(n, tuple(p.shape)) for n, p in module.named_parameters()], seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            p.copy_(torch.from_numpy(st[n]))
    sd = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in st.items()}
    return module.to(dev), sd


@pytest.fixture(scope="module")
def mods(dev):
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models import transformer as T_
    return T_


def _check_grads(module, sd, tol=2e-2):
    # (k_norm.bias adds the same vector to every key of a head: the scores of a query shift by a constant, so its exact
    # gradient is zero and only the rounding noise of either side remains - compared against the weight's scale instead)
    for n, p in module.named_parameters():
        if sd[n].grad is None:
            continue
        if n.endswith("k_norm.bias"):
            assert p.grad.norm().item() < tol * sd[n[:-4] + "weight"].grad.norm().item(), n
            continue
        e = rel_l2(p.grad, sd[n].grad)
        assert e < tol, (n, e)


@pytest.mark.parametrize("dh", [32, 128])
def test_attention_module_hd(mods, dev, dh):
    D, DC = 256, 128                     # cross: H = 256 / dh query heads over 128 / dh kv heads (GQA)
    seed = 300 + dh
    x = torch.from_numpy(gu.make_input("x", (B, N, D), seed))
    dy = torch.from_numpy(gu.make_input("dy", (B, N, D), seed))
    mask = torch.from_numpy(gu.make_mask("m", (B, N), seed))
    at, sd = _seeded(mods.Attention(D, dim_heads=dh), seed, dev)
    rot = mods.RotaryEmbedding(max(dh // 2, 32)).to(dev)
    xr = x.clone().requires_grad_(True)
    ref = ko.attention(sd, xr, mask=mask, rotary=ko.rotary_freqs(N, DIT_ROT[dh]), dim_heads=dh)
    ref.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    y = at(xg, mask=mask.to(dev), rotary_pos_emb=rot.forward_from_seq_len(N))
    y.backward(dy.to(dev))
    assert rel_l2(y, ref) < 1e-2
    assert rel_l2(xg.grad, xr.grad) < 2e-2
    _check_grads(at, sd)

    ctx = torch.from_numpy(gu.make_input("ctx", (B, S, DC), seed))
    cm = torch.from_numpy(gu.make_mask("cm", (B, S), seed))
    at, sd = _seeded(mods.Attention(D, dim_heads=dh, dim_context=DC, qk_norm="ln"), seed + 1, dev)
    assert tuple(at.q_norm.weight.shape) == (dh,)
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    ref = ko.attention(sd, xr, context=cr, context_mask=cm, dim_heads=dh)
    ref.backward(dy)
    xg, cg = x.to(dev).requires_grad_(True), ctx.to(dev).requires_grad_(True)
    y = at(xg, context=cg, context_mask=cm.to(dev))
    y.backward(dy.to(dev))
    assert rel_l2(y, ref) < 1e-2
    assert rel_l2(xg.grad, xr.grad) < 2e-2
    assert rel_l2(cg.grad, cr.grad) < 2e-2
    _check_grads(at, sd)


@pytest.mark.parametrize("dh", [32, 128])
def test_transformer_block_hd(mods, dev, dh):
    D, DC, GD = 256, 128, 64
    seed = 400 + dh
    blk, sd = _seeded(mods.TransformerBlock(D, dim_heads=dh, cross_attend=True, dim_context=DC, global_cond_dim=GD,
                                            attn_kwargs={"qk_norm": "l2"}), seed, dev)
    x = torch.from_numpy(gu.make_input("x", (B, N, D), seed))
    ctx = torch.from_numpy(gu.make_input("ctx", (B, S, DC), seed))
    gl = torch.from_numpy(gu.make_input("g", (B, GD), seed))
    dy = torch.from_numpy(gu.make_input("dy", (B, N, D), seed))
    xr, cr, gr = (t.clone().requires_grad_(True) for t in (x, ctx, gl))
    freqs = ko.rotary_freqs(N, DIT_ROT[dh])
    ref = ko.transformer_block(sd, xr, context=cr, global_cond=gr, rotary=freqs, dim_heads=dh, qk_l2=True)
    ref.backward(dy)
    rot = mods.RotaryEmbedding(max(dh // 2, 32)).to(dev)
    xg, cg, gg = (t.to(dev).requires_grad_(True) for t in (x, ctx, gl))
    y = blk(xg, context=cg, global_cond=gg, rotary_pos_emb=rot.forward_from_seq_len(N))
    y.backward(dy.to(dev))
    assert rel_l2(y, ref) < 1e-2
    for got, want in ((xg.grad, xr.grad), (cg.grad, cr.grad), (gg.grad, gr.grad)):
        assert rel_l2(got, want) < 2e-2
    _check_grads(blk, sd)


def _dit_kw(D, dh, DC, GD, C):
    return dict(io_channels=C, embed_dim=D, depth=2, num_heads=D // dh, cond_token_dim=DC, project_cond_tokens=False,
                global_cond_dim=GD, transformer_type="continuous_transformer", global_cond_type="prepend")


@pytest.mark.parametrize("dh", [128, 32])
def test_dit_train_step_hd(mods, dev, dh):
    """one DataParallelTrainer step of a 2-layer DiT at num_heads = D // dh against the CPU oracle: loss and gradients"""
    from kalle_audio_amd import engine
    from kalle_audio_amd.stable_audio_tools.models.diffusion import ConditionedDiffusionModelWrapper, DiTWrapper
    D, DC, GD, C, T_ = 256, 128, 32, 16, 125
    seed = 500 + dh
    dit = DiTWrapper(**_dit_kw(D, dh, DC, GD, C))
    shapes = ko.dit_shapes(C, D, 2, cond_token_dim=DC, global_cond_dim=GD, project_cond_tokens=False)
    st = gu.make_state(shapes, seed)
    with torch.no_grad():
        for n, p in dit.model.named_parameters():
            p.copy_(torch.from_numpy(st[n]))
    dit.to(dev)
    model = ConditionedDiffusionModelWrapper(dit, None, io_channels=C, sample_rate=16000, min_input_length=1,
                                             cross_attn_cond_ids=["prompt"], global_cond_ids=["g"])
    lat = torch.from_numpy(gu.make_input("lat", (B, C, T_), seed))
    noise = torch.from_numpy(gu.make_input("noise", (B, C, T_), seed))
    t = torch.tensor([0.25, 0.7])
    ctx = torch.from_numpy(gu.make_input("ctx", (B, S, DC), seed))
    cm = torch.from_numpy(gu.make_mask("cm", (B, S), seed))
    gl = torch.from_numpy(gu.make_input("gl", (B, GD), seed))
    sd = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in st.items()}
    loss_ref, *_ = ko.train_step_loss(sd, dict(embed_dim=D, depth=2, num_heads=D // dh, global_cond_type="prepend"), lat,
                                      noise, t, "v", cross_attn_cond=ctx, cross_attn_cond_mask=cm, global_embed=gl)
    loss_ref.backward()
    tr = engine.DataParallelTrainer(model, lr=1e-3, optimizer="Adam")
    cond = {"prompt": (ctx.to(dev), cm.to(dev)), "g": (gl.to(dev), None)}
    loss = tr.train_step(model, lat.to(dev), t.to(dev), noise.to(dev), cond, objective="v")
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_ref.item()) <= 1e-2 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    n = 0
    for name in sd:
        if sd[name].grad is None or sd[name].grad.norm() == 0:
            continue
        e = rel_l2(tr.flat.grad_view("model.model." + name).float(), sd[name].grad)
        assert e < 3e-2, (name, e)
        n += 1
    assert n > 20


@pytest.mark.parametrize("dh", [32, 128])
def test_generate_graph_replay_hd(mods, dev, dh):
    """generate_diffusion_cond at num_heads = D // dh: HIP-graph replay of a frozen model gives the eager launches' bits"""
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from kalle_audio_amd.stable_audio_tools.models.diffusion import ConditionedDiffusionModelWrapper, DiTWrapper
    D, DC, GD, C = 256, 128, 32, 8
    seed = 600 + dh
    dit = DiTWrapper(**_dit_kw(D, dh, DC, GD, C))
    _seeded(dit.model, seed, dev)
    model = ConditionedDiffusionModelWrapper(dit, None, io_channels=C, sample_rate=16000, min_input_length=1,
                                             diffusion_objective="rectified_flow", cross_attn_cond_ids=["prompt"],
                                             global_cond_ids=["g"]).to(dev)
    ctx = torch.from_numpy(gu.make_input("ctx", (2, S, DC), seed)).to(dev)
    cm = torch.ones(2, S, dtype=torch.bool, device=dev)
    gl = torch.from_numpy(gu.make_input("gl", (2, GD), seed)).to(dev)
    kw = dict(steps=4, cfg_scale=3.0, conditioning_tensors={"prompt": (ctx, cm), "g": (gl, None)}, batch_size=2,
              sample_size=100, seed=4242, device="cpu", return_latents=True)
    lat = generate_diffusion_cond(model, **kw)                       # eager (parameters still require grad)
    assert torch.isfinite(lat).all()
    model.requires_grad_(False)
    for _ in range(2):
        lat_g = generate_diffusion_cond(model, **kw)
        assert getattr(model, "_kalle_graphed", None) is not None
        assert torch.equal(lat_g, lat)
