"""Head dims 32 and 128 without a GPU: the CPU oracle against the reference's fixture (tests/golden/head_dims.npz, written by
make_golden_head_dims.py), the drop-in modules' construction rules and state-dict layout, and the C ABI's _hd entry points."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import golden_util as gu  # noqa: E402
import kalle_oracle as ko  # noqa: E402

B, N, D, S, DC, G, C = 2, 40, 256, 7, 128, 32, 16       # (make_golden_head_dims.py)


def case_seed(dh, k):
    return 700 + 10 * k + dh


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "head_dims.npz"))


@pytest.fixture(scope="module")
def T_():
    from kalle_audio_amd.stable_audio_tools.models import transformer
    return transformer


def _state(module, seed):
    """the seeded parameters make_golden's load_seeded gives the reference module of the same layout"""
    st = gu.make_state([(n, tuple(p.shape)) for n, p in module.named_parameters()], seed)
    return {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in st.items()}


def _inp(name, shape, seed, grad=True):
    t = torch.from_numpy(gu.make_input(name, shape, seed))
    return t.requires_grad_(True) if grad else t


def _same(got, ref, tol=2e-5):
    got = gu.digest(got.detach().numpy())
    scale = max(abs(ref[0]), 1e-12)
    assert np.all(np.abs(got - ref) <= tol * scale + 1e-7), (got[:3], ref[:3])


def _check(fx, prefix, sd, **arrs):
    for k, v in arrs.items():
        _same(v, fx[f"{prefix}/{k}"])
    keys = [k for k in fx.files if k.startswith(prefix + "/digest/")]
    assert keys
    # a gradient that is zero in exact arithmetic (the cross-attention k_norm.bias: softmax ignores a shift shared by a row's
    # logits) is fp32 rounding noise on both sides, ~1e-7 of the case's typical gradient norm, and that noise changes with
    # the thread count: such a gradient must be as small on this side too, its samples are not compared
    zero = 1e-6 * float(np.median([fx[k][0] for k in keys]))
    for k in keys:
        g = sd[k[len(prefix) + 8:]].grad
        if fx[k][0] < zero:
            assert gu.digest(g.detach().numpy())[0] < zero, (k, gu.digest(g.detach().numpy())[0], zero)
        else:
            _same(g, fx[k])


@pytest.mark.parametrize("dh", [32, 128])
def test_oracle_matches_reference_at_head_dim(fx, T_, dh):
    rot = ko.rotary_freqs(N, max(dh // 2, 32))
    dy = _inp("dy", (B, N, D), case_seed(dh, 0), False)
    s = case_seed(dh, 1)
    x = _inp("x", (B, N, D), s)
    mask = torch.from_numpy(gu.make_mask("m", (B, N), s))
    sd = _state(T_.Attention(D, dim_heads=dh), s)
    y = ko.attention(sd, x, mask=mask, rotary=rot, dim_heads=dh)
    y.backward(dy)
    _check(fx, f"dh{dh}/attn_self", sd, y=y, dx=x.grad)

    s = case_seed(dh, 2)
    x, ctx = _inp("x", (B, N, D), s), _inp("ctx", (B, S, DC), s)
    cm = torch.from_numpy(gu.make_mask("cm", (B, S), s))
    sd = _state(T_.Attention(D, dim_heads=dh, dim_context=DC, qk_norm="ln"), s)
    y = ko.attention(sd, x, context=ctx, context_mask=cm, dim_heads=dh)
    y.backward(dy)
    _check(fx, f"dh{dh}/attn_cross", sd, y=y, dx=x.grad, dctx=ctx.grad)

    s = case_seed(dh, 3)
    x, ctx, gl = _inp("x", (B, N, D), s), _inp("ctx", (B, S, DC), s), _inp("g", (B, G), s)
    sd = _state(T_.TransformerBlock(D, dim_heads=dh, cross_attend=True, dim_context=DC, global_cond_dim=G,
                                    attn_kwargs={"qk_norm": "l2"}), s)
    y = ko.transformer_block(sd, x, context=ctx, global_cond=gl, rotary=rot, dim_heads=dh, qk_l2=True)
    y.backward(dy)
    _check(fx, f"dh{dh}/block", sd, y=y, dx=x.grad, dctx=ctx.grad, dglobal=gl.grad)

    from kalle_audio_amd.stable_audio_tools.models.dit import DiffusionTransformer
    s = case_seed(dh, 4)
    dit = DiffusionTransformer(io_channels=C, embed_dim=D, depth=2, num_heads=D // dh, cond_token_dim=DC,
                               project_cond_tokens=False, global_cond_dim=G, transformer_type="continuous_transformer")
    sd = _state(dit, s)
    xd, ctx, gl = _inp("x", (B, C, N), s), _inp("ctx", (B, S, DC), s), _inp("g", (B, G), s)
    t = torch.tensor([0.3, 0.8])
    y = ko.dit_forward(sd, dict(embed_dim=D, depth=2, num_heads=D // dh, global_cond_type="prepend"), xd, t,
                       cross_attn_cond=ctx, global_embed=gl)
    y.backward(_inp("dy", (B, C, N), s, False))
    _check(fx, f"dh{dh}/dit", sd, y=y, dx=xd.grad, dctx=ctx.grad, dglobal=gl.grad)


@pytest.mark.parametrize("dh", [32, 128])
def test_modules_construct_at_head_dim(T_, dh):
    at = T_.Attention(D, dim_heads=dh, dim_context=DC, qk_norm="ln")
    assert (at.num_heads, at.kv_heads) == (D // dh, DC // dh)
    shapes = {n: tuple(p.shape) for n, p in at.state_dict().items()}
    assert shapes == {"to_q.weight": (D, D), "to_kv.weight": (2 * DC, DC), "to_out.weight": (D, D),
                      "q_norm.weight": (dh,), "q_norm.bias": (dh,), "k_norm.weight": (dh,), "k_norm.bias": (dh,)}
    blk = T_.TransformerBlock(D, dim_heads=dh, cross_attend=True, dim_context=DC, global_cond_dim=G,
                              attn_kwargs={"qk_norm": "ln"})
    assert tuple(blk.self_attn.q_norm.weight.shape) == (dh,) and tuple(blk.cross_attn.k_norm.bias.shape) == (dh,)
    from kalle_audio_amd.stable_audio_tools.models.dit import DiffusionTransformer
    dit = DiffusionTransformer(io_channels=C, embed_dim=D, depth=2, num_heads=D // dh, cond_token_dim=DC,
                               project_cond_tokens=False, global_cond_dim=G, transformer_type="continuous_transformer")
    want = dict(ko.dit_shapes(C, D, 2, cond_token_dim=DC, global_cond_dim=G, project_cond_tokens=False))
    assert {n: tuple(p.shape) for n, p in dit.named_parameters()} == {k: tuple(v) for k, v in want.items()}
    assert dit.transformer.layers[0].self_attn.dim_heads == dh
    # the rotary width the reference derives from the head dim (transformer.py:730)
    assert dit.transformer.rotary_pos_emb.inv_freq.numel() * 2 == max(dh // 2, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        at(torch.zeros(1, 3, D), context=torch.zeros(1, 2, DC))
    with pytest.raises(RuntimeError, match="GPU only"):
        blk(torch.zeros(1, 3, D), context=torch.zeros(1, 2, DC), global_cond=torch.zeros(1, G))


@pytest.mark.parametrize("dh", [48, 256, 16, 96])
def test_unsupported_head_dims_raise(T_, dh):
    with pytest.raises(NotImplementedError, match=r"\(32, 64, 128\)"):
        T_.Attention(dh * 4, dim_heads=dh)


def test_shapes_the_kernels_cannot_run_raise_at_construction(T_):
    with pytest.raises(ValueError, match="multiples of dim_heads"):
        T_.Attention(200, dim_heads=32)
    with pytest.raises(ValueError, match="multiples of dim_heads"):
        T_.Attention(256, dim_heads=128, dim_context=96)
    with pytest.raises(ValueError, match="kv heads"):
        T_.Attention(384, dim_heads=128, dim_context=256)        # 3 query heads over 2 kv heads
    T_.Attention(384, dim_heads=128, dim_context=128)            # 3 over 1


def test_header_declares_hd_entry_points():
    from kalle_audio_amd import _lib
    protos = _lib.parse_header()
    for name, old in (("kalle_attention_fwd_hd", "kalle_attention_fwd"), ("kalle_attention_bwd_hd", "kalle_attention_bwd"),
                      ("kalle_head_norm_fwd_hd", "kalle_head_norm_fwd"), ("kalle_head_norm_bwd_hd", "kalle_head_norm_bwd")):
        assert name in protos, name
        # the existing arguments, then `int head_dim` just before the stream
        assert protos[name][1] == protos[old][1][:-1] + [protos[name][1][-2], protos[old][1][-1]]
        assert protos[name][1][-2].__name__ == "c_int"
