"""Head-dim golden fixture: the REFERENCE implementation (imported in place, CPU fp32) at dim_heads 32 and 128
(DiffusionTransformer(embed_dim, num_heads) passes dim_heads = embed_dim // num_heads, dit.py:118; ContinuousTransformer
sizes its rotary as RotaryEmbedding(max(dim_heads // 2, 32)), transformer.py:730).  For each head dim:

  * Attention, self-attention with rotary and a key mask;
  * Attention, cross-attention with dim_context != dim (kv heads < heads), a context mask and qk_norm="ln";
  * TransformerBlock with cross-attention, adaLN global conditioning and qk_norm="l2";
  * a 2-layer DiffusionTransformer(transformer_type="continuous_transformer", num_heads=D // dh).

Outputs and input gradients are kept as digests (golden_util.digest), parameter gradients as digests too, so that the file
stays small.  Runs only in the build container.  Writes data only.  Usage: python tests/golden/make_golden_head_dims.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_util as gu  # noqa: E402
import make_golden as mg  # noqa: E402
from make_golden import T, grads, load_seeded  # noqa: E402

B, N, D, S, DC, G, C = 2, 40, 256, 7, 128, 32, 16


def case_seed(dh, k):
    return 700 + 10 * k + dh


def main():
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from stable_audio_tools.models import transformer as rt
    from stable_audio_tools.models.dit import DiffusionTransformer

    out = {}

    def put(prefix, **arrs):
        for k, v in arrs.items():
            out[f"{prefix}/{k}"] = gu.digest(v.detach().numpy())

    def put_grads(prefix, module):
        for n, a in grads(module).items():
            out[f"{prefix}/digest/{n}"] = gu.digest(a)

    for dh in (32, 128):
        rot = rt.RotaryEmbedding(max(dh // 2, 32))
        dy = T(gu.make_input("dy", (B, N, D), case_seed(dh, 0)))
        # self-attention, rotary + key mask
        s = case_seed(dh, 1)
        x = T(gu.make_input("x", (B, N, D), s)).requires_grad_(True)
        mask = T(gu.make_mask("m", (B, N), s))
        at = load_seeded(rt.Attention(D, dim_heads=dh), s)
        y = at(x, mask=mask, rotary_pos_emb=rot.forward_from_seq_len(N))
        y.backward(dy)
        put(f"dh{dh}/attn_self", y=y, dx=x.grad)
        put_grads(f"dh{dh}/attn_self", at)
        # cross-attention, GQA + context mask + qk_norm "ln"
        s = case_seed(dh, 2)
        x = T(gu.make_input("x", (B, N, D), s)).requires_grad_(True)
        ctx = T(gu.make_input("ctx", (B, S, DC), s)).requires_grad_(True)
        cm = T(gu.make_mask("cm", (B, S), s))
        at = load_seeded(rt.Attention(D, dim_heads=dh, dim_context=DC, qk_norm="ln"), s)
        y = at(x, context=ctx, context_mask=cm)
        y.backward(dy)
        put(f"dh{dh}/attn_cross", y=y, dx=x.grad, dctx=ctx.grad)
        put_grads(f"dh{dh}/attn_cross", at)
        # TransformerBlock: cross-attention, adaLN, qk_norm "l2"
        s = case_seed(dh, 3)
        x = T(gu.make_input("x", (B, N, D), s)).requires_grad_(True)
        ctx = T(gu.make_input("ctx", (B, S, DC), s)).requires_grad_(True)
        gl = T(gu.make_input("g", (B, G), s)).requires_grad_(True)
        blk = load_seeded(rt.TransformerBlock(D, dim_heads=dh, cross_attend=True, dim_context=DC, global_cond_dim=G,
                                              attn_kwargs={"qk_norm": "l2"}), s)
        y = blk(x, context=ctx, global_cond=gl, rotary_pos_emb=rot.forward_from_seq_len(N))
        y.backward(dy)
        put(f"dh{dh}/block", y=y, dx=x.grad, dctx=ctx.grad, dglobal=gl.grad)
        put_grads(f"dh{dh}/block", blk)
        # 2-layer DiT at num_heads = D // dh
        s = case_seed(dh, 4)
        dit = load_seeded(DiffusionTransformer(io_channels=C, embed_dim=D, depth=2, num_heads=D // dh, cond_token_dim=DC,
                                               project_cond_tokens=False, global_cond_dim=G,
                                               transformer_type="continuous_transformer"), s)
        xd = T(gu.make_input("x", (B, C, N), s)).requires_grad_(True)
        t = T(np.array([0.3, 0.8], dtype=np.float32))
        ctx = T(gu.make_input("ctx", (B, S, DC), s)).requires_grad_(True)
        gl = T(gu.make_input("g", (B, G), s)).requires_grad_(True)
        y = dit(xd, t, cross_attn_cond=ctx, global_embed=gl, cfg_dropout_prob=0.0)
        y.backward(T(gu.make_input("dy", (B, C, N), s)))
        put(f"dh{dh}/dit", y=y, dx=xd.grad, dctx=ctx.grad, dglobal=gl.grad)
        put_grads(f"dh{dh}/dit", dit)

    path = os.path.join(HERE, "head_dims.npz")
    np.savez_compressed(path, **out)
    print(f"head_dims: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB", flush=True)


if __name__ == "__main__":
    main()
