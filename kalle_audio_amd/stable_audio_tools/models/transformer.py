"""Drop-in for stable_audio_tools/models/transformer.py (reference file:line cited per class): same class names,
constructor kwargs, forward signatures and state-dict keys; every forward runs the hand-written gfx950 kernels
(kalle_audio_amd/csrc) through autograd shims.  GPU tensors only - there is no CPU or torch-math fallback.

Off-default options carried over in round 3 (none is reachable from the DiT path, dit.py:107-125, with the configs the
reference ships): ConformerModule (`conformer=True`), ScaledSinusoidalEmbedding / AbsolutePositionalEmbedding
(`use_sinusoidal_emb` / `use_abs_pos_emb`), `causal=True` (parity unpinned: the reference's own causal calls raise, see
Attention).  Not carried over (raise NotImplementedError when requested): natten neighbourhood attention, conv feed-forward,
remove_norms, use_xpos.
"""
import os

import torch
from torch import nn

from ... import functional as KF


def _need_gpu(x):
    if not x.is_cuda:
        raise RuntimeError("kalle_audio_amd modules run on an MI355X GPU only (hand-written HIP kernels, no CPU "
                           "fallback); move the module and its inputs to cuda")


class RotaryEmbedding(nn.Module):
    """transformer.py:89-144 (use_xpos=False path; `inv_freq` is a persistent buffer, line 106)."""

    def __init__(self, dim, use_xpos=False, scale_base=512, interpolation_factor=1., base=10000,
                 base_rescale_factor=1.):
        super().__init__()
        if use_xpos:
            raise NotImplementedError("use_xpos (unreachable in the reference: transformer.py:140 uses an undefined name)")
        base *= base_rescale_factor ** (dim / (dim - 2))
        self.register_buffer("inv_freq", 1. / (base ** (torch.arange(0, dim, 2).float() / dim)))
        assert interpolation_factor >= 1.
        self.interpolation_factor = interpolation_factor
        self.register_buffer("scale", None)

    def forward_from_seq_len(self, seq_len):
        return self.forward(torch.arange(seq_len, device=self.inv_freq.device))

    def forward(self, t):
        # position table set-up (N x rot/2 values), not data-path math
        t = t.to(torch.float32) / self.interpolation_factor
        freqs = t[:, None] * self.inv_freq[None, :].float()
        return torch.cat((freqs, freqs), dim=-1), 1.


class AbsolutePositionalEmbedding(nn.Module):
    """transformer.py:45-65: a learned table, scaled by dim^-0.5 (returns the [n, dim] table of positions 0..n-1; the add to the
    sequence is ContinuousTransformer's, 796-797)."""

    def __init__(self, dim, max_seq_len):
        super().__init__()
        self.scale = dim ** -0.5
        self.max_seq_len = max_seq_len
        self.emb = nn.Embedding(max_seq_len, dim)

    def forward(self, x, pos=None, seq_start_pos=None):
        seq_len = x.shape[1]
        assert seq_len <= self.max_seq_len, (f"you are passing in a sequence length of {seq_len} but your absolute positional "
                                             f"embedding has a max sequence length of {self.max_seq_len}")
        if pos is None:
            pos = torch.arange(seq_len, device=x.device)
        if seq_start_pos is not None:
            pos = (pos - seq_start_pos[..., None]).clamp(min=0)
        return self.emb(pos) * self.scale       # table set-up on [n, dim] (the data-path add is kalle_add_rows)


class ScaledSinusoidalEmbedding(nn.Module):
    """transformer.py:67-87: cat(sin, cos)(pos x theta^(-i / (dim / 2))) times a learned scalar."""

    def __init__(self, dim, theta=10000):
        super().__init__()
        assert (dim % 2) == 0, "dimension must be divisible by 2"
        self.scale = nn.Parameter(torch.ones(1) * dim ** -0.5)
        half_dim = dim // 2
        freq_seq = torch.arange(half_dim).float() / half_dim
        self.register_buffer("inv_freq", theta ** -freq_seq, persistent=False)

    def forward(self, x, pos=None, seq_start_pos=None):
        seq_len = x.shape[1]
        if pos is None:
            pos = torch.arange(seq_len, device=x.device)
        if seq_start_pos is not None:
            pos = pos - seq_start_pos[..., None]
        emb = pos.float()[..., None] * self.inv_freq.float()
        return torch.cat((emb.sin(), emb.cos()), dim=-1) * self.scale


class LayerNorm(nn.Module):
    """transformer.py:173-192: bias-less LayerNorm; gamma Parameter, beta zero buffer unless bias=True."""

    def __init__(self, dim, bias=False, fix_scale=False):
        super().__init__()
        if fix_scale:
            self.register_buffer("gamma", torch.ones(dim))
        else:
            self.gamma = nn.Parameter(torch.ones(dim))
        if bias:
            self.beta = nn.Parameter(torch.zeros(dim))
        else:
            self.register_buffer("beta", torch.zeros(dim))

    def forward(self, x):
        _need_gpu(x)
        beta = self.beta if isinstance(self.beta, nn.Parameter) else None
        return KF.LayerNormFn.apply(x, self.gamma, beta, 1e-5)


class GLU(nn.Module):
    """transformer.py:196-219 (parameter container; the fused FeedForward kernel path does the math)."""

    def __init__(self, dim_in, dim_out, activation, use_conv=False, conv_kernel_size=3):
        super().__init__()
        if use_conv:
            raise NotImplementedError("GLU(use_conv=True)")
        if not isinstance(activation, nn.SiLU):
            raise NotImplementedError("only the SwiGLU activation the reference uses (transformer.py:238)")
        self.act = activation
        self.proj = nn.Linear(dim_in, dim_out * 2)
        self.use_conv = use_conv


class FeedForward(nn.Module):
    """transformer.py:221-269: SwiGLU feed-forward, zero-initialised output projection (255-258)."""

    def __init__(self, dim, dim_out=None, mult=4, no_bias=False, glu=True, use_conv=False, conv_kernel_size=3,
                 zero_init_output=True):
        super().__init__()
        if not glu or use_conv:
            raise NotImplementedError("FeedForward(glu=False / use_conv=True)")
        inner_dim = int(dim * mult)
        dim_out = dim if dim_out is None else dim_out
        linear_in = GLU(dim, inner_dim, nn.SiLU())
        if no_bias:
            linear_in.proj = nn.Linear(dim, inner_dim * 2)  # the reference GLU always has a bias (207)
        linear_out = nn.Linear(inner_dim, dim_out, bias=not no_bias)
        if zero_init_output:
            nn.init.zeros_(linear_out.weight)
            if not no_bias:
                nn.init.zeros_(linear_out.bias)
        self.ff = nn.Sequential(linear_in, nn.Identity(), linear_out, nn.Identity())

    def forward(self, x):
        _need_gpu(x)
        l1, l2 = self.ff[0].proj, self.ff[2]
        return KF.FeedForwardFn.apply(self, x, l1.weight, l1.bias, l2.weight, l2.bias)


SUPPORTED_HEAD_DIMS = (32, 64, 128)     # dim_heads the attention and qk_norm kernels are built for


class Attention(nn.Module):
    """transformer.py:271-547.

    causal: the mask of create_causal_mask (transformer.py:32-33) - query r attends keys c <= r + (keys - queries), a single
    query attends everything (468-469) - applied inside the attention kernels (forward and both backward passes).  PARITY
    UNPINNED for this flag: the reference calls the function as `self.create_causal_mask` (362, 372, 521), a name Attention
    does not have, so its CPU branch raises AttributeError on every causal call and its GPU branch whenever a mask is given
    or keys outnumber queries; the only causal call it completes is SDPA's is_causal on equal lengths, which is this mask."""

    def __init__(self, dim, dim_heads=64, dim_context=None, causal=False, zero_init_output=True, qk_norm='none',
                 natten_kernel_size=None):
        super().__init__()
        if natten_kernel_size is not None:
            raise NotImplementedError("Attention(natten): not on the DiT path (dit.py:252)")
        if qk_norm not in ("none", "l2", "ln"):
            raise ValueError(f"unknown qk_norm {qk_norm!r}")
        if dim_heads not in SUPPORTED_HEAD_DIMS:
            raise NotImplementedError(f"Attention(dim_heads={dim_heads}): the fused attention kernels support head dims "
                                      f"{SUPPORTED_HEAD_DIMS}")
        dim_kv = dim_context if dim_context is not None else dim
        # shapes the kernels cannot run are refused here rather than as a kernel error at the first call
        if dim % dim_heads or dim_kv % dim_heads:
            raise ValueError(f"Attention: dim {dim} and dim_context {dim_kv} must be multiples of dim_heads {dim_heads}")
        if (dim // dim_heads) % (dim_kv // dim_heads):
            raise ValueError(f"Attention: {dim // dim_heads} query heads are not a multiple of {dim_kv // dim_heads} kv heads "
                             f"(dim {dim}, dim_context {dim_kv}, dim_heads {dim_heads})")
        self.dim = dim
        self.dim_heads = dim_heads
        self.causal = causal
        self.num_heads = dim // dim_heads
        self.kv_heads = dim_kv // dim_heads
        if dim_context is not None:
            self.to_q = nn.Linear(dim, dim, bias=False)
            self.to_kv = nn.Linear(dim_kv, dim_kv * 2, bias=False)
        else:
            self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.to_out = nn.Linear(dim, dim, bias=False)
        if zero_init_output:
            nn.init.zeros_(self.to_out.weight)
        self.qk_norm = qk_norm
        if qk_norm == "ln":         # transformer.py:305-307
            self.q_norm = nn.LayerNorm(dim_heads, elementwise_affine=True, eps=1.0e-6)
            self.k_norm = nn.LayerNorm(dim_heads, elementwise_affine=True, eps=1.0e-6)
        self.natten_kernel_size = natten_kernel_size

    def forward(self, x, context=None, mask=None, context_mask=None, rotary_pos_emb=None, causal=None):
        _need_gpu(x)
        causal = self.causal if causal is None else causal
        rope = None
        if rotary_pos_emb is not None and context is None:
            freqs = rotary_pos_emb[0] if isinstance(rotary_pos_emb, (tuple, list)) else rotary_pos_emb
            rope = KF.D.rope_tables(freqs, x.shape[1])
        if hasattr(self, "to_q"):
            params = (self.to_q.weight, self.to_kv.weight, self.to_out.weight)
        else:
            params = (self.to_qkv.weight, self.to_out.weight)
        if self.qk_norm == "ln":
            params += (self.q_norm.weight, self.q_norm.bias, self.k_norm.weight, self.k_norm.bias)
        return KF.AttentionFn.apply(self, x, context, KF._mask8(mask), KF._mask8(context_mask), rope, bool(causal), *params)


class ConformerModule(nn.Module):
    """transformer.py:550-583: LayerNorm -> 1 x 1 conv -> GLU -> depthwise conv (k = 17) -> LayerNorm -> SiLU -> 1 x 1 conv.
    Parameter names and shapes are the reference's (Conv1d weights [out, in / groups, k]); the math runs token-major in
    dit_ops.conformer_fwd / conformer_bwd (the 1 x 1 convolutions are GEMMs, the depthwise one kalle_dwconv1d_*)."""

    def __init__(self, dim, norm_kwargs={}):
        super().__init__()
        self.dim = dim
        self.in_norm = LayerNorm(dim, **norm_kwargs)
        self.pointwise_conv = nn.Conv1d(dim, dim, kernel_size=1, bias=False)
        self.glu = GLU(dim, dim, nn.SiLU())
        self.depthwise_conv = nn.Conv1d(dim, dim, kernel_size=17, groups=dim, padding=8, bias=False)
        self.depthwise_conv.weight._kalle_atomic_grad = True    # (its gradient is ADDED into its sink: cleared with the vectors)
        self.mid_norm = LayerNorm(dim, **norm_kwargs)
        self.swish = nn.SiLU()
        self.pointwise_conv_2 = nn.Conv1d(dim, dim, kernel_size=1, bias=False)

    def forward(self, x):
        _need_gpu(x)
        return KF.ConformerFn.apply(self, x, *self.parameters())


class TransformerBlock(nn.Module):
    """transformer.py:585-695."""

    def __init__(self, dim, dim_heads=64, cross_attend=False, dim_context=None, global_cond_dim=None, causal=False,
                 zero_init_branch_outputs=True, conformer=False, layer_ix=-1, remove_norms=False, attn_kwargs={},
                 ff_kwargs={}, norm_kwargs={}):
        super().__init__()
        if remove_norms:
            raise NotImplementedError("TransformerBlock(remove_norms)")
        self.dim = dim
        self.dim_heads = dim_heads
        self.cross_attend = cross_attend
        self.dim_context = dim_context
        self.causal = causal
        self.pre_norm = LayerNorm(dim, **norm_kwargs)
        self.self_attn = Attention(dim, dim_heads=dim_heads, causal=causal,
                                   zero_init_output=zero_init_branch_outputs, **attn_kwargs)
        if cross_attend:
            self.cross_attend_norm = LayerNorm(dim, **norm_kwargs)
            self.cross_attn = Attention(dim, dim_heads=dim_heads, dim_context=dim_context, causal=causal,
                                        zero_init_output=zero_init_branch_outputs, **attn_kwargs)
        self.ff_norm = LayerNorm(dim, **norm_kwargs)
        self.ff = FeedForward(dim, zero_init_output=zero_init_branch_outputs, **ff_kwargs)
        self.layer_ix = layer_ix
        self.conformer = ConformerModule(dim, norm_kwargs=norm_kwargs) if conformer else None
        self.global_cond_dim = global_cond_dim
        if global_cond_dim is not None:
            self.to_scale_shift_gate = nn.Sequential(nn.SiLU(), nn.Linear(global_cond_dim, dim * 6, bias=False))
            nn.init.zeros_(self.to_scale_shift_gate[1].weight)

    def forward(self, x, context=None, global_cond=None, mask=None, context_mask=None, rotary_pos_emb=None):
        _need_gpu(x)
        if isinstance(self.pre_norm.beta, nn.Parameter):
            raise NotImplementedError("LayerNorm(bias=True) inside the fused block")
        return KF.transformer_block(self, x, context=context, global_cond=global_cond, mask=mask,
                                    context_mask=context_mask, rotary_pos_emb=rotary_pos_emb)


class ContinuousTransformer(nn.Module):
    """transformer.py:697-812.  The reference wraps every layer in torch.utils.checkpoint (802, recompute in
    backward); with 288 GB of HBM3E per MI355X the block kernels keep their activations instead."""

    def __init__(self, dim, depth, *, dim_in=None, dim_out=None, dim_heads=64, cross_attend=False,
                 cond_token_dim=None, global_cond_dim=None, causal=False, rotary_pos_emb=True,
                 zero_init_branch_outputs=True, conformer=False, use_sinusoidal_emb=False, use_abs_pos_emb=False,
                 abs_pos_emb_max_length=10000, **kwargs):
        super().__init__()
        self.dim = dim
        self.depth = depth
        self.causal = causal
        self.layers = nn.ModuleList([])
        self.project_in = nn.Linear(dim_in, dim, bias=False) if dim_in is not None else nn.Identity()
        self.project_out = nn.Linear(dim, dim_out, bias=False) if dim_out is not None else nn.Identity()
        self.rotary_pos_emb = RotaryEmbedding(max(dim_heads // 2, 32)) if rotary_pos_emb else None
        self.use_sinusoidal_emb = use_sinusoidal_emb
        if use_sinusoidal_emb:
            self.pos_emb = ScaledSinusoidalEmbedding(dim)
        self.use_abs_pos_emb = use_abs_pos_emb
        if use_abs_pos_emb:
            self.pos_emb = AbsolutePositionalEmbedding(dim, abs_pos_emb_max_length)
        for i in range(depth):
            self.layers.append(TransformerBlock(dim, dim_heads=dim_heads, cross_attend=cross_attend,
                                                dim_context=cond_token_dim, global_cond_dim=global_cond_dim,
                                                causal=causal, zero_init_branch_outputs=zero_init_branch_outputs,
                                                conformer=conformer, layer_ix=i, **kwargs))

    def _project_context_for_all_layers(self, context):
        """the conditioning is one tensor for every layer: its k | v projections for all of them in ONE GEMM (dit_ops.ContextKV,
        hung on the context tensor for the layers to find); KALLE_BATCH_CTX_KV=0 keeps one projection per layer"""
        if context is None or os.environ.get("KALLE_BATCH_CTX_KV", "1") == "0" or len(self.layers) < 2:
            return
        layers = list(self.layers)
        if not all(l.cross_attend and l.cross_attn.qk_norm == "none" for l in layers):
            return
        dc = layers[0].cross_attn.to_kv.weight.shape[1]
        if context.shape[-1] != dc or any(l.cross_attn.to_kv.weight.shape != layers[0].cross_attn.to_kv.weight.shape for l in layers):
            return
        pre = getattr(context, "_kalle_bf16", None)
        ctxb = (pre if pre is not None else KF._to_bf16(context.contiguous())).view(-1, dc)
        ws = [l.cross_attn.to_kv.weight for l in layers]
        w_all = None
        frozen = not torch.is_grad_enabled() and all(getattr(w, "_kalle_bf16_pinned", None) is None for w in ws)
        if frozen:      # inference: the stacked weights are rebuilt only when a parameter changed (sampler loops call this per step)
            key = KF.ops.weights_key(*ws)
            hit = getattr(self, "_kalle_wall", None)
            if hit is not None and hit[0] == key:
                w_all = hit[1]
        bw = [KF.D.bf16_of(w) for w in ws]
        ckv = KF.D.ContextKV(ctxb, bw, w_all)
        if frozen and w_all is None:
            object.__setattr__(self, "_kalle_wall", (key, ckv.w_all, KF.ops.weights_pin(*ws)))
        try:
            context._kalle_ckv = ckv
        except (AttributeError, RuntimeError):
            pass

    def forward(self, x, mask=None, prepend_embeds=None, prepend_mask=None, global_cond=None, return_info=False,
                **kwargs):
        _need_gpu(x)
        batch, seq, device = *x.shape[:2], x.device
        info = {"hidden_states": []}
        if isinstance(self.project_in, nn.Linear):
            x = KF.linear(x, self.project_in.weight, out_dtype=torch.bfloat16)
        if prepend_embeds is not None:
            prepend_length, prepend_dim = prepend_embeds.shape[1:]
            assert prepend_dim == x.shape[-1], 'prepend dimension must match sequence dimension'
            x = KF.SpliceFn.apply(prepend_embeds, x)
            if prepend_mask is not None or mask is not None:
                mask = mask if mask is not None else torch.ones((batch, seq), device=device, dtype=torch.bool)
                prepend_mask = prepend_mask if prepend_mask is not None else torch.ones(
                    (batch, prepend_length), device=device, dtype=torch.bool)
                mask = torch.cat((prepend_mask, mask), dim=-1)
        else:
            x = KF.SpliceFn.apply(None, x)
        rotary = self.rotary_pos_emb.forward_from_seq_len(x.shape[1]) if self.rotary_pos_emb is not None else None
        if self.use_sinusoidal_emb or self.use_abs_pos_emb:         # transformer.py:796-797
            x = KF.AddRowsFn.apply(x, self.pos_emb(x))
        # transformer.py:800-802 calls every layer with rotary_pos_emb, global_cond and **kwargs only: the mask assembled above
        # is never handed to the layers, so padding masks do not reach the self-attention of a ContinuousTransformer (the
        # reference's behaviour, pinned by tests/golden/training_step.npz).  TransformerBlock / Attention called directly
        # do honour `mask`.
        mask = None
        ctx = kwargs.get("context")
        if ctx is not None and not ctx.requires_grad and ctx.dtype == torch.float32:
            # frozen conditioning (T5 / number embedders): one bf16 cast for all layers instead of one per layer
            kwargs = dict(kwargs, context=KF._to_bf16(ctx.contiguous()))
        elif ctx is not None and ctx.dtype == torch.float32 and ctx.is_cuda:
            # trainable conditioning (to_cond_embed, dit.py:49-53): the fp32 tensor stays the autograd input of every layer;
            # its bf16 copy is made once and rides on it, and the layers share one gradient accumulator (functional.py)
            gated = KF.ContextGateFn.apply(ctx) if ctx.requires_grad else ctx
            gated._kalle_bf16 = KF._to_bf16(ctx.detach().contiguous())
            gated._kalle_dctx = {}
            kwargs = dict(kwargs, context=gated)
        pre_kv = kwargs.pop("kalle_ctx_kv", None)        # DiffusionTransformer.precompute_conditioning: k | v of all layers, done once
        if pre_kv is not None and kwargs.get("context") is not None:
            try:
                kwargs["context"]._kalle_ckv = KF.D.ContextKV.preprojected(pre_kv, len(self.layers))
            except (AttributeError, RuntimeError):
                self._project_context_for_all_layers(kwargs.get("context"))
        else:
            self._project_context_for_all_layers(kwargs.get("context"))
        try:
            for layer in self.layers:
                x = layer(x, rotary_pos_emb=rotary, global_cond=global_cond, mask=mask, **kwargs)
                if return_info:
                    info["hidden_states"].append(x)
        finally:
            # the stacked projections belong to THIS forward of THIS transformer (the backward holds its own reference): a later
            # call with the same context tensor - another model, a block on its own, updated weights - must not find them
            c = kwargs.get("context")
            if c is not None and hasattr(c, "_kalle_ckv"):
                del c._kalle_ckv
        if isinstance(self.project_out, nn.Linear):
            x = KF.linear(x, self.project_out.weight, out_dtype=torch.float32)
        if return_info:
            return x, info
        return x
