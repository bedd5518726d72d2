"""Drop-in for the reference's task model `model_sigmaVAE.Llasa` (model_sigmaVAE.py:8-183, imported by
train_offline.py:19): same constructor, `forward` / `infer` / `sample` / `kl` signatures, returned dict and state-dict
keys (`base_model.model.layers.N.self_attn.q_proj.weight`, ..., `audio_linear.*`, `distribution_linear.{0,2}.*`).

`base_model` replaces `transformers.AutoModelForCausalLM.from_pretrained(path)` for Llama checkpoints: it reads the
local HF directory (config.json + safetensors / .bin) itself and runs the decoder layers on this package's HIP kernels
(llama_ops.py).  q/k/v and up/gate are held as fused parameters (one GEMM each); state_dict() / load_state_dict() split
and merge them under the HF names.  Parameters are fp32 masters with bf16 compute copies (the reference's
use_flash_attention=True path is bf16 weights + fp16 heads; =False is fp32) - the flag is accepted and ignored.
Every arithmetic step runs in a HIP kernel; torch supplies tensors, RNG and the autograd tape.
"""
import json
import os

import torch
from torch import nn

from . import functional as Fn
from . import llama_ops as LO
from . import ops
from .dit_ops import BF16, F32, GradOut, bf16_of, f32_of
from .generation import DeviceHeadSpec, device_head_limits, generate, generate_batch, generate_one
from .generation import RowSchedule, grouped_steps, refill_steps  # noqa: F401  (documented under this module's name)


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError("kalle_audio_amd Llasa modules run on an MI355X GPU only (no CPU fallback)")


# ------------------------------------------------------------------------------------------------ autograd shims
class LlamaLayerFn(torch.autograd.Function):
    """one decoder layer, forward + backward in llama_ops; parameter gradients go straight into the trainer's flat
    buckets when the layer carries `_kalle_grad_sinks` (engine.DataParallelTrainer), else back through autograd"""

    @staticmethod
    def forward(ctx, layer, x, mask8, rope, *params):
        """mask8: the key mask [B, L], None, or an ops.Packed - x is then [1, total_rows, Dm], the packed rows of a ragged batch"""
        B, L, Dm = x.shape
        p = LO.layer_params(layer)
        seqs, mask8 = (mask8, None) if isinstance(mask8, ops.Packed) else (None, mask8)
        y, sv = LO.layer_fwd(p, x.contiguous().view(B * L, Dm), B, L, rope, mask8, seqs=seqs)
        ctx.layer, ctx.sv, ctx.aux, ctx.dims = layer, sv, (mask8, rope, seqs), (B, L, Dm)
        layer._kalle_last_rows = B * L                  # (the trainer picks its gradient-clearing rule from it; packed: total_rows)
        return y.view(B, L, Dm)

    @staticmethod
    def backward(ctx, g):
        layer, sv = ctx.layer, ctx.sv
        mask8, rope, seqs = ctx.aux
        B, L, Dm = ctx.dims
        p = LO.layer_params(layer)
        gf = g.contiguous().view(B * L, Dm)
        sinks = getattr(layer, "_kalle_grad_sinks", None)
        go = GradOut(sinks, getattr(layer, "_kalle_grad_accumulate", False)) if sinks else GradOut()
        go.wgrad_overwrite = bool(sinks) and getattr(layer, "_kalle_wgrad_overwrite", False)
        sh = Fn._GRAD_SHADOW.pop(gf.data_ptr(), None)
        g_bf16 = sh[1] if sh is not None and sh[0] == ("llama", layer.layer_idx + 1) and sh[1].shape == gf.shape else None
        if len(Fn._GRAD_SHADOW) > 8:
            Fn._GRAD_SHADOW.clear()
        dx, dxb, go = LO.layer_bwd(p, sv, gf, B, L, rope, mask8, go=go, g_bf16=g_bf16, want_dx_bf16=layer.layer_idx > 0,
                                   seqs=seqs)
        if dxb is not None:
            Fn._GRAD_SHADOW[dx.data_ptr()] = (("llama", layer.layer_idx), dxb)
        ctx.sv = None
        hook = getattr(layer, "_kalle_on_backward_done", None)
        if hook is not None:
            hook(layer)
        return (None, dx.view(B, L, Dm), None, None) + tuple(go.grads.get(n) for n in LO.PARAM_ORDER)


def _copy_sequences(src, dst, seqs, L, pack):
    """pack: dst [total_rows, D] rows row0[b] .. + lens[b] <- src [B, L, D] rows (b, 0 .. lens[b]); not pack: the opposite copy.
    One kalle_segment_copy launch per 64 sequences (a segment = one sequence's lens[b] * D contiguous elements)."""
    D = src.shape[-1]
    padded = [b * L * D for b in range(seqs.nseq)]
    packed = [r * D for r in seqs.row0]
    n = [m * D for m in seqs.lens]
    so, do = (padded, packed) if pack else (packed, padded)
    return ops.segment_copy(src, dst, so, do, n, 1, 1, src_strides=(0, 0, 0), dst_strides=(0, 0, 0))


class PackRowsFn(torch.autograd.Function):
    """[B, L, D] -> [1, total_rows, D]: the live rows of a right-padded batch, sequence after sequence; rows outside every
    sequence (total_rows is a multiple of LO.PACK_GRANULE) are zero.  unpack=True is the opposite map, [1, total_rows, D] ->
    [B, L, D] with zeros at padded positions; each is the other's backward."""

    @staticmethod
    def forward(ctx, x, seqs, B, L, unpack=False):
        ctx.seqs, ctx.dims, ctx.unpack = seqs, (B, L), unpack
        return PackRowsFn._run(x, seqs, B, L, not unpack)

    @staticmethod
    def _run(x, seqs, B, L, pack):
        x = x.contiguous()
        D = x.shape[-1]
        if pack:
            out = (torch.zeros if seqs.has_gaps else torch.empty)((1, seqs.total_rows, D), device=x.device, dtype=x.dtype)
        else:
            out = (torch.zeros if seqs.live_rows != B * L else torch.empty)((B, L, D), device=x.device, dtype=x.dtype)
        return _copy_sequences(x, out, seqs, L, pack)

    @staticmethod
    def backward(ctx, g):
        B, L = ctx.dims
        return PackRowsFn._run(g, ctx.seqs, B, L, ctx.unpack), None, None, None, None


class EmbedMixFn(torch.autograd.Function):
    """input_embed = audio_embed * audio_mask + embed_tokens(input_ids) * ids_mask   (model_sigmaVAE.py:66, 73)"""

    @staticmethod
    def forward(ctx, ids, table, audio, ids_mask, audio_mask):
        B, L = ids.shape
        D = table.shape[1]
        a = audio.contiguous().view(B * L, D)
        out = ops.embed_mix_fwd(ids.contiguous().view(-1), f32_of(table), a, ids_mask.view(-1), audio_mask.view(-1))
        ctx.save_for_backward(ids, ids_mask, audio_mask)
        ctx.table, ctx.adt, ctx.shape = table, audio.dtype, (B, L, D)
        return out.view(B, L, D)

    @staticmethod
    def backward(ctx, g):
        ids, im, am = ctx.saved_tensors
        B, L, D = ctx.shape
        table = ctx.table
        sink = getattr(table, "_kalle_grad_sink", None)
        dt = sink if sink is not None else (torch.zeros_like(table, dtype=F32) if ctx.needs_input_grad[1] else None)
        da = ops.embed_mix_bwd(g.contiguous().view(B * L, D), ids.contiguous().view(-1), im.view(-1), am.view(-1), dtable=dt,
                               want_daudio=ctx.needs_input_grad[2])
        if da is not None:
            da = Fn._like(da, ctx.adt).view(B, L, D)
        return None, (None if sink is not None else dt), da, None, None


class GELUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(Fn._like(dy.contiguous(), x.dtype), x)


class GaussKLFn(torch.autograd.Function):
    """(audio_loss, end_loss) of model_sigmaVAE.py:85-95: masked means of KL(N(pred, s) || N(label, s)) / latent_dim"""

    @staticmethod
    def forward(ctx, pred, label, target_mask, end_mask, std):
        d = pred.shape[-1]
        p2 = Fn._to_f32(pred.contiguous()).view(-1, d)
        l2 = Fn._to_f32(label.contiguous()).view(-1, d)
        sums = ops.gauss_kl_fwd(p2, l2, target_mask.view(-1), end_mask.view(-1), std)
        ctx.save_for_backward(p2, l2, target_mask, end_mask, sums)
        ctx.std, ctx.pdt, ctx.shape = std, pred.dtype, pred.shape
        # the two ratios are 1-element reductions of four numbers the kernel produced (plumbing, like a .view())
        return sums[0] / sums[1], sums[2] / sums[3]

    @staticmethod
    def backward(ctx, ga, gb):
        p2, l2, tm, em, sums = ctx.saved_tensors
        dp = ops.gauss_kl_bwd(p2, l2, tm.view(-1), em.view(-1), sums, ga.float().reshape(1).contiguous(),
                              gb.float().reshape(1).contiguous(), ctx.std)
        return Fn._like(dp, ctx.pdt).view(ctx.shape), None, None, None, None


# ------------------------------------------------------------------------------------------------ modules
class Linear(nn.Linear):
    """nn.Linear whose forward / backward are kalle_gemm_bf16 launches"""

    def forward(self, x):
        _need_gpu(x)
        return Fn.linear(x, self.weight, self.bias, out_dtype=F32)


class GELU(nn.Module):
    def forward(self, x):
        return GELUFn.apply(x)


class _FusedLinear(nn.Module):
    """several bias-free nn.Linear that share their input, stored as ONE weight [sum(out_i), in] so they run as one
    GEMM; `parts` = ((hf_name, out_features), ...) are the names they carry in state_dict()"""

    def __init__(self, in_features, parts):
        super().__init__()
        self.parts = tuple(parts)
        self.weight = nn.Parameter(torch.empty(sum(n for _, n in parts), in_features))
        nn.init.normal_(self.weight, std=0.02)


class _Holder(nn.Module):
    def __init__(self, out_features, in_features):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.normal_(self.weight, std=0.02)


def _split_hooks(owner, fused_attr):
    """state_dict(): fused weight -> HF names; load_state_dict(): HF names -> fused weight"""
    def save_hook(module, sd, prefix, local_metadata):
        key = prefix + fused_attr + ".weight"
        if key in sd:
            w = sd.pop(key)
            o = 0
            for name, n in getattr(module, fused_attr).parts:
                sd[prefix + name + ".weight"] = w[o:o + n]
                o += n

    def load_hook(module, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        parts = getattr(module, fused_attr).parts
        keys = [prefix + name + ".weight" for name, _ in parts]
        if all(k in sd for k in keys):
            sd[prefix + fused_attr + ".weight"] = torch.cat([sd.pop(k) for k in keys], 0)

    owner._register_state_dict_hook(save_hook)
    owner._register_load_state_dict_pre_hook(load_hook, with_module=True)


class LlamaRMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, x):
        return Fn.RMSNormFn.apply(x, self.weight, self.variance_epsilon)


LLAMA_HEAD_DIMS = (64, 128)     # what the attention kernels rotate a whole head at (Llama-3.2-1B; Llama-3.2-3B, Llama-3.1-8B)


class LlamaAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_heads, self.num_kv_heads = cfg["num_attention_heads"], cfg["num_key_value_heads"]
        D = cfg["hidden_size"]
        hd = self.head_dim = cfg.get("head_dim") or D // self.num_heads
        if hd not in LLAMA_HEAD_DIMS or D != self.num_heads * hd or self.num_heads % self.num_kv_heads or cfg.get("attention_bias"):
            raise NotImplementedError(
                f"Llama decoders are supported with head_dim in {LLAMA_HEAD_DIMS}, hidden_size == num_attention_heads * head_dim, "
                f"num_attention_heads a multiple of num_key_value_heads and no projection biases; got head_dim={hd}, "
                f"hidden_size={D}, num_attention_heads={self.num_heads}, num_key_value_heads={self.num_kv_heads}, "
                f"attention_bias={bool(cfg.get('attention_bias'))}")
        self.qkv_proj = _FusedLinear(D, (("q_proj", self.num_heads * hd), ("k_proj", self.num_kv_heads * hd),
                                         ("v_proj", self.num_kv_heads * hd)))
        self.o_proj = _Holder(D, self.num_heads * hd)
        _split_hooks(self, "qkv_proj")


class LlamaMLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        if cfg.get("mlp_bias") or cfg.get("hidden_act", "silu") != "silu":
            raise NotImplementedError(f"Llama decoders are supported with hidden_act='silu' and no MLP biases; got hidden_act="
                                      f"{cfg.get('hidden_act', 'silu')!r}, mlp_bias={bool(cfg.get('mlp_bias'))}")
        D, I = cfg["hidden_size"], cfg["intermediate_size"]
        # value half first, gate half second: the layout of the fused GEMM + SwiGLU epilogue
        self.up_gate_proj = _FusedLinear(D, (("up_proj", I), ("gate_proj", I)))
        self.down_proj = _Holder(D, I)
        _split_hooks(self, "up_gate_proj")


class LlamaDecoderLayer(nn.Module):
    _kalle_bucket_unit = True      # engine.DataParallelTrainer: one gradient bucket / all-reduce per layer

    def __init__(self, cfg, layer_idx):
        super().__init__()
        self.layer_idx = layer_idx
        self.self_attn = LlamaAttention(cfg)
        self.mlp = LlamaMLP(cfg)
        self.input_layernorm = LlamaRMSNorm(cfg["hidden_size"], cfg.get("rms_norm_eps", 1e-6))
        self.post_attention_layernorm = LlamaRMSNorm(cfg["hidden_size"], cfg.get("rms_norm_eps", 1e-6))

    def forward(self, x, mask8, rope):
        have = dict(self.named_parameters())
        return LlamaLayerFn.apply(self, x, mask8, rope, *[have[n] for n in LO.PARAM_ORDER])


class _Embedding(nn.Module):
    def __init__(self, num_embeddings, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_embeddings, dim))
        nn.init.normal_(self.weight, std=0.02)
        self.weight._kalle_wants_sink = True     # the trainer lets the backward scatter-add into its flat gradient

    def forward(self, ids):
        _need_gpu(ids)
        z = torch.zeros(ids.shape + (self.weight.shape[1],), device=ids.device, dtype=BF16)
        one = torch.ones(ids.shape, device=ids.device, dtype=F32)
        return EmbedMixFn.apply(ids, self.weight, z, one, torch.zeros_like(one))


class LlamaModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.embed_tokens = _Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.layers = nn.ModuleList([LlamaDecoderLayer(cfg, i) for i in range(cfg["num_hidden_layers"])])
        self.norm = LlamaRMSNorm(cfg["hidden_size"], cfg.get("rms_norm_eps", 1e-6))
        hd = cfg.get("head_dim") or cfg["hidden_size"] // cfg["num_attention_heads"]
        self.head_dim = hd
        self._inv_freq = LO.inv_freq(hd, cfg.get("rope_theta", 10000.0), cfg.get("rope_scaling"))
        self._rope_cache = {}
        self._decode_fmt = None

    DECODE_WEIGHT_FORMATS = ("e4m3",)
    _pack = False                   # pack_sequences()

    def quantize_decode_weights(self, fmt="e4m3"):
        """fmt "e4m3": the KV-cached single-position steps (forward_cached at n == 1, forward_cached_batch) read the four
        projections of every layer as OCP e4m3 codes with one fp32 scale per output row (kalle_llama_decode_step_w8 /
        _rows_w8): half the bytes a generated frame streams.  Activations, accumulation and every bf16 rounding point stay.
        The quantised copies are made lazily, per layer, at the next step and re-made when a weight changes; prefill (n > 1,
        prefill_row), training and forward() keep the bf16 weights and kernels, so the copies are 0.5 x the bf16 bytes ON TOP.
        fmt None: back to the bf16 steps; the quantised copies are dropped."""
        if fmt is not None and fmt not in self.DECODE_WEIGHT_FORMATS:
            raise NotImplementedError(f"decode weight format {fmt!r}: supported formats are {self.DECODE_WEIGHT_FORMATS} (or None)")
        if fmt is not None:
            D, I = self.cfg["hidden_size"], self.cfg["intermediate_size"]
            if D % 16 or I % 16:
                raise NotImplementedError(f"decode weight format {fmt!r} needs hidden_size and intermediate_size to be multiples "
                                          f"of 16 (a 16-byte load holds 16 weights); got hidden_size={D}, intermediate_size={I}")
        self._decode_fmt = fmt
        if fmt is None:          # drop the quantised copies (a KV cache built meanwhile holds its plan's until its next step)
            self.__dict__.pop("_decode_weight_list", None)
            for layer in self.layers:
                for w in self._layer_weights(layer):
                    w.__dict__.pop("_kalle_e4m3", None)
        return self

    def _decode_plan(self, cache, device, rows=None):
        """the cache's plan for the current decode weight format; rebuilt when the format changed or a weight did - in EITHER
        format: a bf16 plan holds the addresses of the bf16 compute copies and of the norm scales, a quantised one those of the
        codes and scales, and both go stale with the parameters they were made from (ops.weights_key)"""
        fmt = self._decode_fmt
        plan = cache.get("plan")
        ws = self._decode_weights()
        key = ops.weights_key(*ws)
        if plan is None or plan.get("fmt") != fmt or plan["wkey"] != key:
            if fmt is None:
                ps = [LO.layer_params(layer) for layer in self.layers]
                ts = [(p.g1, p.wqkv, p.wo, p.g2, p.wug, p.wdown, kv) for p, kv in zip(ps, cache["kv"])]
            else:
                ps, qs = zip(*(LO.layer_params_w8(layer) for layer in self.layers))
                ts = [q + (kv,) for q, kv in zip(qs, cache["kv"])]
            p0 = ps[0]
            plan = ops.llama_decode_plan(ts, p0.H, p0.Hkv, p0.wug.shape[0] // 2, device, head_dim=p0.hd, rows=rows)
            plan["eps"], plan["wkey"], plan["wpin"] = p0.eps, key, ops.weights_pin(*ws)
            cache["plan"] = plan
        return plan

    def _decode_weights(self):
        """the parameters a decode plan reads (per layer: two norm scales, four projections), looked up at every step: module
        attribute lookups are too slow to repeat for every frame, so what is collected once is the `_parameters` dict of each
        owning module - a replaced Parameter object (load_state_dict(assign=True)) is found there, a remembered one would not be"""
        slots = self.__dict__.get("_decode_weight_list")
        if slots is None:
            slots = self.__dict__["_decode_weight_list"] = [
                m._parameters for layer in self.layers
                for m in (layer.input_layernorm, layer.self_attn.qkv_proj, layer.self_attn.o_proj, layer.post_attention_layernorm,
                          layer.mlp.up_gate_proj, layer.mlp.down_proj)]
        return [d["weight"] for d in slots]

    @staticmethod
    def _layer_weights(layer):
        return (layer.self_attn.qkv_proj.weight, layer.self_attn.o_proj.weight, layer.mlp.up_gate_proj.weight,
                layer.mlp.down_proj.weight)

    def _rope(self, L, device):
        key = (L, str(device))
        if key not in self._rope_cache:
            self._rope_cache = {key: LO.rope_tables(L, self._inv_freq, device)}
        return self._rope_cache[key]

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, **kwargs):
        """returns (last_hidden_state,) - the reference indexes [0] (model_sigmaVAE.py:78-81, 123-125)"""
        x = self.embed_tokens(input_ids) if inputs_embeds is None else inputs_embeds
        _need_gpu(x)
        B, L, _ = x.shape
        x = Fn._to_f32(x.contiguous())
        rope = self._rope(L, x.device)
        seqs = self._packed(attention_mask, B, L, x.device) if self._pack and attention_mask is not None else None
        if seqs is not None:
            # the live rows alone go through the layers and the final norm; padded positions come back as zeros
            x = PackRowsFn.apply(x, seqs, B, L)
            for layer in self.layers:
                x = layer(x, seqs, rope)
            return (PackRowsFn.apply(self.norm(x), seqs, B, L, True),)
        mask8 = Fn._mask8(attention_mask > 0) if attention_mask is not None else None
        for layer in self.layers:
            x = layer(x, mask8, rope)
        return (self.norm(x),)

    def pack_sequences(self, enable=True):
        """Opt-in: forward() with an attention_mask runs the decoder on the live rows only - the rows of every sample packed
        back to back into [1, total_rows, D] (total_rows = sum of the lengths rounded up to LO.PACK_GRANULE, the extra rows
        zero), varlen causal attention per sequence with rotary positions restarting at 0, the result scattered back with zeros
        at padded positions.  The mask must be right-padded (LO.packed_lengths: ValueError otherwise); reading the lengths costs
        one device-to-host copy of the mask per call.  The KV-cached paths ignore the flag.  Off (the default): nothing changes."""
        self._pack = bool(enable)
        return self

    def _packed(self, attention_mask, B, L, device):
        """the ops.Packed of a right-padded mask, or None where packing gains nothing: no padding and a row count that is a
        multiple of the granule already"""
        lens = LO.packed_lengths((attention_mask > 0).cpu())
        if sum(lens) == B * L and (B * L) % LO.PACK_GRANULE == 0:
            return None
        return ops.Packed.back_to_back(lens, device, granule=LO.PACK_GRANULE)


    # ---- inference with a KV cache (batch 1) ---------------------------------------------------------------------
    def init_cache(self, max_len, device):
        """one bf16 [max_len, 2 * kv_heads * head_dim] buffer per layer (un-rotated k | v rows)"""
        w = 2 * self.cfg["num_key_value_heads"] * self.head_dim
        return {"kv": [torch.zeros((max_len, w), device=device, dtype=BF16) for _ in self.layers], "len": 0,
                "rope": LO.rope_tables(max_len, self._inv_freq, device)}

    @torch.no_grad()
    def forward_cached(self, inputs_embeds, cache, final_norm=True):
        """appends the positions of `inputs_embeds` [1, n, D] to the cache and returns their last hidden states
        (final_norm=False: the residual stream before `self.norm`, what kalle_llasa_frame_head_rows takes)"""
        _need_gpu(inputs_embeds)
        _, n, Dm = inputs_embeds.shape
        t0 = cache["len"]
        if t0 + n > cache["kv"][0].shape[0]:
            raise ValueError("KV cache too short")
        x = Fn._to_f32(inputs_embeds.contiguous()).view(n, Dm)
        if n == 1:
            # one generated frame: the whole stack is sequenced by kalle_llama_decode_step (one host call)
            plan = self._decode_plan(cache, x.device)
            x = ops.llama_decode_step(plan, x.view(Dm), t0, cache["kv"][0].shape[0], cache["rope"], plan["eps"])
        else:
            for layer, kv in zip(self.layers, cache["kv"]):
                x = LO.layer_fwd_cached(LO.layer_params(layer), x, kv, t0, cache["rope"])
        cache["len"] = t0 + n
        return self.norm(x.view(1, n, Dm)) if final_norm else x.view(1, n, Dm)

    # ---- inference with a KV cache, R sequences of different lengths per step -------------------------------------------------
    def init_cache_batch(self, R, max_len, device):
        """one bf16 [R, max_len, 2 * kv_heads * head_dim] buffer per layer, a length per row, rope tables for max_len"""
        if not 1 <= R <= ops.DECODE_WIDE_MAX_ROWS:
            raise ValueError(f"a batch cache holds 1 .. {ops.DECODE_WIDE_MAX_ROWS} sequences, got {R}")
        if R > ops.DECODE_MAX_ROWS and self._decode_fmt is not None:
            raise NotImplementedError(f"quantize_decoder({self._decode_fmt!r}) with more than {ops.DECODE_MAX_ROWS} rows ({R}): "
                                      "the wide decode step reads bf16 weights only")
        w = 2 * self.cfg["num_key_value_heads"] * self.head_dim
        return {"kv": [torch.zeros((R, max_len, w), device=device, dtype=BF16) for _ in self.layers], "len": [0] * R,
                "rope": LO.rope_tables(max_len, self._inv_freq, device)}

    @torch.no_grad()
    def prefill_row(self, inputs_embeds, cache, r, final_norm=True):
        """appends the positions of `inputs_embeds` [1, n, D] to row r of a batch cache (the layers of forward_cached on that
        row's slice) and returns their last hidden states (final_norm=False: before `self.norm`)"""
        _need_gpu(inputs_embeds)
        _, n, Dm = inputs_embeds.shape
        t0 = cache["len"][r]
        if t0 + n > cache["kv"][0].shape[1]:
            raise ValueError("KV cache too short")
        x = Fn._to_f32(inputs_embeds.contiguous()).view(n, Dm)
        for layer, kv in zip(self.layers, cache["kv"]):
            x = LO.layer_fwd_cached(LO.layer_params(layer), x, kv[r], t0, cache["rope"])
        cache["len"][r] = t0 + n
        return self.norm(x.view(1, n, Dm)) if final_norm else x.view(1, n, Dm)

    @torch.no_grad()
    def prefill_rows(self, embeds, cache, rows, final_norm=True):
        """prefill_row for several prompts in ONE pass over the decoder weights: embeds, a list of [1, n_i, D], go through the
        stack packed back to back (ops.Packed, LO.PACK_GRANULE; varlen causal attention, positions from 0) and their k | v rows
        land in rows `rows` (distinct, each at length 0: a prompt does not continue a row) of the batch cache.  Sets
        cache["len"][r] = n_i and returns [len(rows), 1, D], the LAST position's hidden state of every prompt (final_norm=False:
        before `self.norm`).  One prompt is prefill_row.  The bf16 weights, also under quantize_decode_weights."""
        rows = [int(r) for r in rows]
        lens = [int(e.shape[1]) for e in embeds]
        R, room = len(cache["len"]), cache["kv"][0].shape[1]
        if not rows or len(rows) != len(embeds):
            raise ValueError(f"prefill_rows takes one cache row per prompt, got {len(embeds)} prompts and rows {rows}")
        if len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= R:
            raise ValueError(f"prefill_rows takes distinct rows of the cache's {R}, got {rows}")
        busy = [r for r in rows if cache["len"][r] != 0]
        if busy:
            raise ValueError(f"prefill_rows starts at position 0: rows {busy} of the cache are not at length 0")
        if min(lens) < 1 or max(lens) > room:
            raise ValueError("KV cache too short" if max(lens) > room else "an empty prompt")
        _need_gpu(embeds[0])
        if len(rows) == 1:
            return self.prefill_row(embeds[0], cache, rows[0], final_norm=final_norm)[:, -1:, :]
        dev, Dm = embeds[0].device, embeds[0].shape[2]
        seqs = ops.Packed.back_to_back(lens, dev, granule=LO.PACK_GRANULE)
        parts = [Fn._to_f32(e.contiguous()).view(n, Dm) for e, n in zip(embeds, lens)]
        if seqs.has_gaps:
            parts.append(torch.zeros((seqs.total_rows - seqs.live_rows, Dm), device=dev, dtype=F32))
        x = torch.cat(parts, dim=0)
        for layer, kv in zip(self.layers, cache["kv"]):
            x = LO.layer_fwd_cached_varlen(LO.layer_params(layer), x, kv, seqs, rows, cache["rope"])
        last = torch.tensor([r0 + n - 1 for r0, n in zip(seqs.row0, lens)], device=dev)
        x = x.index_select(0, last).view(len(rows), 1, Dm)
        for r, n in zip(rows, lens):
            cache["len"][r] = n
        return self.norm(x) if final_norm else x

    @torch.no_grad()
    def forward_cached_batch(self, inputs_embeds, cache, active=None, final_norm=True):
        """one new position for every active row: appends `inputs_embeds` [R, 1, D] row by row to the caches and returns the last
        hidden states [R, 1, D].  active: R host booleans (default: all); an inactive row's cache and length stay as they are
        and its output row is that of its last active step (zero before the first).  The whole stack is sequenced by kalle_llama_decode_step_rows (one host call).
        final_norm=False: the residual stream before `self.norm` (the step's own buffer, rewritten by the next step)."""
        _need_gpu(inputs_embeds)
        R, n, Dm = inputs_embeds.shape
        if n != 1 or R != len(cache["len"]):
            raise ValueError("forward_cached_batch takes one position for each row of the cache")
        active = [True] * R if active is None else [bool(a) for a in active]
        rows = cache["kv"][0].shape[1]
        t0 = [t if a else -1 for t, a in zip(cache["len"], active)]
        if max(t0) >= rows:
            raise ValueError("KV cache too short")
        x = Fn._to_f32(inputs_embeds.contiguous()).view(R, Dm)
        plan = self._decode_plan(cache, x.device, rows=R)
        x = ops.llama_decode_step(plan, x, t0, rows, cache["rope"], plan["eps"])
        cache["len"] = [t + 1 if a else t for t, a in zip(cache["len"], active)]
        return self.norm(x.view(R, 1, Dm)) if final_norm else x.view(R, 1, Dm)


class LlamaForCausalLM(nn.Module):
    """the parts of transformers' LlamaForCausalLM the task model touches: `.model`, `.config`, `.vocab_size`,
    `resize_token_embeddings`, tied `lm_head.weight` in the state dict"""

    def __init__(self, cfg):
        super().__init__()
        self.config = _Cfg(cfg)
        self.model = LlamaModel(cfg)
        self.lm_head = _Holder(cfg["vocab_size"], cfg["hidden_size"])
        self.vocab_size = cfg["vocab_size"]
        self.tied = bool(cfg.get("tie_word_embeddings", False))
        if self.tied:
            self.lm_head.weight = self.model.embed_tokens.weight

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        if cfg.get("model_type", "llama") != "llama":
            raise NotImplementedError(f"only Llama checkpoints are supported, got model_type={cfg.get('model_type')!r}")
        model = cls(cfg)
        sd = _read_hf_weights(path)
        if sd is not None:
            if model.tied and "lm_head.weight" not in sd:
                sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
            missing, unexpected = model.load_state_dict(sd, strict=False)
            if missing:
                raise RuntimeError(f"checkpoint {path} lacks {missing}")
        return model

    def resize_token_embeddings(self, n):
        """new rows start at the mean of the old ones (transformers draws them around that mean)"""
        old = self.model.embed_tokens.weight.data
        if n != old.shape[0]:
            new = old.mean(0, keepdim=True).repeat(n, 1)
            new[:min(n, old.shape[0])] = old[:n]
            self.model.embed_tokens.weight = nn.Parameter(new)
            self.model.embed_tokens.weight._kalle_wants_sink = True
            if self.tied:
                self.lm_head.weight = self.model.embed_tokens.weight
            else:
                oh = self.lm_head.weight.data
                nh = oh.mean(0, keepdim=True).repeat(n, 1)
                nh[:min(n, oh.shape[0])] = oh[:n]
                self.lm_head.weight = nn.Parameter(nh)
        self.config.vocab_size = n
        self.vocab_size = n
        return self.model.embed_tokens


class _Cfg(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _read_hf_weights(path):
    from safetensors.torch import load_file
    idx = os.path.join(path, "model.safetensors.index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
        sd = {}
        for fn in files:
            sd.update(load_file(os.path.join(path, fn)))
        return {k: v.float() for k, v in sd.items()}
    one = os.path.join(path, "model.safetensors")
    if os.path.exists(one):
        return {k: v.float() for k, v in load_file(one).items()}
    b = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(b):
        return {k: v.float() for k, v in torch.load(b, map_location="cpu").items()}
    return None


class Llasa(nn.Module):
    """model_sigmaVAE.py:8-183"""

    def __init__(self, config, tokenizer, use_flash_attention=True):
        super().__init__()
        self.use_fa = use_flash_attention
        self.base_model = LlamaForCausalLM.from_pretrained(config['llm_model_name_or_path'])
        self.base_model.resize_token_embeddings(len(tokenizer))
        self.base_model.vocab_size = len(tokenizer)
        self.vocab_size = self.base_model.config.vocab_size
        self.hidden_size = self.base_model.config.hidden_size
        self.audio_linear = Linear(config['latent_dim'], config['audio_proj_dim'])
        self.distribution_linear = nn.Sequential(
            Linear(config['audio_proj_dim'], config['latent_dim']),
            GELU(),
            Linear(config['latent_dim'], config['latent_dim']))
        self.init_sigmaVAE()

    def quantize_decoder(self, fmt="e4m3"):
        """LlamaModel.quantize_decode_weights on the decoder: `infer` and `infer_batch` then stream e4m3 weights per frame"""
        self.base_model.model.quantize_decode_weights(fmt)
        return self

    def pack_sequences(self, enable=True):
        """LlamaModel.pack_sequences on the decoder (opt-in): `forward` then spends no decoder work on padded positions.  Its
        signature, returned dict and losses stay; `pre_mean` at padded positions becomes what the head gives a zero hidden state
        (undefined in the reference, and different from the padded mode here)."""
        self.base_model.model.pack_sequences(enable)
        return self

    def forward(self, input_ids, audio_latents, audio_distribution_l, ids_mask, audio_mask, target_mask, end_mask,
                noise=None):
        """`noise` (extension, for seed-free parity tests): the N(0,1) draw of sample(); default torch.randn_like"""
        _need_gpu(input_ids)
        f = lambda m: m.to(F32).contiguous()
        ids_mask, audio_mask, target_mask, end_mask = f(ids_mask), f(audio_mask), f(target_mask), f(end_mask)
        audio_latents = self.sample(mean=audio_latents, noise=noise)
        audio_embed = self.audio_linear(audio_latents)                                   # b,t,d
        audio_latents_dim = audio_latents.shape[-1]
        input_embed = EmbedMixFn.apply(input_ids, self.base_model.model.embed_tokens.weight, audio_embed, ids_mask,
                                       audio_mask)
        attention_mask = ids_mask + audio_mask     # two 0/1 row masks; >0 is all the decoder reads from it
        hidden = self.base_model.model(inputs_embeds=input_embed, attention_mask=attention_mask)[0]
        x = self.distribution_linear(hidden)                                             # b,t,d2
        audio_loss, end_loss = GaussKLFn.apply(x, audio_distribution_l, target_mask, end_mask, float(self.std))
        return {"audio_loss": audio_loss, "end_loss": end_loss, "pre_mean": x, "pre_log_scale": self.std,
                "ground_truth_audio_latents": audio_latents}

    @torch.no_grad()
    def infer(self, input_ids, audio_latents, end_disp_kl_thres=0.5, max_length=200, sample=False, use_cfg=None,
              flow=None, use_cache=True, device_head=False, noise=None, stop_lag=0):
        """model_sigmaVAE.py:106-148: frame-by-frame generation, stopping when KL(N(mean, std) || N(1, e)) / dim drops
        below the threshold.  The reference re-runs the decoder over the whole prefix for every frame (O(T^2) GEMM work);
        with use_cache (default) the prompt is prefilled once and every frame is one single-position pass against a KV
        cache - same arithmetic per position.  use_cache=False reproduces the reference's schedule.
        device_head=True (extension, opt-in): everything between two decode steps - final norm, distribution_linear, the
        sample, the stop KL, audio_linear - is one call of kalle_llasa_frame_head_rows, so a frame is two host calls and one
        4-byte read-back; `sample()` and the head modules' forward are not called.  noise: the N(0, 1) draws, fp32,
        broadcastable to [max_length, 1, latent_dim] (default: one torch.randn((1, 1, latent_dim)) per frame, the shape and order
        `sample()` draws in, so a seeded run consumes the generator as the host path does).  stop_lag=1: frame i + 1 is enqueued
        before frame i's KL is read, so the read-back no longer drains the device; the returned tensor is the same, bit for bit,
        but the frame after the stop has run (and been discarded): the cache holds one extra position and, with noise=None, one
        extra draw has been taken from the generator."""
        return generate_one(self, input_ids, audio_latents, end_disp_kl_thres, max_length, use_cache, device_head, noise,
                            stop_lag)

    infer_batch_rows = ops.DECODE_MAX_ROWS      # sequences decoded per step by infer_batch (the kernels take up to DECODE_MAX_ROWS)

    @torch.no_grad()
    def infer_batch(self, prompts, end_disp_kl_thres=0.5, max_length=200, device_head=False, noise=None, stop_lag=0,
                    refill=False, rows=None):
        """`infer` (KV-cached) for a list of (input_ids, audio_latents or None): the utterances of a group are generated together,
        one decoder pass per frame for all of them, so the decoder weights are read once per frame instead of once per frame
        and utterance.  Returns a list with what `infer` returns for each prompt.  The prompts are prefilled one by one (they
        differ in length); a row that meets `infer`'s stop rule leaves the batch (its cache is not touched again) while the
        others go on.  Lists longer than `infer_batch_rows` are processed in groups; one prompt is `infer` itself.
        device_head / noise / stop_lag: as in `infer`, noise broadcastable to [max_length, len(prompts), latent_dim] and drawn,
        when absent, as one torch.randn((R, 1, latent_dim)) per frame for the R rows of a group; with stop_lag=1 a stopped
        row's cache holds one extra position.
        max_length (extension): an int, or one int per prompt - utterance p leaves after max_length[p] frames and returns
        max_length[p] - 1 of them, as the single cap does.
        refill=True (extension, opt-in): the whole list shares ONE batch cache of min(infer_batch_rows, len(prompts)) rows; a row
        whose utterance stops takes the next waiting prompt at the next frame boundary instead of idling until its group ends,
        and the prompts admitted at one boundary are prefilled together in one packed pass (LlamaModel.prefill_rows).  Results
        come back in prompt order, each what `infer` returns.  With explicit noise utterance p's frame f reads noise[f, p] at
        whatever row and step it runs, so its result depends on its own prompt and noise only (up to rounding: the packed
        prefill GEMMs may pick another plan at another row count).  With noise=None one torch.randn((R, 1, latent_dim)) is
        drawn per global step, so WHICH utterance gets which draw differs from the grouped mode (and, under the host head, one
        draw per step covers all R rows as before).  stop_lag=1: a stopped row is refilled one step later (its discarded extra
        frame has run).  The schedule that ran is left in `self.last_refill_trace`: (utterance, row, first_step, frames).
        rows (extension): None - min(infer_batch_rows, 16) rows per decoder pass, as ever; an int in 1 .. 64 - the group size
        (refill=False) or the row count of the shared cache (refill=True) of THIS call.  Above 16 the decoder runs the wide step
        (kalle_llama_decode_step_wide: up to 64 utterances share one read of the weights; bf16 weights only - with
        quantize_decoder("e4m3") it is a NotImplementedError) and the device head runs once per 16 rows; an utterance's result
        under explicit noise is, bit for bit, what groups of 16 give."""
        return generate_batch(self, prompts, end_disp_kl_thres, max_length, device_head, noise, stop_lag,
                              self.distribution_linear[2].weight.shape[0], refill=refill, rows=rows)

    def _host_frame(self, hidden):
        """the head of one frame on the host for the rows of hidden [R, 1, D]: (what `infer_batch` stacks, the sampled latent
        [R, 1, d] - here the same tensor - and kl [R, 1]).  `std` is read only after distribution_linear is
        enqueued: on a model built on the device that read is a host wait, and the device would idle under the launches."""
        mean2 = self.distribution_linear(hidden.contiguous())                    # [R, 1, d]: every row at once
        audio_latent = self.sample(mean2)
        # KL(N(m, s) || N(1, e)) = log(e/s) + (s^2 + (m-1)^2) / (2 e^2) - 1/2, summed over the latent dim / dim
        s, e = float(self.std), float(torch.e)
        kl =(torch.log(torch.tensor(e / s)) + (s * s + (mean2.float() - 1.0) ** 2) / (2 * e * e) - 0.5).sum(2)
        return audio_latent, audio_latent, kl / mean2.shape[2]

    def _generate_device_head(self, prompts, thres, max_length, noise, stop_lag, refill=False, rows=None):
        """generation.generate with the fixed-std head (ops.llasa_frame_head); returns the sampled latents"""
        dl = self.distribution_linear[2].weight.shape[0]
        device_head_limits(stop_lag, dl, ops.HEAD_MAX_LATENT)
        std = self.std
        if not (isinstance(std, (int, float)) or (torch.is_tensor(std) and std.numel() == 1)) or not float(std) > 0:
            raise NotImplementedError("device_head=True takes the fixed scalar std of init_sigmaVAE; any other std runs on the "
                                      "host path (device_head=False)")
        spec = DeviceHeadSpec(ops.llasa_head_plan, ops.llasa_frame_head, (float(std),), "latent", dl)
        return generate(self, prompts, thres, max_length, spec, noise, stop_lag, refill, rows=rows)

    def init_sigmaVAE(self):
        self.std = torch.tensor(0.5)

    def sample(self, mean, dist_type='fix', noise=None):
        """model_sigmaVAE.py:153-178"""
        if dist_type == 'fix':
            n = torch.randn_like(mean, dtype=F32) if noise is None else noise.to(F32)
            return ops.axpby(mean.to(F32), n, 1.0, float(self.std))
        if dist_type == 'gaussian':
            value = float(self.std) / 0.8
            std = torch.randn(mean.size(0), device=mean.device, dtype=F32) * value
            while std.dim() < mean.dim():
                std = std.unsqueeze(-1)
            return mean + std * torch.randn_like(mean)
        return mean

    def kl(self, mean):
        """model_sigmaVAE.py:180-183: squared distance to zero"""
        return mean * mean


def sample(mean, dist_type='fix'):
    """module-level twin of Llasa.sample (model_sigmaVAE.py:187-215)"""
    if dist_type == 'fix':
        return ops.axpby(mean.to(F32), torch.randn_like(mean, dtype=F32), 1.0, 0.5)
    if dist_type == 'gaussian':
        std = torch.randn(mean.size(0), device=mean.device, dtype=mean.dtype) * (0.5 / 0.8)
        while std.dim() < mean.dim():
            std = std.unsqueeze(-1)
        return mean + std * torch.randn_like(mean)
    return mean
