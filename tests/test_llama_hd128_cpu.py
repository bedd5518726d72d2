"""CPU: the head-dim-128 Llama path without a GPU - the oracle against the reference's fixture (tests/golden/llasa_hd128.npz, made
by tests/golden/make_golden_llama_hd128.py), construction / state-dict layout / refusals of the drop-in classes, the C header's
new entry points, the fp64 kernel references at dh = rot = 128 against torch's SDPA, and the ambiguity cap of
tests/test_llama_hd128_gpu.py on the stage-1 inputs of its decode-step cases."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import decode_cases as dc  # noqa: E402
import golden_util as gu  # noqa: E402
import kalle_oracle as ko  # noqa: E402
import kernel_refs as kr  # noqa: E402
import llama_hd128_cases as lc128  # noqa: E402

G = os.path.join(HERE, "golden")
HEADER = os.path.join(HERE, "..", "include", "kalle_hip.h")


def _inventory():
    return json.load(open(os.path.join(G, "state_dict_keys_llama_hd128.json")))["llasa"]


def _close(a, b, tol):
    a = a.detach().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = ((a - b).norm() / (b.norm() + 1e-30)).item()
    assert err < tol, err


# ------------------------------------------------------------------------------------------------ oracle against the fixture
def test_oracle_matches_reference_at_head_dim_128():
    """ko.llasa_forward against the reference run: the tolerances of tests/test_oracle_golden.py::test_llasa (the four full
    gradients are stored as float16 of grad * gradscale: 1e-3 there, the format's precision)"""
    f = np.load(os.path.join(G, "llasa_hd128.npz"))
    lc = lc128.llasa_config()
    shapes = [(k, tuple(v)) for k, v in _inventory().items() if k != "base_model.lm_head.weight"]
    sd = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in gu.make_state(shapes, lc128.SEED).items()}
    batch = {k: torch.from_numpy(v) for k, v in gu.llasa_batch(lc, lc128.SEED, B=3, L=40).items()}
    eps = torch.from_numpy(gu.make_input("llasa_eps", tuple(batch["audio_latents"].shape), lc128.SEED))
    out = ko.llasa_forward(sd, lc, batch, eps)
    _close(out["audio_loss"], f["audio_loss"], 1e-5)
    _close(out["end_loss"], f["end_loss"], 1e-5)
    _close(out["pre_mean"], f["pre_mean"], 1e-5)
    _close(out["ground_truth_audio_latents"], f["sampled"], 3e-6)
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    n = full = 0
    for k in f.files:
        if k.startswith("digest/"):
            got, ref = gu.digest(sd[k[7:]].grad.numpy()), f[k]
            assert np.all(np.abs(got - ref) <= 5e-5 * max(abs(ref[0]), 1e-12) + 1e-7), (k, got[:3], ref[:3])
            n += 1
        if k.startswith("grad/"):
            _close(sd[k[5:]].grad, f[k].astype(np.float64) / float(f["gradscale/" + k[5:]]), 1e-3)
            full += 1
    assert n == len(shapes) and full == 4, (n, full)


# ------------------------------------------------------------------------------------------------ construction
def _causal_lm(**over):
    from kalle_audio_amd.model_sigmaVAE import LlamaForCausalLM
    return LlamaForCausalLM(dict(lc128.llasa_config()["llama"], **over))


def test_head_dim_128_llama_constructs_with_the_reference_state_dict_layout():
    """fails on a tree whose LlamaAttention accepts head_dim 64 only"""
    m = _causal_lm()
    inv = _inventory()
    want = {k[len("base_model."):]: tuple(v) for k, v in inv.items() if k.startswith("base_model.")}
    want["model.embed_tokens.weight"] = want["lm_head.weight"] = (300, 256)     # (before resize_token_embeddings(310))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    a = m.model.layers[0].self_attn
    assert (a.num_heads, a.num_kv_heads, a.head_dim) == (2, 1, 128)
    assert a.qkv_proj.weight.shape == (2 * 128 + 2 * 128, 256) and a.o_proj.weight.shape == (256, 256)
    # the split q / k / v and up / gate names round-trip through the fused parameters
    sd = {k: torch.randn(v.shape) for k, v in m.state_dict().items()}
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    p = "model.layers.1."
    assert torch.equal(m.model.layers[1].self_attn.qkv_proj.weight,
                       torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0))
    assert torch.equal(m.model.layers[1].mlp.up_gate_proj.weight, torch.cat([sd[p + "mlp.up_proj.weight"], sd[p + "mlp.gate_proj.weight"]], 0))
    cache = m.model.init_cache(9, "cpu")
    assert [tuple(t.shape) for t in cache["kv"]] == [(9, 2 * 1 * 128)] * 2
    assert tuple(cache["rope"][0].shape) == (9, 64)


def test_head_dim_64_llama_still_constructs():
    from kalle_audio_amd.model_sigmaVAE import LlamaForCausalLM
    m = LlamaForCausalLM(dict(gu.LLASA_CONFIG["llama"]))
    assert m.model.layers[0].self_attn.head_dim == 64 and m.model.init_cache(5, "cpu")["kv"][0].shape == (5, 128)


@pytest.mark.parametrize("over", [dict(head_dim=96, hidden_size=192), dict(hidden_size=320), dict(attention_bias=True)],
                         ids=["head_dim-96", "hidden-320-with-2-heads-of-128", "attention_bias"])
def test_unsupported_llama_layouts_are_refused_by_name(over):
    with pytest.raises(NotImplementedError, match=r"\(64, 128\)"):
        _causal_lm(**over)


def test_llasa_classes_load_a_head_dim_128_config(tmp_path):
    """model_sigmaVAE.Llasa and model.Llasa share the Llama classes: both construct over a head-dim-128 config.json"""
    from kalle_audio_amd import model as km
    from kalle_audio_amd import model_sigmaVAE as ks
    lc = lc128.llasa_config()
    (tmp_path / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))

    class Tok:
        def __len__(self):
            return lc["tokenizer_len"]

    cfg = {"llm_model_name_or_path": str(tmp_path), "latent_dim": lc["latent_dim"], "audio_proj_dim": 256}
    for cls in (ks.Llasa, km.Llasa):
        m = cls(cfg, Tok(), use_flash_attention=False)
        assert m.base_model.model.layers[1].self_attn.head_dim == 128
    got = {k: list(v.shape) for k, v in ks.Llasa(cfg, Tok(), use_flash_attention=False).state_dict().items()}
    assert got == _inventory()


# ------------------------------------------------------------------------------------------------ header
def _proto_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, name + " is not declared"
    return [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]


def test_header_declares_the_head_dim_entry_points():
    """fails on a tree without them"""
    assert _proto_args("kalle_attention_decode_hd") == [
        "q", "ldq", "q_off", "k", "ldk", "k_off", "v", "ldv", "v_off", "out", "ldo", "lse", "rope_cos", "rope_sin", "rot", "key_mask",
        "B", "H", "Hkv", "Nk", "head_dim", "stream"]
    assert _proto_args("kalle_llama_decode_ws_bytes_hd") == ["H", "Hkv", "inner", "head_dim"]
    assert _proto_args("kalle_llama_decode_step_hd") == [
        "layers", "n_layers", "x", "out", "H", "Hkv", "inner", "head_dim", "eps", "t0", "cache_rows", "rope_cos", "rope_sin",
        "workspace", "stream"]
    assert _proto_args("kalle_llama_decode_ws_bytes") == ["H", "Hkv", "inner"]
    assert _proto_args("kalle_llama_decode_step") == [
        "layers", "n_layers", "x", "out", "H", "Hkv", "inner", "eps", "t0", "cache_rows", "rope_cos", "rope_sin", "workspace", "stream"]
    from kalle_audio_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["kalle_attention_decode_hd"][1]) == 22 and len(protos["kalle_llama_decode_step_hd"][1]) == 15


# ------------------------------------------------------------------------------------------------ references at dh = rot = 128
def _hf_rotate(x, cos, sin):
    """transformers' apply_rotary_pos_emb: x cos + rotate_half(x) sin with cos / sin repeated over both halves of the head"""
    c, s = torch.cat([cos, cos], -1), torch.cat([sin, sin], -1)
    x1, x2 = x[..., :64], x[..., 64:]
    return x * c + torch.cat([-x2, x1], -1) * s


@pytest.mark.parametrize("Nq", [1, 5])
def test_attention_ref_at_rot_128_is_sdpa_over_hf_rotated_heads(Nq):
    g = torch.Generator().manual_seed(Nq)
    H, Hkv, Nk, Bn = 4, 1, 9, 2
    q = torch.randn(Bn, Nq, H * 128, generator=g, dtype=torch.float64)
    k = torch.randn(Bn, Nk, Hkv * 128, generator=g, dtype=torch.float64)
    v = torch.randn(Bn, Nk, Hkv * 128, generator=g, dtype=torch.float64)
    cos, sin = (t.double() for t in lc128.rope_tables(Nk))
    out, lse, p, qh, kh = kr.attention_ref(q, k, v, H, Hkv, 128, rot=128, cos=cos, sin=sin, causal=True)
    qr = _hf_rotate(q.reshape(Bn, Nq, H, 128).transpose(1, 2), cos[Nk - Nq:], sin[Nk - Nq:])
    kr_ = _hf_rotate(k.reshape(Bn, Nk, Hkv, 128).transpose(1, 2), cos, sin)
    vh = v.reshape(Bn, Nk, Hkv, 128).transpose(1, 2)
    allow = torch.arange(Nk)[None, :] <= torch.arange(Nq)[:, None] + (Nk - Nq)
    ref = F.scaled_dot_product_attention(qr, kr_.repeat_interleave(4, 1), vh.repeat_interleave(4, 1), attn_mask=allow)
    err = (out.reshape(Bn, Nq, H, 128).transpose(1, 2) - ref).abs().max().item()
    assert err < 1e-12, err
    assert (qh - qr).abs().max() < 1e-12 and (kh - kr_).abs().max() < 1e-12


def test_unrotate_is_the_transpose_of_rotate_at_rot_128():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 128, generator=g, dtype=torch.float64)
    y = torch.randn(3, 7, 128, generator=g, dtype=torch.float64)
    cos, sin = (t.double() for t in lc128.rope_tables(20))
    pos = torch.arange(7) + 11
    lhs = (kr._rotate(x, cos, sin, 128, pos) * y).sum()
    rhs = (x * kr._unrotate(y, cos, sin, 128, pos)).sum()
    assert abs(lhs - rhs).item() < 1e-10


# ------------------------------------------------------------------------------------------------ ambiguity cap
@pytest.mark.parametrize("name", list(lc128.STEP_CASES))
def test_ambiguity_cap_on_the_stage_1_inputs_of_every_gpu_case(name):
    """the rule of tests/test_decode_refs_cpu.py: at most 1 % of the K elements of the stage-1 prologue value lie within the
    prologue's fast-math window of a bf16 rounding boundary"""
    c = lc128.STEP_CASES[name]
    x, gamma = lc128.stage1_inputs(c)
    xh = kr.decode_rms_prologue(x.double(), gamma.double(), lc128.EPS)
    amb = kr.bf16_ambiguous(xh, dc.rms_window(xh))
    assert amb.sum().item() <= 0.01 * xh.numel(), (name, amb.sum().item(), xh.numel())
