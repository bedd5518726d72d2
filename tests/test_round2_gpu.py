"""-m gpu, round 2: the HIP path against the round-2 reference fixtures (tests/golden/make_golden_r02.py) - the benchmark's
width, 375-frame sequences, the wide Llasa, model.py's Llasa, DiffusionCondTrainingWrapper.training_step, the end-to-end
generation with int16 export, the batched chunk pipeline - plus the communication path on real hardware and the trainer
surfaces round 1 left untested (FusedAdam, comm_dtype, state_dict, a second consumer of block outputs / of the context).
Tolerances as tests/test_modules_gpu.py: bf16 operands vs fp32 reference rel-L2 <= 1e-2 block outputs, <= 2e-2 gradients,
cosine >= 0.999 whole-model outputs; fp32 conv path <= 1e-4."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import golden_util as gu  # noqa: E402
import kalle_oracle as ko  # noqa: E402
from test_modules_gpu import T, _hf_grads, _Tok, cosine, fx, load_seeded, rel  # noqa: E402

G = os.path.join(HERE, "golden")
D, DC, CIO, GD = 128, 64, 16, 32


def check_digests(f, grads, n, prefix="", tol=2e-2, strip="", skip=()):
    """gradient digests: l2 norm within tol, the n sampled entries within tol of the tensor's rms scale (+ 25 % relative)"""
    cnt = 0
    for k in f.files:
        if not k.startswith(prefix + "digest/"):
            continue
        name = k[len(prefix) + 7:]
        if name in skip:
            continue
        name = name[len(strip):] if strip and name.startswith(strip) else name
        g = grads[name].detach().float().cpu().numpy()
        got, ref = gu.digest(g, n), f[k]
        assert abs(got[0] - ref[0]) <= tol * ref[0] + 1e-6, (name, got[0], ref[0])
        scale = ref[0] / np.sqrt(max(g.size, 1))
        assert np.all(np.abs(got[2:] - ref[2:]) <= 0.25 * np.abs(ref[2:]) + 6 * tol * scale + 1e-6), (name, got[2:6], ref[2:6])
        cnt += 1
    assert cnt > 0
    return cnt


@pytest.fixture(scope="module", autouse=True)
def _drop_in_installed():
    """`stable_audio_tools` / `model` / `flows` resolve to the drop-in for every test of this module, whatever subset runs"""
    import kalle_audio_amd
    kalle_audio_amd.install()


@pytest.fixture(scope="module")
def mods(dev):
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models import transformer as T_
    return T_


# ------------------------------------------------------------------------------------------------ bench width / long T
@pytest.mark.parametrize("name,ada,seed", [("block_wide_plain", False, 50), ("block_wide_adaln", True, 51)])
def test_transformer_block_bench_width(mods, dev, name, ada, seed):
    """D = 1536, 24 heads, context 768 (12 kv heads), 126 tokens, 130 context tokens: every head / kv-head offset, the 256-wide
    GEMM tiles where the shape allows them, a second key block of 2 context tokens"""
    f = fx(name)
    w = gu.WIDE_BLOCK
    Dw, DCw, Nw, Sw, Bw = w["D"], w["DC"], w["N"], w["S"], w["B"]
    x = T(gu.make_input("x", (Bw, Nw, Dw), seed), dev, True)
    ctx = T(gu.make_input("ctx", (Bw, Sw, DCw), seed), dev, True)
    dy = T(gu.make_input("dy", (Bw, Nw, Dw), seed), dev)
    blk = load_seeded(mods.TransformerBlock(Dw, dim_heads=64, cross_attend=True, dim_context=DCw,
                                            global_cond_dim=Dw if ada else None), seed, dev)
    rot = mods.RotaryEmbedding(32).to(dev)
    kw = {}
    if ada:
        gc = T(gu.make_input("g", (Bw, Dw), seed), dev, True)
        kw["global_cond"] = gc
    y = blk(x, context=ctx, rotary_pos_emb=rot.forward_from_seq_len(Nw), **kw)
    y.backward(dy)
    assert rel(y, f["y"].astype(np.float32)) < 1e-2, rel(y, f["y"].astype(np.float32))
    assert rel(x.grad, f["dx"].astype(np.float32)) < 2e-2, rel(x.grad, f["dx"].astype(np.float32))
    assert rel(ctx.grad, f["dctx"].astype(np.float32)) < 2e-2, rel(ctx.grad, f["dctx"].astype(np.float32))
    if ada:
        assert rel(gc.grad, f["dg"].astype(np.float32)) < 2e-2, rel(gc.grad, f["dg"].astype(np.float32))
    check_digests(f, {n: p.grad for n, p in blk.named_parameters()}, 64)


@pytest.mark.parametrize("kind,ada,seed", [("l2", False, 70), ("ln", True, 71)])
def test_transformer_block_qk_norm(mods, dev, kind, ada, seed):
    """Attention(qk_norm="l2" | "ln") (transformer.py:303-307, 422-428): kalle_head_norm_fwd / _bwd on the q and k slices of the
    projection outputs, self-attention and GQA cross-attention with a ragged context mask, "ln" on an adaLN block; outputs
    and input gradients within 1e-2 / 2e-2 of the reference (bf16 GEMM path), the LayerNorm(64) gradients within 3e-2"""
    f = fx("block_qk_norm")
    q = gu.QK_NORM_BLOCK
    Dq, DCq, Nq, Sq, Bq = q["D"], q["DC"], q["N"], q["S"], q["B"]
    x = T(gu.make_input("x", (Bq, Nq, Dq), seed), dev, True)
    ctx = T(gu.make_input("ctx", (Bq, Sq, DCq), seed), dev, True)
    dy = T(gu.make_input("dy", (Bq, Nq, Dq), seed), dev)
    cmask = (torch.arange(Sq)[None, :] < torch.tensor([Sq, Sq - 7])[:, None]).to(dev)
    blk = load_seeded(mods.TransformerBlock(Dq, dim_heads=64, cross_attend=True, dim_context=DCq,
                                            global_cond_dim=Dq if ada else None, attn_kwargs={"qk_norm": kind}), seed, dev)
    rot = mods.RotaryEmbedding(32).to(dev)
    kw = {}
    if ada:
        gc = T(gu.make_input("g", (Bq, Dq), seed), dev, True)
        kw["global_cond"] = gc
    y = blk(x, context=ctx, context_mask=cmask, rotary_pos_emb=rot.forward_from_seq_len(Nq), **kw)
    y.backward(dy)
    assert rel(y, f[f"{kind}/y"]) < 1e-2, rel(y, f[f"{kind}/y"])
    assert rel(x.grad, f[f"{kind}/dx"]) < 2e-2, rel(x.grad, f[f"{kind}/dx"])
    assert rel(ctx.grad, f[f"{kind}/dctx"]) < 2e-2, rel(ctx.grad, f[f"{kind}/dctx"])
    if ada:
        assert rel(gc.grad, f[f"{kind}/dg"]) < 2e-2, rel(gc.grad, f[f"{kind}/dg"])
    g = {n: p.grad for n, p in blk.named_parameters()}
    assert all(v is not None for v in g.values()), [n for n, v in g.items() if v is None]
    zero = "cross_attn.k_norm.bias"       # mathematically zero (a constant added to every key of an un-rotated attention)
    check_digests(f, g, 32, prefix=f"{kind}/", skip=(zero,))
    for k in f.files:
        if k.startswith(f"{kind}/grad/"):
            name = k[len(kind) + 6:]
            if name == zero:
                assert g[name].abs().max().item() < 0.05 * g["cross_attn.q_norm.bias"].abs().max().item()
            else:
                assert rel(g[name], f[k]) < 3e-2, (name, rel(g[name], f[k]))
    # the stand-alone Attention module (its own autograd node) against the oracle
    att = load_seeded(mods.Attention(Dq, dim_heads=64, qk_norm=kind), seed + 5, dev)
    sd = {k_: torch.from_numpy(v) for k_, v in gu.make_state(
        [(n, tuple(p.shape)) for n, p in att.named_parameters()], seed + 5).items()}
    xa = torch.from_numpy(gu.make_input("xa", (Bq, Nq, Dq), seed))
    xr = xa.clone().requires_grad_(True)
    for v in sd.values():
        v.requires_grad_(True)
    ref = ko.attention(sd, xr, rotary=ko.rotary_freqs(Nq), qk_l2=kind == "l2")
    ref.backward(torch.from_numpy(gu.make_input("dy", (Bq, Nq, Dq), seed)))
    xg = xa.to(dev).requires_grad_(True)
    out = att(xg, rotary_pos_emb=rot.forward_from_seq_len(Nq))
    out.backward(dy)
    assert rel(out, ref) < 1e-2 and rel(xg.grad, xr.grad) < 2e-2, (rel(out, ref), rel(xg.grad, xr.grad))
    for n, p in att.named_parameters():
        assert rel(p.grad, sd[n].grad) < 3e-2, (n, rel(p.grad, sd[n].grad))


def test_transformer_block_bench_width_batched_rows(mods, dev):
    """the same block at B = 3 (378 rows: the 256-row GEMM tiles with a ragged last tile) against the CPU oracle"""
    w = gu.WIDE_BLOCK
    Dw, DCw, Nw, Sw, seed, Bq = w["D"], w["DC"], w["N"], w["S"], 57, 3
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(ko.block_shapes(Dw, dim_context=DCw), seed).items()}
    blk = load_seeded(mods.TransformerBlock(Dw, dim_heads=64, cross_attend=True, dim_context=DCw), seed, dev)
    x = torch.from_numpy(gu.make_input("x", (Bq, Nw, Dw), seed))
    ctx = torch.from_numpy(gu.make_input("ctx", (Bq, Sw, DCw), seed))
    ref = ko.transformer_block(sd, x, context=ctx, rotary=ko.rotary_freqs(Nw))
    rot = mods.RotaryEmbedding(32).to(dev)
    with torch.no_grad():
        y = blk(x.to(dev), context=ctx.to(dev), rotary_pos_emb=rot.forward_from_seq_len(Nw))
    assert rel(y, ref) < 1e-2, rel(y, ref)


def test_dit_long_sequence(mods, dev):
    """375 frames + 1 prepended token and 130 context tokens (30 s clips of configs/twj_0828.yaml): three key blocks in the
    self-attention's online softmax, two in the cross-attention"""
    from stable_audio_tools.models.dit import DiffusionTransformer
    from kalle_audio_amd import functional as KF
    from kalle_audio_amd import ops
    f = fx("dit_long")
    Bl, Nl, Sl, seed = 2, 375, 130, 52
    dit = load_seeded(DiffusionTransformer(io_channels=CIO, embed_dim=D, depth=2, num_heads=2, cond_token_dim=DC,
                                           project_cond_tokens=False, global_cond_dim=GD,
                                           transformer_type="continuous_transformer", global_cond_type="prepend"), seed, dev)
    lat = T(gu.make_input("lat", (Bl, CIO, Nl), seed), dev)
    noise = T(gu.make_input("noise", (Bl, CIO, Nl), seed), dev)
    tt = T(np.array([0.2, 0.65], dtype=np.float32), dev)
    ctx = T(gu.make_input("ctx", (Bl, Sl, DC), seed), dev)
    gl = T(gu.make_input("glob", (Bl, GD), seed), dev)
    pm = T(gu.make_mask("pm", (Bl, Nl), seed, 0.7), dev)
    xt, tgt = ops.diffuse_fwd(lat, noise, tt, "v")
    out = dit(xt, tt, cross_attn_cond=ctx, global_embed=gl, cfg_dropout_prob=0.0)
    assert cosine(out, f["output"]) > 0.999 and rel(out, f["output"]) < 2e-2, rel(out, f["output"])
    loss = KF.MSELossFn.apply(out, tgt, None, 1.0)
    lm = KF.MSELossFn.apply(out.detach(), tgt, pm, 1.0)
    assert abs(loss.item() - float(f["loss"])) < 1e-2 * float(f["loss"])
    assert abs(lm.item() - float(f["loss_masked"])) < 1e-2 * float(f["loss_masked"])
    loss.backward()
    check_digests(f, {n: p.grad for n, p in dit.named_parameters()}, 16, tol=3e-2)
    with torch.no_grad():
        o = dit(xt, tt, cross_attn_cond=ctx, global_embed=gl, cfg_scale=2.5)
    assert cosine(o, f["output_cfg"]) > 0.999


# ------------------------------------------------------------------------------------------------ Llasa (both task models)
def _llasa_wide(dev, tmp_path):
    from kalle_audio_amd.model_sigmaVAE import Llasa
    from test_oracle_golden import llasa_wide_shapes
    lc = gu.LLASA_WIDE_CONFIG
    d = tmp_path / "llama_wide"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": lc["latent_dim"],
               "audio_proj_dim": lc["llama"]["hidden_size"]}, _Tok(lc["tokenizer_len"]), use_flash_attention=False)
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(llasa_wide_shapes(), 53).items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to(dev), lc


def test_llasa_wide_ragged(dev, tmp_path):
    """model_sigmaVAE.Llasa at 4 heads / 2 kv heads, three sequences of 300 with ragged right padding (llama3 rope scaling on)"""
    m, lc = _llasa_wide(dev, tmp_path)
    f = fx("llasa_wide")
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch_long(lc, 53).items()}
    eps = T(gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), 53), dev)
    out = m(b["input_ids"], b["audio_latents"], b["audio_distribution_l"], b["ids_mask"], b["audio_mask"],
            b["target_mask"], b["end_mask"], noise=eps)
    assert abs(out["audio_loss"].item() - float(f["audio_loss"])) < 1e-2 * float(f["audio_loss"])
    assert abs(out["end_loss"].item() - float(f["end_loss"])) < 1e-2 * float(f["end_loss"])
    valid = (b["ids_mask"] + b["audio_mask"]) > 0
    ref = torch.from_numpy(f["pre_mean"].astype(np.float32)).to(dev)
    assert rel(out["pre_mean"][valid], ref[valid]) < 1e-2, rel(out["pre_mean"][valid], ref[valid])
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = _hf_grads(m)
    assert check_digests(f, g, 16) == 26
    for k in f.files:
        if k.startswith("grad/"):
            assert rel(g[k[5:]], f[k]) < 2e-2, (k, rel(g[k[5:]], f[k]))


def _model_llasa(dev, tmp_path):
    import kalle_audio_amd
    kalle_audio_amd.install()
    from model import Llasa                                   # train.py:24's import line, served by install()
    lc = gu.LLASA_CONFIG
    d = tmp_path / "llama_m"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": lc["latent_dim"], "audio_proj_dim": 128},
              _Tok(lc["tokenizer_len"]), use_flash_attention=False)
    inv = json.load(open(os.path.join(G, "state_dict_keys_r02.json")))["model_llasa"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == inv          # the reference class's keys and shapes
    shapes = [(k, tuple(v)) for k, v in inv.items() if k != "base_model.lm_head.weight"]
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(shapes, 54).items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to(dev), lc


@pytest.mark.parametrize("inject", [False, True])
def test_model_llasa_two_gaussian_kl(dev, tmp_path, inject):
    """model.py's Llasa (train.py / train_melvae.py): two-Gaussian KL kernel with the label transform fused (default) or
    supplied by the caller (the injection point for the reference's missing twj_utils function)"""
    import kalle_audio_amd.model as KM
    m, lc = _model_llasa(dev, tmp_path)
    f = fx("model_llasa")
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch_long(lc, 54, B=3, L=48, label_mult=2).items()}
    KM.get_mean_stdev_from_stableaudio2_latents = gu.default_mean_stdev if inject else None
    try:
        out = m(b["input_ids"], b["audio_latents"], b["audio_distribution_l"], b["ids_mask"], b["audio_mask"],
                b["target_mask"], b["end_mask"])
    finally:
        KM.get_mean_stdev_from_stableaudio2_latents = None
    assert set(out) == {"audio_loss", "end_loss", "pre_mean", "pre_log_scale"}
    assert abs(out["audio_loss"].item() - float(f["audio_loss"])) < 1e-2 * abs(float(f["audio_loss"]))
    assert abs(out["end_loss"].item() - float(f["end_loss"])) < 1e-2 * abs(float(f["end_loss"]))
    valid = (b["ids_mask"] + b["audio_mask"]) > 0
    for key in ("pre_mean", "pre_log_scale"):
        ref = torch.from_numpy(f[key]).to(dev)
        assert rel(out[key][valid], ref[valid]) < 1e-2, (key, rel(out[key][valid], ref[valid]))
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = _hf_grads(m)
    check_digests(f, g, 16)
    for k in f.files:
        if k.startswith("grad/"):
            assert rel(g[k[5:]], f[k]) < 2e-2, (k, rel(g[k[5:]], f[k]))


def test_gauss_kl2_kernel_vs_torch_distributions(dev):
    """the KL kernel alone (fp32) against torch.distributions on the same numbers, forward and backward, both label modes"""
    import torch.distributions as Dn
    from kalle_audio_amd import ops
    torch.manual_seed(5)
    rows, d = 37, 24
    pred = torch.randn(rows, 2 * d, device=dev)
    label = torch.randn(rows, 2 * d, device=dev)
    ma = (torch.rand(rows, device=dev) < 0.6).float()
    mb = (torch.rand(rows, device=dev) < 0.2).float()
    mb[0] = 1.0
    m1, s1 = gu.default_mean_stdev(label.view(1, rows, 2 * d).transpose(1, 2))
    m1, s1 = m1.transpose(1, 2)[0].contiguous(), s1.transpose(1, 2)[0].contiguous()
    p = pred.clone().requires_grad_(True)
    kl = Dn.kl_divergence(Dn.Normal(m1, s1 * 1.25), Dn.Normal(p[:, :d], torch.exp(p[:, d:]))).sum(1) / d
    la, lb = (kl * ma).sum() / ma.sum(), (kl * mb).sum() / mb.sum()
    (0.7 * la + 1.3 * lb).backward()
    ga, gb = torch.tensor([0.7], device=dev), torch.tensor([1.3], device=dev)
    for lm, ls in ((label, None), (m1, s1)):
        sums = ops.gauss_kl2_fwd(pred, lm, ls, ma, mb)
        assert abs((sums[0] / sums[1]).item() - la.item()) < 1e-5 * abs(la.item())
        assert abs((sums[2] / sums[3]).item() - lb.item()) < 1e-5 * abs(lb.item())
        dp = ops.gauss_kl2_bwd(pred, lm, ls, ma, mb, sums, ga, gb)
        assert rel(dp, p.grad) < 1e-5, rel(dp, p.grad)


def test_model_llasa_infer_kv_cache_and_long_decode(dev, tmp_path):
    """model.Llasa.infer: with / without the KV cache the same frames for the same noise; and a 60 s decode (750 frames at
    12.5 Hz, the VibeVoice-path length) runs through the cached path"""
    m, lc = _model_llasa(dev, tmp_path)
    lat = lc["latent_dim"]
    ids = torch.randint(0, 300, (9,), device=dev)
    prompt = torch.randn(1, 5, lat, device=dev)
    outs = []
    for use_cache in (True, False):
        torch.manual_seed(11)
        outs.append(m.infer(ids, prompt, end_disp_kl_thres=-1.0, max_length=8, use_cache=use_cache))
    assert outs[0].shape == outs[1].shape == (1, 2 * lat, 7)
    assert rel(outs[0], outs[1]) < 3e-2, rel(outs[0], outs[1])
    torch.manual_seed(12)
    long = m.infer(ids, prompt, end_disp_kl_thres=-1.0, max_length=751)
    assert long.shape == (1, 2 * lat, 750) and torch.isfinite(long).all()


# ------------------------------------------------------------------------------------------------ wrappers end to end
class TensorConditioner(torch.nn.Module):
    """the test's conditioner (same as the fixture generator's): metadata already holds the conditioning tensors"""

    def forward(self, metadata, device):
        ctx = torch.stack([md["prompt"] for md in metadata]).to(device)
        cm = torch.stack([md["prompt_mask"] for md in metadata]).to(device)
        gl = torch.stack([md["g"] for md in metadata]).to(device)
        return {"prompt": (ctx, cm), "g": (gl, None)}


def _cond_model(dev, io_channels, objective, seed):
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models import diffusion as KD
    from stable_audio_tools.models.factory import create_model_from_config
    from stable_audio_tools.models.pretransforms import AutoencoderPretransform
    e = gu.E2E
    dit = KD.DiTWrapper(io_channels=io_channels, embed_dim=e["D"], depth=2, num_heads=2, cond_token_dim=e["DC"],
                        project_cond_tokens=False, global_cond_dim=e["G"], transformer_type="continuous_transformer",
                        global_cond_type="prepend")
    load_seeded(dit, seed, dev)
    ae = load_seeded(create_model_from_config(gu.oobleck_cfg(True)), 23, dev)
    pt = AutoencoderPretransform(ae, scale=0.8)
    return KD.ConditionedDiffusionModelWrapper(dit, TensorConditioner(), io_channels=io_channels, sample_rate=16000,
                                               min_input_length=40, diffusion_objective=objective, pretransform=pt,
                                               cross_attn_cond_ids=["prompt"], global_cond_ids=["g"]).to(dev)


def _e2e_cond(seed, dev):
    e = gu.E2E
    return (T(gu.make_input("ctx", (e["B"], e["S"], e["DC"]), seed), dev), T(gu.make_mask("cm", (e["B"], e["S"]), seed), dev),
            T(gu.make_input("glob", (e["B"], e["G"]), seed), dev))


def test_generate_diffusion_cond_end_to_end(dev):
    """seed -> noise -> 4-step CFG sampler -> Oobleck decode -> int16 against the reference's generate_diffusion_cond on the
    same seed (generation.py:138-142: the CPU draw is bit-identical; the reference on a GPU draws with the same torch call)"""
    from stable_audio_tools.inference.generation import generate_diffusion_cond
    from kalle_audio_amd import ops
    f = fx("generate_e2e")
    e = gu.E2E
    ctx, cm, gl = _e2e_cond(60, dev)
    cond = {"prompt": (ctx, cm), "g": (gl, None)}
    neg = {"prompt": (ctx.flip(0), cm.flip(0)), "g": (gl, None)}
    kw = dict(steps=e["steps"], cfg_scale=e["cfg_scale"], conditioning_tensors=cond, batch_size=e["B"],
              sample_size=40 * e["T"], seed=e["seed"], device="cpu")
    model = _cond_model(dev, 4, "rectified_flow", 60)
    lat = generate_diffusion_cond(model, return_latents=True, **kw)
    assert cosine(lat, f["rf/latents"]) > 0.999, cosine(lat, f["rf/latents"])
    audio = model.generate(**kw)                                              # ConditionedDiffusionModelWrapper.generate
    assert audio.shape == (e["B"], 2, 40 * e["T"])
    assert cosine(audio, f["rf/audio"]) > 0.999, cosine(audio, f["rf/audio"])
    # the int16 export of infer_0723.py:292-293 ("b d n -> d (b n)", peak-normalise): kernel vs the reference's own bytes
    flat = audio.permute(1, 0, 2).reshape(2, -1).contiguous()
    i16, peak = ops.peak_normalize_int16(flat)
    want = f["rf/int16"].astype(np.float32)
    got = i16.cpu().numpy().astype(np.float32)
    assert got.shape == want.shape
    assert (got * want).sum() / (np.linalg.norm(got) * np.linalg.norm(want)) > 0.999
    assert abs(np.abs(got).max() - 32767) <= 1
    # decode alone on the reference's latents: the conv path is fp32, so the waveform must match tightly
    dec = model.pretransform.decode(T(f["rf/latents"], dev))
    assert rel(dec, f["rf/audio"]) < 1e-4, rel(dec, f["rf/audio"])
    i16b, _ = ops.peak_normalize_int16(dec.permute(1, 0, 2).reshape(2, -1).contiguous())
    assert np.abs(i16b.cpu().numpy().astype(np.int32) - f["rf/int16"].astype(np.int32)).max() <= 3
    audio_neg = generate_diffusion_cond(model, negative_conditioning_tensors=neg, **kw)
    assert cosine(audio_neg, f["rf_neg/audio"]) > 0.999
    model = _cond_model(dev, 4, "v", 61)
    lat = generate_diffusion_cond(model, return_latents=True, **kw)
    assert cosine(lat, f["v/latents"]) > 0.998, cosine(lat, f["v/latents"])
    audio = generate_diffusion_cond(model, **kw)
    assert cosine(audio, f["v/audio"]) > 0.998, cosine(audio, f["v/audio"])
    # a frozen model samples through one HIP-graph replay per step (kalle_audio_amd/graph.py): same bits as the eager launches,
    # also on the second call (replay of the cached graph with new inputs)
    model.requires_grad_(False)
    for _ in range(2):
        lat_g = generate_diffusion_cond(model, return_latents=True, **kw)
        assert getattr(model, "_kalle_graphed", None) is not None
        assert torch.equal(lat_g, lat)
    lat_s = generate_diffusion_cond(model, return_latents=True, **dict(kw, seed=e["seed"] + 1))
    assert not torch.equal(lat_s, lat) and torch.isfinite(lat_s).all()


@pytest.mark.parametrize("tag,objective,sampler,pre,seed", [("v_uniform", "v", "uniform", False, 62),
                                                            ("rf_logit", "rectified_flow", "logit_normal", False, 63),
                                                            ("v_pre", "v", "uniform", True, 64)])
def test_training_step_wrapper(dev, monkeypatch, tag, objective, sampler, pre, seed):
    """DiffusionCondTrainingWrapper.training_step (the drop-in) against the reference class's own step: conditioner,
    pretransform.encode on the GPU, the scrambled Sobol / logit-normal timestep draw, noising, DiT, masked MSE, backward"""
    from stable_audio_tools.training.diffusion import DiffusionCondTrainingWrapper
    f = fx("training_step")
    e = gu.E2E
    Bt = e["B"]
    model = _cond_model(dev, 8, objective, seed)
    torch.manual_seed(1000 + seed)
    wrap = DiffusionCondTrainingWrapper(model, lr=1e-4, mask_padding=True, mask_padding_dropout=0.0, use_ema=False,
                                        pre_encoded=pre, cfg_dropout_prob=0.0, timestep_sampler=sampler)
    ctx, cm, gl = _e2e_cond(seed, "cpu")
    if pre:
        reals = T(gu.make_input("lat8", (Bt, 8, e["T"]), seed), dev)
        pm = T(gu.make_mask("pm", (Bt, e["T"]), seed, 0.75), "cpu")
    else:
        reals = T(gu.make_input("wav", (Bt, 2, 40 * e["T"]), seed, 0.5), dev)
        pm = T(gu.make_mask("pm", (Bt, e["T"]), seed, 0.75), "cpu").repeat_interleave(40, dim=1)
    meta = [{"prompt": ctx[b], "prompt_mask": cm[b], "g": gl[b], "padding_mask": [pm[b]]} for b in range(Bt)]
    # the device RNG cannot reproduce the reference's CPU draws: feed the recorded ones through the same torch entry points
    noise = T(f[f"{tag}/noise"], dev)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: noise.to(t.dtype))
    drawn = {}
    if sampler == "uniform":
        real_draw = wrap.rng.draw
        wrap.rng.draw = lambda n: drawn.setdefault("t", real_draw(n))
    else:
        z = T(f[f"{tag}/t_logit"], dev)
        monkeypatch.setattr(torch, "randn", lambda *a, **k: z)
    loss = wrap.training_step((reals, meta), 0)
    if sampler == "uniform":          # the wrapper's own Sobol engine (seeded from the global generator) = the reference's
        assert torch.equal(drawn["t"][:, 0], torch.from_numpy(f[f"{tag}/t"]))
    assert abs(loss.item() - float(f[f"{tag}/loss"])) < 1e-2 * float(f[f"{tag}/loss"]), (loss.item(), float(f[f"{tag}/loss"]))
    loss.backward()
    check_digests(f, {n: p.grad for n, p in model.model.named_parameters()}, 16, prefix=f"{tag}/", tol=3e-2)


def test_chunked_vae_batched_pipeline(dev):
    """decode_audio / encode_audio(chunked=True) as ONE batched pass + segment copies: equal to the reference's chunked decode
    (anchored last chunk; odd overlap where the later chunk wins), equal to unchunked away from the seams, both directions"""
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models.factory import create_model_from_config
    f = fx("chunked_vae")
    ae = load_seeded(create_model_from_config(gu.oobleck_cfg(True)), 23, dev)
    z = T(gu.make_input("zc", (2, 4, 125), 65), dev)
    with torch.no_grad():
        assert rel(ae.decode_audio(z, chunked=False), f["dec_full"]) < 1e-4
        for ov, key in ((16, "dec_48_16"), (15, "dec_48_15")):
            got = ae.decode_audio(z, chunked=True, chunk_size=48, overlap=ov)
            assert rel(got, f[key]) < 1e-4, (key, rel(got, f[key]))
        ae.chunk_batch = 4                                       # two chunks per pass: the grouped path gives the same samples
        assert rel(ae.decode_audio(z, chunked=True, chunk_size=48, overlap=16), f["dec_48_16"]) < 1e-4
        ae.chunk_batch = 64
        wav = T(gu.make_input("wavc", (2, 2, 5000), 65, 0.5), dev)
        full = ae.encode_audio(wav, chunked=False)
        assert rel(full, f["enc_full"]) < 1e-4
        ch = ae.encode_audio(wav, chunked=True, chunk_size=48, overlap=16)
        assert ch.shape == full.shape
        # receptive field of this encoder is < 8 latents: the interiors of the kept regions are exact
        for lo, hi in ((0, 32), (48, 64), (100, 125)):
            assert rel(ch[..., lo:hi], full[..., lo:hi]) < 1e-4, (lo, hi, rel(ch[..., lo:hi], full[..., lo:hi]))
        # a 60 s clip at the Stable-Audio layout's 21.5 Hz would be 1290 latents; here 750 latents (60 s @ 12.5 Hz)
        zz = torch.randn(1, 4, 750, device=dev)
        a = ae.decode_audio(zz, chunked=True, chunk_size=128, overlap=32)
        b = ae.decode_audio(zz, chunked=False)
        assert a.shape == b.shape == (1, 2, 750 * 40)
        assert rel(a[..., :40 * 100], b[..., :40 * 100]) < 1e-4
        with pytest.raises(ValueError):
            ae.decode_audio(zz[..., :100], chunked=True, chunk_size=128, overlap=32)


# ------------------------------------------------------------------------------------------------ trainer surfaces
def _small_dit(dev, seed=70, depth=2, **kw):
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models.diffusion import ConditionedDiffusionModelWrapper, DiTWrapper
    kw.setdefault("global_cond_type", "prepend")
    dit = DiTWrapper(io_channels=CIO, embed_dim=D, depth=depth, num_heads=2, cond_token_dim=DC, project_cond_tokens=False,
                     global_cond_dim=GD, transformer_type="continuous_transformer", **kw)
    load_seeded(dit, seed, dev)
    return ConditionedDiffusionModelWrapper(dit, None, io_channels=CIO, sample_rate=16000, min_input_length=1,
                                            cross_attn_cond_ids=["prompt"], global_cond_ids=["g"]).to(dev)


def _batch(dev, B, seed, T_=125, S=7):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, CIO, T_, generator=g).to(dev)
    noise = torch.randn(B, CIO, T_, generator=g).to(dev)
    t = torch.rand(B, generator=g).to(dev)
    ctx = torch.randn(B, S, DC, generator=g).to(dev)
    gl = torch.randn(B, GD, generator=g).to(dev)
    cond = {"prompt": (ctx, torch.ones(B, S, dtype=torch.bool, device=dev)), "g": (gl, None)}
    return lat, noise, t, cond


def _slice_cond(cond, s):
    return {k: (v[0][s], None if v[1] is None else v[1][s]) for k, v in cond.items()}


def test_fused_adam_optimizer_moves_compute_weights(dev):
    """engine.FusedAdam (training/utils.py:88-90's optional optimizer) on a small DiT through plain autograd: three steps
    against torch.optim.Adam on an identical model - same weights, and the forward output follows (the bf16 compute copies
    cached per parameter must be refreshed by the kernel that moves the fp32 weights)"""
    from kalle_audio_amd.engine import FusedAdam
    from stable_audio_tools.training.diffusion import diffusion_train_step
    from stable_audio_tools.training.utils import create_optimizer_from_config
    ma, mb = _small_dit(dev), _small_dit(dev)
    oa = create_optimizer_from_config({"type": "FusedAdam", "config": {"lr": 1e-3, "adam_w_mode": False}}, ma.parameters())
    assert isinstance(oa, FusedAdam)
    ob = torch.optim.Adam(mb.parameters(), lr=1e-3)
    lat, noise, t, cond = _batch(dev, 2, 1)
    outs = []
    for _ in range(3):
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad(set_to_none=True)
            loss, info = diffusion_train_step(m, lat, t, noise, cond)
            loss.backward()
            o.step()
        outs.append(info["output"].detach().clone())
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert rel(pa, pb) < 2e-3, (n, rel(pa, pb))
    with torch.no_grad():
        la, ia = diffusion_train_step(ma, lat, t, noise, cond)
        lb, ib = diffusion_train_step(mb, lat, t, noise, cond)
    assert rel(ia["output"], ib["output"]) < 2e-2
    assert abs(la.item() - lb.item()) < 1e-2 * lb.item()
    assert rel(ia["output"], outs[0]) > 1e-3            # the compute weights really moved between step 1 and step 4


def test_second_consumers_of_block_outputs_and_context(mods, dev):
    """return_info taps every block output a second time, and the trainable context also feeds a term outside the transformer:
    the bf16 gradient hand-over between blocks and the shared context-gradient accumulator must not lose those paths"""
    seed = 71
    ct = load_seeded(mods.ContinuousTransformer(dim=D, depth=3, dim_in=CIO, dim_out=CIO, dim_heads=64, cross_attend=True,
                                                cond_token_dim=DC), seed, dev)
    x = T(gu.make_input("x", (2, 40, CIO), seed), dev, True)
    ctx = T(gu.make_input("ctx", (2, 7, DC), seed), dev, True)
    wy = T(gu.make_input("wy", (2, 40, CIO), seed), dev)
    wh = [T(gu.make_input(f"wh{i}", (2, 40, D), seed), dev) for i in range(3)]
    wc = T(gu.make_input("wc", (2, 7, DC), seed), dev)

    def run(tap):
        for p in ct.parameters():
            p.grad = None
        x.grad = ctx.grad = None
        if tap:
            y, info = ct(x, context=ctx, return_info=True)
            loss = (y * wy).sum() + sum((h.float() * w).sum() for h, w in zip(info["hidden_states"], wh)) + (ctx * wc).sum()
        else:
            y = ct(x, context=ctx)
            loss = (y * wy).sum()
        loss.backward()
        return x.grad.clone(), ctx.grad.clone(), {n: p.grad.clone() for n, p in ct.named_parameters()}

    # reference for the tapped graph: the oracle on the CPU
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in
          gu.make_state(ko.continuous_transformer_shapes(D, 3, CIO, CIO, DC), seed).items()}
    xc, cc = x.detach().cpu().requires_grad_(True), ctx.detach().cpu().requires_grad_(True)
    hs = []
    h = xc @ sd["project_in.weight"].T
    rot = ko.rotary_freqs(40)
    for i in range(3):
        h = ko.transformer_block(ko._sub(sd, f"layers.{i}."), h, context=cc, rotary=rot)
        hs.append(h)
    yo = h @ sd["project_out.weight"].T
    (yo * wy.cpu()).sum().add(sum((a * w.cpu()).sum() for a, w in zip(hs, wh))).add((cc * wc.cpu()).sum()).backward()
    dx, dctx, gp = run(True)
    assert rel(dx, xc.grad) < 2e-2, rel(dx, xc.grad)
    assert rel(dctx, cc.grad) < 2e-2, rel(dctx, cc.grad)
    for n in ("layers.0.ff.ff.0.proj.weight", "layers.1.self_attn.to_qkv.weight", "layers.2.cross_attn.to_kv.weight"):
        assert rel(gp[n], sd[n].grad) < 2e-2, (n, rel(gp[n], sd[n].grad))
    dx0, dctx0, _ = run(False)                      # and the untapped graph still differs (the taps really contribute)
    assert rel(dx0, dx) > 1e-2 and rel(dctx0, dctx) > 1e-2


def test_overlapped_optimizer_equals_single_pass(dev):
    """the fused Adam launched per bucket from the backward hooks on the optimizer stream (engine.py, default on a GPU) against
    the single pass at the end of the step: same weights, moments and bf16 mirror after three steps with gradient accumulation,
    up to the order of the fp32 atomics inside the gradients"""
    from kalle_audio_amd import engine
    lat, noise, t, cond = _batch(dev, 4, 6)
    res = []
    for overlap in (True, False):
        m = _small_dit(dev)
        tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2,
                                        lr_schedule=lambda s: engine.cosine_with_warmup(s, 1, 20))
        assert tr.overlap_adam
        tr.overlap_adam = overlap
        tr.overlap_min_rows = 0                 # (by default only micro-batches of >= 4096 rows overlap)
        for i in range(6):
            s_ = slice(0, 2) if i % 2 == 0 else slice(2, 4)
            tr.train_step(m, lat[s_], t[s_], noise[s_], _slice_cond(cond, s_))
        torch.cuda.synchronize()
        assert tr.step_count == 3
        res.append((tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.flat.param_bf16.float(), tr.last_lr))
    a, b = res
    assert a[4] == b[4]
    # (Adam's first steps move every weight by ~lr whatever the gradient's size: an element whose tiny gradient changes sign with
    # the atomics' order moves the other way - 2e-5 of the weight norm was seen between two runs of the SAME mode)
    assert rel(a[0], b[0]) < 2e-4 and rel(a[1], b[1]) < 5e-3 and rel(a[2], b[2]) < 5e-3 and rel(a[3], b[3]) < 1e-3


def test_trainer_state_dict_roundtrip_resumes(dev):
    """DataParallelTrainer.state_dict / load_state_dict: weights, Adam moments, step, accumulation phase and the EMA; a
    restored trainer continues exactly like the original"""
    from kalle_audio_amd import engine
    lat, noise, t, cond = _batch(dev, 4, 2)
    a = _small_dit(dev)
    ta = engine.DataParallelTrainer(a, lr=1e-3, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2,
                                    lr_schedule=lambda s: engine.cosine_with_warmup(s, 2, 50))
    ta.enable_ema(beta=0.9999, power=3 / 4, update_every=1, update_after_step=1)
    for i in range(5):                                # ends in the middle of an accumulation window
        ta.train_step(a, lat[:2] if i % 2 == 0 else lat[2:], t[:2], noise[:2], _slice_cond(cond, slice(0, 2)))
    sd = {k: (v.clone() if torch.is_tensor(v) else (dict(v) if isinstance(v, dict) else v)) for k, v in ta.state_dict().items()}
    sd["model"] = {k: v.clone() for k, v in sd["model"].items()}
    b = _small_dit(dev, seed=99)                      # different weights: everything must come from the checkpoint
    tb = engine.DataParallelTrainer(b, lr=1e-3, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2,
                                    lr_schedule=lambda s: engine.cosine_with_warmup(s, 2, 50))
    assert "grad" in sd and "layout" in sd            # the half-finished accumulation window travels with the checkpoint
    tb.load_state_dict(sd)
    assert torch.equal(tb.flat.grad, sd["grad"])
    bad = dict(sd, layout={k: [v[0] + 64, v[1]] for k, v in sd["layout"].items()})
    with pytest.raises(ValueError):                   # moments written under another flat layout must not load silently
        tb.load_state_dict(bad)
    assert tb.step_count == ta.step_count == 2 and tb.micro == ta.micro == 5
    assert torch.equal(tb.flat.param, ta.flat.param) and torch.equal(tb.flat.param_bf16, ta.flat.param_bf16)
    assert torch.equal(tb.ema, ta.ema)
    for tr, m in ((ta, a), (tb, b)):
        for i in range(3):
            tr.train_step(m, lat[2:], t[2:], noise[2:], _slice_cond(cond, slice(2, 4)))
    torch.cuda.synchronize()
    assert ta.last_lr == tb.last_lr and ta.step_count == tb.step_count == 4
    # (same state, same inputs: equal up to the order of the fp32 atomics in the split-K / gamma gradients)
    assert rel(tb.flat.param, ta.flat.param) < 1e-4
    assert rel(tb.ema, ta.ema) < 1e-4
    # (a weight whose fp32 value sits on a bf16 rounding boundary may round differently after an update that differs in the last
    # fp32 bits: the later gradients then differ at the 1e-3 level in a few entries, which the second moment squares)
    assert rel(tb.exp_avg_sq, ta.exp_avg_sq) < 5e-3, rel(tb.exp_avg_sq, ta.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ communication on hardware
def test_two_rank_emulation_equals_one_rank_on_concatenated_batch(dev):
    """SURVEY 8(e) with the real kernels: two trainers (two "ranks") on the halves of a batch, their flat gradients summed as
    the all-reduce would, against one trainer on the whole batch; then the fused Adam with 1/world folded in gives the same
    weights as the single-rank step"""
    from kalle_audio_amd import engine
    lat, noise, t, cond = _batch(dev, 4, 3)
    one = _small_dit(dev)
    t1 = engine.DataParallelTrainer(one, lr=1e-3, optimizer="Adam")
    t1.lr = 0.0
    t1.train_step(one, lat, t, noise, cond)
    g_one = t1.flat.grad.clone()
    ranks = []
    for r in range(2):
        m = _small_dit(dev)
        tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam")
        tr.lr = 0.0
        s = slice(2 * r, 2 * r + 2)
        tr.train_step(m, lat[s], t[s], noise[s], _slice_cond(cond, s))
        ranks.append(tr)
    g_sum = ranks[0].flat.grad + ranks[1].flat.grad          # what all_reduce(SUM) leaves in every rank's bucket
    # MSE is a mean over the batch: the mean of the two half-batch gradients is the full-batch gradient
    assert rel(g_sum * 0.5, g_one) < 2e-2, rel(g_sum * 0.5, g_one)
    from kalle_audio_amd import ops
    p1, p2 = t1.flat.param.clone(), ranks[0].flat.param.clone()
    z = torch.zeros_like(p1)
    ops.adam_step(p1, g_one, z.clone(), z.clone(), None, lr=1e-3, step=1, grad_scale=1.0)
    ops.adam_step(p2, g_sum, z.clone(), z.clone(), None, lr=1e-3, step=1, grad_scale=0.5)       # 1 / world
    d1, d2 = p1 - t1.flat.param, p2 - ranks[0].flat.param     # Adam's first step: -lr * g / (|g| + eps) per element
    big = g_one.abs() > 1e-3 * g_one.abs().max()
    assert rel(d2[big], d1[big]) < 5e-2, rel(d2[big], d1[big])


def test_qk_norm_dit_through_trainer_matches_autograd(dev):
    """a DiT with attn_kwargs={"qk_norm": "ln"}: the trainer path (LayerNorm(64) gradients added atomically into the flat
    bucket's vector range, two accumulated micro-batches, grouped weight gradients) equals plain autograd on the whole batch"""
    from kalle_audio_amd import engine
    from stable_audio_tools.training.diffusion import diffusion_train_step
    lat, noise, t, cond = _batch(dev, 4, 5)
    ref = _small_dit(dev, attn_kwargs={"qk_norm": "ln"})
    loss, _ = diffusion_train_step(ref, lat, t, noise, cond)
    loss.backward()
    want = {n: p.grad.clone() for n, p in ref.named_parameters()}
    assert sum("q_norm" in n or "k_norm" in n for n in want) == 2 * 2 * 4        # 2 layers x (self, cross) x (q, k) x (w, b)
    m = _small_dit(dev, attn_kwargs={"qk_norm": "ln"})
    tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam", grad_accum_steps=2)
    tr.lr = 0.0
    for r in range(2):
        s = slice(2 * r, 2 * r + 2)
        tr.train_step(m, lat[s], t[s], noise[s], _slice_cond(cond, s))
    for n, p in m.named_parameters():
        a, cnt = tr.flat.slices[n]
        got = tr.flat.grad[a:a + cnt].view(p.shape) * 0.5         # two half-batch means
        if "cross_attn.k_norm.bias" in n:
            continue                                              # mathematically zero: rounding noise on both sides
        assert rel(got, want[n]) < 3e-2, (n, rel(got, want[n]))


_COMM_WORKER = r'''
import os, sys, json, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "golden"))
os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], KALLE_FORCE_COMM="1")
import torch.distributed as dist
from kalle_audio_amd import engine
import test_round2_gpu as R
dev = torch.device("cuda:0")
rank, world, _ = engine.init_distributed()
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
lat, noise, t, cond = R._batch(dev, 4, 4)
res = {}
os.environ.pop("KALLE_FORCE_COMM")
m = R._small_dit(dev); tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam")
for _ in range(2): tr.train_step(m, lat, t, noise, cond)
torch.cuda.synchronize(); base_p, base_g = tr.flat.param.clone(), tr.flat.grad.clone()
assert tr._pending == []
os.environ["KALLE_FORCE_COMM"] = "1"
for name, cd in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    m = R._small_dit(dev); tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam", comm_dtype=cd)
    tr.overlap_min_rows = 0          # fp32 buckets: all-reduce wait + Adam slice per bucket on the optimizer stream
    tr.comm_timing = []
    for _ in range(2): tr.train_step(m, lat, t, noise, cond)
    torch.cuda.synchronize()
    s = tr.comm_summary()
    res[name] = {"grad": R.rel(tr.flat.grad, base_g), "param": R.rel(tr.flat.param, base_p), "summary": s}
# sharded optimizer (KALLE_SHARD_OPTIMIZER=1): reduce-scatter -> Adam on the own chunk -> all-gather -> bf16 mirror, on RCCL (one rank),
# with the per-bucket overlap and with the single optimizer pass of small micro-batches
os.environ["KALLE_SHARD_OPTIMIZER"] = "1"
for name, min_rows in (("shard", 0), ("shard_small", 1 << 30)):
    m = R._small_dit(dev); tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam")
    assert tr._sharded_active()
    tr.overlap_min_rows = min_rows
    for _ in range(2): tr.train_step(m, lat, t, noise, cond)
    torch.cuda.synchronize()
    sd = tr.state_dict()
    res[name] = {"grad": R.rel(tr.flat.grad, base_g), "param": R.rel(tr.flat.param, base_p),
                 "mirror": float((tr.flat.param_bf16.float() - tr.flat.param.bfloat16().float()).abs().max()),
                 "moments": bool(torch.count_nonzero(sd["exp_avg_sq"]) > 0.5 * sd["exp_avg_sq"].numel())}
os.environ["KALLE_SHARD_OPTIMIZER"] = "0"
# gradient accumulation: the all-reduce fires on the boundary micro-batch only
m = R._small_dit(dev); tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="Adam", grad_accum_steps=2)
tr.comm_timing = []
for i in range(4): tr.train_step(m, lat, t, noise, cond)
torch.cuda.synchronize()
res["accum_events"] = len(tr.comm_timing)
dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_rccl_path_world1_forced_comm(dev, tmp_path):
    """KALLE_FORCE_COMM=1 with a world-1 "nccl" (= RCCL) group, in a child process: every bucket really goes through
    ncclAllReduce on RCCL's stream behind the backward hook, with fp32 and with bf16 buckets; gradients and the updated
    weights equal the no-communication run (fp32 exactly up to atomics order, bf16 within its rounding)"""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "comm_worker.py"
    script.write_text(_COMM_WORKER)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), os.path.join(HERE, ".."), str(port)], capture_output=True, text=True,
                       timeout=420, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["fp32"]["grad"] < 1e-4 and res["fp32"]["param"] < 1e-6, res["fp32"]
    assert res["bf16"]["grad"] < 8e-3, res["bf16"]                # one bf16 rounding of every gradient element
    assert res["bf16"]["param"] < 1e-3, res["bf16"]
    for k in ("fp32", "bf16"):
        sm = res[k]["summary"]
        assert sm["backend"] == "nccl" and sm["ranks"] == 1 and sm["allreduce_active"] and sm["buckets_per_step"] == 3, sm
        assert sm["exposed_ms_per_step"] >= 0.0
    assert res["accum_events"] == 2
    for k in ("shard", "shard_small"):       # same kernels on the same gradients: the weights of the plain run, mirror = bf16(weights)
        assert res[k]["grad"] < 1e-4 and res[k]["param"] < 1e-6 and res[k]["mirror"] == 0.0 and res[k]["moments"], (k, res[k])


# ------------------------------------------------------------------------------------------------ grouped weight gradients
# (tiles, whole, slices) as kalle_gemm_wgrad_group_last_plan reports them
@pytest.mark.parametrize("tokens,shapes,plan", [
    (512, [(4096, 4096), (512, 256), (264, 136)], (260, 260, 0)),     # 8 K-tiles are never sliced: 260 whole tiles
    (4096, [(512, 384), (256, 640), (128, 128)], (8, 0, 8)),          # few tiles: all cut into K slices
    (8064, [(1536, 1536), (4608, 1536), (1536, 768)], (162, 162, 0)),
    (2016, [(1536, 1536), (4608, 1536), (1536, 768)], None),          # B = 16: ragged last K-tile
    (1024, [(4096, 4096), (512, 256), (264, 136)], (260, 256, 2))],   # 256 whole tiles + a sliced tail
    ids=["512-shapes0", "4096-shapes1", "8064-shapes2", "2016-shapes3", "1024-shapes4"])
def test_grouped_wgrad_kernel_vs_fp32(dev, tokens, shapes, plan):
    """kalle_gemm_wgrad_group: several dW += dY^T X problems in one launch (whole tiles: read-add-store; sliced tiles: atomics)
    against an fp32 matmul of the same bf16 operands, accumulating onto a non-zero sink; and against one kalle_gemm_bf16 each"""
    from kalle_audio_amd import ops
    g = torch.Generator().manual_seed(tokens)
    probs, refs, singles = [], [], []
    for n, k in shapes:
        dy = (torch.randn(tokens, n, generator=g) * 0.5).to(dev).to(torch.bfloat16)
        x = torch.randn(tokens, k, generator=g).to(dev).to(torch.bfloat16)
        base = torch.randn(n, k, generator=g).to(dev)
        probs.append((dy, x, base.clone()))
        refs.append(base.double() + dy.double().T @ x.double())
        singles.append(base + ops.gemm(dy, x, a_kmajor=True, b_kmajor=True, out_dtype=torch.float32))
    want = ops.wgrad_group_plan([(tokens, n, k) for n, k in shapes])
    assert ops.gemm_wgrad_group(probs)
    got = ops.wgrad_group_last_plan()
    assert got == dict(want, cached=got["cached"]) and (plan is None or (got["tiles"], got["whole"], got["slices"]) == plan), (got, want)
    torch.cuda.synchronize()
    for (dy, x, out), ref, one in zip(probs, refs, singles):
        assert rel(out, ref.float()) < 2e-5, rel(out, ref.float())          # fp32 accumulation of exact bf16 products
        assert rel(out, one) < 2e-5
    assert not ops.gemm_wgrad_group([(probs[0][0][:100], probs[0][1][:100], probs[0][2])])   # tokens % 8: caller falls back


@pytest.mark.parametrize("M,N,K", [(512, 384, 200), (2016, 1536, 1544), (304, 256, 72)])
@pytest.mark.parametrize("layout", ["nn", "nt", "tt"])
def test_gemm_ragged_k_on_the_lds_dma_kernels(dev, M, N, K, layout):
    """K not a multiple of 64 (B = 16 per GPU gives 2016-token weight gradients): the 256-wide LDS-DMA kernels take the missing
    pieces of the last K-tile from a block of zeros; result = fp32 matmul of the bf16 operands.  The memory behind the
    operands is poisoned with NaN so that any read past K shows."""
    from kalle_audio_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a_km, b_km = layout == "tt", layout in ("nt", "tt")
    def operand(rows, cols):                                 # a [rows, cols] view at the START of a NaN-filled buffer
        buf = torch.full((rows + 64, cols), float("nan"), device=dev, dtype=torch.bfloat16)
        buf[:rows] = torch.randn(rows, cols, generator=g).to(dev).to(torch.bfloat16)
        return buf[:rows]
    a = operand(K, M) if a_km else operand(M, K)
    b = operand(K, N) if b_km else operand(N, K)
    A = a.double().T if a_km else a.double()
    Bm = b.double() if b_km else b.double().T
    ref = (A @ Bm).float()
    out = ops.gemm(a, b, a_kmajor=a_km, b_kmajor=b_km, out_dtype=torch.float32)
    assert torch.isfinite(out).all()
    assert rel(out, ref) < 2e-5, rel(out, ref)


# ------------------------------------------------------------------------------------------------ VAE backward (enable_grad)
@pytest.mark.parametrize("snake", [True, False])
def test_vae_backward_units_and_chain(dev, snake):
    """the conv stacks as autograd units (csrc/conv1d_bwd.hip + the forward kernels over dy): ResidualUnit, EncoderBlock,
    DecoderBlock and encode -> decode against the reference's torch autograd; fp32 path, rel-L2 <= 1e-4 (2e-4 on the chain)"""
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models import autoencoders as A
    from stable_audio_tools.models.factory import create_model_from_config
    f = fx("vae_backward")
    tag = "snake" if snake else "elu"
    Bv = 2
    units = (("ru", A.ResidualUnit(16, 16, dilation=3, use_snake=snake), 20, (Bv, 16, 200)),
             ("eb", A.EncoderBlock(16, 32, stride=4, use_snake=snake), 21, (Bv, 16, 203)),
             ("db", A.DecoderBlock(32, 16, stride=4, use_snake=snake), 22, (Bv, 32, 50)))
    for name, mod, seed, shp in units:
        load_seeded(mod, seed, dev)
        x = T(gu.make_input("x", shp, seed + 100, 1.0), dev, True)
        y = mod(x)
        assert rel(y, f[f"{tag}/{name}/y"]) < 1e-4, (name, rel(y, f[f"{tag}/{name}/y"]))
        y.backward(T(gu.make_input("dy", tuple(y.shape), seed + 100), dev))
        assert rel(x.grad, f[f"{tag}/{name}/dx"]) < 1e-4, (name, rel(x.grad, f[f"{tag}/{name}/dx"]))
        g = {n: p.grad for n, p in mod.named_parameters()}
        assert all(v is not None for v in g.values()), [n for n, v in g.items() if v is None]
        check_digests(f, g, 16, prefix=f"{tag}/{name}/", tol=1e-3)
        for k in f.files:
            if k.startswith(f"{tag}/{name}/grad/"):
                n = k[len(f"{tag}/{name}/grad/"):]
                assert rel(g[n], f[k]) < 2e-4, (name, n, rel(g[n], f[k]))
    ae = load_seeded(create_model_from_config(gu.oobleck_cfg(snake)), 23, dev)
    ae.requires_grad_(True)
    wav = T(gu.make_input("wav", (Bv, 2, 1200), 66, 0.5), dev, True)
    z = ae.encode(wav)
    rec = ae.decode(z[:, :4] + 0.3 * z[:, 4:])
    assert rel(z, f[f"{tag}/ae/z"]) < 1e-4 and rel(rec, f[f"{tag}/ae/rec"]) < 1e-4
    dz, drec = T(gu.make_input("dz", tuple(z.shape), 66), dev), T(gu.make_input("drec", tuple(rec.shape), 66), dev)
    ((z * dz).sum() + (rec * drec).sum()).backward()
    assert rel(wav.grad, f[f"{tag}/ae/dwav"]) < 2e-4, rel(wav.grad, f[f"{tag}/ae/dwav"])
    check_digests(f, {n: p.grad for n, p in ae.named_parameters()}, 16, prefix=f"{tag}/ae/", tol=1e-3)
    # frozen again: the same modules are back on the fused inference kernels (no autograd graph)
    ae.requires_grad_(False)
    with torch.no_grad():
        z2 = ae.encode(wav.detach())
    assert not z2.requires_grad and rel(z2, z) < 1e-5


@pytest.mark.parametrize("snake", [True, False])
def test_vae_nearest_upsample_decoder(dev, snake):
    """use_nearest_upsample (autoencoders.py:87-96): sample repetition (kalle_upsample_nearest) + a stride-1 conv with an even
    kernel and torch's asymmetric 'same' padding; DecoderBlock and the whole decoder, training path (autograd units) against
    the reference's forward / gradients, then the fused inference path against the same forward; fp32, rel-L2 <= 1e-4"""
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models import autoencoders as A
    f = fx("vae_nearest")
    tag = "snake" if snake else "elu"
    mod = load_seeded(A.DecoderBlock(32, 16, stride=4, use_snake=snake, use_nearest_upsample=True), 31, dev)
    x = T(gu.make_input("x", (2, 32, 50), 131, 1.0), dev, True)
    y = mod(x)
    assert rel(y, f[f"{tag}/db/y"]) < 1e-4, rel(y, f[f"{tag}/db/y"])
    y.backward(T(gu.make_input("dy", tuple(y.shape), 131), dev))
    assert rel(x.grad, f[f"{tag}/db/dx"]) < 1e-4, rel(x.grad, f[f"{tag}/db/dx"])
    g = {n: p.grad for n, p in mod.named_parameters()}
    assert all(v is not None for v in g.values()), [n for n, v in g.items() if v is None]
    check_digests(f, g, 16, prefix=f"{tag}/db/", tol=1e-3)
    for k in f.files:
        if k.startswith(f"{tag}/db/grad/"):
            n = k[len(f"{tag}/db/grad/"):]
            assert rel(g[n], f[k]) < 2e-4, (n, rel(g[n], f[k]))
    dec = load_seeded(A.OobleckDecoder(out_channels=2, channels=8, latent_dim=4, c_mults=[1, 2, 4], strides=[2, 4, 5],
                                       use_snake=snake, use_nearest_upsample=True, final_tanh=snake), 32, dev)
    z = T(gu.make_input("z", (2, 4, 37), 132, 1.0), dev, True)
    w = dec(z)
    assert rel(w, f[f"{tag}/dec/y"]) < 1e-4, rel(w, f[f"{tag}/dec/y"])
    w.backward(T(gu.make_input("dw", tuple(w.shape), 132), dev))
    assert rel(z.grad, f[f"{tag}/dec/dz"]) < 2e-4, rel(z.grad, f[f"{tag}/dec/dz"])
    check_digests(f, {n: p.grad for n, p in dec.named_parameters()}, 16, prefix=f"{tag}/dec/", tol=1e-3)
    dec.requires_grad_(False)
    with torch.no_grad():
        w2 = dec(z.detach())
    assert not w2.requires_grad and rel(w2, f[f"{tag}/dec/y"]) < 1e-4, rel(w2, f[f"{tag}/dec/y"])


def test_training_step_with_enable_grad_pretransform(dev, monkeypatch):
    """training_step with pretransform.enable_grad: the diffusion loss reaches the VAE encoder through x_t AND the target
    (training/diffusion.py:343-346, 371-379); gradients against the CPU oracle's autograd on the same draws; and the trainer
    gives the VAE parameters their own all-reduce bucket"""
    from stable_audio_tools.training.diffusion import DiffusionCondTrainingWrapper
    from kalle_audio_amd import engine
    e = gu.E2E
    seed, Bt = 62, e["B"]
    f = fx("training_step")
    model = _cond_model(dev, 8, "v", seed)
    model.pretransform.enable_grad = True
    model.pretransform.requires_grad_(True)
    torch.manual_seed(1000 + seed)
    wrap = DiffusionCondTrainingWrapper(model, lr=1e-4, mask_padding=False, use_ema=False, pre_encoded=False,
                                        cfg_dropout_prob=0.0, timestep_sampler="uniform")
    ctx, cm, gl = _e2e_cond(seed, "cpu")
    wav = gu.make_input("wav", (Bt, 2, 40 * e["T"]), seed, 0.5)
    meta = [{"prompt": ctx[b], "prompt_mask": cm[b], "g": gl[b]} for b in range(Bt)]
    noise = T(f["v_uniform/noise"], dev)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: noise.to(t.dtype))
    loss = wrap.training_step((T(wav, dev), meta), 0)
    loss.backward()
    # oracle: same weights, same t (the Sobol draw of the fixture), same noise
    from test_oracle_golden import e2e_states
    sd_dit, sd_vae = e2e_states(8, seed, grad=False)
    sd_vae = {k: v.clone().requires_grad_(True) for k, v in sd_vae.items()}
    cfg = dict(embed_dim=e["D"], depth=2, num_heads=2, global_cond_type="prepend")
    ci = ko.conditioning_inputs({"prompt": (ctx, cm), "g": (gl, None)}, ["prompt"], ["g"])
    lat = ko.pretransform_encode(sd_vae, torch.from_numpy(wav), [2, 4, 5], True, 0.8)
    lref, *_ = ko.train_step_loss(sd_dit, cfg, lat, torch.from_numpy(f["v_uniform/noise"]), torch.from_numpy(f["v_uniform/t"]),
                                  "v", **ci)
    lref.backward()
    assert abs(loss.item() - lref.item()) < 1e-2 * lref.item()
    n = 0
    for name, p in model.pretransform.model.named_parameters():
        if not name.startswith("encoder."):
            continue
        ref = sd_vae[name].grad
        assert p.grad is not None, name
        assert rel(p.grad, ref) < 5e-2, (name, rel(p.grad, ref))        # (through the bf16 DiT)
        n += 1
    assert n > 20
    tr = engine.DataParallelTrainer(model, lr=1e-4)
    assert "_vae" in tr.flat.bucket_keys
    assert any(k.startswith("pretransform.") for k in tr.flat.names)


# ------------------------------------------------------------------------------------------------ few-rows GEMM path
@pytest.mark.parametrize("M,N,K", [(252, 1536, 1536), (252, 4608, 1536), (126, 1536, 6144), (504, 1536, 12288), (504, 768, 200),
                                   (2016, 1536, 1536), (2520, 1536, 6144), (252, 1472, 1536)])
@pytest.mark.parametrize("b_km", [False, True])
def test_gemm_few_rows_splitk_path(dev, M, N, K, b_km):
    """M <= 4096 rows (sampling at generation batch sizes, B = 16 training).  k-major weights (data gradients): K is cut into
    slices that write fp32 slabs into the caller's scratch, a finishing pass sums them in order and applies the epilogue (plan 4:
    2048 < M <= 4096, or column counts the small tiles do not take).  M <= 2048 (every nn.Linear of the sampling path, B = 16
    training): small output tiles (64 x 64 ... 128 x 128, two wave groups per tile; k-major weights 128 x 128) over the whole K
    with the epilogue in the same launch, K slices + slabs only for long K (plan 5).
    Same numbers as the ordinary path (fp32 accumulation of the same bf16 products), every epilogue option, and bitwise
    identical from run to run."""
    from kalle_audio_amd import ops, _lib
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16)
    b = (torch.randn(K, N, generator=g) if b_km else torch.randn(N, K, generator=g)).to(dev).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    Bm = b.double() if b_km else b.double().T
    ref = (a.double() @ Bm)
    lib = _lib.load()

    def run(**kw):
        out = ops.gemm(a, b, b_kmajor=b_km, **kw)
        return out, lib.kalle_gemm_last_plan() & 255

    y, plan = run(out_dtype=torch.float32)
    want = 5 if (M <= 2048 and N % 64 == 0 and (not b_km or N % 128 == 0)) else 4
    assert plan == want, (plan, want)                              # the few-rows path meant for this layout really ran
    assert rel(y, ref.float()) < 2e-5
    y2, _ = run(out_dtype=torch.float32)
    assert torch.equal(y, y2)                                      # slabs summed in slice order: reproducible bit for bit
    y, _ = run(out_dtype=torch.float32, bias=bias, residual=res)
    assert rel(y, (ref + bias.double() + res.double()).float()) < 2e-5
    y, _ = run(out_dtype=torch.bfloat16, bias=bias)
    assert rel(y, (ref + bias.double()).float()) < 4e-3
    acc = res.clone()
    y, _ = run(out=acc, accumulate=True)
    assert rel(acc, (ref + res.double()).float()) < 2e-5
    ops.FEW_ROWS = False
    try:
        y0, plan0 = run(out_dtype=torch.float32, bias=bias, residual=res)
    finally:
        ops.FEW_ROWS = True
    assert plan0 != 4
    y, _ = run(out_dtype=torch.float32, bias=bias, residual=res)
    assert rel(y, y0) < 1e-5


def test_gemm_few_rows_fused_swiglu_forward(dev):
    """the FeedForward's first GEMM at sampling sizes: h = x W^T + b and act = h_x * silu(h_gate) out of the finishing pass,
    against the separate GEMM + kalle_swiglu_fwd"""
    from kalle_audio_amd import ops
    M, D, inner = 252, 1536, 6144
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, D, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(2 * inner, D, generator=g) * 0.03).to(dev).to(torch.bfloat16)
    bias = torch.randn(2 * inner, generator=g).to(dev)
    hf = torch.empty(M, 2 * inner, device=dev, dtype=torch.bfloat16)
    act = torch.empty(M, inner, device=dev, dtype=torch.bfloat16)
    assert ops.gemm(x, w, bias=bias, out=hf, glu_mode=1, glu_inner=inner, glu_aux=act) is not None
    ops.FEW_ROWS = False
    try:
        h0 = ops.gemm(x, w, bias=bias)
    finally:
        ops.FEW_ROWS = True
    a0 = ops.swiglu_fwd(h0)
    assert rel(hf, h0) < 4e-3 and rel(act, a0) < 6e-3


def test_encode_latents_example_writes_reference_latent_files(dev, tmp_path):
    """examples/encode_latents_hip.py (the GPU replacement of the reference's CPU-worker encode, twj_dataset.py:225-239):
    writes mean || scale [2 * latent_dim, T] .npy files (the format twj_data_offline_sd2.py:279-287 reads) equal to a direct
    pretransform.encode of the same normalised clip"""
    import subprocess
    import kalle_audio_amd
    kalle_audio_amd.install()
    from stable_audio_tools.models.factory import create_model_from_config
    cfg = gu.oobleck_cfg(True)
    (tmp_path / "model_config.json").write_text(json.dumps(cfg))
    ae = create_model_from_config(cfg)
    load_seeded(ae, 23, dev)
    torch.save({"state_dict": ae.state_dict()}, tmp_path / "vae.ckpt")
    wav = gu.make_input("clip", (2, 9013), 67, 0.3)                 # not a multiple of the downsampling ratio (40)
    np.save(tmp_path / "clip0.npy", wav)
    (tmp_path / "clips.txt").write_text(str(tmp_path / "clip0.npy") + "\n")
    script = os.path.join(HERE, "..", "examples", "encode_latents_hip.py")
    r = subprocess.run([sys.executable, script, "--model-config", str(tmp_path / "model_config.json"), "--ckpt",
                        str(tmp_path / "vae.ckpt"), "--list", str(tmp_path / "clips.txt"), "--out", str(tmp_path / "lat")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(tmp_path / "lat" / "clip0.npy")
    mono = wav.mean(0)
    mono = mono / np.abs(mono).max() * 0.95
    mono = np.pad(mono, (0, (-len(mono)) % 40))
    x = torch.from_numpy(mono).to(dev).view(1, 1, -1).repeat(1, 2, 1)
    with torch.no_grad():
        ref = ae.encode(x)[0]
    assert z.shape == (8, len(mono) // 40) and z.dtype == np.float32
    assert rel(torch.from_numpy(z), ref) < 1e-5


def test_gemm_random_shapes_every_dispatch_path(dev):
    """seeded sweep over (M, N, K, layout, output type, epilogue options): whichever kernel the dispatcher picks - single-row
    GEMV, small tiles (plan 5), few-rows slabs (4), 256 x 128 (2), 256 x 256 (3), first-generation 128 x 128 (1) - the result
    matches fp64 on the same bf16 operands (fp32 accumulation: 3e-5 for fp32 outputs, one bf16 rounding for bf16 outputs)"""
    from kalle_audio_amd import ops, _lib
    lib = _lib.load()
    rng = np.random.RandomState(1234)
    seen = set()
    for it in range(48):
        M = int(rng.choice([1, 7, 16, 100, 126, 252, 504, 520, 1000, 2016, 2100, 3000, 4100]))
        N = int(rng.choice([64, 128, 192, 768, 1472, 1536, 2048])) if it % 5 else int(rng.choice([8, 24, 1000]))
        K = int(rng.choice([8, 64, 200, 768, 1536, 2056]))
        b_km = bool(rng.randint(2))
        f32 = bool(rng.randint(2))
        g = torch.Generator().manual_seed(it)
        a = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16)
        b = (torch.randn(K, N, generator=g) if b_km else torch.randn(N, K, generator=g)).to(dev).to(torch.bfloat16)
        ref = a.double() @ (b.double() if b_km else b.double().T)
        kw = dict(b_kmajor=b_km, out_dtype=torch.float32 if f32 else torch.bfloat16)
        opt = int(rng.randint(4))
        if opt & 1:
            bias = torch.randn(N, generator=g).to(dev)
            kw["bias"] = bias
            ref = ref + bias.double()
        if (opt & 2) and f32:
            res = torch.randn(M, N, generator=g).to(dev)
            kw["residual"] = res
            ref = ref + res.double()
        y = ops.gemm(a, b, **kw)
        seen.add(lib.kalle_gemm_last_plan() & 255 if M > 1 else 0)
        tol = 3e-5 if f32 else 4e-3
        assert y.shape == (M, N) and rel(y, ref.float()) < tol, (it, M, N, K, b_km, f32, opt, rel(y, ref.float()))
    assert {1, 2, 4, 5} <= seen, seen       # (the sweep really went through the different kernels)


def test_conv_random_shapes_against_torch(dev):
    """seeded sweep over the conv kernels' dispatch (position-per-lane tiles of 2 / 8 / 16 channels, 8-wave tiles, channels-per-lane
    kernel with and without the input-channel split, strided and transposed forms): channel counts that are no multiple of the
    tile widths, kernel sizes 1-16, dilations, strides, asymmetric padding, odd lengths - against torch's fp32 conv (1e-4).
    kalle_conv_last_plan of every iteration is collected and the families named above must all have been seen: the 40 seeded
    shapes stay below the ~6 M outputs at which pick_tile's cost model takes the 16-channel and 8-wave tiles, so three explicit
    shapes follow them."""
    import torch.nn.functional as F
    from kalle_audio_amd import _lib, conv_ops
    lib = _lib.load()
    rng = np.random.RandomState(77)
    # (B, Cin, Cout, K, L): 16 x 8 x 4 tiles; 8-wave pointwise; 8-wave wide
    explicit = [(3, 8, 64, 3, 32910), (1, 8, 272, 1, 21943), (2, 8, 272, 7, 21943)]
    seen = set()
    for it in range(40 + len(explicit)):
        if it >= 40:
            B, Cin, Cout = explicit[it - 40][:3]
        else:
            B = int(rng.choice([1, 2, 3]))
            Cin = int(rng.choice([1, 2, 3, 8, 17, 32, 64, 130, 256, 520]))
            Cout = int(rng.choice([1, 2, 6, 16, 17, 24, 64, 100, 256, 512]))
        g = torch.Generator().manual_seed(1000 + it)
        if it >= 40:
            stride, dil, (K, L) = 1, 1, explicit[it - 40][3:]
            pad = pr = (K - 1) // 2
            L += K - 1
            x = torch.randn(B, Cin, L, generator=g).to(dev)
            v = (torch.randn(Cout, Cin, K, generator=g) * 0.2).to(dev)
            gg = (1 + 0.1 * torch.randn(Cout, generator=g)).to(dev)
            bias = torch.randn(Cout, generator=g).to(dev)
            w = gg.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
            ref = F.conv1d(F.pad(F.elu(x), (pad, pr)), w, bias)
            y = conv_ops.conv1d(x, conv_ops.weight_norm_fold(v, gg), bias, Cout=Cout, K=K, stride=1, padding=pad, dilation=1, act=2,
                                pad_right=pr)
        elif it % 4 == 3:                                   # transposed conv (decoder up-sampling): K = 2 s + s % 2, pad = ceil(s / 2)
            stride = int(rng.choice([2, 4, 5, 8]))
            K, pad = 2 * stride + stride % 2, (stride + 1) // 2
            L = int(rng.choice([5, 27, 130, 431]))
            x = torch.randn(B, Cin, L, generator=g).to(dev)
            v = (torch.randn(Cin, Cout, K, generator=g) * 0.2).to(dev)
            gg = (1 + 0.1 * torch.randn(Cin, generator=g)).to(dev)
            bias = torch.randn(Cout, generator=g).to(dev)
            w = gg.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
            ref = F.conv_transpose1d(x, w, bias, stride=stride, padding=pad)
            y = conv_ops.conv_transpose1d(x, conv_ops.weight_norm_fold(v, gg, transposed=True), bias, Cout=Cout, K=K, stride=stride,
                                          padding=pad)
        else:
            stride = int(rng.choice([1, 1, 1, 2, 4, 8]))
            K = int(rng.choice([1, 2, 3, 7, 11])) if stride == 1 else 2 * stride
            dil = int(rng.choice([1, 3, 9])) if stride == 1 else 1
            total = dil * (K - 1)
            pad = (stride + 1) // 2 if stride > 1 else total // 2
            pr = (total - pad) if stride == 1 else pad     # torch 'same' for even kernels: the odd zero goes to the right
            L = int(rng.choice([40, 203, 1000, 4099])) + total
            x = torch.randn(B, Cin, L, generator=g).to(dev)
            v = (torch.randn(Cout, Cin, K, generator=g) * 0.2).to(dev)
            gg = (1 + 0.1 * torch.randn(Cout, generator=g)).to(dev)
            bias = torch.randn(Cout, generator=g).to(dev) if it % 3 else None
            w = gg.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
            ref = F.conv1d(F.pad(F.elu(x), (pad, pr)), w, bias, stride=stride, dilation=dil)
            y = conv_ops.conv1d(x, conv_ops.weight_norm_fold(v, gg), bias, Cout=Cout, K=K, stride=stride, padding=pad,
                                dilation=dil, act=2, pad_right=pr)
        assert y.shape == ref.shape, (it, y.shape, ref.shape)
        assert rel(y, ref) < 1e-4, (it, B, Cin, Cout, K, stride, rel(y, ref))
        seen.add(lib.kalle_conv_last_plan())
    fam = lambda p: p & 15                                                      # noqa: E731  (encoding: include/kalle_hip.h)
    v2 = {p for p in seen if fam(p) in (2, 4)}
    assert {2, 8, 16} <= {p >> 8 & 31 for p in v2}, sorted(map(hex, seen))      # tiles of 2 / 8 / 16 channels per wave
    assert any(p >> 21 & 15 == 8 for p in v2), sorted(map(hex, seen))           # 8-wave tiles
    cfirst = {p for p in seen if fam(p) in (5, 6, 7)}
    assert {False, True} <= {(p >> 12 & 31) > 1 for p in cfirst}, sorted(map(hex, seen))    # with and without the input-channel split
    assert any(fam(p) == 6 or (fam(p) == 2 and p >> 28 & 7) for p in seen)      # strided forms
    assert {4, 7} <= {fam(p) for p in seen}, sorted(map(hex, seen))             # transposed: position-per-lane and channels-per-lane
    assert 1 in {fam(p) for p in seen}                                          # the fallback kernel


def test_attention_random_lengths_and_groups(dev):
    """seeded sweep of the fused attention (forward, both backward kernels) over query / key lengths around the 128-row block
    boundaries, GQA group sizes 1 / 2 / 4 and key masks, against fp32 torch on the same bf16 operands"""
    from kalle_audio_amd import ops
    from test_kernels_gpu import _attn_ref, _mk
    rng = np.random.RandomState(5)
    # (explicit cases for the fused backward with tail keys in the free rows of the query tiles: full tail of 16, tail keys masked,
    # group of 4, fewer than 112 queries)
    explicit = [(112, 144, 2, 4), (126, 130, 1, 4), (100, 140, 2, 2), (126, 129, 2, 2), (97, 128, 1, 2), (128, 128, 2, 4)]
    for it in range(14 + len(explicit)):
        Nq = int(rng.choice([1, 15, 126, 128, 129, 257, 300]))
        Nk = int(rng.choice([2, 17, 127, 128, 130, 256, 259]))
        Hkv = int(rng.choice([1, 2]))
        H = Hkv * int(rng.choice([1, 2, 4]))
        if it >= 14:
            Nq, Nk, Hkv, grp = explicit[it - 14]
            H = Hkv * grp
        B, D, Dc = 2, H * 64, Hkv * 64
        q = (_mk((B, Nq, D), dev, seed=300 + it) * 0.8).bfloat16()
        kv = (_mk((B, Nk, 2 * Dc), dev, seed=400 + it) * 0.8).bfloat16()
        dout = _mk((B, Nq, D), dev, seed=500 + it).bfloat16()
        mask = None
        if it % 2:
            mask = torch.rand(B, Nk, device=dev) > 0.3
            mask[:, 0] = True
            if it >= 14 and Nk > 128:
                mask[0, 128:] = False            # every tail key of the first clip masked
        qr, kvr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
        k, v = kvr.chunk(2, -1)
        ref = _attn_ref(qr, k, v, mask, None, H, Hkv)
        ref.backward(dout.float())
        out, lse = ops.attention_fwd(q, kv, kv, ldq=D, q_off=0, ldk=2 * Dc, k_off=0, ldv=2 * Dc, v_off=Dc, B=B, H=H, Hkv=Hkv,
                                     Nq=Nq, Nk=Nk, key_mask=mask)
        assert rel(out, ref) < 1e-2, (it, Nq, Nk, H, Hkv, rel(out, ref))
        dq, dkv = torch.zeros_like(q), torch.zeros_like(kv)
        ops.attention_bwd(q, kv, kv, out, dout, lse, dq, dkv, dkv, ldq=D, q_off=0, ldk=2 * Dc, k_off=0, ldv=2 * Dc, v_off=Dc,
                          B=B, H=H, Hkv=Hkv, Nq=Nq, Nk=Nk, key_mask=mask)
        assert rel(dq, qr.grad) < 2e-2 and rel(dkv, kvr.grad) < 2e-2, (it, Nq, Nk, H, Hkv, rel(dq, qr.grad), rel(dkv, kvr.grad))


def test_batched_context_projection_equals_per_layer(dev, monkeypatch):
    """the k | v projections of the conditioning for all layers in one GEMM (dit_ops.ContextKV: strided k / v columns into the
    attention kernels, dk | dv written in place, ONE context-gradient GEMM at the end of the backward pass) against one projection
    per layer: same output, same parameter gradients, same context gradient up to the order of the fp32 sum over layers"""
    from stable_audio_tools.models.transformer import ContinuousTransformer
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("KALLE_BATCH_CTX_KV", mode)
        ct = load_seeded(ContinuousTransformer(D, 3, dim_heads=64, cross_attend=True, cond_token_dim=DC, global_cond_dim=None), 91, dev)
        x = T(gu.make_input("x", (2, 40, D), 91), dev, True)
        ctx = T(gu.make_input("ctx", (2, 24, DC), 91), dev, True)
        cm = (torch.arange(24)[None, :] < torch.tensor([24, 17])[:, None]).to(dev)
        y = ct(x, context=ctx, context_mask=cm)
        y.backward(T(gu.make_input("dy", (2, 40, D), 91), dev))
        res[mode] = (y.detach().clone(), x.grad.clone(), ctx.grad.clone(), {n: p.grad.clone() for n, p in ct.named_parameters()})
        with torch.no_grad():
            res[mode + "i"] = ct(x.detach(), context=ctx.detach(), context_mask=cm)
        if mode == "1":     # the stacked projections do not outlive the forward that made them
            assert not hasattr(ctx, "_kalle_ckv")
            blk_alone = ct.layers[1](x.detach(), context=ctx.detach(), context_mask=cm)
            assert torch.isfinite(blk_alone).all()
    a, b = res["1"], res["0"]
    assert torch.equal(a[0], b[0]) and torch.equal(res["1i"], res["0i"]) and torch.equal(a[0], res["1i"])
    assert rel(a[1], b[1]) < 1e-6 and rel(a[2], b[2]) < 1e-5, (rel(a[1], b[1]), rel(a[2], b[2]))
    for n in a[3]:
        assert rel(a[3][n], b[3][n]) < 1e-5, (n, rel(a[3][n], b[3][n]))


@pytest.mark.parametrize("B,N,Dm", [(3, 126, 1536), (2, 7, 128), (1, 40, 260)])
def test_grad_cast_gate_backward_vs_torch(dev, B, N, Dm):
    """kalle_grad_cast: bf16 GEMM operand of the residual-stream gradient with the adaLN gate backward
    (transformer.py:667-668, 681-682: x_out = x_in + branch * sigmoid(1 - gate)), row mask, chunked row sums"""
    from kalle_audio_amd import ops
    g_ = torch.Generator().manual_seed(B * 1000 + N)
    g = torch.randn(B * N, Dm, generator=g_).to(dev)
    xi = torch.randn(B * N, Dm, generator=g_).to(dev)
    br = torch.randn(B * N, Dm, generator=g_).to(dev)
    gate = torch.randn(B, Dm, generator=g_).to(dev)
    sg = torch.sigmoid(1 - gate)
    xo = xi + br * sg.repeat_interleave(N, 0)
    mask = (torch.rand(B * N, generator=g_) > 0.2).to(dev)
    for rm in (None, mask):
        gm = g if rm is None else g * rm[:, None].float()
        gb, dg = ops.grad_cast(g, B, N, gate=gate, x_out=xo, x_in=xi, row_mask=rm)
        want_gb = gm * sg.repeat_interleave(N, 0)
        want_dg = -(1 - sg) * (gm * (xo - xi)).view(B, N, Dm).sum(1)
        assert rel(gb, want_gb) < 4e-3 and rel(dg, want_dg) < 1e-5, (rel(gb, want_gb), rel(dg, want_dg))
    gb, dg = ops.grad_cast(g, B, N, row_mask=mask)
    assert dg is None and rel(gb, g * mask[:, None].float()) < 4e-3
