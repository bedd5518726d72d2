"""-m gpu: Llasa.pack_sequences() - the decoder on the live rows of a right-padded batch only (PackRowsFn, varlen attention,
llama_ops.layer_fwd / layer_bwd with seqs=) - held to the checks the padded path is held to, with their methods and numbers
imported: the per-slice fp64 check of tests/test_grad_slices_gpu.py::test_llasa_slices (M = 3 yardsticks, seeded defects), the
trainer's 1e-5 agreement with plain autograd of test_llasa_through_trainer_matches_autograd, and the reference fixtures
model_llasa.npz / llasa_wide.npz at the bars of tests/test_round2_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_slices as gs  # noqa: E402
import test_grad_slices_gpu as tg  # noqa: E402
import test_round2_gpu as r2  # noqa: E402
from test_modules_gpu import T, _hf_grads, _llasa, _Tok, rel  # noqa: E402

gu = gs.gu
ARGS = ("input_ids", "audio_latents", "audio_distribution_l", "ids_mask", "audio_mask", "target_mask", "end_mask")


def _call(m, b, **kw):
    return m(*[b[k] for k in ARGS], **kw)


def _zero_hidden_head(m, hidden_shape, like):
    """what the head gives a zero hidden state: distribution_linear on zeros of the batch's own shape [B, L, D] (the same GEMM
    kernels at the same rows, so the comparison can be bit for bit)"""
    with torch.no_grad():
        return m.distribution_linear(torch.zeros(hidden_shape, device=like.device, dtype=like.dtype))


def _on_backward_done(layer, fn):
    """run fn() after `layer`'s backward, on the thread that ran it (autograd's: the plan words are per thread), in front of
    whatever hook the layer already carries"""
    prev = getattr(layer, "_kalle_on_backward_done", None)

    def hook(l):
        fn()
        if prev is not None:
            prev(l)
    layer._kalle_on_backward_done = hook


@pytest.mark.parametrize("c", gs.LLASA_CASES, ids=lambda c: c["id"])
def test_packed_llasa_slices(dev, tmp_path, c):
    """test_llasa_slices with pack_sequences() on: every parameter gradient slice, pre_mean at every valid position and both
    losses against grad_slices.llasa_reference in fp64; pre_mean at padded positions is the head of a zero hidden state"""
    from kalle_audio_amd import ops
    from kalle_audio_amd.model_sigmaVAE import Llasa
    ref = tg.llasa_ref(c["id"])
    lc = gs.llasa_config(c)
    d = tmp_path / "llama"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": c["lat"], "audio_proj_dim": lc["llama"]["hidden_size"]}, _Tok(310),
              use_flash_attention=False)
    sd = {k: torch.from_numpy(v) for k, v in ref["st"].items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    m = m.to(dev)
    assert m.pack_sequences() is m and m.base_model.model._pack is True
    b = {k: torch.from_numpy(v).to(dev) for k, v in ref["batch"].items()}
    out = _call(m, b, noise=torch.from_numpy(ref["eps"]).to(dev))
    assert ops.attn_last_plan() == 8 | c["hd"] << 8, hex(ops.attn_last_plan())              # the varlen forward ran
    seen = []
    _on_backward_done(m.base_model.model.layers[0], lambda: seen.append(ops.attn_last_plan()))
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    torch.cuda.synchronize()
    assert seen == [9 | 16 | c["hd"] << 8], [hex(w) for w in seen]                         # the varlen backward ran
    valid = ((b["ids_mask"] + b["audio_mask"]) > 0).cpu()
    rows = int(valid.sum())
    assert rows < valid.numel() and all(l._kalle_last_rows == -(-rows // 8) * 8 for l in m.base_model.model.layers)
    for k in ("audio_loss", "end_loss"):
        assert abs(out[k].item() - ref["g64"][k].item()) <= 1e-2 * abs(ref["g64"][k].item()), k
    g = {n: t.float().cpu() for n, t in _hf_grads(m).items()}
    pm = out["pre_mean"].detach().float().cpu()
    g["act:pre_mean"] = pm[valid]
    assert set(g) == set(ref["layout"]), set(g) ^ set(ref["layout"])
    tg.assert_slices(g, ref, None, f"llasa packed {c['id']}")
    assert len(tg.assert_defects_caught(ref)) == 5
    pad = pm[~valid]
    zero = _zero_hidden_head(m, b["input_ids"].shape + (m.hidden_size,), out["pre_mean"]).float().cpu()
    assert torch.isfinite(pad).all() and torch.equal(pad, zero[~valid])


def _packed_autograd(m, b, eps):
    m.zero_grad(set_to_none=True)
    out = _call(m, b, noise=eps)
    (out["audio_loss"] + 0.5 * out["end_loss"]).backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return want


def test_packed_llasa_through_trainer(dev, tmp_path):
    """engine.DataParallelTrainer over the packed model: _kalle_last_rows is the packed row count (a multiple of 8), so the grouped
    weight-gradient launch runs; gradients equal packed plain autograd within the 1e-5 of
    test_llasa_through_trainer_matches_autograd; two micro-batches with different packed row counts in one accumulation window
    give the sum of the two"""
    from kalle_audio_amd import ops
    from kalle_audio_amd.engine import DataParallelTrainer
    m, lc, _ = _llasa(dev, tmp_path)
    m.pack_sequences()
    bs, epss, wants, rows = [], [], [], []
    for seed, kw in ((40, {}), (41, dict(B=2, L=33))):
        b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch(lc, seed, **kw).items()}
        eps = T(gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), seed), dev)
        bs.append(b), epss.append(eps), wants.append(_packed_autograd(m, b, eps))
        live = int(((b["ids_mask"] + b["audio_mask"]) > 0).sum())
        rows.append(-(-live // 8) * 8)
        assert live < b["ids_mask"].numel() and m.base_model.model.layers[0]._kalle_last_rows == rows[-1]
    assert rows[0] != rows[1]
    tr = DataParallelTrainer(m, lr=1e-3, optimizer="AdamW", weight_decay=0.0)
    before = tr.flat.param.clone()
    tr.lr = 0.0                                                              # gradients only
    p0 = m.base_model.model.layers[0]
    plans = []
    _on_backward_done(p0, lambda: plans.append(ops.wgrad_group_last_plan()))
    out = _call(m, bs[0], noise=epss[0])
    tr.backward(out["audio_loss"] + 0.5 * out["end_loss"])
    for n, p in m.named_parameters():
        assert rel(tr.flat.grad_view(n), wants[0][n]) < 1e-5, n
    hid, inner, ld = lc["llama"]["hidden_size"], lc["llama"]["intermediate_size"], p0.self_attn.qkv_proj.weight.shape[0]
    asked = ops.wgrad_group_plan([(rows[0], hid, inner), (rows[0], 2 * inner, hid), (rows[0], hid, hid), (rows[0], ld, hid)], overwrite=True)
    ran = plans[0]
    assert ran["tiles"] > 0 and ran["tiles"] == asked["tiles"], (ran, asked)   # the grouped launch ran, at the packed row count
    # one accumulation window of two micro-batches with different packed row counts.  Each micro-batch agrees with its own
    # autograd gradient to 1e-5 (above); the window adds the second onto the first in fp32 (one rounding per element, as the
    # reference sum does), so the sum agrees to 1e-5 of the summands' size plus those roundings
    tr.grad_accum_steps, tr.micro = 2, 0
    for b, eps in zip(bs, epss):
        out = _call(m, b, noise=eps)
        tr.backward(out["audio_loss"] + 0.5 * out["end_loss"])
    for n, p in m.named_parameters():
        w0, w1 = wants[0][n].float(), wants[1][n].float()
        bound = 1e-5 * ((w0.norm() + w1.norm()) / ((w0 + w1).norm() + 1e-30)).item() + 2.0 ** -23
        assert rel(tr.flat.grad_view(n), w0 + w1) < bound, (n, rel(tr.flat.grad_view(n), w0 + w1), bound)
    assert torch.equal(tr.flat.param, before)


def test_packed_model_llasa_fixture(dev, tmp_path):
    """model.Llasa.pack_sequences(): losses, pre_mean / pre_log_scale at valid positions and every gradient against
    tests/golden/model_llasa.npz at the bars (and with the inputs) of test_round2_gpu.test_model_llasa_two_gaussian_kl"""
    m, lc = r2._model_llasa(dev, tmp_path)
    assert m.pack_sequences() is m
    f = r2.fx("model_llasa")
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch_long(lc, 54, B=3, L=48, label_mult=2).items()}
    out = _call(m, b)
    assert m.base_model.model.layers[0]._kalle_last_rows < 3 * 48
    assert set(out) == {"audio_loss", "end_loss", "pre_mean", "pre_log_scale"}
    assert abs(out["audio_loss"].item() - float(f["audio_loss"])) < 1e-2 * abs(float(f["audio_loss"]))
    assert abs(out["end_loss"].item() - float(f["end_loss"])) < 1e-2 * abs(float(f["end_loss"]))
    valid = (b["ids_mask"] + b["audio_mask"]) > 0
    for key in ("pre_mean", "pre_log_scale"):
        ref = torch.from_numpy(f[key]).to(dev)
        assert rel(out[key][valid], ref[valid]) < 1e-2, (key, rel(out[key][valid], ref[valid]))
    zero = _zero_hidden_head(m, b["input_ids"].shape + (m.hidden_size,), out["pre_mean"])
    lat = zero.shape[-1] // 2
    for key, z in (("pre_mean", zero[..., :lat]), ("pre_log_scale", zero[..., lat:])):
        assert torch.isfinite(out[key]).all() and torch.equal(out[key][~valid], z[~valid]), key
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = _hf_grads(m)
    r2.check_digests(f, g, 16)
    for k in f.files:
        if k.startswith("grad/"):
            assert rel(g[k[5:]], f[k]) < 2e-2, (k, rel(g[k[5:]], f[k]))


def test_packed_llasa_wide_fixture(dev, tmp_path):
    """model_sigmaVAE.Llasa.pack_sequences() against tests/golden/llasa_wide.npz at the bars of test_llasa_wide_ragged"""
    m, lc = r2._llasa_wide(dev, tmp_path)
    m.pack_sequences()
    f = r2.fx("llasa_wide")
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch_long(lc, 53).items()}
    eps = T(gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), 53), dev)
    out = _call(m, b, noise=eps)
    assert abs(out["audio_loss"].item() - float(f["audio_loss"])) < 1e-2 * float(f["audio_loss"])
    assert abs(out["end_loss"].item() - float(f["end_loss"])) < 1e-2 * float(f["end_loss"])
    valid = (b["ids_mask"] + b["audio_mask"]) > 0
    ref = torch.from_numpy(f["pre_mean"].astype(np.float32)).to(dev)
    assert rel(out["pre_mean"][valid], ref[valid]) < 1e-2, rel(out["pre_mean"][valid], ref[valid])
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = _hf_grads(m)
    assert r2.check_digests(f, g, 16) == 26
    for k in f.files:
        if k.startswith("grad/"):
            assert rel(g[k[5:]], f[k]) < 2e-2, (k, rel(g[k[5:]], f[k]))


def test_flag_off_is_bit_identical_and_a_left_padded_mask_raises(dev, tmp_path):
    """With the flag off again the padded step is bit for bit what it was before pack_sequences() was ever called: pre_mean and
    every matrix gradient (the GEMMs and the attention kernels: no atomics).  What the kernels sum ATOMICALLY - the two losses
    (per-block sums of the KL kernel), the vector gradients (column sums: biases, norm scales) and the embedding's scatter-add -
    is not reproducible bit for bit between two runs of the padded step on the code before this feature either (measured there,
    four runs: audio_loss 2.4e-7 and the gradient of audio_linear.bias 8.5e-9 relative, intermittently); those are held to the
    reordering of an fp32 sum instead: n 2^-24 of the tensor's largest entry for the n <= B L addends."""
    m, lc, _ = _llasa(dev, tmp_path)
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch(lc, 40).items()}
    eps = T(gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), 40), dev)

    def run():
        m.zero_grad(set_to_none=True)
        out = _call(m, b, noise=eps)
        (out["audio_loss"] + 0.5 * out["end_loss"]).backward()
        torch.cuda.synchronize()
        return ({k: out[k].detach().clone() for k in ("audio_loss", "end_loss", "pre_mean")},
                {n: p.grad.clone() for n, p in m.named_parameters()})

    o0, g0 = run()
    exact = {"pre_mean"} | {n for n, g in g0.items() if g.dim() == 2 and "embed_tokens" not in n}
    assert len(exact) == 1 + 4 * len(m.base_model.model.layers) + 3
    assert m.pack_sequences(True) is m
    o1, _ = run()
    assert not torch.equal(o1["pre_mean"], o0["pre_mean"])                   # (the packed path did run: padded positions differ)
    # a left-padded row: no silent fall-back
    bad = dict(b)
    bad["ids_mask"], bad["audio_mask"] = b["ids_mask"].flip(1).contiguous(), b["audio_mask"].flip(1).contiguous()
    with pytest.raises(ValueError, match="row 1 "):
        _call(m, bad, noise=eps)
    assert m.pack_sequences(False) is m
    o2, g2 = run()
    reorder = b["ids_mask"].numel() * 2.0 ** -24
    for k, (a, c) in {**{k: (o0[k], o2[k]) for k in o0}, **{n: (g0[n], g2[n]) for n in g0}}.items():
        if k in exact:
            assert torch.equal(a, c), k
        else:
            assert (a - c).abs().max().item() <= reorder * a.abs().max().item(), (k, (a - c).abs().max().item())
    # a mask of ones whose row count is a multiple of 8 takes the padded path (nothing to gain); with no mask likewise
    model = m.base_model.model
    x = torch.randn(2, 16, lc["llama"]["hidden_size"], device=dev)
    with torch.no_grad():
        want = model(inputs_embeds=x, attention_mask=torch.ones(2, 16, device=dev))[0]
        m.pack_sequences()
        got = model(inputs_embeds=x, attention_mask=torch.ones(2, 16, device=dev))[0]
        none = model(inputs_embeds=x)[0]
    assert torch.equal(want, got) and torch.isfinite(none).all()
