"""-m gpu: weight-only e4m3 decoding at module level - LlamaModel.quantize_decode_weights / Llasa.quantize_decoder - on the tiny
Llama configs of tests/test_llasa_batch_gpu.py (head dims 64 and 128).  The decoder's linear weights are overwritten with
"lossless" weights (tests/fp8_refs.py: each row 2^e_n x e4m3 values holding +-448, exact in bf16 and reproduced exactly by the
quantiser), so the quantised and the bf16 decoder hold the SAME values and differ only in summation order: the comparisons take the
tolerances that file already holds the batched path to.  The plumbing is checked bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_refs as f8  # noqa: E402
from test_llasa_batch_gpu import build, fixed_noise, prompts, rel  # noqa: E402

pytestmark = pytest.mark.gpu


def projections(layer):
    return (layer.self_attn.qkv_proj.weight, layer.self_attn.o_proj.weight, layer.mlp.up_gate_proj.weight, layer.mlp.down_proj.weight)


def make_lossless(model, seed=21):
    """rows of 2^-11 .. 2^-9 x e4m3 values: |w| <= 0.875, of the size the decoder's own initialisation has at these widths"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in model.layers:
            for w in projections(layer):
                w.copy_(f8.lossless_weights(w.shape[0], w.shape[1], g, emin=-11, emax=-9)[0].float())


def lossless_model(hd, dev, tmp_path):
    m, d, D = build(hd, dev, tmp_path)
    make_lossless(m.base_model.model)
    return m, d, D


@pytest.mark.parametrize("hd", [64, 128])
def test_quantised_copies_of_lossless_weights_hold_the_same_values(dev, tmp_path, hd):
    from kalle_audio_amd import llama_ops as LO
    m, _, _ = lossless_model(hd, dev, tmp_path)
    tab = f8.decode_table().to(dev)
    for layer in m.base_model.model.layers:
        for w in projections(layer):
            w8, s = LO.e4m3_of(w)
            assert torch.equal(tab[w8.long()] * s.double()[:, None], w.detach().double())
            assert torch.equal(torch.log2(s.double()), torch.log2(s.double()).round())


@pytest.mark.parametrize("hd", [64, 128])
def test_forward_cached_and_batch_match_the_bf16_path(dev, tmp_path, hd):
    m, _, D = lossless_model(hd, dev, tmp_path)
    model = m.base_model.model
    torch.manual_seed(3)
    lens = (20, 5, 33)
    xs = [torch.randn(1, n + 2, D, device=dev) for n in lens]

    def run(fmt):
        model.quantize_decode_weights(fmt)
        singles, cache = [], model.init_cache_batch(3, 48, dev)
        for r, (x, n) in enumerate(zip(xs, lens)):
            one = model.init_cache(48, dev)
            model.forward_cached(x[:, :n].contiguous(), one)                       # prefill: bf16 in either mode
            model.prefill_row(x[:, :n].contiguous(), cache, r)
            singles.append([model.forward_cached(x[:, n + i:n + i + 1].contiguous(), one) for i in range(2)])
            assert one["plan"].get("fmt") == fmt
        batch = [model.forward_cached_batch(torch.cat([x[:, n + i:n + i + 1] for x, n in zip(xs, lens)], 0).contiguous(), cache)
                 for i in range(2)]
        assert cache["plan"].get("fmt") == fmt and cache["len"] == [22, 7, 35]
        return singles, batch, cache

    s16, b16, c16 = run(None)
    s8, b8, c8 = run("e4m3")
    for a, b in zip(c16["kv"], c8["kv"]):
        for r, n in enumerate(lens):
            assert torch.equal(a[r, :n], b[r, :n])                                  # the prefilled rows: the same kernels
    for r in range(3):
        for i in range(2):
            print("row", r, "step", i, "forward_cached e4m3 vs bf16", rel(s8[r][i], s16[r][i]), "batch", rel(b8[i][r], b16[i][r]))
            assert rel(s8[r][i], s16[r][i]) < 1e-2, (r, i, rel(s8[r][i], s16[r][i]))
            assert rel(b8[i][r], b16[i][r]) < 1e-2, (r, i, rel(b8[i][r], b16[i][r]))


@pytest.mark.parametrize("hd", [64, 128])
def test_infer_and_infer_batch_match_the_bf16_path(dev, tmp_path, hd):
    m, d, _ = lossless_model(hd, dev, tmp_path)
    ps = prompts(dev, d)
    noise = torch.randn(12, 1, 1, d, device=dev)

    def run(fmt):
        assert m.quantize_decoder(fmt) is m
        fixed_noise(m, noise)
        batch = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=8)
        fixed_noise(m, noise)
        return batch, m.infer(ps[0][0], ps[0][1], end_disp_kl_thres=-1.0, max_length=8)

    b16, o16 = run(None)
    b8, o8 = run("e4m3")
    assert o8.shape == o16.shape == (1, d, 7)
    print("infer e4m3 vs bf16", rel(o8, o16))
    assert rel(o8, o16) < 2e-2, rel(o8, o16)
    for r in range(3):
        print("prompt", r, "infer_batch e4m3 vs bf16", rel(b8[r], b16[r]))
        assert b8[r].shape == b16[r].shape and rel(b8[r], b16[r]) < 2e-2, (r, rel(b8[r], b16[r]))


@pytest.mark.parametrize("hd", [64, 128])
def test_module_step_is_the_ops_step_on_the_ops_quantiser(dev, tmp_path, hd):
    """bit for bit, one row and three rows, on the model's own (random, not lossless) weights"""
    from kalle_audio_amd import llama_ops as LO, ops
    m, _, D = build(hd, dev, tmp_path)
    model = m.base_model.model.quantize_decode_weights("e4m3")
    torch.manual_seed(4)
    x = torch.randn(1, 6, D, device=dev)

    def tensors(kvs):
        out = []
        for layer, kv in zip(model.layers, kvs):
            p = LO.layer_params(layer)
            q = [ops.quantize_rows_e4m3(w) for w in (p.wqkv, p.wo, p.wug, p.wdown)]
            out.append((p.g1, *q[0], *q[1], p.g2, *q[2], *q[3], kv))
        return out, p

    with torch.no_grad():
        cache = model.init_cache(16, dev)
        model.forward_cached(x[:, :5].contiguous(), cache)
        kvs = [k.clone() for k in cache["kv"]]
        got = model.forward_cached(x[:, 5:].contiguous(), cache)
        ts, p = tensors(kvs)
        plan = ops.llama_decode_plan(ts, p.H, p.Hkv, model.cfg["intermediate_size"], dev, head_dim=hd)
        want = model.norm(ops.llama_decode_step(plan, x[0, 5].float().contiguous(), 5, 16, cache["rope"], p.eps).view(1, 1, D))
        assert torch.equal(got, want)
        for a, b in zip(cache["kv"], kvs):
            assert torch.equal(a, b) and torch.isfinite(a[5]).all() and a[5].abs().sum() > 0
        # three rows, the middle one inactive
        bc = model.init_cache_batch(3, 16, dev)
        for r, n in enumerate((5, 2, 3)):
            model.prefill_row(x[:, :n].contiguous(), bc, r)
        kvs = [k.clone() for k in bc["kv"]]
        xb = torch.randn(3, 1, D, device=dev)
        got = model.forward_cached_batch(xb, bc, active=[True, False, True])
        ts, p = tensors(kvs)
        plan = ops.llama_decode_plan(ts, p.H, p.Hkv, model.cfg["intermediate_size"], dev, head_dim=hd, rows=3)
        want = model.norm(ops.llama_decode_step(plan, xb.view(3, D).float().contiguous(), [5, -1, 3], 16, bc["rope"], p.eps).view(3, 1, D))
        assert torch.equal(got, want)
        for a, b in zip(bc["kv"], kvs):
            assert torch.equal(a, b)


def test_a_changed_weight_is_requantised_at_the_next_step(dev, tmp_path):
    """weight.mul_(2) on one projection: its scales exactly doubled and its codes unchanged at the next step, the other copies not
    re-made; the same through ops.WEIGHTS_EPOCH for a write torch does not see"""
    from kalle_audio_amd import ops
    m, _, D = build(64, dev, tmp_path)
    model = m.base_model.model.quantize_decode_weights("e4m3")
    x = torch.randn(1, 1, D, device=dev)
    with torch.no_grad():
        cache = model.init_cache(8, dev)
        a = model.forward_cached(x, cache)
        keep0 = cache["plan"]["keep"]
        model.layers[1].self_attn.o_proj.weight.mul_(2)
        b = model.forward_cached(x, cache)
        keep1 = cache["plan"]["keep"]
    assert keep1 is not keep0 and not torch.equal(a, b)
    for l in range(2):
        for i in (1, 2, 3, 4, 6, 7, 8, 9):               # (codes, scale) of qkv, o, up|gate, down
            if l == 1 and i in (3, 4):
                continue
            assert keep1[l][i] is keep0[l][i], (l, i, "a copy of an unchanged weight was re-made")
    assert torch.equal(keep1[1][3], keep0[1][3]) and torch.equal(keep1[1][4], keep0[1][4] * 2)
    assert keep1[1][3] is not keep0[1][3]
    with torch.no_grad():
        w = model.layers[0].mlp.down_proj.weight
        w.data.view(-1)[:w.shape[1]].mul_(4)            # (.data: no version bump - what a raw-pointer optimiser step looks like)
        w._kalle_bf16 = None                            # (its bf16 compute copy follows, as the optimiser's pinned one does)
        ops.WEIGHTS_EPOCH += 1
        model.forward_cached(x, cache)
        keep2 = cache["plan"]["keep"]
    assert torch.equal(keep2[0][8], keep1[0][8]) and torch.equal(keep2[0][9][0], keep1[0][9][0] * 4)
    assert torch.equal(keep2[0][9][1:], keep1[0][9][1:])


@pytest.mark.parametrize("hd", [64, 128])
def test_none_restores_the_bf16_path_bit_for_bit(dev, tmp_path, hd):
    m, d, D = build(hd, dev, tmp_path)
    model = m.base_model.model
    x = torch.randn(1, 7, D, device=dev)

    def run():
        cache = model.init_cache(16, dev)
        outs = [model.forward_cached(x[:, :5].contiguous(), cache)]
        outs += [model.forward_cached(x[:, 5 + i:6 + i].contiguous(), cache) for i in range(2)]
        return outs, cache

    never, _ = run()
    model.quantize_decode_weights("e4m3")
    q8, cache = run()
    assert cache["plan"]["fmt"] == "e4m3" and torch.equal(q8[0], never[0]) and not torch.equal(q8[1], never[1])
    model.quantize_decode_weights(None)
    # a cache whose plan was built for the other format gets a new plan, in either direction
    cache["len"] = 5
    again = model.forward_cached(x[:, 5:6].contiguous(), cache)
    assert cache["plan"].get("fmt") is None and torch.equal(again, never[1])
    model.quantize_decode_weights("e4m3")
    cache["len"] = 5
    assert torch.equal(model.forward_cached(x[:, 5:6].contiguous(), cache), q8[1]) and cache["plan"]["fmt"] == "e4m3"
    assert all(hasattr(w, "_kalle_e4m3") for layer in model.layers for w in projections(layer))
    model.quantize_decode_weights(None)
    assert not any(hasattr(w, "_kalle_e4m3") for layer in model.layers for w in projections(layer)), "None keeps the e4m3 copies alive"
    back, _ = run()
    for a, b in zip(back, never):
        assert torch.equal(a, b)


def test_refusals_name_what_is_supported(dev, tmp_path):
    from kalle_audio_amd.model_sigmaVAE import LlamaModel
    m, _, _ = build(64, dev, tmp_path)
    for fmt in ("e5m2", "int8", "mxfp4"):
        with pytest.raises(NotImplementedError, match="e4m3"):
            m.quantize_decoder(fmt)
    assert m.base_model.model._decode_fmt is None
    odd = LlamaModel(dict(m.base_model.model.cfg, intermediate_size=264, num_hidden_layers=1))
    with pytest.raises(NotImplementedError, match="intermediate_size=264"):
        odd.quantize_decode_weights("e4m3")
    assert odd._decode_fmt is None
    assert odd.quantize_decode_weights(None) is odd
