"""-m gpu: batched KV-cached generation at module level - LlamaModel.init_cache_batch / prefill_row / forward_cached_batch and
Llasa.infer_batch - against the single-sequence path (forward_cached, infer) on the tiny Llama configs of the existing module
tests (head dims 64 and 128)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def build(hd, dev, tmp_path):
    """(model, latent_dim, hidden size)"""
    if hd == 64:
        from test_modules_gpu import _llasa
        m, lc, _ = _llasa(dev, tmp_path)
        return m, lc["latent_dim"], 128
    from test_llama_hd128_gpu import _llasa
    m, lc = _llasa(dev, tmp_path)
    return m, lc["latent_dim"], 256


def fixed_noise(m, noise):
    """m.sample draws frame i's noise from noise[i] for every row, as the existing infer tests substitute it"""
    from kalle_audio_amd import ops
    it = iter(noise)
    m.sample = lambda mean, dist_type='fix', noise=None, it=it: ops.axpby(
        mean.float().contiguous(), next(it).expand(mean.shape).float().contiguous(), 1.0, 0.5)


def prompts(dev, d):
    g = torch.Generator(device=dev).manual_seed(11)
    return [(torch.randint(0, 300, (9,), device=dev, generator=g), torch.randn(1, 5, d, device=dev, generator=g)),
            (torch.randint(0, 300, (4,), device=dev, generator=g), None),
            (torch.randint(0, 300, (17,), device=dev, generator=g), torch.randn(1, 2, d, device=dev, generator=g))]


@pytest.mark.parametrize("hd", [64, 128])
def test_forward_cached_batch_matches_forward_cached_per_sequence(dev, tmp_path, hd):
    m, _, D = build(hd, dev, tmp_path)
    model = m.base_model.model
    torch.manual_seed(3)
    lens = (20, 5, 33)
    xs = [torch.randn(1, n + 1, D, device=dev) for n in lens]
    with torch.no_grad():
        cache = model.init_cache_batch(3, 48, dev)
        assert cache["kv"][0].shape == (3, 48, 2 * model.cfg["num_key_value_heads"] * hd)
        want = []
        for r, (x, n) in enumerate(zip(xs, lens)):
            one = model.init_cache(48, dev)
            a = model.forward_cached(x[:, :n].contiguous(), one)
            b = model.prefill_row(x[:, :n].contiguous(), cache, r)
            assert torch.equal(a, b)                                           # the same kernels on the row's slice
            want.append(model.forward_cached(x[:, n:n + 1].contiguous(), one))
            for kb, k1 in zip(cache["kv"], one["kv"]):
                assert torch.equal(kb[r, :n], k1[:n])
        got = model.forward_cached_batch(torch.cat([x[:, n:n + 1] for x, n in zip(xs, lens)], 0).contiguous(), cache)
    assert cache["len"] == [21, 6, 34] and cache["plan"]["R"] == 3 and cache["plan"]["head_dim"] == hd
    assert got.shape == (3, 1, D)
    for r in range(3):
        print("row", r, "batch vs single", rel(got[r], want[r][0]))
        assert rel(got[r], want[r][0]) < 1e-2, (r, rel(got[r], want[r][0]))
    # an inactive row: cache, length and the other rows' results unchanged
    with torch.no_grad():
        before = [k.clone() for k in cache["kv"]]
        x = torch.randn(3, 1, D, device=dev)
        model.forward_cached_batch(x, cache, active=[True, False, True])
    assert cache["len"] == [22, 6, 35]
    for k, k0 in zip(cache["kv"], before):
        assert torch.equal(k[1], k0[1])
        assert not torch.equal(k[0, 21], k0[0, 21])


@pytest.mark.parametrize("hd", [64, 128])
def test_infer_batch_matches_infer_per_prompt(dev, tmp_path, hd):
    m, d, _ = build(hd, dev, tmp_path)
    ps = prompts(dev, d)
    noise = torch.randn(12, 1, 1, d, device=dev)
    fixed_noise(m, noise)
    outs = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=8)
    assert len(outs) == 3
    for r, (ids, lat) in enumerate(ps):
        fixed_noise(m, noise)
        one = m.infer(ids, lat, end_disp_kl_thres=-1.0, max_length=8)
        assert outs[r].shape == one.shape == (1, d, 7)
        print("prompt", r, "infer_batch vs infer", rel(outs[r], one))
        assert rel(outs[r], one) < 2e-2, (r, rel(outs[r], one))
    # one prompt is infer itself
    fixed_noise(m, noise)
    a = m.infer_batch(ps[:1], end_disp_kl_thres=-1.0, max_length=8)
    fixed_noise(m, noise)
    b = m.infer(ps[0][0], ps[0][1], end_disp_kl_thres=-1.0, max_length=8)
    assert len(a) == 1 and torch.equal(a[0], b)


def test_infer_batch_stops_one_row_and_leaves_the_others_alone(dev, tmp_path):
    """KL(N(m, s) || N(1, e)) grows with (m - 1)^2: a forward hook on distribution_linear adds 100 to the predicted mean (KL ~ 660)
    wherever a row must go on and nothing where row 1 must stop (its KL of a mean of order 1 stays far below the threshold of 300):
    row 1 stops at the fifth frame (i = 4, the first the rule allows), rows 0 and 2 run to max_length"""
    m, d, _ = build(64, dev, tmp_path)
    model = m.base_model.model
    ps = prompts(dev, d)
    noise = torch.randn(12, 1, 1, d, device=dev)

    def run(row1_stops):
        fixed_noise(m, noise)
        frame = [0]
        caches, snaps = [], []

        def bump(mod, inp, out):
            b = torch.full_like(out, 100.0)
            if row1_stops and frame[0] == 4:
                b[1] = 0.0
            frame[0] += 1
            return out + b

        init, fwd = model.init_cache_batch, model.forward_cached_batch

        def init_spy(*a, **k):
            caches.append(init(*a, **k))
            return caches[-1]

        def fwd_spy(x, cache, active=None):
            if active is not None and not active[1] and not snaps:
                snaps.append(([k[1].clone() for k in cache["kv"]], cache["len"][1]))
            return fwd(x, cache, active)

        h = m.distribution_linear.register_forward_hook(bump)
        model.init_cache_batch, model.forward_cached_batch = init_spy, fwd_spy
        try:
            outs = m.infer_batch(ps, end_disp_kl_thres=300.0, max_length=8)
        finally:
            h.remove()
            del model.init_cache_batch, model.forward_cached_batch
        return outs, caches[0], snaps

    outs, cache, snaps = run(True)
    assert [o.shape[2] for o in outs] == [7, 4, 7], [o.shape for o in outs]
    assert len(snaps) == 1                                         # row 1's cache right after its stop ...
    for k, k0 in zip(cache["kv"], snaps[0][0]):
        assert torch.equal(k[1], k0)                               # ... and after the run: bit for bit
    assert cache["len"][1] == snaps[0][1] == len(ps[1][0]) + 4     # prompt + the four frames fed back
    assert cache["len"][0] == len(ps[0][0]) + 5 + 7 and cache["len"][2] == len(ps[2][0]) + 2 + 7
    free, _, none = run(False)
    assert [o.shape[2] for o in free] == [7, 7, 7] and not none
    assert torch.equal(outs[0], free[0]) and torch.equal(outs[2], free[2])
    assert torch.equal(outs[1], free[1][:, :, :4])


def test_infer_batch_processes_long_lists_in_groups(dev, tmp_path):
    m, d, _ = build(64, dev, tmp_path)
    g = torch.Generator(device=dev).manual_seed(5)
    ps = [(torch.randint(0, 300, (3 + i % 4,), device=dev, generator=g), None) for i in range(17)]
    outs = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=3)
    assert len(outs) == 17 and all(o.shape == (1, d, 2) for o in outs)
    assert m.infer_batch([]) == []
