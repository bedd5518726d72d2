"""-m gpu: Llasa.infer / Llasa.infer_batch with device_head=True (one decode-step call plus one kalle_llasa_frame_head_rows call per
frame) against the host head on the tiny head-dim 64 and 128 models of the existing Llasa tests: the generated latents, the stop
rule, stop_lag=1 against stop_lag=0 bit for bit, and the plumbing (final_norm=False, a changed head weight, the refusals)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_llasa_batch_gpu import build, fixed_noise, prompts, rel  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 8
# the stop tests: distribution_linear[2].weight times STOP_SCALE spreads the predicted means, and with them the per-frame KLs of
# the three rows, far enough apart for rows to stop at different frames; STOP_SEED draws the noise
STOP_FRAMES, STOP_SEED, STOP_SCALE = 10, 0, 100.0


def no_host_head(m):
    """m.sample and distribution_linear.forward raise: the device path must not reach them"""
    def boom(*a, **k):
        raise AssertionError("the host head ran under device_head=True")
    m.sample = boom
    return m.distribution_linear.register_forward_pre_hook(boom)


def host_and_device(m, ps, noise, dev_noise, **kw):
    """(host infer_batch outputs, device_head outputs) under the same noise"""
    fixed_noise(m, noise)
    host = m.infer_batch(ps, **kw)
    del m.sample
    h = no_host_head(m)
    try:
        devo = m.infer_batch(ps, device_head=True, noise=dev_noise, **kw)
    finally:
        h.remove()
        del m.sample
    return host, devo


@pytest.mark.parametrize("fmt", [None, "e4m3"], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("hd", [64, 128])
def test_device_head_matches_the_host_head(dev, tmp_path, hd, fmt):
    """infer_batch (three prompts, the R-row step) and infer (the one-row step): same shapes, rel < 2e-2 - the bound
    test_infer_batch_matches_infer_per_prompt holds "same arithmetic, other summation order, 8 frames" to"""
    m, d, _ = build(hd, dev, tmp_path)
    if fmt:
        m.quantize_decoder(fmt)
    ps = prompts(dev, d)
    noise = torch.randn(12, 1, 1, d, device=dev)
    host, devo = host_and_device(m, ps, noise, noise.view(12, 1, d)[:FRAMES], end_disp_kl_thres=-1.0, max_length=FRAMES)
    assert len(devo) == 3
    for r in range(3):
        assert devo[r].shape == host[r].shape == (1, d, FRAMES - 1)
        print("prompt", r, "infer_batch device head vs host head", rel(devo[r], host[r]))
        assert rel(devo[r], host[r]) < 2e-2, (r, rel(devo[r], host[r]))
    ids, lat = ps[0]
    fixed_noise(m, noise)
    one = m.infer(ids, lat, end_disp_kl_thres=-1.0, max_length=FRAMES)
    del m.sample
    h = no_host_head(m)
    try:
        got = m.infer(ids, lat, end_disp_kl_thres=-1.0, max_length=FRAMES, device_head=True, noise=noise.view(12, 1, d)[:FRAMES])
    finally:
        h.remove()
        del m.sample
    assert got.shape == one.shape == (1, d, FRAMES - 1) and got.stride() == one.stride()
    print("infer device head vs host head", rel(got, one))
    assert rel(got, one) < 2e-2, rel(got, one)


@pytest.mark.parametrize("hd", [64, 128])
def test_seeded_run_draws_as_the_host_path_does(dev, tmp_path, hd):
    """noise=None: one torch.randn((R, 1, d)) per frame, the shape and order of sample(), so the same seed gives the host path's
    noise - and leaves the generator where the host path leaves it"""
    m, d, _ = build(hd, dev, tmp_path)
    ps = prompts(dev, d)
    for run in (lambda **k: m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=FRAMES, **k),
                lambda **k: [m.infer(ps[2][0], ps[2][1], end_disp_kl_thres=-1.0, max_length=FRAMES, **k)]):
        torch.manual_seed(7)
        host = run()
        after_host = torch.randn(4, device=dev)
        torch.manual_seed(7)
        devo = run(device_head=True)
        after_dev = torch.randn(4, device=dev)
        assert torch.equal(after_host, after_dev)
        for a, b in zip(devo, host):
            assert a.shape == b.shape
            print("seeded device head vs host head", rel(a, b))
            assert rel(a, b) < 2e-2, rel(a, b)


def kl_of(mean):
    """the stop KL of model_sigmaVAE.py:135-139 from a predicted mean [..., d], float64"""
    s, e = 0.5, math.e
    return (math.log(e / s) + (s * s + (mean.double() - 1.0) ** 2) / (2 * e * e) - 0.5).mean(-1)


def free_run_kls(m, ps, noise):
    """per-frame, per-row KL of a free run (threshold -1) on the host path and on the device path: [frames, R] each"""
    from kalle_audio_amd import ops
    host = []
    h = m.distribution_linear.register_forward_hook(lambda mod, inp, out: host.append(kl_of(out.view(len(ps), -1))))
    fixed_noise(m, noise)
    try:
        m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=STOP_FRAMES)
    finally:
        h.remove()
        del m.sample
    devk, head = [], ops.llasa_frame_head

    def spy(*a, **k):
        out = head(*a, **k)
        devk.append(out[2].double().clone())
        return out

    ops.llasa_frame_head = spy
    try:
        m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=STOP_FRAMES, device_head=True, noise=noise.view(-1, 1, noise.shape[-1]))
    finally:
        ops.llasa_frame_head = head
    return torch.stack(host).cpu(), torch.stack(devk).cpu()


def stop_setup(m, dev, d, seed=STOP_SEED, scale=STOP_SCALE):
    with torch.no_grad():
        m.distribution_linear[2].weight.mul_(scale)
    ps = prompts(dev, d)
    noise = torch.randn(STOP_FRAMES, 1, 1, d, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    host, devk = free_run_kls(m, ps, noise)
    assert host.shape == devk.shape == (STOP_FRAMES, 3)
    v = host[4:].reshape(-1).sort().values
    gaps = v[1:] - v[:-1]
    i = int(gaps.argmax())
    thres, gap, diff = float((v[i] + v[i + 1]) / 2), float(gaps[i]), float((host - devk).abs().max())
    print("free-run KL: widest gap", gap, "at", thres, "largest device-vs-host difference", diff, "ratio", gap / diff)
    return ps, noise, thres, gap, diff


def test_stop_rule_stops_the_rows_the_host_path_stops(dev, tmp_path):
    """the threshold sits in the widest gap of the host path's free-run KLs at i >= 4, a gap at least 20 x the largest difference
    between the two paths' KLs, so both paths must stop every row at the same frame"""
    m, d, _ = build(64, dev, tmp_path)
    ps, noise, thres, gap, diff = stop_setup(m, dev, d)
    assert gap >= 20 * diff, (gap, diff)
    host, devo = host_and_device(m, ps, noise, noise.view(STOP_FRAMES, 1, d), end_disp_kl_thres=thres, max_length=STOP_FRAMES)
    lens = [o.shape[2] for o in host]
    print("frames per row", lens)
    assert [o.shape[2] for o in devo] == lens
    assert min(lens) < max(lens), ("no row stops while another goes on", lens)
    for a, b in zip(devo, host):
        assert rel(a, b) < 2e-2, rel(a, b)
    ids, lat = ps[lens.index(min(lens))]
    r = lens.index(min(lens))
    one = m.infer(ids, lat, end_disp_kl_thres=thres, max_length=STOP_FRAMES, device_head=True, noise=noise.view(STOP_FRAMES, 1, d))
    assert one.shape[2] == lens[r]


@pytest.mark.parametrize("early", [True, False], ids=["early-stop", "to-max-length"])
def test_stop_lag_one_returns_the_bits_of_stop_lag_zero(dev, tmp_path, early):
    m, d, _ = build(64, dev, tmp_path)
    ps, noise, thres, _, _ = stop_setup(m, dev, d)
    kw = dict(end_disp_kl_thres=thres if early else -1.0, max_length=STOP_FRAMES, device_head=True, noise=noise.view(STOP_FRAMES, 1, d))
    a, b = m.infer_batch(ps, stop_lag=0, **kw), m.infer_batch(ps, stop_lag=1, **kw)
    if early:
        assert min(o.shape[2] for o in a) < STOP_FRAMES - 1
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for ids, lat in ps[:2]:
        assert torch.equal(m.infer(ids, lat, stop_lag=0, **kw), m.infer(ids, lat, stop_lag=1, **kw))


@pytest.mark.parametrize("hd", [64, 128])
def test_final_norm_false_is_the_stream_before_the_norm(dev, tmp_path, hd):
    m, d, D = build(hd, dev, tmp_path)
    model = m.base_model.model
    torch.manual_seed(5)
    x, step = torch.randn(1, 6, D, device=dev), torch.randn(2, 1, D, device=dev)
    with torch.no_grad():
        a, b = model.init_cache(16, dev), model.init_cache(16, dev)
        assert torch.equal(model.norm(model.forward_cached(x, a, final_norm=False)), model.forward_cached(x, b))
        assert torch.equal(model.norm(model.forward_cached(step[:1], a, final_norm=False)), model.forward_cached(step[:1], b))
        a, b = model.init_cache_batch(2, 16, dev), model.init_cache_batch(2, 16, dev)
        for r in range(2):
            assert torch.equal(model.norm(model.prefill_row(x, a, r, final_norm=False)), model.prefill_row(x, b, r))
        assert torch.equal(model.norm(model.forward_cached_batch(step, a, final_norm=False)), model.forward_cached_batch(step, b))


def test_a_changed_head_weight_is_picked_up_at_the_next_call(dev, tmp_path):
    m, d, _ = build(64, dev, tmp_path)
    ps = prompts(dev, d)
    noise = torch.randn(FRAMES, 1, d, device=dev)
    kw = dict(end_disp_kl_thres=-1.0, max_length=FRAMES, device_head=True, noise=noise)
    before = m.infer_batch(ps, **kw)
    assert torch.equal(before[0], m.infer_batch(ps, **kw)[0])
    with torch.no_grad():
        m.distribution_linear[2].weight.mul_(3.0)
    fixed_noise(m, noise.view(FRAMES, 1, 1, d))
    host = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=FRAMES)
    del m.sample
    after = m.infer_batch(ps, **kw)
    assert rel(before[0], host[0]) > 2e-2, "the change is too small to tell a stale copy from a fresh one"
    assert rel(after[0], host[0]) < 2e-2, rel(after[0], host[0])


def test_refusals_name_the_host_path(dev, tmp_path):
    m, d, _ = build(64, dev, tmp_path)
    ids, lat = prompts(dev, d)[0]
    with pytest.raises(NotImplementedError, match="device_head=False"):
        m.infer(ids, lat, max_length=4, use_cache=False, device_head=True)
    m.std = torch.tensor([0.5, 0.5])
    with pytest.raises(NotImplementedError, match="device_head=False"):
        m.infer(ids, lat, max_length=4, device_head=True)
    m.init_sigmaVAE()
    from kalle_audio_amd.model_sigmaVAE import Linear
    odd = Linear(12, 12).to(dev)
    keep = m.distribution_linear[2]
    m.distribution_linear[2] = odd
    try:
        with pytest.raises(NotImplementedError, match="device_head=False"):
            m.infer(ids, lat, max_length=4, device_head=True)
    finally:
        m.distribution_linear[2] = keep
    with pytest.raises(ValueError):
        m.infer(ids, lat, max_length=4, stop_lag=1)
