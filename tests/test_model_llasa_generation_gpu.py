"""-m gpu: model.Llasa (mean || log-scale head) generation - infer / infer_batch with the head on the host and with
device_head=True (one decode-step call plus one kalle_llasa_frame_head2_rows call per frame) - on the tiny head-dim 64 and 128
Llama configs of the existing Llasa tests, with bf16 and e4m3 decode steps: device head against host head, infer_batch against
sequential infer, a seeded run, the stop rule, stop_lag=1 against stop_lag=0 bit for bit, and the plumbing (host modules not
reached, a changed head weight, the refusals, more than one group), by the method of tests/test_llasa_device_head_gpu.py.

The host path draws its noise with torch.randn_like(mean) for mean [R, 1, lat]; `host_noise` substitutes frame i's draw by
noise[i] (rows of a batch: noise[i, r]) the way fixed_noise substitutes Llasa.sample for the fixed-std class."""
import contextlib
import json
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import golden_util as gu  # noqa: E402
import llama_hd128_cases as lc128  # noqa: E402
from test_llasa_batch_gpu import prompts, rel  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = 8
# the stop tests: the MEAN rows of distribution_linear[2].weight times STOP_SCALE spread the predicted means, and with them the
# per-frame KLs of the three rows, as tests/test_llasa_device_head_gpu.py spreads them.  The log-scale rows keep their size: 100 x
# would put logs at +-30 and exp(logs) at 1e13, a head no checkpoint has and whose latents overflow the next step's bf16 input.
STOP_FRAMES, STOP_SEED, STOP_SCALE = 10, 0, 100.0


class _Tok:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def build(hd, dev, tmp_path):
    """(model.Llasa, latent_dim, hidden size): the tiny configs of test_modules_gpu / test_llama_hd128_gpu with this class's head"""
    from kalle_audio_amd.model import Llasa
    lc, D, seed = (gu.LLASA_CONFIG, 128, 54) if hd == 64 else (lc128.llasa_config(), 256, lc128.SEED)
    d = tmp_path / f"llama_m{hd}"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": lc["latent_dim"], "audio_proj_dim": D}, _Tok(lc["tokenizer_len"]),
              use_flash_attention=False)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k != "base_model.lm_head.weight"]
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(shapes, seed).items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to(dev), lc["latent_dim"], D


@contextlib.contextmanager
def host_noise(noise, row=None):
    """torch.randn_like(mean) returns noise[i] at the i-th call (row: that row of it alone), noise [frames, R, lat]"""
    real, it = torch.randn_like, iter(noise)

    def fed(t, **kw):
        n = next(it)
        n = n if row is None else n[row:row + 1]
        assert n.numel() == t.numel(), (n.shape, t.shape)
        return n.reshape(t.shape).to(t.dtype)

    torch.randn_like = fed
    try:
        yield
    finally:
        torch.randn_like = real


@contextlib.contextmanager
def no_host_head(m):
    """distribution_linear / audio_linear forward and the host frame raise: the device path must not reach them after the prompt"""
    def boom(*a, **k):
        raise AssertionError("the host head ran under device_head=True")
    hooks = [m.distribution_linear.register_forward_pre_hook(boom)]
    m._host_frame = boom
    try:
        yield
    finally:
        hooks[0].remove()
        del m._host_frame


def draw(dev, frames, R, lat, seed=3):
    return torch.randn(frames, R, lat, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


@pytest.mark.parametrize("fmt", [None, "e4m3"], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("hd", [64, 128])
def test_device_head_matches_the_host_head(dev, tmp_path, hd, fmt):
    """infer_batch (three ragged prompts, the R-row step) and infer (the one-row step): same shapes and strides, rel < 2e-2 - the
    bound tests/test_llasa_device_head_gpu.py holds "same arithmetic, other summation order, 8 frames" to"""
    m, lat, _ = build(hd, dev, tmp_path)
    if fmt:
        m.quantize_decoder(fmt)
    ps = prompts(dev, lat)
    noise = draw(dev, FRAMES, 3, lat)
    kw = dict(end_disp_kl_thres=-1.0, max_length=FRAMES)
    with host_noise(noise):
        host = m.infer_batch(ps, **kw)
    with no_host_head(m):
        devo = m.infer_batch(ps, device_head=True, noise=noise, **kw)
    assert len(devo) == len(host) == 3
    for r in range(3):
        assert devo[r].shape == host[r].shape == (1, 2 * lat, FRAMES - 1) and devo[r].stride() == host[r].stride()
        print("prompt", r, "infer_batch device head vs host head", rel(devo[r], host[r]))
        assert rel(devo[r], host[r]) < 2e-2, (r, rel(devo[r], host[r]))
    ids, pl = ps[0]
    with host_noise(noise, row=0):
        one = m.infer(ids, pl, **kw)
    with no_host_head(m):
        got = m.infer(ids, pl, device_head=True, noise=noise[:, :1], **kw)
    assert got.shape == one.shape == (1, 2 * lat, FRAMES - 1) and got.stride() == one.stride()
    print("infer device head vs host head", rel(got, one))
    assert rel(got, one) < 2e-2, rel(got, one)


@pytest.mark.parametrize("hd", [64, 128])
def test_host_infer_batch_matches_sequential_infer(dev, tmp_path, hd):
    m, lat, _ = build(hd, dev, tmp_path)
    ps = prompts(dev, lat)
    noise = draw(dev, FRAMES, 3, lat, seed=4)
    kw = dict(end_disp_kl_thres=-1.0, max_length=FRAMES)
    with host_noise(noise):
        batch = m.infer_batch(ps, **kw)
    for r, (ids, pl) in enumerate(ps):
        with host_noise(noise, row=r):
            one = m.infer(ids, pl, **kw)
        assert batch[r].shape == one.shape and batch[r].stride() == one.stride()
        print("prompt", r, "host infer_batch vs infer", rel(batch[r], one))
        assert rel(batch[r], one) < 2e-2, (r, rel(batch[r], one))
    assert m.infer_batch([]) == []
    with host_noise(noise, row=1):
        a = m.infer_batch(ps[1:2], **kw)[0]                    # one prompt falls through to infer
    with host_noise(noise, row=1):
        assert torch.equal(a, m.infer(ps[1][0], ps[1][1], **kw))


@pytest.mark.parametrize("hd", [64, 128])
def test_seeded_run_draws_as_the_host_path_does(dev, tmp_path, hd):
    """noise=None: one torch.randn((R, 1, lat)) per frame, the shape and order of the host path's randn_like(mean), so the same seed
    gives the host path's noise - and leaves the generator where the host path leaves it"""
    m, lat, _ = build(hd, dev, tmp_path)
    ps = prompts(dev, lat)
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


def kl_of(disp):
    """the stop KL of model.py:133-136 from mean || log-scale [..., 2 lat], float64"""
    lat = disp.shape[-1] // 2
    mean, logs = disp[..., :lat].double(), disp[..., lat:].double()
    return ((1.0 - logs) + (torch.exp(2 * logs) + (mean - 1.0) ** 2) / (2 * math.e ** 2) - 0.5).mean(-1)


def free_run_kls(m, ps, noise):
    """per-frame, per-row KL of a free run (threshold -1) on the host path and on the device path: [frames, R] each"""
    from kalle_audio_amd import ops
    host = []
    h = m.distribution_linear.register_forward_hook(lambda mod, inp, out: host.append(kl_of(out.view(len(ps), -1))))
    try:
        with host_noise(noise):
            m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=STOP_FRAMES)
    finally:
        h.remove()
    devk, head = [], ops.llasa_frame_head2

    def spy(*a, **k):
        out = head(*a, **k)
        devk.append(out[2].double().clone())
        return out

    ops.llasa_frame_head2 = spy
    try:
        m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=STOP_FRAMES, device_head=True, noise=noise)
    finally:
        ops.llasa_frame_head2 = head
    return torch.stack(host).cpu(), torch.stack(devk).cpu()


def pick_threshold(kls):
    """(threshold, gap): the middle of the widest gap between two neighbouring free-run KLs [frames, R] at i >= 4 among those gaps
    whose threshold stops the rows at different frames (a row no KL of which lies below it runs to the end)"""
    v = kls[4:].reshape(-1).sort().values
    best = None
    for i in range(len(v) - 1):
        t, gap = float((v[i] + v[i + 1]) / 2), float(v[i + 1] - v[i])
        stops = [next((f for f in range(4, kls.shape[0]) if kls[f, r] < t), kls.shape[0]) for r in range(kls.shape[1])]
        if min(stops) < max(stops) and (best is None or gap > best[1]):
            best = (t, gap)
    assert best is not None, "no threshold stops the rows at different frames"
    return best


def stop_setup(m, dev, lat):
    with torch.no_grad():
        m.distribution_linear[2].weight[:lat].mul_(STOP_SCALE)
    ps = prompts(dev, lat)
    noise = draw(dev, STOP_FRAMES, 3, lat, seed=STOP_SEED)
    host, devk = free_run_kls(m, ps, noise)
    assert host.shape == devk.shape == (STOP_FRAMES, 3)
    thres, gap = pick_threshold(host)
    diff = float((host - devk).abs().max())
    print("free-run KL: widest gap", gap, "at", thres, "largest device-vs-host difference", diff, "ratio", gap / diff)
    return ps, noise, thres, gap, diff


def test_stop_rule_stops_the_rows_the_host_path_stops(dev, tmp_path):
    """the threshold sits in the widest gap of the host path's free-run KLs at i >= 4 that stops the rows at different frames, a gap
    at least 20 x the largest difference between the two paths' KLs, so both paths must stop every row at the same frame"""
    m, lat, _ = build(64, dev, tmp_path)
    ps, noise, thres, gap, diff = stop_setup(m, dev, lat)
    assert gap >= 20 * diff, (gap, diff)
    kw = dict(end_disp_kl_thres=thres, max_length=STOP_FRAMES)
    with host_noise(noise):
        host = m.infer_batch(ps, **kw)
    with no_host_head(m):
        devo = m.infer_batch(ps, device_head=True, noise=noise, **kw)
    lens = [o.shape[2] for o in host]
    print("frames per row", lens)
    assert [o.shape[2] for o in devo] == lens
    assert min(lens) < max(lens), ("no row stops while another goes on", lens)
    for a, b in zip(devo, host):
        assert rel(a, b) < 2e-2, rel(a, b)
    r = lens.index(min(lens))
    one = m.infer(ps[r][0], ps[r][1], device_head=True, noise=noise[:, r:r + 1], **kw)
    assert one.shape[2] == lens[r]


@pytest.mark.parametrize("early", [True, False], ids=["early-stop", "to-max-length"])
def test_stop_lag_one_returns_the_bits_of_stop_lag_zero(dev, tmp_path, early):
    m, lat, _ = build(64, dev, tmp_path)
    ps, noise, thres, _, _ = stop_setup(m, dev, lat)
    kw = dict(end_disp_kl_thres=thres if early else -1.0, max_length=STOP_FRAMES, device_head=True)
    a, b = m.infer_batch(ps, stop_lag=0, noise=noise, **kw), m.infer_batch(ps, stop_lag=1, noise=noise, **kw)
    if early:
        assert min(o.shape[2] for o in a) < STOP_FRAMES - 1
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for r, (ids, pl) in enumerate(ps[:2]):
        nz = noise[:, r:r + 1]
        assert torch.equal(m.infer(ids, pl, stop_lag=0, noise=nz, **kw), m.infer(ids, pl, stop_lag=1, noise=nz, **kw))


def test_a_changed_head_weight_is_picked_up_at_the_next_call(dev, tmp_path):
    m, lat, _ = build(64, dev, tmp_path)
    ps = prompts(dev, lat)
    noise = draw(dev, FRAMES, 3, lat, seed=9)
    kw = dict(end_disp_kl_thres=-1.0, max_length=FRAMES)
    before = m.infer_batch(ps, device_head=True, noise=noise, **kw)
    assert torch.equal(before[0], m.infer_batch(ps, device_head=True, noise=noise, **kw)[0])
    with torch.no_grad():
        m.distribution_linear[2].weight[:lat].mul_(3.0)
    with host_noise(noise):
        host = m.infer_batch(ps, **kw)
    after = m.infer_batch(ps, device_head=True, noise=noise, **kw)
    assert rel(before[0], host[0]) > 2e-2, "the change is too small to tell a stale copy from a fresh one"
    assert rel(after[0], host[0]) < 2e-2, rel(after[0], host[0])


def test_refusals_name_the_host_path(dev, tmp_path):
    from kalle_audio_amd.model_sigmaVAE import Linear
    m, lat, D = build(64, dev, tmp_path)
    ps = prompts(dev, lat)
    ids, pl = ps[0]
    with pytest.raises(NotImplementedError, match="device_head=False"):
        m.infer(ids, pl, max_length=4, use_cache=False, device_head=True)
    for lag in (2, -1):
        with pytest.raises(NotImplementedError, match="device_head=False"):
            m.infer(ids, pl, max_length=4, device_head=True, stop_lag=lag)
        with pytest.raises(NotImplementedError, match="device_head=False"):
            m.infer_batch(ps, max_length=4, device_head=True, stop_lag=lag)
    keep = m.audio_linear, m.distribution_linear[0], m.distribution_linear[2]
    for odd in (12, 264):                                      # no multiple of 8; over the kernel's bound
        m.audio_linear, m.distribution_linear[0], m.distribution_linear[2] = (Linear(odd, D).to(dev), Linear(D, 2 * odd).to(dev),
                                                                              Linear(2 * odd, 2 * odd).to(dev))
        try:
            with pytest.raises(NotImplementedError, match="device_head=False"):
                m.infer(ids, None, max_length=4, device_head=True)
            with pytest.raises(NotImplementedError, match="device_head=False"):
                m.infer_batch([(ids, None), (ids, None)], max_length=4, device_head=True)
        finally:
            m.audio_linear, m.distribution_linear[0], m.distribution_linear[2] = keep
    for kw in (dict(stop_lag=1), dict(noise=torch.zeros(4, 1, lat, device=dev))):
        with pytest.raises(ValueError):
            m.infer(ids, pl, max_length=4, **kw)
        with pytest.raises(ValueError):
            m.infer_batch(ps, max_length=4, **kw)


@pytest.mark.parametrize("device_head", [False, True], ids=["host", "device"])
def test_seventeen_prompts_run_in_two_groups(dev, tmp_path, device_head):
    """17 prompts: a group of 16 and a group of one (which is `infer`); every output that of the prompt generated alone"""
    m, lat, _ = build(64, dev, tmp_path)
    base = prompts(dev, lat)
    ps = [base[i % 3] for i in range(17)]
    noise = draw(dev, 6, 17, lat, seed=12)
    kw = dict(end_disp_kl_thres=-1.0, max_length=6)
    if device_head:
        outs = m.infer_batch(ps, device_head=True, noise=noise, **kw)
    else:
        with host_noise(noise[:, :16]):
            first = m.infer_batch(ps[:16], **kw)
        with host_noise(noise, row=16):
            outs = first + [m.infer(ps[16][0], ps[16][1], **kw)]
        calls = []
        real = torch.randn_like
        torch.randn_like = lambda t, **k: (calls.append(tuple(t.shape)), real(t, **k))[1]
        try:
            assert len(m.infer_batch(ps, **kw)) == 17
        finally:
            torch.randn_like = real
        assert calls == [(16, 1, lat)] * 6 + [(1, 1, lat)] * 6      # the groups: sixteen rows, then `infer` for the last
    assert len(outs) == 17 and all(o.shape == (1, 2 * lat, 5) for o in outs)
    for r in (0, 7, 15, 16):
        if device_head:
            one = m.infer(ps[r][0], ps[r][1], device_head=True, noise=noise[:, r:r + 1], **kw)
        else:
            with host_noise(noise, row=r):
                one = m.infer(ps[r][0], ps[r][1], **kw)
        print("row", r, "of 17 vs alone", rel(outs[r], one))
        assert rel(outs[r], one) < 2e-2, (r, rel(outs[r], one))
