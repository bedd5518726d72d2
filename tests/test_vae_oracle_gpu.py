"""-m gpu: the VAE conv stacks on the device, per slice, against the fp64 oracle (tests/vae_oracle.py; the yardstick, M, the seeded
defects and the chunk loop are checked on the reference alone in tests/test_vae_oracle_cpu.py).

Every output, input gradient and parameter gradient of the Oobleck autoencoder - the fused inference path under the three settings
of KALLE_CONV_CFIRST, the autograd units of conv_train.py, four partly frozen sets, the chunked encode / decode on both of its
paths - and the mel-VAE's three entry points: |g - f64|_slice <= M r scale on every slice of every tensor, r and M from the CPU.
A slice above M r is a finding (a wrong path, or a rounding point the emulation lacks); no tolerance is set per case.  Each test
prints its largest rho = |g - f64|_slice / (r scale); DESIGN.md "VAE per slice" records them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_oracle as vo  # noqa: E402

pytestmark = pytest.mark.gpu
gu, ko = vo.gu, vo.ko
F32, BF16 = torch.float32, torch.bfloat16
CFIRST = [None, "1", "0"]
TILE_FAMILIES, LANE_FAMILIES = {2, 4}, {5, 6, 7}       # include/kalle_hip.h: the low four bits of kalle_conv_last_plan
_INFERENCE = {}                                         # (case, setting) -> (rho, families per direction)


@pytest.fixture(scope="module", autouse=True)
def _drop_in_installed():
    import kalle_audio_amd
    kalle_audio_amd.install()


def build(c, dev, st=None):
    """the drop-in autoencoder of a case with the case's state (a decoder alone: no encoder, encode passes through)"""
    from stable_audio_tools.models import autoencoders as A
    kw = dict(channels=c["ch"], c_mults=c["c_mults"], strides=c["strides"], use_snake=c["snake"], antialias_activation=c["antialias"])
    enc = A.OobleckEncoder(in_channels=c["audio"], latent_dim=2 * c["lat"], **kw) if c["encoder"] else None
    dec = A.OobleckDecoder(out_channels=c["audio"], latent_dim=c["lat"], use_nearest_upsample=c["nearest"], final_tanh=True, **kw)
    ae = A.AudioAutoencoder(enc, dec, latent_dim=c["lat"], downsampling_ratio=c["ratio"], sample_rate=16000, io_channels=c["audio"])
    st = vo.state(c) if st is None else st
    with torch.no_grad():
        for n, p in ae.named_parameters():
            p.copy_(torch.from_numpy(st[n.replace(".act.", ".")]))        # (Activation1d keeps its SnakeBeta as .act)
    assert len(list(ae.named_parameters())) == len(st)
    return ae.to(dev)


def names_of(ae):
    return {n.replace(".act.", "."): p for n, p in ae.named_parameters()}


def cpu(t):
    return t.detach().float().cpu()


def report(what, rho):
    w = max(rho, key=rho.get)
    print(f"{what}: largest rho {rho[w]:.2f} ({w})")
    assert not vo.failures(rho), (what, vo.failures(rho))


_ORIG = {}


class _Families:
    """records the plan family of every conv launch (kalle_conv_last_plan right after it) into .seen, which the caller swaps"""

    def __init__(self, monkeypatch):
        from kalle_audio_amd import _lib, conv_ops
        self.seen, lib = set(), _lib.load()
        for name in ("conv1d", "conv_transpose1d"):
            orig = _ORIG.setdefault(name, getattr(conv_ops, name))

            def wrapped(*a, _orig=orig, **kw):
                y = _orig(*a, **kw)
                self.seen.add(lib.kalle_conv_last_plan() & 0xF)
                return y

            monkeypatch.setattr(conv_ops, name, wrapped)


def _inference(dev, monkeypatch, cid, setting):
    if (cid, setting) in _INFERENCE:
        return _INFERENCE[cid, setting]
    c = vo.CASES[cid]
    if setting is None:
        monkeypatch.delenv("KALLE_CONV_CFIRST", raising=False)
    else:
        monkeypatch.setenv("KALLE_CONV_CFIRST", setting)
    ae = build(c, dev).eval().requires_grad_(False)
    dt = BF16 if c["bf16"] else F32
    got, fam = {}, {}
    zl = vo.latents_in(cid)                                  # (the reference runs its own autograd: outside no_grad)
    with torch.no_grad():
        rec_ = _Families(monkeypatch)
        if c["encoder"]:
            z = ae.encode(vo.inputs(c)["wav"].to(dev, dt))
            assert z.dtype == dt and not z.requires_grad
            got["inf:z"], fam["encode"] = cpu(z), frozenset(rec_.seen)
        rec_.seen = set()
        rec = ae.decode(zl.to(dev, dt))
        assert rec.dtype == dt
        got["inf:rec"], fam["decode"] = cpu(rec), frozenset(rec_.seen)
    ref = {n: v for n, v in vo.select(vo.reference(cid)).items() if n.startswith("inf:")}
    r, _ = vo.yardstick(cid)
    assert sorted(got) == sorted(ref)
    _INFERENCE[cid, setting] = (vo.rho_of(got, ref, r), fam)
    return _INFERENCE[cid, setting]


@pytest.mark.parametrize("setting", CFIRST, ids=lambda s: f"cfirst-{s}")
@pytest.mark.parametrize("cid", list(vo.CASES))
def test_inference_path(dev, monkeypatch, cid, setting):
    """frozen, under no_grad: ae.encode(wav) and ae.decode of the reference's mean latents, every 16-position run of every (b, c)"""
    rho, fam = _inference(dev, monkeypatch, cid, setting)
    print(cid, setting, "families", {k: sorted(v) for k, v in fam.items()})
    report(f"{cid} cfirst={setting}", rho)
    if setting == "0":
        assert not (set().union(*fam.values()) & LANE_FAMILIES), fam


def test_plan_families_reached_over_the_table(dev, monkeypatch):
    """over the whole table both the tile kernels and the channels-per-lane kernels (families 5 - 7) ran; which case reaches which
    family is recorded here (and in DESIGN.md), not assumed"""
    seen = {}
    for cid in vo.CASES:
        for setting in CFIRST:
            _, fam = _inference(dev, monkeypatch, cid, setting)
            seen[cid, setting] = set().union(*fam.values())
            print(cid, f"cfirst={setting}", {k: sorted(v) for k, v in fam.items()})
    every = set().union(*seen.values())
    assert every & TILE_FAMILIES == TILE_FAMILIES and every & LANE_FAMILIES, every


def _train(ae, c, dev, wav_grad=True):
    """the loss of the older test on the device: {name: tensor} of z, rec, the input gradient and every parameter gradient"""
    inp = vo.inputs(c)
    if c["encoder"]:
        wav = inp["wav"].to(dev).requires_grad_(wav_grad)
        z = ae.encode(wav)
        rec = ae.decode(z[:, :c["lat"]] + 0.3 * z[:, c["lat"]:])
        loss = (z * vo.cotangent(c, "dz", z.shape).to(dev)).sum() + (rec * vo.cotangent(c, "drec", rec.shape).to(dev)).sum()
        loss.backward()
        got = {"act:z": z, "act:rec": rec}
        if wav_grad:
            got["act:dwav"] = wav.grad
    else:
        z = inp["z"].to(dev).requires_grad_(True)
        rec = ae.decode(z)
        (rec * vo.cotangent(c, "drec", rec.shape).to(dev)).sum().backward()
        got = {"act:rec": rec, "act:dz": z.grad}
    got.update({n: p.grad for n, p in names_of(ae).items() if p.grad is not None})
    return {n: cpu(v) for n, v in got.items()}, z


_TRAINED = {}


def _trained(dev, cid):
    """what the device gives for a case with everything trainable, computed once"""
    if cid not in _TRAINED:
        c = vo.CASES[cid]
        ae = build(c, dev)
        ae.requires_grad_(True)
        got, _ = _train(ae, c, dev)
        assert all(p.grad is not None for p in ae.parameters())
        _TRAINED[cid] = vo.select(got)
    return _TRAINED[cid]


def _training_reference(cid, defect=None):
    return {n: v for n, v in vo.select(vo.reference(cid, "f64", 0, defect)).items() if not n.startswith("inf:")}


@pytest.mark.parametrize("cid", vo.TRAIN_CASES)
def test_training_path(dev, cid):
    """all trainable, the input requires a gradient: z, rec, dwav and the gradient of every weight_v, weight_g, bias, alpha, beta"""
    got, ref = _trained(dev, cid), _training_reference(cid)
    r, _ = vo.yardstick(cid)
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    report(f"{cid} training", vo.rho_of(got, ref, r))


@pytest.mark.parametrize("cid", vo.TRAIN_CASES)
def test_device_fails_every_defective_reference(dev, cid):
    """the check bites on the device too: against the reference with ONE seeded defect (every defect the case has the structure
    for and that is not listed blind) the device's tensors fail, as they must if the device is right and the reference is not"""
    got = _trained(dev, cid)
    r, _ = vo.yardstick(cid)
    weakest = None
    for d in vo.DEFECTS:
        if not vo.applies(d, vo.CASES[cid]) or (cid, d) in vo.BLIND:
            continue
        rho = vo.rho_of(got, _training_reference(cid, d), r)
        assert vo.failures(rho), (cid, d, max(rho.values()))
        if weakest is None or max(rho.values()) < weakest[1]:
            weakest = (d, max(rho.values()))
    print(f"{cid}: weakest defect on the device {weakest[0]} at rho {weakest[1]:.1f}")


@pytest.mark.parametrize("frozen", list(vo.FROZEN_SETS))
@pytest.mark.parametrize("cid", vo.FROZEN_CASES)
def test_partly_frozen(dev, cid, frozen):
    """a frozen parameter keeps grad None and its bits; the trainable slices pass; with the encoder frozen and an input without
    gradient the encoder stays on the fused inference path under grad mode (its output has no grad_fn) while the decoder runs as
    autograd units"""
    c = vo.CASES[cid]
    ae = build(c, dev)
    is_frozen = vo.FROZEN_SETS[frozen]
    params = names_of(ae)
    for n, p in params.items():
        p.requires_grad_(not is_frozen(n))
    before = {n: p.detach().clone() for n, p in params.items()}
    got, z = _train(ae, c, dev, wav_grad=frozen != "encoder")
    assert (z.grad_fn is None and not z.requires_grad) == (frozen == "encoder")
    for n, p in params.items():
        assert (p.grad is None) == is_frozen(n), n
        assert torch.equal(p.detach(), before[n]), n
    ref = {n: v for n, v in vo.select(vo.reference(cid), frozen).items() if not n.startswith("inf:")}
    r, _ = vo.yardstick(cid, frozen)
    got = vo.select(got, frozen)
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    assert any(not vo.is_act(n) for n in ref)
    report(f"{cid} frozen {frozen}", vo.rho_of(got, ref, r))


@pytest.mark.parametrize("path", ["segment_copy", "slicing"])
@pytest.mark.parametrize("i", range(len(vo.CHUNKED)), ids=lambda i: "-".join(map(str, vo.CHUNKED[i])))
def test_chunked(dev, i, path):
    """decode_audio / encode_audio(chunked=True) at 100 latents - an anchored last chunk in each, several passes of _run_chunked -
    against the reference project's chunk loop restated over the fp64 oracle, cut at every seam of that loop: the batched
    segment_copy path, and the differentiable torch-slicing path with the gradient of its input"""
    direction, size, overlap = vo.CHUNKED[i]
    c = vo.CASES[vo.CHUNK_CASE]
    ae = build(c, dev)
    ae.chunk_batch = 2 * c["B"]
    ref, seams = vo.chunk_reference(i)
    r, _ = vo.chunk_yardstick(i)
    plan_len = len(ae._chunk_plan(100, size, size - overlap, lambda s: s * c["ratio"], size * c["ratio"], 100 * c["ratio"], 0))
    assert plan_len > ae.chunk_batch // c["B"]                   # more chunks than one pass takes
    x = vo.chunk_inputs(c, direction).to(dev)
    fn = ae.decode_audio if direction == "decode" else ae.encode_audio
    if path == "segment_copy":
        ae.requires_grad_(False)
        with torch.no_grad():
            y = fn(x, chunked=True, chunk_size=size, overlap=overlap)
        assert not y.requires_grad
        got = {"chunk:y": cpu(y)}
    else:
        ae.requires_grad_(True)
        x.requires_grad_(True)
        y = fn(x, chunked=True, chunk_size=size, overlap=overlap)
        assert y.grad_fn is not None
        (y * vo.cotangent(c, "dy_" + direction, y.shape).to(dev)).sum().backward()
        got = {"chunk:y": cpu(y), "chunk:dx": cpu(x.grad)}
    report(f"chunked {direction} ({size}, {overlap}) {path}", vo.rho_of(got, ref, r, seams))


@pytest.mark.parametrize("cid", list(vo.MELVAE_CASES))
def test_melvae(dev, cid):
    """flows.py, forward only: extract_latents, forward(wav, eps) -> (rec, z_p, logs_q), inference_from_latents"""
    c = vo.MELVAE_CASES[cid]
    vae = vo.melvae_module(cid)
    st = vo.melvae_state(cid)
    with torch.no_grad():
        for n, p in vae.named_parameters():
            p.copy_(torch.from_numpy(st[n]))
    vae = vae.to(dev).eval()
    inp = {k: v.to(dev) for k, v in vo.melvae_inputs(cid).items()}
    with torch.no_grad():
        got = {"mel:latents": vae.extract_latents(inp["wav"])}
        rec, (z_p, logs_q, _, _) = vae(inp["wav"], noise=inp["eps"])
        got.update({"mel:rec": rec, "mel:z_p": z_p, "mel:logs_q": logs_q,
                    "mel:dec": vae.inference_from_latents(inp["z"], do_sample=False)})
    ref = vo.melvae_reference(cid)
    r, _ = vo.melvae_yardstick(cid)
    report(f"mel-VAE {cid}", vo.rho_of({n: cpu(v) for n, v in got.items()}, ref, r))
    assert c["h"]["latent_dim"] * 2 == got["mel:latents"].shape[1]
