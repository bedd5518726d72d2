"""-m gpu: ragged batches through the Oobleck stacks on the device - AudioAutoencoder.decode(z, lengths) / encode(wav, lengths),
decode_list / encode_list - held row by row to the fp64 oracle run of that row ALONE (tests/vae_ragged.py: the per-slice method, M,
r and the emulation of tests/vae_oracle.py; the yardstick, the definition and the defects' sensitivity are checked on the
reference alone in tests/test_conv_lens_cpu.py).

Under every setting of KALLE_CONV_CFIRST, plan families recorded: every row inside M r of its own reference and exactly zero past
its length; the list forms equal the lengths= call of their groups bit for bit and keep the input order under a cap that forces
three groups; the device's tensors FAIL each seeded defect of the reference (zero padding instead of lengths first of all);
lengths=None and all-full lengths equal the dense call bit for bit; Llasa.infer_batch's list decodes to one waveform per prompt."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_oracle as vo  # noqa: E402
import vae_ragged as vr  # noqa: E402
from test_vae_oracle_gpu import CFIRST, LANE_FAMILIES, _Families, build, cpu  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
_GOT = {}                                               # (case, direction, setting) -> (rows on the CPU, the padded result, families)


@pytest.fixture(scope="module", autouse=True)
def _drop_in_installed():
    import kalle_audio_amd
    kalle_audio_amd.install()


def _setting(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("KALLE_CONV_CFIRST", raising=False)
    else:
        monkeypatch.setenv("KALLE_CONV_CFIRST", setting)


def _run(dev, monkeypatch, cid, direction, setting):
    key = (cid, direction, setting)
    if key in _GOT:
        return _GOT[key]
    c = vo.CASES[cid]
    _setting(monkeypatch, setting)
    ae = build(c, dev).eval().requires_grad_(False)
    dt = BF16 if c["bf16"] else F32
    x, L = vr.padded(cid, direction)
    # what lies past a row's length is the caller's business: NaN here, so that anything read from there shows
    pos = torch.arange(x.shape[2])[None, None, :]
    x = torch.where(pos < torch.tensor(L)[:, None, None], x, torch.full_like(x, float("nan")))
    with torch.no_grad():
        rec = _Families(monkeypatch)
        y = (ae.decode if direction == "decode" else ae.encode)(x.to(dev, dt), lengths=L)
        fam = frozenset(rec.seen)
    assert y.dtype == dt and y.shape[0] == len(L)
    y = cpu(y)
    out_len = [r.shape[2] for r in vr.alone(cid, direction)]
    assert y.shape[2] == max(out_len)
    _GOT[key] = ([y[b:b + 1, :, :n] for b, n in enumerate(out_len)], y, fam)
    return _GOT[key]


DIRECTED = [(cid, d) for cid in vr.CIDS for d in ("decode", "encode") if d == "decode" or cid in vr.ENC_CIDS]


@pytest.mark.parametrize("setting", CFIRST, ids=lambda s: f"cfirst-{s}")
@pytest.mark.parametrize("cid,direction", DIRECTED)
def test_rows_against_the_rows_alone(dev, monkeypatch, cid, direction, setting):
    rows, y, fam = _run(dev, monkeypatch, cid, direction, setting)
    rho = vr.rho(rows, cid, direction)
    w = max(rho, key=rho.get)
    print(f"{cid} {direction} cfirst={setting}: families {sorted(fam)}, largest rho {rho[w]:.2f} ({w}), all " + " ".join(f"{v:.2f}" for v in rho.values()))
    assert not vo.failures(rho), (cid, direction, setting, vo.failures(rho))
    for b, r in enumerate(rows):                        # exact zeros past each row's length, and nothing non-finite anywhere
        assert (y[b, :, r.shape[2]:] == 0).all(), (cid, direction, b)
    assert torch.isfinite(y).all()
    if setting == "0":
        assert not (fam & LANE_FAMILIES), fam
    if setting == "1" and not vo.CASES[cid]["bf16"]:    # (the channels-per-lane kernels are fp32 only)
        assert fam & LANE_FAMILIES, fam


@pytest.mark.parametrize("cid,direction", DIRECTED)
def test_device_fails_the_seeded_defects(dev, monkeypatch, cid, direction):
    """the same comparison against a reference with one defect: zero padding instead of lengths, the neighbouring row's lengths,
    the input-rate length kept after the first resampling block, one k = 1 residual conv unmasked"""
    rows, _, _ = _run(dev, monkeypatch, cid, direction, None)
    for defect in vr.DEFECTS:
        if (direction, cid, defect) in vr.BLIND:
            continue
        rho = vr.rho(rows, cid, direction, ref_rows=vr.masked(cid, direction, defect))
        print(f"{cid} {direction} vs {defect}: " + " ".join(f"{v:.3g}" for v in rho.values()))
        assert vo.failures(rho), (cid, direction, defect, "the device's rows pass a defective reference", rho)


@pytest.mark.parametrize("cid", ["O1", "O2", "O5", "O7"])
def test_list_forms(dev, monkeypatch, cid):
    """decode_list / encode_list: the rows of the lengths= call of each group, bit for bit, in input order, under a cap that
    forces three groups; through the pretransform too"""
    from stable_audio_tools.models.pretransforms import AutoencoderPretransform
    c = vo.CASES[cid]
    _setting(monkeypatch, None)
    ae = build(c, dev).eval().requires_grad_(False)
    dt = BF16 if c["bf16"] else F32
    for direction in ["decode"] + (["encode"] if c["encoder"] else []):
        items = [t.to(dev, dt) for t in vr.rows(cid, direction)]
        order = [3, 0, 4, 1, 2][:len(items)] if direction == "decode" else [2, 0, 3, 1]
        shuffled = [items[i] for i in order]
        sizes = [t.shape[2] for t in shuffled]
        per = (lambda n: n * c["ratio"]) if direction == "decode" else (lambda n: n)
        top = sorted(sizes)
        cap = 2 * per(top[-2]) if direction == "encode" else 3 * per(top[2])     # [the short ones] [next] [longest]
        fn, one = (ae.decode_list, ae.decode) if direction == "decode" else (ae.encode_list, ae.encode)
        groups = ae._ragged_groups(sizes, per, cap)
        assert len(groups) == 3, (groups, sizes, cap)
        with torch.no_grad():
            outs = fn(shuffled, max_batch_samples=cap)
            assert len(outs) == len(shuffled)
            for g in groups:
                x, L = ae._stack([shuffled[i] for i in g], shuffled[0].shape[1])
                y = one(x, lengths=L)
                for b, i in enumerate(g):
                    n = outs[i].shape[2]
                    assert outs[i].shape[:2] == (1, y.shape[1]) and torch.equal(outs[i][0], y[b, :, :n]), (direction, i)
                    assert (y[b, :, n:] == 0).all()
            # input order: item i of the result is the row of item i, whatever group it ran in
            alone = vr.alone(cid, direction)
            for j, i in enumerate(order):
                assert outs[j].shape == alone[i].shape, (direction, j, outs[j].shape, alone[i].shape)
            rho = vr.rho([cpu(outs[order.index(i)]) for i in range(len(items))], cid, direction)
            assert not vo.failures(rho), (direction, vo.failures(rho))
            # the default cap takes them all in one group; the pretransform hands the list through (scale applied)
            assert len(ae._ragged_groups(sizes, per, ae._default_cap())) == 1
            pt = AutoencoderPretransform(ae, scale=2.0, model_half=c["bf16"])
            if direction == "decode":
                ys = pt.decode_list([t.float() / 2.0 for t in shuffled])
                for a, b in zip(ys, fn(shuffled)):
                    assert torch.equal(a, b.float())


@pytest.mark.parametrize("cid", ["O1", "O5", "O7"])
def test_no_lengths_and_full_lengths_are_the_dense_call(dev, monkeypatch, cid):
    c = vo.CASES[cid]
    _setting(monkeypatch, None)
    ae = build(c, dev).eval().requires_grad_(False)
    dt = BF16 if c["bf16"] else F32
    z = vo.latents_in(cid).to(dev, dt)                   # (the reference runs its own autograd: outside no_grad)
    with torch.no_grad():
        dense = ae.decode(z)
        assert torch.equal(ae.decode(z, lengths=None), dense)
        assert torch.equal(ae.decode(z, lengths=[z.shape[2]] * z.shape[0]), dense)
        if c["encoder"]:
            wav = vo.inputs(c)["wav"].to(dev, dt)
            dense = ae.encode(wav)
            assert torch.equal(ae.encode(wav, lengths=None), dense)
            assert torch.equal(ae.encode(wav, lengths=[wav.shape[2]] * wav.shape[0]), dense)


def test_decode_list_takes_what_infer_batch_returns(dev, tmp_path):
    """text -> latents -> waveform, batched end to end: the list Llasa.infer_batch returns (rows of different length) goes into
    decode_list as it is; one waveform per prompt, T_i x ratio samples, each the row decoded alone (to fp32 rounding)"""
    from stable_audio_tools.models import autoencoders as A
    from test_llasa_batch_gpu import build as build_llasa, prompts
    m, d, _ = build_llasa(64, dev, tmp_path)
    ps = prompts(dev, d)
    lat = m.infer_batch(ps[:2], end_disp_kl_thres=-1.0, max_length=8) + m.infer_batch(ps[2:], end_disp_kl_thres=-1.0, max_length=4)
    T = [t.shape[2] for t in lat]
    assert len(lat) == 3 and len(set(T)) == 2 and all(t.shape[:2] == (1, d) for t in lat)
    torch.manual_seed(5)
    dec = A.OobleckDecoder(out_channels=1, channels=8, latent_dim=d, c_mults=[1, 2], strides=[2, 4], use_snake=True)
    ae = A.AudioAutoencoder(None, dec, latent_dim=d, downsampling_ratio=8, sample_rate=16000, io_channels=1).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        wavs = ae.decode_list(lat)
        assert len(wavs) == 3
        for z, w in zip(lat, wavs):
            assert w.shape == (1, 1, z.shape[2] * 8)
            one = ae.decode(z.contiguous())             # (another batch size: another tile form, another order of summation)
            tol = 1e-4 if z.dtype == torch.float32 else 3e-2
            assert torch.isfinite(w).all() and (w.float() - one.float()).abs().max() <= tol * max(1.0, one.abs().max().item())
