"""No GPU: the ragged-batch contract that can be held without a device.
 - every refusal of the five ..._lens entry points (they refuse before any launch) and of the Python layer;
 - an all-inactive batch: KALLE_OK, nothing launched, the dense call's plan word;
 - the cases of tests/conv_lens_cases.py get the kernel family they are there for;
 - the per-layer length propagation against the lengths torch's conv1d / conv_transpose1d give each row alone;
 - the definition: in fp64, the stack masked layer by layer equals each row run alone, to rounding (tests/vae_ragged.py);
 - the sensitivity the device test relies on: the zero-padded stack, and each other seeded defect, lies 2 M r or more from the
   rows run alone - on the reference alone - except the triples listed blind, which lie under it."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_lens_cases as lc  # noqa: E402
import vae_oracle as vo  # noqa: E402
import vae_ragged as vr  # noqa: E402

ERR_ARG = -1
F32 = 1
DUMMY = ctypes.c_void_p(4096)       # a "device pointer" no refused call may touch


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def arr(*v):
    return (ctypes.c_int32 * len(v))(*v)


# ================================================================================================ the C ABI's refusals
# B = 3, a conv of K = 4, stride 2, padding 1 over Lin = 20 (Lout 10), and its transposed twin 10 -> 20
def conv_call(lib, hi, di, ho, do):
    return lib.kalle_conv1d_fwd_lens(DUMMY, F32, DUMMY, None, DUMMY, F32, 3, 8, 20, 8, 10, 4, 2, 1, 1, None, None, hi, di, ho, do, None)


def convT_call(lib, hi, di, ho, do):
    return lib.kalle_conv_transpose1d_fwd_lens(DUMMY, F32, DUMMY, None, DUMMY, F32, 3, 8, 10, 8, 20, 4, 2, 1, None, None, hi, di, ho, do, None)


def cfirst_call(lib, hi, di, ho, do):
    Lp = lib.kalle_conv_pad_len(10, 4, 2, 1, 1)
    return lib.kalle_conv1d_cfirst_fwd_lens(DUMMY, DUMMY, None, DUMMY, 3, 8, Lp, 8, 10, 4, 2, 1, 1, None, None, hi, di, ho, do, None)


def cfirstT_call(lib, ho, do):
    Lp = lib.kalle_convT_pad_len(20, 4, 2, 1)
    return lib.kalle_conv_transpose1d_cfirst_fwd_lens(DUMMY, DUMMY, None, DUMMY, 3, 8, Lp, 8, 20, 4, 2, 1, None, ho, do, None)


def pad_call(lib, hi, di):
    return lib.kalle_conv_pad_act_lens(DUMMY, DUMMY, 3, 8, 20, 32, 2, None, 2, hi, di, None)


PAIRS = {   # entry -> (call, a valid all-inactive (lens_in, lens_out), Lin, Lout, wrong ones: (lens_in, lens_out, why))
    "conv": (conv_call, 20, 10, [((21, 0, 0), (10, 0, 0), "lens_in > Lin"), ((20, 0, 0), (11, 0, 0), "lens_out > Lout"),
                                 ((-1, 0, 0), (0, 0, 0), "negative"), ((20, 4, 0), (10, -1, 0), "negative"),
                                 ((20, 4, 0), (10, 4, 0), "4 inputs yield 3 at most (left pad 1, stride 2)"), ((20, 0, 0), (10, 1, 0), "an inactive row with outputs")]),
    "convT": (convT_call, 10, 20, [((11, 0, 0), (20, 0, 0), "lens_in > Lin"), ((10, 0, 0), (21, 0, 0), "lens_out > Lout"),
                                   ((10, -2, 0), (20, 0, 0), "negative"), ((10, 3, 0), (20, 8, 0), "3 inputs yield 7 at most"),
                                   ((10, 0, 0), (20, 2, 0), "an inactive row with outputs")]),
    "cfirst": (cfirst_call, 20, 10, [((20, 0, 0), (11, 0, 0), "lens_out > Lout"), ((-1, 0, 0), (0, 0, 0), "negative"),
                                     ((20, 4, 0), (10, 4, 0), "4 inputs yield 3 at most (left pad 1, stride 2)"), ((20, 0, 0), (10, 1, 0), "an inactive row with outputs")]),
}


@pytest.mark.parametrize("entry", list(PAIRS))
def test_refusals_of_the_two_sided_entry_points(lib, entry):
    call, Lin, Lout, wrong = PAIRS[entry]
    hi, ho = arr(0, 0, 0), arr(0, 0, 0)
    # every mix of NULL and given: only all four (and none: the dense call, not made here - it would launch) pass
    for mask in range(1, 15):
        args = [a if mask >> i & 1 else None for i, a in enumerate((hi, DUMMY, ho, DUMMY))]
        assert call(lib, *args) == ERR_ARG, (entry, mask)
    for li, lo, why in wrong:
        assert call(lib, arr(*li), DUMMY, arr(*lo), DUMMY) == ERR_ARG, (entry, why)
        assert lib.kalle_conv_last_plan() == 0
    # every row inactive: KALLE_OK without a device, and the plan word of the dense call on the same shapes
    assert call(lib, hi, DUMMY, ho, DUMMY) == 0
    from kalle_audio_amd import conv_ops
    if entry == "convT":
        rc, q = conv_ops.conv_transpose_plan(3, 8, 10, 8, 20, 4, stride=2, padding=1, prefer=2)
    else:
        rc, q = conv_ops.conv_plan(3, 8, 20, 8, 10, 4, stride=2, padding=1, prefer=1 if entry == "cfirst" else 2)
    assert rc == 0 and lib.kalle_conv_last_plan() == q["word"], (entry, hex(lib.kalle_conv_last_plan()), q)


def test_refusals_of_the_one_sided_entry_points(lib):
    h = arr(0, 0, 0)
    for call in (cfirstT_call, pad_call):
        assert call(lib, h, None) == ERR_ARG and call(lib, None, DUMMY) == ERR_ARG
        assert call(lib, arr(0, -1, 0), DUMMY) == ERR_ARG
        assert call(lib, arr(0, 21, 0), DUMMY) == ERR_ARG          # past Lout = 20 / past Lin = 20
        assert call(lib, h, DUMMY) == 0                             # all inactive: nothing launched
    rc, q = __import__("kalle_audio_amd").conv_ops.conv_transpose_plan(3, 8, 10, 8, 20, 4, stride=2, padding=1, prefer=1)
    assert cfirstT_call(lib, h, DUMMY) == 0 and lib.kalle_conv_last_plan() == q["word"] and q["family"] == 7
    # the dense checks still come first: a bad shape is refused whatever the lengths say
    assert lib.kalle_conv1d_fwd_lens(DUMMY, F32, DUMMY, None, DUMMY, F32, 3, 8, 20, 8, 12, 4, 2, 1, 1, None, None, h, DUMMY, h, DUMMY, None) == ERR_ARG


def test_cases_get_their_family():
    for c in lc.CASES:
        rc, q = lc.plan(c)
        assert rc == 0 and q["family"] == c["family"], (lc.cid(c), rc, q)
        assert max(lc.lens_out(c)) == c["Lout"], lc.cid(c)
    assert {c["family"] for c in lc.CASES} == set(range(1, 8))
    assert {c["family"] for c in lc.CASES if c["xdt"] != F32 or c["ydt"] != F32} >= {1, 2, 3, 4}


# ================================================================================================ the Python layer
def _ae(antialias=False, **kw):
    from kalle_audio_amd.stable_audio_tools.models import autoencoders as A
    cfg = dict(channels=8, c_mults=[1, 2], strides=[2, 3], use_snake=True, antialias_activation=antialias)
    enc = A.OobleckEncoder(in_channels=1, latent_dim=8, **cfg)
    dec = A.OobleckDecoder(out_channels=1, latent_dim=4, **cfg, **kw)
    return A.AudioAutoencoder(enc, dec, latent_dim=4, downsampling_ratio=6, sample_rate=16000, io_channels=1).requires_grad_(False)


def test_python_refusals():
    from kalle_audio_amd import conv_ops, flows
    from kalle_audio_amd.stable_audio_tools.models.pretransforms import AutoencoderPretransform
    ae = _ae()
    z, wav = torch.zeros(3, 4, 10), torch.zeros(3, 1, 60)
    for bad in ([10, 5], [10, 5, 3, 1], [10, 0, 3], [11, 5, 3], [-1, 5, 3]):
        with pytest.raises(ValueError):
            ae.decode(z, lengths=bad)
    for bad in ([60, 30], [61, 30, 12], [60, 0, 12]):
        with pytest.raises(ValueError):
            ae.encode(wav, lengths=bad)
    with pytest.raises(ValueError, match="too short"):
        ae.encode(wav, lengths=[60, 30, 2])                        # under one latent frame
    for fn, x in ((ae.decode_audio, z), (ae.encode_audio, wav)):
        with pytest.raises(NotImplementedError, match="chunked"):
            fn(x, chunked=True, lengths=[5, 5, 5])
    with pytest.raises(NotImplementedError, match="chunked"):
        AutoencoderPretransform(ae, chunked=True).decode(z, lengths=[5, 5, 5])
    aa = _ae(antialias=True)
    with pytest.raises(NotImplementedError, match="antialias"):
        aa.decode(z, lengths=[10, 5, 3])
    with pytest.raises(NotImplementedError, match="antialias"):
        aa.encode(wav, lengths=[60, 30, 12])
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="gradients"):
            ae.decode(z.clone().requires_grad_(True), lengths=[10, 5, 3])
        tr = _ae().requires_grad_(True)
        with pytest.raises(NotImplementedError, match="gradients"):
            tr.encode(wav, lengths=[60, 30, 12])
    with pytest.raises(NotImplementedError, match="mel-VAE"):
        flows.BigVGANFlowVAE._no_lengths([1, 2])
    # conv_ops itself: lengths past the tensor, the wrong count, a gradient
    lens = conv_ops.RaggedLengths([(12, 5, 3)], "cpu").at(0)
    w = torch.zeros(4, 3, 8)
    with pytest.raises(ValueError):
        conv_ops.conv1d(torch.zeros(3, 4, 10), w, None, Cout=8, K=3, padding=1, lens=lens)
    with pytest.raises(ValueError):
        conv_ops.conv1d(torch.zeros(2, 4, 12), w, None, Cout=8, K=3, padding=1, lens=lens)
    with torch.enable_grad(), pytest.raises(NotImplementedError):
        conv_ops.conv1d(torch.zeros(3, 4, 12, requires_grad=True), w, None, Cout=8, K=3, padding=1, lens=lens)
    with pytest.raises(ValueError, match="planned"):
        lens.map(lambda L: L + 1)                                  # a level the stack did not plan


def test_list_grouping():
    """sorted by length, B x Lmax_out under the cap, every index once"""
    ae = _ae()
    sizes = [33, 1, 17, 2, 5, 40, 3]
    groups = ae._ragged_groups(sizes, lambda T: T * 6, 3 * 17 * 6)
    assert sorted(i for g in groups for i in g) == list(range(len(sizes)))
    flat = [sizes[i] for g in groups for i in g]
    assert flat == sorted(sizes)
    for g in groups:
        assert len(g) == 1 or len(g) * max(sizes[i] for i in g) * 6 <= 3 * 17 * 6
    assert [[sizes[i] for i in g] for g in groups] == [[1, 2, 3, 5], [17], [33], [40]], groups
    assert ae._default_cap() == ae.chunk_batch * 128 * 6


# ================================================================================================ length propagation
@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("strides", [(2, 4, 5), (3, 8), (5, 3, 2), (8, 2)])
def test_length_propagation_matches_torch(strides, nearest):
    """the levels a stack plans (each layer's own formula, row by row) are the lengths torch's conv1d / conv_transpose1d produce
    for the row alone, layer by layer: every layer type of the stack, odd strides, input lengths off the ratio"""
    from kalle_audio_amd import conv_ops
    from kalle_audio_amd.stable_audio_tools.models import autoencoders as A
    import math
    ratio = math.prod(strides)
    cfg = dict(channels=4, c_mults=[1] * len(strides), strides=list(strides), use_snake=False)
    enc = A.OobleckEncoder(in_channels=1, latent_dim=4, **cfg)
    dec = A.OobleckDecoder(out_channels=1, latent_dim=4, use_nearest_upsample=nearest, **cfg)

    def torch_lengths(L, mods):
        """L through every length-changing layer, by running torch on a row of zeros"""
        out, x = [L], torch.zeros(1, 1, L)
        for m in mods:
            if isinstance(m, int):
                x = x.repeat_interleave(m, 2)
            elif isinstance(m, A.WNConvTranspose1d):
                x = TF.conv_transpose1d(x, torch.zeros(1, 1, m.kernel_size), None, m.stride, m.padding)
            else:
                pr = m.padding if m.pad_right is None else m.pad_right
                x = TF.conv1d(TF.pad(x, (m.padding, pr)), torch.zeros(1, 1, m.kernel_size), None, m.stride, 0, m.dilation)
            out.append(x.shape[2])
        return out

    n = len(enc.layers)
    enc_mods = [enc.layers[0]] + [enc.layers[i].layers[4] for i in range(1, n - 2)] + [enc.layers[n - 1]]
    for L in (2 * ratio, 2 * ratio + 1, 3 * ratio - 1, 7 * ratio + ratio // 2, 257):
        got = [lv[0] for lv in conv_ops.plan_levels([L], enc.length_maps())]
        assert got == torch_lengths(L, enc_mods), (strides, L, got)
    n = len(dec.layers)
    dec_mods = [dec.layers[0]] + [dec.layers[i].nearest if nearest else dec.layers[i].layers[1] for i in range(1, n - 3)] + [dec.layers[n - 2]]
    for T in (1, 2, 5, 17, 33):
        got = [lv[0] for lv in conv_ops.plan_levels([T], dec.length_maps())]
        assert got == torch_lengths(T, dec_mods) and got[-1] == T * ratio, (strides, T, got)
    # the layers inside a block keep the length (k = 7 at every dilation, k = 1, the 'same' conv behind the repetition)
    blk = dec.layers[1]
    for m in [blk.layers[j].layers[k] for j in (2, 3, 4) for k in (1, 3)] + ([blk.layers[1][1]] if nearest else []):
        assert all(m.out_len(L) == L for L in (1, 2, 5, 27, 64)), m


# ================================================================================================ the definition, the sensitivity
DIRECTED = [(cid, d) for cid in vr.CIDS for d in ("decode", "encode") if d == "decode" or cid in vr.ENC_CIDS]


@pytest.mark.parametrize("cid,direction", DIRECTED)
def test_masked_stack_equals_the_rows_alone(cid, direction):
    """fp64: every layer's output cut to its rows' lengths = the row run alone (proves the definition; not a device check)"""
    for b, (a, m) in enumerate(zip(vr.alone(cid, direction), vr.masked(cid, direction))):
        assert a.shape == m.shape and a.dtype == torch.float64
        assert (a - m).abs().max() <= 1e-12 * max(1.0, a.abs().max().item()), (cid, direction, b)
    ratio = vo.CASES[cid]["ratio"]
    if direction == "decode":
        assert [a.shape[2] for a in vr.alone(cid, direction)] == [T * ratio for T in vr.DEC_T]


@pytest.mark.parametrize("cid,direction", DIRECTED)
def test_defects_show_on_the_reference_alone(cid, direction):
    """each seeded defect - first of all the zero-padded batch, the only substitute there was - lies 2 M r or more from the rows
    run alone; the triples of vr.BLIND lie under it.  (What the device test's defect checks rely on.)"""
    for defect in vr.DEFECTS:
        rho = vr.rho(vr.masked(cid, direction, defect), cid, direction)
        worst = max(rho.values())
        print(f"{cid} {direction} {defect}: " + " ".join(f"{v:.3g}" for v in rho.values()))
        if (direction, cid, defect) in vr.BLIND:
            assert worst < vr.SHOWN, (cid, direction, defect, rho)
        else:
            assert worst >= vr.SHOWN, (cid, direction, defect, rho)
    assert all(t[2] in vr.DEFECTS and t[1] in vr.CIDS for t in vr.BLIND)


def test_padding_error_is_of_the_order_of_the_signal():
    """the figure behind the feature: decoding a zero-padded latent differs from decoding it alone by a sizeable share of the
    waveform's peak, from several frames before the end on"""
    for cid in ("O1", "O2", "O4", "O5"):
        al, pd = vr.alone(cid, "decode"), vr.masked(cid, "decode", "padded")
        for b in range(3):                                         # T = 1, 2, 5 padded to 33
            assert (al[b] - pd[b]).abs().max() >= 0.1 * al[b].abs().max(), (cid, b)
