"""CPU: the yardstick of the e4m3 tests (tests/fp8_refs.py) - the decode table against torch's own cast for all 256 codes, the
reference quantiser's properties per element and independently of that cast, and the "lossless" weights the module tests rest
on.  These pass without the feature by design: they pin what the GPU tests compare against."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_refs as f8  # noqa: E402


def test_decode_table_matches_the_definition_and_torch_for_all_256_codes():
    t = f8.decode_table()
    assert t[0x7E].item() == 448.0 and t[0xFE].item() == -448.0
    assert torch.isnan(t[0x7F]) and torch.isnan(t[0xFF]) and int(torch.isnan(t).sum()) == 2
    assert t[0x00].item() == 0.0 and t[0x01].item() == 2.0 ** -9 and t[0x08].item() == 2.0 ** -6 and t[0x38].item() == 1.0
    ref = torch.arange(256, dtype=torch.int16).to(torch.uint8).view(torch.float8_e4m3fn).float().double()
    same = (t == ref) | (torch.isnan(t) & torch.isnan(ref))
    assert same.all(), same.logical_not().nonzero().flatten().tolist()
    assert torch.equal(torch.signbit(t[~torch.isnan(t)]), torch.signbit(ref[~torch.isnan(ref)]))     # (0x80 is -0)


def test_fnuz_table_is_a_different_decoding():
    t, z = f8.decode_table(), f8.decode_table_fnuz()
    fin = ~torch.isnan(t) & ~torch.isnan(z) & (t != 0)
    assert torch.equal(z[fin] * 2, t[fin]) and z[0x7F].item() == 240.0 and torch.isnan(z[0x80])


def _weights():
    g = torch.Generator().manual_seed(11)
    w = (torch.randn((37, 208), generator=g) / 208 ** 0.5).to(torch.bfloat16)
    w[3] = 0
    w[5] = 0
    w[5, 17] = -0.3
    w[7] = (torch.randn(208, generator=g) * 1e-3).to(torch.bfloat16)
    w[7, 0] = 500.0                       # most of the row below 2^-6 after scaling, many below the smallest code
    return w


def test_reference_quantiser_properties():
    w = _weights()
    codes, scale = f8.quantize_ref(w)
    table = f8.decode_table()
    assert not ((codes & 0x7F) == 0x7F).any(), "a NaN code"
    assert scale[3].item() == 1.0 and (codes[3] == 0).all()
    assert scale[5].item() == torch.tensor(0.3).to(torch.bfloat16).float().item() / 448 and codes[5, 17].item() == 0xFE
    assert int((codes[5] != 0).sum()) == 1
    t = f8.quantize_t(w).double()
    assert (t.abs() <= 448.0 * (1 + 2.0 ** -23)).all()
    dq = table[codes.long()]
    err = (dq - t.clamp(-448, 448)).abs()
    # the distance from t to the nearest code, by search in the sorted finite values (independent of the cast)
    vals = torch.unique(table[~torch.isnan(table)])
    i = torch.searchsorted(vals, t.clamp(-448, 448).contiguous()).clamp(1, vals.numel() - 1)
    nearest = torch.minimum((vals[i] - t.clamp(-448, 448)).abs(), (vals[i - 1] - t.clamp(-448, 448)).abs())
    assert (err <= nearest + 2.0 ** -20 * t.abs()).all()
    big = t.abs() >= 2.0 ** -6
    assert (err[big] <= 2.0 ** -4 * t.abs()[big]).all() and (err[~big] <= 2.0 ** -10).all()
    assert int((~big).sum()) > 100 and int(big.sum()) > 1000


def test_unclamped_cast_would_emit_nan():
    x = torch.tensor([500.0])
    assert torch.isnan(x.to(torch.float8_e4m3fn).float()).all()
    assert x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).item() == 0x7E


def test_lossless_weights_quantise_to_themselves():
    g = torch.Generator().manual_seed(5)
    w, codes, scale = f8.lossless_weights(19, 144, g)
    assert w.dtype == torch.bfloat16
    c2, s2 = f8.quantize_ref(w)
    assert torch.equal(s2, scale) and torch.equal(c2, codes)
    assert torch.equal(torch.log2(scale.double()), torch.log2(scale.double()).round())
    dq = f8.decode_table()[c2.long()] * s2.double()[:, None]
    assert torch.equal(dq, w.double())
    assert ((codes == 0x7E).any(1) & (codes == 0xFE).any(1)).all()
