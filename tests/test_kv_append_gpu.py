"""-m gpu: kalle_kv_append_varlen (ops.kv_append_varlen) bit for bit against torch slicing and against the numpy reference of
tests/refill_cases.py, on a cache filled with NaN: every position outside the named ones, other rows included, must still hold
the NaN it held.  Cases (refill_cases.KV_CASES): kvw 256 and 1024, lengths 1, 7 and one row past the kernel's row chunk,
destination rows out of order, t0 = 0 and > 0, packed buffers with gaps.  A reference with two destination rows swapped must fail."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refill_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
_ID = lambda c: c["id"]


def bits(t):
    return t.view(torch.int16).cpu()


def run(dev, c, dst=None):
    """(cache after the call, the untouched copy, src, seqs) for case c"""
    from kalle_audio_amd import ops
    g = torch.Generator().manual_seed(17)
    src = torch.randn(c["total"], c["ld"], generator=g).to(torch.bfloat16).to(dev)
    cache = torch.full((c["R"], c["cache_rows"], c["kvw"]), float("nan"), dtype=torch.bfloat16, device=dev)
    before = cache.clone()
    seqs = ops.Packed(c["row0"], c["lens"], c["total"], dev)
    out = ops.kv_append_varlen(src, seqs, cache, c["dst"] if dst is None else dst, c["t0"], src_off=c["src_off"])
    assert out is cache
    torch.cuda.synchronize()
    return cache, before, src


def sliced(c, src, before, dst=None):
    want = before.clone()
    for r0, n, d, t in zip(c["row0"], c["lens"], c["dst"] if dst is None else dst, c["t0"]):
        want[d, t:t + n] = src[r0:r0 + n, c["src_off"]:c["src_off"] + c["kvw"]]
    return want


@pytest.mark.parametrize("c", rc.KV_CASES, ids=_ID)
def test_kv_append_bit_for_bit(dev, c):
    assert rc.KV_ROWS + 1 in c["lens"] or 2 * rc.KV_ROWS in c["lens"]          # more than one workgroup per sequence
    cache, before, src = run(dev, c)
    want = sliced(c, src, before)
    assert torch.equal(bits(cache), bits(want))
    ref = rc.kv_append_ref(bits(src).numpy().view(np.uint16), c["src_off"], bits(before).numpy().view(np.uint16), c["row0"],
                           c["lens"], c["dst"], c["t0"])
    assert np.array_equal(bits(cache).numpy().view(np.uint16), ref)
    named = torch.zeros(cache.shape[:2], dtype=torch.bool)
    for n, d, t in zip(c["lens"], c["dst"], c["t0"]):
        named[d, t:t + n] = True
    got = cache.float().cpu()
    assert torch.isnan(got[~named]).all(), "a position outside the named ones was written"
    assert not torch.isnan(got[named]).any()
    assert named.sum().item() == sum(c["lens"])


def test_kv_append_swapped_destination_rows_fail(dev):
    c = rc.KV_BASE
    cache, before, src = run(dev, c)
    swapped = [c["dst"][1], c["dst"][0]] + c["dst"][2:]
    assert torch.equal(bits(cache), bits(sliced(c, src, before)))
    assert not torch.equal(bits(cache), bits(sliced(c, src, before, dst=swapped)))
    other, _, _ = run(dev, c, dst=swapped)                                      # and the kernel follows the rows it is given
    assert torch.equal(bits(other), bits(sliced(c, src, before, dst=swapped)))
