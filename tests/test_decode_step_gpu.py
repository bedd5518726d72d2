"""-m gpu: the four forms of the decode step (bf16 / e4m3 weights, one row / R rows) behind their one sequencer (csrc/llasa.hip:
decode_step), two layers at the smallest legal shape and either head dim.  A NULL weight (bf16) or scale (e4m3) in the SECOND
layer is refused before the first layer runs: nothing is written anywhere.  With the hole repaired, ops.llama_decode_step on a
plan over the same tensors and a direct call of the C entry point give the same bits (every kernel sums in a fixed order)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_rows_cases as rc  # noqa: E402
import fp8_refs as f8  # noqa: E402
import test_decode_rows_gpu as tr  # noqa: E402
import test_decode_w8_gpu as tw  # noqa: E402
from gpu_checks import _exact  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
P, iarr = tr.P, tr.iarr
# form -> (e4m3 weights, t0 per row; negative = inactive), the C entry point
FORMS = {"one-row": (False, (3,), "kalle_llama_decode_step_hd"), "one-row-e4m3": (True, (3,), "kalle_llama_decode_step_w8"),
         "rows": (False, (3, -1, 5), "kalle_llama_decode_step_rows"), "rows-e4m3": (True, (3, -1, 5), "kalle_llama_decode_step_rows_w8")}


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


@pytest.fixture(scope="module")
def table():
    return f8.decode_table().cuda()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("form", list(FORMS))
def test_hole_in_layer_1_writes_nothing_and_the_wrapper_matches_the_entry_point(kl, table, form, hd):
    ops, lib = kl
    w8, t0, entry = FORMS[form]
    c = dict(hd=hd, H=2, Hkv=1, inner=16, t0=t0, rows=8, seed=950 + hd + len(t0), one=len(t0) == 1)
    if w8:
        W = tw.Setup(kl, table, c, 2)
        S, arr = W.s, W.arr
        tensors = [(L.input_norm, *q["wqkv"], *q["wo"], L.post_norm, *q["wug"], *q["wdown"], L.cache) for L, q in zip(S.layers, W.q)]
    else:
        S = tr.Setup(lib, c, 2)
        arr, tensors = S.arr, [tuple(L.fields()) for L in S.layers]
    R, D = len(t0), S.D

    def call():
        pos = (iarr(list(t0)),) if R > 1 else (t0[0],)
        rows = (R,) if R > 1 else ()
        rcode = getattr(lib, entry)(ctypes.cast(arr, ctypes.c_void_p), 2, P(S.x), P(S.out), *rows, c["H"], c["Hkv"], c["inner"], hd,
                                    ctypes.c_float(rc.EPS), *pos, c["rows"], P(S.cos), P(S.sin), P(S.ws), None)
        torch.cuda.synchronize()
        return rcode

    field = "sdown" if w8 else "wdown"
    old = getattr(arr[1], field)
    setattr(arr[1], field, None)
    assert call() == ERR_ARG and ops.attn_last_plan() == 0
    assert torch.isnan(S.out).all() and (S.wsbuf == 0xFF).all()
    for l, L in enumerate(S.layers):
        _exact(L.cache, L.cache_before, f"cache of layer {l} after the refused step")
    setattr(arr[1], field, old)

    plan = ops.llama_decode_plan(tensors, c["H"], c["Hkv"], c["inner"], S.x.device, head_dim=hd, rows=R if R > 1 else None)
    x, pos = (S.x, list(t0)) if R > 1 else (S.x.view(D), t0[0])
    got = ops.llama_decode_step(plan, x, pos, c["rows"], (S.cos, S.sin), rc.EPS).view(R, D).clone()
    torch.cuda.synchronize()
    got_kv = [L.cache.clone() for L in S.layers]
    for L in S.layers:
        L.cache.copy_(L.cache_before)
    assert call() == 0
    for r, t in enumerate(t0):
        if t < 0:
            assert (got[r] == 0).all() and torch.isnan(S.out[r]).all()          # the plan's zero-initialised buffer; the caller's NaN
            continue
        assert torch.isfinite(S.out[r]).all() and torch.equal(got[r], S.out[r]), (form, hd, r)
        for l, L in enumerate(S.layers):
            assert torch.isfinite(L.cache[r, t]).all() and torch.equal(got_kv[l][r, t], L.cache[r, t]), (form, hd, l, r)
            _exact(got_kv[l][r], L.cache[r], f"cache of layer {l}, row {r}")
