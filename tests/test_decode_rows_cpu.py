"""CPU side of the batched decode path: the reference helper of tests/decode_rows_cases.py against torch, the 1 % cap on ambiguous
prologue elements for every input tests/test_decode_rows_gpu.py commits to, the argument refusals of the three new entry points
that return before any HIP call (the library loads without a device), and kalle_llama_decode_ws_bytes_rows against the layout
the header publishes."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc  # noqa: E402
import decode_rows_cases as rc  # noqa: E402
import kernel_refs as kr  # noqa: E402

ERR_ARG = -1
FAKE = ctypes.c_void_p(4096)        # a non-NULL pointer for calls that must return before touching memory


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def test_gemm_rows_ref_is_a_linear_layer_per_row():
    g = torch.Generator().manual_seed(1)
    W, X, res = torch.randn((70, 64), generator=g), torch.randn((3, 64), generator=g), torch.randn((3, 70), generator=g)
    want = torch.nn.functional.linear(X.double(), W.double())
    assert torch.allclose(rc.gemm_rows_ref(W, X), want, rtol=0, atol=1e-12)
    assert torch.allclose(rc.gemm_rows_ref(W, X, res), want + res.double(), rtol=0, atol=1e-12)
    for r in range(3):      # a row is the one-row reference
        assert torch.allclose(rc.gemm_rows_ref(W, X)[r], kr.gemv(W.double(), X[r].double()), rtol=0, atol=1e-12)


def test_rope_tables_match_the_single_sequence_ones():
    import llama_hd128_cases as lc128
    for hd, one in ((64, dc.rope_tables), (128, lc128.rope_tables)):
        for a, b in zip(rc.rope_tables(41, hd), one(41)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("N,K,nsplit", rc.GEMM_SHAPES + rc.GEMM_TILE_SHAPES)
@pytest.mark.parametrize("R", rc.GEMM_ROWS)
def test_ambiguous_prologue_elements_stay_under_the_cap_gemm(N, K, nsplit, R):
    x, gamma = rc.gemm_inputs(N, K, R, rc.PRO_RMS)
    hf, _ = rc.gemm_inputs(N, K, R, rc.PRO_SWIGLU)
    for r in range(R):
        xh = kr.decode_rms_prologue(x[r].double(), gamma.double(), rc.EPS)
        assert kr.bf16_ambiguous(xh, dc.rms_window(xh)).sum().item() <= 0.01 * K, ("rms", N, K, R, r)
        h = hf[r].double()
        assert kr.bf16_ambiguous(kr.decode_swiglu_prologue(h), dc.swiglu_window(h)).sum().item() <= 0.01 * K, ("swiglu", N, K, R, r)


@pytest.mark.parametrize("name", list(rc.STEP_CASES))
def test_ambiguous_prologue_elements_stay_under_the_cap_step(name):
    c = rc.STEP_CASES[name]
    x, gamma = rc.step_inputs(c)
    for r, t in enumerate(c["t0"]):
        if t >= 0:
            xh = kr.decode_rms_prologue(x[r].double(), gamma.double(), rc.EPS)
            assert kr.bf16_ambiguous(xh, dc.rms_window(xh)).sum().item() <= 0.01 * xh.numel(), (name, r)


def gemm_args(R=3, N=70, K=64, ldx=None, pro=0, nsplit=None, y2=None, off=None):
    return (FAKE, K if ldx is None else ldx, pro, FAKE, ctypes.c_float(1e-5), FAKE, FAKE, K, FAKE, N, 1, y2, N if nsplit is None else nsplit,
            off, None, 0, None, R, N, K, None)


def test_gemm_rows_refusals(lib):
    for kw in (dict(R=0), dict(R=17), dict(K=60), dict(K=32776), dict(N=0), dict(pro=3), dict(ldx=60), dict(nsplit=32),
               dict(nsplit=80), dict(pro=1, ldx=66)):
        assert lib.kalle_gemm_rows_fused(*gemm_args(**kw)) == ERR_ARG, kw
    for R, K in ((0, 64), (17, 64), (3, 60), (3, 32776)):
        assert lib.kalle_gemm_rows_bf16(FAKE, K, FAKE, K, FAKE, 70, 1, None, 0, R, 70, K, None) == ERR_ARG, (R, K)
    assert lib.kalle_gemm_rows_bf16(FAKE, 64, FAKE, 64, FAKE, 70, 2, None, 0, 3, 70, 64, None) == ERR_ARG       # y_dtype
    assert lib.kalle_gemm_rows_bf16(None, 64, FAKE, 64, FAKE, 70, 1, None, 0, 3, 70, 64, None) == ERR_ARG


def attn_call(lib, nk, R=None, hd=64, rot=64, H=4, Hkv=2, stride=8 * 512):
    arr = (ctypes.c_int32 * len(nk))(*nk)
    w = 2 * Hkv * hd
    return lib.kalle_attention_decode_rows(FAKE, H * hd, 0, FAKE, w, 0, FAKE, w, Hkv * hd, stride, FAKE, H * hd, None, FAKE, FAKE, rot,
                                           ctypes.cast(arr, ctypes.c_void_p), len(nk) if R is None else R, H, Hkv, hd, None)


def test_attention_rows_refusals_leave_plan_zero(lib):
    for kw in (dict(nk=[], R=0), dict(nk=[1] * 17), dict(nk=[1, 15361, 3]), dict(nk=[1, 2, 3], hd=32, rot=32),
               dict(nk=[1, 2, 3], hd=128, rot=64), dict(nk=[1, 2, 3], rot=32), dict(nk=[1, 2, 3], Hkv=3), dict(nk=[1, 2, 3], stride=12)):
        assert attn_call(lib, **kw) == ERR_ARG, kw
        assert lib.kalle_attn_last_plan() == 0
    assert attn_call(lib, [0, -1, 0]) == 0 and lib.kalle_attn_last_plan() == 0        # every row inactive: nothing to launch


def test_step_rows_refusals_and_workspace_bytes(lib):
    from kalle_audio_amd import _lib
    arr = (_lib.LlamaLayer * 1)()
    for f, _ in _lib.LlamaLayer._fields_:
        setattr(arr[0], f, 4096)

    def step(t0, R=None, H=2, Hkv=1, inner=8, hd=64, rows=40, layers=arr):
        t = (ctypes.c_int32 * max(len(t0), 1))(*t0)
        return lib.kalle_llama_decode_step_rows(ctypes.cast(layers, ctypes.c_void_p), 1, FAKE, FAKE, len(t0) if R is None else R, H, Hkv, inner, hd, ctypes.c_float(1e-5),
                                                ctypes.cast(t, ctypes.c_void_p), rows, FAKE, FAKE, FAKE, None)

    for kw in (dict(t0=[], R=0), dict(t0=[0] * 17), dict(t0=[0, 40, 1]), dict(t0=[0, 1, 2], Hkv=3), dict(t0=[0, 1, 2], inner=12),
               dict(t0=[0, 1, 2], hd=32), dict(t0=[0, 1, 2], H=513), dict(t0=[0, 15360, 2], rows=20000), dict(t0=[0, 1, 2], inner=32776)):
        assert step(**kw) == ERR_ARG, kw
        assert lib.kalle_attn_last_plan() == 0
    arr[0].wug = None
    assert step([0, 1, 2]) == ERR_ARG
    arr[0].wug = 4096
    assert step([-1, -1, -1]) == 0 and lib.kalle_attn_last_plan() == 0                 # every row inactive
    for R, H, inner, hd in ((1, 2, 8, 64), (3, 2, 8, 64), (3, 2, 8, 128), (16, 32, 8192, 64), (16, 24, 8192, 128), (5, 2, 2056, 64)):
        assert lib.kalle_llama_decode_ws_bytes_rows(R, H, 1, inner, hd) == rc.ws_bytes(R, H, inner, hd), (R, H, inner, hd)
    for a in ((0, 2, 1, 8, 64), (17, 2, 1, 8, 64), (3, 2, 1, 8, 32), (3, 0, 1, 8, 64)):
        assert lib.kalle_llama_decode_ws_bytes_rows(*a) == ERR_ARG, a
