"""CPU side of the wide decode path (17 .. 64 rows per read of the weights): the reseed table of tests/decode_wide_cases.py - every
committed prologue input under the 1 % ambiguity cap, every reseed the FIRST that is - the refusals of the three entry points,
which return before any HIP call (the library loads without a device), kalle_llama_decode_ws_bytes_wide against the published
layout, the ABI version, and `rows=` of generate_batch on the fake decoder and heads of tests/test_generation_loop_cpu.py."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_rows_cases as rc  # noqa: E402
import decode_wide_cases as wc  # noqa: E402
import test_generation_loop_cpu as tg  # noqa: E402

from kalle_audio_amd import generation as gen  # noqa: E402

ERR_ARG = -1
FAKE = ctypes.c_void_p(4096)        # a non-NULL pointer for calls that must return before touching memory


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("N,K,nsplit", wc.GEMM_SHAPES)
@pytest.mark.parametrize("R", wc.GEMM_ROWS)
def test_reseed_table(N, K, nsplit, R):
    for pro in (wc.PRO_RMS, wc.PRO_SWIGLU):
        k = wc.RESEED.get((N, K, R, pro), 0)
        assert wc.under_cap(*wc.gemm_inputs(N, K, R, pro), pro, K), (N, K, R, pro)
        for earlier in range(k):
            assert not wc.under_cap(*wc.draw(N, K, R, pro, earlier), pro, K), (N, K, R, pro, earlier, "an earlier seed meets the cap")
    assert all(key[:2] in {s[:2] for s in wc.GEMM_SHAPES} and key[2] in wc.GEMM_ROWS for key in wc.RESEED)


def test_seed_formula_and_the_16_row_draws_agree():
    assert wc.seed(70, 64, 33, 2, 13) == 7000 + 131 * 70 + 17 * 64 + 33 + 2000 + 1300000
    for pro in (0, 1, 2):           # reseed 0 is decode_rows_cases' own draw
        a, b = wc.draw(264, 1000, 8, pro, 0), rc.gemm_inputs(264, 1000, 8, pro)
        assert torch.equal(a[0], b[0]) and (a[1] is None) == (b[1] is None)


def test_abi_version_and_bound(lib):
    from kalle_audio_amd import ops
    assert lib.kalle_abi_version() == 2
    assert ops.DECODE_WIDE_MAX_ROWS == 64 and ops.DECODE_MAX_ROWS == 16


def gemm_args(R=33, N=70, K=64, ldx=None, pro=0, nsplit=None, y2=None, off=None, x=FAKE, gamma=FAKE, xhat=FAKE, ydt=1):
    return (x, K if ldx is None else ldx, pro, gamma, ctypes.c_float(1e-5), xhat, FAKE, K, FAKE, N, ydt, y2, N if nsplit is None else nsplit,
            off, None, 0, None, R, N, K, None)


def test_gemm_wide_refusals(lib):
    for R in (33, 3):               # the _rows list at either side of the forwarding point
        for kw in (dict(K=60), dict(K=32776), dict(N=0), dict(pro=3), dict(ldx=60), dict(nsplit=32), dict(nsplit=80), dict(pro=1, ldx=66),
                   dict(pro=1, gamma=None), dict(pro=2, ldx=64), dict(pro=1, xhat=None), dict(ydt=2), dict(x=None), dict(nsplit=32, y2=FAKE)):
            assert lib.kalle_gemm_rows_wide(*gemm_args(R=R, **kw)) == ERR_ARG, (R, kw)
    for R in (0, -1, 65, 1000):
        assert lib.kalle_gemm_rows_wide(*gemm_args(R=R)) == ERR_ARG, R
    none = (ctypes.c_int32 * 64)()
    a = list(gemm_args(R=64))
    a[16] = ctypes.cast(none, ctypes.c_void_p)
    assert lib.kalle_gemm_rows_wide(*a) == 0                                    # every row inactive: nothing launched


def test_step_wide_refusals_and_workspace_bytes(lib):
    from kalle_audio_amd import _lib
    arr = (_lib.LlamaLayer * 2)()
    for d in arr:
        for f, _ in _lib.LlamaLayer._fields_:
            setattr(d, f, 4096)

    def step(t0, R=None, H=2, Hkv=1, inner=8, hd=64, rows=40, ws=FAKE):
        t = (ctypes.c_int32 * max(len(t0), 1))(*t0)
        return lib.kalle_llama_decode_step_wide(ctypes.cast(arr, ctypes.c_void_p), 2, FAKE, FAKE, len(t0) if R is None else R, H, Hkv, inner, hd,
                                                ctypes.c_float(1e-5), ctypes.cast(t, ctypes.c_void_p), rows, FAKE, FAKE, ws, None)

    ok = [r % 30 for r in range(33)]
    for kw in (dict(t0=[], R=0), dict(t0=[0] * 65), dict(t0=ok[:32] + [40]), dict(t0=ok, Hkv=3), dict(t0=ok, inner=12), dict(t0=ok, hd=32),
               dict(t0=ok, H=513), dict(t0=ok[:32] + [15360], rows=20000), dict(t0=ok, inner=32776), dict(t0=ok, ws=None), dict(t0=[0] * 17, hd=32)):
        assert step(**kw) == ERR_ARG, kw
        assert lib.kalle_attn_last_plan() == 0
    arr[1].wug = None                                                           # a NULL in the second layer
    assert step(ok) == ERR_ARG
    arr[1].wug = 4096
    assert step([-1] * 64) == 0 and lib.kalle_attn_last_plan() == 0             # every row inactive
    assert step([-1] * 3) == 0                                                  # (forwarded to the _rows step)
    for R, H, inner, hd in ((17, 2, 8, 64), (33, 2, 8, 128), (64, 32, 8192, 64), (64, 24, 8192, 128), (33, 2, 2056, 64), (5, 2, 8, 64)):
        assert lib.kalle_llama_decode_ws_bytes_wide(R, H, 1, inner, hd) == rc.ws_bytes(R, H, inner, hd), (R, H, inner, hd)
    for a in ((0, 2, 1, 8, 64), (65, 2, 1, 8, 64), (33, 2, 1, 8, 32), (33, 0, 1, 8, 64), (33, 2, 0, 8, 64), (33, 2, 1, 0, 64), (33, 513, 1, 8, 64),
              (33, 2, 1, 32776, 64)):
        assert lib.kalle_llama_decode_ws_bytes_wide(*a) == ERR_ARG, a


# ------------------------------------------------------------------------------------------------ rows= of generate_batch
class Owner(tg.FakeOwner):
    """FakeOwner with what generate_batch asks of a task model beyond `generate`"""

    def _generate_device_head(self, prompts, thres, max_length, noise, stop_lag, refill=False, rows=None):
        return gen.generate(self, prompts, thres, max_length, self.spec(), noise, stop_lag, refill, rows=rows)


def batch(owner, caps, device_head, **kw):
    N = len(caps)
    noise = owner.noise(N) if device_head else None
    return gen.generate_batch(owner, tg.prompts_of([3 + u % 4 for u in range(N)]), 0.0, list(caps), device_head, noise, 0, 1, **kw)


@pytest.mark.parametrize("device_head", [False, True], ids=["host", "device"])
def test_rows_33_refill_follows_refill_steps(device_head):
    caps = tg.seeded_caps(5, 70, 2, 40)
    owner = Owner([None] * 70, rows=16, top=max(caps))
    with tg.without_device():
        out = batch(owner, caps, device_head, refill=True, rows=33)
    total, first = gen.refill_steps(caps, 33, 0)
    assert owner.last_refill_trace == [(u, r, t, n) for u, ((r, t), n) in enumerate(zip(first, caps))]
    decodes = [e for e in owner.log if e[0] == "decode"]
    assert len(decodes) == total - 1 and all(len(e[1]) == 33 for e in decodes)
    assert len(owner.base_model.model.caches) == 1 and len(owner.base_model.model.caches[0]["len"]) == 33
    for u, n in enumerate(caps):
        assert torch.equal(out[u], tg.frames_of(u, n)), u


@pytest.mark.parametrize("device_head", [False, True], ids=["host", "device"])
def test_grouped_mode_cuts_groups_of_rows(device_head):
    caps = tg.seeded_caps(6, 70, 2, 20)
    owner = Owner([None] * 70, rows=16, top=max(caps))
    with tg.without_device():
        out = batch(owner, caps, device_head, rows=33)
    assert [len(c["len"]) for c in owner.base_model.model.caches] == [33, 33, 4]
    for u, n in enumerate(caps):
        assert torch.equal(out[u], tg.frames_of(u, n)), u


def test_rows_none_is_the_grouping_at_16():
    caps = tg.seeded_caps(7, 40, 2, 12)
    for ibr, want in ((16, [16, 16, 8]), (64, [16, 16, 8]), (5, [5] * 8)):      # an infer_batch_rows above 16 stays clamped
        owner = Owner([None] * 40, rows=ibr, top=max(caps))
        with tg.without_device():
            batch(owner, caps, False)
        assert [len(c["len"]) for c in owner.base_model.model.caches] == want, ibr
        logs = []
        for kw in ({}, dict(rows=None), dict(rows=min(ibr, 16))):
            o = Owner([None] * 40, rows=ibr, top=max(caps))
            with tg.without_device():
                batch(o, caps, True, **kw)
            logs.append(o.log)
        assert logs[0] == logs[1] == logs[2]


@pytest.mark.parametrize("rows", [0, 65, 2.5, "8", -1, True])
@pytest.mark.parametrize("refill", [False, True])
def test_bad_rows_is_a_value_error(rows, refill):
    owner = Owner([None] * 3, top=4)
    with pytest.raises(ValueError, match="rows"):
        batch(owner, [4, 4, 4], False, refill=refill, rows=rows)
    with pytest.raises(ValueError, match="rows"):
        gen.generate_batch(owner, [], 0.0, 4, False, None, 0, 1, rows=rows)
    assert owner.log == []


def test_e4m3_with_17_rows_is_not_implemented():
    owner = Owner([None] * 20, top=4)
    owner.base_model.model._decode_fmt = "e4m3"
    for refill in (False, True):
        with pytest.raises(NotImplementedError, match=r"(?s)e4m3.*17"):
            batch(owner, [4] * 20, False, refill=refill, rows=17)
    assert owner.log == []
    with tg.without_device():
        assert len(batch(owner, [4] * 20, False, rows=16)) == 20               # 16 rows: the e4m3 step exists
