"""CPU: the planner of kalle_gemm_bf16 through its host query kalle_gemm_plan (no device, no launch).  Every case of
tests/gemm_cases.py gets the return code and kalle_gemm_last_plan word that the dispatcher gave before the planner was split
from the launches (tests/golden/gemm_plans.json: recorded from that dispatcher with every launch made a no-op), the case list
reaches every family and refusal, and the query rejects what the entry point rejects."""
import ctypes
import json
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")


@pytest.fixture(scope="module")
def table():
    t = {k: tuple(v) for k, v in json.load(open(GOLDEN)).items()}
    assert set(t) == {gc.key(c) for c in gc.CASES}, "every case has a row, keyed by gemm_cases.key, and no row is left over"
    return t


def query(c):
    """(return code, word; 0 where the call is refused) on a fresh thread: an empty cache of mixed split-K plans"""
    from kalle_audio_amd import ops
    shape, kw = gc.plan_kwargs(c)
    rc, word = gc.fresh_thread(ops.gemm_plan, *shape, **kw)
    return rc, word or 0


def test_every_case_gets_the_recorded_plan(table):
    bad = [(gc.key(c), table[gc.key(c)], got) for c in gc.CASES for got in [query(c)] if got != table[gc.key(c)]]
    assert not bad, (len(bad), bad[:10])


def test_case_list_reaches_every_family(table):
    keys = {gc.key(c) for c in gc.CASES}
    assert {gc.key(c) for c in gc.epilogue_cases()} <= keys
    for rows in (252, 504, 2016, 4032, 32256):              # the bench step at model width 1536, inner 6144 / FF-in 12288
        for n, k in ((1536, 1536), (4608, 1536), (12288, 1536), (1536, 6144)):
            assert {gc.key(gc.case(rows, n, k, f32=False)), gc.key(gc.case(rows, k, n, bkm=1)),
                    gc.key(gc.case(n, k, rows, akm=1, bkm=1))} <= keys, (rows, n, k)
        assert {gc.key(gc.glu1_case(rows, 6144, 1536)), gc.key(gc.glu2_case(rows, 6144, 1536))} <= keys
    ok = [(c, w) for c in gc.CASES for rc, w in [table[gc.key(c)]] if rc == 0]
    assert {w & 255 for _, w in ok} == {1, 2, 3, 4, 5}
    assert {rc for rc, _ in table.values()} == {0, -1, -3}
    assert any(w >> 24 & 1 for _, w in ok)
    assert all(w & 255 == 3 for _, w in ok if w & 255 != 5 and w >> 24 & 1)
    assert any(w & 255 == 3 and (w >> 8) & 0xFFFF > 1 and not w >> 24 & 1 for _, w in ok)
    five = [w for _, w in ok if w & 255 == 5]
    assert {((w >> 8) & 15, (w >> 12) & 15) for w in five} == {(1, 1), (2, 1), (2, 2)}
    assert {((w >> 8) & 15, (w >> 12) & 15) for w in five if w >> 16 > 1} == {(1, 1), (2, 1), (2, 2)}
    # both fused-SwiGLU modes on every family that takes them: forward on 3, 4 and 5, backward on 3 only
    assert {(w & 255, c["glu"]) for c, w in ok if c.get("glu")} == {(3, 1), (4, 1), (5, 1), (3, 2)}
    # a null, a short (under two slabs) and a misaligned workspace each change the outcome of the same call with the lent one
    changed = Counter()
    for c in gc.CASES:
        ws = c.get("ws")
        if ws is not None:
            kind = ws if isinstance(ws, str) else "short" if ws < 8 * c["M"] * c["N"] else "slabs"
            lent = {k: v for k, v in c.items() if k != "ws"}
            changed[kind] += table[gc.key(lent)] != table[gc.key(c)]
    assert changed["none"] and changed["short"] and changed["odd"] and changed["slabs"], changed


def test_replay_pair_starts_from_the_plans_it_names():
    """the GPU test launches the first shape and expects its mixed plan for the second one: their fresh plans must differ"""
    M, N, ka, plan_a, kb, plan_b = gc.REPLAY
    assert (ka + 63) // 64 // 16 == (kb + 63) // 64 // 16                       # one cache bucket
    assert query(gc.case(M, N, ka, akm=1, bkm=1)) == (0, plan_a) and query(gc.case(M, N, kb, akm=1, bkm=1)) == (0, plan_b)
    assert plan_a >> 24 & 1 and plan_a != plan_b


def test_query_is_pure_and_rejects_like_the_entry_point():
    from kalle_audio_amd import _lib, ops
    lib = _lib.load()
    out = ctypes.c_int(77)

    def rc(M=2560, N=3328, K=6144, plan=out, pos=(), ep_set=(), **kw):
        """the query's return code; pos: argument positions to overwrite, ep_set: epilogue fields to overwrite.  A call the
        query refuses is also made through the entry point, which must refuse it in the same way (it launches nothing)"""
        args, ep = ops._gemm_plan_args(M, N, K, **{**dict(a_kmajor=True, b_kmajor=True, f32=True), **kw})
        args = list(args)
        for i, v in dict(pos).items():
            args[i] = v
        for f, v in dict(ep_set).items():
            setattr(ep, f, v)
        r = lib.kalle_gemm_plan(*args, ctypes.byref(plan) if plan is not None else None)
        if r != 0 and plan is not None:
            assert lib.kalle_gemm_bf16(*args, None) == r
        return r
    assert rc() == 0 and out.value == gc.REPLAY[3]
    # positions in the argument list: 0 A, 1 lda, 3 B, 4 ldb, 6 C, 7 ldc, 8 c_dtype
    for bad in (dict(pos={0: None}), dict(pos={3: None}), dict(pos={6: None}), dict(pos={0: 24}), dict(pos={3: 8}), dict(pos={6: 4}),
                dict(pos={1: 2564}), dict(pos={4: 3332}), dict(pos={7: 3332}), dict(pos={8: 2}), dict(M=0), dict(N=-8), dict(K=0),
                dict(N=3332), dict(M=2564), dict(K=6148, a_kmajor=False), dict(K=6148, b_kmajor=False),
                dict(accumulate=True, f32=False, a_kmajor=False), dict(bias=True, ep_set=dict(bias=20)),
                dict(gate=True, ep_set=dict(gate=8)), dict(gate=True, ep_set=dict(ldg=3330)), dict(residual=True, ep_set=dict(residual=4)),
                dict(residual=True, ep_set=dict(ldr=3329)), dict(ep_set=dict(glu_mode=3)), dict(ep_set=dict(glu_mode=-1)),
                dict(ep_set=dict(glu_mode=1, glu_inner=1664)), dict(ep_set=dict(glu_mode=1, glu_aux=16))):
        out.value = 77
        assert rc(**bad) == -1, bad
        assert out.value == 77, bad
    for unsupported in (dict(a_kmajor=False, b_kmajor=False, f32=False, N=2 * 1664, glu_mode=1, glu_inner=1664, residual=True),
                        dict(a_kmajor=False, f32=False, N=1664, glu_mode=2, glu_inner=1664, bias=True),
                        dict(M=5000, a_kmajor=False, b_kmajor=False, f32=False, N=192, glu_mode=1, glu_inner=96)):
        out.value = 77
        assert rc(**unsupported) == -3, unsupported
        assert out.value == 77, unsupported
    assert rc(plan=None) == -1

    def twice():
        # the query leaves the cache alone: after it, a shape of the same bucket still gets its own fresh plan, not the first one's
        M, N, ka, plan_a, kb, plan_b = gc.REPLAY
        a, b = ops.gemm_plan(M, N, ka, a_kmajor=True, b_kmajor=True, f32=True), ops.gemm_plan(M, N, ka, a_kmajor=True, b_kmajor=True, f32=True)
        other = ops.gemm_plan(M, N, kb, a_kmajor=True, b_kmajor=True, f32=True)
        return a, b, other, lib.kalle_gemm_last_plan()
    a, b, other, last = gc.fresh_thread(twice)
    assert a == b == (0, gc.REPLAY[3]) and other == (0, gc.REPLAY[5])
    assert last == 0                                        # nothing was launched on that thread
