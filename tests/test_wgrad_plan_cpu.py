"""CPU: the planner of kalle_gemm_wgrad_group through its host query kalle_gemm_wgrad_group_plan (no device, no launch): the
case list of tests/wgrad_cases.py gets the plans written there and reaches every region, the planner's own rules hold over a
sweep of shapes, and the query rejects what the entry point rejects."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_cases as wc  # noqa: E402


def query(problems, overwrite=False):
    """on a fresh thread: an empty plan cache"""
    from kalle_audio_amd import ops
    p = wc.fresh_thread(ops.wgrad_group_plan, problems, overwrite)
    return p


def triple(p):
    return p["tiles"], p["whole"], p["slices"]


@pytest.mark.parametrize("name", list(wc.CASES))
@pytest.mark.parametrize("overwrite", [False, True])
def test_case_list_gets_the_plans_it_names(name, overwrite):
    problems, plan = wc.CASES[name]
    p = query(problems, overwrite)
    assert triple(p) == plan, p
    assert p["cleared"] == int(overwrite and plan[2] > 0) and p["cached"] == 0, p


@pytest.mark.parametrize("name", list(wc.REPLAY))
def test_replay_cases_start_from_the_plan_they_name(name):
    """shape A's fresh plan is the one the replay will hand to B; B planned afresh differs from it in every case but the one
    where the guard (fewer K-tiles than slices) decides, so the GPU test can tell a replayed plan from a fresh one"""
    shapes, ta, tb, plan_a, plan_b = wc.REPLAY[name]
    assert ta // 1024 == tb // 1024                       # one cache bucket
    assert triple(query([(ta, n, k) for n, k in shapes])) == plan_a
    fresh_b = triple(query([(tb, n, k) for n, k in shapes]))
    if name == "fewer-ktiles-than-slices":
        assert wc.ktiles(tb) < plan_a[2] and fresh_b == plan_b
    else:
        assert fresh_b != plan_b and plan_b == plan_a, fresh_b


def test_case_list_reaches_every_region():
    seen = set()
    for ow in (False, True):
        for problems, plan in wc.CASES.values():
            seen |= wc.regions(problems, plan, ow)
        for shapes, ta, tb, plan_a, plan_b in wc.REPLAY.values():
            seen |= wc.regions([(tb, n, k) for n, k in shapes], plan_b, ow)
    assert seen == set(wc.REGIONS), set(wc.REGIONS) ^ seen
    # cache keys: no two cases share one (the GPU file runs every case on a thread of its own, so this is belt and braces)
    keys = [tuple((n, k, t // 1024) for t, n, k in pr) for pr, _ in wc.CASES.values()]
    assert len(set(keys)) == len(keys)


def test_the_older_test_comment_was_wrong():
    """tests/test_round2_gpu.py used to call 512 tokens of (4096, 4096), (512, 256), (264, 136) "256 whole tiles + a sliced
    tail": 8 K-tiles are never sliced"""
    assert triple(query([(512, 4096, 4096), (512, 512, 256), (512, 264, 136)])) == (260, 260, 0)


@pytest.mark.parametrize("n,k", [(8, 256 * 300), (264, 136), (1536, 1536), (2056, 8456)])
def test_planner_rules_over_token_counts(n, k):
    """whole is all tiles or a multiple of 256; slices in 2 .. 12 with at least 8 K-tiles per slice before rounding; never a
    slice under 16 K-tiles (968 tokens); a fresh plan has no empty slice"""
    tiles = wc.tiles_of(n, k)
    for tokens in list(range(8, 1024, 56)) + list(range(1024, 16384, 328)):
        p = query([(tokens, n, k)])
        assert p["tiles"] == tiles
        if p["slices"] == 0:
            assert p["whole"] == tiles
            continue
        nk = wc.ktiles(tokens)
        assert nk >= 16 and p["whole"] % 256 == 0 and p["whole"] < tiles, (tokens, p)
        assert 2 <= p["slices"] <= 12 and nk // p["slices"] >= 8, (tokens, p)
        assert "empty-trailing-slice" not in wc.regions([(tokens, n, k)], triple(p), False)


def test_query_is_pure_and_rejects_like_the_entry_point():
    from kalle_audio_amd import _lib, ops
    lib = _lib.load()
    out = (ctypes.c_int * 5)(*[77] * 5)

    def rc(problems, nprob=None, **field):
        arr = ops._wgrad_problems(problems)
        for f, v in field.items():
            setattr(arr[0], f, v)
        return lib.kalle_gemm_wgrad_group_plan(ctypes.cast(arr, ctypes.c_void_p), len(problems) if nprob is None else nprob, 0,
                                               ctypes.cast(out, ctypes.c_void_p))
    ok = [(1024, 264, 136)]
    assert rc(ok, nprob=0) == -1 and rc(ok * 9) == -1 and rc(ok * 8) == 0
    for field in (dict(N=260), dict(K=132), dict(lddy=268), dict(ldx=140), dict(lddw=138), dict(dy=24), dict(x=8), dict(dw=4),
                  dict(dw=None), dict(tokens=0)):
        out[:] = [77] * 5
        assert rc(ok, **field) == -1, field
        assert list(out) == [77] * 5
    assert rc(ok, tokens=1020) == -3
    assert lib.kalle_gemm_wgrad_group_plan(None, 1, 0, ctypes.cast(out, ctypes.c_void_p)) == -1
    assert lib.kalle_gemm_wgrad_group_plan(ctypes.cast(ops._wgrad_problems(ok), ctypes.c_void_p), 1, 0, None) == -1

    def twice():
        # the query leaves the cache alone (the second answer is not "cached") and nothing was launched on this thread
        a, b = ops.wgrad_group_plan(ok), ops.wgrad_group_plan(ok)
        return a, b, ops.wgrad_group_last_plan()
    a, b, last = wc.fresh_thread(twice)
    assert a == b and a["cached"] == 0 and triple(a) == (2, 0, 2)
    assert set(last.values()) == {0}
