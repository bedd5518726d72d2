"""CPU: the host side of `infer_batch(refill=True)` without a device - the row schedule (generation.RowSchedule, driven by the real
generation loop on fakes, against the closed form refill_steps), the numpy reference of kalle_kv_append_varlen that
tests/test_kv_append_gpu.py holds the kernel to, every refusal of the real entry point (they return before any launch), and the
argument checks of LlamaModel.prefill_rows."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refill_cases as rc  # noqa: E402
import test_generation_loop_cpu as loop  # noqa: E402

ERR_ARG = -1


# ------------------------------------------------------------------------------------------------ the schedule
def drive(frames, R, stop_lag=0, log=None):
    """the schedule the real loop (generation.run_frames on the fakes of tests/test_generation_loop_cpu.py) leaves for utterances
    that run frames[u] frames each.  log: receives (step, admitted pairs, live rows) per step."""
    return loop.drive(frames, R, stop_lag, log)[0]


LISTS = loop.LISTS
seeded_caps = loop.seeded_caps


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("i", range(len(LISTS)))
def test_every_prompt_once_in_order_in_ascending_rows(i, lag):
    frames, R = LISTS[i]
    log = []
    sched = drive(frames, R, lag, log)
    order, seen = [], set()
    for s, pairs, live in log:
        assert len(live) <= R and len({r for r, _, _ in live}) == len(live)            # never more than R, one utterance a row
        assert [r for _, r in pairs] == sorted(r for _, r in pairs)                      # free rows in ascending index
        assert [u for u, _ in pairs] == list(range(len(order), len(order) + len(pairs)))   # prompts in list order
        for u, r in pairs:
            assert (r, u, 0) in live and u not in seen
            seen.add(u)
            order.append(u)
    assert order == list(range(len(frames)))                                             # each exactly once
    assert [t[0] for t in sched.trace] == list(range(len(frames)))
    assert [t[3] for t in sched.trace] == list(frames)
    assert len({r for _, r, _, _ in sched.trace}) <= min(R, len(frames))                 # a list shorter than R leaves rows empty


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("i", range(len(LISTS)))
def test_class_driven_with_stops_equals_the_closed_form(i, lag):
    from kalle_audio_amd.model_sigmaVAE import refill_steps
    frames, R = LISTS[i]
    sched = drive(frames, R, lag)
    total, first = refill_steps(frames, R, stop_lag=lag)
    assert total == sched.steps
    assert first == [(r, t) for _, r, t, _ in sched.trace]
    rc.occupants(frames, first, R)                                                       # no two utterances share a (step, row)


def test_the_five_caps_on_two_rows():
    from kalle_audio_amd.model_sigmaVAE import grouped_steps, refill_steps
    assert refill_steps(rc.CAPS, rc.ROWS) == (14, [(0, 0), (1, 0), (1, 3), (0, 6), (0, 9)])
    assert refill_steps(rc.CAPS, rc.ROWS, stop_lag=1) == (16, [(0, 0), (1, 0), (1, 4), (0, 7), (0, 11)])
    assert grouped_steps(rc.CAPS, rc.ROWS) == 19
    assert drive(rc.CAPS, rc.ROWS).trace == [(0, 0, 0, 6), (1, 1, 0, 3), (2, 1, 3, 8), (3, 0, 6, 3), (4, 0, 9, 5)]
    # the refilled prompt that is shorter than what its row held before (tests/test_llasa_refill_gpu.py relies on it)
    assert rc.PS[3] < rc.PS[0] + rc.CAPS[0] - 1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_refill_needs_fewer_steps_than_groups_on_the_seeded_list(seed):
    from kalle_audio_amd.model_sigmaVAE import grouped_steps, refill_steps
    caps = seeded_caps(seed)
    steps, grouped = refill_steps(caps, 16)[0], grouped_steps(caps, 16)
    print(f"REFILL seed {seed}: {steps} steps against {grouped} grouped, x {grouped / steps:.3f}")
    assert steps < grouped
    assert steps >= -(-sum(caps) // 16)                      # no schedule beats full rows
    assert refill_steps(caps, 64)[0] == max(caps) == grouped_steps(caps, 64)       # no list longer than R: nothing to refill


def test_schedule_arguments():
    from kalle_audio_amd.model_sigmaVAE import RowSchedule
    with pytest.raises(ValueError):
        RowSchedule(3, 0)
    s = RowSchedule(0, 4)
    assert s.done and s.admit(0) == [] and s.trace == [] and s.steps == 0


# ------------------------------------------------------------------------------------------------ kalle_kv_append_varlen
def _src(c, seed=5):
    return np.random.default_rng(seed).integers(0, 0x7f80, size=(c["total"], c["ld"]), dtype=np.uint16)


@pytest.mark.parametrize("c", rc.KV_CASES, ids=lambda c: c["id"])
def test_numpy_reference_of_kv_append(c):
    """against torch slicing, and nothing written outside the named positions"""
    src = _src(c)
    cache = np.full((c["R"], c["cache_rows"], c["kvw"]), 0xffff, dtype=np.uint16)
    got = rc.kv_append_ref(src, c["src_off"], cache, c["row0"], c["lens"], c["dst"], c["t0"])
    want = torch.from_numpy(cache.astype(np.int32))
    s = torch.from_numpy(src.astype(np.int32))
    named = torch.zeros(want.shape[:2], dtype=torch.bool)
    for r0, n, d, t in zip(c["row0"], c["lens"], c["dst"], c["t0"]):
        want[d, t:t + n] = s[r0:r0 + n, c["src_off"]:c["src_off"] + c["kvw"]]
        named[d, t:t + n] = True
    assert np.array_equal(got.astype(np.int32), want.numpy())
    assert named.sum().item() == sum(c["lens"]) and (got[~named.numpy()] == 0xffff).all() and (got[named.numpy()] < 0x7f80).all()
    assert (cache == 0xffff).all()                           # the reference leaves its input alone


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def kv_call(lib, c, **kw):
    """kalle_kv_append_varlen for case c with overrides kw; placeholder pointers (the refusals come before any launch)"""
    a = dict(c, src=16, cache=16, nseq=len(kw.get("lens", c["lens"])), stride=c["cache_rows"] * c["kvw"])
    a.update(kw)
    arrays = [_i32(a[k]) for k in ("row0", "lens", "dst", "t0")]
    ptrs = [None if k in a and a[k] is None else ctypes.cast(arr, ctypes.c_void_p)
            for k, arr in zip(("row0_ptr", "len_ptr", "dst_ptr", "t0_ptr"), arrays)]
    return lib.kalle_kv_append_varlen(a["src"], a["ld"], a["src_off"], a["cache"], a["stride"], a["kvw"], a["nseq"], *ptrs,
                                      a["total"], a["R"], a["cache_rows"], None)


@pytest.mark.parametrize("name", list(rc.KV_REFUSALS))
def test_kv_append_refusals_without_a_device(lib, name):
    assert kv_call(lib, rc.KV_BASE, **rc.KV_REFUSALS[name]) == ERR_ARG, name


def test_kv_append_refusal_list_is_the_headers():
    """one refusal at least for every item of the header's list"""
    names = " ".join(rc.KV_REFUSALS)
    for item in ("NULL", "nseq 0", "nseq 17", "len 0", "t0 negative", "cache_rows", "dst_row negative", "dst_row = R", "twice",
                 "total_rows", "overlapping", "unordered", "kvw % 8", "ld_src % 8", "src_off % 8", "cache_row_stride % 8"):
        assert item in names, item


# ------------------------------------------------------------------------------------------------ prefill_rows
CFG = dict(vocab_size=32, hidden_size=128, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
           head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0)


def test_prefill_rows_argument_checks():
    """on the host, before any tensor is looked at: duplicate rows, a row outside the cache, a row not at length 0, a cache too
    short, a count mismatch; valid arguments get as far as the device check (CPU tensors: RuntimeError, no fallback)"""
    from kalle_audio_amd.model_sigmaVAE import LlamaModel
    model = LlamaModel(CFG)
    cache = model.init_cache_batch(4, 12, "cpu")
    cache["len"][3] = 5
    e = lambda n: torch.zeros(1, n, 128)
    with pytest.raises(ValueError, match="distinct"):
        model.prefill_rows([e(3), e(4)], cache, [1, 1])
    with pytest.raises(ValueError, match="distinct"):
        model.prefill_rows([e(3), e(4)], cache, [1, 4])
    with pytest.raises(ValueError, match="length 0"):
        model.prefill_rows([e(3), e(4)], cache, [3, 0])
    with pytest.raises(ValueError, match="too short"):
        model.prefill_rows([e(3), e(13)], cache, [0, 1])
    with pytest.raises(ValueError, match="one cache row per prompt"):
        model.prefill_rows([e(3)], cache, [0, 1])
    with pytest.raises(ValueError, match="one cache row per prompt"):
        model.prefill_rows([], cache, [])
    assert cache["len"] == [0, 0, 0, 5]
    with pytest.raises(RuntimeError, match="GPU"):
        model.prefill_rows([e(3), e(12)], cache, [2, 0])
    assert cache["len"] == [0, 0, 0, 5]


def test_frame_caps_and_empty_list():
    from kalle_audio_amd.generation import _frame_caps, generate_batch
    assert _frame_caps(7, 3) is None and _frame_caps([6, 3, 8], 3) == [6, 3, 8] and _frame_caps((2, 2), 2) == [2, 2]
    with pytest.raises(ValueError):
        _frame_caps([6, 3], 3)
    with pytest.raises(ValueError):
        _frame_caps([6, 0, 3], 3)
    assert generate_batch(None, [], -1.0, 5, False, None, 0, 8, refill=True) == []
