"""CPU: the planners of the VAE conv entry points through their host queries kalle_conv_plan / kalle_conv_transpose_plan /
kalle_conv_wgrad_plan (no device, no launch).  Every case of tests/conv_cases.py gets the entry point, return code, plan word and
padded-copy geometry that conv_ops / conv_train reached before the family rule moved into the library
(tests/golden/conv_plans.json, recorded from that code with every launch made a no-op), the case list reaches every family,
tile form and refusal, and the queries are pure."""
import ctypes
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc  # noqa: E402
from conv_cases import BF16, cf, fb, tv2, v2, wg_lane, wg_lds  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")


@pytest.fixture(scope="module")
def table():
    t = json.load(open(GOLDEN))
    assert set(t) == {cc.key(c) for c in cc.PLAN_CASES}, "every case has a row, keyed by conv_cases.key, and no row is left over"
    return t


def test_every_case_gets_the_recorded_row(table):
    from kalle_audio_amd import _lib
    lib = _lib.load()
    before = lib.kalle_conv_last_plan()
    # (a refused row names the function that refused, which a query cannot: code and word there; the test below calls that function)
    bad = [(cc.key(c), row, got) for c in cc.PLAN_CASES for row, got in [(table[cc.key(c)], cc.query(c))]
           if (got != row if row[1] == 0 else got[1:] != row[1:])]
    assert not bad, (len(bad), bad[:10])
    assert lib.kalle_conv_last_plan() == before             # thousands of queries later


def test_case_list_reaches_every_family_and_form(table):
    keys = set(table)
    for c in cc.CONV_CASES + cc.CONVT_CASES + cc.CFIRST_CASES + cc.CFIRST_T_CASES + cc.EDGE_CASES + cc.CFIRST_EDGES:
        row = table[cc.key(cc.from_test(c))]
        assert c in cc.EDGE_CASES or cc.key(cc.from_test(c, 0)) in keys           # (and under the automatic rule, but for the edge list)
        if c["ws"]:     # (lent a workspace, as conv_ops does): the word and return code the GPU test expects of the entry point
            assert (row[1], row[2]) == (c["rc"], c["plan"]) and (row[1] != 0 or row[0] == c["entry"]), (c, row)
    for c in cc.WGRAD_CASES:
        assert table[cc.key(cc.from_wgrad(c))][1:3] == [0, c["plan"]], c
    for B in (1, 4, 8, 16):
        assert {cc.key(c) for c in cc.oobleck(B, 440320) + cc.oobleck(B, 128 * 2048) + cc.flows_vae(B, 24000)} <= keys
    ok = [r for r in table.values() if r[1] == 0]
    words = {r[2] for r in ok}
    assert {w & 15 for w in words} == set(range(1, 10))
    assert {r[0] for r in ok} == set(cc.ENTRIES) and all(cc.FAMILY_ENTRY[r[2] & 15] == r[0] for r in ok)
    # every word test_conv_gpu.py's test_every_plan_family_and_tile_form_was_seen asks for
    want = {v2(2, 2, 1), v2(8, 8, 4), v2(8, 4, 4), v2(8, 2, 4), v2(16, 8, 4), v2(16, 8, 4, ci=16), v2(16, 4, 8, nw=8, ci=32),
            v2(16, 8, 8, nw=8), v2(8, 8, 4, stride=2), v2(8, 4, 4, stride=4), v2(16, 4, 4, stride=4), v2(8, 2, 4, stride=8),
            v2(2, 2, 1, dt=BF16), v2(8, 2, 4, dt=BF16), fb(), fb(cc.F32, BF16), fb(BF16, cc.F32),
            tv2(2, 2, 1), tv2(8, 8, 4), tv2(8, 4, 4), tv2(8, 2, 4), tv2(16, 8, 4), tv2(8, 2, 4, dt=BF16), fb(cc.F32, BF16, 3), fb(BF16, cc.F32, 3),
            cf(1), cf(2), cf(4), cf(4, 4), cf(4, 16), cf(4, 1, 6), cf(4, 16, 6), cf(1, 1, 7), cf(2, 1, 7), cf(4, 1, 7),
            wg_lds(16, 1), wg_lds(16, 4), wg_lds(16, 7), wg_lds(16, 8), wg_lds(8, 16), wg_lane(4, 8, 4), wg_lane(4, 4, 8), wg_lane(2, 4, 16)}
    assert want <= words, [hex(w) for w in sorted(want - words)]
    for fam in (5, 6, 7):
        assert {w >> 8 & 15 for w in words if w & 15 == fam} == {1, 2, 4}, fam
    assert {w >> 12 & 31 for w in words if w & 15 == 5} == {1, 2, 4, 8, 16} and any(w >> 12 & 31 > 1 for w in words if w & 15 == 6)
    assert all((r[6] > 0) == ((r[2] >> 12 & 31) > 1) for r in ok if r[0] == "cfirst")
    assert {r[1] for r in table.values()} == {0, -1, -3}
    assert {cc.full(c)["prefer"] for c in cc.PLAN_CASES if c["kind"] != "wgrad"} == {0, 1, 2}
    # `prefer` decides: some shape gets three different answers... at least auto differs from each forced side somewhere
    by = {}
    for c in cc.PLAN_CASES:
        if c["kind"] != "wgrad":
            by.setdefault(cc.key({k: v for k, v in c.items() if k != "prefer"}), {})[cc.full(c)["prefer"]] = table[cc.key(c)][0]
    trip = [v for v in by.values() if len(v) == 3]
    assert any(v[0] == v[1] != v[2] for v in trip) and any(v[0] == v[2] != v[1] for v in trip)


def test_refused_queries_match_the_entry_points_and_write_nothing(table):
    """every refused case: the query refuses with the recorded code and leaves `out` as it was, and so does the function that
    the table names as the one that refused (an entry point, or kalle_conv_pad_act ahead of a channels-per-lane one), called
    with placeholder tensors and the padded-copy geometry the header describes: a refused call launches nothing"""
    from kalle_audio_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)
    called = set()
    n = 0
    for c in cc.PLAN_CASES:
        who, code, _ = table[cc.key(c)][:3]
        if code == 0:
            continue
        f = cc.full(c)
        out = (ctypes.c_int32 * 6)(*[77] * 6)
        ab = None if f["noab"] else 16
        ia = _lib.Act(f["act"], 1, ab, ab, 0.2)
        if f["kind"] == "wgrad":
            args = (f["B"], f["CU"], f["CV"], f["MU"], f["LV"], f["K"], f["stride"], f["pl"], f["dil"], f["act_on"], ctypes.addressof(ia))
            assert who == "wgrad" and lib.kalle_conv_wgrad_plan(*args, out) == code and lib.kalle_conv_wgrad(P, P, P, *args, None) == code, c
        else:
            ep = _lib.ConvEpilogue(16 if f["res"] else None, f["scale"], int(f["acc"]), int(f["tanh"]), _lib.Act(f["post"], 1, ab, ab, 0.1),
                                   16 if f["raw"] else None)
            B, Cin, Lin, Cout, Lout, K, s, pl, dil = (f[k] for k in ("B", "Cin", "Lin", "Cout", "Lout", "K", "stride", "pl", "dil"))
            shape = (B, Cin, Lin, Cout, Lout, K, s, pl) + ((dil,) if f["kind"] == "conv" else ())
            q = lib.kalle_conv_plan if f["kind"] == "conv" else lib.kalle_conv_transpose_plan
            assert q(f["xdt"], f["ydt"], *shape, ctypes.addressof(ia), ctypes.addressof(ep), f["prefer"], out) == code, c
            ea, ia_ = ctypes.addressof(ep), ctypes.addressof(ia)
            if who in ("pad_act", "cfirst", "cfirstT"):          # (the pad-length helpers check nothing: only where the dispatch got that far)
                if f["kind"] == "conv":
                    Lp, lead, phases = lib.kalle_conv_pad_len(Lout, K, s, pl, dil), pl if s == 1 else (pl + s - 1) // s * s, s
                else:
                    Lp, lead, phases = lib.kalle_convT_pad_len(Lout, K, s, pl), (K + s - 1) // s - 1, 1
            if who == "conv":
                rc = lib.kalle_conv1d_fwd(P, f["xdt"], P, P, P, f["ydt"], *shape, ia_, ea, None)
            elif who == "convT":
                rc = lib.kalle_conv_transpose1d_fwd(P, f["xdt"], P, P, P, f["ydt"], *shape, ia_, ea, None)
            elif who == "pad_act":
                rc = lib.kalle_conv_pad_act(P, P, B, Cin, Lin, Lp, lead, ia_, phases, None)
            elif who == "cfirst":
                rc = lib.kalle_conv1d_cfirst_fwd(P, P, P, P, B, Cin, Lp, Cout, Lout, K, s, pl, dil, ea, P, None)
            else:
                assert who == "cfirstT", who
                rc = lib.kalle_conv_transpose1d_cfirst_fwd(P, P, P, P, B, Cin, Lp, Cout, Lout, K, s, pl, ea, None)
            assert rc == code, (c, who, rc)
        called.add(who)
        assert list(out) == [77] * 6, c
        assert lib.kalle_conv_last_plan() == 0
        n += 1
    assert called == {"conv", "convT", "cfirst", "cfirstT", "pad_act", "wgrad"}, called
    assert n > 100
    out = (ctypes.c_int32 * 6)(*[77] * 6)
    for prefer in (-1, 3):
        assert lib.kalle_conv_plan(1, 1, 3, 9, 200, 20, 200, 3, 1, 1, 1, None, None, prefer, out) == -1
        assert lib.kalle_conv_transpose_plan(1, 1, 2, 8, 50, 20, 100, 4, 2, 1, None, None, prefer, out) == -1
    assert lib.kalle_conv_plan(1, 1, 3, 9, 200, 20, 200, 3, 1, 1, 1, None, None, 0, None) == -1
    assert lib.kalle_conv_transpose_plan(1, 1, 2, 8, 50, 20, 100, 4, 2, 1, None, None, 0, None) == -1
    assert lib.kalle_conv_wgrad_plan(1, 8, 16, 64, 64, 7, 1, 3, 1, 0, None, None) == -1
    assert list(out) == [77] * 6
    assert lib.kalle_conv_plan(1, 1, 3, 9, 200, 20, 200, 3, 1, 1, 1, None, None, 0, out) == 0 and list(out) == [2, v2(8, 2, 4), 0, 0, 0, 0]


def test_wrappers_follow_the_environment(monkeypatch):
    from kalle_audio_amd import conv_ops, conv_train
    shape = (1, 8, 32, 256, 32, 3)
    monkeypatch.delenv("KALLE_CONV_CFIRST", raising=False)
    assert conv_ops.conv_plan(*shape, padding=1)[1]["family"] == 5
    monkeypatch.setenv("KALLE_CONV_CFIRST", "0")
    assert conv_ops.conv_plan(*shape, padding=1)[1]["family"] == 2 and conv_ops.conv_plan(*shape, padding=1, prefer=1)[1]["family"] == 5
    monkeypatch.setenv("KALLE_CONV_CFIRST", "1")
    assert conv_ops.conv_plan(3, 9, 200, 20, 200, 3, padding=1)[1] == dict(family=5, word=cf(4), Lp=210, lead=1, phases=1, ws_floats=0)
    assert conv_ops.conv_transpose_plan(1, 8, 16, 256, 32, 4, stride=2, padding=1)[1]["family"] == 7
    rc, r = conv_train.conv_wgrad_plan(1, 8, 16, 64, 64, K=7, stride=1, padding=3, dilation=1, act_on=0)
    assert rc == 0 and r["word"] == wg_lds(16, 7) and r["grid"][1:] == (1, 1)
