"""CPU: the planner of the attention entry points through its host queries kalle_attention_fwd_plan / _bwd_plan / _decode_plan /
_decode_rows_plan (no device, no launch).  Every case of tests/attn_cases.py gets the return code, plan word, launch count and
launch geometry that the entry points gave before the dispatch became plan_attention (tests/golden/attn_plans.json: recorded from
that code with the HIP runtime replaced by a recorder), the case list reaches every word the GPU tests ask for
and every refusal, every named predicate of csrc/attention.hip flips somewhere in it, and the queries are pure."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plans.json")
OK, ERR_ARG = 0, -1


@pytest.fixture(scope="module")
def table():
    t = json.load(open(GOLDEN))
    assert set(t["cases"]) == {ac.key(c) for c in ac.CASES}, "every case has a row, keyed by attn_cases.key, and no row is left over"
    assert len(ac.CASES) == len(t["cases"])
    return {k: t["rows"][i] for k, i in t["cases"].items()}


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def test_every_case_gets_the_recorded_row(table, lib):
    before = lib.kalle_attn_last_plan()
    bad = []
    for c in ac.CASES:
        rc, out = ac.query(lib, c)
        row = table[ac.key(c)]
        if ac.row_of(rc, out) != row or (rc == OK and any(out[2 + 5 * out[1]:])) or (rc != OK and out != [77] * ac.OUT_INTS):
            bad.append((ac.key(c), row, rc, out))
    assert not bad, (len(bad), bad[:10])
    assert lib.kalle_attn_last_plan() == before             # thousands of queries later
    assert len(ac.CASES) > 3000


def test_refused_cases_are_refused_by_the_entry_points_and_a_null_plan_by_the_queries(table, lib):
    """a refused call launches nothing, so the entry point itself can be asked with placeholder pointers and no device; so can
    the rows call whose rows are all inactive (KALLE_OK, nothing launched)"""
    n = 0
    for c in ac.CASES:
        row = table[ac.key(c)]
        if row[2] != 0:
            continue
        assert row[1] == 0, (ac.key(c), "no launch, but a plan word")
        assert ac.entry_point(lib, c)(*ac.args(c), None) == row[0], ac.key(c)
        assert lib.kalle_attn_last_plan() == 0, ac.key(c)
        n += 1
    assert n > 500
    for c in [c for _n, c, _kw, a, _b in ac.FLIPS if a][:8]:
        assert getattr(lib, ac.FUNCS[c["entry"]] + "_plan")(*ac.args(c), None) == ERR_ARG
    # the head-dim-64 forwarders of the ABI refuse what the _hd forms refuse
    c = ac.C("fwd", H=3, Hkv=2)
    assert lib.kalle_attention_fwd(*ac.args(c)[:-1], None) == ERR_ARG
    assert lib.kalle_attention_bwd(*ac.args(dict(c, entry="bwd"))[:-1], None) == ERR_ARG


def test_case_list_reaches_every_word_and_refusal(table):
    import llama_hd128_cases as lc
    import test_attention_gpu as ta
    import test_decode_gpu as td
    for k, want in ac.EXPECT.items():                       # the literal words of the GPU case lists
        assert table[k][:2] == [OK, want], (k, table[k], hex(want))
    assert len(ac.EXPECT) > 200
    words = {r[1] for r in table.values() if r[0] == OK}
    # test_attention_gpu.test_every_family_and_head_dim_was_seen
    want = {ta.tiled(d, f) for d in (32, 64, 128) for f in (False, True)} | {ta.decode(r) for r in (0, 32, 64)} | \
           {ta.two_pass(d) for d in (32, 64, 128)} | {ta.FUSED, ta.FUSED_GQA}
    # test_llama_hd128_gpu.test_every_plan_and_edge_was_seen, test_decode_gpu, test_decode_rows_gpu
    want |= {lc.T128, lc.TP128, lc.decode128(), td.DECODE_PLAN} | {lc.decode64(r) for r in (0, 32, 64)}
    want |= {ac.rows_word(64, 0), ac.rows_word(64, 64), ac.rows_word(128, 128)}
    assert words == want | {0}, ([hex(w) for w in sorted(want - words)], [hex(w) for w in sorted(words - want - {0})])
    assert {r[0] for r in table.values()} == {OK, ERR_ARG}              # every return code that occurs without a device
    refused = {c["entry"] for c in ac.CASES if table[ac.key(c)][0] == ERR_ARG}
    assert refused == set(ac.ENTRIES)
    assert {r[2] for r in table.values()} == {0, 1, 2}
    assert any(r[:3] == [OK, 0, 0] for r in table.values())             # every row inactive
    # a NULL in each pointer argument, for each entry
    for e in ac.ENTRIES:
        assert {c["null"] for c in ac.CASES if c["entry"] == e and c["null"]} == set(ac.POINTERS[e]), e


@pytest.mark.parametrize("i", range(len(ac.FLIPS)), ids=lambda i: f"{ac.FLIPS[i][0]}-{i}")
def test_each_predicate_flips(table, i):
    name, c, kw, before, after = ac.FLIPS[i]
    assert len(kw) == 1 and before != after
    d = ac.C(c["entry"], **{k: v for k, v in dict(c, **kw).items() if k in ac.DEFAULT})
    got = []
    for x, want in ((c, before), (d, after)):
        rc, word = table[ac.key(x)][:2]
        got.append(word & (15 | 1 << 16))
        assert (rc, word & (15 | 1 << 16)) == (OK if want else ERR_ARG, want), (name, ac.key(x), rc, hex(word))
    assert got[0] != got[1]


def test_wrapper(lib):
    from kalle_audio_amd import ops
    rc, p = ops.attention_plan("bwd", B=2, H=4, Hkv=1, Nq=300, Nk=330, dh=128, rot=64, causal=True)
    assert rc == OK and p == dict(word=3 | 16 | 128 << 8, family=3, launches=[dict(grid=(3, 4, 2), block=512, lds=74752),
                                                                           dict(grid=(3, 1, 2), block=512, lds=74752)])
    rc, p = ops.attention_plan("fwd", B=2, H=2, Hkv=2, Nq=1, Nk=130, rot=32)
    assert rc == OK and p == dict(word=2 | 64 << 8 | 32 << 17, family=2, launches=[dict(grid=(2, 2, 1), block=256, lds=520)])
    assert ops.attention_plan("decode", B=1, H=24, Hkv=8, Nk=71, dh=128, rot=128)[1]["family"] == 6
    rc, p = ops.attention_plan("rows", nk=(0, -1), H=4, Hkv=2, rot=64)
    assert rc == OK and p == dict(word=0, family=0, launches=[])
    assert ops.attention_plan("rows", nk=(3, 0, 15361), H=4, Hkv=2, rot=64) == (ERR_ARG, None)
    assert ops.attention_plan("fwd", B=2, H=3, Hkv=2, Nq=16, Nk=16) == (ERR_ARG, None)
