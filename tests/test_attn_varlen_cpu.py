"""CPU: the varlen attention entry points without a device - the planner through its host queries
kalle_attention_fwd_varlen_plan / _bwd_varlen_plan (word, launches, grids, block, LDS; one refusal per item of the header's
list), the fairness of the wrong references tests/test_attn_varlen_gpu.py uses (each moves some element of the GPU file's own
inputs by more than twice its allowance, from the fp64 references alone, as tests/test_attention_refs_cpu.py does for the dense
kernels), and the mask check behind Llasa.pack_sequences()."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import attn_varlen_cases as vc  # noqa: E402

OK, ERR_ARG = 0, -1
SENTINEL = 77


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def query(lib, entry, c, **kw):
    """(rc, the 12 plan ints) of the host query for case c with overrides kw (placeholder pointers: only tested for null)"""
    a = dict(c, q=16, k=16, v=16, out=16, lse=16, cos=16, sin=16, dout=16, delta=16, dq=16, dk=16, dv=16, row0_dev=16, len_dev=16,
             q_off=0, ld=(c["H"] + 2 * c["Hkv"]) * c["dh"], ldo=c["H"] * c["dh"], nseq=len(c["lens"]), max_len=max(c["lens"]),
             row0_host=True, len_host=True)
    a.update(kw)
    if not a["rot"] and "cos" not in kw:
        a["cos"] = a["sin"] = None
    r0, ln = _i32(a["row0"]), _i32(a["lens"])
    D, kvw = a["H"] * a["dh"], a["Hkv"] * a["dh"]
    head = (a["q"], a["ld"], a["q_off"], a["k"], a["ld"], D, a["v"], a["ld"], D + kvw)
    seqs = (a["nseq"], ctypes.cast(r0, ctypes.c_void_p) if a["row0_host"] else None, ctypes.cast(ln, ctypes.c_void_p) if a["len_host"] else None,
            a["row0_dev"], a["len_dev"], a["total"], a["max_len"], a["H"], a["Hkv"], a["dh"])
    plan = (ctypes.c_int32 * 12)(*[SENTINEL] * 12)
    if entry == "fwd":
        rc = lib.kalle_attention_fwd_varlen_plan(*head, a["out"], a["ldo"], a["lse"], a["cos"], a["sin"], a["rot"], *seqs, plan)
    else:
        rc = lib.kalle_attention_bwd_varlen_plan(*head, a["out"], a["dout"], a["ldo"], a["lse"], a["delta"], a["dq"], a["dk"], a["dv"],
                                                 a["cos"], a["sin"], a["rot"], *seqs, plan)
    return rc, list(plan)


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=lambda i: vc.case_id(vc.CASES[i]))
def test_queries_name_word_launches_and_grids(lib, i):
    c = vc.CASES[i]
    before = lib.kalle_attn_last_plan()
    nb, H, Hkv, S, dh = (max(c["lens"]) + 127) // 128, c["H"], c["Hkv"], len(c["lens"]), c["dh"]
    dense = (16, H * dh, 0, 16, 2 * Hkv * dh, 0, 16, 2 * Hkv * dh, Hkv * dh)
    tab = 16 if c["rot"] else None
    df, db = (ctypes.c_int32 * 12)(), (ctypes.c_int32 * 12)()
    N = max(c["lens"])
    assert lib.kalle_attention_fwd_plan(*dense, 16, H * dh, 16, tab, tab, c["rot"], None, 1, 1, H, Hkv, N, N, dh, df) == OK
    assert lib.kalle_attention_bwd_plan(*dense, 16, 16, H * dh, 16, 16, 16, 16, 16, tab, tab, c["rot"], None, 1, 1, H, Hkv, N, N, dh, db) == OK
    rc, p = query(lib, "fwd", c)
    assert (rc, p[:2]) == (OK, [vc.fwd_word(c), 1]), (rc, p)
    assert p[2:5] == [nb, H, S] and p[5:7] == [512, df[6]] == list(df[5:7]) and not any(p[7:]), (p, list(df))
    rc, p = query(lib, "bwd", c)
    assert (rc, p[:2]) == (OK, [vc.bwd_word(c), 2]), (rc, p)
    assert p[2:5] == [nb, H, S] and p[7:10] == [nb, Hkv, S], p
    assert p[5:7] == list(db[5:7]) == p[10:12] == list(db[10:12]) and p[5] == 512, (p, list(db))
    assert lib.kalle_attn_last_plan() == before                 # a query is pure
    # a longer max_len only widens the grid
    rc, p = query(lib, "fwd", c, max_len=N + 300)
    assert rc == OK and p[2] == (N + 300 + 127) // 128


def test_wrapper(lib):
    from kalle_audio_amd import ops
    s = ops.Packed([8, 200, 464], [129, 257, 1], 472, None)
    assert s.has_gaps and s.max_len == 257
    rc, p = ops.attention_plan("fwd_varlen", H=4, Hkv=2, rot=64, seqs=s)
    assert rc == OK and p["word"] == 8 | 64 << 8 and p["family"] == 8 and [l["grid"] for l in p["launches"]] == [(3, 4, 3)]
    rc, p = ops.attention_plan("bwd_varlen", H=4, Hkv=2, dh=128, rot=128, seqs=s)
    assert rc == OK and p["word"] == 9 | 16 | 128 << 8 and [l["grid"] for l in p["launches"]] == [(3, 4, 3), (3, 2, 3)]
    b = ops.Packed.back_to_back([3, 4], None, granule=8)
    assert (b.row0, b.total_rows, b.has_gaps) == ([0, 3], 8, True)
    assert ops.attention_plan("fwd_varlen", H=4, Hkv=2, dh=32, seqs=b) == (ERR_ARG, None)


REFUSALS = [
    ("head_dim_32", dict(dh=32, rot=0)), ("head_dim_48", dict(dh=48, rot=0)), ("rot_32", dict(rot=32)), ("rot_128_at_64", dict(rot=128)),
    ("nseq_0", dict(nseq=0)), ("nseq_65536", dict(nseq=65536)), ("len_0", dict(lens=[129, 0, 1])), ("len_negative", dict(lens=[129, -3, 1])),
    ("overlap", dict(row0=[8, 136, 464])), ("unordered", dict(row0=[200, 8, 464], lens=[129, 129, 1])),
    ("past_total_rows", dict(total=464)), ("max_len_short", dict(max_len=256)),
    ("null_row0_host", dict(row0_host=False)), ("null_len_host", dict(len_host=False)), ("null_row0_dev", dict(row0_dev=None)),
    ("null_len_dev", dict(len_dev=None)),
    ("null_q", dict(q=None)), ("null_k", dict(k=None)), ("null_v", dict(v=None)), ("null_out", dict(out=None)), ("null_cos", dict(cos=None, sin=16)),
    ("null_sin", dict(sin=None, cos=16)), ("ld_unaligned", dict(ld=(4 + 4) * 64 + 4)), ("ldo_unaligned", dict(ldo=4 * 64 + 4)),
    ("q_off_unaligned", dict(q_off=4)), ("heads_not_a_multiple", dict(H=3)),
]
BWD_ONLY = [("null_" + n, {n: None}) for n in ("dout", "delta", "dq", "dk", "dv", "lse")]


@pytest.mark.parametrize("name,kw", REFUSALS + BWD_ONLY, ids=[r[0] for r in REFUSALS + BWD_ONLY])
def test_refusals_leave_the_plan_as_found(lib, name, kw):
    c = vc.CASES[5]
    assert query(lib, "fwd", c)[0] == OK and query(lib, "bwd", c)[0] == OK
    for entry in ("bwd",) if (name, kw) in BWD_ONLY else ("fwd", "bwd"):
        rc, p = query(lib, entry, c, **kw)
        assert rc == ERR_ARG and p == [SENTINEL] * 12, (name, entry, rc, p)


def test_refused_entry_points_launch_nothing(lib):
    """a refused call returns before any launch, so the entry points themselves can be asked without a device"""
    c = vc.CASES[5]
    D, kvw, ld = c["H"] * c["dh"], c["Hkv"] * c["dh"], (c["H"] + 2 * c["Hkv"]) * c["dh"]
    r0, ln = _i32(c["row0"]), _i32([129, 0, 1])
    seqs = (3, ctypes.cast(r0, ctypes.c_void_p), ctypes.cast(ln, ctypes.c_void_p), 16, 16, c["total"], 257, c["H"], c["Hkv"], c["dh"])
    head = (16, ld, 0, 16, ld, D, 16, ld, D + kvw)
    assert lib.kalle_attention_fwd_varlen(*head, 16, D, 16, 16, 16, 64, *seqs, None) == ERR_ARG
    assert lib.kalle_attn_last_plan() == 0
    assert lib.kalle_attention_bwd_varlen(*head, 16, 16, D, 16, 16, 16, 16, 16, 16, 16, 64, *seqs, None) == ERR_ARG
    assert lib.kalle_attn_last_plan() == 0
    assert lib.kalle_attention_fwd_varlen_plan(*head, 16, D, 16, 16, 16, 64, *seqs, None) == ERR_ARG       # NULL plan


# ------------------------------------------------------------------------------------------------ the wrong references are fair
def _moved(right, wrong, tol):
    return bool(((right - wrong).abs() > 2 * tol).any())


@pytest.mark.parametrize("wrong", [w for w in vc.WRONG if w != "lse_max_len_stride"])
def test_wrong_reference_moves_an_element_by_twice_its_allowance(wrong):
    i = vc.WRONG_CASE[wrong]
    right, bad = vc.refs(i), vc.wrong_refs(i, wrong)
    moved = {t: any(_moved(r[t], w[t], vc.tolerances(r)[t]) for r, w in zip(right, bad)) for t in ("out", "lse", "dq", "dk", "dv")}
    print(wrong, moved)
    if wrong == "rotary_packed_row":
        # rotary scores depend on position differences only, so shifting a whole sequence changes nothing but WHERE the rotated
        # q and k are rounded to bf16: far below the bf16 outputs' allowances, far above the fp32 lse's
        assert moved["lse"], (wrong, moved)
    else:
        assert moved["out"] and (moved["dq"] or moved["dk"] or moved["dv"]), (wrong, moved)   # the forward AND the backward catch it


def test_wrong_lse_stride_moves_an_element_by_twice_its_allowance():
    i = vc.WRONG_CASE["lse_max_len_stride"]
    c, right = vc.CASES[i], vc.refs(i)
    flat = vc.flat_stats(c, [r["lse"] for r in right])
    moved = []
    for b, r in enumerate(right):
        assert torch.equal(vc.stat_block(flat, c, b), r["lse"])                          # the header's layout reads back what it wrote
        got = vc.stat_block(flat, c, b, stride=max(c["lens"]))
        moved.append(bool((((got - r["lse"]).abs() > 2 * vc.tolerances(r)["lse"]) | torch.isnan(got)).any()))
    assert any(moved[:-1]), moved                        # (the longest sequence has stride max_len: the two layouts agree on it)
    assert not moved[c["lens"].index(max(c["lens"]))]


def test_hot_keys_and_case_list():
    """the case list is the one the feature was specified with; every hot key of every sequence holds p >= 0.2 (refs asserts)"""
    assert [c["lens"] for c in vc.CASES] == [[1, 2, 127, 128, 129], [257, 5, 256, 130], [129, 1, 128, 3], [130, 7], [300], [129, 257, 1]]
    assert vc.CASES[0]["row0"] == [0, 1, 3, 130, 258] and vc.CASES[5]["row0"] == [8, 200, 464] and vc.CASES[5]["total"] == 472
    assert [(c["dh"], c["H"], c["Hkv"], c["rot"]) for c in vc.CASES] == [(64, 4, 2, 64), (64, 2, 1, 64), (128, 2, 1, 128), (64, 2, 2, 0),
                                                                           (64, 4, 2, 64), (64, 4, 2, 64)]
    vc.refs(2)


# ------------------------------------------------------------------------------------------------ the mask check of pack_sequences
def test_mask_check_accepts_the_ragged_golden_batches():
    import golden_util as gu
    from kalle_audio_amd import llama_ops as LO
    n = 0
    for seed in range(1, 9):
        for kw in (dict(), dict(B=5, L=129), dict(B=2, L=64)):
            for b in (gu.llasa_batch_long(gu.LLASA_WIDE_CONFIG, seed, **kw), gu.llasa_batch(gu.LLASA_WIDE_CONFIG, seed)):
                m = torch.as_tensor(b["ids_mask"]) + torch.as_tensor(b["audio_mask"])
                lens = LO.packed_lengths(m)
                assert lens == [int(v) for v in (m > 0).sum(1)] and min(lens) >= 1 and lens[0] == m.shape[1]
                n += 1
    assert n == 48


def test_mask_check_rejects_left_padding_holes_and_empty_rows():
    from kalle_audio_amd import llama_ops as LO
    assert LO.packed_lengths(torch.tensor([[1., 2., 0.], [1., 0., 0.], [1., 1., 1.]])) == [2, 1, 3]
    for mask, row in (([[1, 1, 0], [0, 1, 1]], 1), ([[1, 0, 1, 0]], 0), ([[1, 1], [1, 0], [0, 0]], 2)):
        with pytest.raises(ValueError, match=f"row {row} "):
            LO.packed_lengths(torch.tensor(mask))
