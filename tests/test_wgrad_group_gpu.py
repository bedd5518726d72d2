"""-m gpu: kalle_gemm_wgrad_group (csrc/gemm2.hip: gemm3_wgrad_group_kernel, gemm3_group_zero_kernel), every element of every
dw against fp64 on every region of its planner.

The cases are those of tests/wgrad_cases.py, found on the CPU with the host query kalle_gemm_wgrad_group_plan (which
tests/test_wgrad_plan_cpu.py checks there); every case asserts the five plan values kalle_gemm_wgrad_group_last_plan reports -
a case whose plan does not come out is a wrong case.  Every call runs on a thread of its own: the plan cache and the report are
per thread, so a case neither inherits a plan from an earlier test nor leaves one behind; the replay tests make both of their
calls on one such thread.

Reference per problem: ref = (0 or base) + dy.double().T @ x.double().
Bound per element, derived (the one tests/test_gemm_epilogue_gpu.py uses for fp32 weight gradients), not measured:
    2 * (tokens * 2^-24 * (|dy|^T |x|) + 8 * 2^-24 * (|base| + |dy|^T |x|))
fp32 accumulation of exact bf16 products in any order (the atomic slices come in any order) plus the final adds.

Operands: dy = 0.5 N(0, 1), x = N(0, 1) in bf16, each inside a NaN-filled allocation: the columns behind N / K up to the leading
dimension and the rows behind `tokens` are NaN, so a read past N, K or tokens shows.  Where a case has problems with different
token counts, the longest one's dy is a column window [N, 2N) of a [tokens][3N] buffer (the to_kv gradient of the DiT).  dw lives
in a Guard window, with lddw > K in the cases marked below (more than a third); accumulate mode starts from a random base,
overwrite mode from a window full of NaN: a tile that is neither stored nor cleared stays NaN, a tile cleared after a slice has
added to it loses that slice."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_cases as wc  # noqa: E402
from gpu_checks import Guard, check  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -24
ERR_ARG, ERR_UNSUPPORTED = -1, -3
SEEN = set()
PADDED_DW = {"whole-t8-nprob1", "whole-t72", "whole-t512-nprob8", "sliced-nprob1", "sliced-short-last", "sliced-tokens-differ",
             "mixed-inside-nprob1", "mixed-between", "mixed-tokens-differ"}        # lddw > K: 9 of 16 cases, and every replay


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def operands(problems, overwrite, padded, seed):
    """per problem (dy Guard, x Guard, dw Guard, base or None)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    longest = max(t for t, _, _ in problems) if len({t for t, _, _ in problems}) > 1 else -1
    out = []
    for tokens, n, k in problems:
        def rnd(r, c, s):
            return torch.randn((r, c), generator=g, device="cuda") * s
        if tokens == longest:
            dy = Guard(tokens, n, ld=3 * n, dtype=torch.bfloat16, init=rnd(tokens, n, 0.5), col0=n)
            longest = -1
        else:
            dy = Guard(tokens, n, ld=n + 8, dtype=torch.bfloat16, init=rnd(tokens, n, 0.5))
        x = Guard(tokens, k, ld=k + 16, dtype=torch.bfloat16, init=rnd(tokens, k, 1.0))
        base = None if overwrite else rnd(n, k, 1.0)
        dw = Guard(n, k, ld=k + (4 if padded else 0), init=base, col0=4 if padded else 0)
        out.append((dy, x, dw, base))
    return out


def reference(dy, x, base):
    """(ref, tol) in fp64"""
    prod = dy.v.double().T @ x.v.double()
    mag = dy.v.double().abs().T @ x.v.double().abs()
    b = base.double() if base is not None else torch.zeros_like(prod)
    tokens = dy.v.shape[0]
    return b + prod, 2 * (tokens * F32_EPS * mag + 8 * F32_EPS * (b.abs() + mag))


def launch(ops, ops_list, overwrite):
    """one kalle_gemm_wgrad_group + its report, on the calling thread"""
    assert ops.gemm_wgrad_group([(dy.v, x.v, dw.v) for dy, x, dw, _ in ops_list], overwrite=overwrite)
    return ops.wgrad_group_last_plan()


def verify(ops_list, what):
    torch.cuda.synchronize()
    for i, (dy, x, dw, base) in enumerate(ops_list):
        ref, tol = reference(dy, x, base)
        check(dw.v, ref, tol, f"{what} problem {i} dw {tuple(ref.shape)}")
        dw.clean(f"{what} problem {i}")


def expect(plan, overwrite, cached=0):
    return dict(tiles=plan[0], whole=plan[1], slices=plan[2], cleared=int(overwrite and plan[2] > 0), cached=cached)


@pytest.mark.parametrize("overwrite", [False, True], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("name", list(wc.CASES))
def test_every_region_per_element(kl, name, overwrite):
    ops, _ = kl
    problems, plan = wc.CASES[name]
    ol = operands(problems, overwrite, name in PADDED_DW, seed=len(name) + 100 * overwrite)
    got = wc.fresh_thread(launch, ops, ol, overwrite)
    assert got == expect(plan, overwrite), got
    verify(ol, name)
    SEEN.update(wc.regions(problems, plan, overwrite))
    SEEN.add("bench-plan" if name == "mixed-bench-reduced" else "")


@pytest.mark.parametrize("overwrite", [False, True], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("name", list(wc.REPLAY))
def test_plan_cache_replay_per_element(kl, name, overwrite):
    """shape A, then shape B of the same cache bucket on the same thread: B runs A's plan (tests/test_wgrad_plan_cpu.py shows
    that B planned afresh would get another one) with its own K-tile count - slices of another length, a short or an empty last
    slice, or no slices at all where B has fewer K-tiles than A's plan has slices"""
    ops, _ = kl
    shapes, ta, tb, plan_a, plan_b = wc.REPLAY[name]
    pa, pb = [(ta, n, k) for n, k in shapes], [(tb, n, k) for n, k in shapes]
    oa, ob = operands(pa, overwrite, True, seed=7), operands(pb, overwrite, True, seed=8)

    def both():
        return launch(ops, oa, overwrite), launch(ops, ob, overwrite)
    ga, gb = wc.fresh_thread(both)
    assert ga == expect(plan_a, overwrite) and gb == expect(plan_b, overwrite, cached=1), (ga, gb)
    verify(oa, name + " A")
    verify(ob, name + " B")
    SEEN.update(wc.regions(pb, plan_b, overwrite))
    SEEN.add("replay-" + name)


def test_rejections_leave_dw_untouched(kl):
    ops, lib = kl
    from kalle_audio_amd import _lib
    dy = Guard(1024, 264, ld=272, dtype=torch.bfloat16, init=torch.zeros(1024, 264))
    x = Guard(1024, 136, ld=144, dtype=torch.bfloat16, init=torch.zeros(1024, 136))
    dw = Guard(264, 136, ld=140)

    def rc(nprob=1, **field):
        arr = (_lib.WgradProblem * max(nprob, 1))()
        for w in arr:
            w.dy, w.lddy, w.x, w.ldx, w.dw, w.lddw = dy.v.data_ptr(), 272, x.v.data_ptr(), 144, dw.v.data_ptr(), 140
            w.N, w.K, w.tokens = 264, 136, 1024
        for f, v in field.items():
            setattr(arr[0], f, v)
        r = lib.kalle_gemm_wgrad_group(ctypes.cast(arr, ctypes.c_void_p), nprob, 1, None)
        assert set(ops.wgrad_group_last_plan().values()) == {0}          # nothing was launched
        return r
    assert rc(nprob=0) == ERR_ARG and rc(nprob=9) == ERR_ARG
    for field in (dict(N=260), dict(K=132), dict(lddy=268), dict(ldx=140), dict(lddw=138), dict(dy=dy.v.data_ptr() + 8),
                  dict(x=x.v.data_ptr() + 2), dict(dw=dw.v.data_ptr() + 4), dict(dw=None), dict(tokens=0)):
        assert rc(**field) == ERR_ARG, field
    assert rc(tokens=1020) == ERR_UNSUPPORTED
    assert lib.kalle_gemm_wgrad_group(None, 1, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    dw.untouched("rejected kalle_gemm_wgrad_group")
    assert not ops.gemm_wgrad_group([(dy.v[:100], x.v[:100], dw.v)])      # tokens % 8: the Python caller is told to fall back
    dw.untouched("tokens % 8")


# ------------------------------------------------------------------------------------------------ wrong references
# On "sliced-nprob1" - 1024 tokens of (264, 136): tile 0 = rows 0 .. 255, tile 1 = the 8-row edge tile, both cut into two slices
# of 512 tokens.  Each wrong reference differs from the right one by more than MARGIN x the allowance at some element (asserted
# before the check), and the same check that passes the right reference must fail it.
MARGIN = 2.0


def _wrong_refs(dy, x, base, ref):
    d, xx = dy.v.double(), x.v.double()
    b = base.double()
    half = d[512:].T @ xx[512:]
    g = torch.Generator().manual_seed(3)
    extra = torch.outer((torch.randn(264, generator=g) * 0.5).bfloat16().double(), torch.randn(136, generator=g).bfloat16().double())
    w = {}
    w["one 4-column group of the edge tile left at base"] = ref.clone()
    w["one 4-column group of the edge tile left at base"][263, 132:136] = b[263, 132:136]
    w["the second slice of the edge tile dropped"] = ref.clone()
    w["the second slice of the edge tile dropped"][256:] -= half[256:]
    w["the edge tile counted twice"] = ref.clone()
    w["the edge tile counted twice"][256:] += (ref - b)[256:]
    w["one token row behind `tokens` included"] = ref + extra.to(ref.device)
    return w


def _wrong_case(ops, overwrite):
    problems, plan = wc.CASES["sliced-nprob1"]
    ol = operands(problems, overwrite, True, seed=11)
    assert wc.fresh_thread(launch, ops, ol, overwrite) == expect(plan, overwrite)
    torch.cuda.synchronize()
    return ol[0]


@pytest.fixture(scope="module")
def wrong_acc(kl):
    dy, x, dw, base = _wrong_case(kl[0], False)
    ref, tol = reference(dy, x, base)
    check(dw.v, ref, tol, "right reference")
    return dw.v.clone(), ref, tol, _wrong_refs(dy, x, base, ref)


@pytest.mark.parametrize("which", range(4))
def test_wrong_reference_is_caught(wrong_acc, which):
    out, ref, tol, wrongs = wrong_acc
    name, wrong = list(wrongs.items())[which]
    margin = ((wrong - ref).abs() / tol).max().item()
    assert margin > MARGIN, (name, margin)
    with pytest.raises(AssertionError, match="out of bound"):
        check(out, wrong, tol, name)
    SEEN.add("wrong-" + str(which))


def test_wrong_reference_base_added_in_overwrite_mode(kl):
    dy, x, dw, _ = _wrong_case(kl[0], True)
    ref, tol = reference(dy, x, None)
    check(dw.v, ref, tol, "right reference")
    base = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5)).to(ref.device).double()
    assert (base.abs() / tol).max().item() > MARGIN
    with pytest.raises(AssertionError, match="out of bound"):
        check(dw.v, ref + base, tol, "base added in overwrite mode")
    SEEN.add("wrong-4")


def test_every_region_was_reached():
    """closing test: in this process every planner region ran in a per-element case, every replay and wrong reference ran,
    and so did the bench's mixed plan"""
    want = set(wc.REGIONS) | {"replay-" + n for n in wc.REPLAY} | {f"wrong-{i}" for i in range(5)} | {"bench-plan"}
    assert want <= SEEN, sorted(want - SEEN)
