"""-m gpu: kalle_attention_fwd_varlen / _bwd_varlen (csrc/attention.hip) on the cases of tests/attn_varlen_cases.py, by the
method of tests/test_attention_gpu.py.

Per case: q | k | v in ONE buffer with the fused layout's leading dimension (H + 2 Hkv) dh, every operand row outside the
sequences NaN (and every column outside the head windows of out / dout); out, lse, delta and dq | dk | dv in NaN-filled guarded
buffers.  Checked: the plan word (and that the host query named it); every sequence BIT FOR BIT against kalle_attention_fwd_hd /
_bwd_hd on that sequence alone (B = 1, causal, Nq = Nk = len, pointers advanced to its rows) - derived, not measured: a
workgroup runs the same statements on the same values - except the forward of a one-row sequence at head dim 64, which the dense
entry point sends to the single-query family; every element against the fp64 references per sequence in the units of DESIGN 2
with the allowances out/tiled, lse/tiled, dq|dk|dv/two_pass of test_attention_gpu.ALLOW (imported: the arithmetic is the tiled
and two-pass kernels'); the NaN sentinels outside every sequence in every output, lse and delta included; the four wrong
references (tests/test_attn_varlen_cpu.py shows each is fair) raise; refusals write nothing and leave plan word 0."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_varlen_cases as vc  # noqa: E402
from gpu_checks import NAN, U, Guard, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG = -1


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def _packed_operand(t, live, ld, col0):
    """bf16 [total + 2][ld] NaN buffer holding the live rows of the float64 t [total (+ 1)][cols] at column col0"""
    total = live.numel()
    buf = torch.full((total + 2, ld), NAN, device="cuda", dtype=torch.bfloat16)
    rows = live.nonzero().view(-1).cuda()
    buf[rows, col0:col0 + t.shape[1]] = t[:total].cuda()[rows].to(torch.bfloat16)
    return buf


def _sentinels_intact(t, live, what):
    """rows of `t` [total, ...] outside every sequence still NaN"""
    dead = (~live).nonzero().view(-1).cuda()
    assert torch.isnan(t[dead]).all(), (what, "a row outside every sequence was written")


def run_case(kl, i, wrong=None):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    c, x = vc.CASES[i], vc.inputs(i)
    right = vc.refs(i)
    ref = right if wrong in (None, "lse_max_len_stride") else vc.wrong_refs(i, wrong)
    lse_stride = max(c["lens"]) if wrong == "lse_max_len_stride" else None
    what = vc.case_id(c) + (f" [{wrong}]" if wrong else "")
    dh, H, Hkv, rot, total, lens, row0 = (c[k] for k in ("dh", "H", "Hkv", "rot", "total", "lens", "row0"))
    S, D, kvw = len(lens), H * dh, Hkv * dh
    ld, ldo = D + 2 * kvw, D + 16
    live = x["live"]
    qkv = _packed_operand(torch.cat([x["q"], x["k"], x["v"]], 1), live, ld, 0)
    cos, sin = (x["cos"].cuda(), x["sin"].cuda()) if rot else (None, None)
    seqs = ops.Packed(row0, lens, total, "cuda")
    og = Guard(total, D, ldo, torch.bfloat16, col0=8)
    lbuf, lse = _guarded(torch.full((H * total,), NAN, device="cuda"))
    fa = (P(qkv), ld, 0, P(qkv), ld, D, P(qkv), ld, D + kvw, og.buf.data_ptr() + 16, ldo, P(lse), P(cos), P(sin), rot, *seqs._args(), H, Hkv, dh)
    plan = (torch.zeros(12, dtype=torch.int32)).numpy()
    import ctypes
    assert lib.kalle_attention_fwd_varlen_plan(*fa, plan.ctypes.data_as(ctypes.c_void_p)) == 0
    rc = lib.kalle_attention_fwd_varlen(*fa, st)
    word = lib.kalle_attn_last_plan()
    torch.cuda.synchronize()
    assert rc == 0 and word == vc.fwd_word(c) == int(plan[0]), (what, rc, hex(word), hex(int(plan[0])))
    for b in range(S):
        r, tol = ref[b], vc.tolerances(right[b])
        n, r0 = lens[b], row0[b]
        check(og.v[r0:r0 + n], r["out"].cuda(), tol["out"].cuda(), f"{what} out of sequence {b}")
        check(vc.stat_block(lse, c, b, lse_stride), r["lse"].cuda(), tol["lse"].cuda(), f"{what} lse of sequence {b}")
    og.clean(what + " out")
    _clean(lbuf, lse, what + " lse")
    _sentinels_intact(og.v, live, what + " out")
    _sentinels_intact(lse.view(total, H), live, what + " lse")          # (blocks [H][len] at H row0: whole rows of H floats)
    # ---- backward, fed the reference's out (bf16) and lse (fp32) in the packed layout
    oo = torch.full((total + 2, ldo), NAN, device="cuda", dtype=torch.bfloat16)
    lse_in = vc.flat_stats(c, [r["lse"] for r in right]).float().cuda()
    for b in range(S):
        oo[row0[b]:row0[b] + lens[b], 8:8 + D] = right[b]["out"].cuda().to(torch.bfloat16)
    do = _packed_operand(x["dout"], live, ldo, 8)
    dbuf, delta = _guarded(torch.full((H * total,), NAN, device="cuda"))
    dg = Guard(total, ld, ld, torch.bfloat16)
    ba = (P(qkv), ld, 0, P(qkv), ld, D, P(qkv), ld, D + kvw, oo.data_ptr() + 16, do.data_ptr() + 16, ldo, P(lse_in), P(delta),
          P(dg.buf), P(dg.buf), P(dg.buf), P(cos), P(sin), rot, *seqs._args(), H, Hkv, dh)
    assert lib.kalle_attention_bwd_varlen_plan(*ba, plan.ctypes.data_as(ctypes.c_void_p)) == 0
    rc = lib.kalle_attention_bwd_varlen(*ba, st)
    word = lib.kalle_attn_last_plan()
    torch.cuda.synchronize()
    assert rc == 0 and word == vc.bwd_word(c) == int(plan[0]), (what, rc, hex(word), hex(int(plan[0])))
    for b in range(S):
        r, tol = ref[b], vc.tolerances(right[b])
        n, r0 = lens[b], row0[b]
        ob, dob = right[b]["out"].to(torch.bfloat16).double().view(n, H, dh), x["dout"][r0:r0 + n].view(n, H, dh)
        check(vc.stat_block(delta, c, b), r["delta"].cuda(), ((dh + 2) * U * (ob * dob).abs().sum(-1).t() + 1e-30).cuda(), f"{what} delta of sequence {b}")
        check(dg.v[r0:r0 + n, :D], r["dq"].cuda(), tol["dq"].cuda(), f"{what} dq of sequence {b}")
        check(dg.v[r0:r0 + n, D:D + kvw], r["dk"].cuda(), tol["dk"].cuda(), f"{what} dk of sequence {b}")
        check(dg.v[r0:r0 + n, D + kvw:], r["dv"].cuda(), tol["dv"].cuda(), f"{what} dv of sequence {b}")
    dg.clean(what + " dq | dk | dv")
    _clean(dbuf, delta, what + " delta")
    _sentinels_intact(dg.v, live, what + " dq | dk | dv")
    _sentinels_intact(delta.view(total, H), live, what + " delta")
    if wrong is not None:
        return
    # ---- bit identity with the dense entry points on every sequence alone
    esz = 2
    for b in range(S):
        n, r0 = lens[b], row0[b]
        tag = f"{what} sequence {b} vs dense"
        qp = qkv.data_ptr() + r0 * ld * esz
        d_og = Guard(n, D, ldo, torch.bfloat16, col0=8)
        d_lbuf, d_lse = _guarded(torch.full((H * n,), NAN, device="cuda"))
        if not (dh == 64 and n == 1):               # (Nq == 1 at head dim 64: the single-query family)
            rc = lib.kalle_attention_fwd_hd(qp, ld, 0, qp, ld, D, qp, ld, D + kvw, d_og.buf.data_ptr() + 16, ldo, P(d_lse), P(cos), P(sin), rot,
                                            None, 1, 1, H, Hkv, n, n, dh, st)
            assert rc == 0 and lib.kalle_attn_last_plan() == 1 | dh << 8, (tag, rc, hex(lib.kalle_attn_last_plan()))
            torch.cuda.synchronize()
            _exact(og.v[r0:r0 + n], d_og.v, tag + " out")
            _exact(vc.stat_block(lse, c, b), d_lse.view(H, n), tag + " lse")
        d_dbuf, d_delta = _guarded(torch.full((H * n,), NAN, device="cuda"))
        d_dg = Guard(n, ld, ld, torch.bfloat16)
        rc = lib.kalle_attention_bwd_hd(qp, ld, 0, qp, ld, D, qp, ld, D + kvw, oo.data_ptr() + 16 + r0 * ldo * esz, do.data_ptr() + 16 + r0 * ldo * esz,
                                        ldo, lse_in.data_ptr() + 4 * H * r0, P(d_delta), P(d_dg.buf), P(d_dg.buf), P(d_dg.buf), P(cos), P(sin), rot,
                                        None, 1, 1, H, Hkv, n, n, dh, st)
        assert rc == 0 and lib.kalle_attn_last_plan() == 3 | 16 | dh << 8, (tag, rc, hex(lib.kalle_attn_last_plan()))
        torch.cuda.synchronize()
        _exact(dg.v[r0:r0 + n], d_dg.v, tag + " dq | dk | dv")
        _exact(vc.stat_block(delta, c, b), d_delta.view(H, n), tag + " delta")


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=lambda i: vc.case_id(vc.CASES[i]))
def test_varlen_case(kl, i):
    run_case(kl, i)


@pytest.mark.parametrize("wrong", vc.WRONG)
def test_wrong_references_are_caught(kl, wrong):
    with pytest.raises(AssertionError, match="out of bound"):
        run_case(kl, vc.WRONG_CASE[wrong], wrong=wrong)


def test_wrappers_zero_the_rows_outside_every_sequence(kl):
    """ops.attention_fwd_varlen / _bwd_varlen on the case with gaps: what the kernels wrote is what the C ABI call wrote, and rows
    outside every sequence are exact zeros in out, lse and dq | dk | dv (the GEMMs behind read them)"""
    ops, lib = kl
    i = 5
    c, x = vc.CASES[i], vc.inputs(i)
    dh, H, Hkv, total = c["dh"], c["H"], c["Hkv"], c["total"]
    D, kvw = H * dh, Hkv * dh
    live = x["live"]
    qkv = torch.nan_to_num(_packed_operand(torch.cat([x["q"], x["k"], x["v"]], 1), live, D + 2 * kvw, 0)[:total])
    dout = torch.nan_to_num(_packed_operand(x["dout"], live, D, 0)[:total])
    seqs = ops.Packed(c["row0"], c["lens"], total, "cuda")
    rope = (x["cos"].cuda(), x["sin"].cuda())
    kw = dict(ldq=D + 2 * kvw, q_off=0, ldk=D + 2 * kvw, k_off=D, ldv=D + 2 * kvw, v_off=D + kvw, H=H, Hkv=Hkv, rope=rope, dh=dh)
    out, lse = ops.attention_fwd_varlen(qkv, qkv, qkv, seqs, **kw)
    assert ops.attn_last_plan() == vc.fwd_word(c)
    dq, dk, dv = ops.attention_bwd_varlen(qkv, qkv, qkv, out, dout, lse, seqs, **kw)
    assert ops.attn_last_plan() == vc.bwd_word(c) and dq is dk is dv and dq.shape == qkv.shape
    torch.cuda.synchronize()
    dead = (~live).nonzero().view(-1).cuda()
    for name, t in (("out", out), ("lse", lse.view(total, H)), ("dqkv", dq)):
        assert (t[dead] == 0).all() and torch.isfinite(t).all(), name
    right = vc.refs(i)
    for b, r in enumerate(right):
        r0, n = c["row0"][b], c["lens"][b]
        check(out[r0:r0 + n], r["out"].cuda(), vc.tolerances(r)["out"].cuda(), f"wrapper out of sequence {b}")


def test_refused_calls_write_nothing(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    c = vc.CASES[5]
    dh, H, Hkv, total = c["dh"], c["H"], c["Hkv"], c["total"]
    D, kvw = H * dh, Hkv * dh
    ld = D + 2 * kvw
    z = torch.zeros((total + 2, ld), device="cuda", dtype=torch.bfloat16)
    tab = torch.ones((total, dh // 2), device="cuda")
    og, dg = Guard(total, D, D, torch.bfloat16), Guard(total, ld, ld, torch.bfloat16)
    lse, delta = Guard(total, H), Guard(total, H)
    zl = torch.zeros((H * total,), device="cuda")
    base = dict(row0=c["row0"], lens=c["lens"], total=total, max_len=max(c["lens"]), dh=dh, rot=64, H=H, ld=ld, nseq=3)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        s = ops.Packed(a["row0"], a["lens"], a["total"], "cuda", max_len=a["max_len"])
        sa = list(s._args())
        sa[0] = a["nseq"]
        rf = lib.kalle_attention_fwd_varlen(P(z), a["ld"], 0, P(z), a["ld"], D, P(z), a["ld"], D + kvw, P(og.buf), D, P(lse.buf), P(tab), P(tab),
                                            a["rot"], *sa, a["H"], Hkv, a["dh"], st)
        pf = lib.kalle_attn_last_plan()
        rb = lib.kalle_attention_bwd_varlen(P(z), a["ld"], 0, P(z), a["ld"], D, P(z), a["ld"], D + kvw, P(z), P(z), D, P(zl), P(delta.buf),
                                            P(dg.buf), P(dg.buf), P(dg.buf), P(tab), P(tab), a["rot"], *sa, a["H"], Hkv, a["dh"], st)
        return rf, pf, rb, lib.kalle_attn_last_plan()

    bad = [dict(dh=32, rot=0), dict(rot=32), dict(rot=128), dict(nseq=0), dict(lens=[129, 0, 1]), dict(row0=[8, 136, 464]),
           dict(row0=[200, 8, 464], lens=[129, 129, 1]), dict(total=464), dict(max_len=256), dict(ld=ld + 4), dict(H=3)]
    for kw in bad:
        assert call(**kw) == (ERR_ARG, 0, ERR_ARG, 0), kw
    torch.cuda.synchronize()
    for gd, name in ((og, "out"), (lse, "lse"), (dg, "dq | dk | dv"), (delta, "delta")):
        gd.untouched(name)
