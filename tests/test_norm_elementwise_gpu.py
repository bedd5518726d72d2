"""-m gpu: the norm, elementwise, Llasa-tail and conformer entry points of include/kalle_hip.h, element by element against
the fp64 references of tests/kernel_refs.py (which test_kernel_refs_cpu.py checks against torch on the CPU).

Conventions (those of test_gemm_epilogue_gpu.py): every element is bounded and the first offender is reported; everything a
call must not write starts NaN and must still be NaN (`Guard`); operand padding is NaN so that a read at a wrong place
shows; accumulating outputs start from random contents and are checked as before + ref; second outputs defined as a rounding
of the first (dx_bf16, Adam's param_bf16) are compared bit for bit with torch's rounding of the first.  The calls go through
ctypes (`ops._p`, `ops._stream`): the Python wrappers allocate their outputs themselves, which leaves no room for sentinels,
leading dimensions, NULL arguments or caller-initialised accumulators.

Error model.  u = 2^-24: one fp32 rounding is u |term|; an n-term fp32 sum is within n u sum|terms| of the exact sum in any
order (which is what the atomics need); one rounding to bf16 is BF16_REL |ref| = 2^-8 |ref|.  Each check states its terms.
  LayerNorm forward (y bf16, row statistics fp32), m1 = mean_D|x|:
      dmu <= (D + 2) u m1;  dvar / (var + eps) <= (D + 4) u + 4 dmu^2 / (var + eps);  drs / rs <= dvar / 2 + RSQRT u
      |y - ref| <= |gamma (1 + scale)| (rs (dmu + 2 u (|x| + |mu|)) + |xhat| drs / rs) + 6 u mag + BF16_REL |ref|
  LayerNorm backward (statistics are inputs: the fp32 roundings of the reference's), exh = 3 u (|x| + |mu|) rs:
      dx:  rs (dc1 + |xh| dc2 + |c2| exh + 6 u (|dh| + |c1| + |xh c2|)) + 2 u |dres| + u |ref|,
           dc1 = (D + 4) u mean|dh|, dc2 = (D + 6) u mean|dh xh| + mean(|dh| exh)
      dgamma / dbeta / colsum / dscale / dshift: the n-term sum bound over the rows (+ the accumulator's contents) + the
           propagated exh.
  RMSNorm the same without the mean.  Elementwise kernels: a few u of the magnitude of each TERM (never of a cancelling
  result: 1 - sigmoid and 1 + erf are bounded by the terms), + BF16_REL |ref| where the output is bf16.  Pure data movement is
  bit-exact.
The library is built with -ffast-math: rsqrtf, __expf and the reciprocal, erff, sinf / cosf, the division and sqrtf have no
bound derivable from the source.  Their allowances (ALLOW below) are MEASURED: the worst |kernel - fp64 ref| over this file's
cases on fp32 outputs, in units of u * (the magnitude named next to each constant), times a margin of 4 - never taken from
another run's kernel output.  `_check(..., key=, unit=)` records the figures in MEASURED; the last test of the file prints them
(`-s`) and holds each to its allowance."""
import ctypes
import itertools
import math
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as kr  # noqa: E402
from gpu_checks import Guard, _bits, _exact, check  # noqa: E402,F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16_REL = 2.0 ** -8
F32, BF16 = 1, 0
ERR_ARG = -1
NAN = float("nan")

# measured on one MI355X (ROCm 7, -O3 -ffast-math), 2026-10-16: worst deviation over this file's cases in units of u * magnitude,
# then x 4 margin (other seeds, other compiler versions; a structural error is of order 1 / u in these units)
ALLOW = {
    "RSQRT": 10.0,      # rsqrtf: LayerNorm / RMSNorm row statistic (fp32), unit |rstd|                          measured 2.41
    "SIGMOID": 10.0,    # __expf + reciprocal: silu fwd fp32, unit |x|; silu bwd fp32, unit |dy| (1 + |x|)           measured 2.37
    "ERF": 8.0,         # erff (+ __expf): gelu fwd fp32, unit |x|; gelu bwd fp32, unit |dy| (1 + |x|)               measured 1.97
    "SINCOS": 9.0,      # sinf / cosf: Fourier features fp32, unit 1 + |angle|; diffuse "v", unit 3 (|x| + |noise|)   measured 2.19
    "DIV": 15.0,        # division / sqrtf: MSE dout and KL backward (fp32), unit |quotient|; also applied to Adam's update
                        # (unit |update|) and the l2 head norm                                                     measured 3.59
    "EXP": 27.0,        # expf / logf / log1pf of the two-Gaussian KL: its backward (fp32), unit = the products' magnitudes  measured 6.65
}
MEASURED = {}


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


def _check(out, ref, tol, what, key=None, unit=None):
    return check(out, ref, tol, what, key, unit, MEASURED)


def _nan_tail(t, extra=2):
    """`t` [rows][D] followed by `extra` NaN rows (what a read past `rows` would see); returns the [rows] view"""
    buf = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), NAN, device="cuda", dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def _mod(nb, D, g, slot):
    """a [nb + 1][6 D] modulation tensor, NaN except the [slot D, slot D + D) slice of the first nb rows"""
    m = torch.full((nb + 1, 6 * D), NAN, device="cuda")
    m[:nb, slot * D:(slot + 1) * D] = _randn((nb, D), g, 0.3)
    return m, m[:nb, slot * D:(slot + 1) * D]


def _win(buf, B, R, ld, C):
    """the [B][R][C] window of a [B'][batch stride] buffer whose matrices have leading dimension ld"""
    return torch.as_strided(buf, (B, R, C), (buf.stride(0), ld, 1))


def _outside(buf, B, R, ld, C):
    m = torch.ones_like(buf, dtype=torch.bool)
    _win(m, B, R, ld, C)[:] = False
    return m


def _bf16_ties_away(t):
    """fp32 -> bf16 with ties rounded AWAY from zero (the wrong rounding, for the tests that must fail)"""
    b = t.contiguous().view(torch.int32)
    return (((b + 0x8000) >> 16) << 16).view(torch.float32).bfloat16()


# ================================================================================================ LayerNorm / adaLN
LN_FACTORS = {
    "D": [8, 64, 520, 1536, 2048, 2560, 3584, 4096],
    "rows": [1, 3, 9, 2016, 8200],
    "rpb": [1, 21, 126],
    "xf32": [True, False],
    "beta": [False, True],
    "mod": ["none", "scale", "shift", "both"],
    "nostat": [False, True],                    # mean / rstd NULL in the forward
    "dres": ["none", "sep", "alias"],
    "dxb": [False, True],
    "null": ["none", "dgamma", "second", "both"],
    "flavour": ["parts", "acc", "colsum"],
}


def _ln_valid(c):
    if c["rows"] > 8192 and c["D"] > 520:        # the grid-stride regime at a small D only
        return False
    if c["flavour"] == "colsum" and c["null"] in ("second", "both"):     # (kalle_layernorm_bwd_colsum requires its accumulator)
        return False
    return True


def _pairwise(factors, valid, seed, n_cand=300):
    rnd = random.Random(seed)
    keys = list(factors)
    base = {k: factors[k][0] for k in keys}
    need = {(k1, i1, k2, i2) for k1, k2 in itertools.combinations(keys, 2)
            for i1 in range(len(factors[k1])) for i2 in range(len(factors[k2]))
            if _pair_possible(factors, valid, k1, i1, k2, i2)}
    rows = []
    while need:
        best, best_cov, best_ix = None, -1, None
        for _ in range(n_cand):
            ix = {k: rnd.randrange(len(factors[k])) for k in keys}
            c = {k: factors[k][i] for k, i in ix.items()}
            if not valid(c):
                continue
            cov = sum((k1, ix[k1], k2, ix[k2]) in need for k1, k2 in itertools.combinations(keys, 2))
            if cov > best_cov:
                best, best_cov, best_ix = c, cov, ix
        assert best_cov > 0, sorted(need)[:5]
        rows.append(best)
        need -= {(k1, best_ix[k1], k2, best_ix[k2]) for k1, k2 in itertools.combinations(keys, 2)}
    return rows


def _pair_possible(factors, valid, k1, i1, k2, i2):
    """some valid case holds this pair of values (the other factors are free)"""
    keys = [k for k in factors if k not in (k1, k2)]
    fixed = {k1: factors[k1][i1], k2: factors[k2][i2]}
    if valid({**{k: factors[k][0] for k in keys}, **fixed}):
        return True
    return any(valid({**{k: factors[k][0] for k in keys}, **fixed, ka: va, kb: vb})
               for ka, kb in itertools.combinations(keys, 2) for va in factors[ka] for vb in factors[kb])


LN_PAIRWISE = _pairwise(LN_FACTORS, _ln_valid, 20261016)
LN_HEADLINE = dict(D=1536, rows=256 * 126, rpb=126, xf32=True, beta=False, mod="both", nostat=False, dres="alias", dxb=True,
                   null="none", flavour="colsum")


def _cover_complete(factors, valid, cases):
    for k1, k2 in itertools.combinations(list(factors), 2):
        for i1, i2 in itertools.product(range(len(factors[k1])), range(len(factors[k2]))):
            if _pair_possible(factors, valid, k1, i1, k2, i2):
                v1, v2 = factors[k1][i1], factors[k2][i2]
                assert any(r[k1] == v1 and r[k2] == v2 for r in cases), (k1, v1, k2, v2)


def test_ln_pairwise_cover_is_complete():
    """(host side) every possible pair of option values appears in some LayerNorm case"""
    _cover_complete(LN_FACTORS, _ln_valid, LN_PAIRWISE)
    assert all(_ln_valid(c) for c in LN_PAIRWISE)


LN_CHUNK = 4096


def run_ln(kl, c, seed, wrong=None):
    """forward, one backward flavour and (whole batches only) kalle_adaln_mod_bwd of case `c`; `wrong` names a deliberately
    wrong reference (see test_ln_wrong_reference_is_caught)"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(seed)
    D, rows, rpb = c["D"], c["rows"], c["rpb"]
    nb = (rows + rpb - 1) // rpb
    xdt = torch.float32 if c["xf32"] else torch.bfloat16
    x = _nan_tail((_randn((rows, D), g, 1.3) + 0.4).to(xdt))
    gamma = _nan_tail(1 + 0.2 * _randn((D,), g), 8)
    beta = _nan_tail(0.2 * _randn((D,), g), 8) if c["beta"] else None
    has_sc, has_sh = c["mod"] in ("scale", "both"), c["mod"] in ("shift", "both")
    modbuf_sc, scale = _mod(nb, D, g, 1) if has_sc else (None, None)
    modbuf_sh, shift = _mod(nb, D, g, 3) if has_sh else (None, None)
    ld_mod = 6 * D
    eps = 1e-5
    y = Guard(rows, D, dtype=torch.bfloat16)
    mean, rstd = Guard(1, rows), Guard(1, rows)
    rc = lib.kalle_layernorm_fwd(P(x), F32 if c["xf32"] else BF16, P(gamma), P(beta), P(scale), P(shift), ld_mod, rpb, P(y.v),
                                 None if c["nostat"] else P(mean.v), None if c["nostat"] else P(rstd.v), rows, D, eps, st)
    assert rc == 0, rc
    # ---- backward operands: the statistics are the fp32 roundings of the REFERENCE's (inputs, not results under test)
    dy = _nan_tail(_randn((rows, D), g).bfloat16())
    dres0 = _randn((rows, D), g) if c["dres"] != "none" else None
    dx = Guard(rows, D, init=dres0 if c["dres"] == "alias" else None)
    dres = None if c["dres"] == "none" else (dx.v if c["dres"] == "alias" else _nan_tail(dres0))
    dxb = Guard(rows, D, dtype=torch.bfloat16) if c["dxb"] else None
    nparts = lib.kalle_layernorm_bwd_parts(rows)
    assert nparts == min(1024, max(1, (rows + 7) // 8))
    acc = c["flavour"] != "parts"
    prow = 1 if acc else nparts
    before_g, before_b = (_randn((1, D), g), _randn((1, D), g)) if acc else (None, None)
    dgp = Guard(prow, D, init=before_g) if c["null"] not in ("dgamma", "both") else None
    dbp = Guard(prow, D, init=before_b) if c["null"] not in ("second", "both") else None
    xd = x.double()
    gam, bet = gamma.double(), None if beta is None else beta.double()
    scd, shd = None if scale is None else scale.double(), None if shift is None else shift.double()
    _, mu_all, rs_all = kr.layernorm_fwd(xd, gam) if rows <= LN_CHUNK else (None,) + tuple(
        torch.cat(p) for p in zip(*[kr.layernorm_fwd(xd[r:r + LN_CHUNK], gam)[1:] for r in range(0, rows, LN_CHUNK)]))
    mean32, rstd32 = _nan_tail(mu_all.float(), 8), _nan_tail(rs_all.float(), 8)
    fn = {"parts": lib.kalle_layernorm_bwd, "acc": lib.kalle_layernorm_bwd_acc, "colsum": lib.kalle_layernorm_bwd_colsum}[c["flavour"]]
    rc = fn(P(dy), P(x), F32 if c["xf32"] else BF16, P(gamma), P(scale), ld_mod, rpb, P(mean32), P(rstd32), P(dres), P(dx.v),
            P(dxb.v) if dxb else None, P(dgp.v) if dgp else None, P(dbp.v) if dbp else None, rows, D, st)
    assert rc == 0, rc
    nfull = rows // rpb
    if nfull:
        dsc, dsh = Guard(nfull, D, ld=ld_mod), Guard(nfull, D, ld=ld_mod)
        rc = lib.kalle_adaln_mod_bwd(P(dy), P(x), F32 if c["xf32"] else BF16, P(gamma), P(beta), P(mean32), P(rstd32), P(dsc.v),
                                     P(dsh.v), ld_mod, nfull, rpb, D, st)
        assert rc == 0, rc
    torch.cuda.synchronize()

    what = f"ln {c}"
    sum_g = torch.zeros(D, dtype=torch.float64, device="cuda")
    sum_b, abs_g, abs_b, exh_g, col_dxb, abs_dxb = (torch.zeros_like(sum_g) for _ in range(6))
    for r0 in range(0, rows, LN_CHUNK):
        r1 = min(rows, r0 + LN_CHUNK)
        xc = xd[r0:r1]
        idx = torch.arange(r0, r1, device="cuda") // rpb
        sc_r = None if scd is None else scd[idx]
        sh_r = None if shd is None else shd[idx]
        if wrong == "next_batch_mod":                       # the last row of every batch reads the next batch's modulation
            last = (torch.arange(r0, r1, device="cuda") % rpb == rpb - 1) & (idx + 1 < nb)
            widx = torch.where(last, idx + 1, idx)
            sc_r = None if scd is None else scd[widx]
            sh_r = None if shd is None else shd[widx]
        yr, mu, rs = kr.layernorm_fwd(xc, gam, None if wrong == "beta_dropped" else bet, sc_r, sh_r, 1, eps)
        # forward bound
        m1 = xc.abs().mean(-1, keepdim=True)
        var_e = rs[:, None].pow(-2)
        dmu = (D + 2) * U * m1
        drs_rel = 0.5 * ((D + 4) * U + 4 * dmu.pow(2) / var_e) + ALLOW["RSQRT"] * U
        xhat = (xc - mu[:, None]) * rs[:, None]
        mul = gam.abs() * (1 if sc_r is None else (1 + sc_r).abs())
        mag = xhat.abs() * mul + (0 if bet is None else bet.abs() * (1 if sc_r is None else (1 + sc_r).abs())) \
            + (0 if sh_r is None else sh_r.abs())
        tol = mul * (rs[:, None] * (dmu + 2 * U * (xc.abs() + mu[:, None].abs())) + xhat.abs() * drs_rel) + 6 * U * mag \
            + BF16_REL * yr.abs() + 1e-30
        _check(y.v[r0:r1], yr, tol, what + f" y rows {r0}..", None)
        if not c["nostat"]:
            _check(mean.v[0, r0:r1], mu, (dmu[:, 0] + U * mu.abs()), what + " mean")
            _check(rstd.v[0, r0:r1], rs, drs_rel[:, 0] * rs, what + " rstd", "RSQRT", rs)
        # backward bound (statistics as given)
        mu32, rs32 = mean32[r0:r1].double(), rstd32[r0:r1].double()
        dyc = dy[r0:r1].double()
        dres_c = None if dres0 is None else dres0[r0:r1].double()
        sc_b = None if scd is None else scd[idx]
        dxr, dg_r, db_r = kr.layernorm_bwd(dyc, xc, gam, mu32, rs32, sc_b, 1, dres_c)
        if wrong == "dres_twice":
            dxr = dxr + dres_c
        gq = dyc if sc_b is None else dyc * (1 + sc_b)
        if wrong == "dgamma_no_scale":
            dg_r = (dyc * ((xc - mu32[:, None]) * rs32[:, None])).sum(0)
        xh = (xc - mu32[:, None]) * rs32[:, None]
        exh = 3 * U * (xc.abs() + mu32[:, None].abs()) * rs32[:, None]
        dh = gq * gam
        c1, c2 = dh.mean(-1, keepdim=True), (dh * xh).mean(-1, keepdim=True)
        dc1 = (D + 4) * U * dh.abs().mean(-1, keepdim=True)
        dc2 = (D + 6) * U * (dh * xh).abs().mean(-1, keepdim=True) + (dh.abs() * exh).mean(-1, keepdim=True)
        tol = rs32[:, None] * (dc1 + xh.abs() * dc2 + c2.abs() * exh + 6 * U * (dh.abs() + c1.abs() + (xh * c2).abs())) \
            + (0 if dres_c is None else 2 * U * dres_c.abs()) + U * dxr.abs() + 1e-30
        if wrong == "last_row" and r1 == rows:
            dxr = dxr.clone()
            dxr[-1] = 0 if dres_c is None or c["dres"] != "alias" else dres_c[-1]       # (left at its previous contents)
        if wrong == "last8":
            dxr = dxr.clone()
            dxr[:, -8:] = 0 if dres_c is None or c["dres"] != "alias" else dres_c[:, -8:]
        _check(dx.v[r0:r1], dxr, tol, what + f" dx rows {r0}..")
        sum_g += dg_r
        sum_b += db_r
        abs_g += (gq * xh).abs().sum(0)
        abs_b += gq.abs().sum(0)
        exh_g += (gq.abs() * exh).sum(0)
        rb = dx.v[r0:r1].bfloat16().double()
        col_dxb += rb.sum(0)
        abs_dxb += rb.abs().sum(0)
        del yr, xhat, mag, tol, dxr, xh, exh, dh, gq, rb
    y.clean(what + " y")
    dx.clean(what + " dx")
    mean.clean(what) if not c["nostat"] else mean.untouched(what)
    rstd.clean(what) if not c["nostat"] else rstd.untouched(what)
    if dxb:
        expect = _bf16_ties_away(dx.v) if wrong == "tie_away" else dx.v.bfloat16()
        _exact(dxb.v, expect, what + " dx_bf16 == bf16(dx_out)")
        dxb.clean(what + " dx_bf16")
    n = rows + nparts + 4
    for buf, before, ref, mag_abs, prop, name in ((dgp, before_g, sum_g, abs_g, exh_g, "dgamma"),
                                                  (dbp, before_b, col_dxb if c["flavour"] == "colsum" else sum_b,
                                                   abs_dxb if c["flavour"] == "colsum" else abs_b, 0, "second")):
        if buf is None:
            continue
        b0 = before[0].double() if acc else 0
        tol = n * U * ((before[0].double().abs() if acc else 0) + mag_abs) + prop + 1e-30
        _check(buf.v.double().sum(0), ref + b0, tol, what + " " + name)
        buf.clean(what + " " + name)
    if nfull:
        nr = nfull * rpb
        ds_ref = torch.zeros((nfull, D), dtype=torch.float64, device="cuda")
        dh_ref, ds_tol, dh_tol = torch.zeros_like(ds_ref), torch.zeros_like(ds_ref), torch.zeros_like(ds_ref)
        bstep = max(1, LN_CHUNK // rpb)
        for b0 in range(0, nfull, bstep):
            b1 = min(nfull, b0 + bstep)
            sl = slice(b0 * rpb, b1 * rpb)
            xc, dyc, mu32, rs32 = xd[sl], dy[sl].double(), mean32[sl].double(), rstd32[sl].double()
            ds_ref[b0:b1], dh_ref[b0:b1] = kr.adaln_mod_bwd(dyc, xc, gam, None if wrong == "beta_dropped" else bet, mu32, rs32,
                                                            b1 - b0, rpb)
            ln = (xc - mu32[:, None]) * rs32[:, None] * gam + (0 if bet is None else bet)
            exh = 3 * U * (xc.abs() + mu32[:, None].abs()) * rs32[:, None]
            ds_tol[b0:b1] = ((rpb + 4) * U * (dyc * ln).abs() + dyc.abs() * (exh * gam.abs() + 3 * U * ln.abs())).view(b1 - b0, rpb, D).sum(1)
            dh_tol[b0:b1] = (rpb * U * dyc.abs()).view(b1 - b0, rpb, D).sum(1)
        _check(dsc.v, ds_ref, ds_tol + 1e-30, what + " dscale")
        _check(dsh.v, dh_ref, dh_tol + 1e-30, what + " dshift")
        dsc.clean(what + " dscale")
        dsh.clean(what + " dshift")


@pytest.mark.parametrize("idx", range(len(LN_PAIRWISE)))
def test_layernorm_pairwise(kl, idx):
    run_ln(kl, LN_PAIRWISE[idx], 100 + idx)


def test_layernorm_headline_shape(kl):
    run_ln(kl, LN_HEADLINE, 7)


LN_WRONG_CASES = [
    dict(D=520, rows=9, rpb=1, xf32=True, beta=True, mod="both", nostat=False, dres="sep", dxb=True, null="none", flavour="parts"),
    dict(D=1536, rows=2016, rpb=126, xf32=False, beta=True, mod="both", nostat=False, dres="alias", dxb=True, null="none", flavour="acc"),
    dict(D=4096, rows=3, rpb=1, xf32=True, beta=True, mod="scale", nostat=True, dres="sep", dxb=True, null="none", flavour="acc"),
]


@pytest.mark.parametrize("ci", range(len(LN_WRONG_CASES)))
@pytest.mark.parametrize("wrong", ["beta_dropped", "next_batch_mod", "dgamma_no_scale", "dres_twice", "last_row", "last8", "tie_away"])
def test_ln_wrong_reference_is_caught(kl, wrong, ci):
    """the real kernel against a deliberately wrong reference: the comparison must raise on every case the error applies to"""
    c = LN_WRONG_CASES[ci]
    if wrong == "tie_away":
        if c["rows"] * c["D"] < 2 ** 21:
            c = dict(c, rows=2016, rpb=126, D=1536)        # an exact tie needs ~2^16 elements: run it where there are 3 M
    with pytest.raises(AssertionError, match="out of bound|differ"):
        run_ln(kl, c, 55 + ci, wrong=wrong)


def test_layernorm_rejects(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    x, gam = torch.zeros((4, 4104), device="cuda"), torch.ones(4104, device="cuda")
    dyb = torch.zeros((4, 4104), device="cuda", dtype=torch.bfloat16)
    stat = torch.ones(4, device="cuda")
    for D in (12, 4104, 0):
        y, dx = Guard(4, 4104, dtype=torch.bfloat16), Guard(4, 4104)
        assert lib.kalle_layernorm_fwd(P(x), F32, P(gam), None, None, None, 0, 1, P(y.v), None, None, 4, D, 1e-5, st) == ERR_ARG
        assert lib.kalle_layernorm_bwd(P(dyb), P(x), F32, P(gam), None, 0, 1, P(stat), P(stat), None, P(dx.buf), None, None, None,
                                       4, D, st) == ERR_ARG
        assert lib.kalle_rmsnorm_fwd(P(x), F32, P(gam), 0, 0, P(dx.buf), F32, None, 4, D, 1e-6, st) == ERR_ARG
        assert lib.kalle_rmsnorm_bwd(P(x), F32, P(x), F32, P(gam), 0, 0, P(stat), P(dx.buf), None, None, None, 4, D, st) == ERR_ARG
        torch.cuda.synchronize()
        y.untouched("ln fwd")
        dx.untouched("bwd")
    y = Guard(4, 64, dtype=torch.bfloat16)
    assert lib.kalle_layernorm_fwd(None, F32, P(gam), None, None, None, 0, 1, P(y.v), None, None, 4, 64, 1e-5, st) == ERR_ARG
    assert lib.kalle_layernorm_fwd(P(x), F32, None, None, None, None, 0, 1, P(y.v), None, None, 4, 64, 1e-5, st) == ERR_ARG
    assert lib.kalle_layernorm_fwd(P(x), F32, P(gam), None, P(gam), None, 6 * 64 + 2, 1, P(y.v), None, None, 4, 64, 1e-5, st) == ERR_ARG
    assert lib.kalle_layernorm_fwd(P(x), F32, P(gam), None, P(gam), None, 6 * 64, 0, P(y.v), None, None, 4, 64, 1e-5, st) == ERR_ARG
    assert lib.kalle_layernorm_fwd(P(x), F32, P(gam), None, None, None, 0, 1, P(y.v), None, None, 0, 64, 1e-5, st) == ERR_ARG
    dx = Guard(4, 64)
    assert lib.kalle_layernorm_bwd_colsum(P(dyb), P(x), F32, P(gam), None, 0, 1, P(stat), P(stat), None, P(dx.v), None, None, None,
                                          4, 64, st) == ERR_ARG
    assert lib.kalle_layernorm_bwd_acc(P(dyb), P(x), F32, P(gam), None, 0, 1, None, P(stat), None, P(dx.v), None, None, None,
                                       4, 64, st) == ERR_ARG
    assert lib.kalle_adaln_mod_bwd(P(dyb), P(x), F32, P(gam), None, P(stat), P(stat), P(dx.v), None, 64, 1, 4, 64, st) == ERR_ARG
    assert lib.kalle_adaln_mod_bwd(P(dyb), P(x), F32, P(gam), None, P(stat), P(stat), P(dx.v), P(dx.v), 64, 1, 4, 12, st) == ERR_ARG
    assert lib.kalle_colsum(P(x), F32, 4104, P(dx.v), 4, 3, 0, st) == ERR_ARG
    assert lib.kalle_colsum(P(x), F32, 4103, P(dx.v), 4, 2, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    y.untouched("ln fwd")
    dx.untouched("ln bwd")


# ================================================================================================ RMSNorm
RMS_CASES = [  # (D, rows, xf32, second-type f32 (y fwd / dy bwd), per-batch rpb (0 = shared scale), dres, dxb, acc)
    (8, 1, True, True, 0, "none", False, False), (64, 3, True, False, 2, "sep", True, True),
    (520, 9, False, True, 4, "alias", True, False), (1536, 2016, False, False, 126, "sep", True, True),
    (2048, 9, True, True, 0, "alias", False, True), (2560, 3, False, False, 1, "none", True, False),
    (3584, 9, True, False, 0, "sep", True, False), (4096, 2016, False, True, 21, "none", False, True),
    (64, 8200, False, False, 0, "sep", True, True), (520, 8200, True, True, 126, "alias", True, False),
]


def run_rms(kl, case, seed, wrong=None):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    D, rows, xf32, sf32, rpb, dresm, want_dxb, acc = case
    g = _gen(seed)
    what = f"rms {case}"
    xdt, sdt = (torch.float32 if xf32 else torch.bfloat16), (torch.float32 if sf32 else torch.bfloat16)
    x = _nan_tail((_randn((rows, D), g, 1.3) + 0.2).to(xdt))
    if rpb:
        nb = (rows + rpb - 1) // rpb
        sbuf = torch.full((nb + 1, D + 24), NAN, device="cuda")
        sbuf[:nb, :D] = 1 + 0.2 * _randn((nb, D), g)
        scale, ld = sbuf[:nb, :D], D + 24
    else:
        scale, ld = _nan_tail(1 + 0.2 * _randn((D,), g), 8), 0
    y, rr = Guard(rows, D, dtype=sdt), Guard(1, rows)
    assert lib.kalle_rmsnorm_fwd(P(x), int(xf32), P(scale), ld, rpb, P(y.v), int(sf32), P(rr.v), rows, D, 1e-6, st) == 0
    xd, sd = x.double(), scale.double()
    yr, rrms = kr.rmsnorm_fwd(xd, sd, rpb, 1e-6)
    rr32 = _nan_tail(rrms.float(), 8)
    dy = _nan_tail(_randn((rows, D), g).to(sdt))
    dres0 = _randn((rows, D), g) if dresm != "none" else None
    dx = Guard(rows, D, init=dres0 if dresm == "alias" else None)
    dres = None if dresm == "none" else (dx.v if dresm == "alias" else _nan_tail(dres0))
    dxb = Guard(rows, D, dtype=torch.bfloat16) if want_dxb else None
    nparts = lib.kalle_layernorm_bwd_parts(rows)
    before = _randn((1, D), g) if acc else None
    dsp = Guard(1 if acc else nparts, D, init=before)
    fn = lib.kalle_rmsnorm_bwd_acc if acc else lib.kalle_rmsnorm_bwd
    assert fn(P(dy), int(sf32), P(x), int(xf32), P(scale), ld, rpb, P(rr32), P(dx.v), P(dsp.v), P(dres), P(dxb.v) if dxb else None,
              rows, D, st) == 0
    torch.cuda.synchronize()
    rel = 0.5 * (D + 4) * U + ALLOW["RSQRT"] * U
    _check(rr.v[0], rrms, rel * rrms, what + " rrms", "RSQRT", rrms)
    _check(y.v, yr, yr.abs() * (rel + 3 * U + (0 if sf32 else BF16_REL)) + 1e-30, what + " y")
    y.clean(what + " y")
    rr.clean(what + " rrms")
    r32, dyd = rr32.double(), dy.double()
    dxr, dsr = kr.rmsnorm_bwd(dyd, xd, sd, r32, rpb, None if dres0 is None else dres0.double())
    if wrong == "dres_twice":
        dxr = dxr + dres0.double()
    srow = sd if sd.dim() == 1 else sd[torch.arange(rows, device="cuda") // rpb]
    dh = dyd * srow
    dc = (D + 8) * U * (dh * xd).abs().mean(-1, keepdim=True) * r32[:, None].pow(3)
    cc = ((dh * xd).mean(-1, keepdim=True) * r32[:, None].pow(3)).abs()
    tol = xd.abs() * dc + 4 * U * (dh.abs() * r32[:, None] + xd.abs() * cc) + (0 if dres0 is None else 2 * U * dres0.double().abs()) \
        + U * dxr.abs() + 1e-30
    if wrong in ("last_row", "last8"):
        prev = dres0.double() if dresm == "alias" else torch.zeros_like(dxr)
        dxr = dxr.clone()
        if wrong == "last_row":
            dxr[-1] = prev[-1]
        else:
            dxr[:, -8:] = prev[:, -8:]
    _check(dx.v, dxr, tol, what + " dx")
    dx.clean(what + " dx")
    if dxb:
        _exact(dxb.v, dx.v.bfloat16(), what + " dx_bf16 == bf16(dx)")
        dxb.clean(what + " dx_bf16")
    b0 = before[0].double() if acc else 0
    terms = (dyd * xd * r32[:, None]).abs().sum(0)
    _check(dsp.v.double().sum(0), dsr + b0, (rows + nparts + 4) * U * (terms + (before[0].double().abs() if acc else 0)) + 1e-30,
           what + " dscale")
    dsp.clean(what + " dscale")


@pytest.mark.parametrize("ci", range(len(RMS_CASES)))
def test_rmsnorm(kl, ci):
    run_rms(kl, RMS_CASES[ci], 300 + ci)


@pytest.mark.parametrize("ci", [1, 2, 3, 9])
@pytest.mark.parametrize("wrong", ["dres_twice", "last_row", "last8"])
def test_rms_wrong_reference_is_caught(kl, wrong, ci):
    with pytest.raises(AssertionError, match="out of bound"):
        run_rms(kl, RMS_CASES[ci], 350 + ci, wrong=wrong)


# ================================================================================================ head norm
@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("rows,null", [(5, "none"), (5, "dgamma"), (5, "dbeta"), (257, "both"), (11000, "none")])
def test_head_norm(kl, dh, mode, rows, null):
    """q slice of a fused [rows][3 heads dh] projection, y / dx into the k slice of other padded buffers; 11000 rows exceed both
    grid caps (4096 / 2048 workgroups).  mode 1: head (1, 0) is all zero - the clamp of F.normalize is active there and both
    directions follow x / max(||x||, 1e-12) (forward 0, backward g * 1e12).
    The forward's `stat` (mean | clamp flag, reciprocal std | reciprocal norm) is bounded like LayerNorm's row statistics and the
    clamp flag is asserted.  y and dx: the statistic's error (RSQRT in mode 2, DIV in mode 1) propagated as in run_ln, (dh + 8) u of
    the terms' magnitudes, one bf16 rounding."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    heads = 768 // dh if rows > 1000 else 3
    W = heads * dh
    ld = 3 * W
    g = _gen(900 + dh + mode + rows)
    what = f"head_norm dh {dh} mode {mode} rows {rows} null {null}"
    xb = torch.full((rows + 1, ld), NAN, device="cuda", dtype=torch.bfloat16)
    xb[:rows, W:2 * W] = (_randn((rows, W), g, 1.3) + 0.2).bfloat16()
    if mode == 1 and rows > 1:
        xb[1, W:W + dh] = 0
    gb = torch.full((rows + 1, ld), NAN, device="cuda", dtype=torch.bfloat16)
    gb[:rows, :W] = _randn((rows, W), g).bfloat16()
    gam = _nan_tail(1 + 0.2 * _randn((dh,), g), 8) if mode == 2 else None
    bet = _nan_tail(0.1 * _randn((dh,), g), 8) if mode == 2 else None
    y = torch.full((rows + 1, ld), NAN, device="cuda", dtype=torch.bfloat16)
    stat = Guard(rows, heads * 2)
    assert lib.kalle_head_norm_fwd_hd(P(xb), ld, W, P(y), ld, 2 * W, P(stat.v), P(gam), P(bet), mode, rows, heads, dh, st) == 0
    dxo = torch.full((rows + 1, ld), NAN, device="cuda", dtype=torch.bfloat16)
    bg, bb = _randn((1, dh), g), _randn((1, dh), g)
    dga = Guard(1, dh, init=bg) if mode == 2 and null not in ("dgamma", "both") else None
    dbe = Guard(1, dh, init=bb) if mode == 2 and null not in ("dbeta", "both") else None
    assert lib.kalle_head_norm_bwd_hd(P(xb), ld, W, P(stat.v), P(gb), ld, 0, P(dxo), ld, 2 * W, P(gam), P(dga.v) if dga else None,
                                      P(dbe.v) if dbe else None, mode, rows, heads, dh, st) == 0
    torch.cuda.synchronize()
    xh = xb[:rows, W:2 * W].double().view(rows, heads, dh)
    gh = gb[:rows, :W].double().view(rows, heads, dh)
    gd, bd = (gam.double(), bet.double()) if mode == 2 else (None, None)
    allow = ALLOW["DIV"] if mode == 1 else ALLOW["RSQRT"]
    yr = kr.head_norm_fwd(xh, mode, gd, bd)
    st_ = stat.v.double().view(rows, heads, 2)
    m1 = xh.abs().mean(-1, keepdim=True)
    if mode == 1:
        # stat = (clamp flag, 1 / max(||x||, 1e-12)): the norm is a dh-term sum under a square root
        nrm = xh.pow(2).sum(-1, keepdim=True).sqrt()
        rs = 1 / nrm.clamp_min(1e-12)
        drs_rel = 0.5 * (dh + 2) * U + allow * U
        assert (st_[..., 0] == (nrm[..., 0] <= 1e-12).double()).all(), what + " clamp flag"
        if rows > 1:
            assert st_[1, 0, 0].item() == 1.0 and int(st_[..., 0].sum()) == 1, what + " clamp flag of the all-zero head"
        _check(st_[..., 1], rs[..., 0], drs_rel * rs[..., 0], what + " stat: reciprocal norm", "DIV", rs[..., 0])
        ytol = (drs_rel + 2 * U) * yr.abs()
    else:
        # stat = (mean, rstd), bounded as LayerNorm's row statistics
        mu = xh.mean(-1, keepdim=True)
        var_e = (xh - mu).pow(2).mean(-1, keepdim=True) + 1e-6
        rs = var_e.rsqrt()
        dmu = (dh + 2) * U * m1
        drs_rel = 0.5 * ((dh + 4) * U + 4 * dmu.pow(2) / var_e) + allow * U
        _check(st_[..., 0], mu[..., 0], (dmu + U * mu.abs())[..., 0], what + " stat: mean")
        _check(st_[..., 1], rs[..., 0], (drs_rel * rs)[..., 0], what + " stat: rstd", "RSQRT", rs[..., 0])
        xhat = (xh - mu) * rs
        ytol = gd.abs() * (rs * (dmu + 2 * U * (xh.abs() + mu.abs())) + xhat.abs() * drs_rel) + 4 * U * ((xhat * gd).abs() + bd.abs())
    _check(y[:rows, 2 * W:].double().view(rows, -1), yr.view(rows, -1), (ytol + BF16_REL * yr.abs()).view(rows, -1) + 1e-30, what + " y")
    mask = torch.ones_like(y, dtype=torch.bool)
    mask[:rows, 2 * W:] = False
    assert torch.isnan(y[mask]).all() and torch.isnan(dxo[mask]).all(), what + " stray writes"
    stat.clean(what + " stat")
    # backward: the kernel reads the statistics its forward saved; their error (drs_rel, dmu) enters every element of the head
    dxr, dgr, dbr = kr.head_norm_bwd(xh, gh, mode, gd)
    if mode == 1:
        yy = xh * rs
        dot_abs = (yy * gh).abs().sum(-1, keepdim=True)
        terms = rs * (gh.abs() + yy.abs() * dot_abs)                      # |rs g| + |rs y <y, g>|
        tol = ((dh + 8) * U + 3 * drs_rel) * terms + BF16_REL * dxr.abs() + 1e-30
    else:
        dhh = gh * gd
        c1a, c2 = dhh.abs().mean(-1, keepdim=True), (dhh * xhat).mean(-1, keepdim=True)
        c2a = (dhh * xhat).abs().mean(-1, keepdim=True)
        exh = rs * (dmu + 3 * U * (xh.abs() + mu.abs())) + xhat.abs() * drs_rel           # error of xhat as the backward rebuilds it
        terms = rs * (dhh.abs() + c1a + xhat.abs() * c2a)
        tol = ((dh + 8) * U + drs_rel) * terms + rs * (c2.abs() * exh + xhat.abs() * (dhh.abs() * exh).mean(-1, keepdim=True)) \
            + BF16_REL * dxr.abs() + 1e-30
    _check(dxo[:rows, 2 * W:].double().view(rows, -1), dxr.view(rows, -1), tol.view(rows, -1), what + " dx")
    if mode == 1 and rows > 1:
        assert (y[1, 2 * W:2 * W + dh] == 0).all()
        # (the clamped head's backward, g * 1e12, is part of the bound above: kr.head_norm_bwd takes that branch)
    if mode == 2:
        nn_ = rows * heads + 8
        for buf, before, ref, terms_, prop, name in ((dga, bg, dgr, (gh * xhat).abs().sum((0, 1)), (gh.abs() * exh).sum((0, 1)), "dgamma"),
                                                     (dbe, bb, dbr, gh.abs().sum((0, 1)), 0, "dbeta")):
            if buf is None:
                continue
            _check(buf.v[0], ref + before[0].double(), nn_ * U * (terms_ + before[0].double().abs()) + prop + 1e-30, what + " " + name)
            buf.clean(what + " " + name)


def test_head_norm_dh64_entry_points(kl):
    """kalle_head_norm_fwd / _bwd forward to the _hd forms at head_dim 64: same bits in y, stat, dx, dgamma, dbeta"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    rows, heads, dh = 37, 3, 64
    W = heads * dh
    g = _gen(64)
    x, gr = (_randn((rows, W), g, 1.3) + 0.2).bfloat16(), _randn((rows, W), g).bfloat16()
    gam, bet = 1 + 0.2 * _randn((dh,), g), 0.1 * _randn((dh,), g)
    for mode in (1, 2):
        outs = []
        for hd in (False, True):
            y, dx, stat = Guard(rows, W, dtype=torch.bfloat16), Guard(rows, W, dtype=torch.bfloat16), Guard(rows, 2 * heads)
            dga, dbe = Guard(1, dh, init=torch.ones((1, dh), device="cuda")), Guard(1, dh, init=torch.ones((1, dh), device="cuda"))
            fa = (P(x), W, 0, P(y.v), W, 0, P(stat.v), P(gam), P(bet), mode, rows, heads)
            assert (lib.kalle_head_norm_fwd_hd(*fa, 64, st) if hd else lib.kalle_head_norm_fwd(*fa, st)) == 0
            ba = (P(x), W, 0, P(stat.v), P(gr), W, 0, P(dx.v), W, 0, P(gam), P(dga.v), P(dbe.v), mode, rows, heads)
            assert (lib.kalle_head_norm_bwd_hd(*ba, 64, st) if hd else lib.kalle_head_norm_bwd(*ba, st)) == 0
            torch.cuda.synchronize()
            for b in (y, dx, stat, dga, dbe):
                b.clean("head norm dh 64")
            outs.append((y.v.clone(), stat.v.clone(), dx.v.clone()))
        for a, b, name in zip(outs[0], outs[1], ("y", "stat", "dx")):
            _exact(a, b, f"head norm dh 64 mode {mode} {name}")
    y = Guard(rows, W, dtype=torch.bfloat16)
    assert lib.kalle_head_norm_fwd(P(x), W, 4, P(y.v), W, 0, P(stat.v), P(gam), P(bet), 2, rows, heads, st) == ERR_ARG
    assert lib.kalle_head_norm_bwd(P(x), W, 0, P(stat.v), P(gr), W, 0, P(y.v), W, 0, None, None, None, 2, rows, heads, st) == ERR_ARG
    torch.cuda.synchronize()
    y.untouched("head norm dh 64")


def test_head_norm_rejects(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    x = torch.zeros((4, 256), device="cuda", dtype=torch.bfloat16)
    gam = torch.ones(128, device="cuda")
    y, stat = Guard(4, 256, dtype=torch.bfloat16), Guard(4, 8)
    f, b = lib.kalle_head_norm_fwd_hd, lib.kalle_head_norm_bwd_hd
    for kw in (dict(dh=48), dict(mode=3), dict(mode=2, gamma=None), dict(ld=252), dict(ld=64), dict(off=4), dict(off=-8),
               dict(rows=0), dict(heads=0)):
        a = dict(dh=64, mode=2, gamma=gam, ld=256, off=0, rows=4, heads=2)
        a.update(kw)
        assert f(P(x), a["ld"], a["off"], P(y.v), 256, 0, P(stat.v), P(a["gamma"]), None, a["mode"], a["rows"], a["heads"], a["dh"],
                 st) == ERR_ARG, kw
        assert b(P(x), a["ld"], a["off"], P(stat.v), P(x), 256, 0, P(y.v), 256, 0, P(a["gamma"]), None, None, a["mode"], a["rows"],
                 a["heads"], a["dh"], st) == ERR_ARG, kw
    torch.cuda.synchronize()
    y.untouched("head norm")
    stat.untouched("head norm stat")


def test_colsum_small(kl):
    """rows = 1, cols = 2, padded ld, accumulate on / off, fp32 and bf16; out[cols:] stays NaN"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(5)
    for dt, accum, (rows, cols) in itertools.product((torch.float32, torch.bfloat16), (0, 1), ((1, 2), (37, 130))):
        src = torch.full((rows + 1, cols + 6), NAN, device="cuda", dtype=dt)
        src[:rows, :cols] = _randn((rows, cols), g).to(dt)
        before = _randn((1, cols), g)
        out = Guard(1, cols, init=before)
        assert lib.kalle_colsum(P(src), int(dt == torch.float32), cols + 6, P(out.v), rows, cols, accum, st) == 0
        torch.cuda.synchronize()
        s = src[:rows, :cols].double()
        b0 = before[0].double() * accum
        _check(out.v[0], s.sum(0) + b0, (rows + 8) * U * (s.abs().sum(0) + b0.abs()) + 1e-30, f"colsum {dt} {accum} {rows}x{cols}")
        out.clean("colsum")


# ================================================================================================ SwiGLU / SiLU / GELU
EDGE = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 6.0, -6.0, 20.0, -20.0, 90.0, -90.0]


def _with_edges(t):
    """random values with the edge values written over the head of the flattened tensor (as far as they fit)"""
    f = t.reshape(-1)
    e = torch.tensor(EDGE, device="cuda", dtype=t.dtype)[:f.numel()]
    f[:e.numel()] = e
    return t


def run_swiglu(kl, rows, inner, dbias_on, seed, wrong=None):
    """fwd: x silu(g): (SIGMOID + 4) u |x| |g| ... relative to the terms, + one bf16 rounding.  bwd: dh_x = d g s, dh_g = d x s (1 + g (1 - s)):
    (SIGMOID + 6) u |d| (|g| | |x| (1 + |g|)) + one bf16 rounding; dbias += column sums of the ROUNDED dh (fp32 sum bound)."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(seed)
    what = f"swiglu {rows}x{inner} dbias {dbias_on}"
    hv = _randn((rows, 2 * inner), g, 2.0)
    hv[:, inner:] = _with_edges(hv[:, inner:].contiguous())
    h = _nan_tail(hv.bfloat16())
    out = Guard(rows, inner, dtype=torch.bfloat16)
    assert lib.kalle_swiglu_fwd(P(h), P(out.v), rows, inner, st) == 0
    do = _nan_tail(_randn((rows, inner), g).bfloat16())
    dh = Guard(rows, 2 * inner, dtype=torch.bfloat16)
    before = _randn((1, 2 * inner), g)
    db = Guard(1, 2 * inner, init=before) if dbias_on else None
    assert lib.kalle_swiglu_bwd(P(do), P(h), P(dh.v), P(db.v) if db else None, rows, inner, st) == 0
    torch.cuda.synchronize()
    hd, dd = h.double(), do.double()
    x_, g_ = hd[:, :inner], hd[:, inner:]
    ref = kr.swiglu_fwd(hd)
    _check(out.v, ref, (ALLOW["SIGMOID"] + 4) * U * (x_ * g_).abs() + BF16_REL * ref.abs() + 1e-38, what + " fwd")
    out.clean(what)
    dref = kr.swiglu_bwd(dd, hd)
    mag = torch.cat([(dd * g_).abs(), (dd * x_).abs() * (1 + g_.abs())], 1)
    if wrong == "last_row":
        dref = dref.clone()
        dref[-1] = 0
    if wrong == "last8":
        dref = dref.clone()
        dref[:, -8:] = 0
    _check(dh.v, dref, (ALLOW["SIGMOID"] + 6) * U * mag + BF16_REL * dref.abs() + 1e-38, what + " bwd")
    dh.clean(what)
    if db:
        r = dh.v.double()
        _check(db.v[0], r.sum(0) + before[0].double(), (rows + 8) * U * (r.abs().sum(0) + before[0].double().abs()) + 1e-30,
               what + " dbias")
        db.clean(what)


@pytest.mark.parametrize("inner", [8, 136, 512, 1544])
@pytest.mark.parametrize("rows", [1, 5, 37, 4100])
def test_swiglu(kl, rows, inner):
    run_swiglu(kl, rows, inner, (rows + inner // 8) % 2 == 0, rows + inner)


@pytest.mark.parametrize("rows,inner", [(5, 136), (4100, 512)])
@pytest.mark.parametrize("wrong", ["last_row", "last8"])
def test_swiglu_wrong_reference_is_caught(kl, wrong, rows, inner):
    with pytest.raises(AssertionError, match="out of bound"):
        run_swiglu(kl, rows, inner, True, 3, wrong=wrong)


@pytest.mark.parametrize("n", [1, 7, 255, 257, 2048 * 256 + 3])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("op", ["silu", "gelu"])
def test_silu_gelu(kl, op, dt, n):
    """silu = x s(x): (A + 3) u |x|; silu' = d s (1 + x (1 - s)): (A + 4) u |d| (1 + |x|)  - 1 - s is a difference of numbers near 1;
    gelu = 0.5 x (1 + erf): (A + 3) u |x|; gelu' = d (Phi + x phi): (A + 4) u |d| (1 + |x|).  bf16: + one rounding."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(n % 1000 + len(op))
    x = _nan_tail(_with_edges(_randn((n,), g, 3.0)).to(dt), 8)
    dy = _nan_tail(_randn((n,), g).to(dt), 8)
    y, dx = Guard(1, n, dtype=dt, extra=1), Guard(1, n, dtype=dt, extra=1)
    fwd, bwd = (lib.kalle_silu_fwd, lib.kalle_silu_bwd) if op == "silu" else (lib.kalle_gelu_fwd, lib.kalle_gelu_bwd)
    code = int(dt == torch.float32)
    assert fwd(P(x), P(y.v), code, n, st) == 0
    assert bwd(P(dy), P(x), P(dx.v), code, n, st) == 0
    torch.cuda.synchronize()
    xd, dd = x.double(), dy.double()
    key = "SIGMOID" if op == "silu" else "ERF"
    rf = (kr.silu_fwd if op == "silu" else kr.gelu_fwd)(xd)
    rb = (kr.silu_bwd if op == "silu" else kr.gelu_bwd)(dd, xd)
    rnd = 0 if dt == torch.float32 else BF16_REL
    meas = key if dt == torch.float32 else None
    _check(y.v[0], rf, (ALLOW[key] + 3) * U * xd.abs() + rnd * rf.abs() + 1e-44, f"{op} fwd {dt} n {n}", meas, xd.abs())
    _check(dx.v[0], rb, (ALLOW[key] + 4) * U * dd.abs() * (1 + xd.abs()) + rnd * rb.abs() + 1e-44, f"{op} bwd {dt} n {n}", meas,
           dd.abs() * (1 + xd.abs()))
    y.clean(op)
    dx.clean(op)


# ================================================================================================ cast / transpose / copies
def _all_bf16():
    return torch.arange(65536, device="cuda", dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def test_cast_exhaustive(kl):
    """all 65 536 bf16 patterns -> fp32 -> bf16 is the identity; fp32 -> bf16 equals torch's rounding bit for bit on, for every
    finite bf16 value: the value, the midpoint to its successor (the tie) and the floats one ulp either side of the midpoint"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    pat = _all_bf16()
    f = Guard(1, 65536)
    assert lib.kalle_cast(P(pat), BF16, P(f.v), F32, 65536, st) == 0
    back = Guard(1, 65536, dtype=torch.bfloat16)
    assert lib.kalle_cast(P(f.v), F32, P(back.v), BF16, 65536, st) == 0
    torch.cuda.synchronize()
    _exact(f.v[0], pat.float(), "bf16 -> fp32")
    _exact(back.v[0], pat, "bf16 -> fp32 -> bf16")
    fin = pat[torch.isfinite(pat.float())]
    base = fin.float().view(torch.int32)
    src = torch.stack([base, base + 0x8000, base + 0x7fff, base + 0x8001], 1).reshape(-1).view(torch.float32).contiguous()
    n = src.numel()
    assert n % 2 == 0 and n > 4 * 65000
    src = src[:n - 1]                                # (odd n)
    out = Guard(1, n - 1, dtype=torch.bfloat16)
    assert lib.kalle_cast(P(src), F32, P(out.v), BF16, n - 1, st) == 0
    torch.cuda.synchronize()
    _exact(out.v[0], src.bfloat16(), "fp32 -> bf16 ties and neighbours")
    out.clean("cast")
    f.clean("cast")
    for a, b in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
        s = _randn((777,), _gen(1)).to(a)
        o = Guard(1, 777, dtype=b)
        assert lib.kalle_cast(P(s), int(a == torch.float32), P(o.v), int(b == torch.float32), 777, st) == 0
        torch.cuda.synchronize()
        _exact(o.v[0], s, "cast same type")
        o.clean("cast")
    o = Guard(1, 8)
    assert lib.kalle_cast(None, F32, P(o.v), F32, 8, st) == ERR_ARG and lib.kalle_cast(P(s), F32, P(o.v), F32, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    o.untouched("cast")


DT = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("R,Cn", [(1, 1), (31, 33), (33, 31), (50, 40), (215, 64)])
@pytest.mark.parametrize("idt,odt", list(itertools.product(DT, DT)), ids=["ff", "fb", "bf", "bb"])
def test_transpose(kl, R, Cn, idt, odt):
    """bit-exact except fp32 -> bf16, which is torch's rounding bit for bit; padded lds, batch strides larger than a matrix"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    B, in_ld, out_ld = 3, Cn + 3, R + 5
    in_bs, out_bs = R * in_ld + 7, Cn * out_ld + 9
    src = torch.full((B, in_bs), NAN, device="cuda", dtype=idt)
    vals = _randn((B, R, Cn), _gen(R * Cn)).to(idt)
    _win(src, B, R, in_ld, Cn)[:] = vals
    dst = torch.full((B + 1, out_bs), NAN, device="cuda", dtype=odt)
    assert lib.kalle_transpose_2d(P(src), int(idt == torch.float32), in_bs, in_ld, P(dst), int(odt == torch.float32), out_bs, out_ld,
                                  B, R, Cn, st) == 0
    torch.cuda.synchronize()
    _exact(_win(dst, B, Cn, out_ld, R).contiguous(), kr.transpose_2d(vals).to(odt).contiguous(), "transpose")
    assert torch.isnan(dst[_outside(dst, B, Cn, out_ld, R)]).all()


@pytest.mark.parametrize("idt,odt", list(itertools.product(DT, DT)), ids=["ff", "fb", "bf", "bb"])
@pytest.mark.parametrize("cols,accum", [(4, 0), (132, 0), (4, 1), (132, 1)])
def test_copy_rows(kl, idt, odt, cols, accum):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    B, rows, in_ld, out_ld = 3, 5, cols + 8, cols + 4
    in_bs, out_bs = rows * in_ld + 12, rows * out_ld + 8
    g = _gen(cols + accum)
    src = torch.full((B, in_bs), NAN, device="cuda", dtype=idt)
    vals = _randn((B, rows, cols), g).to(idt)
    _win(src, B, rows, in_ld, cols)[:] = vals
    dst = torch.full((B + 1, out_bs), NAN, device="cuda", dtype=odt)
    before = _randn((B, rows, cols), g).to(odt)
    win = _win(dst, B, rows, out_ld, cols)
    if accum:
        win[:] = before
    rc = lib.kalle_copy_rows(P(src), int(idt == torch.float32), in_bs, in_ld, P(dst), int(odt == torch.float32), out_bs, out_ld, B, rows,
                             cols, accum, st)
    torch.cuda.synchronize()
    if accum and odt == torch.bfloat16:
        assert rc == ERR_ARG
        _exact(win.contiguous(), before, "rejected call left the output alone")
        return
    assert rc == 0
    if accum:
        _exact(win.contiguous(), before + vals.float(), "copy_rows accumulate (one fp32 add: exact rounding)")
    else:
        _exact(win.contiguous(), vals.to(odt), "copy_rows")
    assert torch.isnan(dst[_outside(dst, B, rows, out_ld, cols)]).all()
    for bad in (dict(cols=6), dict(in_ld=in_ld + 2), dict(out_bs=out_bs + 2)):
        a = dict(cols=cols, in_ld=in_ld, out_bs=out_bs)
        a.update(bad)
        chk = dst.clone()
        assert lib.kalle_copy_rows(P(src), int(idt == torch.float32), in_bs, a["in_ld"], P(dst), int(odt == torch.float32), a["out_bs"],
                                   out_ld, B, rows, a["cols"], 0, st) == ERR_ARG
        torch.cuda.synchronize()
        _exact(dst, chk, "rejected copy_rows")


@pytest.mark.parametrize("dt", DT, ids=["f32", "bf16"])
def test_segment_copy(kl, dt):
    """64 segments whose source / destination offsets fall on and off the 16-byte grid (vector path, its tail, scalar path),
    lengths 0, 1, vector multiples and not; bit-exact, nothing else written; 65 segments / a negative offset: KALLE_ERR_ARG"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    nseg, nb, rows = 64, 2, 3
    V = 4 if dt == torch.float32 else 8
    lens = [(0, 1, V, V + 1, 3 * V, 5 * V + 3, 100, 1031)[s % 8] for s in range(nseg)]
    so = [(s % 4) * V if s % 3 else (s % 4) * V + 1 + s % 5 for s in range(nseg)]          # aligned | unaligned sources
    do = [0 if s % 2 else 1 + s % 3 for s in range(nseg)]                                  # aligned | unaligned destinations
    src_ld, dst_ld = 1104, 1048
    src_bs, dst_bs = rows * src_ld + 16, rows * dst_ld + 8
    src_ss, dst_ss = nb * src_bs + 32, nb * dst_bs + 24
    src = _randn((nseg * src_ss,), _gen(4)).to(dt)
    dst = torch.full((nseg * dst_ss + 16,), NAN, device="cuda", dtype=dt)
    ca = lambda t, v: (t * len(v))(*v)
    args = lambda n, so_, do_: (P(src), P(dst), int(dt == torch.float32), n, ca(ctypes.c_int64, so_), ca(ctypes.c_int64, do_),
                                ca(ctypes.c_int, lens[:1] * (n - nseg) + lens if n > nseg else lens[:n]), nb, rows, src_ss, src_bs,
                                src_ld, dst_ss, dst_bs, dst_ld, st)
    assert lib.kalle_segment_copy(*args(65, so + [0], do + [0])) == ERR_ARG
    assert lib.kalle_segment_copy(*args(64, [-1] + so[1:], do)) == ERR_ARG
    assert lib.kalle_segment_copy(*args(64, so, do[:-1] + [-8])) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()
    assert lib.kalle_segment_copy(*args(64, so, do)) == 0
    torch.cuda.synchronize()
    ref = torch.full_like(dst, NAN)
    for s, b, c in itertools.product(range(nseg), range(nb), range(rows)):
        d0 = s * dst_ss + b * dst_bs + c * dst_ld + do[s]
        s0 = s * src_ss + b * src_bs + c * src_ld + so[s]
        ref[d0:d0 + lens[s]] = src[s0:s0 + lens[s]]
    _exact(dst, ref, "segment_copy")


# ================================================================================================ diffuse / MSE / Fourier / Adam
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("B,per", [(4, 7), (5, 2048 * 256 // 4 + 33)])
def test_diffuse(kl, objective, B, per):
    """x_t = a x + s n, target = a n - s x | n - x; t = 0 and t = 1 exactly among the batch.
    bound: (SINCOS (objective 0) + 4) u (|x| + |n|) (a, s <= 1; the angle pi t / 2 <= 1.6 carries 2 u of its own)"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(B + per)
    x, n = _nan_tail(_randn((B, per), g)), _nan_tail(_randn((B, per), g))
    t = torch.rand(B, generator=g, device="cuda")
    t[0], t[1] = 0.0, 1.0
    t = _nan_tail(t, 4)
    xt, tg = Guard(B, per), Guard(B, per)
    assert lib.kalle_diffuse_fwd(P(x), P(n), P(t), P(xt.v), P(tg.v), B, per, objective, st) == 0
    torch.cuda.synchronize()
    rx, rt = kr.diffuse_fwd(x.double(), n.double(), t.double(), objective)
    unit = x.double().abs() + n.double().abs()
    a = (ALLOW["SINCOS"] * 3 if objective == 0 else 0) + 4
    _check(xt.v, rx, a * U * unit + 1e-30, f"diffuse {objective} x_t", "SINCOS" if objective == 0 else None, 3 * unit)
    _check(tg.v, rt, a * U * unit + 1e-30, f"diffuse {objective} target", "SINCOS" if objective == 0 else None, 3 * unit)
    xt.clean("x_t")
    tg.clean("target")
    xt, tg = Guard(B, per), Guard(B, per)
    assert lib.kalle_diffuse_fwd(P(x), P(n), P(t), P(xt.v), P(tg.v), B, per, 2, st) == ERR_ARG
    assert lib.kalle_diffuse_fwd(P(x), P(n), None, P(xt.v), P(tg.v), B, per, 0, st) == ERR_ARG
    assert lib.kalle_diffuse_fwd(P(x), P(n), P(t), P(xt.v), P(tg.v), 0, per, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    xt.untouched("diffuse x_t")
    tg.untouched("diffuse target")


@pytest.mark.parametrize("mask_kind", ["none", "ones", "empties_one"])
@pytest.mark.parametrize("B,C,T,weight,with_diff", [(3, 4, 7, 1.0, True), (5, 64, 215, 0.37, True), (2, 3, 1001, 2.5, False),
                                                    (3, 8, 12001, 1.0, True)])
def test_mse(kl, mask_kind, B, C, T, weight, with_diff):
    """loss_acc += {sum of squares, count}: the accumulator starts from a random sum and a random integer count and is checked as
    before + ref (the count exactly); kalle_mse_finish then works on that accumulator: loss = w acc[0] / acc[1], diff *= 2 w / acc[1].
    3 x 8 x 12001 elements exceed the 1024-workgroup cap (the grid-stride loop).
    bound: sums (n + 8) u (sum|terms| + |before|); element-wise 3 u; the finish adds (DIV + 4) u of the quotient."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(B * C + T)
    o, tg = _nan_tail(_randn((B, C, T), g)), _nan_tail(_randn((B, C, T), g))
    mask = None
    if mask_kind != "none":
        mask = torch.ones((B, T), device="cuda", dtype=torch.uint8)
        if mask_kind == "empties_one":
            mask = (torch.rand((B, T), generator=g, device="cuda") > 0.3).to(torch.uint8)
            mask[1] = 0
            mask[0, 0] = 1
    n = B * C * T
    before = torch.tensor([[3.25 + T, 17.0 + B]], device="cuda")
    bs, bc = before[0, 0].double(), before[0, 1].double()
    results = []
    for mk in ([None, mask] if mask_kind == "ones" else [mask]):
        acc = Guard(1, 2, init=before)
        diff = Guard(1, n) if with_diff else None
        loss = Guard(1, 1)
        assert lib.kalle_mse_fwd(P(o), P(tg), P(mk), P(acc.v), P(diff.v) if diff else None, B, C, T, st) == 0
        torch.cuda.synchronize()
        acc0 = acc.v.clone()
        assert lib.kalle_mse_finish(P(acc.v), P(loss.v), P(diff.v) if diff else None, n, weight, st) == 0
        torch.cuda.synchronize()
        ssq, cnt, _, _ = kr.mse(o.double(), tg.double(), mk, weight)
        _check(acc0[0, :1], (ssq + bs).reshape(1), (n + 8) * U * (ssq + bs).reshape(1), "mse loss_acc[0] = before + sum")
        assert acc0[0, 1].item() == (cnt + bc).item(), "mse loss_acc[1] = before + count"
        _exact(acc.v, acc0, "kalle_mse_finish leaves loss_acc alone")
        # the finish sees the accumulator as it stands: the reference is built from the same two numbers
        a0, a1 = acc0[0, 0].double(), acc0[0, 1].double()
        _check(loss.v[0], (weight * a0 / a1).reshape(1), (ALLOW["DIV"] + 4) * U * (weight * a0 / a1).abs().reshape(1), "mse loss")
        if diff:
            d = o.double() - tg.double()
            if mk is not None:
                d = d * (mk != 0).double()[:, None, :]
            unit = (2 * weight * (o.double().abs() + tg.double().abs()) / a1).reshape(-1)
            _check(diff.v[0], (2 * weight * d / a1).reshape(-1), (ALLOW["DIV"] + 6) * U * unit + 1e-38, "mse dout", "DIV", unit)
            diff.clean("mse diff")
        acc.clean("mse acc")
        loss.clean("mse loss")
        results.append((acc0.clone(), loss.v.clone(), None if diff is None else diff.v.clone()))
    if mask_kind == "ones":           # an all-ones mask is no mask: the element-wise part bit for bit, the count exactly
        if with_diff:
            _exact(results[0][2], results[1][2], "all-ones mask == no mask (dout)")
        assert results[0][0][0, 1].item() == results[1][0][0, 1].item()
    acc = Guard(1, 2)
    assert lib.kalle_mse_fwd(P(o), None, None, P(acc.v), None, B, C, T, st) == ERR_ARG
    assert lib.kalle_mse_fwd(P(o), P(tg), None, P(acc.v), None, B, 0, T, st) == ERR_ARG
    assert lib.kalle_mse_finish(None, None, None, n, weight, st) == ERR_ARG
    torch.cuda.synchronize()
    acc.untouched("mse")


@pytest.mark.parametrize("nb", [1, 5, 256])
@pytest.mark.parametrize("half", [1, 128, 130])
def test_fourier(kl, nb, half):
    """f = 2 pi t w, |f| up to ~30, computed in fp32 (2 roundings: 2 u |f| of angle) -> |cos / sin - ref| <= (SINCOS + 3) u (1 + |f|);
    bf16 out + one rounding.  bwd: dw[j] = sum_b k (ds cos - dc sin): (nb + 4) u sum|terms| + the same per-term angle error."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(nb * half)
    t = _nan_tail(torch.rand(nb, generator=g, device="cuda"), 4)
    w = _nan_tail(_randn((half,), g, 1.6), 4)
    td, wd = t.double(), w.double()
    # the kernel's angle is the fp32 product; the reference takes the exact product of the same fp32 operands
    ref = kr.fourier_features(td, wd)
    f = (2 * math.pi * td[:, None] * wd[None, :]).abs()
    unit = torch.cat([1 + f, 1 + f], 1)
    for odt in DT:
        out = Guard(nb, 2 * half, dtype=odt)
        assert lib.kalle_fourier_features(P(t), P(w), P(out.v), int(odt == torch.float32), nb, half, st) == 0
        torch.cuda.synchronize()
        _check(out.v, ref, (ALLOW["SINCOS"] + 3) * U * unit + (0 if odt == torch.float32 else BF16_REL * ref.abs()),
               f"fourier {nb}x{half} {odt}", "SINCOS" if odt == torch.float32 else None, unit)
        out.clean("fourier")
    do = _nan_tail(_randn((nb, 2 * half), g))
    dw = Guard(1, half)
    assert lib.kalle_fourier_features_bwd(P(do), P(t), P(w), P(dw.v), nb, half, st) == 0
    torch.cuda.synchronize()
    dd = do.double()
    k = (2 * math.pi * td[:, None]).abs()
    terms = (k * (dd[:, half:].abs() + dd[:, :half].abs()) * (1 + f)).sum(0)
    _check(dw.v[0], kr.fourier_features_bwd(dd, td, wd), ((nb + 4) + ALLOW["SINCOS"] + 3) * U * terms + 1e-30, f"fourier bwd {nb}x{half}")
    dw.clean("fourier bwd")
    out, dw = Guard(nb, 2 * half), Guard(1, half)
    assert lib.kalle_fourier_features(P(t), None, P(out.v), F32, nb, half, st) == ERR_ARG
    assert lib.kalle_fourier_features(P(t), P(w), P(out.v), F32, nb, 0, st) == ERR_ARG
    assert lib.kalle_fourier_features_bwd(P(do), None, P(w), P(dw.v), nb, half, st) == ERR_ARG
    assert lib.kalle_fourier_features_bwd(P(do), P(t), P(w), P(dw.v), 0, half, st) == ERR_ARG
    torch.cuda.synchronize()
    out.untouched("fourier")
    dw.untouched("fourier bwd")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


def run_adam(kl, n, step, decoupled, with_bf16, seed, wrong=None):
    """m' = b1 m + (1 - b1) g', v' = b2 v + (1 - b2) g'^2, p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / bc2 + eps); the reference takes
    the hyper-parameters as the float ABI passes them.  bounds: m': 4 u (|m| + |g'|), v': 6 u (|v| + g'^2) (see below); p': 3 u |p| + R u |update|,
    R = 8 + DIV + 2 b1^t / (1 - b1^t) + b2^t / (1 - b2^t) (bias corrections are fp32 differences on the host) + what dm', dv' carry."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(seed)
    hp = dict(lr=_f32(1e-2), beta1=_f32(0.9), beta2=_f32(0.999), eps=_f32(1e-8), weight_decay=_f32(0.1))
    gs = _f32(0.25)
    p0, gr = _randn((n,), g), _randn((n,), g, 3.0)
    m0, v0 = _randn((n,), g, 0.3), _randn((n,), g).pow(2) * 0.1
    bufs = [Guard(1, n, init=t[None], extra=1) for t in (p0, m0, v0)]
    pb = Guard(1, n, dtype=torch.bfloat16, extra=1) if with_bf16 else None
    grad = _nan_tail(gr, 8)
    assert lib.kalle_adam_step(P(bufs[0].v), P(grad), P(bufs[1].v), P(bufs[2].v), P(pb.v) if pb else None, n, hp["lr"], hp["beta1"],
                               hp["beta2"], hp["eps"], hp["weight_decay"], int(decoupled), step, gs, st) == 0
    torch.cuda.synchronize()
    pr, mr, vr = kr.adam_step(p0.double(), gr.double(), m0.double(), v0.double(), decoupled=decoupled, step=step, grad_scale=gs,
                              decay_after=(wrong == "decay_after"), **hp)
    b1, b2, lr, wd = hp["beta1"], hp["beta2"], hp["lr"], hp["weight_decay"]
    gq = gr.double().abs() * gs + (0 if decoupled else wd * p0.double().abs())
    # -ffast-math lets the compiler evaluate b m + (1 - b) g in any algebraically equal form, and it does: the gfx950 code of
    # adam_kernel is m' = fma(b1, m - g, g), v' = fma(b2, v - g g, g g).  The moments are therefore bounded in their OPERANDS, not
    # in the terms of the written form (at beta2 = 0.999 the two differ by 1000 x)
    dm = 4 * U * (m0.double().abs() + gq)
    dv = 6 * U * (v0.double().abs() + gq * gq)
    what = f"adam n {n} step {step} decoupled {decoupled}"
    _check(bufs[1].v[0], mr, dm + 1e-38, what + " m")
    _check(bufs[2].v[0], vr, dv + 1e-38, what + " v")
    bc1, bc2 = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    denom = vr.sqrt() / bc2 + hp["eps"]
    upd = (lr / bc1) * mr.abs() / denom
    R = 8 + ALLOW["DIV"] + 2 * b1 ** step / bc1 + b2 ** step / bc2 ** 2
    tol = 3 * U * p0.double().abs() + R * U * upd + (lr / bc1) * (dm / denom + mr.abs() / denom.pow(2) * dv / (2 * vr.sqrt() * bc2 + 1e-300))
    # (not a place to MEASURE the division: where g' = g s + wd p cancels and v is tiny, sqrt(v') is ill-conditioned and the
    # deviation is the propagated dv, not the intrinsic's)
    _check(bufs[0].v[0], pr, tol + 1e-38, what + " p")
    for b in bufs:
        b.clean(what)
    if pb:
        _exact(pb.v, bufs[0].v.bfloat16(), what + " param_bf16 == bf16(param)")
        pb.clean(what)


@pytest.mark.parametrize("n", [1, 2, 3, 1003, 4 * 2048 * 256 + 5])
@pytest.mark.parametrize("step", [1, 2, 10000])
@pytest.mark.parametrize("decoupled", [False, True])
def test_adam(kl, n, step, decoupled):
    run_adam(kl, n, step, decoupled, (n + step) % 2 == 0, n % 997 + step)


def test_adam_grid_stride(kl):
    """above 16384 workgroups x 256 threads x 4 elements the kernel's grid-stride loop repeats (and the n % 4 tail follows it)"""
    run_adam(kl, 16384 * 1024 + 4 * 1000 + 3, 7, True, True, 21)


@pytest.mark.parametrize("n,step", [(3, 1), (1003, 2), (1003, 10000)])
def test_adam_wrong_reference_is_caught(kl, n, step):
    """AdamW's decay applied after the update differs by lr wd |update| = 1e-3 |update| ~ 16 000 u of it (the bound allows
    ~ 2000 u at step 1, where 1 - beta2^t = 0.001 is an fp32 difference of numbers near 1)"""
    with pytest.raises(AssertionError, match="out of bound"):
        run_adam(kl, n, step, True, True, 9, wrong="decay_after")


def test_adam_rejects(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    p = Guard(1, 8)
    z = torch.zeros(8, device="cuda")
    assert lib.kalle_adam_step(P(p.v), P(z), P(z), P(z), None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 1.0, st) == ERR_ARG
    assert lib.kalle_adam_step(P(p.v), None, P(z), P(z), None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, 1.0, st) == ERR_ARG
    assert lib.kalle_adam_step(P(p.v), P(z), P(z), P(z), None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, 1.0, st) == ERR_ARG
    torch.cuda.synchronize()
    p.untouched("adam")


# ================================================================================================ Llasa tail
@pytest.mark.parametrize("D,rows,vocab", [(4, 9, 5), (1024, 300, 50)])
@pytest.mark.parametrize("adt", DT, ids=["audio_f32", "audio_bf16"])
def test_embed_mix(kl, D, rows, vocab, adt):
    """out = audio am + table[ids] im: 3 u of the terms; rows with ids_mask 0 carry the padding id -100 and rows with audio_mask 0
    carry NaN audio: neither is read; two read rows carry ids outside the table (vocab + 3, -1), which are clamped.  bwd: daudio exact product rounding (u); dtable accumulates atomically over repeated ids."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(D + rows)
    ids = torch.randint(0, min(vocab, 7), (rows,), generator=g, device="cuda")        # few distinct ids: many repeats
    ids[-1] = vocab - 1
    kind = torch.arange(rows, device="cuda") % 4                                         # 0 text, 1 audio, 2 both fractional, 3 text
    im = torch.where(kind == 1, 0.0, torch.where(kind == 2, 0.5, 1.0)).float()
    am = torch.where(kind == 1, 1.0, torch.where(kind == 2, 0.75, 0.0)).float()
    ids[kind == 1] = -100
    ids[0], ids[3] = vocab + 3, -1                     # read rows (ids_mask 1) with ids outside the table: clamped to [0, vocab)
    audio = _randn((rows, D), g).to(adt)
    audio[am == 0] = NAN
    audio = _nan_tail(audio)
    table = _nan_tail(_randn((vocab, D), g), 3)
    out = Guard(rows, D)
    assert lib.kalle_embed_mix_fwd(P(ids), P(table), P(audio), int(adt == torch.float32), P(im), P(am), P(out.v), rows, D, vocab, st) == 0
    torch.cuda.synchronize()
    ii, ia = im != 0, am != 0
    assert ii[0] and ii[3]
    ids_read = torch.where(ii, ids.clamp(0, vocab - 1), ids)        # (the header: ids of rows that are read are clamped)
    ref = kr.embed_mix_fwd(ids_read, table.double(), audio.double(), im.double(), am.double())
    mag = torch.zeros_like(ref)
    mag[ia] += audio.double()[ia].abs() * am.double()[ia, None]
    mag[ii] += table.double()[ids_read[ii]].abs() * im.double()[ii, None]
    _check(out.v, ref, 3 * U * mag + 1e-38, f"embed_mix fwd D {D}")
    out.clean("embed_mix")
    do = _nan_tail(_randn((rows, D), g))
    for dt_on, da_on in ((True, True), (True, False), (False, True)):
        before = _randn((vocab, D), g)
        dtab = Guard(vocab, D, init=before, extra=3) if dt_on else None
        dau = Guard(rows, D) if da_on else None
        assert lib.kalle_embed_mix_bwd(P(do), P(ids), P(im), P(am), P(dtab.v) if dtab else None, P(dau.v) if dau else None, rows, D,
                                       vocab, st) == 0
        torch.cuda.synchronize()
        rt, ra = kr.embed_mix_bwd(do.double(), ids_read, im.double(), am.double(), vocab)
        if dau:
            _check(dau.v, ra, U * ra.abs() + 1e-38, "embed_mix daudio")
            dau.clean("daudio")
        if dtab:
            ab = torch.zeros_like(rt)
            ab.index_add_(0, ids_read[ii], (do.double()[ii] * im.double()[ii, None]).abs())
            _check(dtab.v, rt + before.double(), (rows + 4) * U * (ab + before.double().abs()) + 1e-38, "embed_mix dtable")
            dtab.clean("dtable")
    out = Guard(rows, D)
    assert lib.kalle_embed_mix_fwd(P(ids), P(table), P(audio), F32, P(im), P(am), P(out.v), rows, 6, vocab, st) == ERR_ARG
    assert lib.kalle_embed_mix_fwd(P(ids), P(table), P(audio), F32, None, P(am), P(out.v), rows, D, vocab, st) == ERR_ARG
    assert lib.kalle_embed_mix_bwd(P(do), P(ids), P(im), P(am), None, None, rows, D, vocab, st) == ERR_ARG
    torch.cuda.synchronize()
    out.untouched("embed_mix")


@pytest.mark.parametrize("rows,dim", [(1, 1), (7, 65), (1000, 64), (9000, 33)])
def test_gauss_kl(kl, rows, dim):
    """sums4 += {sum kl ma, sum ma, sum kl mb, sum mb} (accumulating) against the closed form; (rows + dim + 8) u of the terms.
    bwd with the fp32 sums as inputs: (DIV + 8) u of the magnitude of each product."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(rows + dim)
    std = _f32(0.7)
    pred, label = _nan_tail(_randn((rows, dim), g)), _nan_tail(_randn((rows, dim), g))
    ma = (torch.rand(rows, generator=g, device="cuda") > 0.4).float()
    mb = 1 - ma
    ma[0] = 1.0
    mb[-1] = 1.0                                                         # (each mask keeps at least one row)
    ma, mb = _nan_tail(ma, 4), _nan_tail(mb, 4)
    before = _randn((1, 4), g).abs()
    s4 = Guard(1, 4, init=before)
    assert lib.kalle_gauss_kl_fwd(P(pred), P(label), P(ma), P(mb), P(s4.v), std, rows, dim, st) == 0
    torch.cuda.synchronize()
    ref = kr.gauss_kl_fwd(pred.double(), label.double(), ma.double(), mb.double(), std)
    _check(s4.v[0], ref + before[0].double(), (rows + dim + 8) * U * (ref.abs() + before[0].double()) + 1e-30, f"gauss_kl fwd {rows}x{dim}")
    s4.clean("sums4")
    sums = _nan_tail(ref.float(), 4)
    ga, gb_ = torch.tensor([1.3], device="cuda"), torch.tensor([-0.4], device="cuda")
    dp = Guard(rows, dim)
    assert lib.kalle_gauss_kl_bwd(P(pred), P(label), P(ma), P(mb), P(sums), P(ga), P(gb_), P(dp.v), std, rows, dim, st) == 0
    torch.cuda.synchronize()
    sd = sums.double()
    rb = kr.gauss_kl_bwd(pred.double(), label.double(), ma.double(), mb.double(), sd, ga.double(), gb_.double(), std)
    unit = (pred.double().abs() + label.double().abs()) / (std * std * dim) * (ga.double().abs() * ma.double() / sd[1]
                                                                                + gb_.double().abs() * mb.double() / sd[3])[:, None]
    _check(dp.v, rb, (ALLOW["DIV"] + 8) * U * unit + 1e-38, f"gauss_kl bwd {rows}x{dim}", "DIV", unit)
    dp.clean("dpred")
    s4, dp = Guard(1, 4), Guard(rows, dim)
    assert lib.kalle_gauss_kl_fwd(P(pred), P(label), P(ma), P(mb), P(s4.v), 0.0, rows, dim, st) == ERR_ARG
    assert lib.kalle_gauss_kl_fwd(P(pred), P(label), None, P(mb), P(s4.v), std, rows, dim, st) == ERR_ARG
    assert lib.kalle_gauss_kl_bwd(P(pred), P(label), P(ma), P(mb), P(sums), None, P(gb_), P(dp.v), std, rows, dim, st) == ERR_ARG
    assert lib.kalle_gauss_kl_bwd(P(pred), P(label), P(ma), P(mb), P(sums), P(ga), P(gb_), P(dp.v), -1.0, rows, dim, st) == ERR_ARG
    torch.cuda.synchronize()
    s4.untouched("gauss_kl sums4")
    dp.untouched("gauss_kl dpred")


# ================================================================================================ conformer
def test_add_rows(kl):
    """x[b] += table, one fp32 add per element: exactly torch's fp32 sum"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(12)
    for nb, n in ((1, 4), (3, 1028), (130, 4100)):
        x0, t = _randn((nb, n), g), _nan_tail(_randn((n,), g), 4)
        x = Guard(nb, n, init=x0)
        assert lib.kalle_add_rows(P(x.v), P(t), nb, n, st) == 0
        torch.cuda.synchronize()
        _exact(x.v, x0 + t, f"add_rows {nb}x{n}")
        _check(x.v, kr.add_rows(x0.double(), t.double()), U * (x0.double().abs() + t.double().abs()), "add_rows vs fp64")
        x.clean("add_rows")
    x = Guard(2, 8)
    assert lib.kalle_add_rows(P(x.v), P(t), 2, 6, st) == ERR_ARG and lib.kalle_add_rows(P(x.v), None, 2, 8, st) == ERR_ARG
    assert lib.kalle_add_rows(P(x.buf[0, 1:]), P(t), 1, 4, st) == ERR_ARG                   # (not 16-byte aligned)
    torch.cuda.synchronize()
    x.untouched("add_rows")


DW_CASES = [(K, pad, N, D) for K, pad in ((1, 0), (17, 0), (17, 8), (17, 16), (32, 0), (32, 8), (32, 31))
            for N, D in ((1, 2), (5, 130), (126, 1536), (300, 130))]


def run_dwconv(kl, K, pad, N, D, flip, ydt, seed, wrong=None):
    """y = sum of <= K fma: (K + 1) u sum|terms| (+ one bf16 rounding); dw += sum over B N products, atomically: (B N + 8) u (sum|terms| + |before|)"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(seed)
    B = 2
    what = f"dwconv K {K} pad {pad} N {N} D {D} flip {flip} {ydt}"
    x = _nan_tail(_randn((B, N, D), g).bfloat16(), 1)
    w = _nan_tail(_randn((D, K), g, K ** -0.5), 2)
    y = Guard(B * N, D, dtype=ydt)
    assert lib.kalle_dwconv1d_fwd(P(x), P(w), P(y.v), int(ydt == torch.float32), B, N, D, K, pad, int(flip), st) == 0
    torch.cuda.synchronize()
    xd, wd = x.double(), w.double()
    shift = None
    if wrong == "tap_shift":
        shift = (pad, 1)                 # the term that reads x[n] (inside the signal for every n) reads x[n + 1] instead
    ref = kr.dwconv1d_fwd(xd, wd, pad, flip, tap_shift=shift)
    terms = kr.dwconv1d_fwd(xd.abs(), wd.abs(), pad, flip)
    _check(y.v, ref.view(B * N, D), ((K + 1) * U * terms + (0 if ydt == torch.float32 else BF16_REL * ref.abs())).view(B * N, D) + 1e-38,
           what)
    y.clean(what)
    if wrong is None and not flip:
        dy = _nan_tail(_randn((B, N, D), g).bfloat16(), 1)
        before = _randn((D, K), g)
        dw = Guard(D, K, init=before)
        assert lib.kalle_dwconv1d_wgrad(P(dy), P(x), P(dw.v), B, N, D, K, pad, st) == 0
        torch.cuda.synchronize()
        rw = kr.dwconv1d_wgrad(dy.double(), xd, K, pad)
        tw = kr.dwconv1d_wgrad(dy.double().abs(), xd.abs(), K, pad)
        _check(dw.v, rw + before.double(), (B * N + 8) * U * (tw + before.double().abs()) + 1e-38, what + " wgrad")
        dw.clean(what + " wgrad")


@pytest.mark.parametrize("K,pad,N,D", DW_CASES)
def test_dwconv(kl, K, pad, N, D):
    i = K + pad + N + D
    run_dwconv(kl, K, pad, N, D, False, DT[i % 2], i)
    run_dwconv(kl, K, pad, N, D, True, DT[(i + 1) % 2], i + 1)


@pytest.mark.parametrize("K,pad,N,D", [c for c in DW_CASES if c[2] > 1])
@pytest.mark.parametrize("flip", [False, True])
def test_dwconv_wrong_reference_is_caught(kl, K, pad, N, D, flip):
    """one tap of the filter reads the neighbouring position"""
    with pytest.raises(AssertionError, match="out of bound"):
        run_dwconv(kl, K, pad, N, D, flip, torch.float32, 3, wrong="tap_shift")


def test_dwconv_rejects(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    x = torch.zeros((1, 4, 8), device="cuda", dtype=torch.bfloat16)
    w = torch.zeros((8, 33), device="cuda")
    y = Guard(4, 8)
    for D, K, pad, B in ((7, 3, 1, 1), (8, 33, 1, 1), (8, 3, 3, 1), (8, 3, -1, 1), (8, 0, 0, 1), (8, 3, 1, 65536)):
        assert lib.kalle_dwconv1d_fwd(P(x), P(w), P(y.v), F32, B, 4, D, K, pad, 0, st) == ERR_ARG
        assert lib.kalle_dwconv1d_wgrad(P(x), P(x), P(y.v), B, 4, D, K, pad, st) == ERR_ARG
    assert lib.kalle_dwconv1d_fwd(P(x), P(w), P(y.v), 2, 1, 4, 8, 3, 1, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    y.untouched("dwconv")


def test_elementwise_rejects(kl):
    """the remaining rejections the entry points make before any launch: NaN-filled outputs stay untouched"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    z = torch.zeros(64, device="cuda")
    zb = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    o, ob = Guard(1, 64), Guard(1, 64, dtype=torch.bfloat16)
    assert lib.kalle_swiglu_fwd(P(zb), P(ob.v), 1, 12, st) == ERR_ARG
    assert lib.kalle_swiglu_fwd(P(zb), P(ob.v), 0, 8, st) == ERR_ARG
    assert lib.kalle_swiglu_bwd(P(zb), P(zb), P(ob.v), None, 1, 12, st) == ERR_ARG
    assert lib.kalle_swiglu_bwd(None, P(zb), P(ob.v), None, 1, 8, st) == ERR_ARG
    for f in (lib.kalle_silu_fwd, lib.kalle_gelu_fwd):
        assert f(P(z), P(o.v), F32, 0, st) == ERR_ARG and f(None, P(o.v), F32, 8, st) == ERR_ARG
    for f in (lib.kalle_silu_bwd, lib.kalle_gelu_bwd):
        assert f(P(z), None, P(o.v), F32, 8, st) == ERR_ARG and f(P(z), P(z), P(o.v), F32, -1, st) == ERR_ARG
    assert lib.kalle_transpose_2d(P(z), F32, 64, 8, P(o.v), F32, 64, 8, 65536, 8, 8, st) == ERR_ARG
    assert lib.kalle_transpose_2d(P(z), F32, 64, 8, P(o.v), F32, 64, 8, 1, 0, 8, st) == ERR_ARG
    torch.cuda.synchronize()
    o.untouched("elementwise")
    ob.untouched("elementwise")


# ================================================================================================ more of the DiT path / Llasa tail
@pytest.mark.parametrize("n", [1, 1003, 2048 * 256 + 3])
def test_axpby(kl, n):
    """out = a x + b y: 3 u (|a x| + |b y|) (a product may be fused into the add)"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(n % 1000)
    x, y = _nan_tail(_randn((n,), g), 4), _nan_tail(_randn((n,), g), 4)
    a, b = _f32(0.3), _f32(-1.7)
    out = Guard(1, n, extra=1)
    assert lib.kalle_axpby(P(x), P(y), P(out.v), a, b, n, st) == 0
    torch.cuda.synchronize()
    _check(out.v[0], kr.axpby(x.double(), y.double(), a, b), 3 * U * (abs(a) * x.double().abs() + abs(b) * y.double().abs()) + 1e-38,
           f"axpby n {n}")
    out.clean("axpby")
    out = Guard(1, n, extra=1)
    assert lib.kalle_axpby(P(x), None, P(out.v), a, b, n, st) == ERR_ARG and lib.kalle_axpby(P(x), P(y), P(out.v), a, b, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    out.untouched("axpby")


@pytest.mark.parametrize("n", [1, 1003, 2048 * 256 + 3])
@pytest.mark.parametrize("dt", DT, ids=["f32", "bf16"])
def test_peak_normalize_int16(kl, dt, n):
    """peak = max|x| exactly; out = int16(trunc(clamp(x / peak, -1, 1) * 32767)): the quotient and the product round once each
    (2 u x 32767 = 0.004), so the result equals the truncated fp64 value wherever that is further than 0.01 from an integer and is
    within 1 of it elsewhere; the peak element is +-32767 exactly"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    x = _nan_tail(_randn((n,), _gen(n % 1000 + 1)).to(dt), 8)
    peak = Guard(1, 1)
    tail = torch.full((8,), 12345, device="cuda", dtype=torch.int16)
    buf = torch.cat([torch.full((n,), 12345, device="cuda", dtype=torch.int16), tail])
    assert lib.kalle_peak_normalize_int16(P(x), int(dt == torch.float32), P(peak.v), P(buf), n, st) == 0
    torch.cuda.synchronize()
    v, pk = kr.peak_normalize(x.double())
    assert peak.v.item() == pk.item()
    peak.clean("peak")
    got, want = buf[:n].double(), v.trunc()
    far = (v - v.round()).abs() > 0.01
    assert (got[far] == want[far]).all() and ((got - want).abs() <= 1).all(), int((got != want).sum())
    assert (got[x.double().abs() == pk].abs() == 32767).all()
    assert (buf[n:] == 12345).all(), "stray writes"
    peak = Guard(1, 1)
    assert lib.kalle_peak_normalize_int16(P(x), F32, P(peak.v), None, n, st) == ERR_ARG
    assert lib.kalle_peak_normalize_int16(P(x), F32, P(peak.v), P(buf), 0, st) == ERR_ARG
    torch.cuda.synchronize()
    peak.untouched("peak")
    assert (buf[n:] == 12345).all() and (buf[:n].double() == got).all()


@pytest.mark.parametrize("nb,rpb,D", [(1, 1, 4), (3, 16, 132), (5, 126, 1536), (2, 37, 8)])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_grad_cast(kl, nb, rpb, D, gated, masked):
    """gb = bf16(g sigmoid(1 - gate[b]) row_mask): (SIGMOID + 3) u |g| + one bf16 rounding.  dgate (cleared by the call, then
    summed atomically over 16-row chunks: NOT accumulating, so it starts from garbage and the padding of its rows stays NaN)
    = -(1 - s) sum_t g m (x_out - x_in): 1 - s is a difference of numbers near 1 -> (SIGMOID + 2) u of |sum|, plus (1 - s) times
    the (rpb + 8) u sum|terms| bound with each x_out - x_in carrying u (|x_out| + |x_in|)"""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(nb * rpb + D)
    rows, ldg = nb * rpb, D + 12
    gr = _nan_tail(_randn((rows, D), g))
    xo, xi = _nan_tail(_randn((rows, D), g)), _nan_tail(_randn((rows, D), g))
    gate_buf = torch.full((nb + 1, ldg), NAN, device="cuda")
    gate_buf[:nb, :D] = _with_edges(_randn((nb, D), g, 2.0))[:, :]           # gate values that saturate 1 - s on both sides
    gate = gate_buf[:nb, :D] if gated else None
    mask = None
    if masked:
        mask = (torch.rand(rows, generator=g, device="cuda") > 0.3).to(torch.uint8)
        mask[-1] = 0
    gb = Guard(rows, D, dtype=torch.bfloat16)
    dgate = Guard(nb, D, ld=ldg, init=torch.full((nb, D), 7.0, device="cuda") if gated else None)
    assert lib.kalle_grad_cast(P(gr), P(xo) if gated else None, P(xi) if gated else None, P(gate), ldg if gated else 0, P(mask), P(gb.v),
                               P(dgate.v), nb, rpb, D, st) == 0
    torch.cuda.synchronize()
    gd, xod, xid = gr.double(), xo.double(), xi.double()
    ref, dref = kr.grad_cast(gd, xod, xid, None if gate is None else gate.double(), mask, nb, rpb)
    what = f"grad_cast {nb}x{rpb}x{D} gate {gated} mask {masked}"
    _check(gb.v, ref, (ALLOW["SIGMOID"] + 3) * U * gd.abs() + BF16_REL * ref.abs() + 1e-38, what + " gb")
    gb.clean(what)
    if gated:
        gm = gd if mask is None else gd * (mask != 0).double()[:, None]
        oms = kr.sigmoid(gate.double() - 1)
        raw = (gm * (xod - xid)).view(nb, rpb, D).sum(1)
        terms = (gm.abs() * ((xod - xid).abs() + (rpb + 8) ** -1 * (xod.abs() + xid.abs()))).view(nb, rpb, D).sum(1)
        tol = (ALLOW["SIGMOID"] + 2) * U * raw.abs() + oms * (rpb + 8) * U * terms + 1e-38
        _check(dgate.v, dref, tol, what + " dgate")
        dgate.clean(what)
    else:
        dgate.untouched(what + " dgate without a gate")
    gb = Guard(rows, D, dtype=torch.bfloat16)
    assert lib.kalle_grad_cast(P(gr), None, None, None, 0, None, P(gb.v), None, nb, rpb, 6, st) == ERR_ARG
    assert lib.kalle_grad_cast(P(gr), None, None, None, 0, None, P(gb.v), None, 65536, rpb, D, st) == ERR_ARG
    assert lib.kalle_grad_cast(P(gr), None, P(xi), P(gate_buf), ldg, None, P(gb.v), None, nb, rpb, D, st) == ERR_ARG
    assert lib.kalle_grad_cast(P(gr), P(xo), P(xi), P(gate_buf), ldg + 2, None, P(gb.v), None, nb, rpb, D, st) == ERR_ARG
    torch.cuda.synchronize()
    gb.untouched(what)


@pytest.mark.parametrize("rows,dim", [(1, 1), (7, 65), (1000, 64), (9000, 33)])
@pytest.mark.parametrize("mode", [0, 1])
def test_gauss_kl2(kl, rows, dim, mode):
    """sums4 += ... (accumulating) against the closed form KL(N(m1, s1) || N(m2, exp(l2))); per element the terms are l2, log s1,
    (s1^2 + (m1 - m2)^2) e / 2 and 1/2, e = exp(-2 l2): (rows + dim + 8 + EXP) u of sum|terms| (+ 8 u per element for log s1
    near 0, whose error is s1's relative error).  bwd with the fp32 sums as inputs: (EXP + DIV + 8) u of each product's magnitude."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    g = _gen(rows + dim + mode)
    mult = _f32(1.25)
    pred = _nan_tail(_randn((rows, 2 * dim), g, 0.5))
    if mode == 0:
        lm, ls = _nan_tail(_randn((rows, dim), g)), _nan_tail(_randn((rows, dim), g).abs() + 0.1)
    else:
        raw = _randn((rows, 2 * dim), g, 3.0)
        raw[0, dim] = 25.0                                     # above F.softplus's threshold of 20
        lm, ls = _nan_tail(raw), None
    ma = (torch.rand(rows, generator=g, device="cuda") > 0.4).float()
    mb = 1 - ma
    ma[0], mb[-1] = 1.0, 1.0
    ma, mb = _nan_tail(ma, 4), _nan_tail(mb, 4)
    before = _randn((1, 4), g).abs()
    s4 = Guard(1, 4, init=before)
    assert lib.kalle_gauss_kl2_fwd(P(pred), P(lm), P(ls), mode, mult, P(ma), P(mb), P(s4.v), rows, dim, st) == 0
    torch.cuda.synchronize()
    pd, lmd, lsd, mad, mbd = pred.double(), lm.double(), None if ls is None else ls.double(), ma.double(), mb.double()
    ref = kr.gauss_kl2_fwd(pd, lmd, lsd, mode, mult, mad, mbd)
    m1, s1 = kr._kl2_label(lmd, lsd, mode, mult, dim)
    m2, l2 = pd[:, :dim], pd[:, dim:]
    e = torch.exp(-2 * l2)
    q = 0.5 * (s1 * s1 + (m1 - m2).pow(2)) * e
    absrow = (l2.abs() + s1.log().abs() + q * (1 + 2 * l2.abs()) + 0.5 + 8).sum(-1) / dim
    mag = torch.stack([(absrow * mad).sum(), mad.sum(), (absrow * mbd).sum(), mbd.sum()])
    what = f"gauss_kl2 mode {mode} {rows}x{dim}"
    _check(s4.v[0], ref + before[0].double(), (rows + dim + 8 + ALLOW["EXP"]) * U * (mag + before[0].double()) + 1e-30, what + " fwd")
    s4.clean(what)
    sums = _nan_tail(ref.float(), 4)
    ga, gb_ = torch.tensor([1.3], device="cuda"), torch.tensor([-0.4], device="cuda")
    dp = Guard(rows, 2 * dim)
    assert lib.kalle_gauss_kl2_bwd(P(pred), P(lm), P(ls), mode, mult, P(ma), P(mb), P(sums), P(ga), P(gb_), P(dp.v), rows, dim, st) == 0
    torch.cuda.synchronize()
    sd = sums.double()
    rb = kr.gauss_kl2_bwd(pd, lmd, lsd, mode, mult, mad, mbd, sd, ga.double(), gb_.double())
    w = ((ga.double().abs() * mad / sd[1] + gb_.double().abs() * mbd / sd[3]) / dim)[:, None]
    unit = torch.cat([w * (m1.abs() + m2.abs()) * e * (1 + 2 * l2.abs()), w * (1 + 2 * q * (1 + 2 * l2.abs()))], 1)
    _check(dp.v, rb, (ALLOW["EXP"] + ALLOW["DIV"] + 8) * U * unit + 1e-38, what + " bwd", "EXP", unit)
    dp.clean(what)
    s4, dp = Guard(1, 4), Guard(rows, 2 * dim)
    assert lib.kalle_gauss_kl2_fwd(P(pred), P(lm), P(ls), mode, 0.0, P(ma), P(mb), P(s4.v), rows, dim, st) == ERR_ARG
    assert lib.kalle_gauss_kl2_fwd(P(pred), None, P(ls), mode, mult, P(ma), P(mb), P(s4.v), rows, dim, st) == ERR_ARG
    assert lib.kalle_gauss_kl2_bwd(P(pred), P(lm), P(ls), mode, mult, P(ma), P(mb), P(sums), P(ga), None, P(dp.v), rows, dim, st) == ERR_ARG
    torch.cuda.synchronize()
    s4.untouched(what)
    dp.untouched(what)


def test_measured_deviations_within_allowance(kl):
    """(last in the file) prints what the measurement points above recorded (`-s`), in units of u x the magnitude each names, and
    holds each to its allowance - which the element-wise checks already imply; re-measure from this line when the compiler changes"""
    print("\nmeasured intrinsic deviations (units of u * magnitude): " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(MEASURED.items())))
    for k, v in MEASURED.items():
        assert v <= ALLOW[k], (k, v, ALLOW[k])
