"""-m gpu: the VAE conv stack of include/kalle_hip.h (csrc/conv1d.hip, csrc/conv1d_bwd.hip), element by element against the
fp64 references of tests/kernel_refs.py (which tests/test_conv_refs_cpu.py checks against torch on the CPU).

Conventions: those of test_norm_elementwise_gpu.py; the checks the two files share live in tests/gpu_checks.py - calls through ctypes,
every element bounded and the first offender reported, NaN before and after every operand and output buffer (the tensors are
dense: `guarded`, the one-dimensional form of `Guard`), accumulating
outputs started from random contents and checked as before + ref, pure data movement bit-exact.  Every forward / wgrad case
names the plan word (kalle_conv_last_plan, encoding in the header) it expects and asserts it; the shapes can be checked without
a device through the queries kalle_conv_plan / kalle_conv_transpose_plan / kalle_conv_wgrad_plan (tests/test_conv_plan_cpu.py
does, over tests/conv_cases.py), a case whose plan does not come out is a wrong case.

Error model, u = 2^-24.  A conv output before the activation is an n-term fp32 sum, n = Cin K + 4 (bias, residual, scale,
accumulate), in any order (so the ks > 1 partial sums and the wgrad atomics are covered): |err| <= n u abs_sum, abs_sum = the sum
of the magnitudes of the terms, returned by the reference.  The input activation's own error e(x) goes through the sum as
sum |w| e(x) (a second reference conv over e with |w|).  post_act / tanh: Lipschitz constant times the error so far + the
activation's own error.  A bf16 store: BF16_REL |ref|; bf16 inputs are exact operands (the reference starts from them).
Cancelling expressions are bounded by their terms: ELU's __expf(x) - 1 by u * 1, tanh_bwd's 1 - y^2 by u (1 + y^2).
The intrinsics under -ffast-math have no bound derivable from the source.  Their allowances (ALLOW) are MEASURED on the
elementwise entry point that isolates each (test_measure_*: a dense sweep of arguments and channel parameters), in units of
u * the stated magnitude, times the margin of 4; no conv case sets its own.  The last test prints MEASURED and holds each to its
allowance."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as kr  # noqa: E402
import test_norm_elementwise_gpu as ne  # noqa: E402  (its ALLOW["DIV"], the pairwise-cover generator, _gen / _randn)
from gpu_checks import NAN, U, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402
from test_norm_elementwise_gpu import BF16_REL, _gen, _randn  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = 1, 0
ERR_ARG, ERR_UNSUPPORTED = -1, -3

# measured on one MI355X (ROCm 7, -O3 -ffast-math), 2026-10-16, by the test_measure_* sweeps of this file, in units of
# u * magnitude, then x 4 (other seeds, other compiler versions; a structural error is of order 1 / u in these units)
ALLOW = {
    "SNAKE": 29.0,     # fast_sin (v_sin_f32 on fract(a x / 2 pi)), __expf of alpha / beta, reciprocal: kalle_conv_pad_act act 1 and
                       # kalle_snake_beta_fwd, fp32, unit (1 + |a x|) / (b + 1e-9)                                  measured 7.01
    "ELU": 5.0,        # __expf(x) - 1, x <= 0: kalle_conv_pad_act act 2, unit 1                                    measured 1.17
    "TANH": 6.0,       # tanhf of the epilogue: k = 1, Cin = Cout = 1, weight 1 conv, unit 1                       measured 1.36
    "GATE": 10.0,      # tanhf(x) / (1 + __expf(-g)): the same conv with in_act 4, unit 1                          measured 2.41
    "DIV": ne.ALLOW["DIV"],     # division / sqrtf (weight-norm fold and backward): the existing allowance, not re-measured
}
MEASURED = {}
PLANS_SEEN = set()


def _check(out, ref, tol, what, key=None, unit=None):
    return check(out, ref, tol, what, key, unit, MEASURED)


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load(), _lib


# ------------------------------------------------------------------------------------------------ plan words (header)
def v2(cow, lpt, wco, nw=4, ci=8, stride=1, dt=F32, family=2):
    lg = {8: 0, 16: 1, 32: 2}[ci]
    ls = {1: 0, 2: 1, 4: 2, 8: 3}[stride]
    return family | (0x30 if dt == F32 else 0) | cow << 8 | lpt << 13 | wco << 17 | nw << 21 | lg << 25 | ls << 28


def tv2(cow, lpt, wco, dt=F32):
    return v2(cow, lpt, wco, dt=dt, family=4)


def fb(xdt=F32, ydt=F32, family=1):
    return family | (0x10 if xdt == F32 else 0) | (0x20 if ydt == F32 else 0)


def cf(split, ks=1, family=5):
    return family | 0x30 | split << 8 | ks << 12


def wg_lds(tu, kt):
    return 8 | 0x30 | tu << 8 | kt << 13


def wg_lane(tu, tv, km):
    return 9 | 0x30 | tu << 8 | tv << 13 | km << 18


# ------------------------------------------------------------------------------------------------ helpers
def _act_vals(g, C, spread=1.0):
    """distinct per-channel alpha / beta (log scale) with a wide spread: a neighbour's parameters are far outside the bound"""
    al = (torch.linspace(-spread, spread, C, device="cuda") + 0.05 * _randn((C,), g)).flip(0)
    be = torch.linspace(-spread, spread, C, device="cuda") + 0.05 * _randn((C,), g)
    return al, be


def _act_struct(L, code, al=None, be=None, logscale=1, param=0.0):
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return L.Act(code, logscale, P(al), P(be), param)


def _act_err(x, code, al, be, logscale, param):
    """|kernel act(x) - exact act(x)| allowed per element (x float64, exact operands)"""
    if code == 0:
        return torch.zeros_like(x)
    if code == 1:
        a, b = kr._act_ab(al, be, logscale)
        a, b = a[None, :, None], b[None, :, None] + 1e-9
        return ALLOW["SNAKE"] * U * (1 + (a * x).abs()) / b + 2 * U * x.abs()
    if code == 2:
        return torch.where(x > 0, torch.zeros_like(x), torch.full_like(x, ALLOW["ELU"] * U))
    if code == 3:
        return U * (x * param).abs()
    h = x.shape[1] // 2
    return torch.full_like(x[:, :h], ALLOW["GATE"] * U)


def _act_lip(code, al, be, logscale, param):
    """Lipschitz constant per channel, [1][C][1] or a float"""
    if code == 1:
        a, b = kr._act_ab(al, be, logscale)
        return (1 + a / (b + 1e-9))[None, :, None]
    if code == 3:
        return max(1.0, abs(param))
    return 1.0


DEFAULT = dict(B=3, Cin=9, Cout=20, K=3, stride=1, pl=1, dil=1, Lin=200, Lout=None, xdt=F32, ydt=F32, act=0, logscale=1, bias=True,
               res=False, scale=1.0, acc=False, post=0, plog=1, tanh=False, raw=False, entry="conv", ws=True, rc=0, wrong=None)


def C(plan, **kw):
    c = dict(DEFAULT)
    c.update(kw)
    c["plan"] = plan
    if c["Lout"] is None:
        if c["entry"] in ("conv", "cfirst"):      # 'same'-style: the right pad equals the left pad
            c["Lout"] = (c["Lin"] + 2 * c["pl"] - c["dil"] * (c["K"] - 1) - 1) // c["stride"] + 1
        else:
            c["Lout"] = (c["Lin"] - 1) * c["stride"] - 2 * c["pl"] + c["K"]
    return c


def _id(c):
    keys = ("entry", "B", "Cin", "Cout", "K", "stride", "pl", "dil", "Lin", "Lout", "act", "post", "res", "acc", "tanh", "raw", "xdt", "ydt")
    return "-".join(f"{k}{c[k]:g}" if isinstance(c[k], float) else f"{k}{c[k]}" for k in keys if c[k] != DEFAULT.get(k) or k in ("Cout", "K"))


def run_conv(kl, c, seed=1, wrong=None):
    """one forward case through its entry point: plan word, per-element bound on y and y_raw, guards.  `wrong` names a
    deliberately wrong reference (test_wrong_references_are_caught)"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(seed)
    B, Cin, Cout, K, stride, pl, dil, Lin, Lout = (c[k] for k in ("B", "Cin", "Cout", "K", "stride", "pl", "dil", "Lin", "Lout"))
    entry, act = c["entry"], c["act"]
    transposed = entry in ("convT", "cfirstT")
    tdt = lambda d: torch.float32 if d == F32 else torch.bfloat16  # noqa: E731
    xC = 2 * Cin if act == 4 else Cin
    xbuf, x = _guarded((_randn((B, xC, Lin), g, 1.5)).to(tdt(c["xdt"])))
    al, be = _act_vals(g, Cin)
    if not c["logscale"]:
        al, be = al.exp(), be.exp()
    pal, pbe = _act_vals(g, Cout)
    if not c["plog"]:
        pal, pbe = pal.exp(), pbe.exp()
    # weights: a module's v (no g), folded by the library's own repack (bit-exact, test_weight_norm_fold), NaN around it
    v = _randn((Cin, Cout, K) if transposed else (Cout, Cin, K), g, 0.3)
    CoutP = (Cout + 7) // 8 * 8
    wbuf, w = _guarded(torch.zeros((Cin, K, CoutP), device="cuda"))
    assert lib.kalle_weight_norm_fold(P(v), None, P(w), v.shape[0], v.shape[1], K, 1 if transposed else 0, st) == 0
    bias = _guarded(_randn((Cout,), g))[1] if c["bias"] else None
    res = _guarded(_randn((B, Cout, Lout), g).to(tdt(c["xdt"])))[1] if c["res"] else None
    y0 = _randn((B, Cout, Lout), g).to(tdt(c["ydt"])) if c["acc"] else torch.full((B, Cout, Lout), NAN, device="cuda", dtype=tdt(c["ydt"]))
    ybuf, y = _guarded(y0)
    rbuf, raw = _guarded(torch.full((B, Cout, Lout), NAN, device="cuda", dtype=tdt(c["ydt"]))) if c["raw"] else (None, None)
    ia = _act_struct(L, act, al if act == 1 else None, be if act == 1 else None, c["logscale"], 0.2)
    ep = L.ConvEpilogue(P(res), c["scale"], int(c["acc"]), int(c["tanh"]),
                        _act_struct(L, c["post"], pal if c["post"] == 1 else None, pbe if c["post"] == 1 else None, c["plog"], 0.1),
                        P(raw))
    if entry == "conv":
        rc = lib.kalle_conv1d_fwd(P(x), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride, pl, dil,
                                  ctypes.addressof(ia), ctypes.addressof(ep), st)
    elif entry == "convT":
        rc = lib.kalle_conv_transpose1d_fwd(P(x), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride, pl,
                                            ctypes.addressof(ia), ctypes.addressof(ep), st)
    elif entry == "cfirst":
        Lp = lib.kalle_conv_pad_len(Lout, K, stride, pl, dil)
        lead = pl if stride == 1 else (pl + stride - 1) // stride * stride
        pbuf, xp = _guarded(torch.full((B, Cin, Lp), NAN, device="cuda"))
        assert lib.kalle_conv_pad_act(P(x), P(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), stride, st) == 0
        nws = lib.kalle_conv_cfirst_ws_floats(B, Cin, Cout, Lout, K)
        assert (nws > 0) == ((c["plan"] >> 12 & 31) > 1 or not c["ws"]), nws
        wsb, ws = _guarded(torch.full((max(nws, 1),), NAN, device="cuda")) if c["ws"] and nws else (None, None)
        rc = lib.kalle_conv1d_cfirst_fwd(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl, dil,
                                         ctypes.addressof(ep), P(ws), st)
    else:
        Lp = lib.kalle_convT_pad_len(Lout, K, stride, pl)
        pbuf, xp = _guarded(torch.full((B, Cin, Lp), NAN, device="cuda"))
        assert lib.kalle_conv_pad_act(P(x), P(xp), B, Cin, Lin, Lp, (K + stride - 1) // stride - 1, ctypes.addressof(ia), 1, st) == 0
        rc = lib.kalle_conv_transpose1d_cfirst_fwd(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl,
                                                   ctypes.addressof(ep), st)
    plan = lib.kalle_conv_last_plan()
    torch.cuda.synchronize()
    what = _id(c)
    assert rc == c["rc"], (what, rc)
    assert plan == c["plan"], (what, hex(plan), hex(c["plan"]))
    if rc != 0:
        assert torch.isnan(y).all() and (raw is None or torch.isnan(raw).all()), (what, "a refused call wrote its output")
        return
    PLANS_SEEN.add(plan)
    # ---- reference
    xd, wd = x.double(), w.double()
    in_act = (act, al, be, c["logscale"], 0.2)
    post = (c["post"], pal, pbe, c["plog"], 0.1) if c["post"] else None
    epd = dict(residual=None if res is None else res.double(), out_scale=float(torch.tensor(c["scale"], dtype=torch.float32)),
               accumulate=y0.double() if c["acc"] else None, post=post, tanh=c["tanh"])
    wrong_kw = {}
    if wrong == "first_tap_shifted":
        wrong_kw = dict(tap_shift=(0, 1, pl))
    elif wrong == "last_tap_dropped":
        wrong_kw = dict(drop_last_tap_from=Lout - 64)
    elif wrong == "alpha_next_channel":
        in_act = (act, al.roll(-1), be, c["logscale"], 0.2)
    elif wrong == "post_alpha_next_channel":
        epd["post"] = (c["post"], pal.roll(-1), pbe, c["plog"], 0.1)
    elif wrong == "pad_column":
        wd = wd.clone()
        wd[:, :, Cout - 1] += 0.3 * _randn((Cin, K), g).double()        # (what a non-zero pad column read as channel Cout - 1 gives)
    fn = kr.conv_transpose1d if transposed else kr.conv1d
    geo = dict(stride=stride, padding=pl, Lout=Lout) if transposed else dict(stride=stride, padding=pl, dilation=dil, Lout=Lout)
    ref, ref_raw, asum = fn(xd, wd, Cout, None if bias is None else bias.double(), in_act=in_act, epilogue=epd, **geo, **wrong_kw)
    if wrong == "scale_after_accumulate":
        e2 = dict(epd, accumulate=None, out_scale=1.0)
        r0 = fn(xd, wd, Cout, None if bias is None else bias.double(), in_act=in_act, epilogue=dict(e2, post=None, tanh=False), **geo)[0]
        ref_raw = (r0 + y0.double()) * epd["out_scale"]
        ref = kr._epilogue(ref_raw, asum, Cout, None, dict(post=post, tanh=c["tanh"]))[0]
    elif wrong == "tanh_before_post":
        ref = kr.act(torch.tanh(ref_raw), *post)
    elif wrong == "raw_after_post":
        ref_raw = kr.act(ref_raw, *post)
    elif wrong == "partial_sum_missing":                                    # the last of the ks input-channel slices left out
        ks = c["plan"] >> 12 & 31
        per = ((Cin * K + 7) // 8 + ks - 1) // ks * 8 // K
        xz = xd.clone()
        xz[:, Cin - max(per, 1):] = 0
        ref, ref_raw, _ = fn(xz, wd, Cout, None if bias is None else bias.double(), in_act=in_act, epilogue=epd, **geo)
    # ---- bound
    n = Cin * K + 4
    ex = _act_err(xd, *in_act[:1], al, be, c["logscale"], 0.2)
    eprop = fn(ex, wd.abs(), Cout, None, epilogue=dict(out_scale=abs(epd["out_scale"])), **geo)[0] if act else 0.0
    tol_raw = n * U * asum + eprop
    tol = tol_raw
    vr = ref_raw
    if post:
        tol = tol * _act_lip(*post[:1], pal, pbe, c["plog"], 0.1) + _act_err(vr, c["post"], pal, pbe, c["plog"], 0.1) + U * vr.abs()
        vr = kr.act(vr, *post)
    if c["tanh"]:
        tol = tol + ALLOW["TANH"] * U
    yb = BF16_REL if c["ydt"] == BF16 else 0.0
    _check(y, ref, tol + yb * ref.abs() + 1e-30, what + " y")
    if raw is not None:
        _check(raw, ref_raw, tol_raw + yb * ref_raw.abs() + 1e-30, what + " y_raw")
        _clean(rbuf, raw, what + " y_raw")
    _clean(ybuf, y, what + " y")
    if entry.startswith("cfirst"):
        _clean(pbuf, xp, what + " x_padded")


# ================================================================================================ the intrinsics, isolated
def test_measure_snake_elu(kl):
    """kalle_conv_pad_act with Lp = Lin, padding 0 (act 1, 2, 3) and kalle_snake_beta_fwd over a dense sweep: x in [-8, 8],
    alpha, beta (log scale and plain) over [-1.5, 1.5] per channel, fp32"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    Cn, Ln = 96, 8192
    x = torch.linspace(-8, 8, Ln, device="cuda")[None, None, :].expand(2, Cn, Ln).contiguous() + 1e-3 * _randn((2, Cn, Ln), _gen(1))
    al = torch.linspace(-1.5, 1.5, Cn, device="cuda")
    be = torch.linspace(-1.5, 1.5, Cn, device="cuda").roll(37)
    xd = x.double()
    for logscale in (1, 0):
        a, b = (al, be) if logscale else (al.exp(), be.exp())
        ref = kr.act(xd, 1, a, b, logscale)
        aa, bb = kr._act_ab(a, b, logscale)
        unit = (1 + (aa[None, :, None] * xd).abs()) / (bb[None, :, None] + 1e-9)
        tol = ALLOW["SNAKE"] * U * unit + 2 * U * xd.abs()
        for which in ("pad_act", "snake_beta"):
            ybuf, y = _guarded(torch.full_like(x, NAN))
            if which == "pad_act":
                ia = _act_struct(L, 1, a, b, logscale)
                assert lib.kalle_conv_pad_act(P(x), P(y), 2, Cn, Ln, Ln, 0, ctypes.addressof(ia), 1, st) == 0
            else:
                assert lib.kalle_snake_beta_fwd(P(x), P(y), F32, P(a), P(b), logscale, 2, Cn, Ln, st) == 0
            torch.cuda.synchronize()
            _check(y, ref, tol, f"snake {which} logscale {logscale}", "SNAKE", unit)
            _clean(ybuf, y, which)
    for code, key in ((2, "ELU"), (3, None)):
        ybuf, y = _guarded(torch.full_like(x, NAN))
        ia = _act_struct(L, code, param=0.2)
        assert lib.kalle_conv_pad_act(P(x), P(y), 2, Cn, Ln, Ln, 0, ctypes.addressof(ia), 1, st) == 0
        torch.cuda.synchronize()
        ref = kr.act(xd, code, param=float(torch.tensor(0.2, dtype=torch.float32)))
        if code == 2:
            _check(y, ref, torch.where(xd > 0, 0.0, ALLOW["ELU"] * U), "elu", "ELU", (xd <= 0).double())
        else:
            _check(y, ref, U * ref.abs(), "leaky relu")
        _clean(ybuf, y, "pad_act")


def test_measure_tanh_gate(kl):
    """the tanh store and the WaveNet gate through a k = 1, Cin = Cout = 1, weight 1 conv (v2 2x2x1 / fallback), fp32"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    Ln = 65536
    w = torch.zeros(8, device="cuda")
    w[0] = 1.0
    x = torch.linspace(-9, 9, Ln, device="cuda")[None, None, :].contiguous()
    ybuf, y = _guarded(torch.full_like(x, NAN))
    ep = L.ConvEpilogue(None, 1.0, 0, 1, _act_struct(L, 0), None)
    assert lib.kalle_conv1d_fwd(P(x), F32, P(w), None, P(y), F32, 1, 1, Ln, 1, Ln, 1, 1, 0, 1, None, ctypes.addressof(ep), st) == 0
    assert lib.kalle_conv_last_plan() == v2(2, 2, 1)
    torch.cuda.synchronize()
    _check(y, torch.tanh(x.double()), ALLOW["TANH"] * U, "tanh store", "TANH", 1.0)
    _clean(ybuf, y, "tanh")
    x2 = torch.cat([x, (x * 1.7).flip(2)], 1).contiguous()
    ybuf, y = _guarded(torch.full_like(x, NAN))
    ia = _act_struct(L, 4)
    assert lib.kalle_conv1d_fwd(P(x2), F32, P(w), None, P(y), F32, 1, 1, Ln, 1, Ln, 1, 1, 0, 1, ctypes.addressof(ia), None, st) == 0
    assert lib.kalle_conv_last_plan() == fb()
    torch.cuda.synchronize()
    _check(y, kr.act(x2.double(), 4), ALLOW["GATE"] * U, "gate", "GATE", 1.0)
    _clean(ybuf, y, "gate")


# ================================================================================================ forward: kalle_conv1d_fwd
BIG = 32910
CONV_CASES = [
    C(v2(2, 2, 1), Cout=4, K=7, pl=3, Lin=300, act=1, res=True, raw=True, post=2),
    C(v2(2, 2, 1), Cout=1, Cin=1, K=3, Lin=128, act=2),
    C(v2(2, 2, 1, dt=BF16), Cout=3, Cin=7, K=3, Lin=129, xdt=BF16, ydt=BF16, act=1, raw=True, post=1),
    C(v2(8, 2, 4), Cin=7, Cout=20, K=3, Lin=129, act=1, logscale=0, post=1, plog=0, raw=True),
    C(v2(8, 2, 4), Cin=8, Cout=5, K=7, pl=3, Lin=128, act=3, scale=0.5, acc=True),
    C(v2(8, 2, 4), Cin=9, Cout=33, K=7, pl=6, Lin=127, Lout=127, act=2, tanh=True),                 # causal
    C(v2(8, 2, 4), Cin=17, Cout=31, K=7, pl=0, Lin=122, Lout=122, bias=False, res=True),            # right-heavy
    C(v2(8, 2, 4), Cin=1, Cout=9, K=7, pl=27, dil=9, Lin=20, act=1),                                # Lin shorter than the halo
    C(v2(8, 2, 4), Cin=9, Cout=8, K=3, Lin=1, act=2, post=3),                                       # Lout 1
    C(v2(8, 2, 4, dt=BF16), Cin=9, Cout=65, K=3, Lin=200, xdt=BF16, ydt=BF16, act=1, res=True, acc=True, scale=0.7, raw=True, post=1),
    C(v2(8, 2, 4), B=1, Cin=280, Cout=272, K=7, pl=3, Lin=130, act=2),                              # packed weights > 2 MiB: co_fast off
    C(v2(8, 4, 4), B=1, Cin=8, Cout=5, K=3, Lin=BIG, act=1, post=2, raw=True),
    C(v2(8, 2, 4), B=1, Cin=8, Cout=272, K=7, pl=81, dil=27, Lin=21943, act=2),                     # halo + 512 > 640: no 8-wave tile
    C(v2(8, 8, 4), Cin=8, Cout=33, K=3, Lin=BIG, act=2, res=True, tanh=True),
    C(v2(16, 8, 4), Cin=8, Cout=64, K=3, Lin=BIG, act=1, post=1, raw=True),
    C(v2(16, 8, 4, ci=16), Cin=17, Cout=64, K=1, pl=0, Lin=BIG, act=2, acc=True, scale=1.5),
    C(v2(16, 4, 8, nw=8, ci=32), B=1, Cin=33, Cout=272, K=1, pl=0, Lin=21943, act=1, res=True, post=1, raw=True),
    C(v2(16, 8, 8, nw=8), B=1, Cin=8, Cout=272, K=7, pl=3, Lin=21943, act=2, post=3, tanh=True),
    C(v2(8, 8, 4, stride=2), Cin=9, Cout=20, K=4, stride=2, pl=1, Lin=301, act=1, post=2),
    C(v2(8, 4, 4, stride=4), Cin=9, Cout=20, K=8, stride=4, pl=2, Lin=301, act=2, raw=True, post=1),
    C(v2(16, 4, 4, stride=4), Cin=9, Cout=80, K=8, stride=4, pl=2, Lin=301, act=3, res=True),
    C(v2(8, 2, 4, stride=8), B=1, Cin=9, Cout=20, K=16, stride=8, pl=4, Lin=8192, Lout=1024, act=1),
    C(fb(), B=1, Cin=9, Cout=20, K=16, stride=8, pl=4, Lin=8200, Lout=1025, act=1),                 # Lout * B = 1025: the fallback
    C(fb(), Cin=9, Cout=20, K=6, stride=3, pl=2, Lin=301, act=1, post=1, raw=True, res=True, scale=0.5, acc=True),
    C(fb(), Cin=9, Cout=65, K=3, Lin=130, act=4, tanh=True),
    C(fb(F32, BF16), Cin=9, Cout=20, K=3, Lin=130, ydt=BF16, act=1, raw=True, post=2, res=True),
    C(fb(BF16, F32), Cin=9, Cout=20, K=3, Lin=130, xdt=BF16, act=2, res=True, acc=True),
    C(fb(), B=2, Cin=5, Cout=3, K=16, pl=67, dil=9, Lin=400, act=1),                                # Cout <= 4 with a long halo
    C(0, Cin=5, Cout=20, K=16, stride=3, pl=0, dil=27, Lin=900, Lout=100, rc=ERR_UNSUPPORTED),      # the fallback's span does not fit
]


@pytest.mark.parametrize("c", CONV_CASES, ids=_id)
def test_conv1d_fwd(kl, c):
    run_conv(kl, c)


# ================================================================================================ kalle_conv_transpose1d_fwd
def T(plan, s, **kw):
    K = 2 * s + s % 2
    kw.setdefault("pl", (s + 1) // 2)
    return C(plan, entry="convT", stride=s, K=K, **kw)


CONVT_CASES = [
    T(tv2(2, 2, 1), 2, Cout=3, Lin=40, act=1, post=1, raw=True),
    T(tv2(2, 2, 1), 5, Cout=4, Cin=7, Lin=65, act=2, tanh=True),
    T(tv2(8, 2, 4), 2, Cout=20, Lin=64, act=1, res=True),
    T(tv2(8, 2, 4), 3, Cout=9, Cin=17, Lin=65, act=2, post=2, raw=True),
    T(tv2(8, 2, 4), 4, Cout=33, Lin=63, act=3, scale=0.5),
    T(tv2(8, 2, 4), 5, Cout=20, Lin=1, act=1),
    T(tv2(8, 2, 4), 8, Cout=20, Lin=33, Lout=33 * 8 - 8, act=1),                                    # causal trim of `stride` outputs
    T(tv2(8, 2, 4), 4, Cout=20, Lin=32, Lout=31 * 4 - 4 + 8 + 2, act=2),                            # `padding` longer
    T(tv2(8, 2, 4), 8, Cout=20, Lin=128, Lout=127 * 8 - 8 + 16 + 4, act=1, post=1),                 # `padding` longer at an nq tile seam
    T(tv2(8, 2, 4, dt=BF16), 4, Cout=20, Lin=63, xdt=BF16, ydt=BF16, act=1, raw=True, post=1),
    T(tv2(8, 4, 4), 5, Cout=33, Cin=8, Lin=1062, act=1),
    T(tv2(8, 8, 4), 4, Cout=33, Cin=8, Lin=8344, act=2, post=1),
    T(tv2(16, 8, 4), 8, B=1, Cout=64, Cin=8, Lin=12316, act=1, raw=True, post=2),
    T(fb(F32, BF16, 3), 4, Cout=20, Lin=63, ydt=BF16, act=1),
    T(fb(BF16, F32, 3), 3, Cout=20, Lin=63, xdt=BF16, act=2),
    T(0, 4, Cout=20, Lin=63, ydt=BF16, res=True, rc=ERR_UNSUPPORTED),
    T(0, 4, Cout=20, Lin=63, ydt=BF16, post=2, rc=ERR_UNSUPPORTED),
    T(0, 4, Cout=20, Lin=63, ydt=BF16, raw=True, rc=ERR_UNSUPPORTED),
    T(0, 4, Cout=20, Lin=63, ydt=BF16, scale=0.5, rc=ERR_UNSUPPORTED),
    C(0, entry="convT", stride=2, K=6, pl=1, Cout=20, Lin=63, ydt=BF16, rc=ERR_UNSUPPORTED),         # ksize > 2 stride + 1
]


@pytest.mark.parametrize("c", CONVT_CASES, ids=_id)
def test_conv_transpose1d_fwd(kl, c):
    run_conv(kl, c)


# ================================================================================================ channels-per-lane kernels
def F(plan, **kw):
    return C(plan, entry="cfirst", **kw)


CFIRST_CASES = [
    F(cf(4), B=1, Cin=64, Cout=300, K=3, Lin=100, act=1, post=1, raw=True, res=True),
    F(cf(4), B=3, Cin=9, Cout=5, K=7, pl=3, Lin=17, act=2, acc=True, scale=0.5),
    F(cf(4), B=3, Cin=7, Cout=260, K=3, pl=9, dil=9, Lin=33, act=1, tanh=True),
    F(cf(2), B=3, Cin=16, Cout=256, K=1, pl=0, Lin=6000, act=2, post=2),
    F(cf(1), B=3, Cin=16, Cout=257, K=1, pl=0, Lin=11000 - 15, act=1, res=True),
    F(cf(4, 4), B=2, Cin=512, Cout=64, K=3, Lin=17, act=1, post=1, raw=True, res=True, acc=True, scale=0.7),
    F(cf(4, 1), B=2, Cin=512, Cout=64, K=3, Lin=17, act=1, post=1, raw=True, res=True, acc=True, scale=0.7, ws=False),
    F(cf(4, 16), B=1, Cin=2048, Cout=128, K=3, Lin=215, act=2),                                     # headline: 2048 -> 128 at 215
    F(cf(4, 16, 6), B=1, Cin=1024, Cout=2048, K=16, stride=8, pl=4, Lin=1720, act=1),               # headline: 1024 -> 2048 stride 8
    F(cf(4, 1, 6), B=3, Cin=9, Cout=20, K=4, stride=2, pl=1, Lin=34, act=1, post=1),                # d > 0, Lout % 16 == 1
    F(cf(4, 1, 6), B=3, Cin=9, Cout=20, K=8, stride=4, pl=2, Lin=60, act=2, raw=True, post=3),      # d > 0, Lout 15
    F(cf(4, 1, 6), B=2, Cin=9, Cout=20, K=16, stride=8, pl=8, Lin=128, act=1),                      # d == 0, Lout 16
    F(cf(2, 1), B=1, Cin=8, Cout=512, K=1, pl=0, Lin=13760, act=2),                                 # headline: 512 channels x 13760 pointwise
]
CFIRST_T_CASES = [
    C(cf(4, 1, 7), entry="cfirstT", stride=2, K=4, pl=1, B=3, Cin=9, Cout=20, Lin=17, act=1, post=1, raw=True),
    C(cf(4, 1, 7), entry="cfirstT", stride=5, K=11, pl=3, B=2, Cin=17, Cout=260, Lin=15, act=2, tanh=True),
    C(cf(4, 1, 7), entry="cfirstT", stride=8, K=16, pl=4, B=1, Cin=9, Cout=5, Lin=16, act=1, scale=0.5),
    C(cf(2, 1, 7), entry="cfirstT", stride=8, K=16, pl=4, B=1, Cin=8, Cout=256, Lin=2200, act=2),
    C(cf(1, 1, 7), entry="cfirstT", stride=8, K=16, pl=4, B=1, Cin=8, Cout=257, Lin=2100, act=1, post=2),
]


@pytest.mark.parametrize("c", CFIRST_CASES + CFIRST_T_CASES, ids=_id)
def test_conv_cfirst_fwd(kl, c):
    run_conv(kl, c)


# ================================================================================================ edges on every tile form
# Lout equal to one position tile of the form (64 LPT NW / WCO), one less, one more, two tiles +- 1 on the 16-channel forms, 1, and
# 3 (shorter than the halo: every tap of some outputs in padding); same / causal / right-heavy padding in turn; Cin of 1, 7, 8, 9,
# 17, 33 in turn (below, at, above and off the CI chunk of 8 / 16 / 32); Cout on each side of the channel-tile widths the form allows
# (the 16-channel forms need Cout >= 64 and CoutP % 16 == 0).  B is what pick_tile's cost model needs to choose the form at that size.
EDGE_CASES = [
    C(v2(2, 2, 1), B=3, Cin=1, Cout=1, K=7, stride=1, pl=3, Lin=511, Lout=511, act=2),
    C(v2(2, 2, 1), B=3, Cin=7, Cout=4, K=7, stride=1, pl=6, Lin=511, Lout=511, act=3),
    C(v2(2, 2, 1), B=3, Cin=8, Cout=1, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(2, 2, 1), B=3, Cin=9, Cout=4, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(2, 2, 1), B=3, Cin=17, Cout=1, K=7, stride=1, pl=6, Lin=513, Lout=513, act=3),
    C(v2(2, 2, 1), B=3, Cin=33, Cout=4, K=7, stride=1, pl=0, Lin=513, Lout=513, act=1),
    C(v2(2, 2, 1), B=3, Cin=1, Cout=1, K=7, stride=1, pl=3, Lin=1, Lout=1, act=2),
    C(v2(2, 2, 1), B=3, Cin=7, Cout=4, K=7, stride=1, pl=6, Lin=1, Lout=1, act=3),
    C(v2(2, 2, 1), B=3, Cin=8, Cout=1, K=7, stride=1, pl=0, Lin=3, Lout=3, act=1),
    C(v2(2, 2, 1), B=3, Cin=9, Cout=4, K=7, stride=1, pl=3, Lin=3, Lout=3, act=2),
    C(v2(8, 2, 4), B=3, Cin=1, Cout=5, K=7, stride=1, pl=3, Lin=127, Lout=127, act=2),
    C(v2(8, 2, 4), B=3, Cin=7, Cout=8, K=7, stride=1, pl=6, Lin=127, Lout=127, act=3),
    C(v2(8, 2, 4), B=3, Cin=8, Cout=5, K=7, stride=1, pl=0, Lin=128, Lout=128, act=1),
    C(v2(8, 2, 4), B=3, Cin=9, Cout=8, K=7, stride=1, pl=3, Lin=128, Lout=128, act=2),
    C(v2(8, 2, 4), B=3, Cin=17, Cout=9, K=7, stride=1, pl=6, Lin=128, Lout=128, act=3),
    C(v2(8, 2, 4), B=3, Cin=33, Cout=31, K=7, stride=1, pl=0, Lin=128, Lout=128, act=1),
    C(v2(8, 2, 4), B=3, Cin=1, Cout=32, K=7, stride=1, pl=3, Lin=128, Lout=128, act=2),
    C(v2(8, 2, 4), B=3, Cin=7, Cout=33, K=7, stride=1, pl=6, Lin=128, Lout=128, act=3),
    C(v2(8, 2, 4), B=3, Cin=8, Cout=63, K=7, stride=1, pl=0, Lin=128, Lout=128, act=1),
    C(v2(8, 2, 4), B=3, Cin=9, Cout=64, K=7, stride=1, pl=3, Lin=128, Lout=128, act=2),
    C(v2(8, 2, 4), B=3, Cin=17, Cout=65, K=7, stride=1, pl=6, Lin=128, Lout=128, act=3),
    C(v2(8, 2, 4), B=3, Cin=33, Cout=127, K=7, stride=1, pl=0, Lin=128, Lout=128, act=1),
    C(v2(8, 2, 4), B=3, Cin=1, Cout=128, K=7, stride=1, pl=3, Lin=128, Lout=128, act=2),
    C(v2(8, 2, 4), B=3, Cin=7, Cout=129, K=7, stride=1, pl=6, Lin=128, Lout=128, act=3),
    C(v2(8, 2, 4), B=3, Cin=8, Cout=5, K=7, stride=1, pl=0, Lin=129, Lout=129, act=1),
    C(v2(8, 2, 4), B=3, Cin=9, Cout=8, K=7, stride=1, pl=3, Lin=129, Lout=129, act=2),
    C(v2(8, 2, 4), B=3, Cin=17, Cout=9, K=7, stride=1, pl=6, Lin=129, Lout=129, act=3),
    C(v2(8, 2, 4), B=3, Cin=33, Cout=31, K=7, stride=1, pl=0, Lin=129, Lout=129, act=1),
    C(v2(8, 2, 4), B=3, Cin=1, Cout=32, K=7, stride=1, pl=3, Lin=129, Lout=129, act=2),
    C(v2(8, 2, 4), B=3, Cin=7, Cout=33, K=7, stride=1, pl=6, Lin=129, Lout=129, act=3),
    C(v2(8, 2, 4), B=3, Cin=8, Cout=63, K=7, stride=1, pl=0, Lin=129, Lout=129, act=1),
    C(v2(8, 2, 4), B=3, Cin=9, Cout=64, K=7, stride=1, pl=3, Lin=129, Lout=129, act=2),
    C(v2(8, 2, 4), B=3, Cin=17, Cout=65, K=7, stride=1, pl=6, Lin=129, Lout=129, act=3),
    C(v2(8, 2, 4), B=3, Cin=33, Cout=127, K=7, stride=1, pl=0, Lin=129, Lout=129, act=1),
    C(v2(8, 2, 4), B=3, Cin=1, Cout=128, K=7, stride=1, pl=3, Lin=129, Lout=129, act=2),
    C(v2(8, 2, 4), B=3, Cin=7, Cout=129, K=7, stride=1, pl=6, Lin=129, Lout=129, act=3),
    C(v2(8, 2, 4), B=3, Cin=8, Cout=5, K=7, stride=1, pl=0, Lin=1, Lout=1, act=1),
    C(v2(8, 2, 4), B=3, Cin=9, Cout=8, K=7, stride=1, pl=3, Lin=1, Lout=1, act=2),
    C(v2(8, 2, 4), B=3, Cin=17, Cout=5, K=7, stride=1, pl=6, Lin=3, Lout=3, act=3),
    C(v2(8, 2, 4), B=3, Cin=33, Cout=8, K=7, stride=1, pl=0, Lin=3, Lout=3, act=1),
    C(v2(8, 4, 4), B=140, Cin=1, Cout=5, K=7, stride=1, pl=3, Lin=255, Lout=255, act=2),
    C(v2(8, 4, 4), B=140, Cin=7, Cout=8, K=7, stride=1, pl=6, Lin=255, Lout=255, act=3),
    C(v2(8, 4, 4), B=140, Cin=8, Cout=5, K=7, stride=1, pl=0, Lin=256, Lout=256, act=1),
    C(v2(8, 4, 4), B=140, Cin=9, Cout=8, K=7, stride=1, pl=3, Lin=256, Lout=256, act=2),
    C(v2(8, 4, 4), B=140, Cin=17, Cout=9, K=7, stride=1, pl=6, Lin=256, Lout=256, act=3),
    C(v2(8, 4, 4), B=140, Cin=33, Cout=31, K=7, stride=1, pl=0, Lin=256, Lout=256, act=1),
    C(v2(8, 4, 4), B=70, Cin=1, Cout=33, K=7, stride=1, pl=3, Lin=256, Lout=256, act=2),
    C(v2(8, 4, 4), B=50, Cin=7, Cout=65, K=7, stride=1, pl=6, Lin=256, Lout=256, act=3),
    C(v2(8, 4, 4), B=30, Cin=8, Cout=129, K=7, stride=1, pl=0, Lin=256, Lout=256, act=1),
    C(v2(8, 4, 4), B=90, Cin=9, Cout=5, K=7, stride=1, pl=3, Lin=257, Lout=257, act=2),
    C(v2(8, 4, 4), B=90, Cin=17, Cout=8, K=7, stride=1, pl=6, Lin=257, Lout=257, act=3),
    C(v2(8, 4, 4), B=90, Cin=33, Cout=9, K=7, stride=1, pl=0, Lin=257, Lout=257, act=1),
    C(v2(8, 4, 4), B=90, Cin=1, Cout=31, K=7, stride=1, pl=3, Lin=257, Lout=257, act=2),
    C(v2(8, 4, 4), B=50, Cin=7, Cout=33, K=7, stride=1, pl=6, Lin=257, Lout=257, act=3),
    C(v2(8, 4, 4), B=30, Cin=8, Cout=65, K=7, stride=1, pl=0, Lin=257, Lout=257, act=1),
    C(v2(8, 4, 4), B=20, Cin=9, Cout=129, K=7, stride=1, pl=3, Lin=257, Lout=257, act=2),
    C(v2(8, 8, 4), B=400, Cin=1, Cout=5, K=7, stride=1, pl=3, Lin=511, Lout=511, act=2),
    C(v2(8, 8, 4), B=400, Cin=7, Cout=9, K=7, stride=1, pl=6, Lin=511, Lout=511, act=3),
    C(v2(8, 8, 4), B=400, Cin=8, Cout=5, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(8, 8, 4), B=400, Cin=9, Cout=9, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(8, 8, 4), B=400, Cin=17, Cout=31, K=7, stride=1, pl=6, Lin=512, Lout=512, act=3),
    C(v2(8, 8, 4), B=200, Cin=33, Cout=33, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(8, 8, 4), B=200, Cin=1, Cout=63, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(8, 8, 4), B=140, Cin=7, Cout=65, K=7, stride=1, pl=6, Lin=512, Lout=512, act=3),
    C(v2(8, 8, 4), B=80, Cin=8, Cout=129, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(8, 8, 4), B=160, Cin=1, Cout=33, K=7, stride=1, pl=3, Lin=513, Lout=513, act=2),
    C(v2(8, 8, 4), B=160, Cin=7, Cout=63, K=7, stride=1, pl=6, Lin=513, Lout=513, act=3),
    C(v2(8, 8, 4), B=120, Cin=8, Cout=65, K=7, stride=1, pl=0, Lin=513, Lout=513, act=1),
    C(v2(8, 8, 4), B=70, Cin=9, Cout=129, K=7, stride=1, pl=3, Lin=513, Lout=513, act=2),
    C(v2(16, 8, 4), B=200, Cin=1, Cout=64, K=7, stride=1, pl=3, Lin=511, Lout=511, act=2),
    C(v2(16, 8, 4), B=200, Cin=8, Cout=64, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(16, 8, 4), B=100, Cin=17, Cout=127, K=7, stride=1, pl=6, Lin=512, Lout=512, act=3),
    C(v2(16, 8, 4), B=100, Cin=33, Cout=128, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(16, 8, 4), B=80, Cin=1, Cout=144, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(16, 8, 4, ci=16), B=200, Cin=1, Cout=64, K=1, stride=1, pl=0, Lin=511, Lout=511, act=2),
    C(v2(16, 8, 4, ci=16), B=200, Cin=7, Cout=64, K=1, stride=1, pl=0, Lin=512, Lout=512, act=3),
    C(v2(16, 4, 8, nw=8, ci=32), B=200, Cin=8, Cout=127, K=1, stride=1, pl=0, Lin=257, Lout=257, act=1),
    C(v2(16, 4, 8, nw=8, ci=32), B=200, Cin=9, Cout=128, K=1, stride=1, pl=0, Lin=257, Lout=257, act=2),
    C(v2(16, 4, 8, nw=8, ci=32), B=160, Cin=17, Cout=144, K=1, stride=1, pl=0, Lin=257, Lout=257, act=3),
    C(v2(16, 4, 8, nw=8, ci=32), B=90, Cin=33, Cout=272, K=1, stride=1, pl=0, Lin=257, Lout=257, act=1),
    C(v2(16, 8, 8, nw=8), B=50, Cin=1, Cout=256, K=7, stride=1, pl=3, Lin=511, Lout=511, act=2),
    C(v2(16, 8, 8, nw=8), B=50, Cin=7, Cout=272, K=7, stride=1, pl=6, Lin=511, Lout=511, act=3),
    C(v2(16, 8, 8, nw=8), B=50, Cin=8, Cout=256, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(16, 8, 8, nw=8), B=50, Cin=9, Cout=272, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=1, Cout=5, K=4, stride=2, pl=1, Lin=1022, Lout=511, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=7, Cout=9, K=4, stride=2, pl=1, Lin=1022, Lout=511, act=3),
    C(v2(8, 8, 4, stride=2), B=3, Cin=8, Cout=5, K=4, stride=2, pl=1, Lin=1024, Lout=512, act=1),
    C(v2(8, 8, 4, stride=2), B=3, Cin=9, Cout=9, K=4, stride=2, pl=1, Lin=1024, Lout=512, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=17, Cout=33, K=4, stride=2, pl=1, Lin=1024, Lout=512, act=3),
    C(v2(8, 8, 4, stride=2), B=3, Cin=33, Cout=65, K=4, stride=2, pl=1, Lin=1024, Lout=512, act=1),
    C(v2(8, 8, 4, stride=2), B=3, Cin=1, Cout=129, K=4, stride=2, pl=1, Lin=1024, Lout=512, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=7, Cout=5, K=4, stride=2, pl=1, Lin=1026, Lout=513, act=3),
    C(v2(8, 8, 4, stride=2), B=3, Cin=8, Cout=9, K=4, stride=2, pl=1, Lin=1026, Lout=513, act=1),
    C(v2(8, 8, 4, stride=2), B=3, Cin=9, Cout=33, K=4, stride=2, pl=1, Lin=1026, Lout=513, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=17, Cout=65, K=4, stride=2, pl=1, Lin=1026, Lout=513, act=3),
    C(v2(8, 8, 4, stride=2), B=3, Cin=33, Cout=129, K=4, stride=2, pl=1, Lin=1026, Lout=513, act=1),
    C(v2(8, 8, 4, stride=2), B=3, Cin=1, Cout=5, K=4, stride=2, pl=1, Lin=2, Lout=1, act=2),
    C(v2(8, 8, 4, stride=2), B=3, Cin=7, Cout=9, K=4, stride=2, pl=1, Lin=2, Lout=1, act=3),
    C(v2(8, 8, 4, stride=2), B=3, Cin=8, Cout=5, K=4, stride=2, pl=1, Lin=6, Lout=3, act=1),
    C(v2(8, 8, 4, stride=2), B=3, Cin=9, Cout=9, K=4, stride=2, pl=1, Lin=6, Lout=3, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=1, Cout=5, K=8, stride=4, pl=2, Lin=1020, Lout=255, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=7, Cout=9, K=8, stride=4, pl=2, Lin=1020, Lout=255, act=3),
    C(v2(8, 4, 4, stride=4), B=3, Cin=8, Cout=5, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=1),
    C(v2(8, 4, 4, stride=4), B=3, Cin=9, Cout=9, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=17, Cout=33, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=3),
    C(v2(8, 4, 4, stride=4), B=3, Cin=33, Cout=63, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=1),
    C(v2(8, 4, 4, stride=4), B=3, Cin=1, Cout=65, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=7, Cout=5, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=3),
    C(v2(8, 4, 4, stride=4), B=3, Cin=8, Cout=9, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=1),
    C(v2(8, 4, 4, stride=4), B=3, Cin=9, Cout=33, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=17, Cout=63, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=3),
    C(v2(8, 4, 4, stride=4), B=3, Cin=33, Cout=65, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=1),
    C(v2(8, 4, 4, stride=4), B=3, Cin=1, Cout=5, K=8, stride=4, pl=2, Lin=4, Lout=1, act=2),
    C(v2(8, 4, 4, stride=4), B=3, Cin=7, Cout=9, K=8, stride=4, pl=2, Lin=4, Lout=1, act=3),
    C(v2(8, 4, 4, stride=4), B=3, Cin=8, Cout=5, K=8, stride=4, pl=2, Lin=12, Lout=3, act=1),
    C(v2(8, 4, 4, stride=4), B=3, Cin=9, Cout=9, K=8, stride=4, pl=2, Lin=12, Lout=3, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=1, Cout=64, K=8, stride=4, pl=2, Lin=1020, Lout=255, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=7, Cout=80, K=8, stride=4, pl=2, Lin=1020, Lout=255, act=3),
    C(v2(16, 4, 4, stride=4), B=3, Cin=8, Cout=64, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=1),
    C(v2(16, 4, 4, stride=4), B=3, Cin=9, Cout=80, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=17, Cout=128, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=3),
    C(v2(16, 4, 4, stride=4), B=3, Cin=33, Cout=144, K=8, stride=4, pl=2, Lin=1024, Lout=256, act=1),
    C(v2(16, 4, 4, stride=4), B=3, Cin=1, Cout=64, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=7, Cout=80, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=3),
    C(v2(16, 4, 4, stride=4), B=3, Cin=8, Cout=128, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=1),
    C(v2(16, 4, 4, stride=4), B=3, Cin=9, Cout=144, K=8, stride=4, pl=2, Lin=1028, Lout=257, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=17, Cout=64, K=8, stride=4, pl=2, Lin=4, Lout=1, act=3),
    C(v2(16, 4, 4, stride=4), B=3, Cin=33, Cout=80, K=8, stride=4, pl=2, Lin=4, Lout=1, act=1),
    C(v2(16, 4, 4, stride=4), B=3, Cin=1, Cout=64, K=8, stride=4, pl=2, Lin=12, Lout=3, act=2),
    C(v2(16, 4, 4, stride=4), B=3, Cin=7, Cout=80, K=8, stride=4, pl=2, Lin=12, Lout=3, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=1, Cout=5, K=16, stride=8, pl=4, Lin=1016, Lout=127, act=2),
    C(v2(8, 2, 4, stride=8), B=3, Cin=7, Cout=9, K=16, stride=8, pl=4, Lin=1016, Lout=127, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=8, Cout=5, K=16, stride=8, pl=4, Lin=1024, Lout=128, act=1),
    C(v2(8, 2, 4, stride=8), B=3, Cin=9, Cout=9, K=16, stride=8, pl=4, Lin=1024, Lout=128, act=2),
    C(v2(8, 2, 4, stride=8), B=3, Cin=17, Cout=33, K=16, stride=8, pl=4, Lin=1024, Lout=128, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=33, Cout=65, K=16, stride=8, pl=4, Lin=1024, Lout=128, act=1),
    C(v2(8, 2, 4, stride=8), B=3, Cin=1, Cout=129, K=16, stride=8, pl=4, Lin=1024, Lout=128, act=2),
    C(v2(8, 2, 4, stride=8), B=3, Cin=7, Cout=5, K=16, stride=8, pl=4, Lin=1032, Lout=129, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=8, Cout=9, K=16, stride=8, pl=4, Lin=1032, Lout=129, act=1),
    C(v2(8, 2, 4, stride=8), B=3, Cin=9, Cout=33, K=16, stride=8, pl=4, Lin=1032, Lout=129, act=2),
    C(v2(8, 2, 4, stride=8), B=3, Cin=17, Cout=65, K=16, stride=8, pl=4, Lin=1032, Lout=129, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=33, Cout=129, K=16, stride=8, pl=4, Lin=1032, Lout=129, act=1),
    C(v2(8, 2, 4, stride=8), B=3, Cin=1, Cout=5, K=16, stride=8, pl=4, Lin=8, Lout=1, act=2),
    C(v2(8, 2, 4, stride=8), B=3, Cin=7, Cout=9, K=16, stride=8, pl=4, Lin=8, Lout=1, act=3),
    C(v2(8, 2, 4, stride=8), B=3, Cin=8, Cout=5, K=16, stride=8, pl=4, Lin=24, Lout=3, act=1),
    C(v2(8, 2, 4, stride=8), B=3, Cin=9, Cout=9, K=16, stride=8, pl=4, Lin=24, Lout=3, act=2),
    C(v2(8, 8, 4), B=308, Cin=17, Cout=5, K=7, stride=1, pl=3, Lin=513, Lout=513, act=2),
    C(v2(8, 8, 4), B=154, Cin=7, Cout=33, K=7, stride=1, pl=0, Lin=513, Lout=513, act=3),
    C(v2(8, 8, 4), B=103, Cin=33, Cout=65, K=7, stride=1, pl=3, Lin=513, Lout=513, act=1),
    C(v2(16, 8, 4), B=193, Cin=17, Cout=64, K=7, stride=1, pl=3, Lin=511, Lout=511, act=2),
    C(v2(16, 8, 4), B=97, Cin=7, Cout=128, K=7, stride=1, pl=0, Lin=511, Lout=511, act=3),
    C(v2(16, 8, 4), B=77, Cin=33, Cout=144, K=7, stride=1, pl=3, Lin=511, Lout=511, act=1),
    C(v2(16, 8, 4), B=193, Cin=8, Cout=64, K=7, stride=1, pl=6, Lin=512, Lout=512, act=2),
    C(v2(16, 8, 4), B=97, Cin=1, Cout=128, K=7, stride=1, pl=3, Lin=512, Lout=512, act=3),
    C(v2(16, 8, 4), B=77, Cin=9, Cout=144, K=7, stride=1, pl=0, Lin=512, Lout=512, act=1),
    C(v2(16, 8, 4), B=97, Cin=17, Cout=64, K=7, stride=1, pl=3, Lin=1023, Lout=1023, act=2),
    C(v2(16, 8, 4), B=49, Cin=7, Cout=128, K=7, stride=1, pl=6, Lin=1023, Lout=1023, act=3),
    C(v2(16, 8, 4), B=39, Cin=33, Cout=144, K=7, stride=1, pl=3, Lin=1023, Lout=1023, act=1),
    C(v2(16, 8, 4), B=97, Cin=8, Cout=64, K=7, stride=1, pl=0, Lin=1024, Lout=1024, act=2),
    C(v2(16, 8, 4), B=49, Cin=1, Cout=128, K=7, stride=1, pl=3, Lin=1024, Lout=1024, act=3),
    C(v2(16, 8, 4), B=39, Cin=9, Cout=144, K=7, stride=1, pl=6, Lin=1024, Lout=1024, act=1),
    C(v2(16, 8, 4), B=154, Cin=17, Cout=64, K=7, stride=1, pl=3, Lin=1025, Lout=1025, act=2),
    C(v2(16, 8, 4), B=77, Cin=7, Cout=128, K=7, stride=1, pl=0, Lin=1025, Lout=1025, act=3),
    C(v2(16, 8, 4, ci=16), B=193, Cin=33, Cout=64, K=1, stride=1, pl=0, Lin=511, Lout=511, act=1),
    C(v2(16, 8, 4, ci=16), B=193, Cin=8, Cout=64, K=1, stride=1, pl=0, Lin=512, Lout=512, act=2),
    C(v2(16, 8, 4, ci=16), B=97, Cin=1, Cout=64, K=1, stride=1, pl=0, Lin=1023, Lout=1023, act=3),
    C(v2(16, 8, 4, ci=16), B=97, Cin=9, Cout=64, K=1, stride=1, pl=0, Lin=1024, Lout=1024, act=1),
    C(v2(16, 8, 4, ci=16), B=154, Cin=17, Cout=64, K=1, stride=1, pl=0, Lin=1025, Lout=1025, act=2),
    C(v2(16, 4, 8, nw=8, ci=32), B=97, Cin=7, Cout=128, K=1, stride=1, pl=0, Lin=511, Lout=511, act=3),
    C(v2(16, 4, 8, nw=8, ci=32), B=43, Cin=33, Cout=272, K=1, stride=1, pl=0, Lin=511, Lout=511, act=1),
    C(v2(16, 4, 8, nw=8, ci=32), B=97, Cin=8, Cout=128, K=1, stride=1, pl=0, Lin=512, Lout=512, act=2),
    C(v2(16, 4, 8, nw=8, ci=32), B=43, Cin=1, Cout=272, K=1, stride=1, pl=0, Lin=512, Lout=512, act=3),
    C(v2(16, 4, 8, nw=8, ci=32), B=49, Cin=9, Cout=128, K=1, stride=1, pl=0, Lin=1023, Lout=1023, act=1),
    C(v2(16, 4, 8, nw=8, ci=32), B=22, Cin=17, Cout=272, K=1, stride=1, pl=0, Lin=1023, Lout=1023, act=2),
    C(v2(16, 4, 8, nw=8, ci=32), B=49, Cin=7, Cout=128, K=1, stride=1, pl=0, Lin=1024, Lout=1024, act=3),
    C(v2(16, 4, 8, nw=8, ci=32), B=22, Cin=33, Cout=272, K=1, stride=1, pl=0, Lin=1024, Lout=1024, act=1),
    C(v2(16, 4, 8, nw=8, ci=32), B=77, Cin=8, Cout=128, K=1, stride=1, pl=0, Lin=1025, Lout=1025, act=2),
    C(v2(16, 8, 8, nw=8), B=49, Cin=1, Cout=256, K=7, stride=1, pl=3, Lin=511, Lout=511, act=3),
    C(v2(16, 8, 8, nw=8), B=43, Cin=9, Cout=272, K=7, stride=1, pl=0, Lin=511, Lout=511, act=1),
    C(v2(16, 8, 8, nw=8), B=49, Cin=17, Cout=256, K=7, stride=1, pl=3, Lin=512, Lout=512, act=2),
    C(v2(16, 8, 8, nw=8), B=43, Cin=7, Cout=272, K=7, stride=1, pl=6, Lin=512, Lout=512, act=3),
    C(v2(16, 8, 8, nw=8), B=25, Cin=33, Cout=256, K=7, stride=1, pl=3, Lin=1023, Lout=1023, act=1),
    C(v2(16, 8, 8, nw=8), B=22, Cin=8, Cout=272, K=7, stride=1, pl=0, Lin=1023, Lout=1023, act=2),
    C(v2(16, 8, 8, nw=8), B=25, Cin=1, Cout=256, K=7, stride=1, pl=3, Lin=1024, Lout=1024, act=3),
    C(v2(16, 8, 8, nw=8), B=22, Cin=9, Cout=272, K=7, stride=1, pl=6, Lin=1024, Lout=1024, act=1),
    C(v2(16, 8, 8, nw=8), B=39, Cin=17, Cout=256, K=7, stride=1, pl=3, Lin=1025, Lout=1025, act=2),
]
CFIRST_EDGES = [F(cf(4), B=3, Cin=ci, Cout=co, K=K, pl=pl, dil=dil, Lin=L, Lout=L, act=1 + (ci + co) % 3)
                for (ci, co, K, pl, dil, L) in [(1, 1, 7, 3, 1, 1), (7, 4, 7, 6, 1, 15), (8, 5, 7, 0, 1, 16), (9, 8, 7, 3, 1, 17), (17, 9, 3, 9, 9, 31),
                                                (33, 255, 3, 1, 1, 32), (8, 256, 3, 2, 1, 33), (9, 257, 3, 0, 1, 3), (1, 31, 1, 0, 1, 17),
                                                (7, 33, 7, 27, 9, 20), (9, 64, 7, 54, 9, 47), (8, 65, 7, 0, 9, 49)]]
CFIRST_EDGES += [F(cf(4, 1, 6), B=3, Cin=ci, Cout=co, K=2 * s, stride=s, pl=pl, Lin=(L - 1) * s + 2 * s - 2 * pl, Lout=L, act=1 + ci % 3)
                 for (ci, co, s, pl, L) in [(1, 5, 2, 1, 17), (7, 9, 4, 2, 17), (9, 257, 8, 4, 17), (8, 4, 4, 1, 16), (9, 8, 8, 3, 15), (17, 1, 2, 1, 1)]]
CFIRST_EDGES += [C(cf(4, 1, 7), entry="cfirstT", stride=s, K=2 * s + s % 2, pl=(s + 1) // 2, B=3, Cin=ci, Cout=co, Lin=L, act=1 + ci % 3)
                 for (ci, co, s, L) in [(1, 1, 2, 1), (7, 4, 3, 15), (8, 5, 4, 16), (9, 9, 5, 17), (17, 257, 8, 3), (9, 255, 2, 33)]]


@pytest.mark.parametrize("c", EDGE_CASES + CFIRST_EDGES, ids=_id)
def test_conv_edges(kl, c):
    run_conv(kl, c)


# ================================================================================================ epilogue / activation cover
COVER_PATHS = {
    # name: (base case, dtype values, input activations)
    "v2_4wave": (C(v2(8, 2, 4), Cin=9, Cout=20, K=3, Lin=200), ["ff", "bb"], [0, 1, 2, 3]),
    "v2_8wave": (C(v2(16, 8, 8, nw=8), B=1, Cin=8, Cout=272, K=7, pl=3, Lin=21943), ["ff", "bb"], [0, 1, 2, 3]),
    "fallback": (C(fb(), Cin=9, Cout=20, K=6, stride=3, pl=2, Lin=301), ["ff", "bb", "fb", "bf"], [0, 1, 2, 3, 4]),
    "cfirst": (F(cf(4), B=1, Cin=64, Cout=300, K=3, Lin=100), ["ff"], [0, 1, 2, 3]),
    "cfirst_ks": (F(cf(4, 4), B=2, Cin=512, Cout=64, K=3, Lin=17), ["ff"], [0, 1, 2, 3]),
    "convT_v2": (T(tv2(8, 2, 4), 4, Cout=20, Lin=63), ["ff", "bb"], [0, 1, 2, 3]),
    "cfirstT": (C(cf(4, 1, 7), entry="cfirstT", stride=2, K=4, pl=1, B=3, Cin=9, Cout=20, Lin=17), ["ff"], [0, 1, 2, 3]),
}


def _cover_factors(name):
    _, dts, acts = COVER_PATHS[name]
    return {"act": acts, "logscale": [1, 0], "bias": [True, False], "res": [False, True], "scale": [1.0, 0.5], "acc": [False, True],
            "post": [0, 1, 2, 3], "plog": [1, 0], "tanh": [False, True], "raw": [False, True], "dt": dts}


def _cover_cases():
    out = []
    for i, name in enumerate(COVER_PATHS):
        base = COVER_PATHS[name][0]
        for row in ne._pairwise(_cover_factors(name), lambda c: True, 20261017 + i):
            c = dict(base)
            c.update({k: v for k, v in row.items() if k != "dt"})
            dt = row["dt"]
            c["xdt"], c["ydt"] = (F32 if dt[0] == "f" else BF16), (F32 if dt[1] == "f" else BF16)
            if name == "fallback":
                c["plan"] = fb(c["xdt"], c["ydt"])
            elif dt == "bb":
                c["plan"] = base["plan"] & ~0x30
            out.append(pytest.param(c, id=name + "-" + "-".join(f"{k}{v:g}" if isinstance(v, float) else f"{k}{int(v) if isinstance(v, bool) else v}"
                                                               for k, v in row.items())))
    return out


def test_cover_is_pairwise_complete():
    """(host side) every pair of option values appears in some case of every path"""
    for i, name in enumerate(COVER_PATHS):
        f = _cover_factors(name)
        ne._cover_complete(f, lambda c: True, ne._pairwise(f, lambda c: True, 20261017 + i))


@pytest.mark.parametrize("c", _cover_cases())
def test_conv_epilogue_activation_cover(kl, c):
    """pairwise cover of in_act x logscale x bias x residual x out_scale x accumulate x post_act x its logscale x tanh x y_raw x
    dtype on a 4-wave v2 form, an 8-wave form, the fallback (with the gate and both mixed dtype pairs), the channels-per-lane
    kernel without and with the finishing kernel (ks > 1), the transposed v2 kernel and the transposed channels-per-lane kernel"""
    run_conv(kl, c)


# ================================================================================================ weight-norm fold
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("d0,d1,K", [(5, 11, 4), (16, 9, 7), (33, 1, 1), (1, 20, 16)])
def test_weight_norm_fold(kl, flags, d0, d1, K):
    """repack only: bit-exact, pad columns exactly 0; with g: the n-term bound on the norm + the division allowance"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(7)
    v, gg = _randn((d0, d1, K), g), 1 + 0.3 * _randn((d0,), g)
    cout = d1 if flags & 1 else d0
    cin = d0 if flags & 1 else d1
    for with_g in (False, True):
        wbuf, w = _guarded(torch.full((cin, K, (cout + 7) // 8 * 8), NAN, device="cuda"))
        assert lib.kalle_weight_norm_fold(P(_guarded(v)[1]), P(gg) if with_g else None, P(w), d0, d1, K, flags, st) == 0
        torch.cuda.synchronize()
        ref = kr.weight_norm_fold(v.double(), gg.double() if with_g else None, flags)
        if not with_g:
            _exact(w, ref.float(), f"fold flags {flags}")
        else:
            n = d1 * K
            _check(w, ref, ((n + 2) / 2 * U + (ALLOW["DIV"] + 2) * U) * ref.abs(), f"fold flags {flags} g")
        assert (w[:, :, cout:] == 0).all()
        _clean(wbuf, w, "fold")


# ================================================================================================ weight gradient
def W(plan, **kw):
    c = dict(B=3, CU=9, CV=20, K=7, stride=1, pl=3, dil=1, LV=300, act_on=0, act=0, plan=plan, wrong=None)
    c.update(kw)
    return c


WGRAD_CASES = [
    W(wg_lds(16, 1), K=1, pl=0, CV=16, act=1),
    W(wg_lds(16, 4), K=4, stride=2, pl=1, CV=17, act=2),
    W(wg_lds(16, 7), K=7, CV=63, LV=257),
    W(wg_lds(16, 7), K=7, CV=64, pl=27, dil=9, act=1),
    W(wg_lds(16, 8), K=8, stride=4, pl=2, CV=65, act=2),
    W(wg_lds(8, 16), K=16, stride=8, pl=4, CV=20, CU=5, LV=2000, act=1),
    W(wg_lds(16, 7), K=7, stride=3, pl=2, CV=20, act_on=1, act=0),
    W(wg_lane(4, 4, 8), K=5, pl=2, CV=20, act=1),
    W(wg_lane(2, 4, 16), K=11, stride=5, pl=3, CV=33, act=2),
    W(wg_lane(4, 4, 8), K=7, CV=15, act=1),                                # fewer than 16 V channels
    W(wg_lane(4, 8, 4), K=4, stride=2, pl=1, CV=20, act_on=1, act=1),      # the activation on U
    W(wg_lane(4, 4, 8), K=7, stride=6, pl=3, CV=20, act_on=1, act=2),
    W(wg_lane(2, 4, 16), K=16, stride=7, pl=4, CV=9, CU=17, act=0),
]


def run_wgrad(kl, c, wrong=None):
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(3)
    B, CU, CV, K, stride, pl, dil, LV = (c[k] for k in ("B", "CU", "CV", "K", "stride", "pl", "dil", "LV"))
    MU = (LV + 2 * pl - dil * (K - 1) - 1) // stride + 1
    Ub, Um = _guarded(_randn((B, CU, MU), g))
    Vb, Vm = _guarded(_randn((B, CV, LV), g, 1.5))
    ca = CV if c["act_on"] == 0 else CU
    al, be = _act_vals(g, ca)
    before = _randn((CU, CV, K), g)
    dWb, dW = _guarded(before.clone())
    ia = _act_struct(L, c["act"], al if c["act"] == 1 else None, be if c["act"] == 1 else None, 1)
    rc = lib.kalle_conv_wgrad(P(Um), P(Vm), P(dW), B, CU, CV, MU, LV, K, stride, pl, dil, c["act_on"], ctypes.addressof(ia), st)
    plan = lib.kalle_conv_last_plan()
    torch.cuda.synchronize()
    what = f"wgrad {c}"
    assert rc == 0 and plan == c["plan"], (what, rc, hex(plan), hex(c["plan"]))
    PLANS_SEEN.add(plan)
    args = (c["act"], al, be, 1, 0.0)
    ref, asum = kr.conv_wgrad(Um.double(), Vm.double(), K, stride, pl + (1 if wrong == "padding_off_by_one" else 0), dil, c["act_on"], args)
    src = Vm.double() if c["act_on"] == 0 else Um.double()
    ex = _act_err(src, c["act"], al, be, 1, 0.0)
    eprop = kr.conv_wgrad(*((Um.double().abs(), ex) if c["act_on"] == 0 else (ex, Vm.double().abs())), K, stride, pl, dil)[0] if c["act"] else 0.0
    n = B * MU + 1
    _check(dW, before.double() + ref, n * U * (asum + before.double().abs()) + eprop + 1e-30, what)
    _clean(dWb, dW, what)


@pytest.mark.parametrize("c", WGRAD_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k not in ("plan", "wrong", "B")))
def test_conv_wgrad(kl, c):
    run_wgrad(kl, c)


# ================================================================================================ small backward kernels
@pytest.mark.parametrize("code,logscale", [(0, 0), (1, 0), (1, 1), (2, 0)])
@pytest.mark.parametrize("B,Cn,Ln", [(2, 5, 8191), (1, 3, 8193), (3, 4, 8192), (2, 32769, 9)])      # (the last: B C > 65535 rows on grid x)
def test_act_bwd(kl, code, logscale, B, Cn, Ln):
    """dx per element; dalpha / dbeta accumulate into random contents (n-term bound over B L positions)"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(11)
    xb, x = _guarded(_randn((B, Cn, Ln), g, 1.5))
    gb, gr = _guarded(_randn((B, Cn, Ln), g))
    al, be = _act_vals(g, Cn)
    if not logscale:
        al, be = al.exp(), be.exp()
    dxb, dx = _guarded(torch.full((B, Cn, Ln), NAN, device="cuda"))
    a0, b0 = _randn((Cn,), g), _randn((Cn,), g)
    dab, da = _guarded(a0.clone())
    dbb, db = _guarded(b0.clone())
    ia = _act_struct(L, code, al if code == 1 else None, be if code == 1 else None, logscale)
    if code == 1:
        assert lib.kalle_act_bwd(P(x), P(gr), P(dx), ctypes.addressof(ia), P(da), None, B, Cn, Ln, st) == ERR_ARG
        assert torch.isnan(dx).all()
    assert lib.kalle_act_bwd(P(x), P(gr), P(dx), ctypes.addressof(ia), P(da), P(db), B, Cn, Ln, st) == 0
    torch.cuda.synchronize()
    xd, gd = x.double(), gr.double()
    rdx, rda, rdb, absab = kr.act_bwd(xd, gd, code, al, be, logscale)
    if code == 1:
        a, b = kr._act_ab(al, be, logscale)
        a3, b3 = a[None, :, None], b[None, :, None] + 1e-9
        unit = (1 + (a3 * xd).abs()) / b3
        tol = gd.abs() * (ALLOW["SNAKE"] * U * 2 * a3 * unit + 4 * U * (1 + a3 / b3))
        _check(dx, rdx, tol, "act_bwd dx")
        lg = (a, b) if logscale else (1.0, 1.0)
        ea = (gd.abs() * (ALLOW["SNAKE"] * U * 2 * unit * xd.abs() + 6 * U * xd.abs() / b3)).sum((0, 2)) * lg[0]
        eb = (gd.abs() * (ALLOW["SNAKE"] * U * 2 * unit / b3 + 6 * U / b3.pow(2))).sum((0, 2)) * lg[1]
        n = B * Ln + 2
        _check(da, a0.double() + rda, n * U * (absab[0] + a0.double().abs()) + ea, "act_bwd dalpha")
        _check(db, b0.double() + rdb, n * U * (absab[1] + b0.double().abs()) + eb, "act_bwd dbeta")
    else:
        _check(dx, rdx, gd.abs() * (ALLOW["ELU"] + 2) * U, "act_bwd dx")
        _exact(da, a0, "dalpha untouched")
    for buf, view in ((dxb, dx), (dab, da), (dbb, db)):
        _clean(buf, view, "act_bwd")


def test_tanh_bwd_upsample_channel_sum_weight_norm_bwd(kl):
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(13)
    n = 70001
    dy, y = _guarded(_randn((n,), g))[1], _guarded(torch.tanh(_randn((n,), g, 2.0)))[1]
    ob, o = _guarded(torch.full((n,), NAN, device="cuda"))
    assert lib.kalle_tanh_bwd(P(dy), P(y), P(o), n, st) == 0
    torch.cuda.synchronize()
    _check(o, kr.tanh_bwd(dy.double(), y.double()), 3 * U * dy.double().abs() * (1 + y.double().pow(2)), "tanh_bwd")
    _clean(ob, o, "tanh_bwd")
    for scale in (1, 2, 7, 64):
        rows, Ln = 5, 37
        x = _guarded(_randn((rows, Ln), g))[1]
        ub, up = _guarded(torch.full((rows, Ln * scale), NAN, device="cuda"))
        assert lib.kalle_upsample_nearest(P(x), P(up), rows, Ln, scale, 0, st) == 0
        d = _guarded(_randn((rows, Ln * scale), g))[1]
        bb, back = _guarded(torch.full((rows, Ln), NAN, device="cuda"))
        assert lib.kalle_upsample_nearest(P(d), P(back), rows, Ln, scale, 1, st) == 0
        torch.cuda.synchronize()
        _exact(up, kr.upsample_nearest(x.double(), scale).float(), f"upsample x{scale}")
        _check(back, kr.upsample_nearest(d.double(), scale, True), scale * U * kr.upsample_nearest(d.double().abs(), scale, True),
               f"upsample bwd x{scale}")
        _clean(ub, up, "upsample")
        _clean(bb, back, "upsample bwd")
    B, Cn, Ln = 3, 7, 16385
    x = _guarded(_randn((B, Cn, Ln), g))[1]
    s0 = _randn((Cn,), g)
    sb, s = _guarded(s0.clone())
    assert lib.kalle_channel_sum(P(x), P(s), B, Cn, Ln, st) == 0
    torch.cuda.synchronize()
    _check(s, s0.double() + kr.channel_sum(x.double()), (B * Ln + 1) * U * (x.double().abs().sum((0, 2)) + s0.double().abs()), "channel_sum")
    _clean(sb, s, "channel_sum")
    d0, nn = 6, 9 * 7
    v, gg, dw = _randn((d0, nn), g), 1 + 0.3 * _randn((d0,), g), _randn((d0, nn), g)
    v[3] *= 1e-4                                                                          # a slice with tiny ||v||
    v, gg, dw = _guarded(v)[1], _guarded(gg)[1], _guarded(dw)[1]
    rdv, rdg = kr.weight_norm_bwd(dw.double(), v.double(), gg.double())
    vd, dwd = v.double(), dw.double()
    nrm = vd.pow(2).sum(1).sqrt()
    adot = (dwd * vd).abs().sum(1)
    e_dot = (nn + 2) * U * adot                                                           # the n-term sum <dw, v>
    tol_dg = e_dot / nrm + ((nn + 2) * U + ALLOW["DIV"] * U) * adot / nrm
    sc = (gg.double() / nrm).abs()[:, None]
    tol_dv = sc * (vd.abs() * (e_dot / nrm.pow(2))[:, None]
                   + ((nn + 6) * U + 2 * ALLOW["DIV"] * U) * (dwd.abs() + vd.abs() * (adot / nrm.pow(2))[:, None]))
    for accumulate in (0, 1):
        v0, g0 = _randn((d0, nn), g), _randn((d0,), g)
        dvb, dv = _guarded(v0.clone() if accumulate else torch.full((d0, nn), NAN, device="cuda"))
        dgb, dg = _guarded(g0.clone() if accumulate else torch.full((d0,), NAN, device="cuda"))
        assert lib.kalle_weight_norm_bwd(P(dw), P(v), P(gg), P(dv), P(dg), d0, nn, accumulate, st) == 0
        torch.cuda.synchronize()
        pv, pg = (v0.double(), g0.double()) if accumulate else (0.0, 0.0)
        _check(dv, pv + rdv, tol_dv + U * (rdv.abs() + abs(pv)), f"weight_norm_bwd dv acc {accumulate}")
        _check(dg, pg + rdg, tol_dg + U * (rdg.abs() + abs(pg)), f"weight_norm_bwd dg acc {accumulate}")
        _clean(dvb, dv, "dv")
        _clean(dgb, dg, "dg")


# ================================================================================================ data-gradient recipes
@pytest.mark.parametrize("stride,K,pl,dil,Lin", [(1, 7, 3, 1, 200), (1, 3, 9, 9, 130), (2, 4, 1, 1, 201), (4, 8, 2, 1, 202), (8, 16, 4, 1, 210)])
def test_data_gradient_recipes(kl, stride, K, pl, dil, Lin):
    """the header's backward section through the forward entry points, against float64 autograd of F.conv1d / conv_transpose1d"""
    import torch.nn.functional as Fn
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(17)
    B, Cin, Cout = 3, 9, 20
    v, gg = _randn((Cout, Cin, K), g, 0.3), 1 + 0.2 * _randn((Cout,), g)
    x = _randn((B, Cin, Lin), g).double().requires_grad_(True)
    wt = (v.double() * (gg.double() / v.double().flatten(1).norm(dim=1)).view(-1, 1, 1))
    y = Fn.conv1d(Fn.pad(x, (pl, pl)), wt, None, stride=stride, dilation=dil)
    Lout = y.shape[2]
    dyb, dy = _guarded(_randn((B, Cout, Lout), g))
    y.backward(dy.double())
    w = torch.zeros((Cout, K, (Cin + 7) // 8 * 8), device="cuda")
    dxb, dx = _guarded(torch.full((B, Cin, Lin), NAN, device="cuda"))
    wabs = wt.abs()
    if stride == 1:
        assert lib.kalle_weight_norm_fold(P(v), P(gg), P(w), Cout, Cin, K, 1 | 2, st) == 0
        assert lib.kalle_conv1d_fwd(P(dy), F32, P(w), None, P(dx), F32, B, Cout, Lout, Cin, Lin, K, 1, (K - 1) * dil - pl, dil, None, None, st) == 0
    else:
        assert lib.kalle_weight_norm_fold(P(v), P(gg), P(w), Cout, Cin, K, 1, st) == 0
        assert Lin <= (Lout - 1) * stride - pl + K
        assert lib.kalle_conv_transpose1d_fwd(P(dy), F32, P(w), None, P(dx), F32, B, Cout, Lout, Cin, Lin, K, stride, pl, None, None, st) == 0
    PLANS_SEEN.add(lib.kalle_conv_last_plan())
    torch.cuda.synchronize()
    asum = torch.autograd.grad(Fn.conv1d(Fn.pad(x, (pl, pl)), wabs, None, stride=stride, dilation=dil), x, dy.double().abs())[0]
    # n-term sum over Cout K terms of folded weights, each within ((Cin K + 2) / 2 + DIV + 2) u of the exact fold
    tol = (Cout * K + 2 + (Cin * K + 2) / 2 + ALLOW["DIV"] + 2) * U * asum + 1e-30
    _check(dx, x.grad, tol, f"data gradient stride {stride}")
    _clean(dxb, dx, "dx")
    # ConvTranspose1d (v [Cin'][Cout'][K]): dx = conv1d over dy with fold flag 0, the module's stride and padding
    vt = _randn((Cout, Cin, K), g, 0.3)                       # a transposed conv Cout -> Cin channels
    xt = _randn((B, Cout, 40), g).double().requires_grad_(True)
    if dil == 1:
        yt = Fn.conv_transpose1d(xt, vt.double(), None, stride=stride, padding=pl)
        dyt = _guarded(_randn(tuple(yt.shape), g))[1]
        yt.backward(dyt.double())
        w2 = torch.zeros((Cin, K, (Cout + 7) // 8 * 8), device="cuda")
        assert lib.kalle_weight_norm_fold(P(vt), None, P(w2), Cout, Cin, K, 0, st) == 0
        dxb, dxt = _guarded(torch.full((B, Cout, 40), NAN, device="cuda"))
        assert lib.kalle_conv1d_fwd(P(dyt), F32, P(w2), None, P(dxt), F32, B, Cin, yt.shape[2], Cout, 40, K, stride, pl, 1, None, None, st) == 0
        PLANS_SEEN.add(lib.kalle_conv_last_plan())
        torch.cuda.synchronize()
        asum = torch.autograd.grad(Fn.conv_transpose1d(xt, vt.double().abs(), None, stride=stride, padding=pl), xt, dyt.double().abs())[0]
        _check(dxt, xt.grad, (Cin * K + 2) * U * asum + 1e-30, f"transposed data gradient stride {stride}")
        _clean(dxb, dxt, "dxt")


# ================================================================================================ snake, act1d, pad_act directly
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("logscale", [0, 1])
@pytest.mark.parametrize("B,Cn,Ln", [(3, 7, 255), (2, 5, 256), (3, 9, 257), (1, 1, 1), (2, 33, 1000)])
def test_snake_beta_fwd(kl, dt, logscale, B, Cn, Ln):
    """per element: the SNAKE allowance + 2 u |x| in fp32, + BF16_REL |ref| in bf16 (the reference starts from the bf16 values)"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(19)
    tdt = torch.float32 if dt == F32 else torch.bfloat16
    xb, x = _guarded(_randn((B, Cn, Ln), g, 2.0).to(tdt))
    al, be = _act_vals(g, Cn)
    if not logscale:
        al, be = al.exp(), be.exp()
    al, be = _guarded(al)[1], _guarded(be)[1]
    yb, y = _guarded(torch.full((B, Cn, Ln), NAN, device="cuda", dtype=tdt))
    assert lib.kalle_snake_beta_fwd(P(x), P(y), dt, P(al), P(be), logscale, B, Cn, Ln, st) == 0
    torch.cuda.synchronize()
    xd = x.double()
    ref = kr.snake_beta(xd, al, be, logscale)
    _check(y, ref, _act_err(xd, 1, al, be, logscale, 0.0) + 2 * U * ref.abs() + (BF16_REL * ref.abs() if dt == BF16 else 0.0), "snake_beta")
    _clean(yb, y, "snake_beta")
    assert lib.kalle_snake_beta_fwd(P(x), P(y), dt, None, P(be), logscale, B, Cn, Ln, st) == ERR_ARG


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mode", ["snake", "snake_log", "elu"])
@pytest.mark.parametrize("B,Cn,Ln", [(3, 5, 255), (2, 5, 256), (3, 3, 257), (2, 2, 1), (1, 4, 2), (2, 7, 1000)])
def test_act1d_fwd(kl, dt, mode, B, Cn, Ln):
    """per element.  up = a 6-term sum (+ gain): 8 u sum |2 f x|; h = act(up): Lipschitz x that + the activation's allowance;
    y = a 12-term sum: 14 u sum |f| |h| + sum |f| e(h); + BF16_REL |ref| in bf16"""
    from kalle_audio_amd import conv_ops
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(23)
    tdt = torch.float32 if dt == F32 else torch.bfloat16
    xb, x = _guarded(_randn((B, Cn, Ln), g, 1.5).to(tdt))
    filt = conv_ops.kaiser_sinc_filter12(torch.device("cuda"))
    al, be = _act_vals(g, Cn, 0.7)
    ls = int(mode == "snake_log")
    if mode == "snake":
        al, be = al.exp(), be.exp()
    al, be = _guarded(al)[1], _guarded(be)[1]
    yb, y = _guarded(torch.full((B, Cn, Ln), NAN, device="cuda", dtype=tdt))
    elu = mode == "elu"
    assert lib.kalle_act1d_fwd(P(x), P(y), dt, P(filt), None if elu else P(al), None if elu else P(be), ls, B, Cn, Ln, st) == 0
    torch.cuda.synchronize()
    xd, fd = x.double(), filt.double()
    ref = kr.act1d(xd, fd) if elu else kr.act1d(xd, fd, al, be, ls)
    up = kr.act1d_up(xd, fd)
    e_up = 8 * U * kr.act1d_up(xd.abs(), fd.abs())
    code = 2 if elu else 1
    h = kr.act(up, code, al, be, ls)
    e_h = e_up * _act_lip(code, al, be, ls, 0.0) + _act_err(up, code, al, be, ls, 0.0) + 2 * U * h.abs()
    tol = 14 * U * kr.act1d_down(h.abs(), fd.abs()) + kr.act1d_down(e_h, fd.abs())
    _check(y, ref, tol + (BF16_REL * ref.abs() if dt == BF16 else 0.0) + 1e-30, f"act1d {mode}")
    _clean(yb, y, "act1d")


@pytest.mark.parametrize("phases,pl,Lin,Lout,K", [(1, 0, 40, 40, 1), (1, 6, 40, 40, 7), (2, 1, 34, 17, 4), (4, 2, 60, 15, 8), (8, 3, 130, 17, 16), (8, 8, 128, 16, 16)])
def test_conv_pad_act_layout(kl, phases, pl, Lin, Lout, K):
    """x_padded element-wise: act 0 is pure data movement (bit-exact: zero fill, the de-interleaved phase rows with d > 0 and
    d == 0), act 1 within the snake allowance"""
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    g = _gen(29)
    B, Cn = 3, 5
    Lp = lib.kalle_conv_pad_len(Lout, K, phases, pl, 1)
    lead = pl if phases == 1 else (pl + phases - 1) // phases * phases
    x = _guarded(_randn((B, Cn, Lin), g, 1.5))[1]
    al, be = _act_vals(g, Cn)
    for code in (0, 1):
        pb, xp = _guarded(torch.full((B, Cn, Lp), NAN, device="cuda"))
        ia = _act_struct(L, code, al if code else None, be if code else None, 1)
        assert lib.kalle_conv_pad_act(P(x), P(xp), B, Cn, Lin, Lp, lead, ctypes.addressof(ia), phases, st) == 0
        torch.cuda.synchronize()
        ref = kr.conv_pad_act(x.double(), Lp, lead, (code, al, be, 1, 0.0), phases)
        if code == 0:
            _exact(xp, ref.float(), f"pad_act phases {phases}")
        else:
            tol = kr.conv_pad_act(_act_err(x.double(), 1, al, be, 1, 0.0), Lp, lead, None, phases)
            _check(xp, ref, tol + 2 * U * ref.abs(), f"pad_act snake phases {phases}")
        _clean(pb, xp, "pad_act")


# ================================================================================================ argument rejections
def test_argument_rejections_leave_outputs_untouched(kl):
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    x, w = torch.zeros((1, 8, 64), device="cuda"), torch.zeros((8, 3, 8), device="cuda")
    y = torch.full((1, 8, 64), NAN, device="cuda")
    bad_act = _act_struct(L, 1)                               # snake without alpha / beta
    bad_code = _act_struct(L, 5)
    ep_bad = L.ConvEpilogue(None, 1.0, 0, 0, _act_struct(L, 4), None)      # the gate is input-side only
    conv = lambda **k: lib.kalle_conv1d_fwd(*[k.get(n, d) for n, d in (  # noqa: E731
        ("x", P(x)), ("xdt", F32), ("w", P(w)), ("bias", None), ("y", P(y)), ("ydt", F32), ("B", 1), ("Cin", 8), ("Lin", 64), ("Cout", 8),
        ("Lout", 64), ("K", 3), ("stride", 1), ("pl", 1), ("dil", 1), ("ia", None), ("ep", None), ("st", st))])
    assert conv() == 0
    torch.cuda.synchronize()
    y.fill_(NAN)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(Cin=0), dict(Lin=0), dict(Cout=0), dict(Lout=0), dict(K=0), dict(K=17),
               dict(stride=0), dict(dil=0), dict(pl=-1), dict(Lout=66), dict(B=65536), dict(ia=ctypes.addressof(bad_act)),
               dict(ia=ctypes.addressof(bad_code)), dict(ep=ctypes.addressof(ep_bad))):
        assert conv(**kw) == ERR_ARG, kw
        assert lib.kalle_conv_last_plan() == 0
    convT = lambda **k: lib.kalle_conv_transpose1d_fwd(*[k.get(n, d) for n, d in (  # noqa: E731
        ("x", P(x)), ("xdt", F32), ("w", P(w)), ("bias", None), ("y", P(y)), ("ydt", F32), ("B", 1), ("Cin", 8), ("Lin", 31), ("Cout", 8),
        ("Lout", 62), ("K", 4), ("stride", 2), ("pl", 1), ("ia", None), ("ep", None), ("st", st))])
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(Cin=0), dict(Lin=0), dict(Cout=0), dict(Lout=0), dict(K=0), dict(stride=0),
               dict(pl=-1), dict(Lout=64), dict(B=65536), dict(ia=ctypes.addressof(bad_act)), dict(ep=ctypes.addressof(ep_bad))):
        assert convT(**kw) == ERR_ARG, kw
        assert lib.kalle_conv_last_plan() == 0
    assert lib.kalle_conv_pad_act(P(x), P(y), 1, 8, 64, 64, 0, None, 0, st) == ERR_ARG
    assert lib.kalle_conv_pad_act(P(x), P(y), 1, 8, 64, 63, 0, None, 2, st) == ERR_ARG          # Lp % phases
    assert lib.kalle_conv_pad_act(None, P(y), 1, 8, 64, 64, 0, None, 1, st) == ERR_ARG
    assert lib.kalle_conv_pad_act(P(x), P(y), 1, 8, 64, 64, -1, None, 1, st) == ERR_ARG
    assert lib.kalle_conv_pad_act(P(x), P(y), 1, 8, 64, 64, 0, ctypes.addressof(_act_struct(L, 4)), 1, st) == ERR_ARG
    Lp = lib.kalle_conv_pad_len(64, 3, 1, 1, 1)
    xp = torch.zeros((1, 8, Lp), device="cuda")
    assert lib.kalle_conv1d_cfirst_fwd(P(xp), P(w), None, P(y), 1, 8, Lp - 1, 8, 64, 3, 1, 1, 1, None, None, st) == ERR_ARG       # Lp too short
    assert lib.kalle_conv1d_cfirst_fwd(None, P(w), None, P(y), 1, 8, Lp, 8, 64, 3, 1, 1, 1, None, None, st) == ERR_ARG
    assert lib.kalle_conv1d_cfirst_fwd(P(xp), P(w), None, P(y), 1, 8, Lp, 8, 64, 3, 2, 1, 2, None, None, st) == ERR_UNSUPPORTED    # strided and dilated
    assert lib.kalle_conv_transpose1d_cfirst_fwd(P(xp), P(w), None, P(y), 1, 8, 3, 8, 62, 4, 2, 1, None, st) == ERR_ARG           # Lp too short
    assert lib.kalle_conv_last_plan() == 0
    assert lib.kalle_conv_wgrad(P(x), P(x), P(y), 1, 8, 8, 64, 64, 17, 1, 1, 1, 0, None, st) == ERR_ARG
    assert lib.kalle_conv_wgrad(P(x), P(x), P(y), 1, 8, 8, 64, 64, 3, 1, 1, 1, 2, None, st) == ERR_ARG
    assert lib.kalle_conv_last_plan() == 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ================================================================================================ the bounds bite
WRONG = [
    ("first_tap_shifted", "conv", C(v2(8, 2, 4), Cin=9, Cout=20, K=7, pl=3, Lin=200, act=1)),
    ("last_tap_dropped", "conv", T(tv2(8, 2, 4), 4, Cout=20, Lin=200, act=1)),
    ("alpha_next_channel", "conv", C(v2(8, 2, 4), Cin=9, Cout=20, K=3, Lin=200, act=1)),
    ("post_alpha_next_channel", "conv", F(cf(4), B=1, Cin=64, Cout=300, K=3, Lin=100, act=2, post=1)),
    ("scale_after_accumulate", "conv", C(v2(8, 2, 4), Cin=9, Cout=20, K=3, Lin=200, acc=True, scale=0.5)),
    ("tanh_before_post", "conv", C(fb(), Cin=9, Cout=20, K=6, stride=3, pl=2, Lin=301, post=1, tanh=True)),
    ("raw_after_post", "conv", C(v2(8, 2, 4), Cin=9, Cout=20, K=3, Lin=200, post=2, raw=True)),
    ("pad_column", "conv", C(v2(8, 2, 4), Cin=9, Cout=20, K=3, Lin=200)),
    ("partial_sum_missing", "conv", F(cf(4, 4), B=2, Cin=512, Cout=64, K=3, Lin=17, act=1)),
    ("padding_off_by_one", "wgrad", W(wg_lds(16, 7), K=7, CV=64)),
]


@pytest.mark.parametrize("wrong,kind,c", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_references_are_caught(kl, wrong, kind, c):
    """the same case passes against the right reference and `_check` raises against the deliberately wrong one"""
    run = run_conv if kind == "conv" else run_wgrad
    run(kl, c)
    with pytest.raises(AssertionError, match="out of bound"):
        run(kl, c, wrong=wrong)
    print(f"wrong reference {wrong}: caught")


# ================================================================================================ the host queries
def _query_cases():
    """(family, ks > 1, plan case): one tiny shape per family, each checked against tests/golden/conv_plans.json.  (conv_cases
    imports this module's lists, so it is imported here and not at the top)"""
    import conv_cases as cc
    return [
        (2, False, cc.conv(3, 9, 20, 3, 200)),
        (1, False, cc.conv(3, 9, 20, 3, 200, xdt=BF16)),
        (4, False, cc.convT(2, 8, 20, 4, 50, 2)),
        (3, False, cc.convT(2, 8, 20, 4, 50, 2, ydt=BF16)),
        (5, False, cc.conv(1, 8, 256, 3, 32)),
        (5, True, cc.conv(1, 352, 64, 3, 16)),
        (6, False, cc.conv(1, 8, 256, 4, 64, stride=2)),
        (7, False, cc.convT(1, 8, 256, 4, 16, 2)),
        (8, False, cc.wgrad(1, 8, 16, 7, 64, pl=3)),
        (9, False, cc.wgrad(1, 8, 8, 7, 64, pl=3)),
    ]


@pytest.mark.parametrize("i", range(10), ids=["family2", "family1", "family4", "family3", "family5", "family5ks", "family6", "family7", "family8", "family9"])
def test_conv_query_matches_launch(kl, i):
    """conv_ops / conv_train launch what the host query predicts: the plan word, and bit for bit the output of the entry point the
    query names, called directly with the query's Lp / lead / phases / workspace"""
    import json
    import conv_cases as cc
    from kalle_audio_amd import conv_ops, conv_train
    family, split, c = _query_cases()[i]
    ops, lib, L = kl
    P, st = ops._p, ops._stream()
    row = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")))[cc.key(c)]
    assert row[1] == 0 and row[2] & 15 == family and (family in (5, 6, 7) and ((row[2] >> 12) & 31) > 1) == split, (row, "a wrong case")
    q = cc.query(c)
    assert q == row, (q, row)
    f, g = cc.full(c), _gen(5)
    tdt = lambda d: torch.float32 if d == F32 else torch.bfloat16  # noqa: E731
    if f["kind"] == "wgrad":
        U_, V_ = _randn((f["B"], f["CU"], f["MU"]), g), _randn((f["B"], f["CV"], f["LV"]), g)
        geo = dict(K=f["K"], stride=f["stride"], padding=f["pl"], dilation=f["dil"], act_on=0)
        dW = conv_train.conv_wgrad(U_, V_, torch.zeros((f["CU"], f["CV"], f["K"]), device="cuda"), **geo)
        assert lib.kalle_conv_last_plan() == q[2]
        dW2 = torch.zeros_like(dW)
        assert lib.kalle_conv_wgrad(P(U_), P(V_), P(dW2), f["B"], f["CU"], f["CV"], f["MU"], f["LV"], f["K"], f["stride"], f["pl"], f["dil"], 0,
                                    None, st) == 0
        assert lib.kalle_conv_last_plan() == q[2]
        torch.cuda.synchronize()
        assert torch.equal(dW, dW2) and dW.abs().sum() > 0
        return
    B, Cin, Lin, Cout, Lout, K, s, pl, dil = (f[k] for k in ("B", "Cin", "Lin", "Cout", "Lout", "K", "stride", "pl", "dil"))
    x = _randn((B, Cin, Lin), g).to(tdt(f["xdt"]))
    tr = f["kind"] == "convT"
    w = conv_ops.weight_norm_fold(_randn((Cin, Cout, K) if tr else (Cout, Cin, K), g, 0.3), None, transposed=tr)
    bias = _randn((Cout,), g)
    if tr:
        y = conv_ops.conv_transpose1d(x, w, bias, Cout=Cout, K=K, stride=s, padding=pl, out_dtype=tdt(f["ydt"]))
    else:
        y = conv_ops.conv1d(x, w, bias, Cout=Cout, K=K, stride=s, padding=pl, dilation=dil, out_dtype=tdt(f["ydt"]))
    assert lib.kalle_conv_last_plan() == q[2] and tuple(y.shape) == (B, Cout, Lout)
    y2 = torch.full_like(y, NAN)
    entry, word = q[0], q[2]
    Lp, lead, phases, nws = q[3:] or (0, 0, 0, 0)
    if entry.startswith("cfirst"):
        xp = torch.full((B, Cin, Lp), NAN, device="cuda")
        assert lib.kalle_conv_pad_act(P(x), P(xp), B, Cin, Lin, Lp, lead, None, phases, st) == 0
        ws = torch.full((nws,), NAN, device="cuda") if nws else None
        assert (nws > 0) == split
    if entry == "conv":
        rc = lib.kalle_conv1d_fwd(P(x), f["xdt"], P(w), P(bias), P(y2), f["ydt"], B, Cin, Lin, Cout, Lout, K, s, pl, dil, None, None, st)
    elif entry == "convT":
        rc = lib.kalle_conv_transpose1d_fwd(P(x), f["xdt"], P(w), P(bias), P(y2), f["ydt"], B, Cin, Lin, Cout, Lout, K, s, pl, None, None, st)
    elif entry == "cfirst":
        rc = lib.kalle_conv1d_cfirst_fwd(P(xp), P(w), P(bias), P(y2), B, Cin, Lp, Cout, Lout, K, s, pl, dil, None, P(ws), st)
    else:
        rc = lib.kalle_conv_transpose1d_cfirst_fwd(P(xp), P(w), P(bias), P(y2), B, Cin, Lp, Cout, Lout, K, s, pl, None, st)
    assert rc == 0 and lib.kalle_conv_last_plan() == word
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and not torch.isnan(y.float()).any()


# ================================================================================================ coverage and allowances
def test_every_plan_family_and_tile_form_was_seen(kl):
    """every kernel family and tile form of the header's plan word came out of some case.  Reads PLANS_SEEN, which the case lists
    above fill: meaningful only when the whole file runs in one process, in order (not with -k, a node id or xdist)"""
    want = {v2(2, 2, 1), v2(8, 8, 4), v2(8, 4, 4), v2(8, 2, 4), v2(16, 8, 4), v2(16, 8, 4, ci=16), v2(16, 4, 8, nw=8, ci=32),
            v2(16, 8, 8, nw=8), v2(8, 8, 4, stride=2), v2(8, 4, 4, stride=4), v2(16, 4, 4, stride=4), v2(8, 2, 4, stride=8),
            v2(2, 2, 1, dt=BF16), v2(8, 2, 4, dt=BF16), fb(), fb(F32, BF16), fb(BF16, F32),
            tv2(2, 2, 1), tv2(8, 8, 4), tv2(8, 4, 4), tv2(8, 2, 4), tv2(16, 8, 4), tv2(8, 2, 4, dt=BF16), fb(F32, BF16, 3), fb(BF16, F32, 3),
            cf(1), cf(2), cf(4), cf(4, 4), cf(4, 16), cf(4, 1, 6), cf(4, 16, 6), cf(1, 1, 7), cf(2, 1, 7), cf(4, 1, 7),
            wg_lds(16, 1), wg_lds(16, 4), wg_lds(16, 7), wg_lds(16, 8), wg_lds(8, 16), wg_lane(4, 8, 4), wg_lane(4, 4, 8), wg_lane(2, 4, 16)}
    print("conv plan words seen:", " ".join(hex(p) for p in sorted(PLANS_SEEN)))
    assert want <= PLANS_SEEN, [hex(p) for p in sorted(want - PLANS_SEEN)]


def test_measured_allowances(kl):
    """prints the measured worst cases (u * magnitude units) and holds each to its allowance.  Reads MEASURED, which the
    test_measure_* sweeps at the top of the file fill: whole file, one process, in order"""
    for k in ("SNAKE", "ELU", "TANH", "GATE"):
        assert k in MEASURED, (k, "not measured")
        print(f"MEASURED {k}: {MEASURED[k]:.3f} (allowed {ALLOW[k]})")
        assert MEASURED[k] <= ALLOW[k], (k, MEASURED[k], ALLOW[k])
