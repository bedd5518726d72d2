"""-m gpu: the ragged-batch conv entry points (kalle_conv1d_fwd_lens, kalle_conv_transpose1d_fwd_lens, kalle_conv_pad_act_lens,
kalle_conv1d_cfirst_fwd_lens, kalle_conv_transpose1d_cfirst_fwd_lens), every kernel family, over tests/conv_lens_cases.py.

Per case, four rows of mixed length (one full, one inactive):
 (a) bits: the ragged call sees an x whose positions past lens_in[b] are NaN, the dense entry point the same x with those
     positions zeroed (same shapes, same plan); the two outputs agree bit for bit at every position < lens_out[b];
 (b) no stray write: y and y_raw start from an all-ones byte pattern (or, accumulating, from random contents) inside NaN fences;
     positions >= lens_out[b], the whole inactive row and the fences keep their bytes;
 (c) semantics: each row ALONE, cut to its length, against the fp64 conv reference of tests/kernel_refs.py, per element, under the
     error model and the allowances of tests/test_conv_gpu.py (imported: ALLOW, the activation error and Lipschitz terms);
 (d) references that are wrong on purpose must fail (c): the row convolved with its tail left in (no mask on the input - what a
     dense batch computes), the neighbouring row's length, lens_in used as lens_out on a strided layer.
Also: the query's word equals the launch's, and an all-inactive batch returns KALLE_OK without touching anything."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_lens_cases as lc  # noqa: E402
import kernel_refs as kr  # noqa: E402
import test_conv_gpu as tcg  # noqa: E402
from gpu_checks import NAN, U, _bits, _exact, check, clean, guarded  # noqa: E402
from test_conv_gpu import ALLOW, BF16, F32, _act_err, _act_lip, _act_struct, _act_vals  # noqa: E402
from test_norm_elementwise_gpu import BF16_REL, _gen, _randn  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load(), _lib


def _i32(vals):
    """(host ctypes array, device tensor) of one length array"""
    return (ctypes.c_int32 * len(vals))(*vals), torch.tensor(list(vals), dtype=torch.int32, device="cuda")


def _ones_bytes(shape, dtype):
    """a tensor whose every byte is 0xff (a NaN in fp32 and in bf16)"""
    return torch.full(shape, -1, device="cuda", dtype=torch.int16 if dtype == torch.bfloat16 else torch.int32).view(dtype)


class Run:
    """one case on the device: the ragged call and the dense call on the zeroed x.  tail: what x holds past each row's length in
    the ragged call - "nan" (checks a, b, c) or "data" (d: finite values a missing mask would fold in)"""

    def __init__(self, kl, c, lens=None, tail="nan", louts=None, seed=1):
        ops, lib, L = kl
        P, st = ops._p, ops._stream()
        g = _gen(seed)
        B, Cin, Cout, K, stride, pl, dil, Lin, Lout = (c[k] for k in ("B", "Cin", "Cout", "K", "stride", "pl", "dil", "Lin", "Lout"))
        self.c, self.entry, act = c, c["entry"], c["act"]
        self.transposed = transposed = self.entry in ("convT", "cfirstT")
        self.lens = lens = tuple(c["lens"] if lens is None else lens)
        self.louts = louts = tuple(lc.lens_out(c, lens) if louts is None else louts)
        tdt = lambda d: torch.float32 if d == F32 else torch.bfloat16  # noqa: E731
        xC = 2 * Cin if act == 4 else Cin
        self.x = x_full = _randn((B, xC, Lin), g, 1.5).to(tdt(c["xdt"]))       # data everywhere: the tail is what a dense batch would see
        pos = torch.arange(Lin, device="cuda")[None, None, :]
        live = pos < torch.tensor(lens, device="cuda")[:, None, None]
        x_zero = torch.where(live, x_full, torch.zeros_like(x_full))
        x_rag = x_full if tail == "data" else torch.where(live, x_full, torch.full_like(x_full, NAN))
        self.al, self.be = al, be = _act_vals(g, Cin)
        self.pal, self.pbe = pal, pbe = _act_vals(g, Cout)
        v = _randn((Cin, Cout, K) if transposed else (Cout, Cin, K), g, 0.3)
        CoutP = (Cout + 7) // 8 * 8
        self.w = w = torch.zeros((Cin, K, CoutP), device="cuda")
        assert lib.kalle_weight_norm_fold(P(v), None, P(w), v.shape[0], v.shape[1], K, 1 if transposed else 0, st) == 0
        self.bias = bias = _randn((Cout,), g) if c["bias"] else None
        self.res = res = _randn((B, Cout, Lout), g).to(tdt(c["xdt"])) if c["res"] else None
        ydt = tdt(c["ydt"])
        self.y0 = y0 = _randn((B, Cout, Lout), g).to(ydt) if c["acc"] else _ones_bytes((B, Cout, Lout), ydt)
        ia = _act_struct(L, act, al if act == 1 else None, be if act == 1 else None, 1, 0.2)
        hi, di = _i32(lens)
        ho, do = _i32(louts)
        self.out = {}
        for which, xin in (("ragged", x_rag), ("dense", x_zero)):
            xin = xin.contiguous()
            ybuf, y = guarded(y0.clone())
            rbuf, raw = guarded(_ones_bytes((B, Cout, Lout), ydt)) if c["raw"] else (None, None)
            ep = L.ConvEpilogue(P(res), c["scale"], int(c["acc"]), int(c["tanh"]),
                                _act_struct(L, c["post"], pal if c["post"] == 1 else None, pbe if c["post"] == 1 else None, 1, 0.1), P(raw))
            rag = which == "ragged"
            li = (hi, P(di)) if rag else (None, None)
            lo = (ho, P(do)) if rag else (None, None)
            if self.entry == "conv":
                rc = lib.kalle_conv1d_fwd_lens(P(xin), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride, pl, dil,
                                               ctypes.addressof(ia), ctypes.addressof(ep), *li, *lo, st) if rag else \
                    lib.kalle_conv1d_fwd(P(xin), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride, pl, dil,
                                         ctypes.addressof(ia), ctypes.addressof(ep), st)
            elif self.entry == "convT":
                rc = lib.kalle_conv_transpose1d_fwd_lens(P(xin), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride,
                                                         pl, ctypes.addressof(ia), ctypes.addressof(ep), *li, *lo, st) if rag else \
                    lib.kalle_conv_transpose1d_fwd(P(xin), c["xdt"], P(w), P(bias), P(y), c["ydt"], B, Cin, Lin, Cout, Lout, K, stride, pl,
                                                   ctypes.addressof(ia), ctypes.addressof(ep), st)
            else:
                if self.entry == "cfirst":
                    Lp = lib.kalle_conv_pad_len(Lout, K, stride, pl, dil)
                    lead, phases = (pl, 1) if stride == 1 else ((pl + stride - 1) // stride * stride, stride)
                else:
                    Lp = lib.kalle_convT_pad_len(Lout, K, stride, pl)
                    lead, phases = (K + stride - 1) // stride - 1, 1
                pbuf, xp = guarded(torch.full((B, Cin, Lp), NAN, device="cuda"))
                if rag:
                    assert lib.kalle_conv_pad_act_lens(P(xin), P(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, *li, st) == 0
                    for b in range(B):      # an inactive row's copy is not made
                        assert lens[b] > 0 or torch.isnan(xp[b]).all(), "pad_act wrote an inactive row"
                else:
                    assert lib.kalle_conv_pad_act(P(xin), P(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, st) == 0
                nws = lib.kalle_conv_cfirst_ws_floats(B, Cin, Cout, Lout, K) if self.entry == "cfirst" else 0
                ws = torch.full((max(nws, 1),), NAN, device="cuda") if nws else None
                if self.entry == "cfirst":
                    rc = lib.kalle_conv1d_cfirst_fwd_lens(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl, dil,
                                                          ctypes.addressof(ep), P(ws), *li, *lo, st) if rag else \
                        lib.kalle_conv1d_cfirst_fwd(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl, dil,
                                                    ctypes.addressof(ep), P(ws), st)
                else:
                    rc = lib.kalle_conv_transpose1d_cfirst_fwd_lens(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl,
                                                                    ctypes.addressof(ep), *lo, st) if rag else \
                        lib.kalle_conv_transpose1d_cfirst_fwd(P(xp), P(w), P(bias), P(y), B, Cin, Lp, Cout, Lout, K, stride, pl,
                                                              ctypes.addressof(ep), st)
                clean(pbuf, xp, which + " x_padded")
            plan = lib.kalle_conv_last_plan()
            torch.cuda.synchronize()
            assert rc == 0, (lc.cid(c), which, rc)
            clean(ybuf, y, which + " y")
            if raw is not None:
                clean(rbuf, raw, which + " y_raw")
            self.out[which] = (y, raw, plan)

    # ---- (c): row b alone, cut to its length
    def row_reference(self, b, lin=None, lout=None, x=None):
        """(ref, ref_raw, tol, tol_raw) of row b as a tensor of its own length: fp64, the bound of tests/test_conv_gpu.py"""
        c = self.c
        lin = self.lens[b] if lin is None else lin
        lout = self.louts[b] if lout is None else lout
        xd = (self.x if x is None else x)[b:b + 1, :, :lin].double()
        wd = self.w.double()
        Cin, Cout, K = c["Cin"], c["Cout"], c["K"]
        in_act = (c["act"], self.al, self.be, 1, 0.2)
        post = (c["post"], self.pal, self.pbe, 1, 0.1) if c["post"] else None
        cut = lambda t: None if t is None else t[b:b + 1, :, :lout].double()  # noqa: E731
        epd = dict(residual=cut(self.res), out_scale=float(torch.tensor(c["scale"], dtype=torch.float32)),
                   accumulate=cut(self.y0) if c["acc"] else None, post=post, tanh=c["tanh"])
        fn = kr.conv_transpose1d if self.transposed else kr.conv1d
        geo = dict(stride=c["stride"], padding=c["pl"], Lout=lout)
        if not self.transposed:
            geo["dilation"] = c["dil"]
        bd = None if self.bias is None else self.bias.double()
        ref, ref_raw, asum = fn(xd, wd, Cout, bd, in_act=in_act, epilogue=epd, **geo)
        n = Cin * K + 4
        ex = _act_err(xd, c["act"], self.al, self.be, 1, 0.2)
        eprop = fn(ex, wd.abs(), Cout, None, epilogue=dict(out_scale=abs(epd["out_scale"])), **geo)[0] if c["act"] else 0.0
        tol_raw = n * U * asum + eprop
        tol = tol_raw
        if post:
            tol = tol * _act_lip(c["post"], self.pal, self.pbe, 1, 0.1) + _act_err(ref_raw, c["post"], self.pal, self.pbe, 1, 0.1) + U * ref_raw.abs()
        if c["tanh"]:
            tol = tol + ALLOW["TANH"] * U
        yb = BF16_REL if c["ydt"] == BF16 else 0.0
        return ref, ref_raw, tol + yb * ref.abs() + 1e-30, tol_raw + yb * ref_raw.abs() + 1e-30

    def check_rows(self, what, **kw):
        y, raw, _ = self.out["ragged"]
        for b in range(self.c["B"]):
            lout = kw.get("lout", {}).get(b, self.louts[b])
            if lout == 0:
                continue
            ref, ref_raw, tol, tol_raw = self.row_reference(b, lin=kw.get("lin", {}).get(b), lout=kw.get("lout", {}).get(b), x=kw.get("x"))
            check(y[b:b + 1, :, :lout], ref, tol, f"{what} row {b} y")
            if raw is not None:
                check(raw[b:b + 1, :, :lout], ref_raw, tol_raw, f"{what} row {b} y_raw")


@pytest.mark.parametrize("c", lc.CASES, ids=lc.cid)
def test_conv_lens(kl, c):
    rc, q = lc.plan(c)
    assert rc == 0 and q["family"] == c["family"], (lc.cid(c), rc, q)
    r = Run(kl, c)
    what = lc.cid(c)
    (y, raw, plan), (yd, rawd, pland) = r.out["ragged"], r.out["dense"]
    # the plan does not depend on the lengths: the query's word, the dense launch's and the ragged launch's are one
    assert plan == pland == q["word"], (what, hex(plan), hex(pland), hex(q["word"]))
    tcg.PLANS_SEEN.add(plan)
    for b in range(c["B"]):
        lo = r.louts[b]
        # (a) bits
        _exact(y[b, :, :lo], yd[b, :, :lo], f"{what} row {b}: ragged vs dense on the zeroed x")
        if raw is not None:
            _exact(raw[b, :, :lo], rawd[b, :, :lo], f"{what} row {b} y_raw: ragged vs dense on the zeroed x")
        # (b) nothing at or past the row's length (a whole inactive row) was written
        assert torch.equal(_bits(y[b, :, lo:]), _bits(r.y0[b, :, lo:])), (what, b, "y written past the row's length")
        if raw is not None:
            assert (_bits(raw[b, :, lo:]) == -1).all(), (what, b, "y_raw written past the row's length")
    # (c) each row alone
    r.check_rows(what)


WRONG = [lc.CASES[i] for i in (3, 8, 15, 19, 23, 25)]     # k = 7, strided, transposed; position-per-lane and channels-per-lane


@pytest.mark.parametrize("c", WRONG, ids=lc.cid)
def test_wrong_references_are_caught(kl, c):
    """(d): the same comparison against references that are wrong in the ways a ragged batch goes wrong.  The device's x holds
    finite data past each row's length here, so that a reference which folds the tail in is a finite, plausible tensor"""
    r = Run(kl, c, tail="data")
    what = lc.cid(c)
    r.check_rows(what)                                   # the right reference passes with data in the tail too
    B = c["B"]
    short = [b for b in range(B) if 0 < r.lens[b] < c["Lin"]]
    # the row with its tail left in: what a dense batch (no mask on the input) computes for the same outputs
    with pytest.raises(AssertionError, match="out of bound"):
        r.check_rows(what, lin={b: c["Lin"] for b in short})
    # the neighbouring row's input length
    if r.transposed:                                     # the next longer row's: the reference folds part of the tail in
        b = min(short, key=lambda i: r.lens[i])
        other = min(v for v in r.lens if v > r.lens[b])
    else:                                                # a shorter row's: the reference loses the row's last inputs
        b = max(short, key=lambda i: r.lens[i])
        other = min(v for v in r.lens if 0 < v < r.lens[b])
    with pytest.raises(AssertionError, match="out of bound"):
        r.check_rows(what, lin={b: other})
    # lens_in used as lens_out (strided and transposed layers: the two differ)
    if c["stride"] > 1:
        b = max(short, key=lambda i: r.lens[i])
        wrong_out = min(r.lens[b], c["Lout"])
        assert wrong_out != r.louts[b]
        if wrong_out < r.louts[b]:                       # transposed: outputs past lens_in exist, so "nothing written from there on" fails
            y = r.out["ragged"][0]
            assert not torch.equal(_bits(y[b, :, wrong_out:]), _bits(r.y0[b, :, wrong_out:]))
        else:                                            # strided: outputs up to lens_in do not exist - the device left them unwritten
            with pytest.raises(AssertionError, match="out of bound"):
                r.check_rows(what, lout={b: wrong_out})


def test_all_rows_inactive(kl):
    """every row inactive: KALLE_OK, the dense call's plan word, nothing launched - the outputs keep every byte"""
    c = lc.CASES[3]
    r = Run(kl, c, lens=(0, 0, 0, 0))
    y, raw, plan = r.out["ragged"]
    assert plan == r.out["dense"][2] == lc.plan(c)[1]["word"]
    assert (_bits(y) == -1).all() and (_bits(raw) == -1).all()
    c = lc.CASES[20]                                     # channels per lane: neither the padded copy nor y is touched (Run asserts the copy)
    r = Run(kl, c, lens=(0, 0, 0, 0))
    assert (_bits(r.out["ragged"][0]) == -1).all() and r.out["ragged"][2] == r.out["dense"][2]


def test_full_rows_equal_dense(kl):
    """lengths of all-full rows: bit for bit the dense call, on every output position"""
    for i in (3, 9, 15, 21, 24, 26):
        c = lc.CASES[i]
        r = Run(kl, c, lens=(c["Lin"],) * 4)
        _exact(r.out["ragged"][0], r.out["dense"][0], lc.cid(c) + " full rows")
