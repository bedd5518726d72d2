"""-m gpu: kalle_llasa_frame_head_rows (csrc/llasa.hip: the RMSNorm pre-pass and R-row GEMM for W1, llasa_head_kernel, the R-row
GEMM for Wa) element by element against the float64 reference of tests/llasa_head_refs.py, by the method of
tests/test_decode_rows_gpu.py: every stage from its own inputs as the kernels published them, NaN-guarded buffers with row strides
larger than their widths, a fenced workspace, untouched memory compared bit for bit, wrong references caught.

Bounds (those of test_decode_gpu.py / test_norm_elementwise_gpu.py, nothing new measured):
  h1, mean, x_next   K 2^-24 sum_k |W_nk| |x_rk| + 4 x 2^-24 (|bias| + that sum)   (td.gemv_ref: an fp32 dot in any order)
  xn, a              the bf16 rounding of the float64 value, bit for bit, except where that value lies within the stage's fp32
                     window of a rounding boundary (either neighbour then; such elements are capped at max(1, 1 %) of a row for
                     the norm and max(1, 5 %) for the GELU, see GELU_CAP): dc.rms_window for the norm, (ALLOW["ERF"] + 3) u |h1|
                     for the GELU
  latent             3 u (|mean| + |std noise|): one product, one sum (or their fused form)
  lat                the bf16 rounding of the fp32 latent the kernel stored: bit for bit
  kl                 per term 8 u of the magnitudes that enter it (c0, c1 rounded to fp32; m - 1, its square, one product, two sums),
                     the fp32 sum of dl terms in any order dl u sum_j |term_j|, both over dl, + (ALLOW["DIV"] + 1) u |kl| for the division
An INACTIVE row's inputs hold NaN and its outputs and workspace rows their fill, and must come back bit for bit."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc  # noqa: E402
import kernel_refs as kr  # noqa: E402
import llasa_head_cases as hc  # noqa: E402
import llasa_head_refs as hr  # noqa: E402
import test_decode_gpu as td  # noqa: E402
from gpu_checks import NAN, U, Guard, _bits, check, guarded as _guarded, clean as _clean  # noqa: E402
from test_norm_elementwise_gpu import ALLOW  # noqa: E402

pytestmark = pytest.mark.gpu

FENCE = 64
BF, F32 = torch.bfloat16, torch.float32
P = td.P
WRONG_MARGIN = 2.0
# The GELU allowance is in units of |x| while the output x Phi(x) is far smaller on the negative side, so the chance that an
# element lies within the window of a bf16 boundary is 2 x 11 u |x| / ulp_bf16(x Phi(x)) ~ 3.4e-4 / Phi(x): 0.07 % at x = 0,
# 1.5 % at x = -2, 25 % at x = -3 - about 1 % averaged over h1 ~ N(0, 1.1) as these inputs give.  The 1 % cap of the norm stage
# (window and value both proportional to |x|) would sit at the expectation; 5 % leaves 95 % of a row compared bit for bit.
GELU_CAP = 0.05
assert (hc.ERF_U, hc.DIV_U) == (ALLOW["ERF"], ALLOW["DIV"])


def iarr(vals):
    return ctypes.cast((ctypes.c_int32 * len(vals))(*vals), ctypes.c_void_p)


def same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), (what, "not bit for bit")


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


class Head:
    """one call on the inputs of hc.inputs(c): everything the call may write sits in NaN"""

    def __init__(self, lib, c, inactive=None, mask_arg=True):
        from kalle_audio_amd import _lib
        self.c, self.lib = c, lib
        R, D, dl = c["R"], c["D"], c["dl"]
        self.inactive = tuple(c["inactive"] if inactive is None else inactive)
        x = hc.inputs(c)
        self.h = Guard(R, D, ld=D + 4, init=x["h"].cuda())
        self.noise = Guard(R, dl, ld=dl + 3, init=x["noise"].cuda())
        for r in self.inactive:
            self.h.v[r], self.noise.v[r] = NAN, NAN
        self.w1 = Guard(dl, D, ld=D + 8, dtype=BF, init=x["w1"].cuda())
        self.w2 = Guard(dl, dl, ld=dl + 8, dtype=BF, init=x["w2"].cuda())
        self.wa = Guard(D, dl, ld=dl + 16, dtype=BF, init=x["wa"].cuda())
        self.norm, self.b1, self.b2, self.ba = (x[k].cuda() for k in ("norm", "b1", "b2", "ba"))
        self.desc = _lib.LlasaHead()
        d = self.desc
        d.norm, d.w1, d.b1, d.w2, d.b2, d.wa, d.ba = (t.data_ptr() for t in (self.norm, self.w1.v, self.b1, self.w2.v, self.b2, self.wa.v, self.ba))
        d.ldw1, d.ldw2, d.ldwa = D + 8, dl + 8, dl + 16
        self.bufs = {k: _guarded(torch.full(s, NAN, device="cuda")) for k, s in
                     (("mean", (R, dl)), ("latent", (R, dl)), ("kl", (R,)), ("x_next", (R, D)))}
        self.lay, self.ws_bytes = hc.ws_layout(R, D, dl)
        assert lib.kalle_llasa_head_ws_bytes(R, D, dl) == self.ws_bytes
        self.wsbuf = torch.full((self.ws_bytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)   # all-ones bytes: NaN as fp32 and as bf16
        self.ws = self.wsbuf[FENCE:FENCE + self.ws_bytes]
        assert self.ws.data_ptr() % 64 == 0
        act = iarr([0 if r in self.inactive else 1 for r in range(R)]) if (mask_arg or self.inactive) else None
        self.rc = self.run(act)

    def run(self, act, **over):
        c = dict(self.c, std=hc.STD, ldh=self.c["D"] + 4)
        c.update(over)
        o = {k: v[1] for k, v in self.bufs.items()}
        rc = self.lib.kalle_llasa_frame_head_rows(ctypes.addressof(self.desc), P(self.h.v), c["ldh"], P(self.noise.v), self.c["dl"] + 3,
                                                  ctypes.c_float(c["std"]), ctypes.c_float(hc.EPS), P(o["mean"]), P(o["latent"]), P(o["kl"]),
                                                  P(o["x_next"]), act, c["R"], c["D"], c["dl"], P(self.ws), None)
        torch.cuda.synchronize()
        return rc

    def out(self, k):
        return self.bufs[k][1]

    def region(self, k):
        o, nb, dt, n = self.lay[k]
        return self.ws[o:o + nb].view(dt).view(self.c["R"], n)

    def everything(self):
        """every output and workspace region as the call left it"""
        return {**{k: self.out(k).clone() for k in self.bufs}, **{k: self.region(k).clone() for k in self.lay}}

    def untouched(self, what):
        for k, (buf, view) in self.bufs.items():
            _clean(buf, view, f"{what} {k}")
            for r in self.inactive:
                assert torch.isnan(view[r]).all(), (what, "output row of an inactive row written", k, r)
        assert (self.wsbuf[:FENCE] == 0xFF).all() and (self.wsbuf[FENCE + self.ws_bytes:] == 0xFF).all(), (what, "write outside the workspace")
        for k, (o, nb, dt, n) in self.lay.items():
            assert (self.ws[o + nb:o + ((nb + 63) & ~63)] == 0xFF).all(), (what, "padding written after", k)
            for r in self.inactive:
                assert (self.region(k)[r].contiguous().view(torch.uint8) == 0xFF).all(), (what, "workspace row of an inactive row written", k, r)
        for g, n in ((self.h, "h"), (self.noise, "noise"), (self.w1, "w1"), (self.w2, "w2"), (self.wa, "wa")):
            g.clean(f"{what} {n}")


def rounded(v, window, what, cap=0.01):
    """(bf16 rounding of the float64 row v, allowance: one bf16 ulp where v lies within `window` of a rounding boundary, else 0)"""
    amb = kr.bf16_ambiguous(v, window)
    assert amb.sum().item() <= max(1, cap * v.numel()), (what, "ambiguous elements over the cap", int(amb.sum()), v.numel())
    return hr.bf16r(v), torch.where(amb, kr.bf16_ulp(v), torch.zeros_like(v))


def stages(s, r, wrong=None):
    """the eight (name, kernel output, ref, tol) of row r, each from the inputs the kernels themselves read; `wrong` swaps one
    reference for a deliberately wrong one"""
    c = s.c
    D, dl = c["D"], c["dl"]
    ws = {k: s.region(k)[r].clone() for k in s.lay}
    o = {k: s.out(k)[r].clone() for k in s.bufs}
    res = []
    h = s.h.v[r].double()
    xh = hr.rms(h[None], s.norm.double(), hc.EPS)[0]
    ref, tol = rounded(xh, dc.rms_window(xh), f"xn row {r}")
    if wrong == "no_eps":
        ref = hr.bf16r(hr.rms(h[None], s.norm.double(), hc.EPS, "no_eps")[0])
    res.append(("xn", ws["xn"], ref, tol))
    ref, tol = td.gemv_ref(s.w1.v, ws["xn"].double(), D, res=None if wrong == "no_b1" else s.b1.double())
    if wrong == "no_b1":
        tol = td.gemv_ref(s.w1.v, ws["xn"].double(), D, res=s.b1.double())[1]
    res.append(("h1", ws["h1"], ref, tol))
    h1 = ws["h1"].double()
    ref, tol = rounded(hr.gelu(h1), (ALLOW["ERF"] + 3) * U * h1.abs(), f"a row {r}", cap=GELU_CAP)
    if wrong == "tanh":
        ref = hr.bf16r(hr.gelu(h1, "tanh"))
    res.append(("a", ws["a"], ref, tol))
    ref, tol = td.gemv_ref(s.w2.v, ws["a"].double(), dl, res=s.b2.double())
    res.append(("mean", o["mean"], ref, tol))
    m = o["mean"].double()
    nz = s.noise.v[(r + 1) % c["R"] if wrong == "other_row_noise" else r].double()
    res.append(("latent", o["latent"], m + hc.STD * nz, 3 * U * (m.abs() + (hc.STD * s.noise.v[r].double()).abs()) + 1e-30))
    res.append(("lat", ws["lat"], hr.bf16r(o["latent"].double()), torch.zeros(dl, dtype=torch.float64, device="cuda")))
    terms, mag = hr.kl_terms(m, hc.STD)
    ref = terms.mean()
    tol = (8 * U * mag.sum() + dl * U * terms.abs().sum()) / dl + (ALLOW["DIV"] + 1) * U * ref.abs()
    if wrong in ("no_half", "kl_vs_n01", "no_std2"):
        ref = hr.kl(m, hc.STD, wrong)
    res.append(("kl", o["kl"].reshape(1), ref.reshape(1), tol.reshape(1)))
    ref, tol = td.gemv_ref(s.wa.v, ws["lat"].double(), dl, res=s.ba.double())
    res.append(("x_next", o["x_next"], ref, tol))
    return res


@pytest.fixture(scope="module")
def runs(kl):
    ops, lib = kl
    out = {}
    for name, c in hc.CASES.items():
        s = Head(lib, c)
        assert s.rc == 0, (name, s.rc, lib.kalle_last_error())
        out[name] = s
    return out


@pytest.mark.parametrize("name", list(hc.CASES))
def test_every_stage_of_every_active_row(runs, name):
    s = runs[name]
    for r in range(s.c["R"]):
        if r in s.inactive:
            continue
        for stage, got, ref, tol in stages(s, r):
            assert torch.isfinite(got).all(), (name, r, stage, "NaN of an inactive row or of the fill leaked")
            check(got, ref, tol, f"{name} row {r} {stage}")
    s.untouched(name)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_two_calls_give_equal_bits(kl, runs, name):
    ops, lib = kl
    s = runs[name]
    t = Head(lib, s.c)
    assert t.rc == 0
    for (k, a), b in zip(s.everything().items(), t.everything().values()):
        same_bits(a, b, f"{name} {k}")


@pytest.mark.parametrize("name", ["r3-hole", "r16-dl24", "r5-dl512", "r16-dl512-holes"])
def test_an_active_row_does_not_depend_on_the_mask(kl, runs, name):
    """the same inputs with all but two of the active rows masked off: those two rows' outputs and workspace rows bit for bit"""
    ops, lib = kl
    s = runs[name]
    act = [r for r in range(s.c["R"]) if r not in s.inactive]
    keep = (act[0], act[-1])
    t = Head(lib, s.c, inactive=[r for r in range(s.c["R"]) if r not in keep])
    assert t.rc == 0
    full, part = s.everything(), t.everything()
    for k in full:
        for r in keep:
            same_bits(full[k][r], part[k][r], f"{name} {k} row {r}")
    t.untouched(name + " masked")


def test_a_null_mask_is_every_row(kl, runs):
    ops, lib = kl
    t = Head(lib, hc.CASES["r16-dl24"], mask_arg=False)
    assert t.rc == 0
    for (k, a), b in zip(runs["r16-dl24"].everything().items(), t.everything().values()):
        same_bits(a, b, k)


def test_small_magnitude_rows_take_eps_into_the_norm(kl):
    ops, lib = kl
    s = Head(lib, hc.SMALL_H)
    assert s.rc == 0
    for r in range(2):
        for stage, got, ref, tol in stages(s, r):
            check(got, ref, tol, f"small h row {r} {stage}")
    right = {k: (g, rf, t) for k, g, rf, t in stages(s, 0)}
    bad = {k: rf for k, _, rf, _ in stages(s, 0, wrong="no_eps")}
    caught(("RMSNorm without eps", *right["xn"], bad["xn"]))
    s.untouched("small h")


def caught(case):
    what, got, ref, tol, wref = case
    check(got, ref, tol, what + ": right reference")
    moved = (wref - ref).abs()
    assert (moved[moved > 0] / tol.double().expand_as(moved)[moved > 0].clamp_min(1e-300)).max().item() > WRONG_MARGIN, what
    with pytest.raises(AssertionError, match="out of bound"):
        check(got, wref, tol, what)


@pytest.mark.parametrize("wrong,stage", [("tanh", "a"), ("no_half", "kl"), ("kl_vs_n01", "kl"), ("no_b1", "h1"), ("no_std2", "kl"),
                                         ("other_row_noise", "latent")])
def test_wrong_references_are_caught_at_their_stage(runs, wrong, stage):
    """each wrong reference moves some element by more than WRONG_MARGIN x its allowance and fails the check the right one passes;
    every other stage's reference is the right one"""
    s = runs["r5-dl512"]
    right = {k: (g, rf, t) for k, g, rf, t in stages(s, 1)}
    bad = {k: rf for k, _, rf, _ in stages(s, 1, wrong=wrong)}
    caught((wrong, *right[stage], bad[stage]))
    for k in right:
        if k != stage:
            assert torch.equal(bad[k], right[k][1]), (wrong, "moved the reference of", k)


def test_refusals_write_nothing(kl):
    ops, lib = kl
    s = Head(lib, hc.CASES["r3-hole"], inactive=(0, 1, 2))
    assert s.rc == 0                                                # every row inactive: KALLE_OK, nothing launched
    act = iarr([1, 1, 1])
    for over in (dict(R=0), dict(R=17), dict(dl=12), dict(D=4), dict(std=0.0), dict(std=-1.0), dict(ldh=6)):
        assert s.run(act, **over) == -1, over
    assert (s.wsbuf == 0xFF).all()
    for k, (buf, view) in s.bufs.items():
        assert torch.isnan(buf).all(), k


def test_wrapper_runs_the_same_call(kl, runs):
    """ops.llasa_head_plan / ops.llasa_frame_head on fp32 master weights: the bits of the direct call on their bf16 copies"""
    ops, lib = kl
    c = hc.CASES["r3-hole"]
    s = runs["r3-hole"]
    x = {k: v.cuda() for k, v in hc.inputs(c).items()}
    par = [torch.nn.Parameter(x[k].float()) for k in ("norm", "w1", "b1", "w2", "b2", "wa", "ba")]
    plan = ops.llasa_head_plan(*par, c["R"], hc.EPS, "cuda", frames=2)
    h = x["h"].clone()
    mean, latent, klv, x_next = ops.llasa_frame_head(plan, h, x["noise"], hc.STD, active=[True, False, True], frame=1)
    torch.cuda.synchronize()
    assert latent.data_ptr() == plan["latent"][1].data_ptr() and klv.data_ptr() == plan["kl"][1].data_ptr()
    for r in (0, 2):
        for k, t in (("mean", mean), ("latent", latent), ("kl", klv), ("x_next", x_next)):
            same_bits(t[r], s.out(k)[r], f"wrapper {k} row {r}")
    assert (mean[1] == 0).all() and (x_next[1] == 0).all() and (plan["latent"][0] == 0).all()     # (the plan's buffers start as zeros)
