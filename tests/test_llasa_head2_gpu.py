"""-m gpu: kalle_llasa_frame_head2_rows (csrc/llasa.hip: the RMSNorm pre-pass and R-row GEMM for W1, llasa_head2_kernel, the R-row
GEMM for Wa) element by element against the float64 reference of tests/llasa_head2_refs.py, by the method of
tests/test_llasa_head_gpu.py: every stage from its own inputs as the kernels published them, NaN-guarded buffers with row strides
larger than their widths, a fenced workspace, untouched memory compared bit for bit, wrong references caught.

Bounds (those of test_llasa_head_gpu.py, plus s / latent / kl for the predicted scale); u = 2^-24:
  h1, disp, x_next   K u sum_k |W_nk| |x_rk| + 4 u (|bias| + that sum)              (td.gemv_ref: an fp32 dot in any order)
  xn, a              the bf16 rounding of the float64 value, bit for bit, except within the stage's fp32 window of a rounding
                     boundary (capped at max(1, 1 %) of a row for the norm, max(1, 5 %) for the GELU: GELU_CAP of that file)
  s                  ALLOW["EXP"] u (1 + |logs|) s, from the logs the kernel stored: expf of this build is an exp2 of logs * log2(e),
                     whose argument error grows with |logs|.  ALLOW["EXP"] = 27 is the project's measured-x-4 allowance for
                     expf / logf; the worst ratio seen here is printed by test_every_stage_of_every_active_row (MEASURED, -s)
  latent             3 u (|mean| + |s noise|) (one product, one sum, or their fused form) + |noise| x the s bound, where the
                     reference is mean + s_fp64 noise; against the s the kernel stored the first part alone must hold, and does
  lat                the bf16 rounding of the fp32 latent the kernel stored: bit for bit
  kl                 per term 8 u of the magnitudes that enter it (1, logs, c1 rounded to fp32; m - 1, its square, s^2, one product,
                     three sums) + 2 x the s bound x s / (2 e^2) for the s^2 term (d(s^2) = 2 s ds), the fp32 sum of lat terms
                     in any order lat u sum_j |term_j|, both over lat, + (ALLOW["DIV"] + 1) u |kl| for the division
An INACTIVE row's inputs hold NaN and its outputs and workspace rows their fill, and must come back bit for bit."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc  # noqa: E402
import kernel_refs as kr  # noqa: E402
import llasa_head2_cases as hc  # noqa: E402
import llasa_head2_refs as hr  # noqa: E402
import test_decode_gpu as td  # noqa: E402
from gpu_checks import NAN, U, Guard, _bits, check, guarded as _guarded, clean as _clean  # noqa: E402
from test_llasa_head_gpu import FENCE, GELU_CAP, WRONG_MARGIN, caught, iarr, same_bits  # noqa: E402
from test_norm_elementwise_gpu import ALLOW  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
P = td.P
assert (hc.ERF_U, hc.DIV_U, hc.EXP_U) == (ALLOW["ERF"], ALLOW["DIV"], ALLOW["EXP"])
MEASURED = {}          # worst |s - exp(logs)| / (u (1 + |logs|) s) over the cases run so far


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


class Head:
    """one call on the inputs of hc.inputs(c): everything the call may write sits in NaN"""

    def __init__(self, lib, c, inactive=None, mask_arg=True):
        from kalle_audio_amd import _lib
        self.c, self.lib = c, lib
        R, D, lat = c["R"], c["D"], c["lat"]
        d2 = 2 * lat
        self.inactive = tuple(c["inactive"] if inactive is None else inactive)
        x = hc.inputs(c)
        self.h = Guard(R, D, ld=D + 4, init=x["h"].cuda())
        self.noise = Guard(R, lat, ld=lat + 3, init=x["noise"].cuda())
        for r in self.inactive:
            self.h.v[r], self.noise.v[r] = NAN, NAN
        self.w1 = Guard(d2, D, ld=D + 8, dtype=BF, init=x["w1"].cuda())
        self.w2 = Guard(d2, d2, ld=d2 + 8, dtype=BF, init=x["w2"].cuda())
        self.wa = Guard(D, lat, ld=lat + 16, dtype=BF, init=x["wa"].cuda())
        self.norm, self.b1, self.b2, self.ba = (x[k].cuda() for k in ("norm", "b1", "b2", "ba"))
        self.desc = _lib.LlasaHead()
        d = self.desc
        d.norm, d.w1, d.b1, d.w2, d.b2, d.wa, d.ba = (t.data_ptr() for t in (self.norm, self.w1.v, self.b1, self.w2.v, self.b2, self.wa.v, self.ba))
        d.ldw1, d.ldw2, d.ldwa = D + 8, d2 + 8, lat + 16
        self.bufs = {k: _guarded(torch.full(s, NAN, device="cuda")) for k, s in
                     (("disp", (R, d2)), ("latent", (R, lat)), ("kl", (R,)), ("x_next", (R, D)))}
        self.lay, self.ws_bytes = hc.ws_layout(R, D, lat)
        assert lib.kalle_llasa_head2_ws_bytes(R, D, lat) == self.ws_bytes
        self.wsbuf = torch.full((self.ws_bytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)   # all-ones bytes: NaN as fp32 and as bf16
        self.ws = self.wsbuf[FENCE:FENCE + self.ws_bytes]
        assert self.ws.data_ptr() % 64 == 0
        act = iarr([0 if r in self.inactive else 1 for r in range(R)]) if (mask_arg or self.inactive) else None
        self.rc = self.run(act)

    def run(self, act, **over):
        c = dict(self.c, ldh=self.c["D"] + 4)
        c.update(over)
        o = {k: v[1] for k, v in self.bufs.items()}
        rc = self.lib.kalle_llasa_frame_head2_rows(ctypes.addressof(self.desc), P(self.h.v), c["ldh"], P(self.noise.v), self.c["lat"] + 3,
                                                   ctypes.c_float(hc.EPS), P(o["disp"]), P(o["latent"]), P(o["kl"]), P(o["x_next"]),
                                                   act, c["R"], c["D"], c["lat"], P(self.ws), None)
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
    """(bf16 rounding of the float64 row v, allowance) as `rounded` of tests/test_llasa_head_gpu.py, with the allowance of an
    ambiguous element worked out for any window: the kernel rounds v + d, |d| <= window, so its result lies within
    floor(window / ulp + 1) bf16 ulps of the rounding of v - the one ulp ("either neighbour") of that file wherever the window
    is below an ulp, which is everywhere but on the far negative side of the GELU: at x = -5, x Phi(x) = -1.4e-6 has an ulp of
    1.5e-8 while 1 + erff(x / sqrt 2) alone cancels to an absolute 3e-8 |x| / 2.  Such elements are ambiguous and count
    towards the same cap."""
    amb = kr.bf16_ambiguous(v, window)
    assert amb.sum().item() <= max(1, cap * v.numel()), (what, "ambiguous elements over the cap", int(amb.sum()), v.numel())
    ulp = kr.bf16_ulp(v)
    return hr.bf16r(v), torch.where(amb, torch.floor(window / ulp + 1) * ulp, torch.zeros_like(v))


def stages(s, r, wrong=None):
    """the nine (name, kernel output, ref, tol) of row r, each from the inputs the kernels themselves read; `wrong` swaps one
    reference for a deliberately wrong one"""
    c = s.c
    D, lat = c["D"], c["lat"]
    d2 = 2 * lat
    ws = {k: s.region(k)[r].clone() for k in s.lay}
    o = {k: s.out(k)[r].clone() for k in s.bufs}
    res = []
    h = s.h.v[r].double()
    xh = hr.rms(h[None], s.norm.double(), hc.EPS)[0]
    ref, tol = rounded(xh, dc.rms_window(xh), f"xn row {r}")
    if wrong == "no_eps":
        ref = hr.bf16r(hr.rms(h[None], s.norm.double(), hc.EPS, "no_eps")[0])
    res.append(("xn", ws["xn"], ref, tol))
    ref, tol = td.gemv_ref(s.w1.v, ws["xn"].double(), D, res=s.b1.double())
    res.append(("h1", ws["h1"], ref, tol))
    h1 = ws["h1"].double()
    ref, tol = rounded(hr.gelu(h1), (ALLOW["ERF"] + 3) * U * h1.abs(), f"a row {r}", cap=GELU_CAP)
    res.append(("a", ws["a"], ref, tol))
    ref, tol = td.gemv_ref(s.w2.v, ws["a"].double(), d2, res=s.b2.double())
    res.append(("disp", o["disp"], ref, tol))
    swap = "swapped" if wrong == "swapped" else None
    m, logs = hr.halves(o["disp"].double(), swap)
    sref = hr.scale(logs, "fixed_std" if wrong == "fixed_std" else None)
    rs, rl = hr.halves(o["disp"].double())                 # (the tolerances are always those of the right reference)
    s_right = hr.scale(rl)
    s_tol = ALLOW["EXP"] * U * (1 + rl.abs()) * s_right
    res.append(("s", ws["s"], sref, s_tol))
    nz = s.noise.v[r].double()
    res.append(("latent", o["latent"], m + sref * nz, 3 * U * (rs.abs() + (s_right * nz).abs()) + nz.abs() * s_tol + 1e-30))
    res.append(("lat", ws["lat"], hr.bf16r(o["latent"].double()), torch.zeros(lat, dtype=torch.float64, device="cuda")))
    terms, mag = hr.kl_terms(rs, rl)
    ref = terms.mean()
    tol = ((8 * U * mag + 2 * s_tol * s_right / (2 * math.e ** 2)).sum() + lat * U * terms.abs().sum()) / lat + (ALLOW["DIV"] + 1) * U * ref.abs()
    if wrong in ("swapped", "over_d2", "reversed", "fixed_std"):
        ref = hr.kl(o["disp"].double()[None], wrong)[0]
    res.append(("kl", o["kl"].reshape(1), ref.reshape(1), tol.reshape(1)))
    ref, tol = td.gemv_ref(s.wa.v, ws["lat"].double(), lat, res=s.ba.double())
    res.append(("x_next", o["x_next"], ref, tol))
    return res


def measure_s(s, r):
    """|s - exp(logs)| / (u (1 + |logs|) s) of row r, worst element, and the sample held against the s the kernel itself stored"""
    lat = s.c["lat"]
    logs = s.out("disp")[r, lat:].double()
    m = s.out("disp")[r, :lat].double()
    got, ref = s.region("s")[r].double(), torch.exp(logs)
    MEASURED["EXP"] = max(MEASURED.get("EXP", 0.0), float(((got - ref).abs() / (U * (1 + logs.abs()) * ref)).max()))
    nz = s.noise.v[r].double()
    check(s.out("latent")[r], m + got * nz, 3 * U * (m.abs() + (got * nz).abs()) + 1e-30, f"row {r} latent from the stored s")


ALL = dict(hc.CASES, **{"small-h": hc.SMALL_H, "wide-scale": hc.WIDE_SCALE})


@pytest.fixture(scope="module")
def runs(kl):
    ops, lib = kl
    out = {}
    for name, c in ALL.items():
        s = Head(lib, c)
        assert s.rc == 0, (name, s.rc, lib.kalle_last_error())
        out[name] = s
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_every_stage_of_every_active_row(runs, name):
    s = runs[name]
    for r in range(s.c["R"]):
        if r in s.inactive:
            continue
        for stage, got, ref, tol in stages(s, r):
            assert torch.isfinite(got).all(), (name, r, stage, "NaN of an inactive row or of the fill leaked")
            check(got, ref, tol, f"{name} row {r} {stage}")
        measure_s(s, r)
    s.untouched(name)
    print(f"\n[head2] {name}: worst |s - exp(logs)| / (u (1 + |logs|) s) so far {MEASURED['EXP']:.3f}  (ALLOW['EXP'] = {ALLOW['EXP']})")
    assert 4 * MEASURED["EXP"] <= ALLOW["EXP"], ("four times the measured expf error exceeds the project's allowance", MEASURED)


@pytest.mark.parametrize("name", list(ALL))
def test_two_calls_give_equal_bits(kl, runs, name):
    ops, lib = kl
    s = runs[name]
    t = Head(lib, s.c)
    assert t.rc == 0
    for (k, a), b in zip(s.everything().items(), t.everything().values()):
        same_bits(a, b, f"{name} {k}")


@pytest.mark.parametrize("name", ["r3-hole", "r16-lat24", "r5-lat256", "r16-lat256-holes"])
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
    t = Head(lib, hc.CASES["r16-lat24"], mask_arg=False)
    assert t.rc == 0
    for (k, a), b in zip(runs["r16-lat24"].everything().items(), t.everything().values()):
        same_bits(a, b, k)


def test_small_magnitude_rows_take_eps_into_the_norm(runs):
    s = runs["small-h"]
    right = {k: (g, rf, t) for k, g, rf, t in stages(s, 0)}
    bad = {k: rf for k, _, rf, _ in stages(s, 0, wrong="no_eps")}
    caught(("RMSNorm without eps", *right["xn"], bad["xn"]))


def test_the_wide_scale_case_spans_three_decades_on_the_device(runs):
    s = runs["wide-scale"]
    sc, logs = s.region("s").double(), s.out("disp")[:, s.c["lat"]:].double()
    assert sc.max() / sc.min() > 1e3 and (logs > 1).any() and (logs < 1).any()


@pytest.mark.parametrize("wrong,moved", [("fixed_std", ("s", "latent", "kl")), ("swapped", ("s", "latent", "kl")), ("over_d2", ("kl",)),
                                         ("reversed", ("kl",))])
@pytest.mark.parametrize("name", ["r5-lat256", "wide-scale"])
def test_wrong_references_are_caught(runs, name, wrong, moved):
    """each wrong reference moves some element of every stage it reaches by more than WRONG_MARGIN x its allowance and fails the
    check the right one passes; every other stage's reference is the right one"""
    s = runs[name]
    right = {k: (g, rf, t) for k, g, rf, t in stages(s, 1)}
    bad = {k: rf for k, _, rf, _ in stages(s, 1, wrong=wrong)}
    for stage in moved:
        caught((f"{wrong} at {stage}", *right[stage], bad[stage]))
    for k in right:
        if k not in moved:
            assert torch.equal(bad[k], right[k][1]), (wrong, "moved the reference of", k)


def test_refusals_write_nothing(kl):
    ops, lib = kl
    s = Head(lib, hc.CASES["r3-hole"], inactive=(0, 1, 2))
    assert s.rc == 0                                                # every row inactive: KALLE_OK, nothing launched
    act = iarr([1, 1, 1])
    for over in (dict(R=0), dict(R=17), dict(lat=12), dict(lat=4), dict(lat=264), dict(D=4), dict(ldh=6)):
        assert s.run(act, **over) == -1, over
    assert (s.wsbuf == 0xFF).all()
    for k, (buf, view) in s.bufs.items():
        assert torch.isnan(buf).all(), k


def test_wrapper_runs_the_same_call(kl, runs):
    """ops.llasa_head2_plan / ops.llasa_frame_head2 on fp32 master weights: the bits of the direct call on their bf16 copies; a
    changed weight is read at the next call"""
    ops, lib = kl
    c = hc.CASES["r3-hole"]
    s = runs["r3-hole"]
    x = {k: v.cuda() for k, v in hc.inputs(c).items()}
    par = [torch.nn.Parameter(x[k].float()) for k in ("norm", "w1", "b1", "w2", "b2", "wa", "ba")]
    plan = ops.llasa_head2_plan(*par, c["R"], hc.EPS, "cuda", frames=2)
    assert tuple(plan["disp"].shape) == (2, 3, 16) and tuple(plan["latent"].shape) == (2, 3, 8) and tuple(plan["kl"].shape) == (2, 3)
    h = x["h"].clone()
    disp, latent, klv, x_next = ops.llasa_frame_head2(plan, h, x["noise"], active=[True, False, True], frame=1)
    torch.cuda.synchronize()
    assert disp.data_ptr() == plan["disp"][1].data_ptr() and latent.data_ptr() == plan["latent"][1].data_ptr()
    assert klv.data_ptr() == plan["kl"][1].data_ptr()
    for r in (0, 2):
        for k, t in (("disp", disp), ("latent", latent), ("kl", klv), ("x_next", x_next)):
            same_bits(t[r], s.out(k)[r], f"wrapper {k} row {r}")
    assert (disp[1] == 0).all() and (x_next[1] == 0).all() and (plan["latent"][0] == 0).all()     # (the plan's buffers start as zeros)
    before = disp.clone()
    with torch.no_grad():
        par[4].add_(0.25)                                           # b2
    disp2 = ops.llasa_frame_head2(plan, h, x["noise"], active=[True, False, True], frame=1)[0]
    torch.cuda.synchronize()
    assert torch.allclose(disp2[0], before[0] + 0.25, atol=1e-5)
