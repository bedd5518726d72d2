"""CPU side of the mean || log-scale per-frame head (kalle_llasa_frame_head2_rows, csrc/llasa.hip): the float64 reference of
tests/llasa_head2_refs.py against torch's own modules; one table of refusals, each returned before any HIP call so the library is
driven without a device; the workspace size against the layout the header documents; the prototypes as kalle_audio_amd._lib sees
them; and the cases themselves - that the reference inputs alone keep the elements a bf16 rounding cannot decide within the caps
the GPU test applies (1 % of a row for the norm, 5 % for the GELU), and that the wide-scale case is as wide as it claims."""
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

OK, ERR_ARG = 0, -1
U = 2.0 ** -24
NORM_CAP, GELU_CAP = 0.01, 0.05     # those of tests/test_llasa_head_gpu.py
FAKE = 4096                         # a non-NULL pointer for calls that must return before touching memory
FIELDS = ("norm", "w1", "b1", "w2", "b2", "wa", "ba")
BASE = dict(head=True, h=FAKE, ldh=128, noise=FAKE, ldn=8, disp=FAKE, latent=FAKE, kl=FAKE, x_next=FAKE, R=3, D=128, lat=8,
            ws=FAKE, ldw1=128, ldw2=16, ldwa=8)
REFUSED = ([dict(head=None)] + [{k: None} for k in ("h", "noise", "disp", "latent", "kl", "x_next", "ws")] +
           [dict(hole=f) for f in FIELDS] +
           [dict(R=0), dict(R=17), dict(lat=0), dict(lat=12, ldn=16, ldw2=24, ldwa=16), dict(lat=4),
            dict(lat=264, ldn=264, ldw2=528, ldwa=264), dict(lat=512, ldn=512, ldw2=1024, ldwa=512), dict(lat=-8),
            dict(D=4, ldh=128), dict(D=32776, ldh=32776, ldw1=32776), dict(ldh=6), dict(ldh=120), dict(ldh=130), dict(ldn=4),
            dict(ldw1=132), dict(ldw1=120), dict(ldw2=8), dict(ldw2=20), dict(ldwa=0), dict(ldwa=12)])


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def call(lib, hole=None, active=None, **over):
    """kalle_llasa_frame_head2_rows on BASE with `over`; hole: that descriptor field is NULL"""
    from kalle_audio_amd import _lib
    a = dict(BASE)
    a.update(over)
    d = _lib.LlasaHead()
    for f in FIELDS:
        setattr(d, f, None if hole == f else FAKE)
    d.ldw1, d.ldw2, d.ldwa = a["ldw1"], a["ldw2"], a["ldwa"]
    act = None if active is None else ctypes.cast((ctypes.c_int32 * len(active))(*active), ctypes.c_void_p)
    return lib.kalle_llasa_frame_head2_rows(ctypes.addressof(d) if a["head"] else None, a["h"], a["ldh"], a["noise"], a["ldn"],
                                            ctypes.c_float(hc.EPS), a["disp"], a["latent"], a["kl"], a["x_next"], act, a["R"],
                                            a["D"], a["lat"], a["ws"], None)


@pytest.mark.parametrize("kw", REFUSED, ids=str)
def test_refusals_return_err_arg_before_any_hip_call(lib, kw):
    """KALLE_ERR_ARG, not the KALLE_ERR_LAUNCH of a launch without a device"""
    assert call(lib, active=(1, 1, 1), **kw) == ERR_ARG


def test_every_row_inactive_is_ok_and_launches_nothing(lib):
    assert call(lib, active=(0, 0, 0)) == OK
    assert call(lib, active=(0,) * 16, R=16) == OK
    assert call(lib, active=(0, 0, 0), lat=256, ldn=256, ldw2=512, ldwa=256) == OK       # (the bound itself is taken)
    assert call(lib, active=(0, 0, 0), hole="w2") == ERR_ARG                             # (the arguments are still checked)


@pytest.mark.parametrize("c", list(hc.CASES.values()) + [hc.SMALL_H, hc.WIDE_SCALE, dict(R=16, D=32768, lat=8), dict(R=1, D=8, lat=8)],
                         ids=str)
def test_workspace_size_is_the_documented_layout(lib, c):
    lay, total = hc.ws_layout(c["R"], c["D"], c["lat"])
    assert lib.kalle_llasa_head2_ws_bytes(c["R"], c["D"], c["lat"]) == total
    assert all(o % 64 == 0 for o, _, _, _ in lay.values()) and total % 64 == 0
    assert list(lay) == ["xn", "h1", "a", "s", "lat"]


def test_workspace_size_refusals(lib):
    for a in ((0, 128, 8), (17, 128, 8), (3, 4, 8), (3, 132, 8), (3, 32776, 8), (3, 128, 0), (3, 128, 12), (3, 128, 264), (3, 128, 512),
              (-1, 128, 8)):
        assert lib.kalle_llasa_head2_ws_bytes(*a) <= 0, a


def test_prototypes_parse(lib):
    from kalle_audio_amd import _lib, ops
    protos = _lib.parse_header()
    vp, i32, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert protos["kalle_llasa_frame_head2_rows"] == (ctypes.c_int, [vp, vp, i64, vp, i64, f, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp])
    assert protos["kalle_llasa_head2_ws_bytes"] == (ctypes.c_int, [i32, i32, i32])
    assert ops.HEAD2_MAX_LATENT == hc.MAX_LAT == 256 and ops.DECODE_MAX_ROWS == hc.MAX_ROWS


def test_reference_without_roundings_is_torch_in_fp64():
    """tests/llasa_head2_refs.py with round_points=False against F.rms_norm, nn.Linear, nn.GELU and kl_divergence, all float64"""
    from torch import nn
    from torch.distributions import Normal, kl_divergence
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    for c in (dict(R=5, D=96, lat=24), dict(hc.WIDE_SCALE, D=96)):
        x = {k: v.double() for k, v in hc.inputs(c).items()}
        s = hr.head(x["h"], x["norm"], x["w1"], x["b1"], x["w2"], x["b2"], x["wa"], x["ba"], x["noise"], hc.EPS, round_points=False)

        def lin(w, b):
            m = nn.Linear(w.shape[1], w.shape[0]).double()
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(b)
            return m

        with torch.no_grad():
            xn = torch.nn.functional.rms_norm(x["h"], (c["D"],), x["norm"], hc.EPS)
            h1 = lin(x["w1"], x["b1"])(xn)
            a = nn.GELU()(h1)
            disp = lin(x["w2"], x["b2"])(a)
            mean, logs = disp[:, :c["lat"]], disp[:, c["lat"]:]
            sc = torch.exp(logs)
            latent = mean + sc * x["noise"]
            kl = kl_divergence(Normal(mean, sc), Normal(f64(1.0), f64(math.e))).mean(-1)
            x_next = lin(x["wa"], x["ba"])(latent)
        for k, v in dict(xn=xn, h1=h1, a=a, disp=disp, s=sc, latent=latent, lat=latent, kl=kl, x_next=x_next).items():
            err = ((s[k] - v).abs() / (v.abs() + 1.0)).max().item()
            assert err < 1e-13, (k, err)
        # the rounding points move what they should and nothing before them
        r = hr.head(x["h"], x["norm"], x["w1"], x["b1"], x["w2"], x["b2"], x["wa"], x["ba"], x["noise"], hc.EPS)
        for k in ("xn", "a", "lat"):
            assert torch.equal(r[k], r[k].to(torch.bfloat16).double()) and not torch.equal(r[k], s[k])


def reference(c):
    x = {k: v.double() for k, v in hc.inputs(c).items()}
    return x, hr.head(x["h"], x["norm"], x["w1"], x["b1"], x["w2"], x["b2"], x["wa"], x["ba"], x["noise"], hc.EPS)


@pytest.mark.parametrize("name,c", list(hc.CASES.items()) + [("small-h", hc.SMALL_H), ("wide", hc.WIDE_SCALE)], ids=lambda v: v if isinstance(v, str) else "")
def test_reference_inputs_stay_within_the_rounding_caps(name, c):
    """the elements a bf16 rounding cannot decide, counted on the float64 reference alone with the windows the GPU test uses: at
    most max(1, 1 %) of a row at the norm and max(1, 5 %) at the GELU.  (The kernel's h1 differs from the reference's by fp32
    dot-product error, far below the spread of h1: the same distribution, so the same expected count.)"""
    x, s = reference(c)
    for r in range(c["R"]):
        xh = hr.rms(x["h"][r:r + 1], x["norm"], hc.EPS)[0]
        n = int(kr.bf16_ambiguous(xh, dc.rms_window(xh)).sum())
        assert n <= max(1, NORM_CAP * c["D"]), (name, r, "norm", n)
        h1 = s["h1"][r]
        n = int(kr.bf16_ambiguous(hr.gelu(h1), (hc.ERF_U + 3) * U * h1.abs()).sum())
        assert n <= max(1, GELU_CAP * 2 * c["lat"]), (name, r, "gelu", n)
    assert torch.isfinite(s["kl"]).all() and torch.isfinite(s["x_next"]).all()


def test_the_wide_scale_case_is_wide_and_the_small_h_case_small():
    x, s = reference(hc.WIDE_SCALE)
    logs = hr.halves(s["disp"])[1]
    assert logs.min() < -5.0 and 1.5 < logs.max() < 3.0
    assert s["s"].max() / s["s"].min() > 1e3                         # three decades
    assert ((1.0 - logs) > 0).any() and ((1.0 - logs) < 0).any()     # log(e / s) changes sign
    x, _ = reference(hc.SMALL_H)
    assert x["h"].pow(2).mean(-1).max() < 2 * hc.EPS
    for c in hc.CASES.values():                                      # the ordinary cases: halves around 1 and -1
        if c["lat"] < 64:                                            # (eight or 24 draws do not pin their own mean)
            continue
        _, s = reference(c)
        mean, logs = hr.halves(s["disp"])
        assert 0.5 < mean.mean() < 1.5 and -1.5 < logs.mean() < -0.5


def test_the_wrong_references_differ_from_the_right_ones():
    g = torch.Generator().manual_seed(5)
    disp = torch.cat([1.0 + 0.5 * torch.randn(4, 24, generator=g), -1.0 + 0.5 * torch.randn(4, 24, generator=g)], dim=1).double()
    right = hr.kl(disp)
    for w in ("swapped", "over_d2", "reversed", "fixed_std"):
        assert (hr.kl(disp, w) - right).abs().min() > 1e-3, w
    assert torch.allclose(hr.kl(disp, "over_d2") * 2, right)
    mean, logs = hr.halves(disp)
    assert (hr.scale(logs, "fixed_std") - hr.scale(logs)).abs().min() > 1e-3
    assert torch.equal(hr.halves(disp, "swapped")[0], logs)
