"""CPU side of the per-frame head (kalle_llasa_frame_head_rows, csrc/llasa.hip): the float64 reference of tests/llasa_head_refs.py
against torch's own modules; one table of refusals, each returned before any HIP call so the library is driven without a device;
the workspace size against the layout the header documents; the prototype and the descriptor as kalle_audio_amd._lib sees them."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llasa_head_cases as hc  # noqa: E402
import llasa_head_refs as hr  # noqa: E402

OK, ERR_ARG = 0, -1
FAKE = 4096                         # a non-NULL pointer for calls that must return before touching memory
FIELDS = ("norm", "w1", "b1", "w2", "b2", "wa", "ba")
BASE = dict(head=True, h=FAKE, ldh=128, noise=FAKE, ldn=16, std=0.5, mean=FAKE, latent=FAKE, kl=FAKE, x_next=FAKE, R=3, D=128, dl=16,
            ws=FAKE, ldw1=128, ldw2=16, ldwa=16)
REFUSED = ([dict(head=None)] + [{k: None} for k in ("h", "noise", "mean", "latent", "kl", "x_next", "ws")] +
           [dict(hole=f) for f in FIELDS] +
           [dict(R=0), dict(R=17), dict(dl=0, ldn=16), dict(dl=12, ldn=16), dict(dl=520, ldn=520, ldw2=520, ldwa=520),
            dict(D=4, ldh=128), dict(D=32776, ldh=32776, ldw1=32776), dict(std=0.0), dict(std=-0.5), dict(ldh=6),
            dict(ldh=120), dict(ldn=8), dict(ldw1=132), dict(ldw1=120), dict(ldw2=8), dict(ldwa=20)])


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def call(lib, hole=None, active=None, **over):
    """kalle_llasa_frame_head_rows on BASE with `over`; hole: that descriptor field is NULL"""
    from kalle_audio_amd import _lib
    a = dict(BASE)
    a.update(over)
    d = _lib.LlasaHead()
    for f in FIELDS:
        setattr(d, f, None if hole == f else FAKE)
    d.ldw1, d.ldw2, d.ldwa = a["ldw1"], a["ldw2"], a["ldwa"]
    act = None if active is None else ctypes.cast((ctypes.c_int32 * len(active))(*active), ctypes.c_void_p)
    return lib.kalle_llasa_frame_head_rows(ctypes.addressof(d) if a["head"] else None, a["h"], a["ldh"], a["noise"], a["ldn"],
                                           ctypes.c_float(a["std"]), ctypes.c_float(hc.EPS), a["mean"], a["latent"], a["kl"],
                                           a["x_next"], act, a["R"], a["D"], a["dl"], a["ws"], None)


@pytest.mark.parametrize("kw", REFUSED, ids=str)
def test_refusals_return_err_arg_before_any_hip_call(lib, kw):
    """KALLE_ERR_ARG, not the KALLE_ERR_LAUNCH of a launch without a device"""
    assert call(lib, active=(1, 1, 1), **kw) == ERR_ARG


def test_every_row_inactive_is_ok_and_launches_nothing(lib):
    assert call(lib, active=(0, 0, 0)) == OK
    assert call(lib, active=(0,) * 16, R=16) == OK
    assert call(lib, active=(0, 0, 0), hole="w2") == ERR_ARG           # (the arguments are still checked)


@pytest.mark.parametrize("c", list(hc.CASES.values()) + [dict(R=16, D=32768, dl=8), dict(R=1, D=8, dl=8)], ids=str)
def test_workspace_size_is_the_documented_layout(lib, c):
    lay, total = hc.ws_layout(c["R"], c["D"], c["dl"])
    assert lib.kalle_llasa_head_ws_bytes(c["R"], c["D"], c["dl"]) == total
    assert all(o % 64 == 0 for o, _, _, _ in lay.values()) and total % 64 == 0
    assert list(lay) == ["xn", "h1", "a", "lat"]


def test_workspace_size_refusals(lib):
    for a in ((0, 128, 16), (17, 128, 16), (3, 4, 16), (3, 132, 16), (3, 32776, 16), (3, 128, 0), (3, 128, 12), (3, 128, 520), (-1, 128, 16)):
        assert lib.kalle_llasa_head_ws_bytes(*a) <= 0, a


def test_prototype_and_descriptor_parse(lib):
    from kalle_audio_amd import _lib
    protos = _lib.parse_header()
    vp, i32, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert protos["kalle_llasa_frame_head_rows"] == (ctypes.c_int, [vp, vp, i64, vp, i64, f, f, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp])
    assert protos["kalle_llasa_head_ws_bytes"] == (ctypes.c_int, [i32, i32, i32])
    assert [n for n, _ in _lib.LlasaHead._fields_] == list(FIELDS) + ["ldw1", "ldw2", "ldwa"]
    assert ctypes.sizeof(_lib.LlasaHead) == 7 * 8 + 3 * 8
    assert lib.kalle_abi_version() == 2


def test_reference_without_roundings_is_torch_in_fp64():
    """tests/llasa_head_refs.py with round_points=False against F.rms_norm, nn.Linear, nn.GELU and kl_divergence, all float64"""
    from torch import nn
    from torch.distributions import Normal, kl_divergence
    c = dict(R=5, D=96, dl=24)
    x = {k: v.double() for k, v in hc.inputs(c).items()}
    s = hr.head(x["h"], x["norm"], x["w1"], x["b1"], x["w2"], x["b2"], x["wa"], x["ba"], x["noise"], hc.STD, hc.EPS, round_points=False)

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
        mean = lin(x["w2"], x["b2"])(a)
        latent = mean + hc.STD * x["noise"]
        kl = kl_divergence(Normal(mean, torch.tensor(hc.STD, dtype=torch.float64)),
                           Normal(torch.tensor(1.0, dtype=torch.float64), torch.tensor(math.e, dtype=torch.float64))).mean(-1)
        x_next = lin(x["wa"], x["ba"])(latent)
    for k, v in dict(xn=xn, h1=h1, a=a, mean=mean, latent=latent, lat=latent, kl=kl, x_next=x_next).items():
        err = ((s[k] - v).abs() / (v.abs() + 1.0)).max().item()
        assert err < 1e-13, (k, err)
    # the rounding points move what they should and nothing before them
    r = hr.head(x["h"], x["norm"], x["w1"], x["b1"], x["w2"], x["b2"], x["wa"], x["ba"], x["noise"], hc.STD, hc.EPS)
    for k in ("xn", "a", "lat"):
        assert torch.equal(r[k], r[k].to(torch.bfloat16).double()) and not torch.equal(r[k], s[k])


def test_the_wrong_references_differ_from_the_right_ones():
    m = torch.linspace(-2, 3, 24, dtype=torch.float64)[None]
    right = hr.kl(m, hc.STD)
    for w in ("no_half", "kl_vs_n01", "no_std2"):
        assert (hr.kl(m, hc.STD, w) - right).abs().min() > 1e-3, w
    x = torch.linspace(-3, 3, 64, dtype=torch.float64)
    assert 1e-5 < (hr.gelu(x, "tanh") - hr.gelu(x)).abs().max() < 1e-3
    h = torch.full((1, 8), 1e-3, dtype=torch.float64)
    g = torch.ones(8, dtype=torch.float64)
    assert (hr.rms(h, g, hc.EPS, "no_eps") / hr.rms(h, g, hc.EPS)).min() > 3
