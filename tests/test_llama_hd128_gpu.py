"""-m gpu: the Llama path at head dim 128 (Llama-3.2-3B / Llama-3.1-8B head layout) - the tiled forward and the two-pass backward
at rot = 128, the single-query kernel attn_decode128_kernel behind kalle_attention_decode_hd, kalle_llama_decode_step_hd stage by
stage, and the drop-in modules against the reference's fixture (tests/golden/llasa_hd128.npz).

Conventions, operands, bounds and allowances are those of tests/test_attention_gpu.py and tests/test_decode_gpu.py, imported:
every element against the fp64 references of tests/kernel_refs.py inside ALLOW[...] x the derived unit (both scale with dh and K),
outputs in NaN-guarded allocations, the plan word of every call asserted.  run_case mirrors test_attention_gpu.run_case with this
file's own PLANS_SEEN / MEASURED (that file asserts set equality on its own at its end).

One case of the issue's list meets a hole in the header's contract: (128, 128) causal with the `row` mask has a batch element
whose keys are all masked, and "with causal != 0 as well such a row is not defined" (include/kalle_hip.h: -1e30 is also what a
causally excluded key gets).  For that batch element the forward's out / lse are held to finiteness only; its backward (exact
zeros, the header's contract) and everything of the other batch element are checked like every other case."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import attn_cases as ac  # noqa: E402
import decode_cases as dc  # noqa: E402
import golden_util as gu  # noqa: E402
import kernel_refs as kr  # noqa: E402
import llama_hd128_cases as lc128  # noqa: E402
import test_attention_gpu as ta  # noqa: E402
import test_decode_gpu as td  # noqa: E402
from gpu_checks import NAN, U, Guard, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402
from test_attention_gpu import ALLOW, BF, A, B, Operand, _id, layout, make_inputs, wrong_kw  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
HD = lc128.HD
MEASURED = {}
PLANS_SEEN = set()
SEEN = set()
FAMILY = {1: "tiled", 2: "decode", 3: "two_pass", 6: "decode"}       # family 6 rounds where family 2 does: its allowances
G = os.path.join(HERE, "golden")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def _chk(out, ref, key, unit, what):
    return check(out, ref, ALLOW[key] * U * unit, what, key, unit, MEASURED)


# ================================================================================================ one attention case
def run_case(kl, c, seed=None, wrong=None, inputs=None, entry="fwd_hd"):
    """test_attention_gpu.run_case with `entry`: "fwd_hd" kalle_attention_fwd_hd, "decode" kalle_attention_decode_hd (Nq == 1, the
    case is causal: the query is the last position)"""
    ops, lib = kl
    st = ops._stream()
    dh, H, Hkv, Nq, Nk, rot, causal = (c[k] for k in ("dh", "H", "Hkv", "Nq", "Nk", "rot", "causal"))
    what = _id(c) + ("-decode_hd" if entry == "decode" else "")
    x = inputs or make_inputs(c, seed)
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    q, k, v, dout, mask = cu(x["q"]), cu(x["k"]), cu(x["v"]), cu(x["dout"]), cu(x["mask"])
    cos, sin = cu(x["cos"]), cu(x["sin"])
    cosd, sind = (cos.double(), sin.double()) if rot else (None, None)
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    ldq, q_off, ldk, k_off, ldv, v_off = layout(c)
    nanf = lambda n: torch.full((B, n, 8), NAN, device="cuda", dtype=torch.float64)  # noqa: E731
    if c["layout"] == "fused":
        qb = kb = vb = Operand(torch.cat([q, nanf(Nq), k, nanf(Nq), v], -1), ldq, q_off).buf
    else:
        qb = Operand(q, ldq, q_off).buf
        kb = vb = Operand(torch.cat([k, nanf(Nk), v], -1), ldk, k_off).buf
    ldo = H * dh + 16
    fill = -1.0e30 * dh ** -0.5
    fam_f = FAMILY[c["fwd"] & 15]
    fw = wrong if wrong not in ("dk_missing_head", "dq_not_unrotated", "delta_dout_squared") else None
    args = (H, Hkv, dh, rot, cosd, sind, mask, causal)
    ref, rlse, p, qh, kh = kr.attention_ref(q, k, v, *args, round_points=True, mask_fill=fill, wrong=wrong_kw(fw, c) if fw else None)
    if wrong is None:
        for (b, h, r, j) in x["hot"]:
            assert p[b, h, r, j] >= 0.2, (what, "hot key", b, h, r, j, float(p[b, h, r, j]))
    # batch elements the header leaves undefined in the forward: causal and every key masked
    defined = torch.ones(B, dtype=torch.bool, device="cuda") if mask is None or not causal else mask.any(1)
    og = Guard(B * Nq, H * dh, ldo, torch.bfloat16, col0=8)
    lbuf, lse = _guarded(torch.full((B, H, Nq), NAN, device="cuda"))
    op = og.buf.data_ptr() + 16
    head = (P(qb), ldq, q_off, P(kb), ldk, k_off, P(vb), ldv, v_off, op, ldo, P(lse), P(cos), P(sin), rot, P(m8))
    if entry == "decode":
        assert Nq == 1 and causal
        fa = head + (B, H, Hkv, Nk, dh)
        word = ta.asked(lib, "decode", fa)
        rc = lib.kalle_attention_decode_hd(*fa, st)
    else:
        fa = head + (int(causal), B, H, Hkv, Nq, Nk, dh)
        word = ta.asked(lib, "fwd", fa)
        rc = lib.kalle_attention_fwd_hd(*fa, st)
    plan = lib.kalle_attn_last_plan()
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    assert plan == c["fwd"], (what, hex(plan), hex(c["fwd"]))
    assert word == plan, (what, "the query named", hex(word))
    PLANS_SEEN.add(plan)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, v, ref, rlse, H, Hkv, dh)
    out = og.v.reshape(B, Nq, H * dh)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all(), (what, "not finite")
    _chk(out[defined], ref[defined], "out/" + fam_f, BF * u_out[defined], what + " out")
    _chk(lse[defined], rlse[defined], "lse/" + fam_f, u_lse[defined], what + " lse")
    og.clean(what + " out")
    _clean(lbuf, lse, what + " lse")
    res = (out.double(), ref, ALLOW["out/" + fam_f] * 2.0 ** -9 * u_out, lse.double(), rlse, ALLOW["lse/" + fam_f] * U * u_lse)
    if c["bwd"] is None:
        return res
    fam_b = FAMILY[c["bwd"] & 15]
    right = kr.attention_ref(q, k, v, *args, round_points=True, mask_fill=fill) if fw is not None else (ref, rlse)
    out_b, lse_in = right[0].to(torch.bfloat16), right[1].float().contiguous()
    oo, do = Operand(out_b, ldo, 8), Operand(dout, ldo, 8)
    dbuf, delta = _guarded(torch.full((B, H, Nq), NAN, device="cuda"))
    dqg = Guard(B * Nq, H * dh, ldq, torch.bfloat16, col0=q_off)
    dkg = Guard(B * Nk, Hkv * dh, ldk, torch.bfloat16, col0=k_off)
    dvg = Guard(B * Nk, Hkv * dh, ldv, torch.bfloat16, col0=v_off)
    ba = (P(qb), ldq, q_off, P(kb), ldk, k_off, P(vb), ldv, v_off, oo.buf.data_ptr() + 16, do.buf.data_ptr() + 16, ldo,
          P(lse_in), P(delta), P(dqg.buf), P(dkg.buf), P(dvg.buf), P(cos), P(sin), rot, P(m8), int(causal), B, H, Hkv, Nq, Nk, dh)
    word = ta.asked(lib, "bwd", ba)
    rc = lib.kalle_attention_bwd_hd(*ba, st)
    plan = lib.kalle_attn_last_plan()
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    assert plan == c["bwd"], (what, hex(plan), hex(c["bwd"]))
    assert word == plan, (what, "the query named", hex(word))
    PLANS_SEEN.add(plan)
    rdq, rdk, rdv, rdelta, mags = kr.attention_bwd_ref(q, k, v, dout, *args, round_points=True, out=out_b.double(), masked_rows_zero=True,
                                                       wrong=wrong_kw(wrong, c) if wrong else None)
    ob = out_b.double().reshape(B, Nq, H, dh).transpose(1, 2)
    dob = dout.reshape(B, Nq, H, dh).transpose(1, 2)
    check(delta, rdelta, (dh + 2) * U * (ob * dob).abs().sum(-1) + 1e-30, what + " delta")
    _chk(dqg.v.reshape(B, Nq, H * dh), rdq, "dq/" + fam_b, BF * mags["dq"], what + " dq")
    _chk(dkg.v.reshape(B, Nk, Hkv * dh), rdk, "dk/" + fam_b, BF * mags["dk"], what + " dk")
    _chk(dvg.v.reshape(B, Nk, Hkv * dh), rdv, "dv/" + fam_b, BF * mags["dv"], what + " dv")
    if mask is not None:
        dead = ~mask
        for name, t in (("dk", dkg.v.reshape(B, Nk, -1)), ("dv", dvg.v.reshape(B, Nk, -1))):
            assert (t[dead] == 0).all(), (what, name, "of a masked key is not exactly zero")
        full = ~mask.any(1)
        assert (dqg.v.reshape(B, Nq, -1)[full] == 0).all(), (what, "dq of a fully masked batch row is not exactly zero")
    for gd, name in ((dqg, "dq"), (dkg, "dk"), (dvg, "dv")):
        gd.clean(what + " " + name)
    _clean(dbuf, delta, what + " delta")
    return res


# ================================================================================================ 1: tiled + two-pass at rot 128
@pytest.mark.parametrize("c", lc128.TILED_CASES, ids=_id)
def test_tiled_forward_and_two_pass_backward_at_rot_128(kl, c):
    run_case(kl, c)


# ================================================================================================ 2: the bounds bite at rot 128
@pytest.mark.parametrize("wrong,c", lc128.WRONG, ids=[w[0] for w in lc128.WRONG])
def test_wrong_references_are_caught_at_rot_128(kl, wrong, c):
    run_case(kl, c)
    saved = dict(MEASURED)
    try:
        with pytest.raises(AssertionError, match="out of bound"):
            run_case(kl, c, wrong=wrong)
    finally:
        MEASURED.clear()
        MEASURED.update(saved)


# ================================================================================================ 3: the single-query kernel
@pytest.mark.parametrize("c", lc128.DECODE_CASES, ids=_id)
def test_single_query_kernel_at_head_dim_128(kl, c):
    run_case(kl, c, entry="decode")
    SEEN.add("Nk=%d" % c["Nk"])


# ================================================================================================ 4: single-query vs tiled
def test_single_query_agrees_with_tiled_per_element_at_head_dim_128(kl):
    c2 = A(2, 33, lc128.T128, None, dh=HD, rot=HD, causal=True, H=4, Hkv=1, mask="random")
    c1 = dict(c2, Nq=1, fwd=lc128.decode128())
    o2, r2, t2, l2, rl2, tl2 = run_case(kl, c2)
    x = make_inputs(c2)
    x["q"], x["dout"], x["hot"] = x["q"][:, 1:].contiguous(), x["dout"][:, 1:].contiguous(), []
    o1, r1, t1, l1, rl1, tl1 = run_case(kl, c1, inputs=x, entry="decode")
    assert (r1[:, 0] - r2[:, 1]).abs().max() < 1e-12
    check(o1[:, 0], o2[:, 1], t1[:, 0] + t2[:, 1], "decode128 vs tiled out")
    check(l1[:, :, 0], l2[:, :, 1], tl1[:, :, 0] + tl2[:, :, 1], "decode128 vs tiled lse")


# ================================================================================================ 5: decode_hd at head dim 64
@pytest.mark.parametrize("rot", [0, 32, 64])
def test_decode_hd_at_head_dim_64_is_attention_fwd_bit_for_bit(kl, rot):
    ops, lib = kl
    st = ops._stream()
    c = A(1, 257, lc128.decode64(rot), None, rot=rot, causal=True, H=4, Hkv=2, mask="random")
    x = make_inputs(c)
    ldq, q_off, ldk, k_off, ldv, v_off = layout(c)
    qb = Operand(x["q"].cuda(), ldq, q_off).buf
    kb = Operand(torch.cat([x["k"].cuda(), torch.full((B, 257, 8), NAN, device="cuda", dtype=torch.float64), x["v"].cuda()], -1), ldk, k_off).buf
    cos, sin = (x["cos"].cuda(), x["sin"].cuda()) if rot else (None, None)
    m8 = x["mask"].cuda().to(torch.uint8).contiguous()
    outs = []
    for new in (False, True):
        og = Guard(B, 4 * 64, 4 * 64 + 16, torch.bfloat16, col0=8)
        lbuf, lse = _guarded(torch.full((B, 4, 1), NAN, device="cuda"))
        head = (P(qb), ldq, q_off, P(kb), ldk, k_off, P(kb), ldv, v_off, og.buf.data_ptr() + 16, 4 * 64 + 16, P(lse), P(cos), P(sin), rot, P(m8))
        word = ta.asked(lib, "decode", head + (B, 4, 2, 257, 64)) if new else ta.asked(lib, "fwd", head + (1, B, 4, 2, 1, 257, 64))
        rc = lib.kalle_attention_decode_hd(*head, B, 4, 2, 257, 64, st) if new else lib.kalle_attention_fwd(*head, 1, B, 4, 2, 1, 257, st)
        plan = lib.kalle_attn_last_plan()
        torch.cuda.synchronize()
        assert rc == 0 and plan == lc128.decode64(rot), (rc, hex(plan))
        assert word == plan, ("the query named", hex(word))
        og.clean("out")
        _clean(lbuf, lse, "lse")
        assert torch.isfinite(og.v).all() and torch.isfinite(lse).all()
        outs.append((og.v.clone(), lse.clone()))
        if new:
            PLANS_SEEN.add(plan)
    _exact(outs[1][0], outs[0][0], "out")
    _exact(outs[1][1], outs[0][1], "lse")


# ================================================================================================ 6: rejections
def test_rejected_attention_calls_write_nothing(kl):
    ops, lib = kl
    st = ops._stream()
    N, H = 16, 2
    z = torch.zeros((B * N + 2, 3 * H * HD + 32), device="cuda", dtype=torch.bfloat16)
    cos, sin = (t.cuda() for t in ta.rope_tables(N, HD))
    og, lse = Guard(B, H * HD, H * HD + 16, torch.bfloat16), Guard(B, H)
    base = dict(ldq=z.shape[1], q_off=8, ldk=z.shape[1], k_off=16 + H * HD, ldv=z.shape[1], v_off=24 + 2 * H * HD, ldo=H * HD + 16,
                cos=P(cos), sin=P(sin), rot=HD, H=H, Hkv=H, Nk=N, dh=HD)
    bad = [dict(dh=32, rot=32), dict(dh=96), dict(dh=64, rot=128), dict(rot=48), dict(rot=64), dict(rot=0), dict(cos=None), dict(sin=None),
           dict(H=3, Hkv=2), dict(q_off=4), dict(k_off=20 + H * HD), dict(v_off=12), dict(ldk=z.shape[1] + 4), dict(ldo=H * HD + 12), dict(Nk=0)]
    for kw in bad:
        a = dict(base)
        a.update(kw)
        rc = lib.kalle_attention_decode_hd(P(z), a["ldq"], a["q_off"], P(z), a["ldk"], a["k_off"], P(z), a["ldv"], a["v_off"], P(og.buf), a["ldo"],
                                           P(lse.buf), a["cos"], a["sin"], a["rot"], None, B, a["H"], a["Hkv"], a["Nk"], a["dh"], st)
        assert (rc, lib.kalle_attn_last_plan()) == (ERR_ARG, 0), (kw, rc, hex(lib.kalle_attn_last_plan()))
    torch.cuda.synchronize()
    og.untouched("out")
    lse.untouched("lse")


# ================================================================================================ 7: the decode step at head dim 128
F32_EPS, BF16_REL, FENCE = td.F32_EPS, td.BF16_REL, td.FENCE


class Layer:
    def __init__(self, c, g, index, hd=HD):
        H, Hkv, inner, t0, rows = c["H"], c["Hkv"], c["inner"], c["t0"], c["rows"]
        D, kvw = hd * H, 2 * hd * Hkv
        cpu = torch.Generator().manual_seed(c["seed"] + 1000 + index)
        self.input_norm = (lc128.stage1_inputs(c)[1] if index == 0 else 1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.post_norm = (1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.wqkv, self.wo = td.dev_weight(D + kvw, D, g), td.dev_weight(D, D, g)
        self.wug, self.wdown = td.dev_weight(2 * inner, D, g), td.dev_weight(D, inner, g)
        cache = torch.full((rows, kvw), NAN, device="cuda", dtype=torch.bfloat16)
        cache[:t0] = (torch.randn((t0, kvw), generator=g, device="cuda") * 0.8).to(torch.bfloat16)
        self.cache_buf, self.cache = _guarded(cache)
        self.cache_before = self.cache.clone()

    def fields(self):
        return [self.input_norm, self.wqkv, self.wo, self.post_norm, self.wug, self.wdown, self.cache]


class Setup:
    def __init__(self, lib, c, n_layers=1):
        from kalle_audio_amd import _lib
        self.c, self.lib = c, lib
        H, Hkv, inner = c["H"], c["Hkv"], c["inner"]
        self.D = HD * H
        g = torch.Generator(device="cuda").manual_seed(c["seed"])
        self.layers = [Layer(c, g, i) for i in range(n_layers)]
        self.arr = (_lib.LlamaLayer * n_layers)()
        for d, L in zip(self.arr, self.layers):
            d.input_norm, d.wqkv, d.wo, d.post_norm, d.wug, d.wdown, d.kv_cache = (t.data_ptr() for t in L.fields())
        self.xbuf, self.x = _guarded(lc128.stage1_inputs(c)[0].cuda())
        self.obuf, self.out = _guarded(torch.full((self.D,), NAN, device="cuda"))
        cos, sin = lc128.rope_tables(c["rows"])
        cos[c["t0"] + 1:], sin[c["t0"] + 1:] = NAN, NAN
        self.cos, self.sin = cos.cuda(), sin.cuda()
        self.ws_bytes = lib.kalle_llama_decode_ws_bytes_hd(H, Hkv, inner, HD)
        assert self.ws_bytes == 8 * self.D + ((4 * H + 63) & ~63) + 4 * self.D + 4 * inner
        self.wsbuf = torch.full((self.ws_bytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)
        self.ws = self.wsbuf[FENCE:FENCE + self.ws_bytes]
        assert self.ws.data_ptr() % 64 == 0

    def step(self, n_layers=None, x=None, layer0=0, **over):
        c = self.c
        a = dict(H=c["H"], Hkv=c["Hkv"], inner=c["inner"], t0=c["t0"], rows=c["rows"], hd=HD)
        a.update(over)
        arr = ctypes.c_void_p(ctypes.addressof(self.arr) + layer0 * ctypes.sizeof(self.arr[0]))
        return self.lib.kalle_llama_decode_step_hd(arr, len(self.layers) if n_layers is None else n_layers, P(self.x if x is None else x),
                                                   P(self.out), a["H"], a["Hkv"], a["inner"], a["hd"], ctypes.c_float(lc128.EPS), a["t0"],
                                                   a["rows"], P(self.cos), P(self.sin), P(self.ws), None)

    def regions(self):
        D, H, inner = self.D, self.c["H"], self.c["inner"]
        o, out = 0, {}
        for name, n, dt in (("x2", D, torch.float32), ("x3", D, torch.float32), ("lse", ((4 * H + 63) & ~63) // 4, torch.float32),
                            ("q", D, torch.bfloat16), ("ao", D, torch.bfloat16), ("hf", 2 * inner, torch.bfloat16)):
            nb = n * (4 if dt == torch.float32 else 2)
            out[name] = self.ws[o:o + nb].view(dt)
            o += nb
        assert o == self.ws_bytes
        return out

    def fences_clean(self, what):
        assert (self.wsbuf[:FENCE] == 0xFF).all() and (self.wsbuf[FENCE + self.ws_bytes:] == 0xFF).all(), (what, "write outside the workspace")
        _clean(self.xbuf, self.x, what + " x")
        _clean(self.obuf, self.out, what + " out")
        for L in self.layers:
            _clean(L.cache_buf, L.cache, what + " cache")


def stages(s, L, x, out):
    """the five stages of test_decode_gpu.stages at head dim 128, each from the kernel's own inputs"""
    c, D = s.c, s.D
    H, Hkv, t0 = c["H"], c["Hkv"], c["t0"]
    ws = {k: v.clone() for k, v in s.regions().items()}
    res = []
    xh = kr.decode_rms_prologue(x.double(), L.input_norm.double(), lc128.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 1")
    ref, tol = td.gemv_ref(L.wqkv, xr, D, bf16_out=True, amb_ulp=au)
    res.append(("q | k | v", torch.cat([ws["q"], L.cache[t0]]), ref, tol))
    kvw = Hkv * HD
    cache = L.cache.double()
    ao, lse, p, qh, kh = kr.attention_ref(ws["q"].double()[None, None, :], cache[None, :t0 + 1, :kvw], cache[None, :t0 + 1, kvw:], H, Hkv, HD,
                                          rot=HD, cos=s.cos.double(), sin=s.sin.double(), causal=True, round_points=True)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, cache[None, :t0 + 1, kvw:], ao, lse, H, Hkv, HD)
    res.append(("ao", ws["ao"], ao.reshape(-1), ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1)))
    res.append(("lse", ws["lse"][:H], lse.reshape(-1), ALLOW["lse/decode"] * U * u_lse.reshape(-1)))
    ref, tol = td.gemv_ref(L.wo, ws["ao"].double(), D, res=x.double())
    res.append(("x2", ws["x2"], ref, tol))
    xh = kr.decode_rms_prologue(ws["x2"].double(), L.post_norm.double(), lc128.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 4")
    ref, tol = td.gemv_ref(L.wug, xr, D, bf16_out=True, amb_ulp=au)
    res.append(("hf", ws["hf"], ref, tol))
    hf = ws["hf"].double()
    ar, au = td.prologue(kr.decode_swiglu_prologue(hf), dc.swiglu_window(hf), "stage 5")
    ref, tol = td.gemv_ref(L.wdown, ar, c["inner"], res=ws["x2"].double(), amb_ulp=au)
    res.append(("out", out, ref, tol))
    return res


@pytest.mark.parametrize("name", list(lc128.STEP_CASES))
def test_decode_step_at_head_dim_128_stage_by_stage(kl, name):
    ops, lib = kl
    c = lc128.STEP_CASES[name]
    s = Setup(lib, c)
    L = s.layers[0]
    rc = s.step()
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, lib.kalle_last_error())
    assert ops.attn_last_plan() == lc128.decode128(), hex(ops.attn_last_plan())
    assert ac.step_word(lib, HD, c["H"], c["Hkv"], c["t0"]) == ops.attn_last_plan()
    PLANS_SEEN.add(ops.attn_last_plan())
    assert torch.isfinite(s.out).all(), (name, "NaN rows above t0 leaked into the output")
    for stage, got, ref, tol in stages(s, L, s.x, s.out):
        check(got, ref, tol, f"{name} {stage}")
        SEEN.add(stage)
    keep = torch.arange(c["rows"], device="cuda") != c["t0"]
    _exact(L.cache[keep], L.cache_before[keep], name + " cache rows other than t0")
    s.fences_clean(name)
    r = s.regions()
    assert torch.isnan(r["x3"]).all() and torch.isnan(r["lse"][c["H"]:]).all(), (name, "x3 / lse padding written by a one-layer call")
    SEEN.update({name, "gqa%d" % (c["H"] // c["Hkv"])})


def test_three_layers_in_one_call_equal_three_chained_calls_at_head_dim_128(kl):
    ops, lib = kl
    c = dict(lc128.STEP_CASES["gqa4"], seed=377)
    a, b = Setup(lib, c, 3), Setup(lib, c, 3)
    assert a.step() == 0
    torch.cuda.synchronize()
    x = b.x
    for i in range(3):
        assert b.step(n_layers=1, x=x, layer0=i) == 0
        torch.cuda.synchronize()
        x = b.out.clone()
    _exact(a.out, b.out, "out")
    assert torch.isfinite(a.out).all()
    for i, (la, lb) in enumerate(zip(a.layers, b.layers)):
        _exact(la.cache, lb.cache, f"cache of layer {i}")
        assert torch.isfinite(la.cache[c["t0"]]).all()
    x_last = a.regions()["x3"].clone()
    for stage, got, ref, tol in stages(a, a.layers[2], x_last, a.out):
        check(got, ref, tol, f"three layers, last layer {stage}")
    a.fences_clean("three layers")
    SEEN.add("three-layers")


def test_rejected_decode_steps_leave_everything_untouched(kl):
    ops, lib = kl
    s = Setup(lib, lc128.STEP_CASES["gqa4"])
    for over in (dict(hd=96), dict(hd=32), dict(H=257, Hkv=1), dict(t0=s.c["rows"]), dict(t0=-1), dict(Hkv=3), dict(inner=12)):
        assert s.step(**over) == ERR_ARG, over
        assert ops.attn_last_plan() == 0, over
    assert lib.kalle_llama_decode_ws_bytes_hd(4, 1, 16, 96) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(s.out).all() and (s.wsbuf == 0xFF).all()
    _exact(s.layers[0].cache, s.layers[0].cache_before, "cache after rejected calls")
    assert ops.attn_last_plan() == 0


# ================================================================================================ 8: old entry points = new at 64
@pytest.mark.parametrize("name", ["base", "gqa4"])
def test_old_decode_step_equals_the_hd_form_at_64(kl, name):
    ops, lib = kl
    c = dc.CASES[name]
    a, b = td.Setup(lib, c), td.Setup(lib, c)
    assert lib.kalle_llama_decode_ws_bytes(c["H"], c["Hkv"], c["inner"]) == lib.kalle_llama_decode_ws_bytes_hd(c["H"], c["Hkv"], c["inner"], 64)
    assert a.step() == 0
    rc = lib.kalle_llama_decode_step_hd(ctypes.c_void_p(ctypes.addressof(b.arr)), 1, P(b.x), P(b.out), c["H"], c["Hkv"], c["inner"], 64,
                                        ctypes.c_float(dc.EPS), c["t0"], c["rows"], P(b.cos), P(b.sin), P(b.ws), None)
    assert rc == 0 and ops.attn_last_plan() == td.DECODE_PLAN
    assert ac.step_word(lib, 64, c["H"], c["Hkv"], c["t0"]) == ops.attn_last_plan()
    PLANS_SEEN.add(ops.attn_last_plan())
    torch.cuda.synchronize()
    assert torch.isfinite(a.out).all()
    _exact(a.out, b.out, "out")
    _exact(a.layers[0].cache, b.layers[0].cache, "cache")
    assert torch.equal(a.wsbuf, b.wsbuf), "workspace bytes"


# ================================================================================================ 9: modules
def rel(a, b):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


class _Tok:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _llasa(dev, tmp_path):
    from kalle_audio_amd.model_sigmaVAE import Llasa
    lc = lc128.llasa_config()
    d = tmp_path / "llama_hd128"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": lc["latent_dim"], "audio_proj_dim": 256}, _Tok(lc["tokenizer_len"]),
              use_flash_attention=False)
    inv = json.load(open(os.path.join(G, "state_dict_keys_llama_hd128.json")))["llasa"]
    shapes = [(k, tuple(v)) for k, v in inv.items() if k != "base_model.lm_head.weight"]
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(shapes, lc128.SEED).items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to(dev), lc


def _batch(lc, dev):
    b = {k: torch.from_numpy(v).to(dev) for k, v in gu.llasa_batch(lc, lc128.SEED, B=3, L=40).items()}
    eps = torch.from_numpy(gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), lc128.SEED)).to(dev)
    args = (b["input_ids"], b["audio_latents"], b["audio_distribution_l"], b["ids_mask"], b["audio_mask"], b["target_mask"], b["end_mask"])
    return b, eps, args


def test_llasa_hd128_forward_backward_vs_reference_fixture(dev, tmp_path):
    from test_modules_gpu import _hf_grads
    m, lc = _llasa(dev, tmp_path)
    f = np.load(os.path.join(G, "llasa_hd128.npz"))
    b, eps, args = _batch(lc, dev)
    out = m(*args, noise=eps)
    assert rel(out["ground_truth_audio_latents"], f["sampled"]) < 1e-6
    assert ops_plan() == lc128.T128, hex(ops_plan())        # (the backward runs on autograd's thread: the plan word is per thread)
    print("audio_loss", out["audio_loss"].item(), float(f["audio_loss"]), "end_loss", out["end_loss"].item(), float(f["end_loss"]))
    assert abs(out["audio_loss"].item() - float(f["audio_loss"])) < 1e-2 * float(f["audio_loss"])
    assert abs(out["end_loss"].item() - float(f["end_loss"])) < 1e-2 * float(f["end_loss"])
    valid = ((b["ids_mask"] + b["audio_mask"]) > 0).cpu()
    r = rel(out["pre_mean"].cpu()[valid], torch.from_numpy(f["pre_mean"])[valid])
    print("pre_mean rel-L2", r)
    assert r < 1e-2
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = _hf_grads(m)
    n = full = 0
    for k in f.files:
        if k.startswith("digest/"):
            ref = f[k]
            got = gu.digest(g[k[7:]].detach().float().cpu().numpy())
            assert abs(got[0] - ref[0]) <= 2e-2 * ref[0] + 1e-7, (k, got[0], ref[0])
            n += 1
        if k.startswith("grad/"):
            r = rel(g[k[5:]], f[k].astype(np.float64) / float(f["gradscale/" + k[5:]]))
            print(k, "rel-L2", r)
            assert r < 2e-2, (k, r)
            full += 1
    assert n == 26 and full == 4, (n, full)


def ops_plan():
    from kalle_audio_amd import ops
    return ops.attn_last_plan()


def test_llasa_hd128_through_trainer_matches_autograd(dev, tmp_path):
    from kalle_audio_amd.engine import DataParallelTrainer
    m, lc = _llasa(dev, tmp_path)
    b, eps, args = _batch(lc, dev)
    out = m(*args, noise=eps)
    (out["audio_loss"] + 0.5 * out["end_loss"]).backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    tr = DataParallelTrainer(m, lr=1e-3, optimizer="AdamW", weight_decay=0.0)
    tr.lr = 0.0                                                         # gradients only
    out = m(*args, noise=eps)
    tr.backward(out["audio_loss"] + 0.5 * out["end_loss"])
    for n, p in m.named_parameters():
        assert rel(tr.flat.grad_view(n), want[n]) < 1e-5, n


def test_llasa_hd128_kv_cache_matches_full_forward(dev, tmp_path):
    from kalle_audio_amd import llama_ops as LO
    from test_modules_gpu import ops_axpby
    m, lc = _llasa(dev, tmp_path)
    model = m.base_model.model
    torch.manual_seed(3)
    x = torch.randn(1, 37, 256, device=dev)
    with torch.no_grad():
        full = model(inputs_embeds=x)[0]
        cache = model.init_cache(64, dev)
        assert cache["kv"][0].shape == (64, 2 * 1 * 128)
        got = [model.forward_cached(x[:, :20].contiguous(), cache)]
        for t in range(20, 37):
            got.append(model.forward_cached(x[:, t:t + 1].contiguous(), cache))
            assert ops_plan() == lc128.decode128(), hex(ops_plan())
        got = torch.cat(got, 1)
    assert cache["len"] == 37
    print("prefill + steps vs full", rel(got, full))
    assert rel(got, full) < 1e-2, rel(got, full)
    with torch.no_grad():
        c1, c2 = model.init_cache(64, dev), model.init_cache(64, dev)
        model.forward_cached(x[:, :20].contiguous(), c1)
        model.forward_cached(x[:, :20].contiguous(), c2)
        a = model.forward_cached(x[:, 20:21].contiguous(), c1)
        assert "plan" in c1 and c1["plan"]["head_dim"] == 128
        xx = x[0, 20:21].float().contiguous()
        for layer, kv in zip(model.layers, c2["kv"]):
            xx = LO.layer_fwd_cached(LO.layer_params(layer), xx, kv, 20, c2["rope"])
        bb = model.norm(xx.view(1, 1, -1))
    print("decode step vs layer_fwd_cached", rel(a, bb))
    assert rel(a, bb) < 5e-3, rel(a, bb)
    for k1, k2 in zip(c1["kv"], c2["kv"]):
        assert rel(k1[20], k2[20]) < 1e-2 and torch.equal(k1[21:], k2[21:])
    ids = torch.randint(0, 300, (9,), device=dev)
    prompt = torch.randn(1, 5, lc["latent_dim"], device=dev)
    noise = torch.randn(12, 1, 1, lc["latent_dim"], device=dev)
    outs = []
    for use_cache in (True, False):
        it = iter(noise)
        m.sample = lambda mean, dist_type='fix', noise=None, it=it: ops_axpby(mean, next(it))
        outs.append(m.infer(ids, prompt, end_disp_kl_thres=-1.0, max_length=8, use_cache=use_cache))
    assert outs[0].shape == outs[1].shape == (1, lc["latent_dim"], 7)
    print("infer cache vs none", rel(outs[0], outs[1]))
    assert rel(outs[0], outs[1]) < 2e-2, rel(outs[0], outs[1])


# ================================================================================================ 10: coverage, allowances
def test_every_plan_and_edge_was_seen():
    """whole file, one process, in order"""
    want = {lc128.T128, lc128.TP128, lc128.decode128()} | {lc128.decode64(r) for r in (0, 32, 64)}
    print("attention plan words seen:", " ".join(hex(p) for p in sorted(PLANS_SEEN)))
    assert PLANS_SEEN == want, ([hex(p) for p in sorted(want - PLANS_SEEN)], [hex(p) for p in sorted(PLANS_SEEN - want)])
    edges = {"Nk=%d" % n for n in (1, 7, 8, 31, 32, 33, 255, 256, 257, 1025, lc128.KB128 - 1, lc128.KB128, lc128.KB128 + 1,
                                   lc128.PV_GROUPS128 - 1, lc128.PV_GROUPS128, lc128.PV_GROUPS128 + 1)}
    edges |= {"q | k | v", "ao", "lse", "x2", "hf", "out", "gqa1", "gqa2", "gqa3", "gqa4", "gqa256", "three-layers"} | set(lc128.STEP_CASES)
    assert edges <= SEEN, sorted(edges - SEEN)


def test_measured_allowances():
    """prints the measured worst cases (in units) of this file's cases and holds each to test_attention_gpu's allowance"""
    keys = ("out/tiled", "lse/tiled", "out/decode", "lse/decode", "dq/two_pass", "dk/two_pass", "dv/two_pass")
    for k in keys:
        assert k in MEASURED, (k, "not measured")
        print(f"MEASURED {k}: {MEASURED[k]:.3f} (allowed {ALLOW[k]})")
        assert MEASURED[k] <= ALLOW[k], (k, MEASURED[k], ALLOW[k])
