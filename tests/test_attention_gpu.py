"""-m gpu: the attention kernels of include/kalle_hip.h (csrc/attention.hip), element by element against the fp64 references
of tests/kernel_refs.py (which tests/test_attention_refs_cpu.py checks against torch's SDPA and float64 autograd on the CPU).

Conventions: those of test_conv_gpu.py - calls through ctypes, every element bounded by its own tolerance and the first
offender reported (tests/gpu_checks.py), every case names the plan word (kalle_attn_last_plan, encoding in the header) it
expects for the forward and for the backward; a case whose plan does not come out is a wrong case.

Operands: bf16 q / k / v / dout at 0.8 N(0, 1) inside NaN: the rows behind the last batch element and the columns before,
between and behind the head windows of every operand allocation are NaN (masked keys stay finite: the kernels read them).
"Hot keys": for the key indices where the kernels change path (0, 15, 16, 127, 128, Nk - 1: the first and last key of the folded
tail among them) one query row per (batch, head) points along that key (reference p >= 0.2, asserted) and the key's v row has
magnitude 2.5, so that a dropped, doubled or misplaced edge key moves an output by far more than a unit.  out, lse, delta, dq,
dk, dv live in Guard / guarded buffers with a leading dimension wider than the heads and a non-zero column offset; every call
is followed by .clean().  The backward is fed the reference's own out (rounded to bf16) and lse (fp32), so that its bound
does not inherit the forward's error.

Bounds: tol = ALLOW[key] x unit, the unit per element in float64 from the round_points=True reference alone:
  out   2^-9 (sum_j p_ij |v_jd| + |ref|)                       probability rounding (bf16 operand of P V) and the bf16 store
  lse   2^-24 (1 + |ref| + sum_d |q~_id| max_j |k~_jd| dh^-0.5) fp32 score sums, exp / log
  dv    2^-9 (sum_i p_ij |dout_id| + |ref|)                     P as a bf16 operand, bf16 store
  dq    2^-9 (sum_j |dS_ij| |k~_jd| + |ref|), dk likewise over i and the sharing heads, |dS_ij| = p_ij (|dP_ij| + sum_j' p_ij'
        |dP_ij'|) dh^-0.5, then through the un-rotation as the sum of the two partners' bounds   dS as a bf16 operand, bf16 store
  delta (dh + 2) 2^-24 sum_d |dout_id out_id|                   an fp32 sum of exact products (not measured: derived)
ALLOW is MEASURED: the worst deviation over the whole case list in those units on one MI355X, times 4 (other seeds), rounded up.
tests/test_attention_refs_cpu.py asserts from the references alone that every wrong reference of WRONG below moves some
element of its case by more than twice unit x ALLOW."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as kr  # noqa: E402
from gpu_checks import NAN, U, Guard, check, clean as _clean, guarded as _guarded  # noqa: E402


def asked(lib, entry, call_args):
    """the word the host query of `entry` names for a call about to be made with `call_args` (those in front of `stream`): every
    case asserts that it is the word kalle_attn_last_plan() holds after the call (attn_cases imports this file: imported here)"""
    import attn_cases as ac
    rc, out = ac.query(lib, entry, call_args)
    assert rc == 0, (entry, rc)
    return out[0]

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B = 2
# measured on one MI355X (ROCm 7, -O3 -ffast-math), 2026-10-17, over the case lists of this file at seeds 1, 2, 3, in units of the
# docstring's per-element magnitudes (2^-9 ... for the bf16 outputs, 2^-24 ... for lse), then x 4 and rounded up to an integer
ALLOW = {
    "out/tiled": 7.0,        # measured 1.553
    "lse/tiled": 170.0,      # measured 42.495
    "out/decode": 5.0,       # measured 1.202
    "lse/decode": 4.0,       # measured 0.849
    "dq/two_pass": 4.0,      # measured 0.773
    "dk/two_pass": 4.0,      # measured 0.990
    "dv/two_pass": 5.0,      # measured 1.195
    "dq/fused": 3.0,         # measured 0.683
    "dk/fused": 3.0,         # measured 0.685
    "dv/fused": 4.0,         # measured 0.909
    "dq/fused_gqa": 4.0,     # measured 0.785
    "dk/fused_gqa": 2.0,     # measured 0.449
    "dv/fused_gqa": 4.0,     # measured 0.883
}
MEASURED = {}
PLANS_SEEN = set()
BF = 2.0 ** -9 / U          # gpu_checks.check measures in units of U x unit: a 2^-9 unit is BF of them


# ------------------------------------------------------------------------------------------------ plan words (header)
def tiled(dh=64, fold=False):
    return 1 | dh << 8 | int(fold) << 16


def decode(rot):
    return 2 | 64 << 8 | rot << 17


def two_pass(dh=64):
    return 3 | 16 | dh << 8


FUSED, FUSED_GQA = 4 | 16 | 64 << 8, 5 | 16 | 64 << 8
FAMILY = {1: "tiled", 2: "decode", 3: "two_pass", 4: "fused", 5: "fused_gqa"}

DEFAULT = dict(dh=64, H=2, Hkv=2, rot=0, causal=False, mask="none", layout="split", bwd=None, seed=1)


def A(Nq, Nk, fwd, bwd=None, **kw):
    c = dict(DEFAULT)
    c.update(kw)
    c.update(Nq=Nq, Nk=Nk, fwd=fwd, bwd=bwd)
    assert c["layout"] == "split" or Nq == Nk
    return c


def _id(c):
    return "-".join(f"{k}{c[k]}" for k in ("dh", "Nq", "Nk", "H", "Hkv", "rot", "causal", "mask", "layout") if k in ("Nq", "Nk") or c[k] != DEFAULT[k])


# ------------------------------------------------------------------------------------------------ inputs (CPU, seeded)
def rope_tables(npos, rot):
    """[npos][rot / 2] fp32 cos / sin (transformer.py:89-138: inv_freq over the rotated dims)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2).double() / rot))
    f = torch.arange(npos).double()[:, None] * inv[None, :]
    return f.cos().float(), f.sin().float()


def edge_keys(Nk):
    return sorted({j for j in (0, 15, 16, 127, 128, Nk - 1) if j < Nk})


def make_mask(c, g):
    Nk, kind = c["Nk"], c["mask"]
    if kind == "none":
        return None
    m = torch.ones((B, Nk), dtype=torch.bool)
    if kind == "random":
        m = torch.rand((B, Nk), generator=g) > 0.3
        m[:, 0] = True                       # (a causal query always keeps a live key)
        m[0, Nk - 1] = True
        m[1, Nk - 1] = Nk == 1
    elif kind == "first":                    # only the first key masked
        m[:, 0] = Nk == 1
    elif kind == "last_only":                # only the last key live
        m[:] = False
        m[:, Nk - 1] = True
    elif kind == "row":                      # batch element 1 fully masked, element 0 random
        m[0] = torch.rand((Nk,), generator=g) > 0.3
        m[0, 0] = True
        m[1] = False
    return m


def make_inputs(c, seed=None):
    """bf16-exact float64 operands of a case: q [B][Nq][H dh], k, v [B][Nk][Hkv dh], dout, the tables, the mask, and
    `hot`: the (b, h, row, key) whose probability the hot-key construction promises to be >= 0.2"""
    g = torch.Generator().manual_seed(1000 * (c["seed"] if seed is None else seed) + 7)
    dh, H, Hkv, Nq, Nk, rot, causal = (c[k] for k in ("dh", "H", "Hkv", "Nq", "Nk", "rot", "causal"))
    rn = lambda *s: kr.bf16r(0.8 * torch.randn(*s, generator=g))  # noqa: E731
    q, k, v, dout = rn(B, Nq, H * dh), rn(B, Nk, Hkv * dh), rn(B, Nk, Hkv * dh), rn(B, Nq, H * dh)
    cos, sin = rope_tables(max(Nq, Nk) + 1, rot) if rot else (None, None)
    mask = make_mask(c, g)
    E = edge_keys(Nk)
    off = Nk - Nq if causal else 0
    group = H // Hkv
    hot = []
    qh = q.view(B, Nq, H, dh)
    nslots = min(len(E), Nq)
    stride = max(Nq // nslots, 1)
    for b in range(B):
        for h in range(H):
            taken = set()
            for t in range(nslots):
                j = E[(t + b * H + h) % len(E)]
                r = min(max(j - off, 0), Nq - 1) if causal else (t * stride + b + h) % Nq
                if r in taken or (causal and j > r + off) or (mask is not None and not mask[b, j]):
                    continue
                taken.add(r)
                kj = k.view(B, Nk, Hkv, dh)[b, j, h // group]
                kt = kr._rotate(kj[None], cos.double() if rot else None, sin.double() if rot else None, rot, torch.tensor([j]))
                qt = kr._unrotate(2.5 * kt, cos.double() if rot else None, sin.double() if rot else None, rot, torch.tensor([r + off]))
                qh[b, r, h] = kr.bf16r(qt[0])
                hot.append((b, h, r, j))
    for j in E:
        vj = v[:, j]
        v[:, j] = torch.where(vj >= 0, 2.5, -2.5)
    return dict(q=q, k=k, v=v, dout=dout, cos=cos, sin=sin, mask=mask, hot=hot)


def wrong_kw(name, c):
    """the reference arguments of a deliberately wrong variant (kernel_refs `wrong`)"""
    if name == "last_key_dropped":
        return ("drop_key", c["Nk"] - 1)
    if name == "first_tail_key_dropped":
        return ("drop_key", 128)
    return name


# ------------------------------------------------------------------------------------------------ one case
@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def _chk(out, ref, key, unit, what):
    assert ALLOW[key] is not None, (key, "no allowance")
    return check(out, ref, ALLOW[key] * U * unit, what, key, unit, MEASURED)


class Operand:
    """a [B][N][cols] bf16 operand at column `col0` of a [B N + 2][ld] allocation that is NaN everywhere else"""

    def __init__(self, t, ld, col0):
        Bn, N, cols = t.shape
        self.buf = torch.full((Bn * N + 2, ld), NAN, device="cuda", dtype=torch.bfloat16)
        self.buf[:Bn * N, col0:col0 + cols] = t.reshape(Bn * N, cols).to(torch.bfloat16)
        self.col0 = col0


def layout(c):
    """(ldq, q_off, ldk, k_off, ldv, v_off): `fused` one q | k | v row (Nq == Nk), `split` q and k | v rows; 8 spare columns
    before, between and behind the windows"""
    dh, H, Hkv = c["dh"], c["H"], c["Hkv"]
    wq, wk = H * dh, Hkv * dh
    if c["layout"] == "fused":
        ld = wq + 2 * wk + 32
        return ld, 8, ld, 16 + wq, ld, 24 + wq + wk
    return wq + 16, 8, 2 * wk + 24, 8, 2 * wk + 24, 16 + wk


def run_case(kl, c, seed=None, wrong=None, inputs=None):
    """forward (and backward when the case names a backward plan) through the C ABI: plan words, per-element bounds, guards.
    Returns the forward's out / lse windows (float64) and their references and tolerances."""
    ops, lib = kl
    P, st = ops._p, ops._stream()
    dh, H, Hkv, Nq, Nk, rot, causal = (c[k] for k in ("dh", "H", "Hkv", "Nq", "Nk", "rot", "causal"))
    what = _id(c)
    x = inputs or make_inputs(c, seed)
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    q, k, v, dout, mask = cu(x["q"]), cu(x["k"]), cu(x["v"]), cu(x["dout"]), cu(x["mask"])
    cos, sin = cu(x["cos"]), cu(x["sin"])
    cosd, sind = (cos.double(), sin.double()) if rot else (None, None)
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    ldq, q_off, ldk, k_off, ldv, v_off = layout(c)
    if c["layout"] == "fused":
        qkv = Operand(torch.cat([q, torch.full((B, Nq, 8), NAN, device="cuda", dtype=torch.float64), k,
                                 torch.full((B, Nq, 8), NAN, device="cuda", dtype=torch.float64), v], -1), ldq, q_off)
        qb = kb = vb = qkv.buf
    else:
        qb = Operand(q, ldq, q_off).buf
        kb = vb = Operand(torch.cat([k, torch.full((B, Nk, 8), NAN, device="cuda", dtype=torch.float64), v], -1), ldk, k_off).buf
    ldo = H * dh + 16
    fill = -1.0e30 * dh ** -0.5           # the header: lse of a fully masked row from the tiled kernels
    fam_f = FAMILY[c["fwd"] & 15]
    fw = wrong if wrong not in ("dk_missing_head", "dq_not_unrotated", "delta_dout_squared") else None
    args = (H, Hkv, dh, rot, cosd, sind, mask, causal)
    ref, rlse, p, qh, kh = kr.attention_ref(q, k, v, *args, round_points=True, mask_fill=fill, wrong=wrong_kw(fw, c) if fw else None)
    if wrong is None:
        for (b, h, r, j) in x["hot"]:
            assert p[b, h, r, j] >= 0.2, (what, "hot key", b, h, r, j, float(p[b, h, r, j]))
    res = None
    og = Guard(B * Nq, H * dh, ldo, torch.bfloat16, col0=8)
    lbuf, lse = _guarded(torch.full((B, H, Nq), NAN, device="cuda"))
    op = og.buf.data_ptr() + 16
    fa = (P(qb), ldq, q_off, P(kb), ldk, k_off, P(vb), ldv, v_off, op, ldo, P(lse), P(cos), P(sin), rot, P(m8), int(causal), B, H, Hkv, Nq, Nk, dh)
    word = asked(lib, "fwd", fa)
    rc = lib.kalle_attention_fwd_hd(*fa, st)
    plan = lib.kalle_attn_last_plan()
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    assert plan == c["fwd"], (what, hex(plan), hex(c["fwd"]))
    assert word == plan, (what, "the query named", hex(word))
    PLANS_SEEN.add(plan)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, v, ref, rlse, H, Hkv, dh)
    out = og.v.reshape(B, Nq, H * dh)
    _chk(out, ref, "out/" + fam_f, BF * u_out, what + " out")
    _chk(lse, rlse, "lse/" + fam_f, u_lse, what + " lse")
    og.clean(what + " out")
    _clean(lbuf, lse, what + " lse")
    res = (out.double(), ref, ALLOW["out/" + fam_f] * 2.0 ** -9 * u_out, lse.double(), rlse, ALLOW["lse/" + fam_f] * U * u_lse)
    if c["bwd"] is None:
        return res
    # ---- backward, fed the reference's out (bf16) and lse (fp32)
    fam_b = FAMILY[c["bwd"] & 15]
    out_b = ref.to(torch.bfloat16) if fw is None else kr.attention_ref(q, k, v, *args, round_points=True, mask_fill=fill)[0].to(torch.bfloat16)
    lse_in = (rlse if fw is None else kr.attention_ref(q, k, v, *args, round_points=True, mask_fill=fill)[1]).float().contiguous()
    oo, do = Operand(out_b, ldo, 8), Operand(dout, ldo, 8)
    dbuf, delta = _guarded(torch.full((B, H, Nq), NAN, device="cuda"))
    dqg = Guard(B * Nq, H * dh, ldq, torch.bfloat16, col0=q_off)
    dkg = Guard(B * Nk, Hkv * dh, ldk, torch.bfloat16, col0=k_off)
    dvg = Guard(B * Nk, Hkv * dh, ldv, torch.bfloat16, col0=v_off)
    ba = (P(qb), ldq, q_off, P(kb), ldk, k_off, P(vb), ldv, v_off, oo.buf.data_ptr() + 16, do.buf.data_ptr() + 16, ldo,
          P(lse_in), P(delta), P(dqg.buf), P(dkg.buf), P(dvg.buf), P(cos), P(sin), rot, P(m8), int(causal), B, H, Hkv, Nq, Nk, dh)
    word = asked(lib, "bwd", ba)
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
    if mask is not None:       # the header's contract, spelled out: a masked key's dk / dv and a fully masked batch row are exact zeros
        dead = ~mask
        for name, t in (("dk", dkg.v.reshape(B, Nk, -1)), ("dv", dvg.v.reshape(B, Nk, -1))):
            assert (t[dead] == 0).all(), (what, name, "of a masked key is not exactly zero")
        full = ~mask.any(1)
        assert (dqg.v.reshape(B, Nq, -1)[full] == 0).all(), (what, "dq of a fully masked batch row is not exactly zero")
    for gd, name in ((dqg, "dq"), (dkg, "dk"), (dvg, "dv")):
        gd.clean(what + " " + name)
    _clean(dbuf, delta, what + " delta")
    return res


# ================================================================================================ forward + backward, head dim 64
# Which family a shape gets is the list of predicates next to attn_fold_tail in csrc/attention.hip; that every case below reaches
# the word it names is known without a GPU: tests/test_attn_plan_cpu.py asks the host queries for every case of this file
# (tests/attn_cases.py) and compares with a table recorded before the predicates existed.
T64, TF, TP = tiled(), tiled(fold=True), two_pass()
CASES_64 = [
    # ---- tiled forward at the edge lengths (backward: whatever the shape dispatches to)
    A(2, 2, T64, TP, rot=32, causal=True, layout="fused"),
    A(15, 15, T64, FUSED, mask="random", layout="fused"),
    A(16, 16, T64, TP, H=4, rot=32),                                     # GQA with rotary: two-pass
    A(17, 17, T64, FUSED_GQA, H=4, Hkv=1, mask="first"),
    A(127, 127, T64, FUSED, rot=64, mask="row", layout="fused"),
    A(128, 128, T64, FUSED, rot=32, mask="random", layout="fused"),
    A(129, 129, TF, TP, layout="fused"),
    A(257, 257, T64, TP, H=4, rot=32, causal=True, layout="fused"),
    A(128, 128, T64, FUSED_GQA, H=4, rot=0, mask="row"),
    # ---- fold_tail on: Nk 129 (above), 144, 145, 160; off: 161, 130 with rot 32, 130 causal
    A(100, 144, TF, FUSED_GQA, H=4, mask="random"),
    A(37, 145, TF, TP),                                                  # tail 17: just past the fused_gqa tail
    A(126, 160, TF, TP, H=4, Hkv=1, mask="row"),
    A(50, 161, T64, TP, mask="random"),
    A(130, 130, T64, TP, rot=32, layout="fused"),
    A(125, 130, T64, TP, causal=True),
    A(130, 130, T64, TP, causal=True, rot=64, mask="random", layout="fused"),
    # ---- causal: Nk = Nq, Nq + 5, Nq + 131
    A(17, 17, T64, TP, causal=True, rot=64),
    A(128, 128, T64, TP, causal=True, H=4, layout="fused"),
    A(129, 129, T64, TP, causal=True, rot=32, layout="fused"),
    A(60, 65, T64, TP, causal=True, rot=64, H=4, Hkv=1),
    A(126, 257, T64, TP, causal=True, rot=32),
    # ---- two-pass: Nq 129, GQA 4:1 with Nq 260 / Nk 200
    A(129, 100, T64, TP, mask="random"),
    A(260, 200, T64, TP, H=4, Hkv=1, rot=32, mask="row"),
    # ---- fused: (Nq, Nk), rot 0 / 32 / 64, mask on and off  (Nq == 1: the forward is the decode kernel)
    A(1, 1, decode(0), FUSED),
    A(1, 1, decode(64), FUSED, rot=64, mask="random"),
    A(16, 16, T64, FUSED, rot=64, layout="fused"),
    A(17, 17, T64, FUSED, rot=32, mask="random"),
    A(127, 127, T64, FUSED, mask="first", layout="fused"),
    A(128, 128, T64, FUSED, rot=64),
    A(37, 128, T64, FUSED, rot=32, mask="row"),
    A(128, 37, T64, FUSED, mask="random"),
    # ---- fused_gqa: 4:2, 4:1, 2:2 with Nq != Nk; Nk in {7, 128, 129, 144}, Nq in {112, 126, 127}; both sides of tail <= 128 - Nq
    A(112, 7, T64, FUSED_GQA, H=4),
    A(126, 128, T64, FUSED_GQA, H=4, Hkv=1, mask="random"),
    A(127, 129, TF, FUSED_GQA, H=4),
    A(112, 144, TF, FUSED_GQA),
    A(112, 129, TF, FUSED_GQA, mask="random"),
    A(126, 130, TF, FUSED_GQA, H=4, Hkv=1),
    A(127, 130, TF, TP, H=4, Hkv=1),                                     # tail 2 > 128 - 127: two-pass
    A(113, 144, TF, TP, H=4),                                            # tail 16 > 128 - 113
    A(127, 128, T64, FUSED_GQA, H=4, mask="row"),
    A(126, 129, TF, FUSED_GQA, H=4, Hkv=1, mask="row"),
]


@pytest.mark.parametrize("c", CASES_64, ids=_id)
def test_attention_dh64(kl, c):
    run_case(kl, c)


# ================================================================================================ head dims 32 and 128
def _hd_cases(dh, rots):
    t, tf, tp = tiled(dh), tiled(dh, True), two_pass(dh)
    r0, r1 = rots
    return [
        A(1, 1, t, tp, dh=dh, rot=r0),
        A(1, 130, tf, tp, dh=dh, mask="random"),
        A(2, 2, t, tp, dh=dh, rot=r1, causal=True, layout="fused"),
        A(15, 15, t, tp, dh=dh, mask="random", layout="fused"),
        A(16, 16, t, tp, dh=dh, rot=r0, H=4),
        A(17, 17, t, tp, dh=dh, rot=r1, H=4, mask="row"),
        A(127, 127, t, tp, dh=dh, rot=r0, causal=True, layout="fused"),
        A(128, 128, t, tp, dh=dh, rot=r1, H=4, mask="first"),
        A(129, 129, tf, tp, dh=dh, H=4, mask="random", layout="fused"),
        A(129, 129, t, tp, dh=dh, rot=r0, causal=True, H=4, layout="fused"),
        A(100, 160, tf, tp, dh=dh, mask="row"),
        A(50, 161, t, tp, dh=dh, H=4, Hkv=1),
        A(257, 257, t, tp, dh=dh, rot=r0, mask="random", layout="fused"),
        A(60, 191, t, tp, dh=dh, rot=r1, causal=True),
    ]


@pytest.mark.parametrize("c", _hd_cases(32, (32, 32)), ids=_id)
def test_attention_dh32(kl, c):
    run_case(kl, c)


@pytest.mark.parametrize("c", _hd_cases(128, (64, 32)), ids=_id)
def test_attention_dh128(kl, c):
    run_case(kl, c)


# ================================================================================================ the single-query kernel
DECODE_CASES = [A(1, Nk, decode(rot), None, rot=rot, causal=causal, H=H, Hkv=Hkv, mask=mask)
                for Nk, rot, causal, (H, Hkv), mask in [
                    (1, 32, True, (2, 2), "none"), (7, 0, False, (4, 1), "random"), (8, 64, True, (4, 1), "none"),
                    (31, 32, False, (2, 2), "last_only"), (32, 0, True, (4, 1), "random"), (33, 64, False, (4, 2), "none"),
                    (255, 32, True, (4, 1), "first"), (256, 64, True, (2, 2), "random"), (257, 0, False, (4, 1), "last_only"),
                    (1025, 64, True, (4, 1), "random"), (1025, 32, False, (2, 2), "none")]]


@pytest.mark.parametrize("c", DECODE_CASES, ids=_id)
def test_attention_decode(kl, c):
    run_case(kl, c)


def test_decode_agrees_with_tiled_per_element(kl):
    """the last query row of a causal 2-query call (tiled kernel; position Nk - 1, sees every key) and the causal single-query
    call on that row alone (decode kernel): each inside its fp64 bound, and the two within the sum of their bounds"""
    c2 = A(2, 33, T64, None, rot=32, causal=True, H=4, Hkv=1, mask="random")
    c1 = dict(c2, Nq=1, fwd=decode(32))
    o2, r2, t2, l2, rl2, tl2 = run_case(kl, c2)
    x = make_inputs(c2)
    x["q"], x["dout"], x["hot"] = x["q"][:, 1:].contiguous(), x["dout"][:, 1:].contiguous(), []
    o1, r1, t1, l1, rl1, tl1 = run_case(kl, c1, inputs=x)
    assert (r1[:, 0] - r2[:, 1]).abs().max() < 1e-12
    check(o1[:, 0], o2[:, 1], t1[:, 0] + t2[:, 1], "decode vs tiled out")
    check(l1[:, :, 0], l2[:, :, 1], tl1[:, :, 0] + tl2[:, :, 1], "decode vs tiled lse")


# ================================================================================================ rejected calls
def test_rejected_calls_write_nothing(kl):
    ops, lib = kl
    P, st = ops._p, ops._stream()
    N, H, dh = 16, 2, 64
    z = torch.zeros((B * N + 2, 3 * H * dh + 32), device="cuda", dtype=torch.bfloat16)
    cos, sin = (t.cuda() for t in rope_tables(N, 32))
    og, dq, dk, dv = (Guard(B * N, H * dh, H * dh + 16, torch.bfloat16) for _ in range(4))
    lse, delta = Guard(B * H, N), Guard(B * H, N)
    base = dict(ldq=z.shape[1], q_off=8, ldk=z.shape[1], k_off=16 + H * dh, ldv=z.shape[1], v_off=24 + 2 * H * dh, ldo=H * dh + 16,
                cos=P(cos), sin=P(sin), rot=32, causal=0, H=H, Hkv=H, Nq=N, Nk=N, dh=dh, dq=P(dq.buf))

    def call(**kw):
        a = dict(base)
        a.update(kw)
        rf = lib.kalle_attention_fwd_hd(P(z), a["ldq"], a["q_off"], P(z), a["ldk"], a["k_off"], P(z), a["ldv"], a["v_off"], P(og.buf), a["ldo"],
                                        P(lse.buf), a["cos"], a["sin"], a["rot"], None, a["causal"], B, a["H"], a["Hkv"], a["Nq"], a["Nk"], a["dh"], st)
        pf = lib.kalle_attn_last_plan()
        rb = lib.kalle_attention_bwd_hd(P(z), a["ldq"], a["q_off"], P(z), a["ldk"], a["k_off"], P(z), a["ldv"], a["v_off"], P(z), P(z), a["ldo"],
                                        P(z), P(delta.buf), a["dq"], P(dk.buf), P(dv.buf), a["cos"], a["sin"], a["rot"], None, a["causal"],
                                        B, a["H"], a["Hkv"], a["Nq"], a["Nk"], a["dh"], st)
        return rf, pf, rb, lib.kalle_attn_last_plan()

    bad = [dict(causal=1, Nk=N - 1), dict(H=3, Hkv=2), dict(ldq=z.shape[1] + 4), dict(ldk=z.shape[1] + 4), dict(ldv=z.shape[1] + 4),
           dict(ldo=H * dh + 12), dict(q_off=4), dict(k_off=20), dict(v_off=12), dict(rot=16), dict(rot=48), dict(rot=64, dh=32),
           dict(cos=None), dict(sin=None), dict(dh=48)]
    for kw in bad:
        rf, pf, rb, pb = call(**kw)
        assert (rf, pf, rb, pb) == (ERR_ARG, 0, ERR_ARG, 0), (kw, rf, hex(pf), rb, hex(pb))
    rf, pf, rb, pb = call(dq=None)                      # NULL dq: the forward has no such argument
    assert (rb, pb) == (ERR_ARG, 0), (rb, hex(pb))
    torch.cuda.synchronize()
    for gd, name in ((dq, "dq"), (dk, "dk"), (dv, "dv"), (delta, "delta")):
        gd.untouched(name)
    og.buf.fill_(NAN)
    lse.buf.fill_(NAN)
    for kw in bad:
        call(**kw)
    torch.cuda.synchronize()
    og.untouched("out")
    lse.untouched("lse")


# ================================================================================================ the bounds bite
WRONG = [
    ("last_key_dropped", A(126, 130, TF, None, H=4, Hkv=1)),
    ("first_tail_key_dropped", A(126, 130, TF, None, H=4, Hkv=1)),
    ("causal_boundary", A(129, 129, T64, None, causal=True, rot=32, layout="fused")),
    ("query_position", A(60, 65, T64, None, causal=True, rot=64, H=4, Hkv=1)),
    ("rotate_half_sign", A(128, 128, T64, None, rot=32, mask="random", layout="fused")),
    ("gqa_modulo", A(16, 16, T64, None, H=4, rot=32)),
    ("mask_other_batch", A(15, 15, T64, None, mask="random", layout="fused")),
    ("scale_eighth", A(17, 17, tiled(32), None, dh=32, rot=32, H=4)),
    ("dk_missing_head", A(126, 128, T64, FUSED_GQA, H=4, Hkv=1, mask="random")),
    ("dq_not_unrotated", A(17, 17, T64, FUSED, rot=32, mask="random")),
    ("delta_dout_squared", A(129, 100, T64, TP, mask="random")),
]


@pytest.mark.parametrize("wrong,c", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_references_are_caught(kl, wrong, c):
    """the same case passes against the right reference and `check` raises against the deliberately wrong one"""
    run_case(kl, c)
    saved = dict(MEASURED)                  # (a deviation from a wrong reference is no measurement of the kernel)
    try:
        with pytest.raises(AssertionError, match="out of bound"):
            run_case(kl, c, wrong=wrong)
    finally:
        MEASURED.clear()
        MEASURED.update(saved)


# ================================================================================================ coverage and allowances
def test_every_family_and_head_dim_was_seen(kl):
    """every kernel family x head dim the dispatch can reach came out of some case, the tiled forward with the folded tail on and
    off, the decode kernel at each ROT.  Reads PLANS_SEEN, which the case lists above fill: whole file, one process, in order"""
    want = {tiled(d, f) for d in (32, 64, 128) for f in (False, True)} | {decode(r) for r in (0, 32, 64)} | \
           {two_pass(d) for d in (32, 64, 128)} | {FUSED, FUSED_GQA}
    print("attention plan words seen:", " ".join(hex(p) for p in sorted(PLANS_SEEN)))
    assert want <= PLANS_SEEN, [hex(p) for p in sorted(want - PLANS_SEEN)]
    assert PLANS_SEEN <= want, [hex(p) for p in sorted(PLANS_SEEN - want)]


def test_measured_allowances(kl):
    """prints the measured worst cases (in units) and holds each to its allowance; whole file, one process, in order"""
    for k in sorted(ALLOW):
        assert k in MEASURED, (k, "not measured")
        print(f"MEASURED {k}: {MEASURED[k]:.3f} (allowed {ALLOW[k]})")
        assert MEASURED[k] <= ALLOW[k], (k, MEASURED[k], ALLOW[k])
