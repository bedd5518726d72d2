"""The case list, inputs, fp64 references and deliberately wrong references of the varlen attention tests
(tests/test_attn_varlen_gpu.py on the device; tests/test_attn_varlen_cpu.py shows without one that every wrong reference moves
some element by more than twice its allowance).  Nothing here touches a device.

A case packs `lens` sequences into buffers of `total` rows at `row0`.  Every sequence's operands are those of
test_attention_gpu.make_inputs for the dense causal call on it alone (its batch element 0: bf16-exact 0.8 N(0, 1), hot keys at
the tile edges); rows outside every sequence hold finite filler here (the row0-off-by-one reference reads them) and NaN on the
device.  Units and allowances: DESIGN 2 / test_attention_gpu (`out/tiled`, `lse/tiled`, `dq|dk|dv/two_pass`, imported)."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as kr  # noqa: E402
import test_attention_gpu as ta  # noqa: E402
from gpu_checks import U  # noqa: E402

ALLOW = ta.ALLOW
BF = 2.0 ** -9


def V(dh, H, Hkv, rot, lens, row0=None, total=None, seed=1):
    row0 = list(row0) if row0 is not None else [sum(lens[:b]) for b in range(len(lens))]
    return dict(dh=dh, H=H, Hkv=Hkv, rot=rot, lens=list(lens), row0=row0, total=total or row0[-1] + lens[-1], seed=seed)


CASES = [
    V(64, 4, 2, 64, [1, 2, 127, 128, 129]),                 # back to back: starts 0, 1, 3, 130, 258
    V(64, 2, 1, 64, [257, 5, 256, 130]),
    V(128, 2, 1, 128, [129, 1, 128, 3]),
    V(64, 2, 2, 0, [130, 7]),
    V(64, 4, 2, 64, [300]),
    V(64, 4, 2, 64, [129, 257, 1], row0=[8, 200, 464], total=472),
]
WRONG = ("rotary_packed_row", "sees_previous_key", "row0_off_by_one", "lse_max_len_stride")
# the case each wrong reference is shown on (rotary needs rot != 0 and a sequence that does not start at row 0; the previous key a
# second sequence; the lse stride H > 1 and a sequence shorter than max_len)
WRONG_CASE = {"rotary_packed_row": 0, "sees_previous_key": 1, "row0_off_by_one": 5, "lse_max_len_stride": 0}


def case_id(c):
    return f"dh{c['dh']}-H{c['H']}.{c['Hkv']}-rot{c['rot']}-" + ".".join(str(n) for n in c["lens"]) + ("-gaps" if c["total"] != sum(c["lens"]) else "")


def fwd_word(c):
    return 8 | c["dh"] << 8


def bwd_word(c):
    return 9 | 16 | c["dh"] << 8


def dense_case(c, n):
    return ta.A(n, n, ta.tiled(c["dh"]), ta.two_pass(c["dh"]), dh=c["dh"], H=c["H"], Hkv=c["Hkv"], rot=c["rot"], causal=True)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    c = CASES[i]
    dh, H, Hkv, rot, total = c["dh"], c["H"], c["Hkv"], c["rot"], c["total"]
    g = torch.Generator().manual_seed(4242 + i)
    fill = lambda w: kr.bf16r(0.8 * torch.randn(total + 1, w, generator=g))  # noqa: E731   (one row behind the last: row0 + 1)
    x = dict(q=fill(H * dh), k=fill(Hkv * dh), v=fill(Hkv * dh), dout=fill(H * dh), hot=[])
    for b, (r0, n) in enumerate(zip(c["row0"], c["lens"])):
        d = ta.make_inputs(dense_case(c, n), seed=10 * c["seed"] + b)
        for name in ("q", "k", "v", "dout"):
            x[name][r0:r0 + n] = d[name][0]
        x["hot"] += [(b, h, r, j) for (bb, h, r, j) in d["hot"] if bb == 0]
    x["cos"], x["sin"] = ta.rope_tables(total + 2, rot) if rot else (None, None)
    live = torch.zeros(total, dtype=torch.bool)
    for r0, n in zip(c["row0"], c["lens"]):
        live[r0:r0 + n] = True
    x["live"] = live
    return x


def inputs(i):
    """packed float64 operands [total + 1][H dh | Hkv dh] of case i (shared, do not modify), tables [total + 2][rot / 2], `live`
    [total] and the hot (sequence, head, row, key) list"""
    return _inputs(i)


def _seq_ref(c, x, b, wrong=None):
    """the dense causal references of sequence b alone (float64): dict(out, lse, dq, dk, dv, delta, u_out, u_lse, mags, p)"""
    dh, H, Hkv, rot = c["dh"], c["H"], c["Hkv"], c["rot"]
    r0, n = c["row0"][b], c["lens"][b]
    if wrong == "row0_off_by_one":
        r0 += 1
    cos, sin = (x["cos"].double(), x["sin"].double()) if rot else (None, None)
    if wrong == "rotary_packed_row" and rot:
        cos, sin = cos[r0:], sin[r0:]
    q, k, v, dout = (x[t][r0:r0 + n][None] for t in ("q", "k", "v", "dout"))
    extra = wrong == "sees_previous_key" and b > 0
    if extra:                                       # the row in front of the sequence as a key every query sees
        pr = c["row0"][b - 1] + c["lens"][b - 1] - 1
        k, v = torch.cat([x["k"][pr:pr + 1][None], k], 1), torch.cat([x["v"][pr:pr + 1][None], v], 1)
    args = (H, Hkv, dh, rot, cos, sin, None, True)
    out, lse, p, qh, kh = kr.attention_ref(q, k, v, *args, round_points=True)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, v, out, lse, H, Hkv, dh)
    ob = kr.bf16r(out)
    dq, dk, dv, delta, mags = kr.attention_bwd_ref(q, k, v, dout, *args, round_points=True, out=ob)
    if extra:
        dk, dv, mags["dk"], mags["dv"] = dk[:, 1:], dv[:, 1:], mags["dk"][:, 1:], mags["dv"][:, 1:]
    return dict(out=out[0], lse=lse[0], dq=dq[0], dk=dk[0], dv=dv[0], delta=delta[0], u_out=u_out[0], u_lse=u_lse[0],
                mags={t: m[0] for t, m in mags.items()}, p=p[0])


@functools.lru_cache(maxsize=None)
def refs(i):
    """the right references of every sequence of case i (computed once, shared, do not modify)"""
    c, x = CASES[i], inputs(i)
    r = [_seq_ref(c, x, b) for b in range(len(c["lens"]))]
    for (b, h, row, j) in x["hot"]:
        assert r[b]["p"][h, row, j] >= 0.2, (case_id(c), "hot key", b, h, row, j, float(r[b]["p"][h, row, j]))
    return r


def wrong_refs(i, wrong):
    c, x = CASES[i], inputs(i)
    return [_seq_ref(c, x, b, wrong) for b in range(len(c["lens"]))]


def tolerances(r):
    """per element, from the right reference of a sequence: out, lse, dq, dk, dv (allowance x unit)"""
    return dict(out=ALLOW["out/tiled"] * BF * r["u_out"], lse=ALLOW["lse/tiled"] * U * r["u_lse"],
                dq=ALLOW["dq/two_pass"] * BF * r["mags"]["dq"], dk=ALLOW["dk/two_pass"] * BF * r["mags"]["dk"],
                dv=ALLOW["dv/two_pass"] * BF * r["mags"]["dv"])


def stat_block(flat, c, b, stride=None):
    """sequence b's [H][len] block of a flat lse / delta buffer [H total]: at H * row0[b] with row stride len[b] - or with the
    wrong `stride`; positions past the buffer read as NaN"""
    H, n, r0 = c["H"], c["lens"][b], c["row0"][b]
    stride = n if stride is None else stride
    idx = H * r0 + torch.arange(H)[:, None] * stride + torch.arange(n)[None, :]
    ok = idx < flat.numel()
    out = torch.full((H, n), float("nan"), dtype=flat.dtype, device=flat.device)
    out[ok.to(flat.device)] = flat[idx[ok].to(flat.device)]
    return out


def flat_stats(c, blocks):
    """the flat [H total] buffer (NaN outside every block) holding sequence b's [H][len] block at H * row0[b]"""
    flat = torch.full((c["H"] * c["total"],), float("nan"), dtype=torch.float64)
    for b, blk in enumerate(blocks):
        o = c["H"] * c["row0"][b]
        flat[o:o + blk.numel()] = blk.reshape(-1)
    return flat
