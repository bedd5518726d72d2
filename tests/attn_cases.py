"""Case list of the attention planner (csrc/attention.hip: plan_attention behind kalle_attention_fwd_hd / _bwd_hd / _decode_hd /
_decode_rows) shared by tests/test_attn_plan_cpu.py, which asserts with the host queries kalle_attention_*_plan alone that every
case gets the row recorded in tests/golden/attn_plans.json, and by the GPU tests, which ask the query before a real call and
compare its word with kalle_attn_last_plan() afterwards (query()).

A case is a dict over DEFAULT; key(case) names it by the fields that differ, so cases can be added without touching the rows of
the others.  The table was recorded from the dispatcher as it was before plan_attention existed (the library linked against a
stand-in HIP runtime that writes every launch down instead of making it: DESIGN.md 5.9), never from the planner.  CASES holds

- every case of the GPU lists that read a plan word (test_attention_gpu.py, test_llama_hd128_gpu.py, test_decode_rows_gpu.py;
  the attention calls of the decode steps of test_decode_gpu.py / test_decode_rows_gpu.py / test_llama_hd128_gpu.py; the shapes
  of test_head_dims_gpu.py, which reads none), with the literal word the GPU test expects in EXPECT;
- every refusal of their refusal tests;
- a sweep around every edge of the rule for the four entries (sweep());
- FLIPS: per named predicate of attention.hip, pairs of cases that differ in one argument and get different families."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("fwd", "bwd", "decode", "rows")
# lay: where the operands sit (ldq, q_off, ldk, k_off, ldv, v_off, ldo): "plain" q [H dh] and k | v [2 Hkv dh] rows (what the
# decode steps pass), "split" / "fused" the padded layouts of test_attention_gpu.layout; explicit ldq ... ldo override it.
# tables: None = given exactly when rot != 0.  null: the pointer argument that is NULL.  rows: nk, R (None: len(nk)), stride
# (None: (max(nk) + 3) ldk)
DEFAULT = dict(B=2, H=2, Hkv=2, Nq=16, Nk=16, rot=0, causal=0, dh=64, mask=0, tables=None, lay="plain", null=None,
               ldq=None, q_off=None, ldk=None, k_off=None, ldv=None, v_off=None, ldo=None, nk=None, R=None, stride=None)
PTR = dict(q=0x1000, k=0x2000, v=0x3000, out=0x4000, lse=0x5000, cos=0x6000, sin=0x7000, mask=0x8000, dout=0x9000, delta=0xa000,
           dq=0xb000, dk=0xc000, dv=0xd000)
POINTERS = {"fwd": ("q", "k", "v", "out", "lse", "cos", "sin", "mask"),
            "bwd": ("q", "k", "v", "out", "dout", "lse", "delta", "dq", "dk", "dv", "cos", "sin", "mask"),
            "decode": ("q", "k", "v", "out", "lse", "cos", "sin", "mask"),
            "rows": ("q", "k", "v", "out", "lse", "cos", "sin", "nk")}
STRIDES = ("ldq", "q_off", "ldk", "k_off", "ldv", "v_off", "ldo")
OUT_INTS = 12           # kalle_hip.h: word, launches, 2 x (grid x, y, z, block, dynamic LDS)


def C(entry, **kw):
    assert entry in ENTRIES and set(kw) <= set(DEFAULT), kw
    c = dict(DEFAULT, entry=entry)
    c.update(kw)
    if entry in ("decode", "rows"):
        c.update(Nq=1, causal=1)
    if entry == "rows":
        c.update(B=DEFAULT["B"], Nk=DEFAULT["Nk"], mask=0, nk=tuple(c["nk"]))
    return c


def key(c):
    shape = "nk=" + ",".join(map(str, c["nk"])) if c["entry"] == "rows" else f"{c['Nq']}x{c['Nk']}"
    skip = ("Nq", "Nk", "nk") + (("causal",) if c["entry"] in ("decode", "rows") else ())
    return " ".join([c["entry"], shape] + [f"{k}={c[k]}" for k in DEFAULT if k not in skip and c[k] != DEFAULT[k]])


def strides(c):
    """(ldq, q_off, ldk, k_off, ldv, v_off, ldo) of a case"""
    wq, wk = c["H"] * c["dh"], c["Hkv"] * c["dh"]
    if c["lay"] == "fused":
        ld = wq + 2 * wk + 32
        s = [ld, 8, ld, 16 + wq, ld, 24 + wq + wk, wq + 16]
    elif c["lay"] == "split":
        s = [wq + 16, 8, 2 * wk + 24, 8, 2 * wk + 24, 16 + wk, wq + 16]
    else:
        assert c["lay"] == "plain", c
        s = [wq, 0, 2 * wk, 0, 2 * wk, wk, wq]
    return [s[i] if c[n] is None else c[n] for i, n in enumerate(STRIDES)]


def args(c):
    """the arguments of the case's entry point in front of `stream` (of its query in front of `plan`), placeholder pointers: a
    refused call and a query read none of them (but nk, a real host array)"""
    e = c["entry"]
    tables = c["rot"] != 0 if c["tables"] is None else c["tables"]
    have = dict(PTR, cos=PTR["cos"] if tables else None, sin=PTR["sin"] if tables else None, mask=PTR["mask"] if c["mask"] else None)
    if e == "rows":
        have["nk"] = ctypes.cast((ctypes.c_int32 * max(len(c["nk"]), 1))(*c["nk"]), ctypes.c_void_p)
    if c["null"]:
        assert c["null"] in POINTERS[e], c
        have[c["null"]] = None
    p = have.get
    ldq, q_off, ldk, k_off, ldv, v_off, ldo = strides(c)
    head = [p("q"), ldq, q_off, p("k"), ldk, k_off, p("v"), ldv, v_off]
    rope = [p("cos"), p("sin"), c["rot"]]
    if e == "fwd":
        return head + [p("out"), ldo, p("lse")] + rope + [p("mask"), c["causal"], c["B"], c["H"], c["Hkv"], c["Nq"], c["Nk"], c["dh"]]
    if e == "bwd":
        return head + [p("out"), p("dout"), ldo, p("lse"), p("delta"), p("dq"), p("dk"), p("dv")] + rope + \
            [p("mask"), c["causal"], c["B"], c["H"], c["Hkv"], c["Nq"], c["Nk"], c["dh"]]
    if e == "decode":
        return head + [p("out"), ldo, p("lse")] + rope + [p("mask"), c["B"], c["H"], c["Hkv"], c["Nk"], c["dh"]]
    R = len(c["nk"]) if c["R"] is None else c["R"]
    stride = (max(max(c["nk"], default=0), 0) + 3) * ldk if c["stride"] is None else c["stride"]
    return head + [stride, p("out"), ldo, p("lse")] + rope + [have["nk"], R, c["H"], c["Hkv"], c["dh"]]


FUNCS = {"fwd": "kalle_attention_fwd", "bwd": "kalle_attention_bwd", "decode": "kalle_attention_decode", "rows": "kalle_attention_decode_rows"}


def entry_point(lib, c):
    return getattr(lib, FUNCS[c["entry"]] + ("" if c["entry"] == "rows" else "_hd"))


def query(lib, c_or_entry, call_args=None, fill=77):
    """the host query of an entry point: (return code, the OUT_INTS ints of `plan`, which stay `fill` on a refusal).  Either a
    case, or an entry name and the real call's arguments in front of `stream`"""
    entry, a = (c_or_entry["entry"], args(c_or_entry)) if call_args is None else (c_or_entry, list(call_args))
    out = (ctypes.c_int32 * OUT_INTS)(*[fill] * OUT_INTS)
    rc = getattr(lib, FUNCS[entry] + "_plan")(*a, out)
    return rc, list(out)


def step_word(lib, hd, H, Hkv, t0, cache_rows=None):
    """the query's word for the attention call of a decode step (csrc/llasa.hip: decode_step): t0 an int for the one-row
    step, a tuple for the R-row step (t0[r] < 0: row r inactive)"""
    if isinstance(t0, int):
        c = C("decode", B=1, H=H, Hkv=Hkv, Nk=t0 + 1, rot=hd, dh=hd)
    else:
        c = C("rows", nk=tuple(max(t + 1, 0) for t in t0), H=H, Hkv=Hkv, rot=hd, dh=hd, stride=cache_rows * 2 * Hkv * hd)
    rc, out = query(lib, c)
    assert rc == 0, (key(c), rc)
    return out[0]


def row_of(rc, out):
    """the table's row of a query result: [return code, word, launches, then grid x, y, z, block, LDS of each launch]"""
    return [rc, 0, 0] if rc != 0 else [rc, out[0], out[1]] + out[2:2 + 5 * out[1]]


# ------------------------------------------------------------------------------------------------ the GPU tests' cases
def from_A(c, entry, **kw):
    """a case dict of test_attention_gpu.A"""
    d = dict(H=c["H"], Hkv=c["Hkv"], Nq=c["Nq"], Nk=c["Nk"], rot=c["rot"], causal=int(c["causal"]), dh=c["dh"],
             mask=int(c["mask"] != "none"), lay=c["layout"])
    d.update(kw)
    return C(entry, **d)


def decode_word(dh, rot):
    return (2 if dh == 64 else 6) | dh << 8 | rot << 17


def rows_word(dh, rot):
    return 7 | dh << 8 | rot << 17


def gpu_cases():
    """(case, the word the GPU test that runs it expects, or None where that test reads none)"""
    import decode_cases as dc
    import decode_rows_cases as rc
    import llama_hd128_cases as lc
    import test_attention_gpu as ta
    import test_head_dims_gpu as th
    out = []

    def both(c):
        out.append((from_A(c, "fwd"), c["fwd"]))
        if c["bwd"] is not None:
            out.append((from_A(c, "bwd"), c["bwd"]))

    pair = ta.A(2, 33, ta.T64, None, rot=32, causal=True, H=4, Hkv=1, mask="random")
    pair128 = ta.A(2, 33, lc.T128, None, dh=128, rot=128, causal=True, H=4, Hkv=1, mask="random")
    for c in ta.CASES_64 + ta._hd_cases(32, (32, 32)) + ta._hd_cases(128, (64, 32)) + ta.DECODE_CASES + [w[1] for w in ta.WRONG] + \
            [pair, dict(pair, Nq=1, fwd=ta.decode(32))] + lc.TILED_CASES + [w[1] for w in lc.WRONG] + [pair128]:
        both(c)
    for c in lc.DECODE_CASES + [dict(pair128, Nq=1, fwd=lc.decode128())]:
        out.append((from_A(c, "decode"), c["fwd"]))
    for rot in (0, 32, 64):         # test_decode_hd_at_head_dim_64_is_attention_fwd_bit_for_bit
        c = ta.A(1, 257, lc.decode64(rot), None, rot=rot, causal=True, H=4, Hkv=2, mask="random")
        out += [(from_A(c, "decode"), c["fwd"]), (from_A(c, "fwd"), c["fwd"])]
    for dh in (32, 64, 128):        # test_head_dims_gpu.py (through ops: no plan word read)
        for Nq, Nk, H, Hkv, rot, mask, causal, _lay in th._cases(dh):
            for e in ("fwd", "bwd")[:1 + (Nq > 1)]:
                out.append((C(e, Nq=Nq, Nk=Nk, H=H, Hkv=Hkv, rot=rot, mask=int(mask), causal=int(causal), dh=dh), None))
    for Nq, Nk, H, Hkv, rot, causal in [(126, 126, 4, 4, 32, 0), (126, 130, 4, 2, 0, 0), (300, 300, 2, 2, 64, 1), (1, 200, 4, 1, 64, 1)]:
        out += [(C(e, Nq=Nq, Nk=Nk, H=H, Hkv=Hkv, rot=rot, causal=causal, mask=1), None) for e in ("fwd", "bwd")]
    # the attention call of the decode steps (csrc/llasa.hip: decode_step): one batch row, the layer's cache as k | v
    for dh, cases in ((64, dc.CASES), (128, lc.STEP_CASES)):
        for c in cases.values():
            out.append((C("decode", B=1, H=c["H"], Hkv=c["Hkv"], Nk=c["t0"] + 1, rot=dh, dh=dh), decode_word(dh, dh)))
    for c in rc.STEP_CASES.values():
        nk = tuple(max(t + 1, 0) for t in c["t0"])
        out.append((C("rows", nk=nk, H=c["H"], Hkv=c["Hkv"], rot=c["hd"], dh=c["hd"], stride=c["rows"] * 2 * c["Hkv"] * c["hd"]),
                    rows_word(c["hd"], c["hd"])))
    for dh, rot in rc.ATTN_HEADS:   # test_attention_rows: the rows call, then each live row alone through decode_hd
        for nk in rc.ATTN_NK:
            out.append((C("rows", nk=nk, H=4, Hkv=2, rot=rot, dh=dh), rows_word(dh, rot)))
            out += [(C("decode", B=1, H=4, Hkv=2, Nk=n, rot=rot, dh=dh), decode_word(dh, rot)) for n in nk if n > 0]
    out.append((C("rows", nk=(1, 2, 3), H=4, Hkv=2, rot=64), rows_word(64, 64)))
    return out


def refusals():
    """the refusal tests of the GPU files, argument for argument: every one is KALLE_ERR_ARG with plan word 0"""
    N, H = 16, 2
    out = []
    # test_attention_gpu.test_rejected_calls_write_nothing (forward and backward), its NULL dq
    base = dict(Nq=N, Nk=N, H=H, Hkv=H, rot=32, lay="fused")
    ld = 3 * H * 64 + 32
    for kw in [dict(causal=1, Nk=N - 1), dict(H=3, Hkv=2), dict(ldq=ld + 4), dict(ldk=ld + 4), dict(ldv=ld + 4), dict(ldo=H * 64 + 12),
               dict(q_off=4), dict(k_off=20), dict(v_off=12), dict(rot=16), dict(rot=48), dict(rot=64, dh=32), dict(null="cos"),
               dict(null="sin"), dict(dh=48)]:
        out += [C(e, **dict(base, **kw)) for e in ("fwd", "bwd")]
    out.append(C("bwd", **dict(base, null="dq")))
    # test_llama_hd128_gpu.test_rejected_attention_calls_write_nothing
    base = dict(Nk=N, H=H, Hkv=H, rot=128, dh=128, lay="fused")
    for kw in [dict(dh=32, rot=32), dict(dh=96), dict(dh=64, rot=128), dict(rot=48), dict(rot=64), dict(rot=0), dict(null="cos"),
               dict(null="sin"), dict(H=3, Hkv=2), dict(q_off=4), dict(k_off=20 + H * 128), dict(v_off=12), dict(ldk=3 * H * 128 + 36),
               dict(ldo=H * 128 + 12), dict(Nk=0)]:
        out.append(C("decode", **dict(base, **kw)))
    # test_decode_rows_gpu.test_attention_rows_refusals
    for kw in [dict(nk=(1, 15361, 2)), dict(nk=(1,), R=0), dict(nk=(1,) * 17), dict(nk=(1, 2, 3), rot=32), dict(nk=(1, 2, 3), dh=32)]:
        out.append(C("rows", **dict(dict(H=4, Hkv=2, rot=64, null="lse"), **kw)))
    # test_head_dims_gpu.test_attention_hd_rejects_bad_arguments
    for dh, rot in ((48, 0), (256, 0), (0, 0), (32, 64), (128, 16)):
        out.append(C("fwd", B=1, H=1, Hkv=1, Nq=4, Nk=4, dh=dh, rot=rot, tables=1, ldq=384, q_off=0, ldk=384, k_off=128, ldv=384,
                     v_off=256, ldo=128))
    return out


# ------------------------------------------------------------------------------------------------ the sweep
NQ = (1, 2, 16, 17, 112, 113, 126, 127, 128, 129, 257)
NK = (1, 7, 127, 128, 129, 130, 144, 145, 160, 161, 257, 15360, 15361)
ROT = (0, 16, 32, 48, 64, 128)
HEADS = ((2, 2), (4, 1), (4, 2), (3, 2))
DH = (32, 48, 64, 128)
NK_ROWS = ((0, 0, 0), (-1, 0), (0, 5, 0), (1, 257, 130), (37, 0, 37), (15360, 1), (15361, 1), (1, 15361), (15360,) * 16)
ROWS_R = (0, 1, 16, 17)
ROWS_STRIDE = (0, 8, 12, -8)
ROWS_HEADS = ((64, 0), (64, 32), (64, 64), (64, 128), (128, 128), (128, 64), (128, 0), (32, 32), (32, 0), (48, 0))   # (head dim, rot)


def sweep():
    out = []
    # the backward's rule lives at head dim 64 in (Nq, Nk, causal, rot == 0, H == Hkv): the full product; the forward's in
    # (Nq == 1, Nk, causal, rot == 0)
    for Nq in NQ:
        for Nk in NK:
            for causal in (0, 1):
                for rot in (0, 32):
                    out += [C("bwd", Nq=Nq, Nk=Nk, causal=causal, rot=rot, H=H, Hkv=Hkv) for H, Hkv in ((2, 2), (4, 1))]
                    if Nq in (1, 2, 129):
                        out.append(C("fwd", Nq=Nq, Nk=Nk, causal=causal, rot=rot))
    # every head dim x rot x entry, tables given: at a small shape, at one query, and past the ceiling
    for dh in DH:
        for rot in ROT:
            for Nq, Nk in ((17, 130), (1, 130), (1, 15361), (129, 160)):
                out += [C(e, Nq=Nq, Nk=Nk, dh=dh, rot=rot, tables=1) for e in ("fwd", "bwd")]
            out += [C("decode", Nk=Nk, dh=dh, rot=rot, tables=1, H=4, Hkv=1) for Nk in (1, 130, 15360, 15361)]
    # the head dims away from 64: the shape axes alone
    for dh in (32, 128):
        for Nq in (1, 2, 128, 129, 257):
            for Nk in NK:
                out += [C(e, Nq=Nq, Nk=Nk, dh=dh, causal=causal) for e in ("fwd", "bwd") for causal in (0, 1)]
    for dh, rot in ((64, 0), (64, 32), (64, 64), (128, 128)):
        out += [C("decode", Nk=Nk, dh=dh, rot=rot, H=H, Hkv=Hkv) for Nk in NK for H, Hkv in ((2, 2), (4, 1))]
    # heads; mask and tables given or not; B and H at the grid limit
    for e in ("fwd", "bwd", "decode"):
        for dh in (64, 128):
            rot0 = 128 if (e, dh) == ("decode", 128) else 0
            out += [C(e, H=H, Hkv=Hkv, dh=dh, rot=rot0, Nq=Nq, Nk=Nk) for H, Hkv in HEADS + ((65535, 1), (65536, 1), (65535, 65535), (2, 0), (0, 1))
                    for Nq, Nk in ((16, 16), (126, 130))]
            out += [C(e, B=B, dh=dh, rot=rot0) for B in (0, 1, 65535, 65536)]
            out += [C(e, dh=dh, rot=rot, mask=mask, tables=tables, Nq=Nq, Nk=Nk) for rot in sorted({rot0, 32, dh}) for mask in (0, 1)
                    for tables in (0, 1) for Nq, Nk in ((16, 16), (1, 130))]
            out += [C(e, dh=dh, rot=rot0, Nq=Nq, Nk=Nk) for Nq, Nk in ((0, 16), (16, 0), (-1, 16), (16, -1))]
    out += [C(e, causal=causal, Nq=17, Nk=Nk) for e in ("fwd", "bwd") for causal in (2, -1) for Nk in (16, 17, 144)]
    # a NULL in each pointer argument in turn, each ld / offset misaligned in turn
    for e in ENTRIES:
        for dh, rot in ((64, 64), (128, 128), (64, 0)):
            base = C(e, dh=dh, rot=rot, mask=int(e != "rows"), nk=(3, 0, 9) if e == "rows" else None, Nq=17, Nk=130)
            out += [dict(base, null=n) for n in POINTERS[e]]
            out += [dict(base, **{n: v + 4}) for n, v in zip(STRIDES, strides(base))]
            out += [dict(base, **{n: v + 8}) for n, v in zip(STRIDES, strides(base))]
    # rows: the key counts, R, the cache stride, the instantiations
    for dh, rot in ROWS_HEADS:
        out += [C("rows", nk=nk, dh=dh, rot=rot, H=H, Hkv=Hkv) for nk in NK_ROWS for H, Hkv in ((4, 2), (3, 2))]
        out += [C("rows", nk=(5,) * max(R, 1), R=R, dh=dh, rot=rot) for R in ROWS_R + (-1,)]
        out += [C("rows", nk=nk, stride=s, dh=dh, rot=rot) for s in ROWS_STRIDE for nk in ((3, 0, 9), (0, 0))]
        out += [C("rows", nk=(3, 0, 9), dh=dh, rot=rot, H=H, Hkv=Hkv) for H, Hkv in HEADS + ((65535, 1), (65536, 1))]
        out += [C("rows", nk=(3, 0, 9), dh=dh, rot=rot, tables=t) for t in (0, 1)]
    out += [C("rows", nk=(0, 0), null=n) for n in POINTERS["rows"]] + [C("rows", nk=(0, 0), rot=32), C("rows", nk=(0, 0), H=3, Hkv=2)]
    return out


# ------------------------------------------------------------------------------------------------ each predicate flips
# (the predicate of attention.hip, a case, the one argument changed, the families before and after; 0 = refused)
FLIPS = [
    ("attn_bwd_fused", C("bwd", Nq=128, Nk=128), dict(Nk=129), 4, 3),
    ("attn_bwd_fused", C("bwd", Nq=128, Nk=128), dict(Nq=129), 4, 3),
    ("attn_bwd_fused", C("bwd", Nq=16, Nk=16, rot=32), dict(causal=1), 4, 3),
    ("attn_bwd_fused", C("bwd", Nq=16, Nk=16, rot=32, H=4, Hkv=1), dict(Hkv=4), 3, 4),
    ("attn_bwd_fused", C("bwd", Nq=16, Nk=16), dict(dh=128), 4, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=112, Nk=144), dict(Nq=113), 5, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=112, Nk=144), dict(Nk=145), 5, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=127, Nk=129), dict(Nk=130), 5, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=128, Nk=128, H=4, Hkv=1), dict(Nq=129), 5, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=16, Nk=16, H=4, Hkv=1), dict(rot=32), 5, 3),
    ("attn_bwd_fused_gqa", C("bwd", Nq=16, Nk=16, H=4, Hkv=1), dict(causal=1), 5, 3),
    ("attn_fold_tail", C("fwd", Nq=2, Nk=128), dict(Nk=129), 1, 1 | 1 << 16),
    ("attn_fold_tail", C("fwd", Nq=2, Nk=160), dict(Nk=161), 1 | 1 << 16, 1),
    ("attn_fold_tail", C("fwd", Nq=2, Nk=144), dict(rot=32), 1 | 1 << 16, 1),
    ("attn_fold_tail", C("fwd", Nq=2, Nk=144), dict(causal=1), 1 | 1 << 16, 1),
    ("attn_decode_fits", C("fwd", Nq=1, Nk=15360), dict(Nk=15361), 2, 1),
    ("attn_decode_fits", C("decode", Nk=15360, dh=128, rot=128), dict(Nk=15361), 6, 1),
    ("attn_decode_fits", C("rows", nk=(15360, 1)), dict(nk=(15361, 1)), 7, 0),
    ("attn_fwd_decode", C("fwd", Nq=1, Nk=130), dict(Nq=2), 2, 1 | 1 << 16),
    ("attn_fwd_decode", C("fwd", Nq=1, Nk=130), dict(dh=128), 2, 1 | 1 << 16),
    ("attn_fwd_decode128", C("decode", Nk=130, dh=128, rot=128, H=4, Hkv=1), dict(dh=64), 6, 0),
    ("attn_rot_exists", C("rows", nk=(3, 0, 9), rot=64, dh=64), dict(rot=32), 7, 0),
    ("attn_rot_exists", C("decode", Nk=130, rot=128, dh=128, tables=1, H=4, Hkv=1), dict(rot=64), 6, 0),
    ("attn_rot_exists", C("fwd", Nq=17, Nk=130, rot=32, dh=32, tables=1), dict(rot=64), 1, 0),
    ("attn_head_dim_exists", C("decode", Nk=130, dh=64, H=4, Hkv=1), dict(dh=32), 2, 0),
    ("attn_head_dim_exists", C("fwd", Nq=17, Nk=130, dh=32, tables=1), dict(dh=48), 1 | 1 << 16, 0),
]


def _build():
    seen, cases, expect = set(), [], {}
    for c, want in gpu_cases() + [(c, None) for c in refusals() + sweep()] + \
            [(x, None) for _n, c, kw, _a, _b in FLIPS for x in (c, C(c["entry"], **{k: v for k, v in dict(c, **kw).items() if k in DEFAULT}))]:
        k = key(c)
        if want is not None:
            assert expect.setdefault(k, want) == want, k
        if k not in seen:
            seen.add(k)
            cases.append(c)
    return cases, expect


CASES, EXPECT = _build()
