"""-m gpu: the wide decode path - gemm_rows_kernel at NCB = 2 .. 4 behind kalle_gemm_rows_wide and kalle_llama_decode_step_wide, 17 .. 64
rows per read of the weights - by the method, helpers and bounds of tests/test_decode_rows_gpu.py (nothing new is measured): every
element of the GEMM against the fp64 reference under NaN-guarded buffers, and, the property the wide path promises, every row BIT
FOR BIT what the 16-row entry points give for the chunk of up to 16 rows that holds it - outputs, second destination, xhat,
caches and the published workspace regions.  Inactive rows are neither read (NaN inputs) nor written (fills come back bit for bit);
refusals write nothing; wrong references are caught."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_rows_cases as rc  # noqa: E402
import decode_wide_cases as wc  # noqa: E402
import test_decode_gpu as td  # noqa: E402
import test_decode_rows_gpu as tr  # noqa: E402
from gpu_checks import NAN, Guard, _bits, check, guarded as _guarded  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FENCE = tr.FENCE
BF, F32 = torch.bfloat16, torch.float32
P, iarr, same_bits = td.P, tr.iarr, tr.same_bits
PROS = [rc.PRO_BF16, rc.PRO_RMS, rc.PRO_SWIGLU]
PRO_IDS = ["bf16", "rms", "swiglu"]


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


# ------------------------------------------------------------------------------------------------ the GEMM
class Gemm(tr.Gemm):
    """tr.Gemm through kalle_gemm_rows_wide on the inputs of decode_wide_cases; `rows_entry` runs kalle_gemm_rows_fused on one
    chunk of the SAME buffers into fresh outputs"""

    def __init__(self, lib, N, K, nsplit, R, pro, f32, with_res, inactive=(), entry="kalle_gemm_rows_wide", fill=NAN):
        self.a = (N, K, nsplit, R, pro, f32, with_res, tuple(inactive))
        xin, gamma = wc.gemm_inputs(N, K, R, pro) if R > 16 else rc.gemm_inputs(N, K, R, pro)
        self.cols = cols = 2 * K if pro == rc.PRO_SWIGLU else K
        self.X = Guard(R, cols, ld=cols + 8, dtype=F32 if pro == rc.PRO_RMS else BF, init=xin.cuda())
        for r in inactive:
            self.X.v[r] = NAN
        self.gamma = gamma.cuda() if gamma is not None else None
        g = torch.Generator(device="cuda").manual_seed(N * K + R)
        self.W = Guard(N, K, ld=K + 8, dtype=BF, init=torch.randn((N, K), generator=g, device="cuda") / K ** 0.5)
        self.res = torch.randn((R, N), generator=g, device="cuda") if with_res else None
        for r in inactive if with_res else ():
            self.res[r] = NAN
        self.n2 = N - nsplit
        self.outputs(R)
        self.rc = self.call(lib, entry, 0, R, [0 if r in inactive else 1 for r in range(R)])

    def outputs(self, R):
        N, K, nsplit, _, pro, f32, _, _ = self.a
        ydt = F32 if f32 else BF
        self.Y = Guard(R, nsplit, ld=nsplit + 5, dtype=ydt)
        self.y2 = torch.full((R, 3, max(self.n2, 1)), NAN, device="cuda", dtype=ydt)      # row r's destination: y2[r][1]
        self.hbuf, self.xhat = _guarded(torch.full((R, K), NAN, device="cuda", dtype=BF))

    def call(self, lib, entry, r0, rn, active):
        """rows r0 .. r0 + rn of the inputs into rows 0 .. rn of the current outputs"""
        N, K, nsplit, _, pro, f32, with_res, _ = self.a
        code = getattr(lib, entry)(
            P(self.X.v[r0:]), self.cols + 8, pro, P(self.gamma), ctypes.c_float(rc.EPS), P(self.xhat), P(self.W.v), K + 8, P(self.Y.v),
            nsplit + 5, 1 if f32 else 0, P(self.y2) if self.n2 else None, nsplit,
            iarr([(3 * r + 1) * self.n2 for r in range(rn)], ctypes.c_int64) if self.n2 else None,
            P(self.res[r0:]) if with_res else None, N if with_res else 0, iarr(active), rn, N, K, None)
        torch.cuda.synchronize()
        return code

    def rows_entry(self, lib, r0):
        """(Y, y2, xhat) of kalle_gemm_rows_fused on rows r0 .. min(r0 + 16, R) of the same X, W, residual"""
        R, inactive = self.a[3], self.a[7]
        rn = min(16, R - r0)
        keep = self.Y, self.y2, self.hbuf, self.xhat
        self.outputs(rn)
        code = self.call(lib, "kalle_gemm_rows_fused", r0, rn, [0 if r0 + r in inactive else 1 for r in range(rn)])
        assert code == 0, (self.a, r0, code)
        out = self.Y.v, self.y2, self.xhat
        self.Y, self.y2, self.hbuf, self.xhat = keep
        return out

    def same_as_rows_entry(self, lib):
        R = self.a[3]
        for r0 in range(0, R, 16):
            Y, y2, xhat = self.rows_entry(lib, r0)
            rn = Y.shape[0]
            what = f"{self.a} rows {r0} .. {r0 + rn}"
            same_bits(self.Y.v[r0:r0 + rn], Y, what + " y vs kalle_gemm_rows_fused")
            same_bits(self.y2[r0:r0 + rn], y2, what + " y2 vs kalle_gemm_rows_fused")
            same_bits(self.xhat[r0:r0 + rn], xhat, what + " xhat vs kalle_gemm_rows_fused")


@pytest.mark.parametrize("pro", PROS, ids=PRO_IDS)
@pytest.mark.parametrize("R", wc.GEMM_ROWS)
@pytest.mark.parametrize("N,K,nsplit", wc.GEMM_SHAPES)
def test_gemm_wide_every_element_and_bits_of_the_rows_entry(kl, N, K, nsplit, R, pro):
    """fp32 and bf16 outputs, with and without residual, row strides larger than the widths, (520, 2056): a second destination
    with NaN rows either side; then every row against kalle_gemm_rows_fused on its chunk of 16, bit for bit"""
    ops, lib = kl
    for f32 in (True, False):
        for with_res in (False, True):
            g = Gemm(lib, N, K, nsplit, R, pro, f32, with_res)
            g.verify(lib)
            g.same_as_rows_entry(lib)


@pytest.mark.parametrize("R", [1, 16])
def test_gemm_wide_up_to_16_rows_is_the_rows_entry(kl, R):
    ops, lib = kl
    for (N, K, nsplit), pro in ((rc.GEMM_SHAPES[2], rc.PRO_RMS), (rc.GEMM_SHAPES[1], rc.PRO_SWIGLU), (rc.GEMM_TILE_SHAPES[1], rc.PRO_BF16)):
        g = Gemm(lib, N, K, nsplit, R, pro, False, True)
        g.verify(lib)
        g.same_as_rows_entry(lib)


DEAD = [(48, tuple(range(16, 32))), (33, (32,)), (64, tuple(range(63)))]


@pytest.mark.parametrize("pro", PROS, ids=PRO_IDS)
@pytest.mark.parametrize("R,dead", DEAD, ids=["block1-dead", "last-row-dead", "only-row-63"])
@pytest.mark.parametrize("N,K,nsplit", [rc.GEMM_SHAPES[0], rc.GEMM_SHAPES[2], wc.WIDE_TILE_SHAPES[1]])
def test_gemm_wide_inactive_rows(kl, N, K, nsplit, R, dead, pro):
    """their x and residual rows are NaN (never read); their y rows, second destinations and xhat rows come back bit for bit"""
    ops, lib = kl
    for f32 in (True, False):
        g = Gemm(lib, N, K, nsplit, R, pro, f32, True, inactive=dead)
        g.verify(lib)
        g.same_as_rows_entry(lib)
        d = list(dead)
        same_bits(g.Y.v[d], torch.full_like(g.Y.v[d], NAN), "inactive y rows")
        same_bits(g.y2[d], torch.full_like(g.y2[d], NAN), "inactive second destinations")
        same_bits(g.xhat[d], torch.full_like(g.xhat[d], NAN), "inactive xhat rows")


@pytest.mark.parametrize("pro", PROS, ids=PRO_IDS)
def test_gemm_wide_every_row_inactive_writes_nothing(kl, pro):
    ops, lib = kl
    N, K, nsplit = rc.GEMM_SHAPES[2]
    g = Gemm(lib, N, K, nsplit, 33, pro, True, True, inactive=tuple(range(33)))
    assert g.rc == 0
    for t in (g.Y.buf, g.y2, g.hbuf):
        assert torch.isnan(t).all()


def test_gemm_wide_wrapper(kl):
    """ops.gemm_rows_wide: strided x rows, residual, both output types; a row is ops.gemm_rows' on its chunk, bit for bit"""
    ops, lib = kl
    g = torch.Generator(device="cuda").manual_seed(6)
    W = (torch.randn((264, 1000), generator=g, device="cuda") / 1000 ** 0.5).to(BF)
    xfull = torch.randn((40, 1016), generator=g, device="cuda").to(BF)
    res = torch.randn((40, 264), generator=g, device="cuda")
    for dt, r in ((F32, res), (BF, None)):
        y = ops.gemm_rows_wide(xfull[:, :1000], W, residual=r, out_dtype=dt)
        torch.cuda.synchronize()
        for i in (0, 15, 16, 39):
            ref, tol = td.gemv_ref(W, xfull[i, :1000].double(), 1000, res=r[i].double() if r is not None else None, bf16_out=dt == BF)
            check(y[i], ref, tol, f"ops.gemm_rows_wide row {i}")
        for r0 in (0, 16, 32):
            same_bits(y[r0:r0 + 16], ops.gemm_rows(xfull[r0:r0 + 16, :1000], W, residual=None if r is None else r[r0:r0 + 16], out_dtype=dt),
                      "ops.gemm_rows_wide vs ops.gemm_rows")


def test_gemm_wide_refusals_write_nothing(kl):
    ops, lib = kl
    W = torch.zeros((70, 32776), device="cuda", dtype=BF)
    x = torch.zeros((65, 32776), device="cuda", dtype=BF)
    y = torch.full((65, 70), NAN, device="cuda")
    y2 = torch.full((65, 70), NAN, device="cuda")
    gamma = torch.ones(32776, device="cuda")
    xhat = torch.full((65, 64), NAN, device="cuda", dtype=BF)
    off = iarr([70 * r for r in range(65)], ctypes.c_int64)

    def call(R=33, K=64, N=70, pro=0, ldx=32776, nsplit=None, y2=None, off=None, gamma=gamma, xhat=xhat, ydt=1, x=x):
        return lib.kalle_gemm_rows_wide(P(x), ldx, pro, P(gamma), ctypes.c_float(1e-5), P(xhat), P(W), 32776, P(y), 70, ydt, P(y2), N if nsplit is None else nsplit,
                                        off, None, 0, None, R, N, K, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert (y[:33] == 0).all() and torch.isnan(y[33:]).all()
    y.fill_(NAN)
    for kw in (dict(R=0), dict(R=65), dict(K=60), dict(K=32776), dict(N=0), dict(pro=3), dict(ldx=60), dict(nsplit=32), dict(nsplit=80),
               dict(nsplit=32, y2=y2), dict(nsplit=32, off=off), dict(pro=1, ldx=66), dict(pro=1, gamma=None), dict(pro=2, xhat=None), dict(ydt=2),
               dict(x=None)):
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(y2).all() and torch.isnan(xhat).all()


WRONG_MARGIN = tr.WRONG_MARGIN


def test_gemm_wide_wrong_references_are_caught(kl):
    """the mix-ups a wide kernel can make: the operand of the same lane's row in the next column block, the second destination
    of the row one block back, the residual of the next row"""
    ops, lib = kl
    cases = []
    g = Gemm(lib, 264, 1000, 264, 33, rc.PRO_RMS, True, True)
    ref, tol = g.ref(3)
    cases.append(("row r + 16's operand", g.got(3), ref, tol, g.ref(3, x_row=19)[0]))
    cases.append(("row r + 1's residual", g.got(3), ref, tol, g.ref(3, res_row=4)[0]))
    N, K, nsplit = rc.GEMM_SHAPES[2]
    g = Gemm(lib, N, K, nsplit, 33, rc.PRO_BF16, True, False)
    ref, tol = g.ref(20)
    there = torch.cat([g.Y.v[20], g.y2[4, 1, :g.n2]])           # y2_off of row r - 16: what a kernel indexing y2_off by lane would fill
    cases.append(("row r - 16's y2_off", g.got(20), ref, tol, None))
    for what, got, ref, tol, wref in cases:
        check(got, ref, tol, what + ": right reference")
        if wref is None:
            with pytest.raises(AssertionError, match="out of bound"):
                check(there, ref, tol, what)
            assert ((there.double() - ref).abs() / tol).max().item() > WRONG_MARGIN, what
            continue
        assert ((wref - ref).abs() / tol).max().item() > WRONG_MARGIN, what
        with pytest.raises(AssertionError, match="out of bound"):
            check(got, wref, tol, what)


# ------------------------------------------------------------------------------------------------ the step
def regions(ws, R, D, H, inner):
    """tr.Setup.regions for any R: the workspace as the header lays it out"""
    o, out = 0, {}
    for name, n, dt in (("x2", D, F32), ("x3", D, F32), ("lse", H, F32), ("q", D, BF), ("ao", D, BF), ("hf", 2 * inner, BF),
                        ("xn", max(D, inner), BF)):
        nb = R * n * (4 if dt == F32 else 2)
        out[name] = ws[o:o + nb].view(dt).view(R, n)
        if name == "lse":
            out["lse_pad"] = ws[o + nb:o + ((nb + 63) & ~63)]
            nb = (nb + 63) & ~63
        o += nb
    assert o == ws.numel()
    return out


class Step:
    """tr.Setup for the wide step (its layers, x, out, tables and fenced workspace at any R), and the same call through
    kalle_llama_decode_step_rows for one chunk of 16 rows on copies of the caches"""

    def __init__(self, lib, c, n_layers=2):
        from kalle_audio_amd import _lib
        self.c, self.lib, self._lib = c, lib, _lib
        hd, H, Hkv, inner, t0 = c["hd"], c["H"], c["Hkv"], c["inner"], c["t0"]
        self.R, self.D = len(t0), hd * H
        g = torch.Generator(device="cuda").manual_seed(c["seed"])
        self.layers = [tr.Layer(c, g, i) for i in range(n_layers)]
        self.arr = self.descriptors([L.cache for L in self.layers])
        x = rc.step_inputs(c)[0].cuda()
        for r, t in enumerate(t0):
            if t < 0:
                x[r] = NAN
        self.xbuf, self.x = _guarded(x)
        self.obuf, self.out = _guarded(torch.full((self.R, self.D), NAN, device="cuda"))
        cos, sin = rc.rope_tables(c["rows"], hd)
        cos[max(t0) + 1:], sin[max(t0) + 1:] = NAN, NAN
        self.cos, self.sin = cos.cuda(), sin.cuda()
        self.ws_bytes = lib.kalle_llama_decode_ws_bytes_wide(self.R, H, Hkv, inner, hd)
        assert self.ws_bytes == rc.ws_bytes(self.R, H, inner, hd)
        self.wsbuf, self.ws = self.workspace(self.ws_bytes)

    @staticmethod
    def workspace(nbytes):
        buf = torch.full((nbytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)
        ws = buf[FENCE:FENCE + nbytes]
        assert ws.data_ptr() % 64 == 0
        return buf, ws

    def descriptors(self, caches):
        arr = (self._lib.LlamaLayer * len(self.layers))()
        for d, L, cache in zip(arr, self.layers, caches):
            d.input_norm, d.wqkv, d.wo, d.post_norm, d.wug, d.wdown, d.kv_cache = (
                t.data_ptr() for t in (L.input_norm, L.wqkv, L.wo, L.post_norm, L.wug, L.wdown, cache))
        return arr

    def step(self, entry="kalle_llama_decode_step_wide", arr=None, x=None, out=None, ws=None, **over):
        c = self.c
        a = dict(R=self.R, H=c["H"], Hkv=c["Hkv"], inner=c["inner"], hd=c["hd"], t0=c["t0"], rows=c["rows"], n=len(self.layers))
        a.update(over)
        code = getattr(self.lib, entry)(ctypes.cast(self.arr if arr is None else arr, ctypes.c_void_p), a["n"], P(self.x if x is None else x),
                                        P(self.out if out is None else out), a["R"], a["H"], a["Hkv"], a["inner"], a["hd"], ctypes.c_float(rc.EPS),
                                        iarr(list(a["t0"])), a["rows"], P(self.cos), P(self.sin), P(self.ws if ws is None else ws), None)
        torch.cuda.synchronize()
        return code

    def rows_step(self, r0, caches_of=None):
        """kalle_llama_decode_step_rows on rows r0 .. r0 + 16: (out, caches per layer, workspace regions), the caches copies of
        what the wide call started from (caches_of: of the rows from THAT row on instead - a seeded defect)"""
        c = self.c
        rn = min(16, self.R - r0)
        c0 = r0 if caches_of is None else caches_of
        caches = [L.cache_before[c0:c0 + rn].clone() for L in self.layers]
        out = torch.full((rn, self.D), NAN, device="cuda")
        nbytes = self.lib.kalle_llama_decode_ws_bytes_rows(rn, c["H"], c["Hkv"], c["inner"], c["hd"])
        wsbuf, ws = self.workspace(nbytes)
        code = self.step("kalle_llama_decode_step_rows", arr=self.descriptors(caches), x=self.x[r0:r0 + rn].clone(), out=out, ws=ws, R=rn,
                         t0=c["t0"][r0:r0 + rn])
        assert code == 0, (r0, code)
        assert (wsbuf[:FENCE] == 0xFF).all() and (wsbuf[FENCE + nbytes:] == 0xFF).all()
        return out, caches, regions(ws, rn, self.D, c["H"], c["inner"])

    def untouched(self, what):
        assert (self.wsbuf == 0xFF).all() and torch.isnan(self.out).all(), what
        for L in self.layers:
            same_bits(L.cache, L.cache_before, what + " cache")


STEPS = [(name, R) for name in rc.STEP_CASES for R in (33, 64)]


@pytest.mark.parametrize("name,R", STEPS, ids=[f"{n}-R{r}" for n, r in STEPS])
def test_step_wide_is_the_rows_step_per_chunk(kl, name, R):
    """R = 33: t0 mixes 0, 37, mid values and -1 and rows 16 .. 31 are all inactive (a chunk that launches no attention); R = 64:
    every row active.  Two layers, so x3 is handed over.  Everything a row owns - out, its cache rows in both layers, its rows of
    every workspace region - equals the _rows step on its chunk bit for bit; an inactive row's come back as they were"""
    ops, lib = kl
    c = wc.step_case(name, R)
    s = Step(lib, c)
    assert s.step() == 0, (name, R, lib.kalle_last_error())
    assert ops.attn_last_plan() == tr.rows_plan(c["hd"], c["hd"]), hex(ops.attn_last_plan())
    reg = regions(s.ws, R, s.D, c["H"], c["inner"])
    for r0 in range(0, R, 16):
        out, caches, creg = s.rows_step(r0)
        rn = out.shape[0]
        what = f"{name} R {R} rows {r0} .. {r0 + rn}"
        same_bits(s.out[r0:r0 + rn], out, what + " out")
        for L, cache in zip(s.layers, caches):
            same_bits(L.cache[r0:r0 + rn], cache, what + " caches")
        for k in creg:
            if not k.endswith("_pad"):
                same_bits(reg[k][r0:r0 + rn], creg[k], f"{what} workspace {k}")
    for r, t in enumerate(c["t0"]):
        if t >= 0:
            assert torch.isfinite(s.out[r]).all(), (name, r)
            for L in s.layers:
                assert torch.isfinite(L.cache[r, t]).all()
                keep = torch.arange(c["rows"], device="cuda") != t
                same_bits(L.cache[r][keep], L.cache_before[r][keep], f"{name} cache rows of sequence {r} other than t0")
        else:
            assert torch.isnan(s.out[r]).all()
            for L in s.layers:
                same_bits(L.cache[r], L.cache_before[r], f"{name} cache of inactive sequence {r}")
            for k, v in reg.items():
                if not k.endswith("_pad"):
                    assert (v[r].contiguous().view(torch.uint8) == 0xFF).all(), (name, "workspace row of an inactive row written", k, r)
    assert (reg["lse_pad"] == 0xFF).all()
    assert (s.wsbuf[:FENCE] == 0xFF).all() and (s.wsbuf[FENCE + s.ws_bytes:] == 0xFF).all(), "write outside the workspace"
    from gpu_checks import clean as _clean
    _clean(s.xbuf, s.x, name + " x")
    _clean(s.obuf, s.out, name + " out")
    for L in s.layers:
        _clean(L.cache_buf, L.cache, name + " cache")


def test_step_wide_attention_over_chunk_0s_caches_is_caught(kl):
    """The seeded defect of the sequencer: the attention chunk offset applied to q / out but NOT to the cache, i.e. rows 32 .. 47
    attend over the caches of rows 0 .. 15.  Modelled with the _rows step of chunk 2 (its x and t0) on copies of chunk 0's
    caches; t0 repeats every 16 rows, so those caches hold exactly as many keys as the rows expect and nothing is NaN.  The bit
    comparison of the test above rejects it, and so does the fp64 attention check of test_decode_rows_gpu.stages (the last
    layer's `ao` from the q and cache the wide step left), by more than WRONG_MARGIN allowances"""
    import kernel_refs as kr
    ops, lib = kl
    c = wc.step_case("hd64", 64)
    c["t0"] = tuple((7 * (r % 16)) % 38 for r in range(64))
    s = Step(lib, c)
    assert s.step() == 0
    reg = regions(s.ws, 64, s.D, c["H"], c["inner"])
    good, _, greg = s.rows_step(32)
    bad, _, breg = s.rows_step(32, caches_of=0)
    same_bits(s.out[32:48], good, "right chunk")
    same_bits(reg["ao"][32:48], greg["ao"], "right chunk ao")
    assert torch.isfinite(bad).all()
    for r in range(1, 16):                                  # (row 32 has t0 = 0: its one key is the one the step itself appends)
        assert not torch.equal(_bits(s.out[32 + r]), _bits(bad[r])), r
        assert not torch.equal(_bits(reg["ao"][32 + r]), _bits(breg["ao"][r])), r
    hd, H, Hkv, L, w = c["hd"], c["H"], c["Hkv"], s.layers[-1], c["Hkv"] * c["hd"]
    for r in (32, 41, 47):
        n = c["t0"][r] + 1
        cache = L.cache[r].double()
        ao, lse, p, qh, kh = kr.attention_ref(reg["q"][r].double()[None, None, :], cache[None, :n, :w], cache[None, :n, w:], H, Hkv, hd, rot=hd,
                                              cos=s.cos.double(), sin=s.sin.double(), causal=True, round_points=True)
        u_out, _ = kr.attention_fwd_units(p, qh, kh, cache[None, :n, w:], ao, lse, H, Hkv, hd)
        ref, tol = ao.reshape(-1), tr.ATTN_ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1)
        check(reg["ao"][r], ref, tol, f"row {r} ao: right reference")
        if n > 1:                                           # (one key: softmax over one score, any cache gives v of the row itself)
            assert ((breg["ao"][r - 32].double() - ref).abs() / tol).max().item() > WRONG_MARGIN, r
            with pytest.raises(AssertionError, match="out of bound"):
                check(breg["ao"][r - 32], ref, tol, f"row {r} ao over chunk 0's cache")


def test_step_wide_refusals_leave_everything_untouched(kl):
    ops, lib = kl
    s = Step(lib, wc.step_case("hd64", 33))
    t0 = s.c["t0"]
    for over in (dict(R=0), dict(R=65, t0=(0,) * 65), dict(t0=(40,) + t0[1:]), dict(t0=t0[:32] + (40,)), dict(Hkv=3), dict(inner=12), dict(hd=32),
                 dict(H=513)):
        assert s.step(**over) == ERR_ARG, over
        assert ops.attn_last_plan() == 0, over
    s.arr[1].wug = None                                    # a NULL in the second layer
    assert s.step() == ERR_ARG
    s.untouched("refused calls")
