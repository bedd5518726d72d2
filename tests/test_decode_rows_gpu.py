"""-m gpu: the batched decode path - gemm_rows_kernel at NCB = 1 / rows_prologue_kernel (kalle_gemm_rows_bf16, kalle_gemm_rows_fused),
the per-row single-query attention (kalle_attention_decode_rows) and kalle_llama_decode_step_rows - element by element against
the fp64 references of tests/kernel_refs.py, by the method of tests/test_decode_gpu.py: each stage from its own inputs as the
kernel produced them, NaN-guarded buffers and a fenced workspace, untouched memory compared bit for bit, wrong references caught.

Bounds (those of test_decode_gpu.py, nothing new measured): a GEMM output gets K 2^-24 sum_k |W_nk| |xhat_rk| (an fp32 dot in any
order - the MFMA's, then the four waves' partials) + 4 x 2^-24 (|residual| + that sum) + 2^-8 |ref| where stored as bf16, plus
|W_nk| ulp_bf16(xhat_rk) for the ambiguous prologue elements (capped at 1 % of K, asserted here on the values the kernel saw and
in tests/test_decode_rows_cpu.py for the committed inputs).  Attention takes the single-query allowances of
tests/test_attention_gpu.py.  An INACTIVE row's buffers hold NaN (inputs) / their fill (outputs) and must come back bit for bit."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
import decode_cases as dc  # noqa: E402
import decode_rows_cases as rc  # noqa: E402
import kernel_refs as kr  # noqa: E402
import test_decode_gpu as td  # noqa: E402
from gpu_checks import NAN, U, Guard, _bits, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402
from test_attention_gpu import ALLOW as ATTN_ALLOW  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FENCE = 64
BF, F32 = torch.bfloat16, torch.float32
P = td.P


def rows_plan(hd, rot):
    """kalle_attn_last_plan: family 7 (fwd_decode_rows), head dim, ROT"""
    return 7 | hd << 8 | rot << 17


def iarr(vals, ty=ctypes.c_int32):
    return ctypes.cast((ty * len(vals))(*vals), ctypes.c_void_p)


def same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), (what, "not bit for bit")


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


# ------------------------------------------------------------------------------------------------ skinny GEMM
class Gemm:
    def __init__(self, lib, N, K, nsplit, R, pro, f32, with_res, inactive=()):
        self.a = (N, K, nsplit, R, pro, f32, with_res, tuple(inactive))
        xin, gamma = rc.gemm_inputs(N, K, R, pro)
        cols = 2 * K if pro == rc.PRO_SWIGLU else K
        self.X = Guard(R, cols, ld=cols + 8, dtype=F32 if pro == rc.PRO_RMS else BF, init=xin.cuda())   # row stride > K
        for r in inactive:
            self.X.v[r] = NAN
        self.gamma = gamma.cuda() if gamma is not None else None
        g = torch.Generator(device="cuda").manual_seed(N * K + R)
        self.W = Guard(N, K, ld=K + 8, dtype=BF, init=torch.randn((N, K), generator=g, device="cuda") / K ** 0.5)
        ydt = F32 if f32 else BF
        self.Y = Guard(R, nsplit, ld=nsplit + 5, dtype=ydt)
        self.n2 = N - nsplit
        self.y2 = torch.full((R, 3, max(self.n2, 1)), NAN, device="cuda", dtype=ydt)     # row r's destination: y2[r][1]
        self.res = torch.randn((R, N), generator=g, device="cuda") if with_res else None
        for r in inactive if with_res else ():
            self.res[r] = NAN
        self.hbuf, self.xhat = _guarded(torch.full((R, K), NAN, device="cuda", dtype=BF))
        self.rc = lib.kalle_gemm_rows_fused(
            P(self.X.v), cols + 8, pro, P(self.gamma), ctypes.c_float(rc.EPS), P(self.xhat), P(self.W.v), K + 8, P(self.Y.v), nsplit + 5,
            1 if f32 else 0, P(self.y2) if self.n2 else None, nsplit, iarr([(3 * r + 1) * self.n2 for r in range(R)], ctypes.c_int64) if self.n2 else None,
            P(self.res), N if with_res else 0, iarr([0 if r in inactive else 1 for r in range(R)]), R, N, K, None)
        torch.cuda.synchronize()

    def operand(self, r):
        """(bf16 operand of row r as fp64, ulps of its ambiguous elements) from the input the kernel read"""
        K, pro = self.a[1], self.a[4]
        if pro == rc.PRO_BF16:
            return self.X.v[r].double(), None
        if pro == rc.PRO_RMS:
            xh = kr.decode_rms_prologue(self.X.v[r].double(), self.gamma.double(), rc.EPS)
            return td.prologue(xh, dc.rms_window(xh), f"rms row {r}")
        h = self.X.v[r].double()
        return td.prologue(kr.decode_swiglu_prologue(h), dc.swiglu_window(h), f"swiglu row {r}")

    def ref(self, r, x_row=None, res_row=None):
        N, K, nsplit, R, pro, f32, with_res, _ = self.a
        xr, au = self.operand(r if x_row is None else x_row)
        rr = r if res_row is None else res_row
        return td.gemv_ref(self.W.v, xr, K, res=self.res[rr].double() if with_res else None, bf16_out=not f32, amb_ulp=au)

    def got(self, r):
        return torch.cat([self.Y.v[r], self.y2[r, 1, :self.n2]]) if self.n2 else self.Y.v[r]

    def verify(self, lib):
        N, K, nsplit, R, pro, f32, with_res, inactive = self.a
        what = f"gemm_rows N {N} K {K} R {R} pro {pro} {'f32' if f32 else 'bf16'} res {with_res}"
        assert self.rc == 0, (what, self.rc, lib.kalle_last_error())
        for r in range(R):
            if r in inactive:
                assert torch.isnan(self.Y.v[r]).all() and torch.isnan(self.y2[r]).all() and torch.isnan(self.xhat[r]).all(), (what, "inactive row written", r)
                continue
            ref, tol = self.ref(r)
            check(self.got(r), ref, tol, f"{what} row {r}")
            assert torch.isnan(self.y2[r, 0]).all() and torch.isnan(self.y2[r, 2]).all(), (what, "stray write next to the second destination")
            if not self.n2:
                assert torch.isnan(self.y2[r]).all()
            assert torch.isfinite(self.xhat[r]).all() if pro != rc.PRO_BF16 else torch.isnan(self.xhat[r]).all(), (what, "xhat", r)
        self.Y.clean(what + " y")
        self.X.clean(what + " x")
        self.W.clean(what + " W")
        _clean(self.hbuf, self.xhat, what + " xhat")


@pytest.mark.parametrize("pro", [rc.PRO_BF16, rc.PRO_RMS, rc.PRO_SWIGLU], ids=["bf16", "rms", "swiglu"])
@pytest.mark.parametrize("R", rc.GEMM_ROWS)
@pytest.mark.parametrize("N,K,nsplit", rc.GEMM_SHAPES + rc.GEMM_TILE_SHAPES)
def test_gemm_rows_every_element(kl, N, K, nsplit, R, pro):
    """fp32 and bf16 outputs, with and without residual; X, W and Y with row strides larger than their widths"""
    ops, lib = kl
    for f32 in (True, False):
        for with_res in (False, True):
            Gemm(lib, N, K, nsplit, R, pro, f32, with_res).verify(lib)


@pytest.mark.parametrize("pro", [rc.PRO_BF16, rc.PRO_RMS, rc.PRO_SWIGLU], ids=["bf16", "rms", "swiglu"])
@pytest.mark.parametrize("R,dead", [(3, 1), (16, 7)])
@pytest.mark.parametrize("N,K,nsplit", rc.GEMM_SHAPES)
def test_gemm_rows_inactive_row_in_the_middle(kl, N, K, nsplit, R, dead, pro):
    """its x and residual rows are NaN (never read); its y row, second destination and xhat row come back bit for bit"""
    ops, lib = kl
    for f32 in (True, False):
        g = Gemm(lib, N, K, nsplit, R, pro, f32, True, inactive=(dead,))
        g.verify(lib)
        fill = torch.full_like(g.Y.v[dead], NAN)
        same_bits(g.Y.v[dead], fill, "inactive y row")
        same_bits(g.y2[dead], torch.full_like(g.y2[dead], NAN), "inactive second destination")
        same_bits(g.xhat[dead], torch.full_like(g.xhat[dead], NAN), "inactive xhat row")


def test_gemm_rows_public_entry_and_wrapper(kl):
    """kalle_gemm_rows_bf16 through ops.gemm_rows: strided x rows, residual, both output types"""
    ops, lib = kl
    g = torch.Generator(device="cuda").manual_seed(5)
    W = (torch.randn((264, 1000), generator=g, device="cuda") / 1000 ** 0.5).to(BF)
    xfull = torch.randn((5, 1016), generator=g, device="cuda").to(BF)
    res = torch.randn((5, 264), generator=g, device="cuda")
    for dt, r in ((F32, res), (BF, None)):
        y = ops.gemm_rows(xfull[:, :1000], W, residual=r, out_dtype=dt)
        torch.cuda.synchronize()
        for i in range(5):
            ref, tol = td.gemv_ref(W, xfull[i, :1000].double(), 1000, res=r[i].double() if r is not None else None, bf16_out=dt == BF)
            check(y[i], ref, tol, f"ops.gemm_rows row {i}")


def test_gemm_rows_refusals_write_nothing(kl):
    ops, lib = kl
    W = torch.zeros((70, 32776), device="cuda", dtype=BF)
    x = torch.zeros((16, 32776), device="cuda", dtype=BF)
    y = torch.full((16, 70), NAN, device="cuda")
    for R, K in ((0, 64), (17, 64), (3, 60), (3, 32776)):
        assert lib.kalle_gemm_rows_bf16(P(x), 32776, P(W), 32776, P(y), 70, 1, None, 0, R, 70, K, None) == ERR_ARG, (R, K)
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ------------------------------------------------------------------------------------------------ attention rows
class Attn:
    H, Hkv = 4, 2

    def __init__(self, lib, hd, rot, nk, twins=None):
        H, Hkv = self.H, self.Hkv
        self.hd, self.rot, self.nk = hd, rot, nk
        R, D, kvw, mx = len(nk), H * hd, 2 * Hkv * hd, max(nk)
        self.D, self.kvw, self.rows = D, kvw, mx + 3                   # kv_row_stride = (max(nk) + 3) ldk
        g = torch.Generator(device="cuda").manual_seed(1000 * hd + rot + sum(nk))
        q = torch.randn((R, D), generator=g, device="cuda").to(BF)
        cache = torch.full((R, self.rows, kvw), NAN, device="cuda", dtype=BF)
        for r, n in enumerate(nk):
            if n > 0:
                cache[r, :n] = (torch.randn((n, kvw), generator=g, device="cuda") * 0.8).to(BF)
            else:
                q[r] = NAN
        if twins:
            q[twins[1]], cache[twins[1]] = q[twins[0]], cache[twins[0]]
        self.qbuf, self.q = _guarded(q)
        self.cbuf, self.cache = _guarded(cache)
        self.before = self.cache.clone()
        self.cos = self.sin = None
        if rot:
            cos, sin = rc.rope_tables(mx + 2, hd)
            cos[mx:], sin[mx:] = NAN, NAN
            self.cos, self.sin = cos.cuda(), sin.cuda()
        self.obuf, self.out = _guarded(torch.full((R, D), NAN, device="cuda", dtype=BF))
        self.lbuf, self.lse = _guarded(torch.full((R, H), NAN, device="cuda"))
        a = (P(self.q), D, 0, P(self.cache), kvw, 0, P(self.cache), kvw, Hkv * hd, self.rows * kvw,
             P(self.out), D, P(self.lse), P(self.cos), P(self.sin), rot, iarr(nk), R, H, Hkv, hd)
        self.asked = ac.query(lib, "rows", a)              # (return code, plan ints) of the host query, before the call
        self.rc = lib.kalle_attention_decode_rows(*a, None)
        torch.cuda.synchronize()

    def ref(self, r, keys=None):
        """(out ref, out tol, lse ref, lse tol) of row r in fp64 from the kernel's inputs"""
        H, Hkv, hd = self.H, self.Hkv, self.hd
        n, w = self.nk[r] if keys is None else keys, Hkv * hd
        c = self.cache[r].double()
        kw = dict(rot=self.rot, cos=self.cos.double(), sin=self.sin.double()) if self.rot else {}
        ao, lse, p, qh, kh = kr.attention_ref(self.q[r].double()[None, None, :], c[None, :n, :w], c[None, :n, w:], H, Hkv, hd, causal=True,
                                              round_points=True, **kw)
        u_out, u_lse = kr.attention_fwd_units(p, qh, kh, c[None, :n, w:], ao, lse, H, Hkv, hd)
        return (ao.reshape(-1), ATTN_ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1), lse.reshape(-1),
                ATTN_ALLOW["lse/decode"] * U * u_lse.reshape(-1))


@pytest.mark.parametrize("nk", rc.ATTN_NK, ids=lambda v: "nk" + "-".join(map(str, v)))
@pytest.mark.parametrize("hd,rot", rc.ATTN_HEADS)
def test_attention_rows(kl, hd, rot, nk):
    ops, lib = kl
    twins = (0, 2) if nk[0] == nk[2] else None
    a = Attn(lib, hd, rot, nk, twins)
    what = f"attention rows hd {hd} rot {rot} nk {nk}"
    assert a.rc == 0, (what, a.rc, lib.kalle_last_error())
    assert ops.attn_last_plan() == rows_plan(hd, rot), hex(ops.attn_last_plan())
    assert a.asked[0] == 0 and a.asked[1][0] == ops.attn_last_plan(), a.asked
    H, Hkv = a.H, a.Hkv
    for r, n in enumerate(nk):
        if n <= 0:
            same_bits(a.out[r], torch.full_like(a.out[r], NAN), what + " inactive out row")
            same_bits(a.lse[r], torch.full_like(a.lse[r], NAN), what + " inactive lse row")
            continue
        ro, to, rl, tl = a.ref(r)
        check(a.out[r], ro, to, f"{what} out row {r}")
        check(a.lse[r], rl, tl, f"{what} lse row {r}")
        # the row alone through kalle_attention_decode_hd: inside the same bound of the fp64 reference, and the two within ONE
        # allowance of each other (the same statements; two results that are each only inside their bound could be two apart)
        o1 = torch.full((1, a.D), NAN, device="cuda", dtype=BF)
        l1 = torch.full((1, H), NAN, device="cuda")
        assert lib.kalle_attention_decode_hd(P(a.q[r]), a.D, 0, P(a.cache[r]), a.kvw, 0, P(a.cache[r]), a.kvw, Hkv * hd, P(o1), a.D, P(l1),
                                             P(a.cos), P(a.sin), rot, None, 1, H, Hkv, n, hd, None) == 0
        torch.cuda.synchronize()
        check(o1[0], ro, to, f"{what} decode_hd out row {r}")
        check(a.out[r], o1[0].double(), to, f"{what} rows vs decode_hd out row {r}")
        check(a.lse[r], l1[0].double(), tl, f"{what} rows vs decode_hd lse row {r}")
    if twins:
        same_bits(a.out[0], a.out[2], what + " equal rows around an inactive one")
        same_bits(a.lse[0], a.lse[2], what + " equal rows around an inactive one (lse)")
    same_bits(a.cache, a.before, what + " cache")
    for buf, v, n in ((a.qbuf, a.q, "q"), (a.cbuf, a.cache, "cache"), (a.obuf, a.out, "out"), (a.lbuf, a.lse, "lse")):
        _clean(buf, v, f"{what} {n}")


def test_attention_rows_refusals(kl):
    ops, lib = kl
    a = Attn(lib, 64, 64, (1, 2, 3))
    assert ops.attn_last_plan() == rows_plan(64, 64)
    assert a.asked[0] == 0 and a.asked[1][0] == ops.attn_last_plan(), a.asked
    H, Hkv, hd = a.H, a.Hkv, 64
    out = torch.full_like(a.out, NAN)

    def call(nk, R=None, rot=64, head_dim=64):
        return lib.kalle_attention_decode_rows(P(a.q), a.D, 0, P(a.cache), a.kvw, 0, P(a.cache), a.kvw, Hkv * hd, a.rows * a.kvw, P(out), a.D,
                                               None, P(a.cos), P(a.sin), rot, iarr(nk), len(nk) if R is None else R, H, Hkv, head_dim, None)

    for kw in (dict(nk=[1, 15361, 2]), dict(nk=[1], R=0), dict(nk=[1] * 17), dict(nk=[1, 2, 3], rot=32), dict(nk=[1, 2, 3], head_dim=32)):
        assert call(**kw) == ERR_ARG, kw
        assert ops.attn_last_plan() == 0, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ the step
class Layer:
    def __init__(self, c, g, index):
        hd, H, Hkv, inner, t0, rows = c["hd"], c["H"], c["Hkv"], c["inner"], c["t0"], c["rows"]
        D, kvw = hd * H, 2 * hd * Hkv
        cpu = torch.Generator().manual_seed(c["seed"] + 1000 + index)
        self.input_norm = (rc.step_inputs(c)[1] if index == 0 else 1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.post_norm = (1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.wqkv, self.wo = td.dev_weight(D + kvw, D, g), td.dev_weight(D, D, g)
        self.wug, self.wdown = td.dev_weight(2 * inner, D, g), td.dev_weight(D, inner, g)
        cache = torch.full((len(t0), rows, kvw), NAN, device="cuda", dtype=BF)
        for r, t in enumerate(t0):
            n = t if t >= 0 else 5            # (an inactive sequence keeps what it had: 5 rows of data, NaN above)
            cache[r, :n] = (torch.randn((n, kvw), generator=g, device="cuda") * 0.8).to(BF)
        self.cache_buf, self.cache = _guarded(cache)
        self.cache_before = self.cache.clone()

    def fields(self):
        return [self.input_norm, self.wqkv, self.wo, self.post_norm, self.wug, self.wdown, self.cache]


class Setup:
    def __init__(self, lib, c, n_layers=1):
        from kalle_audio_amd import _lib
        self.c, self.lib = c, lib
        hd, H, Hkv, inner, t0 = c["hd"], c["H"], c["Hkv"], c["inner"], c["t0"]
        self.R, self.D = len(t0), hd * H
        g = torch.Generator(device="cuda").manual_seed(c["seed"])
        self.layers = [Layer(c, g, i) for i in range(n_layers)]
        self.arr = (_lib.LlamaLayer * n_layers)()
        for d, L in zip(self.arr, self.layers):
            d.input_norm, d.wqkv, d.wo, d.post_norm, d.wug, d.wdown, d.kv_cache = (t.data_ptr() for t in L.fields())
        x = rc.step_inputs(c)[0].cuda()
        for r, t in enumerate(t0):
            if t < 0:
                x[r] = NAN
        self.xbuf, self.x = _guarded(x)
        self.obuf, self.out = _guarded(torch.full((self.R, self.D), NAN, device="cuda"))
        cos, sin = rc.rope_tables(c["rows"], hd)
        cos[max(t0) + 1:], sin[max(t0) + 1:] = NAN, NAN
        self.cos, self.sin = cos.cuda(), sin.cuda()
        self.ws_bytes = lib.kalle_llama_decode_ws_bytes_rows(self.R, H, Hkv, inner, hd)
        assert self.ws_bytes == rc.ws_bytes(self.R, H, inner, hd)
        self.wsbuf = torch.full((self.ws_bytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)   # all-ones bytes: NaN as fp32 and as bf16
        self.ws = self.wsbuf[FENCE:FENCE + self.ws_bytes]
        assert self.ws.data_ptr() % 64 == 0

    def step(self, **over):
        c = self.c
        a = dict(R=self.R, H=c["H"], Hkv=c["Hkv"], inner=c["inner"], hd=c["hd"], t0=c["t0"], rows=c["rows"])
        a.update(over)
        rcode = self.lib.kalle_llama_decode_step_rows(ctypes.cast(self.arr, ctypes.c_void_p), len(self.layers), P(self.x), P(self.out), a["R"],
                                                      a["H"], a["Hkv"], a["inner"], a["hd"], ctypes.c_float(rc.EPS), iarr(list(a["t0"])),
                                                      a["rows"], P(self.cos), P(self.sin), P(self.ws), None)
        torch.cuda.synchronize()
        return rcode

    def regions(self):
        """the workspace as the header lays it out, each region [R][...]"""
        R, D, H, inner = self.R, self.D, self.c["H"], self.c["inner"]
        o, out = 0, {}
        for name, n, pad, dt in (("x2", D, 0, F32), ("x3", D, 0, F32), ("lse", H, 1, F32), ("q", D, 0, BF), ("ao", D, 0, BF),
                                 ("hf", 2 * inner, 0, BF), ("xn", max(D, inner), 0, BF)):
            nb = R * n * (4 if dt == F32 else 2)
            out[name] = self.ws[o:o + nb].view(dt).view(R, n)
            if pad:
                out[name + "_pad"] = self.ws[o + nb:o + ((nb + 63) & ~63)]
                nb = (nb + 63) & ~63
            o += nb
        assert o == self.ws_bytes
        return out

    def fences_clean(self, what):
        assert (self.wsbuf[:FENCE] == 0xFF).all() and (self.wsbuf[FENCE + self.ws_bytes:] == 0xFF).all(), (what, "write outside the workspace")
        _clean(self.xbuf, self.x, what + " x")
        _clean(self.obuf, self.out, what + " out")
        for L in self.layers:
            _clean(L.cache_buf, L.cache, what + " cache")


def stages(s, L, r, x, out, wrong=None):
    """the five stages of test_decode_gpu.stages for row r (x: its layer input, out: its layer output), each from the kernel's own
    inputs; `wrong`: "other_row_residual" (stage 3 adds another row's x), "one_key_short" (attention over t0 keys)"""
    c, D = s.c, s.D
    hd, H, Hkv, t0 = c["hd"], c["H"], c["Hkv"], c["t0"][r]
    ws = {k: v[r].clone() for k, v in s.regions().items() if not k.endswith("_pad")}
    res = []
    xh = kr.decode_rms_prologue(x.double(), L.input_norm.double(), rc.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 1")
    ref, tol = td.gemv_ref(L.wqkv, xr, D, bf16_out=True, amb_ulp=au)
    res.append(("q | k | v", torch.cat([ws["q"], L.cache[r, t0]]), ref, tol))
    w = Hkv * hd
    cache = L.cache[r].double()
    n = t0 if wrong == "one_key_short" else t0 + 1
    ao, lse, p, qh, kh = kr.attention_ref(ws["q"].double()[None, None, :], cache[None, :n, :w], cache[None, :n, w:], H, Hkv, hd, rot=hd,
                                          cos=s.cos.double(), sin=s.sin.double(), causal=True, round_points=True)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, cache[None, :n, w:], ao, lse, H, Hkv, hd)
    res.append(("ao", ws["ao"], ao.reshape(-1), ATTN_ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1)))
    res.append(("lse", ws["lse"], lse.reshape(-1), ATTN_ALLOW["lse/decode"] * U * u_lse.reshape(-1)))
    ref, tol = td.gemv_ref(L.wo, ws["ao"].double(), D, res=(s.x[0] if wrong == "other_row_residual" else x).double())
    res.append(("x2", ws["x2"], ref, tol))
    xh = kr.decode_rms_prologue(ws["x2"].double(), L.post_norm.double(), rc.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 4")
    ref, tol = td.gemv_ref(L.wug, xr, D, bf16_out=True, amb_ulp=au)
    res.append(("hf", ws["hf"], ref, tol))
    hf = ws["hf"].double()
    ar, au = td.prologue(kr.decode_swiglu_prologue(hf), dc.swiglu_window(hf), "stage 5")
    ref, tol = td.gemv_ref(L.wdown, ar, c["inner"], res=ws["x2"].double(), amb_ulp=au)
    res.append(("out", out, ref, tol))
    return res


def untouched(s, name, n_layers):
    """everything an inactive row owns, every cache row but t0[r] of an active one, x3 of a one-layer call, the lse padding"""
    c = s.c
    reg = s.regions()
    for r, t in enumerate(c["t0"]):
        for L in s.layers:
            keep = torch.arange(c["rows"], device="cuda") != t
            same_bits(L.cache[r][keep], L.cache_before[r][keep], f"{name} cache rows of sequence {r} other than t0")
        if t < 0:
            assert torch.isnan(s.out[r]).all(), (name, "out row of an inactive row written")
            for k, v in reg.items():
                if not k.endswith("_pad"):
                    assert (v[r].contiguous().view(torch.uint8) == 0xFF).all(), (name, "workspace row of an inactive row written", k)
    if n_layers == 1:
        assert (reg["x3"].contiguous().view(torch.uint8) == 0xFF).all(), (name, "x3 written by a one-layer call")
    assert (reg["lse_pad"] == 0xFF).all(), (name, "lse padding written")
    s.fences_clean(name)


@pytest.fixture(scope="module")
def step_runs(kl):
    ops, lib = kl
    runs = {}
    for name, c in rc.STEP_CASES.items():
        s = Setup(lib, c)
        assert s.step() == 0, (name, lib.kalle_last_error())
        assert ops.attn_last_plan() == rows_plan(c["hd"], c["hd"]), hex(ops.attn_last_plan())
        assert ac.step_word(lib, c["hd"], c["H"], c["Hkv"], c["t0"], c["rows"]) == ops.attn_last_plan()
        runs[name] = s
    return runs


@pytest.mark.parametrize("name", list(rc.STEP_CASES))
def test_step_rows_stage_by_stage(step_runs, name):
    s = step_runs[name]
    for r, t in enumerate(s.c["t0"]):
        if t >= 0:
            assert torch.isfinite(s.out[r]).all(), (name, r, "NaN rows above t0 leaked into the output")
            for stage, got, ref, tol in stages(s, s.layers[0], r, s.x[r], s.out[r]):
                check(got, ref, tol, f"{name} row {r} {stage}")
    untouched(s, name, 1)


def test_step_rows_two_layers_hand_x3_over(kl):
    """the last layer's stages from x3 (the first layer's output), per row; the inactive row untouched in both layers"""
    ops, lib = kl
    c = rc.STEP_CASES["hd64"]
    s = Setup(lib, c, 2)
    assert s.step() == 0
    x3 = s.regions()["x3"].clone()
    for r, t in enumerate(c["t0"]):
        if t >= 0:
            assert torch.isfinite(x3[r]).all() and torch.isfinite(s.out[r]).all()
            for stage, got, ref, tol in stages(s, s.layers[1], r, x3[r], s.out[r]):
                check(got, ref, tol, f"two layers, last layer, row {r} {stage}")
            assert torch.isfinite(s.layers[0].cache[r, t]).all()
    untouched(s, "two layers", 2)


def test_step_rows_refusals_leave_everything_untouched(kl):
    ops, lib = kl
    s = Setup(lib, rc.STEP_CASES["hd64"])
    for over in (dict(R=0), dict(R=17, t0=(0,) * 17), dict(Hkv=3), dict(inner=12), dict(t0=(0, 40, -1)), dict(hd=32), dict(H=513)):
        assert s.step(**over) == ERR_ARG, over
        assert ops.attn_last_plan() == 0, over
    assert (s.wsbuf == 0xFF).all() and torch.isnan(s.out).all()
    same_bits(s.layers[0].cache, s.layers[0].cache_before, "cache after refused calls")


WRONG_MARGIN = 2.0


def test_wrong_references_are_caught(kl, step_runs):
    """each wrong reference moves some element by more than WRONG_MARGIN x its allowance and fails the check the right one passes"""
    ops, lib = kl
    cases = []
    g = Gemm(lib, 264, 1000, 264, 3, rc.PRO_RMS, True, True)
    (ref, tol), (wref, _) = g.ref(1), g.ref(1, x_row=2)
    cases.append(("gemm: another row's operand", g.got(1), ref, tol, wref))
    cases.append(("gemm: another row's residual", g.got(1), ref, tol, g.ref(1, res_row=0)[0]))
    a = Attn(lib, 128, 128, (1, 257, 130))
    ro, to, _, _ = a.ref(1)
    cases.append(("attention: another row's key count", a.out[1], ro, to, a.ref(1, keys=130)[0]))
    s = step_runs["hd64"]
    for wrong, stage in (("other_row_residual", "x2"), ("one_key_short", "ao")):
        right = {k: (g_, r_, t_) for k, g_, r_, t_ in stages(s, s.layers[0], 1, s.x[1], s.out[1])}
        bad = {k: r_ for k, _, r_, _ in stages(s, s.layers[0], 1, s.x[1], s.out[1], wrong=wrong)}
        cases.append(("step: " + wrong, *right[stage], bad[stage]))
    for what, got, ref, tol, wref in cases:
        check(got, ref, tol, what + ": right reference")
        assert ((wref - ref).abs() / tol).max().item() > WRONG_MARGIN, what
        with pytest.raises(AssertionError, match="out of bound"):
            check(got, wref, tol, what)
