"""-m gpu: the weight-only e4m3 decode path (csrc/llasa.hip: quantize_rows_e4m3_kernel, gemv_e4m3_kernel, gemm_rows_e4m3_kernel,
kalle_llama_decode_step_w8 / _rows_w8) by the method of tests/test_decode_gpu.py and tests/test_decode_rows_gpu.py.

Quantiser: codes and scales bit for bit against the CPU reference of tests/fp8_refs.py (checked by tests/test_fp8_refs_cpu.py).

GEMV, skinny GEMM and every GEMV stage of the two steps: every element against fp64 with W replaced by scale[n] * table[code].
The bound is the one test_decode_gpu.py states - K 2^-24 sum_k |w_nk| |xhat_k| (an fp32 dot product in any order) + 4 x 2^-24
(|residual| + that sum) + 2^-8 |ref| where stored as bf16 + |w_nk| ulp_bf16(xhat_k) for the ambiguous prologue elements (capped
at 1 % of K, asserted on the values the kernel saw) - plus ONE more 2^-24 sum_k |w_nk x_k| for the multiply by scale[n].  Derived,
not measured: e4m3 (4 significant bits) times bf16 (8) is exact in fp32, so only the summation order and that one rounding differ.
Each stage of a step is checked from that stage's own inputs as the kernel left them in the published workspace."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as dc  # noqa: E402
import decode_w8_cases as wc  # noqa: E402
import fp8_refs as f8  # noqa: E402
import kernel_refs as kr  # noqa: E402
import llama_hd128_cases as lc128  # noqa: E402
import test_decode_gpu as td  # noqa: E402
import test_decode_rows_gpu as tr  # noqa: E402
from gpu_checks import NAN, U, Guard, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402
from test_attention_gpu import ALLOW as ATTN_ALLOW  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG = -1
F32_EPS = td.F32_EPS
BF, F32 = torch.bfloat16, torch.float32
P, iarr, same_bits = td.P, tr.iarr, tr.same_bits
SEEN = set()
NAN_CODE = 0x7F
GEMV_STAGES = ("q | k | v", "x2", "hf", "out")


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


@pytest.fixture(scope="module")
def table():
    return f8.decode_table().cuda()


def dequant(codes, scale, tab):
    """scale[n] * table[code] in fp64, by chunks of rows (the largest weight here has 1.1e9 elements)"""
    out = torch.empty(codes.shape, device=codes.device, dtype=torch.float64)
    for r in range(0, codes.shape[0], td.CHUNK):
        out[r:r + td.CHUNK] = tab[codes[r:r + td.CHUNK].long()] * scale[r:r + td.CHUNK].double()[:, None]
    return out


def gemv8_ref(Wdq, xr, K, **kw):
    """test_decode_gpu.gemv_ref on the dequantised weights, plus 2^-24 sum_k |w_nk x_k| for the scale multiply"""
    ref, tol = td.gemv_ref(Wdq, xr, K, **kw)
    extra = torch.cat([Wdq[r:r + td.CHUNK].abs() @ xr.abs() for r in range(0, Wdq.shape[0], td.CHUNK)])
    return ref, tol + F32_EPS * extra


class W8:
    """codes [N][K] inside a [N + 2][ldq] buffer whose every other byte is the NaN code: a read outside the window poisons the
    output"""

    def __init__(self, N, K, pad, seed):
        codes, scale = wc.weights(N, K, seed)
        self.buf = torch.full((N + 2, K + pad), NAN_CODE, device="cuda", dtype=torch.uint8)
        self.buf[:N, :K] = codes.cuda()
        self.v, self.ld = self.buf[:N, :K], K + pad
        self.sbuf, self.scale = _guarded(scale.cuda())


# ------------------------------------------------------------------------------------------------ quantiser
def quant_inputs(N, K, kind):
    g = torch.Generator().manual_seed(31 * N + K)
    if kind == "lossless":
        return f8.lossless_weights(N, K, g)[0]
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(BF)
    if kind == "zero-and-single":
        w[0] = 0
        w[N - 1] = 0
        w[N - 1, K // 3] = -0.37
    return w


@pytest.mark.parametrize("kind", ["normal", "zero-and-single", "lossless"])
@pytest.mark.parametrize("N,K,padw,padq", wc.QUANT_SHAPES)
def test_quantiser_bit_for_bit(kl, N, K, padw, padq, kind):
    """N = 1, N no multiple of the 4 rows of a workgroup, ldw > K, ldq > K; an all-zero row, a row with one non-zero; nothing
    written outside [N][K] of W8 (0xAA fences) or [N] of scale"""
    ops, lib = kl
    w = quant_inputs(N, K, kind)
    Wg = Guard(N, K, ld=K + padw, dtype=BF, init=w.cuda())
    q = torch.full((N + 2, K + padq), 0xAA, device="cuda", dtype=torch.uint8)
    sbuf, scale = _guarded(torch.full((N,), NAN, device="cuda"))
    rc = lib.kalle_quantize_rows_e4m3(P(Wg.v), K + padw, P(q), K + padq, P(scale), N, K, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.kalle_last_error())
    codes, sref = f8.quantize_ref(w)
    assert torch.equal(scale.cpu().view(torch.int32), sref.view(torch.int32)), "scales differ from the CPU reference"
    got = q[:N, :K].cpu()
    bad = got != codes
    assert not bad.any(), (int(bad.sum()), "codes differ; first", bad.nonzero()[0].tolist())
    q[:N, :K] = 0xAA
    assert (q == 0xAA).all(), "W8 written outside [N][K]"
    _clean(sbuf, scale, "scale")
    if kind == "lossless":
        _, c0, s0 = f8.lossless_weights(N, K, torch.Generator().manual_seed(31 * N + K))
        assert torch.equal(got, c0) and torch.equal(scale.cpu(), s0)
    if kind == "zero-and-single":
        assert int((got[N - 1] != 0).sum()) == 1 and got[N - 1, K // 3].item() == 0xFE
        assert N == 1 or (scale[0].item() == 1.0 and (got[0] == 0).all())
    SEEN.update({"quant-" + kind, f"quant-N{N}"})


def test_ops_quantize_rows_on_a_strided_view(kl):
    ops, lib = kl
    g = torch.Generator().manual_seed(3)
    full = (torch.randn((10, 96), generator=g) / 8).to(BF).cuda()
    w8, s = ops.quantize_rows_e4m3(full[:, :80])
    torch.cuda.synchronize()
    codes, sref = f8.quantize_ref(full[:, :80])
    assert torch.equal(w8.cpu(), codes) and torch.equal(s.cpu(), sref)
    SEEN.add("quant-ops")


# ------------------------------------------------------------------------------------------------ one-row GEMV
@pytest.mark.parametrize("N,K,pad", wc.GEMV_SHAPES)
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_gemv_e4m3_every_element(kl, table, N, K, pad, f32, with_res):
    """N = 1, 7, 9; K = 16 (one load), one load below / at / above a full wave batch of loads, the K limit; N either side of
    both thresholds of rows per workgroup with a ragged last workgroup, at one K batch and at two; ldq > K"""
    ops, lib = kl
    W = W8(N, K, pad, 5 * N + K)
    xbuf, x = _guarded(wc.gemm_inputs(N, K, 1, wc.PRO_BF16)[0][0].cuda())
    g = torch.Generator(device="cuda").manual_seed(N + K)
    res = torch.randn(N, generator=g, device="cuda") if with_res else None
    ybuf, y = _guarded(torch.full((N,), NAN, device="cuda", dtype=F32 if f32 else BF))
    rc = lib.kalle_gemv_e4m3(P(x), P(W.v), W.ld, P(W.scale), P(y), 1 if f32 else 0, P(res), N, K, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.kalle_last_error())
    ref, tol = gemv8_ref(dequant(W.v, W.scale, table), x.double(), K, res=res.double() if with_res else None, bf16_out=not f32)
    check(y, ref, tol, f"gemv_e4m3 N {N} K {K}")
    _clean(ybuf, y, "gemv y")
    SEEN.update({f"gemv-N{N}", f"gemv-K{K}", f"gemv-{N}x{K}"})


def fused_operand(xin, gamma, pro, what):
    if pro == wc.PRO_BF16:
        return xin.double(), None
    if pro == wc.PRO_RMS:
        xh = kr.decode_rms_prologue(xin.double(), gamma.double(), wc.EPS)
        return td.prologue(xh, dc.rms_window(xh), what)
    return td.prologue(kr.decode_swiglu_prologue(xin.double()), dc.swiglu_window(xin.double()), what)


@pytest.mark.parametrize("pro", [wc.PRO_BF16, wc.PRO_RMS, wc.PRO_SWIGLU], ids=["bf16", "rms", "swiglu"])
@pytest.mark.parametrize("N,K,nsplit", wc.GEMV_FUSED_SHAPES)
def test_gemv_e4m3_prologues_and_second_destination(kl, table, N, K, nsplit, pro):
    """each prologue from the input the kernel read; nsplit < N inside a wave's four rows; both output types, with a residual"""
    ops, lib = kl
    W = W8(N, K, 16, 7 * N + K + pro)
    xin, gamma = wc.gemm_inputs(N, K, 1, pro)
    xbuf, x = _guarded(xin[0].cuda())
    gamma = gamma.cuda() if gamma is not None else None
    res = torch.randn(N, generator=torch.Generator(device="cuda").manual_seed(N), device="cuda")
    Wdq = dequant(W.v, W.scale, table)
    n2 = N - nsplit
    for f32 in (True, False):
        dt = F32 if f32 else BF
        ybuf, y = _guarded(torch.full((nsplit,), NAN, device="cuda", dtype=dt))
        y2buf, y2 = _guarded(torch.full((max(n2, 1),), NAN, device="cuda", dtype=dt))
        rc = lib.kalle_gemv_fused_e4m3(P(x), pro, P(gamma), ctypes.c_float(wc.EPS), P(W.v), W.ld, P(W.scale), P(y), 1 if f32 else 0,
                                       P(y2) if n2 else None, nsplit, P(res), N, K, None)
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.kalle_last_error())
        xr, au = fused_operand(x, gamma, pro, f"gemv pro {pro}")
        ref, tol = gemv8_ref(Wdq, xr, K, res=res.double(), bf16_out=not f32, amb_ulp=au)
        check(torch.cat([y, y2[:n2]]) if n2 else y, ref, tol, f"gemv_fused_e4m3 N {N} K {K} pro {pro}")
        _clean(ybuf, y, "y")
        _clean(y2buf, y2, "y2")
        if not n2:
            assert torch.isnan(y2).all()
    _clean(xbuf, x, "x")
    SEEN.update({f"gemv-pro{pro}", "gemv-nsplit" if n2 else "gemv-whole"})


# ------------------------------------------------------------------------------------------------ skinny GEMM
class Gemm:
    """test_decode_rows_gpu.Gemm on e4m3 weights"""

    def __init__(self, lib, tab, N, K, nsplit, R, pro, f32, with_res, inactive=()):
        self.a = (N, K, nsplit, R, pro, f32, with_res, tuple(inactive))
        xin, gamma = wc.gemm_inputs(N, K, R, pro)
        cols = 2 * K if pro == wc.PRO_SWIGLU else K
        self.X = Guard(R, cols, ld=cols + 8, dtype=F32 if pro == wc.PRO_RMS else BF, init=xin.cuda())
        for r in inactive:
            self.X.v[r] = NAN
        self.gamma = gamma.cuda() if gamma is not None else None
        self.W = W8(N, K, 16, N * K + R)
        self.Wdq = dequant(self.W.v, self.W.scale, tab)
        ydt = F32 if f32 else BF
        self.Y = Guard(R, nsplit, ld=nsplit + 5, dtype=ydt)
        self.n2 = N - nsplit
        self.y2 = torch.full((R, 3, max(self.n2, 1)), NAN, device="cuda", dtype=ydt)
        g = torch.Generator(device="cuda").manual_seed(N * K + R)
        self.res = torch.randn((R, N), generator=g, device="cuda") if with_res else None
        for r in inactive if with_res else ():
            self.res[r] = NAN
        self.hbuf, self.xhat = _guarded(torch.full((R, K), NAN, device="cuda", dtype=BF))
        self.rc = lib.kalle_gemm_rows_fused_e4m3(
            P(self.X.v), cols + 8, pro, P(self.gamma), ctypes.c_float(wc.EPS), P(self.xhat), P(self.W.v), self.W.ld, P(self.W.scale),
            P(self.Y.v), nsplit + 5, 1 if f32 else 0, P(self.y2) if self.n2 else None, nsplit,
            iarr([(3 * r + 1) * self.n2 for r in range(R)], ctypes.c_int64) if self.n2 else None, P(self.res), N if with_res else 0,
            iarr([0 if r in inactive else 1 for r in range(R)]), R, N, K, None)
        torch.cuda.synchronize()

    def ref(self, r, x_row=None, W=None):
        N, K, nsplit, R, pro, f32, with_res, _ = self.a
        xr, au = fused_operand(self.X.v[r if x_row is None else x_row], self.gamma, pro, f"row {r}")
        return gemv8_ref(self.Wdq if W is None else W, xr, K, res=self.res[r].double() if with_res else None, bf16_out=not f32, amb_ulp=au)

    def got(self, r):
        return torch.cat([self.Y.v[r], self.y2[r, 1, :self.n2]]) if self.n2 else self.Y.v[r]

    def verify(self, lib):
        N, K, nsplit, R, pro, f32, with_res, inactive = self.a
        what = f"gemm_rows_e4m3 N {N} K {K} R {R} pro {pro} {'f32' if f32 else 'bf16'} res {with_res}"
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
            assert torch.isfinite(self.xhat[r]).all() if pro != wc.PRO_BF16 else torch.isnan(self.xhat[r]).all(), (what, "xhat", r)
        self.Y.clean(what + " y")
        self.X.clean(what + " x")
        _clean(self.hbuf, self.xhat, what + " xhat")


@pytest.mark.parametrize("pro", [wc.PRO_BF16, wc.PRO_RMS, wc.PRO_SWIGLU], ids=["bf16", "rms", "swiglu"])
@pytest.mark.parametrize("R", wc.GEMM_ROWS)
@pytest.mark.parametrize("N,K,nsplit", wc.GEMM_SHAPES + wc.GEMM_TILE_SHAPES)
def test_gemm_rows_e4m3_every_element(kl, table, N, K, nsplit, R, pro):
    ops, lib = kl
    for f32 in (True, False):
        for with_res in (False, True):
            Gemm(lib, table, N, K, nsplit, R, pro, f32, with_res).verify(lib)
    SEEN.update({f"gemm-R{R}", f"gemm-N{N}", f"gemm-pro{pro}"})


@pytest.mark.parametrize("pro", [wc.PRO_BF16, wc.PRO_RMS, wc.PRO_SWIGLU], ids=["bf16", "rms", "swiglu"])
@pytest.mark.parametrize("R,dead", [(3, 1), (16, 7)])
@pytest.mark.parametrize("N,K,nsplit", wc.GEMM_SHAPES)
def test_gemm_rows_e4m3_inactive_row_in_the_middle(kl, table, N, K, nsplit, R, dead, pro):
    """its x and residual rows are NaN (never read); its y row, second destination and xhat row come back bit for bit"""
    ops, lib = kl
    for f32 in (True, False):
        g = Gemm(lib, table, N, K, nsplit, R, pro, f32, True, inactive=(dead,))
        g.verify(lib)
        same_bits(g.Y.v[dead], torch.full_like(g.Y.v[dead], NAN), "inactive y row")
        same_bits(g.y2[dead], torch.full_like(g.y2[dead], NAN), "inactive second destination")
        same_bits(g.xhat[dead], torch.full_like(g.xhat[dead], NAN), "inactive xhat row")
    SEEN.add("gemm-inactive")


def test_ops_wrappers(kl, table):
    """ops.gemv_e4m3 and ops.gemm_rows_e4m3 on ops.quantize_rows_e4m3 of bf16 weights: strided x rows, residual, both dtypes"""
    ops, lib = kl
    g = torch.Generator(device="cuda").manual_seed(5)
    w8, s = ops.quantize_rows_e4m3((torch.randn((264, 1008), generator=g, device="cuda") / 1008 ** 0.5).to(BF))
    Wdq = dequant(w8, s, table)
    xfull = torch.randn((5, 1024), generator=g, device="cuda").to(BF)
    res = torch.randn((5, 264), generator=g, device="cuda")
    for dt, r in ((F32, res), (BF, None)):
        y = ops.gemm_rows_e4m3(xfull[:, :1008], w8, s, residual=r, out_dtype=dt)
        y1 = ops.gemv_e4m3(xfull[2, :1008], w8, s, residual=r[2] if r is not None else None, out_dtype=dt)
        torch.cuda.synchronize()
        for i in range(5):
            ref, tol = gemv8_ref(Wdq, xfull[i, :1008].double(), 1008, res=r[i].double() if r is not None else None, bf16_out=dt == BF)
            check(y[i], ref, tol, f"ops.gemm_rows_e4m3 row {i}")
            if i == 2:
                check(y1, ref, tol, "ops.gemv_e4m3")
    SEEN.add("ops")


def test_refusals_leave_outputs_untouched(kl):
    """K % 16, ldq % 16, K > 32768, a NULL scale: KALLE_ERR_ARG from each entry point, nothing written"""
    ops, lib = kl
    W = torch.zeros((20, 32784), device="cuda", dtype=torch.uint8)
    Wb = torch.zeros((20, 32784), device="cuda", dtype=BF)
    s = torch.ones(20, device="cuda")
    x = torch.zeros((16, 32784), device="cuda", dtype=BF)
    y = torch.full((16, 20), NAN, device="cuda")
    q = torch.full((20, 32784), 0xAA, device="cuda", dtype=torch.uint8)
    so = torch.full((20,), NAN, device="cuda")
    for K, ldq, sc in ((72, 80, s), (64, 72, s), (32784, 32784, s), (64, 80, None)):
        assert lib.kalle_gemv_e4m3(P(x), P(W), ldq, P(sc), P(y), 1, None, 20, K, None) == ERR_ARG, (K, ldq)
        assert lib.kalle_gemv_fused_e4m3(P(x), 0, None, ctypes.c_float(0), P(W), ldq, P(sc), P(y), 1, None, 20, None, 20, K, None) == ERR_ARG, (K, ldq)
        assert lib.kalle_gemm_rows_fused_e4m3(P(x), 32784, 0, None, ctypes.c_float(0), None, P(W), ldq, P(sc), P(y), 20, 1, None, 20, None,
                                              None, 0, None, 3, 20, K, None) == ERR_ARG, (K, ldq)
        if K <= 32768:
            assert lib.kalle_quantize_rows_e4m3(P(Wb), 32784, P(q), ldq, P(so if sc is not None else None), 20, K, None) == ERR_ARG, (K, ldq)
    for R in (0, 17):
        assert lib.kalle_gemm_rows_fused_e4m3(P(x), 32784, 0, None, ctypes.c_float(0), None, P(W), 80, P(s), P(y), 20, 1, None, 20, None,
                                              None, 0, None, R, 20, 64, None) == ERR_ARG, R
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and (q == 0xAA).all() and torch.isnan(so).all()
    SEEN.add("refusals")


# ------------------------------------------------------------------------------------------------ the two steps
class Setup:
    """test_decode_rows_gpu.Setup with the layers' weights quantised by the kernel; c["one"]: the one-row step on the same
    buffers (R = 1: the one-row workspace is the rows workspace without its last region, xn, which must then stay untouched)"""

    def __init__(self, kl, tab, c, n_layers=1):
        from kalle_audio_amd import _lib
        ops, lib = kl
        self.ops, self.lib, self.c, self.tab = ops, lib, c, tab
        self.s = tr.Setup(lib, c, n_layers)
        self.s.x.mul_(c.get("xscale", 1.0))
        self.one = bool(c.get("one"))
        self.q, self.dq, self.bf = [], [], []
        self.arr = (_lib.LlamaLayerW8 * n_layers)()
        for d, L in zip(self.arr, self.s.layers):
            qs = {k: ops.quantize_rows_e4m3(getattr(L, k)) for k in ("wqkv", "wo", "wug", "wdown")}
            self.q.append(qs)
            self.dq.append({k: dequant(w8, sc, tab) for k, (w8, sc) in qs.items()})
            d.input_norm, d.post_norm, d.kv_cache = L.input_norm.data_ptr(), L.post_norm.data_ptr(), L.cache.data_ptr()
            for k, sk in (("wqkv", "sqkv"), ("wo", "so"), ("wug", "sug"), ("wdown", "sdown")):
                setattr(d, k, qs[k][0].data_ptr())
                setattr(d, sk, qs[k][1].data_ptr())
        torch.cuda.synchronize()

    def step(self, n_layers=None, layer0=0, x=None, **over):
        s, c = self.s, self.c
        a = dict(R=s.R, H=c["H"], Hkv=c["Hkv"], inner=c["inner"], hd=c["hd"], t0=c["t0"], rows=c["rows"])
        a.update(over)
        arr = ctypes.c_void_p(ctypes.addressof(self.arr) + layer0 * ctypes.sizeof(self.arr[0]))
        n = len(s.layers) if n_layers is None else n_layers
        xin = s.x if x is None else x
        if self.one:
            rcode = self.lib.kalle_llama_decode_step_w8(arr, n, P(xin), P(s.out), a["H"], a["Hkv"], a["inner"], a["hd"], ctypes.c_float(wc.EPS),
                                                        a["t0"][0], a["rows"], P(s.cos), P(s.sin), P(s.ws), None)
        else:
            rcode = self.lib.kalle_llama_decode_step_rows_w8(arr, n, P(xin), P(s.out), a["R"], a["H"], a["Hkv"], a["inner"], a["hd"],
                                                             ctypes.c_float(wc.EPS), iarr(list(a["t0"])), a["rows"], P(s.cos), P(s.sin),
                                                             P(s.ws), None)
        torch.cuda.synchronize()
        return rcode

    def plan(self):
        hd = self.c["hd"]
        if not self.one:
            return tr.rows_plan(hd, hd)
        return td.DECODE_PLAN if hd == 64 else lc128.decode128()

    def weights(self, layer, wrong=None):
        """the dequantised weights of a layer, or a deliberately wrong set: "bf16_weights" (the unquantised ones),
        "neighbour_scale" (row n with the scale of row n + 1), "fnuz" (the MI300 decoding of the codes; its NaN code 0x80 - which is
        -0 here - taken as 0)"""
        if wrong is None:
            return self.dq[layer]
        if wrong == "bf16_weights":
            L = self.s.layers[layer]
            return {k: getattr(L, k).double() for k in ("wqkv", "wo", "wug", "wdown")}
        if wrong == "neighbour_scale":
            return {k: dequant(w8, torch.roll(sc, -1), self.tab) for k, (w8, sc) in self.q[layer].items()}
        assert wrong == "fnuz"
        z = torch.nan_to_num(f8.decode_table_fnuz(), nan=0.0).cuda()
        return {k: dequant(w8, sc, z) for k, (w8, sc) in self.q[layer].items()}


def stages(S, layer, r, x, out, wrong=None):
    """test_decode_rows_gpu.stages for row r with the dequantised weights (or a wrong set) in the four GEMV stages; wrong =
    "no_eps": stage 1 from an RMSNorm without eps (test_decode_gpu.stages' wrong reference of that name)"""
    s, L, W = S.s, S.s.layers[layer], S.weights(layer, None if wrong == "no_eps" else wrong)
    c, D = s.c, s.D
    hd, H, Hkv, t0 = c["hd"], c["H"], c["Hkv"], c["t0"][r]
    ws = {k: v[r].clone() for k, v in s.regions().items() if not k.endswith("_pad")}
    res = []
    xh = kr.decode_rms_prologue(x.double(), L.input_norm.double(), wc.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 1")
    if wrong == "no_eps":
        xr = kr.bf16r(kr.decode_rms_prologue(x.double(), L.input_norm.double(), wc.EPS, "no_eps"))
    ref, tol = gemv8_ref(W["wqkv"], xr, D, bf16_out=True, amb_ulp=au)
    res.append(("q | k | v", torch.cat([ws["q"], L.cache[r, t0]]), ref, tol))
    w = Hkv * hd
    cache = L.cache[r].double()
    n = t0 + 1
    ao, lse, p, qh, kh = kr.attention_ref(ws["q"].double()[None, None, :], cache[None, :n, :w], cache[None, :n, w:], H, Hkv, hd, rot=hd,
                                          cos=s.cos.double(), sin=s.sin.double(), causal=True, round_points=True)
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, cache[None, :n, w:], ao, lse, H, Hkv, hd)
    res.append(("ao", ws["ao"], ao.reshape(-1), ATTN_ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1)))
    res.append(("lse", ws["lse"], lse.reshape(-1), ATTN_ALLOW["lse/decode"] * U * u_lse.reshape(-1)))
    ref, tol = gemv8_ref(W["wo"], ws["ao"].double(), D, res=x.double())
    res.append(("x2", ws["x2"], ref, tol))
    xh = kr.decode_rms_prologue(ws["x2"].double(), L.post_norm.double(), wc.EPS)
    xr, au = td.prologue(xh, dc.rms_window(xh), "stage 4")
    ref, tol = gemv8_ref(W["wug"], xr, D, bf16_out=True, amb_ulp=au)
    res.append(("hf", ws["hf"], ref, tol))
    hf = ws["hf"].double()
    ar, au = td.prologue(kr.decode_swiglu_prologue(hf), dc.swiglu_window(hf), "stage 5")
    ref, tol = gemv8_ref(W["wdown"], ar, c["inner"], res=ws["x2"].double(), amb_ulp=au)
    res.append(("out", out, ref, tol))
    return res


def run_case(kl, tab, name, c):
    ops, lib = kl
    S = Setup(kl, tab, c)
    s = S.s
    assert S.step() == 0, (name, lib.kalle_last_error())
    assert ops.attn_last_plan() == S.plan(), hex(ops.attn_last_plan())
    for r, t in enumerate(c["t0"]):
        if t >= 0:
            assert torch.isfinite(s.out[r]).all(), (name, r, "NaN rows above t0 leaked into the output")
            for stage, got, ref, tol in stages(S, 0, r, s.x[r], s.out[r]):
                check(got, ref, tol, f"{name} row {r} {stage}")
                SEEN.add(stage)
        else:
            SEEN.add("inactive-row")
    tr.untouched(s, name, 1)
    if S.one:
        assert (s.regions()["xn"].contiguous().view(torch.uint8) == 0xFF).all(), (name, "the one-row step wrote past its workspace")
    SEEN.update({name, f"hd{c['hd']}", f"gqa{c['H'] // c['Hkv']}", "one-row" if S.one else "rows"})
    return S


@pytest.mark.parametrize("name", list(wc.ONE_ROW_CASES))
def test_decode_step_w8_stage_by_stage(kl, table, name):
    run_case(kl, table, name, wc.ONE_ROW_CASES[name])


@pytest.mark.parametrize("name", list(wc.ROWS_CASES))
def test_decode_step_rows_w8_stage_by_stage(kl, table, name):
    run_case(kl, table, "rows-" + name, wc.ROWS_CASES[name])


@pytest.mark.parametrize("which", ["one-row", "rows"])
def test_three_layers_in_one_call_equal_three_chained_calls(kl, table, which):
    """bit for bit, for out and for every cache; the workspace then holds the LAST layer's stages (x3: the layer before it), whose
    four GEMV stages - the code this path adds - are checked against fp64 as well.  The attention stages of a step are checked in
    the one-layer cases above; the attention calls are those of the bf16 steps."""
    c = dict(wc.ONE_ROW_CASES["gqa4"], seed=77) if which == "one-row" else dict(wc.ROWS_CASES["hd128"], seed=78)
    a, b = Setup(kl, table, c, 3), Setup(kl, table, c, 3)
    assert a.step() == 0
    x = b.s.x
    for i in range(3):
        assert b.step(n_layers=1, layer0=i, x=x) == 0
        x = b.s.out.clone()
    live = [r for r, t in enumerate(c["t0"]) if t >= 0]
    _exact(a.s.out[live], b.s.out[live], "out")
    assert torch.isfinite(a.s.out[live]).all()
    for i, (la, lb) in enumerate(zip(a.s.layers, b.s.layers)):
        _exact(la.cache, lb.cache, f"cache of layer {i}")
    x3 = a.s.regions()["x3"].clone()
    for r in live:
        for stage, got, ref, tol in stages(a, 2, r, x3[r], a.s.out[r]):
            if stage in GEMV_STAGES:
                check(got, ref, tol, f"three layers ({which}), last layer, row {r} {stage}")
    tr.untouched(a.s, "three layers " + which, 3)
    SEEN.add("three-layers-" + which)


def test_step_refusals_leave_everything_untouched(kl, table):
    """the refusals of the bf16 steps, plus inner % 16 (inner = 8 is fine there)"""
    ops, lib = kl
    for c, overs in ((wc.ROWS_CASES["hd64"], (dict(R=0), dict(R=17, t0=(0,) * 17), dict(Hkv=3), dict(inner=8), dict(inner=24), dict(t0=(0, 40, -1)),
                                                dict(hd=32), dict(H=513))),
                     (wc.ONE_ROW_CASES["base"], (dict(Hkv=3), dict(inner=8), dict(inner=32784), dict(t0=(-1,)), dict(t0=(6,)), dict(hd=32), dict(H=513)))):
        S = Setup(kl, table, c)
        for over in overs:
            assert S.step(**over) == ERR_ARG, over
            assert ops.attn_last_plan() == 0, over
        for f in ("sqkv", "so", "sug", "sdown", "wqkv", "kv_cache"):
            old = getattr(S.arr[0], f)
            setattr(S.arr[0], f, None)
            assert S.step() == ERR_ARG, f
            setattr(S.arr[0], f, old)
        S2 = Setup(kl, table, c, 2)              # a NULL field in the SECOND layer: refused before the first layer runs
        for f in ("sdown", "wug"):
            old = getattr(S2.arr[1], f)
            setattr(S2.arr[1], f, None)
            assert S2.step() == ERR_ARG, f
            setattr(S2.arr[1], f, old)
        assert (S2.s.wsbuf == 0xFF).all() and torch.isnan(S2.s.out).all()
        same_bits(S2.s.layers[0].cache, S2.s.layers[0].cache_before, "cache of layer 0 after a refusal in layer 1")
        assert (S.s.wsbuf == 0xFF).all() and torch.isnan(S.s.out).all()
        same_bits(S.s.layers[0].cache, S.s.layers[0].cache_before, "cache after refused calls")
    SEEN.add("step-refusals")


# ------------------------------------------------------------------------------------------------ wrong references
WRONG_MARGIN = 2.0


@pytest.fixture(scope="module")
def wrong_runs(kl, table):
    runs = {}
    for which, c in (("one-row", wc.ONE_ROW_CASES["gqa4"]), ("rows", wc.ROWS_CASES["hd128"])):
        S = Setup(kl, table, c)
        assert S.step() == 0
        runs[which] = S
    return runs


@pytest.mark.parametrize("stage", GEMV_STAGES)
@pytest.mark.parametrize("wrong", ["bf16_weights", "neighbour_scale", "fnuz"])
@pytest.mark.parametrize("which", ["one-row", "rows"])
def test_wrong_reference_is_caught(wrong_runs, which, wrong, stage):
    """each wrong weight set moves some element of each GEMV stage by more than WRONG_MARGIN x its allowance, and the check that
    passes the right reference fails it"""
    S = wrong_runs[which]
    r = 0 if which == "one-row" else 1
    right = {k: (g, rf, t) for k, g, rf, t in stages(S, 0, r, S.s.x[r], S.s.out[r])}
    bad = {k: rf for k, _, rf, _ in stages(S, 0, r, S.s.x[r], S.s.out[r], wrong=wrong)}
    got, ref, tol = right[stage]
    check(got, ref, tol, f"{wrong}: right reference")
    assert ((bad[stage] - ref).abs() / tol).max().item() > WRONG_MARGIN, (which, wrong, stage)
    with pytest.raises(AssertionError, match="out of bound"):
        check(got, bad[stage], tol, wrong)
    SEEN.add(f"wrong-{which}-{wrong}-{stage}")


def test_wrong_reference_without_eps_is_caught(kl, table):
    """small-x (mean(x^2) ~ eps) on the q | k | v stage of the one-row step, whose RMSNorm prologue is gemv_e4m3_kernel's own: a
    reference that drops eps lies outside the bound that holds the right one"""
    S = Setup(kl, table, wc.ONE_ROW_CASES["small-x"])
    assert S.step() == 0
    got, ref, tol = next((g, rf, t) for k, g, rf, t in stages(S, 0, 0, S.s.x[0], S.s.out[0]) if k == "q | k | v")
    bad = next(rf for k, _, rf, _ in stages(S, 0, 0, S.s.x[0], S.s.out[0], wrong="no_eps") if k == "q | k | v")
    check(got, ref, tol, "no_eps: right reference")
    assert ((bad - ref).abs() / tol).max().item() > WRONG_MARGIN
    with pytest.raises(AssertionError, match="out of bound"):
        check(got, bad, tol, "no_eps")
    SEEN.add("wrong-no_eps")


def test_every_stage_and_edge_was_reached():
    want = {"q | k | v", "ao", "lse", "x2", "hf", "out", "gqa1", "gqa2", "gqa4", "hd64", "hd128", "one-row", "rows", "inactive-row",
            "three-layers-one-row", "three-layers-rows", "step-refusals", "refusals", "ops", "quant-ops", "gemm-inactive", "gemv-nsplit",
            "gemv-whole", "quant-normal", "quant-zero-and-single", "quant-lossless", "wrong-no_eps"}
    want |= set(wc.ONE_ROW_CASES) | {"rows-" + n for n in wc.ROWS_CASES}
    want |= {f"quant-N{s[0]}" for s in wc.QUANT_SHAPES} | {f"gemv-N{s[0]}" for s in wc.GEMV_SHAPES} | {f"gemv-K{s[1]}" for s in wc.GEMV_SHAPES} | {f"gemv-{s[0]}x{s[1]}" for s in wc.GEMV_SHAPES}
    want |= {f"gemv-pro{p}" for p in range(3)} | {f"gemm-pro{p}" for p in range(3)} | {f"gemm-R{r}" for r in wc.GEMM_ROWS}
    want |= {f"gemm-N{s[0]}" for s in wc.GEMM_SHAPES + wc.GEMM_TILE_SHAPES}
    want |= {f"wrong-{a}-{w}-{s}" for a in ("one-row", "rows") for w in ("bf16_weights", "neighbour_scale", "fnuz") for s in GEMV_STAGES}
    assert want <= SEEN, sorted(want - SEEN)
