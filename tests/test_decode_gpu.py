"""-m gpu: the KV-cached decode path (csrc/llasa.hip: gemv_kernel<YF32, PRO>, kalle_gemv_bf16, kalle_llama_decode_step), stage by
stage and element by element against the fp64 references of tests/kernel_refs.py (checked on the CPU by
tests/test_decode_refs_cpu.py).

The workspace of kalle_llama_decode_step is caller-owned and its layout is part of the header: after a one-layer call it holds
every stage's output.  Each stage is checked against fp64 from that stage's own inputs AS THE KERNEL PRODUCED THEM, so no bound
inherits an earlier stage's error:
  1 q, cache row t0   bf16(Wqkv . bf16(rmsnorm(x)))                            from x
  2 ao, lse           attention_ref(q, cache rows 0 .. t0), rot 64, causal      from the kernel's q and cache
  3 x2                x + Wo . ao                                               from the kernel's ao
  4 hf                bf16(Wug . bf16(rmsnorm(x2)))                             from the kernel's x2
  5 out               x2 + Wdown . bf16(up * silu(gate))                        from the kernel's x2 and hf

Bounds (derived): a GEMV output gets K 2^-24 sum_k |W_nk| |xhat_k| (an fp32 dot product in any order) + 4 x 2^-24 (|residual| + that
sum) for the closing adds, + 2^-8 |ref| where it is stored as bf16.  The prologue value xhat is rounded to bf16 inside the kernel,
from an fp32 value that differs from the float64 one by the fast-math allowances of tests/test_norm_elementwise_gpu.py (rsqrtf
10 u, sigmoid 10 u; decode_cases.rms_window / swiglu_window): an element whose float64 value lies within that window of a bf16
rounding boundary is AMBIGUOUS, and only such an element k adds |W_nk| ulp_bf16(xhat_k) to the allowance of output n.  The
ambiguous elements are capped at 1 % of K in every case (asserted here on the values the kernel saw, and on the CPU for stage
1's inputs); nothing new was measured.  Attention takes the single-query family's allowances of tests/test_attention_gpu.py.

Buffers: x, out and every cache in NaN-guarded allocations; the workspace in an allocation of exactly
kalle_llama_decode_ws_bytes between two 64-byte fences; cache rows above t0 and the rope rows above t0 are NaN before the call
(the output must still be finite), every cache row but t0 must come back bit for bit."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
import decode_cases as dc  # noqa: E402
import kernel_refs as kr  # noqa: E402
from gpu_checks import NAN, U, Guard, _exact, check, clean as _clean, guarded as _guarded  # noqa: E402
from test_attention_gpu import ALLOW as ATTN_ALLOW  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -24
BF16_REL = 2.0 ** -8
CHUNK = 4096                    # rows of a weight matrix per piece of the fp64 reference
ERR_ARG = -1
DECODE_PLAN = 2 | 64 << 8 | 64 << 17          # kalle_attn_last_plan: single-query family, head dim 64, ROT 64
SEEN = set()
FENCE = 64


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def kl():
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def dev_weight(n, k, g):
    w = torch.empty((n, k), device="cuda", dtype=torch.bfloat16)
    for r in range(0, n, CHUNK):
        w[r:r + CHUNK] = (torch.randn((min(CHUNK, n - r), k), generator=g, device="cuda") / k ** 0.5).to(torch.bfloat16)
    return w


class Layer:
    def __init__(self, c, g, index):
        H, Hkv, inner, t0, rows = c["H"], c["Hkv"], c["inner"], c["t0"], c["rows"]
        D, kvw = 64 * H, 128 * Hkv
        cpu = torch.Generator().manual_seed(c["seed"] + 1000 + index)
        self.input_norm = (dc.stage1_inputs(c)[1] if index == 0 else 1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.post_norm = (1 + 0.1 * torch.randn(D, generator=cpu)).cuda()
        self.wqkv, self.wo = dev_weight(D + kvw, D, g), dev_weight(D, D, g)
        self.wug, self.wdown = dev_weight(2 * inner, D, g), dev_weight(D, inner, g)
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
        self.D = 64 * H
        g = torch.Generator(device="cuda").manual_seed(c["seed"])
        self.layers = [Layer(c, g, i) for i in range(n_layers)]
        self.arr = (_lib.LlamaLayer * n_layers)()
        for d, L in zip(self.arr, self.layers):
            d.input_norm, d.wqkv, d.wo, d.post_norm, d.wug, d.wdown, d.kv_cache = (t.data_ptr() for t in L.fields())
        self.xbuf, self.x = _guarded(dc.stage1_inputs(c)[0].cuda())
        self.obuf, self.out = _guarded(torch.full((self.D,), NAN, device="cuda"))
        cos, sin = dc.rope_tables(c["rows"])
        cos[c["t0"] + 1:], sin[c["t0"] + 1:] = NAN, NAN
        self.cos, self.sin = cos.cuda(), sin.cuda()
        self.ws_bytes = lib.kalle_llama_decode_ws_bytes(H, Hkv, inner)
        assert self.ws_bytes == 8 * self.D + ((4 * H + 63) & ~63) + 4 * self.D + 4 * inner
        self.wsbuf = torch.full((self.ws_bytes + 2 * FENCE,), 0xFF, device="cuda", dtype=torch.uint8)   # all-ones bytes: NaN as fp32 and as bf16
        self.ws = self.wsbuf[FENCE:FENCE + self.ws_bytes]
        assert self.ws.data_ptr() % 64 == 0

    def step(self, n_layers=None, x=None, layer0=0, **over):
        c = self.c
        a = dict(H=c["H"], Hkv=c["Hkv"], inner=c["inner"], t0=c["t0"], rows=c["rows"])
        a.update(over)
        arr = ctypes.c_void_p(ctypes.addressof(self.arr) + layer0 * ctypes.sizeof(self.arr[0]))
        return self.lib.kalle_llama_decode_step(arr, len(self.layers) if n_layers is None else n_layers, P(self.x if x is None else x),
                                                P(self.out), a["H"], a["Hkv"], a["inner"], ctypes.c_float(dc.EPS), a["t0"], a["rows"],
                                                P(self.cos), P(self.sin), P(self.ws), None)

    def regions(self):
        """the workspace as the header lays it out: x2 | x3 fp32, lse fp32 (padded to 64 bytes), q | ao | hf bf16"""
        D, H, inner = self.D, self.c["H"], self.c["inner"]
        o = 0
        out = {}
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


def gemv_ref(W, xr, K, res=None, bf16_out=False, amb_ulp=None):
    """(ref, tol) of y = W . xr (+ res) in fp64, by chunks of rows; amb_ulp [K]: ulp_bf16 of the ambiguous prologue elements, else 0"""
    refs, tols = [], []
    for r0 in range(0, W.shape[0], CHUNK):
        Wd = W[r0:r0 + CHUNK].double()
        ref, mag = Wd @ xr, Wd.abs() @ xr.abs()
        r = res[r0:r0 + CHUNK] if res is not None else torch.zeros_like(ref)
        ref = ref + r
        tol = K * F32_EPS * mag + 4 * F32_EPS * (r.abs() + mag) + 1e-30
        if bf16_out:
            tol = tol + BF16_REL * ref.abs()
        if amb_ulp is not None:
            tol = tol + Wd.abs() @ amb_ulp
        refs.append(ref)
        tols.append(tol)
    return torch.cat(refs), torch.cat(tols)


def prologue(xh, window, what):
    """the bf16 operand the kernel builds from the prologue value xh (fp64), and the ulps of its ambiguous elements"""
    amb = kr.bf16_ambiguous(xh, window)
    assert amb.sum().item() <= 0.01 * xh.numel(), (what, "ambiguous prologue elements over the 1 % cap", int(amb.sum()), xh.numel())
    return kr.bf16r(xh), torch.where(amb, kr.bf16_ulp(xh), torch.zeros_like(xh))


def stages(s, L, x, out, wrong=None):
    """the five (name, kernel output, ref, tol) of one layer, from the workspace after a one-layer call; `wrong` swaps one
    reference for a deliberately wrong one"""
    c, D = s.c, s.D
    H, Hkv, t0 = c["H"], c["Hkv"], c["t0"]
    ws = {k: v.clone() for k, v in s.regions().items()}
    res = []
    # 1: q and cache row t0
    w1 = wrong if wrong in ("no_eps", "gamma_after_rounding") else None
    xh = kr.decode_rms_prologue(x.double(), L.input_norm.double(), dc.EPS, w1)
    xr, au = prologue(kr.decode_rms_prologue(x.double(), L.input_norm.double(), dc.EPS), dc.rms_window(xh), "stage 1")
    if w1:
        xr = xh if w1 == "gamma_after_rounding" else kr.bf16r(xh)
    ref, tol = gemv_ref(L.wqkv, xr, D, bf16_out=True, amb_ulp=au)
    if wrong == "kv_swapped":
        ref = torch.cat([ref[:D], ref[D + 64 * Hkv:], ref[D:D + 64 * Hkv]])
    res.append(("q | k | v", torch.cat([ws["q"], L.cache[t0]]), ref, tol))
    # 2: attention from the kernel's own q and cache
    ao, lse, p, qh, kh = kr.decode_attention(ws["q"].double(), L.cache.double(), H, Hkv, t0, s.cos.double(), s.sin.double(),
                                             round_points=True, wrong="t0_rows" if wrong == "t0_rows" else None)
    rows = p.shape[-1]
    u_out, u_lse = kr.attention_fwd_units(p, qh, kh, L.cache[None, :rows, 64 * Hkv:].double(), ao, lse, H, Hkv, 64)
    res.append(("ao", ws["ao"], ao.reshape(-1), ATTN_ALLOW["out/decode"] * 2.0 ** -9 * u_out.reshape(-1)))
    res.append(("lse", ws["lse"][:H], lse.reshape(-1), ATTN_ALLOW["lse/decode"] * U * u_lse.reshape(-1)))
    # 3: x2 = x + Wo . ao
    ref, tol = gemv_ref(L.wo, ws["ao"].double(), D, res=x.double())
    res.append(("x2", ws["x2"], ref, tol))
    # 4: hf = bf16(Wug . bf16(rmsnorm(x2)))
    xh = kr.decode_rms_prologue(ws["x2"].double(), L.post_norm.double(), dc.EPS)
    xr, au = prologue(xh, dc.rms_window(xh), "stage 4")
    if wrong == "gamma_after_rounding":
        xr = kr.decode_rms_prologue(ws["x2"].double(), L.post_norm.double(), dc.EPS, wrong)
    ref, tol = gemv_ref(L.wug, xr, D, bf16_out=True, amb_ulp=au)
    res.append(("hf", ws["hf"], ref, tol))
    # 5: out = x2 + Wdown . bf16(up * silu(gate))
    hf = ws["hf"].double()
    act = kr.decode_swiglu_prologue(hf, "gate_silu_up" if wrong == "gate_silu_up" else None)
    ar, au = prologue(kr.decode_swiglu_prologue(hf), dc.swiglu_window(hf), "stage 5")
    if wrong == "gate_silu_up":
        ar = kr.bf16r(act)
    ref, tol = gemv_ref(L.wdown, ar, c["inner"], res=(x if wrong == "residual_x" else ws["x2"]).double(), amb_ulp=au)
    res.append(("out", out, ref, tol))
    return res


def run_case(lib, ops, name):
    c = dc.CASES[name]
    s = Setup(lib, c)
    L = s.layers[0]
    rc = s.step()
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, lib.kalle_last_error())
    assert ops.attn_last_plan() == DECODE_PLAN, hex(ops.attn_last_plan())
    assert ac.step_word(lib, 64, c["H"], c["Hkv"], c["t0"]) == ops.attn_last_plan()       # (what the host query names for the step's attention call)
    assert torch.isfinite(s.out).all(), (name, "NaN rows above t0 leaked into the output")
    for stage, got, ref, tol in stages(s, L, s.x, s.out):
        check(got, ref, tol, f"{name} {stage}")
        SEEN.add(stage)
    # the cache: every row but t0 bit for bit; the buffers: nothing outside them, x3 untouched by a one-layer call
    keep = torch.arange(c["rows"], device="cuda") != c["t0"]
    _exact(L.cache[keep], L.cache_before[keep], name + " cache rows other than t0")
    s.fences_clean(name)
    r = s.regions()
    assert torch.isnan(r["x3"]).all() and torch.isnan(r["lse"][c["H"]:]).all(), (name, "x3 / lse padding written by a one-layer call")
    return s


SMALL = [n for n in dc.CASES if not n.startswith(("limit-", "llama-"))]


@pytest.mark.parametrize("name", SMALL)
def test_decode_step_stage_by_stage(kl, name):
    ops, lib = kl
    run_case(lib, ops, name)
    c = dc.CASES[name]
    SEEN.update({f"gqa{c['H'] // c['Hkv']}", "t0=%d" % c["t0"] if name.startswith("t0") else "", name})


@pytest.mark.parametrize("name", ["llama-3.2-1b", "limit-inner32768", "limit-D32768"])
def test_decode_step_at_model_width_and_at_the_limits(kl, name):
    """one Llama-3.2-1B layer; inner = 32768 (the down projection stages 64 KiB of x in LDS); D = 32768 (every other GEMV does,
    the RMSNorm ones with 16 bytes of static LDS on top: 4.3 GB of weights, references by chunks of rows)"""
    ops, lib = kl
    run_case(lib, ops, name)
    SEEN.add(name)


# ------------------------------------------------------------------------------------------------ kalle_gemv_bf16 alone
@pytest.mark.parametrize("N,K,pad", [(1, 264, 0), (7, 264, 8), (9, 2056, 8), (9, 32768, 0), (8192, 64, 8), (16392, 72, 0)])
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_gemv_rows_not_a_multiple_of_8_and_the_k_limit(kl, N, K, pad, f32, with_res):
    """N = 1, 7, 9 (a wave's second row missing; a workgroup with one live wave), ldw > K, K = 32768 (64 KiB of LDS), and N at the
    two thresholds of several row pairs per wave with a ragged last workgroup"""
    ops, lib = kl
    g = torch.Generator(device="cuda").manual_seed(N + K)
    Wg = Guard(N, K, ld=K + pad, dtype=torch.bfloat16, init=torch.randn((N, K), generator=g, device="cuda") / K ** 0.5)
    xbuf, x = _guarded(torch.randn(K, generator=g, device="cuda").to(torch.bfloat16))
    res = torch.randn(N, generator=g, device="cuda") if with_res else None
    ybuf, y = _guarded(torch.full((N,), NAN, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16))
    rc = lib.kalle_gemv_bf16(P(x), P(Wg.v), K + pad, P(y), 1 if f32 else 0, P(res), N, K, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.kalle_last_error())
    ref, tol = gemv_ref(Wg.v, x.double(), K, res=res.double() if with_res else None, bf16_out=not f32)
    check(y, ref, tol, f"gemv N {N} K {K}")
    _clean(ybuf, y, "gemv y")
    SEEN.add(f"gemv-N{N}")


def test_rejections_leave_outputs_untouched(kl):
    ops, lib = kl
    s = Setup(lib, dc.CASES["gqa4"])
    for over in (dict(Hkv=3), dict(inner=12), dict(t0=-1), dict(t0=s.c["rows"]), dict(H=0), dict(inner=32776), dict(H=513, Hkv=1)):
        assert s.step(**over) == ERR_ARG, over
    for f in ("input_norm", "wqkv", "wo", "post_norm", "wug", "wdown", "kv_cache"):
        old = getattr(s.arr[0], f)
        setattr(s.arr[0], f, None)
        assert s.step() == ERR_ARG, f
        setattr(s.arr[0], f, old)
    torch.cuda.synchronize()
    assert torch.isnan(s.out).all() and (s.wsbuf == 0xFF).all()
    _exact(s.layers[0].cache, s.layers[0].cache_before, "cache after rejected calls")
    W = torch.zeros((9, 272), device="cuda", dtype=torch.bfloat16)
    x = torch.zeros(32776, device="cuda", dtype=torch.bfloat16)
    y = torch.full((9,), NAN, device="cuda")
    for K, ldw, dt in ((260, 272, 1), (264, 268, 1), (32776, 32776, 1), (264, 272, 2), (264, 272, -1), (0, 272, 1)):
        assert lib.kalle_gemv_bf16(P(x), P(W), ldw, P(y), dt, None, 9, K, None) == ERR_ARG, (K, ldw, dt)
    assert lib.kalle_gemv_bf16(None, P(W), 272, P(y), 1, None, 9, 264, None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


def test_three_layers_in_one_call_equal_three_chained_calls(kl):
    """bit for bit, for out and for row t0 of each cache: pins the x2 / x3 ping-pong and the walk over the layer descriptors
    (every kernel of the step sums in a fixed order, so a repeat is exact)"""
    ops, lib = kl
    c = dict(dc.CASES["gqa4"], seed=77)
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
    # the workspace holds the LAST layer's stages (x3: the output of the layer before it): check them against fp64 as well
    x_last = a.regions()["x3"].clone()
    for stage, got, ref, tol in stages(a, a.layers[2], x_last, a.out):
        check(got, ref, tol, f"three layers, last layer {stage}")
    a.fences_clean("three layers")
    SEEN.add("three-layers")


# ------------------------------------------------------------------------------------------------ wrong references
# (gamma after the rounding moves every operand element by up to half a bf16 ulp, an output by ~2^-9 of its terms' root sum of
# squares - as much as the bf16 store of an output of typical size allows.  It shows where an output is small against its terms,
# one element in a thousand: the case with the most outputs, the 16384 of hf at inner = 8192, has a dozen of them.)
WRONG = {"no_eps": ("small-x", "q | k | v"), "gamma_after_rounding": ("rpw4", "hf"), "gate_silu_up": ("base", "out"),
         "kv_swapped": ("base", "q | k | v"), "residual_x": ("base", "out"), "t0_rows": ("base", "ao")}
MARGIN = 2.0


@pytest.fixture(scope="module")
def wrong_runs(kl):
    ops, lib = kl
    runs = {}
    for name in {v[0] for v in WRONG.values()}:
        s = Setup(lib, dc.CASES[name])
        assert s.step() == 0
        torch.cuda.synchronize()
        runs[name] = s
    return runs


@pytest.mark.parametrize("wrong", list(WRONG))
def test_wrong_reference_is_caught(wrong_runs, wrong):
    """each wrong reference moves some element of its stage by more than MARGIN x that element's allowance, and the check that
    passes the right reference fails it"""
    name, stage = WRONG[wrong]
    s = wrong_runs[name]
    right = {k: (g, r, t) for k, g, r, t in stages(s, s.layers[0], s.x, s.out)}
    bad = {k: (g, r, t) for k, g, r, t in stages(s, s.layers[0], s.x, s.out, wrong=wrong)}
    got, ref, tol = right[stage]
    check(got, ref, tol, f"{wrong}: right reference")
    _, wref, wtol = bad[stage]
    margin = ((wref - ref).abs() / tol).max().item()
    assert margin > MARGIN, (wrong, margin)
    with pytest.raises(AssertionError, match="out of bound"):
        check(got, wref, tol, wrong)
    SEEN.add("wrong-" + wrong)


def test_every_stage_and_edge_was_reached():
    want = {"q | k | v", "ao", "lse", "x2", "hf", "out", "gqa1", "gqa2", "gqa4", "three-layers", "llama-3.2-1b", "limit-inner32768",
            "limit-D32768", "gemv-N1", "gemv-N7", "gemv-N9"} | set(SMALL) | {"wrong-" + w for w in WRONG}
    want |= {"t0=%d" % t for t in (0, dc.KB - 1, dc.KB, dc.KB + 1, dc.PV_GROUPS)}
    assert want <= SEEN, sorted(want - SEEN)
