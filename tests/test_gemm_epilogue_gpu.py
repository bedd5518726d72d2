"""-m gpu: kalle_gemm_bf16 on every dispatcher plan x every epilogue field, against an fp64 product of the same bf16 operands.

The reference (in `run_plain`, `run_glu1`, `run_glu2`) is written from the header's text (include/kalle_hip.h, kalle_gemm_epilogue), not from the
kernels: acc = op(A) @ op(B); v = alpha * acc (alpha 0 reads as 1); + bias; * sigmoid(1 - gate[m // rows_per_batch]); rows with
row_mask 0 become 0; + residual[crow]; C[crow] (+)= v, crow being the remapped output row.  Every element is bounded, not only
the rel-L2 of the whole output (one wrong row or tile of a 32 256-row output hides in a rel-L2):
    fp32 C:  |out - ref| <= K 2^-24 |alpha| (|A| @ |B|^T) s + 8 * 2^-24 * (every term's magnitude)
    bf16 C:  the fp32 bound twice + 2^-8 |ref|                 (one rounding of the result to bf16)
Everything the call must not write (rows a remap skips, rows between batches, the columns between N and ldc, the tails of
glu_aux and glu_dbias) starts as NaN and must still be NaN afterwards; the operands' padding (gate and residual columns
beyond N, residual rows a remap skips, the bias tail) is NaN too, so a read at a wrong row or column shows in the output.
Each case also asserts which plan ran (kalle_gemm_last_plan), and that it is the one the host query kalle_gemm_plan named just
before the launch.  The shapes live in tests/gemm_cases.py, which tests/test_gemm_plan_cpu.py checks against the planner
(gemm2.hip: plan_gemm) without a GPU: that every shape reaches the plan it names is known before this file runs."""
import itertools
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
from gemm_cases import (FACTORS, GLU1, GLU2, HEADLINE, HEADLINE_GLU, PAIRWISE, PAIRWISE_ROUTES, PRODUCT, ROUTES,  # noqa: E402
                        UNSUPPORTED, WGRAD, WGRAD_EPI)
from gemm_cases import pairwise_valid as _valid  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -24
BF16_REL = 2.0 ** -8          # one round-to-nearest to bf16 is <= 2^-9 relative: 2^-8 leaves room for the fp32 error it rounds
CHUNK = 4096                  # rows of the fp64 reference per piece


@pytest.fixture(scope="module")
def kl(dev):
    from kalle_audio_amd import _lib, ops
    return ops, _lib.load()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


def _crow(m, remap):
    """stored row of logical row m (header: (m / c_rows_per_batch) * c_batch_rows + c_row_offset + m % c_rows_per_batch)"""
    if not remap:
        return m
    rpb, brows, off = remap
    return (m // rpb) * brows + off + m % rpb


def _nan_padded(rows, cols, ld, g, scale=1.0, dtype=torch.float32):
    """[rows][ld] buffer: random [:, :cols], NaN beyond"""
    t = torch.full((rows, ld), float("nan"), device="cuda", dtype=dtype)
    t[:, :cols] = _randn((rows, cols), g, scale).to(dtype)
    return t


class Spec:
    """one kalle_gemm_bf16 call: shape, layout, output type and epilogue fields"""

    def __init__(self, M, N, K, *, akm=0, bkm=0, f32=True, bias=False, gate=0, residual=False, mask=False, remap=None,
                 accumulate=False, alpha=1.0, ldc_pad=0, ldr_pad=24, ldg_pad=36, plan=None, slices=None, seed=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def __repr__(self):
        f = [f"{self.M}x{self.N}x{self.K}", f"<{self.akm},{self.bkm},{int(self.f32)}>"]
        for k in ("bias", "gate", "residual", "mask", "remap", "accumulate", "ldc_pad"):
            if getattr(self, k):
                f.append(f"{k}={getattr(self, k)}")
        if self.alpha != 1.0:
            f.append(f"alpha={self.alpha}")
        return " ".join(f)


def _row_mask(M, g):
    """random zeros, plus a whole 256-row tile and the last row"""
    m = (torch.rand(M, generator=g, device="cuda") > 0.2).to(torch.uint8)
    if M > 512:
        m[256:512] = 0
    m[-1] = 0
    return m


def _operands(s, g):
    """bf16 operands scaled so that acc ~ N(0, 1): A stored [M][K] or [K][M] (a_kmajor), B [N][K] or [K][N] (b_kmajor)"""
    sc = s.K ** -0.25
    a = _randn((s.K, s.M) if s.akm else (s.M, s.K), g, sc).bfloat16()
    b = _randn((s.K, s.N) if s.bkm else (s.N, s.K), g, sc).bfloat16()
    return a, b


def _op(a, b, s):
    """op(A) [M][K] and op(B) [N][K] as fp64 views"""
    A = a.double().T if s.akm else a.double()
    B = b.double().T if s.bkm else b.double()
    return A, B


def _elementwise(out, ref, tol, what):
    bad = (out - ref).abs() > tol
    bad |= torch.isnan(out)
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        r, c = idx[0], idx[1]
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound; first at (row {r}, col {c}): "
                             f"out {out[r, c].item():.6g} ref {ref[r, c].item():.6g} tol {tol[r, c].item():.3g}")


def _query(ops, s):
    """what the host query says the call of `s` will launch, asked on the launching thread"""
    shape, kw = gc.plan_kwargs(gc.case(**{k: v for k, v in s.__dict__.items() if k in ("M", "N", "K") or k in gc.DEFAULTS}))
    rc, word = ops.gemm_plan(*shape, **kw)
    assert rc == 0, (s, rc)
    return word


def _plan_check(lib, s, queried):
    plan = lib.kalle_gemm_last_plan()
    assert plan == queried, (s, hex(plan), hex(queried))
    if s.plan is not None:
        assert plan & 255 == s.plan, (s, hex(plan))
    if s.slices is not None:
        assert (plan >> 16 > 1) == s.slices, (s, hex(plan))
    return plan


def run_plain(ops, lib, s):
    """one non-GLU call of `s` with NaN sentinels; checked element by element against the fp64 reference"""
    g = _gen(1000 + s.seed)
    M, N, K = s.M, s.N, s.K
    a, b = _operands(s, g)
    m_idx = torch.arange(M, device="cuda")
    crow = _crow(m_idx, s.remap)
    rows = int(crow[-1]) + 3                        # (a few rows past the last stored one, which must stay NaN too)
    ldc = N + s.ldc_pad
    cdt = torch.float32 if s.f32 else torch.bfloat16
    C = torch.full((rows, ldc), float("nan"), device="cuda", dtype=cdt)
    C0 = None
    if s.accumulate:
        C0 = _randn((M, N), g)
        C[crow, :N] = C0
    kw = {}
    bias = gate = res = mask = None
    if s.bias:
        bias_buf = torch.full((N + 16,), float("nan"), device="cuda")
        bias_buf[:N] = _randn((N,), g)
        bias = bias_buf[:N]
        kw["bias"] = bias
    if s.gate:
        nb = (M + s.gate - 1) // s.gate
        gate = _nan_padded(nb, N, N + s.ldg_pad, g)
        kw.update(gate=gate[:, :N], rows_per_batch=s.gate)
    if s.residual:
        res = torch.full((rows, N + s.ldr_pad), float("nan"), device="cuda")
        res[crow, :N] = _randn((M, N), g)          # (the rows a remap skips stay NaN: reading one shows)
        kw["residual"] = res[:, :N]
    if s.mask:
        mask = _row_mask(M, g)
        kw["row_mask"] = mask
    if s.remap:
        kw.update(c_rows_per_batch=s.remap[0], c_batch_rows=s.remap[1], c_row_offset=s.remap[2])
    queried = _query(ops, s)
    y = ops.gemm(a, b, a_kmajor=bool(s.akm), b_kmajor=bool(s.bkm), out=C[:, :N], accumulate=s.accumulate, alpha=s.alpha,
                 M=M, N=N, K=K, **kw)
    assert y is not None
    _plan_check(lib, s, queried)
    torch.cuda.synchronize()

    A, B = _op(a, b, s)
    alpha = s.alpha if s.alpha != 0.0 else 1.0
    num = den = 0.0
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        acc = A[r0:r1] @ B.T
        absacc = A[r0:r1].abs() @ B.abs().T
        v = alpha * acc
        mag = abs(alpha) * absacc
        if s.bias:
            v = v + bias.double()
            mag = mag + bias.double().abs()
        sg = torch.ones_like(v[:, :1])
        if s.gate:
            sg = torch.sigmoid(1.0 - gate[m_idx[r0:r1] // s.gate, :N].double())
            v = v * sg
            mag = mag * sg
        if s.mask:
            keep = mask[r0:r1].double()[:, None]
            v = v * keep
            mag = mag * keep
            sg = sg * keep
        cr = crow[r0:r1]
        if s.residual:
            v = v + res[cr, :N].double()
            mag = mag + res[cr, :N].double().abs()
        if s.accumulate:
            v = v + C0[r0:r1].double()
            mag = mag + C0[r0:r1].double().abs()
        tol = K * F32_EPS * abs(alpha) * absacc * sg + 8 * F32_EPS * mag + 1e-30
        if not s.f32:
            tol = 2 * tol + BF16_REL * v.abs()
        out = C[cr, :N].double()
        _elementwise(out, v, tol, f"{s} rows {r0}..{r1}")
        num += (out - v).pow(2).sum().item()
        den += v.pow(2).sum().item()
        del acc, absacc, v, mag, tol, out
    rel = math.sqrt(num / max(den, 1e-300))
    assert rel < (2e-5 if s.f32 else 4e-3), (s, rel)
    written = torch.zeros((rows, ldc), dtype=torch.bool, device="cuda")
    written[crow, :N] = True
    assert torch.isnan(C[~written]).all(), (s, "stray writes", int((~torch.isnan(C[~written])).sum()))


# ------------------------------------------------------------------------------------------------ plan routes (gemm_cases.ROUTES) x the product's epilogues
def _product_cases():
    out = []
    for rn, r in ROUTES.items():
        for en, e in PRODUCT.items():
            out.append(pytest.param(rn, en, id=f"{rn}-{en}"))
    return out


@pytest.mark.parametrize("route,epi", _product_cases())
def test_product_epilogue_on_every_plan(kl, route, epi):
    ops, lib = kl
    s = Spec(**{**ROUTES[route], **PRODUCT[epi]}, seed=zlib.crc32(f"{route}-{epi}".encode()) % 1000)
    run_plain(ops, lib, s)


def _pairwise_cases():
    out = []
    for rn in PAIRWISE_ROUTES:
        for i, c in enumerate(PAIRWISE):
            out.append(pytest.param(rn, i, id=f"{rn}-pw{i}"))
    return out


@pytest.mark.parametrize("route,idx", _pairwise_cases())
def test_pairwise_epilogue_cover(kl, route, idx):
    ops, lib = kl
    s = Spec(**{**ROUTES[route], **PAIRWISE[idx]}, seed=idx)
    run_plain(ops, lib, s)


def test_pairwise_cover_is_complete():
    """(host side) every pair of option values appears in some case of the cover"""
    keys = list(FACTORS)
    for k1, k2 in itertools.combinations(keys, 2):
        for v1, v2 in itertools.product(FACTORS[k1], FACTORS[k2]):
            c = {**{k: FACTORS[k][0] for k in keys}, k1: v1, k2: v2}
            if _valid(c):
                assert any(r[k1] == v1 and r[k2] == v2 for r in PAIRWISE), (k1, v1, k2, v2)


# ------------------------------------------------------------------------------------------------ weight gradients
# a_kmajor (dy^T x, K = tokens), fp32 out: plain calls take atomic split-K into C (zeroed first when overwriting); the 256 x 256
# kernel may mix two slice counts.  Epilogue fields turn the split off (the whole K in one workgroup).
@pytest.mark.parametrize("shape,plan,plan_ep", [pytest.param(shape, plan, plan_ep, id=i) for i, shape, plan, plan_ep in WGRAD])
@pytest.mark.parametrize("epi", list(WGRAD_EPI.values()), ids=list(WGRAD_EPI))
def test_wgrad_epilogue(kl, shape, plan, plan_ep, epi):
    ops, lib = kl
    plain = not any(epi.get(k) for k in ("bias", "gate", "residual", "mask", "remap"))
    s = Spec(akm=1, bkm=1, f32=True, **shape, **epi, plan=plan if plain else plan_ep, seed=7)
    run_plain(ops, lib, s)
    split = (lib.kalle_gemm_last_plan() >> 8) & 255 > 1
    if shape["K"] == 32256:
        assert split == plain, (s, hex(lib.kalle_gemm_last_plan()))      # the atomic split-K path ran where it may


def test_gemv_single_row(kl):
    """one output row (decoding): the weight-streaming kernel, with bias or residual"""
    ops, lib = kl
    g = _gen(3)
    K, N = 1536, 4616
    a = _randn((1, K), g, K ** -0.25).bfloat16()
    b = _randn((N, K), g, K ** -0.25).bfloat16()
    bias, res = _randn((N,), g), _randn((1, N), g)
    acc = a.double() @ b.double().T
    absacc = a.double().abs() @ b.double().abs().T
    for kw, ref, mag in [(dict(bias=bias), acc + bias.double(), absacc + bias.double().abs()),
                         (dict(residual=res, out_dtype=torch.float32), acc + res.double(), absacc + res.double().abs())]:
        y = ops.gemm(a, b, **kw).double()
        tol = 2 * (K * F32_EPS * absacc + 8 * F32_EPS * mag) + (BF16_REL * ref.abs() if "bias" in kw else 0)
        _elementwise(y, ref, tol, f"gemv {list(kw)}")


# ------------------------------------------------------------------------------------------------ fused SwiGLU
def _silu(x):
    return x * torch.sigmoid(x)


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def run_glu1(ops, lib, M, inner, K, plan, ldc_pad=0, seed=0):
    """forward: C = h = x W^T + b [M][2 inner] (bf16), glu_aux = act = bf16(h_x) * silu(bf16(h_g)) [M][inner]"""
    g = _gen(2000 + seed)
    N = 2 * inner
    sc = K ** -0.25
    x = _randn((M, K), g, sc).bfloat16()
    w = _randn((N, K), g, sc).bfloat16()
    bias = _randn((N,), g)
    C = torch.full((M + 2, N + ldc_pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    aux = torch.full((M * inner + 256,), float("nan"), device="cuda", dtype=torch.bfloat16)
    act = aux[:M * inner].view(M, inner)
    y = ops.gemm(x, w, bias=bias, out=C[:M, :N], glu_mode=1, glu_inner=inner, glu_aux=act)
    assert y is not None, (M, inner, K)
    plan_v = lib.kalle_gemm_last_plan()
    assert plan_v & 255 == plan, (M, inner, K, hex(plan_v))
    torch.cuda.synchronize()
    X, W = x.double(), w.double()
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        h = X[r0:r1] @ W.T + bias.double()
        mag = X[r0:r1].abs() @ W.abs().T + bias.double().abs()
        tol = 2 * (K * F32_EPS * mag) + BF16_REL * h.abs()
        hout = C[r0:r1, :N].double()
        _elementwise(hout, h, tol, f"glu1 h M={M} inner={inner} rows {r0}..")
        # act from the kernel's own bf16 h (the header's formula; h itself was just bounded against fp64)
        aref = hout[:, :inner] * _silu(hout[:, inner:])
        _elementwise(act[r0:r1].double(), aref, BF16_REL * aref.abs() + 1e-6 * (1 + hout[:, :inner].abs()),
                     f"glu1 act M={M} inner={inner} rows {r0}..")
        del h, mag, tol, hout, aref
    assert torch.isnan(C[M:]).all() and torch.isnan(C[:, N:]).all(), "stray writes into C"
    assert torch.isnan(aux[M * inner:]).all(), "stray writes beyond glu_aux"


def run_glu2(ops, lib, M, inner, K, alpha=1.0, ldc_pad=0, seed=0):
    """backward: acc = dact = gb @ W2 (k-major B), d = bf16(alpha acc), dh = (d silu(g), d x silu'(g)), glu_dbias += colsum(dh)"""
    g = _gen(3000 + seed)
    sc = K ** -0.25
    gb = _randn((M, K), g, sc).bfloat16()
    w2 = _randn((K, inner), g, sc).bfloat16()                   # nn.Linear(inner, D).weight [D][inner]: B k-major
    h = _randn((M, 2 * inner), g, 1.5).bfloat16()
    C = torch.full((M + 2, 2 * inner + ldc_pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    db_buf = torch.full((2 * inner + 16,), float("nan"), device="cuda")
    db0 = _randn((2 * inner,), g, 10.0)
    db_buf[:2 * inner] = db0
    y = ops.gemm(gb, w2, b_kmajor=True, out=C[:M, :2 * inner], N=inner, glu_mode=2, glu_inner=inner, glu_aux=h,
                 glu_dbias=db_buf[:2 * inner], alpha=alpha)
    assert y is not None, (M, inner, K)
    plan_v = lib.kalle_gemm_last_plan()
    assert plan_v & 255 == 3, (M, inner, K, hex(plan_v))
    torch.cuda.synchronize()
    A, B = gb.double(), w2.double()
    a = alpha if alpha != 0.0 else 1.0
    colsum_out = torch.zeros(2 * inner, dtype=torch.float64, device="cuda")
    colsum_abs = torch.zeros_like(colsum_out)
    colsum_ref = torch.zeros_like(colsum_out)
    colsum_tol = torch.zeros_like(colsum_out)
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        d = a * (A[r0:r1] @ B)
        ed = 2 * abs(a) * K * F32_EPS * (A[r0:r1].abs() @ B.abs()) + BF16_REL * d.abs()   # d: fp32 product, one bf16 rounding
        x, gg = h[r0:r1, :inner].double(), h[r0:r1, inner:].double()
        dx, dg = d * _silu(gg), d * x * _dsilu(gg)
        tx = _silu(gg).abs() * ed + BF16_REL * dx.abs() + 1e-6 * d.abs() * (1 + gg.abs())
        tg = (x * _dsilu(gg)).abs() * ed + BF16_REL * dg.abs() + 1e-6 * d.abs() * (1 + x.abs() * (1 + gg.abs()))
        out = C[r0:r1, :2 * inner].double()
        _elementwise(out[:, :inner], dx, tx, f"glu2 dh_x M={M} inner={inner} rows {r0}..")
        _elementwise(out[:, inner:], dg, tg, f"glu2 dh_g M={M} inner={inner} rows {r0}..")
        colsum_out += out.sum(0)
        colsum_abs += out.abs().sum(0)
        colsum_ref += torch.cat([dx, dg], 1).sum(0)
        colsum_tol += torch.cat([tx, tg], 1).sum(0)
        del d, ed, x, gg, dx, dg, tx, tg, out
    db = db_buf[:2 * inner].double()
    # the bias gradient sums exactly the dh the kernel stored (fp32 atomics: M additions), and that sum is the fp64 one's
    ftol = 2 * M * F32_EPS * colsum_abs + 4 * F32_EPS * db0.double().abs()
    _elementwise(db[None], (db0.double() + colsum_out)[None], ftol[None], f"glu2 dbias vs stored dh M={M} inner={inner}")
    _elementwise(db[None], (db0.double() + colsum_ref)[None], (ftol + colsum_tol)[None], f"glu2 dbias vs fp64 M={M}")
    assert torch.isnan(C[M:]).all() and torch.isnan(C[:, 2 * inner:]).all(), "stray writes into C"
    assert torch.isnan(db_buf[2 * inner:]).all(), "stray writes beyond glu_dbias"


@pytest.mark.parametrize("M,inner,K,plan", list(GLU1.values()), ids=list(GLU1))
def test_fused_swiglu_forward_vs_fp64(kl, M, inner, K, plan):
    ops, lib = kl
    run_glu1(ops, lib, M, inner, K, plan, ldc_pad=24 if plan == 3 else 0, seed=inner)


@pytest.mark.parametrize("M,inner,K,alpha", list(GLU2.values()), ids=list(GLU2))
def test_fused_swiglu_backward_vs_fp64(kl, M, inner, K, alpha):
    """inner 384 / 640: the last 256-column tile is half (a third) full: the h loads, the j0 < glu_inner guards, the dbias lanes"""
    ops, lib = kl
    run_glu2(ops, lib, M, inner, K, alpha=alpha, ldc_pad=8 if inner == 640 else 0, seed=inner)


# combinations no fused kernel takes (gemm_cases.UNSUPPORTED): None from ops.gemm (kalle_gemm_bf16: KALLE_ERR_UNSUPPORTED), C and glu_aux untouched
@pytest.mark.parametrize("name", list(UNSUPPORTED))
def test_fused_swiglu_unsupported_is_reported(kl, name):
    ops, lib = kl
    mode, shp, ex = UNSUPPORTED[name]
    M, inner, K = shp["M"], shp["inner"], shp["K"]
    g = _gen(4000)
    sc = K ** -0.25
    N = 2 * inner
    cdt = torch.float32 if ex.get("f32") else torch.bfloat16
    C = torch.full((M + 4, N + 8), float("nan"), device="cuda", dtype=cdt)
    kw = {}
    if "gate" in ex:
        kw.update(gate=_randn(((M + 125) // 126, N if mode == 1 else inner), g), rows_per_batch=ex["gate"])
    if ex.get("residual"):
        kw["residual"] = _randn((M, N if mode == 1 else inner), g)
    if ex.get("mask"):
        kw["row_mask"] = _row_mask(M, g)
    if "remap" in ex:
        kw.update(c_rows_per_batch=ex["remap"][0], c_batch_rows=ex["remap"][1], c_row_offset=ex["remap"][2])
    if "alpha" in ex:
        kw["alpha"] = ex["alpha"]
    if mode == 1:
        x = _randn((M, K), g, sc).bfloat16()
        w = _randn((N, K), g, sc).bfloat16()
        if ex.get("bias", True):
            kw["bias"] = _randn((N,), g)
        aux = torch.full((M * inner + 64,), float("nan"), device="cuda", dtype=torch.bfloat16)
        aux0 = aux.clone()
        y = ops.gemm(x, w, out=C[:M, :N], glu_mode=1, glu_inner=inner, glu_aux=aux[:M * inner].view(M, inner), **kw)
    else:
        gb = _randn((M, K), g, sc).bfloat16()
        w2 = _randn((K, inner), g, sc).bfloat16()
        aux = _randn((M, N), g).bfloat16()
        aux0 = aux.clone()
        if ex.get("bias"):
            kw["bias"] = _randn((inner,), g)
        db = torch.zeros(N, device="cuda")
        y = ops.gemm(gb, w2, b_kmajor=True, out=C[:M, :N], N=inner, glu_mode=2, glu_inner=inner, glu_aux=aux, glu_dbias=db, **kw)
    torch.cuda.synchronize()
    assert y is None, (name, "a fused call that drops an epilogue field must report unsupported", hex(lib.kalle_gemm_last_plan()))
    assert torch.isnan(C).all(), (name, "C written by an unsupported call")
    assert torch.equal(aux.view(torch.int16), aux0.view(torch.int16)), (name, "glu_aux written by an unsupported call")
    if mode == 2:
        assert not db.any(), name


# ------------------------------------------------------------------------------------------------ headline shapes, M = 32 256
@pytest.mark.parametrize("name", list(HEADLINE))
def test_headline_shapes_vs_fp64(kl, name):
    ops, lib = kl
    run_plain(ops, lib, Spec(**HEADLINE[name], seed=11))


def test_headline_ff_in_glu1(kl):
    ops, lib = kl
    run_glu1(ops, lib, *HEADLINE_GLU, 3, seed=1)


def test_headline_ff_out_dgrad_glu2(kl):
    ops, lib = kl
    run_glu2(ops, lib, *HEADLINE_GLU, seed=1)


# ------------------------------------------------------------------------------------------------ the mixed split-K plan cache
def test_entry_point_remembers_the_mixed_plan(kl):
    """a launched weight gradient enters its mixed plan into the thread's cache, where a K of the same 16-K-tile bucket finds
    it; the same query on a thread that launched nothing gets that K's own (uniform) plan"""
    ops, lib = kl
    M, N, ka, plan_a, kb, plan_b = gc.REPLAY
    s = Spec(M, N, ka, akm=1, bkm=1, f32=True, plan=3, seed=5)

    def launch_then_query():
        run_plain(ops, lib, s)
        return lib.kalle_gemm_last_plan(), ops.gemm_plan(M, N, kb, a_kmajor=True, b_kmajor=True, f32=True)
    launched, after = gc.fresh_thread(launch_then_query)
    assert launched == plan_a and after == (0, plan_a), (hex(launched), after)
    assert gc.fresh_thread(ops.gemm_plan, M, N, kb, a_kmajor=True, b_kmajor=True, f32=True) == (0, plan_b)
