"""Thin tensor-level wrappers over the C-ABI (kalle_audio_amd/_lib.py).

Every function here takes CUDA (HIP) tensors, launches the hand-written gfx950 kernel on torch's current
stream and returns immediately.  Nothing here falls back to torch math: CPU tensors raise.
PyTorch is used only for device memory and streams.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import KALLE_BF16, KALLE_F32, GemmEpilogue, check


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    if t.dtype == torch.bfloat16:
        return KALLE_BF16
    if t.dtype == torch.float32:
        return KALLE_F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("kalle_audio_amd ops run on the GPU only (HIP kernels); got a CPU tensor")
    return ctypes.c_void_p(t.data_ptr())


def _rows2d(t):
    """(rows, ld) of a tensor viewed as a row-major matrix whose last dim is contiguous."""
    assert t.stride(-1) == 1
    return t.numel() // t.shape[-1], t.shape[-1]


# ------------------------------------------------------------------------------------------------ GEMM
def gemm(a, b, *, a_kmajor=False, b_kmajor=False, out=None, out_dtype=torch.bfloat16, M=None, N=None, K=None,
         lda=None, ldb=None, ldc=None, bias=None, gate=None, rows_per_batch=0, residual=None, accumulate=False,
         alpha=1.0, c_rows_per_batch=0, c_batch_rows=0, c_row_offset=0, row_mask=None, glu_mode=0, glu_inner=0,
         glu_aux=None, glu_dbias=None):
    """C = op(a) @ op(b) with the fused epilogue of kalle_gemm_bf16.

    a: [M,K] (or [K,M] when a_kmajor), b: [N,K] (or [K,N] when b_kmajor); both bf16, last dim contiguous.
    """
    lib = _lib.load()
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
    ar, ac = _rows2d(a)
    br, bc = _rows2d(b)
    if (ar == 1 and not a_kmajor and not b_kmajor and out is None and (bias is None or residual is None)
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())) and gate is None and not glu_mode
            and row_mask is None and not accumulate and alpha == 1.0 and M is None and N is None and K is None
            and ac % 8 == 0 and ac <= 32768 and (residual is None or residual.is_contiguous())):
        # single row (decoding against the KV cache): weight-streaming kernel instead of a 128-row MFMA tile
        y = torch.empty((1, br), device=a.device, dtype=out_dtype)
        check(lib.kalle_gemv_bf16(_p(a), _p(b), b.stride(-2) if b.dim() >= 2 else bc, _p(y), _dt(y),
                                  _p(residual if residual is not None else bias), br, ac,
                                  _stream()), "kalle_gemv_bf16")
        return y
    if M is None:
        M = ac if a_kmajor else ar
    if K is None:
        K = ar if a_kmajor else ac
    if N is None:
        N = bc if b_kmajor else br
    lda = lda if lda is not None else a.stride(-2) if a.dim() >= 2 else ac
    ldb = ldb if ldb is not None else b.stride(-2) if b.dim() >= 2 else bc
    if out is None:
        assert c_rows_per_batch == 0
        out = torch.empty((M, N), device=a.device, dtype=out_dtype)
    ldc = ldc if ldc is not None else out.stride(-2)
    ep = GemmEpilogue()
    ep.bias = bias.data_ptr() if bias is not None else None
    ep.gate = gate.data_ptr() if gate is not None else None
    ep.ldg = gate.stride(-2) if gate is not None else 0
    ep.rows_per_batch = rows_per_batch
    ep.residual = residual.data_ptr() if residual is not None else None
    ep.ldr = residual.stride(-2) if residual is not None else 0
    ep.accumulate = 1 if accumulate else 0
    ep.alpha = alpha
    ep.c_rows_per_batch, ep.c_batch_rows, ep.c_row_offset = c_rows_per_batch, c_batch_rows, c_row_offset
    ep.row_mask = row_mask.data_ptr() if row_mask is not None else None
    ep.glu_mode, ep.glu_inner = glu_mode, glu_inner
    ep.glu_aux = glu_aux.data_ptr() if glu_aux is not None else None
    ep.glu_dbias = glu_dbias.data_ptr() if glu_dbias is not None else None
    lend = _lend_request(M, N, a_kmajor)
    if lend:
        ws = _workspace(a.device, lend)
        ep.workspace, ep.workspace_bytes = ws.data_ptr(), ws.numel()
    if bias is not None:
        assert bias.dtype == torch.float32
    if gate is not None:
        assert gate.dtype == torch.float32
    if residual is not None:
        assert residual.dtype == torch.float32
    prof = KERNEL_TIMER if KERNEL_TIMER_ONLY is None else None     # (a filter names the grouped weight-gradient launch only)
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = lib.kalle_gemm_bf16(_p(a), lda, int(a_kmajor), _p(b), ldb, int(b_kmajor), _p(out), ldc, _dt(out),
                             M, N, K, ctypes.byref(ep), _stream())
    if rc == -3 and glu_mode:
        return None          # fused SwiGLU not available for this shape: the caller runs the unfused sequence
    check(rc, "kalle_gemm_bf16")
    if prof is not None:
        e1.record()
        plan = lib.kalle_gemm_last_plan()
        kname = {1: "gemm_bf16_kernel", 2: "gemm2_kernel", 3: "gemm3_kernel", 4: "gemm2_splitk+finish",
                 5: "gemm2_ks2_kernel"}.get(plan & 255, "gemm")
        variant = "%s<%d,%d,%d%s>" % (kname, int(a_kmajor), int(b_kmajor), int(out.dtype == torch.float32),
                                      ",glu%d" % glu_mode if glu_mode else "")      # (the fused-SwiGLU kernels are their own rows)
        abytes = 2.0 * (M * K + N * K) + M * N * out.element_size() + (4.0 * M * N if residual is not None else 0.0)
        prof.append((variant, 2.0 * M * N * K, e0, e1, abytes, (M, N, K)))
    return out


FEW_ROWS = os.environ.get("KALLE_GEMM_FEW_ROWS", "1") != "0"
FEW_ROWS_MAX = int(os.environ.get("KALLE_GEMM_FEW_ROWS_MAX", "4096"))  # (the dispatcher decides per shape)
_WS = {}
_WS_KEEP = []


def _lend_request(M, N, a_kmajor):
    """bytes gemm() asks _workspace for (0: the call is lent no scratch): few output rows (sampling, small training batches)
    get 8 fp32 [M][N] slabs so that the kernel may split K.  The one rule for gemm() and gemm_plan()."""
    return 4 * M * N * 8 if M <= FEW_ROWS_MAX and not a_kmajor and FEW_ROWS else 0


def _workspace_size(key, nbytes):
    """size of the scratch that _workspace hands out for a request: at least 64 MiB, capped at 1 GiB - the kernel is told the
    size and splits K only as far as the scratch reaches - and never less than the (device, stream)'s scratch has grown to"""
    t = _WS.get(key)
    return max(min(nbytes, 1 << 30), 64 << 20, t.numel() if t is not None else 0)


def _workspace(device, nbytes):
    """per (device, stream) scratch for kalle_gemm_bf16's few-rows path, grown on demand (never shrinks)"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _WS.get(key)
    # (the comparison must use the CAPPED size: comparing with the uncapped request re-allocated - and kept - a fresh GiB on
    # every call once a shape asked for more than the cap, 4032 rows x 12288 columns at B = 32 per GPU: 11 GB per step until
    # the device was full)
    need = _workspace_size(key, nbytes)
    if t is None or t.numel() < need:
        if t is not None:
            _WS_KEEP.append(t)          # a captured HIP graph may still point at the old scratch: never hand it back
        t = _WS[key] = torch.empty(need, device=device, dtype=torch.uint8)
    return t


def _gemm_plan_args(M, N, K, *, a_kmajor=False, b_kmajor=False, f32=False, bias=False, gate=False, rows_per_batch=0,
                    residual=False, accumulate=False, alpha=1.0, c_rows_per_batch=0, row_mask=False, glu_mode=0, glu_inner=0,
                    workspace="lend", workspace_ptr=16):
    """the arguments of kalle_gemm_bf16 in front of `stream` for a call given by its shape and by WHICH epilogue fields it sets,
    with placeholder pointers (the planner tests them for null and alignment only); workspace: "lend" = the scratch gemm()
    lends such a call on the current stream, None, or a byte count.  Returns (arguments, the epilogue they point to)."""
    ep = GemmEpilogue()
    ep.bias = 16 if bias else None
    ep.gate, ep.ldg, ep.rows_per_batch = (16 if gate else None), (N if gate else 0), rows_per_batch
    ep.residual, ep.ldr = (16 if residual else None), (N if residual else 0)
    ep.accumulate = 1 if accumulate else 0
    ep.alpha = alpha
    ep.c_rows_per_batch = ep.c_batch_rows = c_rows_per_batch
    ep.row_mask = 16 if row_mask else None
    ep.glu_mode, ep.glu_inner, ep.glu_aux = glu_mode, glu_inner, (16 if glu_mode else None)
    if workspace == "lend":
        lend = _lend_request(M, N, a_kmajor)
        key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream) if torch.cuda.is_initialized() else None
        workspace = _workspace_size(key, lend) if lend else 0
    if workspace:
        ep.workspace, ep.workspace_bytes = workspace_ptr, workspace
    ldc = 2 * glu_inner if glu_mode == 2 else N
    return (16, M if a_kmajor else K, int(a_kmajor), 16, N if b_kmajor else K, int(b_kmajor), 16, ldc,
            KALLE_F32 if f32 else KALLE_BF16, M, N, K, ctypes.byref(ep)), ep


def gemm_plan(M, N, K, **call):
    """kalle_gemm_plan for a call described as in _gemm_plan_args: (return code, the kalle_gemm_last_plan word kalle_gemm_bf16
    would leave now on this thread, or None where it refuses the call); host code only, no device needed"""
    args, _ep = _gemm_plan_args(M, N, K, **call)
    plan = ctypes.c_int(0)
    rc = _lib.load().kalle_gemm_plan(*args, ctypes.byref(plan))
    return rc, plan.value if rc == 0 else None


# bench.py sets this to a list to collect (kernel variant, algorithmic flops, start event, end event) per GEMM launch:
# HIP events recorded on the launch stream, read back after the timed region (no host sync while timing).
KERNEL_TIMER = None
# Two event records per launch are not free (~4.5 us each on this stack: 300 GEMMs per step = 2.7 ms of a 222-ms step), so the timed
# region of bench.py times ONLY the kernel named here (the dominant one: its roofline figure must come from the timed region) and
# collects the table of all variants in one extra step afterwards.  None: every launch.
KERNEL_TIMER_ONLY = None


# ------------------------------------------------------------------------------------------------ norms
def layernorm_fwd(x, gamma, beta=None, scale=None, shift=None, rows_per_batch=0, eps=1e-5):
    lib = _lib.load()
    rows, D = _rows2d(x)
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    ld_mod = scale.stride(-2) if scale is not None else (shift.stride(-2) if shift is not None else 0)
    check(lib.kalle_layernorm_fwd(_p(x), _dt(x), _p(gamma), _p(beta), _p(scale), _p(shift), ld_mod, rows_per_batch,
                                  _p(y), _p(mean), _p(rstd), rows, D, eps, _stream()), "kalle_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, scale=None, rows_per_batch=0, dres=None, dx_out=None, want_dbeta=False,
                  dgamma_out=None, accumulate=False, dx_bf16=None, dx_colsum_out=None):
    """returns (dx fp32, dgamma fp32 [D], dbeta fp32 [D] or None); dgamma_out (+accumulate) writes dgamma in place;
    dx_bf16: optional bf16 tensor that receives a rounded copy of dx; dx_colsum_out (trainer mode only: dgamma_out +
    accumulate): fp32 [D] that the kernel atomically ADDS the column sums of the bf16-rounded dx to"""
    lib = _lib.load()
    rows, D = _rows2d(x)
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and x.is_contiguous()
    if dx_out is None:
        dx_out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    ld_mod = scale.stride(-2) if scale is not None else 0
    if dx_colsum_out is not None:
        assert dgamma_out is not None and accumulate and not want_dbeta
        check(lib.kalle_layernorm_bwd_colsum(_p(dy), _p(x), _dt(x), _p(gamma), _p(scale), ld_mod, rows_per_batch, _p(mean),
                                             _p(rstd), _p(dres), _p(dx_out), _p(dx_bf16), _p(dgamma_out), _p(dx_colsum_out),
                                             rows, D, _stream()), "kalle_layernorm_bwd_colsum")
        return dx_out, dgamma_out, None
    if dgamma_out is not None and accumulate and not want_dbeta and os.environ.get("KALLE_LN_ATOMIC", "1") != "0":
        # trainer mode: the gradient sink already holds this step's running sum - add into it from the kernel
        check(lib.kalle_layernorm_bwd_acc(_p(dy), _p(x), _dt(x), _p(gamma), _p(scale), ld_mod, rows_per_batch, _p(mean),
                                          _p(rstd), _p(dres), _p(dx_out), _p(dx_bf16), _p(dgamma_out), None, rows, D,
                                          _stream()), "kalle_layernorm_bwd_acc")
        return dx_out, dgamma_out, None
    nparts = lib.kalle_layernorm_bwd_parts(rows)
    dgp = torch.empty((nparts, D), device=x.device, dtype=torch.float32)
    dbp = torch.empty((nparts, D), device=x.device, dtype=torch.float32) if want_dbeta else None
    check(lib.kalle_layernorm_bwd(_p(dy), _p(x), _dt(x), _p(gamma), _p(scale), ld_mod, rows_per_batch, _p(mean),
                                  _p(rstd), _p(dres), _p(dx_out), _p(dx_bf16), _p(dgp), _p(dbp), rows, D, _stream()),
          "kalle_layernorm_bwd")
    dgamma = colsum(dgp, out=dgamma_out, accumulate=accumulate)
    dbeta = colsum(dbp) if want_dbeta else None
    return dx_out, dgamma, dbeta


def adaln_mod_bwd(dy, x, gamma, beta, mean, rstd, nbatch, rows_per_batch):
    lib = _lib.load()
    D = x.shape[-1]
    dscale = torch.empty((nbatch, D), device=x.device, dtype=torch.float32)
    dshift = torch.empty((nbatch, D), device=x.device, dtype=torch.float32)
    check(lib.kalle_adaln_mod_bwd(_p(dy), _p(x), _dt(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dscale),
                                  _p(dshift), D, nbatch, rows_per_batch, D, _stream()), "kalle_adaln_mod_bwd")
    return dscale, dshift


def rmsnorm_fwd(x, scale, rows_per_batch=0, eps=1e-6, out_dtype=None):
    lib = _lib.load()
    rows, D = _rows2d(x)
    x = x.contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    rrms = torch.empty(rows, device=x.device, dtype=torch.float32)
    ld = scale.stride(-2) if scale.dim() >= 2 else 0
    check(lib.kalle_rmsnorm_fwd(_p(x), _dt(x), _p(scale), ld, rows_per_batch, _p(y), _dt(y), _p(rrms), rows, D, eps,
                                _stream()), "kalle_rmsnorm_fwd")
    return y, rrms


def rmsnorm_bwd(dy, x, scale, rrms, rows_per_batch=0, dres=None, dx_bf16=None, dscale_out=None, accumulate=False):
    """returns (dx fp32 [+ dres], dscale) - dscale is written / accumulated into `dscale_out` when given"""
    lib = _lib.load()
    rows, D = _rows2d(x)
    dy = dy.contiguous()
    dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    ld = scale.stride(-2) if scale.dim() >= 2 else 0
    if dscale_out is not None and accumulate and ld == 0:
        # trainer mode: add into the gradient sink from the kernel (no partial rows, no reduction launch)
        check(lib.kalle_rmsnorm_bwd_acc(_p(dy), _dt(dy), _p(x), _dt(x), _p(scale), ld, rows_per_batch, _p(rrms), _p(dx),
                                        _p(dscale_out), _p(dres), _p(dx_bf16), rows, D, _stream()), "kalle_rmsnorm_bwd_acc")
        return dx, None
    nparts = lib.kalle_layernorm_bwd_parts(rows)
    dsp = torch.empty((nparts, D), device=x.device, dtype=torch.float32)
    check(lib.kalle_rmsnorm_bwd(_p(dy), _dt(dy), _p(x), _dt(x), _p(scale), ld, rows_per_batch, _p(rrms), _p(dx),
                                _p(dsp), _p(dres), _p(dx_bf16), rows, D, _stream()), "kalle_rmsnorm_bwd")
    if dscale_out is not None:
        colsum(dsp, out=dscale_out, accumulate=accumulate)
        return dx, None
    return dx, colsum(dsp)


def colsum(x, out=None, accumulate=False):
    lib = _lib.load()
    rows, cols = _rows2d(x)
    ld = x.stride(-2) if x.dim() >= 2 else cols
    if out is None:
        out = torch.empty(cols, device=x.device, dtype=torch.float32)
        accumulate = False
    check(lib.kalle_colsum(_p(x), _dt(x), ld, _p(out), rows, cols, int(accumulate), _stream()), "kalle_colsum")
    return out


# ------------------------------------------------------------------------------------------------ elementwise
def swiglu_fwd(h):
    lib = _lib.load()
    rows, two_inner = _rows2d(h)
    inner = two_inner // 2
    out = torch.empty(h.shape[:-1] + (inner,), device=h.device, dtype=torch.bfloat16)
    check(lib.kalle_swiglu_fwd(_p(h), _p(out), rows, inner, _stream()), "kalle_swiglu_fwd")
    return out


def swiglu_bwd(dout, h, dbias=None):
    """dbias: optional fp32 [2*inner] that the kernel atomically adds the column sums of dh to"""
    lib = _lib.load()
    rows, two_inner = _rows2d(h)
    dh = torch.empty_like(h)
    check(lib.kalle_swiglu_bwd(_p(dout), _p(h), _p(dh), _p(dbias), rows, two_inner // 2, _stream()),
          "kalle_swiglu_bwd")
    return dh


def silu_fwd(x):
    lib = _lib.load()
    y = torch.empty_like(x)
    check(lib.kalle_silu_fwd(_p(x), _p(y), _dt(x), x.numel(), _stream()), "kalle_silu_fwd")
    return y


def silu_bwd(dy, x):
    lib = _lib.load()
    dx = torch.empty_like(x)
    check(lib.kalle_silu_bwd(_p(dy), _p(x), _p(dx), _dt(x), x.numel(), _stream()), "kalle_silu_bwd")
    return dx


def diffuse_fwd(x, noise, t, objective="v"):
    lib = _lib.load()
    x = x.contiguous()
    noise = noise.contiguous()
    xt = torch.empty_like(x)
    target = torch.empty_like(x)
    B = x.shape[0]
    check(lib.kalle_diffuse_fwd(_p(x), _p(noise), _p(t), _p(xt), _p(target), B, x.numel() // B,
                                0 if objective == "v" else 1, _stream()), "kalle_diffuse_fwd")
    return xt, target


def mse_loss(out, target, mask=None, weight=1.0, want_grad=True):
    """returns (loss scalar tensor, dout or None). out/target fp32 [B,C,T]; mask bool/uint8 [B,T]."""
    lib = _lib.load()
    out = out.contiguous()
    target = target.contiguous()
    B, C, T = out.shape
    acc = torch.zeros(2, device=out.device, dtype=torch.float32)
    diff = torch.empty_like(out) if want_grad else None
    m8 = mask.to(torch.uint8).contiguous() if mask is not None else None
    check(lib.kalle_mse_fwd(_p(out), _p(target), _p(m8), _p(acc), _p(diff), B, C, T, _stream()), "kalle_mse_fwd")
    loss = torch.empty((), device=out.device, dtype=torch.float32)
    check(lib.kalle_mse_finish(_p(acc), _p(loss), _p(diff), out.numel(), weight, _stream()), "kalle_mse_finish")
    return loss, diff


def transpose_2d(x, out_dtype=None, out=None, R=None, Cn=None, in_batch_stride=None, in_ld=None,
                 out_batch_stride=None, out_ld=None):
    """out[b][c][r] = x[b][r][c]"""
    lib = _lib.load()
    B = x.shape[0]
    R = R if R is not None else x.shape[1]
    Cn = Cn if Cn is not None else x.shape[2]
    in_batch_stride = in_batch_stride if in_batch_stride is not None else x.stride(0)
    in_ld = in_ld if in_ld is not None else x.stride(1)
    if out is None:
        out = torch.empty((B, Cn, R), device=x.device, dtype=out_dtype or x.dtype)
    out_batch_stride = out_batch_stride if out_batch_stride is not None else out.stride(0)
    out_ld = out_ld if out_ld is not None else out.stride(1)
    check(lib.kalle_transpose_2d(_p(x), _dt(x), in_batch_stride, in_ld, _p(out), _dt(out), out_batch_stride, out_ld,
                                 B, R, Cn, _stream()), "kalle_transpose_2d")
    return out


def copy_rows(src, dst, nbatch, rows, cols, src_batch_stride, src_ld, dst_batch_stride, dst_ld, accumulate=False):
    lib = _lib.load()
    check(lib.kalle_copy_rows(_p(src), _dt(src), src_batch_stride, src_ld, _p(dst), _dt(dst), dst_batch_stride,
                              dst_ld, nbatch, rows, cols, int(accumulate), _stream()), "kalle_copy_rows")
    return dst


def cast(x, dtype):
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    check(lib.kalle_cast(_p(x), _dt(x), _p(out), _dt(out), x.numel(), _stream()), "kalle_cast")
    return out


def fourier_features(t, w, out_dtype=torch.float32):
    lib = _lib.load()
    B, half = t.shape[0], w.shape[0]
    out = torch.empty((B, 2 * half), device=t.device, dtype=out_dtype)
    check(lib.kalle_fourier_features(_p(t.contiguous()), _p(w.contiguous()), _p(out), _dt(out), B, half, _stream()),
          "kalle_fourier_features")
    return out


def fourier_features_bwd(dout, t, w):
    lib = _lib.load()
    dw = torch.empty_like(w)
    check(lib.kalle_fourier_features_bwd(_p(dout.contiguous()), _p(t.contiguous()), _p(w.contiguous()), _p(dw),
                                         t.shape[0], w.shape[0], _stream()), "kalle_fourier_features_bwd")
    return dw


def grad_cast(g, nbatch, rows_per_batch, gate=None, x_out=None, x_in=None, row_mask=None):
    """fp32 residual-stream gradient -> bf16 GEMM operand (+ adaLN gate backward). Returns (gb, dgate or None)."""
    lib = _lib.load()
    D = g.shape[-1]
    g = g.contiguous()
    gb = torch.empty(g.shape, device=g.device, dtype=torch.bfloat16)
    if gate is not None:
        gate = gate.contiguous()  # [B, D] slice of the adaLN modulation; dgate shares its leading dim
    dgate = torch.empty_like(gate) if gate is not None else None
    check(lib.kalle_grad_cast(_p(g), _p(x_out), _p(x_in), _p(gate), gate.stride(-2) if gate is not None else 0,
                              _p(row_mask), _p(gb), _p(dgate), nbatch, rows_per_batch, D, _stream()),
          "kalle_grad_cast")
    return gb, dgate


WEIGHTS_EPOCH = 0      # bumped by every write to weights that torch does not record (raw-pointer launches, re-pointed storage,
                       # collectives on .data, weights_changed()): the last field of weights_key()


def weights_changed():
    """Tell every cache derived from weights that some weight was written in a way neither torch nor this package can see
    (`p.data.copy_`, `p.data.lerp_` - ema_pytorch's writes -, a collective on `p.data`): all of them are re-made at their next use.
    The package's own raw-pointer writers (adam_step, the trainer's construction) call it themselves."""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


def weights_key(*params):
    """THE key of every copy derived from parameters ("Weight-derived caches"): per parameter its identity,
    torch's version counter, the address, device and dtype of its storage, then the write epoch.  Pure: reads, never writes.
    `_version` follows in-place ops, load_state_dict and torch.optim steps; the address a re-pointed `p.data` (only while the
    cache also holds weights_pin() of the same parameters - a freed block may be handed out again at the same address); the
    identity a replaced Parameter (load_state_dict(assign=True)); the epoch everything torch does not record."""
    return tuple([(id(p), p._version, p.data_ptr(), p.device, p.dtype) for p in params]) + (WEIGHTS_EPOCH,)


def weights_key_is(key, p):
    """key == weights_key(p) for a cache entry that hangs ON the parameter `p` and holds weights_pin(p), without building the
    key: dit_ops.bf16_of asks this in front of every GEMM, so it reads what can move on its own - epoch, version, address.
    The identity is the entry's place; device and dtype belong to the storage, and while the old storage is pinned another
    one has another address (tests/test_weight_caches_cpu.py holds this to the full comparison on every route)."""
    k = key[0]
    return key[1] == WEIGHTS_EPOCH and k[1] == p._version and k[2] == p.data_ptr()


def weights_pin(*params):
    """aliases of the parameters' CURRENT storage, kept next to a weights_key(): while they live, that storage is not freed, so
    a tensor `p.data` is re-pointed to (module.half().float() allocates the same size again) cannot land on the keyed address"""
    return tuple([p.detach() for p in params])


def adam_step(param, grad, exp_avg, exp_avg_sq, param_bf16, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              decoupled=False, step=1, grad_scale=1.0):
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1
    lib = _lib.load()
    check(lib.kalle_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(param_bf16), param.numel(), lr,
                              beta1, beta2, eps, weight_decay, int(decoupled), step, grad_scale, _stream()),
          "kalle_adam_step")


# gradient-norm clipping / non-finite skip, decided on the device (include/kalle_hip.h, "Gradient-norm clipping ...")
GRAD_NORM_PARTIALS = 1024          # KALLE_GRAD_NORM_PARTIALS / _BLOCK / _UNROLL: tests/test_grad_clip_cpu.py holds them to the header
GRAD_NORM_BLOCK = 256
GRAD_NORM_UNROLL = 4


class OptCtl:
    """`kalle_opt_ctl` as a small device tensor (`t`, 8 x int32) with named views: norm, coef (fp32), nonfinite, skip (int32),
    skipped, clipped (int64).  Reading a view is asynchronous like any tensor; `.item()` on one is a host sync."""

    def __init__(self, device):
        self.t = torch.zeros(8, device=device, dtype=torch.int32)
        self.norm = self.t[0:1].view(torch.float32)
        self.coef = self.t[1:2].view(torch.float32)
        self.nonfinite = self.t[2:3]
        self.skip = self.t[3:4]
        self.skipped = self.t[4:6].view(torch.int64)
        self.clipped = self.t[6:8].view(torch.int64)
        self.coef.fill_(1.0)


def grad_norm_ws(nslots, device):
    """workspace of `nslots` regions for grad_sumsq / grad_norm_finish (a uint8 tensor; layout: include/kalle_hip.h)"""
    nbytes = _lib.load().kalle_grad_norm_ws_bytes(int(nslots))
    check(min(nbytes, 0), "kalle_grad_norm_ws_bytes")
    return torch.zeros(nbytes, device=device, dtype=torch.uint8)


def grad_norm_ws_views(ws, nslots):
    """(sumsq [nslots, PARTIALS] float64, bad [nslots, PARTIALS] int32): read-only views of the workspace's stages"""
    r = ws.view(nslots, GRAD_NORM_PARTIALS * 12)
    return r[:, :GRAD_NORM_PARTIALS * 8].view(torch.float64), r[:, GRAD_NORM_PARTIALS * 8:].view(torch.int32)


def grad_sumsq(grad, ws, slot, nslots):
    """region `slot` of `ws` <- per-workgroup partial sums of grad^2 (double) and non-finite flags; grad: contiguous fp32"""
    assert grad.dtype == torch.float32 and grad.is_contiguous()
    check(_lib.load().kalle_grad_sumsq(_p(grad), grad.numel(), _p(ws), slot, nslots, _stream()), "kalle_grad_sumsq")


def grad_norm_finish(ws, nslots, ctl, *, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """ctl (OptCtl) <- norm of grad_scale * (all slots), clip coefficient for max_norm (0 / inf: none), skip decision, counters"""
    check(_lib.load().kalle_grad_norm_finish(_p(ws), nslots, grad_scale, max_norm, int(skip_nonfinite), _p(ctl.t), _stream()),
          "kalle_grad_norm_finish")


def adam_step_ctl(param, grad, exp_avg, exp_avg_sq, param_bf16, ctl, *, lr, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, decoupled=False, step=1, grad_scale=1.0):
    """adam_step with the gradient factor f32(grad_scale * ctl.coef), a no-op where ctl.skip is set - both read on the device"""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1
    lib = _lib.load()
    check(lib.kalle_adam_step_ctl(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(param_bf16), param.numel(), lr,
                                  beta1, beta2, eps, weight_decay, int(decoupled), step, grad_scale, _p(ctl.t), _stream()),
          "kalle_adam_step_ctl")


# ------------------------------------------------------------------------------------------------ attention
def attention_fwd(q, k, v, *, ldq, q_off, ldk, k_off, ldv, v_off, B, H, Hkv, Nq, Nk, rope=None, key_mask=None,
                  causal=False, dh=64):
    """q/k/v: base tensors (bf16) of the projection outputs; see kalle_attention_fwd_hd (dh = 32, 64 or 128).
    Returns (out [B,Nq,H*dh], lse)."""
    lib = _lib.load()
    out = torch.empty((B, Nq, H * dh), device=q.device, dtype=torch.bfloat16)
    lse = torch.empty((B, H, Nq), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    m8 = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    check(lib.kalle_attention_fwd_hd(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, _p(out), H * dh, _p(lse),
                                     _p(cos), _p(sin), rot, _p(m8), int(causal), B, H, Hkv, Nq, Nk, dh, _stream()),
          "kalle_attention_fwd_hd")
    return out, lse


def attention_decode(q, k, v, *, ldq, q_off, ldk, k_off, ldv, v_off, B, H, Hkv, Nk, rope=None, key_mask=None, dh=64):
    """one query per batch row (q [B][ldq], the LAST position) against Nk cached keys: kalle_attention_decode_hd.
    Returns (out [B,1,H*dh], lse [B,H,1])."""
    lib = _lib.load()
    out = torch.empty((B, 1, H * dh), device=q.device, dtype=torch.bfloat16)
    lse = torch.empty((B, H, 1), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    m8 = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    check(lib.kalle_attention_decode_hd(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, _p(out), H * dh, _p(lse),
                                        _p(cos), _p(sin), rot, _p(m8), B, H, Hkv, Nk, dh, _stream()),
          "kalle_attention_decode_hd")
    return out, lse


def attn_last_plan():
    """the calling thread's kalle_attn_last_plan word (encoding: include/kalle_hip.h)"""
    return _lib.load().kalle_attn_last_plan()


def attention_plan(entry, *, H, Hkv, B=1, Nq=1, Nk=1, dh=64, rot=0, causal=False, key_mask=False, nk=None, kv_row_stride=None,
                   seqs=None):
    """kalle_attention_fwd_plan / _bwd_plan / _decode_plan / _decode_rows_plan (entry "fwd", "bwd", "decode", "rows") and
    kalle_attention_fwd_varlen_plan / _bwd_varlen_plan ("fwd_varlen", "bwd_varlen": seqs = a Packed, which may have been made
    with device=None) for a call given by its shape, with placeholder pointers in dense layouts (q [H dh], k | v [2 Hkv dh] rows; the planner tests pointers for
    null only) and tables exactly when rot != 0; rows: nk host ints, kv_row_stride None = (max(nk) + 1) rows.  Returns (return
    code, dict(word = what kalle_attn_last_plan would hold after the call, family, launches = [dict(grid, block, lds)]), or None
    where the entry point refuses the call); host code only, no device needed"""
    lib = _lib.load()
    tab = 16 if rot else None
    head = (16, H * dh, 0, 16, 2 * Hkv * dh, 0, 16, 2 * Hkv * dh, Hkv * dh)
    tail = (tab, tab, rot, 16 if key_mask else None)
    plan = (ctypes.c_int32 * 12)()
    if entry == "fwd":
        rc = lib.kalle_attention_fwd_plan(*head, 16, H * dh, 16, *tail, int(causal), B, H, Hkv, Nq, Nk, dh, plan)
    elif entry == "bwd":
        rc = lib.kalle_attention_bwd_plan(*head, 16, 16, H * dh, 16, 16, 16, 16, 16, *tail, int(causal), B, H, Hkv, Nq, Nk, dh, plan)
    elif entry == "fwd_varlen":
        rc = lib.kalle_attention_fwd_varlen_plan(*head, 16, H * dh, 16, *tail[:3], *seqs._args(), H, Hkv, dh, plan)
    elif entry == "bwd_varlen":
        rc = lib.kalle_attention_bwd_varlen_plan(*head, 16, 16, H * dh, 16, 16, 16, 16, 16, *tail[:3], *seqs._args(), H, Hkv, dh, plan)
    elif entry == "decode":
        rc = lib.kalle_attention_decode_plan(*head, 16, H * dh, 16, *tail, B, H, Hkv, Nk, dh, plan)
    else:
        assert entry == "rows", entry
        stride = (max(max(nk), 0) + 1) * 2 * Hkv * dh if kv_row_stride is None else kv_row_stride
        rc = lib.kalle_attention_decode_rows_plan(*head, stride, 16, H * dh, 16, tab, tab, rot, ctypes.cast(_i32(nk), ctypes.c_void_p),
                                                  len(nk), H, Hkv, dh, plan)
    if rc != 0:
        return rc, None
    return rc, dict(word=plan[0], family=plan[0] & 15,
                    launches=[dict(grid=tuple(plan[2 + 5 * i:5 + 5 * i]), block=plan[5 + 5 * i], lds=plan[6 + 5 * i]) for i in range(plan[1])])


class Packed:
    """The sequences of a packed ragged batch for kalle_attention_fwd_varlen / _bwd_varlen: sequence b owns the packed rows
    row0[b] .. row0[b] + lens[b] - 1 of a buffer of total_rows rows (increasing, not overlapping; rows in between and behind
    belong to nobody).  row0 / lens: host ints (the planner reads them); dev: the same values as ONE device int32 tensor
    [2, nseq] (row0 | lens; the kernels read it) - made here from the host lists, so the two cannot disagree."""

    def __init__(self, row0, lens, total_rows, device, max_len=None):
        self.row0, self.lens = [int(r) for r in row0], [int(n) for n in lens]
        assert len(self.row0) == len(self.lens) >= 1
        self.nseq, self.total_rows = len(self.lens), int(total_rows)
        self.max_len = int(max_len) if max_len is not None else max(self.lens)
        self.live_rows = sum(self.lens)
        self.has_gaps = self.live_rows != self.total_rows       # rows outside every sequence: outputs start as zeros
        self.host = (_i32(self.row0), _i32(self.lens))
        self.dev = torch.tensor([self.row0, self.lens], dtype=torch.int32).to(device) if device is not None else None

    @classmethod
    def back_to_back(cls, lens, device, granule=1):
        """sequences packed back to back from row 0; total_rows = sum(lens) rounded up to a multiple of `granule`"""
        lens = [int(n) for n in lens]
        row0 = [sum(lens[:b]) for b in range(len(lens))]
        return cls(row0, lens, -(-sum(lens) // granule) * granule, device)

    def _args(self):
        cast = ctypes.cast
        d = self.dev
        if d is not None and not d.is_cuda:
            raise RuntimeError("kalle_audio_amd ops run on the GPU only (HIP kernels); got a CPU tensor")
        dev = (ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(d.data_ptr() + 4 * self.nseq)) if d is not None else (16, 16)
        return (self.nseq, cast(self.host[0], ctypes.c_void_p), cast(self.host[1], ctypes.c_void_p), *dev, self.total_rows,
                self.max_len)


def attention_fwd_varlen(q, k, v, seqs, *, ldq, q_off, ldk, k_off, ldv, v_off, H, Hkv, rope=None, dh=64):
    """causal attention of every sequence of `seqs` (a Packed) inside packed buffers: kalle_attention_fwd_varlen.
    Returns (out [total_rows, H*dh], lse [H * total_rows]: sequence b's [H][len] block at H * row0[b]); rows outside every
    sequence are zeros in both (torch.zeros; without such rows torch.empty as attention_fwd)."""
    lib = _lib.load()
    new = torch.zeros if seqs.has_gaps else torch.empty
    out = new((seqs.total_rows, H * dh), device=q.device, dtype=torch.bfloat16)
    lse = new((H * seqs.total_rows,), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    check(lib.kalle_attention_fwd_varlen(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, _p(out), H * dh, _p(lse),
                                         _p(cos), _p(sin), rot, *seqs._args(), H, Hkv, dh, _stream()),
          "kalle_attention_fwd_varlen")
    return out, lse


def kv_append_varlen(src, seqs, cache, dst_rows, t0, *, src_off):
    """kalle_kv_append_varlen: the k|v window (columns src_off .. src_off + kvw of the packed bf16 buffer src [total_rows, ld]) of
    every sequence of `seqs` (a Packed) goes to cache [R, cache_rows, kvw], sequence s to cache[dst_rows[s], t0[s] + j]; dst_rows /
    t0: host ints, one per sequence.  One launch, nothing else written.  Returns cache.
    A cache of more than DECODE_MAX_ROWS rows (the wide step's): one launch per block of 16 cache rows that receives a sequence,
    on that block's slice of the cache with the sequences that land in it (at most 16, in their packed order)."""
    lib = _lib.load()
    assert src.dtype == cache.dtype == torch.bfloat16 and src.dim() == 2 and src.stride(1) == 1 and src.shape[0] == seqs.total_rows
    assert cache.dim() == 3 and cache.stride(2) == 1 and cache.stride(1) == cache.shape[2]
    assert len(dst_rows) == len(t0) == seqs.nseq
    R, cache_rows, kvw = cache.shape
    cast = ctypes.cast
    if R > DECODE_MAX_ROWS and all(0 <= int(d) < R for d in dst_rows):
        for b0 in range(0, R, DECODE_MAX_ROWS):
            pick = [s for s, d in enumerate(dst_rows) if b0 <= int(d) < b0 + DECODE_MAX_ROWS]
            if not pick:
                continue
            block = cache[b0:b0 + DECODE_MAX_ROWS]
            check(lib.kalle_kv_append_varlen(_p(src), src.stride(0), src_off, _p(block), cache.stride(0), kvw, len(pick),
                                             cast(_i32([seqs.row0[s] for s in pick]), ctypes.c_void_p),
                                             cast(_i32([seqs.lens[s] for s in pick]), ctypes.c_void_p),
                                             cast(_i32([int(dst_rows[s]) - b0 for s in pick]), ctypes.c_void_p),
                                             cast(_i32([t0[s] for s in pick]), ctypes.c_void_p), seqs.total_rows, block.shape[0],
                                             cache_rows, _stream()), "kalle_kv_append_varlen")
        return cache
    check(lib.kalle_kv_append_varlen(_p(src), src.stride(0), src_off, _p(cache), cache.stride(0), kvw, seqs.nseq,
                                     cast(seqs.host[0], ctypes.c_void_p), cast(seqs.host[1], ctypes.c_void_p),
                                     cast(_i32(dst_rows), ctypes.c_void_p), cast(_i32(t0), ctypes.c_void_p), seqs.total_rows, R,
                                     cache_rows, _stream()), "kalle_kv_append_varlen")
    return cache


def attention_bwd_varlen(q, k, v, out, dout, lse, seqs, *, ldq, q_off, ldk, k_off, ldv, v_off, H, Hkv, rope=None, dh=64,
                         dq=None, dk=None, dv=None):
    """kalle_attention_bwd_varlen.  dq / dk / dv None: ONE new buffer shaped like q that receives all three (the fused qkv
    layout: q, k and v are windows of one tensor), zeros where `seqs` has rows outside every sequence so that the GEMMs behind
    read no uninitialised memory, torch.empty otherwise.  Returns (dq, dk, dv)."""
    lib = _lib.load()
    if dq is None:
        assert dk is None and dv is None and q.data_ptr() == k.data_ptr() == v.data_ptr()
        dq = dk = dv = (torch.zeros_like if seqs.has_gaps else torch.empty_like)(q)
    delta = torch.empty((H * seqs.total_rows,), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    check(lib.kalle_attention_bwd_varlen(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, _p(out), _p(dout), H * dh,
                                         _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(cos), _p(sin), rot, *seqs._args(),
                                         H, Hkv, dh, _stream()), "kalle_attention_bwd_varlen")
    return dq, dk, dv


def attention_bwd(q, k, v, out, dout, lse, dq, dk, dv, *, ldq, q_off, ldk, k_off, ldv, v_off, B, H, Hkv, Nq, Nk,
                  rope=None, key_mask=None, causal=False, dh=64):
    lib = _lib.load()
    delta = torch.empty((B, H, Nq), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    m8 = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    check(lib.kalle_attention_bwd_hd(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, _p(out), _p(dout), H * dh,
                                     _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(cos), _p(sin), rot, _p(m8),
                                     int(causal), B, H, Hkv, Nq, Nk, dh, _stream()), "kalle_attention_bwd_hd")


def head_norm_fwd(x, ldx, x_off, rows, heads, mode, gamma=None, beta=None, dh=64):
    """qk_norm (transformer.py:422-428) on the q or k slice of a projection output: returns (y bf16 [rows, heads*dh], stat)"""
    lib = _lib.load()
    y = torch.empty((rows, heads * dh), device=x.device, dtype=torch.bfloat16)
    stat = torch.empty((rows, heads, 2), device=x.device, dtype=torch.float32)
    if dh == 64:
        check(lib.kalle_head_norm_fwd(_p(x), ldx, x_off, _p(y), heads * 64, 0, _p(stat), _p(gamma), _p(beta), mode, rows, heads,
                                      _stream()), "kalle_head_norm_fwd")
    else:
        check(lib.kalle_head_norm_fwd_hd(_p(x), ldx, x_off, _p(y), heads * dh, 0, _p(stat), _p(gamma), _p(beta), mode, rows,
                                         heads, dh, _stream()), "kalle_head_norm_fwd_hd")
    return y, stat


def head_norm_bwd(x, ldx, x_off, stat, g, dx, lddx, dx_off, rows, heads, mode, gamma=None, dgamma=None, dbeta=None, dh=64):
    """g: bf16 [rows, heads*dh] gradient w.r.t. the normalised values; writes the gradient w.r.t. x into dx (ld / offset)"""
    lib = _lib.load()
    if dh == 64:
        check(lib.kalle_head_norm_bwd(_p(x), ldx, x_off, _p(stat), _p(g), heads * 64, 0, _p(dx), lddx, dx_off, _p(gamma),
                                      _p(dgamma), _p(dbeta), mode, rows, heads, _stream()), "kalle_head_norm_bwd")
    else:
        check(lib.kalle_head_norm_bwd_hd(_p(x), ldx, x_off, _p(stat), _p(g), heads * dh, 0, _p(dx), lddx, dx_off, _p(gamma),
                                         _p(dgamma), _p(dbeta), mode, rows, heads, dh, _stream()), "kalle_head_norm_bwd_hd")


# ------------------------------------------------------------------------------------------------ Llasa head / tail
def peak_normalize_int16(x):
    """int16(clamp(x / max|x|, -1, 1) * 32767) (infer_0723.py:293); returns (int16 tensor of x's shape, peak [1] fp32)"""
    lib = _lib.load()
    x = x.contiguous()
    peak = torch.empty(1, device=x.device, dtype=torch.float32)
    out = torch.empty(x.shape, device=x.device, dtype=torch.int16)
    check(lib.kalle_peak_normalize_int16(_p(x), _dt(x), _p(peak), _p(out), x.numel(), _stream()),
          "kalle_peak_normalize_int16")
    return out, peak


def axpby(x, y, a, b, out=None):
    """out = a x + b y (fp32); out may alias x or y"""
    lib = _lib.load()
    x, y = x.contiguous(), y.contiguous()
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.shape == y.shape
    out = torch.empty_like(x) if out is None else out
    check(lib.kalle_axpby(_p(x), _p(y), _p(out), float(a), float(b), x.numel(), _stream()), "kalle_axpby")
    return out


def add_rows(x, table):
    """x[b] += table for every batch element b, in place (transformer.py:796-797); x fp32 [B, ...] contiguous, table fp32 with
    the element count of x[0]"""
    lib = _lib.load()
    assert x.dtype == torch.float32 and table.dtype == torch.float32 and x.is_contiguous() and table.is_contiguous()
    assert x[0].numel() == table.numel()
    check(lib.kalle_add_rows(_p(x), _p(table), x.shape[0], table.numel(), _stream()), "kalle_add_rows")
    return x


def dwconv1d(x, w, B, N, out_dtype, pad, flip=False):
    """depthwise conv along the sequence of token-major bf16 activations [B * N, D] (ConformerModule, transformer.py:564);
    w fp32 [D, K]; flip=True with pad = K - 1 - padding is the data gradient"""
    lib = _lib.load()
    D, K = w.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous()
    assert x.numel() == B * N * D
    y = torch.empty((B * N, D), device=x.device, dtype=out_dtype)
    check(lib.kalle_dwconv1d_fwd(_p(x), _p(w), _p(y), _dt(y), B, N, D, K, pad, int(flip), _stream()), "kalle_dwconv1d_fwd")
    return y


def dwconv1d_wgrad(dy, x, dw, B, N, pad):
    """dw [D, K] fp32 += sum_{b, n} dy[b, n, :, None] * x[b, n + k - pad, :, None]   (atomic adds)"""
    lib = _lib.load()
    D, K = dw.shape
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.dtype == torch.float32
    assert dy.is_contiguous() and x.is_contiguous() and dw.is_contiguous() and dy.numel() == B * N * D == x.numel()
    check(lib.kalle_dwconv1d_wgrad(_p(dy), _p(x), _p(dw), B, N, D, K, pad, _stream()), "kalle_dwconv1d_wgrad")
    return dw


def embed_mix_fwd(ids, table, audio, ids_mask, audio_mask):
    """ids [rows] int64, table fp32 [V, D], audio fp32/bf16 [rows, D], masks fp32 [rows] -> fp32 [rows, D]"""
    lib = _lib.load()
    rows, D = audio.shape
    out = torch.empty((rows, D), device=audio.device, dtype=torch.float32)
    check(lib.kalle_embed_mix_fwd(_p(ids), _p(table), _p(audio), _dt(audio), _p(ids_mask), _p(audio_mask), _p(out), rows, D,
                                  table.shape[0], _stream()), "kalle_embed_mix_fwd")
    return out


def embed_mix_bwd(dout, ids, ids_mask, audio_mask, dtable=None, want_daudio=True):
    lib = _lib.load()
    rows, D = dout.shape
    daudio = torch.empty((rows, D), device=dout.device, dtype=torch.float32) if want_daudio else None
    V = dtable.shape[0] if dtable is not None else 1
    check(lib.kalle_embed_mix_bwd(_p(dout), _p(ids), _p(ids_mask), _p(audio_mask), _p(dtable), _p(daudio), rows, D, V,
                                  _stream()), "kalle_embed_mix_bwd")
    return daudio


def gelu_fwd(x):
    lib = _lib.load()
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib.kalle_gelu_fwd(_p(x), _p(y), _dt(x), x.numel(), _stream()), "kalle_gelu_fwd")
    return y


def gelu_bwd(dy, x):
    lib = _lib.load()
    dy = dy.contiguous()
    assert dy.dtype == x.dtype
    dx = torch.empty_like(x)
    check(lib.kalle_gelu_bwd(_p(dy), _p(x), _p(dx), _dt(x), x.numel(), _stream()), "kalle_gelu_bwd")
    return dx


def gauss_kl_fwd(pred, label, mask_a, mask_b, std):
    """returns sums4 = [sum kl*ma, sum ma, sum kl*mb, sum mb] (fp32, device)"""
    lib = _lib.load()
    rows, d = pred.shape
    sums = torch.zeros(4, device=pred.device, dtype=torch.float32)
    check(lib.kalle_gauss_kl_fwd(_p(pred), _p(label), _p(mask_a), _p(mask_b), _p(sums), float(std), rows, d, _stream()),
          "kalle_gauss_kl_fwd")
    return sums


def gauss_kl_bwd(pred, label, mask_a, mask_b, sums, grad_a, grad_b, std):
    lib = _lib.load()
    rows, d = pred.shape
    dpred = torch.empty_like(pred)
    check(lib.kalle_gauss_kl_bwd(_p(pred), _p(label), _p(mask_a), _p(mask_b), _p(sums), _p(grad_a), _p(grad_b), _p(dpred),
                                 float(std), rows, d, _stream()), "kalle_gauss_kl_bwd")
    return dpred


# ---- KV-cached decoding (include/kalle_hip.h): one row or R <= DECODE_MAX_ROWS sequences per step, bf16 weights or uint8 OCP
# e4m3fn codes [N, K] + one fp32 scale per output row
DECODE_MAX_ROWS = 16
DECODE_WIDE_MAX_ROWS = 64        # the wide step (kalle_llama_decode_step_wide): bf16 layers only
BF16_FIELDS = ("input_norm", "wqkv", "wo", "post_norm", "wug", "wdown", "kv_cache")
W8_FIELDS = ("input_norm", "wqkv", "sqkv", "wo", "so", "post_norm", "wug", "sug", "wdown", "sdown", "kv_cache")
_DECODE_STEP = {(False, False): "kalle_llama_decode_step_hd", (False, True): "kalle_llama_decode_step_w8",      # (R-row, e4m3)
                (True, False): "kalle_llama_decode_step_rows", (True, True): "kalle_llama_decode_step_rows_w8"}


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _proj_args(x, w, wdtype, scale, residual, yshape):
    """the assertions the GEMV / skinny-GEMM wrappers share: x bf16 [.., K] against w [N, K] (+ scale fp32 [N]), residual fp32"""
    assert w.dim() == 2 and w.stride(1) == 1 and w.dtype == wdtype and x.shape[-1] == w.shape[1]
    assert x.dtype == torch.bfloat16 and x.stride(-1) == 1
    if scale is not None:
        assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],) and scale.is_contiguous()
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == yshape and residual.stride(-1) == 1


def gemm_rows(x, w, *, residual=None, out_dtype=torch.float32):
    """Y[r] = W . x[r] (+ residual[r]) for the R <= 16 rows of x (bf16 [R, K], rows may be strided); W bf16 [N, K] is read once
    for all rows: kalle_gemm_rows_bf16"""
    lib = _lib.load()
    assert x.dim() == 2
    R, K = x.shape
    y = torch.empty((R, w.shape[0]), device=x.device, dtype=out_dtype)
    _proj_args(x, w, torch.bfloat16, None, residual, y.shape)
    check(lib.kalle_gemm_rows_bf16(_p(x), x.stride(0), _p(w), w.stride(0), _p(y), y.stride(0), _dt(y), _p(residual),
                                   residual.stride(0) if residual is not None else 0, R, w.shape[0], K, _stream()),
          "kalle_gemm_rows_bf16")
    return y


def gemm_rows_wide(x, w, *, residual=None, out_dtype=torch.float32):
    """gemm_rows for the R <= 64 rows of x: kalle_gemm_rows_wide without a prologue (up to 16 rows it is gemm_rows' kernel; a
    row's bits are the same either way)"""
    lib = _lib.load()
    assert x.dim() == 2
    R, K = x.shape
    N = w.shape[0]
    y = torch.empty((R, N), device=x.device, dtype=out_dtype)
    _proj_args(x, w, torch.bfloat16, None, residual, y.shape)
    check(lib.kalle_gemm_rows_wide(_p(x), x.stride(0), 0, None, 0.0, None, _p(w), w.stride(0), _p(y), y.stride(0), _dt(y), None, N,
                                   None, _p(residual), residual.stride(0) if residual is not None else 0, None, R, N, K,
                                   _stream()), "kalle_gemm_rows_wide")
    return y


def attention_decode_rows(q, k, v, nk, *, ldq, q_off, ldk, k_off, ldv, v_off, kv_row_stride, H, Hkv, rope=None, dh=64):
    """one query per row r (q [R][ldq]) at position nk[r] - 1 against the nk[r] keys of row r's own cache (k + r * kv_row_stride);
    nk: host ints, <= 0 = inactive row (its out / lse rows are not written): kalle_attention_decode_rows.
    Returns (out [R, 1, H*dh], lse [R, H, 1])."""
    lib = _lib.load()
    R = len(nk)
    out = torch.empty((R, 1, H * dh), device=q.device, dtype=torch.bfloat16)
    lse = torch.empty((R, H, 1), device=q.device, dtype=torch.float32)
    cos, sin, rot = (rope[0], rope[1], rope[0].shape[-1] * 2) if rope is not None else (None, None, 0)
    check(lib.kalle_attention_decode_rows(_p(q), ldq, q_off, _p(k), ldk, k_off, _p(v), ldv, v_off, kv_row_stride, _p(out), H * dh,
                                          _p(lse), _p(cos), _p(sin), rot, ctypes.cast(_i32(nk), ctypes.c_void_p), R, H, Hkv, dh,
                                          _stream()), "kalle_attention_decode_rows")
    return out, lse


def quantize_rows_e4m3(w):
    """w bf16 [N, K] (rows may be strided, K % 16 == 0) -> (w8 uint8 [N, K], scale fp32 [N]): kalle_quantize_rows_e4m3"""
    lib = _lib.load()
    assert w.dim() == 2 and w.stride(1) == 1 and w.dtype == torch.bfloat16
    N, K = w.shape
    w8 = torch.empty((N, K), device=w.device, dtype=torch.uint8)
    scale = torch.empty((N,), device=w.device, dtype=torch.float32)
    check(lib.kalle_quantize_rows_e4m3(_p(w), w.stride(0), _p(w8), K, _p(scale), N, K, _stream()), "kalle_quantize_rows_e4m3")
    return w8, scale


def gemv_e4m3(x, w8, scale, *, residual=None, out_dtype=torch.float32):
    """y = scale * (e4m3(w8) . x) (+ residual) for one bf16 row x [K]: kalle_gemv_e4m3"""
    lib = _lib.load()
    assert x.dim() == 1
    N, K = w8.shape
    y = torch.empty((N,), device=x.device, dtype=out_dtype)
    _proj_args(x, w8, torch.uint8, scale, residual, y.shape)
    check(lib.kalle_gemv_e4m3(_p(x), _p(w8), w8.stride(0), _p(scale), _p(y), _dt(y), _p(residual), N, K, _stream()),
          "kalle_gemv_e4m3")
    return y


def gemm_rows_e4m3(x, w8, scale, *, residual=None, out_dtype=torch.float32):
    """gemm_rows on e4m3 weights: Y[r] = scale * (e4m3(w8) . x[r]) (+ residual[r]) for the R <= 16 rows of x (bf16 [R, K]):
    kalle_gemm_rows_fused_e4m3 without a prologue"""
    lib = _lib.load()
    assert x.dim() == 2
    R, K = x.shape
    N = w8.shape[0]
    y = torch.empty((R, N), device=x.device, dtype=out_dtype)
    _proj_args(x, w8, torch.uint8, scale, residual, y.shape)
    check(lib.kalle_gemm_rows_fused_e4m3(_p(x), x.stride(0), 0, None, 0.0, None, _p(w8), w8.stride(0), _p(scale), _p(y),
                                         y.stride(0), _dt(y), None, N, None, _p(residual),
                                         residual.stride(0) if residual is not None else 0, None, R, N, K, _stream()),
          "kalle_gemm_rows_fused_e4m3")
    return y


def llama_decode_plan(layer_tensors, H, Hkv, inner, device, head_dim=64, rows=None):
    """The host-side descriptor array + workspace of the decode step (keeps the tensors alive).  layer_tensors: per layer the
    tensors of BF16_FIELDS (input_norm fp32, wqkv bf16, wo bf16, post_norm fp32, wug bf16, wdown bf16, kv_cache bf16) or of
    W8_FIELDS (each weight uint8 and followed by its fp32 scale, the pairs as quantize_rows_e4m3 returns them); the tuple length
    tells which.  rows = R: the R-row step, kv_cache of a layer is bf16 [R, cache_rows, 2*Hkv*head_dim]; R above DECODE_MAX_ROWS
    (up to DECODE_WIDE_MAX_ROWS): the wide step, bf16 layers only."""
    lib = _lib.load()
    nf = len(layer_tensors[0])
    assert nf in (len(BF16_FIELDS), len(W8_FIELDS)), f"a layer is {len(BF16_FIELDS)} (bf16) or {len(W8_FIELDS)} (e4m3) tensors"
    w8 = nf == len(W8_FIELDS)
    fields, desc = (W8_FIELDS, _lib.LlamaLayerW8) if w8 else (BF16_FIELDS, _lib.LlamaLayer)
    arr = (desc * len(layer_tensors))()
    for d, ts in zip(arr, layer_tensors):
        assert len(ts) == nf
        for f, t in zip(fields, ts):
            assert t.is_contiguous() and t.device == torch.device(device)
            setattr(d, f, t.data_ptr())
        if rows is not None:
            assert ts[-1].dim() == 3 and ts[-1].shape[0] == rows
    wide = rows is not None and rows > DECODE_MAX_ROWS
    if wide and w8:
        raise NotImplementedError(f"e4m3 layers with more than {DECODE_MAX_ROWS} rows ({rows}): there is no wide e4m3 step")
    if rows is None:
        nbytes, what = lib.kalle_llama_decode_ws_bytes_hd(H, Hkv, inner, head_dim), "kalle_llama_decode_ws_bytes_hd"
    elif wide:
        nbytes, what = lib.kalle_llama_decode_ws_bytes_wide(rows, H, Hkv, inner, head_dim), "kalle_llama_decode_ws_bytes_wide"
    else:
        nbytes, what = lib.kalle_llama_decode_ws_bytes_rows(rows, H, Hkv, inner, head_dim), "kalle_llama_decode_ws_bytes_rows"
    check(min(nbytes, 0), what)
    plan = {"layers": arr, "n": len(layer_tensors), "keep": layer_tensors, "ws": torch.empty(nbytes, device=device, dtype=torch.uint8),
            "H": H, "Hkv": Hkv, "inner": inner, "head_dim": head_dim,
            "step": "kalle_llama_decode_step_wide" if wide else _DECODE_STEP[rows is not None, w8]}
    if rows is not None:
        plan["R"] = rows
    if w8:
        plan["fmt"] = "e4m3"
    return plan


def llama_decode_step(plan, x, t0, cache_rows, rope, eps):
    """every decoder layer at the new position against the KV caches of `plan`, one host call (the entry point is the plan's).
    One-row plan: x fp32 [D], t0 an int -> a fresh fp32 [D].  R-row plan: x fp32 [R, D], t0 R host ints (negative = inactive
    row) -> fp32 [R, D], the plan's own buffer, reused by the next step: an inactive row keeps what its last active step left
    there (zeros before the first)"""
    lib = _lib.load()
    R = plan.get("R")
    if R is None:
        out, rows, pos = torch.empty_like(x), (), t0
    else:
        assert x.shape[0] == R == len(t0) and x.is_contiguous() and x.dtype == torch.float32
        out = plan.get("out")
        if out is None:
            out = plan["out"] = torch.zeros_like(x)
        rows, pos = (R,), ctypes.cast(_i32(t0), ctypes.c_void_p)
    check(getattr(lib, plan["step"])(ctypes.cast(plan["layers"], ctypes.c_void_p), plan["n"], _p(x), _p(out), *rows, plan["H"],
                                     plan["Hkv"], plan["inner"], plan["head_dim"], eps, pos, cache_rows, _p(rope[0]),
                                     _p(rope[1]), _p(plan["ws"]), _stream()), plan["step"])
    return out


# ---- the per-frame head of KV-cached generation (kalle_llasa_frame_head_rows): final norm, distribution_linear, sample, stop KL,
# audio_linear in one host call
HEAD_FIELDS = ("norm", "w1", "b1", "w2", "b2", "wa", "ba")
HEAD_MAX_LATENT = 512


def _head_chunks(ws_bytes, R, what):
    """the head entry points serve up to DECODE_MAX_ROWS rows (a workgroup per row): more rows (up to DECODE_WIDE_MAX_ROWS) run as
    one call per chunk of up to 16 rows on row slices, so a row's bits are those of the 16-row call.  Returns ([(first row, rows,
    workspace offset)], workspace bytes: the sum of the chunks')"""
    if R <= DECODE_MAX_ROWS or R > DECODE_WIDE_MAX_ROWS:      # (one chunk, or too many rows: the library's own size and refusal)
        nbytes = ws_bytes(R)
        check(min(nbytes, 0), what)
        return [(0, R, 0)], nbytes
    chunks, off = [], 0
    for r0 in range(0, R, DECODE_MAX_ROWS):
        rn = min(DECODE_MAX_ROWS, R - r0)
        nbytes = ws_bytes(rn)
        check(min(nbytes, 0), what)
        chunks.append((r0, rn, off))
        off += (nbytes + 63) & ~63
    return chunks, off


def llasa_head_plan(norm, w1, b1, w2, b2, wa, ba, R, eps, device, frames=1):
    """The descriptor, workspace and output buffers of the frame head for R rows.  The seven arguments are the PARAMETERS (final
    RMSNorm weight [D], distribution_linear[0] weight [dl, D] / bias, distribution_linear[2] weight [dl, dl] / bias, audio_linear
    weight [D, dl] / bias): every call reads the weights' bf16 compute copies through dit_ops.bf16_of, so a changed weight is
    picked up at the next frame.  frames: how many frames of `latent` [frames, R, dl] and `kl` [frames, R] the plan keeps (the head
    writes frame i into slot i); `mean` [R, dl] and `x_next` [R, D] are rewritten by every call."""
    lib = _lib.load()
    dl, D = w1.shape
    assert tuple(w2.shape) == (dl, dl) and tuple(wa.shape) == (D, dl) and norm.shape[0] == D
    chunks, nbytes = _head_chunks(lambda rn: lib.kalle_llasa_head_ws_bytes(rn, D, dl), R, "kalle_llasa_head_ws_bytes")
    f32 = dict(device=device, dtype=torch.float32)
    return {"params": (norm, w1, b1, w2, b2, wa, ba), "desc": _lib.LlasaHead(), "keep": None, "R": R, "D": D, "dl": dl,
            "chunks": chunks, "eps": float(eps), "frames": frames, "ws": torch.empty(nbytes, device=device, dtype=torch.uint8),
            "mean": torch.zeros((R, dl), **f32), "latent": torch.zeros((frames, R, dl), **f32),
            "kl": torch.zeros((frames, R), **f32), "x_next": torch.zeros((R, D), **f32)}


def _head_call(plan, h, noise, lat, lds, active, frame):
    """what llasa_frame_head and llasa_frame_head2 share: the argument checks, the descriptor filled from the parameters' compute
    copies (kept alive in the plan until the next call) with the leading dimensions `lds` of w1 / w2 / wa, the active flags"""
    from .dit_ops import bf16_of, f32_of
    R, D = plan["R"], plan["D"]
    assert h.dtype == torch.float32 and tuple(h.shape) == (R, D) and h.stride(1) == 1
    assert noise.dtype == torch.float32 and tuple(noise.shape) == (R, lat) and noise.stride(1) == 1
    assert 0 <= frame < plan["frames"]
    desc = plan["desc"]
    keep = [bf16_of(p) if f[0] == "w" else f32_of(p) for f, p in zip(HEAD_FIELDS, plan["params"])]
    for f, t in zip(HEAD_FIELDS, keep):
        assert t.is_contiguous() and t.device == h.device
        setattr(desc, f, t.data_ptr())
    desc.ldw1, desc.ldw2, desc.ldwa = lds
    plan["keep"] = keep
    # per chunk of up to 16 rows: (first row, rows, workspace, that chunk's active flags or None); of SEVERAL chunks one with no
    # active row is left out (a single chunk is always called, as it was before there were chunks)
    calls, single = [], len(plan["chunks"]) == 1
    for r0, rn, off in plan["chunks"]:
        act = None if active is None else [1 if a else 0 for a in active[r0:r0 + rn]]
        if single or act is None or any(act):
            calls.append((r0, rn, plan["ws"][off:], None if act is None else ctypes.cast(_i32(act), ctypes.c_void_p)))
    return desc, calls


def llasa_frame_head(plan, h, noise, std, active=None, frame=0):
    """one frame's head, one host call.  h: the UN-NORMED residual stream, fp32 [R, D] (rows may be strided); noise fp32 [R, dl]
    (rows may be strided); active: R host booleans (None: all) - an inactive row's outputs are not touched.  Returns
    (mean [R, dl], latent [R, dl], kl [R], x_next [R, D]): views of the plan's buffers, latent and kl those of slot `frame`."""
    lib = _lib.load()
    R, D, dl = plan["R"], plan["D"], plan["dl"]
    desc, calls = _head_call(plan, h, noise, dl, (D, dl, dl), active, frame)
    latent, kl = plan["latent"][frame], plan["kl"][frame]
    for r0, rn, ws, act in calls:
        check(lib.kalle_llasa_frame_head_rows(ctypes.addressof(desc), _p(h[r0:]), h.stride(0), _p(noise[r0:]), noise.stride(0),
                                              float(std), plan["eps"], _p(plan["mean"][r0:]), _p(latent[r0:]), _p(kl[r0:]),
                                              _p(plan["x_next"][r0:]), act, rn, D, dl, _p(ws), _stream()),
              "kalle_llasa_frame_head_rows")
    return plan["mean"], latent, kl, plan["x_next"]


# ---- the same for the head that predicts mean || log-scale (kalle_llasa_frame_head2_rows; model.Llasa)
HEAD2_MAX_LATENT = 256


def llasa_head2_plan(norm, w1, b1, w2, b2, wa, ba, R, eps, device, frames=1):
    """llasa_head_plan for the mean || log-scale head: distribution_linear[0] weight [2 lat, D], distribution_linear[2] weight
    [2 lat, 2 lat], audio_linear weight [D, lat].  The plan keeps `disp` [frames, R, 2 lat] (mean || log-scale, what `infer`
    returns), `latent` [frames, R, lat] and `kl` [frames, R] (the head writes frame i into slot i); `x_next` [R, D] is
    rewritten by every call.  The weights are read through dit_ops.bf16_of / f32_of at every call."""
    lib = _lib.load()
    d2, D = w1.shape
    lat = d2 // 2
    assert d2 == 2 * lat and tuple(w2.shape) == (d2, d2) and tuple(wa.shape) == (D, lat) and norm.shape[0] == D
    chunks, nbytes = _head_chunks(lambda rn: lib.kalle_llasa_head2_ws_bytes(rn, D, lat), R, "kalle_llasa_head2_ws_bytes")
    f32 = dict(device=device, dtype=torch.float32)
    return {"params": (norm, w1, b1, w2, b2, wa, ba), "desc": _lib.LlasaHead(), "keep": None, "R": R, "D": D, "lat": lat,
            "chunks": chunks, "eps": float(eps), "frames": frames, "ws": torch.empty(nbytes, device=device, dtype=torch.uint8),
            "disp": torch.zeros((frames, R, d2), **f32), "latent": torch.zeros((frames, R, lat), **f32),
            "kl": torch.zeros((frames, R), **f32), "x_next": torch.zeros((R, D), **f32)}


def llasa_frame_head2(plan, h, noise, active=None, frame=0):
    """one frame's head, one host call.  h: the UN-NORMED residual stream, fp32 [R, D] (rows may be strided); noise fp32 [R, lat]
    (rows may be strided); active: R host booleans (None: all) - an inactive row's outputs are not touched.  Returns
    (disp [R, 2 lat], latent [R, lat], kl [R], x_next [R, D]): views of the plan's buffers, the first three those of slot `frame`."""
    lib = _lib.load()
    R, D, lat = plan["R"], plan["D"], plan["lat"]
    desc, calls = _head_call(plan, h, noise, lat, (D, 2 * lat, lat), active, frame)
    disp, latent, kl = plan["disp"][frame], plan["latent"][frame], plan["kl"][frame]
    for r0, rn, ws, act in calls:
        check(lib.kalle_llasa_frame_head2_rows(ctypes.addressof(desc), _p(h[r0:]), h.stride(0), _p(noise[r0:]), noise.stride(0),
                                               plan["eps"], _p(disp[r0:]), _p(latent[r0:]), _p(kl[r0:]), _p(plan["x_next"][r0:]),
                                               act, rn, D, lat, _p(ws), _stream()), "kalle_llasa_frame_head2_rows")
    return disp, latent, kl, plan["x_next"]


def gauss_kl2_fwd(pred, label_mean, label_std, mask_a, mask_b, std_mult=1.25):
    """two-Gaussian KL (model.py:84-100); label_std None -> label_mean is the raw mean | scale label [rows, 2 dim]"""
    lib = _lib.load()
    rows, d2 = pred.shape
    sums = torch.zeros(4, device=pred.device, dtype=torch.float32)
    check(lib.kalle_gauss_kl2_fwd(_p(pred), _p(label_mean), _p(label_std), 0 if label_std is not None else 1, float(std_mult),
                                  _p(mask_a), _p(mask_b), _p(sums), rows, d2 // 2, _stream()), "kalle_gauss_kl2_fwd")
    return sums


def gauss_kl2_bwd(pred, label_mean, label_std, mask_a, mask_b, sums, grad_a, grad_b, std_mult=1.25):
    lib = _lib.load()
    rows, d2 = pred.shape
    dpred = torch.empty_like(pred)
    check(lib.kalle_gauss_kl2_bwd(_p(pred), _p(label_mean), _p(label_std), 0 if label_std is not None else 1, float(std_mult),
                                  _p(mask_a), _p(mask_b), _p(sums), _p(grad_a), _p(grad_b), _p(dpred), rows, d2 // 2,
                                  _stream()), "kalle_gauss_kl2_bwd")
    return dpred


def segment_copy(src, dst, src_off, dst_off, lens, nbatch, rows, *, src_strides, dst_strides):
    """kalle_segment_copy: per segment s, dst[s, b, c, dst_off[s] + j] = src[s, b, c, src_off[s] + j], j < lens[s]; strides =
    (segment, batch, row) in elements; every segment in one launch (groups of KALLE_MAX_SEGMENTS)"""
    lib = _lib.load()
    assert src.dtype == dst.dtype
    MAXS = 64
    esz = src.element_size()
    for g in range(0, len(lens), MAXS):
        n = min(MAXS, len(lens) - g)
        so = (ctypes.c_int64 * n)(*[int(v) for v in src_off[g:g + n]])
        do = (ctypes.c_int64 * n)(*[int(v) for v in dst_off[g:g + n]])
        ln = (ctypes.c_int * n)(*[int(v) for v in lens[g:g + n]])
        sp = ctypes.c_void_p(src.data_ptr() + g * src_strides[0] * esz)
        dp = ctypes.c_void_p(dst.data_ptr() + g * dst_strides[0] * esz)
        if not src.is_cuda or not dst.is_cuda:
            raise RuntimeError("kalle_audio_amd ops run on the GPU only (HIP kernels); got a CPU tensor")
        check(lib.kalle_segment_copy(sp, dp, _dt(src), n, so, do, ln, nbatch, rows, src_strides[0], src_strides[1],
                                     src_strides[2], dst_strides[0], dst_strides[1], dst_strides[2], _stream()),
              "kalle_segment_copy")
    return dst


MAX_GROUP = 8
WGRAD_PLAN_FIELDS = ("tiles", "whole", "slices", "cleared", "cached")


def _wgrad_problems(shapes):
    """(tokens, N, K) triples as a kalle_wgrad_problem array with placeholder pointers, for the host query"""
    arr = (_lib.WgradProblem * len(shapes))()
    for w, (tokens, n, k) in zip(arr, shapes):
        w.dy = w.x = w.dw = 16
        w.lddy, w.ldx, w.lddw, w.N, w.K, w.tokens = n, k, k, n, k, tokens
    return arr


def wgrad_group_plan(shapes, overwrite=False):
    """kalle_gemm_wgrad_group_plan for problems given as (tokens, N, K): the plan kalle_gemm_wgrad_group would run now on this
    thread, as a dict of WGRAD_PLAN_FIELDS (encoding: include/kalle_hip.h); host code only, no device needed"""
    out = (ctypes.c_int * 5)()
    arr = _wgrad_problems(shapes)
    check(_lib.load().kalle_gemm_wgrad_group_plan(ctypes.cast(arr, ctypes.c_void_p), len(shapes), int(bool(overwrite)),
                                                  ctypes.cast(out, ctypes.c_void_p)), "kalle_gemm_wgrad_group_plan")
    return dict(zip(WGRAD_PLAN_FIELDS, out))


def wgrad_group_last_plan():
    """the calling thread's kalle_gemm_wgrad_group_last_plan as a dict of WGRAD_PLAN_FIELDS"""
    out = (ctypes.c_int * 5)()
    check(_lib.load().kalle_gemm_wgrad_group_last_plan(ctypes.cast(out, ctypes.c_void_p)), "kalle_gemm_wgrad_group_last_plan")
    return dict(zip(WGRAD_PLAN_FIELDS, out))


def gemm_wgrad_group(problems, overwrite=False):
    """problems: list of (dy bf16 [tokens, N], x bf16 [tokens, K], dw fp32 [N, K]); dw += dy^T x (overwrite: dw = dy^T x) for
    all of them in one launch per 8.  Returns False (nothing launched) when the shapes are outside the grouped kernel's domain."""
    lib = _lib.load()
    for dy, x, dw in problems:
        if dy.shape[0] % 8 or dy.shape[0] != x.shape[0] or dy.shape[1] % 8 or x.shape[1] % 8:
            return False
        assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.dtype == torch.float32
        assert dy.stride(-1) == 1 and x.stride(-1) == 1 and dw.stride(-1) == 1
    prof = KERNEL_TIMER if KERNEL_TIMER_ONLY in (None, "gemm3_wgrad_group_kernel") else None
    for g in range(0, len(problems), MAX_GROUP):
        grp = problems[g:g + MAX_GROUP]
        arr = (_lib.WgradProblem * len(grp))()
        flops = abytes = 0.0
        for w, (dy, x, dw) in zip(arr, grp):
            w.dy, w.lddy, w.x, w.ldx, w.dw, w.lddw = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0)
            w.N, w.K, w.tokens = dy.shape[1], x.shape[1], dy.shape[0]
            _p(dy), _p(x), _p(dw)                                     # (CPU tensors raise)
            flops += 2.0 * dy.shape[0] * dy.shape[1] * x.shape[1]
            abytes += 2.0 * dy.shape[0] * (dy.shape[1] + x.shape[1]) + 8.0 * dy.shape[1] * x.shape[1]
        if prof is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        rc = lib.kalle_gemm_wgrad_group(ctypes.cast(arr, ctypes.c_void_p), len(grp), int(bool(overwrite)), _stream())
        if rc == -3 and g == 0:
            return False
        check(rc, "kalle_gemm_wgrad_group")
        if prof is not None:
            e1.record()
            prof.append(("gemm3_wgrad_group_kernel", flops, e0, e1, abytes, (len(grp), 0, grp[0][0].shape[0])))
    return True
