"""Tensor-level wrappers for the VAE conv kernels (csrc/conv1d.hip). GPU tensors only, no fallback."""
import ctypes
import os

import torch

from . import _lib
from ._lib import check
from .ops import _dt, _p, _stream


def weight_norm_fold(v, g, transposed=False):
    """v: Conv1d [Cout,Cin,K] (or ConvTranspose1d [Cin,Cout,K] when transposed), g: [dim0] or None.
    Returns the packed fp32 weight [Cin][K][roundup(Cout, 8)] (pad columns zero)."""
    lib = _lib.load()
    v = v.detach().float().contiguous()
    d0, d1, K = v.shape
    cin, cout = (d0, d1) if transposed else (d1, d0)
    gg = g.detach().float().contiguous().view(-1) if g is not None else None
    w = torch.empty((cin, K, (cout + 7) // 8 * 8), device=v.device, dtype=torch.float32)   # Cout padded to 8
    check(lib.kalle_weight_norm_fold(_p(v), _p(gg), _p(w), d0, d1, K, int(transposed), _stream()),
          "kalle_weight_norm_fold")
    return w


def _act_struct(code, alpha, beta, logscale, param):
    return _lib.Act(int(code), int(bool(logscale)), _p(alpha), _p(beta), float(param))


def _epilogue(residual, out_scale, accumulate, tanh, post_act, y_raw=None):
    """post_act: None or (code, alpha, beta, logscale, param) - the next layer's input activation, applied at the store;
    y_raw: optional tensor that also receives the un-activated value"""
    pa = _act_struct(*post_act) if post_act is not None else _lib.Act(0, 0, None, None, 0.0)
    return _lib.ConvEpilogue(_p(residual), float(out_scale), int(accumulate), int(tanh), pa, _p(y_raw))


def _prefer():
    """KALLE_CONV_CFIRST -> the queries' `prefer`: unset = auto, "1" = the channels-per-lane kernels wherever eligible, else never"""
    want = os.environ.get("KALLE_CONV_CFIRST")
    return 0 if want is None else 1 if want == "1" else 2


_PLANS = {}     # answers of the plan queries: a model asks for the same few layers again and again, and a query costs 4 us more than a lookup


def _query(fn, what, ia, ep, *shape):
    """(family, word, Lp, lead, phases, workspace floats) of a plan query, kept per distinct call: the key is every argument,
    with every field of ia / ep, pointers as set / null (all the planners may do with them: include/kalle_hip.h)"""
    pa, prefer = ep.post_act, _prefer()
    key = (what, prefer, shape, ia.code, ia.logscale, ia.alpha is None, ia.beta is None, ia.param, ep.residual is None, ep.out_scale,
           ep.accumulate, ep.tanh, pa.code, pa.logscale, pa.alpha is None, pa.beta is None, pa.param, ep.y_raw is None)
    hit = _PLANS.get(key)
    if hit is None:
        out = (ctypes.c_int32 * 6)()
        check(fn(*shape, ctypes.addressof(ia), ctypes.addressof(ep), prefer, out), what)
        if len(_PLANS) >= 4096:
            _PLANS.clear()
        hit = _PLANS[key] = tuple(out)
    return hit


def _plan(fn, args, act, act_params, epilogue, prefer, x_f32, y_f32):
    """(return code, None or dict) of a plan query for shapes alone: the pointers the planner only tests for null are placeholders"""
    on = lambda f: 16 if f else None  # noqa: E731
    ia = _lib.Act(int(act), 1, on(act_params), on(act_params), 0.0)
    e = dict(residual=False, out_scale=1.0, accumulate=False, tanh=False, post_act=0, want_raw=False, post_params=True)
    e.update(epilogue)
    pa = _lib.Act(int(e["post_act"]), 1, on(e["post_params"]), on(e["post_params"]), 0.0)
    ep = _lib.ConvEpilogue(on(e["residual"]), float(e["out_scale"]), int(e["accumulate"]), int(e["tanh"]), pa, on(e["want_raw"]))
    out = (ctypes.c_int32 * 6)()
    rc = fn(int(x_f32), int(y_f32), *args, ctypes.addressof(ia), ctypes.addressof(ep), _prefer() if prefer is None else prefer, out)
    return rc, dict(zip(("family", "word", "Lp", "lead", "phases", "ws_floats"), out)) if rc == 0 else None


def conv_plan(B, Cin, Lin, Cout, Lout, K, *, stride=1, padding=0, dilation=1, act=0, act_params=True, x_f32=True, y_f32=True,
              prefer=None, **epilogue):
    """what conv1d would launch for these shapes (kalle_conv_plan: no device, nothing launched): (return code, None or dict of
    family, word, Lp, lead, phases, ws_floats).  Cin: the conv's (half of x's channels under act 4); prefer: None = from
    KALLE_CONV_CFIRST, 0 auto, 1 always / 2 never the channels-per-lane kernels; epilogue: which of residual, accumulate, tanh,
    want_raw are set, out_scale, post_act code; act_params / post_params: SnakeBeta's alpha and beta are given"""
    return _plan(_lib.load().kalle_conv_plan, (B, Cin, Lin, Cout, Lout, K, stride, padding, dilation), act, act_params, epilogue, prefer,
                 x_f32, y_f32)


def conv_transpose_plan(B, Cin, Lin, Cout, Lout, K, *, stride, padding, act=0, act_params=True, x_f32=True, y_f32=True, prefer=None,
                        **epilogue):
    """the same for conv_transpose1d (kalle_conv_transpose_plan)"""
    return _plan(_lib.load().kalle_conv_transpose_plan, (B, Cin, Lin, Cout, Lout, K, stride, padding), act, act_params, epilogue, prefer,
                 x_f32, y_f32)


def conv_len(L, K, stride=1, padding=0, pad_right=None, dilation=1):
    """outputs a conv makes of L inputs (torch's formula; left pad `padding`, right pad `pad_right`, default the same)"""
    pr = padding if pad_right is None else pad_right
    return (L + padding + pr - dilation * (K - 1) - 1) // stride + 1


def conv_transpose_len(L, K, stride, padding, trim=0):
    """outputs a transposed conv makes of L inputs, less `trim`"""
    return (L - 1) * stride - 2 * padding + K - trim


class RaggedLengths:
    """The per-row lengths of a ragged batch at every resolution a conv stack takes it through: `levels[i]` is a tuple of B
    ints, level 0 the stack's input.  All levels sit in ONE host int32 array and ONE device int32 tensor [levels][B],
    uploaded here, once per encode / decode call; a layer gets its two rows of it as a `Lens`.  The stack plans the
    levels before it runs (each from the layer's own output-length formula, row by row); a layer recomputes its own from its
    input level and must find it (`Lens.to`), so a stack that plans one thing and runs another fails loudly."""

    def __init__(self, levels, device):
        self.levels = [tuple(int(v) for v in lv) for lv in levels]
        self.B = len(self.levels[0])
        if any(len(lv) != self.B for lv in self.levels) or any(v < 0 for lv in self.levels for v in lv):
            raise ValueError("RaggedLengths: every level holds one non-negative length per row")
        flat = [v for lv in self.levels for v in lv]
        self._host = (ctypes.c_int32 * len(flat))(*flat)
        self._dev = torch.tensor(flat, dtype=torch.int32).to(device)         # the one upload

    def at(self, i=0):
        return Lens(self, i)


class Lens:
    """the row lengths of one level of a RaggedLengths: `host` (tuple), and the host / device addresses the C ABI takes"""
    __slots__ = ("owner", "i")

    def __init__(self, owner, i):
        self.owner, self.i = owner, i

    @property
    def host(self):
        return self.owner.levels[self.i]

    def host_ptr(self):
        return ctypes.c_void_p(ctypes.addressof(self.owner._host) + 4 * self.owner.B * self.i)

    def dev_ptr(self):
        return ctypes.c_void_p(self.owner._dev.data_ptr() + 4 * self.owner.B * self.i)

    def to(self, lengths):
        """the level that holds `lengths`: this one or the nearest later one"""
        lengths = tuple(lengths)
        for j in range(self.i, len(self.owner.levels)):
            if self.owner.levels[j] == lengths:
                return Lens(self.owner, j)
        raise ValueError(f"lengths {lengths} are not a planned level of this ragged batch (from level {self.i}: "
                         f"{self.owner.levels[self.i:]})")

    def map(self, fn):
        """fn applied to every live row (an inactive row, length 0, stays inactive; a result below 0 counts as 0)"""
        return self.to(max(0, fn(v)) if v > 0 else 0 for v in self.host)


def plan_levels(lengths, maps):
    """levels for RaggedLengths: `lengths`, then one level per length map of the stack, applied row by row as Lens.map does"""
    levels = [tuple(int(v) for v in lengths)]
    for fn in maps:
        levels.append(tuple(max(0, fn(v)) if v > 0 else 0 for v in levels[-1]))
    return levels


def _check_lens(lens, x, B, L, *others):
    if not isinstance(lens, Lens):
        raise TypeError("lens: a conv_ops.Lens (RaggedLengths(...).at(level))")
    if lens.owner.B != B or lens.owner._dev.device != x.device:
        raise ValueError(f"lens holds {lens.owner.B} rows on {lens.owner._dev.device}, x {B} on {x.device}")
    if max(lens.host) > L:
        raise ValueError(f"a length of {lens.host} exceeds the tensor's {L}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x,) + others):
        raise NotImplementedError("ragged lengths are inference only: no backward kernel takes them")


def conv1d(x, w_packed, bias, *, Cout, K, stride=1, padding=0, dilation=1, act=0, alpha=None, beta=None,
           logscale=True, residual=None, post=0, out_dtype=None, pad_right=None, act_param=0.0, out_scale=1.0,
           accumulate_into=None, post_act=None, want_raw=False, lens=None, zero_tail=False):
    """padding = left pad; pad_right defaults to the same (symmetric). act: 0 none, 1 snake(-beta), 2 ELU, 3 LeakyReLU,
    4 WaveNet gate.  Store: (conv + bias + residual) * out_scale (+= accumulate_into) -> post_act -> tanh (post=1).
    lens: a Lens over x's rows - row b is a tensor of lens.host[b] positions (include/kalle_hip.h, ragged batches); the output's
    lengths are this layer's own formula per row.  Outputs past a row's length are not written: zero_tail starts y from zeros
    (the last layer of a stack), otherwise they hold whatever the allocator left and the next layer's lens masks them."""
    lib = _lib.load()
    x = x.contiguous()
    B, Cin, Lin = x.shape
    if act == 4:
        Cin //= 2
    Lout = conv_len(Lin, K, stride, padding, pad_right, dilation)
    lens_out = None
    if lens is not None:
        _check_lens(lens, x, B, Lin, residual, accumulate_into)
        lens_out = lens.map(lambda v: conv_len(v, K, stride, padding, pad_right, dilation))
    if accumulate_into is not None:
        y = accumulate_into
        assert y.is_contiguous() and tuple(y.shape) == (B, Cout, Lout)
    else:
        y = (torch.zeros if lens is not None and zero_tail else torch.empty)((B, Cout, Lout), device=x.device, dtype=out_dtype or x.dtype)
    if residual is not None:
        residual = residual.contiguous()
        assert residual.dtype == x.dtype and residual.shape == y.shape
    ia = _act_struct(act, alpha, beta, logscale, act_param)
    y_raw = torch.empty_like(y) if want_raw else None      # dual output: (post_act(y), y)
    ep = _epilogue(residual, out_scale, accumulate_into is not None, post & 1, post_act, y_raw)
    # the library picks the kernel family (kalle_conv_plan); families 5 / 6 run over a padded, pre-activated copy of x
    family, _, Lp, lead, phases, nws = _query(lib.kalle_conv_plan, "kalle_conv_plan", ia, ep, _dt(x), _dt(y), B, Cin, Lin, Cout, Lout, K,
                                              stride, padding, dilation)
    if lens is not None:      # the same plan, the ..._lens entry points
        li = (lens.host_ptr(), lens.dev_ptr())
        lo = (lens_out.host_ptr(), lens_out.dev_ptr())
        if family >= 5:
            xp = torch.empty((B, Cin, Lp), device=x.device, dtype=torch.float32)
            check(lib.kalle_conv_pad_act_lens(_p(x), _p(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, *li, _stream()),
                  "kalle_conv_pad_act_lens")
            ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws > 0 else None
            check(lib.kalle_conv1d_cfirst_fwd_lens(_p(xp), _p(w_packed), _p(bias), _p(y), B, Cin, Lp, Cout, Lout, K, stride, padding,
                                                   dilation, ctypes.addressof(ep), _p(ws), *li, *lo, _stream()),
                  "kalle_conv1d_cfirst_fwd_lens")
        else:
            check(lib.kalle_conv1d_fwd_lens(_p(x), _dt(x), _p(w_packed), _p(bias), _p(y), _dt(y), B, Cin, Lin, Cout, Lout, K, stride,
                                            padding, dilation, ctypes.addressof(ia), ctypes.addressof(ep), *li, *lo, _stream()),
                  "kalle_conv1d_fwd_lens")
        return (y, y_raw) if want_raw else y
    if family >= 5:
        xp = torch.empty((B, Cin, Lp), device=x.device, dtype=torch.float32)
        check(lib.kalle_conv_pad_act(_p(x), _p(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, _stream()),
              "kalle_conv_pad_act")
        ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws > 0 else None    # input channels split over workgroups too
        check(lib.kalle_conv1d_cfirst_fwd(_p(xp), _p(w_packed), _p(bias), _p(y), B, Cin, Lp, Cout, Lout, K, stride, padding,
                                          dilation, ctypes.addressof(ep), _p(ws), _stream()), "kalle_conv1d_cfirst_fwd")
        return (y, y_raw) if want_raw else y
    check(lib.kalle_conv1d_fwd(_p(x), _dt(x), _p(w_packed), _p(bias), _p(y), _dt(y), B, Cin, Lin, Cout, Lout, K, stride,
                               padding, dilation, ctypes.addressof(ia), ctypes.addressof(ep), _stream()),
          "kalle_conv1d_fwd")
    return (y, y_raw) if want_raw else y


def conv_transpose1d(x, w_packed, bias, *, Cout, K, stride, padding, act=0, alpha=None, beta=None, logscale=True,
                     out_dtype=None, trim=0, act_param=0.0, post_act=None, want_raw=False, lens=None, zero_tail=False):
    """trim: drop the last `trim` outputs (causal transposed conv); negative: keep up to `padding` outputs beyond the symmetric
    right trim (data gradient of a strided conv).  lens / zero_tail: as in conv1d"""
    lib = _lib.load()
    x = x.contiguous()
    B, Cin, Lin = x.shape
    Lout = conv_transpose_len(Lin, K, stride, padding, trim)
    lens_out = None
    if lens is not None:
        _check_lens(lens, x, B, Lin)
        lens_out = lens.map(lambda v: conv_transpose_len(v, K, stride, padding, trim))
    y = (torch.zeros if lens is not None and zero_tail else torch.empty)((B, Cout, Lout), device=x.device, dtype=out_dtype or x.dtype)
    ia = _act_struct(act, alpha, beta, logscale, act_param)
    y_raw = torch.empty_like(y) if want_raw else None
    ep = _epilogue(None, 1.0, False, False, post_act, y_raw)
    family, _, Lp, lead, phases, _ = _query(lib.kalle_conv_transpose_plan, "kalle_conv_transpose_plan", ia, ep, _dt(x), _dt(y), B, Cin,
                                            Lin, Cout, Lout, K, stride, padding)
    if lens is not None:
        li = (lens.host_ptr(), lens.dev_ptr())
        lo = (lens_out.host_ptr(), lens_out.dev_ptr())
        if family == 7:
            xp = torch.empty((B, Cin, Lp), device=x.device, dtype=torch.float32)
            check(lib.kalle_conv_pad_act_lens(_p(x), _p(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, *li, _stream()),
                  "kalle_conv_pad_act_lens")
            check(lib.kalle_conv_transpose1d_cfirst_fwd_lens(_p(xp), _p(w_packed), _p(bias), _p(y), B, Cin, Lp, Cout, Lout, K, stride,
                                                             padding, ctypes.addressof(ep), *lo, _stream()),
                  "kalle_conv_transpose1d_cfirst_fwd_lens")
        else:
            check(lib.kalle_conv_transpose1d_fwd_lens(_p(x), _dt(x), _p(w_packed), _p(bias), _p(y), _dt(y), B, Cin, Lin, Cout, Lout, K,
                                                      stride, padding, ctypes.addressof(ia), ctypes.addressof(ep), *li, *lo, _stream()),
                  "kalle_conv_transpose1d_fwd_lens")
        return (y, y_raw) if want_raw else y
    if family == 7:
        xp = torch.empty((B, Cin, Lp), device=x.device, dtype=torch.float32)
        check(lib.kalle_conv_pad_act(_p(x), _p(xp), B, Cin, Lin, Lp, lead, ctypes.addressof(ia), phases, _stream()),
              "kalle_conv_pad_act")
        check(lib.kalle_conv_transpose1d_cfirst_fwd(_p(xp), _p(w_packed), _p(bias), _p(y), B, Cin, Lp, Cout, Lout, K, stride,
                                                    padding, ctypes.addressof(ep), _stream()),
              "kalle_conv_transpose1d_cfirst_fwd")
        return (y, y_raw) if want_raw else y
    check(lib.kalle_conv_transpose1d_fwd(_p(x), _dt(x), _p(w_packed), _p(bias), _p(y), _dt(y), B, Cin, Lin, Cout,
                                         Lout, K, stride, padding, ctypes.addressof(ia), ctypes.addressof(ep),
                                         _stream()), "kalle_conv_transpose1d_fwd")
    return (y, y_raw) if want_raw else y


def snake_beta(x, alpha, beta, logscale=True):
    lib = _lib.load()
    x = x.contiguous()
    B, C, L = x.shape
    y = torch.empty_like(x)
    check(lib.kalle_snake_beta_fwd(_p(x), _p(y), _dt(x), _p(alpha), _p(beta), int(logscale), B, C, L, _stream()),
          "kalle_snake_beta_fwd")
    return y


def activate(x, act, alpha=None, beta=None, logscale=True):
    """act(x) as a tensor of its own (the VAE's conv kernels apply their input activation on the fly; the weight gradient of a
    transposed conv wants the activated input as its scalar operand): codes 0 none / 1 SnakeBeta / 2 ELU, x fp32 [B, C, L]"""
    if not act:
        return x
    if act == 1:
        return snake_beta(x.contiguous(), alpha, beta, logscale)
    lib = _lib.load()
    x = x.contiguous()
    B, C, L = x.shape
    y = torch.empty_like(x)
    ia = _act_struct(act, alpha, beta, logscale, 0.0)
    check(lib.kalle_conv_pad_act(_p(x), _p(y), B, C, L, L, 0, ctypes.addressof(ia), 1, _stream()), "kalle_conv_pad_act")
    return y


def kaiser_sinc_filter12(device, cutoff=0.25, half_width=0.3, kernel_size=12):
    """the 12-tap low-pass of alias-free-torch's UpSample1d / DownSample1d at ratio 2 (cutoff 0.5/2, half-width 0.6/2):
    kaiser window (beta from the attenuation implied by the transition width) x sinc, normalised to unit sum."""
    import math
    half = kernel_size // 2
    delta_f = 4 * half_width
    A = 2.285 * (half - 1) * math.pi * delta_f + 7.95
    if A > 50.0:
        kb = 0.1102 * (A - 8.7)
    elif A >= 21.0:
        kb = 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0)
    else:
        kb = 0.0
    window = torch.kaiser_window(kernel_size, beta=kb, periodic=False, dtype=torch.float64)
    time = torch.arange(-half, half, dtype=torch.float64) + 0.5
    filt = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    filt = filt / filt.sum()
    return filt.to(device=device, dtype=torch.float32).contiguous()


def act1d(x, filt, alpha, beta, logscale):
    """anti-aliased snake(-beta): up 2x FIR -> activation -> down 2x FIR, one fused kernel"""
    lib = _lib.load()
    x = x.contiguous()
    B, C, L = x.shape
    y = torch.empty_like(x)
    check(lib.kalle_act1d_fwd(_p(x), _p(y), _dt(x), _p(filt), _p(alpha), _p(beta), int(logscale), B, C, L, _stream()),
          "kalle_act1d_fwd")
    return y
