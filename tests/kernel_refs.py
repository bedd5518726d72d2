"""fp64 references of the norm / elementwise / Llasa-tail / conformer / VAE-conv / attention entry points of include/kalle_hip.h.

Plain torch functions on float64 tensors (any device), one per operation, written from the header comment of the entry
point and the reference call sites it cites - not from the kernels.  Callers round whatever the kernel reads as bf16 with
`bf16r` first, so the reference sees the operands the kernel sees.  Each backward says whether it is a closed form or
float64 autograd over the forward reference; tests/test_kernel_refs_cpu.py checks every forward against the torch op it
stands for and every closed-form backward against float64 autograd, so a reader without a GPU can trust them."""
import math

import torch


def bf16r(t):
    """the values a kernel sees when it reads `t` as bf16: rounded once (nearest even), promoted to float64"""
    return t.to(torch.bfloat16).double()


def _per_row(mod, rows, rows_per_batch):
    """[B][D] modulation -> [rows][D]: row r uses batch r // rows_per_batch"""
    idx = torch.arange(rows, device=mod.device) // max(int(rows_per_batch), 1)
    return mod[idx]


# ------------------------------------------------------------------------------------------------ LayerNorm / adaLN
def layernorm_fwd(x, gamma, beta=None, scale=None, shift=None, rows_per_batch=1, eps=1e-5):
    """y = ((x - mean) * rstd * gamma + beta) * (1 + scale[b]) + shift[b]; returns (y, mean, rstd), biased variance"""
    rows = x.shape[0]
    mean = x.mean(-1)
    var = (x - mean[:, None]).pow(2).mean(-1)
    rstd = (var + eps).rsqrt()
    y = (x - mean[:, None]) * rstd[:, None] * gamma
    if beta is not None:
        y = y + beta
    if scale is not None:
        y = y * (1 + _per_row(scale, rows, rows_per_batch))
    if shift is not None:
        y = y + _per_row(shift, rows, rows_per_batch)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, scale=None, rows_per_batch=1, dres=None):
    """closed form, with the saved statistics as given: g = dy (1 + scale[b]); xh = (x - mean) rstd; dh = g gamma;
    dx = dres + rstd (dh - mean_D(dh) - xh mean_D(dh xh)); dgamma = sum_rows g xh; dbeta = sum_rows g.
    Returns (dx, dgamma, dbeta)."""
    g = dy if scale is None else dy * (1 + _per_row(scale, x.shape[0], rows_per_batch))
    xh = (x - mean[:, None]) * rstd[:, None]
    dh = g * gamma
    dx = rstd[:, None] * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres
    return dx, (g * xh).sum(0), g.sum(0)


def adaln_mod_bwd(dy, x, gamma, beta, mean, rstd, nbatch, rows_per_batch):
    """closed form: dscale[b, d] = sum_t dy * ln, dshift[b, d] = sum_t dy, ln = (x - mean) rstd gamma + beta"""
    ln = (x - mean[:, None]) * rstd[:, None] * gamma
    if beta is not None:
        ln = ln + beta
    D = x.shape[1]
    return ((dy * ln).view(nbatch, rows_per_batch, D).sum(1), dy.view(nbatch, rows_per_batch, D).sum(1))


# ------------------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_fwd(x, scale, rows_per_batch=0, eps=1e-6):
    """y = x * scale * rsqrt(mean(x^2) + eps); scale [D] (rows_per_batch 0) or [B][D]; returns (y, rrms)"""
    rrms = (x.pow(2).mean(-1) + eps).rsqrt()
    s = scale if scale.dim() == 1 else _per_row(scale, x.shape[0], rows_per_batch)
    return x * s * rrms[:, None], rrms


def rmsnorm_bwd(dy, x, scale, rrms, rows_per_batch=0, dres=None):
    """closed form with the saved rrms: dh = dy scale; dx = dres + dh rrms - x rrms^3 mean_D(dh x);
    dscale[d] = sum_rows dy x rrms (the shared-scale gradient).  Returns (dx, dscale)."""
    s = scale if scale.dim() == 1 else _per_row(scale, x.shape[0], rows_per_batch)
    dh = dy * s
    dx = dh * rrms[:, None] - x * (rrms.pow(3) * (dh * x).mean(-1))[:, None]
    if dres is not None:
        dx = dx + dres
    return dx, (dy * x * rrms[:, None]).sum(0)


# ------------------------------------------------------------------------------------------------ head norm
def head_norm_fwd(x, mode, gamma=None, beta=None):
    """x [rows][heads][dh].  mode 1: x / max(||x||_2, 1e-12); mode 2: LayerNorm(dh, eps 1e-6) with gamma / beta"""
    if mode == 1:
        return x / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + 1e-6).rsqrt()
    y = (x - mean) * rstd * gamma
    return y if beta is None else y + beta


def head_norm_bwd(x, g, mode, gamma=None):
    """closed form.  mode 1: n = ||x||; n > 1e-12: (g - y <y, g>) / n; else the clamp is active and the map is the linear
    x * 1e12: g * 1e12.  mode 2: LayerNorm backward (dx, dgamma, dbeta) summed over rows and heads.  Returns (dx, dgamma,
    dbeta) (the last two None in mode 1)."""
    if mode == 1:
        n = x.pow(2).sum(-1, keepdim=True).sqrt()
        y = x / n.clamp_min(1e-12)
        dx = torch.where(n > 1e-12, (g - y * (y * g).sum(-1, keepdim=True)) / n.clamp_min(1e-12), g * 1e12)
        return dx, None, None
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + 1e-6).rsqrt()
    xh = (x - mean) * rstd
    dh = g * gamma
    dx = rstd * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))
    return dx, (g * xh).sum((0, 1)), g.sum((0, 1))


def colsum(x):
    return x.sum(0)


# ------------------------------------------------------------------------------------------------ activations
def sigmoid(v):
    """1 / (1 + e^-v) without overflow"""
    e = torch.exp(-v.abs())
    return torch.where(v >= 0, 1 / (1 + e), e / (1 + e))


def silu_fwd(x):
    return x * sigmoid(x)


def silu_bwd(dy, x):
    """closed form: dy * s (1 + x (1 - s)), 1 - s = sigmoid(-x)"""
    return dy * sigmoid(x) * (1 + x * sigmoid(-x))


def swiglu_fwd(h):
    """h [rows][2 inner]: out[m, j] = h[m, j] * silu(h[m, inner + j])"""
    inner = h.shape[1] // 2
    return h[:, :inner] * silu_fwd(h[:, inner:])


def swiglu_bwd(dout, h):
    """closed form: dh[:, :inner] = dout silu(g); dh[:, inner:] = dout x silu'(g)"""
    inner = h.shape[1] // 2
    x, g = h[:, :inner], h[:, inner:]
    return torch.cat([dout * silu_fwd(g), dout * x * silu_bwd(torch.ones_like(g), g)], 1)


def gelu_fwd(x):
    """0.5 x (1 + erf(x / sqrt 2)), the cancelling side through erfc"""
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_bwd(dy, x):
    """closed form: dy (Phi(x) + x phi(x))"""
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + x * pdf)


# ------------------------------------------------------------------------------------------------ diffusion / loss
def diffuse_fwd(x, noise, t, objective):
    """x, noise [B][per]; t [B].  0 ("v"): a = cos(pi t / 2), s = sin(pi t / 2), target = a n - s x; 1: a = 1 - t, s = t,
    target = n - x.  Returns (x_t, target)."""
    if objective == 0:
        a, s = torch.cos(t * (math.pi / 2)), torch.sin(t * (math.pi / 2))
        return a[:, None] * x + s[:, None] * noise, a[:, None] * noise - s[:, None] * x
    return (1 - t)[:, None] * x + t[:, None] * noise, noise - x


def mse(out, target, mask, weight=1.0):
    """out, target [B][C][T]; mask [B][T] (0 / 1) or None.  Returns (sum of squares, count, loss, dout):
    loss = weight * sum / count; dout = 2 weight (out - target) mask / count; count = masked ELEMENTS (mask broadcast over C)"""
    d = out - target
    if mask is not None:
        m = (mask != 0).double()[:, None, :].expand_as(d)
        d = d * m
        cnt = m.sum()
    else:
        cnt = torch.tensor(float(d.numel()), dtype=torch.float64, device=d.device)
    ssq = d.pow(2).sum()
    return ssq, cnt, weight * ssq / cnt, 2 * weight * d / cnt


# ------------------------------------------------------------------------------------------------ data movement
def transpose_2d(x):
    """[B][R][Cn] -> [B][Cn][R]"""
    return x.transpose(1, 2)


def fourier_features(t, w):
    """out[b, j] = cos(2 pi t[b] w[j]), out[b, half + j] = sin(...)"""
    f = 2 * math.pi * t[:, None] * w[None, :]
    return torch.cat([f.cos(), f.sin()], 1)


def fourier_features_bwd(dout, t, w):
    """closed form: dw[j] = sum_b 2 pi t[b] (dout[b, half + j] cos f - dout[b, j] sin f)"""
    half = w.numel()
    f = 2 * math.pi * t[:, None] * w[None, :]
    return (2 * math.pi * t[:, None] * (dout[:, half:] * f.cos() - dout[:, :half] * f.sin())).sum(0)


# ------------------------------------------------------------------------------------------------ optimizer
def adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale, decay_after=False):
    """one torch.optim.Adam (coupled L2: g += wd p) / AdamW (decoupled: p *= 1 - lr wd first) step.  Hyper-parameters are
    taken as given (pass float32-rounded values to see what a float ABI sees).  Returns (p, m, v).
    decay_after: the WRONG order for AdamW (decay applied to the updated parameter) - for the tests that must fail."""
    g = g * grad_scale
    if decoupled and not decay_after:
        p = p * (1 - lr * weight_decay)
    if not decoupled:
        g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = math.sqrt(1 - beta2 ** step)
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2 + eps))
    if decoupled and decay_after:
        p = p * (1 - lr * weight_decay)
    return p, m, v


# ------------------------------------------------------------------------------------------------ Llasa head / tail
def embed_mix_fwd(ids, table, audio, ids_mask, audio_mask):
    """out[r] = audio[r] audio_mask[r] + table[ids[r]] ids_mask[r]; a row whose mask is 0 contributes exactly 0 whatever its
    id / audio holds (padding ids lie outside the table, padded audio rows may hold anything)"""
    rows, D = audio.shape
    out = torch.zeros((rows, D), dtype=torch.float64, device=audio.device)
    ia, ii = audio_mask != 0, ids_mask != 0
    out[ia] = audio[ia] * audio_mask[ia, None]
    out[ii] = out[ii] + table[ids[ii]] * ids_mask[ii, None]
    return out


def embed_mix_bwd(dout, ids, ids_mask, audio_mask, vocab):
    """closed form: daudio = dout audio_mask; dtable[v] = sum_{r: ids[r] = v, ids_mask[r] != 0} dout[r] ids_mask[r].
    Returns (dtable [vocab][D], daudio)."""
    dtable = torch.zeros((vocab, dout.shape[1]), dtype=torch.float64, device=dout.device)
    ii = ids_mask != 0
    dtable.index_add_(0, ids[ii], dout[ii] * ids_mask[ii, None])
    return dtable, dout * audio_mask[:, None]


def gauss_kl_fwd(pred, label, mask_a, mask_b, std):
    """kl[r] = sum_c (pred - label)^2 / (2 std^2) / dim; returns sums4 = (sum kl ma, sum ma, sum kl mb, sum mb)"""
    kl = (pred - label).pow(2).sum(-1) / (2 * std * std) / pred.shape[1]
    return torch.stack([(kl * mask_a).sum(), mask_a.sum(), (kl * mask_b).sum(), mask_b.sum()])


def gauss_kl_bwd(pred, label, mask_a, mask_b, sums4, grad_a, grad_b, std):
    """closed form of d(grad_a s0 / s1 + grad_b s2 / s3) / dpred with the sums as given"""
    w = grad_a * mask_a / sums4[1] + grad_b * mask_b / sums4[3]
    return (pred - label) / (std * std * pred.shape[1]) * w[:, None]


# ------------------------------------------------------------------------------------------------ conformer
def add_rows(x, table):
    """x [B][n] + table [n]"""
    return x + table[None, :]


def dwconv1d_fwd(x, w, pad, flip=False, tap_shift=None):
    """x [B][N][D], w [D][K]: y[b][n][c] = sum_k w[c][flip ? K-1-k : k] x[b][n + k - pad][c], x = 0 outside 0 <= . < N.
    tap_shift (k, s): the WRONG filter whose tap k reads position n + k - pad + s - for the tests that must fail."""
    B, N, D = x.shape
    K = w.shape[1]
    y = torch.zeros((B, N, D), dtype=torch.float64, device=x.device)
    for k in range(K):
        wk = w[:, K - 1 - k] if flip else w[:, k]
        o = k - pad + (tap_shift[1] if tap_shift is not None and tap_shift[0] == k else 0)
        lo, hi = max(0, -o), min(N, N - o)               # output rows n with 0 <= n + o < N
        if hi > lo:
            y[:, lo:hi] += wk * x[:, lo + o:hi + o]
    return y


def dwconv1d_wgrad(dy, x, K, pad):
    """closed form: dw[c][k] = sum_{b, n} dy[b][n][c] x[b][n + k - pad][c]"""
    B, N, D = x.shape
    dw = torch.zeros((D, K), dtype=torch.float64, device=x.device)
    for k in range(K):
        o = k - pad
        lo, hi = max(0, -o), min(N, N - o)
        if hi > lo:
            dw[:, k] = (dy[:, lo:hi] * x[:, lo + o:hi + o]).sum((0, 1))
    return dw


# ------------------------------------------------------------------------------------------------ more of the Llasa tail / DiT path
def axpby(x, y, a, b):
    return a * x + b * y


def grad_cast(g, x_out, x_in, gate, row_mask, nbatch, rows_per_batch):
    """g, x_out, x_in [B T][D]; gate [B][D] or None; row_mask [B T] (0 / 1) or None.
    gb = g * sigmoid(1 - gate[b]) * row_mask (before the rounding to bf16);
    dgate[b] = -(1 - sigmoid(1 - gate[b])) * sum_t g row_mask (x_out - x_in), 1 - sigmoid(v) = sigmoid(-v).
    closed form (checked against autograd of x_out = x_in + branch * sigmoid(1 - gate)).  Returns (gb, dgate or None)."""
    D = g.shape[1]
    gm = g if row_mask is None else g * (row_mask != 0).double()[:, None]
    if gate is None:
        return gm, None
    s = sigmoid(1 - gate)
    idx = torch.arange(g.shape[0], device=g.device) // rows_per_batch
    dgate = -sigmoid(gate - 1) * (gm * (x_out - x_in)).view(nbatch, rows_per_batch, D).sum(1)
    return gm * s[idx], dgate


def softplus(v):
    """log(1 + e^v), v itself above the threshold 20 (F.softplus)"""
    return torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp_max(20))))


def _kl2_label(label_mean, label_std, label_mode, std_mult, dim):
    if label_mode == 0:
        return label_mean, label_std * std_mult
    return label_mean[:, :dim], (softplus(label_mean[:, dim:]) + 1e-4) * std_mult


def gauss_kl2_fwd(pred, label_mean, label_std, label_mode, std_mult, mask_a, mask_b):
    """kl[r] = sum_c KL(N(m1, s1) || N(m2, exp(l2))) / dim = sum_c (l2 - log s1 + (s1^2 + (m1 - m2)^2) / (2 exp(2 l2)) - 1/2) / dim,
    m2 | l2 = the halves of pred [rows][2 dim]; sums4 as gauss_kl_fwd"""
    dim = pred.shape[1] // 2
    m1, s1 = _kl2_label(label_mean, label_std, label_mode, std_mult, dim)
    m2, l2 = pred[:, :dim], pred[:, dim:]
    kl = (l2 - s1.log() + 0.5 * (s1 * s1 + (m1 - m2).pow(2)) * torch.exp(-2 * l2) - 0.5).sum(-1) / dim
    return torch.stack([(kl * mask_a).sum(), mask_a.sum(), (kl * mask_b).sum(), mask_b.sum()])


def gauss_kl2_bwd(pred, label_mean, label_std, label_mode, std_mult, mask_a, mask_b, sums4, grad_a, grad_b):
    """closed form: d / d m2 = w (m2 - m1) e, d / d l2 = w (1 - (s1^2 + (m1 - m2)^2) e), e = exp(-2 l2),
    w = (grad_a mask_a / sums4[1] + grad_b mask_b / sums4[3]) / dim"""
    dim = pred.shape[1] // 2
    m1, s1 = _kl2_label(label_mean, label_std, label_mode, std_mult, dim)
    m2, l2 = pred[:, :dim], pred[:, dim:]
    w = ((grad_a * mask_a / sums4[1] + grad_b * mask_b / sums4[3]) / dim)[:, None]
    e = torch.exp(-2 * l2)
    return torch.cat([w * (m2 - m1) * e, w * (1 - (s1 * s1 + (m1 - m2).pow(2)) * e)], 1)


def peak_normalize(x):
    """clamp(x / max|x|, -1, 1) * 32767 BEFORE the truncation to int16; returns (that, max|x|)"""
    peak = x.abs().max()
    return (x / peak).clamp(-1, 1) * 32767, peak


# ------------------------------------------------------------------------------------------------ VAE conv stack
# Written from the header text of the conv section of include/kalle_hip.h as explicit sums over taps on shifted slices (one
# einsum per tap), never by calling F.conv1d: tests/test_conv_refs_cpu.py checks them against torch.nn.functional, torch's
# weight_norm parametrisation and float64 autograd.  Activations are (B, C, L); `w` is the packed [Cin][K][CoutP] weight.
def weight_norm_fold(v, g, transposed):
    """flags bit 0: v is [Cin][Cout][K] (ConvTranspose1d) instead of [Cout][Cin][K]; bit 1: tap k is stored at K-1-k.
    w[ci][k][co] = g[o] v[o][.][k] / ||v[o]||, o = the index of dim 0 (g None: repack only); CoutP = Cout rounded up to 8,
    pad columns 0"""
    d0, d1, K = v.shape
    w = v if g is None else v * (g / v.reshape(d0, -1).pow(2).sum(1).sqrt())[:, None, None]
    if transposed & 2:
        w = w.flip(2)
    w = w.permute(0, 2, 1) if transposed & 1 else w.permute(1, 2, 0)          # -> [Cin][K][Cout]
    cout = w.shape[2]
    out = torch.zeros((w.shape[0], K, (cout + 7) // 8 * 8), dtype=torch.float64, device=v.device)
    out[:, :, :cout] = w
    return out


def _act_ab(alpha, beta, logscale):
    a, b = alpha.double(), beta.double()
    return (a.exp(), b.exp()) if logscale else (a, b)


def act(x, code, alpha=None, beta=None, logscale=0, param=0.0):
    """kalle_act on (B, C, L): 0 none, 1 x + sin^2(a x) / (b + 1e-9) per channel (a, b = exp(alpha), exp(beta) when logscale),
    2 ELU, 3 LeakyReLU(param), 4 WaveNet gate tanh(x[:, :C/2]) * sigmoid(x[:, C/2:])"""
    if code == 0:
        return x
    if code == 1:
        a, b = _act_ab(alpha, beta, logscale)
        return x + torch.sin(x * a[None, :, None]).pow(2) / (b[None, :, None] + 1e-9)
    if code == 2:
        return torch.where(x > 0, x, torch.expm1(x.clamp_max(0)))
    if code == 3:
        return torch.where(x > 0, x, x * param)
    if code == 4:
        h = x.shape[1] // 2
        return torch.tanh(x[:, :h]) * sigmoid(x[:, h:])
    raise ValueError(code)


def snake_beta(x, alpha, beta, logscale):
    """kalle_snake_beta_fwd"""
    return act(x, 1, alpha, beta, logscale)


def _epilogue(conv, asum, w_cout, bias, ep):
    """(conv + bias + residual) * out_scale; += y (accumulate); y_raw = that; post_act; tanh.  ep: dict with the optional keys
    residual, out_scale, accumulate (the previous contents of y), post (code, alpha, beta, logscale, param), tanh.
    Returns (y, y_raw, abs_sum = the sum of the magnitudes of all terms that were added)"""
    ep = ep or {}
    v, a = conv, asum
    if bias is not None:
        v, a = v + bias[None, :, None], a + bias.abs()[None, :, None]
    if ep.get("residual") is not None:
        v, a = v + ep["residual"], a + ep["residual"].abs()
    s = ep.get("out_scale", 1.0)
    v, a = v * s, a * abs(s)
    if ep.get("accumulate") is not None:
        v, a = v + ep["accumulate"], a + ep["accumulate"].abs()
    raw = v
    if ep.get("post"):
        v = act(v, *ep["post"])
    if ep.get("tanh"):
        v = torch.tanh(v)
    return v, raw, a


def conv1d(x, w, Cout, bias=None, stride=1, padding=0, dilation=1, Lout=None, in_act=None, epilogue=None, tap_shift=None):
    """y[b][co][l] = sum_{ci, k} w[ci][k][co] act(x)[b][ci][l stride - padding + k dilation] (0 outside 0 <= . < Lin): `padding`
    is the LEFT pad, the right pad is whatever Lout implies.  in_act: (code, alpha, beta, logscale, param).
    tap_shift (k, s, lmax): the WRONG conv whose tap k reads one position + s for outputs l < lmax (tests that must fail).
    Returns (y, y_raw, abs_sum)"""
    xa = act(x, *in_act) if in_act else x
    B, Cin, Lin = xa.shape
    K = w.shape[1]
    conv = torch.zeros((B, Cout, Lout), dtype=torch.float64, device=x.device)
    asum = torch.zeros_like(conv)
    for k in range(K):
        segs = [(0, Lout, 0)]
        if tap_shift is not None and tap_shift[0] == k:
            segs = [(0, min(tap_shift[2], Lout), tap_shift[1]), (min(tap_shift[2], Lout), Lout, 0)]
        for s0, s1, sh in segs:
            # outputs l in [s0, s1) whose input position i = l stride + o lies in [0, Lin)
            o = k * dilation - padding + sh
            lo = max(s0, -(o // stride) if o < 0 else 0)
            hi = min(s1, (Lin - 1 - o) // stride + 1 if Lin - 1 - o >= 0 else 0)
            if hi <= lo:
                continue
            xs = xa[:, :, lo * stride + o:(hi - 1) * stride + o + 1:stride]
            conv[:, :, lo:hi] += torch.einsum("bil,io->bol", xs, w[:, k, :Cout])
            asum[:, :, lo:hi] += torch.einsum("bil,io->bol", xs.abs(), w[:, k, :Cout].abs())
    return _epilogue(conv, asum, Cout, bias, epilogue)


def conv_transpose1d(x, w, Cout, bias=None, stride=1, padding=0, Lout=None, in_act=None, epilogue=None, drop_last_tap_from=None):
    """y[b][co][lo] = sum_{ci, k, li : li stride - padding + k = lo} w[ci][k][co] act(x)[b][ci][li], for any
    0 < Lout <= (Lin - 1) stride - padding + K (the full length minus the LEFT trim only).
    drop_last_tap_from: the WRONG conv without tap K-1 for outputs lo >= that (tests that must fail).
    Returns (y, y_raw, abs_sum)"""
    xa = act(x, *in_act) if in_act else x
    B, Cin, Lin = xa.shape
    K = w.shape[1]
    full = (Lin - 1) * stride + K
    conv = torch.zeros((B, Cout, full), dtype=torch.float64, device=x.device)
    asum = torch.zeros_like(conv)
    for k in range(K):
        t = torch.einsum("bil,io->bol", xa, w[:, k, :Cout])
        ta = torch.einsum("bil,io->bol", xa.abs(), w[:, k, :Cout].abs())
        if drop_last_tap_from is not None and k == K - 1:
            pos = torch.arange(Lin, device=x.device) * stride + k - padding
            t, ta = t * (pos < drop_last_tap_from), ta * (pos < drop_last_tap_from)
        conv[:, :, k:k + (Lin - 1) * stride + 1:stride] += t
        asum[:, :, k:k + (Lin - 1) * stride + 1:stride] += ta
    assert 0 < Lout <= full - padding
    return _epilogue(conv[:, :, padding:padding + Lout], asum[:, :, padding:padding + Lout], Cout, bias, epilogue)


def conv_pad_act(x, Lp, padding, act_args=None, phases=1):
    """x_padded [B][C][Lp]: padded index j holds act(x)[j - padding] (0 outside 0 <= . < Lin); with phases > 1 padded index j
    is stored at slot (j % phases) * (Lp / phases) + j / phases (phase rows)"""
    xa = act(x, *act_args) if act_args else x
    B, C, Lin = xa.shape
    xp = torch.zeros((B, C, Lp), dtype=torch.float64, device=x.device)
    n = min(Lin, Lp - padding)
    if n > 0:
        xp[:, :, padding:padding + n] = xa[:, :, :n]
    if phases > 1:
        xp = xp.view(B, C, Lp // phases, phases).transpose(2, 3).reshape(B, C, Lp)
    return xp


def conv_wgrad(U, V, K, stride, padding, dilation, act_on=0, act_args=None):
    """dW[cu][cv][k] = sum_{b, m} U[b][cu][m] V[b][cv][m stride - padding + k dilation] (0 outside V), the activation applied
    to V (act_on 0) or U (act_on 1) first.  Returns (dW, abs_sum)"""
    if act_args:
        U, V = (U, act(V, *act_args)) if act_on == 0 else (act(U, *act_args), V)
    B, CU, MU = U.shape
    LV = V.shape[2]
    dW = torch.zeros((CU, V.shape[1], K), dtype=torch.float64, device=U.device)
    asum = torch.zeros_like(dW)
    for k in range(K):
        o = k * dilation - padding
        lo = -(o // stride) if o < 0 else 0
        hi = min(MU, (LV - 1 - o) // stride + 1 if LV - 1 - o >= 0 else 0)
        if hi <= lo:
            continue
        vs = V[:, :, lo * stride + o:(hi - 1) * stride + o + 1:stride]
        dW[:, :, k] = torch.einsum("bum,bvm->uv", U[:, :, lo:hi], vs)
        asum[:, :, k] = torch.einsum("bum,bvm->uv", U[:, :, lo:hi].abs(), vs.abs())
    return dW, asum


def act_bwd(x, g, code, alpha=None, beta=None, logscale=0):
    """closed form of dx = g act'(x) for codes 0 / 1 / 2; the snake also returns d alpha, d beta [C] (through the exp when
    logscale): d/da = x sin(2 a x) / (b + 1e-9), d/db = -sin^2(a x) / (b + 1e-9)^2.  Returns (dx, dalpha, dbeta, abs terms of the
    two channel sums)"""
    if code == 0:
        return g, None, None, None
    if code == 2:
        return g * torch.where(x > 0, torch.ones_like(x), torch.exp(x.clamp_max(0))), None, None, None
    a, b = _act_ab(alpha, beta, logscale)
    a3, b3 = a[None, :, None], b[None, :, None] + 1e-9
    s2 = torch.sin(2 * a3 * x)
    dx = g * (1 + a3 * s2 / b3)
    ta = g * x * s2 / b3
    tb = -g * torch.sin(a3 * x).pow(2) / b3.pow(2)
    if logscale:
        ta, tb = ta * a3, tb * b[None, :, None]
    return dx, ta.sum((0, 2)), tb.sum((0, 2)), (ta.abs().sum((0, 2)), tb.abs().sum((0, 2)))


def tanh_bwd(dy, y):
    return dy * (1 - y * y)


def upsample_nearest(x, scale, backward=False):
    """[rows][L] -> [rows][L scale], y[r][l] = x[r][l // scale]; backward: dx[r][m] = sum_{j < scale} dy[r][m scale + j]"""
    if backward:
        return x.view(x.shape[0], -1, scale).sum(-1)
    return x[:, :, None].expand(-1, -1, scale).reshape(x.shape[0], -1)


def channel_sum(x):
    return x.sum((0, 2))


def weight_norm_bwd(dw, v, g):
    """closed form for w = g v / ||v|| per slice of dim 0: dg = <dw, v> / ||v||, dv = g / ||v|| (dw - v <dw, v> / ||v||^2)"""
    d0 = v.shape[0]
    v2, dw2 = v.reshape(d0, -1), dw.reshape(d0, -1)
    nn = v2.pow(2).sum(1)
    dot = (dw2 * v2).sum(1)
    dv = (g / nn.sqrt())[:, None] * (dw2 - v2 * (dot / nn)[:, None])
    return dv.view_as(v), dot / nn.sqrt()


def act1d_up(x, filt):
    """2x up-sampling of Activation1d: replicate pad 5, zero-stuffed 12-tap FIR, gain 2, crop 15 each side -> [B][C][2 L]"""
    B, C, L = x.shape
    xp = torch.cat([x[:, :, :1].expand(-1, -1, 5), x, x[:, :, -1:].expand(-1, -1, 5)], 2)
    full = torch.zeros((B, C, 2 * (L + 10 - 1) + 12), dtype=torch.float64, device=x.device)
    for k in range(12):
        full[:, :, k:k + 2 * (L + 9) + 1:2] += 2 * filt[k] * xp
    up = full[:, :, 15:full.shape[2] - 15]
    assert up.shape[2] == 2 * L
    return up


def act1d_down(h, filt):
    """2x down-sampling of Activation1d: replicate pad (5, 6), 12-tap FIR, stride 2 -> [B][C][L]"""
    B, C, L2 = h.shape
    L = L2 // 2
    hp = torch.cat([h[:, :, :1].expand(-1, -1, 5), h, h[:, :, -1:].expand(-1, -1, 6)], 2)
    y = torch.zeros((B, C, L), dtype=torch.float64, device=h.device)
    for k in range(12):
        y += filt[k] * hp[:, :, k:k + 2 * (L - 1) + 1:2]
    return y


def act1d(x, filt, alpha=None, beta=None, logscale=0):
    """Activation1d: act1d_up -> snake (ELU when alpha is None) -> act1d_down"""
    up = act1d_up(x, filt)
    h = act(up, 2) if alpha is None else act(up, 1, alpha, beta, logscale)
    return act1d_down(h, filt)


# ------------------------------------------------------------------------------------------------ attention
# kalle_attention_fwd / _bwd (_hd).  Operands are the head windows, already float64: q [B][Nq][H dh], k / v [B][Nk][Hkv dh],
# cos / sin [positions][rot / 2], key_mask bool / uint8 [B][Nk] or None.  `round_points`: round to bf16 (nearest even) where the
# kernels are documented to (the rotated q and k; in the backward also the P and dS operands of the gradient products, and
# delta from the bf16 `out` the caller stored).  The forward's probabilities are never rounded here.  `wrong`: a deliberately wrong
# variant, for the tests that show each would be caught.
def _rotate(x, cos, sin, rot, pos, sign=1.0):
    """rotate-half on the first `rot` dims of x [..][n][dh], row r at position pos[r]: x cos + cat(-x2, x1) sin"""
    if not rot:
        return x
    h = rot // 2
    c, s = cos[pos][:, :h], sign * sin[pos][:, :h]
    x1, x2 = x[..., :h], x[..., h:rot]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, x[..., rot:]], -1)


def _unrotate(g, cos, sin, rot, pos):
    """the transpose of _rotate: what the gradient of the rotated tensor becomes for the tensor before rotation"""
    if not rot:
        return g
    h = rot // 2
    c, s = cos[pos][:, :h], sin[pos][:, :h]
    g1, g2 = g[..., :h], g[..., h:rot]
    return torch.cat([g1 * c + g2 * s, g2 * c - g1 * s, g[..., rot:]], -1)


def _unrotate_abs(u, rot):
    """a bound through _unrotate: |cos|, |sin| <= 1, so each rotated dim is bounded by the sum of the two partners' bounds"""
    if not rot:
        return u
    h = rot // 2
    t = u[..., :h] + u[..., h:rot]
    return torch.cat([t, t, u[..., rot:]], -1)


def _attn_core(q, k, v, H, Hkv, dh, rot, cos, sin, key_mask, causal, round_points, mask_fill, wrong):
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    group = H // Hkv
    dev = q.device
    hmap = torch.arange(H, device=dev) // group
    if wrong == "gqa_modulo":
        hmap = torch.arange(H, device=dev) % Hkv
    off = Nk - Nq if causal else 0
    qpos = torch.arange(Nq, device=dev) + off + (1 if wrong == "query_position" else 0)
    kpos = torch.arange(Nk, device=dev)
    sign = -1.0 if wrong == "rotate_half_sign" else 1.0
    qh = _rotate(q.reshape(B, Nq, H, dh).transpose(1, 2), cos, sin, rot, qpos, sign)
    kh = _rotate(k.reshape(B, Nk, Hkv, dh).transpose(1, 2), cos, sin, rot, kpos, sign)
    vh = v.reshape(B, Nk, Hkv, dh).transpose(1, 2)
    if round_points:
        qh, kh = bf16r(qh), bf16r(kh)
    scale = 0.125 if wrong == "scale_eighth" else dh ** -0.5
    s = (qh @ kh[:, hmap].transpose(-1, -2)) * scale
    if key_mask is not None:
        m = key_mask.bool()
        if wrong == "mask_other_batch":
            m = m.flip(0)
        fill = -torch.finfo(torch.float64).max if mask_fill is None else mask_fill
        s = s.masked_fill(~m[:, None, None, :], fill)
    if causal:
        lim = torch.arange(Nq, device=dev)[:, None] + off - (1 if wrong == "causal_boundary" else 0)
        s = s.masked_fill(kpos[None, :] > lim, -math.inf)
    if isinstance(wrong, tuple) and wrong[0] == "drop_key":
        s = s.clone()
        s[..., wrong[1]] = -math.inf
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)          # (not exp(s - lse): the fill of a fully masked row absorbs log n)
    return qh, kh, vh, hmap, scale, s, lse, p


def attention_ref(q, k, v, H, Hkv, dh, rot=0, cos=None, sin=None, key_mask=None, causal=False, round_points=False,
                  mask_fill=None, wrong=None):
    """out [B][Nq][H dh], lse [B][H][Nq], p [B][H][Nq][Nk], rotated q [B][H][Nq][dh], rotated k [B][Hkv][Nk][dh]:
    p = softmax_j(q~_i . k~_j dh^-0.5), head h reads kv head h // (H // Hkv), a query's rotary position is i + (Nk - Nq) when
    causal and i otherwise, masked keys masked_fill(-finfo.max) (or `mask_fill`), causally excluded keys -inf"""
    qh, kh, vh, hmap, scale, s, lse, p = _attn_core(q, k, v, H, Hkv, dh, rot, cos, sin, key_mask, causal, round_points, mask_fill, wrong)
    out = (p @ vh[:, hmap]).transpose(1, 2).reshape(q.shape[0], q.shape[1], H * dh)
    return out, lse, p, qh, kh


def attention_fwd_units(p, qh, kh, v, out, lse, H, Hkv, dh):
    """the magnitudes the forward's errors scale with: out sum_j p_ij |v_jd| + |out_id|; lse 1 + |lse| + sum_d |q~_id| max_j |k~_jd| dh^-0.5"""
    B, Nq = out.shape[0], out.shape[1]
    hmap = torch.arange(H, device=out.device) // (H // Hkv)
    vh = v.reshape(B, -1, Hkv, dh).transpose(1, 2)
    u_out = (p @ vh[:, hmap].abs()).transpose(1, 2).reshape(B, Nq, H * dh) + out.abs()
    kmax = kh.abs().amax(-2)[:, hmap]                                      # [B][H][dh]
    u_lse = 1 + lse.abs() + (qh.abs() * kmax[:, :, None, :]).sum(-1) * dh ** -0.5
    return u_out, u_lse


def attention_bwd_ref(q, k, v, dout, H, Hkv, dh, rot=0, cos=None, sin=None, key_mask=None, causal=False, round_points=False,
                      out=None, masked_rows_zero=False, wrong=None):
    """dq [B][Nq][H dh], dk, dv [B][Nk][Hkv dh], delta [B][H][Nq] and the per-element magnitudes {"dq", "dk", "dv"} their
    errors scale with, as explicit sums (no autograd):
      delta_i = sum_d dout_id out_id  (`out`: the stored output when given, else the exact one)
      dv_jd = sum_{h in group} sum_i p_ij dout_id;  dP_ij = sum_d dout_id v_jd;  dS_ij = p_ij (dP_ij - delta_i) dh^-0.5
      dq~_id = sum_j dS_ij k~_jd;  dk~_jd = sum_{h in group} sum_i dS_ij q~_id;  dq, dk = un-rotated dq~, dk~
    `masked_rows_zero`: a masked key is absent (p = 0) even where every key of its batch row is masked - the header's
    contract for the backward, where the fill of the forward would give uniform weights"""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    group = H // Hkv
    fwd_wrong = wrong if wrong in ("gqa_modulo", "query_position", "rotate_half_sign", "mask_other_batch", "scale_eighth",
                                   "causal_boundary") or isinstance(wrong, tuple) else None
    qh, kh, vh, hmap, scale, s, lse, p = _attn_core(q, k, v, H, Hkv, dh, rot, cos, sin, key_mask, causal, round_points, None, fwd_wrong)
    if masked_rows_zero and key_mask is not None:
        p = p * key_mask.bool()[:, None, None, :]
    doh = dout.reshape(B, Nq, H, dh).transpose(1, 2)
    oh = (p @ vh[:, hmap]) if out is None else out.reshape(B, Nq, H, dh).transpose(1, 2)
    delta = (doh * (doh if wrong == "delta_dout_squared" else oh)).sum(-1)
    dP = doh @ vh[:, hmap].transpose(-1, -2)
    dS = p * (dP - delta[..., None]) * scale
    pv = bf16r(p) if round_points else p
    dSr = bf16r(dS) if round_points else dS
    aS = p * (dP.abs() + (p * dP.abs()).sum(-1, keepdim=True)) * scale       # |dS| bounded term by term
    heads = lambda t: t.reshape(B, Hkv, group, *t.shape[2:])  # noqa: E731
    dvh = heads(pv.transpose(-1, -2) @ doh).sum(2)
    a_dv = heads(p.transpose(-1, -2) @ doh.abs()).sum(2)
    dkh = heads(dSr.transpose(-1, -2) @ qh)
    a_dk = heads(aS.transpose(-1, -2) @ qh.abs()).sum(2)
    dkh = dkh[:, :, 1:].sum(2) if wrong == "dk_missing_head" else dkh.sum(2)
    dqh = dSr @ kh[:, hmap]
    a_dq = aS @ kh[:, hmap].abs()
    off = Nk - Nq if causal else 0
    qpos, kpos = torch.arange(Nq, device=q.device) + off, torch.arange(Nk, device=q.device)
    dq = dqh if wrong == "dq_not_unrotated" else _unrotate(dqh, cos, sin, rot, qpos)
    dk = _unrotate(dkh, cos, sin, rot, kpos)
    flat = lambda t, n, h: t.transpose(1, 2).reshape(B, n, h * dh)  # noqa: E731
    dq, dk, dv = flat(dq, Nq, H), flat(dk, Nk, Hkv), flat(dvh, Nk, Hkv)
    mags = {"dq": flat(_unrotate_abs(a_dq, rot), Nq, H) + dq.abs(), "dk": flat(_unrotate_abs(a_dk, rot), Nk, Hkv) + dk.abs(),
            "dv": flat(a_dv, Nk, Hkv) + dv.abs()}
    return dq, dk, dv, delta, mags


# ------------------------------------------------------------------------------------------------ Llama decode step
# kalle_gemv_bf16 and the stages of kalle_llama_decode_step (include/kalle_hip.h), float64.  A GEMV with a prologue builds its
# bf16 operand on the fly: the references return the prologue value BEFORE that rounding too, so that a test can tell which
# elements sit so close to a bf16 rounding boundary that the kernel's fast-math value may round the other way.
def gemv(W, x, residual=None):
    """y[n] = sum_k W[n][k] x[k] (+ residual[n])"""
    y = W @ x
    return y if residual is None else y + residual


def decode_rms_prologue(x, gamma, eps, wrong=None):
    """x * (gamma * rsqrt(mean(x^2) + eps)), not yet rounded (LlamaRMSNorm)"""
    rr = (x.pow(2).mean() + (0.0 if wrong == "no_eps" else eps)).rsqrt()
    if wrong == "gamma_after_rounding":
        return bf16r(x * rr) * gamma
    return x * (gamma * rr)


def decode_swiglu_prologue(hf, wrong=None):
    """hf = up | gate -> up * silu(gate), not yet rounded (LlamaMLP)"""
    inner = hf.shape[0] // 2
    up, gate = hf[:inner], hf[inner:]
    return gate * silu_fwd(up) if wrong == "gate_silu_up" else up * silu_fwd(gate)


def bf16_ulp(v):
    """spacing of the bf16 numbers around v (normal range)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


def bf16_ambiguous(v, window):
    """elements of v (float64) within `window` (absolute, per element) of a bf16 rounding boundary - the midpoint of two
    neighbouring bf16 numbers: a value computed with an error of up to `window` may round to either neighbour"""
    ulp = bf16_ulp(v)
    frac = torch.remainder(v.abs() / ulp, 1.0)                   # position between the two neighbours, in ulps
    return (frac - 0.5).abs() * ulp <= window


def decode_qkv(x, gamma, eps, wqkv, D, wrong=None):
    """stage 1: (q [D], k | v row [2 Hkv 64]) = Wqkv . bf16(rmsnorm(x)) before the bf16 store, and the prologue value"""
    xh = decode_rms_prologue(x, gamma, eps, wrong)
    y = gemv(wqkv, bf16r(xh))
    kv = y[D:]
    if wrong == "kv_swapped":
        kv = torch.cat([kv[kv.shape[0] // 2:], kv[:kv.shape[0] // 2]])
    return y[:D], kv, xh


def decode_attention(q, cache, H, Hkv, t0, cos, sin, round_points=False, wrong=None):
    """stage 2: the query of position t0 against cache rows 0 .. t0 (k | v per row, un-rotated), rot 64, causal; returns
    attention_ref's tuple with B = Nq = 1"""
    rows = t0 if wrong == "t0_rows" else t0 + 1
    kvw = Hkv * 64
    return attention_ref(q[None, None, :], cache[None, :rows, :kvw], cache[None, :rows, kvw:], H, Hkv, 64, rot=64, cos=cos, sin=sin,
                         causal=True, round_points=round_points)


def decode_mlp_out(x2, hf, wdown, wrong=None, x=None):
    """stage 5: x2 + Wdown . bf16(up * silu(gate)), and the prologue value"""
    act = decode_swiglu_prologue(hf, "gate_silu_up" if wrong == "gate_silu_up" else None)
    return gemv(wdown, bf16r(act), x if wrong == "residual_x" else x2), act
