"""fp64 references of the norm / elementwise / Llasa-tail / conformer entry points of include/kalle_hip.h.

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
