"""The fp64 references of tests/kernel_refs.py against the torch ops they stand for (CPU, float64, 1e-12 relative): every
hand-written forward against the torch op, every closed-form backward against float64 autograd over that op.  This is what
lets tests/test_norm_elementwise_gpu.py trust them."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as kr  # noqa: E402

REL = 1e-12


def _rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _close(a, b, what=""):
    err = (a - b).abs().max().item()
    mag = max(b.abs().max().item(), 1e-300)
    assert err <= REL * mag, (what, err, mag)


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("mod", ["none", "scale", "shift", "both"])
def test_layernorm(beta, mod):
    rows, D, rpb = 11, 40, 4
    nb = (rows + rpb - 1) // rpb
    x, gam, bet = _leaf(_rn(rows, D, seed=1) * 1.5 + 0.3), _leaf(1 + 0.2 * _rn(D, seed=2)), _leaf(0.1 * _rn(D, seed=3))
    sc, sh = _rn(nb, D, seed=4, scale=0.3), _rn(nb, D, seed=5, scale=0.3)
    idx = torch.arange(rows) // rpb
    ln = F.layer_norm(x, (D,), gam, bet if beta else None, 1e-5)
    y = ln
    if mod in ("scale", "both"):
        y = y * (1 + sc[idx])
    if mod in ("shift", "both"):
        y = y + sh[idx]
    yr, mean, rstd = kr.layernorm_fwd(x.detach(), gam.detach(), bet.detach() if beta else None,
                                      sc if mod in ("scale", "both") else None, sh if mod in ("shift", "both") else None, rpb, 1e-5)
    _close(yr, y.detach(), "y")
    _close(mean, x.detach().mean(-1), "mean")
    _close(rstd, (x.detach().var(-1, unbiased=False) + 1e-5).rsqrt(), "rstd")
    dy, dres = _rn(rows, D, seed=6), _rn(rows, D, seed=7)
    y.backward(dy)
    dx, dg, db = kr.layernorm_bwd(dy, x.detach(), gam.detach(), mean, rstd, sc if mod in ("scale", "both") else None, rpb, dres)
    _close(dx, x.grad + dres, "dx")
    _close(dg, gam.grad, "dgamma")
    if beta:
        _close(db, bet.grad, "dbeta")


@pytest.mark.parametrize("beta", [False, True])
def test_adaln_mod_bwd(beta):
    nb, rpb, D = 3, 5, 24
    x, gam, bet = _rn(nb * rpb, D, seed=1), 1 + 0.2 * _rn(D, seed=2), 0.1 * _rn(D, seed=3)
    sc, sh = _leaf(_rn(nb, D, seed=4, scale=0.3)), _leaf(_rn(nb, D, seed=5, scale=0.3))
    idx = torch.arange(nb * rpb) // rpb
    y = F.layer_norm(x, (D,), gam, bet if beta else None, 1e-5) * (1 + sc[idx]) + sh[idx]
    dy = _rn(nb * rpb, D, seed=6)
    y.backward(dy)
    _, mean, rstd = kr.layernorm_fwd(x, gam)
    ds, dh = kr.adaln_mod_bwd(dy, x, gam, bet if beta else None, mean, rstd, nb, rpb)
    _close(ds, sc.grad)
    _close(dh, sh.grad)


@pytest.mark.parametrize("per_batch", [False, True])
def test_rmsnorm(per_batch):
    rows, D, rpb = 10, 48, 4
    nb = (rows + rpb - 1) // rpb
    x = _leaf(_rn(rows, D, seed=1) * 1.4)
    s = _leaf(1 + 0.2 * _rn(*((nb, D) if per_batch else (D,)), seed=2))
    srow = s[torch.arange(rows) // rpb] if per_batch else s
    y = x * srow * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
    if not per_batch and hasattr(F, "rms_norm"):
        _close(y.detach(), F.rms_norm(x.detach(), (D,), s.detach(), 1e-6), "F.rms_norm")
    yr, rrms = kr.rmsnorm_fwd(x.detach(), s.detach(), rpb if per_batch else 0, 1e-6)
    _close(yr, y.detach())
    dy, dres = _rn(rows, D, seed=3), _rn(rows, D, seed=4)
    y.backward(dy)
    dx, ds = kr.rmsnorm_bwd(dy, x.detach(), s.detach(), rrms, rpb if per_batch else 0, dres)
    _close(dx, x.grad + dres)
    if not per_batch:
        _close(ds, s.grad)


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("mode", [1, 2])
def test_head_norm(mode, dh):
    rows, heads = 7, 3
    x = _leaf(_rn(rows, heads, dh, seed=1) * 1.3 + 0.2)
    gam, bet = _leaf(1 + 0.2 * _rn(dh, seed=2)), _leaf(0.1 * _rn(dh, seed=3))
    y = F.normalize(x, dim=-1) if mode == 1 else F.layer_norm(x, (dh,), gam, bet, 1e-6)
    _close(kr.head_norm_fwd(x.detach(), mode, gam.detach(), bet.detach()), y.detach())
    g = _rn(rows, heads, dh, seed=4)
    y.backward(g)
    dx, dg, db = kr.head_norm_bwd(x.detach(), g, mode, gam.detach())
    _close(dx, x.grad)
    if mode == 2:
        _close(dg, gam.grad)
        _close(db, bet.grad)


def test_head_norm_l2_zero_head():
    """an all-zero head: F.normalize gives 0 forward and, the clamp being active, the gradient g / 1e-12 - the map is x * 1e12"""
    x = _rn(2, 2, 32, seed=1)
    x[1, 0] = 0
    x = _leaf(x)
    y = F.normalize(x, dim=-1)
    g = _rn(2, 2, 32, seed=2)
    y.backward(g)
    assert y[1, 0].abs().max().item() == 0 and kr.head_norm_fwd(x.detach(), 1)[1, 0].abs().max().item() == 0
    _close(kr.head_norm_bwd(x.detach(), g, 1)[0], x.grad)
    _close(x.grad[1, 0], g[1, 0] * 1e12)


EDGE = [0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 20.0, -20.0, 90.0, -90.0]


def _act_inputs():
    return torch.cat([_rn(200, seed=1) * 3, torch.tensor(EDGE, dtype=torch.float64)])


def test_silu_swiglu():
    x = _leaf(_act_inputs())
    y = F.silu(x)
    _close(kr.silu_fwd(x.detach()), y.detach())
    _close(kr.sigmoid(x.detach()), torch.sigmoid(x.detach()))
    dy = _rn(x.numel(), seed=2)
    y.backward(dy)
    _close(kr.silu_bwd(dy, x.detach()), x.grad)
    h = _leaf(torch.cat([_rn(6, 16, seed=3), _act_inputs()[-16:].repeat(6, 1)], 1))
    out = h[:, :16] * F.silu(h[:, 16:])
    _close(kr.swiglu_fwd(h.detach()), out.detach())
    do = _rn(6, 16, seed=4)
    out.backward(do)
    _close(kr.swiglu_bwd(do, h.detach()), h.grad)


def test_gelu():
    x = _leaf(_act_inputs())
    y = F.gelu(x)
    ref = kr.gelu_fwd(x.detach())
    # F.gelu computes 1 + erf, which cancels below -4: compare there in absolute terms of |x| eps64, elsewhere at 1e-12
    assert ((ref - y.detach()).abs() <= REL * y.detach().abs() + 2.0 ** -52 * x.detach().abs()).all()
    assert abs(ref[x.detach() == -6.0].item() / (-6.0 * 0.5 * math.erfc(6 / math.sqrt(2))) - 1) < 1e-12
    dy = _rn(x.numel(), seed=2)
    y.backward(dy)
    assert ((kr.gelu_bwd(dy, x.detach()) - x.grad).abs() <= REL * x.grad.abs() + 2.0 ** -51 * dy.abs() * (1 + x.detach().abs())).all()


@pytest.mark.parametrize("objective", [0, 1])
def test_diffuse(objective):
    x, n = _rn(4, 9, seed=1), _rn(4, 9, seed=2)
    t = torch.tensor([0.0, 1.0, 0.3, 0.77], dtype=torch.float64)
    if objective == 0:
        a, s = torch.cos(t * math.pi / 2)[:, None], torch.sin(t * math.pi / 2)[:, None]
        xt, tg = x * a + n * s, n * a - x * s
    else:
        xt, tg = x * (1 - t[:, None]) + n * t[:, None], n - x
    r = kr.diffuse_fwd(x, n, t, objective)
    _close(r[0], xt)
    _close(r[1], tg)


@pytest.mark.parametrize("masked", [False, True])
def test_mse(masked):
    B, C, T = 3, 4, 7
    out, tgt = _leaf(_rn(B, C, T, seed=1)), _rn(B, C, T, seed=2)
    mask = None
    if masked:
        mask = (torch.rand(B, T, generator=torch.Generator().manual_seed(3)) > 0.4).to(torch.uint8)
        mask[1] = 0
        sel = mask.bool()[:, None, :].expand(B, C, T)
        loss = 0.7 * F.mse_loss(out[sel], tgt[sel])
    else:
        loss = 0.7 * F.mse_loss(out, tgt)
    loss.backward()
    ssq, cnt, lr, dout = kr.mse(out.detach(), tgt, mask, 0.7)
    _close(lr, loss.detach())
    _close(dout, out.grad)


def test_fourier_features():
    t, w = _rn(5, seed=1).abs(), _leaf(_rn(6, seed=2))
    f = 2 * math.pi * t[:, None] * w[None, :]
    out = torch.cat([f.cos(), f.sin()], -1)
    _close(kr.fourier_features(t, w.detach()), out.detach())
    do = _rn(5, 12, seed=3)
    out.backward(do)
    _close(kr.fourier_features_bwd(do, t, w.detach()), w.grad)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("steps", [1, 3])
def test_adam(decoupled, steps):
    n = 37
    p0 = _rn(n, seed=1)
    hp = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    p = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], **hp)
    pr, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for s in range(1, steps + 1):
        g = _rn(n, seed=10 + s)
        p.grad = g.clone()
        opt.step()
        pr, m, v = kr.adam_step(pr, g * 4.0, m, v, lr=hp["lr"], beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.05,
                                decoupled=decoupled, step=s, grad_scale=0.25)
    _close(pr, p.detach())
    _close(m, opt.state[p]["exp_avg"])
    _close(v, opt.state[p]["exp_avg_sq"])
    wrong = kr.adam_step(p0, _rn(n, seed=11), 0 * p0, 0 * p0, lr=hp["lr"], beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.05,
                         decoupled=True, step=1, grad_scale=1.0, decay_after=True)[0]
    right = kr.adam_step(p0, _rn(n, seed=11), 0 * p0, 0 * p0, lr=hp["lr"], beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.05,
                         decoupled=True, step=1, grad_scale=1.0)[0]
    assert (wrong - right).abs().max().item() > 1e-8          # (the wrong order is a different function)


def test_embed_mix():
    rows, D, V = 9, 8, 5
    ids = torch.tensor([0, 3, 3, 4, -100, 3, 0, 1, -100])
    im = torch.tensor([1, 1, 0.5, 1, 0, 1, 1, 0.25, 0], dtype=torch.float64)
    am = torch.tensor([0, 0, 0.5, 0, 1, 0, 1, 0.75, 1], dtype=torch.float64)
    table, audio = _leaf(_rn(V, D, seed=1)), _leaf(_rn(rows, D, seed=2))
    out = audio * am[:, None] + F.embedding(ids.clamp_min(0), table) * im[:, None]
    a2 = audio.detach().clone()
    a2[am == 0] = float("nan")
    _close(kr.embed_mix_fwd(ids, table.detach(), a2, im, am), out.detach())
    do = _rn(rows, D, seed=3)
    out.backward(do)
    dt, da = kr.embed_mix_bwd(do, ids, im, am, V)
    _close(dt, table.grad)
    _close(da, audio.grad)


def test_gauss_kl():
    rows, dim, std = 6, 5, 0.7
    pred, label = _leaf(_rn(rows, dim, seed=1)), _rn(rows, dim, seed=2)
    ma = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.float64)
    mb = torch.tensor([0, 1, 0, 0, 1, 1], dtype=torch.float64)
    s = torch.full((rows, dim), std, dtype=torch.float64)
    kl = torch.distributions.kl_divergence(torch.distributions.Normal(pred, s), torch.distributions.Normal(label, s)).sum(-1) / dim
    la, lb = (kl * ma).sum() / ma.sum(), (kl * mb).sum() / mb.sum()
    s4 = kr.gauss_kl_fwd(pred.detach(), label, ma, mb, std)
    _close(s4[0] / s4[1], la.detach())
    _close(s4[2] / s4[3], lb.detach())
    (1.3 * la - 0.4 * lb).backward()
    _close(kr.gauss_kl_bwd(pred.detach(), label, ma, mb, s4, 1.3, -0.4, std), pred.grad)


@pytest.mark.parametrize("K,pad", [(1, 0), (17, 8), (17, 0), (17, 16), (32, 8), (32, 31)])
@pytest.mark.parametrize("N", [1, 5, 40])
def test_dwconv(K, pad, N):
    B, D = 2, 6
    x, w = _leaf(_rn(B, N, D, seed=1)), _leaf(_rn(D, K, seed=2))
    # y[n] = sum_k w[k] x[n + k - pad]: cross-correlation with left pad `pad`, right pad K - 1 - pad
    y = F.conv1d(F.pad(x.transpose(1, 2), (pad, K - 1 - pad)), w[:, None, :], groups=D).transpose(1, 2)
    _close(kr.dwconv1d_fwd(x.detach(), w.detach(), pad), y.detach())
    dy = _rn(B, N, D, seed=3)
    y.backward(dy)
    _close(kr.dwconv1d_wgrad(dy, x.detach(), K, pad), w.grad)
    _close(kr.dwconv1d_fwd(dy, w.detach(), K - 1 - pad, flip=True), x.grad)        # the data gradient, as the header says
    if N > 1:
        k = min(K - 1, pad)                                  # a tap that reaches inside the signal
        assert (kr.dwconv1d_fwd(x.detach(), w.detach(), pad, tap_shift=(k, 1)) - y.detach()).abs().max().item() > 1e-6


def test_small_ones():
    x, t = _rn(3, 8, seed=1), _rn(8, seed=2)
    _close(kr.add_rows(x, t), x + t)
    _close(kr.transpose_2d(_rn(2, 3, 5, seed=3)), _rn(2, 3, 5, seed=3).permute(0, 2, 1))
    _close(kr.colsum(x), x.sum(0))
    v = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -9, 3.14159], dtype=torch.float32)      # two ties, one plain
    assert kr.bf16r(v).tolist() == [1.0, 1.0 + 2.0 ** -7, 3.140625]


def test_axpby_peak():
    x, y = _rn(9, seed=1), _rn(9, seed=2)
    _close(kr.axpby(x, y, 0.3, -1.7), torch.add(0.3 * x, y, alpha=-1.7))
    v, peak = kr.peak_normalize(x)
    assert peak.item() == x.abs().max().item()
    assert (v.trunc().to(torch.int16) == ((x / x.abs().max()).clamp(-1, 1) * 32767).to(torch.int16)).all()
    assert v.abs().max().item() == 32767


@pytest.mark.parametrize("masked", [False, True])
def test_grad_cast(masked):
    """x_out = x_in + branch * sigmoid(1 - gate[b]) (rows with row_mask 0 contribute nothing): d / d branch and d / d gate"""
    nb, rpb, D = 3, 4, 6
    branch, gate = _leaf(_rn(nb * rpb, D, seed=1)), _leaf(_rn(nb, D, seed=2) * 2)
    x_in, g = _rn(nb * rpb, D, seed=3), _rn(nb * rpb, D, seed=4)
    mask = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0], dtype=torch.uint8) if masked else None
    keep = 1.0 if mask is None else mask.double()[:, None]
    idx = torch.arange(nb * rpb) // rpb
    x_out = x_in + branch * keep * torch.sigmoid(1 - gate)[idx]
    x_out.backward(g)
    gb, dgate = kr.grad_cast(g, x_out.detach(), x_in, gate.detach(), mask, nb, rpb)
    _close(gb, branch.grad)
    # the identity the kernel's form rests on: branch * keep = (x_out - x_in) / s, so d gate = -(1 - s) sum g (x_out - x_in)
    _close(dgate, gate.grad)
    _close(kr.grad_cast(g, None, None, None, mask, nb, rpb)[0], g * keep)


@pytest.mark.parametrize("mode", [0, 1])
def test_gauss_kl2(mode):
    rows, dim, mult = 6, 5, 1.25
    pred = _leaf(_rn(rows, 2 * dim, seed=1) * 0.5)
    ma = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.float64)
    mb = 1 - ma
    if mode == 0:
        lm, ls = _rn(rows, dim, seed=2), _rn(rows, dim, seed=3).abs() + 0.1
        m1, s1 = lm, ls * mult
    else:
        lm, ls = _rn(rows, 2 * dim, seed=2) * 3, None
        lm[0, dim] = 25.0                                   # above F.softplus's threshold
        m1, s1 = lm[:, :dim], (F.softplus(lm[:, dim:]) + 1e-4) * mult
    kl = torch.distributions.kl_divergence(torch.distributions.Normal(m1, s1),
                                           torch.distributions.Normal(pred[:, :dim], pred[:, dim:].exp())).sum(-1) / dim
    la, lb = (kl * ma).sum() / ma.sum(), (kl * mb).sum() / mb.sum()
    s4 = kr.gauss_kl2_fwd(pred.detach(), lm, ls, mode, mult, ma, mb)
    _close(s4[0] / s4[1], la.detach())
    _close(s4[2] / s4[3], lb.detach())
    (1.3 * la - 0.4 * lb).backward()
    _close(kr.gauss_kl2_bwd(pred.detach(), lm, ls, mode, mult, ma, mb, s4, 1.3, -0.4), pred.grad)
