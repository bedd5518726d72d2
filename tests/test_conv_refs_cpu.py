"""The fp64 references of the VAE conv stack (tests/kernel_refs.py, "VAE conv stack") against the torch ops they stand for
(CPU, float64, 1e-12 relative): F.conv1d over F.pad for the asymmetric padding, F.conv_transpose1d sliced or right-extended,
torch's weight_norm parametrisation for the fold and its backward, float64 autograd for every gradient, the oracle's
activation1d for act1d.  The data-gradient recipes of the header's backward section (stride-1 conv via fold flag 1 | 2, strided
conv via the transposed conv, transposed conv via the strided conv) are checked here reference against autograd, so that
tests/test_conv_gpu.py can hold the kernels to a target that is known to be right."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import kernel_refs as kr  # noqa: E402

REL = 1e-12


def _rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _close(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    mag = max(b.abs().max().item(), 1e-300)
    assert err <= REL * mag, (what, err, mag)


def _leaf(t):
    return t.clone().requires_grad_(True)


def _torch_act(x, code, alpha=None, beta=None, logscale=0, param=0.0):
    if code == 0:
        return x
    if code == 1:
        a, b = (alpha.exp(), beta.exp()) if logscale else (alpha, beta)
        return x + torch.sin(x * a[None, :, None]) ** 2 / (b[None, :, None] + 1e-9)
    if code == 2:
        return F.elu(x)
    if code == 3:
        return F.leaky_relu(x, param)
    h = x.shape[1] // 2
    return torch.tanh(x[:, :h]) * torch.sigmoid(x[:, h:])


def _unpack(w, Cout):
    """packed [Cin][K][CoutP] -> torch's Conv1d layout [Cout][Cin][K]"""
    return w[:, :, :Cout].permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("with_g", [False, True])
def test_weight_norm_fold(flags, with_g):
    d0, d1, K = 5, 11, 4
    v, g = _rn(d0, d1, K, seed=1), 1 + 0.3 * _rn(d0, seed=2)
    if flags & 1:
        m = torch.nn.utils.parametrizations.weight_norm(torch.nn.ConvTranspose1d(d0, d1, K, bias=False).double(), dim=0)
    else:
        m = torch.nn.utils.parametrizations.weight_norm(torch.nn.Conv1d(d1, d0, K, bias=False).double(), dim=0)
    with torch.no_grad():
        m.parametrizations.weight.original0.copy_(g.view(-1, 1, 1))
        m.parametrizations.weight.original1.copy_(v)
    wt = m.weight.detach() if with_g else v                    # [d0][d1][K]
    if flags & 2:
        wt = wt.flip(2)
    want = wt.permute(0, 2, 1) if flags & 1 else wt.permute(1, 2, 0)
    got = kr.weight_norm_fold(v, g if with_g else None, flags)
    cout = d1 if flags & 1 else d0
    assert got.shape == (want.shape[0], K, (cout + 7) // 8 * 8)
    _close(got[:, :, :cout], want.contiguous(), "fold")
    assert (got[:, :, cout:] == 0).all()


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("logscale", [0, 1])
def test_act(code, logscale):
    C = 6
    x = _rn(2, C, 33, seed=3, scale=2.0)
    al, be = _rn(C // 2 if code == 4 else C, seed=4, scale=0.5), _rn(C // 2 if code == 4 else C, seed=5, scale=0.5)
    if not logscale:
        al, be = al.exp(), be.exp()
    _close(kr.act(x, code, al, be, logscale, 0.2), _torch_act(x, code, al, be, logscale, 0.2), "act")
    if code == 1:
        _close(kr.snake_beta(x, al, be, logscale), _torch_act(x, 1, al, be, logscale), "snake_beta")


CONV_CASES = [
    # Cin, Cout, K, stride, pad_left, pad_right, dilation, Lin
    (3, 5, 1, 1, 0, 0, 1, 17),
    (4, 9, 7, 1, 3, 3, 1, 40),
    (4, 9, 7, 1, 6, 0, 1, 40),          # causal
    (4, 3, 7, 1, 0, 6, 1, 40),          # right-heavy
    (5, 4, 3, 1, 9, 9, 9, 30),
    (5, 4, 7, 1, 27, 27, 9, 20),        # Lin shorter than the halo
    (2, 6, 4, 2, 1, 1, 1, 31),
    (2, 6, 8, 4, 2, 2, 1, 45),
    (3, 2, 16, 8, 4, 4, 1, 70),
    (3, 2, 6, 3, 2, 1, 1, 29),
    (3, 7, 2, 1, 0, 1, 1, 12),          # torch 'same' for an even kernel: the odd zero goes to the right
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("act", [0, 1, 4])
def test_conv1d(case, act):
    Cin, Cout, K, stride, pl, pr, dil, Lin = case
    B = 2
    x = _rn(B, 2 * Cin if act == 4 else Cin, Lin, seed=6)
    v, bias = _rn(Cout, Cin, K, seed=7), _rn(Cout, seed=8)
    al, be = _rn(Cin, seed=9, scale=0.4), _rn(Cin, seed=10, scale=0.4)
    w = kr.weight_norm_fold(v, None, 0)
    Lout = (Lin + pl + pr - dil * (K - 1) - 1) // stride + 1
    want = F.conv1d(F.pad(_torch_act(x, act, al, be, 1), (pl, pr)), v, bias, stride=stride, dilation=dil)
    y, raw, asum = kr.conv1d(x, w, Cout, bias, stride, pl, dil, Lout, (act, al, be, 1, 0.0))
    _close(y, want, "conv1d")
    _close(raw, want, "y_raw without post")
    wa = F.conv1d(F.pad(_torch_act(x, act, al, be, 1).abs(), (pl, pr)), v.abs(), bias.abs(), stride=stride, dilation=dil)
    _close(asum, wa, "abs_sum")


def test_conv1d_epilogue_order():
    B, Cin, Cout, K, L = 2, 3, 5, 3, 20
    x, v, bias = _rn(B, Cin, L, seed=11), _rn(Cout, Cin, K, seed=12), _rn(Cout, seed=13)
    res, y0 = _rn(B, Cout, L, seed=14), _rn(B, Cout, L, seed=15)
    pa, pb = _rn(Cout, seed=16, scale=0.3), _rn(Cout, seed=17, scale=0.3)
    conv = F.conv1d(x, v, bias, padding=1)
    raw_want = (conv + res) * 0.7 + y0
    want = torch.tanh(_torch_act(raw_want, 1, pa, pb, 1))
    ep = dict(residual=res, out_scale=0.7, accumulate=y0, post=(1, pa, pb, 1, 0.0), tanh=1)
    y, raw, asum = kr.conv1d(x, kr.weight_norm_fold(v, None, 0), Cout, bias, 1, 1, 1, L, None, ep)
    _close(y, want, "y")
    _close(raw, raw_want, "y_raw")
    wa = (F.conv1d(x.abs(), v.abs(), bias.abs(), padding=1) + res.abs()) * 0.7 + y0.abs()
    _close(asum, wa, "abs_sum")


CONVT_CASES = [
    # Cin, Cout, K, stride, padding, Lin, extra (Lout - symmetric length: < 0 trims, > 0 extends by up to `padding`)
    (3, 5, 4, 2, 1, 13, 0),
    (3, 5, 7, 3, 2, 13, 0),
    (4, 2, 8, 4, 2, 9, -4),             # causal trim of the last `stride` outputs
    (4, 2, 8, 4, 2, 9, 2),              # `padding` longer
    (2, 9, 11, 5, 3, 7, 3),
    (2, 9, 16, 8, 4, 6, 1),
    (5, 3, 3, 1, 1, 10, 0),
]


@pytest.mark.parametrize("case", CONVT_CASES)
def test_conv_transpose1d(case):
    Cin, Cout, K, stride, pad, Lin, extra = case
    B = 2
    x, v, bias = _rn(B, Cin, Lin, seed=18), _rn(Cin, Cout, K, seed=19), _rn(Cout, seed=20)
    Lout = (Lin - 1) * stride - 2 * pad + K + extra
    full = F.conv_transpose1d(F.elu(x), v, bias, stride=stride, padding=0)       # every output, no trim
    want = full[:, :, pad:pad + Lout]
    if extra <= 0:
        sym = F.conv_transpose1d(F.elu(x), v, bias, stride=stride, padding=pad)
        _close(want, sym[:, :, :Lout], "torch slicing")
    y, raw, asum = kr.conv_transpose1d(x, kr.weight_norm_fold(v, None, 1), Cout, bias, stride, pad, Lout, (2, None, None, 0, 0.0))
    _close(y, want, "conv_transpose1d")
    wa = F.conv_transpose1d(F.elu(x).abs(), v.abs(), bias.abs(), stride=stride)[:, :, pad:pad + Lout]
    _close(asum, wa, "abs_sum")


@pytest.mark.parametrize("phases,padding,Lp", [(1, 0, 20), (1, 6, 40), (1, 3, 16), (2, 2, 32), (4, 4, 48), (8, 8, 64)])
def test_conv_pad_act(phases, padding, Lp):
    B, C, Lin = 2, 3, 20
    x = _rn(B, C, Lin, seed=21)
    al, be = _rn(C, seed=22, scale=0.3), _rn(C, seed=23, scale=0.3)
    got = kr.conv_pad_act(x, Lp, padding, (1, al, be, 1, 0.0), phases)
    a = _torch_act(x, 1, al, be, 1)
    lin = F.pad(a, (padding, max(0, Lp - padding - Lin)))[:, :, :Lp]
    want = torch.empty_like(lin)
    for j in range(Lp):                                        # the header's sentence, slot by slot
        want[:, :, (j % phases) * (Lp // phases) + j // phases] = lin[:, :, j]
    _close(got, want, "pad_act")


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_gradients_and_data_gradient_recipes(case):
    """dW = conv_wgrad(U = dy, V = x, act on V); dx of a stride-1 conv = conv1d over dy with fold flag 1 | 2 and padding
    (K-1) dil - pad; dx of a strided conv = conv_transpose1d over dy with fold flag 1 and the same padding, Lout = Lin"""
    Cin, Cout, K, stride, pl, pr, dil, Lin = case
    B = 2
    x, v, g = _leaf(_rn(B, Cin, Lin, seed=24)), _leaf(_rn(Cout, Cin, K, seed=25)), _rn(Cout, seed=26).abs() + 0.5
    h = F.elu(x)
    h.retain_grad()
    w = v * (g / v.flatten(1).norm(dim=1)).view(-1, 1, 1)
    w.retain_grad()
    y = F.conv1d(F.pad(h, (pl, pr)), w, None, stride=stride, dilation=dil)
    Lout = y.shape[2]
    dy = _rn(B, Cout, Lout, seed=27)
    y.backward(dy)
    dW, _ = kr.conv_wgrad(dy, x.detach(), K, stride, pl, dil, 0, (2, None, None, 0, 0.0))
    _close(dW, w.grad, "dW")
    vd = v.detach()
    if stride == 1:
        wd = kr.weight_norm_fold(vd, g, 1 | 2)               # a Conv1d's (v, g) read as [Cin' = Cout][Cout' = Cin][K], flipped
        dh, _, _ = kr.conv1d(dy, wd, Cin, None, 1, (K - 1) * dil - pl, dil, Lin)
    else:
        wd = kr.weight_norm_fold(vd, g, 1)
        if Lin > (Lout - 1) * stride - pl + K:               # inputs no output ever read: beyond the transposed conv's range
            n = (Lout - 1) * stride - pl + K
            dh, _, _ = kr.conv_transpose1d(dy, wd, Cin, None, stride, pl, n)
            dh = F.pad(dh, (0, Lin - n))
        else:
            dh, _, _ = kr.conv_transpose1d(dy, wd, Cin, None, stride, pl, Lin)
    _close(dh, h.grad, "data gradient")
    dv, dg = kr.weight_norm_bwd(w.grad, vd, g)
    _close(dv, v.grad, "weight_norm_bwd dv")
    gl = _leaf(g)
    (vd * (gl / vd.flatten(1).norm(dim=1)).view(-1, 1, 1) * w.grad).sum().backward()
    _close(dg, gl.grad, "weight_norm_bwd dg")


@pytest.mark.parametrize("case", [c for c in CONVT_CASES if c[6] <= 0])      # (no module produces the extended length)
def test_conv_transpose_gradients(case):
    """ConvTranspose1d: dW [Cin][Cout][K] = conv_wgrad(U = act(x), V = dy, act on U); dx = conv1d over dy with fold flag 0 on
    the module's (v, g), the module's stride and padding"""
    Cin, Cout, K, stride, pad, Lin, extra = case
    B = 2
    x, v = _leaf(_rn(B, Cin, Lin, seed=28)), _leaf(_rn(Cin, Cout, K, seed=29))
    h = F.elu(x)
    h.retain_grad()
    y = F.conv_transpose1d(h, v, None, stride=stride, padding=pad)
    Lout = y.shape[2] + extra
    y = y[:, :, :Lout]
    dy = _rn(B, Cout, Lout, seed=30)
    y.backward(dy)
    dW, _ = kr.conv_wgrad(x.detach(), dy, K, stride, pad, 1, 1, (2, None, None, 0, 0.0))
    _close(dW, v.grad, "dW")
    dh, _, _ = kr.conv1d(dy, kr.weight_norm_fold(v.detach(), None, 0), Cin, None, stride, pad, 1, Lin)
    _close(dh, h.grad, "data gradient")


@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("logscale", [0, 1])
def test_act_bwd(code, logscale):
    B, C, L = 2, 5, 40
    x, g = _leaf(_rn(B, C, L, seed=31, scale=2.0)), _rn(B, C, L, seed=32)
    al, be = _leaf(_rn(C, seed=33, scale=0.4)), _leaf(_rn(C, seed=34, scale=0.4))
    if not logscale:
        al, be = _leaf(al.detach().exp()), _leaf(be.detach().exp())
    _torch_act(x, code, al, be, logscale).backward(g)
    dx, da, db, _ = kr.act_bwd(x.detach(), g, code, al.detach(), be.detach(), logscale)
    _close(dx, x.grad if code else g, "dx")
    if code == 1:
        _close(da, al.grad, "dalpha")
        _close(db, be.grad, "dbeta")


def test_tanh_bwd_upsample_channel_sum():
    x = _leaf(_rn(3, 4, 10, seed=35))
    y = torch.tanh(x)
    dy = _rn(3, 4, 10, seed=36)
    y.backward(dy)
    _close(kr.tanh_bwd(dy, y.detach()), x.grad, "tanh_bwd")
    _close(kr.channel_sum(dy), dy.sum((0, 2)), "channel_sum")
    for scale in (1, 2, 7, 64):
        r = _leaf(_rn(6, 9, seed=37))
        up = F.interpolate(r[None], scale_factor=scale, mode="nearest")[0]
        assert torch.equal(kr.upsample_nearest(r.detach(), scale), up.detach())
        d = _rn(6, 9 * scale, seed=38)
        up.backward(d)
        _close(kr.upsample_nearest(d, scale, backward=True), r.grad, "upsample bwd")


@pytest.mark.parametrize("mode", ["snake", "snake_log", "elu"])
@pytest.mark.parametrize("L", [1, 2, 13, 64])
def test_act1d_matches_oracle(mode, L):
    import kalle_oracle as ko
    B, C = 2, 3
    x = _rn(B, C, L, seed=39, scale=1.5)
    filt = ko.kaiser_sinc_filter1d(0.25, 0.3, 12).double()
    al, be = _rn(C, seed=40, scale=0.3), _rn(C, seed=41, scale=0.3)
    if mode == "elu":
        want = ko.downsample1d_2x(F.elu(ko.upsample1d_2x(x, filt)), filt)
        got = kr.act1d(x, filt)
    else:
        ls = mode == "snake_log"
        a, b = (al, be) if ls else (al.exp(), be.exp())
        want = ko.downsample1d_2x(ko.snake(ko.upsample1d_2x(x, filt), a, b, ls), filt)
        got = kr.act1d(x, filt, a, b, ls)
    _close(got, want, "act1d")
