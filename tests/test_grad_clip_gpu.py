"""-m gpu, kernel level: kalle_grad_sumsq / kalle_grad_norm_finish / kalle_adam_step_ctl against tests/grad_clip_refs.py.

Norm          every n of grad_clip_refs.NORM_N x nslots of NORM_SLOTS x four value kinds; slot s reads the window
              buf[64 (s + 1) : 64 (s + 1) + n] of one buffer.  |norm - N64| <= N64 (2^-24 + n_total 2^-53) - the derivation stands next
              to grad_clip_refs.norm_bound.  The same slots written in a permuted order give the same workspace and ctl bytes; the
              workspace and ctl sit between NaN sentinels that must survive; every partial of every region is written.
Coefficient   within one fp32 ulp of grad_clip_refs.coef64 of the device's published norm; exactly 1 for max_norm 0 / inf / far above.
Non-finite    +inf, -inf, NaN at element 0, in the scalar tail and in a middle workgroup's range.
Adam          kalle_adam_step_ctl bit for bit against kalle_adam_step(grad_scale = f32(gs * coef)); skip leaves every byte.
Wrong refs    grad_clip_refs.NORM_WRONG against the device's norm: all outside the bound."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_clip_refs as gc  # noqa: E402
import trainer_oracle as to  # noqa: E402

GUARD = 4096          # sentinel bytes on either side of the workspace


def _guarded_ws(nslots, dev):
    from kalle_audio_amd import ops
    nbytes = ops.grad_norm_ws(nslots, dev).numel()
    assert nbytes == nslots * gc.PARTIALS * 12
    raw = torch.full((GUARD + nbytes + GUARD,), 0xFF, device=dev, dtype=torch.uint8)        # (all-ones bytes: NaN as fp64 / fp32, -1 as int)
    return raw, raw[GUARD:GUARD + nbytes]


def _guarded_ctl(dev):
    from kalle_audio_amd import ops
    raw = torch.full((24,), -1, device=dev, dtype=torch.int32)
    c = ops.OptCtl.__new__(ops.OptCtl)
    t = raw[8:16]
    t.zero_()
    c.t, c.norm, c.coef, c.nonfinite, c.skip = t, t[0:1].view(torch.float32), t[1:2].view(torch.float32), t[2:3], t[3:4]
    c.skipped, c.clipped = t[4:6].view(torch.int64), t[6:8].view(torch.int64)
    return raw, c


def _guards_intact(raw_ws, raw_ctl):
    return (bool((raw_ws[:GUARD] == 0xFF).all()) and bool((raw_ws[-GUARD:] == 0xFF).all())
            and bool((raw_ctl[:8] == -1).all()) and bool((raw_ctl[16:] == -1).all()))


def _run_norm(buf_dev, n, nslots, dev, order=None, **fin):
    """sums of the slots' windows in `order`, then finish.  Returns (raw_ws, ws, raw_ctl, ctl)."""
    from kalle_audio_amd import ops
    raw_ws, ws = _guarded_ws(nslots, dev)
    raw_ctl, ctl = _guarded_ctl(dev)
    win = gc.slot_windows(n, nslots)
    for s in (order if order is not None else range(nslots)):
        a, b = win[s]
        ops.grad_sumsq(buf_dev[a:b], ws, s, nslots)
    ops.grad_norm_finish(ws, nslots, ctl, **fin)
    torch.cuda.synchronize()
    return raw_ws, ws, raw_ctl, ctl


@pytest.mark.parametrize("kind", gc.NORM_KINDS)
@pytest.mark.parametrize("nslots", gc.NORM_SLOTS)
@pytest.mark.parametrize("n", gc.NORM_N)
def test_norm(dev, n, nslots, kind):
    from kalle_audio_amd import ops
    buf = gc.norm_values(kind, gc.buffer_len(n, nslots), seed=n % 97 + nslots)
    chunks = [buf[a:b] for a, b in gc.slot_windows(n, nslots)]
    gs = 0.125
    sums = gc.sumsq64(chunks)
    n64 = gc.norm64(chunks, gs)
    bd = buf.to(dev)
    raw_ws, ws, raw_ctl, ctl = _run_norm(bd, n, nslots, dev, grad_scale=gs, max_norm=0.0)
    assert _guards_intact(raw_ws, raw_ctl)
    part, bad = ops.grad_norm_ws_views(ws, nslots)
    part, bad = part.cpu(), bad.cpu()
    assert torch.isfinite(part).all() and (part >= 0).all() and (bad == 0).all()        # every partial written, none flagged
    if n < 4 * gc.PARTIALS * gc.BLOCK:
        assert (part[:, (n // 4 + gc.BLOCK - 1) // gc.BLOCK + 1:] == 0).all()             # workgroups with no element write zeros
    for s in range(nslots):                                                              # each region holds ITS window's sum
        got = part[s].sum().item()
        assert abs(got - sums[s]) <= sums[s] * (n + gc.PARTIALS) * 2.0 ** -53, (s, got, sums[s])
    norm = ctl.norm.item()
    err, lim = abs(norm - n64), gc.norm_bound(n64, n * nslots)
    print(f"GRADNORM n {n} slots {nslots} {kind}: norm {norm:.9e} ref {n64:.9e} err/bound {err / lim:.3f}")
    assert err <= lim, (norm, n64, err, lim)
    assert ctl.coef.item() == 1.0 and ctl.nonfinite.item() == 0 and ctl.skip.item() == 0
    assert ctl.skipped.item() == 0 and ctl.clipped.item() == 0
    # the same slots in a permuted order: the same bytes everywhere
    order = list(reversed(range(nslots)))
    if nslots > 2:
        order = order[1::2] + order[0::2]
    raw2, ws2, rawc2, ctl2 = _run_norm(bd, n, nslots, dev, order=order, grad_scale=gs, max_norm=0.0)
    assert torch.equal(raw2, raw_ws) and torch.equal(rawc2, raw_ctl)


@pytest.fixture(scope="module")
def mid_case(dev):
    """one mid-sized case shared by the coefficient / wrong-reference tests: (n, nslots, chunks, device buffer)"""
    n, nslots = 4097, 3
    buf = gc.norm_values("normal", gc.buffer_len(n, nslots), seed=4)
    return n, nslots, [buf[a:b] for a, b in gc.slot_windows(n, nslots)], buf.to(dev)


def test_coefficient(dev, mid_case):
    n, nslots, chunks, bd = mid_case
    gs = 0.5
    n64 = gc.norm64(chunks, gs)
    for max_norm, exact_one in ((0.0, True), (math.inf, True), (1e30, True), (n64 * 1e3, True), (n64 * 0.5, False), (n64 * 0.999, False),
                                (1e-3, False), (1e-30, False)):
        raw_ws, ws, raw_ctl, ctl = _run_norm(bd, n, nslots, dev, grad_scale=gs, max_norm=max_norm)
        norm, coef = ctl.norm.item(), ctl.coef.item()
        assert abs(norm - n64) <= gc.norm_bound(n64, n * nslots)
        want = gc.coef64(norm, max_norm, round32=False)
        assert abs(coef - want) <= gc.ulp32(want), (max_norm, coef, want)
        assert (coef == 1.0) == exact_one, (max_norm, coef)
        assert ctl.clipped.item() == (0 if exact_one else 1) and ctl.skipped.item() == 0
        assert _guards_intact(raw_ws, raw_ctl)


@pytest.mark.parametrize("where", ["first", "tail", "middle"])
@pytest.mark.parametrize("value", [math.inf, -math.inf, math.nan], ids=["+inf", "-inf", "nan"])
def test_nonfinite(dev, value, where):
    from kalle_audio_amd import ops
    n, nslots = 4 * 75000 + 3, 3
    pos = {"first": 0, "tail": n - 1, "middle": 4 * (37 * gc.BLOCK + 11) + 2}[where]        # (workgroup 37's first sweep)
    buf = gc.norm_values("normal", gc.buffer_len(n, nslots), seed=9)
    a, b = gc.slot_windows(n, nslots)[1]
    buf[a + pos] = value
    bd = buf.to(dev)
    for skip_nonfinite in (False, True):
        raw_ws, ws, raw_ctl, ctl = _run_norm(bd, n, nslots, dev, grad_scale=1.0, max_norm=1.0, skip_nonfinite=skip_nonfinite)
        part, bad = ops.grad_norm_ws_views(ws, nslots)
        bad = bad.cpu()
        want = torch.zeros_like(bad)         # (the slots' windows overlap: the element lies in every window that covers a + pos)
        for s, (lo, hi) in enumerate(gc.slot_windows(n, nslots)):
            rel = a + pos - lo
            if 0 <= rel < n:
                want[s, 0 if rel >= n // 4 * 4 else (rel // 4) % (gc.PARTIALS * gc.BLOCK) // gc.BLOCK] = 1
        assert want[1].sum().item() == 1 and torch.equal(bad, want), (bad.nonzero(), want.nonzero())
        assert ctl.nonfinite.item() == 1 and ctl.skip.item() == int(skip_nonfinite)
        assert ctl.skipped.item() == int(skip_nonfinite) and _guards_intact(raw_ws, raw_ctl)
        # the counters advance by one per finish
        ops.grad_norm_finish(ws, nslots, ctl, grad_scale=1.0, max_norm=1.0, skip_nonfinite=skip_nonfinite)
        torch.cuda.synchronize()
        assert ctl.skipped.item() == 2 * int(skip_nonfinite)


def test_large_finite_values_raise_no_flag(dev):
    n, nslots = 4099, 3
    bd = torch.full((gc.buffer_len(n, nslots),), 3e38, device=dev)
    raw_ws, ws, raw_ctl, ctl = _run_norm(bd, n, nslots, dev, grad_scale=1.0, max_norm=0.0, skip_nonfinite=True)
    assert ctl.nonfinite.item() == 0 and ctl.skip.item() == 0 and ctl.skipped.item() == 0
    assert math.isinf(ctl.norm.item())          # 3e38 sqrt(12297) is no fp32 - the norm says so, the flags speak of the ELEMENTS


def test_wrong_norm_references_fail_on_the_device_norm(dev, mid_case):
    n, nslots, chunks, bd = mid_case
    gs = 0.125
    _, _, _, ctl = _run_norm(bd, n, nslots, dev, grad_scale=gs, max_norm=0.0)
    norm = ctl.norm.item()
    n64 = gc.norm64(chunks, gs)
    assert abs(norm - n64) <= gc.norm_bound(n64, n * nslots)
    for wrong in gc.NORM_WRONG:
        w = gc.norm64(chunks, gs, wrong=wrong)
        assert abs(norm - w) > gc.norm_bound(w, n * nslots), wrong


# ------------------------------------------------------------------------------------------------ kalle_adam_step_ctl
def _adam_state(n, dev, with_bf16, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev)
    st = dict(p=p, g=(torch.randn(n, generator=g) * 3).to(dev), m=(torch.randn(n, generator=g) * 1e-2).to(dev),
              v=(torch.rand(n, generator=g) * 1e-3).to(dev), b=p.bfloat16() if with_bf16 else None)
    return st


@pytest.mark.parametrize("with_bf16", [True, False], ids=["mirror", "nomirror"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_adam_step_ctl_is_adam_step_with_the_product(dev, coef, decoupled, with_bf16):
    from kalle_audio_amd import ops
    n = 4 * 5000 + 3
    gs = 1.0 / 3
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, decoupled=decoupled, step=3)
    a, b = _adam_state(n, dev, with_bf16, 21), _adam_state(n, dev, with_bf16, 21)
    raw_ctl, ctl = _guarded_ctl(dev)
    ctl.coef.fill_(coef)
    ops.adam_step(a["p"], a["g"], a["m"], a["v"], a["b"], grad_scale=gc.f32_product(gs, coef), **hp)
    ops.adam_step_ctl(b["p"], b["g"], b["m"], b["v"], b["b"], ctl, grad_scale=gs, **hp)
    torch.cuda.synchronize()
    for key in ("p", "m", "v") + (("b",) if with_bf16 else ()):
        assert to._bits_equal(a[key].cpu(), b[key].cpu()), key
    assert (a["p"] != _adam_state(n, dev, with_bf16, 21)["p"]).any()
    # skip = 1: every output buffer keeps every byte
    ctl.skip.fill_(1)
    before = {k: v.clone() for k, v in b.items() if v is not None}
    ops.adam_step_ctl(b["p"], b["g"], b["m"], b["v"], b["b"], ctl, grad_scale=gs, **hp)
    torch.cuda.synchronize()
    for key, v in before.items():
        assert to._bits_equal(v.cpu(), b[key].cpu()), key
    assert bool((raw_ctl[:8] == -1).all()) and bool((raw_ctl[16:] == -1).all())
