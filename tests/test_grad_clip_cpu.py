"""CPU: the gradient-norm clipping / non-finite skip feature without a device.

  * tests/grad_clip_refs.py against torch itself: clip_grad_norm_ + torch.optim.Adam / AdamW in fp64;
  * every refusal of the four C entry points (all made before any launch) and kalle_grad_norm_ws_bytes;
  * every wrong reference the GPU tests use lies outside the norm bound on the chosen inputs, and an fp32-accumulating sum
    lies outside it at the largest case;
  * engine.DataParallelTrainer's control flow with the four new ops functions replaced by torch stand-ins that record calls."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grad_clip_refs as gc  # noqa: E402
import kernel_refs as kr  # noqa: E402
import trainer_oracle as to  # noqa: E402

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the reference vs torch
@pytest.mark.parametrize("active", [True, False], ids=["clipping", "inactive"])
@pytest.mark.parametrize("opt", ["Adam", "AdamW"])
def test_reference_equals_torch_clip_and_adam_fp64(opt, active):
    """three steps of clip_grad_norm_ + torch.optim.Adam / AdamW in fp64 against norm64 / coef64 / kernel_refs.adam_step: final
    weights to 1e-12 (coefficient left in double), and the fp32-rounded coefficient within 2 fp32 ulp of torch's"""
    g0 = torch.Generator().manual_seed(5)
    shapes = [(37, 5), (64,), (3, 3, 7)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g0, dtype=F64)) for s in shapes]
    hp = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    o = (torch.optim.AdamW if opt == "AdamW" else torch.optim.Adam)(params, **hp)
    p = torch.cat([q.detach().reshape(-1) for q in params]).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    first = None
    for k in (1, 2, 3):
        grads = [torch.randn(s, generator=g0, dtype=F64) * 3 for s in shapes]
        first = first or gc.norm64(grads)
        max_norm = 0.5 * first if active else 1e9
        for q, g in zip(params, grads):
            q.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm).item()
        want_coef = min(1.0, max_norm / (total + 1e-6))
        n64 = gc.norm64(grads)
        assert abs(n64 - total) <= 1e-13 * total
        c = gc.coef64(n64, max_norm, round32=False)
        assert abs(gc.coef64(gc.f32(n64), max_norm) - want_coef) <= 2 * gc.ulp32(want_coef), (k, want_coef)
        assert (c < 1) == active
        o.step()
        p, m, v = kr.adam_step(p, torch.cat([g.reshape(-1) for g in grads]), m, v, lr=hp["lr"], beta1=0.9, beta2=0.999,
                               eps=hp["eps"], weight_decay=hp["weight_decay"], decoupled=opt == "AdamW", step=k, grad_scale=c)
    got = torch.cat([q.detach().reshape(-1) for q in params])
    assert (got - p).abs().max().item() <= 1e-12


def test_coef64_edges():
    assert gc.coef64(5.0, None) == 1.0 and gc.coef64(5.0, 0.0) == 1.0 and gc.coef64(5.0, math.inf) == 1.0
    assert gc.coef64(1e-3, 1.0) == 1.0 and gc.coef64(2.0, 1.0) == gc.f32(1.0 / (2.0 + 1e-6))
    assert gc.ulp32(1.0) == 2.0 ** -23 and gc.f32_product(0.5, 0.37) == gc.f32(0.5 * gc.f32(0.37))


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def _lib():
    from kalle_audio_amd import _lib as L
    return L.load()


def test_header_constants_and_ctl_layout():
    """ops.py / grad_clip_refs.py mirror the header's constants; kalle_opt_ctl is laid out as ops.OptCtl's views assume"""
    import subprocess
    from kalle_audio_amd import _lib as L, ops
    src = open(L.HEADER).read()
    const = {k: int(v) for k, v in re.findall(r"#define (KALLE_GRAD_NORM_\w+) (\d+)\n", src)}
    assert const == {"KALLE_GRAD_NORM_PARTIALS": gc.PARTIALS, "KALLE_GRAD_NORM_BLOCK": gc.BLOCK, "KALLE_GRAD_NORM_UNROLL": gc.UNROLL}
    assert (ops.GRAD_NORM_PARTIALS, ops.GRAD_NORM_BLOCK, ops.GRAD_NORM_UNROLL) == (gc.PARTIALS, gc.BLOCK, gc.UNROLL)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "kalle_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", '
            "sizeof(kalle_opt_ctl), offsetof(kalle_opt_ctl, norm), offsetof(kalle_opt_ctl, coef), offsetof(kalle_opt_ctl, nonfinite), "
            "offsetof(kalle_opt_ctl, skip), offsetof(kalle_opt_ctl, skipped), offsetof(kalle_opt_ctl, clipped), "
            "KALLE_GRAD_NORM_SLOT_BYTES); return 0; }\n")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.dirname(L.HEADER), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 12, 16, 24, gc.PARTIALS * 12]
    c = ops.OptCtl(torch.device("cpu"))
    base = c.t.data_ptr()
    assert [x.data_ptr() - base for x in (c.norm, c.coef, c.nonfinite, c.skip, c.skipped, c.clipped)] == [0, 4, 8, 12, 16, 24]
    assert c.coef.item() == 1.0 and c.skipped.dtype == torch.int64 and c.norm.dtype == torch.float32


def test_ws_bytes():
    lib = _lib()
    assert lib.kalle_grad_norm_ws_bytes(1) == gc.PARTIALS * 12 and lib.kalle_grad_norm_ws_bytes(26) == 26 * gc.PARTIALS * 12
    assert lib.kalle_grad_norm_ws_bytes(0) == -1 and lib.kalle_grad_norm_ws_bytes(-3) == -1
    assert lib.kalle_abi_version() == 2


P = ctypes.c_void_p(1 << 20)           # a plausible, aligned, never dereferenced address: every row below is refused before a launch
ODD = ctypes.c_void_p((1 << 20) + 4)   # not 16-byte (nor 8-byte) aligned
ADAM_OK = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, param_bf16=None, n=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
               weight_decay=0.0, decoupled=0, step=1, grad_scale=1.0, ctl=P, stream=None)
REFUSALS = {
    "kalle_grad_sumsq": (dict(grad=P, n=8, ws=P, slot=0, nslots=1, stream=None),
                         [dict(grad=None), dict(ws=None), dict(n=0), dict(n=-4), dict(nslots=0), dict(slot=-1), dict(slot=1),
                          dict(slot=3, nslots=3), dict(grad=ODD), dict(ws=ODD)]),
    "kalle_grad_norm_finish": (dict(ws=P, nslots=1, grad_scale=1.0, max_norm=1.0, skip_nonfinite=0, ctl=P, stream=None),
                               [dict(ws=None), dict(ctl=None), dict(nslots=0), dict(nslots=-1), dict(ws=ODD), dict(ctl=ODD)]),
    "kalle_adam_step_ctl": (ADAM_OK, [dict(param=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(ctl=None),
                                      dict(n=0), dict(n=-1), dict(step=0), dict(step=-2), dict(ctl=ODD)]),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_points_refuse_before_any_launch(name):
    """one table per entry point; each row breaks ONE argument of an otherwise valid call and must return KALLE_ERR_ARG (no
    device exists here: anything that got as far as a launch would report KALLE_ERR_LAUNCH instead)"""
    good, rows = REFUSALS[name]
    fn = getattr(_lib(), name)
    for row in rows:
        assert set(row) <= set(good), row
        args = dict(good, **row)
        assert fn(*args.values()) == -1, (name, row)


# ------------------------------------------------------------------------------------------------ the bound can tell
SENS = [("normal", 4097, 3), ("mixed", 255, 26), ("normal", gc.NORM_N[-1], 1)]      # the inputs of test_grad_clip_gpu's wrong references


@pytest.mark.parametrize("kind,n,nslots", SENS)
def test_wrong_norm_references_lie_outside_the_bound(kind, n, nslots):
    buf = gc.norm_values(kind, gc.buffer_len(n, nslots))
    chunks = [buf[a:b] for a, b in gc.slot_windows(n, nslots)]
    gs = 0.125
    n64 = gc.norm64(chunks, gs)
    lim = gc.norm_bound(n64, n * nslots)
    assert abs(gc.f32(n64) - n64) <= lim                       # what a right device publishes at best
    for wrong in gc.NORM_WRONG:
        assert abs(gc.norm64(chunks, gs, wrong=wrong) - n64) > lim, wrong


def test_fp32_accumulation_lies_outside_the_bound_at_the_largest_case():
    n = gc.NORM_N[-1]
    assert 8.3e6 < n < 8.5e6 and gc.SWEEP == gc.PARTIALS * gc.BLOCK * gc.UNROLL * 4
    buf = gc.norm_values("normal", gc.buffer_len(n, 1))
    chunks = [buf[a:b] for a, b in gc.slot_windows(n, 1)]
    n64 = gc.norm64(chunks)
    assert abs(gc.norm_fp32_accumulating(chunks) - n64) > gc.norm_bound(n64, n)


def test_step_defects_lie_outside_the_bound_on_a_standin():
    """clip_step's seeded defects against an fp32 stand-in of a right device (trainer_oracle.standin_step fed the clipped scale)"""
    g0 = torch.Generator().manual_seed(11)
    n = 512
    ranges = {"a.": (0, 192), "b.": (192, 384), "_rest": (384, 512)}
    cfg = to.make_cfg(lr=1e-2, weight_decay=0.01, decoupled=True, accum=2)
    st = dict(param=torch.randn(n, generator=g0), exp_avg=torch.randn(n, generator=g0) * 1e-2,
              exp_avg_sq=torch.rand(n, generator=g0) * 1e-3)
    G = torch.randn(n, generator=g0) * 4
    gs = gc.f32(0.5)
    norm = gc.f32(gc.norm64([G], gs))
    max_norm = 0.5 * norm
    coef = gc.coef64(norm, max_norm)
    assert coef < 1
    k, skipped = 3, 1                   # (step 2 was skipped)
    cfg_dev = dict(cfg, accum=1, world=1)
    p, m, v = to.standin_step(st, G * gc.f32_product(gs, coef), cfg_dev, k)
    after = dict(param=p, exp_avg=m, exp_avg_sq=v)
    kw = dict(coef=coef, max_norm=max_norm, skipped_before=skipped)
    assert not to.failures(gc.check_clip_step(st, after, G, cfg, k, ranges, **kw))
    for d in ("clip_per_bucket", "norm_of_sum", "coef_on_m_only", "torch_step_after_skip"):
        assert to.failures(gc.check_clip_step(st, after, G, cfg, k, ranges, defect=d, **kw)), d
    # a skipped step: a device that left every bit passes, and only the `_rest`-stepped reference objects
    Ginf = G.clone()
    Ginf[7] = math.inf
    same = dict(param=st["param"].clone(), exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone())
    assert not to.failures(gc.check_clip_step(st, same, Ginf, cfg, k, ranges, skip=True))
    bad = to.failures(gc.check_clip_step(st, same, Ginf, cfg, k, ranges, skip=True, defect="rest_on_skip"))
    assert bad and all(b[1] == "_rest" for b in bad)
    assert to.failures(gc.check_clip_step(st, after, G, cfg, k, ranges, skip=True))


# ------------------------------------------------------------------------------------------------ trainer control flow
class _Standins:
    """torch stand-ins of ops.grad_norm_ws / grad_sumsq / grad_norm_finish / adam_step_ctl (and a recording ops.adam_step)"""

    def __init__(self, monkeypatch):
        from kalle_audio_amd import ops
        self.calls = []
        for name in ("grad_norm_ws", "grad_sumsq", "grad_norm_finish", "adam_step_ctl", "adam_step"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def grad_norm_ws(self, nslots, device):
        self.calls.append(("ws", nslots))
        return torch.full((nslots, 2), math.nan, dtype=F64)

    def grad_sumsq(self, grad, ws, slot, nslots):
        self.calls.append(("sumsq", slot, grad.data_ptr(), grad.numel()))
        ws[slot, 0] = grad.double().pow(2).sum()
        ws[slot, 1] = float((~torch.isfinite(grad)).any())

    def grad_norm_finish(self, ws, nslots, ctl, *, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
        self.calls.append(("finish", nslots, grad_scale, max_norm, skip_nonfinite))
        norm = gc.f32(math.sqrt(ws[:, 0].sum().item()) * gc.f32(grad_scale)) if not ws[:, 0].isnan().any() else math.nan
        coef = gc.coef64(norm, max_norm) if norm == norm else 1.0
        bad = bool(ws[:, 1].sum().item() > 0)
        ctl.norm.fill_(norm)
        ctl.coef.fill_(coef)
        ctl.nonfinite.fill_(int(bad))
        ctl.skip.fill_(int(bad and skip_nonfinite))
        ctl.skipped.add_(int(bad and skip_nonfinite))
        ctl.clipped.add_(int(coef < 1))
        ws.fill_(math.nan)                 # (the trainer must write every slot again before the next finish)

    def adam_step_ctl(self, param, grad, exp_avg, exp_avg_sq, param_bf16, ctl, **kw):
        self.calls.append(("adam_ctl", param.numel(), dict(kw)))
        if ctl.skip.item():
            return
        self._adam(param, grad, exp_avg, exp_avg_sq, param_bf16, **dict(kw, grad_scale=gc.f32_product(kw["grad_scale"], ctl.coef.item())))

    def adam_step(self, param, grad, exp_avg, exp_avg_sq, param_bf16, **kw):
        self.calls.append(("adam", param.numel(), dict(kw)))
        self._adam(param, grad, exp_avg, exp_avg_sq, param_bf16, **kw)

    @staticmethod
    def _adam(param, grad, exp_avg, exp_avg_sq, param_bf16, *, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale):
        p, m, v = kr.adam_step(param, grad, exp_avg, exp_avg_sq, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                               decoupled=decoupled, step=step, grad_scale=grad_scale)
        param.copy_(p), exp_avg.copy_(m), exp_avg_sq.copy_(v)
        if param_bf16 is not None:
            param_bf16.copy_(param)

    def take(self):
        c, self.calls = self.calls, []
        return c


class _Net(torch.nn.Module):
    """three bucket units and a head outside them: buckets "a.", "b.", "c." and "_rest" """

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        for n in "abc":
            lin = torch.nn.Linear(6, 6)
            lin._kalle_bucket_unit = True
            setattr(self, n, lin)
        self.head = torch.nn.Linear(6, 1)

    def forward(self, x):
        return self.head(self.c(self.b(self.a(x)).tanh()).tanh())


ADAM_KW = {"lr", "beta1", "beta2", "eps", "weight_decay", "decoupled", "step", "grad_scale"}


def _micro(tr, net, seed, scale=1.0):
    if tr.micro % tr.grad_accum_steps == 0:
        tr.flat.grad.zero_()              # (plain autograd accumulates into the block buckets; the real blocks' kernels overwrite)
    x = torch.randn(5, 6, generator=torch.Generator().manual_seed(seed))
    tr.backward(net(x).pow(2).mean() * scale)


def _trainer(monkeypatch, **kw):
    from kalle_audio_amd import engine
    monkeypatch.delenv("KALLE_SHARD_OPTIMIZER", raising=False)
    rec = _Standins(monkeypatch)
    net = _Net()
    tr = engine.DataParallelTrainer(net, lr=1e-2, optimizer="AdamW", weight_decay=0.01, **kw)
    assert tr.flat.bucket_keys == ["a.", "b.", "c.", "_rest"]
    return rec, net, tr


def _assert_norm_calls(tr, calls, gated, accum):
    """every bucket's slot exactly once, in bucket order, over its bucket_range; ONE finish after all of them; Adam after it"""
    kinds = [c[0] for c in calls]
    n = len(tr.flat.bucket_keys)
    assert kinds == ["sumsq"] * n + ["finish"] + (["adam_ctl"] if gated else ["adam"]), kinds
    for i, key in enumerate(tr.flat.bucket_keys):
        a, b = tr.flat.bucket_range[key]
        assert calls[i][1:] == (i, tr.flat.grad[a:b].data_ptr(), b - a), (key, calls[i])
    assert calls[n][1:3] == (n, 1.0 / accum)
    assert calls[n + 1][1] == tr.flat.total and set(calls[n + 1][2]) == ADAM_KW
    assert calls[n + 1][2]["grad_scale"] == 1.0 / accum and calls[n + 1][2]["step"] == tr.step_count


@pytest.mark.parametrize("accum", [1, 3])
@pytest.mark.parametrize("mode", ["clip", "skip", "clip+skip", "track"])
def test_trainer_control_flow(monkeypatch, mode, accum):
    kw = {"clip": dict(max_grad_norm=0.05), "skip": dict(skip_nonfinite=True), "clip+skip": dict(max_grad_norm=0.05, skip_nonfinite=True),
          "track": dict(track_grad_norm=True)}[mode]
    rec, net, tr = _trainer(monkeypatch, grad_accum_steps=accum, **kw)
    gated = mode != "track"
    assert rec.take() == [("ws", 4)]
    for step in range(3):
        for i in range(accum):
            _micro(tr, net, 10 * step + i)
            calls = rec.take()
            if i < accum - 1:
                assert calls == [], calls                    # nothing on the non-boundary micro-batches of a window
        _assert_norm_calls(tr, calls, gated, accum)
        fin = calls[4]
        assert fin[3] == (0.05 if "clip" in mode else 0.0) and fin[4] == ("skip" in mode)
        c = tr.opt_ctl()
        G = tr.flat.grad.clone()
        assert c["grad_norm"] == gc.f32(gc.norm64([G], 1.0 / accum))
        assert c["clip_coef"] == gc.coef64(c["grad_norm"], kw.get("max_grad_norm")) and (c["clip_coef"] < 1) == ("clip" in mode)
        assert c["clipped_steps"] == ((step + 1) if "clip" in mode else 0) and c["skipped_steps"] == 0 and not c["nonfinite"]
    assert tr.grad_norm.data_ptr() == tr._ctl.t.data_ptr() and tr.clip_coef.item() == c["clip_coef"]
    assert tr.skipped_steps.item() == 0 and tr.clipped_steps.item() == c["clipped_steps"]


def test_trainer_skip_rule_and_state_dict(monkeypatch):
    """a non-finite gradient under skip_nonfinite: nothing moves, step_count / last_lr / the EMA schedule advance, the next step
    uses the bias corrections of the spent number; the counters travel in the state dict and may be absent from it"""
    from kalle_audio_amd import engine
    sched = lambda s: 1.0 / (1 + s)
    rec, net, tr = _trainer(monkeypatch, skip_nonfinite=True, max_grad_norm=1e9, lr_schedule=sched)
    tr.enable_ema(update_every=1, update_after_step=100)      # (copy steps only: the averaging launch needs the GPU)
    _micro(tr, net, 1)
    before = to.snapshot(tr)
    _micro(tr, net, 2, scale=math.inf)                        # a loss scaled by inf
    after = to.snapshot(tr)
    c = tr.opt_ctl()
    assert c["nonfinite"] and c["skip"] and c["skipped_steps"] == 1 and not torch.isfinite(after["grad"]).all()
    for key in ("param", "exp_avg", "exp_avg_sq", "mirror"):
        assert to._bits_equal(before[key], after[key]), key
    assert after["step_count"] == 2 and after["last_lr"] == 1e-2 * sched(1) and after["ema_sched"].step == 2
    rec.take()
    _micro(tr, net, 3)
    adam = [x for x in rec.take() if x[0] == "adam_ctl"]
    assert len(adam) == 1 and adam[0][2]["step"] == 3 and tr.step_count == 3 and not tr.opt_ctl()["skip"]
    assert (tr.flat.param != after["param"]).any()
    # direct optimizer_step() on a poisoned bucket
    tr.flat.bucket_grad("b.")[3] = -math.inf
    p = tr.flat.param.clone()
    tr.optimizer_step()
    _assert_norm_calls(tr, rec.take(), True, 1)
    assert torch.equal(tr.flat.param, p) and tr.opt_ctl()["skipped_steps"] == 2 and tr.step_count == 4
    sd = tr.state_dict()
    assert sd["skipped_steps"] == 2 and sd["clipped_steps"] == 1      # (an inf norm under max_grad_norm: coef 0 < 1 counts as clipped)
    _, net2, tr2 = _trainer(monkeypatch, skip_nonfinite=True)
    tr2.load_state_dict(sd)
    assert tr2.opt_ctl()["skipped_steps"] == 2 and tr2.step_count == 4
    del sd["skipped_steps"], sd["clipped_steps"]
    _, net3, tr3 = _trainer(monkeypatch, track_grad_norm=True)
    tr3.load_state_dict(sd)
    assert tr3.opt_ctl()["skipped_steps"] == 0
    # without skip_nonfinite the same gradient is stepped (and poisons, as under clip_grad_norm_ alone): the flag is still raised
    _, net4, tr4 = _trainer(monkeypatch, track_grad_norm=True)
    _micro(tr4, net4, 2, scale=math.inf)
    assert tr4.opt_ctl()["nonfinite"] and not tr4.opt_ctl()["skip"] and tr4.opt_ctl()["skipped_steps"] == 0


def test_default_trainer_never_touches_the_new_functions(monkeypatch):
    rec, net, tr = _trainer(monkeypatch, grad_accum_steps=2)
    for i in range(4):
        _micro(tr, net, i)
    calls = rec.take()
    assert [c[0] for c in calls] == ["adam", "adam"]
    for k, c in enumerate(calls, 1):
        assert c[1] == tr.flat.total and set(c[2]) == ADAM_KW and c[2]["step"] == k and c[2]["grad_scale"] == 0.5
    assert tr.grad_norm is None and tr.clip_coef is None and tr.skipped_steps is None and tr.clipped_steps is None
    assert tr.opt_ctl() is None
    assert set(tr.state_dict()) == {"model", "exp_avg", "exp_avg_sq", "step", "micro", "layout"}
    assert not hasattr(tr, "_norm_slot") and tr._norm_ws is None


def test_trainer_refusals(monkeypatch):
    from kalle_audio_amd import engine
    monkeypatch.delenv("KALLE_SHARD_OPTIMIZER", raising=False)
    _Standins(monkeypatch)
    for bad in (0, 0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm"):
            engine.DataParallelTrainer(_Net(), max_grad_norm=bad)
    engine.DataParallelTrainer(_Net(), max_grad_norm=math.inf)
    monkeypatch.setenv("KALLE_SHARD_OPTIMIZER", "1")
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(track_grad_norm=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            engine.DataParallelTrainer(_Net(), **kw)
    engine.DataParallelTrainer(_Net())                      # the sharded optimizer alone is still accepted
