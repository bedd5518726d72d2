"""Teacher-forced fp64 reference of ONE optimizer step of engine.DataParallelTrainer / engine.FusedAdam, element by element.
Pure torch on the CPU; shared by tests/test_trainer_oracle_cpu.py (an fp32 stand-in of the device and the seeded defects on the
reference itself) and tests/test_trainer_oracle_gpu.py (the HIP path).

Teacher forcing   the reference consumes the trainer's OWN flat param / exp_avg / exp_avg_sq from before the step and the flat
                  gradient the trainer holds after the window's last backward (the window's SUM; 1 / (world accum) travels as
                  grad_scale).  A gradient from fp64 would not do: Adam's first updates are lr sign(g), and every element whose
                  sign a bf16-operand gradient flips would be off by 2 lr.  The gradient itself is held by tests/grad_slices.py.
Reference         kernel_refs.adam_step in fp64 with the hyper-parameters rounded to fp32, as the C ABI receives them:
                  grad_scale = 1 / (world accum), step = k, lr = cfg.lr * schedule(k - 1), decay decoupled or coupled as configured.
Bounds            p, m, v: adam_bound() - the formula of run_adam (tests/test_norm_elementwise_gpu.py), U and ALLOW["DIV"] imported.
                  EMA: 3 u (|a ema0| + |b p|), a = f32(d), b = f32(1 - d) - the bound of test_axpby.
                  Bit for bit: the bf16 mirror (== bf16(param)), EMA copy and skip steps, last_lr, step_count, the alignment gaps
                  between parameters (exactly 0 in p, m, v).
Defects           DEFECTS are seeded into the REFERENCE, never into production code: the device's (or the stand-in's) recorded
                  states are then checked against the wrong reference and must fall out of bound."""
import copy
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_refs as kr  # noqa: E402
from test_norm_elementwise_gpu import ALLOW, U  # noqa: E402

F64 = torch.float64
INF = math.inf

DEFECTS = (
    "step_plus",          # bias correction with step k + 1
    "step_minus",         # ... with step k - 1 (from the second step on: the kernel refuses step 0)
    "sched_at_k",         # lr = cfg.lr * schedule(k) instead of schedule(k - 1)
    "no_accum_scale",     # grad_scale = 1 / world: the 1 / accum is lost
    "decay_after",        # AdamW's decay applied to the updated weights
    "decay_swapped",      # coupled <-> decoupled
    "bucket_twice",       # one named bucket stepped by its hook AND by the final pass
    "bucket_skipped",     # one named bucket not stepped
    "mirror_before",      # the bf16 mirror cast from the weights before the step
    "ema_before",         # the EMA fed the weights before the step
    "ema_epoch_early",    # the EMA decay of the previous epoch
    "moments_lost",       # the moments of one named bucket zero (not restored on resume)
)
BUCKET_DEFECTS = ("bucket_twice", "bucket_skipped", "moments_lost")


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


def make_cfg(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, accum=1, world=1, schedule=None):
    return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled, accum=accum, world=world,
                schedule=schedule)


def cfg_of(tr):
    """the configuration a DataParallelTrainer was built with"""
    return make_cfg(tr.lr, tr.betas, tr.eps, tr.weight_decay, tr.decoupled, tr.grad_accum_steps, tr.world, tr.lr_schedule)


# ------------------------------------------------------------------------------------------------ the kernel's bound
def adam_bound(p0, g, m0, v0, pr, mr, vr, hp, step, grad_scale, decoupled):
    """(dm, dv, tol_p): the bound of run_adam / _assert_adam_step, term for term.  p0, g, m0, v0: fp64 inputs (g unscaled);
    pr, mr, vr: the fp64 reference's outputs; hp: lr, beta1, beta2, eps, weight_decay as the float ABI passes them."""
    b1, b2, lr, wd = hp["beta1"], hp["beta2"], hp["lr"], hp["weight_decay"]
    gq = g.abs() * grad_scale + (0 if decoupled else wd * p0.abs())
    dm = 4 * U * (m0.abs() + gq)
    dv = 6 * U * (v0.abs() + gq * gq)
    bc1, bc2 = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    denom = vr.sqrt() / bc2 + hp["eps"]
    upd = (lr / bc1) * mr.abs() / denom
    R = 8 + ALLOW["DIV"] + 2 * b1 ** step / bc1 + b2 ** step / bc2 ** 2
    tol = 3 * U * p0.abs() + R * U * upd + (lr / bc1) * (dm / denom + mr.abs() / denom.pow(2) * dv / (2 * vr.sqrt() * bc2 + 1e-300))
    return dm, dv, tol


# ------------------------------------------------------------------------------------------------ one optimizer step
def lr_of(cfg, k, at_k=False):
    """exactly engine._begin_optimizer_step's expression (a Python double: tr.last_lr must EQUAL it)"""
    s = k if at_k else k - 1
    return cfg["lr"] * (cfg["schedule"](s) if cfg["schedule"] else 1.0)


def expected_step(state, G, cfg, k, defect=None, rng=None):
    """state: dict(param, exp_avg, exp_avg_sq) before the step; G: the flat gradient after the window's last backward; k: the
    number of this optimizer step (1, 2, ...); rng: (a, b) of the named bucket of a BUCKET_DEFECTS entry.
    Returns dict(p, m, v (fp64), dm, dv, tol_p, lr (exact), mirror_from ("after" | "before": which weights the bf16 mirror is
    the rounding of - a rule, since bf16 of an fp64 reference says nothing about a value on a rounding boundary))."""
    lr = lr_of(cfg, k, at_k=defect == "sched_at_k")
    hp = dict(lr=f32(lr), beta1=f32(cfg["betas"][0]), beta2=f32(cfg["betas"][1]), eps=f32(cfg["eps"]),
              weight_decay=f32(cfg["weight_decay"]))
    step = k + 1 if defect == "step_plus" else (k - 1 if defect == "step_minus" and k > 1 else k)
    gs = f32(1.0 / (cfg["world"] * (1 if defect == "no_accum_scale" else cfg["accum"])))
    decoupled = cfg["decoupled"] != (defect == "decay_swapped")
    p0, m0, v0, g = (t.to(F64) for t in (state["param"], state["exp_avg"], state["exp_avg_sq"], G))
    if defect == "moments_lost":
        m0, v0 = m0.clone(), v0.clone()
        m0[rng[0]:rng[1]] = 0
        v0[rng[0]:rng[1]] = 0
    kw = dict(decoupled=decoupled, step=step, grad_scale=gs, decay_after=defect == "decay_after", **hp)
    pr, mr, vr = kr.adam_step(p0, g, m0, v0, **kw)
    dm, dv, tol = adam_bound(p0, g, m0, v0, pr, mr, vr, hp, step, gs, decoupled)
    if defect == "bucket_twice":
        a, b = rng
        pr[a:b], mr[a:b], vr[a:b] = kr.adam_step(pr[a:b].clone(), g[a:b], mr[a:b].clone(), vr[a:b].clone(), **kw)
    if defect == "bucket_skipped":
        a, b = rng
        pr[a:b], mr[a:b], vr[a:b] = p0[a:b], m0[a:b], v0[a:b]
    return dict(p=pr, m=mr, v=vr, dm=dm, dv=dv, tol_p=tol, lr=lr, mirror_from="before" if defect == "mirror_before" else "after")


def expected_ema(ema0, p_after, sched_state, early=False):
    """follows EMASchedule.next() on a COPY of the schedule as it stood before the step.  Returns (kind, ref, tol):
    ("skip", ema0, None) bit-unchanged; ("copy", p_after, None) bit-equal; ("avg", a ema0 + b p_after in fp64, 3 u (|a ema0| + |b p|))
    with a = f32(d), b = f32(1 - d) as ops.axpby passes them.  early (a DEFECT): the decay of the previous epoch."""
    sc = copy.copy(sched_state)
    d = sc.next()
    if d is None:
        return "skip", ema0, None
    if d == "copy":
        return "copy", p_after, None
    if early:
        epoch = max(sc.step - sc.update_after_step - 1, 0) - 1
        d = 0.0 if epoch <= 0 else min(max(1 - (1 + epoch / sc.inv_gamma) ** -sc.power, sc.min_value), sc.beta)
    a, b = f32(d), f32(1.0 - d)
    e, p = ema0.to(F64), p_after.to(F64)
    return "avg", a * e + b * p, 3 * U * (abs(a) * e.abs() + abs(b) * p.abs())


def _bits_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def _ratio(out, ref, tol):
    return torch.nan_to_num((out.to(F64) - ref).abs() / (tol + 1e-38), nan=INF)


def check_step(before, after, G, cfg, k, ranges, gaps=None, defect=None, bucket=None):
    """before / after: snapshots (CPU) with param, exp_avg, exp_avg_sq and optionally mirror, ema (+ ema_sched in `before`),
    last_lr, step_count; ranges: bucket key -> (a, b); gaps: bool mask of the elements that belong to no parameter.
    Returns {(quantity, bucket): worst deviation / bound}; bit-for-bit checks give 0 or inf.  A pass is every value <= 1."""
    exp = expected_step(before, G, cfg, k, defect, ranges[bucket] if defect in BUCKET_DEFECTS else None)
    out = {}
    for q, key, tol in (("p", "param", exp["tol_p"]), ("m", "exp_avg", exp["dm"]), ("v", "exp_avg_sq", exp["dv"])):
        r = _ratio(after[key], exp[q], tol)
        for name, (a, b) in ranges.items():
            out[(q, name)] = r[a:b].max().item()
        if gaps is not None:
            out[("gap", q)] = 0.0 if not (after[key][gaps] != 0).any() else INF
    if after.get("mirror") is not None:
        src = after["param"] if exp["mirror_from"] == "after" else before["param"]
        out[("mirror", "all")] = 0.0 if _bits_equal(after["mirror"], src.bfloat16()) else INF
    if after.get("last_lr") is not None:
        out[("lr", "all")] = 0.0 if after["last_lr"] == exp["lr"] else INF
    if after.get("step_count") is not None:
        out[("step_count", "all")] = 0.0 if after["step_count"] == k else INF
    if before.get("ema") is not None:
        src = before["param"] if defect == "ema_before" else after["param"]
        kind, ref, tol = expected_ema(before["ema"], src, before["ema_sched"], early=defect == "ema_epoch_early")
        if kind == "avg":
            r = _ratio(after["ema"], ref, tol)
            for name, (a, b) in ranges.items():
                out[("ema", name)] = r[a:b].max().item()
        else:
            out[("ema", kind)] = 0.0 if _bits_equal(after["ema"], ref) else INF
        if gaps is not None:
            out[("gap", "ema")] = 0.0 if not (after["ema"][gaps] != 0).any() else INF
    return out


def failures(ratios):
    return sorted((k for k, v in ratios.items() if not v <= 1.0), key=str)


def worst(ratios):
    """quantity -> worst ratio over the buckets"""
    out = {}
    for (q, _), v in ratios.items():
        out[q] = max(out.get(q, 0.0), v)
    return out


def evaluate(records, cfg, ranges, gaps=None, defect=None, bucket=None, stop=None):
    """check_step over a run's records [dict(before, after, G, k)]: quantity -> worst ratio over the steps and buckets.
    stop(out): end the run early (a defect that has shown needs no further steps)"""
    out = {}
    for r in records:
        for q, v in worst(check_step(r["before"], r["after"], r["G"], cfg, r["k"], ranges, gaps, defect, bucket)).items():
            out[q] = max(out.get(q, 0.0), v)
        if stop is not None and stop(out):
            break
    return out


def caught(w):
    return any(not v <= 1.0 for v in w.values())


def shown(defect):
    """stop rule of evaluate() for a seeded defect: it is out of bound (the lost 1 / accum in BOTH moments)"""
    if defect == "no_accum_scale":
        return lambda w: w.get("m", 0) > 1 and w.get("v", 0) > 1
    return caught


# ------------------------------------------------------------------------------------------------ snapshots of a trainer
def gap_mask(flat):
    m = torch.ones(flat.total, dtype=torch.bool)
    for s, ne in flat.slices.values():
        m[s:s + ne] = False
    return m


def snapshot(tr):
    """everything check_step reads, as CPU copies (call after a device synchronise)"""
    c = lambda t: t.detach().cpu().clone()
    s = dict(param=c(tr.flat.param), exp_avg=c(tr.exp_avg), exp_avg_sq=c(tr.exp_avg_sq), mirror=c(tr.flat.param_bf16),
             grad=c(tr.flat.grad), last_lr=tr.last_lr, step_count=tr.step_count, micro=tr.micro)
    if getattr(tr, "ema", None) is not None:
        s["ema"] = c(tr.ema)
        s["ema_sched"] = copy.copy(tr.ema_schedule)
    return s


# ------------------------------------------------------------------------------------------------ configurations
def _cos(s):
    from kalle_audio_amd.engine import cosine_with_warmup
    return cosine_with_warmup(s, 2, 8)          # every step of a short run has a distinct lr (0 at the first)


EMA_KW = dict(beta=0.9999, power=3 / 4, update_after_step=1)
# name -> (trainer keywords, EMA update_every or None, optimizer steps).  T1 / T3 / T4 are the issue's; "plain" is the
# configuration of a direct optimizer_step() (T6): constant lr, no decay - the one that confirms the blind pairs below.
CONFIGS = {
    "T1": (dict(lr=1e-2, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2, lr_schedule=_cos), None, 4),
    "T3": (dict(lr=1e-3, optimizer="Adam", weight_decay=0.1, grad_accum_steps=1, lr_schedule=_cos), None, 4),
    "T4-every1": (dict(lr=1e-2, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2, lr_schedule=_cos), 1, 5),
    "T4-every2": (dict(lr=1e-2, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2, lr_schedule=_cos), 2, 5),
    "plain": (dict(lr=1e-3, optimizer="Adam", weight_decay=0.0, grad_accum_steps=1, lr_schedule=None), 1, 5),
}
# (configuration, defect) pairs that CANNOT show, each with its reason; tests/test_trainer_oracle_cpu.py asserts every one blind
# (so the list cannot rot) and every other pair caught, and holds the table to one fifth of all pairs.
BLIND = {
    ("T1", "ema_before"): "no EMA enabled",
    ("T1", "ema_epoch_early"): "no EMA enabled",
    ("T3", "ema_before"): "no EMA enabled",
    ("T3", "ema_epoch_early"): "no EMA enabled",
    ("T3", "no_accum_scale"): "accum = 1: 1 / (world accum) = 1 / world",
    ("T3", "decay_after"): "coupled L2 has no separate decay factor to misplace",
    ("plain", "sched_at_k"): "constant schedule",
    ("plain", "decay_swapped"): "weight_decay = 0",
    ("plain", "decay_after"): "weight_decay = 0",
    ("plain", "no_accum_scale"): "accum = 1",
}


def cfg_from_kw(kw):
    return make_cfg(lr=kw["lr"], weight_decay=kw["weight_decay"], decoupled=kw["optimizer"].lower() in ("adamw", "fusedadam"),
                    accum=kw["grad_accum_steps"], schedule=kw["lr_schedule"])


# ------------------------------------------------------------------------------------------------ fp32 stand-in of the device
def standin_step(state, G, cfg, k):
    """the same formulas in fp32 torch, in the written order (what a device that is right computes, up to its own roundings)"""
    lr = lr_of(cfg, k)
    b1, b2 = cfg["betas"]
    wd, eps = cfg["weight_decay"], cfg["eps"]
    p, m, v = state["param"].clone(), state["exp_avg"].clone(), state["exp_avg_sq"].clone()
    g = G * f32(1.0 / (cfg["world"] * cfg["accum"]))
    if cfg["decoupled"]:
        p = p * f32(1 - f32(lr) * f32(wd))
    else:
        g = g + f32(wd) * p
    m = f32(b1) * m + f32(1 - f32(b1)) * g
    v = f32(b2) * v + f32(1 - f32(b2)) * (g * g)
    bc1, bc2 = 1 - f32(b1) ** k, math.sqrt(1 - f32(b2) ** k)
    p = p - f32(f32(lr) / bc1) * (m / (v.sqrt() / f32(bc2) + f32(eps)))
    return p, m, v


def standin_run(state, grads, cfg, ema_every=None):
    """records of a run of len(grads) optimizer steps of the stand-in from `state` (fp32 param / exp_avg / exp_avg_sq)"""
    from kalle_audio_amd.engine import EMASchedule
    st = dict(state, mirror=state["param"].bfloat16(), last_lr=cfg["lr"], step_count=0)
    if ema_every is not None:
        st["ema"], st["ema_sched"] = state["param"].clone(), EMASchedule(update_every=ema_every, **EMA_KW)
    recs = []
    for k, G in enumerate(grads, 1):
        p, m, v = standin_step(st, G, cfg, k)
        new = dict(param=p, exp_avg=m, exp_avg_sq=v, mirror=p.bfloat16(), last_lr=lr_of(cfg, k), step_count=k)
        if ema_every is not None:
            sc = copy.copy(st["ema_sched"])
            d = sc.next()
            new["ema_sched"] = sc
            new["ema"] = st["ema"].clone() if d is None else (p.clone() if d == "copy" else f32(d) * st["ema"] + f32(1.0 - d) * p)
        recs.append(dict(before=st, after=new, G=G, k=k))
        st = new
    return recs
