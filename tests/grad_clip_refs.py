"""fp64 references of the gradient-norm stage (kalle_grad_sumsq / kalle_grad_norm_finish / kalle_adam_step_ctl) and of ONE clipped or
skipped optimizer step of engine.DataParallelTrainer.  Pure torch on the CPU; shared by tests/test_grad_clip_cpu.py (the references
against torch itself, the wrong references, an fp32-accumulating stand-in), tests/test_grad_clip_gpu.py (the kernels) and
tests/test_trainer_clip_gpu.py (the trainer).  Built on kernel_refs.adam_step and trainer_oracle.adam_bound.

Norm          N64 = sqrt(sum over every slot of g^2, in fp64) * f32(grad_scale).
Norm bound    |norm - N64| <= N64 (2^-24 + n_total 2^-53), derived, not measured:
                2^-24          the ONE rounding of the published norm to fp32 (half an ulp, relative);
                n_total 2^-53  the worst case of ANY order of summing n_total non-negative doubles: each of the n_total - 1 additions
                               rounds by at most 2^-53 relative to a partial sum that never exceeds the total (all terms >= 0), so
                               the sum is off by at most (n_total - 1) 2^-53 S; the squares themselves are exact (a 24-bit
                               significand squared fits 53 bits, and neither 1e20^2 nor 1e-30^2 leaves the double range); sqrt
                               halves the relative error and adds 2^-53, the product with grad_scale another 2^-53 - all inside
                               n_total 2^-53 from n_total = 3 on, and below the fp32 term's slack (a rounding to nearest is
                               2^-24 / (1 + 2^-24) relative) for n_total < 3.  The fp64 reference's own summation error is of the
                               same kind and an order below (torch sums pairwise).
Coefficient   coef64(norm, max_norm): 0 < max_norm < inf ? (float) min(1, max_norm / (norm + 1e-6)) : 1, in double from the fp32
              norm - torch.nn.utils.clip_grad_norm_'s rule (clip_coef = max_norm / (total_norm + 1e-6), clamped to 1).
Step          clip_step(): kernel_refs.adam_step with grad_scale = f32(f32(1 / (world accum)) * coef) - the single fp32 product the
              kernel forms - teacher-forced from the trainer's own state and flat gradient and the DEVICE's published coef (itself
              held to coef64 of the device's norm, itself held to N64).  A skipped step leaves every bit; the step number is spent.
Defects       NORM_WRONG (kernel level) and STEP_DEFECTS (trainer level) are seeded into the REFERENCE, never into production code."""
import math
import os
import struct
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_refs as kr  # noqa: E402
import trainer_oracle as to  # noqa: E402

F64 = torch.float64
f32 = to.f32

# include/kalle_hip.h (tests/test_grad_clip_cpu.py holds these to the header)
PARTIALS, BLOCK, UNROLL = 1024, 256, 4
SWEEP = PARTIALS * BLOCK * UNROLL * 4            # elements one grid sweep of kalle_grad_sumsq covers
NORM_N = (1, 3, 4, 255, 4097, SWEEP + 5, 2 * SWEEP + 4097)        # the last: about 8.4 M
NORM_SLOTS = (1, 3, 26)
NORM_KINDS = ("normal", "1e20", "1e-30", "mixed")
OFFSET = 64                                       # slot s reads buf[OFFSET (s + 1) : OFFSET (s + 1) + n]


def norm_values(kind, count, seed=0):
    """the shared buffer a case's slots are windows of (fp32, CPU)"""
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "normal":
        return torch.randn(count, generator=g)
    if kind == "1e20":
        return torch.full((count,), 1e20)
    if kind == "1e-30":
        return torch.full((count,), 1e-30)
    if kind == "mixed":        # magnitudes from 1e-15 to 1e15 side by side
        return torch.randn(count, generator=g) * torch.pow(10.0, torch.rand(count, generator=g) * 30 - 15)
    raise KeyError(kind)


def slot_windows(n, nslots):
    return [(OFFSET * (s + 1), OFFSET * (s + 1) + n) for s in range(nslots)]


def buffer_len(n, nslots):
    return OFFSET * (nslots + 1) + n


# ------------------------------------------------------------------------------------------------ norm and coefficient
def sumsq64(chunks):
    """[sum of g^2 in fp64] per chunk"""
    return [float(c.to(F64).pow(2).sum().item()) for c in chunks]


def norm64(chunks, grad_scale=1.0, wrong=None):
    """fp64 norm of grad_scale * (all chunks).  wrong: one of NORM_WRONG - a reference that must NOT be met."""
    if wrong == "last_slot_out":
        chunks = chunks[:-1]
    if wrong == "l1":
        return float(sum(c.to(F64).abs().sum().item() for c in chunks)) * f32(grad_scale)
    s = math.fsum(sumsq64(chunks))
    return math.sqrt(s) * (1.0 if wrong == "no_grad_scale" else f32(grad_scale))


NORM_WRONG = ("no_grad_scale", "last_slot_out", "l1")


def norm_bound(n64, n_total):
    """see the module docstring: one rounding to fp32 + the worst case of any double summation order"""
    return n64 * (2.0 ** -24 + n_total * 2.0 ** -53)


def norm_fp32_accumulating(chunks, grad_scale=1.0):
    """a stand-in that squares and accumulates in fp32, element after element (what the kernel must NOT be)"""
    import numpy as np
    s = np.float32(0.0)
    for c in chunks:
        q = c.float().pow(2).numpy().copy()
        q[0] += s
        s = np.cumsum(q, dtype=np.float32)[-1]           # (numpy's running sum stays in fp32, in element order)
    return f32(math.sqrt(float(s)) * f32(grad_scale))


def coef64(norm, max_norm, round32=True):
    """the clip coefficient from a published norm; round32=False: left in double (the comparison with torch in fp64)"""
    if not (max_norm is not None and 0 < max_norm < math.inf):
        return 1.0
    c = min(1.0, max_norm / (norm + 1e-6))
    return f32(c) if round32 else c


def ulp32(x):
    """spacing of fp32 at |x|"""
    x = abs(f32(x))
    if x == 0 or math.isinf(x) or math.isnan(x):
        return 2.0 ** -149
    i = struct.unpack("<I", struct.pack("<f", x))[0]
    return struct.unpack("<f", struct.pack("<I", i + 1))[0] - x


def f32_product(a, b):
    """the ONE fp32 product f32(a) * f32(b), as the Adam kernel forms grad_scale * coef"""
    return float((torch.tensor(a, dtype=torch.float32) * torch.tensor(b, dtype=torch.float32)).item())


# ------------------------------------------------------------------------------------------------ one clipped / skipped step
STEP_DEFECTS = (
    "clip_per_bucket",        # every bucket clipped to max_norm by its OWN norm
    "norm_of_sum",            # the coefficient from the norm of the window's SUM instead of its average
    "coef_on_m_only",         # exp_avg fed the clipped gradient, exp_avg_sq the unclipped one
    "rest_on_skip",           # `_rest` stepped on a skipped step
    "torch_step_after_skip",  # bias corrections of torch's un-advanced state['step'] (k minus the skips so far)
)


def clip_step(state, G, cfg, k, coef=1.0, skip=False, defect=None, ranges=None, max_norm=None, skipped_before=0):
    """state: dict(param, exp_avg, exp_avg_sq) before the step; G: the flat gradient (the window's SUM); k: this optimizer
    step's number (skipped ones count: the number is spent); coef, skip: what the device published; ranges: bucket -> (a, b).
    Returns dict(p, m, v (fp64), dm, dv, tol_p, lr) - on a skipped step the inputs themselves with zero tolerances."""
    lr = to.lr_of(cfg, k)
    hp = dict(lr=f32(lr), beta1=f32(cfg["betas"][0]), beta2=f32(cfg["betas"][1]), eps=f32(cfg["eps"]),
              weight_decay=f32(cfg["weight_decay"]))
    gs = f32(1.0 / (cfg["world"] * cfg["accum"]))
    step = k - skipped_before if defect == "torch_step_after_skip" else k
    p0, m0, v0, g = (t.to(F64) for t in (state["param"], state["exp_avg"], state["exp_avg_sq"], G))
    zero = torch.zeros_like(p0)
    if skip:
        out = dict(p=p0.clone(), m=m0.clone(), v=v0.clone(), dm=zero.clone(), dv=zero.clone(), tol_p=zero.clone(), lr=lr)
        if defect == "rest_on_skip":
            a, b = ranges["_rest"]
            gfin = torch.nan_to_num(g[a:b], nan=1.0, posinf=1.0, neginf=-1.0)        # (whatever it stepped with: it MOVED)
            kw = dict(decoupled=cfg["decoupled"], step=step, grad_scale=gs, **hp)
            out["p"][a:b], out["m"][a:b], out["v"][a:b] = kr.adam_step(p0[a:b], gfin, m0[a:b], v0[a:b], **kw)
        return out
    gse = f32_product(gs, coef)
    if defect == "norm_of_sum":
        gse = f32_product(gs, coef64(f32(norm64([G], 1.0)), max_norm))
    if defect == "clip_per_bucket":
        gse = torch.empty_like(g)
        for a, b in ranges.values():
            gse[a:b] = f32_product(gs, coef64(f32(norm64([G[a:b]], gs)), max_norm))
    kw = dict(decoupled=cfg["decoupled"], step=step, **hp)
    pr, mr, vr = kr.adam_step(p0, g, m0, v0, grad_scale=gse, **kw)
    if defect == "coef_on_m_only":
        _, _, vr = kr.adam_step(p0, g, m0, v0, grad_scale=gs, **kw)
        pd = p0 * (1 - hp["lr"] * hp["weight_decay"]) if cfg["decoupled"] else p0
        bc1, bc2 = 1 - hp["beta1"] ** step, math.sqrt(1 - hp["beta2"] ** step)
        pr = pd - (hp["lr"] / bc1) * (mr / (vr.sqrt() / bc2 + hp["eps"]))
    dm, dv, tol = to.adam_bound(p0, g, m0, v0, pr, mr, vr, hp, step, gse, cfg["decoupled"])
    return dict(p=pr, m=mr, v=vr, dm=dm, dv=dv, tol_p=tol, lr=lr)


def check_clip_step(before, after, G, cfg, k, ranges, gaps=None, **kw):
    """as trainer_oracle.check_step: {(quantity, bucket): worst deviation / bound}, bit-for-bit checks 0 or inf; <= 1 passes.
    kw: coef, skip, defect, max_norm, skipped_before of clip_step."""
    exp = clip_step(before, G, cfg, k, ranges=ranges, **kw)
    out = {}
    for q, key, tol in (("p", "param", exp["tol_p"]), ("m", "exp_avg", exp["dm"]), ("v", "exp_avg_sq", exp["dv"])):
        r = to._ratio(after[key], exp[q], tol)
        for name, (a, b) in ranges.items():
            out[(q, name)] = r[a:b].max().item()
        if gaps is not None:
            out[("gap", q)] = 0.0 if not (after[key][gaps] != 0).any() else to.INF
    if after.get("mirror") is not None:
        out[("mirror", "all")] = 0.0 if to._bits_equal(after["mirror"], after["param"].bfloat16()) else to.INF
    if after.get("last_lr") is not None:
        out[("lr", "all")] = 0.0 if after["last_lr"] == exp["lr"] else to.INF
    if after.get("step_count") is not None:
        out[("step_count", "all")] = 0.0 if after["step_count"] == k else to.INF
    return out
