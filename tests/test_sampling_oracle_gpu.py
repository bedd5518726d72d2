"""-m gpu: guided DiT sampling on the HIP path held to the fp64 oracle of tests/sample_oracle.py, step by step.  The real
generate_diffusion_cond (graph replay, conditioning hoisted out of the loop, or neither, as the case says - asserted), sample_rf with a
variation start point, and single guided forwards (CFG rescale, a prepended conditioning) run once; every denoiser call is recorded
through a proxy of the sampler's `model` argument; after one synchronize everything else is CPU work: every token row of every step
within M = 3 times a yardstick that comes from the reference alone, the schedule bit for bit, every sampler update and the returned
tensor inside the rounding of their fp32 operations, and each seeded defect, put into the reference at the recorded inputs, reported.

Measured on an MI355X: DESIGN.md, "Sampling per step"."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_oracle as so  # noqa: E402
from test_grad_slices_gpu import _wrapped  # noqa: E402
from test_modules_gpu import load_seeded  # noqa: E402

gs = so.gs
_ID = lambda k: k["id"]


@functools.lru_cache(maxsize=None)
def ref(case_id):
    """state, inputs, fp64 free run and yardstick of the case (computed once, read-only afterwards)"""
    return so.reference(so.BY_ID[case_id])


class Recorder:
    """records every denoiser call of a sampler: x, t and the returned tensor are cloned IMMEDIATELY - the graph replay returns a
    static buffer that the next step overwrites (kalle_audio_amd/graph.py, GraphedForward.__call__)"""

    def __init__(self):
        self.calls, self.denoiser, self.samplers = [], None, []

    def proxy(self, model):
        self.denoiser = model

        def call(x, t, **kw):
            xr, tr = x.detach().clone(), t.detach().clone()
            out = model(x, t, **kw)
            self.calls.append(dict(x=xr, t=tr, out=out.detach().clone(), kw=frozenset(kw)))
            return out
        return call

    def sampler(self, real):
        def run(model, *a, **kw):
            self.samplers.append(real.__name__)
            return real(self.proxy(model), *a, **kw)
        return run


def _to(inp, dev):
    return {n: v.to(dev) if torch.is_tensor(v) else v for n, v in inp.items()}


def _check(k, R, calls, returned):
    """everything after the synchronize, on the CPU.  calls: [dict(x [B, C, T], t [B], out [B, C, T'])]; returned: what the
    sampler gave back (None: a single forward)"""
    W, inp, r = R["W"], R["inp"], R["r"]
    B, steps = k["B"], max(k["steps"], 1)
    assert len(calls) == steps
    xs = [c["x"].float().cpu() for c in calls]
    outs = [c["out"].float().cpu() for c in calls]
    assert all(c["x"].dtype == torch.float32 and c["out"].dtype == torch.float32 for c in calls)
    # schedule: the fp32 values of the sampler's own linspace, the same for every clip
    sched = so.schedule(k)[:-1] if k["steps"] else R["traj"]["ts"]
    for i, c in enumerate(calls):
        assert c["t"].dtype == torch.float32 and torch.equal(c["t"].cpu(), torch.full((B,), float(sched[i]))), (i, c["t"], sched[i])
    ts = [c["t"][0].cpu() for c in calls]
    # per step and token row against the fp64 output ON THE RECORDED INPUTS
    rows = [gs.rows_bct(o) for o in outs]
    out64 = so.outputs(k, W, inp, xs, ts)
    v, step, row, q = so.worst(rows, out64, r)
    print(f"SAMPLING {k['id']}: worst ratio / (M r) {v:.3f} at step {step} row {row} (ratio {q:.3e}, r {r[step]:.3e}); per step "
          + " ".join(f"{so.worst([a], [b], [c])[0]:.3f}" for a, b, c in zip(rows, out64, r)))
    assert so.failure(rows, out64, r, k["id"]) is None, so.failure(rows, out64, r, k["id"])
    if k["steps"]:
        # start point, updates, returned tensor: element-wise inside the allowances sample_oracle derives for the fp32 formulas
        x0, tol0 = so.start(k, inp)
        assert so.over(xs[0], x0, tol0) <= 0, ("start", so.over(xs[0], x0, tol0))
        if not k["init"]:
            assert torch.equal(xs[0], inp["noise"])
        ret = returned.float().cpu()
        assert returned.dtype == torch.float32 and ret.shape == xs[0].shape
        for i in range(steps):
            u = so.update(k, i, xs[i], outs[i])
            if i < steps - 1:
                assert so.over(xs[i + 1], u["next"], u["next_tol"]) <= 0, ("update", i, so.over(xs[i + 1], u["next"], u["next_tol"]))
            else:
                assert so.over(ret, u["ret"], u["ret_tol"]) <= 0, ("returned", so.over(ret, u["ret"], u["ret_tol"]))
        # the free-running fp64 latents: printed and recorded, not asserted - the per-step check and the update check imply the
        # deviation, and no bound for it can be derived in advance
        fin = gs.rows_bct(R["traj"]["final"])
        print(f"SAMPLING {k['id']}: final latents against the free-running fp64 latents: rel l2 {gs.rel_l2(gs.rows_bct(ret), fin):.3e}, "
              f"worst row ratio {so.ratios(gs.rows_bct(ret), fin).max().item():.3e}")
    # a wrong reference is caught: each defect the state can show, seeded into the reference at the recorded inputs
    caught, weakest = 0, (float("inf"), None)
    for d in so.defects_of(k, so.MODEL_DEFECTS):
        if (k["id"], d) in so.BLIND:
            continue
        bad = so.outputs(k, W, inp, xs, ts, "f64", d)
        assert so.failure(rows, bad, r, d) is not None, (k["id"], d, so.worst(rows, bad, r))
        weakest = min(weakest, (so.worst(rows, bad, r)[0], d))
        caught += 1
    print(f"SAMPLING {k['id']}: {caught} seeded defects reported, the weakest ({weakest[1]}) at {weakest[0]:.3f} M r")
    for d in so.defects_of(k, so.UPDATE_DEFECTS):
        for i in range(steps - 1):
            bad = so.update(k, i, xs[i], outs[i], d)
            assert so.over(xs[i + 1], bad["next"], bad["next_tol"]) > 0, (d, i)
        caught += 1
    assert caught >= 2, caught
    return caught


def _cond(k, inp, dev):
    B, S = k["B"], so.base(k)["S"]
    ones = torch.ones(B, S, dtype=torch.bool, device=dev)
    cond = {"prompt": (inp["ctx"], ones), "g": (inp["gl"], None)}
    neg = {"prompt": (inp["neg"], inp["negm"]), "g": (inp["gl"], None)} if k["neg"] else None
    return cond, neg


def _model(k, dev):
    model = _wrapped(so.base(k), dev)
    model.diffusion_objective = k["obj"]
    assert {n: tuple(p.shape) for n, p in model.model.model.named_parameters()} == dict(so.shapes(k))
    model.requires_grad_(k["trainable"])
    return model


@pytest.mark.parametrize("k", [k for k in so.CASES if not k["init"]], ids=_ID)
def test_generate_diffusion_cond_per_step(dev, monkeypatch, k):
    from kalle_audio_amd.stable_audio_tools.inference import generation
    R = ref(k["id"])
    inp = _to(R["inp"], dev)
    model = _model(k, dev)
    rec = Recorder()
    for name in ("sample", "sample_discrete_euler", "sample_rf"):
        monkeypatch.setattr(generation, name, rec.sampler(getattr(generation, name)))
    cond, neg = _cond(k, inp, dev)
    lat = generation.generate_diffusion_cond(model, steps=k["steps"], cfg_scale=k["cfg"], conditioning_tensors=cond,
                                             negative_conditioning_tensors=neg, batch_size=k["B"], sample_size=so.base(k)["T"],
                                             seed=k["base"], device="cpu", return_latents=True)
    torch.cuda.synchronize()
    # the intended path has run
    assert rec.samplers == ["sample" if k["obj"] == "v" else "sample_discrete_euler"]
    graph, hoisted = k["path"]
    g = getattr(model, "_kalle_graphed", None)
    if graph:
        assert g is not None and rec.denoiser is g and len(g._cache) == 1
        assert not any(p.requires_grad for p in model.parameters())
    else:
        assert g is None and rec.denoiser is model.model
        assert all(p.requires_grad for p in model.parameters())
    for c in rec.calls:
        assert ("kalle_ctx_kv" in c["kw"]) == hoisted and ("kalle_ctx_embed" in c["kw"]) == hoisted, sorted(c["kw"])
    _check(k, R, rec.calls, lat)


def test_sample_rf_variation_per_step(dev):
    """G7: sample_rf called directly with init_data and sigma_max = 0.6 - the variation start point and the shortened schedule"""
    from kalle_audio_amd.stable_audio_tools.inference import sampling
    k = so.BY_ID["G7"]
    R = ref(k["id"])
    inp = _to(R["inp"], dev)
    model = _model(k, dev)
    rec = Recorder()
    ones = torch.ones(k["B"], so.base(k)["S"], dtype=torch.bool, device=dev)
    lat = sampling.sample_rf(rec.proxy(model.model), inp["noise"], init_data=inp["init"], steps=k["steps"], sigma_max=k["sigma_max"],
                             cross_attn_cond=inp["ctx"], cross_attn_mask=ones, global_cond=inp["gl"], cfg_scale=k["cfg"],
                             batch_cfg=True, rescale_cfg=True)
    torch.cuda.synchronize()
    _check(k, R, rec.calls, lat)


@pytest.mark.parametrize("k", so.SINGLE, ids=_ID)
def test_guided_forward_single_call(dev, k):
    """S1 / S2: the rescale branch of _guided (cfg_scale 3, scale_phi 0.5); S3 / S4: prepend_cond with its mask through SpliceFn and
    _with_unconditional(prepend_cond), on a prepend and an adaLN model"""
    from kalle_audio_amd.stable_audio_tools.models.dit import DiffusionTransformer
    R = ref(k["id"])
    inp = _to(R["inp"], dev)
    dit = load_seeded(DiffusionTransformer(**so.module_kwargs(k)), k["base"], dev)
    assert {n: tuple(p.shape) for n, p in dit.named_parameters()} == dict(so.shapes(k))
    x = inp["x"]
    t = torch.full((k["B"],), float(R["traj"]["ts"][0]), device=dev)
    with torch.no_grad():
        out = dit(x, t, cross_attn_cond=inp["ctx"], global_embed=inp["gl"], prepend_cond=inp["prepend"],
                  prepend_cond_mask=inp["prepend_mask"], cfg_scale=k["cfg"], scale_phi=k["phi"])
    torch.cuda.synchronize()
    assert out.shape == (k["B"], gs.CIO, so.tokens(k))
    _check(k, R, [dict(x=x, t=t, out=out)], None)
