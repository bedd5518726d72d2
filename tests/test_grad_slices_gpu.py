"""-m gpu: the COMPOSED backward (functional.py, dit_ops.py, llama_ops.py, the trainer's clear / overwrite rules in engine.py) held
slice by slice to the fp64 oracle - tests/grad_slices.py: every parameter gradient in runs of 16 rows cut at the chunk boundaries of
fused parameters, the output and every input gradient per token row, each slice within M = 3 times a yardstick that comes from the
reference alone.  Four families: the DiT through plain autograd, through the trainer's flat buckets (accumulation windows, grouped /
single weight-gradient launches, two consecutive windows), partially frozen models (sinks and fresh tensors mixed inside a block), and
Llasa.  Every test ends by seeding the defects of grad_slices.seeded_defects into the reference and asserting that the check
reports each of them (CPU post-processing).

Measured on an MI355X (worst rho = |g - g64|_slice / (r(p) scale) per family): see DESIGN.md, "Gradients per slice"."""
import functools
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_slices as gs  # noqa: E402
import kernel_refs as kr  # noqa: E402
from test_modules_gpu import _Tok, _hf_grads, load_seeded  # noqa: E402

gu = gs.gu
_ID = lambda c: c["id"]
_BY_ID = {c["id"]: c for c in gs.DIT_CASES + [t["base"] for t in gs.TRAINER_CASES] + [f["base"] for f in gs.FROZEN_CASES]}


@functools.lru_cache(maxsize=None)
def dit_ref(case_id, seeds):
    """fp64 reference of the case's window, its slices and its yardstick (computed once per case, read-only afterwards)"""
    c = _BY_ID[case_id]
    st = gu.make_state(gs.dit_shapes(c), c["seed"])
    sites = gs.dit_defect_sites(c)
    g64 = gs.dit_window(c, st, seeds, bias_rows=sites["bias"] if len(seeds) == 1 else None)
    layout = gs.dit_layout(c, g64)
    r, _ = gs.yardstick(gs.dit_window(c, st, seeds, "emu"), g64, layout)
    return dict(st=st, g64=g64, layout=layout, r=r, sites=sites)


def assert_slices(g, ref, names, what):
    rho = gs.check(g, ref["g64"], ref["r"], ref["layout"], names)
    n, v, rows = gs.worst(rho)
    print(f"SLICES {what}: worst rho {v:.2f} at {n} rows {rows} (r(p) {ref['r'][n]:.2e}); {len(rho)} tensors")
    kb = [v for k, (v, _) in rho.items() if k.endswith("k_norm.bias")]      # (the slices the attention roundings were added for)
    if kb:
        print(f"SLICES {what}: k_norm.bias worst rho {max(kb):.2f}")
    assert not gs.failures(rho), (what, gs.failures(rho))
    return rho


def assert_defects_caught(ref):
    """sensitivity: each seeded defect, put into the fp64 reference itself, is reported"""
    sites = ref["sites"]
    defects = gs.seeded_defects(ref["g64"], ref["layout"], sites, ref["g64"].get("rows:" + sites["bias"]))
    for label, n, gd in defects:
        rho = gs.check(gd, ref["g64"], ref["r"], ref["layout"], [n])
        assert gs.failures(rho), (label, n, rho[n])
        if label.startswith("tail slice"):
            assert gs.old_rule_passes(gd, ref["g64"], n), n
    return [n for _, n, _ in defects]


# ------------------------------------------------------------------------------------------------ DiT, plain autograd
def _dit_module(c, dev):
    from kalle_audio_amd.stable_audio_tools.models.dit import DiffusionTransformer
    dit = load_seeded(DiffusionTransformer(**gs.dit_module_kwargs(c)), c["seed"], dev)
    assert {n: tuple(p.shape) for n, p in dit.named_parameters()} == dict(gs.dit_shapes(c))     # the oracle's inventory
    return dit


def _dit_step(dit, c, dev, inputs_grad=True):
    """one train step through plain autograd: diffuse_fwd -> DiT -> MSELossFn.  Returns the gradients under the reference's names"""
    from kalle_audio_amd import functional as KF, ops
    inp = {k: None if v is None else v.to(dev) for k, v in gs.dit_inputs(c).items()}
    xt, tgt = ops.diffuse_fwd(inp["lat"], inp["noise"], inp["t"], c["obj"])
    xt.requires_grad_(True)
    ctx, gl = inp["ctx"].requires_grad_(inputs_grad), inp["gl"].requires_grad_(inputs_grad)
    out = dit(xt, inp["t"], cross_attn_cond=ctx, cross_attn_cond_mask=inp["cm"], global_embed=gl, cfg_dropout_prob=0.0)
    loss = KF.MSELossFn.apply(out, tgt, inp["pm"], 1.0)
    loss.backward()
    torch.cuda.synchronize()
    g = {n: p.grad.float().cpu() for n, p in dit.named_parameters() if p.grad is not None}
    g.update({"act:out": gs.rows_bct(out.detach().float().cpu()), "act:d_xt": gs.rows_bct(xt.grad.float().cpu())})
    if inputs_grad:
        g.update({"act:d_ctx": ctx.grad.float().cpu().flatten(0, 1), "act:d_glob": gl.grad.float().cpu()})
    return g, loss.item()


@pytest.mark.parametrize("c", gs.DIT_CASES, ids=_ID)
def test_dit_autograd_slices(dev, c):
    """depth 3 (the bf16 gradient shadow crosses two block boundaries): every parameter gradient, the output, and the gradients of
    x_t, the context and the global conditioning"""
    ref = dit_ref(c["id"], (c["seed"],))
    g, loss = _dit_step(_dit_module(c, dev), c, dev)
    assert set(g) == set(ref["layout"]), set(g) ^ set(ref["layout"])
    assert abs(loss - ref["g64"]["loss"].item()) <= 1e-2 * abs(ref["g64"]["loss"].item())
    assert_slices(g, ref, None, f"dit-autograd {c['id']}")
    seeded = assert_defects_caught(ref)
    assert len(seeded) == (7 if c["gtype"] == "adaLN" else 6) and "act:d_xt" in seeded and "act:d_ctx" in seeded


# ------------------------------------------------------------------------------------------------ DiT, trainer
def _wrapped(c, dev):
    from kalle_audio_amd.stable_audio_tools.models.diffusion import ConditionedDiffusionModelWrapper, DiTWrapper
    dit = DiTWrapper(**gs.dit_module_kwargs(c))
    load_seeded(dit.model, c["seed"], dev)
    return ConditionedDiffusionModelWrapper(dit, None, io_channels=gs.CIO, sample_rate=16000, min_input_length=1,
                                            cross_attn_cond_ids=["prompt"], global_cond_ids=["g"]).to(dev)


def _train_step(tr, model, c, seed, dev):
    inp = {k: None if v is None else v.to(dev) for k, v in gs.dit_inputs(c, seed).items()}
    cm = inp["cm"] if inp["cm"] is not None else torch.ones(inp["ctx"].shape[:2], dtype=torch.bool, device=dev)
    cond = {"prompt": (inp["ctx"], cm), "g": (inp["gl"], None)}
    return tr.train_step(model, inp["lat"], inp["t"], inp["noise"], cond, objective=c["obj"], padding_mask=inp["pm"])


PRE = "model.model."     # ConditionedDiffusionModelWrapper.model (DiTWrapper) .model (DiffusionTransformer)


def _flat_grads(tr):
    return {n[len(PRE):]: tr.flat.grad_view(n).float().cpu().clone() for n in tr.flat.names}


@pytest.mark.parametrize("tc", gs.TRAINER_CASES, ids=_ID)
def test_dit_trainer_slices(dev, monkeypatch, tc):
    """tr.flat.grad_view(n) at lr = 0 against the fp64 gradient SUMMED over the window's micro-batches (the flat buffer holds the
    sum; engine._adam_range folds 1 / (world accum) into the fused Adam step as grad_scale).  The second window runs on other data:
    whatever the first left in the flat buffer must be gone."""
    from kalle_audio_amd import dit_ops, engine
    c = tc["base"]
    monkeypatch.setattr(dit_ops, "GROUP_WGRAD", tc["group"])
    model = _wrapped(c, dev)
    tr = engine.DataParallelTrainer(model, lr=0.0, optimizer="Adam", grad_accum_steps=tc["accum"])
    assert len(tr.blocks) == gs.DEPTH
    for w in (0, 1):
        seeds = tuple(gs.window_seeds(tc, w))
        ref = dit_ref(c["id"], seeds)
        for s in seeds:
            _train_step(tr, model, c, s, dev)
        torch.cuda.synchronize()
        rows = c["B"] * (c["T"] + (c["gtype"] == "prepend"))
        assert all(blk._kalle_last_rows == rows for _, blk in tr.blocks)
        g = _flat_grads(tr)
        names = [n for n in ref["layout"] if not n.startswith("act:")]
        assert set(g) == set(names)
        assert_slices(g, ref, names, f"dit-trainer {tc['id']} window {w}")
        # sensitivity at the scale of the summed gradient (a window of one micro-batch carries the bias defect too)
        assert len(assert_defects_caught(ref)) >= 3
    # ... and the bias defect on the single-micro-batch reference of the same model, which keeps the per-token rows
    assert dit_ref(c["id"], (c["seed"],))["sites"]["bias"] in assert_defects_caught(dit_ref(c["id"], (c["seed"],)))


# ------------------------------------------------------------------------------------------------ partially frozen
def _freeze(module, frozen):
    for n, p in module.named_parameters():
        p.requires_grad_(not frozen(n))


def _adam_hp():
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32).item())
    return dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), weight_decay=0.0)


def _assert_adam_step(p, m, v, p0, g, m0, v0, step, what):
    """one kalle_adam_step against kernel_refs.adam_step in fp64 ON THE SAME GRADIENT, inside the bound tests/test_norm_elementwise_gpu.py
    (run_adam) derives for the kernel"""
    from test_norm_elementwise_gpu import ALLOW, U
    hp = _adam_hp()
    p0, g, m0, v0 = (t.double().cpu() for t in (p0, g, m0, v0))
    pr, mr, vr = kr.adam_step(p0, g, m0, v0, decoupled=False, step=step, grad_scale=1.0, **hp)
    b1, b2, lr = hp["beta1"], hp["beta2"], hp["lr"]
    gq = g.abs()
    dm = 4 * U * (m0.abs() + gq)
    dv = 6 * U * (v0.abs() + gq * gq)
    bc1, bc2 = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    denom = vr.sqrt() / bc2 + hp["eps"]
    upd = (lr / bc1) * mr.abs() / denom
    R = 8 + ALLOW["DIV"] + 2 * b1 ** step / bc1 + b2 ** step / bc2 ** 2
    tol = 3 * U * p0.abs() + R * U * upd + (lr / bc1) * (dm / denom + mr.abs() / denom.pow(2) * dv / (2 * vr.sqrt() * bc2 + 1e-300))
    for got, want, t, nm in ((m, mr, dm, "m"), (v, vr, dv, "v"), (p, pr, tol, "p")):
        over = ((got.double().cpu() - want).abs() - (t + 1e-38)).max().item()
        assert over <= 0, (what, nm, over)


@pytest.mark.parametrize("fc", gs.FROZEN_CASES, ids=_ID)
def test_partially_frozen_slices(dev, fc):
    """some parameters frozen, the others trainable: (1) plain autograd - the trainable gradients pass the slice check, the frozen
    parameters get no .grad; (2) the trainer, whose GradOut then mixes sinks and fresh tensors inside one block: the frozen names
    are absent from the flat buffer, the step-1 gradients pass the slice check, two steps at lr = 1e-3 leave the frozen weights
    and their bf16 compute copies bit-unchanged and move the trainable ones as an fp64 Adam does.

    The Adam reference consumes the gradient the trainer's flat buffer holds (itself held to the fp64 gradient by the slice check
    at both steps), not the fp64 gradient: the bound of tests/test_norm_elementwise_gpu.py is a few fp32 ulps of the update, and a
    bf16-operand gradient differs from the fp64 one by r(p) ~ 1e-2 - at step 1 Adam's update is lr * sign(g), so every element
    whose sign the rounding flips would be off by 2 lr.  The step-2 reference gradient is taken at the trainer's own step-1 weights."""
    from kalle_audio_amd import dit_ops, engine
    c, frozen = fc["base"], gs.FROZEN_SETS[fc["frozen"]]
    ref = dit_ref(c["id"], (c["seed"],))
    all_names = [n for n in ref["layout"] if not n.startswith("act:")]
    train = [n for n in all_names if not frozen(n)]
    assert train and len(train) < len(all_names)
    acts = ["act:out", "act:d_xt"] + (["act:d_ctx", "act:d_glob"] if fc["inputs_grad"] else [])
    # (1) plain autograd
    dit = _dit_module(c, dev)
    _freeze(dit, frozen)
    g, _ = _dit_step(dit, c, dev, inputs_grad=fc["inputs_grad"])
    assert all(p.grad is None for n, p in dit.named_parameters() if frozen(n))
    assert set(g) == set(train + acts), set(g) ^ set(train + acts)
    assert_slices(g, ref, train + acts, f"frozen-autograd {fc['id']}")
    del dit, g
    # (2) trainer
    model = _wrapped(c, dev)
    _freeze(model.model.model, frozen)
    params = dict(model.model.model.named_parameters())
    tr = engine.DataParallelTrainer(model, lr=1e-3, optimizer="Adam")
    assert {n[len(PRE):] for n in tr.flat.slices} == set(train)
    for n in all_names:
        if frozen(n):
            assert params[n].grad is None and not params[n].requires_grad, n
    w0 = {n: params[n].detach().clone() for n in all_names if frozen(n)}
    st_now = dict(ref["st"])
    state = (tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
    b0 = None
    for step in (1, 2):
        _train_step(tr, model, c, c["seed"], dev)
        torch.cuda.synchronize()
        if step == 1:       # the frozen matrices' bf16 compute copies exist now (made by the first forward)
            b0 = {n: dit_ops.bf16_of(params[n]).clone() for n in w0 if params[n].dim() >= 2}
            assert b0 or fc["frozen"] == "ff_bias"
        g = _flat_grads(tr)
        assert set(g) == set(train)
        if step == 2:       # the reference at the weights this step actually started from
            g64 = gs.dit_window(c, st_now, (c["seed"],))       # (and its own yardstick: a step of lr * sign(g) on few tensors
            ref = dict(ref, g64=g64, r=gs.yardstick(gs.dit_window(c, st_now, (c["seed"],), "emu"), g64, ref["layout"])[0])  # shrinks |g|)
        assert_slices(g, ref, train, f"frozen-trainer {fc['id']} step {step}")
        _assert_adam_step(tr.flat.param, tr.exp_avg, tr.exp_avg_sq, state[0], tr.flat.grad, state[1], state[2], step,
                          f"{fc['id']} step {step}")
        assert torch.equal(tr.flat.param_bf16, tr.flat.param.bfloat16())
        state = (tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
        st_now = {n: (params[n].detach().float().cpu().numpy().copy() if n in train else v) for n, v in st_now.items()}
    for n, w in w0.items():
        assert torch.equal(params[n].detach(), w), n
        assert params[n].grad is None, n
    for n, b in b0.items():
        assert torch.equal(dit_ops.bf16_of(params[n]), b), n
    assert (state[0] != 0).any() and max((params[n].detach().float().cpu() - torch.from_numpy(ref["st"][n])).abs().max().item()
                                         for n in train) > 1e-4           # the trainable weights did move
    # sensitivity on the reference: the defects are seeded into the tensors this case checks (what the frozen set leaves of them)
    ref0 = dit_ref(c["id"], (c["seed"],))
    sites = ref0["sites"]
    caught = 0
    for label, n, gd in gs.seeded_defects(ref0["g64"], ref0["layout"], sites, ref0["g64"]["rows:" + sites["bias"]]):
        if n in train + acts:
            rho = gs.check(gd, ref0["g64"], ref0["r"], ref0["layout"], [n])
            assert gs.failures(rho), (label, n, rho[n])
            caught += 1
    assert caught >= 1 + fc["inputs_grad"]            # the token row of the x_t gradient (and of the context's) at the least
    # ... and one 16-row slice x 1.10 in EVERY trainable matrix, wherever the frozen set left it
    for n in train:
        if ref0["g64"][n].dim() >= 2:
            mid = ref0["layout"][n][len(ref0["layout"][n]) // 2]
            gd = dict(ref0["g64"])
            gd[n] = ref0["g64"][n].clone()
            gs.view2d(gd[n])[mid[0]:mid[1]] *= 1.10
            rho = gs.check(gd, ref0["g64"], ref0["r"], ref0["layout"], [n])
            assert gs.failures(rho) and rho[n][1] == mid, (n, rho[n])


# ------------------------------------------------------------------------------------------------ Llasa
@functools.lru_cache(maxsize=None)
def llasa_ref(case_id):
    c = next(c for c in gs.LLASA_CASES if c["id"] == case_id)
    st = gu.make_state(gs.llasa_shapes(c), c["seed"])
    batch, eps = gs.llasa_inputs(c)
    sites = gs.llasa_defect_sites(c)
    g64 = gs.llasa_reference(c, st, batch, eps, bias_rows=sites["bias"])
    layout = gs.llasa_layout(c, g64)
    r, _ = gs.yardstick(gs.llasa_reference(c, st, batch, eps, "emu"), g64, layout)
    return dict(st=st, batch=batch, eps=eps, g64=g64, layout=layout, r=r, sites=sites)


@pytest.mark.parametrize("c", gs.LLASA_CASES, ids=_ID)
def test_llasa_slices(dev, tmp_path, c):
    """model_sigmaVAE.Llasa: every parameter gradient under the reference's names (q | k | v and gate | up split at the HF
    boundaries, heads of 64 / 128 rows), and pre_mean per valid position, against ko.llasa_forward in fp64"""
    from kalle_audio_amd.model_sigmaVAE import Llasa
    ref = llasa_ref(c["id"])
    lc = gs.llasa_config(c)
    d = tmp_path / "llama"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": c["lat"], "audio_proj_dim": lc["llama"]["hidden_size"]}, _Tok(310),
              use_flash_attention=False)
    sd = {k: torch.from_numpy(v) for k, v in ref["st"].items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    m = m.to(dev)
    b = {k: torch.from_numpy(v).to(dev) for k, v in ref["batch"].items()}
    out = m(b["input_ids"], b["audio_latents"], b["audio_distribution_l"], b["ids_mask"], b["audio_mask"], b["target_mask"],
            b["end_mask"], noise=torch.from_numpy(ref["eps"]).to(dev))
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    torch.cuda.synchronize()
    for k in ("audio_loss", "end_loss"):
        assert abs(out[k].item() - ref["g64"][k].item()) <= 1e-2 * abs(ref["g64"][k].item()), k
    valid = ((b["ids_mask"] + b["audio_mask"]) > 0).cpu()
    g = {n: t.float().cpu() for n, t in _hf_grads(m).items()}
    g["act:pre_mean"] = out["pre_mean"].detach().float().cpu()[valid]
    assert set(g) == set(ref["layout"]), set(g) ^ set(ref["layout"])
    assert_slices(g, ref, None, f"llasa {c['id']}")
    assert len(assert_defects_caught(ref)) == 5
