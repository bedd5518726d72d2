"""-m gpu: the code between a finished gradient and the next forward's weights - engine.DataParallelTrainer and
engine.FusedAdam - held element by element to the teacher-forced fp64 reference of tests/trainer_oracle.py after EVERY optimizer
step: the flat param, both moments, the bf16 mirror, last_lr, step_count, the EMA and the alignment gaps, per bucket, inside the
bound run_adam derives for kalle_adam_step (and test_axpby's for the EMA).  T1 ... T9 are the cases of DESIGN.md, "Optimizer
steps per element", where the measured worst ratios are recorded.  Models: the depth-3 DiTs of grad_slices.TRAINER_CASES and the
Llasa models of grad_slices.LLASA_CASES."""
import copy
import functools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_slices as gs  # noqa: E402
import trainer_oracle as to  # noqa: E402
import test_grad_slices_gpu as tg  # noqa: E402
from test_modules_gpu import _Tok  # noqa: E402

gu = gs.gu
TC = {int(tc["base"]["id"][1:4]): tc for tc in gs.TRAINER_CASES}
MID = tg.PRE + "transformer.layers.1."
RECORDS = {}        # name -> (cfg, records, ranges, gaps): the device's recorded states, shared with the sensitivity test (T9)


def _report(what, w):
    print(f"TRAINER {what}: " + " ".join(f"{q} {v:.3f}" for q, v in sorted(w.items())))


def _assert_step(tr, cfg, before, after, k, what, total):
    ratios = to.check_step(before, after, after["grad"], cfg, k, tr.flat.bucket_range, to.gap_mask(tr.flat))
    assert not to.failures(ratios), (what, k, to.failures(ratios), to.worst(ratios))
    for q, v in to.worst(ratios).items():
        total[q] = max(total.get(q, 0.0), v)


def _windows(tr, model, c, dev, windows, what, on_window=None):
    """`windows` accumulation windows on fresh data each; every optimizer step is checked.  Returns the records."""
    cfg, accum, recs, total = to.cfg_of(tr), tr.grad_accum_steps, [], {}
    seed0 = c["seed"]
    for w in range(windows):
        torch.cuda.synchronize()
        before = to.snapshot(tr)
        for i in range(accum):
            tg._train_step(tr, model, c, seed0 + 10 * (w * accum + i), dev)
        torch.cuda.synchronize()
        after = to.snapshot(tr)
        k = before["step_count"] + 1
        _assert_step(tr, cfg, before, after, k, what, total)
        if on_window is not None:
            on_window(w)
        recs.append(dict(before=before, after=after, G=after["grad"], k=k))
    _report(what, total)
    assert (recs[-1]["after"]["param"] != recs[0]["before"]["param"]).any()
    return recs


def _dit_trainer(name, case, dev, **over):
    from kalle_audio_amd import engine
    kw, every, steps = to.CONFIGS[name]
    c = TC[case]["base"]
    model = tg._wrapped(c, dev)
    tr = engine.DataParallelTrainer(model, **dict(kw, **over))
    if every is not None:
        tr.enable_ema(update_every=every, **to.EMA_KW)
    assert len(tr.blocks) == gs.DEPTH and "_rest" in tr.flat.bucket_keys
    return model, tr, c, steps


def _record(name, case, dev, group=True):
    """the device's run of configuration `name` on TRAINER_CASES' `case` (run once, kept for T9)"""
    from kalle_audio_amd import dit_ops
    key = (name, case, group)
    if key not in RECORDS:
        old, dit_ops.GROUP_WGRAD = dit_ops.GROUP_WGRAD, group
        try:
            model, tr, c, steps = _dit_trainer(name, case, dev)
            recs = _windows(tr, model, c, dev, steps, f"{name} case {case}" + ("" if group else " nogroup"))
            assert tr._overlap_now is False                 # 68 ... 504 rows: below overlap_min_rows, one pass at the end of the step
            RECORDS[key] = (to.cfg_of(tr), recs, dict(tr.flat.bucket_range), to.gap_mask(tr.flat))
        finally:
            dit_ops.GROUP_WGRAD = old
    return RECORDS[key]


# ------------------------------------------------------------------------------------------------ T1 ... T4
@pytest.mark.parametrize("case", [711, 712])
def test_t1_adamw_schedule_accumulation(dev, case):
    """AdamW, weight_decay 0.01, accum 2, a schedule with a distinct lr at every step (0 at the first), 4 windows"""
    cfg, recs, _, _ = _record("T1", case, dev)
    assert len({r["after"]["last_lr"] for r in recs}) == 4 and recs[0]["after"]["last_lr"] == 0.0
    assert [r["after"]["micro"] for r in recs] == [2, 4, 6, 8]


@pytest.mark.parametrize("case", [712, 715])
def test_t2_overlapped_buckets_step_exactly_once(dev, case):
    """T1 with overlap_min_rows = 0: every bucket, `_rest` included, is stepped on the side stream - the blocks' from their
    backward hooks, the rest from _finish_comm - and by nothing else; same bounds"""
    model, tr, c, steps = _dit_trainer("T1", case, dev)
    assert tr.overlap_adam
    tr.overlap_min_rows = 0
    queued, stepped, whole = [], [], []
    qb, ab, ar = tr._queue_bucket, tr._adam_bucket, tr._adam_range

    def queue_bucket(keys, ev):
        assert tr._overlap_now and torch.cuda.current_stream() != tr._opt_stream
        queued.extend(keys)
        return qb(keys, ev)

    def adam_bucket(key):
        assert torch.cuda.current_stream() == tr._opt_stream, key
        stepped.append(key)
        return ab(key)

    def adam_range(a, b, grad=None):
        whole.append((a, b))
        return ar(a, b, grad)

    tr._queue_bucket, tr._adam_bucket, tr._adam_range = queue_bucket, adam_bucket, adam_range

    def on_window(w):
        assert sorted(queued) == sorted(tr.flat.bucket_keys) and sorted(stepped) == sorted(queued), (queued, stepped)
        assert queued[-1] == "_rest" and sorted(whole) == sorted(tr.flat.bucket_range[k] for k in tr.flat.bucket_keys)
        del queued[:], stepped[:], whole[:]

    _windows(tr, model, c, dev, steps, f"T2 case {case} overlapped", on_window=on_window)


@pytest.mark.parametrize("group", [True, False], ids=["group", "nogroup"])
@pytest.mark.parametrize("case", [713, 715])
def test_t3_coupled_l2(dev, case, group):
    """Adam with coupled L2, weight_decay 0.1, accum 1, on the adaLN cases, grouped weight-gradient launch on and off"""
    cfg, recs, _, _ = _record("T3", case, dev, group)
    assert not cfg["decoupled"] and cfg["weight_decay"] == 0.1


@pytest.mark.parametrize("every", [1, 2])
def test_t4_ema(dev, every):
    """T1 plus the EMA as the reference configures it, update_every 1 and 2, 5 windows: copy steps, skipped steps, averaged steps"""
    cfg, recs, _, _ = _record(f"T4-every{every}", 713, dev)
    kinds = [to.expected_ema(r["before"]["ema"], r["after"]["param"], r["before"]["ema_sched"])[0] for r in recs]
    assert kinds == (["copy", "copy", "copy", "avg", "avg"] if every == 1 else ["copy", "skip", "copy", "skip", "avg"])
    assert [r["after"]["ema_sched"].step for r in recs] == [1, 2, 3, 4, 5]


# ------------------------------------------------------------------------------------------------ T5: resume
def _clone(v):
    if torch.is_tensor(v):
        return v.detach().clone()
    if isinstance(v, dict):
        return type(v)((k, _clone(x)) for k, x in v.items())
    return copy.deepcopy(v)


def test_t5_resume_in_the_middle_of_a_window(dev):
    """state_dict() after 5 micro-batches (accum 2: a half-finished window), loaded into a trainer over a differently seeded
    model: bit-equal state; both trainers then run 3 more micro-batches on the same data, the resumed one's steps pass the
    teacher-forced check with the ORIGINAL step numbers and learning rates, and its finished window's gradient is the saved
    partial sum plus the new micro-batch.

    The two gradients differ by the order of the fp32 atomics of the new micro-batch alone (same weights, same data): the bound
    of test_llasa_packed_gpu.py for atomically summed gradients, n 2^-24 of the tensor's largest entry, n the addends of a
    column sum or split-K sum: the token rows or the context rows of the micro-batch, whichever is more."""
    from kalle_audio_amd import engine
    kw, every, _ = to.CONFIGS["T4-every1"]
    c = TC[713]["base"]
    ma = tg._wrapped(c, dev)
    ta = engine.DataParallelTrainer(ma, **kw).enable_ema(update_every=every, **to.EMA_KW)
    for i in range(5):
        tg._train_step(ta, ma, c, c["seed"] + 10 * i, dev)
    torch.cuda.synchronize()
    sd = _clone(ta.state_dict())                       # (a checkpoint as a file would hold it: no storage shared with `ta`)
    assert "grad" in sd and sd["micro"] == 5 and sd["step"] == 2
    mb = tg._wrapped(dict(c, seed=c["seed"] + 1), dev)
    tb = engine.DataParallelTrainer(mb, **kw)
    assert not torch.equal(tb.flat.param, ta.flat.param)
    tb.load_state_dict(sd)
    torch.cuda.synchronize()
    a0, b0 = to.snapshot(ta), to.snapshot(tb)
    for key in ("param", "mirror", "exp_avg", "exp_avg_sq", "grad", "ema"):
        assert to._bits_equal(a0[key], b0[key]), key
    assert (b0["step_count"], b0["micro"]) == (2, 5) and (a0["grad"] != 0).any()
    assert vars(b0["ema_sched"]) == vars(a0["ema_sched"]) and b0["ema_sched"].step == 2
    cfg = to.cfg_of(tb)
    assert cfg == dict(to.cfg_of(ta))
    total, snaps = {}, {}
    for tr, m, tag in ((ta, ma, "a"), (tb, mb, "b")):
        before = to.snapshot(tr)
        for i in (5, 6, 7):
            tg._train_step(tr, m, c, c["seed"] + 10 * i, dev)
            torch.cuda.synchronize()
            if i in (5, 7):                            # micro-batch 6 ends window 3, micro-batch 8 window 4
                after = to.snapshot(tr)
                k = 3 if i == 5 else 4
                assert after["step_count"] == k and after["last_lr"] == to.lr_of(cfg, k)
                _assert_step(tr, cfg, before, after, k, f"T5 {tag}", total)
                snaps[(tag, k)] = after
                if (tag, k) == ("b", 3):               # ... and a bucket whose moments had NOT come back would show right here
                    for bucket in (MID, "_rest"):
                        lost = to.check_step(before, after, after["grad"], cfg, k, tb.flat.bucket_range, defect="moments_lost", bucket=bucket)
                        assert {("m", bucket), ("v", bucket)} <= set(to.failures(lost)), (bucket, to.failures(lost))
                before = after
    _report("T5 resume", total)
    n = c["B"] * max(c["T"] + (c["gtype"] == "prepend"), c["S"])
    ga, gb = snaps[("a", 3)]["grad"], snaps[("b", 3)]["grad"]
    worst = 0.0
    for name, (s, ne) in tb.flat.slices.items():
        a, b = ga[s:s + ne].double(), gb[s:s + ne].double()
        lim = n * 2.0 ** -24 * a.abs().max().item()
        worst = max(worst, (a - b).abs().max().item() / max(lim, 1e-300))
        assert (a - b).abs().max().item() <= lim, (name, (a - b).abs().max().item(), lim)
    print(f"TRAINER T5 resumed window gradient vs original: worst {worst:.3f} of the reordering bound")
    assert (gb != b0["grad"]).any()                 # the new micro-batch was added onto the restored partial sum


# ------------------------------------------------------------------------------------------------ T6: optimizer_step() directly
def test_t6_direct_optimizer_step(dev):
    """optimizer_step() after a manual loss.backward(): the `_opt_lr is None` route fixes step number and lr itself"""
    from kalle_audio_amd.stable_audio_tools.training.diffusion import diffusion_train_step
    model, tr, c, steps = _dit_trainer("plain", 711, dev)
    cfg, total = to.cfg_of(tr), {}
    for k in range(1, steps + 1):
        inp = {n: None if v is None else v.to(dev) for n, v in gs.dit_inputs(c, c["seed"] + 10 * k).items()}
        cond = {"prompt": (inp["ctx"], torch.ones(inp["ctx"].shape[:2], dtype=torch.bool, device=dev)), "g": (inp["gl"], None)}
        tr.flat.grad.zero_()
        loss, _ = diffusion_train_step(model, inp["lat"], inp["t"], inp["noise"], cond, objective=c["obj"], padding_mask=inp["pm"])
        loss.backward()
        torch.cuda.synchronize()
        assert tr._opt_lr is None
        before = to.snapshot(tr)
        assert (before["grad"] != 0).any()
        tr.optimizer_step()
        torch.cuda.synchronize()
        after = to.snapshot(tr)
        assert to._bits_equal(after["grad"], before["grad"]) and tr._opt_lr is None
        _assert_step(tr, cfg, before, after, k, "T6", total)
    _report("T6 direct optimizer_step", total)


# ------------------------------------------------------------------------------------------------ T7: FusedAdam
@pytest.mark.parametrize("adam_w_mode", [True, False], ids=["adamw", "adam"])
def test_t7_fused_adam_front_end(dev, adam_w_mode):
    """engine.FusedAdam on the small DiT through plain autograd, 3 steps, weight_decay 0.05: teacher-forced per parameter from
    p.grad and the optimizer's own state; a live bf16 compute copy is bit-equal to bf16(p) after the step, a stale one is gone,
    a parameter with grad None is untouched and has no state"""
    import test_round2_gpu as r2
    from kalle_audio_amd import ops
    from kalle_audio_amd.engine import FusedAdam
    from kalle_audio_amd.stable_audio_tools.training.diffusion import diffusion_train_step
    m = r2._small_dit(dev)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    opt = FusedAdam([p for _, p in named], lr=1e-3, weight_decay=0.05, adam_w_mode=adam_w_mode)
    cfg = to.make_cfg(lr=1e-3, weight_decay=0.05, decoupled=adam_w_mode)
    lat, noise, t, cond = r2._batch(dev, 2, 1)
    total = {}
    for k in (1, 2, 3):
        opt.zero_grad(set_to_none=True)
        loss, _ = diffusion_train_step(m, lat, t, noise, cond)
        loss.backward()
        live = [n for n, p in named if getattr(p, "_kalle_bf16", None) is not None and p._kalle_bf16[0] == ops.weights_key(p)]
        assert len(live) >= 8, live
        frozen_n, frozen_p = next((n, p) for n, p in named if p.dim() == 1 and p.grad is not None)
        stale_n, stale_p = next((n, p) for n, p in named if n in live)
        if k == 3:
            frozen_p.grad = None
            w_frozen = frozen_p.detach().clone()
        if k == 2:
            with torch.no_grad():
                stale_p.add_(0.0)                      # moves the version: the cached bf16 copy no longer belongs to these weights
            assert stale_p._kalle_bf16[0] != ops.weights_key(stale_p)
        act = [(n, p) for n, p in named if p.grad is not None]
        zero = lambda p: torch.zeros_like(p, dtype=torch.float32)
        cat = lambda ts: torch.cat([x.detach().float().reshape(-1) for x in ts]).cpu()
        before = dict(param=cat(p for _, p in act), exp_avg=cat(opt.state[p].get("exp_avg", zero(p)) for _, p in act),
                      exp_avg_sq=cat(opt.state[p].get("exp_avg_sq", zero(p)) for _, p in act))
        G = cat(p.grad for _, p in act)
        ranges, o = {}, 0
        for n, p in act:
            ranges[n] = (o, o + p.numel())
            o += p.numel()
        opt.step()
        torch.cuda.synchronize()
        after = dict(param=cat(p for _, p in act), exp_avg=cat(opt.state[p]["exp_avg"] for _, p in act),
                     exp_avg_sq=cat(opt.state[p]["exp_avg_sq"] for _, p in act))
        ratios = to.check_step(before, after, G, cfg, k, ranges)
        assert not to.failures(ratios), (k, to.failures(ratios)[:4])
        for q, v in to.worst(ratios).items():
            total[q] = max(total.get(q, 0.0), v)
        assert all(opt.state[p]["step"] == k for n, p in act) and (k < 3 or frozen_n not in dict(act))
        for n, p in named:
            if n in live and not (k == 2 and n == stale_n):
                assert p._kalle_bf16[0] == ops.weights_key(p) and to._bits_equal(p._kalle_bf16[1], p.detach().bfloat16()), n
        if k == 2:
            assert not hasattr(stale_p, "_kalle_bf16")
        if k == 3:
            assert to._bits_equal(frozen_p.detach(), w_frozen) and opt.state[frozen_p]["step"] == 2
    # a parameter that never had a gradient has no state at all
    extra = torch.nn.Parameter(torch.ones(70, device=dev))
    opt2 = FusedAdam([extra], lr=1e-3)
    opt2.step()
    assert extra not in opt2.state and bool((extra == 1).all())
    _report(f"T7 FusedAdam adam_w_mode {adam_w_mode}", total)


# ------------------------------------------------------------------------------------------------ T8: Llasa through the trainer
LLASA = {c["seed"]: c for c in gs.LLASA_CASES}


def _llasa_seeds(c, w):
    return tuple(c["seed"] + 10 * (2 * w + i) for i in range(2))         # (window 0 starts with the case's own data)


@functools.lru_cache(maxsize=None)
def llasa_window_ref(seed, w):
    c = LLASA[seed]
    base = tg.llasa_ref(c["id"])
    seeds = _llasa_seeds(c, w)
    g64 = gs.llasa_window(c, base["st"], seeds)
    layout = {n: v for n, v in base["layout"].items() if not n.startswith("act:")}
    r, _ = gs.yardstick(gs.llasa_window(c, base["st"], seeds, "emu"), g64, layout)
    return dict(g64=g64, layout=layout, r=r)


def _llasa_model(c, dev, tmp_path):
    from kalle_audio_amd.model_sigmaVAE import Llasa
    ref = tg.llasa_ref(c["id"])
    lc = gs.llasa_config(c)
    d = tmp_path / "llama"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": c["lat"], "audio_proj_dim": lc["llama"]["hidden_size"]}, _Tok(310),
              use_flash_attention=False)
    sd = {k: torch.from_numpy(v) for k, v in ref["st"].items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    return m.to(dev)


def _llasa_micro(tr, m, c, seed, dev):
    batch, eps = gs.llasa_inputs(c, seed)
    b = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    out = m(b["input_ids"], b["audio_latents"], b["audio_distribution_l"], b["ids_mask"], b["audio_mask"], b["target_mask"],
            b["end_mask"], noise=torch.from_numpy(eps).to(dev))
    tr.backward(out["audio_loss"] * 1.0 + out["end_loss"] * 0.5)


def _hf_flat_grads(tr, m):
    """tr.flat.grad_view(n) under the reference's (HF) names: the fused q | k | v and gate | up split like the weights"""
    g = {}
    for n in tr.flat.names:
        t = tr.flat.grad_view(n).float().cpu().clone()
        if n.endswith(("qkv_proj.weight", "up_gate_proj.weight")):
            o = 0
            for name, k in m.get_submodule(n.rsplit(".", 1)[0]).parts:
                g[n.rsplit(".", 2)[0] + "." + name + ".weight"] = t[o:o + k]
                o += k
        else:
            g[n] = t
    return g


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("seed", [801, 803])
def test_t8a_llasa_trainer_gradient_slices(dev, tmp_path, seed, packed):
    """lr = 0: tr.flat.grad_view(n) per slice against the fp64 gradient summed over the window's two micro-batches (M = 3,
    grad_slices' own yardstick), two windows on different data - the per-layer sinks, the embedding table's scatter-add into the
    `_rest` bucket, the clear of the first micro-batch and the accumulation of the second"""
    from kalle_audio_amd import engine
    c = LLASA[seed]
    m = _llasa_model(c, dev, tmp_path)
    if packed:
        m.pack_sequences()
    tr = engine.DataParallelTrainer(m, lr=0.0, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2)
    assert len(tr.blocks) == c["layers"] and "_rest" in tr.flat.bucket_range
    p0 = tr.flat.param.clone()
    for w in (0, 1):
        ref = llasa_window_ref(seed, w)
        for s in _llasa_seeds(c, w):
            _llasa_micro(tr, m, c, s, dev)
        torch.cuda.synchronize()
        g = _hf_flat_grads(tr, m)
        assert set(g) == set(ref["layout"]), set(g) ^ set(ref["layout"])
        rho = tg.assert_slices(g, ref, None, f"T8a llasa-trainer {c['id']} {'packed' if packed else 'padded'} window {w}")
        assert "base_model.model.embed_tokens.weight" in rho
        assert tr.step_count == w + 1 and torch.equal(tr.flat.param, p0)
    # sensitivity at the scale of the summed gradient: the defects a whole-tensor norm cannot see, seeded into the window's reference
    ref = dict(llasa_window_ref(seed, 1), sites=dict(gs.llasa_defect_sites(c), token=[]))
    assert len(tg.assert_defects_caught(ref)) == 3


@pytest.mark.parametrize("seed", [801, 803])
def test_t8b_llasa_trainer_steps(dev, tmp_path, seed):
    """lr = 1e-3, AdamW, accum 2, two windows: the teacher-forced step check on Llasa's buckets (whose layout has alignment gaps)"""
    from kalle_audio_amd import engine
    c = LLASA[seed]
    m = _llasa_model(c, dev, tmp_path)
    tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2)
    cfg, total = to.cfg_of(tr), {}
    assert to.gap_mask(tr.flat).any()
    for w in (0, 1):
        torch.cuda.synchronize()
        before = to.snapshot(tr)
        for s in _llasa_seeds(c, w):
            _llasa_micro(tr, m, c, s, dev)
        torch.cuda.synchronize()
        _assert_step(tr, cfg, before, to.snapshot(tr), w + 1, f"T8b {c['id']}", total)
    _report(f"T8b llasa {c['id']}", total)


# ------------------------------------------------------------------------------------------------ T9: sensitivity on the device's output
@pytest.mark.parametrize("name,case", [("T1", 712), ("T3", 713), ("T4-every1", 713), ("T4-every2", 713)])
def test_t9_defects_fail_on_the_device_states(dev, name, case):
    """every DEFECTS entry, seeded into the reference, against the states the DEVICE recorded: out of bound, except the pairs of
    trainer_oracle.BLIND (each asserted blind on the CPU)"""
    cfg, recs, ranges, gaps = _record(name, case, dev)
    for defect in to.DEFECTS:
        for bucket in ((MID, "_rest") if defect in to.BUCKET_DEFECTS else (None,)):
            w = to.evaluate(recs, cfg, ranges, gaps, defect, bucket, stop=to.shown(defect))
            if (name, defect) in to.BLIND:
                assert not to.caught(w), (name, defect, w)
            else:
                assert to.caught(w), (name, defect, bucket, w)
                if defect == "no_accum_scale":
                    assert w["m"] > 1 and w["v"] > 1, w
