"""The optimizer-step check of tests/trainer_oracle.py on the reference alone (no GPU): an fp32 torch evaluation of the same
formulas stands in for the device, over the flat layout of a real engine.FlatBuckets built from the depth-3 DiT shapes of
grad_slices.TRAINER_CASES with synthetic gradients.  The stand-in must stay inside every bound at every step of every
configuration; every seeded defect must fall out of bound on every configuration, except the pairs of trainer_oracle.BLIND,
each of which is asserted blind.  FlatBuckets' ordering (vectors lead a bucket) and 64-element alignment are checked here too."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_slices as gs  # noqa: E402
import trainer_oracle as to  # noqa: E402

gu = gs.gu
CASE = gs.TRAINER_CASES[2]["base"]          # 713: adaLN (the widest inventory of vectors), D = 128
BLOCK = "transformer.layers.1."


def _bucket_of(n):
    for i in range(gs.DEPTH):
        if n.startswith(f"transformer.layers.{i}."):
            return f"transformer.layers.{i}."
    return "_rest"


@functools.lru_cache(maxsize=None)
def flat_and_params():
    from kalle_audio_amd.engine import FlatBuckets
    st = gu.make_state(gs.dit_shapes(CASE), CASE["seed"])
    named = [(n, torch.nn.Parameter(torch.from_numpy(v).clone())) for n, v in st.items()]
    return FlatBuckets(named, _bucket_of, torch.device("cpu")), named, st


def _grads(flat, n, seed, accum):
    """the window's SUM of `accum` micro-batch gradients: per-parameter magnitudes spread over 1e-4 ... 1e-1, exact zeros in the
    alignment gaps (what the trainer's flat gradient holds there)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        G = torch.zeros(flat.total)
        for i, (name, (s, ne)) in enumerate(flat.slices.items()):
            G[s:s + ne] = sum(torch.randn(ne, generator=g) for _ in range(accum)) * 10.0 ** -(1 + i % 4)
        out.append(G)
    return out


@functools.lru_cache(maxsize=None)
def run(name):
    flat, _, _ = flat_and_params()
    kw, every, steps = to.CONFIGS[name]
    cfg = to.cfg_from_kw(kw)
    state = dict(param=flat.param.clone(), exp_avg=torch.zeros(flat.total), exp_avg_sq=torch.zeros(flat.total))
    return cfg, to.standin_run(state, _grads(flat, steps, 7, cfg["accum"]), cfg, every)


# ------------------------------------------------------------------------------------------------ host helpers
def test_flat_buckets_layout():
    flat, named, st = flat_and_params()
    assert flat.bucket_keys == [k for k in dict.fromkeys(_bucket_of(n) for n, _ in named)] and len(flat.bucket_keys) == gs.DEPTH + 1
    end = 0
    for k in flat.bucket_keys:                      # the buckets tile [0, total) in order
        a, b = flat.bucket_range[k]
        assert a == end and b > a
        end = b
        s0, s1 = flat.small_range[k]
        assert s0 == a and a <= s1 <= b
        for n, p in named:
            if _bucket_of(n) == k:
                s, ne = flat.slices[n]
                assert s % 64 == 0 and ne == p.numel() and a <= s and s + ne <= b, n
                assert (s + ne <= s1) if p.dim() < 2 else (s >= s1), n        # the vectors lead, the matrices follow
    assert end == flat.total and flat.total % 64 == 0
    spans = sorted(flat.slices.values())
    assert all(s0 + n0 <= s1 for (s0, n0), (s1, _) in zip(spans, spans[1:]))       # no overlap
    gaps = to.gap_mask(flat)
    # (every DiT tensor here is a multiple of 64 elements: the gaps appear in the layout of the next test and in Llasa's)
    assert int((~gaps).sum()) == sum(p.numel() for _, p in named)
    assert not flat.param[gaps].any() and not flat.grad[gaps].any() and not flat.param_bf16[gaps].any()
    for n, p in named:
        s, ne = flat.slices[n]
        assert torch.equal(flat.param[s:s + ne], torch.from_numpy(st[n]).reshape(-1)), n
        assert p.data_ptr() == flat.param[s:s + ne].data_ptr() and p.grad.data_ptr() == flat.grad[s:s + ne].data_ptr(), n
    assert torch.equal(flat.param_bf16, flat.param.bfloat16())


def test_atomic_grad_matrices_travel_with_the_vectors():
    from kalle_audio_amd.engine import FlatBuckets
    w = torch.nn.Parameter(torch.ones(5, 17))
    w._kalle_atomic_grad = True
    named = [("b.m", torch.nn.Parameter(torch.ones(3, 70))), ("b.taps", w), ("b.v", torch.nn.Parameter(torch.ones(65)))]
    flat = FlatBuckets(named, lambda n: "b.", torch.device("cpu"), with_bf16=False)
    assert flat.slices == {"b.taps": (0, 85), "b.v": (128, 65), "b.m": (256, 210)}
    assert flat.small_range["b."] == (0, 256) and flat.bucket_range["b."] == (0, 512) and flat.param_bf16 is None
    gaps = to.gap_mask(flat)
    assert int(gaps.sum()) == 512 - 85 - 65 - 210 and not flat.param[gaps].any() and (flat.param[~gaps] == 1).all()


# ------------------------------------------------------------------------------------------------ the stand-in and the defects
@pytest.mark.parametrize("name", list(to.CONFIGS))
def test_standin_is_inside_every_bound(name):
    flat, _, _ = flat_and_params()
    cfg, recs = run(name)
    gaps = to.gap_mask(flat)
    for r in recs:
        ratios = to.check_step(r["before"], r["after"], r["G"], cfg, r["k"], flat.bucket_range, gaps)
        assert not to.failures(ratios), (name, r["k"], to.failures(ratios), to.worst(ratios))
        assert set(flat.bucket_keys) == {b for q, b in ratios if q == "p"}          # every bucket is reported
    w = to.evaluate(recs, cfg, flat.bucket_range, gaps)
    print(f"STANDIN {name}: " + " ".join(f"{q} {v:.3f}" for q, v in sorted(w.items())))
    assert max(w["p"], w["m"], w["v"]) > 0.01         # the bounds are not slack by orders of magnitude: fp32 roundings do register


@pytest.mark.parametrize("defect", to.DEFECTS)
@pytest.mark.parametrize("name", list(to.CONFIGS))
def test_defect_is_caught_or_listed_blind(name, defect):
    flat, _, _ = flat_and_params()
    cfg, recs = run(name)
    for bucket in ((BLOCK, "_rest") if defect in to.BUCKET_DEFECTS else (None,)):
        w = to.evaluate(recs, cfg, flat.bucket_range, to.gap_mask(flat), defect, bucket, stop=to.shown(defect))
        if (name, defect) in to.BLIND:
            assert not to.caught(w), (name, defect, to.BLIND[(name, defect)], w)
        else:
            assert to.caught(w), (name, defect, bucket, w)
            if defect == "no_accum_scale":          # Adam's update is invariant to the gradient's scale: the MOMENTS must show it
                assert w["m"] > 1 and w["v"] > 1, w
            if defect in ("mirror_before",):
                assert w["mirror"] > 1 and max(w["p"], w["m"], w["v"]) <= 1, w
            if defect in ("ema_before", "ema_epoch_early"):
                assert w["ema"] > 1 and max(w["p"], w["m"], w["v"]) <= 1, w


def test_blind_table_is_short_and_well_formed():
    pairs = len(to.CONFIGS) * len(to.DEFECTS)
    assert all(c in to.CONFIGS and d in to.DEFECTS and why for (c, d), why in to.BLIND.items())
    assert 5 * len(to.BLIND) <= pairs, (len(to.BLIND), pairs)
    # the pairs expected blind: the schedule at k under a constant schedule, coupled / decoupled swapped at weight_decay = 0
    assert ("plain", "sched_at_k") in to.BLIND and ("plain", "decay_swapped") in to.BLIND


def test_grad_scale_shows_in_the_moments_only():
    """first step (zero moments) of AdamW at constant lr, accum = 2, |g| >= 1e-3: with the 1 / accum lost the weights move by
    lr eps / (2 |g'|) <= 1e-8 relative to the update - inside p's bound - while m is doubled and v quadrupled"""
    flat, _, _ = flat_and_params()
    cfg = to.make_cfg(lr=1e-3, weight_decay=0.01, decoupled=True, accum=2)
    g = torch.Generator().manual_seed(3)
    G = torch.randn(flat.total, generator=g)
    G = torch.where(to.gap_mask(flat), torch.zeros(()), G.sign() * (G.abs() * 1e-2 + 2e-3))
    state = dict(param=flat.param.clone(), exp_avg=torch.zeros(flat.total), exp_avg_sq=torch.zeros(flat.total))
    rec = to.standin_run(state, [G], cfg)
    assert not to.caught(to.evaluate(rec, cfg, flat.bucket_range, to.gap_mask(flat)))
    w = to.evaluate(rec, cfg, flat.bucket_range, to.gap_mask(flat), "no_accum_scale")
    assert w["p"] <= 1 and w["m"] > 1e3 and w["v"] > 1e3, w


def test_llasa_inputs_seed_keeps_the_default_data():
    c = gs.LLASA_CASES[1]
    (b0, e0), (b1, e1), (b2, e2) = gs.llasa_inputs(c), gs.llasa_inputs(c, c["seed"]), gs.llasa_inputs(c, c["seed"] + 10)
    assert all((b0[k] == b1[k]).all() for k in b0) and (e0 == e1).all()
    assert gu.llasa_batch_long(gs.llasa_config(c), c["seed"], B=c["B"], L=c["L"])["input_ids"].tolist() == b0["input_ids"].tolist()
    assert not (b0["input_ids"] == b2["input_ids"]).all() and not (e0 == e2).all() and e2.shape == e0.shape


def test_expected_ema_follows_the_schedule():
    from kalle_audio_amd.engine import EMASchedule
    sc = EMASchedule(update_every=1, **to.EMA_KW)
    e0, p = torch.randn(70), torch.randn(70)
    kinds = []
    for _ in range(5):
        before = (sc.step, sc.initted)
        kind, ref, tol = to.expected_ema(e0, p, sc)
        assert (sc.step, sc.initted) == before            # the caller's schedule is not advanced
        kinds.append(kind)
        d = sc.next()
        if kind == "avg":
            a, b = to.f32(d), to.f32(1 - d)
            assert torch.equal(ref, a * e0.double() + b * p.double()) and (tol > 0).all()
    assert kinds == ["copy", "copy", "copy", "avg", "avg"]
    sc2 = EMASchedule(update_every=2, **to.EMA_KW)
    kinds = []
    for _ in range(5):
        kinds.append(to.expected_ema(e0, p, sc2)[0])
        sc2.next()
    assert kinds == ["copy", "skip", "copy", "skip", "avg"]


def test_adam_bound_is_the_formula_of_run_adam():
    """the constants are imported, not restated: R at step 1 is 8 + ALLOW["DIV"] + 2 b1 / (1 - b1) + b2 / (1 - b2)"""
    from test_norm_elementwise_gpu import ALLOW, U
    assert to.U is U and to.ALLOW is ALLOW
    hp = dict(lr=to.f32(1e-2), beta1=to.f32(0.9), beta2=to.f32(0.999), eps=to.f32(1e-8), weight_decay=to.f32(0.1))
    one = torch.ones(1, dtype=torch.float64)
    pr, mr, vr = to.kr.adam_step(one, one, 0 * one, 0 * one, decoupled=True, step=1, grad_scale=0.5, **hp)
    dm, dv, tol = to.adam_bound(one, one, 0 * one, 0 * one, pr, mr, vr, hp, 1, 0.5, True)
    assert dm.item() == 4 * U * 0.5 and dv.item() == 6 * U * 0.25
    b1, b2 = hp["beta1"], hp["beta2"]
    R = 8 + ALLOW["DIV"] + 2 * b1 / (1 - b1) + b2 / (1 - b2)
    bc1, bc2 = 1 - b1, (1 - b2) ** 0.5
    den = vr.sqrt() / bc2 + hp["eps"]
    want = 3 * U + R * U * (hp["lr"] / bc1) * mr / den + (hp["lr"] / bc1) * (dm / den + mr / den ** 2 * dv / (2 * vr.sqrt() * bc2 + 1e-300))
    assert abs(tol.item() - want.item()) <= 1e-12 * want.item()
    dmc, _, _ = to.adam_bound(one, one, 0 * one, 0 * one, pr, mr, vr, hp, 1, 0.5, False)
    assert dmc.item() == 4 * U * (0.5 + hp["weight_decay"])
