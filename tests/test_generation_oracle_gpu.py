"""-m gpu: the COMPOSED KV-cached generation - LlamaModel.init_cache* / forward_cached / prefill_row / forward_cached_batch and
Llasa.infer / infer_batch / _generate_device_head - held frame by frame to the fp64 oracle of tests/gen_oracle.py: every hidden
state the cache API returns and every predicted mean of a generated frame within M = 3 times a yardstick that comes from the
reference alone, on a state whose RMSNorm gains make the decoder depend on its own attention.

A  scripted cache drive: the test chooses the inputs and the active schedule (prompts of 1 / 14 / 250 positions, rows that leave and
   come back, a row that crosses 256 -> 257 keys while the others are short, 16 rows), batch cache and single cache, with and
   without the final norm.  The embeddings of an inactive row are NaN: whatever read them would show.
B  infer / infer_batch end to end under fixed noise: each frame's mean is recovered as latent - std noise and compared with the
   oracle teacher-forced on the RETURNED latents.
C  the stop rule against the fp64 frame KLs.
D  wrong references (a gap of one rotary position, two rows swapped, frames shifted by one) fail the same check on the device's
   results, and every (format, head, rows) combination and both sides of Nk = 256 | 257 were seen.

Measured on an MI355X: DESIGN.md, "Generation per frame: the cached path against fp64"."""
import functools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle as go  # noqa: E402
from test_llasa_batch_gpu import fixed_noise  # noqa: E402
from test_modules_gpu import _Tok  # noqa: E402

gs = go.gs
T, PS, ROOM = 12, (1, 14, 250), 262
HEADS = ("host", "dev0", "dev1")          # the host head; device_head=True with stop_lag 0 and 1
PSETS = ("one", "single", "ragged3", "seventeen")
STOP_CASE, STOP_SEED = go.STOP_CASE, go.STOP_SEED
SEEN, KEEP, MEASURED = set(), {}, {}
_ID = lambda c: c["id"]
_CASE = {c["id"]: c for c in go.CASES}


@functools.lru_cache(maxsize=None)
def state(case_id):
    return go.make_state(_CASE[case_id])


@functools.lru_cache(maxsize=None)
def weights(case_id, fmt):
    return go.weights(_CASE[case_id], state(case_id), fmt)


def build(c, dev, tmp_path, fmt=None):
    """model_sigmaVAE.Llasa on the attention-sensitive state, loaded under the reference's names (the loader fuses q | k | v and
    up | gate)"""
    from kalle_audio_amd.model_sigmaVAE import Llasa
    lc = gs.llasa_config(c)
    d = tmp_path / "llama"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps(dict(lc["llama"], model_type="llama")))
    m = Llasa({"llm_model_name_or_path": str(d), "latent_dim": c["lat"], "audio_proj_dim": lc["llama"]["hidden_size"]}, _Tok(310),
              use_flash_attention=False)
    sd = {k: torch.from_numpy(v) for k, v in state(c["id"]).items()}
    sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
    m.load_state_dict(sd)
    m = m.to(dev)
    if fmt:
        m.quantize_decoder(fmt)
    return m


def hold(xs, x64s, r, what, key, offsets=None, P=None):
    """the check of gen_oracle on every (row, position); prints and records the worst ratio in units of r"""
    v, row, i = go.worst(xs, x64s)
    print(f"GEN {what}: worst ratio {v:.3e} = {v / r:.2f} r at row {row} index {i} (r {r:.3e}); {sum(len(x) for x in xs)} positions")
    MEASURED[key] = max(MEASURED.get(key, 0.0), v / r)
    msg = go.failure(xs, x64s, r, what, offsets, P)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ A: scripted cache drive
def three_rows(s):
    """row 0 always on, row 1 off from step 5 on, row 2 off at steps 3 - 4 and on again afterwards"""
    return [True, s < 5, s not in (3, 4)]


def sixteen_rows(s):
    """every other row off from step 3 on"""
    return [s < 3 or r % 2 == 0 for r in range(16)]


def taken_positions(Ps, steps, active_of):
    """per row the indices of its input sequence that the schedule appends: the prompt, then index P + s - 1 at every active step s"""
    return [list(range(P)) + [P + s - 1 for s in range(1, steps) if active_of(s)[r]] for r, P in enumerate(Ps)]


@torch.no_grad()
def drive_batch(model, dev, xs, Ps, steps, active_of, room, final_norm=True):
    R, D = len(xs), xs[0].shape[1]
    cache = model.init_cache_batch(R, room, dev)
    got = [[model.prefill_row(xs[r][:P].to(dev)[None].contiguous(), cache, r, final_norm=final_norm)[0].float().cpu()]
           for r, P in enumerate(Ps)]
    for s in range(1, steps):
        act = active_of(s)
        x = torch.full((R, 1, D), float("nan"))
        for r, P in enumerate(Ps):
            if act[r]:
                x[r, 0] = xs[r][P + s - 1]
        h = model.forward_cached_batch(x.to(dev), cache, act, final_norm=final_norm).float().cpu()
        for r in range(R):
            if act[r]:
                got[r].append(h[r])
    return [torch.cat(g, 0) for g in got], list(cache["len"])


@torch.no_grad()
def drive_single(model, dev, x, P, taken, room):
    """one row through init_cache / forward_cached: the prompt in one call (a one-position prompt is a decode step), then one
    position per call"""
    cache = model.init_cache(room, dev)
    got = [model.forward_cached(x[:P].to(dev)[None].contiguous(), cache)[0].float().cpu()]
    for i in taken[P:]:
        got.append(model.forward_cached(x[i:i + 1].to(dev)[None].contiguous(), cache)[0].float().cpu())
    assert cache["len"] == len(taken)
    return torch.cat(got, 0)


@functools.lru_cache(maxsize=None)
def scripted_ref(case_id, fmt, Ps, steps, sched):
    """fp64 reference and yardstick of a scripted drive (computed once, read-only afterwards).  one[r]: the reference of row r
    driven alone, where it differs: a one-position prompt through forward_cached is a decode step and reads the e4m3 weights"""
    c = _CASE[case_id]
    active_of = three_rows if sched == "three" else sixteen_rows
    xs = go.scripted_rows(c, Ps, steps, tag=f"gen{len(Ps)}")
    taken = taken_positions(Ps, steps, active_of)
    rows = [dict(x=x[t], P=P) for x, t, P in zip(xs, taken, Ps)]
    W = weights(case_id, fmt)
    f64 = go.forward(c, W, rows)
    r = go.yardstick(go.forward(c, W, rows, "emu"), f64)
    one = {i: go.row_forward(c, W, dict(row, step_from=0)) for i, row in enumerate(rows) if fmt and row["P"] == 1}
    return dict(xs=xs, taken=taken, rows=rows, f64=f64, r=r, one=one)


def scripted_case(dev, tmp_path, c, fmt):
    key = ("A", c["id"], fmt)
    if key not in KEEP:
        ref = scripted_ref(c["id"], fmt, PS, T, "three")
        model = build(c, dev, tmp_path, fmt).base_model.model
        hid, lens = drive_batch(model, dev, ref["xs"], PS, T, three_rows, ROOM)
        pre, _ = drive_batch(model, dev, ref["xs"], PS, T, three_rows, ROOM, final_norm=False)
        one = [drive_single(model, dev, x, P, t, ROOM) for x, P, t in zip(ref["xs"], PS, ref["taken"])]
        KEEP[key] = dict(ref=ref, hidden=hid, pre=pre, one=one, lens=lens)
    return KEEP[key]


@pytest.mark.parametrize("fmt", go.FMTS, ids=go.fmt_id)
@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_scripted_cache_drive(dev, tmp_path, c, fmt):
    """three rows in a batch cache of 262 rows: prefill_row once per row (the one-position prompt is its n = 1 path), then 11 calls
    of forward_cached_batch under the schedule of three_rows.  Every returned hidden state, the prefill positions included, against
    the oracle of the positions that row actually appended; once more before the final norm; the rows one by one through
    init_cache / forward_cached."""
    k = scripted_case(dev, tmp_path, c, fmt)
    ref, r = k["ref"], k["ref"]["r"]
    assert [len(t) for t in ref["taken"]] == [1 + 11, 14 + 4, 250 + 9] == k["lens"]
    nk2 = {i + 1 for i in range(250, 259)}          # key counts of row 2's steps: 251 ... 259
    assert {256, 257} <= nk2
    SEEN.update(("Nk", n) for n in nk2)
    what = f"{c['id']} {go.fmt_id(fmt)}"
    hold(k["hidden"], go.pick(ref["f64"], "hidden"), r["hidden"], f"A batch hidden {what}", ("A", c["id"], fmt), P=PS)
    hold(k["pre"], go.pick(ref["f64"], "pre"), r["pre"], f"A batch pre-norm {what}", ("A", c["id"], fmt), P=PS)
    steps = max(go.ratios(x, o["hidden"])[P:].max().item() for x, o, P in zip(k["hidden"], ref["f64"], PS)) / r["hidden"]
    print(f"GEN A batch hidden, decode steps alone {what}: worst {steps:.2f} r")
    MEASURED[("A steps", c["id"], fmt)] = steps
    want = [ref["one"].get(i, o)["hidden"] for i, o in enumerate(ref["f64"])]
    hold(k["one"], want, r["hidden"], f"A single hidden {what}", ("A", c["id"], fmt), P=PS)
    SEEN.add((go.fmt_id(fmt), "cache", 3))


@pytest.mark.parametrize("fmt", go.FMTS, ids=go.fmt_id)
def test_scripted_cache_drive_sixteen_rows(dev, tmp_path, fmt):
    """R = 16 (the most a step takes), head dim 64, prompts of 1 + (5 r mod 37) positions, six frames, every other row off from
    step 3 on"""
    c = go.CASES[0]
    Ps = tuple(1 + (5 * r) % 37 for r in range(16))
    ref = scripted_ref(c["id"], fmt, Ps, 6, "sixteen")
    model = build(c, dev, tmp_path, fmt).base_model.model
    hid, lens = drive_batch(model, dev, ref["xs"], Ps, 6, sixteen_rows, 48)
    assert lens == [P + (5 if r % 2 == 0 else 2) for r, P in enumerate(Ps)]
    hold(hid, go.pick(ref["f64"], "hidden"), ref["r"]["hidden"], f"A sixteen rows hidden {c['id']} {go.fmt_id(fmt)}",
         ("A16", c["id"], fmt), P=Ps)
    SEEN.add((go.fmt_id(fmt), "cache", 16))


# ------------------------------------------------------------------------------------------------ B: infer / infer_batch end to end
def prompt_set(c, name):
    if name == "one":
        return go.ragged_prompts(c)[1:2]            # 9 ids + 5 latents
    if name == "single":
        return go.ragged_prompts(c)[0:1]            # a single id, no latents
    if name == "ragged3":
        return go.ragged_prompts(c)                 # P = 1 / 14 / 250: ids only, ids + latents
    return go.many_prompts(c, 17)                   # a group of 16 and a last group of one: `infer` with noise[:, 16:17]


def on_device(prompts, dev):
    return [(ids.to(dev), None if lat is None else lat[None].to(dev)) for ids, lat in prompts]


def generate(m, dev, prompts, head, frames, thres=-1.0, noise_seed=0, same_noise=False):
    """(latents per row [n_r, lat] fp32 on the CPU, the noise of every (row, frame) [R, frames, lat]).
    host: the fixed_noise idiom - every row of a group draws frame i's noise from the same tensor, a second group goes on in the
    iterator; device head: noise= [frames, R, lat], a draw of its own for every row (same_noise: one for all)"""
    R, lat, G = len(prompts), m.distribution_linear[2].weight.shape[0], m.infer_batch_rows
    gen = torch.Generator().manual_seed(noise_seed)
    ps = on_device(prompts, dev)
    if head == "host":
        draws = torch.randn((R + G - 1) // G * frames, lat, generator=gen)
        noise = torch.stack([draws[(r // G) * frames:(r // G + 1) * frames] for r in range(R)])
        fixed_noise(m, draws.view(-1, 1, 1, lat).to(dev))
        try:
            outs = m.infer_batch(ps, end_disp_kl_thres=thres, max_length=frames)
        finally:
            del m.sample
    else:
        noise = torch.randn(1 if same_noise else R, frames, lat, generator=gen).expand(R, frames, lat)
        kw = dict(end_disp_kl_thres=thres, max_length=frames, device_head=True, noise=noise.transpose(0, 1).contiguous().to(dev),
                  stop_lag=int(head[-1]))
        outs = [m.infer(ps[0][0], ps[0][1], **kw)] if R == 1 else m.infer_batch(ps, **kw)
    assert len(outs) == R
    for o in outs:
        assert o.shape[:2] == (1, lat) and o.dtype == torch.float32
    return [o[0].t().contiguous().cpu() for o in outs], noise


def step_from(prompts, G=16):
    """first position a decode step computed: a prompt generated alone (`infer`) goes through forward_cached, where a one-position
    prompt is a decode step; a group prefills through prefill_row (the bf16 layers at any length)"""
    n, out = len(prompts), []
    for r, (ids, lat) in enumerate(prompts):
        P = len(ids) + (0 if lat is None else lat.shape[0])
        alone = min(G, n - (r // G) * G) == 1
        out.append(0 if alone and P == 1 else P)
    return out


def teacher_check(c, fmt, prompts, lats, noise, what, key, frames=T):
    """the means recovered from the returned latents against the oracle teacher-forced on those latents; returns the reference"""
    assert all(l.shape == (frames - 1, c["lat"]) for l in lats), [tuple(l.shape) for l in lats]
    means = [l.double() - go.STD * n[:frames - 1].double() for l, n in zip(lats, noise)]
    rows = go.teacher_rows(prompts, lats, step_from(prompts) if fmt else None)
    W = weights(c["id"], fmt)
    f64 = go.forward(c, W, rows)
    emu = go.forward(c, W, rows, "emu")
    cut = lambda outs: [o["mean"][:-1] for o in outs]          # frame T - 1 is predicted but never returned
    r = go.worst(cut(emu), cut(f64))[0]
    Ps = [o["P"] for o in f64]
    hold(means, cut(f64), r, what, key, offsets=[P - 1 for P in Ps], P=Ps)
    return dict(rows=rows, f64=f64, r=r, means=means, cut=cut, Ps=Ps)


GRID = [(h, f, p) for h in range(3) for f in range(2) for p in range(4)]


@pytest.mark.parametrize("h,f,p", GRID, ids=[f"{HEADS[h]}-{go.fmt_id(go.FMTS[f])}-{PSETS[p]}" for h, f, p in GRID])
def test_infer_means_per_frame(dev, tmp_path, h, f, p):
    """every head x format x prompt set once, the three architectures in rotation (each meets every head, format and prompt
    set): 12 frames under fixed noise, the mean of every returned (row, frame) against the oracle"""
    c, head, fmt, pset = go.CASES[(h + f + p) % 3], HEADS[h], go.FMTS[f], PSETS[p]
    prompts = prompt_set(c, pset)
    m = build(c, dev, tmp_path, fmt)
    lats, noise = generate(m, dev, prompts, head, T, noise_seed=100 + 10 * h + p)
    what = f"B {head} {go.fmt_id(fmt)} {pset} {c['id']}"
    ref = teacher_check(c, fmt, prompts, lats, noise, what, ("B", c["id"], fmt))
    SEEN.add((go.fmt_id(fmt), head, len(prompts)))
    if (head, fmt, pset) == ("host", None, "ragged3"):
        KEEP[("B", c["id"])] = dict(ref=ref, c=c)


# ------------------------------------------------------------------------------------------------ C: the stop rule
@pytest.mark.parametrize("head", HEADS)
def test_stop_rule_against_fp64(dev, tmp_path, head):
    """the ragged three, free running (threshold -1), then with the threshold at the midpoint of the widest gap among the sorted
    fp64 frame KLs of frames i > 3 (teacher forced on the first run's latents).  An error of M r on a mean moves a frame's KL by at
    most gen_oracle.kl_allowance; every frame's KL must be farther from the threshold than that (gen_oracle.stop_plan's margin > 1),
    else the fp64 KLs do not decide the frame counts and the test FAILS: choose another seed.  Then the frame counts are those the
    fp64 KLs predict and every output is the first run's, truncated, bit for bit.  (A margin of 10 does not exist in this model
    family - DESIGN.md; tests/test_gen_oracle_cpu.py holds the free-running oracle's margin for this seed to 2.)"""
    c = go.CASES[STOP_CASE]
    prompts = go.ragged_prompts(c)
    m = build(c, dev, tmp_path)
    free, noise = generate(m, dev, prompts, head, T, noise_seed=STOP_SEED, same_noise=True)
    ref = teacher_check(c, None, prompts, free, noise, f"C {head} free run {c['id']}", ("C", c["id"], None))
    plan = go.stop_plan([o["kl"] for o in ref["f64"]], [go.kl_allowance(o["mean"], ref["r"]) for o in ref["f64"]])
    print(f"GEN C {head}: threshold {plan['thres']:.5f} gap half-width {plan['half']:.3e} largest allowance {plan['allowance']:.3e} "
          f"margin {plan['margin']:.2f} predicted frames {plan['counts']}")
    assert plan["margin"] > 1.0, (f"no frame-KL gap decides the stop: margin {plan['margin']:.2f} (half-width {plan['half']:.3e}, "
                                  f"allowance {plan['allowance']:.3e}); choose another STOP_SEED", plan)
    assert min(plan["counts"]) < T - 1, ("no row stops", plan)
    stopped, _ = generate(m, dev, prompts, head, T, thres=plan["thres"], noise_seed=STOP_SEED, same_noise=True)
    assert [len(s) for s in stopped] == plan["counts"], ([len(s) for s in stopped], plan)
    for a, b in zip(stopped, free):
        assert torch.equal(a, b[:len(a)])
    MEASURED[("C margin", head)] = plan["margin"]


# ------------------------------------------------------------------------------------------------ D: wrong references, coverage
def test_scripted_wrong_reference_is_caught(dev, tmp_path):
    """the device's hidden states of one scripted drive against three wrong oracles: all three fail the check"""
    c = go.CASES[0]
    k = scripted_case(dev, tmp_path, c, None)
    ref, r = k["ref"], k["ref"]["r"]["hidden"]
    good = go.pick(ref["f64"], "hidden")
    assert go.failure(k["hidden"], good, r) is None
    W = weights(c["id"], None)
    gap = [go.defect_forward(c, W, row, "position gap 1")["hidden"] for row in ref["rows"]]
    for label, wrong in (("position gap 1", gap), ("rows swapped", go.swap_rows(good, 0, 1, 4)),
                         ("frames shifted", go.shift_frames(good, 4))):
        msg = go.failure(k["hidden"], wrong, r, label, P=PS)
        print("GEN D scripted:", msg)
        assert msg is not None, label


def test_infer_wrong_reference_is_caught(dev, tmp_path):
    """the means of one infer_batch run (host head, bf16, the ragged three) against the same three wrong oracles"""
    c = go.CASES[(0 + 0 + 2) % 3]
    if ("B", c["id"]) not in KEEP:
        prompts = prompt_set(c, "ragged3")
        lats, noise = generate(build(c, dev, tmp_path), dev, prompts, "host", T, noise_seed=102)
        KEEP[("B", c["id"])] = dict(ref=teacher_check(c, None, prompts, lats, noise, "D rerun", ("B", c["id"], None)), c=c)
    ref = KEEP[("B", c["id"])]["ref"]
    good, r = ref["cut"](ref["f64"]), ref["r"]
    assert go.failure(ref["means"], good, r) is None
    W = weights(c["id"], None)
    gap = ref["cut"]([go.defect_forward(c, W, row, "position gap 1") for row in ref["rows"]])
    for label, wrong in (("position gap 1", gap), ("rows swapped", go.swap_rows(good, 0, 1, T - 1)),
                         ("frames shifted", go.shift_frames(good, T - 1))):
        msg = go.failure(ref["means"], wrong, r, label, offsets=[P - 1 for P in ref["Ps"]], P=ref["Ps"])
        print("GEN D infer:", msg)
        assert msg is not None, label


def test_every_combination_and_edge_was_seen():
    """whole file, one process, in order"""
    want = {(go.fmt_id(fmt), head, R) for fmt in go.FMTS for head in HEADS for R in (1, 3, 17)}
    want |= {(go.fmt_id(fmt), "cache", R) for fmt in go.FMTS for R in (3, 16)}
    want |= {("Nk", 256), ("Nk", 257)}
    for k in sorted(SEEN, key=str):
        print("GEN seen", k)
    assert want <= SEEN, sorted(want - SEEN, key=str)
    for k in sorted(MEASURED, key=str):
        print(f"GEN MEASURED {k}: {MEASURED[k]:.2f}")
