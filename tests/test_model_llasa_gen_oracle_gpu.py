"""-m gpu: model.Llasa's KV-cached generation - infer, infer_batch with the host head, infer_batch with the device head at
stop_lag 0 and 1 - held frame by frame to the fp64 oracle of tests/gen_oracle2.py, by the method of
tests/test_generation_oracle_gpu.py (whose scripted cache drive already holds the shared decoder, position by position): every
disp = mean || log-scale of a returned frame, and the hidden state (host head) or the stream before the final norm (device head)
it was computed from, within M = 3 times a yardstick that comes from the reference alone.

The oracle is teacher forced on the latents the path itself produced: the sampled latent of every frame is captured where the
path hands it on (the host frame's return value / slot `frame` of the device head's plan), so each frame is compared on identical
inputs whatever the frames before it did.  Then the stop rule against the fp64 frame KLs, and wrong references that must fail."""
import functools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle2 as g2  # noqa: E402
from test_generation_oracle_gpu import on_device, step_from  # noqa: E402
from test_model_llasa_generation_gpu import _Tok, host_noise  # noqa: E402

go, gs = g2.go, g2.gs
T = 12
HEADS = ("host", "dev0", "dev1")          # the host head; device_head=True with stop_lag 0 and 1
PSETS = ("one", "single", "ragged3", "seventeen")
SEEN, KEEP, MEASURED = set(), {}, {}
_CASE = {c["id"]: c for c in g2.CASES}


@functools.lru_cache(maxsize=None)
def state(case_id):
    return g2.make_state(_CASE[case_id])


@functools.lru_cache(maxsize=None)
def weights(case_id, fmt):
    return go.weights(_CASE[case_id], state(case_id), fmt)


def build(c, dev, tmp_path, fmt=None):
    """model.Llasa on the attention-sensitive state, loaded under the reference's names"""
    from kalle_audio_amd.model import Llasa
    lc = gs.llasa_config(c)
    d = tmp_path / "llama2"
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


def prompt_set(c, name):
    if name == "one":
        return go.ragged_prompts(c)[1:2]            # 9 ids + 5 latents
    if name == "single":
        return go.ragged_prompts(c)[0:1]            # a single id, no latents
    if name == "ragged3":
        return go.ragged_prompts(c)                 # P = 1 / 14 / 250: ids only, ids + latents
    return go.many_prompts(c, 17)                   # a group of 16 and a last group of one: `infer`


def per_row(calls, sizes, counts, frames):
    """calls: the [R_g, w] tensors a path produced frame by frame, group after group; sizes: rows per group; counts[r]: frames
    wanted of row r -> per row [counts[r], w].  Several groups only ever run free here: `frames` calls each."""
    assert len(sizes) == 1 or len(calls) == frames * len(sizes), (len(calls), sizes)
    out, row = [], 0
    for g, n in enumerate(sizes):
        run = calls if len(sizes) == 1 else calls[g * frames:(g + 1) * frames]
        assert all(t.shape[0] == n for t in run)
        for j in range(n):
            assert len(run) >= counts[row + j], (len(run), counts[row + j])
            out.append(torch.stack([t[j] for t in run[:counts[row + j]]]).float().cpu())
        row += n
    return out


def generate(m, dev, prompts, head, frames, noise, thres=-1.0):
    """noise [frames, R, lat] on the CPU.  Returns per row (disp [n_r, 2 lat], the latents the path fed back [n_r, lat], what the
    head read [n_r, D]: the hidden state under the host head, the stream before the final norm under the device head), fp32 on
    the CPU, n_r the frames returned"""
    from kalle_audio_amd import ops
    R, lat, G = len(prompts), m.audio_linear.weight.shape[1], m.infer_batch_rows
    ps = on_device(prompts, dev)
    sizes = [min(G, R - g) for g in range(0, R, G)]
    fed, read = [], []
    if head == "host":
        real = m._host_frame

        def spy(hidden):
            out = real(hidden)
            read.append(hidden.reshape(hidden.shape[0], -1).clone())
            fed.append(out[1].reshape(out[1].shape[0], -1).clone())
            return out

        m._host_frame = spy
        feed = [noise[i, g:g + n].to(dev) for g, n in zip(range(0, R, G), sizes) for i in range(frames)]
        try:
            with host_noise(feed):
                outs = m.infer_batch(ps, end_disp_kl_thres=thres, max_length=frames)
        finally:
            del m._host_frame
    else:
        real = ops.llasa_frame_head2

        def spy(plan, h, nz, active=None, frame=0):
            out = real(plan, h, nz, active, frame=frame)
            read.append(h.clone())
            fed.append(out[1].clone())
            return out

        ops.llasa_frame_head2 = spy
        kw = dict(end_disp_kl_thres=thres, max_length=frames, device_head=True, noise=noise.to(dev), stop_lag=int(head[-1]))
        try:
            outs = [m.infer(ps[0][0], ps[0][1], **kw)] if R == 1 else m.infer_batch(ps, **kw)
        finally:
            ops.llasa_frame_head2 = real
    assert len(outs) == R
    for o in outs:
        assert o.shape[:2] == (1, 2 * lat) and o.dtype == torch.float32
    disp = [o[0].t().contiguous().cpu() for o in outs]
    counts = [len(d) for d in disp]
    return disp, per_row(fed, sizes, counts, frames), per_row(read, sizes, counts, frames)


def hold(xs, x64s, r, what, key, offsets=None, P=None):
    v, row, i = go.worst(xs, x64s)
    print(f"GEN2 {what}: worst ratio {v:.3e} = {v / r:.2f} r at row {row} index {i} (r {r:.3e}); {sum(len(x) for x in xs)} frames")
    MEASURED[key] = max(MEASURED.get(key, 0.0), v / r)
    msg = go.failure(xs, x64s, r, what, offsets, P)
    assert msg is None, msg


def teacher_check(c, fmt, prompts, head, disp, fed, read, what, key):
    """disp and what the head read, of every returned frame, against the oracle teacher forced on the latents the path fed back"""
    rows = go.teacher_rows(prompts, [f.double() for f in fed], step_from(prompts) if fmt else None)
    W = weights(c["id"], fmt)
    f64, emu = g2.forward(c, W, rows), g2.forward(c, W, rows, "emu")
    cut = lambda outs, q: [g2.frames_of(o, q)[:-1] for o in outs]       # the last frame is predicted but never returned
    Ps = [o["P"] for o in f64]
    off = [P - 1 for P in Ps]
    q = "hidden" if head == "host" else "pre"
    r = {k: go.worst(cut(emu, k), cut(f64, k))[0] for k in ("disp", q)}
    hold(disp, cut(f64, "disp"), r["disp"], f"{what} disp", key + ("disp",), offsets=off, P=Ps)
    hold(read, cut(f64, q), r[q], f"{what} {q}", key + (q,), offsets=off, P=Ps)
    return dict(rows=rows, f64=f64, r=r["disp"], disp=disp, cut=lambda outs: cut(outs, "disp"), Ps=Ps)


def draw(c, frames, R, seed):
    return torch.randn(frames, R, c["lat"], generator=torch.Generator().manual_seed(seed))


GRID = [(h, f, p) for h in range(3) for f in range(2) for p in range(4)]


@pytest.mark.parametrize("h,f,p", GRID, ids=[f"{HEADS[h]}-{g2.fmt_id(g2.FMTS[f])}-{PSETS[p]}" for h, f, p in GRID])
def test_infer_disp_per_frame(dev, tmp_path, h, f, p):
    """every head x format x prompt set once, the three architectures in rotation: 12 frames under fixed noise (a draw of its own
    for every row and frame), every returned (row, frame) against the oracle.  One prompt is `infer` itself (the one-row step);
    17 are a group of 16 and `infer`."""
    c, head, fmt, pset = g2.CASES[(h + f + p) % 3], HEADS[h], g2.FMTS[f], PSETS[p]
    prompts = prompt_set(c, pset)
    m = build(c, dev, tmp_path, fmt)
    disp, fed, read = generate(m, dev, prompts, head, T, draw(c, T, len(prompts), 200 + 10 * h + p))
    assert all(d.shape == (T - 1, 2 * c["lat"]) for d in disp)
    what = f"B {head} {g2.fmt_id(fmt)} {pset} {c['id']}"
    ref = teacher_check(c, fmt, prompts, head, disp, fed, read, what, ("B", g2.fmt_id(fmt)))
    SEEN.add((g2.fmt_id(fmt), head, len(prompts)))
    if (head, fmt, pset) == ("dev0", None, "ragged3"):
        KEEP["B"] = dict(ref=ref, c=c)


@pytest.mark.parametrize("head", HEADS)
def test_stop_rule_against_fp64(dev, tmp_path, head):
    """the stop test's three rows, free running (threshold -1), then with the threshold gen_oracle2.stop_plan chooses among the
    fp64 frame KLs (teacher forced on the first run's latents).  An error of M r on disp moves a frame's KL by at most
    gen_oracle2.kl_allowance; every KL the rule reads must be farther from the threshold than that (margin > 1), else the fp64
    KLs do not decide the frame counts and the test FAILS: choose another seed.  Then the frame counts are those the fp64 KLs
    predict and every output is the first run's, truncated, bit for bit."""
    c = g2.CASES[g2.STOP_CASE]
    prompts = g2.stop_prompts(c)
    m = build(c, dev, tmp_path)
    F = g2.STOP_FRAMES
    noise = g2.stop_noise(c)[:, None, :].expand(F, 3, c["lat"]).contiguous()
    disp, fed, read = generate(m, dev, prompts, head, F, noise)
    ref = teacher_check(c, None, prompts, head, disp, fed, read, f"C {head} free run {c['id']}", ("C", "bf16"))
    plan = g2.stop_plan([o["kl"] for o in ref["f64"]], [g2.kl_allowance(o["disp"], ref["r"]) for o in ref["f64"]])
    print(f"GEN2 C {head}: threshold {plan['thres']:.5f} margin {plan['margin']:.2f} over {plan['read']} frames read, predicted "
          f"frames {plan['counts']}")
    assert plan["margin"] > 1.0, (f"no frame-KL gap decides the stop: margin {plan['margin']:.2f}; choose another STOP_SEED", plan)
    assert min(plan["counts"]) < max(plan["counts"]), ("the rows stop together", plan)
    stopped, _, _ = generate(m, dev, prompts, head, F, noise, thres=plan["thres"])
    assert [len(s) for s in stopped] == plan["counts"], ([len(s) for s in stopped], plan)
    for a, b in zip(stopped, disp):
        assert torch.equal(a, b[:len(a)])
    MEASURED[("C margin", head)] = plan["margin"]


def test_wrong_references_are_caught(dev, tmp_path):
    """the disp rows of one infer_batch run (device head, bf16, the ragged three) against wrong oracles: teacher forced on a
    feedback drawn with the fixed std, the halves swapped, frames shifted by one, two rows swapped, a gap of one rotary position"""
    if "B" not in KEEP:
        c = g2.CASES[(1 + 0 + 2) % 3]
        prompts = prompt_set(c, "ragged3")
        out = generate(build(c, dev, tmp_path), dev, prompts, "dev0", T, draw(c, T, 3, 212))
        KEEP["B"] = dict(ref=teacher_check(c, None, prompts, "dev0", *out, "D rerun", ("B", "bf16")), c=c)
    ref, c = KEEP["B"]["ref"], KEEP["B"]["c"]
    good, r = ref["cut"](ref["f64"]), ref["r"]
    assert go.failure(ref["disp"], good, r) is None
    W = weights(c["id"], None)
    noise = draw(c, T, 3, 212)
    fixed = [g2.sample(d.double(), noise[:len(d), row], "fixed_std") for row, d in enumerate(ref["disp"])]
    rows = [dict(row, fed=f) for row, f in zip(ref["rows"], fixed)]
    wrongs = (("fixed-std feedback", ref["cut"](g2.forward(c, W, rows))), ("halves swapped", g2.swap_halves(good)),
              ("frames shifted", go.shift_frames(good, T - 1)), ("rows swapped", go.swap_rows(good, 0, 1, T - 1)),
              ("position gap 1", ref["cut"]([g2.defect_forward(c, W, row, "position gap 1") for row in ref["rows"]])))
    for label, wrong in wrongs:
        msg = go.failure(ref["disp"], wrong, r, label, offsets=[P - 1 for P in ref["Ps"]], P=ref["Ps"])
        print("GEN2 D:", msg)
        assert msg is not None, label


def test_every_combination_was_seen():
    """whole file, one process, in order"""
    want = {(g2.fmt_id(fmt), head, R) for fmt in g2.FMTS for head in HEADS for R in (1, 3, 17)}
    assert want <= SEEN, sorted(want - SEEN, key=str)
    for k in sorted(MEASURED, key=str):
        print(f"GEN2 MEASURED {k}: {MEASURED[k]:.2f}")
