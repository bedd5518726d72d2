"""No GPU: the generation oracle of tests/gen_oracle.py on itself - the yardstick r, a heavier emulation inside M r at every position,
every seeded defect reported, the blindness of the fixture gains to a wrong rotary position, M r < 0.10 for the frame means, and the
margin of the stop-rule test's seed.  tests/test_generation_oracle_gpu.py holds the HIP path to the same check.

Measured values: DESIGN.md, "Generation per frame: the cached path against fp64"."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle as go  # noqa: E402

gs, gu, ko = go.gs, go.gu, go.ko
T = 12
PS = (1, 4, 14, 33, 250)          # prompt positions of the teacher-forced rows; the key-mask defects are seeded at P <= 33
_ID = lambda c: c["id"]
_CASE = {c["id"]: c for c in go.CASES}


@functools.lru_cache(maxsize=None)
def ref(case_id, fmt=None, gains="sensitive"):
    """teacher-forced rows (P of PS; the T - 1 latents fed back are what generation feeds: a free run of the fp64 oracle under a
    fixed noise) plus the three rows of the scripted cache drive; f64, emu, r"""
    c = _CASE[case_id]
    W = go.weights(c, go.make_state(c, gains), fmt)
    prompts = go.ragged_prompts(c, PS, tag="cpu")
    rows = go.teacher_rows(prompts, go.free_run(c, W, prompts, go.stop_noise(c, T - 1, c["seed"]), T - 1, "f64"))
    rows += [dict(x=x[:-1], P=P) for x, P in zip(go.scripted_rows(c, (1, 14, 250), T), (1, 14, 250))]
    f64, emu = go.forward(c, W, rows), go.forward(c, W, rows, "emu")
    return dict(c=c, W=W, rows=rows, f64=f64, emu=emu, r=go.yardstick(emu, f64))


@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_row_forward_is_the_oracles_llama_model(c):
    """without a defect the forward with its own positions and mask IS ko.llama_model, and the head is the one of ko.llasa_forward"""
    k = ref(c["id"])
    lc = gs.llasa_config(c)["llama"]
    row, out = k["rows"][2], k["f64"][2]
    m = ko._sub(k["W"], "base_model.model.")
    lat = torch.cat([row["prompt"], row["fed"]], 0).double()
    x = torch.cat([m["embed_tokens.weight"][row["ids"]], ko.linear(lat, k["W"]["audio_linear.weight"], k["W"]["audio_linear.bias"])], 0)
    hidden = ko.llama_model(m, lc, x[None], torch.ones(1, x.shape[0]))[0]
    assert out["L"] == 14 + T - 1 and out["P"] == 14
    torch.testing.assert_close(out["hidden"], hidden, rtol=1e-12, atol=1e-13)
    assert out["mean"].shape == (T, c["lat"]) and out["kl"].shape == (T,)
    h1 = ko.linear(hidden[13:], k["W"]["distribution_linear.0.weight"], k["W"]["distribution_linear.0.bias"])
    mean = ko.linear(torch.nn.functional.gelu(h1), k["W"]["distribution_linear.2.weight"], k["W"]["distribution_linear.2.bias"])
    torch.testing.assert_close(out["mean"], mean, rtol=1e-12, atol=1e-13)


def test_dequantised_weights_are_what_the_quantiser_stands_for():
    """(w, wq) pairs for the seven projections of every layer and nothing else; wq within half an e4m3 step of the bf16 weight"""
    c = go.CASES[0]
    W = go.weights(c, go.make_state(c), "e4m3")
    pairs = [k for k, v in W.items() if isinstance(v, tuple)]
    assert len(pairs) == 7 * c["layers"] and all(k.endswith(go.PROJ) for k in pairs)
    for k in pairs:
        w, wq = W[k]
        wb = w.to(torch.bfloat16).double()
        step = wb.abs().amax(1, keepdim=True) / 448.0
        # half a step of 2^-3 relative (three mantissa bits), or of the subnormal spacing 2^-9 scale near zero
        assert ((wq - wb).abs() <= torch.maximum(wb.abs() / 16.0, step * 2.0 ** -10) * (1 + 1e-6)).all(), k


@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_the_check_tells_e4m3_steps_from_bf16_steps(c):
    """the e4m3 reference is the bf16 one at every position a prefill computed (the prefill keeps the bf16 weights) and more than
    M r away from it at every decode step, r the yardstick of these rows as the scripted drive on the device takes it: a path that
    took the wrong weights for either kind of position would be reported.  A one-position prompt through forward_cached
    (step_from = 0) is a decode step itself."""
    k, kq = ref(c["id"]), ref(c["id"], "e4m3")
    rows = kq["rows"][5:]                                   # the scripted rows: the same inputs under both formats
    r = go.worst(go.pick(kq["emu"][5:], "hidden"), go.pick(kq["f64"][5:], "hidden"))[0]
    for row, spec in enumerate(rows):
        a, b, P = k["f64"][5 + row]["hidden"], kq["f64"][5 + row]["hidden"], spec["P"]
        assert torch.equal(a[:P], b[:P])
        q = go.ratios(b, a)[P:] / r
        print(f"GEN CPU {c['id']} P {P}: e4m3 steps against bf16 steps {q.min().item():.1f} ... {q.max().item():.1f} r")
        assert q.min() > go.M, (P, q.min().item())
    first = go.row_forward(c, kq["W"], dict(rows[0], step_from=0))["hidden"]
    assert go.ratios(first, k["f64"][5]["hidden"])[0] > go.M * r


@pytest.mark.parametrize("fmt", go.FMTS, ids=go.fmt_id)
@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_heavy_emulation_stays_within_M_r(c, fmt):
    """every linear output rounded to bf16 as well (about twice the rounding points): within M r at every row and position"""
    k = ref(c["id"], fmt)
    heavy = go.forward(c, k["W"], k["rows"], "heavy")
    for q in go.QUANTITIES:
        v, row, i = go.worst(go.pick(heavy, q), go.pick(k["f64"], q))
        print(f"GEN CPU {c['id']} {go.fmt_id(fmt)} {q}: r {k['r'][q]:.3e} heavy/r {v / k['r'][q]:.2f} (row {row} index {i})")
        assert go.failure(go.pick(heavy, q), go.pick(k["f64"], q), k["r"][q], f"heavy {q}") is None


@pytest.mark.parametrize("fmt", go.FMTS, ids=go.fmt_id)
@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_one_frame_x_110_is_always_reported(c, fmt):
    """M r < 0.10 for the frame means, so a frame whose mean is off by a tenth of its norm is reported wherever that norm is not
    below the floor"""
    k = ref(c["id"], fmt)
    assert go.M * k["r"]["mean"] < 0.10, (c["id"], fmt, k["r"]["mean"])
    good = go.pick(k["f64"], "mean")
    for row, x in enumerate(good):
        nrm = x.norm(dim=1)
        for i in range(1, T):            # the fed-back frames
            if nrm[i] >= 0.25 * nrm.pow(2).mean().sqrt():
                v, r_, i_ = go.worst(go.scale_frame(good, row, i), good)
                assert (r_, i_) == (row, i) and v > go.M * k["r"]["mean"], (row, i, v)


def reach(k, outs, q, row):
    """the largest ratio of a defective row against the reference, in units of r"""
    return go.worst([outs[q]], [k["f64"][row][q]])[0] / k["r"][q]


@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_seeded_defects_are_reported(c):
    k = ref(c["id"])
    r, f64 = k["r"], k["f64"]
    # through the forward's own positions and mask: a masked key at P <= 33, a gap of one rotary position at every P - at P = 250 on
    # the rows of the scripted drive (4 - 11 r); behind a 250-position TEXT prompt, whose embeddings are 1 / 16 the size of an audio
    # position's, the gap reaches 2.9 r on the architecture without rope scaling and 3.7 - 7 r on the others (printed)
    for row, spec in enumerate(k["rows"]):
        P = go.row_P(spec)
        for kind in go.FORWARD_DEFECTS:
            d = go.defect_forward(c, k["W"], spec, kind)
            assert torch.equal(d["hidden"][:P], f64[row]["hidden"][:P])               # the prompt positions are untouched
            rh, rm = reach(k, d, "hidden", row), reach(k, d, "mean", row)
            print(f"GEN CPU reach {c['id']} P {P} {kind}: hidden {rh:.1f} r, mean {rm:.1f} r")
            if P <= 33 or (kind == "position gap 1" and "x" in spec):
                assert max(rh, rm) > go.M, (kind, P, rh, rm)
                assert (go.failure([d["hidden"]], [f64[row]["hidden"]], r["hidden"])
                        or go.failure([d["mean"]], [f64[row]["mean"]], r["mean"])), (kind, P)
    # on the outputs: two rows swapped, one frame of one row x 1.10, frames shifted by one
    for q in ("hidden", "mean"):
        good = go.pick(f64, q)
        assert go.failure(good, good, r[q]) is None
        msg = go.failure(go.swap_rows(good, 1, 3, T), good, r[q], f"{c['id']} rows swapped {q}")
        assert msg is not None and ("row 1" in msg or "row 3" in msg), msg
        assert go.failure(go.shift_frames(good, T), good, r[q]) is not None
        row, i = 2, len(good[2]) - 5                                                  # a fed-back frame of the P = 14 row
        v, r_, i_ = go.worst(go.scale_frame(good, row, i), good)
        assert (r_, i_) == (row, i) and v > go.M * r[q], (q, v, r_, i_)
        msg = go.failure(go.scale_frame(good, row, i), good, r[q], c["id"], P=[go.row_P(s) for s in k["rows"]] if q == "hidden" else None)
        assert f"row {row} position {i}" in msg and "Nk" in msg and "ratio" in msg, msg


@pytest.mark.parametrize("c", go.CASES, ids=_ID)
def test_fixture_gains_do_not_show_a_wrong_rotary_position(c):
    """with the RMSNorm gains of golden_util.make_param (0.1 n) the normalised streams are x 0.1, the scores tiny and the softmax
    flat: a gap of one rotary position stays below M r at every position (in fact below r / 5) - the SAME defect the sensitive
    state shows at 2.9 r behind a 250-position text prompt and at 3.4 r and more everywhere else.  Do not swap the state back.
    (A masked key shows under both states while the keys are few - 30 r and more at P = 1, about 2 r at P = 33 with the fixture
    gains against 5 - 14 r with the sensitive ones - and under neither at P = 250, where it is 1 / 250 of the softmax mass.)"""
    fix, sen = ref(c["id"], None, "fixture"), ref(c["id"])
    for row, spec in enumerate(fix["rows"]):
        P = go.row_P(spec)
        for kind in go.FORWARD_DEFECTS:
            d = go.defect_forward(c, fix["W"], spec, kind)
            worst = max(reach(fix, d, "hidden", row), reach(fix, d, "mean", row))
            print(f"GEN CPU fixture gains {c['id']} P {P} {kind}: {worst:.2f} r")
            if kind == "position gap 1":
                ds = go.defect_forward(c, sen["W"], sen["rows"][row], kind)
                seen = max(reach(sen, ds, "hidden", row), reach(sen, ds, "mean", row))
                assert worst < 0.2 and seen > 2.5, (P, worst, seen)
                assert seen > go.M or (P == 250 and "ids" in spec), (P, seen)
            elif P >= 33:
                assert worst < go.M, (kind, worst)


def test_stop_seed_leaves_a_margin():
    """the free-running emu oracle under the stop test's fixed noise: the threshold at the midpoint of the widest gap of the fp64
    frame KLs (frames i > 3) is at least 2 allowances away from EVERY frame's KL - twice what the device test needs, for the drift
    between this free run and the device's - and rows stop at different frames.
    The issue asked for a gap half-width of 10 allowances.  It does not exist here: the allowance of a frame is what an error of
    M r |mean| does to |mean - 1|^2, about 2 M r ~ 10 % of the part of the KL that varies, and over noise seeds 0 .. 119 on the three
    architectures the half-width never exceeded 3.1 allowances (printed below for the chosen seed)."""
    c = go.CASES[go.STOP_CASE]
    W = go.weights(c, go.make_state(c))
    prompts = go.ragged_prompts(c)
    lats = go.free_run(c, W, prompts, go.stop_noise(c), go.STOP_FRAMES)
    rows = go.teacher_rows(prompts, [l[:-1] for l in lats])
    f64 = go.forward(c, W, rows)
    r = go.yardstick(go.forward(c, W, rows, "emu"), f64)["mean"]
    plan = go.stop_plan([o["kl"] for o in f64], [go.kl_allowance(o["mean"], r) for o in f64])
    print(f"GEN CPU stop: r {r:.3e} threshold {plan['thres']:.5f} half-width {plan['half']:.3e} largest allowance "
          f"{plan['allowance']:.3e} (ratio {plan['half'] / plan['allowance']:.2f}) margin {plan['margin']:.2f} frames {plan['counts']}")
    assert plan["margin"] >= 2.0, plan
    assert min(plan["counts"]) < max(plan["counts"]), plan
