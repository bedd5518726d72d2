"""No GPU: the generation oracle of tests/gen_oracle2.py (model.Llasa, mean || log-scale head) on itself - the yardstick r per
quantity, a heavier emulation inside M r at every frame, the seeded defects of this head reported (a feedback drawn with the
fixed std of the other class, the two halves swapped, frames shifted by one, two rows swapped, one frame x 1.10), the KL allowance
against brute force, and the margin of the stop-rule test's seed.  tests/test_model_llasa_gen_oracle_gpu.py holds the HIP path to
the same check.  The decoder-side defects (rotary positions, masked keys, e4m3 positions) are head-agnostic and stay with
tests/test_gen_oracle_cpu.py."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle2 as g2  # noqa: E402
import llasa_head2_refs as hr2  # noqa: E402

go = g2.go
T = 12
PS = (1, 14, 33)                  # prompt positions of the teacher-forced rows (the 250-position prompt is the GPU file's)
_ID = lambda c: c["id"]
_CASE = {c["id"]: c for c in g2.CASES}
cut = lambda outs, q: [g2.frames_of(o, q)[:-1] for o in outs]      # frame T - 1 is predicted but never returned


@functools.lru_cache(maxsize=None)
def ref(case_id, fmt=None):
    """teacher-forced rows on the latents a free run of the fp64 oracle feeds back under a fixed noise; f64, emu, r"""
    c = _CASE[case_id]
    W = go.weights(c, g2.make_state(c), fmt)
    prompts = go.ragged_prompts(c, PS, tag="cpu2")
    noise = g2.stop_noise(c, T - 1, c["seed"])
    rows = go.teacher_rows(prompts, g2.free_run(c, W, prompts, noise, T - 1, "f64"))
    f64, emu = g2.forward(c, W, rows), g2.forward(c, W, rows, "emu")
    return dict(c=c, W=W, prompts=prompts, noise=noise, rows=rows, f64=f64, emu=emu, r=g2.yardstick(emu, f64))


@pytest.mark.parametrize("c", g2.CASES, ids=_ID)
def test_row_forward_reads_the_head_as_mean_and_log_scale(c):
    k = ref(c["id"])
    row, out = k["rows"][1], k["f64"][1]
    assert out["L"] == 14 + T - 1 and out["P"] == 14
    assert out["disp"].shape == (T, 2 * c["lat"]) and out["kl"].shape == (T,)
    W = k["W"]
    h1 = go.ko.linear(out["hidden"][13:], W["distribution_linear.0.weight"], W["distribution_linear.0.bias"])
    disp = go.ko.linear(torch.nn.functional.gelu(h1), W["distribution_linear.2.weight"], W["distribution_linear.2.bias"])
    torch.testing.assert_close(out["disp"], disp, rtol=1e-12, atol=1e-13)
    mean, logs = hr2.halves(disp)
    from torch.distributions import Normal, kl_divergence
    one, e = torch.tensor(1.0, dtype=torch.float64), torch.tensor(torch.e, dtype=torch.float64)
    torch.testing.assert_close(out["kl"], kl_divergence(Normal(mean, logs.exp()), Normal(one, e)).mean(-1), rtol=1e-12, atol=1e-13)
    # the free run fed back mean + exp(logs) noise: frame i's latent is position P + i of the row
    for i in range(T - 1):
        torch.testing.assert_close(row["fed"][i], g2.sample(out["disp"][i], k["noise"][i]), rtol=0, atol=1e-6)
    # the state is gen_oracle's but for the head
    a, b = go.make_state(c), g2.make_state(c)
    assert set(a) == set(b)
    moved = sorted(n for n in a if a[n].shape != b[n].shape)
    assert moved == ["distribution_linear.0.bias", "distribution_linear.0.weight", "distribution_linear.2.bias", "distribution_linear.2.weight"]
    assert all((a[n] == b[n]).all() for n in a if n not in moved)


@pytest.mark.parametrize("fmt", g2.FMTS, ids=g2.fmt_id)
@pytest.mark.parametrize("c", g2.CASES, ids=_ID)
def test_heavy_emulation_stays_within_M_r(c, fmt):
    """every linear output rounded to bf16 as well (about twice the rounding points): within M r at every row and frame, and
    M r < 0.10 for disp, so a frame off by a tenth of its norm is reported"""
    k = ref(c["id"], fmt)
    heavy = g2.forward(c, k["W"], k["rows"], "heavy")
    for q in g2.QUANTITIES:
        v, row, i = go.worst(cut(heavy, q), cut(k["f64"], q))
        print(f"GEN2 CPU {c['id']} {g2.fmt_id(fmt)} {q}: r {k['r'][q]:.3e} heavy/r {v / k['r'][q]:.2f} (row {row} frame {i})")
        assert go.failure(cut(heavy, q), cut(k["f64"], q), k["r"][q], f"heavy {q}") is None
    assert go.M * k["r"]["disp"] < 0.10, (c["id"], fmt, k["r"]["disp"])


@pytest.mark.parametrize("c", g2.CASES, ids=_ID)
def test_seeded_defects_are_reported(c):
    k = ref(c["id"])
    r, f64 = k["r"], k["f64"]
    good = cut(f64, "disp")
    assert go.failure(good, good, r["disp"]) is None
    # the feedback drawn with the fixed std of the other class: the reference teacher forced on THOSE latents
    fixed = go.teacher_rows(k["prompts"], g2.free_run(c, k["W"], k["prompts"], k["noise"], T - 1, "f64", wrong="fixed_std"))
    bad = cut(g2.forward(c, k["W"], fixed), "disp")
    for row in range(len(PS)):
        assert torch.equal(bad[row][0], good[row][0])                       # frame 0 has seen no feedback yet
    msg = go.failure(good, bad, r["disp"], f"{c['id']} fixed-std feedback")
    print("GEN2 CPU", msg)
    assert msg is not None
    for q in ("pre", "hidden"):
        assert go.failure(cut(f64, q), cut(g2.forward(c, k["W"], fixed), q), r[q]) is not None, q
    # on the outputs
    for label, wrong in (("halves swapped", g2.swap_halves(good)), ("frames shifted", go.shift_frames(good, T - 1)),
                         ("rows swapped", go.swap_rows(good, 0, 2, T - 1))):
        msg = go.failure(good, wrong, r["disp"], f"{c['id']} {label}")
        print("GEN2 CPU", msg)
        assert msg is not None, label
    row, i = 1, T - 5
    v, r_, i_ = go.worst(go.scale_frame(good, row, i), good)
    assert (r_, i_) == (row, i) and v > go.M * r["disp"], (v, r_, i_)


def test_kl_allowance_bounds_what_an_error_of_that_size_does():
    """random and adversarial error vectors of norm d = M r max(|disp|, floor) on the reference disp: the frame KL never moves by
    more than the allowance, and the adversarial direction (the KL's own gradient) uses a good part of it"""
    c = g2.CASES[0]
    k = ref(c["id"])
    r = k["r"]["disp"]
    g = torch.Generator().manual_seed(0)
    used = 0.0
    for o in k["f64"]:
        x = o["disp"]
        allow = g2.kl_allowance(x, r)
        nrm = x.norm(dim=1)
        d = go.M * r * torch.maximum(nrm, 0.25 * nrm.pow(2).mean().sqrt())
        xg = x.clone().requires_grad_(True)
        hr2.kl(xg).sum().backward()
        dirs = [xg.grad, -xg.grad] + [torch.randn(x.shape, generator=g, dtype=torch.float64) for _ in range(8)]
        for v in dirs:
            moved = (hr2.kl(x + v / v.norm(dim=1, keepdim=True) * d[:, None]) - o["kl"]).abs()
            assert (moved <= allow).all(), (moved / allow).max()
            used = max(used, float((moved / allow).max()))
    print(f"GEN2 CPU kl_allowance: the worst direction tried uses {used:.2f} of it")
    assert used > 0.3


def test_stop_seed_leaves_a_margin():
    """the free-running emu oracle under the stop test's fixed noise: the threshold gen_oracle2.stop_plan chooses among the fp64
    frame KLs (frames i > 3) is farther than MARGIN allowances from the KL of every frame the rule reads, and rows stop at
    different frames"""
    c = g2.CASES[g2.STOP_CASE]
    W = go.weights(c, g2.make_state(c))
    prompts = g2.stop_prompts(c)
    lats = g2.free_run(c, W, prompts, g2.stop_noise(c), g2.STOP_FRAMES)
    rows = go.teacher_rows(prompts, [l[:-1] for l in lats])
    f64 = g2.forward(c, W, rows)
    r = g2.yardstick(g2.forward(c, W, rows, "emu"), f64)["disp"]
    plan = g2.stop_plan([o["kl"] for o in f64], [g2.kl_allowance(o["disp"], r) for o in f64])
    print(f"GEN2 CPU stop: r {r:.3e} threshold {plan['thres']:.5f} margin {plan['margin']:.2f} over {plan['read']} frames read, "
          f"frames returned {plan['counts']}")
    assert plan["margin"] >= MARGIN, plan
    assert min(plan["counts"]) < max(plan["counts"]), plan


MARGIN = 2.0        # twice what the device test needs, for the drift between this free run and the device's
