"""The localised gradient check of tests/grad_slices.py on the reference alone (CPU, no kernel runs): the oracle in fp64, the
yardstick on every case tests/test_grad_slices_gpu.py uses, and the seeded defects a whole-tensor norm cannot see.

Measured here (max over the cases): fp32 vs fp64 oracle 1.6e-6 rel-L2 per gradient tensor; yardstick r(p) median 5.8e-3 ... 1.3e-2,
per-parameter range 3e-4 ... 3.5e-2 (4.1e-2: the k-LayerNorm biases of the qk_norm="ln" case), token rows of the input gradients
at most 2.6e-2; the heavier emulation reaches 1.98 r(p) (pre_norm.gamma of block 0 in one case; median 1.0-1.2), so M = 3 holds
on every case; the weakest seeded defect (one token row of the x_t gradient x 1.10 where r = 2.6e-2) reaches 3.85 r(p)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_slices as gs  # noqa: E402

gu, ko = gs.gu, gs.ko

# (kind, case, micro-batch seeds, names checked (None: all)) of everything the GPU file runs
_frozen_names = lambda fc: [n for n, _ in gs.dit_shapes(fc["base"]) if not gs.FROZEN_SETS[fc["frozen"]](n)]
WINDOWS = ([("dit", c, [c["seed"]], None, c["id"]) for c in gs.DIT_CASES] +
           [("dit", tc["base"], gs.window_seeds(tc, w), None, f"{tc['id']}-w{w}") for tc in gs.TRAINER_CASES for w in (0, 1)] +
           [("dit", fc["base"], [fc["base"]["seed"]], _frozen_names(fc), fc["id"]) for fc in gs.FROZEN_CASES] +
           [("llasa", c, None, None, c["id"]) for c in gs.LLASA_CASES])


@functools.lru_cache(maxsize=None)
def bundle(i):
    """the three oracle runs of WINDOWS[i], computed once and shared: fp64 (with the per-token rows of the bias the defect test
    uses), the bf16-operand emulation -> r(p), the heavier emulation"""
    kind, c, seeds, _, _ = WINDOWS[i]
    if kind == "dit":
        st = gu.make_state(gs.dit_shapes(c), c["seed"])
        sites = gs.dit_defect_sites(c)
        run = lambda mode, **kw: gs.dit_window(c, st, seeds, mode, **kw)
        layout_of = gs.dit_layout
    else:
        st = gu.make_state(gs.llasa_shapes(c), c["seed"])
        sites = gs.llasa_defect_sites(c)
        batch, eps = gs.llasa_inputs(c)
        run = lambda mode, **kw: gs.llasa_reference(c, st, batch, eps, mode, **kw)
        layout_of = gs.llasa_layout
    g64 = run("f64", bias_rows=sites["bias"] if kind == "llasa" or len(seeds) == 1 else None)
    layout = layout_of(c, g64)
    r, raw = gs.yardstick(run("emu"), g64, layout)
    return dict(g64=g64, layout=layout, r=r, raw=raw, heavy=run("heavy"), sites=sites, run=run)


def test_slices_respect_chunks_and_tails():
    assert gs.bounds(40) == [(0, 16), (16, 32), (32, 40)]
    assert gs.bounds(3, 1) == [(0, 1), (1, 2), (2, 3)]
    # six adaLN chunks of 24 rows: every chunk is 16 + 8, no run crosses a multiple of 24
    b = gs.bounds(144, 16, 24)
    assert len(b) == 12 and all(a // 24 == (e - 1) // 24 for a, e in b) and b[:2] == [(0, 16), (16, 24)]
    assert [e - a for a, e in gs.bounds(448 * 2, 16, 448)].count(16) == 56
    # q | k | v of a GQA projection under HF names, heads of 128 rows
    assert gs.llama_chunk("x.self_attn.k_proj.weight", (128, 256), 128) == 128 and gs.llama_chunk("x.mlp.up_proj.weight", (192, 256), 128) is None
    assert gs.dit_chunk("l.to_scale_shift_gate.1.weight", (768, 128), 64) == 128 and gs.dit_chunk("l.ff.ff.0.proj.bias", (1024,), 64) == 512
    # the scale's floor: a silent slice still has a unit; a vector is [n, 1]
    ref = torch.zeros(32, 4, dtype=torch.float64)
    ref[:16] = 1.0
    sc = gs.slice_scale(ref, gs.bounds(32))
    assert sc[0].item() == 8.0 and abs(sc[1].item() - 0.25 * 8.0 * 0.5 ** 0.5) < 1e-12
    assert gs.view2d(torch.zeros(5)).shape == (5, 1)


@pytest.mark.parametrize("i", [1, len(WINDOWS) - 3], ids=lambda i: WINDOWS[i][4])
def test_oracle_fp32_and_fp64_agree(i):
    """dtype-preserving oracle: the same case in fp32 and in fp64 gives the same gradients to 1e-5 rel-L2 per tensor
    (measured 4e-7 ... 1.6e-6), and the fp64 run is fp64 throughout"""
    b = bundle(i)
    g32 = b["run"]("f64", dtype=torch.float32)
    for n in b["layout"]:
        assert b["g64"][n].dtype == torch.float64 and g32[n].dtype == torch.float32, n
        assert gs.rel_l2(g32[n], b["g64"][n]) <= 1e-5, (n, gs.rel_l2(g32[n], b["g64"][n]))


@pytest.mark.parametrize("i", range(len(WINDOWS)), ids=lambda i: WINDOWS[i][4])
def test_heavier_emulation_passes_at_m3(i):
    """the cases are fair: a path with about twice the rounding points of the yardstick's emulation stays inside M r(p) scale on
    every slice of every gradient (and of the output and the input gradients, per token row)"""
    b = bundle(i)
    names = WINDOWS[i][3]
    rho = gs.check(b["heavy"], b["g64"], b["r"], b["layout"], names)
    print("worst", gs.worst(rho), "median r", sorted(b["raw"].values())[len(b["raw"]) // 2])
    assert not gs.failures(rho), gs.failures(rho)
    assert len(rho) == (len(names) if names is not None else len(b["layout"]))
    # a frozen subset keeps at least one fused parameter or vector to check
    assert any(len(b["layout"][n]) > 1 for n in rho)
    # the reach of the per-token check: a row that is not below the floor and is 10 % wrong exceeds M r(p) in EVERY input gradient
    for n in b["layout"]:
        if n.startswith("act:d_") or n == "act:pre_mean":
            assert gs.M * b["r"][n] < 0.10, (n, b["r"][n])


_DEFECT_WINDOWS = [i for i, w in enumerate(WINDOWS) if w[3] is None]       # (the frozen subsets: tests/test_grad_slices_gpu.py)


@pytest.mark.parametrize("i", _DEFECT_WINDOWS, ids=lambda i: WINDOWS[i][4])
def test_seeded_defects_fail(i):
    """each defect, applied to the heavier emulation (which passes), is reported - in the tensor it was put into and at M = 3.
    The token row goes into the gradient of x_t AND into that of the context; an accumulation window of several micro-batches
    has no activations and keeps no per-token rows, so it carries the parameter defects only.  The tail-slice defect passes the configuration fuzz tests' whole-tensor rule (4e-2 of the tensor's norm): that is the gap."""
    b = bundle(i)
    g64, sites = b["g64"], b["sites"]
    defects = gs.seeded_defects(b["heavy"], b["layout"], sites, g64.get("rows:" + sites["bias"]))
    window = WINDOWS[i][2] is not None and len(WINDOWS[i][2]) > 1
    assert len(defects) == (3 if window else 6 if WINDOWS[i][0] == "dit" else 5) + bool(sites["adaln"])
    assert window or "act:d_xt" in [n for _, n, _ in defects] or WINDOWS[i][0] == "llasa"
    for label, n, gd in defects:
        rho = gs.check(gd, g64, b["r"], b["layout"], [n])
        print(f"{label:48s} {n:52s} rho {rho[n][0]:.2f} rows {rho[n][1]}")
        assert gs.failures(rho), (label, n, rho[n])
        if label.startswith("tail slice"):
            assert gs.old_rule_passes(gd, g64, n), n
            assert rho[n][1] == b["layout"][n][-1]               # and it is the tail slice that is named


def test_some_case_carries_the_adaln_defect():
    assert sum(1 for c in gs.DIT_CASES if gs.dit_defect_sites(c)["adaln"]) >= 2
