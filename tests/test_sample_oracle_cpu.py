"""No GPU: the sampling oracle of tests/sample_oracle.py on itself - guided() is ko.dit_forward, the free run is ko.sample_ddim /
ko.sample_euler, the yardstick r per case and step, a heavier emulation inside M r, every seeded defect reported or asserted blind
(BLIND, with the conditions the list has to meet), the update allowances against the oracle's own fp32-coefficient samplers.
tests/test_sampling_oracle_gpu.py holds the HIP path to the same check.

Measured values: DESIGN.md, "Sampling per step"."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_oracle as so  # noqa: E402

gs, ko = so.gs, so.ko
ALL = so.CASES + so.SINGLE
_ID = lambda k: k["id"]


@functools.lru_cache(maxsize=None)
def ref(case_id):
    return so.reference(so.BY_ID[case_id])


def reach(k, defect):
    return _reach(k["id"], defect)


@functools.lru_cache(maxsize=None)
def _reach(case_id, defect):
    """(largest ratio / (M r), step, row, ratio) of the reference with `defect` against the reference, on the fp64 free run"""
    k, R = so.BY_ID[case_id], ref(case_id)
    tr = R["traj"]
    return so.worst(so.outputs(k, R["W"], R["inp"], tr["xs"], tr["ts"], "f64", defect), tr["outs"], R["r"])


def test_the_cases_are_the_ones_the_paths_need():
    """one, two and three key blocks, 2B of 2, 4 and 6, both conditioning types, both objectives, every production path"""
    assert [k["id"] for k in so.CASES] == [f"G{i}" for i in range(1, 8)]
    assert {2 * k["B"] for k in so.CASES if k["cfg"] != 1.0} == {2, 4, 6}
    assert {so.base(k)["S"] for k in so.CASES} == {7, 130, 200} and {so.base(k)["T"] for k in so.CASES} == {33, 125, 257}
    assert {(so.base(k)["gtype"], k["obj"]) for k in so.CASES} >= {("prepend", "v"), ("adaLN", "rectified_flow"), ("prepend", "rectified_flow")}
    assert {k["path"] for k in so.CASES} == {(True, True), (True, False), (False, False)}
    assert all(k["steps"] >= 4 for k in so.CASES)          # (generate_diffusion_cond replays a graph from four steps on)
    assert {so.base(k)["gtype"] for k in so.SINGLE if k["prepend"]} == {"prepend", "adaLN"}


@pytest.mark.parametrize("k", ALL, ids=_ID)
def test_guided_is_the_oracles_dit_forward(k):
    """without a defect the restated guidance arithmetic IS ko.dit_forward, bit for bit, in both modes"""
    R = ref(k["id"])
    inp, x, t = R["inp"], R["traj"]["xs"][0], R["traj"]["ts"][0]
    d = lambda n: None if inp[n] is None else inp[n].double()
    tt = torch.ones(k["B"], dtype=torch.float64) * float(t)
    for mode in ("f64", "emu"):
        with gs.MODES[mode](), torch.no_grad():
            want = ko.dit_forward(R["W"], so.oracle_cfg(k), x, tt, cross_attn_cond=d("ctx"), negative_cross_attn_cond=d("neg"),
                                  negative_cross_attn_mask=inp["negm"], global_embed=d("gl"), prepend_cond=d("prepend"),
                                  prepend_cond_mask=inp["prepend_mask"], cfg_scale=k["cfg"], scale_phi=k["phi"])
        assert torch.equal(so.model_out(k, R["W"], inp, x, tt, mode), want), mode
        if mode == "f64":
            assert torch.equal(gs.rows_bct(want), R["traj"]["outs"][0])
    assert R["traj"]["outs"][0].shape == (k["B"] * so.tokens(k), gs.CIO)


@pytest.mark.parametrize("k", so.CASES, ids=_ID)
def test_free_run_is_the_oracles_sampler(k):
    """the recorded trajectory ends where ko.sample_ddim / ko.sample_euler end on the same function; its t_i are the sampler's fp32
    linspace; and update() - fp64 coefficients from the fp32 schedule - reproduces every recorded x_{i+1} and the returned tensor
    inside its allowance, although the oracle's samplers compute their coefficients (and, for v, round the model output) in fp32:
    the allowance covers exactly that"""
    R = ref(k["id"])
    tr, inp = R["traj"], R["inp"]
    fn = lambda x, t: so.model_out(k, R["W"], inp, x, t)
    x0, tol0 = so.start(k, inp)
    final = ko.sample_ddim(fn, x0, k["steps"]) if k["obj"] == "v" else ko.sample_euler(fn, x0, k["steps"], k["sigma_max"])
    assert torch.equal(final, tr["final"]) and final.dtype == torch.float64
    assert len(tr["xs"]) == k["steps"] and torch.equal(tr["xs"][0], x0)
    assert torch.equal(torch.stack(tr["ts"]), so.schedule(k)[:-1]) and tr["ts"][0].dtype == torch.float32
    assert float(tr["ts"][0]) == float(torch.tensor(k["sigma_max"] if k["obj"] == "rectified_flow" else 1.0, dtype=torch.float32))
    B, T = k["B"], so.base(k)["T"]
    for i in range(k["steps"]):
        out = tr["outs"][i].reshape(B, T, gs.CIO).transpose(1, 2)
        u = so.update(k, i, tr["xs"][i], out)
        last = i == k["steps"] - 1
        if not last:
            assert so.over(tr["xs"][i + 1], u["next"], u["next_tol"]) <= 0, (i, so.over(tr["xs"][i + 1], u["next"], u["next_tol"]))
            if k["obj"] == "v":      # (fp32 cos and sin: the allowance is in use, not idle; Euler's dt is exact on these schedules)
                assert (tr["xs"][i + 1] != u["next"]).any()
        else:
            assert so.over(final, u["ret"], u["ret_tol"]) <= 0, so.over(final, u["ret"], u["ret_tol"])
        # ... and the allowance is the size of fp32 rounding: a relative 2^-17 of |x| + |out| at the most
        assert (u["next_tol"] <= 2.0 ** -17 * (tr["xs"][i].abs() + out.abs()) + 1e-300).all()


@pytest.mark.parametrize("k", ALL, ids=_ID)
def test_yardstick_and_heavy_emulation(k):
    """r(case, step) exists, is finite and leaves room to see a row that is a tenth off (M r < 0.10); about twice the rounding
    points (every linear output rounded as well) stay within M r at every row of every step"""
    R = ref(k["id"])
    tr = R["traj"]
    assert len(R["r"]) == max(k["steps"], 1)
    assert all(math.isfinite(r) and 0 < r and so.M * r < 0.10 for r in R["r"]), R["r"]
    heavy = so.outputs(k, R["W"], R["inp"], tr["xs"], tr["ts"], "heavy")
    w = so.worst(heavy, tr["outs"], R["r"])
    print(f"SAMPLING CPU {k['id']}: r " + " ".join(f"{r:.3e}" for r in R["r"]) + f"; heavy {w[0] * so.M:.2f} r (step {w[1]} row {w[2]})")
    assert so.failure(heavy, tr["outs"], R["r"], "heavy") is None
    assert so.failure(tr["outs"], tr["outs"], R["r"]) is None


@pytest.mark.parametrize("k", ALL, ids=_ID)
def test_seeded_defects_are_reported_or_listed_blind(k):
    R = ref(k["id"])
    tr = R["traj"]
    assert so.defects_of(k, so.MODEL_DEFECTS), k["id"]
    for d in so.defects_of(k, so.MODEL_DEFECTS):
        v, step, row, q = reach(k, d)
        blind = (k["id"], d) in so.BLIND
        print(f"SAMPLING CPU reach {k['id']} {d}: {v:.3f} M r (step {step} row {row}, ratio {q:.3e})" + (" BLIND" if blind else ""))
        if blind:       # (a change of state that un-blinds the pair is noticed here: take it off the list then)
            assert v <= 1.0, (k["id"], d, v)
        else:
            assert v > 1.0, (k["id"], d, v)
            msg = so.failure(so.outputs(k, R["W"], R["inp"], tr["xs"], tr["ts"], "f64", d), tr["outs"], R["r"], k["id"])
            assert msg is not None and "step" in msg and "row" in msg, msg
    # the update defects, against the element-wise allowance
    B, T = k["B"], so.base(k)["T"]
    for d in so.defects_of(k, so.UPDATE_DEFECTS):
        seen = 0
        for i in range(k["steps"]):
            out = tr["outs"][i].reshape(B, T, gs.CIO).transpose(1, 2)
            good, bad = so.update(k, i, tr["xs"][i], out), so.update(k, i, tr["xs"][i], out, d)
            if good["next"] is not None:
                assert so.over(good["next"], bad["next"], bad["next_tol"]) > 0, (d, i)
                seen += 1
        assert seen >= k["steps"] - 1
    assert len(so.defects_of(k, so.UPDATE_DEFECTS)) == (1 if k["steps"] else 0)


def test_the_blind_list_meets_its_conditions():
    """every listed pair is a real (case, defect) pair that applies; no case has more than two; every defect is reported in at
    least one prepend and one adaLN case where it applies to one"""
    for cid, d in so.BLIND:
        assert d in so.MODEL_DEFECTS and so.applies(so.BY_ID[cid], d), (cid, d)
    for k in ALL:
        assert sum(1 for cid, _ in so.BLIND if cid == k["id"]) <= 2, k["id"]
    for d in so.MODEL_DEFECTS:
        for prepend in (True, False):
            cases = [k for k in ALL if so.applies(k, d) and so.is_prepend(k) == prepend]
            if d == "prepended token not skipped" and not prepend:
                assert not cases          # (adaLN puts no token in front, and cuts a prepended conditioning not off again: tokens())
                continue
            if d.startswith("negative") and prepend:
                assert not cases          # (the negative prompt is G2's, an adaLN model)
                continue
            assert cases, (d, prepend)
            seen = [k["id"] for k in cases if (k["id"], d) not in so.BLIND and reach(k, d)[0] > 1.0]
            assert seen, (d, "prepend" if prepend else "adaLN")


def test_emulation_is_switched_off_after_use():
    orig = ko.linear, ko._attn_operands, ko._softmax, ko.continuous_transformer
    k = so.BY_ID["S3"]
    R = so.reference(k)
    so.outputs(k, R["W"], R["inp"], R["traj"]["xs"], R["traj"]["ts"], "f64", "prepended token not skipped")
    assert (ko.linear, ko._attn_operands, ko._softmax, ko.continuous_transformer) == orig
    assert ko.linear is orig[0]
