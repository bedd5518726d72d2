"""The per-slice check of the VAE conv stacks (tests/vae_oracle.py) on the reference alone (CPU, no kernel runs): the seams
leave the fp64 oracle bit-identical, the yardstick on every case tests/test_vae_oracle_gpu.py uses, the heavier emulation that M
is measured with, the seeded defects (each reported, or listed blind and then asserted blind), and the restated chunk loop against
the reference-made fixtures.

Measured here: r on z and rec 8e-7 ... 2.4e-5 (fp32 cases; M r <= 9.2e-5 on the inference path), 1.2e-2 on the bf16 case; the
heavier emulation reaches 2.60 r (z of O2; vae_oracle.py lists every case), M = ceil(1.5 x 2.60) = 4; the weakest reported defect
is one stored intermediate rounded to 11 bits, 24 r on O3 - its whole-tensor rel-L2, what the older tests bound by 1e-4, is
6.9e-5 ... 3.1e-4 over the cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_oracle as vo  # noqa: E402

gu, ko = vo.gu, vo.ko
FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chunked_vae.npz")


def test_slices_scale_and_pools():
    assert vo.cuts_of(40) == [0, 16, 32, 40] and vo.cuts_of(36) == [0, 16, 36] and vo.cuts_of(60, (20, 60, 0)) == [0, 20, 36, 52, 60]
    ref = torch.zeros(1, 2, 32, dtype=torch.float64)
    ref[0, 0, :16] = 1.0
    got = ref.clone()
    got[0, 0, 3] += 0.5
    got[0, 1, 20] += 0.5
    q = vo.act_ratio(got, ref)
    # the loud slice is measured by its own norm (4), a silent one by the floor 0.25 |ref| sqrt(16 / 64) = 0.5; no slice is excluded
    assert q.shape == (2, 2) and abs(q[0, 0].item() - 0.125) < 1e-12 and abs(q[1, 1].item() - 1.0) < 1e-12 and q[0, 1].item() == 0
    t = {"a.alpha": torch.ones(4), "b.alpha": 2 * torch.ones(8), "c.weight_v": torch.ones(4, 4, 7), "d.weight_v": torch.ones(16, 4, 7),
         "act:z": torch.ones(1, 1, 5)}
    p = vo.pooled(t)
    assert sorted(p) == ["act:z", "d.weight_v", "pool:alpha", "pool:weight_v"] and p["pool:alpha"].tolist() == [1.0] * 4 + [2.0] * 8
    assert vo.pool_members(t, "alpha") == [("a.alpha", 0, 4), ("b.alpha", 4, 12)] and p["pool:weight_v"].numel() == 112
    assert not vo.is_act("pool:alpha") and vo.is_act("inf:z")


@pytest.mark.parametrize("cid", ["O1", "O2", "O5"])
def test_seams_leave_the_fp64_oracle_bit_identical(cid):
    """the same fp64 run through every seam of vae_oracle._Run (no perturbation, a defect label nothing answers to) and through the
    untouched oracle: equal bit for bit, every tensor; and kalle_oracle is itself again afterwards"""
    before = (ko._act, ko.F, ko.snake, ko.residual_unit, ko.torch, ko.wn_weight)
    plain = vo.reference(cid)
    seamed = vo._reference(dict(vo.CASES[cid], wide_odd=False), "f64", 0, "none")
    assert (ko._act, ko.F, ko.snake, ko.residual_unit, ko.torch, ko.wn_weight) == before
    assert sorted(plain) == sorted(seamed)
    for n in plain:
        assert plain[n].dtype == torch.float64 and torch.equal(plain[n], seamed[n]), n


@pytest.mark.parametrize("cid", list(vo.CASES))
def test_yardstick(cid):
    """r comes from the reference alone; on z and rec of the inference path M r stays below the 1e-4 the whole-tensor tests
    allow (fp32 cases), and the plain fp32 oracle - no perturbation - is inside r"""
    c = vo.CASES[cid]
    ref = vo.select(vo.reference(cid))
    r, raw = vo.yardstick(cid)
    print(cid, "median r %.2e" % sorted(raw.values())[len(raw) // 2], {n: "%.1e" % v for n, v in r.items() if vo.is_act(n) or n.startswith("pool:")})
    assert set(r) == set(ref) and all(v > 0 for v in r.values())
    for n in ("inf:z", "inf:rec"):
        if n in r and not c["bf16"]:
            assert vo.M * r[n] < 1e-4, (n, r[n])
    if c["bf16"]:
        assert 2.0 ** -9 < r["inf:rec"] < 5e-2, r           # a chain of some forty bf16 stores
    if c["train"]:
        assert {"act:rec", "pool:bias", "pool:weight_g"} <= set(r) and any(n.endswith("weight_v") for n in r)
    for fz in (vo.FROZEN_SETS if cid in vo.FROZEN_CASES else ()):
        rf, _ = vo.yardstick(cid, fz)
        assert ("act:dwav" in rf) == (fz != "encoder") and len(rf) <= len(r), fz


@pytest.mark.parametrize("cid", list(vo.CASES))
def test_heavier_emulation_within_m(cid):
    """allowances doubled, fresh sign seeds, every conv summed tap by tap over two halves of its input channels: inside M r on
    every slice of every tensor, HEAVY_DRAWS draws.  M = ceil(1.5 x the largest figure printed here over all cases) is measured,
    not assumed: vae_oracle.py lists them"""
    ref = vo.select(vo.reference(cid))
    r, _ = vo.yardstick(cid)
    top = {}
    for d in range(vo.HEAVY_DRAWS):
        for n, v in vo.rho_of(vo.select(vo.reference(cid, "heavy", d)), ref, r).items():
            top[n] = max(top.get(n, 0.0), v)
    w = max(top, key=top.get)
    print(cid, "heavier / r: largest %.2f (%s)" % (top[w], w))
    assert len(top) == len(ref) and not vo.failures(top), vo.failures(top)


def test_constants_are_the_documented_ones():
    assert vo.M == 4.0 and vo.ALLOW is vo.tcg.ALLOW and vo.MARGIN == 4.0 and vo.DRAWS == 12 and vo.HEAVY_DRAWS == 4


@pytest.mark.parametrize("cid", list(vo.CASES))
def test_seeded_defects_are_reported(cid):
    """every defect the case has the structure for, seeded alone into the fp64 reference: some slice of some tensor exceeds M r -
    or the pair is in BLIND, and then it is blind.  Prints the whole-tensor rel-L2 of the activations (what the older tests
    bound by 1e-4) next to it."""
    c = vo.CASES[cid]
    ref = vo.select(vo.reference(cid))
    r, _ = vo.yardstick(cid)
    n_applied = 0
    for d in vo.DEFECTS:
        if not vo.applies(d, c):
            continue
        n_applied += 1
        g = vo.select(vo.reference(cid, "f64", 0, d))
        rho = vo.rho_of(g, ref, r)
        w = max(rho, key=rho.get)
        rel = max(vo.rel_l2(g[n], ref[n]) for n in ref if vo.is_act(n))
        print(f"{cid} {d:26s} {w:46s} rho {rho[w]:12.1f}   activations rel-L2 {rel:.1e}" + ("   BLIND" if (cid, d) in vo.BLIND else ""))
        assert bool(vo.failures(rho)) != ((cid, d) in vo.BLIND), (cid, d, w, rho[w])
    assert n_applied >= 5 and all(b[1] in vo.DEFECTS + vo.CHUNK_DEFECTS and b[0] in list(vo.CASES) + ["chunked"] for b in vo.BLIND)


def test_every_defect_has_a_case():
    for d in vo.DEFECTS:
        shown = [cid for cid, c in vo.CASES.items() if vo.applies(d, c) and (cid, d) not in vo.BLIND]
        assert shown, d
    assert sum(vo.applies("bwd_extra_zeroed", c) for c in vo.CASES.values()) == 2        # the "+ 3" cases


# ------------------------------------------------------------------------------------------------ the chunk loop
def _fixture_case():
    """tests/golden/chunked_vae.npz was made by the reference on gu.oobleck_cfg(True), seed 23: O1's layout"""
    c = dict(vo.CASES["O1"], id="fixture", seed=23)
    sd = {k: torch.from_numpy(v) for k, v in gu.make_state(vo.shapes(c), 23).items()}
    return c, sd


def test_chunk_loop_matches_the_reference_made_fixtures():
    """the restated loop, run in fp32 on the oracle, against what the reference's own decode_audio(chunked=True) produced:
    (48, 16) with an anchored last chunk, (48, 15) where kept regions overlap by a latent and the later chunk wins - fp32 noise.
    The reference's own chunked ENCODE does not run on a VAE bottleneck (it allocates latent_dim channels for 2 latent_dim; the
    fixture records that), so the encode side is pinned as the older test pins it: the unchunked encode against the fixture, and
    the chunked one against it where the receptive field stays inside a kept region."""
    f = np.load(FX)
    c, sd = _fixture_case()
    r_ = c["ratio"]
    z = torch.from_numpy(gu.make_input("zc", (2, 4, 125), 65))
    with torch.no_grad():
        for ov, key in ((16, "dec_48_16"), (15, "dec_48_15")):
            y, seams = vo.chunked(lambda t: vo._decode(None, sd, c, t), z, 48, 48 - ov, lambda s: s * r_, 48 * r_, 125 * r_, (ov // 2) * r_)
            e = vo.rel_l2(y, torch.from_numpy(f[key]))
            print(key, "rel-L2 %.1e" % e, "seams", seams)
            assert e < 2e-6, (key, e)
            assert len(seams) >= 4
        assert int(f["enc_chunked_runs"]) == 0
        wav = torch.from_numpy(gu.make_input("wavc", (2, 2, 5000), 65, 0.5))
        full = vo._encode(sd, c, wav)
        assert vo.rel_l2(full, torch.from_numpy(f["enc_full"])) < 2e-6
        ch, seams = vo.chunked(lambda t: vo._encode(sd, c, t), wav, 48 * r_, 32 * r_, lambda s: s // r_, 48, 125, 8)
        assert ch.shape == full.shape and seams == [40, 72, 85, 104]
        for lo, hi in ((0, 32), (48, 64), (100, 125)):
            assert vo.rel_l2(ch[..., lo:hi], full[..., lo:hi]) < 2e-6, (lo, hi)


def test_chunk_loop_differs_from_the_plan_only_in_name():
    """the drop-in's _chunk_plan is NOT what the reference is built from; that the two agree on where pastes begin is checked on
    the device (tests/test_vae_oracle_gpu.py).  Here: the seams of the three chunked cases are where the arithmetic puts them"""
    want = [[1600, 2400, 2880], [1120, 2080, 2880, 3040], [40, 60, 72]]
    for i in range(len(vo.CHUNKED)):
        _, seams = vo.chunk_reference(i)
        assert seams["chunk:y"] == want[i] and len(seams["chunk:dx"]) == len(want[i]), (i, seams)


@pytest.mark.parametrize("i", range(len(vo.CHUNKED)), ids=lambda i: "-".join(map(str, vo.CHUNKED[i])))
def test_chunked_yardstick_heavier_and_defects(i):
    ref, seams = vo.chunk_reference(i)
    r, _ = vo.chunk_yardstick(i)
    assert vo.M * r["chunk:y"] < 1e-4, r
    top = {}
    for d in range(vo.HEAVY_DRAWS):
        for n, v in vo.rho_of(vo.chunk_reference(i, "heavy", d)[0], ref, r, seams).items():
            top[n] = max(top.get(n, 0.0), v)
    print(vo.CHUNKED[i], {n: "%.1e" % v for n, v in r.items()}, "heavier / r", {n: round(v, 2) for n, v in top.items()})
    assert not vo.failures(top), top
    for d in vo.CHUNK_DEFECTS:
        g, _ = vo.chunk_reference(i, "f64", 0, d)
        rho = vo.rho_of(g, ref, r, seams)
        print(f"   {d:22s} rho {max(rho.values()):10.1f}   rel-L2 of y {vo.rel_l2(g['chunk:y'], ref['chunk:y']):.1e}")
        if ("chunked", d) in vo.BLIND:
            assert all(torch.equal(g[n], ref[n]) for n in ref), d          # blind because it is the same arithmetic
        else:
            assert vo.failures({"chunk:y": rho["chunk:y"]}), (d, rho)


# ------------------------------------------------------------------------------------------------ mel-VAE
@pytest.mark.parametrize("cid", list(vo.MELVAE_CASES))
def test_melvae_yardstick_and_heavier(cid):
    ref = vo.melvae_reference(cid)
    r, raw = vo.melvae_yardstick(cid)
    assert set(ref) == {"mel:latents", "mel:rec", "mel:z_p", "mel:logs_q", "mel:dec"} and ref["mel:rec"].dtype == torch.float64
    assert all(vo.M * v < 1e-4 for v in r.values()), r
    top = {}
    for d in range(vo.HEAVY_DRAWS):
        for n, v in vo.rho_of(vo.melvae_reference(cid, "heavy", d), ref, r).items():
            top[n] = max(top.get(n, 0.0), v)
    print(cid, {n: "%.1e" % v for n, v in r.items()}, "heavier / r", {n: round(v, 2) for n, v in top.items()})
    assert not vo.failures(top), top
    if cid == "up5x3":
        assert ref["mel:latents"].shape[2] == 173 and ref["mel:dec"].shape[2] % 16 != 0
