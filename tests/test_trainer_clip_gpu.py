"""-m gpu: engine.DataParallelTrainer(max_grad_norm / skip_nonfinite / track_grad_norm) on the small DiT and Llasa trainers of
tests/test_trainer_oracle_gpu.py, held after EVERY optimizer step to tests/grad_clip_refs.py:

  norm      tr.grad_norm against the fp64 norm of the trainer's own flat gradient (1 / (world accum) applied), inside
            grad_clip_refs.norm_bound; the alignment gaps of flat.grad are exactly zero (they are summed too)
  coef      tr.clip_coef within one fp32 ulp of coef64 of the device's published norm
  step      weights and moments per element against the teacher-forced fp64 step taken with the device's published coef, inside
            trainer_oracle.adam_bound; the bf16 mirror, last_lr and step_count bit for bit

Two runs of the same window do not give the same gradient bits (the weight-gradient kernels add with fp32 atomics), so every
"bit-identical across two trainers" statement is teacher-forced as well: the second trainer is handed the first one's state from
before the step and its flat gradient, takes optimizer_step() on its own route, and must land on the same bits.
The seeded defects (grad_clip_refs.STEP_DEFECTS) are held against the states the DEVICE recorded and must fall out of bound."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grad_clip_refs as gc  # noqa: E402
import trainer_oracle as to  # noqa: E402
import test_grad_slices_gpu as tg  # noqa: E402
import test_trainer_oracle_gpu as tt  # noqa: E402

RUNS = {}          # name -> (cfg, records, ranges, gaps, max_norm): the device's recorded runs, shared with the defect tests
FIRST = {}         # (config, case) -> fp64 norm of the first step's averaged gradient


def _check(tr, before, after, ctl, k, max_norm, skipped_before, what, total):
    """the per-step contract of the module docstring; returns the record kept for the defect tests"""
    cfg, G, gaps = to.cfg_of(tr), after["grad"], to.gap_mask(tr.flat)
    gs = gc.f32(1.0 / (cfg["world"] * cfg["accum"]))
    assert not (G[gaps] != 0).any(), what
    rec = dict(before=before, after=after, G=G, k=k, coef=ctl["clip_coef"], skip=ctl["skip"], skipped_before=skipped_before)
    if torch.isfinite(G).all():
        n64 = gc.norm64([G], gs)
        err, lim = abs(ctl["grad_norm"] - n64), gc.norm_bound(n64, tr.flat.total)
        assert err <= lim, (what, k, ctl["grad_norm"], n64, err / lim)
        total["norm"] = max(total.get("norm", 0.0), err / lim)
        want = gc.coef64(ctl["grad_norm"], max_norm, round32=False)
        assert abs(ctl["clip_coef"] - want) <= gc.ulp32(want), (what, k, ctl["clip_coef"], want)
        assert not ctl["nonfinite"] and not ctl["skip"]
    else:
        assert ctl["nonfinite"], what
    ratios = gc.check_clip_step(before, after, G, cfg, k, tr.flat.bucket_range, gaps, coef=ctl["clip_coef"], skip=ctl["skip"],
                                max_norm=max_norm, skipped_before=skipped_before)
    assert not to.failures(ratios), (what, k, to.failures(ratios), to.worst(ratios))
    for q, v in to.worst(ratios).items():
        total[q] = max(total.get(q, 0.0), v)
    return rec


def _windows(tr, micro, windows, what, max_norm=None, on_window=None):
    """`windows` accumulation windows, every optimizer step checked.  micro(w, i): runs micro-batch i of window w."""
    recs, total = [], {}
    for w in range(windows):
        torch.cuda.synchronize()
        before = to.snapshot(tr)
        for i in range(tr.grad_accum_steps):
            micro(w, i)
        torch.cuda.synchronize()
        after, ctl = to.snapshot(tr), tr.opt_ctl()
        recs.append(_check(tr, before, after, ctl, before["step_count"] + 1, max_norm, ctl["skipped_steps"] - int(ctl["skip"]), what, total))
        if on_window is not None:
            on_window(w, recs[-1], ctl)
    tt._report(what, total)
    return recs


def _dit_micro(tr, model, c, dev):
    return lambda w, i: tg._train_step(tr, model, c, c["seed"] + 10 * (w * tr.grad_accum_steps + i), dev)


def _first_norm(name, case, dev):
    """fp64 norm of the first optimizer step's averaged gradient (a tracking trainer's own flat gradient)"""
    if (name, case) not in FIRST:
        model, tr, c, _ = tt._dit_trainer(name, case, dev, track_grad_norm=True)
        _windows(tr, _dit_micro(tr, model, c, dev), 1, f"CLIP first norm {name} {case}")
        FIRST[(name, case)] = gc.norm64([to.snapshot(tr)["grad"]], 1.0 / tr.grad_accum_steps)
    return FIRST[(name, case)]


def _shadow_step(shadow, before, G):
    """teacher forcing across trainers: `shadow` takes the step from `before` with the gradient G on ITS route"""
    f = shadow.flat
    f.param.copy_(before["param"]), shadow.exp_avg.copy_(before["exp_avg"]), shadow.exp_avg_sq.copy_(before["exp_avg_sq"])
    f.param_bf16.copy_(before["mirror"]), f.grad.copy_(G)
    shadow.step_count = before["step_count"]
    shadow.optimizer_step()
    torch.cuda.synchronize()
    return to.snapshot(shadow)


def _same_bits(a, b, what):
    for key in ("param", "exp_avg", "exp_avg_sq", "mirror"):
        assert to._bits_equal(a[key], b[key]), (what, key)
    assert a["last_lr"] == b["last_lr"] and a["step_count"] == b["step_count"], what


def _bits(t):
    return t.detach().cpu().view(torch.int32).item()


# ------------------------------------------------------------------------------------------------ clipping, accumulation, schedule
@pytest.mark.parametrize("name,case", [("T1", 712), ("T3", 713)])
def test_clipping_active(dev, name, case):
    """max_grad_norm = half the first step's fp64 norm: AdamW / accum 2 / schedule (T1) and coupled Adam / accum 1 (T3)"""
    max_norm = 0.5 * _first_norm(name, case, dev)
    model, tr, c, steps = tt._dit_trainer(name, case, dev, max_grad_norm=max_norm)
    recs = _windows(tr, _dit_micro(tr, model, c, dev), steps, f"CLIP active {name} {case}", max_norm)
    assert tr._overlap_now is False and 0.49 < recs[0]["coef"] < 0.51
    assert tr.opt_ctl()["clipped_steps"] == sum(r["coef"] < 1 for r in recs) and tr.opt_ctl()["skipped_steps"] == 0
    assert len({r["after"]["last_lr"] for r in recs}) == steps
    RUNS[(name, case)] = (to.cfg_of(tr), recs, dict(tr.flat.bucket_range), to.gap_mask(tr.flat), max_norm)


def test_clipping_inactive_is_the_plain_trainer_bit_for_bit(dev):
    """max_grad_norm = 1e9: coef is exactly 1 and every step lands on the bits of a trainer built without the option"""
    model, tr, c, steps = tt._dit_trainer("T1", 712, dev, max_grad_norm=1e9, skip_nonfinite=True)
    _, plain, _, _ = tt._dit_trainer("T1", 712, dev)
    assert plain.grad_norm is None and plain.opt_ctl() is None

    def on_window(w, rec, ctl):
        assert ctl["clip_coef"] == 1.0 and ctl["clipped_steps"] == 0
        _same_bits(rec["after"], _shadow_step(plain, rec["before"], rec["G"]), f"inactive window {w}")

    _windows(tr, _dit_micro(tr, model, c, dev), steps, "CLIP inactive T1 712", 1e9, on_window)


@pytest.mark.parametrize("mode", ["clip", "track"])
def test_overlapped_route_equals_single_pass_bit_for_bit(dev, monkeypatch, mode):
    """overlap_min_rows = 0: every bucket's sum runs on the optimizer stream behind its backward (the Adam slices too under
    track_grad_norm alone; ONE kalle_adam_step_ctl behind the finish under max_grad_norm).  A KALLE_OVERLAP_ADAM=0 trainer handed
    the same state and gradient publishes the same norm bits and lands on the same weights"""
    from kalle_audio_amd import ops
    max_norm = 0.5 * _first_norm("T1", 712, dev) if mode == "clip" else None
    kw = dict(max_grad_norm=max_norm) if mode == "clip" else dict(track_grad_norm=True)
    model, tr, c, steps = tt._dit_trainer("T1", 712, dev, **kw)
    assert tr.overlap_adam
    tr.overlap_min_rows = 0
    monkeypatch.setenv("KALLE_OVERLAP_ADAM", "0")
    _, single, _, _ = tt._dit_trainer("T1", 712, dev, **kw)
    assert not single.overlap_adam
    seen = []
    sumsq, finish, adam, adam_ctl = ops.grad_sumsq, ops.grad_norm_finish, ops.adam_step, ops.adam_step_ctl

    def rec(tag, fn):
        def f(*a, **k):
            seen.append((tag, torch.cuda.current_stream() == tr._opt_stream, a[0].numel()))
            return fn(*a, **k)
        return f

    for nm, fn in (("grad_sumsq", sumsq), ("grad_norm_finish", finish), ("adam_step", adam), ("adam_step_ctl", adam_ctl)):
        monkeypatch.setattr(ops, nm, rec(nm, fn))

    def on_window(w, r, ctl):
        tags = [s[0] for s in seen]
        nb = len(tr.flat.bucket_keys)
        assert all(s[1] for s in seen), seen                                  # all of it on the optimizer stream
        assert tags.count("grad_sumsq") == nb and tags.count("grad_norm_finish") == 1
        assert tags.index("grad_norm_finish") > max(i for i, t in enumerate(tags) if t == "grad_sumsq")
        if mode == "clip":
            assert tags.count("adam_step") == 0 and tags[-1] == "adam_step_ctl" and seen[-1][2] == tr.flat.total
        else:
            assert tags.count("adam_step") == nb and tags.count("adam_step_ctl") == 0
        del seen[:]
        norm_bits = _bits(tr.grad_norm)
        other = _shadow_step(single, r["before"], r["G"])
        del seen[:]
        assert _bits(single.grad_norm) == norm_bits and single.opt_ctl()["clip_coef"] == ctl["clip_coef"]
        _same_bits(r["after"], other, f"overlap vs single pass, window {w}")

    _windows(tr, _dit_micro(tr, model, c, dev), steps, f"CLIP overlapped {mode} T1 712", max_norm, on_window)
    assert tr._overlap_now


def test_track_grad_norm_alone(dev):
    """the norm is published, nothing else changes: ops.adam_step stays, coef stays 1, no counter moves"""
    model, tr, c, steps = tt._dit_trainer("T3", 713, dev, track_grad_norm=True)
    recs = _windows(tr, _dit_micro(tr, model, c, dev), steps, "CLIP track only T3 713")
    ctl = tr.opt_ctl()
    assert ctl["clip_coef"] == 1.0 and ctl["clipped_steps"] == 0 and ctl["skipped_steps"] == 0 and ctl["grad_norm"] > 0
    assert set(tr.state_dict()) >= {"skipped_steps", "clipped_steps"}


# ------------------------------------------------------------------------------------------------ skip
def _inf_loss_step(tr, model, c, seed, dev):
    from kalle_audio_amd.stable_audio_tools.training.diffusion import diffusion_train_step
    inp = {n: None if v is None else v.to(dev) for n, v in tg.gs.dit_inputs(c, seed).items()}
    cm = inp["cm"] if inp["cm"] is not None else torch.ones(inp["ctx"].shape[:2], dtype=torch.bool, device=dev)
    cond = {"prompt": (inp["ctx"], cm), "g": (inp["gl"], None)}
    loss, _ = diffusion_train_step(model, inp["lat"], inp["t"], inp["noise"], cond, objective=c["obj"], padding_mask=inp["pm"])
    tr.backward(loss * math.inf)


@pytest.mark.parametrize("how", ["bucket", "loss"])
def test_skip_at_step_two(dev, how):
    """step 2 is poisoned - an inf written into one bucket of flat.grad followed by optimizer_step(), or a loss scaled by inf:
    nothing moves, counters and schedule advance, step 3 matches the reference with the SPENT step number, and a trainer
    resumed from the state dict continues on the same bits"""
    name, case = "T3", 713
    max_norm = 0.5 * _first_norm(name, case, dev)
    model, tr, c, _ = tt._dit_trainer(name, case, dev, max_grad_norm=max_norm, skip_nonfinite=True)
    tr.enable_ema(update_every=1, **to.EMA_KW)
    data = _dit_micro(tr, model, c, dev)

    def micro(w, i):
        if w != 1:
            return data(w, i)
        if how == "loss":
            return _inf_loss_step(tr, model, c, c["seed"] + 10, dev)
        a, b = tr.flat.bucket_range[tt.MID]
        tr.flat.grad[a + 5] = math.inf                 # (the flat gradient still holds step 1's)
        tr.optimizer_step()
        tr.micro += 1

    seen = []

    def on_window(w, rec, ctl):
        seen.append(ctl)
        if w == 1:
            assert ctl["skip"] and ctl["nonfinite"] and ctl["skipped_steps"] == 1
            _same_bits(dict(rec["before"], last_lr=rec["after"]["last_lr"], step_count=2), rec["after"], "skipped step")
            assert rec["after"]["last_lr"] == to.lr_of(to.cfg_of(tr), 2) and rec["after"]["ema_sched"].step == 2
            assert to._bits_equal(rec["after"]["ema"], rec["after"]["param"])           # (a copy step of the EMA: it ran)

    recs = _windows(tr, micro, 3, f"CLIP skip via {how}", max_norm, on_window)
    assert [s["skipped_steps"] for s in seen] == [0, 1, 1] and not seen[2]["skip"] and recs[2]["k"] == 3
    assert (recs[2]["after"]["param"] != recs[1]["after"]["param"]).any()
    if how == "bucket":
        RUNS["skip"] = (to.cfg_of(tr), recs, dict(tr.flat.bucket_range), to.gap_mask(tr.flat), max_norm)
        # resume: the counters travel, and the resumed trainer takes step 3 from step 3's state on the same bits
        sd = tt._clone(tr.state_dict())
        assert sd["skipped_steps"] == 1 and sd["clipped_steps"] == seen[2]["clipped_steps"] and sd["step"] == 3
        _, tb, _, _ = tt._dit_trainer(name, case, dev, max_grad_norm=max_norm, skip_nonfinite=True)
        tb.load_state_dict(sd)
        assert tb.opt_ctl()["skipped_steps"] == 1 and tb.step_count == 3
        tb.step_count = 2
        _same_bits(recs[2]["after"], _shadow_step(tb, recs[2]["before"], recs[2]["G"]), "resumed")
        assert tb.opt_ctl()["skipped_steps"] == 1 and tb.opt_ctl()["clipped_steps"] == sd["clipped_steps"] + int(recs[2]["coef"] < 1)


# ------------------------------------------------------------------------------------------------ Llasa
def test_llasa_trainer_clipped(dev, tmp_path):
    """Llasa (alignment gaps in the flat layout, the embedding table's scatter-add in `_rest`), AdamW, accum 2, 3 windows"""
    from kalle_audio_amd import engine
    c = tt.LLASA[801]
    m = tt._llasa_model(c, dev, tmp_path)
    probe = engine.DataParallelTrainer(m, lr=0.0, optimizer="AdamW", grad_accum_steps=2, track_grad_norm=True)
    micro = lambda tr: (lambda w, i: tt._llasa_micro(tr, m, c, tt._llasa_seeds(c, w)[i], dev))
    _windows(probe, micro(probe), 1, "CLIP llasa first norm")
    max_norm = 0.5 * gc.norm64([to.snapshot(probe)["grad"]], 0.5)
    m = tt._llasa_model(c, dev, tmp_path)
    tr = engine.DataParallelTrainer(m, lr=1e-3, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=2, max_grad_norm=max_norm,
                                    skip_nonfinite=True)
    assert to.gap_mask(tr.flat).any()
    recs = _windows(tr, micro(tr), 3, "CLIP llasa 801", max_norm)
    assert 0.49 < recs[0]["coef"] < 0.51 and tr.opt_ctl()["skipped_steps"] == 0


# ------------------------------------------------------------------------------------------------ forced communication
_COMM_WORKER = r'''
import os, sys, json, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tests", "golden"))
os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], KALLE_FORCE_COMM="1")
import torch.distributed as dist
from kalle_audio_amd import engine
import test_trainer_clip_gpu as T
dev = torch.device("cuda:0")
rank, world, _ = engine.init_distributed()
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
max_norm = float(sys.argv[3])
model, tr, c, steps = T.tt._dit_trainer("T1", 712, dev, max_grad_norm=max_norm, skip_nonfinite=True)
assert tr._comm_active()
tr.overlap_min_rows = 0
recs = T._windows(tr, T._dit_micro(tr, model, c, dev), 3, "CLIP forced comm", max_norm)
assert tr._overlap_now and tr._comm_events == len(tr.flat.bucket_keys)
res = {"coef": [r["coef"] for r in recs], "ctl": tr.opt_ctl()}
dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_forced_comm_world1(dev, tmp_path):
    """KALLE_FORCE_COMM=1 with a world-1 RCCL group in a child process (as tests/test_round2_gpu.py sets it up): every bucket's
    sum waits for its all-reduce on the optimizer stream; the same per-step checks run inside the child"""
    max_norm = 0.5 * _first_norm("T1", 712, dev)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "clip_comm_worker.py"
    script.write_text(_COMM_WORKER)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), os.path.join(HERE, ".."), str(port), repr(max_norm)], capture_output=True,
                       text=True, timeout=420, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert 0.49 < res["coef"][0] < 0.51 and res["ctl"]["clipped_steps"] == sum(x < 1 for x in res["coef"])
    assert res["ctl"]["skipped_steps"] == 0


# ------------------------------------------------------------------------------------------------ defects on the device's states
def _caught(run, defect, only=None):
    cfg, recs, ranges, gaps, max_norm = run
    bad = []
    for r in recs:
        if only is not None and r["k"] not in only:
            continue
        ratios = gc.check_clip_step(r["before"], r["after"], r["G"], cfg, r["k"], ranges, gaps, coef=r["coef"], skip=r["skip"],
                                    max_norm=max_norm, skipped_before=r["skipped_before"], defect=defect)
        bad += to.failures(ratios)
    return bad


def test_defects_fail_on_the_device_states(dev):
    """clipping per bucket, the norm of the window's sum, the coefficient on exp_avg only (T1: accum 2); `_rest` stepped on the
    skipped step and torch's un-advanced step number after it (skip at step 2, where the bias corrections differ most)"""
    if ("T1", 712) not in RUNS:
        test_clipping_active(dev, "T1", 712)
    if "skip" not in RUNS:
        test_skip_at_step_two(dev, "bucket")
    for defect in ("clip_per_bucket", "norm_of_sum", "coef_on_m_only"):
        assert not _caught(RUNS[("T1", 712)], None) and _caught(RUNS[("T1", 712)], defect), defect
    assert not _caught(RUNS["skip"], None)
    bad = _caught(RUNS["skip"], "rest_on_skip", only=(2,))
    assert bad and all(b[1] == "_rest" for b in bad), bad
    assert _caught(RUNS["skip"], "torch_step_after_skip", only=(3,))
    assert not _caught(RUNS["skip"], "torch_step_after_skip", only=(1, 2))      # (no skip yet / nothing stepped: blind there)
