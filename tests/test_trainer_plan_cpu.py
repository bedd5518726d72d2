"""CPU: engine.plan_step / DataParallelTrainer.step_plan, and the trainer's launch trace against the record of the engine that
had no planner.

  * plan_step over the full product of its switches, rows and window positions against the route table restated here;
  * step_plan() of constructed trainers agrees with it, also after a test flips a switch;
  * outside __init__ and step_plan no method of the trainer names a switch: they branch on the plan;
  * tests/trainer_trace.py's CPU cases equal tests/golden/trainer_trace.json call for call."""
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import trainer_trace as tt  # noqa: E402
import test_grad_clip_cpu as tc  # noqa: E402

ROWS = (None, 0, 68, 504, 4095, 4096, 8191, 8192)
SWITCHES = ("group_wgrad", "overlap_adam", "sharded", "comm", "norm_on", "norm_gate", "blocks", "cuda", "first", "boundary")


def _table(*, rows, first, boundary, group_wgrad, overlap_adam, overlap_min_rows, sharded, comm, norm_on, norm_gate, blocks, cuda):
    """the route table, one question at a time (rows None: nothing went through backward(), nothing runs on the side)"""
    n = rows or 0
    grouped = group_wgrad and n > 0 and n % 8 == 0
    clear_once = n >= 8192 and not grouped
    want = {"accumulate": True if (clear_once or grouped) else not first, "wgrad_overwrite": grouped and first}
    if not first:
        want["clear"] = "none"
    elif clear_once:
        want["clear"] = "all"
    else:
        want["clear"] = "small+tail" if grouped else "tail"
    overlap = False
    if boundary and rows is not None and overlap_adam:
        overlap = n >= overlap_min_rows or not blocks
    if not boundary:
        hook = "none"
    elif sharded:
        hook = "shard"
    elif not overlap:
        hook = "allreduce" if comm else "none"          # (the deferred all-reduce is a no-op without comm)
    else:
        hook = "queue"
    want.update(boundary=boundary, sharded=sharded, overlap=overlap, hook=hook, norm=norm_on, gate=norm_gate,
                reduce_tail=boundary and comm and not overlap, wait_side=boundary and sharded and cuda and not overlap)
    return want


def test_plan_step_full_product():
    from kalle_audio_amd import engine
    assert set(engine.StepPlan._fields) == set(_table(rows=0, overlap_min_rows=0, **dict.fromkeys(SWITCHES, False)))
    seen, refused = set(), 0
    for bits in itertools.product((False, True), repeat=len(SWITCHES)):
        sw = dict(zip(SWITCHES, bits))
        for rows, min_rows in itertools.product(ROWS, (0, 4096)):
            kw = dict(sw, rows=rows, overlap_min_rows=min_rows)
            if (sw["sharded"] and not sw["comm"]) or (sw["norm_gate"] and not sw["norm_on"]) or (sw["sharded"] and sw["norm_on"]):
                refused += 1
                with pytest.raises(AssertionError):       # pairs that never meet: the constructor refuses / derives them
                    engine.plan_step(**kw)
                continue
            plan = engine.plan_step(**kw)
            assert plan._asdict() == _table(**kw), kw
            assert all(type(v) is (str if f in ("hook", "clear") else bool) for f, v in plan._asdict().items()), plan
            seen.add((plan.hook, plan.clear, plan.overlap))
    assert refused and {h for h, _, _ in seen} == {"none", "shard", "allreduce", "queue"}
    assert {c for _, c, _ in seen} == {"none", "all", "tail", "small+tail"}


def test_plan_step_is_pure():
    """no self, no torch, no environment: plain values in, an immutable record out"""
    from kalle_audio_amd import engine
    src = inspect.getsource(engine.plan_step)
    assert "os.environ" not in src and "torch" not in src and "self" not in inspect.signature(engine.plan_step).parameters
    plan = engine.plan_step(rows=4096, overlap_min_rows=4096, **dict.fromkeys(SWITCHES, False))
    with pytest.raises(AttributeError):
        plan.overlap = True


@pytest.mark.parametrize("accum", [1, 3])
@pytest.mark.parametrize("mode", ["plain", "track", "clip", "plain-comm", "plain-shard"])
def test_step_plan_of_a_trainer(monkeypatch, mode, accum):
    from kalle_audio_amd import dit_ops, engine
    base, _, comm = mode.partition("-")
    monkeypatch.delenv("KALLE_SHARD_OPTIMIZER", raising=False)
    monkeypatch.delenv("KALLE_FORCE_COMM", raising=False)
    if comm:
        monkeypatch.setenv("KALLE_FORCE_COMM", "1")
        monkeypatch.setenv("KALLE_SHARD_OPTIMIZER", str(int(comm == "shard")))
    tc._Standins(monkeypatch)
    tt.Trace(monkeypatch, standin_collectives=bool(comm))
    tr = engine.DataParallelTrainer(tc._Net(), grad_accum_steps=accum, **tt.MODES[base])
    assert not tr.overlap_adam and tr.overlap_min_rows == 4096 and tr._overlap_now is False and tr._opt_lr is None
    for group, overlap, min_rows in itertools.product((False, True), (False, True), (0, 4096)):
        monkeypatch.setattr(dit_ops, "GROUP_WGRAD", group)
        tr.overlap_adam, tr.overlap_min_rows = overlap, min_rows            # (as the GPU tests flip them on a built trainer)
        for rows, micro in itertools.product(ROWS, range(2 * accum)):
            want = _table(rows=rows, first=micro % accum == 0, boundary=micro % accum == accum - 1, group_wgrad=group,
                          overlap_adam=overlap, overlap_min_rows=min_rows, sharded=comm == "shard", comm=bool(comm),
                          norm_on=base != "plain", norm_gate=base == "clip", blocks=True, cuda=False)
            assert tr.step_plan(rows, micro)._asdict() == want, (group, overlap, min_rows, rows, micro)
    tr.micro = accum - 1
    assert tr.step_plan(68) == tr.step_plan(68, accum - 1) and tr.step_plan(68).boundary and tr._boundary()
    assert tr._sharded_active() == (comm == "shard") and tr._comm_active() == bool(comm)
    if not comm:            # (with the stand-ins there is no process group to ask for its backend)
        assert tr.comm_summary()["sharded_optimizer"] is False and tr.comm_summary()["allreduce_active"] is False


def test_methods_branch_on_the_plan_only():
    """outside __init__ and step_plan (the adapter that hands the switches to plan_step) no method names a switch"""
    from kalle_audio_amd import engine
    for name, fn in vars(engine.DataParallelTrainer).items():
        if name in ("__init__", "step_plan") or not callable(fn):
            continue
        src = inspect.getsource(fn)
        for word in ("overlap_adam", "shard_opt", "_norm_gate", "overlap_min_rows", "GROUP_WGRAD", "_norm_on"):
            assert word not in src, (name, word)


def test_step_state_lives_for_one_step(monkeypatch):
    monkeypatch.delenv("KALLE_SHARD_OPTIMIZER", raising=False)
    from kalle_audio_amd import engine
    tc._Standins(monkeypatch)
    net = tc._Net()
    tr = engine.DataParallelTrainer(net, lr=1e-2, grad_accum_steps=2, lr_schedule=lambda s: 0.5 ** s)
    assert tr._step is None and tr.ema is None and tr.ema_schedule is None
    tc._micro(tr, net, 1)
    assert tr._step is None and tr._opt_lr is None and tr.step_count == 0           # a window's first micro-batch begins nothing
    tr._begin_optimizer_step()
    st = tr._step
    assert (st.k, st.lr, tr._opt_lr) == (1, 1e-2, 1e-2) and st.plan == tr.step_plan(None) and not st.adam_done
    assert st.adam_kw["step"] == 1 and st.adam_kw["grad_scale"] == tr.grad_scale == 0.5
    tr.optimizer_step()
    assert tr._step is None and tr._opt_lr is None and tr._last is st and tr.last_lr == 1e-2 and tr._comm_events == 0
    tr.optimizer_step()                                                             # directly: it begins its own
    assert tr._last.k == 2 and tr.last_lr == 0.5e-2 and tr._step is None


# ------------------------------------------------------------------------------------------------ the launch trace
GOLDEN = json.load(open(tt.GOLDEN))
CPU_CASES = [f"{m}/accum{a}/{d}" for m in tt.CPU_MODES for a in (1, 3) for d in tt.DRIVES]


def test_golden_covers_the_cases():
    assert sorted(GOLDEN["cpu"]) == sorted(CPU_CASES) and "commit" in GOLDEN["made_by"]
    kinds = {c[0] for case in GOLDEN["cpu"].values() for micro in case for c in micro}
    assert kinds == set(tt.OPS) | set(tt.COLLECTIVES)


@pytest.mark.parametrize("case", CPU_CASES)
def test_launch_trace_equals_the_parents(monkeypatch, case):
    """(call, first element offset, numel, step, grad_scale, lr) of every ops / torch.distributed call, micro-batch by micro-batch"""
    from kalle_audio_amd import engine
    mode, accum, drive = case.split("/")
    got = tt.canon(tt.cpu_case(engine, monkeypatch, mode, int(accum[5:]), drive))
    assert got == GOLDEN["cpu"][case]
