"""-m gpu: the overlapped routes of engine.DataParallelTrainer issue the calls of the engine that had no step planner - same
ops functions, same element ranges, step numbers, grad_scale and lr, same order, and the same ones on the optimizer stream.
tests/trainer_trace.py drives T1 of trainer_oracle.CONFIGS on the smallest DiT of grad_slices.TRAINER_CASES with
overlap_min_rows = 0 (every bucket queued from its hook, `_rest` from _finish_comm); tests/golden/trainer_trace.json holds what
that engine did there."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trainer_trace as tt  # noqa: E402

GOLDEN = json.load(open(tt.GOLDEN))


@pytest.mark.parametrize("mode", tt.GPU_MODES)
def test_overlapped_launch_trace_equals_the_parents(dev, monkeypatch, mode):
    """plain: Adam slices on the optimizer stream; track: a sum of squares in front of each, the finish behind the last; clip: the
    sums, the finish and ONE kalle_adam_step_ctl over [0, total), all on the optimizer stream"""
    from kalle_audio_amd import engine
    want = GOLDEN["gpu"][mode]
    assert len(want) == 2 * tt.GPU_WINDOWS and want[0] == [] and all(c[-1] is True for c in want[1])
    got = tt.canon(tt.gpu_case(engine, monkeypatch, mode, dev))
    assert got == want
