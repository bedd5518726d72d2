"""Launch trace of engine.DataParallelTrainer: which ops / torch.distributed calls a step issues, over which element ranges
of the flat buffers, with which step number, grad_scale and lr (and, on the GPU, whether on the optimizer stream).  Shared by
tests/test_trainer_plan_cpu.py and tests/test_trainer_plan_gpu.py; tests/golden/trainer_trace.json holds the record the same
functions made of the engine BEFORE the step planner existed (`python tests/trainer_trace.py cpu|gpu` prints one), so equality
says the refactored trainer issues the parent's calls in the parent's order.

CPU cases   {plain, track, clip, skip, plain-comm, clip-comm, plain-shard} x accum {1, 3} x {through backward(), the hooks called
            by hand as tests/test_dp_gloo.py does, optimizer_step() called directly}; ops functions are test_grad_clip_cpu's
            stand-ins, the collectives (no process group here) world-1 stand-ins of torch.distributed.
GPU cases   trainer_oracle's T1 on the smallest DiT of grad_slices.TRAINER_CASES with overlap_min_rows = 0: plain, track, clip."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OPS = ("adam_step", "adam_step_ctl", "grad_sumsq", "grad_norm_finish")
COLLECTIVES = ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor")
MODES = {"plain": {}, "track": dict(track_grad_norm=True), "clip": dict(max_grad_norm=0.05), "skip": dict(skip_nonfinite=True)}
CPU_MODES = ("plain", "track", "clip", "skip", "plain-comm", "clip-comm", "plain-shard")
DRIVES = ("backward", "hooks", "direct")
GPU_CASE, GPU_MODES, GPU_WINDOWS = 711, ("plain", "track", "clip"), 2
GOLDEN = os.path.join(HERE, "golden", "trainer_trace.json")


class _Work:
    def wait(self):
        return True


class Trace:
    """wraps the four ops functions (whatever they are at the time: the library's or a test's stand-ins) and the three
    collectives with recorders.  patch: a pytest MonkeyPatch."""

    def __init__(self, patch, standin_collectives=False):
        from kalle_audio_amd import ops
        self.calls, self.tr = [], None
        for name in OPS:
            patch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        if standin_collectives:
            patch.setattr(dist, "is_initialized", lambda: True)
            patch.setattr(dist, "get_world_size", lambda group=None: 1)
            patch.setattr(dist, "get_rank", lambda group=None: 0)
            patch.setattr(dist, "all_reduce", lambda t, **k: _Work())                      # (a world of one: the sum is the input)
            patch.setattr(dist, "reduce_scatter_tensor", lambda out, inp, **k: (out.copy_(inp), _Work())[1])
            patch.setattr(dist, "all_gather_into_tensor", lambda out, inp, **k: (out.copy_(inp), _Work())[1])
        for name in COLLECTIVES:
            patch.setattr(dist, name, self._wrap(name, getattr(dist, name)))

    def _where(self, t):
        """(first element offset, numel) of a tensor inside one of the trainer's flat buffers; offset None outside them"""
        tr = self.tr
        for buf in (tr.flat.param, tr.flat.grad):
            off = (t.data_ptr() - buf.data_ptr()) // buf.element_size()
            if t.dtype == buf.dtype and 0 <= off < buf.numel():
                return off, t.numel()
        return None, t.numel()

    def _wrap(self, name, fn):
        def f(*a, **k):
            if self.tr is not None:
                # the tensor that names the range: the weights of an Adam pass, the gradient of a sum or a reduction, the
                # gathered weights of an all-gather; grad_norm_finish has none (its workspace: numel = the slot count)
                t = a[1] if name == "reduce_scatter_tensor" else a[0]
                off, n = (None, a[1]) if name == "grad_norm_finish" else self._where(t)
                rec = [name, off, n, k.get("step"), k.get("grad_scale"), k.get("lr")]
                if t.is_cuda:
                    rec.append(bool(self.tr._opt_stream is not None and torch.cuda.current_stream() == self.tr._opt_stream))
                self.calls.append(rec)
            return fn(*a, **k)
        return f

    def take(self):
        c, self.calls = self.calls, []
        return c


# ------------------------------------------------------------------------------------------------ CPU
def _fill(tr, seed):
    """a gradient for the hand-driven routes (small integers: exact under any order of summation)"""
    g = torch.Generator().manual_seed(seed)
    tr.flat.grad.copy_(torch.randint(-3, 4, (tr.flat.total,), generator=g).float())


def cpu_case(engine, patch, mode, accum, drive, windows=2):
    """the trace of `windows` optimizer steps of one case; engine: the module under test"""
    import test_grad_clip_cpu as tc
    base, _, comm = mode.partition("-")
    patch.delenv("KALLE_SHARD_OPTIMIZER", raising=False)
    patch.delenv("KALLE_FORCE_COMM", raising=False)
    if comm:
        patch.setenv("KALLE_FORCE_COMM", "1")
    if comm == "shard":
        patch.setenv("KALLE_SHARD_OPTIMIZER", "1")
    tc._Standins(patch)
    trace = Trace(patch, standin_collectives=bool(comm))
    net = tc._Net()
    tr = engine.DataParallelTrainer(net, lr=1e-2, optimizer="AdamW", weight_decay=0.01, grad_accum_steps=accum,
                                    lr_schedule=lambda s: 1.0 / (1 + s), **MODES[base])
    trace.tr = tr
    assert bool(comm) == tr._comm_active() and (comm == "shard") == tr._sharded_active()
    out = []
    for w in range(windows):
        if drive == "direct":
            _fill(tr, w)
            tr.optimizer_step()
            out.append(trace.take())
            continue
        for i in range(accum):
            if drive == "backward":
                tc._micro(tr, net, 10 * w + i)
            else:
                _fill(tr, 10 * w + i)
                if tr._boundary():
                    tr._begin_optimizer_step()
                for _, blk in reversed(tr.blocks):
                    tr._on_block_done(blk)
                tr._finish_comm()
                assert tr._pending == []
                if tr._boundary():
                    tr.optimizer_step()
                tr.micro += 1
            out.append(trace.take())
    assert tr.step_count == windows and tr._opt_lr is None
    return out


def cpu_traces(engine):
    import pytest
    out = {}
    for mode in CPU_MODES:
        for accum in (1, 3):
            for drive in DRIVES:
                with pytest.MonkeyPatch.context() as patch:
                    out[f"{mode}/accum{accum}/{drive}"] = cpu_case(engine, patch, mode, accum, drive)
    return out


# ------------------------------------------------------------------------------------------------ GPU
def gpu_case(engine, patch, mode, dev):
    """T1 (AdamW, accum 2, schedule) on TRAINER_CASES' smallest DiT with every bucket overlapped; one list per micro-batch"""
    import test_grad_slices_gpu as tg
    import test_trainer_oracle_gpu as tt
    kw, _, _ = tt.to.CONFIGS["T1"]
    c = tt.TC[GPU_CASE]["base"]
    model = tg._wrapped(c, dev)
    over = dict(MODES[mode], max_grad_norm=0.5) if mode == "clip" else MODES[mode]
    tr = engine.DataParallelTrainer(model, **dict(kw, **over))
    assert tr.overlap_adam
    tr.overlap_min_rows = 0
    trace = Trace(patch)
    trace.tr = tr
    out = []
    for m in range(GPU_WINDOWS * tr.grad_accum_steps):
        tg._train_step(tr, model, c, c["seed"] + 10 * m, dev)
        out.append(trace.take())
    torch.cuda.synchronize()
    assert tr.step_count == GPU_WINDOWS and tr._overlap_now
    return out


def gpu_traces(engine, dev):
    import pytest
    out = {}
    for mode in GPU_MODES:
        with pytest.MonkeyPatch.context() as patch:
            out[mode] = gpu_case(engine, patch, mode, dev)
    return out


def canon(x):
    """what json keeps of a trace (lists, not tuples)"""
    return json.loads(json.dumps(x))


if __name__ == "__main__":
    # python tests/trainer_trace.py cpu|gpu [path of an engine.py to load in place of the package's]
    sys.path.insert(0, os.path.dirname(HERE))
    from kalle_audio_amd import engine
    if len(sys.argv) > 2:
        import importlib.util
        spec = importlib.util.spec_from_file_location("kalle_audio_amd._engine_under_trace", sys.argv[2])
        engine = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(engine)
    print(json.dumps(cpu_traces(engine) if sys.argv[1] == "cpu" else gpu_traces(engine, torch.device("cuda:0"))))
