"""No GPU: ops.weights_key - the one key of every cache derived from weights ("Weight-derived caches") - against
the ways a model's weights can change, on a small nn.Linear and on a conv module with weight_g / weight_v.  The file also
documents which routes torch itself reports (the version counter moves) and which only the address, the identity or the write
epoch can show.  tests/test_weight_caches_gpu.py runs the same routes through the caches themselves."""
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _linear():
    torch.manual_seed(0)
    return nn.Linear(24, 16)


def _wn_conv():
    from kalle_audio_amd import flows
    torch.manual_seed(0)
    return flows.weight_norm(flows.Conv1d(6, 8, 3))


MODULES = {"linear": _linear, "weight_g_v": _wn_conv}


def _key(m):
    from kalle_audio_amd import ops
    return ops.weights_key(*m.parameters())


def _hold(m):
    """what a cache keeps next to its key: while it lives, a re-pointed parameter cannot land on the keyed address"""
    from kalle_audio_amd import ops
    return ops.weights_pin(*m.parameters())


def _versions(m):
    return [p._version for p in m.parameters()]


def _other(m):
    return {k: torch.randn_like(v) for k, v in m.state_dict().items()}


@pytest.fixture
def no_gpu_adam(monkeypatch):
    """ops.adam_step as it is - the epoch it moves included - with the launch itself replaced (it needs the GPU)"""
    from kalle_audio_amd import ops
    monkeypatch.setattr(ops._lib, "load", lambda: SimpleNamespace(kalle_adam_step=lambda *a: 0))
    monkeypatch.setattr(ops, "_p", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)


def r1(m):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)


def r2(m):
    m.load_state_dict(_other(m))


def r3(m):
    old = {n: p._version for n, p in m.named_parameters()}
    sd = _other(m)
    for n, v in old.items():
        for _ in range(v):
            sd[n].add_(0)
    m.load_state_dict(sd, assign=True)
    assert {n: p._version for n, p in m.named_parameters()} == old      # the counters coincide: identity and address tell


def r4(m):
    for p in m.parameters():
        p.data = torch.randn_like(p)


def r4_half_float(m):
    m.half().float()


def r4_vector_to_parameters(m):
    ps = list(m.parameters())
    torch.nn.utils.vector_to_parameters(torch.randn(sum(p.numel() for p in ps)), ps)


def r5(m):
    from kalle_audio_amd.engine import FusedAdam
    opt = FusedAdam(m.parameters(), lr=1e-2)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()


def r6_construct(m):
    from kalle_audio_amd import engine
    m._tr = engine.DataParallelTrainer(m, lr=1e-2)


def r6_step(m):
    from kalle_audio_amd import engine
    tr = engine.DataParallelTrainer(m, lr=1e-2)
    before = _key(m)
    tr.flat.grad.fill_(1.0)
    tr.optimizer_step()
    assert _key(m) != before
    m._tr = tr


def r6_load(m):
    from kalle_audio_amd import engine
    tr = engine.DataParallelTrainer(m, lr=1e-2)
    before = _key(m)
    sd = tr.state_dict()
    sd["model"] = _other(m)
    tr.load_state_dict(sd)
    assert _key(m) != before
    m._tr = tr


def r7(m):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()


# route -> does torch's version counter move?  (the table of INTEGRATION.md; asserted below)
ROUTES = {"R1-inplace": (r1, True), "R2-load_state_dict": (r2, True), "R3-assign": (r3, False), "R4-data": (r4, False),
          "R4-half-float": (r4_half_float, False), "R4-vector_to_parameters": (r4_vector_to_parameters, False),
          "R5-FusedAdam": (r5, False), "R6-trainer-construction": (r6_construct, False), "R6-trainer-step": (r6_step, False),
          "R6-trainer-load_state_dict": (r6_load, True), "R7-AdamW": (r7, True)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("module", list(MODULES))
def test_key_moves(module, route, no_gpu_adam):
    from kalle_audio_amd import ops
    fn, torch_reports = ROUTES[route]
    m = MODULES[module]()
    k0, hold, v0 = _key(m), _hold(m), _versions(m)
    assert _key(m) == k0                                   # stable across two reads with no change in between
    first = next(m.parameters())
    one = ops.weights_key(first)
    assert ops.weights_key_is(one, first)
    fn(m)
    assert _key(m) != k0, "the key did not move"
    first = next(m.parameters())
    assert ops.weights_key_is(one, first) == (one == ops.weights_key(first)) and not ops.weights_key_is(one, first)
    assert (_versions(m) != v0) == torch_reports, (v0, _versions(m))
    assert _key(m) == _key(m)
    del hold


@pytest.mark.parametrize("module", list(MODULES))
def test_r8_key_moves_only_after_weights_changed(module):
    """p.data.copy_ / p.data.lerp_ (ema_pytorch's writes): nothing torch or the package can see - the key stays, and moves with
    the one public call"""
    import kalle_audio_amd
    m = MODULES[module]()
    k0, v0 = _key(m), _versions(m)
    for p in m.parameters():
        p.data.copy_(torch.randn_like(p))
        p.data.lerp_(torch.randn_like(p), 0.5)
    assert _key(m) == k0 and _versions(m) == v0
    kalle_audio_amd.weights_changed()
    k1 = _key(m)
    assert k1 != k0 and _key(m) == k1


def test_r9_key_moves_with_weight_norm_removed_and_applied():
    from kalle_audio_amd import flows
    m = _wn_conv()
    keys, holds = [_key(m)], [_hold(m)]
    flows.remove_weight_norm(m)
    assert sorted(n for n, _ in m.named_parameters()) == ["bias", "weight"]
    keys.append(_key(m))
    holds.append(_hold(m))
    flows.weight_norm(m)
    assert sorted(n for n, _ in m.named_parameters()) == ["bias", "weight_g", "weight_v"]
    keys.append(_key(m))
    assert len({k for k in keys}) == 3


def test_key_is_pure_and_names_every_field():
    from kalle_audio_amd import ops
    m = _linear()
    e0 = ops.WEIGHTS_EPOCH
    k = ops.weights_key(m.weight, m.bias)
    assert ops.WEIGHTS_EPOCH == e0 and _versions(m) == [p._version for p in m.parameters()]
    assert k == ((id(m.weight), m.weight._version, m.weight.data_ptr(), m.weight.device, m.weight.dtype),
                 (id(m.bias), m.bias._version, m.bias.data_ptr(), m.bias.device, m.bias.dtype), e0)
    assert ops.weights_key() == (e0,)
    one = ops.weights_key(m.weight)
    assert ops.weights_key_is(one, m.weight) and not ops.weights_key_is(one, m.bias)
    pins = ops.weights_pin(m.weight, m.bias)
    assert [t.data_ptr() for t in pins] == [m.weight.data_ptr(), m.bias.data_ptr()] and not any(t.requires_grad for t in pins)


def test_a_held_pin_keeps_a_repointed_parameter_off_the_keyed_address():
    """module.half().float() frees an fp32 block and allocates one of the same size: without the pin the allocator may hand the
    old address out again, and version, address, device and dtype would all read as before"""
    from kalle_audio_amd import ops
    m = _linear()
    for _ in range(8):
        key, pin = ops.weights_key(m.weight), ops.weights_pin(m.weight)
        m.half().float()
        assert ops.weights_key(m.weight) != key and m.weight.data_ptr() != pin[0].data_ptr()
        del pin


def test_fused_adam_restamps_current_copies_and_drops_others(no_gpu_adam):
    """FusedAdam.step moves the epoch with every launch: a bf16 copy that was current before the step is stamped with the new key
    (the launch updated it, or the parameter was not written), one that was not is dropped - never a re-cast of every weight"""
    from kalle_audio_amd import ops
    from kalle_audio_amd.engine import FusedAdam
    ps = [nn.Parameter(torch.randn(4, 4)) for _ in range(4)]
    for p in ps:
        p._kalle_bf16 = (ops.weights_key(p), p.detach().bfloat16(), ops.weights_pin(p))
    copies = [p._kalle_bf16[1] for p in ps]
    with torch.no_grad():
        ps[1].add_(0.0)                                    # its copy no longer belongs to these weights
    for p in ps[:3]:
        p.grad = torch.ones_like(p)                        # ps[3]: no gradient, not written
    e0 = ops.WEIGHTS_EPOCH
    FusedAdam(ps, lr=1e-2).step()
    assert ops.WEIGHTS_EPOCH == e0 + 3
    for i in (0, 2, 3):
        assert ps[i]._kalle_bf16[0] == ops.weights_key(ps[i]) and ps[i]._kalle_bf16[1] is copies[i]
    assert not hasattr(ps[1], "_kalle_bf16")


# ------------------------------------------------------------------------------------------------ world 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        torch.set_num_threads(1)
        import torch.distributed as dist
        from kalle_audio_amd import engine, ops
        engine.init_distributed(backend="gloo")
        torch.manual_seed(100 + rank)
        model = nn.Linear(8, 8)
        key, pin, e0 = ops.weights_key(*model.parameters()), ops.weights_pin(*model.parameters()), ops.WEIGHTS_EPOCH
        w_own = model.weight.detach().clone()
        tr = engine.DataParallelTrainer(model, lr=1e-3)
        # the broadcast wrote rank 0's weights through .data and the flat buffers re-pointed every parameter: the epoch moved
        # for both, and the key with it
        assert ops.WEIGHTS_EPOCH >= e0 + 2, (e0, ops.WEIGHTS_EPOCH)
        assert ops.weights_key(*model.parameters()) != key
        assert torch.equal(model.weight, w_own) == (rank == 0)
        assert tr.world == world
        del pin
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_epoch_moves_across_trainer_construction_at_world_2():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"
