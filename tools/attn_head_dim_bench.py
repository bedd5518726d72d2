"""time the attention kernels and one DiT train step at head dims 32, 64 and 128 (fixed D = 1536, so attention's bytes and
FLOPs do not depend on the head dim):  python tools/attn_head_dim_bench.py [--kernels-only] [--steps-only]

  kernels: self / cross forward and backward at the bench shape (B = 256, N = 126, S = 130, Dc = 768; rotary 32 / 32 / 64)
  steps:   a 24-layer DiT (a copy of bench.CFG with num_heads = 48 / 24 / 12) at B = 64 and 256, median of 5 steps"""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kalle_audio_amd import ops  # noqa: E402

dev = torch.device("cuda")
B, N, D, Dc = 256, 126, 1536, 768
S = 130
ROT = {32: 32, 64: 32, 128: 64}


def timed(fn, reps=8):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        ts.append((e0, e1))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ts)[len(ts) // 2]


def kernels():
    mk = lambda *s: (torch.randn(*s, device=dev) * 0.7).bfloat16()  # noqa: E731
    qkv, q, kv, dout = mk(B, N, 3 * D), mk(B, N, D), mk(B, S, 2 * Dc), mk(B, N, D)
    res = {}
    for dh in (32, 64, 128):
        H, Hkv, rot = D // dh, Dc // dh, ROT[dh]
        inv = 1.0 / (10000 ** (torch.arange(0, rot, 2, device=dev).float() / rot))
        f = torch.arange(N, device=dev).float()[:, None] * inv[None]
        rope = (f.cos().contiguous(), f.sin().contiguous())
        sa = dict(ldq=3 * D, q_off=0, ldk=3 * D, k_off=D, ldv=3 * D, v_off=2 * D, B=B, H=H, Hkv=H, Nq=N, Nk=N, dh=dh)
        ca = dict(ldq=D, q_off=0, ldk=2 * Dc, k_off=0, ldv=2 * Dc, v_off=Dc, B=B, H=H, Hkv=Hkv, Nq=N, Nk=S, dh=dh)
        o1, l1 = ops.attention_fwd(qkv, qkv, qkv, rope=rope, **sa)
        o2, l2 = ops.attention_fwd(q, kv, kv, **ca)
        dqkv, dq, dkv = torch.empty_like(qkv), torch.empty_like(q), torch.empty_like(kv)
        cases = [("self fwd", lambda: ops.attention_fwd(qkv, qkv, qkv, rope=rope, **sa)),
                 ("cross fwd", lambda: ops.attention_fwd(q, kv, kv, **ca)),
                 ("self bwd", lambda: ops.attention_bwd(qkv, qkv, qkv, o1, dout, l1, dqkv, dqkv, dqkv, rope=rope, **sa)),
                 ("cross bwd", lambda: ops.attention_bwd(q, kv, kv, o2, dout, l2, dq, dkv, dkv, **ca))]
        for _, fn in cases:
            fn()
        torch.cuda.synchronize()
        for name, fn in cases:
            res[(name, dh)] = timed(fn) * 1e3
    print(f"{'kernel (us)':12s} {'dh 32':>9s} {'dh 64':>9s} {'dh 128':>9s} {'32/64':>6s} {'128/64':>7s}")
    for name in ("self fwd", "cross fwd", "self bwd", "cross bwd"):
        a, b, c = (res[(name, dh)] for dh in (32, 64, 128))
        print(f"{name:12s} {a:9.1f} {b:9.1f} {c:9.1f} {a / b:6.2f} {c / b:7.2f}")


def steps():
    import bench
    from kalle_audio_amd import engine
    res = {}
    for dh in (32, 64, 128):
        cfg = copy.deepcopy(bench.CFG)
        cfg["num_heads"] = cfg["embed_dim"] // dh
        model = bench.build_model(dev, cfg=cfg)
        tr = engine.DataParallelTrainer(model, lr=1e-5, optimizer="Adam")
        for Bs in (64, 256):
            lat, noise, t, cond = bench.make_batch(Bs, dev, 1234, cfg=cfg)
            step = lambda: tr.train_step(model, lat, t, noise, cond, objective="v")  # noqa: E731
            step(); step()
            torch.cuda.synchronize()
            res[(Bs, dh)] = timed(step, 5)
            del lat, noise, t, cond
        del tr, model
        torch.cuda.empty_cache()
    print(f"{'train step (ms)':16s} {'dh 32':>9s} {'dh 64':>9s} {'dh 128':>9s}")
    for Bs in (64, 256):
        a, b, c = (res[(Bs, dh)] for dh in (32, 64, 128))
        print(f"B = {Bs:<12d} {a:9.1f} {b:9.1f} {c:9.1f}")


if __name__ == "__main__":
    if "--steps-only" not in sys.argv:
        kernels()
    if "--kernels-only" not in sys.argv:
        steps()
