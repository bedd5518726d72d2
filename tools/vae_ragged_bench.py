"""Ragged lists through the Oobleck VAE (the Stable-Audio-Open layout of tools/vae_bench.py): decode_list / encode_list against
the B = 1 loop and against the zero-padded dense batch.  The padded batch computes WRONG tails and is here only as a
yardstick of what batching can reach; it runs over the same groups as the list form, without lengths.

Lists: 16 and 64 latents with lengths uniform in 20..215 frames, and 16 and 64 short ones, 20..60 frames (seeded).  Each list is
timed whole (wall clock around a synchronize), the three ways in rotation, one warm-up and three repeats each, min - max.
python tools/vae_ragged_bench.py [bf16]"""
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kalle_audio_amd  # noqa: E402

kalle_audio_amd.install()
from stable_audio_tools.models.factory import create_model_from_config  # noqa: E402

half = "bf16" in sys.argv[1:]
LAT, RATIO = 64, 2048
cfg = {"model_type": "autoencoder", "sample_rate": 44100, "sample_size": 441000, "audio_channels": 2,
       "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 2, "channels": 128, "c_mults": [1, 2, 4, 8, 16],
                                                          "strides": [2, 4, 4, 8, 8], "latent_dim": 128, "use_snake": True}},
                 "decoder": {"type": "oobleck", "config": {"out_channels": 2, "channels": 128, "c_mults": [1, 2, 4, 8, 16],
                                                          "strides": [2, 4, 4, 8, 8], "latent_dim": LAT, "use_snake": True,
                                                          "final_tanh": False}},
                 "bottleneck": {"type": "vae"}, "latent_dim": LAT, "downsampling_ratio": RATIO, "io_channels": 2}}
dev = torch.device("cuda")
torch.manual_seed(0)
with torch.device(dev):
    ae = create_model_from_config(cfg)
ae.eval().requires_grad_(False)
dt = torch.bfloat16 if half else torch.float32
REPEATS = 3


def padded_dense(items, sizes, per, fn):
    """the same groups as the list form, zero-padded, no lengths (wrong tails: a yardstick only)"""
    out = [None] * len(items)
    for grp in ae._ragged_groups(sizes, per, ae._default_cap()):
        x, L = ae._stack([items[i] for i in grp], items[0].shape[1])
        y = fn(x)
        for b, i in enumerate(grp):
            out[i] = y[b:b + 1]
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(name, direction, frames):
    if direction == "decode":
        items = [torch.randn(1, LAT, T, device=dev).to(dt) for T in frames]
        per, one, lst = (lambda T: T * RATIO), ae.decode, ae.decode_list
    else:
        items = [(torch.rand(1, 2, T * RATIO, device=dev) * 2 - 1).to(dt) for T in frames]
        per, one, lst = (lambda n: n), ae.encode, ae.encode_list
    sizes = [t.shape[2] for t in items]
    ways = {"list": lambda: lst(items), "loop B=1": lambda: [one(t) for t in items],
            "padded dense": lambda: padded_dense(items, sizes, per, one)}
    times = {k: [] for k in ways}
    with torch.no_grad():
        for k, f in ways.items():
            timed(f)                                        # warm-up: plans, weight folds, the allocator's pools
        for _ in range(REPEATS):
            for k, f in ways.items():                       # rotating
                times[k].append(timed(f))
    groups = ae._ragged_groups(sizes, per, ae._default_cap())
    audio_s = sum(frames) * RATIO / 44100
    live = sum(frames) / sum(len(g) * max(frames[i] for i in g) for g in groups)
    row = f"{name} {direction}: n={len(frames)} frames {min(frames)}..{max(frames)} ({audio_s:.0f} s of audio), {len(groups)} group(s), live share {live:.2f}"
    for k, v in times.items():
        row += f" | {k} {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} ms"
    row += f" | list vs loop {min(times['loop B=1']) / min(times['list']):.2f}x, list vs padded {min(times['padded dense']) / min(times['list']):.2f}x"
    print(row, flush=True)


rng = random.Random(1234)
LISTS = [("mixed16", [rng.randint(20, 215) for _ in range(16)]), ("mixed64", [rng.randint(20, 215) for _ in range(64)]),
         ("short16", [rng.randint(20, 60) for _ in range(16)]), ("short64", [rng.randint(20, 60) for _ in range(64)])]
print(f"activations {'bf16' if half else 'fp32'}, default cap {ae._default_cap()} samples per group, chunk_batch {ae.chunk_batch}")
for name, frames in LISTS:
    for direction in ("decode", "encode"):
        bench(name, direction, frames)
