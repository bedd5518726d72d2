"""What the gradient-norm options of engine.DataParallelTrainer cost on the DiT bench shape.

  python tools/trainer_clip_bench.py --batch 64 [--modes off,track,clip] [--blocks 5] [--steps 5]
      one process: a (model, trainer) pair per mode, timed in interleaved blocks of `--steps` train steps
      (off | track_grad_norm=True | max_grad_norm=1.0); prints one JSON line with every block's ms per step.
  python tools/trainer_clip_bench.py --ab OTHER_CHECKOUT --batch 64,256 --repeats 3
      alternates child processes: OTHER_CHECKOUT (another built checkout of this repository, e.g. the parent commit: only
      the trainer without options exists there) and this tree, `--repeats` times each, and prints medians and spreads.
  python tools/trainer_clip_bench.py --sumsq
      kalle_grad_sumsq alone: GB/s on a 175 MB bucket and on the whole 4.2 GB flat gradient."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"off": {}, "track": dict(track_grad_norm=True), "clip": dict(max_grad_norm=1.0)}


def run_modes(root, batch, modes, blocks, steps):
    sys.path.insert(0, root)
    import torch
    import bench
    from kalle_audio_amd import engine
    dev = torch.device("cuda:0")
    lat, noise, t, cond = bench.make_batch(batch, dev, 1234)
    pairs = []
    for m in modes:
        model = bench.build_model(dev)
        pairs.append((m, model, engine.DataParallelTrainer(model, lr=1e-5, optimizer="Adam", **MODES[m])))
    for _, model, tr in pairs:
        for _ in range(2):
            tr.train_step(model, lat, t, noise, cond, objective="v")
    torch.cuda.synchronize()
    out = {m: [] for m in modes}
    for _ in range(blocks):
        for m, model, tr in pairs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                tr.train_step(model, lat, t, noise, cond, objective="v")
            e1.record()
            torch.cuda.synchronize()
            out[m].append(e0.elapsed_time(e1) / steps)
    ctl = {m: tr.opt_ctl() for m, _, tr in pairs if getattr(tr, "opt_ctl", None) and tr.opt_ctl()}
    print("RESULT " + json.dumps({"root": root, "batch": batch, "ms_per_step": out, "ctl": ctl}), flush=True)


def run_sumsq():
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from kalle_audio_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for name, n in (("bucket_175MB", 175_000_000 // 4), ("flat_4.2GB", 1_050_000_000)):
        g = torch.randn(n, device=dev)
        ws, ctl = ops.grad_norm_ws(1, dev), ops.OptCtl(dev)
        for _ in range(3):
            ops.grad_sumsq(g, ws, 0, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.grad_sumsq(g, ws, 0, 1)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        ops.grad_norm_finish(ws, 1, ctl)
        res[name] = {"n": n, "ms": ms, "GB_per_s": 4 * n / ms / 1e6, "norm": ctl.norm.item(), "norm_torch_fp64": g.double().norm().item()}
        del g
    print("RESULT " + json.dumps(res), flush=True)


def run_ab(other, batches, repeats, blocks, steps):
    me = os.path.dirname(HERE)
    rows = {}
    for batch in batches:
        for _ in range(repeats):
            for tag, root, modes in (("other", other, "off"), ("this", me, "off,track,clip")):
                cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--batch", str(batch), "--modes", modes,
                       "--blocks", str(blocks), "--steps", str(steps)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
                if r.returncode != 0:
                    raise SystemExit(f"{tag} B={batch} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                for m, v in res["ms_per_step"].items():
                    rows.setdefault((batch, tag, m), []).append(statistics.median(v))
                    print(f"B={batch} {tag}:{m} blocks {' '.join(f'{x:.2f}' for x in v)}", flush=True)
    summary = {f"B{b}:{tag}:{m}": {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": v}
               for (b, tag, m), v in rows.items()}
    print("SUMMARY " + json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--batch", default="64")
    ap.add_argument("--modes", default="off,track,clip")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ab", metavar="OTHER_CHECKOUT", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sumsq", action="store_true")
    a = ap.parse_args()
    if a.sumsq:
        return run_sumsq()
    if a.ab:
        return run_ab(os.path.abspath(a.ab), [int(b) for b in a.batch.split(",")], a.repeats, a.blocks, a.steps)
    run_modes(os.path.abspath(a.root), int(a.batch), a.modes.split(","), a.blocks, a.steps)


if __name__ == "__main__":
    main()
