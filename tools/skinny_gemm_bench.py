"""the forward GEMMs of one DiT block at generation batch sizes (M = 252 rows for B = 1 with CFG), each timed alone with HIP events
over launches captured into a HIP graph: python tools/skinny_gemm_bench.py [M]
--decode [R ...]: the eight decoder GEMMs of a KV-cached step (Llama-3.2-1B / 3B shapes) instead - gemv_kernel against
gemv_e4m3_kernel, and gemm_rows_kernel<YF32, TR, 1> against gemm_rows_e4m3_kernel at each R (default 1 8 16) - fp32 output, no residual, the
weights rotating through > 600 MB of copies so that no call finds them in a cache; per kernel the median of 5 runs (min - max)
in microseconds and the TB/s of weight bytes
--decode-wide: those GEMMs at 16 rows (gemm_rows_kernel at NCB = 1), 32 and 64 rows (NCB = 2 and 4) and, for comparison, ops.gemm at
64 rows"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kalle_audio_amd import ops, _lib
dev = torch.device("cuda")


def decode_bench(rows):
    shapes = [("1B q|k|v", 3072, 2048), ("1B o", 2048, 2048), ("1B up|gate", 16384, 2048), ("1B down", 2048, 8192),
              ("3B q|k|v", 5120, 3072), ("3B o", 3072, 3072), ("3B up|gate", 16384, 3072), ("3B down", 3072, 8192)]

    def timed(fns):
        """median, min, max over 5 runs of the mean time per call over one pass through the rotating copies, microseconds.  The
        pass is captured into one HIP graph (as the DiT shapes below are): device time per launch, without the host's per-call
        cost (a torch.empty, the wrapper's asserts, ctypes), which differs between the wrappers and exceeds the small GEMVs"""
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for f in fns[:2]:
                f()
            side.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for f in fns:
                    f()
        gr.replay()
        torch.cuda.synchronize()
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / len(fns))
        runs.sort()
        return runs[2], runs[0], runs[-1]

    for name, n, k in shapes:
        copies = 600 * 2 ** 20 // (n * k) + 2              # > 600 MB of e4m3 copies (twice that in bf16)
        ws = [(torch.randn(n, k, device=dev) / k ** 0.5).bfloat16() for _ in range(copies)]
        qs = [ops.quantize_rows_e4m3(w) for w in ws]
        x1 = torch.randn(k, device=dev).bfloat16()
        cols = []
        for what, bytes_per, fns in (("gemv_kernel", 2, [lambda w=w: _gemv(x1, w) for w in ws]),
                                     ("gemv_e4m3", 1, [lambda q=q: ops.gemv_e4m3(x1, q[0], q[1]) for q in qs])):
            med, lo, hi = timed(fns)
            cols.append(f"{what} {med:5.1f} ({lo:.1f} - {hi:.1f}) us {n * k * bytes_per / med / 1e6:4.1f} TB/s")
        for R in rows:
            xr = torch.randn(R, k, device=dev).bfloat16()
            for what, bytes_per, fns in ((f"rows R={R}", 2, [lambda w=w: ops.gemm_rows(xr, w) for w in ws]),
                                         (f"rows_e4m3 R={R}", 1, [lambda q=q: ops.gemm_rows_e4m3(xr, q[0], q[1]) for q in qs])):
                med, lo, hi = timed(fns)
                cols.append(f"{what} {med:5.1f} ({lo:.1f} - {hi:.1f}) us {n * k * bytes_per / med / 1e6:4.1f} TB/s")
        print(f"{name:10s} {n} x {k}: " + " | ".join(cols), flush=True)
        del ws, qs


def decode_wide_bench():
    """--decode-wide: the same eight GEMMs through kalle_gemm_rows_fused at R = 16 and kalle_gemm_rows_wide at R = 32 and 64, and
    - for comparison only, it is not wired into the decode step - the training GEMM's few-rows plan (ops.gemm) at 64 rows.  Per
    kernel the median of 5 runs (min - max) in microseconds, the TB/s of weight bytes, and the time of four 16-row calls over
    the 64-row call.  KALLE_LIB_PATH selects the build, so two tile rules can be compared on one box."""
    shapes = [("1B q|k|v", 3072, 2048), ("1B o", 2048, 2048), ("1B up|gate", 16384, 2048), ("1B down", 2048, 8192),
              ("3B q|k|v", 5120, 3072), ("3B o", 3072, 3072), ("3B up|gate", 16384, 3072), ("3B down", 3072, 8192)]
    for name, n, k in shapes:
        copies = 300 * 2 ** 20 // (n * k) + 2              # > 600 MB of bf16 copies
        ws = [(torch.randn(n, k, device=dev) / k ** 0.5).bfloat16() for _ in range(copies)]
        cols, med = [], {}
        for R, fn in ((16, ops.gemm_rows), (32, ops.gemm_rows_wide), (64, ops.gemm_rows_wide), (-64, ops.gemm)):
            xr = torch.randn(abs(R), k, device=dev).bfloat16()
            kw = {} if R > 0 else dict(out_dtype=torch.float32)
            med[R], lo, hi = _timed([lambda w=w: fn(xr, w, **kw) for w in ws])
            what = f"rows R={R}" if R == 16 else f"wide R={R}" if R > 0 else "ops.gemm M=64"
            cols.append(f"{what} {med[R]:5.1f} ({lo:.1f} - {hi:.1f}) us {n * k * 2 / med[R] / 1e6:4.1f} TB/s")
        print(f"{name:10s} {n} x {k}: " + " | ".join(cols) + f" | 4 x rows16 / wide64 x {4 * med[16] / med[64]:.2f}", flush=True)
        del ws


def _timed(fns):
    """decode_bench's `timed`: one pass through the rotating copies captured into a HIP graph, median / min / max of 5 replays"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for f in fns[:2]:
            f()
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for f in fns:
                f()
    gr.replay()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / len(fns))
    runs.sort()
    return runs[2], runs[0], runs[-1]


def _gemv(x, w):
    lib = _lib.load()
    y = torch.empty(w.shape[0], device=dev)
    _lib.check(lib.kalle_gemv_bf16(ops._p(x), ops._p(w), w.stride(0), ops._p(y), 1, None, w.shape[0], w.shape[1], ops._stream()),
               "kalle_gemv_bf16")
    return y


if "--decode-wide" in sys.argv:
    decode_wide_bench()
    sys.exit(0)
if "--decode" in sys.argv:
    decode_bench([int(a) for a in sys.argv[sys.argv.index("--decode") + 1:]] or [1, 8, 16])
    sys.exit(0)
M = int(sys.argv[1]) if len(sys.argv) > 1 else 252
Mc = M // 126 * 130
shapes = [("qkv", M, 4608, 1536, {}), ("out+res", M, 1536, 1536, {"res": True}), ("q", M, 1536, 1536, {}), ("kv", Mc, 1536, 768, {}),
          ("ff1+glu", M, 12288, 1536, {"glu": True}), ("ff2+res", M, 1536, 6144, {"res": True})]
if len(sys.argv) > 2 and sys.argv[2]:
    shapes = [s for s in shapes if s[0] == sys.argv[2]]
mk = lambda r, c: (torch.randn(r, c, device=dev) * 0.5).bfloat16()
tot = 0.0
for name, m, n, k, opt in shapes:
    x, w = mk(m, k), mk(n, k)
    kw = {}
    if opt.get("res"):
        kw = dict(out_dtype=torch.float32, residual=torch.randn(m, n, device=dev))
    if opt.get("glu"):       # as dit_ops.ff_fwd: GLU projection with the SwiGLU in the epilogue
        hf, act = torch.empty(m, n, device=dev, dtype=torch.bfloat16), torch.empty(m, n // 2, device=dev, dtype=torch.bfloat16)
        kw = dict(bias=torch.randn(n, device=dev), out=hf, glu_mode=1, glu_inner=n // 2, glu_aux=act)
    fn = lambda: ops.gemm(x, w, **kw)
    assert fn() is not None, "shape not supported on this path"
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    # 20 launches inside one HIP graph: device time per launch without the host's per-call cost (~15 us of Python + ctypes)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(20):
                fn()
    gr.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 100 * 1e3
    plan = _lib.load().kalle_gemm_last_plan()
    if len(sys.argv) > 3:        # check against fp32 torch
        ref = x.float() @ w.float().t()
        got = fn()
        if opt.get("res"):
            ref = ref + kw["residual"]
        if not opt.get("glu"):
            print("   rel err", ((got.float() - ref).norm() / ref.norm()).item())
    tot += us * (2 if name in ("out+res",) else 1)
    print(f"{name:8s} M={m} N={n} K={k}: {us:6.1f} us  {2.0*m*n*k/us/1e6:6.0f} TFLOP/s  weights {n*k*2/us/1e6:5.2f} TB/s  plan {plan & 255}/s{plan >> 8}")
print(f"block total (out counted twice): {tot:.0f} us -> x24 = {tot*24/1e3:.2f} ms")
