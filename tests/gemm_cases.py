"""The case list of kalle_gemm_bf16's dispatcher, shared by tests/test_gemm_epilogue_gpu.py (runs the epilogue tables below on the
GPU) and tests/test_gemm_plan_cpu.py (asserts, with the host query kalle_gemm_plan alone, that every case of CASES gets the
return code and plan word recorded in tests/golden/gemm_plans.json, and that the list reaches every family of the planner).

A case is a dict: M, N, K and whatever differs from DEFAULTS.  The epilogue fields say only WHETHER a field is set (gate and
remap: its rows per batch), which is all the planner looks at; `ws` is the scratch the caller lends: "lend" (what ops.gemm
lends: 64 MiB or 8 fp32 slabs, for M <= 4096 and a k-contiguous A), "none", "odd" (the lent one at a pointer that is not 16-byte
aligned) or a byte count.  The table is keyed by key(case), so cases can be added without touching the rows of the others.  It was recorded from the dispatcher as it was before plan_gemm existed (every launch made a
no-op, kalle_gemm_last_plan read back), every case on a fresh thread; the sweep's shapes were found with that recorder."""
import itertools
import random

from wgrad_cases import fresh_thread  # noqa: F401 - a new thread: an empty cache of mixed split-K plans, last-plan word 0

DEFAULTS = dict(akm=0, bkm=0, f32=True, bias=False, gate=0, residual=False, mask=False, remap=0, accumulate=False, alpha=1.0,
                glu=0, inner=0, ws="lend")


def case(M, N, K, **kw):
    """a case in canonical form; accepts a Spec's fields (remap as a tuple, paddings, expected plan: dropped)"""
    c = dict(M=M, N=N, K=K)
    for k, d in DEFAULTS.items():
        v = kw.get(k, d)
        if k == "remap":
            v = v[0] if isinstance(v, tuple) else v or 0
        if v != d:
            c[k] = v
    assert not set(kw) - set(DEFAULTS) - {"ldc_pad", "ldr_pad", "ldg_pad", "plan", "slices", "seed"}, kw
    return c


def key(c):
    return " ".join([f"{c['M']}x{c['N']}x{c['K']}"] + [f"{k}={c[k]}" for k in DEFAULTS if k in c])


def plan_kwargs(c):
    """the arguments of ops.gemm_plan for a case"""
    g = {**DEFAULTS, **c}
    ws = g["ws"]
    kw = dict(a_kmajor=bool(g["akm"]), b_kmajor=bool(g["bkm"]), f32=g["f32"], bias=g["bias"], gate=bool(g["gate"]),
              rows_per_batch=g["gate"], residual=g["residual"], accumulate=g["accumulate"], alpha=g["alpha"],
              c_rows_per_batch=g["remap"], row_mask=g["mask"], glu_mode=g["glu"], glu_inner=g["inner"],
              workspace="lend" if ws == "odd" else None if ws == "none" else ws, workspace_ptr=24 if ws == "odd" else 16)
    return (g["M"], g["N"], g["K"]), kw


# ------------------------------------------------------------------------------------------------ the epilogue test's tables
# (plan, base shape (M, N, K), layout) - the M / N / K of most are ragged: M % 16 == 1, N % 64 != 0, K % 64 != 0
P5 = dict(M=2017, N=1472, K=1480, plan=5, slices=False)          # small tiles (128 x 128), whole K
P5S = dict(M=252, N=1536, K=6144, plan=5, slices=True)           # small tiles + K slices + finishing pass
P5B = dict(M=2017, N=1536, K=1480, bkm=1, plan=5)                # small tiles, k-major B (data gradient)
P4 = dict(M=2529, N=1544, K=4104, plan=4)                        # few-rows K slices + finishing pass
P4B = dict(M=2520, N=1536, K=6144, bkm=1, plan=4)
P3 = dict(M=8193, N=1544, K=1544, plan=3)                        # persistent 256 x 256
P3B = dict(M=8193, N=1536, K=1480, bkm=1, plan=3)
P2 = dict(M=5000, N=192, K=1544, plan=2)                         # 256 x 128
P2B = dict(M=5000, N=192, K=1544, bkm=1, plan=2)
P1 = dict(M=5000, N=64, K=1544, plan=1)                          # v1 128 x 128
P1A = dict(M=520, N=1536, K=1544, akm=1, plan=1)                 # v1: k-major A with a k-contiguous B
ROUTES = {"p5": P5, "p5s": P5S, "p5b": P5B, "p4": P4, "p4b": P4B, "p3": P3, "p3b": P3B, "p2": P2, "p2b": P2B, "p1": P1,
          "p1a": P1A}

# the epilogues the product uses (dit_ops.py), on every plan: rows_per_batch 126 = tokens per clip of the benchmark
PRODUCT = {
    "attn_out_f32": dict(residual=True, gate=126, mask=True),               # self-attention out-projection (dit_ops.py:236)
    "attn_out_bf16": dict(f32=False, residual=True, gate=126, mask=True),
    "ff_out": dict(bias=True, gate=126, residual=True),                     # FF-out (dit_ops.py:388)
    "xattn_out": dict(residual=True, mask=True),                            # cross-attention out
    "proj_in_off1": dict(bias=True, remap=(125, 130, 1)),                   # project_in behind 1 / 4 prepended tokens
    "proj_in_off4": dict(bias=True, residual=True, remap=(126, 130, 4)),
    "dgrad_acc": dict(accumulate=True, alpha=0.37),                          # data-gradient accumulate
    "qkv_bf16": dict(f32=False, bias=True),
}

# seeded pairwise cover of every option on every plan: rows_per_batch values put batch boundaries inside tiles
FACTORS = {
    "f32": [True, False],
    "bias": [False, True],
    "gate": [0, 1, 126, 130, 257],
    "residual": [False, True],
    "mask": [False, True],
    "remap": [None, (126, 130, 1), (130, 133, 3), (257, 260, 0)],
    "accumulate": [False, True],
    "alpha": [1.0, 0.37, -1.5, 0.0],
    "ldc_pad": [0, 24],
}


def pairwise_valid(c):
    return not (c["accumulate"] and not c["f32"])


def _pairwise(seed, n_cand=400):
    rnd = random.Random(seed)
    keys = list(FACTORS)
    need = {(k1, i1, k2, i2) for k1, k2 in itertools.combinations(keys, 2)
            for i1 in range(len(FACTORS[k1])) for i2 in range(len(FACTORS[k2]))
            if pairwise_valid({**{k: FACTORS[k][0] for k in keys}, k1: FACTORS[k1][i1], k2: FACTORS[k2][i2]})}
    rows = []
    while need:
        best, best_cov = None, -1
        for _ in range(n_cand):
            ix = {k: rnd.randrange(len(FACTORS[k])) for k in keys}
            c = {k: FACTORS[k][i] for k, i in ix.items()}
            if not pairwise_valid(c):
                continue
            cov = sum((k1, ix[k1], k2, ix[k2]) in need for k1, k2 in itertools.combinations(keys, 2))
            if cov > best_cov:
                best, best_cov, best_ix = c, cov, ix
        rows.append(best)
        need -= {(k1, best_ix[k1], k2, best_ix[k2]) for k1, k2 in itertools.combinations(keys, 2)}
    return rows


PAIRWISE = _pairwise(20261016)
PAIRWISE_ROUTES = ("p5", "p5s", "p4", "p3", "p2", "p1")

# weight gradients: a_kmajor (dy^T x, K = tokens), fp32 out
# (id, shape, plan of a plain call, plan with epilogue fields: without the split the 256 x 128 tiles fill the chip better at 1536 x 1536)
WGRAD = [
    ("p3-split", dict(M=1536, N=1536, K=32256), 3, 2),          # split / mixed split at the bench's token count
    ("p3-split-ff", dict(M=6144, N=1536, K=32256), 3, 3),
    ("p2-split", dict(M=1536, N=192, K=32256), 2, 2),
    ("p2-ragged", dict(M=1544, N=1544, K=4104), 2, 2),
]
WGRAD_EPI = {"over": dict(), "over-alpha": dict(alpha=0.37), "acc": dict(accumulate=True),
             "acc-alpha": dict(accumulate=True, alpha=-1.5), "bias-res": dict(bias=True, residual=True, alpha=0.5),
             "gate-mask": dict(gate=257, mask=True, ldc_pad=24)}

# fused SwiGLU forward: id -> (M, inner, K, plan)
GLU1 = {
    "p3-384": (5000, 384, 1544, 3), "p3-640": (5000, 640, 1536, 3), "p3-6144": (4113, 6144, 1536, 3),   # 256 x 256: 3 / 5 / 48 column tiles
    "p5-96": (1000, 96, 520, 5), "p5-160": (2017, 160, 1480, 5),                                       # small tiles, inner % 32 == 0
    "p4-768": (2520, 768, 4096, 4), "p4-100": (300, 100, 1024, 4),                                     # few-rows finishing pass (inner % 4 == 0)
}
# fused SwiGLU backward: id -> (M, inner, K, alpha)
GLU2 = {"384": (5000, 384, 1544, 1.0), "640-alpha": (5000, 640, 1536, 0.37), "6144": (4113, 6144, 1536, 1.0),
        "m257-alpha": (257, 128, 1024, -1.5), "m2017": (2017, 640, 1480, 1.0)}

# combinations no fused kernel takes: None from ops.gemm (kalle_gemm_bf16: KALLE_ERR_UNSUPPORTED), C and glu_aux untouched
UNSUPPORTED = {
    "glu1-gate-few-rows": (1, dict(M=2520, inner=768, K=4096), dict(gate=126)),
    "glu1-residual-few-rows": (1, dict(M=2520, inner=768, K=4096), dict(residual=True)),
    "glu1-mask-few-rows": (1, dict(M=2520, inner=768, K=4096), dict(mask=True)),
    "glu1-remap-few-rows": (1, dict(M=2520, inner=768, K=4096), dict(remap=(126, 130, 1))),
    "glu1-gate-p3": (1, dict(M=5000, inner=384, K=1536), dict(gate=126)),
    "glu1-residual-p5": (1, dict(M=1000, inner=96, K=512), dict(residual=True)),
    "glu1-alpha-p3": (1, dict(M=5000, inner=384, K=1536), dict(alpha=0.5)),
    "glu1-alpha-p5": (1, dict(M=1000, inner=96, K=512), dict(alpha=0.5)),
    "glu1-alpha-few-rows": (1, dict(M=2520, inner=768, K=4096), dict(alpha=0.5)),
    "glu1-f32": (1, dict(M=5000, inner=384, K=1536), dict(f32=True)),
    "glu1-inner-not-128-large": (1, dict(M=5000, inner=96, K=1536), dict()),
    "glu2-few-rows": (2, dict(M=200, inner=384, K=1536), dict()),
    "glu2-bias": (2, dict(M=5000, inner=384, K=1536), dict(bias=True)),
    "glu2-residual": (2, dict(M=5000, inner=384, K=1536), dict(residual=True)),
    "glu2-gate": (2, dict(M=5000, inner=384, K=1536), dict(gate=126)),
    "glu2-mask": (2, dict(M=5000, inner=384, K=1536), dict(mask=True)),
    "glu2-inner-not-128": (2, dict(M=5000, inner=200, K=1536), dict()),
}

HEADLINE_M = 126 * 256
HEADLINE = {
    "qkv": dict(M=HEADLINE_M, N=4608, K=1536, f32=False, bias=True, plan=3),
    "attn_out": dict(M=HEADLINE_M, N=1536, K=1536, residual=True, gate=126, plan=3),
    "attn_out_mask": dict(M=HEADLINE_M, N=1536, K=1536, residual=True, gate=126, mask=True, plan=3),
    "ff_out": dict(M=HEADLINE_M, N=1536, K=6144, bias=True, gate=126, residual=True, plan=3),
    "ff_out_dgrad": dict(M=HEADLINE_M, N=1536, K=1536, bkm=1, accumulate=True, alpha=0.5, plan=3),
    "ragged_m": dict(M=HEADLINE_M - 8, N=1536, K=1536, residual=True, gate=126, mask=True, ldc_pad=8, plan=3),
    "persist_16100": dict(M=16100, N=4608, K=1536, f32=False, bias=True, gate=130, plan=3),
}
HEADLINE_GLU = (HEADLINE_M, 6144, 1536)


def glu1_case(M, inner, K, **kw):
    return case(M, 2 * inner, K, **{**dict(f32=False, bias=True, glu=1, inner=inner), **kw})


def glu2_case(M, inner, K, **kw):
    return case(M, inner, K, **{**dict(bkm=1, f32=False, glu=2, inner=inner), **kw})


def epilogue_cases():
    """every kalle_gemm_bf16 call of tests/test_gemm_epilogue_gpu.py"""
    out = [case(**{**r, **e}) for r in ROUTES.values() for e in PRODUCT.values()]
    out += [case(**{**ROUTES[r], **c}) for r in PAIRWISE_ROUTES for c in PAIRWISE]
    for _, shape, _, _ in WGRAD:
        out += [case(akm=1, bkm=1, f32=True, **shape, **e) for e in WGRAD_EPI.values()]
    out += [glu1_case(M, inner, K) for M, inner, K, _ in GLU1.values()] + [glu1_case(*HEADLINE_GLU)]
    out += [glu2_case(M, inner, K, alpha=a) for M, inner, K, a in GLU2.values()] + [glu2_case(*HEADLINE_GLU)]
    for mode, shp, ex in UNSUPPORTED.values():
        if mode == 1:
            out.append(glu1_case(shp["M"], shp["inner"], shp["K"], **{"f32": False, **ex}))
        else:
            out.append(glu2_case(shp["M"], shp["inner"], shp["K"], **ex))
    out += [case(**h) for h in HEADLINE.values()]
    return out


# ------------------------------------------------------------------------------------------------ the bench step
BENCH_ROWS = (252, 504, 2016, 4032, 32256)          # tokens of a step at 2, 4, 16, 32 and 256 clips of 126
BENCH_WEIGHTS = [(4608, 1536), (1536, 1536), (3072, 768), (12288, 1536), (1536, 6144)]      # [out][in] at model width 1536


def bench_cases():
    """forward, data-gradient and weight-gradient GEMMs of a DiT block at the bench's width: inner 6144, FF-in 12288 wide"""
    out = []
    for rows in BENCH_ROWS:
        for n, k in BENCH_WEIGHTS:
            out += [case(rows, n, k, f32=False, bias=True), case(rows, n, k, residual=True, gate=126, mask=True),
                    case(rows, n, k, bias=True, gate=126, residual=True), case(rows, n, k, f32=False),
                    case(rows, k, n, bkm=1), case(rows, k, n, bkm=1, accumulate=True, alpha=0.5), case(rows, k, n, bkm=1, f32=False),
                    case(n, k, rows, akm=1, bkm=1), case(n, k, rows, akm=1, bkm=1, accumulate=True)]
        out += [glu1_case(rows, 6144, 1536), glu2_case(rows, 6144, 1536)]
    return out


# ------------------------------------------------------------------------------------------------ sweep
def sweep_cases():
    out = []
    Ms = (8, 136, 256, 264, 520, 1000, 2048, 2056, 2520, 4096, 4104, 16104)
    Ns = (8, 64, 72, 128, 192, 640, 1536, 4608)
    Ks = (8, 520, 1024, 1480, 4096, 12288)
    for M, N, K in itertools.product(Ms, Ns, Ks):
        out += [case(M, N, K), case(M, N, K, f32=False, bias=True), case(M, N, K, bkm=1), case(M, N, K, akm=1, bkm=1)]
    # weight gradients over token counts: uniform and mixed atomic split-K of both big-tile kernels, epilogue fields turn it off
    for M, N in ((1536, 1536), (4608, 1536), (6144, 1536), (1536, 768), (1536, 192), (2056, 8456), (264, 136), (256, 128)):
        for K in (512, 960, 1024, 1032, 1088, 2016, 4032, 8200, 16128, 32256, 65536):
            out += [case(M, N, K, akm=1, bkm=1), case(M, N, K, akm=1, bkm=1, accumulate=True),
                    case(M, N, K, akm=1, bkm=1, bias=True), case(M, N, K, akm=1, bkm=1, f32=False), case(M, N, K, akm=1)]
    # the scratch: none, too short for two slabs, 2 / 3 / 5 slabs, misaligned
    for M, N, K in ((252, 1536, 6144), (504, 1536, 6144), (1008, 4608, 12288), (2520, 1536, 6144), (2529, 1544, 4104), (4032, 1536, 6144)):
        for ws in ("none", "odd", 8 * M * N - 16, 8 * M * N, 12 * M * N, 20 * M * N):
            out += [case(M, N, K, ws=ws), case(M, N, K, bkm=1, ws=ws)]
        out += [case(M, N, K), case(M, N, K, bkm=1), glu1_case(M, N // 2, K), glu1_case(M, N // 2, K, ws="none")]
    # fused SwiGLU over the families' tile rules: inner % 128 (256 x 256), % 32 (small tiles), % 4 (finishing pass)
    for M in (200, 1000, 2017, 2520, 4096, 5000):
        for inner in (96, 100, 104, 128, 160, 384, 768):
            for K in (512, 1536, 4096):
                out += [glu1_case(M, inner, K), glu2_case(M, inner, K)]
    # refused arguments
    out += [case(256, 260, 512), case(256, 256, 516), case(260, 256, 512, akm=1, bkm=1), case(256, 256, 516, bkm=1),
            case(256, 256, 512, f32=False, accumulate=True), case(0, 256, 512), glu1_case(1000, 0, 512),
            glu1_case(5000, 384, 1536, accumulate=True), glu2_case(5000, 384, 1536, accumulate=True)]
    return out


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


CASES = _unique(epilogue_cases() + bench_cases() + sweep_cases())

# Cache replay: the smallest weight gradient (found with the query) whose fresh plan is mixed - 130 tiles of 256 x 256, 96 K-tiles -
# and a second K of the same 16-K-tile bucket whose own fresh plan is uniform: (M, N, K launched, its plan, K queried, its own plan)
REPLAY = (2560, 3328, 6144, 0x1000303, 6208, 0x303)
