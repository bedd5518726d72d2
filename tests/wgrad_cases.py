"""The case list of kalle_gemm_wgrad_group shared by tests/test_wgrad_group_gpu.py (runs them) and tests/test_wgrad_plan_cpu.py
(asserts, with the host query kalle_gemm_wgrad_group_plan alone, that every case gets the plan written here and that the list
reaches every region of the planner).  The shapes were found with that query, not guessed.

A problem is (tokens, N, K): dw [N][K] (+)= dy [tokens][N]^T x [tokens][K].  The tile count of a problem is
ceil(N / 256) * ceil(K / 256), so a problem with few rows and a wide K buys many tiles for little work; the planner runs a
multiple of 256 tiles whole and cuts the rest into 2 .. 12 token slices of ceil(ktiles / slices) 64-token K-tiles each, but
only where the shortest problem keeps 8 K-tiles per slice (16 K-tiles: more than 960 tokens)."""
import threading

SEVEN = [(4608, 1536), (1536, 1536), (1536, 1536), (1536, 768), (1536, 1536), (12288, 1536), (1536, 6144)]
BENCH_TOKENS = 8200            # the smallest token count (found with the query) at which SEVEN still gets the bench's mixed plan


def seven(tokens):
    """the seven weight gradients of a bench-width block; to_kv (K = 768) runs over the context tokens, 1024 more"""
    return [(tokens + (1024 if k == 768 else 0), n, k) for n, k in SEVEN]


# name -> (problems, (tiles, whole, slices))
CASES = {
    # ---- every tile whole: up to 960 tokens nothing is ever sliced; 8 / 64 / 72 tokens are one (ragged) and two K-tiles
    "whole-t8-nprob1": ([(8, 264, 136)], (2, 2, 0)),
    "whole-t64": ([(64, 264, 136), (64, 72, 520)], (5, 5, 0)),
    "whole-t72": ([(72, 520, 264), (72, 8, 8)], (7, 7, 0)),
    "whole-t512-nprob8": ([(512, 8 + 64 * i, 264 - 8 * i) for i in range(8)], (13, 13, 0)),
    "whole-t1024-two-rounds": ([(1024, 264, 256 * 255 + 8)], (512, 512, 0)),      # sliceable, but two full rounds of tiles
    # ---- every tile sliced: fewer than 256 tiles, at least 16 K-tiles
    "sliced-nprob1": ([(1024, 264, 136)], (2, 0, 2)),
    "sliced-two": ([(1024, 520, 264), (1024, 72, 520)], (9, 0, 2)),
    "sliced-short-last": ([(1088, 264, 136), (1088, 8, 8)], (3, 0, 2)),            # 17 K-tiles in 2 slices: 9 + 8
    "sliced-by-8": ([(4096, 512, 384), (4096, 256, 640), (4096, 128, 128)], (8, 0, 8)),
    "sliced-nprob8": ([(1152, 8 + 64 * i, 264 - 8 * i) for i in range(8)], (13, 0, 2)),
    "sliced-tokens-differ": ([(2048, 264, 136), (1024, 136, 264), (1096, 72, 8)], (5, 0, 2)),
    # ---- mixed: a multiple of 256 tiles whole, the tail sliced
    "mixed-inside-nprob1": ([(1024, 264, 256 * 150 + 136)], (302, 256, 2)),
    "mixed-inside-second": ([(1024, 264, 256 * 100), (1024, 264, 256 * 40 + 136), (1096, 72, 520)], (285, 256, 2)),
    "mixed-between": ([(1024, 264, 256 * 128), (1024, 72, 520), (1024, 264, 136)], (261, 256, 2)),
    "mixed-tokens-differ": ([(1024, 264, 256 * 150), (2048, 264, 136), (1032, 72, 520)], (305, 256, 2)),
    "mixed-bench-reduced": (seven(BENCH_TOKENS), (666, 512, 3)),
}

# cache replay: shape A, then shape B with the same (N, K) and another token count of the same 1024-token bucket; B's plan
# comes from the cache.  name -> (shapes (N, K), tokens A, tokens B, plan of A, plan of B after A)
REPLAY = {
    "up": ([(264, 136), (72, 520)], 1024, 1528, (5, 0, 2), (5, 0, 2)),              # 16 -> 24 K-tiles
    "down": ([(264, 136), (72, 264)], 2040, 1032, (4, 0, 4), (4, 0, 4)),            # 32 -> 17 K-tiles: slices of 5, 5, 5, 2
    "fewer-ktiles-than-slices": ([(264, 136), (8, 520)], 1016, 64, (5, 0, 2), (5, 5, 0)),   # 16 -> 1 K-tile: all whole
    "empty-trailing-slice": ([(264, 136), (8, 264)], 6144, 6152, (4, 0, 12), (4, 0, 12)),   # 96 -> 97 K-tiles: 10 x 9 + 7 + none
    "mixed-up": ([(264, 256 * 150 + 136)], 1024, 1984, (302, 256, 2), (302, 256, 2)),
}

REGIONS = ("all-whole", "all-sliced", "mixed", "boundary-inside-a-problem", "boundary-between-problems",
           "later-problem-all-sliced", "short-last-slice", "empty-trailing-slice", "nprob-1", "nprob-max", "tokens-differ",
           "single-k-tile", "ragged-k-tile", "ragged-whole", "ragged-sliced", "ragged-mixed", "cleared-edge-tile")


def fresh_thread(fn, *a, **kw):
    """fn(*a, **kw) on a new thread, whose plan cache is empty (the cache and the last-plan report are per thread)"""
    box = {}

    def run():
        try:
            box["v"] = fn(*a, **kw)
        except BaseException as e:  # noqa: BLE001 - re-raised below on the caller's thread
            box["e"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "e" in box:
        raise box["e"]
    return box["v"]


def ktiles(tokens):
    return (tokens + 63) // 64


def tiles_of(n, k):
    return ((n + 255) // 256) * ((k + 255) // 256)


def regions(problems, plan, overwrite):
    """the planner regions that a call with this plan (tiles, whole, slices) passes through"""
    tiles, whole, slices = plan
    assert tiles == sum(tiles_of(n, k) for _, n, k in problems)
    out = {"nprob-1"} if len(problems) == 1 else set()
    if len(problems) == 8:
        out.add("nprob-max")
    if len({t for t, _, _ in problems}) > 1:
        out.add("tokens-differ")
    out.add("all-whole" if whole == tiles else "all-sliced" if whole == 0 else "mixed")
    first = 0
    for t, n, k in problems:
        cnt = tiles_of(n, k)
        ragged = n % 64 != 0 and k % 64 != 0                   # edge tiles of 8 rows and of 8 columns
        w = min(max(whole - first, 0), cnt)                    # this problem's whole tiles
        if 0 < w < cnt:
            out.add("boundary-inside-a-problem")
        if w == cnt and first + cnt == whole < tiles:
            out.add("boundary-between-problems")
        if w == 0 and whole > 0:
            out.add("later-problem-all-sliced")
        if w > 0:
            if ktiles(t) == 1:
                out.add("single-k-tile")
            if t % 64:
                out.add("ragged-k-tile")
        if ragged:
            out.add("ragged-whole" if w == cnt else "ragged-sliced" if w == 0 else "ragged-mixed")
            if w < cnt and overwrite:
                out.add("cleared-edge-tile")
        if w < cnt:
            per = -(-ktiles(t) // slices)
            if (slices - 1) * per >= ktiles(t):
                out.add("empty-trailing-slice")
            elif ktiles(t) % per:
                out.add("short-last-slice")
        first += cnt
    return out
