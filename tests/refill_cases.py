"""Cases and host references shared by tests/test_llasa_refill_cpu.py, tests/test_kv_append_gpu.py and
tests/test_llasa_refill_gpu.py: kalle_kv_append_varlen (shapes, the base call every refusal departs from, a numpy reference on
bf16 bit patterns) and the ragged list `infer_batch(refill=True)` is driven with (frame caps, prompt lengths, rows, the map from
a schedule to the per-step noise of the host head).  numpy only; torch is the callers' business."""
import numpy as np

# ------------------------------------------------------------------------------------------------ kalle_kv_append_varlen
KV_ROWS = 32            # KALLE_KV_APPEND_ROWS: packed rows a workgroup moves
MAX_SEQ = 16            # KALLE_DECODE_MAX_ROWS


def _kv(name, H, Hkv, hd, lens, row0, total, dst, t0, R=6, cache_rows=40):
    """q|k|v buffer of (H + 2 Hkv) hd columns, the k|v window behind the H hd query columns"""
    return dict(id=name, ld=(H + 2 * Hkv) * hd, src_off=H * hd, kvw=2 * Hkv * hd, lens=list(lens), row0=list(row0), total=total,
                dst=list(dst), t0=list(t0), R=R, cache_rows=cache_rows)


# lengths 1, 7 and KV_ROWS + 1 (one row into a second workgroup); destination rows out of order; t0 0 and > 0; packed back to back
# (granule 8: the gap is behind the last sequence) and with gaps between the sequences; kvw 256 (head dim 64) and 1024 (128)
KV_CASES = [
    _kv("hd64-back-to-back", 4, 2, 64, (1, 7, KV_ROWS + 1), (0, 1, 8), 48, (5, 0, 3), (0, 0, 0)),
    _kv("hd64-gaps-t0", 4, 2, 64, (1, 7, KV_ROWS + 1), (0, 8, 16), 56, (5, 0, 3), (0, 4, 2)),
    _kv("hd128-gaps-t0", 8, 4, 128, (KV_ROWS + 1, 1, 7), (3, 40, 48), 64, (3, 5, 0), (7, 39, 0)),
    _kv("hd128-one", 8, 4, 128, (2 * KV_ROWS,), (0,), 64, (1,), (0,), R=2, cache_rows=2 * KV_ROWS),
]
KV_BASE = KV_CASES[1]   # the valid call every refusal changes ONE thing of (the GPU file runs it as it is)

# name -> overrides of KV_BASE that kalle_kv_append_varlen must refuse with KALLE_ERR_ARG before any launch
KV_REFUSALS = {
    "src NULL": dict(src=None),
    "cache NULL": dict(cache=None),
    "row0 NULL": dict(row0_ptr=None),
    "len NULL": dict(len_ptr=None),
    "dst_row NULL": dict(dst_ptr=None),
    "t0 NULL": dict(t0_ptr=None),
    "nseq 0": dict(nseq=0),
    "nseq 17": dict(nseq=MAX_SEQ + 1, lens=[1] * 17, row0=list(range(17)), dst=list(range(17)), t0=[0] * 17, R=16),
    "len 0": dict(lens=[1, 0, 33]),
    "len negative": dict(lens=[1, -7, 33]),
    "t0 negative": dict(t0=[0, -1, 2]),
    "t0 + len > cache_rows": dict(t0=[0, 4, 8]),
    "dst_row negative": dict(dst=[5, -1, 3]),
    "dst_row = R": dict(dst=[6, 0, 3]),
    "dst_row twice": dict(dst=[5, 3, 3]),
    "row0 + len > total_rows": dict(total=48),
    "overlapping": dict(row0=[0, 8, 14]),
    "unordered": dict(row0=[8, 0, 16], lens=[7, 1, 33]),
    "kvw % 8": dict(kvw=252),
    "ld_src % 8": dict(ld=516),
    "src_off % 8": dict(src_off=252),
    "cache_row_stride % 8": dict(stride=40 * 256 + 4),
}


def kv_append_ref(src, src_off, cache, row0, lens, dst, t0):
    """src uint16 [total, ld] (bf16 bit patterns), cache uint16 [R, cache_rows, kvw] -> the cache after the append (a copy):
    packed row row0[s] + j, columns src_off .. src_off + kvw, lands at cache[dst[s], t0[s] + j]"""
    out = np.array(cache, copy=True)
    kvw = out.shape[2]
    for s in range(len(lens)):
        for j in range(lens[s]):
            out[dst[s], t0[s] + j, :] = src[row0[s] + j, src_off:src_off + kvw]
    return out


# ------------------------------------------------------------------------------------------------ the refill list
CAPS = [6, 3, 8, 3, 5]          # frame caps of the five utterances: 14 steps on 2 rows, 16 with stop_lag=1, 19 grouped
ROWS = 2
# prompt positions: utterance 3 (3 positions) follows utterance 0 (14 + 5 positions) in row 0 - a refilled prompt SHORTER than
# what the row held, so the previous occupant's keys lie behind it in the buffer - and utterance 2 (33) follows utterance 1 (5 + 2)
PS = (14, 5, 33, 3, 9)


def occupants(frames, first, R):
    """{(step, row): (utterance, frame)} of a schedule given per utterance as (row, first_step) and the frames it ran"""
    out = {}
    for u, ((r, t), n) in enumerate(zip(first, frames)):
        for f in range(n):
            assert (t + f, r) not in out, "two utterances in one row at one step"
            out[(t + f, r)] = (u, f)
    return out


def step_noise(noise, frames, first, R, steps):
    """noise [frames, utterances, lat] -> [steps, R, lat]: what each row of the batch must draw at each global step so that
    utterance u's frame f reads noise[f, u] (zeros where a row is empty) - the feed of the host head, whose one draw per step
    covers all R rows"""
    out = np.zeros((steps, R, noise.shape[2]), dtype=noise.dtype)
    for (s, r), (u, f) in occupants(frames, first, R).items():
        out[s, r] = noise[f, u]
    return out
