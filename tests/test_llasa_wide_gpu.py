"""-m gpu: `infer_batch(rows=R)` above 16 rows - the wide decode step, the device heads in chunks of 16 rows, prefill_rows with
more than 16 prompts - on the tiny Llama of the golden Llasa configs (gen_oracle.CASES).

7  device head, explicit noise, grouped: 40 prompts with rows=64 and rows=33 return, per utterance, the BITS of rows=None (groups
   of 16) - both task models, stop_lag 0 and 1, per-prompt caps, and a threshold in the middle of the free run's frame KLs so that
   rows leave through the KL rule at different frames.
8  host head against the fp64 oracle of tests/gen_oracle.py with its yardstick (nothing new measured): rows=33 grouped, and
   rows=33 with refill=True on 70 prompts with per-prompt caps, the trace equal to refill_steps; prefill_rows with 33 prompts at
   once, the hidden states and a following 33-row decode step against the fp64 row forward.
9  one seeded defect per path: the head of one chunk of 16 rows given the other chunk's active flags fails the bit comparison of
   7; the packed prefill's KV append without the block offset on the cache fails the fp64 check of the refill run of 8 by more
   than WRONG_MARGIN x its bound.  (The sequencer's own chunk defect - attention over chunk 0's caches - is seeded in
   tests/test_decode_wide_gpu.py.)"""
import contextlib
import ctypes
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle as go  # noqa: E402
import gen_oracle2 as g2  # noqa: E402
import test_generation_oracle_gpu as t1  # noqa: E402
import test_llasa_refill_gpu as tf  # noqa: E402
import test_model_llasa_gen_oracle_gpu as t2  # noqa: E402
from test_llasa_batch_gpu import fixed_noise  # noqa: E402

WRONG_MARGIN = 2.0
N7, TOP = 40, 9
CAPS7 = [TOP - u % 5 for u in range(N7)]            # (period 5: rows r and r + 16 of a group never share a cap)


def frame_kls(model, outs, lat):
    """the stop quantity of every returned frame, from what infer_batch returns ([1, w, n] per utterance)"""
    e = math.e
    kls = []
    for o, nz in outs:
        x = o[0].t().double().cpu()
        if model == 1:      # the sampled latent: mean = latent - std * noise
            m = x - go.STD * nz.double()
            kls.append((math.log(e / go.STD) + (go.STD ** 2 + (m - 1) ** 2) / (2 * e * e) - 0.5).sum(1) / lat)
        else:               # mean || log-scale
            m, logs = x[:, :lat], x[:, lat:]
            kls.append(((1 - logs) + (torch.exp(logs) ** 2 + (m - 1) ** 2) / (2 * e * e) - 0.5).sum(1) / lat)
    return kls


def setup7(model, dev, tmp_path):
    c = (go if model == 1 else g2).CASES[0]
    m = (t1 if model == 1 else t2).build(c, dev, tmp_path)
    ps = t1.on_device(go.many_prompts(c, N7, tag="wide"), dev)
    noise = tf.draw(c, TOP, N7, 70 + model)
    return c, m, ps, noise


def grouped7(m, ps, noise, dev, lag, thres, rows):
    return m.infer_batch(ps, end_disp_kl_thres=thres, max_length=CAPS7, device_head=True, noise=noise.to(dev), stop_lag=lag, rows=rows)


@pytest.mark.parametrize("model", [1, 2], ids=["head", "head2"])
def test_wide_groups_return_the_bits_of_groups_of_16(dev, tmp_path, model):
    c, m, ps, noise = setup7(model, dev, tmp_path)
    free = grouped7(m, ps, noise, dev, 0, -1.0, None)
    assert [o.shape[2] for o in free] == [n - 1 for n in CAPS7]
    kls = frame_kls(model, [(o, noise[:o.shape[2], u]) for u, o in enumerate(free)], c["lat"])
    later = torch.cat([k[4:] for k in kls])                 # the rule stops at frames i > 3
    thres = float(later.median())
    for lag in (0, 1):
        base = grouped7(m, ps, noise, dev, lag, thres, None)
        frames = [o.shape[2] for o in base]
        assert len(set(f - n for f, n in zip(frames, CAPS7))) > 1, "no row left through the KL rule before its cap"
        assert min(frames) >= 4 and any(f == n - 1 for f, n in zip(frames, CAPS7))
        for rows in (64, 33):
            got = grouped7(m, ps, noise, dev, lag, thres, rows)
            same = [torch.equal(a, b) for a, b in zip(got, base)]
            assert len(got) == N7 and all(same), (model, lag, rows, [u for u, s in enumerate(same) if not s])
        assert all(torch.equal(a, b) for a, b in zip(grouped7(m, ps, noise, dev, lag, thres, 16), base))


def test_a_chunk_given_the_other_chunks_active_flags_is_caught(dev, tmp_path):
    """rows=32: two head chunks of 16 per frame.  With their active lists exchanged the utterances whose caps differ from their
    partner's 16 rows away get frames they should not (or miss ones they should), and the bit comparison of 7 fails"""
    from kalle_audio_amd import ops
    c, m, ps, noise = setup7(1, dev, tmp_path)
    base = grouped7(m, ps, noise, dev, 0, -1.0, None)
    assert all(torch.equal(a, b) for a, b in zip(grouped7(m, ps, noise, dev, 0, -1.0, 32), base))
    real = ops._head_call

    def exchanged(*a, **k):
        desc, calls = real(*a, **k)
        if len(calls) == 2 and calls[0][1] == calls[1][1] == 16:
            calls = [calls[0][:3] + (calls[1][3],), calls[1][:3] + (calls[0][3],)]
        return desc, calls

    ops._head_call = exchanged
    try:
        bad = grouped7(m, ps, noise, dev, 0, -1.0, 32)
    finally:
        ops._head_call = real
    assert not all(torch.equal(a, b) for a, b in zip(bad, base))


# ------------------------------------------------------------------------------------------------ 8: host head against fp64
def host_run(m, dev, prompts, caps, noise, feed, nan=True, **kw):
    """infer_batch under the host head with `feed` (one draw [R, 1, lat] per head call, in call order): latents per utterance.
    nan: the batch caches start as NaN instead of zeros"""
    ps = t1.on_device(prompts, dev)
    with (tf.nan_cache(m.base_model.model) if nan else contextlib.nullcontext([])) as made:
        fixed_noise(m, [f.to(dev) for f in feed])
        try:
            outs = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=caps, **kw)
        finally:
            del m.sample
    return [o[0].t().contiguous().cpu() for o in outs], [tuple(cache["kv"][0].shape) for cache in made]


def test_grouped_rows_33_host_head_against_fp64(dev, tmp_path):
    c = go.CASES[0]
    m = t1.build(c, dev, tmp_path)
    n = 40
    prompts = go.many_prompts(c, n, tag="wide8")
    caps = [4 + (u * 3) % 4 for u in range(n)]
    noise = tf.draw(c, max(caps), n, 81)
    feed = []
    for i in range(0, n, 33):                               # a group runs max(its caps) head calls, row r = utterance i + r
        g = caps[i:i + 33]
        feed += [noise[f, i:i + len(g)].reshape(len(g), 1, -1) for f in range(max(g))]
    lats, made = host_run(m, dev, prompts, caps, noise, feed, rows=33)
    assert [s[0] for s in made] == [33, 7]
    tf.check1(c, None, prompts, lats, noise, caps, f"WIDE 8 grouped rows=33 {c['id']}", ("W8", "grouped"))


def test_refill_rows_33_host_head_against_fp64(dev, tmp_path):
    c = go.CASES[0]
    m = t1.build(c, dev, tmp_path)
    n, R = 70, 33
    prompts = go.many_prompts(c, n, tag="wide8r")
    caps = [3 + (u * 7) % 5 for u in range(n)]
    noise = tf.draw(c, max(caps), n, 82)
    total, first, trace = tf.schedule(caps, R, 0)
    feed = torch.from_numpy(tf.rc.step_noise(noise.numpy(), caps, first, R, total)).view(total, R, 1, c["lat"])
    lats, made = host_run(m, dev, prompts, caps, noise, list(feed), rows=R, refill=True)
    assert m.last_refill_trace == trace
    assert len(made) == 1 and made[0][0] == R
    ref = tf.check1(c, None, prompts, lats, noise, caps, f"WIDE 8 refill rows=33 {c['id']}", ("W8", "refill"))
    # 9, the seeded defect of this path: the packed prefill's KV append forgets the block offset on the CACHE (every block of 16
    # rows lands in rows 0 .. 15), so the prompts of rows >= 16 are never written (the caches start as zeros here: nothing is
    # NaN) and rows < 16 hold other prompts' keys.  The same check against the oracle teacher-forced on what THAT run fed back
    # must fail, by more than WRONG_MARGIN x its bound of M r
    from kalle_audio_amd import _lib, ops
    real = ops.kv_append_varlen

    def block_offset_dropped(src, seqs, cache, dst_rows, t0, *, src_off):
        R, cache_rows, kvw = cache.shape
        assert R == 33
        cast, lib = ctypes.cast, _lib.load()
        for b0 in range(0, R, 16):
            pick = [q for q, d in enumerate(dst_rows) if b0 <= int(d) < b0 + 16]
            if pick:
                arr = lambda v: cast(ops._i32(v), ctypes.c_void_p)
                ops.check(lib.kalle_kv_append_varlen(ops._p(src), src.stride(0), src_off, ops._p(cache[0:16]), cache.stride(0), kvw, len(pick),
                                                     arr([seqs.row0[q] for q in pick]), arr([seqs.lens[q] for q in pick]),
                                                     arr([int(dst_rows[q]) - b0 for q in pick]), arr([t0[q] for q in pick]), seqs.total_rows,
                                                     16, cache_rows, ops._stream()), "kalle_kv_append_varlen")
        return cache

    ops.kv_append_varlen = block_offset_dropped
    try:
        bad, _ = host_run(m, dev, prompts, caps, noise, list(feed), nan=False, rows=R, refill=True)
    finally:
        ops.kv_append_varlen = real
    assert m.last_refill_trace == trace and all(torch.isfinite(b).all() for b in bad)
    means = [l.double() - go.STD * noise[:len(l), u].double() for u, l in enumerate(bad)]
    x64 = ref["cut"](go.forward(c, t1.weights(c["id"], None), go.teacher_rows(prompts, bad, None)))
    msg = go.failure(means, x64, ref["r"], "KV append without the block offset", offsets=[P - 1 for P in ref["Ps"]], P=ref["Ps"])
    print("WIDE 9:", msg)
    assert msg is not None
    assert go.worst(means, x64)[0] > WRONG_MARGIN * go.M * ref["r"]


def test_prefill_rows_33_prompts_at_once(dev, tmp_path):
    """test_prefill_rows_against_fp64 with 33 prompts into the rows of a 40-row cache, then one 40-row (wide) decode step"""
    from kalle_audio_amd import ops
    c = go.CASES[0]
    PS = tuple(1 + (5 * i) % 23 for i in range(33))
    rows = [(7 * i + 3) % 40 for i in range(33)]            # distinct (7 and 40 are coprime), spread over all three blocks of 16
    room = 30
    xs = go.scripted_rows(c, PS, 1, tag="prefill_rows_wide")
    model = t1.build(c, dev, tmp_path).base_model.model
    D = xs[0].shape[1]
    with tf.nan_cache(model):
        cache = model.init_cache_batch(40, room, dev)
    got = model.prefill_rows([x[:P].to(dev)[None].contiguous() for x, P in zip(xs, PS)], cache, rows)
    assert got.shape == (33, 1, D)
    assert ops.attn_last_plan() == 8 | c["hd"] << 8, hex(ops.attn_last_plan())
    want_len = [0] * 40
    for r, P in zip(rows, PS):
        want_len[r] = P
    assert cache["len"] == want_len
    step = torch.full((40, 1, D), float("nan"))
    for x, P, r in zip(xs, PS, rows):
        step[r, 0] = x[P]
    nxt = model.forward_cached_batch(step.to(dev), cache, [n > 0 for n in want_len])
    for kv in cache["kv"]:
        k = kv.float().cpu()
        for r, n in enumerate(cache["len"]):
            assert not torch.isnan(k[r, :n]).any() and torch.isnan(k[r, n:]).all(), r
    W = t1.weights(c["id"], None)
    ref = [dict(x=x, P=P) for x, P in zip(xs, PS)]
    f64, emu = go.forward(c, W, ref), go.forward(c, W, ref, "emu")
    have = [torch.stack([got[i, 0], nxt[r, 0]]).float().cpu() for i, r in enumerate(rows)]
    cut = lambda outs: [o["hidden"][o["P"] - 1:o["P"] + 1] for o in outs]
    r = go.worst(cut(emu), cut(f64))[0]
    tf.hold(have, cut(f64), r, f"WIDE 8 prefill_rows 33 prompts {c['id']}", ("W8", "prefill"), offsets=[P - 1 for P in PS], P=list(PS))
    with pytest.raises(ValueError, match="1 .. 64"):
        model.init_cache_batch(65, room, dev)


def test_e4m3_with_more_than_16_rows_is_refused(dev, tmp_path):
    c = go.CASES[0]
    m = t1.build(c, dev, tmp_path, go.FMTS[1])
    ps = t1.on_device(go.many_prompts(c, 20, tag="wide"), dev)
    with pytest.raises(NotImplementedError, match=r"(?s)e4m3.*17"):
        m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=4, rows=17)
    for bad in (0, 65, 2.5, "8"):
        with pytest.raises(ValueError, match="rows"):
            m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=4, rows=bad)
    assert len(m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=4, rows=16)) == 20
