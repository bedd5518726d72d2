"""-m gpu: `infer_batch(refill=True)` and LlamaModel.prefill_rows held to the fp64 oracles of tests/gen_oracle.py (fixed-std head)
and tests/gen_oracle2.py (mean || log-scale head), with their yardstick and M = 3, on the tiny Llama configs of gen_oracle.CASES
(head dims 64 and 128).

0  nothing that existed moved: refill=False returns the same bits before and after a refill run; one prompt is `infer`; [] is [].
A  prefill_rows: prompts of 1 / 14 / 250 positions into rows 2, 0, 1 of a NaN-filled 4-row cache, the returned hidden states and
   a following forward_cached_batch step against the fp64 row forward; lengths, the untouched row, the attention plan word.
B  refill end to end: five prompts on two rows with frame caps [6, 3, 8, 3, 5] and explicit noise, both task models, host head
   and device head (stop_lag 0 and 1), bf16 and e4m3: the trace equals refill_steps, every returned frame within the bound of the
   oracle teacher-forced on the latents the path fed back.  The batch cache starts as NaN (a spy on init_cache_batch), so a read
   of a previous occupant's positions - utterance 3 is shorter than what row 0 held before it - would surface as NaN.
C  defects seeded into the oracle that the device's tensors fail: the previous occupant's keys visible, rotary positions going on
   from the previous occupant's length, the neighbouring utterance's noise, two utterances swapped.
D  the stop rule: rows leaving through the KL rule at different frames (host head), stop_lag 1 against 0 (device head).
E  no row ever refilled (prompts <= rows), and 17 prompts on 16 rows."""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_oracle as go  # noqa: E402
import gen_oracle2 as g2  # noqa: E402
import refill_cases as rc  # noqa: E402
import test_generation_oracle_gpu as t1  # noqa: E402
import test_model_llasa_gen_oracle_gpu as t2  # noqa: E402
from test_llasa_batch_gpu import build as tiny_build, fixed_noise  # noqa: E402
from test_model_llasa_generation_gpu import host_noise  # noqa: E402

ko = go.ko
HEADS = ("host", "dev0", "dev1")
CAPS, ROWS, N = rc.CAPS, rc.ROWS, len(rc.CAPS)
KEEP, MEASURED = {}, {}


def prompts_of(c):
    return go.ragged_prompts(c, rc.PS, tag="refill")


def draw(c, frames, n, seed):
    return torch.randn(frames, n, c["lat"], generator=torch.Generator().manual_seed(seed))


@contextlib.contextmanager
def nan_cache(model):
    """every batch cache the model makes starts as NaN instead of zeros"""
    init, made = model.init_cache_batch, []

    def spy(*a, **k):
        cache = init(*a, **k)
        for kv in cache["kv"]:
            kv.fill_(float("nan"))
        made.append(cache)
        return cache

    model.init_cache_batch = spy
    try:
        yield made
    finally:
        del model.init_cache_batch


@contextlib.contextmanager
def rows_per_step(m, rows):
    m.infer_batch_rows = rows
    try:
        yield
    finally:
        del m.infer_batch_rows


def schedule(caps, rows, lag):
    from kalle_audio_amd.model_sigmaVAE import refill_steps
    total, first = refill_steps(caps, rows, stop_lag=lag)
    return total, first, [(u, r, t, n) for u, ((r, t), n) in enumerate(zip(first, caps))]


def hold(xs, x64s, r, what, key, offsets=None, P=None):
    v, row, i = go.worst(xs, x64s)
    print(f"REFILL {what}: worst ratio {v:.3e} = {v / r:.2f} r at utterance {row} index {i} (r {r:.3e}); "
          f"{sum(len(x) for x in xs)} frames")
    MEASURED[key] = max(MEASURED.get(key, 0.0), v / r)
    msg = go.failure(xs, x64s, r, what, offsets, P)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ the fixed-std model
def run1(m, dev, prompts, head, caps, noise, rows=ROWS, refill=True, thres=-1.0):
    """model_sigmaVAE.Llasa.infer_batch under explicit noise [frames, N, lat] (CPU): the latents per utterance [n_u, lat] on the
    CPU and the shapes of the batch caches the run made.  host: the one draw per step covers all rows, so the feed is laid out
    by the schedule the caps predict."""
    lat = noise.shape[2]
    ps = t1.on_device(prompts, dev)
    with rows_per_step(m, rows), nan_cache(m.base_model.model) as made:
        if head == "host":
            assert refill
            R = min(rows, len(prompts))
            total, first, _ = schedule(caps, R, 0)
            feed = torch.from_numpy(rc.step_noise(noise.numpy(), caps, first, R, total))
            fixed_noise(m, feed.view(total, R, 1, lat).to(dev))
            try:
                outs = m.infer_batch(ps, end_disp_kl_thres=thres, max_length=caps, refill=True)
            finally:
                del m.sample
        else:
            outs = m.infer_batch(ps, end_disp_kl_thres=thres, max_length=caps, device_head=True, noise=noise.to(dev),
                                 stop_lag=int(head[-1]), refill=refill)
    assert len(outs) == len(prompts)
    for o in outs:
        assert o.shape[:2] == (1, lat) and o.dtype == torch.float32
    return [o[0].t().contiguous().cpu() for o in outs], [tuple(c["kv"][0].shape) for c in made]     # (no cache outlives the run)


def check1(c, fmt, prompts, lats, noise, caps, what, key):
    """the means recovered from the returned latents (utterance u's frame f drew noise[f, u]) against the oracle teacher-forced
    on those latents"""
    assert [len(l) for l in lats] == [n - 1 for n in caps], [tuple(l.shape) for l in lats]
    assert not any(torch.isnan(l).any() for l in lats), "NaN: a position nobody wrote was read"
    means = [l.double() - go.STD * noise[:len(l), u].double() for u, l in enumerate(lats)]
    Ps = [go.row_P(dict(ids=ids, prompt=lat)) for ids, lat in prompts]
    rows = go.teacher_rows(prompts, lats, Ps if fmt else None)             # every prompt is prefilled with the bf16 weights
    W = t1.weights(c["id"], fmt)
    f64, emu = go.forward(c, W, rows), go.forward(c, W, rows, "emu")
    cut = lambda outs: [o["mean"][:-1] for o in outs]                       # the last frame is predicted but never returned
    r = go.worst(cut(emu), cut(f64))[0]
    hold(means, cut(f64), r, what, key, offsets=[P - 1 for P in Ps], P=Ps)
    return dict(rows=rows, f64=f64, r=r, means=means, cut=cut, Ps=Ps, lats=lats)


# ------------------------------------------------------------------------------------------------ 0: nothing that existed moved
def test_grouped_mode_returns_the_same_bits_before_and_after_a_refill_run(dev, tmp_path):
    """FIRST in this file: the grouped call is made before any refill run of the process, then again after one"""
    c = go.CASES[0]
    m = t1.build(c, dev, tmp_path)
    prompts = prompts_of(c)
    ps = t1.on_device(prompts, dev)
    noise = draw(c, 6, N, 7)
    kw = dict(end_disp_kl_thres=-1.0, max_length=6, device_head=True, noise=noise.to(dev))
    draws = torch.randn(18, 1, 1, c["lat"], generator=torch.Generator().manual_seed(8)).to(dev)

    def grouped():
        with rows_per_step(m, ROWS):
            a = m.infer_batch(ps, **kw)
            b = m.infer_batch(ps, refill=False, stop_lag=1, **kw)
            fixed_noise(m, draws)
            try:
                h = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=6)
            finally:
                del m.sample
        return a, b, h

    before = grouped()
    assert not hasattr(m, "last_refill_trace")
    with rows_per_step(m, ROWS):
        full = m.infer_batch(ps, refill=True, **kw)
        assert m.infer_batch([], refill=True) == []
        one = m.infer_batch(ps[1:2], refill=True, **dict(kw, noise=noise[:, 1:2].to(dev)))
    assert len(full) == N and m.last_refill_trace == schedule([6] * N, ROWS, 0)[2]
    after = grouped()
    for x, y in zip(before, after):
        assert len(x) == len(y) == N and all(torch.equal(p, q) for p, q in zip(x, y))
    assert all(torch.equal(p, q) for p, q in zip(before[0], before[1]))                    # stop_lag returns the same bits
    alone = m.infer(ps[1][0], ps[1][1], end_disp_kl_thres=-1.0, max_length=6, device_head=True, noise=noise[:, 1:2].to(dev))
    assert len(one) == 1 and torch.equal(one[0], alone)
    same = [torch.equal(p, q) for p, q in zip(full, before[0])]
    print("REFILL 0: refill=True equals refill=False bit for bit, per utterance:", same)


# ------------------------------------------------------------------------------------------------ A: prefill_rows
@pytest.mark.parametrize("ci", [0, 2], ids=lambda i: go.CASES[i]["id"])
def test_prefill_rows_against_fp64(dev, tmp_path, ci):
    from kalle_audio_amd import ops
    c = go.CASES[ci]
    PS, rows, room = (1, 14, 250), [2, 0, 1], 262
    xs = go.scripted_rows(c, PS, 1, tag="prefill_rows")                     # [P + 1, D]: the prompt and one fed-back position
    model = t1.build(c, dev, tmp_path).base_model.model
    D = xs[0].shape[1]
    with nan_cache(model):
        cache = model.init_cache_batch(4, room, dev)
    got = model.prefill_rows([x[:P].to(dev)[None].contiguous() for x, P in zip(xs, PS)], cache, rows)
    assert ops.attn_last_plan() == 8 | c["hd"] << 8, hex(ops.attn_last_plan())            # fwd_varlen
    assert got.shape == (3, 1, D) and cache["len"] == [14, 250, 1, 0]
    pre = model.prefill_rows([x[:P].to(dev)[None].contiguous() for x, P in zip(xs, PS)], model.init_cache_batch(4, room, dev),
                             rows, final_norm=False)
    step = torch.full((4, 1, D), float("nan"))
    for x, P, r in zip(xs, PS, rows):
        step[r, 0] = x[P]
    nxt = model.forward_cached_batch(step.to(dev), cache, [True, True, True, False])
    assert cache["len"] == [15, 251, 2, 0]
    for kv in cache["kv"]:
        k = kv.float().cpu()
        assert torch.isnan(k[3]).all(), "the untouched row was written"
        for r, n in enumerate(cache["len"][:3]):
            assert not torch.isnan(k[r, :n]).any() and torch.isnan(k[r, n:]).all()
    W = t1.weights(c["id"], None)
    ref = [dict(x=x, P=P) for x, P in zip(xs, PS)]
    f64, emu = go.forward(c, W, ref), go.forward(c, W, ref, "emu")
    for q, have in (("hidden", [torch.stack([got[i, 0], nxt[r, 0]]).float().cpu() for i, r in enumerate(rows)]),
                    ("pre", [pre[i].float().cpu() for i in range(3)])):
        n = have[0].shape[0]
        cut = lambda outs: [o[q][o["P"] - 1:o["P"] - 1 + n] for o in outs]
        r = go.worst(cut(emu), cut(f64))[0]
        hold(have, cut(f64), r, f"A prefill_rows {q} {c['id']}", ("A", c["id"], q), offsets=[P - 1 for P in PS], P=list(PS))
    with pytest.raises(ValueError, match="length 0"):
        model.prefill_rows([xs[0][:1].to(dev)[None], xs[1][:14].to(dev)[None]], cache, [3, 0])


# ------------------------------------------------------------------------------------------------ B: refill end to end
GRID = [(h, f) for h in range(3) for f in range(2)]
_GID = [f"{HEADS[h]}-{go.fmt_id(go.FMTS[f])}" for h, f in GRID]


def case1(dev, tmp_path, h, f):
    key = ("B1", h, f)
    if key not in KEEP:
        c, head, fmt = go.CASES[(h + f) % 3], HEADS[h], go.FMTS[f]
        prompts, noise = prompts_of(c), draw(c, max(CAPS), N, 300 + 10 * h + f)
        m = t1.build(c, dev, tmp_path, fmt)
        lats, made = run1(m, dev, prompts, head, CAPS, noise)
        KEEP[key] = dict(c=c, fmt=fmt, head=head, prompts=prompts, noise=noise, lats=lats, trace=m.last_refill_trace, caches=made)
    return KEEP[key]


@pytest.mark.parametrize("h,f", GRID, ids=_GID)
def test_refill_means_per_frame(dev, tmp_path, h, f):
    """model_sigmaVAE.Llasa: every head x format once, the three architectures in rotation"""
    k = case1(dev, tmp_path, h, f)
    c, head = k["c"], k["head"]
    lag = 1 if head == "dev1" else 0
    total, first, trace = schedule(CAPS, ROWS, lag)
    assert k["trace"] == trace and total == (16 if lag else 14)
    assert len(k["caches"]) == 1 and k["caches"][0][:2] == (ROWS, max(rc.PS) + max(CAPS))     # ONE batch cache
    assert first[3][0] == first[0][0] and rc.PS[3] < rc.PS[0] + CAPS[0] - 1          # utterance 3 sits on utterance 0's longer past
    k["ref"] = check1(c, k["fmt"], k["prompts"], k["lats"], k["noise"], CAPS, f"B {head} {go.fmt_id(k['fmt'])} {c['id']}",
                      ("B1", head, k["fmt"]))


def run2(m, dev, prompts, head, caps, noise, rows=ROWS):
    """model.Llasa.infer_batch(refill=True): per utterance (disp [n_u, 2 lat], the latents the path fed back [n_u, lat], what the
    head read [n_u, D]), cut from what the head saw step by step with the trace the run left"""
    from kalle_audio_amd import ops
    lat = noise.shape[2]
    ps = t1.on_device(prompts, dev)
    R = min(rows, len(prompts))
    fed, read = [], []
    with rows_per_step(m, rows), nan_cache(m.base_model.model):
        if head == "host":
            real = m._host_frame

            def spy(hidden):
                out = real(hidden)
                read.append(hidden.reshape(hidden.shape[0], -1).clone())
                fed.append(out[1].reshape(out[1].shape[0], -1).clone())
                return out

            m._host_frame = spy
            total, first, _ = schedule(caps, R, 0)
            feed = torch.from_numpy(rc.step_noise(noise.numpy(), caps, first, R, total)).to(dev)
            try:
                with host_noise(list(feed)):
                    outs = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=caps, refill=True)
            finally:
                del m._host_frame
        else:
            real = ops.llasa_frame_head2

            def spy(plan, h, nz, active=None, frame=0):
                out = real(plan, h, nz, active, frame=frame)
                read.append(h.clone())
                fed.append(out[1].clone())
                return out

            ops.llasa_frame_head2 = spy
            try:
                outs = m.infer_batch(ps, end_disp_kl_thres=-1.0, max_length=caps, device_head=True, noise=noise.to(dev),
                                     stop_lag=int(head[-1]), refill=True)
            finally:
                ops.llasa_frame_head2 = real
    assert len(outs) == len(prompts)
    disp = [o[0].t().contiguous().cpu() for o in outs]
    assert all(d.shape == (n - 1, 2 * lat) for d, n in zip(disp, caps)), [tuple(d.shape) for d in disp]
    per = lambda calls: [torch.stack([calls[t + j][r] for j in range(n - 1)]).float().cpu() for _, r, t, n in m.last_refill_trace]
    return disp, per(fed), per(read)


@pytest.mark.parametrize("h,f", GRID, ids=_GID)
def test_refill_disp_per_frame(dev, tmp_path, h, f):
    """model.Llasa: every head x format once; disp and what the head read, of every returned frame"""
    c, head, fmt = g2.CASES[(h + f + 1) % 3], HEADS[h], g2.FMTS[f]
    prompts, noise = prompts_of(c), draw(c, max(CAPS), N, 400 + 10 * h + f)
    m = t2.build(c, dev, tmp_path, fmt)
    disp, fed, read = run2(m, dev, prompts, head, CAPS, noise)
    assert m.last_refill_trace == schedule(CAPS, ROWS, 1 if head == "dev1" else 0)[2]
    assert not any(torch.isnan(d).any() for d in disp), "NaN: a position nobody wrote was read"
    for u, (d, l) in enumerate(zip(disp, fed)):         # the fed-back latent is mean + exp(logs) * noise[f, u]: the utterance's own column
        want = g2.sample(d.double(), noise[:len(d), u])
        assert torch.allclose(l.double(), want, rtol=1e-4, atol=1e-5), (u, (l.double() - want).abs().max().item())
    t2.teacher_check(c, fmt, prompts, head, disp, fed, read, f"REFILL B2 {head} {g2.fmt_id(fmt)} {c['id']}", ("B2", head, fmt))


# ------------------------------------------------------------------------------------------------ C: seeded defects
def embed(W, row):
    """the fp64 input embeddings of a teacher row [L, D]"""
    m = ko._sub(W, "base_model.model.")
    lat = row["fed"].to(go.F64) if row.get("prompt") is None else torch.cat([row["prompt"].to(go.F64), row["fed"].to(go.F64)], 0)
    return torch.cat([m["embed_tokens.weight"][row["ids"]], ko.linear(lat, W["audio_linear.weight"], W["audio_linear.bias"])], 0)


def previous_occupant(trace):
    """utterance -> the utterance that held its row before it"""
    prev, last = {}, {}
    for u, r, t, n in sorted(trace, key=lambda x: x[2]):
        if r in last:
            prev[u] = last[r]
        last[r] = u
    return prev


@pytest.mark.parametrize("h", [0, 1], ids=["host", "dev0"])
def test_refill_wrong_references_are_caught(dev, tmp_path, h):
    k = case1(dev, tmp_path, h, 0)
    c = k["c"]
    ref = k.get("ref") or check1(c, None, k["prompts"], k["lats"], k["noise"], CAPS, "C rerun", ("B1", k["head"], None))
    good, r, means, rows = ref["cut"](ref["f64"]), ref["r"], ref["means"], ref["rows"]
    off = [P - 1 for P in ref["Ps"]]
    assert go.failure(means, good, r) is None
    W = t1.weights(c["id"], None)
    prev = previous_occupant(k["trace"])
    assert sorted(prev) == [2, 3, 4] and prev[3] == 0
    stale, rotary = [g.clone() for g in good], [g.clone() for g in good]
    for u, v in prev.items():
        xv, xu = embed(W, rows[v]), embed(W, rows[u])
        Lv, Lu, P = xv.shape[0], xu.shape[0], ref["Ps"][u]
        # the previous occupant's keys left visible: its positions stay in front of the utterance's own, which restart at 0
        both = dict(x=torch.cat([xv, xu], 0), P=Lv + P)
        pos = torch.cat([torch.arange(Lv), torch.arange(Lu)])
        stale[u] = go.row_forward(c, W, both, "f64", pos, torch.ones(Lv + Lu, Lv + Lu, dtype=torch.bool).tril())["mean"][:-1]
        # rotary positions of the decode steps going on from the previous occupant's length instead of the prompt's
        pos = torch.arange(Lu) + (torch.arange(Lu) >= P).long() * (Lv - P)
        rotary[u] = go.row_forward(c, W, rows[u], "f64", pos)["mean"][:-1]
    neighbour = [l.double() - go.STD * k["noise"][:len(l), (u + 1) % N].double() for u, l in enumerate(k["lats"])]
    swapped = list(means)
    swapped[1], swapped[3] = means[3], means[1]
    for label, xs, x64 in (("previous occupant's keys visible", means, stale), ("rotary from the previous length", means, rotary),
                           ("the neighbour's noise", neighbour, good), ("utterances 1 and 3 swapped", swapped, good)):
        msg = go.failure(xs, x64, r, label, offsets=off, P=ref["Ps"])
        print("REFILL C:", msg)
        assert msg is not None, label


# ------------------------------------------------------------------------------------------------ D: the stop rule
def test_refill_rows_leave_through_the_kl_rule(dev, tmp_path):
    """host head, the tiny hd-64 module config: a forward hook on distribution_linear adds 100 to the predicted mean (KL ~ 660)
    wherever an utterance must go on and nothing where it must stop (threshold 300), as
    test_infer_batch_stops_one_row_and_leaves_the_others_alone does.  Utterances stop after 6 / 5 / - / 5 / 7 frames (the third
    runs into the cap of 9); which (step, row) that is comes from the schedule those counts predict, and the trace must equal it."""
    m, d, _ = tiny_build(64, dev, tmp_path)
    g = torch.Generator(device=dev).manual_seed(12)
    ps = [(torch.randint(0, 300, (n,), device=dev, generator=g), torch.randn(1, 2, d, device=dev, generator=g) if n % 2 else None)
          for n in (9, 4, 17, 3, 6)]
    want = [6, 5, 9, 5, 7]
    total, first, trace = schedule(want, ROWS, 0)
    occ = rc.occupants(want, first, ROWS)
    step = [0]

    def bump(mod, inp, out):
        b = torch.full_like(out, 100.0)
        for r in range(ROWS):
            u, f = occ.get((step[0], r), (None, None))
            if u is not None and f == want[u] - 1 and want[u] < 9:
                b[r] = 0.0
        step[0] += 1
        return out + b

    hook = m.distribution_linear.register_forward_hook(bump)
    try:
        with rows_per_step(m, ROWS), nan_cache(m.base_model.model):
            outs = m.infer_batch(ps, end_disp_kl_thres=300.0, max_length=9, refill=True)
    finally:
        hook.remove()
    assert [o.shape[2] for o in outs] == [n - 1 for n in want], [o.shape for o in outs]
    assert m.last_refill_trace == trace and step[0] == total
    assert not any(torch.isnan(o).any() for o in outs)


def test_refill_stop_lag_one_against_zero(dev, tmp_path):
    """device head, one model, the same prompts and noise: the same frame counts under stop_lag 1 and 0 although the rows are
    refilled one step later, every frame of both within the oracle bound; whether the bits agree is printed"""
    a = case1(dev, tmp_path, 1, 0)
    c = a["c"]
    m = t1.build(c, dev, tmp_path)
    lats, _ = run1(m, dev, a["prompts"], "dev1", CAPS, a["noise"])
    assert [len(x) for x in a["lats"]] == [len(x) for x in lats] == [n - 1 for n in CAPS]
    assert [t[3] for t in a["trace"]] == [t[3] for t in m.last_refill_trace] == CAPS
    assert [t[2] for t in a["trace"]] == [0, 0, 3, 6, 9] and [t[2] for t in m.last_refill_trace] == [0, 0, 4, 7, 11]
    if "ref" not in a:
        check1(c, None, a["prompts"], a["lats"], a["noise"], CAPS, f"D stop_lag 0 {c['id']}", ("D", 0))
    check1(c, None, a["prompts"], lats, a["noise"], CAPS, f"D stop_lag 1 {c['id']}", ("D", 1))
    print("REFILL D: stop_lag 1 equals stop_lag 0 bit for bit, per utterance:", [torch.equal(x, y) for x, y in zip(lats, a["lats"])])


# ------------------------------------------------------------------------------------------------ E: no refill, and 17 on 16
def test_refill_with_no_more_prompts_than_rows(dev, tmp_path):
    c = go.CASES[1]
    m = t1.build(c, dev, tmp_path)
    prompts = go.ragged_prompts(c)                                          # P = 1 / 14 / 250
    caps, noise = [6, 4, 5], draw(c, 6, 3, 21)
    lats, made = run1(m, dev, prompts, "dev0", caps, noise, rows=16)
    assert m.last_refill_trace == [(0, 0, 0, 6), (1, 1, 0, 4), (2, 2, 0, 5)] and made[0][0] == 3
    check1(c, None, prompts, lats, noise, caps, f"E three prompts, sixteen rows {c['id']}", ("E", 3))
    grouped, _ = run1(m, dev, prompts, "dev0", caps, noise, rows=16, refill=False)
    assert [len(x) for x in grouped] == [5, 3, 4]
    check1(c, None, prompts, grouped, noise, caps, f"E the same list grouped, per-prompt caps {c['id']}", ("E", "grouped"))
    print("REFILL E: refill=True equals refill=False bit for bit, per utterance:", [torch.equal(x, y) for x, y in zip(lats, grouped)])


def test_refill_seventeen_prompts_on_sixteen_rows(dev, tmp_path):
    c = go.CASES[0]
    m = t1.build(c, dev, tmp_path)
    prompts = go.many_prompts(c, 17)
    caps = [4 + u % 3 for u in range(17)]
    noise = draw(c, 6, 17, 22)
    lats, made = run1(m, dev, prompts, "dev1", caps, noise, rows=16)
    assert m.last_refill_trace == schedule(caps, 16, 1)[2] and m.last_refill_trace[16][1:3] == (0, 5)
    assert made[0][0] == 16
    check1(c, None, prompts, lats, noise, caps, f"E seventeen prompts {c['id']}", ("E", 17))


def test_measured():
    for k in sorted(MEASURED, key=str):
        print(f"REFILL MEASURED {k}: {MEASURED[k]:.2f} r")
