"""KV-cached generation of both Llasa task models (model_sigmaVAE.Llasa, model.Llasa): ONE frame loop (`run_frames`) for `infer`
and `infer_batch`, the host head and the device head, stop_lag 0 / 1, groups and refill.  The loop is host bookkeeping only - which
utterance sits in which row at which step (RowSchedule), the stop rule, the stop_lag skew - and calls no device API; what touches
the device lives in two collaborators:
  decoder rows  OneRow (init_cache / forward_cached, the one-row decode kernel) or BatchRows (init_cache_batch /
                forward_cached_batch, prompts prefilled row by row or packed),
  a head        HostHead (owner._host_frame and owner.audio_linear) or DeviceHead (ops.llasa_frame_head / llasa_frame_head2 on a
                plan, the KL through pinned memory and an event).
A group of `infer_batch(refill=False)` is the refill loop with three differences, each a piece of data here: the prompts are
prefilled row by row (BatchRows.packed=False: the packed GEMMs may pick another plan, so the bits would differ), no step >= the
cap is ever enqueued (`horizon`), and every group makes its own cache, head and schedule (one `generate` call per group)."""
from typing import Callable, NamedTuple

import torch

from . import ops
from .dit_ops import F32


def device_head_limits(stop_lag, lat, max_lat):
    """the refusals both task models share before a device-head generation starts"""
    if stop_lag not in (0, 1):
        raise NotImplementedError(f"stop_lag is 0 or 1, got {stop_lag!r}; the host path (device_head=False) takes neither")
    if lat % 8 or not 8 <= lat <= max_lat:
        raise NotImplementedError(f"device_head=True takes a latent_dim that is a multiple of 8 in 8 .. {max_lat}, "
                                  f"got {lat}; the host path (device_head=False) has no such limit")


def _prompt_embeds(owner, prompts):
    model = owner.base_model.model
    embeds = []
    for ids, lat in prompts:
        parts = [model.embed_tokens(ids.unsqueeze(0))]
        if lat is not None:
            parts.append(owner.audio_linear(lat))
        embeds.append(torch.cat(parts, dim=1))
    return embeds


class RowSchedule:
    """Which utterance runs in which row of the batch cache at which global step, when a row freed by a stopped utterance takes
    the next waiting prompt (`infer_batch(refill=True)`; a group without refill is n_prompts = R: everything is admitted at step 0).
    Host bookkeeping only: prompts are admitted in list order, free rows are taken in ascending row index.  A step s is `admit(s)`
    (the frame boundary), then one frame for every row of `live(s)`; `release(row, frames)` frees a row once its utterance's stop
    is known - before `admit(s + 1)` when every step is resolved before the next is enqueued, one `admit` later when the loop runs
    one step ahead (stop_lag=1)."""

    def __init__(self, n_prompts, R):
        if n_prompts < 0 or R < 1:
            raise ValueError(f"RowSchedule takes n_prompts >= 0 and R >= 1, got {n_prompts}, {R}")
        self.n, self.R = int(n_prompts), int(R)
        self.rows, self.first = [None] * self.R, [0] * self.R       # the utterance in each row and the step of its frame 0
        self.waiting = 0                                            # the next prompt of the list
        self._trace = []

    def admit(self, step):
        """the (utterance, row) pairs to prefill at the frame boundary of `step`: frame 0 of each runs at that step"""
        pairs = []
        if self.waiting >= self.n:
            return pairs
        for r in range(self.R):
            if self.rows[r] is None and self.waiting < self.n:
                self.rows[r], self.first[r] = self.waiting, step
                pairs.append((self.waiting, r))
                self.waiting += 1
        return pairs

    def live(self, step):
        """(row, utterance, frame) of every occupied row at `step`"""
        return [(r, u, step - self.first[r]) for r, u in enumerate(self.rows) if u is not None]

    def release(self, row, frames):
        """the utterance in `row` stopped after `frames` frames (its last one included)"""
        self._trace.append((self.rows[row], row, self.first[row], int(frames)))
        self.rows[row] = None

    @property
    def done(self):
        return self.waiting >= self.n and all(u is None for u in self.rows)

    @property
    def trace(self):
        """(utterance, row, first_step, frames) of every released utterance, in list order"""
        return sorted(self._trace)

    @property
    def steps(self):
        """global steps up to the last frame of the last utterance (the discarded look-ahead frame of stop_lag=1 not counted)"""
        return max((first + frames for _, _, first, frames in self._trace), default=0)


def refill_steps(frames, R, stop_lag=0):
    """What RowSchedule does for utterances that run frames[u] frames each, in closed form: (total steps, [(row, first_step)] per
    utterance).  Utterance u starts at the first step >= its predecessor's start at which a row is free, in the lowest such row;
    its row is free again frames[u] + stop_lag steps later.  `grouped_steps` is the count without refill."""
    free_at = [0] * R
    out, t, total = [], 0, 0
    for n in frames:
        t = max(t, min(free_at))
        r = min(i for i in range(R) if free_at[i] <= t)
        out.append((r, t))
        free_at[r] = t + int(n) + stop_lag
        total = max(total, t + int(n))
    return total, out


def grouped_steps(frames, R):
    """decoder steps of `infer_batch` without refill: groups of R, each as long as its longest utterance"""
    frames = list(frames)
    return sum(max(frames[i:i + R]) for i in range(0, len(frames), R))


def _frame_caps(max_length, n):
    """max_length as one cap per prompt (a sequence of n ints), or None for the plain int"""
    if not hasattr(max_length, "__iter__"):
        return None
    caps = [int(m) for m in max_length]
    if len(caps) != n or min(caps) < 1:
        raise ValueError(f"max_length is an int or one int >= 1 per prompt; got {len(caps)} values for {n} prompts")
    return caps


# ---- the loop
def run_frames(sched, rows, head, thres, caps, ring, stop_lag=0, horizon=None):
    """Every frame of the utterances `sched` (a RowSchedule) admits, on the decoder rows `rows` with the head `head`; returns what
    head.cut gives for each utterance, in prompt order.  A global step s is
      enqueue(s)  admit the waiting prompts into the free rows; the decode step for the rows that continue (the rows being
                  admitted are inactive in it); the prefill of the admitted prompts into the step's hidden buffer; the head for
                  every occupied row, into slot s % ring,
      resolve(s)  the one host wait (head.kl); an utterance stops at its frame f when kl < thres and f > 3, or at its cap
                  (f + 1 >= caps[u]); a stopped utterance's frames 0 .. f - 1 are cut from the slots of steps s - f .. s - 1 (its
                  last frame is predicted but never returned) and its row is released.
    stop_lag=1: step s + 1 is enqueued before step s is resolved, so a stopped utterance has run one discarded look-ahead frame
    (one extra cache position, one extra draw) and its row is refilled one step later.  ring: an utterance spans at most
    max(caps) + stop_lag consecutive steps, the look-ahead frame included, so that many slots keep every frame until it is cut.
    horizon: no step >= horizon is enqueued (a group without refill: the look-ahead frame of the rows at the highest cap does not
    run; every row has stopped by step horizon - 1, so no such step is resolved either)."""
    results, live = [None] * sched.n, {}

    def enqueue(s):
        admitted = sched.admit(s)
        now = live[s] = sched.live(s)
        if not now:
            return
        cont = [False] * sched.R
        for r, _, f in now:
            cont[r] = f > 0             # (frame 0 is the prefill's)
        h = rows.decode(head.next_input(), cont) if any(cont) else None
        if admitted:
            h = rows.prefill(admitted, h)
        head.run(s % ring, h, now)

    def resolve(s):
        now = live.pop(s)
        if not now:
            return
        kl = head.kl(s % ring)
        for r, u, f in now:
            if sched.rows[r] != u:          # (stop_lag=1: the look-ahead frame of an utterance that has stopped)
                continue
            if (kl[r] < thres and f > 3) or f + 1 >= caps[u]:
                results[u] = head.cut(r, [(s - f + j) % ring for j in range(f)])
                sched.release(r, f + 1)

    s = 0
    if stop_lag:
        enqueue(0)
    while True:
        if horizon is None or s + stop_lag < horizon:
            enqueue(s + stop_lag)
        resolve(s)
        if sched.done:
            return results
        s += 1


# ---- decoder rows: decode(x [R, 1, D], cont) -> the step's hidden rows [R, 1, D]; prefill(admitted, h) -> h with the last hidden
# state of every admitted prompt in its row (h None: no row continued)
def _norm_kw(final_norm):
    """the keyword the cache methods are called with: none where the head reads normed rows (the methods' default, and the call
    the host loops always made - an instance-level replacement of a cache method need not know the keyword), final_norm=False
    for the device head, which norms the residual stream itself"""
    return {} if final_norm else {"final_norm": False}


class OneRow:
    """one utterance on the one-row cache: the prompt through forward_cached, then the one-row decode kernel per frame"""

    def __init__(self, model, embeds, room, final_norm):
        self.model, self.embeds, self.norm_kw = model, embeds, _norm_kw(final_norm)
        self.cache = model.init_cache(room, embeds[0].device)

    def decode(self, x, cont):
        return self.model.forward_cached(x, self.cache, **self.norm_kw)

    def prefill(self, admitted, h):
        return self.model.forward_cached(self.embeds[0], self.cache, **self.norm_kw)[:, -1:, :]


class BatchRows:
    """R rows of one batch cache.  packed=False: the admitted prompts go through prefill_row one by one, in row order;
    packed=True: through prefill_rows in ONE pass, after their rows' cache lengths were reset to 0 (the previous occupant's
    positions stay in the buffer and are never read: every key count comes from cache["len"]).  Either way their last hidden
    states are copied into the step's hidden buffer row by row - the decode step's own output buffer, or `idle` at a step without
    a decode step."""

    def __init__(self, model, embeds, R, room, final_norm, packed):
        self.model, self.embeds, self.norm_kw, self.packed = model, embeds, _norm_kw(final_norm), packed
        dev, self.D = embeds[0].device, embeds[0].shape[2]
        self.cache = model.init_cache_batch(R, room, dev)
        self.idle = torch.zeros((R, 1, self.D), device=dev, dtype=F32)

    def decode(self, x, cont):
        return self.model.forward_cached_batch(x, self.cache, cont, **self.norm_kw)

    def prefill(self, admitted, h):
        h = self.idle if h is None else h
        if self.packed:
            for _, r in admitted:
                self.cache["len"][r] = 0
            first = self.model.prefill_rows([self.embeds[u] for u, _ in admitted], self.cache, [r for _, r in admitted],
                                            **self.norm_kw)
        else:
            first = [self.model.prefill_row(self.embeds[u], self.cache, r, **self.norm_kw)[:, -1, :]
                     for u, r in admitted]
        for j, (_, r) in enumerate(admitted):
            ops.copy_rows(first[j], h[r], 1, 1, self.D, 0, self.D, 0, self.D)
        return h


# ---- heads: run(k, h, now) the head of one step into slot k, for the (row, utterance, frame) triples of the occupied rows;
# next_input() the next decode step's input [R, 1, D]; kl(k) slot k's KL per row as a host list (the one host wait of a step);
# cut(r, slots) what `infer` returns for the frames row r left in `slots`
class HostHead:
    """owner._host_frame(hidden [R, 1, D]) -> (kept [R, 1, w], audio_latent [R, 1, lat], kl [R, 1]) per step: `kept` is what
    `infer` stacks per frame (the sampled latent / mean || log-scale), `audio_latent` feeds owner.audio_linear - launched when the
    next step asks for its input, so never after the last frame - and `kl` is the stop quantity."""

    def __init__(self, owner, R, ring):
        self.owner, self.R = owner, R
        self.kept, self.kls, self.latent = [None] * ring, [None] * ring, None

    def run(self, k, h, now):
        self.kept[k], self.latent, self.kls[k] = self.owner._host_frame(h)

    def next_input(self):
        return self.owner.audio_linear(self.latent)

    def kl(self, k):
        return self.kls[k].view(self.R).tolist()

    def cut(self, r, slots):
        return torch.stack([self.kept[k][r:r + 1] for k in slots], dim=1).squeeze(1).squeeze(2).transpose(1, 2)


class DeviceHeadSpec(NamedTuple):
    """what differs between the two task models' device heads"""
    plan: Callable      # ops.llasa_head_plan / ops.llasa_head2_plan
    call: Callable      # ops.llasa_frame_head / ops.llasa_frame_head2: call(plan, h, noise, *args, active, frame=slot)
    args: tuple         # (std,) / ()
    kept: str           # the plan's [ring, R, w] buffer a result is cut from: "latent" / "disp"
    lat: int


class DeviceHead:
    """spec.call on a plan of `ring` slots per step: final norm, distribution_linear, the sample, the stop KL and audio_linear in
    one host call; the KL goes to slot k of a device buffer, from there to pinned host memory without blocking, followed by an
    event.  noise [top, N, lat]: utterance u's frame f reads noise[f, u] at whatever row and step it runs (the discarded
    look-ahead frame of an utterance at its cap reads its last draw again; an unoccupied row's outputs are not touched, so what
    it reads is free); None: one torch.randn((R, 1, lat)) per step.  all_rows: the head runs without an active list (OneRow)."""

    def __init__(self, owner, spec, R, ring, dev, noise, all_rows):
        dlin, alin, model = owner.distribution_linear, owner.audio_linear, owner.base_model.model
        self.spec, self.R, self.dev, self.noise, self.all_rows = spec, R, dev, noise, all_rows
        self.plan = spec.plan(model.norm.weight, dlin[0].weight, dlin[0].bias, dlin[2].weight, dlin[2].bias, alin.weight,
                              alin.bias, R, model.norm.variance_epsilon, dev, frames=ring)
        self.kl_host = torch.empty((ring, R), dtype=F32, pin_memory=True)
        self.events = [None] * ring

    def run(self, k, h, now):
        R, lat, plan = self.R, self.spec.lat, self.plan
        fi, ui, occupied = [0] * R, [0] * R, [False] * R
        for r, u, f in now:
            fi[r], ui[r], occupied[r] = f, u, True
        if self.noise is None:
            nz = torch.randn((R, 1, lat), device=self.dev, dtype=F32).view(R, lat)
        else:
            nz = self.noise[[min(f, self.noise.shape[0] - 1) for f in fi], ui]
        self.spec.call(plan, h.view(R, -1), nz, *self.spec.args, None if self.all_rows else occupied, frame=k)
        self.kl_host[k].copy_(plan["kl"][k], non_blocking=True)
        self.events[k] = torch.cuda.Event()
        self.events[k].record()

    def next_input(self):
        return self.plan["x_next"].view(self.R, 1, -1)

    def kl(self, k):
        self.events[k].synchronize()
        return self.kl_host[k].tolist()

    def cut(self, r, slots):
        slots = torch.tensor(slots, device=self.dev, dtype=torch.long)
        return self.plan[self.spec.kept][:, r, :].index_select(0, slots).unsqueeze(0).transpose(1, 2)


# ---- the callers
def batch_rows(owner, rows):
    """the rows per decoder pass of a batched call.  rows None: min(owner.infer_batch_rows, DECODE_MAX_ROWS), as before the wide
    step existed (a larger infer_batch_rows stays clamped); an int in 1 .. DECODE_WIDE_MAX_ROWS: that many, above DECODE_MAX_ROWS
    through the wide step - which has no e4m3 form."""
    if rows is not None and (isinstance(rows, bool) or not isinstance(rows, int) or not 1 <= rows <= ops.DECODE_WIDE_MAX_ROWS):
        raise ValueError(f"rows: None or an int in 1 .. {ops.DECODE_WIDE_MAX_ROWS}, got {rows!r}")
    if owner is None:                # (the argument check alone)
        return rows
    if rows is None:
        return max(1, min(int(owner.infer_batch_rows), ops.DECODE_MAX_ROWS))
    fmt = getattr(owner.base_model.model, "_decode_fmt", None)
    if rows > ops.DECODE_MAX_ROWS and fmt is not None:
        raise NotImplementedError(f"quantize_decoder({fmt!r}) together with rows={rows}: more than {ops.DECODE_MAX_ROWS} rows "
                                  "per decoder pass run the wide step, which reads bf16 weights only")
    return rows


def generate(owner, prompts, thres, max_length, spec=None, noise=None, stop_lag=0, refill=False, rows=None):
    """One run of the loop.  refill=False: `infer` (one prompt: OneRow) or one group of `infer_batch` (a row per prompt, nothing
    admitted after step 0).  refill=True: the whole list on ONE batch cache of R = min(batch_rows(owner, rows), len(prompts))
    rows (rows=None: infer_batch_rows clamped to DECODE_MAX_ROWS); the schedule's trace is left in owner.last_refill_trace.
    max_length: an int, or one frame cap per prompt.
    spec: the DeviceHeadSpec of the owner's device head (None: the host head, which takes neither noise nor stop_lag).  Returns the
    results in prompt order."""
    model = owner.base_model.model
    embeds = _prompt_embeds(owner, prompts)
    N, dev = len(embeds), embeds[0].device
    caps = _frame_caps(max_length, N) or [max_length] * N
    top = max(caps)
    R = min(batch_rows(owner, rows), N) if refill else N
    if noise is not None:
        noise = noise.to(device=dev, dtype=F32).expand(top, N, spec.lat)
    host, one, ring = spec is None, N == 1 and not refill, top + stop_lag
    room = max(e.shape[1] for e in embeds) + top
    seats = OneRow(model, embeds, room, host) if one else BatchRows(model, embeds, R, room, host, packed=refill)
    head = HostHead(owner, R, ring) if host else DeviceHead(owner, spec, R, ring, dev, noise, all_rows=one)
    sched = RowSchedule(N, R)
    results = run_frames(sched, seats, head, thres, caps, ring, stop_lag, horizon=None if refill else top)
    if refill:
        owner.last_refill_trace = sched.trace
    return results


def generate_uncached(owner, prompt, thres, max_length):
    """`infer(use_cache=False)`: the reference's schedule, the decoder over the whole prefix for every frame (O(T^2) GEMM work)"""
    input_embed = _prompt_embeds(owner, [prompt])[0]
    final = []
    for i in range(max_length):
        hidden = owner.base_model.model(inputs_embeds=input_embed)[0]
        kept, audio_latent, kl = owner._host_frame(hidden[:, -1:, :])
        final.append(kept)
        if kl.item() < thres and i > 3:
            break
        input_embed = torch.cat((input_embed, owner.audio_linear(audio_latent)), dim=1)
    return torch.stack(final[:-1], dim=1).squeeze(1).squeeze(2).transpose(1, 2)


def generate_one(owner, input_ids, audio_latents, thres, max_length, use_cache, device_head, noise, stop_lag):
    """`infer` of both task models"""
    if device_head:
        if not use_cache:
            raise NotImplementedError("device_head=True generates against a KV cache; use_cache=False runs on the host path "
                                      "(device_head=False)")
        return owner._generate_device_head([(input_ids, audio_latents)], thres, max_length, noise, stop_lag)[0]
    if noise is not None or stop_lag:
        raise ValueError("noise= and stop_lag= belong to device_head=True")
    if not use_cache:
        return generate_uncached(owner, (input_ids, audio_latents), thres, max_length)
    return generate(owner, [(input_ids, audio_latents)], thres, max_length)[0]


def generate_batch(owner, prompts, thres, max_length, device_head, noise, stop_lag, lat, refill=False, rows=None):
    """`infer_batch` of both task models: the checks, one prompt = `owner.infer`, lists longer than `owner.infer_batch_rows` in
    groups, a group through owner._generate_device_head or through `generate` with the host head; refill=True: the whole list in
    one run.  max_length: an int, or one frame cap per prompt.  rows: batch_rows' argument - the group size / the shared cache's
    row count of this call."""
    prompts = list(prompts)
    batch_rows(None, rows)
    if not prompts:
        return []
    G = batch_rows(owner, rows)
    if not device_head and (noise is not None or stop_lag):
        raise ValueError("noise= and stop_lag= belong to device_head=True")
    caps = _frame_caps(max_length, len(prompts))
    top = max_length if caps is None else max(caps)
    if device_head and noise is not None:
        noise = noise.to(F32).expand(top, len(prompts), lat)
    if len(prompts) == 1:
        return [owner.infer(prompts[0][0], prompts[0][1], end_disp_kl_thres=thres, max_length=top,
                            device_head=device_head, noise=noise, stop_lag=stop_lag)]
    if not refill and len(prompts) > G:
        part = lambda i: max_length if caps is None else caps[i:i + G]
        cut = lambda i: noise[:, i:i + G] if caps is None else noise[:max(part(i)), i:i + G]
        return [o for i in range(0, len(prompts), G)
                for o in generate_batch(owner, prompts[i:i + G], thres, part(i), device_head,
                                        None if noise is None else cut(i), stop_lag, lat, rows=rows)]
    if device_head:
        return owner._generate_device_head(prompts, thres, max_length, noise, stop_lag, refill=refill, rows=rows)
    return generate(owner, prompts, thres, max_length, refill=refill, rows=rows)
