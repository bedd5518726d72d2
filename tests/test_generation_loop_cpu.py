"""CPU: the generation loop of kalle_audio_amd/generation.py - `run_frames`, its decoder rows (OneRow, BatchRows) and its heads
(HostHead, DeviceHead) - driven as `infer` / `infer_batch` drive it, on fakes of what lies below them: a decoder model that logs
init_cache / forward_cached / init_cache_batch / prefill_row / prefill_rows / forward_cached_batch and keeps cache["len"] as the
real one does, a device-head description whose call logs its arguments, an owner whose _host_frame / audio_linear log theirs.
Nothing here launches a kernel: ops.copy_rows, the pinned KL buffer and the event are replaced (`no_device`).

The fakes carry WHO a hidden row belongs to through the real loop: a hidden row is (utterance, frame) - the prompt's token ids are
its utterance index, a prefill gives (u, 0), the head's next input is (u, f + 1), a decode step hands its input on - and explicit
noise is noise[f, u] = 1000 f + u, so the head sees which row holds which utterance's which frame and which draw it was given, and
scripts its KL from that: utterance u's frame stops[u] - 1 is below the threshold.  The returned tensors are then the frames
(u, 0) .. (u, n - 2) of every utterance, whatever row, step and slot they went through."""
import contextlib
import os
import random
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refill_cases as rc  # noqa: E402

from kalle_audio_amd import generation as gen  # noqa: E402

STEP = torch.tensor([0.0, 1.0])


def seeded_caps(seed, n=64, lo=50, hi=250):
    g = random.Random(seed)
    return [g.randint(lo, hi) for _ in range(n)]


LISTS = [(rc.CAPS, rc.ROWS), ([4, 4, 4], 16), ([5], 3), ([2, 9, 2, 2, 7, 1, 3], 3), (seeded_caps(0, 23, 2, 30), 4),
         (seeded_caps(1), 16)]


# ------------------------------------------------------------------------------------------------ the fakes
class FakeModel:
    """LlamaModel's cache methods: hidden rows are [.., 2] = (utterance, frame); every call goes to `log`"""

    def __init__(self, log):
        self.log, self.caches = log, []
        self.norm = SimpleNamespace(weight=None, variance_epsilon=1e-5)

    def embed_tokens(self, ids):
        return torch.stack([ids.float(), -torch.ones(ids.shape)], dim=2)

    @staticmethod
    def _prefilled(emb):
        h = emb.clone()
        h[:, -1, 1] = 0.0
        return h

    def init_cache(self, room, dev):
        self.caches.append({"len": 0, "room": room})
        return self.caches[-1]

    def forward_cached(self, x, cache, final_norm=True):
        prompt = cache["len"] == 0
        cache["len"] += x.shape[1]
        assert cache["len"] <= cache["room"]
        self.log.append(("prefill", 0, final_norm) if prompt else ("decode", None, final_norm))
        return self._prefilled(x) if prompt else x.clone()

    def init_cache_batch(self, R, room, dev):
        self.caches.append({"len": [0] * R, "room": room, "out": torch.zeros(R, 1, 2)})
        return self.caches[-1]

    def prefill_row(self, emb, cache, r, final_norm=True):
        cache["len"][r] += emb.shape[1]
        self.log.append(("prefill", r, final_norm))
        return self._prefilled(emb)

    def prefill_rows(self, embeds, cache, rows, final_norm=True):
        assert all(cache["len"][r] == 0 for r in rows), "a packed prefill into a row whose length was not reset"
        for e, r in zip(embeds, rows):
            cache["len"][r] = e.shape[1]
        self.log.append(("prefill_rows", [(int(e[0, 0, 0]), r) for e, r in zip(embeds, rows)], final_norm))
        return torch.cat([self._prefilled(e)[:, -1:, :] for e in embeds], dim=0)

    def forward_cached_batch(self, x, cache, active=None, final_norm=True):
        for r, a in enumerate(active):
            if a:
                cache["out"][r] = x[r]
                cache["len"][r] += 1
        assert max(cache["len"]) <= cache["room"]
        self.log.append(("decode", tuple(active), final_norm))
        return cache["out"]


class FakeLinear:
    weight = bias = None

    def __init__(self, log):
        self.log = log

    def __call__(self, latent):
        self.log.append(("audio_linear",))
        return latent + STEP


class FakeOwner:
    """what generation.py touches of a Llasa: utterance u stops through the KL rule at its frame stops[u] - 1 (None: never)"""

    def __init__(self, stops, rows=16, top=None):
        self.log, self.stops, self.top = [], stops, top
        self.base_model = SimpleNamespace(model=FakeModel(self.log))
        self.audio_linear = FakeLinear(self.log)
        self.distribution_linear = [SimpleNamespace(weight=None, bias=None)] * 3
        self.infer_batch_rows = rows

    def kl(self, u, f):
        return -1.0 if self.stops[u] == f + 1 else 1.0

    def _host_frame(self, hidden):
        R = hidden.shape[0]
        self.log.append(("head",))
        who = [(int(hidden[r, 0, 0]), int(hidden[r, 0, 1])) for r in range(R)]
        return hidden.clone(), hidden.clone(), torch.tensor([[self.kl(u, f) if u >= 0 else 9.0] for u, f in who])

    # the device head's description: a plan of CPU buffers, a call that does what the kernel's contract says
    def plan(self, norm, w1, b1, w2, b2, wa, ba, R, eps, dev, frames=1):
        self.log.append(("plan", R, frames))
        return {"kl": torch.zeros(frames, R), "kept": torch.zeros(frames, R, 2), "x_next": torch.zeros(R, 2)}

    def call(self, plan, h, nz, active=None, frame=0):
        R = h.shape[0]
        assert tuple(h.shape) == (R, 2) and tuple(nz.shape) == (R, 1)
        seen = []
        for r in range(R):
            if active is None or active[r]:
                u, f = int(h[r, 0]), int(h[r, 1])
                seen.append((r, u, f, None if self.top is None else int(nz[r, 0])))
                plan["kept"][frame, r], plan["kl"][frame, r], plan["x_next"][r] = h[r], self.kl(u, f), h[r] + STEP
        self.log.append(("head", frame, None if active is None else tuple(active), seen))

    def spec(self):
        return gen.DeviceHeadSpec(self.plan, self.call, (), "kept", 1)

    def noise(self, n):
        """[top, n, 1]: noise[f, u] = 1000 f + u"""
        return (1000.0 * torch.arange(self.top).view(-1, 1, 1) + torch.arange(n).view(1, -1, 1)).float()


class FakeEvent:
    def record(self):
        pass

    def synchronize(self):
        pass


@contextlib.contextmanager
def without_device():
    """the three things the collaborators ask of a device, replaced: the row copy, the pinned buffer, the event"""
    empty = torch.empty
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))
        mp.setattr(torch.cuda, "Event", FakeEvent)
        mp.setattr(gen.ops, "copy_rows", lambda src, dst, *a, **k: dst.copy_(src.reshape(dst.shape)))
        yield


@pytest.fixture
def no_device():
    with without_device():
        yield


def prompts_of(lens):
    return [(torch.full((n,), u), None) for u, n in enumerate(lens)]


def frames_of(u, n):
    """what `infer` returns for an utterance that ran n frames: [1, 2, n - 1], frame j = (u, j)"""
    return torch.tensor([[float(u), float(j)] for j in range(n - 1)]).view(1, n - 1, 2).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ refill
class LoggedSchedule(gen.RowSchedule):
    """RowSchedule that notes (step, admitted pairs, live rows) of every step the loop enqueues"""

    def __init__(self, n, R, log):
        super().__init__(n, R)
        self.log, self.pairs = log, []

    def admit(self, step):
        self.pairs = super().admit(step)
        return self.pairs

    def live(self, step):
        now = super().live(step)
        if self.log is not None:
            self.log.append((step, self.pairs, now))
        return now


def drive(frames, R, stop_lag=0, log=None, host=False):
    """`generate(refill=True)` on the fakes, the stops those of the caps: utterance u runs frames[u] frames.  Returns the
    schedule, the owner (its log) and the results.  log: receives (step, admitted pairs, live rows) per step."""
    N, top, R = len(frames), max(frames), min(R, len(frames))
    owner = FakeOwner([None] * N, R, top)
    embeds = gen._prompt_embeds(owner, prompts_of([3 + u % 4 for u in range(N)]))
    ring = top + stop_lag
    sched = LoggedSchedule(N, R, log)
    with without_device():
        rows = gen.BatchRows(owner.base_model.model, embeds, R, 6 + top, host, packed=True)
        head = gen.HostHead(owner, R, ring) if host else gen.DeviceHead(owner, owner.spec(), R, ring, "cpu", owner.noise(N), False)
        results = gen.run_frames(sched, rows, head, 0.0, list(frames), ring, stop_lag)
    return sched, owner, results


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("i", range(len(LISTS)))
def test_refill_call_script(no_device, i, lag):
    frames, R = LISTS[i]
    R = min(R, len(frames))
    top, ring = max(frames), max(frames) + lag
    sched, owner, results = drive(frames, R, lag)
    total, first = gen.refill_steps(frames, R, stop_lag=lag)
    assert sched.trace == [(u, r, t, n) for u, ((r, t), n) in enumerate(zip(first, frames))] and sched.steps == total
    # what the closed form says of every step: who is in which row (the look-ahead frame of stop_lag=1 included)
    occupied = [[None] * R for _ in range(total + lag)]
    for u, ((r, t), n) in enumerate(zip(first, frames)):
        for s in range(t, t + n + lag):
            assert occupied[s][r] is None
            occupied[s][r] = u
    log = [e for e in owner.log if e[0] != "plan"]
    assert owner.log[0] == ("plan", R, ring) and len(owner.base_model.model.caches) == 1
    k = 0
    for s, occ in enumerate(occupied):
        admitted = [(u, r) for r, u in enumerate(occ) if u is not None and first[u][1] == s]
        cont = tuple(u is not None and first[u][1] < s for u in occ)
        if any(cont):                                   # decode-active: occupied and not just admitted
            assert log[k] == ("decode", cont, False), (s, log[k])
            k += 1
        if admitted:                                    # ONE packed prefill of exactly the admitted pairs (the fake refuses a length not reset)
            assert log[k] == ("prefill_rows", sorted(admitted), False), (s, log[k])
            k += 1
        name, slot, active, seen = log[k]
        k += 1
        assert name == "head" and slot == s % ring and active == tuple(u is not None for u in occ)      # head-active: occupied
        want = [(r, u, s - first[u][1], min(s - first[u][1], top - 1) * 1000 + u) for r, u in enumerate(occ) if u is not None]
        assert seen == want, (s, seen, want)            # the row holds its utterance's frame, and drew noise[min(f, top - 1), u]
    assert k == len(log)
    for u, n in enumerate(frames):        # cut from slots (s - f + j) % ring: its own frames 0 .. n - 2
        assert torch.equal(results[u], frames_of(u, n)), (u, results[u])
    cache = owner.base_model.model.caches[0]
    for r in range(R):            # a row's last occupant: prompt, fed-back frames, look-ahead
        u = max(u for u, (r0, _) in enumerate(first) if r0 == r)
        assert cache["len"][r] == 3 + u % 4 + frames[u] - 1 + lag


@pytest.mark.parametrize("i", [0, 1, 2, 4, 5])
def test_refill_host_head(no_device, i):
    """the host head on the same loop: one _host_frame per step, audio_linear only when a row continues, the same results"""
    frames, R = LISTS[i]
    sched, owner, results = drive(frames, R, 0, host=True)
    total, first = gen.refill_steps(frames, min(R, len(frames)))
    assert sched.steps == total and [(r, t) for _, r, t, _ in sched.trace] == first
    names = [e[0] for e in owner.log]
    assert names.count("head") == total and names.count("audio_linear") == names.count("decode") <= total - 1
    assert all(e[2] is True for e in owner.log if e[0] in ("decode", "prefill_rows"))  # the host head reads normed rows
    for u, n in enumerate(frames):
        assert torch.equal(results[u], frames_of(u, n)), (u, results[u])


# ------------------------------------------------------------------------------------------------ a group without refill
def parent_grouped(R, max_length, stops, lag):
    """The call script of one group as the loops this module replaced ran it (generate_device_head; generate_host_batch is its
    lag = 0 case), written out from their control flow and independent of run_frames: every prompt prefilled in ascending row
    order, then per frame the decode step and the head for the rows still active; a row leaves at its KL stop or its cap; with
    lag = 1 frame i + 1 is enqueued before frame i is resolved - but never a frame >= max(max_length).  Returns (script, frames
    per row)."""
    caps = max_length if isinstance(max_length, list) else None
    top = max(caps) if caps else max_length
    caps = caps or [top + 1] * R
    active, count, script = [True] * R, [0] * R, []

    def enqueue(i):
        if i == 0:
            script.extend(("prefill", r) for r in range(R))
        else:
            script.append(("decode", tuple(active)))
        script.append(("head", i, tuple(active)))

    def resolve(i):
        for r in range(R):
            if active[r]:
                count[r] = i + 1
                if (stops[r] == i + 1 and i > 3) or i + 1 >= caps[r]:
                    active[r] = False

    if lag:
        enqueue(0)
    for i in range(top):
        if not lag:
            enqueue(i)
        elif i + 1 < top:
            enqueue(i + 1)
        resolve(i)
        if not any(active):
            break
    return script, count


def grouped_cases():
    g = random.Random(2)
    cases = []
    for k in range(60):
        R = g.randint(1, 6)
        top = g.randint(1, 12)
        caps = top if k % 2 else [g.randint(1, top) for _ in range(R)]
        stops = [g.choice([None, None, g.randint(5, 13)]) for _ in range(R)]
        cases.append((R, caps, stops))
    cases.append((3, 9, [None, None, None]))            # every row at the cap: the look-ahead frame 9 must not run
    cases.append((1, 7, [None]))
    return cases


@pytest.mark.parametrize("head", ["host", "dev0", "dev1"])
def test_grouped_call_script_is_the_parents(no_device, head):
    lag, host = int(head == "dev1"), head == "host"
    for R, caps, stops in grouped_cases():
        if host and min(caps if isinstance(caps, list) else [caps]) < 2:
            continue                                    # (the host head cannot return zero frames: torch.stack of nothing raises)
        top = max(caps) if isinstance(caps, list) else caps
        lens = [2 + (3 * r) % 5 for r in range(R)]
        owner = FakeOwner(stops, top=None if host else top)
        results = gen.generate(owner, prompts_of(lens), 0.0, caps, None if host else owner.spec(),
                               None if host else owner.noise(R), lag)
        script, count = parent_grouped(R, caps, stops, lag)
        one = R == 1
        got = []
        for e in owner.log:
            if e[0] == "prefill":
                assert e[2] is host
                got.append(e[:2])
            elif e[0] == "decode":
                assert e[2] is host
                got.append(("decode", (True,) if one else e[1]))
            elif e[0] == "head" and not host:
                assert e[2] == (None if one else script[len(got)][2])          # one row: the head runs without an active list
                got.append(("head", e[1], script[len(got)][2]))
                assert all((r, u, f) == (r, r, e[1]) and nz == 1000 * f + u for r, u, f, nz in e[3])
            elif e[0] == "head":
                got.append(script[len(got)])            # (the host head sees neither slot nor active list: one call per step)
                assert got[-1][0] == "head"
        assert got == script, (R, caps, stops, lag, got, script)
        assert max(e[1] for e in script if e[0] == "head") < top               # no step >= max_length is ever enqueued
        assert not hasattr(owner, "last_refill_trace")
        model = owner.base_model.model
        assert len(model.caches) == 1 and model.caches[0]["room"] == max(lens) + top
        steps = [sum(1 for e in script if e[0] == "decode" and e[1][r]) for r in range(R)]
        assert model.caches[0]["len"] == (lens[0] + steps[0] if one else [n + s for n, s in zip(lens, steps)])
        for r in range(R):
            assert torch.equal(results[r], frames_of(r, count[r])), (R, caps, stops, r)
        if host:                                        # audio_linear: once per decode step, never after the last frame
            assert [e[0] for e in owner.log].count("audio_linear") == sum(1 for e in script if e[0] == "decode")


def test_a_stopped_row_is_never_active_again(no_device):
    owner = FakeOwner([5, None, 6], top=9)
    gen.generate(owner, prompts_of([2, 3, 4]), 0.0, 9, owner.spec(), owner.noise(3), 1)
    seen = [e[2] for e in owner.log if e[0] == "head"]
    for r in range(3):
        flags = [a[r] for a in seen]
        assert flags == sorted(flags, reverse=True)
    assert [sum(a[r] for a in seen) for r in range(3)] == [6, 9, 7]            # 5 / 9 / 6 frames, the look-ahead where one ran


# ------------------------------------------------------------------------------------------------ one row
@pytest.mark.parametrize("head", ["host", "dev0", "dev1"])
def test_one_prompt_runs_on_the_one_row_cache(no_device, head):
    host = head == "host"
    owner = FakeOwner([6], top=None if host else 8)
    out = gen.generate(owner, prompts_of([4]), 0.0, 8, None if host else owner.spec(), None if host else owner.noise(1),
                       int(head == "dev1"))
    model = owner.base_model.model
    assert len(model.caches) == 1 and isinstance(model.caches[0]["len"], int)              # init_cache, not init_cache_batch
    assert model.caches[0]["len"] == 4 + 5 + int(head == "dev1") and model.caches[0]["room"] == 12
    steps = 5 + int(head == "dev1")
    assert [e[:2] for e in owner.log if e[0] in ("prefill", "decode")] == [("prefill", 0)] + [("decode", None)] * steps
    if not host:
        assert all(e[2] is None for e in owner.log if e[0] == "head")                      # active=None
    assert len(out) == 1 and torch.equal(out[0], frames_of(0, 6))
