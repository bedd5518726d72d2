"""Llasa train step (model_sigmaVAE.Llasa.forward + backward + fused AdamW) at the Llama-3.2-1B shape the reference trains
(hidden 2048, 16 layers, 32 heads / 8 kv heads, intermediate 8192, vocab 128256 + 8 special tokens, latent_dim 64),
random weights, synthetic batch: text prefix + audio frames per sample.   python tools/llasa_bench.py [B] [L] [steps]
The decoder shape is an option (defaults: Llama-3.2-1B): --hidden --layers --heads --kv-heads --head-dim --inner, e.g. the
Llama-3.2-3B shape  --hidden 3072 --layers 28 --heads 24 --kv-heads 8 --head-dim 128 --inner 8192
--infer-only: KV-cached generation only; --infer-batch R: also Llasa.infer_batch on R prompts (aggregate and per-row frames/s)
--decode-weights e4m3: the --infer-only and --infer-batch lines with Llasa.quantize_decoder("e4m3") (weight-only FP8 decode steps)
--device-head: after the host-head lines, the same KV-cached generation with device_head=True (the per-frame head as one call of
kalle_llasa_frame_head_rows) in the same process, each line with its ratio to the host-head line; --stop-lag N (0 or 1): one more
set of lines with stop_lag=N
--infer-batch R accepts up to 64 rows (above 16: infer_batch(rows=R), the wide decode step).
--wide-list [--refill] [--device-head]: INSTEAD of the lines above, 64 prompts x 200 frames through infer_batch with rows=16, 32 and
64 in one process, three repeats each (min - max, ms per step, the acceptance comparison of DESIGN.md 5.16).
--infer-batch R --refill [--utterances N]: INSTEAD of the lines above, N (default 64) prompts with per-prompt frame caps drawn in
50 .. 250 (random.Random(0), printed; the stop threshold off) through infer_batch(refill=False) and infer_batch(refill=True) in one
process, alternating, three repeats each, for every head selected: aggregate frames/s of both (min - max), the measured gain next
to the step ratio refill_steps predicts for the list, then the time to the first frame of R prompts prefilled one by one
(prefill_row) and packed (prefill_rows)
--scale-head: the generation lines for model.Llasa (the mean || log-scale head of train.py / configs/twj_0828.yaml; its device
head is kalle_llasa_frame_head2_rows) in place of model_sigmaVAE.Llasa; implies --infer-only
--ragged SEED [--pack]: the train step on a batch shaped like the reference's collate - sample 0 at full length L, the others
with lengths drawn uniformly from [L/4, L], right-padded (about 35 % padding) - with Llasa.pack_sequences() when --pack is given;
prints ms/step, LIVE tokens/s and the padding share
--ragged SEED --ab [REPEATS]: the three arms in ONE process on the same batch, alternating, REPEATS (default 3) timed windows
each: padded (the default path), packed (pack_sequences()), and the floor - a dense unpadded batch [1, total_rows] of the packed
row count; and the time of the one host read of the lengths per packed step"""
import json, os, sys, tempfile, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kalle_audio_amd.engine import DataParallelTrainer
SCALE_HEAD = "--scale-head" in sys.argv      # model.Llasa (predicted scale) in place of model_sigmaVAE.Llasa (fixed std)
if SCALE_HEAD:
    sys.argv.remove("--scale-head")
    from kalle_audio_amd.model import Llasa
    if "--infer-only" not in sys.argv:
        sys.argv.append("--infer-only")
else:
    from kalle_audio_amd.model_sigmaVAE import Llasa
SHAPE = {"--hidden": 2048, "--layers": 16, "--heads": 32, "--kv-heads": 8, "--head-dim": 64, "--inner": 8192}
for _o in SHAPE:
    if _o in sys.argv:
        _i = sys.argv.index(_o)
        SHAPE[_o] = int(sys.argv[_i + 1])
        del sys.argv[_i:_i + 2]
INFER_BATCH = 0                              # --infer-batch R: Llasa.infer_batch on R prompts next to the batch-1 line
if "--infer-batch" in sys.argv:
    _i = sys.argv.index("--infer-batch")
    INFER_BATCH = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
    if "--infer-only" not in sys.argv and "--infer" not in sys.argv:
        sys.argv.append("--infer-only")
DECODE_WEIGHTS = None                        # --decode-weights e4m3: generation streams e4m3 weights (prefill stays bf16)
if "--decode-weights" in sys.argv:
    _i = sys.argv.index("--decode-weights")
    DECODE_WEIGHTS = sys.argv[_i + 1]
    del sys.argv[_i:_i + 2]
HEADS = [("host head", {})]                  # (label, keywords of infer / infer_batch); --device-head / --stop-lag N add to it
if "--device-head" in sys.argv:
    sys.argv.remove("--device-head")
    HEADS.append(("device head", dict(device_head=True)))
if "--stop-lag" in sys.argv:
    _i = sys.argv.index("--stop-lag")
    _lag = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
    if len(HEADS) < 2:
        sys.exit("--stop-lag belongs to --device-head")
    if _lag:
        HEADS.append((f"device head, stop_lag={_lag}", dict(device_head=True, stop_lag=_lag)))
REFILL = "--refill" in sys.argv               # --infer-batch R --refill [--utterances N]: infer_batch(refill=True) against the groups
if REFILL:
    sys.argv.remove("--refill")
    if not INFER_BATCH and "--wide-list" not in sys.argv:
        sys.exit("--refill belongs to --infer-batch R or --wide-list")
WIDE_LIST = "--wide-list" in sys.argv         # --wide-list [--refill]: 64 prompts x 200 frames with rows=16 / 32 / 64 in ONE process
if WIDE_LIST:
    sys.argv.remove("--wide-list")
    if "--infer-only" not in sys.argv and "--infer" not in sys.argv:
        sys.argv.append("--infer-only")
UTTERANCES = 64
if "--utterances" in sys.argv:
    _i = sys.argv.index("--utterances")
    UTTERANCES = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
RAGGED = None                                # --ragged SEED: a right-padded batch with lengths from [L/4, L]
if "--ragged" in sys.argv:
    _i = sys.argv.index("--ragged")
    RAGGED = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
PACK = "--pack" in sys.argv
if PACK:
    sys.argv.remove("--pack")
AB = 0                                       # --ab [REPEATS]: padded / packed / dense floor in one process, alternating
if "--ab" in sys.argv:
    _i = sys.argv.index("--ab")
    _n = sys.argv[_i + 1] if _i + 1 < len(sys.argv) and sys.argv[_i + 1].isdigit() else None
    AB = int(_n) if _n else 3
    del sys.argv[_i:_i + (2 if _n else 1)]
if (PACK or AB) and RAGGED is None:
    sys.exit("--pack and --ab belong to --ragged SEED")
HID, NLAYER = SHAPE["--hidden"], SHAPE["--layers"]
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(_pos[0]) if len(_pos) > 0 else 8
L = int(_pos[1]) if len(_pos) > 1 else 1024
steps = int(_pos[2]) if len(_pos) > 2 else 5
cfg = dict(model_type="llama", vocab_size=128256, hidden_size=HID, intermediate_size=SHAPE["--inner"], num_hidden_layers=NLAYER,
           num_attention_heads=SHAPE["--heads"], num_key_value_heads=SHAPE["--kv-heads"], head_dim=SHAPE["--head-dim"],
           rms_norm_eps=1e-5, rope_theta=500000.0,
           rope_scaling=dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                             original_max_position_embeddings=8192), tie_word_embeddings=True)
d = tempfile.mkdtemp(prefix="kalle_llama_")
json.dump(cfg, open(os.path.join(d, "config.json"), "w"))


class Tok:
    def __len__(self):
        return 128264


dev = torch.device("cuda")
torch.manual_seed(0)
with torch.device(dev):
    m = Llasa({"llm_model_name_or_path": d, "latent_dim": 64, "audio_proj_dim": HID}, Tok(), use_flash_attention=False)
INFER_ONLY = "--infer-only" in sys.argv      # generation with the KV cache only (for profiling the decode step)
tr = None if INFER_ONLY else DataParallelTrainer(m, lr=1e-5, optimizer="AdamW", weight_decay=0.01)
nparam = sum(p.numel() for p in m.parameters())
ids = torch.randint(0, 128264, (B, L), device=dev)
lat = torch.randn(B, L, 64, device=dev)
lbl = torch.randn(B, L, 64, device=dev)
ids_mask = torch.zeros(B, L, device=dev); ids_mask[:, :64] = 1
audio_mask = 1 - ids_mask
target_mask = torch.zeros(B, L, device=dev); target_mask[:, 63:L - 1] = 1
end_mask = torch.zeros(B, L, device=dev); end_mask[:, L - 1] = 1


def ragged_batch(lens, width):
    """masks of a collate-shaped batch: 64 text tokens (fewer for a short sample), audio frames up to the sample's length, padding"""
    im, am, tm, em = (torch.zeros(len(lens), width) for _ in range(4))
    for b, n in enumerate(lens):
        nt = min(64, n // 2)
        im[b, :nt] = 1
        am[b, nt:n] = 1
        tm[b, nt - 1:n - 1] = 1
        em[b, n - 1] = 1
    return tuple(t.to(dev) for t in (im, am, tm, em))


LENS = None
if RAGGED is not None:
    g = torch.Generator().manual_seed(RAGGED)
    LENS = [L] + [int(v) for v in torch.randint(L // 4, L + 1, (B - 1,), generator=g)]
    ids_mask, audio_mask, target_mask, end_mask = ragged_batch(LENS, L)
    LIVE = sum(LENS)
    print(f"ragged batch (seed {RAGGED}): lengths {LENS}, {LIVE} live of {B * L} positions, padding share {1 - LIVE / (B * L):.3f}")


def step(batch=None):
    out = m(*(batch or (ids, lat, lbl, ids_mask, audio_mask, target_mask, end_mask)))
    tr.backward(out["audio_loss"] * 1.0 + out["end_loss"] * 1.0)
    return out


def timed(batch, pack, n):
    """ms per step over a window of n steps that ends in a device synchronise"""
    m.pack_sequences(pack)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        o = step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3, o


if AB:
    from kalle_audio_amd import llama_ops as LO
    rows = -(-LIVE // LO.PACK_GRANULE) * LO.PACK_GRANULE
    padded = (ids, lat, lbl, ids_mask, audio_mask, target_mask, end_mask)
    # the floor: a dense batch without padding of the packed row count, B equal sequences (no more attention work than the ragged
    # lengths need: sum of squares is least for equal lengths)
    Bd, Ld = (B, rows // B) if rows % B == 0 else (1, rows)
    dense = (torch.randint(0, 128264, (Bd, Ld), device=dev), torch.randn(Bd, Ld, 64, device=dev), torch.randn(Bd, Ld, 64, device=dev),
             *ragged_batch([Ld] * Bd, Ld))
    print(f"dense floor: B={Bd} L={Ld} ({rows} rows, no padding)")
    arms = [("padded", padded, False), ("packed", padded, True), ("dense floor", dense, False)]
    for name, batch, pack in arms:                    # warm every shape the timed windows use
        timed(batch, pack, 2)
    res = {name: [] for name, _, _ in arms}
    for r in range(AB):
        for name, batch, pack in (arms if r % 2 == 0 else arms[::-1]):      # alternate the order
            ms, o = timed(batch, pack, steps)
            res[name].append(ms)
            print(f"repeat {r} {name:12s}: {ms:8.2f} ms/step  (loss {o['audio_loss'].item():.3f})")
    mask = ids_mask + audio_mask
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        LO.packed_lengths((mask > 0).cpu())
    read_ms = (time.perf_counter() - t0) / 20 * 1e3
    for name, _, _ in arms:
        v = sorted(res[name])
        n_live = rows if name == "dense floor" else LIVE
        print(f"{name:12s} B={B} L={L}: median {v[len(v) // 2]:.2f} ms/step (min {v[0]:.2f}, max {v[-1]:.2f}), "
              f"{n_live / v[len(v) // 2] * 1e3:.0f} live tokens/s, rows through the decoder {B * L if name == 'padded' else rows}")
    print(f"padding share {1 - LIVE / (B * L):.3f}; packed rows {rows}; host read of the lengths (idle device): {read_ms:.3f} ms per step")
    sys.exit(0)
if PACK:
    m.pack_sequences()

for _ in range(0 if INFER_ONLY else 2):
    out = step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(0 if INFER_ONLY else steps):
    out = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
# algorithmic FLOPs: 6 * (non-embedding params) per token + attention 12 * L * D per token per layer (causal: half)
nonemb = nparam - 128264 * HID
fl = (6.0 * nonemb + NLAYER * 12.0 * L * HID * 0.5) * B * L
if not INFER_ONLY and RAGGED is not None:
  print(f"Llasa ragged train step ({'packed' if PACK else 'padded'}) B={B} L={L}: {dt*1e3:.1f} ms/step, {LIVE/dt:.0f} live tokens/s, "
        f"padding share {1 - LIVE / (B * L):.3f}, loss {out['audio_loss'].item():.3f}")
elif not INFER_ONLY:
  print(f"Llasa {'Llama-3.2-1B-shape' if HID == 2048 and NLAYER == 16 else f'hidden-{HID}-x-{NLAYER}-layers'} train step B={B} L={L}: {dt*1e3:.1f} ms/step, {B*L/dt:.0f} tokens/s, "
        f"{B*L/12.5/dt:.0f} audio-s/s (12.5 Hz frames), {fl/dt/1e12:.0f} TFLOP/s algorithmic, params {nparam/1e9:.2f} B, "
        f"loss {out['audio_loss'].item():.3f}")

if WIDE_LIST:
    # the wide step's acceptance measurement: UTTERANCES prompts of 64 / 56 / 48 / 40 tokens, 200 frames each (no early stop), the
    # whole infer_batch call timed, rows = 16 / 32 / 64 in one process, three repeats each with the order rotating; grouped, and
    # with --refill also refill=True.  Accepted: min of the wide repeats above max of the 16-row repeats, in aggregate frames/s.
    m.eval()
    nfr = 200
    prompts = [(torch.randint(0, 128264, (64 - 8 * (r % 4),), device=dev), None) for r in range(UTTERANCES)]
    ROWS = (16, 32, 64)

    def run(rows, refill, kw, frames=nfr):
        torch.cuda.synchronize()
        t = time.perf_counter()
        outs = m.infer_batch(prompts, end_disp_kl_thres=-1.0, max_length=frames, refill=refill, rows=rows, **kw)
        torch.cuda.synchronize()
        assert len(outs) == UTTERANCES and all(o.shape[2] == frames - 1 for o in outs)
        return time.perf_counter() - t

    for label, kw in HEADS:
        for refill in ((False, True) if REFILL else (False,)):
            for rows in ROWS:
                run(rows, refill, kw, frames=4)
            dts = {rows: [] for rows in ROWS}
            for rep in range(3):
                for rows in ROWS[rep:] + ROWS[:rep]:
                    dts[rows].append(run(rows, refill, kw))
            fps = {rows: sorted(UTTERANCES * nfr / dt for dt in v) for rows, v in dts.items()}
            steps = {rows: -(-UTTERANCES // rows) * nfr for rows in ROWS}
            mode = "refill" if refill else "grouped"
            for rows in ROWS:
                print(f"wide list [{label}, {mode}] rows={rows}: {fps[rows][0]:.0f} - {fps[rows][-1]:.0f} frames/s aggregate (min - max of 3), "
                      f"{min(dts[rows]) / steps[rows] * 1e3:.3f} - {max(dts[rows]) / steps[rows] * 1e3:.3f} ms/step incl. prefill")
            ok = all(fps[rows][0] > fps[16][-1] for rows in (32, 64))
            print(f"wide list [{label}, {mode}]: min(rows=32) {fps[32][0]:.0f}, min(rows=64) {fps[64][0]:.0f} against max(rows=16) "
                  f"{fps[16][-1]:.0f} frames/s: {'ACCEPTED' if ok else 'NOT accepted'}; rows=64 / rows=16 x "
                  f"{fps[64][0] / fps[16][-1]:.2f} - x {fps[64][-1] / fps[16][0]:.2f}")
    sys.exit(0)

if REFILL:
    # a ragged list through both modes of infer_batch in ONE process: UTTERANCES prompts of 64 / 56 / 48 / 40 tokens on R rows,
    # per-prompt frame caps from a seeded draw in 50 .. 250 (the stop threshold off, so the caps alone decide the lengths)
    import random
    from kalle_audio_amd.model_sigmaVAE import grouped_steps, refill_steps
    m.eval()
    if DECODE_WEIGHTS:
        m.quantize_decoder(DECODE_WEIGHTS)
    R = m.infer_batch_rows = INFER_BATCH
    ROWS_KW = dict(rows=R) if R > 16 else {}               # (above 16 rows: the wide step, asked for per call)
    rng = random.Random(0)
    caps = [rng.randint(50, 250) for _ in range(UTTERANCES)]
    prompts = [(torch.randint(0, 128264, (64 - 8 * (r % 4),), device=dev), None) for r in range(UTTERANCES)]
    frames = sum(caps)
    print(f"refill: {UTTERANCES} utterances on {R} rows, decode weights {DECODE_WEIGHTS or 'bf16'}, frame caps (random.Random(0), 50 .. 250): {caps}")
    print(f"  {frames} frames; decoder steps predicted: grouped {grouped_steps(caps, R)}, refill {refill_steps(caps, R)[0]} "
          f"(stop_lag=1: {refill_steps(caps, R, 1)[0]})")

    def run(refill, kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        outs = m.infer_batch(prompts, end_disp_kl_thres=-1.0, max_length=caps, refill=refill, **ROWS_KW, **kw)
        torch.cuda.synchronize()
        assert [o.shape[2] for o in outs] == [n - 1 for n in caps]
        return time.perf_counter() - t

    for label, kw in HEADS:
        pred = grouped_steps(caps, R) / refill_steps(caps, R, kw.get("stop_lag", 0))[0]
        for refill in (False, True):                      # warm every shape the timed runs use: one whole run of each mode
            run(refill, kw)
        dts = {False: [], True: []}
        for rep in range(3):
            for refill in ((False, True) if rep % 2 == 0 else (True, False)):      # alternate the order
                dts[refill].append(run(refill, kw))
        fps = {k: sorted(frames / dt for dt in v) for k, v in dts.items()}
        print(f"refill [{label}]: grouped {fps[False][0]:.0f} - {fps[False][-1]:.0f} frames/s aggregate, refill {fps[True][0]:.0f} - "
              f"{fps[True][-1]:.0f} frames/s aggregate (min - max of 3), measured gain x {min(dts[False]) / min(dts[True]):.3f} - "
              f"x {max(dts[False]) / max(dts[True]):.3f} (best / worst runs), step ratio predicted x {pred:.3f}; "
              f"grouped {min(dts[False]) * 1e3:.0f} ms, refill {min(dts[True]) * 1e3:.0f} ms")
    # time to the first frame of R prompts: every prompt through the stack alone (prefill_row) against one packed pass (prefill_rows)
    model = m.base_model.model
    with torch.no_grad():
        embeds = [model.embed_tokens(ids.unsqueeze(0)) for ids, _ in prompts[:R]]
        room = max(e.shape[1] for e in embeds) + 8

        def first_frame(packed):
            cache = model.init_cache_batch(R, room, dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            if packed:
                h = model.prefill_rows(embeds, cache, list(range(R)))
            else:
                h = torch.cat([model.prefill_row(e, cache, r)[:, -1:, :] for r, e in enumerate(embeds)], dim=0)
            m._host_frame(h)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        for packed in (False, True):
            first_frame(packed)
        ms = {False: [], True: []}
        for rep in range(3):
            for packed in ((False, True) if rep % 2 == 0 else (True, False)):
                ms[packed].append(first_frame(packed))
    print(f"time to the first frame, {R} prompts of {[e.shape[1] for e in embeds[:4]]} ... tokens (prefill + the host head): one by one "
          f"{min(ms[False]):.2f} - {max(ms[False]):.2f} ms, packed {min(ms[True]):.2f} - {max(ms[True]):.2f} ms (min - max of 3)")
    sys.exit(0)

if "--infer" in sys.argv or INFER_ONLY:
    # frame-by-frame generation (Llasa.infer): 64 prompt tokens, 200 frames, KV cache vs the reference's full re-forward
    m.eval()
    if SCALE_HEAD:
        print("model.Llasa: the head predicts mean || log-scale (latent 64, audio_proj_dim = hidden)")
    if DECODE_WEIGHTS:
        m.quantize_decoder(DECODE_WEIGHTS)
        print(f"decode weights: {DECODE_WEIGHTS} (use_cache=True lines; quantised at the first step, inside the warm-up call)")
    pid = torch.randint(0, 128264, (64,), device=dev)
    for use_cache, nfr in ((True, 200),) if INFER_ONLY else ((True, 200), (False, 200)):
        for label, kw in HEADS if use_cache else HEADS[:1]:
            m.infer(pid, None, end_disp_kl_thres=-1.0, max_length=4, use_cache=use_cache, **kw)
            for rep in range(3 if INFER_ONLY else 1):          # (--infer-only: three repeats, for a min and a max)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.infer(pid, None, end_disp_kl_thres=-1.0, max_length=nfr, use_cache=use_cache, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                tag = "" if not kw else f" [{label}: {nfr/dt/one_fps:.3f} x the host head's last repeat]"
                print(f"infer use_cache={use_cache}: {nfr} frames in {dt*1e3:.0f} ms = {nfr/dt:.1f} frames/s "
                      f"({nfr/dt/12.5:.2f} x real time at 12.5 Hz), out {tuple(out.shape)}{tag}")
            if use_cache and not kw:
                one_fps = nfr / dt

if INFER_BATCH:
    # the same generation for R utterances at once (Llasa.infer_batch): prompts of 64, 56, 48, ... tokens, 200 frames each
    m.eval()
    m.infer_batch_rows = max(m.infer_batch_rows, INFER_BATCH)
    nfr = 200
    prompts = [(torch.randint(0, 128264, (64 - 8 * (r % 4),), device=dev), None) for r in range(INFER_BATCH)]
    ROWS_KW = dict(rows=INFER_BATCH) if INFER_BATCH > 16 else {}       # (above 16 rows: the wide step, asked for per call)
    for label, kw in HEADS:
        kw = dict(kw, **ROWS_KW)
        m.infer_batch(prompts, end_disp_kl_thres=-1.0, max_length=4, **kw)
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = m.infer_batch(prompts, end_disp_kl_thres=-1.0, max_length=nfr, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            R = len(outs)
            tag = "" if label == "host head" else f" [{label}: {host_dt/dt:.3f} x the host head's last repeat]"
            print(f"infer_batch R={R} (repeat {rep}): {nfr} frames x {R} rows in {dt*1e3:.0f} ms = {dt/nfr*1e3:.3f} ms/step incl. prefill, "
                  f"{R*nfr/dt:.1f} frames/s aggregate, {nfr/dt:.1f} frames/s per row, "
                  f"{R*nfr/dt/one_fps:.2f} x {R} sequential infer calls ({one_fps:.1f} frames/s), out {tuple(outs[0].shape)}{tag}")
        if label == "host head":
            host_dt = dt
