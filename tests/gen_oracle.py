"""KV-cached Llasa generation held to an fp64 oracle, frame by frame.  Pure torch on the CPU; shared by tests/test_gen_oracle_cpu.py
(the yardstick, the seeded defects and the blindness of the fixture gains, on the reference itself) and
tests/test_generation_oracle_gpu.py (LlamaModel's cache API and Llasa.infer / infer_batch on the HIP path).

State      gu.make_state(gs.llasa_shapes(c), seed) with every RMSNorm gain mapped from 0.1 n to 1 + 0.1 n ("sensitive").  With the
           fixture gains the normalised streams are x 0.1, the scores are tiny, the softmax is flat and both branches are small
           against the residual: a wrong rotary position or a missing key moves nothing a test can see ("Generation per
           frame").  gains="fixture" keeps them, for the test that shows exactly that.
Reference  teacher forced: a row is [embed(ids) | audio_linear(prompt latents) | audio_linear(latents fed back for frames 0 .. T-2)]
           (or the caller's own embeddings), run ONCE through the decoder layers of oracle/kalle_oracle.py - the layer is causal, so
           position P - 1 + i is frame i - then through the head.  Per position: the stream before the final norm ("pre") and the
           hidden state; per frame (positions P - 1 on, the only ones whose mean generation ever uses): the predicted mean and
           the frame KL (llasa_head_refs.kl).  Every frame is compared on identical inputs.
Modes      f64 (the reference), emu and heavy: grad_slices.emulate, the bf16-operand emulations of the gradient checks.
e4m3       the four projections of every layer (q | k | v, o, up | gate, down), AT THE POSITIONS A DECODE STEP COMPUTED
           (row["step_from"] on: forward_cached with one position, forward_cached_batch; prefill keeps the bf16 weights), are the
           dequantised values decode_table()[codes] scale of fp8_refs.quantize_ref on the bf16-rounded weight, so quantisation
           error is not part of what is measured.  The emulation rounds the activation operand there and nothing else: the kernels
           widen the codes exactly and apply the scale in fp32 (include/kalle_hip.h, "weight-only FP8 decoding").
Check      per quantity and (row, position): |x - x64| / max(|x64| at that position, 0.25 rms over the row's positions of |x64|).
           Yardstick r(case, quantity) = the largest such ratio of emu against f64: from the reference alone.  Assertion:
           ratio <= M r, M = grad_slices.M = 3, at every row and position.
Defects    seeded into the REFERENCE: through the forward's own positions and allow-mask (rotary positions of the fed-back positions
           shifted by one, the newest key / key 0 / key P - 1 masked for them), or on its outputs (two rows swapped, one frame of one
           row x 1.10, frames shifted by one).
Stop rule  kl_allowance: what an error of M r on a mean can do to that frame's KL; stop_plan: the threshold in the widest gap of the
           fp64 frame KLs, the frame counts they predict, and the margin - the distance of the nearest frame KL to the threshold
           in allowances.  Above 1 the fp64 KLs decide where every row stops."""
import contextlib
import math
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp8_refs  # noqa: E402
import grad_slices as gs  # noqa: E402
import llasa_head_refs as hr  # noqa: E402

gu, ko = gs.gu, gs.ko
F64, M, STD = torch.float64, gs.M, 0.5
CASES = gs.LLASA_CASES
FMTS = (None, "e4m3")
QUANTITIES = ("pre", "hidden", "mean")
PROJ = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
        "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
MASK_DEFECTS = ("newest key masked", "key 0 masked", "key P-1 masked")
FORWARD_DEFECTS = ("position gap 1",) + MASK_DEFECTS


def fmt_id(fmt):
    return fmt or "bf16"


# ------------------------------------------------------------------------------------------------ state
def make_state(c, gains="sensitive"):
    """name -> numpy fp32 under the reference's (HF) names.  sensitive: RMSNorm gains 1 + 0.1 n; fixture: 0.1 n as make_param
    draws them"""
    st = gu.make_state(gs.llasa_shapes(c), c["seed"])
    if gains == "sensitive":
        for n in st:
            if n.endswith("norm.weight"):
                st[n] = (1.0 + st[n]).astype(st[n].dtype)
    else:
        assert gains == "fixture", gains
    return st


def dequantised(w):
    """fp64 values the e4m3 kernels multiply by: quantize_ref of the bf16 compute copy, decoded and scaled (one scale per row, so
    the rows of a fused q | k | v or up | gate matrix quantise as those of its parts)"""
    codes, scale = fp8_refs.quantize_ref(w.to(torch.bfloat16))
    return fp8_refs.decode_table()[codes.long()] * scale.double()[:, None]


def weights(c, st, fmt=None):
    """the oracle's state in fp64; fmt "e4m3": every projection is the pair (weight, dequantised weight)"""
    sd = {k: torch.from_numpy(v).to(F64) for k, v in st.items()}
    if fmt is not None:
        assert fmt == "e4m3", fmt
        for k in list(sd):
            if k.endswith(PROJ):
                sd[k] = (sd[k], dequantised(sd[k]))
    return sd


@contextlib.contextmanager
def _stepped_weights(mode, stepped):
    """ko.linear for a weight given as (w, wq): positions where `stepped` [L] holds take wq - un-rounded, the activation rounded
    as the mode rounds it - the others w through the mode's own linear"""
    inner = ko.linear

    def linear(x, w, b=None):
        if not isinstance(w, tuple):
            return inner(x, w, b)
        assert b is None and x.shape[-2] == stepped.numel()
        y = inner(x, w[0])
        yq = (x if mode == "f64" else gs._round(x)) @ w[1].t()
        if mode == "heavy":
            yq = gs._round(yq)
        return torch.where(stepped[:, None], yq, y)

    ko.linear = linear
    try:
        yield
    finally:
        ko.linear = inner


# ------------------------------------------------------------------------------------------------ teacher-forced reference
def row_P(row):
    """prompt positions of a row"""
    if "x" in row:
        return row["P"]
    return len(row["ids"]) + (0 if row.get("prompt") is None else row["prompt"].shape[0])


def _tables(lc, pos):
    inv = ko.llama_inv_freq(lc["head_dim"], lc["rope_theta"], lc.get("rope_scaling"))
    fr = pos.to(torch.float32)[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    return emb.cos()[None, None], emb.sin()[None, None]


@torch.no_grad()
def row_forward(c, W, row, mode="f64", positions=None, allow=None):
    """one row through the decoder and the head.
    row: dict(ids= int64 [nt], prompt= [np, lat] or None, fed= [n, lat]) or dict(x= [L, D] embeddings, P=); step_from (default P):
         first position a decode step computed.
    positions [L] / allow [L, L] bool (query, key): the seeded defects' own rotary positions and mask; default arange / causal.
    Returns dict(pre, hidden [L, D], mean [L - P + 1, lat], kl [L - P + 1] (frame i is position P - 1 + i), P=, L=)."""
    lc = gs.llasa_config(c)["llama"]
    m = ko._sub(W, "base_model.model.")
    P = row_P(row)
    with gs.MODES[mode]():
        if "x" in row:
            x = row["x"].to(F64)
        else:
            lat = row["fed"].to(F64) if row.get("prompt") is None else torch.cat([row["prompt"].to(F64), row["fed"].to(F64)], 0)
            x = torch.cat([m["embed_tokens.weight"][row["ids"]], ko.linear(lat, W["audio_linear.weight"], W["audio_linear.bias"])], 0)
        L = x.shape[0]
        pos = torch.arange(L) if positions is None else positions
        allow = torch.ones(L, L, dtype=torch.bool).tril() if allow is None else allow
        cos, sin = _tables(lc, pos)
        stepped = torch.arange(L) >= row.get("step_from", P)
        x = x[None]
        with _stepped_weights(mode, stepped):
            for i in range(lc["num_hidden_layers"]):
                x = ko.llama_layer(ko._sub(m, f"layers.{i}."), x, cos, sin, allow[None, None], lc["num_attention_heads"],
                                   lc["num_key_value_heads"], lc["rms_norm_eps"])
        hidden = ko.llama_rms_norm(x, m["norm.weight"], lc["rms_norm_eps"])
        h1 = ko.linear(hidden, W["distribution_linear.0.weight"], W["distribution_linear.0.bias"])
        mean = ko.linear(F.gelu(h1), W["distribution_linear.2.weight"], W["distribution_linear.2.bias"])
    mean = mean[0, P - 1:]
    return dict(pre=x[0], hidden=hidden[0], mean=mean, kl=hr.kl(mean, STD), P=P, L=L)


def forward(c, W, rows, mode="f64"):
    return [row_forward(c, W, row, mode) for row in rows]


def defect_forward(c, W, row, kind):
    """the f64 reference of a row with ONE defect of FORWARD_DEFECTS in how the fed-back positions (index >= P) see the cache"""
    P = row_P(row)
    L = (row["x"].shape[0] if "x" in row else P + row["fed"].shape[0])
    pos, allow = torch.arange(L), torch.ones(L, L, dtype=torch.bool).tril()
    fed = torch.arange(L) >= P
    if kind == "position gap 1":
        pos = pos + fed.long()
    elif kind == "newest key masked":
        idx = torch.arange(L)[fed]
        allow[idx, idx] = False
    elif kind == "key 0 masked":
        allow[fed, 0] = False
    elif kind == "key P-1 masked":
        allow[fed, P - 1] = False
    else:
        raise ValueError(kind)
    return row_forward(c, W, row, "f64", pos, allow)


def pick(outs, q):
    return [o[q] for o in outs]


# ------------------------------------------------------------------------------------------------ the check
def ratios(x, x64):
    """[n, d] against the reference [n, d] -> [n]: |x - x64| / max(|x64|, 0.25 rms over the row's positions of |x64|)"""
    assert tuple(x.shape) == tuple(x64.shape), (tuple(x.shape), tuple(x64.shape))
    x, x64 = x.detach().to(F64).cpu(), x64.to(F64)
    nrm = x64.norm(dim=1)
    return (x - x64).norm(dim=1) / torch.maximum(nrm, 0.25 * nrm.pow(2).mean().sqrt())


def worst(xs, x64s):
    """(largest ratio, row, position) over lists of per-row tensors"""
    best = (-1.0, None, None)
    for r, (x, x64) in enumerate(zip(xs, x64s)):
        q = ratios(x, x64)
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        i = int(q.argmax())
        if q[i].item() > best[0]:
            best = (q[i].item(), r, i)
    return best


def yardstick(emu, f64):
    """r per quantity: emu against f64 over every row and position (both lists of row_forward results)"""
    return {q: worst(pick(emu, q), pick(f64, q))[0] for q in QUANTITIES}


def failure(xs, x64s, r, what="", offsets=None, P=None):
    """None when every (row, position) is within M r, else the message: case, row, position / frame, key count, ratio, r.
    offsets[row]: position of xs[row][0] in its sequence (default 0); P[row]: prompt positions (frame = position - P + 1)"""
    v, row, i = worst(xs, x64s)
    if v <= M * r:
        return None
    pos = i + (offsets[row] if offsets else 0)
    frame = "" if P is None else f" frame {pos - P[row] + 1}"
    return f"{what}: row {row} position {pos}{frame} Nk {pos + 1}: ratio {v:.3e} = {v / r:.2f} r > M r (r {r:.3e}, M {M})"


# ------------------------------------------------------------------------------------------------ defects on the outputs
def swap_rows(xs, a, b, T):
    """the last T positions (the frames) of rows a and b swapped"""
    out = [x.clone() for x in xs]
    out[a][-T:], out[b][-T:] = xs[b][-T:].clone(), xs[a][-T:].clone()
    return out


def scale_frame(xs, row, pos, f=1.10):
    out = [x.clone() for x in xs]
    out[row][pos] *= f
    return out


def shift_frames(xs, T):
    """frame i reports frame i + 1 (the last one keeps its own)"""
    out = [x.clone() for x in xs]
    for o, x in zip(out, xs):
        o[-T:-1] = x[-T + 1:]
    return out


# ------------------------------------------------------------------------------------------------ inputs
def scripted_rows(c, Ps, T, tag="gen"):
    """random embedding sequences [P_r + T, D] for the scripted cache drive (unit normal: the size of audio_linear's outputs)"""
    D = c["hd"] * c["H"]
    return [torch.from_numpy(gu.make_input(f"{tag}_x{r}", (P + T, D), c["seed"])) for r, P in enumerate(Ps)]


def ragged_prompts(c, Ps=(1, 14, 250), tag="gen"):
    """(ids, prompt latents [n, lat] or None) of P positions each: ids only below 8 positions, 5 latents below 100, 20 above - P = 1
    is one id, 14 is 9 ids + 5 latents, 250 is 230 ids + 20 latents"""
    out = []
    for r, P in enumerate(Ps):
        nl = 0 if P < 8 else (5 if P < 100 else 20)
        ids = torch.from_numpy(gu.make_input(f"{tag}_ids{r}", (P - nl,), c["seed"])).mul(97).abs().long() % 300
        lat = torch.from_numpy(gu.make_input(f"{tag}_lat{r}", (nl, c["lat"]), c["seed"])) if nl else None
        out.append((ids, lat))
    return out


def many_prompts(c, n=17, tag="many"):
    """n short prompts: 3 + r % 4 ids, every third with two prompt latents (more than one group of infer_batch_rows = 16)"""
    out = []
    for r in range(n):
        ids = torch.from_numpy(gu.make_input(f"{tag}_ids{r}", (3 + r % 4,), c["seed"])).mul(97).abs().long() % 300
        lat = torch.from_numpy(gu.make_input(f"{tag}_lat{r}", (2, c["lat"]), c["seed"])) if r % 3 == 0 else None
        out.append((ids, lat))
    return out


def teacher_rows(prompts, fed, step_from=None):
    """rows of row_forward from prompts [(ids, latents [n, lat] or None)] and the latents fed back per row [n_r, lat]"""
    rows = []
    for r, ((ids, lat), f) in enumerate(zip(prompts, fed)):
        row = dict(ids=ids, prompt=lat, fed=f)
        if step_from is not None:
            row["step_from"] = step_from[r]
        rows.append(row)
    return rows


@torch.no_grad()
def free_run(c, W, prompts, noise, T, mode="emu", step_from=None):
    """autoregressive generation on the oracle: frame i's latent = mean_i + STD noise[i] is fed back.  noise [T, lat] (every row
    the same draw, as the fixed_noise idiom of the host head gives it).  Returns the latents per row [T, lat]."""
    out = []
    for r, (ids, lat) in enumerate(prompts):
        fed = torch.zeros(0, c["lat"], dtype=F64)
        for i in range(T):
            row = teacher_rows([(ids, lat)], [fed], None if step_from is None else [step_from[r]])[0]
            mean = row_forward(c, W, row, mode)["mean"][-1]
            fed = torch.cat([fed, (mean + STD * noise[i].to(F64))[None].float().double()], 0)
        out.append(fed)
    return out


# ------------------------------------------------------------------------------------------------ the stop rule
# the stop-rule tests: the architecture (index into CASES) and the seed of the fixed noise [T, lat], every row the same draw.  Of
# seeds 0 .. 119 on the three architectures this one leaves the widest margin (stop_plan) with rows that stop at different frames
STOP_CASE, STOP_SEED, STOP_FRAMES = 0, 64, 12


def stop_noise(c, frames=STOP_FRAMES, seed=STOP_SEED):
    return torch.randn(1, frames, c["lat"], generator=torch.Generator().manual_seed(seed))[0]


def kl_allowance(mean64, r):
    """the largest change of the frame KL that an error of M r on the mean permits, per position.
    KL = c + |m - 1|^2 / (2 e^2 dl); an error d with |d| <= M r max(|m|, floor) changes |m - 1|^2 by at most 2 |m - 1| |d| + |d|^2
    (Cauchy-Schwarz)"""
    m = mean64.to(F64)
    nrm = m.norm(dim=1)
    d = M * r * torch.maximum(nrm, 0.25 * nrm.pow(2).mean().sqrt())
    return (2 * (m - 1.0).norm(dim=1) * d + d * d) / (2 * math.e ** 2 * m.shape[1])


def stop_plan(kls, allow, first=4):
    """kls, allow: per row [T] (frame KLs in fp64 and their allowances).  The threshold is the midpoint of the widest gap among the
    sorted KLs of frames >= first (the rule stops at i > 3).  Returns dict(thres, half (half-width of the gap), allowance (the
    largest over those frames), counts (frames returned per row: a row that stops at frame i returns i, one that never stops T - 1))"""
    v = torch.cat([k[first:] for k in kls]).sort().values
    gaps = v[1:] - v[:-1]
    i = int(gaps.argmax())
    thres = float((v[i] + v[i + 1]) / 2)
    counts = []
    for k in kls:
        hit = [j for j in range(first, len(k)) if k[j].item() < thres]
        counts.append(hit[0] if hit else len(k) - 1)
    al = torch.cat([a[first:] for a in allow])
    margin = float(((torch.cat([k[first:] for k in kls]) - thres).abs() / al).min())
    return dict(thres=thres, half=float(gaps[i]) / 2, allowance=float(al.max()), margin=margin, counts=counts)
