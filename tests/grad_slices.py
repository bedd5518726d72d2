"""Localised gradient check: every gradient tensor is cut into small slices and each slice is held to an fp64 run of the
oracle, with a yardstick that comes from the reference alone.  Pure torch on the CPU; shared by tests/test_grad_slices_cpu.py
(the yardstick and the seeded defects on the reference itself) and tests/test_grad_slices_gpu.py (the HIP path).

Slices     a tensor is viewed as [shape[0], -1] (a vector as [n, 1]) and cut into runs of 16 consecutive rows; a fused parameter
           is cut at its chunk boundaries first (q | k | v, k | v, the six adaLN chunks, value | gate, heads), so no slice straddles
           two chunks; activations and input gradients are viewed as [tokens, D] and cut per token row.
Scale      of a slice: max(|g_slice|, 0.25 |g| sqrt(numel_slice / numel)), g the fp64 reference - the floor gives an unusually
           quiet slice a unit; no slice is excluded.
Yardstick  r(p) = the largest |g_emu - g64|_slice / scale over p's slices, where g_emu is the fp64 oracle run again with both
           operands of every ko.linear rounded to bf16 (fp64 carrier) and with the roundings of the attention kernels (q, k, v
           and their gradients, P and dS in bf16: emulate()); floored at the model-wide median of r.
Assertion  |g - g64|_slice <= M r(p) scale for every slice, M = 3: a heavier emulation (every linear output and every gradient
           that passes through a linear rounded to bf16 as well - about twice the rounding points) reaches 2.0 r(p) on the CPU
           (median 1.0-1.2; tests/test_grad_slices_cpu.py holds it to M on every case), which leaves the HIP path room for its
           own points (bf16 activations between kernels, fast-math).
Reach      a slice whose own norm is above the floor and that is wrong by a fraction f is reported when f > M r(p): 2-4 % for most
           parameters (r(p) at the median), up to 10 % where r(p) is 3.5e-2.  A slice below the floor needs a larger fraction in
           proportion.  tests/test_grad_slices_cpu.py asserts M r < 0.10 for the token rows of every input gradient, so one token
           row x 1.10 is reported in every row that is not below the floor."""
import contextlib
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import golden_util as gu  # noqa: E402
import kalle_oracle as ko  # noqa: E402

RUN = 16        # rows of a parameter slice
M = 3.0         # allowed multiple of the yardstick
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ slices and norms
def bounds(rows, run=RUN, chunk=None):
    """[(r0, r1)]: runs of `run` consecutive rows that never cross a multiple of `chunk` rows (the last run of a chunk is short)"""
    chunk = rows if not chunk else chunk
    return [(r, min(r + run, c + chunk, rows)) for c in range(0, rows, chunk) for r in range(c, min(c + chunk, rows), run)]


def view2d(t):
    return t.reshape(t.shape[0], -1) if t.dim() >= 2 else t.reshape(-1, 1)


def dit_chunk(name, shape, dim_heads):
    """rows per chunk of a fused DiT parameter (None: not fused).  Head boundaries subsume q | k | v and k | v."""
    if name.endswith(("self_attn.to_qkv.weight", "cross_attn.to_kv.weight", "cross_attn.to_q.weight")):
        return dim_heads
    if "to_scale_shift_gate" in name:
        return shape[0] // 6
    if name.endswith(("ff.ff.0.proj.weight", "ff.ff.0.proj.bias", "glu.proj.weight", "glu.proj.bias")):
        return shape[0] // 2
    return None


def llama_chunk(name, shape, head_dim):
    """under the reference's (HF) names q | k | v and gate | up are tensors of their own; what is left are the heads"""
    return head_dim if name.endswith(("q_proj.weight", "k_proj.weight", "v_proj.weight")) else None


def make_layout(g64, chunk_of):
    """name -> [(r0, r1)] for a dict of reference tensors; names that start with "act:" are [tokens, D] and cut per row"""
    return {n: bounds(view2d(t).shape[0], 1) if n.startswith("act:") else bounds(view2d(t).shape[0], RUN, chunk_of(n, t.shape))
            for n, t in g64.items()}


def _slice_sq(t2d, bnds):
    cs = torch.cat([torch.zeros(1, dtype=F64), (t2d.to(F64) ** 2).sum(1).cumsum(0)])
    a = torch.tensor([b[0] for b in bnds])
    b = torch.tensor([b[1] for b in bnds])
    return (cs[b] - cs[a]).clamp_min(0.0), (b - a) * t2d.shape[1]


def unit_norm(g64, name):
    """|g| of the scale's floor.  ONE family of gradients has no unit of its own: the bias of the k LayerNorm of a cross-attention
    (qk_norm="ln").  Without a rotary embedding a vector added to every key shifts all scores of a query by the same amount, the
    softmax does not move, and the gradient is exactly zero - the fp64 reference holds 1e-17 of cancellation noise.  Its unit is
    the norm of the gradient of that LayerNorm's weight: the same per-key terms dk summed over the same keys, there weighted by
    normalised activations of unit RMS (no cancellation), so it is the size a bias gradient of these terms has."""
    own = g64[name].to(F64).norm()
    if name.endswith("cross_attn.k_norm.bias"):
        own = torch.maximum(own, g64[name[:-len("bias")] + "weight"].to(F64).norm())
    return own


def slice_scale(ref, bnds, unit=None):
    r2 = view2d(ref)
    sq, numel = _slice_sq(r2, bnds)
    unit = r2.to(F64).norm() if unit is None else unit
    return torch.maximum(sq.sqrt(), 0.25 * unit * (numel.to(F64) / r2.numel()).sqrt())


def slice_ratio(g, ref, bnds, unit=None):
    """|g - ref|_slice / scale per slice (0 where a whole tensor and its error vanish)"""
    assert tuple(g.shape) == tuple(ref.shape), (tuple(g.shape), tuple(ref.shape))
    err = _slice_sq(view2d(g).to(F64) - view2d(ref).to(F64), bnds)[0].sqrt()
    sc = slice_scale(ref, bnds, unit)
    return torch.where(sc > 0, err / sc.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))


def yardstick(g_emu, g64, layout):
    """r(p) per name, floored at the median over the PARAMETERS (the activations take the same floor); also the raw values"""
    raw = {n: slice_ratio(g_emu[n], g64[n], layout[n], unit_norm(g64, n)).max().item() for n in layout}
    med = statistics.median(v for n, v in raw.items() if not n.startswith("act:"))
    return {n: max(v, med) for n, v in raw.items()}, raw


def check(g, g64, r, layout, names=None):
    """rho per name: (the worst |g - g64|_slice / (r(p) scale), its rows).  The caller asserts rho <= M (see failures())."""
    rho = {}
    for n in (names if names is not None else layout):
        q = slice_ratio(g[n], g64[n], layout[n], unit_norm(g64, n)) / r[n]
        i = int(q.argmax())
        rho[n] = (q[i].item(), layout[n][i])
    return rho


def failures(rho, m=M):
    return sorted(((n, round(v, 2), rows) for n, (v, rows) in rho.items() if not v <= m), key=lambda f: -f[1])


def worst(rho):
    n = max(rho, key=lambda k: rho[k][0])
    return n, rho[n][0], rho[n][1]


def rel_l2(a, b):
    return ((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ bf16 emulations of ko.linear
def _round(x):
    return x.detach().to(torch.bfloat16).to(x.dtype)


def _st(x):
    """x rounded to bf16 on the carrier dtype, gradient passed straight through (r - x is exact, so the sum is r itself)"""
    return x + (_round(x) - x.detach())


class _RoundBoth(torch.autograd.Function):
    """rounds the value on the way forward and the gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return _round(x)

    @staticmethod
    def backward(ctx, g):
        return _round(g)


class _RoundGrad(torch.autograd.Function):
    """identity on the way forward, rounds the gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _round(g)


@contextlib.contextmanager
def emulate(heavy=False):
    """ko.linear with both operands rounded to bf16; heavy: its output, and the gradients of its input and output, as well.
    Both also carry the rounding points of the attention kernels (DESIGN.md "Gradients per slice"): q, k, v and their gradients are bf16 tensors (dit_ops: qkv / qn / kn and dqkv / dqn / dkn), and the backward kernel feeds P and
    dS to its MFMAs in bf16 (attention.hip, pack_pair before dK^T += Q^T dS).  Without them the emulation keeps exact a
    cancellation the kernels cannot keep: a vector added to every key moves no softmax, so the gradient of a k-LayerNorm bias is
    zero wherever no rotary embedding acts (dims 32-63 of a self-attention head) - in bf16 the sum over the keys of dS, and of
    the rounded dk, leaves rounding noise there, which is what the yardstick has to measure."""
    orig = ko.linear, ko._attn_operands, ko._softmax

    def linear(x, w, b=None):
        if heavy:
            y = _RoundBoth.apply(x) @ _st(w).t()
            return _RoundBoth.apply(y + b if b is not None else y)
        y = _st(x) @ _st(w).t()
        return y + b if b is not None else y

    ko.linear = linear
    ko._attn_operands = lambda q, k, v: tuple(_RoundBoth.apply(t) for t in (q, k, v))
    ko._softmax = lambda dots: _st(_RoundGrad.apply(dots).softmax(-1))
    try:
        yield
    finally:
        ko.linear, ko._attn_operands, ko._softmax = orig


@contextlib.contextmanager
def capture_rows(bias):
    """box["dy"]: the gradient of the output of the linear whose bias IS `bias`, per row - row t is token t's contribution to the
    bias gradient"""
    orig, box = ko.linear, {}

    def linear(x, w, b=None):
        y = orig(x, w, b)
        if b is bias:
            box["dy"] = torch.zeros_like(y, requires_grad=True)
            y = y + box["dy"]
        return y

    ko.linear = linear
    try:
        yield box
    finally:
        ko.linear = orig


MODES = {"f64": contextlib.nullcontext, "emu": emulate, "heavy": lambda: emulate(heavy=True)}


# ------------------------------------------------------------------------------------------------ DiT cases and reference
# 64 latent channels, the narrowest width of the reference's configurations (64 / 512 / 1024): the gradient of x_t is checked per
# token row, and the worst of several hundred rows of only 16 numbers sets an r of 3e-2 ... 4e-2, above what a row x 1.10 can show
CIO, GD, DEPTH = 64, 32, 3


def _dit(seed, D, heads, kv, gtype, T, S, B, **kw):
    """kv: kv heads of the cross-attention (context width 64 kv, not projected; kv < heads is GQA), 0: project_cond_tokens"""
    c = dict(seed=seed, D=D, heads=heads, kv=kv, gtype=gtype, T=T, S=S, B=B, obj="v", pad=False, cmask=False, qk="none",
             conformer=False, causal=False)
    c.update(kw)
    c["id"] = f"s{seed}-D{D}-{gtype}-T{T}-S{S}-B{B}" + "".join(f"-{k}" for k in ("pad", "cmask", "conformer", "causal") if c[k]) + \
        (f"-qk{c['qk']}" if c["qk"] != "none" else "") + (f"-kv{kv}" if kv else "-proj")
    return c


# T in {33, 125, 257}, S in {7, 130, 200} (one to three key blocks, the folded tail), B in {2, 3}, both conditioning types, the loss
# mask and the context mask on and off, both qk norms, a conformer block, GQA cross-attention, one causal case (S >= N: every
# query sees a key)
DIT_CASES = [
    _dit(701, 128, 2, 2, "prepend", 33, 7, 2),
    _dit(702, 128, 2, 1, "adaLN", 125, 130, 3, pad=True, cmask=True, obj="rectified_flow"),
    _dit(703, 192, 3, 1, "prepend", 257, 200, 2, pad=True),
    _dit(704, 128, 2, 2, "prepend", 125, 7, 2, qk="ln", cmask=True),
    _dit(705, 128, 2, 2, "adaLN", 33, 130, 3, qk="l2"),
    _dit(706, 128, 2, 1, "prepend", 125, 200, 2, conformer=True),
    _dit(707, 128, 2, 2, "adaLN", 33, 200, 2, causal=True, pad=True),
    _dit(708, 192, 3, 0, "adaLN", 257, 7, 2, obj="rectified_flow"),
]


def dit_dims(c):
    dc = 64 * c["kv"] if c["kv"] else 48
    return dc, c["D"] // c["heads"]


def dit_shapes(c, depth=DEPTH):
    dc, dh = dit_dims(c)
    return ko.dit_shapes(CIO, c["D"], depth, cond_token_dim=dc, global_cond_dim=GD, global_cond_type=c["gtype"],
                         project_cond_tokens=not c["kv"], dim_heads=dh, qk_ln=c["qk"] == "ln", conformer=c["conformer"])


def dit_module_kwargs(c, depth=DEPTH):
    """constructor arguments of the drop-in DiffusionTransformer for the case"""
    dc, _ = dit_dims(c)
    kw = dict(io_channels=CIO, embed_dim=c["D"], depth=depth, num_heads=c["heads"], cond_token_dim=dc,
              project_cond_tokens=not c["kv"], global_cond_dim=GD, transformer_type="continuous_transformer",
              global_cond_type=c["gtype"])
    if c["qk"] != "none":
        kw["attn_kwargs"] = dict(qk_norm=c["qk"])
    if c["conformer"]:
        kw["conformer"] = True
    if c["causal"]:
        kw["causal"] = True
    return kw


def dit_inputs(c, seed=None, B=None):
    """fp32 inputs of one (micro-)batch, built like the configuration fuzz builds them"""
    seed = c["seed"] if seed is None else seed
    B = c["B"] if B is None else B
    dc, _ = dit_dims(c)
    T, S = c["T"], c["S"]
    mk = lambda n, shape: torch.from_numpy(gu.make_input(n, shape, seed))
    return dict(lat=mk("lat", (B, CIO, T)), noise=mk("noise", (B, CIO, T)), t=torch.linspace(0.08, 0.93, B),
                ctx=mk("ctx", (B, S, dc)), gl=mk("glob", (B, GD)),
                pm=torch.from_numpy(gu.make_mask("pm", (B, T), seed, 0.8)) if c["pad"] else None,
                cm=torch.from_numpy(gu.make_mask("cm", (B, S), seed, 0.7)) if c["cmask"] else None)


def rows_bct(x):
    """[B, C, T] -> [B T, C]: one row per token"""
    return x.transpose(1, 2).reshape(-1, x.shape[1])


def dit_reference(c, st, inp, mode="f64", dtype=F64, depth=DEPTH, bias_rows=None):
    """one train step of the oracle (diffuse -> DiT -> masked MSE) on the state `st` (name -> numpy fp32) in `dtype`.
    Returns {name: gradient} for every parameter the loss reaches, plus "act:out", "act:d_xt", "act:d_ctx", "act:d_glob"
    (one row per token / clip) and "loss".  bias_rows: a parameter name - also "rows:<name>", the per-token contributions to that
    bias gradient [tokens, n]."""
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in st.items()}
    fl = lambda k: inp[k].to(dtype)
    cfg = dict(embed_dim=c["D"], depth=depth, num_heads=c["heads"], global_cond_type=c["gtype"], causal=c["causal"],
               qk_l2=c["qk"] == "l2")
    xt, target = ko.diffuse(fl("lat"), fl("noise"), fl("t"), c["obj"])
    xt, ctx, gl = (v.detach().requires_grad_(True) for v in (xt, fl("ctx"), fl("gl")))
    cap = capture_rows(sd[bias_rows]) if bias_rows else contextlib.nullcontext()
    with MODES[mode](), cap as box:
        out = ko.dit_forward(sd, cfg, xt, fl("t"), cross_attn_cond=ctx, cross_attn_cond_mask=inp["cm"], global_embed=gl)
        loss = ko.mse_loss(out, target, inp["pm"])
        loss.backward()
    g = {k: v.grad for k, v in sd.items() if v.grad is not None}
    g.update({"act:out": rows_bct(out.detach()), "act:d_xt": rows_bct(xt.grad), "act:d_ctx": ctx.grad.flatten(0, 1),
              "act:d_glob": gl.grad, "loss": loss.detach()})
    if bias_rows:
        g["rows:" + bias_rows] = box["dy"].grad.reshape(-1, box["dy"].shape[-1])
    return g


def dit_window(c, st, seeds, mode="f64", dtype=F64, bias_rows=None):
    """dit_reference summed over the micro-batches built from `seeds` - what the trainer's flat gradient holds at the end of an
    accumulation window (1 / accum is folded into the Adam step).  One seed: the activations and the loss as well."""
    runs = [dit_reference(c, st, dit_inputs(c, s), mode, dtype, bias_rows=bias_rows) for s in seeds]
    if len(runs) == 1:
        return runs[0]
    return {k: sum(g[k] for g in runs) for k in runs[0] if k in st}


def dit_layout(c, g64):
    _, dh = dit_dims(c)
    return make_layout({n: t for n, t in g64.items() if n != "loss" and not n.startswith("rows:")},
                       lambda n, shape: dit_chunk(n, shape, dh))


# trainer: accumulation windows of 1 and 2 micro-batches, row counts (B tokens) that are a multiple of 8 (the grouped launch writes
# the flat gradient in place) and that are not (one GEMM each), the grouped launch switched off once; every case runs two
# consecutive windows on different data
TRAINER_CASES = [
    dict(base=_dit(711, 128, 2, 2, "prepend", 33, 7, 2), accum=1, group=True),                       # 68 rows
    dict(base=_dit(712, 128, 2, 1, "prepend", 125, 130, 4, pad=True), accum=2, group=True),          # 504 rows
    dict(base=_dit(713, 128, 2, 2, "adaLN", 64, 130, 3), accum=2, group=True),                       # 192 rows
    dict(base=_dit(714, 128, 2, 1, "prepend", 125, 7, 4), accum=1, group=False),                     # 504 rows, one GEMM each
    dict(base=_dit(715, 192, 3, 1, "adaLN", 33, 200, 3, cmask=True), accum=2, group=True),           # 99 rows
]
for _c in TRAINER_CASES:
    _c["id"] = _c["base"]["id"] + f"-accum{_c['accum']}" + ("" if _c["group"] else "-nogroup")


def window_seeds(tc, window):
    """seeds of the micro-batches of accumulation window `window` (0, 1)"""
    return [tc["base"]["seed"] + 10 * (window * tc["accum"] + i) for i in range(tc["accum"])]


# partially frozen models (the usual fine-tuning set-up): name -> is the parameter frozen
FROZEN_SETS = {
    "self_attn": lambda n: ".self_attn." in n,
    "ff_bias": lambda n: n.endswith(("ff.ff.0.proj.bias", "ff.ff.2.bias")),
    "first_block": lambda n: n.startswith("transformer.layers.0."),
    "last_block": lambda n: n.startswith(f"transformer.layers.{DEPTH - 1}."),
    "all_but_cross_attn": lambda n: ".cross_attn." not in n,
    "cond_embedders": lambda n: n.startswith(("to_cond_embed.", "to_global_embed.")),
}
# 128 rows per micro-batch (the grouped launch's overwrite rule applies).  inputs_grad False: additionally the context and the
# global conditioning do not require grad - with their embedders frozen the transformer sees a conditioning without gradient
FROZEN_CASES = [
    dict(base=_dit(721, 128, 2, 2, "adaLN", 64, 7, 2), frozen="self_attn", inputs_grad=True),
    # (prepend: only there the LayerNorm backward of block i + 1 fuses the FF-out bias column sum of block i - with every FF bias
    # frozen the sink it would add into is missing, with the last block frozen the block above has no sinks at all)
    dict(base=_dit(722, 128, 2, 1, "prepend", 63, 130, 2), frozen="ff_bias", inputs_grad=True),
    dict(base=_dit(723, 128, 2, 2, "adaLN", 64, 7, 2), frozen="first_block", inputs_grad=True),
    dict(base=_dit(724, 128, 2, 1, "prepend", 63, 130, 2), frozen="last_block", inputs_grad=True),
    dict(base=_dit(725, 128, 2, 1, "prepend", 63, 130, 2), frozen="all_but_cross_attn", inputs_grad=True),
    dict(base=_dit(726, 128, 2, 2, "adaLN", 64, 7, 2), frozen="cond_embedders", inputs_grad=False),
]
for _c in FROZEN_CASES:
    _c["id"] = _c["base"]["id"] + "-frozen-" + _c["frozen"]


# ------------------------------------------------------------------------------------------------ Llasa cases and reference
def _llasa(seed, H, Hkv, hd, inter, lat, B, L, scaling):
    return dict(seed=seed, H=H, Hkv=Hkv, hd=hd, layers=2, inter=inter, lat=lat, B=B, L=L, scaling=scaling,
                id=f"s{seed}-H{H}k{Hkv}-hd{hd}-I{inter}-B{B}-n{L}" + ("-llama3" if scaling else ""))


# 4 / 2 and 6 / 3 heads, two layers, MLP widths that are no multiple of 128, ragged lengths 24 ... 257, with and without llama3
# rope scaling, one head-dim-128 case
LLASA_CASES = [
    _llasa(801, 4, 2, 64, 192, 16, 2, 257, True),
    _llasa(802, 6, 3, 64, 448, 8, 3, 24, False),
    _llasa(803, 2, 1, 128, 192, 16, 2, 130, True),
]


def llasa_config(c):
    hid = c["hd"] * c["H"]
    llama = dict(vocab_size=300, hidden_size=hid, intermediate_size=c["inter"], num_hidden_layers=c["layers"],
                 num_attention_heads=c["H"], num_key_value_heads=c["Hkv"], head_dim=c["hd"], rms_norm_eps=1e-5,
                 rope_theta=500000.0, max_position_embeddings=1024, tie_word_embeddings=True, attention_bias=False,
                 mlp_bias=False, hidden_act="silu")
    if c["scaling"]:
        llama["rope_scaling"] = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                     original_max_position_embeddings=64)
    return dict(latent_dim=c["lat"], tokenizer_len=310, llama=llama)


def llasa_shapes(c):
    """the reference's (HF) names: the drop-in fuses q | k | v and gate | up at load time"""
    hid, lat, I, H, Hkv, hd = c["hd"] * c["H"], c["lat"], c["inter"], c["H"], c["Hkv"], c["hd"]
    names = [("audio_linear.bias", (hid,)), ("audio_linear.weight", (hid, lat)), ("base_model.model.embed_tokens.weight", (310, hid)),
             ("base_model.model.norm.weight", (hid,)), ("distribution_linear.0.bias", (lat,)), ("distribution_linear.0.weight", (lat, hid)),
             ("distribution_linear.2.bias", (lat,)), ("distribution_linear.2.weight", (lat, lat))]
    for i in range(c["layers"]):
        pre = f"base_model.model.layers.{i}."
        names += [(pre + "input_layernorm.weight", (hid,)), (pre + "post_attention_layernorm.weight", (hid,)),
                  (pre + "mlp.down_proj.weight", (hid, I)), (pre + "mlp.gate_proj.weight", (I, hid)), (pre + "mlp.up_proj.weight", (I, hid)),
                  (pre + "self_attn.q_proj.weight", (H * hd, hid)), (pre + "self_attn.k_proj.weight", (Hkv * hd, hid)),
                  (pre + "self_attn.v_proj.weight", (Hkv * hd, hid)), (pre + "self_attn.o_proj.weight", (hid, H * hd))]
    return names


def llasa_inputs(c, seed=None):
    """(batch as numpy arrays, sampling noise as numpy); seed: another micro-batch of the same shape (other ragged lengths)"""
    seed = c["seed"] if seed is None else seed
    lc = llasa_config(c)
    b = gu.llasa_batch_long(lc, seed, B=c["B"], L=c["L"])
    return b, gu.make_input("llasa_eps", tuple(b["audio_latents"].shape), seed)


def llasa_window(c, st, seeds, mode="f64", dtype=F64):
    """llasa_reference summed over the micro-batches built from `seeds`: the parameter gradients the trainer's flat buffer holds
    at the end of an accumulation window"""
    runs = [llasa_reference(c, st, *llasa_inputs(c, s), mode, dtype) for s in seeds]
    return {k: sum(g[k] for g in runs) for k in runs[0] if k in st}


def llasa_reference(c, st, batch, eps, mode="f64", dtype=F64, bias_rows=None):
    """audio_loss + 0.5 end_loss of ko.llasa_forward in `dtype`: {HF name: gradient}, "act:pre_mean" (the valid positions, one
    row each), "audio_loss", "end_loss" (and "rows:<bias>", see dit_reference)"""
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in st.items()}
    b = {k: torch.from_numpy(v) for k, v in batch.items()}
    b = {k: v.to(dtype) if v.is_floating_point() else v for k, v in b.items()}
    cap = capture_rows(sd[bias_rows]) if bias_rows else contextlib.nullcontext()
    with MODES[mode](), cap as box:
        out = ko.llasa_forward(sd, llasa_config(c), b, torch.from_numpy(eps).to(dtype))
        (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    valid = (b["ids_mask"] + b["audio_mask"]) > 0
    g = {k: v.grad for k, v in sd.items() if v.grad is not None}
    g.update({"act:pre_mean": out["pre_mean"].detach()[valid], "audio_loss": out["audio_loss"].detach(),
              "end_loss": out["end_loss"].detach()})
    if bias_rows:
        g["rows:" + bias_rows] = box["dy"].grad.reshape(-1, box["dy"].shape[-1])
    return g


def llasa_layout(c, g64):
    return make_layout({n: t for n, t in g64.items() if not n.endswith("_loss") and not n.startswith("rows:")},
                       lambda n, shape: llama_chunk(n, shape, c["hd"]))


# ------------------------------------------------------------------------------------------------ seeded defects
def _with(g, name, fn):
    out = dict(g)
    t = g[name].detach().clone()
    fn(view2d(t))
    out[name] = t
    return out


def _scale_rows(rows, f):
    def fn(t):
        t[rows[0]:rows[1]] *= f
    return fn


def _swap_rows(a, b, n):
    def fn(t):
        t[a:a + n], t[b:b + n] = t[b:b + n].clone(), t[a:a + n].clone()
    return fn


def seeded_defects(g, layout, where, rows_of_bias):
    """[(label, name, g with ONE defect in `name`)] - the defects a whole-tensor norm cannot see.
    where: dict(slice=, tail=, token= (name or names), qkv=(name, rows per head), bias=, adaln= (name or None)); rows_of_bias:
    [tokens, n] contributions to g[where["bias"]] - the row with the LARGEST contribution is the one left out; None: a window of
    several micro-batches, whose reference keeps no per-token rows (no bias defect)"""
    out = []
    n = where["slice"]
    out.append(("one 16-row slice x 1.10", n, _with(g, n, _scale_rows(layout[n][len(layout[n]) // 2], 1.10))))
    n = where["tail"]
    out.append(("tail slice x 0.93", n, _with(g, n, _scale_rows(layout[n][-1], 0.93))))
    for n in ([where["token"]] if isinstance(where["token"], str) else where["token"]):
        if n in g:
            out.append(("one token row x 1.10", n, _with(g, n, _scale_rows(layout[n][len(layout[n]) // 2], 1.10))))
    if where.get("adaln"):
        n = where["adaln"]
        k = view2d(g[n]).shape[0] // 6
        out.append(("one adaLN chunk zeroed", n, _with(g, n, _scale_rows((2 * k, 3 * k), 0.0))))
    n, dh = where["qkv"]
    out.append(("one head's rows swapped with the next head's", n, _with(g, n, _swap_rows(0, dh, dh))))
    if rows_of_bias is None:
        return out
    n = where["bias"]
    tok = int(rows_of_bias.to(F64).norm(dim=1).argmax())

    def drop(t, tok=tok):
        t -= rows_of_bias[tok].to(t.dtype).reshape(t.shape)
    out.append(("bias gradient without one token's contribution", n, _with(g, n, drop)))
    return out


def dit_defect_sites(c, depth=DEPTH, token=("act:d_xt", "act:d_ctx")):
    """token: the gradient of x_t (the dx of the model) and that of the context, where they exist.
    bias: a bias gradient is a column sum over n rows and one row left out changes it by about |g| / sqrt(n); against
    M r(p) ~ 3.5e-2 that shows up to n ~ 100 rows and is inside the rounding noise of a 16-element slice beyond.  So the FF-out bias
    of the last block carries the defect where the batch has at most 100 tokens (the row with the largest contribution is left
    out; an arbitrary row is reported for 50 of 66 ... 66 of 68 rows), and the bias of the timestep embedding, where
    a row is a whole clip, elsewhere."""
    last, mid = f"transformer.layers.{depth - 1}.", f"transformer.layers.{depth // 2}."
    tokens = c["B"] * (c["T"] + (c["gtype"] == "prepend"))
    return dict(slice=mid + "ff.ff.0.proj.weight", tail=last + "self_attn.to_out.weight", token=token,
                qkv=(mid + "self_attn.to_qkv.weight", dit_dims(c)[1]),
                bias=last + "ff.ff.2.bias" if tokens <= 100 else "to_timestep_embed.2.bias",
                adaln=mid + "to_scale_shift_gate.1.weight" if c["gtype"] == "adaLN" else None)


def llasa_defect_sites(c):
    l0, l1 = "base_model.model.layers.0.", "base_model.model.layers.1."
    return dict(slice=l0 + "mlp.down_proj.weight", tail=l1 + "self_attn.o_proj.weight", token="act:pre_mean",
                qkv=(l0 + "self_attn.q_proj.weight", c["hd"]), bias="distribution_linear.0.bias", adaln=None)


def old_rule_passes(g, g64, name):
    """the whole-tensor rule of the configuration fuzz tests: |g - g64| <= 4e-2 |g64|"""
    return (g[name].to(F64) - g64[name].to(F64)).norm().item() <= 4e-2 * g64[name].to(F64).norm().item()
