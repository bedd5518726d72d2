"""Guided DiT sampling held to an fp64 oracle, step by step.  Pure torch on the CPU; shared by tests/test_sample_oracle_cpu.py (the
yardstick, the seeded defects and the blind pairs, on the reference itself) and tests/test_sampling_oracle_gpu.py
(generate_diffusion_cond, sample_rf and DiffusionTransformer.forward on the HIP path).

State      gu.make_state(dit_shapes(case), seed of the base case): the fixture state of the gradient checks, unchanged.  It shows
           every defect below in a prepend and in an adaLN case; what it cannot show is listed in BLIND, pair by pair.
Reference  teacher forced: for a recorded step (x_i, t_i) the guided model output in fp64 ON EXACTLY THOSE INPUTS, as token rows
           [B T, C] (outputs), and the fp64 sampler update computed from (x_i, out_i) (update).  free_run: the fp64 trajectory of
           the case from its seeded noise through ko.sample_ddim / ko.sample_euler themselves - x_i, t_i, out_i, the final latents.
           guided() restates ko.dit_forward's guidance arithmetic with seams for the defects; without a defect it IS ko.dit_forward,
           bit for bit (asserted on the CPU).
Modes      f64 (the reference) and emu: grad_slices.emulate, the bf16-operand emulation of the gradient checks.  No rounding point
           was added for the sampling path: the frozen, hoisted, replayed forward rounds where the training forward rounds.
Check      per step and token row: |out - out64|_row / max(|out64|_row, 0.25 rms over the rows of |out64|_row), the unit of
           gen_oracle.py.  Yardstick r(case, step) = the largest such ratio of emu against f64 ON THE fp64 FREE-RUNNING TRAJECTORY:
           from the reference alone.  Assertion: ratio <= M r(case, step), M = grad_slices.M = 3, at every row of every step.
           Schedule: the recorded t_i are the fp32 values of the sampler's own linspace.  Update: x_{i+1} and the returned tensor
           against the fp64 update of the recorded (x_i, out_i), element-wise, inside the rounding of the formula's fp32 operations
           (update()).
Defects    seeded into the REFERENCE, one at a time: in the guidance mix (halves swapped, cfg_scale - 1, scale x 1.10), in what the
           unconditional half sees (negative prompt ignored, its mask ignored, global embedding zeroed), in the layout (to_kv of
           layers 0 and 1 exchanged - a mis-sliced stacked k | v -, the doubled batch interleaved but split as halves, the
           prepended token not skipped), in the schedule (the timestep of the next step fed to the model), and in the update
           (alpha, sigma of step i in the update of step i + 1; dt with the wrong sign)."""
import contextlib
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_oracle as go  # noqa: E402
import grad_slices as gs  # noqa: E402

gu, ko = gs.gu, gs.ko
F64, M = torch.float64, gs.M
U = 2.0 ** -24            # unit roundoff of fp32
ratios = go.ratios        # the unit of the check
_BASE = {c["seed"]: c for c in gs.DIT_CASES}
PREPEND_TOKENS, PREPEND_DIM = 3, 24


def _case(id, base, B, obj, cfg, steps, path, **kw):
    assert not _BASE[base]["causal"]
    k = dict(id=id, base=base, B=B, obj=obj, cfg=cfg, steps=steps, path=path, neg=False, trainable=False, sigma_max=1.0,
             init=False, phi=0.0, prepend=False)
    k.update(kw)
    return k


# the smallest shapes at which this path can still go wrong: one, two and three key blocks with the folded tail, 2B of 2, 4 and 6, both
# conditioning types.  path: (graph replay, conditioning hoisted out of the loop) as generate_diffusion_cond must choose them
CASES = [
    _case("G1", 701, 2, "v", 3.0, 4, (True, True)),
    _case("G2", 702, 3, "rectified_flow", 2.0, 4, (True, True), neg=True),
    _case("G3", 703, 1, "v", 6.0, 5, (True, True)),
    _case("G4", 708, 2, "rectified_flow", 1.0, 4, (True, True)),                      # unguided: no batch doubling
    _case("G5", 704, 2, "v", 3.0, 4, (True, False)),                                  # qk-LayerNorm: precompute_conditioning gives {}
    _case("G6", 706, 2, "rectified_flow", 3.5, 4, (False, False), trainable=True),    # sampling during training
    _case("G7", 702, 2, "rectified_flow", 3.0, 4, (False, False), init=True, sigma_max=0.6),   # sample_rf called directly
]
# one forward, no sampler: the rescale branch of _guided (generate_diffusion_cond never reaches it) and a prepended conditioning with
# its mask (SpliceFn, _with_unconditional(prepend_cond))
SINGLE = [
    _case("S1", 701, 2, "v", 3.0, 0, None, phi=0.5),
    _case("S2", 702, 3, "rectified_flow", 3.0, 0, None, phi=0.5),
    _case("S3", 701, 2, "v", 3.0, 0, None, prepend=True),
    _case("S4", 705, 3, "v", 3.0, 0, None, prepend=True),
]
BY_ID = {k["id"]: k for k in CASES + SINGLE}

MODEL_DEFECTS = ("halves swapped", "cfg_scale - 1", "scale x 1.10", "negative prompt ignored", "negative mask ignored",
                 "global zeroed in the unconditional half", "to_kv of layers 0 and 1 exchanged", "interleaved batch split as halves",
                 "prepended token not skipped", "timestep of the next step")
UPDATE_DEFECTS = ("alpha, sigma of the step before", "dt with the wrong sign")
DEFECTS = MODEL_DEFECTS + UPDATE_DEFECTS

# the (case, defect) pairs the state cannot show: the defective reference stays within M r of the reference at every row of every
# step (tests/test_sample_oracle_cpu.py asserts each of them blind, and the largest ratio in units of M r is in DESIGN.md,
# "Sampling per step").  Never extended to make a device test pass.
BLIND = frozenset({
    ("G3", "timestep of the next step"),                      # T 257, prepend: one token among 258 carries the timestep
    ("G5", "timestep of the next step"),
    ("G5", "global zeroed in the unconditional half"),        # T 125, prepend, qk-LayerNorm
})


def base(k):
    return _BASE[k["base"]]


def is_prepend(k):
    return base(k)["gtype"] == "prepend"


def applies(k, defect):
    guided_ = k["cfg"] != 1.0
    if defect in ("halves swapped", "cfg_scale - 1", "scale x 1.10", "global zeroed in the unconditional half"):
        return guided_
    if defect in ("negative prompt ignored", "negative mask ignored"):
        return guided_ and k["neg"]
    if defect == "interleaved batch split as halves":
        return guided_ and k["B"] > 1
    if defect == "prepended token not skipped":
        return is_prepend(k)
    if defect == "timestep of the next step":
        return k["steps"] > 0
    if defect == "alpha, sigma of the step before":
        return k["steps"] > 0 and k["obj"] == "v"
    if defect == "dt with the wrong sign":
        return k["steps"] > 0 and k["obj"] == "rectified_flow"
    return defect == "to_kv of layers 0 and 1 exchanged"


def tokens(k):
    """token rows per clip of the output.  With global_cond_type="adaLN" a prepended conditioning is NOT cut off again: the reference
    sets prepend_length only in its "prepend" branch (dit.py:183-195), the oracle and the drop-in follow it"""
    return base(k)["T"] + (PREPEND_TOKENS if k["prepend"] and not is_prepend(k) else 0)


def defects_of(k, kind=DEFECTS):
    return [d for d in kind if applies(k, d)]


# ------------------------------------------------------------------------------------------------ state and inputs
def shapes(k):
    c = base(k)
    if not k["prepend"]:
        return gs.dit_shapes(c)
    dc, dh = gs.dit_dims(c)
    return ko.dit_shapes(gs.CIO, c["D"], gs.DEPTH, cond_token_dim=dc, global_cond_dim=gs.GD, prepend_cond_dim=PREPEND_DIM,
                         global_cond_type=c["gtype"], project_cond_tokens=not c["kv"], dim_heads=dh, qk_ln=c["qk"] == "ln",
                         conformer=c["conformer"])


def module_kwargs(k):
    kw = gs.dit_module_kwargs(base(k))
    if k["prepend"]:
        kw["prepend_cond_dim"] = PREPEND_DIM
    return kw


def make_state(k):
    """name -> numpy fp32"""
    return gu.make_state(shapes(k), k["base"])


def weights(st):
    return {n: torch.from_numpy(v).to(F64) for n, v in st.items()}


def oracle_cfg(k):
    c = base(k)
    return dict(embed_dim=c["D"], depth=gs.DEPTH, num_heads=c["heads"], global_cond_type=c["gtype"], causal=False,
                qk_l2=c["qk"] == "l2")


def inputs(k):
    """fp32: ctx [B, S, dc], gl [B, GD]; neg / negm (the negative prompt ctx.flip(0) and its mask, density 0.6) or None; prepend
    [B, 3, 24] / prepend_mask or None; noise [B, C, T]: the draw generate_diffusion_cond(seed = the base case's, device="cpu")
    makes; init [B, C, T] or None; single calls: x [B, C, T] and t [B]"""
    c, B = base(k), k["B"]
    inp = gs.dit_inputs(c, B=B)
    mk = lambda n, shape: torch.from_numpy(gu.make_input(n, shape, c["seed"]))
    out = dict(ctx=inp["ctx"], gl=inp["gl"], neg=None, negm=None, prepend=None, prepend_mask=None, init=None, x=inp["lat"], t=inp["t"])
    if k["neg"]:
        out["neg"] = inp["ctx"].flip(0).contiguous()
        out["negm"] = torch.from_numpy(gu.make_mask("negm", (B, c["S"]), c["seed"], 0.6))
    if k["prepend"]:
        out["prepend"] = mk("prepend", (B, PREPEND_TOKENS, PREPEND_DIM))
        out["prepend_mask"] = torch.from_numpy(gu.make_mask("prependm", (B, PREPEND_TOKENS), c["seed"], 0.7))
    out["noise"] = torch.randn([B, gs.CIO, c["T"]], generator=torch.Generator().manual_seed(c["seed"]))
    if k["init"]:
        out["init"] = mk("init", (B, gs.CIO, c["T"]))
    return out


def start(k, inp):
    """x_0 in fp64 and the element-wise allowance of its fp32 computation: the noise itself, or (sample_rf with init_data)
    init (1 - sigma_max) + noise sigma_max - two coefficients rounded to fp32, two products, one sum: at most
    3 u (|init| (1 - sigma_max) + |noise| sigma_max) to first order; allowed 4 u (|init| + |noise|)"""
    noise = inp["noise"].to(F64)
    if not k["init"]:
        return noise, torch.zeros_like(noise)
    init, s = inp["init"].to(F64), k["sigma_max"]
    return init * (1 - s) + noise * s, 4 * U * (init.abs() + noise.abs())


def schedule(k):
    """the sampler's own fp32 linspace, steps + 1 values (the v sampler drops the last, 0, and never calls the model there)"""
    return torch.linspace(k["sigma_max"] if k["obj"] == "rectified_flow" else 1, 0, k["steps"] + 1)


# ------------------------------------------------------------------------------------------------ the guided forward
def _il(a, b):
    """[a0, b0, a1, b1, ...]"""
    return torch.stack([a, b], 1).flatten(0, 1)


@contextlib.contextmanager
def _prepend_not_skipped():
    """the transformer's output moved by one token: dit_inner's [plen:] then reads [plen - 1:-1]"""
    orig = ko.continuous_transformer

    def shifted(*a, **kw):
        out = orig(*a, **kw)
        return torch.cat([out[:, :1], out[:, :-1]], 1)

    ko.continuous_transformer = shifted
    try:
        yield
    finally:
        ko.continuous_transformer = orig


def guided(W, cfg, x, t, ctx, gl, neg=None, negm=None, prepend=None, prepend_mask=None, cfg_scale=1.0, scale_phi=0.0, defect=None):
    """ko.dit_forward (the operations and their order are its own) with one seam per defect"""
    if defect == "to_kv of layers 0 and 1 exchanged":
        a, b = ("transformer.layers.%d.cross_attn.to_kv.weight" % i for i in (0, 1))
        W = dict(W)
        W[a], W[b] = W[b], W[a]
    shift = _prepend_not_skipped() if defect == "prepended token not skipped" else contextlib.nullcontext()
    if cfg_scale == 1.0:
        with shift:
            return ko.dit_inner(W, cfg, x, t, cross_attn_cond=ctx, global_embed=gl, prepend_cond=prepend, prepend_cond_mask=prepend_mask)
    cat = _il if defect == "interleaved batch split as halves" else (lambda a, b: torch.cat([a, b], 0))
    null = torch.zeros_like(ctx)
    other = null
    if neg is not None and defect != "negative prompt ignored":
        other = neg
        if negm is not None and defect != "negative mask ignored":
            other = torch.where(negm.bool().unsqueeze(2), neg, null)
    bg = cat(gl, torch.zeros_like(gl) if defect == "global zeroed in the unconditional half" else gl)
    bp = bpm = None
    if prepend is not None:
        bp = cat(prepend, torch.zeros_like(prepend))
        bpm = cat(prepend_mask, prepend_mask) if prepend_mask is not None else None
    with shift:
        bo = ko.dit_inner(W, cfg, cat(x, x), cat(t, t), cross_attn_cond=cat(ctx, other), global_embed=bg, prepend_cond=bp,
                          prepend_cond_mask=bpm)
    cond, uncond = bo.chunk(2, 0)
    if defect == "halves swapped":
        cond, uncond = uncond, cond
    scale = {"cfg_scale - 1": cfg_scale - 1, "scale x 1.10": cfg_scale * 1.10}.get(defect, cfg_scale)
    out = uncond + (cond - uncond) * scale
    if scale_phi != 0.0:
        out = scale_phi * (out * (cond.std(1, keepdim=True) / out.std(1, keepdim=True))) + (1 - scale_phi) * out
    return out


@torch.no_grad()
def model_out(k, W, inp, x, t, mode="f64", defect=None):
    """the guided output [B, C, T] of the case's model on (x [B, C, T], t [B]) in fp64"""
    d = lambda n: None if inp[n] is None else inp[n].to(F64)
    with gs.MODES[mode]():
        return guided(W, oracle_cfg(k), x.to(F64), t.to(F64), d("ctx"), d("gl"), d("neg"), inp["negm"], d("prepend"), inp["prepend_mask"],
                      k["cfg"], k["phi"], defect)


def outputs(k, W, inp, xs, ts, mode="f64", defect=None):
    """teacher forced: the output per step as token rows [B T, C] on the recorded xs[i] [B, C, T] and ts[i] (a scalar: every clip of
    a step has the same).  "timestep of the next step": the model is fed the schedule's next value instead"""
    if defect == "timestep of the next step":
        nxt = schedule(k)
        ts = [nxt[i + 1] for i in range(len(xs))]
    elif defect in UPDATE_DEFECTS:
        raise ValueError(defect)
    ones = torch.ones(k["B"], dtype=F64)
    return [gs.rows_bct(model_out(k, W, inp, x, ones * float(t), mode, defect)) for x, t in zip(xs, ts)]


@torch.no_grad()
def free_run(k, W, inp, mode="f64"):
    """the oracle's own samplers from the case's start point: dict(xs [steps] [B, C, T], ts [steps] fp32 scalars, outs [steps]
    [B T, C], final [B, C, T])"""
    xs, ts, outs = [], [], []
    sched = schedule(k)

    def fn(x, t):
        assert len(set(t.tolist())) == 1 and float(t[0]) == float(sched[len(xs)])
        out = model_out(k, W, inp, x, t, mode)
        xs.append(x.clone()), ts.append(sched[len(ts)].clone()), outs.append(gs.rows_bct(out))
        return out

    x0 = start(k, inp)[0]
    final = ko.sample_ddim(fn, x0, k["steps"]) if k["obj"] == "v" else ko.sample_euler(fn, x0, k["steps"], k["sigma_max"])
    return dict(xs=xs, ts=ts, outs=outs, final=final)


# ------------------------------------------------------------------------------------------------ the sampler update
def update(k, i, x, out, defect=None):
    """fp64 update of step i from (x_i [B, C, T], out_i [B, C, T]) on the fp32 schedule values.  Returns dict(next=, next_tol=,
    ret=, ret_tol=): x_{i+1} (None after the last v step) and what the sampler would return after this step, each with the
    element-wise allowance for the fp32 operations of the formula, u = 2^-24, A = |x| + |out|, to first order in u:
    v      alpha, sigma = cos, sin(t pi / 2): pi rounded (0.5 u), one product (u), the function (1 ulp <= 2 u absolute, its argument
           <= pi / 2 off by 1.5 u relative, 2.4 u absolute): each within 5 u absolute.  pred = x alpha - out sigma and
           eps = x sigma + out alpha: the coefficients (5 u A), two products and one sum (2 u A): 7 u A each -> ret_tol 8 u A.
           x' = pred alpha' + eps sigma'', sigma'' = sqrt(sigma'^2 - 0) (a square and a root more: 7 u absolute):
           7 u A (|alpha'| + |sigma'|) <= 9.9 u A from pred and eps, (5 + 1) u A and (7 + 1) u A from the coefficients and
           products, 1.4 u A from the sum: 25.3 u A -> next_tol 32 u A.
    Euler  dt = t' - t rounded once, one product, one sum: u (|x| + 3 |dt out|) -> 4 u (|x| + |dt out|); the sampler returns x'."""
    x, out = x.to(F64), out.to(F64)
    t = schedule(k).to(F64)
    if k["obj"] == "v":
        al, si = torch.cos(t * math.pi / 2), torch.sin(t * math.pi / 2)
        A = x.abs() + out.abs()
        pred = x * al[i] - out * si[i]
        eps = x * si[i] + out * al[i]
        nxt = None
        if i < k["steps"] - 1:
            j = i if defect == "alpha, sigma of the step before" else i + 1
            nxt = pred * al[j] + eps * si[j]
        return dict(next=nxt, next_tol=32 * U * A, ret=pred, ret_tol=8 * U * A)
    dt = t[i + 1] - t[i]
    if defect == "dt with the wrong sign":
        dt = -dt
    nxt = x + dt * out
    tol = 4 * U * (x.abs() + (dt * out).abs())
    return dict(next=nxt, next_tol=tol, ret=nxt, ret_tol=tol)


def over(x, ref, tol):
    """the largest |x - ref| - tol over the elements (<= 0: inside)"""
    return ((x.to(F64) - ref).abs() - tol).max().item()


# ------------------------------------------------------------------------------------------------ the check
def yardstick(k, W, inp, traj):
    """r per step: emu against f64 on the fp64 free-running trajectory"""
    emu = outputs(k, W, inp, traj["xs"], traj["ts"], "emu")
    return [ratios(e, o).max().item() for e, o in zip(emu, traj["outs"])]


def worst(outs, outs64, r):
    """(the largest ratio / (M r(step)), step, row, that ratio) over the steps"""
    best = (-1.0, None, None, None)
    for i, (o, o64) in enumerate(zip(outs, outs64)):
        q = ratios(o, o64)
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        j = int(q.argmax())
        if q[j].item() / (M * r[i]) > best[0]:
            best = (q[j].item() / (M * r[i]), i, j, q[j].item())
    return best


def failure(outs, outs64, r, what=""):
    """None when every row of every step is within M r(step), else the message: the FIRST step that left the allowance"""
    for i, (o, o64) in enumerate(zip(outs, outs64)):
        q = ratios(o, o64)
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        j = int(q.argmax())
        if not q[j].item() <= M * r[i]:
            return f"{what}: step {i} row {j}: ratio {q[j].item():.3e} = {q[j].item() / r[i]:.2f} r > M r (r {r[i]:.3e}, M {M})"
    return None


def reference(k):
    """everything that comes from the reference alone: state, weights, inputs, the fp64 free run and the yardstick per step.  A
    single-call case is a trajectory of one step at (x, t) of inputs(), t the same for every clip"""
    st = make_state(k)
    W, inp = weights(st), inputs(k)
    if k["steps"]:
        traj = free_run(k, W, inp)
    else:
        x, t = inp["x"].to(F64), inp["t"][-1]
        traj = dict(xs=[x], ts=[t], final=None)
        traj["outs"] = outputs(k, W, inp, traj["xs"], traj["ts"])
    return dict(k=k, st=st, W=W, inp=inp, traj=traj, r=yardstick(k, W, inp, traj))
