"""The VAE conv stacks per slice: every output, input gradient and parameter gradient of the Oobleck autoencoder (inference path,
autograd units, partly frozen, chunked) and of the mel-VAE is cut into runs of 16 and each run is held to an fp64 run of the
oracle, with a yardstick that comes from the reference alone.  Pure torch on the CPU; shared by tests/test_vae_oracle_cpu.py (the
yardstick, the seeded defects and the chunk loop on the reference itself) and tests/test_vae_oracle_gpu.py (the HIP path).

Reference  ko.oobleck_encoder / ko.oobleck_decoder / ko.melvae_* on an fp64 state (they keep the dtype they are given).  Without a
           defect and in fp64 nothing of the oracle is replaced.  The chunk loop of the reference project (its autoencoders.py:
           429-560: chunks one by one, pasted in order, the last one anchored at the end) is restated in chunked() - not the
           drop-in's _chunk_plan - and pinned against the reference-made fixtures of tests/golden/chunked_vae.npz.
Slices     a [B, C, L] tensor: per (b, c), runs of RUN = 16 consecutive positions that start anew at every seam of the
           reference's chunk loop (a seam's neighbourhood is then a slice of its own; a piece under 8 positions joins its
           neighbour); a parameter gradient: gs.view2d and gs.bounds, runs of 16 rows.
Scale      gs.slice_scale's: max(|ref_slice|, 0.25 |ref| sqrt(slice share)); no slice is excluded.
Yardstick  r(case, tensor) = the largest |emu - f64|_slice / scale over the tensor's slices and over DRAWS seeded sign draws,
           floored at the case's median.  emu: the oracle in fp32 end to end (forward and autograd) from the same fp32 state, with
           a signed perturbation on every activation and on its derivative, of the size the project measured for that intrinsic
           on the device: ALLOW of tests/test_conv_gpu.py (imported, not copied) divided by the margin of 4 that file states -
           SNAKE in units of (1 + |a x|) / (b + 1e-9), ELU / TANH / GATE in units of 1, the derivative terms as test_act_bwd
           bounds them (dx: 2 a unit; dalpha: 2 unit |x| a; dbeta: 2 unit); DIV on the row scale of every weight-norm fold and of
           its backward (one fast-math division and square root per output row: csrc/conv1d.hip wn_fold_kernel - the mel-VAE's
           encoder, which has no other intrinsic, showed on the device that the emulation needs this point).  A bf16 case (O7)
           rounds to bf16 at every store the kernels make: each conv's output, and the activated second output of a dual store
           separately, from the unrounded accumulator.  The mel-VAE's anti-aliased activation runs its FIRs in fp32 like everything else.
Pools      a gradient too small for slices of its own - every vector (alpha, beta, bias, weight_g: 4 to 32 numbers) and every
           weight with fewer than 16 rows (the 4- and 8-channel convs) - is joined with the others of its kind, flattened and in
           the order of their names, into "pool:<kind>", cut into runs of RUN_VECTOR = 32 numbers.  Tensor by tensor these drove M:
           one alpha gradient of 4 numbers reached 4.1 r on a fresh sign draw, where no activation tensor passes 2.6.
Assertion  |g - f64|_slice <= M r scale on every slice of every tensor, M = 4.  M is measured: the heavier emulation (allowances
           doubled, fresh sign seeds - HEAVY_DRAWS of them -, every conv summed tap by tap in fp32 over two halves of its input
           channels: another order, like the split-K partials and the weight-gradient atomics) reaches the multiples of r
           below; M = ceil(1.5 x the largest) = ceil(1.5 x 2.60), 1.5 for the rounding points only the device has.
           tests/test_vae_oracle_cpu.py holds the heavier emulation to M on every case and prints what it reaches (the figures
           move in the second digit with the CPU's thread count: O2 2.50 ... 2.60).
           heavier / r per case (largest over the tensors and the draws):
               O1 2.49  O2 2.60  O3 2.24  O4 2.02  O5 2.09  O6 2.37  O7 0.96
               chunked: decode (48, 16) 1.78  decode (32, 8) 1.71  encode (48, 16) 2.22
               mel-VAE: amp1_causal 1.82  amp2_same 2.41  up5x3 2.03
Defects    DEFECTS, seeded one at a time into the reference (through the seams this file puts around ko._act, ko.F, ko.snake,
           ko.residual_unit, ko.wn_weight for one run - kalle_oracle.py itself is unchanged); BLIND: the (case, defect) pairs the
           fixture state cannot show, asserted blind on the CPU.
"""
import contextlib
import functools
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grad_slices as gs  # noqa: E402
import test_conv_gpu as tcg  # noqa: E402  (ALLOW: the measured allowances of the fast-math intrinsics, x 4)

gu, ko = gs.gu, gs.ko
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
RUN = 16
RUN_VECTOR = 32         # rows of a slice of a vector's gradient (alpha, beta, bias, weight_g): see M
M = 4.0
DRAWS = 12              # seeded sign draws of the yardstick's emulation (one draw is noisy on 16-row slices); draw d sums in order d % 3
HEAVY_DRAWS = 4         # draws of the heavier emulation M is measured with
MARGIN = 4.0            # tests/test_conv_gpu.py: ALLOW = measured x 4
ALLOW = tcg.ALLOW


# ------------------------------------------------------------------------------------------------ cases
def _case(cid, strides, ch, c_mults, lat, snake, audio, B, frames, seed, extra=0, nearest=False, antialias=False, bf16=False,
          encoder=True, train=True):
    ratio = math.prod(strides)
    return dict(id=cid, strides=list(strides), ch=ch, c_mults=list(c_mults), lat=lat, snake=snake, audio=audio, B=B, frames=frames,
                seed=seed, extra=extra, nearest=nearest, antialias=antialias, bf16=bf16, encoder=encoder, train=train, ratio=ratio,
                samples=frames * ratio + extra)


CASES = {c["id"]: c for c in [
    _case("O1", (2, 4, 5), 8, (1, 2, 4), 4, True, 2, 2, 30, 901),                      # the fixture's configuration
    _case("O2", (3, 8), 12, (1, 2), 6, False, 1, 3, 17, 902, extra=3),                 # odd stride (K = 2s + 1), 12 / 24 channels
    _case("O3", (5, 3, 2), 4, (1, 2, 4), 2, True, 2, 1, 40, 903, extra=3),             # trailing inputs no strided conv reads
    _case("O4", (8, 2), 16, (1, 2), 8, False, 2, 2, 5, 904),                           # deepest length 5 < the dilation-9 padding of 27
    _case("O5", (2, 4, 5), 8, (1, 2, 4), 4, True, 2, 2, 37, 905, nearest=True, encoder=False),
    _case("O6", (2, 4), 8, (1, 2), 4, True, 2, 2, 20, 906, antialias=True, train=False),
    _case("O7", (2, 4, 5), 8, (1, 2, 4), 4, True, 2, 2, 30, 901, bf16=True, train=False),
]}
TRAIN_CASES = [k for k, c in CASES.items() if c["train"]]
FROZEN_CASES = ["O1", "O2"]
# name -> is the parameter frozen
FROZEN_SETS = {
    "encoder": lambda n: n.startswith("encoder."),              # and the input requires no gradient
    "decoder": lambda n: n.startswith("decoder."),              # gradients pass through it to the encoder
    "alpha_beta": lambda n: n.endswith((".alpha", ".beta")),
    "all_but_bias": lambda n: not n.endswith(".bias"),
}


def shapes(c):
    s = []
    if c["encoder"]:
        s += ko.oobleck_encoder_shapes(c["audio"], c["ch"], 2 * c["lat"], c["c_mults"], c["strides"], c["snake"], prefix="encoder.")
    return s + ko.oobleck_decoder_shapes(c["audio"], c["ch"], c["lat"], c["c_mults"], c["strides"], c["snake"], prefix="decoder.",
                                         nearest=c["nearest"])


@functools.lru_cache(maxsize=None)
def _state(cid):
    c = CASES[cid]
    return gu.make_state(shapes(c), c["seed"])


def state(c):
    return _state(c["id"])


def inputs(c):
    """fp32 inputs (numpy -> torch): wav (bf16 values in a bf16 case: the reference starts from them), or z for a decoder alone"""
    mk = lambda n, shape, sc=1.0: torch.from_numpy(gu.make_input(n, shape, c["seed"], sc))
    if not c["encoder"]:
        return dict(z=mk("z", (c["B"], c["lat"], c["frames"])))
    wav = mk("wav", (c["B"], c["audio"], c["samples"]), 0.5)
    return dict(wav=wav.to(BF16).float() if c["bf16"] else wav)


def cotangent(c, name, shape):
    return torch.from_numpy(gu.make_input(name, tuple(shape), c["seed"]))


# ------------------------------------------------------------------------------------------------ slices, scale, ratios
def cuts_of(L, seams=()):
    """runs of RUN positions that start anew at every seam; a last piece shorter than half a run joins the run before it (a slice
    of a few positions would be measured by its own noise)"""
    edges = [0] + sorted({s for s in seams if 0 < s < L}) + [L]
    cuts = {L}
    for a, b in zip(edges, edges[1:]):
        pts = list(range(a, b, RUN))
        if len(pts) > 1 and b - pts[-1] < RUN // 2:
            pts.pop()
        cuts |= set(pts)
    return sorted(cuts)


def act_ratio(g, ref, seams=()):
    """[B C, slices]: |g - ref|_slice / scale per (b, c) and run of positions"""
    assert tuple(g.shape) == tuple(ref.shape), (tuple(g.shape), tuple(ref.shape))
    L = ref.shape[-1]
    g2, r2 = g.detach().to(F64).reshape(-1, L), ref.detach().to(F64).reshape(-1, L)
    cuts = torch.tensor(cuts_of(L, seams))

    def seg(t):
        cs = torch.cat([torch.zeros(t.shape[0], 1, dtype=F64), (t ** 2).cumsum(1)], 1)
        return (cs[:, cuts[1:]] - cs[:, cuts[:-1]]).clamp_min(0.0)

    err, own = seg(g2 - r2).sqrt(), seg(r2).sqrt()
    floor = 0.25 * r2.norm() * ((cuts[1:] - cuts[:-1]).to(F64) / r2.numel()).sqrt()
    sc = torch.maximum(own, floor[None, :])
    return torch.where(sc > 0, err / sc.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))


def is_act(name):
    """a [B, C, L] tensor cut along L (the pooled vectors, "pool:<kind>", are cut by rows like a parameter)"""
    return ":" in name and not name.startswith("pool:")


def ratio(g, ref, name, seams=()):
    """the per-slice ratios of one tensor (any shape of result; the caller takes the largest)"""
    if is_act(name):
        return act_ratio(g, ref, seams)
    rows, cols = gs.view2d(ref).shape
    return gs.slice_ratio(g.detach(), ref, gs.bounds(rows, RUN_VECTOR if cols == 1 else RUN))


VECTOR_KINDS = ("alpha", "beta", "bias", "weight_g")


def _pool_kind(name, t):
    """the pool a parameter's gradient joins (None: it is cut on its own): every vector, and every weight with fewer rows than a
    run - the 4- and 8-channel convs, whose whole gradient would be one slice of a few dozen numbers"""
    kind = name.rsplit(".", 1)[1]
    if kind in VECTOR_KINDS or (kind == "weight_v" and t.shape[0] < RUN):
        return kind
    return None


def pooled(t):
    """the gradients too small for slices of their own (see M) joined per kind, flattened and in the order of their names, into
    "pool:<kind>" - one long vector per kind, cut like any other into runs of RUN_VECTOR numbers"""
    out, pools = {}, {}
    for n in sorted(t):
        kind = None if is_act(n) else _pool_kind(n, t[n])
        if kind is None:
            out[n] = t[n]
        else:
            pools.setdefault(kind, []).append(t[n].detach().reshape(-1))
    out.update({"pool:" + k: torch.cat(v) for k, v in pools.items()})
    return out


def pool_members(t, kind):
    """[(name, first, end)]: where each tensor of `t` lies in the pool of its kind"""
    out, at = [], 0
    for n in sorted(t):
        if not is_act(n) and _pool_kind(n, t[n]) == kind:
            out.append((n, at, at + t[n].numel()))
            at += t[n].numel()
    return out


def worst(got, ref, seams=None):
    """name -> the largest slice ratio, over the names of `ref` that `got` holds"""
    seams = seams or {}
    return {n: ratio(got[n], ref[n], n, seams.get(n, ())).max().item() for n in ref if n in got}


def yardstick_of(ref, emus, seams=None):
    """(r, raw): raw = the largest ratio over the draws, r = raw floored at the median over the tensors"""
    ws = [worst(e, ref, seams) for e in emus]
    raw = {n: max(w[n] for w in ws) for n in ref}
    med = statistics.median(raw.values())
    return {n: max(v, med) for n, v in raw.items()}, raw


def rho_of(got, ref, r, seams=None):
    """name -> worst slice ratio / r"""
    return {n: v / r[n] for n, v in worst(got, ref, seams).items()}


def failures(rho, m=M):
    return sorted(((n, round(v, 2)) for n, v in rho.items() if not v <= m), key=lambda f: -f[1])


def rel_l2(a, b):
    return gs.rel_l2(a.detach(), b.detach())


# ------------------------------------------------------------------------------------------------ the seams around the oracle
def _bf16(x):
    return x.detach().to(BF16).to(x.dtype)


class _RoundST(torch.autograd.Function):
    """rounds to bf16 on the way forward (nothing differentiates through a bf16 case: forward only)"""

    @staticmethod
    def forward(ctx, x):
        return _bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _PertSnake(torch.autograd.Function):
    """the perturbation of one SnakeBeta call: k u unit on the value, and on the way back the derivative terms of test_act_bwd"""

    @staticmethod
    def forward(ctx, x, alpha, beta, k, s):
        a, b = alpha.detach().exp()[None, :, None], beta.detach().exp()[None, :, None]
        unit = (1 + (a * x.detach()).abs()) / (b + 1e-9)
        ctx.save_for_backward(x.detach(), a, b, unit, s)
        ctx.k = k
        return s[0] * (k * U) * unit

    @staticmethod
    def backward(ctx, g):
        x, a, b, unit, s = ctx.saved_tensors
        e = 2 * ctx.k * U * unit * g
        return (s[1] * e * a, (s[2] * e * x.abs()).sum((0, 2)) * a.view(-1), (s[3] * e / (b + 1e-9)).sum((0, 2)) * b.view(-1), None,
                None)


class _PertElu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s):
        neg = (x.detach() <= 0).to(x.dtype)
        ctx.save_for_backward(neg, s)
        ctx.k = k
        return s[0] * (k * U) * neg

    @staticmethod
    def backward(ctx, g):
        neg, s = ctx.saved_tensors
        return s[1] * (ctx.k * U) * neg * g, None, None


class _ScaleRows(torch.autograd.Function):
    """w (1 + e) per row on the way forward, the gradient (1 + e') per row on the way back: the division and the square root of
    the weight-norm fold (scale = g / sqrtf(sum v^2), one per output row) and of its backward"""

    @staticmethod
    def forward(ctx, w, e, eb):
        ctx.save_for_backward(eb)
        return w * (1 + e)

    @staticmethod
    def backward(ctx, g):
        return g * (1 + ctx.saved_tensors[0]), None, None


class _ZeroGrad(torch.autograd.Function):
    """identity; the gradient of positions [lo, hi) of the last axis is dropped"""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.span = (lo, hi)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[..., ctx.span[0]:ctx.span[1]] = 0
        return g, None, None


class _TapShift(torch.autograd.Function):
    """identity on a weight [.., .., K]; on the way back the gradient of the middle tap is the next tap's"""

    @staticmethod
    def forward(ctx, w):
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        k = g.shape[-1] // 2
        g[..., k] = g[..., k + 1]
        return g


def _round_bits(x, bits):
    m, e = torch.frexp(x.detach())
    return x + (torch.ldexp((m * 2.0 ** bits).round() / 2.0 ** bits, e) - x.detach())


class _Shim:
    """stands where kalle_oracle keeps a module (torch.nn.functional, torch): the named functions replaced, the rest passed on"""

    def __init__(self, base, **over):
        self.__dict__["_base"] = base
        self.__dict__.update(over)

    def __getattr__(self, n):
        return getattr(self._base, n)


def _is_unit(sd):
    """a ResidualUnit's state (layers.{0..3}.*): no nested keys"""
    return all(k.count(".") <= 2 for k in sd)


# defects: label -> (kind, the cases' property it needs)
FORWARD_DEFECTS = ["dilated_right_edge", "act_params_of_neighbour", "skip_activated", "convT_pad_floor", "nearest_pad_swapped",
                   "cout_tail_zeroed", "stored_11_bits"]
BACKWARD_DEFECTS = ["bwd_extra_zeroed", "dalpha_no_logscale", "dalpha_dbeta_swapped", "dg_dropped", "wgrad_tap_shifted",
                    "bwd_residual_dropped"]
CHUNK_DEFECTS = ["seam_moved", "anchored_at_start", "keep_from_off_by_one"]
DEFECTS = FORWARD_DEFECTS + BACKWARD_DEFECTS


def applies(defect, c):
    """does the case have the structure the defect lives in (whether the fixture state SHOWS it is another matter: BLIND)"""
    if defect == "act_params_of_neighbour":
        return c["snake"]
    if defect in ("dalpha_no_logscale", "dalpha_dbeta_swapped"):
        return c["snake"] and c["train"]
    if defect == "convT_pad_floor":
        return any(s % 2 for s in c["strides"]) and not c["nearest"]
    if defect == "nearest_pad_swapped":
        return c["nearest"]
    if defect == "bwd_extra_zeroed":
        return c["encoder"] and c["train"] and c["extra"] > 0
    if defect in BACKWARD_DEFECTS:
        return c["train"]
    return True


# pairs the fixture state cannot show (asserted blind in tests/test_vae_oracle_cpu.py; never extended to make a device test pass)
BLIND = {
    # the anchored chunk's place: the reference pastes it so that it ends at the output's end, the defect at to_out(start).  The
    # anchored chunk starts at total_in - chunk_in, a whole chunk is chunk_out outputs, and both lengths are whole multiples of
    # the ratio (or its remainder falls off both alike), so the two places are the same number at every length
    ("chunked", "anchored_at_start"),
    # the bf16 case: every store rounds to 8 bits, r is 1.2e-2, and what moves a slice by less than that is not seen - an edge tap,
    # a neighbour's alpha and beta in one unit, 11 bits where 8 are kept.  The fp32 cases O1 ... O6 show all three
    ("O7", "dilated_right_edge"), ("O7", "act_params_of_neighbour"), ("O7", "stored_11_bits"),
}


class _Run:
    """one run of the oracle with its seams: mode "f64" (exact), "emu" / "heavy" (fp32 + perturbations), and at most one defect"""

    def __init__(self, c, mode, draw=0, defect=None):
        self.c, self.mode, self.defect = c, mode, defect
        self.k = {"f64": 0.0, "emu": 1.0 / MARGIN, "heavy": 2.0 / MARGIN}[mode]
        # the order every conv is summed in: 0 the library's, 1 tap by tap, 2 tap by tap from the last, 3 (heavier) tap by tap
        # over two halves of the input channels, added at the end like split-K partials.  The draws of the yardstick's emulation
        # go through 0, 1, 2 in turn: a draw samples the fp32 rounding as well as the signs
        self.order = 3 if mode == "heavy" else draw % 3 if mode == "emu" else 0
        self.bf16 = bool(c.get("bf16")) and mode != "f64"
        self.gen = torch.Generator().manual_seed(7919 * draw + (104729 if mode == "heavy" else 1) + c.get("seed", 0))
        self.n = dict(unit=0, unit_act=0)
        self.seen = set()          # defect sites already used (every defect is seeded ONCE per run)
        self.keep = {}             # id(rounded tensor) -> (rounded, unrounded): a dual store activates the unrounded accumulator
        self.orig = dict(_act=ko._act, F=ko.F, snake=ko.snake, residual_unit=ko.residual_unit, torch=ko.torch, wn_weight=ko.wn_weight)

    # -- helpers
    def signs(self, n, like):
        return (torch.randint(0, 2, (n,) + tuple(like.shape), generator=self.gen, dtype=torch.int8) * 2 - 1).to(like.dtype)

    def begin(self):
        """a new pass (inference encode, inference decode, the training pass): the defect is seeded once in each"""
        self.n = dict(unit=0, unit_act=0)
        self.seen = set()

    def once(self, site):
        if site in self.seen:
            return False
        self.seen.add(site)
        return True

    def store(self, y):
        if not self.bf16:
            return y
        r = _RoundST.apply(y)
        self.keep[id(r)] = (r, y)
        return r

    def unrounded(self, x):
        hit = self.keep.get(id(x))
        return hit[1] if hit is not None and hit[0] is x else x

    # -- activations
    def snake_value(self, x, alpha, beta=None, logscale=False):
        y = self.orig["snake"](x, alpha, beta, logscale)
        if self.k:
            if not torch.is_grad_enabled():         # forward only (also the mel-VAE's Snake: b = a, log scale or not)
                a = alpha.detach().view(1, -1, 1)
                b = a if beta is None else beta.detach().view(1, -1, 1)
                a, b = (a.exp(), b.exp()) if logscale else (a, b)
                y = y + self.signs(1, x)[0] * (self.k * ALLOW["SNAKE"] * U) * (1 + (a * x.detach()).abs()) / (b + 1e-9)
            else:
                y = y + _PertSnake.apply(x, alpha, beta, self.k * ALLOW["SNAKE"], self.signs(4, x))
        return y

    def act(self, sd, pre, x, use_snake):
        c, unit = self.c, _is_unit(sd)
        x = self.unrounded(x)
        if unit and pre == "layers.0":
            self.n["unit_act"] += 1
            if self.defect == "act_params_of_neighbour" and use_snake and self.n["unit_act"] == 2 and self.once("act"):
                pre = "layers.2"                     # the same unit's second activation: same width, other alpha and beta
        if c.get("antialias") and not use_snake:
            raise NotImplementedError("anti-aliased ELU")
        if use_snake and c.get("antialias") and not unit and "layers.0.layers.1.weight_v" not in sd:
            # Activation1d around the block's own / the last activation (the reference hands the flag to no ResidualUnit and to no
            # EncoderBlock): ko.activation1d calls ko.snake, which this run has replaced by snake_value
            return self.store(ko.activation1d(x, sd[pre + ".alpha"], sd[pre + ".beta"], logscale=True))
        if use_snake:
            return self.store(self.snake_value(x, sd[pre + ".alpha"], sd[pre + ".beta"], True))
        y = TF.elu(x)
        if self.k:
            y = y + _PertElu.apply(x, self.k * ALLOW["ELU"], self.signs(2, x))
        return self.store(y)

    def tanh(self, x):
        y = torch.tanh(self.unrounded(x))
        if self.k:
            y = y + self.signs(1, y)[0] * (self.k * ALLOW["TANH"] * U)
        return self.store(y)

    def gate_tanh(self, x):
        """ko.torch.tanh of the mel-VAE (the WaveNet gate's tanh and the output's): TANH u"""
        y = torch.tanh(x)
        return y + self.signs(1, y)[0] * (self.k * ALLOW["TANH"] * U) if self.k else y

    def gate_sigmoid(self, x):
        """the gate's other factor: tanh x sigmoid is allowed GATE u in all, so the sigmoid carries GATE u on its own"""
        y = torch.sigmoid(x)
        return y + self.signs(1, y)[0] * (self.k * ALLOW["GATE"] * U) if self.k else y

    def wn_weight(self, sd, pre):
        """ko.wn_weight with the fold kernel's rounding point: its row scale g / sqrtf(sum v^2) is a fast-math division and square
        root, DIV u of the quotient, the same for a whole row of the weight"""
        w = self.orig["wn_weight"](sd, pre)
        if not self.k:
            return w
        e = self.signs(2, w[:, :1, :1]) * (self.k * ALLOW["DIV"] * U)
        return _ScaleRows.apply(w, e[0], e[1])

    # -- convs
    def _after(self, y, Cout, kind):
        d = self.defect
        if d == "cout_tail_zeroed" and Cout % 8 and (Cout > 8 or not self.c.get("wide_odd")) and self.once("cout"):
            y = torch.cat([y[:, :Cout - Cout % 8], torch.zeros_like(y[:, Cout - Cout % 8:])], 1)
        if d == "stored_11_bits" and kind in ("down", "up") and self.once("r11"):
            y = _round_bits(y, 11)
        return y

    def _ordered(self, term, K, Cin):
        """sum of term(tap, first channel, end channel) in this run's order"""
        taps = range(K - 1, -1, -1) if self.order == 2 else range(K)
        halves = [(0, Cin // 2), (Cin // 2, Cin)] if self.order == 3 and Cin > 1 else [(0, Cin)]
        parts = []
        for lo, hi in halves:
            y = None
            for k in taps:
                t = term(k, lo, hi)
                y = t if y is None else y + t
            parts.append(y)
        return parts[0] if len(parts) == 1 else parts[0] + parts[1]

    def conv1d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1, _store=True):
        if groups != 1:                               # the depthwise FIRs of the anti-aliased activation
            return TF.conv1d(x, w, b, stride, padding, dilation, groups)
        d = self.defect
        Cout, _, K = w.shape
        L = x.shape[2]
        kind = "down" if stride > 1 else "up" if (K % 2 == 0 and padding == 0) else "k1" if K == 1 else "k"
        if d == "dilated_right_edge" and dilation == 3 and self.once("edge"):
            x = torch.cat([x[..., :-1], torch.zeros_like(x[..., -1:])], -1)      # the last sample is read as padding
        if d == "wgrad_tap_shifted" and dilation == 3 and self.once("tap"):
            w = _TapShift.apply(w)
        if d == "bwd_extra_zeroed" and stride > 1:
            nat = ((L + 2 * padding - K) // stride) * stride - 2 * padding + K
            extra = max(0, min(L - nat, padding))
            if extra and self.once("extra"):
                x = _ZeroGrad.apply(x, nat, nat + extra)
        if self.order:
            xp = TF.pad(x, (padding, padding))
            Lout = (L + 2 * padding - dilation * (K - 1) - 1) // stride + 1
            span = (Lout - 1) * stride + 1
            y = self._ordered(lambda k, lo, hi: TF.conv1d(xp[:, lo:hi, k * dilation:k * dilation + span], w[:, lo:hi, k:k + 1], None,
                                                          stride), K, x.shape[1])
            y = y + b[None, :, None] if b is not None else y
        else:
            y = TF.conv1d(x, w, b, stride, padding, dilation)
        y = self._after(y, Cout, kind)
        return self.store(y) if _store else y

    def conv_transpose1d(self, x, w, b=None, stride=1, padding=0, groups=1):
        if groups != 1:
            return TF.conv_transpose1d(x, w, b, stride, padding, groups=groups)
        Cout, K = w.shape[1], w.shape[2]
        Lout = (x.shape[2] - 1) * stride - 2 * padding + K
        if self.defect == "convT_pad_floor" and stride % 2 and padding == (stride + 1) // 2 and self.once("floor"):
            y = TF.conv_transpose1d(x, w, b, stride, stride // 2)[..., :Lout]
        elif self.order:
            y = self._ordered(lambda k, lo, hi: TF.pad(TF.conv_transpose1d(x[:, lo:hi], w[lo:hi, :, k:k + 1], None, stride),
                                                       (k, K - 1 - k)), K, x.shape[1])
            y = y[..., padding:padding + Lout]
            y = y + b[None, :, None] if b is not None else y
        else:
            y = TF.conv_transpose1d(x, w, b, stride, padding)
        return self.store(self._after(y, Cout, "up"))

    def pad(self, x, pads, mode="constant", value=None):
        if self.defect == "nearest_pad_swapped" and mode == "constant" and len(pads) == 2 and pads[1] == pads[0] + 1 and self.once("pad"):
            pads = (pads[1], pads[0])
        return TF.pad(x, pads, mode, value)

    def residual_unit(self, sd, x, dilation, use_snake):
        """ko.residual_unit with its store made explicit (conv + bias + skip is ONE store of the k = 1 conv) and two defect sites"""
        self.n["unit"] += 1
        d, site = self.defect, self.n["unit"] == 2
        h0 = ko._act(sd, "layers.0", x, use_snake)
        h = ko.F.conv1d(h0, ko.wn_weight(sd, "layers.1"), sd["layers.1.bias"], dilation=dilation, padding=3 * dilation)
        h = ko._act(sd, "layers.2", h, use_snake)
        h = self.conv1d(h, ko.wn_weight(sd, "layers.3"), sd["layers.3.bias"], _store=False)
        skip = x
        if d == "skip_activated" and site:
            skip = h0
        if d == "bwd_residual_dropped" and site:
            skip = x.detach()
        return self.store(skip + h)

    @contextlib.contextmanager
    def installed(self, melvae=False):
        ko._act, ko.snake, ko.residual_unit, ko.wn_weight = self.act, self.snake_value, self.residual_unit, self.wn_weight
        ko.F = _Shim(TF, conv1d=self.conv1d, conv_transpose1d=self.conv_transpose1d, pad=self.pad)
        if melvae:
            ko.torch = _Shim(torch, tanh=self.gate_tanh, sigmoid=self.gate_sigmoid)
        try:
            yield self
        finally:
            for k, v in self.orig.items():
                setattr(ko, k, v)


def _post_defect(defect, g, st):
    """the backward defects that are a wrong last step of one parameter's gradient: applied to the finished gradients"""
    pick = lambda suffix: sorted(n for n in g if n.endswith(suffix) and not is_act(n))      # noqa: E731
    g = dict(g)
    if defect in ("dalpha_no_logscale", "dalpha_dbeta_swapped"):
        names = pick(".alpha")
        n = names[len(names) // 2]
        nb = n[:-len("alpha")] + "beta"
        if defect == "dalpha_no_logscale":
            g[n] = g[n] / torch.from_numpy(st[n]).to(g[n].dtype).exp()
        else:
            g[n], g[nb] = g[nb], g[n]
    if defect == "dg_dropped":
        names = pick(".weight_g")
        n = names[len(names) // 2]
        g[n] = torch.zeros_like(g[n])
    return g


# ------------------------------------------------------------------------------------------------ the Oobleck reference
def _sub(sd, prefix):
    return ko._sub(sd, prefix)


def _decode(run, sd, c, z):
    y = ko.oobleck_decoder(_sub(sd, "decoder."), z, c["strides"], c["snake"], final_tanh=False, nearest=c["nearest"])
    return run.tanh(y) if run is not None else torch.tanh(y)


def _encode(sd, c, wav):
    return ko.oobleck_encoder(_sub(sd, "encoder."), wav, c["strides"], c["snake"])


@functools.lru_cache(maxsize=None)
def latents_in(cid):
    """what the inference check of the decoder is fed: the fp64 reference's mean latents, rounded to the input's format"""
    c = CASES[cid]
    if not c["encoder"]:
        return inputs(c)["z"]
    z = reference(cid)["inf:z"][:, :c["lat"]]
    return (z.to(BF16) if c["bf16"] else z).float().contiguous()


def _reference(c, mode, draw, defect):
    dtype = F64 if mode == "f64" else F32
    plain = mode == "f64" and defect is None and not c["antialias"]     # nothing of the oracle is replaced
    run = None if plain else _Run(c, mode, draw, None if defect in ("dalpha_no_logscale", "dalpha_dbeta_swapped", "dg_dropped") else defect)
    st = state(c)
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(c["train"]) for k, v in st.items()}
    inp = {k: v.to(dtype) for k, v in inputs(c).items()}
    out = {}
    begin = run.begin if run is not None else (lambda: None)
    first = c["encoder"] and mode == "f64" and defect is None       # the run latents_in itself reads
    zl_in = None if first else latents_in(c["id"]).to(dtype)        # (computed outside this run's seams and grad mode)
    with (run.installed() if run is not None else contextlib.nullcontext()):
        with torch.no_grad():
            if c["encoder"]:
                out["inf:z"] = _encode(sd, c, inp["wav"])
            begin()
            if first:
                zl = out["inf:z"][:, :c["lat"]]
                zl = (zl.to(BF16) if c["bf16"] else zl.float()).to(dtype)
            else:
                zl = zl_in
            out["inf:rec"] = _decode(run, sd, c, zl)
        begin()
        if c["train"]:
            if c["encoder"]:
                wav = inp["wav"].requires_grad_(True)
                z = _encode(sd, c, wav)
                rec = _decode(run, sd, c, z[:, :c["lat"]] + 0.3 * z[:, c["lat"]:])
                loss = (z * cotangent(c, "dz", z.shape).to(dtype)).sum() + (rec * cotangent(c, "drec", rec.shape).to(dtype)).sum()
                loss.backward()
                out.update({"act:z": z.detach(), "act:rec": rec.detach(), "act:dwav": wav.grad})
            else:
                z = inp["z"].requires_grad_(True)
                rec = _decode(run, sd, c, z)
                (rec * cotangent(c, "drec", rec.shape).to(dtype)).sum().backward()
                out.update({"act:rec": rec.detach(), "act:dz": z.grad})
            out.update({k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in sd.items()})
    if defect in ("dalpha_no_logscale", "dalpha_dbeta_swapped", "dg_dropped"):
        out = _post_defect(defect, out, st)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid, mode="f64", draw=0, defect=None):
    """every tensor of a case, as computed (select() makes of it what is compared): "inf:z", "inf:rec" (the inference path: encode, decode of latents_in), and for a training
    case "act:z", "act:rec", "act:dwav" (a decoder alone: "act:rec", "act:dz") and the gradient of every parameter, by its name"""
    c = dict(CASES[cid])
    widths = [c["ch"] * m for m in [1] + c["c_mults"]] + [2 * c["lat"], c["audio"]]
    c["wide_odd"] = any(w % 8 and w > 8 for w in widths)
    return _reference(c, mode, draw, defect)


def select(raw, frozen=None):
    """what is compared of a run: the activations and the gradients of the trainable parameters (frozen: a key of FROZEN_SETS;
    with the encoder frozen the input carries no gradient either), the small ones pooled"""
    keep = (lambda n: True) if frozen is None else (lambda n: not FROZEN_SETS[frozen](n))
    return pooled({n: v for n, v in raw.items() if (n != "act:dwav" or frozen != "encoder") if is_act(n) or keep(n)})


@functools.lru_cache(maxsize=None)
def yardstick(cid, frozen=None):
    """(r, raw) over select(reference(cid), frozen)"""
    return yardstick_of(select(reference(cid), frozen), [select(reference(cid, "emu", d), frozen) for d in range(DRAWS)])


# ------------------------------------------------------------------------------------------------ chunked encode / decode
CHUNK_CASE = "O1"
CHUNK_LATENTS = 100
# (direction, chunk size, overlap) in latents: 100 latents anchor a last chunk at every one of them
CHUNKED = [("decode", 48, 16), ("decode", 32, 8), ("encode", 48, 16)]


def chunked(fn, x, chunk_in, hop_in, to_out, chunk_out, total_out, trim, defect=None):
    """the reference project's chunk loop, restated: chunks start every hop_in inputs, one more is anchored at the end when they
    do not end there; each is run through fn on its own and pasted in order (a later chunk overwrites an earlier one); `trim`
    outputs are dropped on every edge that has a neighbour; the last chunk ends at total_out.  Returns (y, seams): the places
    where a paste begins or ends."""
    total_in = x.shape[2]
    starts = list(range(0, total_in - chunk_in + 1, hop_in))
    if starts[-1] + chunk_in != total_in:
        starts.append(total_in - chunk_in)
    y, seams = None, set()
    for i, s0 in enumerate(starts):
        yc = fn(x[:, :, s0:s0 + chunk_in])
        last = i == len(starts) - 1
        if y is None:
            y = torch.zeros((x.shape[0], yc.shape[1], total_out), dtype=yc.dtype)
        if last:
            hi = total_out
            lo = hi - yc.shape[2]
            if defect == "anchored_at_start":
                lo = to_out(s0)
                hi = lo + yc.shape[2]
        else:
            lo = to_out(i * hop_in)
            hi = lo + chunk_out
        a, b = 0, yc.shape[2]
        if i > 0:
            lo, a = lo + trim, a + trim
        if not last:
            hi, b = hi - trim, b - trim
        if defect == "seam_moved" and i == 1:           # the seam between chunks 0 and 1, one latent later: chunk 0 is kept longer
            step = seam_step(chunk_in, chunk_out)
            y[:, :, lo:lo + step] = prev[:, :, prev_b:prev_b + step]
            lo, a = lo + step, a + step
        if defect == "keep_from_off_by_one" and i == 1:  # the kept part of chunk 1 is read one output later
            a, b = a + 1, min(b + 1, yc.shape[2])
            hi = lo + (b - a)
        y[:, :, lo:hi] = yc[:, :, a:b]
        seams |= {lo, hi}
        prev, prev_b = yc, b
    return y, sorted(s for s in seams if 0 < s < total_out)


def seam_step(chunk_in, chunk_out):
    """one latent in output positions: the ratio for a decode (40 outputs per latent), 1 for an encode"""
    return max(1, chunk_out // chunk_in)


def chunk_inputs(c, direction):
    mk = lambda n, shape, sc=1.0: torch.from_numpy(gu.make_input(n, shape, c["seed"] + 50, sc))   # noqa: E731
    if direction == "decode":
        return mk("zc", (c["B"], c["lat"], CHUNK_LATENTS))
    return mk("wavc", (c["B"], c["audio"], CHUNK_LATENTS * c["ratio"]), 0.5)


def _chunk_reference(c, direction, size, overlap, mode, draw, defect):
    dtype = F64 if mode == "f64" else F32
    run = None if mode == "f64" else _Run(c, mode, draw)
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in state(c).items()}
    x = chunk_inputs(c, direction).to(dtype).requires_grad_(True)
    r = c["ratio"]
    with (run.installed() if run is not None else contextlib.nullcontext()):
        if direction == "decode":
            y, seams = chunked(lambda t: _decode(run, sd, c, t), x, size, size - overlap, lambda s: s * r, size * r, x.shape[2] * r,
                               (overlap // 2) * r, defect)
        else:
            y, seams = chunked(lambda t: _encode(sd, c, t), x, size * r, (size - overlap) * r, lambda s: s // r, size, x.shape[2] // r,
                               overlap // 2, defect)
        (y * cotangent(c, "dy_" + direction, y.shape).to(dtype)).sum().backward()
    return {"chunk:y": y.detach(), "chunk:dx": x.grad}, {"chunk:y": seams, "chunk:dx": [to_in(s, direction, r) for s in seams]}


def to_in(s, direction, r):
    return s // r if direction == "decode" else s * r


@functools.lru_cache(maxsize=None)
def chunk_reference(i, mode="f64", draw=0, defect=None):
    """({"chunk:y", "chunk:dx"}, seams per name) of CHUNKED[i]: the chunked output and the gradient of its input under
    (y * dy).sum(); the input gradient is cut where the seams fall in the input"""
    return _chunk_reference(dict(CASES[CHUNK_CASE]), *CHUNKED[i], mode, draw, defect)


@functools.lru_cache(maxsize=None)
def chunk_yardstick(i):
    ref, seams = chunk_reference(i)
    return yardstick_of(ref, [chunk_reference(i, "emu", d)[0] for d in range(DRAWS)], seams)


# ------------------------------------------------------------------------------------------------ mel-VAE (forward only)
MELVAE_CASES = {
    "amp1_causal": dict(h=gu.MELVAE_CONFIGS["amp1_causal"], samples=256, B=2, seed=911, frames=None),
    "amp2_same": dict(h=gu.MELVAE_CONFIGS["amp2_same"], samples=256, B=2, seed=912, frames=None),
    # odd up-sampling rates (5, 3), 173 latent frames: lengths no tile divides
    "up5x3": dict(h=dict(latent_dim=8, use_vae=True, downsample_channels=[12, 16, 24], downsample_rates=[3, 5], upsample_rates=[5, 3],
                         upsample_kernel_sizes=[10, 6], upsample_initial_channel=24, resblock="1", resblock_kernel_sizes=[3, 5],
                         resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]], activation="snakebeta", snake_logscale=True, causal=False,
                         flow_hidden_channels=8), samples=173 * 15, B=2, seed=913, frames=173),
}


def melvae_module(cid):
    """the drop-in module of a case on the CPU (its parameters name the state; nothing runs on it here)"""
    from kalle_audio_amd.flows import BigVGANFlowVAE
    return BigVGANFlowVAE(MELVAE_CASES[cid]["h"])


@functools.lru_cache(maxsize=None)
def melvae_state(cid):
    c = MELVAE_CASES[cid]
    return gu.make_state([(n, tuple(p.shape)) for n, p in melvae_module(cid).named_parameters()], c["seed"])


def melvae_inputs(cid):
    c = MELVAE_CASES[cid]
    wav = torch.from_numpy(gu.make_input("wav", (c["B"], 1, c["samples"]), c["seed"], 0.5))
    with torch.no_grad():
        sd = {k: torch.from_numpy(v) for k, v in melvae_state(cid).items()}
        T = ko.melvae_encoder(ko._sub(sd, "audio_encoder."), wav, c["h"]["downsample_rates"]).shape[2]
    lat = c["h"]["latent_dim"]
    return dict(wav=wav, eps=torch.from_numpy(gu.make_input("eps", (c["B"], lat, T), c["seed"])),
                z=torch.from_numpy(gu.make_input("zz", (c["B"], lat, c["frames"] or T), c["seed"])))


@functools.lru_cache(maxsize=None)
def melvae_reference(cid, mode="f64", draw=0):
    """"mel:latents" (extract_latents), "mel:rec" / "mel:z_p" / "mel:logs_q" (forward(wav, eps)), "mel:dec" (inference_from_latents)"""
    c = MELVAE_CASES[cid]
    dtype = F64 if mode == "f64" else F32
    run = None if mode == "f64" else _Run(dict(seed=c["seed"]), mode, draw)
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in melvae_state(cid).items()}
    inp = {k: v.to(dtype) for k, v in melvae_inputs(cid).items()}
    with torch.no_grad(), (run.installed(melvae=True) if run is not None else contextlib.nullcontext()):
        out = {"mel:latents": ko.melvae_encoder(ko._sub(sd, "audio_encoder."), inp["wav"], c["h"]["downsample_rates"])}
        out["mel:rec"], out["mel:z_p"], out["mel:logs_q"] = ko.melvae_forward(sd, inp["wav"], inp["eps"], c["h"])
        out["mel:dec"] = ko.melvae_decode(sd, inp["z"], c["h"])
    return out


@functools.lru_cache(maxsize=None)
def melvae_yardstick(cid):
    return yardstick_of(melvae_reference(cid), [melvae_reference(cid, "emu", d) for d in range(DRAWS)])
