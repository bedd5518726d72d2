"""Ragged batches through the Oobleck stacks, held to the fp64 oracle ROW BY ROW: the per-slice method of tests/vae_oracle.py
(runs of 16 positions, the bound M x r, its emulation - all imported) with each sequence run ALONE as the reference and as the
yardstick's source.  Pure torch on the CPU; shared by tests/test_conv_lens_cpu.py (the definition and the sensitivity, on the
reference alone) and tests/test_vae_ragged_gpu.py (the HIP path).

Cases      O1, O2, O3, O4, O5, O7 of vae_oracle.CASES: snake / ELU, odd stride, trailing inputs, deepest length under the
           dilation-9 pad, nearest up-sampling, bf16 (O6 is the anti-aliased activation, which refuses lengths).
Inputs     decode: five latents of T = 1, 2, 5, 17, 33 frames; encode (cases with an encoder): four clips of 2, 3 r + 1, 6 r and
           9 r + r // 2 + 1 samples (r the down-sampling ratio): two of them no multiple of it.  Seeded, as vae_oracle.inputs.
Reference  ko.oobleck_decoder / ko.oobleck_encoder in fp64 on ONE sequence, nothing replaced.
Yardstick  per row: the largest slice ratio of vae_oracle's fp32 emulation of that row alone over vae_oracle.DRAWS draws, floored
           at the median over the rows of the case (vae_oracle.yardstick_of).  Nothing of it comes from a batch.
Masked     `masked(...)`: the stack on the zero-padded BATCH with every layer's output cut to its rows' lengths - each from the
           layer's own length formula per row.  This is the definition the device implements; in fp64 it equals the rows run
           alone to rounding (test_conv_lens_cpu.py).
Defects    seeded into `masked`, one at a time; the device's tensors must fail each:
             padded     no lengths at all: the zero-padded dense batch (the only substitute the code had)
             neighbour  every row gets the length of the next row
             unscaled   after the first up-sampling (down-sampling) block the input-rate lengths are kept unscaled
             k1_open    the k = 1 conv of the second residual unit stores past its rows' lengths (bias leaks into the next conv)
Shown      a defect counts as shown when the defective reference lies 2 M r or more from the clean one on some slice of some row:
           a device tensor inside M r of the clean reference is then M r or more from the defective one on that slice (triangle
           inequality on the slice norm), so "the device fails the defect" cannot hinge on the device's own noise.
BLIND      (direction, case, defect) triples under that 2 M, asserted blind in tests/test_conv_lens_cpu.py: the bf16 case stores
           8 bits (r about 1e-2), and the bias of one k = 1 conv leaking through one k = 7 conv moves a slice by 0.9 r (encode)
           to 4.4 r (decode)."""
import contextlib
import functools

import torch
import torch.nn.functional as TF

import vae_oracle as vo

gu, ko = vo.gu, vo.ko
F64, F32, BF16 = vo.F64, vo.F32, vo.BF16
CIDS = ["O1", "O2", "O3", "O4", "O5", "O7"]
ENC_CIDS = [k for k in CIDS if vo.CASES[k]["encoder"]]
DEC_T = (1, 2, 5, 17, 33)
DEFECTS = ["padded", "neighbour", "unscaled", "k1_open"]
BLIND = {("decode", "O7", "k1_open"), ("encode", "O7", "k1_open")}
SHOWN = 2 * vo.M


def enc_lengths(c):
    r = c["ratio"]
    return (2 * r, 3 * r + 1, 6 * r, 9 * r + r // 2 + 1)


def lengths(cid, direction):
    return DEC_T if direction == "decode" else enc_lengths(vo.CASES[cid])


def rows(cid, direction):
    """the sequences, each [1, C, L_i] fp32 (bf16 values in a bf16 case)"""
    c = vo.CASES[cid]
    C, sc, tag = (c["lat"], 1.0, "rz") if direction == "decode" else (c["audio"], 0.5, "rw")
    out = []
    for i, L in enumerate(lengths(cid, direction)):
        t = torch.from_numpy(gu.make_input(f"{tag}{i}", (1, C, L), c["seed"], sc))
        out.append(t.to(BF16).float() if c["bf16"] else t)
    return out


def padded(cid, direction):
    """([B, C, Lmax] zero-padded, lengths)"""
    rs = rows(cid, direction)
    L = [t.shape[2] for t in rs]
    x = torch.zeros(len(rs), rs[0].shape[1], max(L))
    for b, t in enumerate(rs):
        x[b, :, :L[b]] = t[0]
    return x, L


def _sd(c, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in vo.state(c).items()}


def _stack(run, sd, c, x, direction):
    if direction == "decode":
        return vo._decode(run, sd, c, x)
    return vo._encode(sd, c, x)


@functools.lru_cache(maxsize=None)
def alone(cid, direction, mode="f64", draw=0):
    """every row through the stack ALONE: tuple of [1, C, L_out_i]"""
    c = vo.CASES[cid]
    dtype = F64 if mode == "f64" else F32
    sd = _sd(c, dtype)
    out = []
    for x in rows(cid, direction):
        run = None if mode == "f64" else vo._Run(c, mode, draw)
        with (run.installed() if run is not None else contextlib.nullcontext()), torch.no_grad():
            out.append(_stack(run, sd, c, x.to(dtype), direction))
    return tuple(out)


def named(ts):
    return {f"row:{i}": t for i, t in enumerate(ts)}


@functools.lru_cache(maxsize=None)
def yardstick(cid, direction):
    """(r, raw) per row, from the rows alone"""
    return vo.yardstick_of(named(alone(cid, direction)), [named(alone(cid, direction, "emu", d)) for d in range(vo.DRAWS)])


def rho(got_rows, cid, direction, ref_rows=None):
    """name -> worst slice ratio / r of each row (got_rows: list of [1, C, L_out_i])"""
    ref = named(alone(cid, direction) if ref_rows is None else ref_rows)
    return vo.rho_of(named(got_rows), ref, yardstick(cid, direction)[0])


# ------------------------------------------------------------------------------------------------ the masked stack (the definition)
class _Masked:
    """ko.F for one pass over a zero-padded batch: every conv's output is cut to its rows' lengths, each from the layer's own
    formula applied to the row's input length.  The lengths travel with the pass (`lens`, at the resolution `Lmax`)."""

    def __init__(self, lens, Lmax, defect=None):
        self.lens, self.Lmax, self.defect = [int(v) for v in lens], Lmax, defect
        if defect == "neighbour":
            self.lens = self.lens[1:] + self.lens[:1]
        self.pads = (0, 0)
        self.resamplings = 0
        self.k1 = 0

    def _mask(self, y, lens):
        if self.defect == "padded":
            return y
        pos = torch.arange(y.shape[2])[None, None, :]
        return y * (pos < torch.tensor(lens)[:, None, None]).to(y.dtype)

    def _lens_in(self, L):
        """the rows' lengths at a tensor of L positions: the current ones, or (behind sample repetition) a multiple of them"""
        if L == self.Lmax:
            return self.lens
        assert L % self.Lmax == 0, (L, self.Lmax)
        return [v * (L // self.Lmax) for v in self.lens]

    def _set(self, lens_in, lens_out, y, resampled):
        if resampled:
            self.resamplings += 1
            if self.defect == "unscaled" and self.resamplings == 1:
                lens_out = [min(v, y.shape[2]) for v in self.lens]     # (the lengths before the block, repetition included)
        self.lens, self.Lmax = lens_out, y.shape[2]
        return lens_out

    def pad(self, x, pads, mode="constant", value=None):
        self.pads = tuple(pads)
        return TF.pad(x, pads, mode, value)

    def conv1d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        K = w.shape[2]
        pl, pr = self.pads
        self.pads = (0, 0)
        lens_in = self._lens_in(x.shape[2] - pl - pr)
        lens_out = [max(0, (v + pl + pr + 2 * padding - dilation * (K - 1) - 1) // stride + 1) if v > 0 else 0 for v in lens_in]
        y = TF.conv1d(x, w, b, stride, padding, dilation, groups)
        resampled = stride > 1 or x.shape[2] - pl - pr != self.Lmax
        if K == 1:
            self.k1 += 1
            if self.defect == "k1_open" and self.k1 == 2:
                self._set(lens_in, lens_out, y, resampled)
                return y
        return self._mask(y, self._set(lens_in, lens_out, y, resampled))

    def conv_transpose1d(self, x, w, b=None, stride=1, padding=0, groups=1):
        K = w.shape[2]
        lens_in = self._lens_in(x.shape[2])
        lens_out = [(v - 1) * stride - 2 * padding + K if v > 0 else 0 for v in lens_in]
        y = TF.conv_transpose1d(x, w, b, stride, padding, groups=groups)
        return self._mask(y, self._set(lens_in, lens_out, y, True))

    def __getattr__(self, name):
        return getattr(TF, name)


def masked(cid, direction, defect=None, dtype=F64):
    """the batch through the masked stack: list of rows [1, C, L_out_i] (each cut to the length the row has ALONE, so a defect that
    changes a length is compared over the true one)"""
    c = vo.CASES[cid]
    x, L = padded(cid, direction)
    sd = _sd(c, dtype)
    m = _Masked(L, x.shape[2], defect)
    orig = ko.F
    ko.F = m
    try:
        with torch.no_grad():
            y = _stack(None, sd, c, x.to(dtype), direction)
    finally:
        ko.F = orig
    out = []
    for b, ref in enumerate(alone(cid, direction)):
        n = ref.shape[2]
        row = y[b:b + 1, :, :n]
        out.append(TF.pad(row, (0, n - row.shape[2])) if row.shape[2] < n else row)
    return out
