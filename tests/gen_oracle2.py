"""The generation oracle of tests/gen_oracle.py for model.Llasa, whose head predicts mean || log-scale and samples
mean + exp(log_scale) noise (model.py:109-150).  Pure torch on the CPU; shared by tests/test_gen_oracle2_cpu.py and
tests/test_model_llasa_gen_oracle_gpu.py.  Everything head-agnostic is gen_oracle's own: the decoder rows and their e4m3
positions, `ratios` / `worst` / `failure`, the prompts, the sensitive gains, the output defects.  Here is only what that file
hard-wires to the fixed-std head:

State      gen_oracle.make_state with distribution_linear redrawn at this class's shapes ([2 lat, D], [2 lat, 2 lat]).
Reference  gen_oracle.row_forward already runs the head as two linears around a GELU; with this state its "mean" IS disp
           (mean || log-scale, what `infer` returns per frame).  It is renamed and the frame KL is llasa_head2_refs.kl.
           Teacher forced on the latents the path itself produced (the sampled latent of every frame, captured where the path
           feeds it to audio_linear): every frame is compared on identical inputs.
Quantities pre, hidden, disp.
Free run   latent_i = mean_i + exp(logs_i) noise_i fed back; wrong="fixed_std" feeds mean_i + 0.5 noise_i, the other class's rule.
Stop rule  kl_allowance and stop_plan below: the allowance of the two-parameter KL, and a threshold judged on the frames the
           rule actually reads."""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_oracle as go  # noqa: E402
import llasa_head2_refs as hr2  # noqa: E402

gs, gu, ko = go.gs, go.gu, go.ko
F64, M = go.F64, go.M
CASES, FMTS, fmt_id = go.CASES, go.FMTS, go.fmt_id
QUANTITIES = ("pre", "hidden", "disp")


def make_state(c, gains="sensitive"):
    st = go.make_state(c, gains)
    hid, d2 = c["hd"] * c["H"], 2 * c["lat"]
    st.update(gu.make_state([("distribution_linear.0.bias", (d2,)), ("distribution_linear.0.weight", (d2, hid)),
                             ("distribution_linear.2.bias", (d2,)), ("distribution_linear.2.weight", (d2, d2))], c["seed"]))
    return st


def row_forward(c, W, row, mode="f64", positions=None, allow=None):
    """gen_oracle.row_forward with the head read as mean || log-scale: dict(pre, hidden [L, D], disp [L - P + 1, 2 lat],
    kl [L - P + 1], P=, L=)"""
    o = go.row_forward(c, W, row, mode, positions, allow)
    o["disp"] = o.pop("mean")
    assert o["disp"].shape[1] == 2 * c["lat"]
    o["kl"] = hr2.kl(o["disp"])
    return o


def forward(c, W, rows, mode="f64"):
    return [row_forward(c, W, row, mode) for row in rows]


def defect_forward(c, W, row, kind):
    o = go.defect_forward(c, W, row, kind)
    o["disp"] = o.pop("mean")
    o["kl"] = hr2.kl(o["disp"])
    return o


def frames_of(o, q):
    """quantity q of a row_forward result at the positions generation reads: the frames, position P - 1 on"""
    return o[q] if q == "disp" else o[q][o["P"] - 1:]


def yardstick(emu, f64, cut=lambda x: x):
    """r per quantity over the frame positions: emu against f64"""
    return {q: go.worst([cut(frames_of(o, q)) for o in emu], [cut(frames_of(o, q)) for o in f64])[0] for q in QUANTITIES}


def swap_halves(xs):
    """mean and log-scale exchanged in every disp row"""
    return [torch.cat([x[:, x.shape[1] // 2:], x[:, :x.shape[1] // 2]], 1) for x in xs]


def sample(disp, noise, wrong=None):
    """the latent a frame feeds back, rounded to fp32 as the path holds it"""
    mean, logs = hr2.halves(disp)
    return (mean + hr2.scale(logs, wrong) * noise.to(F64)).float().double()


@torch.no_grad()
def free_run(c, W, prompts, noise, T, mode="emu", step_from=None, wrong=None):
    """autoregressive generation on the oracle.  noise [T, lat] (every row the same draw) or [T, R, lat].  Returns the latents
    per row [T, lat]."""
    out = []
    for r, (ids, lat) in enumerate(prompts):
        fed = torch.zeros(0, c["lat"], dtype=F64)
        for i in range(T):
            row = go.teacher_rows([(ids, lat)], [fed], None if step_from is None else [step_from[r]])[0]
            disp = row_forward(c, W, row, mode)["disp"][-1]
            nz = noise[i] if noise.dim() == 2 else noise[i, r]
            fed = torch.cat([fed, sample(disp, nz, wrong)[None]], 0)
        out.append(fed)
    return out


# ------------------------------------------------------------------------------------------------ the stop rule
# the architecture (index into CASES) and the seed of the fixed noise [T, lat], every row the same draw: of seeds 0 .. 59 on the
# three architectures the one that leaves the widest margin (stop_plan: 5.4 allowances over 21 frames read, rows returning 8 / 11 /
# 11 frames); 46 of the 180 leave less than 1
STOP_CASE, STOP_SEED, STOP_FRAMES = 2, 21, 12


STOP_PS = (1, 14, 33)         # prompt positions of the stop test's three rows (short: the seed search runs a free run per seed)


def stop_prompts(c):
    return go.ragged_prompts(c, STOP_PS, tag="stop2")


def stop_noise(c, frames=STOP_FRAMES, seed=STOP_SEED):
    return torch.randn(1, frames, c["lat"], generator=torch.Generator().manual_seed(seed))[0]


def kl_allowance(disp64, r):
    """the largest change of the frame KL that an error of M r on disp = mean || logs permits, per position.
    lat KL = sum_j [ (1 - l_j) + (exp(2 l_j) + (m_j - 1)^2) / (2 e^2) - 1/2 ].  The check bounds the error vector v = (dm, dl) of a
    position by |v|_2 <= d = M r max(|disp|, floor), the floor of gen_oracle.ratios.  Exactly,
      lat dKL = <g, v> + sum_j dm_j^2 / (2 e^2) + sum_j s_j^2 (exp(2 dl_j) - 1 - 2 dl_j) / (2 e^2),     s = exp(l),
      g = (dKL/dm, dKL/dl) lat = ((m - 1) / e^2, -1 + s^2 / e^2)            the first-order part: |<g, v>| <= |g| d (Cauchy-Schwarz)
      sum_j dm_j^2 <= d^2;   exp(x) - 1 - x <= x^2 exp(|x|) / 2 with |dl_j| <= d:  the last sum <= max_j s_j^2 exp(2 d) d^2 / e^2.
    New against the fixed-std head: the log-scale half of g - the KL now moves with an error in logs, through log(e / s) with
    weight 1 per element and through s^2 with a weight that grows with the predicted scale itself - and the last term."""
    x = disp64.to(F64)
    lat = x.shape[1] // 2
    m, l = x[:, :lat], x[:, lat:]
    nrm = x.norm(dim=1)
    d = M * r * torch.maximum(nrm, 0.25 * nrm.pow(2).mean().sqrt())
    s2 = torch.exp(2 * l)
    e2 = math.e ** 2
    g = torch.cat([(m - 1.0) / e2, s2 / e2 - 1.0], 1).norm(dim=1)
    return (g * d + d * d / (2 * e2) + s2.amax(dim=1) * torch.exp(2 * d) * d * d / e2) / lat


def stop_plan(kls, allow, first=4):
    """kls, allow: per row [T] (frame KLs in fp64 and their allowances).  The stop rule reads a row's KL at frames first .. its
    stop frame and nothing after it, so those are the frames that must be clear of the threshold.  Candidates: the midpoints
    between neighbouring sorted KLs of frames >= first.  Chosen: the one with the largest margin - the smallest
    |KL - threshold| / allowance over the frames the rule reads - among those that stop the rows at different frames.
    Returns dict(thres, margin, counts (frames returned per row: a row that stops at frame i returns i, one that never stops
    T - 1), read (frames compared with the threshold))"""
    v = torch.cat([k[first:] for k in kls]).sort().values
    best = None
    for t in ((v[1:] + v[:-1]) / 2).tolist():
        counts, margin, read = [], math.inf, 0
        for k, a in zip(kls, allow):
            hit = [j for j in range(first, len(k)) if k[j].item() < t]
            last = hit[0] if hit else len(k) - 1
            counts.append(last)
            margin = min(margin, float(((k[first:last + 1] - t).abs() / a[first:last + 1]).min()))
            read += last + 1 - first
        if min(counts) < max(counts) and (best is None or margin > best["margin"]):
            best = dict(thres=t, margin=margin, counts=counts, read=read)
    assert best is not None, "no threshold stops the rows at different frames"
    return best
