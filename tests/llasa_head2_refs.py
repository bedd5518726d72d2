"""float64 reference of the per-frame head of model.Llasa's KV-cached generation (kalle_llasa_frame_head2_rows; model.py:109-150),
stage by stage, with the three bf16 roundings of the kernel sequence at the points the header states - bf16(rmsnorm(h)),
bf16(gelu(h1)), bf16(latent) - or without them (round_points=False: the plain mathematics, what the CPU test holds against
nn.Linear / nn.GELU / torch.distributions).  All tensors float64, rows first: h [R, D], noise [R, lat]; disp = mean || logs.
The stages this head shares with the fixed-std one (rms, linear, gelu, bf16r) are those of tests/llasa_head_refs.py."""
import math

import torch

from llasa_head_refs import bf16r, gelu, linear, rms  # noqa: F401


def halves(disp, wrong=None):
    """(mean, logs) of disp [..., 2 lat]; wrong="swapped": the halves exchanged"""
    lat = disp.shape[-1] // 2
    mean, logs = disp[..., :lat], disp[..., lat:]
    return (logs, mean) if wrong == "swapped" else (mean, logs)


def scale(logs, wrong=None):
    """s = exp(logs); wrong="fixed_std": the 0.5 of the fixed-std head"""
    return torch.full_like(logs, 0.5) if wrong == "fixed_std" else torch.exp(logs)


def kl_terms(mean, logs, s=None):
    """the lat terms of KL(N(mean, s) || N(1, e)) = log(e / s) + (s^2 + (mean - 1)^2) / (2 e^2) - 1/2 with log(e / s) = 1 - logs
    (model.py:133-136), and the sum of the magnitudes that enter each.  s: exp(logs) unless given"""
    e = math.e
    s = torch.exp(logs) if s is None else s
    q = (s * s + (mean - 1.0) ** 2) / (2.0 * e * e)
    return (1.0 - logs) + q - 0.5, 1.0 + logs.abs() + q + 0.5


def kl(disp, wrong=None):
    """[R] from disp [R, 2 lat].  wrong: "swapped" (halves exchanged), "over_d2" (divided by 2 lat), "reversed" (KL(N(1, e) ||
    N(mean, s))), "fixed_std" (s = 0.5 in place of exp(logs))"""
    mean, logs = halves(disp, "swapped" if wrong == "swapped" else None)
    lat = mean.shape[-1]
    if wrong == "reversed":
        e = math.e
        s = torch.exp(logs)
        return ((logs - 1.0) + (e * e + (mean - 1.0) ** 2) / (2.0 * s * s) - 0.5).sum(-1) / lat
    if wrong == "fixed_std":
        return kl_terms(mean, torch.full_like(logs, math.log(0.5)))[0].sum(-1) / lat
    return kl_terms(mean, logs)[0].sum(-1) / (2 * lat if wrong == "over_d2" else lat)


def head(h, norm, w1, b1, w2, b2, wa, ba, noise, eps, round_points=True):
    """every stage of the head for the rows of h, each from the stage before it"""
    r = bf16r if round_points else (lambda t: t)
    s = {}
    s["xn"] = r(rms(h, norm, eps))
    s["h1"] = linear(w1, s["xn"], b1)[0]
    s["a"] = r(gelu(s["h1"]))
    s["disp"] = linear(w2, s["a"], b2)[0]
    mean, logs = halves(s["disp"])
    s["s"] = scale(logs)
    s["latent"] = mean + s["s"] * noise
    s["lat"] = r(s["latent"])
    s["kl"] = kl(s["disp"])
    s["x_next"] = linear(wa, s["lat"], ba)[0]
    return s
