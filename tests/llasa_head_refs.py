"""float64 reference of the per-frame head of KV-cached generation (kalle_llasa_frame_head_rows; model_sigmaVAE.py:123-146),
stage by stage, with the three bf16 roundings of the kernel sequence at the points the header states - bf16(rmsnorm(h)),
bf16(gelu(h1)), bf16(latent) - or without them (round_points=False: the plain mathematics, what the CPU test holds against
nn.Linear / nn.GELU / torch.distributions).  All tensors float64, rows first: h [R, D], noise [R, dl]."""
import math

import torch


def bf16r(t):
    """rounded once to bf16 (nearest even), promoted to float64"""
    return t.to(torch.bfloat16).double()


def rms(h, gamma, eps, wrong=None):
    """h * (gamma * rsqrt(mean(h^2) + eps)) per row, not yet rounded (LlamaRMSNorm)"""
    rr = (h.pow(2).mean(-1, keepdim=True) + (0.0 if wrong == "no_eps" else eps)).rsqrt()
    return h * (gamma * rr)


def linear(W, x, b=None):
    """x [R, K] against W [N, K] (+ b [N]); also returns sum_k |W_nk| |x_rk|, the magnitude the fp32 dot is bounded by"""
    y, mag = x @ W.T, x.abs() @ W.abs().T
    return (y if b is None else y + b), mag


def gelu(x, wrong=None):
    """exact GELU, the cancelling side through erfc; wrong="tanh": the tanh approximation"""
    if wrong == "tanh":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def kl_terms(mean, std, wrong=None):
    """the dl terms of KL(N(mean, std) || N(1, e)) (model_sigmaVAE.py:135-139) and the sum of the magnitudes that enter each"""
    e = math.e
    c0 = math.log(e / std)
    d2 = mean ** 2 if wrong == "kl_vs_n01" else (mean - 1.0) ** 2
    s2 = 0.0 if wrong == "no_std2" else std * std
    half = 0.0 if wrong == "no_half" else 0.5
    if wrong == "kl_vs_n01":                       # KL(N(m, s) || N(0, 1))
        return math.log(1.0 / std) + (s2 + d2) / 2.0 - half, None
    return c0 + (s2 + d2) / (2.0 * e * e) - half, abs(c0) + (s2 + d2) / (2.0 * e * e) + 0.5


def kl(mean, std, wrong=None):
    return kl_terms(mean, std, wrong)[0].mean(-1)


def head(h, norm, w1, b1, w2, b2, wa, ba, noise, std, eps, round_points=True):
    """every stage of the head for the rows of h, each from the stage before it"""
    r = bf16r if round_points else (lambda t: t)
    s = {}
    s["xn"] = r(rms(h, norm, eps))
    s["h1"] = linear(w1, s["xn"], b1)[0]
    s["a"] = r(gelu(s["h1"]))
    s["mean"] = linear(w2, s["a"], b2)[0]
    s["latent"] = s["mean"] + std * noise
    s["lat"] = r(s["latent"])
    s["kl"] = kl(s["mean"], std)
    s["x_next"] = linear(wa, s["lat"], ba)[0]
    return s
