"""generate_diffusion_cond (stable_audio_tools/inference/generation.py:90-250) for the DiT + the in-tree samplers this
build carries: seed -> noise (138-142: torch.manual_seed(seed); randn on `device`) -> conditioning inputs (150-162) ->
sampler with batched CFG (221-234) -> pretransform.decode (244-247).

Objectives: "rectified_flow" runs sample_rf -> sample_discrete_euler exactly as the reference (sampling.py:200-232);
"v" is routed by the reference to third-party k-diffusion (`sample_k`, absent here) - this build runs the in-tree v-DDIM
sampler instead (sampling.py:47-86, the call the reference keeps commented out at generation.py:236).

init_audio / mask_args (generation.py:164-224): carried over for rectified flow exactly as the reference runs them -
variations start from `init (1 - sigma_max) + noise sigma_max` with sigma_max = init_noise_level (sampling.py:200-232); with
mask_args the reference cuts / pastes the init audio and builds the soft mask but its rectified-flow branch hands neither the
mask nor a sigma_max to sample_rf, so the call degenerates to plain sampling (pinned by tests/golden/generate_init_audio.npz).
For the "v" objective both live in k-diffusion and are refused."""
import math
import os

import numpy as np
import torch

from .sampling import sample, sample_discrete_euler, sample_rf
from .utils import prepare_audio


def build_mask(sample_size, mask_args):
    """generation.py:254-274: soft mask (0 = fresh generation, 1 = keep the input) with Hann ramps"""
    maskstart = math.floor(mask_args["maskstart"] / 100.0 * sample_size)
    maskend = math.ceil(mask_args["maskend"] / 100.0 * sample_size)
    softnessL = round(mask_args["softnessL"] / 100.0 * sample_size)
    softnessR = round(mask_args["softnessR"] / 100.0 * sample_size)
    marination = mask_args["marination"]
    hannL = torch.hann_window(softnessL * 2, periodic=False)[:softnessL]
    hannR = torch.hann_window(softnessR * 2, periodic=False)[softnessR:]
    mask = torch.zeros((sample_size))
    mask[maskstart:maskend] = 1
    mask[maskstart:maskstart + softnessL] = hannL
    mask[maskend - softnessR:maskend] = hannR
    if marination > 0:
        mask = mask * (1 - marination)
    return mask


def generate_diffusion_cond(model, steps: int = 250, cfg_scale=6, conditioning: dict = None, conditioning_tensors=None,
                            negative_conditioning: dict = None, negative_conditioning_tensors=None, batch_size: int = 1,
                            sample_size: int = 2097152, sample_rate: int = 48000, seed: int = -1, device: str = "cuda",
                            init_audio=None, init_noise_level: float = 1.0, mask_args: dict = None, return_latents=False,
                            eta=0.0, **sampler_kwargs):
    if init_audio is not None and model.diffusion_objective != "rectified_flow":
        raise NotImplementedError("generate_diffusion_cond(init_audio) for the v objective runs inside third-party k-diffusion "
                                  "(sample_k) in the reference; only the rectified-flow branch is in its tree")
    audio_sample_size = sample_size
    if model.pretransform is not None:
        sample_size = sample_size // model.pretransform.downsampling_ratio
    seed = seed if seed != -1 else np.random.randint(0, 2 ** 32 - 1, dtype=np.uint32)
    torch.manual_seed(int(seed))
    # the initial noise immediately after the seed (generation.py:141-142).  `device` is where the reference draws it; the
    # kernels run on the model's device, so a CPU draw (bit-identical to the reference's CPU draw) is moved over.
    model_device = next(model.model.parameters()).device
    noise = torch.randn([batch_size, model.io_channels, sample_size], device=device).to(model_device)
    assert conditioning is not None or conditioning_tensors is not None, \
        "Must provide either conditioning or conditioning_tensors"
    if conditioning_tensors is None:
        conditioning_tensors = model.conditioner(conditioning, model_device)
    cond_inputs = model.get_conditioning_inputs(conditioning_tensors)
    if negative_conditioning is not None or negative_conditioning_tensors is not None:
        if negative_conditioning_tensors is None:
            negative_conditioning_tensors = model.conditioner(negative_conditioning, model_device)
        neg = model.get_conditioning_inputs(negative_conditioning_tensors, negative=True)
    else:
        neg = {}
    init_data = None
    if init_audio is not None:                                       # generation.py:164-183
        in_sr, init_audio = init_audio
        io_channels = model.pretransform.io_channels if model.pretransform is not None else model.io_channels
        init_data = prepare_audio(init_audio, in_sr=in_sr, target_sr=model.sample_rate, target_length=audio_sample_size,
                                  target_channels=io_channels, device=model_device)
        if model.pretransform is not None:
            init_data = model.pretransform.encode(init_data)
        init_data = init_data.repeat(batch_size, 1, 1)
        if mask_args is not None:                                    # 186-214 (the mask is built and, as there, not used)
            cropfrom = math.floor(mask_args["cropfrom"] / 100.0 * sample_size)
            pastefrom = math.floor(mask_args["pastefrom"] / 100.0 * sample_size)
            pasteto = math.ceil(mask_args["pasteto"] / 100.0 * sample_size)
            assert pastefrom < pasteto, "Paste From should be less than Paste To"
            croplen = pasteto - pastefrom
            if cropfrom + croplen > sample_size:
                croplen = sample_size - cropfrom
            cutpaste = init_data.new_zeros(init_data.shape)
            cutpaste[:, :, pastefrom:pastefrom + croplen] = init_data[:, :, cropfrom:cropfrom + croplen]
            init_data = cutpaste
            build_mask(sample_size, mask_args)
        else:
            sampler_kwargs["sigma_max"] = init_noise_level           # 215-218: variations
    for k in ("sigma_min", "sampler_type", "rho") + (() if init_data is not None else ("sigma_max",)):
        sampler_kwargs.pop(k, None)                                  # k-diffusion knobs of the reference's call sites
    # One sampler step is ~400 launches that take less GPU time than the host needs to issue them: the denoiser call is captured
    # into a HIP graph once per shape signature and replayed (kalle_audio_amd/graph.py; bit-identical to the eager launches;
    # KALLE_SAMPLE_GRAPH=0 keeps the eager path).  Only frozen models: a captured graph does not see parameter updates' new
    # bf16 copies.  "Frozen" is requires_grad=False, not immutable - load_state_dict of the next checkpoint changes the weights
    # in place, and a re-cast bf16 copy lives at a new address: the captured graphs are dropped whenever the weights' key
    # (ops.weights_key: every parameter's identity, version, address, device and dtype + the write epoch) has moved.  An EMA
    # swap as ema_pytorch does it (`.data.copy_` / `.data.lerp_`) moves none of these: the caller follows it with
    # kalle_audio_amd.weights_changed(), which moves the epoch ("Weight-derived caches", rule d).
    denoiser = model.model
    frozen = not any(p.requires_grad for p in denoiser.parameters())
    if steps >= 4 and frozen and os.environ.get("KALLE_SAMPLE_GRAPH", "1") != "0":     # (the samplers run under no_grad)
        from ... import ops
        from ...graph import GraphedForward
        ps = list(denoiser.parameters())
        fp = ops.weights_key(*ps)
        g = getattr(model, "_kalle_graphed", None)
        if g is None or g.fn is not denoiser or getattr(g, "weights_fingerprint", None) != fp:
            g = GraphedForward(denoiser)
            g.weights_fingerprint, g.weights_pin = fp, ops.weights_pin(*ps)
            object.__setattr__(model, "_kalle_graphed", g)      # (not a submodule: keeps it out of state_dict / parameters)
        denoiser = g
    # the conditioning is the same at every sampler step: project it ONCE (cond | uncond halves, to_cond_embed, to_global_embed,
    # the cross-attention k | v of all layers) instead of once per step - same arithmetic, hoisted out of the loop
    # (KALLE_SAMPLE_PRECOND=0 keeps it inside)
    dit = getattr(model.model, "model", None)
    if frozen and os.environ.get("KALLE_SAMPLE_PRECOND", "1") != "0" and hasattr(dit, "precompute_conditioning"):
        pre = dit.precompute_conditioning(cross_attn_cond=cond_inputs.get("cross_attn_cond"),
                                          negative_cross_attn_cond=neg.get("negative_cross_attn_cond"),
                                          negative_cross_attn_mask=neg.get("negative_cross_attn_mask"),
                                          global_embed=cond_inputs.get("global_cond"),
                                          prepend_cond=cond_inputs.get("prepend_cond"), cfg_scale=cfg_scale)
        sampler_kwargs.update(pre)
    if model.diffusion_objective == "v":
        sampled = sample(denoiser, noise, steps, eta, **cond_inputs, **neg, cfg_scale=cfg_scale, batch_cfg=True,
                         rescale_cfg=True, **sampler_kwargs)
    elif model.diffusion_objective == "rectified_flow":
        if init_data is not None:
            sampled = sample_rf(denoiser, noise, init_data=init_data.to(noise.dtype), steps=steps, **sampler_kwargs,
                                **cond_inputs, **neg, cfg_scale=cfg_scale, batch_cfg=True, rescale_cfg=True)
        else:
            sampled = sample_discrete_euler(denoiser, noise, steps, **cond_inputs, **neg, cfg_scale=cfg_scale,
                                            batch_cfg=True, rescale_cfg=True, **sampler_kwargs)
    else:
        raise ValueError(f"unknown diffusion objective {model.diffusion_objective!r}")
    if model.pretransform is not None and not return_latents:
        sampled = model.pretransform.decode(sampled.float())
    return sampled
