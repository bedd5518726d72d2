"""Llasa over a head-dim-128 Llama: the REFERENCE implementation (model_sigmaVAE.Llasa imported in place, CPU fp32,
use_flash_attention=False) over a tiny locally built `transformers` Llama with the head layout of Llama-3.2-3B / Llama-3.1-8B
(head_dim 128, rotary over the whole head with partners 64 apart, GQA 2:1) - hidden 256, 2 heads, 1 kv head, inner 512, 2
layers; everything else as golden_util.LLASA_WIDE_CONFIG["llama"] (llama3 rope scaling active at these lengths, tied embeddings).

Writes llasa_hd128.npz (losses, pre_mean, sampled latents, digests of every parameter gradient, four gradients in full: these
as float16 of grad * gradscale, gradscale the power of two that brings the largest element into [0.5, 1), so that the file
stays at half the size and every element within 2^-14 of the largest keeps 11 bits) and state_dict_keys_llama_hd128.json (the reference's key -> shape inventory).  Weights are rebuilt from the seed on both sides
(golden_util.make_state) and not stored.  Runs only in the build container.  Writes data only.
Usage: python tests/golden/make_golden_llama_hd128.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import golden_util as gu  # noqa: E402
import make_golden as mg  # noqa: E402
from make_golden import T, grads, load_seeded, pack_grads, save  # noqa: E402

SEED = 140
FULL = ("base_model.model.layers.1.self_attn.k_proj.weight", "base_model.model.layers.0.self_attn.o_proj.weight",
        "base_model.model.layers.1.mlp.gate_proj.weight", "base_model.model.layers.0.post_attention_layernorm.weight")


def config():
    """the fixture's config: LLASA_WIDE_CONFIG with 2 heads of 128 over 1 kv head"""
    lc = dict(gu.LLASA_WIDE_CONFIG)
    lc["llama"] = dict(lc["llama"], hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                       intermediate_size=512, num_hidden_layers=2)
    return lc


def main():
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for stub in ("torchaudio", "torchaudio.transforms"):   # the empty stubs confuse transformers' availability probes
        sys.modules.pop(stub, None)
    from transformers import LlamaConfig, LlamaForCausalLM
    import model_sigmaVAE as rl
    lc = config()
    tmp = tempfile.mkdtemp(prefix="kalle_llama_hd128_")
    LlamaForCausalLM(LlamaConfig(**lc["llama"])).save_pretrained(tmp)

    class _Tok:
        def __len__(self):
            return lc["tokenizer_len"]

    llasa = rl.Llasa({"llm_model_name_or_path": tmp, "latent_dim": lc["latent_dim"], "audio_proj_dim": lc["llama"]["hidden_size"]},
                     _Tok(), use_flash_attention=False)
    load_seeded(llasa, SEED)
    inv = {k: list(v.shape) for k, v in llasa.state_dict().items()}
    batch = gu.llasa_batch(lc, SEED, B=3, L=40)
    tb = {k: T(v) for k, v in batch.items()}
    eps = T(gu.make_input("llasa_eps", batch["audio_latents"].shape, SEED))
    orig = torch.randn_like
    torch.randn_like = lambda t, **k: eps
    try:
        out = llasa(tb["input_ids"], tb["audio_latents"], tb["audio_distribution_l"], tb["ids_mask"], tb["audio_mask"],
                    tb["target_mask"], tb["end_mask"])
    finally:
        torch.randn_like = orig
    (out["audio_loss"] * 1.0 + out["end_loss"] * 0.5).backward()
    g = grads(llasa)
    full = {}
    for k in FULL:
        scale = 2.0 ** -np.ceil(np.log2(np.abs(g[k]).max()))
        full[f"grad/{k}"] = (g[k] * scale).astype(np.float16)
        full[f"gradscale/{k}"] = np.float64(scale)
    save("llasa_hd128", audio_loss=out["audio_loss"], end_loss=out["end_loss"], pre_mean=out["pre_mean"],
         sampled=out["ground_truth_audio_latents"], **pack_grads("", g), **full)
    with open(os.path.join(HERE, "state_dict_keys_llama_hd128.json"), "w") as f:
        json.dump({"llasa": inv}, f, indent=0, sort_keys=True)
    print("done")


if __name__ == "__main__":
    main()
