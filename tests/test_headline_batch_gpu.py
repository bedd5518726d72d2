"""-m gpu: the benchmark's train step at its own batch size, B = 256 DISTINCT clips (32 256 rows in every GEMM: the persistent
256 x 256 kernel, the grouped weight gradients with split K), checked per clip and per parameter tensor - so that corruption
limited to a few batch indices or to one matrix cannot average away.

Forward: each clip of the B = 256 output against a B = 1 forward of that clip (126 rows: the small-tile and few-rows plans, other
kernels), and clips 0, 127, 128 and 255 against the CPU oracle (cosine >= 0.999 as in SURVEY 8c, rel 1.2e-2).
Gradient: by linearity, the B = 256 step's gradient is the mean of the gradients of its 8 micro-batches of 32 (4032 rows: other
plans again), compared tensor by tensor for every matrix of blocks 0, 12 and 23, project_in / project_out and every bias.

Run once with global_cond_type "prepend" (126 tokens per clip) and once with "adaLN" (125 tokens: 32 000 rows through the gate
epilogue of every block).
Bounds: about 3x the margins measured on an MI355X (printed as BATCH_MARGINS), quoted per constant below."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import kalle_oracle as ko  # noqa: E402

B, MICRO = 256, 32
# measured on an MI355X (prepend / adaLN): worst clip's rel error vs its B = 1 forward 1.48e-3 / 1.22e-3 (median 1.45e-3 /
# 1.19e-3, worst / median 1.02 / 1.03); per-tensor gradient rel 6.8e-4 / 7.7e-4 (worst: layers.0.cross_attn.to_q); loss rel
# 4.7e-7 / 1.9e-7; clips 0, 127, 128, 255 vs the CPU oracle: rel 3.79e-3 ... 3.87e-3, cosine 1.000
CLIP_REL_MAX = 5e-3
CLIP_WORST_OVER_MEDIAN = 1.5        # (one clip computed wrong stands out of 256 that agree to within 3 %)
GRAD_REL_MAX = 2.5e-3
LOSS_REL_MAX = 2e-6
ORACLE_COS_MIN, ORACLE_REL_MAX = 0.999, 1.2e-2     # (SURVEY 8c allows 3e-2)


@pytest.fixture(scope="module", autouse=True)
def _drop_in_installed():
    import kalle_audio_amd
    kalle_audio_amd.install()


def _slice_cond(cond, s):
    return {k: (v[0][s], None if v[1] is None else v[1][s]) for k, v in cond.items()}


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


@pytest.mark.parametrize("gtype", ["prepend", "adaLN"])
def test_headline_batch_distinct_clips(dev, gtype):
    import bench
    from kalle_audio_amd import engine
    from kalle_audio_amd.stable_audio_tools.training.diffusion import diffusion_train_step
    cfg = dict(bench.CFG, global_cond_type=gtype)
    model = bench.build_model(dev, cfg=cfg)
    lat, noise, t, cond = bench.make_batch(B, dev, 2026, cfg)
    margins = {}

    # ---- forward, per clip: B = 256 against B = 1
    with torch.no_grad():
        _, info = diffusion_train_step(model, lat, t, noise, cond, objective="v")
        out = info["output"].float().clone()
        del info
        errs = []
        for i in range(B):
            s = slice(i, i + 1)
            _, one = diffusion_train_step(model, lat[s], t[s], noise[s], _slice_cond(cond, s), objective="v")
            errs.append(_rel(out[s], one["output"].float()))
    errs = torch.tensor(errs)
    worst, med = errs.max().item(), errs.median().item()
    margins.update(clip_rel_worst=worst, clip_rel_median=med, worst_clip=int(errs.argmax()), worst_over_median=worst / med)

    # ---- clips 0, 127, 128, 255 against the CPU oracle (fp32, the same weights)
    pick = torch.tensor([0, 127, 128, 255], device=dev)
    sd = {n: p.detach().float().cpu() for n, p in model.model.model.named_parameters()}
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    ocfg = dict(embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], global_cond_type=gtype)
    with torch.no_grad():
        _, out_ref, _, _ = ko.train_step_loss(sd, ocfg, lat[pick].cpu(), noise[pick].cpu(), t[pick].cpu(), "v",
                                              cross_attn_cond=cond["prompt"][0][pick].cpu(),
                                              global_embed=cond["global"][0][pick].cpu())
    del sd
    got = out[pick].cpu()
    for j, i in enumerate(pick.tolist()):
        margins[f"oracle_cos_{i}"] = _cos(got[j], out_ref[j])
        margins[f"oracle_rel_{i}"] = _rel(got[j], out_ref[j])
    del out

    # ---- gradient: one B = 256 step against the mean of 8 micro-batches of 32 (lr 0: the weights stay put)
    tr = engine.DataParallelTrainer(model, lr=0.0, optimizer="Adam")
    prefix = "model.model.transformer."
    names = [n for n in tr.flat.names if n.startswith(prefix + "project_")]
    for layer in (0, 12, 23):
        names += [n for n in tr.flat.names if n.startswith(f"{prefix}layers.{layer}.") and tr.flat.grad_view(n).dim() == 2]
    names += [n for n in tr.flat.names if n.endswith(".bias") and n not in names]
    assert len(names) > 3 * 8, names

    loss_full = tr.train_step(model, lat, t, noise, cond, objective="v").item()
    torch.cuda.synchronize()
    g_full = {n: tr.flat.grad_view(n).detach().double().clone() for n in names}
    tr.grad_accum_steps, tr.micro = B // MICRO, 0
    losses = []
    for k in range(B // MICRO):
        s = slice(k * MICRO, (k + 1) * MICRO)
        losses.append(tr.train_step(model, lat[s], t[s], noise[s], _slice_cond(cond, s), objective="v").item())
    torch.cuda.synchronize()
    loss_mean = sum(losses) / len(losses)
    margins["loss_rel"] = abs(loss_full - loss_mean) / abs(loss_mean)
    worst_g, worst_n = 0.0, None
    for n in names:
        # (the flat buffer holds the SUM over the accumulation window; 1 / steps is folded into Adam)
        r = _rel(g_full[n], tr.flat.grad_view(n).double() / (B // MICRO))
        assert g_full[n].abs().max() > 0, n
        if r > worst_g:
            worst_g, worst_n = r, n
    margins["grad_rel_worst"] = worst_g
    print(f"BATCH_MARGINS {gtype} worst_grad={worst_n} " + " ".join(
        f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in margins.items()))

    assert worst <= CLIP_REL_MAX, margins
    assert worst <= CLIP_WORST_OVER_MEDIAN * med, margins
    for i in pick.tolist():
        assert margins[f"oracle_cos_{i}"] >= ORACLE_COS_MIN, margins
        assert margins[f"oracle_rel_{i}"] <= ORACLE_REL_MAX, margins
    assert margins["loss_rel"] <= LOSS_REL_MAX, margins
    assert worst_g <= GRAD_REL_MAX, (worst_n, margins)
