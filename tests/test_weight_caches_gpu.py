"""-m gpu: every cache derived from weights against every way a model's weights can change ("Weight-derived
caches").  A cell = one cache x one route: build the smallest model that owns the cache, run it twice under weights W0 (the
second call must hit the cache where that is observable), change the weights to W1 by the route, run again, and compare with
a FRESH TWIN - a newly constructed model of the same config that has never run, given the model's current state_dict by plain
load_state_dict and called once through the same entry point.  The twin owns no cache that could be stale; the suite holds it
to fp64 oracles elsewhere.  Two assertions per cell:

  rel(before, twin) >= 1e-2     the change is large enough to tell a stale copy from a fresh one
                                (the bound of test_captured_sampler_graph_follows_new_weights)
  rel(after,  twin) <= 1e-6     the bound of test_stacked_context_weights_follow_fused_adam for the same kind of comparison:
                                same kernels, same weights, same inputs; torch.equal on the sampler-graph path, which the suite
                                already holds to bit-equality

Caches: C1 bf16 compute copy per GEMM weight (dit_ops.bf16_of), C2 stacked cross-attention k | v weights, C3 captured sampler
graph, C4 folded weight-norm conv weights of the Oobleck VAE, C5 the same for the mel-VAE, C6 e4m3 codes / scales and the
quantised decode plan, C7 bf16 decode plan and the device head's weights.
Routes: R1 no_grad in-place, R2 load_state_dict, R3 load_state_dict(assign=True) with coinciding version counters, R4 p.data = t
(and module.half().float()), R5 FusedAdam.step, R6 a DataParallelTrainer step / trainer.load_state_dict, R7 torch.optim.AdamW,
R8 p.data.copy_ then weights_changed(), R9 remove_weight_norm / weight_norm."""
import os
import sys

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import golden_util as gu  # noqa: E402
from test_modules_gpu import T, load_seeded, rel  # noqa: E402

pytestmark = pytest.mark.gpu

D, DC, NTOK, S = 128, 64, 12, 7          # C1: D = 128, 2 heads of 64, 12 tokens (the family of test_round2_gpu._small_dit)
LR = 2e-2                                # Adam's first step moves every weight by ~lr: far above a bf16 ulp of these weights
CHANGED, FOLLOWED = 1e-2, 1e-6


# ------------------------------------------------------------------------------------------------ the routes
def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _named(model):
    return list(model.named_parameters())


def r1_inplace(cell, m):
    w1 = cell.other()
    with torch.no_grad():
        for n, p in _named(m):
            p.copy_(w1[n])


def r2_load_state_dict(cell, m):
    m.load_state_dict(cell.other())


def r3_assign(cell, m):
    """load_state_dict(assign=True): new Parameter objects whose version counters restart - brought to the OLD parameters' counts
    here, so that a key made of versions alone cannot tell them apart (asserted)"""
    old = {n: p._version for n, p in _named(m)}
    sd = cell.other()
    for n, v in old.items():
        for _ in range(v - sd[n]._version):
            sd[n].add_(0)
    ids = {n: id(p) for n, p in _named(m)}
    m.load_state_dict(sd, assign=True)
    for n, p in _named(m):
        assert id(p) != ids[n] and p._version == old[n], (n, p._version, old[n])


def r4_repoint(cell, m):
    w1 = cell.other()
    for n, p in _named(m):
        v = p._version
        p.data = w1[n].clone()
        assert p._version == v


def _set_grads(m):
    g = torch.Generator().manual_seed(5)
    for _, p in _named(m):
        p.grad = torch.randn(p.shape, generator=g).to(p.device)


def r5_fused_adam(cell, m):
    from kalle_audio_amd.engine import FusedAdam
    m.requires_grad_(True)
    opt = FusedAdam(m.parameters(), lr=LR)
    _set_grads(m)
    vs = [p._version for _, p in _named(m)]
    opt.step()
    assert vs == [p._version for _, p in _named(m)]         # (the raw-pointer write torch does not see)
    opt.zero_grad(set_to_none=True)


def r7_adamw(cell, m):
    m.requires_grad_(True)
    opt = torch.optim.AdamW(m.parameters(), lr=LR)
    _set_grads(m)
    opt.step()
    opt.zero_grad(set_to_none=True)


def r8_data_copy(cell, m):
    import kalle_audio_amd
    w1 = cell.other()
    for n, p in _named(m):
        v = p._version
        p.data.copy_(w1[n])
        assert p._version == v
    kalle_audio_amd.weights_changed()


def _trainer(cell, m):
    from kalle_audio_amd import engine
    m.requires_grad_(True)
    return engine.DataParallelTrainer(cell.train_root(m), lr=LR, optimizer="AdamW")


def r6_trainer_step(cell, m):
    tr = _trainer(cell, m)
    tr.backward(cell.loss(m))
    assert tr.step_count == 1


def r6_trainer_load(cell, m):
    tr = _trainer(cell, m)
    sd = tr.state_dict()
    pre = cell.train_prefix
    sd["model"] = {pre + k: v for k, v in cell.other().items()}
    tr.load_state_dict(sd)


ROUTES = {"R1": r1_inplace, "R2": r2_load_state_dict, "R3": r3_assign, "R4": r4_repoint, "R5": r5_fused_adam,
          "R6step": r6_trainer_step, "R6load": r6_trainer_load, "R7": r7_adamw, "R8": r8_data_copy}
R1_TO_R8 = list(ROUTES)


class _Root(nn.Module):
    """the module tree a trainer is built over when the cell's model is a bare layer: `name` decides its bucket"""
    def __init__(self, name, child):
        super().__init__()
        setattr(self, name, child)


# ------------------------------------------------------------------------------------------------ the cells
class Cell:
    """make(seed) -> a new model on the GPU; run(m) -> the output of the entry point (a new tensor); probe(m) -> the cache
    objects a second call must find again; loss(m) -> a scalar through the training path (for the trainer's step)"""
    seeds = (70, 71)
    train_prefix = ""
    exact = False                       # torch.equal instead of rel <= 1e-6

    def __init__(self, dev):
        self.dev = dev

    def other(self):
        return _state(self.make(self.seeds[1]))

    def train_root(self, m):
        return m

    def probe(self, m):
        return []

    def check(self, route):
        m = self.make(self.seeds[0])
        first = self.run(m)
        held = self.probe(m)
        before = self.run(m)
        again = self.probe(m)
        assert len(held) == len(again) and all(a is b for a, b in zip(held, again)), "the second call did not hit the cache"
        assert torch.equal(first, before) if self.exact else rel(first, before) <= FOLLOWED
        route(self, m)
        after = self.run(m)
        twin = self.make(self.seeds[0] + 7)
        twin.load_state_dict(_state(m))
        want = self.run(twin)
        self.verdict(before, after, want)

    def verdict(self, before, after, want):
        changed, followed = rel(before, want), rel(after, want)
        print(f"{type(self).__name__}: rel(before, twin) {changed:.3e}  rel(after, twin) {followed:.3e}")
        assert changed >= CHANGED, ("the change is too small to tell a stale copy from a fresh one", changed)
        if self.exact:
            assert torch.equal(after, want), followed
        assert followed <= FOLLOWED, followed


def _bf16_copies(m):
    return [p._kalle_bf16[1] for p in m.parameters() if getattr(p, "_kalle_bf16", None) is not None]


class C1Block(Cell):
    """one TransformerBlock forward under no_grad: six GEMM weights through bf16_of"""
    train_prefix = "blk."

    def make(self, seed):
        import kalle_audio_amd
        kalle_audio_amd.install()
        from stable_audio_tools.models import transformer as TR
        self.rot = TR.RotaryEmbedding(32).to(self.dev)
        return load_seeded(TR.TransformerBlock(D, dim_heads=64, cross_attend=True, dim_context=DC), seed, self.dev)

    def _inputs(self):
        return T(gu.make_input("x", (1, NTOK, D), 3), self.dev), T(gu.make_input("ctx", (1, S, DC), 3), self.dev)

    def _fwd(self, m):
        x, ctx = self._inputs()
        return m(x, context=ctx, rotary_pos_emb=self.rot.forward_from_seq_len(NTOK))

    def run(self, m):
        with torch.no_grad():
            return self._fwd(m).float().clone()

    def probe(self, m):
        c = _bf16_copies(m)
        assert len(c) >= 6
        return c

    def train_root(self, m):
        return _Root("blk", m)

    def loss(self, m):
        return self._fwd(m).float().pow(2).mean()


class C1Linear(Cell):
    """KF.linear, as ContinuousTransformer calls it for project_in"""
    train_prefix = "project_in."

    def make(self, seed):
        return load_seeded(nn.Linear(DC, D, bias=False), seed, self.dev)

    def _fwd(self, m):
        from kalle_audio_amd import functional as KF
        return KF.linear(T(gu.make_input("x", (1, NTOK, DC), 4), self.dev), m.weight, out_dtype=torch.bfloat16)

    def run(self, m):
        with torch.no_grad():
            return self._fwd(m).float().clone()

    def probe(self, m):
        return _bf16_copies(m)

    def train_root(self, m):
        return _Root("project_in", m)

    def loss(self, m):
        return self._fwd(m).float().pow(2).mean()


class C2Dit(Cell):
    """diffusion_train_step under no_grad on the small DiT: the stacked k | v weights of all layers (KALLE_BATCH_CTX_KV default)"""

    def make(self, seed):
        import test_round2_gpu as r2
        return r2._small_dit(self.dev, seed=seed)

    def _batch(self):
        import test_round2_gpu as r2
        return r2._batch(self.dev, 2, 12)

    def run(self, m):
        from stable_audio_tools.training.diffusion import diffusion_train_step
        lat, noise, t, cond = self._batch()
        with torch.no_grad():
            return diffusion_train_step(m, lat, t, noise, cond)[1]["output"].float().clone()

    def probe(self, m):
        tr = m.model.model.transformer
        hit = getattr(tr, "_kalle_wall", None)
        pinned = any(getattr(p, "_kalle_bf16_pinned", None) is not None for p in m.parameters())
        assert hit is not None or pinned, "the stacked k | v weights were not cached"
        return [] if hit is None else [hit[1]]

    def loss(self, m):
        from stable_audio_tools.training.diffusion import diffusion_train_step
        lat, noise, t, cond = self._batch()
        return diffusion_train_step(m, lat, t, noise, cond)[0]


class C3Sampler(C2Dit):
    """generate_diffusion_cond on a frozen model: the captured graph (and, by default, the hoisted conditioning); the twin samples
    through its own graph, so the comparison is bit for bit"""
    exact = True

    def make(self, seed):
        return super().make(seed).eval().requires_grad_(False)

    def run(self, m):
        from stable_audio_tools.inference.generation import generate_diffusion_cond
        import test_round2_gpu as r2
        _, _, _, cond = r2._batch(self.dev, 1, 13)
        m.eval().requires_grad_(False)
        return generate_diffusion_cond(m, steps=6, cfg_scale=3.0, conditioning_tensors=cond, batch_size=1, sample_size=125,
                                       seed=7, device="cpu").float().clone()

    def probe(self, m):
        g = getattr(m, "_kalle_graphed", None)
        assert g is not None and g._cache
        return [g] + [e[0] for e in g._cache.values()]


class C4Oobleck(Cell):
    """ae.encode and ae.decode under no_grad: WNConv1d and WNConvTranspose1d fold weight_g / weight_v once per weight change"""
    seeds = (23, 24)
    train_prefix = "pretransform."

    def make(self, seed):
        import kalle_audio_amd
        kalle_audio_amd.install()
        from stable_audio_tools.models.factory import create_model_from_config
        return load_seeded(create_model_from_config(gu.oobleck_cfg(True)), seed, self.dev)

    def _fwd(self, m):
        torch.manual_seed(0)            # (a sampling bottleneck draws the same noise in every run)
        z = m.encode(T(gu.make_input("wav", (2, 2, 1200), 66, 0.5), self.dev))
        rec = m.decode(z[:, :4] + 0.3 * z[:, 4:] if z.shape[1] == 8 else z)
        return z, rec

    def run(self, m):
        with torch.no_grad():
            z, rec = self._fwd(m)
        return torch.cat([z.float().reshape(-1), rec.float().reshape(-1)]).clone()

    def probe(self, m):
        from stable_audio_tools.models import autoencoders as A
        kinds = {type(x) for x in m.modules() if isinstance(x, A._WNBase)}
        assert kinds == {A.WNConv1d, A.WNConvTranspose1d}
        packed = [x._kalle_packed[1] for x in m.modules() if isinstance(x, A._WNBase) and getattr(x, "_kalle_packed", None)]
        assert packed
        return packed

    def train_root(self, m):
        return _Root("pretransform", m)        # a VAE trained as a pretransform (enable_grad): the trainer's `_vae` bucket

    def loss(self, m):
        z, rec = self._fwd(m)
        return z.float().pow(2).mean() + rec.float().pow(2).mean()


class C5MelVae(Cell):
    """the smallest BigVGANFlowVAE of the mel-VAE tests: extract_latents and inference_from_latents"""
    seeds = (30, 31)

    def make(self, seed):
        from kalle_audio_amd.flows import BigVGANFlowVAE
        return load_seeded(BigVGANFlowVAE(gu.MELVAE_CONFIGS["amp1_causal"]), seed, self.dev)

    def run(self, m):
        with torch.no_grad():
            enc = m.extract_latents(T(gu.make_input("melwav", (2, 1, 256), 30, 0.5), self.dev))
            eps = T(gu.make_input("meleps", (2, enc.shape[1] // 2, enc.shape[2]), 30), self.dev)
            rec = m.inference_from_latents(enc, do_sample=True, noise=eps)
        return torch.cat([enc.float().reshape(-1), rec.float().reshape(-1)]).clone()

    def probe(self, m):
        from kalle_audio_amd import flows
        packed = [x._kalle_packed[1] for x in m.modules() if isinstance(x, flows._ConvBase) and getattr(x, "_kalle_packed", None)]
        assert packed
        return packed


# ------------------------------------------------------------------------------------------------ C1, C2, C4, C5: the matrix
@pytest.mark.parametrize("route", R1_TO_R8)
@pytest.mark.parametrize("cell", [C1Block, C1Linear, C2Dit, C4Oobleck], ids=["C1block", "C1linear", "C2", "C4"])
def test_cache_follows(dev, cell, route):
    cell(dev).check(ROUTES[route])


@pytest.mark.parametrize("route", ["R1", "R2", "R3", "R4", "R5", "R8"])
def test_cache_follows_melvae(dev, route):
    C5MelVae(dev).check(ROUTES[route])


@pytest.mark.parametrize("cell", [C1Block, C1Linear], ids=["C1block", "C1linear"])
def test_cache_follows_half_float_round_trip(dev, cell):
    """R4, module.half().float() (the reference's model_half, pretransforms.py:48): W0 is not representable in fp16 - nor in bf16 -
    so the round trip changes the weights; version counters do not move, and the new fp32 storage has the size of the freed one.
    fp16 keeps 11 significant bits and the GEMMs read 8: the stale copy bf16(W0) and the fresh bf16(fp16(W0)) differ only where
    the first rounding lands on a bf16 tie, so the change cannot reach 1e-2.  The precondition here is what the bound needs to
    tell the two apart: some bf16 weight differs, and the stale output is more than 10 x the bound away from the twin's"""
    c = cell(dev)
    m = c.make(c.seeds[0])
    w0 = _state(m)
    c.run(m)
    before = c.run(m)
    vs = [p._version for p in m.parameters()]
    ptrs = [p.data_ptr() for p in m.parameters()]
    m.half().float()
    assert vs == [p._version for p in m.parameters()]
    differ = sum(int((w0[n].bfloat16() != p.detach().bfloat16()).sum()) for n, p in m.named_parameters() if p.dim() == 2)
    assert differ > 0, "the round trip left every bf16 weight as it was"
    after = c.run(m)
    twin = c.make(c.seeds[0] + 7)
    twin.load_state_dict(_state(m))
    want = c.run(twin)
    print("half().float():", differ, "bf16 weights differ; same addresses:", ptrs == [p.data_ptr() for p in m.parameters()],
          "rel(before, twin)", rel(before, want), "rel(after, twin)", rel(after, want))
    assert rel(before, want) > 10 * FOLLOWED, rel(before, want)
    assert rel(after, want) <= FOLLOWED, rel(after, want)


def test_cache_follows_remove_and_apply_weight_norm(dev):
    """R9 on the mel-VAE: weight_norm -> forward -> remove_weight_norm -> change weight -> forward -> weight_norm -> forward"""
    from kalle_audio_amd import flows
    c = C5MelVae(dev)
    m = c.make(c.seeds[0])
    convs = [x for x in m.modules() if isinstance(x, flows._ConvBase) and x._wn]
    assert len(convs) >= 8
    c.run(m)
    before = c.run(m)
    for x in convs:                     # (every weight-normed conv, also those BigVGANFlowVAE.remove_weight_norm leaves)
        flows.remove_weight_norm(x)
    assert not any(x._wn for x in convs)
    assert rel(c.run(m), before) <= 1e-4                 # the same weights folded on the host: the suite's bound for the fp32 conv path
    with torch.no_grad():
        for x in convs:
            x.weight[: max(1, x.weight.shape[0] // 2)].mul_(3.0)
    plain = c.run(m)
    twin = c.make(c.seeds[0] + 7)
    for x in [x for x in twin.modules() if isinstance(x, flows._ConvBase) and x._wn]:
        flows.remove_weight_norm(x)
    twin.load_state_dict(_state(m))
    want = c.run(twin)
    print("R9 removed: rel(before, twin)", rel(before, want), "rel(after, twin)", rel(plain, want))
    assert rel(before, want) >= CHANGED and rel(plain, want) <= FOLLOWED, (rel(before, want), rel(plain, want))
    for x in convs:
        flows.weight_norm(x)
    with torch.no_grad():
        for x in convs:
            x.weight_g[: max(1, x.weight_g.shape[0] // 2)].mul_(1.0 / 3.0)
    again = c.run(m)
    twin = c.make(c.seeds[0] + 7)
    twin.load_state_dict(_state(m))
    want = c.run(twin)
    print("R9 re-applied: rel(previous, twin)", rel(plain, want), "rel(after, twin)", rel(again, want))
    assert rel(plain, want) >= CHANGED and rel(again, want) <= FOLLOWED, (rel(plain, want), rel(again, want))


# ------------------------------------------------------------------------------------------------ C3: the sampler graph
@pytest.mark.parametrize("precond", ["1", "0"], ids=["precond", "inloop"])
@pytest.mark.parametrize("route", ["R2", "R3", "R4", "R6step", "R6load", "R8"])
def test_sampler_graph_follows(dev, monkeypatch, route, precond):
    monkeypatch.setenv("KALLE_SAMPLE_PRECOND", precond)
    C3Sampler(dev).check(ROUTES[route])


# ------------------------------------------------------------------------------------------------ C6, C7: Llasa generation
FRAMES = 5


class LlasaCell(Cell):
    """build(64) of test_model_llasa_generation_gpu.  W1 = W0 with a factor 3 on a slice of `target`: a projection weight, a norm
    scale, a head weight - or all three"""
    TARGETS = {"proj": ["base_model.model.layers.1.self_attn.o_proj.weight"],
               "norm": ["base_model.model.layers.0.post_attention_layernorm.weight"],
               "head": ["distribution_linear.2.weight"]}

    def __init__(self, dev, tmp_path, mode, target="all"):
        super().__init__(dev)
        self.tmp_path, self.mode = tmp_path, mode
        self.names = sum(self.TARGETS.values(), []) if target == "all" else self.TARGETS[target]
        self.fmt, self.batch, self.device_head = mode

    def make(self, seed):
        import test_model_llasa_generation_gpu as G
        m, self.lat, _ = G.build(64, self.dev, self.tmp_path)
        if seed == "w1":
            with torch.no_grad():
                sd = dict(m.named_parameters())
                for n in self.names:
                    w = sd[n]
                    w[: max(1, w.shape[0] // 2)].mul_(3.0)
        m.quantize_decoder(self.fmt)
        return m

    seeds = (0, "w1")

    def other(self):
        return _state(self.make("w1"))

    def run(self, m):
        import test_model_llasa_generation_gpu as G
        base = G.prompts(self.dev, self.lat)
        R = {"one": 1, "rows": 3, "wide": 17}[self.batch]
        ps = [base[i % 3] for i in range(R)]
        noise = G.draw(self.dev, FRAMES, R, self.lat)
        kw = dict(end_disp_kl_thres=-1.0, max_length=FRAMES)
        if self.batch == "one":
            call = lambda **k: [m.infer(ps[0][0], ps[0][1], **kw, **k)]                  # noqa: E731
        else:
            call = lambda **k: m.infer_batch(ps, rows=R if R > 16 else None, **kw, **k)   # noqa: E731
        if self.device_head:
            outs = call(device_head=True, noise=noise)
        else:
            with G.host_noise(noise):
                outs = call()
        return torch.cat([o.float().reshape(-1) for o in outs]).clone()

    def probe(self, m):
        from kalle_audio_amd.model_sigmaVAE import LlamaModel
        model = m.base_model.model
        ws = [w for layer in model.layers for w in LlamaModel._layer_weights(layer)]
        held = [w._kalle_bf16[1] for w in ws]
        if self.fmt:
            held += [w._kalle_e4m3[1] for w in ws]
        if self.device_head:
            held.append(m.distribution_linear[2].weight._kalle_bf16[1])
        return held


def _llasa_routes(cell, m, route):
    """the routes on the cell's target parameters only (the tied lm_head and the embedding stay as they are)"""
    w1 = cell.other()
    params = dict(m.named_parameters())
    if route in ("R2", "R3"):
        sd = {k: v for k, v in w1.items()}
        if route == "R3":
            # (state_dict() carries the reference's split names, which the load hook concatenates into NEW tensors; under the
            # parameters' own names the tensors handed over become the parameters)
            sd = {n: p.detach().clone() for n, p in cell.make("w1").named_parameters()}
            old = {n: p._version for n, p in params.items()}
            ids = {n: id(p) for n, p in params.items()}
            for n, v in old.items():
                for _ in range(v - sd[n]._version):
                    sd[n].add_(0)
            sd["base_model.lm_head.weight"] = sd["base_model.model.embed_tokens.weight"]
            m.load_state_dict(sd, assign=True)
            for n, p in m.named_parameters():        # (assign=True unties lm_head from the embedding: one more name)
                assert n not in ids or (id(p) != ids[n] and p._version == old[n]), (n, p._version, old[n])
        else:
            m.load_state_dict(sd)
        return
    for n in cell.names:
        p, v = params[n], params[n]._version
        if route == "R1":
            with torch.no_grad():
                p.copy_(w1[n])
        elif route == "R4":
            p.data = w1[n].clone()
            assert p._version == v
        elif route == "R8":
            p.data.copy_(w1[n])
            assert p._version == v
    if route == "R8":
        import kalle_audio_amd
        kalle_audio_amd.weights_changed()
    if route == "R5":
        from kalle_audio_amd.engine import FusedAdam
        # Adam's first step moves a weight by lr against the sign of its gradient: the gradient -sign(W1 - W0) and a step of
        # |W1 - W0| per element would need a per-element lr; one step at lr = the mean |W1 - W0| of the changed slice instead
        for n in cell.names:
            p = params[n]
            d = (w1[n] - p.detach())
            lr = float(d.abs().sum() / max(1, int((d != 0).sum())))
            p.grad = -torch.sign(d)
            opt = FusedAdam([p], lr=lr, weight_decay=0.0)
            v = p._version
            opt.step()
            assert p._version == v
            p.grad = None


LLASA_MODES = [(None, "one", False), ("e4m3", "one", True), ("e4m3", "rows", False), (None, "rows", True), (None, "wide", False),
               (None, "wide", True)]
LLASA_IDS = ["bf16-infer-host", "e4m3-infer-device", "e4m3-rows-host", "bf16-rows-device", "bf16-wide-host", "bf16-wide-device"]


def _llasa_check(cell, route):
    m = cell.make(0)
    first = cell.run(m)
    held = cell.probe(m)
    before = cell.run(m)
    again = cell.probe(m)
    assert all(a is b for a, b in zip(held, again)) and len(held) == len(again), "the second call did not hit the cache"
    assert rel(first, before) <= FOLLOWED
    _llasa_routes(cell, m, route)
    after = cell.run(m)
    twin = cell.make(0)
    twin.load_state_dict(_state(m))
    want = cell.run(twin)
    cell.verdict(before, after, want)


@pytest.mark.parametrize("route", ["R1", "R2", "R3", "R4", "R5", "R8"])
@pytest.mark.parametrize("mode", LLASA_MODES, ids=LLASA_IDS)
def test_llasa_generation_follows(dev, tmp_path, mode, route):
    """C6 / C7 through infer and infer_batch: one-row, R-row and wide steps, both weight formats, both heads; a projection weight,
    a norm scale and a head weight change together"""
    _llasa_check(LlasaCell(dev, tmp_path, mode), route)


@pytest.mark.parametrize("route", ["R1", "R4"])
@pytest.mark.parametrize("target", ["proj", "norm", "head"])
@pytest.mark.parametrize("mode", [("e4m3", "one", True), (None, "rows", True)], ids=["e4m3-infer-device", "bf16-rows-device"])
def test_llasa_generation_follows_each_weight(dev, tmp_path, mode, target, route):
    """the three kinds of weight one at a time: a stale copy of one of them cannot hide behind the change of the others"""
    _llasa_check(LlasaCell(dev, tmp_path, mode, target), route)


@pytest.mark.parametrize("route", ["R1", "R4", "R8"])
@pytest.mark.parametrize("fmt", [None, "e4m3"], ids=["bf16", "e4m3"])
def test_live_kv_cache_follows_a_changed_weight(dev, tmp_path, fmt, route):
    """a weight changes between two forward_cached steps on a LIVE KV cache.  The contract: the cache's decode plan
    follows in both weight formats - the next step reads the new weights against the rows already cached.  Twin: a fresh model
    with the new weights and a cache holding the SAME rows, stepping once"""
    import test_model_llasa_generation_gpu as G
    m, _, Dm = G.build(64, dev, tmp_path)
    model = m.base_model.model.quantize_decode_weights(fmt)
    x = T(gu.make_input("x", (1, 8, Dm), 9), dev)
    with torch.no_grad():
        cache = model.init_cache(16, dev)
        model.forward_cached(x[:, :5].contiguous(), cache)
        model.forward_cached(x[:, 5:6].contiguous(), cache)
        plan = cache["plan"]
        model.forward_cached(x[:, 6:7].contiguous(), cache)
        assert cache["plan"] is plan, "the second step did not hit the plan"
        kvs, n = [k.clone() for k in cache["kv"]], cache["len"]
        stale = model.forward_cached(x[:, 7:8].contiguous(), cache).float().clone()
        cache["len"] = n
        for k, s in zip(cache["kv"], kvs):
            k.copy_(s)
        ws = [model.layers[1].self_attn.o_proj.weight, model.layers[0].mlp.down_proj.weight, model.layers[1].input_layernorm.weight]
        for w in ws:
            w1 = w.detach().clone()
            w1[: max(1, w.shape[0] // 2)] *= 3.0
            v = w._version
            if route == "R1":
                w.copy_(w1)
            elif route == "R4":
                w.data = w1
                assert w._version == v
            else:
                w.data.copy_(w1)
                assert w._version == v
        if route == "R8":
            import kalle_audio_amd
            kalle_audio_amd.weights_changed()
        after = model.forward_cached(x[:, 7:8].contiguous(), cache).float().clone()
        t, _, _ = G.build(64, dev, tmp_path)
        t.load_state_dict(_state(m))
        twin = t.base_model.model.quantize_decode_weights(fmt)
        tc = twin.init_cache(16, dev)
        tc["len"] = n
        for k, s in zip(tc["kv"], kvs):
            k.copy_(s)
        want = twin.forward_cached(x[:, 7:8].contiguous(), tc).float().clone()
    print("live cache: rel(before, twin)", rel(stale, want), "rel(after, twin)", rel(after, want))
    assert rel(stale, want) >= CHANGED, rel(stale, want)
    assert rel(after, want) <= FOLLOWED, rel(after, want)
