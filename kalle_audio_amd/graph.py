"""HIP-graph replay of a fixed-shape forward for the launch-bound inference loops.

One sampler step of the DiT at generation batch sizes is ~400 kernel launches that take less GPU time than the host
needs to issue them (`stable_audio_tools/inference/sampling.py:24-86` calls `model(x, t, **extra_args)` once per step).
`GraphedForward` captures that call once per (shapes, dtypes, scalar arguments) signature into a HIP graph - torch's
`CUDAGraph` on ROCm records the hipLaunchKernelGGL calls the C-ABI issues on the capturing stream - and replays it with
the inputs copied into static buffers.  Inference only (no autograd, no RNG inside the captured region).
"""
import gc

import torch


class GraphedForward:
    def __init__(self, fn, warmup=2):
        self.fn = fn
        self.warmup = warmup
        self._cache = {}

    @staticmethod
    def _sig(v):
        if torch.is_tensor(v):
            return ("T", tuple(v.shape), v.dtype, v.device)
        if isinstance(v, (list, tuple)):
            return tuple(GraphedForward._sig(x) for x in v)
        return ("V", v)

    @torch.no_grad()
    def __call__(self, *args, **kwargs):
        names = sorted(kwargs)
        key = (tuple(self._sig(a) for a in args), tuple((n, self._sig(kwargs[n])) for n in names))
        ent = self._cache.get(key)
        if ent is None:
            s_args = [a.clone() if torch.is_tensor(a) else a for a in args]
            s_kw = {n: (kwargs[n].clone() if torch.is_tensor(kwargs[n]) else kwargs[n]) for n in names}
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # lazy initialisation (function attributes, bf16 weight copies)
                for _ in range(self.warmup):
                    self.fn(*s_args, **s_kw)
            torch.cuda.current_stream().wait_stream(side)
            # Python's cyclic collector must not run inside the capture: a dead cycle that owns another captured graph (a model and
            # the trainer hooked into its blocks refer to each other) would be destroyed there, which the runtime refuses
            # while a stream is capturing - the process aborts.  torch.cuda.graph collected before a capture until 2.9 and
            # no longer does: collect here, and keep the collector off until the capture has ended.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = self.fn(*s_args, **s_kw)
            finally:
                if gc_was_on:
                    gc.enable()
            ent = self._cache[key] = (g, s_args, s_kw, out)
        g, s_args, s_kw, out = ent
        for dst, src in zip(s_args, args):
            if torch.is_tensor(dst):
                dst.copy_(src)
        for n in names:
            if torch.is_tensor(s_kw[n]):
                s_kw[n].copy_(kwargs[n])
        g.replay()
        return out          # static buffer: valid until the next call with the same signature
