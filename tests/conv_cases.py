"""The case list of the VAE conv dispatch: the entry-point lists of tests/test_conv_gpu.py (imported from there) and a sweep.
tests/test_conv_plan_cpu.py asserts, with the host queries kalle_conv_plan / kalle_conv_transpose_plan /
kalle_conv_wgrad_plan alone, that every case of PLAN_CASES gets the row recorded in tests/golden/conv_plans.json.

A plan case is a dict: kind (conv / convT / wgrad), the shape, and whatever differs from PLAN_DEFAULTS; `prefer` is the
queries' argument (0 auto, 1 always, 2 never the channels-per-lane kernels; in conv_ops: KALLE_CONV_CFIRST unset, "1", "0").
The table is keyed by key(case).  A row is [entry, return code, kalle_conv_last_plan word] and, where entry is
cfirst / cfirstT, Lp, lead, phases, workspace floats.  It was recorded from the code as it was before the planners existed, on a
CPU: that library built with every launch and the launch check made no-ops, conv_ops.conv1d / conv_ops.conv_transpose1d /
conv_train.conv_wgrad driven with shape-only (meta) tensors under each KALLE_CONV_CFIRST value, every C-ABI call they made
logged; entry is the kernel entry point the call reached.  A refused call's row is [the function that refused (an entry
point or pad_act, kalle_conv_pad_act), its return code, 0]; a query has no such name to give, so test_conv_plan_cpu.py compares
code and word there and calls the named function itself.  Calls that conv_ops cannot form (a zero stride, a negative length)
were made at the position-per-lane entry point directly.  The flows-VAE layer
shapes use the module defaults of flows.py with BigVGAN's 24 kHz up-sampling stack (rates 4 4 2 2 2 2, 1536 channels), the
Oobleck ones the Stable-Audio-Open layout of tools/vae_bench.py at 440320 samples and at the 128-latent chunks of
tools/vae_chunked_bench.py."""
import itertools

from test_conv_gpu import (BF16, CFIRST_CASES, CFIRST_EDGES, CFIRST_T_CASES, CONV_CASES, CONVT_CASES, EDGE_CASES, F32, WGRAD_CASES,  # noqa: F401
                           cf, fb, tv2, v2, wg_lane, wg_lds)

# ================================================================================================ the plan table's cases
PLAN_DEFAULTS = dict(stride=1, pl=0, dil=1, xdt=F32, ydt=F32, act=0, res=False, scale=1.0, acc=False, post=0, tanh=False, raw=False,
                     prefer=0, act_on=0, noab=False)
ENTRIES = ("conv", "convT", "cfirst", "cfirstT", "wgrad")
FAMILY_ENTRY = {1: "conv", 2: "conv", 3: "convT", 4: "convT", 5: "cfirst", 6: "cfirst", 7: "cfirstT", 8: "wgrad", 9: "wgrad"}


SHAPE = {"conv": ("B", "Cin", "Lin", "Cout", "Lout", "K"), "convT": ("B", "Cin", "Lin", "Cout", "Lout", "K"), "wgrad": ("B", "CU", "CV", "MU", "LV", "K")}


def pc(kind, **kw):
    """a plan case in canonical form.  conv / convT: B Cin Lin Cout Lout K (+ stride pl dil, dtypes, act, epilogue flags, prefer;
    noab: SnakeBeta without its parameters); wgrad: B CU CV MU LV K (+ stride pl dil act_on act)"""
    c = dict(kind=kind, **{k: kw.pop(k) for k in SHAPE[kind]})
    c.update({k: kw.pop(k) for k in PLAN_DEFAULTS if k in kw and kw[k] != PLAN_DEFAULTS[k]})      # (in one order, whatever the caller's)
    assert not set(kw) - set(PLAN_DEFAULTS), kw
    return c


def key(c):
    """kind, the six shape values in the order of SHAPE, then name=value for whatever differs from PLAN_DEFAULTS"""
    pos = SHAPE[c["kind"]]
    rest = [f"{k}={v:g}" if isinstance(v, float) else f"{k}={int(v)}" for k, v in c.items() if k != "kind" and k not in pos]
    return " ".join([c["kind"]] + [str(c[k]) for k in pos] + rest)


def full(c):
    return {**PLAN_DEFAULTS, **c}


def from_test(c, prefer=None):
    """the plan case of a forward case of test_conv_gpu.py (which calls the entry point its `entry` names: prefer always / never)"""
    kind = "convT" if c["entry"] in ("convT", "cfirstT") else "conv"
    if prefer is None:
        prefer = 1 if c["entry"].startswith("cfirst") else 2
    kw = dict(B=c["B"], Cin=c["Cin"], Lin=c["Lin"], Cout=c["Cout"], Lout=c["Lout"], K=c["K"], stride=c["stride"], pl=c["pl"])
    if kind == "conv":
        kw["dil"] = c["dil"]
    return pc(kind, **kw, xdt=c["xdt"], ydt=c["ydt"], act=c["act"], res=c["res"], scale=c["scale"], acc=c["acc"], post=c["post"],
              tanh=c["tanh"], raw=c["raw"], prefer=prefer)


def from_wgrad(c):
    MU = (c["LV"] + 2 * c["pl"] - c["dil"] * (c["K"] - 1) - 1) // c["stride"] + 1
    return pc("wgrad", B=c["B"], CU=c["CU"], CV=c["CV"], MU=MU, LV=c["LV"], K=c["K"], stride=c["stride"], pl=c["pl"], dil=c["dil"],
              act_on=c["act_on"], act=c["act"])


def conv(B, Cin, Cout, K, Lin, stride=1, pl=None, dil=1, Lout=None, **kw):
    """'same'-style conv: symmetric padding (K - 1) dil / 2 at stride 1, ceil(stride / 2) when strided"""
    if pl is None:
        pl = (K - 1) * dil // 2 if stride == 1 else (stride + 1) // 2
    if Lout is None:
        Lout = (Lin + 2 * pl - dil * (K - 1) - 1) // stride + 1
    return pc("conv", B=B, Cin=Cin, Lin=Lin, Cout=Cout, Lout=Lout, K=K, stride=stride, pl=pl, dil=dil, **kw)


def convT(B, Cin, Cout, K, Lin, stride, pl=None, trim=0, **kw):
    if pl is None:
        pl = (stride + 1) // 2
    return pc("convT", B=B, Cin=Cin, Lin=Lin, Cout=Cout, Lout=(Lin - 1) * stride - 2 * pl + K - trim, K=K, stride=stride, pl=pl, **kw)


def wgrad(B, CU, CV, K, LV, stride=1, pl=0, dil=1, **kw):
    return pc("wgrad", B=B, CU=CU, CV=CV, MU=(LV + 2 * pl - dil * (K - 1) - 1) // stride + 1, LV=LV, K=K, stride=stride, pl=pl, dil=dil, **kw)


def oobleck(B, n, lat_in=64, lat_out=128):
    """conv launches of one Oobleck encode of [B, 2, n] and one decode of [B, lat_in, n / 2048] (autoencoders.py:39-191)"""
    ch, strides = [128, 128, 256, 512, 1024, 2048], [2, 4, 4, 8, 8]
    out, L = [conv(B, 2, 128, 7, n)], n
    for i, s in enumerate(strides):
        for d in (1, 3, 9):
            out += [conv(B, ch[i], ch[i], 7, L, dil=d, act=1, post=1, raw=True), conv(B, ch[i], ch[i], 1, L, res=True)]
        out.append(conv(B, ch[i], ch[i + 1], 2 * s, L, stride=s, act=1))
        L = out[-1]["Lout"]
    out.append(conv(B, 2048, lat_out, 3, L, act=1))
    out.append(conv(B, lat_in, 2048, 7, L))
    for i, s in reversed(list(enumerate(strides))):
        out.append(convT(B, ch[i + 1], ch[i], 2 * s, L, s, act=1))
        L = out[-1]["Lout"]
        for d in (1, 3, 9):
            out += [conv(B, ch[i], ch[i], 7, L, dil=d, act=1, post=1, raw=True), conv(B, ch[i], ch[i], 1, L, res=True)]
    out.append(conv(B, 128, 2, 7, L, act=1))
    return out


def flows_vae(B, n, latent=100, hidden=192, uc=1536):
    """conv launches of the flows VAE (flows.py): encoder, coupling flow, BigVGAN-style decoder"""
    chans, downs = [12, 24, 48, 96, 192, 384, 768], [2, 2, 2, 2, 4, 4]
    out, L = [conv(B, 1, 12, 3, n)], n
    for (ci, co), s in zip(zip(chans[:-1], chans[1:]), downs):
        out.append(conv(B, ci, co, 2 * s, L, stride=s, pl=s // 2 + s % 2, act=3))
        L = out[-1]["Lout"]
        for i in range(6):
            out += [conv(B, co, co, 3, L, dil=2 ** i, act=3), conv(B, co, co, 3, L, act=3, res=True)]
    out.append(conv(B, 768, latent, 3, L, act=3))
    half = latent // 2
    for _ in range(4):
        out.append(conv(B, half, hidden, 1, L))
        for _ in range(4):
            out += [conv(B, hidden, 2 * hidden, 5, L), conv(B, hidden, 2 * hidden, 1, L, act=4), conv(B, hidden, hidden, 1, L, act=4, res=True)]
        out.append(conv(B, hidden, half, 1, L))
    out.append(conv(B, latent, uc, 7, L))
    c = uc
    for u, k in zip([4, 4, 2, 2, 2, 2], [8, 8, 4, 4, 4, 4]):
        out.append(convT(B, c, c // 2, k, L, u, pl=(k - u) // 2, act=3))
        c, L = c // 2, out[-1]["Lout"]
        for kk in (3, 7, 11):
            for d in (1, 3, 5):
                out += [conv(B, c, c, kk, L, dil=d, act=1), conv(B, c, c, kk, L, act=1, res=True, acc=(kk != 3), scale=1 / 3 if kk == 11 else 1.0)]
    out.append(conv(B, c, 1, 7, L, act=1, tanh=True))
    return out


def _plan_cases():
    cs = []
    # ---- the GPU test's own lists (as called there, and under the automatic rule)
    cs += [from_test(c) for c in CONV_CASES + CONVT_CASES + CFIRST_CASES + CFIRST_T_CASES + EDGE_CASES + CFIRST_EDGES]
    cs += [from_test(c, 0) for c in CONV_CASES + CONVT_CASES + CFIRST_CASES + CFIRST_T_CASES + CFIRST_EDGES]
    cs += [from_wgrad(c) for c in WGRAD_CASES]
    # ---- the models' layers
    for B in (1, 4, 8, 16):
        for n in (440320, 128 * 2048):
            cs += oobleck(B, n)
        cs += flows_vae(B, 24000)
    # ---- the data-gradient recipes of conv_train.py and the weight gradients, on the Oobleck encoder's layers
    for B in (1, 4):
        for c in oobleck(B, 440320)[:28] + oobleck(B, 65536)[:28]:
            f = full(c)
            if f["stride"] == 1:      # a conv with flipped taps over dy
                cs.append(conv(B, f["Cout"], f["Cin"], f["K"], f["Lout"], pl=(f["K"] - 1) * f["dil"] - f["pl"], dil=f["dil"]))
            else:                     # a transposed conv over dy, extended by the outputs the symmetric trim drops
                nat = (f["Lout"] - 1) * f["stride"] - 2 * f["pl"] + f["K"]
                cs.append(convT(B, f["Cout"], f["Cin"], f["K"], f["Lout"], f["stride"], pl=f["pl"], trim=-max(0, min(f["Lin"] - nat, f["pl"]))))
            cs.append(wgrad(B, f["Cout"], f["Cin"], f["K"], f["Lin"], stride=f["stride"], pl=f["pl"], dil=f["dil"], act=f["act"] & 1))
        for c in oobleck(B, 440320)[29:35]:       # a transposed conv's data gradient: a strided conv over dy
            f = full(c)
            if c["kind"] == "convT":
                cs.append(conv(B, f["Cout"], f["Cin"], f["K"], f["Lout"], stride=f["stride"], pl=f["pl"], Lout=f["Lin"]))
                cs.append(wgrad(B, f["Cin"], f["Cout"], f["K"], f["Lout"], stride=f["stride"], pl=f["pl"], act_on=1))
    for extra in (1, 2, 3, 4):        # extended transposed convs: never the channels-per-lane kernel, whatever is preferred
        for prefer in (0, 1, 2):
            cs.append(convT(1, 512, 256, 16, 215, 8, trim=-extra, prefer=prefer))
    # ---- the family rule, one side and the other of every threshold
    prefer = 0          # (the rule acts under auto only; the forced sides are in the lists above and below)
    for K in (1, 7):
        lt = 256 if K == 1 else 512
        for Cout in (255, 256, 511, 512, 1024):                 # 160 workgroups of 128 channels x lt positions
            per = -(-Cout // 128)
            for nwg in (159, 160):
                for B in (1, 5):
                    if nwg % (per * B) == 0:
                        cs += [conv(B, 64, Cout, K, nwg // (per * B) * lt, prefer=prefer), conv(B, 64, Cout, K, nwg // (per * B) * lt + 1, prefer=prefer)]
            cs += [conv(2, 64, Cout, K, 159 * lt // (2 * per), prefer=prefer), conv(3, 64, Cout, K, 161 * lt // (3 * per) + lt, prefer=prefer)]
    for Cout in (63, 64, 128, 255):                             # few channels: nwg64 64 / 256, Lout B 1024, Cin 1024
        per = -(-Cout // 64)
        for Cin in (1023, 1024):
            for B, Lout in ((1, 1024), (1, 1025), (2, 512), (2, 513), (4, 256), (3, 342), (16, 215), (64 // per, 512), (64 // per + 1, 512),
                            (64 // per, 513), (255 // per, 512), (256 // per, 512), (256 // per + 1, 512), (1, 512 * (64 // per)),
                            (1, 512 * (64 // per) + 1), (1, 512 * (256 // per) - 1), (1, 512 * (256 // per) + 1)):
                cs.append(conv(B, Cin, Cout, 3, Lout, prefer=prefer))
    for s in (2, 4, 8):                                          # strided: Cout 256
        for Cout in (255, 256, 257):
            cs += [conv(2, 128, Cout, 2 * s, 4096, stride=s, prefer=prefer), conv(2, 128, Cout, 2 * s, 4096, stride=s, dil=2, prefer=prefer)]
    for Cout, lim in ((255, 1536), (256, 1536), (511, 1536), (512, 4096), (1024, 4096)):       # transposed: 1536 / 4096 phase workgroups
        per = -(-Cout // 64)
        for s in (2, 8):
            for B in (1, 3):
                q = lim // (per * B * s)
                for nq512 in (q - 1, q, q + 1):
                    if nq512 > 0:
                        cs += [convT(B, 64, Cout, 2 * s, nq512 * 512 - 1, s, prefer=prefer), convT(B, 64, Cout, 2 * s, nq512 * 512 + 1, s, prefer=prefer)]
    # ---- the channels-per-lane launch: split 1 / 2 / 4 at 2048 / 1024 waves, ks 1 .. 16, with and without the strided / transposed form
    for waves in (1023, 1024, 1025, 2047, 2048, 2049):
        for Cout, B in ((256, 1), (257, 1), (64, 3), (512, 7)):
            tiles = -(-waves // (-(-Cout // 256) * B))
            cs += [conv(B, 16, Cout, 3, 16 * tiles, prefer=1), conv(B, 16, Cout, 3, 16 * tiles - 16, prefer=1),
                   conv(B, 16, Cout, 8, 16 * tiles * 4, stride=4, prefer=1), convT(B, 16, Cout, 8, max(1, 16 * tiles // 4 * 4 // 4 - 1), 4, prefer=1),
                   convT(B, 16, Cout, 8, 16 * tiles // 4 + 3, 4, prefer=1)]
    for Cin, K in itertools.product((64, 171, 172, 342, 343, 683, 1366, 2731, 4096), (1, 3)):
        for B, Lout, Cout in ((1, 16, 64), (1, 215, 128), (2, 17, 64), (1, 1024, 256), (1, 4081, 64), (1, 4097, 64)):
            cs.append(conv(B, Cin, Cout, K, Lout, pl=(K - 1) // 2, Lout=Lout, prefer=1))
    cs += [conv(1, 1024, 2048, 16, 1720, stride=8, prefer=p) for p in (0, 1, 2)]
    # ---- pick_tile: every outcome, Cout <= 4, halo against the span, strides, stride 8 at Lout B 1024
    for Cout in (1, 4, 5, 63, 64, 72, 256, 272):
        for K, dil in ((1, 1), (7, 1), (3, 64), (3, 65), (2, 129)):
            for B, L in ((3, 129), (140, 256), (400, 512), (1, 32910), (50, 512), (22, 1023)):
                cs.append(conv(B, 9, Cout, K, L, prefer=2, act=(Cout + K) % 4))
        for s, L in ((2, 1024), (4, 1024), (8, 8192), (8, 8200), (3, 900)):
            for B in (1,):
                cs += [conv(B, 9, Cout, 2 * s if s <= 8 else 16, L, stride=s, prefer=2), conv(B, 9, Cout, min(2 * s, 16), L, stride=s, dil=2, pl=s, prefer=2)]
        for s in (1, 2, 4, 5, 8):                                     # transposed: every tile form, fallback limits
            for B, L in ((3, 65), (3, 1062), (3, 8344), (1, 12316)):
                cs.append(convT(B, 8, Cout, 2 * s + s % 2, L, s, prefer=2))
        cs += [convT(2, 8, Cout, K, 50, 1, pl=0, prefer=2) for K in (64, 65, 66)]                   # mmax 64 / 65 / 66
        cs += [convT(2, 8, Cout, K, 50, s, pl=1, prefer=2, xdt=BF16) for s, K in ((2, 5), (2, 6), (8, 17), (8, 18), (9, 19), (16, 18))]
    cs += [conv(2, 2048, 264, 16, 600, prefer=2), conv(2, 2047, 264, 16, 600, prefer=2), conv(2, 16, 8, 16, 600, prefer=2),      # co_fast: 2 MiB of weights
           conv(1, 128, 512, 8, 8192, prefer=2), conv(1, 129, 512, 8, 8192, prefer=2)]
    # ---- mixed dtypes, the gate, every epilogue field that decides something
    for xdt, ydt in ((F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)):
        for prefer in (0, 1, 2):
            for act in (0, 4):
                cs += [conv(3, 9, 20, 3, 200, xdt=xdt, ydt=ydt, act=act, prefer=prefer), conv(1, 8, 256, 3, 32, xdt=xdt, ydt=ydt, act=act, prefer=prefer),
                       conv(2, 8, 20, 4, 50, stride=2, xdt=xdt, ydt=ydt, act=act, prefer=prefer), conv(1, 8, 256, 4, 64, stride=2, xdt=xdt, ydt=ydt, act=act, prefer=prefer),
                       convT(2, 8, 20, 4, 50, 2, xdt=xdt, ydt=ydt, act=act, prefer=prefer), convT(1, 8, 256, 4, 16, 2, xdt=xdt, ydt=ydt, act=act, prefer=prefer)]
            for ep in (dict(res=True), dict(post=2), dict(raw=True), dict(scale=0.5), dict(tanh=True), dict(acc=True)) if prefer == 2 else ():
                cs.append(convT(2, 8, 20, 4, 50, 2, xdt=xdt, ydt=ydt, prefer=prefer, **{k: v for k, v in ep.items() if k in ("post", "raw")}))
                cs.append(conv(3, 9, 20, 3, 200, xdt=xdt, ydt=ydt, prefer=prefer, **ep))
    # ---- refused calls
    for prefer in (0, 1, 2):
        cs += [conv(1, 8, 8, 17, 64, prefer=prefer), conv(65536, 8, 8, 3, 64, prefer=prefer), conv(1, 8, 8 * 65536, 3, 64, prefer=prefer),
               conv(1, 8, 8, 3, 64, act=5, prefer=prefer), conv(1, 8, 8, 3, 64, act=1, noab=True, prefer=prefer), conv(1, 8, 8, 3, 64, post=4, prefer=prefer),
               conv(1, 8, 8, 3, 64, post=1, noab=True, prefer=prefer), conv(1, 8, 8, 3, 64, Lout=67, prefer=prefer), conv(1, 8, 8, 3, 64, pl=-1, Lout=60, prefer=prefer),
               conv(3, 5, 20, 16, 900, stride=3, pl=0, dil=27, prefer=prefer), conv(3, 5, 20, 16, 900, stride=9, pl=0, prefer=prefer),
               conv(1, 8, 256, 16, 64, prefer=prefer), conv(1, 8, 256, 20, 64, prefer=prefer), conv(2, 8, 256, 4, 64, stride=2, dil=2, pl=2, prefer=prefer),
               convT(65536, 8, 8, 4, 31, 2, prefer=prefer), convT(1, 8, 8, 4, 31, 2, trim=-2, prefer=prefer), convT(1, 8, 8, 4, 31, 2, act=4, prefer=prefer),
               convT(1, 8, 8, 4, 31, 2, act=1, noab=True, prefer=prefer), convT(1, 8, 8, 4, 31, 2, post=4, prefer=prefer), convT(1, 8, 8, 4, 31, 2, pl=-1, prefer=prefer),
               convT(1, 8, 8 * 65536, 4, 31, 2, prefer=prefer), convT(2, 8, 20, 6, 63, 2, ydt=BF16, prefer=prefer), convT(2, 8, 20, 19, 63, 8, ydt=BF16, prefer=prefer)]
        # the grid limits that an int-sized call can reach: position tiles x channel tiles (x phases) past 2^31.  (The other two,
        # B ks > 65535 and the transposed channels-per-lane grid x, need B >= 1024 with waves < 4096 or Lout > 2^31: unreachable)
        cs += [conv(1, 1, 524280, 1, 2000000000, prefer=prefer), convT(1, 1, 524280, 4096, 12800, 2048, prefer=prefer)]
        # zero sizes; where conv_ops cannot even form the call (a zero stride or dilation, a negative length) the recorder made it
        # at the position-per-lane entry point itself, so these are prefer 2 only
        cs += [conv(0, 8, 8, 3, 64, Lout=64, prefer=prefer), conv(1, 0, 8, 3, 64, prefer=prefer), conv(1, 8, 0, 3, 64, prefer=prefer),
               convT(0, 8, 8, 4, 31, 2, prefer=prefer), convT(1, 0, 8, 4, 31, 2, prefer=prefer), convT(1, 8, 0, 4, 31, 2, prefer=prefer)]
    cs += [pc("conv", B=1, Cin=8, Lin=64, Cout=8, Lout=64, K=3, stride=s, pl=1, dil=d, prefer=2) for s, d in ((0, 1), (-1, 1), (1, 0), (1, -2))]
    cs += [pc("conv", B=1, Cin=8, Lin=Lin, Cout=8, Lout=Lout, K=K, pl=1, prefer=2) for Lin, Lout, K in ((64, 0, 3), (64, -3, 3), (0, 64, 3), (64, 64, 0))]
    cs += [pc("convT", B=1, Cin=8, Lin=Lin, Cout=8, Lout=Lout, K=K, stride=s, pl=1, prefer=2)
           for Lin, Lout, K, s in ((31, 62, 4, 0), (31, 0, 4, 2), (0, 62, 4, 2), (31, 62, 0, 2))]
    # ---- weight gradient: tap counts, CV 15 / 16, the activation's side, the LDS budget, grid limits, refusals
    for K in (1, 3, 4, 5, 7, 8, 9, 16):
        for CV in (15, 16, 65):
            for act_on, act in ((0, 1), (1, 0), (1, 2)):
                for B, CU, LV, s, dil in ((3, 9, 300, 1, 1), (4, 2048, 215, 1, 1), (1, 64, 4000, 4, 40)):
                    cs.append(wgrad(B, CU, CV, K, LV, stride=s, pl=(K - 1) * dil // 2, dil=dil, act_on=act_on, act=act))
    cs += [wgrad(1, 8, 8, 17, 64), wgrad(1, 8, 8, 3, 64, act_on=2), wgrad(1, 8, 8, 3, 64, act=3), wgrad(1, 8, 8, 3, 64, act=1, noab=True),
           wgrad(1, 8, 4 * 65535 + 1, 5, 64), wgrad(1, 2 * 65535 + 1, 8, 11, 64), wgrad(1, 64 * 65535 + 1, 16, 7, 64), wgrad(1, 8, 64 * 65535 + 1, 7, 64),
           wgrad(1, 8, 8, 3, 64, pl=-1), pc("wgrad", B=1, CU=8, CV=8, MU=62, LV=64, K=3, stride=0, pl=0, dil=1)]
    # ---- the shapes of test_conv_query_matches_launch
    cs += [conv(3, 9, 20, 3, 200, xdt=BF16), convT(2, 8, 20, 4, 50, 2, ydt=BF16), conv(1, 352, 64, 3, 16), wgrad(1, 8, 16, 7, 64, pl=3),
           wgrad(1, 8, 8, 7, 64, pl=3)]
    seen, out = set(), []
    for c in cs:
        k = key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


PLAN_CASES = _plan_cases()


def query(c):
    """the row of a case through the host queries of the built library: [entry, rc, word (, Lp, lead, phases, workspace floats)]"""
    from kalle_audio_amd import conv_ops, conv_train
    f = full(c)
    ab = dict(act=f["act"], act_params=not f["noab"])
    if f["kind"] == "wgrad":
        rc, r = conv_train.conv_wgrad_plan(f["B"], f["CU"], f["CV"], f["MU"], f["LV"], K=f["K"], stride=f["stride"], padding=f["pl"],
                                           dilation=f["dil"], act_on=f["act_on"], **ab)
        return ["wgrad" if r else None, rc, r["word"] if r else 0]
    ep = dict(residual=f["res"], out_scale=f["scale"], accumulate=f["acc"], tanh=f["tanh"], post_act=f["post"], want_raw=f["raw"], post_params=not f["noab"])
    kw = dict(stride=f["stride"], padding=f["pl"], x_f32=f["xdt"] == F32, y_f32=f["ydt"] == F32, prefer=f["prefer"], **ab, **ep)
    if f["kind"] == "conv":
        rc, r = conv_ops.conv_plan(f["B"], f["Cin"], f["Lin"], f["Cout"], f["Lout"], f["K"], dilation=f["dil"], **kw)
    else:
        rc, r = conv_ops.conv_transpose_plan(f["B"], f["Cin"], f["Lin"], f["Cout"], f["Lout"], f["K"], **kw)
    if rc != 0:
        return [None, rc, 0]            # (the table names the function that refused: compared by the caller)
    row = [FAMILY_ENTRY[r["family"]], rc, r["word"]]
    return row + [r["Lp"], r["lead"], r["phases"], r["ws_floats"]] if r["family"] >= 5 else row
