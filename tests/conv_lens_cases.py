"""Cases of the ragged-batch conv entry points (kalle_*_lens, include/kalle_hip.h): tests/test_conv_lens_gpu.py runs them on the
device, tests/test_conv_lens_cpu.py checks without one that every case gets the kernel family it is meant for.

A case is a forward case of tests/test_conv_gpu.py (its builders C / T / F, imported) with B = 4 rows and `lens`, the rows'
input lengths: always one full row (Lin), one inactive row (0) and two drawn from 1, K - 1, 5 (under a dilation-9 pad of 27),
63, 64, 65 (the seams of the 64-position tiles and 16-position channels-per-lane tiles) and Lin - 1.  The shapes are the
smallest that cross each kernel's seams: more than one position tile (or 16-position tile), Cin off the chunk of 8, Cout off the
channel tile.  The plan word is not written down here: `plan(c)` asks the host query with `prefer` forced the way the entry
point is, `family` says which family the case is there for, and both files assert it.

The rows' output lengths are the layer's own formula per row (`out_len`): symmetric padding for the convs (the 'same' K = 2 s
conv behind nearest up-sampling keeps the length: pad 1 left, 2 right), (l - 1) s - 2 p + K for the transposed ones."""
from test_conv_gpu import BF16, C, F, F32, T  # noqa: F401


def L(family, c, lens, same=False):
    assert c["B"] == 4 and len(lens) == 4 and max(lens) == c["Lin"] and min(lens) == 0, c
    c = dict(c, family=family, lens=tuple(lens), same=same, plan=None)
    return c


def out_len(c, l):
    """outputs of a row of l inputs: the formula the case's Lout was made with (0 of 0: an inactive row)"""
    if l == 0:
        return 0
    if c["same"]:
        return l
    if c["entry"] in ("conv", "cfirst"):
        return max(0, (l + 2 * c["pl"] - c["dil"] * (c["K"] - 1) - 1) // c["stride"] + 1)
    return (l - 1) * c["stride"] - 2 * c["pl"] + c["K"]


def lens_out(c, lens=None):
    return tuple(out_len(c, l) for l in (c["lens"] if lens is None else lens))


def plan(c):
    """(return code, dict) of the host query for the case's shapes, prefer forced as the entry point is"""
    from kalle_audio_amd import conv_ops
    ep = dict(residual=c["res"], out_scale=c["scale"], accumulate=c["acc"], tanh=c["tanh"], post_act=c["post"], want_raw=c["raw"])
    kw = dict(stride=c["stride"], padding=c["pl"], x_f32=c["xdt"] == F32, y_f32=c["ydt"] == F32, act=c["act"],
              prefer=1 if c["entry"].startswith("cfirst") else 2, **ep)
    if c["entry"] in ("conv", "cfirst"):
        return conv_ops.conv_plan(c["B"], c["Cin"], c["Lin"], c["Cout"], c["Lout"], c["K"], dilation=c["dil"], **kw)
    return conv_ops.conv_transpose_plan(c["B"], c["Cin"], c["Lin"], c["Cout"], c["Lout"], c["K"], **kw)


def cid(c):
    keys = ("entry", "Cin", "Cout", "K", "stride", "dil", "Lin", "act", "post", "res", "acc", "tanh", "raw", "xdt", "ydt")
    return f"f{c['family']}-" + "-".join(f"{k}{c[k]}" for k in keys) + "-" + "_".join(map(str, c["lens"]))


CT = lambda **kw: C(0, entry="cfirstT", **kw)  # noqa: E731

CASES = [
    # ---- family 1: the fallback conv (gate, odd stride, mixed dtypes)
    L(1, C(0, B=4, Cin=9, Cout=65, K=3, Lin=130, act=4, tanh=True), (130, 0, 65, 2)),
    L(1, C(0, B=4, Cin=9, Cout=20, K=6, stride=3, pl=2, Lin=196, act=1, post=1, raw=True, res=True, scale=0.5, acc=True), (196, 5, 0, 195)),
    L(1, C(0, B=4, Cin=9, Cout=20, K=6, stride=3, pl=2, Lin=130, xdt=BF16, ydt=BF16, act=2), (64, 130, 0, 1)),
    # ---- family 2: k = 7 at dilation 1 / 3 / 9, k = 1 with a residual, strided, the 'same' conv behind nearest up-sampling
    L(2, C(0, B=4, Cin=9, Cout=33, K=7, pl=3, Lin=200, act=1, post=1, raw=True), (200, 0, 6, 129)),
    L(2, C(0, B=4, Cin=17, Cout=20, K=7, pl=9, dil=3, Lin=200, act=2, post=2), (63, 200, 0, 199)),
    L(2, C(0, B=4, Cin=8, Cout=9, K=7, pl=27, dil=9, Lin=130, act=1), (5, 0, 130, 65)),
    L(2, C(0, B=4, Cin=9, Cout=20, K=1, pl=0, Lin=200, res=True, post=1, raw=True), (1, 200, 64, 0)),
    L(2, C(0, B=4, Cin=9, Cout=4, K=7, pl=3, Lin=600, act=1, tanh=True), (600, 513, 0, 6)),                 # Cout <= 4: the 2 x 2 x 1 form
    L(2, C(0, B=4, Cin=9, Cout=20, K=4, stride=2, pl=1, Lin=300, act=1, post=2), (300, 0, 3, 64)),
    L(2, C(0, B=4, Cin=9, Cout=20, K=16, stride=8, pl=4, Lin=1200, act=2, raw=True, post=1), (1200, 15, 0, 1199)),
    L(2, C(0, B=4, Cin=9, Cout=20, K=4, pl=1, Lin=200, Lout=200, act=1, bias=False), (200, 3, 0, 65), same=True),
    L(2, C(0, B=4, Cin=9, Cout=20, K=3, Lin=200, act=3, scale=0.5, acc=True), (0, 200, 2, 64)),
    L(2, C(0, B=4, Cin=9, Cout=65, K=7, pl=3, Lin=200, xdt=BF16, ydt=BF16, act=1, res=True, raw=True, post=1), (200, 0, 63, 6)),
    # ---- family 3: the fallback transposed conv (mixed dtypes)
    L(3, T(0, 4, B=4, Cout=20, Lin=70, ydt=BF16, act=1), (70, 0, 1, 65)),
    L(3, T(0, 5, B=4, Cout=20, Lin=70, xdt=BF16, act=2), (5, 70, 0, 69)),
    # ---- family 4: transposed K = 4 / s = 2, K = 16 / s = 8, K = 11 / s = 5
    L(4, T(0, 2, B=4, Cout=20, Lin=200, act=1, post=1, raw=True), (200, 0, 3, 129)),
    L(4, T(0, 8, B=4, Cout=33, Cin=17, Lin=70, act=2, tanh=True), (1, 70, 0, 65)),
    L(4, T(0, 5, B=4, Cout=9, Lin=130, act=1, post=2), (130, 5, 64, 0)),
    L(4, T(0, 4, B=4, Cout=20, Lin=70, xdt=BF16, ydt=BF16, act=1, raw=True, post=1), (0, 63, 70, 7)),
    # ---- family 5: channels per lane, stride 1 (one with the workgroup-level input-channel split: ks > 1)
    L(5, F(0, B=4, Cin=9, Cout=260, K=7, pl=27, dil=9, Lin=70, act=1, tanh=True), (70, 0, 5, 65)),
    L(5, F(0, B=4, Cin=16, Cout=20, K=1, pl=0, Lin=70, res=True, post=1, raw=True), (17, 70, 0, 1)),
    L(5, F(0, B=4, Cin=512, Cout=64, K=3, Lin=40, act=2, res=True, acc=True, scale=0.7, post=1, raw=True), (40, 2, 0, 17)),
    L(5, F(0, B=4, Cin=9, Cout=20, K=4, pl=1, Lin=70, Lout=70, act=1, bias=False), (70, 3, 0, 64), same=True),
    # ---- family 6: the same strided
    L(6, F(0, B=4, Cin=9, Cout=20, K=4, stride=2, pl=1, Lin=70, act=1, post=1), (70, 0, 3, 64)),
    L(6, F(0, B=4, Cin=9, Cout=260, K=16, stride=8, pl=4, Lin=400, act=2, raw=True, post=3), (15, 400, 0, 399)),
    # ---- family 7: the same transposed
    L(7, CT(stride=2, K=4, pl=1, B=4, Cin=9, Cout=20, Lin=40, act=1, post=1, raw=True), (40, 0, 3, 17)),
    L(7, CT(stride=8, K=16, pl=4, B=4, Cin=9, Cout=260, Lin=20, act=2, tanh=True), (1, 20, 0, 19)),
    L(7, CT(stride=5, K=11, pl=3, B=4, Cin=17, Cout=5, Lin=40, act=1, scale=0.5), (40, 5, 16, 0)),
]
