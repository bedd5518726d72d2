"""Cases, inputs and the documented workspace layout of kalle_llasa_frame_head2_rows (the mean || log-scale head of model.Llasa),
shared by tests/test_llasa_head2_cpu.py and tests/test_llasa_head2_gpu.py.  d2 = 2 lat.  Shapes: the smallest at which each path
of the sequence is taken - one row at d2 = 16 (two lanes per weight row), a hole in the middle of the mask, all 16 rows at
d2 = 48 (no power of two: G = 8 lanes per weight row, six of them loaded; the two halves split inside one pass of the W2 walk),
the shipped shape (lat 64, D 2048: d2 = 128, exactly one pass), the bound (lat 256: d2 = 512, G = 64, four passes, the halves in
different passes) with a K tail in the skinny GEMM (3072 = 12 K blocks of 256 over 4 waves), and the bound with rows masked off
at the 16-row width."""
import torch

EPS = 1e-5
MAX_ROWS = 16
MAX_LAT = 256
ERF_U, DIV_U, EXP_U = 8.0, 15.0, 27.0       # ALLOW["ERF"] / ["DIV"] / ["EXP"] of tests/test_norm_elementwise_gpu.py (measured there, x 4)

# name -> R, D, lat, inactive rows
CASES = {
    "r1": dict(R=1, D=128, lat=8, inactive=()),
    "r3-hole": dict(R=3, D=128, lat=8, inactive=(1,)),
    "r16-lat24": dict(R=16, D=256, lat=24, inactive=()),
    "r2-lat64": dict(R=2, D=2048, lat=64, inactive=()),
    "r5-lat256": dict(R=5, D=3072, lat=256, inactive=()),
    "r16-lat256-holes": dict(R=16, D=2048, lat=256, inactive=(0, 3, 8, 9, 15)),
}
SMALL_H = dict(R=2, D=256, lat=24, inactive=(), hscale=1e-3)      # mean(h^2) = 1e-6 against eps = 1e-5: eps decides the norm
# b2's log-scale half runs from -6 to 2: exp spans three decades (2.5e-3 .. 7.4) and (1 - logs) changes sign
WIDE_SCALE = dict(R=2, D=256, lat=64, inactive=(), wide=True)


def inputs(c, seed=0):
    """CPU tensors: h fp32 [R, D], norm fp32 [D], w1 [d2, D] / w2 [d2, d2] / wa [D, lat] bf16, b1 / b2 [d2] / ba [D] fp32, noise
    fp32 [R, lat].  b2: 1 + 0.5 n for the mean half, -1 + 0.5 n for the log-scale half (wide: linspace(-6, 2) + 0.1 n)"""
    R, D, lat = c["R"], c["D"], c["lat"]
    d2 = 2 * lat
    g = torch.Generator().manual_seed(2000 * R + D + lat + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = dict(h=rn(R, D) * c.get("hscale", 1.0) * 3.0, norm=1 + 0.1 * rn(D),
             w1=(rn(d2, D) / D ** 0.5).to(torch.bfloat16), b1=0.5 * rn(d2),
             w2=(rn(d2, d2) / d2 ** 0.5).to(torch.bfloat16),
             b2=torch.cat([1.0 + 0.5 * rn(lat), -1.0 + 0.5 * rn(lat)]),
             wa=(rn(D, lat) / lat ** 0.5).to(torch.bfloat16), ba=0.5 * rn(D), noise=rn(R, lat))
    if c.get("wide"):
        x["b2"][lat:] = torch.linspace(-6.0, 2.0, lat) + 0.1 * rn(lat)
        x["w2"][lat:] = (0.25 * x["w2"][lat:].float()).to(torch.bfloat16)      # (the bias, not W2 . a, places logs)
    return x


def ws_layout(R, D, lat):
    """the header's layout: name -> (byte offset, bytes of data, torch dtype, row width); and the total size"""
    out, o = {}, 0
    for name, n, dt in (("xn", D, torch.bfloat16), ("h1", 2 * lat, torch.float32), ("a", 2 * lat, torch.bfloat16),
                        ("s", lat, torch.float32), ("lat", lat, torch.bfloat16)):
        nb = R * n * (4 if dt == torch.float32 else 2)
        out[name] = (o, nb, dt, n)
        o += (nb + 63) & ~63
    return out, o
