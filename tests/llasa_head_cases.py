"""Cases, inputs and the documented workspace layout of kalle_llasa_frame_head_rows, shared by tests/test_llasa_head_cpu.py and
tests/test_llasa_head_gpu.py.  Shapes: the smallest at which each path of the sequence is taken - one row, a hole in the middle,
all 16 rows with a latent dim that is no power of two (G = 4 lanes per weight row, three of them loaded), the reference's two
latent dims (64: one pass of the W2 walk; 512: G = 64 and four passes), D with a K tail in the skinny GEMM (3072 = 12 K blocks
of 256 over 4 waves) and rows masked off at the 16-row width."""
import torch

EPS = 1e-5
STD = 0.5
MAX_ROWS = 16
ERF_U, DIV_U = 8.0, 15.0       # ALLOW["ERF"] / ALLOW["DIV"] of tests/test_norm_elementwise_gpu.py (measured there, x 4)

# name -> R, D, dl, inactive rows
CASES = {
    "r1": dict(R=1, D=128, dl=16, inactive=()),
    "r3-hole": dict(R=3, D=128, dl=16, inactive=(1,)),
    "r16-dl24": dict(R=16, D=256, dl=24, inactive=()),
    "r2-dl64": dict(R=2, D=2048, dl=64, inactive=()),
    "r5-dl512": dict(R=5, D=3072, dl=512, inactive=()),
    "r16-dl512-holes": dict(R=16, D=2048, dl=512, inactive=(0, 3, 8, 9, 15)),
}
SMALL_H = dict(R=2, D=256, dl=24, inactive=(), hscale=1e-3)       # mean(h^2) = 1e-6 against eps = 1e-5: eps decides the norm


def inputs(c, seed=0):
    """CPU tensors: h fp32 [R, D], norm fp32 [D], w1 / w2 / wa bf16, b1 / b2 / ba fp32, noise fp32 [R, dl]"""
    R, D, dl = c["R"], c["D"], c["dl"]
    g = torch.Generator().manual_seed(1000 * R + D + dl + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(h=rn(R, D) * c.get("hscale", 1.0) * 3.0, norm=1 + 0.1 * rn(D),
                w1=(rn(dl, D) / D ** 0.5).to(torch.bfloat16), b1=0.5 * rn(dl),
                w2=(rn(dl, dl) / dl ** 0.5).to(torch.bfloat16), b2=1.0 + 0.5 * rn(dl),
                wa=(rn(D, dl) / dl ** 0.5).to(torch.bfloat16), ba=0.5 * rn(D), noise=rn(R, dl))


def ws_layout(R, D, dl):
    """the header's layout: name -> (byte offset, bytes of data, torch dtype, row width); and the total size"""
    out, o = {}, 0
    for name, n, dt in (("xn", D, torch.bfloat16), ("h1", dl, torch.float32), ("a", dl, torch.bfloat16), ("lat", dl, torch.bfloat16)):
        nb = R * n * (4 if dt == torch.float32 else 2)
        out[name] = (o, nb, dt, n)
        o += (nb + 63) & ~63
    return out, o
