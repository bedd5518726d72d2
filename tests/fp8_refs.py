"""CPU references of the weight-only e4m3 decode path (include/kalle_hip.h, "weight-only FP8 decoding"), checked by
tests/test_fp8_refs_cpu.py and used by tests/test_decode_w8_gpu.py and tests/test_llasa_w8_gpu.py:
  decode_table()       the 256 values of OCP e4m3fn, built from the format's definition (float64; 0x7F and 0xFF NaN)
  decode_table_fnuz()  the MI300 e4m3fnuz values of the same codes (bias 8, 0x80 NaN): a deliberately wrong decoding
  quantize_ref(w)      the quantiser's contract in torch fp32 on the CPU
  lossless_weights()   rows of 2^e_n x random e4m3 values holding +-448: bf16 weights that quantise to themselves"""
import torch

E4M3_MAX = 448.0


def decode_table():
    t = torch.empty(256, dtype=torch.float64)
    for c in range(256):
        sign, exp, man = -1.0 if c & 0x80 else 1.0, (c >> 3) & 15, c & 7
        if exp == 15 and man == 7:
            t[c] = float("nan")
        elif exp == 0:
            t[c] = sign * (man / 8.0) * 2.0 ** -6
        else:
            t[c] = sign * (1 + man / 8.0) * 2.0 ** (exp - 7)
    return t


def decode_table_fnuz():
    t = torch.empty(256, dtype=torch.float64)
    for c in range(256):
        sign, exp, man = -1.0 if c & 0x80 else 1.0, (c >> 3) & 15, c & 7
        if c == 0x80:
            t[c] = float("nan")
        elif exp == 0:
            t[c] = sign * (man / 8.0) * 2.0 ** -7
        else:
            t[c] = sign * (1 + man / 8.0) * 2.0 ** (exp - 8)
    return t


def quantize_ref(w):
    """w [N, K] (any float dtype, CPU) -> (codes uint8 [N, K], scale fp32 [N]): scale = amax / 448 (1 for an all-zero row),
    t = w / scale, both IEEE fp32 divisions; clamp to +-448 (unclamped, 500 becomes NaN in the cast); round to nearest even"""
    w = w.detach().cpu().float()
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.tensor(E4M3_MAX, dtype=torch.float32), torch.ones_like(amax))
    t = (w / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    return t.to(torch.float8_e4m3fn).view(torch.uint8), scale


def quantize_t(w):
    """the fp32 value the code is rounded from (before the clamp), for the property checks"""
    w = w.detach().cpu().float()
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.tensor(E4M3_MAX, dtype=torch.float32), torch.ones_like(amax))
    return w / scale[:, None]


def random_codes(shape, g):
    """uniform random bytes without the two NaN codes"""
    c = torch.randint(0, 256, shape, generator=g, dtype=torch.int16)
    c = torch.where((c & 0x7F) == 0x7F, c - 1, c)
    return c.to(torch.uint8)


def lossless_weights(N, K, g, emin=-12, emax=4):
    """(w bf16 [N, K], codes uint8 [N, K], scale fp32 [N]): w[n] = 2^e_n x e4m3(codes[n]), each row holding +448 and -448 and no
    negative zero, so that amax / 448 is 2^e_n exactly and the quantiser returns (codes, 2^e_n).  Exact in bf16: 4 significant bits
    out of 8, exponents well inside the range."""
    codes = random_codes((N, K), g)
    codes = torch.where(codes == 0x80, torch.zeros_like(codes), codes)
    for n in range(N):
        a, b = torch.randperm(K, generator=g)[:2].tolist()
        codes[n, a], codes[n, b] = 0x7E, 0xFE
    e = torch.randint(emin, emax + 1, (N,), generator=g)
    scale = (2.0 ** e.double()).float()
    w = (decode_table()[codes.long()] * scale.double()[:, None])
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.double(), w)
    return wb, codes, scale
