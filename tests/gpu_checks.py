"""Shared checks of the -m gpu kernel-test files (test_norm_elementwise_gpu.py, test_conv_gpu.py): every element of an output
bounded by its own tolerance with the first offender reported, bit-exact comparison, and NaN-filled buffers around whatever a
call may write (`Guard` for a [rows][cols] window with a leading dimension, `guarded` / `clean` for a dense tensor)."""
import torch

U = 2.0 ** -24
NAN = float("nan")


def check(out, ref, tol, what, key=None, unit=None, measured=None):
    """`measured`: the caller's table of worst deviations in units of u * unit, updated under `key`; every element of `out` within `tol` of `ref` (NaN never passes); reports the count and the first offender"""
    out = out.double()
    if not torch.is_tensor(tol):
        tol = torch.tensor(float(tol), dtype=torch.float64, device=ref.device)
    tol = torch.broadcast_to(tol.double(), ref.shape)
    if key is not None:
        unit = torch.broadcast_to(torch.as_tensor(unit, dtype=torch.float64, device=ref.device), ref.shape)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    w = ref.shape[-1] if ref.dim() >= 1 and ref.numel() else 1
    out, ref, tol = out.reshape(-1, w), ref.reshape(-1, w), tol.reshape(-1, w)
    err = (out - ref).abs()
    if key is not None:
        un = unit.reshape(-1, w)
        ok = (un > 0) & ~torch.isnan(err)
        if ok.any():
            measured[key] = max(measured.get(key, 0.0), float((err[ok] / (U * un[ok])).max()))
    bad = (err > tol) | torch.isnan(out)
    if bad.any():
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound; first at (row {r}, col {c}): "
                             f"out {out[r, c].item():.9g} ref {ref[r, c].item():.9g} tol {tol[r, c].item():.3g}")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _exact(out, ref, what):
    """bit for bit (NaN patterns compare equal to any NaN)"""
    assert out.dtype == ref.dtype and out.shape == ref.shape, (what, out.dtype, ref.dtype, out.shape, ref.shape)
    bad = (_bits(out) != _bits(ref)) & ~(torch.isnan(out) & torch.isnan(ref))
    if bad.any():
        i = bad.reshape(-1).nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ; first at flat index {i}: "
                             f"out {out.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r}")


class Guard:
    """a [rows + 2][ld] buffer of NaN (or of random contents inside the window when `init`) whose [:rows, col0:col0 + cols]
    window a call may write: `.v` is the window, `.clean()` asserts that everything else is still NaN"""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, init=None, extra=2, col0=0):
        ld = ld or col0 + cols
        self.buf = torch.full((rows + extra, ld), NAN, device="cuda", dtype=dtype)
        self.rows, self.cols, self.col0 = rows, cols, col0
        if init is not None:
            self.buf[:rows, col0:col0 + cols] = init.to(dtype)
        self.v = self.buf[:rows, col0:col0 + cols]

    def clean(self, what):
        m = torch.ones_like(self.buf, dtype=torch.bool)
        m[:self.rows, self.col0:self.col0 + self.cols] = False
        stray = ~torch.isnan(self.buf[m])
        assert not stray.any(), (what, "stray writes", int(stray.sum()))

    def untouched(self, what):
        assert torch.isnan(self.buf).all(), (what, "output written by a rejected call")


def guarded(t, extra=64):
    """the dense tensor `t` inside a NaN-filled allocation (NaN before the first and after the last element); returns (buffer, view)"""
    n = t.numel()
    buf = torch.full((n + 2 * extra,), NAN, device="cuda", dtype=t.dtype)
    buf[extra:extra + n] = t.reshape(-1)
    return buf, buf[extra:extra + n].view(t.shape)


def clean(buf, view, what, extra=64):
    n = view.numel()
    assert torch.isnan(buf[:extra]).all() and torch.isnan(buf[extra + n:]).all(), (what, "stray writes")
