"""CPU side of the decode step's one sequencer (csrc/llasa.hip: decode_step behind the six exported steps): every refusal returns
before any HIP call, so the library is driven without a device.  One table of refusals per entry point, the return codes as the
four separate step functions gave them before they were merged (recorded from that build); a NULL field in a LATER layer is
refused by all four forms before anything is launched; the one-row workspace is the R-row one at R = 1 without xn; and
ops.llama_decode_plan tells the weight format from the tuple length."""
import ctypes

import pytest
import torch

OK, ERR_ARG = 0, -1
FAKE = 4096                         # a non-NULL pointer for calls that must return before touching memory
BASE = dict(n=1, x=FAKE, out=FAKE, H=2, Hkv=1, inner=16, hd=64, rows=40, cos=FAKE, sin=FAKE, ws=FAKE, layers=True)
# entry point -> (descriptor is the e4m3 one, R-row form, takes head_dim)
FORMS = {"kalle_llama_decode_step": (False, False, False), "kalle_llama_decode_step_hd": (False, False, True),
         "kalle_llama_decode_step_w8": (True, False, True), "kalle_llama_decode_step_rows": (False, True, True),
         "kalle_llama_decode_step_rows_w8": (True, True, True)}

COMMON = [dict(Hkv=3), dict(Hkv=0), dict(H=0), dict(inner=0), dict(inner=12), dict(H=513), dict(rows=0), dict(n=0), dict(n=-1),
          dict(x=None), dict(out=None), dict(ws=None), dict(cos=None), dict(sin=None), dict(layers=None), dict(hole=(0, "wug")),
          dict(hole=(0, "kv_cache")), dict(hole=(0, "input_norm"))]
HD = [dict(hd=32), dict(hd=96), dict(hd=0), dict(hd=128, H=257)]
BF16 = [dict(inner=32776)]                                  # a multiple of 8 past the GEMV's K limit
W8 = [dict(inner=8), dict(inner=24), dict(inner=32784), dict(hole=(0, "sqkv")), dict(hole=(0, "so")), dict(hole=(0, "sug")),
      dict(hole=(0, "sdown"))]
ONE = [dict(t0=-1), dict(t0=40), dict(t0=41)]
ROWS = [dict(R=0), dict(R=17, t0=(0,) * 17), dict(R=-1), dict(t0=(0, 40, -1)), dict(t0=(0, 15360, 2), rows=20000), dict(t0=None, R=3)]
# (code, keyword overrides): KALLE_ERR_ARG for every refusal; every row inactive is KALLE_OK with nothing launched
TABLE = {name: [(ERR_ARG, kw) for kw in COMMON + (HD if hd else []) + (W8 if w8 else BF16) + (ROWS if batched else ONE)] +
               ([(OK, dict(t0=(-1, -1, -1))), (ERR_ARG, dict(t0=(-1, -1, -1), hole=(0, "wo")))] if batched else [])
         for name, (w8, batched, hd) in FORMS.items()}
WS_TABLE = {"kalle_llama_decode_ws_bytes": [(0, 1, 8), (2, 0, 8), (2, 1, 0), (-1, 1, 8)],
            "kalle_llama_decode_ws_bytes_hd": [(0, 1, 8, 64), (2, 0, 8, 64), (2, 1, 0, 64), (2, 1, 8, 32), (2, 1, 8, 96)],
            "kalle_llama_decode_ws_bytes_rows": [(0, 2, 1, 8, 64), (17, 2, 1, 8, 64), (3, 2, 1, 8, 32), (3, 0, 1, 8, 64), (3, 2, 0, 8, 64),
                                                 (3, 2, 1, 0, 64), (3, 513, 1, 8, 64), (3, 257, 1, 8, 128), (3, 2, 1, 32776, 64)]}


@pytest.fixture(scope="module")
def lib():
    from kalle_audio_amd import _lib
    return _lib.load()


def step(lib, name, hole=None, **over):
    """the entry point `name` on BASE with `over`; hole = (layer, field): that descriptor field is NULL"""
    from kalle_audio_amd import _lib
    w8, batched, hd = FORMS[name]
    a = dict(BASE, t0=(0, 1, 2) if batched else 3)
    a.update(over)
    desc = _lib.LlamaLayerW8 if w8 else _lib.LlamaLayer
    arr = (desc * max(a["n"], 1))()
    for l, d in enumerate(arr):
        for f, _ in desc._fields_:
            setattr(d, f, None if hole == (l, f) else FAKE)
    args = [ctypes.cast(arr, ctypes.c_void_p) if a["layers"] else None, a["n"], a["x"], a["out"]]
    if batched:
        t0 = a["t0"]
        args.append(a.get("R", 0 if t0 is None else len(t0)))
        pos = None if t0 is None else ctypes.cast((ctypes.c_int32 * len(t0))(*t0), ctypes.c_void_p)
    else:
        pos = a["t0"]
    args += [a["H"], a["Hkv"], a["inner"]] + ([a["hd"]] if hd else []) + [ctypes.c_float(1e-5), pos, a["rows"], a["cos"], a["sin"],
                                                                         a["ws"], None]
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("name,code,kw", [pytest.param(n, c, kw, id=f"{n[19:]}-{kw}") for n, rows in TABLE.items() for c, kw in rows])
def test_refusals_return_the_recorded_code_and_leave_no_attention_plan(lib, name, code, kw):
    assert step(lib, name, **kw) == code
    assert lib.kalle_attn_last_plan() == 0


@pytest.mark.parametrize("name", list(WS_TABLE))
def test_workspace_size_refusals(lib, name):
    for a in WS_TABLE[name]:
        assert getattr(lib, name)(*a) == ERR_ARG, a


@pytest.mark.parametrize("name", list(FORMS))
def test_a_hole_in_the_second_layer_is_refused_before_the_first_runs(lib, name):
    """KALLE_ERR_ARG, not the KALLE_ERR_LAUNCH of a first layer launched without a device: nothing may run before the refusal"""
    from kalle_audio_amd import _lib
    for f, _ in (_lib.LlamaLayerW8 if FORMS[name][0] else _lib.LlamaLayer)._fields_:
        assert step(lib, name, n=2, hole=(1, f)) == ERR_ARG, f
        assert lib.kalle_attn_last_plan() == 0, f


def test_one_row_workspace_is_the_rows_workspace_at_one_row_without_xn(lib):
    for H, inner, hd in ((2, 8, 64), (2, 8, 128), (32, 8192, 64), (24, 8192, 128), (2, 2056, 64)):
        xn = max(H * hd, inner) * 2                          # bf16 [1][max(D, inner)], the last region the header documents
        assert lib.kalle_llama_decode_ws_bytes_hd(H, 1, inner, hd) == lib.kalle_llama_decode_ws_bytes_rows(1, H, 1, inner, hd) - xn
    assert lib.kalle_llama_decode_ws_bytes(2, 1, 8) == lib.kalle_llama_decode_ws_bytes_hd(2, 1, 8, 64)


@pytest.mark.parametrize("n", [6, 10])
def test_plan_refuses_a_layer_tuple_of_neither_format(lib, n):
    from kalle_audio_amd import ops
    assert n not in (len(ops.BF16_FIELDS), len(ops.W8_FIELDS))
    with pytest.raises(AssertionError):
        ops.llama_decode_plan([tuple(torch.zeros(1) for _ in range(n))], 2, 1, 16, "cpu")
