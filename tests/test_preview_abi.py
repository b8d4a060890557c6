"""The order preview's boundary: me_order_preview and me_service_preview_order are declared in the headers,
exported by the library and prototyped for ctypes; PREVIEW_DTYPE lays its fields out as the C compiler lays out
me_preview; preview_notional joins the two halves of the 128-bit notional. No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import preview_model as pm
from tests.abi_layout import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("first_price_q4", "last_price_q4", "opp_price_q4", "notional_hi", "notional_lo", "filled_qty", "remaining_qty",
          "fill_count", "levels", "status", "reason", "flags", "pad")


def test_declared_exported_and_prototyped(built):
    from matching_engine_amd import _abi

    eh = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    sh = open(os.path.join(ROOT, "include", "me_service.h")).read()
    assert re.search(r"\bint\s+me_order_preview\s*\(\s*me_engine\s*\*\s*e\s*,\s*const\s+me_order_soa\s*\*\s*q\s*,\s*size_t\s+n\s*,"
                     r"\s*me_preview\s*\*\s*out\s*\)\s*;", eh)
    assert re.search(r"\bint\s+me_service_preview_order\s*\(\s*me_service\s*\*\s*s\s*,\s*const\s+me_order_request\s*\*\s*req\s*,"
                     r"\s*int32_t\s+tif\s*,\s*me_preview\s*\*\s*out\s*\)\s*;", sh)
    assert re.search(r"typedef\s+struct\s+me_preview\b", eh)
    for name, v in (("ME_PV_HAS_OPP", 1), ("ME_PV_CROSSES", 2), ("ME_PV_RESTS", 4)):
        assert re.search(rf"#define\s+{name}\s+{v}u\b", eh), name
    syms = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], check=True, capture_output=True,
                          text=True).stdout
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("me_order_preview", "me_service_preview_order"):
        assert re.search(rf"\bT {name}\b", syms), name
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES, name
    assert (_abi.PV_HAS_OPP, _abi.PV_CROSSES, _abi.PV_RESTS) == (1, 2, 4) == (pm.PV_HAS_OPP, pm.PV_CROSSES, pm.PV_RESTS)
    # a null engine or service is refused, not dereferenced
    lib = _abi.load()
    assert lib.me_order_preview(None, None, 0, None) == _abi.ME_E_INVALID
    assert lib.me_service_preview_order(None, None, 0, None) == _abi.ME_E_INVALID


def test_preview_dtype_matches_the_header(built, tmp_path):
    from matching_engine_amd import _abi

    c = c_layout(tmp_path, "me_engine.h", "me_preview", FIELDS)
    dt = _abi.PREVIEW_DTYPE
    assert dt.itemsize == 64 == c["sizeof"]
    assert dt.names == FIELDS
    for f in FIELDS:
        assert dt.fields[f][1] == c[f], (f, dt.fields[f][1], c[f])
    assert dt.fields["pad"][0].shape == (5,)
    assert dt == pm.PREVIEW_DTYPE  # the model restates it
    import matching_engine_amd as me

    assert me.PREVIEW_DTYPE is dt and me.preview_notional is _abi.preview_notional


def test_preview_notional_round_trips(built):
    from matching_engine_amd import _abi

    for v in (1 << 94, -(1 << 94), -1, 0, 1, (1 << 64) - 1, -(1 << 64), (1 << 127) - 1, -(1 << 127)):
        row = np.zeros(1, dtype=_abi.PREVIEW_DTYPE)[0]
        row["notional_hi"], row["notional_lo"] = v >> 64, v & ((1 << 64) - 1)
        assert _abi.preview_notional(row) == v == pm.notional(row), v
