"""bk_plate_footprint / bk_upload_plate_rgba_footprint / bk_upload_plate_rgba_footprint_device at the C-ABI boundary (no GPU), as
test_rgba_ss2_abi.py checks its entry point: declared in include/blinky_hip.h, exported by libblinkyhip.so, bound by blinky_amd/ffi.py with
Context methods; a host-only (BK_DEVICE_NONE) context refuses all three with BK_E_STATE instead of touching a device, and a NULL context,
source or rect is BK_E_INVALID."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bk_plate_footprint": ("plate_footprint", 5),
         "bk_upload_plate_rgba_footprint": ("upload_plate_rgba_footprint", 5),
         "bk_upload_plate_rgba_footprint_device": ("upload_plate_rgba_footprint_device", 5)}
BK_E_INVALID, BK_E_STATE = -1, -6


def test_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blinky_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bk_[a-z_0-9]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "blinky_amd", "libblinkyhip.so")], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    import blinky_amd.ffi as ffi
    for name, (method, nargs) in NAMES.items():
        assert name in declared, f"{name} is not declared in blinky_hip.h"
        assert name in exported, f"{name} is not exported by libblinkyhip.so"
        assert name in ffi.EXPORTS and getattr(ffi.lib, name).argtypes is not None, f"{name} is not bound by blinky_amd/ffi.py"
        assert len(getattr(ffi.lib, name).argtypes) == nargs
        assert callable(getattr(ffi.Context, method))


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "blinky_hip.h")).read()
    conventions = text[:text.index("#ifndef BLINKY_HIP_H")]
    for name in NAMES:
        assert name in conventions, f"{name} is missing from the TRUECOLOUR sentence of the conventions block"
    flat = " ".join(text.split()).lower().replace("* ", "")
    assert "source texels outside rect are never read" in flat
    assert "no counterpart in the reference beyond `display`" in flat


def test_host_only_context_refuses_them():
    import blinky_amd as bk
    ffi = bk.ffi
    ctx = bk.Context(ffi.DEVICE_NONE)
    ctx.resize(64, 48)
    fake = C.c_void_p(4096)                                    # never dereferenced: the calls are refused before any device work
    src = np.zeros((48, 48, 4), np.uint8)
    rect, n = (C.c_int * 4)(), C.c_int()
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.plate_footprint(0)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.plate_footprint(0, tiles=True)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.upload_plate_rgba_footprint(0, 0, src)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.upload_plate_rgba_footprint_device(0, 0, fake, 4 * 48)
    assert ffi.lib.bk_plate_footprint(ctx._h, 0, rect, C.byref(n), None) == BK_E_STATE
    # NULL arguments are invalid whatever the context
    assert ffi.lib.bk_plate_footprint(None, 0, rect, C.byref(n), None) == BK_E_INVALID
    assert ffi.lib.bk_plate_footprint(ctx._h, 0, None, C.byref(n), None) == BK_E_INVALID
    for name in ("bk_upload_plate_rgba_footprint", "bk_upload_plate_rgba_footprint_device"):
        assert getattr(ffi.lib, name)(None, 0, 0, fake, 4 * 48) == BK_E_INVALID
        assert getattr(ffi.lib, name)(ctx._h, 0, 0, None, 4 * 48) == BK_E_INVALID
    ctx.close()
