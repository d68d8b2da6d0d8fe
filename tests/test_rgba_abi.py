"""The truecolour entry points at the C-ABI boundary (no GPU): bk_upload_plate_rgba, bk_upload_plate_rgba_device and
bk_apply_rgba_device are declared in include/blinky_hip.h, exported by libblinkyhip.so, bound by blinky_amd/ffi.py, and a
host-only (BK_DEVICE_NONE) context refuses each of them with an error instead of touching a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bk_upload_plate_rgba", "bk_upload_plate_rgba_device", "bk_apply_rgba_device")
BK_E_INVALID, BK_E_STATE = -1, -6


def test_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blinky_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bk_[a-z_0-9]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "blinky_amd", "libblinkyhip.so")], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    import blinky_amd.ffi as ffi
    for n in NAMES:
        assert n in declared, f"{n} is not declared in blinky_hip.h"
        assert n in exported, f"{n} is not exported by libblinkyhip.so"
        assert n in ffi.EXPORTS and getattr(ffi.lib, n).argtypes is not None, f"{n} is not bound by blinky_amd/ffi.py"
    for m in ("upload_plate_rgba", "upload_plate_rgba_device", "apply_rgba_device"):
        assert callable(getattr(ffi.Context, m))


def test_host_only_context_refuses_them():
    import blinky_amd as bk
    ffi = bk.ffi
    ctx = bk.Context(ffi.DEVICE_NONE)
    ctx.resize(64, 48)
    src = np.zeros((48, 48, 4), np.uint8)
    fake = C.c_void_p(4096)                                    # never dereferenced: the calls are refused before any device work
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        ctx.upload_plate_rgba(0, 0, src)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        ctx.upload_plate_rgba_device(0, 0, fake, 4 * 48)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.apply_rgba_device(fake, 4 * 64, 4 * 64 * 48)
    # NULL arguments are invalid whatever the context
    assert ffi.lib.bk_upload_plate_rgba(ctx._h, 0, 0, None, 4 * 48) == BK_E_INVALID
    assert ffi.lib.bk_upload_plate_rgba_device(ctx._h, 0, 0, None, 4 * 48) == BK_E_INVALID
    assert ffi.lib.bk_apply_rgba_device(ctx._h, 0, 1, None, 4 * 64, 4 * 64 * 48, 0, 0) == BK_E_INVALID
    assert ffi.lib.bk_apply_rgba_device(None, 0, 1, fake, 4 * 64, 4 * 64 * 48, 0, 0) == BK_E_INVALID
    ctx.close()
