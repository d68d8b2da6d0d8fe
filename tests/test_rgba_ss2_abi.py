"""bk_apply_rgba_ss2_device at the C-ABI boundary (no GPU), as test_rgba_abi.py checks its siblings: declared in
include/blinky_hip.h, exported by libblinkyhip.so, bound by blinky_amd/ffi.py; a host-only (BK_DEVICE_NONE) context refuses it with
BK_E_STATE instead of touching a device, and a NULL context or destination is BK_E_INVALID."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bk_apply_rgba_ss2_device"
BK_E_INVALID, BK_E_STATE = -1, -6


def test_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blinky_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bk_[a-z_0-9]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "blinky_amd", "libblinkyhip.so")], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    import blinky_amd.ffi as ffi
    assert NAME in declared, f"{NAME} is not declared in blinky_hip.h"
    assert NAME in exported, f"{NAME} is not exported by libblinkyhip.so"
    assert NAME in ffi.EXPORTS and getattr(ffi.lib, NAME).argtypes is not None, f"{NAME} is not bound by blinky_amd/ffi.py"
    assert len(getattr(ffi.lib, NAME).argtypes) == 9       # ... with the nullable LUT as its last argument
    assert callable(ffi.Context.apply_rgba_ss2_device)


@pytest.mark.parametrize("with_lut", [False, True])
def test_host_only_context_refuses_it(with_lut):
    import blinky_amd as bk
    ffi = bk.ffi
    ctx = bk.Context(ffi.DEVICE_NONE)
    ctx.resize(64, 48)
    lut = np.zeros((4, 6, 256), np.uint8) if with_lut else None
    fake = C.c_void_p(4096)                                    # never dereferenced: the call is refused before any device work
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.apply_rgba_ss2_device(fake, 4 * 32, 4 * 32 * 24, lut=lut)
    # NULL arguments are invalid whatever the context
    lp = None if lut is None else lut.ctypes.data_as(C.c_void_p)
    assert ffi.lib.bk_apply_rgba_ss2_device(ctx._h, 0, 1, None, 4 * 32, 4 * 32 * 24, 0, 0, lp) == BK_E_INVALID
    assert ffi.lib.bk_apply_rgba_ss2_device(None, 0, 1, fake, 4 * 32, 4 * 32 * 24, 0, 0, lp) == BK_E_INVALID
    ctx.close()
