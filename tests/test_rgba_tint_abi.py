"""The truecolour rubix entry points at the C-ABI boundary (no GPU): bk_apply_rgba_tinted_device and bk_create_tintmap_rgba are
declared in include/blinky_hip.h, exported by libblinkyhip.so and bound by blinky_amd/ffi.py; a host-only (BK_DEVICE_NONE) context
refuses the apply; and bk_create_tintmap_rgba holds the reference's blend (create_palmap, fisheye.c:863-901, without the palette
search that follows it there) for every order of the channels over the four bytes."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bk_apply_rgba_tinted_device", "bk_create_tintmap_rgba")
BK_E_INVALID, BK_E_STATE = -1, -6
TINT = np.array([[255, 255, 255], [0, 0, 255], [255, 0, 0], [255, 255, 0], [255, 0, 255], [0, 255, 255]], np.int64)   # fisheye.c:866-886


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
    assert callable(getattr(ffi.Context, "apply_rgba_tinted_device"))
    assert callable(ffi.create_tintmap_rgba)


def test_host_only_context_refuses_the_apply():
    import blinky_amd as bk
    ffi = bk.ffi
    ctx = bk.Context(ffi.DEVICE_NONE)
    ctx.resize(64, 48)
    lut = ffi.create_tintmap_rgba()
    fake = C.c_void_p(4096)                                    # never dereferenced: the call is refused before any device work
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.apply_rgba_tinted_device(fake, 4 * 64, 4 * 64 * 48, lut)
    # NULL arguments are invalid whatever the context
    lp = lut.ctypes.data_as(C.c_void_p)
    f = ffi.lib.bk_apply_rgba_tinted_device
    assert f(None, 0, 1, fake, 4 * 64, 4 * 64 * 48, 0, 0, lp) == BK_E_INVALID
    assert f(ctx._h, 0, 1, None, 4 * 64, 4 * 64 * 48, 0, 0, lp) == BK_E_INVALID
    assert f(ctx._h, 0, 1, fake, 4 * 64, 4 * 64 * 48, 0, 0, None) == BK_E_INVALID
    with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
        ctx.apply_rgba_tinted_device(fake, 4 * 64, 4 * 64 * 48, None)
    ctx.close()


def transcription(channel_of_byte):
    """fisheye.c:863-901 in numpy over int64: v + ((42 * (tint - v)) >> 8), clipped; a byte that is no colour channel keeps its value"""
    v = np.arange(256, dtype=np.int64)
    percent = 256 // 6
    out = np.empty((4, 6, 256), np.uint8)
    for c, ch in enumerate(channel_of_byte):
        for j in range(6):
            out[c, j] = v if ch not in (0, 1, 2) else np.clip(v + ((percent * (TINT[j, ch] - v)) >> 8), 0, 255)
    return out


def test_tintmap_equals_the_reference_blend_for_every_byte_order():
    import blinky_amd.ffi as ffi
    identity = np.arange(256, dtype=np.uint8)
    orders = list(itertools.permutations((0, 1, 2, 3)))
    assert len(orders) == 24
    for order in orders:
        got = ffi.create_tintmap_rgba(order)
        assert got.shape == (4, 6, 256) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, transcription(order), err_msg=f"channel_of_byte {order}")
        a = order.index(3)
        for j in range(6):
            np.testing.assert_array_equal(got[a, j], identity, err_msg=f"alpha row, order {order}, plate {j}")
    np.testing.assert_array_equal(ffi.create_tintmap_rgba(), transcription((0, 1, 2, 3)))          # the default: RGBA
    # two alpha bytes (and values beyond 3 / below 0): both rows are identities
    for order in ((0, 3, 1, 3), (3, 2, 3, 7), (-1, 0, 1, -5)):
        got = ffi.create_tintmap_rgba(order)
        np.testing.assert_array_equal(got, transcription(order), err_msg=f"channel_of_byte {order}")
        for c, ch in enumerate(order):
            if ch not in (0, 1, 2):
                for j in range(6):
                    np.testing.assert_array_equal(got[c, j], identity)
    # the blend is not the identity where it applies: plate 0 (white) brightens, and the rows of different plates differ
    rgba = ffi.create_tintmap_rgba()
    assert (rgba[0, 0, :249] > identity[:249]).all() and not np.array_equal(rgba[0, 1], rgba[0, 2])
