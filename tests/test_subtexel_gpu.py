"""The sub-texel plane on the GPU (bk_set_subtexel, bk_read_subtexel, bk_set_lensmap_subtexel): what bk_build leaves in it on the device
path - fix-ups of flagged pixels included, by the compiled host module and by the interpreter - against the numpy plane model (libm-free
lenses) and against the host build paths bit for bit (tests/test_subtexel_cpu.py holds those two to each other); how the plane follows
the lensmap through its life; and that with the switch off a build is what it was."""
import time

import numpy as np
import pytest

import scripts as S
import subtexel_model as SM
import test_subtexel_cpu as TC

pytestmark = pytest.mark.gpu

NULL = SM.NULL
SIZE = TC.SIZE
STRIPES = [(0, 37), (37, 38), (38, SIZE[1])]                        # an odd cut, one row
_HOST = {}


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def host_plane(bk, lens, rows=None):
    """(offsets, tints, sub, display, scale) of the host build (one sequential scan) on a device-less context, once per module"""
    key = (lens, rows)
    if key not in _HOST:
        ctx = TC.host_ctx(bk, lens, SIZE, rows)
        off, tin, sub, display, scale, err = ctx.host_build_subtexel(2)
        assert err is None
        ctx.close()
        for a in (off, tin, sub):
            a.flags.writeable = False
        _HOST[key] = (off, tin, sub, display, scale)
    return _HOST[key]


def device_build(bk, lens, on, rows=None):
    ctx = TC.host_ctx(bk, lens, SIZE, rows, device=True)
    ctx.set_subtexel(on)
    display, scale = ctx.build()
    assert ctx.last_build_path()[0] == (1 if lens == "declined-hammer" else 0)
    return ctx, display, scale


# ---- 1. what a build leaves in the plane -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", sorted(SM.LIBM_FREE))
def test_build_equals_the_plane_model(bk, lens):
    for rows in [None] + STRIPES:
        ctx, display, scale = device_build(bk, lens, True, rows)
        off, _ = ctx.read_lensmap()
        sub = ctx.read_subtexel()
        want_off, want_sub = SM.plane_model(SM.build_params_head(ctx), SM.RAYS[lens])
        np.testing.assert_array_equal(off, want_off, err_msg=f"rows {rows}")
        np.testing.assert_array_equal(sub, want_sub, err_msg=f"rows {rows}")
        assert ctx.last_build_fixups() == (0, 0)                    # no libm: nothing flagged
        ctx.close()


@pytest.mark.parametrize("fixups", ["host module", "interpreter"])
@pytest.mark.parametrize("lens", ["panini", "hammer", "quincuncial", "declined-hammer", "integrated_arc"])
def test_build_equals_the_host_build_bit_for_bit(bk, lens, fixups, request, monkeypatch):
    import os
    monkeypatch.chdir(os.path.dirname(TC.HERE))                     # (the examples' paths are relative to the repository root)
    if fixups == "host module":
        bk.debug_set_option("host_module", 1)                       # the compiled module, waited for
        request.addfinalizer(lambda: bk.debug_set_option("host_module", 0))
    else:
        assert bk.ffi.lib.bk_set_host_compile(0) == 0               # the interpreter re-derives
        request.addfinalizer(lambda: bk.ffi.lib.bk_set_host_compile(1))
    for rows in [None] + (STRIPES if lens == "quincuncial" else []):
        want_off, want_tin, want_sub, want_display, want_scale = host_plane(bk, lens, rows)
        ctx, display, scale = device_build(bk, lens, True, rows)
        off, tin = ctx.read_lensmap()
        np.testing.assert_array_equal(off, want_off)
        np.testing.assert_array_equal(tin, want_tin)
        np.testing.assert_array_equal(ctx.read_subtexel(), want_sub, err_msg=f"rows {rows}")
        assert scale == want_scale and display == want_display
        flagged, changed = ctx.last_build_fixups()
        if (lens, rows) == (TC.FLAGGED_CASE[1], None):
            print(f"{lens}: {flagged} flagged, {changed} changed")
            assert flagged >= 1
            assert ctx.build_breakdown()["compiled_host_module"] == (fixups == "host module")
        # the switch off: the same build is what it was
        off_ctx, display0, scale0 = device_build(bk, lens, False, rows)
        off0, tin0 = off_ctx.read_lensmap()
        np.testing.assert_array_equal(off0, off)
        np.testing.assert_array_equal(tin0, tin)
        assert (display0, scale0, off_ctx.last_build_fixups()) == (display, scale, (flagged, changed))
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*switched off"):
            off_ctx.read_subtexel()
        off_ctx.close()
        ctx.close()


def test_forward_build_is_all_centres(bk):
    ctx = TC.host_ctx(bk, "winkel2", (96, 64), device=True)
    ctx.set_subtexel(True)
    ctx.build()
    assert ctx.last_build_path()[0] == 0 and (ctx.read_lensmap()[0] != NULL).any()
    np.testing.assert_array_equal(ctx.read_subtexel(), SM.CENTRE)
    ctx.set_sequential_build(2)                                     # ... and on the host's forward path
    ctx.build()
    assert ctx.last_build_path()[0] == 2
    np.testing.assert_array_equal(ctx.read_subtexel(), SM.CENTRE)
    ctx.close()


def test_sequential_host_build_fills_the_plane_on_the_device_context(bk):
    want_off, _, want_sub, _, _ = host_plane(bk, "panini")
    ctx = TC.host_ctx(bk, "panini", SIZE, device=True)
    ctx.set_subtexel(True)
    ctx.set_sequential_build(2)
    ctx.build()
    assert ctx.last_build_path()[0] == 2
    np.testing.assert_array_equal(ctx.read_lensmap()[0], want_off)
    np.testing.assert_array_equal(ctx.read_subtexel(), want_sub)
    ctx.close()


# ---- 2. the plane follows the lensmap ---------------------------------------------------------------------------------------------------
def test_the_plane_follows_the_lensmap(bk, tmp_path, monkeypatch):
    monkeypatch.setenv("BLINKY_HIP_CACHE", str(tmp_path))
    W, H = SIZE
    want_off, want_tin, want_sub, _, _ = host_plane(bk, "panini")
    ctx = TC.host_ctx(bk, "panini", SIZE, device=True)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):            # no lensmap
        ctx.read_subtexel()
    ctx.build()                                                     # the switch is off
    for call in (ctx.read_subtexel, lambda: ctx.set_lensmap_subtexel(want_sub)):
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*switched off"):
            call()
    ctx.set_subtexel(True)                                          # on over an old map: absent
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*before bk_set_subtexel"):
        ctx.read_subtexel()
    ctx.set_lensmap_subtexel(want_sub[::-1])                        # ... until it is set
    np.testing.assert_array_equal(ctx.read_subtexel(), want_sub[::-1])
    ctx.build()
    np.testing.assert_array_equal(ctx.read_subtexel(), want_sub)
    ctx.set_lensmap(want_off, want_tin)                             # bk_set_lensmap: centres
    np.testing.assert_array_equal(ctx.read_subtexel(), SM.CENTRE)
    mine = np.arange(W * H, dtype=np.uint32).astype(np.uint16)
    ctx.set_lensmap_subtexel(mine)
    np.testing.assert_array_equal(ctx.read_subtexel(), mine)
    # bk_truncate_build: what it NULLs goes back to the centre, the rest stays
    ctx.build()
    ly, lx = np.divmod(np.arange(W * H), W)
    key = ly * W + (W - 1 - lx) + 1
    bad_key = int(key[(ly == H // 2) & (lx == W // 3)][0])
    ctx.truncate_build(bad_key)
    off = ctx.read_lensmap()[0]
    np.testing.assert_array_equal(off, np.where(key <= bad_key, NULL, want_off))
    np.testing.assert_array_equal(ctx.read_subtexel(), np.where(key <= bad_key, SM.CENTRE, want_sub))
    assert ((key <= bad_key) & (want_off != NULL)).any()
    # kept across a BK_PENDING build
    ctx.build()
    ctx.set_async_compile(True)
    unique = 1.0 + (int(time.time() * 1e6) % 100000) * 1e-9        # a lens nobody has compiled yet: the constant ends up in the kernel
    ctx.load_lens(f"lens_width = 4 lens_height = 3 function lens_inverse(x,y) local k = {unique!r} "
                  "return latlon_to_ray(y * k * 0.5, x * k * 0.5) end", "unique.lua")
    ctx.set_zoom(bk.ffi.ZOOM_CONTAIN)
    assert ctx.build_nowait() is None
    np.testing.assert_array_equal(ctx.read_subtexel(), want_sub)
    ctx.set_async_compile(False)
    # the empty map of a failing script: centres
    ctx.load_lens("lens_width = 4 lens_height = 3 function lens_inverse(x, y) local t = nil return x + t, y, 1 end", "failing.lua")
    ctx.set_zoom(bk.ffi.ZOOM_CONTAIN)
    with pytest.raises(bk.BlinkyError, match=r"\[-3\]"):
        ctx.build()
    assert (ctx.read_lensmap()[0] == NULL).all()
    np.testing.assert_array_equal(ctx.read_subtexel(), SM.CENTRE)
    # gone after bk_set_rows / bk_resize
    ctx.set_rows(10, 20)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        ctx.read_subtexel()
    ctx.set_lensmap(want_off.reshape(H, W)[10:20], want_tin.reshape(H, W)[10:20])
    assert ctx.read_subtexel().shape == (10 * W,)
    ctx.resize(W + 8, H)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        ctx.read_subtexel()
    ctx.close()
