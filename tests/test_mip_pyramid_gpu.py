"""The mip pyramid of bk_apply_rgba_fb_trilinear_device on the GPU: bk_read_mip_level of every level against tests/trilinear_model.py's
pyramid (held to a texel loop by tests/test_trilinear_cpu.py), over platesizes on both sides of the first kernel's 128 x 16 tile and
of the three levels it makes, every source class of the frame-buffer calls, NULL plates and the pyramid's life.  Exact equality."""
import numpy as np
import pytest

import test_apply_rgba_fb_gpu as FB
import trilinear_model as TM

pytestmark = pytest.mark.gpu

PLATESIZES = [1, 2, 3, 5, 16, 17, 33, 64, 65, 203]
LAYOUT_OF = dict(zip(PLATESIZES, ["tight", "pitch16", "pitch+20", "ptr4", "atlas", "six-pitches", "pitch+20", "atlas", "ptr4", "pitch16"]))


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def make_ctx(bk, ps, W=None):
    """a context of platesize ps whose lensmap names texel 0 of plate 0 only: the pyramid does not depend on it"""
    W = W or ps + 3
    ctx = bk.Context()
    ctx.resize(W, ps)
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    off = np.full(W * ps, TM.NULL, np.uint32)
    off[0] = 0
    ctx.set_lensmap(off.reshape(ps, W), np.full((ps, W), 255, np.uint8))
    return ctx, W


def make(ctx, ptrs, pitches, W, ps, mips=True):
    import torch
    dst = torch.zeros(ps * W * 4, dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr(), 4 * W, mips=mips)
    torch.cuda.synchronize()


def check(ctx, plates, what, only=range(6)):
    want = TM.pyramid(plates)
    for p in only:
        for k in range(1, len(want)):
            np.testing.assert_array_equal(ctx.read_mip_level(p, k), want[k][p], err_msg=f"{what}: plate {p} level {k}")


@pytest.mark.parametrize("ps", PLATESIZES)
def test_every_level_is_the_model(bk, ps):
    ctx, W = make_ctx(bk, ps)
    assert ctx.mip_info() == TM.level_sizes(ps)
    plates = FB.texels(ps, 60 + ps % 7)
    plates[:, ::3, ::2] = 255                                           # (sums that round at the top of the range)
    dev, ptrs, pitches = FB.source(plates, LAYOUT_OF[ps])
    make(ctx, ptrs, pitches, W, ps)
    check(ctx, plates, f"ps {ps} {LAYOUT_OF[ps]}")
    ctx.close()


@pytest.mark.parametrize("layout", FB.LAYOUTS)
def test_source_classes_and_the_bytes_between_rows(bk, layout):
    """ps 203 (two tiles across, thirteen down, every size from level 2 on odd or clamped): each layout, and two different guard values in
    the bytes between 4 * ps and the pitch give the same pyramid"""
    ps = 203
    ctx, W = make_ctx(bk, ps)
    plates = FB.texels(ps, 61)
    for guard in (0x3C, 0xC3):
        FB.SRC_GUARD, keep = guard, FB.SRC_GUARD
        try:
            dev, ptrs, pitches = FB.source(plates, layout)
        finally:
            FB.SRC_GUARD = keep
        make(ctx, ptrs, pitches, W, ps)
        check(ctx, plates, f"{layout} guard {guard:#x}")
    ctx.close()


def test_a_null_plate_keeps_its_levels(bk):
    ps = 33
    ctx, W = make_ctx(bk, ps)
    first, second = FB.texels(ps, 62), FB.texels(ps, 63)
    dev, ptrs, pitches = FB.source(first, "pitch16")
    make(ctx, ptrs, pitches, W, ps)
    check(ctx, first, "first")
    dev2, ptrs2, pitches2 = FB.source(second, "pitch16", skip=(2, 5))   # (plate 0 is named by the lensmap: it must be given)
    make(ctx, ptrs2, pitches2, W, ps)
    check(ctx, second, "second", only=(0, 1, 3, 4))
    check(ctx, first, "kept", only=(2, 5))
    ctx.close()


def test_the_pyramid_by_itself_is_the_calls_pyramid(bk):
    """bk_debug_mip_pyramid (what tools/bench_rgba.py times as M): the same levels with no apply, usable by mips = 0 afterwards"""
    import torch
    ps = 65
    ctx, W = make_ctx(bk, ps)
    plates = FB.texels(ps, 66)
    dev, ptrs, pitches = FB.source(plates, "pitch+20", skip=(4,))
    ctx.debug_mip_pyramid(ptrs, pitches)
    torch.cuda.synchronize()
    check(ctx, plates, "by itself", only=(0, 1, 2, 3, 5))
    np.testing.assert_array_equal(ctx.read_mip_level(4, 1), 0)         # (never made: as allocated)
    make(ctx, ptrs, pitches, W, ps, mips=False)
    with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
        ctx.debug_mip_pyramid([ptrs[0] + 2] + ptrs[1:], pitches)
    ctx.close()


def test_the_pyramid_lives_with_the_platesize(bk):
    ps = 16
    ctx, W = make_ctx(bk, ps)
    plates = FB.texels(ps, 64)
    dev, ptrs, pitches = FB.source(plates)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*mips = 0"):
        make(ctx, ptrs, pitches, W, ps, mips=False)                    # none made yet
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no pyramid"):
        ctx.read_mip_level(0, 1)
    make(ctx, ptrs, pitches, W, ps)
    make(ctx, ptrs, pitches, W, ps, mips=False)
    for bad in ((6, 1), (-1, 1), (0, 0), (0, 5)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.read_mip_level(*bad)
    # a resize that keeps the platesize keeps the pyramid; one that changes it drops it
    for size, kept in (((W + 5, ps), True), ((40, 17), False)):
        ctx.resize(*size)
        w, h = size
        off = np.full(w * h, TM.NULL, np.uint32)
        off[0] = 0
        ctx.set_lensmap(off.reshape(h, w), np.full((h, w), 255, np.uint8))
        big = FB.texels(min(size), 65)
        devb, ptrsb, pitchesb = FB.source(big)
        if kept:
            make(ctx, ptrsb, pitchesb, w, h, mips=False)
            check(ctx, plates, "kept across a resize of the same platesize")
        else:
            with pytest.raises(bk.BlinkyError, match=r"\[-6\].*mips = 0"):
                make(ctx, ptrsb, pitchesb, w, h, mips=False)
            make(ctx, ptrsb, pitchesb, w, h)
            check(ctx, big, "after the resize")
    ctx.close()
    none = bk.Context(bk.ffi.DEVICE_NONE)
    none.resize(300, 203)
    assert none.mip_info() == TM.level_sizes(203)
    none.close()
