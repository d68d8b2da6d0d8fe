"""The mip pyramid at DEPTH: tests/test_mip_pyramid_gpu.py's comparison - bk_read_mip_level of every level of every plate against
tests/trilinear_model.py's pyramid, exact - at the smallest platesizes that reach what platesizes up to 203 cannot: a last tile of
mip_head_kernel one texel column wide, more than two tiles across, mip_tail_kernel's strided loop taking a second trip (and every thread
taking one), and a layout of more than nine levels.  Every level is read AFTER the one build, so levels (or plates) that overlap in the
layout show; a mismatch names its first differing plate, level and texel."""
import functools

import numpy as np
import pytest

import test_apply_rgba_fb_gpu as FB
import test_mip_pyramid_gpu as MP
import trilinear_model as TM

pytestmark = pytest.mark.gpu

# platesize -> source class (FB.LAYOUTS; all six occur).  Where the base and the pitch are multiples of 16 the head kernel loads 16 bytes
# a row ("pitch16", "tight" at 260 and 640, "atlas" at 1024, plates 1 and 4 of "six-pitches"), elsewhere eight clamped dwords.
# The head kernel's LDS clamps show at few sizes only: an LDS entry past a level's size is made of coordinates clamped on the level
# below, and where that level's size is ODD it EQUALS the level's last entry, so reading it instead changes nothing (129, 257, 203).
# The level-2 stage's clamp matters where s_1 is odd and ps even (ps = 2 mod 4), the level-3 stage's where s_2 is odd and s_1 even.
DEEP = {
    129: "six-pitches",     # s_1 = 65: TWO tiles across, the last ONE texel column wide (its level-1 origin is s_1 - 1: xa = xb = 0 in LDS)
    130: "ptr4",            # the same tiles with ps = 2 mod 4: level 1's entry 65 of the last tile is NOT its entry 64 - the level-2 clamp decides
    257: "pitch+20",        # s_1 = 129: a one-column last tile with THREE tiles across
    258: "pitch16",         # ... and ps = 2 mod 4
    260: "tight",           # s_1 = 130, s_2 = 65: the level-3 stage's clamp decides (the last tile's level-2 origin is s_2 - 1)
    513: "pitch16",         # s_4 = 33, 1089 texels: the first size at which a thread of the tail comes round again
    640: "tight",           # an even chain down to 5 (640, 320, 160, 80, 40, 20, 10, 5, 3, 2, 1): no clamp in the head, five tiles across
    721: "ptr4",            # s_4 = 46, 2116 texels: EVERY thread of the tail takes a second trip (and 68 a third)
    1024: "atlas",          # a power of two: eleven levels, no clamp anywhere, whole tiles only
    1025: "six-pitches",    # twelve levels (past the table's entry 9), s_4 = 65 (five trips), s_5 = 33 (a second trip at level 5 too)
}


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def structured_texels(ps, seed):
    """uint8 [6][ps][ps][4]: half FB.texels' noise, half a random 4 x 4 field of blocks per plate and byte.  Uniform noise alone averages to
    127 or 128 from level 4 or so on: deep levels that all hold the same value cannot tell one texel, level or plate from another"""
    coarse = np.random.default_rng(950 + seed).integers(0, 256, (6, 4, 4, 4)).astype(np.uint16)
    side = (ps + 3) // 4
    field = coarse.repeat(side, axis=1).repeat(side, axis=2)[:, :ps, :ps]
    return ((FB.texels(ps, seed) + field) >> 1).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def plates_and_pyramid(ps, seed):
    plates = structured_texels(ps, seed)
    plates[:, ::3, ::2] = 255                                           # (sums that round at the top of the range)
    pyr = TM.pyramid(plates)
    assert all(len(np.unique(level[..., 0])) >= 4 for level in pyr)     # (no level is flat, the six texels of the last one included)
    for level in [plates] + pyr:
        level.flags.writeable = False
    return plates, pyr


def check_levels(ctx, want, what, only=range(6)):
    """every level from 1 on of the plates in `only` against `want` (a pyramid, or None for "zeros, as allocated")"""
    sizes = ctx.mip_info()
    for p in only:
        for k in range(1, len(sizes)):
            got = ctx.read_mip_level(p, k)
            exp = np.zeros((sizes[k], sizes[k], 4), np.uint8) if want is None else want[k][p]
            assert got.shape == exp.shape, f"{what}: plate {p} level {k}: shape {got.shape}, expected {exp.shape}"
            if not np.array_equal(got, exp):
                y, x, c = np.argwhere(got != exp)[0]
                raise AssertionError(f"{what}: plate {p} level {k}: {int((got != exp).any(axis=2).sum())} of {exp.shape[0] * exp.shape[1]} texels differ, the first "
                                     f"at (x {x}, y {y}) byte {c}: {got[y, x, c]}, expected {exp[y, x, c]}")


@pytest.mark.parametrize("ps", sorted(DEEP))
def test_every_level_of_every_plate_after_one_build(bk, ps):
    ctx, W = MP.make_ctx(bk, ps)
    assert ctx.mip_info() == TM.level_sizes(ps)
    plates, pyr = plates_and_pyramid(ps, 60 + ps % 7)
    dev, ptrs, pitches = FB.source(plates, DEEP[ps])
    MP.make(ctx, ptrs, pitches, W, ps)
    check_levels(ctx, pyr, f"ps {ps} {DEEP[ps]}")
    ctx.close()


def test_a_null_plate_keeps_its_deep_levels(bk):
    """ps 721: the tail's skip bit where its loop loops - the NULL plates keep every level of the first build, levels 4 .. L - 1 among them"""
    ps = 721
    ctx, W = MP.make_ctx(bk, ps)
    first, pyr_first = plates_and_pyramid(ps, 62)
    second, pyr_second = plates_and_pyramid(ps, 63)
    dev, ptrs, pitches = FB.source(first, "pitch16")
    MP.make(ctx, ptrs, pitches, W, ps)
    check_levels(ctx, pyr_first, "first")
    dev2, ptrs2, pitches2 = FB.source(second, "pitch16", skip=(2, 5))   # (plate 0 is named by the lensmap: it must be given)
    MP.make(ctx, ptrs2, pitches2, W, ps)
    check_levels(ctx, pyr_second, "second", only=(0, 1, 3, 4))
    check_levels(ctx, pyr_first, "kept", only=(2, 5))
    ctx.close()


def test_the_pyramid_by_itself_is_the_calls_pyramid_at_depth(bk):
    """ps 721, bk_debug_mip_pyramid with plate 4 NULL: the call's levels for the five, and plate 4's as allocated - zeros, every level"""
    import torch
    ps = 721
    ctx, W = MP.make_ctx(bk, ps)
    plates, pyr = plates_and_pyramid(ps, 62)
    dev, ptrs, pitches = FB.source(plates, "pitch+20", skip=(4,))
    ctx.debug_mip_pyramid(ptrs, pitches)
    torch.cuda.synchronize()
    check_levels(ctx, pyr, "by itself", only=(0, 1, 2, 3, 5))
    check_levels(ctx, None, "never made", only=(4,))
    ctx.close()
