"""bk_apply_rgba_fb_trilinear_device at DEPTH: tests/test_apply_rgba_fb_trilinear_gpu.py's comparison - its check(), exact, over the whole
destination allocation - at platesizes whose pyramids have 10 to 12 levels, where the apply addresses the table's entries 9 to 11
(U >> k for k up to 11, the LDS copy of those entries, top = 10 and 11), and at padded plate widths other than 64, 192 and 256 (gp =
320, 576, 768, 1024, 1088).  Deep cases are STRIPES: the frame, the platesize, gp and the pyramid are full size, the context owns about
17 rows (the first no multiple of 8), so the kernels and the model do stripe-sized work.  tests/test_trilinear_cpu.py holds
deep_cases() to the census of what the owned rows have to reach.  Plates and their pyramid are made once per platesize."""
import functools

import numpy as np
import pytest

import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB
import test_apply_rgba_fb_trilinear_gpu as T
import test_mip_pyramid_deep_gpu as MD
import trilinear_model as TM

pytestmark = pytest.mark.gpu

# (W, H) -> the owned rows.  ps = H: 257 (10 levels), 513, 721 (11), 1025 (12) - the platesizes of tests/test_mip_pyramid_deep_gpu.py - and
# 1024 (11 levels), the size at which a plate's last texel is the last texel of EVERY level: at 2^n + 1 the last texel of a level
# k >= 1 holds one level-0 column, positions never pass its centre and its right / bottom clamp cannot occur (test_trilinear_cpu.py).
# W % 4 = 0, 3, 0, 3, 2.  DRAWN_SEED: the drawn table's seed - for each size one whose table has NULLs sprinkled through every row (a NULL
# inside a lane's four pixels in any stripe); the tables are of the kinds columns, random, random, random, columns.
STRIPES = {(260, 257): (123, 140), (515, 513): (243, 260), (724, 721): (355, 372), (1027, 1025): (501, 518), (1026, 1024): (509, 526)}
DRAWN_SEED = {(260, 257): 1, (515, 513): 3, (724, 721): 6, (1027, 1025): 3, (1026, 1024): 2}
KINDS = ("drawn", "corners")
STITCH = ((243, 262), (262, 263), (263, 290))                           # of 515 x 513: an odd cut, one row; 47 rows


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def deep_case(size, kind):
    """(table, sub, lod, rows); the plane is drawn for the whole frame, the owned rows' part is what the context is given"""
    W, H = size
    table, sub = BL.drawn_case(W, H, DRAWN_SEED[size]) if kind == "drawn" else BL.corner_case(W, H)
    return table, sub, TM.random_lods(W * H, table[4], W + H + KINDS.index(kind)), STRIPES[size]


def deep_cases():
    """[(name, kind, table, sub, lod, rows)] of every case below: what the census of tests/test_trilinear_cpu.py runs over"""
    return [(f"{kind} {size[0]}x{size[1]}", kind) + deep_case(size, kind) for size in STRIPES for kind in KINDS]


@functools.lru_cache(maxsize=1)
def plates_and_pyramid(ps):
    plates = MD.structured_texels(ps, 110 + ps % 5)                    # (deep levels that differ from texel to texel)
    pyr = TM.pyramid(plates)
    for level in [plates] + pyr:
        level.flags.writeable = False
    return plates, pyr


# ---- 1. drawn tables and rims on stripes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", list(STRIPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_deep_stripes(bk, size, kind):
    table, sub, lod, rows = deep_case(size, kind)
    ps = table[4]
    plates, pyr = plates_and_pyramid(ps)
    ctx = T.make_ctx(bk, table, sub, lod, rows=rows)
    assert len(ctx.mip_info()) == len(pyr) >= 10
    layout = FB.LAYOUTS[(ps + KINDS.index(kind)) % len(FB.LAYOUTS)]
    T.check(ctx, table, sub, lod, plates, FB.luts(111), f"{kind} {size} rows {rows} {layout}", layout, rows=rows, pyr=pyr)
    ctx.close()


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------------
def test_a_plane_of_zeros_is_the_bilinear_call_at_gp_576(bk):
    """515 x 513 on a stripe: the trilinear call with a plane of zeros = the bilinear call = the bilinear model; and on the same context
    one nearest frame against its model - the bilinear and the nearest kernel at gp = 576 too"""
    size = (515, 513)
    W, H = size
    rows = STRIPES[size]
    table, sub = BL.drawn_case(W, H, DRAWN_SEED[size])
    plates, _ = plates_and_pyramid(table[4])
    lut = FB.luts(112)
    dev, ptrs, pitches = FB.source(plates, "pitch+20")
    d = FB.dest(W, H, False)
    ctx = T.make_ctx(bk, table, sub, np.zeros(W * H, np.uint16), rows=rows)
    for tinted in (False, True):
        got = T.run(ctx, ptrs, pitches, d, lut if tinted else None)
        T.same(got, BL.run(ctx, ptrs, pitches, d, lut if tinted else None), d, f"tinted {tinted}: the bilinear call")
        T.same(got, BL.model(plates, table, sub, d, lut if tinted else None, rows), d, f"tinted {tinted}: the bilinear model")
    T.same(FB.run_fb(ctx, ptrs, pitches, d, lut, False), FB.model(plates, table, d, lut, False, rows), d, "the nearest call")
    ctx.close()


# ---- 3. stripes ---------------------------------------------------------------------------------------------------------------------------
def test_deep_stripe_contexts_stitch_one_frame(bk):
    """515 x 513: three adjacent stripe contexts into one destination = the model of their union"""
    import torch
    size = (515, 513)
    W, H = size
    table, sub, lod, _ = deep_case(size, "drawn")
    plates, pyr = plates_and_pyramid(table[4])
    lut = FB.luts(113)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    assert all(a[1] == b[0] for a, b in zip(STITCH, STITCH[1:])) and STITCH[-1][1] - STITCH[0][0] <= 48
    for tinted in (False, True):
        dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
        for rows in STITCH:
            ctx = T.make_ctx(bk, table, sub, lod, rows=rows)
            ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr(), d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut if tinted else None)
            torch.cuda.synchronize()
            ctx.close()
        T.same(dst.cpu().numpy(), T.model(pyr, table, sub, lod, d, lut if tinted else None, (STITCH[0][0], STITCH[-1][1])), d, f"tinted {tinted}: stitched")
