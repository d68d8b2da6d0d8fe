"""What hangs off the lensmap - the sub-texel plane, the spans, the block map, the footprint - across the two changes that keep the
map buffers in place because the pixel count stays: bk_resize(96 x 64 -> 64 x 96, platesize 64 both) and bk_set_rows([0, 32) ->
[32, 64)).  One context with the sub-texel switch on; a drawn table is set and every consumer touched once, so that each has made what it
keeps; then the change, after which every one answers BK_E_STATE; then a different table, after which every frame equals its numpy model
over the whole allocation - nothing of the first table, its plane, its spans, its block map or its footprint is left.  Tables, plates,
sources, destinations and models are those of the frame-buffer tests (by import).  Every comparison is exact equality."""
import numpy as np
import pytest

import footprint_model as FM
import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB
import test_apply_rgba_fb_seams_gpu as SE

pytestmark = pytest.mark.gpu

NULL = BL.NULL
NO_LENSMAP = r"\[-6\].*no lensmap"


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def case(W, H, seed):
    table = FB.drawn_table(W, H, seed)
    ps = table[4]
    pal = np.random.default_rng(8300 + seed).integers(0, 256, (6, 256)).astype(np.uint8)
    return dict(table=table, sub=BL.random_subs(W * H, 300 + seed), seams=SE.drawn_seams(ps, 20 + seed), plates=FB.texels(ps, 90 + seed),
                lut=FB.luts(95 + seed), pal=pal)


def install(ctx, c, rows):
    """the case's table, plane and seam table into the context, its plates into truecolour globe 0 (ring slot 2 = byte 2 of every texel)"""
    BL.set_table(ctx, c["table"], c["sub"], rows)
    ctx.set_seam_table(c["seams"])
    FB.upload_globe(ctx, c["plates"])
    c["src"] = FB.source(c["plates"], "pitch16")


def expect8(c, rows):
    """the 8-bit rubix frame of ring slot 2 through the case's palette: the owned rows' mapped pixels, everything else as it was"""
    off, tints, W, H, ps = c["table"]
    m = off != NULL
    v = np.ascontiguousarray(c["plates"][..., 2]).reshape(-1)[np.where(m, off, 0)]
    t = tints.astype(np.int64)
    px = np.where(m, np.where(t < 6, c["pal"][np.where(t < 6, t, 0), v], v), FB.FILL).astype(np.uint8).reshape(H, W)
    want = np.full((H, W), FB.FILL, np.uint8)
    want[rows[0]:rows[1]] = px[rows[0]:rows[1]]
    return want


# ---- the consumers: each makes its call and, if the call comes back, holds the result to the model of case c, owned rows `rows` ----------
def apply8_device(ctx, c, rows):
    import torch
    off, tints, W, H, ps = c["table"]
    dst = torch.full((H, W), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx.apply_device(dst.data_ptr(), W, H * W, frame0=2, rubix_on=True, pal=c["pal"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy(), expect8(c, rows), err_msg="bk_apply_device")


def apply8_host(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    got = ctx.apply(np.full((H, W), FB.FILL, np.uint8), frame=2, rubix_on=True, pal=c["pal"])
    np.testing.assert_array_equal(got, expect8(c, rows), err_msg="bk_apply (spans)")


def staged_rgba(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    d = FB.dest(W, H, False)
    np.testing.assert_array_equal(FB.run_existing(ctx, d, None, False), FB.model(c["plates"], c["table"], d, None, False, rows),
                                  err_msg="bk_apply_rgba_device")


def footprint(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    masks, counts, rects = FM.footprint(off, W, H, ps, rows)
    for p in range(6):
        rect, n, mask = ctx.plate_footprint(p, tiles=True)
        assert (rect, n) == (rects[p], counts[p]), f"bk_plate_footprint plate {p}"
        np.testing.assert_array_equal(mask, masks[p], err_msg=f"bk_plate_footprint plate {p}")


def fb_nearest(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    d, (_, ptrs, pitches) = FB.dest(W, H, False), c["src"]
    for lut in (None, c["lut"]):
        np.testing.assert_array_equal(FB.run_fb(ctx, ptrs, pitches, d, lut, False), FB.model(c["plates"], c["table"], d, lut, False, rows),
                                      err_msg=f"bk_apply_rgba_fb_device lut {lut is not None}")


def fb_bilinear(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    d, (_, ptrs, pitches) = FB.dest(W, H, False), c["src"]
    np.testing.assert_array_equal(BL.run(ctx, ptrs, pitches, d, c["lut"]), BL.model(c["plates"], c["table"], c["sub"], d, c["lut"], rows),
                                  err_msg="bk_apply_rgba_fb_bilinear_device")


def fb_seams(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    d, (_, ptrs, pitches) = FB.dest(W, H, False), c["src"]
    np.testing.assert_array_equal(SE.run(ctx, ptrs, pitches, d, c["lut"]),
                                  SE.model(c["plates"], c["table"], c["sub"], c["seams"], d, c["lut"], rows),
                                  err_msg="bk_apply_rgba_fb_bilinear_seams_device")


def read_back(ctx, c, rows):
    off, tints, W, H, ps = c["table"]
    got_off, got_tints = ctx.read_lensmap()
    got_sub = ctx.read_subtexel()
    cut = slice(rows[0] * W, rows[1] * W)
    np.testing.assert_array_equal(got_off, off[cut], err_msg="bk_read_lensmap")
    np.testing.assert_array_equal(got_tints, tints[cut], err_msg="bk_read_lensmap: tints")
    np.testing.assert_array_equal(got_sub, c["sub"][cut], err_msg="bk_read_subtexel")


CONSUMERS = [apply8_device, staged_rgba, footprint, fb_nearest, fb_bilinear, fb_seams, apply8_host]


def through(bk, first, rows_first, change, second, rows_second):
    off, tints, W, H, ps = first["table"]
    ctx = bk.Context()
    ctx.set_frames(4)
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    install(ctx, first, rows_first)
    for use in CONSUMERS + [read_back]:
        use(ctx, first, rows_first)
    change(ctx)
    assert ctx.size()[2] == ps and (ctx.size()[4] - ctx.size()[3]) * ctx.size()[0] == (rows_first[1] - rows_first[0]) * W      # the same pixel count
    for use in CONSUMERS:
        with pytest.raises(bk.BlinkyError, match=NO_LENSMAP):
            use(ctx, first, rows_first)
    with pytest.raises(bk.BlinkyError, match=NO_LENSMAP):
        ctx.read_subtexel()
    with pytest.raises(bk.BlinkyError, match=NO_LENSMAP):
        ctx.read_lensmap()
    install(ctx, second, rows_second)
    for use in CONSUMERS + [read_back] + CONSUMERS[::-1]:
        use(ctx, second, rows_second)
    ctx.close()


def test_resize_to_the_same_pixel_count_and_platesize(bk):
    first, second = case(96, 64, 0), case(64, 96, 1)
    assert first["table"][4] == second["table"][4] == 64
    assert (first["table"][0] != second["table"][0]).any() and (first["sub"] != second["sub"]).any()
    through(bk, first, (0, 64), lambda ctx: ctx.resize(64, 96), second, (0, 96))


def test_set_rows_that_moves_a_stripe_of_the_same_height(bk):
    first, second = case(96, 64, 0), case(96, 64, 1)
    assert (first["table"][0][:32 * 96] != second["table"][0][32 * 96:]).any()
    through(bk, first, (0, 32), lambda ctx: ctx.set_rows(32, 64), second, (32, 64))
