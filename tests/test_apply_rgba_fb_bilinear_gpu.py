"""bk_apply_rgba_fb_bilinear_device on the GPU: the frame-buffer apply with bilinear texel filtering through the sub-texel plane.  Every
case has two expectations over the WHOLE destination allocation (fill 77, a pitch wider than the frame, an origin, rows below):
(a) the numpy model of tests/subtexel_model.py (held to a second formulation by tests/test_subtexel_cpu.py) and (b) the identity "a
plane that is 0x8080 everywhere gives bk_apply_rgba_fb_device's frame byte for byte".  Every frame is made TWICE, from plates whose
texels farther than one from a named texel hold one guard value and then another: it may not depend on them.  Tables come from the
generator of the existing frame-buffer tests (by import) through bk_set_lensmap + bk_set_lensmap_subtexel unless a test says otherwise;
tests/test_subtexel_cpu.py holds the cases below to the census they have to reach.  Every comparison is exact equality."""
import numpy as np
import pytest

import subtexel_model as SM
import test_apply_rgba_fb_gpu as FB

pytestmark = pytest.mark.gpu

NULL = SM.NULL
GUARDS = (0x3C, 0xC3)
# W x H; ps = min(W, H): 1, 3, 8, 15, 64, 203 (gp = 64, 64, 64, 64, 64, 256: never ps but at 64); W % 4 != 0 at 1, 3, 130, 131, 261
SIZES = [(1, 1), (3, 9), (130, 8), (131, 15), (256, 64), (261, 203)]
EDGE_VALUES = np.array([0, 127, 128, 255])


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def random_subs(n, seed):
    """uint16 [n]: each axis one of 0, 127, 128, 255 four times in ten, any value otherwise"""
    rng = np.random.default_rng(7100 + seed)
    axis = lambda: np.where(rng.random(n) < 0.4, EDGE_VALUES[rng.integers(0, 4, n)], rng.integers(0, 256, n))
    return (axis() | (axis() << 8)).astype(np.uint16)


def drawn_case(W, H, seed=0):
    """(table, sub): a table of the existing tests' generator with a random plane"""
    table = FB.drawn_table(W, H, seed)
    return table, random_subs(W * H, 10 * seed + W + H)


def walk_case():
    """256 x 64, ps 64: qx walks 0..255 along a row, qy all 256 values over the frame"""
    table = FB.drawn_table(256, 64, 1)
    ly, lx = np.divmod(np.arange(256 * 64), 256)
    return table, ((lx % 256) | (((4 * ly + lx // 64) % 256) << 8)).astype(np.uint16)


def corner_case(W=131, H=15):
    """every pixel on the rim of its plate - a corner, or an edge at a random place along it - with the plane's axes drawn from 0, 127, 128,
    255 half the time: each of the four clamps, at px = 0 and px = ps - 1; every fifth pixel of the odd columns NULL (a NULL inside a
    lane's four beside mapped ones); tints 0..5, 6, 200, 255"""
    ps = min(W, H)
    rng = np.random.default_rng(7200 + W + H)
    n = W * H
    rim = lambda: np.where(rng.random(n) < 0.5, 0, ps - 1)
    kind = rng.integers(0, 3, n)                                       # 0: a corner, 1: x on the rim, 2: y on the rim
    px = np.where(kind == 2, rng.integers(0, ps, n), rim())
    py = np.where(kind == 1, rng.integers(0, ps, n), rim())
    off = (rng.integers(0, 6, n) * ps * ps + py * ps + px).astype(np.uint32)
    lx = np.arange(n) % W
    off[(lx % 2 == 1) & (np.arange(n) % 5 == 0)] = NULL
    tints = np.array([0, 1, 2, 3, 4, 5, 6, 200, 255], np.uint8)[rng.integers(0, 9, n)]
    axis = lambda: np.where(rng.random(n) < 0.5, EDGE_VALUES[rng.integers(0, 4, n)], rng.integers(0, 256, n))
    return (off, tints, W, H, ps), (axis() | (axis() << 8)).astype(np.uint16)


def committed_cases():
    """every (table, sub) the tests below apply through drawn tables: what the census of tests/test_subtexel_cpu.py runs over"""
    return [drawn_case(W, H, seed) for W, H in SIZES for seed in (0, 1)] + [walk_case(), corner_case()]


# ---- running it -----------------------------------------------------------------------------------------------------------------------
def make_ctx(bk, table, sub, rows=None, slots=1):
    off, tints, W, H, ps = table
    ctx = bk.Context()
    ctx.set_frames(slots)
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    set_table(ctx, table, sub, rows)
    return ctx


def set_table(ctx, table, sub, rows=None):
    off, tints, W, H, ps = table
    FB.set_table(ctx, table, rows)
    r0, r1 = rows or (0, H)
    if sub is not None:
        ctx.set_lensmap_subtexel(np.asarray(sub).reshape(H, W)[r0:r1])


def guarded(plates, table, sub, guard, rows=None):
    """the plates with `guard` in every byte of every texel farther than one from a texel the owned rows name"""
    off, tints, W, H, ps = table
    r0, r1 = rows or (0, H)
    mask = SM.read_mask(np.asarray(off).reshape(H, W)[r0:r1], None, ps)
    g = plates.copy()
    g[~mask] = guard
    return g, mask


def run(ctx, ptrs, pitches, d, lut, ptr_off=0):
    import torch
    dst = torch.full((ptr_off + d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_fb_bilinear_device(ptrs, pitches, dst.data_ptr() + ptr_off, d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def model(plates, table, sub, d, lut, rows=None, ptr_off=0):
    off, tints, W, H, ps = table
    want = np.full(ptr_off + d["rows"] * d["pitch"], FB.FILL, np.uint8)
    SM.bilinear_frame(plates, off, sub, tints, W, H, ps, rows or (0, H), lut, want[ptr_off:].reshape(d["rows"], d["pitch"]), d["x0"], d["y0"])
    return want


def check(ctx, table, sub, plates, lut, what, layout="tight", rows=None, d=None, null_unread=False):
    """plain and tinted, each from both guarded copies of the plates, against the model of the TRUE plates"""
    off, tints, W, H, ps = table
    d = d or FB.dest(W, H, False)
    for guard in GUARDS:
        g, mask = guarded(plates, table, sub, guard, rows)
        skip = [p for p in range(6) if not mask[p].any()] if null_unread else ()
        dev, ptrs, pitches = FB.source(g, layout, skip=skip)
        for tinted in (False, True):
            got = run(ctx, ptrs, pitches, d, lut if tinted else None)
            np.testing.assert_array_equal(got, model(plates, table, sub, d, lut if tinted else None, rows),
                                          err_msg=f"{what} {'tinted' if tinted else 'plain'} guard {guard:#x}: the model")


# ---- 1. drawn tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_drawn_tables(bk, W, H):
    for seed in (0, 1):
        table, sub = drawn_case(W, H, seed)
        plates, lut = FB.texels(table[4], 30 + seed), FB.luts(40 + seed)
        ctx = make_ctx(bk, table, sub)
        check(ctx, table, sub, plates, lut, f"drawn {W}x{H} seed {seed}", FB.LAYOUTS[(W + seed) % len(FB.LAYOUTS)])
        ctx.close()


def test_subs_that_walk_every_value_of_both_axes(bk):
    table, sub = walk_case()
    assert set(sub & 255) == set(range(256)) and set(sub >> 8) == set(range(256))
    plates, lut = FB.texels(table[4], 32), FB.luts(42)
    ctx = make_ctx(bk, table, sub)
    check(ctx, table, sub, plates, lut, "walk", "pitch16")
    ctx.close()


def test_plate_corners_and_edges_clamp_to_the_plate(bk):
    table, sub = corner_case()
    plates, lut = FB.texels(table[4], 33), FB.luts(43)
    ctx = make_ctx(bk, table, sub)
    check(ctx, table, sub, plates, lut, "corners", "six-pitches")
    ctx.close()


def test_a_constant_plate_gives_that_constant(bk):
    table, sub = drawn_case(131, 15)
    off, tints, W, H, ps = table
    plates = np.empty((6, ps, ps, 4), np.uint8)
    plates[...] = np.array([[7, 99, 200, 255], [0, 1, 254, 128], [255, 255, 255, 255], [0, 0, 0, 0], [13, 14, 15, 16], [250, 3, 77, 1]],
                           np.uint8)[:, None, None, :]
    ctx = make_ctx(bk, table, sub)
    dev, ptrs, pitches = FB.source(plates)
    d = FB.dest(W, H, False)
    got = run(ctx, ptrs, pitches, d, None)
    np.testing.assert_array_equal(got, FB.model(plates, table, d, None, False))      # the NEAREST model: the blend changes nothing
    ctx.close()


# ---- 2. all centres = the nearest apply ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_a_plane_of_centres_is_the_nearest_apply_byte_for_byte(bk, W, H):
    table = FB.drawn_table(W, H, 1)
    plates, lut = FB.texels(table[4], 34), FB.luts(44)
    ctx = make_ctx(bk, table, None)                                    # bk_set_lensmap alone: the plane is all 0x8080
    np.testing.assert_array_equal(ctx.read_subtexel(), SM.CENTRE)
    dev, ptrs, pitches = FB.source(plates, "pitch+20")
    d = FB.dest(W, H, False)
    for tinted in (False, True):
        got = run(ctx, ptrs, pitches, d, lut if tinted else None)
        np.testing.assert_array_equal(got, FB.run_fb(ctx, ptrs, pitches, d, lut if tinted else None, False), err_msg=f"tinted {tinted}: the nearest call")
        np.testing.assert_array_equal(got, FB.model(plates, table, d, lut if tinted else None, False), err_msg=f"tinted {tinted}: the nearest model")
    ctx.close()


# ---- 3. sources and destinations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", FB.LAYOUTS)
def test_source_classes(bk, layout):
    table, sub = drawn_case(261, 203)                                  # ps 203: gp 256
    plates, lut = FB.texels(table[4], 35), FB.luts(45)
    ctx = make_ctx(bk, table, sub)
    check(ctx, table, sub, plates, lut, layout, layout, null_unread=layout == "atlas")
    ctx.close()


def test_unread_plates_may_be_null(bk):
    off, tints, W, H, ps = FB.drawn_table(131, 15)
    off = np.where(off // (ps * ps) >= 3, NULL, off).astype(np.uint32)      # (NULL // ps^2 is far above 3)
    table, sub = (off, tints, W, H, ps), random_subs(W * H, 3)
    plates, lut = FB.texels(ps, 36), FB.luts(46)
    ctx = make_ctx(bk, table, sub)
    _, mask = guarded(plates, table, sub, 0)
    unread = [p for p in range(6) if not mask[p].any()]
    assert {3, 4, 5} <= set(unread) and len(unread) < 6
    check(ctx, table, sub, plates, lut, "NULL plates", "ptr4", null_unread=True)
    ctx.close()


@pytest.mark.parametrize("cls", FB.G.ALIGN_CLASSES)
@pytest.mark.parametrize("W,H", [(256, 64), (131, 15)])
def test_destination_classes(bk, W, H, cls):
    table, sub = drawn_case(W, H)
    plates, lut = FB.texels(table[4], 37), FB.luts(47)
    ctx = make_ctx(bk, table, sub)
    x0 = {"16": 4, "8-only": 2, "4-only": 1}[cls]
    px_pitch = (W + x0 + 3) // 4 * 4 + {"16": 4, "8-only": 2, "4-only": 1}[cls]
    d = FB.dest(W, H, False, x0=x0, y0=2, extra_px=px_pitch - W)
    assert FB.G.align_class(d["y0"] * d["pitch"] + 4 * x0, d["pitch"], 0) == cls
    check(ctx, table, sub, plates, lut, f"{W}x{H} {cls}", "pitch16", d=d)
    ctx.close()


# ---- 4. stripes ------------------------------------------------------------------------------------------------------------------------
def test_stripe_contexts_stitch_the_single_context_frame(bk):
    import torch
    table, sub = drawn_case(261, 203)
    off, tints, W, H, ps = table
    plates, lut = FB.texels(ps, 38), FB.luts(48)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    for tinted in (False, True):
        dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
        for rows in ((0, 101), (101, 102), (102, H)):                  # an odd cut, one row
            ctx = make_ctx(bk, table, sub, rows=rows)
            ctx.apply_rgba_fb_bilinear_device(ptrs, pitches, dst.data_ptr(), d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut if tinted else None)
            torch.cuda.synchronize()
            check(ctx, table, sub, plates, lut, f"rows {rows}", "pitch16", rows=rows)
            ctx.close()
        np.testing.assert_array_equal(dst.cpu().numpy(), model(plates, table, sub, d, lut if tinted else None), err_msg=f"tinted {tinted}: stitched")


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import ctypes as C
    import torch
    table, sub = drawn_case(131, 15)
    off, tints, W, H, ps = table
    plates = FB.texels(ps, 39)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx = bk.Context()
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())

    def call(ptrs=ptrs, pitches=pitches, dp=dst.data_ptr(), pitch=d["pitch"], x0=4, y0=2):
        ctx.apply_rgba_fb_bilinear_device(ptrs, pitches, dp, pitch, x0=x0, y0=y0)

    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        call()
    FB.set_table(ctx, table)                                           # the switch is off: a lensmap, no plane
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    ctx.set_subtexel(True)                                             # switched on over a map already in place: still none
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    set_table(ctx, table, sub)
    call()                                                             # (the arguments the cases below bend one at a time are fine)
    for bad in (dict(ptrs=[None] + ptrs[1:]),                          # a NULL plate whose footprint is not empty
                dict(pitches=[4 * ps - 4] + pitches[1:]),
                dict(pitches=[pitches[0] + 2] + pitches[1:]),
                dict(ptrs=[ptrs[0] + 2] + ptrs[1:]),
                dict(pitch=4 * (W + 4) - 4),
                dict(pitch=d["pitch"] + 2),
                dict(dp=dst.data_ptr() + 2),
                dict(x0=-1), dict(y0=-1)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            call(**bad)
    lib, h = bk.ffi.lib, ctx._h
    pp = (C.c_void_p * 6)(*ptrs)
    pi = (C.c_int * 6)(*pitches)
    assert lib.bk_apply_rgba_fb_bilinear_device(None, pp, pi, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_device(h, None, pi, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_device(h, pp, None, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_device(h, pp, pi, None, d["pitch"], 4, 2, None) == -1
    ctx.set_subtexel(False)                                            # switching off takes the plane away
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(d["rows"], d["pitch"])[-FB.ROWS_BELOW:], FB.FILL)
    ctx.close()
    none = bk.Context(bk.ffi.DEVICE_NONE)
    none.resize(W, H)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        none.apply_rgba_fb_bilinear_device(ptrs, pitches, dst.data_ptr(), d["pitch"])
    none.close()


# ---- 6. beside the other launches ------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_launches_on_one_context(bk):
    import torch
    table, sub = drawn_case(261, 203)
    off, tints, W, H, ps = table
    plates, lut, lut2 = FB.texels(ps, 50), FB.luts(51), FB.luts(52)
    pal = np.random.default_rng(53).integers(0, 256, (6, 256)).astype(np.uint8)
    ctx = make_ctx(bk, table, sub, slots=4)
    FB.upload_globe(ctx, plates)
    dev, ptrs, pitches = FB.source(plates, "atlas")
    d = FB.dest(W, H, False)

    def bilinear(tinted_lut):
        np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, tinted_lut), model(plates, table, sub, d, tinted_lut), err_msg=f"bilinear lut {tinted_lut is not None}")

    def nearest(tinted_lut):
        np.testing.assert_array_equal(FB.run_fb(ctx, ptrs, pitches, d, tinted_lut, False), FB.model(plates, table, d, tinted_lut, False),
                                      err_msg=f"fb lut {tinted_lut is not None}")

    def staged(tinted_lut):
        np.testing.assert_array_equal(FB.run_existing(ctx, d, tinted_lut, False), FB.model(plates, table, d, tinted_lut, False),
                                      err_msg=f"staged lut {tinted_lut is not None}")

    def apply8():
        dst = torch.full((H, W), FB.FILL, dtype=torch.uint8, device="cuda")
        ctx.apply_device(dst.data_ptr(), W, H * W, frame0=2, rubix_on=True, pal=pal)
        torch.cuda.synchronize()
        # (in numpy, not through the oracle's render_lensmap: the drawn table has tints 6 and 200, which the 8-bit apply leaves as they
        #  are and the reference - fisheye.c:2418 - would index its six palettes with)
        m = off != NULL
        v = np.ascontiguousarray(plates[..., 2]).reshape(-1)[np.where(m, off, 0)]
        t = tints.astype(np.int64)
        want = np.where(m, np.where(t < 6, pal[np.where(t < 6, t, 0), v], v), FB.FILL).astype(np.uint8).reshape(H, W)
        np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg="8-bit rubix")

    steps = [lambda: bilinear(None), lambda: nearest(None), lambda: bilinear(lut), lambda: staged(lut2), lambda: bilinear(lut2), apply8,
             lambda: nearest(lut), lambda: bilinear(lut), lambda: staged(None)]
    for step in steps + steps[::-1]:
        step()
    ctx.close()


# ---- 7. a real build ---------------------------------------------------------------------------------------------------------------------
def test_after_a_real_build(bk):
    import scripts as S
    W, H = 203, 131
    ctx = bk.Context()
    ctx.set_frames(1)
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", "panini", None, (W, H))
    display, _ = ctx.build()
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    assert len(np.unique(sub[off != NULL])) > 1000 and (sub[off == NULL] == SM.CENTRE).all()
    table = (off.reshape(-1), tints.reshape(-1), W, H, min(W, H))
    plates, lut = FB.texels(table[4], 54), FB.luts(55)
    check(ctx, table, sub, plates, lut, "built", "pitch+20", null_unread=True)
    ctx.close()
