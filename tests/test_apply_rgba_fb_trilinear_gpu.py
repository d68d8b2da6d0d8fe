"""bk_apply_rgba_fb_trilinear_device on the GPU: the frame-buffer apply blended between two levels of a mip pyramid of the plates.  Every
frame is compared over the WHOLE destination allocation (fill 77, a pitch wider than the frame, an origin, rows below) with the numpy
model of tests/trilinear_model.py (held to a second formulation, and its drawn cases to a census, by tests/test_trilinear_cpu.py).  A
case makes its frame with mips = 1 from the true plates, and then twice with mips = 0 from plates whose level-0 texels farther than
one from a named texel hold one guard value and then another: level 0 is read as the bilinear call reads it, everything else comes
from the pyramid.  Tables, sub planes, plates and layouts are the bilinear tests' (by import); planes are set by hand through
bk_set_lensmap_lod unless a test says otherwise.  Every comparison is exact equality."""
import numpy as np
import pytest

import scripts as S
import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB
import trilinear_model as TM

pytestmark = pytest.mark.gpu

NULL = TM.NULL
SIZES = BL.SIZES


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def with_lods(case, seed):
    table, sub = case
    off, tints, W, H, ps = table
    return table, sub, TM.random_lods(W * H, ps, seed)


def drawn_case(W, H, seed=0):
    return with_lods(BL.drawn_case(W, H, seed), 10 * seed + W + H)


def committed_cases():
    """every (table, sub, lod) the tests below apply through drawn tables: what the census of tests/test_trilinear_cpu.py runs over"""
    return [drawn_case(W, H, seed) for W, H in SIZES for seed in (0, 1)] + [with_lods(BL.walk_case(), 5), with_lods(BL.corner_case(), 6)]


# ---- running it -----------------------------------------------------------------------------------------------------------------------
def make_ctx(bk, table, sub, lod, rows=None, slots=1):
    off, tints, W, H, ps = table
    ctx = BL.make_ctx(bk, table, sub, rows, slots)
    if lod is not None:
        r0, r1 = rows or (0, H)
        ctx.set_lensmap_lod(np.asarray(lod).reshape(H, W)[r0:r1])
    return ctx


def run(ctx, ptrs, pitches, d, lut, mips=True, ptr_off=0):
    import torch
    dst = torch.full((ptr_off + d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr() + ptr_off, d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut, mips=mips)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def model(pyr, table, sub, lod, d, lut, rows=None):
    """lod: the WHOLE frame's plane ([H * W]); the owned rows' part is what the call uses"""
    off, tints, W, H, ps = table
    r0, r1 = rows or (0, H)
    want = np.full(d["rows"] * d["pitch"], FB.FILL, np.uint8)
    TM.trilinear_frame(pyr, off, sub, np.asarray(lod).reshape(H, W)[r0:r1], tints, W, H, ps, (r0, r1), lut, want.reshape(d["rows"], d["pitch"]), d["x0"], d["y0"])
    return want


def same(got, want, d, what):
    """two whole destination allocations are equal; if not, the first differing byte as a pixel of the frame"""
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        y, xb = divmod(at, d["pitch"])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {want.size} bytes differ, the first at pixel (x {xb // 4 - d['x0']}, y {y - d['y0']}) "
                             f"byte {xb % 4}: {int(got[at])}, expected {int(want[at])}")


def check(ctx, table, sub, lod, plates, lut, what, layout="tight", rows=None, d=None, null_unread=False, pyr=None):
    """pyr: TM.pyramid(plates), where the caller has it already"""
    off, tints, W, H, ps = table
    d = d or FB.dest(W, H, False)
    pyr = pyr or TM.pyramid(plates)
    _, mask = BL.guarded(plates, table, sub, 0, rows)
    skip = [p for p in range(6) if not mask[p].any()] if null_unread else ()
    dev, ptrs, pitches = FB.source(plates, layout, skip=skip)
    if skip:                                                           # (their levels, never made, must not matter: no entry names them)
        pyr = [pyr[0]] + [np.where(np.isin(np.arange(6), skip)[:, None, None, None], 0, level) for level in pyr[1:]]
    for tinted in (False, True):
        got = run(ctx, ptrs, pitches, d, lut if tinted else None)
        same(got, model(pyr, table, sub, lod, d, lut if tinted else None, rows), d, f"{what} tinted {tinted} mips 1")
    for guard in BL.GUARDS:
        g, _ = BL.guarded(plates, table, sub, guard, rows)
        devg, ptrsg, pitchesg = FB.source(g, layout, skip=skip)
        for tinted in (False, True):
            got = run(ctx, ptrsg, pitchesg, d, lut if tinted else None, mips=False)
            same(got, model(pyr, table, sub, lod, d, lut if tinted else None, rows), d, f"{what} tinted {tinted} mips 0 guard {guard:#x}")


# ---- 1. drawn tables, planes set by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_drawn_tables(bk, W, H):
    for seed in (0, 1):
        table, sub, lod = drawn_case(W, H, seed)
        plates, lut = FB.texels(table[4], 80 + seed), FB.luts(90 + seed)
        ctx = make_ctx(bk, table, sub, lod)
        check(ctx, table, sub, lod, plates, lut, f"drawn {W}x{H} seed {seed}", FB.LAYOUTS[(W + seed) % len(FB.LAYOUTS)])
        ctx.close()


@pytest.mark.parametrize("which", ["walk", "corners"])
def test_every_sub_value_and_every_rim(bk, which):
    table, sub, lod = with_lods(BL.walk_case(), 5) if which == "walk" else with_lods(BL.corner_case(), 6)
    plates, lut = FB.texels(table[4], 82), FB.luts(92)
    ctx = make_ctx(bk, table, sub, lod)
    check(ctx, table, sub, lod, plates, lut, which, "pitch16" if which == "walk" else "six-pitches")
    ctx.close()


@pytest.mark.parametrize("layout", FB.LAYOUTS)
def test_source_classes(bk, layout):
    table, sub, lod = drawn_case(261, 203)
    plates, lut = FB.texels(table[4], 83), FB.luts(93)
    ctx = make_ctx(bk, table, sub, lod)
    check(ctx, table, sub, lod, plates, lut, layout, layout, null_unread=layout == "atlas")
    ctx.close()


def test_unread_plates_may_be_null(bk):
    off, tints, W, H, ps = FB.drawn_table(131, 15)
    off = np.where(off // (ps * ps) >= 3, NULL, off).astype(np.uint32)
    table, sub = (off, tints, W, H, ps), BL.random_subs(W * H, 3)
    lod = TM.random_lods(W * H, ps, 7)
    plates, lut = FB.texels(ps, 84), FB.luts(94)
    ctx = make_ctx(bk, table, sub, lod)
    check(ctx, table, sub, lod, plates, lut, "NULL plates", "ptr4", null_unread=True)
    ctx.close()


@pytest.mark.parametrize("cls", FB.G.ALIGN_CLASSES)
def test_destination_classes(bk, cls):
    W, H = 131, 15
    table, sub, lod = drawn_case(W, H)
    plates, lut = FB.texels(table[4], 85), FB.luts(95)
    ctx = make_ctx(bk, table, sub, lod)
    x0 = {"16": 4, "8-only": 2, "4-only": 1}[cls]
    px_pitch = (W + x0 + 3) // 4 * 4 + {"16": 4, "8-only": 2, "4-only": 1}[cls]
    d = FB.dest(W, H, False, x0=x0, y0=2, extra_px=px_pitch - W)
    assert FB.G.align_class(d["y0"] * d["pitch"] + 4 * x0, d["pitch"], 0) == cls
    check(ctx, table, sub, lod, plates, lut, cls, "pitch16", d=d)
    ctx.close()


# ---- 2. derived planes on real builds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(203, 131), (96, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("lens", ["hammer", "panini", "quincuncial", "winkel2"])
def test_derived_planes_on_real_builds(bk, lens, size):
    W, H = size
    ctx = bk.Context()
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", lens, None, size)
    ctx.build()
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    ps = min(W, H)
    lod = TM.derive_lod(off, sub, W, H, ps)
    # (levels above 0 are in play: panini, which magnifies its centre, has 4.6 % of 203 x 131 at level 1 or above - test_trilinear_cpu.py)
    assert (lod >= 256).sum() > W * H // 50
    table = (off, tints, W, H, ps)
    plates, lut = FB.texels(ps, 86), FB.luts(96)
    check(ctx, table, sub, lod, plates, lut, f"{lens} {size}", "pitch+20", null_unread=True)
    np.testing.assert_array_equal(ctx.read_lod(), lod)
    ctx.close()


# ---- 3. identities and the purpose -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_a_plane_of_zeros_is_the_bilinear_call_and_with_centres_the_nearest_call(bk, W, H):
    table, sub = BL.drawn_case(W, H, 1)
    plates, lut = FB.texels(table[4], 87), FB.luts(97)
    dev, ptrs, pitches = FB.source(plates, "pitch+20")
    d = FB.dest(W, H, False)
    ctx = make_ctx(bk, table, sub, np.zeros(W * H, np.uint16))
    for tinted in (False, True):
        got = run(ctx, ptrs, pitches, d, lut if tinted else None)
        np.testing.assert_array_equal(got, BL.run(ctx, ptrs, pitches, d, lut if tinted else None), err_msg=f"tinted {tinted}: the bilinear call")
    BL.set_table(ctx, table, None)                                     # bk_set_lensmap alone: subs of 0x8080, and the plane is dropped
    ctx.set_lensmap_lod(np.zeros(W * H, np.uint16))
    for tinted in (False, True):
        got = run(ctx, ptrs, pitches, d, lut if tinted else None)
        np.testing.assert_array_equal(got, FB.run_fb(ctx, ptrs, pitches, d, lut if tinted else None, False), err_msg=f"tinted {tinted}: the nearest call")
    ctx.close()


def test_a_checkerboard_at_level_one_is_grey(bk):
    """what the call is for: one-texel checkers of 0 / 255, every pixel at lod 256 - level 1 is 128 throughout, nearest gives 0 and 255"""
    W = H = ps = 16
    rng = np.random.default_rng(99)
    n = W * H
    off = (rng.integers(0, 6, n) * ps * ps + rng.integers(0, ps, n) * ps + rng.integers(0, ps, n)).astype(np.uint32)
    off[::9] = NULL
    table, sub = (off, np.full(n, 255, np.uint8), W, H, ps), BL.random_subs(n, 9)
    y, x = np.divmod(np.arange(ps * ps), ps)
    board = np.repeat((((x + y) % 2) * 255).astype(np.uint8).reshape(1, ps, ps, 1), 6, axis=0).repeat(4, axis=3)
    dev, ptrs, pitches = FB.source(board)
    d = FB.dest(W, H, False)
    ctx = make_ctx(bk, table, sub, np.full(n, 256, np.uint16))
    got = run(ctx, ptrs, pitches, d, None)
    want = np.full(d["rows"] * d["pitch"], FB.FILL, np.uint8).reshape(d["rows"], d["pitch"])
    window = want[d["y0"]:d["y0"] + H, 4 * d["x0"]:4 * (d["x0"] + W)].reshape(H, W, 4)
    window[(off != NULL).reshape(H, W)] = 128
    np.testing.assert_array_equal(got, want.reshape(-1))
    nearest = FB.run_fb(ctx, ptrs, pitches, d, None, False).reshape(d["rows"], d["pitch"])
    seen = set(nearest[d["y0"]:d["y0"] + H, 4 * d["x0"]:4 * (d["x0"] + W)].reshape(H, W, 4)[(off != NULL).reshape(H, W)].reshape(-1).tolist())
    assert seen == {0, 255}
    ctx.close()


def test_mips_0_shows_the_pyramid_as_last_made(bk):
    table, sub, lod = drawn_case(131, 15)
    old, new, lut = FB.texels(table[4], 88), FB.texels(table[4], 89), FB.luts(98)
    d = FB.dest(131, 15, False)
    ctx = make_ctx(bk, table, sub, lod)
    dev, ptrs, pitches = FB.source(old)
    run(ctx, ptrs, pitches, d, None)
    dev2, ptrs2, pitches2 = FB.source(new, "pitch16")
    stale = [new] + TM.pyramid(old)[1:]
    for tinted in (False, True):
        np.testing.assert_array_equal(run(ctx, ptrs2, pitches2, d, lut if tinted else None, mips=False), model(stale, table, sub, lod, d, lut if tinted else None))
    np.testing.assert_array_equal(run(ctx, ptrs2, pitches2, d, None), model(TM.pyramid(new), table, sub, lod, d, None))
    ctx.close()


# ---- 4. stripes ------------------------------------------------------------------------------------------------------------------------
def test_stripe_contexts_stitch_the_single_context_frame(bk):
    import torch
    table, sub, lod = drawn_case(261, 203)
    off, tints, W, H, ps = table
    plates, lut = FB.texels(ps, 100), FB.luts(101)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    pyr = TM.pyramid(plates)
    for tinted in (False, True):
        dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
        for rows in ((0, 101), (101, 102), (102, H)):                  # an odd cut, one row
            ctx = make_ctx(bk, table, sub, lod, rows=rows)
            ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr(), d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut if tinted else None)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, lut if tinted else None), model(pyr, table, sub, lod, d, lut if tinted else None, rows),
                                          err_msg=f"rows {rows}")
            ctx.close()
        np.testing.assert_array_equal(dst.cpu().numpy(), model(pyr, table, sub, lod, d, lut if tinted else None), err_msg=f"tinted {tinted}: stitched")


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import ctypes as C
    import torch
    table, sub, lod = drawn_case(131, 15)
    off, tints, W, H, ps = table
    plates = FB.texels(ps, 102)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx = bk.Context()
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())

    def call(ptrs=ptrs, pitches=pitches, dp=dst.data_ptr(), pitch=d["pitch"], x0=4, y0=2, mips=True):
        ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dp, pitch, x0=x0, y0=y0, mips=mips)

    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        call()
    FB.set_table(ctx, table)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    ctx.set_subtexel(True)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    BL.set_table(ctx, table, sub)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*mips = 0"):
        call(mips=False)
    call()
    call(mips=False)
    lib, h = bk.ffi.lib, ctx._h
    pp = (C.c_void_p * 6)(*ptrs)
    pi = (C.c_int * 6)(*pitches)
    for mips in (2, -1):
        assert lib.bk_apply_rgba_fb_trilinear_device(h, pp, pi, dst.data_ptr(), d["pitch"], 4, 2, None, mips) == -1
    for bad in (dict(ptrs=[None] + ptrs[1:]), dict(pitches=[4 * ps - 4] + pitches[1:]), dict(pitches=[pitches[0] + 2] + pitches[1:]),
                dict(ptrs=[ptrs[0] + 2] + ptrs[1:]), dict(pitch=4 * (W + 4) - 4), dict(pitch=d["pitch"] + 2), dict(dp=dst.data_ptr() + 2),
                dict(x0=-1), dict(y0=-1)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            call(**bad)
    assert lib.bk_apply_rgba_fb_trilinear_device(None, pp, pi, dst.data_ptr(), d["pitch"], 4, 2, None, 1) == -1
    assert lib.bk_apply_rgba_fb_trilinear_device(h, None, pi, dst.data_ptr(), d["pitch"], 4, 2, None, 1) == -1
    assert lib.bk_apply_rgba_fb_trilinear_device(h, pp, None, dst.data_ptr(), d["pitch"], 4, 2, None, 1) == -1
    assert lib.bk_apply_rgba_fb_trilinear_device(h, pp, pi, None, d["pitch"], 4, 2, None, 1) == -1
    ctx.set_subtexel(False)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(d["rows"], d["pitch"])[-FB.ROWS_BELOW:], FB.FILL)
    ctx.close()
    none = bk.Context(bk.ffi.DEVICE_NONE)
    none.resize(W, H)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        none.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr(), d["pitch"])
    none.close()


# ---- 6. beside the other launches ------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_launches_on_one_context(bk):
    import torch
    table, sub, lod = drawn_case(261, 203)
    off, tints, W, H, ps = table
    plates, lut, lut2 = FB.texels(ps, 103), FB.luts(104), FB.luts(105)
    pal = np.random.default_rng(106).integers(0, 256, (6, 256)).astype(np.uint8)
    ctx = make_ctx(bk, table, sub, lod, slots=4)
    FB.upload_globe(ctx, plates)
    dev, ptrs, pitches = FB.source(plates, "atlas")
    d = FB.dest(W, H, False)
    pyr = TM.pyramid(plates)
    import test_apply_rgba_fb_seams_gpu as SE
    seam_table = SE.drawn_seams(ps, 4)
    ctx.set_seam_table(seam_table)

    def trilinear(tinted_lut, mips=True):
        np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, tinted_lut, mips), model(pyr, table, sub, lod, d, tinted_lut), err_msg="trilinear")

    def bilinear(tinted_lut):
        np.testing.assert_array_equal(BL.run(ctx, ptrs, pitches, d, tinted_lut), BL.model(plates, table, sub, d, tinted_lut), err_msg="bilinear")

    def nearest(tinted_lut, ss2=False):
        ds = FB.dest(W, H, ss2)
        np.testing.assert_array_equal(FB.run_fb(ctx, ptrs, pitches, ds, tinted_lut, ss2), FB.model(plates, table, ds, tinted_lut, ss2), err_msg=f"fb ss2 {ss2}")

    def staged(tinted_lut):
        np.testing.assert_array_equal(FB.run_existing(ctx, d, tinted_lut, False), FB.model(plates, table, d, tinted_lut, False), err_msg="staged")

    def seams(tinted_lut):
        np.testing.assert_array_equal(SE.run(ctx, ptrs, pitches, d, tinted_lut), SE.model(plates, table, sub, seam_table, d, tinted_lut), err_msg="seams")

    def apply8():
        dst = torch.full((H, W), FB.FILL, dtype=torch.uint8, device="cuda")
        ctx.apply_device(dst.data_ptr(), W, H * W, frame0=2, rubix_on=True, pal=pal)
        torch.cuda.synchronize()
        m = off != NULL
        v = np.ascontiguousarray(plates[..., 2]).reshape(-1)[np.where(m, off, 0)]
        t = tints.astype(np.int64)
        want = np.where(m, np.where(t < 6, pal[np.where(t < 6, t, 0), v], v), FB.FILL).astype(np.uint8).reshape(H, W)
        np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg="8-bit rubix")

    steps = [lambda: trilinear(None), lambda: nearest(None), lambda: trilinear(lut), lambda: staged(lut2), lambda: trilinear(lut2, False), apply8,
             lambda: bilinear(lut), lambda: seams(lut), lambda: trilinear(lut), lambda: nearest(lut2, True), lambda: seams(None), lambda: staged(None),
             lambda: trilinear(None, False), lambda: bilinear(None)]
    for step in steps + steps[::-1]:
        step()
    ctx.close()
