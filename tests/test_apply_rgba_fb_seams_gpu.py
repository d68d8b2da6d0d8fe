"""bk_apply_rgba_fb_bilinear_seams_device on the GPU: the bilinear frame-buffer apply that filters across plate seams through the seam
table.  Every case compares the WHOLE destination allocation (fill 77, a pitch wider than the frame, an origin, rows below) with the
numpy model of tests/seam_model.py (held to a second formulation by tests/test_seam_table_cpu.py), and every frame is made TWICE, from
plates whose texels outside the model's read_mask hold one guard value and then another.  Tables, sources and destinations come from
the existing frame-buffer tests' generators (by import); tests/test_seam_table_cpu.py holds the cases below to their census.  Every
comparison is exact equality."""
import numpy as np
import pytest

import seam_model as M
import subtexel_model as SM
import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB

pytestmark = pytest.mark.gpu

NULL = M.NULL
GUARDS = BL.GUARDS
ALL = (True,) * 6
# W x H; ps = min(W, H): 1, 2, 9, 33, 203; W % 4 != 0 at 1, 5, 131, 130, 261
SIZES = [(1, 1), (5, 2), (131, 9), (130, 33), (261, 203)]
TINTS = np.array([0, 1, 2, 3, 4, 5, 6, 200, 255], np.uint8)


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def drawn_seams(ps, seed, null_share=0.25):
    """uint32 [6][4][ps + 2]: arbitrary targets on any plate (the own one included), NULLs, non-monotone; a corner's two copies agree"""
    rng = np.random.default_rng(9100 + 31 * seed + ps)
    t = rng.integers(0, 6 * ps * ps, (6, 4, ps + 2)).astype(np.uint32)
    t[rng.random(t.shape) < null_share] = NULL
    t[:, 2, 0], t[:, 3, 0], t[:, 2, -1], t[:, 3, -1] = t[:, 0, 0], t[:, 0, -1], t[:, 1, 0], t[:, 1, -1]
    return t


def rim_case(W, H, seed=0):
    """(table, sub): every pixel on the rim of its plate - a corner, or an edge at a random place - with the plane's axes from 0, 127, 128,
    255 half the time and any value otherwise; every fifth pixel of the odd columns NULL; tints 0..5, 6, 200, 255"""
    ps = min(W, H)
    rng = np.random.default_rng(9200 + 13 * seed + W + H)
    n = W * H
    rim = lambda: np.where(rng.random(n) < 0.5, 0, ps - 1)
    kind = rng.integers(0, 3, n)
    px = np.where(kind == 2, rng.integers(0, ps, n), rim())
    py = np.where(kind == 1, rng.integers(0, ps, n), rim())
    off = (rng.integers(0, 6, n) * ps * ps + py * ps + px).astype(np.uint32)
    off[(np.arange(n) % W % 2 == 1) & (np.arange(n) % 5 == 0)] = NULL
    tints = TINTS[rng.integers(0, 9, n)]
    axis = lambda: np.where(rng.random(n) < 0.5, BL.EDGE_VALUES[rng.integers(0, 4, n)], rng.integers(0, 256, n))
    return (off, tints, W, H, ps), (axis() | (axis() << 8)).astype(np.uint16)


def walk_case():
    """256 x 64, ps 64: qx walks 0..255 along a row, qy all 256 values over the frame; the drawn table's texels, every fourth on a rim"""
    off, tints, W, H, ps = FB.drawn_table(256, 64, 1)
    off = off.copy()
    k = np.flatnonzero(off != NULL)[::4]
    plate, rem = off[k] // (ps * ps), off[k] % (ps * ps)
    off[k] = plate * ps * ps + np.where(k % 8 == 0, 0, ps - 1) * ps + rem % ps      # row 0 or ps - 1
    return (off, tints, W, H, ps), BL.walk_case()[1]


def computed_cube_table(bk, ps):
    """the cube's own table at platesize ps, from a device-less context"""
    import scripts as S
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.resize(ps + 3, ps)
    t = ctx.read_seam_table().copy()
    ctx.close()
    return t


def committed_cases():
    """(table, sub, seam table, which plates are given) of the cases below that the census runs over"""
    cases = []
    for W, H in SIZES:
        for seed in (0, 1):
            table, sub = BL.drawn_case(W, H, seed)
            cases.append((table, sub, drawn_seams(table[4], seed), ALL))
            table, sub = rim_case(W, H, seed)
            cases.append((table, sub, drawn_seams(table[4], 2 + seed), ALL))
    table, sub = walk_case()
    cases.append((table, sub, drawn_seams(64, 5), ALL))
    table, sub = null_plate_table()
    cases.append((table, sub, drawn_seams(9, 7, 0.0), null_plate_case(table)))
    return cases


def null_plate_table():
    """rim_case(131, 9) with plates 4 and 5 unnamed"""
    (off, tints, W, H, ps), sub = rim_case(131, 9, 7)
    off = np.where(off // (ps * ps) >= 4, NULL, off).astype(np.uint32)      # (NULL // ps^2 is far above 4)
    return (off, tints, W, H, ps), sub


def null_plate_case(table):
    """which plates are given when every plate the table does not name is passed as NULL"""
    off, tints, W, H, ps = table
    named = set((off[off != NULL] // (ps * ps)).tolist())
    return tuple(p in named for p in range(6))


# ---- running it -------------------------------------------------------------------------------------------------------------------------
def make_ctx(bk, table, sub, seams, rows=None, slots=1):
    ctx = BL.make_ctx(bk, table, sub, rows, slots)
    if seams is not None:
        ctx.set_seam_table(seams)
    return ctx


def run(ctx, ptrs, pitches, d, lut, ptr_off=0):
    import torch
    dst = torch.full((ptr_off + d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_fb_bilinear_seams_device(ptrs, pitches, dst.data_ptr() + ptr_off, d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def model(plates, table, sub, seams, d, lut, rows=None, given=ALL):
    off, tints, W, H, ps = table
    want = np.full(d["rows"] * d["pitch"], FB.FILL, np.uint8)
    M.seam_frame(plates, off, sub, tints, W, H, ps, rows or (0, H), lut, want.reshape(d["rows"], d["pitch"]), d["x0"], d["y0"], seams, given)
    return want


def check(ctx, table, sub, seams, plates, lut, what, layout="tight", rows=None, d=None, given=ALL):
    """plain and tinted, each from both guarded copies of the plates, against the model of the TRUE plates"""
    off, tints, W, H, ps = table
    d = d or FB.dest(W, H, False)
    r0, r1 = rows or (0, H)
    mask = M.read_mask(np.asarray(off).reshape(H, W)[r0:r1], None, ps, seams)
    skip = [p for p in range(6) if not given[p]]
    for guard in GUARDS:
        g = plates.copy()
        g[~mask] = guard
        dev, ptrs, pitches = FB.source(g, layout, skip=skip)
        for tinted in (False, True):
            got = run(ctx, ptrs, pitches, d, lut if tinted else None)
            np.testing.assert_array_equal(got, model(plates, table, sub, seams, d, lut if tinted else None, rows, given),
                                          err_msg=f"{what} {'tinted' if tinted else 'plain'} guard {guard:#x}: the model")


# ---- 1. drawn tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_drawn_tables_and_rims(bk, W, H):
    for seed in (0, 1):
        for kind, (table, sub), seams in (("drawn", BL.drawn_case(W, H, seed), drawn_seams(min(W, H), seed)),
                                          ("rim", rim_case(W, H, seed), drawn_seams(min(W, H), 2 + seed))):
            plates, lut = FB.texels(table[4], 60 + seed), FB.luts(70 + seed)
            ctx = make_ctx(bk, table, sub, seams)
            check(ctx, table, sub, seams, plates, lut, f"{kind} {W}x{H} seed {seed}", FB.LAYOUTS[(W + seed) % len(FB.LAYOUTS)])
            ctx.close()


def test_subs_that_walk_every_value_of_both_axes(bk):
    table, sub = walk_case()
    assert set(sub & 255) == set(range(256)) and set(sub >> 8) == set(range(256))
    seams = drawn_seams(64, 5)
    plates, lut = FB.texels(64, 62), FB.luts(72)
    ctx = make_ctx(bk, table, sub, seams)
    check(ctx, table, sub, seams, plates, lut, "walk", "pitch16")
    ctx.close()


@pytest.mark.parametrize("W,H", [(131, 9), (130, 33)])
def test_every_corner_and_edge_with_the_computed_cube_table(bk, W, H):
    table, sub = rim_case(W, H, 3)
    ps = table[4]
    seams = computed_cube_table(bk, ps)
    plates, lut = FB.texels(ps, 63), FB.luts(73)
    ctx = make_ctx(bk, table, sub, seams)
    check(ctx, table, sub, seams, plates, lut, "cube table", "six-pitches")
    ctx.close()


# ---- 2. the two identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_an_all_null_table_is_the_bilinear_apply_and_a_plane_of_centres_the_nearest_one(bk, W, H):
    table, sub = rim_case(W, H, 4)
    ps = table[4]
    plates, lut = FB.texels(ps, 64), FB.luts(74)
    dev, ptrs, pitches = FB.source(plates, "pitch+20")
    d = FB.dest(W, H, False)
    ctx = make_ctx(bk, table, sub, np.full((6, 4, ps + 2), NULL, np.uint32))
    for l in (None, lut):
        np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, l), BL.run(ctx, ptrs, pitches, d, l), err_msg="all NULL: the bilinear call")
    ctx.set_seam_table(drawn_seams(ps, 4))
    BL.set_table(ctx, table, None)                                     # bk_set_lensmap alone: a plane of centres
    for l in (None, lut):
        np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, l), FB.run_fb(ctx, ptrs, pitches, d, l, False), err_msg="centres: the nearest call")
    ctx.close()


# ---- 3. tints, NULL plates ------------------------------------------------------------------------------------------------------------------
def test_the_tint_is_the_pixels_not_the_targets(bk):
    table, sub = rim_case(131, 9, 5)
    off, tints, W, H, ps = table
    seams = drawn_seams(ps, 6, 0.0)                                      # non-monotone, no NULL: every outside position is resolved
    plates, lut = FB.texels(ps, 65), FB.luts(75)
    ctx = make_ctx(bk, table, sub, seams)
    check(ctx, table, sub, seams, plates, lut, "tints", "pitch16")
    # the mutant "tint by the target's plate" gives another frame on these inputs: the check above can tell
    P, _, _, R, _, _ = M.positions(off, sub, ps, seams)
    m = (off != NULL) & (tints < 6)
    assert (R & (P != tints.astype(np.int64)) & m).any()
    ctx.close()


def test_a_null_plate_clamps_the_entries_into_it(bk):
    table, sub = null_plate_table()
    off, tints, W, H, ps = table
    given = null_plate_case(table)
    assert given == (True, True, True, True, False, False)
    seams = drawn_seams(ps, 7, 0.0)
    assert ((seams // (ps * ps)) >= 4).any()
    plates, lut = FB.texels(ps, 66), FB.luts(76)
    ctx = make_ctx(bk, table, sub, seams)
    check(ctx, table, sub, seams, plates, lut, "NULL plates", "ptr4", given=given)
    # ... which is the frame of the same table with those entries NULLed, all plates given
    nulled = np.where((seams != NULL) & (seams // (ps * ps) >= 4), NULL, seams).astype(np.uint32)
    d = FB.dest(W, H, False)
    np.testing.assert_array_equal(model(plates, table, sub, seams, d, lut, given=given), model(plates, table, sub, nulled, d, lut))
    ctx.close()


# ---- 4. sources and destinations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", FB.LAYOUTS)
def test_source_classes(bk, layout):
    table, sub = rim_case(261, 203)
    seams = drawn_seams(203, 8)
    plates, lut = FB.texels(203, 67), FB.luts(77)
    ctx = make_ctx(bk, table, sub, seams)
    check(ctx, table, sub, seams, plates, lut, layout, layout)
    ctx.close()


@pytest.mark.parametrize("cls", FB.G.ALIGN_CLASSES)
@pytest.mark.parametrize("W,H", [(256, 64), (131, 9)])
def test_destination_classes(bk, W, H, cls):
    table, sub = rim_case(W, H, 9)
    seams = drawn_seams(table[4], 9)
    plates, lut = FB.texels(table[4], 68), FB.luts(78)
    ctx = make_ctx(bk, table, sub, seams)
    x0 = {"16": 4, "8-only": 2, "4-only": 1}[cls]
    px_pitch = (W + x0 + 3) // 4 * 4 + {"16": 4, "8-only": 2, "4-only": 1}[cls]
    d = FB.dest(W, H, False, x0=x0, y0=2, extra_px=px_pitch - W)
    assert FB.G.align_class(d["y0"] * d["pitch"] + 4 * x0, d["pitch"], 0) == cls
    check(ctx, table, sub, seams, plates, lut, f"{W}x{H} {cls}", "pitch16", d=d)
    ctx.close()


# ---- 5. stripes ---------------------------------------------------------------------------------------------------------------------------
def test_stripe_contexts_stitch_the_single_context_frame(bk):
    import torch
    table, sub = rim_case(261, 203, 10)
    off, tints, W, H, ps = table
    seams = drawn_seams(ps, 10)
    plates, lut = FB.texels(ps, 69), FB.luts(79)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    for l in (None, lut):
        dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
        for rows in ((0, 101), (101, 102), (102, H)):                  # an odd cut, one row
            ctx = make_ctx(bk, table, sub, seams, rows=rows)
            ctx.apply_rgba_fb_bilinear_seams_device(ptrs, pitches, dst.data_ptr(), d["pitch"], x0=d["x0"], y0=d["y0"], lut=l)
            torch.cuda.synchronize()
            ctx.close()
        np.testing.assert_array_equal(dst.cpu().numpy(), model(plates, table, sub, seams, d, l), err_msg="stitched")


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import ctypes as C
    import torch
    table, sub = rim_case(131, 9)
    off, tints, W, H, ps = table
    plates = FB.texels(ps, 80)
    dev, ptrs, pitches = FB.source(plates, "pitch16")
    d = FB.dest(W, H, False)
    dst = torch.full((d["rows"] * d["pitch"],), FB.FILL, dtype=torch.uint8, device="cuda")
    ctx = bk.Context()
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())

    def call(ptrs=ptrs, pitches=pitches, dp=dst.data_ptr(), pitch=d["pitch"], x0=4, y0=2):
        ctx.apply_rgba_fb_bilinear_seams_device(ptrs, pitches, dp, pitch, x0=x0, y0=y0)

    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        call()
    FB.set_table(ctx, table)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        call()
    ctx.set_subtexel(True)
    BL.set_table(ctx, table, sub)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*globe"):           # no globe, no table set: the seam table cannot be made
        call()
    ctx.set_seam_table(drawn_seams(ps, 11))
    call()
    for bad in (dict(ptrs=[None] + ptrs[1:]), dict(pitches=[4 * ps - 4] + pitches[1:]), dict(pitches=[pitches[0] + 2] + pitches[1:]),
                dict(ptrs=[ptrs[0] + 2] + ptrs[1:]), dict(pitch=4 * (W + 4) - 4), dict(pitch=d["pitch"] + 2), dict(dp=dst.data_ptr() + 2),
                dict(x0=-1), dict(y0=-1)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            call(**bad)
    lib, h = bk.ffi.lib, ctx._h
    pp, pi = (C.c_void_p * 6)(*ptrs), (C.c_int * 6)(*pitches)
    assert lib.bk_apply_rgba_fb_bilinear_seams_device(None, pp, pi, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_seams_device(h, None, pi, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_seams_device(h, pp, None, dst.data_ptr(), d["pitch"], 4, 2, None) == -1
    assert lib.bk_apply_rgba_fb_bilinear_seams_device(h, pp, pi, None, d["pitch"], 4, 2, None) == -1
    assert lib.bk_read_seam_table(h, None) == -1 and lib.bk_set_seam_table(h, None) == -1
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(d["rows"], d["pitch"])[-FB.ROWS_BELOW:], FB.FILL)
    ctx.close()
    none = bk.Context(bk.ffi.DEVICE_NONE)
    none.resize(W, H)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        none.apply_rgba_fb_bilinear_seams_device(ptrs, pitches, dst.data_ptr(), d["pitch"])
    none.close()


# ---- 7. beside the other launches -----------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_launches_on_one_context(bk):
    import torch
    table, sub = rim_case(261, 203, 12)
    off, tints, W, H, ps = table
    seams, seams2 = drawn_seams(ps, 12), drawn_seams(ps, 13)
    plates, lut, lut2 = FB.texels(ps, 81), FB.luts(82), FB.luts(83)
    pal = np.random.default_rng(84).integers(0, 256, (6, 256)).astype(np.uint8)
    ctx = make_ctx(bk, table, sub, seams, slots=4)
    FB.upload_globe(ctx, plates)
    dev, ptrs, pitches = FB.source(plates, "atlas")
    d = FB.dest(W, H, False)
    current = [seams]

    def seamed(l):
        np.testing.assert_array_equal(run(ctx, ptrs, pitches, d, l), model(plates, table, sub, current[0], d, l), err_msg=f"seams lut {l is not None}")

    def swap():
        current[0] = seams2 if current[0] is seams else seams
        ctx.set_seam_table(current[0])

    def bilinear(l):
        np.testing.assert_array_equal(BL.run(ctx, ptrs, pitches, d, l), BL.model(plates, table, sub, d, l), err_msg=f"bilinear lut {l is not None}")

    def nearest(l):
        np.testing.assert_array_equal(FB.run_fb(ctx, ptrs, pitches, d, l, False), FB.model(plates, table, d, l, False), err_msg=f"fb lut {l is not None}")

    def staged(l):
        np.testing.assert_array_equal(FB.run_existing(ctx, d, l, False), FB.model(plates, table, d, l, False), err_msg=f"staged lut {l is not None}")

    def apply8():
        dst = torch.full((H, W), FB.FILL, dtype=torch.uint8, device="cuda")
        ctx.apply_device(dst.data_ptr(), W, H * W, frame0=2, rubix_on=True, pal=pal)
        torch.cuda.synchronize()
        m = off != NULL
        v = np.ascontiguousarray(plates[..., 2]).reshape(-1)[np.where(m, off, 0)]
        t = tints.astype(np.int64)
        want = np.where(m, np.where(t < 6, pal[np.where(t < 6, t, 0), v], v), FB.FILL).astype(np.uint8).reshape(H, W)
        np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg="8-bit rubix")

    steps = [lambda: seamed(None), lambda: nearest(None), lambda: seamed(lut), lambda: bilinear(lut2), swap, lambda: seamed(lut2), apply8,
             lambda: staged(lut), lambda: seamed(lut), lambda: bilinear(None)]
    for step in steps + steps[::-1]:
        step()
    ctx.close()


# ---- 8. a real build ------------------------------------------------------------------------------------------------------------------------
def test_after_a_real_build_with_the_computed_table(bk):
    import scripts as S
    W, H = 203, 131
    ctx = bk.Context()
    ctx.set_frames(1)
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", "panini", None, (W, H))
    ctx.build()
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    seams = ctx.read_seam_table()
    np.testing.assert_array_equal(seams, computed_cube_table(bk, min(W, H)))
    table = (off.reshape(-1), tints.reshape(-1), W, H, min(W, H))
    _, _, _, R, _, _ = M.positions(table[0], sub, table[4], seams)
    assert (R.any(0) & (table[0] != NULL)).sum() > 50                  # the seams run through the picture
    plates, lut = FB.texels(table[4], 85), FB.luts(86)
    check(ctx, table, sub, seams, plates, lut, "built", "pitch+20")
    # bk_build leaves the table alone: one that no computation gives is still there after a build, and the frame follows it
    drawn = drawn_seams(table[4], 14)
    assert (drawn != seams).any()
    ctx.set_seam_table(drawn)
    ctx.build()
    np.testing.assert_array_equal(ctx.read_seam_table(), drawn, err_msg="bk_build dropped a table that was set")
    off2, tints2 = ctx.read_lensmap()
    np.testing.assert_array_equal(off2.reshape(-1), table[0])
    check(ctx, table, sub, drawn, plates, lut, "built, a set table kept across bk_build", "pitch+20")
    ctx.close()
