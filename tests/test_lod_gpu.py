"""The level-of-detail plane on the GPU: bk_read_lod against tests/trilinear_model.py's derivation from bk_read_lensmap +
bk_read_subtexel (held to a pixel loop, and to the counts that make it say something, by tests/test_trilinear_cpu.py) - device builds,
stripes, biases, drawn tables - and the plane's life: when it is derived again, how long a set plane holds, the errors."""
import numpy as np
import pytest

import scripts as S
import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB
import trilinear_model as TM

pytestmark = pytest.mark.gpu

NULL = TM.NULL
BIASES = (-300, 0, 300)
STRIPES = (None, (37, 90), (50, 51))                                    # the full frame, an odd cut, one row


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def drawn_cases():
    """(table, sub) of every drawn table below: what the census of tests/test_trilinear_cpu.py runs over"""
    return [BL.drawn_case(W, H, seed) for W, H in BL.SIZES for seed in (0, 1)]


def expect(ctx, bias=0):
    """the model's plane from what the context itself reads back"""
    w, h, ps, r0, r1 = ctx.size()
    off, _ = ctx.read_lensmap()
    return TM.derive_lod(off, ctx.read_subtexel(), w, r1 - r0, ps, bias)


@pytest.mark.parametrize("W,H", BL.SIZES)
def test_drawn_tables(bk, W, H):
    for seed in (0, 1):
        table, sub = BL.drawn_case(W, H, seed)
        off, tints, _, _, ps = table
        ctx = BL.make_ctx(bk, table, sub)
        for bias in BIASES:
            ctx.set_lod_bias(bias)
            np.testing.assert_array_equal(ctx.read_lod(), TM.derive_lod(off, sub, W, H, ps, bias), err_msg=f"{W}x{H} seed {seed} bias {bias}")
        ctx.close()


def test_drawn_stripes(bk):
    table, sub = BL.drawn_case(261, 203)
    off, tints, W, H, ps = table
    for rows in ((0, 101), (101, 102), (102, H)):
        ctx = BL.make_ctx(bk, table, sub, rows=rows)
        r0, r1 = rows
        want = TM.derive_lod(off.reshape(H, W)[r0:r1].reshape(-1), sub.reshape(H, W)[r0:r1].reshape(-1), W, r1 - r0, ps)
        np.testing.assert_array_equal(ctx.read_lod(), want, err_msg=f"rows {rows}")
        ctx.close()


@pytest.mark.parametrize("size", [(203, 131), (96, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("lens", ["hammer", "panini", "quincuncial", "winkel2"])
def test_device_builds(bk, lens, size):
    W, H = size
    ctx = bk.Context()
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", lens, None, size)
    for rows in STRIPES:
        if rows:
            rows = (rows[0] * H // 131, max(rows[1] * H // 131, rows[0] * H // 131 + 1))
            ctx.set_rows(*rows)
        ctx.build()
        for bias in BIASES if rows is None else (0,):
            ctx.set_lod_bias(bias)
            got, want = ctx.read_lod(), expect(ctx, bias)
            np.testing.assert_array_equal(got, want, err_msg=f"{lens} {size} rows {rows} bias {bias}")
            if rows is None and bias == 0:
                off, _ = ctx.read_lensmap()
                # (a plane, not a constant; a forward map's steps are whole texels, rho a multiple of 256: a handful of values)
                assert (got[off == NULL] == 0).all() and len(np.unique(got)) > (3 if lens == "winkel2" else 50)
    ctx.close()


def test_life_cycle(bk):
    """derived again after each event that changes what it is made from; a set plane kept across applies and dropped by each of them"""
    import torch
    W, H = 203, 131
    ctx = bk.Context()
    ctx.set_stream(FB._stream())
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", "hammer", None, (W, H))
    ctx.build()
    ps = min(W, H)
    plates = FB.texels(ps, 70)
    dev, ptrs, pitches = FB.source(plates)
    dst = torch.zeros(H * (W + 1) * 4, dtype=torch.uint8, device="cuda")      # (the resize below makes the frame a pixel wider)
    top = (len(TM.level_sizes(ps)) - 1) * 256

    def apply():
        ctx.apply_rgba_fb_trilinear_device(ptrs, pitches, dst.data_ptr(), 4 * (W + 1))
        torch.cuda.synchronize()

    def hand():
        w, h, _, r0, r1 = ctx.size()
        return ((np.arange((r1 - r0) * w) * 37) % (top + 1)).astype(np.uint16)

    def rebuild():
        ctx.build()

    def set_lensmap():
        off, tints = ctx.read_lensmap()
        off = off.copy()
        off[::7] = NULL
        ctx.set_lensmap(off, tints)                                    # (the plane is all centres now)

    def set_sub():
        sub = ctx.read_subtexel()
        ctx.set_lensmap_subtexel(sub ^ np.uint16(0x0101))

    def set_rows():
        ctx.set_rows(20, 91)
        ctx.build()

    def resize():
        ctx.resize(W, H)                                               # the same size: nothing changes, the stripe stays
        np.testing.assert_array_equal(ctx.read_lod(), hand())
        ctx.resize(W + 1, H)
        ctx.build()

    def bias():
        ctx.set_lod_bias(40)
        ctx.set_lod_bias(40)

    first = ctx.read_lod()
    np.testing.assert_array_equal(first, expect(ctx))
    for event in (rebuild, set_lensmap, set_sub, set_rows, resize, bias):
        mine = hand()
        ctx.set_lensmap_lod(mine)
        apply()
        apply()
        np.testing.assert_array_equal(ctx.read_lod(), mine, err_msg=f"before {event.__name__}: a set plane holds across applies")
        ctx.set_lod_bias(0)                                            # (the bias it has: nothing is dropped)
        ctx.set_subtexel(True)                                         # (the switch as it stands: nothing is dropped either)
        np.testing.assert_array_equal(ctx.read_lod(), mine)
        event()
        want = expect(ctx, 40 if event is bias else 0)
        assert not np.array_equal(want, hand())
        np.testing.assert_array_equal(ctx.read_lod(), want, err_msg=f"after {event.__name__}: derived again")
        apply()
        np.testing.assert_array_equal(ctx.read_lod(), want)
        ctx.set_lod_bias(0)
    ctx.close()


def test_errors(bk):
    table, sub = BL.drawn_case(131, 15)
    off, tints, W, H, ps = table
    top = (len(TM.level_sizes(ps)) - 1) * 256
    ctx = bk.Context()
    ctx.resize(W, H)
    ctx.set_stream(FB._stream())
    good = np.zeros(W * H, np.uint16)
    for call in (ctx.read_lod, lambda: ctx.set_lensmap_lod(good)):
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
            call()
    FB.set_table(ctx, table)                                           # the switch is off: a lensmap, no sub-texel plane
    for call in (ctx.read_lod, lambda: ctx.set_lensmap_lod(good)):
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
            call()
    ctx.set_subtexel(True)
    BL.set_table(ctx, table, sub)
    ctx.set_lensmap_lod(np.full(W * H, top, np.uint16))
    with pytest.raises(bk.BlinkyError, match=r"\[-1\].*above"):
        ctx.set_lensmap_lod(np.where(np.arange(W * H) == 77, top + 1, 0).astype(np.uint16))
    np.testing.assert_array_equal(ctx.read_lod(), top)                 # (the refused plane replaced nothing)
    lib, h = bk.ffi.lib, ctx._h
    assert lib.bk_read_lod(h, None) == -1 and lib.bk_set_lensmap_lod(h, None) == -1 and lib.bk_read_lod(None, None) == -1
    assert lib.bk_set_lod_bias(None, 0) == -1
    ctx.set_subtexel(False)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*sub-texel plane"):
        ctx.read_lod()
    ctx.close()
    none = bk.Context(bk.ffi.DEVICE_NONE)
    none.resize(W, H)
    for call in (none.read_lod, lambda: none.set_lensmap_lod(good)):
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
            call()
    none.close()
