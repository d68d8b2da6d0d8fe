"""The lensmap's FOOTPRINT on the GPU: bk_plate_footprint against the numpy model (tests/footprint_model.py, itself held to a second
formulation and to the oracle by tests/test_footprint_model_cpu.py), and bk_upload_plate_rgba_footprint / _device: they write the
footprint's tiles and nothing else, and every truecolour apply produces from a globe uploaded that way - over sentinels - exactly what
it produces after a full upload.  Lensmaps come from the CPU oracle through bk_set_lensmap unless a test says otherwise.  Every
comparison is exact equality."""
import numpy as np
import pytest

import footprint_model as FM
import oracle_ffi as O

pytestmark = pytest.mark.gpu

_LM = {}


def lensmap(cfg):
    """the oracle's lensmap of a configuration, computed once for the module and never changed"""
    if cfg not in _LM:
        _LM[cfg] = O.lensmap(*cfg)
        _LM[cfg].offsets.flags.writeable = False
    return _LM[cfg]


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def make_ctx(bk, W, H, slots=1, rows=None):
    ctx = bk.Context()
    ctx.set_frames(slots)
    ctx.resize(W, H)
    if rows:
        ctx.set_rows(*rows)
    ctx.set_stream(_stream())
    return ctx


def set_table(ctx, off, W, H, rows=None):
    r0, r1 = rows if rows else (0, H)
    ctx.set_lensmap(np.asarray(off).reshape(H, W)[r0:r1])


def check_query(ctx, off, W, H, ps, rows=None, what=""):
    masks, counts, rects = FM.footprint(off, W, H, ps, rows)
    for p in range(6):
        rect, n, mask = ctx.plate_footprint(p, tiles=True)
        assert n == counts[p], f"{what} plate {p}: {n} tiles, the model has {counts[p]}"
        assert rect == rects[p], f"{what} plate {p}: rect {rect}, the model has {rects[p]}"
        np.testing.assert_array_equal(mask, masks[p], err_msg=f"{what} plate {p}")
        assert ctx.plate_footprint(p) == (rect, n)
    return masks, counts, rects


def one_pixel_per_plate():
    off = np.full(17 * 17, O.NULL, np.uint32)
    for p in range(6):
        off[20 * p + 3] = p * 289 + (16 - p) * 17 + (p * 3 + 1)
    return off


# ---- 1. the query ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(FM.PARTIAL) + [FM.FULL, ("trism", "panini", None, 960, 540)])
def test_query_equals_model(bk, cfg):
    lm = lensmap(cfg)
    ctx = make_ctx(bk, lm.W, lm.H)
    set_table(ctx, lm.offsets, lm.W, lm.H)
    _, counts, _ = check_query(ctx, lm.offsets, lm.W, lm.H, lm.ps, what=str(cfg))
    if cfg in FM.PARTIAL:
        assert counts == FM.PARTIAL[cfg]
    ctx.close()


def test_query_on_small_and_empty_tables(bk):
    ctx = make_ctx(bk, 17, 17)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.plate_footprint(0)
    off = one_pixel_per_plate()
    set_table(ctx, off, 17, 17)
    _, counts, _ = check_query(ctx, off, 17, 17, 17, what="one pixel per plate")
    assert counts == [1] * 6
    off = np.full(17 * 17, O.NULL, np.uint32)
    set_table(ctx, off, 17, 17)
    _, counts, rects = check_query(ctx, off, 17, 17, 17, what="all NULL")
    assert counts == [0] * 6 and rects == [(0, 0, 0, 0)] * 6
    with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
        ctx.plate_footprint(6)
    with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
        ctx.plate_footprint(-1)
    ctx.close()


def test_query_after_a_real_build_agrees_with_display(bk):
    import scripts as S
    cfg = ("cube", "panini", "f_fov 120", 322, 203)
    ctx = bk.Context()
    ctx.set_stream(_stream())
    S.configure(ctx, cfg[0], cfg[1], cfg[2], (cfg[3], cfg[4]))
    display, _ = ctx.build()
    off, _ = ctx.read_lensmap()
    _, counts, _ = check_query(ctx, off, 322, 203, 203, what="built")
    assert [c > 0 for c in counts] == [bool(d) for d in display]
    assert 0 < sum(bool(d) for d in display) < 6
    ctx.close()


# ---- 2. stripes -------------------------------------------------------------------------------------------------------------
def test_stripe_contexts_get_the_footprint_of_their_rows(bk):
    lm = lensmap(("cube", "panini", None, 640, 480))
    W, H, ps = lm.W, lm.H, lm.ps
    got = []
    for rows in ((0, 240), (240, 480), (96, 104)):
        ctx = make_ctx(bk, W, H, rows=rows)
        set_table(ctx, lm.offsets, W, H, rows)
        got.append(check_query(ctx, lm.offsets, W, H, ps, rows, what=f"rows {rows}")[0])
        ctx.close()
    np.testing.assert_array_equal(got[0] | got[1], FM.footprint(lm.offsets, W, H, ps)[0])
    assert 0 < got[2].sum() < got[0].sum()


# ---- 3. invalidation ----------------------------------------------------------------------------------------------------------
def test_every_lensmap_or_row_change_gives_a_new_footprint(bk):
    cfg = ("cube", "panini", "f_fov 120", 322, 203)
    lm = lensmap(cfg)
    W, H, ps = lm.W, lm.H, lm.ps
    ctx = make_ctx(bk, W, H)
    set_table(ctx, lm.offsets, W, H)
    first = check_query(ctx, lm.offsets, W, H, ps, what="golden")
    half = lm.offsets.copy().reshape(H, W)
    half[:, :W // 2] = O.NULL
    half = half.reshape(-1)
    set_table(ctx, half, W, H)                                         # bk_set_lensmap
    second = check_query(ctx, half, W, H, ps, what="left half NULL")
    assert second[1] != first[1]
    ctx.set_rows(50, 120)                                              # bk_set_rows: no lensmap, then the stripe's
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.plate_footprint(0)
    set_table(ctx, lm.offsets, W, H, (50, 120))
    third = check_query(ctx, lm.offsets, W, H, ps, (50, 120), what="rows 50..120")
    assert third[1] != first[1]
    ctx.set_rows(0, H)
    set_table(ctx, lm.offsets, W, H)
    assert check_query(ctx, lm.offsets, W, H, ps, what="whole again")[1] == first[1]
    lm2 = lensmap(("cube", "stereographic", "f_vfov 90", 300, 500))   # bk_resize: another platesize, another bitmap
    ctx.resize(lm2.W, lm2.H)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.plate_footprint(0)
    set_table(ctx, lm2.offsets, lm2.W, lm2.H)
    check_query(ctx, lm2.offsets, lm2.W, lm2.H, lm2.ps, what="resized")
    ctx.close()


# ---- 4. the upload writes the footprint and nothing else --------------------------------------------------------------------------
def patterns(ps, seed):
    """A (bytes 0..99) and B (100..199): uint8 [6][ps][ps][4] that differ in every byte; 255 is the guard no plate holds"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 100, (6, ps, ps, 4), dtype=np.uint8), rng.integers(100, 200, (6, ps, ps, 4), dtype=np.uint8)


GUARD = 255
PITCH_EXTRA = {"host": 20, "device-16": 16, "device-4": 20, "device-1": 21}


def guarded_source(texels, rect, pitch):
    """uint8 [ps][pitch]: the plate's texels inside rect, GUARD everywhere else (outside rect and right of the plate)"""
    ps = texels.shape[0]
    src = np.full((ps, pitch), GUARD, np.uint8)
    x0, y0, x1, y1 = rect
    src[y0:y1, 4 * x0:4 * x1] = texels[y0:y1, x0:x1].reshape(y1 - y0, 4 * (x1 - x0))
    return src


def footprint_upload(ctx, path, g, p, src, pitch):
    import torch
    if path == "host":
        ctx.upload_plate_rgba_footprint(g, p, src, pitch=pitch)
    else:
        dev = torch.from_numpy(src).cuda()
        ctx.upload_plate_rgba_footprint_device(g, p, dev.data_ptr(), pitch)
        ctx.synchronize()


@pytest.mark.parametrize("cfg", FM.UNTOUCHED_OUTSIDE)
@pytest.mark.parametrize("path", list(PITCH_EXTRA))
def test_footprint_upload_writes_the_footprint_and_nothing_else(bk, cfg, path):
    lm = lensmap(cfg)
    W, H, ps = lm.W, lm.H, lm.ps
    masks, counts, rects = FM.footprint(lm.offsets, W, H, ps)
    A, B = patterns(ps, ps)
    ctx = make_ctx(bk, W, H, slots=8)
    g = 1                                                              # the second truecolour globe: ring slots 4 .. 7
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.upload_plate_rgba_footprint(g, 0, B[0])
    set_table(ctx, lm.offsets, W, H)
    pitch = (4 * ps + 15) // 16 * 16 + PITCH_EXTRA[path]
    assert pitch % 16 == {"host": 4, "device-16": 0, "device-4": 4, "device-1": 5}[path]
    for p in range(6):
        ctx.upload_plate_rgba(g, p, A[p])
    for p in range(6):
        footprint_upload(ctx, path, g, p, guarded_source(B[p], rects[p], pitch), pitch)
    for p in range(6):
        inside = FM.texel_mask(masks[p], ps)
        for c in range(4):
            want = np.where(inside, B[p, :, :, c], A[p, :, :, c])
            np.testing.assert_array_equal(ctx.download_plate(4 * g + c, p), want, err_msg=f"{cfg} {path} plate {p} byte {c}")
            assert not ctx.download_plate(c, p).any(), "the other truecolour globe was written"
    # the arguments are bk_upload_plate_rgba's
    for gg, pl, pt in ((2, 0, pitch), (-1, 0, pitch), (0, 6, pitch), (0, -1, pitch), (0, 0, 4 * ps - 4)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            footprint_upload(ctx, path, gg, pl, guarded_source(B[0], rects[0], pitch), pt)
    ctx.close()


# ---- 5. frames ------------------------------------------------------------------------------------------------------------------
def luts(seed):
    lut = np.random.default_rng(seed).integers(0, 256, (4, 6, 256)).astype(np.uint8)
    assert len({r.tobytes() for r in lut.reshape(24, 256)}) == 24
    return lut


def frames(ctx, W, H, lut, nframes=2, rows_below=3, fill=77):
    """the whole destination allocations of the four truecolour applies, nframes frames from globes 0 .. nframes - 1: a pitch wider than
    the frame, an origin, rows below, a gap between the frames"""
    import torch
    out = []
    for ss2 in (False, True):
        Wd, Hd = ((W + 1) // 2, (H + 1) // 2) if ss2 else (W, H)
        pitch, x0, y0 = 4 * (Wd + 8), 4, 2
        stride = (y0 + Hd + rows_below) * pitch + 32
        for tinted in (False, True):
            dst = torch.full((nframes * stride,), fill, dtype=torch.uint8, device="cuda")
            if ss2:
                ctx.apply_rgba_ss2_device(dst.data_ptr(), pitch, stride, nframes=nframes, x0=x0, y0=y0, lut=lut if tinted else None)
            elif tinted:
                ctx.apply_rgba_tinted_device(dst.data_ptr(), pitch, stride, lut, nframes=nframes, x0=x0, y0=y0)
            else:
                ctx.apply_rgba_device(dst.data_ptr(), pitch, stride, nframes=nframes, x0=x0, y0=y0)
            torch.cuda.synchronize()
            out.append(dst.cpu().numpy())
    return out


def real_plates(ps, g):
    return np.random.default_rng(1000 + g).integers(0, 256, (6, ps, ps, 4), dtype=np.uint8)


@pytest.mark.parametrize("cfg,shapes", [(("cube", "panini", "f_fov 120", 322, 203), (1, 2, 4)), (("cube", "panini", None, 640, 480), (0,))])
def test_frames_after_a_footprint_upload_equal_frames_after_a_full_upload(bk, cfg, shapes):
    import torch
    lm = lensmap(cfg)
    W, H, ps = lm.W, lm.H, lm.ps
    ctx = make_ctx(bk, W, H, slots=8)
    ctx.set_lensmap(lm.offsets, lm.tints)
    lut = luts(5)
    plates = [real_plates(ps, g) for g in range(2)]
    for g in range(2):
        for p in range(6):
            ctx.upload_plate_rgba(g, p, plates[g][p])
    want = {}
    for shape in shapes:
        ctx.set_tile_shape(shape)
        want[shape] = frames(ctx, W, H, lut)
    assert any((w != 77).any() for w in want[shapes[0]])
    for g in range(2):                                                 # sentinels everywhere: every byte differs from the real plate's
        for p in range(6):
            ctx.upload_plate_rgba(g, p, plates[g][p] ^ 0xFF)
    assert not np.array_equal(frames(ctx, W, H, lut)[0], want[shapes[-1]][0]), "the sentinels do not show in the frame"
    for g in range(2):
        for p in range(6):
            if g == 0:
                ctx.upload_plate_rgba_footprint(g, p, plates[g][p])
            else:
                dev = torch.from_numpy(plates[g][p]).cuda()
                ctx.upload_plate_rgba_footprint_device(g, p, dev.data_ptr(), 4 * ps)
                ctx.synchronize()
    for shape in shapes:
        ctx.set_tile_shape(shape)
        for name, got, exp in zip(("plain", "tinted", "ss2", "ss2 tinted"), frames(ctx, W, H, lut), want[shape]):
            np.testing.assert_array_equal(got, exp, err_msg=f"{cfg} block height {8 * shape} {name}")
    ctx.close()


# ---- 6. two stripe contexts -----------------------------------------------------------------------------------------------------
def test_two_stripe_contexts_stitch_the_single_context_frame(bk):
    import torch
    lm = lensmap(("cube", "panini", None, 640, 480))
    W, H, ps = lm.W, lm.H, lm.ps
    plates = real_plates(ps, 0)
    lut = luts(6)
    pitch = 4 * W

    def launch(ctx, dst, tinted):
        if tinted:
            ctx.apply_rgba_tinted_device(dst.data_ptr(), pitch, H * pitch, lut)
        else:
            ctx.apply_rgba_device(dst.data_ptr(), pitch, H * pitch)
        torch.cuda.synchronize()

    ctx = make_ctx(bk, W, H, slots=4)
    ctx.set_lensmap(lm.offsets, lm.tints)
    for p in range(6):
        ctx.upload_plate_rgba(0, p, plates[p])
    want = []
    for tinted in (False, True):
        dst = torch.full((H * pitch,), 77, dtype=torch.uint8, device="cuda")
        launch(ctx, dst, tinted)
        want.append(dst.cpu().numpy())
    ctx.close()
    stitched = [torch.full((H * pitch,), 77, dtype=torch.uint8, device="cuda") for _ in range(2)]
    written = []
    for rows in ((0, 172), (172, H)):
        ctx = make_ctx(bk, W, H, slots=4, rows=rows)
        ctx.set_lensmap(lm.offsets.reshape(H, W)[rows[0]:rows[1]], lm.tints.reshape(H, W)[rows[0]:rows[1]])
        for p in range(6):
            ctx.upload_plate_rgba(0, p, plates[p] ^ 0xFF)
        for p in range(6):
            ctx.upload_plate_rgba_footprint(0, p, plates[p])
        written.append(sum(ctx.plate_footprint(p)[1] for p in range(6)))
        for tinted in (False, True):
            launch(ctx, stitched[tinted], tinted)
        ctx.close()
    whole = sum(FM.footprint(lm.offsets, W, H, ps)[1])
    assert all(0 < w < whole for w in written), (written, whole)       # each stripe re-tiles less than the whole map's footprint
    for tinted in (False, True):
        np.testing.assert_array_equal(stitched[tinted].cpu().numpy(), want[tinted], err_msg=f"tinted {tinted}")


# ---- 7. an empty footprint -------------------------------------------------------------------------------------------------------
def test_a_plate_nothing_reads_is_left_alone(bk):
    import torch
    lm = lensmap(("cube", "panini", None, 640, 480))
    W, H, ps = lm.W, lm.H, lm.ps
    assert FM.footprint(lm.offsets, W, H, ps)[1][3] == 0
    A, B = patterns(ps, 3)
    ctx = make_ctx(bk, W, H, slots=4)
    set_table(ctx, lm.offsets, W, H)
    ctx.upload_plate_rgba(0, 3, A[3])
    assert ctx.plate_footprint(3) == ((0, 0, 0, 0), 0)
    ctx.upload_plate_rgba_footprint(0, 3, B[3])
    dev = torch.from_numpy(B[3]).cuda()
    ctx.upload_plate_rgba_footprint_device(0, 3, dev.data_ptr(), 4 * ps)
    ctx.synchronize()
    for c in range(4):
        np.testing.assert_array_equal(ctx.download_plate(c, 3), A[3, :, :, c])
    ctx.close()
