"""Rubix on truecolour frames (bk_apply_rgba_tinted_device): byte c of a mapped pixel whose tint t is below 6 leaves as lut[c][t][v].
A truecolour globe is four byte planes in four consecutive ring slots and a tint is a byte -> byte table per (byte plane, plate), so
the expected value needs no oracle code of its own: byte c of the result must equal the oracle's 8-bit RUBIX render_lensmap (O.apply
with rubix_on, fisheye.c:2406-2424) of byte plane c with pal = lut[c].  Every comparison is exact equality.

The tests bite: with plane 0's LUT requested for every plane in the staging pass (a value-only mutant, never committed) every test
here but test_errors fails (profiles/rgba_tint_apply.txt (4))."""
import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def make_ctx(bk, W, H, slots, rows=None):
    ctx = bk.Context()
    ctx.set_frames(slots)
    ctx.resize(W, H)
    if rows:
        ctx.set_rows(*rows)
    ctx.set_stream(_stream())
    return ctx


def planes_of(ps, g, seed=0):
    """the four byte planes of truecolour globe g: four different LCG globes, uint8 [4][6][ps][ps]"""
    return [O.lcg_globe(ps, 6, seed + 4 * g + c) for c in range(4)]


def upload_planes(ctx, g, planes):
    for p in range(6):
        ctx.upload_plate_rgba(g, p, np.stack([planes[c][p] for c in range(4)], axis=-1))


def background(nbytes_rows, pitch):
    return (np.arange(nbytes_rows * pitch, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(nbytes_rows, pitch)


def random_luts(seed):
    """uint8 [4][6][256]: every row differs from every other, so a swapped plane, plate or class shows"""
    lut = np.random.default_rng(seed).integers(0, 256, (4, 6, 256)).astype(np.uint8)
    rows = lut.reshape(24, 256)
    assert len({r.tobytes() for r in rows}) == 24 and not any(np.array_equal(r, np.arange(256)) for r in rows)
    return lut


def expect(off, tints, W, H, planes, bg, x0, y0, lut=None):
    """the oracle's 8-bit apply of every byte plane into the byte planes of the 32-bit frame `bg` [rows][pitch bytes]; with `lut` the
    RUBIX apply of plane c through pal = lut[c]"""
    want = bg.copy()
    px_pitch = bg.shape[1] // 4
    for c in range(4):
        plane = np.ascontiguousarray(want[:, c::4])
        if lut is None:
            O.apply(off, None, W, H, planes[c], plane, px_pitch, x0, y0)
        else:
            O.apply(off, tints, W, H, planes[c], plane, px_pitch, x0, y0, True, lut[c])
        want[:, c::4] = plane
    return want


def run(ctx, bg, pitch, lut, globe0=0, nframes=1, x0=0, y0=0, frame_stride=None):
    """bg: uint8 [nframes][rows][pitch] -> the same after bk_apply_rgba_tinted_device (lut None: bk_apply_rgba_device)"""
    import torch
    out = torch.from_numpy(np.ascontiguousarray(bg)).cuda()
    stride = out.shape[-2] * out.shape[-1] if frame_stride is None else frame_stride
    if lut is None:
        ctx.apply_rgba_device(out.data_ptr(), pitch, stride, globe0=globe0, nframes=nframes, x0=x0, y0=y0)
    else:
        ctx.apply_rgba_tinted_device(out.data_ptr(), pitch, stride, lut, globe0=globe0, nframes=nframes, x0=x0, y0=y0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def table_properties(off, tints, ps):
    """of the INPUT: the tint values of the mapped pixels, and how many 16-texel chunks (plate, py, px // 16) are read under two or
    more different tint classes (class = tint + 1 below 6, else 0: what a tinted block map lists a chunk once for)"""
    off, tints = np.asarray(off).ravel(), np.asarray(tints).ravel()
    m = off != O.NULL
    o, t = off[m].astype(np.int64), tints[m].astype(np.int64)
    cls = np.where(t < 6, t + 1, 0)
    chunk = (o // ps) * 4096 + (o % ps) // 16
    pairs = np.unique(chunk * 8 + cls)
    _, n = np.unique(pairs >> 3, return_counts=True)
    return set(int(v) for v in np.unique(t)), int((n >= 2).sum()), int(n.max())


def assert_exercises_classes(off, tints, ps, what):
    """a precondition on the table, never a filter on results: a table that stops exercising the class machinery fails loudly"""
    present, two, _ = table_properties(off, tints, ps)
    assert len([v for v in present if v < 6]) >= 3, f"{what}: tints present {present}"
    assert 255 in present, f"{what}: tints present {present}"
    assert two >= 100, f"{what}: {two} chunks read under two classes"


TABLES = [
    ("cube", "panini", None, 640, 480),
    ("cube", "hammer", None, 960, 540),                    # unmapped corners
    ("trism", "panini", None, 960, 540),
    ("cube", "panini", "f_fov 120", 322, 203),             # W not a multiple of 4
]


# ---- 1. parity against the oracle, per byte plane -------------------------------------------------------------------
@pytest.mark.parametrize("cfg", TABLES)
def test_tinted_apply_matches_oracle_per_plane(bk, cfg):
    lm = O.lensmap(*cfg)
    W, H = lm.W, lm.H
    assert_exercises_classes(lm.offsets, lm.tints, lm.ps, cfg)
    planes = planes_of(lm.ps, 0, seed=3)
    lut = random_luts(W)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * (W + 24)
    bg = background(H + 7, pitch)
    want = {o: expect(lm.offsets, lm.tints, W, H, planes, bg, *o, lut=lut) for o in ((4, 3), (5, 3))}
    assert not np.array_equal(want[(4, 3)], expect(lm.offsets, lm.tints, W, H, planes, bg, 4, 3))      # (the tints change the frame)
    for shape in (1, 2, 4):                                # all three block heights
        ctx.set_tile_shape(shape)
        for x0, y0 in ((4, 3), (5, 3)):                    # wide stores (where W % 4 == 0) / one dword per pixel
            got = run(ctx, bg[None], pitch, lut, x0=x0, y0=y0)[0]
            np.testing.assert_array_equal(got, want[(x0, y0)], err_msg=f"{cfg} block height {8 * shape} origin ({x0},{y0})")
    ctx.close()


# ---- 2. the helper's LUTs ---------------------------------------------------------------------------------------------
def test_reference_tints_for_bgra_texels(bk):
    lm = O.lensmap(*TABLES[0])
    W, H = lm.W, lm.H
    assert_exercises_classes(lm.offsets, lm.tints, lm.ps, TABLES[0])
    planes = planes_of(lm.ps, 0, seed=7)
    lut = bk.ffi.create_tintmap_rgba((2, 1, 0, 3))
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * W
    bg = background(H, pitch)
    want = expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0, lut=lut)
    got = run(ctx, bg[None], pitch, lut)[0]
    np.testing.assert_array_equal(got, want)
    mapped = (lm.offsets != O.NULL).reshape(H, W)
    plain = expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0)
    np.testing.assert_array_equal(got[:, 3::4][mapped], plain[:, 3::4][mapped])       # alpha: as it was
    ctx.close()


# ---- 3. batch and ring wrap ------------------------------------------------------------------------------------------
def test_tinted_batch_wraps_the_ring_of_truecolour_globes(bk):
    import torch
    lm = O.lensmap("cube", "hammer", None, 960, 540)
    W, H, G, F = lm.W, lm.H, 3, 5
    assert_exercises_classes(lm.offsets, lm.tints, lm.ps, "cube/hammer")
    ctx = make_ctx(bk, W, H, 4 * G)
    planes = [planes_of(lm.ps, g) for g in range(G)]
    for g in range(G):
        upload_planes(ctx, g, planes[g])
    ctx.set_lensmap(lm.offsets, lm.tints)
    lut = random_luts(3)
    pitch = 4 * W
    want = [expect(lm.offsets, lm.tints, W, H, planes[g], np.full((H, pitch), 9, np.uint8), 0, 0, lut=lut) for g in range(G)]
    # frames back to back / a frame_stride larger than the frame / one that is a multiple of 4 but not of 16 (no wide stores in any frame)
    for extra in (0, 3 * pitch + 16, 3 * pitch + 4):
        stride = H * pitch + extra
        out = torch.from_numpy(np.full(F * stride, 9, np.uint8)).cuda()
        ctx.apply_rgba_tinted_device(out.data_ptr(), pitch, stride, lut, globe0=2, nframes=F)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for f in range(F):
            np.testing.assert_array_equal(got[f * stride:f * stride + H * pitch].reshape(H, pitch), want[(2 + f) % G], err_msg=f"frame {f} extra {extra}")
            assert (got[f * stride + H * pitch:(f + 1) * stride] == 9).all(), "bytes between the frames were written"
    ctx.close()


# ---- 4. hand-set tint planes: up to seven classes per chunk, blocks without staging ----------------------------------------
def test_hand_set_tints_and_blocks_without_staging(bk):
    """a table no lens produces, its tints drawn from {0..5, 255} pixel by pixel: (a) every block staged (lists above 1024 chunks: the
    extra rounds), (b) the staging buffer forced so small that every list exceeds it; and (c) a table whose 128x32 blocks read 4096
    different chunks each: blocks that have no chunk list at all"""
    rng = np.random.default_rng(77)
    values = np.array([0, 1, 2, 3, 4, 5, 255], np.uint8)
    W, H, ps = 517, 301, 301
    n = W * H
    off = rng.integers(0, 6 * ps * ps, n, dtype=np.uint32)
    off[rng.random(n) < 0.07] = O.NULL
    tints = values[rng.integers(0, 7, n)]
    present, two, most = table_properties(off, tints, ps)
    assert present == set(int(v) for v in values) and two >= 100 and most > 2, (present, two, most)     # (lens tables never exceed two)
    planes = planes_of(ps, 0, seed=11)
    lut = random_luts(4)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, tints)
    pitch = 4 * (W + 3)
    bg = background(H + 4, pitch)
    want = expect(off, tints, W, H, planes, bg, 2, 1, lut=lut)
    for shape, ldskb, direct in ((4, 64, False), (2, 1, True), (1, 4, True), (0, 0, False)):
        ctx.set_tile_shape(shape)
        ctx.set_tile_shape(400 + ldskb)
        got = run(ctx, bg[None], pitch, lut, x0=2, y0=1)[0]
        st = ctx.tile_stats()                              # (of the tinted block map: the launch above made it the current one)
        if direct:
            assert st["slow"] > 0, st                      # lists larger than the buffer: gathered straight from the lensmap
        np.testing.assert_array_equal(got, want, err_msg=f"shape {shape} lds {ldskb} KiB {st}")
    ctx.close()
    # (c) pixel i reads chunk i: the fully mapped right half's 128x32 blocks have 4096 unique chunks (> 4095: no list), the left half has NULLs
    W = H = ps = 512
    n = W * H
    off = ((np.arange(n, dtype=np.uint64) * 16) % (6 * ps * ps)).astype(np.uint32)
    holes = (rng.random(n) < 0.07) & (np.arange(n) % W < 256)
    off[holes] = O.NULL
    tints = values[rng.integers(0, 7, n)]
    planes = planes_of(ps, 0, seed=5)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, tints)
    ctx.set_tile_shape(4)
    ctx.set_tile_shape(464)                                # 64 KiB: every list that exists fits, so "slow" counts the blocks without one
    pitch = 4 * W
    bg = background(H, pitch)
    got = run(ctx, bg[None], pitch, lut)[0]
    st = ctx.tile_stats()
    assert st["slow"] > 0, st
    np.testing.assert_array_equal(got, expect(off, tints, W, H, planes, bg, 0, 0, lut=lut), err_msg=str(st))
    ctx.close()


# ---- 5. stripes -------------------------------------------------------------------------------------------------------
def test_tinted_stripe_contexts_write_their_rows_only_and_concatenate(bk):
    lm = O.lensmap("trism", "panini", None, 960, 540)
    W, H = lm.W, lm.H
    assert_exercises_classes(lm.offsets, lm.tints, lm.ps, "trism/panini")
    planes = planes_of(lm.ps, 0, seed=1)
    lut = random_luts(5)
    pitch = 4 * W
    bg = background(H, pitch)
    want = expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0, lut=lut)
    frame = bg.copy()
    for r0, r1 in ((0, 101), (101, H)):                    # r0 = 101: not a multiple of 8
        ctx = make_ctx(bk, W, H, 4, rows=(r0, r1))
        upload_planes(ctx, 0, planes)
        ctx.set_lensmap(lm.offsets.reshape(H, W)[r0:r1], lm.tints.reshape(H, W)[r0:r1])
        before = frame.copy()
        frame = run(ctx, frame[None], pitch, lut)[0]
        assert np.array_equal(frame[:r0], before[:r0]) and np.array_equal(frame[r1:], before[r1:]), f"rows outside [{r0},{r1}) changed"
        np.testing.assert_array_equal(frame[r0:r1], want[r0:r1])
        ctx.close()
    np.testing.assert_array_equal(frame, want)


# ---- 6. flavour switching on one context ----------------------------------------------------------------------------------
def test_flavours_alternate_on_one_context(bk):
    """plain truecolour, tinted truecolour, the 8-bit applies with and without rubix through a palette of their own, tinted truecolour
    through OTHER tables, plain truecolour: the two kept block maps, the LUT cache and the 8-bit palette cache each stay what they were"""
    import torch
    lm = O.lensmap(*TABLES[0])
    W, H = lm.W, lm.H
    assert_exercises_classes(lm.offsets, lm.tints, lm.ps, TABLES[0])
    planes = planes_of(lm.ps, 0, seed=2)                   # slot c = 8-bit globe c
    pal = O.palmap(O.synthetic_basepal())
    lut_a, lut_b = random_luts(6), random_luts(7)
    for lut in (lut_a, lut_b):
        assert not any(np.array_equal(lut[c], pal) for c in range(4))
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    bg = background(H, 4 * W)
    want_plain = expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0)
    want8 = {(rubix, slot): O.apply(lm.offsets, lm.tints, W, H, planes[slot], np.full((H, W), 5, np.uint8), W, 0, 0, rubix, pal)
             for rubix in (False, True) for slot in range(4)}

    def eight_bit():
        for rubix in (False, True):
            for slot in (0, 3):
                got = ctx.apply(np.full((H, W), 5, np.uint8), slot, rubix_on=rubix, pal=pal)
                np.testing.assert_array_equal(got, want8[(rubix, slot)], err_msg=f"bk_apply, rubix {rubix}, slot {slot}")
            out = torch.full((4, H, W), 5, dtype=torch.uint8, device="cuda")
            ctx.apply_device(out.data_ptr(), W, H * W, frame0=1, nframes=4, rubix_on=rubix, pal=pal)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for f in range(4):
                np.testing.assert_array_equal(got[f], want8[(rubix, (1 + f) % 4)], err_msg=f"bk_apply_device, rubix {rubix}, frame {f}")

    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W, None)[0], want_plain, err_msg="plain, first")
    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W, lut_a)[0], expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0, lut=lut_a), err_msg="tinted, first tables")
    eight_bit()
    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W, lut_b)[0], expect(lm.offsets, lm.tints, W, H, planes, bg, 0, 0, lut=lut_b), err_msg="tinted, other tables")
    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W, None)[0], want_plain, err_msg="plain, last")
    ctx.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import torch
    W, H = 64, 48
    lm = O.lensmap("cube", "panini", None, W, H)
    lut = random_luts(8)
    out = torch.zeros((H, W + 8, 4), dtype=torch.uint8, device="cuda")
    p, pitch, stride = out.data_ptr(), 4 * (W + 8), 4 * (W + 8) * H
    ctx = make_ctx(bk, W, H, 4)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.apply_rgba_tinted_device(p, pitch, stride, lut)
    ctx.set_lensmap(lm.offsets, lm.tints)
    ctx.apply_rgba_tinted_device(p, pitch, stride, lut, x0=8)                     # the widest origin the pitch allows
    for kw in (dict(pitch=4 * W - 4), dict(x0=9), dict(x0=-1), dict(y0=-1), dict(globe0=-1), dict(nframes=0),
               dict(pitch=pitch + 2), dict(stride=stride + 1), dict(ptr=p + 2), dict(lut=None)):
        a = dict(ptr=p, pitch=pitch, stride=stride, globe0=0, nframes=1, x0=0, y0=0, lut=lut)
        a.update(kw)
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.apply_rgba_tinted_device(a["ptr"], a["pitch"], a["stride"], a["lut"], globe0=a["globe0"], nframes=a["nframes"], x0=a["x0"], y0=a["y0"])
    ctx.set_apply_variant(0)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*staged variant"):
        ctx.apply_rgba_tinted_device(p, pitch, stride, lut)
    ctx.set_apply_variant(2)
    ctx.close()
    ctx = make_ctx(bk, W, H, 3)                                                   # fewer than four ring slots: no truecolour globe
    ctx.set_lensmap(lm.offsets, lm.tints)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*four ring slots"):
        ctx.apply_rgba_tinted_device(p, pitch, stride, lut)
    ctx.close()
    torch.cuda.synchronize()
