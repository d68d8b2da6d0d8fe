"""The TRUECOLOUR apply (bk_upload_plate_rgba / bk_upload_plate_rgba_device / bk_apply_rgba_device): 32-bit plates warped into
32-bit frames.  A truecolour globe is four byte planes in four consecutive ring slots, so the expected value needs no oracle code of
its own: byte c of the truecolour result must equal the oracle's 8-bit render_lensmap (O.apply, fisheye.c:2406-2424) of byte
plane c.  Every comparison is exact equality."""
import json
import os

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = {(r["globe"], r["lens"], r["zoom"], r["W"], r["H"]): r
        for r in json.load(open(os.path.join(HERE, "golden", "lensmaps.json")))["lensmaps"]}


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
    """truecolour globe g through the host upload: texel = the four planes' bytes interleaved"""
    for p in range(6):
        ctx.upload_plate_rgba(g, p, np.stack([planes[c][p] for c in range(4)], axis=-1))


def background(nbytes_rows, pitch):
    return (np.arange(nbytes_rows * pitch, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(nbytes_rows, pitch)


def expect(off, W, H, planes, bg, x0, y0):
    """the oracle's 8-bit apply of every byte plane into the byte planes of the 32-bit frame `bg` [rows][pitch bytes]"""
    want = bg.copy()
    px_pitch = bg.shape[1] // 4
    for c in range(4):
        plane = np.ascontiguousarray(want[:, c::4])
        O.apply(off, None, W, H, planes[c], plane, px_pitch, x0, y0)
        want[:, c::4] = plane
    return want


def run(ctx, bg, pitch, globe0=0, nframes=1, x0=0, y0=0, frame_stride=None):
    """bg: uint8 [nframes][rows][pitch] -> the same after bk_apply_rgba_device"""
    import torch
    out = torch.from_numpy(np.ascontiguousarray(bg)).cuda()
    stride = out.shape[-2] * out.shape[-1] if frame_stride is None else frame_stride
    ctx.apply_rgba_device(out.data_ptr(), pitch, stride, globe0=globe0, nframes=nframes, x0=x0, y0=y0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. upload layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [131, 203])
@pytest.mark.parametrize("path", ["host", "device", "device-odd-pitch"])
def test_upload_puts_byte_c_into_slot_4g_plus_c(bk, ps, path):
    import torch
    ctx = make_ctx(bk, ps + 69, ps, 8)
    rng = np.random.default_rng(ps)
    pitch = 4 * ps + (21 if path == "device-odd-pitch" else 20)      # rows wider than the plate (not a multiple of 16 / not even of 4)
    src = rng.integers(0, 256, (2, 6, ps, pitch), dtype=np.uint8)
    for g in range(2):
        for p in range(6):
            if path == "host":
                ctx.upload_plate_rgba(g, p, src[g, p], pitch=pitch)
            else:
                dev = torch.from_numpy(src[g, p]).cuda()
                ctx.upload_plate_rgba_device(g, p, dev.data_ptr(), pitch)
                ctx.synchronize()
    for g in range(2):
        for p in range(6):
            texels = src[g, p, :, :4 * ps].reshape(ps, ps, 4)
            for c in range(4):
                np.testing.assert_array_equal(ctx.download_plate(4 * g + c, p), texels[:, :, c], err_msg=f"globe {g} plate {p} byte {c}")
    ctx.close()


# ---- 2. parity against the oracle, per byte plane -------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [
    ("cube", "panini", None, 640, 480),
    ("cube", "hammer", None, 960, 540),
    ("cube", "quincuncial", None, 640, 480),
    ("trism", "panini", None, 960, 540),
    ("cube", "panini", "f_fov 120", 322, 203),
    ("cube", "stereographic", "f_vfov 90", 300, 500),
    ("cube", "eckert5", None, 640, 480),
])
def test_apply_rgba_matches_oracle_per_plane(bk, cfg):
    lm = O.lensmap(*cfg)
    W, H = lm.W, lm.H
    planes = planes_of(lm.ps, 0, seed=3)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * (W + 24)
    bg = background(H + 7, pitch)
    for shape in (1, 2, 4):                                # all three block heights
        ctx.set_tile_shape(shape)
        for x0, y0 in ((4, 3), (5, 3)):                    # 16-byte aligned pixels (whole-lane stores where W % 4 == 0) / not
            want = expect(lm.offsets, W, H, planes, bg, x0, y0)
            got = run(ctx, bg[None], pitch, x0=x0, y0=y0)[0]
            np.testing.assert_array_equal(got, want, err_msg=f"{cfg} block height {8 * shape} origin ({x0},{y0})")
    ctx.close()


# ---- 3. batch and ring wrap ------------------------------------------------------------------------------------------
def test_batch_wraps_the_ring_of_truecolour_globes(bk):
    lm = O.lensmap("cube", "hammer", None, 960, 540)
    W, H, G, F = lm.W, lm.H, 3, 5
    ctx = make_ctx(bk, W, H, 4 * G)
    planes = [planes_of(lm.ps, g) for g in range(G)]
    for g in range(G):
        upload_planes(ctx, g, planes[g])
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * W
    # frames back to back / a frame_stride larger than the frame / one that is a multiple of 4 but not of 16 (no wide stores in any frame)
    for extra in (0, 3 * pitch + 16, 3 * pitch + 4):
        stride = H * pitch + extra
        flat = np.full(F * stride, 9, np.uint8)
        import torch
        out = torch.from_numpy(flat).cuda()
        ctx.apply_rgba_device(out.data_ptr(), pitch, stride, globe0=2, nframes=F)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for f in range(F):
            want = expect(lm.offsets, W, H, planes[(2 + f) % G], np.full((H, pitch), 9, np.uint8), 0, 0)
            np.testing.assert_array_equal(got[f * stride:f * stride + H * pitch].reshape(H, pitch), want, err_msg=f"frame {f} extra {extra}")
            assert (got[f * stride + H * pitch:(f + 1) * stride] == 9).all(), "bytes between the frames were written"
    ctx.close()


# ---- 4. scrambled tables: direct-gather blocks -----------------------------------------------------------------------
def test_scrambled_tables_and_blocks_without_staging(bk):
    """a table no lens produces, (a) with every block staged (lists above 1024 chunks: the extra rounds), (b) with the staging
    buffer forced so small that every list exceeds it; and (c) a table whose 128x32 blocks read 4096 different chunks each: blocks
    that have no chunk list at all"""
    rng = np.random.default_rng(77)
    W, H, ps = 517, 301, 301
    n = W * H
    off = rng.integers(0, 6 * ps * ps, n, dtype=np.uint32)
    off[rng.random(n) < 0.07] = O.NULL
    planes = planes_of(ps, 0, seed=11)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, None)
    pitch = 4 * (W + 3)
    bg = background(H + 4, pitch)
    want = expect(off, W, H, planes, bg, 2, 1)
    for shape, ldskb, direct in ((4, 64, False), (2, 1, True), (1, 4, True), (0, 0, False)):
        ctx.set_tile_shape(shape)
        ctx.set_tile_shape(400 + ldskb)
        st = ctx.tile_stats()
        if direct:
            assert st["slow"] > 0, st                      # lists larger than the buffer: gathered straight from the lensmap
        got = run(ctx, bg[None], pitch, x0=2, y0=1)[0]
        np.testing.assert_array_equal(got, want, err_msg=f"shape {shape} lds {ldskb} KiB {st}")
    ctx.close()
    # (c) pixel i reads chunk i: the fully mapped right half's 128x32 blocks have 4096 unique chunks (> 4095: no list), the left half has NULLs
    W = H = ps = 512
    n = W * H
    off = ((np.arange(n, dtype=np.uint64) * 16) % (6 * ps * ps)).astype(np.uint32)
    holes = (rng.random(n) < 0.07) & (np.arange(n) % W < 256)
    off[holes] = O.NULL
    planes = planes_of(ps, 0, seed=5)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, None)
    ctx.set_tile_shape(4)
    ctx.set_tile_shape(464)                                # 64 KiB: every list that exists fits, so "slow" counts the blocks without one
    st = ctx.tile_stats()
    assert st["slow"] > 0, st
    pitch = 4 * W
    bg = background(H, pitch)
    got = run(ctx, bg[None], pitch)[0]
    np.testing.assert_array_equal(got, expect(off, W, H, planes, bg, 0, 0), err_msg=str(st))
    ctx.close()


# ---- 5. stripes -------------------------------------------------------------------------------------------------------
def test_stripe_contexts_write_their_rows_only_and_concatenate(bk):
    lm = O.lensmap("trism", "panini", None, 960, 540)
    W, H = lm.W, lm.H
    planes = planes_of(lm.ps, 0, seed=1)
    pitch = 4 * W
    bg = background(H, pitch)
    want = expect(lm.offsets, W, H, planes, bg, 0, 0)
    frame = bg.copy()
    for r0, r1 in ((0, 101), (101, H)):                    # r0 = 101: not a multiple of 8
        ctx = make_ctx(bk, W, H, 4, rows=(r0, r1))
        upload_planes(ctx, 0, planes)
        ctx.set_lensmap(lm.offsets.reshape(H, W)[r0:r1], lm.tints.reshape(H, W)[r0:r1])
        before = frame.copy()
        frame = run(ctx, frame[None], pitch)[0]
        assert np.array_equal(frame[:r0], before[:r0]) and np.array_equal(frame[r1:], before[r1:]), f"rows outside [{r0},{r1}) changed"
        np.testing.assert_array_equal(frame[r0:r1], want[r0:r1])
        ctx.close()
    np.testing.assert_array_equal(frame, want)


# ---- 6. full size, pinned to the reference's goldens ---------------------------------------------------------------------
def test_4k_truecolour_batch_equals_reference_golden_frames(bk):
    """3840x2160 cube/panini built from the scripts, the 64 ring slots filled as test_batch_launch_equals_reference_golden_frames fills
    them: slot s is at once 8-bit globe s and byte plane s % 4 of truecolour globe s // 4, so byte c of truecolour frame f must hash
    to the golden of 8-bit frame 4f + c (frame 0 recorded from the unmodified reference, the others from the oracle's gather)."""
    import torch
    import scripts as S
    key = ("cube", "panini", None, 3840, 2160)
    rec = GOLD[key]
    globe, lens, zoom, W, H = key
    F = len(rec["fnv_frames"])
    assert F == 64
    ctx = bk.Context()
    ctx.set_stream(_stream())
    ctx.set_frames(F)
    S.configure(ctx, globe, lens, zoom, (W, H))
    ctx.build()
    off, tin = ctx.read_lensmap()
    assert O.fnv(off) == rec["fnv_offsets"]
    del off, tin
    for f in range(F):
        for p in range(len(rec["display"])):
            ctx.fill_plate_lcg(f, p, seed_frame=f)
    out = torch.zeros((F // 4, H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_device(out.data_ptr(), 4 * W, 4 * W * H, globe0=0, nframes=F // 4)
    torch.cuda.synchronize()
    for f in range(F // 4):
        frame = out[f].cpu().numpy()
        for c in range(4):
            assert O.fnv(frame[:, :, c]) == rec["fnv_frames"][4 * f + c], f"frame {f} byte {c}"
    ctx.close()


# ---- 7. the 8-bit path is undisturbed ------------------------------------------------------------------------------------
def test_8bit_apply_is_the_same_before_and_after_a_truecolour_launch(bk):
    import torch
    lm = O.lensmap("cube", "panini", None, 640, 480)
    W, H = lm.W, lm.H
    planes = planes_of(lm.ps, 0, seed=2)                   # slot c = 8-bit globe c
    pal = O.palmap(O.synthetic_basepal())
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)

    def eight_bit(when):
        for rubix in (False, True):
            for slot in (0, 3):
                want = O.apply(lm.offsets, lm.tints, W, H, planes[slot], np.full((H, W), 5, np.uint8), W, 0, 0, rubix, pal)
                got = ctx.apply(np.full((H, W), 5, np.uint8), slot, rubix_on=rubix, pal=pal)
                np.testing.assert_array_equal(got, want, err_msg=f"bk_apply {when}, rubix {rubix}, slot {slot}")
            out = torch.full((4, H, W), 5, dtype=torch.uint8, device="cuda")
            ctx.apply_device(out.data_ptr(), W, H * W, frame0=1, nframes=4, rubix_on=rubix, pal=pal)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for f in range(4):
                want = O.apply(lm.offsets, lm.tints, W, H, planes[(1 + f) % 4], np.full((H, W), 5, np.uint8), W, 0, 0, rubix, pal)
                np.testing.assert_array_equal(got[f], want, err_msg=f"bk_apply_device {when}, rubix {rubix}, frame {f}")

    eight_bit("before")
    bg = background(H, 4 * W)
    want = expect(lm.offsets, W, H, planes, bg, 0, 0)
    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W)[0], want)
    eight_bit("after")
    np.testing.assert_array_equal(run(ctx, bg[None], 4 * W)[0], want)      # ... and after a rubix launch has switched the block map's flavour
    ctx.close()


# ---- 8. errors --------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import torch
    W, H = 64, 48
    lm = O.lensmap("cube", "panini", None, W, H)
    out = torch.zeros((H, W + 8, 4), dtype=torch.uint8, device="cuda")
    p, pitch, stride = out.data_ptr(), 4 * (W + 8), 4 * (W + 8) * H
    ctx = make_ctx(bk, W, H, 4)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.apply_rgba_device(p, pitch, stride)
    ctx.set_lensmap(lm.offsets, lm.tints)
    ctx.apply_rgba_device(p, pitch, stride, x0=8)                                 # the widest origin the pitch allows
    for kw in (dict(pitch=4 * W - 4), dict(x0=9), dict(x0=-1), dict(y0=-1), dict(globe0=-1), dict(nframes=0),
               dict(pitch=pitch + 2), dict(stride=stride + 1), dict(ptr=p + 2)):
        a = dict(ptr=p, pitch=pitch, stride=stride, globe0=0, nframes=1, x0=0, y0=0)
        a.update(kw)
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.apply_rgba_device(a["ptr"], a["pitch"], a["stride"], globe0=a["globe0"], nframes=a["nframes"], x0=a["x0"], y0=a["y0"])
    ctx.set_apply_variant(0)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*staged variant"):
        ctx.apply_rgba_device(p, pitch, stride)
    ctx.set_apply_variant(2)
    # the uploads: globe, plate, pitch
    src = np.zeros((48, 48, 4), np.uint8)
    dev = torch.zeros((48, 48, 4), dtype=torch.uint8, device="cuda")
    for g, pl, pt in ((1, 0, 192), (-1, 0, 192), (0, 6, 192), (0, -1, 192), (0, 0, 188)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.upload_plate_rgba(g, pl, src, pitch=pt)
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.upload_plate_rgba_device(g, pl, dev.data_ptr(), pt)
    ctx.upload_plate_rgba(0, 5, src)
    ctx.close()
    ctx = make_ctx(bk, W, H, 3)                                                   # fewer than four ring slots: no truecolour globe
    ctx.set_lensmap(lm.offsets, lm.tints)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*four ring slots"):
        ctx.apply_rgba_device(p, pitch, stride)
    ctx.close()
    torch.cuda.synchronize()
