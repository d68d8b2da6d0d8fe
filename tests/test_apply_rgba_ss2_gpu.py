"""2x2 supersampling fused into the truecolour apply (bk_apply_rgba_ss2_device): the context is W x H, the frames written are
(W + 1) // 2 x (H + 1) // 2, output pixel (X, Y) is the rounded mean (sum + n // 2) // n of the n samples (2X + i, 2Y + j) that lie
inside W x H and are mapped; n == 0 leaves the pixel untouched.  The expected value needs no oracle code of its own: a sample's byte c
is the oracle's 8-bit render_lensmap (O.apply, fisheye.c:2406-2424) of byte plane c - with rubix_on and lut[c] as the palette for the
tinted launch - the mapped mask is offsets != O.NULL, and the average is numpy.  Every comparison is exact equality over the WHOLE
destination allocation.

Two places where the tables differ from a literal reading of the issue that asked for this file, because that reading cannot be built:
 - the directed "every sum at every count" table is 128 wide, not 64: a fully mapped 128 x 8*RG tile - the only way to the wide stores -
   does not fit into 64 columns;
 - the stripe cut that leaves a gap is (0, 270) / (272, 540), not (0, 271) / (272, 540): 271 is an odd row1 below H, which the same
   issue makes BK_E_STATE (and the test holds it to that).
The hand-set tints of test 4 include 6 and 7, for which the oracle would read past its six plates: quad_means says what it does."""
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
    lut = np.random.default_rng(seed).integers(0, 256, (4, 6, 256)).astype(np.uint8)
    assert len({r.tobytes() for r in lut.reshape(24, 256)}) == 24
    return lut


def quad_means(off, tints, W, H, planes, lut=None):
    """-> (mean uint8 [Ho][Wo][4], n [Ho][Wo]): the oracle's samples of the full-size frame, averaged per 2x2 quad in numpy"""
    off = np.ascontiguousarray(np.asarray(off).reshape(-1), np.uint32)
    # the oracle has six plates and indexes them with any tint but 255; the library leaves texels of tints 6 .. 254 as they are
    # (blinky_hip.h), which for the oracle is tint 255 - the kernels are given the tints as they are
    oracle_tints = None if tints is None else np.where(np.asarray(tints) < 6, tints, 255).astype(np.uint8)
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    mapped = np.zeros((2 * Ho, 2 * Wo), np.int64)
    mapped[:H, :W] = (off != O.NULL).reshape(H, W)
    vals = np.zeros((2 * Ho, 2 * Wo, 4), np.int64)
    for c in range(4):
        plane = np.zeros((H, W), np.uint8)
        if lut is None:
            O.apply(off, None, W, H, planes[c], plane, W, 0, 0)
        else:
            O.apply(off, oracle_tints, W, H, planes[c], plane, W, 0, 0, True, lut[c])
        vals[:H, :W, c] = plane
    vals *= mapped[:, :, None]
    n = mapped.reshape(Ho, 2, Wo, 2).sum(axis=(1, 3))
    s = vals.reshape(Ho, 2, Wo, 2, 4).sum(axis=(1, 3))
    mean = (s + (n // 2)[:, :, None]) // np.maximum(n, 1)[:, :, None]
    assert mean.max() <= 255
    return mean.astype(np.uint8), n


def paste(bg, means, x0, y0, rows=None):
    """the quads with n > 0 of output rows `rows` (default: all) into the half-size frame `bg` [rows][pitch bytes] at pixel (x0, y0)"""
    mean, n = means
    Ho, Wo = n.shape
    r0, r1 = rows if rows else (0, Ho)
    want = bg.copy()
    view = want[y0 + r0:y0 + r1, 4 * x0:4 * (x0 + Wo)].reshape(r1 - r0, Wo, 4)
    m = n[r0:r1] > 0
    view[m] = mean[r0:r1][m]
    want[y0 + r0:y0 + r1, 4 * x0:4 * (x0 + Wo)] = view.reshape(r1 - r0, 4 * Wo)
    return want


def run(ctx, bg, pitch, lut=None, globe0=0, nframes=1, x0=0, y0=0, frame_stride=None):
    """bg: uint8 [nframes][rows][pitch] -> the same after bk_apply_rgba_ss2_device"""
    import torch
    out = torch.from_numpy(np.ascontiguousarray(bg)).cuda()
    stride = out.shape[-2] * out.shape[-1] if frame_stride is None else frame_stride
    ctx.apply_rgba_ss2_device(out.data_ptr(), pitch, stride, globe0=globe0, nframes=nframes, x0=x0, y0=y0, lut=lut)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def counts_present(n):
    return set(int(v) for v in np.unique(n))


# ---- 1. lenses, block heights, origins --------------------------------------------------------------------------------------
CONFIGS = [
    ("cube", "panini", None, 640, 480),
    ("cube", "hammer", None, 960, 540),                    # the ellipse's border: quads with 1, 2 and 3 mapped samples
    ("trism", "panini", None, 960, 540),
    ("cube", "panini", "f_fov 120", 322, 203),             # odd H; 322 = 2 mod 4: the last four-pixel group is partial
    ("cube", "eckert5", None, 640, 480),
]


@pytest.mark.parametrize("flavour", ["plain", "tintmap", "random-lut"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_ss2_matches_the_averaged_oracle(bk, cfg, flavour):
    lm = O.lensmap(*cfg)
    W, H = lm.W, lm.H
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    planes = planes_of(lm.ps, 0, seed=3)
    lut = None if flavour == "plain" else bk.ffi.create_tintmap_rgba((0, 1, 2, 3)) if flavour == "tintmap" else random_luts(W)
    means = quad_means(lm.offsets, lm.tints, W, H, planes, lut)
    if cfg[1] == "hammer":
        assert counts_present(means[1]) == {0, 1, 2, 3, 4}, counts_present(means[1])
    if lut is not None:
        assert not np.array_equal(means[0], quad_means(lm.offsets, lm.tints, W, H, planes)[0])       # (the tints change the frame)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * (Wo + 24)                                  # wider than the frame; rows below it
    bg = background(Ho + 7, pitch)
    for shape in (1, 2, 4):                                # all three block heights
        ctx.set_tile_shape(shape)
        for x0, y0 in ((4, 3), (5, 3)):                    # 16-byte aligned output pixels (wide stores) / not
            got = run(ctx, bg[None], pitch, lut, x0=x0, y0=y0)[0]
            np.testing.assert_array_equal(got, paste(bg, means, x0, y0), err_msg=f"{cfg} {flavour} block height {8 * shape} origin ({x0},{y0})")
    ctx.close()


# ---- 2. every sum at every count ----------------------------------------------------------------------------------------------
def directed_table():
    """128 x 112, sample i reads texel i.  Rows 0-31: 1024 quads of four samples, sums 0 .. 1020 in plane 0 - whole 128 x 8 / 16 / 32
    tiles, fully mapped: the wide stores.  Rows 32-111: 2560 quads, one per (n, sum) for n = 1 .. 4 and sum = 0 .. 255 n - the n = 3
    ones with the missing sample at each of the four places in turn - in shuffled order, the rest n = 0.  Plane 1 holds the
    complementary sums 255 n - sum, planes 2 and 3 random bytes."""
    W, H, ps = 128, 112, 112
    rng = np.random.default_rng(5)
    off = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    planes = [np.zeros(6 * ps * ps, np.uint8) for _ in range(4)]
    for c in (2, 3):
        planes[c][:] = rng.integers(0, 256, 6 * ps * ps)
    cases = [(4, s, -1) for s in range(1021)] + [(4, int(s), -1) for s in rng.integers(0, 1021, 3)]      # the fully mapped part
    mixed = [(n, s, (s % 4) if n == 3 else -1) for n in (1, 2, 3, 4) for s in range(255 * n + 1)]
    assert len(mixed) == 2554
    mixed += [(0, 0, -1)] * (2560 - len(mixed))
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    cases += mixed
    assert len(cases) == (H // 2) * (W // 2)
    for q, (n, s, missing) in enumerate(cases):
        Y, X = divmod(q, W // 2)
        places = [(2 * Y + (k >> 1), 2 * X + (k & 1)) for k in range(4)]
        if n == 3:
            keep = [k for k in range(4) if k != missing]
        else:
            keep = sorted(int(k) for k in rng.permutation(4)[:n])
        for k in range(4):
            if k not in keep:
                off[places[k]] = O.NULL
        for i, k in enumerate(keep):
            v = s // n + (1 if i < s % n else 0)
            planes[0][off[places[k]]] = v
            planes[1][off[places[k]]] = 255 - v
    return W, H, ps, off.reshape(-1), [p.reshape(6, ps, ps) for p in planes], cases


def test_every_sum_at_every_count(bk):
    W, H, ps, off, planes, cases = directed_table()
    means = quad_means(off, None, W, H, planes)
    # the table holds what it is meant to hold (a precondition on the INPUT): per count every sum, in the mixed part and - n = 4 - in the
    # fully mapped part; all four places of the missing sample at n = 3
    mapped = (off != O.NULL).reshape(H, W)
    sums0 = (planes[0].reshape(-1)[np.where(off == O.NULL, 0, off)].astype(np.int64) * mapped.reshape(-1)).reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
    n = means[1]
    assert mapped[:32].all() and set(sums0[:16].ravel()) == set(range(1021))
    for cnt in (1, 2, 3, 4):
        assert set(sums0[16:][n[16:] == cnt]) == set(range(255 * cnt + 1)), cnt
    holes3 = {tuple(np.argwhere(~mapped[2 * Y:2 * Y + 2, 2 * X:2 * X + 2])[0]) for Y, X in np.argwhere(n == 3)}
    assert holes3 == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert counts_present(n) == {0, 1, 2, 3, 4}
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, None)
    pitch = 4 * (W // 2)
    bg = background(H // 2, pitch)
    want = paste(bg, means, 0, 0)
    for shape in (1, 2, 4):
        ctx.set_tile_shape(shape)
        got = run(ctx, bg[None], pitch)[0]
        st = ctx.tile_stats()
        assert st["slow"] == 0, st                         # every block staged: the register path is what is being tested
        np.testing.assert_array_equal(got, want, err_msg=f"block height {8 * shape}")
    ctx.close()


# ---- 3. batch and ring wrap ---------------------------------------------------------------------------------------------------
def test_batch_wraps_the_ring_of_truecolour_globes(bk):
    import torch
    lm = O.lensmap("cube", "hammer", None, 960, 540)
    W, H, G, F = lm.W, lm.H, 3, 5
    Wo, Ho = W // 2, H // 2
    ctx = make_ctx(bk, W, H, 4 * G)
    planes = [planes_of(lm.ps, g) for g in range(G)]
    for g in range(G):
        upload_planes(ctx, g, planes[g])
    ctx.set_lensmap(lm.offsets, lm.tints)
    pitch = 4 * Wo
    want = [paste(np.full((Ho, pitch), 9, np.uint8), quad_means(lm.offsets, lm.tints, W, H, planes[g]), 0, 0) for g in range(G)]
    # frames back to back / padded by a multiple of 16 / padded by 4 mod 16 (no wide stores in frames 1 .. 3)
    for extra in (0, 3 * pitch + 16, 3 * pitch + 4):
        stride = Ho * pitch + extra
        out = torch.from_numpy(np.full(F * stride, 9, np.uint8)).cuda()
        ctx.apply_rgba_ss2_device(out.data_ptr(), pitch, stride, globe0=2, nframes=F)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for f in range(F):
            np.testing.assert_array_equal(got[f * stride:f * stride + Ho * pitch].reshape(Ho, pitch), want[(2 + f) % G], err_msg=f"frame {f} extra {extra}")
            assert (got[f * stride + Ho * pitch:(f + 1) * stride] == 9).all(), "bytes between the frames were written"
    ctx.close()


# ---- 4. blocks without staging ------------------------------------------------------------------------------------------------
TINTS_0_TO_7_AND_255 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 255], np.uint8)


def scrambled_table(rng):
    """517 x 301 random offsets, 7 % of them NULL, tints drawn from 0 .. 7 and 255 pixel by pixel -> W, H, ps, off, tints"""
    W, H, ps = 517, 301, 301
    n = W * H
    off = rng.integers(0, 6 * ps * ps, n, dtype=np.uint32)
    off[rng.random(n) < 0.07] = O.NULL
    tints = TINTS_0_TO_7_AND_255[rng.integers(0, len(TINTS_0_TO_7_AND_255), n)]
    return W, H, ps, off, tints


@pytest.mark.parametrize("tinted", [False, True])
def test_scrambled_tables_and_blocks_without_staging(bk, tinted):
    """the tables of test_apply_rgba_gpu.py's test of the same name: (a) every block staged, (b) the staging buffer forced so small
    that every list exceeds it, (c) blocks that have no chunk list at all; tints drawn from 0 .. 7 and 255 pixel by pixel"""
    rng = np.random.default_rng(77)
    values = TINTS_0_TO_7_AND_255
    lut = random_luts(4) if tinted else None
    W, H, ps, off, tints = scrambled_table(rng)
    planes = planes_of(ps, 0, seed=11)
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, tints)
    pitch = 4 * (Wo + 3)
    bg = background(Ho + 4, pitch)
    want = paste(bg, quad_means(off, tints, W, H, planes, lut), 2, 1)
    for shape, ldskb, direct in ((4, 64, False), (2, 1, True), (1, 4, True), (0, 0, False)):
        ctx.set_tile_shape(shape)
        ctx.set_tile_shape(400 + ldskb)
        got = run(ctx, bg[None], pitch, lut, x0=2, y0=1)[0]
        st = ctx.tile_stats()                              # (of the block map the launch above made the current one)
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
    tints = values[rng.integers(0, len(values), n)]
    planes = planes_of(ps, 0, seed=5)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(off, tints)
    ctx.set_tile_shape(4)
    ctx.set_tile_shape(464)                                # 64 KiB: every list that exists fits, so "slow" counts the blocks without one
    pitch = 4 * (W // 2)
    bg = background(H // 2, pitch)
    got = run(ctx, bg[None], pitch, lut)[0]
    st = ctx.tile_stats()
    assert st["slow"] > 0, st
    np.testing.assert_array_equal(got, paste(bg, quad_means(off, tints, W, H, planes, lut), 0, 0), err_msg=str(st))
    ctx.close()


@pytest.mark.parametrize("tinted", [False, True])
def test_blocks_without_staging_in_a_batch(bk, tinted):
    """the frame loop of the direct gather: table (a) above under 128 x 8 blocks and 1 KiB of staging - every list exceeds it - launched
    for FIVE frames from globe 1 of a ring of two truecolour globes, so that a block visit serves several frames of alternating globes
    (test 4 launches such blocks for one frame, test 3's batch is fully staged).  Every frame and the bytes between the frames are
    compared: a visit that read its first frame's globe for all its frames fails here."""
    import torch
    W, H, ps, off, tints = scrambled_table(np.random.default_rng(77))
    lut = random_luts(4) if tinted else None
    G, F, globe0 = 2, 5, 1
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    ctx = make_ctx(bk, W, H, 4 * G)
    planes = [planes_of(ps, g, seed=11) for g in range(G)]
    for g in range(G):
        upload_planes(ctx, g, planes[g])
    ctx.set_lensmap(off, tints)
    ctx.set_tile_shape(1)
    ctx.set_tile_shape(401)
    pitch = 4 * (Wo + 3)
    bg = background(Ho + 4, pitch)
    want = [paste(bg, quad_means(off, tints, W, H, planes[g], lut), 2, 1) for g in range(G)]
    assert not np.array_equal(want[0], want[1])
    stride = bg.size + 3 * pitch + 4                       # frames apart by rows nobody owns and 4 bytes more
    filled = np.full(F * stride, 9, np.uint8)
    for f in range(F):
        filled[f * stride:f * stride + bg.size] = bg.ravel()
    out = torch.from_numpy(filled).cuda()
    ctx.apply_rgba_ss2_device(out.data_ptr(), pitch, stride, globe0=globe0, nframes=F, x0=2, y0=1, lut=lut)
    torch.cuda.synchronize()
    st = ctx.tile_stats()
    assert st["slow"] > 0, st
    got = out.cpu().numpy()
    for f in range(F):
        np.testing.assert_array_equal(got[f * stride:f * stride + bg.size].reshape(bg.shape), want[(globe0 + f) % G], err_msg=f"frame {f} {st}")
        assert (got[f * stride + bg.size:(f + 1) * stride] == 9).all(), f"bytes behind frame {f} were written"
    ctx.close()


# ---- 5. stripes ------------------------------------------------------------------------------------------------------------------
def test_stripe_contexts_write_their_output_rows_only_and_concatenate(bk):
    import torch
    lm = O.lensmap("trism", "panini", None, 960, 540)
    W, H = lm.W, lm.H
    Wo, Ho = W // 2, H // 2
    planes = planes_of(lm.ps, 0, seed=1)
    means = quad_means(lm.offsets, lm.tints, W, H, planes)
    pitch = 4 * Wo
    bg = background(Ho, pitch)
    want = paste(bg, means, 0, 0)
    off2, tin2 = lm.offsets.reshape(H, W), lm.tints.reshape(H, W)

    def stripe(frame, r0, r1):
        ctx = make_ctx(bk, W, H, 4, rows=(r0, r1))
        upload_planes(ctx, 0, planes)
        ctx.set_lensmap(off2[r0:r1], tin2[r0:r1])
        got = run(ctx, frame[None], pitch)[0]
        ctx.close()
        np.testing.assert_array_equal(got, paste(frame, means, 0, 0, rows=(r0 // 2, (r1 + 1) // 2)), err_msg=f"rows [{r0},{r1})")
        return got

    frame = bg.copy()
    for r0, r1 in ((0, 102), (102, H)):                    # 102: even, not a multiple of 8
        frame = stripe(frame, r0, r1)
    np.testing.assert_array_equal(frame, want)
    # a cut with a gap: output row 135 is nobody's
    frame = bg.copy()
    for r0, r1 in ((0, 270), (272, H)):
        frame = stripe(frame, r0, r1)
    np.testing.assert_array_equal(frame[135], bg[135])
    np.testing.assert_array_equal(np.delete(frame, 135, axis=0), np.delete(want, 135, axis=0))
    # a quad must not straddle two contexts
    out = torch.zeros((Ho, pitch), dtype=torch.uint8, device="cuda")
    for r0, r1 in ((101, H), (0, 101), (0, 271)):          # odd row0 / odd row1 below H
        ctx = make_ctx(bk, W, H, 4, rows=(r0, r1))
        ctx.set_lensmap(off2[r0:r1], tin2[r0:r1])
        with pytest.raises(bk.BlinkyError, match=r"\[-6\].*row0 must be even and row1 even or"):
            ctx.apply_rgba_ss2_device(out.data_ptr(), pitch, Ho * pitch)
        ctx.close()
    torch.cuda.synchronize()
    assert not out.any()


# ---- 6. neighbours undisturbed ------------------------------------------------------------------------------------------------
def test_neighbouring_launches_are_undisturbed(bk):
    import torch
    lm = O.lensmap("cube", "panini", None, 640, 480)
    W, H = lm.W, lm.H
    Wo, Ho = W // 2, H // 2
    planes = planes_of(lm.ps, 0, seed=2)                   # slot c = 8-bit globe c
    pal = O.palmap(O.synthetic_basepal())
    lut = random_luts(6)
    ctx = make_ctx(bk, W, H, 4)
    upload_planes(ctx, 0, planes)
    ctx.set_lensmap(lm.offsets, lm.tints)
    bg, bgo = background(H, 4 * W), background(Ho, 4 * Wo)

    def full(l):
        want = bg.copy()
        for c in range(4):
            plane = np.ascontiguousarray(want[:, c::4])
            if l is None:
                O.apply(lm.offsets, None, W, H, planes[c], plane, W, 0, 0)
            else:
                O.apply(lm.offsets, lm.tints, W, H, planes[c], plane, W, 0, 0, True, l[c])
            want[:, c::4] = plane
        return want

    want = {"plain": full(None), "tinted": full(lut),
            "ss2": paste(bgo, quad_means(lm.offsets, lm.tints, W, H, planes), 0, 0),
            "ss2-tinted": paste(bgo, quad_means(lm.offsets, lm.tints, W, H, planes, lut), 0, 0)}
    for rubix in (False, True):
        want[f"8bit-{int(rubix)}"] = np.stack([O.apply(lm.offsets, lm.tints, W, H, planes[(1 + f) % 4], np.full((H, W), 5, np.uint8), W, 0, 0, rubix, pal)
                                               for f in range(4)])

    def launch(what):
        if what.startswith("8bit"):
            out = torch.full((4, H, W), 5, dtype=torch.uint8, device="cuda")
            ctx.apply_device(out.data_ptr(), W, H * W, frame0=1, nframes=4, rubix_on=what.endswith("1"), pal=pal)
        elif what.startswith("ss2"):
            out = torch.from_numpy(bgo).cuda()
            ctx.apply_rgba_ss2_device(out.data_ptr(), 4 * Wo, 4 * Wo * Ho, lut=lut if what == "ss2-tinted" else None)
        else:
            out = torch.from_numpy(bg).cuda()
            if what == "plain":
                ctx.apply_rgba_device(out.data_ptr(), 4 * W, 4 * W * H)
            else:
                ctx.apply_rgba_tinted_device(out.data_ptr(), 4 * W, 4 * W * H, lut)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    orders = (("8bit-0", "8bit-1", "plain", "tinted", "ss2", "ss2-tinted"),
              ("ss2-tinted", "8bit-1", "ss2", "plain", "ss2", "tinted", "ss2-tinted", "8bit-0", "ss2"))
    for order in orders:
        for what in order:
            np.testing.assert_array_equal(launch(what), want[what], err_msg=f"{what} in {order}")
    ctx.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lut", [False, True])
def test_errors(bk, with_lut):
    import torch
    W, H = 64, 48
    Wo, Ho = W // 2, H // 2
    lm = O.lensmap("cube", "panini", None, W, H)
    lut = random_luts(8) if with_lut else None
    out = torch.zeros((Ho, Wo + 8, 4), dtype=torch.uint8, device="cuda")
    p, pitch, stride = out.data_ptr(), 4 * (Wo + 8), 4 * (Wo + 8) * Ho
    ctx = make_ctx(bk, W, H, 4)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        ctx.apply_rgba_ss2_device(p, pitch, stride, lut=lut)
    ctx.set_lensmap(lm.offsets, lm.tints)
    ctx.apply_rgba_ss2_device(p, pitch, stride, x0=8, lut=lut)                     # the widest origin the pitch allows
    ctx.apply_rgba_ss2_device(p, 4 * Wo, stride, lut=lut)                          # the pitch bound is at Wo, not at W
    for kw in (dict(pitch=4 * Wo - 4), dict(x0=9), dict(x0=-1), dict(y0=-1), dict(globe0=-1), dict(nframes=0),
               dict(pitch=pitch + 2), dict(stride=stride + 1), dict(ptr=p + 2)):
        a = dict(ptr=p, pitch=pitch, stride=stride, globe0=0, nframes=1, x0=0, y0=0)
        a.update(kw)
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            ctx.apply_rgba_ss2_device(a["ptr"], a["pitch"], a["stride"], globe0=a["globe0"], nframes=a["nframes"], x0=a["x0"], y0=a["y0"], lut=lut)
    ctx.set_apply_variant(0)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*staged variant"):
        ctx.apply_rgba_ss2_device(p, pitch, stride, lut=lut)
    ctx.set_apply_variant(2)
    ctx.close()
    ctx = make_ctx(bk, W, H, 3)                                                   # fewer than four ring slots: no truecolour globe
    ctx.set_lensmap(lm.offsets, lm.tints)
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*four ring slots"):
        ctx.apply_rgba_ss2_device(p, pitch, stride, lut=lut)
    ctx.close()
    torch.cuda.synchronize()
