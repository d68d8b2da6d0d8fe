"""The trilinear apply without a GPU: the three models of tests/trilinear_model.py (pyramid, level of detail, frame) each against a second
formulation in plain Python loops, the blend's identities, the level-of-detail derivation on host builds - the CONDITIONS that keep the
GPU files from testing nothing - and the census of the drawn cases those files apply."""
import numpy as np
import pytest

import rgba_fb_model as M
import subtexel_model as SM
import test_subtexel_cpu as SC
import trilinear_model as TM

NULL = TM.NULL
PLATESIZES = [1, 2, 3, 5, 16, 33]


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


# ---- 1. second formulations -----------------------------------------------------------------------------------------------------------
def test_level_counts():
    assert [len(TM.level_sizes(ps)) for ps in (1, 2, 3, 5, 16, 33, 203, 2160, 26752)] == [1, 2, 3, 4, 5, 7, 9, 13, 16]
    assert TM.level_sizes(203) == [203, 102, 51, 26, 13, 7, 4, 2, 1]


@pytest.mark.parametrize("ps", PLATESIZES)
def test_the_numpy_pyramid_is_the_texel_loop(ps):
    plates = np.random.default_rng(8100 + ps).integers(0, 256, (2, ps, ps, 4)).astype(np.uint8)
    plates[0, ::2, ::2] = 255                                           # (rounding at the top of the range)
    pyr = TM.pyramid(plates)
    assert [l.shape[1] for l in pyr] == TM.level_sizes(ps)
    for p in range(2):
        for a, b in zip(pyr, TM.pyramid_loops(plates[p])):
            np.testing.assert_array_equal(a[p], b)


def test_a_checkerboard_averages_to_128():
    y, x = np.divmod(np.arange(256), 16)
    board = np.repeat((((x + y) % 2) * 255).astype(np.uint8).reshape(16, 16, 1), 4, axis=2)
    assert (TM.pyramid(board)[1] == 128).all()


def test_the_lod_values_are_the_comparison_against_powers_of_two():
    rho = np.concatenate([np.arange(0, 3000), [4095, 4096, 4097, 65535, 65536, 2 ** 23 - 1], np.random.default_rng(1).integers(0, 2 ** 23, 2000)])
    for bias, levels in ((0, 16), (-300, 9), (300, 9), (0, 1), (5000, 3)):
        np.testing.assert_array_equal(TM.lod_value(rho, bias, levels), [TM.lod_value_loops(int(r), bias, levels) for r in rho])
    v = TM.lod_value(np.arange(0, 70000), 0, 16)
    assert (np.diff(v) >= 0).all() and np.diff(v).max() <= 2            # monotone, steps of at most 2
    assert [int(TM.lod_value(r, 0, 16)) for r in (256, 257, 511, 512, 768)] == [0, 1, 255, 256, 384]


def small_case(seed, ps=None):
    rng = np.random.default_rng(8200 + seed)
    W, H = int(rng.integers(1, 14)), int(rng.integers(1, 10))
    if ps is not None:
        W, H = (ps, ps + int(rng.integers(0, 4))) if seed % 2 else (ps + int(rng.integers(0, 6)), ps)
    ps = min(W, H)
    n = W * H
    # runs of neighbouring texels on one plate, so that steps exist, with jumps and NULLs between
    plate = np.repeat(rng.integers(0, 6, n), 3)[:n]
    px, py = (np.arange(n) * 2 + rng.integers(0, 2, n)) % ps, (np.arange(n) // W * 3 + rng.integers(0, 2, n)) % ps
    off = (plate * ps * ps + py * ps + px).astype(np.uint32)
    off[rng.random(n) < 0.2] = NULL
    edge = np.array([0, 127, 128, 255])
    axis = lambda: np.where(rng.random(n) < 0.5, edge[rng.integers(0, 4, n)], rng.integers(0, 256, n))
    sub = (axis() | (axis() << 8)).astype(np.uint16)
    tints = np.array([0, 1, 2, 3, 4, 5, 6, 200, 255], np.uint8)[rng.integers(0, 9, n)]
    plates = rng.integers(0, 256, (6, ps, ps, 4)).astype(np.uint8)
    lut = rng.integers(0, 256, (4, 6, 256)).astype(np.uint8)
    return W, H, ps, off, sub, tints, plates, lut


CASES = [(seed, None) for seed in range(6)] + [(10 + i, ps) for i, ps in enumerate(PLATESIZES)]


@pytest.mark.parametrize("seed,ps", CASES)
def test_the_numpy_lod_is_the_pixel_loop(seed, ps):
    W, H, ps, off, sub, tints, plates, lut = small_case(seed, ps)
    for bias in (0, -300, 300):
        for r0, r1 in ((0, H), (H // 3, H)):
            o, s = off.reshape(H, W)[r0:r1].reshape(-1), sub.reshape(H, W)[r0:r1].reshape(-1)
            np.testing.assert_array_equal(TM.derive_lod(o, s, W, r1 - r0, ps, bias), TM.derive_lod_loops(o, s, W, r1 - r0, ps, bias))


@pytest.mark.parametrize("seed,ps", CASES)
def test_the_numpy_frame_is_the_written_out_weights(seed, ps):
    W, H, ps, off, sub, tints, plates, lut = small_case(seed, ps)
    rows = (0, H) if seed % 3 else (H // 3, H)
    lod = TM.random_lods((rows[1] - rows[0]) * W, ps, seed)
    pyr = TM.pyramid(plates)
    for table in (None, lut):
        a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
        b = a.copy()
        TM.trilinear_frame(pyr, off, sub, lod, tints, W, H, ps, rows, table, a, 2, 1)
        TM.trilinear_frame_loops(pyr, off, sub, lod, tints, W, H, ps, rows, table, b, 2, 1)
        np.testing.assert_array_equal(a, b)


# ---- 2. the blend's identities ------------------------------------------------------------------------------------------------------------
def test_blend_identities_for_every_fraction():
    v = np.concatenate([np.arange(0, 255 * 65536 + 1, 4099), [255 * 65536]]).astype(np.int64)
    assert (((v * 256 + (1 << 23)) >> 24) == ((v + 32768) >> 16)).all()                      # fl = 0: the bilinear call's rounding
    for fl in range(256):
        for c in (0, 1, 127, 128, 254, 255):                                                # a constant plate: v = c * 65536 on both levels
            assert (c * 65536 * (256 - fl) + c * 65536 * fl + (1 << 23)) >> 24 == c
        assert 255 * 65536 * 256 + (1 << 23) < 1 << 32


@pytest.mark.parametrize("seed,ps", CASES)
def test_a_plane_of_zeros_is_the_bilinear_frame_and_a_constant_plate_its_constant(seed, ps):
    W, H, ps, off, sub, tints, plates, lut = small_case(seed, ps)
    zeros = np.zeros(W * H, np.uint16)
    for table in (None, lut):
        a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
        b = a.copy()
        TM.trilinear_frame(TM.pyramid(plates), off, sub, zeros, tints, W, H, ps, (0, H), table, a, 2, 1)
        SM.bilinear_frame(plates, off, sub, tints, W, H, ps, (0, H), table, b, 2, 1)
        np.testing.assert_array_equal(a, b)
    flat = np.empty_like(plates)
    flat[...] = plates[:, :1, :1, :]
    a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
    b = a.copy()
    TM.trilinear_frame(TM.pyramid(flat), off, sub, TM.random_lods(W * H, ps, seed), tints, W, H, ps, (0, H), None, a, 2, 1)
    M.fb_frame(flat, off, tints, W, H, ps, (0, H), None, False, b, 2, 1)
    np.testing.assert_array_equal(a, b)


# ---- 3. the derivation on host builds: what the GPU files' real builds reach ------------------------------------------------------------
def host_lod(bk, lens, onload=None):
    ctx = SC.host_ctx(bk, lens)
    if onload:
        import scripts as S
        ctx.set_zoom(*S.zoom_args(onload))
    off, tin, sub, display, scale, err = ctx.host_build_subtexel(1)
    assert err is None
    ctx.close()
    W, H = SC.SIZE
    lod = TM.derive_lod(off, sub, W, H, min(W, H))
    m = off != NULL
    return lod[m], int(m.sum())


def test_hammer_minifies_everywhere(bk):
    lod, mapped = host_lod(bk, "hammer")
    counts = [int(((lod >> 8) == k).sum()) for k in range(3)]
    print(f"hammer 203x131: {mapped} mapped, lower level 0 / 1 / 2: {counts}, lod 0: {int((lod == 0).sum())} (recorded: 562 / 13001 / 2612, 0)")
    assert counts[1] >= 10000 and counts[2] >= 2000 and (lod == 0).sum() == 0


def test_panini_magnifies_its_centre(bk):
    lod, mapped = host_lod(bk, "panini", "f_fov 180")
    print(f"panini 203x131: {mapped} mapped, lod 0: {int((lod == 0).sum())}, level >= 1: {int((lod >= 256).sum())} (recorded: 8253, 1212)")
    assert (lod == 0).sum() >= 5000 and (lod >= 256).sum() >= 500


def test_a_forward_map_minifies_like_hammer(bk):
    lod, mapped = host_lod(bk, "winkel2")
    print(f"winkel2 203x131: {mapped} mapped, level 1: {int(((lod >> 8) == 1).sum())} (recorded: 18126)")
    assert ((lod >> 8) == 1).sum() >= 10000


# ---- 4. the census of the committed drawn cases ---------------------------------------------------------------------------------------------
def test_census_of_the_committed_apply_cases():
    """tests/test_apply_rgba_fb_trilinear_gpu.py's drawn cases (tables, subs, hand-set planes) and tests/test_lod_gpu.py's drawn tables reach
    what the kernels can get wrong"""
    import test_apply_rgba_fb_trilinear_gpu as T
    import test_lod_gpu as TL
    lo_seen, fl_seen, tint_values, sizes_seen = {}, set(), set(), set()
    top_clamped = null_in_lane = 0
    clamped = dict(left=0, right=0, top=0, bottom=0)
    for (off, tints, W, H, ps), sub, lod in T.committed_cases():
        off, sub, tints, lod = (np.asarray(a) for a in (off, sub, tints, lod))
        assert off.shape == sub.shape == tints.shape == lod.shape == (W * H,)
        sizes = TM.level_sizes(ps)
        top = len(sizes) - 1
        assert (lod <= top * 256).all()
        m = off != NULL
        mapped, plate, U, V = TM.positions(off[m], sub[m], ps)
        lo, fl = lod[m].astype(np.int64) >> 8, lod[m] & 255
        lo_seen.setdefault(ps, set()).update(lo.tolist())
        fl_seen |= set(fl.tolist())
        top_clamped += int(((lo == top) & (top > 0)).sum())
        tint_values |= set(tints[m].tolist())
        sizes_seen |= set(sizes)
        for k in range(1, top + 1):
            at = (lo == k) | (np.minimum(lo + 1, top) == k)
            Uk, Vk, s = U[at] >> k, V[at] >> k, sizes[k]
            if s > 1:
                sx, sy = (Uk & 255) + 128, (Vk & 255) + 128
                clamped["left"] += int((((Uk >> 8) == 0) & (sx < 256)).sum())
                clamped["right"] += int((((Uk >> 8) == s - 1) & (sx >= 256) & ((sx & 255) > 0)).sum())
                clamped["top"] += int((((Vk >> 8) == 0) & (sy < 256)).sum())
                clamped["bottom"] += int((((Vk >> 8) == s - 1) & (sy >= 256) & ((sy & 255) > 0)).sum())
        grid = m.reshape(H, W)
        for x in range(0, W - W % 4, 4):
            lane = grid[:, x:x + 4].sum(axis=1)
            null_in_lane += int(((lane > 0) & (lane < 4)).sum())
    for ps, seen in lo_seen.items():
        assert seen == set(range(len(TM.level_sizes(ps)))), (ps, seen)      # every level as the lower one, the top one included
    assert 1 in lo_seen and top_clamped > 0
    assert {0, 1, 127, 128, 255} <= fl_seen
    assert all(v > 0 for v in clamped.values()), clamped
    assert any(s % 2 == 1 and s > 1 for s in sizes_seen)
    assert null_in_lane > 0
    assert {0, 1, 2, 3, 4, 5, 6, 200, 255} <= tint_values
    # the derivation's drawn tables: steps forward, backward and none on both axes, a neighbour refused for its plate
    ways = dict(h=set(), v=set())
    refused = 0
    for (off, tints, W, H, ps), sub in TL.drawn_cases():
        _, detail = TM.derive_lod(off, sub, W, H, ps, detail=True)
        m = (np.asarray(off) != NULL).reshape(H, W)
        for axis in "hv":
            ways[axis] |= set(detail[axis][m].tolist())
        refused += detail["other_plate"]
    assert ways["h"] == {1, -1, 0} and ways["v"] == {1, -1, 0}, ways
    assert refused > 0
