"""The trilinear apply without a GPU: the three models of tests/trilinear_model.py (pyramid, level of detail, frame) each against a second
formulation in plain Python loops, the blend's identities, the level-of-detail derivation on host builds - the CONDITIONS that keep the
GPU files from testing nothing - and the census of the drawn cases those files apply; the same for the deep files (tests/test_*_deep_gpu.py,
platesizes with 10 to 12 levels): the directed ramp against the pixel loop, and what the ramp and the deep stripes have to reach."""
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


# ---- 5. depth: what tests/test_*_deep_gpu.py run - platesizes with 10 to 12 levels ------------------------------------------------------
def test_the_deep_platesizes_reach_what_they_are_there_for():
    """the arithmetic behind the comments of tests/test_mip_pyramid_deep_gpu.py's DEEP"""
    import test_apply_rgba_fb_gpu as FB
    import test_mip_pyramid_deep_gpu as MD
    s = {ps: TM.level_sizes(ps) for ps in MD.DEEP}
    assert sorted(MD.DEEP) == [129, 130, 257, 258, 260, 513, 640, 721, 1024, 1025] and set(MD.DEEP.values()) == set(FB.LAYOUTS)
    assert [len(s[ps]) for ps in sorted(MD.DEEP)] == [9, 9, 10, 10, 10, 11, 11, 11, 11, 12]
    assert s[129][1] - 64 == s[130][1] - 64 == 1 and s[257][1] - 128 == s[258][1] - 128 == 1      # the last tile's level-1 width: one texel column
    assert s[260][1] % 2 == 0 and s[260][2] - 64 == 1                   # ... and its level-2 width at 260
    assert s[513][4] ** 2 > 1024 >= TM.level_sizes(512)[4] ** 2         # 513 is the first platesize at which the tail's loop comes round
    assert s[721][4] ** 2 >= 2048 > TM.level_sizes(720)[4] ** 2         # 721 the first at which every one of its 1024 threads does
    assert all(v % 2 == 0 for v in s[1024][:-1]) and s[640][:8] == [640, 320, 160, 80, 40, 20, 10, 5]
    assert s[1025][4:6] == [65, 33] and len(s[1025]) <= TM.MAX_LEVELS


def test_rho_stays_below_2_to_the_23_at_the_largest_platesize():
    """lod_kernel's `rho << 8` and its comment rest on this bound alone: no GPU test reaches platesizes near it"""
    ps_max = 26752                                                      # the widest padded plate bk_resize accepts (tests/test_rgba_fb_abi.py)
    assert (ps_max - 1) * 256 + 255 < 2 ** 23 and ((ps_max - 1) * 256 + 255) << 8 < 2 ** 31


@pytest.mark.parametrize("ps,W", [(2, 3), (3, 51), (5, 13), (33, 100), (65, 196)])
def test_the_ramp_is_the_pixel_loop_and_its_rows_hold_their_step(ps, W):
    table, sub, (r0, r1) = TM.ramp_case(ps, W, r0=2, H=40)
    off, tints, W, H, ps = table
    assert r1 - r0 == len(TM.ramp_steps(ps)) == 3 * (((ps - 1) * 256).bit_length() - 8)
    o, s = off.reshape(H, W)[r0:r1].reshape(-1), sub.reshape(H, W)[r0:r1].reshape(-1)
    for bias in (0, -300, 300):
        np.testing.assert_array_equal(TM.derive_lod(o, s, W, r1 - r0, ps, bias), TM.derive_lod_loops(o, s, W, r1 - r0, ps, bias))
    _, detail = TM.derive_lod(o, s, W, r1 - r0, ps, detail=True)
    m = (o != NULL).reshape(r1 - r0, W)
    for i, step in enumerate(TM.ramp_steps(ps)):
        assert m[i].any() and (detail["rho"][i][m[i]] == step).all(), (i, step)
    assert (off.reshape(H, W)[:r0] == NULL).all() and (off.reshape(H, W)[r1:] == NULL).all()


def test_census_of_the_deep_ramp():
    """tests/test_lod_deep_gpu.py's ramp: every targeted rho on a mapped pixel, every lower level below the top at bias 0, the top level at
    the bias that puts the deepest row on it; steps forward and backward along a row, none and refused ones across rows"""
    import test_lod_deep_gpu as LD
    ps, W = LD.RAMP
    table, sub, (r0, r1) = TM.ramp_case(ps, W)
    off, tints, W, H, ps = table
    assert r0 % 8 != 0
    o, s = off.reshape(H, W)[r0:r1].reshape(-1), sub.reshape(H, W)[r0:r1].reshape(-1)
    m = o != NULL
    top = len(TM.level_sizes(ps)) - 1
    lod, detail = TM.derive_lod(o, s, W, r1 - r0, ps, detail=True)
    rho = detail["rho"].reshape(-1)[m]
    targets = [(1 << k) + d for k in range(8, 19) for d in (-1, 0, 1)]      # written out for ps 1025: (ps - 1) * 256 = 2^18
    assert targets == TM.ramp_steps(ps) and {255, 256, 257, 65535, 65536, 65537, 2 ** 18 + 1} <= set(targets)
    counts = {t: int((rho == t).sum()) for t in targets}
    assert all(c > 0 for c in counts.values()), counts
    assert set(rho.tolist()) == set(targets)                            # ... and nothing else: every step is exact
    levels = [int(((lod[m] >> 8) == k).sum()) for k in range(top + 1)]
    assert all(c > 0 for c in levels[:top]) and levels[top] == 0, levels
    biases = LD.biases(ps)
    assert biases[:3] == (-300, 0, 300) and biases[3] == 256
    at_top = TM.derive_lod(o, s, W, r1 - r0, ps, biases[3])[m]
    assert (at_top == top * 256).sum() == counts[2 ** 18] + counts[2 ** 18 + 1] and at_top.max() == top * 256      # reached, not clamped
    assert (TM.derive_lod(o, s, W, r1 - r0, ps, 300)[m] == top * 256).sum() > (at_top == top * 256).sum()           # (300 clamps more onto it)
    assert (TM.derive_lod(o, s, W, r1 - r0, ps, -300)[m] == 0).sum() > (lod[m] == 0).sum()
    ways = {a: set(detail[a][m.reshape(r1 - r0, W)].tolist()) for a in "hv"}
    assert ways == dict(h={1, -1}, v={0}) and detail["other_plate"] > 0, ways
    print(f"ramp ps {ps} W {W} rows {r0}..{r1}: {int(m.sum())} mapped, pixels per rho {min(counts.values())}..{max(counts.values())}, "
          f"lower level 0..{top} at bias 0: {levels}, on the top level at bias {biases[3]}: {int((at_top == top * 256).sum())}, "
          f"refused for their plate: {detail['other_plate']} (recorded: 33528 mapped, 1016 a rho, [4064, 3048 nine times, 2032, 0], 2032, 65024)")


def right_clamp_reachable(ps, k):
    """can a position inside a plate of side ps pass the centre of level k's last texel?  The right (bottom) clamp at level k needs
    U >> k >= (s_k - 1) * 256 + 129 (sx >= 256 with a weight), and U is at most (ps - 1) * 256 + 255.  At ps = 2^n + 1 the last texel of
    every level k >= 1 holds ONE level-0 column and the answer is no; at ps = 2^n it is yes at every level."""
    s = TM.level_sizes(ps)[k]
    return (((s - 1) * 256 + 129) << k) <= (ps - 1) * 256 + 255


def test_census_of_the_deep_apply_cases():
    """tests/test_apply_rgba_fb_trilinear_deep_gpu.py's cases, WITHIN THE OWNED ROWS of each: every level as the lower one; the fractions and
    tints that matter; a NULL inside a lane beside mapped pixels; and for the rims each of the four clamps at every level k >= 1 with
    s_k > 1 - the right and the bottom one at every level where a position can reach them at all (right_clamp_reachable).
    Recorded: the fewest pixels with one lower level 361 (corners 260x257, level 4), 1255 at 1027x1025; a NULL inside a lane 297 to 1742
    times a case; on the rims the fewest pixels at one clamp and level: left / top 223 (260x257, level 4), right / bottom 826 at 1026x1024
    (every level 1 to 10) and 558 at 724x721 (levels 5, 7, 8; 0 at 1, 2, 3, 4, 6, 9 and at every level of 257, 513, 1025, as the geometry says)"""
    import test_apply_rgba_fb_trilinear_deep_gpu as TD
    assert [right_clamp_reachable(1024, k) for k in range(1, 10)] == [True] * 9
    assert not any(right_clamp_reachable(ps, k) for ps in (257, 513, 1025) for k in range(1, len(TM.level_sizes(ps)) - 1))
    assert [k for k in range(1, 10) if right_clamp_reachable(721, k)] == [5, 7, 8]
    sides = ("left", "right", "top", "bottom")
    for name, kind, (off, tints, W, H, ps), sub, lod, (r0, r1) in TD.deep_cases():
        assert ps == min(W, H) == H and r0 % 8 != 0 and 0 < r0 < r1 < H and 16 <= r1 - r0 <= 18
        own = lambda a: np.asarray(a).reshape(H, W)[r0:r1]
        off, sub, tints, lod = own(off), own(sub), own(tints), own(lod)
        sizes = TM.level_sizes(ps)
        top = len(sizes) - 1
        assert top >= 9 and (lod <= top * 256).all()
        m = off != NULL
        mapped, plate, U, V = TM.positions(off[m], sub[m], ps)
        lo, fl = lod[m].astype(np.int64) >> 8, lod[m] & 255
        lower = [int((lo == k).sum()) for k in range(top + 1)]
        assert min(lower) >= 200, (name, lower)                         # (the smallest stripe: 17 x 260 pixels, a fifth of them NULL, over 10 levels)
        assert {0, 1, 127, 128, 255} <= set(fl.tolist()), name
        assert {0, 1, 2, 3, 4, 5, 6, 200, 255} <= set(tints[m].tolist()), name
        lanes = m[:, :W - W % 4].reshape(r1 - r0, -1, 4).sum(axis=2)
        null_in_lane = int(((lanes > 0) & (lanes < 4)).sum())
        assert null_in_lane > 0, name
        clamped = {side: [0] * (top + 1) for side in sides}
        for k in range(1, top + 1):
            at = (lo == k) | (np.minimum(lo + 1, top) == k)
            Uk, Vk, s = U[at] >> k, V[at] >> k, sizes[k]
            sx, sy = (Uk & 255) + 128, (Vk & 255) + 128
            clamped["left"][k] = int((((Uk >> 8) == 0) & (sx < 256)).sum())
            clamped["right"][k] = int((((Uk >> 8) == s - 1) & (sx >= 256) & ((sx & 255) > 0)).sum())
            clamped["top"][k] = int((((Vk >> 8) == 0) & (sy < 256)).sum())
            clamped["bottom"][k] = int((((Vk >> 8) == s - 1) & (sy >= 256) & ((sy & 255) > 0)).sum())
        if kind == "corners":
            for k in range(1, top + 1):
                if sizes[k] > 1:
                    for side in sides:
                        if side in ("left", "top") or right_clamp_reachable(ps, k):
                            assert clamped[side][k] > 0, (name, side, k, clamped)
                        else:
                            assert clamped[side][k] == 0, (name, side, k)
        print(f"{name} rows {r0}..{r1}: {int(m.sum())} mapped, lower level 0..{top}: {lower}, NULL inside a lane {null_in_lane}, clamps per level 1..{top} "
              + ", ".join(f"{side} {clamped[side][1:]}" for side in sides))
