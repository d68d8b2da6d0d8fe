"""TEST INFRASTRUCTURE: texel-corner tables for the forward build's QUAD PASS (tests/test_forward_quads_cpu.py,
tests/test_forward_quads_gpu.py).

bk_forward_quads / bk_forward_resolve are a pure integer function of the corner table, the globe's plates, the rubix grid and the
stripe: draw_quad's three paths, the wrapped INT_MIN arithmetic, the 48 x 48 LDS window with its 16-bit box vote, the ordered-overwrite
commit through atomicMax keys across workgroups and plates, the second key plane of the stale tint, the stripe filter, the
bk_forward_tiles shortcut.  A lens only hands them the quads it happens to produce; bk_debug_set_forward_corners hands them ANY table,
and the oracle's ok_forward_from_corners says what the reference's loop makes of it.  Here a seed is one such table:

    table(seed) -> Table(globe, W, H, grid, rows, xy, ok, kind)

ps = min(W, H); xy int32 [n, 2] and ok uint8 [n] in bk_debug_host_corners' numbering, corner (plate, j, i) = (plate * (ps+1) + j) *
(ps+1) + i; rows = the stripes to build it on, ((0, H),) or one arbitrary stripe or two complementary ones; kind = what the seed drew,
for failure messages.  The complementary cut is a row that is no multiple of 8, one to five rows below the screen point one of the
table's plates - any of them, magnifying or not - was aimed at; that cuts do pass through tiles' windows is the census class
tile_cut_by_stripe's to show, not the cut's construction.  Every plate of a table draws its own family and parameters, so plates land on top of each other.

ONE EXCLUSION.  A quad with one bound at INT_MIN and the other at exactly 0 on the same axis passes the reference's size check
(abs(INT_MIN) == INT_MIN) and the oracle then scans 2^31 rows or columns, ten seconds apiece.  No INT_MIN corner is put into a quad that
has a 0 on that axis (`_keep_int_min_from_zero`), and census() counts such quads so that the tests can hold the count to 0.  That class
stays with test_draw_quad_with_int_min_corners_scans_like_the_reference and the script-fuzz seeds 368 and 605.

numpy only, like sessiongen.py."""
import collections

import numpy as np

BASE_SEED = 47000
COMMITTED = range(40)            # the seeds both test files run; the coverage test holds this range to every census class

INT_MIN = -2 ** 31
MAXDIFF = 20                     # fisheye.c:2248
TILE, WIN = 16, 48               # BK_FWD_TILE, BK_FWD_WIN (blinky_amd/csrc/bk_build_kernels.h)

NPLATES = {"cube": 6, "cube_corner": 6, "trism": 5, "tetra": 4}      # (globes with a globe_plate script are out of scope)
GLOBES = tuple(NPLATES)
# ps in {8, 15, 16, 17, 33, 48, 70}: below one tile, one tile less a row, exactly one, one plus a live row and column, the same across
# three tiles, three whole tiles, five with a ragged edge; the other side up to 131 so that a window can overflow 48 pixels in x and -
# W < H - in y.  Both orientations.  (13 sizes against 4 globes and 4 grids: a seed range of 40 walks all of them past each other.)
SIZES = ((131, 48), (15, 40), (48, 131), (16, 16), (131, 70), (17, 131), (70, 131), (8, 13), (131, 33), (33, 70), (131, 17), (40, 15), (72, 48))
# the default grid (fisheye.c:672) and three from the build campaign's list: a wide pad, a fractional one, none at all
GRIDS = ((10, 4.0, 1.0), (5, 1.0, 3.0), (23, 7.5, 0.25), (1, 4.0, 0.0))
# minifying, 1:1, magnifying up to the 20-pixel limit and one past it
FACTORS = (0.25, 0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 20.0, 21.0)
BIG = (32766, 32767, 32768, 32769, -32767, -32768, -32769, 2 ** 24 - 1, 2 ** 24, -(2 ** 24 - 1), -(2 ** 24))

Table = collections.namedtuple("Table", "globe W H grid rows xy ok kind")


def _affine(rng, ps, W, H):
    """(A, t, anchor on the screen): round(A (i, j) + t) with one chosen corner of the grid landing on a chosen point of the screen - across an
    edge, across a corner, inside, or the whole image outside"""
    if rng.random() < 0.5:                     # entries straight from the list, zeros and signs included
        pick = lambda: float(rng.choice(FACTORS)) * (1 if rng.random() < 0.5 else -1)
        a, d = pick(), pick()
        b = pick() if rng.random() < 0.25 else 0.0
        c = pick() if rng.random() < 0.25 else 0.0
        if rng.random() < 0.08:
            a = 0.0                            # a collapsed axis: every quad a vertical line
        if rng.random() < 0.08:
            d = 0.0
        A = np.array([[a, b], [c, d]])
        how = "axes %g %g %g %g" % (a, b, c, d)
    else:                                      # rotations by multiples of 30 degrees times a factor, mirrored or not
        f = float(rng.choice(FACTORS))
        k = int(rng.integers(0, 12))
        th = np.deg2rad(30.0 * k)
        A = f * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        mirror = rng.random() < 0.5
        if mirror:
            A = A @ np.diag([-1.0, 1.0])
        how = "rot %d x%g%s" % (30 * k, f, " mirrored" if mirror else "")
    where = int(rng.integers(0, 12))
    tx, ty = [(W // 2, H // 2), (0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1), (0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0),
              (W // 3, H // 3), (2 * W // 3, 2 * H // 3), None][where] or (None, None)
    i0, j0 = int(rng.integers(0, ps + 1)), int(rng.integers(0, ps + 1))
    if tx is None:                             # wholly outside: the image's box ends a few pixels short of the screen, or far away
        ext = np.abs(A).sum(axis=1) * ps
        off = float(rng.choice([3.0, 40.0, 1000.0]))
        side = int(rng.integers(0, 4))
        c0 = A @ np.array([ps / 2.0, ps / 2.0])
        centre = [(-ext[0] / 2 - off, H / 2.0), (W + ext[0] / 2 + off, H / 2.0), (W / 2.0, -ext[1] / 2 - off), (W / 2.0, H + ext[1] / 2 + off)][side]
        t = np.array(centre) - c0
        anchor = (W // 2, H // 2)
        how += " outside"
    else:
        t = np.array([tx, ty], float) - A @ np.array([i0, j0], float)
        anchor = (tx, ty)
        how += " at (%d, %d)" % (tx, ty)
    return A, t, anchor, how


def _plate(rng, ps, W, H):
    """one plate's corners, int64 [ps+1, ps+1, 2] (j, i, xy), its family's name and the screen point it was aimed at"""
    n1 = ps + 1
    jj, ii = np.meshgrid(np.arange(n1), np.arange(n1), indexing="ij")
    A, t, anchor, how = _affine(rng, ps, W, H)
    g = np.stack([A[0, 0] * ii + A[0, 1] * jj + t[0], A[1, 0] * ii + A[1, 1] * jj + t[1]], axis=-1)
    xy = np.rint(g).astype(np.int64)
    family = int(rng.integers(0, 4))
    if family == 1 or family == 3:             # per-corner jitter: bow ties, one-row / one-column / one-pixel quads, boxes at the limit
        m = int(rng.integers(1, 13))
        part = 1.0 if rng.random() < 0.5 else 0.3
        jit = rng.integers(-m, m + 1, size=xy.shape)
        xy = xy + jit * (rng.random(xy.shape[:2]) < part)[..., None]
        how += " jitter %d on %g" % (m, part)
    if family == 2 or family == 3:             # folds: many texels of the plate on one pixel, neighbouring quads crossing
        for axis, size in ((0, W), (1, H)):
            r = rng.random()
            if r < 0.4:
                c = int(rng.integers(size // 4, 3 * size // 4 + 1))
                xy[..., axis] = np.abs(xy[..., axis] - c) + (0 if rng.random() < 0.5 else c - 3)
                how += " fold%s |v-%d|" % ("xy"[axis], c)
            elif r < 0.8:
                mod = int(rng.integers(5, 41))
                xy[..., axis] = np.mod(xy[..., axis], mod) + int(rng.integers(-3, size))
                how += " fold%s mod %d" % ("xy"[axis], mod)
    return xy, how, anchor


def _scatter(rng, xy, ok, nplates, ps):
    """the scattered corners, 1-5 % each: ok = 0; INT_MIN with ok = 1; whole neighbourhoods moved out to +-32 767 and +-2^24"""
    n1 = ps + 1
    names = []
    if rng.random() < 0.6:
        ok[rng.random(ok.shape) < rng.uniform(0.01, 0.05)] = 0
        names.append("ok0")
    if rng.random() < 0.6:
        # blocks of 3..6 x 3..6 corners keep their shape and move: their inner quads pass the size check far from the screen, in tiles
        # whose other quads stay on it
        for _ in range(max(1, int(rng.uniform(0.01, 0.05) * nplates * n1 * n1 / 16))):
            p, bh, bw = int(rng.integers(0, nplates)), int(rng.integers(3, 7)), int(rng.integers(3, 7))
            j, i = int(rng.integers(0, max(1, n1 - bh))), int(rng.integers(0, max(1, n1 - bw)))
            axis, v = int(rng.integers(0, 2)), int(rng.choice(BIG))
            blk = xy[p, j:j + bh, i:i + bw, axis]
            blk += v - blk[blk.shape[0] // 2, blk.shape[1] // 2]
        names.append("far")
    if rng.random() < 0.6:
        hit = rng.random(ok.shape) < rng.uniform(0.01, 0.05)
        which = rng.integers(0, 3, size=ok.shape)            # x, y or both
        xy[..., 0][hit & (which != 1)] = INT_MIN
        xy[..., 1][hit & (which != 0)] = INT_MIN
        names.append("intmin")
    return names


def _keep_int_min_from_zero(xy):
    """THE EXCLUSION (module docstring): a 0 that shares a quad and an axis with an INT_MIN becomes a 1"""
    for axis in (0, 1):
        v = xy[..., axis]
        im = v == INT_MIN
        q_im = im[:, :-1, :-1] | im[:, :-1, 1:] | im[:, 1:, :-1] | im[:, 1:, 1:]          # per quad
        near = np.zeros(v.shape, bool)                                                  # corners of such quads
        near[:, :-1, :-1] |= q_im
        near[:, :-1, 1:] |= q_im
        near[:, 1:, :-1] |= q_im
        near[:, 1:, 1:] |= q_im
        v[near & (v == 0)] = 1


def table(seed):
    rng = np.random.default_rng(BASE_SEED + seed)
    globe = GLOBES[seed % len(GLOBES)]
    W, H = SIZES[seed % len(SIZES)]
    grid = GRIDS[(seed // 2) % len(GRIDS)]
    ps, nplates = min(W, H), NPLATES[globe]
    n1 = ps + 1
    xy = np.zeros((nplates, n1, n1, 2), np.int64)
    ok = np.ones((nplates, n1, n1), np.uint8)
    kinds, anchors = [], []
    for p in range(nplates):
        xy[p], how, anchor = _plate(rng, ps, W, H)
        kinds.append(how)
        anchors.append(anchor)
    kinds += _scatter(rng, xy, ok, nplates, ps)
    _keep_int_min_from_zero(xy)
    assert xy.min() >= INT_MIN and xy.max() < 2 ** 31
    # rows: full, one arbitrary stripe, or two complementary stripes cut at a row that is no multiple of 8, just below where a plate was aimed
    r = seed % 3
    if r == 0 or H < 4:
        rows = ((0, H),)
    elif r == 1:
        r0 = int(rng.integers(0, H - 1))
        rows = ((r0, int(rng.integers(r0 + 1, H + 1))),)
    else:
        cut = min(max(anchors[int(rng.integers(0, nplates))][1] + int(rng.integers(1, 6)), 1), H - 1)
        while cut % 8 == 0:
            cut = cut - 1 if cut > 1 else cut + 1
        rows = ((0, cut), (cut, H))
    return Table(globe, W, H, grid, rows, xy.reshape(-1, 2).astype(np.int32), ok.reshape(-1), "; ".join(kinds))


# ---- the census: what the committed seeds contain, counted from the corner tables ------------------------------------------------
CLASSES = (
    # quads that own their ray and have four ok corners ("live"), by what draw_quad does with them
    "rows_1", "rows_2", "rows_3_19", "extent_20", "rejected_21", "rejected_beyond",
    "straddle_left", "straddle_right", "straddle_top", "straddle_bottom", "accepted_offscreen", "int_min_corner", "ok0_corner",
    # tiles of 16 x 16 texels
    "tile_box_over_48_x", "tile_box_over_48_y", "tile_no_vote", "tile_far_vote_and_onscreen", "tile_cut_by_stripe",
    "tile_on_region_border", "tile_on_region_border_drawing",
    # pixels
    "px_boxes_of_two_plates", "px_stale_tint", "px_null_inside",
)
EXCLUDED = "int_min_with_zero"


def quads(t, owners):
    """per quad [plates, ps, ps] of a table: live (owns its ray, four ok corners), the box minx / maxx / miny / maxy (int64), any_ok0"""
    ps = min(t.W, t.H)
    n1 = ps + 1
    xy = t.xy.reshape(-1, n1, n1, 2).astype(np.int64)
    ok = t.ok.reshape(-1, n1, n1).astype(bool)
    c = np.stack([xy[:, :-1, :-1], xy[:, :-1, 1:], xy[:, 1:, :-1], xy[:, 1:, 1:]])          # tl, tr, bl, br
    ok4 = ok[:, :-1, :-1] & ok[:, :-1, 1:] & ok[:, 1:, :-1] & ok[:, 1:, 1:]
    own = np.asarray(owners, bool)
    return dict(c=c, own=own, live=own & ok4, ok0=own & ~ok4, minx=c[..., 0].min(0), maxx=c[..., 0].max(0), miny=c[..., 1].min(0), maxy=c[..., 1].max(0))


def accepted(q):
    """the reference's size check (fisheye.c:2272) with its wrapping abs()"""
    def within(lo, hi):
        d = ((lo - hi + 2 ** 31) % 2 ** 32) - 2 ** 31            # int subtraction, wrapped
        a = np.where(d < 0, ((-d + 2 ** 31) % 2 ** 32) - 2 ** 31, d)   # abs(): INT_MIN stays INT_MIN
        return a <= MAXDIFF
    return q["live"] & within(q["minx"], q["maxx"]) & within(q["miny"], q["maxy"])


def census(tables, owners_of=None, result_of=None):
    """Counter over CLASSES + EXCLUDED for a list of tables.  owners_of(table) -> bool [plates, ps, ps], which texels own their ray (the
    oracle's texel_owners; None: all of them); result_of(table) -> (offsets, tints) of the oracle's full table for the last three
    classes' pixel counts (None: they stay 0)."""
    n = collections.Counter({k: 0 for k in CLASSES + (EXCLUDED,)})
    for t in tables:
        W, H, ps = t.W, t.H, min(t.W, t.H)
        nplates = NPLATES[t.globe]
        q = quads(t, np.ones((nplates, ps, ps), bool) if owners_of is None else owners_of(t))
        minx, maxx, miny, maxy, live = q["minx"], q["maxx"], q["miny"], q["maxy"], q["live"]
        im = (q["c"] == INT_MIN)
        has_im = im.any(axis=(0, -1))
        for axis in (0, 1):
            n[EXCLUDED] += int((im[..., axis].any(0) & (q["c"][..., axis] == 0).any(0)).sum())
        acc = accepted(q)
        plain = acc & ~has_im                                   # (boxes of INT_MIN quads wrap: they are counted on their own)
        on = plain & (maxx >= 0) & (minx < W) & (maxy >= 0) & (miny < H)
        dx, dy = maxx - minx, maxy - miny
        ext = np.maximum(dx, dy)
        n["rows_1"] += int((on & (dy == 0)).sum())
        n["rows_2"] += int((on & (dy == 1)).sum())
        n["rows_3_19"] += int((on & (dy >= 2) & (dy <= 18)).sum())
        n["extent_20"] += int((on & (ext == 20)).sum())
        box_on = live & ~has_im & (maxx >= 0) & (minx < W) & (maxy >= 0) & (miny < H)
        n["rejected_21"] += int((box_on & (ext == 21)).sum())
        n["rejected_beyond"] += int((box_on & (ext > 21)).sum())
        n["straddle_left"] += int((on & (minx < 0)).sum())
        n["straddle_right"] += int((on & (maxx >= W)).sum())
        n["straddle_top"] += int((on & (miny < 0)).sum())
        n["straddle_bottom"] += int((on & (maxy >= H)).sum())
        n["accepted_offscreen"] += int((plain & ~on).sum())
        n["int_min_corner"] += int((live & has_im).sum())
        n["ok0_corner"] += int(q["ok0"].sum())
        # tiles: the box vote of bk_forward_quads - every live quad whose corners are all inside (-2^24, 2^24), clamped to 16 bits
        votes = live & (minx > -(1 << 24)) & (miny > -(1 << 24)) & (maxx < (1 << 24)) & (maxy < (1 << 24))
        far = votes & ((maxx > 32767) | (maxy > 32767) | (minx < -32767) | (miny < -32767))
        bounds = sorted({b for r in t.rows for b in r if 0 < b < H})
        for p in range(nplates):
            for ty in range(0, ps, TILE):
                for tx in range(0, ps, TILE):
                    s = (p, slice(ty, ty + TILE), slice(tx, tx + TILE))
                    # a tile with texels on both sides of its plate's region border (what bk_forward_tiles must leave to the exact test),
                    # and such a tile with a live on-screen quad next to a texel that must not draw
                    mixed = bool(q["own"][s].any() and not q["own"][s].all())
                    n["tile_on_region_border"] += mixed
                    n["tile_on_region_border_drawing"] += bool(mixed and on[s].any())
                    v = votes[s]
                    if not v.any():
                        n["tile_no_vote"] += 1
                        continue
                    x0 = min(int(np.maximum(minx[s][v], 0).min()), 32767)
                    y0 = min(int(np.maximum(miny[s][v], 0).min()), 32767)
                    x1 = min(max(int(maxx[s][v].max()), -1), 32767)
                    y1 = min(max(int(maxy[s][v].max()), -1), 32767)
                    n["tile_box_over_48_x"] += x1 - x0 + 1 > WIN
                    n["tile_box_over_48_y"] += y1 - y0 + 1 > WIN
                    n["tile_far_vote_and_onscreen"] += bool(far[s].any() and on[s].any())
                    h = min(max(y1 - y0 + 1, 0), WIN)
                    n["tile_cut_by_stripe"] += any(y0 <= b - 1 and b <= y0 + h - 1 for b in bounds)
        # pixels under the boxes of accepted quads of two plates or more (difference arrays, one per plate)
        D = np.zeros((nplates, H + 1, W + 1), np.int64)
        pp, yy, xx = np.nonzero(on)
        ax0, ax1 = np.clip(minx[on], 0, W), np.clip(maxx[on] + 1, 0, W)
        ay0, ay1 = np.clip(miny[on], 0, H), np.clip(maxy[on] + 1, 0, H)
        np.add.at(D, (pp, ay0, ax0), 1)
        np.add.at(D, (pp, ay0, ax1), -1)
        np.add.at(D, (pp, ay1, ax0), -1)
        np.add.at(D, (pp, ay1, ax1), 1)
        cover = D.cumsum(1).cumsum(2)[:, :H, :W] > 0
        n["px_boxes_of_two_plates"] += int((cover.sum(0) >= 2).sum())
        if result_of is not None:
            off, tin = result_of(t)
            off, tin = off.reshape(H, W), tin.reshape(H, W)
            mapped = off != 0xFFFFFFFF
            n["px_stale_tint"] += int((mapped & (tin != 255) & (tin != (off // (ps * ps)).astype(np.uint8))).sum())
            # NULL inside the image: an unmapped pixel with mapped ones on both sides of it in its row
            left = np.maximum.accumulate(mapped, axis=1)
            right = np.maximum.accumulate(mapped[:, ::-1], axis=1)[:, ::-1]
            n["px_null_inside"] += int((~mapped & left & right).sum())
    return n
