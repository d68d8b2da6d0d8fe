"""tests/footprint_model.py (the expectation of tests/test_footprint_gpu.py) held to a second formulation and to the CPU oracle, without
a GPU: a Python set of (plate, py // 8, px // 16), the tile counts recorded for three partial configurations, and the conditions that
keep the GPU tests from being vacuous - every configuration whose plates they upload through the footprint has a plate that is read
in part, cube/hammer reads every tile."""
import numpy as np
import pytest

import footprint_model as FM
import oracle_ffi as O


def by_set(offsets, W, H, ps, rows=None):
    """the second formulation: entry by entry in plain Python"""
    r0, r1 = rows if rows is not None else (0, H)
    seen = set()
    for o in np.asarray(offsets).reshape(H, W)[r0:r1].ravel().tolist():
        if o == O.NULL:
            continue
        plate, rem = divmod(o, ps * ps)
        py, px = divmod(rem, ps)
        seen.add((plate, py // 8, px // 16))
    return seen


def check_against_set(offsets, W, H, ps, rows=None):
    masks, counts, rects = FM.footprint(offsets, W, H, ps, rows)
    seen = by_set(offsets, W, H, ps, rows)
    assert {(int(p), int(y), int(x)) for p, y, x in np.argwhere(masks)} == seen
    th, tw = FM.tile_grid(ps)
    assert masks.shape == (6, th, tw) and th == ((ps + 7) & ~7) // 8 and tw == ((ps + 63) & ~63) // 16
    for p in range(6):
        mine = [(y, x) for q, y, x in seen if q == p]
        assert counts[p] == len(mine)
        if not mine:
            assert rects[p] == (0, 0, 0, 0)
            continue
        x0, y0, x1, y1 = rects[p]
        assert x0 == 16 * min(x for _, x in mine) and y0 == 8 * min(y for y, _ in mine)
        assert x1 == min(ps, 16 * (max(x for _, x in mine) + 1)) and y1 == min(ps, 8 * (max(y for y, _ in mine) + 1))
        assert all(x < (ps + 15) // 16 and y < (ps + 7) // 8 for y, x in mine), "a padding tile is marked"
    return counts


@pytest.mark.parametrize("cfg", list(FM.PARTIAL))
def test_model_equals_the_set_and_the_recorded_counts(cfg):
    lm = O.lensmap(*cfg)
    counts = check_against_set(lm.offsets, lm.W, lm.H, lm.ps)
    assert counts == FM.PARTIAL[cfg]
    assert [c > 0 for c in counts[:lm.numplates]] == [bool(d) for d in lm.display]      # ntiles > 0 exactly where `display` is set


def test_model_on_stripes_and_small_tables():
    cfg = ("cube", "panini", None, 640, 480)
    lm = O.lensmap(*cfg)
    whole = FM.footprint(lm.offsets, lm.W, lm.H, lm.ps)[0]
    parts = []
    for rows in ((0, 240), (240, 480), (96, 104)):
        check_against_set(lm.offsets, lm.W, lm.H, lm.ps, rows)
        parts.append(FM.footprint(lm.offsets, lm.W, lm.H, lm.ps, rows)[0])
    assert np.array_equal(parts[0] | parts[1], whole)
    assert 0 < parts[2].sum() < min(parts[0].sum(), parts[1].sum())
    # 17 x 17 with one mapped pixel per plate, and nothing mapped at all
    off = np.full(17 * 17, O.NULL, np.uint32)
    for p in range(6):
        off[20 * p + 3] = p * 289 + (16 - p) * 17 + (p * 3 + 1)
    assert check_against_set(off, 17, 17, 17) == [1] * 6
    assert FM.footprint(off, 17, 17, 17)[2][0] == (0, 16, 16, 17) and FM.footprint(off, 17, 17, 17)[2][5] == (16, 8, 17, 16)
    masks, counts, rects = FM.footprint(np.full(17 * 17, O.NULL, np.uint32), 17, 17, 17)
    assert not masks.any() and counts == [0] * 6 and rects == [(0, 0, 0, 0)] * 6


@pytest.mark.parametrize("cfg", FM.UNTOUCHED_OUTSIDE)
def test_untouched_outside_configurations_have_a_plate_read_in_part(cfg):
    lm = O.lensmap(*cfg)
    counts = FM.footprint(lm.offsets, lm.W, lm.H, lm.ps)[1]
    assert any(0 < c < FM.tiles_inside(lm.ps) for c in counts), counts
    assert any(c == 0 for c in counts), counts              # ... and one that is not read at all (the empty-footprint upload)


def test_trism_panini_is_partial_and_hammer_reads_every_tile():
    lm = O.lensmap("trism", "panini", None, 960, 540)
    assert check_against_set(lm.offsets, lm.W, lm.H, lm.ps) == [855, 852, 0, 140, 138, 0]
    lm = O.lensmap(*FM.FULL)
    masks, counts, rects = FM.footprint(lm.offsets, lm.W, lm.H, lm.ps)
    assert counts == [FM.tiles_inside(lm.ps)] * 6 and rects == [(0, 0, lm.ps, lm.ps)] * 6
    assert FM.texel_mask(masks[0], lm.ps).all()
