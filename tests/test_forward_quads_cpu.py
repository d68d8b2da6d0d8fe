"""The inputs and the reference of tests/test_forward_quads_gpu.py, checked without a GPU: what the committed corner tables contain
(tests/quad_tables.py: census), and the oracle's ok_forward_from_corners held to the oracle's own forward build and - quad by quad -
to its draw_quad."""
import numpy as np
import pytest

import oracle_ffi as O
import quad_tables as Q
import scripts as S

NULL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def tables():
    return [Q.table(s) for s in Q.COMMITTED]


@pytest.fixture(scope="module")
def results(tables):
    """the oracle's full table of every committed seed, computed once"""
    return {i: O.forward_from_corners(t.globe, t.W, t.H, t.grid, t.xy, t.ok) for i, t in enumerate(tables)}


def test_the_generator_knows_the_globes_and_repeats_itself(tables):
    for g, n in Q.NPLATES.items():
        assert len(O.globe_plates(g)) == n, g
        assert g in S.GLOBES and "globe_plate" not in S.script("globes", g), g
    for s in (0, 7, 39):
        a, b = Q.table(s), tables[s]
        assert (a.globe, a.W, a.H, a.grid, a.rows, a.kind) == (b.globe, b.W, b.H, b.grid, b.rows, b.kind)
        assert np.array_equal(a.xy, b.xy) and np.array_equal(a.ok, b.ok)
    for t in tables:
        ps = min(t.W, t.H)
        assert t.xy.dtype == np.int32 and t.ok.dtype == np.uint8
        assert t.ok.size == Q.NPLATES[t.globe] * (ps + 1) ** 2 and t.xy.shape == (t.ok.size, 2)
        assert all(0 <= a < b <= t.H for a, b in t.rows)
        if len(t.rows) == 2:                                     # a pair: complementary, cut at a row that is no multiple of 8
            assert t.rows[0][0] == 0 and t.rows[0][1] == t.rows[1][0] and t.rows[1][1] == t.H and t.rows[0][1] % 8
    assert {min(t.W, t.H) for t in tables} == {8, 15, 16, 17, 33, 48, 70}
    assert {t.globe for t in tables} == set(Q.GLOBES) and {t.grid for t in tables} == set(Q.GRIDS)
    assert {len(t.rows) for t in tables} == {1, 2} and any(t.rows == ((0, t.H),) for t in tables) and any(len(t.rows) == 1 and t.rows != ((0, t.H),) for t in tables)
    assert any(t.W < t.H for t in tables) and any(t.W > t.H for t in tables)


def test_the_committed_tables_hold_every_class_of_quad_tile_and_pixel(tables, results):
    """A condition on the INPUTS of the GPU test: at least 50 of every class the quad pass treats differently, none of the excluded one."""
    index = {id(t): i for i, t in enumerate(tables)}
    c = Q.census(tables, lambda t: O.texel_owners(t.globe, min(t.W, t.H)), lambda t: (results[index[id(t)]].offsets, results[index[id(t)]].tints))
    text = "\n".join("%-28s %d" % (k, c[k]) for k in Q.CLASSES + (Q.EXCLUDED,))
    print(text)
    assert c[Q.EXCLUDED] == 0, text
    thin = [k for k in Q.CLASSES if c[k] < 50]
    assert not thin, f"fewer than 50 of {thin}:\n{text}"


FORWARD_LENSES = [l for l in S.LENSES if O.lens_def(l)["has_forward"] and not O.lens_def(l)["has_inverse"]]


def test_there_are_ten_forward_lenses():
    assert len(FORWARD_LENSES) == 10, FORWARD_LENSES


@pytest.mark.parametrize("size", [(64, 48), (45, 70)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lens", FORWARD_LENSES)
def test_from_corners_gives_the_forward_build_its_own_table(lens, size):
    """the oracle's forward build, asked for the corner table it computed; that table through ok_forward_from_corners: the same
    offsets, tints and display"""
    W, H = size
    for globe, grid in (("cube", (10, 4.0, 1.0)), ("tetra", (5, 1.0, 3.0))):
        lm = O.lensmap(globe, lens, None, W, H, grid, corners=True)
        assert lm.built and lm.map_type == 2 and lm.corner_ok is not None, (globe, lens)
        assert set(np.unique(lm.corner_ok)) <= {0, 1}, "a corner the build never wrote"
        got = O.forward_from_corners(globe, W, H, grid, lm.corner_xy, lm.corner_ok)
        np.testing.assert_array_equal(got.offsets, lm.offsets, err_msg=f"{globe}/{lens}")
        np.testing.assert_array_equal(got.tints, lm.tints, err_msg=f"{globe}/{lens}")
        assert got.display == lm.display and got.numplates == lm.numplates
        assert lm.nonnull > 0


@pytest.mark.parametrize("seed", [16, 7, 14, 5, 10, 24])      # 16x16, 8x13, 15x40, 17x131, 131x17, 40x15 on cube, tetra, trism, cube_corner, trism, cube
def test_from_corners_is_draw_quad_in_scan_order(tables, results, seed):
    """Every accepted quad of a table painted with ok_test_draw_quad alone - plates ascending, py descending, px ascending, later ones
    over earlier ones - gives the from-corners offsets: the loop order and the ownership test of the new entry, pinned without its code.
    (Ownership is the oracle's texel_owners; the size check and the four ok flags are restated in tests/quad_tables.py.)"""
    t = tables[seed]
    W, H, ps = t.W, t.H, min(t.W, t.H)
    q = Q.quads(t, O.texel_owners(t.globe, ps))
    acc = Q.accepted(q)
    want = np.full(W * H, NULL, np.uint32)
    painted = 0
    for plate in range(Q.NPLATES[t.globe]):
        for py in range(ps - 1, -1, -1):
            for px in range(ps):
                if not q["live"][plate, py, px]:
                    continue
                mask = O.draw_quad_mask(W, H, q["c"][:, plate, py, px].reshape(8))
                assert acc[plate, py, px] or not mask.any()        # (what the size check rejects draws nothing)
                want[mask != 0] = (plate * ps + py) * ps + px
                painted += int(mask.any())
    assert painted > 20, t.kind
    np.testing.assert_array_equal(results[seed].offsets, want, err_msg=t.kind)
    shown = [int(((want != NULL) & (want // (ps * ps) == p)).any()) for p in range(Q.NPLATES[t.globe])]
    assert all(d >= s for d, s in zip(results[seed].display, shown))      # (display also counts plates later painted over)
