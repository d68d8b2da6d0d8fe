"""The NUMBERS of the staged apply's block map against tests/blockmap_model.py, exactly: bk_debug_tile_stats, bk_debug_traffic_model,
bk_debug_band_balance and bk_debug_row_costs are integer functions of (table, tints, W, owned rows, block height, flavour, block-cost
knob), and a wrong one changes no frame - the ~700 byte-for-byte frame tests cannot see it - but moves bench.py's compulsory bytes, the
launcher's choices or where the multi-GPU stripes are cut.  Tables go in through bk_set_lensmap; every comparison is equality.
tests/test_blockmap_model_cpu.py holds the model itself (second formulation, recorded device values) and the census of these tables."""
import numpy as np
import pytest

import blockmap_model as BM
import oracle_ffi as O
import scripts as S

pytestmark = pytest.mark.gpu

_MODELS = {}


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def model(t, rows, rg, tinted, block_cost=BM.BLOCK_COST):
    k = (t.name, rows, rg, tinted)
    if k not in _MODELS:
        _MODELS[k] = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, tinted)
    return _MODELS[k].with_block_cost(block_cost)


def context(bk, t, rows=None, tuning=False):
    ctx = bk.Context()
    ctx.resize(t.W, t.H)
    ctx.set_blockmap_tuning(tuning)
    load(ctx, t, rows)
    return ctx


def load(ctx, t, rows=None):
    r0, r1 = rows if rows is not None else (0, t.H)
    ctx.set_rows(r0, r1)
    ctx.set_lensmap(t.off.reshape(t.H, t.W)[r0:r1].ravel(), t.tints.reshape(t.H, t.W)[r0:r1].ravel())


def check(ctx, t, rows, tinted, block_cost=BM.BLOCK_COST, rg=None, lds_kb=None, what=""):
    """the four debug calls of the context's current block map against the model at the height the map reports (rg: the height it must
    report) and the staging buffer it reports (lds_kb: the one it must report)"""
    ts = ctx.tile_stats()
    assert ts["tile_h"] // 1000 == 128 and ts["tile_h"] % 1000 in (8, 16, 32), ts
    got_rg = ts["tile_h"] % 1000 // 8
    where = f"{t} rows {rows} rg {got_rg} tinted {tinted} block cost {block_cost} lds {ts['lds_bytes_per_wave']} {what}"
    if rg is not None:
        assert got_rg == rg, where
    if lds_kb is not None:
        assert ts["lds_bytes_per_wave"] == lds_kb * 1024, where
    bm = model(t, rows, got_rg, tinted, block_cost)
    assert ts == BM.tile_stats(bm, ts["lds_bytes_per_wave"]), "tile_stats: " + where
    assert ctx.traffic_model() == BM.traffic_model(bm), "traffic_model: " + where
    assert ctx.band_balance() == BM.band_balance(bm), "band_balance: " + where
    np.testing.assert_array_equal(ctx.row_costs(), BM.row_costs(bm), err_msg="row_costs: " + where)
    return got_rg


def launch(ctx, t, rows, rubix):
    """one 8-bit launch; the frame is the oracle's on the owned rows and untouched elsewhere"""
    pal = O.palmap(((np.arange(768) * 37 + 11) % 256).astype(np.uint8))
    got = ctx.apply(np.full((t.H, t.W), 77, np.uint8), rubix_on=rubix, pal=pal)
    want = np.full((t.H, t.W), 77, np.uint8)
    tints = np.where(t.tints < 6, t.tints, 255).astype(np.uint8)       # (a tint that names no plate leaves the texel as it is: class 0;
    #                                                                      the oracle has palettes for the six plates and 255 only)
    full = O.apply(t.off, tints, t.W, t.H, O.lcg_globe(t.ps, 6, 0), np.full((t.H, t.W), 77, np.uint8), rubix_on=rubix, pal=pal)
    want[rows[0]:rows[1]] = full[rows[0]:rows[1]]
    np.testing.assert_array_equal(got, want, err_msg=f"{t} rows {rows} rubix {rubix}: frame")


def fill_globe(ctx):
    for p in range(6):
        ctx.fill_plate_lcg(0, p, 0)


@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_forced_heights(bk, t):
    """every table x stripe x forced height: the default knobs, the staging buffer forced to 1 and 4 KiB (400 + kb: `slow` counts the
    blocks that need more), the block-cost knob at 0 and 9 (601 + n: costs, bands, row prices)"""
    ctx = context(bk, t)
    for rows in t.stripes():
        load(ctx, t, rows)
        for rg in BM.HEIGHTS:
            ctx.set_tile_shape(rg)
            check(ctx, t, rows, False, rg=rg)
            for kb in (1, 4):
                ctx.set_tile_shape(400 + kb)
                check(ctx, t, rows, False, rg=rg, lds_kb=kb)
            ctx.set_tile_shape(400)
            for n in (0, 9):
                ctx.set_tile_shape(601 + n)
                check(ctx, t, rows, False, block_cost=n, rg=rg)
            ctx.set_tile_shape(600)
    ctx.close()


@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_tinted_flavour_and_back(bk, t):
    """an 8-bit rubix launch makes the tinted map the current one: (chunk, class) is what its blocks count; a plain launch brings the
    plain map back.  Both are kept, so neither may have changed - at the three forced heights and at the height the cost model picks"""
    rows = t.stripes()[1 if t.H > 1 else 0]
    ctx = context(bk, t, rows)
    fill_globe(ctx)
    for rg in (1, 2, 4, 0):
        ctx.set_tile_shape(rg)
        for rep in range(2):
            launch(ctx, t, rows, True)
            check(ctx, t, rows, True, rg=rg or None, what=f"rubix launch {rep}")
            launch(ctx, t, rows, False)
            check(ctx, t, rows, False, rg=rg or None, what=f"plain launch {rep}")
    ctx.close()


@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_the_chosen_map_reports_itself(bk, t):
    """no forced height, tuning off: whatever height and buffer the cost model picks (neither is under test), the numbers are the
    model's at that height - before any launch (the row costs compile a map of their own) and after one"""
    for rows in t.stripes()[:2]:
        ctx = context(bk, t, rows)
        np.testing.assert_array_equal(ctx.row_costs(), BM.row_costs(model(t, rows, ctx.tile_stats()["tile_h"] % 1000 // 8, False)))
        fill_globe(ctx)
        launch(ctx, t, rows, False)
        check(ctx, t, rows, False, what="chosen")
        ctx.close()


def test_the_measured_map_reports_itself(bk):
    """... and with tuning on (the measured choice of height, form and buffer), single-frame launches"""
    t = BM.small_tables()[1]
    for rows in t.stripes()[:2]:
        ctx = context(bk, t, rows, tuning=True)
        fill_globe(ctx)
        launch(ctx, t, rows, False)
        check(ctx, t, rows, False, what="measured")
        launch(ctx, t, rows, True)
        check(ctx, t, rows, True, what="measured, tinted")
        ctx.close()


def test_after_a_table_change(bk):
    """a second table through bk_set_lensmap, bk_set_rows to another stripe, bk_resize: the numbers are the new table's"""
    draws = [t for t in BM.small_tables() if t.name.startswith("draw")]
    a, b = [t for t in draws if (t.W, t.H) == (257, 100)][:2]
    c = [t for t in draws if (t.W, t.H) == (517, 199)][0]
    d = [t for t in BM.small_tables() if t.name == "3x9"][0]
    ctx = context(bk, a)
    fill_globe(ctx)
    for rg in BM.HEIGHTS:
        ctx.set_tile_shape(rg)
        load(ctx, a)
        check(ctx, a, (0, a.H), False, rg=rg)
        launch(ctx, a, (0, a.H), True)                      # (both flavours compiled for table a; the tinted one is current)
        load(ctx, b)
        check(ctx, b, (0, b.H), True, rg=rg, what="second table: the flavour stays, the numbers are the new table's")
        launch(ctx, b, (0, b.H), False)
        check(ctx, b, (0, b.H), False, rg=rg, what="second table, plain")
        load(ctx, b, (37, 90))
        check(ctx, b, (37, 90), False, rg=rg, what="another stripe")
        launch(ctx, b, (37, 90), True)
        check(ctx, b, (37, 90), True, rg=rg, what="another stripe, tinted")
        load(ctx, a, (99, 100))
        check(ctx, a, (99, 100), True, rg=rg, what="one row of the first table")
        launch(ctx, a, (99, 100), False)
        check(ctx, a, (99, 100), False, rg=rg, what="one row of the first table, plain")
    ctx.resize(c.W, c.H)                                    # larger: the block map's buffers grow
    load(ctx, c, (5, 190))
    check(ctx, c, (5, 190), False, rg=4, what="after a resize")
    ctx.resize(d.W, d.H)
    load(ctx, d)
    check(ctx, d, (0, d.H), False, rg=4, what="after a resize to 3x9")
    ctx.close()


@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_direct_apply_prices_rows_by_their_pixels(bk, t):
    """variant 0: mapped pixels + max(1, W / 32) on the owned rows, 0 elsewhere"""
    ctx = context(bk, t)
    ctx.set_apply_variant(0)
    for rows in t.stripes():
        load(ctx, t, rows)
        np.testing.assert_array_equal(ctx.row_costs(), BM.row_costs_direct(model(t, rows, 4, False)), err_msg=f"{t} rows {rows}")
    ctx.close()


@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_two_device_kernels_and_the_model_agree_on_the_lines_read(bk, t):
    """mark_lines_kernel (the traffic model) and the footprint query count the same tiles, whole frame and stripes"""
    ctx = context(bk, t)
    for rows in t.stripes():
        load(ctx, t, rows)
        lines = ctx.traffic_model()["unique_globe_lines"]
        assert lines == sum(ctx.plate_footprint(p)[1] for p in range(6)) == model(t, rows, 4, False).unique_lines, f"{t} rows {rows}"
    ctx.close()


@pytest.mark.parametrize("N", [2, 4])
def test_the_stripe_cut_is_the_models(bk, N):
    """bk_multi_rebalance on 640x400 cube/hammer with the block height forced on every stripe context (the rebalance prices rows through
    the same ensure_coopmap as bk_debug_row_costs, so the forced height reaches it): the cut is stripe_bounds_from_costs of the MODEL's
    row costs summed over the equal-height stripes, not of costs the device reported; the frames after the rebuild are the oracle's"""
    globe, lens, W, H = "cube", "hammer", 640, 400
    lm = O.lensmap(globe, lens, None, W, H)
    t = BM.Table(f"multi{N}-hammer", W, H, lm.offsets, lm.tints)
    for rg in BM.HEIGHTS:
        m = bk.Multi([0] * N)
        m.load_globe(S.script("globes", globe), globe)
        m.load_lens(S.script("lenses", lens), lens)
        m.set_zoom(bk.ffi.ZOOM_CONTAIN)
        m.resize(W, H)
        for r in range(N):
            m.ctx(r).set_tile_shape(rg)
        m.build()
        equal = [H * r // N for r in range(N + 1)]
        cost = np.zeros(H, np.int64)
        for r in range(N):
            rows = (equal[r], equal[r + 1])
            assert m.ctx(r).size()[3:] == rows
            want = BM.row_costs(model(t, rows, rg, False))
            np.testing.assert_array_equal(m.ctx(r).row_costs(), want, err_msg=f"N {N} rg {rg} rank {r}")
            cost += want
        bounds = m.rebalance()
        assert bounds == bk.ffi.stripe_bounds_from_costs(cost.astype(np.uint32), 0, N), (N, rg)
        m.build()
        for r in range(N):
            rows = (bounds[r], bounds[r + 1])
            assert m.ctx(r).size()[3:] == rows
            np.testing.assert_array_equal(m.ctx(r).row_costs(), BM.row_costs(model(t, rows, rg, False)), err_msg=f"N {N} rg {rg} rank {r} after the cut")
        for p in range(6):
            m.fill_plate_lcg(0, p, 0)
        want = O.apply(lm.offsets, lm.tints, W, H, O.lcg_globe(lm.ps, 6, 0), np.zeros((H, W), np.uint8))
        np.testing.assert_array_equal(m.apply(np.zeros((H, W), np.uint8)), want)
        m.close()
