"""The seam table (bk_read_seam_table / bk_set_seam_table) on a BK_DEVICE_NONE context, the numpy models of tests/seam_model.py held to
their second formulations, what the table is FOR (less error at the seams than clamping), and the census of the GPU cases of
tests/test_apply_rgba_fb_seams_gpu.py.  No GPU."""
import numpy as np
import pytest

import scripts as S
import seam_model as M
import subtexel_model as SM

NULL = M.NULL
# sizes whose min(W, H) gives ps 1, 2, 9, 16, 33, 203
SIZES = [(1, 3), (5, 2), (131, 9), (96, 16), (64, 33), (261, 203)]
CALLBACK_FREE = [g for g in S.GLOBES if "globe_plate" not in S.script("globes", g)]
WITH_CALLBACK = [g for g in S.GLOBES if "globe_plate" in S.script("globes", g)]


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def host_ctx(bk, globe="cube", size=(96, 64), lens=SM.FLAT_LENS):
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    ctx.load_globe(S.script("globes", globe), globe + ".lua")
    ctx.load_lens(lens, "lens.lua")
    ctx.set_zoom(*S.zoom_args(ctx.lens_info().onload.decode()))
    ctx.resize(*size)
    return ctx


# ---- 1. the table against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_cube_table_is_the_model(bk, W, H):
    ctx = host_ctx(bk, "cube", (W, H))
    head = M.head_of(ctx)
    assert head["ps"] == min(W, H)
    got = ctx.read_seam_table()
    np.testing.assert_array_equal(got, M.seam_table(head))
    if head["ps"] <= 33:
        np.testing.assert_array_equal(got, M.seam_table_loops(head))
    ctx.close()


@pytest.mark.parametrize("globe", [g for g in CALLBACK_FREE if g != "cube"])
def test_every_other_callback_free_globe(bk, globe):
    for size in SIZES:
        ctx = host_ctx(bk, globe, size)
        head = M.head_of(ctx)
        got = ctx.read_seam_table()
        np.testing.assert_array_equal(got, M.seam_table(head), err_msg=f"{globe} {size}")
        if head["ps"] <= 33:
            np.testing.assert_array_equal(got, M.seam_table_loops(head), err_msg=f"{globe} {size}: loops")
        assert (got[len(head["dist64"]):] == NULL).all()
        ctx.close()


@pytest.mark.parametrize("ps", [2, 9, 16, 33, 203])
def test_structure_on_cube(bk, ps):
    ctx = host_ctx(bk, "cube", (ps + 30, ps))
    T = ctx.read_seam_table()
    for p in range(6):
        e = T[p]
        assert (e[e != NULL] // (ps * ps) != p).all(), "an entry targets its own plate"
        assert (e[:, 1:-1] != NULL).all(), "an edge entry is NULL"
        assert e[0, 0] == e[2, 0] and e[0, -1] == e[3, 0] and e[1, 0] == e[2, -1] and e[1, -1] == e[3, -1], "a corner's copies differ"
        rem = e[e != NULL] % (ps * ps)
        ty, tx = rem // ps, rem % ps
        assert ((ty == 0) | (ty == ps - 1) | (tx == 0) | (tx == ps - 1)).all(), "a target off its plate's rim"
    ctx.close()


# ---- 2. a globe with a globe_plate callback -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("globe", WITH_CALLBACK)
def test_callback_globe_is_the_interpreter_texel_by_texel(bk, globe):
    ctx = host_ctx(bk, globe, (40, 12))
    head = M.head_of(ctx)
    ps, n = head["ps"], len(head["dist64"])
    got = ctx.read_seam_table()
    want = np.full((6, 4, ps + 2), NULL, np.uint32)
    x, y = M.virtual_texels(ps)
    for p in range(n):
        ray = M._plate_uv_to_ray(head, p, (x + 0.5) / ps, (y + 0.5) / ps)
        for edge in range(4):
            for i in range(ps + 2):
                r = [ray[k][edge, i] for k in range(3)]
                res = ctx.eval_host(2, *[float(c) for c in r])
                if not res:
                    continue
                d = res[-1]
                q = int(np.rint(d))
                if not (0 <= q < n) or q == p:
                    continue
                px_, py_, pz_ = (np.float64(SM._dot3(head[name][q], r)) for name in ("right", "up", "forward"))
                with np.errstate(all="ignore"):
                    tu, tv = px_ / pz_ * head["dist64"][q] + 0.5, -py_ / pz_ * head["dist64"][q] + 0.5
                if 0 <= tu <= 1 and 0 <= tv <= 1 and 0 <= int(tu * ps) < ps and 0 <= int(tv * ps) < ps:
                    want[p, edge, i] = q * ps * ps + int(tv * ps) * ps + int(tu * ps)
    np.testing.assert_array_equal(got, want)
    assert (got != NULL).any()
    # the same plates without the callback: another table
    ctx.set_globe_plates(ctx.globe())
    plain = ctx.read_seam_table()
    np.testing.assert_array_equal(plain, M.seam_table(M.head_of(ctx)))
    assert (plain != got).any()
    ctx.close()


# ---- 3. life cycle ------------------------------------------------------------------------------------------------------------------------
def marked(ctx):
    """set a table that no computation gives (all NULL) and return it"""
    ps = ctx.size()[2]
    t = np.full((6, 4, ps + 2), NULL, np.uint32)
    ctx.set_seam_table(t)
    return t


def test_kept_and_dropped(bk):
    ctx = host_ctx(bk, "cube", (40, 12))
    computed = ctx.read_seam_table().copy()
    assert (computed != NULL).any()
    t = marked(ctx)
    np.testing.assert_array_equal(ctx.read_seam_table(), t)                      # round trip
    ctx.set_rows(2, 7)
    ctx.host_build(1)                                                          # a build on this context's only path
    np.testing.assert_array_equal(ctx.read_seam_table(), t, err_msg="bk_set_rows / a build dropped it")
    ctx.set_rows(0, 12)
    drops = {"bk_load_globe": lambda: ctx.load_globe(S.script("globes", "cube"), "cube.lua"),
             "bk_set_globe_plates": lambda: ctx.set_globe_plates(ctx.globe()),
             "bk_load_lens": lambda: ctx.load_lens(SM.FLAT_LENS, "lens.lua"),
             "bk_clear_lens": lambda: ctx.clear_lens(),                  # (alone: the table needs no lens, and bk_load_lens drops it itself)
             "bk_resize": lambda: (ctx.resize(41, 12), ctx.resize(40, 12))}
    for name, call in drops.items():
        marked(ctx)
        call()
        np.testing.assert_array_equal(ctx.read_seam_table(), computed, err_msg=f"{name} kept a table that was set")
    marked(ctx)
    ctx.clear_globe()
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*globe"):
        ctx.read_seam_table()
    ctx.close()
    empty = bk.Context(bk.ffi.DEVICE_NONE)
    empty.load_globe(S.script("globes", "cube"), "cube.lua")
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        empty.read_seam_table()                                                   # no size
    empty.close()


def test_bk_build_on_a_device_less_context_is_not_needed_for_the_table(bk):
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")                      # no lens at all
    ctx.resize(40, 12)
    T = ctx.read_seam_table()
    assert T.shape == (6, 4, 14) and (T[:, :, 1:-1] != NULL).all()
    ctx.close()


def test_set_rejects_an_entry_out_of_range_and_a_torn_corner(bk):
    ctx = host_ctx(bk, "cube", (40, 12))
    good = ctx.read_seam_table().copy()
    ctx.set_seam_table(good)
    bad = good.copy()
    bad[3, 2, 5] = 6 * 12 * 12
    with pytest.raises(bk.BlinkyError, match=r"\[-1\].*neither NULL"):
        ctx.set_seam_table(bad)
    for (e0, i0), (e1, i1) in (((0, 0), (2, 0)), ((0, -1), (3, 0)), ((1, 0), (2, -1)), ((1, -1), (3, -1))):
        torn = good.copy()
        torn[4, e0, i0], torn[4, e1, i1] = 7, 8
        with pytest.raises(bk.BlinkyError, match=r"\[-1\].*corner"):
            ctx.set_seam_table(torn)
        torn[4, e1, i1] = 7
        ctx.set_seam_table(torn)
    np.testing.assert_array_equal(ctx.read_seam_table(), torn)
    ctx.close()


# ---- 4. the two frame models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_numpy_frame_is_the_loops(seed):
    import test_apply_rgba_fb_seams_gpu as GPU
    rng = np.random.default_rng(8800 + seed)
    W, H = 13, 5 + seed
    ps = min(W, H)
    table, sub = GPU.rim_case(W, H, seed)
    off, tints = table[0], table[1]
    seams = GPU.drawn_seams(ps, seed)
    plates = rng.integers(0, 256, (6, ps, ps, 4)).astype(np.uint8)
    lut = rng.integers(0, 256, (4, 6, 256)).astype(np.uint8)
    for given in ((True,) * 6, (True, False, True, True, False, True)):
        for l in (None, lut):
            a = M.seam_frame(plates, off, sub, tints, W, H, ps, (1, H), l, np.full((H + 2, 4 * W + 12), 77, np.uint8), 1, 2, seams, given)
            b = M.seam_frame_loops(plates, off, sub, tints, W, H, ps, (1, H), l, np.full((H + 2, 4 * W + 12), 77, np.uint8), 1, 2, seams, given)
            np.testing.assert_array_equal(a, b)
    # an all-NULL table is the clamped frame; a plane of centres the nearest texel whatever the table holds
    none = np.full((6, 4, ps + 2), NULL, np.uint32)
    a = M.seam_frame(plates, off, sub, tints, W, H, ps, (0, H), lut, np.full((H, 4 * W), 77, np.uint8), 0, 0, none)
    b = SM.bilinear_frame(plates, off, sub, tints, W, H, ps, (0, H), lut, np.full((H, 4 * W), 77, np.uint8), 0, 0)
    np.testing.assert_array_equal(a, b)
    centre = np.full(W * H, SM.CENTRE, np.uint16)
    a = M.seam_frame(plates, off, centre, tints, W, H, ps, (0, H), lut, np.full((H, 4 * W), 77, np.uint8), 0, 0, seams)
    b = SM.bilinear_frame(plates, off, centre, tints, W, H, ps, (0, H), lut, np.full((H, 4 * W), 77, np.uint8), 0, 0)
    np.testing.assert_array_equal(a, b)


# ---- 5. what it is for ------------------------------------------------------------------------------------------------------------------------
def smooth(ray):
    """a smooth function of a unit ray, four bytes"""
    x, y, z = ray
    f = [0.5 + 0.5 * np.sin(3 * x + 2 * y), 0.5 + 0.5 * np.cos(2 * z - 3 * y + 1), 0.5 + 0.4 * x * y + 0.1 * z, 0.5 + 0.5 * np.sin(4 * z + x)]
    return np.stack([np.clip(np.rint(255 * c), 0, 255) for c in f], -1).astype(np.uint8)


@pytest.mark.parametrize("lens,size", [("flat", (96, 64)), ("sheared", (131, 77))])
def test_the_seam_frame_is_nearer_the_truth_than_the_clamped_one(bk, lens, size):
    W, H = size
    ctx = host_ctx(bk, "cube", size, SM.LIBM_FREE[lens])
    head = M.head_of(ctx)
    ps = head["ps"]
    off, sub = SM.plane_model(head, SM.RAYS[lens])
    seams = ctx.read_seam_table()
    ctx.close()
    # plates: the function at every texel's own ray
    yy, xx = np.meshgrid(np.arange(ps), np.arange(ps), indexing="ij")
    plates = np.stack([smooth([r.astype(np.float64) for r in M._plate_uv_to_ray(head, p, (xx + 0.5) / ps, (yy + 0.5) / ps)]) for p in range(6)])
    # the truth: the function at every pixel's own (normalised) ray
    ly, lx = np.divmod(np.arange(W * H), W)
    r = [np.asarray(c, np.float64) for c in SM.RAYS[lens]((lx - W // 2) * head["scale"], -(ly - H // 2) * head["scale"])]
    norm = np.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)
    truth = smooth([c / norm for c in r]).astype(np.int64).reshape(H, W, 4)
    tints = np.full(W * H, 255, np.uint8)
    frame = lambda f, *more: f(plates, off, sub, tints, W, H, ps, (0, H), None, np.zeros((H, 4 * W), np.uint8), 0, 0, *more).reshape(H, W, 4)
    clamped, seamed = frame(SM.bilinear_frame).astype(np.int64), frame(M.seam_frame, seams).astype(np.int64)
    # the pixels with an out-of-plate neighbour: those whose texel lies on its plate's first or last row or column (the 3 x 3 window of
    # the read contract leaves the plate); `blended` of them have one of their four positions outside, the others come out the same
    idx = np.where(off != NULL, off, 0).astype(np.int64) % (ps * ps)
    rim = ((off != NULL) & ((idx // ps == 0) | (idx // ps == ps - 1) | (idx % ps == 0) | (idx % ps == ps - 1))).reshape(H, W)
    _, _, _, resolved, _, _ = M.positions(off, sub, ps, np.zeros((6, 4, ps + 2), np.uint32))      # (any non-NULL table: which positions lie outside)
    blended = (resolved.any(0) & (off != NULL)).reshape(H, W)
    assert (rim | ~blended).all() and blended.sum() > 0
    print(f"{lens} {size}: {blended.sum()} of the rim pixels have a position outside")
    assert rim.sum() >= 100
    err_clamped, err_seamed = np.abs(clamped - truth)[rim].sum(), np.abs(seamed - truth)[rim].sum()
    print(f"{lens} {size}: {rim.sum()} rim pixels, summed |error| clamped {err_clamped}, seam table {err_seamed}")
    assert err_seamed < err_clamped
    assert (clamped[~rim] == seamed[~rim]).all()


# ---- 6. the census of the GPU cases -----------------------------------------------------------------------------------------------------------
def test_census_of_the_committed_gpu_cases():
    import test_apply_rgba_fb_seams_gpu as GPU
    edges, corners, resolved_counts, tints_seen, qx, qy = set(), {"NULL": 0, "set": 0}, set(), set(), set(), set()
    null_plate_target = null_in_lane = False
    for table, sub, seams, given in GPU.committed_cases():
        off, tints, W, H, ps = table
        off, sub = np.asarray(off), np.asarray(sub)
        m = off != NULL
        P, Y, X, R, fx, fy = M.positions(off, sub, ps, seams, given)
        P0, Y0, X0, R0, _, _ = M.positions(off, sub, ps, np.zeros((6, 4, ps + 2), np.uint32))      # R0: the position lies outside
        R, R0 = R & m, R0 & m
        resolved_counts |= set(np.unique(R.sum(0)[m]).tolist())
        T = np.asarray(seams, np.uint32).reshape(6, 4, ps + 2)
        idx = np.where(m, off, 0).astype(np.int64)
        plate, py, px = idx // (ps * ps), idx % (ps * ps) // ps, idx % ps
        s = sub.astype(np.int64)
        xa, ya = px - 1 + (((s & 255) + 128) >> 8), py - 1 + (((s >> 8) + 128) >> 8)
        for j, (yn, xn) in enumerate(((ya, xa), (ya, xa + 1), (ya + 1, xa), (ya + 1, xa + 1))):
            for k in np.flatnonzero(R0[j]):
                edge, i = M.slot(ps, int(xn[k]), int(yn[k]))
                E = int(T[plate[k], edge, i])
                if i in (0, ps + 1):
                    corners["NULL" if E == NULL else "set"] += 1
                    edges.add(("corner", edge, i == 0))
                else:
                    edges.add(edge)
                if E != NULL and not given[E // (ps * ps)]:
                    null_plate_target = True
        tints_seen |= set(np.asarray(tints)[m].tolist())
        qx |= set((sub[m] & 255).tolist())
        qy |= set((sub[m] >> 8).tolist())
        if W >= 4:
            lanes = off[: H * W].reshape(H, W)[:, : W // 4 * 4].reshape(H, W // 4, 4)
            null_in_lane |= bool((((lanes == NULL).sum(-1) > 0) & ((lanes != NULL).sum(-1) > 0)).any())
    assert {0, 1, 2, 3} <= edges
    assert {("corner", e, first) for e in (0, 1) for first in (True, False)} <= edges, "a corner no case reaches"
    assert corners["NULL"] > 0 and corners["set"] > 0
    # (one, two and three: the named texel is always one of the four positions - xa is px - 1 or px - so a fourth cannot lie outside)
    assert {1, 2, 3} <= resolved_counts and 4 not in resolved_counts
    assert null_plate_target and null_in_lane
    assert {0, 1, 2, 3, 4, 5, 6, 200, 255} <= tints_seen
    assert {0, 127, 128, 255} <= qx and {0, 127, 128, 255} <= qy
