"""The sub-texel plane and the bilinear frame without a GPU: the two models of tests/subtexel_model.py against each other, the plane
model against the host build paths (bk_debug_host_build_subtexel on a device-less context), the plane's properties on lenses that do use
libm, and the two CONDITIONS the GPU tests rest on - the census of their committed cases and the flagged configuration."""
import os
import sys

import numpy as np
import pytest

import rgba_fb_model as M
import scripts as S
import subtexel_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
NULL = SM.NULL
SIZE = (203, 131)                                                  # ps 131: gp 192, ph 136
STRIPE = (37, 90)
# a lens the GPU emitter declines (tests/test_host_path_gpu.py): hammer with its values parked in a table whose keys exist at run time only.
# (Every lens under examples/lenses is emitted as it stands - test_build_gpu.py builds all four on the device - so the declined one is
# this; examples/lenses/integrated_arc.lua stands in for the directory.)
RUNTIME_TABLE = """
local straight = lens_inverse
function lens_inverse(x, y)
   local t = {}
   t[x > 0 and "east" or "west"] = x
   t["y" .. ""] = y
   local pick = function(tab, k) return tab[k] end
   return straight(pick(t, "east") or pick(t, "west"), pick(t, "y"))
end
"""
# the configuration whose build the DEVICE code flags pixels of (chosen with emu.build_inverse): cube / quincuncial at 203 x 131 flags 207
FLAGGED_CASE = ("cube", "quincuncial", SIZE)
FLAGGED_COUNT = 207


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def lens_source(name):
    if name in SM.LIBM_FREE:
        return SM.LIBM_FREE[name]
    if name == "declined-hammer":
        return S.script("lenses", "hammer") + RUNTIME_TABLE
    if name == "integrated_arc":
        return open(os.path.join(os.path.dirname(HERE), "examples", "lenses", name + ".lua")).read()
    return S.script("lenses", name)


def host_ctx(bk, lens, size=SIZE, rows=None, device=None):
    ctx = bk.Context(bk.ffi.DEVICE_NONE) if device is None else bk.Context()
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(lens_source(lens), lens + ".lua")
    ctx.set_zoom(*S.zoom_args(ctx.lens_info().onload.decode()))
    ctx.resize(*size)
    if rows:
        ctx.set_rows(*rows)
    return ctx


# ---- 1. the bilinear frame: two formulations ---------------------------------------------------------------------------------------
def small_case(seed):
    rng = np.random.default_rng(8000 + seed)
    W, H = int(rng.integers(1, 14)), int(rng.integers(1, 10))
    ps = min(W, H)
    n = W * H
    off = (rng.integers(0, 6, n) * ps * ps + rng.integers(0, ps, n) * ps + rng.integers(0, ps, n)).astype(np.uint32)
    off[rng.random(n) < 0.2] = NULL
    edge = np.array([0, 127, 128, 255])
    axis = lambda: np.where(rng.random(n) < 0.5, edge[rng.integers(0, 4, n)], rng.integers(0, 256, n))
    sub = (axis() | (axis() << 8)).astype(np.uint16)
    tints = np.array([0, 1, 2, 3, 4, 5, 6, 200, 255], np.uint8)[rng.integers(0, 9, n)]
    plates = rng.integers(0, 256, (6, ps, ps, 4)).astype(np.uint8)
    lut = rng.integers(0, 256, (4, 6, 256)).astype(np.uint8)
    return W, H, ps, off, sub, tints, plates, lut


@pytest.mark.parametrize("seed", range(12))
def test_the_numpy_frame_is_the_written_out_weights(seed):
    W, H, ps, off, sub, tints, plates, lut = small_case(seed)
    rows = (0, H) if seed % 3 else (H // 3, H)
    for table in (None, lut):
        a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
        b = a.copy()
        SM.bilinear_frame(plates, off, sub, tints, W, H, ps, rows, table, a, 2, 1)
        SM.bilinear_frame_loops(plates, off, sub, tints, W, H, ps, rows, table, b, 2, 1)
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("seed", range(4))
def test_a_plane_of_centres_is_the_nearest_frame_and_a_constant_plate_its_constant(seed):
    W, H, ps, off, sub, tints, plates, lut = small_case(20 + seed)
    for table in (None, lut):
        a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
        b = a.copy()
        SM.bilinear_frame(plates, off, np.full(W * H, SM.CENTRE, np.uint16), tints, W, H, ps, (0, H), table, a, 2, 1)
        M.fb_frame(plates, off, tints, W, H, ps, (0, H), table, False, b, 2, 1)
        np.testing.assert_array_equal(a, b)
    flat = np.empty_like(plates)
    flat[...] = plates[:, :1, :1, :]
    a = np.full((H + 3, 4 * (W + 5)), 77, np.uint8)
    b = a.copy()
    SM.bilinear_frame(flat, off, sub, tints, W, H, ps, (0, H), None, a, 2, 1)
    M.fb_frame(flat, off, tints, W, H, ps, (0, H), None, False, b, 2, 1)
    np.testing.assert_array_equal(a, b)


def test_tint_before_the_blend_is_not_tint_after_it():
    """the LUTs the GPU tests use are not monotone: tinting the blended value would give another frame"""
    W, H, ps, off, sub, tints, plates, lut = small_case(3)
    before = np.full((H, 4 * W), 77, np.uint8)
    SM.bilinear_frame(plates, off, sub, tints, W, H, ps, (0, H), lut, before, 0, 0)
    plain = np.full((H, 4 * W), 77, np.uint8)
    SM.bilinear_frame(plates, off, sub, tints, W, H, ps, (0, H), None, plain, 0, 0)
    t = np.repeat(tints.reshape(H, W).astype(np.int64), 4, axis=1)
    c = np.tile(np.arange(4), W)[None, :].repeat(H, axis=0)
    after = np.where(t < 6, lut[c, np.where(t < 6, t, 0), plain], plain)
    mapped = np.repeat((off != NULL).reshape(H, W), 4, axis=1)
    assert (after[mapped] != before[mapped]).any()


# ---- 2. the plane model against the host build paths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [None, STRIPE], ids=["full", "stripe"])
@pytest.mark.parametrize("mode", [1, 2], ids=["pool", "sequential"])
@pytest.mark.parametrize("lens", sorted(SM.LIBM_FREE))
def test_plane_model_is_the_host_build(bk, lens, mode, rows):
    ctx = host_ctx(bk, lens, rows=rows)
    off, tin, sub, display, scale, err = ctx.host_build_subtexel(mode)
    assert err is None
    head = SM.build_params_head(ctx)
    assert head["scale"] == scale and (head["row0"], head["rows"]) == ((rows or (0, SIZE[1]))[0], (rows or (0, SIZE[1]))[1] - (rows or (0, SIZE[1]))[0])
    want_off, want_sub = SM.plane_model(head, SM.RAYS[lens])
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(sub, want_sub)
    mapped = off != NULL
    assert mapped.sum() > off.size // 2 and len(np.unique(sub[mapped])) > 2000      # (a plane, not a constant)
    ctx.close()


# ---- 3. properties on lenses that do use libm --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,size", [("panini", SIZE), ("hammer", SIZE), ("quincuncial", SIZE), ("winkel2", (96, 64)), ("declined-hammer", SIZE),
                                       ("integrated_arc", (160, 100))])
def test_plane_properties_through_the_host_paths(bk, lens, size, monkeypatch):
    monkeypatch.chdir(os.path.dirname(HERE))                        # (the examples' paths are relative to the repository root)
    ctx = host_ctx(bk, lens, size)
    forward = lens == "winkel2"
    assert (ctx.lens_info().map_type == bk.ffi.MAP_FORWARD) == forward
    results = {}
    for mode in (1, 2):
        off0, tin0, display0, scale0, err0 = ctx.host_build(mode)
        off, tin, sub, display, scale, err = ctx.host_build_subtexel(mode)
        assert err is None and err0 is None and display == display0 and scale == scale0
        np.testing.assert_array_equal(off, off0)
        np.testing.assert_array_equal(tin, tin0)
        mapped = off != NULL
        assert mapped.any() and (sub[~mapped] == SM.CENTRE).all()
        if forward:
            assert (sub == SM.CENTRE).all()
        else:
            assert len(np.unique(sub[mapped])) > 1000
        results[mode] = sub
    np.testing.assert_array_equal(results[1], results[2])
    ctx.close()


# ---- 4. the conditions the GPU tests rest on -------------------------------------------------------------------------------------------
def test_census_of_the_committed_apply_cases():
    """tests/test_apply_rgba_fb_bilinear_gpu.py's drawn cases reach: qx and qy each of 0, 127, 128, 255; px = 0 and px = ps - 1 (py
    alike) with the neighbour clamped on each of the four sides; a NULL beside a mapped pixel inside a lane's four; tints 0..5, 6, 200, 255"""
    import test_apply_rgba_fb_bilinear_gpu as T
    qx, qy, tint_values = set(), set(), set()
    clamped = dict(left=0, right=0, top=0, bottom=0)
    null_in_lane = 0
    for (off, tints, W, H, ps), sub in T.committed_cases():
        off, sub, tints = np.asarray(off), np.asarray(sub), np.asarray(tints)
        assert off.shape == sub.shape == tints.shape == (W * H,)
        m = off != NULL
        assert (off[m] < 6 * ps * ps).all()
        qx |= set((sub[m] & 255).tolist())
        qy |= set((sub[m] >> 8).tolist())
        tint_values |= set(tints[m].tolist())
        rem = off[m].astype(np.int64) % (ps * ps)
        px, py = rem % ps, rem // ps
        sx, sy = (sub[m].astype(np.int64) & 255) + 128, (sub[m].astype(np.int64) >> 8) + 128
        if ps > 1:
            clamped["left"] += int(((px == 0) & (sx < 256)).sum())
            clamped["right"] += int(((px == ps - 1) & (sx >= 256) & ((sx & 255) > 0)).sum())
            clamped["top"] += int(((py == 0) & (sy < 256)).sum())
            clamped["bottom"] += int(((py == ps - 1) & (sy >= 256) & ((sy & 255) > 0)).sum())
        grid = m.reshape(H, W)
        for x in range(0, W - W % 4, 4):
            lane = grid[:, x:x + 4].sum(axis=1)
            null_in_lane += int(((lane > 0) & (lane < 4)).sum())
    assert {0, 127, 128, 255} <= qx and {0, 127, 128, 255} <= qy
    assert all(v > 0 for v in clamped.values()), clamped
    assert null_in_lane > 0
    assert {0, 1, 2, 3, 4, 5, 6, 200, 255} <= tint_values


def test_the_flagged_configuration_still_flags(bk):
    """the GPU tests hold the plane of FLAGGED_CASE to the host build bit for bit, fix-ups included; that says something only while the
    device code does flag pixels there.  Chosen with emu.build_inverse: cube / quincuncial at 203 x 131 flags 207 pixels."""
    sys.path.insert(0, os.path.join(HERE, "hostemu"))
    import emu
    globe, lens, size = FLAGGED_CASE
    ctx = bk.Context(bk.ffi.DEVICE_NONE)
    S.configure(ctx, globe, lens, None, size)
    off, tin, flagged, err = emu.build_inverse(ctx)                 # (a context with the switch off: the generated kernel tolerates subtexel == NULL)
    ctx.close()
    print(f"{lens} {size}: {len(flagged)} flagged (recorded: {FLAGGED_COUNT})")
    assert err == 0 and len(flagged) >= 1
