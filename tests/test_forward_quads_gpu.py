"""The forward build's QUAD PASS as a kernel (bk_forward_tiles, bk_forward_quads, bk_forward_resolve), exact for ANY corner table:
bk_debug_set_forward_corners puts a table of tests/quad_tables.py where the corner pass would have put its own, the oracle's
ok_forward_from_corners (the reference's quad loop, fisheye.c:2189-2202, over the same table) says what has to come out.  Every entry
of every table is compared - offsets and tints exactly, display and the verdict as the build campaign compares them - on the
one-submission path and pass by pass ("forward_careful"), whole and in stripes.  tests/test_forward_quads_cpu.py holds the tables to
their census and the oracle entry to the oracle's own forward build.

The hook bypasses the corner pass, so four generated lenses keep corners -> quads -> resolve together UNDER MAGNIFICATION (a texel on
3-15 pixels), which of the shipped lenses and campaign seeds only two reach."""
import re

import numpy as np
import pytest

import oracle_ffi as O
import quad_tables as Q
import scripts as S

pytestmark = pytest.mark.gpu

# gives the build its module and its scale; the table replaces what it would project
TRIVIAL_LENS = """
lens_width = 2
lens_height = 2
onload = "f_contain"
function lens_forward(x, y, z) return x, y end
"""


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


@pytest.fixture(scope="module")
def want():
    """the oracle's full table of every committed seed: computed once, shared, never written to"""
    out = {}
    for s in Q.COMMITTED:
        t = Q.table(s)
        lm = O.forward_from_corners(t.globe, t.W, t.H, t.grid, t.xy, t.ok)
        for a in (lm.offsets, lm.tints, t.xy, t.ok):
            a.setflags(write=False)
        out[s] = (t, lm)
    return out


@pytest.fixture
def careful(bk, request):
    """the process-wide "forward_careful" switch, put back whatever happens"""
    request.addfinalizer(lambda: bk.debug_set_option("forward_careful", 0))
    return lambda on: bk.debug_set_option("forward_careful", int(on))


def _context(bk, t, rows=None):
    ctx = bk.Context()
    ctx.load_globe(S.script("globes", t.globe), t.globe + ".lua")
    ctx.load_lens(TRIVIAL_LENS, "trivial.lua")
    ctx.set_zoom(*S.zoom_args("f_contain"))
    ctx.resize(t.W, t.H)
    ctx.set_rubixgrid(*t.grid)
    if rows:
        ctx.set_rows(*rows)
    return ctx


def _build_and_compare(ctx, t, lm, rows, cfg):
    """test_random_build_configuration's assertions, on a table"""
    r0, r1 = rows
    W, H = t.W, t.H
    display, scale = ctx.build()                                    # (raises when not built: from-corners tables always build)
    off, tin = ctx.read_lensmap()
    want_off = lm.offsets.reshape(H, W)[r0:r1].ravel()
    bad = np.flatnonzero(off != want_off)
    assert bad.size == 0, (f"{cfg}: {bad.size} of {off.size} offsets differ, first at (y, x) = {divmod(int(bad[0]), W)} (stripe row): "
                           f"{off[bad[0]]} != {want_off[bad[0]]}; fixups {ctx.last_build_fixups()}")
    np.testing.assert_array_equal(tin, lm.tints.reshape(H, W)[r0:r1].ravel(), err_msg=cfg)
    if (r0, r1) == (0, H):
        assert display[: lm.numplates] == lm.display, cfg
    else:
        assert all(d <= w for d, w in zip(display[: lm.numplates], lm.display)), cfg
    assert ctx.last_build_fixups() == (0, 0), cfg                   # no corner is flagged
    return off, tin


@pytest.mark.parametrize("path", ["one_submission", "careful"])
@pytest.mark.parametrize("seed", Q.COMMITTED)
def test_quad_pass_builds_the_oracle_table_of_any_corner_table(bk, want, careful, seed, path):
    t, lm = want[seed]
    careful(path == "careful")
    ps = min(t.W, t.H)
    parts = []
    for rows in t.rows:                                             # (a pair of stripes: two contexts)
        cfg = f"seed {seed} {path}: {t.globe} {t.W}x{t.H} grid {t.grid} rows {rows}: {t.kind}"
        ctx = _context(bk, t, rows)
        ctx.set_forward_corners(t.xy, t.ok)
        parts.append(_build_and_compare(ctx, t, lm, rows, cfg))
        taken, total = ctx.forward_tiles()
        assert total == Q.NPLATES[t.globe] * ((ps + 15) // 16) ** 2
        if path == "careful":
            assert taken == -1, cfg
        else:
            assert taken >= 0, cfg                                  # the shortcut's flags were used ...
            assert taken > 0 or not (t.globe == "cube" and ps >= 48), cfg      # ... and on a cube of three tiles a side some tile lies inside its plate's region
        ctx.close()
    if len(t.rows) == 2:                                            # the two stripes concatenate to the full table
        np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), lm.offsets)
        np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), lm.tints)


def _reload(ctx, t):
    ctx.load_globe(S.script("globes", t.globe), t.globe + ".lua")
    ctx.resize(t.W, t.H)
    ctx.set_rows(0, t.H)
    ctx.set_rubixgrid(*t.grid)
    ctx.set_forward_corners(t.xy, t.ok)


@pytest.mark.parametrize("path", ["one_submission", "careful"])
def test_one_context_through_six_tables_and_back(bk, want, careful, path):
    """the key planes, the tables per platesize and the tile flags are kept from one build to the next: sizes growing and shrinking,
    globes of 6, 5 and 4 plates, ending on the first table again"""
    careful(path == "careful")
    seeds = [0, 5, 14, 7, 19, 34, 0]
    assert len({(want[s][0].W, want[s][0].H) for s in seeds}) == 6 and len({want[s][0].globe for s in seeds}) == 4
    ctx = _context(bk, want[seeds[0]][0])
    for k, s in enumerate(seeds):
        t, lm = want[s]
        _reload(ctx, t)
        _build_and_compare(ctx, t, lm, (0, t.H), f"step {k} seed {s} {path}: {t.globe} {t.W}x{t.H}: {t.kind}")
    ctx.close()


def _trivial_map(bk, t):
    info_ctx = bk.Context(bk.ffi.DEVICE_NONE)
    info_ctx.load_globe(S.script("globes", t.globe), t.globe + ".lua")
    info_ctx.load_lens(TRIVIAL_LENS, "trivial.lua")
    info = info_ctx.lens_info()
    lm = O.lensmap_with_callbacks(t.globe, info, None, lambda x, y, z: (x, y), "f_contain", t.W, t.H)
    info_ctx.close()
    assert lm.built and lm.nonnull > 0
    return lm


def test_clearing_the_table_leaves_the_lens_its_own_map(bk, want):
    """with the table cleared the same context builds the trivial lens's own map - the hook leaves nothing behind - and the calls that
    change what the table was sized for (bk_resize, bk_load_globe, bk_set_globe_plates) clear it themselves"""
    t, lm = want[0]                                                 # cube, 131x48, the default grid (the one lensmap_with_callbacks has)
    assert t.globe == "cube" and t.grid == (10, 4.0, 1.0)
    own = _trivial_map(bk, t)
    ctx = _context(bk, t)

    def builds_its_own(what):
        display, scale = ctx.build()
        off, tin = ctx.read_lensmap()
        np.testing.assert_array_equal(off, own.offsets, err_msg=what)
        np.testing.assert_array_equal(tin, own.tints, err_msg=what)
        assert display[: own.numplates] == own.display and scale == own.scale, what

    builds_its_own("before any table")
    ctx.set_forward_corners(t.xy, t.ok)
    _build_and_compare(ctx, t, lm, (0, t.H), "table set")
    ctx.set_forward_corners(None, None)
    builds_its_own("cleared")
    ctx.set_forward_corners(t.xy, t.ok)
    ctx.resize(t.W, t.H)                                            # (even the size it has)
    builds_its_own("after bk_resize")
    ctx.set_forward_corners(t.xy, t.ok)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    builds_its_own("after bk_load_globe")
    ctx.set_forward_corners(t.xy, t.ok)
    ctx.set_globe_plates(ctx.globe())
    builds_its_own("after bk_set_globe_plates")
    ctx.set_forward_corners(t.xy, t.ok)
    _build_and_compare(ctx, t, lm, (0, t.H), "table set again")
    ctx.close()


def _fails(bk, ctx, code):
    with pytest.raises(bk.ffi.BlinkyError) as e:
        ctx.build()
    assert re.match(r"\[%d\]" % code, str(e.value)), str(e.value)
    return str(e.value)


def test_a_table_the_build_cannot_use_is_an_error(bk, want):
    """a test must not be able to pass while testing nothing: BK_E_INVALID (-1) for a table of the wrong size, BK_E_STATE (-6) for a
    build that does not go through the device's forward passes - over an empty map"""
    t, lm = want[3]                                                 # tetra, 16x16
    ctx = _context(bk, t)
    ctx.set_forward_corners(t.xy[:-1], t.ok[:-1])
    assert "bk_debug_set_forward_corners" in _fails(bk, ctx, -1)
    ctx.set_forward_corners(np.concatenate([t.xy, t.xy[:17]]), np.concatenate([t.ok, t.ok[:17]]))
    _fails(bk, ctx, -1)
    ctx.set_forward_corners(t.xy, t.ok)
    _build_and_compare(ctx, t, lm, (0, t.H), "the right size")
    # an inverse map
    ctx.load_lens("max_fov = 180\nlens_width = 2\nonload = \"f_contain\"\nfunction lens_inverse(x, y) return x, y, 1 end\n", "inverse.lua")
    assert "corner table" in _fails(bk, ctx, -6)
    off, tin = ctx.read_lensmap()
    assert (off == O.NULL).all() and (tin == 255).all()
    ctx.set_forward_corners(None, None)
    assert (ctx.read_lensmap()[0] == O.NULL).all() and ctx.build() and (ctx.read_lensmap()[0] != O.NULL).any()
    # a host path: the forward scan in the reference's order
    ctx.load_lens(TRIVIAL_LENS, "trivial.lua")
    ctx.set_forward_corners(t.xy, t.ok)
    ctx.set_sequential_build(2)
    _fails(bk, ctx, -6)
    assert (ctx.read_lensmap()[0] == O.NULL).all()
    ctx.set_sequential_build(1)
    _build_and_compare(ctx, t, lm, (0, t.H), "back on the device")
    ctx.close()
    # a device-less context builds nothing at all
    host = bk.Context(bk.ffi.DEVICE_NONE)
    host.load_globe(S.script("globes", t.globe), t.globe + ".lua")
    host.load_lens(TRIVIAL_LENS, "trivial.lua")
    host.resize(t.W, t.H)
    host.set_forward_corners(t.xy, t.ok)
    _fails(bk, host, -6)
    host.close()


# ---- corners -> quads -> resolve in one submission, magnified ---------------------------------------------------------------------
GNOMONIC = """
lens_width = %(width)r
onload = "f_contain"
function lens_forward(x, y, z)
  if z <= 0 then return nil end
  local u, v = %(k)r * x / z, %(k)r * y / z
  return %(a)r * u + %(b)r * v, %(c)r * u + %(d)r * v
end
"""
# gnomonic x/z, y/z times 3, times 12, rotated by 30 degrees, mirrored.  A texel at the middle of the front plate is 2 k / platesize lens
# units wide and a pixel lens_width / W, so it spans 2 k W / (platesize lens_width) pixels - 3 k / lens_width at 72x48, 2 k / lens_width at
# 48x131, more towards the plate's edges: 9 and 6, 14.4 and 9.6, 4.5 and 3, 12 and 8 pixels for the four lenses (`span`, checked
# against the corners the lens projects)
MAGNIFIED = {
    "times3": dict(k=3.0, width=1.0, a=1.0, b=0.0, c=0.0, d=1.0),
    "times12": dict(k=12.0, width=2.5, a=1.0, b=0.0, c=0.0, d=1.0),
    "rotated30": dict(k=3.0, width=2.0, a=0.8660254037844386, b=-0.5, c=0.5, d=0.8660254037844386),
    "mirrored": dict(k=3.0, width=0.75, a=-1.0, b=0.0, c=0.0, d=1.0),
}


def _front_plate_quads(host, W, H):
    """from the corners the lens projects (the host's interpreter, bk_debug_host_corners): the pixels between neighbouring corners at the
    middle of the front plate, and how many of that plate's quads the size check accepts on the screen on three rows or more"""
    ps = min(W, H)
    n1 = ps + 1
    sx, sy, ok = host.host_corners(np.arange(n1 * n1, dtype=np.uint32))
    x, y, ok = sx.reshape(n1, n1).astype(np.int64), sy.reshape(n1, n1).astype(np.int64), ok.reshape(n1, n1).astype(bool)
    m = ps // 2
    span = float(np.hypot(x[m, m + 4] - x[m, m - 4], y[m, m + 4] - y[m, m - 4])) / 8
    c = np.stack([np.stack([x[:-1, :-1], x[:-1, 1:], x[1:, :-1], x[1:, 1:]]), np.stack([y[:-1, :-1], y[:-1, 1:], y[1:, :-1], y[1:, 1:]])])
    ok4 = ok[:-1, :-1] & ok[:-1, 1:] & ok[1:, :-1] & ok[1:, 1:]
    lo, hi = c.min(1), c.max(1)
    on = ok4 & (hi[0] >= 0) & (lo[0] < W) & (hi[1] >= 0) & (lo[1] < H) & (hi[0] - lo[0] <= Q.MAXDIFF) & (hi[1] - lo[1] <= Q.MAXDIFF)
    return span, int((on & (hi[1] - lo[1] >= 2)).sum())
_magnified_want = {}


def _magnified_oracle(bk, name, W, H):
    """O.lensmap_with_callbacks on the host interpreter's callbacks and the portable libm, as test_script_fuzz_gpu's
    _builds_the_oracle_table has it; once per lens and size"""
    if (name, W, H) not in _magnified_want:
        src = GNOMONIC % MAGNIFIED[name]
        host = bk.Context(bk.ffi.DEVICE_NONE)
        host.set_host_math(True)
        host.load_globe(S.script("globes", "cube"), "cube.lua")
        host.load_lens(src, name + ".lua")
        host.resize(W, H)
        info = host.lens_info()
        host.set_zoom(*S.zoom_args(info.onload.decode()))
        lm = O.lensmap_with_callbacks("cube", info, None, lambda x, y, z: host.eval_host(1, x, y, z), info.onload.decode(), W, H, portable=True)
        span, tall = _front_plate_quads(host, W, H)
        host.close()
        lm.offsets.setflags(write=False)
        lm.tints.setflags(write=False)
        _magnified_want[(name, W, H)] = (src, info.onload.decode(), lm, span, tall)
    return _magnified_want[(name, W, H)]


@pytest.mark.parametrize("stripe", [False, True], ids=["full", "stripe"])
@pytest.mark.parametrize("size", [(72, 48), (48, 131)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(MAGNIFIED))
def test_magnifying_lens_through_the_whole_forward_build(bk, name, size, stripe):
    W, H = size
    src, onload, lm, span, tall = _magnified_oracle(bk, name, W, H)
    assert lm.built and lm.nonnull > W * H // 4, name
    p = MAGNIFIED[name]
    assert abs(span - 2 * p["k"] * W / (min(W, H) * p["width"])) < 0.5 and 3 <= span <= 15, (name, span)      # the magnification meant ...
    assert tall >= 20, (name, tall)                                 # ... and the general scanline of draw_quad at work: quads of three rows and more
    r0, r1 = (H // 3 + 1, 2 * H // 3 + 3) if stripe else (0, H)
    ctx = bk.Context()
    ctx.set_host_math(True)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(src, name + ".lua")
    ctx.set_zoom(*S.zoom_args(onload))
    ctx.resize(W, H)
    ctx.set_rows(r0, r1)
    display, scale = ctx.build()
    off, tin = ctx.read_lensmap()
    assert scale == lm.scale
    bad = int((off != lm.offsets.reshape(H, W)[r0:r1].ravel()).sum())
    assert bad == 0, f"{name} {W}x{H} rows [{r0},{r1}): {bad} of {off.size} entries differ\n{src}"
    np.testing.assert_array_equal(tin, lm.tints.reshape(H, W)[r0:r1].ravel())
    if not stripe:
        assert display[: lm.numplates] == lm.display
    else:
        assert all(d <= w for d, w in zip(display[: lm.numplates], lm.display))
    assert ctx.last_build_path()[0] == 0                            # the GPU kernels
    ctx.close()
