"""The exactness bookkeeping of the generated build code (blinky_amd/csrc/bk_device_rt.h), checked WITHOUT a GPU:
tests/hostemu compiles the very translation unit hiprtc gets as host C++ and runs the inverse build kernel serially.

What must hold: wherever the table built on the portable libm (what the device computes) differs from the table
the reference computes on the platform libm, the device code has FLAGGED that pixel - so the host fix-up
(bk_build.cpp) re-derives it and the final table is the reference's.  And the flagged set stays small."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hostemu"))

import emu              # noqa: E402
import oracle_ffi as O  # noqa: E402
import scripts as S     # noqa: E402


def emu_build(globe, lens, zoom, W, H):
    import blinky_amd
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    S.configure(ctx, globe, lens, zoom, (W, H))
    off, tin, flagged, err = emu.build_inverse(ctx)
    ctx.close()
    assert err == 0
    return emu.device_to_reference_layout(off, min(W, H)), tin, flagged


@pytest.mark.parametrize("cfg", [
    ("cube", "quincuncial", None, 1920, 1080),     # the size at which one exact tie separates glibc from any other libm
    ("cube", "quincuncial", None, 640, 480),
    ("cube", "stereographic", None, 960, 540),
    ("cube", "hammer", None, 960, 540),
    ("trism", "panini", None, 640, 360),
    ("cube", "winkeltripel", None, 640, 400),      # Newton iteration with `break`: comparisons against eps
    ("cube", "mollweide", None, 640, 320),
    ("cube", "eckert4", None, 400, 200),           # 20 Newton steps: the bounds blow up near the poles (many flags)
    ("cube", "cubestereo", None, 400, 250),
    ("cube", "fisheye1", None, 320, 320),
    ("cube", "miller", None, 400, 300),
    ("cube", "debug", None, 300, 200),             # plate_to_ray: u, v narrowed to float
    ("tetra", "panini", None, 320, 200),
    ("fast", "panini", "f_fov 200", 320, 200),     # globe_plate override: comparisons on u, v
    ("cube", "cube", None, 320, 240),              # math.modf on the cell coordinates
    ("cube", "fahey", None, 400, 250),
    ("cube", "fisheye2", None, 300, 300),
    ("cube", "gallstereo", None, 400, 250),
    ("cube", "gumby", None, 400, 250),
    ("cube", "vandergrinten", None, 360, 360),     # cubic solved with acos / cos, many comparisons against TOL
    ("cube_corner", "stereographic", None, 320, 200),
    ("cube_edge", "rectilinear", None, 320, 200),
])
def test_every_libm_dependent_pixel_is_flagged(cfg):
    globe, lens, zoom, W, H = cfg
    off, tin, flagged = emu_build(globe, lens, zoom, W, H)
    portable = O.lensmap(globe, lens, zoom, W, H, portable=True)
    platform = O.lensmap(globe, lens, zoom, W, H)
    # the generated code IS the portable-libm oracle, entry for entry
    np.testing.assert_array_equal(off, portable.offsets)
    np.testing.assert_array_equal(tin, portable.tints)
    # and every entry the platform libm decides differently has been flagged for the host
    differs = np.nonzero((platform.offsets != off) | (platform.tints != tin))[0]
    assert set(differs.tolist()) <= set(flagged.tolist()), f"{len(differs)} differing entries, not all flagged"
    if (lens, W) == ("quincuncial", 1920):
        assert len(differs) >= 1          # (the case DESIGN.md section 5 describes; it is why the fix-up exists)
    if lens != "eckert4":
        assert len(flagged) <= max(64, 8 * (W + H)), len(flagged)     # lines of symmetry at most, never areas


@pytest.mark.parametrize("lens", [l for l in S.LENSES if l not in ("eckert4",)])
def test_flagged_set_is_small_for_every_inverse_lens(lens):
    import blinky_amd
    W, H = 320, 240
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    info = S.configure(ctx, "cube", lens, None, (W, H))
    if not info.has_inverse or info.map_type != blinky_amd.ffi.MAP_INVERSE:
        ctx.close()
        pytest.skip("forward-map lens")
    off, tin, flagged, err = emu.build_inverse(ctx)
    ctx.close()
    assert err == 0
    assert len(flagged) <= 8 * (W + H), f"{lens}: {len(flagged)} of {W * H} pixels flagged"


def test_platform_libm_is_within_the_assumed_bound_of_bkm():
    """BK_LIBM_REL (2^-50): the bound the bookkeeping assumes between bkm.h and the platform libm, sampled."""
    import ctypes as C
    import math
    lib = C.CDLL(os.path.join(os.path.dirname(HERE), "blinky_amd", "libbkm_host.so"))
    rng = np.random.default_rng(11)
    cases = {
        "sin": (math.sin, rng.uniform(-20, 20, 20000)), "cos": (math.cos, rng.uniform(-20, 20, 20000)),
        "tan": (math.tan, rng.uniform(-1.5, 1.5, 20000)), "asin": (math.asin, rng.uniform(-1, 1, 20000)),
        "acos": (math.acos, rng.uniform(-1, 1, 20000)), "atan": (math.atan, rng.uniform(-50, 50, 20000)),
        "exp": (math.exp, rng.uniform(-20, 20, 20000)), "log": (math.log, rng.uniform(1e-6, 1e3, 20000)),
        "sinh": (math.sinh, rng.uniform(-10, 10, 20000)), "cosh": (math.cosh, rng.uniform(-10, 10, 20000)),
        "tanh": (math.tanh, rng.uniform(-5, 5, 20000)), "log10": (math.log10, rng.uniform(1e-6, 1e3, 20000)),
    }
    two = {"atan2": (math.atan2, rng.uniform(-5, 5, 20000), rng.uniform(-5, 5, 20000)),
           "pow": (math.pow, rng.uniform(0.01, 20, 20000), rng.uniform(-6, 6, 20000))}
    for name, (ref, xs, ys) in two.items():
        fn = getattr(lib, "bkmh_" + name)
        fn.restype, fn.argtypes = C.c_double, [C.c_double, C.c_double]
        worst = max(abs(fn(float(x), float(y)) - ref(float(x), float(y))) / abs(ref(float(x), float(y))) for x, y in zip(xs, ys))
        assert worst <= 2.0 ** -50, (name, worst)
    for name, (ref, xs) in cases.items():
        fn = getattr(lib, "bkmh_" + name)
        fn.restype, fn.argtypes = C.c_double, [C.c_double]
        worst = 0.0
        for x in xs:
            a, b = fn(float(x)), ref(float(x))
            if b != 0:
                worst = max(worst, abs(a - b) / abs(b))
        assert worst <= 2.0 ** -50, (name, worst)


@pytest.mark.parametrize("seed", [s for s in range(40) if s % 3 != 2])
def test_random_scripts_every_libm_dependent_pixel_is_flagged(seed):
    """The same on random lens scripts (the generator of tests/test_script_fuzz_gpu.py: operator soup, loops, tables, script
    functions, comparisons everywhere): the generated code equals the fisheye.c restatement fed by the interpreter on the
    PORTABLE libm, and wherever the interpreter on the PLATFORM libm decides an entry differently, the code flagged it."""
    import blinky_amd
    from test_script_fuzz_gpu import Gen
    W, H = 96, 64
    src = Gen(5000 + seed).script(False).replace('onload = "f_fov 90"', 'lens_width = 5\nlens_height = 3.5\nonload = "f_contain"')

    def host(portable):
        c = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
        c.set_host_math(portable)
        c.load_globe(S.script("globes", "cube"), "cube.lua")
        c.load_lens(src, f"fuzz{seed}.lua")
        c.set_zoom(blinky_amd.ffi.ZOOM_CONTAIN)
        c.resize(W, H)
        return c

    tables = {}
    for portable in (True, False):
        c = host(portable)
        info = c.lens_info()
        tables[portable] = O.lensmap_with_callbacks("cube", info, lambda x, y: c.eval_host(0, x, y), None, "f_contain", W, H,
                                                    portable=portable)
        c.close()
    if not tables[True].built:
        pytest.skip("the random script does not build a map")
    ctx = host(True)
    off, tin, flagged, err = emu.build_inverse(ctx)
    ctx.close()
    if err:
        pytest.skip("the random script fails at run time (covered by the GPU fuzz)")
    off = emu.device_to_reference_layout(off, min(W, H))
    np.testing.assert_array_equal(off, tables[True].offsets, err_msg=src)
    np.testing.assert_array_equal(tin, tables[True].tints, err_msg=src)
    differs = np.nonzero((tables[False].offsets != off) | (tables[False].tints != tin))[0]
    assert set(differs.tolist()) <= set(flagged.tolist()), f"{len(differs)} entries differ, not all flagged\n{src}"


ADVERSARIAL = [
    ("cube", "quincuncial", None, 320, 240),
    ("cube", "stereographic", None, 320, 200),
    ("cube", "hammer", None, 320, 200),
    ("trism", "panini", None, 320, 200),
    ("cube", "winkeltripel", None, 240, 160),
    ("cube", "mollweide", None, 240, 120),
    ("cube", "cubestereo", None, 240, 160),
    ("cube", "fisheye1", None, 200, 200),
    ("cube", "fisheye2", None, 200, 200),
    ("cube", "debug", None, 200, 140),
    ("fast", "panini", "f_fov 200", 240, 160),
    ("cube", "cube", None, 240, 180),
    ("cube", "vandergrinten", None, 200, 200),
    ("cube", "eckert4", None, 160, 80),
    ("tetra", "equirect", None, 240, 120),
    ("cube", "mercator", None, 240, 160),
    ("cube", "cylinder", None, 240, 160),
    ("cube", "fahey", None, 240, 160),
    ("cube", "gallstereo", None, 240, 160),
    ("cube", "gumby", None, 240, 160),
    ("cube", "miller", None, 240, 160),
    ("cube_edge", "rectilinear", None, 240, 160),
]


@pytest.mark.parametrize("cfg", ADVERSARIAL)
def test_flags_cover_an_adversarial_libm(cfg):
    """The platform libm of this machine differs from bkm.h in about one result in a thousand and by one ulp, so the test
    above meets a handful of libm-dependent pixels at most.  Here the situation is scaled up until it is common: the host
    side (the `reference libm') is bkm.h with every inexact result pushed pseudo-randomly by up to 2^-30 relative
    (bk_set_host_math(ctx, 30)), the generated code is compiled with BK_LIBM_REL = 2^-30, and every entry the host
    interpreter then decides differently from the device code must be in the flagged list: this exercises the
    propagation rules (Lipschitz factors of every operation and libm call, the narrowing / comparison / floor checks,
    loop bounds, table indices) on thousands of real disagreements per lens instead of a few."""
    import blinky_amd
    globe, lens, zoom, W, H = cfg
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(30)
    S.configure(ctx, globe, lens, zoom, (W, H))
    off, tin, flagged, err = emu.build_inverse(ctx, defines=("BK_LIBM_REL=0x1p-30",))
    assert err == 0
    off = emu.device_to_reference_layout(off, min(W, H))
    ids = np.arange(W * H, dtype=np.uint32)
    hoff, htin = ctx.host_entries(ids)
    ctx.close()
    differs = np.nonzero((hoff != off) | (htin != tin))[0]
    missed = np.setdiff1d(differs, flagged)
    print(f"{lens}: {len(differs)} entries differ, {len(flagged)} flagged of {W * H}")
    assert len(missed) == 0, (len(differs), len(flagged), missed[:10])
    if lens == "quincuncial":           # (a float ray component one ulp off moves the texel about once in 2^16: few entries differ)
        assert len(differs) > 100


def check_bounds(ctx, which, dev, args, picks, label):
    """dev: emu.inverse_values / forward_values; the host interpreter of ctx on args[o] must land within dev's bounds"""
    checked = exceeded = 0
    worst = 0.0
    for o in picks:
        if dev["flag"][o] or dev["err"][o]:
            continue
        r = ctx.eval_host(which, *[float(a) for a in args[o]])
        n = int(dev["nret"][o])
        assert (r is None) == (n == -1), (o, r, n)
        if r is None:
            continue
        assert len(r) == n, (o, r, n)
        for i in range(n):
            if dev["tag"][o, i] != 3:
                continue
            v, e, h = dev["val"][o, i], dev["bound"][o, i], r[i]
            if np.isnan(v) or np.isnan(h):
                assert (np.isnan(v) and np.isnan(h)) or not np.isfinite(e), (o, i, v, h, e)
                continue
            checked += 1
            d = abs(h - v)
            if d > 0:
                worst = max(worst, d / e if e > 0 else np.inf)
            if not d <= e and not np.isnan(e):
                exceeded += 1
    print(f"{label}: {checked} values, worst |host - device| / bound = {worst:.3f}")
    assert checked > 0
    assert exceeded == 0, (exceeded, worst)


RAW_LATLON = "local function latlon_to_ray(lat, lon) return lat, lon, 0 end\n"


@pytest.mark.parametrize("raw", [False, True], ids=["ray", "latlon"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["random", "all-high", "all-low"])
@pytest.mark.parametrize("cfg", ADVERSARIAL)
def test_error_bounds_hold_against_an_adversarial_libm(cfg, mode, raw):
    """The invariant under the flags, checked directly and on EVERY pixel instead of on the rare ties: each value the
    generated lens_inverse returns carries a bound e, and the same script run by the host interpreter on any libm within
    BK_LIBM_REL of bkm.h must return a value within e of it - unless the evaluation raised the flag (an `if`, a loop bound, a
    table index depended on an inexact value).  Three stand-in libms at 2^-30: pseudo-random signs, every result high,
    every result low (the last two make the errors of a long chain add up instead of cancelling).  `latlon': the script's
    latlon_to_ray is shadowed by a function that hands latitude and longitude straight back, so that the bounds of the whole
    projection chain are what is compared (the built-in narrows to float, after which the bound is 0 or the flag is up)."""
    import blinky_amd
    globe, lens, zoom, W, H = cfg
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(30 + 64 * mode)
    if raw:
        if "latlon_to_ray" not in S.script("lenses", lens):
            pytest.skip("the lens does not go through latitude / longitude")
        info = S.configure(ctx, globe, lens, zoom, None)
        ctx.load_lens(RAW_LATLON + S.script("lenses", lens), lens + ".lua")
        ctx.resize(W, H)
        try:
            ctx.calc_zoom()
        except blinky_amd.ffi.BlinkyError:
            pytest.skip("the lens sizes itself through its own latlon_to_ray")
    else:
        S.configure(ctx, globe, lens, zoom, (W, H))
    dev = emu.inverse_values(ctx, defines=("BK_LIBM_REL=0x1p-30",))
    args = np.stack([dev["x"], dev["y"]], axis=1)
    check_bounds(ctx, 0, dev, args, range(0, W * H, 3), f"{lens}/{mode}")    # every third pixel, a different phase on each row
    ctx.close()


FORWARD = ["eckert1", "eckert5", "gins8", "kavrayskiy7", "larrivee", "polyconic", "sinusoidal", "wagner6", "winkel1", "winkel2",
           "winkeltripel", "vandergrinten", "gumby", "hammer", "panini", "quincuncial", "mollweide"]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["random", "all-high", "all-low"])
@pytest.mark.parametrize("lens", FORWARD)
def test_forward_error_bounds_hold_against_an_adversarial_libm(lens, mode):
    """The same for lens_forward (what the forward build of the lenses without an inverse evaluates at every texel corner),
    on float rays all over the sphere, the axes and the poles included."""
    import blinky_amd
    if "function lens_forward" not in S.script("lenses", lens):
        pytest.skip("no lens_forward")
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(30 + 64 * mode)
    S.configure(ctx, "cube", lens, None, (160, 120))
    rng = np.random.default_rng(11)
    rays = rng.normal(size=(6000, 3))
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 1], [0, 1, 1], [1, 1, 0]], float)
    rays = np.concatenate([axes / np.linalg.norm(axes, axis=1, keepdims=True), rays]).astype(np.float32).astype(np.float64)
    dev = emu.forward_values(ctx, rays, defines=("BK_LIBM_REL=0x1p-30",))
    check_bounds(ctx, 1, dev, rays, range(len(rays)), f"{lens}/{mode}")
    ctx.close()


@pytest.mark.parametrize("lens", ["eckert1", "eckert5", "gins8", "kavrayskiy7", "larrivee", "polyconic", "sinusoidal", "wagner6", "winkel1",
                                  "winkel2"])
def test_forward_corner_flags_cover_an_adversarial_libm(lens):
    """The forward build's discrete step - a texel corner's screen position (int)(x / scale + W/2), (int)(-y / scale + H/2),
    or none - against a stand-in libm of 2^-22 (coarser than elsewhere: a corner changes pixel only when x / scale lands
    within ~100 * 2^-22 of an integer): every corner the host interpreter places differently from the generated code is in
    the generated code's flagged list (the 10 lenses that only have lens_forward)."""
    import blinky_amd
    W, H = 200, 150
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(22)
    S.configure(ctx, "cube", lens, None, (W, H))
    xy, ok, flagged, err = emu.forward_corners(ctx, defines=("BK_LIBM_REL=0x1p-22",))
    assert err == 0
    n = len(ok)
    hx, hy, hok = ctx.host_corners(np.arange(n, dtype=np.uint32))
    ctx.close()
    same = (hok == ok) & ((ok == 0) | ((hx == xy[:, 0]) & (hy == xy[:, 1])))
    differs = np.nonzero(~same)[0]
    missed = np.setdiff1d(differs, flagged)
    print(f"{lens}: {len(differs)} of {n} corners differ, {len(flagged)} flagged")
    assert len(missed) == 0, (len(differs), len(flagged), missed[:10])
    assert len(flagged) < n                                    # (and the flags are not simply everything)


def test_draw_quad_with_int_min_corners_scans_like_the_reference():
    """draw_quad (fisheye.c:2246-2338) on quads a NaN projection produces: a corner at INT_MIN.  With the opposite bound at exactly 0 the
    reference's size check passes (abs(INT_MIN) is INT_MIN) and it scans 2^31 rows / columns; the generated code visits the visible part.
    The oracle really scans them (about ten seconds per such quad on one core: three of them here)."""
    import ctypes as C
    import blinky_amd
    IMIN = -2 ** 31
    W, H = 40, 24
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    S.configure(ctx, "cube", "eckert5", None, (W, H))
    quads = [
        (21, -2, 24, IMIN, 22, 0, 24, IMIN),          # the campaign's case: tall (y from INT_MIN to 0), row 0 visible
        (IMIN, 3, 0, 3, IMIN, 5, 0, 6),               # wide: x from INT_MIN to 0, rows 3..6
        (IMIN, 4, 0, 4, -7, 4, 0, 4),                 # a horizontal line from INT_MIN to 0
        (3, 2, 9, 2, 3, 8, 10, 9),                    # an ordinary quad
        (3, 2, 30, 2, 3, 8, 10, 9),                   # too wide: rejected
        (IMIN, IMIN, IMIN, IMIN, IMIN, IMIN, IMIN, IMIN),   # a single off-screen point
        (5, -5, 9, IMIN, 6, -1, 9, IMIN),             # tall, the other bound at -1: rejected by the size check
    ]
    O._o.ok_test_draw_quad.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for q in quads:
        c = np.array(q, np.int32)
        want = np.zeros((H, W), np.uint8)
        O._o.ok_test_draw_quad(W, H, c.ctypes.data, want.ctypes.data)
        got = emu.draw_quad(ctx, c)
        np.testing.assert_array_equal(got, want, err_msg=str(q))
    ctx.close()


def test_draw_quad_small_quads_equal_the_reference_pixel_for_pixel():
    """(r6) The generated draw_quad settles a quad on one or two rows with integer rules (row miny: [minx, maxx]; row miny + 1: the x of the
    ends that lie on it) and interpolates only from three rows on, with a table of quotients instead of the division.  4000 random quads
    around and across the screen's edges - one pixel, lines, two rows, three and more, wider than the 20-pixel limit, bow ties - against
    the oracle's draw_quad (fisheye.c:2246-2338), pixel for pixel."""
    import ctypes as C
    import blinky_amd
    W, H = 40, 24
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    S.configure(ctx, "cube", "eckert5", None, (W, H))
    O._o.ok_test_draw_quad.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(20260930)
    kinds = {"one row": 0, "two rows": 0, "three or more": 0, "rejected": 0}
    for k in range(4000):
        cx, cy = int(rng.integers(-6, W + 6)), int(rng.integers(-6, H + 6))
        spread_x = int(rng.choice([0, 1, 1, 2, 3, 6, 12, 22]))
        spread_y = int(rng.choice([0, 1, 1, 1, 2, 3, 6, 12, 22]))
        c = np.empty(8, np.int32)
        c[0::2] = cx + rng.integers(0, spread_x + 1, 4)
        c[1::2] = cy + rng.integers(0, spread_y + 1, 4)
        ys, xs = c[1::2], c[0::2]
        dy, dx = int(ys.max() - ys.min()), int(xs.max() - xs.min())
        kinds["rejected" if dx > 20 or dy > 20 else "one row" if dy == 0 else "two rows" if dy == 1 else "three or more"] += 1
        want = np.zeros((H, W), np.uint8)
        O._o.ok_test_draw_quad(W, H, c.ctypes.data, want.ctypes.data)
        got = emu.draw_quad(ctx, c)
        np.testing.assert_array_equal(got, want, err_msg=f"quad {k}: {c.tolist()}")
    assert min(kinds.values()) > 30, kinds
    ctx.close()


# ---- self-correcting iterations: the contraction-aware bound (bk_emit.cpp contraction_pattern, bk_device_rt.h bk_contract) ----------
ITERATIONS = {
    # Kepler's equation by Newton's method: converges quadratically, forgets its starting error
    "kepler": ("local M = x * 2.5\n   local ecc = 0.55 + y * 0.2\n   local E = M\n   local dE = 0\n"
               "   for i = 1, 12 do\n      dE = (M - E + ecc * sin(E)) / (1 - ecc * cos(E))\n      E = E + dE\n   end\n", "E * 0.3", "dE + y"),
    # eckert4's own iteration, away from and near the pole (cos t -> 0: the classic bound grew by thousands per step there)
    "eckert4-theta": ("local lat = (x / 1.3) * (pi / 2) * 0.9999\n   local t = lat / 2\n   local dt = 0\n"
                      "   for i = 1, 20 do\n      dt = -(t + sin(t) * cos(t) + 2 * sin(t) - (2 + pi * 0.5) * sin(lat)) / (2 * cos(t) * (1 + cos(t)))\n      t = t + dt\n   end\n",
                      "t", "y + dt"),
    # a fixed-point iteration that converges linearly (|g'| up to 0.7): the errors of ALL steps add up, weighted
    "fixed-point": ("local t = 0.5\n   for i = 1, 30 do\n      t = cos(t) * 0.7 + x * 0.2\n   end\n", "t", "y"),
    # a map that EXPANDS (|g'| up to 1.5): the bound has to grow with it
    "expanding": ("local t = y\n   for i = 1, 6 do\n      t = t + 0.5 * sin(t) + x * 0.1\n   end\n", "t * 0.2", "x"),
    # two locals assigned per step, the second one computed from the new value of the first and used after the loop
    "two-locals": ("local t = x\n   local u = 0\n   for i = 1, 8 do\n      t = t - (t - 0.8 * sin(t) - y) / (1 - 0.8 * cos(t))\n      u = atan2(sin(t), 1.5 + cos(t))\n   end\n", "u", "t * 0.25"),
    # square root and division inside the step, a local declared in the body
    "sqrt-step": ("local t = 1 + x * x\n   for i = 1, 10 do\n      local s = sqrt(t * t + 1)\n      t = t - (t + atan(t) - 2 - y) * s / (s + 1 / s)\n   end\n", "t * 0.3", "x"),
}


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["random", "all-high", "all-low"])
@pytest.mark.parametrize("name", sorted(ITERATIONS))
def test_contracted_iterations_hold_against_an_adversarial_libm(name, mode):
    """Loops with one carried variable get the contraction-aware bound: every value the generated code returns must still lie within
    its bound of what the host interpreter computes on a libm 2^-30 off (unless flagged), for iterations that forget their errors
    (Newton), that accumulate them (linear convergence), that amplify them, and for the other variables a step assigns.  And the
    rule must actually be in force: the generated code calls bk_contract, and near eckert4's pole the bound stays small."""
    import blinky_amd
    body, lat, lon = ITERATIONS[name]
    src = (RAW_LATLON + "max_fov = 360\nmax_vfov = 180\nlens_width = 2.6\nlens_height = 2\nonload = \"f_contain\"\n"
           "function lens_inverse(x, y)\n   " + body + "   return latlon_to_ray(" + lat + ", " + lon + ")\nend\n")
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(30 + 64 * mode)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(src, name + ".lua")
    ctx.set_zoom(blinky_amd.ffi.ZOOM_CONTAIN)
    W, H = 120, 90
    ctx.resize(W, H)
    ctx.calc_zoom()
    assert "bk_contract(" in ctx.kernel_source(compile=False)
    dev = emu.inverse_values(ctx, defines=("BK_LIBM_REL=0x1p-30",))
    args = np.stack([dev["x"], dev["y"]], axis=1)
    check_bounds(ctx, 0, dev, args, range(W * H), f"{name}/{mode}")
    unflagged = (dev["flag"] == 0) & (dev["err"] == 0) & (dev["nret"] == 3)
    assert unflagged.mean() > 0.9, unflagged.mean()                      # (the rule is not "flag everything")
    if name == "eckert4-theta":
        # |x| = 1.3 is 0.9999 of the pole: cos t ~ 0.02 there.  The classic propagation multiplied the bound by ~ 4 / (2 cos t) = 100 per
        # step, twenty times over; contracted, it stays a few hundred libm errors at most
        assert np.nanmax(dev["bound"][unflagged, 0]) < 1e4 * 2.0 ** -30, np.nanmax(dev["bound"][unflagged, 0])
    ctx.close()


def _random_iteration(rng):
    """a random loop of the contracted kind: Newton or a damped fixed point on a random smooth f, one carried variable, sometimes a second local"""
    c = [float(np.round(rng.uniform(0.2, 1.5), 3)) for _ in range(4)]
    fs = [  # (f(t), f'(t)) with parameters from x, y
        (f"(t + {c[0]} * sin(t) - x * {c[1]} - y)", f"(1 + {c[0]} * cos(t))"),
        (f"(t * {c[0]} + tanh(t) - x)", f"({c[0]} + 1 - tanh(t) * tanh(t))"),
        (f"(exp(t * {c[0] * 0.3}) + t - 2 - x * {c[1]})", f"({c[0] * 0.3} * exp(t * {c[0] * 0.3}) + 1)"),
        (f"(atan(t) * {c[0]} + t * {c[1]} - y * 2 - x)", f"({c[0]} / (1 + t * t) + {c[1]})"),
        (f"(t + sin(t) * cos(t) * {min(c[0], 0.9)} - x)", f"(1 + {min(c[0], 0.9)} * (cos(t) * cos(t) - sin(t) * sin(t)))"),
    ]
    f, df = fs[int(rng.integers(len(fs)))]
    steps = int(rng.integers(3, 25))
    kind = int(rng.integers(3))
    if kind == 0:       # Newton
        body = f"local t = x * {c[2]}\n   local d = 0\n   for i = 1, {steps} do\n      d = {f} / {df}\n      t = t - d\n   end\n"
        return body, "t * 0.2", "d + y"
    if kind == 1:       # damped fixed point (linear convergence, or slow divergence)
        lam = float(np.round(rng.uniform(0.1, 0.9), 3))
        body = f"local t = y\n   for i = 1, {steps} do\n      t = t - {lam} * {f}\n   end\n"
        return body, "t * 0.1", "x"
    body = (f"local t = x\n   local u = 0\n   for i = 1, {steps} do\n      local g = {f}\n      t = t - g / {df}\n      u = sqrt(1 + t * t) * {c[3]} + g\n   end\n")
    return body, "u * 0.1", "t * 0.2"


@pytest.mark.parametrize("seed", range(40))
def test_random_contracted_iterations_hold_against_an_adversarial_libm(seed):
    """The contraction-aware bound on random iterations (Newton / damped fixed point on five families of smooth functions, 3-24 steps, random
    coefficients, with and without a second assigned local), libm stand-in chosen by the seed: every unflagged value within its bound."""
    import blinky_amd
    rng = np.random.default_rng(9100 + seed)
    body, lat, lon = _random_iteration(rng)
    src = (RAW_LATLON + "max_fov = 360\nmax_vfov = 180\nlens_width = 2.6\nlens_height = 2\nonload = \"f_contain\"\n"
           "function lens_inverse(x, y)\n   " + body + "   return latlon_to_ray(" + lat + ", " + lon + ")\nend\n")
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(30 + 64 * (seed % 3))
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(src, f"iter{seed}.lua")
    ctx.set_zoom(blinky_amd.ffi.ZOOM_CONTAIN)
    W, H = 64, 48
    ctx.resize(W, H)
    ctx.calc_zoom()
    assert "bk_contract(" in ctx.kernel_source(compile=False), src
    dev = emu.inverse_values(ctx, defines=("BK_LIBM_REL=0x1p-30",))
    args = np.stack([dev["x"], dev["y"]], axis=1)
    check_bounds(ctx, 0, dev, args, range(W * H), f"iter{seed}")
    ctx.close()


NOT_CONTRACTED = {
    # two variables carried from step to step: a Jacobian, not a derivative - left to the classic rule
    "two-carried": "local a, b = x, y\n   for i = 1, 5 do\n      a = a + 0.1 * sin(b)\n      b = b - 0.1 * sin(a)\n   end\n   return a, b, 0",
    # a comparison inside the step: a discrete decision on a value whose bound was set to 0 for the step would go unnoticed
    "comparison": "local t = x\n   for i = 1, 8 do\n      local d = (t - cos(t)) / (1 + sin(t))\n      if d < 0.001 then break end\n      t = t - d\n   end\n   return t, y, 0",
    # a script function in the step (it may do anything)
    "call": "local function f(v) return v - cos(v) end\n   local t = x\n   for i = 1, 8 do\n      t = t - f(t) / (1 + sin(t))\n   end\n   return t, y, 0",
    # a global as the carried variable: another callback could read it
    "global": "g = x\n   for i = 1, 8 do\n      g = g - (g - cos(g)) / (1 + sin(g))\n   end\n   return g, y, 0",
    # operations without a derivative rule here
    "floor": "local t = x\n   for i = 1, 4 do\n      t = t + math.floor(t) * 0.1 + sin(t)\n   end\n   return t, y, 0",
    "power": "local t = x\n   for i = 1, 4 do\n      t = t - (t ^ 3 - y) * 0.1\n   end\n   return t, y, 0",
    # nothing carried at all: every step starts from the arguments
    "nothing-carried": "local t = 0\n   for i = 1, 4 do\n      t = sin(x * i) + cos(y)\n   end\n   return t, y, 0",
    # a while loop (its condition is a comparison)
    "while": "local t = x\n   local n = 0\n   while n < 5 do\n      t = t - (t - cos(t)) / (1 + sin(t))\n      n = n + 1\n   end\n   return t, y, 0",
}


@pytest.mark.parametrize("name", sorted(NOT_CONTRACTED))
def test_loops_outside_the_pattern_keep_the_classic_bound(name):
    """contraction_pattern is deliberately narrow: one carried local, straight-line smooth arithmetic.  Everything else is generated as
    before (no bk_contract in the source) - and still correct against the interpreter."""
    import blinky_amd
    src = ("g = 0\nmax_fov = 360\nmax_vfov = 180\nlens_width = 2.6\nlens_height = 2\nonload = \"f_contain\"\n"
           "function lens_inverse(x, y)\n   " + NOT_CONTRACTED[name] + "\nend\n")
    ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
    ctx.set_host_math(True)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(src, name + ".lua")
    ctx.set_zoom(blinky_amd.ffi.ZOOM_CONTAIN)
    ctx.resize(32, 24)
    ctx.calc_zoom()
    assert "bk_contract(" not in ctx.kernel_source(compile=False), name
    v = emu.inverse_values(ctx)
    xy = np.stack([v["x"], v["y"]], axis=1)
    h_out, h_n = ctx.eval_host_many(0, xy)
    np.testing.assert_array_equal(v["nret"], h_n)
    d_out = v["val"][:, : h_out.shape[1]]
    used = np.arange(h_out.shape[1])[None, :] < h_n[:, None]
    assert (((d_out.view(np.uint64) == h_out.view(np.uint64)) | (np.isnan(d_out) & np.isnan(h_out))) | ~used).all()
    ctx.close()
