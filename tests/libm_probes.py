"""Probe lenses and input sets that take the device libm (blinky_amd/csrc/bkm.h as hiprtc builds it) and the error bounds of the
generated code (bk_device_rt.h) over WHOLE domains instead of where the shipped lenses go: small forward lenses whose
lens_forward(x, y, z) receives three arbitrary doubles (bk_debug_eval_device, bk_debug_eval and tests/hostemu all hand doubles over
without narrowing them).  tests/test_libm_probes_cpu.py runs them through the host interpreter, the generated code under hostemu and
libbkm_host.so; tests/test_libm_probes_gpu.py runs the same probes on the device.  A plain module: no fixtures, no GPU.

The generators of tests/test_bkm.py live here too (u, logu, TRIG, the seam sets): that test draws them from `rng` below, everything
else in this module draws from generators of its own, so that what test_bkm.py sees does not depend on who imported this first."""
import math

import numpy as np

# ---- the generators of tests/test_bkm.py ------------------------------------------------------------------------------------------
rng = np.random.default_rng(20240924)
N = 700


def u(a, b, n=N, rng=None):
    return (rng or globals()["rng"]).uniform(a, b, n)


def logu(a, b, n=N, rng=None):
    r = rng or globals()["rng"]
    return np.exp(r.uniform(math.log(a), math.log(b), n)) * r.choice([-1.0, 1.0], n)


def TRIG(rng=None):
    return np.concatenate([u(-10, 10, rng=rng), logu(1e-8, 1e6, rng=rng), logu(1e6, 1e300, N // 4, rng=rng),
                           np.arange(1, 120) * math.pi / 2, np.arange(1, 120) * math.pi / 32])


def seam_trig(rng=None):
    """multiples of pi/32 and their neighbours, and both sides of 2^16 where sin / cos switch reductions"""
    r = rng or globals()["rng"]
    k = np.arange(-3000, 3000)
    near = np.concatenate([k * math.pi / 32 + d for d in (0.0, 1e-9, -1e-13, 3e-16)])
    edge = np.concatenate([65536.0 + r.uniform(-40, 40, 400), -65536.0 + r.uniform(-40, 40, 400), [65535.99999999999, 65536.0, 65536.00000000001]])
    return near, edge


def seam_atan():
    """atan: the table's decision points i/8 - 1/16 (+ the 2^-13 bias), both sides, and their reciprocals"""
    pts = (np.arange(1, 17) - 0.5) / 8.0
    at = np.concatenate([pts + d for d in (0.0, 2.0 ** -13, -2.0 ** -13, 1e-15, -1e-15)])
    return np.concatenate([at, 1.0 / at[at > 0], [1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52]])


def seam_atan2():
    """(ys, xs): atan2 at the ends of the exponent range and across the "quotient below 2^-59" switch"""
    ys = np.array([5e-324, 1e-310, 1e-300, 1e300, 1.7e308, 1e-320, 3.0, 1e-17, 1e-18, 2.0 ** -60, 2.0 ** -61, 1e308, 1e-308, 1e-308, 4e-324])
    xs = np.array([5e-324, 3e-310, 1e300, 1e-300, 1.7e308, 1e-322, -1e-320, 1.0, 1.0, 1.0, 1.0, -1e308, 1e308, -1e-308, 1e-323])
    return ys, xs


def seam_fmod(n, rng=None):
    """(fx, fy): fmod's fma path, its fallback above a quotient of 2^52, subnormals"""
    r = rng or globals()["rng"]
    fx = np.concatenate([r.uniform(-1e4, 1e4, n), logu(1e-300, 1e300, n // 2, rng=r), r.integers(0, 2 ** 53, n // 2).astype(float), logu(1e-320, 1e-305, max(n // 50, 1), rng=r), [2.0 ** 60, 2.0 ** 53 + 2, 7.0]])
    fy = np.concatenate([r.uniform(-9, 9, n), logu(1e-300, 1e300, n // 2, rng=r), r.integers(1, 2 ** 20, n // 2).astype(float), logu(1e-320, 1e-305, max(n // 50, 1), rng=r), [3.0, 3.0, 2.0 ** -1074]])
    return fx, fy


# ---- the special values of test_bkm.py's test_special_values ---------------------------------------------------------------------
inf, nan = math.inf, math.nan
SPECIAL1 = [inf, -inf, nan, 0.0, -0.0, 1.0000001, -1.5, 1.0, -1.0, 710.0, -746.0, 30.0]
# (y, x, atan2(y, x)): quadrants / zeros / infinities (C99 F.9.1.4)
ATAN2_CASES = [(0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, math.pi), (-0.0, -1.0, -math.pi),
               (1.0, 0.0, math.pi / 2), (-1.0, 0.0, -math.pi / 2), (0.0, -0.0, math.pi), (-0.0, -0.0, -math.pi),
               (0.0, 0.0, 0.0), (1.0, inf, 0.0), (1.0, -inf, math.pi), (inf, 1.0, math.pi / 2),
               (inf, inf, math.pi / 4), (inf, -inf, 3 * math.pi / 4), (-inf, -inf, -3 * math.pi / 4)]
# (x, y, pow(x, y)) (C99 F.9.4.4)
POW_CASES = [(2.0, 0.0, 1.0), (nan, 0.0, 1.0), (1.0, nan, 1.0), (-8.0, 3.0, -512.0), (-8.0, 2.0, 64.0),
             (0.0, -1.0, inf), (-0.0, -1.0, -inf), (-0.0, 3.0, -0.0), (0.0, 2.5, 0.0), (inf, -2.0, 0.0),
             (-inf, 3.0, -inf), (0.5, inf, 0.0), (2.0, inf, inf), (2.0, -inf, 0.0), (-1.0, inf, 1.0),
             (3.0, 2.0, 9.0), (2.0, 0.5, math.sqrt(2.0)), (2.0, -1.0, 0.5), (10.0, 308.0, 1e308), (2.0, -1074.0, 5e-324)]
CONVERSION_EDGES = [2.0 ** 31, -2.0 ** 31 - 1, 2.0 ** 53 + 2, 2.0 ** 63, 1e19]
NONFINITE = [0.0, -0.0, inf, -inf, nan]


def _triples(cols):
    return np.stack([np.asarray(c, np.float64) for c in cols], axis=1)


def wide_inputs(seed=20261017):
    """about 3300 tuples (x, y, z): blocks in which the three arguments are of one kind (so that two-argument functions meet operands of
    comparable size), blocks of pairs that belong together (atan2 / pow / fmod cases and seams, in both argument orders), a block drawn
    at random from ALL the values above (arguments of wildly different size), and +-0 / +-inf / NaN in every argument position."""
    r = np.random.default_rng(seed)
    near, edge = seam_trig(r)
    at = seam_atan()
    sub = logu(1e-320, 1e-300, 300, rng=r)
    one_minus = 1 - logu(1e-16, 1e-3, 100, rng=r) ** 2                 # asin / acos next to +-1
    pool = np.concatenate([TRIG(r), r.choice(near, 300), edge, at, -at, sub, one_minus, -one_minus, u(-745, 709, 200, rng=r),
                           logu(1e-300, 1e300, 200, rng=r), 1 + logu(1e-12, 1e-2, 100, rng=r), SPECIAL1, CONVERSION_EDGES,
                           -np.array(CONVERSION_EDGES), [10.0, 2.0, 0.5, 1e308, -1e308, 5e-324, -5e-324, 2.2250738585072014e-308]])
    blocks = [
        _triples([u(-10, 10, 800, rng=r) for _ in range(3)]),
        _triples([u(-1, 1, 400, rng=r) for _ in range(3)]),
        _triples([logu(1e-8, 1e6, 400, rng=r) for _ in range(3)]),
        _triples([logu(1e6, 1e300, 150, rng=r) for _ in range(3)]),
        _triples([logu(1e-320, 1e-300, 150, rng=r) for _ in range(3)]),
        _triples([u(-745, 709, 150, rng=r), u(-60, 60, 150, rng=r), r.integers(-6, 7, 150).astype(float)]),
        _triples([np.abs(logu(1e-5, 1e5, 150, rng=r)), u(-60, 60, 150, rng=r), u(0.01, 4, 150, rng=r)]),
        _triples([r.choice(near, 200), r.choice(edge, 200), r.choice(np.concatenate([at, -at, one_minus, -one_minus]), 200)]),
        _triples([r.choice(pool, 400) for _ in range(3)]),
    ]
    ys, xs = seam_atan2()
    fx, fy = seam_fmod(60, r)
    pairs = ([(c[0], c[1]) for c in ATAN2_CASES] + [(c[0], c[1]) for c in POW_CASES] + list(zip(ys, xs)) + list(zip(-ys, xs)) +
             list(zip(fx, fy)) + [(5.0, 5.0), (-5.0, 5.0), (0.0, 3.0), (7.5, 2.5), (1e308, 3e-310), (5e-324, 3.0), (100.0, 10.0), (8.0, 2.0)])
    pairs = np.array(pairs, np.float64)
    third = r.choice(pool, len(pairs))
    blocks += [np.column_stack([pairs[:, 0], pairs[:, 1], third]), np.column_stack([pairs[:, 1], pairs[:, 0], third]),
               np.column_stack([third, pairs[:, 0], pairs[:, 1]])]
    special = np.array(NONFINITE + CONVERSION_EDGES + [-c for c in CONVERSION_EDGES])
    blocks.append(np.array([(a, b, c) for a in NONFINITE for b in NONFINITE for c in NONFINITE]))
    for pos in range(3):                         # every special value in every position, beside ordinary and beside extreme company
        for other in (u(-3, 3, (len(special), 3), rng=r), r.choice(pool, (len(special), 3))):
            t = np.array(other, np.float64)
            t[:, pos] = special
            blocks.append(t)
    return np.ascontiguousarray(np.concatenate(blocks), np.float64)


def control_inputs(seed=20261018):
    """(x, y, z) for the control probe: x indexes a four-element table (fractional, negative, huge, NaN indices), `for i = 1, y, z` counts
    at most a few hundred steps - or runs away, on the last tuple (one only: the host interpreter's budget is fifty times the device's
    and costs it seconds), where both sides must report the loop budget"""
    r = np.random.default_rng(seed)
    idx = np.concatenate([r.integers(-2, 8, 200).astype(float), u(-2, 7, 100, rng=r), [1.0, 4.0, 0.0, -0.0, 5.0, 0.5, 1.5, 4.000000000000001, 3.9999999999999996,
                          nan, inf, -inf, 1e19, -1e19, 2.0 ** 31, 2.0 ** 32 + 1, -2.0 ** 31 - 1, 2.0 ** 53 + 2, 2.0 ** 63, 5e-324]])
    n = len(idx)
    lim = np.concatenate([r.integers(-3, 300, n // 2).astype(float), u(-3, 300, n - n // 2, rng=r)])
    step = np.where(r.random(n) < 0.5, 1.0, r.choice([2.0, 0.5, 3.0, 7.25, 100.0, 1e19, inf], n))
    ordinary = np.column_stack([idx, lim, step])
    # limits and steps at the edges: empty ranges, a NaN limit or step, an infinite limit reached by an infinite step, a negative step
    edges = np.array([(1.0, nan, 1.0), (2.0, 10.0, nan), (3.0, inf, inf), (4.0, -inf, 1.0), (1.0, -50.0, -1.0), (2.0, -50.0, -0.75), (3.0, 1.0, 1e300),
                      (4.0, 2.0 ** 53 + 2, 2.0 ** 52), (1.0, 1e19, 1e18), (2.0, 1.0, -inf), (3.0, 0.0, 1.0), (4.0, 1.0, 1.0), (nan, 10.0, 0.0), (2.0, 5.0, 0.0)])        # (step 0: OP_FORLOOP tests limit <= idx, so these two do not run at all)
    runaway = np.array([(2.5, 1e19, 1.0)])
    return np.ascontiguousarray(np.concatenate([ordinary, edges, runaway]), np.float64)


# ---- the probe lenses ---------------------------------------------------------------------------------------------------------------
HEADER = 'max_fov = 360\nmax_vfov = 180\nlens_width = 5\nlens_height = 3.5\nonload = "f_contain"\n'


def lens(body):
    return HEADER + "function lens_forward(x, y, z)\n" + "".join("   " + l.strip() + "\n" for l in body.strip().splitlines()) + "end\n"


# references of the operator columns: the Lua 5.2 definitions (luai_nummod of luaconf.h, math_log / math_modf / math_deg / math_rad /
# math_min / math_max of lmathlib.c) written out in numpy.  libm1 / libm2 columns are compared with libbkm_host.so itself.
def lua_mod(a, b):
    with np.errstate(all="ignore"):
        return a - np.floor(a / b) * b


def lua_modf_int(x):                           # math_modf of lmathlib.c is C modf, which numpy's modf is
    return np.modf(x)[1]


def lua_modf_frac(x):                          # (the fraction carries the argument's sign: -0.0 for -2 and for -0.0, +-0 for +-inf)
    return np.modf(x)[0]


RADIANS_PER_DEGREE = 3.14159265358979323846 / 180.0


def lua_min3(a, b, c):
    m = np.where(b < a, b, a)
    return np.where(c < m, c, m)


def lua_max3(a, b, c):
    m = np.where(b > a, b, a)
    return np.where(c > m, c, m)


_bkm = None


def _bkm_lib():
    """libbkm_host.so: the HOST build of bkm.h (tests/test_bkm.py measures it against mpmath)"""
    global _bkm
    if _bkm is None:
        import ctypes as C
        import os
        _bkm = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blinky_amd", "libbkm_host.so"))
        _bkm.bkmh_map1.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_long]
        _bkm.bkmh_map2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    return _bkm


def bkm1(name, xs):
    xs = np.ascontiguousarray(xs, np.float64)
    out = np.empty_like(xs)
    _bkm_lib().bkmh_map1(name.encode(), xs.ctypes.data, out.ctypes.data, len(xs))
    return out


def bkm2(name, xs, ys):
    xs, ys = np.ascontiguousarray(xs, np.float64), np.ascontiguousarray(ys, np.float64)
    out = np.empty_like(xs)
    _bkm_lib().bkmh_map2(name.encode(), xs.ctypes.data, ys.ctypes.data, out.ctypes.data, len(xs))
    return out


# A column of a value probe is described by its reference: a function of the argument array [n, 3], or None where there is no closed
# reference (compared between the interpreter, hostemu and the device only).
def L1(name, a):                               # a libm entry of one argument: libbkm_host.so itself
    return lambda t: bkm1(name, t[:, a])


def L2(name, a, b):
    return lambda t: bkm2(name, t[:, a], t[:, b])


def OP(fn, *argpos):                           # an operator / IEEE function: numpy
    def ref(t):
        with np.errstate(all="ignore"):
            return fn(*[t[:, k] for k in argpos])
    return ref


def lua_log_base(t, a, b):                     # math_log of lmathlib.c (5.2): log10 for base 10, else log(x) / log(base)
    with np.errstate(all="ignore"):
        return np.where(t[:, b] == 10.0, bkm1("log10", t[:, a]), bkm1("log", t[:, a]) / bkm1("log", t[:, b]))


X, Y, Z = 0, 1, 2

# The three C functions the reference registers for scripts, transcribed: doubles from libbkm_host.so narrowed into a float vector, float
# arithmetic with one rounding per operation, widened back.  A result that is nil is NaN here, as in what the debug entries return.
F32 = np.float32
CUBE_PLATES = [((0, 0, 1), (0, 1, 0)), ((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)),
               ((0, -1, 0), (0, 0, 1))]              # (forward, up) of globes/cube.lua, each with a fov of 90 degrees


def plate_index_valid(x, numplates=len(CUBE_PLATES)):
    """`int plate_index = luaL_checknumber(...)` truncates; NaN and everything outside int are INT_MIN: nil unless 0 <= index < numplates"""
    return (x > -1.0) & (x < numplates)


def ray_of_latlon(t):                          # latlon_to_ray(lat, lon) of (x, y)
    with np.errstate(all="ignore"):
        slat, clat, slon, clon = bkm1("sin", t[:, X]), bkm1("cos", t[:, X]), bkm1("sin", t[:, Y]), bkm1("cos", t[:, Y])
        return [c.astype(F32).astype(np.float64) for c in (slon * clat, slat, clon * clat)]


def latlon_of_ray(t):                          # ray_to_latlon(x, y, z): (lat, lon)
    with np.errstate(all="ignore"):
        r = t.astype(F32)
        lon = bkm2("atan2", r[:, 0].astype(np.float64), r[:, 2].astype(np.float64))
        lat = bkm2("atan2", r[:, 1].astype(np.float64), np.sqrt((r[:, 0] * r[:, 0] + r[:, 2] * r[:, 2]).astype(np.float64)))
        return [lat, lon]


def ray_of_cube_plate(t):                      # plate_to_ray(plate, u, v) of (x, y, z) on the cube globe
    with np.errstate(all="ignore"):
        n = len(t)
        valid = plate_index_valid(t[:, X])
        idx = np.where(valid, np.trunc(t[:, X]), 0).astype(np.int64)
        fwd = np.array([p[0] for p in CUBE_PLATES], F32)
        up0 = np.array([p[1] for p in CUBE_PLATES], F32)
        right = np.cross(up0, fwd).astype(F32)                        # (axis vectors: the cross products are exact)
        up = np.cross(fwd, right).astype(F32)
        fov = F32(90 * 3.14159265358979323846 / 180)
        dist = bkm1("tan", np.array([np.float64(fov / F32(2))]))
        dist = F32(0.5 / dist[0])
        fu, fv = (t[:, Y] - 0.5).astype(F32), (-(t[:, Z] - 0.5)).astype(F32)
        ray = np.zeros((n, 3), F32)
        ray = ray + dist * fwd[idx]                                   # VectorMA, three times
        ray = ray + fu[:, None] * right[idx]
        ray = ray + fv[:, None] * up[idx]
        length = ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1] + ray[:, 2] * ray[:, 2]
        length = np.sqrt(length.astype(np.float64)).astype(F32)
        ilength = F32(1) / length
        ray = np.where((length != 0)[:, None], ray * ilength[:, None], ray)
        return [np.where(valid, ray[:, k].astype(np.float64), np.nan) for k in range(3)]

VALUE_PROBES = {
    "trig": ("""
        local a, b = math.sin(x), math.cos(x)
        local c = math.tan(x)
        local d = math.sin(y)
        local e = math.cos(z)
        local f = math.tan(y)
        return a, b, c, d, e, f""", [L1("sin", X), L1("cos", X), L1("tan", X), L1("sin", Y), L1("cos", Z), L1("tan", Y)]),
    "inv_trig": ("""
        local a, b, c = math.asin(x), math.acos(x), math.atan(x)
        local d, e = math.atan2(y, x), math.atan2(x, y)
        local f = math.atan(z)
        return a, b, c, d, e, f""", [L1("asin", X), L1("acos", X), L1("atan", X), L2("atan2", Y, X), L2("atan2", X, Y), L1("atan", Z)]),
    "exp_family": ("""
        local a, b, c, d = math.exp(x), math.sinh(x), math.cosh(x), math.tanh(x)
        local e, f = math.exp(y), math.tanh(z)
        return a, b, c, d, e, f""", [L1("exp", X), L1("sinh", X), L1("cosh", X), L1("tanh", X), L1("exp", Y), L1("tanh", Z)]),
    "log_family": ("""
        local a, b = math.log(x), math.log10(x)
        local c = math.log(x, y)
        local d = math.sqrt(x)
        local e, f = math.log(y, 10), math.log(z, 2)
        return a, b, c, d, e, f""", [L1("log", X), L1("log10", X), lambda t: lua_log_base(t, X, Y), OP(np.sqrt, X), L1("log10", Y), OP(lambda c: bkm1("log", c) / bkm1("log", np.full_like(c, 2.0)), Z)]),
    "pow": ("""
        local a, b = math.pow(x, y), x ^ y
        local c, d = math.pow(y, z), z ^ x
        local e, f, g = x ^ 2, 2 ^ x, y ^ 0.5
        return a, b, c, d, e, f, g""", [L2("pow", X, Y), L2("pow", X, Y), L2("pow", Y, Z), L2("pow", Z, X), lambda t: bkm2("pow", t[:, X], np.full(len(t), 2.0)),
                                        lambda t: bkm2("pow", np.full(len(t), 2.0), t[:, X]), lambda t: bkm2("pow", t[:, Y], np.full(len(t), 0.5))]),
    "mod": ("""
        local a, b = math.fmod(x, y), x % y
        local c, d = math.fmod(y, z), y % z
        local e, f = x % 1, math.fmod(z, x)
        return a, b, c, d, e, f""", [L2("fmod", X, Y), OP(lua_mod, X, Y), L2("fmod", Y, Z), OP(lua_mod, Y, Z),
                                     OP(lambda a: lua_mod(a, np.ones_like(a)), X), L2("fmod", Z, X)]),
    "rounding": ("""
        local a, b = math.floor(x), math.ceil(x)
        local c, d = math.modf(x)
        local e = math.abs(x)
        local f, g = math.deg(x), math.rad(x)
        return a, b, c, d, e, f, g""", [OP(np.floor, X), OP(np.ceil, X), OP(lua_modf_int, X), OP(lua_modf_frac, X), OP(np.abs, X),
                                        OP(lambda a: a / RADIANS_PER_DEGREE, X), OP(lambda a: a * RADIANS_PER_DEGREE, X)]),
    "minmax": ("""
        local a, b = math.min(x, y, z), math.max(x, y, z)
        local c, d = math.min(z, x), math.max(y)
        return a, b, c, d""", [OP(lua_min3, X, Y, Z), OP(lua_max3, X, Y, Z), OP(lambda c, a: np.where(a < c, a, c), Z, X), OP(lambda b: b, Y)]),
    "rays": ("""
        local a, b, c = latlon_to_ray(x, y)
        local d, e = ray_to_latlon(x, y, z)
        local f, g, h = plate_to_ray(x, y, z)
        return a, b, c, d, e, f, g, h""", [lambda t: ray_of_latlon(t)[0], lambda t: ray_of_latlon(t)[1], lambda t: ray_of_latlon(t)[2],
                                           lambda t: latlon_of_ray(t)[0], lambda t: latlon_of_ray(t)[1],
                                           lambda t: ray_of_cube_plate(t)[0], lambda t: ray_of_cube_plate(t)[1], lambda t: ray_of_cube_plate(t)[2]]),
}

# nil or number?  NaN beside NaN cannot tell a nil result from a NaN number, so this one counts plate_to_ray's nils in Lua
PLATE_NIL_PROBE = """
    local f, g, h = plate_to_ray(x, y, z)
    local n = 0
    if f == nil then n = n + 1 end
    if g == nil then n = n + 1 end
    if h == nil then n = n + 1 end
    return n"""


def plate_nil_inputs():
    """(args, valid): plate indices at the edges of the cube's six plates and of int, NaN among them, each with u = 0.25, v = 0.75"""
    edge = np.array([nan, -inf, inf, -1.0, -0.999, -0.0, 0.0, 5.999, 6.0, 2.0 ** 31, -2.0 ** 31 - 1, 2.0 ** 32 + 1, 2.0 ** 63, 1e19, 3.5])
    return np.column_stack([edge, np.full(len(edge), 0.25), np.full(len(edge), 0.75)]), plate_index_valid(edge)


# the control probe: a local array table indexed by x, a numeric for whose limit and step are arguments
CONTROL_PROBE = """
    local t = {10, 20, 30, 40}
    local a = t[x] or -1
    local s, n = 0, 0
    for i = 1, y, z do
       s = s + i
       n = n + 1
    end
    return a, s, n"""

# ---- bound probes: composites whose inner value is INEXACT (a libm result), fed into each family of operations.  The inner values are
# bounded functions (sin, cos, tanh) of the arguments, so that the probes stay in well-conditioned territory over the whole wide set. -----
INNER = """
    local v, w = math.sin(x), math.tanh(y) * 3
    local p = math.exp(math.cos(z))
"""
BOUND_PROBES = {
    "trig_of_inexact": INNER + """
        local a, b, c = math.sin(w), math.cos(w * 5), math.tan(v)
        local d, e = math.sin(v * p), math.cos(p + w)
        local f = math.tan(w * 0.4)
        return a, b, c, d, e, f""",
    "inv_trig": INNER + """
        local a, b, c = math.asin(v * 0.99), math.acos(v * 0.99), math.atan(w * p)
        local d, e = math.atan2(v, w), math.atan2(w, p)
        local f = math.atan2(p, v)
        return a, b, c, d, e, f""",
    "exp_family": INNER + """
        local a, b, c, d = math.exp(w), math.sinh(w), math.cosh(w * p), math.tanh(v)
        local e = math.exp(v * w - p)
        return a, b, c, d, e""",
    "log_family": INNER + """
        local a, b = math.log(p), math.log10(p + w * w)
        local c, d = math.log(p, 2.5), math.log(p * 3, 10)
        local e, f = math.sqrt(p), math.sqrt(math.abs(w) + p)
        return a, b, c, d, e, f""",
    "pow": INNER + """
        local a, b = p ^ v, math.pow(p, w)
        local c, d = v ^ 3, math.pow(w, 2)
        local e, f = p ^ 0.5, 2 ^ w
        return a, b, c, d, e, f""",
    "mod": INNER + """
        local a, b = math.fmod(w * 7, 0.4), (v * 7) % p
        local c, d = math.fmod(p * 5, w + 4), (w * 0.7) % 0.25
        local e, f = math.modf(w * p)
        return a, b, c, d, e, f""",
    "arith": INNER + """
        local a, b, c, d = v + w, v - p, v * w, v / p
        local e, f = math.deg(v), math.rad(-w)
        local g, h = math.min(v, w, p), math.max(v, w) * math.abs(v - w)
        return a, b, c, d, e, f, g, h""",
}

# the `extreme` group: such values scaled so that intermediate products, quotients and atan2's bookkeeping pass through the subnormal range
# and near overflow, and latlon_to_ray's narrowing to float (which flags half of everything at 2^-30).  Flags are free here.  The first
# three are the scripts that found the holes of DESIGN.md section 5, each with the tuple it was found at.
EXTREME_PROBES = {
    "found_atan2": ("""
        local u = math.sin(x)
        local v = math.tanh(y)
        return math.atan2(u, v)""", [(2.0950642976666754e-231, 1.2257718596839592e-160, 0.0)]),
    "found_subnormal": ("""
        local u = math.sin(x) * 1e-160
        local v = math.cos(y) * 1e-150
        local a = u * v
        local b = u / (v * 1e300)
        return a, b""", [(-8.633357169193324e-06, -129995.95248942303, 0.0)]),
    "found_tiny": ("""
        local u = math.sin(x) * y
        local a = math.tanh(u)
        local b = math.sqrt(math.abs(u))
        return a, b""", [(9.713854227694006e-275, 1.2817197854403765e-39, 0.0)]),
    "atan2_scaled": ("""
        local u = math.sin(x)
        local v = math.tanh(y) + 2
        local a = math.atan2(u * 1e-160, v * 1e-150)
        local b = math.atan2(u * 1e-140, v * 1e-140)
        local c = math.atan2(v * 1e-200, u * 1e-160 * 1e-150)
        return a, b, c""", []),
    "atan2_overflow": ("""
        local u = math.sin(x)
        local v = math.tanh(y) + 2
        local a = math.atan2(u * 1e300, v * 1e200 * 1e100)
        local b = math.atan2(u * 1e150, v * 1e160)
        return a, b""", []),
    "near_threshold": ("""
        local u = math.sin(x) * 1e-140
        local v = (math.cos(y) + 1.5) * 1e-145
        local a = u * v
        local b = u / (1 / v)
        local c = math.sqrt(math.abs(u * v)) * 1e-140
        local d = math.tanh(u * v * 1e-3)
        local e = (u * v) % 1e-287
        return a, b, c, d, e""", []),
    "subnormal_mixed": ("""
        local u = math.sin(x) * 1e-160
        local v = math.tanh(y) * 1e-150
        local a = (u * v) % 1e-315
        local b = math.fmod(u * 1e-150, v * 1e-160 + 1e-312)
        local c = (u * 1e-100) ^ 2
        local d = math.log(math.abs(u * v) + 1e-318)
        local e = math.min(u * v, v * 1e-170) * 1e10
        local f = (u * 1e-150) + (v * 1e-160)
        local g = u * 1e-200 - v * 1e-200 * 1e-10
        return a, b, c, d, e, f, g""", []),
    "overflow": ("""
        local u = math.sin(x)
        local v = math.cos(y) + 2
        local a = (u * 1e154) * (v * 1e154)
        local b = math.cosh(math.tanh(z) * 700) * 1e4 * v
        local c = (u * 1e200) / (v * 1e-108)
        local d = (v * 1e153) ^ 2
        local e = math.exp(v * 236) * u
        return a, b, c, d, e""", []),
    "overflow_always": ("""
        local u = math.sin(x)
        local v = math.cos(y) + 2
        local a = (u * 1e300) * (v * 1e200)
        local b = math.cosh(z) * 1e300 * v
        return a, b, u""", []),
    "narrowing": ("""
        local v, w = math.sin(x), math.tanh(y) * 3
        local a, b, c = latlon_to_ray(v, w)
        local d, e = ray_to_latlon(v, w, math.cos(z))
        return a, b, c, d, e""", []),
}

# the same scalings on EXACT arguments only (no libm call upstream): nothing may be flagged and every bound is exactly 0
EXACT_PROBE = """
    local a = x * 1e-160 * (y * 1e-150)
    local b = (x * 1e-160) / (y * 1e-150 * 1e300)
    local c = (x * 1e300) * (y * 1e200)
    local d = x * 1e-200 * 1e-200 + z * 1e-200 * 1e-200
    local e = math.sqrt(math.abs(x * 1e-160 * 1e-160))
    local f = (x * 1e-160 * 1e-160) % (y * 1e-300)
    local g = math.fmod(x * 1e-310, y * 1e-320) - z * 1e-315
    local h = math.abs(x * 1e-320) * 0.5
    return a, b, c, d, e, f, g, h"""


def make_context(bk, src, name, device=None, host_math=True):
    """a context with the probe lens loaded, sized and zoomed as tests/test_script_fuzz_gpu.py does for its sized lenses"""
    import scripts as S
    ctx = bk.Context(bk.ffi.DEVICE_NONE) if device is None else bk.Context()
    ctx.set_host_math(host_math)
    ctx.load_globe(S.script("globes", "cube"), "cube.lua")
    ctx.load_lens(src, name + ".lua")
    ctx.set_zoom(*S.zoom_args(ctx.lens_info().onload.decode()))
    ctx.resize(96, 64)
    return ctx


ERR_LOOP = 16                                    # BK_ERR_LOOP of bk_build_params.h


def eval_host_errs(bk, ctx, which, args):
    """Context.eval_host_many that survives run-time errors: (out [n, 8], nout [n]) with nout = -100 - ERR_LOOP where the interpreter
    ran out of its execution budget - what bk_debug_eval_device reports for BK_ERR_LOOP"""
    out = np.full((len(args), 8), np.nan)
    nout = np.empty(len(args), np.int32)
    for i, a in enumerate(args):
        try:
            r = ctx.eval_host(which, *[float(v) for v in a])
        except bk.BlinkyError as e:
            assert "execution budget" in str(e), (a, str(e))
            nout[i] = -100 - ERR_LOOP
            continue
        if r is None:
            nout[i] = -1
        else:
            nout[i] = len(r)
            out[i, : len(r)] = r
    return out, nout


def same_bits(a, b):
    """elementwise: identical bit patterns, or NaN beside NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def first_mismatch(ok, args, *cols):
    """assertion message: the first failing tuple and what each side has there"""
    i = int(np.argmax(~ok))
    return f"tuple {i}: args {[float(v).hex() for v in args[i]]} = {args[i].tolist()}: " + " vs ".join(repr(float(c[i])) for c in cols)
