"""TEST INFRASTRUCTURE: the sub-texel plane (bk_set_subtexel) and the bilinear frame-buffer apply (bk_apply_rgba_fb_bilinear_device) in
numpy - no GPU, no kernel code.

1. bilinear_frame: what the call writes, from (reference-layout table, sub plane, tints, six row-major plates uint8 [6][ps][ps][4], LUT).
   bilinear_frame_loops is the second formulation it is held to (tests/test_subtexel_cpu.py): plain Python loops with the four weight
   products written out, (sum of w * a + 32768) >> 16.
2. plane_model: the plane itself (and the table beside it) for lenses whose lens_inverse uses only + - * / - no libm, nothing flagged:
   float narrowing, VectorNormalize as bk_vector_normalize writes it (mathlib.c:413), the max-dot plate choice (fisheye.c:2023-2050),
   the plate position of :2055-2062 and the split at :1988 into the texel and the eight fraction bits the plane keeps.  Plate vectors and
   dist64 come from bk_debug_build_params (build_params_head)."""
import ctypes as C

import numpy as np

NULL = 0xFFFFFFFF
CENTRE = 0x8080

# libm-free lenses (both callbacks: calc_zoom's f_fov goes through lens_forward); RAYS = the same lens_inverse in numpy, float64
FLAT_LENS = 'max_fov = 170\nmax_vfov = 170\nonload = "f_fov 130"\nfunction lens_inverse(x, y)\n   return x, y, 1\nend\n' \
            'function lens_forward(x, y, z)\n   return x / z, y / z\nend\n'
SHEARED_LENS = 'max_fov = 170\nmax_vfov = 170\nonload = "f_fov 150"\nfunction lens_inverse(x, y)\n   return x + 0.375 * y, y - 0.25 * x, 1\nend\n' \
               'function lens_forward(x, y, z)\n   return x / z, y / z\nend\n'
RAYS = {"flat": lambda x, y: (x, y, np.ones_like(x)), "sheared": lambda x, y: (x + 0.375 * y, y - 0.25 * x, np.ones_like(x))}
LIBM_FREE = {"flat": FLAT_LENS, "sheared": SHEARED_LENS}


class _Plate(C.Structure):
    _fields_ = [("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("fov", C.c_float), ("dist", C.c_float),
                ("dist64", C.c_double)]


class _Head(C.Structure):
    """BkBuildParams (bk_build_params.h) up to its plates"""
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("row0", C.c_int), ("rows", C.c_int), ("ps", C.c_int), ("gp", C.c_int), ("ph", C.c_int),
                ("numplates", C.c_int), ("has_globe_plate", C.c_int), ("scale", C.c_double), ("rubix_block", C.c_double),
                ("rubix_pad", C.c_double), ("rubix_unit_px", C.c_double), ("grid_bits", C.c_uint * 256), ("grid_n", C.c_int),
                ("plates", _Plate * 6)]


def build_params_head(ctx):
    """dict(W, H, row0, rows, ps, scale, forward / right / up float32 [n][3], dist64 float64 [n]) of ctx.build_params()"""
    h = _Head.from_buffer_copy(bytes(ctx.build_params())[: C.sizeof(_Head)])
    n = h.numplates
    vec = lambda name: np.array([list(getattr(h.plates[i], name)) for i in range(n)], np.float32)
    return dict(W=h.W, H=h.H, row0=h.row0, rows=h.rows, ps=h.ps, scale=h.scale, forward=vec("forward"), right=vec("right"), up=vec("up"),
                dist64=np.array([h.plates[i].dist64 for i in range(n)], np.float64))


def _dot3(a, b):
    """mathlib.h:70 in float: ((a0 * b0 + a1 * b1) + a2 * b2), every operation rounded to float32"""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def plane_model(head, rays):
    """-> (offsets uint32 in the reference layout, sub uint16), both [rows * W], of the owned rows of `head` for lens_inverse = rays"""
    W, H, ps, row0, rows, scale = head["W"], head["H"], head["ps"], head["row0"], head["rows"], head["scale"]
    ly, lx = np.divmod(np.arange(rows * W), W)
    ly = ly + row0
    y = (-(ly - H // 2)).astype(np.float64) * scale                     # :2100
    x = (lx - W // 2).astype(np.float64) * scale                        # :2105
    ray = [np.asarray(r, np.float64).astype(np.float32) for r in rays(x, y)]      # :1559-1561
    length = (ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]      # VectorNormalize, float32 throughout but for the root
    assert length.dtype == np.float32
    length = np.sqrt(length.astype(np.float64)).astype(np.float32)
    ilength = (np.float32(1) / np.where(length != 0, length, np.float32(1))).astype(np.float32)
    ray = [np.where(length != 0, r * ilength, r) for r in ray]
    assert all(r.dtype == np.float32 for r in ray)
    plate = np.zeros(rows * W, np.int64)                                # :2023-2050: the first strict maximum from -2 on
    best = np.full(rows * W, -2.0, np.float32)
    for i in range(len(head["dist64"])):
        dp = _dot3(ray, head["forward"][i])
        take = dp > best
        best = np.where(take, dp, best)
        plate = np.where(take, i, plate)
    pick = lambda name: [head[name][plate, k] for k in range(3)]
    px_ = _dot3(pick("right"), ray).astype(np.float64)                  # :2055-2057
    py_ = _dot3(pick("up"), ray).astype(np.float64)
    pz_ = _dot3(pick("forward"), ray).astype(np.float64)
    with np.errstate(all="ignore"):
        u = px_ / pz_ * head["dist64"][plate] + 0.5                     # :2061
        v = -py_ / pz_ * head["dist64"][plate] + 0.5                    # :2062
        inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)              # :2065
        us, vs = np.where(inside, u, 0.0) * ps, np.where(inside, v, 0.0) * ps
    px, py = np.trunc(us).astype(np.int64), np.trunc(vs).astype(np.int64)        # :1988
    mapped = inside & (px >= 0) & (px < ps) & (py >= 0) & (py < ps)               # :1971
    qx = ((us - px) * 256.0).astype(np.int64)
    qy = ((vs - py) * 256.0).astype(np.int64)
    off = np.where(mapped, plate * ps * ps + py * ps + px, NULL).astype(np.uint32)
    sub = np.where(mapped, qx | (qy << 8), CENTRE).astype(np.uint16)
    return off, sub


# ---- the bilinear frame -------------------------------------------------------------------------------------------------------------
def neighbours(off, sub, ps):
    """per entry (int64 arrays shaped like off; NULL entries give plate 0, texel 0): plate, xa, xb, ya, yb, fx, fy"""
    idx = np.where(off != NULL, off, 0).astype(np.int64)
    plate, rem = idx // (ps * ps), idx % (ps * ps)
    py, px = rem // ps, rem % ps
    s = np.asarray(sub).astype(np.int64)
    sx, sy = (s & 255) + 128, (s >> 8) + 128
    xa, ya = px - 1 + (sx >> 8), py - 1 + (sy >> 8)
    xb, yb = xa + 1, ya + 1
    clamp = lambda a: np.clip(a, 0, ps - 1)
    return plate, clamp(xa), clamp(xb), clamp(ya), clamp(yb), sx & 255, sy & 255


def _tinted(tex, t, lut):
    """uint8 [..., 4] texels through the pixel's tint (int64 [...]): lut[c][t][v] where t < 6"""
    if lut is None:
        return tex
    out = tex.copy()
    classed = t < 6
    tt = np.where(classed, t, 0)
    for c in range(4):
        out[..., c] = np.where(classed, np.asarray(lut)[c][tt, tex[..., c]], tex[..., c])
    return out


def bilinear_frame(plates, off, sub, tints, W, H, ps, rows, lut, frame, x0, y0):
    """the call's effect on `frame` (uint8 [frame rows][pitch bytes], holding the background; changed in place).  off / sub / tints cover
    the WHOLE frame ([H * W]); only the owned rows [r0, r1) are written, at pixel (x0, y0 + r0)"""
    r0, r1 = rows
    o = np.asarray(off, np.uint32).reshape(H, W)[r0:r1]
    s = np.asarray(sub, np.uint16).reshape(H, W)[r0:r1]
    t = np.asarray(tints).reshape(H, W)[r0:r1].astype(np.int64)
    mapped = o != NULL
    plate, xa, xb, ya, yb, fx, fy = neighbours(o, s, ps)
    P = np.asarray(plates)
    tex = lambda yy, xx: _tinted(P[plate, yy, xx], t, lut).astype(np.int64)
    a00, a01, a10, a11 = tex(ya, xa), tex(ya, xb), tex(yb, xa), tex(yb, xb)
    fx, fy = fx[..., None], fy[..., None]
    h0 = a00 * (256 - fx) + a01 * fx
    h1 = a10 * (256 - fx) + a11 * fx
    out = ((h0 * (256 - fy) + h1 * fy + 32768) >> 16).astype(np.uint8)
    for c in range(4):
        window = frame[y0 + r0:y0 + r1, 4 * x0 + c:4 * (x0 + W):4]
        window[mapped] = out[..., c][mapped]
    return frame


def bilinear_frame_loops(plates, off, sub, tints, W, H, ps, rows, lut, frame, x0, y0):
    """the same, pixel by pixel, with the four weights multiplied out: (w00 a00 + w01 a01 + w10 a10 + w11 a11 + 32768) >> 16"""
    r0, r1 = rows
    for ly in range(r0, r1):
        for lx in range(W):
            o = int(off[ly * W + lx])
            if o == NULL:
                continue
            plate, rem = divmod(o, ps * ps)
            py, px = divmod(rem, ps)
            s, t = int(sub[ly * W + lx]), int(tints[ly * W + lx])
            sx, sy = (s & 255) + 128, (s >> 8) + 128
            xa, ya = px - 1 + (sx >> 8), py - 1 + (sy >> 8)
            xb, yb = min(xa + 1, ps - 1), min(ya + 1, ps - 1)
            xa, ya = max(xa, 0), max(ya, 0)
            fx, fy = sx & 255, sy & 255
            w = [(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy]
            for c in range(4):
                a = [int(plates[plate][yy][xx][c]) for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]
                if lut is not None and t < 6:
                    a = [int(lut[c][t][v]) for v in a]
                frame[y0 + ly][4 * (x0 + lx) + c] = (sum(wi * ai for wi, ai in zip(w, a)) + 32768) >> 16
    return frame


def read_mask(off, sub, ps):
    """bool [6][ps][ps]: the texels the call may read - within one texel of a named one, clamped to the plate (the four it blends lie inside)"""
    o = np.asarray(off, np.uint32).reshape(-1)
    o = o[o != NULL].astype(np.int64)
    mask = np.zeros((6, ps, ps), bool)
    plate, rem = o // (ps * ps), o % (ps * ps)
    py, px = rem // ps, rem % ps
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            mask[plate, np.clip(py + dy, 0, ps - 1), np.clip(px + dx, 0, ps - 1)] = True
    return mask
