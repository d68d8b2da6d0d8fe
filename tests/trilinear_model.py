"""TEST INFRASTRUCTURE: the trilinear frame-buffer apply (bk_apply_rgba_fb_trilinear_device) in numpy - no GPU, no kernel code.

1. pyramid: the mip levels of a plate ((a + b + c + d + 2) >> 2 over clamped coordinates, each level from the rounded one below).
2. derive_lod: the level-of-detail plane from a reference-layout table and its sub-texel plane (neighbour differences, the
   piecewise-linear log2, bias, clamp); ramp_case: a directed table that places chosen values of rho.
3. trilinear_frame: what the call writes.  Every level's four texels and weights come from subtexel_model.neighbours - the bilinear
   stage itself - handed (Uk >> 8, Uk & 255) in the place of (px, qx) and s_k in the place of ps.
Each has a second formulation in plain Python loops (*_loops) that tests/test_trilinear_cpu.py holds it to."""
import numpy as np

import subtexel_model as SM

NULL = SM.NULL
MAX_LEVELS = 16


def level_sizes(ps):
    """[s_0 = ps, s_1, ..., 1]"""
    sizes = [ps]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


# ---- 1. the pyramid -------------------------------------------------------------------------------------------------------------------
def pyramid(plates):
    """plates uint8 [..., ps, ps, 4] -> [level 0 (the plates), level 1, ...], level k uint8 [..., s_k, s_k, 4]"""
    levels = [np.asarray(plates)]
    for s in level_sizes(levels[0].shape[-2])[1:]:
        below = levels[-1].astype(np.int64)
        sb = below.shape[-2]
        a, b = np.minimum(2 * np.arange(s), sb - 1), np.minimum(2 * np.arange(s) + 1, sb - 1)
        take = lambda yy, xx: below[..., yy, :, :][..., xx, :]
        levels.append(((take(a, a) + take(a, b) + take(b, a) + take(b, b) + 2) >> 2).astype(np.uint8))
    return levels


def pyramid_loops(plate):
    """one plate uint8 [ps][ps][4], texel by texel"""
    levels = [np.asarray(plate)]
    for s in level_sizes(levels[0].shape[0])[1:]:
        below, sb = levels[-1], levels[-1].shape[0]
        out = np.zeros((s, s, 4), np.uint8)
        for y in range(s):
            for x in range(s):
                xs, ys = (min(2 * x, sb - 1), min(2 * x + 1, sb - 1)), (min(2 * y, sb - 1), min(2 * y + 1, sb - 1))
                for c in range(4):
                    out[y][x][c] = (sum(int(below[yy][xx][c]) for yy in ys for xx in xs) + 2) // 4
        levels.append(out)
    return levels


# ---- 2. the level of detail -----------------------------------------------------------------------------------------------------------
def lod_value(rho, bias, levels):
    """int64 array rho (1/256 texel) -> level << 8 | fraction, biased and clamped to [0, (levels - 1) * 256]"""
    rho = np.asarray(rho, np.int64)
    big = rho > 256
    r = np.where(big, rho, 512)
    k = np.floor(np.log2(r.astype(np.float64))).astype(np.int64)       # (exact: rho < 2^24 is a float64 integer, log2 of a power of two is exact)
    k = np.where((1 << k) > r, k - 1, np.where((1 << (k + 1)) <= r, k + 1, k))
    v = np.where(big, (k - 8) * 256 + ((r << 8) >> k) - 256, 0)
    return np.clip(v + int(bias), 0, (levels - 1) * 256)


def lod_value_loops(rho, bias, levels):
    """one value, by comparison against powers of two"""
    v = 0
    if rho > 256:
        k = 8
        while 2 ** (k + 1) <= rho:
            k += 1
        v = (k - 8) * 256 + (rho * 256) // 2 ** k - 256
    return min(max(v + bias, 0), (levels - 1) * 256)


def positions(off, sub, ps):
    """(mapped, plate, U, V), int64, shaped like off"""
    off = np.asarray(off, np.uint32)
    m = off != NULL
    idx = np.where(m, off, 0).astype(np.int64)
    plate, rem = idx // (ps * ps), idx % (ps * ps)
    s = np.asarray(sub).astype(np.int64)
    return m, plate, (rem % ps) * 256 + (s & 255), (rem // ps) * 256 + (s >> 8)


def derive_lod(off, sub, W, rows, ps, bias=0, detail=False):
    """off (reference layout), sub: the OWNED rows, [rows * W] -> uint16 [rows * W]; detail: also dict(h=, v=) of int8 [rows][W]:
    1 = the step went forward, -1 = backward, 0 = none (unmapped pixels 0), other_plate = mapped neighbours refused for their plate, and
    rho = int64 [rows][W], the larger of the two steps in 1/256 texel (what lod_value is given; meaningless where unmapped)"""
    m, plate, U, V = (a.reshape(rows, W) for a in positions(off, sub, ps))
    steps, way, refused = [], {}, 0
    for axis, name in ((1, "h"), (0, "v")):
        def shifted(a, by, fill):
            out = np.full_like(a, fill)
            src = [slice(None)] * 2
            dst = [slice(None)] * 2
            src[axis], dst[axis] = (slice(by, None), slice(None, -by)) if by > 0 else (slice(None, by), slice(-by, None))
            out[tuple(dst)] = a[tuple(src)]
            return out
        cand = []
        for by in (1, -1):
            m2, p2, U2, V2 = shifted(m, by, False), shifted(plate, by, -1), shifted(U, by, 0), shifted(V, by, 0)
            refused += int((m & m2 & (p2 != plate)).sum())
            cand.append((m & m2 & (p2 == plate), np.maximum(np.abs(U2 - U), np.abs(V2 - V))))
        (okf, df), (okb, db) = cand
        steps.append(np.where(okf, df, np.where(okb, db, 0)))
        way[name] = np.where(okf, 1, np.where(okb, -1, 0)).astype(np.int8)
    rho = np.maximum(steps[0], steps[1])
    lod = np.where(m, lod_value(rho, bias, len(level_sizes(ps))), 0).astype(np.uint16).reshape(-1)
    return (lod, dict(way, other_plate=refused, rho=rho)) if detail else lod


def derive_lod_loops(off, sub, W, rows, ps, bias=0):
    levels = len(level_sizes(ps))
    out = np.zeros(rows * W, np.uint16)

    def pos(y, x):
        o = int(off[y * W + x])
        if o == NULL:
            return None
        plate, rem = divmod(o, ps * ps)
        s = int(sub[y * W + x])
        return plate, (rem % ps) * 256 + (s & 255), (rem // ps) * 256 + (s >> 8)

    for y in range(rows):
        for x in range(W):
            me = pos(y, x)
            if me is None:
                continue
            rho = 0
            for cands in (((y, x + 1), (y, x - 1)), ((y + 1, x), (y - 1, x))):
                for yy, xx in cands:
                    if 0 <= xx < W and 0 <= yy < rows:
                        other = pos(yy, xx)
                        if other is not None and other[0] == me[0]:
                            rho = max(rho, abs(other[1] - me[1]), abs(other[2] - me[2]))
                            break
            out[y * W + x] = lod_value_loops(rho, bias, levels)
    return out


def ramp_steps(ps):
    """the values of rho a ramp table places on purpose: 2^k - 1, 2^k, 2^k + 1 for k = 8 (the rho <= 256 edge: 255, 256, 257) up to
    floor(log2((ps - 1) * 256)), the largest power of two a step inside one plate can reach; ps >= 2"""
    kmax = ((ps - 1) * 256).bit_length() - 1
    return [(1 << k) + d for k in range(8, kmax + 1) for d in (-1, 0, 1)]


def ramp_case(ps, W, r0=3, H=None):
    """((off, tints, W, H, ps), sub, (r0, r1)), H = ps unless given (a model may be handed any H): a DIRECTED table for the level of detail.  One row per value of ramp_steps(ps), from
    row r0 on, everything else NULL.  Row i lies on plate i % 6 at one V, so both vertical neighbours are refused for their plate and the
    vertical step is 0; along the row U starts below 255 and advances by the row's step, turning round where it would leave
    [0, (ps - 1) * 256 + 255], so |dU| is the step at every pixel; a NULL every 97 pixels sends its left neighbour to the backward step.
    rho is therefore the row's step at every mapped pixel of it (W >= 3)."""
    steps = ramp_steps(ps)
    H, umax = H or ps, (ps - 1) * 256 + 255
    assert W >= 3 and ps >= 2 and r0 + len(steps) <= H
    off = np.full((H, W), NULL, np.uint32)
    sub = np.full((H, W), SM.CENTRE, np.uint16)
    for i, step in enumerate(steps):
        u, way, us = (37 * i + 11) % 255, 1, []
        for _ in range(W):
            us.append(u)
            if not 0 <= u + way * step <= umax:
                way = -way
            u += way * step
            assert 0 <= u <= umax
        U, V = np.array(us, np.int64), ((5 * i + 1) % ps) * 256 + (29 * i) % 256
        off[r0 + i] = (i % 6) * ps * ps + (V >> 8) * ps + (U >> 8)
        sub[r0 + i] = (U & 255) | ((V & 255) << 8)
        off[r0 + i, 50::97] = NULL
    tints = np.full(H * W, 255, np.uint8)
    return (off.reshape(-1), tints, W, H, ps), sub.reshape(-1), (r0, r0 + len(steps))


# ---- 3. the frame ---------------------------------------------------------------------------------------------------------------------
def level_v(level, size, plate, U, V, k, t, lut):
    """the UNROUNDED blend at level k (uint8 [6][size][size][4]) of every pixel: int64 [..., 4]; the four texels and the weights are
    subtexel_model.neighbours' for the texel (Uk >> 8, Vk >> 8) of a plate of side `size` with sub Uk & 255 | (Vk & 255) << 8"""
    Uk, Vk = U >> k, V >> k
    off_k = (plate * size * size + (Vk >> 8) * size + (Uk >> 8)).astype(np.uint32)
    _, xa, xb, ya, yb, fx, fy = SM.neighbours(off_k, (Uk & 255) | ((Vk & 255) << 8), size)
    tex = lambda yy, xx: SM._tinted(level[plate, yy, xx], t, lut).astype(np.int64)
    a00, a01, a10, a11 = tex(ya, xa), tex(ya, xb), tex(yb, xa), tex(yb, xb)
    fx, fy = fx[..., None], fy[..., None]
    return (a00 * (256 - fx) + a01 * fx) * (256 - fy) + (a10 * (256 - fx) + a11 * fx) * fy


def trilinear_frame(pyr, off, sub, lod, tints, W, H, ps, rows, lut, frame, x0, y0):
    """the call's effect on `frame` (uint8 [frame rows][pitch bytes], changed in place).  pyr = pyramid(plates [6][ps][ps][4]) - or any
    list of levels: level 0 is what the call is given as plates, the others what the pyramid holds; off / sub / tints cover the WHOLE
    frame ([H * W]), lod the OWNED rows [r0, r1) only, which are written at pixel (x0, y0 + r0)"""
    r0, r1 = rows
    o = np.asarray(off, np.uint32).reshape(H, W)[r0:r1]
    s = np.asarray(sub, np.uint16).reshape(H, W)[r0:r1]
    t = np.asarray(tints).reshape(H, W)[r0:r1].astype(np.int64)
    d = np.asarray(lod).reshape(r1 - r0, W).astype(np.int64)
    mapped, plate, U, V = positions(o, s, ps)
    top = len(pyr) - 1
    lo, fl = d >> 8, (d & 255)[..., None]
    hi = np.minimum(lo + 1, top)
    assert (lo[mapped] <= top).all()
    v_lo, v_hi = np.zeros(o.shape + (4,), np.int64), np.zeros(o.shape + (4,), np.int64)
    for k, level in enumerate(pyr):
        if not ((lo == k) | (hi == k))[mapped].any():
            continue
        v = level_v(np.asarray(level), level.shape[1], plate, U, V, k, t, lut)
        v_lo = np.where((lo == k)[..., None], v, v_lo)
        v_hi = np.where((hi == k)[..., None], v, v_hi)
    total = v_lo * (256 - fl) + v_hi * fl + (1 << 23)
    assert (total[mapped] < 1 << 32).all()
    out = (total >> 24).astype(np.uint8)
    for c in range(4):
        window = frame[y0 + r0:y0 + r1, 4 * x0 + c:4 * (x0 + W):4]
        window[mapped] = out[..., c][mapped]
    return frame


def trilinear_frame_loops(pyr, off, sub, lod, tints, W, H, ps, rows, lut, frame, x0, y0):
    """the same, pixel by pixel, the eight weights multiplied out: (sum of w * a + 2^23) >> 24"""
    r0, r1 = rows
    top = len(pyr) - 1
    for ly in range(r0, r1):
        for lx in range(W):
            o = int(off[ly * W + lx])
            if o == NULL:
                continue
            plate, rem = divmod(o, ps * ps)
            s, t, d = int(sub[ly * W + lx]), int(tints[ly * W + lx]), int(lod[(ly - r0) * W + lx])
            U, V = (rem % ps) * 256 + (s & 255), (rem // ps) * 256 + (s >> 8)
            l, fl = d >> 8, d & 255
            terms = []                                                 # (weight, level, y, x)
            for k, wl in ((l, 256 - fl), (min(l + 1, top), fl)):
                size = pyr[k].shape[1]
                Uk, Vk = U >> k, V >> k
                sx, sy = (Uk & 255) + 128, (Vk & 255) + 128
                xa, ya = (Uk >> 8) - 1 + (sx >> 8), (Vk >> 8) - 1 + (sy >> 8)
                xb, yb = min(xa + 1, size - 1), min(ya + 1, size - 1)
                xa, ya = max(xa, 0), max(ya, 0)
                fx, fy = sx & 255, sy & 255
                terms += [(wl * (256 - fx) * (256 - fy), k, ya, xa), (wl * fx * (256 - fy), k, ya, xb), (wl * (256 - fx) * fy, k, yb, xa),
                          (wl * fx * fy, k, yb, xb)]
            assert sum(w for w, _, _, _ in terms) == 1 << 24
            for c in range(4):
                a = [int(pyr[k][plate][yy][xx][c]) for _, k, yy, xx in terms]
                if lut is not None and t < 6:
                    a = [int(lut[c][t][v]) for v in a]
                frame[y0 + ly][4 * (x0 + lx) + c] = (sum(w * v for (w, _, _, _), v in zip(terms, a)) + (1 << 23)) >> 24
    return frame


def random_lods(n, ps, seed):
    """uint16 [n]: every level as the lower one, fractions 0, 1, 127, 128, 255 half the time; the top level with fraction 0"""
    rng = np.random.default_rng(9100 + seed)
    top = len(level_sizes(ps)) - 1
    level = rng.integers(0, top + 1, n)
    frac = np.where(rng.random(n) < 0.5, np.array([0, 1, 127, 128, 255])[rng.integers(0, 5, n)], rng.integers(0, 256, n))
    return np.minimum(level * 256 + frac, top * 256).astype(np.uint16)
