"""TEST INFRASTRUCTURE: the seam table (bk_read_seam_table) and the seam-aware bilinear apply (bk_apply_rgba_fb_bilinear_seams_device) in
numpy - no GPU, no kernel code.

1. seam_table: uint32 [6][4][ps + 2] for globes WITHOUT a globe_plate callback, from build_params_head's plate vectors: plate_uv_to_ray
   (fisheye.c:1198) in float32 as bk_lens_priv.h writes VectorMA and VectorNormalize, the max-dot plate choice (:2023-2050) and the plate
   position of :2055-2062 / :2065 / :1988 / :1971 as subtexel_model.plane_model writes them.  seam_table_loops is the second formulation:
   one virtual texel at a time, numpy float32 / float64 scalars.
2. seam_frame: subtexel_model.bilinear_frame with each of the four positions resolved on its own - inside the plate: that texel;
   outside: the table's entry for the virtual texel (the corner entry when both coordinates are outside); a NULL entry, or one into a
   plate that is not given, is the clamped own-plate texel.  seam_frame_loops: pixel by pixel.
3. read_mask: the texels the call may read."""
import numpy as np

import subtexel_model as SM

NULL = SM.NULL
f32 = np.float32


def virtual_texels(ps):
    """(x, y) int64 [4][ps + 2] of the virtual texels: edge 0 row y = -1, 1 row y = ps, 2 column x = -1, 3 column x = ps"""
    along = np.arange(-1, ps + 1)
    x = np.stack([along, along, np.full(ps + 2, -1), np.full(ps + 2, ps)])
    y = np.stack([np.full(ps + 2, -1), np.full(ps + 2, ps), along, along])
    return x, y


def slot(ps, x, y):
    """(edge, index) of the table entry for virtual texel (x, y), one coordinate at least outside [0, ps - 1]: rows own the corners"""
    if y < 0 or y >= ps:
        return (0 if y < 0 else 1), x + 1
    return (2 if x < 0 else 3), y + 1


def _plate_uv_to_ray(head, p, u, v):
    """float32 [3][...]: VectorMA three times from zero, then VectorNormalize (float32 but for the root)"""
    fu, fv = (u - 0.5).astype(f32), (-(v - 0.5)).astype(f32)
    fwd, right, up = head["forward"][p], head["right"][p], head["up"][p]
    dist = f32(head["dist"][p])
    ray = [f32(0) + dist * fwd[k] for k in range(3)]
    ray = [ray[k] + fu * right[k] for k in range(3)]
    ray = [ray[k] + fv * up[k] for k in range(3)]
    assert all(np.asarray(r).dtype == f32 for r in ray)
    length = (ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]
    length = np.sqrt(length.astype(np.float64)).astype(f32)
    il = (f32(1) / np.where(length != 0, length, f32(1))).astype(f32)
    return [np.where(length != 0, r * il, r).astype(f32) for r in ray]


def seam_table(head):
    """head: subtexel_model.build_params_head(ctx) plus "dist" (float32 [n], bk_get_globe's) -> uint32 [6][4][ps + 2]"""
    ps, n = head["ps"], len(head["dist64"])
    out = np.full((6, 4, ps + 2), NULL, np.uint32)
    x, y = virtual_texels(ps)
    u, v = (x + 0.5) / ps, (y + 0.5) / ps
    for p in range(n):
        ray = _plate_uv_to_ray(head, p, u, v)
        q = np.zeros(u.shape, np.int64)
        best = np.full(u.shape, -2.0, f32)
        for i in range(n):
            dp = SM._dot3(ray, head["forward"][i])
            take = dp > best
            best, q = np.where(take, dp, best), np.where(take, i, q)
        pick = lambda name: [head[name][q, k] for k in range(3)]
        px_ = SM._dot3(pick("right"), ray).astype(np.float64)
        py_ = SM._dot3(pick("up"), ray).astype(np.float64)
        pz_ = SM._dot3(pick("forward"), ray).astype(np.float64)
        with np.errstate(all="ignore"):
            tu = px_ / pz_ * head["dist64"][q] + 0.5
            tv = -py_ / pz_ * head["dist64"][q] + 0.5
            inside = (tu >= 0) & (tu <= 1) & (tv >= 0) & (tv <= 1)
            tx = np.trunc(np.where(inside, tu, 0.0) * ps).astype(np.int64)
            ty = np.trunc(np.where(inside, tv, 0.0) * ps).astype(np.int64)
        ok = inside & (q != p) & (tx >= 0) & (tx < ps) & (ty >= 0) & (ty < ps)
        out[p] = np.where(ok, q * ps * ps + ty * ps + tx, NULL).astype(np.uint32)
    return out


def seam_table_loops(head):
    """the same, one virtual texel at a time on numpy scalars"""
    ps, n = head["ps"], len(head["dist64"])
    out = np.full((6, 4, ps + 2), NULL, np.uint32)
    dot = lambda a, b: f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))
    for p in range(n):
        for edge in range(4):
            for i in range(ps + 2):
                x = -1 if edge == 2 else ps if edge == 3 else i - 1
                y = -1 if edge == 0 else ps if edge == 1 else i - 1
                u, v = (np.float64(x) + 0.5) / ps - 0.5, -((np.float64(y) + 0.5) / ps - 0.5)
                ray = [f32(0)] * 3
                for scale, vec in ((f32(head["dist"][p]), head["forward"][p]), (f32(u), head["right"][p]), (f32(v), head["up"][p])):
                    ray = [f32(ray[k] + f32(scale * vec[k])) for k in range(3)]
                length = f32(np.sqrt(np.float64(dot(ray, ray))))
                if length:
                    il = f32(f32(1) / length)
                    ray = [f32(r * il) for r in ray]
                q, best = 0, np.float64(-2)
                for k in range(n):
                    dp = np.float64(dot(ray, head["forward"][k]))
                    if dp > best:
                        q, best = k, dp
                if q == p:
                    continue
                px_, py_, pz_ = (np.float64(dot(head[name][q], ray)) for name in ("right", "up", "forward"))
                with np.errstate(all="ignore"):
                    tu, tv = px_ / pz_ * head["dist64"][q] + 0.5, -py_ / pz_ * head["dist64"][q] + 0.5
                if not (0 <= tu <= 1 and 0 <= tv <= 1):
                    continue
                tx, ty = int(tu * ps), int(tv * ps)
                if 0 <= tx < ps and 0 <= ty < ps:
                    out[p, edge, i] = q * ps * ps + ty * ps + tx
    return out


# ---- the frame ------------------------------------------------------------------------------------------------------------------------
def positions(off, sub, ps, table, given=(True,) * 6):
    """per entry and per position j (0: ya xa, 1: ya xb, 2: yb xa, 3: yb xb): int64 arrays [4][...] plate, y, x of the texel it is, and
    bool `resolved` - it came through the table.  NULL entries give plate 0, texel 0"""
    idx = np.where(off != NULL, off, 0).astype(np.int64)
    plate, rem = idx // (ps * ps), idx % (ps * ps)
    py, px = rem // ps, rem % ps
    s = np.asarray(sub).astype(np.int64)
    sx, sy = (s & 255) + 128, (s >> 8) + 128
    xa, ya = px - 1 + (sx >> 8), py - 1 + (sy >> 8)
    T = np.asarray(table, np.uint32).reshape(6, 4, ps + 2)
    given = np.asarray(given, bool)
    P, Y, X, R = [], [], [], []
    for yn, xn in ((ya, xa), (ya, xa + 1), (ya + 1, xa), (ya + 1, xa + 1)):
        oy, ox = (yn < 0) | (yn >= ps), (xn < 0) | (xn >= ps)
        edge = np.where(oy, np.where(yn < 0, 0, 1), np.where(xn < 0, 2, 3))
        i = np.clip(np.where(oy, xn + 1, yn + 1), 0, ps + 1)
        E = T[plate, edge, i].astype(np.int64)
        ep = np.where(E != NULL, E // (ps * ps), 0)
        use = (oy | ox) & (E != NULL) & given[ep]
        erem = E % (ps * ps)
        P.append(np.where(use, ep, plate))
        Y.append(np.where(use, erem // ps, np.clip(yn, 0, ps - 1)))
        X.append(np.where(use, erem % ps, np.clip(xn, 0, ps - 1)))
        R.append(use)
    return np.stack(P), np.stack(Y), np.stack(X), np.stack(R), sx & 255, sy & 255


def seam_frame(plates, off, sub, tints, W, H, ps, rows, lut, frame, x0, y0, table, given=(True,) * 6):
    """the call's effect on `frame` (subtexel_model.bilinear_frame's arguments, then the seam table and which plates are passed)"""
    r0, r1 = rows
    o = np.asarray(off, np.uint32).reshape(H, W)[r0:r1]
    s = np.asarray(sub, np.uint16).reshape(H, W)[r0:r1]
    t = np.asarray(tints).reshape(H, W)[r0:r1].astype(np.int64)
    mapped = o != NULL
    P, Y, X, _, fx, fy = positions(o, s, ps, table, given)
    tex = np.asarray(plates)
    a = [SM._tinted(tex[P[j], Y[j], X[j]], t, lut).astype(np.int64) for j in range(4)]
    fx, fy = fx[..., None], fy[..., None]
    h0 = a[0] * (256 - fx) + a[1] * fx
    h1 = a[2] * (256 - fx) + a[3] * fx
    out = ((h0 * (256 - fy) + h1 * fy + 32768) >> 16).astype(np.uint8)
    for c in range(4):
        window = frame[y0 + r0:y0 + r1, 4 * x0 + c:4 * (x0 + W):4]
        window[mapped] = out[..., c][mapped]
    return frame


def seam_frame_loops(plates, off, sub, tints, W, H, ps, rows, lut, frame, x0, y0, table, given=(True,) * 6):
    """the same, pixel by pixel, the four weights multiplied out"""
    T = np.asarray(table, np.uint32).reshape(6, 4, ps + 2)
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
            fx, fy = sx & 255, sy & 255
            w = [(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy]
            where = []
            for yn, xn in ((ya, xa), (ya, xa + 1), (ya + 1, xa), (ya + 1, xa + 1)):
                here = (plate, min(max(yn, 0), ps - 1), min(max(xn, 0), ps - 1))
                if not (0 <= xn < ps and 0 <= yn < ps):
                    edge, i = slot(ps, xn, yn)
                    E = int(T[plate, edge, i])
                    if E != NULL and given[E // (ps * ps)]:
                        here = (E // (ps * ps), E % (ps * ps) // ps, E % ps)
                where.append(here)
            for c in range(4):
                a = [int(plates[p][yy][xx][c]) for p, yy, xx in where]
                if lut is not None and t < 6:
                    a = [int(lut[c][t][v]) for v in a]
                frame[y0 + ly][4 * (x0 + lx) + c] = (sum(wi * ai for wi, ai in zip(w, a)) + 32768) >> 16
    return frame


def read_mask(off, sub, ps, table):
    """bool [6][ps][ps]: subtexel_model.read_mask and, for every named texel on its plate's first or last row or column, the table's
    targets of its virtual neighbours"""
    mask = SM.read_mask(off, sub, ps)
    T = np.asarray(table, np.uint32).reshape(6, 4, ps + 2)
    o = np.asarray(off, np.uint32).reshape(-1)
    o = np.unique(o[o != NULL].astype(np.int64))
    plate, rem = o // (ps * ps), o % (ps * ps)
    py, px = rem // ps, rem % ps
    targets = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yn, xn = py + dy, px + dx
            oy, ox = (yn < 0) | (yn >= ps), (xn < 0) | (xn >= ps)
            edge = np.where(oy, np.where(yn < 0, 0, 1), np.where(xn < 0, 2, 3))
            i = np.clip(np.where(oy, xn + 1, yn + 1), 0, ps + 1)
            E = T[plate, edge, i][oy | ox]
            targets.append(E[E != NULL].astype(np.int64))
    E = np.concatenate(targets)
    mask.reshape(-1)[E] = True
    return mask


def head_of(ctx):
    """build_params_head plus the plates' float dist (bk_get_globe): what seam_table wants"""
    head = SM.build_params_head(ctx)
    head["dist"] = np.array([p.dist for p in ctx.globe()], f32)
    return head
