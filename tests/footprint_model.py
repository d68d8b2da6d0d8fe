"""TEST INFRASTRUCTURE: the lensmap's FOOTPRINT in numpy, no GPU and no built library (bk_plate_footprint's expectation in
tests/test_footprint_gpu.py; tests/test_footprint_model_cpu.py holds it to a second formulation and to counts recorded from the oracle).

A globe slot on the device is 6 plates of gp = round_up(ps, 64) by ph = round_up(ps, 8) texels, stored as tiles of 16 x 8 texels; tile
(ty, tx) of a plate holds the texels px in [16 tx, 16 tx + 16), py in [8 ty, 8 ty + 8).  The footprint of a lensmap (its owned rows) is
the set of tiles some non-NULL entry reads.  Entries are in the reference layout, plate * ps^2 + py * ps + px; tints play no part."""
import numpy as np

NULL = 0xFFFFFFFF
PLATES = 6
# configurations (arguments of oracle_ffi.lensmap) whose footprint is PARTIAL, with the tiles read per plate as the CPU oracle gives them
PARTIAL = {
    ("cube", "panini", None, 640, 480): [1800, 876, 876, 0, 444, 436],                 # of 1800
    ("cube", "panini", "f_fov 120", 322, 203): [273, 62, 63, 0, 0, 0],                # of 338
    ("cube", "stereographic", "f_vfov 90", 300, 500): [442, 0, 0, 0, 21, 15],         # of 722
}
# ... the two whose plates test_footprint_gpu.py uploads through the footprint to see what stays untouched outside it (ps 203, ps 300)
UNTOUCHED_OUTSIDE = [("cube", "panini", "f_fov 120", 322, 203), ("cube", "stereographic", "f_vfov 90", 300, 500)]
FULL = ("cube", "hammer", None, 960, 540)                  # every tile of every plate is read


def tile_grid(ps):
    """(tile rows, tile columns) of a plate on the device, padding included: (ph / 8, gp / 16)"""
    return ((ps + 7) // 8, ((ps + 63) // 64) * 4)


def tiles_inside(ps):
    """tiles of a plate that hold a texel: ceil(ps / 8) * ceil(ps / 16) (the rest of tile_grid is padding, never read)"""
    return ((ps + 7) // 8) * ((ps + 15) // 16)


def footprint(offsets, W, H, ps, rows=None):
    """offsets: the WHOLE table, uint32 [H * W]; rows = (r0, r1) the owned rows (default all) -> (masks uint8 [6][ph/8][gp/16] with 1 = read,
    counts [6], rects [6] of (x0, y0, x1, y1) in texels: half-open, tile-granular, clipped to ps, all 0 for a plate nothing reads)"""
    r0, r1 = rows if rows is not None else (0, H)
    o = np.asarray(offsets, dtype=np.uint32).reshape(H, W)[r0:r1].ravel()
    o = o[o != NULL].astype(np.int64)
    plate, rem = o // (ps * ps), o % (ps * ps)
    py, px = rem // ps, rem % ps
    th, tw = tile_grid(ps)
    masks = np.zeros((PLATES, th, tw), np.uint8)
    keep = plate < PLATES                                  # (an entry past the globe reads nothing: bk_set_lensmap turns it into NULL)
    masks[plate[keep], py[keep] // 8, px[keep] // 16] = 1
    counts = [int(m.sum()) for m in masks]
    rects = []
    for m in masks:
        ys, xs = np.nonzero(m)
        if len(ys) == 0:
            rects.append((0, 0, 0, 0))
        else:
            rects.append((16 * int(xs.min()), 8 * int(ys.min()), min(16 * (int(xs.max()) + 1), ps), min(8 * (int(ys.max()) + 1), ps)))
    return masks, counts, rects


def texel_mask(mask, ps):
    """a plate's tile mask [ph/8][gp/16] -> bool [ps][ps]: the texels of the tiles read"""
    return np.repeat(np.repeat(mask.astype(bool), 8, axis=0), 16, axis=1)[:ps, :ps]
