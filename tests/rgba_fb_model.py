"""TEST INFRASTRUCTURE: what bk_apply_rgba_fb_device writes, in numpy, no GPU and no built library (the expectation of
tests/test_apply_rgba_fb_gpu.py; tests/test_rgba_fb_abi.py holds it to rgbagen.oracle_frame on committed campaign seeds).

The call warps one truecolour frame out of six row-major plates, so the model indexes plates[plate][py][px] - uint8 [6][ps][ps][4] -
through the REFERENCE-layout table (entry = plate * ps^2 + py * ps + px, 0xFFFFFFFF = NULL): byte c of a mapped pixel whose tint t is
below 6 becomes lut[c][t][byte]; ss2 = the rounded mean (s + n // 2) // n over the mapped samples of a 2x2 quad, tinted per sample."""
import numpy as np

NULL = 0xFFFFFFFF


def samples(plates, off, tints, W, H, ps, rows, lut):
    """-> (texels uint8 [r1 - r0][W][4], mapped bool [r1 - r0][W]) of the owned rows: what every mapped pixel of a full-size frame gets"""
    r0, r1 = rows
    o = np.asarray(off, dtype=np.uint32).reshape(H, W)[r0:r1]
    mapped = o != NULL
    idx = np.where(mapped, o, 0).astype(np.int64)
    plate, rem = idx // (ps * ps), idx % (ps * ps)
    tex = np.asarray(plates)[plate, rem // ps, rem % ps].copy()
    if lut is not None:
        t = np.asarray(tints).reshape(H, W)[r0:r1].astype(np.int64)
        classed = t < 6
        tt = np.where(classed, t, 0)
        for c in range(4):
            tex[..., c] = np.where(classed, np.asarray(lut)[c][tt, tex[..., c]], tex[..., c])
    return tex, mapped


def fb_frame(plates, off, tints, W, H, ps, rows, lut, ss2, frame, x0, y0):
    """the call's effect on `frame` (uint8 [frame rows][pitch bytes], holding the background; changed in place): full size - the owned
    rows [r0, r1) at pixel (x0, y0 + r0); ss2 - output rows [r0 // 2, (r1 + 1) // 2) of the half-size frame, Wo = (W + 1) // 2 wide
    (r0 even, r1 even or H: every quad of those rows lies inside the stripe or hangs below the frame)"""
    r0, r1 = rows
    tex, mapped = samples(plates, off, tints, W, H, ps, rows, lut)
    if not ss2:
        for c in range(4):
            window = frame[y0 + r0:y0 + r1, 4 * x0 + c:4 * (x0 + W):4]
            window[mapped] = tex[..., c][mapped]
        return frame
    assert r0 % 2 == 0 and (r1 % 2 == 0 or r1 == H)
    n_rows, Wo = (r1 - r0 + 1) // 2, (W + 1) // 2
    m = np.zeros((2 * n_rows, 2 * Wo), np.int64)
    m[:r1 - r0, :W] = mapped
    v = np.zeros((2 * n_rows, 2 * Wo, 4), np.int64)
    v[:r1 - r0, :W] = tex
    v *= m[:, :, None]
    n = m.reshape(n_rows, 2, Wo, 2).sum(axis=(1, 3))
    s = v.reshape(n_rows, 2, Wo, 2, 4).sum(axis=(1, 3))
    mean = ((s + (n // 2)[:, :, None]) // np.maximum(n, 1)[:, :, None]).astype(np.uint8)
    for c in range(4):
        window = frame[y0 + r0 // 2:y0 + r0 // 2 + n_rows, 4 * x0 + c:4 * (x0 + Wo):4]
        window[n > 0] = mean[..., c][n > 0]
    return frame


def plates_of_planes(planes):
    """four 8-bit globes (byte planes, uint8 [6][ps][ps] each) -> uint8 [6][ps][ps][4]"""
    return np.stack([np.asarray(p) for p in planes], axis=-1)
