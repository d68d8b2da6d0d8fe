"""The level-of-detail plane at DEPTH: bk_read_lod against tests/trilinear_model.py's derivation where rho passes 2^16 - at platesize 203
it stays below 203 * 256, and the power-of-two boundaries of k = floor(log2 rho) occur only where random neighbours happen to produce
them.  A DIRECTED ramp table (TM.ramp_case: one row per rho in 2^k - 1, 2^k, 2^k + 1 up to the largest step a plate of 1025 allows,
2^18 + 1) on a stripe of a 1027 x 1025 frame, and one drawn table through a whole 515 x 513 frame (levels 0 to 9 from random
neighbours, W % 4 = 3, gp = 576: 36 tiles a row, no power of two).  tests/test_trilinear_cpu.py holds the ramp to the pixel loop and to
the census of what it has to place.  Every comparison is exact equality."""
import numpy as np
import pytest

import test_apply_rgba_fb_bilinear_gpu as BL
import trilinear_model as TM

pytestmark = pytest.mark.gpu

RAMP = (1025, 1027)                                                     # ps, W (H = ps)
DRAWN = (515, 513)


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def biases(ps):
    """-300, 0, 300 and the bias that puts the deepest ramp row (rho = 2^kmax + 1) exactly on the top level, fraction 0"""
    top = (len(TM.level_sizes(ps)) - 1) * 256
    return (-300, 0, 300, top - int(TM.lod_value(TM.ramp_steps(ps)[-1], 0, TM.MAX_LEVELS)))


def assert_plane(got, want, W, r0, what):
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {want.size} pixels differ, the first at (x {at % W}, y {r0 + at // W}): "
                             f"{int(got[at])}, expected {int(want[at])}")


def test_the_ramp(bk):
    ps, W = RAMP
    table, sub, rows = TM.ramp_case(ps, W)
    off, tints, W, H, ps = table
    r0, r1 = rows
    assert r0 % 8 != 0 and H == ps
    ctx = BL.make_ctx(bk, table, sub, rows=rows)
    o, s = off.reshape(H, W)[r0:r1].reshape(-1), sub.reshape(H, W)[r0:r1].reshape(-1)
    for bias in biases(ps):
        ctx.set_lod_bias(bias)
        assert_plane(ctx.read_lod(), TM.derive_lod(o, s, W, r1 - r0, ps, bias), W, r0, f"ramp ps {ps} bias {bias}")
    ctx.close()


def test_a_drawn_table_through_a_whole_deep_frame(bk):
    W, H = DRAWN
    table, sub = BL.drawn_case(W, H)
    off, tints, _, _, ps = table
    ctx = BL.make_ctx(bk, table, sub)
    for bias in biases(ps):
        ctx.set_lod_bias(bias)
        assert_plane(ctx.read_lod(), TM.derive_lod(off, sub, W, H, ps, bias), W, 0, f"drawn {W}x{H} bias {bias}")
    ctx.close()
