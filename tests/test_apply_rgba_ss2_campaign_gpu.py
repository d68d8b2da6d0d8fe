"""Randomised launch SEQUENCES with the supersampling apply in them (bk_apply_rgba_ss2_device, plain and tinted) against the CPU oracle:
the second family of tests/rgbagen.py (sequence_ss2).  One context per seed as in tests/test_apply_rgba_campaign_gpu.py - frames down to
1x1 with W and H odd, stripes of two rows and the lone last row of an odd H, rings that are no multiple of four, forced and measured
block heights, staging buffers of 1 KiB, both upload paths - and 4-7 launches on it, at least half of them ss2 into HALF-SIZE frames at
any pitch, origin, frame stride and 0 / 4 / 8 bytes into the allocation, the others full-size launches of both flavours and 8-bit ones on
the same block maps, with a second lensmap or a LUT changed in place in front of an ss2 launch.  After EVERY launch the whole destination
allocation is compared byte for byte with rgbagen.expected: an ss2 frame's values are quad_means' (tests/test_apply_rgba_ss2_gpu.py: the
oracle's 8-bit apply of every byte plane, (sum + n // 2) // n over the mapped samples of a quad), everything else keeps its fill.
tests/test_rgba_campaign_cpu.py holds that expectation to a second model and counts what the committed seeds reach.
The committed range runs in the suite; BLINKY_RGBA_SS2_CAMPAIGN=lo:hi runs a longer developer campaign.  Byte-exact, nothing filtered."""
import os

import numpy as np
import pytest

import rgbagen as G
from test_apply_rgba_campaign_gpu import _upload

pytestmark = pytest.mark.gpu


def _seeds():
    v = os.environ.get("BLINKY_RGBA_SS2_CAMPAIGN")
    if not v:
        return G.COMMITTED_SS2
    lo, hi = [int(x) for x in v.split(":")]
    return range(lo, hi)


@pytest.mark.parametrize("seed", _seeds())
def test_random_ss2_launch_sequence(seed):
    import blinky_amd as bk
    import torch
    seq = G.sequence_ss2(seed)
    W, H, r0, r1 = seq["W"], seq["H"], seq["r0"], seq["r1"]
    pal = G.palette(seq)
    globes = {}

    def slots(s):
        if s not in globes:
            globes[s] = G.slot_globe(seq, s)
        return globes[s]

    ctx = bk.Context()
    ctx.set_frames(seq["R"])
    ctx.resize(W, H)
    ctx.set_rows(r0, r1)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_blockmap_tuning(seq["tuning"])
    if seq["shape"]:
        ctx.set_tile_shape(seq["shape"])
    if seq["ldskb"]:
        ctx.set_tile_shape(400 + seq["ldskb"])
    ctx.set_ablation(seq["ablation"])
    keep = []
    _upload(ctx, seq, slots, keep)

    def set_lensmap(off, tints):
        ctx.set_lensmap(off.reshape(H, W)[r0:r1].ravel(), tints.reshape(H, W)[r0:r1].ravel())

    set_lensmap(*seq["tables"][0][:2])
    for i, L, off, tints, lut, ev in G.walk(seq):
        if ev == "set_lensmap":
            set_lensmap(off, tints)
        want = G.expected(seq, L, off, tints, lut, pal, slots)
        out = torch.full((G.alloc_bytes(L),), G.FILL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0
        ptr = out.data_ptr() + L["ptr_off"]
        kw = dict(nframes=L["nframes"], x0=L["x0"], y0=L["y0"])
        if L["kind"] == "apply8":
            ctx.apply_device(ptr, L["pitch"], L["stride"], frame0=L["first"], rubix_on=L["rubix"], pal=pal, **kw)
        elif L["kind"] in G.SS2_KINDS:
            ctx.apply_rgba_ss2_device(ptr, L["pitch"], L["stride"], globe0=L["first"], lut=lut, **kw)
        elif lut is None:
            ctx.apply_rgba_device(ptr, L["pitch"], L["stride"], globe0=L["first"], **kw)
        else:
            ctx.apply_rgba_tinted_device(ptr, L["pitch"], L["stride"], lut, globe0=L["first"], **kw)
        torch.cuda.synchronize()
        if L["kind"] != "apply8" and seq["shape"] and seq["ldskb"]:
            # preconditions, never filters.  Where the census counts a list larger than the staging buffer, the block map just launched
            # must have sent blocks to the direct gather (the statistic counts in 1 KiB bins: asked only where the list is a bin larger) ...
            tinted = L["kind"] in G.TINTED_KINDS
            if max(G.block_chunks(off, tints, seq, seq["shape"], False)) * 16 > (seq["ldskb"] + 1) * 1024:
                st = ctx.tile_stats()
                assert st["slow"] > 0, f"{G.describe(seq, i)}: no block on the direct gather: {st}"
            # ... and where it counts a fully mapped table as STAGED (the wide stores: the same bin the other way), none
            what = seq["tables"][1 if len(seq["tables"]) > 1 and off is seq["tables"][1][0] else 0][2]
            if L["kind"] in G.SS2_KINDS and G.wide_staged(seq, what, lambda: G.block_chunks(off, tints, seq, seq["shape"], tinted)):
                st = ctx.tile_stats()
                assert st["slow"] == 0, f"{G.describe(seq, i)}: blocks on the direct gather: {st}"
        got = out.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            at = int(bad[0])
            f, rest = divmod(max(at - L["ptr_off"], 0), L["stride"])
            y, xb = divmod(rest, L["pitch"])
            half = " of the HALF-SIZE frame" if L["kind"] in G.SS2_KINDS else ""
            raise AssertionError(f"{G.describe(seq, i)}\n{len(bad)} of {got.size} bytes differ, first at byte {at} of the allocation = frame {f}, "
                                 f"y {y}, x {xb // (1 if L['kind'] == 'apply8' else 4)}, byte {xb % (1 if L['kind'] == 'apply8' else 4)} "
                                 f"(frame coordinates{half}, origin ({L['x0']},{L['y0']}) not subtracted): got {got[at]} want {want[at]}")
    ctx.close()
