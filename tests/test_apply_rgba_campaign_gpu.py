"""Randomised launch SEQUENCES of the truecolour apply (bk_apply_rgba_device, bk_apply_rgba_tinted_device) against the CPU oracle:
tests/rgbagen.py draws one context per seed - frames down to 1x1 and off every alignment, stripes of one row, rings that are no multiple of
four, tables no lens produces, forced and measured block heights, small staging buffers, both upload paths - and 4-7 launches on it that
change flavour (plain, tinted, 8-bit), kind (1 frame, up to 4, 5 and more: 4, <= 16 and > 16 planes for the block map's tuning), pitch,
origin, frame stride and pointer alignment, with a second lensmap or a LUT changed in place in the middle.  After EVERY launch the whole
destination allocation is compared byte for byte with rgbagen.expected: byte plane c of a frame is the oracle's 8-bit render_lensmap
(O.apply, fisheye.c:2406-2424) of plane c, through pal = lut[c] with rubix for a tinted launch; everything else keeps its fill.
tests/test_rgba_campaign_cpu.py holds that expectation to a second model and counts what the committed seeds reach.
The committed range runs in the suite; BLINKY_RGBA_CAMPAIGN=lo:hi runs a longer developer campaign.  Byte-exact, nothing filtered."""
import os

import numpy as np
import pytest

import rgbagen as G

pytestmark = pytest.mark.gpu


def _seeds():
    v = os.environ.get("BLINKY_RGBA_CAMPAIGN")
    if not v:
        return G.COMMITTED
    lo, hi = [int(x) for x in v.split(":")]
    return range(lo, hi)


def _upload(ctx, seq, slots, keep):
    """truecolour globe g = slots 4g .. 4g+3 through the path drawn for it; the slots behind the last whole globe as 8-bit globes"""
    import torch
    ps, G4 = seq["ps"], 4 * seq["G"]
    rng = np.random.default_rng(seq["seed"])
    for g, u in enumerate(seq["uploads"]):
        for p in range(6):
            texels = np.stack([slots(4 * g + c)[p] for c in range(4)], axis=-1)       # [ps][ps][4]
            if u["path"] == "host":
                ctx.upload_plate_rgba(g, p, texels)
            else:
                pitch = 4 * ps + u["extra"]
                src = rng.integers(0, 256, (ps, pitch), dtype=np.uint8)               # (the bytes right of the plate are never read as texels)
                src[:, :4 * ps] = texels.reshape(ps, 4 * ps)
                dev = torch.from_numpy(src).cuda()
                keep.append(dev)
                ctx.upload_plate_rgba_device(g, p, dev.data_ptr(), pitch)
    ctx.synchronize()
    for s in range(G4, seq["R"]):
        for p in range(6):
            ctx.upload_plate(s, p, slots(s)[p])


@pytest.mark.parametrize("seed", _seeds())
def test_random_truecolour_launch_sequence(seed):
    import blinky_amd as bk
    import torch
    seq = G.sequence(seed)
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
        if L["kind"] == "apply8":
            ctx.apply_device(ptr, L["pitch"], L["stride"], frame0=L["first"], nframes=L["nframes"], x0=L["x0"], y0=L["y0"],
                             rubix_on=L["rubix"], pal=pal)
        elif lut is None:
            ctx.apply_rgba_device(ptr, L["pitch"], L["stride"], globe0=L["first"], nframes=L["nframes"], x0=L["x0"], y0=L["y0"])
        else:
            ctx.apply_rgba_tinted_device(ptr, L["pitch"], L["stride"], lut, globe0=L["first"], nframes=L["nframes"], x0=L["x0"], y0=L["y0"])
        torch.cuda.synchronize()
        if L["kind"] != "apply8" and seq["shape"] and seq["ldskb"]:
            # a precondition, never a filter: where the census counts a list larger than the staging buffer, the block map just launched
            # must have sent blocks to the direct gather (the statistic counts in 1 KiB bins: asked only where the list is a bin larger)
            if max(G.block_chunks(off, tints, seq, seq["shape"], False)) * 16 > (seq["ldskb"] + 1) * 1024:
                st = ctx.tile_stats()
                assert st["slow"] > 0, f"{G.describe(seq, i)}: no block on the direct gather: {st}"
        got = out.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            at = int(bad[0])
            f, rest = divmod(max(at - L["ptr_off"], 0), L["stride"])
            y, xb = divmod(rest, L["pitch"])
            raise AssertionError(f"{G.describe(seq, i)}\n{len(bad)} of {got.size} bytes differ, first at byte {at} of the allocation = frame {f}, "
                                 f"y {y}, x {xb // (1 if L['kind'] == 'apply8' else 4)}, byte {xb % (1 if L['kind'] == 'apply8' else 4)} "
                                 f"(frame coordinates, origin ({L['x0']},{L['y0']}) not subtracted): got {got[at]} want {want[at]}")
    ctx.close()
