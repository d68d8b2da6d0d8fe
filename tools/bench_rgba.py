#!/usr/bin/env python3
"""Truecolour apply against the 8-bit batch launch that moves the same bytes (GPU only).

At 3840x2160 cube/panini and cube/hammer, over the 64-slot LCG ring of the bench's headline job:
  A  one bk_apply_device launch of 64 8-bit frames into planar 8-bit frames (the 8-bit path, unchanged)
  B  one bk_apply_rgba_device launch of 16 truecolour frames from the same slots (slot 4g+c = byte plane c of truecolour globe g)
B's output is compared with A's plane by plane before anything is timed.  Timing: HIP events on the context's stream, warm-up
launches first, regions of at least --region seconds made of ten event-timed trains of launches (a region's figure is the median
train), A / B / A / B ... alternated --repeats times inside this one process.  The target: B's median <= A's median + A's own spread
(max - min of A's region medians).  usage: python tools/bench_rgba.py [--lenses panini,hammer] [--repeats 5] [--out FILE] [--tint] [--ss2] [--upload] [--fb [--bilinear [--seams] | --trilinear]]

--tint: the same protocol for f_rubix on truecolour frames, three launches alternated A' / B' / B:
  A'  one bk_apply_device launch of 64 8-bit frames with rubix_on = 1 (existing code: the same bytes through the same number of LUT
      passes per chunk)
  B'  one bk_apply_rgba_tinted_device launch of 16 truecolour frames with lut[c] = that same palette for all four c
  B   the plain truecolour launch
B' must equal A' plane by plane before anything is timed.  The target: B''s median <= A''s median + A''s own spread.

--ss2 [--tint]: the same protocol for the fused 2x2 supersampling, on one context at the supersampled size, A / B alternated:
  A  one bk_apply_rgba_device (--tint: bk_apply_rgba_tinted_device) launch of 16 full-size truecolour frames
  B  one bk_apply_rgba_ss2_device launch over the same globes (--tint: through the same tables) into 16 half-size frames
B must equal the numpy average of A's full-size output (mapped samples only, (sum + n // 2) // n) before anything is timed.  B reads
what A reads and stores a quarter of its bytes; the expectation: B's median <= A's median + A's own spread.

--upload [--reps 31]: the per-frame loop of a live renderer, one truecolour globe per frame from device plates (16-byte aligned):
  A  bk_upload_plate_rgba_device of every displayed plate
  B  bk_upload_plate_rgba_footprint_device of the same plates (only the tiles the lensmap reads)
  P  the one-frame bk_apply_rgba_device behind either; A + P and B + P are the frame
The frame after B must equal the frame after A byte for byte before anything is timed.  Frames rotate through 16 truecolour globes and 4
sets of source plates (out of the Infinity Cache by the time their turn comes again), A and B alternate frame by frame, --repeats blocks of
--reps frames each way; a figure is the median of the block medians, its spread their max - min.  Printed with the footprint's tile
count and the byte model (8 bytes per texel of every chunk / tile written).  The expectations: cube/hammer (footprint = everything)
B <= A + A's spread; cube/panini B / A reported next to the tile ratio.

--fb [--tint] [--ss2] [--reps 31]: the same live renderer with and without the globe, alternated frame by frame:
  B + P  bk_upload_plate_rgba_footprint_device of every displayed plate, then the one-frame bk_apply_rgba_device (--tint:
         bk_apply_rgba_tinted_device, --ss2: bk_apply_rgba_ss2_device, with --tint through the same tables) - existing code
  D      bk_apply_rgba_fb_device straight from the same plates: no upload, no globe, no block map
D's frame must equal B + P's byte for byte before anything is timed.  The source is a ring of 16 sets of six device plates (1.8 GB at 4K,
16-byte aligned) advanced every frame, so the texels come from HBM and not from the Infinity Cache; B + P also rotates through 16
truecolour globes.  --repeats blocks of --reps frames each way; a figure is the median of the block medians, its spread their max - min.
The expectation: D < B + P by more than the two spreads together; D against P alone is printed beside it (what a caller whose globes
stay resident would pay).

--fb --bilinear --seams [--tint] [--reps 31]: L (bk_apply_rgba_fb_bilinear_device, its kernel unchanged) against S
  (bk_apply_rgba_fb_bilinear_seams_device with the cube's computed seam table), alternated frame by frame as below; S is held to the numpy
  model (tests/seam_model.py) at full size before anything is timed; the target is S <= L + the two spreads.  Also: the host cost of making
  the seam table at this platesize, without and with a globe_plate callback.
--fb --trilinear [--tint] [--reps 31]: L (bk_apply_rgba_fb_bilinear_device, its kernel unchanged), T0 and T (bk_apply_rgba_fb_trilinear_device
  without and with making the mip pyramid) and M (the pyramid by itself: bk_debug_mip_pyramid, its two launches and no apply), alternated
  frame by frame as below; T is held to the numpy model of tests/trilinear_model.py at full size before anything is timed.
--fb --bilinear [--tint] [--reps 31]: bilinear texel filtering against the nearest-texel launch it extends, alternated frame by frame:
  D  bk_apply_rgba_fb_device (--tint: with the tables) - existing code
  L  bk_apply_rgba_fb_bilinear_device from the same plates through the sub-texel plane the build kept (bk_set_subtexel)
L's frame must equal the numpy model of tests/subtexel_model.py at full size before anything is timed.  The same ring of 16 plate sets
and the same fill in front of every timed frame as --fb.  There is no pass / fail ratio: L reads the 16.6 MB plane on top of D's bytes and
up to three neighbours per pixel that mostly share the named texel's lines; L, D, L / D and the spreads are printed.  The build's side is
timed too: bk_build of the same lens with the switch off and on, alternated (--repeats pairs, bk_last_build_ms)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import blinky_amd  # noqa: E402
import scripts as S  # noqa: E402

W, H, SLOTS = 3840, 2160, 64


def region(stream, launch, per_train, trains=10):
    """median over `trains` event-timed trains of `per_train` launches: seconds per launch"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(trains + 1)]
    ev[0].record(stream)
    for t in range(trains):
        for _ in range(per_train):
            launch()
        ev[t + 1].record(stream)
    ev[-1].synchronize()
    return statistics.median(ev[t].elapsed_time(ev[t + 1]) * 1e-3 / per_train for t in range(trains))


def measure(lens, repeats, region_s):
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(SLOTS)
    S.configure(ctx, "cube", lens, None, (W, H))
    ctx.build()
    for f in range(SLOTS):
        for p in range(6):
            ctx.fill_plate_lcg(f, p, seed_frame=f)
    out_a = torch.zeros((SLOTS, H, W), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((SLOTS // 4, H, W, 4), dtype=torch.uint8, device="cuda")

    def a():
        ctx.apply_device(out_a.data_ptr(), W, H * W, frame0=0, nframes=SLOTS)

    def b():
        ctx.apply_rgba_device(out_b.data_ptr(), 4 * W, 4 * W * H, globe0=0, nframes=SLOTS // 4)

    for _ in range(3):                                     # warm-up: the first launch compiles and tunes the block map both share
        a()
        b()
    torch.cuda.synchronize()
    # B against A, plane by plane: byte c of truecolour frame f = 8-bit frame 4f + c
    planar = out_b.permute(0, 3, 1, 2).reshape(SLOTS, H, W)
    if not torch.equal(planar, out_a):
        bad = int((planar != out_a).sum())
        raise SystemExit(f"{lens}: the truecolour frames differ from the 8-bit frames of the same slots in {bad} bytes - nothing timed")
    del planar
    # launches per train: a region of ten trains lasts at least region_s
    pilot = min(region(stream, a, 4, trains=3), region(stream, b, 4, trains=3))
    per_train = max(2, int(region_s / 10 / pilot) + 1)
    ra, rb = [], []
    for _ in range(repeats):
        ra.append(region(stream, a, per_train))
        rb.append(region(stream, b, per_train))
    tm = ctx.traffic_model()
    st = ctx.tile_stats()
    ctx.close()
    med_a, med_b, spread = statistics.median(ra), statistics.median(rb), max(ra) - min(ra)
    visit = max(1, tm["frames_per_visit"] // 4)            # truecolour frames per block visit
    # two byte models per truecolour frame, both with every mapped pixel stored once and the block map read once per visit: "staged" counts
    # a globe line once per block that stages it, "compulsory" once per frame (DESIGN.md 3's model: L2 serves what blocks share)
    bytes_frame = 4 * (tm["mapped_pixels"] + 128 * tm["staged_lines"]) + tm["blockmap_bytes_per_visit"] / visit
    bytes_min = 4 * (tm["mapped_pixels"] + 128 * tm["unique_globe_lines"]) + tm["blockmap_bytes_per_visit"] / visit
    return dict(lens=lens, W=W, H=H, block=f"128x{st['tile_h'] % 1000}", lds_kib=st["lds_bytes_per_wave"] // 1024, launches_per_train=per_train,
                region_s=10 * per_train * med_a, a_regions_us=[t * 1e6 for t in ra], b_regions_us=[t * 1e6 for t in rb],
                a_us=med_a * 1e6, b_us=med_b * 1e6, a_spread_us=spread * 1e6, b_over_a=med_b / med_a,
                us_per_truecolour_frame=med_b * 1e6 / (SLOTS // 4), model_bytes_per_truecolour_frame=bytes_frame,
                implied_tb_s=bytes_frame * (SLOTS // 4) / med_b / 1e12,
                compulsory_bytes_per_truecolour_frame=bytes_min, compulsory_tb_s=bytes_min * (SLOTS // 4) / med_b / 1e12, target_met=bool(med_b <= med_a + spread))


def measure_tint(lens, repeats, region_s):
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(SLOTS)
    S.configure(ctx, "cube", lens, None, (W, H))
    ctx.build()
    for f in range(SLOTS):
        for p in range(6):
            ctx.fill_plate_lcg(f, p, seed_frame=f)
    pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
    lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    out_a = torch.zeros((SLOTS, H, W), dtype=torch.uint8, device="cuda")
    out_t = torch.zeros((SLOTS // 4, H, W, 4), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((SLOTS // 4, H, W, 4), dtype=torch.uint8, device="cuda")

    def a():
        ctx.apply_device(out_a.data_ptr(), W, H * W, frame0=0, nframes=SLOTS, rubix_on=True, pal=pal)

    def t():
        ctx.apply_rgba_tinted_device(out_t.data_ptr(), 4 * W, 4 * W * H, lut, globe0=0, nframes=SLOTS // 4)

    def b():
        ctx.apply_rgba_device(out_b.data_ptr(), 4 * W, 4 * W * H, globe0=0, nframes=SLOTS // 4)

    for _ in range(3):                                     # warm-up: the first launches compile and tune the block map of either flavour
        a()
        t()
        b()
    torch.cuda.synchronize()
    planar = out_t.permute(0, 3, 1, 2).reshape(SLOTS, H, W)
    if not torch.equal(planar, out_a):
        bad = int((planar != out_a).sum())
        raise SystemExit(f"{lens}: the tinted truecolour frames differ from the 8-bit rubix frames of the same slots in {bad} bytes - nothing timed")
    tinted_bytes = int((out_t != out_b).sum())
    del planar
    a()                                                    # the statistics below: of the TINTED block map
    torch.cuda.synchronize()
    st = ctx.tile_stats()
    pilot = min(region(stream, a, 4, trains=3), region(stream, t, 4, trains=3), region(stream, b, 4, trains=3))
    per_train = max(2, int(region_s / 10 / pilot) + 1)
    ra, rt, rb = [], [], []
    for _ in range(repeats):
        ra.append(region(stream, a, per_train))
        rt.append(region(stream, t, per_train))
        rb.append(region(stream, b, per_train))
    ctx.close()
    med_a, med_t, med_b, spread = statistics.median(ra), statistics.median(rt), statistics.median(rb), max(ra) - min(ra)
    return dict(lens=lens, W=W, H=H, tinted_block=f"128x{st['tile_h'] % 1000}", tinted_lds_kib=st["lds_bytes_per_wave"] // 1024,
                tinted_slow_blocks=st["slow"], launches_per_train=per_train, bytes_changed_by_the_tint=tinted_bytes,
                a_regions_us=[x * 1e6 for x in ra], t_regions_us=[x * 1e6 for x in rt], b_regions_us=[x * 1e6 for x in rb],
                a_us=med_a * 1e6, t_us=med_t * 1e6, b_us=med_b * 1e6, a_spread_us=spread * 1e6, t_over_a=med_t / med_a, t_over_b=med_t / med_b,
                target_met=bool(med_t <= med_a + spread))


def measure_ss2(lens, repeats, region_s, tint):
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(SLOTS)
    S.configure(ctx, "cube", lens, None, (W, H))
    ctx.build()
    for f in range(SLOTS):
        for p in range(6):
            ctx.fill_plate_lcg(f, p, seed_frame=f)
    lut = None
    if tint:
        pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
        lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    F, Wo, Ho = SLOTS // 4, (W + 1) // 2, (H + 1) // 2
    out_a = torch.zeros((F, H, W, 4), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((F, Ho, Wo, 4), dtype=torch.uint8, device="cuda")

    def a():
        if tint:
            ctx.apply_rgba_tinted_device(out_a.data_ptr(), 4 * W, 4 * W * H, lut, globe0=0, nframes=F)
        else:
            ctx.apply_rgba_device(out_a.data_ptr(), 4 * W, 4 * W * H, globe0=0, nframes=F)

    def b():
        ctx.apply_rgba_ss2_device(out_b.data_ptr(), 4 * Wo, 4 * Wo * Ho, globe0=0, nframes=F, lut=lut)

    for _ in range(3):                                     # warm-up: the first launch compiles and tunes the block map both share
        a()
        b()
    torch.cuda.synchronize()
    # B against the numpy average of A at full size: unmapped samples do not count, quads without a mapped sample stay as they were (0)
    off, _ = ctx.read_lensmap()
    mapped = (np.asarray(off).reshape(H, W) != 0xFFFFFFFF)
    del off
    n = mapped.reshape(Ho, 2, Wo, 2).sum(axis=(1, 3), dtype=np.uint32)
    div = np.maximum(n, 1)[:, :, None]
    for f in range(F):
        full = out_a[f].cpu().numpy().astype(np.uint32) * mapped[:, :, None]
        want = ((full.reshape(Ho, 2, Wo, 2, 4).sum(axis=(1, 3), dtype=np.uint32) + (n // 2)[:, :, None]) // div).astype(np.uint8)
        want[n == 0] = 0
        got = out_b[f].cpu().numpy()
        if not np.array_equal(got, want):
            raise SystemExit(f"{lens}: supersampled frame {f} differs from the average of the full-size frame in {int((got != want).sum())} bytes - nothing timed")
    del full, want, got
    pilot = min(region(stream, a, 4, trains=3), region(stream, b, 4, trains=3))
    per_train = max(2, int(region_s / 10 / pilot) + 1)
    ra, rb = [], []
    for _ in range(repeats):
        ra.append(region(stream, a, per_train))
        rb.append(region(stream, b, per_train))
    st = ctx.tile_stats()
    ctx.close()
    med_a, med_b, spread = statistics.median(ra), statistics.median(rb), max(ra) - min(ra)
    return dict(lens=lens, W=W, H=H, tint=bool(tint), block=f"128x{st['tile_h'] % 1000}", lds_kib=st["lds_bytes_per_wave"] // 1024, launches_per_train=per_train,
                quads_by_mapped_samples=[int((n == k).sum()) for k in range(5)],
                a_regions_us=[t * 1e6 for t in ra], b_regions_us=[t * 1e6 for t in rb], a_us=med_a * 1e6, b_us=med_b * 1e6,
                a_spread_us=spread * 1e6, b_spread_us=(max(rb) - min(rb)) * 1e6, b_over_a=med_b / med_a, target_met=bool(med_b <= med_a + spread))


def measure_upload(lens, repeats, reps):
    """the per-frame loop of a live renderer (INTEGRATION.md "Plates that are frame buffers"): upload the displayed plates, apply one frame.
    A = full uploads (bk_upload_plate_rgba_device), B = footprint uploads (bk_upload_plate_rgba_footprint_device), P = the one-frame apply
    behind either.  Frame k goes to truecolour globe k % 16 from source set k % 4, so neither globe nor source is in the Infinity Cache when
    its turn comes again; a 1 GiB fill in front of every timed frame keeps the GPU busy while the host enqueues the frame's launches, so the
    events time the kernels and not the host.  `repeats` blocks of `reps` frames each, A and B alternated frame by frame."""
    G, SETS = SLOTS // 4, 4
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(SLOTS)
    S.configure(ctx, "cube", lens, None, (W, H))
    display, _ = ctx.build()
    ps = min(W, H)
    shown = [p for p in range(6) if p < len(display) and display[p]]
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [[torch.randint(0, 256, (ps, ps, 4), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)] for _ in range(SETS)]
    pitch = 4 * ps
    assert all(t.data_ptr() % 16 == 0 for s in src for t in s) and pitch % 16 == 0
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    plug = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def full(g, s):
        for p in shown:
            ctx.upload_plate_rgba_device(g, p, src[s][p].data_ptr(), pitch)

    def foot(g, s):
        for p in shown:
            ctx.upload_plate_rgba_footprint_device(g, p, src[s][p].data_ptr(), pitch)

    def apply(g):
        ctx.apply_rgba_device(out.data_ptr(), 4 * W, 4 * W * H, globe0=g, nframes=1)

    # before anything is timed: the frame after B (over another source's texels) must be the frame after A, byte for byte
    fp = [ctx.plate_footprint(p) for p in range(6)]
    full(0, 0)
    apply(0)
    torch.cuda.synchronize()
    frame_a = out.clone()
    full(1, 1)
    foot(1, 0)
    out.zero_()
    apply(1)
    torch.cuda.synchronize()
    if not torch.equal(out, frame_a):
        raise SystemExit(f"{lens}: the frame after the footprint upload differs from the frame after the full upload in {int((out != frame_a).sum())} bytes - nothing timed")
    del frame_a
    for k in range(2 * G):                                 # warm-up: every globe through both uploads, the block map compiled and tuned
        (full if k % 2 else foot)(k % G, k % SETS)
        apply(k % G)
    torch.cuda.synchronize()
    blocks = {"a": [], "b": [], "pa": [], "pb": [], "ap": [], "bp": []}
    k = 0
    for _ in range(repeats):
        ev = []
        for r in range(2 * reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            plug.fill_(r & 255)
            e[0].record(stream)
            (foot if r % 2 else full)(k % G, k % SETS)
            e[1].record(stream)
            apply(k % G)
            e[2].record(stream)
            ev.append(e)
            k += 1
        torch.cuda.synchronize()
        up = [e[0].elapsed_time(e[1]) * 1e3 for e in ev]
        ap = [e[1].elapsed_time(e[2]) * 1e3 for e in ev]
        both = [e[0].elapsed_time(e[2]) * 1e3 for e in ev]
        for name, xs, odd in (("a", up, 0), ("b", up, 1), ("pa", ap, 0), ("pb", ap, 1), ("ap", both, 0), ("bp", both, 1)):
            blocks[name].append(statistics.median(xs[odd::2]))
    ctx.close()
    med = {n: statistics.median(v) for n, v in blocks.items()}
    spread = {n: max(v) - min(v) for n, v in blocks.items()}
    tiles_plate = ((ps + 7) // 8) * ((ps + 15) // 16)
    tiles = sum(fp[p][1] for p in shown)
    return dict(lens=lens, W=W, H=H, ps=ps, displayed_plates=shown, frames_per_block=reps, blocks=repeats,
                footprint_tiles=[fp[p][1] for p in range(6)], footprint_rects=[list(fp[p][0]) for p in range(6)], tiles_per_plate=tiles_plate,
                tile_ratio=tiles / (tiles_plate * len(shown)),
                model_bytes_a=8 * 16 * ((ps + 15) // 16) * ps * len(shown), model_bytes_b=8 * 128 * tiles,
                blocks_us=blocks, median_us=med, spread_us=spread, b_over_a=med["b"] / med["a"], bp_over_ap=med["bp"] / med["ap"],
                a_gb_s=8 * 16 * ((ps + 15) // 16) * ps * len(shown) / med["a"] / 1e3, b_gb_s=8 * 128 * tiles / med["b"] / 1e3,
                target_met=bool(med["b"] <= med["a"] + spread["a"]))


def measure_fb(lens, repeats, reps, tint, ss2):
    """B + P (footprint uploads into a globe + the one-frame staged apply) against D (bk_apply_rgba_fb_device from the same plates), frame
    by frame.  Frame k reads source set k % 16 (and, B + P, writes truecolour globe k % 16): by the time a set's turn comes again 1.7 GB of
    other plates and a 1 GiB fill have passed through the Infinity Cache.  The fill in front of every timed frame also keeps the GPU busy
    while the host enqueues the frame's launches, so the events time the kernels and not the host."""
    G = SETS = SLOTS // 4
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(SLOTS)
    S.configure(ctx, "cube", lens, None, (W, H))
    display, _ = ctx.build()
    ps = min(W, H)
    shown = [p for p in range(6) if p < len(display) and display[p]]
    lut = None
    if tint:
        pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
        lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [[torch.randint(0, 256, (ps, ps, 4), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)] for _ in range(SETS)]
    pitch = 4 * ps
    assert all(t.data_ptr() % 16 == 0 for s in src for t in s) and pitch % 16 == 0
    ptrs = [[src[s][p].data_ptr() if p in shown else None for p in range(6)] for s in range(SETS)]
    pitches = [pitch] * 6
    Wd, Hd = ((W + 1) // 2, (H + 1) // 2) if ss2 else (W, H)
    out = torch.zeros((Hd, Wd, 4), dtype=torch.uint8, device="cuda")
    plug = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def foot(g, s):
        for p in shown:
            ctx.upload_plate_rgba_footprint_device(g, p, src[s][p].data_ptr(), pitch)

    def staged(g):
        if ss2:
            ctx.apply_rgba_ss2_device(out.data_ptr(), 4 * Wd, 4 * Wd * Hd, globe0=g, nframes=1, lut=lut)
        elif tint:
            ctx.apply_rgba_tinted_device(out.data_ptr(), 4 * Wd, 4 * Wd * Hd, lut, globe0=g, nframes=1)
        else:
            ctx.apply_rgba_device(out.data_ptr(), 4 * Wd, 4 * Wd * Hd, globe0=g, nframes=1)

    def direct(s):
        ctx.apply_rgba_fb_device(ptrs[s], pitches, out.data_ptr(), 4 * Wd, lut=lut, ss2=ss2)

    # before anything is timed: D's frame must be B + P's, byte for byte - at full size, plain, and in the flavour that is timed
    fp = [ctx.plate_footprint(p) for p in range(6)]
    full_out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    foot(0, 0)
    ctx.apply_rgba_device(full_out.data_ptr(), 4 * W, 4 * W * H, globe0=0, nframes=1)
    torch.cuda.synchronize()
    frame_bp = full_out.clone()
    full_out.zero_()
    ctx.apply_rgba_fb_device(ptrs[0], pitches, full_out.data_ptr(), 4 * W)
    torch.cuda.synchronize()
    if not torch.equal(full_out, frame_bp):
        raise SystemExit(f"{lens}: the frame from the frame buffers differs from the frame after upload + apply in {int((full_out != frame_bp).sum())} bytes - nothing timed")
    del full_out, frame_bp
    staged(0)
    torch.cuda.synchronize()
    frame_bp = out.clone()
    out.zero_()
    direct(0)
    torch.cuda.synchronize()
    if not torch.equal(out, frame_bp):
        raise SystemExit(f"{lens}: the timed flavour's frame from the frame buffers differs from the existing path's in {int((out != frame_bp).sum())} bytes - nothing timed")
    del frame_bp
    for k in range(2 * G):                                 # warm-up: every globe and every set once each way, the block map compiled and tuned
        if k % 2:
            direct(k % SETS)
        else:
            foot(k % G, k % SETS)
            staged(k % G)
    torch.cuda.synchronize()
    blocks = {"b": [], "p": [], "bp": [], "d": []}
    k = 0
    for _ in range(repeats):
        ev = []
        for r in range(2 * reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            plug.fill_(r & 255)
            e[0].record(stream)
            if r % 2:
                direct(k % SETS)
                e[1].record(stream)
            else:
                foot(k % G, k % SETS)
                e[1].record(stream)
                staged(k % G)
            e[2].record(stream)
            ev.append(e)
            k += 1
        torch.cuda.synchronize()
        blocks["b"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[0::2]))
        blocks["p"].append(statistics.median(e[1].elapsed_time(e[2]) * 1e3 for e in ev[0::2]))
        blocks["bp"].append(statistics.median(e[0].elapsed_time(e[2]) * 1e3 for e in ev[0::2]))
        blocks["d"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[1::2]))
    off, _ = ctx.read_lensmap()
    mapped = int((np.asarray(off) != 0xFFFFFFFF).sum())
    del off
    ctx.close()
    med = {n: statistics.median(v) for n, v in blocks.items()}
    spread = {n: max(v) - min(v) for n, v in blocks.items()}
    tiles = sum(fp[p][1] for p in shown)
    # the issue's estimate of D's bytes: the lensmap once, every mapped pixel (ss2: every quad) stored once, the footprint's tiles once
    model_d = 4 * W * H + (1 if tint else 0) * W * H + 4 * (mapped // 4 if ss2 else mapped) + 4 * 128 * tiles
    return dict(lens=lens, W=W, H=H, ps=ps, tint=bool(tint), ss2=bool(ss2), displayed_plates=shown, frames_per_block=reps, blocks=repeats,
                footprint_tiles=[fp[p][1] for p in range(6)], mapped_pixels=mapped, model_bytes_d=model_d,
                blocks_us=blocks, median_us=med, spread_us=spread, d_over_bp=med["d"] / med["bp"], d_over_p=med["d"] / med["p"],
                d_model_gb_s=model_d / med["d"] / 1e3, target_met=bool(med["d"] + spread["d"] + spread["bp"] < med["bp"]))


def measure_fb_bilinear(lens, repeats, reps, tint):
    """D (bk_apply_rgba_fb_device) against L (bk_apply_rgba_fb_bilinear_device), frame by frame, from the ring of measure_fb"""
    import subtexel_model as SM
    SETS = SLOTS // 4
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(1)
    S.configure(ctx, "cube", lens, None, (W, H))
    # the build with the switch off and on, alternated: what the extra 2 bytes per pixel cost it
    build_ms = {"off": [], "on": []}
    ctx.build()
    for _ in range(repeats):
        for name, on in (("off", False), ("on", True)):
            ctx.set_subtexel(on)
            ctx.build()
            build_ms[name].append(ctx.last_build_ms())
    display, _ = ctx.build()                                # (the switch is on)
    fixups = ctx.last_build_fixups()
    ps = min(W, H)
    shown = [p for p in range(6) if p < len(display) and display[p]]
    lut = None
    if tint:
        pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
        lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [[torch.randint(0, 256, (ps, ps, 4), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)] for _ in range(SETS)]
    pitch = 4 * ps
    assert all(t.data_ptr() % 16 == 0 for s in src for t in s) and pitch % 16 == 0
    ptrs = [[src[s][p].data_ptr() if p in shown else None for p in range(6)] for s in range(SETS)]
    pitches = [pitch] * 6
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    plug = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def nearest(s):
        ctx.apply_rgba_fb_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut)

    def bilinear(s):
        ctx.apply_rgba_fb_bilinear_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut)

    # before anything is timed: L's frame is the numpy model's, at full size, in the flavour that is timed (in bands of rows: the model
    # keeps several int64 arrays of a band's size)
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    plates = np.stack([src[0][p].cpu().numpy() for p in range(6)])
    bilinear(0)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(H, 4 * W)
    want = np.zeros((H, 4 * W), np.uint8)
    for r0 in range(0, H, 120):
        SM.bilinear_frame(plates, off, sub, tints, W, H, ps, (r0, min(H, r0 + 120)), lut, want, 0, 0)
    if not np.array_equal(got, want):
        raise SystemExit(f"{lens}: the bilinear frame differs from the numpy model in {int((got != want).sum())} bytes - nothing timed")
    mapped = int((off != 0xFFFFFFFF).sum())
    moved = int((sub[off != 0xFFFFFFFF] != SM.CENTRE).sum())
    del off, tints, sub, plates, got, want
    for k in range(2 * SETS):                              # warm-up: every set once each way
        (bilinear if k % 2 else nearest)(k % SETS)
    torch.cuda.synchronize()
    blocks = {"d": [], "l": []}
    k = 0
    for _ in range(repeats):
        ev = []
        for r in range(2 * reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            plug.fill_(r & 255)
            e[0].record(stream)
            (bilinear if r % 2 else nearest)(k % SETS)
            e[1].record(stream)
            ev.append(e)
            k += 1
        torch.cuda.synchronize()
        blocks["d"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[0::2]))
        blocks["l"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[1::2]))
    fp = [ctx.plate_footprint(p) for p in range(6)]
    ctx.close()
    med = {n: statistics.median(v) for n, v in blocks.items()}
    spread = {n: max(v) - min(v) for n, v in blocks.items()}
    tiles = sum(fp[p][1] for p in shown)
    model_d = 4 * W * H + (1 if tint else 0) * W * H + 4 * mapped + 4 * 128 * tiles      # measure_fb's estimate of D's bytes
    return dict(lens=lens, W=W, H=H, ps=ps, tint=bool(tint), bilinear=True, displayed_plates=shown, frames_per_block=reps, blocks=repeats,
                footprint_tiles=[fp[p][1] for p in range(6)], mapped_pixels=mapped, pixels_off_centre=moved, fixups=list(fixups),
                model_bytes_d=model_d, model_bytes_l=model_d + 2 * W * H, blocks_us=blocks, median_us=med, spread_us=spread,
                l_over_d=med["l"] / med["d"], bytes_l_over_d=(model_d + 2 * W * H) / model_d, build_ms=build_ms,
                build_median_ms={n: statistics.median(v) for n, v in build_ms.items()},
                build_spread_ms={n: max(v) - min(v) for n, v in build_ms.items()})


def seam_table_host_ms(globe, repeats=3):
    """wall ms of making the seam table at 4K's platesize on the host (a device-less context), best of `repeats`"""
    import time
    best = None
    for _ in range(repeats):
        ctx = blinky_amd.Context(blinky_amd.ffi.DEVICE_NONE)
        ctx.load_globe(S.script("globes", globe), globe + ".lua")
        ctx.resize(W, H)
        t0 = time.perf_counter()
        ctx.read_seam_table()
        ms = (time.perf_counter() - t0) * 1e3
        ctx.close()
        best = ms if best is None else min(best, ms)
    return best


def measure_fb_seams(lens, repeats, reps, tint):
    """L (bk_apply_rgba_fb_bilinear_device) against S (bk_apply_rgba_fb_bilinear_seams_device, the cube's computed seam table), frame by
    frame, from the ring of measure_fb"""
    import seam_model as M
    SETS = SLOTS // 4
    ctx = blinky_amd.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(1)
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", lens, None, (W, H))
    display, _ = ctx.build()
    ps = min(W, H)
    shown = [p for p in range(6) if p < len(display) and display[p]]
    given = tuple(p in shown for p in range(6))
    lut = None
    if tint:
        pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
        lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [[torch.randint(0, 256, (ps, ps, 4), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)] for _ in range(SETS)]
    pitch = 4 * ps
    ptrs = [[src[s][p].data_ptr() if p in shown else None for p in range(6)] for s in range(SETS)]
    pitches = [pitch] * 6
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    plug = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def bilinear(s):
        ctx.apply_rgba_fb_bilinear_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut)

    def seams(s):
        ctx.apply_rgba_fb_bilinear_seams_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut)

    # before anything is timed: S's frame is the numpy model's, at full size, in the flavour that is timed
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    table = ctx.read_seam_table()
    plates = np.stack([src[0][p].cpu().numpy() for p in range(6)])
    seams(0)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(H, 4 * W)
    want = np.zeros((H, 4 * W), np.uint8)
    for r0 in range(0, H, 120):
        M.seam_frame(plates, off.reshape(-1), sub, tints.reshape(-1), W, H, ps, (r0, min(H, r0 + 120)), lut, want, 0, 0, table, given)
    if not np.array_equal(got, want):
        raise SystemExit(f"{lens}: the seam frame differs from the numpy model in {int((got != want).sum())} bytes - nothing timed")
    mapped = int((off != 0xFFFFFFFF).sum())
    rim = 0
    for r0 in range(0, H, 120):                            # (in bands, as the model above: positions keeps a dozen int64 arrays)
        band = slice(r0 * W, min(H, r0 + 120) * W)
        o_band = off.reshape(-1)[band]
        rim += int((M.positions(o_band, sub[band], ps, table, given)[3].any(0) & (o_band != 0xFFFFFFFF)).sum())
    del off, tints, sub, plates, got, want
    for k in range(2 * SETS):
        (seams if k % 2 else bilinear)(k % SETS)
    torch.cuda.synchronize()
    blocks = {"l": [], "s": []}
    k = 0
    for _ in range(repeats):
        ev = []
        for r in range(2 * reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            plug.fill_(r & 255)
            e[0].record(stream)
            (seams if r % 2 else bilinear)(k % SETS)
            e[1].record(stream)
            ev.append(e)
            k += 1
        torch.cuda.synchronize()
        blocks["l"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[0::2]))
        blocks["s"].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[1::2]))
    ctx.close()
    med = {n: statistics.median(v) for n, v in blocks.items()}
    spread = {n: max(v) - min(v) for n, v in blocks.items()}
    return dict(lens=lens, W=W, H=H, ps=ps, tint=bool(tint), seams=True, displayed_plates=shown, frames_per_block=reps, blocks=repeats,
                mapped_pixels=mapped, pixels_resolved_through_the_table=rim, blocks_us=blocks, median_us=med, spread_us=spread,
                s_over_l=med["s"] / med["l"], target_met=bool(med["s"] <= med["l"] + spread["l"] + spread["s"]))


def measure_fb_trilinear(lens, repeats, reps, tint):
    """L (bk_apply_rgba_fb_bilinear_device), T0 (bk_apply_rgba_fb_trilinear_device, mips = 0), T (mips = 1) and M (the pyramid by itself:
    bk_debug_mip_pyramid, the two launches that mips = 1 puts in front of the apply and nothing else), frame by frame, from the ring of
    measure_fb"""
    import trilinear_model as TM
    SETS = SLOTS // 4
    stream = torch.cuda.current_stream()

    ctx = blinky_amd.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_frames(1)
    ctx.set_subtexel(True)
    S.configure(ctx, "cube", lens, None, (W, H))
    display, _ = ctx.build()
    ps = min(W, H)
    shown = [p for p in range(6) if p < len(display) and display[p]]
    lut = None
    if tint:
        pal = blinky_amd.ffi.create_palmap(((np.arange(768) * 37) % 256).astype(np.uint8))
        lut = np.ascontiguousarray(np.broadcast_to(pal, (4, 6, 256)))
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [[torch.randint(0, 256, (ps, ps, 4), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)] for _ in range(SETS)]
    pitch = 4 * ps
    ptrs = [[src[s][p].data_ptr() if p in shown else None for p in range(6)] for s in range(SETS)]
    pitches = [pitch] * 6
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    plug = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    def bilinear(s):
        ctx.apply_rgba_fb_bilinear_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut)

    def tri0(s):
        ctx.apply_rgba_fb_trilinear_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut, mips=False)

    def tri(s):
        ctx.apply_rgba_fb_trilinear_device(ptrs[s], pitches, out.data_ptr(), 4 * W, lut=lut, mips=True)

    def pyramid(s):
        ctx.debug_mip_pyramid(ptrs[s], pitches)

    # before anything is timed: T's frame is the numpy model's, at full size, in the flavour that is timed, and the plane the derivation's
    off, tints = ctx.read_lensmap()
    sub = ctx.read_subtexel()
    lod = ctx.read_lod()
    if not np.array_equal(lod, TM.derive_lod(off.reshape(-1), sub, W, H, ps)):
        raise SystemExit(f"{lens}: the level-of-detail plane differs from the numpy derivation - nothing timed")
    plates = np.stack([src[0][p].cpu().numpy() for p in range(6)])
    pyr = TM.pyramid(plates)
    pyr = [pyr[0]] + [np.where(np.isin(np.arange(6), shown)[:, None, None, None], level, 0) for level in pyr[1:]]
    tri(0)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(H, 4 * W)
    want = np.zeros((H, 4 * W), np.uint8)
    for r0 in range(0, H, 120):                            # (in bands: the model keeps a dozen int64 arrays a level)
        r1 = min(H, r0 + 120)
        TM.trilinear_frame(pyr, off.reshape(-1), sub, lod[r0 * W:r1 * W], tints.reshape(-1), W, H, ps, (r0, r1), lut, want, 0, 0)
    if not np.array_equal(got, want):
        raise SystemExit(f"{lens}: the trilinear frame differs from the numpy model in {int((got != want).sum())} bytes - nothing timed")
    m = off.reshape(-1) != 0xFFFFFFFF
    census = [int(((lod[m] >> 8) == k).sum()) for k in range(len(pyr))]
    mapped, lod0 = int(m.sum()), int((lod[m] == 0).sum())
    del off, tints, sub, plates, pyr, got, want
    calls = [("l", bilinear), ("t0", tri0), ("t", tri), ("m", pyramid)]
    for k in range(2 * SETS):
        calls[k % 4][1](k % SETS)
    torch.cuda.synchronize()
    blocks = {n: [] for n, _ in calls}
    k = 0
    for _ in range(repeats):
        ev = []
        for r in range(4 * reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            plug.fill_(r & 255)
            e[0].record(stream)
            calls[r % 4][1](k % SETS)
            e[1].record(stream)
            ev.append(e)
            k += 1
        torch.cuda.synchronize()
        for i, (n, _) in enumerate(calls):
            blocks[n].append(statistics.median(e[0].elapsed_time(e[1]) * 1e3 for e in ev[i::4]))
    ctx.close()
    med = {n: statistics.median(v) for n, v in blocks.items()}
    spread = {n: max(v) - min(v) for n, v in blocks.items()}
    moved = len(shown) * 4 * ps * ps * 4 // 3               # the pyramid's bytes: every shown plate read once, a third of that written
    return dict(lens=lens, W=W, H=H, ps=ps, tint=bool(tint), trilinear=True, displayed_plates=shown, frames_per_block=reps, blocks=repeats,
                mapped_pixels=mapped, pixels_at_lod_0=lod0, pixels_by_lower_level=census, blocks_us=blocks, median_us=med, spread_us=spread,
                t0_over_l=med["t0"] / med["l"], t_minus_t0_us=med["t"] - med["t0"], pyramid_bytes=moved,
                pyramid_gb_s=moved / (med["m"] * 1e-6) / 1e9)


def main_fb_trilinear(args):
    rows = []
    what = "tinted" if args.tint else "plain"
    for lens in args.lenses.split(","):
        r = measure_fb_trilinear(lens, args.repeats, max(31, args.reps), args.tint)
        rows.append(r)
        m, s, b = r["median_us"], r["spread_us"], r["blocks_us"]
        print(f"4K cube/{lens}, one {what} truecolour frame per call from device plates (a ring of 16 sets), plates {r['displayed_plates']} displayed, "
              f"{r['mapped_pixels']} mapped pixels, {r['pixels_at_lod_0']} at lod 0, by lower level {r['pixels_by_lower_level']}, "
              f"{r['blocks']} blocks of {r['frames_per_block']} frames each, L / T0 / T / M alternated:\n"
              f"  L   bk_apply_rgba_fb_bilinear_device             {m['l']:8.1f} us (blocks {fmt(b['l'])}; spread {s['l']:.1f})\n"
              f"  T0  bk_apply_rgba_fb_trilinear_device, mips = 0  {m['t0']:8.1f} us (blocks {fmt(b['t0'])}; spread {s['t0']:.1f})\n"
              f"  T   bk_apply_rgba_fb_trilinear_device, mips = 1  {m['t']:8.1f} us (blocks {fmt(b['t'])}; spread {s['t']:.1f})\n"
              f"  M   the pyramid by itself (bk_debug_mip_pyramid)  {m['m']:8.1f} us (blocks {fmt(b['m'])}; spread {s['m']:.1f})\n"
              f"  T == the numpy model at full size; T0 / L = {r['t0_over_l']:.3f}; T - T0 = {r['t_minus_t0_us']:.1f} us; "
              f"M moves {r['pyramid_bytes'] / 1e6:.1f} MB: {r['pyramid_gb_s']:.0f} GB/s", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_fb_seams(args):
    rows = []
    what = "tinted" if args.tint else "plain"
    for lens in args.lenses.split(","):
        r = measure_fb_seams(lens, args.repeats, max(31, args.reps), args.tint)
        rows.append(r)
        m, s, b = r["median_us"], r["spread_us"], r["blocks_us"]
        print(f"4K cube/{lens}, one {what} truecolour frame per call from device plates (a ring of 16 sets), plates {r['displayed_plates']} displayed, "
              f"{r['mapped_pixels']} mapped pixels of which {r['pixels_resolved_through_the_table']} take a texel through the seam table, "
              f"{r['blocks']} blocks of {r['frames_per_block']} frames each way, L / S alternated:\n"
              f"  L  bk_apply_rgba_fb_bilinear_device        {m['l']:8.1f} us (blocks {fmt(b['l'])}; spread {s['l']:.1f})\n"
              f"  S  bk_apply_rgba_fb_bilinear_seams_device  {m['s']:8.1f} us (blocks {fmt(b['s'])}; spread {s['s']:.1f})\n"
              f"  S == the numpy model at full size; S / L = {r['s_over_l']:.3f}; S <= L + both spreads: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    host = {g: seam_table_host_ms(g) for g in ("cube", "fast")}
    print(f"the seam table on the host at platesize {min(W, H)}: cube (no callback) {host['cube']:.2f} ms, fast (globe_plate callback) {host['fast']:.2f} ms", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(dict(seam_table_host_ms=host)) + "\n")


def main_fb_bilinear(args):
    rows = []
    what = "tinted" if args.tint else "plain"
    for lens in args.lenses.split(","):
        r = measure_fb_bilinear(lens, args.repeats, max(31, args.reps), args.tint)
        rows.append(r)
        m, s, b = r["median_us"], r["spread_us"], r["blocks_us"]
        bm, bs = r["build_median_ms"], r["build_spread_ms"]
        print(f"4K cube/{lens}, one {what} truecolour frame per call from device plates (16-byte aligned, a ring of 16 sets), plates {r['displayed_plates']} "
              f"displayed, {r['mapped_pixels']} mapped pixels of which {r['pixels_off_centre']} off their texel's centre, {r['blocks']} blocks of "
              f"{r['frames_per_block']} frames each way, D / L alternated:\n"
              f"  D  bk_apply_rgba_fb_device           {m['d']:8.1f} us (blocks {fmt(b['d'])}; spread {s['d']:.1f})  estimate {r['model_bytes_d'] / 1e6:.1f} MB\n"
              f"  L  bk_apply_rgba_fb_bilinear_device  {m['l']:8.1f} us (blocks {fmt(b['l'])}; spread {s['l']:.1f})  estimate {r['model_bytes_l'] / 1e6:.1f} MB\n"
              f"  L == the numpy model at full size; L / D = {r['l_over_d']:.3f} (bytes alone: {r['bytes_l_over_d']:.3f})\n"
              f"  bk_build, switch off / on alternated: {bm['off']:.3f} / {bm['on']:.3f} ms (runs {fmt(r['build_ms']['off'])} / {fmt(r['build_ms']['on'])}; "
              f"spreads {bs['off']:.3f} / {bs['on']:.3f}); fix-ups (flagged, changed) {r['fixups']}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_fb(args):
    rows = []
    what = ("ss2 " if args.ss2 else "") + ("tinted" if args.tint else "plain")
    for lens in args.lenses.split(","):
        r = measure_fb(lens, args.repeats, max(31, args.reps), args.tint, args.ss2)
        rows.append(r)
        m, s, b = r["median_us"], r["spread_us"], r["blocks_us"]
        print(f"4K cube/{lens}, one {what} truecolour frame per call from device plates (16-byte aligned, a ring of 16 sets), plates {r['displayed_plates']} "
              f"displayed, footprint {r['footprint_tiles']} tiles, {r['blocks']} blocks of {r['frames_per_block']} frames each way, B + P / D alternated:\n"
              f"  B      footprint uploads        {m['b']:8.1f} us (blocks {fmt(b['b'])}; spread {s['b']:.1f})\n"
              f"  P      one-frame staged apply   {m['p']:8.1f} us (blocks {fmt(b['p'])}; spread {s['p']:.1f})\n"
              f"  B + P                           {m['bp']:8.1f} us (blocks {fmt(b['bp'])}; spread {s['bp']:.1f})\n"
              f"  D      bk_apply_rgba_fb_device  {m['d']:8.1f} us (blocks {fmt(b['d'])}; spread {s['d']:.1f})  estimate {r['model_bytes_d'] / 1e6:.1f} MB -> {r['d_model_gb_s']:.0f} GB/s\n"
              f"  D == B + P byte for byte; D / (B + P) = {r['d_over_bp']:.3f}, D / P = {r['d_over_p']:.3f}; "
              f"expectation D < B + P by more than both spreads: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_upload(args):
    rows = []
    for lens in args.lenses.split(","):
        r = measure_upload(lens, args.repeats, max(31, args.reps))
        rows.append(r)
        m, s, b = r["median_us"], r["spread_us"], r["blocks_us"]
        print(f"4K cube/{lens}, one truecolour globe per frame, device plates (16-byte aligned), plates {r['displayed_plates']} displayed; footprint "
              f"{r['footprint_tiles']} of {r['tiles_per_plate']} tiles per plate (ratio over the displayed plates {r['tile_ratio']:.3f}), "
              f"{r['blocks']} blocks of {r['frames_per_block']} frames each way, A/B alternated:\n"
              f"  A  full uploads          {m['a']:8.1f} us (blocks {fmt(b['a'])}; spread {s['a']:.1f})  model {r['model_bytes_a'] / 1e6:.1f} MB -> {r['a_gb_s']:.0f} GB/s\n"
              f"  B  footprint uploads     {m['b']:8.1f} us (blocks {fmt(b['b'])}; spread {s['b']:.1f})  model {r['model_bytes_b'] / 1e6:.1f} MB -> {r['b_gb_s']:.0f} GB/s\n"
              f"  P  one-frame apply       {m['pa']:8.1f} us after A, {m['pb']:.1f} us after B (spreads {s['pa']:.1f}, {s['pb']:.1f})\n"
              f"  A + P {m['ap']:.1f} us, B + P {m['bp']:.1f} us per frame (spreads {s['ap']:.1f}, {s['bp']:.1f}); (B + P) / (A + P) = {r['bp_over_ap']:.3f}\n"
              f"  frame after B == frame after A; B / A = {r['b_over_a']:.3f} next to the tile ratio {r['tile_ratio']:.3f}; "
              f"expectation B <= A + A's spread: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_ss2(args):
    rows = []
    what = "tinted" if args.tint else "plain"
    for lens in args.lenses.split(","):
        r = measure_ss2(lens, args.repeats, max(0.2, args.region), args.tint)
        rows.append(r)
        print(f"4K cube/{lens}, 2x2 supersampling, {what} [{r['block']} blocks, {r['lds_kib']} KiB staging; quads with 0..4 mapped samples: "
              f"{r['quads_by_mapped_samples']}], {r['launches_per_train']} launches per train, {args.repeats} x A/B alternated:\n"
              f"  A  16 full-size frames, {what:6s}   {r['a_us']:8.1f} us per launch (regions {fmt(r['a_regions_us'])}; spread {r['a_spread_us']:.1f})\n"
              f"  B  16 half-size frames, ss2      {r['b_us']:8.1f} us per launch (regions {fmt(r['b_regions_us'])}; spread {r['b_spread_us']:.1f})\n"
              f"  B == numpy average of A; B / A = {r['b_over_a']:.3f}; expectation B <= A + spread: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def fmt(ts):
    return ", ".join("%.1f" % x for x in ts)


def main_tint(args):
    rows = []
    for lens in args.lenses.split(","):
        r = measure_tint(lens, args.repeats, max(0.2, args.region))
        rows.append(r)
        print(f"4K cube/{lens}, f_rubix [tinted block map: {r['tinted_block']} blocks, {r['tinted_lds_kib']} KiB staging + 1.5 KiB LUT, "
              f"{r['tinted_slow_blocks']} blocks without staging], {r['launches_per_train']} launches per train, {args.repeats} x A'/B'/B alternated:\n"
              f"  A' 64 8-bit frames, rubix      {r['a_us']:8.1f} us per launch (regions {fmt(r['a_regions_us'])}; spread {r['a_spread_us']:.1f})\n"
              f"  B' 16 truecolour frames, tinted {r['t_us']:7.1f} us per launch (regions {fmt(r['t_regions_us'])})\n"
              f"  B  16 truecolour frames, plain  {r['b_us']:7.1f} us per launch (regions {fmt(r['b_regions_us'])})\n"
              f"  B' == A' plane by plane ({r['bytes_changed_by_the_tint']} bytes differ from the plain frames); B' / A' = {r['t_over_a']:.3f}; "
              f"B' / B = {r['t_over_b']:.3f}; target B' <= A' + spread: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lenses", default="panini,hammer")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.25, help="seconds per timed region (at least 0.2)")
    ap.add_argument("--out", default=None, help="also write the results as JSON lines to this file")
    ap.add_argument("--tint", action="store_true", help="f_rubix: 8-bit rubix launch A' / tinted truecolour B' / plain truecolour B")
    ap.add_argument("--ss2", action="store_true", help="2x2 supersampling: full-size truecolour launch A (with --tint: the tinted one) / fused ss2 launch B")
    ap.add_argument("--upload", action="store_true", help="the per-frame loop: full plate uploads A / footprint uploads B / the one-frame apply P behind them")
    ap.add_argument("--fb", action="store_true", help="one frame per call: footprint uploads + the staged one-frame apply B + P / bk_apply_rgba_fb_device D (with --tint / --ss2: the matching pairs)")
    ap.add_argument("--seams", action="store_true", help="with --fb --bilinear: bk_apply_rgba_fb_bilinear_device L / bk_apply_rgba_fb_bilinear_seams_device S, and the host cost of the seam table")
    ap.add_argument("--bilinear", action="store_true", help="with --fb: bk_apply_rgba_fb_device D / bk_apply_rgba_fb_bilinear_device L (with --tint: both through the tables), and bk_build with the sub-texel plane off / on")
    ap.add_argument("--trilinear", action="store_true", help="with --fb: bk_apply_rgba_fb_bilinear_device L / bk_apply_rgba_fb_trilinear_device without (T0) and with (T) the pyramid / the pyramid alone M")
    ap.add_argument("--reps", type=int, default=31, help="--upload / --fb: frames each way per block (at least 31)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rgba.py measures on the GPU; there is none here")
    if args.seams:
        if not (args.fb and args.bilinear) or args.ss2:
            raise SystemExit("--seams goes with --fb --bilinear (and not with --ss2)")
        return main_fb_seams(args)
    if args.trilinear:
        if not args.fb or args.ss2 or args.bilinear or args.seams:
            raise SystemExit("--trilinear goes with --fb (and not with --ss2, --bilinear or --seams)")
        return main_fb_trilinear(args)
    if args.bilinear:
        if not args.fb or args.ss2:
            raise SystemExit("--bilinear goes with --fb (and not with --ss2)")
        return main_fb_bilinear(args)
    if args.fb:
        return main_fb(args)
    if args.upload:
        return main_upload(args)
    if args.ss2:
        return main_ss2(args)
    if args.tint:
        return main_tint(args)
    rows = []
    for lens in args.lenses.split(","):
        r = measure(lens, args.repeats, max(0.2, args.region))
        rows.append(r)
        print(f"4K cube/{lens} [{r['block']} blocks, {r['lds_kib']} KiB staging], regions of {r['region_s']:.2f} s, {args.repeats} x A/B alternated:\n"
              f"  A  64 8-bit frames      {r['a_us']:8.1f} us per launch (regions {', '.join('%.1f' % t for t in r['a_regions_us'])}; spread {r['a_spread_us']:.1f})\n"
              f"  B  16 truecolour frames {r['b_us']:8.1f} us per launch (regions {', '.join('%.1f' % t for t in r['b_regions_us'])})\n"
              f"  B / A = {r['b_over_a']:.3f}; {r['us_per_truecolour_frame']:.2f} us per truecolour frame; model {r['model_bytes_per_truecolour_frame'] / 1e6:.1f} MB per frame"
              f" staged -> {r['implied_tb_s']:.2f} TB/s, {r['compulsory_bytes_per_truecolour_frame'] / 1e6:.1f} MB compulsory -> {r['compulsory_tb_s']:.2f} TB/s; "
              f"target B <= A + spread: {'met' if r['target_met'] else 'MISSED'}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
