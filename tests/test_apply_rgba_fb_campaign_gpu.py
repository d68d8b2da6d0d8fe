"""Randomised EVENT AND LAUNCH sequences on the five frame-buffer applies (bk_apply_rgba_fb_device plain and ss2, _bilinear_, _bilinear_seams_,
_trilinear_ with mips 0 / 1) against the shadow state of tests/fbgen.py.  One context per seed - frames from 1x1 to 260x131, stripes down
to one row, the sub-texel switch on or off - and 10-16 steps on it: bk_set_lensmap, bk_set_lensmap_subtexel, bk_set_lensmap_lod,
bk_set_lod_bias, bk_set_subtexel, bk_set_seam_table, bk_set_rows, bk_resize, bk_truncate_build, a LUT changed in place; launches of every
kind, plain and tinted, from every source layout, with plates passed as NULL, at every destination alignment class; reads of every piece
of state.  After EVERY step: a launch the shadow calls "ok" left the whole destination allocation - fill 77 included - byte for byte as
the numpy models of the five applies say; a read gave the shadow's array; a call the shadow calls "refused" raised BlinkyError with that
code and message, and a destination filled with 77 beforehand is still all 77 after torch.cuda.synchronize().  Every refusal is a
host-side argument or state check that returns before any launch: no step asks the device for anything invalid.
tests/test_fb_campaign_cpu.py holds the shadow to a second statement and to the loop twins of the models, and counts what the committed
seeds reach.  The committed range runs in the suite; BLINKY_FB_CAMPAIGN=lo:hi runs a developer range.  Byte-exact, nothing filtered.

Measured on an MI355X: the file alone 3.0 s for its 48 seeds (1.9 s of it the first seed, which starts the runtime); inside the whole suite
0.4 s, its slowest seed (45: 260 x 129) 0.10 s.  The whole suite with it 659 s, of which this file and tests/test_fb_campaign_cpu.py are
6.2 s: 653 s without them, the parent commit's suite (the same run, their durations taken off; not a run of its own).

Native mutants, each one state rule taken out of a scratch copy of the library (value-only: no address, size or NULL check depends on the
flag) - the seed and step of this file that caught it, and the older directed files that do:
  1 lod_invalidate out of lensmap_edited (kept in lensmap_dropped: a plane that outlives a size change could name a level the new platesize
    has not)                                       seed 0 step 8 (trilinear frame), 8 seeds;  also tests/test_lod_gpu.py::test_life_cycle
  2 lod_invalidate out of bk_set_lensmap_subtexel  seed 4 step 9 (read_lod), 8 seeds;         also test_lod_gpu.py::test_life_cycle
  3 lod_invalidate out of bk_set_lod_bias          seed 3 step 10 (trilinear frame), 2 seeds; also test_lod_gpu.py (life_cycle, device_builds, drawn_tables)
  4 d_seam_current = false out of bk_set_seam_table  seed 9 step 8 (seams frame), 2 seeds;    also test_apply_rgba_fb_seams_gpu.py (interleaved, real
    build) and test_lensmap_state_gpu.py::test_set_rows_that_moves_a_stripe_of_the_same_height
  5 lensmap_dropped out of bk_set_rows' same-height path  seed 7 step 5 (a launch not refused), 9 seeds;  also test_lensmap_state_gpu.py (same test)
  6 the memset to 0x80 out of bk_set_lensmap       seed 0 step 4 (bilinear frame), 28 seeds;   also the plane-of-centres identities of the bilinear,
    seams and trilinear files and test_subtexel_gpu.py::test_the_plane_follows_the_lensmap
  7 upload_lut's compare always equal after the first upload  seed 3 step 10 (tinted trilinear frame), 17 seeds;  also the four
    test_interleaved_with_the_other_launches_on_one_context and two tests of test_lensmap_state_gpu.py
The unmutated scratch build passes all of them.  No mutant is seen by the campaign alone: each of the seven rules has a directed test already.
Mutant 4 shows only where a second seam table is set over one the device already holds: the steps of rule 11 (tests/fbgen.py) begin
with two tables and two seams launches for that."""
import os
import re

import numpy as np
import pytest

import fbgen as G

pytestmark = pytest.mark.gpu
FB = G.FB


def _seeds():
    v = os.environ.get("BLINKY_FB_CAMPAIGN")
    if not v:
        return G.COMMITTED
    lo, hi = [int(x) for x in v.split(":")]
    return range(lo, hi)


def _differs(seq, i, got, want, what, d=None, ptr_off=0):
    """the failure message: the sequence up to this step and the first differing element (of a frame: as a pixel, as trilinear_gpu.same does)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{G.describe(seq, i)}\n{what}: shape {got.shape}, expected {want.shape}"
    at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    where = f"element {at}"
    if d is not None and at >= ptr_off:
        y, xb = divmod(at - ptr_off, d["pitch"])
        where = f"byte {at} of the allocation = pixel (x {xb // 4 - d['x0']}, y {y - d['y0']}) byte {xb % 4}"
    return (f"{G.describe(seq, i)}\n{what}: {int((got != want).sum())} of {want.size} differ, the first at {where}: "
            f"{int(got.reshape(-1)[at])}, expected {int(want.reshape(-1)[at])}")


@pytest.mark.parametrize("seed", _seeds())
def test_random_event_and_launch_sequence(seed):
    import blinky_amd as bk
    import torch
    seq = G.sequence(seed)
    sh = G.shadow_of(seq)
    ctx = bk.Context()
    ctx.set_frames(seq["slots"])
    ctx.resize(seq["W"], seq["H"])
    ctx.set_rows(seq["r0"], seq["r1"])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_subtexel(seq["sub_on"])
    luts = {k: G.luts_of(k).copy() for k in (0, 1)}                    # the caller's two arrays: the SAME objects through every tinted launch
    sources = {}

    def source(ps, st):
        key = (ps, st["plates"], st["layout"], st["nulls"])
        if key not in sources:
            sources[key] = FB.source(G.plates_of(ps, st["plates"]), st["layout"], skip=st["nulls"])
        return sources[key]

    for i, st in enumerate(seq["steps"]):
        op = st["op"]
        W, H, ps, r0, r1 = sh.W, sh.H, sh.ps, sh.r0, sh.r1                # (what the call meets: no step changes the size its own arguments have)
        rows = lambda a: G.rows_of(a, W, r0, r1)
        dst = d = None
        if op == "launch":
            d = G.dest_of(W, H, st)
            dst = torch.full((st["ptr_off"] + d["rows"] * d["pitch"],), G.FILL, dtype=torch.uint8, device="cuda")
            assert dst.data_ptr() % 16 == 0
            _, ptrs, pitches = source(ps, st)
            args = (ptrs, pitches, dst.data_ptr() + st["ptr_off"], d["pitch"])
            kw = dict(x0=d["x0"], y0=d["y0"], lut=None if st["lut"] is None else luts[st["lut"]])
            call = {"nearest": lambda: ctx.apply_rgba_fb_device(*args, ss2=False, **kw), "ss2": lambda: ctx.apply_rgba_fb_device(*args, ss2=True, **kw),
                    "bilinear": lambda: ctx.apply_rgba_fb_bilinear_device(*args, **kw), "seams": lambda: ctx.apply_rgba_fb_bilinear_seams_device(*args, **kw),
                    "trilinear": lambda: ctx.apply_rgba_fb_trilinear_device(*args, mips=st["mips"], **kw)}[st["kind"]]
        elif op == "set_lensmap":
            off, tints = G.table_of(W, H, st["table"], st["drop"])
            call = lambda: ctx.set_lensmap(rows(off), rows(tints))
        elif op == "set_lensmap_subtexel":
            call = lambda: ctx.set_lensmap_subtexel(rows(G.subs_of(W, H, st["sub"])))
        elif op == "set_lensmap_lod":
            plane = sh.lod_argument(st)
            call = lambda: ctx.set_lensmap_lod(plane)
        elif op == "set_lod_bias":
            call = lambda: ctx.set_lod_bias(st["bias"])
        elif op == "set_subtexel":
            call = lambda: ctx.set_subtexel(st["on"])
        elif op == "set_seam_table":
            call = lambda: ctx.set_seam_table(G.seams_of(ps, st["seams"]))
        elif op == "set_rows":
            call = lambda: ctx.set_rows(*st["rows"])
        elif op == "resize":
            call = lambda: ctx.resize(*st["size"])
        elif op == "truncate_build":
            call = lambda: ctx.truncate_build(st["key"])
        elif op == "lut_in_place":
            def call():
                luts[st["lut"]][...] = G.luts_of(st["bytes"])          # new bytes in the array object the next tinted call passes
        elif op == "read_mip_level":
            call = lambda: ctx.read_mip_level(st["plate"], st["level"])
        else:
            call = getattr(ctx, op)                                    # read_lod, read_subtexel, read_seam_table, read_lensmap
        outcome = sh.apply(st)
        if outcome[0] == "refused":
            try:
                call()
            except bk.BlinkyError as e:
                assert re.search(rf"\[{outcome[1]}\].*{re.escape(outcome[2])}", str(e)), \
                    f"{G.describe(seq, i)}\nrefused with {e}: the shadow expects [{outcome[1]}] ... {outcome[2]}"
            else:
                raise AssertionError(f"{G.describe(seq, i)}\nnot refused: the shadow expects [{outcome[1]}] {outcome[2]}")
            if dst is not None:
                torch.cuda.synchronize()
                assert bool((dst == G.FILL).all()), f"{G.describe(seq, i)}\na refused launch wrote to its destination"
            continue
        try:
            got = call()
        except bk.BlinkyError as e:
            raise AssertionError(f"{G.describe(seq, i)}\nrefused with {e}: the shadow expects it to run") from None
        want = outcome[1]
        if op == "launch":
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert np.array_equal(got, want), _differs(seq, i, got, want, "the destination allocation", d, st["ptr_off"])
        elif op == "read_lensmap":
            for g, w, name in zip(got, want, ("offsets", "tints")):
                assert np.array_equal(g, w), _differs(seq, i, g, w, name)
        elif op in G.READS:
            assert np.array_equal(np.asarray(got).reshape(want.shape), want), _differs(seq, i, np.asarray(got).reshape(want.shape), want, op)
    ctx.close()
