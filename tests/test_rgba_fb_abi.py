"""bk_apply_rgba_fb_device at the C-ABI boundary (no GPU), as test_footprint_abi.py checks its entry points: declared in
include/blinky_hip.h with its contract, exported by libblinkyhip.so, bound by blinky_amd/ffi.py with a Context method; a host-only
(BK_DEVICE_NONE) context refuses it with BK_E_STATE instead of touching a device, NULL arguments are BK_E_INVALID.  Also without a GPU:
the kernel's way from a lensmap entry back to (plate, px, py) is exact for every globe layout bk_resize accepts, and the
expectation function of tests/test_apply_rgba_fb_gpu.py (tests/rgba_fb_model.py) agrees with the campaign's oracle expectation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rgba_fb_model as M
import rgbagen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, METHOD, NARGS = "bk_apply_rgba_fb_device", "apply_rgba_fb_device", 9
BK_E_INVALID, BK_E_STATE = -1, -6


def test_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "blinky_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bk_[a-z_0-9]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "blinky_amd", "libblinkyhip.so")], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    import blinky_amd.ffi as ffi
    assert NAME in declared, f"{NAME} is not declared in blinky_hip.h"
    assert NAME in exported, f"{NAME} is not exported by libblinkyhip.so"
    assert NAME in ffi.EXPORTS and getattr(ffi.lib, NAME).argtypes is not None, f"{NAME} is not bound by blinky_amd/ffi.py"
    assert len(getattr(ffi.lib, NAME).argtypes) == NARGS
    assert callable(getattr(ffi.Context, METHOD))


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "blinky_hip.h")).read()
    conventions = text[:text.index("#ifndef BLINKY_HIP_H")]
    assert NAME in conventions, f"{NAME} is missing from the TRUECOLOUR sentence of the conventions block"
    start = text.index("/* " + NAME)
    comment = " ".join(text[start:text.index("*/", start)].split()).lower().replace("* ", "")
    assert "source texels outside rect are never read" in comment
    for phrase in ("multiples of 16", "may be null", "one host synchronisation", "out of scope"):
        assert phrase in comment, phrase


def test_host_only_context_refuses_it_and_null_arguments_are_invalid():
    import blinky_amd as bk
    ffi = bk.ffi
    ctx = bk.Context(ffi.DEVICE_NONE)
    ctx.resize(64, 48)
    fake = 4096                                                # never dereferenced: the call is refused before any device work
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*BK_DEVICE_NONE"):
        ctx.apply_rgba_fb_device([fake] * 6, [4 * 48] * 6, C.c_void_p(fake), 4 * 64)
    plates = (C.c_void_p * 6)(*[fake] * 6)
    pitches = (C.c_int * 6)(*[4 * 48] * 6)
    fn = ffi.lib.bk_apply_rgba_fb_device
    assert fn(ctx._h, plates, pitches, C.c_void_p(fake), 4 * 64, 0, 0, None, 0) == BK_E_STATE
    assert fn(None, plates, pitches, C.c_void_p(fake), 4 * 64, 0, 0, None, 0) == BK_E_INVALID
    assert fn(ctx._h, None, pitches, C.c_void_p(fake), 4 * 64, 0, 0, None, 0) == BK_E_INVALID
    assert fn(ctx._h, plates, None, C.c_void_p(fake), 4 * 64, 0, 0, None, 0) == BK_E_INVALID
    assert fn(ctx._h, plates, pitches, None, 4 * 64, 0, 0, None, 0) == BK_E_INVALID
    ctx.close()


def accepted_layouts():
    """every padded plate width bk_resize accepts (6 * gp * ph < 2^32 - 1 with gp = round_up(ps, 64), ph = round_up(ps, 8)), each with the
    LARGEST height it accepts with it: every tile index a lower plate of that width has occurs there too"""
    out = []
    for gp in range(64, 1 << 16, 64):
        ph = [h for h in range(gp - 56, gp + 1, 8) if 6 * gp * h < 0xFFFFFFFF]
        if not ph:
            break
        out.append((gp, ph[-1]))
    return out


def test_the_kernels_decode_is_exact_for_every_layout():
    """plate by comparisons, tile row by a host-made reciprocal and one correction step (bk_apply_rgba_fb.inc): against bk_texel_coords'
    divisions over every tile of a plate and every plate's boundaries, for EVERY padded plate width bk_resize accepts - the largest is
    26752, far past where an uncorrected reciprocal goes wrong (21184) - and at a few lower heights, which move the plate boundaries"""
    import blinky_amd.ffi as ffi
    check = ffi.lib.bk_debug_fb_decode_check
    layouts = accepted_layouts()
    assert layouts[0] == (64, 64) and layouts[-1][0] == 26752 and [g for g, _ in layouts] == list(range(64, 26752 + 1, 64))
    assert 6 * 26752 * layouts[-1][1] < 0xFFFFFFFF <= 6 * 26816 * (26816 - 56)     # (the next width is refused at every height)
    for gp, ph in layouts:
        assert check(gp, ph) == 0, (gp, ph)
    for gp, ph in ((64, 8), (64, 16), (256, 208), (320, 304), (2176, 2160), (4096, 4040), (8192, 8136), (21184, 21128), (26752, 26696)):
        assert check(gp, ph) == 0, (gp, ph)
    assert check(100, 96) == -1 and check(64, 60) == -1 and check(32768, 32768) == -1 and check(26816, 26760) == -1


def test_a_bare_reciprocal_fails_from_gp_21184_on():
    """why the correction step is there: floor(2^32 / tpr) + 1 and no step puts tile 3254391 of a gp 21184 plate one row too low"""
    tpr, tile = 21184 // 16, 3254391
    assert (tile * ((1 << 32) // tpr + 1)) >> 32 == tile // tpr + 1
    q = (tile * ((1 << 32) // tpr)) >> 32
    assert q + (tile - q * tpr >= tpr) == tile // tpr


# ---- the expectation function of the GPU file, held to the campaign's (oracle_frame: the CPU oracle's 8-bit apply plane by plane,
# quad_means for ss2) on the tables of committed rgbagen seeds: two of the full-size family, two of the ss2 family
# (full 0: 127 x 17, rows [13, 15); full 3: 3 x 9; ss2 0: 209 x 17, odd both ways, all four kinds; ss2 5: 128 x 240, rows [122, 156))
MODEL_SEEDS = [("full", 0), ("full", 3), ("ss2", 0), ("ss2", 5)]


@pytest.mark.parametrize("family,seed", MODEL_SEEDS)
def test_expectation_function_equals_the_campaigns_oracle_frames(family, seed):
    seq = G.sequence(seed) if family == "full" else G.sequence_ss2(seed)
    globes = {}

    def slots(s):
        if s not in globes:
            globes[s] = G.slot_globe(seq, s)
        return globes[s]

    checked = set()
    for i, L, off, tints, lut, ev in G.walk(seq):
        if L["kind"] == "apply8":
            continue
        g = G.ring_slot(seq, L, 0)
        want = np.full((L["frame_h"], L["pitch"]), G.FILL, np.uint8)
        G.oracle_frame(seq, L, off, tints, lut, None, slots, g, want)
        plates = M.plates_of_planes([slots(4 * g + c) for c in range(4)])
        got = np.full((L["frame_h"], L["pitch"]), G.FILL, np.uint8)
        M.fb_frame(plates, off, tints, seq["W"], seq["H"], seq["ps"], (seq["r0"], seq["r1"]), lut, L["kind"] in G.SS2_KINDS, got, L["x0"], L["y0"])
        np.testing.assert_array_equal(got, want, err_msg=G.describe(seq, i))
        checked.add(L["kind"])
    assert checked & (set(G.SS2_KINDS) if family == "ss2" else {"rgba", "rgba_tinted"}), (checked, G.describe(seq))


def test_model_seeds_hold_every_flavour():
    kinds = set()
    for family, seed in MODEL_SEEDS:
        seq = G.sequence(seed) if family == "full" else G.sequence_ss2(seed)
        kinds |= {L["kind"] for L in seq["launches"]}
    assert {"rgba", "rgba_tinted", "ss2", "ss2_tinted"} <= kinds, kinds
