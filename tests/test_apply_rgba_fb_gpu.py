"""bk_apply_rgba_fb_device on the GPU: one truecolour frame straight out of six row-major plates in device memory.  Every case has two
expectations over the WHOLE destination allocation (fill 77, a pitch wider than the frame, an origin, rows below): (a) the numpy model of
tests/rgba_fb_model.py (held to the campaign's oracle frames by tests/test_rgba_fb_abi.py), and (b) the existing path - the same plates
through bk_upload_plate_rgba_device into a globe and the matching existing apply - byte for byte.  Lensmaps come from the CPU oracle or
from the campaign's table generator through bk_set_lensmap unless a test says otherwise.  Every comparison is exact equality."""
import numpy as np
import pytest

import footprint_model as FM
import oracle_ffi as O
import rgba_fb_model as M
import rgbagen as G

pytestmark = pytest.mark.gpu

FILL, ROWS_BELOW = 77, 3
MODES = [("plain", False, False), ("tinted", True, False), ("ss2", False, True), ("ss2 tinted", True, True)]
PANINI = ("cube", "panini", "f_fov 120", 322, 203)                      # ps 203: gp 256 != ps; plates 3-5 unread; H odd
STEREO = ("cube", "stereographic", "f_vfov 90", 300, 500)               # portrait, ps 300
ORACLE_TABLES = [PANINI, STEREO, FM.FULL]
DRAWN_SIZES = [(1, 1), (3, 9), (4, 2), (130, 17), (131, 9), (256, 64)]   # ps 1, 3, 2, 17, 9, 64
_CACHE = {}


@pytest.fixture(scope="module")
def bk():
    import blinky_amd
    return blinky_amd


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def oracle_table(cfg):
    """(off, tints, W, H, ps) of an oracle lensmap, computed once for the module and never changed"""
    if cfg not in _CACHE:
        lm = O.lensmap(*cfg)
        lm.offsets.flags.writeable = False
        lm.tints.flags.writeable = False
        _CACHE[cfg] = (lm.offsets, lm.tints, lm.W, lm.H, lm.ps)
    return _CACHE[cfg]


def drawn_table(W, H, seed=0):
    """a table of the campaign's generator, tints from its values plus 6 and 200 (both leave the texel as it is)"""
    key = ("drawn", W, H, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(5000 + 1000 * seed + 7 * W + H)
        ps = min(W, H)
        off, tints, _ = G._draw_table(rng, W, H, ps)
        tints = tints.copy()
        pick = rng.random(W * H)
        tints[pick < 0.1] = 6
        tints[pick > 0.9] = 200
        off.flags.writeable = False
        tints.flags.writeable = False
        _CACHE[key] = (off, tints, W, H, ps)
    return _CACHE[key]


def luts(seed):
    lut = np.random.default_rng(seed).integers(0, 256, (4, 6, 256)).astype(np.uint8)
    assert len({r.tobytes() for r in lut.reshape(24, 256)}) == 24        # the 24 rows pairwise distinct
    return lut


def texels(ps, seed):
    """uint8 [6][ps][ps][4]: the four bytes of every texel pairwise different, so a byte-plane mix-up shows"""
    base = np.random.default_rng(900 + seed).integers(0, 256, (6, ps, ps, 1))
    t = ((base + np.array([0, 61, 127, 190])) % 256).astype(np.uint8)
    assert all((t[..., a] != t[..., b]).all() for a in range(4) for b in range(a))
    return t


# ---- the source: six plates somewhere in ONE device allocation ---------------------------------------------------------------------
LAYOUTS = ("tight", "pitch16", "pitch+20", "ptr4", "atlas", "six-pitches")
SRC_GUARD = 0xA5


def place(ps, layout):
    """-> ([(byte offset, pitch)] * 6, total bytes): where the plates lie in the allocation (itself 16-byte aligned)"""
    row = 4 * ps
    r16 = (row + 15) // 16 * 16
    if layout == "atlas":                                              # 3 x 2 plates side by side in one image
        pitch = 3 * row
        return [((p // 3) * ps * pitch + (p % 3) * row, pitch) for p in range(6)], 2 * ps * pitch
    pitches = {"tight": [row] * 6, "pitch16": [r16 + 16] * 6, "pitch+20": [r16 + 20] * 6, "ptr4": [r16 + 16] * 6,
               "six-pitches": [row, r16 + 16, r16 + 20, row + 4, r16 + 32, r16 + 36]}[layout]
    out, at = [], 0
    for p in range(6):
        at = (at + 15) // 16 * 16 + (4 if layout == "ptr4" else 0)
        out.append((at, pitches[p]))
        at += ps * pitches[p]
    return out, at


def source(plates, layout="tight", skip=()):
    """-> (the device tensor that must stay alive, six addresses - None for the plates in `skip` -, six pitches)"""
    import torch
    ps = plates.shape[1]
    where, total = place(ps, layout)
    buf = np.full(total, SRC_GUARD, np.uint8)
    for p, (at, pitch) in enumerate(where):
        rows = np.lib.stride_tricks.as_strided(buf[at:], shape=(ps, 4 * ps), strides=(pitch, 1))
        rows[...] = plates[p].reshape(ps, 4 * ps)
    dev = torch.from_numpy(buf).cuda()
    return dev, [None if p in skip else dev.data_ptr() + where[p][0] for p in range(6)], [w[1] for w in where]


# ---- the destination ----------------------------------------------------------------------------------------------------------------
def dest(W, H, ss2, x0=4, y0=2, extra_px=8):
    Wd, Hd = ((W + 1) // 2, (H + 1) // 2) if ss2 else (W, H)
    pitch = 4 * (Wd + extra_px)
    return dict(pitch=pitch, x0=x0, y0=y0, rows=y0 + Hd + ROWS_BELOW)


def run_fb(ctx, ptrs, pitches, d, lut, ss2, ptr_off=0):
    import torch
    dst = torch.full((ptr_off + d["rows"] * d["pitch"],), FILL, dtype=torch.uint8, device="cuda")
    ctx.apply_rgba_fb_device(ptrs, pitches, dst.data_ptr() + ptr_off, d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut, ss2=ss2)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def run_existing(ctx, d, lut, ss2, ptr_off=0):
    """the matching existing apply of truecolour globe 0, one frame, into the same allocation"""
    import torch
    dst = torch.full((ptr_off + d["rows"] * d["pitch"],), FILL, dtype=torch.uint8, device="cuda")
    stride = d["rows"] * d["pitch"]
    if ss2:
        ctx.apply_rgba_ss2_device(dst.data_ptr() + ptr_off, d["pitch"], stride, x0=d["x0"], y0=d["y0"], lut=lut)
    elif lut is not None:
        ctx.apply_rgba_tinted_device(dst.data_ptr() + ptr_off, d["pitch"], stride, lut, x0=d["x0"], y0=d["y0"])
    else:
        ctx.apply_rgba_device(dst.data_ptr() + ptr_off, d["pitch"], stride, x0=d["x0"], y0=d["y0"])
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def model(plates, table, d, lut, ss2, rows=None, ptr_off=0):
    off, tints, W, H, ps = table
    want = np.full(ptr_off + d["rows"] * d["pitch"], FILL, np.uint8)
    frame = want[ptr_off:].reshape(d["rows"], d["pitch"])
    M.fb_frame(plates, off, tints, W, H, ps, rows or (0, H), lut, ss2, frame, d["x0"], d["y0"])
    return want


def make_ctx(bk, table, slots=4, rows=None):
    off, tints, W, H, ps = table
    ctx = bk.Context()
    ctx.set_frames(slots)
    ctx.resize(W, H)
    ctx.set_stream(_stream())
    set_table(ctx, table, rows)
    return ctx


def set_table(ctx, table, rows=None):
    off, tints, W, H, ps = table
    if rows:
        ctx.set_rows(*rows)
    r0, r1 = rows or (0, H)
    ctx.set_lensmap(np.asarray(off).reshape(H, W)[r0:r1], np.asarray(tints).reshape(H, W)[r0:r1])
    assert ctx.size()[2] == ps


def upload_globe(ctx, plates):
    """the same plates into truecolour globe 0 through bk_upload_plate_rgba_device"""
    import torch
    ps = plates.shape[1]
    for p in range(6):
        dev = torch.from_numpy(plates[p]).cuda()
        ctx.upload_plate_rgba_device(0, p, dev.data_ptr(), 4 * ps)
        ctx.synchronize()


def check_modes(ctx, table, plates, lut, src, what, rows=None, existing=True, modes=MODES, dest_kw=None):
    off, tints, W, H, ps = table
    _, ptrs, pitches = src
    for name, tinted, ss2 in modes:
        d = dest(W, H, ss2, **(dest_kw or {}))
        got = run_fb(ctx, ptrs, pitches, d, lut if tinted else None, ss2)
        np.testing.assert_array_equal(got, model(plates, table, d, lut if tinted else None, ss2, rows), err_msg=f"{what} {name}: the model")
        if existing:
            np.testing.assert_array_equal(got, run_existing(ctx, d, lut if tinted else None, ss2), err_msg=f"{what} {name}: the existing path")


# ---- 1. tables: plain, tinted, ss2, ss2 tinted ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ORACLE_TABLES, ids=lambda c: f"{c[0]}-{c[1]}-{c[3]}x{c[4]}")
def test_oracle_lensmaps(bk, cfg):
    table = oracle_table(cfg)
    ps = table[4]
    plates, lut = texels(ps, 1), luts(11)
    ctx = make_ctx(bk, table)
    upload_globe(ctx, plates)
    check_modes(ctx, table, plates, lut, source(plates), str(cfg))
    ctx.close()


def test_drawn_sizes_cover_the_platesize_classes():
    ps = [min(w, h) for w, h in DRAWN_SIZES]
    assert any(p < 16 for p in ps) and any(p % 8 for p in ps) and any(p % 64 == 0 for p in ps)


@pytest.mark.parametrize("W,H", DRAWN_SIZES)
def test_drawn_tables(bk, W, H):
    for seed in (0, 1):
        table = drawn_table(W, H, seed)
        ps = table[4]
        plates, lut = texels(ps, 2 + seed), luts(12 + seed)
        ctx = make_ctx(bk, table)
        upload_globe(ctx, plates)
        check_modes(ctx, table, plates, lut, source(plates, LAYOUTS[(W + seed) % len(LAYOUTS)]), f"drawn {W}x{H} seed {seed}")
        ctx.close()


# ---- 2. source and destination classes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_source_classes(bk, layout):
    table = oracle_table(PANINI)
    ps = table[4]
    where, _ = place(ps, layout)
    r16 = (4 * ps + 15) // 16 * 16
    if layout == "tight":
        assert all(w[1] == 4 * ps for w in where) and all(w[0] % 16 == 0 for w in where)
    elif layout == "pitch16":
        assert all(w[1] % 16 == 0 and w[1] > 4 * ps and w[0] % 16 == 0 for w in where)
    elif layout == "pitch+20":
        assert all(w[1] == r16 + 20 and w[1] % 16 == 4 for w in where)
    elif layout == "ptr4":
        assert all(w[0] % 16 == 4 for w in where)
    elif layout == "six-pitches":
        assert len({w[1] for w in where}) == 6
    plates, lut = texels(ps, 3), luts(13)
    ctx = make_ctx(bk, table)
    upload_globe(ctx, plates)
    check_modes(ctx, table, plates, lut, source(plates, layout), layout)
    ctx.close()


@pytest.mark.parametrize("cls", G.ALIGN_CLASSES)
@pytest.mark.parametrize("which", ["panini", "drawn 256x64"])
def test_destination_classes(bk, which, cls):
    table = oracle_table(PANINI) if which == "panini" else drawn_table(256, 64)
    off, tints, W, H, ps = table
    plates, lut = texels(ps, 4), luts(14)
    ctx = make_ctx(bk, table)
    upload_globe(ctx, plates)
    src = source(plates, "pitch16")
    for name, tinted, ss2 in MODES:
        Wd = (W + 1) // 2 if ss2 else W
        x0 = {"16": 4, "8-only": 2, "4-only": 1}[cls]
        px_pitch = (Wd + x0 + 3) // 4 * 4 + {"16": 4, "8-only": 2, "4-only": 1}[cls]
        d = dest(W, H, ss2, x0=x0, y0=2, extra_px=px_pitch - Wd)
        assert G.align_class(d["y0"] * d["pitch"] + 4 * x0, d["pitch"], 0) == cls
        got = run_fb(ctx, src[1], src[2], d, lut if tinted else None, ss2)
        np.testing.assert_array_equal(got, model(plates, table, d, lut if tinted else None, ss2), err_msg=f"{which} {cls} {name}: the model")
        np.testing.assert_array_equal(got, run_existing(ctx, d, lut if tinted else None, ss2), err_msg=f"{which} {cls} {name}: the existing path")
    ctx.close()


# ---- 3. nothing outside what the lensmap names is read ----------------------------------------------------------------------------------
def test_values_outside_the_footprint_do_not_matter_and_unread_plates_may_be_null(bk):
    table = oracle_table(PANINI)
    off, tints, W, H, ps = table
    masks, counts, _ = FM.footprint(off, W, H, ps)
    unread = [p for p in range(6) if counts[p] == 0]
    assert unread == [3, 4, 5]
    plates, lut = texels(ps, 5), luts(15)
    ctx = make_ctx(bk, table, slots=1)
    frames = []
    for guard in (0x3C, 0xC3):                                         # a guard value and its complement
        g = plates.copy()
        for p in range(6):
            g[p][~FM.texel_mask(masks[p], ps)] = guard
        src = source(g)
        frames.append([run_fb(ctx, src[1], src[2], dest(W, H, ss2), lut if tinted else None, ss2) for _, tinted, ss2 in MODES])
    src = source(plates, skip=unread)
    assert src[1][3] is None and src[1][0] is not None
    frames.append([run_fb(ctx, src[1], [pt if ptr else -12345 for ptr, pt in zip(src[1], src[2])], dest(W, H, ss2), lut if tinted else None, ss2)
                   for _, tinted, ss2 in MODES])
    for i, (name, tinted, ss2) in enumerate(MODES):
        want = model(plates, table, dest(W, H, ss2), lut if tinted else None, ss2)
        for j, what in enumerate(("guard", "complement", "unread plates NULL")):
            np.testing.assert_array_equal(frames[j][i], want, err_msg=f"{name}: {what}")
    ctx.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(bk):
    import torch
    table = oracle_table(PANINI)
    off, tints, W, H, ps = table
    plates = texels(ps, 6)
    ctx = bk.Context()
    ctx.resize(W, H)
    ctx.set_stream(_stream())
    dev, ptrs, pitches = source(plates, "pitch16")
    d = dest(W, H, False)
    dst = torch.full((d["rows"] * d["pitch"],), FILL, dtype=torch.uint8, device="cuda")

    def call(ptrs=ptrs, pitches=pitches, dp=dst.data_ptr(), pitch=d["pitch"], x0=4, y0=2, ss2=False):
        ctx.apply_rgba_fb_device(ptrs, pitches, dp, pitch, x0=x0, y0=y0, ss2=ss2)

    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*no lensmap"):
        call()
    set_table(ctx, table)
    call()                                                             # (the arguments the cases below bend one at a time are fine)
    for bad in (dict(ptrs=[None] + ptrs[1:]),                          # a NULL plate whose footprint is not empty
                dict(pitches=[4 * ps - 4] + pitches[1:]),
                dict(pitches=[pitches[0] + 2] + pitches[1:]),
                dict(ptrs=[ptrs[0] + 2] + ptrs[1:]),
                dict(pitch=4 * (W + 4) - 4),
                dict(pitch=d["pitch"] + 2),
                dict(dp=dst.data_ptr() + 2),
                dict(x0=-1), dict(y0=-1), dict(ss2=2), dict(ss2=-1)):
        with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):
            call(**bad)
    with pytest.raises(bk.BlinkyError, match=r"\[-1\]"):               # the half-size frame's pitch test is its own
        call(pitch=4 * ((W + 1) // 2 + 4) - 4, ss2=True)
    call(ptrs=ptrs[:3] + [None] * 3, pitches=pitches[:3] + [0, 2, -7])   # unread plates: NULL, their pitches ignored
    set_table(ctx, table, rows=(1, H))                                 # ss2 needs whole row pairs
    with pytest.raises(bk.BlinkyError, match=r"\[-6\].*row0"):
        call(ss2=True)
    call()
    set_table(ctx, table, rows=(0, 101))
    with pytest.raises(bk.BlinkyError, match=r"\[-6\]"):
        call(ss2=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(d["rows"], d["pitch"])[-ROWS_BELOW:], FILL)
    ctx.close()


# ---- 5. stripes -----------------------------------------------------------------------------------------------------------------------
def test_two_stripe_contexts_stitch_the_single_context_frame(bk):
    import torch
    table = oracle_table(PANINI)                                       # H = 203: ss2's lone last row
    off, tints, W, H, ps = table
    plates, lut = texels(ps, 7), luts(17)
    dev, ptrs, pitches = source(plates, "pitch16")
    for name, tinted, ss2 in MODES:
        r = 100 if ss2 else 101
        d = dest(W, H, ss2)
        dst = torch.full((d["rows"] * d["pitch"],), FILL, dtype=torch.uint8, device="cuda")
        for rows in ((0, r), (r, H)):
            ctx = make_ctx(bk, table, slots=1, rows=rows)
            ctx.apply_rgba_fb_device(ptrs, pitches, dst.data_ptr(), d["pitch"], x0=d["x0"], y0=d["y0"], lut=lut if tinted else None, ss2=ss2)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(run_fb(ctx, ptrs, pitches, d, lut if tinted else None, ss2),
                                          model(plates, table, d, lut if tinted else None, ss2, rows), err_msg=f"{name} rows {rows}")
            ctx.close()
        np.testing.assert_array_equal(dst.cpu().numpy(), model(plates, table, d, lut if tinted else None, ss2), err_msg=f"{name}: stitched")


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------
def test_one_ring_slot_direct_variant_and_every_lensmap_change(bk):
    table = oracle_table(PANINI)
    off, tints, W, H, ps = table
    plates, lut = texels(ps, 8), luts(18)
    ctx = bk.Context()
    ctx.set_frames(1)
    ctx.set_apply_variant(0)
    ctx.resize(W, H)
    ctx.set_stream(_stream())
    set_table(ctx, table)
    src = source(plates)
    check_modes(ctx, table, plates, lut, src, "one slot, variant 0", existing=False)
    second = (np.ascontiguousarray(off[::-1]), np.ascontiguousarray(tints[::-1]), W, H, ps)      # bk_set_lensmap: a second table
    set_table(ctx, second)
    check_modes(ctx, second, plates, lut, src, "second table", existing=False)
    set_table(ctx, second, rows=(50, 120))                             # bk_set_rows
    check_modes(ctx, second, plates, lut, src, "rows 50..120", rows=(50, 120), existing=False)
    other = oracle_table(STEREO)                                       # bk_resize: another platesize
    ctx.resize(other[2], other[3])
    set_table(ctx, other)
    plates2 = texels(other[4], 9)
    check_modes(ctx, other, plates2, lut, source(plates2, "six-pitches"), "resized", existing=False)
    ctx.close()


def test_interleaved_with_the_other_launches_on_one_context(bk):
    import torch
    table = oracle_table(PANINI)
    off, tints, W, H, ps = table
    plates, lut, lut2 = texels(ps, 10), luts(19), luts(20)
    pal = np.random.default_rng(21).integers(0, 256, (6, 256)).astype(np.uint8)
    ctx = make_ctx(bk, table)
    upload_globe(ctx, plates)
    dev, ptrs, pitches = source(plates, "atlas")

    def fb(tinted_lut, ss2):
        d = dest(W, H, ss2)
        np.testing.assert_array_equal(run_fb(ctx, ptrs, pitches, d, tinted_lut, ss2), model(plates, table, d, tinted_lut, ss2),
                                      err_msg=f"fb lut {tinted_lut is not None} ss2 {ss2}")

    def staged(tinted_lut, ss2=False):
        d = dest(W, H, ss2)
        np.testing.assert_array_equal(run_existing(ctx, d, tinted_lut, ss2), model(plates, table, d, tinted_lut, ss2),
                                      err_msg=f"staged lut {tinted_lut is not None} ss2 {ss2}")

    def apply8():
        dst = torch.full((H, W), FILL, dtype=torch.uint8, device="cuda")
        ctx.apply_device(dst.data_ptr(), W, H * W, frame0=2, rubix_on=True, pal=pal)
        torch.cuda.synchronize()
        want = O.apply(off, tints, W, H, np.ascontiguousarray(plates[..., 2]), np.full((H, W), FILL, np.uint8), W, 0, 0, True, pal)
        np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg="8-bit rubix")

    steps = [lambda: fb(None, False), lambda: staged(None), lambda: fb(lut, False), lambda: staged(lut2), lambda: fb(lut, True),
             apply8, lambda: fb(lut2, False), lambda: staged(lut2, True), lambda: fb(None, True)]
    for step in steps + steps[::-1]:
        step()
    ctx.close()


# ---- 7. a real build --------------------------------------------------------------------------------------------------------------------
def test_after_a_real_build(bk):
    import scripts as S
    cfg = PANINI
    ctx = bk.Context()
    ctx.set_frames(4)
    ctx.set_stream(_stream())
    S.configure(ctx, cfg[0], cfg[1], cfg[2], (cfg[3], cfg[4]))
    display, _ = ctx.build()
    off, tints = ctx.read_lensmap()
    table = (off.reshape(-1), tints.reshape(-1), cfg[3], cfg[4], min(cfg[3], cfg[4]))
    plates, lut = texels(table[4], 11), luts(22)
    upload_globe(ctx, plates)
    unread = [p for p in range(6) if not display[p]]
    assert 0 < len(unread) < 6
    check_modes(ctx, table, plates, lut, source(plates, "pitch+20", skip=unread), "built")
    ctx.close()
