"""TEST INFRASTRUCTURE: random launch SEQUENCES for the truecolour apply campaign (tests/test_apply_rgba_campaign_gpu.py runs them on
a GPU, tests/test_rgba_campaign_cpu.py holds their expectation to a second model and counts what the committed seeds reach).

A seed is one context and everything that happens to it: a frame size down to 1x1, a stripe, a ring of 4..14 slots (R // 4 truecolour
globes, R mostly no multiple of four), a table no lens produces with tints drawn pixel by pixel, the developer knobs (block height,
staging buffer, tuning, the row-major walk), one upload path per globe, then 4-7 launches - plain truecolour, tinted truecolour, 8-bit -
of 1, 2..4 or 5..7 frames at any pitch, origin, frame stride and pointer alignment, with ONE event in the middle: bk_set_lensmap with a
second table, or the LUT array of two tinted launches changed in place between them.  `sequence(seed)` is plain data; `walk` plays the
event and hands every launch the table and LUT it runs with; `expected` is the whole destination allocation after that launch, byte
plane c of a truecolour frame being the oracle's 8-bit apply of plane c (O.apply; through pal = lut[c] with rubix for a tinted launch),
as tests/test_apply_rgba_gpu.py and tests/test_apply_rgba_tint_gpu.py build it.  Nothing here touches a GPU: numpy, the CPU oracle,
the 8-bit campaign's table function and, for the one ablation bit drawn, the enum in the kernel source.  Loading it needs no built library.

The draws are biased by a per-seed FOCUS (small frames, long chunk lists, lists larger than the staging buffer) so that 24 seeds reach
every line of the census in test_rgba_campaign_cpu.py; a focus moves probabilities only, every value it picks also occurs without it.

A SECOND FAMILY, `sequence_ss2(seed)` (tests/test_apply_rgba_ss2_campaign_gpu.py runs it), puts the supersampling apply into such sequences:
launches of five kinds - "ss2" and "ss2_tinted" (bk_apply_rgba_ss2_device, at least half of a sequence's launches) among full-size launches
of both flavours and 8-bit ones on the same stripe and the same block maps - on the stripes that entry point accepts (r0 even, r1 even or
H: two rows, cut off the multiples of 8, the lone last row of an odd H), into HALF-SIZE frames 0 / 4 / 8 bytes into the allocation with a
fourth frame stride (+ 8 mod 16); the event sits in front of an ss2 launch.  Its "direct" focus gives every ss2 launch at least two frames
on at least two truecolour globes, its "wide" focus walks the three alignment classes of a half-size destination at one forced block
height.  `walk`, `expected` and the rest serve both families; an ss2 frame's expectation is quad_means' (tests/test_apply_rgba_ss2_gpu.py).
It has its own base seed and its own draws: `sequence` is untouched by it, which tests/test_rgba_campaign_cpu.py pins with a digest."""
import os
import re

import numpy as np

import oracle_ffi as O
from test_apply_campaign_gpu import SIZES_H, SIZES_W as _SIZES_W8, _table
from test_apply_rgba_ss2_gpu import paste, quad_means
from test_apply_rgba_tint_gpu import random_luts


def ablation_bit(name):
    """the value of a BkAblation bit, read from the enum the launchers compile (blinky_amd/csrc/bk_apply_coop.hip): no number is kept here, and
    loading this module needs no built library"""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "blinky_amd", "csrc", "bk_apply_coop.hip")
    with open(src) as f:
        m = re.findall(r"^\s*%s\s*=\s*(\d+)\s*," % re.escape(name), f.read(), re.M)
    assert len(m) == 1, f"{name}: {len(m)} definitions in bk_apply_coop.hip"
    return int(m[0])


AB_ROW_MAJOR = ablation_bit("BK_AB_ROW_MAJOR")
BASE_SEED = 129000
COMMITTED = range(24)            # the seeds the suite runs; contiguous
SIZES_W = sorted(_SIZES_W8 + [4, 130, 131])
TINT_VALUES = np.array([0, 1, 2, 3, 4, 5, 255], np.uint8)
STAGING_KB = (0, 1, 4, 16, 48, 64)
UPLOAD_PITCH_EXTRA = (0, 4, 20, 21)      # device upload: rows 4 * ps + k bytes apart (20: no multiple of 16, 21: not even of 4)
FILL = 77                                # what the destination holds where nothing is written ...
ROWS_BELOW = 2                           # ... rows of it below every frame (and y0 above)
# the second family (sequence_ss2): bk_apply_rgba_ss2_device among full-size launches, into half-size frames
BASE_SEED_SS2 = 234900
COMMITTED_SS2 = range(24)
SS2_KINDS = ("ss2", "ss2_tinted")
TINTED_KINDS = ("rgba_tinted", "ss2_tinted")
ALIGN_CLASSES = ("16", "8-only", "4-only")       # of (first written byte | pitch | frame stride): 0 mod 16 / 8 mod 16 / 4 mod 8


def kind_of(planes):
    """coop_kind_of (bk_apply_coop.hip): the kind of launch a block map's measured choice is filed under"""
    return 0 if planes <= 1 else 1 if planes <= 16 else 2


def _draw_table(rng, W, H, ps, kinds=None, nulls=None):
    """the 8-bit campaign's table (its own function), of one of `kinds` / `nulls` where a focus asks for them (drawn again until it is);
    tints pixel by pixel from {0..5, 255}: up to seven classes per chunk"""
    for _ in range(200):
        off, _, what = _table(rng, W, H, ps)
        k, n = what.split("/")
        if (kinds is None or k in kinds) and (nulls is None or n in nulls):
            break
    else:
        raise AssertionError(f"no table of {kinds} / {nulls} in 200 draws")
    tints = TINT_VALUES[rng.integers(0, 7, W * H)]
    return off, tints, what


def sequence(seed):
    """-> dict: the whole sequence of this seed as data (tables as arrays, everything else plain numbers and strings)"""
    rng = np.random.default_rng(BASE_SEED + seed)
    focus = str(rng.choice(["none", "small", "lists", "direct", "kinds", "wide"], p=[0.08, 0.35, 0.12, 0.14, 0.19, 0.12]))
    # ---- geometry
    W = int(rng.choice(SIZES_W)) if rng.random() < 0.7 else int(rng.integers(1, 720))
    H = int(rng.choice(SIZES_H)) if rng.random() < 0.7 else int(rng.integers(1, 420))
    small_h = 0
    if focus == "small":                                              # a narrow frame, a frame lower than a forced block, or both
        if rng.random() < 0.55:
            W = int(rng.choice([1, 2, 3])) if rng.random() < 0.4 else int(rng.choice([w for w in SIZES_W if w % 4 or 0 < w % 128 < 4]))
        if rng.random() < 0.7:
            small_h = int(rng.choice([1, 2, 4]))
            H = int(rng.choice([h for h in SIZES_H if h < 8 * small_h]))
    elif focus == "lists":                                            # frames with whole 128 x 32 blocks of a plate that has > 1280 chunks
        W = int(rng.choice([w for w in SIZES_W if w >= 128])) if rng.random() < 0.7 else int(rng.integers(128, 720))
        H = int(rng.choice([h for h in SIZES_H if h >= 100])) if rng.random() < 0.7 else int(rng.integers(100, 420))
    elif focus == "direct":
        W, H = max(W, 17), max(H, 17)
    elif focus == "kinds" and rng.random() < 0.75:                     # a frame of many blocks: the tuning has heights to choose between
        W = int(rng.choice([w for w in SIZES_W if w >= 256]))
        H = int(rng.choice([h for h in SIZES_H if h >= 100]))
    elif focus == "wide":                                             # whole-lane stores: W a multiple of 4, every pixel mapped
        W = int(rng.choice([w for w in SIZES_W if w % 4 == 0 and w >= 128]))
        if H < 32:
            H = int(rng.choice([h for h in SIZES_H if h >= 32]))
    ps = min(W, H)
    r0, r1 = 0, H
    if H > 1 and focus != "lists" and rng.random() < 0.36:
        u = rng.random()
        if u < 0.3:
            r0 = int(rng.integers(0, H))
            r1 = r0 + 1
        elif u < 0.5:
            r0 = int(rng.integers(0, H - 1))
            r1 = r0 + 2
        else:
            r0 = int(rng.integers(0, H - 1))
            r1 = int(rng.integers(r0 + 1, H + 1))
    R = int(rng.integers(4, 15))
    G = R // 4
    # ---- tables
    want = dict(kinds=("random",), nulls=("none", "sprinkled")) if focus in ("lists", "direct") else dict(nulls=("none",)) if focus == "wide" else {}
    tables = [_draw_table(rng, W, H, ps, **want)]
    # ---- context knobs
    shape = int(rng.choice([0, 1, 2, 4]))
    ldskb = int(rng.choice(STAGING_KB))
    tuning = bool(rng.random() < 0.5)
    ablation = AB_ROW_MAJOR if rng.random() < 0.25 else 0
    if small_h:                                                       # a forced block taller than the frame
        shape = small_h
    elif focus == "lists":
        shape, ldskb = 4, 64
    elif focus == "direct":
        shape, ldskb = int(rng.choice([1, 2, 4])), int(rng.choice([1, 4]))
    elif focus == "kinds":                                            # the measured choice, filed per kind of launch and recalled
        shape, tuning = 0, True
    # ---- uploads: per truecolour globe the host upload, or the device upload with rows 4 * ps + k bytes apart
    uploads = [dict(path="host", extra=0) if rng.random() < 0.4 else dict(path="device", extra=int(rng.choice(UPLOAD_PITCH_EXTRA)))
               for _ in range(G)]
    # ---- launches
    n = int(rng.integers(4, 8))
    event_kind = "set_lensmap" if rng.random() < 0.5 else "mutate_lut"
    event_at = int(rng.integers(1, n))                                # the event happens in front of launch `event_at`
    launches = []
    plain_wanted = focus == "direct"                                  # (that focus: lists larger than the buffer in BOTH flavours)
    for i in range(n):
        kind = str(rng.choice(["rgba", "rgba_tinted", "apply8"], p=[0.4, 0.4, 0.2]))
        lut = int(rng.integers(0, 2))
        if event_kind == "mutate_lut" and i in (event_at - 1, event_at):      # two tinted launches through the SAME array object
            kind, lut = "rgba_tinted", 0
        if focus in ("lists", "direct") and i == 0:
            kind = "rgba_tinted"
        elif plain_wanted and i > 0 and not (event_kind == "mutate_lut" and i in (event_at - 1, event_at)):
            kind, plain_wanted = "rgba", False
        rubix = bool(rng.random() < 0.5)
        if kind == "apply8":
            nframes = 1 if rng.random() < 0.5 else R
            first = int(rng.integers(0, R))
        else:
            cls = int(rng.choice(3, p=[0.35, 0.3, 0.35]))
            nframes = 1 if cls == 0 else int(rng.integers(2, 5)) if cls == 1 else int(rng.integers(5, 8))
            first = int(rng.integers(0, 2 * G + 2))
        px_pitch = W + int(rng.integers(0, 9))
        x0 = int(rng.integers(0, px_pitch - W + 1))
        if focus == "wide" and rng.random() < 0.7:
            px_pitch, x0 = W + 4 * int(rng.integers(0, 3)), 4 * int(rng.integers(0, 2))
            x0 = min(x0, px_pitch - W)
        y0 = int(rng.integers(0, 4))
        frame_h = y0 + H + ROWS_BELOW
        bpp = 1 if kind == "apply8" else 4
        pitch = bpp * px_pitch
        s = int(rng.integers(0, 3))                                   # the frame's size / + a multiple of 16 / + 4 mod 16
        extra = 0 if s == 0 else 16 * int(rng.integers(1, 4)) if s == 1 else 4 + 16 * int(rng.integers(0, 3))
        launches.append(dict(kind=kind, rubix=rubix if kind == "apply8" else kind == "rgba_tinted", nframes=nframes, first=first, pitch=pitch,
                             x0=x0, y0=y0, frame_h=frame_h, stride=frame_h * pitch + extra, ptr_off=4 * int(rng.integers(0, 2)), lut=lut))
    event = dict(kind=event_kind, at=event_at)
    if event_kind == "set_lensmap":
        tables.append(_draw_table(rng, W, H, ps, **want))
    else:
        event["lut_seed"] = 3 * seed + 2
    return dict(seed=seed, focus=focus, W=W, H=H, ps=ps, r0=r0, r1=r1, R=R, G=G, tables=tables, shape=shape, ldskb=ldskb, tuning=tuning,
                ablation=ablation, uploads=uploads, globe_seed=31 * seed, lut_seeds=(3 * seed, 3 * seed + 1),
                pal_mul=int(rng.integers(1, 250)), launches=launches, event=event)


def align_class(first, pitch, stride):
    """the class of an ss2 destination the kernel's wide stores depend on (rgba_workgroup's `aligned`: 8 bytes do for RG 1 / 2, RG 4 needs 16)"""
    v = first | pitch | stride
    return ALIGN_CLASSES[0] if v % 16 == 0 else ALIGN_CLASSES[1] if v % 8 == 0 else ALIGN_CLASSES[2]


def ss2_first_byte(seq, L):
    """the first byte an ss2 launch owns: output pixel (x0, y0 + r0 // 2) of frame 0, counted from the 16-byte aligned allocation"""
    return L["ptr_off"] + (L["y0"] + seq["r0"] // 2) * L["pitch"] + 4 * L["x0"]


def _draw_dest(rng, Wd, Hd, bpp, ss):
    """where a launch writes: pixel pitch Wd + 0..8, any origin the pitch allows, y0 0..3, ROWS_BELOW rows below; the pointer 0 / 4 (ss2: / 8)
    bytes into the allocation; frame stride = the frame's size / + a multiple of 16 / + 4 mod 16 (ss2: / + 8 mod 16)"""
    px_pitch = Wd + int(rng.integers(0, 9))
    x0 = int(rng.integers(0, px_pitch - Wd + 1))
    y0 = int(rng.integers(0, 4))
    frame_h = y0 + Hd + ROWS_BELOW
    pitch = bpp * px_pitch
    s = int(rng.integers(0, 4 if ss else 3))
    extra = 0 if s == 0 else 16 * int(rng.integers(1, 4)) if s == 1 else (4 if s == 2 else 8) + 16 * int(rng.integers(0, 3))
    return dict(pitch=pitch, x0=x0, y0=y0, frame_h=frame_h, stride=frame_h * pitch + extra, ptr_off=4 * int(rng.integers(0, 3 if ss else 2)))


def sequence_ss2(seed):
    """-> dict: the sequence of this seed of the SECOND family, the same data as sequence(seed) gives with launches of five kinds - "ss2",
    "ss2_tinted" (at least half of them), "rgba", "rgba_tinted", "apply8" - the stripes bk_apply_rgba_ss2_device accepts (r0 even, r1 even
    or H) and half-size destinations for the ss2 launches.  Its own base seed and its own draws: sequence() is not touched by it."""
    rng = np.random.default_rng(BASE_SEED_SS2 + seed)
    focus = str(rng.choice(["none", "small", "lists", "direct", "kinds", "wide"], p=[0.03, 0.34, 0.08, 0.13, 0.15, 0.27]))
    # ---- geometry
    W = int(rng.choice(SIZES_W)) if rng.random() < 0.7 else int(rng.integers(1, 720))
    H = int(rng.choice(SIZES_H)) if rng.random() < 0.7 else int(rng.integers(1, 420))
    small_h = 0
    if focus == "small":                                              # 1x1, a narrow frame, a frame lower than a forced block, or both
        if rng.random() < 0.15:
            W = H = 1
        else:
            if rng.random() < 0.55:
                W = int(rng.choice([1, 2, 3])) if rng.random() < 0.4 else int(rng.choice([w for w in SIZES_W if w % 2 or 0 < w % 128 < 4]))
            if rng.random() < 0.8:
                small_h = int(rng.choice([1, 2, 4]))
                H = int(rng.choice([h for h in SIZES_H if h < 8 * small_h]))
    elif focus == "lists":                                            # frames with whole 128 x 32 blocks of a plate that has > 1280 chunks
        W = int(rng.choice([w for w in SIZES_W if w >= 128])) if rng.random() < 0.7 else int(rng.integers(128, 720))
        H = int(rng.choice([h for h in SIZES_H if h >= 100])) if rng.random() < 0.7 else int(rng.integers(100, 420))
    elif focus == "direct":
        W, H = max(W, 64), max(H, 17)
    elif focus == "kinds" and rng.random() < 0.75:                     # a frame of many blocks: the tuning has heights to choose between
        W = int(rng.choice([w for w in SIZES_W if w >= 256]))
        H = int(rng.choice([h for h in SIZES_H if h >= 100]))
    elif focus == "wide":                                             # the wide stores: W a multiple of 4, every pixel mapped, whole blocks
        W = int(rng.choice([w for w in SIZES_W if w % 4 == 0 and w >= 128]))
        if H < 32:
            H = int(rng.choice([h for h in SIZES_H if h >= 32]))
    ps = min(W, H)
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    # ---- the stripe: whole row pairs, or the lone last row of an odd H
    r0, r1 = 0, H
    if H > 2 and focus != "lists" and rng.random() < 0.45:
        u = rng.random()
        if u < 0.3 and H % 2:
            r0, r1 = H - 1, H
        elif u < 0.55:
            r0 = 2 * int(rng.integers(0, H // 2))
            r1 = r0 + 2
        else:
            r0 = 2 * int(rng.integers(0, (H + 1) // 2))
            r1 = min(H, r0 + 2 * int(rng.integers(1, (H - r0 + 1) // 2 + 1)))
        if focus == "wide" and r1 - r0 < 32:                          # (that focus: at least 32 rows, cut at any even row)
            r0 = 2 * int(rng.integers(0, (H - 32) // 2 + 1))
            r1 = H if rng.random() < 0.5 else r0 + 32
    R = int(rng.integers(8, 15)) if focus == "direct" else int(rng.integers(4, 15))      # (direct: two truecolour globes at least)
    G = R // 4
    # ---- tables
    want = (dict(kinds=("random",), nulls=("none", "sprinkled")) if focus in ("lists", "direct") else
            dict(kinds=("rows", "columns", "smooth"), nulls=("none",)) if focus == "wide" else {})
    tables = [_draw_table(rng, W, H, ps, **want)]
    # ---- context knobs
    shape = int(rng.choice([0, 1, 2, 4]))
    ldskb = int(rng.choice(STAGING_KB))
    tuning = bool(rng.random() < 0.5)
    ablation = AB_ROW_MAJOR if rng.random() < 0.25 else 0
    if small_h:                                                       # a forced block taller than the frame
        shape = small_h
    elif focus == "lists":
        shape, ldskb = 4, 64
    elif focus == "direct":
        shape, ldskb = int(rng.choice([1, 2, 4])), int(rng.choice([1, 4])) if (r1 - r0) * min(W, 128) > 1024 else 1      # (a stripe of two rows: 1 KiB)
    elif focus == "kinds":                                            # the measured choice, filed per kind of launch and recalled
        shape, tuning = 0, True
    elif focus == "wide":                                             # every block staged, at each forced height
        shape, ldskb = int(rng.choice([1, 2, 4])), 64
    uploads = [dict(path="host", extra=0) if rng.random() < 0.4 else dict(path="device", extra=int(rng.choice(UPLOAD_PITCH_EXTRA)))
               for _ in range(G)]
    # ---- launches: the kinds first
    n = int(rng.integers(4, 8))
    event_kind = "set_lensmap" if rng.random() < 0.5 else "mutate_lut"
    event_at = int(rng.integers(1, n))                                # the event happens in front of launch `event_at`
    kinds = [str(rng.choice(["ss2", "ss2_tinted", "rgba", "rgba_tinted", "apply8"], p=[0.27, 0.27, 0.15, 0.15, 0.16])) for _ in range(n)]
    pinned = set()
    if event_kind == "mutate_lut":                                    # two ss2_tinted launches through the SAME array object
        kinds[event_at - 1] = kinds[event_at] = "ss2_tinted"
        pinned |= {event_at - 1, event_at}
    else:                                                             # the second table in front of an ss2 launch
        if kinds[event_at] not in SS2_KINDS:
            kinds[event_at] = str(rng.choice(SS2_KINDS))
        pinned.add(event_at)
    if focus in ("lists", "direct") and 0 not in pinned:
        kinds[0] = "ss2_tinted"
        pinned.add(0)
    if focus == "direct":                                             # lists larger than the buffer in BOTH flavours
        for k in SS2_KINDS:
            if k not in kinds:
                kinds[[i for i in range(n) if i not in pinned][0]] = k
    need = max(3, (n + 1) // 2) if focus == "wide" else (n + 1) // 2  # at least half are ss2 launches (wide: three, one per alignment class)
    free = [i for i in range(n) if kinds[i] not in SS2_KINDS]
    while n - len(free) < need:
        i = free.pop(int(rng.integers(0, len(free))))
        kinds[i] = {"rgba": "ss2", "rgba_tinted": "ss2_tinted"}.get(kinds[i]) or str(rng.choice(SS2_KINDS))
    launches = []
    wide_j = int(rng.integers(0, 3))
    for i, kind in enumerate(kinds):
        ss = kind in SS2_KINDS
        lut = 0 if event_kind == "mutate_lut" and i in (event_at - 1, event_at) else int(rng.integers(0, 2))
        rubix = bool(rng.random() < 0.5)
        if kind == "apply8":
            nframes = 1 if rng.random() < 0.5 else R
            first = int(rng.integers(0, R))
        else:
            cls = int(rng.choice(3, p=[0.35, 0.3, 0.35]))
            nframes = 1 if cls == 0 else int(rng.integers(2, 5)) if cls == 1 else int(rng.integers(5, 8))
            if focus == "direct" and ss and nframes < 2:              # the direct gather's frame loop: more than one frame per visit
                nframes = int(rng.integers(2, 8))
            first = int(rng.integers(0, 2 * G + 2))
        Wd, Hd, bpp = (Wo, Ho, 4) if ss else (W, H, 1 if kind == "apply8" else 4)
        dest = _draw_dest(rng, Wd, Hd, bpp, ss)
        if focus == "wide" and ss:                                    # the three alignment classes in turn: drawn again until it is that one
            for _ in range(4000):
                if align_class(ss2_first_byte(dict(r0=r0), dest), dest["pitch"], dest["stride"]) == ALIGN_CLASSES[wide_j % 3]:
                    break
                dest = _draw_dest(rng, Wd, Hd, bpp, ss)
            else:
                raise AssertionError(f"no destination of class {ALIGN_CLASSES[wide_j % 3]} in 4000 draws")
            wide_j += 1
        launches.append(dict(kind=kind, rubix=rubix if kind == "apply8" else kind in TINTED_KINDS, nframes=nframes, first=first, lut=lut, **dest))
    event = dict(kind=event_kind, at=event_at)
    if event_kind == "set_lensmap":
        tables.append(_draw_table(rng, W, H, ps, **want))
    else:
        event["lut_seed"] = 3 * seed + 2
    return dict(seed=seed, focus=focus, W=W, H=H, ps=ps, r0=r0, r1=r1, R=R, G=G, tables=tables, shape=shape, ldskb=ldskb, tuning=tuning,
                ablation=ablation, uploads=uploads, globe_seed=31 * seed + 7, lut_seeds=(3 * seed + 100, 3 * seed + 101),
                pal_mul=int(rng.integers(1, 250)), launches=launches, event=event)


def describe(seq, i=None):
    """the configuration in words, for failure messages (with launch i's own numbers)"""
    s = (f"seed {seq['seed']} ({seq['focus']}): {seq['W']}x{seq['H']} ps {seq['ps']} rows [{seq['r0']},{seq['r1']}) ring {seq['R']} "
         f"({seq['G']} truecolour globes) tables {[t[2] for t in seq['tables']]} shape {seq['shape']} lds {seq['ldskb']}K "
         f"tuning {seq['tuning']} ablation {seq['ablation']} uploads {[(u['path'], u['extra']) for u in seq['uploads']]} "
         f"event {seq['event']} kinds {[(l['kind'], l['nframes']) for l in seq['launches']]}")
    if i is not None:
        s += f"\nlaunch {i}: {seq['launches'][i]}"
    return s


def slot_globe(seq, slot):
    """ring slot `slot` as an 8-bit globe, uint8 [6][ps][ps]; slot 4g + c is byte plane c of truecolour globe g"""
    return O.lcg_globe(seq["ps"], 6, seq["globe_seed"] + slot)


def palette(seq):
    """the palette of the sequence's 8-bit rubix launches"""
    return O.palmap(((np.arange(768) * seq["pal_mul"] + 11) % 256).astype(np.uint8))


def walk(seq):
    """plays the event: yields (i, launch, offsets, tints, lut, event) per launch - the FULL table the launch runs on, the LUT array of a
    tinted launch (else None) and the event's kind where it happens in front of this launch (else None).  The two LUT arrays live as long
    as the generator; "mutate_lut" writes new bytes into the first, the same object the launch before was given."""
    luts = [random_luts(s) for s in seq["lut_seeds"]]
    table = 0
    for i, L in enumerate(seq["launches"]):
        ev = None
        if i == seq["event"]["at"]:
            ev = seq["event"]["kind"]
            if ev == "set_lensmap":
                table = 1
            else:
                luts[0][...] = random_luts(seq["event"]["lut_seed"])
        off, tints, _ = seq["tables"][table]
        yield i, L, off, tints, (luts[L["lut"]] if L["kind"] in TINTED_KINDS else None), ev


def oracle_frame(seq, L, off, tints, lut, pal, slots, g, frame):
    """one frame of launch L into `frame` (uint8 [frame_h][pitch], holding the background): truecolour globe g (8-bit: ring slot g)
    applied by the oracle, byte plane by byte plane; rows outside the context's stripe stay as they are.
    An ss2 launch: `frame` is the HALF-SIZE frame, its values quad_means' (tests/test_apply_rgba_ss2_gpu.py: the oracle's samples of the
    full-size frame, (sum + n // 2) // n over the mapped ones inside W x H) in the output rows [r0 // 2, (r1 + 1) // 2) the stripe owns -
    r0 is even and r1 even or H, so every quad of those rows lies in the stripe or below the frame"""
    W, H, r0, r1, x0, y0 = seq["W"], seq["H"], seq["r0"], seq["r1"], L["x0"], L["y0"]
    if L["kind"] in SS2_KINDS:
        means = quad_means(off, tints, W, H, [slots(4 * g + c) for c in range(4)], lut)
        frame[...] = paste(frame, means, x0, y0, rows=(r0 // 2, (r1 + 1) // 2))
        return
    full = frame.copy()
    if L["kind"] == "apply8":
        O.apply(off, tints, W, H, slots(g), full, L["pitch"], x0, y0, L["rubix"], pal)
    else:
        for c in range(4):
            plane = np.ascontiguousarray(full[:, c::4])
            if lut is None:
                O.apply(off, None, W, H, slots(4 * g + c), plane, L["pitch"] // 4, x0, y0)
            else:
                O.apply(off, tints, W, H, slots(4 * g + c), plane, L["pitch"] // 4, x0, y0, True, lut[c])
            full[:, c::4] = plane
    frame[y0 + r0:y0 + r1] = full[y0 + r0:y0 + r1]


def numpy_frame(seq, L, off, tints, lut, pal, slots, g, frame):
    """the same frame a second way, with no oracle call: the four planes interleaved into 32-bit texels, gathered with the raw offsets,
    lut[c][tint] applied where tint < 6, NULL pixels and the rows outside the stripe left alone"""
    W, H, r0, r1, x0, y0 = seq["W"], seq["H"], seq["r0"], seq["r1"], L["x0"], L["y0"]
    off2, tin2 = np.asarray(off).reshape(H, W)[r0:r1], np.asarray(tints).reshape(H, W)[r0:r1]
    mapped = off2 != O.NULL
    idx = np.where(mapped, off2, 0).astype(np.int64)
    classed = mapped & (tin2 < 6)
    t = np.where(classed, tin2, 0).astype(np.int64)
    if L["kind"] == "apply8":
        v = slots(g).reshape(-1)[idx]
        if L["rubix"]:
            v = np.where(classed, pal[t, v], v)
        window = frame[y0 + r0:y0 + r1, x0:x0 + W]
        window[mapped] = v[mapped]
        return
    texels = np.zeros(6 * seq["ps"] ** 2, np.uint32)
    for c in range(4):
        texels |= slots(4 * g + c).reshape(-1).astype(np.uint32) << np.uint32(8 * c)
    px = texels[idx]
    if lut is not None:
        out = np.zeros_like(px)
        for c in range(4):
            b = ((px >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.int64)
            b = np.where(classed, lut[c][t, b], b).astype(np.uint32)
            out |= b << np.uint32(8 * c)
        px = out
    window = frame.view(np.uint32)[y0 + r0:y0 + r1, x0:x0 + W]       # (pitch is a multiple of 4: whole pixels)
    window[mapped] = px[mapped]


def ring_slot(seq, L, f):
    """the truecolour globe (8-bit launch: the ring slot) frame f of launch L is made from"""
    return (L["first"] + f) % (seq["R"] if L["kind"] == "apply8" else seq["G"])


def alloc_bytes(L):
    return L["ptr_off"] + L["nframes"] * L["stride"]


def expected(seq, L, off, tints, lut, pal, slots, frame_fn=oracle_frame):
    """the whole destination allocation after launch L, uint8 [alloc_bytes(L)]: FILL before the pointer, between and below the frames,
    in the padding right of W and in the rows the stripe does not own.  slots(s) -> ring slot s as an 8-bit globe"""
    want = np.full(alloc_bytes(L), FILL, np.uint8)
    size = L["frame_h"] * L["pitch"]
    done = {}
    for f in range(L["nframes"]):
        g = ring_slot(seq, L, f)
        if g not in done:                                             # (every frame has the same background: one frame per globe)
            done[g] = np.full((L["frame_h"], L["pitch"]), FILL, np.uint8)
            frame_fn(seq, L, off, tints, lut, pal, slots, g, done[g])
        at = L["ptr_off"] + f * L["stride"]
        want[at:at + size] = done[g].reshape(-1)
    return want


# ---- what the census reads off a sequence -----------------------------------------------------------------------------------------
def block_chunks(off, tints, seq, rg, tinted):
    """entries of every 128 x 8*rg block's chunk list, counted on the CPU as table_properties (tests/test_apply_rgba_tint_gpu.py) counts
    chunks: a chunk = 16 texels of a plate row; a tinted map lists it once per tint class (tint + 1 below 6, else 0).  Blocks are laid over
    the STRIPE's rows, as the block map is."""
    W, H, ps = seq["W"], seq["H"], seq["ps"]
    o2 = np.asarray(off).reshape(H, W)[seq["r0"]:seq["r1"]]
    t2 = np.asarray(tints).reshape(H, W)[seq["r0"]:seq["r1"]].astype(np.int64)
    counts = []
    for y in range(0, o2.shape[0], 8 * rg):
        for x in range(0, W, 128):
            o, t = o2[y:y + 8 * rg, x:x + 128].ravel(), t2[y:y + 8 * rg, x:x + 128].ravel()
            m = o != O.NULL
            o, t = o[m].astype(np.int64), t[m]
            chunk = (o // ps) * 4096 + (o % ps) // 16
            if tinted:
                chunk = chunk * 8 + np.where(t < 6, t + 1, 0)
            counts.append(len(np.unique(chunk)))
    return counts


def tint_classes_per_chunk(off, tints, seq):
    """the most tint classes any chunk of the stripe's table is read under (table_properties' third value)"""
    W, H, ps = seq["W"], seq["H"], seq["ps"]
    o = np.asarray(off).reshape(H, W)[seq["r0"]:seq["r1"]].ravel()
    t = np.asarray(tints).reshape(H, W)[seq["r0"]:seq["r1"]].ravel().astype(np.int64)
    m = o != O.NULL
    if not m.any():
        return 0
    o, t = o[m].astype(np.int64), t[m]
    pairs = np.unique(((o // ps) * 4096 + (o % ps) // 16) * 8 + np.where(t < 6, t + 1, 0))
    return int(np.unique(pairs >> 3, return_counts=True)[1].max())


def launch_planes(L):
    """what the launcher asks ensure_coopmap for: 8-bit frames, four per truecolour frame"""
    return L["nframes"] if L["kind"] == "apply8" else 4 * L["nframes"]


def launch_aligned16(seq, L):
    """rgba_workgroup's `aligned`: first owned pixel, pitch and frame stride all multiples of 16 bytes (the allocation itself is)"""
    first = L["ptr_off"] + (L["y0"] + seq["r0"]) * L["pitch"] + 4 * L["x0"]
    return (first | L["pitch"] | L["stride"]) % 16 == 0


def features(seq):
    """the census lines this sequence reaches (names as CENSUS in tests/test_rgba_campaign_cpu.py)"""
    W, H, ps, R, G, shape, ldskb = seq["W"], seq["H"], seq["ps"], seq["R"], seq["G"], seq["shape"], seq["ldskb"]
    f = set()
    if W < 4: f.add("W<4")
    if W < 128 and W % 4: f.add("W<128,W%4!=0")
    if W > 128 and 1 <= W % 128 <= 3: f.add("W>128,W%128 in 1..3")
    for rg in (1, 2, 4):
        if shape == rg and H < 8 * rg: f.add(f"H<block height, RG {rg}")
    if ps < 16: f.add("ps<16")
    if ps < 8: f.add("ps<8")
    stripe = (seq["r0"], seq["r1"]) != (0, H)
    if stripe and seq["r1"] - seq["r0"] == 1: f.add("one-row stripe")
    if stripe and seq["r1"] - seq["r0"] == 2: f.add("two-row stripe")
    if stripe and seq["r0"] % 8: f.add("stripe r0%8!=0")
    if R % 4: f.add("R%4!=0")
    if seq["ablation"] & AB_ROW_MAJOR: f.add("BK_AB_ROW_MAJOR")
    if not seq["tuning"]: f.add("tuning off")
    f.add("event " + seq["event"]["kind"])
    for u in seq["uploads"]:
        f.add("upload " + u["path"])
        if u["path"] == "device" and (4 * ps + u["extra"]) % 16: f.add("device upload pitch%16!=0")
        if u["path"] == "device" and (4 * ps + u["extra"]) % 4: f.add("device upload pitch%4!=0")
    counts = {}

    def chunks(table, tinted):
        key = (table, tinted)
        if key not in counts:
            off, tints, _ = seq["tables"][table]
            counts[key] = block_chunks(off, tints, seq, shape, tinted)
        return counts[key]

    table, prev, prev_flavour = 0, None, {}
    for i, L, off, tints, lut, ev in walk(seq):
        if ev == "set_lensmap":
            table, prev, prev_flavour = 1, None, {}                   # (a new lensmap: both block maps start over)
        true = L["kind"] != "apply8"
        flavour = L["rubix"]
        k = kind_of(launch_planes(L))
        if seq["tuning"] and prev is not None and prev != k: f.add("tuning on, consecutive launches change kind")
        if seq["tuning"] and shape == 0 and flavour in prev_flavour and prev_flavour[flavour] != k:
            f.add("tuning on, no forced height: a block map of one flavour meets another kind")   # (coop_recall_kind's own condition)
            if W >= 256 and seq["r1"] - seq["r0"] >= 64: f.add("... on a stripe of at least 256 x 64 pixels")
        prev, prev_flavour[flavour] = k, k
        if not true:
            f.add("apply8 between truecolour launches")
            continue
        tinted = L["kind"] == "rgba_tinted"
        name = "tinted" if tinted else "plain"
        if L["first"] >= G: f.add("globe0>=G")
        if L["nframes"] >= 5: f.add(f">=5 frames, {name}")
        if 2 <= L["nframes"] <= 4: f.add("2..4 frames")
        if L["nframes"] == 1: f.add("1 frame")
        nulls = seq["tables"][table][2].split("/")[1]
        # (... with whole blocks in it: at least 128 x 32 pixels of the stripe, which every block height tiles with fully mapped waves)
        if nulls == "none" and W % 4 == 0 and W >= 128 and seq["r1"] - seq["r0"] >= 32:
            f.add("fully mapped, W%4==0, " + ("16-byte aligned" if launch_aligned16(seq, L) else "not 16-byte aligned"))
        if tinted and tint_classes_per_chunk(off, tints, seq) >= 3: f.add("tinted: a chunk under >=3 classes")
        if shape and ldskb:
            # (unique chunks WITHOUT the class, also for a tinted map, whose lists are no shorter: the conservative count)
            if max(chunks(table, False)) * 16 > ldskb * 1024: f.add(f"staging buffer < a block's list, {name}")
            # (the list itself, classes and all: it must exist - at most 4095 entries, BK_COOP_MAX_CHUNKS - and then fits 64 KiB)
            if tinted and shape == 4 and ldskb == 64 and any(1024 + 256 < n <= 4095 for n in chunks(table, True)):
                f.add("tinted, RG 4, 64 KiB: a block above 1280 chunks")
    return f


def quad_counts(off, seq):
    """-> (n [rows/2][Wo], mapped [2 rows/2][2 Wo]): the mapped samples per 2x2 quad of the STRIPE's rows, samples outside W x H unmapped"""
    W, H, r0, r1 = seq["W"], seq["H"], seq["r0"], seq["r1"]
    m = (np.asarray(off).reshape(H, W)[r0:r1] != O.NULL)
    mapped = np.zeros((m.shape[0] + m.shape[0] % 2, W + W % 2), bool)
    mapped[:m.shape[0], :W] = m
    return sum(mapped[j::2, i::2].astype(np.int64) for j in (0, 1) for i in (0, 1)), mapped


def wide_staged(seq, what, counts):
    """whether a launch on table `what` whose blocks' lists have counts() entries (block_chunks, of the launch's flavour) runs the wide
    stores: fully mapped with whole blocks in it (at least 128 x 32 pixels of the stripe, W a multiple of 4), every block STAGED - its
    list, classes and all, exists (<= 4095 entries, BK_COOP_MAX_CHUNKS) and is a 1 KiB bin of tile_stats' statistic smaller than the forced
    staging buffer"""
    if what.split("/")[1] != "none" or seq["W"] % 4 or seq["W"] < 128 or seq["r1"] - seq["r0"] < 32 or not (seq["shape"] and seq["ldskb"]):
        return False
    longest = max(counts())
    return longest <= 4095 and longest * 16 <= (seq["ldskb"] - 1) * 1024


def features_ss2(seq):
    """the census lines a sequence of the second family reaches (names as CENSUS_SS2 in tests/test_rgba_campaign_cpu.py)"""
    W, H, ps, R, G, shape, ldskb = seq["W"], seq["H"], seq["ps"], seq["R"], seq["G"], seq["shape"], seq["ldskb"]
    r0, r1 = seq["r0"], seq["r1"]
    f = set()
    if W % 2: f.add("W odd")
    if H % 2: f.add("H odd")
    if W < 4: f.add("W<4")
    if W == 1 and H == 1: f.add("W=H=1")
    if W > 128 and 1 <= W % 128 <= 3: f.add("W>128,W%128 in 1..3")
    for rg in (1, 2, 4):
        if shape == rg and H < 8 * rg: f.add(f"H<block height, RG {rg}")
    stripe = (r0, r1) != (0, H)
    if stripe and r1 - r0 == 2: f.add("two-row stripe")
    if stripe and r0 % 8: f.add("stripe r0%8!=0")
    if stripe and H % 2 and (r0, r1) == (H - 1, H): f.add("lone last row of an odd H")
    if R % 4: f.add("R%4!=0")
    if seq["ablation"] & AB_ROW_MAJOR: f.add("BK_AB_ROW_MAJOR")
    if not seq["tuning"]: f.add("tuning off")
    f.add("event " + seq["event"]["kind"])
    for u in seq["uploads"]:
        f.add("upload " + u["path"])
        if u["path"] == "device" and (4 * ps + u["extra"]) % 16: f.add("device upload pitch%16!=0")
        if u["path"] == "device" and (4 * ps + u["extra"]) % 4: f.add("device upload pitch%4!=0")
    counts, quads = {}, {}

    def chunks(table, tinted):
        key = (table, tinted)
        if key not in counts:
            off, tints, _ = seq["tables"][table]
            counts[key] = block_chunks(off, tints, seq, shape, tinted)
        return counts[key]

    kinds = [L["kind"] for L in seq["launches"]]
    table, prev_flavour = 0, {}
    for i, L, off, tints, lut, ev in walk(seq):
        if ev == "set_lensmap":
            table, prev_flavour = 1, {}                               # (a new lensmap: both block maps start over)
        ss, flavour, k = L["kind"] in SS2_KINDS, L["rubix"], kind_of(launch_planes(L))
        if ss and seq["tuning"] and shape == 0 and flavour in prev_flavour and prev_flavour[flavour] != k:
            f.add("tuning on, no forced height: an ss2 launch meets a block map of its flavour filed under another kind")
        prev_flavour[flavour] = k
        if L["kind"] == "apply8":
            if 0 < i < len(kinds) - 1 and kinds[i - 1] in SS2_KINDS and kinds[i + 1] in SS2_KINDS: f.add("apply8 between two ss2 launches")
            continue
        if i and ev != "set_lensmap":                                 # (the same block map: no new lensmap in between)
            full_size = {"ss2": "rgba", "ss2_tinted": "rgba_tinted"}
            if ss and kinds[i - 1] == full_size[L["kind"]]: f.add("ss2 directly after a full-size launch of its flavour")
            if not ss and full_size.get(kinds[i - 1]) == L["kind"]: f.add("full-size directly after an ss2 launch of its flavour")
        if not ss:
            continue
        tinted = L["kind"] == "ss2_tinted"
        name = "tinted" if tinted else "plain"
        if L["first"] >= G: f.add("globe0>=G")
        if L["nframes"] >= 5: f.add(f"ss2 of >=5 frames, {name}")
        if 2 <= L["nframes"] <= 4: f.add("ss2 of 2..4 frames")
        if L["nframes"] == 1: f.add("ss2 of 1 frame")
        if table not in quads:
            quads[table] = quad_counts(off, seq)
        nq, mapped = quads[table]
        if set(np.unique(nq)) == {0, 1, 2, 3, 4}: f.add("ss2: quads of every count 0..4 in the stripe")
        for Y, X in np.argwhere(nq == 3)[:20000]:
            j, k2 = np.argwhere(~mapped[2 * Y:2 * Y + 2, 2 * X:2 * X + 2])[0]
            f.add(f"ss2: n=3, the hole at ({j},{k2})")
        if wide_staged(seq, seq["tables"][table][2], lambda: chunks(table, tinted)):
            f.add(f"fully mapped, W%4==0, staged, RG {shape}, {align_class(ss2_first_byte(seq, L), L['pitch'], L['stride'])}")
        if tinted and tint_classes_per_chunk(off, tints, seq) >= 3: f.add("ss2_tinted: a chunk under >=3 classes")
        if shape and ldskb:
            if L["nframes"] >= 2 and max(chunks(table, False)) * 16 > ldskb * 1024: f.add(f"ss2 of >=2 frames: staging buffer < a block's list, {name}")
            if tinted and shape == 4 and ldskb == 64 and any(1024 + 256 < n <= 4095 for n in chunks(table, True)):
                f.add("ss2_tinted, RG 4, 64 KiB: a block above 1280 chunks")
    return f
