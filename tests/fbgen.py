"""TEST INFRASTRUCTURE: random EVENT AND LAUNCH sequences for the frame-buffer applies (tests/test_apply_rgba_fb_campaign_gpu.py plays them
on a GPU, tests/test_fb_campaign_cpu.py holds their expectation to a second statement and counts what the committed seeds reach).

A seed is one context - a frame from 1x1 to 260x131 (platesizes of 1, 2 and 3 levels, 5..64, and 129 / 130 / 131), a stripe (the full frame,
an odd cut, one row), the sub-texel switch on or off, a ring of 1 or 4 slots - and 10-16 steps on it, each drawn with its arguments:
EVENTS (set_lensmap, set_lensmap_subtexel, set_lensmap_lod, set_lod_bias, set_subtexel, set_seam_table, set_rows, resize, truncate_build,
lut_in_place), LAUNCHES of the five applies (nearest, ss2, bilinear, seams, trilinear with mips 0 or 1; plain or tinted; any source layout,
plates passed as NULL - legal and illegal ones -, any destination origin, pitch and pointer offset) and READS (read_lod, read_subtexel,
read_seam_table, read_mip_level, read_lensmap).  `sequence(seed)` is plain data: numbers, strings and tuples; the arrays a step stands for
are made from its numbers by the functions below (tables by FB.drawn_table, planes by BL.random_subs and TM.random_lods, seam tables by
SE.drawn_seams, plates by FB.texels, LUTs by FB.luts), each once per process.

`Shadow` is the state of a context in plain Python, written from include/blinky_hip.h: the lensmap in place, the sub-texel plane and its
switch, the level-of-detail plane (to be derived / derived / set), the seam table, the mip pyramid plate by plate as last made, the LUT
bytes.  `Shadow.apply(step)` answers ("ok", expected) - the whole destination allocation of a launch, fill included, from the numpy models
of the five applies; the array of a read; None for an event - or ("refused", code, regexp) with the state unchanged.  Where several reasons
for a refusal hold at once the header names no order; the shadow takes the library's: the lensmap, the arguments (a NULL plate), the
sub-texel plane, then the seam table / the pyramid.  `forget` takes one rule away (FORGETFUL): the variants tests/test_fb_campaign_cpu.py
must be able to tell from the true shadow on the committed seeds.

Every seed carries two of the 50 (event, next launch) pairs and the directed steps of one rule of FORGETFUL, in turn, among random steps
that mend a context without a lensmap or a plane more often than not and pick the launch kind the seed has had least of: 48 seeds reach
every line of the census in tests/test_fb_campaign_cpu.py, and no smaller range from 0 does.

Nothing here touches a GPU or the built library.  The generator steers its draws with a Shadow of its own (no frames are computed for
that): it knows which plates the lensmap in place names, whether the stripe takes an ss2 launch, which LUT the last tinted launch used."""
import hashlib
import json

import numpy as np

import rgba_fb_model as M
import seam_model as SEM
import subtexel_model as SM
import test_apply_rgba_fb_bilinear_gpu as BL
import test_apply_rgba_fb_gpu as FB
import test_apply_rgba_fb_seams_gpu as SE
import trilinear_model as TM

NULL = SM.NULL
CENTRE = SM.CENTRE
FILL = FB.FILL
BASE_SEED = 377000
COMMITTED = range(48)            # the seeds the suite runs; contiguous
E_INVALID, E_STATE = -1, -6

LAUNCHES = ("nearest", "ss2", "bilinear", "seams", "trilinear")
EVENTS = ("set_lensmap", "set_lensmap_subtexel", "set_lensmap_lod", "set_lod_bias", "set_subtexel", "set_seam_table", "set_rows", "resize",
          "truncate_build", "lut_in_place")
READS = ("read_lod", "read_subtexel", "read_seam_table", "read_mip_level", "read_lensmap")
BIASES = (-300, 0, 40, 300)
MESSAGES = ("no lensmap", "sub-texel plane", "mips = 0", "no valid globe", "is NULL, but the lensmap reads", "above")
# W x H by class; ps = min(W, H).  ps 1, 2, 3: pyramids of 1, 2 and 3 levels; mid: ps 5..64; deep: ps 129, 130, 131 (two head tiles across, the
# clamp at an odd level size); W % 4 != 0 in most, W < 4 in (1, 1) (1, 4) (2, 3) (2, 2) (3, 9) (3, 3)
SIZES = {"ps1": [(1, 1), (5, 1), (1, 4)], "ps2": [(5, 2), (2, 3), (2, 2)], "ps3": [(3, 9), (130, 3), (3, 3)],
         "mid": [(131, 9), (130, 10), (17, 33), (64, 64), (66, 40), (33, 5)], "deep": [(133, 130), (130, 131), (260, 129), (131, 260)]}
CLASS_OF_SEED = ("deep", "ps1", "mid", "mid", "ps2", "deep", "mid", "ps3", "mid")
MAX_W, MAX_H = 264, 260
PAIRS = [(e, k) for e in EVENTS for k in LAUNCHES]       # every (event, next launch) pair: two a seed, in turn
SCENARIOS = (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)      # the rules of FORGETFUL a few directed steps can show: one a seed, in turn
MAX_STEPS = 16


class _Full(Exception):
    """the sequence has its 16 steps"""


# the rules a forgetful shadow leaves out, numbered as tests/test_fb_campaign_cpu.py lists them
FORGETFUL = {
    1: "lod kept by set_lensmap", 2: "lod kept by set_lensmap_subtexel", 3: "lod kept by truncate_build", 4: "lod kept by a real bias change",
    5: "lod kept by a real switch change", 6: "set lod dropped by a same-value bias or switch", 7: "sub not recentred by set_lensmap",
    8: "sub not recentred where truncate_build NULLs", 9: "lensmap survives a same-height set_rows", 10: "lensmap survives a same-pixel-count resize",
    11: "seam table survives a resize", 12: "pyramid dropped by a same-platesize resize", 13: "pyramid survives a platesize change",
    14: "a NULL plate's levels zeroed", 15: "mips = 0 shows this call's plates", 16: "a LUT changed in place is not seen", 17: "a refused call changes state"}

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        a = make()
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
        _CACHE[key] = a
    return _CACHE[key]


# ---- the arrays a step's numbers stand for (whole frames; a context is handed its owned rows) -----------------------------------------
def table_of(W, H, tseed, drop):
    """(off, tints) of FB.drawn_table(W, H, tseed) with every entry on a plate in `drop` NULLed: those plates may then be passed as NULL"""
    def make():
        off, tints, _, _, ps = FB.drawn_table(W, H, tseed)
        off = np.where(np.isin(off.astype(np.int64) // (ps * ps), list(drop)), NULL, off).astype(np.uint32)
        off.flags.writeable = False
        return off, tints
    return _cached(("table", W, H, tseed, tuple(drop)), make)


def subs_of(W, H, sseed):
    return _cached(("sub", W, H, sseed), lambda: BL.random_subs(W * H, 10 * sseed + W + H))


def lods_of(W, H, lseed):
    return _cached(("lod", W, H, lseed), lambda: TM.random_lods(W * H, min(W, H), 10 * lseed + W + H))


def seams_of(ps, sseed):
    return _cached(("seam", ps, sseed), lambda: SE.drawn_seams(ps, sseed))


def plates_of(ps, pid):
    return _cached(("plates", ps, pid), lambda: FB.texels(ps, 300 + pid))


def pyramid_of(ps, pid):
    """TM.pyramid of plates_of(ps, pid), once per set of plates"""
    return _cached(("pyramid", ps, pid), lambda: TM.pyramid(plates_of(ps, pid)))


def pyramid_loops_of(ps, pid):
    def make():
        per_plate = [TM.pyramid_loops(plates_of(ps, pid)[p]) for p in range(6)]
        return [np.stack([per_plate[p][k] for p in range(6)]) for k in range(len(per_plate[0]))]
    return _cached(("pyramid_loops", ps, pid), make)


def luts_of(lseed):
    return FB.luts(700 + lseed)


def rows_of(a, W, r0, r1):
    return np.asarray(a)[r0 * W:r1 * W]


def dest_of(W, H, st):
    """FB.dest of a launch step: dict(pitch, x0, y0, rows) of the frame it writes (the half-size one for ss2)"""
    return FB.dest(W, H, st["kind"] == "ss2", x0=st["x0"], y0=st["y0"], extra_px=st["extra_px"])


def scan_keys(W, r0, r1):
    """the scan key + 1 of every pixel of the owned rows [r0, r1), as launch_truncate_scan counts it: ly * W + (W - 1 - lx) + 1 with ly the
    row in the WHOLE frame - a stripe's keys start at r0 * W + 1 -, and bk_truncate_build(bad_key) NULLs every entry whose key <= bad_key
    (tests/test_subtexel_gpu.py:149-157 is the full-frame form)"""
    i = np.arange((r1 - r0) * W)
    return (r0 + i // W) * W + (W - 1 - i % W) + 1


def ss2_allowed(H, r0, r1):
    """fb_apply_args: whole row pairs - row0 even, row1 even or H"""
    return r0 % 2 == 0 and (r1 % 2 == 0 or r1 == H)


def first_byte(st, d, r0):
    """the first byte a launch owns, counted from the 16-byte aligned allocation"""
    return st["ptr_off"] + (d["y0"] + (r0 // 2 if st["kind"] == "ss2" else r0)) * d["pitch"] + 4 * d["x0"]


# ---- the two sets of models ----------------------------------------------------------------------------------------------------------------
class Vector:
    """the vectorised numpy models: what the GPU campaign is compared with"""
    fb_frame = staticmethod(M.fb_frame)
    bilinear_frame = staticmethod(SM.bilinear_frame)
    seam_frame = staticmethod(SEM.seam_frame)
    trilinear_frame = staticmethod(TM.trilinear_frame)
    derive_lod = staticmethod(TM.derive_lod)
    pyramid = staticmethod(pyramid_of)


class Loops:
    """their loop twins.  rgba_fb_model has none: the nearest frame is the bilinear loops' with a plane of centres (the header's identity),
    the ss2 frame tests/test_apply_rgba_ss2_gpu.py's quad_means - the CPU oracle's samples, averaged - pasted as rgbagen.oracle_frame does"""
    bilinear_frame = staticmethod(SM.bilinear_frame_loops)
    seam_frame = staticmethod(SEM.seam_frame_loops)
    trilinear_frame = staticmethod(TM.trilinear_frame_loops)
    derive_lod = staticmethod(TM.derive_lod_loops)
    pyramid = staticmethod(pyramid_loops_of)

    @staticmethod
    def fb_frame(plates, off, tints, W, H, ps, rows, lut, ss2, frame, x0, y0):
        if not ss2:
            return SM.bilinear_frame_loops(plates, off, np.full(W * H, CENTRE, np.uint16), tints, W, H, ps, rows, lut, frame, x0, y0)
        from test_apply_rgba_ss2_gpu import paste, quad_means
        planes = [np.ascontiguousarray(np.asarray(plates)[..., c]) for c in range(4)]
        frame[...] = paste(frame, quad_means(off, tints, W, H, planes, lut), x0, y0, rows=(rows[0] // 2, (rows[1] + 1) // 2))
        return frame


# ---- the shadow ----------------------------------------------------------------------------------------------------------------------------
class Shadow:
    """the state of one context and what every step does to it.  forget: numbers of FORGETFUL; frames False: outcomes and state only, no
    expectation is computed (the generator's steering, the state walk); models: Vector or Loops"""

    def __init__(self, W, H, rows, sub_on, forget=(), frames=True, models=Vector):
        self.W, self.H, self.ps = W, H, min(W, H)
        self.r0, self.r1 = rows
        self.sub_on = bool(sub_on)
        self.forget, self.frames, self.models = frozenset(forget), frames, models
        self.off = self.tints = None         # the lensmap in place (owned rows), or None
        self.sub = None                      # the sub-texel plane (owned rows), or None
        self.bias = 0
        self.lod = ("derive", 0)             # ("derive", bias): to be derived on first use | ("derived", plane) | ("set", plane)
        self.seam = None                     # the seam table, or None (these contexts have no globe: none can be computed)
        self.mip = None                      # dict(ps, levels [k] -> uint8 [6][s_k][s_k][4] for k >= 1, src [plate] -> the set of plates its levels were made from)
        self.luts = {0: luts_of(0), 1: luts_of(1)}      # the caller's two LUT arrays, as they are now
        self.last_lut = None                 # (which, bytes) of the last tinted launch: the library's copy

    # -- what the tests read off it
    def kinds(self):
        """the kind of every piece of state, no arrays"""
        return dict(lensmap="there" if self.off is not None else "none", sub="there" if self.sub is not None else "none",
                    lod="set" if self.lod[0] == "set" else "derive", seam="there" if self.seam is not None else "none",
                    pyramid="there" if self.mip is not None else "none")

    def named(self):
        """the plates the lensmap in place names in the owned rows (the footprint is empty for every other one); none without a lensmap"""
        if self.off is None:
            return set()
        return set((self.off[self.off != NULL].astype(np.int64) // (self.ps * self.ps)).tolist())

    def levels(self):
        return len(TM.level_sizes(self.ps))

    def px(self):
        return (self.r1 - self.r0) * self.W

    # -- helpers
    def _drop_lod(self, rule=None):
        if rule is None or rule not in self.forget:
            self.lod = ("derive", self.bias)

    def _full(self, a, fill, dtype):
        out = np.full(self.W * self.H, fill, dtype)
        out[self.r0 * self.W:self.r1 * self.W] = a
        return out

    def _lod_plane(self):
        if self.lod[0] == "derive":
            plane = self.models.derive_lod(self.off, self.sub, self.W, self.r1 - self.r0, self.ps, self.lod[1]) if self.frames else None
            self.lod = ("derived", plane)
        return self.lod[1]

    def _drop_lensmap(self):
        self.off = self.tints = self.sub = None
        self._drop_lod()

    def _make_pyramid(self, st):
        L = self.levels()
        if self.mip is None or self.mip["ps"] != self.ps:                  # allocated, every level zero
            self.mip = dict(ps=self.ps, levels=[None] + [np.zeros((6, s, s, 4), np.uint8) for s in TM.level_sizes(self.ps)[1:]], src=[None] * 6)
        pyr = self.models.pyramid(self.ps, st["plates"]) if self.frames else None
        for p in range(6):
            if p in st["nulls"]:                                           # a NULL plate's levels stay as they were
                if 14 in self.forget:
                    self.mip["src"][p] = None
                    for k in range(1, L):
                        self.mip["levels"][k][p] = 0
                continue
            self.mip["src"][p] = st["plates"]
            for k in range(1, L):
                if self.frames:
                    self.mip["levels"][k][p] = pyr[k][p]

    # -- events
    def _set_lensmap(self, st):
        off, tints = table_of(self.W, self.H, st["table"], st["drop"])
        self.off, self.tints = rows_of(off, self.W, self.r0, self.r1).copy(), rows_of(tints, self.W, self.r0, self.r1).copy()
        if not self.sub_on:
            self.sub = None
        elif self.sub is None or 7 not in self.forget:                     # every entry at its texel's centre
            self.sub = np.full(self.px(), CENTRE, np.uint16)
        self._drop_lod(1)
        return ("ok", None)

    def _set_lensmap_subtexel(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        if not self.sub_on:
            return ("refused", E_STATE, "switched off")
        self.sub = rows_of(subs_of(self.W, self.H, st["sub"]), self.W, self.r0, self.r1).copy()
        self._drop_lod(2)
        return ("ok", None)

    def lod_argument(self, st):
        """the plane a set_lensmap_lod step passes: TM.random_lods', its first entry one above the top where the step says `over`"""
        plane = rows_of(lods_of(self.W, self.H, st["lod"]), self.W, self.r0, self.r1).copy()
        if st["over"]:
            plane[0] = (self.levels() - 1) * 256 + 1
        return plane

    def _set_lensmap_lod(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        if self.sub is None:
            return ("refused", E_STATE, "sub-texel plane")
        plane = self.lod_argument(st)
        if st["over"]:
            if 17 in self.forget:
                self.lod = ("set", np.minimum(plane, (self.levels() - 1) * 256).astype(np.uint16))
            return ("refused", E_INVALID, "above")
        self.lod = ("set", plane)
        return ("ok", None)

    def _set_lod_bias(self, st):
        if st["bias"] != self.bias:                                        # a real change drops the plane, a set one too
            self.bias = st["bias"]
            if self.lod[0] == "derive" or 4 not in self.forget:
                self._drop_lod()
        elif 6 in self.forget:
            self._drop_lod()
        return ("ok", None)

    def _set_subtexel(self, st):
        if not st["on"]:
            self.sub = None
        if st["on"] != self.sub_on:
            self._drop_lod(5)
        elif 6 in self.forget:
            self._drop_lod()
        self.sub_on = st["on"]                                             # (switched on over a lensmap in place: no plane until one is set)
        return ("ok", None)

    def _set_seam_table(self, st):
        self.seam = seams_of(self.ps, st["seams"])
        return ("ok", None)

    def _set_rows(self, st):
        r0, r1 = st["rows"]
        if (r0, r1) == (self.r0, self.r1):
            return ("ok", None)
        same_height = r1 - r0 == self.r1 - self.r0
        self.r0, self.r1 = r0, r1
        if not (same_height and 9 in self.forget):
            self._drop_lensmap()                                           # the seam table and the pyramid stay
        return ("ok", None)

    def _resize(self, st):
        W, H = st["size"]
        if (W, H) == (self.W, self.H):
            return ("ok", None)                                            # the size it has: nothing changes, a stripe stays
        same_px, same_ps = W * H == self.px(), min(W, H) == self.ps
        self.W, self.H, self.ps = W, H, min(W, H)
        self.r0, self.r1 = 0, H
        if not (same_px and 10 in self.forget):
            self._drop_lensmap()
        if not (same_ps and 11 in self.forget):
            self.seam = None
        if self.mip is not None:
            if not same_ps and 13 in self.forget:
                self.mip = dict(ps=self.ps, levels=[None] + [np.zeros((6, s, s, 4), np.uint8) for s in TM.level_sizes(self.ps)[1:]], src=[None] * 6)
            elif not same_ps or 12 in self.forget:
                self.mip = None                                            # kept across a resize that keeps the platesize
        return ("ok", None)

    def _truncate_build(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        if st["key"] == 0:
            return ("ok", None)
        cut = scan_keys(self.W, self.r0, self.r1) <= st["key"]
        self.off[cut], self.tints[cut] = NULL, 255
        if self.sub is not None and 8 not in self.forget:
            self.sub[cut] = CENTRE                                         # what it NULLs goes back to the centre
        self._drop_lod(3)
        return ("ok", None)

    def _lut_in_place(self, st):
        self.luts[st["lut"]] = luts_of(st["bytes"])
        return ("ok", None)

    # -- reads
    def _read_lensmap(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        return ("ok", (self.off.copy(), self.tints.copy()))

    def _read_subtexel(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        if not self.sub_on:
            return ("refused", E_STATE, "switched off")
        if self.sub is None:
            return ("refused", E_STATE, "before bk_set_subtexel")
        return ("ok", self.sub.copy())

    def _read_lod(self, st):
        if self.off is None:
            return ("refused", E_STATE, "no lensmap")
        if self.sub is None:
            return ("refused", E_STATE, "sub-texel plane")
        plane = self._lod_plane()
        return ("ok", None if plane is None else plane.copy())

    def _read_seam_table(self, st):
        if self.seam is None:
            return ("refused", E_STATE, "no valid globe")
        return ("ok", np.asarray(self.seam).copy())

    def _read_mip_level(self, st):
        if self.mip is None:
            return ("refused", E_STATE, "no pyramid")
        if not 1 <= st["level"] < self.levels():
            return ("refused", E_INVALID, "plate %d, level %d" % (st["plate"], st["level"]))
        return ("ok", self.mip["levels"][st["level"]][st["plate"]].copy())

    # -- launches
    def _launch(self, st):
        kind = st["kind"]
        refusal = None
        if self.off is None:
            refusal = ("refused", E_STATE, "no lensmap")
        elif set(st["nulls"]) & self.named():
            refusal = ("refused", E_INVALID, "is NULL, but the lensmap reads")
        elif kind in ("bilinear", "seams", "trilinear") and self.sub is None:
            refusal = ("refused", E_STATE, "sub-texel plane")
        elif kind == "seams" and self.seam is None:
            refusal = ("refused", E_STATE, "no valid globe")
        elif kind == "trilinear" and not st["mips"] and self.mip is None:
            refusal = ("refused", E_STATE, "mips = 0")
        if refusal:
            if 17 in self.forget and kind == "trilinear" and st["mips"]:
                self._make_pyramid(st)
            return refusal
        assert kind != "ss2" or ss2_allowed(self.H, self.r0, self.r1), "the generator draws ss2 only on a stripe of whole row pairs"
        lut = None
        if st["lut"] is not None:                                          # the bytes as they are NOW: a LUT changed in place is seen
            lut = self.luts[st["lut"]]
            if 16 in self.forget and self.last_lut is not None and self.last_lut[0] == st["lut"]:
                lut = self.last_lut[1]
            self.last_lut = (st["lut"], lut)
        lod = self._lod_plane() if kind == "trilinear" else None
        if kind == "trilinear" and st["mips"]:
            self._make_pyramid(st)
        if not self.frames:
            return ("ok", None)
        W, H, ps, rows = self.W, self.H, self.ps, (self.r0, self.r1)
        d = dest_of(W, H, st)
        want = np.full(st["ptr_off"] + d["rows"] * d["pitch"], FILL, np.uint8)
        frame = want[st["ptr_off"]:].reshape(d["rows"], d["pitch"])
        plates = plates_of(ps, st["plates"])
        off, tints = self._full(self.off, NULL, np.uint32), self._full(self.tints, 255, np.uint8)
        sub = None if self.sub is None else self._full(self.sub, CENTRE, np.uint16)
        if kind in ("nearest", "ss2"):
            self.models.fb_frame(plates, off, tints, W, H, ps, rows, lut, kind == "ss2", frame, d["x0"], d["y0"])
        elif kind == "bilinear":
            self.models.bilinear_frame(plates, off, sub, tints, W, H, ps, rows, lut, frame, d["x0"], d["y0"])
        elif kind == "seams":
            given = tuple(p not in st["nulls"] for p in range(6))
            self.models.seam_frame(plates, off, sub, tints, W, H, ps, rows, lut, frame, d["x0"], d["y0"], self.seam, given)
        else:                                                              # level 0 from the plates given, the others as the pyramid holds them
            pyr = [plates] + (self.models.pyramid(ps, st["plates"])[1:] if 15 in self.forget and not st["mips"] else self.mip["levels"][1:])
            self.models.trilinear_frame(pyr, off, sub, lod, tints, W, H, ps, rows, lut, frame, d["x0"], d["y0"])
        return ("ok", want)

    def apply(self, st):
        """-> ("ok", expected) | ("refused", code, regexp); the state moves on an "ok" only"""
        return getattr(self, "_" + st["op"])(st)


# ---- the generator -------------------------------------------------------------------------------------------------------------------------
def _draw_rows(rng, H, not_height=None):
    """the full frame, an odd cut, an even cut or one row"""
    for _ in range(100):
        u = rng.random()
        if H == 1 or u < 0.4:
            rows = (0, H)
        elif u < 0.6:
            r0 = int(rng.integers(0, H))
            rows = (r0, r0 + 1)
        elif u < 0.8 and H >= 3:                                           # an odd cut: the stripe starts or ends at an odd row
            r0 = 2 * int(rng.integers(0, (H - 1) // 2)) + 1
            rows = (r0, int(rng.integers(r0 + 1, H + 1)))
        else:                                                              # whole row pairs
            r0 = 2 * int(rng.integers(0, (H + 1) // 2))
            rows = (r0, min(H, r0 + 2 * int(rng.integers(1, (H - r0 + 1) // 2 + 1))))
        if rows[1] - rows[0] != not_height:
            return rows
    return (0, H)


def sequence(seed):
    """-> dict: the context and the steps of this seed, plain data"""
    rng = np.random.default_rng(BASE_SEED + seed)
    cls = CLASS_OF_SEED[seed % len(CLASS_OF_SEED)]
    W, H = SIZES[cls][int(rng.integers(0, len(SIZES[cls])))]
    rows = _draw_rows(rng, H)
    sub_on = bool(rng.random() < 0.85)
    slots = int(rng.choice([1, 4]))
    sh = Shadow(W, H, rows, sub_on, frames=False)
    steps, queue = [], []
    state = dict(want_kind=None, force_lut=None, last_nulls=(), back=None, done=dict.fromkeys(LAUNCHES, 0))

    def emit(st):
        if len(steps) == MAX_STEPS:
            raise _Full
        steps.append(st)
        if sh.apply(st)[0] == "ok" and st["op"] == "launch":
            state["done"][st["kind"]] += 1

    def draw_launch(kind=None):
        if kind is None:                                                   # (a kind the state in place refuses: a fifth of its weight)
            w = np.array([0.17, 0.2, 0.15, 0.26, 0.22])
            w[2:] *= 1.0 if sh.sub is not None else 0.2
            w[3] *= 1.0 if sh.seam is not None else 0.2
            kind = state["want_kind"] if state["want_kind"] and rng.random() < 0.5 else str(rng.choice(LAUNCHES, p=w / w.sum()))
            fine = [k for k in LAUNCHES if (k != "ss2" or ss2_allowed(sh.H, sh.r0, sh.r1)) and (k in ("nearest", "ss2") or sh.sub is not None)
                    and (k != "seams" or sh.seam is not None)]
            if state["want_kind"] is None and sh.off is not None and rng.random() < 0.75:      # the kind this seed has had least of, among those the state takes
                least = min(state["done"][k] for k in fine)
                kind = str(rng.choice([k for k in fine if state["done"][k] == least]))
        state["want_kind"] = None
        if kind == "ss2" and not ss2_allowed(sh.H, sh.r0, sh.r1):          # (ss2 only where fb_apply_args allows it)
            kind = "nearest"
        lut = int(rng.integers(0, 2)) if rng.random() < 0.5 else None
        if state["force_lut"] is not None:
            lut, state["force_lut"] = state["force_lut"], None
        mips = None
        if kind == "trilinear":
            mips = bool(rng.random() < (0.45 if sh.mip is not None else 0.8))
        plates = int(rng.integers(0, 3))
        if kind == "trilinear" and not mips and sh.mip is not None and rng.random() < 0.7:      # plates newer than the pyramid's levels
            plates = int(rng.choice([p for p in range(3) if p != next((s for s in sh.mip["src"] if s is not None), -1)]))
        named = sh.named()
        unnamed = [p for p in range(6) if p not in named]
        nulls, u = (), rng.random()
        if sh.off is not None and unnamed and u < 0.45:                    # legal: plates whose footprint is empty
            nulls = tuple(unnamed) if rng.random() < 0.5 else tuple(sorted(rng.choice(unnamed, int(rng.integers(1, len(unnamed) + 1)), replace=False).tolist()))
        elif sh.off is not None and named and u > 0.93:                    # illegal: one the lensmap reads (and the unread ones)
            nulls = tuple(sorted([int(rng.choice(sorted(named)))] + (unnamed if rng.random() < 0.5 else [])))
        Wd = (sh.W + 1) // 2 if kind == "ss2" else sh.W
        x0, y0, ptr_off = int(rng.integers(0, 6)), int(rng.integers(0, 4)), 4 * int(rng.integers(0, 3))
        extra_px = x0 + int(rng.integers(0, 9))
        if rng.random() < 0.3:                                             # the 16-byte class: pitch, origin and pointer all multiples of 16
            x0, ptr_off = 4 * int(rng.integers(0, 2)), 0
            extra_px = x0 + (-(Wd + x0)) % 4 + 4 * int(rng.integers(0, 2))
        if kind == "trilinear" and mips:
            state["last_nulls"] = nulls
        return dict(op="launch", kind=kind, lut=lut, mips=mips, layout=str(rng.choice(FB.LAYOUTS)), plates=plates, nulls=nulls, x0=x0, y0=y0,
                    extra_px=extra_px, ptr_off=ptr_off)

    def draw_size(kind):
        """the four kinds of resize: the same size; W x H -> H x W; the same platesize with another pixel count; another platesize"""
        W, H = sh.W, sh.H
        if kind == "swap" and W != H and H <= MAX_W and W <= MAX_H:
            return (H, W)
        if kind in ("swap", "same_ps"):                                    # the longer side grows (at the limit: shrinks), min(W, H) stays
            by = int(rng.integers(1, 4))
            if W >= H:
                return (W + by, H) if W + by <= MAX_W else (max(W - by, H), H)
            return (W, H + by) if H + by <= MAX_H else (W, max(H - by, W))
        if kind == "other_ps":
            pool = [s for c in (("mid",) if cls in ("mid", "deep") else ("ps1", "ps2", "ps3")) for s in SIZES[c] if min(s) != sh.ps]
            return pool[int(rng.integers(0, len(pool)))]
        return (W, H)

    def draw_event(op, next_kind=None):
        if op == "set_lensmap":
            drop, u = (), rng.random()
            if u < 0.55:
                drop = tuple(sorted(rng.choice(6, int(rng.integers(1, 5)), replace=False).tolist()))
            return dict(op=op, table=int(rng.integers(0, 4)), drop=drop)
        if op == "set_lensmap_subtexel":
            return dict(op=op, sub=int(rng.integers(0, 4)))
        if op == "set_lensmap_lod":
            return dict(op=op, lod=int(rng.integers(0, 4)), over=bool(rng.random() < 0.15))
        if op == "set_lod_bias":
            same = rng.random() < 0.35
            return dict(op=op, bias=sh.bias if same else int(rng.choice([b for b in BIASES if b != sh.bias])))
        if op == "set_subtexel":
            return dict(op=op, on=sh.sub_on if rng.random() < 0.4 else not sh.sub_on)
        if op == "set_seam_table":
            return dict(op=op, seams=int(rng.integers(0, 4)))
        if op == "set_rows":
            u, h = rng.random(), sh.r1 - sh.r0
            moved = [(r, r + h) for r in range(sh.H - h + 1) if r != sh.r0 and (next_kind != "ss2" or ss2_allowed(sh.H, r, r + h))]
            if next_kind is not None and moved:                            # in front of a pair's launch: the same height somewhere else
                rows = moved[int(rng.integers(0, len(moved)))]
            elif next_kind == "ss2":                                       # (a stripe the ss2 launch behind it is allowed on)
                for _ in range(100):
                    rows = _draw_rows(rng, sh.H)
                    if ss2_allowed(sh.H, *rows):
                        break
                else:
                    rows = (0, sh.H)
            elif u < 0.2 or sh.H == 1:
                rows = (sh.r0, sh.r1)                                      # the same stripe
            elif u < 0.65 and h < sh.H:                                    # a stripe of the same height somewhere else
                rows = (sh.r0, sh.r1)
                while rows == (sh.r0, sh.r1):
                    r0 = int(rng.integers(0, sh.H - h + 1))
                    rows = (r0, r0 + h)
            else:
                rows = _draw_rows(rng, sh.H, not_height=h)
            return dict(op=op, rows=rows)
        if op == "resize":
            kind = str(rng.choice(["same", "swap", "same_ps", "other_ps"], p=[0.12, 0.33, 0.3, 0.25]))
            if kind == "other_ps" and state["back"] is None:
                state["back"] = (len(steps) + int(rng.integers(3, 6)), (sh.W, sh.H))      # ... and back again a few steps later
            return dict(op=op, size=draw_size(kind))
        if op == "truncate_build":
            if rng.random() < 0.12:
                return dict(op=op, key=0)
            keys = scan_keys(sh.W, sh.r0, sh.r1)                           # the key of one pixel of the stripe
            return dict(op=op, key=int(keys[int(rng.integers(0, len(keys)))]))
        if op == "lut_in_place":
            which = sh.last_lut[0] if sh.last_lut is not None else int(rng.integers(0, 2))
            state["force_lut"] = which
            return dict(op=op, lut=which, bytes=int(rng.integers(2, 40)))
        raise AssertionError(op)

    def draw_read(op=None):
        op = op or str(rng.choice(READS))
        if op == "read_mip_level":
            L = sh.levels()
            plate = int(rng.choice(state["last_nulls"])) if state["last_nulls"] and rng.random() < 0.6 else int(rng.integers(0, 6))
            return dict(op=op, plate=plate, level=int(rng.integers(1, L)) if L > 1 else 1)
        return dict(op=op)

    # what tells whether an event was taken in: the launch that reads the state it changes, and the read of it
    relevant = {"set_lensmap": (None, "read_lod"), "set_lensmap_subtexel": ("trilinear", "read_lod"), "set_lensmap_lod": ("trilinear", "read_lod"),
                "set_lod_bias": ("trilinear", "read_lod"), "set_subtexel": ("bilinear", "read_subtexel"), "set_seam_table": ("seams", "read_seam_table"),
                "set_rows": (None, "read_lensmap"), "resize": (None, "read_mip_level"), "truncate_build": ("bilinear", "read_subtexel"),
                "lut_in_place": (None, None)}

    def after_event(st):
        kind, read = relevant[st["op"]]
        state["want_kind"] = kind
        if read and rng.random() < 0.2:
            if st["op"] == "resize" and rng.random() < 0.5:
                read = "read_seam_table" if rng.random() < 0.5 else "read_lensmap"
            queue.append(lambda: draw_read(read))
        if st["op"] == "set_lensmap_lod" and rng.random() < 0.35:          # a set plane in front of a bias / switch that changes nothing
            queue.insert(0, lambda: dict(op="set_lod_bias", bias=sh.bias) if rng.random() < 0.5 else dict(op="set_subtexel", on=sh.sub_on))

    # ---- the directed parts: a seed's share of the (event, next launch) pairs and of the scenarios
    def ensure_lensmap():
        if sh.off is None:
            emit(draw_event("set_lensmap"))

    def ensure_sub():
        ensure_lensmap()
        if not sh.sub_on:
            emit(dict(op="set_subtexel", on=True))
        if sh.sub is None:
            emit(draw_event("set_lensmap_subtexel"))

    def ensure_pyramid():
        ensure_sub()
        if sh.mip is None or None in sh.mip["src"]:
            launch("trilinear", mips=True)

    def launch(kind, **force):
        st = draw_launch(kind)
        st.update({"nulls": (), **force})
        if kind == "trilinear" and st["mips"]:
            state["last_nulls"] = st["nulls"]
        emit(st)
        return st

    def observe_lod():
        if rng.random() < 0.5:
            emit(dict(op="read_lod"))
        else:
            launch("trilinear", mips=True if sh.mip is None else bool(rng.random() < 0.5))

    def other_plates():
        src = next((s for s in sh.mip["src"] if s is not None), -1)
        return int(rng.choice([p for p in range(3) if p != src]))

    def do_pair(op, kind):
        """the event, then at once the launch (two steps; four where the stripe has to be made one that takes an ss2 launch first)"""
        if kind == "ss2" and op != "set_rows" and not ss2_allowed(sh.H, sh.r0, sh.r1):
            emit(dict(op="set_rows", rows=(0, sh.H)))
            emit(draw_event("set_lensmap"))
        if op == "set_rows" and sh.H > 2 and sh.r1 - sh.r0 == sh.H:         # (a stripe first: the pair's set_rows moves it and keeps its height)
            r0 = 2 * int(rng.integers(0, (sh.H - 1) // 2))
            emit(dict(op="set_rows", rows=(r0, r0 + (2 if sh.H > 4 else 1))))
            emit(draw_event("set_lensmap"))
        st = draw_event(op, kind)
        emit(st)
        after_event(st)
        emit(draw_launch(kind))

    def do_scenario(v):
        """a few steps after which the shadow that forgets rule v (FORGETFUL) and the true one part; where the frame or the platesize in
        place leaves no room for them, those of rule 16"""
        L = sh.levels()
        if v in (1, 2, 3, 4, 6):                                           # a set plane, the event, then whoever reads the plane
            ensure_sub()
            emit(dict(op="set_lensmap_lod", lod=int(rng.integers(0, 4)), over=False))
            if v == 1:
                emit(draw_event("set_lensmap"))
            elif v == 2:
                emit(draw_event("set_lensmap_subtexel"))
            elif v == 3:
                keys = scan_keys(sh.W, sh.r0, sh.r1)
                emit(dict(op="truncate_build", key=int(keys[int(rng.integers(0, len(keys)))])))
            elif v == 4:                                                   # (... while a seam table waits for its upload)
                emit(draw_event("set_seam_table"))
                emit(dict(op="set_lod_bias", bias=int(rng.choice([b for b in BIASES if b != sh.bias]))))
                launch("seams")
            else:
                emit(dict(op="set_lod_bias", bias=sh.bias) if rng.random() < 0.5 else dict(op="set_subtexel", on=True))
            observe_lod()
        elif v == 7:
            ensure_sub()
            emit(draw_event("set_lensmap_subtexel"))
            emit(draw_event("set_lensmap"))
            if rng.random() < 0.5:
                emit(dict(op="read_subtexel"))
            else:
                launch("bilinear")
        elif v == 8:                                                       # (an unmapped pixel shows in no frame: the read tells)
            ensure_sub()
            emit(draw_event("set_lensmap_subtexel"))
            keys = scan_keys(sh.W, sh.r0, sh.r1)
            emit(dict(op="truncate_build", key=int(keys[int(rng.integers(0, len(keys)))])))
            emit(dict(op="read_subtexel"))
        elif v == 9 and sh.H > 1:
            if sh.r1 - sh.r0 == sh.H:
                emit(dict(op="set_rows", rows=_draw_rows(rng, sh.H, not_height=sh.H)))
            ensure_lensmap()
            h, rows = sh.r1 - sh.r0, (sh.r0, sh.r1)
            while rows == (sh.r0, sh.r1):
                r0 = int(rng.integers(0, sh.H - h + 1))
                rows = (r0, r0 + h)
            emit(dict(op="set_rows", rows=rows))
            if rng.random() < 0.5:
                emit(dict(op="read_lensmap"))
            else:
                launch("nearest")
        elif v == 10 and sh.W != sh.H:
            if sh.r1 - sh.r0 != sh.H:
                emit(dict(op="set_rows", rows=(0, sh.H)))
            ensure_lensmap()
            emit(dict(op="resize", size=(sh.H, sh.W)))
            if rng.random() < 0.5:
                emit(dict(op="read_lensmap"))
            else:
                launch("nearest")
        elif v == 11:                                                      # (first: a second table over one the device already holds)
            ensure_sub()
            first = int(rng.integers(0, 4))
            for seams in (first, (first + 1 + int(rng.integers(0, 3))) % 4):
                emit(dict(op="set_seam_table", seams=seams))
                launch("seams")
            emit(dict(op="resize", size=draw_size("same_ps")))
            emit(dict(op="read_seam_table"))
        elif v in (12, 13):
            ensure_pyramid()
            if v == 13 and state["back"] is None:
                state["back"] = (len(steps) + int(rng.integers(3, 6)), (sh.W, sh.H))
            emit(dict(op="resize", size=draw_size("swap" if v == 12 else "other_ps")))
            emit(draw_read("read_mip_level"))
            if v == 12:                                                    # the kept pyramid, read with mips = 0 through a new table
                emit(draw_event("set_lensmap"))
                launch("trilinear", mips=False, plates=other_plates())
        elif v == 14 and L > 1:                                            # a plate NULL with mips = 1 between two looks at its levels
            ensure_pyramid()
            drop = tuple(sorted(rng.choice(6, int(rng.integers(2, 4)), replace=False).tolist()))
            emit(dict(op="set_lensmap", table=int(rng.integers(0, 4)), drop=drop))
            st = launch("trilinear", mips=True, plates=other_plates(), nulls=tuple(p for p in range(6) if p not in sh.named()))
            for plate in rng.choice(st["nulls"], 2, replace=False).tolist():
                emit(dict(op="read_mip_level", plate=int(plate), level=int(rng.integers(1, L))))
            emit(dict(op="set_lensmap", table=int(rng.integers(0, 4)), drop=()))      # ... and a call that reads the plate again
            launch("trilinear", mips=False)
        elif v == 15 and L > 1:                                            # plates newer than the pyramid, read with mips = 0
            ensure_pyramid()
            emit(dict(op="set_lensmap_lod", lod=int(rng.integers(0, 4)), over=False))
            launch("trilinear", mips=False, plates=other_plates())
        elif v == 16:
            ensure_lensmap()
            fine = [k for k in LAUNCHES if (k != "ss2" or ss2_allowed(sh.H, sh.r0, sh.r1)) and (k in ("nearest", "ss2") or sh.sub is not None)
                    and (k != "seams" or sh.seam is not None)]
            which = int(rng.integers(0, 2))
            # the same array object through two applies, its bytes changed in between: a bilinear and a trilinear call wherever there is
            # a sub-texel plane, two kinds the state takes where there is none
            kinds = ("bilinear", "trilinear") if sh.sub is not None else (str(rng.choice(fine)), str(rng.choice(fine)))
            for j, kind in enumerate(kinds):
                launch(kind, lut=which, **(dict(mips=True) if kind == "trilinear" else {}))
                if j == 0:
                    emit(dict(op="lut_in_place", lut=which, bytes=int(rng.integers(2, 40))))
        elif v == 17:                                                      # a refused call, then a look at what it would have changed
            ensure_sub()
            if rng.random() < 0.5 or not sh.named():
                emit(dict(op="set_lensmap_lod", lod=int(rng.integers(0, 4)), over=True))
                emit(dict(op="read_lod"))
            else:
                launch("trilinear", mips=True, plates=int(rng.integers(0, 3)) if sh.mip is None else other_plates(),
                       nulls=(int(rng.choice(sorted(sh.named()))),))
                emit(draw_read("read_mip_level"))
        else:                                                              # (a frame of one row, a square one, a pyramid of one level)
            do_scenario(16)

    def random_step():
        if state["back"] is not None and len(steps) >= state["back"][0]:
            size, state["back"] = state["back"][1], None
            emit(dict(op="resize", size=size))
            return
        if queue:
            emit(queue.pop(0)())
            return
        u = rng.random()
        if sh.off is None:                                                 # mostly mended at once: a context without a lensmap refuses everything
            what = "set_lensmap" if u < 0.8 else "launch" if u < 0.86 else "read" if u < 0.92 else "event"
        elif sh.sub is None and u < 0.8:
            what = "set_lensmap_subtexel" if sh.sub_on else "set_subtexel"
        elif sh.sub is not None and (sh.sub == CENTRE).all() and u < 0.2:
            what = "set_lensmap_subtexel"
        elif sh.seam is None and u < 0.6:
            what = "set_seam_table"
        else:
            u = rng.random()
            what = "launch" if u < 0.78 else "event" if u < 0.93 else "read"
        if what == "launch":
            emit(draw_launch())
        elif what == "read":
            emit(draw_read())
        else:
            op = what if what != "event" else str(rng.choice(EVENTS, p=[0.08, 0.1, 0.12, 0.12, 0.1, 0.08, 0.11, 0.11, 0.1, 0.08]))
            st = dict(op=op, on=True) if what == "set_subtexel" else draw_event(op)
            emit(st)
            after_event(st)

    n = int(rng.integers(13, MAX_STEPS + 1))
    plan = [("pair", PAIRS[(2 * seed) % len(PAIRS)]), ("scenario", SCENARIOS[seed % len(SCENARIOS)]), ("pair", PAIRS[(2 * seed + 1) % len(PAIRS)])]
    try:
        for _ in range(int(rng.integers(0, 3))):
            random_step()
        for what, arg in plan:
            if what == "pair":
                do_pair(*arg)
            else:
                do_scenario(arg)
            for _ in range(int(rng.integers(1, 3))):
                random_step()
        while len(steps) < n:
            random_step()
    except _Full:
        pass
    assert 10 <= len(steps) <= 16, len(steps)
    return dict(seed=seed, cls=cls, W=W, H=H, ps=min(W, H), r0=rows[0], r1=rows[1], sub_on=sub_on, slots=slots, steps=steps)


def shadow_of(seq, **kw):
    return Shadow(seq["W"], seq["H"], (seq["r0"], seq["r1"]), seq["sub_on"], **kw)


def walk(seq, **kw):
    """plays a sequence on a Shadow(**kw): yields (i, step, before, outcome, shadow) - `before` is what the step met: the geometry, the
    levels of the platesize, the plates the lensmap names, the scalars and the kind of every piece of state"""
    sh = shadow_of(seq, **kw)
    for i, st in enumerate(seq["steps"]):
        before = dict(W=sh.W, H=sh.H, ps=sh.ps, r0=sh.r0, r1=sh.r1, L=sh.levels(), named=sh.named(), bias=sh.bias, sub_on=sh.sub_on,
                      lod=sh.lod[0], src=None if sh.mip is None else list(sh.mip["src"]), kinds=sh.kinds())
        yield i, st, before, sh.apply(st), sh


def digest(seq):
    """SHA-256 over the sequence as canonical JSON (it is plain data)"""
    return hashlib.sha256(json.dumps(seq, sort_keys=True).encode()).hexdigest()


def _words(st):
    return st["op"] + "(" + ", ".join(f"{k}={v}" for k, v in st.items() if k != "op" and v is not None and v != ()) + ")"


def describe(seq, i=None):
    """the seed, the context and steps 0..i (all of them without i) in words, for failure messages"""
    s = (f"seed {seq['seed']} ({seq['cls']}): {seq['W']}x{seq['H']} ps {seq['ps']} rows [{seq['r0']},{seq['r1']}) sub-texel switch "
         f"{'on' if seq['sub_on'] else 'off'} ring {seq['slots']}")
    last = len(seq["steps"]) - 1 if i is None else i
    return s + "".join(f"\n  {j:2d} {_words(st)}" for j, st in enumerate(seq["steps"][:last + 1]))
