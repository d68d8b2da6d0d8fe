"""The frame-buffer campaign (tests/fbgen.py, tests/test_apply_rgba_fb_campaign_gpu.py), as far as it can be checked without a GPU.

(a) Determinism: sequence(seed) twice is the same data; the first and the last committed seed have pinned digests.
(b) A second statement of the shadow: TRANSITIONS, one row per event / launch / read (split where the arguments decide: the same bias or a
    new one ...), one column per piece of state, each cell keep / drop / make; MUST_REFUSE, the state each call cannot do without.  A walk
    of more than 2000 generated steps (seeds outside the committed range, state kinds only, no arrays) holds Shadow to both.
(c) The expectation against the loop twins: for three small committed seeds every frame and every read through the vectorised models
    equals the one through bilinear_frame_loops / seam_frame_loops / trilinear_frame_loops / derive_lod_loops / pyramid_loops.
    rgba_fb_model.fb_frame has no loop twin: the nearest frame is held to the bilinear loops with a plane of centres, the ss2 frame to
    the CPU oracle's samples averaged by tests/test_apply_rgba_ss2_gpu.py's quad_means.
(d) Forgetful shadows: Shadow with one rule removed (fbgen.FORGETFUL) must answer differently from the true one - another outcome, or
    one different byte - on at least 3 steps of the committed seeds, in at least 2 seeds.  Measured on COMMITTED (steps / seeds):
        1 lod kept by set_lensmap 6 / 5; 2 by set_lensmap_subtexel 12 / 8; 3 by truncate_build 3 / 3; 4 by a real bias change 5 / 2;
        6 a set lod dropped by a same-value bias or switch 5 / 4; 7 sub not recentred by set_lensmap 11 / 4; 8 nor where truncate_build NULLs
        3 / 3; 9 lensmap survives a same-height set_rows 16 / 9; 10 a same-pixel-count resize 6 / 3; 11 seam table survives a resize 3 / 3;
        12 pyramid dropped by a same-platesize resize 8 / 4; 13 survives a platesize change 3 / 3; 14 a NULL plate's levels zeroed 5 / 2;
        15 mips = 0 shows this call's plates 11 / 10; 16 a LUT changed in place not seen 9 / 4; 17 a refused call changes state 5 / 4.
        COMMITTED is range(48), the smallest range from 0 that meets every condition of this file (up to 47 seeds the message "above"
        occurs once; rules 13 and 14 need seeds 43 and 44).
    Rule 5 CANNOT be told apart by any sequence of these calls, which the test states instead of a count: a real change of the switch
    leaves the context without a sub-texel plane (switching off frees it, switching on conjures none), every reader of the
    level-of-detail plane is refused without one, and the two calls that bring a plane back - bk_set_lensmap and
    bk_set_lensmap_subtexel - each drop the level-of-detail plane themselves.  The rule is redundant as the header stands.
(e) The census over the committed seeds: what their steps reach, read off the generator's output and the true shadow alone.  Measured:
        48 seeds, 708 steps, none left out.  Launches ok / refused: nearest 32 / 16, ss2 28 / 8, bilinear 37 / 11, seams 34 / 17, trilinear
        61 / 16; all 50 (event, next launch) pairs, the launch the step right behind the event.  Refusals: "no lensmap" 59, "no valid globe"
        12, "is NULL, but the lensmap reads" 13, "sub-texel plane" 7, "no pyramid" 6, "mips = 0" 3, "above" 2.  Trilinear at L = 1: 6 calls,
        2: 8, 3: 3, 4: 5, 5: 12, 6: 6, 7: 9, 9: 12 (39 of 61 at L >= 5).  W % 4 != 0 in 42 contexts, successful launches on a one-row
        stripe in 9, all six layouts, all three alignment classes, 11 successful mips = 0 calls that read a level at or above 1 made from
        other plates than their level 0 (older_levels below), 62 derived planes, 43 of them with a level at or above 1.
No seed and no step is filtered or skipped anywhere: every count runs over every step of every committed seed."""
import collections

import numpy as np
import pytest

import fbgen as G
from rgbagen import align_class

K, D, M, S = "keep", "drop", "make", "make if the switch is on, else drop"
PIECES = ("lensmap", "sub", "lod", "seam", "pyramid")
KEEP = (K,) * 5
#                                   lensmap sub lod seam pyramid
TRANSITIONS = {
    "set_lensmap":                  (M, S, D, K, K),
    "set_lensmap_subtexel":         (K, M, D, K, K),
    "set_lensmap_lod":              (K, K, M, K, K),
    "set_lod_bias/same":            KEEP,
    "set_lod_bias/new":             (K, K, D, K, K),
    "set_subtexel/same":            KEEP,
    "set_subtexel/on":              (K, K, D, K, K),      # (no plane is conjured: the sub piece stays "none")
    "set_subtexel/off":             (K, D, D, K, K),
    "set_seam_table":               (K, K, K, M, K),
    "set_rows/same":                KEEP,
    "set_rows/moved":               (D, D, D, K, K),      # (a stripe of the same height too)
    "resize/same":                  KEEP,
    "resize/same platesize":        (D, D, D, D, K),      # (the same pixel count too)
    "resize/other platesize":       (D, D, D, D, D),
    "truncate_build/0":             KEEP,
    "truncate_build/key":           (K, K, D, K, K),
    "lut_in_place":                 KEEP,
    "nearest": KEEP, "ss2": KEEP, "bilinear": KEEP, "seams": KEEP,
    "trilinear/mips 0":             KEEP,
    "trilinear/mips 1":             (K, K, K, K, M),
    "read_lod": KEEP, "read_subtexel": KEEP, "read_seam_table": KEEP, "read_mip_level": KEEP, "read_lensmap": KEEP,
}
# the pieces a call is refused without
MUST_REFUSE = {
    "set_lensmap_subtexel": ("lensmap",), "set_lensmap_lod": ("lensmap", "sub"), "truncate_build/0": ("lensmap",), "truncate_build/key": ("lensmap",),
    "nearest": ("lensmap",), "ss2": ("lensmap",), "bilinear": ("lensmap", "sub"), "seams": ("lensmap", "sub", "seam"),
    "trilinear/mips 0": ("lensmap", "sub", "pyramid"), "trilinear/mips 1": ("lensmap", "sub"),
    "read_lod": ("lensmap", "sub"), "read_subtexel": ("lensmap", "sub"), "read_seam_table": ("seam",), "read_mip_level": ("pyramid",),
    "read_lensmap": ("lensmap",),
}
MODEL_SEEDS = (13, 26, 29)          # 2 x 3, 33 x 5 and 130 x 10: the loop twins run in seconds
DIGESTS = {0: "b284170015a44c93871cbdd1eea6a9baec50ae8ec947a8d6b5a9aa75a71e84e5", 47: "254ee55b655f19d68f44d9ff338c4571bff9449faad9dd03bf34bcf37952ee1c"}
FLOORS = dict(launch_ok=20, launch_refused=3, message=2, stale_mips0=3, one_row=2)


def case_of(st, before):
    """the row of TRANSITIONS a step belongs to, from its arguments and the scalars it met"""
    op = st["op"]
    if op == "launch":
        return st["kind"] if st["kind"] != "trilinear" else "trilinear/mips %d" % st["mips"]
    if op == "set_lod_bias":
        return op + ("/same" if st["bias"] == before["bias"] else "/new")
    if op == "set_subtexel":
        return op + ("/same" if st["on"] == before["sub_on"] else "/on" if st["on"] else "/off")
    if op == "set_rows":
        return op + ("/same" if tuple(st["rows"]) == (before["r0"], before["r1"]) else "/moved")
    if op == "resize":
        W, H = st["size"]
        return op + ("/same" if (W, H) == (before["W"], before["H"]) else "/same platesize" if min(W, H) == before["ps"] else "/other platesize")
    if op == "truncate_build":
        return op + ("/0" if st["key"] == 0 else "/key")
    return op


def after_of(case, kinds, sub_on):
    made = dict(lensmap="there", sub="there", lod="set", seam="there", pyramid="there")
    dropped = dict(lensmap="none", sub="none", lod="derive", seam="none", pyramid="none")
    out = {}
    for piece, cell in zip(PIECES, TRANSITIONS[case]):
        if cell == S:
            cell = M if sub_on else D
        out[piece] = kinds[piece] if cell == K else made[piece] if cell == M else dropped[piece]
    return out


@pytest.fixture(scope="module")
def runs():
    """every committed sequence played once on the true shadow: [(seq, [(i, step, before, outcome)], derived planes)]; `before` of a
    successful trilinear call with mips = 0 also says whether it read levels older than its level 0 (older_levels)"""
    out = []
    for seed in G.COMMITTED:
        seq = G.sequence(seed)
        played, planes = [], []
        for i, st, before, outcome, sh in G.walk(seq):
            if st["op"] == "launch" and st["kind"] == "trilinear" and not st["mips"] and outcome[0] == "ok":
                before["older_levels"] = older_levels(st, before, sh)
            played.append((i, st, before, outcome))
            if before["lod"] == "derive" and sh.lod[0] == "derived":
                planes.append(sh.lod[1])
        out.append((seq, played, planes))
    return out


def older_levels(st, before, sh):
    """a successful mips = 0 call read a level at or above 1 that was made from OTHER plates than its level 0: the pyramid has such a
    level (L >= 2), and on some plate whose levels were made (src not None) from another set of plates a mapped pixel of the owned rows has
    a plane value above 0 - its upper level, at or above 1, then has a weight"""
    if before["L"] < 2:
        return False
    mapped = sh.off != G.NULL
    plate = np.where(mapped, sh.off, 0).astype(np.int64) // (sh.ps * sh.ps)
    return any(before["src"][p] is not None and before["src"][p] != st["plates"] and bool((np.asarray(sh.lod[1])[mapped & (plate == p)] > 0).any())
               for p in before["named"])


def same(a, b):
    """two outcomes are the same: the same kind, code and message, or equal arrays"""
    if a[0] != b[0]:
        return False
    if a[0] == "refused":
        return a[1:] == b[1:]
    x, y = a[1], b[1]
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, tuple):
        return all(np.array_equal(p, q) for p, q in zip(x, y))
    return np.array_equal(x, y)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
def test_sequences_are_deterministic_and_pinned():
    assert list(G.COMMITTED) == list(range(G.COMMITTED[0], G.COMMITTED[-1] + 1))
    assert sorted(DIGESTS) == [G.COMMITTED[0], G.COMMITTED[-1]]
    for seed in G.COMMITTED:
        a, b = G.sequence(seed), G.sequence(seed)
        assert a == b and G.digest(a) == G.digest(b), seed
        assert 10 <= len(a["steps"]) <= 16 and max(a["W"], a["H"]) <= 264
    for seed, want in DIGESTS.items():
        assert G.digest(G.sequence(seed)) == want, f"seed {seed} has moved"


def test_describe_prints_the_steps_up_to_the_one_named():
    seq = G.sequence(G.COMMITTED[0])
    text = G.describe(seq, 3)
    assert f"seed {seq['seed']}" in text and len(text.splitlines()) == 5 and seq["steps"][3]["op"] in text.splitlines()[-1]


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
def test_the_shadow_follows_the_transition_table_on_a_long_walk():
    steps, seen, seed = 0, collections.Counter(), 1000
    while steps < 2000 or set(TRANSITIONS) - set(seen):
        assert seed < 1400, f"rows never reached: {sorted(set(TRANSITIONS) - set(seen))}"
        for i, st, before, outcome, sh in G.walk(G.sequence(seed), frames=False):
            case = case_of(st, before)
            missing = [p for p in MUST_REFUSE.get(case, ()) if before["kinds"][p] == "none"]
            if missing:
                assert outcome[0] == "refused", f"seed {seed} step {i} {case}: accepted without {missing}"
            want = after_of(case, before["kinds"], before["sub_on"]) if outcome[0] == "ok" else before["kinds"]
            assert sh.kinds() == want, f"seed {seed} step {i} {case} ({outcome[0]}): {before['kinds']} -> {sh.kinds()}, the table says {want}"
            if outcome[0] == "ok":
                seen[case] += 1
            steps += 1
        seed += 1
    assert steps >= 2000 and min(seen.values()) >= 1


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_every_expectation_equals_the_loop_twins(seed):
    seq = G.sequence(seed)
    assert seed in G.COMMITTED and seq["W"] * seq["H"] <= 1400
    frames = 0
    for (i, st, _, a, _), (_, _, _, b, _) in zip(G.walk(seq), G.walk(seq, models=G.Loops)):
        assert same(a, b), f"{G.describe(seq, i)}\nthe vectorised models and the loops differ"
        frames += a[0] == "ok" and st["op"] == "launch"
    assert frames >= 3


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------
def differences(runs, rule):
    """{seed: steps on which the shadow without `rule` answers differently from the true one}"""
    out = {}
    for seq, played, _ in runs:
        n = sum(not same(outcome, played[i][3]) for i, _, _, outcome, _ in G.walk(seq, forget=(rule,)))
        if n:
            out[seq["seed"]] = n
    return out


@pytest.mark.parametrize("rule", [r for r in G.FORGETFUL if r != 5])
def test_a_forgetful_shadow_is_told_apart(runs, rule):
    d = differences(runs, rule)
    print(f"{rule:2d}. {G.FORGETFUL[rule]}: {sum(d.values())} / {len(d)}")
    assert sum(d.values()) >= 3 and len(d) >= 2, f"rule {rule} ({G.FORGETFUL[rule]}): differs on {d}"


def test_the_switch_rule_is_redundant(runs):
    """rule 5 (see the docstring): no step tells the shadow without it from the true one, here or on the long walk's seeds"""
    assert differences(runs, 5) == {}
    for seed in range(1000, 1040):
        seq = G.sequence(seed)
        if seq["ps"] <= 17:
            assert all(same(a, b) for (_, _, _, a, _), (_, _, _, b, _) in zip(G.walk(seq), G.walk(seq, forget=(5,)))), seed


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------
def test_census(runs):
    pairs, ok, refused, messages, layouts, classes = set(), collections.Counter(), collections.Counter(), collections.Counter(), set(), set()
    tri_levels, stale, one_row, derived = [], 0, set(), [bool((p >= 256).any()) for _, _, planes in runs for p in planes]
    steps = 0
    for seq, played, _ in runs:
        for i, st, before, outcome in played:
            steps += 1
            if outcome[0] == "refused":
                messages[outcome[2]] += 1
            if st["op"] != "launch":
                continue
            if i and seq["steps"][i - 1]["op"] in G.EVENTS:
                pairs.add((seq["steps"][i - 1]["op"], st["kind"]))
            (ok if outcome[0] == "ok" else refused)[st["kind"]] += 1
            if outcome[0] != "ok":
                continue
            layouts.add(st["layout"])
            d = G.dest_of(before["W"], before["H"], st)
            classes.add(align_class(G.first_byte(st, d, before["r0"]), d["pitch"], 0))
            if before["r1"] - before["r0"] == 1 and before["H"] > 1:
                one_row.add(seq["seed"])
            if st["kind"] == "trilinear":
                tri_levels.append(before["L"])
                stale += before.get("older_levels", False)
    assert steps == sum(len(seq["steps"]) for seq, _, _ in runs)          # nothing left out
    contexts = [seq for seq, _, _ in runs]
    print(f"{len(contexts)} seeds, {steps} steps; launches ok {dict(ok)} refused {dict(refused)}; messages {dict(messages)}; pairs {len(pairs)} of "
          f"{len(G.PAIRS)}; trilinear at L {dict(collections.Counter(tri_levels))}; W % 4 != 0 in {sum(s['W'] % 4 != 0 for s in contexts)} contexts; "
          f"one-row stripes in {len(one_row)}; mips = 0 over older levels {stale}; derived planes {len(derived)}, {sum(derived)} with a level >= 1")
    assert pairs == set(G.PAIRS), f"missing {sorted(set(G.PAIRS) - pairs)}"
    for kind in G.LAUNCHES:
        assert ok[kind] >= FLOORS["launch_ok"] and refused[kind] >= FLOORS["launch_refused"], (kind, ok[kind], refused[kind])
    for m in G.MESSAGES:
        assert messages[m] >= FLOORS["message"], (m, messages[m])
    assert {1, 2, 3} <= set(tri_levels) and 2 * sum(L >= 5 for L in tri_levels) >= len(tri_levels)
    assert 3 * sum(s["W"] % 4 != 0 for s in contexts) >= len(contexts)
    assert len(one_row) >= FLOORS["one_row"]
    assert layouts == set(G.FB.LAYOUTS) and classes == set(G.FB.G.ALIGN_CLASSES)
    assert stale >= FLOORS["stale_mips0"]
    assert 3 * sum(derived) >= len(derived) > 0
    assert any(s["W"] < 4 for s in contexts) and any(s["ps"] >= 129 and s["ps"] % 4 for s in contexts) and any(5 <= s["ps"] <= 64 for s in contexts)
    assert {s["slots"] for s in contexts} == {1, 4} and {s["sub_on"] for s in contexts} == {True, False}
