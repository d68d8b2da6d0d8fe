"""The truecolour apply campaign (tests/rgbagen.py, tests/test_apply_rgba_campaign_gpu.py), as far as it can be checked without a GPU.

(a) The expectation is right.  The GPU campaign compares against rgbagen.expected, which asks the oracle's 8-bit apply for every byte plane.
For a few seeds the same allocations are computed a second way with no oracle call - the four planes interleaved into 32-bit texels, gathered
with the raw offsets, lut[c][tint] where tint < 6, NULL pixels and the rows outside the stripe left alone - and must be equal byte for byte.

(b) The census.  What the committed seeds reach, read off the generator's output alone: a precondition on the campaign's INPUTS, never a
filter on its results.  A generator or seed-range change that empties a line fails here and says which.

(c) The second family (rgbagen.sequence_ss2: the 2x2 supersampling apply among full-size launches) the same way: its census, and a model of
an ss2 frame that shares neither the oracle nor the averaging code with the expectation.

(d) The first family has not moved: a digest of its committed sequences, computed before the second was written."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import rgbagen as G

HERE = os.path.dirname(os.path.abspath(__file__))

# line -> how many committed seeds must reach it
CENSUS = {
    "W<4": 2,
    "W<128,W%4!=0": 2,
    "W>128,W%128 in 1..3": 2,
    "H<block height, RG 1": 2,
    "H<block height, RG 2": 2,
    "H<block height, RG 4": 2,
    "ps<16": 2,
    "ps<8": 2,
    "one-row stripe": 2,
    "two-row stripe": 1,
    "stripe r0%8!=0": 2,
    "R%4!=0": 8,                              # (a third of the seeds, and no fewer than 6)
    "globe0>=G": 2,
    "1 frame": 2,
    "2..4 frames": 2,
    ">=5 frames, plain": 2,
    ">=5 frames, tinted": 2,
    "tuning on, consecutive launches change kind": 4,
    "tuning on, no forced height: a block map of one flavour meets another kind": 4,
    "... on a stripe of at least 256 x 64 pixels": 2,
    "tinted, RG 4, 64 KiB: a block above 1280 chunks": 2,
    "staging buffer < a block's list, plain": 2,
    "staging buffer < a block's list, tinted": 2,
    "tinted: a chunk under >=3 classes": 2,
    "fully mapped, W%4==0, 16-byte aligned": 2,
    "fully mapped, W%4==0, not 16-byte aligned": 2,
    "BK_AB_ROW_MAJOR": 2,
    "tuning off": 2,
    "event set_lensmap": 2,
    "event mutate_lut": 2,
    "upload host": 2,
    "upload device": 2,
    "device upload pitch%16!=0": 2,
    "device upload pitch%4!=0": 2,
    "apply8 between truecolour launches": 2,
}
MODEL_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
# SHA-256 over sequence(s) for s in COMMITTED as `_digest` serialises it, computed on the commit BEFORE the ss2 family was added to
# rgbagen.py: the first family's draws - and with them its census, its mutant record and profiles/rgba_campaign.txt - have not moved
FIRST_FAMILY_SHA256 = "fdf8c51390c25e065f7f5d3973abddefbe51d6017587a44a77cc18e94d980492"


def _digest(values):
    """SHA-256 over a canonical serialisation: every value behind a type tag, dicts by sorted key, arrays as dtype, shape and bytes"""
    h = hashlib.sha256()

    def put(x):
        if isinstance(x, np.ndarray):
            h.update(f"A{x.dtype.str}{x.shape}".encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, dict):
            h.update(f"D{len(x)}".encode())
            for k in sorted(x):
                put(k)
                put(x[k])
        elif isinstance(x, (list, tuple)):
            h.update(f"L{len(x)}".encode())
            for v in x:
                put(v)
        elif isinstance(x, (bool, np.bool_)):
            h.update(b"b1" if x else b"b0")
        elif isinstance(x, (int, np.integer)):
            h.update(f"i{int(x)};".encode())
        elif isinstance(x, str):
            h.update(f"s{len(x)}:{x}".encode())
        else:
            raise TypeError(f"no canonical form for {type(x)}")

    put(values)
    return h.hexdigest()


def test_the_first_family_of_sequences_has_not_moved():
    """the sequences the first campaign committed, bit for bit: the ss2 family was added BESIDE them (its own base seed, its own draws)"""
    assert _digest([G.sequence(s) for s in G.COMMITTED]) == FIRST_FAMILY_SHA256


def test_generator_loads_without_the_library_and_reads_the_bit_from_the_source():
    """loading rgbagen imports neither blinky_amd nor torch (the census and the model check run from the generator alone, on a tree whose
    library is not built yet), and the ablation bit it draws is one bit of the enum the launchers compile"""
    code = "import sys, rgbagen; print(rgbagen.AB_ROW_MAJOR, any(m == 'torch' or m.startswith('blinky_amd') for m in sys.modules))"
    out = subprocess.run([sys.executable, "-c", code], cwd=HERE, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(G.AB_ROW_MAJOR), "False"], out
    assert G.AB_ROW_MAJOR > 0 and G.AB_ROW_MAJOR & (G.AB_ROW_MAJOR - 1) == 0
    assert G.ablation_bit("BK_AB_ROW_MAJOR") != G.ablation_bit("BK_AB_PERSISTENT")


def test_committed_seeds_are_contiguous():
    assert list(G.COMMITTED) == list(range(G.COMMITTED[0], G.COMMITTED[-1] + 1)) and len(G.COMMITTED) == 24


def test_generator_draws_what_the_issue_lists():
    """shape of the data over the committed seeds: 4-7 launches, ring 4..14, the three frame strides, both pointer offsets, the upload
    pitches, a stripe in about a third of the seeds"""
    seqs = [G.sequence(s) for s in G.COMMITTED]
    assert all(4 <= len(q["launches"]) <= 7 for q in seqs)
    assert all(4 <= q["R"] <= 14 and q["G"] == q["R"] // 4 and q["ps"] == min(q["W"], q["H"]) for q in seqs)
    assert all(0 <= q["r0"] < q["r1"] <= q["H"] for q in seqs)
    stripes = sum((q["r0"], q["r1"]) != (0, q["H"]) for q in seqs)
    assert len(seqs) // 6 <= stripes <= len(seqs) // 2, stripes
    L = [(q, l) for q in seqs for l in q["launches"]]
    extras = {(l["stride"] - l["frame_h"] * l["pitch"]) % 16 if l["stride"] != l["frame_h"] * l["pitch"] else -1 for _, l in L}
    assert extras == {-1, 0, 4}, extras
    assert {l["ptr_off"] for _, l in L} == {0, 4}
    assert all(l["pitch"] % 4 == 0 and l["stride"] % 4 == 0 for _, l in L if l["kind"] != "apply8")
    assert all(0 <= l["first"] <= 2 * q["G"] + 1 for q, l in L if l["kind"] != "apply8")
    assert {u["extra"] for q in seqs for u in q["uploads"] if u["path"] == "device"} == set(G.UPLOAD_PITCH_EXTRA)
    assert {q["shape"] for q in seqs} == {0, 1, 2, 4} and {q["ldskb"] for q in seqs} <= set(G.STAGING_KB)
    for q in seqs:                                                    # the in-place LUT change sits between two tinted launches of one array
        if q["event"]["kind"] == "mutate_lut":
            a, b = q["launches"][q["event"]["at"] - 1], q["launches"][q["event"]["at"]]
            assert a["kind"] == b["kind"] == "rgba_tinted" and a["lut"] == b["lut"] == 0


def test_census_of_the_committed_seeds():
    reached = {line: [] for line in CENSUS}
    for seed in G.COMMITTED:
        for line in G.features(G.sequence(seed)):
            assert line in reached, f"rgbagen.features names a line the census does not know: {line}"
            reached[line].append(seed)
    short = {line: (seeds, CENSUS[line]) for line, seeds in reached.items() if len(seeds) < CENSUS[line]}
    assert not short, "census lines the committed seeds do not reach (line: (seeds that do, seeds wanted)): " + repr(short)


@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_oracle_expectation_equals_the_numpy_model(seed):
    seq = G.sequence(seed)
    pal = G.palette(seq)
    globes = {}

    def slots(s):
        if s not in globes:
            globes[s] = G.slot_globe(seq, s)
        return globes[s]

    flavours = set()
    for i, L, off, tints, lut, ev in G.walk(seq):
        want = G.expected(seq, L, off, tints, lut, pal, slots)
        # the model's own placement, written out here: frame f comes from globe (first + f) mod the truecolour globes (8-bit: ring slot,
        # mod the ring), and starts ptr_off + f * stride bytes into an allocation that ends with the last frame's stride
        ring = seq["R"] if L["kind"] == "apply8" else seq["R"] // 4
        size = L["frame_h"] * L["pitch"]
        model = np.full(L["ptr_off"] + L["nframes"] * L["stride"], G.FILL, np.uint8)
        for f in range(L["nframes"]):
            frame = np.full((L["frame_h"], L["pitch"]), G.FILL, np.uint8)
            G.numpy_frame(seq, L, off, tints, lut, pal, slots, (L["first"] + f) % ring, frame)
            model[L["ptr_off"] + f * L["stride"]:L["ptr_off"] + f * L["stride"] + size] = frame.ravel()
        assert want.shape == model.shape, G.describe(seq, i)
        if not np.array_equal(want, model):
            at = int(np.flatnonzero(want != model)[0])
            raise AssertionError(f"{G.describe(seq, i)}: the oracle's expectation and the numpy model differ at byte {at}: {want[at]} / {model[at]}")
        flavours.add(L["kind"])
    assert flavours, seed


def test_model_seeds_hold_both_flavours_a_stripe_and_both_events():
    seqs = [G.sequence(s) for s in MODEL_SEEDS]
    kinds = {l["kind"] for q in seqs for l in q["launches"]}
    assert kinds == {"rgba", "rgba_tinted", "apply8"}, kinds
    assert any((q["r0"], q["r1"]) != (0, q["H"]) for q in seqs)
    assert {q["event"]["kind"] for q in seqs} == {"set_lensmap", "mutate_lut"}


# ---- the second family: bk_apply_rgba_ss2_device among full-size launches (rgbagen.sequence_ss2) ---------------------------------------------
# line -> how many of the committed ss2 seeds must reach it
CENSUS_SS2 = {
    "W odd": 2,
    "H odd": 2,
    "W<4": 2,
    "W=H=1": 1,
    "W>128,W%128 in 1..3": 2,
    "H<block height, RG 1": 2,
    "H<block height, RG 2": 2,
    "H<block height, RG 4": 2,
    "two-row stripe": 2,
    "stripe r0%8!=0": 2,
    "lone last row of an odd H": 1,
    "R%4!=0": 8,
    "globe0>=G": 2,
    "ss2 of 1 frame": 2,
    "ss2 of 2..4 frames": 2,
    "ss2 of >=5 frames, plain": 2,
    "ss2 of >=5 frames, tinted": 2,
    "ss2: quads of every count 0..4 in the stripe": 2,
    "ss2: n=3, the hole at (0,0)": 2,
    "ss2: n=3, the hole at (0,1)": 2,
    "ss2: n=3, the hole at (1,0)": 2,
    "ss2: n=3, the hole at (1,1)": 2,
    "ss2 of >=2 frames: staging buffer < a block's list, plain": 2,
    "ss2 of >=2 frames: staging buffer < a block's list, tinted": 2,
    "ss2_tinted, RG 4, 64 KiB: a block above 1280 chunks": 2,
    "ss2_tinted: a chunk under >=3 classes": 2,
    # (every block of these launches is staged: the wide stores are what runs - 8 bytes aligned do for RG 1 / 2, RG 4 needs 16.
    #  One seed per line: two would be six seeds of one focus with the three heights in balance, beside everything else 24 seeds hold;
    #  profiles/rgba_ss2_campaign.txt has what the committed seeds reach - RG 2 three, RG 4 two, RG 1 one)
    "fully mapped, W%4==0, staged, RG 1, 16": 1,
    "fully mapped, W%4==0, staged, RG 1, 8-only": 1,
    "fully mapped, W%4==0, staged, RG 1, 4-only": 1,
    "fully mapped, W%4==0, staged, RG 2, 16": 1,
    "fully mapped, W%4==0, staged, RG 2, 8-only": 1,
    "fully mapped, W%4==0, staged, RG 2, 4-only": 1,
    "fully mapped, W%4==0, staged, RG 4, 16": 1,
    "fully mapped, W%4==0, staged, RG 4, 8-only": 1,
    "fully mapped, W%4==0, staged, RG 4, 4-only": 1,
    "ss2 directly after a full-size launch of its flavour": 2,
    "full-size directly after an ss2 launch of its flavour": 2,
    "tuning on, no forced height: an ss2 launch meets a block map of its flavour filed under another kind": 2,
    "tuning off": 2,
    "BK_AB_ROW_MAJOR": 2,
    "event set_lensmap": 2,
    "event mutate_lut": 2,
    "upload host": 2,
    "upload device": 2,
    "device upload pitch%16!=0": 2,
    "device upload pitch%4!=0": 2,
    "apply8 between two ss2 launches": 2,
}


def test_committed_ss2_seeds_are_contiguous_and_drawn_from_their_own_base():
    assert list(G.COMMITTED_SS2) == list(range(24)) and G.BASE_SEED_SS2 != G.BASE_SEED
    assert not set(range(G.BASE_SEED, G.BASE_SEED + 24)) & set(range(G.BASE_SEED_SS2, G.BASE_SEED_SS2 + 24))


def test_ss2_generator_draws_what_the_issue_lists():
    """shape of the data over the committed ss2 seeds: 4-7 launches of five kinds, at least half of them ss2; stripes the entry point accepts;
    half-size destinations at pitch Wo + 0..8, pointer offsets 0 / 4 / 8, the four frame strides; the events in front of ss2 launches"""
    seqs = [G.sequence_ss2(s) for s in G.COMMITTED_SS2]
    assert {l["kind"] for q in seqs for l in q["launches"]} == {"ss2", "ss2_tinted", "rgba", "rgba_tinted", "apply8"}
    for q in seqs:
        W, H, r0, r1, L = q["W"], q["H"], q["r0"], q["r1"], q["launches"]
        Wo, Ho = (W + 1) // 2, (H + 1) // 2
        assert 4 <= len(L) <= 7 and 2 * sum(l["kind"] in G.SS2_KINDS for l in L) >= len(L), G.describe(q)
        assert 4 <= q["R"] <= 14 and q["G"] == q["R"] // 4 and q["ps"] == min(W, H)
        assert 0 <= r0 < r1 <= H and r0 % 2 == 0 and (r1 % 2 == 0 or r1 == H), G.describe(q)
        for l in L:
            if l["kind"] in G.SS2_KINDS:
                assert l["pitch"] % 4 == 0 and Wo <= l["pitch"] // 4 <= Wo + 8 and 0 <= l["x0"] <= l["pitch"] // 4 - Wo and 0 <= l["y0"] <= 3
                assert l["frame_h"] == l["y0"] + Ho + G.ROWS_BELOW and l["ptr_off"] in (0, 4, 8) and l["stride"] >= l["frame_h"] * l["pitch"]
                assert l["stride"] % 4 == 0 and 0 <= l["first"] <= 2 * q["G"] + 1 and 1 <= l["nframes"] <= 7
                assert l["rubix"] == (l["kind"] == "ss2_tinted")
        at = q["event"]["at"]
        if q["event"]["kind"] == "mutate_lut":
            assert L[at - 1]["kind"] == L[at]["kind"] == "ss2_tinted" and L[at - 1]["lut"] == L[at]["lut"] == 0
        else:
            assert L[at]["kind"] in G.SS2_KINDS and len(q["tables"]) == 2
        if q["focus"] == "direct":                                    # the direct gather's frame loop, its ring arithmetic included
            assert q["G"] >= 2 and q["shape"] in (1, 2, 4) and q["ldskb"] in (1, 4)
            assert {l["kind"] for l in L if l["kind"] in G.SS2_KINDS} == set(G.SS2_KINDS)
            assert all(l["nframes"] >= 2 for l in L if l["kind"] in G.SS2_KINDS)
    ss = [l for q in seqs for l in q["launches"] if l["kind"] in G.SS2_KINDS]
    assert {l["ptr_off"] for l in ss} == {0, 4, 8}
    extras = {(l["stride"] - l["frame_h"] * l["pitch"]) % 16 if l["stride"] != l["frame_h"] * l["pitch"] else -1 for l in ss}
    assert extras == {-1, 0, 4, 8}, extras


def test_census_of_the_committed_ss2_seeds():
    reached = {line: [] for line in CENSUS_SS2}
    for seed in G.COMMITTED_SS2:
        for line in G.features_ss2(G.sequence_ss2(seed)):
            assert line in reached, f"rgbagen.features_ss2 names a line the census does not know: {line}"
            reached[line].append(seed)
    short = {line: (seeds, CENSUS_SS2[line]) for line, seeds in reached.items() if len(seeds) < CENSUS_SS2[line]}
    assert not short, "census lines the committed ss2 seeds do not reach (line: (seeds that do, seeds wanted)): " + repr(short)


def numpy_frame_ss2(seq, L, off, tints, lut, slots, g, frame):
    """one half-size frame of an ss2 launch with no oracle call and none of quad_means' code: the stripe's rows ONLY, texels interleaved
    from the four planes and gathered with the raw offsets, lut[c][tint] where tint < 6, zero-padded to even size, the four samples of a
    quad as strided slices, and round-half-up written as (2 s + n) // (2 n) - equal to (s + n // 2) // n for every s and n = 1 .. 4"""
    W, H, r0, r1, x0, y0 = seq["W"], seq["H"], seq["r0"], seq["r1"], L["x0"], L["y0"]
    off2, tin2 = np.asarray(off).reshape(H, W)[r0:r1], np.asarray(tints).reshape(H, W)[r0:r1]
    rows = r1 - r0
    mapped = off2 != 0xFFFFFFFF
    idx = np.where(mapped, off2, 0).astype(np.int64)
    classed = mapped & (tin2 < 6)
    t = np.where(classed, tin2, 0).astype(np.int64)
    texels = np.zeros(6 * seq["ps"] ** 2, np.uint32)
    for c in range(4):
        texels |= slots(4 * g + c).reshape(-1).astype(np.uint32) << np.uint32(8 * c)
    px = texels[idx]
    He, We = rows + rows % 2, W + W % 2
    cnt = np.zeros((He, We), np.int64)
    cnt[:rows, :W] = mapped
    n = cnt[0::2, 0::2] + cnt[0::2, 1::2] + cnt[1::2, 0::2] + cnt[1::2, 1::2]
    out = np.zeros((He // 2, We // 2), np.uint32)
    for c in range(4):
        b = ((px >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.int64)
        if lut is not None:
            b = np.where(classed, lut[c][t, b], b).astype(np.int64)
        v = np.zeros((He, We), np.int64)
        v[:rows, :W] = np.where(mapped, b, 0)
        s = v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
        out |= ((2 * s + n) // (2 * np.maximum(n, 1))).astype(np.uint32) << np.uint32(8 * c)
    window = frame.view(np.uint32)[y0 + r0 // 2:y0 + r0 // 2 + He // 2, x0:x0 + We // 2]
    window[n > 0] = out[n > 0]


def test_round_half_up_both_ways():
    """the two roundings - the expectation's and the model's - are the same function on everything a quad can hold"""
    for n in (1, 2, 3, 4):
        s = np.arange(255 * n + 1)
        assert np.array_equal((s + n // 2) // n, (2 * s + n) // (2 * n)), n


@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_oracle_expectation_equals_the_numpy_model_ss2(seed):
    seq = G.sequence_ss2(seed)
    pal = G.palette(seq)
    globes = {}

    def slots(s):
        if s not in globes:
            globes[s] = G.slot_globe(seq, s)
        return globes[s]

    for i, L, off, tints, lut, ev in G.walk(seq):
        want = G.expected(seq, L, off, tints, lut, pal, slots)
        # the model's own placement, as above; an ss2 launch's frames are frame_h rows of `pitch` bytes like any other, only half the size
        ring = seq["R"] if L["kind"] == "apply8" else seq["R"] // 4
        size = L["frame_h"] * L["pitch"]
        model = np.full(L["ptr_off"] + L["nframes"] * L["stride"], G.FILL, np.uint8)
        for f in range(L["nframes"]):
            frame = np.full((L["frame_h"], L["pitch"]), G.FILL, np.uint8)
            if L["kind"] in ("ss2", "ss2_tinted"):
                numpy_frame_ss2(seq, L, off, tints, lut, slots, (L["first"] + f) % ring, frame)
            else:
                G.numpy_frame(seq, L, off, tints, lut, pal, slots, (L["first"] + f) % ring, frame)
            model[L["ptr_off"] + f * L["stride"]:L["ptr_off"] + f * L["stride"] + size] = frame.ravel()
        assert want.shape == model.shape, G.describe(seq, i)
        if not np.array_equal(want, model):
            at = int(np.flatnonzero(want != model)[0])
            raise AssertionError(f"{G.describe(seq, i)}: the oracle's expectation and the numpy model differ at byte {at}: {want[at]} / {model[at]}")


def test_ss2_model_seeds_hold_both_ss2_flavours_a_stripe_and_both_events():
    seqs = [G.sequence_ss2(s) for s in MODEL_SEEDS]
    kinds = {l["kind"] for q in seqs for l in q["launches"]}
    assert {"ss2", "ss2_tinted"} <= kinds, kinds
    assert any((q["r0"], q["r1"]) != (0, q["H"]) for q in seqs)
    assert {q["event"]["kind"] for q in seqs} == {"set_lensmap", "mutate_lut"}
