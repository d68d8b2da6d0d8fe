"""The truecolour apply campaign (tests/rgbagen.py, tests/test_apply_rgba_campaign_gpu.py), as far as it can be checked without a GPU.

(a) The expectation is right.  The GPU campaign compares against rgbagen.expected, which asks the oracle's 8-bit apply for every byte plane.
For a few seeds the same allocations are computed a second way with no oracle call - the four planes interleaved into 32-bit texels, gathered
with the raw offsets, lut[c][tint] where tint < 6, NULL pixels and the rows outside the stripe left alone - and must be equal byte for byte.

(b) The census.  What the committed seeds reach, read off the generator's output alone: a precondition on the campaign's INPUTS, never a
filter on its results.  A generator or seed-range change that empties a line fails here and says which."""
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
