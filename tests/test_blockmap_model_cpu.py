"""tests/blockmap_model.py (the expectation of tests/test_blockmap_stats_gpu.py) without a GPU: held to a second formulation - Python
sets per block and plain loops, none of the model's helpers -, to identities between its numbers, and to the values an MI355X
reported for the bench configurations (profiles/r05_bench_line.json, quoted inline); and the CENSUS of the small tables the GPU file
runs, which fails when one of the cases a block map can go wrong at is no longer reached by any of them."""
import numpy as np
import pytest

import blockmap_model as BM
import footprint_model as FM
import oracle_ffi as O


# ---- the second formulation ----------------------------------------------------------------------------------------------------
def collect(t, rows):
    """one pass over the stripe's pixels, in plain Python -> {(rg, tinted): (chunk sets, line sets, mapped counts)}, all lines seen"""
    W, ps = t.W, t.ps
    r0, r1 = rows
    bx = -(-W // 128)
    out = {}
    for rg in (1, 2, 4):
        nb = bx * -(-(r1 - r0) // (8 * rg))
        lines, mapped = [set() for _ in range(nb)], [0] * nb
        out[(rg, False)] = ([set() for _ in range(nb)], lines, mapped)
        out[(rg, True)] = ([set() for _ in range(nb)], lines, mapped)
    all_lines = set()
    off, tin = t.off.tolist(), t.tints.tolist()
    for y in range(r0, r1):
        for x in range(W):
            o = off[y * W + x]
            if o == 0xFFFFFFFF:
                continue
            plate, rem = divmod(o, ps * ps)
            py, px = divmod(rem, ps)
            tint = tin[y * W + x]
            line = (plate, py // 8, px // 16)
            all_lines.add(line)
            for rg in (1, 2, 4):
                b = ((y - r0) // (8 * rg)) * bx + x // 128
                plain, lines, mapped = out[(rg, False)]
                plain[b].add((plate, py, px // 16))
                out[(rg, True)][0][b].add((plate, py, px // 16, tint + 1 if tint < 6 else 0))
                lines[b].add(line)
                mapped[b] += 1
    return out, all_lines


def by_sets(t, rows, rg, tinted, collected, block_cost=4, lds_bytes=65536):
    """everything the model gives, from the sets, in plain loops -> (tile_stats, traffic_model, band_balance, row_costs list)"""
    W, H = t.W, t.H
    r0, r1 = rows
    bh = 8 * rg
    bx, by = -(-W // 128), -(-(r1 - r0) // bh)
    (chunks, lines, mapped), all_lines = collected[0][(rg, tinted)], collected[1]
    cost, nslow, nover, nempty, slines, schunks = [], 0, 0, 0, 0, 0
    for b in range(bx * by):
        n = len(chunks[b])
        if n == 0:
            nempty += 1
            cost.append(0)
        elif n > 4095:
            nslow += 1
            cost.append(1024 * rg // 4)
        else:
            slines += len(lines[b])
            schunks += n
            nover += 1 if min(64, -(-n * 16 // 1024)) > lds_bytes // 1024 else 0
            cost.append(len(lines[b]) + mapped[b] * 5 // 512 + block_cost)
    stats = dict(tiles=bx * by, slow=nslow + nover, empty=nempty, lds_bytes_per_wave=lds_bytes, tile_h=bh + 128000, lines=slines)
    traffic = dict(unique_globe_lines=len(all_lines), staged_lines=slines, staged_chunks=schunks,
                   blockmap_bytes_per_visit=8 * bx * by + 4 * schunks + (bx * by - nempty) * 1024 * rg * 2, mapped_pixels=sum(mapped),
                   frames_per_visit=8, blocks=bx * by, block_height=bh)
    # the walk: patches of 8 block rows, column by column
    order = []
    for p0 in range(0, by, 8):
        for col in range(bx):
            for row in range(p0, min(p0 + 8, by)):
                order.append(row * bx + col)
    live = [b for b in order if cost[b]]
    total = sum(cost)
    starts = [0]
    for k in range(1, 8):
        run, at = 0, len(live)
        for i, b in enumerate(live):
            run += cost[b]
            if run > total * k // 8:
                at = i
                break
        starts.append(at)
    starts.append(len(live))
    band_cost = [sum(cost[b] for b in live[starts[k]:starts[k + 1]]) for k in range(8)]
    per = -(-bx * by // 8)
    u = [0] * 8
    for l, b in enumerate(order):
        u[min(7, l // per)] += cost[b]
    bands = dict(starts=starts, live_blocks=len(live), equal_count_bands_uneven=max(u) * 80 > total * 11, band_cost=band_cost)
    rc = [0] * H
    for y in range(r1 - r0):
        b = y // bh
        here = min(bh, (r1 - r0) - b * bh)
        rc[r0 + y] = (sum(cost[b * bx:(b + 1) * bx]) * 16 + here // 2) // here + 16
    return stats, traffic, bands, rc


def model_outputs(t, rows, rg, tinted, block_cost=4, lds_bytes=65536):
    bm = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, tinted, block_cost)
    return BM.tile_stats(bm, lds_bytes), BM.traffic_model(bm), BM.band_balance(bm), BM.row_costs(bm).tolist()


def _set_cases():
    """the small tables, the 100 000-pixel ones as stripes only (the loop above is plain Python)"""
    out = []
    for t in BM.small_tables():
        for rows in t.stripes():
            if t.W * (rows[1] - rows[0]) <= 30000:
                out.append((t, rows))
    return out


@pytest.mark.parametrize("t,rows", _set_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_model_equals_the_sets(t, rows):
    collected = collect(t, rows)
    for rg in BM.HEIGHTS:
        for tinted in (False, True):
            for block_cost, lds in ((4, 65536), (0, 1024), (9, 4096)):
                want = by_sets(t, rows, rg, tinted, collected, block_cost, lds)
                got = model_outputs(t, rows, rg, tinted, block_cost, lds)
                for g, w, what in zip(got, want, ("tile_stats", "traffic_model", "band_balance", "row_costs")):
                    assert g == w, f"{t} rows {rows} rg {rg} tinted {tinted} block cost {block_cost} lds {lds}: {what}"


def test_walk_is_a_permutation_and_follows_the_patches():
    for bx, by in ((1, 1), (5, 1), (5, 8), (5, 9), (3, 25), (1, 17), (7, 16)):
        w = BM.walk(bx, by).tolist()
        assert sorted(w) == list(range(bx * by))
        want = [row * bx + col for p0 in range(0, by, 8) for col in range(bx) for row in range(p0, min(p0 + 8, by))]
        assert w == want


# ---- identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", BM.small_tables(), ids=str)
def test_identities(t):
    for rows in t.stripes():
        mapped = int((t.off.reshape(t.H, t.W)[rows[0]:rows[1]] != BM.NULL).sum())
        foot = sum(FM.footprint(t.off, t.W, t.H, t.ps, rows)[1])
        for rg in BM.HEIGHTS:
            plain = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, False)
            tinted = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, True)
            assert (plain.nchunks <= tinted.nchunks).all() and (plain.lines == tinted.lines).all() and (plain.mapped == tinted.mapped).all()
            assert (tinted.nchunks <= 7 * plain.nchunks).all() and (plain.lines <= plain.nchunks).all() and (plain.nchunks <= plain.mapped).all()
            for bm in (plain, tinted):
                tm, bb = BM.traffic_model(bm), BM.band_balance(bm)
                assert tm["unique_globe_lines"] == foot and tm["mapped_pixels"] == mapped
                if not bm.slow.any():
                    assert tm["staged_lines"] >= tm["unique_globe_lines"]
                assert sum(bb["band_cost"]) == int(bm.cost.sum())
                assert bb["starts"] == sorted(bb["starts"]) and bb["starts"][0] == 0 and bb["starts"][8] == bb["live_blocks"]
                rc = BM.row_costs(bm).astype(np.int64)
                assert (rc[rows[0]:rows[1]] >= 16).all() and not rc[:rows[0]].any() and not rc[rows[1]:].any()
                # a row's price times the rows of its block row is the block row's cost x 16, to rounding, + 16 per row
                S = bm.cost.reshape(bm.by, bm.bx).sum(axis=1)
                for b in range(bm.by):
                    seg = rc[rows[0] + b * bm.bh:min(rows[0] + (b + 1) * bm.bh, rows[1])]
                    assert abs(int((seg - 16).sum()) - 16 * int(S[b])) <= len(seg) // 2 + 1 and len(set(seg.tolist())) == 1
                d = BM.row_costs_direct(bm).astype(np.int64)
                assert int(d.sum()) == mapped + (rows[1] - rows[0]) * max(1, t.W // 32)


# ---- what the device reported ---------------------------------------------------------------------------------------------------
def compulsory_bytes(model, F):
    """bench.py's compulsory_bytes, restated"""
    visits = -(-F // int(model["frames_per_visit"])) if F >= 8 else 1
    if 8 <= F < 16:
        visits = 2
    return F * (model["mapped_pixels"] + 128 * model["unique_globe_lines"]) + visits * model["blockmap_bytes_per_visit"]


# profiles/r05_bench_line.json: (globe, lens, zoom, W, H), tile_h of the record, its tile_stats words, {frames per launch: compulsory_bytes_per_launch}.
# The 8K line (C5) is left out for time: its table alone takes the CPU oracle several seconds.  That file's "headline, rubix on" line
# (459 707 608) is NOT used: it is stale - it is the PLAIN map's figure plus a tint byte per pixel and frame (16 x 8 294 400 more, 2 x 4 x
# 63 102 bytes of chunk list fewer = 16 x 8 262 849), which the byte model lost when the tint moved into the chunk list (bench.py: "the
# tint plane is not read by the apply any more").  The record
# taken after that change, profiles/r05_bench_line_final_code.json, has the same line at 327 502 024: the tinted model's figure, below.
RECORDED = [
    (("cube", "panini", "f_fov 180", 3840, 2160), 128032, dict(tiles=2040, empty=0, lines=108133), {64: 1307988832}),
    (("cube", "stereographic", None, 1920, 1080), 128016, dict(tiles=1020, empty=0, lines=37421), {16: 90340720, 64: 361362880}),
    (("cube", "quincuncial", None, 3840, 2160), 128008, dict(tiles=8100, empty=3240, lines=346590), {16: 556502920}),
    (("cube", "hammer", None, 3840, 2160), 128016, dict(tiles=4050, empty=1088, lines=289536), {16: 579462504}),
]
HEADLINE_MODEL = dict(unique_globe_lines=75719, staged_lines=108133, staged_chunks=719787, blockmap_bytes_per_visit=19607148,
                      mapped_pixels=8294400, frames_per_visit=8, blocks=2040, block_height=32)        # "roofline" / "model" of the same file


RUBIX_ON_FINAL_CODE = 327502024        # profiles/r05_bench_line_final_code.json, "headline, rubix on": 16 frames per launch, tile_h 128032


@pytest.mark.parametrize("cfg,tile_h,stats,launches", RECORDED, ids=lambda v: "-".join(map(str, v[:2])) if isinstance(v, tuple) else None)
def test_recorded_device_values(cfg, tile_h, stats, launches):
    lm = O.lensmap(*cfg)
    rg = (tile_h - 128000) // 8
    bm = BM.block_map(lm.offsets, lm.tints, lm.W, lm.H, lm.ps, None, rg, False)
    ts, tm = BM.tile_stats(bm, 65536), BM.traffic_model(bm)
    assert ts["tile_h"] == tile_h and {k: ts[k] for k in stats} == stats
    for F, want in launches.items():
        assert compulsory_bytes(tm, F) == want, F
    if cfg[2] == "f_fov 180":
        assert tm == HEADLINE_MODEL
        tinted = BM.block_map(lm.offsets, lm.tints, lm.W, lm.H, lm.ps, None, rg, True)      # the default rubix grid's tints
        assert BM.tile_stats(tinted, 65536)["lines"] == 108133 and compulsory_bytes(BM.traffic_model(tinted), 16) == RUBIX_ON_FINAL_CODE


# ---- the census ----------------------------------------------------------------------------------------------------------------
def test_census_of_the_small_tables():
    """every case the GPU file is there for is reached by at least one (table, stripe, height) it runs"""
    seen = set()
    kinds, nulls = set(), set()
    for t in BM.small_tables():
        if t.name.startswith("draw"):
            kind, null = t.name.split("-")[-1].split("/")
            kinds.add(kind)
            nulls.add(null)
        if t.W % 128:
            seen.add("W % 128 != 0")
        if ((t.tints >= 6) & (t.tints < 255) & (t.off != BM.NULL)).any():
            seen.add("a tint in 6..254")
        for rows in t.stripes():
            n = rows[1] - rows[0]
            if rows[0] % 8:
                seen.add("r0 % 8 != 0")
            if n == 1:
                seen.add("one-row stripe")
            for rg in BM.HEIGHTS:
                if n % (8 * rg):
                    seen.add(f"rows % {8 * rg} != 0")
                plain = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, False)
                tinted = BM.block_map(t.off, t.tints, t.W, t.H, t.ps, rows, rg, True)
                if (tinted.nchunks > plain.nchunks).any():
                    seen.add("a chunk under two tint classes")
                for bm in (plain, tinted):
                    if bm.empty.any():
                        seen.add("empty blocks")
                    if bm.slow.any():
                        seen.add("a slow block")
                    if (bm.nchunks == 4095).any():
                        seen.add("a listed block of 4095 chunks")
                    if (bm.mapped == 1).any():
                        seen.add("a block with one mapped pixel")
                    if bm.by < 8:
                        seen.add("by < 8")
                    if bm.by > 8 and bm.by % 8:
                        seen.add("by > 8, by % 8 != 0")
                    if bm.nblocks < 8:
                        seen.add("fewer than 8 blocks")
                    bb = BM.band_balance(bm)
                    if bb["live_blocks"] >= 64:
                        seen.add(">= 64 live blocks")
                    seen.add("uneven" if bb["equal_count_bands_uneven"] else "even")
                    if bb["live_blocks"] >= 8 and any(bb["starts"][k] == bb["starts"][k + 1] for k in range(8)):
                        seen.add("a band of length 0 among >= 8 live blocks")
                    if any(bb["starts"][k] == bb["starts"][k + 1] for k in range(8)):
                        seen.add("a band of length 0")
                    c = bm.cost[BM.walk(bm.bx, bm.by)]
                    cum, total = np.cumsum(c[c > 0]), int(c.sum())
                    if any(total * k // 8 in cum for k in range(1, 8)):
                        seen.add("a cost prefix equal to a band target")             # (where <= and < in the band search part)
                    S = bm.cost.reshape(bm.by, bm.bx).sum(axis=1)
                    here = np.minimum(bm.bh, n - np.arange(bm.by) * bm.bh)
                    if ((S * 16 + here // 2) // here != S * 16 // here).any():
                        seen.add("a row price that rounds up")
                    for kb in (1, 4):
                        if (bm.listed & (BM.lds_need_bin(bm.nchunks) > kb)).any():
                            seen.add(f"LDS need over {kb} KiB")
                        if (bm.listed & (BM.lds_need_bin(bm.nchunks) <= kb)).any():
                            seen.add(f"LDS need within {kb} KiB")
    want = {"W % 128 != 0", "a tint in 6..254", "r0 % 8 != 0", "one-row stripe", "rows % 8 != 0", "rows % 16 != 0", "rows % 32 != 0",
            "a chunk under two tint classes", "empty blocks", "a slow block", "a listed block of 4095 chunks", "a block with one mapped pixel",
            "by < 8", "by > 8, by % 8 != 0", "fewer than 8 blocks", ">= 64 live blocks", "uneven", "even", "a band of length 0",
            "a band of length 0 among >= 8 live blocks", "LDS need over 1 KiB", "LDS need over 4 KiB", "LDS need within 1 KiB", "LDS need within 4 KiB",
            "a cost prefix equal to a band target", "a row price that rounds up"}
    assert want - seen == set(), sorted(want - seen)
    assert kinds == {"random", "rows", "columns", "smooth"} and nulls == {"none", "sprinkled", "blob", "most"}, (kinds, nulls)
