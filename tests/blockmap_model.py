"""TEST INFRASTRUCTURE: the NUMBERS of the staged apply's block map in numpy, no GPU and no built library - what coop_compile_kernel and
coop_order_kernel (blinky_amd/csrc/bk_apply_coop.hip) report beside the chunk lists: per-block cost, the CS_* statistics, walk order, band
starts, the "uneven" flag, the traffic model's words and the row costs.  tests/test_blockmap_stats_gpu.py holds bk_debug_tile_stats,
bk_debug_traffic_model, bk_debug_band_balance and bk_debug_row_costs to it, exactly; tests/test_blockmap_model_cpu.py holds it to a second
formulation (Python sets), to identities, to device values recorded in profiles/r05_bench_line.json, and keeps the census of the small
tables below.

What is a REFERENCE here and what a DEFINITION.  The counts - distinct chunks, distinct 128-byte lines and mapped pixels of a block, the
distinct lines of a stripe - are counted independently of the device code: from the table in the reference layout (plate * ps^2 +
py * ps + px, NULL = 0xFFFFFFFF) and the fact that a globe line is a tile of 16 x 8 texels and a chunk one 16-texel row of it (as in
tests/footprint_model.py); nothing of bk_texel_offset is needed, any numbering that keeps distinct chunks distinct counts the same.  The
formulas that turn counts into a block's cost, a row's price, the band targets and the uneven flag are definitions restated from the
code, each with the line it restates (bk_apply_coop.hip unless another file is named); a change of such a formula on purpose changes
this file with it.

Blocks are 128 x 8 * rg pixels of the OWNED rows, counted from r0: bx = ceil(W / 128), by = ceil(rows / (8 rg)), block b = row * bx +
column; pixels outside the frame or the stripe count as NULL."""
import numpy as np

import footprint_model as FM

NULL = 0xFFFFFFFF
PLATES = 6
BLOCK_COST = 4              # BK_COOP_BLOCK_COST (:51)
MAX_CHUNKS = 4095           # BK_COOP_MAX_CHUNKS (:46): more chunks than 16-bit LDS addresses reach = a direct-gather ("slow") block
BINS = 65                   # BK_COOP_BINS (:49)
PATCH = 8                   # bk_block_at's PH (:375)


def tint_class(tints):
    """the class a tinted map keeps with a chunk (:198): tint + 1 for the six plates' tints, 0 for everything else (255 and 6 ... 254)"""
    t = np.asarray(tints).astype(np.int64)
    return np.where(t < PLATES, t + 1, 0)


class BlockMap:
    """the per-block numbers of one (table, stripe, height, flavour, block-cost knob); arrays are [by * bx], row-major"""

    def __init__(self, W, H, ps, rows, rg, tinted, block_cost, nchunks, lines, mapped, unique_lines, row_mapped):
        self.W, self.H, self.ps, self.rows, self.rg, self.tinted, self.block_cost = W, H, ps, rows, rg, tinted, block_cost
        self.bh = 8 * rg
        self.bx = (W + 127) // 128
        self.by = (rows[1] - rows[0] + self.bh - 1) // self.bh
        self.nblocks = self.bx * self.by
        self.nchunks, self.lines, self.mapped = nchunks, lines, mapped
        self.unique_lines = unique_lines            # distinct lines of the whole stripe
        self.row_mapped = row_mapped                # mapped pixels of every owned row
        self.slow = nchunks > MAX_CHUNKS            # :245
        self.empty = nchunks == 0                   # :296 (any_blk)
        self.listed = ~self.slow & ~self.empty      # has a chunk list; what the statistics sum over (:306)
        # :303  cost[blk] = !any_blk ? 0 : slow ? N / 4 : lines + mapped * 5 / 512 + block_cost, N = 1024 rg pixels per block
        self.cost = np.where(self.empty, 0, np.where(self.slow, 1024 * rg // 4, lines + mapped * 5 // 512 + block_cost)).astype(np.int64)

    def with_block_cost(self, block_cost):
        """the same counts priced with another block-cost knob (bk_debug_set_tile_shape 601 + n)"""
        return BlockMap(self.W, self.H, self.ps, self.rows, self.rg, self.tinted, block_cost, self.nchunks, self.lines, self.mapped,
                        self.unique_lines, self.row_mapped)


def block_map(offsets, tints, W, H, ps, rows=None, rg=4, tinted=False, block_cost=BLOCK_COST):
    """offsets: the WHOLE table, uint32 [H * W]; tints uint8 [H * W] (None = all 255); rows = (r0, r1) the owned rows"""
    assert rg in (1, 2, 4)
    r0, r1 = rows if rows is not None else (0, H)
    nrows, bh, bx = r1 - r0, 8 * rg, (W + 127) // 128
    by = (nrows + bh - 1) // bh
    o = np.asarray(offsets, dtype=np.uint32).reshape(H, W)[r0:r1]
    live = o != NULL
    row_mapped = live.sum(axis=1).astype(np.int64)
    yy, xx = np.nonzero(live)
    blk = (yy // bh) * bx + xx // 128
    v = o[live].astype(np.int64)
    plate, rem = v // (ps * ps), v % (ps * ps)
    py, px = rem // ps, rem % ps
    th, tw = FM.tile_grid(ps)
    line = (plate * th + py // 8) * tw + px // 16                       # the tile (plate, py // 8, px // 16), numbered
    key = line * 8 + py % 8                                             # the chunk (plate, py, px // 16): row py % 8 of its tile
    if tinted:
        cls = tint_class(np.full(H * W, 255, np.uint8) if tints is None else tints).reshape(H, W)[r0:r1][live]
        key = key * 8 + cls                                             # ... once per tint class its pixels need
    shift = 6 if tinted else 3                                          # key -> line
    # one sort of (block, key): runs of equal values are the distinct keys of a block, and the line is a prefix of the key
    s = np.sort(blk * (1 << 40) + key)
    first = np.ones(len(s), bool)
    first[1:] = s[1:] != s[:-1]
    first_line = np.ones(len(s), bool)
    first_line[1:] = (s[1:] >> shift) != (s[:-1] >> shift)
    nb = bx * by
    nchunks = np.bincount(s[first] >> 40, minlength=nb).astype(np.int64)
    lines = np.bincount(s[first_line] >> 40, minlength=nb).astype(np.int64)
    mapped = np.bincount(blk, minlength=nb).astype(np.int64)
    seen = np.zeros(PLATES * th * tw + 1, bool)
    seen[line] = True
    return BlockMap(W, H, ps, (r0, r1), rg, tinted, block_cost, nchunks, lines, mapped, int(seen.sum()), row_mapped)


def lds_need_bin(nchunks):
    """:308  the 1 KiB bin of a listed block's LDS need: min(64, ceil(nchunks * 16 / 1024))"""
    return np.minimum(BINS - 1, (nchunks * 16 + 1023) // 1024)


def tile_stats(bm, lds_bytes):
    """bk_debug_tile_stats (coopmap_stats :1738-1739; slow = CS_SLOW_BLOCKS + the listed blocks whose bin is past the staging buffer,
    coop_stats_wait :1099-1101).  lds_bytes: the staging buffer of the launch - the launcher's choice, handed through"""
    over = bm.listed & (lds_need_bin(bm.nchunks) > lds_bytes // 1024)
    return dict(tiles=bm.nblocks, slow=int(bm.slow.sum() + over.sum()), empty=int(bm.empty.sum()), lds_bytes_per_wave=lds_bytes,
                tile_h=bm.bh + 1000 * 128, lines=int(bm.lines[bm.listed].sum()))


def traffic_model(bm):
    """bk_debug_traffic_model (coopmap_traffic_model :1648-1656; unique lines and mapped pixels by mark_lines_kernel :1598-1610)"""
    chunks = int(bm.nchunks[bm.listed].sum())
    nlive = bm.nblocks - int(bm.empty.sum())
    return dict(unique_globe_lines=bm.unique_lines, staged_lines=int(bm.lines[bm.listed].sum()), staged_chunks=chunks,
                blockmap_bytes_per_visit=8 * bm.nblocks + 4 * chunks + nlive * 1024 * bm.rg * 2,       # :1652
                mapped_pixels=int(bm.mapped.sum()), frames_per_visit=8, blocks=bm.nblocks, block_height=bm.bh)


def walk(bx, by):
    """position l of the walk -> block number (bk_block_at :372-381 without BK_AB_ROW_MAJOR): patches of 8 block rows, walked column
    by column; the last patch is by - 8 * srow rows tall"""
    l = np.arange(bx * by, dtype=np.int64)
    per_patch = PATCH * bx
    srow, rem = l // per_patch, l % per_patch
    tall = np.minimum(PATCH, by - srow * PATCH)
    col, row = rem // tall, rem % tall
    return (srow * PATCH + row) * bx + col


def band_balance(bm):
    """bk_debug_band_balance (coop_order_kernel :913-963, coopmap_band_balance :1687-1694)"""
    nb = bm.nblocks
    c = bm.cost[walk(bm.bx, bm.by)]                                     # costs in walk order, empty blocks included
    order = np.nonzero(c)[0]
    cum = np.cumsum(c[order])                                           # :928
    nlive, total = len(order), int(c.sum())
    starts = [0] * 9
    starts[8] = nlive
    for k in range(1, 8):                                               # :938-944  first live block whose prefix passes total * k / 8
        starts[k] = int(np.searchsorted(cum, total * k // 8, side="right"))
    band_cost = [int(c[order][starts[k]:starts[k + 1]].sum()) for k in range(8)]         # :1693
    per = (nb + 7) // 8                                                 # :1282
    u = np.bincount(np.minimum(7, np.arange(nb) // per), weights=c, minlength=8).astype(np.int64)     # :918
    return dict(starts=starts, live_blocks=nlive, equal_count_bands_uneven=bool(int(u.max()) * 80 > total * 11),       # :963
                band_cost=band_cost)


def row_costs(bm):
    """bk_debug_row_costs of the staged apply: uint32 [H], 0 outside the owned rows (coop_row_cost_kernel :1707-1710: a block row's
    cost S spread over the `here` rows it has, x 16, rounded, + 16)"""
    r0, r1 = bm.rows
    out = np.zeros(bm.H, np.int64)
    S = bm.cost.reshape(bm.by, bm.bx).sum(axis=1)
    y = np.arange(r1 - r0)
    b = y // bm.bh
    here = np.minimum(bm.bh, (r1 - r0) - b * bm.bh)
    out[r0:r1] = (S[b] * 16 + here // 2) // here + 16
    return out.astype(np.uint32)


def row_costs_direct(bm):
    """... and of the direct-gather apply (variant 0; row_cost_kernel, bk_probe.hip:36): mapped pixels + max(1, W / 32) - W / 32 for
    every frame at least 32 wide; the floor of 1 keeps a narrower frame's empty rows from costing nothing (bk_debug_stripe_bounds
    prices its rows the same way, bk_comm.cpp:403)"""
    out = np.zeros(bm.H, np.int64)
    out[bm.rows[0]:bm.rows[1]] = bm.row_mapped + max(1, bm.W // 32)
    return out.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the small tables both test files use (tests/test_blockmap_model_cpu.py keeps their census)
# ---------------------------------------------------------------------------------------------------------------------------------
TINTS = np.array([0, 1, 2, 3, 4, 5, 6, 200, 255], np.uint8)
ORACLE_TABLES = [("cube", "panini", None, 640, 480), ("cube", "hammer", None, 640, 400), ("cube", "panini", "f_fov 120", 322, 203)]
DRAW_SIZES = [(129, 33), (257, 100), (517, 199)]
DRAW_SEEDS = {(129, 33): range(0, 8), (257, 100): range(8, 14), (517, 199): range(14, 20)}
HEIGHTS = (1, 2, 4)


class Table:
    def __init__(self, name, W, H, off, tints):
        self.name, self.W, self.H, self.ps = name, W, H, min(W, H)
        self.off, self.tints = np.ascontiguousarray(off, np.uint32).ravel(), np.ascontiguousarray(tints, np.uint8).ravel()

    def stripes(self):
        """whole frame; (r0, r1) off every multiple of 8; one row; the last rows"""
        H = self.H
        out = [(0, H)]
        if H >= 20:
            out += [(3, H - 6), (H // 2 + 1, H // 2 + 2), (H - 13, H)]
        elif H > 1:
            out += [(1, H - 1), (H - 1, H)]
        return out

    def __repr__(self):
        return self.name


def spread_tints(seed, n):
    return TINTS[np.random.default_rng(seed).integers(0, len(TINTS), n)]


def chunk_block_table(ndistinct, seed):
    """128 x 128 (ps 128: 6 * 128 * 8 = 6144 chunks) whose first 128 x 32 pixels read `ndistinct` <= 4096 different chunks, each at
    least once, in a shuffled order; the rows below read plate 5 smoothly, with a NULL hole"""
    rng = np.random.default_rng(seed)
    ps = 128
    chunk = np.concatenate([np.arange(ndistinct), rng.integers(0, ndistinct, 4096 - ndistinct)])
    rng.shuffle(chunk)
    plate, py, cx = chunk // 1024, (chunk % 1024) // 8, chunk % 8
    top = plate * ps * ps + py * ps + cx * 16 + rng.integers(0, 16, 4096)
    yy, xx = np.mgrid[32:128, 0:128]
    rest = 5 * ps * ps + ((yy * 3 + xx // 5) % ps) * ps + (xx + yy) % ps
    rest[20:40, 30:70] = NULL
    return np.concatenate([top, rest.ravel()]).astype(np.uint32)


def draw_tables():
    """draws of test_apply_campaign_gpu._table that between them have every kind and every NULL pattern (the CPU census checks it), with
    tints from TINTS"""
    from test_apply_campaign_gpu import _table
    out = []
    for (W, H) in DRAW_SIZES:
        for seed in DRAW_SEEDS[(W, H)]:
            off, _, what = _table(np.random.default_rng(4400 + seed), W, H, min(W, H))
            out.append(Table(f"draw{seed}-{W}x{H}-{what}", W, H, off, spread_tints(seed, W * H)))
    return out


def constructed_tables():
    out = []
    out.append(Table("1x1", 1, 1, [0], [3]))
    yy, xx = np.mgrid[0:9, 0:3]
    off = ((yy % 6) * 9 + (yy % 3) * 3 + xx).astype(np.uint32)              # ps 3: plate y % 6, texel row y % 3
    off[4, 1] = NULL
    out.append(Table("3x9", 3, 9, off, spread_tints(39, 27)))
    yy, xx = np.mgrid[0:8, 0:128]
    out.append(Table("128x8", 128, 8, ((xx % 6) * 64 + yy * 8 + (xx // 6) % 8).astype(np.uint32), spread_tints(1288, 1024)))   # ps 8
    out.append(Table("chunks4096", 128, 128, chunk_block_table(4096, 1), np.full(128 * 128, 255, np.uint8)))
    out.append(Table("chunks4095", 128, 128, chunk_block_table(4095, 2), np.full(128 * 128, 255, np.uint8)))
    return out


def oracle_tables():
    import oracle_ffi as O
    out = []
    for cfg in ORACLE_TABLES:
        lm = O.lensmap(*cfg)
        name = "-".join(str(c) for c in cfg if c is not None).replace(" ", "")
        tints = lm.tints.copy()
        if cfg[3] == 322:                                                   # (one lens table with tints the rubix grid never writes)
            tints = spread_tints(322, len(tints))
        out.append(Table(name, lm.W, lm.H, lm.offsets, tints))
    return out


_tables = None


def small_tables():
    global _tables
    if _tables is None:
        _tables = oracle_tables() + draw_tables() + constructed_tables()
    return _tables
