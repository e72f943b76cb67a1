"""The persistent kernels (k_decode, k_decode_tile, k_decode_rows, k_encode)
when a workgroup takes SEVERAL units: the table of rows behind
tests/test_persist_ranges.py (CPU) and tests/test_gpu_persistent_ranges.py
(GPU), and a restatement of the work partition in plain Python that calls
nothing of the library.

The partition (csrc/decode.hip launch_persistent, csrc/encode.hip
launch_encode_persistent): a launch of n_units units runs G = min(n_units,
resident workgroups) workgroups; workgroup g walks the contiguous range
[q0, q1) with per = n_units // G, rem = n_units % G and the first rem ranges
one unit longer.  Unit positions q are chunk-major in increasing address:
chunk c = q // nseg, sidx = nseg - 1 - q % nseg (unit sidx ends sidx * 32 KiB
before the 16-byte aligned end of the chunk).  Consecutive positions of one
chunk inside one range are a RUN: one reduction, one shift by the last unit's
constant, one publication.  For k_decode_tile a unit is a tile and nseg the
tiles per chunk (tile_cases.tiles: column block fastest).

In the tuning build the grid is capped by zhip_set_tuning(ZHIP_TUNE_MAX_GRID,
G), so every row names the caps it runs under; G = n_units is the control (one
unit per workgroup, what every other test of these kernels launches)."""

from collections import namedtuple

import numpy as np

import dtype_cases as DC
import tile_cases as TC

LE, BE = TC.LE, TC.BE
UNIT = 32768

K_DEC, K_ROWS, K_TILE, K_ENC = "k_decode", "k_decode_rows", "k_decode_tile", "k_encode"
TUNE_PERSIST = 64  # ablation bit: whole-row layouts keep the persistent kernels (k_decode_rows, k_encode)


def nseg_of(nbytes):
    """Units of a chunk of nbytes decoded bytes: ceil(align16(nbytes) / 32 KiB)."""
    return -(-((nbytes + 15) & ~15) // UNIT)


def ranges(n_units, G):
    """[(q0, q1)] of workgroups 0 .. G - 1."""
    per, rem = divmod(n_units, G)
    out = []
    for g in range(G):
        q0 = g * per + min(g, rem)
        out.append((q0, q0 + per + (1 if g < rem else 0)))
    return out


Run = namedtuple("Run", "wg chunk sidx len")


def runs(n_units, nseg, G):
    """[(workgroup, chunk, last sidx, run_len)] in launch order of each workgroup."""
    out = []
    for g, (q0, q1) in enumerate(ranges(n_units, G)):
        q = q0
        while q < q1:
            c = q // nseg
            end = min(q1, (c + 1) * nseg)
            out.append(Run(g, c, nseg - 1 - (end - 1) % nseg, end - q))
            q = end
    return out


# ------------------------------------------------------------------- features
LONG_RUN = "run of >= 2 units"
THREE_RUNS = "range of >= 3 runs"
SPLIT_LONG = "chunk split over >= 2 workgroups, a part of >= 2 units"
UNEVEN = "longer range next to a shorter one"
DROP_INSIDE = "dropped chunk strictly inside a range"
WHOLE_BIG = "run of nseg > 32 units"
SPLIT_BIG = "chunk of nseg > 32 split, every part > 1 unit"
FEATURES = (LONG_RUN, THREE_RUNS, SPLIT_LONG, UNEVEN, DROP_INSIDE, WHOLE_BIG, SPLIT_BIG)


def features(n_units, nseg, G, dropped=None):
    """The set of FEATURES a launch of G workgroups shows, by the model alone."""
    rs = runs(n_units, nseg, G)
    rg = ranges(n_units, G)
    out = set()
    if any(r.len >= 2 for r in rs):
        out.add(LONG_RUN)
    per_wg = {}
    for r in rs:
        per_wg[r.wg] = per_wg.get(r.wg, 0) + 1
    if any(n >= 3 for n in per_wg.values()):
        out.add(THREE_RUNS)
    parts = {}
    for r in rs:
        parts.setdefault(r.chunk, []).append(r.len)
    if any(len(p) >= 2 and max(p) >= 2 for p in parts.values()):
        out.add(SPLIT_LONG)
    lens = [b - a for a, b in rg]
    if any(a == b + 1 and b >= 1 for a, b in zip(lens, lens[1:])):
        out.add(UNEVEN)
    if dropped is not None and any(a < dropped * nseg and (dropped + 1) * nseg < b for a, b in rg):
        out.add(DROP_INSIDE)
    if nseg > 32:
        if any(r.len == nseg for r in rs):
            out.add(WHOLE_BIG)
        if any(len(p) >= 2 and min(p) > 1 for p in parts.values()):
            out.add(SPLIT_BIG)
    return out


# ---------------------------------------------------------------------- rows
# id; chunk (sharded rows: the INNER chunk, `shard` the shard shape); dtype; endian; crc; chunk grid (shards for
# sharded rows); decode / encode kernel (encode None: the row is not written); transpose order (tile rows);
# ablation bits the row needs (tuning key 2); fill; sweep: the caps the every-step sweep runs under;
# claims: the features that SOME cap of the row must show (every cap but the control must show at least one)
_SWEEP = (1, 3, "n+1")  # (3 workgroups over 3 chunks split nothing: n_chunks + 1 does)
Row = namedtuple("Row", "id chunk dtype endian crc grid decode encode claims sweep order tune fill shard fast rows",
                 defaults=(_SWEEP, None, 0, 3, None, False, False))

_SMALL = (LONG_RUN, THREE_RUNS, SPLIT_LONG, UNEVEN, DROP_INSIDE)
_BIG = _SMALL + (WHOLE_BIG, SPLIT_BIG)
_ALL_CAPS = None  # the sweep under every cap of the row

ROWS = [
    # k_decode generic (62-byte rows: no 16-byte row pieces), ragged head (71 610 B: 3 units, the first starts
    # 26 694 B before the chunk); 7 chunks, 21 units
    Row("generic-u16le", (35, 33, 31), "uint16", LE, True, (7, 1, 1), K_DEC, K_ENC, _SMALL, _ALL_CAPS),
    Row("generic-u16be", (35, 33, 31), "uint16", BE, True, (1, 7, 1), K_DEC, K_ENC, _SMALL),
    # k_decode fast (whole 48-byte rows), not a row layout (48 is no power of two): 96 000 B, 3 units
    Row("fast-f32", (40, 50, 12), "float32", LE, True, (7, 1, 1), K_DEC, K_ENC, _SMALL, _ALL_CAPS, fast=True),
    # 8-byte items swapped, generic (344-byte rows): 1 135 200 B, 35 units -- the counted arrival
    Row("generic-f64be-35", (33, 100, 43), "float64", BE, True, (3, 1, 1), K_DEC, K_ENC, _BIG),
    # exactly 32 units: the one-word arrival with every bit of the mask (1 044 480 B)
    Row("fast-f32-32", (34, 64, 120), "float32", LE, True, (3, 1, 1), K_DEC, K_ENC, _SMALL, fast=True),
    # 34 units, fast: the counted arrival (1 108 800 B)
    Row("fast-f32-34", (33, 100, 84), "float32", LE, True, (3, 1, 1), K_DEC, K_ENC, _BIG, fast=True),
    # without a checksum: no run end at all, the status from the unit that ends the chunk
    Row("generic-u16le-nocrc", (35, 33, 31), "uint16", LE, False, (7, 1, 1), K_DEC, K_ENC, _SMALL, ()),
    Row("fast-f32-nocrc", (40, 50, 12), "float32", LE, False, (7, 1, 1), K_DEC, K_ENC, _SMALL, (), fast=True),
    # 2 shards of 2 x 1 x 2 inner chunks of the generic geometry: 8 inner chunks, 24 units, the shard indexes
    # checked by workgroups j = g, g + G, ... of the same launch
    Row("sharded-u16le", (35, 33, 31), "uint16", LE, True, (1, 1, 2), K_DEC, None, _SMALL, shard=(70, 33, 62)),
    # k_decode_rows / k_encode on whole-row layouts (128-byte rows), ablation bit 64: 81 920 B, 3 units with a
    # ragged head; and 33 units of 32 KiB planes (1 081 344 B): the counted arrival, runs of more than 32 units
    Row("rows-f32", (10, 64, 32), "float32", LE, True, (7, 1, 1), K_ROWS, K_ENC, _SMALL, _ALL_CAPS,
        tune=TUNE_PERSIST, fast=True, rows=True),
    Row("rows-i16be-33", (33, 64, 256), "int16", BE, True, (3, 1, 1), K_ROWS, K_ENC, _BIG,
        tune=TUNE_PERSIST, fast=True, rows=True),
]

# every general-tile row of tile_cases.py with at least 3 tiles per chunk, and dtype_cases' "tile" family for the
# one instantiation tile_cases' seven do not have (complex64 swapped per component)
_TILE_MIN = 3


def _tile_rows():
    out = []
    for r in TC.ROWS:
        if r.decode != TC.TGEN or r.inner is not None or not r.crc:
            continue
        shape, it, ost = TC.stored_geometry(r)
        if len(TC.tiles(shape, it, ost)) < _TILE_MIN:
            continue
        out.append(Row("tile-" + r.id, r.chunk, r.dtype, r.endian, True, r.grid, K_TILE, None,
                       (LONG_RUN, THREE_RUNS, SPLIT_LONG, UNEVEN), order=r.order, fill=r.fill))
    fam = DC.FAMILY["tile"]
    out.append(Row("tile-dtype-c64be", fam.chunk(8), "complex64", BE, True, (2, 1, 1, 2), K_TILE, None,
                   (LONG_RUN, THREE_RUNS, SPLIT_LONG, UNEVEN), order=fam.order))
    return out


ROWS += _tile_rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

DROPPED = 1  # the table entry (chunk, or inner chunk) every read row drops


def array_shape(row):
    outer = row.shard if row.shard is not None else row.chunk
    return tuple(c * g for c, g in zip(outer, row.grid))


def n_chunks(row):
    """Table entries of a whole read: chunks, or inner chunks of every shard."""
    n = int(np.prod(row.grid))
    if row.shard is not None:
        n *= int(np.prod([s // c for s, c in zip(row.shard, row.chunk)]))
    return n


def units_per_chunk(row):
    """nseg of the row's chunk; tiles per chunk for a tile row."""
    it = np.dtype(row.dtype).itemsize
    if row.decode == K_TILE:
        t = TC.Row(row.id, row.chunk, row.order, row.dtype, row.endian, True, row.grid, None, None)
        return len(TC.tiles(*TC.stored_geometry(t)))
    return nseg_of(int(np.prod(row.chunk)) * it)


def caps(n_ch, n_un):
    """The grid caps of a launch of n_un units over n_ch chunks, ascending;
    the last, n_un, is the control."""
    return sorted({g for g in (1, 2, 3, n_ch + 1, n_un - 1, n_un) if 1 <= g <= n_un})


def row_caps(row):
    n = n_chunks(row)
    return caps(n, n * units_per_chunk(row))


def sweep_caps(row):
    if row.sweep is None:
        return row_caps(row)
    want = [n_chunks(row) + 1 if g == "n+1" else g for g in row.sweep]
    return [g for g in row_caps(row) if g in want]


# the write of every encode row: five chunks along the last dim (test_gpu_kernel_matrix.test_encode_row)
WRITE_CHUNKS = 5


def write_caps(row):
    return caps(WRITE_CHUNKS, WRITE_CHUNKS * units_per_chunk(row))
