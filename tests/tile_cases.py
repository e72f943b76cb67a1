"""The transposing ("tile") kernels at ranks 2, 4 and 5: the table of rows
(tests/test_tile_maps.py on the CPU, tests/test_gpu_tile_matrix.py on the GPU)
and an independent restatement of the tile geometry in plain numpy, which
calls nothing of the library.

Each row names its geometry AND the kernels it must take, so a change of a
selection rule fails a row and has to be acknowledged here.  The rules as of
this table (csrc/capi.cpp zhip_plan_create / mapped_params / the encode
parameters, csrc/decode.hip launch_decode -> launch_tile4 / launch_tile_groups,
csrc/encode.hip launch_encode):

  stored shape = chunk[order]; tq = the first stored dim other than the last
  that is contiguous in out and has shape > 1; a tile is 64 rows of tq by 256
  bytes of the innermost stored row (row bytes a multiple of 16, else no tile
  mode at all); T = tiles per chunk, column block fastest, then row block,
  then the other stored dims in C order (last fastest).

  tile4 family: full tiles (shape[tq] % 64 == 0, row_bytes % 256 == 0),
      T % 4 == 0 and every aligned group of four consecutive tiles at one
      uniform base step
          with a checksum (T <= 64)       k_decode_tile2w   k_encode_tile2
          without                         k_decode_tile4    k_encode_tile4
      (k_encode_tile2 / tile4 only while T <= 64; a full-tile chunk of at most
      256 KiB has T <= 16)
  else grouped: some other stored dim (not the innermost) has shape % 4 == 0
      -- the innermost such is gd -- and shape[tq] % (16 / itemsize) == 0
          with a checksum                 k_decode_tileg2w  k_encode_tileg
          without                         k_decode_tileg    k_encode_tileg
  else general                            k_decode_tile     k_encode_tile
  prefix-box selections (ragged edge chunks), any family: k_encode_tile.

Rank 2 has one "other" count of 1 and can never have a group dim (the only
stored dims are tq and the innermost), so gd stays -1 and the grouped kernels
cannot occur there: the grouped names are asserted at ranks 4 and 5 only.

A decode row's array is an exact multiple of its chunk (planner._tile_ok wants
every chunk fully selected; a ragged array takes the generic k_decode, which
the name assertion would catch)."""

from collections import namedtuple

import numpy as np

LE = {"name": "bytes", "configuration": {"endian": "little"}}
BE = {"name": "bytes", "configuration": {"endian": "big"}}

TILE_ROWS, TILE_COLS = 64, 256

# id, chunk shape, transpose order (None: no transpose codec, F-order out), dtype, endian, checksum, chunk grid,
# decode kernel, encode kernel (None: the row is not encoded), in the every-tile sweep, fill value,
# inner (sharded rows: the transposed chunks are inner chunks of this shape, `chunk` is the shard)
Row = namedtuple("Row", "id chunk order dtype endian crc grid decode encode sweep fill inner",
                 defaults=(False, 3, None))

T2W, T4, TG2W, TG, TGEN = "k_decode_tile2w", "k_decode_tile4", "k_decode_tileg2w", "k_decode_tileg", "k_decode_tile"
E2, E4, EG, EGEN = "k_encode_tile2", "k_encode_tile4", "k_encode_tileg", "k_encode_tile"

# the seven (itemsize, swap) instantiations of for_item (csrc/zhip_dispatch.h)
SEVEN = [("u8", "uint8", LE), ("i16le", "int16", LE), ("i16be", "int16", BE), ("f32le", "float32", LE),
         ("f32be", "float32", BE), ("f64le", "float64", LE), ("f64be", "float64", BE)]

# rank 2, order (1, 0), tile4 family with a checksum: stored (b, a) for a chunk (a, b); row bytes a * itemsize.
# Four column blocks of one 1 KiB row (step 256 B, T = 8), one column block (step 64 rows, T = 4), sixteen (T = 16)
_R2_TILE4 = {"u8": (1024, 128), "i16le": (512, 128), "i16be": (128, 256), "f32le": (256, 128), "f32be": (64, 256),
             "f64le": (512, 64), "f64be": (128, 128)}
# rank 4, general: stored (r, 3, 5, n) -- tq 0, other dims 3 and 5 (no group dim), r < 64 rows: T = 15 n_cb.  The
# sizes keep the row bytes and a chunk's out offset along the contiguous dim multiples of 16
_R4_GEN = {1: (3, 5, 48, 48), 2: (3, 5, 40, 24), 4: (3, 5, 40, 20), 8: (3, 5, 40, 20)}

ROWS = (
    [Row("r2_tile4-" + k, _R2_TILE4[k], (1, 0), dt, en, True, (2, 2), T2W, E2, True,
         np.nan if k == "f32le" else 3) for k, dt, en in SEVEN] +
    [
        Row("r2_tile4_nocrc", (256, 128), (1, 0), "float32", LE, False, (2, 2), T4, E4),
        # stored (80, 100): two row blocks (64 + 16 rows), two column blocks (256 + 144 B): T = 4
        Row("r2_gen_partial", (100, 80), (1, 0), "float32", LE, True, (2, 3), TGEN, EGEN, True, np.nan),
        # stored (256, 64): 64-row tiles of 128-byte rows (row_bytes % 256 != 0), T = 4
        Row("r2_gen_128B", (64, 256), (1, 0), "int16", BE, True, (2, 2), TGEN, EGEN, True),
        # stored (128, 128): full tiles, two column blocks -- tiles 1 -> 2 step back to the next row block, no
        # uniform step, and rank 2 has no group dim: T = 4
        Row("r2_gen_full", (128, 128), (1, 0), "float32", LE, True, (2, 2), TGEN, EGEN, True),
        # ---- rank 4
        # stored (64, 3, 4, 64): tq 0, other dims 3 and 4, step 256 B along the 4: T = 12
        Row("r4_tile4_tq0", (4, 3, 64, 64), (3, 1, 0, 2), "float32", LE, True, (2, 2, 1, 1), T2W, E2, True),
        # stored (3, 64, 4, 64): tq 1 (a middle position)
        Row("r4_tile4_tq1", (3, 4, 64, 64), (0, 3, 1, 2), "float32", BE, True, (2, 1, 1, 2), T2W, E2, True),
        Row("r4_tile4_nocrc", (4, 3, 64, 64), (3, 1, 0, 2), "float32", LE, False, (2, 2, 1, 1), T4, E4),
        # stored (3, 24, 4, 40): tq 1, gd 2, 80-byte rows: T = 12 in 3 groups (6 workgroups: the one-word arrival)
        Row("r4_tileg", (4, 3, 40, 24), (1, 3, 0, 2), "int16", LE, True, (2, 2, 1, 2), TG2W, EG, True),
        Row("r4_tileg_nocrc", (4, 3, 40, 24), (1, 3, 0, 2), "int16", BE, False, (2, 2, 1, 2), TG, EG),
        # stored (24, 4, 1, 40): an other dim of size 1 inside the chain; gd 1
        Row("r4_tileg_one", (4, 1, 40, 24), (3, 0, 1, 2), "float64", LE, True, (2, 2, 1, 1), TG2W, EG, True),
        # stored (16, 36, 16, 16) bytes: tq 0, gd 2, tiles of 16 rows by 16 bytes: T = 576 in 144 groups -- 288
        # workgroups of two tiles, more than 256: the decode's XOR-then-count arrival (the encode's 144 groups of
        # four: its two-level words).  Fourteen chunks keep the every-tile sweep at 45 rounds
        Row("r4_tileg_count", (36, 16, 16, 16), (3, 0, 1, 2), "uint8", LE, True, (7, 2, 1, 1), TG2W, EG, True),
    ] +
    [Row("r4_gen-" + k, _R4_GEN[np.dtype(dt).itemsize], (3, 0, 1, 2), dt, en, True, (2, 1, 1, 2), TGEN, EGEN,
         True, np.nan if k == "f64le" else 3) for k, dt, en in SEVEN] +
    [
        # stored (5, 3, 36, 48): tq 2 = ndim - 2, other dims 5 and 3, 192-byte rows: T = 15
        Row("r4_gen_tqlast", (5, 3, 48, 36), (0, 1, 3, 2), "float32", LE, True, (2, 2, 1, 1), TGEN, EGEN, True),
        # stored (20, 3, 1, 40): general with an other dim of size 1
        Row("r4_gen_one", (3, 1, 40, 20), (3, 0, 1, 2), "float32", LE, True, (2, 3, 1, 1), TGEN, EGEN, True),
        # ---- rank 5
        # stored (64, 3, 2, 2, 64): tq 0, other dims 3, 2, 2; a group of four spans the last two: T = 12
        Row("r5_tile4", (2, 3, 2, 64, 64), (4, 1, 0, 2, 3), "float32", LE, True, (2, 1, 2, 1, 1), T2W, E2, True),
        # stored (4, 24, 2, 3, 40): tq 1, gd 0 (the OUTERMOST stored dim: the group stride spans the other two),
        # 320-byte rows: T = 48 in 12 groups, 24 workgroups of two tiles: the two-level arrival words
        Row("r5_tileg", (2, 3, 4, 40, 24), (2, 4, 0, 1, 3), "float64", LE, True, (2, 1, 1, 1, 2), TG2W, EG, True),
        # stored (3, 20, 5, 3, 24): tq 1, three other dims 3, 5, 3: T = 45
        Row("r5_gen", (3, 5, 3, 24, 20), (0, 4, 1, 2, 3), "float32", BE, True, (2, 1, 1, 1, 2), TGEN, EGEN, True),
        # ---- F-order out, no transpose codec: stored = the chunk, out dim 0 contiguous -> tq 0, gd 2: T = 12
        Row("r4_forder", (24, 3, 4, 20), None, "float64", LE, True, (2, 1, 1, 2), TG2W, None, True),
        # ---- transposed inner chunks of a shard (the decode name only by its prefix)
        Row("r2_sharded", (256, 256), (1, 0), "float32", LE, True, (2, 2), "k_decode_tile", None, False, 3,
            (256, 128)),
        Row("r4_sharded", (8, 3, 40, 48), (1, 3, 0, 2), "int16", BE, True, (1, 2, 2, 1), "k_decode_tile", None,
            False, 3, (4, 3, 40, 24)),
    ]
)

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# ragged arrays for the prefix-box encode (k_encode_tile under DF_TILE_PREFIX): id, array shape, chunk, order,
# dtype, endian, fill, write_empty_chunks.  The 4-D and 5-D arrays are ragged along the decoded dims that are
# stored as tq, as the innermost stored dim and as TWO other stored dims: the corner chunk is cut in four dims
Ragged = namedtuple("Ragged", "id shape chunk order dtype endian fill write_empty")
RAGGED = [
    Ragged("rag2", (150, 200), (100, 80), (1, 0), "float32", LE, 0.0, False),
    # stored (20, 3, 5, 40): tq <- dim 3, innermost <- dim 2, others <- dims 0 and 1
    Ragged("rag4_nan", (5, 8, 72, 28), (3, 5, 40, 20), (3, 0, 1, 2), "float32", BE, np.nan, False),
    # tile4 layout (stored (64, 3, 4, 64)): whole chunks take k_encode_tile too once one chunk is a prefix box
    Ragged("rag4_tile4_empty", (6, 5, 100, 96), (4, 3, 64, 64), (3, 1, 0, 2), "float32", LE, 0.0, True),
    # stored (3, 20, 5, 3, 24): tq <- dim 4, innermost <- dim 3, others <- dims 0, 1, 2 (dims 0 and 2 ragged)
    Ragged("rag5", (4, 5, 5, 40, 28), (3, 5, 3, 24, 20), (0, 4, 1, 2, 3), "float64", LE, 0.0, False),
]


# ------------------------------------------------------------------ geometry
def c_strides(shape, itemsize):
    """Byte strides of a C-order array."""
    st, acc = [], itemsize
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return tuple(reversed(st))


def f_strides(shape, itemsize):
    st, acc = [], itemsize
    for s in shape:
        st.append(acc)
        acc *= s
    return tuple(st)


def tile_chunk(row):
    """The chunk the tile kernels see: the inner chunk of a sharded row."""
    return row.inner if row.inner is not None else row.chunk


def array_shape(row):
    return tuple(c * g for c, g in zip(row.chunk, row.grid))


def stored_geometry(row, array=None):
    """(stored shape, itemsize, out byte strides per stored dim) of a row's
    chunk read into a whole-array out (C order; F order when row.order is None)."""
    it = np.dtype(row.dtype).itemsize
    array = array_shape(row) if array is None else array
    chunk = tile_chunk(row)
    if row.order is None:
        return tuple(chunk), it, f_strides(array, it)
    ost = c_strides(array, it)
    return tuple(chunk[p] for p in row.order), it, tuple(ost[p] for p in row.order)


Tile = namedtuple("Tile", "coords qb cb s_off o_off rows cols")


def find_tq(shape, itemsize, ostride):
    for d in range(len(shape) - 1):
        if ostride[d] == itemsize and shape[d] > 1:
            return d
    raise ValueError("no stored dim other than the last is contiguous in out")


def tiles(shape, itemsize, ostride):
    """Every tile of a stored chunk, in the order (other coords in C order, row
    block, column block) with the column block fastest: the byte offset of the
    tile's first element in the stored chunk (s_off) and in out relative to the
    chunk's origin (o_off: np.unravel_index in the stored shape dotted with the
    out strides), and its extents in rows of tq and in bytes of the stored row."""
    nd = len(shape)
    tq = find_tq(shape, itemsize, ostride)
    row_bytes = shape[-1] * itemsize
    assert row_bytes % 16 == 0
    others = [d for d in range(nd - 1) if d != tq]
    n_qb = -(-shape[tq] // TILE_ROWS)
    n_cb = -(-row_bytes // TILE_COLS)
    out = []
    for coords in np.ndindex(*[shape[d] for d in others]):
        for qb in range(n_qb):
            for cb in range(n_cb):
                idx = [0] * nd
                for d, c in zip(others, coords):
                    idx[d] = c
                idx[tq] = qb * TILE_ROWS
                idx[-1] = cb * TILE_COLS // itemsize
                elem = int(np.ravel_multi_index(idx, shape))
                back = np.unravel_index(elem, shape)
                o_off = int(sum(int(b) * int(o) for b, o in zip(back, ostride)))
                out.append(Tile(tuple(int(c) for c in coords), qb, cb, elem * itemsize, o_off,
                                min(TILE_ROWS, shape[tq] - qb * TILE_ROWS),
                                min(TILE_COLS, row_bytes - cb * TILE_COLS)))
    return out


def group_dim(shape, itemsize, ostride):
    """gd: the innermost other stored dim (not the last) with shape % 4 == 0, or None."""
    tq = find_tq(shape, itemsize, ostride)
    for d in range(len(shape) - 2, -1, -1):
        if d != tq and shape[d] % 4 == 0:
            return d
    return None


def tile4_uniform(ts):
    """Every aligned group of four consecutive tiles sits at one uniform step."""
    if len(ts) < 4 or len(ts) % 4 or ts[1].s_off <= ts[0].s_off:
        return False
    step = ts[1].s_off - ts[0].s_off
    return all(t.s_off == ts[i & ~3].s_off + (i & 3) * step for i, t in enumerate(ts))


def family(shape, itemsize, ostride):
    """"tile4" / "grouped" / "general" by the rules of the module docstring."""
    tq = find_tq(shape, itemsize, ostride)
    ts = tiles(shape, itemsize, ostride)
    full = shape[tq] % TILE_ROWS == 0 and (shape[-1] * itemsize) % TILE_COLS == 0
    if full and tile4_uniform(ts):
        return "tile4"
    if group_dim(shape, itemsize, ostride) is not None and shape[tq] % (16 // itemsize) == 0:
        return "grouped"
    return "general"


FAMILY_OF = {T2W: "tile4", T4: "tile4", TG2W: "grouped", TG: "grouped", TGEN: "general"}


# -------------------------------------------- x^(8 n) mod P, for the unit constants
_POLY, _ONE = 0x82F63B78, 0x80000000  # CRC-32C reflected; bit 31 is x^0


def gf_mul(a, b):
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (_POLY if b & 1 else 0)
    return p


def xpow8(n):
    """x^(8 n) mod P: the CRC register advanced over n zero bytes."""
    p, b = _ONE, _ONE >> 8
    while n:
        if n & 1:
            p = gf_mul(p, b)
        b = gf_mul(b, b)
        n >>= 1
    return p
