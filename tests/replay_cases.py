"""Replays of ONE prepared encode: the table of rows behind
tests/test_replay_rules.py (CPU) and tests/test_gpu_encode_replay.py (GPU),
the sources each replay encodes, and what every replay must leave behind,
restated from the oracle alone.  Nothing here calls the library.

The product path builds a fresh launch, a fresh zeroed workspace and fresh
flags for every write, so what a SECOND launch of the same object over another
source can get wrong is invisible to every write test: an arrival word, a
ticket or a non-empty bit that the first launch did not take back, a flag that
is ORed but not zeroed, a trailer or a status that is not rewritten.  Each of
the eight encode kernels has its own arrival / flag protocol (csrc/encode.hip,
csrc/decode_tile.hip, csrc/zhip_arrival.h); the table has one row per protocol,
at the smallest layout that reaches it, and names the kernel the row must take
(the rules of launch_encode, csrc/encode.hip, as tests/test_gpu_kernel_matrix.py
and tests/tile_cases.py state them):

  k_encode        XOR word + fetch_add ticket of run_len, exchanged back to 0;
                  flags ORed after the library's own zeroing
  k_encode_quad   the workgroup owns four chunks: no workspace, no atomics
  k_encode_il     per half of <= 16 workgroups one 64-bit word CRC | arrival
                  bits | non-empty bits; more than 16 workgroups: a third word
  k_encode_pair   even nseg <= 32: the same word per chunk, one bit per pair;
                  otherwise flags ORed after the library's zeroing, the CRC by
                  the mask word (nseg <= 32) or XOR + ticket (nseg > 32)
  k_encode_tile2 / k_encode_tile4   half words + third word, as k_encode_il
  k_encode_tileg  <= 16 groups: one word; <= 256: words of 16 in the workspace
                  tail, then the chunk word
  k_encode_tile   XOR word + ticket whose high 16 bits count non-empty arrivals

Every protocol's completing arrival stores zero back into every word it used,
and k_encode_quad and the layouts without a checksum under k_encode /
k_encode_pair's OR path never touch the workspace: after EVERY launch of EVERY
row the whole workspace is zero (Row.ws is the reason, per row).

Phases.  A row's source is overwritten in place between launches of the same
object.  With the chunks in C order of the chunk grid:
  A   chunk 0 all fill; chunk 1 fill except its first element; chunk 2 fill
      except its last element (of its box inside the array: an edge chunk's
      last selected element); the rest random bytes
  B   the roles move on by two chunks and the single elements change ends
      (chunk 2 all fill, chunk 3 fill except its LAST element, chunk 4 except
      its FIRST), chunks 0 and 1 now hold data, all data new
  F   every element fill
  A   again, bit for bit
The single differing element is the fill with its lowest bit flipped for
integers, -0.0 for floats with a number as fill (bitwise != 0.0: not empty)
and a second NaN payload where the fill is NaN (NDBuffer.all_equal: still
EMPTY, though the bytes differ) -- the oracle decides, not this table."""

from collections import namedtuple

import numpy as np

import dtype_cases as DC
import persist_cases as PC
import tile_cases as TC
from oracle import oracle as O

LE, BE = TC.LE, TC.BE
CRC = {"name": "crc32c"}
UNIT = PC.UNIT
nseg_of = PC.nseg_of  # units of a chunk of n decoded bytes

# what a row's protocol leaves in the workspace
WS_UNUSED = "the kernel never touches the workspace"
WS_RESET = "the completing arrival of every chunk stores zero into every word it used"

# family: what plan_encode must choose ("persist": neither rows nor a tile mode; "rows"; "tile"; "tile_prefix").
# arrivals: workgroups (persistent: units) that meet on one chunk's words, by the restatement in arrivals().
Row = namedtuple("Row", "id proto shape chunk dtype endian crc order fill kernel family arrivals ws")


def _r(id, proto, chunk, grid, dtype, endian, crc, kernel, family, arrivals, order=None, fill=0, shape=None,
       ws=WS_RESET):
    shape = tuple(shape) if shape is not None else tuple(c * g for c, g in zip(chunk, grid))
    return Row(id, proto, shape, tuple(chunk), dtype, endian, crc, order, fill, kernel, family, arrivals, ws)


def _last(chunk, n=5):
    """n chunks along the last dim (test_gpu_kernel_matrix.test_encode_row)."""
    return (1,) * (len(chunk) - 1) + (n,)


K, KQ, KIL, KP = "k_encode", "k_encode_quad", "k_encode_il", "k_encode_pair"
E2, E4, EG, EGEN = TC.E2, TC.E4, TC.EG, TC.EGEN

ROWS = [
    # ---- k_encode
    # 8 KiB chunks, one unit each; the array is ragged in the last two dims: edge chunks are prefix boxes
    _r("persist_edge", "k_encode, one unit per chunk, edge chunks", (16, 16, 8), None, "float32", LE, True, K,
       "persist", 1, fill=0.0, shape=(40, 33, 20)),
    # persist_cases "generic-u16le": 71 610 B, three units with a ragged head: the ticket counts to 3
    _r("persist_nseg3", "k_encode, the counted ticket", (35, 33, 31), _last((35, 33, 31)), "uint16", LE, True, K,
       "persist", 3, fill=3),
    # persist_cases "generic-f64be-35": 35 units, the ticket past 32
    _r("persist_nseg35", "k_encode, the counted ticket", (33, 100, 43), _last((33, 100, 43)), "float64", BE, True, K,
       "persist", 35, fill=0.0),
    # without a checksum: the status from the unit that ends the chunk, nothing in the workspace
    _r("persist_nocrc", "k_encode, no checksum", (35, 33, 31), _last((35, 33, 31)), "uint16", BE, False, K,
       "persist", 3, ws=WS_UNUSED),
    # test_gpu_persistent_ranges row (a): 30-byte chunks, more than twice as many as workgroups can be
    # resident (8 per CU, 256 CUs), so every range holds several chunks: the `parity` double buffer
    _r("persist_resident", "k_encode, ranges of several chunks", (3, 5), (66, 64), "int16", BE, True, K,
       "persist", 1, fill=7),
    # ---- k_encode_quad
    # test_gpu_encode.QUAD_CASES[1]: 12 KiB, NaN fill, an empty head step
    _r("quad_nan", "k_encode_quad", (3, 16, 64), (16, 2, 1), "float32", LE, True, KQ, "rows", 1, fill=np.nan,
       ws=WS_UNUSED),
    # QUAD_CASES[3]: 4 KiB, no checksum, six chunks: the second workgroup holds a partial quad
    _r("quad_nocrc", "k_encode_quad", (16, 128), (6, 1), "int16", BE, False, KQ, "rows", 1, ws=WS_UNUSED),
    # ---- k_encode_il (test_gpu_kernel_matrix.ENCODE_ROWS)
    _r("enc_il_s16", "k_encode_il, one half", (64, 64, 128), _last((64, 64, 128)), "uint8", LE, True, KIL, "rows", 16),
    _r("enc_il_g3", "k_encode_il, two-level word", (48, 64, 64), _last((48, 64, 64)), "float32", BE, True, KIL,
       "rows", 24, fill=0.0),
    _r("enc_il_ragged32", "k_encode_il, ragged head, S = 32", (250, 32, 32), _last((250, 32, 32)), "float32", LE,
       True, KIL, "rows", 32, fill=0.0),
    # ---- k_encode_pair, the pair word (an even number of units, at most 32)
    _r("enc_pair_w2", "k_encode_pair, pair word", (4, 64, 64), _last((4, 64, 64)), "float32", LE, True, KP, "rows", 2,
       fill=0.0),                                                                       # 64 KiB: one pair
    _r("enc_pair_w6", "k_encode_pair, pair word", (12, 64, 64), _last((12, 64, 64)), "int32", BE, True, KP, "rows",
       6),                                                                              # 192 KiB: three pairs
    _r("enc_pair_w8_nocrc", "k_encode_pair, pair word", (16, 64, 64), _last((16, 64, 64)), "float32", LE, False, KP,
       "rows", 8, fill=0.0),                                                            # 256 KiB: il needs a checksum
    # ---- k_encode_pair, flags ORed after the library's zeroing (odd nseg, or nseg > 32)
    _r("enc_pair_33", "k_encode_pair, OR path", (33, 64, 256), _last((33, 64, 256)), "int16", BE, True, KP, "rows", 33),
    _r("enc_pair_64", "k_encode_pair, OR path", (128, 64, 64), _last((128, 64, 64)), "float32", LE, True, KP, "rows",
       64, fill=0.0),
    _r("enc_pair_3r", "k_encode_pair, OR path", (23, 32, 16), _last((23, 32, 16)), "float64", LE, True, KP, "rows", 3,
       fill=0.0),
    # ---- k_encode_tile2 (tile_cases rows; the grids grown to at least five chunks)
    _r("r2_tile4-f32le", "k_encode_tile2", (256, 128), (3, 2), "float32", LE, True, E2, "tile", 4, order=(1, 0),
       fill=np.nan),
    _r("r4_tile4_tq1", "k_encode_tile2", (3, 4, 64, 64), (3, 1, 1, 2), "float32", BE, True, E2, "tile", 6,
       order=(0, 3, 1, 2), fill=3),
    # the flagship's transposed encode: 64 tiles per chunk, 32 workgroups: halves of 16 and the third word
    _r("tile2_third", "k_encode_tile2, third word", (64, 64, 64), _last((64, 64, 64)), "float32", LE, True, E2, "tile",
       32, order=(2, 1, 0), fill=0.0),
    # ---- k_encode_tile4
    _r("r2_tile4_nocrc", "k_encode_tile4", (256, 128), (3, 2), "float32", LE, False, E4, "tile", 2, order=(1, 0),
       fill=3),
    # ---- k_encode_tileg
    _r("r4_tileg", "k_encode_tileg, one-word arrival", (4, 3, 40, 24), (2, 2, 1, 2), "int16", LE, True, EG, "tile", 3,
       order=(1, 3, 0, 2), fill=3),
    _r("r4_tileg_count", "k_encode_tileg, two-level arrival", (36, 16, 16, 16), (7, 2, 1, 1), "uint8", LE, True, EG,
       "tile", 144, order=(3, 0, 1, 2), fill=3),
    _r("r5_tileg", "k_encode_tileg, one-word arrival", (2, 3, 4, 40, 24), (3, 1, 1, 1, 2), "float64", LE, True, EG,
       "tile", 12, order=(2, 4, 0, 1, 3), fill=3),
    _r("r4_tileg_nocrc", "k_encode_tileg, no checksum", (4, 3, 40, 24), (2, 2, 1, 2), "int16", BE, False, EG, "tile",
       3, order=(1, 3, 0, 2), fill=3),
    # ---- k_encode_tile
    _r("r2_gen_partial", "k_encode_tile", (100, 80), (2, 3), "float32", LE, True, EGEN, "tile", 1, order=(1, 0),
       fill=np.nan),
    _r("r4_gen-f64le", "k_encode_tile", (3, 5, 40, 20), (3, 1, 1, 2), "float64", LE, True, EGEN, "tile", 8,
       order=(3, 0, 1, 2), fill=np.nan),                            # 320-byte rows: 30 tiles, the last group of two
    # tile_cases.RAGGED "rag4_nan": the corner chunk is cut in all four dims (ZHIP_DF_TILE_PREFIX)
    _r("rag4_nan", "k_encode_tile, prefix boxes", (3, 5, 40, 20), None, "float32", BE, True, EGEN, "tile_prefix", 4,
       order=(3, 0, 1, 2), fill=np.nan, shape=(5, 8, 72, 28)),
]

BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# every arrival / flag protocol of the table this module's docstring names
PROTOCOLS = sorted({r.proto for r in ROWS})

# the rows of the two-launches-one-plan test: il, pair (OR path), tileg, persistent
TWO_LAUNCH = ("enc_il_s16", "enc_pair_3r", "r4_tileg", "persist_nseg3")

# a persistent launch runs at most 8 workgroups per CU (csrc/capi.cpp), 256 CUs
RESIDENT_BOUND = 8 * 256


def codecs(row):
    tr = [{"name": "transpose", "configuration": {"order": list(row.order)}}] if row.order is not None else []
    return tr + [row.endian] + ([CRC] if row.crc else [])


def fill_of(row):
    return np.asarray(row.fill, np.dtype(row.dtype))[()]


def nbytes(row):
    return int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize


def elen(row):
    return nbytes(row) + (4 if row.crc else 0)


def tiles_per_chunk(row):
    t = TC.Row(row.id, row.chunk, row.order, row.dtype, row.endian, row.crc, None, None, None)
    return len(TC.tiles(*TC.stored_geometry(t, row.shape)))


def arrivals(row):
    """Workgroups (persistent kernel: units) that arrive on one chunk, from the
    kernel's name and the geometry alone."""
    if row.kernel in (K, KIL, KP):
        return nseg_of(nbytes(row))
    if row.kernel == KQ:
        return 1
    T = tiles_per_chunk(row)
    return {E2: T // 2, E4: T // 4, EG: T // 4, EGEN: -(-T // 4)}[row.kernel]


def rows_kernel(row):
    """launch_encode_rows restated: which row-mapped kernel a whole-row layout takes."""
    n, nseg = nbytes(row), nseg_of(nbytes(row))
    if nseg == 1 and n <= UNIT // 2:
        return KQ
    if row.crc and nseg % 8 == 0 and nseg <= 32:
        return KIL
    return KP


def boxes(row):
    """[(grid coords, origin in the array, extent inside the array)] of the chunks in C order."""
    grid = [-(-a // c) for a, c in zip(row.shape, row.chunk)]
    out = []
    for ix in np.ndindex(*grid):
        lo = tuple(i * c for i, c in zip(ix, row.chunk))
        out.append((ix, lo, tuple(min(c, a - o) for c, a, o in zip(row.chunk, row.shape, lo))))
    return out


def n_chunks(row):
    return len(boxes(row))


# ------------------------------------------------------------------- phases
PHASES = ("A", "B", "F", "A")
_SEED = {"A": 11, "B": 12, "F": 13}
_SHIFT = {"A": 0, "B": 2}


def other_of(row):
    """The one element of a single-element chunk."""
    dt = np.dtype(row.dtype)
    fill = fill_of(row)
    if dt.kind == "f":
        # dtype_cases' patterns: a NaN with the sign set and payload 1; -0.0
        return DC._fbits(dt, DC._SNAN_NEG[dt.itemsize] if np.isnan(fill) else DC._NEG0[dt.itemsize])
    return (np.array([fill]).view(f"u{dt.itemsize}") ^ 1).view(dt)[0]


def roles(row, phase):
    """Per chunk: "fill", "first", "last" or "data"."""
    n = n_chunks(row)
    assert n >= 5
    if phase == "F":
        return ["fill"] * n
    s = _SHIFT[phase]
    out = ["data"] * n
    out[s % n] = "fill"
    out[(s + 1) % n], out[(s + 2) % n] = ("first", "last") if phase == "A" else ("last", "first")
    return out


_SOURCES = {}


def source(row, phase):
    """The whole source array of a phase (read-only, made once)."""
    hit = _SOURCES.get((row.id, phase))
    if hit is not None:
        return hit
    dt = np.dtype(row.dtype)
    rng = np.random.default_rng(_SEED[phase])
    a = rng.integers(0, 256, size=int(np.prod(row.shape)) * dt.itemsize, dtype=np.uint8).view(dt).reshape(row.shape)
    fill, other = fill_of(row), other_of(row)
    for (_, lo, n), role in zip(boxes(row), roles(row, phase)):
        if role == "data":
            continue
        a[tuple(slice(o, o + k) for o, k in zip(lo, n))] = fill
        if role == "first":
            a[lo] = other
        elif role == "last":
            a[tuple(o + k - 1 for o, k in zip(lo, n))] = other
    a.setflags(write=False)
    _SOURCES[(row.id, phase)] = a
    return a


Want = namedtuple("Want", "blob empty crc")  # encoded bytes; all_equal(chunk, fill); the trailer as a number, or None
_EXPECTED = {}


def expected(row, phase):
    """[Want] per chunk, from the oracle alone: the chunk as _merge_chunk_array
    leaves it (outside the array = fill), O.chain_encode'd (an all-fill chunk
    is still encoded), with O.all_equal's verdict and the CRC read back from
    the blob's last four bytes."""
    hit = _EXPECTED.get((row.id, phase))
    if hit is not None:
        return hit
    dt = np.dtype(row.dtype)
    chain = O.Chain.from_json(codecs(row))
    spec = O.Spec(row.chunk, dt, fill_of(row))
    src = source(row, phase)
    fill = np.asarray(fill_of(row), dt)
    out = []
    for _, lo, n in boxes(row):
        chunk = np.empty(row.chunk, dt)
        chunk[...] = fill
        chunk[tuple(slice(0, k) for k in n)] = src[tuple(slice(o, o + k) for o, k in zip(lo, n))]
        blob = np.asarray(O.chain_encode(chunk, chain, spec)).view(np.uint8).reshape(-1).copy()
        assert len(blob) == elen(row)
        crc = int.from_bytes(blob[-4:].tobytes(), "little") if row.crc else None
        out.append(Want(blob, bool(O.all_equal(chunk, fill)), crc))
    _EXPECTED[(row.id, phase)] = out
    return out


# ------------------------------------------------------------ the destination
SENTINEL = 0xA5
SLOT_ALIGN = 256
GUARD = 256


def slots(row):
    """(offsets of the chunk slots, total bytes) of the destination: slots of
    elen bytes at 256-byte aligned offsets, at least GUARD sentinel bytes
    before the first, between any two and after the last."""
    stride = -(-elen(row) // SLOT_ALIGN) * SLOT_ALIGN + GUARD
    n = n_chunks(row)
    return [GUARD + i * stride for i in range(n)], GUARD + n * stride


def image(row, phase):
    """The destination after a launch over `phase`: sentinel everywhere but the slots."""
    offs, total = slots(row)
    img = np.full(total, SENTINEL, np.uint8)
    for off, w in zip(offs, expected(row, phase)):
        img[off: off + len(w.blob)] = w.blob
    return img
