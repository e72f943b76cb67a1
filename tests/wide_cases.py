"""Byte offsets beyond 2**31 and 2**32 in every kernel family: the table of
rows behind tests/test_wide_offsets.py (CPU) and tests/test_gpu_wide_offsets.py
(GPU), and a restatement of every address a row makes the kernels form, in
plain numpy and Python integers, which calls nothing of the library.

Every kernel forms an address as a 64-bit base plus narrower parts (the
chunk's out_off and src, a step's rel, a lane's offset, a tile's orel).  A row
takes an EXISTING geometry -- the smallest that reaches its kernel, from
test_gpu_kernel_matrix.DECODE_ROWS / ENCODE_ROWS, tile_cases, persist_cases,
test_gpu_fused_launch and test_gpu_decode.DEFAULT_SHARD_CASES (`of` names the
source row) -- and changes only WHERE its chunks lie:

  out / value side: the tensor handed to prepare_read(out=) or set() is a
  torch.as_strided view into one large uint8 backing.  Only the dimension that
  carries the chunk grid gets a huge stride; the interior of a chunk keeps the
  contiguous strides of the original, so the planner's fast / rows / tile
  verdicts and the kernel choice stay what they were.
    slab    a leading array dimension of chunk extent 1 carries the grid:
            chunk (c0, c1, c2) becomes array (n, c0, c1, c2) in chunks
            (1, c0, c1, c2), dimension-0 stride P.  n is even, chunk n - 2
            starts h = nbytes / 2 (3/4 of a shard) below 2**32 and chunk
            (n - 2) / 2 therefore h / 2 below 2**31: P = (2**32 - h) / (n - 2),
            rounded down to a multiple of 16 (which moves those starts down by
            less than 16 (n - 2) bytes).  Chunk n - 1 lies wholly above 2**32 and
            is the one missing from the store (reads) or all fill (writes).
    near    (64, 64, 64) float32, the grid along dimension 1 -- array
            (64, 64 n, 64), so the chunks' footprints interleave -- and
            dimension-0 stride S0 = NEAR_S0: the largest for which the row map
            exists; its largest rel is 63 S0 + 48 * 256 = 2**31 - 944.
    past    the same with S0 = NEAR_S0 + 16: no row map.
    plane   (4, 64, 64) float32, S0 = 2**30: planes at 0, 2**30, 2**31, 2**32.
    planes  chunk (4, ...), the grid along dimension 1, S0 = (2**32 - d) / 3
            with d a quarter of a chunk's plane: plane 3 of chunk 0 straddles
            2**32, the other chunks' lie above.  For the rank-4 tile rows the
            per-tile out offsets (orel) of planes 2 and 3 pass 2**31; for the
            plane geometry it is the wide-plane row with stores beyond 2**32.

  arena side: the store's arena is a view of a second backing; pad regions are
  reserved so that blob 0 lies at 0, blob 1 straddles 2**31, blob 2 straddles
  2**32 (half on either side, to the placement granule) and the rest follow
  above.  For sharded rows these are shard blobs.

Both backings are [FRONT guard | BODY | BACK guard] with the view (and the
arena's buf) starting at the end of the front guard: offset 0 below is the
first byte of the body.  `narrowed_dest` / `narrowed_src` list, for every
address, every way a correct 64-bit sum can lose its high bits -- so the CPU
test can prove that each lands inside [-FRONT, BODY + BACK) and a truncation on
the device shows as wrong bytes, never as an access outside the allocation."""

from collections import namedtuple

import numpy as np

import tile_cases as TC

LE, BE = TC.LE, TC.BE
CRC = {"name": "crc32c"}

B31, B32 = 1 << 31, 1 << 32
FRONT = 1 << 31                 # sign-extended low words reach down to -2**31
BODY = B32 + 3 * (1 << 28)      # the widest row: eight 2 MiB slabs, the last at 7/6 of 2**32
BACK = 1 << 20
TOTAL = FRONT + BODY + BACK
SENTINEL = 0xA5
GRANULE = 256                   # the arena's placement granule
SLACK = 64                      # the kernels may read this far past a blob

NEAR_S0 = 34086832
PAST_S0 = NEAR_S0 + 16
PLANE_S0 = 1 << 30

SLAB, NEAR, PAST, PLANE, PLANES = "slab", "near", "past", "plane", "planes"

# id; of: the row this geometry is taken from; chunk (sharded rows: the inner chunk, `shard` the shard shape);
# dtype; endian; crc; n: chunks (shards) along the grid dimension; spread; kernel; transpose order of the ORIGINAL
# chunk (tile rows); shard; index location; fill; whole: the whole read runs under ZHIP_DF_WHOLE (affine rows:
# with the row map zeroed); rowmap: the launch has a row map; index: shard indexes checked in the data launch;
# pitch: a slab stride other than the rule's; base: where in the body the view starts (out_off stays relative to
# it); after: the row whose blobs precede this row's in the same arena
Row = namedtuple("Row", "id of chunk dtype endian crc n spread kernel order shard loc fill whole rowmap index "
                        "pitch base after", defaults=(None, None, "end", 3, False, True, False, None, 0, None))

READ_ROWS = [
    # ---- the row kernels (test_gpu_kernel_matrix.DECODE_ROWS)
    Row("il", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 18, SLAB, "k_decode_il", whole=True),
    Row("il_be", "il_s32-i16be", (64, 64, 128), "int16", BE, True, 18, SLAB, "k_decode_il", whole=True),
    Row("il_ragged", "il_ragged32", (250, 32, 32), "float32", LE, True, 18, SLAB, "k_decode_il"),
    Row("ilh", "ilh_u8", (64, 64, 256), "uint8", LE, True, 12, SLAB, "k_decode_ilh", whole=True),
    Row("ilw512", "ilw_w64-f32le", (512, 1024), "float32", LE, True, 8, SLAB, "k_decode_ilw512", whole=True),
    Row("duo", "duo_33-f32le", (33, 64, 128), "float32", LE, True, 12, SLAB, "k_decode_duo"),
    Row("pair", "pair_31r", (247, 32, 16), "float64", BE, True, 12, SLAB, "k_decode_pair"),
    # ---- sharded (test_gpu_fused_launch: 128^3 shards of 64^3; test_gpu_decode.DEFAULT_SHARD_CASES[0])
    Row("il_shard_end", "fused-launch sharded", (64, 64, 64), "float32", LE, True, 12, SLAB, "k_decode_il",
        shard=(128, 128, 128), index=True),
    Row("il_shard_start", "fused-launch sharded", (64, 64, 64), "float32", LE, True, 12, SLAB, "k_decode_il",
        shard=(128, 128, 128), loc="start", index=True),
    Row("lead", "DEFAULT_SHARD_CASES[0]", (32, 32, 32), "float32", LE, False, 12, SLAB, "k_decode_lead",
        shard=(64, 64, 64), fill=0, index=True),
    # ---- the persistent kernels (persist_cases.ROWS), shipped library: no grid cap
    Row("generic", "generic-u16le", (35, 33, 31), "uint16", LE, True, 12, SLAB, "k_decode", rowmap=False),
    Row("fast", "fast-f32", (40, 50, 12), "float32", LE, True, 12, SLAB, "k_decode", rowmap=False),
    Row("tile", "tile-r4_gen-f32le", (3, 5, 40, 20), "float32", LE, True, 12, SLAB, "k_decode_tile",
        order=(3, 0, 1, 2), rowmap=False),
    # ---- the tile kernels (tile_cases.ROWS)
    Row("tile2w_r2", "r2_tile4-f32le", (256, 128), "float32", LE, True, 12, SLAB, TC.T2W, order=(1, 0),
        rowmap=False),
    Row("tile2w", "r4_tile4_tq0", (4, 3, 64, 64), "float32", LE, True, 5, PLANES, TC.T2W, order=(3, 1, 0, 2),
        rowmap=False),
    Row("tile4", "r4_tile4_nocrc", (4, 3, 64, 64), "float32", LE, False, 5, PLANES, TC.T4, order=(3, 1, 0, 2),
        rowmap=False),
    Row("tileg2w", "r4_tileg", (4, 3, 40, 24), "int16", LE, True, 5, PLANES, TC.TG2W, order=(1, 3, 0, 2),
        rowmap=False),
    Row("tileg", "r4_tileg_nocrc", (4, 3, 40, 24), "int16", BE, False, 5, PLANES, TC.TG, order=(1, 3, 0, 2),
        rowmap=False),
    # ---- rel towards INT32_MAX, and past it
    Row("near_il", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 17, NEAR, "k_decode_il", whole=True),
    Row("near_ilh", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 4, NEAR, "k_decode_ilh", whole=True),
    Row("past", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 17, PAST, "k_decode_rows", rowmap=False),
    Row("plane", "rows_map_declines", (4, 64, 64), "float32", LE, True, 5, PLANE, "k_decode_rows", rowmap=False),
    Row("plane_hi", "rows_map_declines", (4, 64, 64), "float32", LE, True, 5, PLANES, "k_decode_rows",
        rowmap=False),
]
READ = {r.id: r for r in READ_ROWS}
assert len(READ) == len(READ_ROWS)

# The two programs of one fused launch (k_decode_il_multi): the il row's geometry twice, from one arena, into outs
# whose address ranges are disjoint (what lets them share a launch).  The low out is 18 slabs 64 MiB apart from
# the start of the body, wholly below 2**31; the high out starts 2**31 into the body with pitch
# (2**31 - nbytes / 2) / 16 = 2**27 - 2**15, so slab 16 starts nbytes / 2 below 2**32 and slab 17 lies above.  The
# low program's blobs take the usual placements; the high program's follow behind them, all above 2**32.
FUSED_ROWS = [
    Row("fused_lo", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 18, SLAB, "k_decode_il", whole=True,
        pitch=1 << 26),
    Row("fused_hi", "il_s32-f32le", (64, 64, 64), "float32", LE, True, 18, SLAB, "k_decode_il", whole=True,
        pitch=(B31 - (1 << 19)) // 16, base=B31, after="fused_lo"),
]
FUSED = {r.id: r for r in FUSED_ROWS}

# encode rows: the value is the same kind of view, its last chunk all fill (elided)
WRITE_ROWS = [
    Row("enc_il", "enc_il_s16", (64, 64, 128), "uint8", LE, True, 12, SLAB, "k_encode_il", fill=0),
    Row("enc_pair", "enc_pair_33", (33, 64, 256), "int16", BE, True, 12, SLAB, "k_encode_pair", fill=0),
    Row("enc", "generic-u16le", (35, 33, 31), "uint16", LE, True, 12, SLAB, "k_encode", fill=0),
    Row("enc_tile2", "r4_tile4_tq0", (4, 3, 64, 64), "float32", LE, True, 5, PLANES, TC.E2, order=(3, 1, 0, 2),
        fill=0),
    Row("enc_tile4", "r4_tile4_nocrc", (4, 3, 64, 64), "float32", LE, False, 5, PLANES, TC.E4,
        order=(3, 1, 0, 2), fill=0),
    Row("enc_tileg", "r4_tileg", (4, 3, 40, 24), "int16", LE, True, 5, PLANES, TC.EG, order=(1, 3, 0, 2), fill=0),
    # k_shard_pack moves the inner chunks inside the shard blobs (the encode kernel before it is k_encode_il)
    Row("enc_shard", "fused-launch sharded", (64, 64, 64), "float32", LE, True, 12, SLAB, "k_encode_il",
        shard=(128, 128, 128), fill=0),
]
WRITE = {r.id: r for r in WRITE_ROWS}
assert len(WRITE) == len(WRITE_ROWS)


# ------------------------------------------------------------------ geometry
def align(n):
    return -(-int(n) // GRANULE) * GRANULE


def itemsize(row):
    return np.dtype(row.dtype).itemsize


def outer(row):
    """The shape one store key covers: the shard, else the chunk."""
    return tuple(row.shard if row.shard is not None else row.chunk)


def nbytes(shape, row):
    return int(np.prod(shape, dtype=np.int64)) * itemsize(row)


def array_shape(row):
    o = outer(row)
    if row.spread == SLAB:
        return (row.n,) + o
    return (o[0], o[1] * row.n) + o[2:]


def array_chunks(row, shape=None):
    """The array's chunk shape for `shape` (default: what a store key covers)."""
    shape = outer(row) if shape is None else tuple(shape)
    return (1,) + shape if row.spread == SLAB else shape


def slab_half(row):
    """h: how far below 2**32 chunk n - 2 starts -- half a chunk; three
    quarters of a shard, so that 2**32 (and 2**31, at 3/8 of shard (n - 2) / 2)
    falls inside inner chunks and not between two."""
    return nbytes(outer(row), row) * (3 if row.shard is not None else 2) // 4


def grid_stride(row):
    """The huge stride, in bytes: P of a slab row, S0 of the others."""
    if row.pitch is not None:
        assert row.spread == SLAB and row.pitch % 16 == 0
        return row.pitch
    if row.spread == SLAB:
        assert row.n % 2 == 0 and row.n >= 4
        return (B32 - slab_half(row)) // (row.n - 2) // 16 * 16
    if row.spread == PLANES:
        o = outer(row)
        return (B32 - nbytes(o[1:], row) // 4) // (o[0] - 1) // 16 * 16
    return {NEAR: NEAR_S0, PAST: PAST_S0, PLANE: PLANE_S0}[row.spread]


def view_strides(row):
    """Byte strides of the view, per array dimension."""
    shape = array_shape(row)
    return (grid_stride(row),) + TC.c_strides(shape[1:], itemsize(row))


def origin(row, i):
    """Byte offset in the view (from its base) of the first element of grid cell i."""
    st = view_strides(row)
    return i * st[0] if row.spread == SLAB else i * outer(row)[1] * st[1]


def key(row, i):
    nd = len(array_shape(row))
    ix = [0] * nd
    ix[0 if row.spread == SLAB else 1] = i
    return "c/" + "/".join(str(x) for x in ix)


def dropped(row):
    """The grid cell missing from the store: the last, wholly above 2**32 in a slab."""
    return row.n - 1


def declined(row):
    """Whole-row layouts whose chunk spans more than 2 GiB of the view: no row map."""
    return row.spread in (PAST, PLANE) or (row.spread == PLANES and row.order is None)


def codecs(row):
    """The codec chain over the array's chunks (a slab's leading dimension
    stays in front of the transpose)."""
    chain = []
    if row.order is not None:
        chain.append({"name": "transpose", "configuration": {
            "order": [0] + [p + 1 for p in row.order] if row.spread == SLAB else list(row.order)}})
    chain.append(row.endian)
    if row.crc:
        chain.append(CRC)
    if row.shard is None:
        return chain
    return [{"name": "sharding_indexed", "configuration": {
        "chunk_shape": list(array_chunks(row, row.chunk)), "codecs": chain, "index_codecs": [LE, CRC],
        "index_location": row.loc}}]


def inner_grid(row):
    return tuple(s // c for s, c in zip(row.shard, row.chunk)) if row.shard is not None else ()


def index_size(row):
    return 16 * int(np.prod(inner_grid(row))) + 4


# ---------------------------------------------------------- destination side
def runs(shape, strides, isz):
    """The contiguous byte runs of a box of `shape` at byte `strides`:
    (int64 run starts relative to the box's first element, bytes per run)."""
    run, d = isz, len(shape)
    while d > 0 and (strides[d - 1] == run or shape[d - 1] == 1):
        run *= shape[d - 1]
        d -= 1
    starts = np.zeros(1, np.int64)
    for n, s in zip(shape[:d], strides[:d]):
        starts = (starts[:, None] + np.arange(n, dtype=np.int64)[None, :] * int(s)).reshape(-1)
    return starts, run


Dest = namedtuple("Dest", "cell inner out_off starts run")


def dest_chunks(row):
    """Every decoded chunk (inner chunk) of a whole read or write, grid cells in
    order and inner chunks in C order: the byte offset of its first element in
    the view (zhip_chunk.out_off) and its contiguous runs relative to that."""
    st = view_strides(row)
    interior = st[1:] if row.spread == SLAB else st
    starts, run = runs(row.chunk, interior, itemsize(row))
    out = []
    for i in range(row.n):
        if row.shard is None:
            out.append(Dest(i, None, origin(row, i), starts, run))
            continue
        for ix in np.ndindex(*inner_grid(row)):
            off = sum(int(a) * c * int(s) for a, c, s in zip(ix, row.chunk, interior))
            out.append(Dest(i, tuple(int(a) for a in ix), origin(row, i) + off, starts, run))
    return out


def dest_ranges(row):
    """[(first byte, end byte)] of every contiguous destination run, absolute in the body."""
    return [r for rs in chunk_ranges(row) for r in rs]


def chunk_ranges(row):
    """dest_ranges, one list per chunk of dest_chunks."""
    return [[(row.base + d.out_off + int(s), row.base + d.out_off + int(s) + d.run) for s in d.starts]
            for d in dest_chunks(row)]


def straddles(ranges, bound):
    """Some chunk's bytes lie on both sides of `bound`."""
    return min(a for a, _ in ranges) < bound < max(b for _, b in ranges)


def stored_tile_geometry(row):
    """tile_cases.stored_geometry for a wide tile row: (stored shape, itemsize,
    out byte strides per stored dim) of ONE chunk in the view (a slab's leading
    dimension of extent 1 left out: it adds nothing to any offset)."""
    st = view_strides(row)
    interior = st[1:] if row.spread == SLAB else st
    return (tuple(row.chunk[p] for p in row.order), itemsize(row), tuple(int(interior[p]) for p in row.order))


# --------------------------------------------------------------- source side
def blob_len(row):
    """Bytes of one store value: the chunk and its trailer, or the full shard
    (every inner chunk present) with its index."""
    one = nbytes(row.chunk, row) + (4 if row.crc else 0)
    if row.shard is None:
        return one
    return one * int(np.prod(inner_grid(row))) + index_size(row)


def placements(lengths):
    """Where blobs of `lengths` must sit, in store order: the first at 0, the
    second straddling 2**31, the third 2**32 (half on either side, to the
    granule), the rest behind it."""
    assert len(lengths) >= 3
    out = [0, B31 - align(lengths[1] // 2), B32 - align(lengths[2] // 2)]
    assert out[1] >= align(lengths[0]) and out[2] >= out[1] + align(lengths[1])
    for n in lengths[2:-1]:
        out.append(out[-1] + align(n))
    assert out[-1] + align(lengths[-1]) + SLACK <= BODY
    return out


def read_placements(row):
    """{grid cell: (arena offset, length)} of the present cells of a read row."""
    cells = [i for i in range(row.n) if i != dropped(row)]
    lens = [blob_len(row)] * len(cells)
    if row.after is not None:  # behind the other row's blobs, one after another
        top = max(o + align(n) for o, n in read_placements(FUSED[row.after]).values())
        offs = [top + k * align(n) for k, n in enumerate(lens)]
        assert offs[-1] + align(lens[-1]) + SLACK <= BODY
        return {c: (o, n) for c, o, n in zip(cells, offs, lens)}
    return {c: (o, n) for c, o, n in zip(cells, placements(lens), lens)}


def parse_index(row, blob):
    """The (offset, length) pairs of a shard blob's index, inner chunks in C
    order; (2**64 - 1, 2**64 - 1) marks a missing one."""
    n = int(np.prod(inner_grid(row)))
    raw = blob[:16 * n] if row.loc == "start" else blob[len(blob) - index_size(row): len(blob) - 4]
    return [(int(a), int(b)) for a, b in np.frombuffer(raw, "<u8").reshape(n, 2)]


def src_ranges(row, place, blobs=None):
    """[(cell, inner, first byte, end byte)] of every encoded chunk the kernels
    read, absolute in the arena, from the placements (and, sharded, the index
    inside each blob: `blobs` {cell: bytes}); inner is "index" for the index."""
    out = []
    for c, (off, n) in place.items():
        if row.shard is None:
            out.append((c, None, off, off + n))
            continue
        ipos = 0 if row.loc == "start" else n - index_size(row)
        out.append((c, "index", off + ipos, off + ipos + index_size(row)))
        for ix, (a, b) in zip(np.ndindex(*inner_grid(row)), parse_index(row, blobs[c])):
            if a != 2 ** 64 - 1:
                out.append((c, tuple(int(x) for x in ix), off + a, off + a + b))
    return out


def enc_len(row):
    """Bytes a write reserves per store key (what an encode may fill)."""
    return blob_len(row)


def write_top(row):
    """Where the arena's top must be before a whole write of the row: the
    writer reserves one region per key, in grid order, each the granule-aligned
    reservation behind the last; regions 0 and 1 then lie below 2**32, region 2
    straddles it and the rest lie above."""
    a = align(enc_len(row))
    return B32 - 2 * a - align(a // 2)


def write_regions(row):
    """{grid cell: arena offset of the region reserved for its key}."""
    return {c: write_top(row) + c * align(enc_len(row)) for c in range(row.n)}


# ---------------------------------------------------------------- narrowings
def narrow(x):
    """The ways a 64-bit offset loses its high bits: as it is, the low 32 bits,
    those sign-extended, the low 31 bits."""
    x = np.asarray(x, np.int64)
    lo = x & 0xFFFFFFFF
    return [x, lo, np.where(lo >= B31, lo - B32, lo), x & 0x7FFFFFFF]


def _span_points(first, run):
    """The 16-byte pieces of [first, first + run) at which a narrowing of the
    running sum can jump: both ends, and either side of a multiple of 2**31
    inside (a run is shorter than 2**31: at most one)."""
    first = np.asarray(first, np.int64)
    last = first + (run - 16)
    k = last // B31 * B31
    inside = k > first
    return [first, last, np.where(inside, k - 16, first), np.where(inside, k, first)]


def narrowed_dest(d):
    """Every address the 16-byte stores of chunk `d` can land at when any
    partial sum of out_off + rel + lane is narrowed (the lane part alone is
    below 2**13 and never narrows): arrays of first bytes, relative to the view."""
    out = []
    for s in _span_points(d.starts, d.run):      # s = rel + lane
        lane = s - d.starts
        for o in narrow(d.out_off):
            out.append(o + s)
        for x in narrow(d.out_off + d.starts):
            out.append(x + lane)
        for x in narrow(s):
            out.append(d.out_off + x)
        out += narrow(d.out_off + s)
    return out


def narrowed_src(first, end):
    """The same for the loads of [first, end + SLACK): src + k."""
    out = []
    for s in _span_points(np.array([0], np.int64), -(-(end - first + SLACK) // 16) * 16):
        out += [o + s for o in narrow(first)] + narrow(first + s)
    return out


def inside(addresses, base=0):
    """Every 16-byte access at `addresses` (relative to a pointer `base` bytes
    into the body) lies inside the backing."""
    return all(base + int(a.min()) >= -FRONT and base + int(a.max()) + 16 <= BODY + BACK for a in addresses)


# ----------------------------------------------------------------- value map
ValueRow = namedtuple("ValueRow", "item k a b count")
VALUE_STRIDE = B31 + 4096
VALUE_ODD = 1001


def value_vector_path(item, asz, bsz):
    """Whether k_value_map takes an item on its vector path (buffers aligned
    to 16 bytes): lanes take V elements at a time -- 16 bytes of the narrower
    side, at most 8 elements -- so the innermost dimension must be contiguous
    on both sides with a count that is a multiple of V, and every row start
    (the bases and the outer strides) a multiple of min(16, V * item size) on
    its side.  Otherwise every element is loaded and stored on its own."""
    a_base, b_base, dims = item[:3]
    narrow_sz = min(asz, bsz)
    V = 8 if narrow_sz == 1 else min(8, 16 // narrow_sz)
    count, sa, sb = dims[-1]
    if (sa, sb) != (asz, bsz) or count % V:
        return False
    al_a, al_b = min(16, V * asz), min(16, V * bsz)
    if a_base % al_a or b_base % al_b:
        return False
    return all(c <= 1 or (s_a % al_a == 0 and s_b % al_b == 0) for c, s_a, s_b in dims[:-1])


def value_items(asz, bsz):
    """Three items of one k_value_map launch over the two bodies, as
    [(a_base, b_base, [(count, sa, sb), ...], flags, status)] in bytes:
    bases at 2**32; an outer dimension of count 3 with sa = sb = 2**31 + 4096
    (row 2 lies past 2**32 by the product alone) -- both of 1001 elements per
    row, no multiple of the vector width, so they take the kernel's
    per-element path; eight contiguous, 16-byte aligned rows of 256 elements
    2**17 apart, four below and four above 2**32: the vector path."""
    rs = 1 << 17
    base = B32 - 4 * rs + (1 << 16)
    return [(B32, B32, [(VALUE_ODD, asz, bsz)], 0, 0),
            (0, 0, [(3, VALUE_STRIDE, VALUE_STRIDE), (VALUE_ODD, asz, bsz)], 0, 0),
            (base, base, [(8, rs, rs), (256, asz, bsz)], 0, 0)]


def value_rows(items):
    """The contiguous rows of `items`: where each starts on either side."""
    out = []
    for i, (a, b, dims, _, _) in enumerate(items):
        outer = dims[:-1] or [(1, 0, 0)]
        assert len(outer) == 1
        out += [ValueRow(i, k, a + k * outer[0][1], b + k * outer[0][2], dims[-1][0]) for k in range(outer[0][0])]
    return out


def narrowed_value(base, k, stride, nbytes_row):
    """Every first byte of a 16-byte access to a row of nbytes_row at
    base + k stride when base, the product or the sum is narrowed."""
    out = []
    for s in _span_points(np.array([0], np.int64), -(-nbytes_row // 16) * 16):
        out += [x + k * stride + s for x in narrow(base)] + [base + x + s for x in narrow(k * stride)]
        out += [x + s for x in narrow(base + k * stride)] + narrow(base + k * stride + s)
    return out
