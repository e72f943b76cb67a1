"""Damaged inputs per decode family: the one table behind
tests/test_damage_rules.py (CPU) and tests/test_gpu_damage_matrix.py (GPU).

The decode kernels decide per chunk whether to touch its bytes at all
(resolve_unit, csrc/zhip_decode_common.h:107-137; its two copies in
k_decode_tile, csrc/decode.hip:273-290, and in the predicted-load kernel
k_decode_ilp, csrc/decode_rows.hip:2037-2054).  A unit whose status is
ST_LENGTH_MISMATCH, ST_INDEX_OOB or ST_MISSING loads nothing from the address
its table or index entry gave, contributes nothing to the chunk's arrival
word, writes one status and one error bit, leaves the workspace clean and does
not disturb its neighbours.  A ROW here is the smallest layout that reaches
one kernel with one scheduling of that rule: its geometry, dtype, byte order
and chain, the kernel zhip_last_kernel() must report, the chunk of the batch
that is damaged and a chunk away from the damage.  Geometries come from the
tables that exist (test_gpu_kernel_matrix.DECODE_ROWS, dtype_cases.FAMILIES,
tile_cases.ROWS, test_gpu_shard_index.A_CASES / B_CASES and the fixtures of
test_gpu_fullrow_order.py / test_gpu_fused_launch.py).  Shipped library only.

Where each family issues its loads relative to the status decision (read
before the first GPU run; `ok` / `mode == ZHIP_ST_OK` is the decision):
  k_decode          decode.hip:86-87, 104-105   resolve_unit, then load_unit (zhip_decode_common.h:180-202: zeros
                    unless mode == OK); trailer under mode == OK (:88, :220); status + bit :213-216
  k_decode_tile     decode.hip:273-290 its own copy of the rule, loads under `mode == ZHIP_ST_OK` (:313-335);
                    status + bit :437-440
  k_decode_pair     decode_rows.hip:671-699.  Predicted launches load from predict_unit's address (:673-675)
                    BEFORE resolve_unit (:676): the address is the plan's (planner.predict_rows checks it inside
                    src), not the damaged length's; then load_unit_rows (:83-93: the zero line unless OK);
                    trailers under OK (:705-711); run ends under OK (:758-764)
  k_decode_lead     decode_rows.hip:822-839, as the pair kernel
  k_decode_lead4/8  decode_rows.hip:905-911 (loads under `ok`), :929 / :937 resolve_unit per chunk of the
                    workgroup, trailers under OK (:949); k_decode_lead8 is the same template with NQ = 8 (:872-873)
  k_decode_duo      decode_rows.hip:1079-1096: predicted loads (:1081) before resolve_unit (:1082), else
                    resolve_unit (:1089) then load_unit_rows (:1091); trailer under crc_on (:1096)
  k_decode_il       decode_rows.hip:1382-1400 (interleaved form: resolve_unit :1382, `ok` :1392, loads under `ok`
                    :1396-1400, trailer :1420); the hot form :1313-1344 the same with its predicted loads first
  k_decode_il (full-row form, fused launches: ilx_body) decode_rows.hip:2661-2697: resolve_unit per wave (:2661),
                    `ok` (:2671), loads (:2680) and trailer (:2697) under it
  k_decode_ilh      decode_rows.hip:2134-2165;  k_decode_ilw512  decode_rows.hip:2316-2350
  k_decode_tile4    decode_tile.hip:138-151;  k_decode_tile4w / tile2w  decode_tile.hip:489-500
  k_decode_tileg    decode_tile.hip:644-663;  k_decode_tilegw / tileg2w decode_tile.hip:852-867
Every kernel but k_decode_tile goes through resolve_unit, which loads the chunk record and (sharded) the 16-byte
index entry through the scalar cache and nothing else.

FORMS.  Unsharded rows: the damaged chunk's blob has the wrong length (U_FORMS).  Under a CRC chain "cut_4"
leaves exactly the payload length (an `expected` computed without the trailer passes it); under a chain
without one "ext_4" is its mirror.  Sharded rows: one index entry is rewritten, the index CRC recomputed
(test_gpu_shard_index.B_FORMS and its helpers).

SAFETY.  A kernel that wrongly followed a damaged input must land on readable bytes and be caught by a wrong
status or wrong data; it must never leave an allocation.  unsharded_safe / index_safe below state the
conditions over a restatement of DeviceStore.from_host's placement (arena_layout); the GPU test checks the
restatement against store.placement."""

from collections import namedtuple

import numpy as np

from test_gpu_shard_index import B_CASES, B_FORMS, LEN_MSG, MAXU, OOB_MSG, _geom  # noqa: F401  (re-exported)

LE = {"name": "bytes", "configuration": {"endian": "little"}}
BE = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}


def T(order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


# include/zarrhip.h ZHIP_ST_*
ST_OK, ST_MISSING, ST_CRC_MISMATCH, ST_INDEX_OOB, ST_LENGTH_MISMATCH = 0, 1, 2, 3, 4

ALIGN, TAIL_SLACK = 256, 64  # zarr_hip/store.py: placements in 256-byte granules, 64 readable bytes past the arena
STEP = 4096

# ------------------------------------------------------------------ unsharded rows
# id, chunk shape, dtype, endian, checksum, transpose order, chunk grid, kernel, damaged batch item, away batch
# item, fused (0: a launch alone; 3: the array planned three times, one k_decode_il_multi launch; 2: planned twice,
# one full-row launch), array shape (None: chunk * grid; the generic rows are ragged)
URow = namedtuple("URow", "id chunk dtype endian crc order grid kernel damaged away fused shape",
                  defaults=(0, None))

M64 = (64, 64, 64)

U_ROWS = [
    # -- k_decode (persistent, generic): 210-byte chunks (214 with the trailer: no multiple of 16), an array
    #    ragged in every dim so edge chunks are boxes; 27 chunks
    URow("gen_crc", (5, 3, 7), "int16", LE, True, None, (3, 3, 3), "k_decode", 13, 26, shape=(12, 7, 16)),
    URow("gen_nocrc", (5, 3, 7), "int16", BE, False, None, (3, 3, 3), "k_decode", 13, 0, shape=(12, 7, 16)),
    # -- k_decode_lead4: 16 KiB chunks, four per workgroup (dtype_cases "quad"); six chunks: a whole workgroup
    #    and a ragged one; the damaged chunk is lane group 2 of workgroup 0
    URow("lead4_crc", (4, 32, 32), "float32", LE, True, None, (1, 1, 6), "k_decode_lead4", 2, 5),
    URow("lead4_nocrc", (4, 32, 32), "int32", BE, False, None, (1, 1, 6), "k_decode_lead4", 1, 4),
    # -- k_decode_lead8: 8 KiB chunks, eight per workgroup (launch_lead4's e8); ten chunks
    URow("lead8", (2, 32, 32), "float32", LE, True, None, (1, 1, 10), "k_decode_lead8", 5, 9),
    # -- k_decode_pair: 96 KiB (three units), five chunks = 15 units, an odd count (DECODE_ROWS pair_3); the
    #    damaged chunk's units 6..8 share workgroups 3 and 4 with chunks 1 and 3
    URow("pair_odd", (3, 64, 512), "uint8", LE, True, None, (1, 1, 5), "k_decode_pair", 2, 4),
    # -- k_decode_duo: nseg 33 (DECODE_ROWS duo_33-f32le), 99 units: the last workgroup's second half idle
    URow("duo_33", (33, 64, 128), "float32", LE, True, None, (1, 1, 3), "k_decode_duo", 1, 2),
    # -- k_decode_ilh (DECODE_ROWS ilh_f64be): half units, the look-back finalizer
    URow("ilh", (32, 64, 64), "float64", BE, True, None, (1, 1, 4), "k_decode_ilh", 1, 3),
    # -- k_decode_ilw512 (DECODE_ROWS ilw_w64-f32le, three chunks of 2 MiB: 192 units)
    URow("ilw512", (512, 1024), "float32", LE, True, None, (1, 3), "k_decode_ilw512", 1, 2),
    # -- k_decode_il, launches of more than 512 units (DECODE_ROWS il_s32-f32le, il_s16, il_s8, il_w40, il_ragged32)
    URow("il_s32", M64, "float32", LE, True, None, (1, 1, 17), "k_decode_il", 8, 16),
    URow("il_s16", M64, "int16", BE, True, None, (1, 1, 33), "k_decode_il", 16, 0),
    URow("il_s8", (32, 32, 32), "float64", LE, True, None, (1, 1, 65), "k_decode_il", 31, 64),
    URow("il_w40", (40, 64, 64), "float64", BE, True, None, (1, 1, 13), "k_decode_il", 6, 12),  # counted arrival
    URow("il_ragged32", (250, 32, 32), "float32", LE, True, None, (1, 1, 17), "k_decode_il", 9, 0),  # ragged head
    # -- the LDS-tiled transposes (tile_cases r2_tile4-f32le, r2_tile4_nocrc, r4_tileg, r4_tileg_nocrc,
    #    r4_gen-f32le; test_gpu_decode.test_transpose_tile4w_many_workgroups_per_chunk with a third chunk)
    URow("tile2w", (256, 128), "float32", LE, True, (1, 0), (2, 2), "k_decode_tile2w", 1, 3),
    URow("tile4_nocrc", (256, 128), "float32", LE, False, (1, 0), (2, 2), "k_decode_tile4", 2, 0),
    URow("tile4w", (128, 64, 256), "int16", BE, True, (2, 1, 0), (1, 3, 1), "k_decode_tile4w", 1, 2),
    URow("tileg2w", (4, 3, 40, 24), "int16", LE, True, (1, 3, 0, 2), (2, 2, 1, 2), "k_decode_tileg2w", 3, 7),
    # k_decode_tilegw cannot be reached on the shipped library: every plan that builds its wave-per-tile chains
    # builds the two-tile lane constants with them (plan_tables.cpp:209, T.tg2w under p.tilegw alone), and
    # launch_tile_groups (decode.hip:882-884) then takes the two-tile form, reported as k_decode_tileg2w; the
    # four-tile name is tuning arm 38's.  The grouped kernel without a checksum, k_decode_tileg, has a row instead.
    URow("tileg_nocrc", (4, 3, 40, 24), "int16", BE, False, (1, 3, 0, 2), (2, 2, 1, 2), "k_decode_tileg", 4, 0),
    URow("tile_gen", (3, 5, 40, 20), "float32", LE, True, (3, 0, 1, 2), (2, 1, 1, 2), "k_decode_tile", 1, 3),
    # -- fused launches: three programs of the il_s32 geometry in one k_decode_il_multi launch (17 chunks: no
    #    multiple of four, the interleaved form), and the full-row pair (20 chunks of 1 MiB, test_gpu_fullrow_order's
    #    `plain`: the damaged chunk 9 is wave 1 of group 2, its neighbours 8, 10, 11 the other three waves)
    URow("fused_il3", M64, "float32", BE, True, None, (1, 1, 17), "k_decode_il", 7, 16, fused=3),
    URow("fused_fullrow", M64, "float32", LE, True, None, (5, 2, 2), "k_decode_il", 9, 19, fused=2),
]
U_BY_ID = {r.id: r for r in U_ROWS}
assert len(U_BY_ID) == len(U_ROWS)

# the rows of the mixed launch (one per family group) and of the host-store run
U_MIXED = ["gen_crc", "lead4_crc", "il_s32", "tile2w", "fused_fullrow"]
U_HOST = ["gen_crc", "il_s32"]

# (name, good length -> damaged length or None where the form does not apply)
U_FORMS = [
    ("cut_1", lambda n: n - 1),
    ("cut_4", lambda n: n - 4),
    ("cut_4096", lambda n: n - STEP if n > STEP else None),  # one 4 KiB step, where the chunk has one to lose
    ("ext_1", lambda n: n + 1),
    ("ext_4", lambda n: n + 4),
    ("ext_16", lambda n: n + 16),
    ("one_byte", lambda n: 1),
    ("empty", lambda n: 0),
]
U_FORM = dict(U_FORMS)


def u_shape(row):
    return row.shape if row.shape is not None else tuple(c * g for c, g in zip(row.chunk, row.grid))


def u_codecs(row):
    return ([T(row.order)] if row.order else []) + [row.endian] + ([CRC] if row.crc else [])


def u_keys(row):
    """Batch items of a whole read: the chunk grid in C order."""
    return ["c/" + "/".join(str(i) for i in ix) for ix in np.ndindex(*row.grid)]


def u_elen(row):
    return int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize + (4 if row.crc else 0)


def u_region(row, item):
    """Array region of batch item `item`, clipped to the array."""
    ix = np.unravel_index(item, row.grid)
    return tuple(slice(int(i) * c, min((int(i) + 1) * c, s)) for i, c, s in zip(ix, row.chunk, u_shape(row)))


def u_forms(row):
    """The forms that apply to the row: (name, damaged length)."""
    n = u_elen(row)
    return [(name, f(n)) for name, f in U_FORMS if f(n) is not None]


# ------------------------------------------------------------------ placement
def _aligned(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def arena_layout(lengths):
    """DeviceStore.from_host restated: {key: (offset, length)} for blobs placed in dict order, each on the next
    256-byte granule; (placements, top, allocation size) -- the allocation keeps TAIL_SLACK readable bytes past
    a capacity of at least the sum of (length + 256) + 256, at least 64 KiB."""
    place, top, total = {}, 0, ALIGN
    for k, n in lengths.items():
        place[k] = (top, n)
        top = _aligned(top + n)
        total += n + ALIGN
    return place, top, _aligned(max(total, 1 << 16)) + TAIL_SLACK


def arena_image(host):
    """The arena's bytes [0, top) as from_host writes them (zero padding)."""
    place, top, _ = arena_layout({k: len(v) for k, v in host.items()})
    img = np.zeros(top, np.uint8)
    for k, (o, n) in place.items():
        img[o: o + n] = np.frombuffer(host[k], np.uint8)
    return img


def damaged_blob(host, key, new_len):
    """The blob a reader of `key` sees once its recorded length is `new_len`: the arena's bytes from the blob's
    offset (a longer blob runs on into the padding, then into the next blob)."""
    place, _, _ = arena_layout({k: len(v) for k, v in host.items()})
    o = place[key][0]
    return arena_image(host)[o: o + new_len].tobytes()


def unsharded_safe(row, place, top, alloc):
    """The damaged blob is not the last in the arena, at least one full chunk's bytes of other blobs follow its
    slot, and every damaged length stays inside the blobs placed (so the bytes a kernel that believed the
    length would read are the store's own)."""
    keys = u_keys(row)
    assert row.damaged != row.away and 0 <= row.damaged < len(keys) and 0 <= row.away < len(keys)
    off, n = place[keys[row.damaged]]
    assert n == u_elen(row)
    assert any(o > off for o, _ in place.values()), "the damaged blob is the last in the arena"
    assert top - (off + _aligned(n)) >= n, "less than one chunk's bytes follow the damaged blob"
    for name, new_len in u_forms(row):
        assert 0 <= new_len and off + new_len + TAIL_SLACK <= top <= alloc, name
    return True


# ------------------------------------------------------------------ sharded rows
# test_gpu_shard_index._geom dicts (shape, shard, inner, dtype, chain) with: slot (the C-order inner chunk whose
# entry is rewritten), item (the batch item -- shard grid in C order -- that is damaged; never the first in the
# arena: the wrapped 2^64 - 1 forms point one byte before the shard), dec (the kernel), fused (as above).
# The away chunk is the inner chunk of the same shard farthest from the slot (test_gpu_shard_index._untouched_sel).
# Every row runs every form of B_FORMS; the two +2^32 forms run in stores placed low in the large backing of
# tests/test_gpu_wide_offsets.py (fixture `backings`), where the displaced address stays inside the backing.
S_ROWS = [
    # k_decode_il alone: 24 inner chunks of 1 MiB in three shards (test_gpu_fullrow_order's `sharded`), 768 units
    _geom((384, 128, 128), (128, 128, 128), M64, "float32", [LE, CRC], id="il", slot=3, item=1, dec="k_decode_il",
          fused=0),
    # the full-row pair over the same array (waves 0..3 of group 2 are slots 0..3 of shard 1)
    _geom((384, 128, 128), (128, 128, 128), M64, "float32", [LE, CRC], id="fused_fullrow", slot=2, item=1,
          dec="k_decode_il", fused=2),
    # k_decode_lead8: 8 KiB inner chunks without a checksum (A_CASES lead8's inner chunk), four per shard, four
    # shards: eight chunks per workgroup, so workgroup 0 holds shard 0 and shard 1
    _geom((128, 256), (64, 128), (32, 64), "int32", [LE], id="lead8", slot=1, item=1, dec="k_decode_lead8", fused=0),
    # tile4 family (tile_cases r2_sharded): transposed 128 KiB inner chunks, two per shard, four shards
    _geom((512, 512), (256, 256), (256, 128), "float32", [T((1, 0)), LE, CRC], id="tile4", slot=0, item=2,
          dec="k_decode_tile2w", fused=0),
    # grouped tiles (tile_cases r4_sharded): four inner chunks per shard, four shards
    _geom((8, 6, 80, 48), (8, 3, 40, 48), (4, 3, 40, 24), "int16", [T((1, 3, 0, 2)), BE, CRC], id="tileg", slot=2,
          item=1, dec="k_decode_tileg2w", fused=0),
    # k_decode_duo: inner chunks of 33 units (1056 KiB), two per shard, three shards = 198 units (three, so that
    # the damaged shard is neither the first nor the last blob of the arena)
    _geom((198, 64, 128), (66, 64, 128), (33, 64, 128), "float32", [LE, CRC], id="duo", slot=0, item=1,
          dec="k_decode_duo", fused=0),
    # k_decode_ilw512: inner chunks of 2 MiB (64 units), two per shard, three shards = 384 units
    _geom((3072, 1024), (1024, 1024), (512, 1024), "float32", [LE, CRC], id="ilw512", slot=0, item=1,
          dec="k_decode_ilw512", fused=0),
]
S_BY_ID = {g["id"]: g for g in S_ROWS}
assert len(S_BY_ID) == len(S_ROWS)

# the mixed launch's sharded rows: part B's generic and lead4 rows (damaged in shard 1), and three from above
S_MIXED = [dict(B_CASES[0], item=1, fused=0, dec="k_decode"), dict(B_CASES[2], item=1, fused=0, dec="k_decode_lead4"),
           S_BY_ID["il"], S_BY_ID["tile4"], S_BY_ID["fused_fullrow"]]

WIDE_FORMS = ("off_plus_2^32", "len_plus_2^32")
WIDE_BASE = 1 << 20  # where a row's first shard sits in the large backing's body


def s_keys(g):
    """Batch items of a whole read: the shard grid in C order."""
    return ["c/" + "/".join(str(i) for i in ix) for ix in np.ndindex(*g["grid"])]


def s_away_slot(g):
    return g["n"] - 1 if g["slot"] < g["n"] // 2 else 0


def index_safe(g, form, entry, good_entry, blob_len, shard_off, alloc, first_off):
    """The address a kernel that followed `entry` would load from, shard base + entry offset (mod 2^64: the
    hardware's address arithmetic), with the chunk's encoded length and the 64 bytes a 16-byte-wide load may
    overrun, lies inside the store's allocation [0, alloc); the damaged shard is not the first blob."""
    assert shard_off > first_off, "the damaged shard is the first in the arena"
    if entry == (MAXU, MAXU):
        return True
    at = (shard_off + entry[0]) % (1 << 64)
    assert 0 <= at and at + g["elen"] + TAIL_SLACK <= alloc, (g["id"], form, at, alloc)
    return True


# ------------------------------------------------------------------ the mixed launch
# Damage of one launch: (kind, batch item, slot).  "absent": the item's key is not in the store (every entry of
# the item is ST_MISSING); "marker": the index entry is (2^64-1, 2^64-1); "crc": one payload bit flipped;
# "length": the blob (unsharded) or the entry's length (sharded) is 4 short; "oob": the entry's length is the
# 2^64-1 marker alone.  Items are placed so that the first damaged item in batch order is the CRC one.
MIXED_CODE = {"absent": ST_MISSING, "marker": ST_MISSING, "crc": ST_CRC_MISMATCH, "length": ST_LENGTH_MISMATCH,
              "oob": ST_INDEX_OOB}


def mixed_damage_unsharded(row):
    """Absent: item 0; a flipped bit in item 1; item 2 four bytes short, with a healthy blob after it."""
    assert len(u_keys(row)) >= 4
    return [("absent", 0, 0), ("crc", 1, 0), ("length", 2, 0)]


def mixed_damage_sharded(g):
    """Absent: shard 0 (so the damaged shards are not the first in the arena and the last blob is whole);
    shard 1: a flipped bit and a marker; the last shard: a short entry and an out-of-bounds one."""
    n_items, n = int(np.prod(g["grid"])), g["n"]
    assert n_items >= 3 and n >= 2
    last = n_items - 1
    if n >= 4:
        return [("absent", 0, 0), ("crc", 1, 1), ("marker", 1, n - 1), ("length", last, 0), ("oob", last, n - 2)]
    # two inner chunks per shard: one kind per slot, the marker in a shard of its own where there is one
    if n_items >= 4:
        return [("absent", 0, 0), ("crc", 1, 1), ("marker", 2, 0), ("length", last, 0), ("oob", last, 1)]
    return [("absent", 0, 0), ("crc", 1, 1), ("marker", 1, 0), ("length", last, 0), ("oob", last, 1)]


def mixed_table(n_items, per_item, damage):
    """{(batch item, slot): status code} of one launch, from the batch order and the damage list alone, and the
    error word: the OR of 1 << code over the error codes present (include/zarrhip.h zhip_decode: not OK, not
    MISSING)."""
    table = {(i, s): ST_OK for i in range(n_items) for s in range(per_item)}
    for kind, item, slot in damage:
        if kind == "absent":
            for s in range(per_item):
                table[(item, s)] = ST_MISSING
        else:
            assert table[(item, slot)] == ST_OK, "two kinds of damage on one chunk"
            table[(item, slot)] = MIXED_CODE[kind]
    err = 0
    for code in table.values():
        if code not in (ST_OK, ST_MISSING):
            err |= 1 << code
    return table, err


def first_damaged(damage):
    """The first entry of `damage` that raises, in batch order (item, then slot)."""
    bad = sorted((item, slot, kind) for kind, item, slot in damage if kind in ("crc", "length", "oob"))
    return bad[0]
