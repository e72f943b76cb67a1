"""What licenses tests/test_gpu_damage_matrix.py, proved on the CPU with nothing
launched, for every row and form of tests/damage_cases.py:

  - the oracle raises ValueError on a whole read and on a read of only the
    damaged chunk, while a window over the "away" chunk reads exactly;
  - SAFETY: the damaged unsharded blob is not the last in the arena and a
    chunk's bytes follow it; every address an index entry displaces a load to
    lies inside the store's allocation (inside the large backing for the two
    +2^32 forms) -- from a restatement of the arena placement;
  - the planner's verdicts and the plan's kernel flags match the row's kernel
    where they decide it, and the planner hands the damaged length on as it
    is (the kernels decide, not the host);
  - the mixed launch's status table and error word follow from the batch
    order and the damage list alone."""

import functools
import struct

import numpy as np
import pytest

import damage_cases as DC
import wide_cases as W
from oracle import oracle as O
from test_gpu_decode import _data
from test_gpu_shard_index import _entry, _index_start, _rewrite_entry, _slot_region

U_IDS = [r.id for r in DC.U_ROWS]
S_IDS = [g["id"] for g in DC.S_ROWS]
LOCS = ["end", "start"]


# ------------------------------------------------------------------ the oracle's stores
def u_meta(row):
    return O.ArrayMeta(DC.u_shape(row), row.chunk, np.dtype(row.dtype), 3, codecs=DC.u_codecs(row))


@functools.lru_cache(maxsize=4)
def u_host(rid):
    """(host store, the whole array) of an unsharded row, written by the oracle."""
    row = DC.U_BY_ID[rid]
    host = {}
    O.write(host, u_meta(row), (Ellipsis,), _data(DC.u_shape(row), row.dtype, 31))
    assert list(host) == DC.u_keys(row)  # the arena order is the batch order
    assert all(len(v) == DC.u_elen(row) for v in host.values())
    return host, O.read(host, u_meta(row))


def s_codecs(g, loc):
    from test_gpu_decode import SHARD

    return [SHARD(g["inner"], g["chain"], loc)]


def s_meta(g, loc):
    return O.ArrayMeta(g["shape"], g["shard"], np.dtype(g["dtype"]), 0, codecs=s_codecs(g, loc))


@functools.lru_cache(maxsize=4)
def _s_host(gid, loc, seed):
    g = DC.S_BY_ID.get(gid) or {m["id"]: m for m in DC.S_MIXED}[gid]
    host = {}
    O.write(host, s_meta(g, loc), (Ellipsis,), _data(g["shape"], g["dtype"], seed))
    assert list(host) == DC.s_keys(g)
    return host, O.read(host, s_meta(g, loc))


def s_host(g, loc, seed=37):
    return _s_host(g["id"], loc, seed)


def s_entry(g, loc, blob, form):
    """(the rewritten shard blob, the entry, the good entry) for one of B_FORMS' functions."""
    off, ln = _entry(blob, g["n"], loc, True, g["slot"])
    assert ln == g["elen"] and off + ln + 4 <= len(blob)
    entry = form(off, ln, g["elen"], len(blob))
    return _rewrite_entry(blob, g["n"], loc, True, g["slot"], *entry), entry, (off, ln)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------ unsharded rows
@pytest.mark.parametrize("rid", U_IDS)
def test_unsharded_oracle_raises_and_placement_is_safe(rid):
    row = DC.U_BY_ID[rid]
    host, want = u_host(rid)
    meta = u_meta(row)
    keys = DC.u_keys(row)
    key = keys[row.damaged]
    place, top, alloc = DC.arena_layout({k: len(v) for k, v in host.items()})
    assert DC.unsharded_safe(row, place, top, alloc)
    touched, away = DC.u_region(row, row.damaged), DC.u_region(row, row.away)
    names = [n for n, _ in DC.u_forms(row)]
    big = DC.u_elen(row) > DC.STEP
    assert names == [n for n, _ in DC.U_FORMS if n != "cut_4096" or big]  # no other form is left out
    for name, new_len in DC.u_forms(row):
        bad = dict(host)
        bad[key] = DC.damaged_blob(host, key, new_len)
        assert len(bad[key]) == new_len != len(host[key])
        if new_len < len(host[key]):
            assert bad[key] == host[key][:new_len]
        else:
            assert bad[key][: len(host[key])] == host[key]
        for sel in ((Ellipsis,), touched):
            with pytest.raises(ValueError):
                O.read(bad, meta, sel)
        assert same(O.read(bad, meta, away), want[away]), name
    if row.crc:  # the form that catches an `expected` computed without the trailer
        assert dict(DC.u_forms(row))["cut_4"] == DC.u_elen(row) - 4 == int(np.prod(row.chunk)) * want.itemsize
    else:
        assert dict(DC.u_forms(row))["ext_4"] == int(np.prod(row.chunk)) * want.itemsize + 4


def _chain(shape, chunks, dtype, fill, codecs):
    from zarr_hip import HipCodecPipeline, planner
    from zarr_hip.spec import ArraySpec

    spec = ArraySpec(tuple(chunks), np.dtype(dtype), fill)
    pipe = HipCodecPipeline.from_codecs(codecs).evolve_from_array_spec(spec)
    return planner.analyze_chain(pipe.codecs, spec), spec


def _tables(shape, chunks, dtype, fill, codecs, place, keys):
    """planner.plan_decode for a whole read of blobs at `place` into a contiguous out."""
    from zarr_hip import planner

    chain, spec = _chain(shape, chunks, dtype, fill, codecs)
    projections, out_shape = O.basic_indexer((Ellipsis,), tuple(shape), tuple(chunks))
    grid = tuple(-(-s // c) for s, c in zip(shape, chunks))
    items = []
    for coords, csel, osel, _ in projections:
        k = keys[int(np.ravel_multi_index(tuple(int(c) for c in coords), grid))]
        off, n = place.get(k, (0, 0))
        items.append((off, n, k not in place, csel, osel))
    it = np.dtype(dtype).itemsize
    strides = [it * int(np.prod(out_shape[d + 1:])) for d in range(len(out_shape))]
    return planner.plan_decode(chain, spec, items, strides, 0)


def _flags_match(t, kernel):
    from zarr_hip import _native as N

    kf = N.Plan(t.layout, upload=False).kernel_flags
    il = kernel in ("k_decode_il", "k_decode_ilh", "k_decode_ilw512")
    rows = il or kernel in ("k_decode_pair", "k_decode_duo", "k_decode_lead4", "k_decode_lead8", "k_decode_lead")
    tile = kernel.startswith("k_decode_tile")
    assert bool(t.rows) == rows and bool(t.tile) == tile, (kernel, t.rows, t.tile)
    if not tile:  # (the flag speaks of the stored layout alone: a transposed chunk of 8 x 32 KiB units has it too)
        assert bool(kf & N.PK_IL) == il, (kernel, kf)
    assert bool(kf & N.PK_TILE) == tile
    if tile:
        t4 = kernel in ("k_decode_tile2w", "k_decode_tile4", "k_decode_tile4w")
        assert bool(kf & N.PK_TILE4) == t4
        if not t4:
            assert bool(kf & N.PK_TILEG) == kernel.startswith("k_decode_tileg")


@pytest.mark.parametrize("rid", U_IDS)
def test_unsharded_plan_names_the_family_and_keeps_the_length(rid):
    from zarr_hip import _native as N

    row = DC.U_BY_ID[rid]
    keys = DC.u_keys(row)
    lengths = {k: DC.u_elen(row) for k in keys}
    place, _, _ = DC.arena_layout(lengths)
    new_len = dict(DC.u_forms(row))["cut_4"]
    place[keys[row.damaged]] = (place[keys[row.damaged]][0], new_len)
    t = _tables(DC.u_shape(row), row.chunk, row.dtype, 3, DC.u_codecs(row), place, keys)
    _flags_match(t, row.kernel)
    assert len(t.chunks) == len(keys) and sorted(int(i) for i in t.item_of_chunk) == list(range(len(keys)))
    for i, ch in zip(t.item_of_chunk, t.chunks):
        assert (int(ch["src"]), int(ch["src_len"])) == place[keys[int(i)]] and not ch["flags"] & N.CF_MISSING
    assert (N.ST_OK, N.ST_MISSING, N.ST_CRC_MISMATCH, N.ST_INDEX_OOB, N.ST_LENGTH_MISMATCH) == \
        (DC.ST_OK, DC.ST_MISSING, DC.ST_CRC_MISMATCH, DC.ST_INDEX_OOB, DC.ST_LENGTH_MISMATCH)


# ------------------------------------------------------------------ sharded rows
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("gid", S_IDS)
def test_sharded_oracle_raises_and_addresses_are_safe(gid, loc):
    g = DC.S_BY_ID[gid]
    host, want = s_host(g, loc)
    meta = s_meta(g, loc)
    keys = DC.s_keys(g)
    key = keys[g["item"]]
    place, top, alloc = DC.arena_layout({k: len(v) for k, v in host.items()})
    shard_coords = tuple(int(i) for i in np.unravel_index(g["item"], g["grid"]))
    touched = _slot_region(g, shard_coords, g["slot"])
    away = _slot_region(g, shard_coords, DC.s_away_slot(g))
    assert g["slot"] != DC.s_away_slot(g)
    assert [n for n, _, _ in DC.B_FORMS if n not in DC.WIDE_FORMS] == \
        ["off_past_blob", "off_in_tail", "off_marker_only", "len_marker_only", "len_minus_4", "len_plus_4", "missing"]
    for name, form, msg in DC.B_FORMS:
        blob, entry, good = s_entry(g, loc, host[key], form)
        if name in DC.WIDE_FORMS:  # in the large backing, the first shard at WIDE_BASE
            wplace = {k: (o + DC.WIDE_BASE, n) for k, (o, n) in place.items()}
            assert DC.index_safe(g, name, entry, good, len(blob), wplace[key][0], W.BODY, wplace[keys[0]][0])
            assert wplace[key][0] + entry[0] >= 1 << 32 or entry[1] >= 1 << 32
        else:
            assert DC.index_safe(g, name, entry, good, len(blob), place[key][0], alloc, place[keys[0]][0])
        bad = dict(host)
        bad[key] = blob
        if msg is None:  # a missing inner chunk reads as fill
            got = O.read(bad, meta)
            filled = want.copy()
            filled[touched] = 0
            assert same(got, filled)
            continue
        for sel in ((Ellipsis,), touched):
            with pytest.raises(ValueError):
                O.read(bad, meta, sel)
        assert same(O.read(bad, meta, away), want[away]), name


@pytest.mark.parametrize("gid", S_IDS)
def test_sharded_plan_names_the_family(gid):
    g = DC.S_BY_ID[gid]
    keys = DC.s_keys(g)
    blob_len = g["n"] * g["elen"] + 16 * g["n"] + 4
    place, _, _ = DC.arena_layout({k: blob_len for k in keys})
    t = _tables(g["shape"], g["shard"], g["dtype"], 0, s_codecs(g, "end"), place, keys)
    _flags_match(t, g["dec"])
    assert len(t.chunks) == len(keys) * g["n"]
    assert t.index_chunks is not None and len(t.index_chunks) == len(keys)  # index checks ride in the launch


# ------------------------------------------------------------------ the mixed launch
def test_mixed_tables_follow_from_the_inputs():
    for rid in DC.U_MIXED:
        row = DC.U_BY_ID[rid]
        n = len(DC.u_keys(row))
        damage = DC.mixed_damage_unsharded(row)
        table, err = DC.mixed_table(n, 1, damage)
        assert sorted(k for k, _, _ in damage) == ["absent", "crc", "length"]
        assert len(table) == n and err == (1 << DC.ST_CRC_MISMATCH) | (1 << DC.ST_LENGTH_MISMATCH)
        codes = [table[(i, 0)] for i in range(n)]
        assert codes.count(DC.ST_OK) == n - 3 and codes.count(DC.ST_MISSING) == 1
        assert DC.first_damaged(damage)[2] == "crc"
        # the wrong-length blob is followed by a healthy one in the arena
        length_item = [i for k, i, _ in damage if k == "length"][0]
        assert all(table[(i, 0)] == DC.ST_OK for i in range(length_item + 1, n)) and length_item + 1 < n
    for g in DC.S_MIXED:
        n_items = int(np.prod(g["grid"]))
        damage = DC.mixed_damage_sharded(g)
        table, err = DC.mixed_table(n_items, g["n"], damage)
        assert sorted(k for k, _, _ in damage) == ["absent", "crc", "length", "marker", "oob"]
        assert err == (1 << DC.ST_CRC_MISMATCH) | (1 << DC.ST_LENGTH_MISMATCH) | (1 << DC.ST_INDEX_OOB)
        codes = list(table.values())
        assert codes.count(DC.ST_MISSING) == g["n"] + 1
        assert codes.count(DC.ST_OK) == n_items * g["n"] - g["n"] - 4
        assert DC.first_damaged(damage)[2] == "crc"
        assert all(item != 0 for kind, item, _ in damage if kind != "absent")  # no damaged shard is the first blob


def _mixed_sharded_host(g, loc="end"):
    """The oracle's store of a sharded row with the mixed damage applied: (host, damage)."""
    host, _ = s_host(g, loc, 41)
    host = dict(host)
    keys = DC.s_keys(g)
    damage = DC.mixed_damage_sharded(g)
    for kind, item, slot in damage:
        key = keys[item]
        if kind == "absent":
            del host[key]
            continue
        blob = host[key]
        off, ln = _entry(blob, g["n"], loc, True, slot)
        if kind == "crc":
            b = bytearray(blob)
            b[off + ln // 2] ^= 0x10
            host[key] = bytes(b)
        else:
            entry = {"marker": (DC.MAXU, DC.MAXU), "length": (off, g["elen"] - 4), "oob": (off, DC.MAXU)}[kind]
            host[key] = _rewrite_entry(blob, g["n"], loc, True, slot, *entry)
    return host, damage


@pytest.mark.parametrize("g", DC.S_MIXED, ids=[g["id"] for g in DC.S_MIXED])
def test_mixed_sharded_oracle(g):
    """Each damaged inner chunk alone raises in the oracle, the marker and the absent shard read as fill."""
    host, damage = _mixed_sharded_host(g)
    meta = s_meta(g, "end")
    for kind, item, slot in damage:
        coords = tuple(int(i) for i in np.unravel_index(item, g["grid"]))
        sel = _slot_region(g, coords, slot)
        if kind in ("absent", "marker"):
            assert not O.read(host, meta, sel).any()
        else:
            with pytest.raises(ValueError):
                O.read(host, meta, sel)


def test_index_start_and_struct_layout():
    """The helpers this table borrows address the entry they say: 16 bytes of two LE u64 at 16 * slot."""
    g = DC.S_BY_ID["lead8"]
    host, _ = s_host(g, "start")
    blob = host[DC.s_keys(g)[g["item"]]]
    at = _index_start(len(blob), g["n"], "start", True) + 16 * g["slot"]
    assert struct.unpack("<QQ", blob[at: at + 16]) == _entry(blob, g["n"], "start", True, g["slot"])
