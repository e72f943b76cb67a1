"""What licenses tests/test_gpu_wide_offsets.py, proved on the CPU with nothing
launched, for every row of tests/wide_cases.py:

  - the planners (Python and native) give chunk records whose out_off and src
    equal the restatement's, and the same fast / rows / tile verdicts and
    kernel flags as for the row's geometry read into a contiguous out;
  - the row has the property it is there for: an offset at or above 2**32, a
    chunk on both sides of 2**31 and one on both sides of 2**32; for the
    near-limit rows rel within 4096 of INT32_MAX; for the past-limit and
    wide-plane rows no row map;
  - SAFETY: every way any partial sum of any address can lose its high bits
    still lands inside the backing [front guard | body | back guard];
  - the exact boundary of the row map, against the scatter semantics;
  - the tile rows' host-built maps carry the restatement's per-tile out
    offsets, which pass 2**31."""

import functools

import numpy as np
import pytest

import tile_cases as TC
import wide_cases as W
from oracle import oracle as O
from test_native_planner import _same, _tables
from test_tile_maps import GROUP_ENT, TILE_ENT, _region

ALL_ROWS = W.READ_ROWS + W.WRITE_ROWS
IDS = [r.id for r in ALL_ROWS]
BY_ID = {r.id: r for r in ALL_ROWS + W.FUSED_ROWS}
assert len(BY_ID) == len(ALL_ROWS) + len(W.FUSED_ROWS)
DECODE_IDS = [r.id for r in W.READ_ROWS + W.FUSED_ROWS]
INT32_MAX = (1 << 31) - 1


def _chain(row):
    from zarr_hip import HipCodecPipeline, planner
    from zarr_hip.spec import ArraySpec

    spec = ArraySpec(W.array_chunks(row), np.dtype(row.dtype), row.fill)
    pipe = HipCodecPipeline.from_codecs(W.codecs(row)).evolve_from_array_spec(spec)
    return planner.analyze_chain(pipe.codecs, spec), spec


def _cell(row, coords):
    return int(coords[0 if row.spread == W.SLAB else 1])


@functools.lru_cache(maxsize=None)
def _blobs(rid):
    """{cell: the shard blob} of a sharded row: every shard holds the same
    index (all inner chunks present, fixed sizes), so one donor shard serves."""
    row = BY_ID[rid]
    if row.shard is None:
        return None
    shape = W.array_chunks(row)
    meta = O.ArrayMeta(shape, shape, np.dtype(row.dtype), row.fill, codecs=W.codecs(row))
    host = {}
    data = np.arange(int(np.prod(shape)), dtype=np.int64).astype(row.dtype).reshape(shape) + 1
    O.write(host, meta, (Ellipsis,), data)
    (blob,) = host.values()
    assert len(blob) == W.blob_len(row)
    return {c: blob for c in range(row.n)}


def _decode_items(row, place):
    projections, out_shape = O.basic_indexer((Ellipsis,), W.array_shape(row), W.array_chunks(row))
    assert tuple(out_shape) == W.array_shape(row) and len(projections) == row.n
    items = []
    for coords, csel, osel, _ in projections:
        c = _cell(row, coords)
        off, n = place.get(c, (0, 0))
        items.append((off, n, c not in place, csel, osel))
    return items


def _decode_tables(row, strides):
    chain, spec = _chain(row)
    items = _decode_items(row, W.read_placements(row))
    a = _tables(True, chain, spec, items, list(strides), 0)
    _same(a, _tables(False, chain, spec, items, list(strides), 0))
    return a


@pytest.mark.parametrize("rid", DECODE_IDS)
def test_decode_tables_equal_the_restatement(rid):
    from zarr_hip import _native as N

    row = BY_ID[rid]
    t = _decode_tables(row, W.view_strides(row))
    place = W.read_placements(row)
    dest = W.dest_chunks(row)
    assert len(t.chunks) == len(dest)
    item_cell = [_cell(row, p[0]) for p in O.basic_indexer((Ellipsis,), W.array_shape(row), W.array_chunks(row))[0]]
    got = sorted((item_cell[int(i)], int(o)) for i, o in zip(t.item_of_chunk, t.chunks["out_off"]))
    assert got == sorted((d.cell, d.out_off) for d in dest)
    for i, ch in zip(t.item_of_chunk, t.chunks):
        c = item_cell[int(i)]
        if c in place:
            assert (int(ch["src"]), int(ch["src_len"])) == place[c] and not ch["flags"] & N.CF_MISSING
        else:
            assert ch["flags"] & N.CF_MISSING
    if row.shard is not None:  # the index checks: at the start or the end of each present blob
        want = sorted(a for c, inner, a, b in W.src_ranges(row, place, _blobs(rid)) if inner == "index")
        assert sorted(int(s) for s in t.index_chunks["src"]) == want
        assert set(int(n) for n in t.index_chunks["src_len"]) == {W.index_size(row)}
    # the verdicts and the kernel flags of the same array read into a contiguous out
    t0 = _decode_tables(row, TC.c_strides(W.array_shape(row), W.itemsize(row)))
    assert (t.fast, t.rows, t.tile) == (t0.fast, t0.rows, t0.tile)
    assert N.Plan(t.layout, upload=False).kernel_flags == N.Plan(t0.layout, upload=False).kernel_flags
    assert t.rows == (row.rowmap or W.declined(row)) and t.tile == (row.order is not None)


def _encode_verdicts(chain, spec, items, strides):
    from zarr_hip import _native as N
    from zarr_hip import planner

    t = planner.plan_encode(chain, spec, items, list(strides), 0)
    return t, (t.fast, t.rows, t.tile, t.tile_prefix, N.Plan(t.layout, upload=False).kernel_flags)


@pytest.mark.parametrize("rid", [r.id for r in W.WRITE_ROWS if r.shard is None])
def test_encode_tables_equal_the_restatement(rid):
    row = W.WRITE[rid]
    chain, spec = _chain(row)
    projections, _ = O.basic_indexer((Ellipsis,), W.array_shape(row), W.array_chunks(row))
    dst = W.write_regions(row)
    cells = [_cell(row, p[0]) for p in projections]
    items = [(dst[c], csel, [s.start for s in osel]) for c, (_, csel, osel, _) in zip(cells, projections)]
    dest = {d.cell: d for d in W.dest_chunks(row)}
    t, wide = _encode_verdicts(chain, spec, items, W.view_strides(row))
    assert [int(o) for o in t.chunks["out_off"]] == [dest[c].out_off for c in cells]
    assert [int(s) for s in t.chunks["src"]] == [dst[c] for c in cells]
    _, plain = _encode_verdicts(chain, spec, items, TC.c_strides(W.array_shape(row), W.itemsize(row)))
    assert wide == plain
    assert max(dst.values()) > W.B32 and any(a < W.B32 < a + W.enc_len(row) for a in dst.values())


@pytest.mark.parametrize("rid", [r.id for r in W.WRITE_ROWS if r.shard is not None])
def test_sharded_encode_tables_equal_the_restatement(rid):
    """A sharded write encodes every inner chunk to its final place in the
    region reserved for its shard (zhip_shard.blob): data start + rank x
    encoded length in the codec's write order -- where the oracle's shard
    holds it, so the restatement reads the places from the oracle's index.
    The writer's order gives the same places; the inner planner's records
    carry them as src and the restatement's out_off; 2**32 falls inside the
    staged chunks of one shard."""
    from zarr_hip.spec import ArraySpec
    from zarr_hip.writer import subchunk_order

    row = W.WRITE[rid]
    chain, spec = _chain(row)
    sh = chain.shard
    inner_shape = W.array_chunks(row, row.chunk)
    assert tuple(sh.chunk_shape) == inner_shape
    inner_spec = ArraySpec(inner_shape, spec.dtype, spec.fill_value, spec.config)
    elen = W.nbytes(row.chunk, row) + (4 if row.crc else 0)
    data_start = W.index_size(row) if row.loc == "start" else 0
    regions = W.write_regions(row)
    where = dict(zip(np.ndindex(*W.inner_grid(row)), W.parse_index(row, _blobs(rid)[0])))
    cps = sh.chunks_per_shard(spec.shape)
    order = [tuple(int(x) for x in ic) for ic in subchunk_order(tuple(cps), sh.subchunk_write_order)]
    lead = len(cps) - len(row.chunk)  # (a slab's leading dimension)
    assert [where[ic[lead:]] for ic in order] == [(data_start + r * elen, elen) for r in range(len(order))]
    full = tuple(slice(0, k, 1) for k in inner_shape)
    dest = W.dest_chunks(row)
    items = [(regions[d.cell] + where[d.inner][0], full, [d.cell] + [a * k for a, k in zip(d.inner, row.chunk)])
             for d in dest]
    t, wide = _encode_verdicts(chain.inner, inner_spec, items, W.view_strides(row))
    assert [int(o) for o in t.chunks["out_off"]] == [d.out_off for d in dest]
    assert [int(x) for x in t.chunks["src"]] == [it[0] for it in items]
    _, plain = _encode_verdicts(chain.inner, inner_spec, items, TC.c_strides(W.array_shape(row), W.itemsize(row)))
    assert wide == plain
    assert any(a < W.B32 < a + elen for a, _, _ in items)
    assert any(r < W.B32 < r + W.blob_len(row) for r in regions.values()) and max(regions.values()) > W.B32


@pytest.mark.parametrize("rid", IDS)
def test_the_row_has_its_property(rid):
    row = BY_ID[rid]
    ranges = W.dest_ranges(row)
    per_chunk = W.chunk_ranges(row)
    if row.spread in (W.NEAR, W.PAST, W.PLANE):  # the out side stays below 2**32; the arena side passes it
        assert max(b for _, b in ranges) < W.B32 and any(W.straddles(r, W.B31) for r in per_chunk)
    else:
        assert max(b for _, b in ranges) > W.B32
        assert any(W.straddles(r, W.B32) for r in per_chunk)
        assert any(W.straddles(r, W.B31) for r in per_chunk)
    if row.spread == W.SLAB:
        if row.shard is None:  # contiguous chunks: one straddles each boundary as a single run
            assert any(a < W.B31 < b for a, b in ranges) and any(a < W.B32 < b for a, b in ranges)
        last = [r for d, r in zip(W.dest_chunks(row), per_chunk) if d.cell == W.dropped(row)]
        assert all(a >= W.B32 for r in last for a, _ in r)  # the missing / all-fill chunk lies wholly above
    if row in W.READ_ROWS:
        src = W.src_ranges(row, W.read_placements(row), _blobs(rid))
        blobs = sorted(W.read_placements(row).values())
        assert blobs[0][0] + blobs[0][1] < W.B31
        assert blobs[1][0] < W.B31 < sum(blobs[1]) and blobs[2][0] < W.B32 < sum(blobs[2])
        assert all(o > W.B32 for o, _ in blobs[3:])
        assert any(b > W.B32 for _, _, _, b in src)
        if row.shard is not None:  # inner chunks and an index on both sides of a straddled boundary
            for bound, (o, n) in ((W.B31, blobs[1]), (W.B32, blobs[2])):
                mine = [(a, b) for _, _, a, b in src if o <= a < o + n]
                assert any(b <= bound for _, b in mine) and any(a >= bound for a, _ in mine)


def test_the_fused_rows_have_their_property():
    """The low out lies wholly below 2**31 and the high out wholly above it,
    so their address ranges are disjoint; the high out's slab 16 straddles
    2**32 as one run and slab 17, the missing one, lies above; out_off of the
    high program reaches 2**31 relative to its own base.  The low program's
    blobs sit at the usual placements, the high program's behind them, above 2**32."""
    lo, hi = W.FUSED_ROWS
    assert max(b for _, b in W.dest_ranges(lo)) < W.B31 <= min(a for a, _ in W.dest_ranges(hi))
    ranges = W.chunk_ranges(hi)
    assert [a < W.B32 < b for (a, b), in ranges] == [c == hi.n - 2 for c in range(hi.n)]
    assert ranges[W.dropped(hi)][0][0] > W.B32 and max(b for _, b in W.dest_ranges(hi)) <= W.BODY
    assert max(d.out_off for d in W.dest_chunks(hi)) >= W.B31
    blobs = sorted(W.read_placements(lo).values())
    assert blobs[1][0] < W.B31 < sum(blobs[1]) and blobs[2][0] < W.B32 < sum(blobs[2])
    top = max(o + W.align(n) for o, n in blobs)
    mine = sorted(W.read_placements(hi).values())
    assert mine[0][0] == top > W.B32 and all(b[0] == a[0] + W.align(a[1]) for a, b in zip(mine, mine[1:]))
    assert sum(mine[-1]) + W.SLACK <= W.BODY


@pytest.mark.parametrize("rid", IDS + [r.id for r in W.FUSED_ROWS])
def test_every_narrowed_address_stays_inside_the_backing(rid):
    """THE SAFETY CONDITION.  For every chunk, every partial sum of
    out_off + rel + lane narrowed to its low 32 bits, those sign-extended, or
    its low 31 bits, gives a 16-byte store inside [-FRONT, BODY + BACK); the
    same for every load of src + k up to SLACK bytes past each blob, and for the
    regions a write reserves.  The un-narrowed addresses lie inside the body."""
    row = BY_ID[rid]
    for d in W.dest_chunks(row):
        assert W.inside(W.narrowed_dest(d), row.base)
        assert row.base + d.out_off + int(d.starts.min()) >= 0
        assert row.base + d.out_off + int(d.starts.max()) + d.run <= W.BODY
    if row not in W.WRITE_ROWS:
        spans = [(a, b) for _, _, a, b in W.src_ranges(row, W.read_placements(row), _blobs(rid))]
    else:
        spans = [(a, a + W.enc_len(row)) for a in W.write_regions(row).values()]
    for a, b in spans:
        assert W.inside(W.narrowed_src(a, b))
        assert a >= 0 and b + W.SLACK <= W.BODY
    assert W.FRONT >= W.B31 and W.BODY >= W.B32 + (1 << 29) and W.BACK >= 1 << 20 and W.TOTAL < 7 << 30


def _rows_map(row):
    """(return code, the map) of zhip_rows_map for the row's whole selection."""
    from zarr_hip import _native as N

    t = _decode_tables(row, W.view_strides(row))
    plan = N.Plan(t.layout, upload=False)
    n = int(N.lib().zhip_rows_map_len(plan.handle, len(t.sels)))
    m = np.zeros(max(n, 1), N.ROWBLK_DT)
    rc = N.lib().zhip_rows_map(plan.handle, np.ascontiguousarray(t.sels).ctypes.data, len(t.sels), m.ctypes.data, n)
    return rc, m, t


@pytest.mark.parametrize("rid", [r.id for r in W.READ_ROWS + W.FUSED_ROWS if r.rowmap or W.declined(r)])
def test_the_row_map_is_kept_or_declined(rid):
    """Rows with a row map keep it in the wide layout; near-limit rows reach
    rel within 4096 of INT32_MAX and rel + lane offset beyond the 0x7FFFFFF0
    records a buffer resource can address; past-limit and wide-plane rows are
    declined with ZHIP_E_UNSUPPORTED."""
    from zarr_hip import _native as N

    row = BY_ID[rid]
    rc, m, t = _rows_map(row)
    if not row.rowmap:
        assert rc == N.E_UNSUPPORTED
        return
    assert rc == 0
    live = m[m["hi"] > m["lo"]]
    want = W.dest_chunks(row)[0]
    rb = row.chunk[-1] * W.itemsize(row)
    lane_off = (4096 // rb - 1) * int(t.layout.out_stride[t.layout.ndim - 2]) + rb - 16
    assert int(live["rel"].min()) >= 0
    assert int(live["rel"].max()) + lane_off == int(want.starts.max()) + want.run - 16
    if row.spread == W.NEAR:
        assert INT32_MAX - 4096 < int(live["rel"].max()) <= INT32_MAX
        assert int(live["rel"].max()) == 2147482704
        assert int(live["rel"].max()) + lane_off > 0x7FFFFFF0


def test_the_exact_row_map_boundary():
    """zhip_rows_map at S0 = 34 086 832 against the scatter semantics (as
    test_native_abi.test_rows_map_matches_scatter_semantics states them), and
    ZHIP_E_UNSUPPORTED 16 bytes further."""
    from zarr_hip import _native as N
    from zarr_hip.planner import SEL_DT, _make_layout

    shape, it = (64, 64, 64), 4
    table = np.zeros(1, SEL_DT)
    table[0]["count"][:3] = shape
    table[0]["step"][:3] = 1
    for s0, ok in ((W.NEAR_S0, True), (W.PAST_S0, False)):
        ost = [s0, 256, 4]
        plan = N.Plan(_make_layout(shape, it, ost, 0, b"\0"), upload=False)
        nseg = plan.units_per_chunk
        n = int(N.lib().zhip_rows_map_len(plan.handle, 1))
        assert n == nseg * 8
        m = np.zeros(n, N.ROWBLK_DT)
        rc = N.lib().zhip_rows_map(plan.handle, table.ctypes.data, 1, m.ctypes.data, n)
        if not ok:
            assert rc == N.E_UNSUPPORTED
            continue
        assert rc == 0
        m = m.reshape(nseg, 8)
        rb = shape[-1] * it
        E = int(np.prod(shape)) * it
        t = np.arange(256)
        lane_row, lane_col = (16 * t) // rb, (16 * t) % rb
        seen = 0
        for u in range(nseg):
            for k in range(8):
                e = m[u, k]
                off = E - (u + 1) * 8 * 4096 + 4096 * k + 16 * t
                coords = np.stack(np.unravel_index(off // rb, shape[:-1]))
                dst = lane_col + coords[0] * ost[0] + coords[1] * ost[1]
                assert ((lane_row >= e["lo"]) & (lane_row < e["hi"])).all()
                np.testing.assert_array_equal(int(e["rel"]) + lane_row * ost[1] + lane_col, dst)
                seen = max(seen, int(e["rel"]))
        assert seen == 2147482704


TILE_ROWS = [r.id for r in ALL_ROWS if r.order is not None]


@pytest.mark.parametrize("rid", TILE_ROWS)
def test_tile_maps_carry_the_restated_offsets(rid):
    """tile4_map / g_map (Plan.table_image(1)) hold the restatement's per-tile
    out offset, which for the planes rows passes 2**31 (plane 2 at 2 S0, plane
    3 at 3 S0 = 2**32 - d)."""
    from zarr_hip import _native as N

    row = BY_ID[rid]
    shape, it, ost = W.stored_tile_geometry(row)
    ts = TC.tiles(shape, it, ost)
    if row in W.READ_ROWS:
        layout = _decode_tables(row, W.view_strides(row)).layout
    else:
        from zarr_hip import planner

        chain, spec = _chain(row)
        full = tuple(slice(0, k, 1) for k in W.array_chunks(row))
        layout = planner.plan_encode(chain, spec, [(0, full, [0] * len(full))], list(W.view_strides(row)), 0).layout
    plan = N.Plan(layout, upload=False)
    kf = plan.kernel_flags
    assert kf & N.PK_TILE
    fam = TC.family(shape, it, ost)
    assert bool(kf & N.PK_TILE4) == (fam == "tile4")
    if fam != "tile4":
        assert bool(kf & N.PK_TILEG) == (fam == "grouped")
    names = {"tile4": (TC.T2W, TC.E2) if row.crc else (TC.T4, TC.E4), "grouped": (TC.TG2W if row.crc else TC.TG, TC.EG),
             "general": (TC.TGEN, TC.EGEN)}[fam]
    assert row.kernel in names
    if row.spread == W.PLANES:
        assert max(t.o_off for t in ts) > W.B31 and max(t.o_off for t in ts) + 256 > W.B32 - (1 << 20)
    tmap = _region(plan, "tile4_map").view(TILE_ENT)
    if kf & N.PK_TILE4:
        assert [int(b) for b in tmap["tbase"]] == [t.s_off for t in ts]
        assert [int(o) for o in tmap["orel"]] == [t.o_off for t in ts]
    gmap = _region(plan, "g_map").view(GROUP_ENT)
    if len(gmap):
        by_base = {t.s_off: t for t in ts}
        for e in gmap:
            assert int(e["orel"]) == by_base[int(e["tbase"])].o_off
        if row.spread == W.PLANES:  # a group's four tiles are one per plane: the first at a small offset, the
            assert max(t.o_off for t in ts) - max(int(e["orel"]) for e in gmap) > W.B31  # step between them huge
    assert len(tmap) or len(gmap) or fam == "general"


@pytest.mark.parametrize("asz,bsz", [(4, 2), (1, 8)])
def test_value_items_are_disjoint_wide_and_safe(asz, bsz):
    """The value-map items of the GPU test: rows pairwise disjoint on either
    side, a base at 2**32, a product k * s past 2**32, rows of one item on both
    sides of 2**32 -- and every narrowing of base, product or sum inside the
    backing."""
    items = W.value_items(asz, bsz)
    rows = W.value_rows(items)
    for side, isz in ((2, asz), (3, bsz)):
        spans = sorted((r[side], r[side] + r.count * isz) for r in rows)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert spans[0][0] >= 0 and spans[-1][1] <= W.BODY
    assert items[0][0] == items[0][1] == W.B32
    # the base and the stride-product items take the per-element path, the third the vector path
    assert [W.value_vector_path(it, asz, bsz) for it in items] == [False, False, True]
    assert 2 * W.VALUE_STRIDE > W.B32 and W.VALUE_STRIDE == W.B31 + 4096
    third = [r for r in rows if r.item == 2]
    assert sum(r.a + r.count * asz <= W.B32 for r in third) == 4 and sum(r.a >= W.B32 for r in third) == 4
    assert all(r.a % 16 == 0 and r.b % 16 == 0 for r in third)
    for r in rows:
        a0, b0, dims = items[r.item][:3]
        sa, sb = (dims[0][1], dims[0][2]) if len(dims) > 1 else (0, 0)
        assert W.inside(W.narrowed_value(a0, r.k, sa, r.count * asz))
        assert W.inside(W.narrowed_value(b0, r.k, sb, r.count * bsz))
