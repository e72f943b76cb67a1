"""The tile kernels' selection and host-built maps on the CPU, for every row of
tests/tile_cases.py (ranks 2, 4 and 5): the plan's kernel flags name the
family the row names, the planner's tile / tile_prefix choice, and the maps
csrc/plan_tables.cpp builds -- tile4_map, g_map and the per-tile unit
constants, whose ORDER is the order the kernels derive tile coordinates in --
against the numpy restatement in tile_cases.py.  No GPU needed."""

import numpy as np
import pytest

import tile_cases as TC
from test_plan_tables import TILE_REGIONS, ROW_REGIONS
from zarr_hip import _native as N
from zarr_hip import codecs as C
from zarr_hip import planner as P
from zarr_hip.spec import ArraySpec

CRCJ = {"name": "crc32c"}
TILE_ENT = np.dtype([("tbase", "<u4"), ("pad", "<u4"), ("orel", "<i8")])
GROUP_ENT = np.dtype([("tbase", "<u4"), ("rows", "<u2"), ("cols", "<u2"), ("orel", "<i8"), ("ku", "<u4"),
                      ("pad", "<u4")])
IDS = [r.id for r in TC.ROWS]


def _chain(row):
    chunk = TC.tile_chunk(row)
    codecs = ([{"name": "transpose", "configuration": {"order": list(row.order)}}] if row.order else []) + \
        [row.endian] + ([CRCJ] if row.crc else [])
    spec = ArraySpec(tuple(chunk), np.dtype(row.dtype), row.fill)
    return P.analyze_chain(C.parse_codecs(codecs), spec), spec


def _layout(row, array=None):
    """The row's zhip_layout, built as planner.plan_decode builds it for the
    row's chain read into a whole-array out."""
    chain, spec = _chain(row)
    shape, it, ost = TC.stored_geometry(row, array)
    assert shape == tuple(spec.shape[p] for p in chain.perm)
    flags = (N.LF_CRC if chain.crc else 0) | (N.LF_SWAP if chain.swap else 0)
    return P._make_layout(shape, it, ost, flags, spec.fill_bytes())


def _region(plan, name):
    offsets, counts = plan.table_regions()
    i = len(ROW_REGIONS) + TILE_REGIONS.index(name)
    return plan.table_image(1)[offsets[i]: offsets[i] + counts[i]]


@pytest.mark.parametrize("rid", IDS)
def test_kernel_flags_name_the_rows_family(rid):
    """PK_TILE for every row; PK_TILE4 exactly for the tile4 family (and
    PK_TILE4_ENCODE with it: T <= 64 at these chunk sizes); PK_TILEG set for
    grouped rows and clear for general ones -- and the restatement's own
    reading of the rules gives the same family."""
    row = TC.BY_ID[rid]
    shape, it, ost = TC.stored_geometry(row)
    kf = N.Plan(_layout(row), upload=False).kernel_flags
    assert kf & N.PK_TILE
    if row.inner is not None:  # sharded rows name only the prefix
        return
    fam = TC.FAMILY_OF[row.decode]
    assert TC.family(shape, it, ost) == fam
    assert bool(kf & N.PK_TILE4) == (fam == "tile4")
    assert bool(kf & N.PK_TILE4_ENCODE) == (fam == "tile4")
    if fam != "tile4":
        assert bool(kf & N.PK_TILEG) == (fam == "grouped")
    if row.encode is not None:
        assert row.encode == {"tile4": TC.E2 if row.crc else TC.E4, "grouped": TC.EG, "general": TC.EGEN}[fam]
    assert row.decode == {"tile4": TC.T2W if row.crc else TC.T4, "grouped": TC.TG2W if row.crc else TC.TG,
                          "general": TC.TGEN}[fam]


def _whole_items(row, array):
    chunk = row.chunk
    grid = [-(-a // c) for a, c in zip(array, chunk)]
    for i, ix in enumerate(np.ndindex(*grid)):
        lo = [c * k for c, k in zip(ix, chunk)]
        n = [min(k, a - o) for k, a, o in zip(chunk, array, lo)]
        yield i, lo, n


@pytest.mark.parametrize("rid", [r.id for r in TC.ROWS if r.inner is None])
def test_planner_yields_tile_for_whole_selections(rid):
    """plan_decode and plan_encode choose tile mode for the row's whole-array
    read / write (both the native and the Python planner)."""
    row = TC.BY_ID[rid]
    chain, spec = _chain(row)
    array = TC.array_shape(row)
    it = spec.dtype.itemsize
    ostr = TC.f_strides(array, it) if row.order is None else TC.c_strides(array, it)
    blob = int(np.prod(row.chunk)) * it + (4 if row.crc else 0)
    items, enc = [], []
    for i, lo, n in _whole_items(row, array):
        csel = tuple(slice(0, k, 1) for k in n)
        items.append((i * 2 * blob, blob, i == 1, csel, tuple(slice(o, o + k, 1) for o, k in zip(lo, n))))
        enc.append((i * 2 * blob, csel, lo))
    for native in (True, False):
        old, P.NATIVE_PLANNER = P.NATIVE_PLANNER, native
        try:
            t = P.plan_decode(chain, spec, items, ostr, 0, ())
        finally:
            P.NATIVE_PLANNER = old
        assert t.tile and not t.fast and not t.rows
        assert bytes(t.layout) == bytes(_layout(row))
    t = P.plan_encode(chain, spec, enc, ostr, 0)
    assert t.tile and not t.tile_prefix


@pytest.mark.parametrize("rid", [r.id for r in TC.RAGGED])
def test_planner_yields_tile_prefix_for_ragged_edges(rid):
    """A whole write of a ragged array: the batch holds prefix-box edge chunks,
    so plan_encode chooses tile_prefix (k_encode_tile), not tile."""
    rg = TC.RAGGED[[r.id for r in TC.RAGGED].index(rid)]
    row = TC.Row(rg.id, rg.chunk, rg.order, rg.dtype, rg.endian, True, None, None, None)
    chain, spec = _chain(row)
    it = spec.dtype.itemsize
    enc = [(i << 20, tuple(slice(0, k, 1) for k in n), lo) for i, lo, n in _whole_items(row, rg.shape)]
    assert any(tuple(s.stop for s in e[1]) != tuple(rg.chunk) for e in enc)
    t = P.plan_encode(chain, spec, enc, TC.c_strides(rg.shape, it), 0)
    assert t.tile_prefix and not t.tile
    kf = N.Plan(_layout(row, rg.shape), upload=False).kernel_flags
    assert kf & N.PK_TILE


@pytest.mark.parametrize("rid", IDS)
def test_host_built_maps_equal_the_restatement(rid):
    """t_kunit[ti] is x^(8 (max base - base[ti])) for the restatement's tile ti
    (the kernels index it by the tile number they derive coordinates from, so
    this pins the order of the other-dim chain); tile4_map holds every tile's
    stored origin once, in that order, with the restatement's out offset;
    g_map holds the first tile of each group of four along gd, once each, with
    its out offset and extents."""
    row = TC.BY_ID[rid]
    shape, it, ost = TC.stored_geometry(row)
    ts = TC.tiles(shape, it, ost)
    plan = N.Plan(_layout(row), upload=False)
    by_base = {t.s_off: t for t in ts}
    assert len(by_base) == len(ts)
    top = max(by_base)
    kunit = _region(plan, "t_kunit")
    assert len(kunit) == len(ts)
    assert [int(k) for k in kunit] == [TC.xpow8(top - t.s_off) for t in ts]
    kf = plan.kernel_flags
    tmap = _region(plan, "tile4_map").view(TILE_ENT)
    if kf & N.PK_TILE4:
        assert [int(b) for b in tmap["tbase"]] == [t.s_off for t in ts]
        assert [int(o) for o in tmap["orel"]] == [t.o_off for t in ts]
        assert not tmap["pad"].any()
    else:
        assert len(tmap) == 0
    gmap = _region(plan, "g_map").view(GROUP_ENT)
    gd = TC.group_dim(shape, it, ost)
    if gd is None:
        assert len(gmap) == 0
        return
    tq = TC.find_tq(shape, it, ost)
    others = [d for d in range(len(shape) - 1) if d != tq]
    firsts = [t for t in ts if t.coords[others.index(gd)] % 4 == 0]
    assert len(gmap) == len(ts) // 4 == len(firsts)
    assert sorted(int(b) for b in gmap["tbase"]) == sorted(t.s_off for t in firsts)
    for e in gmap:
        t = by_base[int(e["tbase"])]
        assert (int(e["orel"]), int(e["rows"]), int(e["cols"])) == (t.o_off, t.rows, t.cols)
        # the group's other three tiles follow at the gd stride, in the stored chunk and in out
        sstride = TC.c_strides(shape, it)
        for j in range(1, 4):
            u = by_base[t.s_off + j * sstride[gd]]
            assert u.o_off == t.o_off + j * ost[gd] and (u.rows, u.cols) == (t.rows, t.cols)


def test_restatement_orders_tiles_as_documented():
    """The restatement itself, on a hand-worked 4-D case: stored (20, 3, 5, 40)
    float32, out strides of decoded (3, 5, 40, 20) -> tile 7 is other coords
    (1, 2): 7 = 1 * 5 + 2."""
    row = TC.BY_ID["r4_gen-f32le"]
    shape, it, ost = TC.stored_geometry(row)
    assert shape == (20, 3, 5, 40) and TC.find_tq(shape, it, ost) == 0
    ts = TC.tiles(shape, it, ost)
    assert len(ts) == 15 and ts[7].coords == (1, 2)
    assert ts[7].s_off == (1 * 5 * 40 + 2 * 40) * 4 and (ts[7].rows, ts[7].cols) == (20, 160)
    a = TC.array_shape(row)  # decoded (6, 5, 40, 40): stored dim 1 <- decoded 0, stored dim 2 <- decoded 1
    assert ts[7].o_off == (1 * a[1] * a[2] * a[3] + 2 * a[2] * a[3]) * 4
    # x^(8 n): the CRC register over n zero bytes (zlib's crc32_combine convention), against a bytewise walk
    r = 0x80000000
    for _ in range(8 * 37):
        r = (r >> 1) ^ (0x82F63B78 if r & 1 else 0)
    assert TC.xpow8(37) == r
