"""Orthogonal, coordinate and mask selections without a GPU: the restated
indexers against numpy, the normaliser (zarr_hip.fancy) through the CPU hook
zhip_emulate_select_copy (the kernel's tile walk and address arithmetic over
host memory) against numpy, the rejected forms by name, validation before any
copy, write dedupe, and the tile decomposition."""

import numpy as np
import pytest

from zarr_hip import _native as N
from zarr_hip import fancy
from zarr_hip.indexing import (CoordinateIndexer, MaskIndexer, OrthogonalIndexer, is_pure_fancy_indexing,
                               is_pure_orthogonal_indexing)


def _chunks(a: np.ndarray, chunk_shape) -> dict:
    """Full-size chunks of `a` (boundary chunks padded with -1)."""
    grid = tuple(-(-n // c) for n, c in zip(a.shape, chunk_shape))
    out = {}
    for co in np.ndindex(*grid):
        ch = np.full(chunk_shape, -1, a.dtype)
        src = a[tuple(slice(i * c, (i + 1) * c) for i, c in zip(co, chunk_shape))]
        ch[tuple(slice(0, s) for s in src.shape)] = src
        out[co] = ch
    return out


def _assemble(indexer, a, chunk_shape) -> np.ndarray:
    """out[osel] = squeeze(chunk[csel], drop_axes) over the indexer's
    projections, with plain numpy (what the reference's scatter_chunk does)."""
    chunks = _chunks(a, chunk_shape)
    out = np.full(indexer.shape, -7, a.dtype)
    for co, csel, osel, _ in indexer:
        sel = chunks[co][csel]
        if indexer.drop_axes:
            sel = sel.squeeze(axis=indexer.drop_axes)
        out[osel] = sel
    return out


def _np_oindex(a, selection):
    sel = [np.asarray(s) if isinstance(s, list) else s for s in selection]
    sel += [slice(None)] * (a.ndim - len(sel))
    drop = tuple(i for i, s in enumerate(sel) if isinstance(s, (int, np.integer)))
    mesh = np.ix_(*[np.arange(n)[s] if isinstance(s, slice) else [s] if isinstance(s, (int, np.integer))
                    else (np.nonzero(s)[0] if s.dtype == bool else s) for s, n in zip(sel, a.shape)])
    return a[mesh].squeeze(axis=drop) if drop else a[mesh]


GEOMS = [((23,), (5,)), ((13, 9), (4, 4)), ((11, 7, 9), (4, 3, 5)), ((6, 5, 7, 4), (4, 2, 3, 3))]


def _rand_dim_sel(rng, n, kind):
    if kind == "int":
        return int(rng.integers(-n, n))
    if kind == "slice":
        a, b = sorted(rng.integers(0, n + 1, 2))
        return slice(int(a), int(b), int(rng.integers(1, 4)))
    if kind == "sorted":
        return np.sort(rng.integers(0, n, rng.integers(1, 2 * n)))
    if kind == "decreasing":
        return np.sort(rng.choice(n, rng.integers(1, n + 1), replace=False))[::-1].copy()
    if kind == "unsorted":
        return rng.integers(-n, n, rng.integers(2, 2 * n + 2))
    if kind == "list":
        return [int(v) for v in rng.integers(0, n, 3)]
    if kind == "mask":
        return rng.random(n) < 0.4
    if kind == "nomask":
        return np.zeros(n, bool)
    raise AssertionError(kind)


@pytest.mark.parametrize("shape,chunks", GEOMS)
def test_orthogonal_indexer_against_numpy(shape, chunks):
    rng = np.random.default_rng(len(shape))
    a = rng.integers(0, 1 << 30, shape).astype(np.int64)
    kinds = ["int", "slice", "sorted", "decreasing", "unsorted", "list", "mask", "nomask"]
    for trial in range(60):
        sel = tuple(_rand_dim_sel(rng, n, kinds[int(rng.integers(len(kinds)))]) for n in shape)
        if trial % 7 == 0:  # fewer entries than dimensions
            sel = sel[: max(1, len(sel) - 1)]
        ix = OrthogonalIndexer(sel, shape, chunks)
        want = _np_oindex(a, sel)
        assert ix.shape == want.shape
        got = _assemble(ix, a, chunks)
        assert np.array_equal(got, want), sel


@pytest.mark.parametrize("shape,chunks", GEOMS)
def test_coordinate_and_mask_indexers_against_numpy(shape, chunks):
    rng = np.random.default_rng(10 + len(shape))
    a = rng.integers(0, 1 << 30, shape).astype(np.int64)
    for trial in range(30):
        n = int(rng.integers(1, 40))
        coords = tuple(rng.integers(-s, s, n) for s in shape)  # negative, unsorted, repeated
        if trial % 3 == 0:
            coords = tuple(np.sort(np.abs(c)) % s for c, s in zip(coords, shape))
        if trial % 5 == 0 and n % 2 == 0:  # 2-d coordinate arrays: sel_shape
            coords = tuple(c.reshape(2, -1) for c in coords)
        ix = CoordinateIndexer(coords, shape, chunks)
        got = _assemble(ix, a, chunks).reshape(ix.sel_shape)
        assert np.array_equal(got, a[coords])
    for p in (0.0, 0.3, 1.0):  # an all-false mask too
        mask = rng.random(shape) < p
        ix = MaskIndexer(mask, shape, chunks)
        assert np.array_equal(_assemble(ix, a, chunks).reshape(ix.sel_shape), a[mask])
    with pytest.raises(IndexError):
        CoordinateIndexer(tuple(np.array([s]) for s in shape), shape, chunks)
    with pytest.raises(IndexError):
        MaskIndexer(np.zeros(tuple(s + 1 for s in shape), bool), shape, chunks)


def test_dispatch_predicates():
    assert is_pure_fancy_indexing(np.array([1, 2]), 1) and is_pure_fancy_indexing(np.zeros((3, 3), bool), 2)
    assert is_pure_fancy_indexing((np.array([1, 2]), 0), 2) and not is_pure_fancy_indexing((np.array([1]), slice(3)), 2)
    assert is_pure_orthogonal_indexing((np.array([1, 2]), slice(3)), 2)
    assert is_pure_orthogonal_indexing(([1, 2], [True, False, True]), 2)
    assert not is_pure_orthogonal_indexing((np.array([1]), np.array([2]), slice(1)), 3)


# ------------------------------------------------- normaliser + CPU hook
def _run(items, chunk_list, out, drop_axes=(), write=False, value=None, dedupe=None):
    """The route's table building over host arrays: chunks stacked as slots of
    one scratch array, one hook call for every item.  read: scratch -> out;
    write: value -> scratch."""
    cshape = chunk_list[0].shape
    scratch = np.ascontiguousarray(np.stack(chunk_list).reshape((-1,) + cshape[1:]))
    other = value if write else out
    scalar = write and np.ndim(value) == 0
    if scalar:
        other = np.asarray(value, scratch.dtype).reshape(1)
    isz = scratch.dtype.itemsize
    sizes = (other.nbytes, scratch.nbytes) if write else (scratch.nbytes, other.nbytes)
    tabs = fancy.SelectTables(isz, *sizes)
    slot = chunk_list[0].nbytes
    for j, (csel, osel) in enumerate(items):
        nz = fancy.normalize(csel, osel, drop_axes, cshape, None if scalar else other.shape,
                             dedupe=write if dedupe is None else dedupe)
        tabs.add(nz, j * slot, chunk_list[0].strides, 0, None if scalar else other.strides, write=write)
    a, b = (other, scratch) if write else (scratch, other)
    assert a.flags.c_contiguous and b.flags.c_contiguous
    tabs.run_host(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))
    return scratch.reshape((len(chunk_list),) + cshape)


@pytest.mark.parametrize("dtype", ["u1", "<u2", "<f4", "<f8"])
def test_accepted_forms_match_numpy(dtype):
    rng = np.random.default_rng(3)
    ch = (rng.random((8, 6, 5)) * 200).astype(dtype)
    mask = np.array([True, False, True, True, False, False])
    cases = [
        # (chunk_selection, out_selection, drop_axes, out shape)
        ((slice(1, 7, 2), np.array([5, 0, 3]), slice(0, 5)), (slice(2, 5), slice(0, 3), slice(0, 5)), (), (6, 3, 5)),
        ((slice(0, 8), mask, slice(1, 4)), (slice(0, 8), slice(1, 4), slice(0, 3)), (), (8, 5, 3)),
        ((slice(0, 8), [1, 4], slice(0, 5)), (slice(0, 8), np.array([3, 0]), slice(0, 5)), (), (8, 4, 5)),
        (np.ix_([7, 2, 2], [0, 5], [4, 1, 0, 3]), (slice(0, 3), slice(1, 3), slice(0, 4)), (), (3, 3, 4)),
        (np.ix_([7, 2], [3], [4, 1, 0]), (slice(0, 2), slice(0, 3)), (1,), (2, 3)),
        (np.ix_([7, 2], [3], [4, 1, 0]), np.ix_([1, 0], [2, 0, 4]), (1,), (2, 5)),
        ((np.array([0, 7, 3, 3]), np.array([5, 0, 2, 2]), np.array([4, 4, 0, 1])), slice(1, 5), (), (6,)),
        ((np.array([0, 7, 3]), np.array([5, 0, 2]), np.array([4, 4, 0])), np.array([2, 0, 1]), (), (3,)),
        ((slice(0, 8), 2, slice(0, 5)), (slice(0, 8), slice(0, 5)), (), (8, 5)),  # basic, through the same tables
    ]
    for csel, osel, drop, oshape in cases:
        out = np.full(oshape, 9, dtype)
        want = out.copy()
        sel = ch[tuple(np.asarray(s) if isinstance(s, list) else s for s in csel)]
        want[osel] = sel.squeeze(axis=drop) if drop else sel
        _run([(csel, osel)], [ch], out, drop)
        assert np.array_equal(out.view(np.uint8), want.view(np.uint8)), (csel, osel)


def test_one_dimensional_chunk_forms():
    ch = np.arange(10, dtype="<u2") * 3
    for csel, osel in [((np.array([9, 0, 4]),), (slice(0, 3),)), ((np.array([9, 0, 4]),), slice(0, 3)),
                       ((np.array([9, 0, 4]),), np.array([2, 1, 0])), ((ch % 2 == 0,), (slice(0, 5),))]:
        out = np.zeros(5, "<u2")
        want = out.copy()
        want[osel] = ch[csel]
        _run([(csel, osel)], [ch], out)
        assert np.array_equal(out, want)


def test_rejected_forms_raise_by_name():
    cs, os_ = (8, 6, 5), (8, 6, 5)
    full = (slice(0, 8), slice(0, 6), slice(0, 5))
    bad = [
        ((np.array([1, 2]), np.array([0, 1]), slice(0, 5)), full, "pointwise arrays mixed with slices"),
        ((np.zeros((8, 6), bool), slice(0, 5), slice(0, 5)), full, "N-d masks"),
        ((np.array([1, 2]), 3, slice(0, 5)), full, "integer next to a bare array"),
        ((np.zeros((2, 2), int), np.zeros((2, 2), int), np.zeros((2, 2), int)), full, "mixed or N-d shapes"),
        (np.array([1, 2]), full, "bare ndarray"),
        ((slice(0, 8), np.array([1.5]), slice(0, 5)), full, "dtype float64"),
        ((slice(0, 2), np.array([1, 2]), slice(0, 5)), (np.array([0, 1]), np.array([0, 1]), slice(0, 5)),
         "more than one integer array in an out selection"),
        ((slice(0, 2), np.array([1, 2]), slice(0, 5)), (slice(0, 2), 3, slice(0, 5)), "integers or boolean arrays in an out"),
    ]
    for csel, osel, name in bad:
        with pytest.raises(NotImplementedError, match=name):
            fancy.normalize(csel, osel, (), cs, os_)


def test_out_of_range_and_mismatched_counts_raise_before_any_copy():
    ch = np.arange(8 * 6, dtype="<u2").reshape(8, 6)
    out = np.zeros((4, 6), "<u2")
    bad = [
        ((np.array([0, 8]), slice(0, 6)), (slice(0, 2), slice(0, 6)), IndexError),       # chunk index == dim
        ((np.array([0, -1]), slice(0, 6)), (slice(0, 2), slice(0, 6)), IndexError),      # negative: not wrapped here
        ((np.array([0, 1]), slice(0, 6)), (np.array([0, 4]), slice(0, 6)), IndexError),  # out index == dim
        ((np.array([0, 1, 2]), slice(0, 6)), (slice(0, 2), slice(0, 6)), ValueError),    # counts differ
        ((np.array([0, 1]), slice(0, 6)), (slice(0, 2), slice(0, 5)), ValueError),
        ((np.ones(7, bool), slice(0, 6)), (slice(0, 4), slice(0, 6)), IndexError),       # mask shorter than the chunk
        ((np.array([0, 1]), np.array([0, 1, 2])), slice(0, 2), ValueError),              # point arrays differ
        ((np.array([0, 1]), slice(0, 6)), (slice(0, 2),), ValueError),                   # out entries
    ]
    good_c, good_o = (np.array([3]), slice(0, 6)), (slice(0, 1), slice(0, 6))
    for csel, osel, exc in bad:
        before = out.copy()
        with pytest.raises(exc):
            _run([(good_c, good_o), (csel, osel)], [ch, ch], out)
        assert np.array_equal(out, before)  # the valid first item was not copied either
    with pytest.raises(ValueError, match="drop_axes"):
        fancy.normalize(np.ix_([1, 2], [3]), (slice(0, 1),), (0,), ch.shape, (1,))
    # offsets that leave a buffer are refused when the tables are built ...
    nz = fancy.normalize((np.array([7]), slice(0, 6)), (slice(0, 1), slice(0, 6)), (), ch.shape, out.shape)
    with pytest.raises(IndexError, match="outside its source buffer"):
        fancy.SelectTables(2, ch.nbytes - 2, out.nbytes).add(nz, 0, ch.strides, 0, out.strides)
    # ... and by the hook itself for tables built by hand
    t = fancy.SelectTables(2, ch.nbytes, out.nbytes)
    t.add(nz, 0, ch.strides, 0, out.strides)
    t.a_size -= 2
    with pytest.raises(N.NativeError, match="outside its buffer"):
        t.run_host(ch.view(np.uint8).reshape(-1), out.view(np.uint8).reshape(-1))
    t = fancy.SelectTables(2, ch.nbytes, out.nbytes)
    t.add(nz, 0, ch.strides, 0, out.strides)
    t.items[0]["dims"][0]["div"] = (1, 1)
    with pytest.raises(N.NativeError, match="divisor"):
        t.run_host(ch.view(np.uint8).reshape(-1), out.view(np.uint8).reshape(-1))


def test_write_scatter_and_dedupe_keeps_the_last_occurrence():
    rng = np.random.default_rng(5)
    ch = rng.integers(0, 1000, (8, 6)).astype("<i4")
    # orthogonal: per-dimension dedupe
    rows, cols = np.array([3, 1, 3, 7, 1]), np.array([5, 5, 0])
    value = rng.integers(1000, 2000, (5, 3)).astype("<i4")
    want = ch.copy()
    for i, r in enumerate(rows):      # sequential assignment: the last occurrence wins
        for j, c in enumerate(cols):
            want[r, c] = value[i, j]
    got = _run([(np.ix_(rows, cols), (slice(0, 5), slice(0, 3)))], [ch], None, write=True, value=value)[0]
    assert np.array_equal(got, want)
    nz = fancy.normalize(np.ix_(rows, cols), (slice(0, 5), slice(0, 3)), (), ch.shape, value.shape, dedupe=True)
    assert [d.count for d in nz.dims] == [3, 2]
    assert nz.dims[0].out.idx.tolist() == [2, 3, 4] and nz.dims[1].out.idx.tolist() == [1, 2]
    # point list: dedupe by flat chunk index
    pr, pc = np.array([2, 4, 2, 2, 0]), np.array([1, 1, 1, 3, 0])
    pv = np.arange(10, 15, dtype="<i4")
    want = ch.copy()
    for k in range(5):
        want[pr[k], pc[k]] = pv[k]
    got = _run([((pr, pc), slice(0, 5))], [ch], None, write=True, value=pv)[0]
    assert np.array_equal(got, want)
    # a scalar value broadcasts: its offsets are all zero
    got = _run([((slice(0, 8), np.array([1, 1, 4])), (slice(0, 8), slice(0, 3)))], [ch], None, write=True,
               value=np.int32(77))[0]
    want = ch.copy()
    want[:, [1, 4]] = 77
    assert np.array_equal(got, want)


def test_tile_decomposition_mixed_item_sizes():
    """Items of 1, 255, 256, 257, 1000 elements and around the tile size
    (ZHIP_SELECT_TILE) and its multiples in ONE call: the tile -> item prefix
    lookup, items of several tiles and the tail tile."""
    T = N.SELECT_TILE
    counts = [1, 255, 256, 257, 1000, T - 1, T, T + 1, 2 * T, 3 * T + 5, 1]
    rng = np.random.default_rng(9)
    ch = rng.integers(0, 1 << 16, (70, 64)).astype("<u2")  # 4480 elements per chunk
    items, want = [], []
    total = sum(counts)
    out = np.zeros(total, "<u2")
    at = 0
    for n in counts:
        flat = rng.choice(ch.size, n, replace=False)
        r, c = np.unravel_index(flat, ch.shape)
        items.append(((r, c), slice(at, at + n)))
        want.append(ch[r, c])
        at += n
    chunks = [np.roll(ch, j, axis=0) for j in range(len(counts))]
    _run(items, chunks, out)
    want = np.concatenate([chunks[j][items[j][0]] for j in range(len(counts))])
    assert np.array_equal(out, want)
    # the same through a 2-d product (division by the inner count) with a tail tile
    out2 = np.zeros((37, 61), "<u2")
    rows = rng.permutation(70)[:37]
    _run([((rows, slice(0, 61)), (slice(0, 37), slice(0, 61)))], [ch], out2)
    assert np.array_equal(out2, ch[rows, :61])


def test_struct_layout_matches_the_header():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "zarrhip.h")).read()
    assert int(re.search(r"#define ZHIP_SELECT_TILE (\d+)u", hdr).group(1)) == N.SELECT_TILE
    assert N.SELECT_ITEM_DT.fields["dims"][1] == 32 and N.SELECT_DIM_DT.fields["div"][1] == 48


def test_routing_detection_and_refusals_need_no_gpu():
    """any_fancy sees arrays, lists, masks and bare (non-tuple) selections and
    passes slices / integers; a mixed-spec batch with non-basic selections and
    planning a non-basic read ahead are refused by name before any device work."""
    import zarr_hip
    from zarr_hip.pipeline import HipCodecPipeline
    from zarr_hip.spec import ArraySpec

    basic = (None, None, (slice(0, 4), np.int64(1), 2), (slice(0, 4),), True)
    assert not fancy.any_fancy([basic, basic])
    for csel, osel in [((slice(0, 4), np.array([1]), 2), (slice(0, 4),)), ((slice(0, 4), [1], 2), (slice(0, 4),)),
                       ((slice(0, 4),), slice(0, 4)), ((np.zeros(4, bool),), (slice(0, 0),)),
                       ((slice(0, 4),), np.array([0, 1, 2, 3]))]:
        assert fancy.any_fancy([basic, (None, None, csel, osel, False)])
    codecs = [{"name": "bytes", "configuration": {"endian": "little"}}]
    pipe = HipCodecPipeline.from_codecs(codecs)
    s1, s2 = ArraySpec((4, 4), np.dtype("float32"), 0.0), ArraySpec((4, 3), np.dtype("float32"), 0.0)
    arrsel = (np.array([0, 2]), slice(0, 3))
    batch = [(None, s1, arrsel, (slice(0, 2), slice(0, 3)), False), (None, s2, arrsel, (slice(2, 4), slice(0, 3)), False)]
    with pytest.raises(NotImplementedError, match="mixes chunk specs"):
        pipe.read_sync(batch, np.zeros((4, 3), np.float32))
    with pytest.raises(NotImplementedError, match="mixes chunk specs"):
        pipe.write_sync(batch, np.zeros((4, 3), np.float32))
    with pytest.raises(NotImplementedError, match="prepare_read"):
        pipe.prepare_read(batch[:1], None)
    arr = zarr_hip.Array.create(zarr_hip.MemoryStore(), (10, 10), (4, 4), "float32", 0.0, codecs=codecs)
    with pytest.raises(NotImplementedError, match="prepare_read"):
        arr.prepare_read((np.array([1, 2]), slice(None)))
    assert arr._dispatch((slice(1, 3), 2)) is None and arr._dispatch(Ellipsis) is None
    assert arr._dispatch(([1, 2], slice(None))) == "oindex" and arr._dispatch((np.array([1]), np.array([2]))) == "vindex"
    assert arr._dispatch(np.zeros((10, 10), bool)) == "vindex"
