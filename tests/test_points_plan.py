"""The device-built point tables on the CPU: zhip_emulate_points (the kernels'
located-point function over host memory) against the tables the host route
builds for the same points -- CoordinateIndexer + fancy.normalize +
SelectTables.add against the same slot layout.  Per touched chunk the two
multisets of (A, B) pairs are equal, the counts are np.bincount's, and the
cursor ends equal to the counts."""

import numpy as np
import pytest

import points_cases as PC
from zarr_hip import fancy
from zarr_hip.indexing import CoordinateIndexer

OK_CASES = [k for k, c in PC.CASES.items() if not c.err]
ERR_CASES = [k for k, c in PC.CASES.items() if c.err]


def host_route_pairs(case: PC.Case) -> dict:
    """{rix: sorted pairs} from the host route: every chunk's slot at byte 0
    (A and B of the slot side are then offsets inside one slot, as the device
    table holds them), out / value at byte 0 with the case's stride."""
    ix = CoordinateIndexer(tuple(case.coords), case.shape, case.chunks)
    n = case.n
    slot_bytes = int(np.prod(case.chunks)) * PC.ITEMSIZE
    lin_bytes = max(n * max(case.stride, PC.ITEMSIZE), PC.ITEMSIZE)
    scalar = case.write and case.stride == 0
    out = {}
    for coords, csel, osel, _ in ix:
        nz = fancy.normalize(csel, osel, (), case.chunks, None if scalar else (n,))
        tabs = fancy.SelectTables(PC.ITEMSIZE, *((lin_bytes, slot_bytes) if case.write else (slot_bytes, lin_bytes)))
        tabs.add(nz, 0, case.slot_strides(), 0, None if scalar else [case.stride], write=case.write)
        (t,) = tabs.tables
        assert tabs.items[0]["a_base"] == 0 and tabs.items[0]["b_base"] == 0
        out[int(np.ravel_multi_index(coords, case.grid))] = t[np.lexsort((t[:, 1], t[:, 0]))]
    return out


@pytest.mark.parametrize("name", OK_CASES)
def test_hook_tables_equal_the_host_routes(name):
    case = PC.CASES[name]
    counts, err, first, cursor, table = PC.run_hook(case)
    assert err == 0
    want_counts = np.bincount(case.rix(), minlength=case.n_chunks) if case.n else np.zeros(case.n_chunks, np.int64)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(cursor, counts)
    assert np.array_equal(first, np.cumsum(want_counts) - want_counts)
    got = PC.chunk_pairs(table, first, counts)
    want = host_route_pairs(case) if case.n else {}
    assert sorted(got) == sorted(want)
    for r in want:
        assert np.array_equal(got[r], want[r]), (name, r)


@pytest.mark.parametrize("name", ERR_CASES)
def test_out_of_range_points_set_their_bits_and_count_nothing(name):
    case = PC.CASES[name]
    counts, err, first, cursor, table = PC.run_hook(case)
    assert err == case.err
    bad = np.zeros(case.n, bool)
    for c, s in zip(case.coords, case.shape):
        bad |= (c < -s) | (c >= s)
    good = PC.Case(case.shape, case.chunks, tuple(c[~bad] for c in case.coords))
    want = np.bincount(good.rix(), minlength=case.n_chunks) if good.n else np.zeros(case.n_chunks, np.int64)
    assert np.array_equal(counts, want)
    assert (table == -7).all() and (cursor == 0).all()  # nothing further
    with pytest.raises(IndexError, match="index out of bounds for dimension with length"):
        CoordinateIndexer(tuple(case.coords), case.shape, case.chunks)


def test_geometries_past_the_limits_are_refused():
    from zarr_hip import _native as N

    case = PC.CASES["1d"]
    coords = [np.ascontiguousarray(c) for c in case.coords]
    counts, err, first, cursor = (np.zeros(1024, np.uint32) for _ in range(4))  # the largest accepted grid here: 1000
    tab = np.zeros((case.n, 2), np.int64)

    def call(g, n=case.n):
        return N.lib().zhip_emulate_points(g.ctypes.data, PC.coord_ptrs(coords), n, counts.ctypes.data,
                                           err.ctypes.data, first.ctypes.data, cursor.ctypes.data, tab.ctypes.data)

    g = case.geom()
    assert call(g, 1 << 31) == N.E_UNSUPPORTED
    g["shape"][0], g["grid"][0] = 1 << 31, 1 << 25
    assert call(g) == N.E_UNSUPPORTED
    g = case.geom()
    g["chunk"][0], g["div"][0], g["grid"][0] = 1, N.fdiv(1), 1000
    assert call(g) == 0
    g["shape"][0] = g["grid"][0] = N.POINTS_MAX_GRID + 1
    assert call(g) == N.E_UNSUPPORTED
    g = case.geom()
    g["div"][0] = N.fdiv(63)
    assert call(g) == N.E_INVALID
    g = case.geom()
    g["grid"][0] += 1
    assert call(g) == N.E_INVALID
    from zarr_hip import points as P
    assert not P.within_limits(1 << 31, (10,), (1,)) and not P.within_limits(1, (1 << 31,), (1 << 20,))
    assert not P.within_limits(1, (N.POINTS_MAX_GRID + 1,), (1,)) and P.within_limits(1, (N.POINTS_MAX_GRID,), (1,))
