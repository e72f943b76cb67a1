"""The device-planned orthogonal axes on the CPU: zhip_emulate_axis (the
kernels' located-index function over host memory) against what the host route
builds for the same indices -- _ortho_dim + fancy.normalize(dedupe=keep-last)
+ SelectTables.add against the same slot layout.  Per touched chunk the counts,
the box bounds and the multisets of (A, B) pairs are equal.  Then the limits,
SelectTables.add_product's validation, and a whole selection gathered and
scattered on the host through add_product items over hook-built tables."""

import itertools

import numpy as np
import pytest

import axis_cases as AC
from zarr_hip import _native as N
from zarr_hip import axes as A
from zarr_hip import fancy
from zarr_hip.indexing import _ortho_dim

OK_CASES = [k for k, c in AC.CASES.items() if not c.err]
ERR_CASES = [k for k, c in AC.CASES.items() if c.err]


def host_route(case: AC.Case) -> dict:
    """{chunk: (count, lo, hi, sorted pairs)} from the host route: the chunk's
    slot at byte 0 (the slot side of a pair is then an offset inside one slot,
    as the device table holds it), out / value at byte 0 with the case's stride."""
    n = case.n
    scalar = case.write and case.stride == 0
    slot_bytes = case.chunk * case.slot_stride
    lin_bytes = max((n - 1) * case.stride, 0) + AC.ITEMSIZE
    out = {}
    for cix, csel, osel in _ortho_dim(case.x, case.length, case.chunk)[0]:
        nz = fancy.normalize((csel,), (osel,), (), (case.chunk,), None if scalar else (n,), dedupe=case.keep_last)
        tabs = fancy.SelectTables(AC.ITEMSIZE, *((lin_bytes, slot_bytes) if case.write else (slot_bytes, lin_bytes)))
        tabs.add(nz, 0, [case.slot_stride], 0, None if scalar else [case.stride], write=case.write)
        (t,) = tabs.tables
        assert tabs.items[0]["a_base"] == 0 and tabs.items[0]["b_base"] == 0
        out[int(cix)] = (nz.dims[0].count, nz.box[0][0], nz.box[0][1] - 1, t[np.lexsort((t[:, 1], t[:, 0]))])
    return out


@pytest.mark.parametrize("name", OK_CASES)
def test_hook_agrees_with_the_host_route(name):
    case = AC.CASES[name]
    counts, lo, hi, err, first, cursor, table, _ = AC.run_hook(case)
    assert err == 0
    want = host_route(case) if case.n else {}
    want_counts = np.zeros(case.grid, np.int64)
    for c, w in want.items():
        want_counts[c] = w[0]
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(cursor, counts)
    assert np.array_equal(first, np.cumsum(want_counts) - want_counts)
    got = AC.chunk_pairs(table, case.table_off, first, counts)
    assert sorted(got) == sorted(want)
    for c, (_, wlo, whi, pairs) in want.items():
        assert (lo[c], hi[c]) == (wlo, whi), (name, c)
        assert np.array_equal(got[c], pairs), (name, c)
    used = case.table_off + int(counts.sum())
    assert (table[:case.table_off] == -7).all() and (table[used:] == -7).all()


@pytest.mark.parametrize("name", [k for k in OK_CASES if AC.CASES[k].keep_last])
def test_keep_last_keeps_the_largest_k_of_every_element(name):
    case = AC.CASES[name]
    counts, _, _, _, first, _, table, last = AC.run_hook(case)
    w = case.wrapped()
    winners = {}
    for k, v in enumerate(w):
        winners[int(v)] = k
    assert int(counts.sum()) == len(winners)
    lin = table[case.table_off:case.table_off + len(winners), 0 if case.write else 1]
    slot = table[case.table_off:case.table_off + len(winners), 1 if case.write else 0]
    assert sorted(lin // case.stride) == sorted(winners.values())
    by_k = {int(k): int(s) for k, s in zip(lin // case.stride, slot)}
    for v, k in winners.items():
        assert last[v] == k + 1
        assert by_k[k] == (v % case.chunk) * case.slot_stride
    assert not last[np.setdiff1d(np.arange(case.length), w)].any()


@pytest.mark.parametrize("name", ERR_CASES)
def test_out_of_range_indices_set_the_axis_bit_and_count_nowhere(name):
    case = AC.CASES[name]
    counts, _, _, err, first, cursor, table, _ = AC.run_hook(case)
    assert err == case.err == case.err_bit
    good = case.x[(case.x >= -case.length) & (case.x < case.length)]
    ok = AC.Case(case.length, case.chunk, good, keep_last=case.keep_last)
    assert np.array_equal(counts, AC.run_hook(ok)[0])
    assert (table == -7).all() and (cursor == 0).all() and (first == 0xDEAD).all()  # nothing further
    with pytest.raises(IndexError, match=f"index out of bounds for dimension with length {case.length}"):
        _ortho_dim(case.x, case.length, case.chunk)


def test_geometries_past_the_limits_are_refused_before_any_launch():
    case = AC.CASES["L100-C16"]
    x = np.ascontiguousarray(case.x)
    words = np.zeros(64, np.uint32)
    tab = np.zeros((case.n, 2), np.int64)
    w = words.ctypes.data
    L = N.lib()

    def calls(g, n=case.n, keep_last=False):
        last = w if keep_last else None
        # the device entry points with host pointers: a refusal launches nothing and touches nothing
        rc = {L.zhip_axis_count(g.ctypes.data, x.ctypes.data, n, last, w, w, w, w, None),
              L.zhip_axis_fill(g.ctypes.data, x.ctypes.data, n, last, w, w, tab.ctypes.data, case.n, None),
              L.zhip_emulate_axis(g.ctypes.data, x.ctypes.data, n, int(keep_last), w, w, w, w, w, w, w,
                                  tab.ctypes.data, case.n)}
        if keep_last:
            rc.add(L.zhip_axis_last(g.ctypes.data, x.ctypes.data, n, w, None))
        assert len(rc) == 1 and not words.any()
        return rc.pop()

    assert calls(case.geom(), 1 << 31) == N.E_UNSUPPORTED
    g = case.geom()
    g["length"], g["grid"] = 1 << 31, 1 << 27
    assert calls(g) == N.E_UNSUPPORTED
    assert calls(A.axis_geom(N.AXIS_MAX_GRID + 1, 1)) == N.E_UNSUPPORTED
    assert calls(A.axis_geom(N.AXIS_LAST_MAX_LEN + 1, 64), keep_last=True) == N.E_UNSUPPORTED
    g = case.geom()
    g["div"] = N.fdiv(15)
    assert calls(g) == N.E_INVALID
    g = case.geom()
    g["grid"] += 1
    assert calls(g) == N.E_INVALID
    g = case.geom()
    g["write"] = 2
    assert calls(g) == N.E_INVALID
    assert not A.within_limits(1 << 31, 10, 1) and not A.within_limits(1, 1 << 31, 1 << 20)
    assert not A.within_limits(1, N.AXIS_MAX_GRID + 1, 1) and A.within_limits(1, N.AXIS_MAX_GRID, 1)
    assert A.within_limits(1, N.AXIS_LAST_MAX_LEN + 1, 64) and not A.within_limits(1, N.AXIS_LAST_MAX_LEN + 1, 64, True)
    assert A.within_limits(N.AXIS_MAX_N, N.AXIS_LAST_MAX_LEN, 64, True)


def test_add_product_validates_both_buffers():
    slot, out = 16 * 20 * 4, 6 * 9 * 4  # a (16, 20) float32 slot; a (6, 9) out
    cstr, ostr = [80, 4], [36, 4]

    def tabs():
        return fancy.SelectTables(4, 2 * slot, out)

    ok = [A.TableDim(4, 10, 3, 15, 6, 0), A.AffineDim(9, 2, 2, 1, 0)]
    t = tabs()
    t.add_product(ok, slot, cstr, ostr)
    (rec,) = t.items
    assert rec["ndim"] == 2 and rec["total"] == 36 and rec["a_base"] == slot and rec["b_base"] == 0
    assert rec["dims"][0]["table"] == 1 and rec["dims"][0]["table_off"] == 10 and rec["dims"][0]["count"] == 4
    assert tuple(rec["dims"][1][k] for k in ("a0", "sa", "b0", "sb", "table")) == (8, 8, 0, 4, 0)
    t = fancy.SelectTables(4, out, 2 * slot)
    t.add_product(ok, slot, cstr, ostr, write=True)  # the two sides change places
    assert t.items[0]["b_base"] == slot and tuple(t.items[0]["dims"][1][k] for k in ("a0", "sa", "b0", "sb")) == (0, 4, 8, 8)
    t = tabs()
    t.add_product([A.TableDim(1, 0, 0, 0, 6, 0), A.AffineDim(1, 19, 1, None, 0)], 0, cstr, ostr)  # an integer: folded
    assert t.items[0]["ndim"] == 1 and t.items[0]["a_base"] == 76 and t.items[0]["total"] == 1
    for bad, what in (
            ([A.TableDim(4, 10, 3, 16, 6, 0), A.AffineDim(9, 2, 2, 1, 0)], "source"),       # hi past the second slot
            ([A.TableDim(4, 10, 3, 15, 7, 0), A.AffineDim(9, 2, 2, 1, 0)], "destination"),  # n past out's rows
            ([A.TableDim(4, 10, 3, 15, 6, 0), A.AffineDim(9, 4, 2, 1, 0)], "source"),       # the slice past the slot
            ([A.TableDim(4, 10, 3, 15, 6, 0), A.AffineDim(9, 2, 2, 1, 1)], "destination"),  # the out slice past out
    ):
        with pytest.raises(IndexError, match=f"outside its {what} buffer"):
            tabs().add_product(bad, slot, cstr, ostr)
    with pytest.raises(IndexError, match="outside its destination buffer"):
        fancy.SelectTables(4, out, 2 * slot).add_product(ok, 2 * slot, cstr, ostr, write=True)
    with pytest.raises(IndexError, match="table dimension"):
        tabs().add_product([A.TableDim(7, 10, 3, 15, 6, 0), A.AffineDim(9, 2, 2, 1, 0)], slot, cstr, ostr)
    t = tabs()
    t.add_product([A.TableDim(4, 10, 3, 15, 6, 0), A.AffineDim(0, 2, 2, 1, 0)], slot, cstr, ostr)  # nothing selected
    assert not t.items


# ------------------------------------------- a whole selection on the host
def _plan(shape, chunks, sel, keep_last, cstr, lin, write):
    """What DeviceOrthogonalIndexer + build_table produce, from the hook: per
    dimension [(chunk, dim)], and the shared table."""
    dims, tables, off, oax = [], [], 0, 0
    for d, (s, L, C) in enumerate(zip(sel, shape, chunks)):
        if isinstance(s, np.ndarray):
            case = AC.Case(L, C, s, write=write, stride=0 if lin is None else lin[oax], keep_last=keep_last)
            g = A.axis_geom(L, C, 1 << d, cstr[d], case.stride, 0, write)
            counts, low, hi, first, cursor = (np.zeros(case.grid, np.uint32) for _ in range(5))
            err, last = np.zeros(1, np.uint32), np.zeros(L, np.uint32)
            t = np.zeros((max(case.n, 1), 2), np.int64)
            N.check(N.lib().zhip_emulate_axis(g.ctypes.data, s.ctypes.data, case.n, int(keep_last), last.ctypes.data,
                                              counts.ctypes.data, low.ctypes.data, hi.ctypes.data, err.ctypes.data,
                                              first.ctypes.data, cursor.ctypes.data, t.ctypes.data, case.n), "hook")
            assert not err[0]
            dims.append([(int(c), A.TableDim(int(counts[c]), off + int(first[c]), C - 1 - int(low[c]), int(hi[c]),
                                             case.n, oax)) for c in np.nonzero(counts)[0]])
            tables.append(t[:case.n])
            off += case.n
            oax += 1
        else:
            proj, _, is_int = _ortho_dim(s, L, C)
            dims.append([(int(c), A.DeviceOrthogonalIndexer._affine(cs, os, None if is_int else oax)) for c, cs, os in proj])
            oax += 0 if is_int else 1
    return dims, np.ascontiguousarray(np.concatenate(tables))


def _run_items(tabs, table, a, b):
    items, _, prefix, n_tiles = tabs.finish()
    N.check(N.lib().zhip_emulate_select_copy(items.ctypes.data, len(items), table.ctypes.data, len(table),
                                             prefix.ctypes.data, n_tiles, a.ctypes.data, a.nbytes, b.ctypes.data,
                                             b.nbytes, 4), "zhip_emulate_select_copy")


def _strides(shape):
    st = [4] * len(shape)
    for d in range(len(shape) - 2, -1, -1):
        st[d] = st[d + 1] * shape[d + 1]
    return st


def _chunks_of(full, chunks, coords):
    """The chunk at coords as a chunk-shaped slot (zero past the array's edge)."""
    slot = np.zeros(chunks, full.dtype)
    part = full[tuple(slice(c * n, (c + 1) * n) for c, n in zip(coords, chunks))]
    slot[tuple(slice(0, n) for n in part.shape)] = part
    return slot


SELECTIONS = {
    "rows": lambda r: (r.integers(-50, 50, 40), slice(None), slice(2, 25, 3)),
    "two-axes-int": lambda r: (r.integers(-50, 50, 30), 5, r.integers(-29, 29, 17)),
    "all-axes": lambda r: (r.integers(0, 50, 9), r.integers(0, 37, 8), r.integers(0, 29, 7)),
}


@pytest.mark.parametrize("name", SELECTIONS)
def test_add_product_items_gather_and_scatter_like_numpy(name):
    rng = np.random.default_rng(5)
    shape, chunks = (50, 37, 29), (16, 7, 10)
    full = rng.integers(0, 1 << 30, shape).astype(np.int32)
    sel = tuple(np.ascontiguousarray(s, np.int64) if isinstance(s, np.ndarray) else s for s in SELECTIONS[name](rng))
    mesh = np.ix_(*[np.arange(n)[s] if isinstance(s, slice) else [s] if isinstance(s, int) else s
                    for s, n in zip(sel, shape)])
    drop = tuple(i for i, s in enumerate(sel) if isinstance(s, int))
    want = np.squeeze(full[mesh], axis=drop)
    cstr, slot_bytes = _strides(chunks), int(np.prod(chunks)) * 4
    # read: every touched chunk's slot in one scratch, gathered into out
    out = np.full(want.shape, -1, np.int32)
    dims, table = _plan(shape, chunks, sel, False, cstr, _strides(want.shape), False)
    combos = list(itertools.product(*dims))
    scratch = np.stack([_chunks_of(full, chunks, tuple(c[0] for c in combo)) for combo in combos])
    tabs = fancy.SelectTables(4, scratch.nbytes, out.nbytes)
    for j, combo in enumerate(combos):
        tabs.add_product([c[1] for c in combo], j * slot_bytes, cstr, _strides(want.shape))
    _run_items(tabs, table, scratch, out)
    assert np.array_equal(out, want)
    # write an array value with repeats: the last occurrence along each axis wins, as in numpy
    value = rng.integers(0, 1 << 30, want.shape).astype(np.int32)
    expect = full.copy()
    expect[mesh] = np.expand_dims(value, drop)
    dims, table = _plan(shape, chunks, sel, True, cstr, _strides(want.shape), True)
    combos = list(itertools.product(*dims))
    scratch = np.stack([_chunks_of(full, chunks, tuple(c[0] for c in combo)) for combo in combos])
    tabs = fancy.SelectTables(4, value.nbytes, scratch.nbytes)
    for j, combo in enumerate(combos):
        tabs.add_product([c[1] for c in combo], j * slot_bytes, cstr, _strides(want.shape), write=True)
    _run_items(tabs, table, value, scratch)
    for j, combo in enumerate(combos):
        coords = tuple(c[0] for c in combo)
        assert np.array_equal(scratch[j], _chunks_of(expect, chunks, coords)), (name, coords)
