"""Every kernel family launched with destination and source byte offsets
around and beyond 2**31 and 2**32 (tests/wide_cases.py; tests/
test_wide_offsets.py proves on the CPU that each row has that property and
that no narrowed address can leave the allocations).

One module fixture allocates two backings of wide_cases.TOTAL bytes (about
6.8 GiB each, uninitialised): the out / value side and the arena side.  Each
test fills both with 0xA5 (a device fill), builds the row's strided view and
a DeviceStore whose arena is a view of the second backing, and compares

  reads   the view with the oracle's array (a donor of three distinct chunks,
          its blobs re-keyed over the row's grid), the row's kernel by name;
          one flipped bit on either side of 2**31 / 2**32 inside the blobs that
          straddle them gives ST_CRC_MISMATCH for exactly that chunk; then the
          view is overwritten with 0xA5 and the WHOLE backing, guards included,
          must be 0xA5: a store to any byte no element selects fails.
  writes  the store with the oracle's, key by key and byte by byte, at the
          placements the padding dictates; the all-fill chunk above 2**32
          elided; the value backing untouched; a partial write then merges
          into one chunk whose blob lies above 2**32.

Only chunk-sized windows cross to the host.  Nothing here is timed and nothing
has a tolerance.  The fixture skips only when the device reports less than
32 GiB free."""

import types

import numpy as np
import pytest

import value_cases as VC
import value_driver as D
import wide_cases as W
from conftest import set_tuning
from oracle import oracle as O
from test_gpu_decode import _data
from test_gpu_kernel_matrix import _flip, _kernel

pytestmark = pytest.mark.gpu

GiB = 1 << 30
DISTINCT = 3  # chunks of distinct data per row; the row's grid cycles through them


@pytest.fixture(scope="module")
def backings(device):
    import torch

    free, _ = torch.cuda.mem_get_info(device)
    if free < 32 * GiB:
        pytest.skip(f"offsets beyond 2**32: torch.cuda.mem_get_info reports {free / GiB:.1f} GiB free on the "
                    "device, less than the 32 GiB below which these tests may skip")
    b = types.SimpleNamespace(out=torch.empty(W.TOTAL, dtype=torch.uint8, device=device),
                              arena=torch.empty(W.TOTAL, dtype=torch.uint8, device=device))
    yield b
    del b.out, b.arena
    torch.cuda.empty_cache()  # 13.5 GiB go back to the device, not to the suite's cache


def _fill(b):
    b.out.fill_(W.SENTINEL)
    b.arena.fill_(W.SENTINEL)


def _all_sentinel(t) -> bool:
    """Every byte of a uint8 tensor is 0xA5 (compared eight at a time)."""
    n8 = t.numel() // 8 * 8
    word = int.from_bytes(bytes([W.SENTINEL]) * 8, "little", signed=True)
    return bool((t[:n8].view(_torch_dt("int64")) == word).all()) and bool((t[n8:] == W.SENTINEL).all())


def _torch_dt(name):
    import torch

    return getattr(torch, name)


def _strided(backing, row, dtype):
    """The row's view of the body of `backing`, in torch `dtype` (of the row's
    item size).  (No storage offset is passed: as_strided then keeps the body's.)"""
    import torch

    isz = W.itemsize(row)
    body = backing[W.FRONT + row.base: W.FRONT + W.BODY].view(dtype)
    v = torch.as_strided(body, W.array_shape(row), [s // isz for s in W.view_strides(row)])
    assert v.data_ptr() == backing.data_ptr() + W.FRONT + row.base
    return v


def _view(backing, row):
    from zarr_hip.buffer import torch_dtype

    return _strided(backing, row, torch_dtype(np.dtype(row.dtype)))


def _sentinel_over(backing, row, sel=(Ellipsis,)):
    """Overwrite the elements the view selects with 0xA5 bytes."""
    dt = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}[W.itemsize(row)]
    word = int.from_bytes(bytes([W.SENTINEL]) * W.itemsize(row), "little", signed=dt != "uint8")
    _strided(backing, row, _torch_dt(dt))[sel].fill_(word)


def _host_bytes(t) -> bytes:
    return t.contiguous().cpu().numpy().tobytes()


def _store(device, b):
    """An empty DeviceStore whose arena is the body of the arena backing: sized
    up front, so it never grows; offset 0 is the first byte behind the front guard."""
    import zarr_hip

    store = zarr_hip.DeviceStore(device, capacity=1 << 16)
    store.arena.buf = b.arena[W.FRONT: W.FRONT + W.BODY]
    assert store.arena.top == 0 and store.arena.capacity >= W.BODY - W.SLACK
    return store


def _pad_to(store, target):
    """Reserve a pad region so that the next reservation starts at `target`."""
    pad = target - store.arena.top
    assert pad >= 0 and pad % W.GRANULE == 0
    if pad:
        assert store.arena.reserve(pad) == target - pad
    assert store.arena.top == target


def _grid_axis(row):
    return 0 if row.spread == W.SLAB else 1


def _cells(row, a):
    """The array split into its grid cells."""
    return np.split(a, row.n, axis=_grid_axis(row))


_DONORS: dict = {}


def _donor(row):
    """The oracle's store and array for DISTINCT chunks of the row's geometry,
    computed once per row and shared: (meta, {donor key: blob}, data cells)."""
    if row.id not in _DONORS:
        _DONORS[row.id] = _make_donor(row)
    return _DONORS[row.id]


def _make_donor(row):
    drow = row._replace(n=DISTINCT)
    shape = W.array_shape(drow)
    meta = O.ArrayMeta(shape, W.array_chunks(drow), np.dtype(row.dtype), row.fill, codecs=W.codecs(drow))
    data = _data(shape, row.dtype, 5)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    assert sorted(host) == sorted(W.key(drow, j) for j in range(DISTINCT))
    assert all(len(v) == W.blob_len(row) for v in host.values())
    want = O.read(host, meta)
    return types.SimpleNamespace(row=drow, meta=meta, host=host, cells=_cells(drow, want))


def _blob(don, j):
    return don.host[W.key(don.row, j % DISTINCT)]


def _array(store, row):
    import zarr_hip

    return zarr_hip.Array.create(store, W.array_shape(row), W.array_chunks(row), row.dtype, row.fill,
                                 codecs=W.codecs(row))


class _ReadCase:
    """A read row on the device: the blobs of the donor, re-keyed over the
    row's grid and placed around 2**31 and 2**32; the last grid cell missing."""

    def __init__(self, device, b, row):
        self.row, self.b = row, b
        self.don = _donor(row)
        self.place = W.read_placements(row)
        self.store = _store(device, b)
        self.put(self.store, row, self.don, self.place)
        self.arr = _array(self.store, row)
        fill = np.full_like(self.don.cells[0], row.fill)
        self.want = np.concatenate([fill if c == W.dropped(row) else self.don.cells[c % DISTINCT]
                                    for c in range(row.n)], axis=_grid_axis(row))
        self.view = _view(b.out, row)

    @staticmethod
    def put(store, row, don, place, prefix=""):
        for c, (off, n) in place.items():
            _pad_to(store, off)
            store.set_sync(prefix + W.key(row, c), _blob(don, c))
            assert store.placement(prefix + W.key(row, c)) == (off, n)

    def exact(self, view=None, want=None):
        return _host_bytes(self.view if view is None else view) == \
            np.ascontiguousarray(self.want if want is None else want).tobytes()


def _entry_of(case, prog, cell, inner):
    """The table entry of grid cell `cell` (its inner chunk `inner`)."""
    projections, _ = O.basic_indexer((Ellipsis,), W.array_shape(case.row), W.array_chunks(case.row))
    item = [int(p[0][_grid_axis(case.row)]) for p in projections].index(cell)
    mine = np.asarray(prog.tables.item_of_chunk) == item
    if inner is not None:
        slot = int(np.ravel_multi_index(inner, W.inner_grid(case.row)))
        mine &= prog.tables.chunks["slot"].astype(np.int64) == slot
    (j,) = np.nonzero(mine)[0]
    return int(j)


def _corruption(case, prog):
    """One flipped bit 1000 bytes below and one 1000 bytes above 2**31 inside
    the blob that straddles it, the same at 2**32: each launch reports
    ST_CRC_MISMATCH for exactly the chunk that holds the byte."""
    from zarr_hip import _native as N

    row, d = case.row, prog.data
    blobs = {c: _blob(case.don, c) for c in case.place}
    ranges = W.src_ranges(row, case.place, blobs)
    missing = (prog.tables.chunks["flags"] & N.CF_MISSING) != 0
    hits = 0
    for bound in (W.B31, W.B32):
        for at in (bound - 1000, bound + 1000):
            owner = [(c, inner) for c, inner, a, e in ranges if a <= at < e and inner != "index"]
            assert len(owner) == 1
            j = _entry_of(case, prog, *owner[0])
            _flip(case.store, [at], [0x04])
            d.reset_errflag()
            prog.launch()
            err = d.errflag()
            codes = d.statuses()["code"]
            _flip(case.store, [at], [0x04])  # restored
            assert err & (1 << N.ST_CRC_MISMATCH) or d.flags & N.DF_DEFER  # (deferred: the verdict words alone)
            assert list(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == [j]
            assert (codes[missing] == N.ST_MISSING).all() and ((codes == N.ST_OK) | missing)[np.arange(d.n) != j].all()
            hits += 1
    assert hits == 4
    d.reset_errflag()


def _window(row):
    """A selection that cuts every chunk dimension but the last and keeps every grid cell."""
    lead = (slice(None),) if row.spread == W.SLAB else ()
    shape = W.array_shape(row)[len(lead):]
    cut = tuple(slice(1 + (d if shape[d] > 8 else 0), shape[d] - (2 if shape[d] > 4 else 1))
                for d in range(len(shape) - 1))
    return lead + cut + (slice(None),)


@pytest.mark.parametrize("row", W.READ_ROWS, ids=[r.id for r in W.READ_ROWS])
def test_read_row(device, backings, row):
    """The whole read into the wide view takes the row's kernel and is exact,
    the cell above 2**32 filled by the same launch; rows whose whole read is
    affine run it with the row map zeroed; every CRC row then reports a flipped
    bit on either side of each boundary; row-map rows also read a window that
    keeps the map; at the end no byte outside the selected elements changed."""
    from zarr_hip import _native as N

    _fill(backings)
    c = _ReadCase(device, backings, row)
    prog, out = c.arr.prepare_read((Ellipsis,), out=c.view)
    assert out is c.view and prog.index is None
    assert (prog.data.p_rowmap is not None) == row.rowmap and bool(prog.data.n_idx) == row.index
    assert bool(prog.tables.tile) == (row.order is not None)
    if row.whole:
        assert prog.data.flags & N.DF_WHOLE
        prog.data.d_rowmap.zero_()  # the destinations can only come from the plan's affine form
    if W.declined(row):
        assert prog.tables.rows and not prog.data.flags & N.DF_WHOLE
    prog.launch()
    prog.results()
    assert _kernel() == row.kernel
    assert c.exact()
    if row.crc:
        _corruption(c, prog)
        prog.launch()
        prog.results()
        assert _kernel() == row.kernel
        assert c.exact()
    if row.rowmap and row.shard is None:
        win = _window(row)
        p2, o2 = c.arr.prepare_read(win, out=c.view[win])
        assert not p2.data.flags & N.DF_WHOLE and p2.data.p_rowmap is not None
        _sentinel_over(backings.out, row)
        p2.launch()
        p2.results()
        assert _kernel() == row.kernel
        assert c.exact(c.view[win], c.want[win])
        _sentinel_over(backings.out, row, win)
    else:
        _sentinel_over(backings.out, row)
    assert _all_sentinel(backings.out)
    assert _all_sentinel(backings.arena[: W.FRONT]) and _all_sentinel(backings.arena[W.FRONT + W.BODY:])


def test_fused_launch_low_and_high_half(device, backings):
    """Two k_decode_il programs in ONE launch (k_decode_il_multi through
    ReadGraph), wide_cases.FUSED_ROWS: the il row's 18 chunks twice, from one
    arena (the second array's blobs lie above 2**32), into disjoint outs --
    the low one wholly below 2**31, the high one based 2**31 into the body
    with its slab 16 straddling 2**32 and slab 17 above."""
    import zarr_hip

    _fill(backings)
    store = _store(device, backings)
    progs, cases = [], []
    for row in W.FUSED_ROWS:
        don = _donor(row)
        _ReadCase.put(store, row, don, W.read_placements(row), row.id + "/")
        out = _view(backings.out, row)
        arr = zarr_hip.Array.create(store, W.array_shape(row), W.array_chunks(row), row.dtype, row.fill,
                                    codecs=W.codecs(row), path=row.id)
        fill = np.full_like(don.cells[0], row.fill)
        want = np.concatenate([fill if c == W.dropped(row) else don.cells[c % DISTINCT] for c in range(row.n)])
        cases.append((row, arr, out, want))
    for row, arr, out, want in cases:  # planned once every blob is placed
        prog, o = arr.prepare_read((Ellipsis,), out=out)
        assert o is out and prog.index is None and prog.data.p_rowmap is not None
        progs.append(prog)
    graph = zarr_hip.ReadGraph(progs, 2, device)
    assert graph.launches == 1 and _kernel() == "k_decode_il"
    graph.replay()
    graph.results()
    for row, arr, out, want in cases:
        assert _host_bytes(out) == want.tobytes()
        _sentinel_over(backings.out, row)
    assert _all_sentinel(backings.out)


def _store_bytes(store) -> dict:
    """{key: bytes} of a device store, value by value (never the whole arena)."""
    return {k: store.get_sync(k).to_bytes() for k in store.keys()}


@pytest.mark.parametrize("row", W.WRITE_ROWS, ids=[r.id for r in W.WRITE_ROWS])
def test_write_row(device, backings, row):
    """A whole write from the wide view: only the chunks' windows of the value
    backing are initialised, the last cell (above 2**32 in a slab) holds only
    fill and is elided; the regions reserved for the keys lie below, across and
    above 2**32; the row's encode kernel ran, the store equals the oracle's key
    by key at exactly those placements and reads back through the oracle; the
    value backing is untouched.  Then a partial write merges into the interior
    of cell n - 2, whose blob lies above 2**32."""
    import torch

    _fill(backings)
    don = _donor(row)
    last = W.dropped(row)
    cells = [np.full_like(don.cells[0], row.fill) if c == last else don.cells[c % DISTINCT] for c in range(row.n)]
    data = np.concatenate(cells, axis=_grid_axis(row))
    view = _view(backings.out, row)
    view.copy_(torch.from_numpy(data).to(device))
    store = _store(device, backings)
    _pad_to(store, W.write_top(row))
    arr = _array(store, row)
    arr.set((Ellipsis,), view)
    assert _kernel() == row.kernel
    got = _store_bytes(store)
    assert sorted(got) == sorted(W.key(row, c) for c in range(row.n) if c != last)
    regions = W.write_regions(row)
    for c in range(row.n):
        if c != last:
            assert got[W.key(row, c)] == _blob(don, c), f"bytes differ for cell {c}"
            assert store.placement(W.key(row, c)) == (regions[c], W.blob_len(row))
    back = O.read({W.key(don.row, j): got[W.key(row, j)] for j in range(DISTINCT)}, don.meta)
    assert back.tobytes() == np.concatenate(don.cells, axis=_grid_axis(row)).tobytes()
    assert _host_bytes(view) == data.tobytes()  # the value is as it was
    # ---- the merge path: the interior of cell n - 2 (its blob above 2**32), from the same view
    target = row.n - 2
    assert regions[target] > W.B32
    one = row._replace(n=1)
    sel1 = tuple(slice(1, s - 1) if s > 2 else slice(0, s) for s in W.array_shape(one))
    ax = _grid_axis(row)
    lo = target * W.array_shape(one)[ax]
    sel = tuple(slice(lo + s.start, lo + s.stop) if d == ax else s for d, s in enumerate(sel1))
    new = _data(tuple(s.stop - s.start for s in sel), row.dtype, 9)
    view[sel] = torch.from_numpy(new).to(device)
    meta1 = O.ArrayMeta(W.array_shape(one), W.array_chunks(one), np.dtype(row.dtype), row.fill, codecs=W.codecs(one))
    host1 = {W.key(one, 0): _blob(don, target)}
    O.write(host1, meta1, sel1, new)
    arr.set(sel, view[sel])
    after = _store_bytes(store)
    assert sorted(after) == sorted(got)
    for k in got:
        assert after[k] == (host1[W.key(one, 0)] if k == W.key(row, target) else got[k]), k
    assert store.placement(W.key(row, target))[0] > W.B32
    _sentinel_over(backings.out, row)
    assert _all_sentinel(backings.out)
    assert _all_sentinel(backings.arena[: W.FRONT]) and _all_sentinel(backings.arena[W.FRONT + W.BODY:])


# ---------------------------------------------------------------- value map
@pytest.mark.parametrize("dn", ["f32-i16-enc", "i8-i64-enc"])
def test_value_map_beyond_4gib(dn, device, backings):
    """k_value_map at the ABI over the two bodies (a: the arena backing, b: the
    out backing), three items in one launch: bases at 2**32; an outer dimension
    of count 3 with sa = sb = 2**31 + 4096 (row 2 past 2**32 by the product
    alone) -- both on the kernel's per-element path (rows of 1001 elements);
    eight vector-path rows, four on either side of 2**32 (test_wide_offsets
    proves which path each item takes).  Expected:
    value_cases.ref_run over the rows, re-based into small windows."""
    import torch

    from zarr_hip import _native as N
    from zarr_hip import values as V

    desc = D.SHAPE_DESCS[dn]
    a_dt, b_dt = D.sides(desc)
    items = W.value_items(a_dt.itemsize, b_dt.itemsize)
    rows = W.value_rows(items)
    rng = np.random.default_rng(41)
    n_el = sum(r.count for r in rows)
    if a_dt.kind == "f":
        a = (rng.integers(-1200, 1200, n_el) / 10.0).astype(a_dt)
    else:
        lo, hi = VC._range(a_dt)
        a = rng.integers(max(lo, -100), min(hi, 100) + 1, n_el).astype(a_dt)
    a[::3] = a_dt.type(desc["fill"])
    # the reference, on compact buffers: the rows one after another
    ref_items, pa, pb = [], 0, 0
    for r in rows:
        ref_items.append((pa, pb, [(r.count, a_dt.itemsize, b_dt.itemsize)], 0, 0))
        pa, pb = pa + r.count * a_dt.itemsize, pb + r.count * b_dt.itemsize
    want = bytearray([W.SENTINEL]) * pb
    err, ne_rows = VC.ref_run(desc, ref_items, a.tobytes(), want)
    ne = [int(any(ne_rows[k] for k, r in enumerate(rows) if r.item == i)) for i in range(len(items))]
    # the device
    _fill(backings)
    da = backings.arena[W.FRONT: W.FRONT + W.BODY]
    db = backings.out[W.FRONT: W.FRONT + W.BODY]
    V._check_items(items, W.BODY, W.BODY, a_dt.itemsize, b_dt.itemsize)  # nothing unchecked reaches the device
    pos = 0
    ab = a.view(np.uint8)
    for r in rows:
        n = r.count * a_dt.itemsize
        da[r.a: r.a + n] = torch.from_numpy(ab[pos: pos + n].copy()).to(device)
        pos += n
    its, prefix = V.make_items(items)
    d_items = torch.from_numpy(its.view(np.uint8).reshape(-1)).to(device)
    d_prefix = torch.from_numpy(prefix.view(np.int32)).to(device)
    words = torch.zeros(1 + len(items), dtype=torch.int32, device=device)
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    V.launch(D.op_of(desc), d_items, len(items), d_prefix, int(prefix[-1]), None, da.data_ptr(), W.BODY,
             db.data_ptr(), W.BODY, words, words[1:], stream)
    assert N.lib().zhip_last_kernel() == b"k_value_map"
    torch.cuda.synchronize(device)
    host = words.cpu().numpy()
    assert int(host[0]) == err and [int(x) for x in host[1:]] == ne
    pos = 0
    for r in rows:
        n = r.count * b_dt.itemsize
        assert db[r.b: r.b + n].cpu().numpy().tobytes() == bytes(want[pos: pos + n]), r
        db[r.b: r.b + n] = W.SENTINEL
        pos += n
    assert _all_sentinel(backings.out)


# --------------------------------------------------------- tuning arms 64 / 65
@pytest.mark.tuning
@pytest.mark.parametrize("arm", [64, 65])
@pytest.mark.parametrize("rid", ["near_il", "il"])
def test_buffer_store_arms_are_exact(device, backings, rid, arm):
    """Arms 64 / 65 (k_decode_il storing through a buffer resource of
    0x7FFFFFF0 records at the 32-bit offset rel + lane_off): the near-limit
    row's whole read, where rel + lane_off passes the resource's range and the
    launch must keep the production stores, and the 18-chunk slab row, where
    every store fits, are exact under either arm."""
    from zarr_hip import _native as N

    set_tuning(6, arm)  # first: in the shipped library's process nothing is built before the skip
    try:
        row = W.READ[rid]
        _fill(backings)
        c = _ReadCase(device, backings, row)
        prog, out = c.arr.prepare_read((Ellipsis,), out=c.view)
        assert prog.data.flags & N.DF_WHOLE
        prog.launch()
        prog.results()
        assert _kernel() == "k_decode_il"
    finally:
        set_tuning(6, 0)
    assert c.exact()
    _sentinel_over(backings.out, row)
    assert _all_sentinel(backings.out)
