"""The transposing ("tile") kernels at ranks 2, 4 and 5, pinned by name: which
kernel a row of tests/tile_cases.py takes (its docstring restates the rules),
bit-exact decodes against the oracle with a missing chunk, every tile of a
chunk reaching its CRC verdict (tiles enumerated by the numpy restatement,
not by a model of which workgroup owns which tile), and encodes -- whole,
merged, into one interior chunk, and the prefix boxes of ragged arrays --
byte-identical to the oracle's store.  Every other GPU test of these kernels
uses a 3-D chunk, where the in-kernel chain over the "other" stored dims has
one live iteration; here it has none (rank 2), two (rank 4) and three (rank 5).

Shipped library only: nothing here forces a tuning arm.  The grouped kernels
cannot occur at rank 2 (tile_cases.py says why); every other tile kernel name
is asserted at rank 2 and at rank 4 or 5."""

import numpy as np
import pytest

import tile_cases as TC
from oracle import oracle as O
from test_gpu_decode import CRC, SHARD, T, _corrupt, _data
from test_gpu_kernel_matrix import _flip, _kernel, _read, _stores_equal

pytestmark = pytest.mark.gpu


def _codecs(row):
    chain = ([T(row.order)] if row.order is not None else []) + [row.endian] + ([CRC] if row.crc else [])
    return [SHARD(row.inner, chain)] if row.inner is not None else chain


class _Case:
    """One row's array, written by the oracle with chunk 1 dropped (a missing
    chunk takes the fill through the same launch), uploaded to the device."""

    def __init__(self, device, row):
        import zarr_hip
        from zarr_hip.spec import ArrayConfig

        self.row = row
        self.shape = TC.array_shape(row)
        codecs = _codecs(row)
        self.meta = O.ArrayMeta(self.shape, row.chunk, np.dtype(row.dtype), row.fill, codecs=codecs)
        self.host = {}
        O.write(self.host, self.meta, (Ellipsis,), _data(self.shape, row.dtype))
        # batch items are the chunk grid in C order
        self.keys = ["c/" + "/".join(str(i) for i in ix) for ix in np.ndindex(*row.grid)]
        assert sorted(self.keys) == sorted(self.host)
        self.dropped = 1
        del self.host[self.keys[self.dropped]]
        self.store = zarr_hip.DeviceStore.from_host(self.host, device)
        self.arr = zarr_hip.Array.create(self.store, self.shape, row.chunk, row.dtype, row.fill, codecs=codecs,
                                         config=ArrayConfig(order="F" if row.order is None else "C"))
        self.nbytes = int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize
        self.want = O.read(self.host, self.meta).tobytes()


def _out_bytes(out):
    return np.ascontiguousarray(out.cpu().numpy()).tobytes()


@pytest.mark.parametrize("row", TC.ROWS, ids=[r.id for r in TC.ROWS])
def test_tile_decode_row(device, row):
    """A whole read plans tile mode, takes the row's kernel (by name) and is
    bit-exact with the oracle, the missing chunk (not the first) filled by the
    same launch -- a NaN fill on some float rows; a window that cuts every dim
    and starts inside the first chunk is exact, whichever kernel it takes.
    Sharded rows (transposed inner chunks) name their kernel by its prefix."""
    c = _Case(device, row)
    prog, out = c.arr.prepare_read((Ellipsis,))
    assert prog.tables.tile
    prog.launch()
    prog.results()
    if row.inner is not None:
        assert _kernel().startswith("k_decode_tile")
    else:
        assert _kernel() == row.decode
    assert _out_bytes(out) == c.want
    if row.inner is not None:
        return
    win = []
    for n, k in zip(c.shape, row.chunk):
        lo = 1 if k > 1 else 0
        win.append(slice(lo, n - 1 if n - 1 > lo else n))
    assert any(s.start for s in win)
    _, got = _read(c.arr, tuple(win))
    assert got == np.ascontiguousarray(O.read(c.host, c.meta, tuple(win))).tobytes()


SWEEP_ROWS = [r for r in TC.ROWS if r.sweep]
assert all(r.crc and r.inner is None for r in SWEEP_ROWS)
# at least one sweep row per decode kernel and rank class
assert {(len(r.chunk), r.decode) for r in SWEEP_ROWS} >= {(2, TC.T2W), (4, TC.T2W), (4, TC.TG2W), (5, TC.TG2W),
                                                           (2, TC.TGEN), (4, TC.TGEN)}


def _raw_statuses(d):
    """The status table as the launch left it (no deferred verdicts merged in)."""
    from zarr_hip.pipeline import STATUS_DT

    return d.d_status[: d.n * 4].cpu().numpy().view(STATUS_DT).copy()


@pytest.mark.parametrize("row", SWEEP_ROWS, ids=[r.id for r in SWEEP_ROWS])
def test_every_tile_reaches_the_verdict(device, row):
    """One flipped bit in EVERY tile of a chunk, and in its trailer, is
    reported: per round chunk i of the n present chunks gets tile round * n + i
    of the restatement's enumeration, at stored row (7 j) % rows and byte
    (13 j) % cols of tile j, bit 1 << (j % 8).  Each launch -- without
    ZHIP_DF_DEFER and with the bank pinned to 0, so the grouped kernels report
    in the launch itself as for a C caller -- sets ST_CRC_MISMATCH in the error
    word and in exactly the hit chunks' statuses, ST_MISSING for the dropped
    chunk, ST_OK elsewhere.  The restored bytes then read exactly twice (no
    stale arrival word).  Under the pipeline's own flags (deferred verdicts for
    the grouped kernels) one corrupted chunk raises the reference's message,
    and the restored bytes read exactly twice (no stale bank word)."""
    from zarr_hip import _native as N

    c = _Case(device, row)
    shape, it, ost = TC.stored_geometry(row)
    tiles = TC.tiles(shape, it, ost)
    sq = TC.c_strides(shape, it)[TC.find_tq(shape, it, ost)]
    prog, out = c.arr.prepare_read((Ellipsis,))
    d = prog.data
    d.flags &= ~N.DF_DEFER

    def launch():
        d._bank = 0  # a caller that never sets ZHIP_DF_BANK1
        d.reset_errflag()
        d.d_status.zero_()
        prog.launch()

    launch()
    assert _kernel() == row.decode
    assert not d.errflag() & (1 << N.ST_CRC_MISMATCH)
    assert _out_bytes(out) == c.want
    item_of = np.asarray(prog.tables.item_of_chunk)
    assert d.n == len(c.keys) and sorted(item_of) == list(range(d.n))
    present = [j for j in range(d.n) if item_of[j] != c.dropped]  # table entries of the present chunks
    base = [c.store.placement(c.keys[item_of[j]])[0] for j in present]
    n_tiles, n = len(tiles), len(present)
    missing = np.array([item_of[j] == c.dropped for j in range(d.n)])

    def at(j):  # byte offset in the stored chunk of tile j's flipped byte
        t = tiles[j]
        off = t.s_off + ((7 * j) % t.rows) * sq + (13 * j) % t.cols
        assert off < c.nbytes
        return off

    rounds, covered = [], set()
    for rnd in range(-(-n_tiles // n)):
        hit = [(i, rnd * n + i) for i in range(n) if rnd * n + i < n_tiles]
        covered |= {j for _, j in hit}
        rounds.append(([present[i] for i, _ in hit], [base[i] + at(j) for i, j in hit],
                       [1 << (j % 8) for _, j in hit]))
    assert covered == set(range(n_tiles))  # every tile was hit
    assert len(rounds) <= 50
    rounds.append((present, [b + c.nbytes + i % 4 for i, b in enumerate(base)], [0x20] * n))  # the trailers
    for ents, offs, bits in rounds:
        _flip(c.store, offs, bits)
        launch()
        err = d.errflag()
        codes = _raw_statuses(d)["code"]
        _flip(c.store, offs, bits)  # restored
        assert err & (1 << N.ST_CRC_MISMATCH)
        assert sorted(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == sorted(ents)
        assert (codes[missing] == N.ST_MISSING).all()
        assert ((codes == N.ST_OK) | (codes == N.ST_CRC_MISMATCH) | missing).all()
    for _ in range(2):
        launch()
        assert not d.errflag() & (1 << N.ST_CRC_MISMATCH)
        assert (_raw_statuses(d)["code"][~missing] == N.ST_OK).all()
        assert _out_bytes(out) == c.want
    # the pipeline's own flags: the reference's message, once per row
    prog, out = c.arr.prepare_read((Ellipsis,))
    assert prog.data.flags & N.DF_DEFER
    host = dict(c.host)
    key = c.keys[item_of[present[-1]]]
    where = at(n_tiles - 1)
    _corrupt(c.store, host, key, at=where)
    with pytest.raises(ValueError) as want:
        O.read(host, c.meta)
    prog.launch()
    with pytest.raises(ValueError) as got:
        prog.results()
    assert _kernel() == row.decode
    assert str(got.value) == str(want.value)
    _corrupt(c.store, host, key, at=where)
    assert host == c.host
    prog.data.reset_errflag()
    for _ in range(2):
        prog.launch()
        prog.results()
        assert _out_bytes(out) == c.want


# ---------------------------------------------------------------- encode
ENCODE_ROWS = [r for r in TC.ROWS if r.encode is not None]
# every encode kernel at rank 2 where it exists there, all four at rank 4, one at rank 5
assert {(len(r.chunk), r.encode) for r in ENCODE_ROWS} >= (
    {(2, k) for k in (TC.E2, TC.E4, TC.EGEN)} | {(4, k) for k in (TC.E2, TC.E4, TC.EG, TC.EGEN)})
assert any(len(r.chunk) == 5 for r in ENCODE_ROWS)


@pytest.mark.parametrize("row", ENCODE_ROWS, ids=[r.id for r in ENCODE_ROWS])
def test_tile_encode_row(device, row):
    """Six chunks, three along the first dim by two along the last -- one
    entirely fill (elided: no key), one fill except its FIRST element, one fill
    except its LAST (the non-empty flag from the first or the last tile alone;
    floats: -0.0 against a 0.0 fill), three of data -- written whole, then a
    partial write that merges into every chunk, then a write into ONE interior
    chunk: after each, the row's kernel ran last and the store equals the
    oracle's key by key (after the last, every other key byte-identical to
    before); the array then reads back exactly."""
    import zarr_hip

    dt = np.dtype(row.dtype)
    fill = 0
    cs = row.chunk
    nd = len(cs)
    grid = (3,) + (1,) * (nd - 2) + (2,)
    shape = tuple(k * g for k, g in zip(cs, grid))
    codecs = _codecs(row)
    meta = O.ArrayMeta(shape, cs, dt, fill, codecs=codecs)
    data = _data(shape, row.dtype, 7)
    cells = list(np.ndindex(*grid))

    def box(ix):
        return tuple(slice(i * k, (i + 1) * k) for i, k in zip(ix, cs))

    def key(ix):
        return "c/" + "/".join(str(i) for i in ix)

    one = -0.0 if dt.kind == "f" else 1          # -0.0: bitwise != fill, the chunk is kept
    for ix in cells[:3]:
        data[box(ix)] = fill
    data[tuple(s.start for s in box(cells[1]))] = one         # chunk 1: its first element
    data[tuple(s.stop - 1 for s in box(cells[2]))] = one      # chunk 2: its last element
    store = zarr_hip.DeviceStore(device)
    arr = zarr_hip.Array.create(store, shape, cs, row.dtype, fill, codecs=codecs)
    host = {}

    def write(sel, val):
        O.write(host, meta, sel, val)
        arr[sel] = val
        assert _kernel() == row.encode
        return _stores_equal(store, host)

    got = write((Ellipsis,), data)
    assert sorted(got) == sorted(key(ix) for ix in cells[1:])       # chunk 0 elided
    part = tuple(slice(1, s - 1) if s > 2 else slice(None) for s in shape)
    before = write(part, _data(tuple(len(range(*s.indices(n))) for s, n in zip(part, shape)), row.dtype, 8))
    assert len(before) == len(cells)
    target = cells[4]
    inner = tuple(slice(s.start + 1, s.stop - 1) if k > 2 else s for s, k in zip(box(target), cs))
    after = write(inner, _data(tuple(s.stop - s.start for s in inner), row.dtype, 9))
    for k in before:
        assert (after[k] == before[k]) == (k != key(target)), k
    assert arr[...].tobytes() == O.read(host, meta).tobytes()
    assert _kernel() == row.decode


@pytest.mark.parametrize("rg", TC.RAGGED, ids=[r.id for r in TC.RAGGED])
def test_tile_encode_ragged_edges(device, rg):
    """The prefix-box path (k_encode_tile under ZHIP_DF_TILE_PREFIX): arrays
    ragged along the decoded dims stored as tq, as the innermost stored dim and
    (ranks 4 and 5) as two other stored dims at once, so the corner chunk is a
    prefix box cut in four dims and tiles beyond either other-dim count are
    outside it.  Written whole: the store equals the oracle's key by key (one
    chunk of fill: elided, or kept under write_empty_chunks; a NaN fill on one
    row), k_encode_tile ran, and the array reads back exactly."""
    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    dt = np.dtype(rg.dtype)
    codecs = [T(rg.order), rg.endian, CRC]
    meta = O.ArrayMeta(rg.shape, rg.chunk, dt, rg.fill, codecs=codecs, write_empty_chunks=rg.write_empty)
    data = _data(rg.shape, rg.dtype, 11)
    data[tuple(slice(0, k) for k in rg.chunk)] = rg.fill      # the first chunk: all fill
    data[tuple(slice(n - n % k if n % k else n - k, n) for n, k in zip(rg.shape, rg.chunk))] = rg.fill  # the corner
    data[tuple(n - 1 for n in rg.shape)] = 1                  # ... but its last element
    store = zarr_hip.DeviceStore(device)
    arr = zarr_hip.Array.create(store, rg.shape, rg.chunk, rg.dtype, rg.fill, codecs=codecs,
                                config=ArrayConfig(write_empty_chunks=rg.write_empty))
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    arr[...] = data
    assert _kernel() == "k_encode_tile"
    got = _stores_equal(store, host)
    n_chunks = int(np.prod([-(-n // k) for n, k in zip(rg.shape, rg.chunk)]))
    assert len(got) == (n_chunks if rg.write_empty else n_chunks - 1)
    assert arr[...].tobytes() == O.read(host, meta).tobytes()
