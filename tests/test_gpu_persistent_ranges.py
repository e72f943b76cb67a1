"""The persistent kernels -- k_decode, k_decode_rows, k_decode_tile, k_encode:
the fallback of every geometry no specialised kernel takes -- with SEVERAL
units per workgroup.  Every other test of them launches at most a few hundred
units, fewer than the resident grid, so each workgroup's range [q0, q1) holds
one unit and the loop that carries a CRC chain over the units of a run,
publishes once per run, retires the previous run's arrival and crosses chunk
boundaries inside a range runs once.

Rows and grid caps come from tests/persist_cases.py; tests/test_persist_ranges.py
shows on the CPU that each (row, cap) here has runs of several units, ranges
of several runs, chunks split between workgroups and the dropped chunk inside
a range.  The capped tests are marked `tuning` (the cap is
zhip_set_tuning(ZHIP_TUNE_MAX_GRID, G): tests/test_gpu_tuning_build.py runs
them on the tuning build).  Two more rows run on the shipped library with no
knob: their launches have more than twice the units that can be resident,
which zhip_last_grid() confirms after the launch.  Last, the shard index of
more than one unit: the only use of k_decode's no-write instantiation.

Everything is byte-exact against the CPU oracle; corruption sites are
enumerated from the chunk's first byte, not from a model of which workgroup
owns them."""

import struct

import numpy as np
import pytest

import dtype_cases as DC
import persist_cases as PC
import tile_cases as TC
from conftest import set_tuning
from oracle import oracle as O
from test_gpu_decode import BE, CRC, LE, SHARD, T, _corrupt, _data
from test_gpu_kernel_matrix import _flip, _kernel, _read, _stores_equal

pytestmark = pytest.mark.gpu

STEP = 4096
KEY_GRID, KEY_ABLATION = 1, 2  # ZHIP_TUNE_MAX_GRID, ZHIP_TUNE_ABLATION


def _grid():
    from zarr_hip import _native as N

    return int(N.lib().zhip_last_grid())


class _capped:
    """The grid cap G (and the row's ablation bits) while the block runs."""

    def __init__(self, G, tune=0):
        self.G, self.tune = G, tune

    def __enter__(self):
        set_tuning(KEY_GRID, self.G)  # skips in the shipped library's process
        if self.tune:
            set_tuning(KEY_ABLATION, self.tune)

    def __exit__(self, *exc):
        set_tuning(KEY_ABLATION, 0)
        set_tuning(KEY_GRID, 0)


def _codecs(row):
    chain = ([T(row.order)] if row.order is not None else []) + [row.endian] + ([CRC] if row.crc else [])
    return [SHARD(row.chunk, chain)] if row.shard is not None else chain


def _box(ix, chunk):
    return tuple(slice(i * k, (i + 1) * k) for i, k in zip(ix, chunk))


_ORACLE = {}


def _oracle(row):
    """(meta, store, keys, whole read) of a row, written by the oracle once:
    the table entry PC.DROPPED is missing -- its key deleted, or for the
    sharded row its inner chunk all fill, which the oracle elides."""
    hit = _ORACLE.get(row.id)
    if hit is not None:
        return hit
    shape = PC.array_shape(row)
    outer = row.shard if row.shard is not None else row.chunk
    meta = O.ArrayMeta(shape, outer, np.dtype(row.dtype), row.fill, codecs=_codecs(row))
    # (complex64: dtype_cases' random bytes, every component different)
    data = DC.sample(shape, row.dtype) if np.dtype(row.dtype).kind == "c" else _data(shape, row.dtype)
    if row.shard is not None:  # entries: shards in C order, their inner chunks in C order
        cps = tuple(s // c for s, c in zip(row.shard, row.chunk))
        data[_box(np.unravel_index(PC.DROPPED, cps), row.chunk)] = row.fill
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    keys = ["c/" + "/".join(str(i) for i in ix) for ix in np.ndindex(*row.grid)]
    assert sorted(keys) == sorted(host)
    if row.shard is None:
        del host[keys[PC.DROPPED]]
    _ORACLE[row.id] = (meta, host, keys, O.read(host, meta).tobytes())
    return _ORACLE[row.id]


class _Case:
    """A fresh device store and array of one row (the launch reads the grid
    cap, so nothing planned under another cap is reused)."""

    def __init__(self, device, row):
        import zarr_hip

        self.row = row
        self.meta, host, self.keys, self.want = _oracle(row)
        self.host = dict(host)
        self.shape = PC.array_shape(row)
        self.outer = row.shard if row.shard is not None else row.chunk
        self.store = zarr_hip.DeviceStore.from_host(self.host, device)
        self.arr = zarr_hip.Array.create(self.store, self.shape, self.outer, row.dtype, row.fill, codecs=_codecs(row))
        self.nbytes = int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize
        self.n_units = PC.n_chunks(row) * PC.units_per_chunk(row)

    def entries(self, prog):
        """Per table entry of a whole read: (key, offset of its payload in the
        key's blob, arena offset of the payload); None for the dropped one."""
        t = prog.tables
        item_of = np.asarray(t.item_of_chunk)
        assert len(item_of) == PC.n_chunks(self.row)
        out = []
        for j in range(len(item_of)):
            key = self.keys[item_of[j]]
            if self.row.shard is None:
                assert item_of[j] == j  # the model's chunk c is table entry c
                out.append(None if j == PC.DROPPED else (key, 0, self.store.placement(key)[0]))
                continue
            blob = self.host[key]
            n = len(item_of) // len(self.keys)
            assert item_of[j] == j // n
            at = len(blob) - (16 * n + 4) + 16 * int(t.chunks["slot"][j])
            off, ln = struct.unpack("<QQ", blob[at: at + 16])
            if j == PC.DROPPED:
                assert (off, ln) == (2 ** 64 - 1, 2 ** 64 - 1)
                out.append(None)
            else:
                assert ln == self.nbytes + 4
                out.append((key, off, self.store.placement(key)[0] + off))
        return out


def _out_bytes(out):
    return np.ascontiguousarray(out.cpu().numpy()).tobytes()


def _cut(shape):
    """A window that cuts every dim it can, the innermost included."""
    win = []
    for n in shape:
        lo = 1 if n > 2 else 0
        win.append(slice(lo, n - 1 if n - 1 > lo else n))
    return tuple(win)


READS = [(r, G) for r in PC.ROWS for G in PC.row_caps(r)]


@pytest.mark.tuning
@pytest.mark.parametrize("row,G", READS, ids=[f"{r.id}-G{G}" for r, G in READS])
def test_capped_read(device, row, G):
    """Under G workgroups: a whole read takes the row's kernel with exactly G
    workgroups and is bit-exact, the dropped chunk filled by the same launch
    and reported ST_MISSING, every other chunk ST_OK; launched twice more it
    stays exact (arrival and ticket words back at zero); a window cutting
    every dim, the first chunk alone and the last chunk alone are exact."""
    from zarr_hip import _native as N

    with _capped(G, row.tune):
        c = _Case(device, row)
        prog, out = c.arr.prepare_read((Ellipsis,))
        assert (bool(prog.tables.fast), bool(prog.tables.rows), bool(prog.tables.tile)) == \
            (row.fast, row.rows, row.decode == PC.K_TILE)
        if row.shard is not None:
            assert prog.index is None and prog.data.n_idx == len(c.keys)  # the indexes: workgroups g, g + G, ...
        ents = c.entries(prog)
        for rep in range(3):
            prog.launch()
            prog.results()
            assert _kernel() == row.decode
            assert _grid() == G
            assert _out_bytes(out) == c.want, rep
            codes = prog.data.statuses()["code"]
            assert [j for j in range(len(ents)) if codes[j] == N.ST_MISSING] == [PC.DROPPED]
            assert {int(k) for k in codes} == {N.ST_OK, N.ST_MISSING}
            if row.shard is not None:
                assert (prog.data.index_statuses()["code"] == N.ST_OK).all()
        for sel in (_cut(c.shape), _box((0,) * len(c.shape), c.outer),
                    _box(tuple(g - 1 for g in row.grid), c.outer)):
            _, got = _read(c.arr, sel)
            assert got == np.ascontiguousarray(O.read(c.host, c.meta, sel)).tobytes(), sel


def _sites(row, nbytes):
    """One byte offset per 4 KiB step of a chunk (from its first byte; lanes and
    words vary with the step), or per tile of a tile row (the restatement's
    enumeration), and the bit to flip there."""
    if row.decode == PC.K_TILE:
        t = TC.Row(row.id, row.chunk, row.order, row.dtype, row.endian, True, row.grid, None, None)
        shape, it, ost = TC.stored_geometry(t)
        tiles = TC.tiles(shape, it, ost)
        sq = TC.c_strides(shape, it)[TC.find_tq(shape, it, ost)]
        sites = [tl.s_off + ((7 * j) % tl.rows) * sq + (13 * j) % tl.cols for j, tl in enumerate(tiles)]
    else:
        sites = [STEP * st + (16 * ((7 * st) % 256) + st % 16) % min(STEP, nbytes - STEP * st)
                 for st in range(-(-nbytes // STEP))]
    assert all(0 <= s < nbytes for s in sites) and len(set(sites)) == len(sites)
    return sites, [1 << (j % 8) for j in range(len(sites))]


SWEEPS = [(r, G) for r in PC.ROWS if r.crc for G in PC.sweep_caps(r)]


@pytest.mark.tuning
@pytest.mark.parametrize("row,G", SWEEPS, ids=[f"{r.id}-G{G}" for r, G in SWEEPS])
def test_capped_every_step_reaches_the_verdict(device, row, G):
    """One flipped bit in EVERY 4 KiB step (every tile) of a chunk, and in its
    trailer, is reported under G workgroups: per round, present chunk i gets
    site round * n + i.  Each launch sets ST_CRC_MISMATCH in the error word
    and in exactly the hit chunks' statuses, every other present chunk is
    ST_OK, the dropped one ST_MISSING.  The restored bytes then read exactly
    twice (no stale ticket or arrival word), and one corrupted chunk raises
    the oracle's message."""
    from zarr_hip import _native as N

    with _capped(G, row.tune):
        c = _Case(device, row)
        prog, out = c.arr.prepare_read((Ellipsis,))
        prog.launch()
        prog.results()
        assert _kernel() == row.decode and _grid() == G
        assert _out_bytes(out) == c.want
        d = prog.data
        ents = c.entries(prog)
        present = [j for j, e in enumerate(ents) if e is not None]
        missing = np.array([e is None for e in ents])
        base = [ents[j][2] for j in present]
        sites, bits = _sites(row, c.nbytes)
        n = len(present)
        rounds = []
        for rnd in range(-(-len(sites) // n)):
            hit = [(i, rnd * n + i) for i in range(n) if rnd * n + i < len(sites)]
            rounds.append(([present[i] for i, _ in hit], [base[i] + sites[s] for i, s in hit],
                           [bits[s] for _, s in hit]))
        assert sum(len(r[0]) for r in rounds) == len(sites)  # every site once
        rounds.append((present, [b + c.nbytes + i % 4 for i, b in enumerate(base)], [0x20] * n))  # the trailers
        for hit_ents, offs, bt in rounds:
            _flip(c.store, offs, bt)
            d.reset_errflag()
            prog.launch()
            err = d.errflag()
            codes = d.statuses()["code"]
            _flip(c.store, offs, bt)  # restored
            assert err & (1 << N.ST_CRC_MISMATCH)
            assert sorted(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == sorted(hit_ents)
            assert (codes[missing] == N.ST_MISSING).all()
            assert ((codes == N.ST_OK) | (codes == N.ST_CRC_MISMATCH) | missing).all()
        d.reset_errflag()
        for _ in range(2):
            prog.launch()
            prog.results()
            assert _out_bytes(out) == c.want
        # the oracle's message, from a site in the middle of the last present chunk
        host = dict(c.host)
        key, in_blob, _ = ents[present[-1]]
        at = in_blob + sites[len(sites) // 2]
        _corrupt(c.store, host, key, at=at)
        with pytest.raises(ValueError) as want:
            O.read(host, c.meta)
        prog.launch()
        with pytest.raises(ValueError) as got:
            prog.results()
        assert str(got.value) == str(want.value)
        _corrupt(c.store, host, key, at=at)
        assert host == c.host
        d.reset_errflag()
        prog.launch()
        prog.results()
        assert _out_bytes(out) == c.want


ENC_ROWS = [r for r in PC.ROWS if r.encode is not None]
# (write_empty_chunks: one short-chunk and one long-chunk row, under the cap that splits every chunk)
WRITES = [(r, G, False) for r in ENC_ROWS for G in PC.write_caps(r)] + \
    [(PC.BY_ID[i], PC.WRITE_CHUNKS + 1, True) for i in ("generic-u16le", "fast-f32-34")]


@pytest.mark.tuning
@pytest.mark.parametrize("row,G,keep", WRITES, ids=[f"{r.id}-G{G}" + ("-keep" if k else "") for r, G, k in WRITES])
def test_capped_write(device, row, G, keep):
    """test_gpu_kernel_matrix.test_encode_row under G workgroups: five chunks
    along the last dim -- one all fill (elided, or kept under
    write_empty_chunks), one fill except its FIRST element, one fill except its
    LAST (the non-empty flag ORed from a run that holds only that end of the
    chunk), two of data -- written whole, then a partial write that merges into
    every chunk, then a write into ONE interior chunk: after each k_encode ran
    last and the store equals the oracle's key by key (trailers from whichever
    run arrived last; the neighbours byte-identical after the interior write);
    the array then reads back exactly."""
    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    with _capped(G):  # (skips before any data is made)
        pass
    dt = np.dtype(row.dtype)
    fill = 0
    cs = row.chunk
    cl = cs[-1]
    shape = cs[:-1] + (PC.WRITE_CHUNKS * cl,)
    codecs = _codecs(row)
    meta = O.ArrayMeta(shape, cs, dt, fill, codecs=codecs, write_empty_chunks=keep)
    data = _data(shape, row.dtype, 7)
    data[..., 0: 3 * cl] = fill
    one = -0.0 if dt.kind == "f" else 1          # -0.0: bitwise != fill, the chunk is kept
    data[(0,) * (len(cs) - 1) + (cl,)] = one                           # chunk 1: its first element
    data[tuple(s - 1 for s in cs[:-1]) + (3 * cl - 1,)] = one          # chunk 2: its last element
    n_units = PC.WRITE_CHUNKS * PC.units_per_chunk(row)
    with _capped(G, row.tune):
        store = zarr_hip.DeviceStore(device)
        arr = zarr_hip.Array.create(store, shape, cs, row.dtype, fill, codecs=codecs,
                                    config=ArrayConfig(write_empty_chunks=keep))
        host = {}

        def write(sel, val):
            O.write(host, meta, sel, val)
            arr[sel] = val
            assert _kernel() == row.encode
            return _stores_equal(store, host)

        got = write((Ellipsis,), data)
        assert _grid() == min(G, n_units)
        lead = "c/" + "0/" * (len(cs) - 1)
        assert sorted(got) == [lead + str(i) for i in ((0, 1, 2, 3, 4) if keep else (1, 2, 3, 4))]
        part = tuple(slice(1, s - 2) for s in shape[:-1]) + (slice(3, shape[-1] - 5),)
        before = write(part, _data(tuple(s.stop - s.start for s in part), row.dtype, 8))
        assert len(before) == PC.WRITE_CHUNKS
        inner = tuple(slice(2, s - 1) for s in cs[:-1]) + (slice(3 * cl + 1, 4 * cl - 3),)
        after = write(inner, _data(tuple(s.stop - s.start for s in inner), row.dtype, 9))
        assert _grid() == min(G, n_units // PC.WRITE_CHUNKS)
        for k in before:
            assert (after[k] == before[k]) == (k != lead + "3"), k
        assert arr[...].tobytes() == O.read(host, meta).tobytes()
        assert _kernel() == row.decode


# ------------------------------------------------ the shipped library, no knob
def _resident_bound(device):
    """What csrc/capi.cpp starts the persistent grid from: 8 workgroups per CU
    (the kernel's occupancy can only lower it)."""
    import torch

    return torch.cuda.get_device_properties(device).multi_processor_count * 8


def _whole_read(arr, kernel, n_units):
    prog, out = arr.prepare_read((Ellipsis,))
    prog.launch()
    assert _kernel() == kernel
    grid = _grid()
    assert 1 <= grid and 2 * grid <= n_units, (grid, n_units)  # every workgroup took at least two units
    return prog, out


def test_resident_grid_over_one_unit_chunks(device):
    """Row (a): more than twice as many 30-byte chunks (int16, big-endian,
    checksummed; one unit each) as workgroups can be resident, so every range
    holds several CHUNKS: each unit is a run of its own, with the previous
    run's arrival retired one run later.  One chunk in 97 is missing.  Exact,
    ST_MISSING exactly where a chunk is missing, and one corrupted chunk in the
    middle raises the oracle's message; restored, it reads exactly again."""
    import zarr_hip
    from zarr_hip import _native as N

    n = 2 * _resident_bound(device) + 3
    grid = (-(-n // 64), 64)
    n = grid[0] * grid[1]
    chunk, codecs, fill = (3, 5), [BE, CRC], 7
    shape = tuple(c * g for c, g in zip(chunk, grid))
    meta = O.ArrayMeta(shape, chunk, np.dtype("int16"), fill, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "int16", 3))
    keys = ["c/%d/%d" % ix for ix in np.ndindex(*grid)]
    gone = list(range(5, n, 97))
    for i in gone:
        del host[keys[i]]
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunk, "int16", fill, codecs=codecs)
    want = O.read(host, meta).tobytes()
    prog, out = _whole_read(arr, "k_decode", n)
    prog.results()
    assert _out_bytes(out) == want
    item_of = np.asarray(prog.tables.item_of_chunk)
    codes = prog.data.statuses()["code"]
    assert sorted(item_of[codes == N.ST_MISSING]) == gone and set(codes) == {N.ST_OK, N.ST_MISSING}
    bad = dict(host)
    key = keys[n // 2 + 1]
    assert key in host
    _corrupt(store, bad, key, at=17)
    with pytest.raises(ValueError) as exp:
        O.read(bad, meta)
    prog.launch()
    with pytest.raises(ValueError) as got:
        prog.results()
    assert str(got.value) == str(exp.value)
    codes = prog.data.statuses()["code"]
    assert list(item_of[codes == N.ST_CRC_MISMATCH]) == [keys.index(key)]
    _corrupt(store, bad, key, at=17)
    assert bad == host
    prog.data.reset_errflag()
    for _ in range(2):
        prog.launch()
        prog.results()
        assert _out_bytes(out) == want


def test_resident_grid_over_two_unit_chunks(device):
    """Row (b): chunks of 32 800 bytes ((2, 4100) float32: whole 16 400-byte
    rows, no row layout) are two units, the first holding the chunk's first 32
    bytes; with more than twice the resident grid of units every range holds
    whole chunks (runs of two units: one chain, one shift, one publication) and
    chunks cut between two workgroups.  Whole read exact; a bit in the first
    unit of one chunk and in the second unit of another fails exactly those two
    chunks, each with the oracle's message; a whole write (k_encode, the same
    partition) equals the oracle's store."""
    import zarr_hip
    from zarr_hip import _native as N

    nc = _resident_bound(device) + 2  # 2 * nc units >= 2 * bound + 3
    chunk, codecs = (2, 4100), [LE, CRC]
    shape = (2 * nc, 4100)
    meta = O.ArrayMeta(shape, chunk, np.dtype("float32"), 0.0, codecs=codecs)
    data = _data(shape, "float32", 5)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    assert PC.nseg_of(2 * 4100 * 4) == 2
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunk, "float32", 0.0, codecs=codecs)
    prog, out = _whole_read(arr, "k_decode", 2 * nc)
    assert prog.tables.fast and not prog.tables.rows
    prog.results()
    want = O.read(host, meta).tobytes()
    assert _out_bytes(out) == want
    item_of = np.asarray(prog.tables.item_of_chunk)
    hits = [(nc // 3, 5), (2 * nc // 3 + 1, 20000)]  # (chunk, byte): its first unit is bytes [0, 32)
    bad = dict(host)
    for i, at in hits:
        _corrupt(store, bad, "c/%d/0" % i, at=at)
    prog.launch()
    with pytest.raises(ValueError):
        prog.results()
    codes = prog.data.statuses()["code"]
    assert sorted(item_of[codes == N.ST_CRC_MISMATCH]) == [i for i, _ in hits]
    assert set(codes) == {N.ST_OK, N.ST_CRC_MISMATCH}
    for i, at in hits:
        _corrupt(store, bad, "c/%d/0" % i, at=at)
    assert bad == host
    for i, at in hits:  # one at a time: the oracle's message
        _corrupt(store, bad, "c/%d/0" % i, at=at)
        with pytest.raises(ValueError) as exp:
            O.read(bad, meta)
        prog.data.reset_errflag()
        prog.launch()
        with pytest.raises(ValueError) as got:
            prog.results()
        assert str(got.value) == str(exp.value)
        _corrupt(store, bad, "c/%d/0" % i, at=at)
    prog.data.reset_errflag()
    prog.launch()
    prog.results()
    assert _out_bytes(out) == want
    del prog, out, arr, store
    wstore = zarr_hip.DeviceStore(device)
    warr = zarr_hip.Array.create(wstore, shape, chunk, "float32", 0.0, codecs=codecs)
    warr[...] = data
    assert _kernel() == "k_encode"
    assert 2 * _grid() <= 2 * nc
    _stores_equal(wstore, host)


# ------------------------------------------------ the index longer than one unit
IDX_SHAPE, IDX_SHARD, IDX_INNER = (46, 92), (46, 46), (1, 1)
IDX_N = 46 * 46
# kind: (host store?, inner chain, the index checked by its own no-write launch?)
IDX_KINDS = {"device_fused": (False, [LE, CRC], False), "device_own": (False, [LE], True),
             "memory_own": (True, [LE, CRC], True)}
IDX_CASES = [pytest.param(k, 0, id=k) for k in IDX_KINDS] + \
    [pytest.param(k, G, id=f"{k}-G{G}", marks=pytest.mark.tuning) for k in ("device_own", "memory_own") for G in (1, 2)]


@pytest.mark.parametrize("kind,G", IDX_CASES)
def test_index_of_two_units(device, kind, G):
    """uint8 shards of 46 x 46 one-byte inner chunks: 2 116 index entries,
    33 856 index bytes, two units.  With a checksummed inner chain on a device
    store the data launch checks the indexes itself (verify_index, nine
    passes); without one, or from a host store, they are checked by a launch
    of their own: k_decode's no-write instantiation, one range over both units
    of an index (under the caps G = 1 and G = 2 of the tuning build: both
    indexes in one range, and one index per workgroup).  The whole read is
    exact, a flipped bit in the first and in the last 4 KiB of an index raises
    the oracle's message, and a whole write reproduces the oracle's shards."""
    import zarr_hip
    from zarr_hip import _native as N

    on_host, chain, own = IDX_KINDS[kind]
    assert 16 * IDX_N == 33856 and PC.nseg_of(16 * IDX_N) == 2
    codecs = [SHARD(IDX_INNER, chain)]
    meta = O.ArrayMeta(IDX_SHAPE, IDX_SHARD, np.dtype("uint8"), 0, codecs=codecs)
    data = _data(IDX_SHAPE, "uint8", 21)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    want = O.read(host, meta).tobytes()

    def run():
        store = zarr_hip.MemoryStore(dict(host)) if on_host else zarr_hip.DeviceStore.from_host(host, device)
        arr = zarr_hip.Array.create(store, IDX_SHAPE, IDX_SHARD, "uint8", 0, codecs=codecs)
        prog, out = arr.prepare_read((Ellipsis,))
        if own:
            assert prog.index is not None and prog.index.n == 2 and prog.data.n_idx == 0
            assert prog.index.plan.units_per_chunk == 2
        else:
            assert prog.index is None and prog.data.n_idx == 2
        prog.launch()
        prog.results()
        assert _kernel() == "k_decode"
        assert _out_bytes(out) == want
        if own:  # the index launch again, on its own: two indexes of two units
            prog.index.launch()
            assert _kernel() == "k_decode" and _grid() == (G or 4)
            assert (prog.index.statuses()["code"] == N.ST_OK).all()
        del prog, out
        for shard, entry in ((0, 0), (1, IDX_N - 1)):  # the first / the last 4 KiB of an index
            key = "c/0/%d" % shard
            good = host[key]
            b = bytearray(good)
            b[len(b) - (16 * IDX_N + 4) + 16 * entry] ^= 0x01  # the offset's low bit: still inside the shard
            bad = dict(host)
            bad[key] = bytes(b)
            with pytest.raises(ValueError) as exp:
                O.read(bad, meta)
            assert "checksum" in str(exp.value)
            store.set_sync(key, bytes(b))
            with pytest.raises(ValueError) as got:
                arr[...]
            assert str(got.value) == str(exp.value)
            store.set_sync(key, good)
            assert arr[...].tobytes() == want
        wstore = zarr_hip.MemoryStore() if on_host else zarr_hip.DeviceStore(device)
        zarr_hip.Array.create(wstore, IDX_SHAPE, IDX_SHARD, "uint8", 0, codecs=codecs)[...] = data
        _stores_equal(wstore, host)

    if G:
        with _capped(G):
            run()
    else:
        run()
