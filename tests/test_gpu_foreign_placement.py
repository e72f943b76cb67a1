"""Every decode family over sources this library did not place, per row and
form of tests/placement_cases.py (tests/test_placement_rules.py proves on the
CPU that the forms cover every address residue, that the oracle reads them,
that three mis-readers would be caught and that every window a kernel may
touch lies inside the allocation).  Shipped library only, everything bit-exact.

The store is built from the restated image: one arena.reserve for the
backing, one copy, the placements set as DeviceStore.from_host sets them.
Keys at an odd base are only ever read (DeviceArena.free takes granules).

Per row and form:
  1. a whole read through read_sync into an out between guard bands: the
     oracle's bytes, the guards intact, the row's kernel by name;
  2. a prepared program: every status ST_OK but ST_MISSING for the dropped
     chunk, the error word zero; sharded row layouts keep their load
     prediction (every predicted address is wrong: the miss path);
  3. one ragged partial selection;
  4. CRC chains: one bit flipped in the first and the last payload byte and in
     each trailer byte of the first chunk at an odd address -- the oracle's
     exception and message, that chunk alone ST_CRC_MISMATCH with the oracle's
     stored / computed values, and the same program clean once restored;
  5. index CRCs: one bit of an index at an odd address.
Then partial writes over foreign shards, the fused launches over stores of
different forms, and host stores."""

import numpy as np
import pytest

import placement_cases as PC
from damage_cases import ST_CRC_MISMATCH, ST_MISSING, ST_OK, TAIL_SLACK
from oracle import oracle as O
from test_gpu_damage_matrix import _Out, _Run, _bits, _entries, _kernel, _lib, _units
from test_gpu_decode import _data
from test_gpu_shard_index import _same

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the store
def _foreign_store(device, p):
    """A DeviceStore over the restated image, its blobs where the restatement says."""
    import torch

    import zarr_hip

    store = zarr_hip.DeviceStore(device, capacity=p.alloc - TAIL_SLACK)
    assert store.arena.buf.numel() == p.alloc and store.arena.buf.data_ptr() % 256 == 0
    assert store.arena.reserve(p.top) == 0 and store.arena.top == p.top
    store.arena.buf[: p.top].copy_(torch.from_numpy(p.image))
    store._index = dict(p.blobs)
    for k, place in p.blobs.items():
        assert store.placement(k) == place
        ref = store.get_sync(k)
        assert (ref.offset, ref.length) == place
    for lo, hi in PC.windows(p):
        assert 0 <= lo and hi <= store.arena.buf.numel()
    return store


def _array(store, row, form):
    import zarr_hip

    meta = PC.meta_of(row, form.loc or "end", True if form.icrc is None else form.icrc)
    arr = zarr_hip.Array.create(store, meta.shape, meta.chunk_shape, PC.dtype_of(row), PC.fill_of(row),
                                codecs=meta.codecs)
    return arr, meta


def _row_units(row):
    if row.kind == "u":
        r = row.src
        return len(PC.keys_of(row)) * _units(int(np.prod(r.chunk)) * np.dtype(r.dtype).itemsize)
    g = row.src
    return len(PC.keys_of(row)) * g["n"] * _units(int(np.prod(g["inner"])) * np.dtype(g["dtype"]).itemsize)


def _flip(store, addr, bit):
    store.arena.buf[addr] ^= bit


def _table(prog, row):
    """(entries, the status codes a healthy launch must leave)."""
    ents = _entries(prog, row.kind == "s")
    drop = (row.drop, 0) if row.kind == "u" else tuple(row.drop)
    assert drop in ents and len(set(ents)) == len(ents)
    return ents, [ST_MISSING if e == drop else ST_OK for e in ents]


def _reset(prog):
    prog.data.reset_errflag()
    if prog.index is not None:
        prog.index.reset_errflag()


def _clean(run, row, want, check_bytes=True):
    """A launch over the healthy store: the whole status table, no error, no verdict word, the oracle's bytes."""
    run.launch()
    for prog, o in zip(run.progs, run.outs):
        assert prog.data.errflag() == 0
        assert not prog.data.d_ws[: prog.data.n * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)[:, 0::2].any()
        _, codes = _table(prog, row)
        assert [int(c) for c in prog.data.statuses()["code"]] == codes
        prog.results()
        if check_bytes:
            assert o.bits().tobytes() == _bits(want).tobytes()
        else:
            o.bits()  # (the guards)


def _oracle_error(p, meta, key, blob, sel):
    host = dict(p.host)
    host[key] = blob
    with pytest.raises(ValueError) as err:
        O.read(host, meta, sel)
    return str(err.value)


def _chunk_region(row, keys, key, slot):
    item = keys.index(key)
    if row.kind == "u":
        from damage_cases import u_region

        return u_region(row.src, item)
    g = row.src
    return PC._slot_region(g, tuple(int(i) for i in np.unravel_index(item, g["grid"])), slot)


def _flipped(blob, at, bit):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


# ------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("row,form", PC.PARAMS, ids=PC.IDS)
def test_foreign_placement(device, row, form):
    from zarr_hip import _native as N

    p = PC.restate(row.id, form.name)
    store = _foreign_store(device, p)
    arr, meta = _array(store, row, form)
    keys, shape, want = PC.keys_of(row), PC.full_shape(row), p.want
    kernel = PC.kernel_of(row, form)
    # 1. read_sync, between guards
    o = _Out(device, shape, PC.dtype_of(row))
    arr.get((Ellipsis,), out=o.view)
    got_kernel = _kernel()
    assert got_kernel.startswith(kernel) if row.prefix else got_kernel == kernel, got_kernel
    assert o.bits().tobytes() == _bits(want).tobytes()
    del o
    # 2. the prepared program (fused rows: the row planned two or three times, one launch)
    run = _Run(device, arr, shape, PC.dtype_of(row), row.fused, got_kernel, _row_units(row))
    for prog in run.progs:  # (the il kernels resolve their own units: the pipeline builds them no prediction)
        il = bool(N.Plan(prog.tables.layout, upload=False).kernel_flags & N.PK_IL)
        assert (prog.tables.predict is not None) == (row.kind == "s" and bool(prog.tables.rows) and not il)
    _clean(run, row, want)
    # 3. a ragged partial selection
    sel = PC.ragged(shape)
    assert _bits(arr[sel]).tobytes() == _bits(want[sel]).tobytes()
    # 4. CRC chains: the first chunk at an odd address (not one two entries name)
    aliased = {(k, s) for k, pair in p.alias.items() for s in pair}
    odd = [ks for ks, (a, _) in p.chunks.items() if a % 4 and ks not in aliased]
    if p.crc and odd:
        key, slot = odd[0]
        a, n = p.chunks[(key, slot)]
        base = p.blobs[key][0]
        region = _chunk_region(row, keys, key, slot)
        entry = (keys.index(key), slot)
        for at, bit in [(a, 0x01), (a + n - 5, 0x80)] + [(a + n - 4 + i, 0x10 << (i % 4)) for i in range(4)]:
            blob = _flipped(p.host[key], at - base, bit)
            raw = blob[a - base: a - base + n]
            stored, computed = int(np.frombuffer(raw[-4:], "<u4")[0]), O.crc32c(raw[:-4])
            assert stored != computed
            msg = _oracle_error(p, meta, key, blob, region)
            _flip(store, at, bit)
            try:
                run.launch()
                for prog in run.progs:
                    with pytest.raises(ValueError) as err:
                        prog.results()
                    assert str(err.value) == msg
                    _reset(prog)
                run.launch()
                for prog in run.progs:
                    ents, codes = _table(prog, row)
                    st = prog.data.statuses()
                    j = ents.index(entry)
                    codes[j] = ST_CRC_MISMATCH
                    assert [int(c) for c in st["code"]] == codes, (at - a, n)
                    assert (int(st[j]["stored"]), int(st[j]["computed"])) == (stored, computed)
                    assert prog.data.errflag() & ~(1 << ST_CRC_MISMATCH) == 0
                    _reset(prog)
            finally:
                _flip(store, at, bit)
        _clean(run, row, want, check_bytes=False)
    # 5. the index CRC, an index at an odd address: the length's low bit of a present entry
    odd_index = [k for k, (a, _) in p.index.items() if a % 4]
    if row.kind == "s" and form.icrc and odd_index:
        key = odd_index[0]
        slot = next(s for (k, s) in p.chunks if k == key)
        at = p.index[key][0] + 16 * slot + 8
        blob = _flipped(p.host[key], at - p.blobs[key][0], 0x01)
        msg = _oracle_error(p, meta, key, blob, _chunk_region(row, keys, key, slot))
        assert "checksum" in msg
        _flip(store, at, 0x01)
        try:
            run.launch()
            for prog in run.progs:
                with pytest.raises(ValueError) as err:
                    prog.results()
                assert str(err.value) == msg
                _reset(prog)
        finally:
            _flip(store, at, 0x01)
    _clean(run, row, want)


# ------------------------------------------------------------------ writes over foreign shards
def _write_sel(g):
    """An interior selection: along the first dimension the first inner chunk cut, the second whole, a third
    cut where there is one; the first inner chunk alone along every other; all other inner chunks untouched."""
    i0, c0 = g["inner"][0], g["shape"][0] // g["inner"][0]
    assert c0 >= 2
    first = slice(i0 // 2, 2 * i0 + i0 // 2 if c0 >= 3 else 2 * i0)
    return (first,) + tuple(slice(0, i) for i in g["inner"][1:])


W_ROWS = [r for r in PC.ROWS if r.kind == "s"]
W_PARAMS = [(r, f) for r in W_ROWS for f in PC.forms(r) if f.name in ("stagger-end-icrc", "alias-end-icrc")]


@pytest.mark.parametrize("row,form", W_PARAMS, ids=[f"{r.id}-{f.name}" for r, f in W_PARAMS])
def test_partial_write_over_a_foreign_shard(device, row, form):
    """The foreign shards at their normal placement: the written store equals the oracle's after the same
    write on the foreign host dict, and reads back like it."""
    import zarr_hip

    p = PC.restate(row.id, form.name)
    g = row.src
    host = dict(p.host)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr, meta = _array(store, row, form)
    sel = _write_sel(g)
    val = _data(tuple(s.stop - s.start for s in sel), g["dtype"], 47)
    if form.inshard == "alias":  # the write's shard holds an aliased pair, one of them under the selection
        key = PC.keys_of(row)[0]
        assert key in p.alias
    O.write(host, meta, sel, val)
    arr[sel] = val
    _same(store, host)
    assert _bits(arr[...]).tobytes() == _bits(O.read(host, meta)).tobytes()


# ------------------------------------------------------------------ one launch over stores of different forms
# (row, forms, full-row order: the grid is a quarter of the units)
FUSED = [("u_fused_il3", ["base0", "base1", "base2"], False),
         ("s_il", ["stagger-end-icrc", "gap-start-icrc", "alias-end-icrc"], True),
         ("s_fused_fullrow", ["stagger-start-icrc", "odd_index2-end-icrc"], True)]


@pytest.mark.parametrize("rid,names,fullrow", FUSED, ids=[r for r, _, _ in FUSED])
def test_one_launch_over_different_forms(device, rid, names, fullrow):
    """k_decode_il_multi over three programs whose stores use three forms: the interleaved form (17 chunks
    each: the grid is the sum of the units) and the full-row form (24 chunks each: a quarter of them), and the
    full-row pair over two."""
    import torch

    import zarr_hip

    row = PC.BY_ID[rid]
    fs = {f.name: f for f in PC.forms(row)}
    progs, outs, wants, keep = [], [], [], []
    for name in names:
        p = PC.restate(rid, name)
        store = _foreign_store(device, p)
        arr, _ = _array(store, row, fs[name])
        o = _Out(device, PC.full_shape(row), PC.dtype_of(row))
        progs.append(arr.prepare_read((Ellipsis,), out=o.view)[0])
        outs.append(o)
        wants.append(_bits(p.want).tobytes())
        keep.append((store, arr))
    graph = zarr_hip.ReadGraph(progs, len(progs), device)
    assert graph.launches == 1 and _kernel() == "k_decode_il"
    units = _row_units(row)
    assert int(_lib().zhip_last_grid()) == (len(progs) * units // 4 if fullrow else len(progs) * units)
    for _ in range(2):
        for o in outs:
            o.refill()
        graph.replay()
        torch.cuda.synchronize(device)
        for prog, o, want in zip(progs, outs, wants):
            _, codes = _table(prog, row)
            assert [int(c) for c in prog.data.statuses()["code"]] == codes and prog.data.errflag() == 0
            assert o.bits().tobytes() == want


# ------------------------------------------------------------------ host stores
HOST = [("b_k_decode", "stagger-end-icrc"), ("s_il", "stagger-end-icrc")]


@pytest.mark.parametrize("kind", ["memory", "pinned"])
@pytest.mark.parametrize("rid,name", HOST, ids=[r for r, _ in HOST])
def test_foreign_shards_in_a_host_store(device, rid, name, kind):
    """Whole shards are staged as one piece, so the in-shard residues survive the staging."""
    import zarr_hip

    row = PC.BY_ID[rid]
    form = {f.name: f for f in PC.forms(row)}[name]
    p = PC.restate(rid, name)
    store = zarr_hip.PinnedMemoryStore(dict(p.host)) if kind == "pinned" else zarr_hip.MemoryStore(dict(p.host))
    arr, _ = _array(store, row, form)
    assert _bits(arr[...]).tobytes() == _bits(p.want).tobytes()
    sel = PC.ragged(PC.full_shape(row))
    assert _bits(arr[sel]).tobytes() == _bits(p.want[sel]).tobytes()
