"""Wrong-length chunks and bad shard-index entries in every decode family, per
row and form of tests/damage_cases.py (tests/test_damage_rules.py proves on
the CPU that the oracle raises for each, that the away window reads, and
that no address a damaged input could displace a load to leaves the store).

Per row and form a read is planned with prepare_read over the damaged store,
into a view between two guard bands of a sentinel, and launched:

  1. the damaged chunk's status is exactly ST_LENGTH_MISMATCH / ST_INDEX_OOB
     (ST_MISSING for the marker entry), every other status ST_OK; the error
     word holds exactly the bits of the codes present; results() raises
     ValueError with part B's message (the length message names the batch
     item); the kernel is the row's, by name (fused rows: one launch, its grid);
  2. the regions of all healthy chunks equal the oracle's bytes and the
     guards are untouched (what the damaged chunk's own region holds is not
     specified: the reference raises);
  3. with the damage still present a read of the away window is exact; with
     the blob restored the SAME program is launched twice more: exact both
     times, every status ST_OK (the stale status of the damaged launch must be
     rewritten), the error word zero after reset_errflag, no verdict word left.

An unsharded blob's length is what the store records for it: the damage
changes the recorded length of a blob that stays where it is (a longer blob
runs on into the padding and the next blob: damage_cases.damaged_blob), so
restoring it moves nothing, and the program's chunk record gets the good
length back in place.  An index entry is rewritten in the arena's bytes.

Then the mixed launch (absent key, marker entry, flipped bit, wrong length,
out-of-bounds entry at once: the whole status table), the same on host
stores, and partial writes over a wrong-length chunk."""

import numpy as np
import pytest

import damage_cases as DC
import wide_cases as W
from oracle import oracle as O
from test_damage_rules import _mixed_sharded_host, s_codecs, s_entry, s_host, s_meta, u_host, u_meta
from test_gpu_decode import _data
from test_gpu_shard_index import _failing_write, _index_start, _same, _slot_region
from test_gpu_wide_offsets import _pad_to, _store, backings  # noqa: F401  (backings: a fixture)

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 1 << 16  # bytes of sentinel on either side of an out
FILL_U = 3       # the unsharded rows' fill value (test_damage_rules.u_meta)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _lib():
    from zarr_hip import _native as N

    return N.lib()


def _kernel():
    return _lib().zhip_last_kernel().decode()


def _units(nbytes):
    """32 KiB units of a chunk of `nbytes` payload bytes."""
    return -(-nbytes // 32768)


# ------------------------------------------------------------------ outs between guards
class _Out:
    """A contiguous out of `shape` between two guard bands of 0xA5."""

    def __init__(self, device, shape, dtype):
        import torch

        from zarr_hip.buffer import torch_dtype

        self.dt = np.dtype(dtype)
        self.shape = tuple(shape)
        self.nbytes = int(np.prod(shape)) * self.dt.itemsize
        self.big = torch.full((self.nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=device)
        self.view = self.big[GUARD: GUARD + self.nbytes].view(torch_dtype(self.dt)).view(self.shape)
        assert self.view.is_contiguous() and self.view.data_ptr() == self.big.data_ptr() + GUARD

    def refill(self):
        self.big.fill_(SENT)

    def bits(self):
        """The out as unsigned integers of the item size; asserts the guards."""
        b = self.big.cpu().numpy()
        assert (b[:GUARD] == SENT).all() and (b[GUARD + self.nbytes:] == SENT).all(), "a guard band was written"
        return b[GUARD: GUARD + self.nbytes].view(UINT[self.dt.itemsize]).reshape(self.shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def _healthy_equal(out, want, skip):
    """Every element outside the regions `skip` equals the oracle's."""
    diff = out.bits() != _bits(want)
    for reg in skip:
        diff[reg] = False
    assert not diff.any(), f"{int(diff.sum())} elements of healthy chunks differ"


# ------------------------------------------------------------------ programs
class _Run:
    """`n` programs of one selection (n > 1: captured as ONE fused launch)."""

    def __init__(self, device, arr, shape, dtype, fused, kernel, units=None):
        import zarr_hip

        self.device = device
        n = fused or 1
        self.outs = [_Out(device, shape, dtype) for _ in range(n)]
        self.progs = [arr.prepare_read((Ellipsis,), out=o.view)[0] for o in self.outs]
        self.graph = None
        if fused:
            self.graph = zarr_hip.ReadGraph(self.progs, n, device)
            assert self.graph.launches == 1 and _kernel() == kernel
            if units is not None:  # fused == 2: the full-row form, a quarter of the units; 3: the interleaved
                assert int(_lib().zhip_last_grid()) == (n * units // 4 if fused == 2 else n * units)
        self.kernel = kernel

    def launch(self):
        import torch

        for o in self.outs:
            o.refill()
        if self.graph is not None:
            self.graph.replay()
        else:
            self.progs[0].launch()
            assert _kernel() == self.kernel, _kernel()
        torch.cuda.synchronize(self.device)


def _entries(prog, sharded):
    """[(batch item, slot)] per table entry."""
    item = np.asarray(prog.tables.item_of_chunk).astype(np.int64)
    slot = prog.tables.chunks["slot"].astype(np.int64) if sharded else np.zeros(len(item), np.int64)
    return list(zip(item.tolist(), slot.tolist()))


def _check_statuses(prog, want_codes, want_err, crc_deferred=False):
    """The error word and the status table of the last launch: exactly `want_codes` per entry."""
    from zarr_hip import _native as N

    d = prog.data
    err = d.errflag()
    crc_bit = 1 << N.ST_CRC_MISMATCH
    verdict = d.d_ws[: d.n * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)[:, 0::2].any()
    codes = d.statuses()["code"]  # (merges and clears the deferred verdict words)
    assert [int(c) for c in codes] == list(want_codes), (list(map(int, codes)), list(want_codes))
    if crc_deferred:
        # a CRC verdict may be deferred to the workspace words (ZHIP_DF_DEFER, include/zarrhip.h): its bit is in
        # the error word or its word is in the chunk's bank; every other bit is exact
        assert err & ~crc_bit == want_err & ~crc_bit, (err, want_err)
        assert (err & crc_bit) or verdict
    else:
        assert err == want_err and not verdict, (err, want_err, bool(verdict))


def _clean_twice(run, want):
    """The restored store: the same programs launched twice more."""
    from zarr_hip import _native as N

    for p in run.progs:
        p.data.reset_errflag()
    for _ in range(2):
        run.launch()
        for p, o in zip(run.progs, run.outs):
            _check_statuses(p, [N.ST_OK] * p.data.n, 0)
            assert all(r["status"] == "present" for r in p.results())
            _healthy_equal(o, want, ())
            assert not p.data.d_ws[: p.data.n * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)[:, 0::2].any()


def _set_src_len(prog, j, n):
    """Entry j of the program's device chunk table gets src_len n, in place."""
    import torch

    from zarr_hip.planner import CHUNK_DT

    at = j * CHUNK_DT.itemsize + CHUNK_DT.fields["src_len"][1]
    t = prog.data.d_chunks.view(torch.uint8)
    t[at: at + 8] = torch.from_numpy(np.array([n], "<u8").view(np.uint8).copy()).to(t.device)


# ------------------------------------------------------------------ unsharded rows
class _UCase:
    """One row's healthy array on the device, the oracle's store uploaded as
    it is; placements checked against the table's restatement."""

    def __init__(self, device, row, memory=False):
        import zarr_hip

        self.row, self.device, self.memory = row, device, memory
        self.host, self.want = u_host(row.id)
        self.meta = u_meta(row)
        self.keys = DC.u_keys(row)
        self.place, self.top, self.alloc = DC.arena_layout({k: len(v) for k, v in self.host.items()})
        assert DC.unsharded_safe(row, self.place, self.top, self.alloc)
        if memory:
            self.store = zarr_hip.MemoryStore(dict(self.host))
        else:
            self.store = zarr_hip.DeviceStore.from_host(self.host, device)
            assert all(self.store.placement(k) == self.place[k] for k in self.keys)
            assert self.store.arena.top == self.top and self.store.arena.buf.numel() == self.alloc
        self.arr = zarr_hip.Array.create(self.store, DC.u_shape(row), row.chunk, row.dtype, FILL_U,
                                         codecs=DC.u_codecs(row))
        self.units = len(self.keys) * _units(DC.u_elen(row) - (4 if row.crc else 0))

    def set_len(self, key, n):
        """The store records length n for `key`'s blob, which stays where it is (a host store gets the bytes)."""
        if self.memory:
            self.store.set_sync(key, DC.damaged_blob(self.host, key, n))
            return
        off = self.place[key][0]
        with self.store.arena.lock:
            self.store._index[key] = (off, n)
            self.store.arena.gen += 1  # plans made before this are stale
        got = self.store.get_sync(key).to_bytes()
        assert got == DC.damaged_blob(self.host, key, n)

    def run(self):
        return _Run(self.device, self.arr, DC.u_shape(self.row), self.row.dtype, self.row.fused, self.row.kernel,
                    self.units)


_CASES: dict = {}


def _ucase(device, row, memory=False):
    """The latest row's case (tests run row by row: one array resident at a time)."""
    k = ("u", row.id, memory)
    if k not in _CASES:
        _CASES.clear()
        _CASES[k] = _UCase(device, row, memory)
    return _CASES[k]


def _unsharded_form(device, row, form, memory=False):
    from zarr_hip import _native as N

    c = _ucase(device, row, memory)
    key = c.keys[row.damaged]
    good_len = DC.u_elen(row)
    new_len = dict(DC.u_forms(row))[form]
    touched, away = DC.u_region(row, row.damaged), DC.u_region(row, row.away)
    c.set_len(key, new_len)
    try:
        run = c.run()
        run.launch()
        for p, o in zip(run.progs, run.outs):
            ents = _entries(p, False)
            assert sorted(i for i, _ in ents) == list(range(len(c.keys)))
            codes = [N.ST_LENGTH_MISMATCH if i == row.damaged else N.ST_OK for i, _ in ents]
            _check_statuses(p, codes, 1 << N.ST_LENGTH_MISMATCH)
            with pytest.raises(ValueError) as err:
                p.results()
            assert DC.LEN_MSG in str(err.value) and f"(chunk {row.damaged})" in str(err.value), str(err.value)
            _healthy_equal(o, c.want, (touched,))
        # the damage still present: the away window alone reads exactly
        got = c.arr[away]
        assert _bits(got).tobytes() == _bits(c.want[away]).tobytes()
    finally:
        c.set_len(key, good_len)
    if memory:  # the staged bytes were the damaged ones: the restored store is planned again
        run = c.run()
    else:
        for p in run.progs:
            (j,) = [j for j, (i, _) in enumerate(_entries(p, False)) if i == row.damaged]
            _set_src_len(p, j, good_len)
            p.generations = ((c.store.arena, c.store.arena.gen),)  # the placements are the planned ones again
    _clean_twice(run, c.want)


U_PARAMS = [(r, name) for r in DC.U_ROWS for name, _ in DC.u_forms(r)]


@pytest.mark.parametrize("row,form", U_PARAMS, ids=[f"{r.id}-{f}" for r, f in U_PARAMS])
def test_wrong_length_blob(device, row, form):
    _unsharded_form(device, row, form)


H_PARAMS = [(DC.U_BY_ID[rid], name) for rid in DC.U_HOST for name, _ in DC.u_forms(DC.U_BY_ID[rid])]


@pytest.mark.parametrize("row,form", H_PARAMS, ids=[f"{r.id}-{f}" for r, f in H_PARAMS])
def test_wrong_length_blob_in_a_host_store(device, row, form):
    """A MemoryStore: the blobs are staged to HBM as they are and the kernel
    decides on the staged length -- the same statuses, the same message."""
    _unsharded_form(device, row, form, memory=True)


# ------------------------------------------------------------------ sharded rows
class _SCase:
    """One sharded row's healthy array on the device (index at `loc`)."""

    def __init__(self, device, g, loc, store=None, base=0):
        import zarr_hip

        self.g, self.loc, self.device = g, loc, device
        self.host, self.want = s_host(g, loc)
        self.meta = s_meta(g, loc)
        self.keys = DC.s_keys(g)
        self.place, self.top, self.alloc = DC.arena_layout({k: len(v) for k, v in self.host.items()})
        if store is None:
            self.store = zarr_hip.DeviceStore.from_host(self.host, device)
            assert self.store.arena.buf.numel() == self.alloc
        else:  # placed in a larger arena at `base`, blob by blob
            self.store = store
            _pad_to(store, base)
            for k in self.keys:
                store.set_sync(k, self.host[k])
            self.alloc = store.arena.buf.numel()
        assert all(self.store.placement(k) == (self.place[k][0] + base, self.place[k][1]) for k in self.keys)
        self.base = base
        self.arr = zarr_hip.Array.create(self.store, g["shape"], g["shard"], g["dtype"], 0, codecs=s_codecs(g, loc))
        self.units = len(self.keys) * g["n"] * _units(g["elen"] - (4 if DC.CRC in g["chain"] else 0))

    def put_index(self, key, blob):
        """The index region of `blob` written over `key`'s in the arena (nothing else differs)."""
        import torch

        g = self.g
        good = self.host[key]
        s = _index_start(len(good), g["n"], self.loc, True)
        e = s + 16 * g["n"] + 4
        assert len(blob) == len(good) and blob[:s] == good[:s] and blob[e:] == good[e:]
        off = self.store.placement(key)[0]
        self.store.arena.buf[off + s: off + e] = torch.from_numpy(
            np.frombuffer(blob[s:e], np.uint8).copy()).to(self.device)

    def run(self):
        g = self.g
        return _Run(self.device, self.arr, g["shape"], g["dtype"], g["fused"], g["dec"], self.units)


def _scase(device, g, loc):
    k = ("s", g["id"], loc)
    if k not in _CASES:
        for old in [o for o in _CASES if o[:2] != ("s", g["id"])]:
            del _CASES[old]
        _CASES[k] = _SCase(device, g, loc)
    return _CASES[k]


def _sharded_form(c, name, form, msg):
    from zarr_hip import _native as N

    g = c.g
    key = c.keys[g["item"]]
    coords = tuple(int(i) for i in np.unravel_index(g["item"], g["grid"]))
    touched = _slot_region(g, coords, g["slot"])
    away = _slot_region(g, coords, DC.s_away_slot(g))
    blob, entry, good = s_entry(g, c.loc, c.host[key], form)
    first = c.store.placement(c.keys[0])[0]
    assert DC.index_safe(g, name, entry, good, len(blob), c.store.placement(key)[0], c.alloc, first)
    code = {DC.OOB_MSG: N.ST_INDEX_OOB, DC.LEN_MSG: N.ST_LENGTH_MISMATCH, None: N.ST_MISSING}[msg]
    c.put_index(key, blob)
    try:
        run = c.run()
        run.launch()
        for p, o in zip(run.progs, run.outs):
            if p.index is None:  # the index checks ride in this launch
                assert p.data.n_idx == len(c.keys)
                idx_codes = p.data.index_statuses()["code"]
            else:  # transposed layouts: a launch of their own before it
                assert p.data.n_idx == 0 and p.index.n == len(c.keys)
                idx_codes = p.index.statuses()["code"]
            assert (idx_codes == N.ST_OK).all()  # the index CRC was recomputed: the entry reaches the parse
            ents = _entries(p, True)
            assert sorted(ents) == [(i, s) for i in range(len(c.keys)) for s in range(g["n"])]
            codes = [code if e == (g["item"], g["slot"]) else N.ST_OK for e in ents]
            _check_statuses(p, codes, 0 if msg is None else 1 << code)
            if msg is None:
                assert all(r["status"] == "present" for r in p.results())  # (per shard: the shard is there)
                filled = c.want.copy()
                filled[touched] = 0
                _healthy_equal(o, filled, ())
                continue
            with pytest.raises(ValueError) as err:
                p.results()
            assert msg in str(err.value), (name, str(err.value))
            if msg == DC.LEN_MSG:
                assert f"(chunk {g['item']})" in str(err.value), str(err.value)
            _healthy_equal(o, c.want, (touched,))
        got = c.arr[away]
        assert _bits(got).tobytes() == _bits(c.want[away]).tobytes()
    finally:
        c.put_index(key, c.host[key])
    _clean_twice(run, c.want)


S_FORMS = [f for f in DC.B_FORMS if f[0] not in DC.WIDE_FORMS]
S_PARAMS = [(g, f) for g in DC.S_ROWS for f in S_FORMS]


@pytest.mark.parametrize("g,form", S_PARAMS, ids=[f"{g['id']}-{f[0]}" for g, f in S_PARAMS])
def test_bad_index_entry(device, g, form):
    """Index at the end and at the start of the shard."""
    for loc in ("end", "start"):
        _sharded_form(_scase(device, g, loc), *form)


@pytest.mark.parametrize("g", DC.S_ROWS, ids=[g["id"] for g in DC.S_ROWS])
def test_bad_index_entry_plus_2_32(device, backings, g):  # noqa: F811
    """The two +2^32 forms, in a store whose arena is the body of the large
    backing with the row's shards from WIDE_BASE: shard base + offset + 2^32
    is still inside the backing (test_damage_rules proves it per row)."""
    _CASES.clear()
    for loc in ("end", "start"):
        c = _SCase(device, g, loc, store=_store(device, backings), base=DC.WIDE_BASE)
        assert c.alloc >= W.BODY
        for f in DC.B_FORMS:
            if f[0] in DC.WIDE_FORMS:
                _sharded_form(c, *f)


# ------------------------------------------------------------------ the mixed launch
def _mixed(device, arr, host, meta, keys, shape, dtype, fused, kernel, units, n_per, damage, region_of):
    """One launch over `host` with `damage` applied: the whole status table,
    the error word, the first damaged item's exception, and chunk by chunk the
    bytes of every chunk that does not raise (absent and marker chunks: the fill)."""
    table, want_err = DC.mixed_table(len(keys), n_per, damage)
    run = _Run(device, arr, shape, dtype, fused, kernel, units)
    run.launch()
    raising = {(item, slot) for kind, item, slot in damage if kind in ("crc", "length", "oob")}
    item, slot, kind = DC.first_damaged(damage)
    assert kind == "crc"
    with pytest.raises(ValueError) as ref:
        O.read(host, meta, region_of(item, slot))
    regions = [(e, region_of(*e)) for e in sorted(table) if e not in raising]
    wants = [_bits(O.read(host, meta, reg)).tobytes() for _, reg in regions]
    for p, o in zip(run.progs, run.outs):
        ents = _entries(p, n_per > 1)
        assert sorted(ents) == sorted(table)
        _check_statuses(p, [table[e] for e in ents], want_err, crc_deferred=True)
        with pytest.raises(ValueError) as got:
            p.results()
        assert str(got.value) == str(ref.value)
        bits = o.bits()
        for (e, reg), want in zip(regions, wants):
            assert bits[reg].tobytes() == want, e


@pytest.mark.parametrize("rid", DC.U_MIXED)
def test_mixed_launch_unsharded(device, rid):
    """An absent key, a flipped payload bit and a wrong length in one launch."""
    import zarr_hip

    _CASES.clear()
    row = DC.U_BY_ID[rid]
    good, _ = u_host(rid)
    keys = DC.u_keys(row)
    damage = DC.mixed_damage_unsharded(row)
    host = dict(good)
    for kind, item, _ in damage:
        k = keys[item]
        if kind == "absent":
            del host[k]
        elif kind == "crc":
            b = bytearray(host[k])
            b[len(b) // 3] ^= 0x04
            host[k] = bytes(b)
        else:
            host[k] = host[k][:-4]
    place, top, _ = DC.arena_layout({k: len(v) for k, v in host.items()})
    (short,) = [keys[i] for kind, i, _ in damage if kind == "length"]
    # a healthy blob follows the short one, and a whole chunk read from its offset stays below the arena's top
    assert any(o > place[short][0] for o, _ in place.values())
    assert place[short][0] + DC.u_elen(row) + DC.TAIL_SLACK <= top
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, DC.u_shape(row), row.chunk, row.dtype, FILL_U, codecs=DC.u_codecs(row))
    units = len(keys) * _units(DC.u_elen(row) - (4 if row.crc else 0))
    _mixed(device, arr, host, u_meta(row), keys, DC.u_shape(row), row.dtype, row.fused, row.kernel, units, 1,
           damage, lambda item, slot: DC.u_region(row, item))


@pytest.mark.parametrize("g", DC.S_MIXED, ids=[g["id"] for g in DC.S_MIXED])
def test_mixed_launch_sharded(device, g):
    """An absent shard, a marker entry, a flipped payload bit, a short entry
    and an out-of-bounds entry in one launch."""
    import zarr_hip

    _CASES.clear()
    host, damage = _mixed_sharded_host(g)
    keys = DC.s_keys(g)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, g["shape"], g["shard"], g["dtype"], 0, codecs=s_codecs(g, "end"))
    units = len(keys) * g["n"] * _units(g["elen"] - (4 if DC.CRC in g["chain"] else 0))

    def region_of(item, slot):
        return _slot_region(g, tuple(int(i) for i in np.unravel_index(item, g["grid"])), slot)

    _mixed(device, arr, host, s_meta(g, "end"), keys, g["shape"], g["dtype"], g["fused"], g["dec"], units, g["n"],
           damage, region_of)


# ------------------------------------------------------------------ writes
# (row, the encode kernel a whole write of the row's array takes)
W_ROWS = [("gen_crc", "k_encode"), ("lead4_crc", "k_encode_quad"), ("pair_odd", "k_encode_pair"),
          ("ilh", "k_encode_il"), ("tile2w", "k_encode_tile2")]


@pytest.mark.parametrize("rid,enc", W_ROWS, ids=[r for r, _ in W_ROWS])
def test_writes_over_a_wrong_length_chunk(device, rid, enc):
    """The array is written whole through the GPU (the row's encode kernel,
    the store equal to the oracle's); then per form the damaged chunk's blob
    is replaced by the wrong-length one.  A
    partial write that touches it raises ValueError three times, the store's
    bytes and arena.used_bytes unchanged; a partial write that touches only
    healthy chunks succeeds; a write that covers the damaged chunk whole
    succeeds (the reference never reads a chunk it overwrites whole) -- the
    store equal to the oracle's key by key after each."""
    import zarr_hip

    _CASES.clear()
    row = DC.U_BY_ID[rid]
    good, _ = u_host(rid)
    meta = u_meta(row)
    keys = DC.u_keys(row)
    key = keys[row.damaged]
    store = zarr_hip.DeviceStore(device)
    arr = zarr_hip.Array.create(store, DC.u_shape(row), row.chunk, row.dtype, FILL_U, codecs=DC.u_codecs(row))
    arr[...] = O.read(good, meta)
    assert _kernel() == enc, _kernel()
    _same(store, good)
    touched, away = DC.u_region(row, row.damaged), DC.u_region(row, row.away)
    on = touched[:-1] + (slice(touched[-1].start + 1, touched[-1].stop),)
    beside = away[:-1] + (slice(away[-1].start + 1, away[-1].stop),)
    v_on = _data(tuple(s.stop - s.start for s in on), row.dtype, 3)
    v_beside = _data(tuple(s.stop - s.start for s in beside), row.dtype, 4)
    v_whole = _data(tuple(s.stop - s.start for s in touched), row.dtype, 5)
    for name, new_len in DC.u_forms(row):
        host = dict(good)
        host[key] = DC.damaged_blob(good, key, new_len)
        store.set_sync(key, host[key])
        at, n = store.placement(key)
        assert n == new_len and store.arena.buf.numel() - (at + DC.u_elen(row)) >= DC.u_elen(row)  # inside the arena
        _same(store, host)
        trial = dict(host)
        with pytest.raises(ValueError):
            O.write(trial, meta, on, v_on)
        _failing_write(arr, store, on, v_on, [DC.LEN_MSG])
        O.write(host, meta, beside, v_beside)
        arr[beside] = v_beside
        _same(store, host)
        O.write(host, meta, touched, v_whole)
        arr[touched] = v_whole
        _same(store, host)
        assert arr[...].tobytes() == O.read(host, meta).tobytes(), name
        for k in keys:  # back to the whole array for the next form
            store.set_sync(k, good[k])
