"""Shard indexes of more than 256 entries, index entries that are wrong as
data, and writes that fail: everything byte-exact against the CPU oracle.

A workgroup is 256 lanes and takes 4096 index bytes (256 entries) per pass, so
with at most 256 inner chunks per shard every loop that walks an index runs one
iteration: verify_index / verify_index_pair (the index CRC of the decode
kernels: `nk` passes, a first pass that starts before the index, the
x^-8(idx_E + 4096 - 16 n) correction), k_shard_pack (presence scan with a
carry, compaction by `newrank` across scan passes, `kiters` index-CRC passes
and the matching constant of zhip_shard_pack).  Part A runs them with 257 to
1031 entries, through the production kernels only.

Part B rewrites one index entry of an oracle-built shard (and recomputes the
index CRC, so the entry reaches the parse): the three copies of the entry
check (resolve_unit, k_decode_tile, the host staging path) must report a
status -- a unit whose mode is not OK loads nothing from the entry's offset --
and the read raises ValueError.  Part C writes over such shards, part D makes
writes fail half way: nothing is stored, no arena region is leaked."""

import struct

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_decode import BE, CRC, LE, SHARD, T, _data

pytestmark = pytest.mark.gpu

MAXU = 2 ** 64 - 1
OOB_MSG = "shard index entry points outside the shard blob"
LEN_MSG = "encoded chunk length does not match the fixed-size codec chain"


def _kernel():
    from zarr_hip import _native as N

    return N.lib().zhip_last_kernel()


def _items(store):
    return {k: bytes(v) for k, v in store.to_dict().items() if not k.endswith("zarr.json")}


def _same(store, host):
    got = _items(store)
    assert sorted(got) == sorted(host), sorted(set(got) ^ set(host))[:10]
    for k in host:
        assert got[k] == host[k], f"bytes differ for {k}"


def _make(store, g, codecs, wec=False):
    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    return zarr_hip.Array.create(store, g["shape"], g["shard"], g["dtype"], 0, codecs=codecs,
                                 config=ArrayConfig(write_empty_chunks=wec))


def _meta(g, codecs, wec=False):
    return O.ArrayMeta(tuple(g["shape"]), tuple(g["shard"]), np.dtype(g["dtype"]), 0, codecs=codecs,
                       write_empty_chunks=wec)


def _geom(shape, shard, inner, dtype, chain, **kw):
    g = dict(shape=tuple(shape), shard=tuple(shard), inner=tuple(inner), dtype=dtype, chain=list(chain))
    g.update(kw)
    g["cps"] = tuple(s // i for s, i in zip(shard, inner))
    g["n"] = int(np.prod(g["cps"]))
    g["grid"] = tuple(-(-s // c) for s, c in zip(shape, shard))
    g["elen"] = int(np.prod(inner)) * np.dtype(dtype).itemsize + (4 if CRC in chain else 0)
    return g


def _slot_region(g, shard_coords, slot):
    """Array region of the inner chunk at C-order `slot` of the shard."""
    ic = np.unravel_index(slot, g["cps"])
    return tuple(slice(sc * s + int(c) * i, sc * s + (int(c) + 1) * i)
                 for sc, s, c, i in zip(shard_coords, g["shard"], ic, g["inner"]))


def _index_start(blob_len, n, loc, has_crc):
    return 0 if loc == "start" else blob_len - (16 * n + (4 if has_crc else 0))


def _entry(blob, n, loc, has_crc, slot):
    at = _index_start(len(blob), n, loc, has_crc) + 16 * slot
    return struct.unpack("<QQ", blob[at: at + 16])


def _rewrite_entry(blob, n, loc, has_crc, slot, off, ln):
    """The blob with index entry `slot` = (off, ln); the index trailer is
    recomputed with the oracle's crc32c so the index check passes."""
    b = bytearray(blob)
    s = _index_start(len(b), n, loc, has_crc)
    b[s + 16 * slot: s + 16 * slot + 16] = struct.pack("<QQ", off, ln)
    if has_crc:
        b[s + 16 * n: s + 16 * n + 4] = struct.pack("<I", O.crc32c(bytes(b[s: s + 16 * n])))
    return bytes(b)


def _first_key(g):
    return "/".join(["c"] + ["0"] * len(g["shape"]))


# ===================================================================== part A

def _k1d(n):
    return _geom((4 * n,), (4 * n,), (4,), "uint8", [LE, CRC], id=f"k_decode_1d_{n}", dec=b"k_decode", index="fused")


A_CASES = [
    # k_decode (generic) with the fused verify_index: idx_E 6720, nk 2, lo -1472
    _geom((40, 84), (40, 42), (2, 2), "int16", [LE, CRC], id="k_decode_420", dec=b"k_decode", index="fused"),
    # the same at the pass boundaries
    _k1d(256), _k1d(257), _k1d(512), _k1d(513), _k1d(1031),
    # no inner CRC, not a row layout: the index is checked by its own launch
    _geom((40, 84), (40, 42), (2, 2), "int16", [BE], id="own_index_420", index="own"),
    # 17 x 16 inner chunks (a non-square Morton order), leading index workgroups
    _geom((1088, 2048), (1088, 1024), (64, 64), "int32", [LE], id="lead4", dec=b"k_decode_lead4",
          enc=b"k_encode_quad", index="fused"),
    _geom((1088, 2048), (1088, 1024), (64, 64), "int32", [LE, CRC], id="lead4_crc", dec=b"k_decode_lead4",
          enc=b"k_encode_quad", index="fused"),
    _geom((544, 2048), (544, 1024), (32, 64), "int32", [LE], id="lead8", dec=b"k_decode_lead8", index="fused"),
    _geom((1088, 2048), (1088, 2048), (64, 128), "float32", [BE, CRC], id="pair", dec=b"k_decode_pair",
          enc=b"k_encode_pair", index="fused"),
    _geom((1088, 2048), (1088, 2048), (64, 128), "float32", [LE], id="lead", dec=b"k_decode_lead", index="fused"),
    # 272 chunks of 256 KiB (2176 units).  k_decode_il / k_decode_ilh fuse an index
    # check of ONE pass per lane, so zhip_decode hands a launch whose indexes
    # have more than 256 entries to k_decode_pair (verify_index_pair's loop) ...
    _geom((544, 1024, 32), (544, 1024, 32), (32, 64, 32), "float32", [LE, CRC], id="il_geometry_index_crc",
          dec=b"k_decode_pair", enc=b"k_encode_il", index="fused", extra=[((slice(0, 64),), b"k_decode_pair")]),
    # ... and the il kernels parse entries past 256 only under an index without a
    # CRC: the whole array is k_decode_il, [0:64] (32 chunks, 256 units) k_decode_ilh
    _geom((544, 1024, 32), (544, 1024, 32), (32, 64, 32), "float32", [LE, CRC], id="il", dec=b"k_decode_il",
          enc=b"k_encode_il", index="none", index_codecs=(LE,), extra=[((slice(0, 64),), b"k_decode_ilh")]),
    # tiled transposed inner chunks
    _geom((68, 64, 64), (68, 64, 64), (4, 16, 16), "float32", [T((2, 1, 0)), LE, CRC], id="tiled", index="own",
          dec_prefix=b"k_decode_tile"),
]

A_SLOTS = [0, 254, 255, 256, 257, 258]


def _elided(g, data):
    """data with the inner chunks at C-order slots 0, 254..258 and n-1 of every
    shard set to fill: runs of elided ranks on both sides of a scan pass."""
    d = data.copy()
    for sc in np.ndindex(*g["grid"]):
        for slot in sorted({s for s in A_SLOTS + [g["n"] - 1] if s < g["n"]}):
            d[_slot_region(g, sc, slot)] = 0
    return d


def _ragged(shape):
    if len(shape) == 1:
        return (slice(3, shape[0] - 5, 3),)
    return tuple(slice(1 + d, n - 2 - d) for d, n in enumerate(shape[:-1])) + (slice(1, shape[-1] - 1, 2),)


def _check_dec_kernel(g):
    if g.get("dec") is not None:
        assert _kernel() == g["dec"], _kernel()
    if g.get("dec_prefix") is not None:
        assert _kernel().startswith(g["dec_prefix"]), _kernel()


@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("g", A_CASES, ids=[c["id"] for c in A_CASES])
def test_large_index(device, g, loc):
    import zarr_hip

    n = g["n"]
    assert n >= 256
    index_codecs = g.get("index_codecs", (LE, CRC))
    codecs = [SHARD(g["inner"], g["chain"], loc, index=index_codecs)]
    meta = _meta(g, codecs)
    data = _data(g["shape"], g["dtype"], seed=11)
    # (i) a whole write through the GPU: k_shard_pack's entries, order and index CRC
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    store = zarr_hip.DeviceStore(device)
    arr = _make(store, g, codecs)
    arr[...] = data
    if g.get("enc") is not None:
        assert _kernel() == g["enc"], _kernel()
    _same(store, host)
    mstore = zarr_hip.MemoryStore()
    _make(mstore, g, codecs)[...] = data
    _same(mstore, host)
    del mstore
    # (ii) elided inner chunks: compaction and newrank across scan passes
    data2 = _elided(g, data)
    O.write(host, meta, (Ellipsis,), data2)
    arr[...] = data2
    _same(store, host)
    # ... kept under write_empty_chunks (ZHIP_PF_KEEP_EMPTY)
    meta_w = _meta(g, codecs, wec=True)
    host_w = {}
    O.write(host_w, meta_w, (Ellipsis,), data2)
    store_w = zarr_hip.DeviceStore(device)
    _make(store_w, g, codecs, wec=True)[...] = data2
    _same(store_w, host_w)
    del store_w, host_w
    # ... and a partial-shard write touching only an inner chunk at a slot >= 256
    # (every other inner chunk keeps its stored state: the writer's `mode`)
    p = min(300, n - 1)
    reg = _slot_region(g, (0,) * len(g["shape"]), p)
    if g["inner"][-1] > 1:
        reg = reg[:-1] + (slice(reg[-1].start + 1, reg[-1].stop),)
    val = _data(tuple(s.stop - s.start for s in reg), g["dtype"], seed=9)
    O.write(host, meta, reg, val)
    arr[reg] = val
    _same(store, host)
    # (iii) reads of a store built by the oracle (elided entries included)
    rstore = zarr_hip.DeviceStore.from_host(host, device)
    rarr = _make(rstore, g, codecs)
    n_shards = int(np.prod(g["grid"]))
    prog, _ = rarr.prepare_read((Ellipsis,))
    if g["index"] == "fused":
        assert prog.index is None and prog.data.n_idx == n_shards
    elif g["index"] == "own":
        assert prog.index is not None
    else:
        assert prog.index is None and prog.data.n_idx == 0
    sels = [((Ellipsis,), True), (_ragged(g["shape"]), False)] + [(s, k) for s, k in g.get("extra", [])]

    def read_all():
        for sel, k in sels:
            got = rarr[sel]
            if k is True:
                _check_dec_kernel(g)
            elif k:
                assert _kernel() == k, _kernel()
            want = O.read(host, meta, sel)
            assert got.shape == want.shape
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), sel

    read_all()
    if CRC not in index_codecs:
        return
    # one bit of an entry in the second pass, the CRC left alone: the oracle's message
    key = _first_key(g)
    good = host[key]
    bad = bytearray(good)
    bad[_index_start(len(bad), n, loc, True) + 16 * min(300, n - 1) + 3] ^= 0x04
    host[key] = bytes(bad)
    rstore.set_sync(key, bytes(bad))
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    assert "checksum" in str(want.value)
    for sel, _ in sels[:1] + sels[2:]:
        with pytest.raises(ValueError) as got:
            rarr[sel]
        assert str(got.value) == str(want.value)
    host[key] = good
    rstore.set_sync(key, good)
    read_all()


# ===================================================================== part B

B_FORMS = [  # (name, (off, len, elen, blob_len) -> entry, message; None: a missing chunk)
    ("off_plus_2^32", lambda o, l, e, b: (o + 2 ** 32, l), OOB_MSG),
    ("len_plus_2^32", lambda o, l, e, b: (o, l + 2 ** 32), OOB_MSG),
    ("off_past_blob", lambda o, l, e, b: (b + 1, l), OOB_MSG),
    ("off_in_tail", lambda o, l, e, b: (b - 4, l), OOB_MSG),
    ("off_marker_only", lambda o, l, e, b: (MAXU, e), OOB_MSG),
    ("len_marker_only", lambda o, l, e, b: (o, MAXU), OOB_MSG),
    ("len_minus_4", lambda o, l, e, b: (o, e - 4), LEN_MSG),
    ("len_plus_4", lambda o, l, e, b: (o, e + 4), LEN_MSG),
    ("missing", lambda o, l, e, b: (MAXU, MAXU), None),
]

B_CASES = [  # slot: the entry rewritten; kernel: with an index CRC / without one
    _geom((16, 24), (8, 8), (4, 4), "int16", [LE, CRC], id="k_decode", slot=1, dec=(b"k_decode", b"k_decode")),
    _geom((256, 256), (128, 128), (64, 64), "int32", [LE], id="lead4", slot=1,
          dec=(b"k_decode_lead4", b"k_decode_lead4")),
    _geom((256, 256), (128, 128), (64, 64), "int32", [LE, CRC], id="lead4_crc", slot=2,
          dec=(b"k_decode_lead4", b"k_decode_lead4")),
    _geom((128, 256), (128, 256), (64, 128), "float32", [LE, CRC], id="pair", slot=1,
          dec=(b"k_decode_pair", b"k_decode_pair")),
    # (without an index CRC there are no leading index workgroups: the pair kernel)
    _geom((128, 256), (128, 256), (64, 128), "float32", [LE], id="lead", slot=2,
          dec=(b"k_decode_lead", b"k_decode_pair")),
    _geom((64, 64, 128), (64, 64, 128), (32, 64, 32), "float32", [LE, CRC], id="ilh", slot=1,
          dec=(b"k_decode_ilh", b"k_decode_ilh")),
    _geom((64, 64, 64), (64, 64, 64), (32, 32, 32), "float32", [T((2, 1, 0)), LE, CRC], id="tiled", slot=5,
          dec=(b"k_decode_tile", b"k_decode_tile"), prefix=True),
    # a host store: the index is parsed on the host while the pieces are staged
    _geom((16, 24), (8, 8), (4, 4), "int16", [LE, CRC], id="k_decode_memory", slot=1, memory=True),
    _geom((256, 256), (128, 128), (64, 64), "int32", [LE], id="lead4_memory", slot=1, memory=True),
    # a bad entry in the second pass of a 420-entry index
    _geom((40, 84), (40, 42), (2, 2), "int16", [LE, CRC], id="k_decode_420", slot=300, dec=(b"k_decode", b"k_decode")),
]


def _b_store(g, host, device):
    import zarr_hip

    return zarr_hip.MemoryStore(dict(host)) if g.get("memory") else zarr_hip.DeviceStore.from_host(host, device)


def _untouched_sel(g, slot):
    """The inner chunk of shard 0 farthest (in C order) from `slot`."""
    other = g["n"] - 1 if slot < g["n"] // 2 else 0
    return _slot_region(g, (0,) * len(g["shape"]), other)


@pytest.mark.parametrize("index", [(LE,), (LE, CRC)], ids=["index_bytes", "index_crc"])
@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("g", B_CASES, ids=[c["id"] for c in B_CASES])
def test_bad_index_entry_read(device, g, loc, index):
    has_crc = CRC in index
    codecs = [SHARD(g["inner"], g["chain"], loc, index=index)]
    meta = _meta(g, codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(g["shape"], g["dtype"], seed=13))
    key, slot, n = _first_key(g), g["slot"], g["n"]
    good = host[key]
    off, ln = _entry(good, n, loc, has_crc, slot)
    assert ln == g["elen"] and off + ln + 4 <= len(good)  # (so elen + 4 stays in range)
    store = _b_store(g, host, device)
    arr = _make(store, g, codecs)
    touched = _slot_region(g, (0,) * len(g["shape"]), slot)
    away = _untouched_sel(g, slot)

    def exact(sel):
        got = arr[sel]
        want = O.read(host, meta, sel)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), sel

    def dec_kernel():
        if g.get("dec") is not None:
            k = g["dec"][0 if has_crc else 1]
            assert _kernel().startswith(k) if g.get("prefix") else _kernel() == k, _kernel()

    exact((Ellipsis,))
    dec_kernel()
    for name, form, msg in B_FORMS:
        e_off, e_len = form(off, ln, g["elen"], len(good))
        host[key] = _rewrite_entry(good, n, loc, has_crc, slot, e_off, e_len)
        store.set_sync(key, host[key])
        if msg is None:  # (2^64-1, 2^64-1): a missing inner chunk, fill
            exact((Ellipsis,))
            exact(touched)
            continue
        for sel in ((Ellipsis,), touched):
            with pytest.raises(ValueError):
                O.read(host, meta, sel)
            with pytest.raises(ValueError) as err:
                arr[sel]
            assert msg in str(err.value), (name, sel, str(err.value))
            if sel == (Ellipsis,):
                dec_kernel()
        exact(away)
    host[key] = good
    store.set_sync(key, good)
    exact((Ellipsis,))
    exact(touched)


# ===================================================================== part C

C_CASES = [
    _geom((16, 24), (8, 8), (4, 4), "int16", [LE, CRC], id="k_decode", slot=1),
    _geom((256, 256), (128, 128), (64, 64), "int32", [LE, CRC], id="lead4_crc", slot=2),
    _geom((256, 256), (128, 128), (64, 64), "int32", [LE], id="lead4", slot=1),
]


def _used(store):
    return store.arena.used_bytes if hasattr(store, "arena") else None


def _failing_write(arr, store, sel, val, msgs):
    """A write that must raise ValueError with one of `msgs`, store nothing
    and leak nothing -- repeated, so a leak per attempt would add up."""
    before, used = store.to_dict(), _used(store)
    for _ in range(3):
        with pytest.raises(ValueError) as err:
            arr[sel] = val
        assert any(m in str(err.value) for m in msgs), str(err.value)
        assert store.to_dict() == before
        assert _used(store) == used


@pytest.mark.parametrize("kind", ["device", "memory"])
@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("g", C_CASES, ids=[c["id"] for c in C_CASES])
def test_partial_write_over_bad_shard(device, g, loc, kind):
    """Partial writes onto a shard with one bad inner chunk, or a bad index.

    Touching the bad inner chunk partially: the oracle raises, and so does the
    GPU write (the oracle's message for a CRC mismatch, the two entry messages
    otherwise).  NOT touching it, the reference carries the stored slice over
    verbatim, whatever its offset and length -- the oracle's write succeeds.
    The fixed-size packer (k_shard_pack: entries of one length at rank * elen)
    cannot reproduce such a shard, so this library refuses the write with the
    out-of-bounds / length ValueError instead; an untouched inner
    chunk that only fails its CRC is carried over like the reference.  Every
    failed write leaves the store's bytes and the arena's accounting as they
    were, and once the shard is restored the same write succeeds and the store
    equals the oracle's."""
    import zarr_hip

    codecs = [SHARD(g["inner"], g["chain"], loc)]
    meta = _meta(g, codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(g["shape"], g["dtype"], seed=17))
    key, slot, n = _first_key(g), g["slot"], g["n"]
    good = host[key]
    off, ln = _entry(good, n, loc, True, slot)
    store = zarr_hip.MemoryStore(dict(host)) if kind == "memory" else zarr_hip.DeviceStore.from_host(host, device)
    arr = _make(store, g, codecs)
    zero = (0,) * len(g["shape"])
    reg = _slot_region(g, zero, slot)
    on = reg[:-1] + (slice(reg[-1].start + 1, reg[-1].stop),)          # the bad inner chunk, partially
    away_reg = _untouched_sel(g, slot)
    away = away_reg[:-1] + (slice(away_reg[-1].start + 1, away_reg[-1].stop),)
    v_on = _data(tuple(s.stop - s.start for s in on), g["dtype"], seed=3)
    v_away = _data(tuple(s.stop - s.start for s in away), g["dtype"], seed=4)

    def oracle_raises(sel, val):
        trial = dict(host)
        with pytest.raises(ValueError) as err:
            O.write(trial, meta, sel, val)
        return str(err.value)

    def restored_write_matches(sel, val):
        store.set_sync(key, good)
        host[key] = good
        trial = dict(host)
        O.write(trial, meta, sel, val)
        arr[sel] = val
        _same(store, trial)
        store.set_sync(key, good)  # back to the unwritten shard for the next form

    bad_entries = [((off + 2 ** 32, ln), OOB_MSG), ((len(good) + 1, ln), OOB_MSG), ((off, MAXU), OOB_MSG),
                   ((off, g["elen"] - 4), LEN_MSG), ((off, g["elen"] + 4), LEN_MSG)]
    for (e_off, e_len), msg in bad_entries:
        host[key] = _rewrite_entry(good, n, loc, True, slot, e_off, e_len)
        store.set_sync(key, host[key])
        oracle_raises(on, v_on)
        _failing_write(arr, store, on, v_on, [msg])
        trial = dict(host)
        O.write(trial, meta, away, v_away)  # the reference succeeds: the slice is carried over
        _failing_write(arr, store, away, v_away, [msg])
        restored_write_matches(on, v_on)
        restored_write_matches(away, v_away)
    if CRC in g["chain"]:  # a payload bit of the inner chunk: the oracle's checksum message
        b = bytearray(good)
        b[off + 5] ^= 0x20
        host[key] = bytes(b)
        store.set_sync(key, host[key])
        _failing_write(arr, store, on, v_on, [oracle_raises(on, v_on)])
        trial = dict(host)  # untouched: carried over verbatim by both
        O.write(trial, meta, away, v_away)
        arr[away] = v_away
        _same(store, trial)
        restored_write_matches(on, v_on)
    # the index CRC wrong: the oracle's message, whichever inner chunk the write touches
    b = bytearray(good)
    b[_index_start(len(b), n, loc, True) + 16 * slot + 2] ^= 0x01
    host[key] = bytes(b)
    store.set_sync(key, host[key])
    for sel, val in ((on, v_on), (away, v_away)):
        _failing_write(arr, store, sel, val, [oracle_raises(sel, val)])
    restored_write_matches(on, v_on)


# ===================================================================== part D

def _d_store(kind, device):
    import zarr_hip

    return zarr_hip.MemoryStore() if kind == "memory" else zarr_hip.DeviceStore(device)


D_GRIDS = [  # (shape, grid, dtype, fill, corrupted chunk of a later spec group, a selection over every group)
    ((30, 30), ([10, 20], [20, 10]), "float32", -1.0, "c/1/1", (slice(8, 14), slice(15, 25))),
    # the reference's rectilinear metadata fixture geometry
    ((100, 100), ([10, 20, 30, 40], 50), "float64", 0.0, "c/2/1", (slice(5, 95), slice(40, 60))),
]


@pytest.mark.parametrize("kind", ["memory", "device"])
@pytest.mark.parametrize("case", range(len(D_GRIDS)))
def test_failed_multi_group_write_stores_nothing(device, case, kind):
    """A partial write over chunks of several spec groups (a rectilinear
    grid), one chunk of a later group corrupted: the merge read's CRC error
    raises the oracle's message before ANY group is committed, and every
    group's reserved arena regions are given back."""
    import zarr_hip

    shape, grid, dtype, fill, bad_key, sel = D_GRIDS[case]
    codecs = [LE, CRC]
    store = _d_store(kind, device)
    arr = zarr_hip.Array.create(store, shape, grid, dtype, fill, codecs=codecs)
    meta = O.ArrayMeta(shape, grid, np.dtype(dtype), fill, codecs=codecs)
    data = _data(shape, dtype, seed=19)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    arr[...] = data
    _same(store, host)
    groups = len({id(it[1]) for it in arr.batch_info(sel)[0]})
    assert groups >= 2
    good = host[bad_key]
    b = bytearray(good)
    b[9] ^= 0x02
    host[bad_key] = bytes(b)
    store.set_sync(bad_key, bytes(b))
    val = _data(tuple(s.stop - s.start for s in sel), dtype, seed=23)
    trial = dict(host)
    with pytest.raises(ValueError) as want:
        O.write(trial, meta, sel, val)
    _failing_write(arr, store, sel, val, [str(want.value)])
    _same(store, host)
    host[bad_key] = good
    store.set_sync(bad_key, good)
    O.write(host, meta, sel, val)
    arr[sel] = val
    _same(store, host)


def test_failed_partial_chunk_write_leaks_nothing(device):
    """The regular-grid path (one spec, ChunkWriter._encode_chunks): a partial
    write that merges with a corrupted chunk leaves the arena's accounting
    unchanged."""
    import zarr_hip

    codecs = [LE, CRC]
    meta = O.ArrayMeta((16, 16), (8, 8), np.dtype("int32"), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((16, 16), "int32", seed=29))
    b = bytearray(host["c/1/1"])
    b[7] ^= 0x40
    host["c/1/1"] = bytes(b)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (16, 16), (8, 8), "int32", 0, codecs=codecs)
    used = store.arena.used_bytes
    for _ in range(3):
        with pytest.raises(ValueError):
            arr[4:12, 4:12] = np.int32(5)
        assert store.arena.used_bytes == used
