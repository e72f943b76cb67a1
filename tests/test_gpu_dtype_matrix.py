"""Every dtype through every kernel family (table: tests/dtype_cases.py): byte
order in store, the fill a missing chunk shows, and chunk emptiness, each
decided by the oracle (O.write / O.read, and O.all_equal inside them).

  test_roundtrip[dtype-endian-family]   read of an oracle-written store with a
      chunk dropped, the same data written here equal to the oracle's store key
      by key, the oracle reading this store, both kernel names
  test_emptiness[dtype-fill-family]     one chunk per content class: the key
      set and bytes of a whole write, write_empty_chunks, and a partial write
      that turns a kept chunk into fill
  the boundary (HipCodecPipeline driven with zarr-shaped objects), the
  selection kernel, and the refusal of complex128 before anything is reserved

On the commit before complex64 became a layout of its own
(ZHIP_LF_COMPLEX) exactly these rows failed: big-endian complex64 (an 8-byte
reversal exchanged the components), the complex emptiness rows (compared
bitwise) and the refusal rows; complex64 arrays could not be created at all
(the fill's JSON form)."""

import numpy as np
import pytest

import dtype_cases as D
from oracle import oracle as O
from tests import zarr_fakes as Z

pytestmark = pytest.mark.gpu


def _kernel():
    from zarr_hip import _native as N

    return N.lib().zhip_last_kernel().decode()


def _chunks_of(store):
    return {k: v for k, v in store.to_dict().items() if not k.endswith("zarr.json")}


def _assert_stores_equal(store, host):
    got = _chunks_of(store)
    assert sorted(got) == sorted(host), sorted(set(got) ^ set(host))[:10]
    for k in host:
        assert store.get_sync(k).to_bytes() == host[k], f"bytes differ for {k}"
    return got


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


_FILL = {"b": True, "i": -3, "u": 3}


def _roundtrip_fill(dt):
    """A fill whose bytes all differ, so a missing chunk shows the byte order
    the fill was planted in."""
    if dt.kind == "f":
        return dt.type(-2.5)
    if dt.kind == "c":
        return D.C("1.5", "-2.5")
    return dt.type(_FILL[dt.kind]) if dt.itemsize == 1 else dt.type(0x0102030405060708 & ((1 << (8 * dt.itemsize - 1)) - 1))


ROUNDTRIP = [(n, e, f) for n, e, _ in D.DTYPES for f in D.FAMILIES]


@pytest.mark.parametrize("name,endian,fam", ROUNDTRIP,
                         ids=[f"{n}-{'le' if e is D.LE else 'be'}-{f.id}" for n, e, f in ROUNDTRIP])
def test_roundtrip(device, name, endian, fam):
    import zarr_hip

    dt = np.dtype(name)
    it = dt.itemsize
    shape, chunk, codecs = fam.shape(it), fam.chunk(it), D.codecs_for(fam, endian, it)
    fill = _roundtrip_fill(dt)
    meta = O.ArrayMeta(shape, chunk, dt, fill, codecs=codecs)
    data = D.sample(shape, dt, seed=len(name) + it)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    # -- the read: the oracle's store with one chunk dropped
    part = dict(host)
    del part[sorted(part)[1]]
    want = O.read(part, meta)
    store = zarr_hip.DeviceStore.from_host(part, device)
    arr = zarr_hip.Array.create(store, shape, chunk, dt, fill, codecs=codecs)
    got = arr[...]
    assert D.kernel_matches(_kernel(), fam.decode), (_kernel(), fam.decode)
    assert got.dtype == dt and _bits(got) == _bits(want)
    # -- the write: the same data through the GPU gives the oracle's store
    out = zarr_hip.DeviceStore(device)
    warr = zarr_hip.Array.create(out, shape, chunk, dt, fill, codecs=codecs)
    warr[...] = data
    assert _kernel() == fam.encode
    ours = _assert_stores_equal(out, host)
    # -- and the oracle reads this store exactly
    assert _bits(O.read(ours, meta)) == _bits(data)
    assert _bits(warr[...]) == _bits(data)


# the swapped store for every multi-byte dtype (emptiness is decided on native-order values, and the swap
# follows it); complex64 in both byte orders: its rule is chosen by the compile-time item mode, and the
# unswapped mode is an encode instantiation of its own (for_item_enc, csrc/zhip_dispatch.h)
EMPT = [(n, fid, fv, f, D.LE if np.dtype(n).itemsize == 1 else D.BE) for n, fid, fv in D.EMPTINESS for f in D.FAMILIES] + \
    [(n, fid, fv, f, D.LE) for n, fid, fv in D.EMPTINESS if np.dtype(n).kind == "c" for f in D.FAMILIES]


@pytest.mark.parametrize("name,fid,fill,fam,endian", EMPT,
                         ids=[f"{n}-{fid}-{f.id}" + ("-le" if n == "complex64" and e is D.LE else "")
                              for n, fid, _, f, e in EMPT])
def test_emptiness(device, name, fid, fill, fam, endian):
    import zarr_hip
    from zarr_hip import ArrayConfig

    dt = np.dtype(name)
    it = dt.itemsize
    chunk, codecs = fam.chunk(it), D.codecs_for(fam, endian, it)
    shape, data, regions = D.truth_table_array(fam, dt, fill)
    classes = D.classes_of(dt, fill)

    def both(wec):
        meta = O.ArrayMeta(shape, chunk, dt, fill, codecs=codecs, write_empty_chunks=wec)
        store = zarr_hip.DeviceStore(device)
        arr = zarr_hip.Array.create(store, shape, chunk, dt, fill, codecs=codecs,
                                    config=ArrayConfig(write_empty_chunks=wec))
        host = {}
        O.write(host, meta, (Ellipsis,), data)
        arr[...] = data
        assert _kernel() == fam.encode
        _assert_stores_equal(store, host)
        return meta, store, arr, host

    # 1. written whole: the oracle's keys (and index entries: the shard bytes) exactly
    meta, store, arr, host = both(False)
    kept = [not O.all_equal(data[r], np.asarray(fill, dt)) for r in regions]
    if dt.kind in "fc":
        assert any(kept) and not all(kept)
    assert _bits(arr[...]) == _bits(O.read(host, meta))
    # 2. a partial write that turns one kept unit into fill (and cuts one row plane off its neighbour): the key
    #    goes, or, in the sharded family, the shard loses the unit's index entry and bytes
    k = kept.index(True, 1) if True in kept[1:] else kept.index(True)
    u0 = D.unit(fam, it)[0]
    sel = (slice(max(u0 * k - 1, 0), u0 * (k + 1)),) + (slice(None),) * (len(shape) - 1)
    val = np.empty(tuple(len(range(*s.indices(n))) for s, n in zip(sel, shape)), dt)
    val[...] = fill
    before = dict(host)
    O.write(host, meta, sel, val)
    arr[sel] = val
    _assert_stores_equal(store, host)
    if fam.inner:
        assert any(key not in host or len(host[key]) < len(before[key]) for key in before), classes[k][0]
    else:
        assert len(host) < len(before), (classes[k][0], sorted(set(before) - set(host)))
    assert _bits(arr[...]) == _bits(O.read(host, meta))
    # 3. write_empty_chunks: every class is kept
    meta, store, arr, host = both(True)
    assert len(host) == int(np.prod([-(-s // c) for s, c in zip(shape, chunk)]))


# ------------------------------------------------------------------ the boundary
BOUNDARY = [(n, sh) for n in ("complex64", "float16") for sh in (False, True)]


@pytest.mark.parametrize("name,sharded", BOUNDARY, ids=[f"{n}-{'sharded' if s else 'plain'}" for n, s in BOUNDARY])
def test_boundary_big_endian(device, name, sharded):
    """HipCodecPipeline driven the way zarr drives it (ZDType, zarr-shaped
    ArraySpec and stores): a big-endian chain, read then a sequence of writes,
    keys and bytes equal to the oracle's after each."""
    from zarr_hip import HipCodecPipeline

    dt = np.dtype(name)
    shape, chunks = (40, 36), (16, 16)
    codecs = [D.SHARD((8, 8), [D.BE, D.CRC])] if sharded else [D.BE, D.CRC]
    fill = D.C("qnan", "+0") if dt.kind == "c" else dt.type(np.nan)
    meta = O.ArrayMeta(shape, chunks, dt, fill, codecs=codecs)
    spec = Z.ArraySpec(chunks, Z.ZDType(dt), fill, Z.ArrayConfig(), Z.cpu_prototype)
    pipe = HipCodecPipeline.from_codecs(Z.zcodecs(codecs)).evolve_from_array_spec(spec)
    data = D.sample(shape, dt, 5)
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    host.pop("c/1/0")
    store = Z.MemoryStore(dict(host))
    for sel in [(Ellipsis,), (slice(3, 39), slice(None, None, 3)), (7, slice(2, 30))]:
        batch, out_shape = Z.batch_for(shape, chunks, sel, store, spec)
        out = Z.NDBuffer.create(shape=out_shape, dtype=dt)
        pipe.read_sync(batch, out)
        assert _bits(out.as_numpy_array()) == _bits(O.read(host, meta, sel))
    ours, want = Z.MemoryStore(), {}
    nan_block = np.empty((10, 10), dt)
    nan_block[...] = D.C("+0", "snan") if dt.kind == "c" else np.array([0xFC01], np.uint16).view(dt)[0]
    for sel, val in [((Ellipsis,), data), ((slice(5, 30), slice(3, 17)), D.sample((25, 14), dt, 6)),
                     ((slice(16, 26), slice(16, 26)), nan_block),       # NaNs of another pattern into a NaN-fill array
                     ((slice(16, 32), slice(16, 32)), np.broadcast_to(nan_block[0, 0], (16, 16)))]:
        batch, _ = Z.batch_for(shape, chunks, sel, ours, spec)
        pipe.write_sync(batch, Z.NDBuffer(np.ascontiguousarray(val)))
        O.write(want, meta, sel, val)
        assert sorted(ours._store_dict) == sorted(want)
        for k in want:
            assert ours._store_dict[k] == want[k], k
    assert "c/1/1" not in want  # the all-NaN chunk was elided under a NaN fill of another pattern


# ------------------------------------------------------------------ the selection kernel
@pytest.mark.parametrize("name", ["complex64", "float16", "bool"])
def test_orthogonal_and_coordinate_reads(device, name):
    """k_select_copy moves items by size alone: one orthogonal and one
    coordinate read of a big-endian array against numpy indexing of the
    oracle's read."""
    import zarr_hip
    from zarr_hip import buffer

    dt = np.dtype(name)
    shape, chunks = (50, 37, 29), (16, 16, 8)
    codecs = [D.LE if dt.itemsize == 1 else D.BE, D.CRC]
    fill = _roundtrip_fill(dt)
    meta = O.ArrayMeta(shape, chunks, dt, fill, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), D.sample(shape, dt, 11))
    del host["c/1/1/1"]
    mirror = O.read(host, meta)
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dt, fill, codecs=codecs)
    i0, i2 = np.array([40, 2, 2, 17]), np.array([28, 0, 9])
    want = mirror[i0][:, 5:30:3][:, :, i2]
    assert _bits(arr.oindex[i0, 5:30:3, i2]) == _bits(want)
    assert _kernel() == "k_select_copy"
    pts = (np.array([0, 49, 17, 20]), np.array([36, 0, 16, 20]), np.array([28, 15, 16, 10]))
    assert _bits(arr.vindex[pts]) == _bits(mirror[pts])
    assert _kernel() == "k_select_copy"
    t = arr.get(pts)  # the device result
    assert t.is_cuda and _bits(buffer.to_numpy(t, dt)) == _bits(mirror[pts])


# ------------------------------------------------------------------ the buffer interface's rule
@pytest.mark.parametrize("name,fid,fill", D.EMPTINESS, ids=[f"{n}-{f}" for n, f, _ in D.EMPTINESS])
def test_ndbuffer_all_equal(device, name, fid, fill):
    """NDBuffer.all_equal on the device (the interface's statement of the rule;
    the write path does not call it) against O.all_equal, class by class."""
    from zarr_hip.buffer import NDBuffer

    dt = np.dtype(name)
    for cls in D.classes_of(dt, fill):
        chunk = D.class_chunk(cls, (3, 5), dt)
        nd = NDBuffer(chunk)
        assert nd.dtype == dt and _bits(nd.as_numpy_array()) == _bits(chunk)
        assert nd.all_equal(fill) == O.all_equal(chunk, np.asarray(fill, dt)), cls[0]
        assert nd.all_equal(None) is False


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("sharded", [False, True], ids=["plain", "sharded"])
def test_complex128_is_refused_before_any_reservation(device, sharded):
    """A complex128 write and read through the drop-in boundary
    (HipCodecPipeline.write_sync / read_sync over a DeviceStore that already
    holds an array) raise the named error and leave the store's keys and the
    arena's used bytes as they were; so does Array.create, before zarr.json."""
    import torch

    import zarr_hip
    from zarr_hip import HipCodecPipeline, UnsupportedDTypeError

    store = zarr_hip.DeviceStore(device)
    keep = zarr_hip.Array.create(store, (32, 32), (16, 16), "float32", 0.0, codecs=[D.LE, D.CRC], path="keep")
    keep[...] = D.sample((32, 32), "float32")
    keys, used = sorted(store.keys()), store.arena.used_bytes
    assert keys and used > 0

    def unchanged():
        return sorted(store.keys()) == keys and store.arena.used_bytes == used and \
            store.get_sync("c16/zarr.json") is None

    shape, chunks, dt = (32, 32), (16, 16), np.dtype("complex128")
    codecs = [D.SHARD((8, 8), [D.LE, D.CRC])] if sharded else [D.LE, D.CRC]
    spec = Z.ArraySpec(chunks, Z.ZDType(dt), dt.type(0), Z.ArrayConfig(), Z.cpu_prototype)
    pipe = HipCodecPipeline.from_codecs(Z.zcodecs(codecs)).evolve_from_array_spec(spec)
    value = np.ones(shape, dt)
    for sel in [(Ellipsis,), (slice(3, 30), slice(5, 20))]:  # whole chunks, then merges
        batch, out_shape = Z.batch_for(shape, chunks, sel, store, spec)
        with pytest.raises(UnsupportedDTypeError, match="complex128"):
            pipe.write_sync(batch, Z.NDBuffer(value[:out_shape[0], :out_shape[1]]))
        assert unchanged()
        with pytest.raises(UnsupportedDTypeError, match="complex128"):
            pipe.write_sync(batch, torch.ones(out_shape, dtype=torch.complex128, device=device))
        assert unchanged()
        with pytest.raises(UnsupportedDTypeError, match="complex128"):
            pipe.read_sync(batch, Z.NDBuffer.create(shape=out_shape, dtype=dt))
        with pytest.raises(UnsupportedDTypeError, match="complex128"):
            pipe.read_sync(batch, torch.empty(out_shape, dtype=torch.complex128, device=device))
        assert unchanged()
    with pytest.raises(UnsupportedDTypeError, match="complex128"):
        zarr_hip.Array.create(store, shape, chunks, dt, 0.0, codecs=codecs, path="c16")
    assert unchanged()
    assert _bits(keep[...]) == _bits(D.sample((32, 32), "float32"))
