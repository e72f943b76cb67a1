"""Orthogonal, coordinate and mask selections on the GPU: Array.oindex /
vindex / __getitem__ dispatch and hand-written batches through
HipCodecPipeline.read_sync / write_sync, bit-exact against numpy fancy
indexing of a host mirror; written stores against the CPU oracle (key set,
every CRC and shard index)."""

import numpy as np
import pytest

from oracle import oracle as O
from test_fancy_selection import _np_oindex

pytestmark = pytest.mark.gpu

LE = {"name": "bytes", "configuration": {"endian": "little"}}
BE = {"name": "bytes", "configuration": {"endian": "big"}}
B1 = {"name": "bytes"}
CRC = {"name": "crc32c"}
GZIP = {"name": "gzip", "configuration": {"level": 1}}


def _T(order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def _NEST(outer, inner, codecs):
    return {"name": "sharding_indexed", "configuration": {
        "chunk_shape": list(outer), "index_location": "end",
        "codecs": [{"name": "sharding_indexed", "configuration": {
            "chunk_shape": list(inner), "codecs": list(codecs)}}]}}


# id -> (shape, chunks, shards | None, index_location, dtype, fill, codecs, store kind)
GEOMS = {
    "u1": ((50, 37, 29), (16, 16, 16), None, "end", "uint8", 7, [B1, CRC], "device"),
    "u2": ((50, 37, 29), (16, 16, 16), None, "end", "uint16", 7, [LE, CRC], "device"),
    "f4be": ((50, 37, 29), (16, 16, 16), None, "end", "float32", 1.5, [BE, CRC], "device"),
    "f8": ((50, 37, 29), (16, 16, 16), None, "end", "float64", -2.25, [LE, CRC], "device"),
    "shard-end": ((40, 36, 33), (16, 16, 16), (32, 32, 32), "end", "float32", 3.0, [LE, CRC], "device"),
    "shard-start": ((40, 36, 33), (16, 16, 16), (32, 32, 32), "start", "uint16", 9, [LE, CRC], "device"),
    "1d": ((1000,), (64,), None, "end", "uint16", 5, [LE, CRC], "device"),
    "4d": ((9, 10, 11, 12), (4, 4, 4, 4), None, "end", "float32", 0.5, [LE, CRC], "device"),
    "transpose": ((20, 19, 18), (8, 8, 8), None, "end", "float32", 2.0, [_T((2, 0, 1)), LE, CRC], "device"),
    "gzip": ((30, 21), (8, 8), None, "end", "float32", 4.0, [LE, GZIP], "memory"),
    "nested": ((70, 36), (20, 20), None, "end", "int32", -1, [_NEST((10, 10), (5, 5), [LE, CRC])], "memory"),
}


class Fixture:
    def __init__(self, gid, device, corrupt=None):
        import zarr_hip

        shape, chunks, shards, loc, dtype, fill, codecs, kind = GEOMS[gid]
        self.gid, self.shape, self.kind, self.device = gid, shape, kind, device
        dt = np.dtype(dtype)
        if shards is None:
            self.meta = O.ArrayMeta(shape, chunks, dt, fill, codecs=list(codecs))
        else:
            self.meta = O.ArrayMeta(shape, shards, dt, fill, codecs=[{"name": "sharding_indexed", "configuration": {
                "chunk_shape": list(chunks), "codecs": list(codecs), "index_codecs": [LE, CRC],
                "index_location": loc}}])
        rng = np.random.default_rng(sum(map(ord, gid)))
        self.mirror = np.full(shape, fill, dt)
        # the leading ~3/4 of every dimension is written: trailing chunks stay missing,
        # the chunks the edge of the region cuts are part data, part fill
        region = tuple(slice(0, max(1, (3 * n) // 4)) for n in shape)
        rshape = self.mirror[region].shape
        data = (rng.random(rshape) * 200).astype(dt) if dt.kind == "f" else \
            rng.integers(0, 200, rshape).astype(dt)
        self.mirror[region] = data
        host: dict = {}
        O.write(host, self.meta, region, data)
        if corrupt is not None:
            raw = bytearray(host[corrupt])
            raw[5] ^= 0x40
            host[corrupt] = bytes(raw)
        self.store = zarr_hip.DeviceStore.from_host(host, device) if kind == "device" else \
            zarr_hip.MemoryStore(dict(host))
        if shards is None:
            self.arr = zarr_hip.Array.create(self.store, shape, chunks, dtype, fill, codecs=list(codecs))
        else:
            self.arr = zarr_hip.Array.create(self.store, shape, chunks, dtype, fill, codecs=list(codecs),
                                             shards=shards, index_location=loc)

    def chunk_dict(self) -> dict:
        return {k: bytes(v) for k, v in self.store.to_dict().items() if not k.endswith("zarr.json")}


_READ: dict = {}


def _read_fixture(gid, device) -> Fixture:
    """One store and mirror per geometry, shared by the read tests (never written)."""
    if gid not in _READ:
        _READ[gid] = Fixture(gid, device)
    return _READ[gid]


def _same(got, want) -> bool:
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _oindex_cases(shape, rng) -> dict:
    nd = len(shape)
    full = [slice(None)] * nd

    def srt(d, k=9):
        return np.sort(rng.choice(shape[d], min(k, shape[d]), replace=False))

    def uns(d, k=11):
        return rng.integers(-shape[d], shape[d], k)  # unsorted, repeated, negative

    cases = {}
    s = list(full)
    s[-1] = srt(nd - 1)
    cases["one-array-bare"] = tuple(s)
    mask = rng.random(shape[0]) < 0.5
    mask[-1] = True  # the mask's length ends in a boundary chunk, and selects there
    s = list(full)
    s[0] = mask
    cases["mask-bare"] = tuple(s)
    s = list(full)
    s[0] = uns(0)
    cases["unsorted-repeated-bare"] = tuple(s)
    s = list(full)
    s[0] = srt(0)[::-1].copy()
    cases["decreasing-bare"] = tuple(s)
    if nd >= 2:
        s = list(full)
        s[0], s[-1] = srt(0), srt(nd - 1)
        cases["two-arrays-mesh"] = tuple(s)
        s = list(full)
        s[0], s[-1] = uns(0), uns(nd - 1)
        cases["two-unsorted-mesh-out-mesh"] = tuple(s)
        s = [srt(d, 5) for d in range(nd)]
        s[0] = int(shape[0] // 2)
        cases["int-with-arrays-drop-axes"] = tuple(s)
        s = list(full)
        s[0], s[1] = -1, [0, shape[1] - 1, 1]
        cases["int-list-slices"] = tuple(s)
    if nd >= 3:
        cases["three-arrays-mesh"] = tuple([srt(0), uns(1, 6), rng.random(shape[2]) < 0.4] + full[3:])
    return cases


def _vindex_cases(shape, rng) -> dict:
    n = 40
    srt = np.sort(rng.choice(int(np.prod(shape)), n, replace=False))
    cases = {"sorted": np.unravel_index(srt, shape)}
    cases["unsorted"] = tuple(rng.integers(0, s, n) for s in shape)
    rep = tuple(rng.integers(0, s, 6) for s in shape)
    cases["repeated"] = tuple(np.concatenate([c, c[::-1], c]) for c in rep)
    cases["negative"] = tuple(rng.integers(-s, s, n) for s in shape)
    cases["2d-coordinate-arrays"] = tuple(rng.integers(0, s, (4, 7)) for s in shape)
    cases["mask"] = rng.random(shape) < 0.02
    return cases


READ_GEOMS = list(GEOMS)


@pytest.mark.parametrize("gid", READ_GEOMS)
def test_oindex_reads_match_numpy(gid, device):
    f = _read_fixture(gid, device)
    rng = np.random.default_rng(1)
    for name, sel in _oindex_cases(f.shape, rng).items():
        got = f.arr.oindex[sel]
        assert _same(got, _np_oindex(f.mirror, list(sel))), (gid, name)


@pytest.mark.parametrize("gid", READ_GEOMS)
def test_vindex_reads_match_numpy(gid, device):
    f = _read_fixture(gid, device)
    rng = np.random.default_rng(2)
    for name, sel in _vindex_cases(f.shape, rng).items():
        got = f.arr.vindex[sel]
        assert _same(got, f.mirror[sel]), (gid, name)


def test_getitem_dispatch_and_device_get(device):
    import torch

    from zarr_hip import _native as N
    from zarr_hip import buffer

    f = _read_fixture("u2", device)
    g = _read_fixture("1d", device)
    idx = np.array([999, 3, 3, 64, 500, -2])
    assert _same(g.arr[idx], g.mirror[idx])                      # arr[np.array([...])]
    assert _same(g.arr[[5, 1, 700]], g.mirror[[5, 1, 700]])
    m1 = g.mirror % 3 == 0
    assert _same(g.arr[m1], g.mirror[m1])
    mask = f.mirror > 150
    assert _same(f.arr[mask], f.mirror[mask])                    # arr[mask]
    pts = (np.array([0, 49, 17]), np.array([36, 0, 16]), np.array([28, 15, 16]))
    assert _same(f.arr[pts], f.mirror[pts])
    osel = (np.array([40, 2, 2]), slice(5, 30, 3), 7)
    assert _same(f.arr[osel], _np_oindex(f.mirror, list(osel)))
    t = f.arr.get(osel)                                          # get() keeps returning a device tensor
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert N.lib().zhip_last_kernel() == b"k_select_copy"
    assert _same(buffer.to_numpy(t, f.mirror.dtype), _np_oindex(f.mirror, list(osel)))
    t = f.arr.get(pts)
    assert t.is_cuda and _same(buffer.to_numpy(t, f.mirror.dtype), f.mirror[pts])
    with pytest.raises(NotImplementedError, match="prepare_read"):
        f.arr.prepare_read(osel)
    with pytest.raises(IndexError):
        f.arr.oindex[np.array([50]), :, :]
    with pytest.raises(IndexError):
        f.arr.vindex[np.array([0]), np.array([37]), np.array([0])]


def test_output_targets(device):
    import torch

    from zarr_hip import buffer

    f = _read_fixture("f4be", device)
    sel = (np.array([44, 3, 3, 20]), slice(None), np.array([28, 0, 15, 16, 1]))
    want = _np_oindex(f.mirror, list(sel))
    dev = torch.full(want.shape, -1.0, dtype=torch.float32, device=device)
    f.arr.get_orthogonal_selection(sel, out=dev)                 # a device out
    assert _same(buffer.to_numpy(dev, np.float32), want)
    host = np.full(want.shape, -1.0, np.float32)
    f.arr.get_orthogonal_selection(sel, out=host)                # a host numpy out
    assert _same(host, want)
    fo = buffer.empty(want.shape, np.float32, device, "F")       # an F-order out
    assert not fo.is_contiguous()
    f.arr.get_orthogonal_selection(sel, out=fo)
    assert _same(buffer.to_numpy(fo, np.float32), want)
    big = torch.full((want.shape[0], want.shape[1] * 2, want.shape[2] + 3), -5.0, dtype=torch.float32, device=device)
    view = big[:, ::2, 2:-1]                                     # a strided view out
    f.arr.get_orthogonal_selection(sel, out=view)
    exp = np.full(tuple(big.shape), -5.0, np.float32)
    exp[:, ::2, 2:-1] = want
    assert _same(buffer.to_numpy(big, np.float32), exp)          # untouched elements unchanged
    pts = tuple(np.random.default_rng(4).integers(0, s, 33) for s in f.shape)
    hv = np.full(40, -1.0, np.float32)
    f.arr.get_coordinate_selection(pts, out=hv[3:36])
    assert _same(hv[3:36], f.mirror[pts]) and hv[:3].tolist() == [-1.0] * 3 and hv[36:].tolist() == [-1.0] * 4


def test_hand_written_batches_in_the_reference_forms(device):
    """chunk_selection / out_selection exactly as the reference's indexers
    emit them, straight into HipCodecPipeline.read_sync: a mesh with
    drop_axes, the bare one-array form, a point list with a bare slice and
    with a bare array, next to a basic item in the same batch."""
    import torch

    from zarr_hip import buffer
    from zarr_hip.store import StorePath

    f = _read_fixture("u2", device)
    pipe, spec = f.arr.codec_pipeline, f.arr.spec
    m = f.mirror

    def sp(*co):
        return StorePath(f.store, "c/" + "/".join(map(str, co)))

    out = torch.zeros((3, 2), dtype=torch.uint16, device=device)
    res = pipe.read_sync([(sp(1, 0, 1), spec, np.ix_([3], [1, 5, 9], [0, 2]), (slice(0, 3), slice(0, 2)), False)],
                         out, drop_axes=(0,))
    assert res[0]["status"] == "present"
    assert _same(buffer.to_numpy(out, np.uint16), m[16 + 3, [1, 5, 9]][:, [16, 18]])
    out = torch.zeros((3, 2), dtype=torch.uint16, device=device)
    pipe.read_sync([(sp(1, 0, 1), spec, np.ix_([3], [1, 5, 9], [0, 2]), np.ix_([2, 0, 1], [1, 0]), False)],
                   out, drop_axes=(0,))
    want = np.zeros((3, 2), np.uint16)
    want[np.ix_([2, 0, 1], [1, 0])] = m[16 + 3, [1, 5, 9]][:, [16, 18]]
    assert _same(buffer.to_numpy(out, np.uint16), want)
    # bare form + a basic item + a missing chunk, one batch
    out = torch.zeros((16, 7, 16), dtype=torch.uint16, device=device)
    keep = np.zeros(16, bool)
    keep[[0, 4, 15]] = True
    res = pipe.read_sync([
        (sp(0, 1, 0), spec, (slice(0, 16), np.array([15, 2, 2]), slice(0, 16)), (slice(0, 16), np.array([2, 0, 1]), slice(0, 16)), False),
        (sp(2, 1, 1), spec, (slice(0, 16), slice(0, 1), slice(0, 13)), (slice(0, 16), slice(3, 4), slice(0, 13)), False),
        (sp(3, 2, 1), spec, (slice(0, 2), keep, slice(0, 13)), (slice(0, 2), slice(4, 7), slice(2, 15)), False),
    ], out)
    assert [r["status"] for r in res] == ["present", "present", "missing"]
    want = np.zeros((16, 7, 16), np.uint16)
    want[:, [2, 0, 1], :] = m[0:16, [31, 18, 18], 0:16]
    want[:, 3:4, 0:13] = m[32:48, 16:17, 16:29]
    want[0:2, 4:7, 2:15] = 7  # the fill value
    assert _same(buffer.to_numpy(out, np.uint16), want)
    # point lists: out as a bare slice, and as a bare array
    r, c, d = np.array([0, 5, 5, 15]), np.array([1, 0, 0, 15]), np.array([9, 9, 9, 3])
    out = torch.zeros(10, dtype=torch.uint16, device=device)
    pipe.read_sync([(sp(0, 0, 0), spec, (r, c, d), slice(2, 6), False),
                    (sp(1, 1, 0), spec, (r, c, d), np.array([9, 0, 7, 6]), False)], out)
    want = np.zeros(10, np.uint16)
    want[2:6] = m[r, c, d]
    want[[9, 0, 7, 6]] = m[16 + r, 16 + c, d]
    assert _same(buffer.to_numpy(out, np.uint16), want)
    # refused by name; out-of-range tables never reach the device
    with pytest.raises(NotImplementedError, match="pointwise arrays mixed with slices"):
        pipe.read_sync([(sp(0, 0, 0), spec, (r, c, slice(0, 16)), (slice(0, 4), slice(0, 16)), False)],
                       torch.zeros((4, 16), dtype=torch.uint16, device=device))
    with pytest.raises(IndexError):
        pipe.read_sync([(sp(0, 0, 0), spec, (r, c, d + 13), slice(0, 4), False)], out)
    with pytest.raises(IndexError):
        pipe.read_sync([(sp(0, 0, 0), spec, (r, c, d), np.array([0, 1, 2, 10]), False)], out)


def _check_written(f: Fixture):
    got = f.arr[...]
    assert _same(got, f.mirror), f.gid                                  # (a)
    full: dict = {}
    O.write(full, f.meta, (Ellipsis,), f.mirror)
    stored = f.chunk_dict()
    assert sorted(stored) == sorted(full), f.gid                        # (b) same key set as a full oracle write
    assert _same(O.read(stored, f.meta), f.mirror), f.gid               # (c) every CRC / shard index decodes


def _np_oindex_set(a, sel, value):
    sel = [np.asarray(s) if isinstance(s, list) else s for s in sel]
    sel += [slice(None)] * (a.ndim - len(sel))
    drop = [i for i, s in enumerate(sel) if isinstance(s, (int, np.integer))]
    mesh = np.ix_(*[np.arange(n)[s] if isinstance(s, slice) else [s] if isinstance(s, (int, np.integer))
                    else (np.nonzero(s)[0] if s.dtype == bool else s) for s, n in zip(sel, a.shape)])
    v = np.asarray(value)
    if v.ndim and drop:
        v = np.expand_dims(v, drop)
    a[mesh] = v


WRITE_GEOMS = ["u1", "f4be", "f8", "shard-end", "shard-start", "1d", "4d", "transpose", "gzip", "nested"]


@pytest.mark.parametrize("gid", WRITE_GEOMS)
def test_writes_match_numpy_and_the_oracle(gid, device):
    import torch

    f = Fixture(gid, device)
    initial = set(f.chunk_dict())
    rng = np.random.default_rng(7)
    dt = f.mirror.dtype
    for name, sel in _oindex_cases(f.shape, rng).items():
        shape = _np_oindex(f.mirror, list(sel)).shape
        value = (rng.random(shape) * 100 + 300).astype(dt) if dt.kind == "f" else rng.integers(200, 250, shape).astype(dt)
        dup = any(isinstance(s, np.ndarray) and s.dtype != bool and len(np.unique(s % n)) != len(s)
                  for s, n in zip(sel, f.shape))
        if dup or name.startswith("int-list"):
            value = value.reshape(-1)[0]  # duplicates: equal values only (a scalar value)
        elif name == "two-arrays-mesh" and dt.kind == "f":
            value = torch.from_numpy(value.astype(dt.newbyteorder("="))).to(device)  # a device value
        f.arr.oindex[sel] = value
        _np_oindex_set(f.mirror, sel, value.cpu().numpy() if isinstance(value, torch.Tensor) else value)
    for name, sel in _vindex_cases(f.shape, rng).items():
        n = f.mirror[sel].size
        if name in ("repeated", "negative", "unsorted", "2d-coordinate-arrays"):
            value = dt.type(251 if name == "repeated" else 252)  # possible duplicates: equal values
        else:
            value = (rng.random(n) * 100 + 500).astype(dt) if dt.kind == "f" else rng.integers(100, 255, n).astype(dt)
        f.arr.vindex[sel] = value
        f.mirror[sel] = value
    _check_written(f)
    # a chunk that becomes all fill is gone; a missing chunk that gets a value exists
    fill = f.meta.fill_value
    first = tuple(np.arange(min(c, n)) for c, n in zip(f.meta.chunk_shape, f.shape))
    if len(first) > 1:
        f.arr.oindex[first] = fill
        _np_oindex_set(f.mirror, first, fill)
    else:
        f.arr[first[0]] = fill
        f.mirror[first[0]] = fill
    last = tuple(np.array([n - 1]) for n in f.shape)
    f.arr.vindex[last] = dt.type(99)
    f.mirror[last] = 99
    after = set(f.chunk_dict())
    assert initial - after and after - initial, (initial, after)
    _check_written(f)


def test_setitem_dispatch_and_mask_write(device):
    f = Fixture("u2", device)
    mask = f.mirror > 150
    f.arr[mask] = np.uint16(1)
    f.mirror[mask] = 1
    idx = (np.array([49, 0, 17]), np.array([0, 36, 5]), np.array([28, 28, 0]))
    f.arr[idx] = np.array([1000, 2000, 3000], np.uint16)
    f.mirror[idx] = [1000, 2000, 3000]
    f.arr[[3, 40], 2:30:5, -1] = np.arange(12, dtype=np.uint16).reshape(2, 6) + 400
    f.mirror[[3, 40], 2:30:5, -1] = np.arange(12, dtype=np.uint16).reshape(2, 6) + 400
    _check_written(f)
    with pytest.raises(ValueError):
        f.arr.vindex[idx] = np.arange(4, dtype=np.uint16)


@pytest.mark.parametrize("gid,key", [("u2", "c/1/0/0"), ("shard-end", "c/0/0/0")])
def test_write_onto_a_corrupt_chunk_raises_and_stores_nothing(gid, key, device):
    f = Fixture(gid, device, corrupt=key)
    before = f.chunk_dict()
    pts = tuple(np.array([17 if gid == "u2" else 1, 40 if gid == "u2" else 33]) if d == 0 else np.array([2, 3])
                for d in range(3))  # the first point's chunk is the corrupt one, the second's is sound
    with pytest.raises(ValueError, match="checksum"):
        f.arr.vindex[pts] = np.array([1, 2], f.mirror.dtype)
    assert f.chunk_dict() == before


@pytest.mark.parametrize("gid", ["u2", "shard-end"])
def test_scratch_budget_sub_batches(gid, device, monkeypatch):
    from zarr_hip import fancy

    f = Fixture(gid, device)
    cshape = f.meta.chunk_shape
    monkeypatch.setattr(fancy, "FANCY_SCRATCH_BYTES", 2 * int(np.prod(cshape)) * f.mirror.dtype.itemsize)
    rng = np.random.default_rng(11)
    sel = (rng.permutation(f.shape[0])[:30], slice(None), rng.integers(0, f.shape[2], 9))
    nchunks = len({(a // cshape[0], c // cshape[2]) for a in sel[0] for c in sel[2]}) * -(-f.shape[1] // cshape[1])
    assert nchunks >= 7 or gid != "u2"
    assert _same(f.arr.oindex[sel], _np_oindex(f.mirror, list(sel)))
    pts = tuple(rng.integers(0, s, 300) for s in f.shape)
    assert _same(f.arr.vindex[pts], f.mirror[pts])
    value = np.asarray(77, f.mirror.dtype)[()]
    f.arr.oindex[sel] = value
    _np_oindex_set(f.mirror, sel, value)
    f.arr.vindex[pts] = value
    f.mirror[pts] = value
    _check_written(f)
