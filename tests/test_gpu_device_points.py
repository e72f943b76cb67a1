"""Coordinate and mask selections whose indices are device tensors
(zarr_hip.points: planned on the GPU by k_points_count / k_points_fill), end
to end through Array: byte-equal to numpy fancy indexing of the host mirror
and to the same call with the indices as numpy (the host-planned route);
written stores against the CPU oracle as test_gpu_fancy_selection.py checks
them."""

import numpy as np
import pytest

from test_gpu_fancy_selection import Fixture, _check_written, _read_fixture, _same, _vindex_cases

pytestmark = pytest.mark.gpu

READ_GEOMS = ["u1", "f8", "f4be", "shard-end", "shard-start", "1d", "4d", "transpose", "gzip", "nested"]


def _dev(sel, device):
    """The selection with every numpy array as a device tensor."""
    import torch

    if isinstance(sel, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(sel)).to(device)
    return tuple(_dev(s, device) if isinstance(s, np.ndarray) else s for s in sel)


def _host(t, f):
    import torch

    from zarr_hip import buffer

    assert isinstance(t, torch.Tensor) and t.is_cuda
    return buffer.to_numpy(t, f.mirror.dtype)


@pytest.mark.parametrize("gid", READ_GEOMS)
def test_device_index_reads_match_numpy_and_the_host_route(gid, device):
    f = _read_fixture(gid, device)
    rng = np.random.default_rng(2)
    for name, sel in _vindex_cases(f.shape, rng).items():
        dsel = _dev(sel, device)
        want = f.mirror[sel]
        if name == "mask":
            got = f.arr.get_mask_selection(dsel)
            assert _same(f.arr.get_mask_selection(sel), want), (gid, name)
        else:
            got = f.arr.get_coordinate_selection(dsel)
            assert _same(f.arr.get_coordinate_selection(sel), want), (gid, name)
        assert _same(_host(got, f), want), (gid, name)
        assert _same(_host(f.arr.vindex[dsel], f), want), (gid, name, "vindex")
        assert _same(_host(f.arr.get(dsel), f), want), (gid, name, "get")
        h = f.arr[dsel]
        assert isinstance(h, np.ndarray) and _same(h, want), (gid, name, "getitem")


@pytest.mark.parametrize("gid", ["f4be", "shard-start"])
def test_index_forms(gid, device):
    import torch

    from zarr_hip import _native as N

    f = _read_fixture(gid, device)
    m, shape = f.mirror, f.shape
    rng = np.random.default_rng(3)
    a = rng.integers(-shape[0], shape[0], (5, 1))
    b = rng.integers(-shape[1], shape[1], (1, 7))
    got = f.arr.vindex[_dev(a, device), _dev(b, device), 3]          # broadcast shapes, a Python integer
    assert _same(_host(got, f), m[a, b, 3])
    got = f.arr.vindex[-1, _dev(b.reshape(-1), device), -2]
    assert _same(_host(got, f), m[-1, b.reshape(-1), -2])
    pts = tuple(rng.integers(-s, s, 50) for s in shape)
    mixed = (torch.from_numpy(pts[0].astype(np.int32)).to(device), _dev(pts[1], device),
             torch.from_numpy(pts[2].astype(np.int16)).to(device))  # int32 / int64 / int16 tensors
    assert _same(_host(f.arr.get_coordinate_selection(mixed), f), m[pts])
    assert N.lib().zhip_last_kernel() == b"k_select_copy"
    dup = tuple(np.repeat(rng.integers(0, s, 5), 30) for s in shape)  # duplicates
    assert _same(_host(f.arr.vindex[_dev(dup, device)], f), m[dup])
    order = np.lexsort(pts[::-1])
    srt = tuple(np.where(p < 0, p + s, p)[order] for p, s in zip(pts, shape))  # sorted by chunk already
    assert _same(_host(f.arr.vindex[_dev(srt, device)], f), m[srt])
    # points only in chunks that were never written: the fill value
    miss = (np.array([shape[0] - 1, shape[0] - 2, -1]), np.array([0, shape[1] - 1, 5]), np.array([1, 2, shape[2] - 1]))
    got = _host(f.arr.vindex[_dev(miss, device)], f)
    assert _same(got, m[miss]) and (got == f.meta.fill_value).all()
    for mask in (np.zeros(shape, bool), np.ones(shape, bool)):        # all-false and all-true masks
        got = f.arr.get_mask_selection(_dev(mask, device))
        assert _same(_host(got, f), m[mask])
    empty = tuple(torch.zeros(0, dtype=torch.int64, device=device) for _ in shape)  # n = 0
    got = f.arr.get_coordinate_selection(empty)
    assert got.is_cuda and tuple(got.shape) == (0,)


def test_out_targets(device):
    import torch

    from zarr_hip import buffer

    f = _read_fixture("f4be", device)
    pts = tuple(np.random.default_rng(4).integers(0, s, 33) for s in f.shape)
    dpts = _dev(pts, device)
    want = f.mirror[pts]
    out = torch.full((33,), -1.0, dtype=torch.float32, device=device)
    assert f.arr.get_coordinate_selection(dpts, out=out) is out
    assert _same(buffer.to_numpy(out, np.float32), want)
    big = torch.full((70,), -5.0, dtype=torch.float32, device=device)
    f.arr.get_coordinate_selection(dpts, out=big[2:68:2])           # a strided view: decoded in place
    exp = np.full(70, -5.0, np.float32)
    exp[2:68:2] = want
    assert _same(buffer.to_numpy(big, np.float32), exp)
    hv = np.full(40, -1.0, np.float32)
    f.arr.get_coordinate_selection(dpts, out=hv[3:36])               # a host out
    assert _same(hv[3:36], want) and hv[:3].tolist() == [-1.0] * 3 and hv[36:].tolist() == [-1.0] * 4
    with pytest.raises(ValueError, match="elements"):
        f.arr.get_coordinate_selection(dpts, out=torch.zeros(34, dtype=torch.float32, device=device))


@pytest.mark.parametrize("gid", ["u2", "shard-end"])
def test_sub_batches_and_a_corrupt_chunk(gid, device, monkeypatch):
    from zarr_hip import fancy

    f = Fixture(gid, device)
    cshape = f.meta.chunk_shape
    monkeypatch.setattr(fancy, "FANCY_SCRATCH_BYTES", 2 * int(np.prod(cshape)) * f.mirror.dtype.itemsize)
    rng = np.random.default_rng(11)
    pts = tuple(rng.integers(0, s, 300) for s in f.shape)
    assert len({tuple(int(p[i]) // c for p, c in zip(pts, cshape)) for i in range(300)}) >= 7
    assert _same(_host(f.arr.vindex[_dev(pts, device)], f), f.mirror[pts])
    mask = rng.random(f.shape) < 0.01
    assert _same(_host(f.arr.vindex[_dev(mask, device)], f), f.mirror[mask])
    bad = Fixture(gid, device, corrupt="c/0/0/0")                    # the first touched chunk: the first sub-batch
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.vindex[_dev(pts, device)]
    value = np.asarray(77, f.mirror.dtype)[()]
    f.arr.vindex[_dev(pts, device)] = value
    f.mirror[pts] = value
    _check_written(f)
    before = bad.chunk_dict()
    first = tuple(np.array([1, 2]) for _ in f.shape)                 # the corrupt chunk only
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.vindex[_dev(first, device)] = value
    assert bad.chunk_dict() == before


def test_errors(device):
    import torch

    from zarr_hip import _native as N

    f = _read_fixture("u1", device)
    ok = tuple(np.array([0, 1, 2]) for _ in f.shape)
    assert _same(_host(f.arr.vindex[_dev(ok, device)], f), f.mirror[ok])
    oob = (np.array([0, 49, 3]), np.array([0, 37, 36]), np.array([28, 29, -30]))  # dimensions 1 and 2 fail
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 37"):
        f.arr.get_coordinate_selection(_dev(oob, device))
    assert N.lib().zhip_last_kernel() == b"k_points_count"           # nothing further was launched
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 37"):
        f.arr.get_coordinate_selection(oob)                           # the host route's message
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 50"):
        f.arr.vindex[_dev((np.array([-51]), np.array([0]), np.array([0])), device)] = 1
    d = _dev(ok, device)
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr.vindex[d[0], torch.from_numpy(ok[1]), d[2]]            # a host tensor among device tensors
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr.get_coordinate_selection((d[0], ok[1], d[2]))           # a numpy array among them
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr[d[0], [0, 1, 2], d[2]]
    with pytest.raises(IndexError, match="invalid mask selection"):
        f.arr.get_mask_selection(torch.zeros((50, 37), dtype=torch.bool, device=device))
    with pytest.raises(IndexError, match="invalid mask selection"):
        f.arr.get_mask_selection(torch.zeros(f.shape, dtype=torch.uint8, device=device))
    with pytest.raises(IndexError, match="invalid coordinate selection"):
        f.arr.get_coordinate_selection((d[0], d[1]))
    with pytest.raises(IndexError, match="invalid coordinate selection"):
        f.arr.get_coordinate_selection((d[0], d[1], d[2].to(torch.float32)))
    with pytest.raises(ValueError, match="device"):
        f.arr.get(d, device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="prepare_read"):
        f.arr.prepare_read(d)


def test_missing_chunks_raise_when_the_array_says_so(device):
    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    f = _read_fixture("u1", device)
    strict = zarr_hip.Array.open(f.store, config=ArrayConfig(read_missing_chunks=False))
    present = tuple(np.array([0, 1]) for _ in f.shape)
    assert _same(_host(strict.vindex[_dev(present, device)], f), f.mirror[present])
    with pytest.raises(zarr_hip.ChunkNotFoundError):
        strict.vindex[_dev(tuple(np.array([s - 1]) for s in f.shape), device)]


def test_past_a_limit_the_host_route_serves_a_host_copy(device, monkeypatch):
    from zarr_hip import points

    f = _read_fixture("u1", device)
    pts = tuple(np.random.default_rng(5).integers(0, s, 40) for s in f.shape)
    monkeypatch.setattr(points, "MAX_GRID", 4)  # the fixture's grid has 4 x 3 x 2 chunks
    with pytest.raises(points.PointsLimit):
        points.DeviceCoordinateIndexer(_dev(pts, device), f.shape, (16, 16, 16))
    got = f.arr.get_coordinate_selection(_dev(pts, device))
    assert _same(_host(got, f), f.mirror[pts])
    mask = f.mirror > 150
    assert _same(_host(f.arr.get_mask_selection(_dev(mask, device)), f), f.mirror[mask])


@pytest.mark.parametrize("gid", ["u2", "shard-end", "nested"])
def test_device_index_writes_match_numpy_and_the_oracle(gid, device):
    import torch

    f = Fixture(gid, device)
    initial = set(f.chunk_dict())
    rng = np.random.default_rng(7)
    dt = f.mirror.dtype
    rep = tuple(rng.integers(-s, s, 6) for s in f.shape)
    dup = tuple(np.concatenate([c, c[::-1], c]) for c in rep)        # a scalar through duplicated coordinates
    f.arr.vindex[_dev(dup, device)] = dt.type(251)
    f.mirror[dup] = 251
    pts = tuple(rng.integers(0, s, 200) for s in f.shape)
    f.arr.set_coordinate_selection(_dev(pts, device), np.asarray(252, dt))
    f.mirror[pts] = 252
    mask = rng.random(f.shape) < 0.03
    f.arr.set_mask_selection(_dev(mask, device), dt.type(253))       # a scalar through a mask
    f.mirror[mask] = 253
    mask = rng.random(f.shape) < 0.03
    value = rng.integers(300, 9000, int(mask.sum())).astype(dt)
    f.arr.vindex[_dev(mask, device)] = value                          # an array value through a mask
    f.mirror[mask] = value
    mask = rng.random(f.shape) < 0.03
    value = rng.integers(300, 9000, int(mask.sum())).astype(dt)
    # __setitem__; a device value where torch holds the dtype as it is
    f.arr[_dev(mask, device)] = value if dt == np.uint16 else torch.from_numpy(value).to(device)
    f.mirror[mask] = value
    _check_written(f)
    # a chunk that becomes all fill is gone; a missing chunk that gets a value exists
    first = np.zeros(f.shape, bool)
    first[tuple(slice(0, c) for c in f.meta.chunk_shape)] = True
    f.arr.vindex[_dev(first, device)] = f.meta.fill_value
    f.mirror[first] = f.meta.fill_value
    last = tuple(np.array([s - 1]) for s in f.shape)
    f.arr.vindex[_dev(last, device)] = dt.type(99)
    f.mirror[last] = 99
    after = set(f.chunk_dict())
    assert initial - after and after - initial, (initial, after)
    _check_written(f)
    # an array value through device coordinates: refused by name, nothing stored
    before = f.chunk_dict()
    with pytest.raises(NotImplementedError, match="keep-last"):
        f.arr.vindex[_dev(pts, device)] = np.arange(200).astype(dt)
    with pytest.raises(ValueError):
        f.arr.vindex[_dev(mask, device)] = np.arange(3).astype(dt)
    assert f.chunk_dict() == before
