"""Orthogonal selections whose index arrays are device tensors (zarr_hip.axes:
planned on the GPU by k_axis_last / k_axis_count / k_axis_fill), end to end
through Array: byte-equal to numpy indexing of the host mirror and to the same
call with the indices as numpy (the host-planned route); written stores
against the CPU oracle as test_gpu_fancy_selection.py checks them.  Array
values are written through REPEATED indices, on one axis and on two at once:
the last occurrence along each axis wins, as in numpy."""

import numpy as np
import pytest

from test_gpu_fancy_selection import (Fixture, _check_written, _np_oindex, _np_oindex_set, _oindex_cases,
                                      _read_fixture, _same)

pytestmark = pytest.mark.gpu

READ_GEOMS = ["u1", "f8", "f4be", "shard-end", "shard-start", "1d", "4d", "transpose", "gzip", "nested"]
WRITE_GEOMS = READ_GEOMS


def _dev(sel, device):
    """The selection with every numpy array and list as a device tensor."""
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(s))).to(device)
                 if isinstance(s, (np.ndarray, list)) else s for s in sel)


def _host(t, f):
    import torch

    from zarr_hip import buffer

    assert isinstance(t, torch.Tensor) and t.is_cuda
    return buffer.to_numpy(t, f.mirror.dtype)


def _getitem_is_orthogonal(sel, nd) -> bool:
    """zarr's dispatch order for arr[sel]: pure fancy first, then pure orthogonal."""
    from zarr_hip.indexing import is_pure_fancy_indexing, is_pure_orthogonal_indexing

    return not is_pure_fancy_indexing(sel, nd) and is_pure_orthogonal_indexing(sel, nd)


@pytest.mark.parametrize("gid", READ_GEOMS)
def test_device_index_reads_match_numpy_and_the_host_route(gid, device):
    import torch

    from zarr_hip import _native as N

    f = _read_fixture(gid, device)
    rng = np.random.default_rng(1)
    nd = len(f.shape)
    for name, sel in _oindex_cases(f.shape, rng).items():
        dsel = _dev(sel, device)
        want = _np_oindex(f.mirror, list(sel))
        assert _same(f.arr.oindex[sel], want), (gid, name, "host route")
        got = f.arr.oindex[dsel]
        assert N.lib().zhip_last_kernel() == b"k_select_copy"
        assert _same(_host(got, f), want), (gid, name, "oindex")
        assert _same(_host(f.arr.get_orthogonal_selection(dsel), f), want), (gid, name)
        # out: a strided device view, decoded in place, and a host array
        big = torch.zeros(tuple(2 * s + 1 for s in want.shape), dtype=got.dtype, device=device)
        view = big[tuple(slice(1, 1 + 2 * s, 2) for s in want.shape)]
        assert f.arr.get_orthogonal_selection(dsel, out=view) is view
        assert _same(_host(view.contiguous(), f), want), (gid, name, "device view out")
        hout = np.zeros(want.shape, f.mirror.dtype)
        f.arr.get_orthogonal_selection(dsel, out=hout)
        assert _same(hout, want), (gid, name, "host out")
        if _getitem_is_orthogonal(tuple(np.asarray(s) if isinstance(s, list) else s for s in sel), nd):
            assert _same(_host(f.arr.get(dsel), f), want), (gid, name, "get")
            h = f.arr[dsel]
            assert isinstance(h, np.ndarray) and _same(h, want), (gid, name, "getitem")


def test_index_forms(device):
    import torch

    from zarr_hip import axes

    f = _read_fixture("f4be", device)
    m, shape = f.mirror, f.shape
    rng = np.random.default_rng(3)
    a, c = rng.integers(-shape[0], shape[0], 20), rng.integers(-shape[2], shape[2], 9)
    mixed = (torch.from_numpy(a.astype(np.int32)).to(device), slice(3, 30, 2),
             torch.from_numpy(c.astype(np.int16)).to(device))          # int32 and int16 tensors, a slice
    assert _same(_host(f.arr.oindex[mixed], f), _np_oindex(m, [a, slice(3, 30, 2), c]))
    u8 = torch.tensor([0, 28, 3, 3], dtype=torch.uint8, device=device)
    assert _same(_host(f.arr.oindex[..., u8], f), _np_oindex(m, [slice(None), slice(None), np.array([0, 28, 3, 3])]))
    ids = torch.from_numpy(a).to(device)
    assert _same(f.arr[ids, 2:9], m[a, 2:9])                          # a tensor next to slices through __getitem__
    assert _same(f.arr[ids], m[a])                                     # a bare tensor, 3-d array: orthogonal
    assert _same(f.arr[5, ids[:4] % shape[1]], m[5, a[:4] % shape[1]])
    # rows only in chunks that were never written: the fill value
    miss = torch.tensor([shape[0] - 1, -1, shape[0] - 2], device=device)
    got = _host(f.arr.oindex[miss, shape[1] - 1, :], f)
    assert _same(got, m[[shape[0] - 1, -1, shape[0] - 2], shape[1] - 1, :]) and (got == f.meta.fill_value).all()
    # empty: an empty result, nothing planned, nothing launched
    before = axes.READBACKS
    empty = torch.zeros(0, dtype=torch.int64, device=device)
    got = f.arr.oindex[empty, :, ids[:3]]
    assert got.is_cuda and tuple(got.shape) == (0, shape[1], 3)
    none = torch.zeros(shape[1], dtype=torch.bool, device=device)
    assert tuple(f.arr.oindex[ids, none].shape) == (20, 0, shape[2])
    f.arr.oindex[empty, :, :] = np.zeros((0, shape[1], shape[2]), np.float32)
    assert axes.READBACKS == before


@pytest.mark.parametrize("gid", WRITE_GEOMS)
def test_device_index_writes_match_numpy_and_the_oracle(gid, device):
    import torch

    f = Fixture(gid, device)
    initial = set(f.chunk_dict())
    rng = np.random.default_rng(7)
    dt = f.mirror.dtype
    nd = len(f.shape)
    torch_value = dt.kind == "f" or dt in (np.dtype("uint8"), np.dtype("int32"))
    for i, (name, sel) in enumerate(_oindex_cases(f.shape, rng).items()):
        dsel = _dev(sel, device)
        shape = _np_oindex(f.mirror, list(sel)).shape
        value = (rng.random(shape) * 100 + 300).astype(dt) if dt.kind == "f" else rng.integers(200, 250, shape).astype(dt)
        if name in ("one-array-bare", "int-list-slices"):
            sent = value = value.reshape(-1)[0]                        # a scalar
        elif name in ("unsorted-repeated-bare", "two-arrays-mesh") and torch_value:
            sent = torch.from_numpy(value.astype(dt.newbyteorder("="))).to(device)  # a device value
        else:
            sent = value                                               # a numpy value: repeats included
        if i % 3 == 0:
            f.arr.oindex[dsel] = sent
        elif i % 3 == 1 or not _getitem_is_orthogonal(tuple(np.asarray(s) if isinstance(s, list) else s for s in sel), nd):
            f.arr.set_orthogonal_selection(dsel, sent)
        else:
            f.arr[dsel] = sent
        _np_oindex_set(f.mirror, sel, value)
    _check_written(f)
    # a chunk that becomes all fill is gone; a missing chunk that gets a value exists
    fill = f.meta.fill_value
    first = tuple(np.arange(min(c, n)) for c, n in zip(f.meta.chunk_shape, f.shape))
    f.arr.oindex[_dev(first, device)] = fill
    _np_oindex_set(f.mirror, first, fill)
    last = tuple(np.array([n - 1]) for n in f.shape)
    f.arr.oindex[_dev(last, device)] = np.full((1,) * nd, 99, dt)
    _np_oindex_set(f.mirror, last, dt.type(99))
    after = set(f.chunk_dict())
    assert initial - after and after - initial, (initial, after)
    _check_written(f)


@pytest.mark.parametrize("gid", ["u2", "shard-end"])
def test_array_values_through_repeats_on_two_axes(gid, device):
    """The case the host tests avoid: every element is named several times,
    with both spellings, and each occurrence carries another value."""
    f = Fixture(gid, device)
    rng = np.random.default_rng(13)
    dt = f.mirror.dtype
    a = np.concatenate([rng.integers(0, f.shape[0], 12)] * 3 + [rng.integers(-f.shape[0], 0, 12)])
    c = np.concatenate([rng.integers(-f.shape[2], f.shape[2], 8)] * 4)
    rng.shuffle(a)
    sel = (a, slice(1, None, 3), c)
    shape = _np_oindex(f.mirror, list(sel)).shape
    value = rng.integers(1000, 60000, shape).astype(dt)
    f.arr.oindex[_dev(sel, device)] = value
    _np_oindex_set(f.mirror, sel, value)
    _check_written(f)
    sel = (7, a[:30] % f.shape[1], c)                                   # an integer: value without that axis
    value = rng.integers(1000, 60000, (30, len(c))).astype(dt)
    f.arr.set_orthogonal_selection(_dev(sel, device), value)
    _np_oindex_set(f.mirror, sel, value)
    f.arr.oindex[_dev((a,), device)] = np.arange(len(a)).astype(dt).reshape(-1, 1, 1)  # a broadcast value
    _np_oindex_set(f.mirror, (a,), np.broadcast_to(np.arange(len(a)).astype(dt).reshape(-1, 1, 1),
                                                    (len(a),) + f.shape[1:]))
    _check_written(f)


def test_narrowed_boxes_decode_only_the_touched_inner_chunks(device):
    """shard-end with one flipped byte in the first inner chunk of shard
    (0, 0, 0).  The host-index route decodes the selection's box only, so a
    selection confined to indices >= 16 on axis 0 reads clean; the device
    route narrows its boxes from the bounds the count kernel folded and does
    the same.  Touching the corrupt inner chunk raises on both routes."""
    good = _read_fixture("shard-end", device)
    bad = Fixture("shard-end", device, corrupt="c/0/0/0")
    rows = np.array([17, 30, 16, 30, 25])
    cols = np.array([31, 2, 2])
    for sel in ((rows, slice(0, 20), slice(3, 30)), (rows, slice(None, 32), cols), (rows - 32, 5, cols - 33)):
        want = _np_oindex(good.mirror, list(sel))
        assert _same(bad.arr.oindex[sel], want), "the fixture: the host route must read clean here"
        assert _same(_host(bad.arr.oindex[_dev(sel, device)], bad), want)
    touching = (np.array([17, 3]), slice(0, 20), cols)
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[touching]
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[_dev(touching, device)]
    before = bad.chunk_dict()
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[_dev(touching, device)] = np.float32(1)
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[_dev(touching, device)] = np.ones((2, 20, 3), np.float32)
    assert bad.chunk_dict() == before
    # a write confined to the sound inner chunks passes the corrupt one through as bytes
    sel = (rows, slice(0, 20), cols)
    value = np.arange(5 * 20 * 3, dtype=np.float32).reshape(5, 20, 3)
    bad.arr.oindex[_dev(sel, device)] = value
    mirror = good.mirror.copy()
    _np_oindex_set(mirror, sel, value)
    whole = (np.arange(16, 32), slice(0, 32), slice(0, 32))
    assert _same(_host(bad.arr.oindex[_dev(whole, device)], bad), _np_oindex(mirror, list(whole)))
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[_dev(touching, device)]


@pytest.mark.parametrize("gid", ["u2", "shard-end"])
def test_sub_batches_and_a_corrupt_chunk(gid, device, monkeypatch):
    from zarr_hip import fancy

    f = Fixture(gid, device)
    cshape = f.meta.chunk_shape
    monkeypatch.setattr(fancy, "FANCY_SCRATCH_BYTES", 2 * int(np.prod(cshape)) * f.mirror.dtype.itemsize)
    rng = np.random.default_rng(11)
    sel = (rng.permutation(f.shape[0])[:30], slice(None), np.append(rng.integers(0, f.shape[2], 9), f.shape[2] - 1))
    nchunks = len({(a // cshape[0], c // cshape[2]) for a in sel[0] for c in sel[2]}) * -(-f.shape[1] // cshape[1])
    assert nchunks >= 7
    dsel = _dev(sel, device)
    assert _same(_host(f.arr.oindex[dsel], f), _np_oindex(f.mirror, list(sel)))
    bad = Fixture(gid, device, corrupt="c/0/0/0")                       # the first touched chunk: the first sub-batch
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[dsel]
    value = rng.integers(300, 9000, (30, f.shape[1], 10)).astype(f.mirror.dtype)
    f.arr.oindex[dsel] = value
    _np_oindex_set(f.mirror, sel, value)
    _check_written(f)
    before = bad.chunk_dict()
    first = (np.array([1, 2]), slice(0, 4), np.array([3]))             # the corrupt chunk only
    with pytest.raises(ValueError, match="checksum"):
        bad.arr.oindex[_dev(first, device)] = value[:2, :4, :1]
    assert bad.chunk_dict() == before


def test_errors_and_dispatch(device, monkeypatch):
    import torch

    import zarr_hip
    from zarr_hip import _native as N
    from zarr_hip import axes

    f = _read_fixture("u1", device)
    m = f.mirror
    ok = (np.array([0, 1, 2]), slice(None), np.array([3, 4]))
    d = _dev(ok, device)
    assert _same(_host(f.arr.oindex[d], f), _np_oindex(m, list(ok)))
    oob = (np.array([0, 49, 3]), np.array([0, 37, 36]), np.array([28, 29, -30]))  # axes 1 and 2 fail
    before = axes.READBACKS
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 37"):
        f.arr.oindex[_dev(oob, device)]
    assert N.lib().zhip_last_kernel() == b"k_axis_count"               # nothing further was launched
    assert axes.READBACKS == before + 1
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 37"):
        f.arr.oindex[oob]                                               # the host route's message
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 50"):
        f.arr.oindex[_dev((np.array([-51]), slice(None)), device)] = 1
    with pytest.raises(IndexError, match="index out of bounds for dimension with length 50"):
        f.arr.oindex[_dev((np.array([5, 50, 5]),), device)] = np.zeros((3, 37, 29), np.uint8)  # keep-last planning
    assert N.lib().zhip_last_kernel() == b"k_axis_count"
    with pytest.raises(IndexError, match="Boolean array has the wrong length for dimension; expected 37, got 36"):
        f.arr.oindex[d[0], torch.zeros(36, dtype=torch.bool, device=device)]
    with pytest.raises(IndexError, match="Boolean array has the wrong length for dimension; expected 37, got 36"):
        f.arr.oindex[ok[0], np.zeros(36, bool)]
    with pytest.raises(IndexError, match="must be 1-dimensional only"):
        f.arr.oindex[torch.zeros((2, 2), dtype=torch.int64, device=device), :, :]
    with pytest.raises(IndexError, match="must be 1-dimensional only"):
        f.arr.oindex[np.zeros((2, 2), np.int64), :, :]
    with pytest.raises(IndexError, match="unsupported selection item"):
        f.arr.oindex[d[0].to(torch.float32), :, :]
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr.oindex[d[0], :, ok[2]]                                    # a numpy array next to a device tensor
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr.get_orthogonal_selection((d[0], [0, 1], slice(None)))
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr.set_orthogonal_selection((d[0], torch.from_numpy(ok[2])), 1)  # a host tensor
    with pytest.raises(TypeError, match="mixes device tensors"):
        f.arr[d[0], 2:9, ok[2]]
    with pytest.raises(ValueError, match="device"):
        f.arr.get((d[0], slice(None), slice(2, 9)), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="out of shape"):
        f.arr.get_orthogonal_selection(d, out=torch.zeros((3, 37, 3), dtype=torch.uint8, device=device))
    with pytest.raises(ValueError):
        f.arr.oindex[d] = np.zeros((3, 37, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="prepare_read"):
        f.arr.prepare_read(d)
    # a store on another device
    monkeypatch.setattr(f.store.arena, "device", torch.device("cuda", 1))
    with pytest.raises(ValueError, match="the store is on"):
        f.arr.oindex[d]
    monkeypatch.undo()
    # one tensor per dimension through arr[...] is still a coordinate selection
    pts = tuple(np.array([0, 20, 49]) % s for s in f.shape)
    assert _same(f.arr[_dev(pts, device)], m[pts])
    assert _same(_host(f.arr.get((_dev(pts, device)[0], 3, 4)), f), m[pts[0], 3, 4])
    assert _same(_host(f.arr.oindex[_dev(pts, device)], f), _np_oindex(m, list(pts)))  # ... and orthogonal when asked
    # rectilinear grids raise as on the host route
    r = zarr_hip.Array.create(zarr_hip.MemoryStore({}), (10, 6), ([3, 7], [6]), "uint8")
    with pytest.raises(NotImplementedError, match="rectilinear"):
        r.oindex[torch.tensor([1], device=device), :]
    with pytest.raises(NotImplementedError, match="rectilinear"):
        r.oindex[np.array([1]), :]


def test_one_planning_readback_per_selection(device):
    from zarr_hip import axes

    f = Fixture("u2", device)
    rng = np.random.default_rng(17)
    idx = [rng.integers(-s, s, 25) for s in f.shape]
    for k, sel in enumerate(((idx[0], slice(None), slice(2, 9)), (idx[0], 4, idx[2]), tuple(idx))):
        dsel = _dev(sel, device)
        before = axes.READBACKS
        got = f.arr.oindex[dsel]
        assert axes.READBACKS == before + 1, k + 1
        assert _same(_host(got, f), _np_oindex(f.mirror, list(sel)))
        value = rng.integers(1000, 60000, got.shape).astype(np.uint16)
        f.arr.oindex[dsel] = value                                      # keep-last planning: still one copy
        assert axes.READBACKS == before + 2, k + 1
        _np_oindex_set(f.mirror, sel, value)
        f.arr.set_orthogonal_selection(dsel, np.uint16(5))
        assert axes.READBACKS == before + 3, k + 1
        _np_oindex_set(f.mirror, sel, np.uint16(5))
    _check_written(f)


def test_missing_chunks_raise_when_the_array_says_so(device):
    import torch

    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    f = _read_fixture("u1", device)
    strict = zarr_hip.Array.open(f.store, config=ArrayConfig(read_missing_chunks=False))
    rows = torch.tensor([0, 1], device=device)
    assert _same(_host(strict.oindex[rows, 0:4, 0:4], f), f.mirror[[0, 1], 0:4, 0:4])
    with pytest.raises(zarr_hip.ChunkNotFoundError):
        strict.oindex[torch.tensor([f.shape[0] - 1], device=device), -1, -1]


def test_past_a_limit_the_host_route_serves_a_host_copy(device, monkeypatch):
    from zarr_hip import axes

    f = Fixture("u2", device)
    rng = np.random.default_rng(5)
    sel = (rng.integers(-50, 50, 40), slice(None), rng.integers(0, 29, 6))
    dsel = _dev(sel, device)
    monkeypatch.setattr(axes, "MAX_GRID", 3)  # axis 0 has 4 chunks
    with pytest.raises(axes.PointsLimit):
        axes.DeviceOrthogonalIndexer(dsel, f.shape, (16, 16, 16))
    before = axes.READBACKS
    assert _same(_host(f.arr.oindex[dsel], f), _np_oindex(f.mirror, list(sel)))
    assert axes.READBACKS == before
    monkeypatch.undo()
    monkeypatch.setattr(axes, "LAST_MAX_LEN", 40)  # keep-last only: reads and scalar writes stay on the device
    assert _same(_host(f.arr.oindex[dsel], f), _np_oindex(f.mirror, list(sel)))
    f.arr.oindex[dsel] = np.uint16(9)
    assert axes.READBACKS == before + 2
    _np_oindex_set(f.mirror, sel, np.uint16(9))
    value = rng.integers(1000, 60000, (40, 37, 6)).astype(np.uint16)
    f.arr.oindex[dsel] = value                                          # the array value: the host route
    assert axes.READBACKS == before + 2
    _np_oindex_set(f.mirror, sel, value)
    _check_written(f)
