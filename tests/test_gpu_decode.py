"""GPU parity: zarr_hip decode (HIP kernels through the C ABI) vs the CPU oracle,
bit-exact (compared as raw bytes so NaN payloads and -0.0 count).

Encoded inputs are produced by the oracle (oracle/oracle.py, test infrastructure)
from seeded data; the decode under test runs only on the GPU."""

import numpy as np
import pytest

from oracle import oracle as O
from conftest import set_tuning

pytestmark = pytest.mark.gpu

LE = {"name": "bytes", "configuration": {"endian": "little"}}
BE = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}


def T(order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def SHARD(inner_shape, codecs, loc="end", index=(LE, CRC)):
    return {"name": "sharding_indexed", "configuration": {
        "chunk_shape": list(inner_shape), "codecs": list(codecs), "index_codecs": list(index),
        "index_location": loc}}


def _data(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        a = rng.standard_normal(shape).astype(dt)
        flat = a.reshape(-1)
        if flat.size > 8:
            flat[3] = -0.0
            if dt.itemsize == 4:
                flat[5:6].view(np.uint32)[0] = 0x7FC00001  # NaN payload
            else:
                flat[5] = np.nan
        return a
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)


def _roundtrip(device, shape, chunks, dtype, codecs, fill=0, selection=(Ellipsis,), drop=None,
               order="C", seed=0, host_store=False):
    import zarr_hip
    from zarr_hip.spec import ArrayConfig

    meta = O.ArrayMeta(tuple(shape), tuple(chunks), np.dtype(dtype), fill, codecs=codecs)
    host = {}
    data = _data(shape, dtype, seed)
    O.write(host, meta, (Ellipsis,), data)
    for k in drop or []:
        host.pop(k, None)
    if host_store == "pinned":
        store = zarr_hip.PinnedMemoryStore(dict(host))
    elif host_store:
        store = zarr_hip.MemoryStore(dict(host))
    else:
        store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunks, dtype, fill, codecs=codecs,
                                config=ArrayConfig(order=order))
    got = arr[selection]
    want = O.read(host, meta, selection)
    assert got.shape == want.shape
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    return arr, host, meta


@pytest.mark.parametrize("dtype", ["float32", "int16", "uint8", "float64", "int32"])
def test_bytes_crc_full(device, dtype):
    _roundtrip(device, (40, 33, 20), (16, 16, 8), dtype, [LE, CRC])


def test_c2_shape(device):
    _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [LE, CRC])


@pytest.mark.parametrize("dtype", ["float32", "int16", "float64", "uint16"])
def test_big_endian(device, dtype):
    _roundtrip(device, (21, 34), (8, 16), dtype, [BE, CRC])


@pytest.mark.parametrize("shape,chunks,dtype,codecs,sel", [
    ((100000,), (16384,), "float32", [LE, CRC], (Ellipsis,)),          # boundary chunk: 128-byte rows
    ((100000,), (16384,), "float32", [LE, CRC], (slice(1000, 99000),)),  # 32-byte rows
    ((10 ** 6,), (2 ** 17,), "float32", [LE], (Ellipsis,)),            # C1 at 1/10 size
    ((300000,), (65536,), "int16", [BE, CRC], (Ellipsis,)),
    ((300000,), (65536,), "uint8", [LE, CRC], (slice(4096, 200704),)),
])
def test_1d_row_decode(device, shape, chunks, dtype, codecs, sel):
    """1-D chunks whose selections are whole R-item rows take the row decode
    (planner._split_1d views each chunk as (N/R, R))."""
    arr, _, _ = _roundtrip(device, shape, chunks, dtype, codecs, fill=5, selection=sel)
    prog, _ = arr.prepare_read(sel)
    assert prog.tables.rows and prog.tables.layout.ndim == 2


@pytest.mark.tuning
@pytest.mark.parametrize("tune", [64, 65536 | 64, 128, 2097152])
def test_rows_fallback_kernels(device, tune):
    """Whole-row batches without a row map (zhip_decode_predicted, or a map the
    library declines) take the persistent k_decode_rows; transposed layouts can
    be forced onto the one-tile k_decode_tile; whole-row batches with a row map
    can be forced onto one unit per workgroup (128) or k_decode_duo (2097152,
    the kernel chunks of > 32 units take by default).  All stay exact."""
    from zarr_hip import _native as N

    set_tuning(2, tune)
    try:
        _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [LE, CRC])
        _roundtrip(device, (128, 128, 64), (64, 64, 64), "float32",
                   [SHARD((32, 32, 64), [LE, CRC])])
        _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [T((2, 1, 0)), LE, CRC])
    finally:
        set_tuning(2, 0)


@pytest.mark.tuning
@pytest.mark.parametrize("case", ["missing", "partial", "sharded_missing_inner", "odd_units", "big_endian"])
def test_duo_kernel_cases(device, case):
    """k_decode_duo forced on whole-row layouts it does not take by default
    (chunks of <= 32 units): absent chunks -> fill, partial row selections,
    shard-index checks with absent inner chunks, an odd unit count (the last
    workgroup's second half idle), big-endian items.  Compared byte for byte
    with the oracle."""
    from zarr_hip import _native as N

    set_tuning(2, 2097152)
    try:
        if case == "missing":
            _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [LE, CRC], fill=7,
                       drop=["c/0/1/0", "c/1/1/1"])
        elif case == "partial":
            _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [LE, CRC],
                       selection=(slice(3, 120), slice(16, 112), slice(None)))
        elif case == "sharded_missing_inner":
            _roundtrip(device, (128, 128, 64), (64, 64, 64), "float32",
                       [SHARD((32, 32, 64), [LE, CRC])], fill=3, drop=["c/1/0/0"])
        elif case == "odd_units":
            # 3 chunks of 32 KiB rows: 3 units -> 2 workgroups, one half idle
            _roundtrip(device, (96, 256), (32, 256), "float32", [LE, CRC])
        else:
            _roundtrip(device, (128, 64, 64), (64, 64, 64), "int16", [BE, CRC])
    finally:
        set_tuning(2, 0)


def test_duo_crc_mismatch(device):
    """A corrupted chunk of > 32 units raises the reference's message.  These
    2 MiB chunks have 64 units, a multiple of 8, and the launch has 128 units
    (at most 512): since round 5 that is k_decode_ilw512, not k_decode_duo,
    which now takes only chunks of more than 32 units whose unit count is no
    multiple of 8 (its corruption cases: tests/test_gpu_kernel_matrix.py,
    duo_33 / duo_ragged)."""
    import zarr_hip
    from zarr_hip import _native as N

    meta = O.ArrayMeta((1024, 1024), (512, 1024), np.dtype("float32"), 0.0, codecs=[LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data((1024, 1024), "float32"))
    bad = bytearray(host["c/1/0"])
    bad[123457] ^= 0x08
    host["c/1/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (1024, 1024), (512, 1024), "float32", 0.0, codecs=[LE, CRC])
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.tables.rows
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)
    assert N.lib().zhip_last_kernel().decode() == "k_decode_ilw512"


def test_bytes_only_no_crc(device):
    _roundtrip(device, (1000,), (128,), "float32", [LE])


@pytest.mark.parametrize("order", [(2, 1, 0), (1, 2, 0), (0, 2, 1), (2, 0, 1)])
def test_transpose(device, order):
    _roundtrip(device, (10, 20, 30), (5, 10, 15), "float32", [T(order), LE, CRC], fill=np.nan)


def test_transpose_c3_shape(device):
    _roundtrip(device, (128, 64, 64), (64, 64, 64), "float32", [T((2, 1, 0)), LE, CRC])


@pytest.mark.parametrize("sel", [(slice(3, 17), slice(None, None, 3)), (5, slice(2, 30, 7)),
                                 (slice(1, 40, 13), 0), (-1, -2), (slice(None), slice(9, 10)),
                                 (slice(7, 8), slice(0, 29))])
def test_partial_selections(device, sel):
    _roundtrip(device, (37, 29), (8, 10), "float32", [LE, CRC], selection=sel)


def test_missing_chunks_fill(device):
    _roundtrip(device, (32, 32), (8, 8), "float32", [LE, CRC], fill=-7.5,
               drop=["c/0/0", "c/2/3", "c/3/3"])


def test_f_order_out(device):
    _roundtrip(device, (24, 20, 12), (8, 8, 8), "float32", [LE, CRC], order="F")


def test_host_store_staging(device):
    _roundtrip(device, (40, 40), (16, 16), "int16", [LE, CRC], host_store=True)


def test_crc_mismatch_raises_reference_message(device):
    import zarr_hip

    meta = O.ArrayMeta((16, 16), (8, 8), np.dtype("float32"), 0.0, codecs=[LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data((16, 16), "float32"))
    bad = bytearray(host["c/1/0"])
    bad[10] ^= 0x40
    host["c/1/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (16, 16), (8, 8), "float32", 0.0, codecs=[LE, CRC])
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)


# ------------------------------------------------------------------ sharding

@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("inner", [[LE, CRC], [LE], [T((1, 0, 2)), LE, CRC]])
def test_sharded(device, loc, inner):
    _roundtrip(device, (32, 32, 32), (16, 16, 16), "float32", [SHARD((8, 8, 8), inner, loc)])


def test_sharded_partial_and_missing_inner(device):
    # fill-valued inner chunks are elided at write time -> missing inner -> fill
    import zarr_hip

    codecs = [SHARD((4, 4), [LE, CRC])]
    meta = O.ArrayMeta((16, 24), (8, 8), np.dtype("int16"), -1, codecs=codecs)
    data = _data((16, 24), "int16")
    data[0:4, 4:8] = -1
    data[8:16, 16:24] = -1  # a whole shard of fill -> shard key absent
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    assert "c/1/2" not in host
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (16, 24), (8, 8), "int16", -1, codecs=codecs)
    for sel in [(Ellipsis,), (slice(3, 13), slice(2, 23, 3)), (7, slice(None)), (slice(9, 10), 20)]:
        got = arr[sel]
        want = O.read(host, meta, sel)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_sharded_index_crc_mismatch(device):
    import zarr_hip

    codecs = [SHARD((4, 4), [LE])]
    meta = O.ArrayMeta((8, 8), (8, 8), np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((8, 8), "float32"))
    bad = bytearray(host["c/0/0"])
    bad[-10] ^= 1  # inside the index
    host["c/0/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (8, 8), (8, 8), "float32", 0.0, codecs=codecs)
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)


def test_sharded_c4_like(device):
    # C4 geometry scaled down: 128^3 f32, 64^3 shards of 16^3 inner, crc
    _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [SHARD((16, 16, 16), [LE, CRC])])


def test_program_relaunch_is_idempotent(device):
    arr, host, meta = _roundtrip(device, (64, 64, 64), (32, 32, 32), "float32", [LE, CRC])
    prog, out = arr.prepare_read((Ellipsis,))
    for _ in range(3):
        prog.launch()
    prog.results()
    from zarr_hip.buffer import to_numpy

    assert to_numpy(out, "float32").tobytes() == O.read(host, meta).tobytes()


def test_read_graph_replay(device):
    """ReadGraph: captured launches over two programs replay to the oracle's bytes."""
    import torch

    import zarr_hip
    from zarr_hip.buffer import to_numpy

    codecs = [SHARD((16, 16, 16), [LE, CRC])]
    arr, host, meta = _roundtrip(device, (64, 64, 64), (32, 32, 32), "float32", codecs)
    p1, out1 = arr.prepare_read((Ellipsis,))
    p2, out2 = arr.prepare_read((slice(5, 60), slice(None, None, 2), 7))
    g = zarr_hip.ReadGraph([p1, p2], 5, device)
    out1.zero_()
    out2.zero_()
    g.replay()
    g.replay()
    g.results()
    torch.cuda.synchronize(device)
    assert to_numpy(out1, "float32").tobytes() == O.read(host, meta).tobytes()
    want2 = O.read(host, meta, (slice(5, 60), slice(None, None, 2), 7))
    assert to_numpy(out2, "float32").tobytes() == np.ascontiguousarray(want2).tobytes()


def test_read_graph_replay_detects_corruption(device):
    import zarr_hip

    meta = O.ArrayMeta((32, 32), (16, 16), np.dtype("float32"), 0.0, codecs=[LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data((32, 32), "float32"))
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (32, 32), (16, 16), "float32", 0.0, codecs=[LE, CRC])
    prog, _ = arr.prepare_read((Ellipsis,))
    g = zarr_hip.ReadGraph([prog], 3, device)
    g.replay()
    g.results()
    # flip one payload bit of chunk c/1/1 in HBM after capture: the replay re-verifies
    ref = store.get_sync("c/1/1")
    ref.arena.buf[ref.offset + 17] ^= 0x08
    bad = bytearray(host["c/1/1"])
    bad[17] ^= 0x08
    host["c/1/1"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    g.replay()
    with pytest.raises(ValueError) as got:
        g.results()
    assert str(got.value) == str(want.value)


# ------------------------------------------------- tiled transpose (ZHIP_DF_TILE)

@pytest.mark.parametrize("order", [(2, 1, 0), (1, 2, 0), (2, 0, 1), (0, 2, 1)])
@pytest.mark.parametrize("shape,chunks", [((64, 96, 128), (32, 48, 64)),   # partial tiles, 2 col blocks
                                          ((128, 128, 64), (128, 64, 64)),  # full 64-row tiles
                                          ((40, 24, 80), (20, 8, 80))])     # rows < 64, cols > 256 B
def test_transpose_tiled(device, order, shape, chunks):
    _roundtrip(device, shape, chunks, "float32", [T(order), LE, CRC], fill=np.nan)


@pytest.mark.parametrize("dtype,endian", [("int16", LE), ("uint8", LE), ("float64", LE),
                                          ("float32", BE), ("int16", BE), ("float64", BE)])
def test_transpose_tiled_dtypes(device, dtype, endian):
    _roundtrip(device, (64, 64, 64), (32, 32, 32), dtype, [T((2, 1, 0)), endian, CRC])


def test_transpose_tiled_missing_and_sharded(device):
    _roundtrip(device, (64, 64, 64), (32, 32, 32), "float32", [T((2, 1, 0)), LE, CRC], fill=-3.0,
               drop=["c/0/1/0", "c/1/1/1"])
    _roundtrip(device, (64, 64, 64), (32, 32, 32), "float32",
               [SHARD((16, 16, 16), [T((2, 1, 0)), LE, CRC])])


# k_decode_tile4: full 64-row x 256-byte tiles, four per workgroup
TILE4_CASES = [
    ("float32", LE, (64, 64, 64), (128, 128, 128)),   # the C3 chunk
    ("float64", BE, (32, 16, 64), (64, 48, 128)),     # 8-byte items, byteswap, 16 tiles per chunk
    ("int16", LE, (128, 8, 64), (256, 16, 64)),
    ("uint8", LE, (256, 8, 64), (256, 24, 128)),
]


def _tile4_engaged(arr):
    from zarr_hip import _native as N

    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.tables.tile
    return bool(N.Plan(prog.tables.layout, upload=False).kernel_flags & N.PK_TILE4)


@pytest.mark.parametrize("dtype,endian,chunks,shape", TILE4_CASES)
def test_transpose_tile4(device, dtype, endian, chunks, shape):
    arr, _, _ = _roundtrip(device, shape, chunks, dtype, [T((2, 1, 0)), endian, CRC])
    assert _tile4_engaged(arr)


@pytest.mark.parametrize("dtype,endian,chunks,shape", TILE4_CASES[:2])
def test_transpose_tile4_no_crc_missing_and_sharded(device, dtype, endian, chunks, shape):
    _roundtrip(device, shape, chunks, dtype, [T((2, 1, 0)), endian])
    arr, _, _ = _roundtrip(device, shape, chunks, dtype, [T((2, 1, 0)), endian, CRC], fill=-3,
                           drop=["c/0/0/1", "c/1/1/0"])
    assert _tile4_engaged(arr)
    shard = tuple(2 * c for c in chunks[:2]) + (chunks[2],)
    _roundtrip(device, shard, shard, dtype, [SHARD(chunks, [T((2, 1, 0)), endian, CRC])])


@pytest.mark.tuning
def test_transpose_tile4_crc_mismatch(device):
    import zarr_hip

    codecs = [T((2, 1, 0)), LE, CRC]
    meta = O.ArrayMeta((128, 64, 64), (64, 64, 64), np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((128, 64, 64), "float32"))
    bad = bytearray(host["c/1/0/0"])
    bad[700001] ^= 0x08
    host["c/1/0/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (128, 64, 64), (64, 64, 64), "float32", 0.0, codecs=codecs)
    assert _tile4_engaged(arr)
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)
    from zarr_hip import _native as N

    set_tuning(2, -(1 << 31))  # the same mismatch through the k_decode_tile4f arm
    try:
        with pytest.raises(ValueError) as got_f:
            zarr_hip.Array.create(store, (128, 64, 64), (64, 64, 64), "float32", 0.0, codecs=codecs)[...]
        assert N.lib().zhip_last_kernel() == b"k_decode_tile4f"
    finally:
        set_tuning(2, 0)
    assert str(got_f.value) == str(want.value)


@pytest.mark.tuning
@pytest.mark.parametrize("dtype,endian,chunks,shape", TILE4_CASES)
def test_transpose_tile4f_chain(device, dtype, endian, chunks, shape):
    """The k_decode_tile4f arm (kTuneTile4F, bit 31: the four tiles of a
    workgroup are 1 KiB of every stored row, one A_64 chain per thread) decodes
    exactly what the oracle wrote; without the bit k_decode_tile4w (its
    two-tile form) runs."""
    from zarr_hip import _native as N

    _roundtrip(device, shape, chunks, dtype, [T((2, 1, 0)), endian, CRC])
    assert N.lib().zhip_last_kernel() == b"k_decode_tile2w"
    set_tuning(2, -(1 << 31))
    try:
        # every case: 256-byte stored rows, one 64-row tile along the transposed dim
        _roundtrip(device, shape, chunks, dtype, [T((2, 1, 0)), endian, CRC])
        assert N.lib().zhip_last_kernel() == b"k_decode_tile4f"
    finally:
        set_tuning(2, 0)


def test_tile_mode_engaged(device):
    import zarr_hip

    meta = O.ArrayMeta((64, 64, 64), (32, 32, 32), np.dtype("float32"), 0.0,
                       codecs=[T((2, 1, 0)), LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data((64, 64, 64), "float32"))
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, meta.shape, meta.chunk_shape, "float32", 0.0, codecs=meta.codecs)
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.tables.tile and not prog.tables.fast


# ------------------------------------- shard-index CRC fused into the data launch

@pytest.mark.parametrize("loc", ["end", "start"])
def test_fused_index_check_engaged_and_correct(device, loc):
    arr, host, meta = _roundtrip(device, (64, 64, 64), (32, 32, 32), "float32",
                                 [SHARD((16, 16, 16), [LE, CRC], loc)])
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.index is None and prog.data.n_idx == 8


@pytest.mark.parametrize("loc", ["end", "start"])
def test_fused_index_crc_mismatch(device, loc):
    import zarr_hip

    codecs = [SHARD((4, 4), [LE, CRC], loc)]
    meta = O.ArrayMeta((8, 16), (8, 8), np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((8, 16), "float32"))
    bad = bytearray(host["c/0/1"])
    pos = len(bad) - 3 if loc == "end" else 3 * 16 + 9  # the CRC trailer / an entry's high bytes
    bad[pos] ^= 0x10
    host["c/0/1"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (8, 16), (8, 8), "float32", 0.0, codecs=codecs)
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.index is None and prog.data.n_idx == 2
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)


# ---- zarr's default sharding codecs (inner bytes only, index bytes + crc32c):
# the index checks ride in leading workgroups of the pair decode (VARIANT 9)

DEFAULT_SHARD_CASES = [
    ((128, 128, 128), (64, 64, 64), (32, 32, 32), "float32", (Ellipsis,), LE),
    ((128, 128, 128), (64, 64, 64), (32, 32, 32), "float32", (slice(3, 120), slice(32, 96), slice(None)), LE),
    ((128, 128, 128), (64, 64, 64), (32, 32, 32), "float32", (70, slice(None), slice(None)), BE),
    ((64, 128, 64), (32, 64, 64), (16, 64, 64), "int16", (Ellipsis,), BE),
    ((32, 64, 128), (16, 64, 128), (8, 32, 128), "float64", (slice(1, 31), slice(None), slice(None)), LE),
    ((64, 512, 64), (32, 256, 64), (16, 256, 64), "uint8", (Ellipsis,), {"name": "bytes"}),
    # inner chunks of <= 16 KiB: four per workgroup (k_decode_lead4) -- the
    # reference example's 64 x 64 int32, one live step (4 KiB), a 12 KiB chunk
    # (an empty head step), a partial last quad (6 chunks), 8-byte items
    ((256, 256), (128, 128), (64, 64), "int32", (Ellipsis,), LE),
    ((96, 256), (48, 128), (16, 64), "float32", (slice(5, 90), slice(64, 256)), BE),
    ((12, 32, 64), (6, 32, 64), (3, 16, 64), "float32", (slice(1, 11), slice(2, 30), slice(None)), LE),
    ((96, 128), (32, 128), (16, 128), "int16", (Ellipsis,), BE),
    ((16, 64, 32), (8, 32, 32), (4, 16, 32), "float64", (slice(1, 15), slice(2, 60), slice(None)), BE),
]


@pytest.mark.tuning
@pytest.mark.parametrize("shape,shards,inner,dtype,sel,endian", DEFAULT_SHARD_CASES)
@pytest.mark.parametrize("loc", ["end", "start"])
def test_default_sharding_chain_fused(device, shape, shards, inner, dtype, sel, endian, loc):
    import zarr_hip

    codecs = [SHARD(inner, [endian], loc)]
    meta = O.ArrayMeta(shape, shards, np.dtype(dtype), 0, codecs=codecs)
    data = _data(shape, dtype, seed=3)
    # one inner chunk of fill (elided: its index entry is the missing marker)
    data[tuple(slice(0, i) for i in inner)] = 0
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, shards, dtype, 0, codecs=codecs)
    prog, _ = arr.prepare_read(sel)
    n_shards = int(np.prod([s // c for s, c in zip(shape, shards)]))
    assert prog.tables.rows and prog.index is None
    assert 0 < prog.data.n_idx <= n_shards
    got = arr[sel]
    from zarr_hip import _native as N
    nb = int(np.prod(inner)) * np.dtype(dtype).itemsize
    small = nb <= 16384
    if small:
        _check_small_kernel(nb)
    else:
        assert N.lib().zhip_last_kernel() == b"k_decode_lead"
    want = O.read(host, meta, sel)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    if small:  # ZHIP_TUNE_ARM 11: the pair kernel for the same layout, same bytes
        set_tuning(6, 11)
        try:
            got2 = arr[sel]
            assert N.lib().zhip_last_kernel() == b"k_decode_lead"
        finally:
            set_tuning(6, 0)
        assert got2.tobytes() == got.tobytes()


def _small_kernel(nbytes):
    """k_decode_lead4 runs four chunks of <= 16 KiB per workgroup, eight of
    4-8 KiB (launched as k_decode_lead8)."""
    return b"k_decode_lead8" if 4096 < nbytes <= 8192 else b"k_decode_lead4"


def _check_small_kernel(nbytes):
    from zarr_hip import _native as N

    k, want = N.lib().zhip_last_kernel(), _small_kernel(nbytes)
    if want is None:
        assert k not in (b"k_decode_lead4", b"k_decode_lead8"), k
    else:
        assert k == want, k


# unsharded chunks of <= 16 KiB without a CRC (zarr's default v3 codecs,
# bytes only) take k_decode_lead4 too, with no leading workgroups
PLAIN_SMALL_CASES = [
    ((8, 32, 64), (2, 16, 64), "float32", (Ellipsis,), LE),
    ((256, 256), (64, 64), "int32", (Ellipsis,), LE),
    ((96, 256), (16, 64), "float32", (slice(5, 90), slice(64, 256)), BE),
    ((12, 32, 64), (3, 16, 64), "float32", (slice(1, 11), slice(2, 30), slice(None)), LE),
    ((96, 128), (16, 128), "int16", (Ellipsis,), BE),
    ((16, 64, 32), (4, 16, 32), "float64", (slice(1, 15), slice(2, 60), slice(None)), LE),
]


@pytest.mark.tuning
@pytest.mark.parametrize("shape,chunks,dtype,sel,endian", PLAIN_SMALL_CASES)
def test_plain_small_chunks_lead4(device, shape, chunks, dtype, sel, endian):
    import zarr_hip
    from zarr_hip import _native as N

    codecs = [endian]
    meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, dtype, seed=5))
    del host[[k for k in sorted(host) if k.startswith("c/")][1]]  # a missing chunk: fill
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunks, dtype, 0, codecs=codecs)
    got = arr[sel]
    _check_small_kernel(int(np.prod(chunks)) * np.dtype(dtype).itemsize)
    assert got.tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
    set_tuning(6, 11)  # the pair kernel on the same layout
    try:
        got2 = arr[sel]
        assert N.lib().zhip_last_kernel() == b"k_decode_pair"
    finally:
        set_tuning(6, 0)
    assert got2.tobytes() == got.tobytes()
    if int(np.prod(chunks)) * np.dtype(dtype).itemsize <= 8192:  # arms 12 / 13: four / eight per workgroup
        for arm, k in ((12, b"k_decode_lead4"), (13, b"k_decode_lead8")):
            set_tuning(6, arm)
            try:
                got3 = arr[sel]
                assert N.lib().zhip_last_kernel() == k
            finally:
                set_tuning(6, 0)
            assert got3.tobytes() == got.tobytes()


# chunks of <= 16 KiB WITH a crc32c trailer (unsharded, or inner chunks of a
# shard): k_decode_lead4's CRC form, one verdict per chunk in its workgroup
CRC_SMALL_CASES = [
    ((256, 256), (64, 64), "int32", (Ellipsis,), [LE, CRC], None),
    ((96, 256), (16, 64), "float32", (slice(5, 90), slice(64, 256)), [BE, CRC], None),
    ((12, 32, 64), (3, 16, 64), "float32", (Ellipsis,), [LE, CRC], None),
    ((96, 128), (16, 128), "int16", (Ellipsis,), [BE, CRC], None),
    ((256, 256), (128, 128), "int32", (Ellipsis,), None, (64, 64)),
    ((64, 64, 32), (16, 32, 32), "float64", (slice(1, 60), slice(None), slice(None)), None, (4, 16, 32)),
]


@pytest.mark.tuning
@pytest.mark.parametrize("shape,chunks,dtype,sel,codecs,inner", CRC_SMALL_CASES)
def test_crc_small_chunks_lead4(device, shape, chunks, dtype, sel, codecs, inner):
    import zarr_hip
    from zarr_hip import _native as N

    if inner is not None:
        codecs = [SHARD(inner, [LE, CRC])]
    meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
    host = {}
    data = _data(shape, dtype, seed=7)
    if inner is not None:
        data[tuple(slice(0, i) for i in inner)] = 0  # an elided inner chunk
    O.write(host, meta, (Ellipsis,), data)
    keys = [k for k in sorted(host) if k.startswith("c/")]
    if inner is None:
        del host[keys[1]]  # a missing chunk: fill
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dtype, 0, codecs=codecs)
    nb = int(np.prod(inner if inner is not None else chunks)) * np.dtype(dtype).itemsize
    got = arr[sel]
    _check_small_kernel(nb)
    assert got.tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
    set_tuning(6, 11)  # the pair kernels on the same layout
    try:
        got2 = arr[sel]
        assert N.lib().zhip_last_kernel() not in (b"k_decode_lead4", b"k_decode_lead8")
    finally:
        set_tuning(6, 0)
    assert got2.tobytes() == got.tobytes()
    bad = dict(host)
    b = bytearray(bad[keys[-1]])
    b[len(b) // 3] ^= 0x01  # inside a chunk's payload
    bad[keys[-1]] = bytes(b)
    with pytest.raises(ValueError) as want:
        O.read(bad, meta)
    arr2 = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(bad, device), shape, chunks, dtype, 0, codecs=codecs)
    with pytest.raises(ValueError) as err:
        arr2[...]
    _check_small_kernel(nb)
    assert str(err.value) == str(want.value)


@pytest.mark.parametrize("loc", ["end", "start"])
def test_default_sharding_chain_index_crc_mismatch(device, loc):
    import zarr_hip

    codecs = [SHARD((16, 256), [LE], loc)]
    meta = O.ArrayMeta((32, 512), (16, 512), np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((32, 512), "float32"))
    bad = bytearray(host["c/1/0"])
    pos = len(bad) - 3 if loc == "end" else 16 + 9
    bad[pos] ^= 0x10
    host["c/1/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (32, 512), (16, 512), "float32", 0.0, codecs=codecs)
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.index is None and prog.data.n_idx == 2 and prog.tables.rows
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)


# ------------------------------------ affine whole-row decode (ZHIP_DF_ROWS)

ROWS_CASES = [
    ((64, 96, 64), (32, 32, 64), "float32", (Ellipsis,)),
    ((64, 96, 64), (32, 32, 64), "float32", (slice(5, 61), slice(3, 90), slice(None))),
    ((64, 96, 64), (32, 32, 64), "float32", (7, slice(10, 70), slice(None))),
    ((40, 64, 64), (20, 32, 64), "int16", (slice(1, 39), slice(31, 33), slice(None))),
    ((16, 64, 64), (8, 16, 64), "float64", (Ellipsis,)),
    ((128, 256), (64, 64), "float32", (slice(17, 100), slice(None))),
    ((4, 512, 16), (2, 256, 16), "uint8", (slice(None), slice(100, 400), slice(None))),
]


@pytest.mark.parametrize("shape,chunks,dtype,sel", ROWS_CASES)
@pytest.mark.parametrize("endian", [LE, BE])
def test_rows_kernel(device, shape, chunks, dtype, sel, endian):
    if dtype == "uint8" and endian is BE:
        endian = {"name": "bytes"}
    arr, host, meta = _roundtrip(device, shape, chunks, dtype, [endian, CRC], selection=sel,
                                 fill=3, drop=["c/0/1/0", "c/1/0"])
    prog, _ = arr.prepare_read(sel)
    assert prog.tables.rows


def test_rows_kernel_sharded_and_missing_inner(device):
    import zarr_hip

    codecs = [SHARD((16, 16, 64), [LE, CRC])]
    meta = O.ArrayMeta((64, 64, 64), (32, 32, 64), np.dtype("float32"), -1.0, codecs=codecs)
    data = _data((64, 64, 64), "float32")
    data[0:16, 16:32, :] = -1.0  # an elided inner chunk
    host = {}
    O.write(host, meta, (Ellipsis,), data)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, (64, 64, 64), (32, 32, 64), "float32", -1.0, codecs=codecs)
    for sel in [(Ellipsis,), (slice(3, 50), slice(9, 60), slice(None))]:
        prog, _ = arr.prepare_read(sel)
        assert prog.tables.rows and prog.data.n_idx == 4
        got = arr[sel]
        assert got.tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()


def test_c2_takes_rows_kernel(device):
    arr, _, _ = _roundtrip(device, (128, 128, 128), (64, 64, 64), "float32", [LE, CRC])
    prog, _ = arr.prepare_read((Ellipsis,))
    assert prog.tables.fast and prog.tables.rows


def _repack_misaligned(blob: bytes, sh, cps) -> bytes:
    """Re-pack a shard so every inner chunk sits at an odd byte offset (padding
    between chunks, reverse order).  The index holds absolute offsets
    (_ShardIndex, sharding.py:205-318), so a reader must accept any placement."""
    import math

    chunks = O.shard_reader(np.frombuffer(blob, np.uint8), sh, cps)
    isz = O.shard_index_size(math.prod(cps), sh.index)
    start = isz if sh.index_location == "start" else 0
    parts, top = [], start
    index = np.full(tuple(cps) + (2,), O.MAX_UINT_64, dtype="<u8")
    for i, coords in enumerate(reversed(O.lexicographic_order_coords(cps))):
        raw = chunks[coords]
        if raw is None:
            continue
        pad = 1 + 2 * (i % 3)
        parts.append(b"\xa5" * pad)
        top += pad
        index[coords] = (top, len(raw))
        parts.append(raw.tobytes())
        top += len(raw)
    ib = O.encode_shard_index(index, sh.index).tobytes()
    body = b"".join(parts)
    return ib + body if sh.index_location == "start" else body + ib


@pytest.mark.parametrize("loc", ["end", "start"])
def test_rows_kernel_misaligned_inner_chunks(device, loc):
    """Inner chunks at byte-misaligned offsets through the rows kernel: bit-exact,
    CRC verified (the unaligned nontemporal loads)."""
    import zarr_hip

    codecs = [SHARD((16, 256), [LE, CRC], loc)]
    meta = O.ArrayMeta((64, 512), (32, 512), np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data((64, 512), "float32"))
    sh = meta.chain.shard
    for k in list(host):
        if k.startswith("c/"):
            host[k] = _repack_misaligned(host[k], sh, (2, 2))
    want = O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, meta.shape, meta.chunk_shape, "float32", 0.0, codecs=codecs)
    prog, out = arr.prepare_read((Ellipsis,))
    assert prog.tables.rows
    # the default-packing prediction is wrong for every inner chunk here: the
    # kernel must notice and reload from the live index
    assert prog.tables.predict is not None
    got = arr[...]
    assert got.tobytes() == want.tobytes()
    # a flipped payload bit in a misaligned chunk is still caught
    k0 = "c/1/0"
    bad = bytearray(host[k0])
    raw = O.shard_reader(np.frombuffer(bytes(bad), np.uint8), sh, (2, 2))[(1, 1)]
    off = bytes(bad).find(raw.tobytes())
    bad[off + 100] ^= 0x01
    host[k0] = bytes(bad)
    with pytest.raises(ValueError) as w:
        O.read(host, meta)
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, meta.shape, meta.chunk_shape, "float32", 0.0, codecs=codecs)
    with pytest.raises(ValueError) as g:
        arr[...]
    assert str(g.value) == str(w.value)


@pytest.mark.parametrize("loc", ["end", "start"])
def test_predicted_loads_engaged_and_exact(device, loc):
    """Default Morton packing: the load-address prediction fits (one 2-level
    progression) and the decode is bit-exact; a missing inner chunk turns the
    prediction off for its batch."""
    # 128 KiB inner chunks (four units: the pair kernel, which uses the
    # prediction; k_decode_il's layouts resolve their own units, no prediction)
    arr, host, meta = _roundtrip(device, (128, 128, 64), (64, 64, 64), "float32",
                                 [SHARD((32, 32, 32), [LE, CRC], loc)])
    prog, out = arr.prepare_read((Ellipsis,))
    assert prog.tables.rows and prog.tables.predict is not None
    assert prog.tables.predict.per == 8
    prog.launch()
    prog.results()
    from zarr_hip.buffer import to_numpy

    assert to_numpy(out, "float32").tobytes() == O.read(host, meta).tobytes()
    sel = (slice(3, 120), slice(None), slice(None))
    got = arr[sel]
    assert got.tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()


# k_decode_tileg: transposed layouts k_decode_tile4 declines (partial tiles,
# > 64 tiles per chunk, irregular steps between consecutive tiles), tiles
# grouped by four along a stored dim with shape % 4 == 0
def _tileg_engaged(arr):
    from zarr_hip import _native as N

    prog, _ = arr.prepare_read((Ellipsis,))
    kf = N.Plan(prog.tables.layout, upload=False).kernel_flags
    return prog.tables.tile and (kf & N.PK_TILEG) and not (kf & N.PK_TILE4)


@pytest.mark.parametrize("order", [(2, 1, 0), (1, 2, 0), (0, 2, 1), (2, 0, 1)])
@pytest.mark.parametrize("dtype,endian", [("float32", LE), ("int16", BE), ("float64", LE), ("uint8", LE)])
def test_transpose_tileg(device, order, dtype, endian):
    arr, _, _ = _roundtrip(device, (96, 160, 160), (96, 80, 80), dtype, [T(order), endian, CRC], fill=3)
    assert _tileg_engaged(arr)


def test_transpose_tileg_missing_sharded_and_crc(device):
    import zarr_hip

    # missing chunks -> fill
    arr, host, meta = _roundtrip(device, (96, 160, 160), (96, 80, 80), "float32", [T((2, 1, 0)), LE, CRC],
                                 fill=np.nan, drop=["c/0/1/0", "c/0/0/1"])
    assert _tileg_engaged(arr)
    # transposed inner chunks of a shard (128^3-like geometry, 512 tiles per inner chunk)
    _roundtrip(device, (128, 128, 128), (128, 128, 128), "float32",
               [SHARD((128, 64, 128), [T((2, 1, 0)), LE, CRC])])
    # CRC mismatch: the reference's message
    meta = O.ArrayMeta((96, 80, 80), (96, 80, 80), np.dtype("float32"), 0.0, codecs=[T((2, 1, 0)), LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data((96, 80, 80), "float32"))
    bad = bytearray(host["c/0/0/0"])
    bad[12345] ^= 4
    host["c/0/0/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), (96, 80, 80), (96, 80, 80),
                                "float32", 0.0, codecs=[T((2, 1, 0)), LE, CRC])
    assert _tileg_engaged(arr)
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)


def test_transpose_tileg_many_groups(device):
    """1024 groups per chunk (> 256: the arrival-count protocol) and 128
    groups (two-level 64-bit arrival, 8 subgroups of 16): decode and encode
    exact.  80-row tiles keep k_decode_tile4 out."""
    import zarr_hip

    for shape in [(512, 256, 80), (128, 128, 80)]:
        arr, host, meta = _roundtrip(device, shape, shape, "float32", [T((2, 1, 0)), LE, CRC])
        assert _tileg_engaged(arr)
        st = zarr_hip.DeviceStore(device, capacity=1 << 20)
        warr = zarr_hip.Array.create(st, shape, shape, "float32", 0.0, codecs=[T((2, 1, 0)), LE, CRC])
        warr[...] = O.read(host, meta)
        got = {k: v for k, v in st.to_dict().items() if not k.endswith("zarr.json")}
        assert got == host


# ------------------------------------------- CRC verdicts across launches
def _il_array(device, fill=0.0, kind="il"):
    """The headline geometry's chunk shape (64^3 f32 = 1 MiB: eight-workgroup
    groups, k_decode_il) on a small array; kind "tileg": 96 x 80 x 80 chunks
    through transpose (2, 1, 0) (k_decode_tileg, whose production publication
    is the deferred verdicts)."""
    import zarr_hip

    shape, chunks, codecs = (128, 64, 64), (64, 64, 64), [LE, CRC]
    if kind.startswith("tileg"):
        shape, chunks, codecs = (192, 80, 80), (96, 80, 80), [T((2, 1, 0)), LE, CRC]
    meta = O.ArrayMeta(shape, chunks, np.dtype("float32"), fill, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunks, "float32", fill, codecs=codecs)
    return arr, store, host, meta


# (kind, ZHIP_TUNE_ARM): k_decode_il's returning publication (arm 33 keeps
# k_decode_il on this small grid), its deferred-verdict arm, the small-grid
# production k_decode_ilh (look-back finalizer) and the round-5 one
# k_decode_ilw512 (arm 61), and the deferred verdicts of k_decode_tilegw
# (production: its two-tile form k_decode_tileg2w; arm 38 keeps four tiles)
# (production) and k_decode_tileg (arm 5)
VERDICT_CASES = [("il", 33), ("il", 2), ("ilh", 0), ("ilw512", 61), ("tileg2w", 0), ("tilegw", 38), ("tileg", 5)]


@pytest.fixture
def verdict_case(request):
    from zarr_hip import _native as N

    kind, arm = request.param
    set_tuning(6, arm)
    yield kind
    set_tuning(6, 0)


def _corrupt(store, host, key, at=4321):
    ref = store.get_sync(key)
    ref.arena.buf[ref.offset + at] ^= 0x10
    b = bytearray(host[key])
    b[at] ^= 0x10
    host[key] = bytes(b)


@pytest.mark.tuning
@pytest.mark.parametrize("verdict_case", VERDICT_CASES, indirect=True)
def test_deferred_verdict_sticky_over_eager_launches(device, verdict_case):
    """Launches without a result check in between: a chunk corrupted before an
    even number of launches still raises (deferred verdicts: consecutive
    launches publish into alternate banks and each checks the previous one),
    with the reference's message; then the restored bytes read clean."""
    from zarr_hip import _native as N

    arr, store, host, meta = _il_array(device, kind=verdict_case)
    prog, out = arr.prepare_read((Ellipsis,))
    prog.launch()
    prog.results()
    assert N.lib().zhip_last_kernel().decode() == "k_decode_" + verdict_case
    clean = dict(host)
    _corrupt(store, host, "c/1/0/0")
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    for n in (2, 3, 4):
        for _ in range(n):
            prog.launch()
        with pytest.raises(ValueError) as got:
            prog.results()
        assert str(got.value) == str(want.value)
    _corrupt(store, host, "c/1/0/0")  # flips the same bit back
    assert host == clean
    for _ in range(2):
        prog.launch()
        prog.results()
    assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()


@pytest.mark.tuning
@pytest.mark.parametrize("verdict_case", VERDICT_CASES, indirect=True)
@pytest.mark.parametrize("repeats", [1, 2, 3])
def test_deferred_verdict_graph_replays(device, repeats, verdict_case):
    """A captured read loop with 1, 2 or 3 launches of one program, replayed
    twice between result checks: corruption after capture raises (an odd
    count ends the graph with a zhip_dv_check node), clean data does not."""
    import zarr_hip

    arr, store, host, meta = _il_array(device, kind=verdict_case)
    prog, out = arr.prepare_read((Ellipsis,))
    g = zarr_hip.ReadGraph([prog], repeats, device)
    assert (g._dv_refs is not None) == (repeats % 2 == 1)
    g.replay()
    g.replay()
    g.results()
    _corrupt(store, host, "c/0/0/0", at=77)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    g.replay()
    g.replay()
    with pytest.raises(ValueError) as got:
        g.results()
    assert str(got.value) == str(want.value)
    _corrupt(store, host, "c/0/0/0", at=77)
    g.replay()
    g.results()
    g.replay()
    g.results()
    assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()


def test_deferred_verdict_host_slabs(device):
    """A host-sourced read through the slab pipeline (range launches of one
    plan) reports a mismatch in any slab, and the next clean read passes."""
    import zarr_hip

    shape, chunks = (512, 64, 64), (64, 64, 64)
    meta = O.ArrayMeta(shape, chunks, np.dtype("float32"), 0.0, codecs=[LE, CRC])
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    bad = dict(host)
    b = bytearray(bad["c/6/0/0"])
    b[999] ^= 0x02
    bad["c/6/0/0"] = bytes(b)
    with pytest.raises(ValueError) as want:
        O.read(bad, meta)
    arr = zarr_hip.Array.create(zarr_hip.MemoryStore(bad), shape, chunks, "float32", 0.0, codecs=[LE, CRC])
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)
    arr2 = zarr_hip.Array.create(zarr_hip.MemoryStore(dict(host)), shape, chunks, "float32", 0.0, codecs=[LE, CRC])
    for _ in range(2):
        assert arr2[...].tobytes() == O.read(host, meta).tobytes()


@pytest.mark.parametrize("sharded", [False, True])
def test_il_and_small_grid_kernels(device, sharded):
    """Production kernel choice for the headline's 1 MiB chunks: k_decode_il
    above kIlwMaxUnits (512) units, k_decode_ilh (16 KiB half units, the
    look-back finalizer) at or below; both bit-exact, a corrupted chunk
    reported with the reference's message."""
    import zarr_hip
    from zarr_hip import _native as N

    shape, chunks = (128, 128, 320), (64, 64, 64)  # 20 chunks = 640 units
    codecs = [SHARD((64, 64, 64), [LE, CRC])] if sharded else [LE, CRC]
    cshape = (128, 128, 64) if sharded else chunks
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 0.0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, cshape, "float32", 0.0, codecs=codecs)
    for sel, kernel in [((Ellipsis,), "k_decode_il"), ((slice(None), slice(None), slice(0, 128)), "k_decode_ilh")]:
        prog, out = arr.prepare_read(sel)
        prog.launch()
        prog.results()
        assert N.lib().zhip_last_kernel().decode() == kernel
        assert out.cpu().numpy().tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
    _corrupt(store, host, "c/0/0/2" if sharded else "c/1/1/2", at=123457)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    for sel in [(Ellipsis,), (slice(None), slice(None), slice(128, 192))]:
        with pytest.raises(ValueError) as got:
            arr[sel]
        assert str(got.value) == str(want.value)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [1, 2])
def test_il_arms_exact_and_crc(device, arm):
    """k_decode_il's timing arms (ZHIP_TUNE_ARM 1: the round-3 publication
    words 16 B apart, 2: deferred verdicts) decode bit-exactly and report a
    corrupted chunk with the reference's message, then read clean once it is
    restored."""
    from zarr_hip import _native as N

    arr, store, host, meta = _il_array(device)
    set_tuning(6, arm)
    try:
        prog, out = arr.prepare_read((Ellipsis,))
        prog.launch()
        prog.results()
        assert N.lib().zhip_last_kernel().decode() == "k_decode_il"
        assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
        _corrupt(store, host, "c/1/0/0", at=700001)
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        prog.launch()
        with pytest.raises(ValueError) as got:
            prog.results()
        assert str(got.value) == str(want.value)
        _corrupt(store, host, "c/1/0/0", at=700001)
        for _ in range(2):
            prog.launch()
            prog.results()
        assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    finally:
        set_tuning(6, 0)


@pytest.mark.tuning
@pytest.mark.parametrize("kind", ["tileg2w", "tilegw", "tileg"])
def test_c_abi_default_reports_mismatch_each_launch(device, kind):
    """A C caller that does not opt in to deferred verdicts (no ZHIP_DF_DEFER,
    never ZHIP_DF_BANK1) gets the documented zhip_decode contract from the
    transposing grouped decodes too: every launch over a corrupted chunk sets
    its status and the error word itself, two back-to-back launches alike, and
    the restored bytes then read clean (nothing stale left in a bank word)."""
    from zarr_hip import _native as N

    arr, store, host, meta = _il_array(device, kind="tileg")
    set_tuning(6, {"tileg": 5, "tilegw": 38, "tileg2w": 0}[kind])
    try:
        prog, out = arr.prepare_read((Ellipsis,))
        d = prog.data
        d.flags &= ~N.DF_DEFER
        d._bank = 0
        prog.launch()
        prog.results()
        assert N.lib().zhip_last_kernel().decode() == "k_decode_" + kind
        _corrupt(store, host, "c/1/0/0")
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        from zarr_hip.pipeline import STATUS_DT

        for _ in range(2):
            d._bank = 0  # a C caller that never sets ZHIP_DF_BANK1
            d.reset_errflag()
            d.d_status.zero_()
            d.launch()
            assert d.errflag() & (1 << N.ST_CRC_MISMATCH)
            st = d.d_status[: d.n * 4].cpu().numpy().view(STATUS_DT)
            assert (st["code"] == N.ST_CRC_MISMATCH).sum() == 1
            with pytest.raises(ValueError) as got:
                prog.results()
            assert str(got.value) == str(want.value)
        _corrupt(store, host, "c/1/0/0")
        for _ in range(2):
            d._bank = 0
            prog.launch()
            prog.results()
        assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    finally:
        set_tuning(6, 0)


ILQ_ARMS = {20: "k_decode_ilq2", 21: "k_decode_ilq4", 22: "k_decode_ilq1_glds", 23: "k_decode_ilq2_glds",
            24: "k_decode_ilq4_glds"}


@pytest.mark.tuning
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("arm", sorted(ILQ_ARMS))
def test_ilq_arms_exact_and_crc(device, arm, sharded):
    """k_decode_ilq (NQ units of one chunk per workgroup, tables by registers
    or LDS-DMA) decodes the headline chunk geometry bit-exactly -- whole
    array, a partial window, a missing chunk filled -- and reports a corrupted
    chunk (and, sharded, a corrupted index) with the reference's message."""
    import zarr_hip
    from zarr_hip import _native as N

    shape, chunks = (128, 128, 64), (64, 64, 64)
    codecs = [SHARD((64, 64, 64), [LE, CRC])] if sharded else [LE, CRC]
    cshape = (128, 128, 64) if sharded else chunks
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 1.5, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    if not sharded:
        host.pop("c/1/0/0")
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, cshape, "float32", 1.5, codecs=codecs)
    set_tuning(6, arm)
    try:
        for sel in [(Ellipsis,), (slice(16, 100), slice(0, 128), slice(0, 64))]:
            prog, out = arr.prepare_read(sel)
            prog.launch()
            prog.results()
            assert N.lib().zhip_last_kernel().decode() == ILQ_ARMS[arm]
            assert out.cpu().numpy().tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
        key = "c/0/0/0" if sharded else "c/0/1/0"
        for at in ([700001, len(host[key]) - 40] if sharded else [700001]):
            _corrupt(store, host, key, at=at)
            with pytest.raises(ValueError) as want:
                O.read(host, meta)
            prog, out = arr.prepare_read((Ellipsis,))
            prog.launch()
            with pytest.raises(ValueError) as got:
                prog.results()
            assert str(got.value) == str(want.value)
            _corrupt(store, host, key, at=at)
            prog.launch()
            prog.results()
            assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    finally:
        set_tuning(6, 0)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [25, 35])
@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("sharded", [False, True])
def test_ilc_arm_exact_and_crc(device, monkeypatch, sharded, loc, arm):
    """k_decode_ilc (ZHIP_TUNE_ARM 25: CRC tables computed in LDS from 64 basis
    words, predicted loads issued before the index resolves) and k_decode_ilp
    (35: the index entry checked after the stores) decode exactly, redo the
    unit when the prediction misses (misaligned repacked shards, an elided
    inner chunk), and report corrupted chunks and indexes with the
    reference's messages."""
    import zarr_hip
    import zarr_hip.pipeline as P
    from zarr_hip import _native as N

    monkeypatch.setattr(P, "IL_PREDICT", True)
    shape, chunks = (128, 128, 64), (64, 64, 64)
    codecs = [SHARD((64, 64, 64), [LE, CRC], loc)] if sharded else [LE, CRC]
    cshape = (128, 128, 64) if sharded else chunks
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 1.5, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    if not sharded and arm == 25:  # (a missing chunk turns the prediction off: k_decode_ilp needs it)
        host.pop("c/1/0/0")
    kname = "k_decode_ilc" if arm == 25 else "k_decode_ilp"
    set_tuning(6, arm)
    try:
        store = zarr_hip.DeviceStore.from_host(host, device)
        arr = zarr_hip.Array.create(store, shape, cshape, "float32", 1.5, codecs=codecs)
        for sel in [(Ellipsis,), (slice(16, 100), slice(0, 128), slice(0, 64))]:
            prog, out = arr.prepare_read(sel)
            assert prog.tables.predict is not None or arm == 25
            prog.launch()
            prog.results()
            assert N.lib().zhip_last_kernel().decode() == kname
            assert out.cpu().numpy().tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
        key = "c/0/0/0" if sharded else "c/0/1/0"
        for at in ([700001, len(host[key]) - 40 if loc == "end" else 20] if sharded else [700001]):
            _corrupt(store, host, key, at=at)
            with pytest.raises(ValueError) as want:
                O.read(host, meta)
            prog, out = arr.prepare_read((Ellipsis,))
            prog.launch()
            with pytest.raises(ValueError) as got:
                prog.results()
            assert str(got.value) == str(want.value)
            _corrupt(store, host, key, at=at)
            prog.launch()
            prog.results()
            assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
        if sharded:  # prediction wrong for every inner chunk: the kernel reloads
            mhost = dict(host)
            for k in list(mhost):
                if k.startswith("c/"):
                    mhost[k] = _repack_misaligned(mhost[k], meta.chain.shard, (2, 2, 1))
            marr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(mhost, device), shape, cshape, "float32",
                                         1.5, codecs=codecs)
            got = marr[...]
            assert N.lib().zhip_last_kernel().decode() == kname
            assert got.tobytes() == O.read(host, meta).tobytes()
            # an inner chunk entirely fill is elided (the index says missing) and
            # the chunks after it move: every later guess misses
            d2 = _data(shape, "float32")
            d2[0:64, 0:64, :] = 1.5
            h2 = {}
            O.write(h2, meta, (Ellipsis,), d2)
            earr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(h2, device), shape, cshape, "float32",
                                         1.5, codecs=codecs)
            got = earr[...]  # (no prediction when a blob is shorter than packed: k_decode_il then)
            assert N.lib().zhip_last_kernel().decode() in (kname, "k_decode_il")
            assert got.tobytes() == O.read(h2, meta).tobytes()
    finally:
        set_tuning(6, 0)


ILW_CASES = [  # (shape, chunks, inner chunks or None, dtype, endian)
    ((128, 128, 64), (64, 64, 64), None, "float32", LE),
    ((128, 128, 64), (128, 128, 64), (64, 64, 64), "float32", LE),
    ((64, 96, 64), (64, 96, 64), (32, 32, 64), "int16", BE),     # 128 KiB inner chunks: 4 units
    ((64, 64, 64), (64, 64, 64), (16, 64, 64), "float64", LE),   # 64 KiB inner chunks
]


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [41, 59, 60])
@pytest.mark.parametrize("case", [0, 1, 3])
def test_ilh_arm_exact_and_crc(device, arm, case):
    """k_decode_ilh (16 KiB per workgroup, the pair tables' A_4096 chain):
    ZHIP_TUNE_ARM 41 with the returning two-level arrival past 32 workgroups
    per chunk, 59 with the look-back finalizer (two words of arrivals), 60 the
    production form (look-back, AFF destinations for whole reads) -- exact,
    corrupted chunks and indexes reported with the reference's messages."""
    _ilw_case(device, arm, case)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [26, 27, 31, 32, 42])
@pytest.mark.parametrize("case", range(len(ILW_CASES)))
def test_ilw_arms_exact_and_crc(device, arm, case):
    """k_decode_ilw (one 32 KiB unit per 1024- / 512-lane workgroup, the
    small-share shape) decodes exactly -- whole array, a partial window, a
    missing chunk filled -- and reports a corrupted chunk (and, sharded, a
    corrupted index) with the reference's message."""
    _ilw_case(device, arm, case)


@pytest.mark.parametrize("shape,cshape,inner,dtype,endian,kname,affine", [
    ((256, 256, 128), (64, 64, 64), None, "float32", LE, "k_decode_il", True),                 # 1 024 units
    ((128, 128, 64), (128, 128, 64), (64, 64, 64), "float32", LE, "k_decode_ilh", True),       # sharded
    ((64, 128, 128), (32, 64, 64), None, "int16", BE, "k_decode_ilh", True),                   # 128-byte rows
    # three 4 KiB steps per z plane: no power-of-two split, the launch keeps the map
    ((128, 96, 64), (64, 48, 64), None, "float32", LE, "k_decode_ilh", False),
])
def test_whole_chunk_reads_compute_destinations(device, shape, cshape, inner, dtype, endian, kname, affine):
    """Whole-chunk reads launch with ZHIP_DF_WHOLE: k_decode_il /
    k_decode_ilh take each step's destination from the plan's affine form
    of the whole-chunk row map, not from the map -- exact with the map zeroed
    on the device (a map-driven launch would write nothing); a layout whose
    map has no two-level affine form keeps the map under the same flag; a
    partial window never sets it."""
    import zarr_hip
    from zarr_hip import _native as N

    codecs = [SHARD(inner, [endian, CRC])] if inner else [endian, CRC]
    meta = O.ArrayMeta(shape, cshape, np.dtype(dtype), 3, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, dtype))
    if not inner:  # a missing chunk: filled through the same destinations
        host.pop(sorted(k for k in host if k.startswith("c/"))[-1])
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, cshape, dtype, 3, codecs=codecs)
    prog, out = arr.prepare_read((Ellipsis,))
    assert prog.data.flags & N.DF_WHOLE
    if affine:
        prog.data.d_rowmap.zero_()
    prog.launch()
    prog.results()
    assert N.lib().zhip_last_kernel().decode() == kname
    assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    win = (slice(5, 60), slice(3, 64), slice(0, 64))
    prog, out = arr.prepare_read(win)
    assert not prog.data.flags & N.DF_WHOLE
    prog.launch()
    prog.results()
    assert out.cpu().numpy().tobytes() == np.ascontiguousarray(O.read(host, meta, win)).tobytes()


@pytest.mark.parametrize("win,kname", [
    ((slice(5, 60), slice(3, 64), slice(0, 64)), "k_decode_ilh"),             # one chunk, partial
    ((slice(5, 250), slice(3, 256), slice(0, 128)), "k_decode_il"),           # 32 chunks, edges partial
    ((slice(0, 256), slice(0, 256), slice(0, 128, 2)), "k_decode_il"),        # every chunk, strided
])
def test_df_whole_is_checked_not_trusted(device, win, kname):
    """ZHIP_DF_WHOLE set by a C caller on PARTIAL selections (the flag the
    Python path sets only for whole-chunk reads): the kernels read each
    chunk's selection record and keep the row map wherever it is not whole,
    so the read stays exact and nothing is written outside the selection --
    the out sits between two 1 MiB guard bands of a sentinel that must come
    back untouched (advisor round 5; chunk_utils.py:88-214 semantics)."""
    import torch

    import zarr_hip
    from zarr_hip import _native as N

    shape, cshape = (256, 256, 128), (64, 64, 64)
    codecs = [LE, CRC]
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 3, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, cshape, "float32", 3,
                                codecs=codecs)
    prog, out = arr.prepare_read(win)
    if prog.data.p_rowmap is None:
        pytest.skip("this window does not take the row-map launch")
    assert not prog.data.flags & N.DF_WHOLE
    guard = (1 << 20) // 4
    big = torch.full((out.numel() + 2 * guard,), -7.25, dtype=torch.float32, device=device)
    view = big[guard: guard + out.numel()].view(out.shape)
    assert view.is_contiguous() and out.is_contiguous()
    prog.retarget(view)
    prog.data.flags |= N.DF_WHOLE  # the false promise
    prog.launch()
    prog.results()
    assert N.lib().zhip_last_kernel().decode() == kname
    want = np.ascontiguousarray(O.read(host, meta, win))
    assert view.cpu().numpy().tobytes() == want.tobytes()
    g = big.cpu().numpy()
    assert (g[:guard] == -7.25).all() and (g[guard + out.numel():] == -7.25).all()


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [45, 49, 61])
@pytest.mark.parametrize("case", [0, 1])
def test_row_map_arm_exact_and_crc(device, arm, case):
    """Tuning arm 45 keeps the row-map loads for whole-chunk launches (the A/B
    reference of ZHIP_DF_WHOLE); arm 49 publishes through two subwords of 16
    on lines of their own: exact, missing chunks filled, corrupted chunks and
    indexes reported with the reference's message."""
    _ilw_case(device, arm, case, whole=True)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [49, 51, 52, 53, 54, 55, 56, 57, 58, 64, 65, 69, 70, 71])
def test_il_split_publication_arm(device, arm):
    """Tuning arms on k_decode_il (1 024 units, whole-chunk reads): 49, the
    split publication, and 51-53, wave priority at the run end / load issue /
    both, decode exactly and report a corrupted chunk."""
    import zarr_hip
    from zarr_hip import _native as N

    shape, cshape = (256, 256, 128), (64, 64, 64)
    codecs = [LE, CRC]
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    set_tuning(6, arm)
    try:
        arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, cshape, "float32", 0,
                                    codecs=codecs)
        assert arr[...].tobytes() == O.read(host, meta).tobytes()
        assert N.lib().zhip_last_kernel().decode() == "k_decode_il"
        bad = bytearray(host["c/1/2/1"])
        bad[70001] ^= 0x10
        host["c/1/2/1"] = bytes(bad)
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, cshape, "float32", 0,
                                    codecs=codecs)
        with pytest.raises(ValueError) as got:
            arr[...]
        assert str(got.value) == str(want.value)
    finally:
        set_tuning(6, 0)


def _il_first_step(r, S):
    """k_decode_il: workgroup r of a chunk takes steps (r / S) S 8 + r % S + S k (k < 8)."""
    return (r // S) * S * 8 + r % S


LB_CASES = {  # arm -> (shape, kernel, positions per chunk, byte offset of position p in a chunk)
    # k_decode_il, 1 MiB chunks (32 units): zhip_decode_mapped takes the widest interleave the plan built,
    # S = 32 (arm 58 is none of the arms 69 / 70 / 71 that force another), one group of 32 workgroups, so
    # workgroup p takes steps p + 32 k and its first step is step p: offset 4096 p + 2000
    58: ((256, 256, 128), "k_decode_il", 32, lambda p: 4096 * _il_first_step(p, 32) + 2000),
    # k_decode_ilw512 (the N = 8 share's shape): unit r takes steps 8 r .. 8 r + 7
    "58w": ((128, 128, 128), "k_decode_ilw512", 32, lambda p: 4096 * 8 * p + 2000),
    # k_decode_ilh: half unit u takes steps 8 (u / 2) + 4 (u % 2) .. + 3
    59: ((256, 256, 128), "k_decode_ilh", 64, lambda p: 4096 * 4 * p + 2000),
}


@pytest.mark.tuning
@pytest.mark.parametrize("case", [58, "58w", 59])
def test_lookback_finalizer_every_position(device, case):
    """The look-back finalizer (tuning arms 58 / 59: every workgroup but the
    chunk's last publishes by a non-returning xor and retires, the last one
    polls and compares): a corrupted byte in EACH workgroup position of a chunk
    -- the finalizer's own and every non-finalizer's -- sets that chunk's
    CRC_MISMATCH status and the error word and raises the reference's message
    (crc32c_.py:34-50), while the other chunks stay OK; the restored bytes then
    read exactly (the self-resetting words hold nothing stale)."""
    import zarr_hip
    from zarr_hip import _native as N
    from zarr_hip.pipeline import STATUS_DT

    arm = 58 if case == "58w" else case
    shape, kname, npos, off = LB_CASES[case]
    cshape = (64, 64, 64)
    codecs = [LE, CRC]
    meta = O.ArrayMeta(shape, cshape, np.dtype("float32"), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, "float32"))
    keys = sorted(k for k in host if k.startswith("c/"))
    nc = len(keys)
    set_tuning(6, arm)
    try:
        store = zarr_hip.DeviceStore.from_host(host, device)
        arr = zarr_hip.Array.create(store, shape, cshape, "float32", 0, codecs=codecs)
        prog, out = arr.prepare_read((Ellipsis,))
        prog.launch()
        prog.results()
        assert N.lib().zhip_last_kernel().decode() == kname
        assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
        d = prog.data
        assert d.n == nc
        for rnd in range((npos + nc - 1) // nc):
            hit = {}
            for i, key in enumerate(keys):
                p = rnd * nc + i
                if p < npos:
                    _corrupt(store, host, key, at=off(p))
                    hit[key] = p
            with pytest.raises(ValueError) as want:
                O.read(host, meta)
            d.reset_errflag()
            prog.launch()
            st = d.d_status[: d.n * 4].cpu().numpy().view(STATUS_DT)
            assert d.errflag() & (1 << N.ST_CRC_MISMATCH)
            assert (st["code"] == N.ST_CRC_MISMATCH).sum() == len(hit), (rnd, sorted(hit.values()))
            with pytest.raises(ValueError) as got:
                prog.results()
            assert str(got.value) == str(want.value)
            for key, p in hit.items():
                _corrupt(store, host, key, at=off(p))
            for _ in range(2):
                prog.launch()
                prog.results()
            assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    finally:
        set_tuning(6, 0)


def _ilw_case(device, arm, case, whole=False):
    import zarr_hip
    from zarr_hip import _native as N

    shape, cshape, inner, dtype, endian = ILW_CASES[case]
    codecs = [SHARD(inner, [endian, CRC])] if inner else [endian, CRC]
    meta = O.ArrayMeta(shape, cshape, np.dtype(dtype), 3, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, dtype))
    if not inner:
        host.pop("c/1/0/0")
    want_kernel = {26: "k_decode_ilw1024", 27: "k_decode_ilw512", 31: "k_decode_ilw1024r", 32: "k_decode_ilw512r",
                   41: "k_decode_ilh", 42: "k_decode_ilw512m", 45: "k_decode_ilw512",
                   49: "k_decode_ilw512", 59: "k_decode_ilh", 60: "k_decode_ilh", 61: "k_decode_ilw512"}[arm]
    set_tuning(6, arm)
    try:
        store = zarr_hip.DeviceStore.from_host(host, device)
        arr = zarr_hip.Array.create(store, shape, cshape, dtype, 3, codecs=codecs)
        # (whole: the affine arms take whole-chunk selections only)
        for sel in [(Ellipsis,)] + ([] if whole else [(slice(5, 60), slice(3, 64), slice(0, 64))]):
            prog, out = arr.prepare_read(sel)
            prog.launch()
            prog.results()
            assert N.lib().zhip_last_kernel().decode() == want_kernel
            assert out.cpu().numpy().tobytes() == np.ascontiguousarray(O.read(host, meta, sel)).tobytes()
        key = "c/0/0/0"
        for at in ([70001, len(host[key]) - 40] if inner else [70001]):
            _corrupt(store, host, key, at=at)
            with pytest.raises(ValueError) as want:
                O.read(host, meta)
            prog, out = arr.prepare_read((Ellipsis,))
            prog.launch()
            with pytest.raises(ValueError) as got:
                prog.results()
            assert str(got.value) == str(want.value)
            _corrupt(store, host, key, at=at)
            prog.launch()
            prog.results()
            assert out.cpu().numpy().tobytes() == O.read(host, meta).tobytes()
    finally:
        set_tuning(6, 0)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [0, 5, 37, 38, 49, 67])
@pytest.mark.parametrize("dtype,endian,chunks,shape", TILE4_CASES)
def test_transpose_tile4w_and_tile4(device, dtype, endian, chunks, shape, arm):
    """k_decode_tile4w's two-tile form (production for CRC layouts of at most
    64 tiles per chunk: two waves per tile, one A_(4 sq) chain per lane),
    its one- and four-tile forms (ZHIP_TUNE_ARM 37 / 38) and k_decode_tile4
    (5) decode exactly what the oracle wrote and report a corrupted chunk
    with the reference's message."""
    import zarr_hip
    from zarr_hip import _native as N

    codecs = [T((2, 1, 0)), endian, CRC]
    kernel = {0: b"k_decode_tile2w", 5: b"k_decode_tile4", 37: b"k_decode_tile1w", 38: b"k_decode_tile4w",
              49: b"k_decode_tile2ws", 67: b"k_decode_tile2w_bt"}[arm]
    set_tuning(6, arm)
    try:
        _roundtrip(device, shape, chunks, dtype, codecs)
        assert N.lib().zhip_last_kernel() == kernel
        meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
        host = {}
        O.write(host, meta, (Ellipsis,), _data(shape, dtype))
        key = sorted(k for k in host if not k.endswith("zarr.json"))[-1]
        bad = bytearray(host[key])
        bad[len(bad) // 3] ^= 0x20
        host[key] = bytes(bad)
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dtype, 0,
                                    codecs=codecs)
        with pytest.raises(ValueError) as got:
            arr[...]
        assert str(got.value) == str(want.value)
        assert N.lib().zhip_last_kernel() == kernel
    finally:
        set_tuning(6, 0)


def test_transpose_tile4w_many_workgroups_per_chunk(device):
    """k_decode_tile4w with more than 32 workgroups per chunk (256 tiles of a
    128 x 64 x 256 int16 chunk: 64 groups of four) reports through subwords
    of 16 arrivals: exact, a missing chunk filled, a corrupted chunk reported
    with the reference's message on every launch of one program."""
    import zarr_hip
    from zarr_hip import _native as N

    shape, chunks, dtype = (128, 128, 256), (128, 64, 256), "int16"
    codecs = [T((2, 1, 0)), BE, CRC]
    _roundtrip(device, shape, chunks, dtype, codecs, fill=3, drop=["c/0/1/0"])
    assert N.lib().zhip_last_kernel() == b"k_decode_tile4w"
    meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, dtype))
    bad = bytearray(host["c/0/1/0"])
    bad[12345] ^= 0x01
    host["c/0/1/0"] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dtype, 0,
                                codecs=codecs)
    prog, out = arr.prepare_read((Ellipsis,))
    for _ in range(3):
        prog.launch()
        with pytest.raises(ValueError) as got:
            prog.results()
        assert str(got.value) == str(want.value)


TILEP_CASES = [  # full tiles that k_decode_tile4 declines: consecutive tile pairs (k_decode_tilep)
    ("float32", LE, (128, 128, 128), (128, 128, 256), (2, 1, 0)),   # C3 in 128^3 chunks
    ("int16", BE, (256, 32, 64), (256, 64, 128), (2, 1, 0)),        # (uniform groups: the tile4 plan's pairs)
    ("float64", LE, (64, 128, 64), (128, 128, 64), (1, 2, 0)),
]


@pytest.mark.tuning
@pytest.mark.parametrize("dtype,endian,chunks,shape,order", TILEP_CASES)
def test_transpose_tile_pairs(device, dtype, endian, chunks, shape, order):
    """Transposed CRC layouts whose tiles are full but whose natural groups of
    four sit at two steps (k_decode_tile4 declines): one workgroup per pair of
    consecutive tiles (the two column blocks of a row band), two waves per
    tile, subword arrival past 32 workgroups per chunk (ZHIP_TUNE_ARM 39) --
    exact, a missing chunk filled, a corrupted chunk reported with the
    reference's message."""

    codecs = [T(order), endian, CRC]
    set_tuning(6, 39)  # (tuning arm: the grouped kernels are the production choice)
    try:
        _tile_pairs_case(device, dtype, endian, chunks, shape, order, codecs)
    finally:
        set_tuning(6, 0)


def _tile_pairs_case(device, dtype, endian, chunks, shape, order, codecs):
    import zarr_hip
    from zarr_hip import _native as N

    grid = [sh // ch for sh, ch in zip(shape, chunks)]
    key = "c/" + "/".join(str(int(x)) for x in np.unravel_index(1, grid))
    _roundtrip(device, shape, chunks, dtype, codecs, fill=3, drop=[key])
    # (where the natural groups of four are uniform, tile4's plan takes the same pairs: k_decode_tile2w)
    assert N.lib().zhip_last_kernel() in (b"k_decode_tilep", b"k_decode_tile2w")
    meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(shape, dtype))
    bad = bytearray(host[key])
    bad[len(bad) // 3 + 7] ^= 0x08
    host[key] = bytes(bad)
    with pytest.raises(ValueError) as want:
        O.read(host, meta)
    arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dtype, 0,
                                codecs=codecs)
    with pytest.raises(ValueError) as got:
        arr[...]
    assert str(got.value) == str(want.value)
    # repeated launches of one program: the arrival words reset themselves
    prog, out = arr.prepare_read((Ellipsis,))
    for _ in range(3):
        prog.launch()
        with pytest.raises(ValueError):
            prog.results()


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [0, 48, 62, 66])
def test_transpose_tileg_128_chunks_arrivals(device, arm):
    """C3's 128^3-chunk geometry (256 workgroups per chunk in the two-tile
    form: 16 arrival subwords and a second level): the returning publication
    with its words on lines of their own (production) and packed (tuning arm
    48) decodes exactly, fills a missing chunk and reports a corrupted one."""
    import zarr_hip
    from zarr_hip import _native as N

    codecs = [T((2, 1, 0)), LE, CRC]
    kernel = {0: b"k_decode_tileg2w", 48: b"k_decode_tileg2wp", 62: b"k_decode_tileg2w_lb",
              66: b"k_decode_tileg2w_bt"}[arm]
    set_tuning(6, arm)
    try:
        arr, host, meta = _roundtrip(device, (128, 256, 256), (128, 128, 128), "float32", codecs, fill=3,
                                     drop=["c/0/1/0"])
        assert N.lib().zhip_last_kernel() == kernel
        bad = bytearray(host["c/0/0/1"])
        bad[len(bad) // 3 + 5] ^= 0x40
        host["c/0/0/1"] = bytes(bad)
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), (128, 256, 256),
                                    (128, 128, 128), "float32", 3, codecs=codecs)
        with pytest.raises(ValueError) as got:
            arr[...]
        assert str(got.value) == str(want.value)
        assert N.lib().zhip_last_kernel() == kernel
    finally:
        set_tuning(6, 0)


@pytest.mark.tuning
@pytest.mark.parametrize("arm", [0, 5, 38, 40, 48, 62, 66])
@pytest.mark.parametrize("order", [(2, 1, 0), (1, 2, 0), (0, 2, 1)])
@pytest.mark.parametrize("dtype,endian", [("float32", LE), ("int16", BE), ("float64", LE), ("uint8", LE)])
def test_transpose_tilegw_and_tileg(device, order, dtype, endian, arm):
    """k_decode_tilegw's two-tile form (production for grouped CRC layouts:
    two workgroups per group of four tiles, two waves per tile, one A_(4 sq)
    chain per lane; partial tiles load zeros), its four-tile form (ZHIP_TUNE_ARM
    38) and k_decode_tileg (5) decode exactly what the oracle wrote, fill
    missing chunks and report a corrupted chunk with the reference's message."""
    import zarr_hip
    from zarr_hip import _native as N

    codecs = [T(order), endian, CRC]
    kernel = {0: b"k_decode_tileg2w", 5: b"k_decode_tileg", 38: b"k_decode_tilegw", 40: b"k_decode_tileglt",
              48: b"k_decode_tileg2wp", 62: b"k_decode_tileg2w_lb", 66: b"k_decode_tileg2w_bt"}[arm]
    set_tuning(6, arm)
    try:
        # (arm 62 takes the look-back form only up to 128 groups per chunk)
        ok_names = (kernel, b"k_decode_tileg2w") if arm == 62 else (kernel,)
        _roundtrip(device, (96, 160, 160), (96, 80, 80), dtype, codecs, fill=3, drop=["c/0/1/0"])
        assert N.lib().zhip_last_kernel() in ok_names
        shape, chunks = (96, 80, 160), (96, 80, 80)
        meta = O.ArrayMeta(shape, chunks, np.dtype(dtype), 0, codecs=codecs)
        host = {}
        O.write(host, meta, (Ellipsis,), _data(shape, dtype))
        bad = bytearray(host["c/0/0/1"])
        bad[len(bad) // 2 + 5] ^= 0x40
        host["c/0/0/1"] = bytes(bad)
        with pytest.raises(ValueError) as want:
            O.read(host, meta)
        arr = zarr_hip.Array.create(zarr_hip.DeviceStore.from_host(host, device), shape, chunks, dtype, 0,
                                    codecs=codecs)
        with pytest.raises(ValueError) as got:
            arr[...]
        assert str(got.value) == str(want.value)
        assert N.lib().zhip_last_kernel() in ok_names
    finally:
        set_tuning(6, 0)
