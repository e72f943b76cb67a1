"""scale_offset / cast_value end to end on the GPU, against the oracle composed
with the independent per-element reference of value_cases.py.

Expected reads: the stored-domain array is written with ``oracle.write`` under
the stored chain (the chain without the value codecs, stored dtype and fill),
chosen keys are deleted, and the read must equal ``decode_ref(oracle.read)``
with the ARRAY fill over the deleted chunks.  Expected stores: per chunk the
key is absent when the array-domain chunk is all_equal to the fill, else it
holds the oracle's chain encoding of ``encode_ref(chunk)``."""

import numpy as np
import pytest

import value_cases as VC
import zarr_hip
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPE, CHUNKS = (20, 13), (8, 8)
BYTES_BE = {"name": "bytes", "configuration": {"endian": "big"}}
BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
CRC = {"name": "crc32c"}
SO = {"name": "scale_offset", "configuration": {"offset": -2.5, "scale": 10}}
CAST16 = {"name": "cast_value", "configuration": {"data_type": "int16"}}
FILL = 0.25


def T(order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


class Packed:
    """One array: its full chain, its stored chain, and both directions of the
    reference map."""

    def __init__(self, codecs, adt="float32", fill=FILL, shape=SHAPE, chunks=CHUNKS):
        self.codecs = list(codecs)
        self.adt = np.dtype(adt)
        self.fill = self.adt.type(fill)
        self.shape, self.chunks = shape, chunks
        so = next((c for c in codecs if c["name"] == "scale_offset"), None)
        cast = next((c for c in codecs if c["name"] == "cast_value"), None)
        self.sdt = np.dtype(cast["configuration"]["data_type"]) if cast else self.adt
        so_t = None
        if so:
            conf = so.get("configuration", {})
            so_t = (self.adt.type(conf.get("offset", 0)), self.adt.type(conf.get("scale", 1)))
        cd = None
        if cast:
            conf = cast["configuration"]
            cd = dict(rounding=conf.get("rounding", "nearest-even"), out_of_range=conf.get("out_of_range"), map=[])
        self.desc = {e: dict(encode=e, array_dt=self.adt.name, stored_dt=self.sdt.name, so=so_t, cast=cd,
                             fill=self.fill) for e in (True, False)}
        self.sfill = self.encode(np.array([self.fill]))[0][0]
        stored_codecs = [c for c in codecs if c["name"] not in ("scale_offset", "cast_value")]
        self.smeta = O.ArrayMeta(shape, chunks, self.sdt, self.sfill, codecs=stored_codecs, write_empty_chunks=True)

    def _map(self, arr, encode):
        dst = self.sdt if encode else self.adt
        out = np.empty(arr.shape, dst)
        err = 0
        for idx in np.ndindex(*arr.shape):
            out[idx], e = VC.ref_one(self.desc[encode], arr[idx])
            err |= e
        return out, err

    def encode(self, arr):
        return self._map(np.asarray(arr, self.adt), True)

    def decode(self, arr):
        return self._map(np.asarray(arr, self.sdt), False)

    def host_store(self, data, delete=()):
        """The store the oracle writes for array-domain data (every chunk
        present), without the deleted keys."""
        host = {}
        stored, err = self.encode(data)
        assert err == 0
        O.write(host, self.smeta, (Ellipsis,), stored)
        for k in delete:
            del host[k]
        return host

    def expected_read(self, host):
        want, err = self.decode(O.read(host, self.smeta))
        assert err == 0
        proj, _ = O.basic_indexer((Ellipsis,), self.shape, self.chunks)
        for coords, csel, osel, _ in proj:
            if self.smeta.chunk_key(coords) not in host:
                want[osel] = self.fill
        return want

    def open(self, host, device):
        store = zarr_hip.DeviceStore.from_host(host, device)
        return store, zarr_hip.Array.create(store, self.shape, self.chunks, self.adt, self.fill, codecs=self.codecs)

    def expected_store(self, host, written, new):
        """The store after a write of new[written] (full-array mask and
        values), by the reference's four steps per touched chunk: decode the
        existing chunk (none for a complete write or an absent key: the fill),
        merge, all_equal(fill) on the array-domain chunk, re-encode it whole."""
        want = dict(host)
        proj, _ = O.basic_indexer((Ellipsis,), self.shape, self.chunks)
        spec = self.smeta.spec()
        for coords, csel, osel, _ in proj:
            w = written[osel]
            if not w.any():
                continue
            key = self.smeta.chunk_key(coords)
            raw = None if w.all() else host.get(key)
            if raw is None:
                chunk = np.full(self.chunks, self.fill, self.adt)
            else:
                chunk, err = self.decode(O.chain_decode(O._as_u8(raw), self.smeta.chain, spec))
                assert err == 0
            chunk[csel][w] = new[osel][w]
            if O.all_equal(chunk, self.fill):
                want.pop(key, None)
            else:
                enc, err = self.encode(chunk)
                assert err == 0
                want[key] = bytes(O.chain_encode(enc, self.smeta.chain, spec))
        return want

    def check_write(self, store, arr, written, new, do):
        host = _chunk_bytes(store.to_dict())
        want = self.expected_store(host, written, new)
        do()
        got = _chunk_bytes(store.to_dict())
        assert set(got) == set(want)
        assert got == want


def _mask(shape, sel):
    m = np.zeros(shape, bool)
    m[sel] = True
    return m


def _data(shape=SHAPE, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3000, 3000, shape) / 10.0 - 2.5).astype(np.float32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _chunk_bytes(d):
    return {k: bytes(v) for k, v in d.items() if not k.endswith("zarr.json")}


CHAINS = {
    "so": [SO, BYTES_BE, CRC],
    "cast": [CAST16, BYTES_BE, CRC],
    "so-cast": [SO, CAST16, BYTES_BE, CRC],
    "t-so-cast": [T((1, 0)), SO, CAST16, BYTES_BE, CRC],
    "so-cast-t": [SO, CAST16, T((1, 0)), BYTES_BE, CRC],
    "so-t-cast": [SO, T((1, 0)), CAST16, BYTES_LE],
    "gzip": [SO, CAST16, BYTES_BE, {"name": "gzip", "configuration": {"level": 1}}],
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_reads_match_the_oracle_and_missing_chunks_read_as_the_array_fill(name, device):
    p = Packed(CHAINS[name])
    data = np.rint(_data()) if name == "cast" else _data()
    host = p.host_store(data, delete=("c/1/0",))
    store, arr = p.open(host, device)
    want = p.expected_read(host)
    assert (want[8:16, 0:8] == np.float32(FILL)).all()  # not decode(encode(0.25)) = 0.2 / -2.5
    assert _same(arr[...], want)
    assert _same(arr[3:19:2, 1:12], want[3:19:2, 1:12])
    assert _same(arr[9, :], want[9, :])


@pytest.mark.parametrize("name", ["so", "so-cast", "t-so-cast", "gzip"])
def test_writes_store_what_the_reference_stores(name, device):
    p = Packed(CHAINS[name])
    host = p.host_store(_data(), delete=("c/1/1", "c/2/0"))
    store, arr = p.open(host, device)
    new = _data(seed=1)
    for sel in ((slice(0, 20), slice(0, 13)),     # every chunk complete
                (slice(2, 7), slice(3, 11)),      # partial, existing chunks: untouched elements re-encoded
                (slice(9, 15), slice(9, 12))):    # partial, into a missing chunk
        def do(sel=sel):
            arr[sel] = new[sel]
        p.check_write(store, arr, _mask(SHAPE, sel), new, do)


def test_a_chunk_that_encodes_to_the_fill_is_stored_and_the_fill_is_elided(device):
    p = Packed(CHAINS["so-cast"])
    host = p.host_store(_data())
    store, arr = p.open(host, device)
    # 0.26 != fill but (0.26 + 2.5) * 10 = 27.6 rounds to 28 = encode(fill) = rint(27.5)
    near = np.full((8, 8), 0.26, np.float32)
    assert p.encode(near)[0].tolist() == np.full((8, 8), p.sfill).tolist()
    sel = (slice(0, 8), slice(0, 8))
    new = np.full(SHAPE, 0.26, np.float32)

    def do():
        arr[sel] = near
    p.check_write(store, arr, _mask(SHAPE, sel), new, do)
    assert "c/0/0" in store.to_dict()
    arr[...] = np.float32(FILL)  # the fill everywhere: every key goes
    assert _chunk_bytes(store.to_dict()) == {}


def test_a_corrupted_crc_on_the_merge_read_stores_nothing(device):
    p = Packed(CHAINS["so-cast"])
    host = p.host_store(_data())
    raw = bytearray(host["c/0/0"])
    raw[5] ^= 0x40
    host["c/0/0"] = bytes(raw)
    store, arr = p.open(host, device)
    before = _chunk_bytes(store.to_dict())
    with pytest.raises(ValueError, match="checksum"):
        arr[2:5, 2:12] = np.float32(1.0)
    assert _chunk_bytes(store.to_dict()) == before


def test_value_errors_raise_and_store_nothing(device):
    # out of range on a write: (40000 + 2.5) * 10 does not fit int16
    p = Packed(CHAINS["so-cast"])
    store, arr = p.open(p.host_store(_data()), device)
    before = _chunk_bytes(store.to_dict())
    bad = _data(seed=2)
    bad[4, 4] = 40000.0
    with pytest.raises(ValueError, match="cast_value.*out of range"):
        arr[...] = bad
    with pytest.raises(ValueError, match="cast_value.*not a number"):
        arr[0:2, 0:2] = np.float32(np.nan)
    assert _chunk_bytes(store.to_dict()) == before
    # a non-exact division on a read: int16 with scale 3, a stored 7
    q = Packed([{"name": "scale_offset", "configuration": {"offset": 1, "scale": 3}}, BYTES_LE], adt="int16", fill=0)
    stored = np.full(SHAPE, 6, np.int16)
    stored[17, 12] = 7
    host = {}
    O.write(host, q.smeta, (Ellipsis,), stored)
    store, arr = q.open(host, device)
    with pytest.raises(ValueError, match="scale_offset decode produced a non-zero remainder"):
        arr[...]
    assert _same(arr[0:16, 0:8], np.full((16, 8), 3, np.int16))
    before = _chunk_bytes(store.to_dict())
    with pytest.raises(ValueError, match="scale_offset produced a value outside the range of dtype int16"):
        arr[0:3, 0:3] = np.int16(20000)
    assert _chunk_bytes(store.to_dict()) == before


def test_orthogonal_coordinate_and_mask_selections(device):
    p = Packed(CHAINS["so-cast"])
    host = p.host_store(_data(), delete=("c/1/0",))
    store, arr = p.open(host, device)
    want = p.expected_read(host)
    rows, cols = np.array([0, 3, 9, 19, 12]), np.array([1, 12, 5])
    assert _same(arr.oindex[rows, cols], want[np.ix_(rows, cols)])
    r, c = np.array([0, 19, 8, 15, 3]), np.array([0, 12, 7, 2, 3])
    assert _same(arr.vindex[r, c], want[r, c])
    mask = want > 100
    mask[10, 3] = True
    assert _same(arr[mask], want[mask])
    new = _data(seed=3)
    om = np.zeros(SHAPE, bool)
    om[np.ix_(rows, cols)] = True

    def do_o():
        arr.oindex[rows, cols] = new[np.ix_(rows, cols)]
    p.check_write(store, arr, om, new, do_o)
    vm = np.zeros(SHAPE, bool)
    vm[r, c] = True

    def do_v():
        arr.vindex[r, c] = new[r, c]
    p.check_write(store, arr, vm, new, do_v)

    def do_m():
        arr[mask] = new[mask]
    p.check_write(store, arr, mask, new, do_m)


def test_host_and_strided_device_outs(device):
    import torch

    p = Packed(CHAINS["so-cast"])
    host = p.host_store(_data(), delete=("c/0/1",))
    store, arr = p.open(host, device)
    want = p.expected_read(host)
    out = np.full(SHAPE, -7, np.float32)
    arr.get(Ellipsis, out=out)
    assert _same(out, want)
    big = torch.full((20, 40), -7.0, dtype=torch.float32, device=device)
    view = big[:, 3:29:2]
    arr.get(Ellipsis, out=view)
    assert _same(view.cpu().numpy(), want)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, 3:29:2] = False
    assert (big[keep] == -7.0).all()


def test_repeated_device_reads_are_replanned_when_the_store_changes(device):
    """A read into a device out keeps its plan and item tables per batch key:
    the second read of a key replays them, a write or a delete in between
    makes the next read plan again.  Every result against the oracle."""
    import torch

    p = Packed(CHAINS["so-cast"])
    host = p.host_store(_data(), delete=("c/1/0",))
    store, arr = p.open(host, device)
    want = p.expected_read(host)
    kept = arr.codec_pipeline._aux
    for rep in range(3):  # a miss, then hits of the same key (another out of the same geometry too)
        out = torch.full(SHAPE, -7.0, dtype=torch.float32, device=device)
        arr.get(Ellipsis, out=out)
        assert _same(out.cpu().numpy(), want), rep
        assert len(kept["value_reads"]) == 1
    first = next(iter(kept["value_reads"].values()))
    out = torch.full(SHAPE, -7.0, dtype=torch.float32, device=device)
    arr.get(Ellipsis, out=out)
    assert next(iter(kept["value_reads"].values())) is first  # replayed, not planned again
    sub = torch.full((6, 5), -7.0, dtype=torch.float32, device=device)  # another key
    arr.get((slice(7, 13), slice(5, 10)), out=sub)
    arr.get((slice(7, 13), slice(5, 10)), out=sub)
    assert _same(sub.cpu().numpy(), want[7:13, 5:10])
    # a write in between: chunks re-encoded, one created
    new = _data(seed=4)
    arr[6:12, 2:11] = new[6:12, 2:11]
    want2 = p.expected_read(_chunk_bytes(store.to_dict()))
    assert not _same(want2, want)
    arr.get(Ellipsis, out=out)
    assert _same(out.cpu().numpy(), want2)
    arr.get(Ellipsis, out=out)
    assert _same(out.cpu().numpy(), want2)
    arr.get((slice(7, 13), slice(5, 10)), out=sub)
    assert _same(sub.cpu().numpy(), want2[7:13, 5:10])
    # a delete in between: the chunk reads as the array fill
    store.delete_sync("c/0/1")
    want3 = p.expected_read(_chunk_bytes(store.to_dict()))
    assert (want3[0:8, 8:13] == np.float32(FILL)).all()
    arr.get(Ellipsis, out=out)
    assert _same(out.cpu().numpy(), want3)


def test_a_value_error_on_a_kept_read_then_a_clean_read(device):
    import torch

    q = Packed([{"name": "scale_offset", "configuration": {"offset": 1, "scale": 3}}, BYTES_LE], adt="int16", fill=0)
    stored = np.full(SHAPE, 6, np.int16)
    host = {}
    O.write(host, q.smeta, (Ellipsis,), stored)
    store, arr = q.open(host, device)
    out = torch.zeros(SHAPE, dtype=torch.int16, device=device)
    arr.get(Ellipsis, out=out)  # planned and kept
    arr.get(Ellipsis, out=out)
    assert _same(out.cpu().numpy(), np.full(SHAPE, 3, np.int16))
    bad = stored.copy()
    bad[17, 12] = 7
    badhost = {}
    O.write(badhost, q.smeta, (Ellipsis,), bad)
    store.set_sync("c/2/1", badhost["c/2/1"])
    for _ in range(2):  # the error is reported by every read, not only the first
        with pytest.raises(ValueError, match="scale_offset decode produced a non-zero remainder"):
            arr.get(Ellipsis, out=out)
    sub = torch.zeros((16, 8), dtype=torch.int16, device=device)
    arr.get((slice(0, 16), slice(0, 8)), out=sub)  # chunks without the bad element
    assert _same(sub.cpu().numpy(), np.full((16, 8), 3, np.int16))
    store.set_sync("c/2/1", host["c/2/1"])
    for _ in range(2):  # clean again, and no error word left over from the failed reads
        out.zero_()
        arr.get(Ellipsis, out=out)
        assert _same(out.cpu().numpy(), np.full(SHAPE, 3, np.int16))


def test_zarr_json_round_trips_both_codecs(device):
    cast = {"name": "cast_value", "configuration": {
        "data_type": "int16", "rounding": "towards-zero", "out_of_range": "clamp",
        "scalar_map": {"encode": [["NaN", -999]], "decode": [[-999, "NaN"]]}}}
    p = Packed([SO, cast, BYTES_LE])
    store, arr = p.open({}, device)
    again = zarr_hip.Array.open(store)
    names = [c.to_dict() for c in again.metadata.codecs]
    assert names[0] == {"name": "scale_offset", "configuration": {"offset": -2.5, "scale": 10}}
    assert names[1]["configuration"]["rounding"] == "towards-zero"
    data = _data()
    data[3, 3] = np.nan
    data[4, 4] = 1e9
    again[...] = data
    got = again[...]
    assert np.isnan(got[3, 3]) and got[4, 4] == np.float32(32767 / 10.0 - 2.5)


# ------------------------------------------------------------------ sharded
def _sharded(index_location):
    inner = [SO, CAST16, BYTES_LE, CRC]
    return {"name": "sharding_indexed", "configuration": {
        "chunk_shape": [8, 8], "codecs": inner, "index_codecs": [BYTES_LE, CRC], "index_location": index_location}}


@pytest.mark.parametrize("index_location", ["end", "start"])
def test_sharded_reads_with_elided_inner_chunks_and_an_absent_shard(index_location, device):
    shape = (40, 30)
    sh = _sharded(index_location)
    p = Packed([SO, CAST16], shape=shape, chunks=(16, 16))
    stored_sh = dict(sh, configuration=dict(sh["configuration"], codecs=[BYTES_LE, CRC]))
    smeta = O.ArrayMeta(shape, (16, 16), p.sdt, p.sfill, codecs=[stored_sh])  # elides inner chunks of sfill
    data = _data(shape)
    data[0:8, 8:16] = FILL     # inner chunk (0, 1) of shard (0, 0): encodes to sfill everywhere -> elided
    data[24:32, 16:24] = 0.26  # inner chunk (1, 0) of shard (1, 1): != fill, but encodes to sfill -> elided too
    stored, err = p.encode(data)
    assert err == 0
    host = {}
    O.write(host, smeta, (Ellipsis,), stored)
    del host["c/2/0"]          # a whole shard absent
    want, err = p.decode(O.read(host, smeta))
    assert err == 0
    want[0:8, 8:16] = FILL     # elided inner chunks and the absent shard read as the ARRAY fill
    want[24:32, 16:24] = FILL
    want[32:40, 0:16] = FILL
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, (16, 16), "float32", FILL, codecs=[sh])
    assert _same(arr[...], want)
    assert _same(arr[5:37:3, 2:29], want[5:37:3, 2:29])
    assert _same(arr[20:36, 10:20], want[20:36, 10:20])
    with pytest.raises(NotImplementedError, match="scale_offset.*writes"):
        arr[0:4, 0:4] = np.float32(1)


def test_sharded_production_rows_write_the_status_the_map_reads(device):
    """128^3 shards of 64^3 int16 inner chunks decoded to float32, one inner
    chunk elided: the production row kernels write the statuses.  Expected by
    numpy float32 arithmetic (x / scale + offset, the specification itself)."""
    shape = (128, 128, 128)
    inner = [SO, CAST16, BYTES_LE, CRC]
    sh = {"name": "sharding_indexed", "configuration": {
        "chunk_shape": [64, 64, 64], "codecs": inner, "index_codecs": [BYTES_LE, CRC], "index_location": "end"}}
    stored_sh = dict(sh, configuration=dict(sh["configuration"], codecs=[BYTES_LE, CRC]))
    sfill = np.int16(28)  # rint((0.25 + 2.5) * 10) = rint(27.5) = 28
    smeta = O.ArrayMeta(shape, shape, np.dtype("int16"), sfill, codecs=[stored_sh])
    rng = np.random.default_rng(5)
    stored = rng.integers(-30000, 30000, shape).astype(np.int16)
    stored[64:, 0:64, 64:] = sfill
    host = {}
    O.write(host, smeta, (Ellipsis,), stored)
    want = (stored.astype(np.float32) / np.float32(10)) + np.float32(-2.5)
    want[64:, 0:64, 64:] = FILL
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, shape, "float32", FILL, codecs=[sh])
    assert _same(arr[...], want)


def test_two_devices(device):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    from zarr_hip.pipeline import HipCodecPipeline

    p = Packed(CHAINS["so-cast"], shape=(64, 64), chunks=(8, 8))
    host = p.host_store(_data((64, 64)), delete=("c/3/3",))
    store, arr = p.open(host, device)
    arr.codec_pipeline = HipCodecPipeline.from_codecs(arr.metadata.codecs, devices=(0, 1)) \
        .evolve_from_array_spec(arr.spec)
    assert _same(arr[...], p.expected_read(host))
