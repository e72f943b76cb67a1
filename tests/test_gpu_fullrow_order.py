"""The full-row form of k_decode_il (decode_rows.hip ilx_body): the four waves
of a workgroup on four consecutive chunks of the batch, each streaming four
8 KiB spans of its own chunk in passes of eight blocks, one publication per
wave.  FUSED launches take it (launch_decode_multi) when every member is a
k_decode_il launch of more than 512 units whose chunk count is a multiple of
four; a launch alone keeps the interleaved form.  It is reported as
"k_decode_il" and recognised here by its grid (a quarter of the units).  So
every read below is planned twice and the two programs run as one fused
launch of a ReadGraph; both outs are checked.

What can go wrong that the interleaved form cannot: a wave using a neighbour
wave's chunk (source, destination, trailer, status or publication line), a
pass using another pass's span or destinations, a Horner chain broken at a
pass boundary, and a group of four that is not four neighbours in the out.
The smallest shapes are just past 512 units: 20 chunks of 1 MiB (640 units,
five groups of four), 24 sharded inner chunks (768), 40 chunks of 512 KiB."""

import types

import numpy as np
import pytest

import wide_cases as W
from conftest import set_tuning
from oracle import oracle as O
from test_gpu_decode import BE, CRC, LE, SHARD
from test_gpu_wide_offsets import _entry_of, _fill, _ReadCase, backings  # noqa: F401  (backings: a fixture)

pytestmark = pytest.mark.gpu

CHUNK = (64, 64, 64)
NO_XW = 536870912  # zhip_set_tuning(2, ...): kTuneNoXw keeps the interleaved form (tuning build)


def _array(device, shape, chunks, codecs, seed, dtype="float32", drop=()):
    import zarr_hip

    dt = np.dtype(dtype)
    raw = np.random.default_rng(seed).integers(0, 2 ** (8 * dt.itemsize), size=shape,
                                               dtype={2: np.uint16, 4: np.uint32}[dt.itemsize])
    data = raw.view(dt)
    fill = 0.0 if dt.kind == "f" else 0
    meta = O.ArrayMeta(shape, chunks, dt, fill, codecs=codecs)
    host: dict = {}
    O.write(host, meta, (Ellipsis,), data)
    for key in drop:
        del host[key]
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunks, dtype, fill, codecs=codecs)
    return types.SimpleNamespace(arr=arr, store=store, host=host, meta=meta)


def _lib():
    from zarr_hip import _native as N

    return N.lib()


def _pair(x, sel=(Ellipsis,)):
    """`sel` planned twice and captured as ONE fused launch: (programs, outs,
    graph, kernel, grid of the captured launch)."""
    import zarr_hip

    progs, outs = zip(*[x.arr.prepare_read(sel) for _ in range(2)])
    assert progs[0] is not progs[1] and outs[0].data_ptr() != outs[1].data_ptr()
    g = zarr_hip.ReadGraph(list(progs), 2, outs[0].device)
    return progs, outs, g, _lib().zhip_last_kernel().decode(), int(_lib().zhip_last_grid())


def _read(x, sel=(Ellipsis,), prefill=0):
    """One replay of the fused pair: (first program, the outs' bytes (equal), kernel, grid, launches)."""
    progs, outs, g, kernel, grid = _pair(x, sel)
    for o in outs:
        o.fill_(prefill)
    g.replay()
    g.results()
    got = [o.cpu().numpy().tobytes() for o in outs]
    assert got[0] == got[1]
    return progs[0], got[0], kernel, grid, g.launches


def _want(x, sel=(Ellipsis,)):
    return np.ascontiguousarray(O.read(x.host, x.meta, sel)).tobytes()


def _flip(x, key, pos, bit=0x08):
    """The same bit in the device store and in the host copy the oracle reads."""
    ref = x.store.get_sync(key)
    at = pos if pos >= 0 else ref.length + pos
    ref.arena.buf[ref.offset + at] ^= bit
    b = bytearray(x.host[key])
    b[at] ^= bit
    x.host[key] = bytes(b)


@pytest.fixture(scope="module")
def plain(device):
    """(320, 128, 128) float32 in 64^3 chunks: 20 chunks, batch order c/i/j/k
    with k fastest, so group i is the four x- and y-neighbours of slab i."""
    x = _array(device, (320, 128, 128), CHUNK, [LE, CRC], 41)
    x.want = _want(x)
    return x


@pytest.fixture(scope="module")
def sharded(device):
    """(384, 128, 128) in 128^3 shards of 64^3: 24 inner chunks, three shard
    indexes checked in the launch's leading workgroups."""
    xs = [_array(device, (384, 128, 128), (128, 128, 128), [SHARD(CHUNK, [LE, CRC])], 51 + i) for i in range(3)]
    for x in xs:
        x.want = _want(x)
    return xs


# ---- parity

def test_unsharded_parity(device, plain):
    prog, got, kernel, grid, launches = _read(plain)
    assert launches == 1 and kernel == "k_decode_il" and grid == 2 * 640 // 4  # two full-row grids
    assert prog.data.p_rowmap is not None and prog.data.n == 20
    assert got == plain.want


def test_sharded_parity(device, sharded):
    prog, got, kernel, grid, launches = _read(sharded[0])
    assert launches == 1 and kernel == "k_decode_il" and grid == 2 * 768 // 4
    assert prog.index is None and prog.data.n_idx == 3
    assert got == sharded[0].want


def test_a_launch_alone_keeps_the_interleaved_form(device, plain):
    prog, out = plain.arr.prepare_read((Ellipsis,))
    out.zero_()
    prog.launch()
    prog.results()
    assert _lib().zhip_last_kernel().decode() == "k_decode_il" and int(_lib().zhip_last_grid()) == 640
    assert out.cpu().numpy().tobytes() == plain.want


@pytest.mark.tuning
def test_the_interleaved_form_gives_the_same_bytes(device, plain, sharded):
    """kTuneNoXw: the pair is declined and runs as two interleaved launches."""
    set_tuning(2, NO_XW)
    try:
        for x, units in ((plain, 640), (sharded[0], 768)):
            _, got, kernel, grid, launches = _read(x)
            assert launches == 2 and kernel == "k_decode_il" and grid == units  # one workgroup per unit
            assert got == x.want
    finally:
        set_tuning(2, 0)
    _, got, _, grid, launches = _read(plain)
    assert launches == 1 and grid == 320 and got == plain.want


# ---- wave and pass boundaries

# workgroup 13 of a group streams spans 52 .. 55 of each of its four chunks:
# the first and the last 16 bytes of its first span and of its last span
R = 13
EDGES = [8192 * (4 * R) + 5, 8192 * (4 * R + 1) - 3, 8192 * (4 * R + 3) + 7, 8192 * (4 * R + 4) - 9]


def _only_mismatch(prog, chunk):
    from zarr_hip import _native as N

    codes = prog.data.statuses()["code"]
    assert list(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == [chunk]
    assert (codes[np.arange(prog.data.n) != chunk] == N.ST_OK).all()


def _replay_corrupted(device, progs, outs, g, chunk, message):
    """One replay over a corrupted store: both programs report `chunk` alone, with `message`."""
    import torch

    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize(device)
    for p in progs:
        _only_mismatch(p, chunk)
        with pytest.raises(ValueError) as got:
            p.results()
        assert str(got.value) == message
        p.data.reset_errflag()


@pytest.mark.parametrize("w", [0, 1, 2, 3])
def test_each_wave_reports_its_own_chunk(device, plain, w):
    """Group 2 (slab 2, the middle of the batch): a bit flipped at each edge
    of wave w's first and last span is a CRC mismatch of chunk 8 + w alone,
    with the reference's message; every byte outside that chunk is exact."""
    x = plain
    key = f"c/2/{w >> 1}/{w & 1}"
    progs, outs, g, _, grid = _pair(x)
    assert g.launches == 1 and grid == 320
    want = np.frombuffer(x.want, np.uint32).reshape(320, 128, 128)
    mine = (slice(128, 192), slice(64 * (w >> 1), 64 * (w >> 1) + 64), slice(64 * (w & 1), 64 * (w & 1) + 64))
    for at in EDGES:
        _flip(x, key, at)
        try:
            with pytest.raises(ValueError) as ref:
                O.read(x.host, x.meta, (slice(128, 129), mine[1], mine[2]))
            _replay_corrupted(device, progs, outs, g, 8 + w, str(ref.value))
            for o in outs:
                diff = o.cpu().numpy().view(np.uint32) != want
                inside = int(diff[mine].sum())
                diff[mine] = False
                assert not diff.any() and inside == 1  # the flipped word alone
        finally:
            _flip(x, key, at)
    g.replay()
    g.results()
    assert all(o.cpu().numpy().tobytes() == x.want for o in outs)


def test_corrupted_trailer_and_shard_index(device, plain, sharded):
    x = plain
    progs, outs, g, _, _ = _pair(x)
    _flip(x, "c/3/1/0", -2)  # the stored CRC of chunk 14 (wave 2 of group 3)
    try:
        with pytest.raises(ValueError) as ref:
            O.read(x.host, x.meta, (slice(192, 193), slice(64, 65), slice(0, 1)))
        _replay_corrupted(device, progs, outs, g, 14, str(ref.value))
        assert all(o.cpu().numpy().tobytes() == x.want for o in outs)  # the payload is intact
    finally:
        _flip(x, "c/3/1/0", -2)
    s = sharded[1]
    progs, outs, g, _, grid = _pair(s)
    assert g.launches == 1 and grid == 384
    _flip(s, "c/1/0/0", -10, 0x01)  # inside shard 1's index
    try:
        with pytest.raises(ValueError) as ref:
            O.read(s.host, s.meta, (slice(128, 129), slice(0, 1), slice(0, 1)))
        g.replay()
        import torch

        torch.cuda.synchronize(device)
        for p in progs:
            with pytest.raises(ValueError) as got:
                p.results()
            assert str(got.value) == str(ref.value)
            p.data.reset_errflag()
    finally:
        _flip(s, "c/1/0/0", -10, 0x01)
    g.replay()
    g.results()
    assert all(o.cpu().numpy().tobytes() == s.want for o in outs)


# ---- ragged groups (exactness, whichever form serves them)

def test_missing_chunk_inside_a_group(device):
    x = _array(device, (320, 128, 128), CHUNK, [LE, CRC], 43, drop=("c/2/1/0",))
    prog, got, kernel, _, _ = _read(x, prefill=7.0)  # the fill must be written, not left
    assert kernel == "k_decode_il"
    assert [r["status"] for r in prog.results()].count("missing") == 1
    assert got == _want(x)


def test_chunk_count_no_multiple_of_four(device):
    x = _array(device, (704, 128, 64), CHUNK, [LE, CRC], 44)  # 11 x 2 x 1 = 22 chunks, 704 units
    prog, got, kernel, _, _ = _read(x)
    assert prog.data.n == 22 and kernel == "k_decode_il"
    assert got == _want(x)


def test_consecutive_chunks_that_are_not_neighbours(device):
    """The upper half along x of a (1280, 64, 128) array: 20 chunks, every
    other one of the grid, whose groups of four are four slabs stacked along
    z -- never neighbours in a row of the out."""
    y = _array(device, (1280, 64, 128), CHUNK, [LE, CRC], 46)
    sel = (slice(None), slice(None), slice(64, 128))
    prog, got, kernel, _, _ = _read(y, sel)
    assert prog.data.n == 20 and kernel == "k_decode_il"
    assert got == _want(y, sel)


# ---- other element types and selections

def test_big_endian_float32(device):
    x = _array(device, (320, 128, 128), CHUNK, [BE, CRC], 47)
    _, got, kernel, grid, _ = _read(x)
    assert kernel == "k_decode_il" and grid == 320
    assert got == _want(x)


def test_int16_half_mebibyte_chunks(device):
    x = _array(device, (640, 128, 128), CHUNK, [LE, CRC], 48, dtype="int16")  # 40 chunks of 512 KiB, 640 units
    prog, got, kernel, grid, _ = _read(x)
    assert prog.data.n == 40 and kernel == "k_decode_il" and grid == 320
    assert got == _want(x)


@pytest.mark.parametrize("window", [(8, 136), (8, 376)])
def test_partial_windows_over_the_sharded_array(device, sharded, window):
    """[8:136] touches 12 inner chunks (384 units: a small-grid kernel serves
    it); [8:376] cuts the first and the last slab of all 24 (768 units, the
    full-row form through the row map)."""
    x = sharded[2]
    sel = (slice(*window), slice(3, 125), slice(None))
    _, got, kernel, grid, _ = _read(x, sel)
    assert got == _want(x, sel)
    if window == (8, 376):
        assert kernel == "k_decode_il" and grid == 2 * 768 // 4


# ---- fused launches of different arrays

@pytest.mark.parametrize("n", [2, 3])
def test_fused_programs(device, sharded, n):
    """n programs of the full-row form in one launch: exact; an index
    corruption and a payload corruption in the LAST program are that
    program's alone."""
    import torch

    import zarr_hip

    xs = sharded[:n]
    progs, outs = zip(*[x.arr.prepare_read((Ellipsis,)) for x in xs])
    g = zarr_hip.ReadGraph(list(progs), n, device)
    assert g.launches == 1 and _lib().zhip_last_kernel().decode() == "k_decode_il"
    assert int(_lib().zhip_last_grid()) == n * 768 // 4
    for o in outs:
        o.zero_()
    g.replay()
    g.results()
    assert all(o.cpu().numpy().tobytes() == x.want for o, x in zip(outs, xs))
    last = xs[-1]
    for key, pos, bit, where in (("c/2/0/0", -10, 0x01, (slice(256, 257), slice(0, 1), slice(0, 1))),
                                 ("c/1/0/0", 3 * (1 << 20) + 8192 * 30 + 11, 0x08, None)):
        _flip(last, key, pos, bit)
        try:
            if where is None:  # the payload byte's inner chunk: read the whole shard
                where = (slice(128, 256), slice(None), slice(None))
            with pytest.raises(ValueError) as ref:
                O.read(last.host, last.meta, where)
            g.replay()
            torch.cuda.synchronize(device)
            for p in progs[:-1]:
                assert all(r["status"] == "present" for r in p.results())
            with pytest.raises(ValueError) as got:
                progs[-1].results()
            assert str(got.value) == str(ref.value)
            assert all(o.cpu().numpy().tobytes() == x.want for o, x in zip(outs[:-1], xs[:-1]))
        finally:
            _flip(last, key, pos, bit)
            progs[-1].data.reset_errflag()
    g.replay()
    g.results()
    assert all(o.cpu().numpy().tobytes() == x.want for o, x in zip(outs, xs))


def test_four_replicas_twenty_decodes_take_seven_launches(device, sharded):
    """The benchmark's graph shape: [0 1 2] [3 0 1] [2 3 0] ... [2 3]."""
    import zarr_hip

    xs = sharded + [_array(device, (384, 128, 128), (128, 128, 128), [SHARD(CHUNK, [LE, CRC])], 54)]
    progs, outs = zip(*[x.arr.prepare_read((Ellipsis,)) for x in xs])
    g = zarr_hip.ReadGraph(list(progs), 20, device)
    assert g.launches == 7
    g.replay()
    g.results()
    assert all(o.cpu().numpy().tobytes() == x.want for o, x in zip(outs[:3], xs[:3]))


# ---- offsets beyond 2**31 and 2**32

WIDE = W.READ["il"]._replace(id="il_fullrow", n=20)  # tests/test_fullrow_tables.py proves its property on the CPU


def test_wide_offsets(device, backings, plain):  # noqa: F811
    """wide_cases' il geometry with 20 slabs (five groups of four), fused with
    an ordinary program of the same form: slab 9 straddles 2**31, slab 18
    straddles 2**32, slab 19 (missing: filled) lies above; blob 1 straddles
    2**31 and blob 2 2**32 in the arena.  Whole read with the row map zeroed
    (the affine destinations), then a flipped bit on either side of each
    boundary reported for exactly its chunk."""
    import torch

    import zarr_hip
    from zarr_hip import _native as N

    _fill(backings)
    c = _ReadCase(device, backings, WIDE)
    prog, out = c.arr.prepare_read((Ellipsis,), out=c.view)
    assert out is c.view and prog.data.flags & N.DF_WHOLE and prog.data.n == 20
    prog.data.d_rowmap.zero_()
    other, other_out = plain.arr.prepare_read((Ellipsis,))
    g = zarr_hip.ReadGraph([prog, other], 2, device)
    assert g.launches == 1 and _lib().zhip_last_kernel().decode() == "k_decode_il"
    assert int(_lib().zhip_last_grid()) == 320
    g.replay()
    g.results()
    assert c.exact() and other_out.cpu().numpy().tobytes() == plain.want
    blobs = {cell: c.don.host[W.key(c.don.row, cell % 3)] for cell in c.place}
    ranges = W.src_ranges(WIDE, c.place, blobs)
    for bound in (W.B31, W.B32):
        for at in (bound - 1000, bound + 1000):
            (owner,) = [(cell, inner) for cell, inner, a, e in ranges if a <= at < e and inner != "index"]
            j = _entry_of(c, prog, *owner)
            c.store.arena.buf[at] ^= 0x04
            g.replay()
            torch.cuda.synchronize(device)
            c.store.arena.buf[at] ^= 0x04  # restored
            codes = prog.data.statuses()["code"]
            assert list(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == [j]
            prog.data.reset_errflag()
            assert all(r["status"] == "present" for r in other.results())
    g.replay()
    g.results()
    assert c.exact()
