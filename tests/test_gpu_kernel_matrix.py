"""The production row kernels, pinned by name: which kernel a geometry takes
(launch_decode / launch_encode choose by units per launch, units per chunk,
the interleave S, item size, byte swap and the affine flag), every 4 KiB step
of a chunk reaching its CRC verdict, and ragged heads (chunks that end on a
4 KiB but not on a 32 KiB boundary: the first steps of the end-aligned frame
lie before the chunk start and must load, store and contribute nothing).

Each table row names its geometry AND the kernel it must take, so a change
of a selection rule fails a row here and has to be acknowledged in the table.
Shipped library only: nothing here forces a tuning arm.

Units are 32 KiB, steps 4 KiB; nseg = units per chunk.  The rules as of this
table (csrc/decode.hip launch_decode -> launch_row_units, csrc/capi.cpp
il_tiles / il_widest):
  nseg % 8 == 0 (interleaved layouts; S = 32 / 16 / 8, the widest that tiles)
      launch <= 512 units, nseg <= 32, fewer chunks than CUs   k_decode_ilh
      launch <= 512 units otherwise (nseg <= 256)              k_decode_ilw512
      launch  > 512 units                                      k_decode_il
  otherwise, nseg > 32                                         k_decode_duo
  otherwise                                                    k_decode_pair
and (csrc/encode.hip launch_encode -> launch_encode_rows) nseg % 8 == 0 and
nseg <= 32 k_encode_il,
every other row layout of more than 16 KiB k_encode_pair."""

from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_decode import BE, CRC, LE, SHARD, _corrupt, _data  # noqa: F401  (SHARD: the shared codec helpers)

pytestmark = pytest.mark.gpu

STEP = 4096
FILL = 3

# id, chunk shape, dtype, endian, chunk grid, kernel, affine (whole reads take
# the plan's affine destinations: exact with the row map zeroed), ragged,
# in the every-step sweep
Row = namedtuple("Row", "id chunk dtype endian grid kernel affine ragged sweep")

DECODE_ROWS = [
    # -- k_decode_il: more than 512 units per launch.  1 MiB chunks (nseg 32, S = 32), 17 chunks = 544 units,
    #    once per instantiation select_il_kernel has for CRC layouts (the last dim keeps the chunk at 1 MiB)
    Row("il_s32-u8", (64, 64, 256), "uint8", LE, (1, 1, 17), "k_decode_il", True, False, False),
    Row("il_s32-i16le", (64, 64, 128), "int16", LE, (1, 1, 17), "k_decode_il", True, False, False),
    Row("il_s32-i16be", (64, 64, 128), "int16", BE, (1, 1, 17), "k_decode_il", True, False, False),
    Row("il_s32-f32le", (64, 64, 64), "float32", LE, (1, 1, 17), "k_decode_il", True, False, True),
    Row("il_s32-f32be", (64, 64, 64), "float32", BE, (1, 1, 17), "k_decode_il", True, False, False),
    Row("il_s32-f64le", (64, 64, 32), "float64", LE, (1, 1, 17), "k_decode_il", True, False, False),
    Row("il_s32-f64be", (64, 64, 32), "float64", BE, (1, 1, 17), "k_decode_il", True, False, False),
    # 512 KiB: nseg 16, S = 16; 33 chunks = 528 units
    Row("il_s16", (64, 64, 64), "int16", BE, (1, 1, 33), "k_decode_il", True, False, True),
    # 256 KiB: nseg 8, S = 8, one group; 65 chunks = 520 units
    Row("il_s8", (32, 32, 32), "float64", LE, (1, 1, 65), "k_decode_il", True, False, True),
    # 768 KiB: nseg 24, S = 8, three groups; 22 chunks = 528 units
    Row("il_s8_g3", (48, 128, 128), "uint8", LE, (1, 1, 22), "k_decode_il", True, False, True),
    # more than 32 workgroups per chunk: publish_il's counted branch (xor, then count; words at ws + 4 c)
    # 1.25 MiB: nseg 40, S = 8; 13 chunks = 520 units
    Row("il_w40", (40, 64, 64), "float64", BE, (1, 1, 13), "k_decode_il", True, False, True),
    # 1.5 MiB: nseg 48, S = 16; 11 chunks = 528 units
    Row("il_w48", (48, 128, 128), "int16", LE, (1, 1, 11), "k_decode_il", True, False, True),
    # 2 MiB: nseg 64, S = 32; 9 chunks = 576 units
    Row("il_w64", (128, 64, 64), "float32", BE, (1, 1, 9), "k_decode_il", True, False, True),
    # ragged heads: 252 KiB (nseg 8, S = 8, lo_frame -4096: workgroup 0's first step is empty), 65 chunks = 520
    # units; 1000 KiB (nseg 32, S = 32, lo_frame -24576: the first step of workgroups 0-5), 17 chunks = 544
    # units.  A chunk that does not end on a unit boundary has no affine form (plan_affine): the map stays.
    Row("il_ragged8", (63, 32, 32), "float32", LE, (1, 1, 65), "k_decode_il", False, True, True),
    Row("il_ragged32", (250, 32, 32), "float32", LE, (1, 1, 17), "k_decode_il", False, True, True),
    # 768 KiB chunks of three steps per plane, TWO chunks along dim 1: a step's destination is
    # (st / 3) * plane + (st % 3) * 16 rows with plane != 3 * 16 rows, which no power-of-two split
    # expresses, so the launch keeps the row map under ZHIP_DF_WHOLE.  (With all 22 chunks along the last
    # dim the out's plane stride is 48 rows, the map is linear in the step and the plan IS affine; the
    # grid 1 x 2 x 11 is the nearest geometry that reaches the map-kept branch.)  528 units.
    Row("il_nonaff", (64, 48, 64), "float32", LE, (1, 2, 11), "k_decode_il", False, False, True),
    # -- k_decode_ilh: at most 512 units, nseg <= 32, fewer chunks than CUs (half units, look-back finalizer)
    Row("ilh_u8", (64, 64, 256), "uint8", LE, (1, 1, 4), "k_decode_ilh", True, False, False),
    Row("ilh_f64be", (32, 64, 64), "float64", BE, (1, 1, 4), "k_decode_ilh", True, False, False),
    Row("ilh_ragged", (63, 32, 32), "float32", LE, (1, 1, 4), "k_decode_ilh", False, True, True),
    # -- k_decode_ilw512: at most 512 units, nseg 64 > 32 (2 MiB chunks), 128 units
    Row("ilw_w64-f32le", (512, 1024), "float32", LE, (1, 2), "k_decode_ilw512", True, False, True),
    Row("ilw_w64-i16be", (1024, 1024), "int16", BE, (1, 2), "k_decode_ilw512", True, False, False),
    # -- k_decode_duo: nseg 33 (1056 KiB: more than 32 units, not a multiple of 8), 3 chunks = 99 units, an
    #    odd count: the last workgroup's second half is idle (32 KiB planes kept by the last dim)
    Row("duo_33-f32le", (33, 64, 128), "float32", LE, (1, 1, 3), "k_decode_duo", False, False, True),
    Row("duo_33-i16be", (33, 64, 256), "int16", BE, (1, 1, 3), "k_decode_duo", False, False, False),
    Row("duo_33-u8", (33, 64, 512), "uint8", LE, (1, 1, 3), "k_decode_duo", False, False, False),
    Row("duo_33-f64be", (33, 64, 64), "float64", BE, (1, 1, 3), "k_decode_duo", False, False, False),
    # 1036 KiB: nseg 33 with a ragged head (lo_frame -20480: five empty steps in the first unit)
    Row("duo_ragged", (259, 32, 32), "float32", LE, (1, 1, 3), "k_decode_duo", False, True, True),
    # -- k_decode_pair: 96 KiB (3 units, 15 in the launch: odd); 988 KiB ragged (247 steps, 31 units, 155)
    Row("pair_3", (3, 64, 512), "uint8", LE, (1, 1, 5), "k_decode_pair", False, False, False),
    Row("pair_31r", (247, 32, 16), "float64", BE, (1, 1, 5), "k_decode_pair", False, True, False),
]

# the kernels that have an affine instantiation (select_il / ilh / ilw_kernel's aff)
AFF_KERNELS = ("k_decode_il", "k_decode_ilh", "k_decode_ilw512")


def _kernel():
    from zarr_hip import _native as N

    return N.lib().zhip_last_kernel().decode()


class _Case:
    """One row's array, written by the oracle with chunk 1 dropped (a missing
    chunk takes the fill through the same launch), uploaded to the device."""

    def __init__(self, device, row):
        import zarr_hip

        self.row = row
        self.shape = tuple(c * g for c, g in zip(row.chunk, row.grid))
        codecs = [row.endian, CRC]
        self.meta = O.ArrayMeta(self.shape, row.chunk, np.dtype(row.dtype), FILL, codecs=codecs)
        self.host = {}
        O.write(self.host, self.meta, (Ellipsis,), _data(self.shape, row.dtype))
        # batch items are the chunk grid in C order
        self.keys = ["c/" + "/".join(str(i) for i in ix) for ix in np.ndindex(*row.grid)]
        assert sorted(self.keys) == sorted(self.host)
        self.dropped = 1
        del self.host[self.keys[self.dropped]]
        self.store = zarr_hip.DeviceStore.from_host(self.host, device)
        self.arr = zarr_hip.Array.create(self.store, self.shape, row.chunk, row.dtype, FILL, codecs=codecs)
        self.nbytes = int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize
        assert self.nbytes % STEP == 0 and (self.nbytes % (8 * STEP) != 0) == row.ragged
        self.want = O.read(self.host, self.meta).tobytes()


def _read(arr, sel):
    prog, out = arr.prepare_read(sel)
    prog.launch()
    prog.results()
    return prog, out.cpu().numpy().tobytes()


@pytest.mark.parametrize("row", DECODE_ROWS, ids=[r.id for r in DECODE_ROWS])
def test_decode_row(device, row):
    """A whole read takes the row's kernel (by name) under ZHIP_DF_WHOLE and is
    bit-exact with the oracle, a missing chunk filled by the same launch --
    affine rows with the row map zeroed on the device, so the destinations can
    only have come from the plan's affine form; a window that cuts every dim
    but the last and starts inside the first chunk never sets ZHIP_DF_WHOLE and
    is exact; ragged rows also read their first and their last chunk alone."""
    from zarr_hip import _native as N

    c = _Case(device, row)
    prog, out = c.arr.prepare_read((Ellipsis,))
    assert prog.tables.rows and prog.data.p_rowmap is not None
    assert prog.data.flags & N.DF_WHOLE
    if row.affine:
        assert row.kernel in AFF_KERNELS
        prog.data.d_rowmap.zero_()
    prog.launch()
    prog.results()
    assert _kernel() == row.kernel
    assert out.cpu().numpy().tobytes() == c.want
    nd = len(c.shape)
    win = tuple(slice(1 + (d if c.shape[d] > 8 else 0), c.shape[d] - (2 if c.shape[d] > 4 else 1))
                for d in range(nd - 1)) + (slice(None),)
    prog, got = _read(c.arr, win)
    assert not prog.data.flags & N.DF_WHOLE
    assert got == np.ascontiguousarray(O.read(c.host, c.meta, win)).tobytes()
    if row.ragged:
        cl = row.chunk[-1]
        for lo in (0, c.shape[-1] - cl):
            one = (slice(None),) * (nd - 1) + (slice(lo, lo + cl),)
            _, got = _read(c.arr, one)
            assert got == np.ascontiguousarray(O.read(c.host, c.meta, one)).tobytes()


SWEEP_ROWS = [r for r in DECODE_ROWS if r.sweep]


def _flip(store, offs, bits):
    """XOR the bytes at arena offsets `offs` with `bits`: one device operation."""
    import torch

    buf = store.arena.buf
    idx = torch.tensor(offs, dtype=torch.int64, device=buf.device)
    buf[idx] = buf[idx] ^ torch.tensor(bits, dtype=torch.uint8, device=buf.device)


@pytest.mark.parametrize("row", SWEEP_ROWS, ids=[r.id for r in SWEEP_ROWS])
def test_every_step_reaches_the_verdict(device, row):
    """One flipped bit in EVERY 4 KiB step of a chunk, and in its trailer, is
    reported: per round chunk i of the present chunks gets step round * n + i
    (counted from the chunk's first byte -- no model of which workgroup owns
    which step), at in-step byte 16 ((7 st) % 256) + st % 16 so lanes and words
    vary; the launch sets ST_CRC_MISMATCH in the error word and in exactly the
    hit chunks' statuses, every other present chunk is ST_OK, the missing one
    ST_MISSING.  The restored bytes then read exactly twice (no stale
    publication word), and one corrupted chunk raises the reference's
    message."""
    from zarr_hip import _native as N

    c = _Case(device, row)
    prog, out = c.arr.prepare_read((Ellipsis,))
    prog.launch()
    prog.results()
    assert _kernel() == row.kernel
    assert out.cpu().numpy().tobytes() == c.want
    d = prog.data
    item_of = np.asarray(prog.tables.item_of_chunk)
    assert d.n == len(c.keys) and sorted(item_of) == list(range(d.n))
    present = [j for j in range(d.n) if item_of[j] != c.dropped]  # table entries of the present chunks
    base = [c.store.placement(c.keys[item_of[j]])[0] for j in present]
    n_steps, n = c.nbytes // STEP, len(present)
    missing = np.array([item_of[j] == c.dropped for j in range(d.n)])
    rounds = []
    for rnd in range(-(-n_steps // n)):
        hit = [(i, rnd * n + i) for i in range(n) if rnd * n + i < n_steps]
        rounds.append(([present[i] for i, _ in hit],
                       [base[i] + STEP * st + 16 * ((7 * st) % 256) + st % 16 for i, st in hit],
                       [1 << (st % 8) for _, st in hit]))
    covered = {}
    for ents, offs, _ in rounds:
        for j, o in zip(ents, offs):
            covered.setdefault(j, set()).add((o - base[present.index(j)]) // STEP)
    assert set().union(*covered.values()) == set(range(n_steps))  # every step index was hit
    rounds.append((present, [b + c.nbytes + i % 4 for i, b in enumerate(base)], [0x20] * n))  # the trailers
    for ents, offs, bits in rounds:
        _flip(c.store, offs, bits)
        d.reset_errflag()
        prog.launch()
        err = d.errflag()
        st = d.statuses()
        _flip(c.store, offs, bits)  # restored
        codes = st["code"]
        assert err & (1 << N.ST_CRC_MISMATCH)
        assert sorted(np.nonzero(codes == N.ST_CRC_MISMATCH)[0]) == sorted(ents)
        assert (codes[missing] == N.ST_MISSING).all()
        assert ((codes == N.ST_OK) | (codes == N.ST_CRC_MISMATCH) | missing).all()
    d.reset_errflag()
    for _ in range(2):
        prog.launch()
        prog.results()
        assert out.cpu().numpy().tobytes() == c.want
    # the reference's message, once per row
    host = dict(c.host)
    key = c.keys[item_of[present[-1]]]
    _corrupt(c.store, host, key, at=c.nbytes - 5000)
    with pytest.raises(ValueError) as want:
        O.read(host, c.meta)
    prog.launch()
    with pytest.raises(ValueError) as got:
        prog.results()
    assert str(got.value) == str(want.value)
    _corrupt(c.store, host, key, at=c.nbytes - 5000)
    assert host == c.host
    prog.launch()
    prog.results()
    assert out.cpu().numpy().tobytes() == c.want


# ---- encode rows: id, chunk shape, dtype, endian, kernel
EncRow = namedtuple("EncRow", "id chunk dtype endian kernel")

ENCODE_ROWS = [
    # k_encode_il: nseg % 8 == 0 and nseg <= 32
    EncRow("enc_il_s16", (64, 64, 128), "uint8", LE, "k_encode_il"),          # 512 KiB: nseg 16, S = 16, one half
    EncRow("enc_il_g3", (48, 64, 64), "float32", BE, "k_encode_il"),          # 768 KiB: nseg 24, S = 8, halves 16 + 8
    EncRow("enc_il_ragged8", (63, 32, 16), "float64", BE, "k_encode_il"),     # 252 KiB: one empty head step
    EncRow("enc_il_ragged32", (250, 32, 32), "float32", LE, "k_encode_il"),   # 1000 KiB: six, S = 32
    # k_encode_pair with the flags ORed after a memset (odd nseg, or nseg > 32)
    EncRow("enc_pair_33", (33, 64, 256), "int16", BE, "k_encode_pair"),       # 1056 KiB: nseg 33
    EncRow("enc_pair_64", (128, 64, 64), "float32", LE, "k_encode_pair"),     # 2 MiB: tiles S = 32 but nseg 64 > 32
    EncRow("enc_pair_3r", (23, 32, 16), "float64", LE, "k_encode_pair"),      # 92 KiB ragged: nseg 3
]


def _stores_equal(dev_store, host):
    got = {k: v for k, v in dev_store.to_dict().items() if not k.endswith("zarr.json")}
    assert sorted(got) == sorted(host), sorted(set(got) ^ set(host))[:10]
    for k in host:
        assert got[k] == host[k], f"bytes differ for {k}"
    return got


@pytest.mark.parametrize("row", ENCODE_ROWS, ids=[r.id for r in ENCODE_ROWS])
def test_encode_row(device, row):
    """Five chunks along the last dim -- one entirely fill (elided: no key), one
    fill except its FIRST element, one fill except its LAST (the non-empty
    flag from a single wave at either end of the frame; on ragged chunks from
    the step next to the empty head), two of data -- written whole, then a
    partial write that merges into every chunk, then a write into ONE interior
    chunk: after each, the row's kernel ran last and the store equals the
    oracle's key by key (after the last, every other key byte-identical to
    before: a store before a chunk's start would land in a neighbour); the
    array then reads back exactly."""
    import zarr_hip

    dt = np.dtype(row.dtype)
    fill = 0
    cs = row.chunk
    shape = cs[:-1] + (5 * cs[-1],)
    codecs = [row.endian, CRC]
    meta = O.ArrayMeta(shape, cs, dt, fill, codecs=codecs)
    data = _data(shape, row.dtype, 7)
    cl = cs[-1]
    data[..., 0: 3 * cl] = fill
    one = -0.0 if dt.kind == "f" else 1          # -0.0: bitwise != fill, the chunk is kept
    data[(0,) * (len(cs) - 1) + (cl,)] = one                           # chunk 1: its first element
    data[tuple(s - 1 for s in cs[:-1]) + (3 * cl - 1,)] = one          # chunk 2: its last element
    store = zarr_hip.DeviceStore(device)
    arr = zarr_hip.Array.create(store, shape, cs, row.dtype, fill, codecs=codecs)
    host = {}

    def write(sel, val):
        O.write(host, meta, sel, val)
        arr[sel] = val
        assert _kernel() == row.kernel
        return _stores_equal(store, host)

    got = write((Ellipsis,), data)
    lead = "c/" + "0/" * (len(cs) - 1)
    assert sorted(got) == [lead + str(i) for i in (1, 2, 3, 4)]       # chunk 0 elided
    part = tuple(slice(1, s - 2) for s in shape[:-1]) + (slice(3, shape[-1] - 5),)
    before = write(part, _data(tuple(s.stop - s.start for s in part), row.dtype, 8))
    assert len(before) == 5
    inner = tuple(slice(2, s - 1) for s in cs[:-1]) + (slice(3 * cl + 1, 4 * cl - 3),)
    after = write(inner, _data(tuple(s.stop - s.start for s in inner), row.dtype, 9))
    for k in before:
        assert (after[k] == before[k]) == (k != lead + "3"), k
    assert arr[...].tobytes() == O.read(host, meta).tobytes()
    assert _kernel().startswith("k_decode_")


def test_persistent_and_tile_encodes_report_their_names(device):
    """launch_encode names the persistent k_encode (layouts without whole-row
    units) and k_encode_tile (transposed layouts whose edge chunks take prefix
    selections), so a name assertion after them does not read the previous
    launch's: each write follows a read, whose decode left another name."""
    import zarr_hip
    from test_gpu_decode import T

    for shape, chunks, codecs, kname in [((40, 33, 20), (16, 16, 8), [LE, CRC], "k_encode"),
                                         ((100, 72, 48), (64, 48, 32), [T((2, 1, 0)), LE, CRC], "k_encode_tile")]:
        meta = O.ArrayMeta(shape, chunks, np.dtype("float32"), 0.0, codecs=codecs)
        store = zarr_hip.DeviceStore(device)
        arr = zarr_hip.Array.create(store, shape, chunks, "float32", 0.0, codecs=codecs)
        data = _data(shape, "float32")
        host = {}
        O.write(host, meta, (Ellipsis,), data)
        for _ in range(2):
            arr[...] = data
            assert _kernel() == kname
            _stores_equal(store, host)
            assert arr[...].tobytes() == O.read(host, meta).tobytes()
            assert _kernel().startswith("k_decode")
