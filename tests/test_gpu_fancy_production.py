"""Orthogonal, coordinate and mask selections over production-size chunks:
the box decode into a scratch slot and the write-back meet the kernels the
project is about, pinned by name per row in the style of
test_gpu_kernel_matrix.py, bit-exact against numpy indexing of a host mirror
(test_gpu_fancy_selection.py does the same on 16^3 chunks, whose boxes only
ever meet k_decode / k_decode_lead4).

The decode kernel of a non-basic read is recorded by wrapping
fancy.SelectTables.launch: when the gather is launched, the last kernel is the
box decode of its sub-batch.  The encode kernel is read after the write.

Shipped library only.  Its transposed full-tile layouts WITH a checksum take
the two-tile forms k_decode_tile2w / k_decode_tileg2w and k_encode_tile2
(launch_decode: the wave-per-tile chains, where the plan built them; with a
checksum the four-tile k_decode_tile4 / k_decode_tileg are arms of the tuning
build, test_gpu_decode.py::test_transpose_tile4w_and_tile4,
::test_transpose_tilegw_and_tileg); k_decode_tileg2w is the kernel whose CRC
verdict reaches the host only through the deferred workspace words.  Without a
checksum the same layouts take k_decode_tile4 / k_decode_tileg and
k_encode_tile4: one row each."""

from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as O
from test_fancy_selection import _np_oindex
from test_gpu_decode import BE, CRC, LE, SHARD, T, _data
from test_gpu_fancy_selection import _np_oindex_set, _same

pytestmark = pytest.mark.gpu

# id, chunk (or shard) shape, dtype, codecs, chunk grid, the kernel of a whole-box decode, of a partial-box
# decode (whole innermost rows, dim 0 cut: the row kernels stay with their map, the tile kernels need full
# chunks and hand over to the general k_decode), of the write-back, sharded
Row = namedtuple("Row", "id chunk dtype codecs grid whole partial encode sharded")

B1 = {"name": "bytes"}

ROWS = [
    # 256 KiB (nseg 8) and 1 MiB (nseg 32) chunks, four of them: at most 512 units, fewer chunks than CUs
    Row("ilh_f64le", (32, 32, 32), "float64", [LE, CRC], (1, 1, 4), "k_decode_ilh", "k_decode_ilh", "k_encode_il", False),
    Row("ilh_f32be", (64, 64, 64), "float32", [BE, CRC], (1, 1, 4), "k_decode_ilh", "k_decode_ilh", "k_encode_il", False),
    # 96 KiB: nseg 3
    Row("pair_u8", (3, 64, 512), "uint8", [B1, CRC], (1, 1, 5), "k_decode_pair", "k_decode_pair", "k_encode_pair", False),
    # 252 KiB: a ragged head
    Row("ilh_ragged", (63, 32, 32), "float32", [LE, CRC], (1, 1, 4), "k_decode_ilh", "k_decode_ilh", "k_encode_il", False),
    # transposed, full 64-row x 256-byte tiles
    Row("tile4", (64, 64, 64), "float32", [T((2, 1, 0)), LE, CRC], (4, 1, 1), "k_decode_tile2w", "k_decode", "k_encode_tile2",
        False),
    # transposed, 80-row tiles grouped by four: the deferred-verdict kernel
    Row("tileg", (96, 80, 80), "float32", [T((2, 1, 0)), LE, CRC], (3, 1, 1), "k_decode_tileg2w", "k_decode", "k_encode_tileg",
        False),
    # the same two layouts without a checksum: the shipped library's four-tile forms (no verdict to defer)
    Row("tile4_nocrc", (64, 64, 64), "float32", [T((2, 1, 0)), LE], (4, 1, 1), "k_decode_tile4", "k_decode", "k_encode_tile4",
        False),
    Row("tileg_nocrc", (96, 80, 80), "float32", [T((2, 1, 0)), LE], (3, 1, 1), "k_decode_tileg", "k_decode", "k_encode_tileg",
        False),
    # zarr's default sharding codecs, 16 KiB inner chunks
    Row("lead4", (128, 128), "int32", [SHARD((64, 64), [LE])], (2, 2), "k_decode_lead4", "k_decode_lead4",
        "k_encode_quad", True),
]
IDS = [r.id for r in ROWS]
# the rows whose chain carries a checksum (the sharded row: its index does)
CRC_ROWS = [r for r in ROWS if CRC in r.codecs or r.sharded]


def _kernel() -> str:
    from zarr_hip import _native as N

    return N.lib().zhip_last_kernel().decode()


class Fix:
    """One row's array: every chunk written by the oracle, on a DeviceStore."""

    def __init__(self, row, device):
        import zarr_hip

        self.row = row
        self.shape = tuple(c * g for c, g in zip(row.chunk, row.grid))
        self.fill = 3
        self.meta = O.ArrayMeta(self.shape, row.chunk, np.dtype(row.dtype), self.fill, codecs=list(row.codecs))
        self.mirror = _data(self.shape, row.dtype, seed=len(row.id))
        self.host: dict = {}
        O.write(self.host, self.meta, (Ellipsis,), self.mirror)
        self.store = zarr_hip.DeviceStore.from_host(self.host, device)
        self.arr = zarr_hip.Array.create(self.store, self.shape, row.chunk, row.dtype, self.fill, codecs=list(row.codecs))
        self.gax = max(range(len(row.grid)), key=lambda d: row.grid[d])  # an axis with more than one chunk
        self.chunk_bytes = int(np.prod(row.chunk)) * np.dtype(row.dtype).itemsize

    def chunk_dict(self) -> dict:
        return {k: bytes(v) for k, v in self.store.to_dict().items() if not k.endswith("zarr.json")}

    # ---- the selections
    def whole_sel(self):
        """oindex: an integer array on dim 0 with the first and the last row of
        every chunk, unsorted and with a repeat; slices elsewhere: every box is
        its whole chunk."""
        c0, g0 = self.row.chunk[0], self.row.grid[0]
        rows = []
        for i in range(g0):
            rows += [i * c0 + c0 - 1, i * c0, i * c0 + c0 // 2]
        rows = rows[::-1] + [rows[0]]
        return (np.array(rows),) + (slice(None),) * (len(self.shape) - 1)

    def partial_sel(self):
        """The rows stay inside [5, n - 7) of each chunk (of a chunk shorter
        than 13: its middle row); whole innermost rows."""
        c0, g0 = self.row.chunk[0], self.row.grid[0]
        lo, hi = (5, c0 - 7) if c0 >= 13 else (c0 // 2, c0 // 2 + 1)
        rows = []
        for i in range(g0):
            rows += [i * c0 + hi - 1, i * c0 + lo, i * c0 + (lo + hi) // 2]
        return (np.array(rows),) + (slice(None),) * (len(self.shape) - 1)

    def points(self, n, seed, distinct=False):
        rng = np.random.default_rng(seed)
        if distinct:
            return np.unravel_index(rng.choice(int(np.prod(self.shape)), n, replace=False), self.shape)
        return tuple(rng.integers(0, s, n) for s in self.shape)

    def first_key(self) -> str:
        return "c/" + "/".join("0" for _ in self.shape)

    def flip(self):
        """One bit of the first chunk (for the sharded row: of its index)."""
        ref = self.store.get_sync(self.first_key())
        n = len(self.host[self.first_key()])
        at = n - 10 if self.row.sharded else n // 2 + 5
        ref.arena.buf[ref.offset + at] ^= 0x10


_READ: dict = {}


def _read_fix(row, device) -> Fix:
    if row.id not in _READ:
        _READ[row.id] = Fix(row, device)
    return _READ[row.id]


@pytest.fixture
def decodes(monkeypatch):
    """The kernel named last at each k_select_copy launch: the box decode of
    that sub-batch."""
    from zarr_hip import fancy

    seen: list = []
    launch = fancy.SelectTables.launch

    def noting(self, a, b, device):
        seen.append(_kernel())
        return launch(self, a, b, device)

    monkeypatch.setattr(fancy.SelectTables, "launch", noting)
    return seen


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_whole_box_read(row, device, decodes):
    f = _read_fix(row, device)
    sel = f.whole_sel()
    got = f.arr.oindex[sel]
    print(row.id, "whole-box decode:", decodes)
    assert _same(got, _np_oindex(f.mirror, list(sel)))
    assert decodes == [row.whole]
    assert _kernel() == "k_select_copy"


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_partial_box_read(row, device, decodes):
    f = _read_fix(row, device)
    sel = f.partial_sel()
    got = f.arr.oindex[sel]
    print(row.id, "partial-box decode:", decodes)
    assert _same(got, _np_oindex(f.mirror, list(sel)))
    assert decodes == [row.partial]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_point_read(row, device, decodes):
    f = _read_fix(row, device)
    pts = f.points(300, 21)
    got = f.arr.vindex[pts]
    print(row.id, "point-read decode:", decodes)
    assert _same(got, f.mirror[pts])
    assert decodes == ["k_decode"]  # bounding boxes that cut the innermost dim: the general kernel, every row


def _two_chunk_budget(monkeypatch, f):
    from zarr_hip import fancy

    monkeypatch.setattr(fancy, "FANCY_SCRATCH_BYTES", 2 * f.chunk_bytes)
    return -(-int(np.prod(f.row.grid)) // 2)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_sub_batched_read(row, device, decodes, monkeypatch):
    f = _read_fix(row, device)
    n_sub = _two_chunk_budget(monkeypatch, f)
    assert n_sub >= 2
    sel = f.whole_sel()
    got = f.arr.oindex[sel]
    print(row.id, "sub-batched decodes:", decodes)
    assert _same(got, _np_oindex(f.mirror, list(sel)))
    assert decodes == [row.whole] * n_sub


@pytest.mark.parametrize("row", CRC_ROWS, ids=[r.id for r in CRC_ROWS])
def test_corruption_on_read(row, device, decodes, monkeypatch):
    """One flipped bit in the first chunk, which the sub-batched read decodes
    in its first sub-batch while the verdict words are read once after the
    last gather: the oindex read and a one-point vindex read of that chunk
    raise the checksum message, a read of the other chunks succeeds, and with
    the bit restored everything reads clean."""
    f = _read_fix(row, device)
    n_sub = _two_chunk_budget(monkeypatch, f)
    sel = f.whole_sel()
    nd = len(f.shape)
    point = tuple(np.array([c // 2]) for c in row.chunk)
    other = list(sel)
    if f.gax == 0:
        other[0] = sel[0][sel[0] >= row.chunk[0]]
    else:
        other[f.gax] = slice(row.chunk[f.gax], None)
    other = tuple(other)
    f.flip()
    try:
        with pytest.raises(ValueError, match="checksum"):
            f.arr.oindex[sel]
        assert decodes == [row.whole] * n_sub  # every sub-batch ran before the one readback
        with pytest.raises(ValueError, match="checksum"):
            f.arr.vindex[point]
        assert _same(f.arr.oindex[other], _np_oindex(f.mirror, list(other)))
    finally:
        f.flip()
    assert _same(f.arr.oindex[sel], _np_oindex(f.mirror, list(sel)))
    assert _same(f.arr.vindex[point], f.mirror[point])
    assert nd == len(point)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_write(row, device, decodes):
    f = Fix(row, device)
    dt = f.mirror.dtype
    sel = f.whole_sel()
    value = dt.type(77)
    f.arr.oindex[sel] = value            # duplicates on dim 0: a scalar value
    enc = [_kernel()]
    _np_oindex_set(f.mirror, sel, value)
    pts = f.points(300, 22, distinct=True)
    vals = (np.arange(300) + 1000).astype(dt) if dt.itemsize > 1 else (np.arange(300) % 251 + 1).astype(dt)
    f.arr.vindex[pts] = vals
    enc.append(_kernel())
    f.mirror[pts] = vals
    print(row.id, "write decodes:", decodes, "encodes:", enc)
    assert decodes[0] == row.whole and all(k.startswith("k_decode") for k in decodes)
    assert enc == [row.encode] * 2
    assert _same(f.arr[...], f.mirror)                                   # (a) the read-back
    full: dict = {}
    O.write(full, f.meta, (Ellipsis,), f.mirror)
    stored = f.chunk_dict()
    assert sorted(stored) == sorted(full)                                # (b) the key set of a full oracle write
    assert _same(O.read(stored, f.meta), f.mirror)                       # (c) every CRC / shard index decodes
    if not row.sharded:
        for k in full:
            assert stored[k] == full[k], k                               # (d) the oracle's bytes
