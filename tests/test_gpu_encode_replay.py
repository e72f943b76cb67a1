"""ONE prepared encode, launched again and again over a source that changes in
between -- what writer.EncodeLaunch's docstring and include/zarrhip.h promise
("a prepared launch can be replayed", "every launch writes every flag") and
what bench.py's encode lines rest on, while the product path (a fresh launch,
workspace and flags per write) never does it.

Rows, phases and every expected byte come from tests/replay_cases.py (the
oracle alone); tests/test_replay_rules.py shows on the CPU that each row takes
the family its kernel name rests on and that no stale arrival word, non-empty
bit, flag, trailer or status survives the phases unnoticed.

The harness is bench.py's _encode_bench in small: batch_info -> analyze_chain
-> plan_encode -> one EncodeLaunch, whose source is a device tensor the phases
overwrite in place and whose destination is a plain byte tensor: chunk slots
at 256-byte aligned offsets between guard bands of a sentinel.  Before every
launch the statuses and the non-empty flags are overwritten with garbage (the
library owes every launch every status and every flag); the workspace is
zeroed once, at allocation, and must be all zero after every launch
(replay_cases.Row.ws says why).  Everything is bit-exact."""

import numpy as np
import pytest

import replay_cases as RC
from test_gpu_kernel_matrix import _kernel

pytestmark = pytest.mark.gpu

FLAG_GARBAGE = 0x5A5A5A5A


class _Prepared:
    """One row's EncodeLaunch over its own source, destination, workspace and flags."""

    def __init__(self, device, row):
        import torch

        import zarr_hip
        from zarr_hip.planner import analyze_chain, plan_encode
        from zarr_hip.writer import EncodeLaunch

        self.row, self.device = row, device
        dt = np.dtype(row.dtype)
        store = zarr_hip.DeviceStore(device, capacity=1 << 12)
        arr = zarr_hip.Array.create(store, row.shape, row.chunk, row.dtype, row.fill, codecs=RC.codecs(row))
        batch, _ = arr.batch_info((Ellipsis,))
        spec = batch[0][1]
        chain = analyze_chain(arr.codec_pipeline.codecs, spec)
        boxes = RC.boxes(row)
        self.n = len(boxes)
        assert len(batch) == self.n
        offs, total = RC.slots(row)
        # table entry c is chunk c of the grid in C order, whatever order the batch comes in
        items = [None] * self.n
        index = {lo: i for i, (_, lo, _) in enumerate(boxes)}
        for _, _, csel, osel, _ in batch:
            lo = tuple(s.start or 0 for s in osel)
            i = index[lo]
            assert tuple(s.stop - (s.start or 0) for s in csel) == boxes[i][2]
            items[i] = (offs[i], csel, list(lo))
        assert all(it is not None for it in items)
        self.src = torch.zeros(int(np.prod(row.shape)) * dt.itemsize, dtype=torch.uint8, device=device)
        self.dst = torch.full((total,), RC.SENTINEL, dtype=torch.uint8, device=device)
        strides = [int(np.prod(row.shape[d + 1:])) * dt.itemsize for d in range(len(row.shape))]
        t = plan_encode(chain, spec, items, strides, self.src.data_ptr())
        self.el = EncodeLaunch(t.layout, t.chunks, t.sels, self.src, self.dst, t.fast, device, t.rows, t.tile,
                               t.tile_prefix)
        assert self.el.n == self.n
        assert not bool(self.el.d_ws.any())  # zeroed before the first launch: the caller's whole duty
        self._host = {}

    def write(self, phase):
        """The phase's source over the previous one, in place; statuses and flags to garbage."""
        import torch

        h = self._host.get(phase)
        if h is None:
            h = self._host[phase] = torch.from_numpy(np.array(RC.source(self.row, phase)).view(np.uint8).reshape(-1))
        self.src.copy_(h)
        self.scramble()

    def scramble(self):
        self.el.d_status.fill_(-1)
        self.el.d_nonempty.fill_(FLAG_GARBAGE)

    def poison(self):
        self.dst.fill_(RC.SENTINEL)

    def check(self, phase, what):
        import torch

        from zarr_hip import _native as N

        row = self.row
        torch.cuda.synchronize(self.device)
        want = RC.expected(row, phase)
        got, img = self.dst.cpu().numpy(), RC.image(row, phase)
        if not np.array_equal(got, img):
            offs, _ = RC.slots(row)
            at = int(np.nonzero(got != img)[0][0])
            c = max(i for i, o in enumerate(offs) if o <= at) if at >= offs[0] else -1
            where = f"chunk {c} byte {at - offs[c]} of {RC.elen(row)}" if c >= 0 and at - offs[c] < RC.elen(row) \
                else f"guard band at {at}"
            raise AssertionError(f"{row.id} {what} phase {phase}: {where}: got {got[at]:#x}, want {img[at]:#x}; "
                                 f"{int((got != img).sum())} bytes differ")
        flags = self.el.d_nonempty[: self.n].cpu().numpy().view(np.uint32)
        assert flags.tolist() == [0 if w.empty else 1 for w in want], (row.id, what, phase)
        st = self.el.d_status.cpu().numpy().view(np.uint32).reshape(-1, 4)[: self.n]
        assert (st[:, 0] == N.ST_OK).all(), (row.id, what, phase, st[:, 0])
        if row.crc:
            assert st[:, 2].tolist() == [w.crc for w in want], (row.id, what, phase)
        ws = self.el.d_ws.cpu().numpy()
        assert not ws.any(), (row.id, what, phase, row.ws, np.nonzero(ws)[0][:8])


class _Prog:
    """A prepared encode in the program interface ReadGraph replays."""

    def __init__(self, launch):
        self.l = launch

    def launch(self, stream=None):
        self.l.launch(stream)

    def check_fresh(self):
        return None

    def results(self):
        return None


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_eager_replays(device, row):
    """A, B, F, A through the SAME launch object: after each the slots hold the
    oracle's blobs (trailers included; an all-fill chunk is encoded too, its
    flag says empty), the flags are exactly the oracle's emptiness as 0 / 1,
    every status is ST_OK with the trailer as `computed`, the guard bands are
    untouched, the workspace is zero and the row's kernel ran.  Then every slot
    is poisoned and the unchanged source encoded once more: every byte comes
    back (a replay that does nothing is what a decode of the store after many
    replays cannot see)."""
    from zarr_hip import _native as N

    h = _Prepared(device, row)
    for i, ph in enumerate(RC.PHASES):
        h.write(ph)
        h.el.launch()
        assert _kernel() == row.kernel
        h.check(ph, f"launch {i}")
    if "several chunks" in row.proto:
        grid = int(N.lib().zhip_last_grid())
        assert 1 <= grid and 2 * grid <= h.n, (grid, h.n)  # every workgroup took at least two chunks
    h.poison()
    h.scramble()
    h.el.launch()
    h.check(RC.PHASES[-1], "poisoned")


@pytest.mark.parametrize("row", RC.ROWS, ids=[r.id for r in RC.ROWS])
def test_graph_replays(device, row):
    """The same through a captured graph of three launches of the one program
    (a linear graph): per phase the source is overwritten, the graph replayed
    and everything asserted again; the destination is poisoned before the F
    replay and before a last replay over the unchanged source."""
    import zarr_hip

    h = _Prepared(device, row)
    g = zarr_hip.ReadGraph([_Prog(h.el)], 3, device)
    assert g.launches == 3 and _kernel() == row.kernel
    for i, ph in enumerate(RC.PHASES):
        h.write(ph)
        if ph == "F":
            h.poison()
        g.replay()
        g.results()
        h.check(ph, f"replay {i}")
    h.poison()
    h.scramble()
    g.replay()
    g.results()
    h.check(RC.PHASES[-1], "poisoned replay")


@pytest.mark.parametrize("rid", RC.TWO_LAUNCH)
def test_two_launches_on_one_plan(device, rid):
    """bench.py's replica rotation: two launches on the SAME cached plan, each
    with its own source, destination, workspace and flags, captured as
    p0 p1 p0 p1 in one graph; with the sources in different phases (A / F),
    then swapped, each destination equals its own oracle result."""
    import zarr_hip

    row = RC.BY_ID[rid]
    h0, h1 = _Prepared(device, row), _Prepared(device, row)
    assert h0.el.plan is h1.el.plan and h0.el.d_ws.data_ptr() != h1.el.d_ws.data_ptr()
    g = zarr_hip.ReadGraph([_Prog(h0.el), _Prog(h1.el)], 4, device, fuse=False)
    assert g.launches == 4 and _kernel() == row.kernel
    for p0, p1 in (("A", "F"), ("F", "A"), ("B", "A")):
        h0.write(p0)
        h1.write(p1)
        g.replay()
        g.results()
        h0.check(p0, f"first of {p0}/{p1}")
        h1.check(p1, f"second of {p0}/{p1}")
