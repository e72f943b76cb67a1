"""Orthogonal, coordinate and mask selections on the GPU.

zarr sends ``arr.oindex[...]``, ``arr.vindex[...]``, masks and
``arr[np.array([...])]`` through the same ``CodecPipeline.read`` / ``write`` as
basic slices; their ``chunk_selection`` / ``out_selection`` carry integer
arrays or masks (OrthogonalIndexer / CoordinateIndexer / MaskIndexer,
src/zarr/core/indexing.py:625-1046, 1171-1373).  The reference applies them
with numpy fancy indexing on host chunks (scatter_chunk / _merge_chunk_array,
src/zarr/core/chunk_utils.py:88-162).  Here the chunks are decoded in HBM, so:

  read   the box of each item's chunk selection is decoded with the basic
         path into a scratch tensor (one chunk-shaped slot per item, the box
         at its own chunk coordinates), then ONE launch of k_select_copy
         gathers the selected elements into out;
  write  the box is decoded into scratch (a missing chunk gives fill, a CRC
         mismatch raises before anything is stored), k_select_copy scatters
         the selected elements of value into it, and the boxes are written
         back through the basic write path.

This module holds the host normaliser (selection forms -> the separable table
form of zhip_select_copy, include/zarrhip.h), its validation -- no table
reaches the device unvalidated -- and the two routes.

Duplicates on writes: repeated destinations would be a store race on the
device, so all but the LAST occurrence (in table order) are dropped on the
host: per dimension for orthogonal forms, by flat chunk index for point
lists.  The reference's own order within a chunk is unspecified: the argsort
that groups indices by chunk is not stable (indexing.py:803, 1299).

Coordinate and mask selections whose indices are device tensors skip the host
normaliser: read_points / write_points run the same slots, scratch budget and
routes over a pair table that k_points_fill built on the device (points.py).
Orthogonal selections whose index arrays are device tensors do the same one
axis at a time: read_axes / write_axes run items that are products of affine
dimensions and ranges of a table k_axis_fill built (axes.py), each decoded in
the box the count kernel's per-chunk bounds give.
"""

from __future__ import annotations

from dataclasses import dataclass
from itertools import chain
from operator import itemgetter

import numpy as np

from . import _native as N

# Upper bound of the decode scratch of one sub-batch; a batch that needs more
# is served in sub-batches on the same stream (reuse is stream-ordered).
FANCY_SCRATCH_BYTES = 1 << 30

_INT = (int, np.integer)


def is_fancy(sel) -> bool:
    """Anything but a tuple of slices and integers (BasicIndexer's form)."""
    if type(sel) is not tuple:
        return True
    for s in sel:
        if not isinstance(s, slice) and not isinstance(s, _INT):
            return True
    return False


_SEL_GETTERS = (itemgetter(2), itemgetter(3))


def any_fancy(items) -> bool:
    """is_fancy of any item's chunk or out selection.  On every read and
    write, so the per-element work stays inside map / chain / set: the
    distinct element TYPES of the whole batch are examined, not each element."""
    for g in _SEL_GETTERS:
        if not set(map(type, map(g, items))) <= {tuple}:
            return True
        for t in set(map(type, chain.from_iterable(map(g, items)))):
            if t is not slice and not issubclass(t, _INT):
                return True
    return False


# ------------------------------------------------------------- normaliser
@dataclass
class Side:
    """Indices of one product dimension along one axis of one side:
    start + k step, or idx[k]."""

    axis: int
    start: int = 0
    step: int = 0
    idx: np.ndarray | None = None

    def values(self, count: int) -> np.ndarray:
        if self.idx is not None:
            return self.idx
        return self.start + self.step * np.arange(count, dtype=np.int64)

    def bounds(self, count: int) -> tuple[int, int]:
        if self.idx is not None:
            return int(self.idx.min()), int(self.idx.max())
        last = self.start + (count - 1) * self.step
        return min(self.start, last), max(self.start, last)

    def take(self, keep: np.ndarray, count: int) -> "Side":
        return Side(self.axis, idx=self.values(count)[keep])


@dataclass
class PDim:
    """One product dimension: its chunk-side axes and its out-side axis."""

    count: int
    chunk: list          # [Side]: orthogonal forms one, point lists one per chunk axis
    out: Side | None     # None: dropped (an integer, or a drop_axes dimension)


@dataclass
class Normalized:
    dims: list           # [PDim], in element order (last fastest)
    box: list            # per chunk axis (lo, hi): min .. max + 1 of the selected indices
    total: int


@dataclass
class AffineDim:
    """A slice or an integer of one item: chunk indices start + k step; out
    indices out_start + k along out_axis (None: an integer, dropped)."""

    count: int
    start: int
    step: int
    out_axis: int | None
    out_start: int

    @property
    def box(self) -> tuple:
        return self.start, self.start + (self.count - 1) * self.step + 1


@dataclass
class TableDim:
    """The indices of one chunk along a tensor axis: pairs [table_off,
    table_off + count) of the DEVICE table; their in-chunk indices lie in
    [lo, hi] and their positions in the index tensor in [0, n)."""

    count: int
    table_off: int
    lo: int
    hi: int
    n: int
    out_axis: int

    @property
    def box(self) -> tuple:
        return self.lo, self.hi + 1


def _arr(x):
    return np.asarray(x) if isinstance(x, list) else x


def _kind(x) -> str:
    if isinstance(x, slice):
        return "s"
    if isinstance(x, _INT) and not isinstance(x, (bool, np.bool_)):
        return "i"
    if isinstance(x, np.ndarray):
        if x.dtype.kind == "b":
            return "b"
        if x.dtype.kind in "iu":
            return "a"
    raise NotImplementedError(f"selection item of type {type(x).__name__}"
                              f"{' dtype ' + str(x.dtype) if isinstance(x, np.ndarray) else ''} "
                              "(expected slice, integer, integer array or boolean array)")


def _mesh_axis(a: np.ndarray, i: int, n: int) -> bool:
    """a is axis i of an np.ix_ mesh over n dimensions."""
    return a.ndim == n and all(s == 1 for j, s in enumerate(a.shape) if j != i)


def _check_idx(idx: np.ndarray, n: int, what: str) -> np.ndarray:
    idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"{what} index out of bounds for dimension with length {n}")
    return idx


def _slice_side(s: slice, n: int, axis: int, what: str) -> tuple[int, Side]:
    if s.step is not None and s.step < 1:
        raise IndexError(f"{what} slice step must be >= 1")
    start, stop, step = s.indices(n)
    return len(range(start, stop, step)), Side(axis, start, step)


def _chunk_dims(csel, chunk_shape) -> tuple[list, bool]:
    """chunk_selection -> ([(count, [Side], naturally dropped)], point list?)."""
    if type(csel) is not tuple:
        raise NotImplementedError(f"chunk selection given as a bare {type(csel).__name__} (expected a tuple "
                                  "with one entry per chunk dimension)")
    csel = tuple(_arr(x) for x in csel)
    nd = len(chunk_shape)
    if len(csel) != nd:
        raise ValueError(f"chunk selection has {len(csel)} entries for a {nd}-dimensional chunk")
    kinds = [_kind(x) for x in csel]
    arrays = [i for i, k in enumerate(kinds) if k in "ab"]
    for i in arrays:
        if kinds[i] == "b" and csel[i].ndim != 1:
            raise NotImplementedError("N-d masks in a chunk selection (MaskIndexer hands coordinate arrays)")
    if len(arrays) == nd and nd > 1:
        if all(csel[i].ndim == 1 for i in arrays):  # CoordinateIndexer's point list
            if any(kinds[i] == "b" for i in arrays):
                raise NotImplementedError("boolean arrays in a pointwise (coordinate) chunk selection")
            n = csel[0].shape[0]
            if any(csel[i].shape[0] != n for i in arrays):
                raise ValueError("coordinate arrays of a chunk selection differ in length")
            sides = [Side(i, idx=_check_idx(csel[i], chunk_shape[i], "chunk")) for i in range(nd)]
            return [(n, sides, False)], True
        if all(_mesh_axis(csel[i], i, nd) for i in arrays):  # np.ix_ mesh
            if any(kinds[i] == "b" for i in arrays):
                raise NotImplementedError("boolean arrays in an np.ix_ mesh (np.ix_ hands integers)")
            return [(csel[i].size, [Side(i, idx=_check_idx(csel[i], chunk_shape[i], "chunk"))], False)
                    for i in range(nd)], False
        raise NotImplementedError("integer arrays of mixed or N-d shapes in a chunk selection (neither a point "
                                  "list of 1-d arrays nor an np.ix_ mesh)")
    if len(arrays) > 1:
        raise NotImplementedError("pointwise arrays mixed with slices or integers in a chunk selection")
    if arrays and any(k == "i" for k in kinds):
        raise NotImplementedError("an integer next to a bare array in a chunk selection (the orthogonal "
                                  "indexer hands these as an np.ix_ mesh with drop_axes)")
    out = []
    for i, (x, k) in enumerate(zip(csel, kinds)):
        n = chunk_shape[i]
        if k == "s":
            cnt, side = _slice_side(x, n, i, "chunk")
            out.append((cnt, [side], False))
        elif k == "i":
            v = int(x)
            if not 0 <= v < n:
                raise IndexError(f"chunk index out of bounds for dimension with length {n}")
            out.append((1, [Side(i, v, 0)], True))
        else:
            if x.ndim != 1:
                raise NotImplementedError("an N-d array in a per-dimension chunk selection")
            if k == "b":
                if x.shape[0] != n:
                    raise IndexError(f"boolean array has the wrong length for a chunk dimension; expected {n}, "
                                     f"got {x.shape[0]}")
                x = np.nonzero(x)[0]
            idx = _check_idx(x, n, "chunk")
            out.append((idx.size, [Side(i, idx=idx)], False))
    return out, False


def _out_sides(osel, out_shape, n_kept: int) -> list:
    """out_selection -> [(count, Side)] per out axis."""
    if isinstance(osel, (slice, np.ndarray, list)):  # CoordinateIndexer: a bare slice / array
        osel = (osel,)
    if type(osel) is not tuple:
        raise NotImplementedError(f"out selection of type {type(osel).__name__}")
    osel = tuple(_arr(x) for x in osel)
    if len(osel) != len(out_shape) or len(osel) != n_kept:
        raise ValueError(f"out selection has {len(osel)} entries for {n_kept} selected dimensions and a "
                         f"{len(out_shape)}-dimensional out")
    kinds = [_kind(x) for x in osel]
    if any(k in "ib" for k in kinds):
        raise NotImplementedError("integers or boolean arrays in an out selection")
    arrays = [j for j, k in enumerate(kinds) if k == "a"]
    mesh = len(osel) > 1 and len(arrays) == len(osel) and all(_mesh_axis(osel[j], j, len(osel)) for j in arrays)
    if not mesh:
        if len(arrays) > 1:
            raise NotImplementedError("more than one integer array in an out selection that is no np.ix_ mesh")
        if arrays and osel[arrays[0]].ndim != 1:
            raise NotImplementedError("an N-d integer array in an out selection")
    res = []
    for j, (x, k) in enumerate(zip(osel, kinds)):
        if k == "s":
            res.append(_slice_side(x, out_shape[j], j, "out"))
        else:
            idx = _check_idx(x, out_shape[j], "out")
            res.append((idx.size, Side(j, idx=idx)))
    return res


def _keep_last(flat: np.ndarray) -> np.ndarray | None:
    """Positions of the last occurrence of each value, ascending; None when
    nothing repeats."""
    n = flat.size
    _, first_rev = np.unique(flat[::-1], return_index=True)
    if first_rev.size == n:
        return None
    return np.sort(n - 1 - first_rev)


def normalize(chunk_selection, out_selection, drop_axes, chunk_shape, out_shape, dedupe: bool = False) -> Normalized:
    """One item's selections as product dimensions, validated: every chunk-side
    index in [0, chunk dim), every out index in [0, out dim), equal counts on
    both sides after drop_axes.  out_shape None: a scalar value (the out side
    is ignored).  dedupe: a write -- keep the last occurrence of a repeated
    chunk-side destination."""
    chunk_shape = tuple(int(s) for s in chunk_shape)
    cd, points = _chunk_dims(chunk_selection, chunk_shape)
    result = [d for d in cd if not d[2]]  # the dimensions numpy's chunk[chunk_selection] keeps
    drop = tuple(int(a) for a in (drop_axes or ()))
    for a in drop:
        if not 0 <= a < len(result):
            raise ValueError(f"drop_axes entry {a} out of range for a selection of {len(result)} dimensions")
        if result[a][0] != 1:
            raise ValueError(f"drop_axes entry {a} names a dimension that selects {result[a][0]} elements")
    kept = [i for i in range(len(result)) if i not in drop]
    outs: dict = {}
    if out_shape is not None:
        sides = _out_sides(out_selection, tuple(int(s) for s in out_shape), len(kept))
        for i, (cnt, side) in zip(kept, sides):
            if cnt != result[i][0]:
                raise ValueError(f"chunk selection picks {result[i][0]} elements along a dimension, out selection "
                                 f"{cnt}")
            outs[id(result[i])] = side
    dims = []
    for d in cd:
        cnt, sides, _ = d
        out = outs.get(id(d))
        if dedupe and cnt > 1 and any(s.idx is not None for s in sides):
            if points:
                flat = np.ravel_multi_index(tuple(s.idx for s in sides), chunk_shape)
            else:
                flat = sides[0].idx
            keep = _keep_last(flat)
            if keep is not None:
                sides = [s.take(keep, cnt) for s in sides]
                out = None if out is None else out.take(keep, cnt)
                cnt = keep.size
        dims.append(PDim(cnt, sides, out))
    total = 1
    for d in dims:
        total *= d.count
    box = [(0, 1)] * len(chunk_shape)
    if total:
        for d in dims:
            for s in d.chunk:
                lo, hi = s.bounds(d.count)
                box[s.axis] = (lo, hi + 1)
    if total >= 1 << 31:
        raise NotImplementedError("a selection of 2**31 or more elements of one chunk")
    return Normalized(dims, box, total)


# ------------------------------------------------------------------ tables
class SelectTables:
    """The host tables of one zhip_select_copy launch.  add() turns a
    normalised item into byte offsets against the two buffers and checks that
    every offset lies inside them."""

    def __init__(self, itemsize: int, a_size: int, b_size: int):
        self.itemsize = int(itemsize)
        self.a_size = int(a_size)
        self.b_size = int(b_size)
        self.items: list = []
        self.tables: list = []
        self.pairs = 0

    def add(self, nz: Normalized, chunk_base: int, chunk_strides, out_base: int, out_strides,
            write: bool = False) -> None:
        """chunk_* / out_*: byte offset of the item's origin and byte strides on
        the chunk side (the decoded scratch) and the out side (out on reads,
        value on writes; out_strides None: a scalar value, read at offset 0).
        read: a = chunk side, b = out side; write: the reverse."""
        if nz.total == 0:
            return
        rec = np.zeros((), N.SELECT_ITEM_DT)
        base = [int(chunk_base), int(out_base)]
        lo = [int(chunk_base), int(out_base)]
        hi = [int(chunk_base), int(out_base)]
        nd = 0
        for d in nz.dims:
            aff = [True, True]
            start = [0, 0]
            step = [0, 0]
            vec = [None, None]
            for s in d.chunk:
                st = int(chunk_strides[s.axis])
                if s.idx is None:
                    start[0] += s.start * st
                    step[0] += s.step * st
                else:
                    aff[0] = False
            if d.out is not None and out_strides is not None:
                st = int(out_strides[d.out.axis])
                if d.out.idx is None:
                    start[1] += d.out.start * st
                    step[1] += d.out.step * st
                else:
                    aff[1] = False
            if d.count == 1 and aff[0] and aff[1]:  # folded into the bases: no division for it
                for z in (0, 1):
                    base[z] += start[z]
                    lo[z] += start[z]
                    hi[z] += start[z]
                continue
            if not aff[0]:
                v = np.zeros(d.count, np.int64)
                for s in d.chunk:
                    v += s.values(d.count) * int(chunk_strides[s.axis])
                vec[0] = v
            if not aff[1]:
                vec[1] = d.out.idx * int(out_strides[d.out.axis])
            for z in (0, 1):
                if vec[z] is None:
                    last = start[z] + (d.count - 1) * step[z]
                    lo[z] += min(start[z], last)
                    hi[z] += max(start[z], last)
                else:
                    lo[z] += int(vec[z].min())
                    hi[z] += int(vec[z].max())
            if nd >= N.MAX_DIMS:
                raise NotImplementedError(f"a selection of more than {N.MAX_DIMS} product dimensions")
            D = rec["dims"][nd]
            D["count"] = d.count
            D["div"] = N.fdiv(d.count)
            za, zb = (1, 0) if write else (0, 1)
            if aff[0] and aff[1]:
                D["a0"], D["sa"], D["b0"], D["sb"] = start[za], step[za], start[zb], step[zb]
            else:
                for z in (0, 1):
                    if vec[z] is None:
                        vec[z] = start[z] + step[z] * np.arange(d.count, dtype=np.int64)
                D["table"] = 1
                D["table_off"] = self.pairs
                self.tables.append(np.stack([vec[za], vec[zb]], axis=1))
                self.pairs += d.count
            nd += 1
        if nd == 0:  # a single element
            rec["dims"][0]["count"] = 1
            rec["dims"][0]["div"] = N.fdiv(1)
            nd = 1
        za, zb = (1, 0) if write else (0, 1)
        for z, size, name in ((za, self.a_size, "source"), (zb, self.b_size, "destination")):
            if lo[z] < 0 or hi[z] + self.itemsize > size:
                raise IndexError(f"selection reaches outside its {name} buffer (bytes {lo[z]} .. "
                                 f"{hi[z] + self.itemsize} of {size})")
        rec["a_base"], rec["b_base"] = base[za], base[zb]
        rec["ndim"] = nd
        rec["total"] = nz.total
        self.items.append(rec)

    def add_points(self, count: int, table_off: int, slot_base: int, slot_bytes: int, lin_last: int,
                   write: bool = False) -> None:
        """One touched chunk of a device-built point table (zhip_points_fill):
        a single table dimension over pairs [table_off, table_off + count) of
        the DEVICE table given to launch().  The slot-side entries lie in
        [0, slot_bytes) by construction and the other side's are at most
        lin_last (zarrhip.h), so the check is of the two ends."""
        if count == 0:
            return
        za, zb = (1, 0) if write else (0, 1)
        lo = [int(slot_base), 0]
        hi = [int(slot_base) + int(slot_bytes) - self.itemsize, int(lin_last)]
        for z, size, name in ((za, self.a_size, "source"), (zb, self.b_size, "destination")):
            if lo[z] < 0 or hi[z] + self.itemsize > size:
                raise IndexError(f"selection reaches outside its {name} buffer (bytes {lo[z]} .. "
                                 f"{hi[z] + self.itemsize} of {size})")
        rec = np.zeros((), N.SELECT_ITEM_DT)
        D = rec["dims"][0]
        D["count"] = count
        D["div"] = N.fdiv(count)
        D["table"] = 1
        D["table_off"] = table_off
        rec["a_base"], rec["b_base"] = lo[za], lo[zb]
        rec["ndim"] = 1
        rec["total"] = count
        self.items.append(rec)

    def add_product(self, dims, slot_base: int, chunk_strides, lin_strides, write: bool = False) -> None:
        """One touched chunk of a device-planned orthogonal selection
        (axes.py): a product of dimensions that are each affine on both sides
        (AffineDim: a slice or an integer) or a range of the DEVICE table
        given to launch() (TableDim, pairs built by zhip_axis_fill).
        chunk_strides: byte strides of the slot at slot_base per array
        dimension; lin_strides: byte strides of out / value per selected
        dimension (None: a scalar value).  A table dimension's slot-side
        entries lie in [lo, hi] * stride -- the bounds read back from the
        count -- and the other side's in [0, (n - 1) * lin stride], so the
        item's extreme offsets are checked from those ends."""
        base = [int(slot_base), 0]
        lo = [int(slot_base), 0]
        hi = [int(slot_base), 0]
        rec = np.zeros((), N.SELECT_ITEM_DT)
        za, zb = (1, 0) if write else (0, 1)
        nd, total = 0, 1
        for d, D in enumerate(dims):
            cst = int(chunk_strides[d])
            ost = 0 if (lin_strides is None or D.out_axis is None) else int(lin_strides[D.out_axis])
            if D.count < 1:
                return
            total *= D.count
            if isinstance(D, TableDim):
                ends = [(D.lo * cst, D.hi * cst), (0, (D.n - 1) * ost)]
                if not (0 <= D.lo <= D.hi and 1 <= D.count <= D.n):
                    raise IndexError(f"a table dimension with bounds {D.lo} .. {D.hi} and {D.count} of {D.n} indices")
            else:
                start = [D.start * cst, D.out_start * ost]
                step = [D.step * cst, ost]
                ends = [(start[z], start[z] + (D.count - 1) * step[z]) for z in (0, 1)]
            for z in (0, 1):
                lo[z] += min(ends[z])
                hi[z] += max(ends[z])
            if D.count == 1 and not isinstance(D, TableDim):  # folded into the bases: no division for it
                for z in (0, 1):
                    base[z] += start[z]
                continue
            if nd >= N.MAX_DIMS:
                raise NotImplementedError(f"a selection of more than {N.MAX_DIMS} product dimensions")
            R = rec["dims"][nd]
            R["count"] = D.count
            R["div"] = N.fdiv(D.count)
            if isinstance(D, TableDim):
                R["table"] = 1
                R["table_off"] = D.table_off
            else:
                R["a0"], R["sa"], R["b0"], R["sb"] = start[za], step[za], start[zb], step[zb]
            nd += 1
        if total >= 1 << 31:
            raise NotImplementedError("a selection of 2**31 or more elements of one chunk")
        if nd == 0:  # a single element
            rec["dims"][0]["count"] = 1
            rec["dims"][0]["div"] = N.fdiv(1)
            nd = 1
        for z, size, name in ((za, self.a_size, "source"), (zb, self.b_size, "destination")):
            if lo[z] < 0 or hi[z] + self.itemsize > size:
                raise IndexError(f"selection reaches outside its {name} buffer (bytes {lo[z]} .. "
                                 f"{hi[z] + self.itemsize} of {size})")
        rec["a_base"], rec["b_base"] = base[za], base[zb]
        rec["ndim"] = nd
        rec["total"] = total
        self.items.append(rec)

    def finish(self):
        """(items, table pairs, tile prefix, n_tiles) as contiguous arrays."""
        items = np.array(self.items, N.SELECT_ITEM_DT) if self.items else np.zeros(0, N.SELECT_ITEM_DT)
        table = np.concatenate(self.tables).astype(np.int64, copy=False) if self.tables else np.zeros((1, 2), np.int64)
        tiles = (items["total"].astype(np.int64) + N.SELECT_TILE - 1) // N.SELECT_TILE
        prefix = np.zeros(len(items) + 1, np.int64)
        np.cumsum(tiles, out=prefix[1:])
        if prefix[-1] >= 1 << 31:
            raise NotImplementedError("a selection batch of 2**31 or more tiles")
        return items, np.ascontiguousarray(table), prefix.astype(np.uint32), int(prefix[-1])

    def run_host(self, a: np.ndarray, b: np.ndarray) -> None:
        """The CPU hook (zhip_emulate_select_copy): the kernel's tile walk and
        address arithmetic over host memory.  a, b: contiguous uint8 views."""
        items, table, prefix, n_tiles = self.finish()
        if a.nbytes < self.a_size or b.nbytes < self.b_size:
            raise ValueError("host buffers shorter than the sizes the tables were checked against")
        N.check(N.lib().zhip_emulate_select_copy(
            items.ctypes.data, len(items), table.ctypes.data, len(table), prefix.ctypes.data, n_tiles,
            a.ctypes.data, self.a_size, b.ctypes.data, self.b_size, self.itemsize), "zhip_emulate_select_copy")

    def launch(self, a, b, device, table=None):
        """One k_select_copy launch on torch's current stream of `device`:
        a, b are device tensors whose extents are a_size / b_size.  table: a
        device-resident pair table (an int64 tensor, add_points' items index
        it): only items and prefix are uploaded then.  Returns the uploaded
        table block (keep it until the stream has passed)."""
        from .pipeline import _stream_handle, _Upload

        items, host_table, prefix, n_tiles = self.finish()
        if n_tiles == 0:
            return None
        if table is not None and self.tables:
            raise ValueError("host-built table dimensions next to a device-resident table")
        stream = _stream_handle(device)
        up = _Upload(device)
        for part in (items, prefix) if table is not None else (items, host_table, prefix):
            up.add(part.view(np.uint8).reshape(-1))
        if table is not None:
            p_items, p_prefix = up.commit(stream)
            p_table = table.data_ptr()
        else:
            p_items, p_table, p_prefix = up.commit(stream)
        N.check(N.lib().zhip_select_copy(p_items, len(items), p_table, p_prefix, n_tiles, a.data_ptr(), self.a_size,
                                         b.data_ptr(), self.b_size, self.itemsize, stream), "zhip_select_copy")
        return up.dev


def tensor_extent(t) -> int:
    """Bytes from t.data_ptr() to the end of t's last element."""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


# ------------------------------------------------------------------ routes
def _split(pipe, items):
    """(normalised specs, fancy item indices, basic item indices)."""
    from .pipeline import ArraySpec, coerce_spec

    seen: dict = {}
    out = []
    for it in items:
        it = tuple(it)
        sp = it[1]
        if type(sp) is not ArraySpec:
            sp = seen.get(id(it[1]))
            if sp is None:
                sp = seen[id(it[1])] = coerce_spec(it[1])
        out.append((it[0], sp) + it[2:])
    fancy = [i for i, it in enumerate(out) if is_fancy(it[2]) or is_fancy(it[3])]
    fs = set(fancy)
    basic = [i for i in range(len(out)) if i not in fs]
    return out, fancy, basic


def _one_spec(batch, fancy):
    from .pipeline import _spec_key

    spec = batch[fancy[0]][1]
    k0 = _spec_key(spec)
    for it in batch:
        if it[1] is not spec and _spec_key(it[1]) != k0:
            raise NotImplementedError("a batch that mixes chunk specs (a rectilinear grid) and carries orthogonal, "
                                      "coordinate or mask selections")
    if spec.ndim == 0:
        raise NotImplementedError("a non-basic selection of a 0-dimensional chunk")
    return spec


def _direct(pipe) -> bool:
    """One device, no nesting, no host stage, no value codecs: the box decode is planned and
    launched here, back to back with the gather; every other route composes
    through the public read_sync / _write_sync (an extra synchronisation)."""
    if pipe._value_split() is not None:  # value codecs: the scratch is array-dtype, through read_sync
        return False
    return len(pipe.devices) <= 1 and pipe._nested() is None and pipe._host_split() is None


def _slots(spec, n: int) -> int:
    nbytes = int(np.prod(spec.shape)) * np.dtype(spec.dtype).itemsize
    return max(1, min(n, FANCY_SCRATCH_BYTES // max(nbytes, 1)))


def _slot_sel(box, j: int, s0: int) -> tuple:
    """The box at its own chunk coordinates inside slot j of the scratch."""
    return (slice(j * s0 + box[0][0], j * s0 + box[0][1]),) + tuple(slice(lo, hi) for lo, hi in box[1:])


def _scratch_strides(spec, itemsize: int) -> list:
    st = [itemsize] * len(spec.shape)
    for d in range(len(spec.shape) - 2, -1, -1):
        st[d] = st[d + 1] * spec.shape[d + 1]
    return st


def read(pipe, items, out, drop_axes) -> tuple:
    """read_sync of a batch with non-basic items (see the module docstring)."""
    from .buffer import torch_dtype
    from .pipeline import ProgramGroup, _resolve_out, _torch

    torch = _torch()
    batch, fancy, basic = _split(pipe, items)
    spec = _one_spec(batch, fancy)
    dev_out, host_out = _resolve_out(
        out, [(it[0], it[1], (), (slice(0, 0),), False) for it in batch], drop_axes)
    device = dev_out.device
    itemsize = dev_out.element_size()
    if np.dtype(spec.dtype).itemsize != itemsize:
        raise TypeError("out dtype itemsize does not match the array dtype")
    ostr = [int(s) * itemsize for s in dev_out.stride()]
    # every table is built and checked before the first launch
    norm = [normalize(batch[i][2], batch[i][3], drop_axes, spec.shape, tuple(dev_out.shape)) for i in fancy]
    results: list = [None] * len(batch)
    direct = _direct(pipe)
    s0 = spec.shape[0]
    cstr = _scratch_strides(spec, itemsize)
    slot_bytes = cstr[0] * s0
    per = _slots(spec, len(fancy))
    progs, groups, keep = [], [], []
    with torch.cuda.device(device):
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        if basic:
            bb = [batch[i] for i in basic]
            if direct:
                p = pipe.prepare_read(bb, dev_out, drop_axes)
                p.launch()
                progs.append(p)
                groups.append(basic)
            else:
                for i, r in zip(basic, pipe.read_sync(bb, dev_out, drop_axes)):
                    results[i] = r
        for at in range(0, len(fancy), per):
            sub = range(at, min(at + per, len(fancy)))
            boxes = []
            tabs = SelectTables(itemsize, tensor_extent(scratch), tensor_extent(dev_out))
            for j, k in enumerate(sub):
                it, nz = batch[fancy[k]], norm[k]
                boxes.append((it[0], spec, tuple(slice(lo, hi) for lo, hi in nz.box), _slot_sel(nz.box, j, s0), False))
                tabs.add(nz, j * slot_bytes, cstr, 0, ostr)
            idx = [fancy[k] for k in sub]
            if direct:
                p = pipe.prepare_read(boxes, scratch)
                p.launch()
                progs.append(p)
                groups.append(idx)
            else:
                for i, r in zip(idx, pipe.read_sync(boxes, scratch)):
                    results[i] = r
            keep.append(tabs.launch(scratch, dev_out, device))
        if progs:  # ONE readback of every launch's error and verdict words, after the last gather
            for i, r in enumerate(ProgramGroup(progs, groups, len(batch)).results_fast()):
                if r is not None:
                    results[i] = r
    if host_out is not None:
        from .buffer import copy_to_host

        copy_to_host(dev_out, host_out)
    del keep
    return tuple(results)


def _write_box(pipe, spec, nz: Normalized):
    """The region of the chunk a write item decodes, updates and writes back:
    the whole chunk (written is_complete) for unsharded chains; for a plain
    sharded chain the selection's box rounded outward to inner-chunk
    boundaries and clipped to the shard -- a partial shard write of whole
    inner chunks (inner chunks outside it pass through as bytes)."""
    from .codecs import ShardingCodec

    ab = pipe.array_bytes_codec
    whole = [(0, int(s)) for s in spec.shape]
    if not isinstance(ab, ShardingCodec) or pipe.array_array_codecs or nz.total == 0:
        return whole, True
    inner = tuple(int(c) for c in ab.chunk_shape)
    box = [((lo // c) * c, min(-(-hi // c) * c, int(n))) for (lo, hi), c, n in zip(nz.box, inner, spec.shape)]
    return box, box == whole


def write(pipe, items, value, drop_axes, partial_encode: bool) -> None:
    """_write_sync of a batch with non-basic items (see the module docstring).
    A batch larger than the scratch budget is written in sub-batches: a CRC
    mismatch then raises before its own and every later sub-batch is stored."""
    from .buffer import torch_dtype
    from .pipeline import _resolve_value, _torch, _write_device
    from .writer import _value_tensor

    torch = _torch()
    batch, fancy, basic = _split(pipe, items)
    spec = _one_spec(batch, fancy)
    value = _resolve_value(value)
    scalar = not isinstance(value, torch.Tensor) and np.ndim(value) == 0
    if isinstance(value, torch.Tensor) and value.dim() == 0:
        scalar = True
    device = _write_device(batch, value)
    itemsize = np.dtype(spec.dtype).itemsize
    with torch.cuda.device(device):
        v = _value_tensor(value, spec.dtype, device)
        if scalar:
            v = v.reshape(1)
        vshape = None if scalar else tuple(v.shape)
        vstr = None if scalar else [int(s) * itemsize for s in v.stride()]
        norm = [normalize(batch[i][2], batch[i][3], drop_axes, spec.shape, vshape, dedupe=True) for i in fancy]
        direct = _direct(pipe)
        s0 = spec.shape[0]
        cstr = _scratch_strides(spec, itemsize)
        slot_bytes = cstr[0] * s0
        per = _slots(spec, len(fancy))
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        for at in range(0, len(fancy), per):
            sub = range(at, min(at + per, len(fancy)))
            rbatch, wbatch = [], []
            tabs = SelectTables(itemsize, tensor_extent(v), tensor_extent(scratch))
            for j, k in enumerate(sub):
                it, nz = batch[fancy[k]], norm[k]
                box, complete = _write_box(pipe, spec, nz)
                csel = tuple(slice(lo, hi) for lo, hi in box)
                osel = _slot_sel(box, j, s0)
                rbatch.append((it[0], spec, csel, osel, False))
                wbatch.append((it[0], spec, csel, osel, complete))
                tabs.add(nz, j * slot_bytes, cstr, 0, vstr, write=True)
            if direct:
                p = pipe.prepare_read(rbatch, scratch)
                p.launch()
                up = tabs.launch(v, scratch, device)
                p.results_fast()  # a checksum mismatch raises here: nothing stored yet
                del up
            else:
                pipe.read_sync(rbatch, scratch)
                tabs.launch(v, scratch, device)
            pipe._write_sync(wbatch, scratch, (), partial_encode)
        if basic:
            pipe._write_sync([batch[i] for i in basic], value, drop_axes, partial_encode)


# ---------------------------------------------- device-planned point lists
def _points_setup(pipe, spec, ix, n_getters: int):
    if spec.ndim == 0:
        raise NotImplementedError("a non-basic selection of a 0-dimensional chunk")
    if tuple(int(s) for s in spec.shape) != tuple(ix.chunk_shape):
        raise ValueError("the indexer's chunk shape is not the spec's")
    if n_getters != len(ix.chunk_rixs):
        raise ValueError(f"{n_getters} byte getters for {len(ix.chunk_rixs)} touched chunks")
    whole = [(0, int(s)) for s in spec.shape]
    return whole, tuple(slice(0, int(s)) for s in spec.shape)


def read_points(pipe, getters, spec, ix, dev_out) -> tuple:
    """A coordinate or mask read planned on the device (points.py): getters[i]
    is the chunk ix.chunk_rixs[i]; dev_out a 1-d device tensor of ix.n
    elements (any stride) on the indexer's device.  Each touched chunk is one
    item whose box is the WHOLE chunk (the whole shard of a sharded chain:
    narrowing it would need per-axis minima from the device), decoded into
    its slot; the selection's pair table is built once by k_points_fill, the
    sub-batches differ only in their items.  Slots, scratch budget, the direct
    and composed routes and the single result readback are read()'s."""
    from .buffer import torch_dtype
    from .pipeline import ProgramGroup, _torch

    torch = _torch()
    whole, csel = _points_setup(pipe, spec, ix, len(getters))
    device = dev_out.device
    if device != ix.device:
        raise ValueError(f"the coordinates are on {ix.device}, the read runs on {device}")
    itemsize = dev_out.element_size()
    if np.dtype(spec.dtype).itemsize != itemsize:
        raise TypeError("out dtype itemsize does not match the array dtype")
    n = ix.n
    if dev_out.dim() != 1 or dev_out.numel() != n:
        raise ValueError(f"out of shape {tuple(dev_out.shape)} for a selection of {n} points")
    if n == 0:
        return ()
    ostride = int(dev_out.stride(0)) * itemsize
    results: list = [None] * len(getters)
    direct = _direct(pipe)
    s0 = spec.shape[0]
    cstr = _scratch_strides(spec, itemsize)
    slot_bytes = cstr[0] * s0
    per = _slots(spec, len(getters))
    progs, groups, keep = [], [], []
    with torch.cuda.device(device):
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        table = ix.build_table(cstr, ostride, False)
        for at in range(0, len(getters), per):
            idx = list(range(at, min(at + per, len(getters))))
            tabs = SelectTables(itemsize, tensor_extent(scratch), tensor_extent(dev_out))
            boxes = []
            for j, k in enumerate(idx):
                boxes.append((getters[k], spec, csel, _slot_sel(whole, j, s0), False))
                tabs.add_points(int(ix.counts[k]), int(ix.first[k]), j * slot_bytes, slot_bytes, (n - 1) * ostride)
            if direct:
                p = pipe.prepare_read(boxes, scratch)
                p.launch()
                progs.append(p)
                groups.append(idx)
            else:
                for i, r in zip(idx, pipe.read_sync(boxes, scratch)):
                    results[i] = r
            keep.append(tabs.launch(scratch, dev_out, device, table=table))
        if progs:  # ONE readback of every launch's error and verdict words, after the last gather
            for i, r in enumerate(ProgramGroup(progs, groups, len(getters)).results_fast()):
                if r is not None:
                    results[i] = r
    del keep, table
    return tuple(results)


def write_points(pipe, getters, spec, ix, value, distinct: bool, partial_encode: bool = True) -> None:
    """A coordinate or mask write planned on the device: every touched chunk
    is decoded whole into its slot (a missing chunk gives fill, a CRC mismatch
    raises before anything of its sub-batch is stored), k_select_copy scatters
    value into the slots, and the chunks are written back whole through the
    basic write path.  distinct: the points are known to differ (a mask's
    nonzero coordinates).  Repeated destinations are not dropped on the
    device, so a coordinate write takes a scalar value only: equal values
    racing to one address."""
    from .buffer import torch_dtype
    from .pipeline import _resolve_value, _torch
    from .writer import _value_tensor

    torch = _torch()
    whole, csel = _points_setup(pipe, spec, ix, len(getters))
    value = _resolve_value(value)
    scalar = (isinstance(value, torch.Tensor) and value.dim() == 0) or \
        (not isinstance(value, torch.Tensor) and np.ndim(value) == 0)
    if not scalar and not distinct:
        raise NotImplementedError("a coordinate write through device indices with an array value: repeated "
                                  "coordinates need a keep-last pass on the device, which is not built; pass "
                                  "the indices as host (numpy) arrays, or write a scalar")
    device = ix.device
    itemsize = np.dtype(spec.dtype).itemsize
    n = ix.n
    if n == 0:
        return
    with torch.cuda.device(device):
        v = _value_tensor(value, spec.dtype, device)
        v = v.reshape(1) if scalar else v
        if not scalar and (v.dim() != 1 or v.numel() != n):
            raise ValueError(f"value of shape {tuple(v.shape)} for a selection of {n} points")
        vstride = 0 if scalar else int(v.stride(0)) * itemsize
        s0 = spec.shape[0]
        cstr = _scratch_strides(spec, itemsize)
        slot_bytes = cstr[0] * s0
        per = _slots(spec, len(getters))
        direct = _direct(pipe)
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        table = ix.build_table(cstr, vstride, True)
        for at in range(0, len(getters), per):
            rbatch, wbatch = [], []
            tabs = SelectTables(itemsize, tensor_extent(v), tensor_extent(scratch))
            for j, k in enumerate(range(at, min(at + per, len(getters)))):
                osel = _slot_sel(whole, j, s0)
                rbatch.append((getters[k], spec, csel, osel, False))
                wbatch.append((getters[k], spec, csel, osel, True))
                tabs.add_points(int(ix.counts[k]), int(ix.first[k]), j * slot_bytes, slot_bytes, (n - 1) * vstride,
                                write=True)
            if direct:
                p = pipe.prepare_read(rbatch, scratch)
                p.launch()
                up = tabs.launch(v, scratch, device, table=table)
                p.results_fast()  # a checksum mismatch raises here: nothing stored yet
                del up
            else:
                pipe.read_sync(rbatch, scratch)
                tabs.launch(v, scratch, device, table=table)
            pipe._write_sync(wbatch, scratch, (), partial_encode)
        del table


# ------------------------------------- device-planned orthogonal selections
def _axes_setup(pipe, spec, ix, n_getters: int):
    if spec.ndim == 0:
        raise NotImplementedError("a non-basic selection of a 0-dimensional chunk")
    if tuple(int(s) for s in spec.shape) != tuple(ix.chunk_shape):
        raise ValueError("the indexer's chunk shape is not the spec's")
    items = ix.items()
    if n_getters != len(items):
        raise ValueError(f"{n_getters} byte getters for {len(items)} touched chunks")
    return items


def read_axes(pipe, getters, spec, ix, dev_out) -> tuple:
    """An orthogonal read planned on the device (axes.py): getters[i] is the
    chunk of ix.items()[i]; dev_out a device tensor of shape ix.shape (any
    strides) on the indexer's device.  Each touched chunk is one item whose
    box is the product of its per-axis ranges -- the minimum .. maximum
    in-chunk index read back for tensor axes -- decoded into its slot at its
    own chunk coordinates (only the touched inner chunks of a shard); every
    tensor axis' pairs sit in one table built once by k_axis_fill, the
    sub-batches differ only in their items.  Slots, scratch budget, the direct
    and composed routes and the single result readback are read()'s."""
    from .buffer import torch_dtype
    from .pipeline import ProgramGroup, _torch

    torch = _torch()
    items = _axes_setup(pipe, spec, ix, len(getters))
    device = dev_out.device
    if device != ix.device:
        raise ValueError(f"the indices are on {ix.device}, the read runs on {device}")
    itemsize = dev_out.element_size()
    if np.dtype(spec.dtype).itemsize != itemsize:
        raise TypeError("out dtype itemsize does not match the array dtype")
    if tuple(dev_out.shape) != tuple(ix.shape):
        raise ValueError(f"out of shape {tuple(dev_out.shape)} for a selection of shape {tuple(ix.shape)}")
    if not items:
        return ()
    ostr = [int(s) * itemsize for s in dev_out.stride()]
    results: list = [None] * len(getters)
    direct = _direct(pipe)
    s0 = spec.shape[0]
    cstr = _scratch_strides(spec, itemsize)
    slot_bytes = cstr[0] * s0
    per = _slots(spec, len(getters))
    progs, groups, keep = [], [], []
    with torch.cuda.device(device):
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        table = ix.build_table(cstr, ostr, False)
        for at in range(0, len(getters), per):
            idx = list(range(at, min(at + per, len(getters))))
            tabs = SelectTables(itemsize, tensor_extent(scratch), tensor_extent(dev_out))
            boxes = []
            for j, k in enumerate(idx):
                it = items[k]
                boxes.append((getters[k], spec, tuple(slice(lo, hi) for lo, hi in it.box), _slot_sel(it.box, j, s0),
                              False))
                tabs.add_product(it.dims, j * slot_bytes, cstr, ostr)
            if direct:
                p = pipe.prepare_read(boxes, scratch)
                p.launch()
                progs.append(p)
                groups.append(idx)
            else:
                for i, r in zip(idx, pipe.read_sync(boxes, scratch)):
                    results[i] = r
            keep.append(tabs.launch(scratch, dev_out, device, table=table))
        if progs:  # ONE readback of every launch's error and verdict words, after the last gather
            for i, r in enumerate(ProgramGroup(progs, groups, len(getters)).results_fast()):
                if r is not None:
                    results[i] = r
    del keep, table
    return tuple(results)


def write_axes(pipe, getters, spec, ix, value, partial_encode: bool = True) -> None:
    """An orthogonal write planned on the device: the box of every touched
    chunk (_write_box's rule on the narrowed box) is decoded into its slot (a
    missing chunk gives fill, a CRC mismatch raises before anything of its
    sub-batch is stored), k_select_copy scatters value into the slots, and the
    boxes are written back through the basic write path.  value: a scalar
    (equal values racing to one address), or an array of shape ix.shape with
    an indexer built with keep_last (only the last occurrence of a repeated
    index along an axis has a pair)."""
    from .buffer import torch_dtype
    from .pipeline import _resolve_value, _torch
    from .writer import _value_tensor

    torch = _torch()
    items = _axes_setup(pipe, spec, ix, len(getters))
    value = _resolve_value(value)
    scalar = (isinstance(value, torch.Tensor) and value.dim() == 0) or \
        (not isinstance(value, torch.Tensor) and np.ndim(value) == 0)
    if not scalar and not ix.keep_last:
        raise ValueError("an array value through a device-planned orthogonal selection needs keep_last planning")
    if not items:
        return
    device = ix.device
    itemsize = np.dtype(spec.dtype).itemsize
    with torch.cuda.device(device):
        v = _value_tensor(value, spec.dtype, device)
        v = v.reshape(1) if scalar else v
        if not scalar and tuple(v.shape) != tuple(ix.shape):
            raise ValueError(f"value of shape {tuple(v.shape)} for a selection of shape {tuple(ix.shape)}")
        vstr = None if scalar else [int(s) * itemsize for s in v.stride()]
        s0 = spec.shape[0]
        cstr = _scratch_strides(spec, itemsize)
        slot_bytes = cstr[0] * s0
        per = _slots(spec, len(getters))
        direct = _direct(pipe)
        scratch = torch.empty((per * s0,) + tuple(spec.shape[1:]), dtype=torch_dtype(spec.dtype), device=device)
        table = ix.build_table(cstr, vstr, True)
        for at in range(0, len(getters), per):
            rbatch, wbatch = [], []
            tabs = SelectTables(itemsize, tensor_extent(v), tensor_extent(scratch))
            for j, k in enumerate(range(at, min(at + per, len(getters)))):
                it = items[k]
                box, complete = _write_box(pipe, spec, Normalized([], it.box, it.total))
                csel = tuple(slice(lo, hi) for lo, hi in box)
                osel = _slot_sel(box, j, s0)
                rbatch.append((getters[k], spec, csel, osel, False))
                wbatch.append((getters[k], spec, csel, osel, complete))
                tabs.add_product(it.dims, j * slot_bytes, cstr, vstr, write=True)
            if direct:
                p = pipe.prepare_read(rbatch, scratch)
                p.launch()
                up = tabs.launch(v, scratch, device, table=table)
                p.results_fast()  # a checksum mismatch raises here: nothing stored yet
                del up
            else:
                pipe.read_sync(rbatch, scratch)
                tabs.launch(v, scratch, device, table=table)
            pipe._write_sync(wbatch, scratch, (), partial_encode)
        del table
