"""Orthogonal selections whose index arrays are DEVICE tensors, planned on the
GPU one axis at a time.

OrthogonalIndexer (indexing.py here; src/zarr/core/indexing.py:625-996 in the
reference) wraps, bounds-checks, groups and slices every index of an integer
array on the host (IntArrayDimIndexer, :732-847).  With the indices already in
HBM none of that needs the host: per tensor axis k_axis_count (csrc/axis.hip)
counts the indices of every chunk along the axis, range-checks them and folds
the smallest and largest in-chunk index; the host reads every axis' words and
one error word back in ONE copy -- the route's only synchronisation before the
decode -- and k_axis_fill writes the axis' grouped (A, B) pairs into the
selection's table, which k_select_copy consumes (fancy.read_axes /
write_axes).  Slices and integers are projected on the host exactly as the
host indexer does.  What stays on the host is per touched chunk, never per
index.

The box of an item is the product of its per-axis ranges (the read back
minimum .. maximum for tensor axes), so only that region of a chunk -- only
the touched inner chunks of a shard -- is decoded.

A write with an array value keeps the LAST occurrence of a repeated index
along each axis (numpy's a[np.ix_(...)] = v): k_axis_last marks the winners
and only they are counted and filled.

This is zarr_hip.Array API: zarr's own indexers hand the pipeline numpy.
"""

from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .fancy import AffineDim, TableDim
from .indexing import _ortho_dim, _replace_ellipsis, is_integer
from .points import PointsLimit, _torch, check_unmixed

# Past these the device route is not taken (Array serves the selection with a
# host copy of the indices); named in include/zarrhip.h.
MAX_N = N.AXIS_MAX_N
MAX_LEN = N.AXIS_MAX_LEN
MAX_GRID = N.AXIS_MAX_GRID
LAST_MAX_LEN = N.AXIS_LAST_MAX_LEN

# Device -> host copies of planning words, one per planned selection (tests
# hold it to exactly that).
READBACKS = 0


def _is_index_tensor(x) -> bool:
    torch = _torch()
    return isinstance(x, torch.Tensor) and x.is_cuda


def is_pure_fancy(selection, ndim: int) -> bool:
    """is_pure_fancy_indexing (indexing.py:270-307) with a device tensor
    counting as an array: Array.__getitem__ sends these to vindex."""
    torch = _torch()
    if _is_index_tensor(selection):
        return selection.dtype == torch.bool or ndim == 1

    def ints(e) -> bool:
        return _is_index_tensor(e) and e.dtype != torch.bool

    no_slicing = (isinstance(selection, tuple) and len(selection) == ndim
                  and not any(isinstance(e, slice) or e is Ellipsis for e in selection))
    return no_slicing and all(is_integer(e) or ints(e) for e in selection) and any(ints(e) for e in selection)


def is_pure_orthogonal(selection, ndim: int) -> bool:
    """is_pure_orthogonal_indexing (indexing.py:310-330) with a device tensor
    counting as an array: Array.__getitem__ sends these to oindex."""
    if not ndim:
        return False
    sel = selection if isinstance(selection, tuple) else (selection,)
    if len(sel) == ndim and all(_is_index_tensor(s) for s in sel):
        return True
    return (len(sel) <= ndim and sum(_is_index_tensor(s) for s in sel) <= 1
            and all(_is_index_tensor(s) or is_integer(s) or isinstance(s, slice) for s in sel))


def axis_geom(length: int, chunk: int, err_bit: int = 1, slot_stride: int = 0, lin_stride: int = 0,
              table_off: int = 0, write: bool = False) -> np.ndarray:
    """zhip_axis_geom (include/zarrhip.h) as a 0-d structured array."""
    g = np.zeros((), N.AXIS_GEOM_DT)
    g["length"] = length
    g["chunk"] = chunk
    g["div"] = N.fdiv(chunk)
    g["grid"] = -(-length // chunk)
    g["write"] = 1 if write else 0
    g["err_bit"] = err_bit
    g["slot_stride"] = slot_stride
    g["lin_stride"] = lin_stride
    g["table_off"] = table_off
    return g


def within_limits(n: int, length: int, chunk: int, keep_last: bool = False) -> bool:
    if length < 1 or length > MAX_LEN or chunk < 1 or n > MAX_N or -(-length // chunk) > MAX_GRID:
        return False
    return not keep_last or length <= LAST_MAX_LEN


@dataclass
class AxisItem:
    coords: tuple
    dims: list      # AffineDim | TableDim per array dimension
    box: list       # per chunk axis (lo, hi)
    total: int


class DeviceOrthogonalIndexer:
    """OrthogonalIndexer for a selection of device tensors, slices, Python
    integers and Ellipsis over a regular grid.  1-d integer tensors of any
    integer dtype; a 1-d Boolean tensor of the axis length becomes its nonzero
    indices (torch.nonzero, plumbing).  Construction launches k_axis_count for
    every tensor axis (after k_axis_last with keep_last) and reads all words
    back in one copy; an index out of range raises the host indexer's
    IndexError for the lowest failing axis and nothing further is launched.

    shape / drop_axes as OrthogonalIndexer; items(): one AxisItem per touched
    chunk; build_table(): the selection's pair table."""

    def __init__(self, selection, shape, chunk_shape, keep_last: bool = False):
        global READBACKS
        torch = _torch()
        from .pipeline import _stream_handle

        check_unmixed(selection)
        self.array_shape = tuple(int(s) for s in shape)
        self.chunk_shape = tuple(int(c) for c in chunk_shape)
        self.keep_last = bool(keep_last)
        sel = _replace_ellipsis(selection, self.array_shape)
        nd = len(self.array_shape)
        if nd > N.MAX_DIMS:
            raise PointsLimit(f"a device-planned orthogonal selection of more than {N.MAX_DIMS} dimensions")
        # per dimension: an int64 index tensor, or the host projections of a slice / an integer
        self.index: list = [None] * nd
        proj: list = [None] * nd
        counts_of: list = [0] * nd
        is_int = [False] * nd
        for d, (s, L, C) in enumerate(zip(sel, self.array_shape, self.chunk_shape)):
            if isinstance(s, torch.Tensor):
                if s.dtype == torch.bool:
                    if s.dim() != 1:
                        raise IndexError("Boolean arrays in an orthogonal selection must be 1-dimensional only")
                    if s.shape[0] != L:
                        raise IndexError(f"Boolean array has the wrong length for dimension; expected {L}, "
                                         f"got {s.shape[0]}")
                    x = torch.nonzero(s).reshape(-1)  # plumbing; synchronises on its own
                elif s.is_floating_point() or s.is_complex():
                    raise IndexError("unsupported selection item for orthogonal indexing; expected integer, slice, "
                                     f"integer array or Boolean array, got {type(s)!r} of dtype {s.dtype}")
                else:
                    if s.dim() != 1:
                        raise IndexError("integer arrays in an orthogonal selection must be 1-dimensional only")
                    x = s
                self.index[d] = x.to(torch.int64).contiguous()
                counts_of[d] = int(x.numel())
            else:
                proj[d], counts_of[d], is_int[d] = _ortho_dim(s, L, C)
        self.tensor_axes = [d for d in range(nd) if self.index[d] is not None]
        if not self.tensor_axes:
            raise TypeError("a device-planned orthogonal selection holds at least one device tensor")
        devices = {self.index[d].device for d in self.tensor_axes}
        if len(devices) != 1:
            raise ValueError(f"the index tensors of one selection are on different devices: {sorted(map(str, devices))}")
        self.device = device = self.index[self.tensor_axes[0]].device
        self.shape = tuple(counts_of[d] for d in range(nd) if not is_int[d])
        self.drop_axes = tuple(d for d in range(nd) if is_int[d])
        out_axis, at = [None] * nd, 0
        for d in range(nd):
            if not is_int[d]:
                out_axis[d] = at
                at += 1
        self.out_axis = out_axis
        for d in self.tensor_axes:
            if not within_limits(counts_of[d], self.array_shape[d], self.chunk_shape[d], self.keep_last):
                raise PointsLimit("a device-planned orthogonal selection past its limits (include/zarrhip.h: "
                                  "ZHIP_AXIS_MAX_N / _MAX_LEN / _MAX_GRID / _LAST_MAX_LEN)")
        self.n = {d: counts_of[d] for d in self.tensor_axes}
        self.table_off, at = {}, 0
        for d in self.tensor_axes:
            self.table_off[d] = at
            at += self.n[d]
        self.table_pairs = at
        self.size = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self._last: dict = {}
        self._first: dict = {}
        self._items = None
        self._dims: list = [None] * nd
        for d in range(nd):
            if proj[d] is not None:
                self._dims[d] = [(int(c), self._affine(cs, os, out_axis[d])) for c, cs, os in proj[d]]
        if self.size == 0:  # nothing selected: nothing launched
            for d in self.tensor_axes:
                self._dims[d] = []
            return
        grids = {d: -(-self.array_shape[d] // self.chunk_shape[d]) for d in self.tensor_axes}
        base, at = {}, 0
        for d in self.tensor_axes:
            base[d] = at
            at += 3 * grids[d]
        with torch.cuda.device(device):
            stream = _stream_handle(device)
            words = torch.zeros(at + 1, dtype=torch.int32, device=device)  # per axis [counts, lo, hi] ..., error word
            p = words.data_ptr()
            for d in self.tensor_axes:
                g = axis_geom(self.array_shape[d], self.chunk_shape[d], err_bit=1 << d)
                x, G = self.index[d], grids[d]
                last = 0
                if self.keep_last:
                    self._last[d] = torch.zeros(self.array_shape[d], dtype=torch.int32, device=device)
                    last = self._last[d].data_ptr()
                    N.check(N.lib().zhip_axis_last(g.ctypes.data, x.data_ptr(), self.n[d], last, stream), "zhip_axis_last")
                at_d = p + 4 * base[d]
                N.check(N.lib().zhip_axis_count(g.ctypes.data, x.data_ptr(), self.n[d], last or None, at_d, at_d + 4 * G,
                                                at_d + 8 * G, p + 4 * at, stream), "zhip_axis_count")
            back = words.cpu().numpy().view(np.uint32)  # the ONE readback (synchronises)
            READBACKS += 1
        err = int(back[at])
        if err:
            d = (err & -err).bit_length() - 1  # the lowest failing axis
            raise IndexError(f"index out of bounds for dimension with length {self.array_shape[d]}")
        for d in self.tensor_axes:
            G, C = grids[d], self.chunk_shape[d]
            counts = back[base[d]:base[d] + G].astype(np.int64)
            lo = C - 1 - back[base[d] + G:base[d] + 2 * G].astype(np.int64)
            hi = back[base[d] + 2 * G:base[d] + 3 * G].astype(np.int64)
            first = np.cumsum(counts) - counts
            self._first[d] = first.astype(np.uint32)
            self._dims[d] = [(int(c), TableDim(int(counts[c]), self.table_off[d] + int(first[c]), int(lo[c]), int(hi[c]),
                                               self.n[d], out_axis[d])) for c in np.nonzero(counts)[0]]

    @staticmethod
    def _affine(csel, osel, out_axis) -> AffineDim:
        if osel is None:  # an integer
            return AffineDim(1, int(csel), 0, None, 0)
        step = csel.step or 1
        return AffineDim(len(range(csel.start, csel.stop, step)), int(csel.start), int(step), out_axis, int(osel.start))

    def items(self) -> list:
        """One AxisItem per touched chunk: the product of the touched chunks
        per axis, in row-major order of the chunk coordinates."""
        if self._items is None:
            out = []
            for combo in itertools.product(*self._dims):
                dims = [c[1] for c in combo]
                total = 1
                for D in dims:
                    total *= D.count
                if total:
                    out.append(AxisItem(tuple(c[0] for c in combo), dims, [D.box for D in dims], total))
            self._items = out
        return self._items

    def build_table(self, slot_strides, lin_strides, write: bool):
        """The whole selection's pair table, once (k_axis_fill per tensor axis
        on torch's current stream): a (table_pairs, 2) int64 device tensor.
        slot_strides: byte strides of a chunk-shaped slot per array dimension;
        lin_strides: byte strides of out / value per selected dimension (None:
        a scalar value).  Sub-batches differ only in their items."""
        torch = _torch()
        from .pipeline import _stream_handle, _upload

        device = self.device
        table = torch.empty((max(self.table_pairs, 1), 2), dtype=torch.int64, device=device)
        stream = _stream_handle(device)
        keep = []
        for d in self.tensor_axes:
            lin = 0 if lin_strides is None else int(lin_strides[self.out_axis[d]])
            g = axis_geom(self.array_shape[d], self.chunk_shape[d], 1 << d, int(slot_strides[d]), lin,
                          self.table_off[d], write)
            first = _upload(self._first[d], device)
            cursor = torch.zeros(len(self._first[d]), dtype=torch.int32, device=device)
            last = self._last[d].data_ptr() if self.keep_last else None
            N.check(N.lib().zhip_axis_fill(g.ctypes.data, self.index[d].data_ptr(), self.n[d], last, first.data_ptr(),
                                           cursor.data_ptr(), table.data_ptr(), self.table_pairs, stream),
                    "zhip_axis_fill")
            keep.append((first, cursor))
        del keep  # stream-ordered: the caching allocator reuses them behind the launches
        return table
