"""Coordinate and mask selections whose indices are DEVICE tensors, planned on
the GPU.

CoordinateIndexer (indexing.py here; src/zarr/core/indexing.py:1171-1350 in
the reference) wraps, bounds-checks and groups every point on the host and
fancy.SelectTables builds and uploads a pair table twice the size of the
coordinates.  With the coordinates already in HBM none of that needs the
host: k_points_count (csrc/points.hip) counts the points of every chunk and
range-checks them, the host reads the counts and one error word back -- the
route's only synchronisation before the decode -- and k_points_fill writes the
grouped (A, B) pair table k_select_copy consumes (fancy.read_points /
write_points).  What stays on the host is per touched chunk, never per point.

This is zarr_hip.Array API: zarr's own indexers hand the pipeline numpy.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N

# Past these the device route is not taken (Array serves the selection with a
# host copy of the indices); named in include/zarrhip.h.
MAX_POINTS = N.POINTS_MAX_N
MAX_DIM = N.POINTS_MAX_DIM
MAX_GRID = N.POINTS_MAX_GRID


class PointsLimit(NotImplementedError):
    """The selection is past a limit of the device route; the caller serves
    it with a host copy of the indices."""


def _torch():
    import torch

    return torch


def is_device_tensor(x) -> bool:
    torch = _torch()
    return isinstance(x, torch.Tensor) and x.is_cuda


def has_device_index(selection) -> bool:
    """The selection is, or holds, a device tensor."""
    import sys

    if "torch" not in sys.modules:
        return False
    if isinstance(selection, tuple):
        return any(is_device_tensor(s) for s in selection)
    return is_device_tensor(selection)


def check_unmixed(selection) -> None:
    """A selection with a device tensor holds only device tensors and Python
    integers: numpy arrays, lists and host tensors next to them raise."""
    torch = _torch()
    sel = selection if isinstance(selection, tuple) else (selection,)
    for s in sel:
        if isinstance(s, (np.ndarray, list)) or (isinstance(s, torch.Tensor) and not s.is_cuda):
            raise TypeError("a selection mixes device tensors with host indices "
                            f"({type(s).__name__}): give every index on the device, or every index on the host")


def within_limits(n: int, shape, chunk_shape) -> bool:
    grid = 1
    for s, c in zip(shape, chunk_shape):
        if s < 1 or s > MAX_DIM or c < 1:
            return False
        grid *= -(-s // c)
    return n <= MAX_POINTS and grid <= MAX_GRID and 1 <= len(shape) <= N.MAX_DIMS


def points_geom(shape, chunk_shape, slot_strides=None, pair_stride: int = 0, write: bool = False) -> np.ndarray:
    """zhip_points_geom (include/zarrhip.h) as a 0-d structured array."""
    g = np.zeros((), N.POINTS_GEOM_DT)
    nd = len(shape)
    g["ndim"] = nd
    g["write"] = 1 if write else 0
    g["pair_stride"] = pair_stride
    for d, (s, c) in enumerate(zip(shape, chunk_shape)):
        g["shape"][d] = s
        g["chunk"][d] = c
        g["div"][d] = N.fdiv(c)
        g["grid"][d] = -(-s // c)
        g["slot_stride"][d] = 0 if slot_strides is None else slot_strides[d]
    return g


def _coord_ptrs(coords):
    return (ctypes.c_void_p * len(coords))(*[c.data_ptr() for c in coords])


class DeviceCoordinateIndexer:
    """CoordinateIndexer for one integer device tensor per dimension (Python
    integers allowed among them).  Construction launches k_points_count and
    reads the per-chunk counts and the error word back in one copy; an index
    out of range raises the host indexer's IndexError and nothing further is
    launched.

    shape / sel_shape / drop_axes as CoordinateIndexer; chunk_rixs, counts and
    first: the touched chunks' row-major grid indices, their point counts and
    the index of each one's first pair in the table; chunk_coords(): their
    grid coordinates."""

    drop_axes = ()

    def __init__(self, selection, shape, chunk_shape):
        torch = _torch()
        from .pipeline import _stream_handle

        sel = selection if isinstance(selection, tuple) else (selection,)
        check_unmixed(sel)
        tensors = [s for s in sel if isinstance(s, torch.Tensor)]
        bad = len(sel) != len(shape) or not tensors
        for s in sel:
            if isinstance(s, torch.Tensor):
                bad = bad or s.dtype in (torch.bool,) or s.is_floating_point() or s.is_complex()
            else:
                bad = bad or not (isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)))
        if bad:
            raise IndexError("invalid coordinate selection; expected one integer (coordinate) array per dimension "
                             f"of the target array, got {selection!r}")
        devices = {t.device for t in tensors}
        if len(devices) != 1:
            raise ValueError(f"the coordinate tensors of one selection are on different devices: {sorted(map(str, devices))}")
        self.device = device = tensors[0].device
        self.array_shape = tuple(int(s) for s in shape)
        self.chunk_shape = tuple(int(c) for c in chunk_shape)
        # plumbing: broadcast, flatten, contiguous int64
        full = [s if isinstance(s, torch.Tensor) else torch.tensor([int(s)], dtype=torch.int64, device=device)
                for s in sel]
        full = torch.broadcast_tensors(*full)  # raises when the coordinate arrays do not match
        self.sel_shape = tuple(full[0].shape) or (1,)
        self.coords = [t.reshape(-1).to(torch.int64).contiguous() for t in full]
        self.n = n = int(self.coords[0].numel())
        self.shape = (n,)
        self.grid_shape = tuple(-(-s // c) for s, c in zip(self.array_shape, self.chunk_shape))
        n_chunks = int(np.prod(self.grid_shape))
        if not within_limits(n, self.array_shape, self.chunk_shape):
            raise PointsLimit("a device-planned point selection past its limits (include/zarrhip.h: "
                              "ZHIP_POINTS_MAX_N / _MAX_DIM / _MAX_GRID)")
        if n == 0:
            counts = np.zeros(n_chunks, np.int64)
        else:
            geom = points_geom(self.array_shape, self.chunk_shape)
            with torch.cuda.device(device):
                words = torch.zeros(n_chunks + 1, dtype=torch.int32, device=device)  # [counts ..., error word]
                N.check(N.lib().zhip_points_count(geom.ctypes.data, _coord_ptrs(self.coords), n, words.data_ptr(),
                                                  words.data_ptr() + 4 * n_chunks, _stream_handle(device)),
                        "zhip_points_count")
                back = words.cpu().numpy().view(np.uint32)  # the ONE readback (synchronises)
            err = int(back[n_chunks])
            if err:
                d = (err & -err).bit_length() - 1  # the lowest failing dimension
                raise IndexError(f"index out of bounds for dimension with length {self.array_shape[d]}")
            counts = back[:n_chunks].astype(np.int64)
        self.chunk_rixs = np.nonzero(counts)[0]
        self.counts = counts[self.chunk_rixs]
        first = np.cumsum(counts) - counts
        self.first = first[self.chunk_rixs]
        self._first_all = first.astype(np.uint32)

    def chunk_coords(self) -> list:
        mixs = np.unravel_index(self.chunk_rixs, self.grid_shape)
        return [tuple(int(m[i]) for m in mixs) for i in range(len(self.chunk_rixs))]

    def build_table(self, slot_strides, pair_stride: int, write: bool):
        """The whole selection's pair table, once (k_points_fill on torch's
        current stream): an (n, 2) int64 device tensor.  Sub-batches differ
        only in their items."""
        torch = _torch()
        from .pipeline import _stream_handle, _upload

        device = self.device
        geom = points_geom(self.array_shape, self.chunk_shape, slot_strides, pair_stride, write)
        table = torch.empty((max(self.n, 1), 2), dtype=torch.int64, device=device)
        first = _upload(self._first_all, device)
        cursor = torch.zeros(len(self._first_all), dtype=torch.int32, device=device)
        N.check(N.lib().zhip_points_fill(geom.ctypes.data, _coord_ptrs(self.coords), self.n, first.data_ptr(),
                                         cursor.data_ptr(), table.data_ptr(), _stream_handle(device)),
                "zhip_points_fill")
        return table


class DeviceMaskIndexer(DeviceCoordinateIndexer):
    """MaskIndexer for a device Boolean tensor of the array's shape: its
    nonzero coordinates (torch.nonzero, plumbing), then the same path."""

    def __init__(self, selection, shape, chunk_shape):
        torch = _torch()
        sel = selection if isinstance(selection, tuple) else (selection,)
        check_unmixed(sel)
        if len(sel) != 1 or not isinstance(sel[0], torch.Tensor) or sel[0].dtype != torch.bool or \
                tuple(sel[0].shape) != tuple(shape):
            raise IndexError("invalid mask selection; expected one Boolean (mask)array with the same shape as the "
                             f"target array, got {sel!r}")
        super().__init__(torch.nonzero(sel[0], as_tuple=True), shape, chunk_shape)


def to_host(selection):
    """A host copy of a device selection (past the device route's limits)."""
    torch = _torch()
    sel = selection if isinstance(selection, tuple) else (selection,)
    host = tuple(s.cpu().numpy() if isinstance(s, torch.Tensor) else s for s in sel)
    return host if isinstance(selection, tuple) else host[0]
