"""A thin Array driver over HipCodecPipeline (the caller side of the boundary).

Restates only what the hot path needs from the reference's Array layer:
  ArrayV3Metadata (zarr.json)      src/zarr/core/metadata/v3.py:464-613 (minimal reader/writer)
  create_codec_pipeline             src/zarr/core/array.py:221-265
  _get_selection                    src/zarr/core/array.py:5393-5514
  _set_selection                    src/zarr/core/array.py:5563-5675
  chunk key encodings               src/zarr/core/chunk_key_encodings.py:87-88 (default, "c/0/0"),
                                    103-105 (v2, "0.0"; "0" for 0-d)
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import axes, buffer, points
from .codecs import BytesCodec, Crc32cCodec, ShardingCodec, parse_codecs
from .grid import ChunkGrid
from .indexing import (CoordinateIndexer, MaskIndexer, OrthogonalIndexer, basic_projections, chunk_batch,
                       is_bool_array, is_pure_fancy_indexing, is_pure_orthogonal_indexing)
from .pipeline import BasicBatch, DecodeProgram, HipCodecPipeline
from .spec import ArrayConfig, ArraySpec
from .store import DeviceStore, StorePath


def _float_to_json(f: float):
    """float_to_json_v3 (src/zarr/core/dtype/npy/common.py:256-293)."""
    if math.isnan(f):
        return "NaN"
    if math.isinf(f):
        return "Infinity" if f > 0 else "-Infinity"
    return f


def _fill_from_json(v, dtype: np.dtype):
    if dtype.kind == "c":
        # [re, im], each a number or "NaN" / "Infinity" / "-Infinity"
        # (complex_float_from_json_v3, common.py:351-365); the components are
        # set one by one: complex(re, im) arithmetic is not involved, so a
        # -0.0 or NaN component keeps its sign
        if not isinstance(v, (list, tuple)) or len(v) != 2:
            raise ValueError(f"a complex fill value is [real, imag] in zarr.json, got {v!r}")
        a = np.zeros((), dtype=dtype)
        a.real = float(v[0])
        a.imag = float(v[1])
        return a[()]
    if isinstance(v, str):
        return np.array(float(v), dtype=dtype)[()]
    return np.array(v, dtype=dtype)[()]


def _fill_to_json(v, dtype: np.dtype):
    a = np.asarray(v, dtype=dtype)
    if dtype.kind == "c":
        # complex_float_to_json_v3 (common.py:296-312)
        return [_float_to_json(float(a.real)), _float_to_json(float(a.imag))]
    if dtype.kind == "f":
        return _float_to_json(float(a))
    if dtype.kind == "b":
        return bool(a)
    return int(a)


def _selection_key(selection):
    """A hashable image of a basic selection (ints, unit or strided slices,
    Ellipsis), None for anything else (arrays, masks: not memoised)."""
    sel = selection if isinstance(selection, tuple) else (selection,)
    out = []
    for s in sel:
        if s is Ellipsis:
            out.append("...")
        elif isinstance(s, slice):
            if not all(v is None or isinstance(v, (int, np.integer)) for v in (s.start, s.stop, s.step)):
                return None
            out.append(("s", s.start, s.stop, s.step))
        elif isinstance(s, (int, np.integer)) and not isinstance(s, bool):
            out.append(int(s))
        else:
            return None
    return tuple(out)


@dataclass
class ArrayMetadata:
    shape: tuple[int, ...]
    chunk_shape: tuple[int, ...]
    dtype: np.dtype
    fill_value: Any
    codecs: tuple
    separator: str = "/"
    attributes: dict = field(default_factory=dict)
    key_encoding: str = "default"  # or "v2"
    # a rectilinear grid (chunk_grids.py:399-546); None: the regular grid of
    # chunk_shape.  With a rectilinear grid chunk_shape is the placeholder
    # (1,) * ndim zarr evolves the pipeline with (array.py:237-247)
    grid: ChunkGrid | None = None

    @property
    def chunk_grid(self) -> ChunkGrid:
        if self.grid is not None:
            return self.grid
        return ChunkGrid.from_sizes(self.shape, tuple(self.chunk_shape))

    @property
    def is_regular(self) -> bool:
        return self.grid is None or self.grid.is_regular

    def to_json(self) -> dict:
        return {
            "zarr_format": 3, "node_type": "array", "shape": list(self.shape),
            "data_type": np.dtype(self.dtype).name,
            "chunk_grid": self.chunk_grid.to_json() if self.grid is not None else
            {"name": "regular", "configuration": {"chunk_shape": list(self.chunk_shape)}},
            "chunk_key_encoding": {"name": self.key_encoding, "configuration": {"separator": self.separator}},
            "fill_value": _fill_to_json(self.fill_value, np.dtype(self.dtype)),
            "codecs": [c.to_dict() for c in self.codecs],
            "attributes": self.attributes,
        }

    @classmethod
    def from_json(cls, d: dict) -> "ArrayMetadata":
        if d.get("zarr_format") != 3 or d.get("node_type") != "array":
            raise ValueError("not a zarr v3 array")
        g = ChunkGrid.from_json(tuple(d["shape"]), d["chunk_grid"])
        dt = np.dtype(d["data_type"])
        cke = d.get("chunk_key_encoding", {"name": "default"})
        name = cke.get("name", "default")
        if name not in ("default", "v2"):
            raise NotImplementedError(f"chunk key encoding {name!r}")
        sep = (cke.get("configuration") or {}).get("separator", "/" if name == "default" else ".")
        chunk_shape = g.chunk_shape if g.is_regular else (1,) * g.ndim
        return cls(tuple(d["shape"]), chunk_shape, dt, _fill_from_json(d["fill_value"], dt),
                   tuple(parse_codecs(d["codecs"])), sep, d.get("attributes", {}), name,
                   None if g.is_regular else g)

    def chunk_key(self, coords) -> str:
        if self.key_encoding == "v2":
            k = self.separator.join(str(int(c)) for c in coords)
            return k or "0"
        return self.separator.join(map(str, ("c",) + tuple(int(c) for c in coords)))

    @property
    def grid_shape(self) -> tuple[int, ...]:
        if self.grid is not None:
            return self.grid.grid_shape
        return tuple(-(-s // c) for s, c in zip(self.shape, self.chunk_shape))


class Array:
    """zarr v3 array on a store, read/written through HipCodecPipeline."""

    def __init__(self, store_path: StorePath, metadata: ArrayMetadata,
                 config: ArrayConfig = ArrayConfig()):
        self.store_path = store_path
        buffer.require_device_dtype(metadata.dtype)
        self.metadata = metadata
        self.config = config
        # (rectilinear grids: the pipeline is evolved with the placeholder
        # shape, every chunk then carries its own spec -- array.py:237-247,
        # 5373-5390)
        self.spec = ArraySpec(metadata.chunk_shape, metadata.dtype, metadata.fill_value, config)
        self.codec_pipeline = HipCodecPipeline.from_codecs(metadata.codecs).evolve_from_array_spec(
            self.spec)
        if metadata.is_regular:
            self.codec_pipeline.validate(shape=metadata.shape, chunk_shape=metadata.chunk_shape)
        else:
            self.codec_pipeline.validate(shape=metadata.shape, chunk_grid=metadata.grid)
        self._programs: dict = {}

    # ------------------------------------------------------------ construction
    @classmethod
    def create(cls, store, shape, chunks, dtype, fill_value=0, codecs=None, *, shards=None,
               inner_codecs=None, index_location="end", path: str = "",
               config: ArrayConfig = ArrayConfig()) -> "Array":
        dtype = np.dtype(dtype)
        buffer.require_device_dtype(dtype)  # (refused by name before zarr.json is written)
        if codecs is None:
            codecs = (BytesCodec(endian="little" if dtype.itemsize > 1 else None),)
        codecs = tuple(parse_codecs(codecs))
        chunk_shape = tuple(c if isinstance(c, int) else tuple(c) for c in chunks)
        if shards is not None:
            inner = tuple(parse_codecs(inner_codecs)) if inner_codecs is not None else codecs
            codecs = (ShardingCodec(chunk_shape=chunk_shape, codecs=inner,
                                    index_location=index_location),)
            chunk_shape = tuple(c if isinstance(c, int) else tuple(c) for c in shards)
        # nested edge lists: a rectilinear grid (regular when they reduce to one)
        grid = None
        if any(not isinstance(c, int) for c in chunk_shape):
            grid = ChunkGrid.from_sizes(tuple(shape), chunk_shape)
            chunk_shape = grid.chunk_shape if grid.is_regular else (1,) * len(chunk_shape)
            grid = None if grid.is_regular else grid
        md = ArrayMetadata(tuple(shape), chunk_shape, dtype, np.array(fill_value, dtype)[()],
                           codecs, grid=grid)
        sp = StorePath(store, path)
        key = f"{path}/zarr.json" if path else "zarr.json"
        store.set_sync(key, json.dumps(md.to_json()).encode())
        return cls(sp, md, config)

    @classmethod
    def open(cls, store, path: str = "", config: ArrayConfig = ArrayConfig()) -> "Array":
        key = f"{path}/zarr.json" if path else "zarr.json"
        raw = store.get_sync(key)
        if raw is None:
            raise FileNotFoundError(key)
        d = json.loads(bytes(raw))
        return cls(StorePath(store, path), ArrayMetadata.from_json(d), config)

    # ---------------------------------------------------------------- helpers
    @property
    def shape(self):
        return self.metadata.shape

    @property
    def dtype(self):
        return self.metadata.dtype

    @property
    def chunks(self):
        """The chunk shape; only defined for regular chunk grids -- a
        rectilinear grid raises NotImplementedError, as the reference's
        Array.chunks does (src/zarr/core/array.py:849-862, 2024-2036)."""
        if not self.metadata.is_regular:
            raise NotImplementedError("chunks is only defined for arrays using a regular chunk grid; "
                                      "this array uses a rectilinear chunk grid")
        return self.metadata.chunk_shape

    def _key(self, coords) -> str:
        k = self.metadata.chunk_key(coords)
        return f"{self.store_path.path}/{k}" if self.store_path.path else k

    def batch_info(self, selection):
        """The CodecPipeline batch of a selection (BasicIndexer's chunk
        projections, src/zarr/core/indexing.py:365-621).  Depends only on the
        metadata and the selection, so basic selections are memoised per array
        (a repeated read skips the indexer: the per-call path)."""
        key = _selection_key(selection)
        cache = self.__dict__.setdefault("_batches", {})
        if key is not None:
            hit = cache.get(key)
            if hit is not None:
                return BasicBatch(hit[0]), hit[1]
        batch, out_shape = self._batch_info(selection)
        if key is not None:
            if len(cache) >= 64:
                cache.pop(next(iter(cache)))
            cache[key] = (tuple(batch), out_shape)
        return BasicBatch(batch), out_shape

    def _batch_info(self, selection):
        md = self.metadata
        if not md.is_regular:
            return self._batch_info_rectilinear(selection)
        rows, out_shape = chunk_batch(selection, self.metadata.shape, self.metadata.chunk_shape)
        store, spec, sep = self.store_path.store, self.spec, self.metadata.separator
        if self.metadata.key_encoding == "v2":
            pre = f"{self.store_path.path}/" if self.store_path.path else ""
            batch = [(StorePath(store, pre + (sep.join(map(str, co)) or "0")), spec, csel, osel, comp)
                     for co, csel, osel, comp in rows]
            return batch, out_shape
        prefix = f"{self.store_path.path}/c" if self.store_path.path else "c"
        batch = [(StorePath(store, sep.join([prefix, *map(str, co)])), spec, csel, osel, comp)
                 for co, csel, osel, comp in rows]
        return batch, out_shape

    def _batch_info_rectilinear(self, selection):
        """_get_selection's batch for a rectilinear grid: one ArraySpec per
        chunk, shape = ChunkGrid[coords].codec_shape (_get_chunk_spec,
        array.py:5373-5390, 5469-5486); specs of equal shape are shared."""
        md = self.metadata
        g = md.grid
        rows, out_shape = chunk_batch(selection, md.shape, g)
        store, sep = self.store_path.store, md.separator
        specs: dict = {}
        batch = []
        for co, csel, osel, comp in rows:
            cs = g.codec_shape(co)
            sp = specs.get(cs)
            if sp is None:
                sp = specs[cs] = ArraySpec(cs, md.dtype, md.fill_value, self.config)
            batch.append((StorePath(store, self._key(co)), sp, csel, osel, comp))
        return batch, out_shape

    # ------------------------------------------------------------------- read
    def prepare_read(self, selection=Ellipsis, out=None, device=None) -> tuple[DecodeProgram, Any]:
        """Plan a selection once; the returned program re-launches without re-planning."""
        import torch

        if self._dispatch(selection) is not None:
            raise NotImplementedError("prepare_read (and hipGraph capture) of an orthogonal, coordinate or mask "
                                      "selection: only basic selections are planned ahead")
        batch, out_shape = self.batch_info(selection)
        if out is None:
            dev = device or getattr(self.store_path.store, "device", None) or torch.device("cuda:0")
            out = buffer.empty(out_shape, self.metadata.dtype, dev, self.config.order)
        prog = self.codec_pipeline.prepare_read(batch, out)
        return prog, out

    def get(self, selection=Ellipsis, out=None, device=None):
        """Device-resident read: returns a torch tensor on the GPU (for
        orthogonal, coordinate and mask selections too: dispatched as
        __getitem__ does)."""
        kind = self._dispatch(selection)
        if kind == "device-oindex":
            return self._get_axes(selection, out, device)
        if kind is not None:
            return self._get_fancy(self._indexer(kind, selection), out, device)
        batch, out_shape = self.batch_info(selection)
        import torch

        if out is None:
            dev = device or getattr(self.store_path.store, "device", None) or torch.device("cuda:0")
            out = buffer.empty(out_shape, self.metadata.dtype, dev, self.config.order)
        if not batch:
            return out
        results = self.codec_pipeline.read_sync(batch, out)
        if not self.config.read_missing_chunks:
            for (bg, *_), r in zip(batch, results):
                if r["status"] == "missing":
                    raise ChunkNotFoundError(f"chunk {bg.path!r} is missing")
        return out

    def __getitem__(self, selection) -> np.ndarray:
        """Host result.  Host-resident stores read into a pinned numpy array:
        the pipeline streams slabs back while later slabs still decode
        (HipCodecPipeline._read_slabs); HBM-resident stores decode on the
        device and copy the result back once."""
        st = self.store_path.store
        kind = self._dispatch(selection)
        if kind == "device-oindex":
            return buffer.to_numpy(self._get_axes(selection), self.metadata.dtype)
        if kind == "device":  # indices on the device: planned there; the result is still a host array
            return buffer.to_numpy(self._get_fancy(self._indexer(kind, selection)), self.metadata.dtype)
        if kind is not None:
            return self._get_fancy_host(self._indexer(kind, selection))
        if isinstance(st, DeviceStore):
            return buffer.to_numpy(self.get(selection), self.metadata.dtype)
        batch, out_shape = self.batch_info(selection)
        out = buffer.empty_pinned(out_shape, self.metadata.dtype, self.config.order)
        if not batch:
            return out
        results = self.codec_pipeline.read_sync(batch, out)
        if not self.config.read_missing_chunks:
            for (bg, *_), r in zip(batch, results):
                if r["status"] == "missing":
                    raise ChunkNotFoundError(f"chunk {bg.path!r} is missing")
        return out

    # ------------------------------------------------------------------ write
    def set(self, selection, value) -> None:
        """Array._set_selection (array.py:5563-5675): value may be a device
        tensor, a numpy array or a scalar."""
        kind = self._dispatch(selection)
        if kind == "device-oindex":
            return self._set_axes(selection, value)
        if kind is not None:
            return self._set_fancy(self._indexer(kind, selection), value)
        batch, out_shape = self.batch_info(selection)
        if not batch:
            return
        import torch

        if not isinstance(value, torch.Tensor):
            a = np.asarray(value, dtype=self.metadata.dtype)
            if a.shape not in ((), tuple(out_shape)):
                a = np.broadcast_to(a, out_shape)
            value = a
        self.codec_pipeline.write_sync(batch, value)

    def __setitem__(self, selection, value) -> None:
        self.set(selection, value)

    # ------------------------------- orthogonal, coordinate and mask selections
    def _dispatch(self, selection):
        """Array.__getitem__'s dispatch (array.py:2635-2641, indexing.py:270-331):
        "vindex", "oindex", or None for a basic selection; for a selection
        that holds device tensors "device" (coordinates or a mask, points.py)
        or "device-oindex" (orthogonal, axes.py)."""
        if _selection_key(selection) is not None:
            return None
        nd = len(self.metadata.shape)
        if points.has_device_index(selection):
            # zarr's order with a device tensor counting as an array: pure fancy
            # first, then pure orthogonal (axes.py); what neither rule admits
            # goes to the coordinate indexer, which raises for it
            if not axes.is_pure_fancy(selection, nd) and axes.is_pure_orthogonal(selection, nd):
                return "device-oindex"
            return "device"
        if is_pure_fancy_indexing(selection, nd):
            return "vindex"
        if is_pure_orthogonal_indexing(selection, nd):
            return "oindex"
        return None

    def _indexer(self, kind: str, selection):
        md = self.metadata
        if not md.is_regular:
            raise NotImplementedError("orthogonal, coordinate and mask selections of a rectilinear chunk grid")
        if kind == "device":
            return self._device_indexer(selection)
        if kind == "oindex":
            return OrthogonalIndexer(selection, md.shape, md.chunk_shape)
        sel = selection if isinstance(selection, tuple) else (selection,)
        first = np.asarray(sel[0]) if isinstance(sel[0], list) else sel[0]
        if len(sel) == 1 and is_bool_array(first) and first.shape == tuple(md.shape):
            return MaskIndexer((first,), md.shape, md.chunk_shape)
        return CoordinateIndexer(selection, md.shape, md.chunk_shape)

    def _fancy_batch(self, indexer) -> list:
        store, spec = self.store_path.store, self.spec
        return [(StorePath(store, self._key(co)), spec, csel, osel, comp) for co, csel, osel, comp in indexer]

    def _check_missing(self, batch, results) -> None:
        if not self.config.read_missing_chunks:
            for (bg, *_), r in zip(batch, results):
                if r["status"] == "missing":
                    raise ChunkNotFoundError(f"chunk {bg.path!r} is missing")

    # --- coordinate and mask selections whose indices are device tensors (points.py)
    def _device_indexer(self, selection, mask: bool | None = None):
        """DeviceMaskIndexer for a Boolean device tensor (vindex's rule: of the
        array's shape), else DeviceCoordinateIndexer.  Past the device route's
        limits: the host indexer over a host copy of the indices."""
        import torch

        md = self.metadata
        chunks = self._regular_chunks()
        points.check_unmixed(selection)
        sel = selection if isinstance(selection, tuple) else (selection,)
        if mask is None:
            mask = (len(sel) == 1 and isinstance(sel[0], torch.Tensor) and sel[0].dtype == torch.bool
                    and tuple(sel[0].shape) == tuple(md.shape))
        try:
            return (points.DeviceMaskIndexer if mask else points.DeviceCoordinateIndexer)(selection, md.shape, chunks)
        except points.PointsLimit:
            host = points.to_host(selection)
            return (MaskIndexer if mask else CoordinateIndexer)(host, md.shape, chunks)

    def _points_getters(self, ix) -> list:
        store = self.store_path.store
        return [StorePath(store, self._key(co)) for co in ix.chunk_coords()]

    def _run_device(self, ix, device=None):
        """The device a selection with device indices runs on: the indices'.
        A store or a caller that names another one raises."""
        import torch

        def index(d):
            d = torch.device(d)
            return torch.cuda.current_device() if d.index is None else d.index

        for what, d in (("device argument", device), ("store", getattr(self.store_path.store, "device", None))):
            if d is not None and (torch.device(d).type != "cuda" or index(d) != index(ix.device)):
                raise ValueError(f"the selection's indices are on {ix.device}, the {what} is on {d}: the indices "
                                 "of a device-planned selection live on the device the array is read on")
        return ix.device

    def _get_points(self, ix, out=None, device=None):
        """A device tensor reshaped to sel_shape; with `out` (a device tensor or
        a host array of the selection's size): out, filled."""
        from .interop import device_tensor, host_array

        dev = self._run_device(ix, device)
        dt = self.metadata.dtype
        target = None
        if out is not None:
            target = device_tensor(out)
            if target is None:
                target = host_array(out)
                if target is None:
                    raise TypeError(f"cannot decode into a {type(out).__name__}")
            size = target.numel() if hasattr(target, "numel") else target.size
            if size != ix.n:
                raise ValueError(f"out holds {size} elements, the selection {ix.n}")
        flat = None
        if target is not None and hasattr(target, "numel") and target.device == dev:
            try:
                flat = target.view(-1)  # decoded in place
            except RuntimeError:
                flat = None
        direct = flat is not None
        if flat is None:
            flat = buffer.empty((ix.n,), dt, dev)
        getters = self._points_getters(ix)
        if getters:
            from . import fancy

            results = fancy.read_points(self.codec_pipeline, getters, self.spec, ix, flat)
            self._check_missing([(g,) for g in getters], results)
        if target is None:
            return flat.reshape(ix.sel_shape)
        if not direct:
            if hasattr(target, "numel"):
                target.copy_(flat.reshape(target.shape))
            else:
                buffer.copy_to_host(flat.reshape(target.shape), target)
        return out

    def _set_points(self, ix, value) -> None:
        import torch

        from . import fancy

        self._run_device(ix)
        if isinstance(value, torch.Tensor):
            if value.numel() == 1:
                value = value.reshape(())
            elif value.numel() != ix.n:
                raise ValueError(f"value of {value.numel()} elements for a selection of {ix.n} points")
            else:
                value = value.reshape(-1)  # point lists: the value is taken flat
        else:
            a = np.asarray(value, dtype=self.metadata.dtype)
            value = a.reshape(()) if a.size == 1 else np.broadcast_to(a.reshape(-1), (ix.n,))
        getters = self._points_getters(ix)
        if getters:
            fancy.write_points(self.codec_pipeline, getters, self.spec, ix, value,
                               distinct=isinstance(ix, points.DeviceMaskIndexer))

    # --- orthogonal selections whose index arrays are device tensors (axes.py)
    def _axes_indexer(self, selection, keep_last: bool):
        """DeviceOrthogonalIndexer; past the device route's limits the host
        OrthogonalIndexer over a host copy of the indices."""
        md = self.metadata
        chunks = self._regular_chunks()
        try:
            return axes.DeviceOrthogonalIndexer(selection, md.shape, chunks, keep_last=keep_last)
        except points.PointsLimit:
            return OrthogonalIndexer(points.to_host(selection), md.shape, chunks)

    def _axes_getters(self, ix) -> list:
        store = self.store_path.store
        return [StorePath(store, self._key(it.coords)) for it in ix.items()]

    def _get_axes(self, selection, out=None, device=None):
        """A device tensor of the selection's shape; with `out` (a device
        tensor, views included, or a host array of that shape): out, filled."""
        from . import fancy
        from .interop import device_tensor, host_array

        ix = self._axes_indexer(selection, keep_last=False)
        if not isinstance(ix, axes.DeviceOrthogonalIndexer):
            return self._get_fancy(ix, out, device)
        dev = self._run_device(ix, device)
        dt = self.metadata.dtype
        target = None
        if out is not None:
            target = device_tensor(out)
            if target is None:
                target = host_array(out)
                if target is None:
                    raise TypeError(f"cannot decode into a {type(out).__name__}")
            if tuple(target.shape) != tuple(ix.shape):
                raise ValueError(f"out of shape {tuple(target.shape)} for a selection of shape {tuple(ix.shape)}")
        direct = target is not None and hasattr(target, "is_cuda") and target.device == dev
        dev_out = target if direct else buffer.empty(ix.shape, dt, dev, self.config.order)
        getters = self._axes_getters(ix)
        if getters:
            results = fancy.read_axes(self.codec_pipeline, getters, self.spec, ix, dev_out)
            self._check_missing([(g,) for g in getters], results)
        if target is None:
            return dev_out
        if not direct:
            if hasattr(target, "is_cuda"):
                target.copy_(dev_out)
            else:
                buffer.copy_to_host(dev_out, target)
        return out

    def _set_axes(self, selection, value) -> None:
        import torch

        from . import fancy

        scalar = value.dim() == 0 if isinstance(value, torch.Tensor) else np.ndim(value) == 0
        # an array value: the last occurrence of a repeated index along an axis wins
        ix = self._axes_indexer(selection, keep_last=not scalar)
        if not isinstance(ix, axes.DeviceOrthogonalIndexer):
            return self._set_fancy(ix, value)
        self._run_device(ix)
        if isinstance(value, torch.Tensor):
            if value.dim() > 0 and tuple(value.shape) != tuple(ix.shape):
                value = value.broadcast_to(ix.shape)
        else:
            a = np.asarray(value, dtype=self.metadata.dtype)
            if a.shape not in ((), tuple(ix.shape)):
                a = np.broadcast_to(a, ix.shape)
            value = a
        getters = self._axes_getters(ix)
        if getters:
            fancy.write_axes(self.codec_pipeline, getters, self.spec, ix, value)

    def _get_fancy(self, indexer, out=None, device=None):
        import torch

        if isinstance(indexer, points.DeviceCoordinateIndexer):
            return self._get_points(indexer, out, device)
        if out is None:
            dev = device or getattr(self.store_path.store, "device", None) or torch.device("cuda:0")
            out = buffer.empty(indexer.shape, self.metadata.dtype, dev, self.config.order)
        batch = self._fancy_batch(indexer)
        if batch:
            self._check_missing(batch, self.codec_pipeline.read_sync(batch, out, indexer.drop_axes))
        return out.reshape(getattr(indexer, "sel_shape", tuple(out.shape)))

    def _get_fancy_host(self, indexer) -> np.ndarray:
        if isinstance(self.store_path.store, DeviceStore):
            return buffer.to_numpy(self._get_fancy(indexer), self.metadata.dtype)
        out = buffer.empty_pinned(indexer.shape, self.metadata.dtype, self.config.order)
        batch = self._fancy_batch(indexer)
        if batch:
            self._check_missing(batch, self.codec_pipeline.read_sync(batch, out, indexer.drop_axes))
        return out.reshape(getattr(indexer, "sel_shape", out.shape))

    def _set_fancy(self, indexer, value) -> None:
        import torch

        if isinstance(indexer, points.DeviceCoordinateIndexer):
            return self._set_points(indexer, value)
        flat = hasattr(indexer, "sel_shape")  # point lists: the value is taken flat (array.py:3596-3610)
        if isinstance(value, torch.Tensor):
            if flat and value.dim() > 0:
                value = value.reshape(-1)
            if value.dim() > 0 and tuple(value.shape) != tuple(indexer.shape):
                value = value.broadcast_to(indexer.shape)
        else:
            a = np.asarray(value, dtype=self.metadata.dtype)
            if flat and a.ndim > 0:
                a = a.reshape(-1)
            if a.shape not in ((), tuple(indexer.shape)):
                a = np.broadcast_to(a, indexer.shape)
            value = a
        batch = self._fancy_batch(indexer)
        if batch:
            self.codec_pipeline.write_sync(batch, value, indexer.drop_axes)

    def get_orthogonal_selection(self, selection, out=None):
        """Array.get_orthogonal_selection: a host result (a device tensor: oindex
        through get(), or pass a device `out`).  Index arrays given as device
        tensors are planned on the device and give a device tensor (axes.py)."""
        if points.has_device_index(selection):
            return self._get_axes(selection, out)
        ix = OrthogonalIndexer(selection, self.metadata.shape, self._regular_chunks())
        return self._get_fancy_host(ix) if out is None else self._get_fancy(ix, out)

    def set_orthogonal_selection(self, selection, value) -> None:
        if points.has_device_index(selection):
            return self._set_axes(selection, value)
        self._set_fancy(OrthogonalIndexer(selection, self.metadata.shape, self._regular_chunks()), value)

    def get_coordinate_selection(self, selection, out=None):
        """Coordinates given as device tensors are planned on the device and
        give a device tensor (points.py); host coordinates a host result."""
        if points.has_device_index(selection):
            return self._get_fancy(self._device_indexer(selection, mask=False), out)
        ix = CoordinateIndexer(selection, self.metadata.shape, self._regular_chunks())
        return self._get_fancy_host(ix) if out is None else self._get_fancy(ix, out)

    def set_coordinate_selection(self, selection, value) -> None:
        if points.has_device_index(selection):
            return self._set_fancy(self._device_indexer(selection, mask=False), value)
        self._set_fancy(CoordinateIndexer(selection, self.metadata.shape, self._regular_chunks()), value)

    def get_mask_selection(self, mask, out=None):
        if points.has_device_index(mask):
            return self._get_fancy(self._device_indexer(mask, mask=True), out)
        ix = MaskIndexer(mask, self.metadata.shape, self._regular_chunks())
        return self._get_fancy_host(ix) if out is None else self._get_fancy(ix, out)

    def set_mask_selection(self, mask, value) -> None:
        if points.has_device_index(mask):
            return self._set_fancy(self._device_indexer(mask, mask=True), value)
        self._set_fancy(MaskIndexer(mask, self.metadata.shape, self._regular_chunks()), value)

    def _regular_chunks(self):
        if not self.metadata.is_regular:
            raise NotImplementedError("orthogonal, coordinate and mask selections of a rectilinear chunk grid")
        return self.metadata.chunk_shape

    @property
    def oindex(self) -> "_OIndex":
        return _OIndex(self)

    @property
    def vindex(self) -> "_VIndex":
        return _VIndex(self)


class _OIndex:
    """Array.oindex (indexing.py:999-1024)."""

    def __init__(self, array: Array):
        self.array = array

    def __getitem__(self, selection):
        return self.array.get_orthogonal_selection(selection)

    def __setitem__(self, selection, value) -> None:
        self.array.set_orthogonal_selection(selection, value)


class _VIndex:
    """Array.vindex (indexing.py:1376-1420): a Boolean mask of the array's
    shape is a mask selection, anything else a coordinate selection."""

    def __init__(self, array: Array):
        self.array = array

    def _indexer(self, selection):
        return self.array._indexer("device" if points.has_device_index(selection) else "vindex", selection)

    def __getitem__(self, selection):
        if points.has_device_index(selection):  # device indices give a device tensor
            return self.array._get_fancy(self._indexer(selection))
        return self.array._get_fancy_host(self._indexer(selection))

    def __setitem__(self, selection, value) -> None:
        self.array._set_fancy(self._indexer(selection), value)


class ChunkNotFoundError(KeyError):
    """array.py:5496-5511 (read_missing_chunks=False)."""
