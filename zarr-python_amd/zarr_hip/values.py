"""The value route: ``scale_offset`` and ``cast_value`` on the GPU.

The value codecs of a chain are element-wise maps, so they commute with
``transpose``: ``split`` takes them out of the chain (keeping their order) and
leaves a *stored pipeline*, the same chain over the stored dtype and the
stored fill value, which planner.analyze_chain accepts.  A read decodes the
batch with the stored pipeline into a stored-dtype twin of ``out`` and one
``k_value_map`` launch (zhip_value_map, include/zarrhip.h) writes ``out``; a
write merges in the array domain, maps array -> stored with the per-chunk
non-empty words, and hands whole stored chunks to the stored pipeline.

Missing chunks read as the array's fill value exactly (not decode(encode(fill)))
and emptiness is decided on array-domain chunks, as the reference decides
both (codec_pipeline.py:1095-1253: the fill and ``all_equal`` are applied
outside the codec chain).

The op record, the item tables and the CPU hook ``emulate`` live here too; the
codec classes cast and encode their fill values through ``map_scalar`` so the
arithmetic is stated once, in csrc/zhip_values.h.
"""

from __future__ import annotations

import ctypes
import threading
from dataclasses import replace

import numpy as np

from . import _native as N

DT_CODES = {"int8": N.VT_I8, "uint8": N.VT_U8, "int16": N.VT_I16, "uint16": N.VT_U16, "int32": N.VT_I32,
            "uint32": N.VT_U32, "int64": N.VT_I64, "float32": N.VT_F32, "float64": N.VT_F64}
SCALE_OFFSET_DTYPES = ("float32", "float64", "int8", "int16", "int32", "uint8", "uint16", "uint32")
_CAST_INTS = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32")
ROUNDING = ("nearest-even", "towards-zero", "towards-positive", "towards-negative", "nearest-away")
OUT_OF_RANGE = (None, "clamp", "wrap")


def cast_pair_ok(array_dt: np.dtype, stored_dt: np.dtype) -> bool:
    """The (array dtype, stored dtype) pairs cast_value is served for: the
    decode direction is exact in every one of them."""
    a, s = np.dtype(array_dt).name, np.dtype(stored_dt).name
    if a == s:
        return False
    if a == "float32":
        return s in ("int8", "uint8", "int16", "uint16")
    if a == "float64":
        return s in ("int8", "uint8", "int16", "uint16", "int32", "uint32")
    return a in _CAST_INTS and s in _CAST_INTS


def parse_scalar(value, dtype: np.dtype):
    """A JSON scalar as a numpy scalar of ``dtype``, as the data types'
    from_json_scalar reads it (core/dtype/npy/int.py:189-218, float.py):
    integers, integral floats and integer strings for integer types; numbers,
    "NaN" / "Infinity" / "-Infinity", hex strings of the raw bits and decimal
    strings for floats.  TypeError / ValueError / OverflowError otherwise."""
    dtype = np.dtype(dtype)
    if isinstance(value, (bool, np.bool_)):
        raise TypeError(f"Invalid type: {value!r}.")
    if isinstance(value, np.generic):
        value = value.item()
    if dtype.kind in "iu":
        if isinstance(value, float):
            if not value.is_integer():
                raise TypeError(f"Invalid type: {value}. Expected an integer.")
            value = int(value)
        elif isinstance(value, str):
            value = int(value)
        elif not isinstance(value, int):
            raise TypeError(f"Invalid type: {value!r}. Expected an integer.")
        info = np.iinfo(dtype)
        if value < info.min or value > info.max:
            raise OverflowError(f"{value} is outside the range of {dtype}")
        return dtype.type(value)
    if dtype.kind != "f":
        raise TypeError(f"dtype {dtype} has no numeric scalars")
    if isinstance(value, str):
        if value == "NaN":
            return dtype.type(np.nan)
        if value in ("Infinity", "-Infinity"):
            return dtype.type(np.inf if value[0] != "-" else -np.inf)
        if value.startswith("0x"):
            raw = int(value, 16).to_bytes(dtype.itemsize, "little")
            return np.frombuffer(raw, dtype.newbyteorder("<"))[0].astype(dtype)
        return dtype.type(float(value))
    if not isinstance(value, (int, float)):
        raise TypeError(f"Invalid type: {value!r}. Expected a float.")
    with np.errstate(over="ignore"):
        return dtype.type(value)


def raw_bits(x, dtype: np.dtype) -> int:
    """The item's bytes as an unsigned integer (the op record's scalar form)."""
    dtype = np.dtype(dtype)
    return int.from_bytes(np.asarray(x, dtype=dtype).astype(dtype.newbyteorder("<")).tobytes(), "little")


def make_op(encode: bool, array_dt, stored_dt, scale_offset=None, cast=None, fill=None) -> np.ndarray:
    """One zhip_value_op.  scale_offset: (offset, scale) numpy scalars of the
    array dtype or None; cast: a dict(rounding=, out_of_range=, map=[(key,
    value) numpy scalars of the cast's input / output dtype for THIS
    direction]) or None; fill: the array fill (numpy scalar / number / None)."""
    array_dt, stored_dt = np.dtype(array_dt), np.dtype(stored_dt)
    op = np.zeros(1, N.VALUE_OP_DT)
    o = op[0]
    o["encode"] = 1 if encode else 0
    o["array_dt"] = DT_CODES[array_dt.name]
    o["stored_dt"] = DT_CODES[stored_dt.name]
    stages = 0
    if scale_offset is not None:
        stages |= N.VS_SCALE_OFFSET
        o["offset"] = raw_bits(scale_offset[0], array_dt)
        o["scale"] = raw_bits(scale_offset[1], array_dt)
    if cast is not None:
        stages |= N.VS_CAST
        o["rounding"] = ROUNDING.index(cast.get("rounding") or "nearest-even")
        o["out_of_range"] = OUT_OF_RANGE.index(cast.get("out_of_range"))
        pairs = list(cast.get("map") or ())
        if len(pairs) > N.VALUE_MAX_MAP:
            raise NotImplementedError(
                f"cast_value: more than {N.VALUE_MAX_MAP} scalar_map entries per direction ({len(pairs)})")
        kd, vd = (array_dt, stored_dt) if encode else (stored_dt, array_dt)
        o["n_map"] = len(pairs)
        for i, (k, v) in enumerate(pairs):
            o["map_key"][i] = raw_bits(k, kd)
            o["map_val"][i] = raw_bits(v, vd)
    o["stages"] = stages
    fv = 0 if fill is None else fill
    o["fill"] = raw_bits(fv, array_dt)
    o["fill_nan"] = 1 if array_dt.kind == "f" and np.isnan(np.asarray(fv, dtype=array_dt)) else 0
    return op


def make_items(specs) -> tuple[np.ndarray, np.ndarray]:
    """(items, tile prefix) from [(a_base, b_base, [(count, sa, sb), ...],
    flags, status), ...] (byte strides, last dimension fastest)."""
    items = np.zeros(len(specs), N.VALUE_ITEM_DT)
    prefix = np.zeros(len(specs) + 1, np.uint32)
    for i, (a_base, b_base, dims, flags, status) in enumerate(specs):
        dims = list(dims) or [(1, 0, 0)]
        if len(dims) > N.MAX_DIMS:
            raise NotImplementedError(f"value map: {len(dims)} dimensions (at most {N.MAX_DIMS})")
        it = items[i]
        it["a_base"], it["b_base"] = a_base, b_base
        it["ndim"] = len(dims)
        total = 1
        for d, (count, sa, sb) in enumerate(dims):
            D = it["dims"][d]
            D["sa"], D["sb"], D["count"] = sa, sb, count
            D["div"] = N.fdiv(count)
            total *= int(count)
        if total >= 1 << 31:
            raise NotImplementedError("value map: an item of 2^31 or more elements")
        it["total"] = total
        it["flags"], it["status"] = flags, status
        prefix[i + 1] = prefix[i] + (total + N.VALUE_TILE - 1) // N.VALUE_TILE
    return items, prefix


def item_extent(dims, base: int, side: int, itemsize: int) -> tuple[int, int]:
    """[lowest byte, one past the highest byte) an item touches on one side."""
    lo = hi = base
    for d in dims:
        s = d[1 + side] * (d[0] - 1)
        if s < 0:
            lo += s
        else:
            hi += s
    return lo, hi + itemsize


def emulate(op: np.ndarray, items: np.ndarray, prefix: np.ndarray, a: np.ndarray, b: np.ndarray,
            status: np.ndarray | None = None) -> tuple[int, np.ndarray]:
    """zhip_emulate_value_map over host byte buffers a (read) and b (written):
    (error bits, per-item non-empty words)."""
    err = np.zeros(1, np.uint32)
    ne = np.zeros(max(len(items), 1), np.uint32)
    st = None if status is None else np.ascontiguousarray(status)
    N.check(N.lib().zhip_emulate_value_map(
        op.ctypes.data, items.ctypes.data, len(items), prefix.ctypes.data, int(prefix[-1]),
        None if st is None else st.ctypes.data, 0 if st is None else len(st),
        a.ctypes.data, a.nbytes, b.ctypes.data, b.nbytes, err.ctypes.data, ne.ctypes.data), "zhip_emulate_value_map")
    return int(err[0]), ne[:len(items)]


def launch(op: np.ndarray, d_items, n_items: int, d_prefix, n_tiles: int, d_status, a_ptr: int, a_size: int,
           b_ptr: int, b_size: int, d_err, d_nonempty, stream: int) -> None:
    """zhip_value_map on device tables (torch uint8 / int32 tensors or None)."""
    N.check(N.lib().zhip_value_map(
        op.ctypes.data, d_items.data_ptr(), n_items, d_prefix.data_ptr(), n_tiles,
        None if d_status is None else (d_status if isinstance(d_status, int) else d_status.data_ptr()),
        a_ptr, a_size, b_ptr, b_size, d_err.data_ptr(),
        None if d_nonempty is None else d_nonempty.data_ptr(), ctypes.c_void_p(stream)), "zhip_value_map")


def error_message(err: int, ops: "ValueOps", encode: bool) -> str:
    """The ValueError of the first stage that failed, in the order the
    reference's codecs run (each raises for the whole chunk before the next
    starts).  scale_offset's texts are the reference's (scale_offset.py:59-74);
    cast_value's are this package's (its backend's are not specified)."""
    adt = ops.array_dt
    so = []
    if err & N.VE_INEXACT:
        so.append(f"scale_offset decode produced a non-zero remainder when dividing by scale={ops.so.scale!r}; "
                  f"result is not exactly representable in dtype {adt}.")
    if err & N.VE_SO_RANGE:
        info = np.iinfo(adt)
        so.append(f"scale_offset produced a value outside the range of dtype {adt} [{info.min}, {info.max}].")
    cv = []
    if err & (N.VE_CAST_RANGE | N.VE_NAN):
        src, dst = (adt, ops.stored_dt) if encode else (ops.stored_dt, adt)
        if err & N.VE_NAN:
            cv.append(f"cast_value: not a number: a NaN of dtype {src} has no value in dtype {dst} "
                      "(and no scalar_map entry)")
        if err & N.VE_CAST_RANGE:
            cv.append(f"cast_value: out of range: a value of dtype {src} is outside the range of dtype {dst} "
                      "(out_of_range is not set)")
    order = so + cv if encode else cv + so
    return order[0]


class ValueOps:
    """The value part of a chain: the codecs in encode order (scale_offset,
    cast_value, or both), the array dtype / fill and the stored dtype / fill."""

    def __init__(self, so, cast, spec):
        self.so, self.cast = so, cast
        self._op_records: dict = {}
        self.array_dt = np.dtype(spec.dtype)
        self.array_fill = spec.fill_value
        s = spec
        if so is not None:
            s = so.resolve_metadata(s)
        if cast is not None:
            s = cast.resolve_metadata(s)
        self.stored_dt = np.dtype(s.dtype)
        self.stored_fill = s.fill_value

    def op(self, encode: bool) -> np.ndarray:
        """The op record of one direction (built once: read-only afterwards)."""
        rec = self._op_records.get(encode)
        if rec is None:
            rec = self._op_records[encode] = self._make_op(encode)
        return rec

    def _make_op(self, encode: bool) -> np.ndarray:
        so = None if self.so is None else self.so.parsed(self.array_dt)
        cast = None if self.cast is None else self.cast.op_fields(self.array_dt, encode)
        return make_op(encode, self.array_dt, self.stored_dt, so, cast, self.array_fill)


def map_scalar(op: np.ndarray, x, what: str):
    """One element through the CPU hook (fill values): numpy scalar of the b
    side's dtype; the hook's error bits raise ValueError(what ...)."""
    o = op[0]
    names = {v: k for k, v in DT_CODES.items()}
    adt = np.dtype(names[int(o["array_dt"] if o["encode"] else o["stored_dt"])])
    bdt = np.dtype(names[int(o["stored_dt"] if o["encode"] else o["array_dt"])])
    a = np.zeros(8, np.uint8)
    a[:adt.itemsize] = np.frombuffer(np.asarray(x, dtype=adt).tobytes(), np.uint8)
    b = np.zeros(8, np.uint8)
    items, prefix = make_items([(0, 0, [(1, 0, 0)], 0, 0)])
    err, _ = emulate(op, items, prefix, a, b)
    if err:
        raise ValueError(f"{what}: error bits {err}")
    return np.frombuffer(b.tobytes()[:bdt.itemsize], bdt)[0]


# ---------------------------------------------------------------- the split
def _check_sequence(vals: list) -> tuple:
    from .codecs import CastValueCodec, ScaleOffsetCodec

    kinds = [type(c) for c in vals]
    if kinds == [ScaleOffsetCodec]:
        return vals[0], None
    if kinds == [CastValueCodec]:
        return None, vals[0]
    if kinds == [ScaleOffsetCodec, CastValueCodec]:
        return vals[0], vals[1]
    names = [c.to_dict()["name"] for c in vals]
    raise NotImplementedError(
        f"value codecs {names}: only [scale_offset], [cast_value] and [scale_offset, cast_value] (in encode "
        "order) are served; any other sequence would need more than one map per element")


def split(pipe):
    """None for a chain without value codecs, else (scale_offset | None,
    cast_value | None, stored pipeline, sharded).  An element-wise map commutes
    with transpose, so the value codecs leave the chain from wherever they
    stand among the array->array codecs, in their own order."""
    from .codecs import ShardingCodec, is_value_codec

    ab = pipe.array_bytes_codec
    outer = [c for c in pipe.array_array_codecs if is_value_codec(c)]
    if isinstance(ab, ShardingCodec):
        inner = [c for c in ab.codecs if is_value_codec(c)]
        deeper = [c for c in ab.codecs if isinstance(c, ShardingCodec)]
        if outer:
            raise NotImplementedError(
                f"{outer[0].to_dict()['name']}: value codecs around a sharding codec are not served (the shard "
                "would hold the stored dtype while its inner chunks are planned in the array dtype); put them "
                "among the sharding codec's inner codecs")
        if not inner:
            if any(is_value_codec(c) for d in deeper for c in d.codecs):
                raise NotImplementedError("value codecs (scale_offset / cast_value) inside nested sharding codecs "
                                          "are not served: nesting is routed on the host")
            return None
        if deeper:
            raise NotImplementedError(f"{inner[0].to_dict()['name']}: value codecs next to a nested sharding "
                                      "codec are not served")
        so, cast = _check_sequence(inner)
        if pipe.array_array_codecs or pipe.bytes_bytes_codecs:
            raise NotImplementedError(
                f"{inner[0].to_dict()['name']}: value codecs inside a sharding codec are served for a lone "
                "sharding_indexed codec only (no codecs around it)")
        stored_ab = replace(ab, codecs=tuple(c for c in ab.codecs if not is_value_codec(c)))
        return so, cast, pipe._sub((stored_ab,)), True
    if not outer:
        return None
    so, cast = _check_sequence(outer)
    stored = pipe._sub(tuple(c for c in pipe.codecs if not is_value_codec(c)))
    return so, cast, replace(stored, devices=pipe.devices, _read_cache={}, _aux={}), False


def refuse(pipe, what: str) -> None:
    """NotImplementedError for the entry points the value route does not serve."""
    vs = pipe._value_split()
    if vs is not None:
        name = (vs[0] or vs[1]).to_dict()["name"]
        raise NotImplementedError(f"{name}: {what} is not served for chains with value codecs "
                                  "(scale_offset / cast_value): use read_sync / write_sync")


def _ops(pipe, vs, spec) -> ValueOps:
    cache = pipe._aux.setdefault("value_ops", {})
    key = (spec.dtype.str, spec.fill_bytes())
    ops = cache.get(key)
    if ops is None:
        ops = cache[key] = ValueOps(vs[0], vs[1], spec)
    return ops


def _one_spec(pipe, batch):
    from .pipeline import spec_groups

    if spec_groups(batch) is not None:
        refuse(pipe, "a batch of mixed chunk specs (rectilinear grid)")
    return batch[0][1]


def _plain(pipe, stored) -> bool:
    """One device, no host stage, no nesting: decode and map launch back to back."""
    return len(pipe.devices) <= 1 and stored._nested() is None and stored._host_split() is None


def _extent(t) -> int:
    """Bytes addressable from t.data_ptr() through t's own strides."""
    if t.numel() == 0:
        return 0
    return (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _check_items(specs, a_size: int, b_size: int, asz: int, bsz: int) -> None:
    for a_base, b_base, dims, _, _ in specs:
        lo, hi = item_extent(dims, a_base, 0, asz)
        if lo < 0 or hi > a_size:
            raise ValueError("value map: an item reaches outside its source buffer")
        lo, hi = item_extent(dims, b_base, 1, bsz)
        if lo < 0 or hi > b_size:
            raise ValueError("value map: an item reaches outside its destination buffer")


def run_map(op, specs, a, b, device, status_ptr=None, want_nonempty=False):
    """Upload the item tables and launch k_value_map over device tensors a -> b
    on the current stream: the error word followed by the non-empty words (one
    tensor; the tables it uploads are freed in stream order).
    Every item is checked against the tensors' extents first."""
    from .pipeline import _stream_handle, _torch

    torch = _torch()
    a_size, b_size = _extent(a), _extent(b)
    _check_items(specs, a_size, b_size, a.element_size(), b.element_size())
    items, prefix = make_items(specs)
    d_items = torch.from_numpy(items.view(np.uint8).reshape(-1)).to(device)
    d_prefix = torch.from_numpy(prefix.view(np.int32)).to(device)
    words = torch.zeros(1 + (len(specs) if want_nonempty else 0), dtype=torch.int32, device=device)
    launch(op, d_items, len(specs), d_prefix, int(prefix[-1]), status_ptr, a.data_ptr(), a_size,
           b.data_ptr(), b_size, words, words[1:] if want_nonempty else None, _stream_handle(device))
    return words


def _sel_dims(sel, strides_a, strides_b):
    """(base a, base b, dims) of a basic selection (slices / integers) over
    element strides given in bytes."""
    a0 = b0 = 0
    dims = []
    for s, sa, sb in zip(sel, strides_a, strides_b):
        if isinstance(s, slice):
            start, stop, step = s.start or 0, s.stop, s.step or 1
            n = max(0, -((start - stop) // step))
            a0 += start * sa
            b0 += start * sb
            dims.append((n, step * sa, step * sb))
        else:
            a0 += int(s) * sa
            b0 += int(s) * sb
    return a0, b0, dims


# -------------------------------------------------------------------- read
def read(pipe, vs, batch_info, out, drop_axes) -> tuple:
    """read_sync of a chain with value codecs (module docstring)."""
    from .buffer import copy_to_host, torch_dtype
    from .pipeline import GetResult, _resolve_out, _stream_handle, _torch, normalize_batch

    torch = _torch()
    batch = normalize_batch(batch_info)
    if not batch:
        return ()
    spec = _one_spec(pipe, batch)
    so, cast, stored, sharded = vs
    ops = _ops(pipe, vs, spec)
    if sharded and not _plain(pipe, stored):
        raise NotImplementedError(
            f"{(so or cast).to_dict()['name']}: value codecs inside a sharding codec are served on one device "
            "without a host stage or nesting (an elided inner chunk is known only on the device)")
    sspec = replace(spec, dtype=ops.stored_dt, fill_value=ops.stored_fill)
    sbatch = [(it[0], sspec) + tuple(it[2:]) for it in batch]
    dev_out, host_out = _resolve_out(out, batch, drop_axes)
    if np.dtype(spec.dtype).itemsize != dev_out.element_size():
        raise TypeError("out dtype itemsize does not match the array dtype")
    device = dev_out.device
    asz, ssz = dev_out.element_size(), ops.stored_dt.itemsize
    op = ops.op(False)
    with torch.cuda.device(device):
        twin = torch.empty_strided(tuple(dev_out.shape), tuple(dev_out.stride()), dtype=torch_dtype(ops.stored_dt),
                                   device=device)
        if _plain(pipe, stored):
            # one value item per decode unit, pointed at the unit's record in the
            # launch's d_status: a chunk (or inner chunk) the device finds absent
            # reads as the array fill.  Decode and map back to back, one wait.
            # (planned once per batch key, like the stored pipeline's own reads:
            # the program and the item tables are kept, outs are retargeted)
            from .pipeline import READ_CACHE_SIZE, _device_resident, _key_alive, _RangeSet, _read_key, _same_arenas

            key = _read_key(sbatch, twin, drop_axes) if (READ_CACHE_SIZE and host_out is None
                                                         and _device_resident(sbatch, device)) else None
            cache = pipe._aux.setdefault("value_reads", {})
            lock = pipe._aux.setdefault("value_lock", threading.Lock())
            # checked out while in use, as in _read_cached: a concurrent read of
            # the same key plans its own program
            with lock:
                ent = cache.pop(key, None) if key is not None else None
            if ent is not None and (ent[0].stale() or not _same_arenas(ent[0], sbatch)):
                ent = None  # the store changed since the plan: plan again
            if ent is None:
                prog = stored.prepare_read(sbatch, twin, drop_axes)
                t = prog.tables
                L = t.layout
                nd = int(L.ndim)
                ostr = [int(L.out_stride[i]) for i in range(nd)]
                specs = []
                for c in range(len(t.chunks)):
                    ch = t.chunks[c]
                    cnt = t.sels[int(ch["sel"])]["count"]
                    dims = [(int(cnt[i]), ostr[i], ostr[i] // ssz * asz) for i in range(nd)]
                    if any(d[0] <= 0 for d in dims):
                        continue
                    off = int(ch["out_off"])
                    specs.append((off, off // ssz * asz, dims, N.VI_STATUS, c))
                _check_items(specs, _extent(twin), _extent(dev_out), ssz, asz)
                items, prefix = make_items(specs)
                words = torch.zeros(1, dtype=torch.int32, device=device)
                # the decode's verdict words and the map's error word: ONE wait
                ent = (prog, torch.from_numpy(items.view(np.uint8).reshape(-1)).to(device) if specs else None,
                       torch.from_numpy(prefix.view(np.int32)).to(device), len(specs), int(prefix[-1]), words,
                       _RangeSet(prog.wait_ranges() + [(words.data_ptr(), 4)]))
            prog, d_items, d_prefix, n_specs, n_tiles, words, ranges = ent
            prog.retarget(twin)
            try:
                prog.launch()
                if n_specs:
                    launch(op, d_items, n_specs, d_prefix, n_tiles, prog.data.p_status, twin.data_ptr(),
                           _extent(twin), dev_out.data_ptr(), _extent(dev_out), words, None, _stream_handle(device))
                host = ranges.wait(device)
            finally:
                prog.retarget(None)
            err = int(host[-1])
            res = prog.results_from_words(host)  # (a CRC mismatch raises here, before any value error)
            if key is not None and not err:  # an entry whose error word is set is not kept
                with lock:
                    for k in [k for k in cache if not _key_alive(k)]:  # stores gone: free their programs
                        del cache[k]
                    while len(cache) >= READ_CACHE_SIZE:
                        del cache[next(iter(cache))]
                    cache[key] = ent
        else:
            res = stored.read_sync(sbatch, twin, drop_axes)
            tstr = [int(s) * ssz for s in twin.stride()]
            bstr = [int(s) * asz for s in dev_out.stride()]
            specs = []
            for it, r in zip(batch, res):
                a0, b0, dims = _sel_dims(it[3], tstr, bstr)
                if all(d[0] > 0 for d in dims):
                    specs.append((a0, b0, dims, N.VI_MISSING if r["status"] == "missing" else 0, 0))
            err = 0
            if specs:
                words = run_map(op, specs, twin, dev_out, device)
                err = int(words[0].item())
        if err:
            raise ValueError(error_message(err, ops, False))
        if host_out is not None:
            copy_to_host(dev_out, host_out)
    return tuple(GetResult(status=r["status"]) for r in res)


# ------------------------------------------------------------------- write
def _selection_count(sel) -> int:
    n = 1
    for s in sel:
        if isinstance(s, slice):
            start, stop, step = s.start or 0, s.stop, s.step or 1
            n *= max(0, -((start - stop) // step))
    return n


def write(pipe, vs, batch_info, value, drop_axes, partial_encode) -> None:
    """_write_sync of a chain with value codecs: merge in the array domain,
    decide emptiness there, store whole chunks of the stored dtype."""
    from . import fancy
    from .buffer import torch_dtype
    from .pipeline import _resolve_value, _torch, _write_device, normalize_batch
    from .writer import _value_tensor

    torch = _torch()
    batch = normalize_batch(batch_info)
    if not batch:
        return
    so, cast, stored, sharded = vs
    if sharded:
        raise NotImplementedError(
            f"{(so or cast).to_dict()['name']}: writes through value codecs inside a sharding codec are not "
            "served yet (the per-inner-chunk keep table has to be driven from the array domain)")
    if drop_axes:
        raise NotImplementedError("drop_axes writes are not on the GPU path")
    spec = _one_spec(pipe, batch)
    ops = _ops(pipe, vs, spec)
    value = _resolve_value(value)
    device = _write_device(batch, value)
    adt, sdt = ops.array_dt, ops.stored_dt
    asz, ssz = adt.itemsize, sdt.itemsize
    # emptiness is decided here, on array-domain chunks: the stored pipeline stores what it is given
    sspec = replace(spec, dtype=sdt, fill_value=ops.stored_fill,
                    config=replace(spec.config, write_empty_chunks=True))
    shape = tuple(spec.shape)
    s0 = shape[0] if shape else 1
    rest = shape[1:] if shape else ()
    full = tuple(slice(0, s, 1) for s in shape)
    chunk_elems = int(np.prod(shape)) if shape else 1
    per = max(1, min(len(batch), fancy.FANCY_SCRATCH_BYTES // max(chunk_elems * (asz + ssz), 1)))
    dec, enc = ops.op(False), ops.op(True)
    with torch.cuda.device(device):
        v = _value_tensor(value, adt, device)
        for lo in range(0, len(batch), per):
            sub = batch[lo: lo + per]
            n = len(sub)
            A = torch.empty((n * s0,) + rest, dtype=torch_dtype(adt), device=device)
            S = torch.empty((n * s0,) + rest, dtype=torch_dtype(sdt), device=device)
            slot = [(slice(j * s0, (j + 1) * s0),) + full[1:] for j in range(n)]
            cdims = [(int(s), 0, 0) for s in shape] or [(1, 0, 0)]
            astr = [int(s) * asz for s in A.stride()]
            sstr = [int(s) * ssz for s in S.stride()]

            def chunk_item(j, flags, swap=False):
                a_st, b_st = (astr, sstr) if not swap else (sstr, astr)
                dims = [(c[0], a_st[i], b_st[i]) for i, c in enumerate(cdims)] if shape else [(1, 0, 0)]
                return (j * s0 * a_st[0] if shape else j * a_st[0], j * s0 * b_st[0] if shape else j * b_st[0],
                        dims, flags, 0)

            merge = [j for j, it in enumerate(sub) if not it[4]]
            if merge:  # the stored chunk, whole, then stored -> array (missing -> the array fill)
                res = stored.read_sync([(sub[j][0], sspec, full, slot[j], True) for j in merge], S)
                specs = [chunk_item(j, N.VI_MISSING if r["status"] == "missing" else 0, swap=True)
                         for j, r in zip(merge, res)]
                words = run_map(dec, specs, S, A, device)
                err = int(words[0].item())
                if err:
                    raise ValueError(error_message(err, ops, False))
            afill = torch.from_numpy(np.array(0 if ops.array_fill is None else ops.array_fill, dtype=adt)).to(device)
            for j, it in enumerate(sub):
                dst = A[slot[j]] if shape else A[j]
                csel = tuple(it[2])
                if it[4] and _selection_count(csel) != chunk_elems:
                    dst.copy_(afill)  # a complete edge chunk: the part outside the array is the fill
                if v.dim() == 0:
                    dst[csel] = v
                else:
                    dst[csel] = v[tuple(it[3])]
            words = run_map(enc, [chunk_item(j, 0) for j in range(n)], A, S, device, want_nonempty=True)
            host = words.cpu().numpy()  # the error word and the non-empty words: one readback
            if int(host[0]):
                raise ValueError(error_message(int(host[0]), ops, True))
            nonempty = host[1:] != 0
            keep_all = spec.config.write_empty_chunks
            store_items = [(sub[j][0], sspec, full, slot[j], True) for j in range(n) if keep_all or nonempty[j]]
            if store_items:
                stored._write_sync(store_items, S, (), partial_encode=False)
            for j in range(n):
                if not (keep_all or nonempty[j]):
                    sub[j][0].delete_sync()  # the writer's call for an elided chunk
