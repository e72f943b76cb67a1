"""What the value-map tests share: a description of value_cases.py as the
product's op record, the buffers of a case with sentinel words around b, and
the reference's verdict, computed once per case."""

from __future__ import annotations

import functools
import zlib

import numpy as np

import value_cases as VC
from zarr_hip import _native as N
from zarr_hip import values as V

SENTINEL = 0xA5
PAD = 64  # sentinel bytes before and after b


def op_of(desc) -> np.ndarray:
    return V.make_op(desc["encode"], desc["array_dt"], desc["stored_dt"], desc.get("so"), desc.get("cast"),
                     desc["fill"])


def sides(desc) -> tuple:
    adt, sdt = np.dtype(desc["array_dt"]), np.dtype(desc["stored_dt"])
    return (adt, sdt) if desc["encode"] else (sdt, adt)


@functools.lru_cache(maxsize=None)
def _value_cases():
    return {name: (desc, vals) for name, desc, vals in VC.value_cases()}


def value_case_names() -> list:
    return list(_value_cases())


@functools.lru_cache(maxsize=None)
def value_case(name: str):
    """(desc, items, prefix-ready item specs, a bytes, expected b bytes with
    sentinels, expected error bits, expected non-empty words)."""
    desc, vals = _value_cases()[name]
    a_dt, b_dt = sides(desc)
    # the values twice: once as one long contiguous item (vector path), once
    # behind a one-element shift (element path)
    n = len(vals)
    reps = -(-64 // n) if n < 64 else 1
    vals = np.tile(vals, reps)
    n = len(vals)
    n8 = n - n % 8
    a = np.concatenate([vals[:n8], vals]).astype(a_dt)
    items = [(0, PAD, [(n8, a_dt.itemsize, b_dt.itemsize)], 0, 0),
             (n8 * a_dt.itemsize, PAD + (n8 + 1) * b_dt.itemsize, [(n, a_dt.itemsize, b_dt.itemsize)], 0, 0)]
    nb = PAD + (n8 + 1 + n) * b_dt.itemsize + PAD
    return (desc, items) + _expect(desc, items, a.tobytes(), nb, None)


def _expect(desc, items, a: bytes, nb: int, status):
    b = bytearray([SENTINEL]) * nb
    err, ne = VC.ref_run(desc, items, a, b, status)
    return a, bytes(b), err, ne


SHAPE_DESCS = {
    # (a itemsize, b itemsize) pairs through real maps, both directions
    "f32-i16-dec": dict(encode=False, array_dt="float32", stored_dt="int16", so=(np.float32(-2.5), np.float32(10)),
                        cast=dict(rounding="nearest-even", out_of_range=None, map=[]), fill=np.float32(0.25)),
    "f32-i16-enc": dict(encode=True, array_dt="float32", stored_dt="int16", so=(np.float32(-2.5), np.float32(10)),
                        cast=dict(rounding="nearest-even", out_of_range="clamp", map=[]), fill=np.float32(0.25)),
    "f64-u8-dec": dict(encode=False, array_dt="float64", stored_dt="uint8", so=None,
                       cast=dict(rounding="nearest-even", out_of_range=None, map=[]), fill=np.float64(np.nan)),
    "i8-i64-enc": dict(encode=True, array_dt="int8", stored_dt="int64", so=None,
                       cast=dict(rounding="nearest-even", out_of_range=None, map=[]), fill=np.int8(-1)),
    "f64-so-enc": dict(encode=True, array_dt="float64", stored_dt="float64", so=(np.float64(1), np.float64(3)),
                       cast=None, fill=np.float64(np.nan)),
    "u16-so-dec": dict(encode=False, array_dt="uint16", stored_dt="uint16", so=(np.uint16(0), np.uint16(1)),
                       cast=None, fill=np.uint16(9)),
    "i32-u8-enc": dict(encode=True, array_dt="int32", stored_dt="uint8", so=None,
                       cast=dict(rounding="nearest-even", out_of_range="wrap", map=[]), fill=np.int32(0)),
}


def shape_case_ids() -> list:
    out = []
    for dn, desc in SHAPE_DESCS.items():
        a_dt, b_dt = sides(desc)
        out += [(dn, sc[0]) for sc in VC.shape_cases(a_dt.itemsize, b_dt.itemsize)]
    return out


@functools.lru_cache(maxsize=None)
def shape_case(dn: str, sn: str):
    desc = SHAPE_DESCS[dn]
    a_dt, b_dt = sides(desc)
    sc = {c[0]: c for c in VC.shape_cases(a_dt.itemsize, b_dt.itemsize)}[sn]
    _, items, na, nb, status = sc
    items = [(a0, b0 + PAD, dims, fl, st) for a0, b0, dims, fl, st in items]
    rng = np.random.default_rng(zlib.crc32(f"{dn}/{sn}".encode()))
    n = -(-na // a_dt.itemsize)
    if a_dt.kind == "f":
        a = (rng.integers(-1200, 1200, n) / 10.0).astype(a_dt)
    else:
        lo, hi = VC._range(a_dt)
        a = rng.integers(max(lo, -100), min(hi, 100) + 1, n).astype(a_dt)
    fill = np.dtype(desc["array_dt"]).type(desc["fill"])
    if desc["encode"]:
        a[::3] = fill  # some fill elements; "scalar-a" and all-fill items decide the non-empty words
    a = np.concatenate([a, np.zeros(2, a_dt)])
    return (desc, items, status) + _expect(desc, items, a.tobytes()[:max(na, 1)], nb + 2 * PAD, status)


def status_table(status) -> np.ndarray | None:
    if status is None:
        return None
    st = np.zeros(len(status), np.dtype([("code", "<u4"), ("stored", "<u4"), ("computed", "<u4"), ("aux", "<u4")]))
    st["code"] = status
    return st


def run_hook(desc, items, a: bytes, nb: int, status=None):
    """zhip_emulate_value_map: (b bytes, error bits, non-empty words)."""
    a_arr = np.frombuffer(bytearray(a) + bytearray(16), np.uint8)[:len(a)]
    b = np.full(nb, SENTINEL, np.uint8)
    its, prefix = V.make_items(items)
    err, ne = V.emulate(op_of(desc), its, prefix, a_arr, b, status_table(status))
    return b.tobytes(), err, [int(x) for x in ne]


def run_device(desc, items, a: bytes, nb: int, device, status=None):
    """zhip_value_map on torch's current stream: the same triple."""
    import torch

    da = torch.from_numpy(np.frombuffer(bytearray(a) + bytearray(16), np.uint8).copy()).to(device)
    db = torch.full((nb,), SENTINEL, dtype=torch.uint8, device=device)
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    its, prefix = V.make_items(items)
    a_dt, b_dt = sides(desc)
    V._check_items(items, len(a), nb, a_dt.itemsize, b_dt.itemsize)  # nothing unchecked reaches the device
    d_items = torch.from_numpy(its.view(np.uint8).reshape(-1)).to(device)
    d_prefix = torch.from_numpy(prefix.view(np.int32)).to(device)
    st = status_table(status)
    d_status = None if st is None else torch.from_numpy(st.view(np.uint8).reshape(-1)).to(device)
    words = torch.zeros(1 + len(items), dtype=torch.int32, device=device)
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    V.launch(op_of(desc), d_items, len(items), d_prefix, int(prefix[-1]), d_status, da.data_ptr(), len(a),
             db.data_ptr(), nb, words, words[1:] if desc["encode"] else None, stream)
    assert N.lib().zhip_last_kernel() == b"k_value_map"
    torch.cuda.synchronize(device)
    host = words.cpu().numpy()
    return db.cpu().numpy().tobytes(), int(host[0]), [int(x) for x in host[1:]]
