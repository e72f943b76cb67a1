"""Named cases and an independent reference for the value map (scale_offset /
cast_value: zhip_value_map and its CPU hook).

The reference is written per element with Python ``int``, ``fractions.Fraction``
and ``math``; the float scale_offset path uses numpy float scalars of the
array's own type (one IEEE operation at a time, which is the specification).
It imports nothing from the package under test.

A *description* is a dict: encode (bool), array_dt / stored_dt (numpy dtype
names), so = (offset, scale) numpy scalars of the array dtype or None, cast =
dict(rounding, out_of_range, map=[(key, value), ...] for this direction) or
None, fill (numpy scalar of the array dtype).

An *item* is (a_base, b_base, [(count, sa, sb), ...], flags, status) in bytes,
last dimension fastest.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

E_INEXACT, E_SO_RANGE, E_CAST_RANGE, E_NAN = 1, 2, 4, 8
F_MISSING, F_STATUS = 1, 2
ST_OK, ST_MISSING = 0, 1
TILE = 2048
ROUNDINGS = ("nearest-even", "towards-zero", "towards-positive", "towards-negative", "nearest-away")


def _is_float(dt) -> bool:
    return np.dtype(dt).kind == "f"


def _range(dt) -> tuple[int, int]:
    info = np.iinfo(np.dtype(dt))
    return int(info.min), int(info.max)


def ref_scale_offset(dt, x, offset, scale, encode: bool):
    """(numpy scalar | None, error bits)."""
    dt = np.dtype(dt)
    if _is_float(dt):
        T = dt.type
        with np.errstate(all="ignore"):
            if encode:
                r = T(T(x) - T(offset))
                r = T(r * T(scale))
            else:
                r = T(T(x) / T(scale))
                r = T(r + T(offset))
        return r, 0
    x, o, s = int(x), int(offset), int(scale)
    if encode:
        r = (x - o) * s
    else:
        if x % s != 0:
            return None, E_INEXACT
        r = x // s + o
    lo, hi = _range(dt)
    if r < lo or r > hi:
        return None, E_SO_RANGE
    return dt.type(r), 0


def _round(fr: Fraction, mode: str) -> int:
    if mode == "nearest-even":
        return round(fr)  # Fraction.__round__ rounds half to even
    if mode == "towards-zero":
        return math.trunc(fr)
    if mode == "towards-positive":
        return math.ceil(fr)
    if mode == "towards-negative":
        return math.floor(fr)
    if mode == "nearest-away":
        n = math.floor(abs(fr) + Fraction(1, 2))
        return n if fr >= 0 else -n
    raise ValueError(mode)


def _key_hits(src, x, key) -> bool:
    if _is_float(src):
        xf, kf = float(x), float(key)
        if math.isnan(xf) or math.isnan(kf):
            return math.isnan(xf) and math.isnan(kf)
        return xf == kf  # +0 == -0
    return int(x) == int(key)


def _int_to(dst, v: int, oor):
    dst = np.dtype(dst)
    lo, hi = _range(dst)
    if v < lo or v > hi:
        if oor == "clamp":
            v = lo if v < lo else hi
        elif oor == "wrap":
            bits = 8 * dst.itemsize
            v %= 1 << bits
            if lo < 0 and v >= 1 << (bits - 1):
                v -= 1 << bits
        else:
            return None, E_CAST_RANGE
    return dst.type(v), 0


def ref_cast(src, dst, x, rounding="nearest-even", oor=None, smap=()):
    src, dst = np.dtype(src), np.dtype(dst)
    for k, v in smap:
        if _key_hits(src, x, k):
            return dst.type(v), 0
    if _is_float(src):
        xf = float(x)
        if math.isnan(xf):
            return None, E_NAN
        if math.isinf(xf):
            if oor == "clamp":
                lo, hi = _range(dst)
                return dst.type(hi if xf > 0 else lo), 0
            return None, E_CAST_RANGE
        return _int_to(dst, _round(Fraction(xf), rounding), oor)
    if _is_float(dst):
        return dst.type(int(x)), 0  # exact in every accepted pair
    return _int_to(dst, int(x), oor)


def ref_one(desc, x):
    """One element through the description: (numpy scalar of the b side's
    dtype, error bits); an element with an error is zero."""
    adt, sdt = np.dtype(desc["array_dt"]), np.dtype(desc["stored_dt"])
    so, cast = desc.get("so"), desc.get("cast")
    err = 0
    if desc["encode"]:
        out_dt = sdt
        if so is not None:
            x, err = ref_scale_offset(adt, x, so[0], so[1], True)
        if not err and cast is not None:
            x, err = ref_cast(adt, sdt, x, cast.get("rounding", "nearest-even"), cast.get("out_of_range"),
                              cast.get("map", ()))
    else:
        out_dt = adt
        if cast is not None:
            x, err = ref_cast(sdt, adt, x, cast.get("rounding", "nearest-even"), cast.get("out_of_range"),
                              cast.get("map", ()))
        if not err and so is not None:
            x, err = ref_scale_offset(adt, x, so[0], so[1], False)
    if err:
        return out_dt.type(0), err
    return out_dt.type(x), 0


def ref_is_fill(desc, x) -> bool:
    """NDBuffer.all_equal's element rule: bitwise, any NaN equals a NaN fill."""
    adt = np.dtype(desc["array_dt"])
    fill = adt.type(desc["fill"])
    if adt.type(x).tobytes() == fill.tobytes():
        return True
    return _is_float(adt) and math.isnan(float(fill)) and math.isnan(float(x))


def ref_run(desc, items, a: bytes, b: bytearray, status=None):
    """The whole map over byte buffers: (error bits, non-empty words)."""
    adt, sdt = np.dtype(desc["array_dt"]), np.dtype(desc["stored_dt"])
    a_dt, b_dt = (adt, sdt) if desc["encode"] else (sdt, adt)
    err = 0
    ne = [0] * len(items)
    a = bytes(a)
    for i, (a_base, b_base, dims, flags, st) in enumerate(items):
        missing = False
        if not desc["encode"]:
            missing = bool(flags & F_MISSING) or bool(flags & F_STATUS and status[st] == ST_MISSING)
        for idx in np.ndindex(*[d[0] for d in dims]):
            ao = a_base + sum(k * d[1] for k, d in zip(idx, dims))
            bo = b_base + sum(k * d[2] for k, d in zip(idx, dims))
            assert 0 <= ao and ao + a_dt.itemsize <= len(a) and 0 <= bo and bo + b_dt.itemsize <= len(b)
            if missing:
                y = adt.type(desc["fill"])
            else:
                x = np.frombuffer(a, a_dt, 1, ao)[0]
                if desc["encode"] and not ref_is_fill(desc, x):
                    ne[i] = 1
                y, e = ref_one(desc, x)
                err |= e
            b[bo: bo + b_dt.itemsize] = y.tobytes()
    return err, ne


# ------------------------------------------------------------------ values
def float_values(dt) -> np.ndarray:
    T = np.dtype(dt).type
    fi = np.finfo(dt)
    vals = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, fi.max, -fi.max, np.inf, -np.inf,
            np.nan, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 0.49999997, 1.7, -1.7, 1e-3, 12345.678, -999.0, 999.0]
    for bits in (8, 16, 32):  # one below, at and one above each end of the integer ranges (and the .5 ties there)
        if bits == 32 and np.dtype(dt) == np.float32:
            continue  # not a served target; the ends are not exact in float32 either
        for end in (-(1 << (bits - 1)), (1 << (bits - 1)) - 1, (1 << bits) - 1, 0):
            vals += [end - 1, end - 0.5, end, end + 0.5, end + 1, end + 0.25, end - 0.25]
    vals += [2.0 ** 40, -(2.0 ** 40) - 4096.0, 2.0 ** 63, -(2.0 ** 64), 70000.0, -70000.0, 65536.0 * 3 + 7]
    with np.errstate(over="ignore"):
        return np.array(vals, dtype=dt)


def int_values(dt) -> np.ndarray:
    lo, hi = _range(dt)
    vals = {lo, lo + 1, hi - 1, hi, 0, 1, 3, 6, 7, 9, 10, 100, 126, 127}
    for v in (-1, -3, -6, -7, -10, -128, -129, -999, 128, 255, 256, 32767, 32768, 65535, 65536, -32768, -32769,
              2 ** 31 - 1, 2 ** 31, -2 ** 31, 2 ** 32 - 1, 2 ** 32, -2 ** 31 - 1, -999, 999, 30, -30, 300, -300):
        if lo <= v <= hi:
            vals.add(v)
    return np.array(sorted(vals), dtype=dt)


def values_of(dt) -> np.ndarray:
    return float_values(dt) if _is_float(dt) else int_values(dt)


CAST_PAIRS = (
    [("float32", s) for s in ("int8", "uint8", "int16", "uint16")]
    + [("float64", s) for s in ("int8", "uint8", "int16", "uint16", "int32", "uint32")]
    + [(a, s) for a in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32")
       for s in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32") if a != s])


def _scalar(dt, v):
    return np.dtype(dt).type(v)


def value_cases() -> list:
    """[(name, description, 1-D input array of the a side's dtype)]."""
    out = []
    # scale_offset alone: scales 3, -3, 0.1, 10, offsets that overflow
    for dt in ("float32", "float64"):
        for off, sc in ((0, 3), (1.5, -3), (0, 0.1), (-2.25, 10), (np.inf, 1), (0, np.nan), (1e30, 1e30)):
            for enc in (True, False):
                with np.errstate(over="ignore"):
                    desc = dict(encode=enc, array_dt=dt, stored_dt=dt, so=(_scalar(dt, off), _scalar(dt, sc)),
                                cast=None, fill=_scalar(dt, np.nan if off == 1.5 else 0.25))
                out.append((f"so-{dt}-{off}-{sc}-{'enc' if enc else 'dec'}", desc, float_values(dt)))
    for dt in ("int8", "int16", "int32", "uint8", "uint16", "uint32"):
        lo, hi = _range(dt)
        pairs = [(0, 3), (5, 10), (hi, 1), (lo if lo else 7, hi), (hi, hi), (1, 2)]
        if lo < 0:
            pairs += [(0, -3), (-5, -1), (lo, lo), (hi, lo), (lo, -1)]
        for off, sc in pairs:
            for enc in (True, False):
                desc = dict(encode=enc, array_dt=dt, stored_dt=dt, so=(_scalar(dt, off), _scalar(dt, sc)), cast=None,
                            fill=_scalar(dt, 7))
                out.append((f"so-{dt}-{off}-{sc}-{'enc' if enc else 'dec'}", desc, int_values(dt)))
    # cast_value alone: every pair, both directions, every mode
    k = 0
    for adt, sdt in CAST_PAIRS:
        for oor in (None, "clamp", "wrap"):
            rounding = ROUNDINGS[k % 5]
            k += 1
            for enc in (True, False):
                src, dst = (adt, sdt) if enc else (sdt, adt)
                smap = []
                if _is_float(src):
                    smap = [(_scalar(src, np.nan), _scalar(dst, -999 if _range(dst)[0] <= -999 else 9)),
                            (_scalar(src, 0.0), _scalar(dst, 1))]
                elif _range(src)[0] <= -999:
                    smap = [(_scalar(src, -999), _scalar(dst, np.nan if _is_float(dst) else 5)),
                            (_scalar(src, 0), _scalar(dst, 2))]
                if k % 3 == 0:
                    smap = []
                desc = dict(encode=enc, array_dt=adt, stored_dt=sdt, so=None,
                            cast=dict(rounding=rounding, out_of_range=oor, map=smap), fill=_scalar(adt, 3))
                out.append((f"cast-{adt}-{sdt}-{oor}-{rounding}-{'enc' if enc else 'dec'}-m{len(smap)}", desc,
                            values_of(src)))
    # every rounding mode on float32 -> int16 and float64 -> int32
    for adt, sdt in (("float32", "int16"), ("float64", "int32")):
        for rounding in ROUNDINGS:
            desc = dict(encode=True, array_dt=adt, stored_dt=sdt, so=None,
                        cast=dict(rounding=rounding, out_of_range="clamp", map=[]), fill=_scalar(adt, 0))
            out.append((f"round-{adt}-{sdt}-{rounding}", desc, float_values(adt)))
    # both stages
    for adt, sdt, off, sc in (("float32", "int16", 0, 10), ("float32", "uint8", -2.5, 0.1), ("float64", "int32", 1e3, -3),
                              ("int32", "int8", 100, 3), ("uint16", "int64", 9, 10), ("int16", "uint8", -30, -3)):
        for enc in (True, False):
            desc = dict(encode=enc, array_dt=adt, stored_dt=sdt, so=(_scalar(adt, off), _scalar(adt, sc)),
                        cast=dict(rounding="nearest-even", out_of_range=None, map=[]), fill=_scalar(adt, 0))
            out.append((f"both-{adt}-{sdt}-{off}-{sc}-{'enc' if enc else 'dec'}", desc,
                        values_of(adt if enc else sdt)))
    return out


# ------------------------------------------------------------------- items
def contiguous_items(n: int, asz: int, bsz: int, a_off: int = 0, b_off: int = 0) -> list:
    return [(a_off, b_off, [(n, asz, bsz)], 0, 0)]


def vec_width(asz: int, bsz: int) -> int:
    n = min(asz, bsz)
    return 8 if n == 1 else min(8, 16 // n)


def shape_cases(asz: int, bsz: int) -> list:
    """[(name, items, a bytes needed, b bytes needed, status | None)] for a map
    whose a side has asz-byte and whose b side has bsz-byte items."""
    V = vec_width(asz, bsz)
    out = []

    def add(name, items, status=None):
        na = max(max(_hi(it, 1, asz) for it in items), 1)
        nb = max(max(_hi(it, 2, bsz) for it in items), 1)
        out.append((name, items, na, nb, status))

    for n in (1, 1023, 1024, 1025):
        add(f"ones-{n}", [(i * asz, i * bsz, [(1, 0, 0)], 0, 0) for i in range(n)])
    add("ones-4097", [(i * asz, i * bsz, [(1, 0, 0)], 0, 0) for i in range(4097)])
    for c in (V - 1, V, V + 1, 3 * V, TILE + V, 2 * TILE + 1):
        if c >= 1:
            add(f"row-{c}", [(0, 0, [(5, c * asz, c * bsz), (c, asz, bsz)], 0, 0)])
    # bases that break the 16-byte alignment on either side
    add("misaligned-a", [(asz, 0, [(4, 8 * V * asz, 8 * V * bsz), (4 * V, asz, bsz)], 0, 0)])
    add("misaligned-b", [(0, bsz, [(4, 8 * V * asz, 8 * V * bsz), (4 * V, asz, bsz)], 0, 0)])
    add("misaligned-row", [(0, 0, [(4, (4 * V + 1) * asz, (4 * V + 1) * bsz), (4 * V, asz, bsz)], 0, 0)])
    # negative strides, a scalar on the a side, a strided innermost dimension
    n = 3 * V + 2
    add("negative", [((n - 1) * asz, 0, [(n, -asz, bsz)], 0, 0), (n * asz, (2 * n - 1) * bsz, [(n, asz, -bsz)], 0, 0)])
    add("scalar-a", [(0, 0, [(6, 0, 40 * bsz), (37, 0, bsz)], 0, 0)])
    add("strided", [(0, 0, [(7, 64 * asz, 48 * bsz), (16, 2 * asz, 3 * bsz)], 0, 0)])
    for nd in range(1, 9):
        counts = [2, 3, 2, 1, 3, 2, 2, 4][8 - nd:]
        counts[-1] = 2 * V
        sa, sb, dims = asz, bsz, []
        for c in reversed(counts):
            dims.append((c, sa, sb))
            sa, sb = sa * c, sb * (c + (1 if len(dims) == 2 else 0))
        add(f"ndim-{nd}", [(0, 0, list(reversed(dims)), 0, 0)])
    # OK and MISSING items alternating, by flag and by status index
    m = 2 * V + 3
    add("missing-flag", [(i * m * asz, i * m * bsz, [(m, asz, bsz)], F_MISSING if i % 2 else 0, 0) for i in range(6)])
    add("missing-status", [(i * 4 * V * asz, i * 4 * V * bsz, [(4 * V, asz, bsz)], F_STATUS, 5 - i) for i in range(6)],
        status=[ST_OK, ST_MISSING, ST_OK, ST_MISSING, ST_MISSING, ST_OK])
    return out


def _hi(item, side: int, itemsize: int) -> int:
    base = item[side - 1]
    hi = base
    for d in item[2]:
        s = d[side] * (d[0] - 1)
        if s > 0:
            hi += s
    return hi + itemsize
