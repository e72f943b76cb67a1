"""The element-type rules on the CPU (table: tests/dtype_cases.py): the truth
table is not vacuous (on the oracle alone), fill values survive zarr.json,
ArraySpec.fill_bytes, the planner's layout flags per dtype, the shared
fill-equality function (csrc/zhip_fill_eq.h through zhip_emulate_fill_eq)
against the oracle's all_equal item by item, and the one host-side refusal of
dtypes the device path does not serve."""

import ctypes
import json

import numpy as np
import pytest

import dtype_cases as D
from oracle import oracle as O


def _one(x, dt):
    return np.array([x], dtype=dt)


def _elided(cls, fill, dt):
    return O.all_equal(D.class_chunk(cls, (2, 3), dt), np.asarray(fill, dt))


KINDED = [(n, fid, fv) for n, fid, fv in D.EMPTINESS if np.dtype(n).kind in "fc"]


@pytest.mark.parametrize("name,fid,fill", KINDED, ids=[f"{n}-{f}" for n, f, _ in KINDED])
def test_truth_table_is_not_vacuous(name, fid, fill):
    """Every (float or complex dtype, fill) row has an elided and a kept class;
    a NaN-fill row elides a class whose bytes differ from the fill's; the
    complex zero rows elide two such classes (the +-0 forms)."""
    dt = np.dtype(name)
    classes = D.classes_of(dt, fill)
    el = [c for c in classes if _elided(c, fill, dt)]
    assert el and len(el) < len(classes)
    differing = [c for c in el if not D.same_bytes(D.class_chunk(c, (1,), dt), _one(fill, dt))]
    if np.isnan(fill):
        assert differing
    if dt.kind == "c" and fid in ("0j", "-0.0+0j"):
        assert len(differing) >= 2


def test_integer_rows_have_both_outcomes():
    for name, fid, fill in D.EMPTINESS:
        dt = np.dtype(name)
        if dt.kind in "fc":
            continue
        got = [_elided(c, fill, dt) for c in D.classes_of(dt, fill)]
        assert got == [True, False, False, False], (name, fid)


def test_table_shape():
    """13 dtypes, the multi-byte ones in both byte orders; every family's chunk
    has the same bytes for every item size, at most 256 KiB; arrays about 2 MiB."""
    assert len(D.NAMES) == 13 and len(D.DTYPES) == 3 + 2 * 10
    for fam in D.FAMILIES:
        sizes = {int(np.prod(fam.chunk(it))) * it for it in (1, 2, 4, 8)}
        # (the two tile families keep BOTH byte extents of a tile -- rows of tq and the innermost row --
        # so their item count, not their byte size, varies)
        assert len(sizes) == 1 or fam.id in ("tile", "tileg"), fam.id
        assert max(sizes) <= 256 << 10
        for it in (1, 2, 4, 8):
            assert int(np.prod(fam.shape(it))) * it <= 2 << 20
            assert all(s > 0 for s in fam.chunk(it))
    for name, _, fill in D.EMPTINESS:
        dt = np.dtype(name)
        for fam in D.FAMILIES:
            shape, data, regions = D.truth_table_array(fam, dt, fill)
            assert data.nbytes <= (5 << 20) // 2 and len(regions) == len(D.classes_of(dt, fill))


# ------------------------------------------------------------------ fill JSON
def _meta(dt, fill):
    from zarr_hip.array import ArrayMetadata
    from zarr_hip.codecs import parse_codecs

    return ArrayMetadata((4,), (2,), np.dtype(dt), fill, tuple(parse_codecs([D.LE])))


@pytest.mark.parametrize("name,fid,fill", D.EMPTINESS, ids=[f"{n}-{f}" for n, f, _ in D.EMPTINESS])
def test_fill_json_round_trip(name, fid, fill):
    """zarr.json text and back: the same value (NaN as NaN, -0.0 with its sign)."""
    from zarr_hip.array import ArrayMetadata

    dt = np.dtype(name)
    doc = json.loads(json.dumps(_meta(dt, fill).to_json()))
    back = ArrayMetadata.from_json(doc).fill_value
    a, b = _one(fill, dt), _one(back, dt)
    if np.isnan(fill):
        # zarr.json has one NaN per component ("NaN"): the class survives, not the payload
        assert (np.isnan(a.real) == np.isnan(b.real)).all() and (np.isnan(a.imag) == np.isnan(b.imag)).all()
    else:
        assert a.tobytes() == b.tobytes()


COMPLEX_JSON = [
    (D.C("1.5", "-2.5"), [1.5, -2.5]),
    (D.C("qnan", "+0"), ["NaN", 0.0]),
    (D.C("+0", "qnan"), [0.0, "NaN"]),
    (D.C("inf", "-0"), ["Infinity", -0.0]),
    (D.C("-0", "inf"), [-0.0, "Infinity"]),
    (np.complex64(complex(-np.inf, 1.0)), ["-Infinity", 1.0]),
]


@pytest.mark.parametrize("fill,want", COMPLEX_JSON, ids=[str(w) for _, w in COMPLEX_JSON])
def test_complex_fill_json_form(fill, want):
    """[re, im] with "NaN" / "Infinity" / "-Infinity" strings
    (complex_float_to_json_v3, src/zarr/core/dtype/npy/common.py:296-312), and
    that form read back gives the same bytes (-0.0 components keep their sign)."""
    from zarr_hip.array import _fill_from_json, _fill_to_json

    dt = np.dtype("complex64")
    got = _fill_to_json(fill, dt)
    assert json.dumps(got) == json.dumps(want)  # the text: -0.0 is not 0.0 there
    back = _fill_from_json(json.loads(json.dumps(got)), dt)
    if not np.isnan(fill):
        assert _one(back, dt).tobytes() == _one(fill, dt).tobytes()
    else:
        assert np.isnan(back.real) == np.isnan(fill.real) and np.isnan(back.imag) == np.isnan(fill.imag)
    with pytest.raises(ValueError):
        _fill_from_json(1.5, dt)


@pytest.mark.parametrize("name,fid,fill", D.EMPTINESS, ids=[f"{n}-{f}" for n, f, _ in D.EMPTINESS])
def test_fill_bytes(name, fid, fill):
    from zarr_hip.spec import ArraySpec

    for order in "<>":
        dt = np.dtype(name).newbyteorder(order)
        spec = ArraySpec((4,), dt, fill)
        assert spec.fill_bytes() == np.asarray(fill, np.dtype(name)).tobytes()


# ------------------------------------------------------------------ planner flags
@pytest.mark.parametrize("name,endian,id_", D.DTYPES, ids=[d[2] for d in D.DTYPES])
def test_layout_flags(name, endian, id_):
    """CRC and SWAP from the chain; ZHIP_LF_FLOAT on the encode of real floats
    only; ZHIP_LF_COMPLEX for complex64, on both directions; through
    plan_encode's layout too."""
    import sys

    from zarr_hip import _native as N
    from zarr_hip.codecs import parse_codecs
    from zarr_hip.planner import analyze_chain, layout_flags, plan_encode
    from zarr_hip.spec import ArraySpec

    dt = np.dtype(name)
    spec = ArraySpec((4, 8), dt, 0)
    for crc in (False, True):
        chain = analyze_chain(parse_codecs([endian] + ([D.CRC] if crc else [])), spec)
        swap = dt.itemsize > 1 and (endian is D.BE) == (sys.byteorder == "little")
        assert chain.swap == swap and chain.crc == crc
        base = (N.LF_CRC if crc else 0) | (N.LF_SWAP if swap else 0) | (N.LF_COMPLEX if dt.kind == "c" else 0)
        assert layout_flags(chain, dt) == base
        assert layout_flags(chain, dt, encode=True) == base | (N.LF_FLOAT if dt.kind == "f" else 0)
        t = plan_encode(chain, spec, [(0, (slice(0, 4), slice(0, 8)), (0, 0))], (8 * dt.itemsize, dt.itemsize), 0)
        assert t.layout.flags == layout_flags(chain, dt, encode=True)
        assert t.layout.itemsize == dt.itemsize
        assert bytes(t.layout.fill)[: dt.itemsize] == np.zeros(1, dt).tobytes()


# ------------------------------------------------------------------ the shared fill-equality function
def _hook(dt, fill, items):
    from zarr_hip import _native as N

    dt = np.dtype(dt)
    flags = N.LF_FLOAT if dt.kind == "f" else N.LF_COMPLEX if dt.kind == "c" else 0
    items = np.ascontiguousarray(items, dt)
    f = _one(fill, dt)
    eq = np.zeros(len(items), np.uint8)
    fnan = ctypes.c_uint32(7)
    N.check(N.lib().zhip_emulate_fill_eq(dt.itemsize, flags, f.ctypes.data, items.ctypes.data, len(items),
                                         eq.ctypes.data, ctypes.addressof(fnan)), "zhip_emulate_fill_eq")
    return eq.astype(bool), fnan.value


@pytest.mark.parametrize("name,fid,fill", D.EMPTINESS, ids=[f"{n}-{f}" for n, f, _ in D.EMPTINESS])
def test_fill_eq_hook_matches_the_oracle(name, fid, fill):
    """Every item of the truth table (each class's bulk, first and last value,
    plus every other row's fill of the dtype), one by one, against
    O.all_equal on a one-item array."""
    dt = np.dtype(name)
    items = [v for c in D.classes_of(dt, fill) for v in c[1:] if v is not None] + [f for _, f in D.fills_of(dt)]
    items = np.array(items, dt)
    got, fnan = _hook(dt, fill, items)
    want = [O.all_equal(items[i:i + 1], np.asarray(fill, dt)) for i in range(len(items))]
    assert got.tolist() == want
    assert fnan == int(dt.kind in "fc" and bool(np.isnan(fill)))


@pytest.mark.parametrize("name", D.FLOATS)
def test_fill_eq_hook_nan_boundaries(name):
    """Either side of each NaN threshold, both signs: infinity is not a NaN,
    the smallest payload is (0x7C00 / 0x7C01 for float16 and their wider
    forms), against numpy's isnan."""
    dt = np.dtype(name)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]
    bits = 8 * dt.itemsize
    mant = {2: 10, 4: 23, 8: 52}[dt.itemsize]
    inf = ((1 << (bits - 1)) - 1) >> mant << mant
    sign = 1 << (bits - 1)
    pats = [inf - 1, inf, inf + 1, inf | (1 << (mant - 1)), sign - 1, 1 << 31 if bits == 64 else 1, inf | (1 << 32 if bits == 64 else 2)]
    pats = np.array(pats + [p | sign for p in pats], u)
    items = pats.view(dt)
    nan_fill = np.array([inf + 1], u).view(dt)[0]
    got, fnan = _hook(dt, nan_fill, items)
    assert fnan == 1
    assert got.tolist() == np.isnan(items).tolist()
    got, fnan = _hook(dt, np.array([inf], u).view(dt)[0], items)  # an infinite fill: bits only
    assert fnan == 0 and got.tolist() == (pats == inf).tolist()


def test_fill_eq_hook_refuses():
    from zarr_hip import _native as N

    z = np.zeros(2, np.uint64)
    eq = np.zeros(2, np.uint8)
    L = N.lib()
    assert L.zhip_emulate_fill_eq(16, 0, z.ctypes.data, z.ctypes.data, 1, eq.ctypes.data, None) == N.E_UNSUPPORTED
    assert L.zhip_emulate_fill_eq(4, N.LF_COMPLEX, z.ctypes.data, z.ctypes.data, 1, eq.ctypes.data, None) == N.E_INVALID
    assert L.zhip_emulate_fill_eq(8, 0, None, z.ctypes.data, 1, eq.ctypes.data, None) == N.E_INVALID


# ------------------------------------------------------------------ refusals
REFUSED = ["complex128", "datetime64[s]", "timedelta64[ms]", "S3", "U2", "V16",
           np.dtype([("a", "<i4"), ("b", "<f4")]), "object"]
if hasattr(np, "float128"):
    REFUSED.append("float128")


@pytest.mark.parametrize("dtype", REFUSED, ids=[str(np.dtype(d)) for d in REFUSED])
def test_unsupported_dtypes_are_refused_by_name(dtype):
    """One named error, raised by the chain analysis every read, write,
    prepare_read and fancy path starts with (and by the device dtype map),
    with the dtype's name in the message -- sharded chains refuse at the outer
    level, before the inner chain is looked at."""
    import zarr_hip
    from zarr_hip.buffer import UnsupportedDTypeError, require_device_dtype, torch_dtype
    from zarr_hip.codecs import parse_codecs
    from zarr_hip.planner import analyze_chain
    from zarr_hip.spec import ArraySpec

    dt = np.dtype(dtype)
    assert issubclass(UnsupportedDTypeError, TypeError) and zarr_hip.UnsupportedDTypeError is UnsupportedDTypeError
    spec = ArraySpec((8, 8), dt, None)
    for codecs in ([D.LE, D.CRC], [D.SHARD((4, 4), [D.LE, D.CRC])]):
        with pytest.raises(UnsupportedDTypeError) as e:
            analyze_chain(parse_codecs(codecs), spec)
        assert dt.name in str(e.value)
    for f in (require_device_dtype, torch_dtype):
        with pytest.raises(UnsupportedDTypeError) as e:
            f(dt)
        assert dt.name in str(e.value)


def test_every_table_dtype_is_admitted():
    from zarr_hip.buffer import DEVICE_DTYPES, require_device_dtype

    assert sorted(DEVICE_DTYPES) == sorted(D.NAMES)
    for name in D.NAMES:
        for order in "<>":
            assert require_device_dtype(np.dtype(name).newbyteorder(order)) == np.dtype(name)


def test_plan_create_refuses_a_malformed_complex_layout():
    """The ABI's own check: ZHIP_LF_COMPLEX is an 8-byte item, never with
    ZHIP_LF_FLOAT; a 16-byte item is refused as before."""
    from zarr_hip import _native as N
    from zarr_hip.planner import _make_layout

    for item, flags in ((4, N.LF_COMPLEX), (8, N.LF_COMPLEX | N.LF_FLOAT), (16, 0)):
        L = _make_layout([4, 8], item, [8 * item, item], flags, b"\0" * item)
        with pytest.raises(N.NativeError):
            N.Plan(L, upload=False)
    N.Plan(_make_layout([4, 8], 8, [64, 8], N.LF_COMPLEX | N.LF_SWAP, b"\0" * 8), upload=False)
