"""scale_offset and cast_value without a GPU: the codec classes against the
reference's recorded vectors (tests/golden/value_codecs.json), their
validation, the chain split and every refusal, and the CPU hook
zhip_emulate_value_map against the independent reference of value_cases.py
(b byte for byte between sentinel bytes, the error bits, the non-empty words).

The U read and write routes themselves have no CPU seam: the existing CPU
tests drive planners and table builders, never a pipeline read or write (those
need a device), so the routes are covered by tests/test_gpu_value_codecs.py."""

import json
import os

import numpy as np
import pytest

import value_cases as VC
import value_driver as D
from zarr_hip import values as V
from zarr_hip.codecs import (BytesCodec, CastValueCodec, Crc32cCodec, ForeignArrayCodec, GzipCodec, ScaleOffsetCodec,
                             ShardingCodec, TransposeCodec, parse_codecs)
from zarr_hip.pipeline import HipCodecPipeline
from zarr_hip.spec import ArraySpec

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "value_codecs.json")))


def _arr(vals, dt):
    return np.array([np.nan if v == "NaN" else v for v in vals], dtype=dt)


def _run(codecs, spec, data, encode):
    """Whole 1-D arrays through the value codecs on the CPU hook."""
    so = next((c for c in codecs if isinstance(c, ScaleOffsetCodec)), None)
    cast = next((c for c in codecs if isinstance(c, CastValueCodec)), None)
    ops = V.ValueOps(so, cast, spec)
    a_dt, b_dt = (ops.array_dt, ops.stored_dt) if encode else (ops.stored_dt, ops.array_dt)
    a = np.ascontiguousarray(data, a_dt)
    b = np.zeros(len(a), b_dt)
    items, prefix = V.make_items([(0, 0, [(len(a), a_dt.itemsize, b_dt.itemsize)], 0, 0)])
    err, ne = V.emulate(ops.op(encode), items, prefix, a.view(np.uint8), b.view(np.uint8))
    return b, err, ops


# ------------------------------------------------------------ golden vectors
@pytest.mark.parametrize("case", GOLDEN["casts"], ids=lambda c: c["id"])
def test_cast_value_golden_vectors(case):
    codec = CastValueCodec.from_dict({"name": "cast_value", "configuration": case["config"]})
    adt = np.dtype(case["array_dtype"])
    spec = ArraySpec((len(case["input"]),), adt, 0)
    stored, err, ops = _run([codec], spec, _arr(case["input"], adt), True)
    assert err == 0 and stored.dtype == np.dtype(case["config"]["data_type"])
    assert stored.tolist() == case["stored"]
    back, err, _ = _run([codec], spec, stored, False)
    assert err == 0 and back.dtype == adt
    np.testing.assert_array_equal(back, _arr(case["decoded"], adt))


def test_packed_golden_vector():
    g = GOLDEN["packed"]
    codecs = [ScaleOffsetCodec(**g["scale_offset"]), CastValueCodec(**g["cast_value"])]
    data = np.arange(100, dtype="float64") * 0.1
    spec = ArraySpec((100,), np.dtype("float64"), 0)
    stored, err, _ = _run(codecs, spec, data, True)
    assert err == 0 and stored.dtype == np.int16 and stored.tolist() == list(range(100))
    back, err, _ = _run(codecs, spec, stored, False)
    assert err == 0
    np.testing.assert_array_equal(back, np.arange(100, dtype="int16").astype("float64") / 10.0 + 0.0)


def _json(d):
    return json.loads(json.dumps(d))


@pytest.mark.parametrize("g", GOLDEN["cast_value_dicts"] + GOLDEN["scale_offset_dicts"], ids=lambda g: str(g["args"]))
def test_to_dict_and_from_dict(g):
    cls = CastValueCodec if g["dict"]["name"] == "cast_value" else ScaleOffsetCodec
    codec = cls(**g["args"])
    assert _json(codec.to_dict()) == g["dict"]
    assert cls.from_dict(g["dict"]) == codec
    assert cls.from_dict(_json(codec.to_dict())) == codec
    if g["dict"]["name"] == "scale_offset" and not g["args"]:
        assert ScaleOffsetCodec.from_dict("scale_offset") == codec


def test_compute_encoded_size_scales_by_the_item_sizes():
    g = GOLDEN["encoded_size"]
    spec = ArraySpec((10,), np.dtype(g["array_dtype"]), 0)
    assert CastValueCodec(g["data_type"]).compute_encoded_size(g["input_bytes"], spec) == g["encoded_bytes"]
    assert ScaleOffsetCodec(scale=2).compute_encoded_size(80, spec) == 80
    pipe = HipCodecPipeline.from_codecs([ScaleOffsetCodec(scale=2), CastValueCodec("int16"), BytesCodec("little"),
                                         Crc32cCodec()]).evolve_from_array_spec(spec)
    assert pipe.compute_encoded_size(80, spec) == 24


# ---------------------------------------------------------------- validation
def test_validate_errors():
    f32, c64 = np.dtype("float32"), np.dtype("complex64")
    with pytest.raises(ValueError, match="scale must be non-zero"):
        ScaleOffsetCodec(scale=0).validate(shape=(4,), dtype=f32)
    with pytest.raises(ValueError, match="scale must be non-zero"):
        ScaleOffsetCodec(scale="0").validate(shape=(4,), dtype=np.dtype("int16"))
    with pytest.raises(ValueError, match="only supports integer and floating-point"):
        ScaleOffsetCodec().validate(shape=(4,), dtype=c64)
    with pytest.raises(ValueError, match="offset value 300 is not representable in dtype uint8"):
        ScaleOffsetCodec(offset=300).validate(shape=(4,), dtype=np.dtype("uint8"))
    with pytest.raises(ValueError, match="not representable"):
        ScaleOffsetCodec(scale=1.5).validate(shape=(4,), dtype=np.dtype("int32"))
    ScaleOffsetCodec(offset="NaN", scale="Infinity").validate(shape=(4,), dtype=f32)
    with pytest.raises(TypeError):
        ScaleOffsetCodec(offset=[1])
    with pytest.raises(ValueError, match="wrap"):
        CastValueCodec("float32", out_of_range="wrap").validate(shape=(4,), dtype=np.dtype("float64"))
    with pytest.raises(ValueError, match="scalar_map encode value 300 is not representable in dtype uint8"):
        CastValueCodec("uint8", scalar_map={"encode": [["NaN", 300]]}).validate(shape=(4,), dtype=f32)
    with pytest.raises(ValueError, match="scalar_map decode key"):
        CastValueCodec("uint8", scalar_map={"decode": [[1.5, 0]]}).validate(shape=(4,), dtype=f32)
    with pytest.raises(ValueError, match="only supports integer and floating-point"):
        CastValueCodec("int16").validate(shape=(4,), dtype=c64)
    with pytest.raises(ValueError, match="Invalid target data type"):
        CastValueCodec("complex64")
    with pytest.raises(ValueError):
        CastValueCodec("int16", rounding="sideways")


def test_dtypes_outside_the_table_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="scale_offset: dtype int64"):
        ScaleOffsetCodec(scale=2).validate(shape=(4,), dtype=np.dtype("int64"))
    with pytest.raises(NotImplementedError, match="scale_offset: dtype uint64"):
        ScaleOffsetCodec().resolve_metadata(ArraySpec((4,), np.dtype("uint64"), 0))
    for adt, sdt in (("float32", "int32"), ("float32", "float64"), ("float64", "int64"), ("int32", "uint64"),
                     ("uint64", "int8"), ("float32", "float16"), ("float32", "int4")):
        with pytest.raises(NotImplementedError, match="cast_value"):
            CastValueCodec(sdt).validate(shape=(4,), dtype=np.dtype(adt))
    many = {"encode": [[i, i] for i in range(9)]}
    with pytest.raises(NotImplementedError, match="cast_value: more than 8 scalar_map entries"):
        CastValueCodec("int8", scalar_map=many).validate(shape=(4,), dtype=np.dtype("int16"))


def test_resolve_metadata_fills():
    s = ArraySpec((8,), np.dtype("float32"), 0.25)
    s1 = ScaleOffsetCodec(offset=-2.5, scale=10).resolve_metadata(s)
    assert s1.dtype == np.float32 and s1.fill_value == 27.5
    s2 = CastValueCodec("int16").resolve_metadata(s1)
    assert s2.dtype == np.int16 and s2.fill_value == 28  # ties to even
    assert CastValueCodec("int16", rounding="towards-zero").resolve_metadata(s1).fill_value == 27
    nan = ArraySpec((8,), np.dtype("float32"), float("nan"))
    with pytest.raises(ValueError, match="cast_value: the fill value"):
        CastValueCodec("int16").resolve_metadata(nan)
    mapped = CastValueCodec("int16", scalar_map={"encode": [["NaN", -999]]}).resolve_metadata(nan)
    assert mapped.fill_value == -999
    with pytest.raises(ValueError, match="cast_value: the fill value"):
        CastValueCodec("uint8").resolve_metadata(ArraySpec((8,), np.dtype("int16"), -1))
    assert CastValueCodec("uint8", out_of_range="wrap").resolve_metadata(
        ArraySpec((8,), np.dtype("int16"), -1)).fill_value == 255
    with pytest.raises(ValueError, match="scale_offset produced a value outside the range of dtype int8"):
        ScaleOffsetCodec(offset=-5, scale=3).resolve_metadata(ArraySpec((8,), np.dtype("int8"), 100))
    assert ScaleOffsetCodec(offset=1, scale=3).resolve_metadata(ArraySpec((8,), np.dtype("int8"), None)).fill_value == -3


# -------------------------------------------------------------- parse_codecs
class ArrayArrayCodec:
    pass


class FakeScaleOffset(ArrayArrayCodec):
    def to_dict(self):
        return {"name": "scale_offset", "configuration": {"offset": 1, "scale": 4}}


class FakeCastValue(ArrayArrayCodec):
    def to_dict(self):
        return {"name": "cast_value", "configuration": {"data_type": "uint8", "out_of_range": "clamp"}}


class FakeOther(ArrayArrayCodec):
    def to_dict(self):
        return {"name": "bitround", "configuration": {"keepbits": 3}}


def test_parse_codecs_accepts_dicts_names_and_zarr_instances():
    got = parse_codecs([{"name": "scale_offset", "configuration": {"scale": 4, "offset": 1}}, "scale_offset",
                        {"name": "cast_value", "configuration": {"data_type": "uint8", "out_of_range": "clamp"}}])
    assert got == [ScaleOffsetCodec(offset=1, scale=4), ScaleOffsetCodec(),
                   CastValueCodec("uint8", out_of_range="clamp")]
    got = parse_codecs([FakeScaleOffset(), FakeCastValue(), FakeOther()])
    assert got[0] == ScaleOffsetCodec(offset=1, scale=4)
    assert got[1] == CastValueCodec("uint8", out_of_range="clamp")
    assert isinstance(got[2], ForeignArrayCodec)  # any other array->array codec: today's behaviour
    assert parse_codecs(got[:2]) == got[:2]


# ------------------------------------------------------------------ the split
SO, CV = ScaleOffsetCodec(offset=-2.5, scale=10), CastValueCodec("int16")
TAIL = (BytesCodec("big"), Crc32cCodec())
SPEC = ArraySpec((8, 8), np.dtype("float32"), 0.25)


def _pipe(codecs, spec=SPEC, **kw):
    return HipCodecPipeline.from_codecs(codecs, warn=False, **kw).evolve_from_array_spec(spec)


def test_the_split_moves_value_codecs_out_from_anywhere_among_the_transposes():
    t = TransposeCodec((1, 0))
    stored = None
    for aa in ((SO, CV, t), (t, SO, CV), (SO, t, CV)):
        vs = _pipe(aa + TAIL)._value_split()
        assert vs[0] == SO and vs[1] == CV and vs[3] is False
        assert vs[2].codecs == (t,) + TAIL
        assert vs[2]._value_split() is None
        stored = stored or vs[2].codecs
        assert vs[2].codecs == stored
    assert _pipe(TAIL)._value_split() is None
    vs = _pipe((CV,) + TAIL)._value_split()
    assert vs[0] is None and vs[1] == CV
    ops = V.ValueOps(SO, CV, SPEC)
    assert ops.stored_dt == np.int16 and ops.stored_fill == 28 and ops.array_fill == 0.25
    # the bytes codec was evolved against the stored dtype
    one = _pipe((CastValueCodec("uint8", out_of_range="clamp"), BytesCodec("little")))
    assert one._value_split()[2].codecs == (BytesCodec(None),)


def test_refusals_name_the_codec_and_the_reason():
    from zarr_hip.planner import analyze_chain

    with pytest.raises(NotImplementedError, match="array->array codec"):
        analyze_chain((SO,) + TAIL, SPEC)  # analyze_chain only ever sees the stored chain
    for seq in ((CV, SO), (SO, SO), (CV, CV), (SO, CV, SO)):
        with pytest.raises(NotImplementedError, match="any other sequence"):
            HipCodecPipeline.from_codecs(seq + (BytesCodec("little"),), warn=False)._value_split()
    inner = ShardingCodec(chunk_shape=(4, 4), codecs=(BytesCodec("little"),))
    with pytest.raises(NotImplementedError, match="scale_offset: value codecs around a sharding codec"):
        _pipe((SO, inner))._value_split()
    sharded = ShardingCodec(chunk_shape=(4, 4), codecs=(SO, CV, BytesCodec("little")))
    vs = _pipe((sharded,))._value_split()
    assert vs[3] is True and vs[2].codecs[0].codecs == (BytesCodec("little"),)
    with pytest.raises(NotImplementedError, match="lone sharding_indexed"):
        _pipe((TransposeCodec((1, 0)), sharded))._value_split()
    nested = ShardingCodec(chunk_shape=(8, 8), codecs=(sharded,))
    with pytest.raises(NotImplementedError, match="nested"):
        _pipe((nested,), ArraySpec((16, 16), np.dtype("float32"), 0.25))._value_split()
    item = [(None, SPEC, (slice(0, 8), slice(0, 8)), (slice(0, 8), slice(0, 8)), True)]
    p = _pipe((SO, CV) + TAIL)
    with pytest.raises(NotImplementedError, match="scale_offset: prepare_read"):
        p.prepare_read(item, None)
    with pytest.raises(NotImplementedError, match="scale_offset: decode_sync"):
        p.decode_sync([(b"", SPEC)])
    with pytest.raises(NotImplementedError, match="scale_offset: encode_sync"):
        p.encode_sync([(np.zeros((8, 8), np.float32), SPEC)])
    other = ArraySpec((8, 4), np.dtype("float32"), 0.25)
    mixed = item + [(None, other, (slice(0, 8), slice(0, 4)), (slice(0, 8), slice(8, 12)), True)]
    with pytest.raises(NotImplementedError, match="scale_offset: a batch of mixed chunk specs"):
        V._one_spec(p, mixed)
    # S: writes and several devices
    ps = _pipe((sharded,))
    with pytest.raises(NotImplementedError, match="scale_offset: writes through value codecs inside a sharding"):
        V.write(ps, ps._value_split(), item, np.float32(1), (), True)
    pm = _pipe((sharded,), devices=(0, 1))
    with pytest.raises(NotImplementedError, match="scale_offset: value codecs inside a sharding codec are served on one"):
        V.read(pm, pm._value_split(), item, np.zeros((8, 8), np.float32), ())


def test_the_sharded_form_is_refused_through_a_host_stage():
    sharded = ShardingCodec(chunk_shape=(4, 4), codecs=(SO, CV, BytesCodec("little")))
    # an outer bytes->bytes codec (a compressor, a checksum) after the sharding codec: refused by the split
    for outer in (GzipCodec(level=1), Crc32cCodec()):
        with pytest.raises(NotImplementedError, match="scale_offset: value codecs inside a sharding codec are served "
                                                      "for a lone sharding_indexed"):
            _pipe((sharded, outer))._value_split()
    with pytest.raises(NotImplementedError, match="cast_value: .*lone sharding_indexed"):
        _pipe((ShardingCodec(chunk_shape=(4, 4), codecs=(CV, BytesCodec("little"))), GzipCodec(level=1)))._value_split()
    # a host-stage codec among the INNER codecs passes the split (the stored
    # chain keeps it) and is refused by the read, by codec name
    item = [(None, SPEC, (slice(0, 8), slice(0, 8)), (slice(0, 8), slice(0, 8)), True)]
    inner = ShardingCodec(chunk_shape=(4, 4), codecs=(SO, CV, BytesCodec("little"), GzipCodec(level=1)))
    ph = _pipe((inner,))
    vs = ph._value_split()
    assert vs[3] is True and vs[2].codecs[0].codecs == (BytesCodec("little"), GzipCodec(level=1))
    with pytest.raises(NotImplementedError, match="scale_offset: value codecs inside a sharding codec are served on one "
                                                  "device without a host stage"):
        V.read(ph, vs, item, np.zeros((8, 8), np.float32), ())
    with pytest.raises(NotImplementedError, match="scale_offset: writes through value codecs inside a sharding"):
        V.write(ph, vs, item, np.float32(1), (), True)
    pc = _pipe((ShardingCodec(chunk_shape=(4, 4), codecs=(CV, BytesCodec("little"), GzipCodec(level=1))),))
    with pytest.raises(NotImplementedError, match="cast_value: value codecs inside a sharding codec are served on one"):
        V.read(pc, pc._value_split(), item, np.zeros((8, 8), np.float32), ())


# ------------------------------------------------------- the hook vs the reference
def test_the_cases_reach_every_error_and_both_empty_verdicts():
    errs, nes = 0, set()
    for name in D.value_case_names():
        desc, items, a, want, err, ne = D.value_case(name)
        errs |= err
        if desc["encode"]:
            nes |= set(ne)
    for dn, sn in D.shape_case_ids():
        desc, items, status, a, want, err, ne = D.shape_case(dn, sn)
        if desc["encode"]:
            nes |= set(ne)
    assert errs == VC.E_INEXACT | VC.E_SO_RANGE | VC.E_CAST_RANGE | VC.E_NAN
    assert nes == {0, 1}


@pytest.mark.parametrize("name", D.value_case_names())
def test_hook_values_match_the_reference(name):
    desc, items, a, want, err, ne = D.value_case(name)
    got, gerr, gne = D.run_hook(desc, items, a, len(want))
    assert gerr == err
    assert got == want
    if desc["encode"]:
        assert gne == ne


@pytest.mark.parametrize("dn,sn", D.shape_case_ids())
def test_hook_item_shapes_match_the_reference(dn, sn):
    desc, items, status, a, want, err, ne = D.shape_case(dn, sn)
    got, gerr, gne = D.run_hook(desc, items, a, len(want), status)
    assert gerr == err
    assert got == want
    if desc["encode"]:
        assert gne == ne


def test_the_hook_checks_its_tables_and_bounds():
    from zarr_hip import _native as N

    desc = D.SHAPE_DESCS["f32-i16-dec"]
    a, b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    items, prefix = V.make_items([(0, 0, [(40, 2, 4)], 0, 0)])  # b needs 160 bytes
    with pytest.raises(N.NativeError, match="outside its buffer"):
        V.emulate(D.op_of(desc), items, prefix, a, b)
    items, prefix = V.make_items([(0, 0, [(4, 2, 4)], N.VI_STATUS, 3)])
    with pytest.raises(N.NativeError, match="status index"):
        V.emulate(D.op_of(desc), items, prefix, a, b)
    op = D.op_of(desc)
    op[0]["stored_dt"] = N.VT_I32
    items, prefix = V.make_items([(0, 0, [(4, 4, 4)], 0, 0)])
    with pytest.raises(N.NativeError, match="outside the served table"):
        V.emulate(op, items, prefix, a, b)
