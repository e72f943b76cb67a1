"""Every element type the device path admits, crossed with every kernel family:
the one table behind tests/test_dtype_rules.py (CPU) and
tests/test_gpu_dtype_matrix.py (GPU).

The kernels are instantiated by item size and byte-order mode, not by type
(csrc/zhip_dispatch.h), so what a dtype can get wrong is its byte order in
store (complex64 swaps per component), the fill bytes a missing chunk shows,
and the rule by which a chunk counts as empty (NDBuffer.all_equal: bits for
integers, bits-or-NaN for floats, np.array_equal(equal_nan=True) for complex).

Nothing here is an expectation: the oracle (O.write / O.read / O.all_equal)
decides every key set and every byte.  The table fixes only the inputs and
the kernel each row must take.

Layout families -- the smallest layout that takes one kernel family; the last
(or the transposed innermost) dim is scaled by the item size so a family's
chunk has the same bytes for every dtype.  Geometries from
test_gpu_kernel_matrix.py, test_gpu_encode.py, test_gpu_shard_index.py and
tile_cases.py.  Encode / decode name the kernel zhip_last_kernel() must
report (decode names ending in "*" are prefixes).

complex64 takes the same family as every other 8-byte item: each kernel
family has the complex form (a compile-time item mode), none is narrowed."""

from collections import namedtuple

import numpy as np

LE = {"name": "bytes", "configuration": {"endian": "little"}}
BE = {"name": "bytes", "configuration": {"endian": "big"}}
CRC = {"name": "crc32c"}


def T(order):
    return {"name": "transpose", "configuration": {"order": list(order)}}


def SHARD(inner_shape, codecs, loc="end"):
    return {"name": "sharding_indexed", "configuration": {
        "chunk_shape": list(inner_shape), "codecs": list(codecs), "index_codecs": [LE, CRC],
        "index_location": loc}}


# ---------------------------------------------------------------- dtypes
NAMES = ["bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64",
         "float16", "float32", "float64", "complex64"]
# (name, endian codec, id): multi-byte items in both byte orders
DTYPES = [(n, e, f"{n}-{'le' if e is LE else 'be'}") for n in NAMES
          for e in ((LE,) if np.dtype(n).itemsize == 1 else (LE, BE))]
FLOATS = ("float16", "float32", "float64")

# ---------------------------------------------------------------- families
# chunk(it): the chunk shape for an item size; shape(it): the round-trip array;
# order: a transpose codec's order; inner(it): sharded rows (chunk = the shard)
Family = namedtuple("Family", "id chunk shape order crc inner encode decode")

_R4_GEN = {1: (3, 5, 48, 48), 2: (3, 5, 40, 24), 4: (3, 5, 40, 20), 8: (3, 5, 40, 20)}  # tile_cases._R4_GEN


def _grid(chunk, grid):
    return lambda it: tuple(c * g for c, g in zip(chunk(it), grid))


def _fam(id, chunk, grid, encode, decode, order=None, crc=True, inner=None, shape=None):
    return Family(id, chunk, shape or _grid(chunk, grid), order, crc, inner, encode, decode)


FAMILIES = [
    # not a row layout: ragged in the last two dims, so edge chunks are boxes (the persistent kernels)
    _fam("generic", lambda it: (16, 16, 32 // it), None, "k_encode", "k_decode",
         shape=lambda it: (40, 33, 80 // it)),
    # row layouts (planner._rows_ok): 16 KiB, one unit, four chunks per workgroup
    _fam("quad", lambda it: (4, 32, 128 // it), (1, 1, 3), "k_encode_quad", "k_decode_lead4"),
    # 96 KiB: three units
    _fam("pair", lambda it: (3, 64, 512 // it), (1, 1, 3), "k_encode_pair", "k_decode_pair"),
    # 256 KiB: eight units, S = 8
    _fam("il", lambda it: (32, 32, 256 // it), (1, 1, 3), "k_encode_il", "k_decode_ilh"),
    # transposed, full tiles at one uniform step: stored (128, 1 KiB rows), T = 8
    _fam("tile2", lambda it: (1024 // it, 128), (2, 2), "k_encode_tile2", "k_decode_tile2w", order=(1, 0)),
    _fam("tile4", lambda it: (1024 // it, 128), (2, 2), "k_encode_tile4", "k_decode_tile4", order=(1, 0),
         crc=False),
    # grouped tiles: stored (3, 48 B of tq, 4, 80-byte rows), gd = the 4
    _fam("tileg", lambda it: (4, 3, 80 // it, 48 // it), (2, 2, 1, 2), "k_encode_tileg", "k_decode_tileg2w",
         order=(1, 3, 0, 2)),
    # general tiles: no group dim (other stored dims 3 and 5), partial tiles
    _fam("tile", lambda it: _R4_GEN[it], (2, 1, 1, 2), "k_encode_tile", "k_decode_tile", order=(3, 0, 1, 2)),
    # prefix boxes: the rank-2 general layout of tile_cases.RAGGED (stored rows of 400 bytes) in an array ragged
    # in both dims, so every edge chunk is a prefix box and the whole write takes k_encode_tile; a ragged array
    # decodes through the persistent k_decode
    _fam("tile_prefix", lambda it: (400 // it, 80), None, "k_encode_tile", "k_decode", order=(1, 0),
         shape=lambda it: (600 // it, 208)),  # (rows of 208 items: 16-byte multiples at every item size)
    # 2 KiB inner chunks, eight per shard (test_gpu_encode.test_sharded_write); the pack kernel follows the
    # inner chunks' encode without a name of its own
    _fam("sharded", lambda it: (16, 16, 64 // it), (2, 2, 2), "k_encode", "k_decode*",
         inner=lambda it: (8, 8, 32 // it)),
]
FAMILY = {f.id: f for f in FAMILIES}
RAGGED = ("generic", "tile_prefix")  # families whose kernel needs an array that is no multiple of the chunk


def codecs_for(fam, endian, it):
    chain = ([T(fam.order)] if fam.order else []) + [endian] + ([CRC] if fam.crc else [])
    if fam.inner:
        return [SHARD(fam.inner(it), chain)]
    return chain


def unit(fam, it):
    """The shape emptiness is decided on: the inner chunk of a sharded family."""
    return fam.inner(it) if fam.inner else fam.chunk(it)


def kernel_matches(got: str, want: str) -> bool:
    return got.startswith(want[:-1]) if want.endswith("*") else got == want


# ---------------------------------------------------------------- values
def sample(shape, dtype, seed=0):
    """Every byte random (so every byte position of an item differs from its
    neighbours: a wrong swap width cannot cancel), NaNs and all."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dt.kind == "b":
        return rng.integers(0, 2, size=shape).astype(bool)
    return rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8).view(dt).reshape(shape)


_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
_QNAN = {2: 0x7E00, 4: 0x7FC00000, 8: 0x7FF8000000000000}
_SNAN_NEG = {2: 0xFC01, 4: 0xFF800001, 8: 0xFFF0000000000001}  # sign set, payload 1
_NEG0 = {2: 0x8000, 4: 0x80000000, 8: 0x8000000000000000}


def _fbits(dt, bits):
    return np.array([bits], _UINT[dt.itemsize]).view(dt)[0]


def _c64(re_bits, im_bits):
    return np.array([re_bits, im_bits], np.uint32).view(np.complex64)[0]


_F32 = {"+0": 0x00000000, "-0": 0x80000000, "qnan": 0x7FC00000, "snan": 0x7F800001, "-snan": 0xFF800001,
        "inf": 0x7F800000, "1": 0x3F800000, "1.5": 0x3FC00000, "-2.5": 0xC0200000}


def C(re, im):
    """A complex64 from the names of two float32 bit patterns (no arithmetic:
    -0.0+0j in Python is +0)."""
    return _c64(_F32[re], _F32[im])


# a class is (id, bulk, first, last): the chunk is `bulk` everywhere, with its
# first / last element replaced when given
def float_classes(dtype):
    dt = np.dtype(dtype)
    q, s = _fbits(dt, _QNAN[dt.itemsize]), _fbits(dt, _SNAN_NEG[dt.itemsize])
    z, nz = dt.type(0.0), _fbits(dt, _NEG0[dt.itemsize])
    return [("pos0", z, None, None), ("neg0", nz, None, None), ("qnan", q, None, None), ("neg_snan", s, None, None),
            ("inf", dt.type(np.inf), None, None), ("one5", dt.type(1.5), None, None),
            ("nan_but_first", q, dt.type(1.5), None), ("nan_but_last", q, None, dt.type(1.5)),
            ("pos0_but_last_neg0", z, None, nz)]


def complex_classes():
    qq = C("qnan", "qnan")
    return [("p0p0", C("+0", "+0"), None, None), ("n0p0", C("-0", "+0"), None, None),
            ("p0n0", C("+0", "-0"), None, None), ("qnan_0", C("qnan", "+0"), None, None),
            ("one_negsnan", C("1", "-snan"), None, None), ("qnan_snan", C("qnan", "snan"), None, None),
            ("inf_0", C("inf", "+0"), None, None), ("one5_m2_5", C("1.5", "-2.5"), None, None),
            # every component NaN except the real part of the first item (still a NaN item)
            ("nan_but_first_component", qq, C("1.5", "qnan"), None),
            ("nan_but_last_item", qq, None, C("1.5", "-2.5"))]


def float_fills(dtype):
    dt = np.dtype(dtype)
    return [("0.0", dt.type(0.0)), ("-0.0", _fbits(dt, _NEG0[dt.itemsize])), ("nan", _fbits(dt, _QNAN[dt.itemsize])),
            ("1.5", dt.type(1.5))]


def complex_fills():
    return [("0j", C("+0", "+0")), ("-0.0+0j", C("-0", "+0")), ("nan+0j", C("qnan", "+0")),
            ("nanj", C("+0", "qnan")), ("1.5-2.5j", C("1.5", "-2.5"))]


def int_fills(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return [("0", np.bool_(False)), ("max", np.bool_(True))]
    info = np.iinfo(dt)
    return [("0", dt.type(0)), ("min", dt.type(info.min)), ("max", dt.type(info.max))] if info.min else \
        [("0", dt.type(0)), ("max", dt.type(info.max))]


def int_classes(dtype, fill):
    dt = np.dtype(dtype)
    other = np.bool_(not fill) if dt.kind == "b" else dt.type(int(fill) ^ 1)
    return [("fill", fill, None, None), ("but_first", fill, other, None), ("but_last", fill, None, other),
            ("other", other, None, None)]


def fills_of(dtype):
    dt = np.dtype(dtype)
    return float_fills(dt) if dt.kind == "f" else complex_fills() if dt.kind == "c" else int_fills(dt)


def classes_of(dtype, fill):
    dt = np.dtype(dtype)
    return float_classes(dt) if dt.kind == "f" else complex_classes() if dt.kind == "c" else int_classes(dt, fill)


def class_chunk(cls, shape, dtype):
    """One chunk of a content class, C order."""
    _, bulk, first, last = cls
    a = np.empty(int(np.prod(shape)), np.dtype(dtype))
    a[:] = bulk
    if first is not None:
        a[0] = first
    if last is not None:
        a[-1] = last
    return a.reshape(shape)


def same_bytes(a, b) -> bool:
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# (dtype name, fill id, fill): one emptiness row each, per family
EMPTINESS = [(n, fid, fv) for n in NAMES for fid, fv in fills_of(n)]


def truth_table_array(fam, dtype, fill):
    """(shape, data, regions): one unit (chunk, or inner chunk) per content class
    along dim 0, at the origin of the other dims; everything else is the fill.
    regions[i] is class i's selection."""
    dt = np.dtype(dtype)
    it = dt.itemsize
    u, ch = unit(fam, it), fam.chunk(it)
    classes = classes_of(dt, fill)
    n0 = -(-len(classes) * u[0] // ch[0]) * ch[0]  # whole chunks (shards) along dim 0
    rest = fam.shape(it)[1:] if fam.id in RAGGED else ch[1:]
    shape = (n0,) + tuple(rest)
    data = np.empty(shape, dt)
    data[...] = fill
    regions = []
    for i, cls in enumerate(classes):
        sel = (slice(i * u[0], (i + 1) * u[0]),) + tuple(slice(0, s) for s in u[1:])
        data[sel] = class_chunk(cls, u, dt)
        regions.append(sel)
    return shape, data, regions
