"""The plan's table images (csrc/plan_tables.cpp) on the CPU: the bytes
zhip_plan_upload puts on the device, and where every region lies, held to the
values recorded in tests/golden/plan_tables.json for a matrix of layouts that
takes every branch of the layout function -- for the shipped library and for
the tuning build (loaded in a child process).  No GPU needed.

Run as a script, this file prints what the loaded library builds for the
matrix as JSON (the child process of the tuning-build tests does that)."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zarr-python_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_tables.json")

# TableLayout's regions (csrc/zhip_plan_tables.h) in declaration order: the
# order of zhip_plan_table_offsets
ROW_REGIONS = (["horner", "kthread", "kunit", "kpair", "pair.tab", "pair.klane", "pair.kidx"] +
               ["il." + k for k in ("tab", "klane", "kidx", "basis")] +
               ["xw." + k for k in ("tab", "klane", "kidx")] +
               ["ilw1024." + k for k in ("tab", "klane", "kidx")] +
               ["ilw512." + k for k in ("tab", "klane", "kidx")] + ["ilh"] +
               ["il16." + k for k in ("tab", "klane", "kidx", "basis")] +
               ["il32." + k for k in ("tab", "klane", "kidx", "basis")])
TILE_REGIONS = ["t_horner", "t_kthread", "t_kunit", "tile4_tz", "tile4_kq", "tile4_map", "g_tz", "g_map",
                "t4f.tab", "t4f.klane", "t4w.tab", "t4w.klane", "tgw.tab", "tgw.klane", "t2w", "t1w", "tg2w", "t2e",
                "tile2_tab", "tile2_map", "tile2_klane", "tgl", "tbt_ad", "tbt_a4"]
REGIONS = ROW_REGIONS + TILE_REGIONS
# every plan has these (t_horner: every tile image, at offset 0 like an absent region)
ALWAYS = {"horner", "kthread", "kunit", "kpair", "pair.tab", "pair.klane", "pair.kidx", "t_horner"}
# built only with ZHIP_TUNING
TUNING_ONLY = {"ilw1024.tab", "ilw1024.klane", "ilw1024.kidx", "t1w", "tile2_tab", "tile2_map", "tile2_klane", "tgl",
               "tbt_ad", "tbt_a4"}

LF_CRC, LF_SHARDED, LF_NO_WRITE, LF_FLOAT = 1, 4, 16, 32


def _matrix():
    """name -> (shape, itemsize, tq or None, flags, n_inner)."""
    m = {}
    for n in (0, 16, 4096, 32768, 65536, 131072, 258048, 258041, 516096, 1024000, 1081344, 2097152, 8650752):
        m[f"bytes{n}"] = ((n,), 1, None, LF_CRC, 0)
    for n in (258048, 1024000):
        m[f"bytes{n}-nocrc"] = ((n,), 1, None, 0, 0)
        m[f"bytes{n}-nowrite"] = ((n,), 1, None, LF_CRC | LF_NO_WRITE, 0)
        m[f"bytes{n}-sharded"] = ((n,), 1, None, LF_CRC | LF_SHARDED, 8)
    for shape, tq in (((64, 64), 0), ((64, 256), 0), ((4, 64, 64), 1), ((128, 128), 0), ((70, 40), 0),
                      ((128, 64, 64), 1)):
        m["tile" + "x".join(map(str, shape))] = (shape, 4, tq, LF_CRC | LF_FLOAT, 0)
    for shape, tq in (((64, 256), 0), ((4, 64, 64), 1)):
        m["tile" + "x".join(map(str, shape)) + "-nocrc"] = (shape, 4, tq, LF_FLOAT, 0)
    return m


MATRIX = _matrix()


def make_layout(N, spec):
    """zhip_layout of a matrix entry: dim tq is the contiguous one of out
    (out_stride[tq] == itemsize), the others follow in stored order."""
    shape, itemsize, tq, flags, n_inner = spec
    L = N.Layout()
    L.ndim, L.itemsize = len(shape), itemsize
    nbytes = itemsize
    for d, s in enumerate(shape):
        L.shape[d] = s
        nbytes *= s
    order = [d for d in range(len(shape)) if d != tq] + ([tq] if tq is not None else [])
    stride = itemsize
    for d in reversed(order):
        L.out_stride[d] = stride
        stride *= shape[d]
    L.nbytes = nbytes
    L.flags = flags
    L.n_inner = n_inner
    L.index_size = 16 * n_inner + 4 if n_inner else 0
    return L


def collect():
    """What the loaded library builds for the matrix: per layout the two
    images' word counts and CRC-32C, and the regions' offsets and word counts."""
    sys.path[:0] = [p for p in (ROOT, PKG) if p not in sys.path]
    from oracle import oracle as O
    from zarr_hip import _native as N

    out = {}
    for name, spec in MATRIX.items():
        plan = N.Plan(make_layout(N, spec), upload=False)
        images = [plan.table_image(w) for w in (0, 1)]
        offsets, counts = plan.table_regions()
        out[name] = {"words": [int(im.size) for im in images],
                     "crc32c": [int(O.crc32c(im.tobytes())) for im in images],
                     "offsets": offsets, "counts": counts}
    return out


_built = {}


def built(build):
    """collect() for the shipped library (in this process) or the tuning build
    (in a child process, as tests/test_native_abi.py loads it)."""
    if build not in _built:
        if build == "production":
            _built[build] = collect()
        else:
            from zarr_hip import _native as N

            if not os.path.exists(N.TUNING_LIB_PATH):
                pytest.skip("tuning build absent (make -C zarr-python_amd tune)")
            env = dict(os.environ, ZHIP_LIB=N.TUNING_LIB_PATH, ZARR_HIP_ALLOW_LIB_OVERRIDE="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
            _built[build] = json.loads(r.stdout)
    return _built[build]


BUILDS = ["production", "tuning"]


@pytest.mark.parametrize("build", BUILDS)
def test_images_and_offsets_match_the_recorded_ones(build):
    """Word counts, CRC-32C of the bytes and every region offset equal the
    values recorded from the commit before the table builders moved into
    plan_tables.cpp (tests/golden/plan_tables.json; its "how" field says how
    they were recorded)."""
    golden = json.load(open(GOLDEN))[build]
    got = built(build)
    assert sorted(got) == sorted(golden) == sorted(MATRIX)
    for name in MATRIX:
        for key in ("words", "crc32c", "offsets"):
            assert got[name][key] == golden[name][key], (name, key)


@pytest.mark.parametrize("build", BUILDS)
def test_regions_tile_their_image_in_declaration_order(build):
    """Per image, the present regions are disjoint, in ascending address order
    (which is declaration order) and inside the image: each begins where the
    one before ends, the first at 0, the last ends at the image's word count."""
    for name, g in built(build).items():
        assert len(g["offsets"]) == len(g["counts"]) == len(REGIONS), name
        for image, (lo, hi) in enumerate(((0, len(ROW_REGIONS)), (len(ROW_REGIONS), len(REGIONS)))):
            at = 0
            for i in range(lo, hi):
                off, n = g["offsets"][i], g["counts"][i]
                if n == 0:
                    assert off == 0, (name, REGIONS[i])
                    continue
                assert off == at, (name, REGIONS[i])
                at = off + n
            assert at == g["words"][image], (name, image)


@pytest.mark.parametrize("build", BUILDS)
def test_matrix_takes_every_branch_of_the_layout(build):
    """Every optional region is present in at least one layout of the matrix
    and absent in another; the regions of the tuning build alone are absent
    everywhere in the shipped library."""
    got = built(build)
    for i, region in enumerate(REGIONS):
        present = {name for name, g in got.items() if g["counts"][i]}
        if region in ALWAYS:
            want = set(got) if region in ROW_REGIONS else {n for n, g in got.items() if g["words"][1]}
            assert present == want, region
        elif region in TUNING_ONLY and build == "production":
            assert not present, region
        else:
            assert present and present != set(got), region


if __name__ == "__main__":
    print(json.dumps(collect()))
