"""The named cases of the device-built point tables (zhip_points_count /
zhip_points_fill, include/zarrhip.h), shared by test_points_plan.py (the CPU
hook against the host route's tables) and test_gpu_points_kernel.py (the
kernels against the hook).  Not a test module."""

from dataclasses import dataclass

import ctypes

import numpy as np

from zarr_hip import _native as N
from zarr_hip import points as P

ITEMSIZE = 4
RUN = N.POINTS_RUN
BINS = N.POINTS_LDS_BINS


@dataclass
class Case:
    shape: tuple
    chunks: tuple
    coords: tuple          # one int64 array of n entries per dimension
    write: bool = False
    stride: int = ITEMSIZE  # out stride (read) / value stride (write; 0: a scalar value)
    err: int = 0           # the error bits the case must set

    @property
    def n(self) -> int:
        return int(self.coords[0].size)

    @property
    def grid(self) -> tuple:
        return tuple(-(-s // c) for s, c in zip(self.shape, self.chunks))

    @property
    def n_chunks(self) -> int:
        return int(np.prod(self.grid))

    def slot_strides(self) -> list:
        st = [ITEMSIZE] * len(self.chunks)
        for d in range(len(self.chunks) - 2, -1, -1):
            st[d] = st[d + 1] * self.chunks[d + 1]
        return st

    def geom(self) -> np.ndarray:
        return P.points_geom(self.shape, self.chunks, self.slot_strides(), self.stride, self.write)

    def wrapped(self) -> tuple:
        return tuple(np.where(c < 0, c + s, c) for c, s in zip(self.coords, self.shape))

    def rix(self) -> np.ndarray:
        """Row-major chunk index of every point (in-range cases)."""
        return np.ravel_multi_index(tuple(w // c for w, c in zip(self.wrapped(), self.chunks)), self.grid)


def coord_ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def run_hook(case: Case):
    """zhip_emulate_points: (counts, error word, first, cursor, table)."""
    coords = [np.ascontiguousarray(c, dtype=np.int64) for c in case.coords]
    g = case.geom()
    nc = case.n_chunks
    counts, first, cursor = (np.full(nc, 0xDEAD, np.uint32) for _ in range(3))
    err = np.full(1, 0xDEAD, np.uint32)
    table = np.full((max(case.n, 1), 2), -7, np.int64)
    N.check(N.lib().zhip_emulate_points(g.ctypes.data, coord_ptrs(coords), case.n, counts.ctypes.data, err.ctypes.data,
                                        first.ctypes.data, cursor.ctypes.data, table.ctypes.data),
            "zhip_emulate_points")
    return counts, int(err[0]), first, cursor, table


def chunk_pairs(table: np.ndarray, first: np.ndarray, counts: np.ndarray) -> dict:
    """{rix: the chunk's pairs, sorted} -- the order inside a chunk's range is unspecified."""
    out = {}
    for r in np.nonzero(counts)[0]:
        t = table[int(first[r]):int(first[r]) + int(counts[r])]
        out[int(r)] = t[np.lexsort((t[:, 1], t[:, 0]))]
    return out


def _uniform(rng, shape, n, negative=False):
    return tuple(rng.integers(-s if negative else 0, s, n).astype(np.int64) for s in shape)


def _cases() -> dict:
    rng = np.random.default_rng(20)
    c: dict = {}
    edge = ((50, 37, 29), (7, 5, 3))
    cube = ((50, 37, 29), (16, 16, 16))
    c["1d"] = Case((1000,), (64,), _uniform(rng, (1000,), 700, True))
    c["1d-chunk-1"] = Case((300,), (1,), _uniform(rng, (300,), 900, True))
    c["2d-chunks-3-1"] = Case((10, 9), (3, 1), _uniform(rng, (10, 9), 500, True))
    c["3d-edges-7-5-3"] = Case(*edge, _uniform(rng, edge[0], 3000, True))
    c["3d-edges-16"] = Case(*cube, _uniform(rng, cube[0], 3000, True))
    c["4d"] = Case((9, 10, 11, 12), (4, 4, 4, 4), _uniform(rng, (9, 10, 11, 12), 2500, True))
    c["4d-chunks-1-3-7-16"] = Case((5, 10, 20, 40), (1, 3, 7, 16), _uniform(rng, (5, 10, 20, 40), 2500, True))
    # the ends of the valid range: -n and n - 1 in every dimension
    ends = tuple(np.array([-s, s - 1, 0, -1, -s, s - 1], np.int64) for s in edge[0])
    c["ends-valid"] = Case(*edge, ends)
    for d in range(3):  # n and -n - 1: exactly that dimension's bit, nothing counted
        for name, v in (("n", edge[0][d]), ("minus-n-1", -edge[0][d] - 1)):
            co = [np.array([1], np.int64) for _ in range(3)]
            co[d] = np.array([v], np.int64)
            c[f"oob-{name}-dim{d}"] = Case(*edge, tuple(co), err=1 << d)
    bad = list(_uniform(rng, cube[0], 600))
    bad[0][[5, 300]] = [50, -51]
    bad[2][[5, 599]] = [29, 1 << 40]
    c["oob-among-valid"] = Case(*cube, tuple(bad), err=0b101)
    rep = _uniform(rng, edge[0], 9)
    c["repeated"] = Case(*edge, tuple(np.tile(x, 40) for x in rep))
    c["one-chunk"] = Case(*cube, tuple(rng.integers(16, min(32, s), 2500).astype(np.int64) for s in cube[0]))
    per = np.stack(np.meshgrid(*[np.arange(g) for g in (8, 8, 10)], indexing="ij"), -1).reshape(-1, 3)
    per = per[rng.permutation(len(per))]
    c["one-point-per-chunk"] = Case(*edge, tuple((per[:, d] * edge[1][d]).astype(np.int64) for d in range(3)))
    for n in (0, 1, 255, 256, 257, RUN - 1, RUN, RUN + 1, 2 * RUN + 3):
        c[f"n-{n}"] = Case(*cube, _uniform(rng, cube[0], n, True))
    c["read-strided-out"] = Case(*edge, _uniform(rng, edge[0], 1500, True), stride=3 * ITEMSIZE)
    c["write-array-value"] = Case(*edge, _uniform(rng, edge[0], 1500, True), write=True)
    c["write-scalar-value"] = Case(*cube, _uniform(rng, cube[0], 1500, True), write=True, stride=0)
    # the two counter forms: grids of 1, 640 and exactly BINS chunks (LDS histogram), BINS + 1 (global atomics)
    c["grid-1"] = Case((13, 11), (16, 16), _uniform(rng, (13, 11), 5000, True))
    c["grid-640"] = Case((40, 16), (1, 1), _uniform(rng, (40, 16), 5000, True))
    def ends_first(co, n):  # the first and the last counter are touched for certain
        co[0][:4] = [0, n - 1, -1, -n]
        return co

    c["grid-lds-bins"] = Case((BINS,), (1,), ends_first(_uniform(rng, (BINS,), 6000, True), BINS))
    c["grid-lds-bins-plus-1"] = Case((BINS + 1,), (1,), ends_first(_uniform(rng, (BINS + 1,), 6000, True), BINS + 1))
    c["grid-lds-bins-plus-1-write"] = Case((BINS + 1,), (1,), ends_first(_uniform(rng, (BINS + 1,), 6000), BINS + 1),
                                           write=True)
    return c


CASES = _cases()
