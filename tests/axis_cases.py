"""The named 1-axis cases of the device-planned orthogonal axes (zhip_axis_last
/ zhip_axis_count / zhip_axis_fill, include/zarrhip.h), shared by
test_axis_plan.py (the CPU hook against the host route's tables) and
test_gpu_axis_kernel.py (the kernels against the hook).  Not a test module."""

from dataclasses import dataclass

import numpy as np

from zarr_hip import _native as N
from zarr_hip import axes as A

ITEMSIZE = 4
INNER = 5               # elements of a slot behind one step along the axis
RUN = N.AXIS_RUN
BINS = N.AXIS_LDS_BINS


@dataclass
class Case:
    length: int
    chunk: int
    x: np.ndarray           # int64 indices
    write: bool = False
    stride: int = ITEMSIZE  # out stride (read) / value stride (write; 0: a scalar value)
    keep_last: bool = False
    err_bit: int = 1
    err: int = 0            # the error word the case must leave
    table_off: int = 0      # the axis' first pair in a table of table_off + n pairs

    @property
    def n(self) -> int:
        return int(self.x.size)

    @property
    def grid(self) -> int:
        return -(-self.length // self.chunk)

    @property
    def slot_stride(self) -> int:
        return ITEMSIZE * INNER

    @property
    def table_pairs(self) -> int:
        return self.table_off + self.n

    def geom(self) -> np.ndarray:
        return A.axis_geom(self.length, self.chunk, self.err_bit, self.slot_stride, self.stride, self.table_off,
                           self.write)

    def wrapped(self) -> np.ndarray:
        return np.where(self.x < 0, self.x + self.length, self.x)


def run_hook(case: Case):
    """zhip_emulate_axis: (counts, lo, hi, error word, first, cursor, table, last).
    lo / hi are the decoded bounds (lo = chunk - 1 - the lo word)."""
    x = np.ascontiguousarray(case.x, dtype=np.int64)
    g = case.geom()
    G = case.grid
    counts, low, hi, first, cursor = (np.full(G, 0xDEAD, np.uint32) for _ in range(5))
    err = np.full(1, 0xDEAD, np.uint32)
    last = np.full(case.length, 0xDEAD, np.uint32)
    table = np.full((max(case.table_pairs, 1), 2), -7, np.int64)
    N.check(N.lib().zhip_emulate_axis(g.ctypes.data, x.ctypes.data, case.n, int(case.keep_last), last.ctypes.data,
                                      counts.ctypes.data, low.ctypes.data, hi.ctypes.data, err.ctypes.data,
                                      first.ctypes.data, cursor.ctypes.data, table.ctypes.data, case.table_pairs),
            "zhip_emulate_axis")
    lo = case.chunk - 1 - low.astype(np.int64)
    return counts, lo, hi.astype(np.int64), int(err[0]), first, cursor, table, last


def chunk_pairs(table: np.ndarray, table_off: int, first: np.ndarray, counts: np.ndarray) -> dict:
    """{chunk: its pairs, sorted} -- the order inside a chunk's range is unspecified."""
    out = {}
    for c in np.nonzero(counts)[0]:
        at = table_off + int(first[c])
        t = table[at:at + int(counts[c])]
        out[int(c)] = t[np.lexsort((t[:, 1], t[:, 0]))]
    return out


def _cases() -> dict:
    rng = np.random.default_rng(31)
    c: dict = {}

    def uni(L, n, negative=True):
        return rng.integers(-L if negative else 0, L, n).astype(np.int64)

    # chunk lengths 1, 3, 7, 16 with a non-dividing last chunk; one chunk; the LDS threshold
    for L, C in ((300, 1), (10, 3), (50, 7), (100, 16), (13, 16)):
        c[f"L{L}-C{C}"] = Case(L, C, uni(L, 700))
        c[f"L{L}-C{C}-keep-last-write"] = Case(L, C, uni(L, 700), write=True, keep_last=True)

    def ends_first(x, L):  # the first and the last counter are touched for certain
        x[:4] = [0, L - 1, -1, -L]
        return x

    for L in (BINS, BINS + 1):
        c[f"grid-{L}"] = Case(L, 1, ends_first(uni(L, 6000), L))
        c[f"grid-{L}-keep-last-write"] = Case(L, 1, ends_first(uni(L, 6000), L), write=True, keep_last=True)
    c["grid-past-lds-C3"] = Case(3 * BINS + 2, 3, ends_first(uni(3 * BINS + 2, 5000), 3 * BINS + 2), keep_last=True)
    # n: none, one, around a workgroup's 256 lanes, around the run, several runs
    for n in (0, 1, 255, 256, 257, RUN - 1, RUN, RUN + 1, 3 * RUN + 3):
        c[f"n-{n}"] = Case(1000, 16, uni(1000, n))
        c[f"n-{n}-keep-last"] = Case(1000, 16, uni(1000, n), write=True, keep_last=True)
    # the ends of the valid range, and one step past them
    L = 50
    c["ends-valid"] = Case(L, 7, np.array([-L, L - 1, 0, -1, -L, L - 1], np.int64))
    c["oob-L"] = Case(L, 7, np.array([L], np.int64), err_bit=4, err=4)
    c["oob-minus-L-1"] = Case(L, 7, np.array([-L - 1], np.int64), err_bit=2, err=2)
    bad = uni(L, 600)
    bad[[5, 300, 599]] = [L, -L - 1, 1 << 40]
    c["oob-among-valid"] = Case(L, 7, bad, err_bit=8, err=8)
    c["oob-among-valid-keep-last"] = Case(L, 7, bad.copy(), write=True, keep_last=True, err_bit=1, err=1)
    # orders
    L = 5000
    perm = rng.permutation(L)[:4500].astype(np.int64)
    c["sorted"] = Case(L, 16, np.sort(perm))
    c["decreasing"] = Case(L, 16, np.sort(perm)[::-1].copy())
    c["unsorted"] = Case(L, 16, perm.copy())
    # repeats, on an otherwise distinct list, read (every occurrence has a pair) and keep-last
    def rep(**kw):
        x = perm.copy()
        for a, b in kw["same"]:
            x[b] = x[a]
        return x

    reps = {
        "one-wave": [(10, 40)],
        "one-workgroup": [(5, 1500)],
        "other-workgroups": [(7, 7 + RUN + 100), (7, 7 + 2 * RUN + 1)],
    }
    for name, same in reps.items():
        c[f"repeat-{name}"] = Case(L, 16, rep(same=same))
        c[f"repeat-{name}-keep-last"] = Case(L, 16, rep(same=same), write=True, keep_last=True)
    x = perm.copy()
    x[3000] = x[20] - L  # the negative and the non-negative spelling of one element
    c["repeat-two-spellings"] = Case(L, 16, x)
    c["repeat-two-spellings-keep-last"] = Case(L, 16, x.copy(), write=True, keep_last=True)
    c["all-equal"] = Case(L, 16, np.full(600, 37, np.int64))
    c["all-equal-keep-last"] = Case(L, 16, np.full(600, 37, np.int64), write=True, keep_last=True)
    c["all-equal-keep-last-read"] = Case(L, 16, np.full(3 * RUN, -1, np.int64), keep_last=True)
    # both pair orders and the scalar write; a strided out; an axis behind others in the table
    c["read-strided-out"] = Case(50, 7, uni(50, 1500), stride=3 * ITEMSIZE)
    c["write-array-value"] = Case(50, 7, uni(50, 1500), write=True, keep_last=True)
    c["write-scalar-value"] = Case(100, 16, uni(100, 1500), write=True, stride=0)
    c["table-offset"] = Case(100, 16, uni(100, 1500), table_off=77)
    return c


CASES = _cases()
