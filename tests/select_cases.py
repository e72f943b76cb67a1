"""Hand-built zhip_select_copy tables and an independent reference, shared by
test_select_kernel.py (the CPU hook) and test_gpu_select_kernel.py (the
kernel).  No test functions here.

A case is described plainly: a list of items, each {"a_base", "b_base",
"dims"}, a dimension ("affine", count, a0, sa, b0, sb) or ("table", count,
A[k], B[k]) with byte offsets.  build_tables() turns the description into the
raw records of include/zarrhip.h without zarr_hip.fancy.SelectTables (the
route's own builder is what the pipeline tests check).  reference_offsets()
enumerates every element with np.unravel_index (C order, the last dimension
fastest) and sums the offsets in int64 numpy: no fast division anywhere.

Every generator keeps the destinations of one case distinct, so the expected
bytes do not depend on the order of the stores, and keeps every offset a
multiple of the item size (the kernel loads and stores whole items).
"""

from collections import namedtuple

import numpy as np

from zarr_hip import _native as N

ITEMSIZES = (1, 2, 4, 8)
T = N.SELECT_TILE

Tables = namedtuple("Tables", "items table prefix n_tiles")


def item(dims, a_base=0, b_base=0) -> dict:
    return {"a_base": int(a_base), "b_base": int(b_base), "dims": list(dims)}


def build_tables(items) -> Tables:
    """(item records, shared int64 pair table, tile prefix, n_tiles)."""
    rec = np.zeros(len(items), N.SELECT_ITEM_DT)
    pairs = []
    n_pairs = 0
    tiles = []
    for i, it in enumerate(items):
        dims = it["dims"]
        assert 1 <= len(dims) <= N.MAX_DIMS
        total = 1
        for d, dim in enumerate(dims):
            kind, count = dim[0], int(dim[1])
            assert count >= 1
            D = rec[i]["dims"][d]
            D["count"] = count
            D["div"] = N.fdiv(count)
            if kind == "affine":
                D["a0"], D["sa"], D["b0"], D["sb"] = (int(x) for x in dim[2:6])
            else:
                assert kind == "table"
                A, B = np.asarray(dim[2], np.int64), np.asarray(dim[3], np.int64)
                assert A.shape == B.shape == (count,)
                D["table"] = 1
                D["table_off"] = n_pairs
                pairs.append(np.stack([A, B], axis=1))
                n_pairs += count
            total *= count
        assert total < 1 << 31
        rec[i]["a_base"], rec[i]["b_base"] = it["a_base"], it["b_base"]
        rec[i]["ndim"], rec[i]["total"] = len(dims), total
        tiles.append(-(-total // T))
    table = np.ascontiguousarray(np.concatenate(pairs)) if pairs else np.zeros((1, 2), np.int64)
    prefix = np.zeros(len(items) + 1, np.int64)
    np.cumsum(tiles, out=prefix[1:])
    assert prefix[-1] < 1 << 31
    return Tables(rec, table, prefix.astype(np.uint32), int(prefix[-1]))


def reference_offsets(it) -> tuple:
    """(a_offset, b_offset) int64 arrays of one item's elements in element order."""
    counts = tuple(int(d[1]) for d in it["dims"])
    total = int(np.prod(counts, dtype=np.int64))
    ks = np.unravel_index(np.arange(total, dtype=np.int64), counts)
    ao = np.full(total, it["a_base"], np.int64)
    bo = np.full(total, it["b_base"], np.int64)
    for dim, k in zip(it["dims"], ks):
        if dim[0] == "affine":
            a0, sa, b0, sb = (np.int64(x) for x in dim[2:6])
            ao += a0 + k * sa
            bo += b0 + k * sb
        else:
            ao += np.asarray(dim[2], np.int64)[k]
            bo += np.asarray(dim[3], np.int64)[k]
    return ao, bo


class Case:
    """Items plus the two buffers they run on.  a_alloc / b_alloc: bytes of the
    real allocations; a and b are passed `ptr_off` bytes into them with the
    declared sizes a_size / b_size (by default the rest of the allocation).
    fenced: some elements lie outside the declared sizes (never outside the
    allocations): the kernel skips exactly those, the hook reports
    ZHIP_E_BOUNDS."""

    def __init__(self, name, itemsize, items, a_alloc, b_alloc, ptr_off=0, a_size=None, b_size=None, fenced=False,
                 seed=0):
        self.name, self.itemsize, self.items = name, int(itemsize), items
        self.a_alloc, self.b_alloc, self.ptr_off = int(a_alloc), int(b_alloc), int(ptr_off)
        self.a_size = self.a_alloc - self.ptr_off if a_size is None else int(a_size)
        self.b_size = self.b_alloc - self.ptr_off if b_size is None else int(b_size)
        self.fenced = fenced
        self.seed = seed
        assert self.ptr_off % 8 == 0

    def tables(self) -> Tables:
        return build_tables(self.items)

    def source(self) -> np.ndarray:
        """The bytes of the whole a allocation."""
        return np.random.default_rng(1000 + self.seed).integers(0, 256, self.a_alloc, dtype=np.uint8)

    def sentinel(self) -> np.ndarray:
        """The bytes the whole b allocation holds before the copy."""
        return sentinel(self.b_alloc)

    def expected(self, a: np.ndarray, b0: np.ndarray) -> np.ndarray:
        """b after the copy: b[bo] = a[ao] over byte views, for the elements
        inside the declared sizes; every offset inside the allocations, the
        kept destinations distinct, all of it checked here."""
        b = b0.copy()
        isz = self.itemsize
        lane = np.arange(isz, dtype=np.int64)
        seen = []
        skipped = 0
        for it in self.items:
            ao, bo = reference_offsets(it)
            assert not (ao % isz).any() and not (bo % isz).any(), self.name
            assert ao.min() + self.ptr_off >= 0 and ao.max() + self.ptr_off + isz <= self.a_alloc, self.name
            assert bo.min() + self.ptr_off >= 0 and bo.max() + self.ptr_off + isz <= self.b_alloc, self.name
            inside = (ao >= 0) & (bo >= 0) & (ao + isz <= self.a_size) & (bo + isz <= self.b_size)
            skipped += int((~inside).sum())
            ao, bo = ao[inside] + self.ptr_off, bo[inside] + self.ptr_off
            seen.append(bo)
            b[bo[:, None] + lane] = a[ao[:, None] + lane]
        allb = np.concatenate(seen)
        assert np.unique(allb).size == allb.size, f"{self.name}: destinations repeat"
        assert (skipped > 0) == self.fenced, self.name
        return b


def sentinel(n: int, at: int = 0) -> np.ndarray:
    i = np.arange(at, at + n, dtype=np.int64)
    return ((i * 131 + (i >> 8) * 7 + 89) & 0xFF).astype(np.uint8)


# ------------------------------------------------------------------ layouts
class _Layout:
    """A padded array with its axes in a shuffled memory order: per axis an
    extent and a byte stride; pick() hands an affine walk or a table of
    distinct indices along one axis."""

    def __init__(self, rng, counts, isz, pad=2, step_max=2):
        self.rng, self.isz = rng, isz
        self.step = [int(rng.integers(1, step_max + 1)) if c > 1 else 1 for c in counts]
        self.start = [int(rng.integers(0, pad + 1)) for _ in counts]
        self.extent = [s + (c - 1) * st + 1 + int(rng.integers(0, pad + 1))
                       for c, s, st in zip(counts, self.start, self.step)]
        order = rng.permutation(len(counts))
        self.stride = [0] * len(counts)
        acc = isz
        for ax in order:
            self.stride[ax] = acc
            acc *= self.extent[ax]
        self.nbytes = acc

    def affine(self, ax, count, reverse=False):
        s, st, sd = self.start[ax], self.step[ax], self.stride[ax]
        if reverse:
            return (s + (count - 1) * st) * sd, -st * sd
        return s * sd, st * sd

    def table(self, ax, count):
        idx = self.rng.permutation(self.extent[ax])[:count]
        assert idx.size == count
        return idx.astype(np.int64) * self.stride[ax]


def _product_case(name, isz, counts, tables=(), reverse=(), seed=0, broadcast=False, bias=0):
    """One item over `counts`: dims in `tables` are table dimensions (both
    sides), the rest affine; dims in `reverse` walk both sides backwards from
    the far end; broadcast: every a offset 0 (a scalar value); bias: table
    entries lowered by it, the bases raised by it."""
    rng = np.random.default_rng(seed)
    small = len(counts) <= 4  # many dimensions: tighter padding, unit steps (the buffers stay a few MiB)
    la, lb = (_Layout(rng, counts, isz, pad=2 if small else 1, step_max=2 if small else 1) for _ in range(2))
    dims = []
    for ax, c in enumerate(counts):
        if ax in tables:
            A, B = la.table(ax, c), lb.table(ax, c)
            if broadcast:
                A = np.zeros(c, np.int64)
            dims.append(("table", c, A - bias, B - 2 * bias))
        else:
            a0, sa = la.affine(ax, c, ax in reverse)
            b0, sb = lb.affine(ax, c, ax in reverse)
            if broadcast:
                a0 = sa = 0
            dims.append(("affine", c, a0, sa, b0, sb))
    nt = len(tables)
    return Case(name, isz, [item(dims, bias * nt, 2 * bias * nt)], la.nbytes, lb.nbytes, seed=seed)


COUNTS8 = (3, 1, 5, 2, 7, 1, 3, 11)
DIVISORS = (1, 2, 3, 7, 255, 256, 257, 641, 1023, 1025, 4097, 65537)
TILE_TOTALS = (1, 255, 256, 257, 1000, T - 1, T, T + 1, 2 * T, 3 * T + 5, 1)


def case_ndim(n, isz) -> Case:
    """n product dimensions, all affine: the trailing n of COUNTS8."""
    return _product_case(f"ndim{n}", isz, COUNTS8[8 - n:], seed=10 + n)


TABLE_PLACES = {"innermost": (3,), "outermost": (0,), "middle": (2,), "two": (1, 3)}


def case_table_at(where, isz) -> Case:
    """Four dimensions (9, 6, 7, 5), two tiles; the table dimension(s) where named."""
    return _product_case(f"table-{where}", isz, (9, 6, 7, 5), tables=TABLE_PLACES[where], seed=20 + len(where))


def case_divisor(c, isz) -> Case:
    """(outer, c): the division by the inner count c over three tiles and a
    tail, at least two outer rows."""
    outer = max(2, -(-(3 * T + 17) // c))
    return _product_case(f"div{c}", isz, (outer, c), seed=30 + c % 97)


def _regions_case(name, isz, totals, seed) -> Case:
    """One item per total, each with its own region of a and of b: even items
    an affine walk (b at every second slot), odd items a table of shuffled
    slots."""
    rng = np.random.default_rng(seed)
    items = []
    a_at = b_at = 0
    for i, n in enumerate(totals):
        if i % 2 == 0:
            dims = [("affine", n, 0, isz, 0, 2 * isz)]
        else:
            dims = [("table", n, rng.permutation(n).astype(np.int64) * isz,
                     rng.permutation(2 * n)[:n].astype(np.int64) * isz)]
        items.append(item(dims, a_at, b_at))
        a_at += n * isz
        b_at += 2 * n * isz + isz  # one untouched slot between neighbours
    return Case(name, isz, items, a_at, b_at, seed=seed)


def case_tiles(isz) -> Case:
    return _regions_case("tile-totals", isz, TILE_TOTALS, 40)


def case_single_elements(n_items, isz) -> Case:
    """n_items items of one element each (one tile per item), sources and
    destinations shuffled: the prefix search alone decides which element a
    workgroup copies."""
    rng = np.random.default_rng(50 + n_items)
    slots = 2 * n_items + 3
    src, dst = rng.permutation(slots)[:n_items], rng.permutation(slots)[:n_items]
    items = [item([("affine", 1, 0, 0, 0, 0)], int(s) * isz, int(d) * isz) for s, d in zip(src, dst)]
    return Case(f"items{n_items}", isz, items, slots * isz, slots * isz, seed=n_items)


def case_many_tiles(isz) -> Case:
    """One item of 2**20 + 3 elements, 1025 tiles: a read backwards, b shifted."""
    n = (1 << 20) + 3
    dims = [("affine", n, (n - 1) * isz, -isz, 3 * isz, isz)]
    return Case("tiles1025", isz, [item(dims)], n * isz, (n + 5) * isz, seed=60)


def case_broadcast(isz) -> Case:
    """sa = 0 everywhere: one scalar value to 37 x 61 destinations."""
    return _product_case("broadcast", isz, (37, 61), seed=70, broadcast=True)


def case_negative_strides(isz) -> Case:
    """sa < 0 and sb < 0 on both dimensions, a0 / b0 at the far end."""
    return _product_case("negative-strides", isz, (41, 53), reverse=(0, 1), seed=71)


def case_negative_tables(isz) -> Case:
    """Negative table entries; the bases bring every sum back inside."""
    return _product_case("negative-tables", isz, (41, 53), tables=(0, 1), seed=72, bias=1 << 40)


FENCE_PTR = 4096


def case_fence(side, isz) -> Case:
    """The second fence on one side (`a` or `b`): pointers 4096 bytes into
    allocations that reach 4096 bytes past the declared sizes.  The edge
    elements, on `side` only (the other side stays well inside): one item
    before the pointer, the pointer's own allocation start, the last item that
    ends at the declared size (copied), the next aligned offset (skipped), the
    allocation's last item (skipped); around them 200 inside elements.  Two
    dimensions, so the edge offsets also pass through the division."""
    rng = np.random.default_rng(80 + isz + (side == "b"))
    size = 1 << 16
    alloc = FENCE_PTR + size + 4096
    inside = rng.permutation(size // isz - 2)[:200].astype(np.int64) * isz
    edge = np.array([-isz, -FENCE_PTR, size - isz, size, size + 4096 - isz], np.int64)
    E = np.concatenate([inside[:100], edge, inside[100:]])
    n = E.size
    plain = (rng.permutation(size // (2 * isz) - 8)[:n].astype(np.int64) + 4) * 2 * isz  # even slots; the inner dim adds one
    A, B = (E, plain) if side == "a" else (plain, E)
    if side == "a":
        dims = [("table", n, A, B), ("affine", 2, 0, 0, 0, isz)]   # each source feeds two destinations
    else:
        dims = [("affine", 1, 0, 0, 0, 0), ("table", n, A, B)]     # destinations stay distinct: divided by n only
    return Case(f"fence-{side}", isz, [item(dims)], alloc, alloc, ptr_off=FENCE_PTR, a_size=size, b_size=size,
                fenced=True, seed=81)


def _bind(fn, *args):
    return lambda isz: fn(*args, isz)


# name -> generator(itemsize): every case that fits in host memory and runs
# through the hook in a second or two; both test files run all of them
HOST_CASES: dict = {}
for _n in range(1, 9):
    HOST_CASES[f"ndim{_n}"] = _bind(case_ndim, _n)
for _w in TABLE_PLACES:
    HOST_CASES[f"table-{_w}"] = _bind(case_table_at, _w)
for _c in DIVISORS:
    HOST_CASES[f"div{_c}"] = _bind(case_divisor, _c)
HOST_CASES["tile-totals"] = case_tiles
for _n in (1, 2, 3, 4097):
    HOST_CASES[f"items{_n}"] = _bind(case_single_elements, _n)
HOST_CASES["tiles1025"] = case_many_tiles
HOST_CASES["broadcast"] = case_broadcast
HOST_CASES["negative-strides"] = case_negative_strides
HOST_CASES["negative-tables"] = case_negative_tables

# the fenced cases: the kernel skips, the hook reports ZHIP_E_BOUNDS
FENCE_CASES = {"fence-a": _bind(case_fence, "a"), "fence-b": _bind(case_fence, "b")}
