"""Selection -> per-chunk projections for regular chunk grids (host planner input).

Semantics follow the reference's BasicIndexer (src/zarr/core/indexing.py:571-621),
IntDimIndexer (365-385) and SliceDimIndexer (388-468), with boundary chunks
stored at full size (FixedDimension.data_size, src/zarr/core/chunk_grids.py:119-130).
The projections are produced per dimension as numpy arrays and combined by a
cartesian product, so planning 10^4-10^5 chunks stays vectorised.
"""

from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np


def _ceildiv(a, b):
    return -(-a // b)


@dataclass
class DimProjection:
    """Projections of one selection item onto one chunked dimension."""

    chunk_ix: np.ndarray   # int64[k]
    sel_start: np.ndarray  # int64[k]   first selected index inside the chunk
    sel_count: np.ndarray  # int64[k]
    step: int
    out_start: np.ndarray  # int64[k]   position along the out dim (0 for int selections)
    complete: np.ndarray   # bool[k]
    dropped: bool          # integer selection: the dim is absent from out
    nitems: int


def normalize_selection(selection, shape: tuple[int, ...]) -> tuple:
    """replace_ellipsis (indexing.py:458-496) + integer normalisation."""
    if not isinstance(selection, tuple):
        selection = (selection,)
    sel = list(selection)
    n_ell = sum(1 for s in sel if s is Ellipsis)
    if n_ell > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if n_ell == 1:
        i = sel.index(Ellipsis)
        fill = len(shape) - (len(sel) - 1)
        sel = sel[:i] + [slice(None)] * max(fill, 0) + sel[i + 1:]
    if len(sel) > len(shape):
        raise IndexError(f"too many indices for array; expected {len(shape)}, got {len(sel)}")
    sel += [slice(None)] * (len(shape) - len(sel))
    out = []
    for s, n in zip(sel, shape):
        if isinstance(s, (int, np.integer)):
            i = int(s)
            if i < 0:
                i += n
            if not 0 <= i < n:
                raise IndexError(f"index out of bounds for dimension with length {n}")
            out.append(i)
        elif isinstance(s, slice):
            if s.step == 0:  # slice.indices raises first (indexing.py:408)
                raise ValueError("slice step cannot be zero")
            if s.step is not None and s.step < 1:
                raise IndexError("only slices with step >= 1 are supported.")
            out.append(slice(*s.indices(n)))
        else:
            raise IndexError(
                "unsupported selection item for basic indexing; expected integer or slice, "
                f"got {type(s)!r}")
    return tuple(out)


def project_dim(sel, dim_len: int, chunk_len: int) -> DimProjection:
    if isinstance(sel, int):
        ix = sel // chunk_len
        data_size = min(chunk_len, dim_len - ix * chunk_len)
        a = np.array([ix], np.int64)
        return DimProjection(a, np.array([sel - ix * chunk_len], np.int64), np.ones(1, np.int64), 1,
                             np.zeros(1, np.int64), np.array([data_size == 1]), True, 1)
    start, stop, step = sel.start, sel.stop, sel.step
    nitems = max(0, _ceildiv(stop - start, step))
    if start >= stop:
        e = np.zeros(0, np.int64)
        return DimProjection(e, e, e, step, e, np.zeros(0, bool), False, 0)
    ix_from = start // chunk_len
    ix_to = (stop - 1) // chunk_len + 1
    ix = np.arange(ix_from, ix_to, dtype=np.int64)
    off = ix * chunk_len
    clen = np.minimum(chunk_len, dim_len - off)
    limit = off + clen
    before = start < off
    rem = np.where(before, (off - start) % step, 0)
    s0 = np.where(before, np.where(rem > 0, step - rem, 0), start - off)
    out_off = np.where(before, -((start - off) // step), 0)  # ceildiv(off-start, step)
    s1 = np.where(stop > limit, clen, stop - off)
    cnt = np.maximum(0, -((s0 - s1) // step))
    complete = (s0 == 0) & (stop >= limit) & (step == 1)
    keep = cnt > 0
    return DimProjection(ix[keep], s0[keep], cnt[keep], step, out_off[keep], complete[keep],
                         False, nitems)


@dataclass
class Projections:
    """Cartesian product of per-dim projections: one row per touched chunk."""

    coords: np.ndarray      # int64[n, ndim]
    sel_start: np.ndarray   # int64[n, ndim]
    sel_count: np.ndarray   # int64[n, ndim]
    step: np.ndarray        # int64[ndim]
    out_start: np.ndarray   # int64[n, ndim]  (0 in dropped dims)
    complete: np.ndarray    # bool[n]
    dropped: tuple[bool, ...]
    out_shape: tuple[int, ...]


def basic_projections(selection, shape: tuple[int, ...], chunk_shape: tuple[int, ...]) -> Projections:
    sel = normalize_selection(selection, shape)
    dims = [project_dim(s, n, c) for s, n, c in zip(sel, shape, chunk_shape)]
    nd = len(dims)
    counts = [len(d.chunk_ix) for d in dims]
    n = int(np.prod(counts)) if counts else 1
    grids = np.indices(counts, dtype=np.int64).reshape(nd, -1) if nd else np.zeros((0, 1), np.int64)

    def take(attr):
        return np.stack([getattr(d, attr)[grids[i]] for i, d in enumerate(dims)], axis=1) \
            if nd else np.zeros((1, 0), np.int64)

    coords = take("chunk_ix")
    complete = np.all(take("complete").astype(bool), axis=1) if nd else np.ones(1, bool)
    return Projections(
        coords=coords.reshape(n, nd), sel_start=take("sel_start").reshape(n, nd),
        sel_count=take("sel_count").reshape(n, nd), step=np.array([d.step for d in dims], np.int64),
        out_start=take("out_start").reshape(n, nd), complete=complete.reshape(n),
        dropped=tuple(d.dropped for d in dims),
        out_shape=tuple(d.nitems for d in dims if not d.dropped))


def to_chunk_selection(p: Projections, i: int) -> tuple:
    """Row i as the reference's (chunk_selection, out_selection) tuples."""
    csel, osel = [], []
    for d in range(p.coords.shape[1]):
        s0 = int(p.sel_start[i, d])
        if p.dropped[d]:
            csel.append(s0)
            continue
        st = int(p.step[d])
        cnt = int(p.sel_count[i, d])
        csel.append(slice(s0, s0 + (cnt - 1) * st + 1, st))
        o = int(p.out_start[i, d])
        osel.append(slice(o, o + cnt))
    return tuple(csel), tuple(osel)


def _project_dim_lists(sel, dim_len: int, chunk_len: int):
    """project_dim as Python lists (ix, sel_start, sel_count, out_start,
    complete, step, dropped, nitems); numpy only for long dims."""
    if isinstance(sel, int):
        ix = sel // chunk_len
        return ([ix], [sel - ix * chunk_len], [1], [0], [min(chunk_len, dim_len - ix * chunk_len) == 1], 1,
                True, 1)
    start, stop, step = sel.start, sel.stop, sel.step
    nitems = max(0, -((start - stop) // step))
    if start >= stop:
        return [], [], [], [], [], step, False, 0
    ix_from, ix_to = start // chunk_len, (stop - 1) // chunk_len + 1
    if ix_to - ix_from > 256:
        d = project_dim(sel, dim_len, chunk_len)
        return (d.chunk_ix.tolist(), d.sel_start.tolist(), d.sel_count.tolist(), d.out_start.tolist(),
                d.complete.tolist(), step, False, nitems)
    ixs, s0s, cnts, oos, cps = [], [], [], [], []
    for ix in range(ix_from, ix_to):
        off = ix * chunk_len
        clen = min(chunk_len, dim_len - off)
        limit = off + clen
        if start < off:
            rem = (off - start) % step
            s0 = step - rem if rem else 0
            oo = -((start - off) // step)
        else:
            s0, oo = start - off, 0
        s1 = clen if stop > limit else stop - off
        cnt = max(0, -((s0 - s1) // step))
        if cnt > 0:
            ixs.append(ix)
            s0s.append(s0)
            cnts.append(cnt)
            oos.append(oo)
            cps.append(s0 == 0 and stop >= limit and step == 1)
    return ixs, s0s, cnts, oos, cps, step, False, nitems


def _project_dim_grid(sel, dim_len: int, g):
    """IntDimIndexer / SliceDimIndexer.__iter__ over any dimension grid
    (indexing.py:369-468 with DimensionGrid's index_to_chunk / chunk_offset /
    data_size): a VaryingDimension of a rectilinear grid (zarr_hip.grid)."""
    if isinstance(sel, int):
        ix = g.index_to_chunk(sel)
        return [ix], [sel - g.chunk_offset(ix)], [1], [0], [g.data_size(ix) == 1], 1, True, 1
    start, stop, step = sel.start, sel.stop, sel.step
    nitems = max(0, -((start - stop) // step))
    if start >= stop:
        return [], [], [], [], [], step, False, 0
    ix_from = g.index_to_chunk(start) if start > 0 else 0
    ix_to = g.index_to_chunk(stop - 1) + 1 if stop > 0 else 0
    ixs, s0s, cnts, oos, cps = [], [], [], [], []
    for ix in range(ix_from, ix_to):
        off = g.chunk_offset(ix)
        clen = g.data_size(ix)
        limit = off + clen
        if start < off:
            rem = (off - start) % step
            s0 = step - rem if rem else 0
            oo = -((start - off) // step)
        else:
            s0, oo = start - off, 0
        s1 = clen if stop > limit else stop - off
        cnt = max(0, -((s0 - s1) // step))
        if cnt > 0:
            ixs.append(ix)
            s0s.append(s0)
            cnts.append(cnt)
            oos.append(oo)
            cps.append(s0 == 0 and stop >= limit and step == 1)
    return ixs, s0s, cnts, oos, cps, step, False, nitems


def chunk_batch(selection, shape: tuple[int, ...], chunk_shape):
    """basic_projections + chunk_selections for a batch: per-dim projections,
    then their Cartesian product (C order over chunk coordinates, as
    basic_projections) built from Python lists.  Returns
    ([(coords, chunk_selection, out_selection, complete)], out_shape).
    `chunk_shape` is a regular chunk shape or a zarr_hip.grid.ChunkGrid
    (rectilinear grids: per-dim projections over the varying edges)."""
    import itertools

    from .grid import ChunkGrid, FixedDimension

    sel = normalize_selection(selection, shape)
    if isinstance(chunk_shape, ChunkGrid):
        dims = chunk_shape.dimensions
        chunk_shape = tuple(d.size if isinstance(d, FixedDimension) else d for d in dims)
    ixs, csels, osels, cps = [], [], [], []
    out_shape = []
    for s, n, c in zip(sel, shape, chunk_shape):
        if isinstance(c, int):
            ix, s0, cnt, oo, cp, st, dropped, nitems = _project_dim_lists(s, n, c)
        else:
            ix, s0, cnt, oo, cp, st, dropped, nitems = _project_dim_grid(s, n, c)
        ixs.append(ix)
        cps.append(cp)
        if dropped:
            csels.append(s0)
        else:
            out_shape.append(nitems)
            csels.append([slice(a, a + (k - 1) * st + 1, st) for a, k in zip(s0, cnt)])
            osels.append([slice(o, o + k) for o, k in zip(oo, cnt)])
    P = itertools.product
    out = list(zip(P(*ixs), P(*csels), P(*osels), map(all, P(*cps))))
    return out, tuple(out_shape)


def chunk_selections(p: Projections) -> list:
    """to_chunk_selection for every row, from Python lists (one pass)."""
    nd = p.coords.shape[1]
    ss, cc, oo = p.sel_start.tolist(), p.sel_count.tolist(), p.out_start.tolist()
    steps = p.step.tolist()
    drop = p.dropped
    out = []
    for s_row, c_row, o_row in zip(ss, cc, oo):
        csel, osel = [], []
        for d in range(nd):
            s0 = s_row[d]
            if drop[d]:
                csel.append(s0)
                continue
            st, cnt, o = steps[d], c_row[d], o_row[d]
            csel.append(slice(s0, s0 + (cnt - 1) * st + 1, st))
            osel.append(slice(o, o + cnt))
        out.append((tuple(csel), tuple(osel)))
    return out


# --- orthogonal, coordinate and mask indexers over regular grids ---------------
# Restated from the reference (src/zarr/core/indexing.py:625-1046, 1171-1373):
# the same projections in the same forms, np.ix_ meshes included, so a batch
# built here is what zarr itself hands HipCodecPipeline.read / write.

def is_integer(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def is_integer_list(x) -> bool:
    return isinstance(x, list) and len(x) > 0 and all(is_integer(i) for i in x)


def is_bool_list(x) -> bool:
    return isinstance(x, list) and len(x) > 0 and all(isinstance(i, (bool, np.bool_)) for i in x)


def is_integer_array(x, ndim: int | None = None) -> bool:
    return isinstance(x, np.ndarray) and x.dtype.kind in "ui" and (ndim is None or x.ndim == ndim)


def is_bool_array(x, ndim: int | None = None) -> bool:
    return isinstance(x, np.ndarray) and x.dtype == bool and (ndim is None or x.ndim == ndim)


def is_int_or_bool_iterable(x) -> bool:
    return is_integer_list(x) or is_integer_array(x) or is_bool_array(x) or is_bool_list(x)


def is_pure_fancy_indexing(selection, ndim: int) -> bool:
    """Only scalars and integer / boolean array-likes: Array.__getitem__ sends
    these to vindex (indexing.py:270-307)."""
    if is_bool_array(selection):
        return True
    if ndim == 1 and (is_integer_list(selection) or is_integer_array(selection) or is_bool_list(selection)):
        return True
    no_slicing = (isinstance(selection, tuple) and len(selection) == ndim
                  and not any(isinstance(e, slice) or e is Ellipsis for e in selection))
    return (no_slicing
            and all(is_integer(e) or is_integer_list(e) or is_integer_array(e) for e in selection)
            and any(is_integer_list(e) or is_integer_array(e) for e in selection))


def is_pure_orthogonal_indexing(selection, ndim: int) -> bool:
    """Array.__getitem__ sends these to oindex (indexing.py:310-330)."""
    if not ndim:
        return False
    sel = selection if isinstance(selection, tuple) else (selection,)
    if len(sel) == ndim and all(is_int_or_bool_iterable(s) for s in sel):
        return True
    return (len(sel) <= ndim and sum(is_int_or_bool_iterable(s) for s in sel) <= 1
            and all(is_int_or_bool_iterable(s) or isinstance(s, (int, slice)) for s in sel))


def replace_lists(selection) -> tuple:
    return tuple(np.asarray(s) if isinstance(s, list) else s for s in selection)


def _replace_ellipsis(selection, shape) -> tuple:
    sel = list(selection) if isinstance(selection, tuple) else [selection]
    n_ell = sum(1 for s in sel if s is Ellipsis)
    if n_ell > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if n_ell == 1:
        i = next(j for j, s in enumerate(sel) if s is Ellipsis)
        sel = sel[:i] + [slice(None)] * max(len(shape) - (len(sel) - 1), 0) + sel[i + 1:]
    if len(sel) > len(shape):
        raise IndexError(f"too many indices for array; expected {len(shape)}, got {len(sel)}")
    return tuple(sel + [slice(None)] * (len(shape) - len(sel)))


def _group_order(chunk_ix: np.ndarray, nchunks: int) -> np.ndarray:
    """A stable argsort of chunk indices.  (The reference's argsort is not
    stable, indexing.py:803, 1299: the order inside a chunk is unspecified
    there.)  Keys that fit 16 bits take numpy's radix sort."""
    key = chunk_ix.astype(np.uint16) if nchunks <= 1 << 16 else chunk_ix
    return np.argsort(key, kind="stable")


def _chunk_of(x: np.ndarray, chunk_len: int) -> np.ndarray:
    """x // chunk_len for non-negative indices (a shift for power-of-two chunks:
    the division is the bottleneck of dense integer selections, indexing.py:786-788)."""
    if chunk_len & (chunk_len - 1) == 0:
        return x >> (chunk_len.bit_length() - 1)
    return x // chunk_len


def _wrap_and_check(x: np.ndarray, dim_len: int) -> np.ndarray:
    """wraparound_indices + boundscheck_indices (indexing.py:732-741), on a copy."""
    x = np.array(x, dtype=np.intp)
    x[x < 0] += dim_len
    if np.any(x < 0) or np.any(x >= dim_len):
        raise IndexError(f"index out of bounds for dimension with length {dim_len}")
    return x


def _ix(selection, shape) -> tuple:
    """ix_ (indexing.py:854-874): np.ix_ with slices as ranges and integers as
    length-1 lists."""
    return np.ix_(*[range(*s.indices(n)) if isinstance(s, slice) else [s] if is_integer(s) else s
                    for s, n in zip(selection, shape)])


def _ortho_dim(sel, dim_len: int, chunk_len: int):
    """One dimension of an orthogonal selection: ([(chunk ix, chunk sel, out
    sel | None)], nitems, is an integer).  IntDimIndexer, SliceDimIndexer,
    IntArrayDimIndexer (increasing / decreasing / unordered) and
    BoolArrayDimIndexer (padded to the codec chunk length at a boundary
    chunk), indexing.py:365-468, 625-847."""
    nchunks = _ceildiv(dim_len, chunk_len)
    if is_integer(sel):
        i = int(sel) + (dim_len if sel < 0 else 0)
        if not 0 <= i < dim_len:
            raise IndexError(f"index out of bounds for dimension with length {dim_len}")
        return [(i // chunk_len, i % chunk_len, None)], 1, True
    if isinstance(sel, slice):
        if sel.step == 0:
            raise ValueError("slice step cannot be zero")
        if sel.step is not None and sel.step < 1:
            raise IndexError("only slices with step >= 1 are supported.")
        ix, s0, cnt, oo, _, st, _, nitems = _project_dim_lists(slice(*sel.indices(dim_len)), dim_len, chunk_len)
        return [(i, slice(a, a + (k - 1) * st + 1, st), slice(o, o + k))
                for i, a, k, o in zip(ix, s0, cnt, oo)], nitems, False
    if is_bool_array(sel):
        if sel.ndim != 1:
            raise IndexError("Boolean arrays in an orthogonal selection must be 1-dimensional only")
        if sel.shape[0] != dim_len:
            raise IndexError(f"Boolean array has the wrong length for dimension; expected {dim_len}, "
                             f"got {sel.shape[0]}")
        out, at = [], 0
        for ix in range(nchunks):
            part = sel[ix * chunk_len:(ix + 1) * chunk_len]
            n = int(np.count_nonzero(part))
            if n:
                if part.shape[0] < chunk_len:
                    part = np.concatenate([part, np.zeros(chunk_len - part.shape[0], bool)])
                out.append((ix, part, slice(at, at + n)))
            at += n
        return out, at, False
    if is_integer_array(sel):
        if sel.ndim != 1:
            raise IndexError("integer arrays in an orthogonal selection must be 1-dimensional only")
        x = _wrap_and_check(sel, dim_len)
        nitems = len(x)
        cix = _chunk_of(x, chunk_len)
        d = np.diff(x)
        if np.all(d >= 0):
            osel = None
        elif not np.any(d >= 0):
            x, osel = x[::-1], np.arange(nitems - 1, -1, -1)
        else:
            osel = _group_order(cix, nchunks)
            x = np.take(x, osel)
        counts = np.bincount(cix, minlength=nchunks)
        cum = np.cumsum(counts)
        out = []
        for ix in np.nonzero(counts)[0]:
            a, b = (0 if ix == 0 else int(cum[ix - 1])), int(cum[ix])
            out.append((int(ix), x[a:b] - ix * chunk_len, slice(a, b) if osel is None else osel[a:b]))
        return out, nitems, False
    raise IndexError("unsupported selection item for orthogonal indexing; expected integer, slice, integer array "
                     f"or Boolean array, got {type(sel)!r}")


def _is_basic(selection) -> bool:
    return all(isinstance(s, slice) or is_integer(s) for s in selection)


class OrthogonalIndexer:
    """OrthogonalIndexer (indexing.py:901-996) over a regular grid.  Iterating
    gives (chunk coords, chunk_selection, out_selection, is_complete_chunk)."""

    def __init__(self, selection, shape, chunk_shape):
        selection = replace_lists(_replace_ellipsis(selection, shape))
        self.chunk_shape = tuple(chunk_shape)
        dims = [_ortho_dim(s, n, c) for s, n, c in zip(selection, shape, chunk_shape)]
        self.dims = [d[0] for d in dims]
        self.shape = tuple(int(d[1]) for d in dims if not d[2])
        self.is_advanced = not _is_basic(selection)
        self.drop_axes = tuple(i for i, d in enumerate(dims) if d[2]) if self.is_advanced else ()

    def __iter__(self):
        for proj in itertools.product(*self.dims):
            coords = tuple(int(p[0]) for p in proj)
            csel = tuple(p[1] for p in proj)
            osel = tuple(p[2] for p in proj if p[2] is not None)
            if self.is_advanced:
                # one array dimension and no integers: numpy takes the tuple as it is;
                # otherwise the orthogonal selection becomes an np.ix_ mesh (:972-993)
                if sum(isinstance(s, np.ndarray) for s in csel) > 1 or self.drop_axes:
                    csel = _ix(csel, self.chunk_shape)
                    if not _is_basic(osel):
                        osel = _ix(osel, self.shape)
            yield coords, csel, osel, False


class CoordinateIndexer:
    """CoordinateIndexer (indexing.py:1171-1350) over a regular grid: points
    grouped by chunk; out is flat (shape), the caller reshapes to sel_shape."""

    drop_axes = ()

    def __init__(self, selection, shape, chunk_shape):
        sel = selection if isinstance(selection, tuple) else (selection,)
        sel = replace_lists(tuple(np.asarray([i], dtype=np.intp) if is_integer(i) else i for i in sel))
        if len(sel) != len(shape) or not all(is_integer_array(s) for s in sel):
            raise IndexError("invalid coordinate selection; expected one integer (coordinate) array per dimension "
                             f"of the target array, got {selection!r}")
        cdata_shape = tuple(_ceildiv(n, c) for n, c in zip(shape, chunk_shape)) or (1,)
        sel = tuple(_wrap_and_check(s, n) for s, n in zip(sel, shape))
        sel = tuple(np.broadcast_arrays(*sel))  # raises when the coordinate arrays do not match
        self.sel_shape = sel[0].shape or (1,)
        sel = tuple(s.reshape(-1) for s in sel)
        rix = np.ravel_multi_index(tuple(_chunk_of(s, c) for s, c in zip(sel, chunk_shape)), cdata_shape)
        if np.any(np.diff(rix) < 0):
            self.sel_sort = _group_order(rix, int(np.prod(cdata_shape)))
            sel = tuple(s[self.sel_sort] for s in sel)
        else:
            self.sel_sort = None
        self.selection = sel
        self.shape = sel[0].shape or (1,)
        counts = np.bincount(rix, minlength=int(np.prod(cdata_shape)))
        self.cum = np.cumsum(counts)
        self.chunk_rixs = np.nonzero(counts)[0]
        self.chunk_mixs = np.unravel_index(self.chunk_rixs, cdata_shape)
        self.chunk_shape = tuple(chunk_shape)

    def __iter__(self):
        for i, rix in enumerate(self.chunk_rixs):
            coords = tuple(int(m[i]) for m in self.chunk_mixs)
            a, b = (0 if rix == 0 else int(self.cum[rix - 1])), int(self.cum[rix])
            osel = slice(a, b) if self.sel_sort is None else self.sel_sort[a:b]
            csel = tuple(s[a:b] - co * c for s, co, c in zip(self.selection, coords, self.chunk_shape))
            yield coords, csel, osel, False


class MaskIndexer(CoordinateIndexer):
    """MaskIndexer (indexing.py:1353-1373): the mask's nonzero coordinates."""

    def __init__(self, selection, shape, chunk_shape):
        sel = replace_lists(selection if isinstance(selection, tuple) else (selection,))
        if len(sel) != 1 or not is_bool_array(sel[0]) or sel[0].shape != tuple(shape):
            raise IndexError("invalid mask selection; expected one Boolean (mask)array with the same shape as the "
                             f"target array, got {sel!r}")
        super().__init__(np.nonzero(sel[0]), shape, chunk_shape)


# --- Morton / lexicographic orders (src/zarr/core/indexing.py:1524-1643) -------

def morton_order(shape: tuple[int, ...]) -> np.ndarray:
    """Coordinates of a grid in Morton (Z) order: codes of the ceiling power-of-2
    hypercube decoded (bit-interleaving over the dims that still have bits) and
    filtered to the grid, as _morton_order does (indexing.py:1578-1630)."""
    n_total = int(np.prod(shape)) if shape else 1
    nd = len(shape)
    if n_total == 0:
        return np.zeros((0, nd), np.int64)
    bits = [(c - 1).bit_length() for c in shape]
    total = sum(bits)
    z = np.arange(1 << total, dtype=np.int64)
    out = np.zeros((len(z), nd), np.int64)
    ib = 0
    for cb in range(max(bits) if bits else 0):
        for d in range(nd):
            if cb < bits[d]:
                out[:, d] |= ((z >> ib) & 1) << cb
                ib += 1
    keep = np.all(out < np.array(shape, np.int64), axis=1)
    return out[keep]


def lexicographic_order(shape: tuple[int, ...]) -> np.ndarray:
    if not shape:
        return np.zeros((1, 0), np.int64)
    return np.indices(shape, dtype=np.int64).reshape(len(shape), -1).T


def colexicographic_order(shape: tuple[int, ...]) -> np.ndarray:
    return lexicographic_order(tuple(shape[::-1]))[:, ::-1]


def subchunk_order(shape: tuple[int, ...], order: str) -> np.ndarray:
    """ShardingCodec._subchunk_order_iter (sharding.py:1090-1107)."""
    if order == "morton":
        return morton_order(shape)
    if order in ("lexicographic", "unordered"):
        return lexicographic_order(shape)
    if order == "colexicographic":
        return colexicographic_order(shape)
    raise ValueError(f"Unrecognized subchunk write order: {order!r}.")


def iter_coords(shape):
    return itertools.product(*(range(s) for s in shape))
