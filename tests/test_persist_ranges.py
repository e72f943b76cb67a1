"""The condition that keeps tests/test_gpu_persistent_ranges.py honest, on the
CPU: for every row of tests/persist_cases.py and every grid cap G the row runs
under, the numpy restatement of the partition tiles the units exactly, the
launch SHOWS the situations the row is in the table for (runs of several
units, ranges of several runs, chunks split between workgroups, the dropped
chunk inside a range, ...), and the planner gives the row the layout flags
(fast / rows / tile) and the units per chunk its kernel name rests on.  A row
or a cap that shows nothing is an error of the table.  No GPU needed."""

import numpy as np
import pytest

import persist_cases as PC
import tile_cases as TC
from zarr_hip import _native as N
from zarr_hip import codecs as C
from zarr_hip import planner as P
from zarr_hip.spec import ArraySpec

CRCJ = {"name": "crc32c"}
IDS = [r.id for r in PC.ROWS]


def test_model_on_a_hand_worked_case():
    """7 chunks of 3 units under 4 workgroups: 21 = 4 * 5 + 1."""
    assert PC.ranges(21, 4) == [(0, 6), (6, 11), (11, 16), (16, 21)]
    assert PC.runs(21, 3, 4) == [(0, 0, 0, 3), (0, 1, 0, 3),                 # two whole chunks
                                 (1, 2, 0, 3), (1, 3, 1, 2),                 # chunk 3's first two units ...
                                 (2, 3, 0, 1), (2, 4, 0, 3), (2, 5, 2, 1),   # ... its last; chunk 5's first
                                 (3, 5, 0, 2), (3, 6, 0, 3)]
    assert PC.features(21, 3, 4, dropped=1) == {PC.LONG_RUN, PC.THREE_RUNS, PC.SPLIT_LONG, PC.UNEVEN}
    assert PC.features(21, 3, 3, dropped=1) >= {PC.DROP_INSIDE}      # [0, 7) holds chunk 1 = [3, 6)
    assert PC.features(21, 3, 21, dropped=1) == set()                # the control
    assert PC.nseg_of(71610) == 3 and PC.nseg_of(32768) == 1 and PC.nseg_of(32769) == 2
    assert PC.nseg_of(32753) == 1 and PC.nseg_of(65537) == 3         # the end rounds up to 16 bytes first


@pytest.mark.parametrize("rid", IDS)
def test_ranges_tile_the_units(rid):
    row = PC.BY_ID[rid]
    nseg, n = PC.units_per_chunk(row), PC.n_chunks(row)
    n_units = n * nseg
    gs = PC.row_caps(row)
    assert gs[-1] == n_units and len(gs) >= 4
    for G in gs:
        rg = PC.ranges(n_units, G)
        assert len(rg) == G and rg[0][0] == 0 and rg[-1][1] == n_units
        assert all(a[1] == b[0] for a, b in zip(rg, rg[1:]))
        lens = [b - a for a, b in rg]
        assert min(lens) >= 1 and max(lens) - min(lens) <= 1
        assert lens == sorted(lens, reverse=True)                    # the longer ranges first
        rs = PC.runs(n_units, nseg, G)
        assert sum(r.len for r in rs) == n_units
        for c in range(n):                                           # every unit of every chunk, once
            assert sum(r.len for r in rs if r.chunk == c) == nseg
        assert all(0 <= r.sidx < nseg and r.sidx + r.len <= nseg for r in rs)


@pytest.mark.parametrize("rid", IDS)
def test_every_cap_shows_what_the_row_claims(rid):
    row = PC.BY_ID[rid]
    nseg, n = PC.units_per_chunk(row), PC.n_chunks(row)
    n_units = n * nseg
    assert nseg >= 3 and 0 < PC.DROPPED < n - 1                      # an interior chunk
    shown = {}
    for G in PC.row_caps(row):
        shown[G] = PC.features(n_units, nseg, G, PC.DROPPED)
        assert shown[G] <= set(PC.FEATURES)
        if G == n_units:
            assert not shown[G], "the control shows a feature"
        else:
            assert shown[G], f"cap {G} shows nothing: an error of the table"
    union = set().union(*shown.values())
    assert set(row.claims) <= union, sorted(set(row.claims) - union)
    if nseg > 32:
        assert PC.WHOLE_BIG in shown[1] and PC.SPLIT_BIG in union
    # the sweep runs under caps that show runs of several units and split chunks
    sw = PC.sweep_caps(row)
    if row.crc:
        assert sw and {PC.LONG_RUN, PC.SPLIT_LONG} <= set().union(*(shown[G] for G in sw)), sw
    # the write: five chunks along the last dim
    if row.encode is not None:
        wu = PC.WRITE_CHUNKS * nseg
        wshown = {G: PC.features(wu, nseg, G) for G in PC.write_caps(row)}
        assert all(v for G, v in wshown.items() if G != wu) and not wshown[wu]
        assert {PC.LONG_RUN, PC.THREE_RUNS, PC.SPLIT_LONG} <= set().union(*wshown.values())


def _chain(row):
    codecs = ([{"name": "transpose", "configuration": {"order": list(row.order)}}] if row.order else []) + \
        [row.endian] + ([CRCJ] if row.crc else [])
    spec = ArraySpec(tuple(row.chunk), np.dtype(row.dtype), row.fill)
    return P.analyze_chain(C.parse_codecs(codecs), spec), spec


@pytest.mark.parametrize("rid", IDS)
def test_planner_gives_the_rows_layout(rid):
    """A whole read of the row's array (sharded rows: of its inner chunks, as
    the expansion plans them): fast / rows / tile as the table says -- neither
    rows nor tile is the generic k_decode, rows the row kernels (k_decode_rows
    under the persist bit), tile without a tile4 or group form k_decode_tile --
    and the plan's units per chunk equal nseg_of."""
    row = PC.BY_ID[rid]
    chain, spec = _chain(row)
    array = PC.array_shape(row)
    it = spec.dtype.itemsize
    ostr = TC.c_strides(array, it)
    grid = [a // c for a, c in zip(array, row.chunk)]
    blob = int(np.prod(row.chunk)) * it + (4 if row.crc else 0)
    items = []
    for i, ix in enumerate(np.ndindex(*grid)):
        lo = [c * k for c, k in zip(ix, row.chunk)]
        items.append((i * 2 * blob, blob, i == PC.DROPPED, tuple(slice(0, k, 1) for k in row.chunk),
                      tuple(slice(o, o + k, 1) for o, k in zip(lo, row.chunk))))
    assert len(items) == PC.n_chunks(row)
    t = P.plan_decode(chain, spec, items, ostr, 0, ())
    assert (bool(t.fast), bool(t.rows), bool(t.tile)) == (row.fast, row.rows, row.decode == PC.K_TILE)
    assert {PC.K_DEC: not t.rows and not t.tile, PC.K_ROWS: t.rows, PC.K_TILE: t.tile}[row.decode]
    plan = N.Plan(t.layout, upload=False)
    if row.decode == PC.K_TILE:
        kf = plan.kernel_flags
        assert kf & N.PK_TILE and not kf & (N.PK_TILE4 | N.PK_TILEG)
    else:
        assert plan.units_per_chunk == PC.units_per_chunk(row) == PC.nseg_of(int(t.layout.nbytes))
    if row.encode is not None:                                       # the write's five chunks along the last dim
        wshape = tuple(row.chunk[:-1]) + (PC.WRITE_CHUNKS * row.chunk[-1],)
        enc = [(i * 2 * blob, tuple(slice(0, k, 1) for k in row.chunk), (0,) * (len(wshape) - 1) + (i * row.chunk[-1],))
               for i in range(PC.WRITE_CHUNKS)]
        e = P.plan_encode(chain, spec, enc, TC.c_strides(wshape, it), 0)
        assert not e.tile and not e.tile_prefix and bool(e.rows) == row.rows
