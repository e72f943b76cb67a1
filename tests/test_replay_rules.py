"""The conditions that keep tests/test_gpu_encode_replay.py honest, on the CPU:
for every row of tests/replay_cases.py the planner and the plan choose the
family the row's kernel name rests on, and the phases are such that a replay
that skipped work, kept a stale arrival word, a stale non-empty bit or a stale
flag cannot produce the expected bytes and flags.  No GPU needed."""

import numpy as np
import pytest

import replay_cases as RC
import tile_cases as TC
from zarr_hip import _native as N
from zarr_hip import codecs as C
from zarr_hip import planner as P
from zarr_hip.spec import ArraySpec

IDS = [r.id for r in RC.ROWS]


def _plan(row):
    dt = np.dtype(row.dtype)
    spec = ArraySpec(tuple(row.chunk), dt, RC.fill_of(row))
    chain = P.analyze_chain(C.parse_codecs(RC.codecs(row)), spec)
    offs, _ = RC.slots(row)
    items = [(offs[i], tuple(slice(0, k, 1) for k in n), list(lo)) for i, (_, lo, n) in enumerate(RC.boxes(row))]
    return P.plan_encode(chain, spec, items, TC.c_strides(row.shape, dt.itemsize), 0)


def test_every_protocol_has_a_row():
    """The protocols of the table's docstring, each with the kernel its rows name."""
    by = {}
    for r in RC.ROWS:
        by.setdefault(r.kernel, set()).add(r.proto)
    assert set(by) == {RC.K, RC.KQ, RC.KIL, RC.KP, RC.E2, RC.E4, RC.EG, RC.EGEN}  # the eight encode kernels
    assert {p for p in RC.PROTOCOLS if "counted ticket" in p or "several chunks" in p or "edge" in p} <= by[RC.K]
    assert {"k_encode_il, one half", "k_encode_il, two-level word", "k_encode_il, ragged head, S = 32"} <= by[RC.KIL]
    assert {"k_encode_pair, pair word", "k_encode_pair, OR path"} <= by[RC.KP]
    assert {"k_encode_tileg, one-word arrival", "k_encode_tileg, two-level arrival"} <= by[RC.EG]
    assert "k_encode_tile, prefix boxes" in by[RC.EGEN] and "k_encode_tile2, third word" in by[RC.E2]
    assert set(RC.TWO_LAUNCH) <= set(RC.BY_ID)
    assert {RC.BY_ID[i].kernel for i in RC.TWO_LAUNCH} == {RC.KIL, RC.KP, RC.EG, RC.K}
    assert RC.BY_ID["enc_pair_3r"].proto == "k_encode_pair, OR path"


@pytest.mark.parametrize("rid", IDS)
def test_plan_chooses_the_rows_family(rid):
    """plan_encode's rows / tile / tile_prefix, the plan's kernel flags and
    units per chunk, and the arrivals per chunk are those the row's kernel and
    protocol need (launch_encode's rules, restated in replay_cases)."""
    row = RC.BY_ID[rid]
    t = _plan(row)
    assert {"persist": not t.rows and not t.tile and not t.tile_prefix, "rows": bool(t.rows and t.fast),
            "tile": bool(t.tile) and not t.tile_prefix, "tile_prefix": bool(t.tile_prefix) and not t.tile}[row.family]
    plan = N.Plan(t.layout, upload=False)
    kf = plan.kernel_flags
    arr = RC.arrivals(row)
    assert arr == row.arrivals
    n, src_bytes = RC.n_chunks(row), int(np.prod(row.shape)) * np.dtype(row.dtype).itemsize
    assert n >= 5 and src_bytes < 16 << 20
    if row.family in ("persist", "rows"):
        assert plan.units_per_chunk == RC.nseg_of(RC.nbytes(row))
        assert row.kernel == (RC.K if row.family == "persist" else RC.rows_kernel(row))
        if row.kernel != RC.KQ:
            assert plan.units_per_chunk == arr
    else:
        assert kf & N.PK_TILE
        t4 = bool(kf & N.PK_TILE4_ENCODE)
        if row.family == "tile_prefix":
            assert row.kernel == RC.EGEN  # any family: the prefix boxes take k_encode_tile
            assert any(b[2] != row.chunk for b in RC.boxes(row))
        else:
            assert row.kernel == ((RC.E2 if row.crc else RC.E4) if t4 else RC.EG if kf & N.PK_TILEG else RC.EGEN)
    # what the protocol's name says about the arrivals
    p = row.proto
    if "several chunks" in p:
        assert arr == 1 and n >= 2 * RC.RESIDENT_BOUND + 3     # every range of a resident grid holds >= 2 chunks
    if "counted ticket" in p:
        assert arr > 1
    if "edge" in p or "prefix" in p:
        cut = [sum(k != c for k, c in zip(b[2], row.chunk)) for b in RC.boxes(row)]
        assert 0 in cut and max(cut) >= 2
        assert cut[2] >= 1                                     # the "last element" chunk of phase A is a prefix box
    if p == "k_encode_il, one half":
        assert arr <= 16
    if p in ("k_encode_il, two-level word", "k_encode_tile2, third word"):
        assert 16 < arr <= 32
    if "ragged head" in p:
        assert RC.nbytes(row) % 4096 == 0 and RC.nbytes(row) % RC.UNIT != 0 and arr == 32
    if p == "k_encode_pair, pair word":
        assert arr % 2 == 0 and arr <= 32
    if p == "k_encode_pair, OR path":
        assert arr % 2 == 1 or arr > 32
    if p == "k_encode_tileg, one-word arrival":
        assert arr <= 16
    if p == "k_encode_tileg, two-level arrival":
        assert 16 < arr <= 256
    if row.ws == RC.WS_UNUSED:
        assert row.kernel == RC.KQ or not row.crc
    offs, total = RC.slots(row)
    assert all(o % RC.SLOT_ALIGN == 0 for o in offs) and offs[0] >= RC.GUARD
    assert all(b - a >= RC.elen(row) + RC.GUARD for a, b in zip(offs, offs[1:] + [total]))


def test_or_path_rows_cover_the_mask_and_the_counted_crc():
    arr = sorted(RC.arrivals(r) for r in RC.ROWS if r.proto == "k_encode_pair, OR path")
    assert arr[0] <= 32 < arr[-1] and any(a > 32 and a % 2 == 0 for a in arr) and any(a % 2 for a in arr)


@pytest.mark.parametrize("rid", IDS)
def test_phases_defeat_a_stale_or_skipped_replay(rid):
    """A -> B: every chunk's blob (trailer included) changes, at least one flag
    falls and at least one rises.  B -> F: every blob is the one fill blob and
    every flag that was set falls (F, all fill, has none to raise).  F -> A:
    flags rise again.  A's single-element chunks differ from the fill blob in
    exactly one item, at either end; the last phase is the first, bit for bit."""
    row = RC.BY_ID[rid]
    dt = np.dtype(row.dtype)
    assert RC.PHASES == ("A", "B", "F", "A")
    A, B, F = (RC.expected(row, ph) for ph in ("A", "B", "F"))
    n = RC.n_chunks(row)
    assert len(A) == len(B) == len(F) == n
    ne = {k: np.array([not w.empty for w in v]) for k, v in (("A", A), ("B", B), ("F", F))}
    assert (ne["A"] & ~ne["B"]).any() and (~ne["A"] & ne["B"]).any()
    assert not ne["F"].any() and ne["B"].any() and ne["A"].any()
    for a, b in zip(A, B):
        assert not np.array_equal(a.blob, b.blob)
        if row.crc:
            assert a.crc != b.crc
    fb = F[0].blob
    assert all(np.array_equal(w.blob, fb) for w in F)
    nb = RC.nbytes(row)
    rl = RC.roles(row, "A")
    assert rl[:3] == ["fill", "first", "last"] and set(rl[3:]) == {"data"}
    assert RC.roles(row, "B")[:5] == ["data", "data", "fill", "last", "first"]
    assert A[0].empty and np.array_equal(A[0].blob, fb)
    assert B[2].empty and np.array_equal(B[2].blob, fb)
    for ph, want, first, last in (("A", A, 1, 2), ("B", B, 4, 3)):
        for c in (first, last):
            diff = np.nonzero(want[c].blob[:nb] != fb[:nb])[0]
            assert len(diff) and len(set(diff // dt.itemsize)) == 1, (ph, c)
        # the oracle decides emptiness: a second NaN payload is still the fill (all_equal), -0.0 and a flipped bit not
        nan_fill = dt.kind == "f" and np.isnan(RC.fill_of(row))
        assert want[first].empty == want[last].empty == nan_fill
        if row.order is None:  # stored order = C order: the single elements sit at the two ends of the payload
            whole = RC.boxes(row)[first][2] == row.chunk and RC.boxes(row)[last][2] == row.chunk
            d1 = np.nonzero(want[first].blob[:nb] != fb[:nb])[0]
            d2 = np.nonzero(want[last].blob[:nb] != fb[:nb])[0]
            assert d1[0] < dt.itemsize and (not whole or d2[-1] >= nb - dt.itemsize)
    # the last A is the first: source() and expected() are pure in (row, phase)
    assert RC.source(row, RC.PHASES[3]) is RC.source(row, RC.PHASES[0])
    again = np.array(RC.source(row, "A"))
    RC._SOURCES.pop((row.id, "A"))
    assert np.array_equal(again.view(np.uint8), RC.source(row, "A").view(np.uint8))
    img = RC.image(row, "A")
    offs, total = RC.slots(row)
    assert len(img) == total and (img[: offs[0]] == RC.SENTINEL).all() and (img[-RC.GUARD:] == RC.SENTINEL).all()
