"""What licenses tests/test_gpu_foreign_placement.py, proved on the CPU with
nothing launched, for every row and form of tests/placement_cases.py:

  - the table names every decode kernel, and a row's forms put its stored
    objects at all 16 address residues; a sharded row's indexes sit at every
    residue mod 4 when they lead the shard, and at 1, 2 and 3 in each
    odd_index form's row;
  - SAFETY: every window a correct kernel may touch (three bytes before a
    chunk, trailer or index, 64 bytes past its end) lies inside the allocation;
  - the oracle reads the foreign host dict to the bytes it reads from the
    canonical one (alias: with the aliased region replaced), and the index
    CRCs in the backing image verify;
  - TEETH: three numpy mis-readers of the image -- one that reads from
    addr & ~3, one that reads from the canonical (predicted) offsets, one that
    uses the first chunk's residue for every chunk -- each return other bytes
    than the chunk's, for every chunk they apply to; the data has no 4- or
    16-byte period that could hide a shifted read;
  - the planner chooses the row's family over the foreign placements as over
    the canonical ones, and keeps its load prediction where it had one."""

import numpy as np
import pytest

import damage_cases as DC
import placement_cases as PC
from oracle import oracle as O
from test_damage_rules import _chain, _flags_match, _tables, same


def test_the_table_names_every_kernel():
    named = {PC.kernel_of(r, f) for r, f in PC.PARAMS}
    assert named == set(PC.KERNELS), named ^ set(PC.KERNELS)
    assert len(set(PC.IDS)) == len(PC.IDS)
    for row in PC.ROWS:  # one dropped chunk per row, a chunk of the row
        if row.kind == "u":
            assert 0 <= row.drop < len(PC.keys_of(row))
        else:
            assert 0 <= row.drop[0] < len(PC.keys_of(row)) and 0 <= row.drop[1] < row.src["n"]
            names = {f.name for f in PC.forms(row)}
            both = row.kernels[1] is not None
            for f in PC.IN_SHARD:
                for loc in ("end", "start")[: 1 if f.startswith("odd_index") else 2]:
                    assert f"{f}-{loc}-icrc" in names and (f"{f}-{loc}-ibytes" in names) == both


@pytest.mark.parametrize("row", PC.ROWS, ids=[r.id for r in PC.ROWS])
def test_a_rows_forms_cover_every_residue(row):
    n = PC.n_objects(row)
    blob_res, start_res = set(), set()
    odd = {f.name: set() for f in PC.forms(row) if (f.inshard or "").startswith("odd_index")}
    for f in PC.forms(row):
        p = PC.restate(row.id, f.name)
        assert len(p.blobs) == n
        for j, (a, _) in enumerate(p.blobs.values()):
            assert a % 16 == (5 * j + 1 + 5 * n * f.k) % 16 and a >= PC.BASE
        blob_res |= {a % 16 for a, _ in p.blobs.values()}
        if row.kind == "s" and f.loc == "start":
            assert all(p.index[k][0] == p.blobs[k][0] for k in p.blobs)
            start_res |= {a % 4 for a, _ in p.index.values()}
        if f.name in odd:
            odd[f.name] = {a % 4 for a, _ in p.index.values()}
            assert odd[f.name] <= {1, 2, 3}
        if f.inshard == "stagger":  # the chunks walk on through the sequence, across the form's shards
            got = [a % 16 for a, _ in p.chunks.values()]
            assert got == [PC.residue(n * f.k + n + q) for q in range(len(got))]
    assert blob_res == set(range(16))
    if row.kind == "s":
        assert start_res == {0, 1, 2, 3}
        assert set().union(*odd.values()) == {1, 2, 3}
        if n >= 3:  # one launch mixes them
            assert all(v == {1, 2, 3} for v in odd.values())


def _index_crc_ok(p, key):
    a, n = p.index[key]
    raw = p.image[a: a + n].tobytes()
    return int(np.frombuffer(raw[-4:], "<u4")[0]) == O.crc32c(raw[:-4])


def _no_period(b):
    return all(len(b) <= q or (b[q:] != b[:-q]).any() for q in (4, 16))


def _misread(image, at, n):
    return image[max(at, 0): max(at, 0) + n]


@pytest.mark.parametrize("row,form", PC.PARAMS, ids=PC.IDS)
def test_restatement_and_teeth(row, form):
    p = PC.restate(row.id, form.name)
    keys = PC.keys_of(row)
    meta = PC.meta_of(row, form.loc or "end", True if form.icrc is None else form.icrc)
    chost, cwant = PC.canonical(row.id, form.loc or "end", True if form.icrc is None else form.icrc)
    # -- the image holds the host dict's bytes at the stated addresses, nothing overlaps, everything is inside
    assert p.image.size == p.top and p.top + DC.TAIL_SLACK <= p.alloc <= 64 << 20
    spans = sorted(p.blobs.values())
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[0][0] >= PC.BASE
    for k, (a, n) in p.blobs.items():
        assert p.image[a: a + n].tobytes() == p.host[k]
    for lo, hi in PC.windows(p):
        assert 0 <= lo and hi <= p.alloc
    # -- the oracle reads it to the canonical bytes
    assert same(O.read(p.host, meta), p.want)
    if form.inshard == "alias":
        assert p.alias and not same(p.want, cwant)
        g = row.src
        for key, (a, b) in p.alias.items():
            assert p.chunks[(key, a)] == p.chunks[(key, b)] and a != b
            coords = tuple(int(i) for i in np.unravel_index(keys.index(key), g["grid"]))
            ra, rb = (PC._slot_region(g, coords, s) for s in (a, b))
            assert same(p.want[rb], cwant[ra]) and same(p.want[ra], cwant[ra])
    else:
        assert same(p.want, cwant) and not p.alias
    sel = PC.ragged(PC.full_shape(row))
    assert same(O.read(p.host, meta, sel), p.want[sel]) and p.want[sel].size
    # -- index entries and CRCs, read from the image
    if row.kind == "s":
        g = row.src
        for key in p.blobs:
            ents = PC.unpack_index(p.host[key], g["n"], form.loc, form.icrc)
            a0 = p.blobs[key][0]
            for s, (o, ln) in enumerate(ents):
                if (key, s) in p.chunks:
                    assert (a0 + o, ln) == p.chunks[(key, s)] and ln == g["elen"]
                else:
                    assert (o, ln) == (DC.MAXU, DC.MAXU) and (keys.index(key), s) == row.drop
            if form.icrc:
                assert _index_crc_ok(p, key)
        if form.inshard == "dense_reversed":
            assert all((a - p.blobs[k][0]) % 4 == 0 for (k, _), (a, _) in p.chunks.items())
        if form.inshard == "gap":
            for key, (_, n) in p.blobs.items():
                laid = sum(ln for (k, _), (_, ln) in p.chunks.items() if k == key)
                assert n == laid + p.index[key][1] + sum(PC.GAPS) + p.dead[key]
    # -- teeth
    a_first = next(iter(p.chunks.values()))[0]
    applied = [0, 0, 0]
    cplace, _, _ = DC.arena_layout({k: len(v) for k, v in chost.items()})
    for (key, s), (a, n) in p.chunks.items():
        true = p.image[a: a + n]
        assert _no_period(true)
        if p.crc:
            t = PC.trailer(p, key, s)
            assert int(np.frombuffer(p.image[t: t + 4].tobytes(), "<u4")[0]) == O.crc32c(true[:-4].tobytes())
        if a % 4:
            applied[0] += 1
            assert not np.array_equal(_misread(p.image, a & ~3, n), true)
        pred = cplace[key][0] if row.kind == "u" else p.blobs[key][0] + p.canon[(key, s)]
        if pred != a:
            applied[1] += 1
            assert not np.array_equal(_misread(p.image, pred, n), true)
        if a % 16 != a_first % 16:
            applied[2] += 1
            assert not np.array_equal(_misread(p.image, (a & ~15) | (a_first & 15), n), true)
    # which mis-readers a form must have caught
    if row.kind == "u":
        assert all(applied), applied
    elif form.inshard in ("stagger", "gap"):
        assert all(applied), applied
    elif form.inshard in ("dense_reversed", "alias"):
        assert applied[1], applied


def _plan(row, form, place, alloc):
    from zarr_hip import _native as N
    from zarr_hip import planner

    keys = PC.keys_of(row)
    if row.kind == "u":
        r = row.src
        args = (DC.u_shape(r), r.chunk, r.dtype, 3, DC.u_codecs(r))
    else:
        g = row.src
        args = (g["shape"], g["shard"], g["dtype"], 0, PC.meta_of(row, form.loc, form.icrc).codecs)
    t = _tables(*args, place, keys)
    chain, spec = _chain(*args)
    # (as the pipeline does: the il kernels resolve their own units and get no prediction)
    if t.rows and not N.Plan(t.layout, upload=False).kernel_flags & N.PK_IL:
        planner.predict_rows(t, chain, spec, alloc)
    return t


@pytest.mark.parametrize("row,form", PC.PARAMS, ids=PC.IDS)
def test_the_planner_chooses_the_same_family(row, form):
    from zarr_hip import _native as N

    p = PC.restate(row.id, form.name)
    chost, _ = PC.canonical(row.id, form.loc or "end", True if form.icrc is None else form.icrc)
    cplace, _, calloc = DC.arena_layout({k: len(v) for k, v in chost.items()})
    tc = _plan(row, form, cplace, calloc)
    tf = _plan(row, form, dict(p.blobs), p.alloc)
    kernel = PC.kernel_of(row, form)
    for t in (tc, tf):
        if row.prefix:  # the row's table names the family alone: which tile kernel, the equal flags below say
            assert t.tile and kernel == "k_decode_tile"
        else:
            _flags_match(t, kernel)
    kf = [N.Plan(t.layout, upload=False).kernel_flags for t in (tc, tf)]
    assert kf[0] == kf[1] and (bool(tc.fast), bool(tc.rows), bool(tc.tile)) == (bool(tf.fast), bool(tf.rows),
                                                                                 bool(tf.tile))
    assert len(tc.chunks) == len(tf.chunks)
    assert (tc.predict is None) == (tf.predict is None)
    il = bool(kf[0] & N.PK_IL)
    assert (tf.predict is not None) == (row.kind == "s" and bool(tc.rows) and not il)  # (sharded: the miss path)
    by_item = {int(i): (int(c["src"]), int(c["src_len"])) for i, c in zip(tf.item_of_chunk, tf.chunks)}
    keys = PC.keys_of(row)
    for i, place in by_item.items():
        if keys[i] in p.blobs:
            assert place == p.blobs[keys[i]]
