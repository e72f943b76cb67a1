"""Foreign placements per decode family: the one table behind
tests/test_placement_rules.py (CPU) and tests/test_gpu_foreign_placement.py (GPU).

Everything the other matrices read was placed by this library: blobs on
256-byte granules, inner chunks packed densely in Morton order, so every
address a kernel sees is a multiple of 4 and every predicted address is right.
Neither the zarr format nor the C ABI promises that: a shard index holds
absolute (offset, nbytes) pairs, zhip_chunk.src is a byte offset, and
DeviceStore.get_sync(key, byte_range) hands out off + a.  A ROW here is the
smallest geometry that reaches one decode kernel (damage_cases.U_ROWS,
damage_cases.S_ROWS and test_gpu_shard_index.B_CASES, as they are), the kernel
zhip_last_kernel() must report, and one dropped chunk.  A FORM places the
row's stored objects (chunk blobs or shard blobs) at odd byte addresses and,
for sharded rows, lays the inside of every shard out as another writer might.

BASE RESIDUES.  Stored object j of a row with n objects sits, in form number
k, at an absolute address = (5 j + 1 + 5 n k) mod 16: objects follow each other
at a constant stride = 5 (mod 16) from arena offset 256 + (1 + 5 n k) mod 16
(a constant stride keeps the planner's load prediction on, so the predicted
loads see the odd addresses too).  ceil(16 / n) forms show a row all 16
residues.

IN-SHARD FORMS (foreign_shard): stagger, dense_reversed, gap, alias and
odd_index1..3, at both index locations, with and without an index CRC where
the row's table has both (B_CASES).

restate() gives, per row and form, the host dict a zarr reader sees, the
backing image, and the absolute address of every blob, inner chunk, trailer
and index in it; windows() the bytes a correct kernel may touch.  A shard whose
body would come out shorter than the canonical one keeps dead bytes after its
chunks, so the planner's predicted addresses stay inside the blob and its load
prediction stays on: every predicted address is then wrong (the miss path).

This module imports nothing of the library under test."""

import functools
import struct
from collections import namedtuple

import numpy as np

import damage_cases as DC
from damage_cases import ALIGN, CRC, LE, MAXU, TAIL_SLACK
from oracle import oracle as O
from test_gpu_decode import SHARD, _data
from test_gpu_shard_index import B_CASES, _entry, _index_start, _slot_region

BASE = 256          # the first placement's granule: three bytes before a chunk are readable (the dword funnel)
FUNNEL = 3          # bytes before an address the aligned-dword funnel may read
PAD = 0x5A          # what lies between placements (nothing a reader may rely on)
GAPS = (4097, 1)

# ------------------------------------------------------------------ rows
# kind "u": src is a damage_cases.URow; "s": a test_gpu_shard_index._geom dict.  kernels: (with an index CRC,
# without one); None: the row's table does not run that variant.  drop: the batch item (unsharded) or
# (batch item, C-order slot) (sharded) that is missing.  prefix: the kernel name is matched by prefix, as the
# row's own table does.
Row = namedtuple("Row", "id kind src kernels drop fused prefix")


def _rows():
    rows = [Row("u_" + r.id, "u", r, (r.kernel, None), r.damaged, r.fused, False) for r in DC.U_ROWS]
    for g in B_CASES:
        if g.get("dec") is not None:
            rows.append(Row("b_" + g["id"], "s", g, tuple(k.decode() for k in g["dec"]), (0, g["slot"]), 0,
                            bool(g.get("prefix"))))
    rows += [Row("s_" + g["id"], "s", g, (g["dec"], None), (g["item"], g["slot"]), g["fused"], False)
             for g in DC.S_ROWS]
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# every kernel name the rows must show (tests/test_placement_rules.py checks the table against it)
KERNELS = ["k_decode", "k_decode_tile", "k_decode_lead", "k_decode_lead4", "k_decode_lead8", "k_decode_pair",
           "k_decode_duo", "k_decode_il", "k_decode_ilh", "k_decode_ilw512", "k_decode_tile4", "k_decode_tile2w",
           "k_decode_tile4w", "k_decode_tileg", "k_decode_tileg2w"]

IN_SHARD = ["stagger", "dense_reversed", "gap", "alias", "odd_index1", "odd_index2", "odd_index3"]
Form = namedtuple("Form", "name k inshard loc icrc")


def keys_of(row):
    return DC.u_keys(row.src) if row.kind == "u" else DC.s_keys(row.src)


def n_objects(row):
    """Stored objects: the chunk blobs that are there, or the shard blobs."""
    return len(keys_of(row)) - (1 if row.kind == "u" else 0)


def forms(row):
    """The row's forms.  Unsharded: base0 .. base(K-1), K = ceil(16 / n) or more.  Sharded: every in-shard form
    at both index locations (odd_index: the end only), with and without an index CRC where the table has both;
    form number i has k = i."""
    n = n_objects(row)
    if row.kind == "u":
        # (a row fused three times gets three forms at the least: one launch over three stores)
        return [Form(f"base{k}", k, None, None, None) for k in range(max(-(-16 // n), row.fused))]
    combos = [(f, loc, icrc) for icrc in (True, False) if row.kernels[0 if icrc else 1] is not None
              for f in IN_SHARD for loc in ("end", "start") if not (f.startswith("odd_index") and loc == "start")]
    assert len(combos) * n >= 16
    return [Form(f"{f}-{loc}-{'icrc' if icrc else 'ibytes'}", k, f, loc, icrc)
            for k, (f, loc, icrc) in enumerate(combos)]


def kernel_of(row, form):
    return row.kernels[0] if row.kind == "u" or form.icrc else row.kernels[1]


PARAMS = [(r, f) for r in ROWS for f in forms(r)]
IDS = [f"{r.id}-{kernel_of(r, f)}-{f.name}" for r, f in PARAMS]


# ------------------------------------------------------------------ the canonical stores
def meta_of(row, loc="end", icrc=True):
    if row.kind == "u":
        r = row.src
        return O.ArrayMeta(DC.u_shape(r), r.chunk, np.dtype(r.dtype), 3, codecs=DC.u_codecs(r))
    g = row.src
    codecs = [SHARD(g["inner"], g["chain"], loc, index=(LE, CRC) if icrc else (LE,))]
    return O.ArrayMeta(g["shape"], g["shard"], np.dtype(g["dtype"]), 0, codecs=codecs)


def full_shape(row):
    return DC.u_shape(row.src) if row.kind == "u" else tuple(row.src["shape"])


def dtype_of(row):
    return np.dtype(row.src.dtype if row.kind == "u" else row.src["dtype"])


def fill_of(row):
    return 3 if row.kind == "u" else 0


def drop_region(row):
    if row.kind == "u":
        return DC.u_region(row.src, row.drop)
    g = row.src
    return _slot_region(g, tuple(int(i) for i in np.unravel_index(row.drop[0], g["grid"])), row.drop[1])


def isz_of(row, icrc):
    return 16 * row.src["n"] + (4 if icrc else 0)


def _set_entry(blob, n, loc, icrc, slot, off, ln, sh):
    """The blob with entry `slot` = (off, ln), the index encoded again by the oracle."""
    s = _index_start(len(blob), n, loc, icrc)
    idx = np.frombuffer(blob[s: s + 16 * n], "<u8").reshape(n, 2).copy()
    idx[slot] = (off, ln)
    ib = O.encode_shard_index(idx, sh.index).tobytes()
    assert len(ib) == 16 * n + (4 if icrc else 0)
    return blob[:s] + ib + blob[s + len(ib):]


@functools.lru_cache(maxsize=2)
def canonical(rid, loc="end", icrc=True):
    """(host dict with the row's chunk dropped, the whole array the oracle reads from it): what this library's
    own writers would have stored."""
    row = BY_ID[rid]
    meta = meta_of(row, loc, icrc)
    host = {}
    O.write(host, meta, (Ellipsis,), _data(full_shape(row), dtype_of(row), 43))
    keys = keys_of(row)
    assert list(host) == keys
    if row.kind == "u":
        del host[keys[row.drop]]
    else:
        g, (item, slot) = row.src, row.drop
        assert all(len(v) == g["n"] * g["elen"] + isz_of(row, icrc) for v in host.values())
        host[keys[item]] = _set_entry(host[keys[item]], g["n"], loc, icrc, slot, MAXU, MAXU, meta.chain.shard)
    want = O.read(host, meta)
    assert (want[drop_region(row)] == fill_of(row)).all()
    return host, want


# ------------------------------------------------------------------ the in-shard forms
def residue(m):
    """Residue number m of the sequence every form walks: 1, 6, 11, 0, 5, ... (all 16 in 16 steps)."""
    return (5 * m + 1) % 16


def _aligned(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def alias_pair(present):
    """(the slot whose bytes stay, the slot whose entry names them too) of a shard's present slots."""
    return (present[0], present[-1]) if len(present) >= 2 else None


def foreign_shard(blob, n, loc, icrc, inshard, sh, cps, base, j, m0):
    """The canonical shard `blob` (shard number j of its row, to sit at absolute address `base`) laid out again.

      stagger         chunks in reverse C order, each preceded by the pad (0..15 bytes) that gives its absolute
                      address residue(m0), residue(m0 + 1), ...
      dense_reversed  reverse C order, nothing between: as aligned as the base, every predicted address wrong
      gap             stored order, a gap of 4097 bytes before the second chunk and of 1 byte before the last
      alias           stored order; the entry of the last present slot names the first present slot's bytes,
                      its own bytes are not stored
      odd_indexR      (index at the end) stored order, then the pad that puts the index at an absolute address
                      = 1 + (j + R) mod 3 (mod 4)
    -> (bytes, {slot: (offset, nbytes)}, offset of the index, chunks laid, dead bytes)."""
    isz = 16 * n + (4 if icrc else 0)
    ents = {s: _entry(blob, n, loc, icrc, s) for s in range(n)}
    present = [s for s in range(n) if ents[s] != (MAXU, MAXU)]
    raw = {s: blob[ents[s][0]: ents[s][0] + ents[s][1]] for s in present}
    stored = sorted(present, key=lambda s: ents[s][0])
    start = isz if loc == "start" else 0
    parts, top, at = [], start, {}

    def pad(p):
        nonlocal top
        parts.append(bytes([PAD]) * p)
        top += p

    def lay(s):
        nonlocal top
        at[s] = (top, len(raw[s]))
        parts.append(raw[s])
        top += len(raw[s])

    if inshard == "stagger":
        for q, s in enumerate(reversed(present)):
            pad((residue(m0 + q) - (base + top)) % 16)
            lay(s)
    elif inshard == "dense_reversed":
        for s in reversed(present):
            lay(s)
    elif inshard == "gap":
        for q, s in enumerate(stored):
            if q == min(1, len(stored) - 1):
                pad(GAPS[0])
            if q == len(stored) - 1:
                pad(GAPS[1])
            lay(s)
    elif inshard == "alias":
        pair = alias_pair(present)
        for s in stored:
            if pair is None or s != pair[1]:
                lay(s)
        if pair is not None:
            at[pair[1]] = at[pair[0]]
    else:
        assert inshard.startswith("odd_index") and loc == "end"
        for s in stored:
            lay(s)
    # the bytes of a chunk that is no longer named stay behind as dead space after the others (a writer that
    # dropped a chunk by rewriting the index alone): the body is never shorter than the canonical one, so the
    # planner's predicted addresses stay inside the blob and its load prediction stays on
    dead = max(0, len(blob) - isz - (top - start))
    pad(dead)
    if inshard.startswith("odd_index"):
        pad((1 + (j + int(inshard[-1])) % 3 - (base + top)) % 4)
    index = np.full((n, 2), MAXU, dtype="<u8")
    for s, (o, ln) in at.items():
        index[s] = (o, ln)
    ib = O.encode_shard_index(index.reshape(tuple(cps) + (2,)), sh.index).tobytes()
    assert len(ib) == isz
    body = b"".join(parts)
    out = ib + body if loc == "start" else body + ib
    return out, at, (0 if loc == "start" else len(body)), len(set(at.values())), dead


# ------------------------------------------------------------------ the restatement
# host: what a zarr reader sees (key -> bytes); want: what it must read; image: the backing's bytes [0, top);
# alloc: the allocation's size (DeviceArena: the capacity in granules and 64 bytes of slack); blobs: key ->
# (address, nbytes); chunks: (key, slot) -> (address, nbytes) with the trailer; index: key -> (address, nbytes);
# canon: (key, slot) -> offset in the canonical blob; alias: key -> (kept slot, aliased slot); dead: key -> dead
# bytes kept after the shard's chunks
Placed = namedtuple("Placed", "host want image top alloc blobs chunks index canon alias crc dead")


@functools.lru_cache(maxsize=2)
def restate(rid, fname):
    row = BY_ID[rid]
    form = {f.name: f for f in forms(row)}[fname]
    keys, n = keys_of(row), n_objects(row)
    host, chunks, index, canon, alias, dead = {}, {}, {}, {}, {}, {}
    if row.kind == "u":
        chost, want = canonical(rid)
        host = dict(chost)
        crc = row.src.crc
    else:
        g = row.src
        chost, want = canonical(rid, form.loc, form.icrc)
        sh = meta_of(row, form.loc, form.icrc).chain.shard
        crc = CRC in g["chain"]
        lens = [len(v) + sum(GAPS) + 16 * g["n"] for v in chost.values()]  # no form adds more than this
    stride = _aligned((max(len(v) for v in chost.values()) if row.kind == "u" else max(lens)) + TAIL_SLACK) + 5
    first = BASE + residue(n * form.k)
    blobs, m = {}, n * form.k + n
    for j, key in enumerate(k for k in keys if k in chost):
        addr = first + j * stride
        assert addr % 16 == residue(j + n * form.k)
        if row.kind == "u":
            chunks[(key, 0)] = (addr, len(host[key]))
            canon[(key, 0)] = 0
        else:
            blob, at, ioff, laid, dead[key] = foreign_shard(chost[key], g["n"], form.loc, form.icrc, form.inshard, sh,
                                                            g["cps"], addr, j, m)
            m += laid
            host[key] = blob
            index[key] = (addr + ioff, isz_of(row, form.icrc))
            for s, (o, ln) in at.items():
                chunks[(key, s)] = (addr + o, ln)
                canon[(key, s)] = _entry(chost[key], g["n"], form.loc, form.icrc, s)[0]
            pair = alias_pair(sorted(at))
            if form.inshard == "alias" and pair is not None:
                alias[key] = pair
                item = keys.index(key)
                coords = tuple(int(i) for i in np.unravel_index(item, g["grid"]))
                if len(alias) == 1:  # (the canonical array is shared)
                    want = want.copy()
                want[_slot_region(g, coords, pair[1])] = want[_slot_region(g, coords, pair[0])]
        assert len(host[key]) + TAIL_SLACK <= stride
        blobs[key] = (addr, len(host[key]))
    top = _aligned(max(a + ln for a, ln in blobs.values()))
    image = np.full(top, PAD, np.uint8)
    for key, (a, ln) in blobs.items():
        image[a: a + ln] = np.frombuffer(host[key], np.uint8)
    alloc = _aligned(max(top + ALIGN, 1 << 16)) + TAIL_SLACK
    return Placed(host, want, image, top, alloc, blobs, chunks, index, canon, alias, crc, dead)


def trailer(p, key, slot):
    """Address of the chunk's CRC trailer (None: the chain has none)."""
    a, ln = p.chunks[(key, slot)]
    return a + ln - 4 if p.crc else None


def windows(p):
    """[lo, hi) of every region a correct kernel may touch: three bytes before a chunk, a trailer or an index
    (the aligned-dword funnel) to 64 bytes past its end (include/zarrhip.h)."""
    regs = list(p.chunks.values()) + list(p.index.values())
    return [(a - FUNNEL, a + ln + TAIL_SLACK) for a, ln in regs]


def ragged(shape):
    """One partial selection that cuts chunks in every dimension long enough to cut (test_gpu_shard_index._ragged
    for short leading dimensions too), every other element of the last."""
    if len(shape) == 1:
        return (slice(3, shape[0] - 5, 3),)
    lead = [slice(1 + d, n - 2 - d) if n - 2 - d > 1 + d else slice(0, n) for d, n in enumerate(shape[:-1])]
    return tuple(lead) + (slice(1, shape[-1] - 1, 2),)


def unpack_index(blob, n, loc, icrc):
    s = _index_start(len(blob), n, loc, icrc)
    return [struct.unpack("<QQ", blob[s + 16 * i: s + 16 * i + 16]) for i in range(n)]
