"""Independent decodes in one kernel launch: zhip_decode_mapped_multi /
k_decode_il_multi, ReadGraph(fuse=True) and ProgramGroup.launch.

A fused grid runs launch i's workgroups after launch i - 1's, each on its own
parameters with its own workgroup index and grid size, so what can go wrong is
a workgroup of one launch using another's index arithmetic, tables, statuses
or arrival words.  The fused path needs the production k_decode_il, which
launches of at most 512 units do not take: the smallest program here is 20
chunks of 1 MiB (64^3 float32, 32 units each: 640 units, an array of
(1280, 64, 64)); the unequal one has 24 (768 units); the sharded one is
(384, 128, 128) in 128^3 shards of 64^3 inner chunks (24 inner chunks, three
shard indexes checked in the launch's leading workgroups).  Outs are compared
with the source arrays through integer views (the bytes the oracle encoded),
so no array takes an oracle read; the error messages come from the oracle
reading one element of the corrupted chunk or shard."""

import types

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_decode import CRC, LE, SHARD

pytestmark = pytest.mark.gpu

CHUNK = (64, 64, 64)
FILL = 0.0


def _array(device, shape, chunks, codecs, seed, drop=()):
    import zarr_hip

    data = np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)
    meta = O.ArrayMeta(shape, chunks, np.dtype("float32"), FILL, codecs=codecs)
    host: dict = {}
    O.write(host, meta, (Ellipsis,), data)
    want = data.copy()
    for key in drop:  # a missing chunk reads as fill
        del host[key]
        i = int(key.split("/")[1])
        want[i * chunks[0]: (i + 1) * chunks[0]] = FILL
    store = zarr_hip.DeviceStore.from_host(host, device)
    arr = zarr_hip.Array.create(store, shape, chunks, "float32", FILL, codecs=codecs)
    return types.SimpleNamespace(arr=arr, store=store, host=host, meta=meta, want=want)


@pytest.fixture(scope="module")
def plain(device):
    """Three arrays of 20 chunks with different seeds (the third with chunk 1
    missing) and one of 24 chunks."""
    a = [_array(device, (1280, 64, 64), CHUNK, [LE, CRC], 11),
         _array(device, (1280, 64, 64), CHUNK, [LE, CRC], 12),
         _array(device, (1280, 64, 64), CHUNK, [LE, CRC], 13, drop=("c/1/0/0",)),
         _array(device, (1536, 64, 64), CHUNK, [LE, CRC], 14)]
    for x in a:
        x.prog, x.out = x.arr.prepare_read((Ellipsis,))
        assert x.prog.index is None and x.prog.data.p_rowmap is not None
    return a


@pytest.fixture(scope="module")
def sharded(device):
    a = [_array(device, (384, 128, 128), (128, 128, 128), [SHARD(CHUNK, [LE, CRC])], 21 + i) for i in range(3)]
    for x in a:
        x.prog, x.out = x.arr.prepare_read((Ellipsis,))
        assert x.prog.index is None and x.prog.data.n_idx == 3  # index checks ride in the data launch
    return a


def _exact(x, out=None, want=None):
    got = (x.out if out is None else out).cpu().numpy().view(np.uint32)
    return np.array_equal(got, (x.want if want is None else want).view(np.uint32))


def _zero(xs):
    for x in xs:
        x.out.zero_()


def _kernel():
    from zarr_hip import _native as N

    return N.lib().zhip_last_kernel().decode()


def _flip(store, key, pos, bit=0x08):
    ref = store.get_sync(key)
    ref.arena.buf[ref.offset + (pos if pos >= 0 else ref.length + pos)] ^= bit


def _graph_pair(device, progs, repeats):
    """The fused and the unfused graph of one sequence."""
    import zarr_hip

    return (zarr_hip.ReadGraph(progs, repeats, device), zarr_hip.ReadGraph(progs, repeats, device, fuse=False))


def test_three_arrays_one_launch_at_the_abi(device, plain):
    import torch

    from zarr_hip import _native as N
    from zarr_hip.pipeline import _stream_handle

    xs = plain[:3]
    _zero(xs)
    lib = N.lib()
    assert lib.zhip_multi_max() == 3
    args = (N.MappedArgs * 3)(*[x.prog.data.mapped_args(x.prog.data._begin()) for x in xs])
    n0 = lib.zhip_launch_count()
    N.check(lib.zhip_decode_mapped_multi(args, 3, _stream_handle(device)), "zhip_decode_mapped_multi")
    assert lib.zhip_launch_count() - n0 == 1
    assert _kernel() == "k_decode_il"
    torch.cuda.synchronize(device)
    for x in xs:
        res = x.prog.results()
        assert [r["status"] for r in res].count("missing") == (1 if x is xs[2] else 0)
        assert _exact(x)
    # a launch of at most 512 units takes another kernel alone: declined, nothing launched
    small = _array(device, (256, 64, 64), CHUNK, [LE, CRC], 15)
    ps, _ = small.arr.prepare_read((Ellipsis,))
    pair = (N.MappedArgs * 2)(xs[0].prog.data.mapped_args(xs[0].prog.data.flags), ps.data.mapped_args(ps.data.flags))
    n0 = lib.zhip_launch_count()
    assert lib.zhip_decode_mapped_multi(pair, 2, _stream_handle(device)) == N.E_UNSUPPORTED
    assert lib.zhip_launch_count() == n0


def test_three_arrays_one_launch_in_a_graph(device, plain):
    xs = plain[:3]
    fused, plainly = _graph_pair(device, [x.prog for x in xs], 3)
    assert fused.launches == 1 and plainly.launches == 3
    assert _kernel() == "k_decode_il"
    _zero(xs)
    fused.replay()
    fused.results()
    got = [x.out.clone() for x in xs]
    assert all(_exact(x) for x in xs)
    _zero(xs)
    plainly.replay()
    plainly.results()
    import torch

    assert all(torch.equal(g.view(torch.int32), x.out.view(torch.int32)) for g, x in zip(got, xs))


@pytest.mark.parametrize("order", [(0, 3), (3, 0)])
def test_unequal_programs(device, plain, order):
    """640 and 768 workgroups: the second program's arithmetic must not see the
    first grid's size (nor the fused grid's)."""
    xs = [plain[i] for i in order]
    fused, _ = _graph_pair(device, [x.prog for x in xs], 2)
    assert fused.launches == 1
    _zero(xs)
    fused.replay()
    fused.results()
    assert all(_exact(x) for x in xs)


def test_sharded_programs_check_their_own_indexes(device, sharded):
    xs = sharded
    fused, _ = _graph_pair(device, [x.prog for x in xs], 3)
    assert fused.launches == 1 and _kernel() == "k_decode_il"
    _zero(xs)
    fused.replay()
    fused.results()
    assert all(_exact(x) for x in xs)
    # an index CRC corrupted in program 3 (g0 > 0: the third grid's leading workgroups check it)
    key = "c/1/0/0"
    _flip(xs[2].store, key, -10, 0x01)
    bad = dict(xs[2].host)
    blob = bytearray(bad[key])
    blob[-10] ^= 0x01
    bad[key] = bytes(blob)
    with pytest.raises(ValueError) as want:
        O.read(bad, xs[2].meta, (slice(128, 129), slice(0, 1), slice(0, 1)))
    _zero(xs)
    fused.replay()
    import torch

    torch.cuda.synchronize(device)
    xs[0].prog.results()
    xs[1].prog.results()
    with pytest.raises(ValueError) as got:
        xs[2].prog.results()
    assert str(got.value) == str(want.value)
    assert _exact(xs[0]) and _exact(xs[1])
    _flip(xs[2].store, key, -10, 0x01)
    xs[2].prog.data.reset_errflag()
    fused.replay()
    fused.results()
    assert all(_exact(x) for x in xs)


def test_corruption_stays_in_its_program(device, plain):
    """A payload bit flipped in program 2: only its results() raises (the
    oracle's message, from reading one element of that chunk); programs 1 and 3
    are exact, program 3's missing chunk is filled; restored, a replay is clean."""
    import torch

    xs = plain[:3]
    fused, _ = _graph_pair(device, [x.prog for x in xs], 3)
    assert fused.launches == 1
    key = "c/3/0/0"
    _flip(xs[1].store, key, 17)
    bad = dict(xs[1].host)
    blob = bytearray(bad[key])
    blob[17] ^= 0x08
    bad[key] = bytes(blob)
    with pytest.raises(ValueError) as want:
        O.read(bad, xs[1].meta, (slice(192, 193), slice(0, 1), slice(0, 1)))
    _zero(xs)
    fused.replay()
    torch.cuda.synchronize(device)
    assert all(r["status"] == "present" for r in xs[0].prog.results())
    with pytest.raises(ValueError) as got:
        xs[1].prog.results()
    assert str(got.value) == str(want.value)
    assert [r["status"] for r in xs[2].prog.results()].count("missing") == 1
    assert _exact(xs[0]) and _exact(xs[2])
    _flip(xs[1].store, key, 17)
    xs[1].prog.data.reset_errflag()
    _zero(xs)
    fused.replay()
    fused.results()
    assert all(_exact(x) for x in xs)


WINDOW = (slice(1, 1279), slice(1, 63), slice(None))  # every chunk, no whole one: 640 units through the row map


def test_mixed_selections(device, plain):
    """A whole read takes k_decode_il's affine form, a window of the same
    geometry the row map: two instantiations, so the pair is NOT fused (two
    launches) and both are exact; two windows are fused and exact."""
    from zarr_hip import _native as N

    a, b = plain[0], plain[1]
    pw, ow = b.arr.prepare_read(WINDOW)
    pv, ov = a.arr.prepare_read(WINDOW)
    assert a.prog.data.flags & N.DF_WHOLE and not pw.data.flags & N.DF_WHOLE and pw.data.p_rowmap is not None
    mixed, _ = _graph_pair(device, [a.prog, pw], 2)
    assert mixed.launches == 2
    a.out.zero_()
    ow.zero_()
    mixed.replay()
    mixed.results()
    assert _kernel() == "k_decode_il"
    assert _exact(a) and _exact(b, ow, np.ascontiguousarray(b.want[WINDOW]))
    both, _ = _graph_pair(device, [pv, pw], 2)
    assert both.launches == 1
    ov.zero_()
    ow.zero_()
    both.replay()
    both.results()
    assert _exact(a, ov, np.ascontiguousarray(a.want[WINDOW])) and _exact(b, ow, np.ascontiguousarray(b.want[WINDOW]))


def test_sequences(device, plain):
    """Ten decodes over four programs: [0 1 2] [3 0 1] [2 3 0] [1]; replayed
    twice, the outs are the unfused graph's.  Programs sharing an out keep
    their order; a lone program keeps one launch per decode."""
    import torch

    import zarr_hip
    from zarr_hip import pipeline as P

    progs = [x.prog for x in plain]
    n0 = P.LAUNCHES[0]
    fused, plainly = _graph_pair(device, progs, 10)
    assert P.LAUNCHES[0] - n0 == 20  # counted per program, fused or not
    assert fused.launches == 4 and plainly.launches == 10
    _zero(plain)
    fused.replay()
    fused.replay()
    fused.results()
    assert all(_exact(x) for x in plain)
    got = [x.out.clone() for x in plain]
    _zero(plain)
    plainly.replay()
    plainly.replay()
    plainly.results()
    assert all(torch.equal(g.view(torch.int32), x.out.view(torch.int32)) for g, x in zip(got, plain))
    # two programs, one out: not fused, the later one's bytes win
    a, b = plain[0], plain[1]
    try:
        b.prog.retarget(a.out)
        shared = zarr_hip.ReadGraph([a.prog, b.prog], 2, device)
        assert shared.launches == 2
        a.out.zero_()
        shared.replay()
        shared.results()
        assert _exact(b, a.out)
    finally:
        b.prog.retarget(b.out)
    assert zarr_hip.ReadGraph([a.prog], 3, device).launches == 3


def test_program_group_one_launch(device):
    """A rectilinear grid whose two chunk shapes give two spec groups of 640
    units each (20 chunks of 1 MiB, 10 of 2 MiB): ProgramGroup.launch reads
    both through one kernel launch, exact."""
    import zarr_hip
    from zarr_hip import _native as N
    from zarr_hip import pipeline as P

    grid = ([64] * 20 + [128] * 10, [64], [64])
    x = _array(device, (2560, 64, 64), grid, [LE, CRC], 31)
    prog, out = x.arr.prepare_read((Ellipsis,))
    assert isinstance(prog, P.ProgramGroup) and len(prog.programs) == 2
    assert sorted(p.data.n * p.data.plan.units_per_chunk for p in prog.programs) == [640, 640]
    for _ in range(2):  # (the second launch takes the cached cut)
        out.zero_()
        n0, l0 = N.lib().zhip_launch_count(), P.LAUNCHES[0]
        prog.launch()
        assert N.lib().zhip_launch_count() - n0 == 1 and P.LAUNCHES[0] - l0 == 2
        assert _kernel() == "k_decode_il"
        assert all(r["status"] == "present" for r in prog.results())
        assert _exact(x, out)
