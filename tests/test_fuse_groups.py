"""CPU-side checks of the fused launch: how a launch sequence is cut into runs
that may share a kernel launch (pipeline.fuse_groups), and the argument checks
of zhip_decode_mapped_multi, which answer before anything is launched (through
the entry point itself where no plan is read, else through its check-only
twin zhip_decode_mapped_multi_check, which takes plans that were never
uploaded).  No GPU needed."""

from zarr_hip.pipeline import FuseEntry, fuse_groups


class _L:  # a launch: compared by identity
    pass


def _entries(n, width=100, **kw):
    return [FuseEntry(_L(), "cuda:0", True, (1000 * i, 1000 * i + width), **kw) for i in range(n)]


def _cycle(es, k):
    return [es[i % len(es)] for i in range(k)]


def _runs(seq, max_n=3):
    runs = fuse_groups(seq, max_n)
    assert [i for r in runs for i in r] == list(range(len(seq)))  # every entry once, in order
    return [len(r) for r in runs]


def test_cycle_of_four_at_three_per_launch():
    es = _entries(4)
    assert _runs(_cycle(es, 20)) == [3, 3, 3, 3, 3, 3, 2]  # 20 decodes, 7 launches
    assert _runs(_cycle(es, 5)) == [3, 2]
    assert _runs(_cycle(es, 10)) == [3, 3, 3, 1]
    assert _runs(_cycle(es, 20), max_n=2) == [2] * 10
    assert _runs([]) == []
    assert _runs(es[:1]) == [1]


def test_a_launch_never_meets_itself():
    a, b, c = _entries(3)
    assert _runs([a, a, a]) == [1, 1, 1]
    assert _runs([a, b, a, b]) == [2, 2]
    assert _runs([a, b, a]) == [2, 1]
    assert _runs([a, b, c, a]) == [3, 1]
    assert _runs(_cycle([a, b], 5)) == [2, 2, 1]


def test_overlapping_outs_stay_ordered():
    a = FuseEntry(_L(), "cuda:0", True, (0, 100))
    b = FuseEntry(_L(), "cuda:0", True, (99, 200))  # one byte in common
    c = FuseEntry(_L(), "cuda:0", True, (100, 200))  # adjacent
    n = FuseEntry(_L(), "cuda:0", True, None)  # no out to compare
    assert _runs([a, b]) == [1, 1]
    assert _runs([a, c]) == [2]
    assert _runs([a, c, b]) == [2, 1]  # b overlaps c (and a)
    assert _runs([a, n]) == [1, 1]
    # one ProgramGroup: disjoint by construction, whatever the outs' extents
    g = object()
    ga, gb = (FuseEntry(_L(), "cuda:0", True, (0, 100), g) for _ in range(2))
    assert _runs([ga, gb]) == [2]
    other = FuseEntry(_L(), "cuda:0", True, (0, 100), object())
    assert _runs([ga, other]) == [1, 1]


def test_only_single_mapped_launches_on_one_device():
    a, b, c, d = _entries(4)
    idx = FuseEntry(_L(), "cuda:0", False, (9000, 9100))  # an index launch, or staging still pending
    assert _runs([a, idx, b, c]) == [1, 1, 2]
    assert _runs([idx, a, b]) == [1, 2]
    assert _runs([a, b, idx]) == [2, 1]
    far = FuseEntry(_L(), "cuda:1", True, (9000, 9100))
    assert _runs([a, far, b]) == [1, 1, 1]
    assert _runs([a, b, far, c, d]) == [2, 1, 2]


# ---------------------------------------------------------------- ABI checks

def _plan(itemsize=4, swap=False, chunk_bytes=1 << 20):
    """A CRC whole-row plan of `chunk_bytes` chunks (1 MiB: 32 units, S = 32), not uploaded."""
    from zarr_hip import _native as N
    from zarr_hip.planner import _make_layout

    shape = (chunk_bytes // (64 * 64 * itemsize), 64, 64)
    ost = [64 * 64 * itemsize, 64 * itemsize, itemsize]
    L = _make_layout(shape, itemsize, ost, N.LF_CRC | (N.LF_SWAP if swap else 0), b"\0")
    return N.Plan(L, upload=False)


def _args(plan, slot, n_chunks=20, whole=True):
    """One entry with plausible, never-read device addresses; `slot` keeps the tables apart."""
    from zarr_hip import _native as N

    a = N.MappedArgs()
    base = 0x10000000 * (slot + 1)
    a.plan, a.src, a.src_size, a.out = plan.handle, base, 1 << 30, base + 0x1000000
    a.d_chunks, a.n_chunks, a.d_sels = base + 0x2000000, n_chunks, base + 0x2100000
    a.d_status, a.d_workspace, a.d_errflag = base + 0x2200000, base + 0x2300000, base + 0x2400000
    a.decode_flags = N.DF_FAST_ROWS | N.DF_ROWS | N.DF_DEFER | (N.DF_WHOLE if whole else 0)
    a.d_rowmap = base + 0x2500000
    return a


def _check(*entries):
    from zarr_hip import _native as N

    arr = (N.MappedArgs * len(entries))(*entries)
    return N.lib().zhip_decode_mapped_multi_check(arr, len(entries))


def test_multi_admits_what_it_documents():
    from zarr_hip import _native as N

    lib = N.lib()
    mx = lib.zhip_multi_max()
    assert mx == 3
    p = _plan()
    assert _check(_args(p, 0), _args(p, 1)) == 0
    assert _check(_args(p, 0), _args(p, 1, n_chunks=24), _args(p, 2)) == 0  # unequal grids
    # the entry counts: 0, 1 and max + 1, answered by the entry point itself before it reads an entry
    arr = (N.MappedArgs * (mx + 1))(*[_args(p, i) for i in range(mx + 1)])
    for n in (0, 1, mx + 1):
        assert lib.zhip_decode_mapped_multi(arr, n, None) == N.E_UNSUPPORTED
        assert lib.zhip_decode_mapped_multi_check(arr, n) == N.E_UNSUPPORTED
    # a shared workspace or status table, also at the entry point
    for field in ("d_workspace", "d_status"):
        a, b = _args(p, 0), _args(p, 1)
        setattr(b, field, getattr(a, field))
        pair = (N.MappedArgs * 2)(a, b)
        assert lib.zhip_decode_mapped_multi(pair, 2, None) == N.E_UNSUPPORTED
        assert b"share" in lib.zhip_last_error()
        assert _check(a, b) == N.E_UNSUPPORTED


def test_multi_declines_mismatched_kernels():
    from zarr_hip import _native as N

    p = _plan()
    # other instantiations of k_decode_il: item size, byte swap, the affine form
    assert _check(_args(p, 0), _args(_plan(itemsize=8), 1)) == N.E_UNSUPPORTED
    assert _check(_args(p, 0), _args(_plan(swap=True), 1)) == N.E_UNSUPPORTED
    assert _check(_args(p, 0), _args(p, 1, whole=False)) == N.E_UNSUPPORTED
    assert _check(_args(p, 0, whole=False), _args(p, 1, whole=False)) == 0
    # an entry that alone would take another kernel: 33 units per chunk (k_decode_duo), 96 KiB chunks
    # (k_decode_pair).  (The small-launch kernels' tables are built at upload: a launch of at most 512
    # units is declined on the device, tests/test_gpu_fused_launch.py.)
    assert _check(_args(p, 0), _args(_plan(chunk_bytes=33 << 15), 1)) == N.E_UNSUPPORTED
    assert _check(_args(p, 0), _args(_plan(chunk_bytes=3 << 15), 1, n_chunks=400)) == N.E_UNSUPPORTED
    # an entry's own argument errors come back as zhip_decode_mapped's
    bad = _args(p, 1)
    bad.d_sels = None
    assert _check(_args(p, 0), bad) == N.E_INVALID
    empty = _args(p, 1, n_chunks=0)
    assert _check(_args(p, 0), empty) == N.E_UNSUPPORTED
