"""k_axis_last / k_axis_count / k_axis_fill driven at the C ABI (zhip_axis_last /
zhip_axis_count / zhip_axis_fill) over the named cases of axis_cases.py,
compared with the CPU hook the way test_axis_plan.py compares the hook with
the host route: equal counts, bounds, last and cursor == counts, and per
touched chunk equal multisets of pairs.  counts, lo / hi, last, cursor and the
table sit between sentinel words that must come back untouched.  Both counter
forms run: axes of 1 .. ZHIP_AXIS_LDS_BINS chunks (the LDS histogram) and of
ZHIP_AXIS_LDS_BINS + 1 and more (global atomics per index).  Every buffer is
valid memory throughout."""

import numpy as np
import pytest

import axis_cases as AC
from zarr_hip import _native as N

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel words on either side
S32 = 0x5EA1ED
S64 = -0x5EA1ED5EA1ED


def run_device(case: AC.Case, device, fill: bool = True):
    """(counts, lo words, hi, error word, cursor, last, table) from the
    kernels, sentinels checked."""
    import torch

    G, L, n = case.grid, case.length, case.n
    g = case.geom()
    x = torch.from_numpy(np.ascontiguousarray(case.x, dtype=np.int64)).to(device)
    # [guard counts guard lo guard hi guard cursor guard err guard last guard]
    at, regions = GUARD, {}
    for name, size in (("counts", G), ("lo", G), ("hi", G), ("cursor", G), ("err", 1), ("last", L)):
        regions[name] = (at, size)
        at += size + GUARD
    words = torch.full((at,), S32, dtype=torch.int32, device=device)
    for a, size in regions.values():
        words[a:a + size] = 0
    pairs = max(case.table_pairs, 1)
    table = torch.full((pairs + 2 * GUARD, 2), S64, dtype=torch.int64, device=device)
    assert (table.data_ptr() + 16 * GUARD) % 16 == 0
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    base = words.data_ptr()

    def p(name):
        return base + 4 * regions[name][0]

    last = p("last") if case.keep_last else None
    if case.keep_last:
        N.check(N.lib().zhip_axis_last(g.ctypes.data, x.data_ptr(), n, last, stream), "zhip_axis_last")
        if n:
            assert N.lib().zhip_last_kernel() == b"k_axis_last"
    N.check(N.lib().zhip_axis_count(g.ctypes.data, x.data_ptr(), n, last, p("counts"), p("lo"), p("hi"), p("err"),
                                    stream), "zhip_axis_count")
    if n:
        assert N.lib().zhip_last_kernel() == b"k_axis_count"
    host = words.cpu().numpy().view(np.uint32)

    def get(h, name):
        a, size = regions[name]
        return h[a:a + size].copy()

    counts, err = get(host, "counts"), int(get(host, "err")[0])
    if fill and not err:
        first = np.cumsum(counts, dtype=np.int64) - counts
        d_first = torch.from_numpy(first.astype(np.uint32).view(np.int32)).to(device)
        N.check(N.lib().zhip_axis_fill(g.ctypes.data, x.data_ptr(), n, last, d_first.data_ptr(), p("cursor"),
                                       table.data_ptr() + 16 * GUARD, case.table_pairs, stream), "zhip_axis_fill")
        if n:
            assert N.lib().zhip_last_kernel() == b"k_axis_fill"
    torch.cuda.synchronize(device)
    before, host = host, words.cpu().numpy().view(np.uint32)
    keep = np.ones(host.size, bool)
    for a, size in regions.values():
        keep[a:a + size] = False
    assert (host[keep] == S32).all(), "a sentinel word next to counts / lo / hi / cursor / err / last changed"
    for name in ("counts", "lo", "hi", "err", "last"):  # the fill leaves them alone
        assert np.array_equal(get(host, name), get(before, name)), name
    t = table.cpu().numpy()
    assert (t[:GUARD] == S64).all() and (t[GUARD + pairs:] == S64).all(), "a sentinel pair next to the table changed"
    return (counts, get(host, "lo"), get(host, "hi"), err, get(host, "cursor"), get(host, "last"),
            t[GUARD:GUARD + pairs].copy())


@pytest.mark.parametrize("name", [k for k, c in AC.CASES.items() if not c.err])
def test_kernels_match_the_hook(name, device):
    case = AC.CASES[name]
    h_counts, h_lo, h_hi, h_err, h_first, h_cursor, h_table, h_last = AC.run_hook(case)
    counts, low, hi, err, cursor, last, table = run_device(case, device)
    assert err == 0 and h_err == 0
    assert np.array_equal(counts, h_counts)
    assert np.array_equal(cursor, counts)
    touched = counts > 0  # lo / hi are defined only there
    assert np.array_equal((case.chunk - 1 - low.astype(np.int64))[touched], h_lo[touched])
    assert np.array_equal(hi[touched], h_hi[touched])
    assert not low[~touched].any() and not hi[~touched].any()
    if case.keep_last:
        assert np.array_equal(last, h_last)  # independent of scheduling
    else:
        assert not last.any()
    got = AC.chunk_pairs(table, case.table_off, h_first, counts)
    want = AC.chunk_pairs(h_table, case.table_off, h_first, h_counts)
    assert sorted(got) == sorted(want)
    for c in want:
        assert np.array_equal(got[c], want[c]), (name, c)
    used = case.table_off + int(counts.sum())
    assert (table[:case.table_off] == S64).all() and (table[used:] == S64).all()


@pytest.mark.parametrize("name", [k for k, c in AC.CASES.items() if c.err])
def test_out_of_range_indices_on_the_device(name, device):
    """The error word is exactly the axis' bit; the out-of-range indices are
    counted nowhere (counts and bounds equal the hook's, which holds the valid
    indices only -- all zero where every index fails)."""
    case = AC.CASES[name]
    h_counts, h_lo, h_hi, h_err, *_ = AC.run_hook(case)
    counts, low, hi, err, cursor, last, table = run_device(case, device)
    assert err == case.err == h_err
    assert np.array_equal(counts, h_counts)
    touched = counts > 0
    assert np.array_equal((case.chunk - 1 - low.astype(np.int64))[touched], h_lo[touched])
    assert np.array_equal(hi[touched], h_hi[touched])
    if case.n == 1:  # every array but the error word untouched
        assert not counts.any() and not low.any() and not hi.any() and not last.any()
    assert not cursor.any() and (table == S64).all()


def test_the_fill_skips_out_of_range_indices_and_stays_inside_a_short_table(device):
    """zhip_axis_fill given a list with out-of-range indices (the Python route
    raises before it; the kernel's own guard): the valid indices' pairs are
    written, with first built from the valid counts, and nothing else.  Then
    the same fill told the table is shorter than it is: no pair at or past
    that length is written."""
    import torch

    case = AC.CASES["oob-among-valid"]
    bad = (case.x < -case.length) | (case.x >= case.length)
    n_good = int((~bad).sum())
    counts, _, _, err, _, _, _ = run_device(case, device, fill=False)
    assert err == case.err and counts.sum() == n_good
    g = case.geom()
    x = torch.from_numpy(np.ascontiguousarray(case.x)).to(device)
    first = (np.cumsum(counts, dtype=np.int64) - counts).astype(np.uint32)
    d_first = torch.from_numpy(first.view(np.int32)).to(device)
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    for pairs in (case.n, n_good - 100):
        cursor = torch.zeros(case.grid, dtype=torch.int32, device=device)
        table = torch.full((case.n, 2), S64, dtype=torch.int64, device=device)
        N.check(N.lib().zhip_axis_fill(g.ctypes.data, x.data_ptr(), case.n, None, d_first.data_ptr(),
                                       cursor.data_ptr(), table.data_ptr(), pairs, stream), "zhip_axis_fill")
        torch.cuda.synchronize(device)
        t = table.cpu().numpy()
        assert np.array_equal(cursor.cpu().numpy().view(np.uint32), counts)
        kept = min(pairs, n_good)
        assert (t[kept:] == S64).all() and (t[:kept] != S64).all()
        if pairs == case.n:  # B = k * stride names the index: exactly the valid ones, each once
            assert np.array_equal(np.sort(t[:n_good, 1]), np.nonzero(~bad)[0] * case.stride)
