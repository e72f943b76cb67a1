"""k_points_count / k_points_fill driven at the C ABI (zhip_points_count /
zhip_points_fill) over the named cases of points_cases.py, compared with the
CPU hook the way test_points_plan.py compares the hook with the host route:
equal counts, cursor == counts, and per touched chunk equal multisets of
pairs.  counts, cursor and the table sit between sentinel words that must
come back untouched.  Both counter forms run: grids of 1, 640 and exactly
ZHIP_POINTS_LDS_BINS chunks (the LDS histogram), ZHIP_POINTS_LDS_BINS + 1 (one
global atomic per point).  Every buffer is valid memory throughout."""

import ctypes

import numpy as np
import pytest

import points_cases as PC
from zarr_hip import _native as N

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel words on either side
S32 = 0x5EA1ED
S64 = -0x5EA1ED5EA1ED


def run_device(case: PC.Case, device, fill: bool = True):
    """(counts, error word, cursor, table) from the kernels, sentinels checked."""
    import torch

    nc, n = case.n_chunks, case.n
    g = case.geom()
    coords = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64)).to(device) for c in case.coords]
    ptrs = (ctypes.c_void_p * len(coords))(*[c.data_ptr() for c in coords])
    words = torch.full((2 * (nc + 2 * GUARD) + 1 + 2 * GUARD,), S32, dtype=torch.int32, device=device)
    at_counts, at_cursor = GUARD, nc + 3 * GUARD
    at_err = 2 * (nc + 2 * GUARD) + GUARD
    words[at_counts:at_counts + nc] = 0
    words[at_cursor:at_cursor + nc] = 0
    words[at_err] = 0
    table = torch.full((max(n, 1) + 2 * GUARD, 2), S64, dtype=torch.int64, device=device)
    assert (table.data_ptr() + 16 * GUARD) % 16 == 0
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    base = words.data_ptr()
    N.check(N.lib().zhip_points_count(g.ctypes.data, ptrs, n, base + 4 * at_counts, base + 4 * at_err, stream),
            "zhip_points_count")
    if n:
        assert N.lib().zhip_last_kernel() == b"k_points_count"
    host = words.cpu().numpy().view(np.uint32)
    counts, err = host[at_counts:at_counts + nc].copy(), int(host[at_err])
    if fill and not err:
        first = np.cumsum(counts, dtype=np.int64) - counts
        d_first = torch.from_numpy(first.astype(np.uint32).view(np.int32)).to(device)
        N.check(N.lib().zhip_points_fill(g.ctypes.data, ptrs, n, d_first.data_ptr(), base + 4 * at_cursor,
                                         table.data_ptr() + 16 * GUARD, stream), "zhip_points_fill")
        if n:
            assert N.lib().zhip_last_kernel() == b"k_points_fill"
    torch.cuda.synchronize(device)
    host = words.cpu().numpy().view(np.uint32)
    keep = np.ones(host.size, bool)
    keep[at_counts:at_counts + nc] = keep[at_cursor:at_cursor + nc] = False
    keep[at_err] = False
    assert (host[keep] == S32).all(), "a sentinel word next to counts / cursor / the error word changed"
    assert np.array_equal(host[at_counts:at_counts + nc], counts)  # the fill leaves counts alone
    t = table.cpu().numpy()
    assert (t[:GUARD] == S64).all() and (t[GUARD + n:] == S64).all(), "a sentinel pair next to the table changed"
    return counts, err, host[at_cursor:at_cursor + nc].copy(), t[GUARD:GUARD + max(n, 1)].copy()


@pytest.mark.parametrize("name", [k for k, c in PC.CASES.items() if not c.err])
def test_kernels_match_the_hook(name, device):
    case = PC.CASES[name]
    h_counts, h_err, h_first, h_cursor, h_table = PC.run_hook(case)
    counts, err, cursor, table = run_device(case, device)
    assert err == 0 and h_err == 0
    assert np.array_equal(counts, h_counts)
    assert np.array_equal(cursor, counts)
    got, want = PC.chunk_pairs(table, h_first, counts), PC.chunk_pairs(h_table, h_first, h_counts)
    assert sorted(got) == sorted(want)
    for r in want:
        assert np.array_equal(got[r], want[r]), (name, r)
    if case.n == 0:
        assert (table == S64).all()


@pytest.mark.parametrize("name", [k for k, c in PC.CASES.items() if c.err])
def test_out_of_range_points_on_the_device(name, device):
    """The error bits are exactly the failing dimensions'; the out-of-range
    points are counted nowhere (counts equal the hook's, which holds the valid
    points only -- all zero where every point fails)."""
    case = PC.CASES[name]
    h_counts, h_err, *_ = PC.run_hook(case)
    counts, err, cursor, table = run_device(case, device)
    assert err == case.err == h_err
    assert np.array_equal(counts, h_counts)
    if case.n == 1:
        assert not counts.any()
    assert not cursor.any() and (table == S64).all()


def test_the_fill_skips_out_of_range_points(device):
    """zhip_points_fill given a list with out-of-range points (the Python route
    raises before it; the kernel's own guard): the valid points' pairs are
    written, with first built from the valid counts, and nothing else."""
    import torch

    case = PC.CASES["oob-among-valid"]
    bad = np.zeros(case.n, bool)
    for c, s in zip(case.coords, case.shape):
        bad |= (c < -s) | (c >= s)
    good = PC.Case(case.shape, case.chunks, tuple(c[~bad] for c in case.coords))
    counts, err, _, _ = run_device(case, device, fill=False)
    assert err == case.err and counts.sum() == good.n
    g = case.geom()
    coords = [torch.from_numpy(np.ascontiguousarray(c)).to(device) for c in case.coords]
    ptrs = (ctypes.c_void_p * 3)(*[c.data_ptr() for c in coords])
    first = (np.cumsum(counts, dtype=np.int64) - counts).astype(np.uint32)
    d_first = torch.from_numpy(first.view(np.int32)).to(device)
    cursor = torch.zeros(case.n_chunks, dtype=torch.int32, device=device)
    table = torch.full((case.n, 2), S64, dtype=torch.int64, device=device)
    N.check(N.lib().zhip_points_fill(g.ctypes.data, ptrs, case.n, d_first.data_ptr(), cursor.data_ptr(),
                                     table.data_ptr(), int(torch.cuda.current_stream(device).cuda_stream)),
            "zhip_points_fill")
    torch.cuda.synchronize(device)
    t = table.cpu().numpy()
    assert np.array_equal(cursor.cpu().numpy().view(np.uint32), counts)
    assert (t[good.n:] == S64).all()
    # B = k * stride names the point: exactly the valid points, each once
    assert np.array_equal(np.sort(t[:good.n, 1]), np.nonzero(~bad)[0] * case.stride)
