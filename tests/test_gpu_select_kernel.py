"""k_select_copy driven at the C ABI with hand-built tables (select_cases.py,
the cases test_select_kernel.py proves against the CPU hook): plain torch
tensors for the tables and buffers, torch's current stream, byte for byte
against the numpy reference over the WHOLE of b -- every case pre-fills b with
a sentinel, so a store to a byte no element selects fails too.

On the device only: the largest item (2**31 - 32768 - 1 elements, 2**21 tiles)
and byte offsets at and beyond 2**32.  These allocate 2 and 8 GiB and skip
only when the device reports less than 16 GiB free."""

import numpy as np
import pytest

import select_cases as S
from zarr_hip import _native as N

pytestmark = pytest.mark.gpu

GiB = 1 << 30


def _launch(tables, a_ptr, a_size, b_ptr, b_size, isz, device):
    """One zhip_select_copy on torch's current stream; synchronised."""
    import torch

    up = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(device)
          for x in (tables.items, tables.table, tables.prefix)]
    stream = int(torch.cuda.current_stream(device).cuda_stream)
    N.check(N.lib().zhip_select_copy(up[0].data_ptr(), len(tables.items), up[1].data_ptr(), up[2].data_ptr(),
                                     tables.n_tiles, a_ptr, a_size, b_ptr, b_size, isz, stream), "zhip_select_copy")
    assert N.lib().zhip_last_kernel() == b"k_select_copy"
    torch.cuda.synchronize(device)
    del up


def run_device(case: S.Case, device) -> tuple:
    """(b after the kernel, the expected b) as host byte arrays.  The
    reference runs first: it also checks that every offset of the case lies
    inside the allocations, so nothing unchecked reaches the device."""
    import torch

    a, sent = case.source(), case.sentinel()
    want = case.expected(a, sent)
    da, db = torch.from_numpy(a).to(device), torch.from_numpy(sent).to(device)
    assert da.data_ptr() % 8 == 0 and db.data_ptr() % 8 == 0
    _launch(case.tables(), da.data_ptr() + case.ptr_off, case.a_size, db.data_ptr() + case.ptr_off, case.b_size,
            case.itemsize, device)
    return db.cpu().numpy(), want


@pytest.mark.parametrize("isz", S.ITEMSIZES)
@pytest.mark.parametrize("name", list(S.HOST_CASES))
def test_kernel_matches_the_reference(name, isz, device):
    case = S.HOST_CASES[name](isz)
    got, want = run_device(case, device)
    assert got.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("isz", S.ITEMSIZES)
@pytest.mark.parametrize("name", list(S.FENCE_CASES))
def test_the_fence_copies_exactly_the_inside_elements(name, isz, device):
    """Declared sizes smaller than the allocations, pointers 4096 bytes in:
    elements before the pointer and at or past the declared size are skipped
    (their bytes keep the sentinel), the element that ends at the declared
    size is copied.  Every offset lies inside the real allocation."""
    case = S.FENCE_CASES[name](isz)
    got, want = run_device(case, device)
    assert got.tobytes() == want.tobytes(), name


def _need_free(device, what):
    import torch

    free, _ = torch.cuda.mem_get_info(device)
    if free < 16 * GiB:
        pytest.skip(f"{what}: torch.cuda.mem_get_info reports {free / GiB:.1f} GiB free on the device, "
                    "less than the 16 GiB below which the multi-GiB select cases may skip")


@pytest.mark.parametrize("cols", [65537, 3, 7, 255, 257, 641, 1023, 1025, 4097])
def test_the_largest_item(cols, device):
    """uint8, dimensions (rows, cols) with rows = (2**31 - 1) // cols -- for
    65537 that is (32767, 65537): 2 147 450 879 elements, element numbers up
    to 2**31 - 32770 through the division by 65537 and
    (tile - prefix) * 1024 + lane at 2 097 120 tiles.  a is one row of cols
    bytes (sa = 0 on the outer dimension), B = k0 * cols + k1: every row of b
    becomes a, and the 4096 sentinel bytes behind them stay.  With the other
    inner counts this is the device's quotient and remainder at EVERY element
    number the item form admits, for the divisors next to a power of two."""
    import torch

    _need_free(device, "the largest item")
    rows = ((1 << 31) - 1) // cols
    total = rows * cols
    assert (1 << 31) - cols <= total < 1 << 31 and (cols != 65537 or (rows, total) == (32767, 2147450879))
    it = S.item([("affine", rows, 0, 0, 0, cols), ("affine", cols, 0, 1, 0, 1)])
    t = S.build_tables([it])
    assert t.n_tiles == -(-total // S.T) and (cols != 65537 or t.n_tiles == 2097120)
    a = np.random.default_rng(5).integers(0, 256, cols, dtype=np.uint8)
    a[1:] += a[1:] == a[:-1]  # neighbours differ: a remainder off by one shows
    da = torch.from_numpy(a).to(device)
    tail = torch.from_numpy(S.sentinel(4096, total)).to(device)
    db = torch.empty(total + 4096, dtype=torch.uint8, device=device)
    db[:total].fill_(0xA5)
    db[total:] = tail
    _launch(t, da.data_ptr(), cols, db.data_ptr(), total + 4096, 1, device)  # the last offset is total - 1
    same = bool((db[:total].view(rows, cols) == da).all())
    tail_kept = torch.equal(db[total:], tail)
    del db
    torch.cuda.empty_cache()
    assert same and tail_kept


HI = 1 << 32
WIN = 1 << 20


def _wide_buffers(device):
    """a and b of 2**32 + 2**20 bytes; only the windows [0, 2**20) and
    [2**32, 2**32 + 2**20) are initialised: a's two windows with different
    data, b's with the sentinel."""
    import torch

    rng = np.random.default_rng(77)
    a_lo, a_hi = (rng.integers(0, 256, WIN, dtype=np.uint8) for _ in range(2))
    assert (a_lo != a_hi).mean() > 0.9
    s_lo, s_hi = S.sentinel(WIN), S.sentinel(WIN, HI)
    da = torch.empty(HI + WIN, dtype=torch.uint8, device=device)
    db = torch.empty(HI + WIN, dtype=torch.uint8, device=device)
    da[:WIN] = torch.from_numpy(a_lo).to(device)
    da[HI:] = torch.from_numpy(a_hi).to(device)
    return da, db, a_lo, a_hi, s_lo, s_hi


@pytest.fixture(scope="module")
def wide(device):
    _need_free(device, "offsets beyond 2**32")
    import torch

    bufs = _wide_buffers(device)
    yield bufs
    del bufs
    torch.cuda.empty_cache()  # 8 GiB go back to the device, not to the suite's cache


def _check_wide(device, wide, it, lo_pairs, hi_pairs):
    """Run `it` (item size 4) on the wide buffers; expected: the (ao, bo) byte
    pairs of lo_pairs copied inside the low windows, of hi_pairs inside the
    high windows (offsets relative to the window)."""
    import torch

    da, db, a_lo, a_hi, s_lo, s_hi = wide
    db[:WIN] = torch.from_numpy(s_lo).to(device)
    db[HI:] = torch.from_numpy(s_hi).to(device)
    _launch(S.build_tables([it]), da.data_ptr(), HI + WIN, db.data_ptr(), HI + WIN, 4, device)
    lane = np.arange(4, dtype=np.int64)
    for (ao, bo), a_w, s_w, win in ((lo_pairs, a_lo, s_lo, db[:WIN]), (hi_pairs, a_hi, s_hi, db[HI:])):
        want = s_w.copy()
        if ao is not None:
            want[bo[:, None] + lane] = a_w[ao[:, None] + lane]
        assert win.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("form", ["table-entries", "bases", "stride-product"])
def test_offsets_beyond_4gib(form, device, wide):
    """Item size 4, buffers of 2**32 + 2**20 bytes.  The high window of b gets
    the high window's data and the low window of b keeps its sentinel (for
    the stride product: gets the k = 0 elements only); address arithmetic
    truncated to 32 bits lands in the low windows and shows as wrong bytes."""
    rng = np.random.default_rng(78)
    n = 3000
    src = rng.permutation(WIN // 4)[:n].astype(np.int64) * 4
    dst = rng.permutation(WIN // 4)[:n].astype(np.int64) * 4
    if form == "table-entries":
        it = S.item([("table", n, src + HI, dst + HI)])
    elif form == "bases":
        it = S.item([("table", n, src, dst)], a_base=HI, b_base=HI)
    else:
        # an outer affine dimension of count 3 with sa = sb = 2**31 + 4096 over an inner table of small offsets:
        # row k = 0 lies in the low windows, k = 1 at 2**31 + 4096 (inside the allocations, uninitialised and
        # not compared), k = 2 at 2**32 + 8192: past 2**32 by the product k * s alone.  The inner entries
        # stay below 2**20 - 8192, so row 2 stays inside the high windows.
        s = (1 << 31) + 4096
        m = 1000
        inner = (WIN - 8192) // 4
        src, dst = (rng.permutation(inner)[:m].astype(np.int64) * 4 for _ in range(2))
        it = S.item([("affine", 3, 0, s, 0, s), ("table", m, src, dst)])
    ao, bo = S.reference_offsets(it)
    assert np.unique(bo).size == bo.size
    assert ao.min() >= 0 and bo.min() >= 0  # every offset inside the allocations, before anything is launched
    assert ao.max() >= HI and bo.max() >= HI and ao.max() + 4 <= HI + WIN and bo.max() + 4 <= HI + WIN
    in_lo, in_hi = (ao < WIN), (ao >= HI)
    assert ((bo < WIN) == in_lo).all() and ((bo >= HI) == in_hi).all()
    if form == "stride-product":
        assert in_lo.sum() == in_hi.sum() == m and (~(in_lo | in_hi)).sum() == m  # the middle row: not compared
        lo_p = (ao[in_lo], bo[in_lo])
    else:
        assert in_hi.all()
        lo_p = (None, None)
    _check_wide(device, wide, it, lo_p, (ao[in_hi] - HI, bo[in_hi] - HI))
