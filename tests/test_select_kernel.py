"""zhip_select_copy at the ABI, without a GPU: the hand-built tables of
select_cases.py through the CPU hook zhip_emulate_select_copy (the kernel's
tile walk and address arithmetic over host memory), byte for byte against the
numpy reference -- which proves the helper and the cases before a GPU sees
them (test_gpu_select_kernel.py runs the same cases through the kernel); the
magic divisors at the values where one fails; the argument checks that return
before any launch."""

import numpy as np
import pytest

import select_cases as S
from zarr_hip import _native as N


def run_hook(case: S.Case):
    """(rc, b after the hook, a) over host copies of the case's allocations."""
    t = case.tables()
    a, b = case.source(), case.sentinel()
    rc = N.lib().zhip_emulate_select_copy(
        t.items.ctypes.data, len(t.items), t.table.ctypes.data, len(t.table), t.prefix.ctypes.data, t.n_tiles,
        a.ctypes.data + case.ptr_off, case.a_size, b.ctypes.data + case.ptr_off, case.b_size, case.itemsize)
    return rc, b, a


@pytest.mark.parametrize("isz", S.ITEMSIZES)
@pytest.mark.parametrize("name", list(S.HOST_CASES))
def test_hook_matches_the_reference(name, isz):
    case = S.HOST_CASES[name](isz)
    rc, b, a = run_hook(case)
    assert rc == 0, N.lib().zhip_last_error()
    want = case.expected(a, case.sentinel())
    assert b.tobytes() == want.tobytes(), name
    assert (want != case.sentinel()).any()  # the case copies something a sentinel byte does not already hold


@pytest.mark.parametrize("isz", S.ITEMSIZES)
@pytest.mark.parametrize("name", list(S.FENCE_CASES))
def test_hook_reports_bounds_for_the_fenced_tables(name, isz):
    """The CPU twin of the GPU fence cases: the same tables are ZHIP_E_BOUNDS
    to the hook and nothing outside the declared sizes is written."""
    case = S.FENCE_CASES[name](isz)
    rc, b, _ = run_hook(case)
    assert rc == N.E_BOUNDS and b"outside its buffer" in N.lib().zhip_last_error()
    lo, hi = case.ptr_off, case.ptr_off + case.b_size
    sent = case.sentinel()
    assert b[:lo].tobytes() == sent[:lo].tobytes() and b[hi:].tobytes() == sent[hi:].tobytes()
    case.expected(case.source(), sent)  # the case's own invariants (fenced, distinct, inside the allocations)


def test_reference_and_builder_agree_with_a_literal_example():
    """The helper itself on a case small enough to write out: a 2 x 3 item,
    outer affine, inner a table."""
    it = S.item([("affine", 2, 4, 100, 0, -8), ("table", 3, [0, 40, 20], [16, 4, 8])], a_base=1000, b_base=50)
    ao, bo = S.reference_offsets(it)
    assert ao.tolist() == [1004, 1044, 1024, 1104, 1144, 1124]
    assert bo.tolist() == [66, 54, 58, 58, 46, 50]
    t = S.build_tables([it, S.item([("affine", S.T + 1, 0, 1, 0, 1)])])
    assert t.prefix.tolist() == [0, 1, 3] and t.n_tiles == 3 and t.prefix.dtype == np.uint32
    r = t.items[0]
    assert (r["ndim"], r["total"], r["a_base"], r["b_base"]) == (2, 6, 1000, 50)
    assert r["dims"][1]["table"] == 1 and r["dims"][1]["table_off"] == 0 and r["dims"][0]["table"] == 0
    assert tuple(r["dims"][1]["div"]) == N.fdiv(3) and tuple(r["dims"][0]["div"]) == N.fdiv(2)
    assert t.table.tolist() == [[0, 16], [40, 4], [20, 8]] and t.table.dtype == np.int64


# ------------------------------------------------------------------ fdiv
NMAX = (1 << 31) - 1


def _fdiv_divisors():
    rng = np.random.default_rng(2024)
    d = list(S.DIVISORS) + [(1 << 30) - 1, 1 << 30, (1 << 30) + 1, NMAX]
    # seeded random ones, spread over every bit length
    d += [int(x) for x in (rng.integers(1, 1 << 31, 1000))]
    d += [int(rng.integers(1 << (k % 31), 1 << (k % 31 + 1))) for k in range(1000)]
    return [min(x, NMAX) for x in d]


def _fdiv_points(d, rng):
    kmax = NMAX // d
    ks = [0, 1, 2, kmax - 1, kmax] + [int(k) for k in rng.integers(0, kmax + 1, 50)]
    ns = {NMAX}
    for k in ks:
        if k < 0:
            continue
        for n in (k * d - 1, k * d, k * d + 1, k * d + d - 1):
            if 0 <= n <= NMAX:
                ns.add(n)
    return sorted(ns)


def test_fdiv_native_matches_floor_division_at_the_edges():
    """zhip_fdiv_eval(n, d) == n // d for n at k d - 1, k d, k d + 1 and
    k d + d - 1, k in {0, 1, 2, kmax - 1, kmax} and 50 random k, and at
    2**31 - 1: the values where a magic divisor that is one too small or too
    large first shows.  The Python mirror N.fdiv gives the native magic
    numbers."""
    L = N.lib()
    rng = np.random.default_rng(7)
    ev = L.zhip_fdiv_eval
    for d in _fdiv_divisors():
        m, s = N.fdiv(d)
        assert m < 1 << 32
        for n in _fdiv_points(d, rng):
            q = n // d
            assert ev(n, d) == q, (n, d)
            assert (n * m) >> s == q, (n, d)


# ------------------------------------------------------- argument checks
def _args(itemsize=4, items=True, prefix=True, a_off=0, n_tiles=1):
    t = S.build_tables([S.item([("affine", 4, 0, itemsize, 0, itemsize)])])
    a = np.zeros(64, np.uint64)
    b = np.zeros(64, np.uint64)
    keep = (t, a, b)
    return keep, (t.items.ctypes.data if items else None, 1, t.table.ctypes.data, t.prefix.ctypes.data if prefix else None,
                  n_tiles, a.ctypes.data + a_off, 256, b.ctypes.data, 256, itemsize, None)


def test_argument_checks_return_before_any_launch():
    """zhip_select_copy itself, on a machine without a GPU: every call here
    returns from the checks in front of the launch."""
    L = N.lib()

    def err():
        return L.zhip_last_error().decode()

    keep, args = _args(n_tiles=0)
    assert L.zhip_select_copy(*args) == 0
    keep, args = _args(n_tiles=0, items=False, itemsize=3)  # no tiles: nothing else is looked at
    assert L.zhip_select_copy(*args) == 0
    keep, args = _args(itemsize=3)
    assert L.zhip_select_copy(*args) == N.E_UNSUPPORTED and err() == "itemsize must be 1, 2, 4 or 8"
    keep, args = _args(items=False)
    assert L.zhip_select_copy(*args) == N.E_INVALID and err() == "null argument"
    keep, args = _args(prefix=False)
    assert L.zhip_select_copy(*args) == N.E_INVALID and err() == "null argument"
    keep, args = _args(a_off=2)
    assert L.zhip_select_copy(*args) == N.E_INVALID and err() == "a / b not aligned to itemsize"
    keep, args = _args(n_tiles=1 << 31)
    assert L.zhip_select_copy(*args) == N.E_UNSUPPORTED and err() == "too many tiles for one launch"
    # the hook shares select_args
    t, a, b = keep
    assert L.zhip_emulate_select_copy(t.items.ctypes.data, 1, t.table.ctypes.data, 1, t.prefix.ctypes.data, 1,
                                      a.ctypes.data, 256, b.ctypes.data + 1, 256, 2) == N.E_INVALID
    assert err() == "a / b not aligned to itemsize"
    assert L.zhip_emulate_select_copy(t.items.ctypes.data, 1, t.table.ctypes.data, 1, t.prefix.ctypes.data, 1,
                                      a.ctypes.data, 256, b.ctypes.data, 256, 3) == N.E_UNSUPPORTED
    # ... and refuses a table dimension without the pair table
    tt = S.build_tables([S.item([("table", 2, [0, 4], [4, 0])])])
    assert L.zhip_emulate_select_copy(tt.items.ctypes.data, 1, None, 0, tt.prefix.ctypes.data, 1,
                                      a.ctypes.data, 256, b.ctypes.data, 256, 4) == N.E_INVALID
    assert err() == "dimension table range"
    assert not a.any() and not b.any()
