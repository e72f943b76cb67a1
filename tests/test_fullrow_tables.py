"""CPU checks of the full-row form of k_decode_il (decode_rows.hip ilx_body):
lane l of span group r runs ONE A_1024 Horner chain through the 8 P blocks of
P consecutive 8 KiB spans and ends on the group's last span, so its lane
constant is k_decode_xw's of that span.  The emulator
(zhip_emulate_chunk_crc_ilx) runs the exact decomposition on the host with the
tables the plan uploads."""

import numpy as np
import pytest

from oracle import oracle as O

# 512 KiB (C5's inner chunk), 1 MiB (the headline's), 1004 KiB (251 steps of
# 4 KiB: no multiple of 8 KiB, so the first span starts before the chunk and
# its leading blocks are zero blocks), 1000 KiB (ragged by six steps) and a
# length that is no multiple of 16 bytes
SIZES = [524288, 1048576, 1028096, 1024000, 262144 + 4100]
SPANS = [1, 2, 4]  # the decode takes 4; 2 is the other count the design weighed; 1 is k_decode_xw's scheme


def _plan(n):
    from zarr_hip import _native as N

    L = N.Layout()
    L.ndim, L.itemsize = 1, 1
    L.shape[0] = n
    L.nbytes = n
    L.flags = N.LF_CRC
    return N.Plan(L, upload=False)


@pytest.mark.parametrize("spans", SPANS)
@pytest.mark.parametrize("n", SIZES)
def test_emulated_fullrow_crc_matches_oracle(n, spans):
    rng = np.random.default_rng(n)
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    plan = _plan(n)
    assert plan.units_per_chunk * 4 % spans == 0  # 8 KiB spans per chunk = 4 per 32 KiB unit
    assert plan.emulate_chunk_crc_fullrow(data, spans) == O.crc32c(data)


@pytest.mark.parametrize("n", SIZES)
def test_one_span_groups_are_the_xw_scheme(n):
    """Where the two schemes coincide (groups of one span) the full-row form
    is k_decode_xw's decomposition: the same tables and lane constants."""
    rng = np.random.default_rng(n + 1)
    data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    plan = _plan(n)
    assert plan.emulate_chunk_crc_fullrow(data, 1) == plan.emulate_chunk_crc(data, pair="xw")


def test_a_flipped_bit_in_any_pass_changes_the_crc():
    """One bit in the first and in the last 16 bytes of each span of one
    group of four: the emulated CRC follows the plain one."""
    n = 1048576
    plan = _plan(n)
    base = bytearray(np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes())
    for span in range(4 * 7, 4 * 8):
        for at in (8192 * span + 3, 8192 * span + 8192 - 5):
            b = bytearray(base)
            b[at] ^= 0x20
            got = plan.emulate_chunk_crc_fullrow(bytes(b), 4)
            assert got == O.crc32c(bytes(b)) != O.crc32c(bytes(base))


def test_the_wide_row_of_the_gpu_test_has_its_property_and_is_safe():
    """tests/test_gpu_fullrow_order.py reads wide_cases' il geometry with 20
    slabs (a multiple of four, so the full-row form takes it).  As
    tests/test_wide_offsets.py proves for wide_cases' own rows: a slab
    straddles 2**31 and one 2**32 as single runs, the missing slab lies above
    2**32, blob 1 / blob 2 straddle the boundaries in the arena -- and every
    way a partial sum of any address can lose its high bits still lands inside
    the backing, the un-narrowed ones inside the body."""
    import wide_cases as W

    row = W.READ["il"]._replace(id="il_fullrow", n=20)
    ranges = W.dest_ranges(row)
    assert max(b for _, b in ranges) > W.B32
    assert any(a < W.B31 < b for a, b in ranges) and any(a < W.B32 < b for a, b in ranges)
    last = [r for d, r in zip(W.dest_chunks(row), W.chunk_ranges(row)) if d.cell == W.dropped(row)]
    assert last and all(a >= W.B32 for r in last for a, _ in r)
    place = W.read_placements(row)
    blobs = sorted(place.values())
    assert blobs[0][0] + blobs[0][1] < W.B31
    assert blobs[1][0] < W.B31 < sum(blobs[1]) and blobs[2][0] < W.B32 < sum(blobs[2])
    assert all(o > W.B32 for o, _ in blobs[3:])
    for d in W.dest_chunks(row):
        assert W.inside(W.narrowed_dest(d), row.base)
        assert row.base + d.out_off + int(d.starts.min()) >= 0
        assert row.base + d.out_off + int(d.starts.max()) + d.run <= W.BODY
    for _, _, a, b in W.src_ranges(row, place, None):
        assert W.inside(W.narrowed_src(a, b))
        assert a >= 0 and b + W.SLACK <= W.BODY


def test_span_counts_that_do_not_tile_are_declined():
    assert _plan(1048576).emulate_chunk_crc_fullrow(b"\0" * 1048576, 3) == 0xFFFFFFFF
    assert _plan(1048576).emulate_chunk_crc_fullrow(b"\0" * 1048576, 0) == 0xFFFFFFFF
