// "This item equals the fill value" as NDBuffer.all_equal defines it
// (src/zarr/core/buffer/core.py:534-558), stated once for the encode kernels
// (encode.hip, decode_tile.hip), the value map (zhip_values.h) and the CPU hook
// zhip_emulate_fill_eq (capi.cpp):
//   integers, bool : equal bits;
//   floats         : equal bits (so -0.0 != +0.0 and payloads count), except
//                    that any NaN equals a NaN fill (equal_nan=True);
//   complex64      : np.array_equal(..., equal_nan=True) -- both components
//                    equal as IEEE values (-0.0 == +0.0, NaN != NaN), or the
//                    fill is NaN in either component and so is the item.
// Items and fills are native-order bit patterns; `fill_nan` is fill_is_nan()
// of the fill, computed once per launch.
#pragma once
#include <stdint.h>

#include "zhip_gf2.h"

namespace zhip {

// ITEM-byte IEEE pattern is a NaN (ITEM 2, 4, 8; false for ITEM 1)
template <int ITEM>
ZHIP_HD bool bits_nan(uint64_t x) {
    if constexpr (ITEM == 2) return ((uint32_t)x & 0x7FFFu) > 0x7C00u;
    else if constexpr (ITEM == 4) return ((uint32_t)x & 0x7FFFFFFFu) > 0x7F800000u;
    else if constexpr (ITEM == 8) return (x & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
    else return false;
}

// two float32 patterns equal as IEEE values
ZHIP_HD bool f32_value_eq(uint32_t a, uint32_t b) {
    if (bits_nan<4>(a) || bits_nan<4>(b)) return false;
    return a == b || ((a | b) & 0x7FFFFFFFu) == 0u;
}

// the fill's `fill_nan` word: is_float -- ZHIP_LF_FLOAT, is_cplx -- ZHIP_LF_COMPLEX
inline bool fill_is_nan(int item, bool is_float, bool is_cplx, uint32_t lo, uint32_t hi) {
    if (is_cplx) return item == 8 && (bits_nan<4>(lo) || bits_nan<4>(hi));
    if (!is_float) return false;
    if (item == 2) return bits_nan<2>(lo);
    if (item == 4) return bits_nan<4>(lo);
    if (item == 8) return bits_nan<8>(((uint64_t)hi << 32) | lo);
    return false;
}

// One item (lo, and hi for ITEM == 8; bits above the item ignored) against
// the fill (f_lo, f_hi).  CPLX: an 8-byte item of two float32 (lo = real).
template <int ITEM, bool CPLX = false>
ZHIP_HD bool item_eq_fill_bits(uint32_t lo, uint32_t hi, uint32_t f_lo, uint32_t f_hi, uint32_t fill_nan) {
    if constexpr (ITEM == 8 && CPLX) {
        if (f32_value_eq(lo, f_lo) && f32_value_eq(hi, f_hi)) return true;
        return fill_nan && (bits_nan<4>(lo) || bits_nan<4>(hi));
    } else if constexpr (ITEM == 8) {
        const bool eq = lo == f_lo && hi == f_hi;
        if (!fill_nan) return eq;
        return eq || bits_nan<8>(((uint64_t)hi << 32) | lo);
    } else {
        constexpr uint32_t mask = ITEM == 4 ? 0xFFFFFFFFu : ((1u << (8 * ITEM)) - 1u);
        const bool eq = (lo & mask) == (f_lo & mask);
        if (!fill_nan) return eq;
        return eq || bits_nan<ITEM>(lo & mask);
    }
}

// The items of one 16-byte block (native order) whose first byte lies below
// `valid`; fill = the fill pattern replicated to 16 bytes.
template <int ITEM, bool CPLX = false>
ZHIP_HD bool block_eq_fill_bits(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t valid,
                                const uint32_t* fill, uint32_t fill_nan) {
    const uint32_t w[4] = {w0, w1, w2, w3};
    bool all = true;
    constexpr int kItems = 16 / ITEM;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if ((uint32_t)(j * ITEM) >= valid) break;
        uint32_t lo, hi = 0;
        if constexpr (ITEM == 8) {
            lo = w[2 * j];
            hi = w[2 * j + 1];
        } else {
            lo = w[(j * ITEM) / 4] >> (8 * ((j * ITEM) % 4));
        }
        all = all && item_eq_fill_bits<ITEM, CPLX>(lo, hi, fill[0], fill[1], fill_nan);
    }
    return all;
}

}  // namespace zhip
