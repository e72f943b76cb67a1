// Per-index arithmetic of zhip_axis_last / zhip_axis_count / zhip_axis_fill
// (include/zarrhip.h, "device-planned orthogonal axes"), shared by the device
// kernels (axis.hip) and the CPU test hook zhip_emulate_axis (capi.cpp): both
// locate every index with axis_locate and form its pair with axis_pair.
#pragma once
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zhip_gf2.h"

namespace zhip {

constexpr uint32_t kAxisThreads = 256;
constexpr uint32_t kAxisPer = ZHIP_AXIS_RUN / kAxisThreads;  // indices per lane, kAxisThreads apart
constexpr uint32_t kAxisLdsBins = ZHIP_AXIS_LDS_BINS;        // axes of up to this many chunks: LDS histogram

// One index x of an axis of length g.length: wraps a negative index
// (wraparound_indices), range-checks it (boundscheck_indices) and, in range,
// gives the wrapped index v, its chunk c = v / chunk (< g.grid) and its index
// inside the chunk r = v - c * chunk (< g.chunk).  Returns false for an index
// out of range (v, c, r are then unspecified).
ZHIP_HD bool axis_locate(const zhip_axis_geom& g, int64_t x, uint32_t& v, uint32_t& c, uint32_t& r) {
    const int64_t n = (int64_t)g.length;
    if (x < 0) x += n;
    if (x < 0 || x >= n) return false;
    v = (uint32_t)x;  // < 2^31: the magic division holds
    c = fdiv_apply(v, g.div.m, g.div.s);
    r = v - c * g.chunk;
    return true;
}

// The (A, B) pair of index k whose in-chunk index is r (zhip_select_copy's
// table form): read A = r * slot_stride, B = k * lin_stride (the out side);
// write A = k * lin_stride (the value side, 0 for a scalar), B = r * slot_stride.
ZHIP_HD void axis_pair(const zhip_axis_geom& g, uint64_t k, uint32_t r, int64_t& A, int64_t& B) {
    const int64_t lin = (int64_t)k * g.lin_stride;
    const int64_t off = (int64_t)r * g.slot_stride;
    A = g.write ? lin : off;
    B = g.write ? off : lin;
}

// The bounds words: lo_w[c] = max(chunk - 1 - r), hi_w[c] = max(r) over the
// counted indices of chunk c, so that ONE zero-filled buffer serves both (an
// atomic max onto zero).  lo = chunk - 1 - lo_w, hi = hi_w; both are defined
// only where counts[c] > 0.
ZHIP_HD uint32_t axis_lo_word(const zhip_axis_geom& g, uint32_t r) { return g.chunk - 1u - r; }

// axis.hip; 0 or a hipError_t
int axis_last_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, uint32_t* d_last, void* stream);
int axis_count_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, const uint32_t* d_last,
                      uint32_t* d_counts, uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_err, void* stream);
int axis_fill_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, const uint32_t* d_last,
                     const uint32_t* d_first, uint32_t* d_cursor, int64_t* d_table, uint64_t table_pairs,
                     void* stream);

}  // namespace zhip
