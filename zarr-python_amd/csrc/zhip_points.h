// Per-point arithmetic of zhip_points_count / zhip_points_fill
// (include/zarrhip.h, "device-built point tables"), shared by the device
// kernels (points.hip) and the CPU test hook zhip_emulate_points (capi.cpp):
// both locate every point with points_locate and form its pair with
// points_pair.
#pragma once
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zhip_gf2.h"

namespace zhip {

constexpr uint32_t kPointsThreads = 256;
constexpr uint32_t kPointsPer = ZHIP_POINTS_RUN / kPointsThreads;  // points per lane, kPointsThreads apart
constexpr uint32_t kPointsLdsBins = ZHIP_POINTS_LDS_BINS;          // grids up to this many chunks: LDS histogram

// One point x[0 .. ndim): wraps negative indices (CoordinateIndexer's
// wraparound_indices), range-checks every dimension (boundscheck_indices) and,
// for an in-range point, gives the row-major index of its chunk in the chunk
// grid and the byte offset of its element inside a C-order chunk-shaped slot
// whose byte strides are g.slot_stride.  Returns 0, or the OR of (1 << d) over
// the dimensions whose index is out of range (rix / off are then unspecified).
// x is indexed with compile-time subscripts only: it stays in registers.
ZHIP_HD uint32_t points_locate(const zhip_points_geom& g, const int64_t* x, uint32_t& rix, int64_t& off) {
    uint32_t err = 0;
    rix = 0;
    off = 0;
#pragma unroll
    for (int d = 0; d < ZHIP_MAX_DIMS; ++d) {
        if (d < g.ndim) {
            const int64_t n = (int64_t)g.shape[d];
            int64_t v = x[d];
            if (v < 0) v += n;
            if (v < 0 || v >= n) {
                err |= 1u << d;
            } else {
                const uint32_t u = (uint32_t)v;  // < 2^31: the magic division holds
                const uint32_t c = fdiv_apply(u, g.div[d].m, g.div[d].s);
                rix = rix * g.grid[d] + c;
                off += (int64_t)(u - c * g.chunk[d]) * g.slot_stride[d];
            }
        }
    }
    return err;
}

// The (A, B) pair of point k whose slot offset is `off` (zhip_select_copy's
// table form): read A = slot offset, B = k * pair_stride (the out side);
// write A = k * pair_stride (the value side, 0 for a scalar), B = slot offset.
ZHIP_HD void points_pair(const zhip_points_geom& g, uint64_t k, int64_t off, int64_t& A, int64_t& B) {
    const int64_t lin = (int64_t)k * g.pair_stride;
    A = g.write ? lin : off;
    B = g.write ? off : lin;
}

// chunks of the grid (the length of counts / first / cursor); 0 for a
// geometry the entry points refuse
inline uint64_t points_grid_size(const zhip_points_geom& g) {
    if (g.ndim < 1 || g.ndim > ZHIP_MAX_DIMS) return 0;
    uint64_t total = 1;
    for (int d = 0; d < g.ndim; ++d) {
        total *= g.grid[d];
        if (total == 0 || total > ZHIP_POINTS_MAX_GRID) return 0;
    }
    return total;
}

struct PointsCoords {
    const int64_t* c[ZHIP_MAX_DIMS];
};

// points.hip; 0 or a hipError_t
int points_count_launch(const zhip_points_geom& g, const PointsCoords& pc, uint32_t n, uint32_t n_chunks,
                        uint32_t* d_counts, uint32_t* d_err, void* stream);
int points_fill_launch(const zhip_points_geom& g, const PointsCoords& pc, uint32_t n, uint32_t n_chunks,
                       const uint32_t* d_first, uint32_t* d_cursor, int64_t* d_table, void* stream);

}  // namespace zhip
