// k_points_count / k_points_fill: the grouped (A, B) pair table of a coordinate
// or mask selection, built on the device from the coordinate arrays
// (zhip_points_count / zhip_points_fill, include/zarrhip.h).  They replace the
// per-point host work of CoordinateIndexer.__init__ (wraparound, bounds check,
// chunk of each point, the grouping argsort) and of the table build; the
// per-point arithmetic is zhip_points.h's, shared with the CPU hook.
//
// Launch shape: one workgroup of 256 lanes per run of ZHIP_POINTS_RUN points;
// lane l takes points l, l + 256, ... of the run, so the int64 coordinate
// loads (one array per dimension) are coalesced.
//
// Counters.  A large point list falls on few chunks (10^6 points on 64
// counters), and adds that share a row serialise.  While the grid has at most
// kPointsLdsBins chunks (LDS = true) a workgroup therefore histograms its run
// in LDS and issues ONE global atomic per non-empty bin: in k_points_fill that
// atomic is a returning add of the bin's count onto cursor[rix], whose result
// is the workgroup's base inside the chunk's range; a lane's rank inside the
// bin is what its LDS atomic returned.  Larger grids (LDS = false) take one
// global atomic per point: that many counters spread the adds by construction.
//
// Stores.  counts / cursor are touched at rix < n_chunks only (points_locate
// range-checks the point in the same call that produces rix); a pair goes to
// table[first[rix] + position] and only when that index is below n, the
// table's length.
#include <hip/hip_runtime.h>

#include "zhip_internal.h"
#include "zhip_points.h"

namespace zhip {

typedef int64_t pair_t __attribute__((ext_vector_type(2)));  // one 16-byte store per pair

constexpr uint32_t kPointsHalf = 4;  // points whose coordinate loads are issued together
static_assert(kPointsPer % kPointsHalf == 0, "a lane's points split into whole load groups");

// Points k0 + i * kPointsThreads, i < kPointsHalf, of one lane: every
// coordinate load first, then the arithmetic.  err[i] is points_locate's
// verdict; ~0u marks a point at or past n.
__device__ __forceinline__ void points_load_locate(const zhip_points_geom& g, const PointsCoords& pc, uint32_t k0,
                                                   uint32_t n, uint32_t* err, uint32_t* rix, int64_t* off) {
    int64_t x[kPointsHalf][ZHIP_MAX_DIMS];
#pragma unroll
    for (uint32_t i = 0; i < kPointsHalf; ++i) {
        const uint32_t k = k0 + i * kPointsThreads;
#pragma unroll
        for (int d = 0; d < ZHIP_MAX_DIMS; ++d) x[i][d] = (d < g.ndim && k < n) ? pc.c[d][k] : 0;
    }
#pragma unroll
    for (uint32_t i = 0; i < kPointsHalf; ++i) {
        const uint32_t k = k0 + i * kPointsThreads;
        err[i] = points_locate(g, x[i], rix[i], off[i]);
        if (k >= n) err[i] = ~0u;
    }
}

template <bool LDS>
__global__ __launch_bounds__(kPointsThreads) void k_points_count(const zhip_points_geom g, const PointsCoords pc,
                                                                  uint32_t n, uint32_t n_chunks,
                                                                  uint32_t* __restrict__ counts,
                                                                  uint32_t* __restrict__ d_err) {
    __shared__ uint32_t hist[LDS ? kPointsLdsBins : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * ZHIP_POINTS_RUN + tid;  // < 2^31 + ZHIP_POINTS_RUN
    if (LDS) {
        for (uint32_t b = tid; b < n_chunks; b += kPointsThreads) hist[b] = 0;
        __syncthreads();
    }
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t h = 0; h < kPointsPer; h += kPointsHalf) {
        uint32_t err[kPointsHalf], rix[kPointsHalf];
        int64_t off[kPointsHalf];
        points_load_locate(g, pc, base + h * kPointsThreads, n, err, rix, off);
#pragma unroll
        for (uint32_t i = 0; i < kPointsHalf; ++i) {
            if (err[i] == ~0u) continue;
            if (err[i]) {
                bad |= err[i];  // not counted, touches nothing else
            } else if (LDS) {
                __hip_atomic_fetch_add(&hist[rix[i]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                __hip_atomic_fetch_add(&counts[rix[i]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (bad) __hip_atomic_fetch_or(d_err, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (LDS) {
        __syncthreads();
        for (uint32_t b = tid; b < n_chunks; b += kPointsThreads) {
            const uint32_t c = hist[b];
            if (c) __hip_atomic_fetch_add(&counts[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kPointsThreads) void k_points_fill(const zhip_points_geom g, const PointsCoords pc,
                                                                 uint32_t n, uint32_t n_chunks,
                                                                 const uint32_t* __restrict__ first,
                                                                 uint32_t* __restrict__ cursor,
                                                                 int64_t* __restrict__ table) {
    __shared__ uint32_t hist[LDS ? kPointsLdsBins : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * ZHIP_POINTS_RUN + tid;
    if (LDS) {
        for (uint32_t b = tid; b < n_chunks; b += kPointsThreads) hist[b] = 0;
        __syncthreads();
    }
    // per point: its chunk, its slot offset, and its position -- the rank
    // inside the workgroup's bin (LDS) or the pair index itself
    uint32_t rix[kPointsPer], pos[kPointsPer];
    int64_t off[kPointsPer];
    bool ok[kPointsPer];
#pragma unroll
    for (uint32_t h = 0; h < kPointsPer; h += kPointsHalf) {
        uint32_t err[kPointsHalf];
        points_load_locate(g, pc, base + h * kPointsThreads, n, err, rix + h, off + h);
#pragma unroll
        for (uint32_t i = 0; i < kPointsHalf; ++i) {
            const uint32_t j = h + i;
            ok[j] = err[i] == 0;
            pos[j] = 0;
            if (!ok[j]) continue;
            if (LDS)
                pos[j] = __hip_atomic_fetch_add(&hist[rix[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
                pos[j] = first[rix[j]] +
                         __hip_atomic_fetch_add(&cursor[rix[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (LDS) {
        __syncthreads();
        // the bin's count becomes the pair index of the workgroup's first point of that chunk
        for (uint32_t b = tid; b < n_chunks; b += kPointsThreads) {
            const uint32_t c = hist[b];
            if (c)
                hist[b] = first[b] + __hip_atomic_fetch_add(&cursor[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t j = 0; j < kPointsPer; ++j) {
        if (!ok[j]) continue;
        const uint32_t p = LDS ? hist[rix[j]] + pos[j] : pos[j];
        if (p >= n) continue;  // first / cursor not this list's: nothing outside the table
        int64_t A, B;
        points_pair(g, base + j * kPointsThreads, off[j], A, B);
        pair_t v;
        v.x = A;
        v.y = B;
        *reinterpret_cast<pair_t*>(table + 2 * (uint64_t)p) = v;
    }
}

static uint32_t points_blocks(uint32_t n) { return (n + ZHIP_POINTS_RUN - 1) / ZHIP_POINTS_RUN; }

int points_count_launch(const zhip_points_geom& g, const PointsCoords& pc, uint32_t n, uint32_t n_chunks,
                        uint32_t* d_counts, uint32_t* d_err, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_chunks <= kPointsLdsBins)
        k_points_count<true><<<points_blocks(n), kPointsThreads, 0, st>>>(g, pc, n, n_chunks, d_counts, d_err);
    else
        k_points_count<false><<<points_blocks(n), kPointsThreads, 0, st>>>(g, pc, n, n_chunks, d_counts, d_err);
    g_last_kernel = "k_points_count";
    return (int)hipGetLastError();
}

int points_fill_launch(const zhip_points_geom& g, const PointsCoords& pc, uint32_t n, uint32_t n_chunks,
                       const uint32_t* d_first, uint32_t* d_cursor, int64_t* d_table, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_chunks <= kPointsLdsBins)
        k_points_fill<true><<<points_blocks(n), kPointsThreads, 0, st>>>(g, pc, n, n_chunks, d_first, d_cursor, d_table);
    else
        k_points_fill<false><<<points_blocks(n), kPointsThreads, 0, st>>>(g, pc, n, n_chunks, d_first, d_cursor, d_table);
    g_last_kernel = "k_points_fill";
    return (int)hipGetLastError();
}

}  // namespace zhip
