// k_axis_last / k_axis_count / k_axis_fill: one axis of an orthogonal selection
// whose indices are a device array, planned on the device (zhip_axis_last /
// zhip_axis_count / zhip_axis_fill, include/zarrhip.h).  They replace the
// per-index host work of IntArrayDimIndexer.__init__ (wraparound, bounds check,
// chunk of each index, the grouping argsort, the per-chunk slices) and, for a
// write with an array value, the per-dimension keep-last dedupe of the host
// normaliser; the per-index arithmetic is zhip_axis.h's, shared with the CPU
// hook.
//
// Launch shape (points.hip's): one workgroup of 256 lanes per run of
// ZHIP_AXIS_RUN indices; lane l takes indices l, l + 256, ... of the run, so
// the int64 loads are coalesced, and a lane issues all of its loads before the
// arithmetic.
//
// Counters.  Many indices fall on few chunks, and adds that share a row
// serialise.  While the axis has at most kAxisLdsBins chunks (LDS = true) a
// workgroup histograms its run in LDS -- count, and in k_axis_count the two
// bounds words -- and issues ONE global atomic per word of a non-empty bin; in
// k_axis_fill that atomic is a returning add of the bin's count onto cursor[c],
// whose result is the workgroup's base inside the chunk's range, and a lane's
// rank inside the bin is what its LDS atomic returned.  Longer axes
// (LDS = false) take global atomics per index: that many counters spread them.
//
// Keep-last.  k_axis_last leaves last[v] = 1 + the largest k with x[k] == v (an
// atomic max: independent of scheduling).  Given `last`, count and fill skip
// every index that is not the winner of its element.
//
// Stores.  counts / lo / hi / cursor are touched at c < g.grid only and last at
// v < g.length only (axis_locate range-checks the index in the same call that
// produces v and c); a pair goes to table[g.table_off + first[c] + position]
// and only when that index is below table_pairs, the table's length.
#include <hip/hip_runtime.h>

#include "zhip_axis.h"
#include "zhip_internal.h"

namespace zhip {

typedef int64_t axis_pair_t __attribute__((ext_vector_type(2)));  // one 16-byte store per pair

// The lane's kAxisPer indices, every load issued before any is used.
__device__ __forceinline__ void axis_load(const int64_t* __restrict__ x, uint32_t base, uint32_t n, int64_t* xv) {
#pragma unroll
    for (uint32_t j = 0; j < kAxisPer; ++j) {
        const uint32_t k = base + j * kAxisThreads;
        xv[j] = k < n ? x[k] : 0;
    }
}

__global__ __launch_bounds__(kAxisThreads) void k_axis_last(const zhip_axis_geom g, const int64_t* __restrict__ x,
                                                            uint32_t n, uint32_t* __restrict__ last) {
    const uint32_t base = blockIdx.x * ZHIP_AXIS_RUN + threadIdx.x;  // < 2^31 + ZHIP_AXIS_RUN
    int64_t xv[kAxisPer];
    axis_load(x, base, n, xv);
#pragma unroll
    for (uint32_t j = 0; j < kAxisPer; ++j) {
        const uint32_t k = base + j * kAxisThreads;
        uint32_t v, c, r;
        if (k < n && axis_locate(g, xv[j], v, c, r))
            __hip_atomic_fetch_max(&last[v], k + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool LDS>
__global__ __launch_bounds__(kAxisThreads) void k_axis_count(const zhip_axis_geom g, const int64_t* __restrict__ x,
                                                             uint32_t n, const uint32_t* __restrict__ last,
                                                             uint32_t* __restrict__ counts, uint32_t* __restrict__ lo,
                                                             uint32_t* __restrict__ hi, uint32_t* __restrict__ d_err) {
    __shared__ uint32_t s_cnt[LDS ? kAxisLdsBins : 1];
    __shared__ uint32_t s_lo[LDS ? kAxisLdsBins : 1];
    __shared__ uint32_t s_hi[LDS ? kAxisLdsBins : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * ZHIP_AXIS_RUN + tid;
    if (LDS) {
        for (uint32_t b = tid; b < g.grid; b += kAxisThreads) s_cnt[b] = s_lo[b] = s_hi[b] = 0;
        __syncthreads();
    }
    int64_t xv[kAxisPer];
    axis_load(x, base, n, xv);
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < kAxisPer; ++j) {
        const uint32_t k = base + j * kAxisThreads;
        if (k >= n) continue;
        uint32_t v, c, r;
        if (!axis_locate(g, xv[j], v, c, r)) {
            bad = true;  // not counted, touches nothing else
            continue;
        }
        if (last && last[v] != k + 1u) continue;  // a later index names the same element
        const uint32_t lw = axis_lo_word(g, r);
        if (LDS) {
            __hip_atomic_fetch_add(&s_cnt[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&s_lo[c], lw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&s_hi[c], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            __hip_atomic_fetch_add(&counts[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&lo[c], lw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&hi[c], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (bad) __hip_atomic_fetch_or(d_err, g.err_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (LDS) {
        __syncthreads();
        for (uint32_t b = tid; b < g.grid; b += kAxisThreads) {
            const uint32_t c = s_cnt[b];
            if (!c) continue;
            __hip_atomic_fetch_add(&counts[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&lo[b], s_lo[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&hi[b], s_hi[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kAxisThreads) void k_axis_fill(const zhip_axis_geom g, const int64_t* __restrict__ x,
                                                            uint32_t n, const uint32_t* __restrict__ last,
                                                            const uint32_t* __restrict__ first,
                                                            uint32_t* __restrict__ cursor, int64_t* __restrict__ table,
                                                            uint64_t table_pairs) {
    __shared__ uint32_t hist[LDS ? kAxisLdsBins : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * ZHIP_AXIS_RUN + tid;
    if (LDS) {
        for (uint32_t b = tid; b < g.grid; b += kAxisThreads) hist[b] = 0;
        __syncthreads();
    }
    int64_t xv[kAxisPer];
    axis_load(x, base, n, xv);
    // per index: its chunk, its in-chunk index, and its position -- the rank
    // inside the workgroup's bin (LDS) or the index inside the axis' pairs
    uint32_t cix[kAxisPer], rr[kAxisPer], pos[kAxisPer];
    bool ok[kAxisPer];
#pragma unroll
    for (uint32_t j = 0; j < kAxisPer; ++j) {
        const uint32_t k = base + j * kAxisThreads;
        uint32_t v = 0;
        cix[j] = rr[j] = pos[j] = 0;
        ok[j] = k < n && axis_locate(g, xv[j], v, cix[j], rr[j]);
        if (ok[j] && last) ok[j] = last[v] == k + 1u;
        if (!ok[j]) continue;
        if (LDS)
            pos[j] = __hip_atomic_fetch_add(&hist[cix[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            pos[j] = first[cix[j]] +
                     __hip_atomic_fetch_add(&cursor[cix[j]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (LDS) {
        __syncthreads();
        // the bin's count becomes the pair index of the workgroup's first index of that chunk
        for (uint32_t b = tid; b < g.grid; b += kAxisThreads) {
            const uint32_t c = hist[b];
            if (c)
                hist[b] = first[b] + __hip_atomic_fetch_add(&cursor[b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t j = 0; j < kAxisPer; ++j) {
        if (!ok[j]) continue;
        const uint64_t p = g.table_off + (uint64_t)(LDS ? hist[cix[j]] + pos[j] : pos[j]);
        if (p >= table_pairs) continue;  // first / cursor not this list's: nothing outside the table
        int64_t A, B;
        axis_pair(g, base + j * kAxisThreads, rr[j], A, B);
        axis_pair_t w;
        w.x = A;
        w.y = B;
        *reinterpret_cast<axis_pair_t*>(table + 2 * p) = w;
    }
}

static uint32_t axis_blocks(uint32_t n) { return (n + ZHIP_AXIS_RUN - 1) / ZHIP_AXIS_RUN; }

int axis_last_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, uint32_t* d_last, void* stream) {
    k_axis_last<<<axis_blocks(n), kAxisThreads, 0, (hipStream_t)stream>>>(g, d_x, n, d_last);
    g_last_kernel = "k_axis_last";
    return (int)hipGetLastError();
}

int axis_count_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, const uint32_t* d_last,
                      uint32_t* d_counts, uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_err, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (g.grid <= kAxisLdsBins)
        k_axis_count<true><<<axis_blocks(n), kAxisThreads, 0, st>>>(g, d_x, n, d_last, d_counts, d_lo, d_hi, d_err);
    else
        k_axis_count<false><<<axis_blocks(n), kAxisThreads, 0, st>>>(g, d_x, n, d_last, d_counts, d_lo, d_hi, d_err);
    g_last_kernel = "k_axis_count";
    return (int)hipGetLastError();
}

int axis_fill_launch(const zhip_axis_geom& g, const int64_t* d_x, uint32_t n, const uint32_t* d_last,
                     const uint32_t* d_first, uint32_t* d_cursor, int64_t* d_table, uint64_t table_pairs,
                     void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (g.grid <= kAxisLdsBins)
        k_axis_fill<true><<<axis_blocks(n), kAxisThreads, 0, st>>>(g, d_x, n, d_last, d_first, d_cursor, d_table,
                                                                   table_pairs);
    else
        k_axis_fill<false><<<axis_blocks(n), kAxisThreads, 0, st>>>(g, d_x, n, d_last, d_first, d_cursor, d_table,
                                                                    table_pairs);
    g_last_kernel = "k_axis_fill";
    return (int)hipGetLastError();
}

}  // namespace zhip
