// k_select_copy: the element gather / scatter of orthogonal, coordinate and
// mask selections (zhip_select_copy, include/zarrhip.h).  Read: decoded chunks
// -> out; write: value -> decoded chunks.  The address arithmetic is
// zhip_select.h's, shared with the CPU hook.
//
// Launch shape: one workgroup per tile of ZHIP_SELECT_TILE elements of ONE
// item (a tile never spans two items); the item is found from the prefix array
// of per-item tile counts by a block-uniform binary search kept on the scalar
// side.  Lane l of the workgroup takes elements l, l + 256, l + 512, l + 768 of
// the tile: consecutive lanes walk the innermost product dimension, so a slice
// innermost dimension gives coalesced loads and stores; all four loads of a
// lane are issued before the first store.  Element-granular gathers through a
// table are uncoalesced by nature and lean on L2 / Infinity Cache.
#include <hip/hip_runtime.h>

#include "zhip_internal.h"
#include "zhip_select.h"

namespace zhip {

template <typename T>
__global__ __launch_bounds__(kSelThreads) void k_select_copy(
    const zhip_select_item* __restrict__ items, uint32_t n_items, const int64_t* __restrict__ table,
    const uint32_t* __restrict__ prefix, const uint8_t* __restrict__ a, uint64_t a_size, uint8_t* __restrict__ b,
    uint64_t b_size) {
    const uint32_t tile = blockIdx.x;
    const uint32_t ii = __builtin_amdgcn_readfirstlane(select_find_item(prefix, n_items, tile));
    const zhip_select_item& it = items[ii];
    const uint32_t total = it.total;
    const uint32_t e0 = (tile - prefix[ii]) * ZHIP_SELECT_TILE + threadIdx.x;
    T v[kSelPer];
    int64_t bo[kSelPer];
    bool ok[kSelPer];
#pragma unroll
    for (uint32_t j = 0; j < kSelPer; ++j) {
        const uint32_t e = e0 + j * kSelThreads;
        ok[j] = false;
        v[j] = T(0);
        bo[j] = 0;
        if (e < total) {
            int64_t ao;
            select_addr(it, table, e, ao, bo[j]);
            ok[j] = select_inside(ao, bo[j], a_size, b_size, (uint32_t)sizeof(T));
            if (ok[j]) v[j] = *reinterpret_cast<const T*>(a + ao);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kSelPer; ++j)
        if (ok[j]) *reinterpret_cast<T*>(b + bo[j]) = v[j];
}

int select_launch(const zhip_select_item* d_items, uint32_t n_items, const int64_t* d_table,
                  const uint32_t* d_tile_prefix, uint32_t n_tiles, const void* a, uint64_t a_size, void* b,
                  uint64_t b_size, uint32_t itemsize, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* pa = (const uint8_t*)a;
    uint8_t* pb = (uint8_t*)b;
    switch (itemsize) {
        case 1: k_select_copy<uint8_t><<<n_tiles, kSelThreads, 0, st>>>(d_items, n_items, d_table, d_tile_prefix, pa, a_size, pb, b_size); break;
        case 2: k_select_copy<uint16_t><<<n_tiles, kSelThreads, 0, st>>>(d_items, n_items, d_table, d_tile_prefix, pa, a_size, pb, b_size); break;
        case 4: k_select_copy<uint32_t><<<n_tiles, kSelThreads, 0, st>>>(d_items, n_items, d_table, d_tile_prefix, pa, a_size, pb, b_size); break;
        default: k_select_copy<uint64_t><<<n_tiles, kSelThreads, 0, st>>>(d_items, n_items, d_table, d_tile_prefix, pa, a_size, pb, b_size); break;
    }
    g_last_kernel = "k_select_copy";
    return (int)hipGetLastError();
}

}  // namespace zhip
