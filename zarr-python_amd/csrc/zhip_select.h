// Address arithmetic of zhip_select_copy (include/zarrhip.h, "the separable
// table form"), shared by the device kernel (select.hip) and the CPU test
// hook zhip_emulate_select_copy (capi.cpp): both walk the same tiles and
// compute every element's two byte offsets with these functions.
#pragma once
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zhip_gf2.h"

namespace zhip {

constexpr uint32_t kSelThreads = 256;
constexpr uint32_t kSelPer = ZHIP_SELECT_TILE / kSelThreads;  // elements per lane, kSelThreads apart

// The item whose tiles include `tile`: the last i with prefix[i] <= tile
// (prefix has n_items + 1 entries, prefix[0] = 0, prefix[n_items] = n_tiles >
// tile; items without elements have no tiles and are never found).
ZHIP_HD uint32_t select_find_item(const uint32_t* prefix, uint32_t n_items, uint32_t tile) {
    uint32_t lo = 0, hi = n_items;  // prefix[lo] <= tile < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// Byte offsets (relative to a and b) of element e of an item, e < it.total:
// the last dimension is the fastest.
ZHIP_HD void select_addr(const zhip_select_item& it, const int64_t* table, uint32_t e, int64_t& ao, int64_t& bo) {
    ao = it.a_base;
    bo = it.b_base;
    for (int d = (int)it.ndim - 1; d >= 0; --d) {
        const zhip_select_dim& D = it.dims[d];
        uint32_t k = e;
        if (d > 0) {
            const uint32_t q = fdiv_apply(e, D.div.m, D.div.s);
            k = e - q * D.count;
            e = q;
        }
        if (D.table) {
            const int64_t* p = table + 2 * (D.table_off + k);
            ao += p[0];
            bo += p[1];
        } else {
            ao += D.a0 + (int64_t)k * D.sa;
            bo += D.b0 + (int64_t)k * D.sb;
        }
    }
}

// the kernel's fence (and the hook's bounds verdict): both offsets inside their buffers
ZHIP_HD bool select_inside(int64_t ao, int64_t bo, uint64_t a_size, uint64_t b_size, uint32_t itemsize) {
    return ao >= 0 && bo >= 0 && (uint64_t)ao + itemsize <= a_size && (uint64_t)bo + itemsize <= b_size;
}

int select_launch(const zhip_select_item* d_items, uint32_t n_items, const int64_t* d_table,
                  const uint32_t* d_tile_prefix, uint32_t n_tiles, const void* a, uint64_t a_size, void* b,
                  uint64_t b_size, uint32_t itemsize, void* stream);  // select.hip; 0 or a hipError_t

}  // namespace zhip
