// Host-side kernel selection and launch helpers shared by the launcher files
// (decode.hip, decode_rows.hip, decode_tile.hip, encode.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "zhip_internal.h"

namespace zhip {

// The (itemsize, byteswap) pair of a kernel instantiation, as a type.
template <int ITEM, bool SWAP>
struct ItemTag {
    static constexpr int item = ITEM;
    static constexpr bool swap = SWAP;
};

// The one item dispatcher: f(ItemTag<item, swap>{}) for the seven kernel
// instantiations of an item type -- 1-byte items never swap, so (1, true) is
// never produced -- and nullptr for any other item size.  f is a generic
// lambda returning the kernel for its tag:
//   for_item(item, swap, [&](auto t) -> KernelFn {
//       using T = decltype(t);
//       return crc ? k<true, T::item, T::swap> : k<false, T::item, T::swap>;
//   });
template <class F>
auto for_item(int item, bool swap, F&& f) -> decltype(f(ItemTag<1, false>{})) {
    switch (item) {
        case 1: return f(ItemTag<1, false>{});
        case 2: return swap ? f(ItemTag<2, true>{}) : f(ItemTag<2, false>{});
        case 4: return swap ? f(ItemTag<4, true>{}) : f(ItemTag<4, false>{});
        case 8: return swap ? f(ItemTag<8, true>{}) : f(ItemTag<8, false>{});
        default: return nullptr;
    }
}

// The headline item type (4-byte little-endian items of a CRC layout): the
// only one most measurement arms are instantiated for.
inline bool headline_item(bool crc, int item, bool swap) { return crc && item == 4 && !swap; }

// One launch: a null kernel is unsupported; an empty grid is done without a
// launch (and without touching zhip_last_kernel); otherwise name, launch, map
// the error.
template <class P>
int fire(void (*fn)(const P), const char* name, uint32_t grid, uint32_t block, const P& params, hipStream_t stream) {
    if (!fn) return ZHIP_E_UNSUPPORTED;
    if (grid == 0) return ZHIP_OK;
    g_last_kernel = name;
    ++g_launch_count;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(block), 0, stream, params);
    return hipGetLastError() == hipSuccess ? ZHIP_OK : ZHIP_E_HIP;
}

// Workgroups of a persistent launch: what is resident at once (max_grid
// arrives as CUs * 8; the kernel's occupancy replaces the 8), or the tuning
// build's ZHIP_TUNE_MAX_GRID as it stands.
template <class P>
int resident_grid(void (*fn)(const P), int max_grid) {
    if (g_tune_max_grid > 0) return g_tune_max_grid;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), kThreads, 0) ==
            hipSuccess && per_cu > 0)
        max_grid = (max_grid / 8) * per_cu;
    return max_grid;
}

}  // namespace zhip
