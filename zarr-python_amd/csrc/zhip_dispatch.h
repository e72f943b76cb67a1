// Host-side kernel selection and launch helpers shared by the launcher files
// (decode.hip, decode_rows.hip, decode_tile.hip, encode.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "zhip_internal.h"

namespace zhip {

// The item type of a kernel instantiation, as a type: the item size and the
// item mode (the SWAP template parameter of every kernel).  Mode bit 0 is
// ZHIP_LF_SWAP: stored endian != native.  Mode bit 1 is ZHIP_LF_COMPLEX on an
// 8-byte item: two float32 (complex64), so a swap reverses each 4-byte half in
// place (swap_block / store_item, zhip_device.h) and the encode kernels compare
// with the fill by the complex rule (zhip_fill_eq.h).
constexpr int kModeSwap = 1, kModeCplx = 2;

inline int item_mode(uint32_t lflags, int item) {
    return ((lflags & ZHIP_LF_SWAP) ? kModeSwap : 0) | ((item == 8 && (lflags & ZHIP_LF_COMPLEX)) ? kModeCplx : 0);
}

template <int ITEM, int SWAP>
struct ItemTag {
    static constexpr int item = ITEM;
    static constexpr int swap = SWAP;
};

// The one item dispatcher: f(ItemTag<item, mode>{}) for the kernel
// instantiations of an item type -- 1-byte items never swap, so (1, swap) is
// never produced -- and nullptr for any other item size.  f is a generic
// lambda returning the kernel for its tag:
//   for_item(item, mode, [&](auto t) -> KernelFn {
//       using T = decltype(t);
//       return crc ? k<true, T::item, T::swap> : k<false, T::item, T::swap>;
//   });
// The decode kernels use the mode to swap only: unswapped complex64 is the
// plain 8-byte item there, so for_item has eight instantiations (the seven of
// the real item types and swapped complex64); for_item_enc, for the encode
// kernels, has the ninth.
template <bool ENC, class F>
auto for_item_impl(int item, int mode, F&& f) -> decltype(f(ItemTag<1, 0>{})) {
    switch (item) {
        case 1: return f(ItemTag<1, 0>{});
        case 2: return (mode & kModeSwap) ? f(ItemTag<2, 1>{}) : f(ItemTag<2, 0>{});
        case 4: return (mode & kModeSwap) ? f(ItemTag<4, 1>{}) : f(ItemTag<4, 0>{});
        case 8:
            if (mode == (kModeSwap | kModeCplx)) return f(ItemTag<8, kModeSwap | kModeCplx>{});
            if constexpr (ENC) {
                if (mode == kModeCplx) return f(ItemTag<8, kModeCplx>{});
            }
            return (mode & kModeSwap) ? f(ItemTag<8, 1>{}) : f(ItemTag<8, 0>{});
        default: return nullptr;
    }
}

template <class F>
auto for_item(int item, int mode, F&& f) -> decltype(f(ItemTag<1, 0>{})) {
    return for_item_impl<false>(item, mode, static_cast<F&&>(f));
}

template <class F>
auto for_item_enc(int item, int mode, F&& f) -> decltype(f(ItemTag<1, 0>{})) {
    return for_item_impl<true>(item, mode, static_cast<F&&>(f));
}

// The headline item type (4-byte little-endian items of a CRC layout): the
// only one most measurement arms are instantiated for.
inline bool headline_item(bool crc, int item, int swap) { return crc && item == 4 && !(swap & kModeSwap); }

// One launch: a null kernel is unsupported; an empty grid is done without a
// launch (and without touching zhip_last_kernel); otherwise name, launch, map
// the error.
template <class P>
int fire(void (*fn)(const P), const char* name, uint32_t grid, uint32_t block, const P& params, hipStream_t stream) {
    if (!fn) return ZHIP_E_UNSUPPORTED;
    if (grid == 0) return ZHIP_OK;
    g_last_kernel = name;
    g_last_grid = grid;
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
