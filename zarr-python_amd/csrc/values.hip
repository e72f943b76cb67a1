// k_value_map: scale_offset and cast_value on the device (zhip_value_map,
// include/zarrhip.h).  Decode: stored elements -> array elements; encode:
// array elements -> stored elements, with the per-item non-empty words.  The
// element and address arithmetic is zhip_values.h's, shared with the CPU hook.
//
// Launch shape (k_select_copy's): one workgroup of 256 lanes per tile of
// ZHIP_VALUE_TILE elements of ONE item; the item is found from the prefix
// array of per-item tile counts by a block-uniform binary search kept on the
// scalar side.  The op record is a kernel argument: every branch on a dtype,
// a stage or a mode is launch-uniform.
//
// Memory access is instantiated per (a item size, b item size).  An item with
// a contiguous, vector-aligned innermost dimension (value_vec_ok) gives each
// lane V consecutive elements, V = 16 bytes of the narrower side (8 elements
// at most): 8 x int16 in, two 16-byte float32 stores out.  Any other item
// goes element by element, lane l taking elements l, l + 256, ... of the
// tile, all loads issued before the first store.  Every store is an ordinary
// vector store.
//
// Errors and emptiness are reduced within the wave (ballots), then lane 0
// issues at most one atomic OR on the error word and one store of 1 to the
// item's non-empty word.
#include <hip/hip_runtime.h>

#include "zhip_internal.h"
#include "zhip_select.h"
#include "zhip_values.h"

namespace zhip {

template <int SZ>
__device__ __forceinline__ uint64_t val_load(const uint8_t* p) {
    if constexpr (SZ == 1) return *p;
    if constexpr (SZ == 2) return *reinterpret_cast<const uint16_t*>(p);
    if constexpr (SZ == 4) return *reinterpret_cast<const uint32_t*>(p);
    return *reinterpret_cast<const uint64_t*>(p);
}

template <int SZ>
__device__ __forceinline__ void val_store(uint8_t* p, uint64_t v) {
    if constexpr (SZ == 1) *p = (uint8_t)v;
    else if constexpr (SZ == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)v;
    else if constexpr (SZ == 4) *reinterpret_cast<uint32_t*>(p) = (uint32_t)v;
    else *reinterpret_cast<uint64_t*>(p) = v;
}

// NB bytes (8, 16, 32 or 64) as words, in 16-byte accesses (one 8-byte access for 8)
template <int NB>
__device__ __forceinline__ void vec_load(const uint8_t* p, uint32_t* w) {
    if constexpr (NB == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x;
        w[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            w[4 * i] = v.x;
            w[4 * i + 1] = v.y;
            w[4 * i + 2] = v.z;
            w[4 * i + 3] = v.w;
        }
    }
}

template <int NB>
__device__ __forceinline__ void vec_store(uint8_t* p, const uint32_t* w) {
    if constexpr (NB == 8) {
        *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; ++i)
            reinterpret_cast<uint4*>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
}

template <int SZ>
__device__ __forceinline__ uint64_t word_get(const uint32_t* w, int j) {
    if constexpr (SZ == 8) return ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
    if constexpr (SZ == 4) return w[j];
    if constexpr (SZ == 2) return (w[j / 2] >> (16 * (j % 2))) & 0xFFFFu;
    return (w[j / 4] >> (8 * (j % 4))) & 0xFFu;
}

template <int SZ>
__device__ __forceinline__ void word_put(uint32_t* w, int j, uint64_t v) {  // w zeroed
    if constexpr (SZ == 8) {
        w[2 * j] = (uint32_t)v;
        w[2 * j + 1] = (uint32_t)(v >> 32);
    } else if constexpr (SZ == 4) {
        w[j] = (uint32_t)v;
    } else if constexpr (SZ == 2) {
        w[j / 2] |= ((uint32_t)v & 0xFFFFu) << (16 * (j % 2));
    } else {
        w[j / 4] |= ((uint32_t)v & 0xFFu) << (8 * (j % 4));
    }
}

template <int ASZ, int BSZ>
__global__ __launch_bounds__(kValThreads) void k_value_map(
    const zhip_value_op op, const zhip_value_item* __restrict__ items, uint32_t n_items,
    const uint32_t* __restrict__ prefix, const zhip_status* __restrict__ status, const uint8_t* __restrict__ a,
    uint64_t a_size, uint8_t* __restrict__ b, uint64_t b_size, uint32_t* __restrict__ d_err,
    uint32_t* __restrict__ d_nonempty) {
    constexpr int kNarrow = ASZ < BSZ ? ASZ : BSZ;
    constexpr int V = kNarrow == 1 ? 8 : (16 / kNarrow > 8 ? 8 : 16 / kNarrow);
    const uint32_t tile = blockIdx.x;
    const uint32_t ii = __builtin_amdgcn_readfirstlane(select_find_item(prefix, n_items, tile));
    const zhip_value_item& it = items[ii];
    const uint32_t total = it.total;
    const uint32_t base = (tile - prefix[ii]) * ZHIP_VALUE_TILE;
    bool missing = false;
    if (!op.encode) {
        if (it.flags & ZHIP_VI_MISSING) missing = true;
        else if (it.flags & ZHIP_VI_STATUS) missing = status[it.status].code == ZHIP_ST_MISSING;
    }
    missing = __builtin_amdgcn_readfirstlane((uint32_t)missing) != 0;
    const bool want_ne = op.encode && d_nonempty != nullptr;
    const uint64_t fillb = op.fill & vt_mask(op.array_dt);
    uint32_t err = 0;
    bool ne = false;

    const bool vec = __builtin_amdgcn_readfirstlane(
                         (uint32_t)value_vec_ok(it, (uint64_t)(uintptr_t)a, (uint64_t)(uintptr_t)b, ASZ, BSZ)) != 0;
    if (vec) {
#pragma unroll
        for (uint32_t j = 0; j < kValPer / V; ++j) {
            const uint32_t e = base + (threadIdx.x + j * kValThreads) * V;
            if (e >= total) continue;
            int64_t ao, bo;
            value_addr(it, e, ao, bo);
            if (!value_inside(ao, bo, a_size, b_size, V * ASZ, V * BSZ)) continue;
            uint32_t win[V * ASZ / 4], wout[V * BSZ / 4];
#pragma unroll
            for (int k = 0; k < V * BSZ / 4; ++k) wout[k] = 0;
            if (!missing) vec_load<V * ASZ>(a + ao, win);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                uint64_t y = fillb;
                if (!missing) {
                    const uint64_t x = word_get<ASZ>(win, k);
                    if (want_ne) ne = ne || !value_eq_fill(op, x);
                    y = value_map_one(op, x, err);
                }
                word_put<BSZ>(wout, k, y);
            }
            vec_store<V * BSZ>(b + bo, wout);
        }
    } else {
        uint64_t x[kValPer];
        int64_t bo[kValPer];
        bool ok[kValPer];
#pragma unroll
        for (uint32_t j = 0; j < kValPer; ++j) {
            const uint32_t e = base + threadIdx.x + j * kValThreads;
            ok[j] = false;
            x[j] = 0;
            bo[j] = 0;
            if (e < total) {
                int64_t ao;
                value_addr(it, e, ao, bo[j]);
                ok[j] = value_inside(ao, bo[j], a_size, b_size, ASZ, BSZ);
                if (ok[j] && !missing) x[j] = val_load<ASZ>(a + ao);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kValPer; ++j) {
            if (!ok[j]) continue;
            uint64_t y = fillb;
            if (!missing) {
                if (want_ne) ne = ne || !value_eq_fill(op, x[j]);
                y = value_map_one(op, x[j], err);
            }
            val_store<BSZ>(b + bo[j], y);
        }
    }

    // wave reduction, then lane 0 alone touches the two words
    if (__any(err != 0)) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t bit = 1; bit <= ZHIP_VE_NAN; bit <<= 1)
            if (__any((err & bit) != 0)) w |= bit;
        if ((threadIdx.x & (warpSize - 1)) == 0) atomicOr(d_err, w);
    }
    if (want_ne && __any(ne) && (threadIdx.x & (warpSize - 1)) == 0) d_nonempty[ii] = 1u;
}

int value_launch(const zhip_value_op& op, const zhip_value_item* d_items, uint32_t n_items,
                 const uint32_t* d_tile_prefix, uint32_t n_tiles, const zhip_status* d_status, const void* a,
                 uint64_t a_size, void* b, uint64_t b_size, uint32_t* d_err, uint32_t* d_nonempty, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* pa = (const uint8_t*)a;
    uint8_t* pb = (uint8_t*)b;
    const uint32_t asz = vt_size(value_a_dt(op)), bsz = vt_size(value_b_dt(op));
#define ZHIP_VAL_ARM(A, B)                                                                                    \
    if (asz == A && bsz == B)                                                                                 \
        k_value_map<A, B><<<n_tiles, kValThreads, 0, st>>>(op, d_items, n_items, d_tile_prefix, d_status, pa, \
                                                           a_size, pb, b_size, d_err, d_nonempty);
    ZHIP_VAL_ARM(1, 1) ZHIP_VAL_ARM(1, 2) ZHIP_VAL_ARM(1, 4) ZHIP_VAL_ARM(1, 8)
    ZHIP_VAL_ARM(2, 1) ZHIP_VAL_ARM(2, 2) ZHIP_VAL_ARM(2, 4) ZHIP_VAL_ARM(2, 8)
    ZHIP_VAL_ARM(4, 1) ZHIP_VAL_ARM(4, 2) ZHIP_VAL_ARM(4, 4) ZHIP_VAL_ARM(4, 8)
    ZHIP_VAL_ARM(8, 1) ZHIP_VAL_ARM(8, 2) ZHIP_VAL_ARM(8, 4) ZHIP_VAL_ARM(8, 8)
#undef ZHIP_VAL_ARM
    g_last_kernel = "k_value_map";
    return (int)hipGetLastError();
}

}  // namespace zhip
