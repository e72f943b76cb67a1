// The element arithmetic and address arithmetic of zhip_value_map
// (include/zarrhip.h, "element-wise value codecs"), shared by the device kernel
// (values.hip) and the CPU hook zhip_emulate_value_map (value_map.cpp): one
// statement of scale_offset (src/zarr/codecs/scale_offset.py:220-279) and of
// the cast_value rules the header lists.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zhip_fill_eq.h"
#include "zhip_gf2.h"

namespace zhip {

constexpr uint32_t kValThreads = 256;
constexpr uint32_t kValPer = ZHIP_VALUE_TILE / kValThreads;  // elements per lane

ZHIP_HD uint32_t vt_size(uint32_t dt) {
    return dt <= ZHIP_VT_U8 ? 1u : dt <= ZHIP_VT_U16 ? 2u : (dt <= ZHIP_VT_U32 || dt == ZHIP_VT_F32) ? 4u : 8u;
}
ZHIP_HD bool vt_float(uint32_t dt) { return dt >= ZHIP_VT_F32; }
ZHIP_HD bool vt_signed(uint32_t dt) { return (dt & 1u) == 0; }  // integer codes only
ZHIP_HD uint64_t vt_mask(uint32_t dt) {
    const uint32_t s = vt_size(dt);
    return s == 8 ? ~0ull : ((1ull << (8 * s)) - 1ull);
}
ZHIP_HD int64_t vt_min(uint32_t dt) {  // integer codes only
    return vt_signed(dt) ? (int64_t)(~0ull << (8 * vt_size(dt) - 1)) : 0;
}
ZHIP_HD int64_t vt_max(uint32_t dt) {
    const uint32_t bits = 8 * vt_size(dt);
    return vt_signed(dt) ? (int64_t)((1ull << (bits - 1)) - 1ull) : (int64_t)((1ull << bits) - 1ull);  // no uint64
}
// raw item bits -> the integer they denote
ZHIP_HD int64_t vt_int(uint32_t dt, uint64_t x) {
    const uint32_t bits = 8 * vt_size(dt);
    if (bits == 64) return (int64_t)x;
    x &= (1ull << bits) - 1ull;
    if (vt_signed(dt) && (x >> (bits - 1))) x |= ~0ull << bits;
    return (int64_t)x;
}

ZHIP_HD float vt_f32(uint64_t x) { return __builtin_bit_cast(float, (uint32_t)x); }
ZHIP_HD double vt_f64(uint64_t x) { return __builtin_bit_cast(double, x); }
ZHIP_HD uint64_t vt_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
ZHIP_HD uint64_t vt_bits(double f) { return __builtin_bit_cast(uint64_t, f); }

ZHIP_HD bool vt_is_nan(uint32_t dt, uint64_t x) {
    if (dt == ZHIP_VT_F32) return bits_nan<4>(x);
    if (dt == ZHIP_VT_F64) return bits_nan<8>(x);
    return false;
}

// NDBuffer.all_equal against the array fill (buffer/core.py:534-558), the rule
// of zhip_fill_eq.h over a value type code (integers, float32, float64):
// bitwise, except that any NaN equals a NaN fill.
ZHIP_HD bool value_eq_fill(const zhip_value_op& op, uint64_t x) {
    const uint64_t m = vt_mask(op.array_dt);
    return (x & m) == (op.fill & m) || (op.fill_nan && vt_is_nan(op.array_dt, x));
}

// scale_offset in the array dtype.  Integers are exact: |x - offset| < 2^33 and
// |scale| <= 2^32, so the product is formed on magnitudes, after the cases
// that cannot be in any accepted dtype's range (|.| > 2^32) are set aside.
ZHIP_HD uint64_t value_scale_offset(const zhip_value_op& op, uint64_t x, uint32_t& err) {
    // (x - offset) * scale and x / scale + offset are two IEEE operations each,
    // as numpy evaluates them: never one fused multiply-add (this function only)
#pragma clang fp contract(off)
    const uint32_t dt = op.array_dt;
    if (dt == ZHIP_VT_F32) {
        const float v = vt_f32(x), o = vt_f32(op.offset), s = vt_f32(op.scale);
        float r;
        if (op.encode) {
            r = v - o;
            r = r * s;
        } else {
            r = v / s;
            r = r + o;
        }
        return vt_bits(r);
    }
    if (dt == ZHIP_VT_F64) {
        const double v = vt_f64(x), o = vt_f64(op.offset), s = vt_f64(op.scale);
        double r;
        if (op.encode) {
            r = v - o;
            r = r * s;
        } else {
            r = v / s;
            r = r + o;
        }
        return vt_bits(r);
    }
    const int64_t v = vt_int(dt, x), o = vt_int(dt, op.offset), s = vt_int(dt, op.scale);
    int64_t r;
    if (op.encode) {
        const int64_t d = v - o;
        const uint64_t ad = d < 0 ? 0ull - (uint64_t)d : (uint64_t)d;
        const uint64_t as = s < 0 ? 0ull - (uint64_t)s : (uint64_t)s;
        const uint64_t p = ad * as;  // < 2^64 when ad < 2^32, as <= 2^32
        if (ad >= (1ull << 32) || p > (1ull << 32)) {  // (scale != 0: beyond every accepted dtype)
            err |= ZHIP_VE_SO_RANGE;
            return 0;
        }
        r = ((d < 0) != (s < 0)) ? -(int64_t)p : (int64_t)p;
    } else {
        if (s == 0 || v % s != 0) {
            err |= ZHIP_VE_INEXACT;
            return 0;
        }
        r = v / s + o;
    }
    if (r < vt_min(dt) || r > vt_max(dt)) {
        err |= ZHIP_VE_SO_RANGE;
        return 0;
    }
    return (uint64_t)r & vt_mask(dt);
}

ZHIP_HD float vround(float v, uint32_t mode) {
    switch (mode) {
        case ZHIP_VR_TOWARDS_ZERO: return truncf(v);
        case ZHIP_VR_TOWARDS_POSITIVE: return ceilf(v);
        case ZHIP_VR_TOWARDS_NEGATIVE: return floorf(v);
        case ZHIP_VR_NEAREST_AWAY: return roundf(v);
        default: return rintf(v);
    }
}
ZHIP_HD double vround(double v, uint32_t mode) {
    switch (mode) {
        case ZHIP_VR_TOWARDS_ZERO: return trunc(v);
        case ZHIP_VR_TOWARDS_POSITIVE: return ceil(v);
        case ZHIP_VR_TOWARDS_NEGATIVE: return floor(v);
        case ZHIP_VR_NEAREST_AWAY: return round(v);
        default: return rint(v);
    }
}
ZHIP_HD float vfmod(float a, float b) { return fmodf(a, b); }
ZHIP_HD double vfmod(double a, double b) { return fmod(a, b); }

// Rules 2-4: the ends of every accepted target (at most 16 bits from float32,
// 32 bits from float64) are exact in F, so the comparisons are.
template <typename F>
ZHIP_HD uint64_t value_cast_float(const zhip_value_op& op, uint32_t to, F v, uint32_t& err) {
    if (v != v) {
        err |= ZHIP_VE_NAN;
        return 0;
    }
    const F r = vround(v, op.rounding);
    const int64_t lo = vt_min(to), hi = vt_max(to);
    if (r < (F)lo || r > (F)hi) {
        if (op.out_of_range == ZHIP_VO_CLAMP) return (uint64_t)(r < (F)lo ? lo : hi) & vt_mask(to);
        if (op.out_of_range == ZHIP_VO_WRAP && !__builtin_isinf(r)) {
            const F m = vfmod(r, (F)(vt_mask(to)) + (F)1);  // exact; |m| < 2^bits
            return (uint64_t)(int64_t)m & vt_mask(to);
        }
        err |= ZHIP_VE_CAST_RANGE;
        return 0;
    }
    return (uint64_t)(int64_t)r & vt_mask(to);
}

ZHIP_HD bool value_map_hit(uint32_t from, uint64_t x, uint64_t key) {
    if (from == ZHIP_VT_F32) {
        const float a = vt_f32(x), k = vt_f32(key);
        return (a != a && k != k) || a == k;
    }
    if (from == ZHIP_VT_F64) {
        const double a = vt_f64(x), k = vt_f64(key);
        return (a != a && k != k) || a == k;
    }
    const uint64_t m = vt_mask(from);
    return (x & m) == (key & m);
}

ZHIP_HD uint64_t value_cast(const zhip_value_op& op, uint32_t from, uint32_t to, uint64_t x, uint32_t& err) {
    for (uint32_t k = 0; k < op.n_map && k < ZHIP_VALUE_MAX_MAP; ++k)
        if (value_map_hit(from, x, op.map_key[k])) return op.map_val[k] & vt_mask(to);
    if (from == ZHIP_VT_F32) return value_cast_float<float>(op, to, vt_f32(x), err);
    if (from == ZHIP_VT_F64) return value_cast_float<double>(op, to, vt_f64(x), err);
    const int64_t v = vt_int(from, x);
    if (to == ZHIP_VT_F32) return vt_bits((float)v);   // exact: at most 16 bits
    if (to == ZHIP_VT_F64) return vt_bits((double)v);  // exact: at most 32 bits
    const int64_t lo = vt_min(to), hi = vt_max(to);
    if (v < lo || v > hi) {
        if (op.out_of_range == ZHIP_VO_CLAMP) return (uint64_t)(v < lo ? lo : hi) & vt_mask(to);
        if (op.out_of_range == ZHIP_VO_WRAP) return (uint64_t)v & vt_mask(to);
        err |= ZHIP_VE_CAST_RANGE;
        return 0;
    }
    return (uint64_t)v & vt_mask(to);
}

// One element: raw bits of the a side's dtype -> raw bits of the b side's.
// The stage that fails ends the element (its later stage never runs, as the
// reference raises between the codecs) and the element is zero bits.
ZHIP_HD uint64_t value_map_one(const zhip_value_op& op, uint64_t x, uint32_t& err) {
    uint32_t e = 0;
    if (op.encode) {
        if (op.stages & ZHIP_VS_SCALE_OFFSET) x = value_scale_offset(op, x, e);
        if (!e && (op.stages & ZHIP_VS_CAST)) x = value_cast(op, op.array_dt, op.stored_dt, x, e);
    } else {
        if (op.stages & ZHIP_VS_CAST) x = value_cast(op, op.stored_dt, op.array_dt, x, e);
        if (!e && (op.stages & ZHIP_VS_SCALE_OFFSET)) x = value_scale_offset(op, x, e);
    }
    err |= e;
    return e ? 0 : x;
}

ZHIP_HD uint32_t value_a_dt(const zhip_value_op& op) { return op.encode ? op.array_dt : op.stored_dt; }
ZHIP_HD uint32_t value_b_dt(const zhip_value_op& op) { return op.encode ? op.stored_dt : op.array_dt; }

// Byte offsets (relative to a and b) of element e of an item, e < it.total
ZHIP_HD void value_addr(const zhip_value_item& it, uint32_t e, int64_t& ao, int64_t& bo) {
    ao = it.a_base;
    bo = it.b_base;
    for (int d = (int)it.ndim - 1; d >= 0; --d) {
        const zhip_value_dim& D = it.dims[d];
        uint32_t k = e;
        if (d > 0) {
            const uint32_t q = fdiv_apply(e, D.div.m, D.div.s);
            k = e - q * D.count;
            e = q;
        }
        ao += (int64_t)k * D.sa;
        bo += (int64_t)k * D.sb;
    }
}

// the kernel's fence (and the hook's bounds verdict)
ZHIP_HD bool value_inside(int64_t ao, int64_t bo, uint64_t a_size, uint64_t b_size, uint32_t a_bytes, uint32_t b_bytes) {
    return ao >= 0 && bo >= 0 && (uint64_t)ao + a_bytes <= a_size && (uint64_t)bo + b_bytes <= b_size;
}

// Elements one lane takes at a time on the vector path: 16 bytes of the
// narrower side, at most 8 elements (so 8 bytes of a 1-byte side).
ZHIP_HD uint32_t value_vec_width(uint32_t asz, uint32_t bsz) {
    const uint32_t n = asz < bsz ? asz : bsz;
    return n == 1 ? 8u : 16u / n > 8u ? 8u : 16u / n;
}

// Whether an item takes the vector path: innermost dimension contiguous on
// both sides with a count that is a multiple of the vector width, every row
// (base and outer strides) aligned to the access size of its side.
ZHIP_HD bool value_vec_ok(const zhip_value_item& it, uint64_t a_addr, uint64_t b_addr, uint32_t asz, uint32_t bsz) {
    const uint32_t V = value_vec_width(asz, bsz);
    const zhip_value_dim& L = it.dims[it.ndim - 1];
    if (L.sa != (int64_t)asz || L.sb != (int64_t)bsz || L.count % V != 0) return false;
    const uint64_t al_a = (V * asz < 16u ? V * asz : 16u) - 1u, al_b = (V * bsz < 16u ? V * bsz : 16u) - 1u;
    if (((a_addr + (uint64_t)it.a_base) & al_a) || ((b_addr + (uint64_t)it.b_base) & al_b)) return false;
    for (uint32_t d = 0; d + 1 < it.ndim; ++d) {
        const zhip_value_dim& D = it.dims[d];
        if (D.count > 1 && (((uint64_t)D.sa & al_a) || ((uint64_t)D.sb & al_b))) return false;
    }
    return true;
}

int value_launch(const zhip_value_op& op, const zhip_value_item* d_items, uint32_t n_items,
                 const uint32_t* d_tile_prefix, uint32_t n_tiles, const zhip_status* d_status, const void* a,
                 uint64_t a_size, void* b, uint64_t b_size, uint32_t* d_err, uint32_t* d_nonempty,
                 void* stream);  // values.hip; 0 or a hipError_t

// value_map.cpp: 0 or a ZHIP_E_* code with *msg set
int value_check_op(const zhip_value_op* op, const char** msg);
int value_emulate(const zhip_value_op& op, const zhip_value_item* items, uint32_t n_items,
                  const uint32_t* tile_prefix, uint32_t n_tiles, const zhip_status* status, uint32_t n_status,
                  const void* a, uint64_t a_size, void* b, uint64_t b_size, uint32_t* err, uint32_t* nonempty,
                  const char** msg);

}  // namespace zhip
