// Host side of zhip_value_map (include/zarrhip.h): the checks of the op record
// and the CPU hook zhip_emulate_value_map, which walks the kernel's tiles and
// items with the kernel's own per-element function (zhip_values.h).  The
// host codec classes cast and encode fill values through the hook, so the
// arithmetic is stated once.
#include <cstring>

#include "../../include/zarrhip.h"
#include "zhip_internal.h"
#include "zhip_select.h"
#include "zhip_values.h"

namespace zhip {

static bool so_dtype(uint32_t dt) { return dt <= ZHIP_VT_U32 || dt == ZHIP_VT_F32 || dt == ZHIP_VT_F64; }

// array dtype -> stored dtype pairs cast_value is served for
static bool cast_pair(uint32_t arr, uint32_t st) {
    if (arr == st) return false;
    if (arr == ZHIP_VT_F32) return st <= ZHIP_VT_U16;
    if (arr == ZHIP_VT_F64) return st <= ZHIP_VT_U32;
    return arr <= ZHIP_VT_I64 && st <= ZHIP_VT_I64;
}

int value_check_op(const zhip_value_op* op, const char** msg) {
    if (!op) return *msg = "null argument", ZHIP_E_INVALID;
    if (op->encode > 1 || op->array_dt > ZHIP_VT_F64 || op->stored_dt > ZHIP_VT_F64 || op->stages == 0 ||
        op->stages > (ZHIP_VS_SCALE_OFFSET | ZHIP_VS_CAST) || op->rounding > ZHIP_VR_NEAREST_AWAY ||
        op->out_of_range > ZHIP_VO_WRAP || op->fill_nan > 1)
        return *msg = "value op field out of range", ZHIP_E_INVALID;
    if (op->n_map > ZHIP_VALUE_MAX_MAP) return *msg = "more than 8 scalar_map entries", ZHIP_E_UNSUPPORTED;
    if (op->stages & ZHIP_VS_SCALE_OFFSET) {
        if (!so_dtype(op->array_dt)) return *msg = "scale_offset dtype outside the served table", ZHIP_E_UNSUPPORTED;
        if (!vt_float(op->array_dt) && vt_int(op->array_dt, op->scale) == 0)
            return *msg = "scale_offset scale must be non-zero", ZHIP_E_INVALID;
    }
    if (op->stages & ZHIP_VS_CAST) {
        if (!cast_pair(op->array_dt, op->stored_dt))
            return *msg = "cast_value dtype pair outside the served table", ZHIP_E_UNSUPPORTED;
    } else if (op->stored_dt != op->array_dt) {
        return *msg = "stored dtype differs from the array dtype without a cast", ZHIP_E_INVALID;
    }
    return ZHIP_OK;
}

static uint64_t host_load(const uint8_t* p, uint32_t sz) {
    uint64_t v = 0;
    memcpy(&v, p, sz);  // little-endian host
    return v;
}

int value_emulate(const zhip_value_op& op, const zhip_value_item* items, uint32_t n_items,
                  const uint32_t* tile_prefix, uint32_t n_tiles, const zhip_status* status, uint32_t n_status,
                  const void* a, uint64_t a_size, void* b, uint64_t b_size, uint32_t* err, uint32_t* nonempty,
                  const char** msg) {
    if (tile_prefix[0] != 0 || tile_prefix[n_items] != n_tiles) return *msg = "tile prefix ends", ZHIP_E_INVALID;
    for (uint32_t i = 0; i < n_items; ++i) {
        const zhip_value_item& it = items[i];
        if (it.ndim < 1 || it.ndim > ZHIP_MAX_DIMS) return *msg = "item ndim", ZHIP_E_INVALID;
        if (it.flags & ~(ZHIP_VI_MISSING | ZHIP_VI_STATUS)) return *msg = "item flags", ZHIP_E_INVALID;
        if ((it.flags & ZHIP_VI_STATUS) && (!status || it.status >= n_status))
            return *msg = "item status index", ZHIP_E_INVALID;
        uint64_t total = 1;
        for (uint32_t d = 0; d < it.ndim; ++d) {
            const zhip_value_dim& D = it.dims[d];
            if (D.count < 1 || D.count >= (1u << 31)) return *msg = "dimension count", ZHIP_E_INVALID;
            const zhip_fdiv f = make_fdiv(D.count);
            if (f.m != D.div.m || f.s != D.div.s) return *msg = "dimension divisor", ZHIP_E_INVALID;
            total *= D.count;
            if (total >= (1ull << 31)) return *msg = "item total", ZHIP_E_INVALID;
        }
        if (total != it.total) return *msg = "item total != prod(count)", ZHIP_E_INVALID;
        if (tile_prefix[i + 1] - tile_prefix[i] != (it.total + ZHIP_VALUE_TILE - 1) / ZHIP_VALUE_TILE)
            return *msg = "tile prefix step", ZHIP_E_INVALID;
    }
    const uint32_t asz = vt_size(value_a_dt(op)), bsz = vt_size(value_b_dt(op));
    const uint64_t fillb = op.fill & vt_mask(op.array_dt);
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
        const uint32_t ii = select_find_item(tile_prefix, n_items, tile);
        const zhip_value_item& it = items[ii];
        bool missing = false;
        if (!op.encode) {
            if (it.flags & ZHIP_VI_MISSING) missing = true;
            else if (it.flags & ZHIP_VI_STATUS) missing = status[it.status].code == ZHIP_ST_MISSING;
        }
        const uint32_t base = (tile - tile_prefix[ii]) * ZHIP_VALUE_TILE;
        for (uint32_t k = 0; k < ZHIP_VALUE_TILE; ++k) {
            const uint32_t e = base + k;
            if (e >= it.total) break;
            int64_t ao, bo;
            value_addr(it, e, ao, bo);
            if (!value_inside(ao, bo, a_size, b_size, asz, bsz))
                return *msg = "element offset outside its buffer", ZHIP_E_BOUNDS;
            uint64_t y = fillb;
            if (!missing) {
                const uint64_t x = host_load((const uint8_t*)a + ao, asz);
                if (op.encode && nonempty && !value_eq_fill(op, x)) nonempty[ii] = 1u;
                y = value_map_one(op, x, *err);
            }
            memcpy((uint8_t*)b + bo, &y, bsz);
        }
    }
    return ZHIP_OK;
}

}  // namespace zhip
