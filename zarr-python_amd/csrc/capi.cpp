// C ABI of zarr_hip (include/zarrhip.h): plan building (host GF(2) math, one
// upload), launches, error reporting, and CPU self-tests of the CRC-combine
// algebra the kernels rely on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/zarrhip.h"
#include "zhip_gf2.h"
#include "zhip_internal.h"
#include "zhip_axis.h"
#include "zhip_fill_eq.h"
#include "zhip_points.h"
#include "zhip_select.h"
#include "zhip_values.h"

using namespace zhip;

namespace {

thread_local std::string g_err;

int set_err(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return set_err(ZHIP_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_));  \
    } while (0)

uint32_t crc_bytewise(const uint8_t* p, size_t n) {
    const uint32_t* T = byte_tables().T;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = (c >> 8) ^ T[(c ^ p[i]) & 255u];
    return ~c;
}

// Host CRC-32C for the host stage of a chain (zhip_crc32c_host): the x86
// crc32 instruction, 8 bytes per step, as google-crc32c uses on this host;
// bytewise tables where the CPU lacks SSE4.2.
__attribute__((target("sse4.2"))) uint32_t crc_sse42(const uint8_t* p, size_t n) {
    uint64_t c = 0xFFFFFFFFu;
    while (n && (reinterpret_cast<uintptr_t>(p) & 7u)) {
        c = __builtin_ia32_crc32qi((uint32_t)c, *p++);
        --n;
    }
    for (; n >= 8; n -= 8, p += 8) {
        uint64_t w;
        memcpy(&w, p, 8);
        c = __builtin_ia32_crc32di(c, w);
    }
    while (n--) c = __builtin_ia32_crc32qi((uint32_t)c, *p++);
    return ~(uint32_t)c;
}

}  // namespace

namespace zhip {
#if ZHIP_TUNING
uint32_t g_tune_bits = 0;
int g_tune_blocks = 0;
int g_tune_arm = 0;
#endif
}

extern "C" {

int zhip_tuning_build(void) { return ZHIP_TUNING; }

int zhip_set_tuning(int key, int value) {
    switch (key) {
#if ZHIP_TUNING
        case ZHIP_TUNE_MAX_GRID: g_tune_max_grid = value; return ZHIP_OK;
        case ZHIP_TUNE_ABLATION: g_tune_bits = (uint32_t)value; return ZHIP_OK;
        case ZHIP_TUNE_BLOCKS: g_tune_blocks = value; return ZHIP_OK;
        case ZHIP_TUNE_ARM: g_tune_arm = value; return ZHIP_OK;
#else
        case ZHIP_TUNE_MAX_GRID:
        case ZHIP_TUNE_ABLATION:
        case ZHIP_TUNE_BLOCKS:
        case ZHIP_TUNE_ARM:
            if (value == 0) return ZHIP_OK;  // the production setting
            return set_err(ZHIP_E_UNSUPPORTED, "kernel tuning knobs exist only in the tuning build "
                                               "(libzarrhip_tune.so, make tune)");
#endif
        case ZHIP_TUNE_STAGE_STREAMS: zhip_stage_set_streams(value >= 2 ? 2u : 1u); return ZHIP_OK;
        case ZHIP_TUNE_STAGE_COPY: zhip_stage_set_copy(value ? 1u : 0u); return ZHIP_OK;
        default: return set_err(ZHIP_E_INVALID, "unknown tuning key");
    }
}

int zhip_dv_check(const zhip_dv_ref* d_refs, uint32_t n_refs, void* stream) {
    if (n_refs && !d_refs) return set_err(ZHIP_E_INVALID, "null argument");
    if (n_refs > 65535u) return set_err(ZHIP_E_INVALID, "too many launches in one check");
    if (zhip::launch_dv_check(d_refs, n_refs, static_cast<hipStream_t>(stream)) != ZHIP_OK)
        return set_err(ZHIP_E_HIP, "k_dv_check launch failed");
    return ZHIP_OK;
}

int zhip_abi_version(void) { return ZHIP_ABI_VERSION; }

int zhip_debug_stamps(uint64_t* host_out, uint32_t n_wg) {
    if (!host_out) return set_err(ZHIP_E_INVALID, "null argument");
    if (zhip::debug_stamps(host_out, n_wg) != 0) return set_err(ZHIP_E_HIP, "hipMemcpyFromSymbol failed");
    return ZHIP_OK;
}

const char* zhip_last_error(void) { return g_err.c_str(); }

int zhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static void plan_affine(zhip_plan* p);

int zhip_plan_create(const zhip_layout* layout, zhip_plan** out) {
    if (!layout || !out) return set_err(ZHIP_E_INVALID, "null argument");
    const zhip_layout& L = *layout;
    if (L.ndim < 1 || L.ndim > ZHIP_MAX_DIMS) return set_err(ZHIP_E_UNSUPPORTED, "ndim must be 1..8");
    if (!(L.itemsize == 1 || L.itemsize == 2 || L.itemsize == 4 || L.itemsize == 8))
        return set_err(ZHIP_E_UNSUPPORTED, "itemsize must be 1, 2, 4 or 8");
    if ((L.flags & ZHIP_LF_COMPLEX) && ((L.flags & ZHIP_LF_FLOAT) || L.itemsize != 8))
        return set_err(ZHIP_E_INVALID, "ZHIP_LF_COMPLEX is an 8-byte item of two float32, without ZHIP_LF_FLOAT");
    uint64_t n = (uint64_t)L.itemsize;
    for (int d = 0; d < L.ndim; ++d) {
        if (L.shape[d] < 0) return set_err(ZHIP_E_INVALID, "negative shape");
        n *= (uint64_t)L.shape[d];
    }
    if (n != L.nbytes) return set_err(ZHIP_E_INVALID, "nbytes != prod(shape)*itemsize");
    if (n >= (1ull << 31) - 8192) return set_err(ZHIP_E_UNSUPPORTED, "chunk payload must be < 2 GiB");
    zhip_plan* p = new (std::nothrow) zhip_plan();
    if (!p) return set_err(ZHIP_E_INVALID, "out of memory");
    p->layout = L;
    p->E = (uint32_t)((n + 15) & ~15ull);
    p->kblocks = (g_tune_blocks == 4 || g_tune_blocks == 16) ? (uint32_t)g_tune_blocks : (uint32_t)kDefaultBlocks;
    if (L.flags & ZHIP_LF_NO_WRITE || !(L.flags & ZHIP_LF_CRC)) p->kblocks = kDefaultBlocks;
    p->seg = (uint32_t)kWgStride * p->kblocks;
    p->nseg = p->E == 0 ? 1u : (p->E + p->seg - 1) / p->seg;
    // k_decode_il: groups of S x 8 steps must tile the chunk's steps
    p->il_S = 0;
    if (p->kblocks == (uint32_t)kDefaultBlocks && (L.flags & ZHIP_LF_CRC) && !(L.flags & ZHIP_LF_NO_WRITE)) {
        const uint32_t n_steps = p->nseg * (uint32_t)kDefaultBlocks;
        for (uint32_t S = 8; S >= 2 && !p->il_S; S /= 2)
            if (n_steps % (S * (uint32_t)kDefaultBlocks) == 0) p->il_S = S;
    }
    // k_decode_xw: 8 KiB spans (whole-row layouts keep E a multiple of 4 KiB)
    p->xw_P = 0;
    p->xw_nsub = 0;
    if (p->kblocks == (uint32_t)kDefaultBlocks && (L.flags & ZHIP_LF_CRC) && !(L.flags & ZHIP_LF_NO_WRITE)) {
        p->xw_P = p->nseg * 4u;
        if (p->xw_P > 32u && p->xw_P <= 1024u) p->xw_nsub = (p->xw_P + 31u) / 32u;
    }
    p->R = (uint64_t)p->E + kWgStride;
    p->c_inv = xpow8_inv(p->R - n);
    p->c3 = gf_mul(xpow8(n), 0xFFFFFFFFu);
    for (int op = 0; op < 4; ++op) p->hx[op] = xpow8((uint64_t)kWgStride - 4u * op);
    for (int a = 0; a < 16; ++a) p->kq[a] = xpow8((uint64_t)kWgStride - 256u * a);
    for (int b = 0; b < 16; ++b) p->kq[16 + b] = xpow8_inv(16u * b);
    for (int d = 0; d < ZHIP_MAX_DIMS; ++d) p->dshape[d] = make_fdiv(d < L.ndim && L.shape[d] > 0 ? (uint32_t)L.shape[d] : 1u);
    p->row_bytes = (uint32_t)L.shape[L.ndim - 1] * (uint32_t)L.itemsize;
    p->drow = make_fdiv(p->row_bytes ? p->row_bytes : 1u);
    // fill pattern replicated to 16 bytes
    uint8_t f16[16];
    for (int i = 0; i < 16; ++i) f16[i] = L.fill[i % L.itemsize];
    std::memcpy(p->fill, f16, 16);
    p->idx_nbytes = 0;
    if (L.flags & ZHIP_LF_SHARDED) {
        const uint64_t ni = 16ull * L.n_inner;
        p->idx_nbytes = (uint32_t)ni;
        p->idx_E = (uint32_t)((ni + 15) & ~15ull);
        p->idx_c_inv = xpow8_inv((uint64_t)p->idx_E + kWgStride - ni);
        p->idx_c3 = gf_mul(xpow8(ni), 0xFFFFFFFFu);
    }
    p->device = -1;
    p->max_grid = 2048;
    p->d_tables = nullptr;
    p->d_tile_tables = nullptr;
    p->tile4 = 0;
    p->gd = -1;
    p->n_groups = 0;
    p->n_sub = 0;
    // tile mode: a stored dim (not the innermost) that is contiguous in out
    p->tq = -1;
    {
        uint64_t st = (uint64_t)L.itemsize;
        for (int d = L.ndim - 1; d >= 0; --d) {
            p->sstride[d] = (uint32_t)st;
            st *= (uint64_t)L.shape[d];
        }
        for (int d = L.ndim; d < ZHIP_MAX_DIMS; ++d) p->sstride[d] = 0;
        if (!(L.flags & ZHIP_LF_NO_WRITE) && L.ndim >= 2 && p->row_bytes % 16 == 0 && p->row_bytes > 0)
            for (int d = 0; d < L.ndim - 1; ++d)
                if (L.out_stride[d] == L.itemsize && L.shape[d] > 1) { p->tq = d; break; }
        if (p->tq >= 0) {
            p->n_qb = (uint32_t)((L.shape[p->tq] + kTileRows - 1) / kTileRows);
            p->n_cb = (p->row_bytes + kTileCols - 1) / kTileCols;
            uint64_t other = 1;
            for (int d = 0; d < L.ndim - 1; ++d)
                if (d != p->tq) other *= (uint64_t)L.shape[d];
            p->t_per_chunk = (uint32_t)(other * p->n_qb * p->n_cb);
            // k_decode_tile4 eligibility: full tiles, and every group of 4
            // consecutive tiles at one uniform base step (so one table multiply
            // carries a thread's Horner state from tile to tile)
            const uint32_t T = p->t_per_chunk;
            const std::vector<uint64_t> base = tile_bases(*p);
            const uint64_t step = T >= 2 ? base[1] - base[0] : 0;
            bool t4 = (L.shape[p->tq] % kTileRows) == 0 && (p->row_bytes % kTileCols) == 0 && T % 4 == 0 &&
                      T >= 4 && base[1] > base[0];
            for (uint32_t ti = 0; t4 && ti < T; ++ti)
                if (base[ti] != base[ti & ~3u] + (uint64_t)(ti & 3u) * step) t4 = false;
            p->tile4 = t4 ? 1u : 0u;
            p->tile4_step = step;
            // k_decode_tile4w over consecutive tile pairs where tile4 declines
            p->tile2 = (!t4 && (L.flags & ZHIP_LF_CRC) && (L.shape[p->tq] % kTileRows) == 0 &&
                        (p->row_bytes % kTileCols) == 0 && T % 2 == 0 && T >= 2 && T / 2 <= 65535u) ? 1u : 0u;
            // k_encode_tileg: the innermost other stored dim with shape % 4 == 0
            for (int d = L.ndim - 2; d >= 0 && p->gd < 0; --d)
                if (d != p->tq && L.shape[d] % 4 == 0) p->gd = d;
            if (p->gd >= 0) {
                p->n_groups = T / 4;
                // two-level arrival (subgroups of 16 workgroups) for 17..256 groups
                p->n_sub = (p->n_groups > 16u && p->n_groups <= 256u) ? (p->n_groups + 15u) / 16u : 0u;
            }
        }
    }
    plan_affine(p);
    plan_layout(*p);
    *out = p;
    return ZHIP_OK;
}

// Upload the constant tables to the current device (done once per plan and device).
int zhip_plan_upload(zhip_plan* p) {
    if (!p) return set_err(ZHIP_E_INVALID, "null plan");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (p->d_tables && p->device == dev) return ZHIP_OK;
    const std::vector<uint32_t> h = build_row_tables(*p);
    if (p->d_tables) (void)hipFree(p->d_tables);
    p->d_tables = nullptr;
    HIP_TRY(hipMalloc(&p->d_tables, h.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(p->d_tables, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (p->tq >= 0) {
        const std::vector<uint32_t> ht = build_tile_tables(*p);
        if (p->d_tile_tables) (void)hipFree(p->d_tile_tables);
        p->d_tile_tables = nullptr;
        HIP_TRY(hipMalloc(&p->d_tile_tables, ht.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(p->d_tile_tables, ht.data(), ht.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        p->max_grid = prop.multiProcessorCount * 8;
    p->device = dev;
    return ZHIP_OK;
}

int zhip_plan_destroy(zhip_plan* p) {
    if (!p) return ZHIP_OK;
    if (p->d_tables) (void)hipFree(p->d_tables);
    if (p->d_tile_tables) (void)hipFree(p->d_tile_tables);
    delete p;
    return ZHIP_OK;
}

int zhip_plan_kernel_flags(const zhip_plan* p, uint32_t* flags) {
    if (!p || !flags) return set_err(ZHIP_E_INVALID, "null argument");
    *flags = (p->tile4 ? ZHIP_PK_TILE4 : 0u) | (p->tile4 && p->t_per_chunk <= 64 ? ZHIP_PK_TILE4_ENCODE : 0u) |
             (p->tq >= 0 ? ZHIP_PK_TILE : 0u) |
             (p->gd >= 0 && p->layout.shape[p->tq] % (16 / p->layout.itemsize) == 0 ? ZHIP_PK_TILEG : 0u) |
             (p->il_S == 8u && (p->layout.flags & ZHIP_LF_CRC) ? ZHIP_PK_IL : 0u);
    return ZHIP_OK;
}

int zhip_plan_info(const zhip_plan* p, uint32_t* units_per_chunk, uint32_t* workspace_words) {
    if (!p) return set_err(ZHIP_E_INVALID, "null plan");
    if (units_per_chunk) *units_per_chunk = p->nseg;
    // + the grouped kernels' / k_decode_xw's arrival subwords
    // (CRC layouts: >= kPubLine, the il / tile4 publication lines)
    // (k_decode_tilegw's two-tile form: arrival subwords for twice the groups)
    const TableLayout& T = p->tl;
    const bool tg2w = T.tg2w.n != 0;
    uint32_t n_sub2 = (tg2w && 2 * p->n_groups > 16u && 2 * p->n_groups <= 256u)
                          ? (2 * p->n_groups + 15u) / 16u : 0u;
    // (the tile-pair decode, tuning builds: subwords of 16 for 33..256 workgroups per chunk)
    const uint32_t wpc2 = T.tile2_tab.n ? p->t_per_chunk / 2u : 0u;
    if (wpc2 > 32u && wpc2 <= 256u) n_sub2 = std::max(n_sub2, (wpc2 + 15u) / 16u);
    // (k_decode_tile4w, four tiles per workgroup: the same subwords past 32 workgroups per chunk)
    const uint32_t wpc4 = T.t4w.tab.n ? p->t_per_chunk / 4u : 0u;
    if (wpc4 > 32u && wpc4 <= 256u) n_sub2 = std::max(n_sub2, (wpc4 + 15u) / 16u);
    uint32_t w = std::max(4 + 2 * std::max(std::max(p->n_sub, p->xw_nsub), n_sub2),
                          (p->layout.flags & ZHIP_LF_CRC) ? kPubLine : 0u);
    // (k_decode_tilegw's two-tile form, tuning arm 47's k_encode_tileg: the
    // arrival words on 128-byte lines of their own, tileg_arrive SPR)
    if (tg2w) w = std::max(w, kPubLine * (1u + (ZHIP_TUNING ? std::max(p->n_sub, n_sub2) : n_sub2)));
    // (tuning arm 49: k_decode_il / k_decode_ilw / two-tile k_decode_tile4w publish
    // through two subwords on lines of their own)
    if (ZHIP_TUNING && (p->layout.flags & ZHIP_LF_CRC) && (p->il_S || p->tile4)) w = std::max(w, 3u * kPubLine);
    // (tuning arm 39, tile pairs past 32 workgroups per chunk: spread subwords)
    if (wpc2 > 32u && wpc2 <= 256u) w = std::max(w, kPubLine * (1u + (wpc2 + 15u) / 16u));
    if (workspace_words) *workspace_words = w;
    return ZHIP_OK;
}

int zhip_decode(const zhip_plan* plan, const void* src, uint64_t src_size, void* out,
                const zhip_chunk* d_chunks, uint32_t n_chunks, const zhip_sel* d_sels,
                zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_errflag, uint32_t decode_flags,
                void* stream) {
    return zhip_decode_indexed(plan, src, src_size, out, d_chunks, n_chunks, d_sels, d_status, d_workspace,
                               d_errflag, nullptr, 0, nullptr, decode_flags, stream);
}

int zhip_decode_indexed(const zhip_plan* plan, const void* src, uint64_t src_size, void* out,
                        const zhip_chunk* d_chunks, uint32_t n_chunks, const zhip_sel* d_sels,
                        zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_errflag,
                        const zhip_chunk* d_index_chunks, uint32_t n_index, zhip_status* d_index_status,
                        uint32_t decode_flags, void* stream) {
    return zhip_decode_predicted(plan, src, src_size, out, d_chunks, n_chunks, d_sels, d_status, d_workspace,
                                 d_errflag, d_index_chunks, n_index, d_index_status, decode_flags, nullptr, stream);
}

int zhip_decode_predicted(const zhip_plan* plan, const void* src, uint64_t src_size, void* out,
                          const zhip_chunk* d_chunks, uint32_t n_chunks, const zhip_sel* d_sels,
                          zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_errflag,
                          const zhip_chunk* d_index_chunks, uint32_t n_index, zhip_status* d_index_status,
                          uint32_t decode_flags, const zhip_predict* pred, void* stream) {
    return zhip_decode_mapped(plan, src, src_size, out, d_chunks, n_chunks, d_sels, d_status, d_workspace,
                              d_errflag, d_index_chunks, n_index, d_index_status, decode_flags, pred, nullptr,
                              stream);
}

uint64_t zhip_rows_map_len(const zhip_plan* plan, uint32_t n_sels) {
    if (!plan) return 0;
    return (uint64_t)n_sels * plan->nseg * (uint64_t)kDefaultBlocks;
}

// The destination arithmetic of the row decode (per step: row R of the
// chunk's flattened leading dims, its place in dims 0..ndim-2 and in the
// selection), evaluated once per (selection, unit, step) on the host.
// Entry of the row map for the step whose first output byte is base_o
// (>= 0) of the chunk: 0 ok (e set, possibly empty), 1 offset beyond 32 bits.
static int rows_entry(const zhip_layout& L, uint32_t shift, const zhip_sel& sel, int64_t base_o, zhip_rowblk& e) {
    const int nd = L.ndim, nd2 = nd - 2;
    const int64_t rps = (int64_t)kWgStride >> shift;  // rows per step
    const int64_t sy = L.shape[nd - 2];
    const int64_t oy = L.out_stride[nd - 2];
    const int64_t sy0 = sel.start[nd2], cy = sel.count[nd2];
    e.rel = 0;
    e.lo = e.hi = 0;
    const int64_t R = base_o >> shift;
    int64_t r = R / sy;
    const int64_t y0 = R - r * sy;
    int64_t dst = (y0 - sy0) * oy;
    bool ok = true;
    for (int d = nd2 - 1; d >= 0; --d) {
        const int64_t qd = d > 0 ? r / L.shape[d] : 0;
        const int64_t rel = r - qd * L.shape[d] - sel.start[d];
        r = qd;
        ok = ok && rel >= 0 && rel < sel.count[d];
        dst += rel * L.out_stride[d];
    }
    const int64_t lo = std::min(std::max(sy0 - y0, (int64_t)0), rps);
    const int64_t hi = std::min(std::max(sy0 - y0 + cy, (int64_t)0), rps);
    if (!ok || hi <= lo) return 0;
    if (dst < INT32_MIN || dst > INT32_MAX) return 1;
    e.rel = (int32_t)dst;
    e.lo = (uint16_t)lo;
    e.hi = (uint16_t)hi;
    return 0;
}

static bool rows_layout(const zhip_plan* plan) {  // zhip_rows_map's admission
    const zhip_layout& L = plan->layout;
    const uint32_t rb = plan->row_bytes;
    const int nd = L.ndim;
    return !(nd < 2 || rb < 16 || rb > (uint32_t)kWgStride || (rb & (rb - 1)) != 0 ||
             (uint32_t)L.shape[nd - 2] % ((uint32_t)kWgStride / rb) != 0 ||
             plan->seg != (uint32_t)kWgStride * kDefaultBlocks);
}

// The whole-chunk selection's row map in two-level affine form (ZHIP_DF_WHOLE
// launches): rel(st) = (st >> sh) B + (st & (2^sh - 1)) C + D with every row
// of every step written, st = (base_o - lo_frame) / 4 KiB; only chunks that
// end on a unit boundary (lo_frame 0).  aff_ok = 0 when no shift fits.
static void plan_affine(zhip_plan* p) {
    p->aff_ok = 0;
    if (!rows_layout(p) || p->E != p->nseg * p->seg || p->nseg == 0) return;
    const zhip_layout& L = p->layout;
    const uint32_t shift = (uint32_t)__builtin_ctz(p->row_bytes);
    const uint16_t rps = (uint16_t)((uint32_t)kWgStride >> shift);
    zhip_sel full{};
    for (int d = 0; d < L.ndim; ++d) full.count[d] = (int32_t)L.shape[d];
    const uint32_t n_st = p->nseg * (uint32_t)kDefaultBlocks;
    std::vector<int32_t> rel(n_st);
    for (uint32_t st = 0; st < n_st; ++st) {
        zhip_rowblk e;
        if (rows_entry(L, shift, full, (int64_t)kWgStride * st, e) || e.lo != 0 || e.hi != rps) return;
        rel[st] = e.rel;
    }
    for (uint32_t sh = 0; sh <= 12; ++sh) {
        const uint32_t mask = (1u << sh) - 1u;
        const int64_t D = rel[0];
        const int64_t C = (sh > 0 && n_st > 1) ? (int64_t)rel[1] - D : 0;
        const int64_t B = ((1u << sh) < n_st) ? (int64_t)rel[1u << sh] - D : 0;
        bool fit = true;
        for (uint32_t st = 0; st < n_st && fit; ++st)
            fit = (int64_t)(st >> sh) * B + (int64_t)(st & mask) * C + D == rel[st];
        if (fit && B >= INT32_MIN && B <= INT32_MAX && C >= INT32_MIN && C <= INT32_MAX) {
            p->aff_ok = 1;
            p->aff_sh = sh;
            p->aff_B = (int32_t)B;
            p->aff_C = (int32_t)C;
            p->aff_D = (int32_t)D;
            return;
        }
    }
}

extern "C++" {
template <class P>
static void set_affine(P& p, const zhip_plan* plan) {  // DecodeParams / EncodeParams
    p.aff_sh = plan->aff_sh;
    p.aff_mask = (1u << plan->aff_sh) - 1u;
    p.aff_B = plan->aff_B;
    p.aff_C = plan->aff_C;
    p.aff_D = plan->aff_D;
}
}

int zhip_rows_map(const zhip_plan* plan, const zhip_sel* h_sels, uint32_t n_sels, zhip_rowblk* h_map,
                  uint64_t map_len) {
    if (!plan) return set_err(ZHIP_E_INVALID, "null plan");
    if (n_sels && (!h_sels || !h_map)) return set_err(ZHIP_E_INVALID, "null host pointer");
    if (map_len < zhip_rows_map_len(plan, n_sels)) return set_err(ZHIP_E_INVALID, "row map too short");
    if (!rows_layout(plan)) return set_err(ZHIP_E_UNSUPPORTED, "not a whole-row layout with 32 KiB units");
    const zhip_layout& L = plan->layout;
    const uint32_t shift = (uint32_t)__builtin_ctz(plan->row_bytes);
    for (uint32_t s = 0; s < n_sels; ++s) {
        for (uint32_t u = 0; u < plan->nseg; ++u) {
            const int64_t seg_lo = (int64_t)(int32_t)plan->E - (int64_t)(u + 1) * plan->seg;
            for (int k = 0; k < kDefaultBlocks; ++k) {
                zhip_rowblk& e = h_map[((uint64_t)s * plan->nseg + u) * kDefaultBlocks + k];
                e.rel = 0;
                e.lo = e.hi = 0;
                const int64_t base_o = seg_lo + (int64_t)kWgStride * k;
                if (base_o < 0) continue;  // before the chunk start: nothing written
                if (rows_entry(L, shift, h_sels[s], base_o, e))
                    return set_err(ZHIP_E_UNSUPPORTED, "row offset does not fit 32 bits");
            }
        }
    }
    return ZHIP_OK;
}

// The argument checks and kernel parameters of one zhip_decode_mapped call
// (zhip_decode_mapped launches them, zhip_decode_mapped_multi several in one
// grid).  `empty`: nothing to decode, p is not filled.
extern "C++" {
// Device pointers of the plan's regions (plan->tl); null where a region is absent.
static const uint32_t* row_at(const zhip_plan* plan, const Region& r) { return r.n ? plan->d_tables + r.off : nullptr; }
static const uint32_t* tile_at(const zhip_plan* plan, const Region& r) {
    return r.n ? plan->d_tile_tables + r.off : nullptr;
}
template <class T>
static const T* tile_at(const zhip_plan* plan, const Region& r) {
    return reinterpret_cast<const T*>(tile_at(plan, r));
}

// k_decode_il / k_encode_il's table set: il_choose's interleave and its four pointers
struct IlTables {
    uint32_t S;
    const uint32_t *tab, *klane, *kidx, *basis;
};
static IlTables il_tables(const zhip_plan* plan, uint32_t want) {
    const IlChoice c = il_choose(*plan, want);
    return {c.S, row_at(plan, c.set->tab), row_at(plan, c.set->klane), row_at(plan, c.set->kidx),
            row_at(plan, c.set->basis)};
}

static int mapped_params(const zhip_plan* plan, const void* src, uint64_t src_size, void* out,
                         const zhip_chunk* d_chunks, uint32_t n_chunks, const zhip_sel* d_sels,
                         zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_errflag,
                         const zhip_chunk* d_index_chunks, uint32_t n_index, zhip_status* d_index_status,
                         uint32_t decode_flags, const zhip_predict* pred, const zhip_rowblk* d_rowmap,
                         DecodeParams& p, bool& empty, bool dry = false) {
    // (dry: zhip_decode_mapped_multi_check -- nothing is launched, so the plan's tables may be absent)
    empty = false;
    if (!plan) return set_err(ZHIP_E_INVALID, "null plan");
    if (!plan->d_tables && !dry) return set_err(ZHIP_E_INVALID, "plan not uploaded (zhip_plan_upload)");
    if (n_chunks == 0 && n_index == 0) {
        empty = true;
        return ZHIP_OK;
    }
    if (!src || !d_chunks || !d_sels || !d_status || !d_workspace || !d_errflag)
        return set_err(ZHIP_E_INVALID, "null device pointer");
    if (n_index) {
        if (!d_index_chunks || !d_index_status) return set_err(ZHIP_E_INVALID, "null index pointer");
        // inner chunks without a CRC: only the mapped pair decode carries the
        // index checks (k_decode_lead, leading workgroups)
        const bool lead_ok = d_rowmap && (decode_flags & ZHIP_DF_ROWS) && (decode_flags & ZHIP_DF_FAST_ROWS) &&
                             plan->nseg <= 32u && plan->seg == (uint32_t)kWgStride * kDefaultBlocks;
        if (!(plan->layout.flags & ZHIP_LF_SHARDED) || (!(plan->layout.flags & ZHIP_LF_CRC) && !lead_ok) ||
            (decode_flags & ZHIP_DF_TILE) || plan->idx_nbytes == 0)
            return set_err(ZHIP_E_UNSUPPORTED, "index check cannot be fused for this plan");
    }
    const zhip_layout& L = plan->layout;
    if (!(L.flags & ZHIP_LF_NO_WRITE) && !out) return set_err(ZHIP_E_INVALID, "null out");
    const uint64_t units = (uint64_t)n_chunks * plan->nseg;
    if (units >= (1ull << 32)) return set_err(ZHIP_E_UNSUPPORTED, "too many units in one batch");
    p = DecodeParams{};
    p.src = static_cast<const uint8_t*>(src);
    p.src_size = src_size;
    p.out = static_cast<uint8_t*>(out);
    p.chunks = d_chunks;
    p.sels = d_sels;
    p.status = d_status;
    p.ws = d_workspace;
    p.errflag = d_errflag;
    const TableLayout& T = plan->tl;
    p.horner = row_at(plan, T.horner);
    p.kthread = row_at(plan, T.kthread);
    p.kunit = row_at(plan, T.kunit);
    p.kpair = row_at(plan, T.kpair);
    p.pair_tab = row_at(plan, T.pair.tab);
    p.kpair11 = row_at(plan, T.pair.klane);
    p.kthread11 = row_at(plan, T.pair.kidx);
    // k_decode_il needs its tables, and a fused index check of one step per lane
    if (plan->il_S && (n_index == 0 || plan->idx_E <= (uint32_t)kWgStride)) {
        // the widest interleave the plan built (S = 32, else 16, else 8); tuning
        // arms 69 / 70 / 71 force 16 / 32 / 8
        const IlTables il = il_tables(plan, g_tune_arm == kArmIlS16 ? 16u : g_tune_arm == kArmIlS32 ? 32u
                                            : g_tune_arm == kArmIlS8 ? 8u : 0u);
        p.il_S = il.S;
        p.il_tab = il.tab;
        p.il_klane = il.klane;
        p.il_kidx = il.kidx;
        p.il_basis = il.basis;
    }
    p.xw = (plan->xw_P && (n_index == 0 || plan->idx_E <= (uint32_t)kWgStride)) ? plan->xw_P : 0u;
    if (p.xw) {
        p.xw_nsub = plan->xw_nsub;
        p.xw_tab = row_at(plan, T.xw.tab);
        p.xw_klane = row_at(plan, T.xw.klane);
        p.xw_kidx = row_at(plan, T.xw.kidx);
    }
    // k_decode_ilw: 512 lanes per unit for grids of at most kIlwMaxUnits
    // units (launch_decode; tuning arms 26 / 31 force 1024 lanes, 27 / 32 512)
    {
        int wi = (n_index == 0 || plan->idx_E <= (uint32_t)kWgStride) && units <= kIlwMaxUnits ? 1 : -1;
#if ZHIP_TUNING
        if (g_tune_arm == kArmIlw1024 || g_tune_arm == kArmIlw1024Reg) wi = 0;
        else if (g_tune_arm == kArmIlw512 || g_tune_arm == kArmIlw512Reg || g_tune_arm == kArmIlw512Half) wi = 1;
        // (the probes' numbers lie inside the ilw arms' range)
        if ((arm_in(kArmIlw1024, kArmIlw512Reg) || g_tune_arm == kArmIlw512Half) &&
            !(n_index == 0 || plan->idx_E <= (uint32_t)kWgStride)) wi = -1;
#endif
        p.ilw_nt = (wi >= 0 && T.ilw[wi].tab.n) ? (1024u >> wi) : 0u;
        if (p.ilw_nt) {
            p.ilw_tab = row_at(plan, T.ilw[wi].tab);
            p.ilw_klane = row_at(plan, T.ilw[wi].klane);
            p.ilw_kidx = row_at(plan, T.ilw[wi].kidx);
        }
    }
    p.ilh_klane = row_at(plan, T.ilh);
    // whole-chunk selections (ZHIP_DF_WHOLE, with a row map) of a plan whose
    // whole-chunk row map is affine: the row kernels compute destinations
    // (tuning arm 45 keeps the map loads: the A/B reference)
    p.aff_ok = (decode_flags & ZHIP_DF_WHOLE) && (decode_flags & ZHIP_DF_ROWS) && d_rowmap && plan->aff_ok &&
               !(ZHIP_TUNING && g_tune_arm == kArmRowMap);
    if (p.aff_ok) set_affine(p, plan);
    for (int op = 0; op < 4; ++op) p.hx[op] = plan->hx[op];
    for (int i = 0; i < 32; ++i) p.kq[i] = plan->kq[i];
    p.n_chunks = n_chunks;
    p.nseg = plan->nseg;
    p.n_units = (uint32_t)units;
    p.n_idx = n_index;
    p.idx_chunks = d_index_chunks;
    p.idx_status = d_index_status;
    p.idx_nbytes = plan->idx_nbytes;
    p.idx_E = plan->idx_E;
    p.idx_c_inv = plan->idx_c_inv;
    p.idx_c3 = plan->idx_c3;
    p.c_inv = plan->c_inv;
    p.c3 = plan->c3;
    p.lflags = L.flags;
    fill_geom(p.g, *plan);
    p.seg = plan->seg;
    p.E = plan->E;
    p.index_size = L.index_size;
    p.n_inner = L.n_inner;
    std::memcpy(p.fill, plan->fill, sizeof(p.fill));
    p.fast = (decode_flags & ZHIP_DF_FAST_ROWS) ? 1u : 0u;
    p.dv_bank = (decode_flags & ZHIP_DF_BANK1) ? 1u : 0u;
    p.defer = (decode_flags & ZHIP_DF_DEFER) ? 1u : 0u;
    p.tune = g_tune_bits;
    p.tq = -1;
    p.rows = 0;
    p.rowmap = nullptr;
    p.pred = 0;
    if (decode_flags & ZHIP_DF_ROWS) {
        const uint32_t rb = plan->row_bytes;
        const int nd = L.ndim;
        const bool pow2 = rb >= 16 && rb <= (uint32_t)kWgStride && (rb & (rb - 1)) == 0;
        if (!(decode_flags & ZHIP_DF_FAST_ROWS) || (decode_flags & ZHIP_DF_TILE) || nd < 2 || !pow2 ||
            (L.flags & ZHIP_LF_NO_WRITE) || (uint32_t)L.shape[nd - 2] % ((uint32_t)kWgStride / rb) != 0)
            return set_err(ZHIP_E_INVALID, "ZHIP_DF_ROWS preconditions do not hold for this layout");
        p.rows = 1;
        p.rowmap = d_rowmap;
        if (pred) {
            if (pred->per == 0) return set_err(ZHIP_E_INVALID, "zhip_predict.per must be >= 1");
            // every predicted unit range must lie inside src (the kernel reads it before checking)
            const uint64_t last = n_chunks ? (uint64_t)(n_chunks - 1) : 0;
            const uint64_t gl = last / pred->per;
            uint64_t top = gl * pred->outer + (last % pred->per) * pred->inner;
            if (gl >= 1) {
                const uint64_t full = (gl - 1) * pred->outer + (uint64_t)(pred->per - 1) * pred->inner;
                if (full > top) top = full;
            }
            const uint64_t hi = pred->base + top + plan->E;
            if (n_chunks && hi > src_size) return set_err(ZHIP_E_INVALID, "zhip_predict range outside src");
            p.pred = 1;
            p.pred_base = pred->base;
            p.pred_outer = pred->outer;
            p.pred_inner = pred->inner;
            p.pred_per = pred->per;
        }
        p.row_shift = (uint32_t)__builtin_ctz(rb);
        p.r_sy = (uint32_t)L.shape[nd - 2];
        p.r_dy = make_fdiv(p.r_sy);
        p.r_oy = L.out_stride[nd - 2];
        p.nd2 = nd - 2;
    }
    if ((decode_flags & ZHIP_DF_TILE) && plan->tq >= 0 && plan->d_tile_tables) {
        p.tq = plan->tq;
        p.t_per_chunk = plan->t_per_chunk;
        p.n_qb = plan->n_qb;
        p.n_cb = plan->n_cb;
        for (int d = 0; d < ZHIP_MAX_DIMS; ++d) p.sstride[d] = plan->sstride[d];
        p.d_qb = make_fdiv(plan->n_qb);
        p.d_cb = make_fdiv(plan->n_cb);
        p.horner = tile_at(plan, T.t_horner);
        p.kthread = tile_at(plan, T.t_kthread);
        p.kunit = tile_at(plan, T.t_kunit);
        p.c_inv = plan->t_c_inv;
        p.tile4 = plan->tile4 && !(g_tune_bits & (kTuneTile1 | kTuneNoTile4));
        if (p.tile4) {
            p.tz = tile_at(plan, T.tile4_tz);
            p.kq4 = tile_at(plan, T.tile4_kq);
            p.tmap = tile_at<TileEnt>(plan, T.tile4_map);
            if (plan->tile4f && (g_tune_bits & kTuneTile4F)) {  // arm: measured 0.3-0.4 us slower on C3
                p.t4f_tab = tile_at(plan, T.t4f.tab);
                p.t4f_kq = tile_at(plan, T.t4f.klane);
            } else if (plan->tile4w && g_tune_arm != kArmPub16 && g_tune_arm != kArmDeferred &&
                       g_tune_arm != kArmNoWaveTile) {
                // production for CRC layouts: a wave per tile, one chain per lane (k_decode_tile4w:
                // C3 28.9 vs 30.3-30.6 us, profiles/r04/k); arms 1 / 2 / 5: k_decode_tile4
                p.t4w_tab = tile_at(plan, T.t4w.tab);
                p.t4w_kq = tile_at(plan, T.t4w.klane);
                p.tbt_tab = tile_at(plan, T.tbt_ad);
                p.t2w_kq = tile_at(plan, T.t2w);
                p.t1w_kq = tile_at(plan, T.t1w);
            }
        } else if (plan->tile2 && T.tile2_tab.n && !(g_tune_bits & kTuneTile1) && g_tune_arm == kArmTilePairs) {
            // consecutive tile pairs (k_decode_tile4w<2>) where tile4 declines
            // (tuning arm 39; the grouped kernels are faster)
            p.tile2 = 1;
            p.t4w_tab = tile_at(plan, T.tile2_tab);
            p.tmap = tile_at<TileEnt>(plan, T.tile2_map);
            p.t4w_kq = tile_at(plan, T.tile2_klane);
        } else if (plan->gd >= 0 && !(g_tune_bits & kTuneTile1) &&
                   L.shape[plan->tq] % (16 / L.itemsize) == 0) {
            // k_decode_tileg: tiles grouped by four along gd, whole out pieces
            p.tileg = 1;
            p.gtz = tile_at(plan, T.g_tz);
            p.gmap = tile_at<GroupEnt>(plan, T.g_map);
            p.n_groups = plan->n_groups;
            p.n_sub = plan->n_sub;
            p.g_step_t = plan->sstride[plan->gd];
            p.g_step_o = L.out_stride[plan->gd];
            // a wave per tile, one chain per lane
            if (plan->tilegw && g_tune_arm != kArmDeferred && g_tune_arm != kArmNoWaveTile) {
                p.t4w_tab = tile_at(plan, T.tgw.tab);
                p.t4w_kq = tile_at(plan, T.tgw.klane);
                p.t2w_kq = tile_at(plan, T.tg2w);  // two tiles per workgroup
                p.tglt_kq = tile_at(plan, T.tgl);  // (arm 40)
                p.tbt_tab = tile_at(plan, T.tbt_ad);  // (arm 66)
            }
        }
        const uint64_t tunits = (uint64_t)n_chunks * plan->t_per_chunk;
        if (tunits >= (1ull << 32)) return set_err(ZHIP_E_UNSUPPORTED, "too many tiles in one batch");
        p.n_units = (uint32_t)tunits;
        p.fast = 0;
    }
    if (p.rows && units >= (1ull << 31)) return set_err(ZHIP_E_UNSUPPORTED, "too many units for a row decode");
    fill_pair_hot(p);
    return ZHIP_OK;
}
}

int zhip_decode_mapped(const zhip_plan* plan, const void* src, uint64_t src_size, void* out,
                       const zhip_chunk* d_chunks, uint32_t n_chunks, const zhip_sel* d_sels,
                       zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_errflag,
                       const zhip_chunk* d_index_chunks, uint32_t n_index, zhip_status* d_index_status,
                       uint32_t decode_flags, const zhip_predict* pred, const zhip_rowblk* d_rowmap,
                       void* stream) {
    DecodeParams p;
    bool empty;
    int rc = mapped_params(plan, src, src_size, out, d_chunks, n_chunks, d_sels, d_status, d_workspace, d_errflag,
                           d_index_chunks, n_index, d_index_status, decode_flags, pred, d_rowmap, p, empty);
    if (rc != ZHIP_OK || empty) return rc;
    rc = launch_decode(p, static_cast<hipStream_t>(stream), plan->max_grid);
    if (rc == ZHIP_E_UNSUPPORTED) return set_err(rc, "no kernel for this layout");
    if (rc != ZHIP_OK) return set_err(rc, std::string("launch failed: ") + hipGetErrorString(hipGetLastError()));
    return ZHIP_OK;
}

uint32_t zhip_multi_max(void) { return (uint32_t)ZHIP_MULTI_MAX; }

extern "C++" {
static int mapped_multi(const zhip_mapped_args* args, uint32_t n, void* stream, bool dry) {
    if (n < 2u || n > (uint32_t)ZHIP_MULTI_MAX)
        return set_err(ZHIP_E_UNSUPPORTED, "zhip_decode_mapped_multi takes 2 .. zhip_multi_max() entries");
    if (!args) return set_err(ZHIP_E_INVALID, "null args");
    DecodeParams ps[ZHIP_MULTI_MAX];
    int max_grid[ZHIP_MULTI_MAX];
    for (uint32_t i = 0; i < n; ++i)  // arrival words and statuses are per launch
        for (uint32_t j = 0; j < i; ++j)
            if (args[i].d_workspace == args[j].d_workspace || args[i].d_status == args[j].d_status)
                return set_err(ZHIP_E_UNSUPPORTED, "fused decodes must not share a workspace or status table");
    for (uint32_t i = 0; i < n; ++i) {
        const zhip_mapped_args& a = args[i];
        bool empty;
        const int rc = mapped_params(a.plan, a.src, a.src_size, a.out, a.d_chunks, a.n_chunks, a.d_sels, a.d_status,
                                     a.d_workspace, a.d_errflag, a.d_index_chunks, a.n_index, a.d_index_status,
                                     a.decode_flags, a.pred, a.d_rowmap, ps[i], empty, dry);
        if (rc != ZHIP_OK) return rc;
        if (empty) return set_err(ZHIP_E_UNSUPPORTED, "an empty decode cannot be fused");
        max_grid[i] = a.plan->max_grid;
    }
    const int rc = launch_decode_multi(ps, max_grid, n, static_cast<hipStream_t>(stream), dry);
    if (rc == ZHIP_E_UNSUPPORTED)
        return set_err(rc, "not fusable: every entry must take the same production k_decode_il");
    if (rc != ZHIP_OK) return set_err(rc, std::string("launch failed: ") + hipGetErrorString(hipGetLastError()));
    return ZHIP_OK;
}
}

int zhip_decode_mapped_multi(const zhip_mapped_args* args, uint32_t n, void* stream) {
    return mapped_multi(args, n, stream, false);
}

int zhip_decode_mapped_multi_check(const zhip_mapped_args* args, uint32_t n) {
    return mapped_multi(args, n, nullptr, true);
}

int zhip_encode(const zhip_plan* plan, const void* arr, void* dst, const zhip_chunk* d_chunks, uint32_t n_chunks,
                const zhip_sel* d_sels, zhip_status* d_status, uint32_t* d_workspace, uint32_t* d_nonempty,
                uint32_t encode_flags, void* stream) {
    return zhip_encode_mapped(plan, arr, dst, d_chunks, n_chunks, d_sels, d_status, d_workspace, d_nonempty,
                              encode_flags, nullptr, stream);
}

int zhip_encode_mapped(const zhip_plan* plan, const void* arr, void* dst, const zhip_chunk* d_chunks,
                       uint32_t n_chunks, const zhip_sel* d_sels, zhip_status* d_status, uint32_t* d_workspace,
                       uint32_t* d_nonempty, uint32_t encode_flags, const zhip_rowblk* d_rowmap, void* stream) {
    if (!plan) return set_err(ZHIP_E_INVALID, "null plan");
    if (!plan->d_tables) return set_err(ZHIP_E_INVALID, "plan not uploaded (zhip_plan_upload)");
    if (n_chunks == 0) return ZHIP_OK;
    if (!arr || !dst || !d_chunks || !d_sels || !d_status || !d_workspace || !d_nonempty)
        return set_err(ZHIP_E_INVALID, "null device pointer");
    if (plan->kblocks != (uint32_t)kDefaultBlocks) return set_err(ZHIP_E_UNSUPPORTED, "encode needs K=8 plans");
    const zhip_layout& L = plan->layout;
    const uint64_t units = (uint64_t)n_chunks * plan->nseg;
    if (units >= (1ull << 32)) return set_err(ZHIP_E_UNSUPPORTED, "too many units in one batch");
    EncodeParams p{};
    // chunks' publication words a 128-byte line apart (zhip_plan_info's >= kPubLine
    // workspace words for CRC layouts); arm ZHIP_TUNE_ARM = 9: 16 bytes apart
    p.pub_stride = ((plan->layout.flags & ZHIP_LF_CRC) && g_tune_arm != kArmEncPub16) ? kPubLine / 2u : 2u;
    p.arr = static_cast<const uint8_t*>(arr);
    p.dst = static_cast<uint8_t*>(dst);
    p.chunks = d_chunks;
    p.sels = d_sels;
    p.status = d_status;
    p.ws = d_workspace;
    p.nonempty = d_nonempty;
    const TableLayout& T = plan->tl;
    p.horner = row_at(plan, T.horner);
    p.kthread = row_at(plan, T.kthread);
    p.kunit = row_at(plan, T.kunit);
    p.n_chunks = n_chunks;
    p.nseg = plan->nseg;
    p.n_units = (uint32_t)units;
    p.c_inv = plan->c_inv;
    p.c3 = plan->c3;
    p.lflags = L.flags;
    fill_geom(p.g, *plan);
    p.seg = plan->seg;
    p.E = plan->E;
    std::memcpy(p.fill, plan->fill, sizeof(p.fill));
    p.fill_nan = fill_is_nan(L.itemsize, (L.flags & ZHIP_LF_FLOAT) != 0, (L.flags & ZHIP_LF_COMPLEX) != 0, p.fill[0],
                             p.fill[1]) ? 1u : 0u;
    p.fast = (encode_flags & ZHIP_DF_FAST_ROWS) ? 1u : 0u;
    p.tune = g_tune_bits;
    p.rowmap = nullptr;
    p.tile4 = 0;
    if ((encode_flags & ZHIP_DF_TILE) && plan->tile4 && plan->t_per_chunk <= 64 && plan->d_tile_tables &&
        !(g_tune_bits & (kTuneTile1 | kTuneNoTile4))) {
        // transposed chunks, full tiles, at most 16 workgroups per chunk (the
        // arrival / non-empty bits of one 64-bit word): k_encode_tile4
        p.tile4 = 1;
        p.tq = plan->tq;
        p.t_per_chunk = plan->t_per_chunk;
        for (int d = 0; d < ZHIP_MAX_DIMS; ++d) p.sstride[d] = plan->sstride[d];
        p.horner = tile_at(plan, T.t_horner);
        p.tz = tile_at(plan, T.tile4_tz);
        p.kq4 = tile_at(plan, T.tile4_kq);
        p.kq2 = tile_at(plan, T.t2e);
        p.tmap = tile_at<TileEnt>(plan, T.tile4_map);
        d_rowmap = nullptr;
    } else if ((encode_flags & ZHIP_DF_TILE) && plan->gd >= 0 && plan->d_tile_tables && !(g_tune_bits & kTuneTile1) &&
               L.shape[plan->tq] % (16 / L.itemsize) == 0 && plan->n_groups < 65536u) {
        // (whole 16-byte pieces along tq: a piece never reaches past the chunk)
        // full selections, tiles grouped by four at a uniform step: k_encode_tileg
        p.tile = 2;
        p.tq = plan->tq;
        p.t_per_chunk = plan->t_per_chunk;
        for (int d = 0; d < ZHIP_MAX_DIMS; ++d) p.sstride[d] = plan->sstride[d];
        p.horner = tile_at(plan, T.t_horner);
        p.kthread = tile_at(plan, T.t_kthread);
        p.gtz = tile_at(plan, T.g_tz);
        p.gmap = tile_at<GroupEnt>(plan, T.g_map);
        p.n_groups = plan->n_groups;
        p.n_sub = plan->n_sub;
        p.g_step_t = plan->sstride[plan->gd];
        p.g_z2 = xpow8(2ull * plan->sstride[plan->gd]);
        p.g_step_o = L.out_stride[plan->gd];
        p.g_a4 = tile_at(plan, T.tbt_a4);  // (arm 68)
        p.g_c96 = xpow8_inv(12);
        d_rowmap = nullptr;
    } else if ((encode_flags & (ZHIP_DF_TILE | ZHIP_DF_TILE_PREFIX)) && plan->tq >= 0 && plan->d_tile_tables &&
               (plan->t_per_chunk + 3u) / 4u < 65536u) {
        // every other transposed batch (partial tiles, many tiles per chunk,
        // edge chunks with prefix selections): k_encode_tile
        p.tile = 1;
        p.tq = plan->tq;
        p.t_per_chunk = plan->t_per_chunk;
        p.n_qb = plan->n_qb;
        p.n_cb = plan->n_cb;
        p.d_qb = make_fdiv(plan->n_qb);
        p.d_cb = make_fdiv(plan->n_cb);
        for (int d = 0; d < ZHIP_MAX_DIMS; ++d) p.sstride[d] = plan->sstride[d];
        p.horner = tile_at(plan, T.t_horner);
        p.kthread = tile_at(plan, T.t_kthread);
        p.kunit = tile_at(plan, T.t_kunit);
        p.c_inv = plan->t_c_inv;
        d_rowmap = nullptr;
    }
    if (d_rowmap) {
        const uint32_t rb = plan->row_bytes;
        const int nd = L.ndim;
        if (!p.fast || nd < 2 || rb < 16 || rb > (uint32_t)kWgStride || (rb & (rb - 1)) != 0 ||
            (uint32_t)L.shape[nd - 2] % ((uint32_t)kWgStride / rb) != 0)
            return set_err(ZHIP_E_INVALID, "row map given for a layout without whole-row encode");
        p.rowmap = d_rowmap;
        p.kpair = row_at(plan, T.kpair);
        p.pair_tab = row_at(plan, T.pair.tab);
        p.kpair11 = row_at(plan, T.pair.klane);
        p.row_shift = (uint32_t)__builtin_ctz(rb);
        p.r_oy = L.out_stride[nd - 2];
        if (plan->il_S == 8u && (L.flags & ZHIP_LF_CRC)) {  // k_encode_il (launch_encode)
            // the decode's widest interleave (S = 32 / 16 where the steps tile
            // it; tuning arm 73 keeps S = 8)
            const IlTables il = il_tables(plan, g_tune_arm == kArmEncIlS8 ? 8u : 0u);
            p.il_S = il.S;
            p.il_tab = il.tab;
            p.il_klane = il.klane;
            // whole-chunk selections: destinations computed (ZHIP_DF_WHOLE, as the
            // decode) only in tuning arm 46 -- graph-timed 29.1 vs 28.6 us on the
            // C2 encode (profiles/r05/x/): the encode keeps the row map
            p.aff_ok = (encode_flags & ZHIP_DF_WHOLE) && plan->aff_ok && ZHIP_TUNING && g_tune_arm == kArmEncAff;
            if (p.aff_ok) set_affine(p, plan);
        }
    }
    int rc = launch_encode(p, static_cast<hipStream_t>(stream), plan->max_grid);
    if (rc == ZHIP_E_UNSUPPORTED) return set_err(rc, "no encode kernel for this layout");
    if (rc != ZHIP_OK) return set_err(rc, std::string("launch failed: ") + hipGetErrorString(hipGetLastError()));
    return ZHIP_OK;
}

int zhip_shard_pack(const zhip_plan* plan, void* dst, const zhip_shard* d_shards, uint32_t n_shards,
                    uint32_t n_inner, uint32_t elen, uint32_t index_size, uint32_t pack_flags,
                    const uint32_t* d_nonempty, uint32_t* d_newrank, const uint32_t* d_rank_of_slot,
                    uint64_t* d_blob_len, void* stream) {
    if (!plan || !plan->d_tables) return set_err(ZHIP_E_INVALID, "plan not uploaded");
    if (n_shards == 0) return ZHIP_OK;
    if (!dst || !d_shards || !d_nonempty || !d_newrank || !d_rank_of_slot || !d_blob_len)
        return set_err(ZHIP_E_INVALID, "null device pointer");
    if (n_inner == 0) return set_err(ZHIP_E_INVALID, "n_inner == 0");
    PackParams p{};
    p.dst = static_cast<uint8_t*>(dst);
    p.shards = d_shards;
    p.nonempty = d_nonempty;
    p.newrank = d_newrank;
    p.rank_of_slot = d_rank_of_slot;
    p.blob_len = d_blob_len;
    p.horner = row_at(plan, plan->tl.horner);
    p.kthread = row_at(plan, plan->tl.kthread);
    p.n_inner = n_inner;
    p.elen = elen;
    p.index_size = index_size;
    p.index_start = (pack_flags & ZHIP_PF_INDEX_START) ? 1u : 0u;
    p.index_crc = (pack_flags & ZHIP_PF_INDEX_CRC) ? 1u : 0u;
    p.keep_empty = (pack_flags & ZHIP_PF_KEEP_EMPTY) ? 1u : 0u;
    // index CRC constants: thread t's Horner state lands at 16t + 4096*kiters,
    // shifted by kthread[t] to R = 4096*(kiters+1); payload = 16*n_inner bytes
    const uint64_t nidx = 16ull * n_inner;
    const uint64_t kiters = (n_inner + kThreads - 1) / kThreads;
    const uint64_t R = (uint64_t)kWgStride * (kiters + 1);
    p.idx_c_inv = xpow8_inv(R - nidx);
    p.idx_c3 = gf_mul(xpow8(nidx), 0xFFFFFFFFu);
    int rc = launch_shard_pack(p, n_shards, static_cast<hipStream_t>(stream));
    if (rc != ZHIP_OK) return set_err(rc, std::string("launch failed: ") + hipGetErrorString(hipGetLastError()));
    return ZHIP_OK;
}

uint32_t zhip_fdiv_eval(uint32_t n, uint32_t d) {
    const zhip_fdiv f = make_fdiv(d);
    return fdiv_apply(n, f.m, f.s);
}

// ---- zhip_select_copy: gather / scatter of non-basic selections (select.hip) ----
static int select_args(uint32_t n_items, const void* items, const void* prefix, const void* a, const void* b,
                       uint32_t itemsize) {
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8)
        return set_err(ZHIP_E_UNSUPPORTED, "itemsize must be 1, 2, 4 or 8");
    if (!n_items || !items || !prefix || !a || !b) return set_err(ZHIP_E_INVALID, "null argument");
    if (((uintptr_t)a | (uintptr_t)b) & (itemsize - 1)) return set_err(ZHIP_E_INVALID, "a / b not aligned to itemsize");
    return ZHIP_OK;
}

int zhip_select_copy(const zhip_select_item* d_items, uint32_t n_items, const int64_t* d_table,
                     const uint32_t* d_tile_prefix, uint32_t n_tiles, const void* a, uint64_t a_size, void* b,
                     uint64_t b_size, uint32_t itemsize, void* stream) {
    if (n_tiles == 0) return ZHIP_OK;
    const int rc = select_args(n_items, d_items, d_tile_prefix, a, b, itemsize);
    if (rc != ZHIP_OK) return rc;
    if (n_tiles > 0x7fffffffu) return set_err(ZHIP_E_UNSUPPORTED, "too many tiles for one launch");
    const int e = select_launch(d_items, n_items, d_table, d_tile_prefix, n_tiles, a, a_size, b, b_size, itemsize, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_select_copy launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

// The kernel's walk on the host: every tile, its item by the same prefix
// search, its kSelThreads x kSelPer element slots in the kernel's order, the
// same offsets.  Checks the tables a caller could get wrong first.
int zhip_emulate_select_copy(const zhip_select_item* items, uint32_t n_items, const int64_t* table,
                             uint64_t table_pairs, const uint32_t* tile_prefix, uint32_t n_tiles, const void* a,
                             uint64_t a_size, void* b, uint64_t b_size, uint32_t itemsize) {
    if (n_tiles == 0) return ZHIP_OK;
    const int rc = select_args(n_items, items, tile_prefix, a, b, itemsize);
    if (rc != ZHIP_OK) return rc;
    if (tile_prefix[0] != 0 || tile_prefix[n_items] != n_tiles) return set_err(ZHIP_E_INVALID, "tile prefix ends");
    for (uint32_t i = 0; i < n_items; ++i) {
        const zhip_select_item& it = items[i];
        if (it.ndim < 1 || it.ndim > ZHIP_MAX_DIMS) return set_err(ZHIP_E_INVALID, "item ndim");
        uint64_t total = 1;
        for (uint32_t d = 0; d < it.ndim; ++d) {
            const zhip_select_dim& D = it.dims[d];
            if (D.count < 1 || D.count >= (1u << 31)) return set_err(ZHIP_E_INVALID, "dimension count");
            const zhip_fdiv f = make_fdiv(D.count);
            if (f.m != D.div.m || f.s != D.div.s) return set_err(ZHIP_E_INVALID, "dimension divisor");
            if (D.table && (!table || D.table_off + D.count > table_pairs))
                return set_err(ZHIP_E_INVALID, "dimension table range");
            total *= D.count;
            if (total >= (1ull << 31)) return set_err(ZHIP_E_INVALID, "item total");
        }
        if (total != it.total) return set_err(ZHIP_E_INVALID, "item total != prod(count)");
        if (tile_prefix[i + 1] - tile_prefix[i] != (it.total + ZHIP_SELECT_TILE - 1) / ZHIP_SELECT_TILE)
            return set_err(ZHIP_E_INVALID, "tile prefix step");
    }
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
        const uint32_t ii = select_find_item(tile_prefix, n_items, tile);
        const zhip_select_item& it = items[ii];
        for (uint32_t t = 0; t < kSelThreads; ++t)
            for (uint32_t j = 0; j < kSelPer; ++j) {
                const uint32_t e = (tile - tile_prefix[ii]) * ZHIP_SELECT_TILE + t + j * kSelThreads;
                if (e >= it.total) continue;
                int64_t ao, bo;
                select_addr(it, table, e, ao, bo);
                if (!select_inside(ao, bo, a_size, b_size, itemsize))
                    return set_err(ZHIP_E_BOUNDS, "element offset outside its buffer");
                memcpy((uint8_t*)b + bo, (const uint8_t*)a + ao, itemsize);
            }
    }
    return ZHIP_OK;
}

// ---- zhip_value_map: scale_offset / cast_value (values.hip, value_map.cpp) ----
static int value_args(const zhip_value_op* op, uint32_t n_items, const void* items, const void* prefix,
                      const void* a, const void* b, const void* err) {
    const char* msg = "";
    const int rc = value_check_op(op, &msg);
    if (rc != ZHIP_OK) return set_err(rc, msg);
    if (!n_items || !items || !prefix || !a || !b || !err) return set_err(ZHIP_E_INVALID, "null argument");
    if (((uintptr_t)a & (vt_size(value_a_dt(*op)) - 1)) || ((uintptr_t)b & (vt_size(value_b_dt(*op)) - 1)))
        return set_err(ZHIP_E_INVALID, "a / b not aligned to their item sizes");
    return ZHIP_OK;
}

int zhip_value_map(const zhip_value_op* op, const zhip_value_item* d_items, uint32_t n_items,
                   const uint32_t* d_tile_prefix, uint32_t n_tiles, const zhip_status* d_status, const void* a,
                   uint64_t a_size, void* b, uint64_t b_size, uint32_t* d_err, uint32_t* d_nonempty,
                   void* stream) {
    if (n_tiles == 0) return ZHIP_OK;
    const int rc = value_args(op, n_items, d_items, d_tile_prefix, a, b, d_err);
    if (rc != ZHIP_OK) return rc;
    if (n_tiles > 0x7fffffffu) return set_err(ZHIP_E_UNSUPPORTED, "too many tiles for one launch");
    const int e = value_launch(*op, d_items, n_items, d_tile_prefix, n_tiles, d_status, a, a_size, b, b_size,
                               d_err, d_nonempty, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_value_map launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

int zhip_emulate_fill_eq(uint32_t itemsize, uint32_t lflags, const void* fill, const void* items, uint64_t n_items,
                         uint8_t* eq, uint32_t* fill_nan) {
    if (!fill || (n_items && (!items || !eq))) return set_err(ZHIP_E_INVALID, "null argument");
    if (!(itemsize == 1 || itemsize == 2 || itemsize == 4 || itemsize == 8))
        return set_err(ZHIP_E_UNSUPPORTED, "itemsize must be 1, 2, 4 or 8");
    const bool cplx = (lflags & ZHIP_LF_COMPLEX) != 0, flt = (lflags & ZHIP_LF_FLOAT) != 0;
    if (cplx && (flt || itemsize != 8))
        return set_err(ZHIP_E_INVALID, "ZHIP_LF_COMPLEX is an 8-byte item of two float32, without ZHIP_LF_FLOAT");
    // the fill replicated to 16 bytes, as zhip_plan_create keeps it
    uint8_t f16[16];
    for (int i = 0; i < 16; ++i) f16[i] = static_cast<const uint8_t*>(fill)[i % itemsize];
    uint32_t f[4];
    std::memcpy(f, f16, 16);
    const uint32_t fnan = fill_is_nan((int)itemsize, flt, cplx, f[0], f[1]) ? 1u : 0u;
    if (fill_nan) *fill_nan = fnan;
    const uint8_t* src = static_cast<const uint8_t*>(items);
    for (uint64_t i = 0; i < n_items; ++i) {
        // item i as the first (and only valid) item of a 16-byte block, as the kernels' tail blocks have it
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        std::memcpy(v, src + i * itemsize, itemsize);
        bool e;
        switch (itemsize) {
            case 1: e = block_eq_fill_bits<1>(v[0], v[1], v[2], v[3], 1u, f, fnan); break;
            case 2: e = block_eq_fill_bits<2>(v[0], v[1], v[2], v[3], 2u, f, fnan); break;
            case 4: e = block_eq_fill_bits<4>(v[0], v[1], v[2], v[3], 4u, f, fnan); break;
            default:
                e = cplx ? block_eq_fill_bits<8, true>(v[0], v[1], v[2], v[3], 8u, f, fnan)
                         : block_eq_fill_bits<8>(v[0], v[1], v[2], v[3], 8u, f, fnan);
        }
        eq[i] = e ? 1u : 0u;
    }
    return ZHIP_OK;
}

int zhip_emulate_value_map(const zhip_value_op* op, const zhip_value_item* items, uint32_t n_items,
                           const uint32_t* tile_prefix, uint32_t n_tiles, const zhip_status* status,
                           uint32_t n_status, const void* a, uint64_t a_size, void* b, uint64_t b_size,
                           uint32_t* err, uint32_t* nonempty) {
    if (n_tiles == 0) return ZHIP_OK;
    int rc = value_args(op, n_items, items, tile_prefix, a, b, err);
    if (rc != ZHIP_OK) return rc;
    const char* msg = "";
    rc = value_emulate(*op, items, n_items, tile_prefix, n_tiles, status, n_status, a, a_size, b, b_size, err,
                       nonempty, &msg);
    return rc == ZHIP_OK ? rc : set_err(rc, msg);
}

// ---- zhip_points_count / zhip_points_fill: device-built point tables (points.hip) ----
// The geometry a caller could get wrong, the limits, and the grid size.
static int points_args(const zhip_points_geom* g, const void* const* coords, uint64_t n, uint64_t* n_chunks) {
    if (!g || !coords) return set_err(ZHIP_E_INVALID, "null argument");
    if (g->ndim < 1 || g->ndim > ZHIP_MAX_DIMS) return set_err(ZHIP_E_INVALID, "points geometry ndim");
    if (g->write > 1) return set_err(ZHIP_E_INVALID, "points geometry write flag");
    if (n > ZHIP_POINTS_MAX_N) return set_err(ZHIP_E_UNSUPPORTED, "2^31 or more points in one selection");
    for (int d = 0; d < g->ndim; ++d) {
        if (g->shape[d] > ZHIP_POINTS_MAX_DIM) return set_err(ZHIP_E_UNSUPPORTED, "an array dimension of 2^31 or more");
        if (g->chunk[d] < 1 || g->chunk[d] > ZHIP_POINTS_MAX_DIM) return set_err(ZHIP_E_INVALID, "points geometry chunk length");
        const zhip_fdiv f = make_fdiv(g->chunk[d]);
        if (f.m != g->div[d].m || f.s != g->div[d].s) return set_err(ZHIP_E_INVALID, "points geometry divisor");
        if (g->grid[d] != (uint32_t)(((uint64_t)g->shape[d] + g->chunk[d] - 1) / g->chunk[d]))
            return set_err(ZHIP_E_INVALID, "points geometry grid length");
        if (n && (!coords[d] || ((uintptr_t)coords[d] & 7))) return set_err(ZHIP_E_INVALID, "coordinate array null or unaligned");
    }
    *n_chunks = points_grid_size(*g);
    if (!*n_chunks) return set_err(ZHIP_E_UNSUPPORTED, "chunk grid larger than ZHIP_POINTS_MAX_GRID");
    return ZHIP_OK;
}

static PointsCoords points_coords(const zhip_points_geom* g, const int64_t* const* coords) {
    PointsCoords pc;
    for (int d = 0; d < ZHIP_MAX_DIMS; ++d) pc.c[d] = d < g->ndim ? coords[d] : nullptr;
    return pc;
}

int zhip_points_count(const zhip_points_geom* geom, const int64_t* const* d_coords, uint64_t n, uint32_t* d_counts,
                      uint32_t* d_err, void* stream) {
    uint64_t n_chunks = 0;
    const int rc = points_args(geom, (const void* const*)d_coords, n, &n_chunks);
    if (rc != ZHIP_OK) return rc;
    if (!d_counts || !d_err) return set_err(ZHIP_E_INVALID, "null argument");
    if (n == 0) return ZHIP_OK;
    const int e = points_count_launch(*geom, points_coords(geom, d_coords), (uint32_t)n, (uint32_t)n_chunks, d_counts,
                                      d_err, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_points_count launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

int zhip_points_fill(const zhip_points_geom* geom, const int64_t* const* d_coords, uint64_t n, const uint32_t* d_first,
                     uint32_t* d_cursor, int64_t* d_table, void* stream) {
    uint64_t n_chunks = 0;
    const int rc = points_args(geom, (const void* const*)d_coords, n, &n_chunks);
    if (rc != ZHIP_OK) return rc;
    if (!d_first || !d_cursor || !d_table) return set_err(ZHIP_E_INVALID, "null argument");
    if ((uintptr_t)d_table & 15) return set_err(ZHIP_E_INVALID, "pair table not 16-byte aligned");
    if (n == 0) return ZHIP_OK;
    const int e = points_fill_launch(*geom, points_coords(geom, d_coords), (uint32_t)n, (uint32_t)n_chunks, d_first,
                                     d_cursor, d_table, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_points_fill launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

// Both steps on the host, in point order, with the kernels' points_locate /
// points_pair: count, then (no index out of range) the prefix sum and the fill.
int zhip_emulate_points(const zhip_points_geom* geom, const int64_t* const* coords, uint64_t n, uint32_t* counts,
                        uint32_t* err, uint32_t* first, uint32_t* cursor, int64_t* table) {
    uint64_t n_chunks = 0;
    const int rc = points_args(geom, (const void* const*)coords, n, &n_chunks);
    if (rc != ZHIP_OK) return rc;
    if (!counts || !err || !first || !cursor || (n && !table)) return set_err(ZHIP_E_INVALID, "null argument");
    const zhip_points_geom& g = *geom;
    memset(counts, 0, n_chunks * sizeof(uint32_t));
    memset(cursor, 0, n_chunks * sizeof(uint32_t));
    *err = 0;
    int64_t x[ZHIP_MAX_DIMS] = {0};
    uint32_t rix;
    int64_t off;
    for (uint64_t k = 0; k < n; ++k) {
        for (int d = 0; d < g.ndim; ++d) x[d] = coords[d][k];
        const uint32_t e = points_locate(g, x, rix, off);
        if (e) *err |= e; else counts[rix] += 1;
    }
    if (*err) return ZHIP_OK;
    uint32_t at = 0;
    for (uint64_t b = 0; b < n_chunks; ++b) {
        first[b] = at;
        at += counts[b];
    }
    for (uint64_t k = 0; k < n; ++k) {
        for (int d = 0; d < g.ndim; ++d) x[d] = coords[d][k];
        if (points_locate(g, x, rix, off)) continue;
        const uint64_t p = (uint64_t)first[rix] + cursor[rix]++;
        if (p >= n) return set_err(ZHIP_E_BOUNDS, "pair index outside the table");
        points_pair(g, k, off, table[2 * p], table[2 * p + 1]);
    }
    return ZHIP_OK;
}

// ---- zhip_axis_last / zhip_axis_count / zhip_axis_fill: device-planned orthogonal axes (axis.hip) ----
// The geometry a caller could get wrong, and the limits.
static int axis_args(const zhip_axis_geom* g, const void* x, uint64_t n, bool keep_last) {
    if (!g) return set_err(ZHIP_E_INVALID, "null argument");
    if (g->write > 1) return set_err(ZHIP_E_INVALID, "axis geometry write flag");
    if (n > ZHIP_AXIS_MAX_N) return set_err(ZHIP_E_UNSUPPORTED, "2^31 or more indices along one axis");
    if (g->length > ZHIP_AXIS_MAX_LEN) return set_err(ZHIP_E_UNSUPPORTED, "an axis of length 2^31 or more");
    if (g->length < 1) return set_err(ZHIP_E_INVALID, "axis geometry length");
    if (g->chunk < 1 || g->chunk > ZHIP_AXIS_MAX_LEN) return set_err(ZHIP_E_INVALID, "axis geometry chunk length");
    const zhip_fdiv f = make_fdiv(g->chunk);
    if (f.m != g->div.m || f.s != g->div.s) return set_err(ZHIP_E_INVALID, "axis geometry divisor");
    if (g->grid != (uint32_t)(((uint64_t)g->length + g->chunk - 1) / g->chunk))
        return set_err(ZHIP_E_INVALID, "axis geometry grid length");
    if (g->grid > ZHIP_AXIS_MAX_GRID) return set_err(ZHIP_E_UNSUPPORTED, "more chunks along an axis than ZHIP_AXIS_MAX_GRID");
    if (keep_last && g->length > ZHIP_AXIS_LAST_MAX_LEN)
        return set_err(ZHIP_E_UNSUPPORTED, "keep-last on an axis longer than ZHIP_AXIS_LAST_MAX_LEN");
    if (n && (!x || ((uintptr_t)x & 7))) return set_err(ZHIP_E_INVALID, "index array null or unaligned");
    return ZHIP_OK;
}

int zhip_axis_last(const zhip_axis_geom* geom, const int64_t* d_x, uint64_t n, uint32_t* d_last, void* stream) {
    const int rc = axis_args(geom, d_x, n, true);
    if (rc != ZHIP_OK) return rc;
    if (!d_last) return set_err(ZHIP_E_INVALID, "null argument");
    if (n == 0) return ZHIP_OK;
    const int e = axis_last_launch(*geom, d_x, (uint32_t)n, d_last, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_axis_last launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

int zhip_axis_count(const zhip_axis_geom* geom, const int64_t* d_x, uint64_t n, const uint32_t* d_last,
                    uint32_t* d_counts, uint32_t* d_lo, uint32_t* d_hi, uint32_t* d_err, void* stream) {
    const int rc = axis_args(geom, d_x, n, d_last != nullptr);
    if (rc != ZHIP_OK) return rc;
    if (!d_counts || !d_lo || !d_hi || !d_err) return set_err(ZHIP_E_INVALID, "null argument");
    if (n == 0) return ZHIP_OK;
    const int e = axis_count_launch(*geom, d_x, (uint32_t)n, d_last, d_counts, d_lo, d_hi, d_err, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_axis_count launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

int zhip_axis_fill(const zhip_axis_geom* geom, const int64_t* d_x, uint64_t n, const uint32_t* d_last,
                   const uint32_t* d_first, uint32_t* d_cursor, int64_t* d_table, uint64_t table_pairs, void* stream) {
    const int rc = axis_args(geom, d_x, n, d_last != nullptr);
    if (rc != ZHIP_OK) return rc;
    if (!d_first || !d_cursor || !d_table) return set_err(ZHIP_E_INVALID, "null argument");
    if ((uintptr_t)d_table & 15) return set_err(ZHIP_E_INVALID, "pair table not 16-byte aligned");
    if (n == 0) return ZHIP_OK;
    const int e = axis_fill_launch(*geom, d_x, (uint32_t)n, d_last, d_first, d_cursor, d_table, table_pairs, stream);
    if (e != 0) return set_err(ZHIP_E_HIP, std::string("k_axis_fill launch: ") + hipGetErrorString((hipError_t)e));
    return ZHIP_OK;
}

// The three steps on the host, in index order, with the kernels' axis_locate /
// axis_pair: keep-last, count, then (no index out of range) the prefix sum and
// the fill.
int zhip_emulate_axis(const zhip_axis_geom* geom, const int64_t* x, uint64_t n, int keep_last, uint32_t* last,
                      uint32_t* counts, uint32_t* lo, uint32_t* hi, uint32_t* err, uint32_t* first, uint32_t* cursor,
                      int64_t* table, uint64_t table_pairs) {
    const int rc = axis_args(geom, x, n, keep_last != 0);
    if (rc != ZHIP_OK) return rc;
    if (!counts || !lo || !hi || !err || !first || !cursor || (n && !table) || (keep_last && !last))
        return set_err(ZHIP_E_INVALID, "null argument");
    const zhip_axis_geom& g = *geom;
    memset(counts, 0, g.grid * sizeof(uint32_t));
    memset(lo, 0, g.grid * sizeof(uint32_t));
    memset(hi, 0, g.grid * sizeof(uint32_t));
    memset(cursor, 0, g.grid * sizeof(uint32_t));
    *err = 0;
    uint32_t v, c, r;
    if (keep_last) {
        memset(last, 0, (size_t)g.length * sizeof(uint32_t));
        for (uint64_t k = 0; k < n; ++k)
            if (axis_locate(g, x[k], v, c, r) && last[v] < (uint32_t)k + 1u) last[v] = (uint32_t)k + 1u;
    }
    for (uint64_t k = 0; k < n; ++k) {
        if (!axis_locate(g, x[k], v, c, r)) {
            *err |= g.err_bit;
            continue;
        }
        if (keep_last && last[v] != (uint32_t)k + 1u) continue;
        counts[c] += 1;
        const uint32_t lw = axis_lo_word(g, r);
        if (lw > lo[c]) lo[c] = lw;
        if (r > hi[c]) hi[c] = r;
    }
    if (*err) return ZHIP_OK;
    uint32_t at = 0;
    for (uint32_t b = 0; b < g.grid; ++b) {
        first[b] = at;
        at += counts[b];
    }
    for (uint64_t k = 0; k < n; ++k) {
        if (!axis_locate(g, x[k], v, c, r)) continue;
        if (keep_last && last[v] != (uint32_t)k + 1u) continue;
        const uint64_t p = g.table_off + first[c] + cursor[c]++;
        if (p >= table_pairs) return set_err(ZHIP_E_BOUNDS, "pair index outside the table");
        axis_pair(g, k, r, table[2 * p], table[2 * p + 1]);
    }
    return ZHIP_OK;
}

uint32_t zhip_crc32c_host(const void* data, uint64_t nbytes) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    if (!nbytes) return 0u;
    static const bool hw = __builtin_cpu_supports("sse4.2");
    return hw ? crc_sse42(p, nbytes) : crc_bytewise(p, nbytes);
}

// ---- test hooks: the table images, and the kernels' CRC decompositions run on them ----
uint64_t zhip_plan_table_image(const zhip_plan* plan, int which, uint32_t* out, uint64_t cap) {
    if (!plan || which < 0 || which > 1 || (which == 1 && plan->tq < 0)) return 0;
    const std::vector<uint32_t> h = which ? build_tile_tables(*plan) : build_row_tables(*plan);
    if (out) std::memcpy(out, h.data(), std::min<uint64_t>(cap, h.size()) * sizeof(uint32_t));
    return h.size();
}

uint32_t zhip_plan_table_offsets(const zhip_plan* plan, uint64_t* out, uint32_t cap) {
    if (!plan) return 0;
    const Region* r = regions(plan->tl);
    for (uint32_t i = 0; i < kNumRegions && out; ++i) {
        if (i < cap) out[i] = r[i].off;
        if (kNumRegions + i < cap) out[kNumRegions + i] = r[i].n;
    }
    return kNumRegions;
}

extern "C++" {
// the chunk's 16 bytes at offset o as four words, zero outside the payload
static void load_block(const zhip_plan* plan, const uint8_t* data, int64_t o, uint32_t w[4]) {
    uint8_t b[16] = {0};
    for (int i = 0; i < 16; ++i) {
        const int64_t q = o + i;
        if (q >= 0 && q < (int64_t)plan->layout.nbytes) b[i] = data[q];
    }
    std::memcpy(w, b, 16);
}

static uint32_t bytes4(const uint32_t* tb, uint32_t x) {  // a [4][256] byte-slice table applied to x
    return tb[x & 255u] ^ tb[256 + ((x >> 8) & 255u)] ^ tb[512 + ((x >> 16) & 255u)] ^ tb[768 + (x >> 24)];
}

// The row kernels' four-accumulator scheme on the uploaded tables: lane i (of
// the klane region's n_lanes) runs its nblk blocks at off(i, k) through the
// 11/11/10 tables `tab`, folds the four word accumulators with the A4 tables
// and multiplies by its lane constant klane[i] (mul); lanes xor-combine.  The
// block schedule off is the kernel's.
template <class Off, class Mul>
static uint32_t emulate_lanes(const zhip_plan* plan, const uint8_t* data, const uint32_t* tab, const uint32_t* klane,
                              uint64_t n_lanes, uint32_t nblk, Off off, Mul mul) {
    auto a11 = [&](uint32_t w) {
        return tab[kPairT1 + (w & 2047u)] ^ tab[kPairT2 + ((w >> 11) & 2047u)] ^ tab[kPairT3 + (w >> 22)];
    };
    uint32_t V = 0;
    for (uint64_t i = 0; i < n_lanes; ++i) {
        uint32_t a[4] = {0, 0, 0, 0}, w[4];
        for (uint32_t k = 0; k < nblk; ++k) {
            load_block(plan, data, off((int64_t)i, (int64_t)k), w);
            for (int j = 0; j < 4; ++j) a[j] = a11(a[j] ^ w[j]);
        }
        const uint32_t* t4 = tab + kPairA4;
        V ^= mul(bytes4(t4, bytes4(t4, bytes4(t4, a[0]) ^ a[1]) ^ a[2]) ^ a[3], klane[i]);
    }
    return ~(V ^ plan->c3);
}
}

// CPU emulation of the device CRC combine for one chunk of a plan (the exact
// decomposition, and the tables and constants zhip_plan_upload puts on the
// device).  Test hook: lets the CPU suite prove the algebra without a GPU.
uint32_t zhip_emulate_chunk_crc(const zhip_plan* plan, const uint8_t* data) {
    const std::vector<uint32_t> h = build_row_tables(*plan);
    const TableLayout& T = plan->tl;
    uint32_t V = 0;
    for (uint32_t s = 0; s < plan->nseg; ++s) {
        const int64_t lo = (int64_t)plan->E - (int64_t)(s + 1) * plan->seg;
        uint32_t unit = 0;
        for (int t = 0; t < kThreads; ++t) {
            uint32_t acc = 0, w[4];
            for (int k = 0; k < (int)plan->kblocks; ++k) {
                load_block(plan, data, lo + kWgStride * k + 16 * t, w);
                auto ap = [&](int op, uint32_t x) { return bytes4(&h[T.horner.off + op * 1024], x); };
                acc = ap(0, acc ^ w[0]) ^ ap(1, w[1]) ^ ap(2, w[2]) ^ ap(3, w[3]);
            }
            unit ^= gf_mul(acc, h[T.kthread.off + t]);
        }
        V ^= gf_mul(unit, h[T.kunit.off + s]);
    }
    return ~(gf_mul(V, plan->c_inv) ^ plan->c3);
}

// k_decode_pair's scheme: unit s, lane t takes the blocks at 4096 k + 16 t of
// the unit; the windowed per-lane multiply by kpair11 (3-bit windows + a
// 2-bit top window, as the kernel's LDS tables).  Test hook.
uint32_t zhip_emulate_chunk_crc_pair(const zhip_plan* plan, const uint8_t* data) {
    auto mulx = [](uint32_t b) { return (b >> 1) ^ (kPoly & (0u - (b & 1u))); };
    auto lanemul3 = [&](uint32_t a, uint32_t k) {  // the kernel's windowed multiply
        uint32_t m3[8], m2[4];
        const uint32_t k1 = mulx(k), k2 = mulx(k1);
        for (uint32_t v = 0; v < 8; ++v) m3[v] = ((v & 4u) ? k : 0u) ^ ((v & 2u) ? k1 : 0u) ^ ((v & 1u) ? k2 : 0u);
        for (uint32_t v = 0; v < 4; ++v) m2[v] = ((v & 2u) ? k : 0u) ^ ((v & 1u) ? k1 : 0u);
        uint32_t p = m3[a & 7u];
        for (int j = 1; j < 10; ++j) p = mulx(mulx(mulx(p))) ^ m3[(a >> (3 * j)) & 7u];
        return mulx(mulx(p)) ^ m2[a >> 30];
    };
    const std::vector<uint32_t> h = build_row_tables(*plan);
    const TabSet& S = plan->tl.pair;
    return emulate_lanes(plan, data, &h[S.tab.off], &h[S.klane.off], S.klane.n, plan->kblocks,
                         [&](int64_t i, int64_t k) {
                             return (int64_t)plan->E - (i / kThreads + 1) * plan->seg + kWgStride * k + 16 * (i % kThreads);
                         },
                         lanemul3);
}

// k_decode_il's scheme: workgroup r takes steps (r / S) S 8 + r % S + S k
// (k < 8) at the interleave the decode launches take (il_choose: the widest
// built); 0xFFFFFFFF when the plan has no interleaved layout.  Test hook.
uint32_t zhip_emulate_chunk_crc_il(const zhip_plan* plan, const uint8_t* data) {
    if (!plan || !plan->il_S) return 0xFFFFFFFFu;
    const IlChoice c = il_choose(*plan, 0);
    const int64_t S = c.S, K = kDefaultBlocks;
    const int64_t lo_frame = (int64_t)plan->E - (int64_t)plan->nseg * K * kWgStride;
    const std::vector<uint32_t> h = build_row_tables(*plan);
    return emulate_lanes(plan, data, &h[c.set->tab.off], &h[c.set->klane.off], c.set->klane.n, (uint32_t)K,
                         [&](int64_t i, int64_t k) {
                             const int64_t r = i / kThreads, st0 = (r / S) * S * K + r % S;
                             return lo_frame + kWgStride * (st0 + S * k) + 16 * (i % kThreads);
                         },
                         [](uint32_t a, uint32_t k) { return gf_mul(a, k); });
}

// k_decode_xw's scheme: lane l of span r takes blocks at 8192 r + 1024 k + 16 l
// (k < 8); 0xFFFFFFFF when the plan has no xw layout.  Test hook.
uint32_t zhip_emulate_chunk_crc_xw(const zhip_plan* plan, const uint8_t* data) {
    if (!plan || !plan->xw_P) return 0xFFFFFFFFu;
    const int64_t lo_frame = (int64_t)plan->E - (int64_t)plan->nseg * kDefaultBlocks * kWgStride;
    const std::vector<uint32_t> h = build_row_tables(*plan);
    const TabSet& S = plan->tl.xw;
    return emulate_lanes(plan, data, &h[S.tab.off], &h[S.klane.off], S.klane.n, kDefaultBlocks,
                         [&](int64_t i, int64_t k) { return lo_frame + 8192 * (i / 64) + 1024 * k + 16 * (i % 64); },
                         [](uint32_t a, uint32_t k) { return gf_mul(a, k); });
}

// k_decode_il's full-row form: lane l of span group r runs one A_1024 chain
// through the blocks at 8192 (P r + s) + 1024 k + 16 l (s < P, k < 8) and
// ends on the group's last span, so its constant is k_decode_xw's of span
// P r + P - 1 (the xw lane table serves every P).  0xFFFFFFFF when the plan
// has no xw layout or its span count is no multiple of P.  Test hook.
uint32_t zhip_emulate_chunk_crc_ilx(const zhip_plan* plan, const uint8_t* data, uint32_t P) {
    if (!plan || !plan->xw_P || P == 0 || plan->xw_P % P) return 0xFFFFFFFFu;
    const int64_t lo_frame = (int64_t)plan->E - (int64_t)plan->nseg * kDefaultBlocks * kWgStride;
    const std::vector<uint32_t> h = build_row_tables(*plan);
    const TabSet& S = plan->tl.xw;
    const uint64_t n_lanes = (uint64_t)(plan->xw_P / P) * 64;
    std::vector<uint32_t> kl(n_lanes);
    for (uint64_t i = 0; i < n_lanes; ++i) kl[i] = h[S.klane.off + ((i / 64) * P + (P - 1)) * 64 + i % 64];
    return emulate_lanes(plan, data, &h[S.tab.off], kl.data(), n_lanes, kDefaultBlocks * P,
                         [&](int64_t i, int64_t k) { return lo_frame + 8192 * (i / 64) * (int64_t)P + 1024 * k + 16 * (i % 64); },
                         [](uint32_t a, uint32_t k) { return gf_mul(a, k); });
}

// CPU self-test of the identities the kernels rely on.  Returns 0 when all hold.
int zhip_selftest(void) {
    // 1. top byte of T[i] is a bijection (needed for the inverse byte step)
    const uint32_t* g_T = byte_tables().T;
    bool seen[256] = {false};
    for (int i = 0; i < 256; ++i) seen[g_T[i] >> 24] = true;
    for (int i = 0; i < 256; ++i)
        if (!seen[i]) return set_err(1, "T top-byte map is not a bijection");
    // 2. A_1(v) == gf_mul(v, x^8) and inverse round trip
    uint32_t v = 0x12345678u;
    for (int it = 0; it < 1000; ++it) {
        v = v * 1664525u + 1013904223u;
        const uint32_t a = (v >> 8) ^ g_T[v & 255u];
        if (a != gf_mul(v, xpow8(1))) return set_err(2, "A_1 != multiply by x^8");
        if (gf_mul(gf_mul(v, xpow8(777)), xpow8_inv(777)) != v) return set_err(3, "x^-8n inverse wrong");
    }
    // 3. crc of "123456789"
    if (crc_bytewise((const uint8_t*)"123456789", 9) != 0xE3069283u) return set_err(4, "check value");
    // 4. fast division
    const uint32_t ds[] = {1, 2, 3, 5, 7, 10, 15, 60, 64, 100, 255, 256, 1000, 4096, 65537, 1000003u};
    for (uint32_t d : ds) {
        const zhip_fdiv f = make_fdiv(d);
        uint32_t x = 1;
        for (int it = 0; it < 20000; ++it) {
            x = x * 1103515245u + 12345u;
            const uint32_t n = (it < 1000) ? (uint32_t)it : (x & 0x7FFFFFFFu);
            if (fdiv_apply(n, f.m, f.s) != n / d) return set_err(5, "fdiv wrong");
        }
        const uint32_t nmax = 0x7FFFFFFFu;
        if (fdiv_apply(nmax, f.m, f.s) != nmax / d) return set_err(5, "fdiv wrong at 2^31-1");
    }
    // 5. kernel decomposition == bytewise CRC for several sizes
    const uint64_t sizes[] = {0, 1, 3, 4, 15, 16, 17, 100, 4095, 4096, 4097, 32768, 32769, 100000, 262148};
    std::vector<uint8_t> buf(262148);
    uint32_t r = 7;
    for (auto& b : buf) {
        r = r * 1664525u + 1013904223u;
        b = (uint8_t)(r >> 24);
    }
    for (uint64_t n : sizes) {
        zhip_layout L{};
        L.ndim = 1;
        L.itemsize = 1;
        L.shape[0] = (int32_t)n;
        L.nbytes = n;
        zhip_plan* p = nullptr;
        if (zhip_plan_create(&L, &p) != ZHIP_OK) return 6;
        const uint32_t got = zhip_emulate_chunk_crc(p, buf.data());
        const uint32_t got_pair = zhip_emulate_chunk_crc_pair(p, buf.data());
        zhip_plan_destroy(p);
        if (got != crc_bytewise(buf.data(), n)) return set_err(7, "emulated kernel CRC wrong at n=" + std::to_string(n));
        if (got_pair != crc_bytewise(buf.data(), n))
            return set_err(8, "emulated pair-kernel CRC wrong at n=" + std::to_string(n));
    }
    return 0;
}

}  // extern "C"
