// Plan table images: where every region of a plan's two device allocations
// (d_tables: the row image, d_tile_tables: the tile image) lies, and the host
// builders that fill them (plan_tables.cpp).  Host only: no HIP calls, no error
// strings.  DESIGN.md "Plan table images" lists every region, its size, when
// it is present and the kernels that read it.
#pragma once
#include <stdint.h>

#include <vector>

struct zhip_plan;

namespace zhip {

struct Geom;

struct Region {
    uint64_t off, n;  // u32 words into the image; n == 0 (and off == 0): absent
};
// 11/11/10 tables of one operator (kPairTab* layout) | lane constants | the
// fused index check's lane constants under those tables
struct TabSet {
    Region tab, klane, kidx;
};
struct IlSet {  // k_decode_il: a TabSet and the tables' single-bit entries (kIlBasisWords)
    Region tab, klane, kidx, basis;
};
struct TileSet {
    Region tab, klane;
};

// Declaration order is address order within each image.
struct TableLayout {
    // row image
    Region horner, kthread, kunit, kpair;
    TabSet pair;
    IlSet il;       // the plan's own il_S (2 / 4 / 8)
    TabSet xw;
    TabSet ilw[2];  // NT = 1024 (tuning builds) / 512
    Region ilh;
    IlSet il_s[2];  // S = 16 / 32 where the chunk's steps tile them
    // tile image
    Region t_horner, t_kthread, t_kunit;
    Region tile4_tz, tile4_kq, tile4_map;
    Region g_tz, g_map;
    TileSet t4f, t4w, tgw;
    Region t2w, t1w, tg2w, t2e;
    Region tile2_tab, tile2_map, tile2_klane;
    Region tgl;
    Region tbt_ad, tbt_a4;
    uint64_t row_words, tile_words;  // image sizes (tile_words 0: no tile image)
};
constexpr uint32_t kNumRegions = (sizeof(TableLayout) - 2 * sizeof(uint64_t)) / sizeof(Region);
static_assert(sizeof(TableLayout) == kNumRegions * sizeof(Region) + 2 * sizeof(uint64_t), "TableLayout: regions only");
inline const Region* regions(const TableLayout& t) { return reinterpret_cast<const Region*>(&t); }

// CRC-32C byte table (A_1(v) = (v >> 8) ^ T[v & 255]) and its top-byte inverse
struct ByteTables {
    uint32_t T[256];
    uint8_t invtop[256];
    ByteTables();
};
const ByteTables& byte_tables();
uint32_t xpow8(uint64_t n);      // x^(8n) mod P
uint32_t xpow8_inv(uint64_t n);  // x^(-8n) mod P
// x^(8e) c_inv x^(-96) for signed e: the lane constant of every kernel that
// folds four word accumulators (the combined state sits 12 bytes later than
// the single-chain one, hence x^(-96))
uint32_t frame_const(const zhip_plan& plan, int64_t e);

// k_decode_il / k_encode_il's interleave: the table set for `want` = 16 / 32
// where the plan built it, else (and for want = 8) the plan's own; want = 0:
// the widest built, which the production launches take
struct IlChoice {
    uint32_t S;
    const IlSet* set;
};
IlChoice il_choose(const zhip_plan& plan, uint32_t want);

// Source offset of every tile's first row in the stored chunk (tile index:
// column block fastest, then row block, then the other dims, last fastest).
std::vector<uint64_t> tile_bases(const zhip_plan& plan);
void fill_geom(Geom& g, const zhip_plan& plan);

// Fills plan.tl and the facts that follow from it (tile4f / tile4w / tilegw,
// t_c_inv); zhip_plan_create calls it once the geometry is final.
void plan_layout(zhip_plan& plan);
// The two images, pure functions of the plan (build_tile_tables: tq >= 0 only).
std::vector<uint32_t> build_row_tables(const zhip_plan& plan);
std::vector<uint32_t> build_tile_tables(const zhip_plan& plan);

}  // namespace zhip
