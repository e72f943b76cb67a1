// The plan's table images (zhip_plan_tables.h): one layout function that
// appends regions in address order, and one short builder per region, called
// in the same order.  Every value is exact GF(2) arithmetic, so the images are
// pure functions of the plan.
#include <algorithm>
#include <cstring>

#include "zhip_internal.h"  // zhip_plan, zhip_plan_tables.h
#include "zhip_gf2.h"

namespace zhip {

ByteTables::ByteTables() {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
        T[i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i) invtop[T[i] >> 24] = (uint8_t)i;
}

const ByteTables& byte_tables() {
    static const ByteTables t;
    return t;
}

static uint32_t gf_pow(uint32_t b, uint64_t n) {  // square-and-multiply
    uint32_t p = kOne;
    while (n) {
        if (n & 1) p = gf_mul(p, b);
        b = gf_mul(b, b);
        n >>= 1;
    }
    return p;
}

uint32_t xpow8(uint64_t n) { return gf_pow(kOne >> 8, n); }

uint32_t xpow8_inv(uint64_t n) {
    // x^-8: one inverse byte step applied to 1
    const ByteTables& bt = byte_tables();
    const uint32_t s = kOne;
    const uint32_t i = bt.invtop[s >> 24];
    return gf_pow((((s ^ bt.T[i]) & 0x00FFFFFFu) << 8) | i, n);
}

static uint32_t c96() {
    static const uint32_t c = xpow8_inv(12);
    return c;
}

uint32_t frame_const(const zhip_plan& plan, int64_t e) {
    const uint32_t xe = e >= 0 ? xpow8((uint64_t)e) : xpow8_inv((uint64_t)(-e));
    return gf_mul(gf_mul(xe, plan.c_inv), c96());
}

// The one rule for k_decode_il / k_encode_il's wider interleave: groups of
// S x 8 steps (S = 16 / 32) must tile the chunk's steps, and only plans whose
// own groups are eight wide widen (il_S = 2 / 4: the tuning arms' narrow
// groups keep theirs).  The layout has a table set (il_s) for every S that
// tiles; the launches and zhip_emulate_chunk_crc_il take the widest.
static bool il_tiles(const zhip_plan& p, uint32_t S) {
    return p.il_S == 8u && ((uint64_t)p.nseg * kDefaultBlocks) % ((uint64_t)S * kDefaultBlocks) == 0;
}

IlChoice il_choose(const zhip_plan& plan, uint32_t want) {
    const TableLayout& T = plan.tl;
    int si = want == 16u ? 0 : want == 32u ? 1 : want == 0u ? (T.il_s[1].tab.n ? 1 : 0) : -1;
    if (si >= 0 && !T.il_s[si].tab.n) si = -1;
    return si >= 0 ? IlChoice{16u << si, &T.il_s[si]} : IlChoice{plan.il_S, &T.il};
}

// Tile ti of a chunk (column block fastest, then row block, then the other
// dims, last fastest): its blocks, the stored offset of its first row and its
// out offset relative to the chunk's out_off (full selection).
struct TilePos {
    uint32_t cb, qb;
    uint64_t base;
    int64_t orel;
};

static TilePos tile_pos(const zhip_plan& p, uint32_t ti) {
    const zhip_layout& L = p.layout;
    uint32_t r = ti;
    TilePos t;
    t.cb = r % p.n_cb;
    r /= p.n_cb;
    t.qb = r % p.n_qb;
    r /= p.n_qb;
    t.base = (uint64_t)t.qb * kTileRows * p.sstride[p.tq] + (uint64_t)t.cb * kTileCols;
    t.orel = (int64_t)t.qb * kTileRows * L.out_stride[p.tq] +
             (int64_t)t.cb * (kTileCols / L.itemsize) * L.out_stride[L.ndim - 1];
    for (int d = L.ndim - 2; d >= 0; --d) {
        if (d == p.tq) continue;
        const uint32_t c = r % (uint32_t)L.shape[d];
        t.base += (uint64_t)c * p.sstride[d];
        t.orel += (int64_t)c * L.out_stride[d];
        r /= (uint32_t)L.shape[d];
    }
    return t;
}

std::vector<uint64_t> tile_bases(const zhip_plan& plan) {
    std::vector<uint64_t> base(plan.t_per_chunk);
    for (uint32_t ti = 0; ti < plan.t_per_chunk; ++ti) base[ti] = tile_pos(plan, ti).base;
    return base;
}

void fill_geom(Geom& g, const zhip_plan& plan) {
    const zhip_layout& L = plan.layout;
    g.ndim = L.ndim;
    g.itemsize = L.itemsize;
    for (int d = 0; d < ZHIP_MAX_DIMS; ++d) {
        g.shape[d] = d < L.ndim ? L.shape[d] : 1;
        g.ostride[d] = d < L.ndim ? L.out_stride[d] : 0;
        g.dshape[d] = plan.dshape[d];
    }
    g.nbytes = (uint32_t)L.nbytes;
    g.row_bytes = plan.row_bytes;
    g.drow = plan.drow;
}

// Thread t's Horner state of a tile lands at rel_t = (64 + t/16) sq + 16 (t%16)
// from the tile base; kthread shifts every thread to REF, kunit every tile from
// base + REF to R_c (past the last tile), t_c_inv from R_c to the payload end.
static uint64_t tile_ref(const zhip_plan& p) { return (uint64_t)(kTileRows + 16) * p.sstride[p.tq] + kTileCols; }

static uint64_t tile_rc(const zhip_plan& p, const std::vector<uint64_t>& base) {
    uint64_t maxb = 0;
    for (uint64_t b : base) maxb = std::max(maxb, b);
    return maxb + tile_ref(p);
}

// ---- layout ----
namespace {
struct Taker {  // appends regions in address order
    uint64_t at = 0;
    Region take(uint64_t n) {
        const Region r{n ? at : 0, n};
        at += n;
        return r;
    }
    TabSet tabset(bool on, uint64_t n_klane) {
        return on ? TabSet{take(kPairTabWords), take(n_klane), take(kThreads)} : TabSet{};
    }
    IlSet ilset(bool on, uint64_t n_klane) {
        return on ? IlSet{take(kPairTabWords), take(n_klane), take(kThreads), take(kIlBasisWords)} : IlSet{};
    }
    TileSet tileset(bool on, uint64_t n_klane) { return on ? TileSet{take(kPairTabWords), take(n_klane)} : TileSet{}; }
};
}  // namespace

void plan_layout(zhip_plan& p) {
    const zhip_layout& L = p.layout;
    const bool crc = (L.flags & ZHIP_LF_CRC) != 0;
    TableLayout& T = p.tl;
    T = TableLayout{};
    const uint64_t lanes = (uint64_t)p.nseg * kThreads;
    Taker r;
    T.horner = r.take(4096);
    T.kthread = r.take(kThreads);
    T.kunit = r.take(p.nseg);
    T.kpair = r.take(lanes);
    T.pair = r.tabset(true, lanes);
    T.il = r.ilset(p.il_S != 0, lanes);
    T.xw = r.tabset(p.xw_P != 0, (uint64_t)p.xw_P * 64);
    // k_decode_ilw (NT = 1024: tuning arms only; 512: the small-grid form of
    // k_decode_il's layouts)
    const bool ilw = (p.il_S == 8u || (ZHIP_TUNING && p.kblocks == (uint32_t)kDefaultBlocks && crc &&
                                       !(L.flags & ZHIP_LF_NO_WRITE))) &&
                     p.nseg <= 256u;
    for (int i = 0; i < 2; ++i) T.ilw[i] = r.tabset(ilw && (ZHIP_TUNING || i == 1), (uint64_t)p.nseg * (1024u >> i));
    T.ilh = r.take(ilw && p.il_S == 8u && 2 * p.nseg <= 64u ? 2 * lanes : 0);
    // k_decode_il's wider interleave (round 6): groups of 16 / 32 workgroups, the
    // same tables and constants for strides S = 16 / 32 where the chunk's steps
    // tile them (the decode and k_encode_il take the widest, il_choose; tuning
    // arms 69 / 70 / 71 force 16 / 32 / 8).  Graph-timed on the headline: S = 32
    // 25.49 / 25.33 us vs 25.76 / 25.76 for S = 8 in two interleaved pairs
    // (profiles/r06/f/)
    for (int i = 0; i < 2; ++i) T.il_s[i] = r.ilset(il_tiles(p, 16u << i), lanes);
    T.row_words = r.at;
    if (p.tq < 0) return;

    const uint64_t n = p.t_per_chunk;
    const bool t4 = p.tile4 != 0;
    Taker t;
    T.t_horner = t.take(4096);
    T.t_kthread = t.take(kThreads);
    T.t_kunit = t.take(n);
    T.tile4_tz = t.take(t4 ? 1024 : 0);
    T.tile4_kq = t.take(t4 ? (n / 4) * kThreads : 0);
    T.tile4_map = t.take(t4 ? n * (sizeof(TileEnt) / 4) : 0);
    T.g_tz = t.take(p.gd >= 0 ? 1024 : 0);
    T.g_map = t.take(p.gd >= 0 ? (uint64_t)p.n_groups * (sizeof(GroupEnt) / 4) : 0);
    // k_decode_tile4f: tile step 256 B; k_decode_tile4w: tile4 layouts with a
    // CRC; k_decode_tilegw: the same for groups
    p.tile4f = t4 && p.tile4_step == (uint64_t)kTileCols && crc;
    p.tile4w = t4 && crc;
    p.tilegw = p.gd >= 0 && crc;
    T.t4f = t.tileset(p.tile4f, (n / 4) * kThreads);
    T.t4w = t.tileset(p.tile4w, (n / 4) * kThreads);
    T.tgw = t.tileset(p.tilegw, (uint64_t)p.n_groups * kThreads);
    // the two-tile forms of k_decode_tile4w / k_encode_tile4 (at most 32
    // workgroups per chunk: the one-word publication): lane constants only
    const bool two = n % 2 == 0 && n / 2 <= 32;
    T.t2w = t.take(p.tile4w && two ? (n / 2) * kThreads : 0);
    T.t1w = t.take(ZHIP_TUNING && p.tile4w ? n * kThreads : 0);  // one tile per workgroup
    // the two-tile form of k_decode_tilegw: two workgroups per group of four
    T.tg2w = t.take(p.tilegw ? (uint64_t)p.n_groups * 2 * kThreads : 0);
    T.t2e = t.take(t4 && crc && two ? (n / 2) * kThreads : 0);
    // (tuning builds: the tile-pair decode, arm 39 -- 29.8-30.0 vs 29.2-29.4 us
    // for the grouped kernel on C3 in 128^3 chunks, profiles/r05/q/)
    const bool t2 = ZHIP_TUNING && p.tile2;
    T.tile2_tab = t.take(t2 ? kPairTabWords : 0);
    T.tile2_map = t.take(t2 ? n * (sizeof(TileEnt) / 4) : 0);
    T.tile2_klane = t.take(t2 ? (n / 2) * kThreads : 0);
    T.tgl = t.take(ZHIP_TUNING && p.tilegw ? (uint64_t)p.n_groups * kThreads : 0);  // lane-tile form, arm 40
    // (tuning arms 66 / 67: A_(4 sq) as byte tables for the chains of the
    // two-tile forms, then the A4 fold tables: kByteTabWords)
    const bool tbt = ZHIP_TUNING && (p.tile4w || p.tilegw);
    T.tbt_ad = t.take(tbt ? 1024 : 0);
    T.tbt_a4 = t.take(tbt ? kByteTabWords - 1024 : 0);
    T.tile_words = t.at;
    p.t_c_inv = xpow8_inv(tile_rc(p, tile_bases(p)) - L.nbytes);
}

// ---- builders ----
namespace {

struct Span {
    uint32_t* p;
    uint64_t n;
};
Span span(std::vector<uint32_t>& v, const Region& r) { return Span{v.data() + r.off, r.n}; }

void fill_mul_table(uint32_t* tab, uint32_t z) {  // [4 byte slices][256]: multiply by z
    for (int sl = 0; sl < 4; ++sl)
        for (uint32_t b = 0; b < 256; ++b) tab[sl * 256 + b] = gf_mul(z, b << (8 * sl));
}

void fill_horner(Span s, uint64_t stride) {  // [op][slice][256], op k = A_(stride - 4k)
    for (int op = 0; op < 4; ++op) fill_mul_table(s.p + op * 1024, xpow8(stride - 4u * op));
}

// kPairTab* layout: A_stride over 11/11/10-bit slices of a word, and the byte
// slices of A4 that fold the four word accumulators
void fill_pair_tables(Span s, uint64_t stride) {
    const uint32_t x = xpow8(stride);
    for (uint32_t i = 0; i < 2048; ++i) {
        s.p[kPairT1 + i] = gf_mul(x, i);
        s.p[kPairT2 + i] = gf_mul(x, i << 11);
    }
    for (uint32_t i = 0; i < 1024; ++i) s.p[kPairT3 + i] = gf_mul(x, i << 22);
    fill_mul_table(s.p + kPairA4, xpow8(4));
}

void fill_kthread(Span s) {
    for (uint64_t t = 0; t < s.n; ++t) s.p[t] = xpow8((uint64_t)kWgStride - 16u * t);
}

void fill_kunit(Span s, const zhip_plan& p) {
    for (uint64_t u = 0; u < s.n; ++u) s.p[u] = xpow8(u * p.seg);
}

// the per-lane constant kthread[t] * kunit[s] * c_inv of k_decode_pair, whose
// run ends then need no uniform multiply at all
void fill_kpair(Span s, const uint32_t* kthread, const uint32_t* kunit, uint32_t c_inv) {
    for (uint64_t u = 0; u < s.n / kThreads; ++u) {
        const uint32_t ku = gf_mul(kunit[u], c_inv);
        for (int t = 0; t < kThreads; ++t) s.p[u * kThreads + t] = gf_mul(kthread[t], ku);
    }
}

void fill_scaled(Span s, const uint32_t* from, uint32_t z) {
    for (uint64_t i = 0; i < s.n; ++i) s.p[i] = gf_mul(from[i], z);
}

// Lane constants of the row kernels that give every unit `lanes` lanes 16
// bytes apart: x^(8 (4096 steps(u) - 16 t)) c_inv x^(-96) for lane t of unit
// u, factored as F(u) G(t) with G(t) = x^(-128 t) (steps may be negative)
template <class F>
void fill_unit_lanes(Span s, const zhip_plan& p, uint64_t lanes, F steps) {
    const uint32_t xm128 = xpow8_inv(16);
    for (uint64_t u = 0; u < s.n / lanes; ++u) {
        uint32_t k = frame_const(p, (int64_t)kWgStride * steps((int64_t)u));
        for (uint64_t t = 0; t < lanes; ++t, k = gf_mul(k, xm128)) s.p[u * lanes + t] = k;
    }
}

// k_decode_il: workgroup r of a chunk (group r / S, offset r % S) takes
// steps st_k = (r / S) S 8 + r % S + S k; lane t's chain over them (stride
// D = 4096 S) leaves word w of step st_0 multiplied by x^(8 D 8), so the
// lane constant x^(8 (E - p_0 + 4096 - 8 D)) c_inv x^(-96) gives every
// word at p the pair kernel's x^(8 (E - p + 4096)) c_inv (p_0 = E -
// 4096 (n_steps - st_0) + 16 t); exponents may be negative
void fill_il(const zhip_plan& p, std::vector<uint32_t>& h, const IlSet& il, uint32_t il_S) {
    if (!il.tab.n) return;
    const uint64_t D = (uint64_t)kWgStride * il_S;
    const Span tab = span(h, il.tab), klane = span(h, il.klane);
    fill_pair_tables(tab, D);
    const int64_t n_steps = (int64_t)p.nseg * kDefaultBlocks, K = kDefaultBlocks, S = il_S;
    fill_unit_lanes(klane, p, kThreads, [&](int64_t r) { return n_steps - ((r / S) * S * K + r % S) + 1 - S * K; });
    // the fused index check (one 4 KiB step per lane) under A_D: its state
    // is A_D(w) instead of A4096(w), so kthread11 times x^(-8(D - 4096))
    fill_scaled(span(h, il.kidx), h.data() + p.tl.pair.kidx.off, xpow8_inv(D - (uint64_t)kWgStride));
    // the tables' bases (they are linear in the index): T1 / T2 / T3 at
    // single bits, then the four A4 byte tables -- k_decode_ilc builds the
    // tables in LDS from these 64 words instead of loading 24 KiB
    uint32_t* bs = span(h, il.basis).p;
    for (int b = 0; b < 11; ++b) bs[b] = tab.p[kPairT1 + (1u << b)];
    for (int b = 0; b < 11; ++b) bs[11 + b] = tab.p[kPairT2 + (1u << b)];
    for (int b = 0; b < 10; ++b) bs[22 + b] = tab.p[kPairT3 + (1u << b)];
    for (int j = 0; j < 4; ++j)
        for (int b = 0; b < 8; ++b) bs[32 + 8 * j + b] = tab.p[kPairA4 + 256 * j + (1u << b)];
}

// k_decode_xw: lane l of span r takes blocks p_k = lo + 8192 r + 1024 k
// + 16 l (k < 8); its chain (A_1024) leaves block 0 multiplied by
// x^(8 8192), so the constant x^(8 (E - p_0 + 4096 - 8192)) c_inv
// x^(-96) gives every word the pair kernel's frame
void fill_xw(const zhip_plan& p, std::vector<uint32_t>& h, const TabSet& xw) {
    if (!xw.tab.n) return;
    fill_pair_tables(span(h, xw.tab), 1024);
    const int64_t n_steps = (int64_t)p.nseg * kDefaultBlocks;
    fill_unit_lanes(span(h, xw.klane), p, 64, [&](int64_t r) { return n_steps - 2 * r - 1; });
    // the fused index check under A_1024: state A_1024(w) instead of A4096(w)
    fill_scaled(span(h, xw.kidx), h.data() + p.tl.pair.kidx.off, xpow8((uint64_t)kWgStride - 1024u));
}

// k_decode_ilw: lane t of unit r (NT lanes) takes the blocks at 16 t + D k
// (D = 16 NT, k < 2048 / NT); its A_D chain leaves every word w at p
// multiplied by x^(8 (p_last + D - p)), so the lane constant
// x^(8 (4096 (n_steps - 8 r - 7) - 16 t)) c_inv x^(-96) gives the pair
// kernel's frame
void fill_ilw(const zhip_plan& p, std::vector<uint32_t>& h, const TabSet& w, uint32_t NT) {
    if (!w.tab.n) return;
    const uint64_t D = 16ull * NT;
    fill_pair_tables(span(h, w.tab), D);
    const int64_t n_steps = (int64_t)p.nseg * kDefaultBlocks;
    fill_unit_lanes(span(h, w.klane), p, NT, [&](int64_t r) { return n_steps - 8 * r - 7; });
    fill_scaled(span(h, w.kidx), h.data() + p.tl.pair.kidx.off, xpow8_inv(D - (uint64_t)kWgStride));
}

// k_decode_ilh (small launches; tuning arm 41): lane t of half unit u = 2 r + h takes the
// sub-steps 8 r + 4 h + k (k < 4) at 16 t through A_4096; the constant
// x^(8 (4096 (n_steps - st0 - 3) - 16 t)) c_inv x^(-96), st0 = 8 r + 4 h
void fill_ilh(const zhip_plan& p, Span s) {
    const int64_t n_steps = (int64_t)p.nseg * kDefaultBlocks;
    fill_unit_lanes(s, p, kThreads, [&](int64_t uu) { return n_steps - (8 * (uu >> 1) + 4 * (uu & 1)) - 3; });
}

// kthread * kunit[last tile of each group of `per` tiles] * t_c_inv: the state
// carried to the group's last tile, then shifted by its unit constant
// (k_decode_tile4 / k_encode_tile4: per = 4, the encode's two-tile form: 2)
void fill_tile_kq(Span s, const zhip_plan& p, const uint32_t* kthread, const uint32_t* kunit, uint32_t per) {
    for (uint64_t g = 0; g < s.n / kThreads; ++g) {
        const uint32_t ku = gf_mul(kunit[per * g + per - 1], p.t_c_inv);
        for (int t = 0; t < kThreads; ++t) s.p[g * kThreads + t] = gf_mul(kthread[t], ku);
    }
}

// tile map (TileEnt): stored base, out offset relative to the chunk's out_off
void fill_tile_map(Span s, const zhip_plan& p) {
    for (uint32_t ti = 0; ti < s.n / 4; ++ti) {
        const TilePos t = tile_pos(p, ti);
        uint32_t* e = s.p + 4ull * ti;
        e[0] = (uint32_t)t.base;
        e[1] = 0;
        std::memcpy(e + 2, &t.orel, sizeof(t.orel));
    }
}

// k_encode_tileg / k_decode_tileg groups: tiles whose gd coordinate is
// 4m .. 4m+3, others equal; one GroupEnt per group's first tile
void fill_group_map(Span s, const zhip_plan& p, const uint32_t* kunit) {
    const zhip_layout& L = p.layout;
    // tile-index stride of the gd coordinate (natural order: cb, qb, then
    // the other dims from ndim-2 down)
    uint64_t tstride = (uint64_t)p.n_cb * p.n_qb;
    for (int d = L.ndim - 2; d > p.gd; --d)
        if (d != p.tq) tstride *= (uint64_t)L.shape[d];
    GroupEnt* gm = reinterpret_cast<GroupEnt*>(s.p);
    uint32_t g = 0;
    for (uint32_t ti = 0; ti < p.t_per_chunk; ++ti) {
        if ((ti / tstride) % (uint64_t)L.shape[p.gd] % 4u != 0u) continue;
        const TilePos t = tile_pos(p, ti);
        GroupEnt e{};
        e.tbase = (uint32_t)t.base;
        e.rows = (uint16_t)std::min<int64_t>(kTileRows, (int64_t)L.shape[p.tq] - (int64_t)t.qb * kTileRows);
        e.cols = (uint16_t)std::min<int64_t>(kTileCols, (int64_t)p.row_bytes - (int64_t)t.cb * kTileCols);
        e.orel = t.orel;
        e.ku = gf_mul(kunit[ti + 3 * tstride], p.t_c_inv);
        gm[g++] = e;
    }
}

// The lane constant of a chain of `nblk` blocks at stride D whose first block
// is at p_0 (the il kernel's frame): x^(8 (E - p_0 + 4096 - nblk D)) c_inv
// x^(-96) gives every word at p the pair kernel's x^(8 (E - p + 4096)) c_inv
uint32_t chain_const(const zhip_plan& p, int64_t p0, int64_t nblk, int64_t D) {
    return frame_const(p, (int64_t)p.E - p0 + kWgStride - nblk * D);
}

// The wave-per-tile kernels: a workgroup owns tpw = 4 / 2 / 1 tiles, 4 / tpw
// waves per tile; wave w loads rows (w % (4 / tpw)) 16 tpw + l/16 + 4 m
// (m < 4 tpw) of its tile at column block l % 16: one chain of 4 tpw blocks at
// stride D = 4 sq per lane.  tile_base(wg, j): stored offset of workgroup wg's
// j-th tile.
template <class F>
void fill_wave_klane(Span s, const zhip_plan& p, int tpw, F tile_base) {
    const int64_t sq = p.sstride[p.tq], per = 4 / tpw;
    for (uint64_t i = 0; i < s.n; ++i) {
        const int64_t t = (int64_t)(i % kThreads), w = t / 64, l = t % 64;
        const int64_t p0 = (int64_t)tile_base((uint32_t)(i / kThreads), (uint32_t)(w / per)) +
                           ((w % per) * 16 * tpw + l / 16) * sq + 16 * (l % 16);
        s.p[i] = chain_const(p, p0, 4 * tpw, 4 * sq);
    }
}

}  // namespace

std::vector<uint32_t> build_row_tables(const zhip_plan& p) {
    const TableLayout& T = p.tl;
    std::vector<uint32_t> h(T.row_words);
    const uint32_t* kthread = h.data() + T.kthread.off;
    fill_horner(span(h, T.horner), kWgStride);
    fill_kthread(span(h, T.kthread));
    fill_kunit(span(h, T.kunit), p);
    fill_kpair(span(h, T.kpair), kthread, h.data() + T.kunit.off, p.c_inv);
    // pair tables; the combined four-accumulator state sits 12 bytes later than
    // the single-chain one, so the lane constants carry x^(-96)
    fill_pair_tables(span(h, T.pair.tab), kWgStride);
    fill_scaled(span(h, T.pair.klane), h.data() + T.kpair.off, c96());
    fill_scaled(span(h, T.pair.kidx), kthread, c96());
    fill_il(p, h, T.il, p.il_S);
    fill_xw(p, h, T.xw);
    for (int i = 0; i < 2; ++i) fill_ilw(p, h, T.ilw[i], 1024u >> i);
    fill_ilh(p, span(h, T.ilh));
    for (int i = 0; i < 2; ++i) fill_il(p, h, T.il_s[i], 16u << i);
    return h;
}

std::vector<uint32_t> build_tile_tables(const zhip_plan& p) {
    const TableLayout& T = p.tl;
    std::vector<uint32_t> h(T.tile_words);
    if (p.tq < 0) return h;
    const int64_t sq = p.sstride[p.tq];
    const uint64_t REF = tile_ref(p);
    const std::vector<uint64_t> base = tile_bases(p);
    const uint64_t Rc = tile_rc(p, base);
    const uint32_t* kthread = h.data() + T.t_kthread.off;
    const uint32_t* kunit = h.data() + T.t_kunit.off;
    fill_horner(span(h, T.t_horner), 16ull * sq);
    for (int t = 0; t < kThreads; ++t)
        h[T.t_kthread.off + t] = xpow8(REF - ((uint64_t)(kTileRows + t / 16) * sq + 16u * (t % 16)));
    for (uint64_t ti = 0; ti < T.t_kunit.n; ++ti) h[T.t_kunit.off + ti] = xpow8(Rc - base[ti] - REF);
    if (T.tile4_tz.n) {
        // one table multiply (by x^(8 step)) carries a thread's Horner state from tile to tile
        fill_mul_table(span(h, T.tile4_tz).p, xpow8(p.tile4_step));
        fill_tile_kq(span(h, T.tile4_kq), p, kthread, kunit, 4);
        fill_tile_map(span(h, T.tile4_map), p);
    }
    const GroupEnt* gm = reinterpret_cast<const GroupEnt*>(h.data() + T.g_map.off);
    const int64_t gstep = p.gd >= 0 ? (int64_t)p.sstride[p.gd] : 0;
    if (T.g_tz.n) {
        fill_mul_table(span(h, T.g_tz).p, xpow8(p.sstride[p.gd]));
        fill_group_map(span(h, T.g_map), p, kunit);
    }
    if (T.t4f.tab.n) {
        // k_decode_tile4f: the four tiles of a group are the 256-byte pieces of
        // 1 KiB of every stored row (step 256), so thread t's blocks (row t/4,
        // 16 (t%4) + 64 n, n < 16) form one chain of stride 64 B: A_64 tables
        fill_pair_tables(span(h, T.t4f.tab), 64);
        const Span s = span(h, T.t4f.klane);
        for (uint64_t i = 0; i < s.n; ++i) {
            const int64_t t = (int64_t)(i % kThreads);
            s.p[i] = chain_const(p, (int64_t)base[4 * (i / kThreads)] + (t / 4) * sq + 16 * (t % 4), 16, 64);
        }
    }
    if (T.t4w.tab.n) {  // k_decode_tile4w: wave w of workgroup g owns tile 4 g + w
        fill_pair_tables(span(h, T.t4w.tab), 4ull * sq);
        fill_wave_klane(span(h, T.t4w.klane), p, 4, [&](uint32_t g, uint32_t j) { return base[4 * g + j]; });
    }
    if (T.tgw.tab.n) {  // k_decode_tilegw: as k_decode_tile4w, tile w of group g at gm[g].tbase + w step(gd)
        fill_pair_tables(span(h, T.tgw.tab), 4ull * sq);
        fill_wave_klane(span(h, T.tgw.klane), p, 4, [&](uint32_t g, uint32_t j) { return gm[g].tbase + j * gstep; });
    }
    // two tiles per workgroup: tiles 2 g, 2 g + 1
    fill_wave_klane(span(h, T.t2w), p, 2, [&](uint32_t g, uint32_t j) { return base[2 * g + j]; });
    fill_wave_klane(span(h, T.t1w), p, 1, [&](uint32_t ti, uint32_t) { return base[ti]; });
    // workgroup 2 g + h of a chunk: tiles 2 h, 2 h + 1 of group g
    fill_wave_klane(span(h, T.tg2w), p, 2,
                    [&](uint32_t wg, uint32_t j) { return gm[wg / 2].tbase + (2 * (wg % 2) + j) * gstep; });
    fill_tile_kq(span(h, T.t2e), p, kthread, kunit, 2);
    if (T.tile2_tab.n) {  // k_decode_tile4w<2> over consecutive tile pairs where tile4 declines
        fill_pair_tables(span(h, T.tile2_tab), 4ull * sq);
        fill_tile_map(span(h, T.tile2_map), p);
        fill_wave_klane(span(h, T.tile2_klane), p, 2, [&](uint32_t g, uint32_t j) { return base[2 * g + j]; });
    }
    {
        // k_decode_tilegw, lanes pick the tile: lane l of wave w takes rows w + 4 m
        // (m < 16) of tile l / 16 at column block l % 16
        const Span s = span(h, T.tgl);
        for (uint64_t i = 0; i < s.n; ++i) {
            const int64_t t = (int64_t)(i % kThreads), w = t / 64, l = t % 64;
            s.p[i] = chain_const(p, (int64_t)gm[i / kThreads].tbase + (l / 16) * gstep + w * sq + 16 * (l % 16), 16, 4 * sq);
        }
    }
    if (T.tbt_ad.n) {
        fill_mul_table(span(h, T.tbt_ad).p, xpow8(4ull * sq));
        fill_mul_table(span(h, T.tbt_a4).p, xpow8(4));
    }
    return h;
}

}  // namespace zhip
