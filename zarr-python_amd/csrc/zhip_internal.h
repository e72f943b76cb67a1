// Internal (non-ABI) structures shared by the plan builder and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/zarrhip.h"
#include "zhip_plan_tables.h"

namespace zhip {

constexpr int kThreads = 256;                            // one workgroup = 4 waves
constexpr int kWgStride = kThreads * 16;                 // 4 KiB per workgroup step
constexpr int kDefaultBlocks = 8;                        // 16-byte blocks per thread per unit
// workspace words per chunk of CRC layouts (zhip_plan_info): k_decode_il /
// k_decode_tile4 publish into word kPubLine * c, one 128-byte line per chunk
// (32 workgroups' returning atomics per line instead of 8 chunks' 256)
constexpr uint32_t kPubLine = 32;

// Stored-chunk geometry + out mapping (shared by decode and encode).
struct Geom {
    int32_t ndim, itemsize;
    int32_t shape[ZHIP_MAX_DIMS];
    int64_t ostride[ZHIP_MAX_DIMS];
    zhip_fdiv dshape[ZHIP_MAX_DIMS];
    uint32_t nbytes;  // N (< 2^31)
    uint32_t row_bytes;
    zhip_fdiv drow;
};

// Kernel argument block (passed by value; indexed only with compile-time
// subscripts inside the kernels so it stays in SGPRs / kernarg memory).
// One tile of a chunk (k_decode_tile4): source offset of its first row in the
// stored chunk, out offset relative to the chunk's out_off.
struct TileEnt {
    uint32_t tbase, _pad;
    int64_t orel;
};

// One group of k_encode_tileg: its first tile's stored offset and array
// offset (relative to the chunk), the tiles' row / byte extent (partial tiles
// at the chunk's edges), and kunit[its last tile] * t_c_inv.
struct GroupEnt {
    uint32_t tbase;
    uint16_t rows, cols;
    int64_t orel;
    uint32_t ku, _pad;
};

// k_decode_pair CRC table layout (u32 words): A4096 by the 11 low, 11 middle
// and 10 high bits of a word, then the four byte slices of A4 (x^32).
constexpr int kPairT1 = 0, kPairT2 = 2048, kPairT3 = 4096, kPairA4 = 5120;
constexpr int kPairTabWords = 6144;
// the byte-table form of the same operator (tuning arms 66 / 67: k_decode_tile4w
// / k_decode_tilegw): A_D's four 256-entry byte tables, then the A4 fold tables
constexpr int kByteTabWords = 2048;
extern const char* g_last_kernel;  // zhip_last_kernel: the kernel the last decode / mapped encode launched
extern uint32_t g_last_grid;       // zhip_last_grid: that launch's workgroups (fire)
constexpr uint32_t kIlwMaxUnits = 512;  // k_decode_ilw (512 lanes) for grids of at most 2 units per CU
// k_decode_il's full-row form: 8 KiB spans a wave streams per workgroup (32 arrivals per 1 MiB chunk, as
// k_decode_il's 32 KiB units; 512 workgroups per headline program.  Two spans -- 1 024 workgroups, 64 arrivals --
// copy 0.5 us slower in the codec-free landscape, profiles/r10/)
constexpr uint32_t kIlxSpans = 4;
constexpr int kIlBasisWords = 64; // T1 / T2 / T3 bases (11 + 11 + 10, padded to 32), A4 bases (4 x 8)

// What k_decode_lead (and the k_decode_il arm) need before their first vector loads,
// FIRST in the kernel arguments and read as one scalar batch (pair_hot): the
// lazily scheduled kernarg loads of the full struct put five to seven
// dependent round trips (and software divisions) between the kernel start and
// the first data load.  Divisors are host-built magic numbers (zhip_fdiv).
struct PairHot {
    uint32_t n_units, nseg, n_idx, xcd_run;
    zhip_fdiv d_nseg, d_xcd, d_per;
    uint32_t pred, pred_per, E, seg;
    uint32_t tune, pad;
    uint64_t pred_base, pred_outer, pred_inner;
    uint64_t src, pair_tab, kpair11, kthread11;
    // k_decode_il
    uint32_t il_S, n_chunks;
    uint64_t il_tab, il_klane, il_kidx;
};

struct DecodeParams {
    PairHot h;
    const uint8_t* src;
    uint64_t src_size;
    uint8_t* out;
    const zhip_chunk* chunks;
    const zhip_sel* sels;
    zhip_status* status;
    uint32_t* ws;
    uint32_t* errflag;
    const uint32_t* horner;   // [4 operators][4 byte slices][256]
    uint32_t hx[4];           // x^(8(4096 - 4k)): the operators, for in-kernel table builds
    uint32_t kq[32];          // lane-shift factors (lane_kthread)
    const uint32_t* kthread;  // [kThreads]
    const uint32_t* kunit;    // [nseg]
    const uint32_t* kpair;    // [nseg][kThreads]: kthread * kunit * c_inv (k_decode_pair)
    // k_decode_pair's CRC tables (kPairTab* layout): A4096 in 11/11/10-bit
    // slices (one operator for all four words: four accumulators per lane) and
    // the A4 byte tables that combine them, then kpair and kthread times
    // x^(-96) (the frame of the combined state), [nseg][kThreads] and [kThreads]
    const uint32_t* pair_tab;
    const uint32_t* kpair11;
    const uint32_t* kthread11;
    uint32_t n_chunks, nseg, n_units;
    uint32_t c_inv, c3;
    uint32_t lflags;
    Geom g;
    uint32_t seg;     // bytes per unit = kWgStride * K
    uint32_t E;       // align16(N)
    uint32_t index_size, n_inner;
    uint32_t fill[4];
    uint32_t fast;
    uint32_t tune;  // kTune* ablation bits (0 in production)
    // tile mode (transposed chunks: stored dim tq is contiguous in out)
    int32_t tq;
    uint32_t t_per_chunk, n_qb, n_cb;
    uint32_t sstride[ZHIP_MAX_DIMS];  // stored-stream byte stride of each dim
    zhip_fdiv d_qb, d_cb;
    // k_decode_tile4 (tile4 != 0): see zhip_plan
    uint32_t tile4;
    uint32_t tile2;  // k_decode_tile4w's two-tile form over consecutive tile pairs (plans without tile4)
    const uint32_t* tz;
    const uint32_t* kq4;
    const struct TileEnt* tmap;
    // k_decode_tile4f (non-null: the layout qualifies): A_64 pair tables, lane constants
    const uint32_t* t4f_tab;
    const uint32_t* t4f_kq;
    // k_decode_tile4w / k_decode_tilegw (non-null: taken): A_(4 sq) pair
    // tables, lane constants [T/4 or n_groups][kThreads]
    const uint32_t* t4w_tab;
    const uint32_t* t4w_kq;
    const uint32_t* t2w_kq;  // k_decode_tile4w with two tiles per workgroup (production when set): lane constants
    const uint32_t* t1w_kq;  // tuning arm 37 (one tile per workgroup)
    const uint32_t* tglt_kq; // tuning arm 40 (k_decode_tilegw, lanes pick the tile): lane constants
    const uint32_t* tbt_tab; // tuning arms 66 / 67: A_(4 sq) as byte tables + A4 (kByteTabWords)
    // k_decode_tileg (tileg != 0): group map, step multiply table, steps
    uint32_t tileg;
    const struct GroupEnt* gmap;
    const uint32_t* gtz;
    uint32_t n_groups, g_step_t, n_sub;
    int64_t g_step_o;
    // fused shard-index CRC verification: workgroup g checks indexes g, g+G, ...
    const zhip_chunk* idx_chunks;
    zhip_status* idx_status;
    uint32_t n_idx, idx_nbytes, idx_E, idx_c_inv, idx_c3;
    // whole-row affine mapping (ZHIP_DF_ROWS, k_decode_rows): rows of 2^row_shift
    // bytes, 4096 / row_bytes rows per workgroup step, never crossing dim ndim-2
    uint32_t row_shift, r_sy;  // log2(row_bytes), shape[ndim-2]
    zhip_fdiv r_dy;            // division by shape[ndim-2]
    int64_t r_oy;              // out stride of dim ndim-2
    int32_t nd2;               // ndim - 2
    uint32_t rows;             // 1: launch k_decode_rows
    uint32_t xcd_run;          // k_decode_pair: pairs per XCD-contiguous run (0: dispatch order)
    const zhip_rowblk* rowmap; // per (sel, unit, step) destinations (zhip_rows_map); k_decode_pair
    // k_decode_il: interleave stride (steps), its A_(4096 S) tables, lane
    // constants per workgroup-in-chunk and for the fused index check
    uint32_t il_S;
    const uint32_t* il_tab;
    const uint32_t* il_klane;
    const uint32_t* il_kidx;
    const uint32_t* il_basis;  // kIlBasisWords: the il tables' single-bit entries (k_decode_ilc)
    uint32_t dv_bank;  // deferred CRC verdicts: bank this launch publishes into (ZHIP_DF_BANK1)
    uint32_t defer;    // ZHIP_DF_DEFER: the caller reads deferred verdicts (tileg / tilegw publish so)
    // k_decode_xw: 8 KiB spans per chunk (0: not available), arrival subwords
    // per chunk in the workspace tail (0: one level or xor + count), its A_1024
    // tables, lane constants per (span, lane) and for the fused index check
    uint32_t xw, xw_nsub;
    const uint32_t* xw_tab;
    const uint32_t* xw_klane;
    const uint32_t* xw_kidx;
    // k_decode_ilw (small shares): ilw_nt lanes per 32 KiB unit (0: not
    // available), its A_(16 ilw_nt) tables, lane constants per (unit, lane),
    // the fused index check's lane constants
    uint32_t ilw_nt;
    const uint32_t* ilh_klane;  // tuning arm 41 (k_decode_ilh, 16 KiB per workgroup): lane constants [2 nseg][kThreads]
    const uint32_t* ilw_tab;
    const uint32_t* ilw_klane;
    const uint32_t* ilw_kidx;
    // ZHIP_DF_WHOLE launches of a plan with aff_ok: the row map of the whole
    // chunk as rel(st) = (st >> aff_sh) aff_B + (st & aff_mask) aff_C + aff_D
    // (zhip_plan aff_*); k_decode_il / k_decode_ilw take their AFF form
    uint32_t aff_ok, aff_sh, aff_mask;
    int32_t aff_B, aff_C, aff_D;
    // load-address prediction (zhip_predict; k_decode_pair): payload of chunk c
    // predicted at src + pred_base + (c / pred_per) * pred_outer + (c % pred_per) * pred_inner
    uint32_t pred, pred_per;
    uint64_t pred_base, pred_outer, pred_inner;
};

// The one argument of k_decode_il_multi (zhip_decode_mapped_multi): the
// parameters of n independent k_decode_il launches and the prefix sums of
// their grids -- workgroups [g0[i], g0[i + 1]) of the fused grid are launch
// i's.  ZHIP_MULTI_MAX is what fits a 4 KiB kernel-argument segment.
#define ZHIP_MULTI_MAX 3
template <int N>
struct MultiParamsN {
    DecodeParams q[N];
    uint32_t g0[N + 1];
    uint32_t n;
};
using MultiParams = MultiParamsN<ZHIP_MULTI_MAX>;
static_assert(sizeof(MultiParams) <= 4096 && sizeof(MultiParamsN<ZHIP_MULTI_MAX + 1>) > 4096,
              "ZHIP_MULTI_MAX: the DecodeParams that fit a 4 KiB kernel-argument segment");

// n / d == (n * m) >> s for 0 <= n < 2^31 (host side; fdiv_apply on the device)
inline zhip_fdiv make_fdiv(uint32_t d) {
    zhip_fdiv f;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    f.s = 31 + l;
    f.m = (uint32_t)(((1ull << (31 + l)) + d - 1) / d);  // ceil(2^(31+l) / d) < 2^32 for d >= 1
    return f;
}

// PairHot from the full parameters (after every field is final); xcd_run and
// its divisor are set again by launch_decode
inline void fill_pair_hot(DecodeParams& p) {
    PairHot& h = p.h;
    h.n_units = p.n_units;
    h.nseg = p.nseg;
    h.n_idx = p.n_idx;
    h.xcd_run = p.xcd_run;
    h.d_nseg = make_fdiv(p.nseg ? p.nseg : 1u);
    h.d_xcd = make_fdiv(p.xcd_run ? p.xcd_run : 1u);
    h.d_per = make_fdiv(p.pred_per ? p.pred_per : 1u);
    h.pred = p.pred;
    h.pred_per = p.pred_per;
    h.E = p.E;
    h.seg = p.seg;
    h.tune = p.tune;
    h.pad = 0;
    h.pred_base = p.pred_base;
    h.pred_outer = p.pred_outer;
    h.pred_inner = p.pred_inner;
    h.src = reinterpret_cast<uint64_t>(p.src);
    h.pair_tab = reinterpret_cast<uint64_t>(p.pair_tab);
    h.kpair11 = reinterpret_cast<uint64_t>(p.kpair11);
    h.kthread11 = reinterpret_cast<uint64_t>(p.kthread11);
    h.il_S = p.il_S;
    h.n_chunks = p.n_chunks;
    h.il_tab = reinterpret_cast<uint64_t>(p.il_tab);
    h.il_klane = reinterpret_cast<uint64_t>(p.il_klane);
    h.il_kidx = reinterpret_cast<uint64_t>(p.il_kidx);
}

constexpr int kTileRows = 64;    // rows of the contiguous-in-out dim per tile
constexpr int kTileCols = 256;   // bytes of the innermost stored row per tile

// Ablation / tuning knobs (zhip_set_tuning): never set on the product path.
constexpr uint32_t kTuneSkipCrc = 1u;   // replace the CRC lookups by a plain xor
constexpr uint32_t kTuneAcqRel = 2u;    // acq_rel ticket (the round-1 first version)
constexpr uint32_t kTuneNoTicket = 4u;  // xor only, no last-arriver finalize
constexpr uint32_t kTuneNT = 8u;        // nontemporal loads / stores (fast rows path)
constexpr uint32_t kTuneNoLaneMul = 16u; // rows kernel: skip the per-lane shift multiply
constexpr uint32_t kTunePersist = 64u;   // whole-row layouts: persistent k_decode_rows instead of k_decode_pair
constexpr uint32_t kTuneSingle = 128u;   // k_decode_pair with one unit per workgroup
constexpr uint32_t kTuneSerialize = 256u; // k_decode_pair: wait for every load before the first store
constexpr uint32_t kTuneNoTables = 512u;  // k_decode_pair: skip the in-LDS table build (results invalid)
constexpr uint32_t kTuneTrailingCrc = 2048u; // k_decode_pair: CRC lookups after all stores (default: per block; headline type)
constexpr uint32_t kTuneNoRunEnd = 4096u;  // k_decode_pair: skip the run-end reduction entirely (results invalid)
constexpr uint32_t kTuneNoBarrier = 8192u; // k_decode_pair: skip the table barrier (results invalid)
constexpr uint32_t kTuneNoConsts = 32768u; // k_decode_pair: skip the lane-constant and trailer loads (results invalid)
constexpr uint32_t kTuneTile1 = 65536u;  // transposed layouts: the one-tile persistent k_decode_tile
constexpr uint32_t kTuneSplitChain = 262144u; // k_decode_pair: independent Horner chains for the two units
constexpr uint32_t kTuneEncNoFlags = 524288u; // k_encode_pair: skip the non-empty flag atomics (results invalid)
constexpr uint32_t kTuneNoTile4 = 1048576u;   // transposed layouts: grouped k_*_tileg where k_*_tile4 would run
constexpr uint32_t kTuneDuo = 2097152u;       // whole-row layouts: k_decode_duo (one unit per half of a 512-thread workgroup)
constexpr uint32_t kTuneNoXcd = 8388608u;     // k_decode_pair: plain dispatch order (no XCD-contiguous runs)
constexpr uint32_t kTunePrio = 16777216u;     // k_decode_pair arm: s_setprio(1) once a wave's loads are out
constexpr uint32_t kTuneDeferB = 33554432u;   // k_decode_pair arm: unit B's loads interleaved with A's stores
constexpr uint32_t kTuneIl = 67108864u;       // whole-row layouts: k_decode_il wherever the layout admits it
constexpr uint32_t kTuneNoIl = 134217728u;    // whole-row layouts: never k_decode_il (k_decode_pair)
constexpr uint32_t kTuneXw = 268435456u;      // whole-row layouts: k_decode_xw where admitted
constexpr uint32_t kTuneNoXw = 536870912u;    // whole-row layouts: never k_decode_xw, nor k_decode_il's full-row form
                                              // (any tuning bit or arm keeps the interleaved k_decode_il: the A/B knob)
constexpr uint32_t kTuneNoPub = 1073741824u;  // timing arm: k_decode_il / k_decode_xw skip the CRC publication
constexpr uint32_t kTuneIlLean = 16384u;    // k_decode_il arm: lean predicted prologue (data loads before the header chain)
constexpr uint32_t kTuneTile4F = 2147483648u;   // transposed layouts arm: k_decode_tile4f where the layout admits it
constexpr uint32_t kTuneIlRegMul = 32u;      // k_decode_il arm: lane multiply in registers (no LDS column)
constexpr uint32_t kTuneIlOcc6 = 4194304u;   // k_decode_il arm: register lane multiply, 6 workgroups per CU
constexpr uint32_t kTuneCfLookup = 131072u;  // k_decode_il timing arm: conflict-free lookup addresses (results invalid)
constexpr uint32_t kTuneStamp = 1024u;    // k_decode_pair: per-workgroup phase timestamps (zhip_debug_stamps)
constexpr uint32_t kStampWG = 8192u;      // workgroups stamped per launch
constexpr uint32_t kStampSlots = 8u;
}  // namespace zhip
extern "C" void zhip_stage_set_streams(uint32_t n);  // staging.cpp (ZHIP_TUNE_STAGE_STREAMS)
extern "C" void zhip_stage_set_copy(uint32_t nt);     // staging.cpp (ZHIP_TUNE_STAGE_COPY)
namespace zhip {
// The kernel knobs (zhip_set_tuning ZHIP_TUNE_MAX_GRID / ABLATION / BLOCKS /
// ARM) and every measurement-arm kernel exist only in the tuning build
// (make tune -> libzarrhip_tune.so, -DZHIP_TUNING=1; scripts/armbench.py).
// The shipped library has them as compile-time zeros: no arm is compiled in
// and no variable of a user's environment can change a launch.
#ifndef ZHIP_TUNING
#define ZHIP_TUNING 0
#endif
#if ZHIP_TUNING
extern int g_tune_max_grid;
extern int g_tune_blocks;
extern uint32_t g_tune_bits;
extern int g_tune_arm;  // ZHIP_TUNE_ARM: experimental kernel variant (0 = production)
#else
constexpr int g_tune_max_grid = 0;
constexpr int g_tune_blocks = 0;
constexpr uint32_t g_tune_bits = 0;
constexpr int g_tune_arm = 0;
#endif

// The values of ZHIP_TUNE_ARM (g_tune_arm): the list of record.  The numbers
// are frozen (tests, scripts/ and profiles/ carry them).  An arm changes only
// the launches of the kernel family named with it; everywhere else, and for
// any number not listed, the production rule holds.  Most arm kernels exist
// for the headline item type only (4-byte little-endian items, CRC).
enum Arm : int {
    kArmProduction = 0,
    kArmPub16 = 1,          // k_decode_il / k_decode_tile4: publication words 16 B apart (round 3);
                            // k_encode_pair: 11/11/10 tables
    kArmDeferred = 2,       // k_decode_il / k_decode_tile4: deferred verdicts; tile layouts: k_decode_tile4 /
                            // k_decode_tileg / four-tile k_decode_tilegw, the returning publication
    kArmNoWaveTile = 5,     // tile layouts: k_decode_tile4 / k_decode_tileg where the wave-per-tile kernels would run
    kArmEncPub16 = 9,       // encodes: chunks' publication words 16 B apart, not a line
    kArmNoLead4 = 11,       // chunks of <= 16 KiB: the pair kernels, not k_decode_lead4 / k_encode_quad
    kArmLead4 = 12,         // chunks of <= 8 KiB: four per workgroup (k_decode_lead4)
    kArmLead8 = 13,         // chunks of <= 8 KiB: eight per workgroup (k_decode_lead8)
    kArmIlq2 = 20,          // k_decode_ilq: two units per workgroup
    kArmIlq4 = 21,          // k_decode_ilq: four
    kArmIlq1Glds = 22,      // k_decode_ilq: one, tables by LDS-DMA
    kArmIlq2Glds = 23,      // k_decode_ilq: two, tables by LDS-DMA
    kArmIlq4Glds = 24,      // k_decode_ilq: four, tables by LDS-DMA
    kArmIlc = 25,           // k_decode_ilc: tables built in LDS, predicted loads first
    kArmIlw1024 = 26,       // k_decode_ilw: 1024 lanes per unit
    kArmIlw512 = 27,        // k_decode_ilw: 512 lanes per unit, whatever the grid
    kArmProbeArgs = 28,     // k_probe: a decode-shaped grid with the decode's arguments (results invalid)
    kArmProbeLds = 29,      // k_probe: plus k_decode_il's LDS footprint
    kArmProbeHeader = 30,   // k_probe: plus each workgroup's header chain
    kArmIlw1024Reg = 31,    // k_decode_ilw: 1024 lanes, the lane multiply in registers
    kArmIlw512Reg = 32,     // k_decode_ilw: 512 lanes, the lane multiply in registers
    kArmKeepIl = 33,        // small grids: k_decode_il (read nowhere: any arm the small-grid rule does not name does this)
    kArmEncNoIl = 34,       // encodes: k_encode_pair where k_encode_il would run
    kArmIlp = 35,           // k_decode_ilp: index entry off the stores' path (predicted plans)
    kArmEncTileg2 = 36,     // k_encode_tileg: two workgroups per group, two tiles each
    kArmTile1w = 37,        // k_decode_tile4w: one tile per workgroup
    kArmTileFour = 38,      // k_decode_tile4w / k_decode_tilegw / k_encode_tile4: four tiles per workgroup, not two
    kArmTilePairs = 39,     // layouts that tile4 declines: k_decode_tile4w<2> over consecutive tile pairs (k_decode_tilep)
    kArmTilegLanes = 40,    // k_decode_tilegw: four tiles, lanes pick the tile
    kArmIlh = 41,           // k_decode_ilh with the returning publication
    kArmIlw512Half = 42,    // k_decode_ilw: 512 lanes, half the lane multiply in registers
    kArmRowMap = 45,        // ZHIP_DF_WHOLE decodes: keep the row-map loads (no AFF form)
    kArmEncAff = 46,        // k_encode_il: the AFF form for ZHIP_DF_WHOLE encodes
    kArmEncTilegSpread = 47,   // k_encode_tileg: four tiles, arrival words on lines of their own
    kArmTilegPacked = 48,   // k_decode_tilegw's two-tile form: the arrival words packed (round-4 layout)
    kArmSplitPub = 49,      // k_decode_il / k_decode_ilw / k_decode_tile4w: the split publication
    kArmEncTileg2Spread = 50,  // k_encode_tileg: two tiles, arrival words on lines of their own
    kArmIlPrioRunEnd = 51,  // k_decode_il (AFF): wave priority at the run end
    kArmIlPrioLoads = 52,   // k_decode_il (AFF): at the load issue
    kArmIlPrioBoth = 53,    // k_decode_il (AFF): both
    kArmIlPrioTables = 54,  // k_decode_il (AFF): to the tables (production)
    kArmIlPrioTablesEnd = 55,  // k_decode_il (AFF): 54 + run end
    kArmIlNoPrio = 56,      // k_decode_il (AFF): no priority (round-5 production)
    kArmIlXcd = 57,         // k_decode_il (AFF): 54 + XCD-contiguous eighths
    kArmLookBack = 58,      // k_decode_il / k_decode_ilw (AFF): the look-back finalizer
    kArmIlhLookBack = 59,   // k_decode_ilh: the look-back finalizer without the AFF form
    kArmIlhProduction = 60, // small grids: production's k_decode_ilh, by number
    kArmIlw512Small = 61,   // small grids: k_decode_ilw512 (round-5 production), not k_decode_ilh
    kArmTilegLookBack = 62, // k_decode_tilegw's two-tile form: the look-back finalizer
    kArmEncTilegLookBack = 63,  // k_encode_tileg: four tiles, the look-back finalizer
    kArmIlStoreWt = 64,     // k_decode_il (AFF): write-through stores
    kArmIlStoreNt = 65,     // k_decode_il (AFF): nontemporal buffer stores
    kArmTilegByteTab = 66,  // k_decode_tilegw's two-tile form: byte-table chains
    kArmTile2wByteTab = 67, // k_decode_tile4w's two-tile form: byte-table chains
    kArmEncTilegA4 = 68,    // k_encode_tileg: four accumulators through one byte-table operator
    kArmIlS16 = 69,         // k_decode_il: interleave stride 16
    kArmIlS32 = 70,         // k_decode_il: 32
    kArmIlS8 = 71,          // k_decode_il: 8
    kArmEncIlS8 = 73,       // k_encode_il: interleave stride 8
};
inline bool arm_in(Arm lo, Arm hi) { return g_tune_arm >= lo && g_tune_arm <= hi; }

struct EncodeParams {
    const uint8_t* arr;   // source array base (device)
    uint8_t* dst;         // encoded destination buffer
    const zhip_chunk* chunks;  // src = dst offset of the encoded chunk, out_off = arr offset
    const zhip_sel* sels;
    zhip_status* status;
    uint32_t* ws;
    uint32_t* nonempty;
    const uint32_t* horner;
    const uint32_t* kthread;
    const uint32_t* kunit;
    uint32_t n_chunks, nseg, n_units;
    uint32_t c_inv, c3;
    uint32_t lflags;
    Geom g;
    uint32_t seg, E;
    uint32_t fill[4];
    uint32_t fill_nan;
    uint32_t fast;
    // k_encode_pair (zhip_encode_mapped): row map and per-lane constants as in
    // the two-unit decode; rows of 2^row_shift bytes, r_oy = arr stride of dim ndim-2
    const zhip_rowblk* rowmap;
    const uint32_t* kpair;
    const uint32_t* pair_tab;  // k_encode_pair: the 11/11/10 tables and their lane constants (kpair11)
    const uint32_t* kpair11;
    uint32_t row_shift;
    int64_t r_oy;
    uint32_t tune;
    // k_encode_tile4 (ZHIP_DF_TILE on a tile4 plan): see zhip_plan / k_decode_tile4
    int32_t tq;
    uint32_t t_per_chunk, tile4;
    uint32_t sstride[ZHIP_MAX_DIMS];
    const uint32_t* tz;
    const uint32_t* kq4;
    const uint32_t* kq2;  // k_encode_tile4's two-tile form: lane constants [T/2][kThreads] (null: four tiles)
    const struct TileEnt* tmap;
    // k_encode_tile (ZHIP_DF_TILE / ZHIP_DF_TILE_PREFIX, not tile4): one tile
    // per workgroup; horner / kthread / kunit / c_inv are the tile tables then
    uint32_t tile, n_qb, n_cb;
    zhip_fdiv d_qb, d_cb;
    // k_encode_tileg (tile == 2): group map, step multiply table, steps
    const struct GroupEnt* gmap;
    const uint32_t* gtz;
    uint32_t n_groups, g_step_t, n_sub;
    uint32_t g_z2;  // k_encode_tileg's two-tile form: x^(8 * 2 g_step_t), the first half's shift to ku's frame
    // tuning arm 68 (k_encode_tileg, four accumulators through one byte-table
    // operator): the A4 fold tables and x^(-96), the folded state's frame
    const uint32_t* g_a4;
    uint32_t g_c96;
    int64_t g_step_o;
    uint32_t xcd_run;     // k_encode_pair: pairs per XCD-contiguous run (0: dispatch order)
    // 64-bit words between chunks' publication words (k_encode_pair / k_encode_tile4):
    // kPubLine / 2 for CRC layouts (a 128-byte line per chunk), else 2
    uint32_t pub_stride;
    // k_encode_il: k_decode_il's interleave stride, tables and lane constants
    // (0: not available for this plan)
    uint32_t il_S;
    const uint32_t* il_tab;
    const uint32_t* il_klane;
    // ZHIP_DF_WHOLE (k_encode_il's AFF form): DecodeParams' aff_* fields
    uint32_t aff_ok, aff_sh, aff_mask;
    int32_t aff_B, aff_C, aff_D;
};

struct PackParams {
    uint8_t* dst;
    const zhip_shard* shards;
    const uint32_t* nonempty;      // per inner chunk, chunk id = first_chunk + Morton rank
    uint32_t* newrank;             // scratch per inner chunk
    const uint32_t* rank_of_slot;  // C-order slot -> Morton rank
    uint64_t* blob_len;            // out, per shard
    const uint32_t* horner;
    const uint32_t* kthread;
    uint32_t n_inner, elen, index_size, index_start, index_crc, keep_empty;
    uint32_t idx_c_inv, idx_c3;
};

int launch_decode(const DecodeParams& p, hipStream_t stream, int max_grid);
// n independent launches in one grid (k_decode_il_multi); ZHIP_E_UNSUPPORTED,
// with nothing launched, unless each would take the production k_decode_il
// arm and all the same instantiation.  max_grid: per launch, as launch_decode's;
// dry: the admission alone, no launch
int launch_decode_multi(const DecodeParams* ps, const int* max_grid, uint32_t n, hipStream_t stream, bool dry);
extern uint64_t g_launch_count;  // zhip_launch_count: kernel launches issued by fire / launch_decode_multi
int launch_encode(const EncodeParams& p, hipStream_t stream, int max_grid);
int launch_shard_pack(const PackParams& p, uint32_t n_shards, hipStream_t stream);
int launch_dv_check(const zhip_dv_ref* d_refs, uint32_t n_refs, hipStream_t stream);
int debug_stamps(uint64_t* host_out, uint32_t n_wg);

// Kernel selection: (layout flags, item type, form) -> instantiation, nullptr
// where none exists.  Each selector lives beside its kernels; launch_decode /
// launch_encode (decode.hip / encode.hip) call them.
using KernelFn = void (*)(const DecodeParams);
using EncodeFn = void (*)(const EncodeParams);
using MultiFn = void (*)(const MultiParams);

// select_pair_kernel: the two-unit kernel, its tuning forms and the kernels
// of its family (the values past kPairTwo exist in the tuning build only,
// except the lead kernels)
enum PairForm {
    kPairSingle = 1,      // kTuneSingle: one unit per workgroup
    kPairTwo = 2,         // k_decode_pair
    kPairNoLookups = 5,   // kTuneSkipCrc: VARIANT 3
    kPairPrio = 6,        // kTunePrio: VARIANT 6
    kPairDeferB = 7,      // kTuneDeferB: VARIANT 7
    kPairPrioDeferB = 8,  // both: VARIANT 8
    kPairLead = 9,        // k_decode_lead (no data CRC, leading index-check workgroups)
    kPairLead4 = 10,      // k_decode_lead4: chunks of <= 16 KiB, four per workgroup
    kPairLead8 = 11,      // k_decode_lead4<.., 8>: chunks of <= 8 KiB, eight per workgroup
};
// select_ilw_kernel (all but kIlw512 in the tuning build only)
enum IlwForm {
    kIlw512 = 512,          // 512 lanes per unit (production)
    kIlw1024 = 1024,        // 1024 lanes
    kIlw512Half = 513,      // 512 lanes, half the lane multiply in registers (kArmIlw512Half)
    kIlw512Split = 515,     // the split publication (kArmSplitPub; AFF)
    kIlw512LookBack = 516,  // the look-back finalizer (kArmLookBack; AFF)
};
// select_tile2w_kernel (all but kT2wTwo in the tuning build only)
enum Tile2wForm {
    kT2wOne = 1,      // one tile per workgroup (kArmTile1w)
    kT2wTwo = 2,      // two (production)
    kT2wSplit = 3,    // two, the split publication (kArmSplitPub)
    kT2wByteTab = 4,  // two, byte-table chains (kArmTile2wByteTab)
};
// select_tilegw_kernel (past kTgwFour in the tuning build only)
enum TilegwForm {
    kTgwTwo = 2,       // two tiles per workgroup, returning publication on spread lines (production)
    kTgwFour = 4,      // four tiles
    kTgwLanes = 5,     // four tiles, lanes pick the tile (kArmTilegLanes)
    kTgwPacked = 6,    // two tiles, arrival words packed (kArmTilegPacked)
    kTgwLookBack = 7,  // two tiles, the look-back finalizer (kArmTilegLookBack)
    kTgwByteTab = 8,   // two tiles, byte-table chains (kArmTilegByteTab)
};
// select_encode_tileg_kernel (past kEtgFour in the tuning build only)
enum EncTilegForm {
    kEtgTwo = 2,         // two tiles per workgroup (CRC layouts; kArmEncTileg2)
    kEtgFour = 4,        // four (production)
    kEtgFourSpread = 6,  // four, arrival words on lines of their own (kArmEncTilegSpread)
    kEtgTwoSpread = 7,   // two, the same (kArmEncTileg2Spread)
    kEtgLookBack = 8,    // four, the look-back finalizer (kArmEncTilegLookBack)
    kEtgA4 = 9,          // four accumulators through one byte-table operator (kArmEncTilegA4)
};

// decode_rows.hip
KernelFn select_rows_kernel(bool crc, int item, int swap, int k);
KernelFn select_pair_kernel(bool crc, int item, int swap, PairForm form);
KernelFn select_duo_kernel(bool crc, int item, int swap);
KernelFn select_il_kernel(bool crc, int item, int swap, bool aff);
MultiFn select_il_multi_kernel(bool crc, int item, int swap, bool aff);  // k_decode_il_multi, the same forms
KernelFn select_ilx_kernel(bool crc, int item, int swap, bool aff);      // k_decode_il's full-row form (CRC only)
MultiFn select_ilx_multi_kernel(bool crc, int item, int swap, bool aff);
KernelFn select_ilw_kernel(int item, int swap, IlwForm form, bool lmr, bool aff);
KernelFn select_ilh_kernel(int item, int swap, bool lb, bool aff);
#if ZHIP_TUNING
KernelFn select_il_kernel_lean(bool crc, int item, int swap);
KernelFn select_il_kernel_tuned(bool crc, int item, int swap);
KernelFn select_il_kernel_arm(bool crc, int item, int swap, int arm);
KernelFn select_il_kernel_cf(bool crc, int item, int swap);
KernelFn select_il_kernel_regmul(bool crc, int item, int swap, bool occ6);
KernelFn select_xw_kernel(bool crc, int item, int swap);
KernelFn select_ilq_kernel(int item, int swap, int nq, bool glds);
KernelFn select_ilc_kernel(int item, int swap);
KernelFn select_ilp_kernel(int item, int swap);
#endif
// decode_tile.hip
#if ZHIP_TUNING
KernelFn select_tile4f_kernel(int item, int swap);
#endif
KernelFn select_tile4_kernel(bool crc, int item, int swap);
KernelFn select_tile4w_kernel(int item, int swap);
KernelFn select_tile2w_kernel(int item, int swap, Tile2wForm form);
KernelFn select_tilegw_kernel(int item, int swap, bool defer, TilegwForm form);
KernelFn select_tileg_kernel(bool crc, int item, int swap, bool defer);
EncodeFn select_encode_tile4_kernel(bool crc, int item, int swap, bool two);
EncodeFn select_encode_tile_kernel(bool crc, int item, int swap);
EncodeFn select_encode_tileg_kernel(bool crc, int item, int swap, EncTilegForm form);

}  // namespace zhip

struct zhip_plan {
    zhip_layout layout;
    uint32_t kblocks;  // K: blocks per thread per unit (4, 8 or 16)
    uint32_t seg;      // kWgStride * K
    uint32_t nseg;
    uint32_t E;
    uint64_t R;
    uint32_t c_inv, c3;
    uint32_t hx[4];    // x^(8(4096 - 4k)), k = 0..3: the Horner operators
    uint32_t kq[32];   // x^(8(4096 - 256a)), a < 16 | x^(-128b), b < 16 (lane_kthread)
    zhip_fdiv dshape[ZHIP_MAX_DIMS];
    uint32_t row_bytes;
    zhip_fdiv drow;
    uint32_t fill[4];
    // Everything but the next four fields is final after zhip_plan_create;
    // zhip_plan_upload sets these.  The images' regions: tl (DESIGN.md "Plan
    // table images").
    int device;
    int max_grid;
    uint32_t* d_tables;       // the row image
    uint32_t* d_tile_tables;  // the tile image (tq >= 0)
    zhip::TableLayout tl;
    // tile mode (layouts with a transposed dim that is contiguous in out)
    int32_t tq;          // -1: no tile mode
    uint32_t t_per_chunk, n_qb, n_cb;
    uint32_t sstride[ZHIP_MAX_DIMS];
    uint32_t t_c_inv;
    // k_decode_tile4 (full tiles, groups of 4 tiles at a uniform base step)
    uint32_t tile4;
    uint64_t tile4_step;  // base step between consecutive tiles
    uint32_t tile4f;      // k_decode_tile4f (tile step 256 B, CRC)
    uint32_t tile4w;      // k_decode_tile4w (tile4 layouts with a CRC)
    // full-tile layouts that tile4 declines (e.g. 128^3 chunks: the four tiles
    // of a natural group at two steps) but whose consecutive tile pairs are the
    // two column blocks of one row band: k_decode_tile4w<2> over pairs (2 k,
    // 2 k + 1), tuning arm 39
    uint32_t tile2;
    // the whole-chunk row map of a whole-row layout in two-level affine form
    // (plan_affine; ZHIP_DF_WHOLE launches): aff_ok, shift, B, C, D
    uint32_t aff_ok, aff_sh;
    int32_t aff_B, aff_C, aff_D;
    uint32_t tilegw;  // k_decode_tilegw (grouped tile layouts with a CRC)
    // k_encode_tileg (full selections): tiles grouped by four along the
    // innermost other stored dim gd with shape[gd] % 4 == 0 (uniform step
    // sstride[gd] inside every group, whatever the natural tile order)
    int32_t gd;                      // -1: no such dim
    uint32_t n_groups;
    uint32_t n_sub;                  // > 16 groups per chunk: arrival subgroups of 16 (workspace tail)
    // shard index (sharded layouts): payload 16*n_inner, E, CRC constants
    uint32_t idx_nbytes, idx_E, idx_c_inv, idx_c3;
    // k_decode_il (interleaved steps, decode_rows.hip): a workgroup takes K = 8
    // of the chunk's 4 KiB steps at a stride of il_S steps (il_S = 0: not
    // available for this layout)
    uint32_t il_S;
    // k_decode_xw (decode_rows.hip): xw_P = 8 KiB spans per chunk (0: not
    // available), xw_nsub = two-level arrival subwords (P > 32, P <= 1024)
    uint32_t xw_P, xw_nsub;
};
