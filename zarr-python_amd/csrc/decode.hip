// Fused zarr v3 decode for MI355X (gfx950): shard sub-chunk resolution,
// CRC-32C verify, bytes-codec byteswap and scatter into the selection of a
// device-resident N-d output — one read of every encoded byte, one write of
// every selected decoded byte.
//
// Reference behaviour restated (file:line under /root/reference):
//   Crc32cCodec._decode_sync        src/zarr/codecs/crc32c_.py:34-50
//   BytesCodec._decode_sync         src/zarr/codecs/bytes.py:97-131
//   TransposeCodec._decode_sync     src/zarr/codecs/transpose.py:98-104 (folded into
//                                   the stored-dim -> out-stride map by the planner)
//   decode_and_scatter_chunk        src/zarr/core/chunk_utils.py:193-214
//   scatter_chunk (missing -> fill) src/zarr/core/chunk_utils.py:88-112
//   _ShardIndex.get_chunk_slice     src/zarr/codecs/sharding.py:248-254 (MAX_UINT_64 -> missing)
//
// Work decomposition.  A chunk's decoded payload [0, N) is cut into "units" of
// seg = 4 KiB * K (K = 8 by default: 32 KiB), aligned to E = align16(N) from the END
// (unit s covers [E-(s+1)seg, E-s*seg)); bytes outside [0, N) are zero.  One 256-thread
// workgroup handles one unit: thread t owns the 16-byte blocks at
// lo + 16t + 4096k, k < 8 (each wave instruction reads 1 KiB contiguous).
//
// CRC.  Each thread keeps a Horner accumulator positioned at the start of its
// next block: acc' = A4096(acc ^ w0) ^ A4092(w1) ^ A4088(w2) ^ A4084(w3), each
// A_k a 32x32 GF(2) operator applied as 4 byte-indexed lookups in LDS
// (16 KiB of tables, host-built).  At the end thread t's value is shifted by a
// per-thread constant to a common point, xor-reduced over the workgroup,
// shifted to the chunk reference R = E + 4096 by a per-unit constant and
// atomically xor-ed into a per-chunk word.  The last unit of a chunk to arrive
// (agent-scope ticket) converts the accumulator into the CRC-32C value, compares
// it with the stored little-endian trailer and writes the chunk status.  Zero
// bytes before the chunk contribute nothing, so no unit needs to know another's
// data: the combine is pure XOR, order-independent and bitwise reproducible.
#include <hip/hip_runtime.h>

#include "../../include/zarrhip.h"
#include "zhip_gf2.h"
#include "zhip_internal.h"
#include "zhip_dispatch.h"
#include "zhip_device.h"
#include "zhip_decode_common.h"
#include "zhip_arrival.h"

namespace zhip {

#if ZHIP_TUNING
int g_tune_max_grid = 0;
#endif

// Work assignment: unit "positions" q are numbered chunk-major in INCREASING
// address order (q = c*nseg + nseg-1-sidx) and every workgroup takes one
// contiguous, balanced range of them.  Consecutive units of one chunk then
// continue the same per-thread Horner chain (stride 4096 B), so a workgroup
// reduces, shifts and publishes once per (chunk, run), not once per unit.
template <bool CRC, bool WRITE, bool FAST, int ITEM, int SWAP, int K = 8>
__global__ __launch_bounds__(kThreads) void k_decode(const DecodeParams p) {
    __shared__ uint32_t s_tab[CRC ? 16 * 256 : 1];
    __shared__ uint32_t s_red[2][kThreads / 64];
    const int t = threadIdx.x;
    uint32_t kth = 0;
    const bool crc_on = CRC && !(p.tune & kTuneSkipCrc);
    if constexpr (CRC) {
        const uint4* g = reinterpret_cast<const uint4*>(p.horner);
        uint4* sv = reinterpret_cast<uint4*>(s_tab);
        for (int i = t; i < 1024; i += kThreads) sv[i] = g[i];
        kth = p.kthread[t];
    }
    const uint32_t expected = p.g.nbytes + (CRC ? 4u : 0u);
    // the mask form up to 32 units per chunk (zhip_arrival.h)
    const bool one_atomic = p.nseg <= 32 && !(p.tune & (kTuneAcqRel | kTuneNoTicket));
    const uint64_t full = mask_of(p.nseg);
    Pending pend;
    pend.valid = 0;

    const uint32_t G = gridDim.x, g = blockIdx.x;
    const uint32_t per = p.n_units / G, rem = p.n_units % G;
    const uint32_t q0 = g * per + (g < rem ? g : rem);
    const uint32_t q1 = q0 + per + (g < rem ? 1u : 0u);
    if (q0 >= q1 && g >= p.n_idx) return;
    uint4 A[K], B[K];
    auto unit_of = [&](uint32_t q) {
        const uint32_t c = q / p.nseg;
        return c * p.nseg + (p.nseg - 1u - (q - c * p.nseg));
    };
    Unit ua;
    uint32_t stored = 0;
    if (q0 < q1) {
        ua = resolve_unit(p, unit_of(q0), expected);
        load_unit<K>(p, ua, t, A);
        if (CRC && t == 0 && ua.mode == ZHIP_ST_OK) stored = load_trailer(ua.cp, p.g.nbytes);
    }
    if constexpr (CRC) {
        __syncthreads();  // tables in LDS
        // fused shard-index checks (_decode_shard_index_sync, sharding.py:624-631):
        // workgroup g verifies indexes g, g+G, ... while its first unit's loads fly
        for (uint32_t j = g; j < p.n_idx; j += G) verify_index(p, j, t, kth, s_tab, s_red[1]);
    }
    if (q0 >= q1) return;
    uint32_t acc = 0, run_bits = 0, run_len = 0, parity = 0;
    for (uint32_t q = q0;;) {
        // software pipeline: issue the next unit's loads before working on this one
        const uint32_t qn = q + 1;
        const bool more = qn < q1;
        Unit ub;
        if (more) {
            ub = resolve_unit(p, unit_of(qn), expected);
            load_unit<K>(p, ub, t, B);
        }
        const bool run_end = !more || ub.c != ua.c;
        const zhip_sel& sel = p.sels[ua.sel];
        if (ua.mode == ZHIP_ST_OK) {
            // stores first: they do not depend on the CRC, and starting the write
            // stream early interleaves it with the read stream of later units
            if constexpr (WRITE) {
                if (FAST && (p.tune & kTuneNT)) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int32_t o = ua.seg_lo + kWgStride * k + 16 * t;
                        if (o < 0 || (uint32_t)o >= p.g.nbytes) continue;
                        scatter_block_rows<ITEM, SWAP, true>(p.g, p.out, sel, ua.out_off, o, A[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int32_t o = ua.seg_lo + kWgStride * k + 16 * t;
                        if (o < 0 || (uint32_t)o >= p.g.nbytes) continue;
                        if constexpr (FAST) scatter_block_rows<ITEM, SWAP>(p.g, p.out, sel, ua.out_off, o, A[k]);
                        else scatter_block_generic<ITEM, SWAP>(p.g, p.out, sel, ua.out_off, o, A[k]);
                    }
                }
            }
            if (crc_on) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint4 v = A[k];
                    acc = tab_apply(s_tab, acc ^ v.x) ^ tab_apply(s_tab + 1024, v.y) ^
                          tab_apply(s_tab + 2048, v.z) ^ tab_apply(s_tab + 3072, v.w);
                }
            } else if constexpr (CRC) {
#pragma unroll
                for (int k = 0; k < K; ++k) acc ^= A[k].x ^ A[k].y ^ A[k].z ^ A[k].w;
            }
            run_bits |= 1u << (ua.sidx & 31u);
            ++run_len;
            if constexpr (CRC) {
                if (run_end) {
                    uint32_t v = crc_on ? gf_mul(acc, kth) : acc;
                    v = wave_xor(v);
                    if ((t & 63) == 0) s_red[parity][t >> 6] = v;
                    __syncthreads();
                    if (t == 0) {
                        uint32_t V = s_red[parity][0] ^ s_red[parity][1] ^ s_red[parity][2] ^
                                     s_red[parity][3];
                        V = gf_mul(V, p.kunit[ua.sidx]);
                        if (one_atomic) {
                            retire(p, pend, full);  // the previous run's arrival has returned by now
                            uint64_t* w = reinterpret_cast<uint64_t*>(p.ws) + 2ull * ua.c;
                            pend.prev = mask_issue(w, run_bits, V);
                            pend.stored = stored;
                            pend.c = ua.c;
                            pend.bits = run_bits;
                            pend.V = V;
                            pend.valid = 1;
                        } else {
                            // the counted form (arrive_count, zhip_arrival.h) written out: the two
                            // tuning-only forms (an acq_rel ticket in place of the wait; no ticket,
                            // no verdict) share its steps
                            uint32_t* accw = p.ws + 4ull * ua.c;
                            uint32_t tk;
                            if (p.tune & kTuneAcqRel) {
                                __hip_atomic_fetch_xor(accw, V, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                tk = __hip_atomic_fetch_add(accw + 2, run_len, __ATOMIC_ACQ_REL,
                                                            __HIP_MEMORY_SCOPE_AGENT);
                            } else {
                                const uint32_t prev = __hip_atomic_fetch_xor(accw, V, __ATOMIC_RELAXED,
                                                                             __HIP_MEMORY_SCOPE_AGENT);
                                asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");
                                tk = (p.tune & kTuneNoTicket)
                                         ? 0u
                                         : __hip_atomic_fetch_add(accw + 2, run_len, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT);
                            }
                            if (tk + run_len == p.nseg && !(p.tune & kTuneNoTicket)) {
                                const uint32_t raw =
                                    __hip_atomic_exchange(accw, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                __hip_atomic_store(accw + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                finalize_chunk(p, ua.c, stored, raw);
                            }
                        }
                    }
                    parity ^= 1u;
                    acc = 0;
                    run_bits = 0;
                    run_len = 0;
                }
            } else {
                if (ua.sidx == 0 && t == 0) {
                    zhip_status st = {ZHIP_ST_OK, 0u, 0u, 0u};
                    p.status[ua.c] = st;
                }
            }
        } else {
            if constexpr (WRITE) {
                if (ua.mode == ZHIP_ST_MISSING) {
                    const uint4 f = make_uint4(p.fill[0], p.fill[1], p.fill[2], p.fill[3]);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int32_t o = ua.seg_lo + kWgStride * k + 16 * t;
                        if (o < 0 || (uint32_t)o >= p.g.nbytes) continue;
                        if constexpr (FAST) scatter_block_rows<ITEM, false>(p.g, p.out, sel, ua.out_off, o, f);
                        else scatter_block_generic<ITEM, false>(p.g, p.out, sel, ua.out_off, o, f);
                    }
                }
            }
            if (ua.sidx == 0 && t == 0) {
                zhip_status st = {ua.mode, 0u, 0u, 0u};
                p.status[ua.c] = st;
                if (ua.mode != ZHIP_ST_MISSING) atomicOr(p.errflag, 1u << ua.mode);
            }
        }
        if (!more) break;
        if (CRC && t == 0 && ub.c != ua.c && ub.mode == ZHIP_ST_OK) stored = load_trailer(ub.cp, p.g.nbytes);
        q = qn;
        ua = ub;
#pragma unroll
        for (int k = 0; k < K; ++k) A[k] = B[k];
    }
    if (t == 0) retire(p, pend, full);
}


// ---------------------------------------------------------------------------
// Tiled transpose decode (TransposeCodec._decode_sync, transpose.py:98-104, for
// orders whose out-contiguous dim is not the innermost stored dim).  A tile =
// kTileRows rows of the stored dim tq (contiguous in out) x kTileCols bytes of
// the innermost stored row, other dims fixed.  Loads: 16 rows x 256 B per pass
// (every wave reads whole 256-byte row pieces); the tile is transposed through
// LDS and stored as whole out rows (256 B contiguous per column element).
// CRC: thread t's blocks sit at a constant stride 16*sstride[tq], so it keeps
// a Horner chain with stride-specific tables; per-thread / per-tile shift
// constants (host-built) bring every tile's contribution to the chunk reference.
// ---------------------------------------------------------------------------
template <bool CRC, int ITEM, int SWAP>
__global__ __launch_bounds__(kThreads) void k_decode_tile(const DecodeParams p) {
    constexpr int kPitch = ITEM == 8 ? 264 : 260;  // bytes per LDS tile row (2-way read conflicts)
    constexpr int kPasses = kTileRows / 16;
    __shared__ uint32_t s_tab[CRC ? 16 * 256 : 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[kTileRows * kPitch];
    __shared__ uint32_t s_red[kThreads / 64];
    const int t = threadIdx.x;
    uint32_t kth = 0;
    if constexpr (CRC) {
        const uint4* g = reinterpret_cast<const uint4*>(p.horner);
        uint4* sv = reinterpret_cast<uint4*>(s_tab);
        for (int i = t; i < 1024; i += kThreads) sv[i] = g[i];
        kth = p.kthread[t];
        __syncthreads();
    }
    const uint32_t expected = p.g.nbytes + (CRC ? 4u : 0u);
    const int32_t last = p.g.ndim - 1;
    const uint32_t rows_q = (uint32_t)p.g.shape[p.tq];
    const uint32_t sq = p.sstride[p.tq];
    const int64_t oq = p.g.ostride[p.tq];      // == ITEM
    const int64_t ocol = p.g.ostride[last];    // out stride of the innermost stored dim
    const uint32_t G = gridDim.x, gi = blockIdx.x;
    const uint32_t per = p.n_units / G, rem = p.n_units % G;
    const uint32_t q0 = gi * per + (gi < rem ? gi : rem);
    const uint32_t q1 = q0 + per + (gi < rem ? 1u : 0u);
    uint32_t runV = 0, run_len = 0;
    for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t c = q / p.t_per_chunk;
        const uint32_t ti = q - c * p.t_per_chunk;
        // chunk source (resolve_unit's rule over vector loads; a shared helper changes that
        // function's scalar code in every kernel that resolves units)
        const zhip_chunk ch = p.chunks[c];
        uint32_t mode = ZHIP_ST_OK;
        uint64_t base = ch.src;
        if (ch.flags & ZHIP_CF_MISSING) {
            mode = ZHIP_ST_MISSING;
        } else if (p.lflags & ZHIP_LF_SHARDED) {
            const uint64_t ipos = (p.lflags & ZHIP_LF_INDEX_START) ? 0ull : ch.src_len - p.index_size;
            const uint8_t* e = p.src + ch.src + ipos + 16ull * ch.slot;
            const uint64_t off = load_u64_le_bytes(e);
            const uint64_t len = load_u64_le_bytes(e + 8);
            if (off == ~0ull && len == ~0ull) mode = ZHIP_ST_MISSING;
            else if (off > ch.src_len || len > ch.src_len - off) mode = ZHIP_ST_INDEX_OOB;
            else if (len != expected) mode = ZHIP_ST_LENGTH_MISMATCH;
            else base = ch.src + off;
        } else if (ch.src_len != expected) {
            mode = ZHIP_ST_LENGTH_MISMATCH;
        }
        mode = __builtin_amdgcn_readfirstlane(mode);
        const uint8_t* cp = p.src + base;
        // tile coordinates
        uint32_t r = ti;
        const uint32_t rq = fdiv_apply(r, p.d_cb.m, p.d_cb.s);
        const uint32_t cb = r - rq * p.n_cb;
        r = rq;
        const uint32_t rr = fdiv_apply(r, p.d_qb.m, p.d_qb.s);
        const uint32_t qb = r - rr * p.n_qb;
        r = rr;
        uint32_t tbase = qb * (uint32_t)kTileRows * sq + cb * (uint32_t)kTileCols;
        int64_t obase = ch.out_off + (int64_t)qb * kTileRows * oq + (int64_t)(cb * (kTileCols / ITEM)) * ocol;
#pragma unroll
        for (int d = ZHIP_MAX_DIMS - 1; d >= 0; --d) {
            if (d >= last || d == p.tq) continue;
            const uint32_t qd = fdiv_apply(r, p.g.dshape[d].m, p.g.dshape[d].s);
            const uint32_t sd = r - qd * (uint32_t)p.g.shape[d];
            r = qd;
            tbase += sd * p.sstride[d];
            obase += (int64_t)sd * p.g.ostride[d];
        }
        const uint32_t rows_here = min((uint32_t)kTileRows, rows_q - qb * kTileRows);
        const uint32_t cols_here = min((uint32_t)kTileCols, p.g.row_bytes - cb * kTileCols);
        if (mode == ZHIP_ST_OK) {
            const int row0 = t >> 4;
            const uint32_t col = 16u * (uint32_t)(t & 15);
            uint4 blk[kPasses];
            const uint32_t al4 =
                __builtin_amdgcn_readfirstlane((uint32_t)(reinterpret_cast<uintptr_t>(cp) & 3u) == 0u ? 1u : 0u);
            if (al4) {
#pragma unroll
                for (int k = 0; k < kPasses; ++k) {
                    const uint32_t row = 16u * k + row0;
                    blk[k] = (row < rows_here && col < cols_here)
                                 ? *reinterpret_cast<const uint4*>(cp + tbase + row * sq + col)
                                 : make_uint4(0, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int k = 0; k < kPasses; ++k) {
                    const uint32_t row = 16u * k + row0;
                    blk[k] = (row < rows_here && col < cols_here)
                                 ? load_block<false>(cp, (int32_t)(tbase + row * sq + col), p.g.nbytes)
                                 : make_uint4(0, 0, 0, 0);
                }
            }
            uint32_t acc = 0;
            if constexpr (CRC) {
#pragma unroll
                for (int k = 0; k < kPasses; ++k) {
                    const uint4 v = blk[k];
                    acc = tab_apply(s_tab, acc ^ v.x) ^ tab_apply(s_tab + 1024, v.y) ^
                          tab_apply(s_tab + 2048, v.z) ^ tab_apply(s_tab + 3072, v.w);
                }
            }
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const uint4 v = swap_block<ITEM, SWAP>(blk[k]);
                uint32_t* d = reinterpret_cast<uint32_t*>(s_tile + (16 * k + row0) * kPitch + col);
                d[0] = v.x;
                d[1] = v.y;
                d[2] = v.z;
                d[3] = v.w;
            }
            __syncthreads();
            // out pieces: column element j, 16/ITEM consecutive rows from q0
            constexpr int kPer = 16 / ITEM;                  // rows per 16-byte piece
            constexpr int kPiecesPerCol = kTileRows / kPer;  // pieces per out row
#pragma unroll
            for (int k = 0; k < kPasses; ++k) {
                const uint32_t pc = (uint32_t)(k * kThreads + t);
                const uint32_t j = pc / kPiecesPerCol;
                const uint32_t r0 = (pc % kPiecesPerCol) * kPer;
                if (j * ITEM >= cols_here || r0 >= rows_here) continue;
                uint32_t w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = 0;
#pragma unroll
                for (int e = 0; e < kPer; ++e) {
                    const uint8_t* src = s_tile + (r0 + e) * kPitch + j * ITEM;
                    if constexpr (ITEM == 8) {
                        const uint2 v = *reinterpret_cast<const uint2*>(src);
                        w[2 * e] = v.x;
                        w[2 * e + 1] = v.y;
                    } else if constexpr (ITEM == 4) {
                        w[e] = *reinterpret_cast<const uint32_t*>(src);
                    } else if constexpr (ITEM == 2) {
                        w[e / 2] |= (uint32_t)(*reinterpret_cast<const uint16_t*>(src)) << (16 * (e & 1));
                    } else {
                        w[e / 4] |= (uint32_t)(*src) << (8 * (e & 3));
                    }
                }
                uint8_t* dst = p.out + obase + (int64_t)j * ocol + (int64_t)r0 * oq;
                if (r0 + kPer <= rows_here) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
                    for (uint32_t e = 0; e < rows_here - r0; ++e)
                        for (int b = 0; b < ITEM; ++b)
                            dst[e * ITEM + b] = (uint8_t)(w[(e * ITEM + b) / 4] >> (8 * ((e * ITEM + b) % 4)));
                }
            }
            if constexpr (CRC) {
                uint32_t v = gf_mul(acc, kth);
                v = wave_xor(v);
                if ((t & 63) == 0) s_red[t >> 6] = v;
            }
            __syncthreads();  // LDS tile and s_red reads done before the next tile
            if constexpr (CRC) {
                if (t == 0) {
                    const uint32_t V = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
                    runV ^= gf_mul(V, p.kunit[ti]);
                    ++run_len;
                    const bool run_end = (q + 1 >= q1) || ((q + 1) / p.t_per_chunk != c);
                    if (run_end) {
                        arrive_count(p.ws + 4ull * c, runV, run_len, p.t_per_chunk, [&](uint32_t raw) {
                            finalize_chunk(p, c, load_trailer(cp, p.g.nbytes), raw);
                        });
                        runV = 0;
                        run_len = 0;
                    }
                }
            } else if (t == 0 && ti == 0) {
                zhip_status st = {ZHIP_ST_OK, 0u, 0u, 0u};
                p.status[c] = st;
            }
        } else {
            // missing chunk: fill this tile's region of out
            const uint4 f = make_uint4(p.fill[0], p.fill[1], p.fill[2], p.fill[3]);
            constexpr int kPer = 16 / ITEM;
            constexpr int kPiecesPerCol = kTileRows / kPer;
            if (mode == ZHIP_ST_MISSING) {
#pragma unroll
                for (int k = 0; k < kPasses; ++k) {
                    const uint32_t pc = (uint32_t)(k * kThreads + t);
                    const uint32_t j = pc / kPiecesPerCol;
                    const uint32_t r0 = (pc % kPiecesPerCol) * kPer;
                    if (j * ITEM >= cols_here || r0 >= rows_here) continue;
                    uint8_t* dst = p.out + obase + (int64_t)j * ocol + (int64_t)r0 * oq;
                    if (r0 + kPer <= rows_here) {
                        *reinterpret_cast<uint4*>(dst) = f;
                    } else {
                        const uint32_t fw[4] = {f.x, f.y, f.z, f.w};
                        for (uint32_t e = 0; e < (rows_here - r0) * ITEM; ++e)
                            dst[e] = (uint8_t)(fw[e / 4] >> (8 * (e % 4)));
                    }
                }
            }
            if (t == 0 && ti == 0) {
                zhip_status st = {mode, 0u, 0u, 0u};
                p.status[c] = st;
                if (mode != ZHIP_ST_MISSING) atomicOr(p.errflag, 1u << mode);
            }
        }
    }
}

template <bool CRC, bool WRITE, bool FAST, int K>
static KernelFn pick_item(int item, int swap) {
    return for_item(item, swap, [](auto t) -> KernelFn {
        return k_decode<CRC, WRITE, FAST, decltype(t)::item, decltype(t)::swap, K>;
    });
}

KernelFn select_decode_kernel(bool crc, bool write, bool fast, int item, int swap, int k) {
    if (!write) {
        if (!crc) return nullptr;
        return k == 4 ? k_decode<true, false, false, 1, false, 4>
             : k == 16 ? k_decode<true, false, false, 1, false, 16> : k_decode<true, false, false, 1, false, 8>;
    }
    if (crc && fast) {
        return k == 4 ? pick_item<true, true, true, 4>(item, swap)
             : k == 16 ? pick_item<true, true, true, 16>(item, swap) : pick_item<true, true, true, 8>(item, swap);
    }
    if (k != 8) return nullptr;
    if (crc) return pick_item<true, true, false, 8>(item, swap);
    return fast ? pick_item<false, true, true, 8>(item, swap) : pick_item<false, true, false, 8>(item, swap);
}

static KernelFn select_tile_kernel(bool crc, int item, int swap) {
    return for_item(item, swap, [&](auto t) -> KernelFn {
        using T = decltype(t);
        return crc ? k_decode_tile<true, T::item, T::swap> : k_decode_tile<false, T::item, T::swap>;
    });
}

// name of the kernel the last launch_decode chose (zhip_last_kernel: bench
// labels and tests; the selection depends on layout, plan and tuning bits)
const char* g_last_kernel = "";
uint32_t g_last_grid = 0;
#if ZHIP_TUNING
// Overhead probes (arms 28-30; results invalid): the launch of a decode-shaped
// grid with the decode's kernel arguments and nothing else (28), plus the
// k_decode_il LDS footprint (29), plus the header chain (resolve_unit) of
// each workgroup's chunk (30).
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_probe(const DecodeParams p) {
    __shared__ uint32_t s_big[MODE >= 1 ? 9216 : 1];
    const uint32_t g = blockIdx.x;
    const int t = threadIdx.x;
    uint32_t v = g;
    if constexpr (MODE >= 1) {
        s_big[(t * 37u + g) % 9216u] = g;
        __syncthreads();
        v ^= s_big[(t * 41u) % 9216u];
    }
    if constexpr (MODE == 2) {
        const uint32_t c = g / p.nseg;
        if (c < p.n_chunks) {
            const Unit U = resolve_unit(p, c * p.nseg, p.g.nbytes + 4u);
            v ^= (uint32_t)U.out_off ^ (uint32_t)(uintptr_t)U.cp ^ U.mode;
        }
    }
    if (v == 0xFFFFFFFFu && t == 1000) p.errflag[0] = v;  // never: keeps the work live
}
#endif


// One launch_decode call: the parameters, where and how wide to launch, and
// what every layout function reads of them.
struct Launch {
    const DecodeParams& p;
    hipStream_t stream;
    int max_grid;    // CUs * 8 (or ZHIP_TUNE_MAX_GRID)
    uint32_t tune;   // the ablation bits: a compile-time 0 outside the tuning build
    // the look-back finalizer (publish_lb) waits only while fewer chunks than
    // CUs are in the launch
    bool lb_ok;
    bool crc;
    int swap;  // item_mode(): ZHIP_LF_SWAP | 2 * ZHIP_LF_COMPLEX
    int item;
};

// one workgroup per unit, or the fused index checks if there are more of them
static uint32_t unit_grid(const DecodeParams& p, uint32_t units) { return units > p.n_idx ? units : p.n_idx; }

// chunks of <= 16 KiB (sharded or not, with a CRC or not): four per
// workgroup over their live steps, after the leading index-check
// workgroups if any (k_decode_lead4; arm 11 keeps the pair kernels)
// (chunks of 4-8 KiB: eight per workgroup over their last two steps;
// graph-timed on the example array unsharded, profiles/r04/lead8/:
// 8 KiB chunks 25.3-25.6 us vs 37.1 with four per workgroup and 30.8
// with the pair kernel; 4 KiB chunks 37.2 with four, 52.4 with eight,
// 41.4 with the pair kernel.  Arms 12 / 13 force four / eight.)
// (k_decode_lead8 covers at most two steps: arm 13 cannot force it
// onto chunks of more than 8 KiB)
static int launch_lead4(const Launch& L) {
    const DecodeParams& p = L.p;
    const bool e8 = p.E <= 2u * kWgStride &&
                    (g_tune_arm == kArmLead8 || (g_tune_arm != kArmLead4 && p.E > (uint32_t)kWgStride));
    KernelFn fn = select_pair_kernel(L.crc, L.item, L.swap, e8 ? kPairLead8 : kPairLead4);
    const uint32_t per = e8 ? 8u : 4u;
    const uint32_t quads = (uint32_t)(((uint64_t)p.n_units + per - 1u) / per);
    const uint32_t lead = (p.n_idx + 7u) & ~7u;
    if ((uint64_t)quads + lead > 0x7FFFFFFFull) return ZHIP_E_UNSUPPORTED;
    return fire(fn, e8 ? "k_decode_lead8" : "k_decode_lead4", quads + lead, kThreads, p, L.stream);
}

// k_decode_pair's XCD-contiguous runs: one resident wave of workgroups (4 per
// CU; max_grid = 8 per CU), the workgroups of one XCD on a contiguous eighth
// of the batch
static DecodeParams with_xcd_runs(const Launch& L, uint32_t pairs, bool on) {
    DecodeParams q = L.p;
    q.xcd_run = (on && !(L.tune & kTuneNoXcd) && pairs % 8u == 0u && pairs <= (uint32_t)(L.max_grid / 8) * 4u)
                    ? pairs / 8u : 0u;
    q.h.xcd_run = q.xcd_run;
    q.h.d_xcd = make_fdiv(q.xcd_run ? q.xcd_run : 1u);
    return q;
}

// inner chunks without a CRC, shard indexes with one (zarr's default
// sharding codecs): leading index-check workgroups, then the pairs
// (k_decode_lead); > 32 units per chunk is not fused
static int launch_lead(const Launch& L) {
    const DecodeParams& p = L.p;
    if (p.nseg > 32u) return ZHIP_E_UNSUPPORTED;
    KernelFn fn = select_pair_kernel(false, L.item, L.swap, kPairLead);
    const uint32_t pairs = (uint32_t)(((uint64_t)p.n_units + 1u) / 2u);
    const uint32_t lead = (p.n_idx + 7u) & ~7u;
    if ((uint64_t)pairs + lead > 0x7FFFFFFFull) return ZHIP_E_UNSUPPORTED;
    return fire(fn, "k_decode_lead", pairs + lead, kThreads, with_xcd_runs(L, pairs, true), L.stream);
}

#if ZHIP_TUNING
// The measurement arms of the whole-row layouts that launch a kernel of their
// own (il: production would take an interleaved kernel).  True: the arm took
// the launch, rc is its result.
static bool launch_row_arm(const Launch& L, bool il, int& rc) {
    const DecodeParams& p = L.p;
    const uint32_t tune = L.tune;
    const uint32_t units = unit_grid(p, p.n_units);
    if (p.xw != 0 && L.crc && (tune & kTuneXw) &&
        !(tune & (kTuneNoXw | kTuneSkipCrc | kTuneSingle | kTuneDuo | kTuneIl))) {
        const uint64_t xg = (uint64_t)((p.n_chunks + 3u) / 4u) * p.xw;
        const uint64_t grid = xg > p.n_idx ? xg : p.n_idx;
        rc = grid > 0x7FFFFFFFull ? ZHIP_E_UNSUPPORTED
                                  : fire(select_xw_kernel(L.crc, L.item, L.swap), "k_decode_xw", (uint32_t)grid,
                                         kThreads, p, L.stream);
        return true;
    }
    if (arm_in(kArmProbeArgs, kArmProbeHeader)) {  // overhead probes
        KernelFn pf = g_tune_arm == kArmProbeArgs ? k_probe<0> : g_tune_arm == kArmProbeLds ? k_probe<1> : k_probe<2>;
        rc = fire(pf, g_tune_arm == kArmProbeArgs ? "k_probe_args"
                      : g_tune_arm == kArmProbeLds ? "k_probe_lds" : "k_probe_header",
                  units, kThreads, p, L.stream);
        return true;
    }
    if (L.crc && p.ilw_nt && (g_tune_arm == kArmIlw1024 || g_tune_arm == kArmIlw512 || g_tune_arm == kArmIlw1024Reg ||
                              g_tune_arm == kArmIlw512Reg || g_tune_arm == kArmIlw512Half)) {
        // k_decode_ilw: one 32 KiB unit per workgroup of 1024 / 512 lanes
        // (31 / 32: the lane multiply in registers; 42: half in registers)
        const bool half = g_tune_arm == kArmIlw512Half;
        const bool reg = g_tune_arm == kArmIlw1024Reg || g_tune_arm == kArmIlw512Reg;
        KernelFn fn = half ? select_ilw_kernel(L.item, L.swap, kIlw512Half, false, false)
                           : select_ilw_kernel(L.item, L.swap, p.ilw_nt == 1024u ? kIlw1024 : kIlw512, reg, p.aff_ok != 0);
        rc = fire(fn, half ? "k_decode_ilw512m"
                      : p.ilw_nt == 1024u ? (reg ? "k_decode_ilw1024r" : "k_decode_ilw1024")
                                          : (reg ? "k_decode_ilw512r" : "k_decode_ilw512"),
                  units, p.ilw_nt, p, L.stream);
        return true;
    }
    if (!il) return false;
    if ((g_tune_arm == kArmIlh || g_tune_arm == kArmIlhLookBack) && p.ilh_klane) {  // k_decode_ilh: 16 KiB per workgroup
        // (59: with the look-back finalizer, at most 64 half units per chunk)
        KernelFn fn = select_ilh_kernel(L.item, L.swap, g_tune_arm == kArmIlhLookBack && L.lb_ok && p.nseg <= 32u, false);
        rc = fire(fn, "k_decode_ilh", unit_grid(p, 2u * p.n_units), kThreads, p, L.stream);
        return true;
    }
    if (g_tune_arm == kArmIlp && p.pred) {  // k_decode_ilp: index entry off the stores' path
        rc = fire(select_ilp_kernel(L.item, L.swap), "k_decode_ilp", units, kThreads, p, L.stream);
        return true;
    }
    if (g_tune_arm == kArmIlc) {  // k_decode_ilc: tables built in LDS, predicted loads first
        rc = fire(select_ilc_kernel(L.item, L.swap), "k_decode_ilc", units, kThreads, p, L.stream);
        return true;
    }
    if (arm_in(kArmIlq2, kArmIlq4Glds)) {
        // k_decode_ilq arms: NQ units per workgroup, tables by registers or LDS-DMA
        static const char* names[] = {"k_decode_ilq2", "k_decode_ilq4", "k_decode_ilq1_glds",
                                      "k_decode_ilq2_glds", "k_decode_ilq4_glds"};
        const int a = g_tune_arm - kArmIlq2;
        const int nq = (a == 0 || a == 3) ? 2 : (a == 1 || a == 4) ? 4 : 1;
        const uint32_t ug = (uint32_t)(((uint64_t)p.n_units + nq - 1u) / nq);
        const uint32_t xg = (p.n_idx + (uint32_t)nq - 1u) / (uint32_t)nq;
        rc = p.nseg % (uint32_t)nq ? ZHIP_E_UNSUPPORTED
                                   : fire(select_ilq_kernel(L.item, L.swap, nq, a >= 2), names[a], ug > xg ? ug : xg,
                                          nq * kThreads, p, L.stream);
        return true;
    }
    return false;
}
#endif

#if ZHIP_TUNING
// Arms 64 / 65 store through a buffer resource of 0x7FFFFFF0 records based at
// the chunk's out position, at the 32-bit offset rel + lane_off: a 16-byte
// store that starts before record 0 or ends past the last is dropped by the
// hardware.  zhip_rows_map admits rel up to INT32_MAX and lane_off adds up to
// a step of rows, so the arm is taken only while every store of the plan's
// affine form fits the resource; otherwise the launch keeps the production
// instantiation.  A chunk whose selection record is not whole (a C caller's
// partial selection under ZHIP_DF_WHOLE) takes its rel from the row map
// instead: for a lane that writes, rel + lane_off is then the whole chunk's
// offset of the same element less the selection's start, so with
// non-negative out strides it lies between 0 and the bound checked here;
// with a negative stride nothing bounds it and the arm is declined.
static bool il_buffer_stores_fit(const DecodeParams& p) {
    const int64_t rps = (int64_t)kWgStride >> p.row_shift;
    const int64_t lane_hi = (rps - 1) * p.r_oy + ((int64_t)1 << p.row_shift) - 16;  // the last lane's lane_off
    const int64_t lane_lo = std::min<int64_t>((rps - 1) * p.r_oy, 0);
    const uint32_t n_st = p.nseg * (uint32_t)kDefaultBlocks;
    if (p.r_oy < 0 || p.aff_B < 0 || p.aff_C < 0) return false;
    for (uint32_t st = 0; st < n_st; ++st) {
        const int64_t rel = (int64_t)(st >> p.aff_sh) * p.aff_B + (int64_t)(st & p.aff_mask) * p.aff_C + p.aff_D;
        if (rel + lane_lo < 0 || rel + std::max(lane_hi, lane_lo) + 16 > 0x7FFFFFF0ll) return false;
    }
    return true;
}
#endif

// k_decode_il's instantiation: production, or in the tuning build the arm's
// (nullptr where the arm has none for this item type)
static KernelFn pick_il_kernel(const Launch& L) {
#if ZHIP_TUNING
    const DecodeParams& p = L.p;
    const uint32_t tune = L.tune;
    if ((g_tune_arm == kArmIlStoreWt || g_tune_arm == kArmIlStoreNt) && p.aff_ok && !il_buffer_stores_fit(p))
        return select_il_kernel(L.crc, L.item, L.swap, true);
    // (arms 1 / 2 are k_decode_il's own; every other arm keeps production here)
    // (58: the look-back finalizer, while fewer chunks than CUs)
    if (g_tune_arm == kArmPub16 || g_tune_arm == kArmDeferred ||
        ((g_tune_arm == kArmSplitPub || arm_in(kArmIlPrioRunEnd, kArmIlXcd) ||
          (g_tune_arm == kArmLookBack && L.lb_ok && p.nseg <= 32u) ||
          g_tune_arm == kArmIlStoreWt || g_tune_arm == kArmIlStoreNt) && p.aff_ok))
        return select_il_kernel_arm(L.crc, L.item, L.swap, g_tune_arm);
    if (tune & kTuneCfLookup) return select_il_kernel_cf(L.crc, L.item, L.swap);
    if (tune & kTuneIlLean) return select_il_kernel_lean(L.crc, L.item, L.swap);
    if (tune & (kTuneIlRegMul | kTuneIlOcc6))
        return select_il_kernel_regmul(L.crc, L.item, L.swap, (tune & kTuneIlOcc6) != 0);
    if (tune & (kTuneNoTables | kTuneNoRunEnd | kTuneNoPub | kTuneStamp))
        return select_il_kernel_tuned(L.crc, L.item, L.swap);
#endif
    return select_il_kernel(L.crc, L.item, L.swap, L.p.aff_ok != 0);
}

// k_decode_pair's instantiation for nu units per workgroup: production, or
// in the tuning build the variant the ablation bits ask for where it exists
static KernelFn pick_pair_kernel(const Launch& L, int nu) {
#if ZHIP_TUNING
    const uint32_t tune = L.tune;
    // (kTuneTrailingCrc / kTuneSplitChain are read by the production kernel itself)
    if (nu == 2 && !(tune & (kTuneTrailingCrc | kTuneSplitChain))) {
        KernelFn fn = (tune & kTuneSkipCrc) ? select_pair_kernel(L.crc, L.item, L.swap, kPairNoLookups)
                      : (tune & (kTunePrio | kTuneDeferB))
                          ? select_pair_kernel(L.crc, L.item, L.swap,
                                               (tune & kTunePrio) && (tune & kTuneDeferB) ? kPairPrioDeferB
                                               : (tune & kTunePrio) ? kPairPrio : kPairDeferB)
                          : nullptr;
        if (fn) return fn;
    }
#endif
    return select_pair_kernel(L.crc, L.item, L.swap, nu == 2 ? kPairTwo : kPairSingle);
}

// The production rule of the whole-row layouts, arm by arm (launch_row_units
// reads them top to bottom; launch_decode_multi admits only the last).
// lead4 / lead8: chunks of one unit of at most 16 KiB
static bool takes_lead4(const Launch& L) {
    return L.p.nseg == 1u && L.p.E <= 4u * kWgStride && g_tune_arm != kArmNoLead4;
}

// lead: inner chunks without a CRC under checked shard indexes
static bool takes_lead(const Launch& L) { return !L.crc && L.p.n_idx; }

// chunks of a multiple of 8 x 32 KiB: interleaved steps in groups of
// eight workgroups (k_decode_il, see decode_rows.hip) -- graph-timed
// 26.4 vs 27.8 us on the headline; groups of four lose to the pair
// kernel at C4 (profiles/r03/il/).  kTuneIl / kTuneNoIl force.
static bool takes_interleaved(const Launch& L) {
    const DecodeParams& p = L.p;
    return p.il_S != 0 && L.crc && !(L.tune & (kTuneNoIl | kTuneSkipCrc | kTuneSingle | kTuneDuo)) &&
           ((L.tune & kTuneIl) || p.il_S >= 8u);
}

// grids of at most kIlwMaxUnits units (2 per CU: the N = 4 / 8 shares of
// the strong-scaled headline) with fewer chunks than CUs: half units of
// 16 KiB (k_decode_ilh, two workgroups per unit) publishing through the
// look-back finalizer -- graph-timed 8.39 vs 9.77 us (k_decode_ilw512)
// at the N = 8 share, 10.73 vs 11.03 at N = 4 (profiles/r06/a/).
// (Tuning build: arm 0 only; arm 58 / 49 keep k_decode_ilw512.)
static bool takes_ilh(const Launch& L, bool il) {
    const DecodeParams& p = L.p;
    return il && p.ilh_klane && p.n_units <= kIlwMaxUnits && L.lb_ok && p.nseg <= 32u &&
           (g_tune_arm == kArmProduction || g_tune_arm == kArmIlhProduction) && (L.tune & ~kTuneStamp) == 0;
}

// otherwise 512 lanes per unit, four blocks per lane (k_decode_ilw,
// decode_rows.hip) -- graph-timed 8.8 vs 9.4 us at the N = 8 share, 10.3
// vs 11.0 at N = 4; 14.6 vs 16.5 for k_decode_il at N = 2
// (profiles/r05/f/).  (Tuning build: any arm keeps k_decode_il.)
static bool takes_ilw512(const Launch& L, bool il) {
    const DecodeParams& p = L.p;
    return il && p.ilw_nt == 512u && p.n_units <= kIlwMaxUnits &&
           (g_tune_arm == kArmProduction || g_tune_arm == kArmRowMap || g_tune_arm == kArmIlw512Small ||
            ((g_tune_arm == kArmSplitPub || g_tune_arm == kArmLookBack) && p.aff_ok)) &&
           (L.tune & ~kTuneStamp) == 0;
}

// Fused launches (launch_decode_multi) whose every member is a k_decode_il
// launch of more than kIlwMaxUnits units and whole groups of four chunks, on
// plans with the xw tables, take the full-row form (wave
// w of a workgroup on chunk 4 G + w, decode_rows.hip ilx_body), at most 32
// workgroups per group (the mask form of the publication).  Chunks of a
// group need not be neighbours in the out or whole reads: each wave stores
// through its own chunk's row map (or the affine form, checked per chunk).
// (Tuning build: any arm or tuning bit, kTuneNoXw for the A/B, keeps the
// interleaved form.)
static bool takes_fullrow(const Launch& L, bool il) {
    const DecodeParams& p = L.p;
    return il && L.crc && p.xw != 0 && p.xw % kIlxSpans == 0u && p.xw / kIlxSpans <= 32u &&
           p.n_units > kIlwMaxUnits && p.n_chunks % 4u == 0u && g_tune_arm == kArmProduction && L.tune == 0u;
}

// its grid: one workgroup per kIlxSpans spans of a group of four chunks, or
// the fused index checks if there are more of them
static uint64_t fullrow_grid(const DecodeParams& p) {
    const uint64_t g = (uint64_t)(p.n_chunks / 4u) * (p.xw / kIlxSpans);
    return g > p.n_idx ? g : p.n_idx;
}

// Whole-row layouts with a row map, 32 KiB units: one workgroup per unit,
// half unit or pair of units, non-persistent.  The production rule reads top
// to bottom: lead4 / lead8, lead, ilh, ilw512, il (full-row, else
// interleaved), duo, pair.
static int launch_row_units(const Launch& L) {
    const DecodeParams& p = L.p;
    const uint32_t tune = L.tune;
    const bool crc = L.crc;
    if (takes_lead4(L)) return launch_lead4(L);
    if (takes_lead(L)) return launch_lead(L);
    const bool il = takes_interleaved(L);
#if ZHIP_TUNING
    int rc;
    if (launch_row_arm(L, il, rc)) return rc;
#endif
    if (takes_ilh(L, il))
        return fire(select_ilh_kernel(L.item, L.swap, true, p.aff_ok != 0), "k_decode_ilh",
                    unit_grid(p, 2u * p.n_units), kThreads, p, L.stream);
    if (takes_ilw512(L, il)) {
        // (tuning arms, whole-chunk reads: 49 the split publication, 58 the
        // look-back finalizer)
        const IlwForm form = g_tune_arm == kArmSplitPub ? kIlw512Split
                             : (g_tune_arm == kArmLookBack && L.lb_ok && p.nseg <= 64u) ? kIlw512LookBack : kIlw512;
        return fire(select_ilw_kernel(L.item, L.swap, form, false, p.aff_ok != 0), "k_decode_ilw512",
                    unit_grid(p, p.n_units), 512, p, L.stream);
    }
    // (the full-row form, takes_fullrow, is taken by fused launches only: alone, the headline's 512 workgroups
    // are half a residency round and graph-time 27.7 us against 25.9 interleaved, profiles/r10/)
    if (il) return fire(pick_il_kernel(L), "k_decode_il", unit_grid(p, p.n_units), kThreads, p, L.stream);
    // one workgroup per pair of units (k_decode_pair)
    const int nu = (tune & kTuneSingle) ? 1 : 2;
    KernelFn fn = pick_pair_kernel(L, nu);
    if (!fn) return ZHIP_E_UNSUPPORTED;
    // chunks of more than 32 units (> 1 MiB): one unit per 256-thread half of
    // a 512-thread workgroup (k_decode_duo; C1 0.55 -> 0.62 of HBM peak,
    // profiles/r02/kernel_arms_ab.jsonl); kTuneDuo forces it
    if ((tune & kTuneDuo) || (p.nseg > 32 && !(tune & (kTuneSingle | kTuneSkipCrc))))
        return fire(select_duo_kernel(crc, L.item, L.swap), "k_decode_duo",
                    unit_grid(p, (uint32_t)(((uint64_t)p.n_units + 1u) / 2u)), 2 * kThreads, p, L.stream);
    const uint32_t grid = unit_grid(p, (uint32_t)(((uint64_t)p.n_units + nu - 1u) / nu));
    return fire(fn, "k_decode_pair", grid, kThreads, with_xcd_runs(L, grid, nu == 2), L.stream);
}

// The persistent kernels (k_decode_rows, k_decode_tile, k_decode): a resident
// grid of workgroups, each over a balanced range of the units (software-
// pipelined per workgroup); a launch without units does nothing
static int launch_persistent(const Launch& L, KernelFn fn, const char* name) {
    uint32_t grid = L.p.n_units;
    if (fn && grid) {
        const uint32_t resident = (uint32_t)resident_grid(fn, L.max_grid);
        if (grid > resident) grid = resident;
    }
    return fire(fn, name, grid, kThreads, L.p, L.stream);
}

// four tiles per workgroup, non-persistent (k_decode_tile4, decode_tile.hip)
// (arm kTuneTile4F: one A_64 chain per thread when the layout's tile step is
// 256 B, k_decode_tile4f -- exact, measured 0.3-0.4 us slower on C3)
static int launch_tile4(const Launch& L) {
    const DecodeParams& p = L.p;
    const bool f4 = ZHIP_TUNING && p.t4f_tab != nullptr && L.crc;
    const bool w4 = !f4 && p.t4w_tab != nullptr && L.crc;
    // two tiles per workgroup (2 048 workgroups on C3: two residency rounds
    // instead of one) -- graph-timed 27.8-27.9 vs 28.4-30.0 us on C3
    // (profiles/r05/l/); tuning arm 38 keeps four, 37 takes one (46 us)
    if (w4 && ((p.t2w_kq && g_tune_arm != kArmTileFour && g_tune_arm != kArmTile1w) ||
               (g_tune_arm == kArmTile1w && p.t1w_kq))) {
        const bool one = g_tune_arm == kArmTile1w;
        // (tuning arm 49: the split publication of 17..32 workgroups per chunk)
        // (tuning arm 67: the byte-table chains, where the plan built them)
        const Tile2wForm form = one ? kT2wOne : g_tune_arm == kArmSplitPub ? kT2wSplit
                                : (g_tune_arm == kArmTile2wByteTab && p.tbt_tab) ? kT2wByteTab : kT2wTwo;
        DecodeParams q = p;
        q.t4w_kq = one ? p.t1w_kq : p.t2w_kq;
        return fire(select_tile2w_kernel(L.item, L.swap, form),
                    one ? "k_decode_tile1w" : form == kT2wSplit ? "k_decode_tile2ws"
                    : form == kT2wByteTab ? "k_decode_tile2w_bt" : "k_decode_tile2w",
                    p.n_units / (one ? 1u : 2u), kThreads, q, L.stream);
    }
#if ZHIP_TUNING
    if (f4) return fire(select_tile4f_kernel(L.item, L.swap), "k_decode_tile4f", p.n_units / 4u, kThreads, p, L.stream);
#endif
    return fire(w4 ? select_tile4w_kernel(L.item, L.swap) : select_tile4_kernel(L.crc, L.item, L.swap),
                w4 ? "k_decode_tile4w" : "k_decode_tile4", p.n_units / 4u, kThreads, p, L.stream);
}

// consecutive tile pairs (k_decode_tile4w<2>, decode_tile.hip): 128^3
// chunks' two 256-byte column blocks of one row band per workgroup
static int launch_tile_pairs(const Launch& L) {
    const DecodeParams& p = L.p;
    if (p.n_units / 2u >= (1u << 31)) return ZHIP_E_UNSUPPORTED;
    return fire(select_tile2w_kernel(L.item, L.swap, kT2wTwo), "k_decode_tilep", p.n_units / 2u, kThreads, p, L.stream);
}

// tiles grouped by four along a stored dim (k_decode_tileg, decode_tile.hip)
// (k_decode_tilegw when the plan's wave-per-tile chains are selected)
static int launch_tile_groups(const Launch& L) {
    const DecodeParams& p = L.p;
    const bool gw = p.t4w_tab != nullptr && L.crc;
    // (arm 2: the returning publication whatever the flags)
    const bool defer = p.defer != 0 && g_tune_arm != kArmDeferred;
    // two tiles per workgroup where the plan built their constants (as
    // k_decode_tile4w); tuning arms 38 (deferred) / 2 (returning) keep four
    TilegwForm form = (gw && p.t2w_kq && g_tune_arm != kArmTileFour && g_tune_arm != kArmDeferred &&
                       g_tune_arm != kArmTilegLanes) ? kTgwTwo : kTgwFour;
    const bool two = form == kTgwTwo;
#if ZHIP_TUNING
    if (gw && g_tune_arm == kArmTilegLanes && p.tglt_kq) form = kTgwLanes;  // four tiles, lanes pick the tile
    if (two && g_tune_arm == kArmTilegPacked) form = kTgwPacked;  // the arrival words packed (round-4 layout)
    // the look-back finalizer (fewer chunks than CUs; the spread subwords)
    if (two && g_tune_arm == kArmTilegLookBack && L.lb_ok && p.n_groups <= 128u) form = kTgwLookBack;
    if (two && g_tune_arm == kArmTilegByteTab && p.tbt_tab) form = kTgwByteTab;  // the byte-table chains
#endif
    KernelFn fn = gw ? select_tilegw_kernel(L.item, L.swap, defer, form)
                     : select_tileg_kernel(L.crc, L.item, L.swap, defer);
    const uint64_t grid = (uint64_t)p.n_chunks * p.n_groups * (two ? 2u : 1u);
    if (grid >= (1ull << 31)) return ZHIP_E_UNSUPPORTED;
    DecodeParams q = p;
    if (two) q.t4w_kq = p.t2w_kq;
    if (form == kTgwLanes) q.t4w_kq = p.tglt_kq;
    return fire(fn, !gw ? "k_decode_tileg" : form == kTgwPacked ? "k_decode_tileg2wp"
                    : form == kTgwLookBack ? "k_decode_tileg2w_lb" : form == kTgwByteTab ? "k_decode_tileg2w_bt"
                    : two ? "k_decode_tileg2w" : form == kTgwLanes ? "k_decode_tileglt" : "k_decode_tilegw",
                (uint32_t)grid, kThreads, q, L.stream);
}

// The kernel of a launch, by layout: whole-row units, persistent rows, the
// tile kernels of transposed layouts (tile4, tile pairs, grouped tiles,
// persistent tile), else the generic persistent k_decode.
static Launch make_launch(const DecodeParams& p, hipStream_t stream, int max_grid) {
    const bool crc = (p.lflags & ZHIP_LF_CRC) != 0;
    const bool lb_ok = p.n_chunks < (uint32_t)(max_grid / 8);  // max_grid arrives as CUs * 8
    if (g_tune_max_grid > 0) max_grid = g_tune_max_grid;
    return {p, stream, max_grid, ZHIP_TUNING ? p.tune : 0u, lb_ok, crc, item_mode(p.lflags, (int)p.g.itemsize),
            p.g.itemsize};
}

static bool takes_row_units(const Launch& L) {
    const DecodeParams& p = L.p;
    // (the kTunePersist arm never applies to a launch carrying fused index
    // checks of CRC-free inner chunks: only k_decode_lead carries those)
    const bool lead_launch = !L.crc && p.n_idx != 0;
    return p.rows && p.rowmap && p.seg == (uint32_t)kWgStride * kDefaultBlocks &&
           (!(L.tune & kTunePersist) || lead_launch);
}

// launch_decode would fire the production k_decode_il for L: the row-unit
// rule down to its `il` arm (tuning build: the production arm, no ablation bit)
static bool takes_plain_il(const Launch& L) {
    if (!takes_row_units(L) || takes_lead4(L) || takes_lead(L)) return false;
    const bool il = takes_interleaved(L);
    if (!il || takes_ilh(L, il) || takes_ilw512(L, il)) return false;
    return g_tune_arm == kArmProduction && L.tune == 0u;
}

uint64_t g_launch_count = 0;

int launch_decode_multi(const DecodeParams* ps, const int* max_grid, uint32_t n, hipStream_t stream, bool dry) {
    if (n < 2u || n > (uint32_t)ZHIP_MULTI_MAX) return ZHIP_E_UNSUPPORTED;
    MultiParams m{};
    MultiFn fn = nullptr;
    uint64_t total = 0;
    // the full-row form when every launch alone would take it; a mixed grid
    // keeps the interleaved form, which serves them all
    bool fr = true;
    for (uint32_t i = 0; i < n; ++i) {
        const Launch L = make_launch(ps[i], stream, max_grid[i]);
        if (!takes_plain_il(L)) return ZHIP_E_UNSUPPORTED;
        fr = fr && takes_fullrow(L, true);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const Launch L = make_launch(ps[i], stream, max_grid[i]);
        MultiFn f = fr ? select_ilx_multi_kernel(L.crc, L.item, L.swap, ps[i].aff_ok != 0)
                       : select_il_multi_kernel(L.crc, L.item, L.swap, ps[i].aff_ok != 0);
        if (!f || (i && f != fn)) return ZHIP_E_UNSUPPORTED;  // one instantiation for the whole grid
        fn = f;
        const uint32_t grid = fr ? (uint32_t)fullrow_grid(ps[i]) : unit_grid(ps[i], ps[i].n_units);
        if (grid == 0) return ZHIP_E_UNSUPPORTED;
        m.q[i] = ps[i];
        m.g0[i] = (uint32_t)total;
        total += grid;
        if (total > 0x7FFFFFFFull) return ZHIP_E_UNSUPPORTED;
    }
    for (uint32_t i = n; i <= (uint32_t)ZHIP_MULTI_MAX; ++i) m.g0[i] = (uint32_t)total;
    m.n = n;
    if (dry) return ZHIP_OK;  // (zhip_decode_mapped_multi_check: the admission alone)
    return fire(fn, "k_decode_il", (uint32_t)total, kThreads, m, stream);  // (the same kernel body)
}

int launch_decode(const DecodeParams& p, hipStream_t stream, int max_grid) {
    const Launch L = make_launch(p, stream, max_grid);
    const bool crc = L.crc;
    if (takes_row_units(L)) return launch_row_units(L);
    if (p.rows)
        return launch_persistent(L, select_rows_kernel(crc, L.item, L.swap, (int)(p.seg / kWgStride)), "k_decode_rows");
    if (p.tq >= 0 && p.tile4) return launch_tile4(L);
    if (p.tq >= 0 && p.tile2) return launch_tile_pairs(L);
    if (p.tq >= 0 && p.tileg) return launch_tile_groups(L);
    if (p.tq >= 0) return launch_persistent(L, select_tile_kernel(crc, L.item, L.swap), "k_decode_tile");
    return launch_persistent(L, select_decode_kernel(crc, (p.lflags & ZHIP_LF_NO_WRITE) == 0, p.fast != 0, L.item,
                                                     L.swap, (int)(p.seg / kWgStride)), "k_decode");
}

}  // namespace zhip

extern "C" const char* zhip_last_kernel(void) { return zhip::g_last_kernel; }
extern "C" uint32_t zhip_last_grid(void) { return zhip::g_last_grid; }
extern "C" uint64_t zhip_launch_count(void) { return zhip::g_launch_count; }
