// The chunk arrival and CRC verdict protocol: the one place where the CRC
// kernels (decode.hip, decode_rows.hip, decode_tile.hip, encode.hip) talk to
// each other across workgroups.  A workgroup reduces its lanes' Horner states
// to one word V in the chunk's frame, publishes V into the chunk's workspace
// word with a sign of arrival, and the arrival that completes the chunk turns
// the accumulated word into a CRC-32C: decode compares it with the stored
// trailer and writes the chunk's zhip_status (crc_verdict), encode writes the
// little-endian trailer (put_le_u32).
//
// Workspace layout (uint32_t words at p.ws; zhip_plan_info sizes it).
//   Packed: four words per chunk at ws + 4c.  CRC layouts of the kernels that
//   pass wstride = kPubLine / 2 (or pub_stride) own a 128-byte line per chunk
//   at ws + kPubLine*c instead, so one chunk's returning atomics do not share
//   a line with seven other chunks'.
//   A chunk's words are used in ONE of these forms per launch:
//   - mask word: the 64-bit word {0,1}: low half the XOR of the contributions,
//     high half the arrival bits (<= 32 arrivals; the grouped and encode forms
//     keep arrival bits in 32..47 and non-empty bits in 48..63, <= 16
//     arrivals).  Kernels with 33..64 arrivals on a line use words {0,1} and
//     {2,3} for 32 each and {4,5} as the second level.
//   - counted pair: accw = ws + 4c holds the XOR, accw + 2 the number of
//     arrivals (encode: arrived | non-empty << 16).  Any number of arrivals.
//   - deferred-verdict banks: bank b is {word, stored} at ws + 4c + 2b;
//     a launch xors into bank p.dv_bank without a returning atomic and reads
//     the other bank, where the previous launch left computed ^ stored
//     (dv_prev / dv_publish / dv_settle; k_dv_check folds both banks).
//   Subword tail, after every chunk's words: 64-bit words of up to 16 (32 for
//   k_decode_xw) arrivals whose completing arrival carries the subgroup's XOR
//   on to the chunk word.  Packed: at ws + 4 n_chunks, word c*n_sub + sg.
//   SPR (spread): chunk lines at ws + 32c, then one 128-byte line per subword
//   at ws + 32 n_chunks + 32 (c*n_sub + sg).
//
// The three rules.
//   Ordering: in the counted form the xor must have been performed at the
//   device-coherent point before the ticket is drawn, so the ticket that
//   completes the chunk sees every contribution: the s_waitcnt vmcnt(0) tied
//   to the xor's returned value.  The mask forms carry contribution and
//   arrival in one atomic and need no wait.
//   Reset: the completing arrival zeroes every word it used (relaxed stores:
//   nobody else touches the chunk again in this launch), so the next launch
//   starts from a clean workspace without a clearing pass.
//   One lane: only one lane of the workgroup touches the workspace.  The wave
//   forms (publish_bits, retire_uniform, finalize_uniform) run wave-uniformly
//   so the GF(2) work stays on the scalar unit, with lane t == 0 at memory.
#pragma once
#include "zhip_decode_common.h"

namespace zhip {

// Wave-uniform multiply (scalar ALU): both operands are read from lane 0.
__device__ __forceinline__ uint32_t gf_mul_uniform(uint32_t a, uint32_t b) {
    return gf_mul(__builtin_amdgcn_readfirstlane(a), __builtin_amdgcn_readfirstlane(b));
}

// ---- verdict ----
// The chunk's accumulated word `raw`, already scaled by c_inv (the kernels
// whose lane or unit constants carry it), against the stored little-endian
// trailer (crc32c_.py:41-49): status and, on mismatch, the error bit.  Every
// calling lane computes; `writer` selects the one that writes.
__device__ __forceinline__ void crc_verdict(const DecodeParams& p, uint32_t c, uint32_t stored, uint32_t raw,
                                            bool writer = true) {
    const uint32_t computed = ~(raw ^ p.c3);
    const uint32_t code = computed == stored ? ZHIP_ST_OK : ZHIP_ST_CRC_MISMATCH;
    if (writer) {
        zhip_status st = {code, stored, computed, 0u};
        p.status[c] = st;
        if (code != ZHIP_ST_OK) atomicOr(p.errflag, 1u << code);
    }
}

// One lane, unscaled raw.
__device__ __forceinline__ void finalize_chunk(const DecodeParams& p, uint32_t c, uint32_t stored, uint32_t raw) {
    crc_verdict(p, c, stored, gf_mul(raw, p.c_inv));
}

// Wave 0, wave-uniform arguments; lane t == 0 writes.
__device__ __forceinline__ void finalize_uniform(const DecodeParams& p, uint32_t c, uint32_t stored, uint32_t raw,
                                                 int t, bool scaled = false) {
    crc_verdict(p, c, stored, scaled ? raw : gf_mul_uniform(raw, p.c_inv), t == 0);
}

// A mismatch found in a deferred-verdict word w = computed ^ stored.
__device__ __forceinline__ void report_mismatch(zhip_status* status, uint32_t* errflag, uint32_t c, uint32_t stored,
                                                uint32_t w) {
    zhip_status st = {ZHIP_ST_CRC_MISMATCH, stored, w ^ stored, 0u};
    status[c] = st;
    atomicOr(errflag, 1u << ZHIP_ST_CRC_MISMATCH);
}

// Encode's trailer (crc32c_.py:64-68): LE u32 at any alignment.
__device__ __forceinline__ void put_le_u32(uint8_t* d, uint32_t v) {
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
    d[2] = (uint8_t)(v >> 16);
    d[3] = (uint8_t)(v >> 24);
}

// ---- mask form: one 64-bit fetch_xor of (bits << 32) | V ----
// Its halves, for the callers that test one run later (Pending / PendingU):
// issue, the completion test on the returned arrival bits, and the reset.
// The helpers below end in done(raw) -- the completing arrival's
// continuation, with the XOR of every contribution -- rather than returning
// a flag: inlined, that is the hand-written nesting, instruction for
// instruction.
__device__ __forceinline__ uint64_t mask_issue(uint64_t* w, uint64_t bits, uint32_t V) {
    return __hip_atomic_fetch_xor(w, (bits << 32) | V, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The one test, arrived ^ own bits == full, in its two operand widths: on the
// returned 64-bit word (one lane) and on its broadcast high half (wave form).
__device__ __forceinline__ bool mask_full(uint64_t prev, uint64_t bits, uint64_t full) {
    return ((prev >> 32) ^ bits) == full;
}

__device__ __forceinline__ bool mask_full_hi(uint32_t hi, uint32_t bits, uint64_t full) {
    return (uint64_t)(hi ^ bits) == full;
}

__device__ __forceinline__ void mask_reset(uint64_t* w) {
    __hip_atomic_store(w, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t mask_of(uint32_t n) {  // n <= 32 arrivals
    return n >= 32u ? 0xFFFFFFFFull : ((1ull << n) - 1ull);
}

// One lane.
template <class Done>
__device__ __forceinline__ void arrive_mask(uint64_t* w, uint64_t bits, uint32_t V, uint64_t full, Done done) {
    const uint64_t prev = mask_issue(w, bits, V);
    if (mask_full(prev, bits, full)) {
        mask_reset(w);
        done((uint32_t)prev ^ V);
    }
}

struct Pending {  // thread 0's outstanding arrival for one run, checked one run later
    uint64_t prev;
    uint32_t stored, c, bits, V, valid;
};

__device__ __forceinline__ void retire(const DecodeParams& p, Pending& q, uint64_t full) {
    if (!q.valid) return;
    q.valid = 0;
    if (mask_full(q.prev, q.bits, full)) {
        uint64_t* w = reinterpret_cast<uint64_t*>(p.ws) + 2ull * q.c;
        mask_reset(w);
        finalize_chunk(p, q.c, q.stored, (uint32_t)q.prev ^ q.V);
    }
}

struct PendingU {   // the same, held by wave 0 wave-uniformly
    uint64_t prev;  // lane 0: returned 64-bit arrival word (consumed one run later)
    uint32_t stored, c, bits, V, valid;
};

__device__ __forceinline__ void retire_uniform(const DecodeParams& p, PendingU& q, uint64_t full, int t,
                                               bool scaled = false) {
    if (!q.valid) return;
    q.valid = 0;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)q.prev);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(q.prev >> 32));
    if (mask_full_hi(hi, q.bits, full)) {
        if (t == 0) {
            uint64_t* w = reinterpret_cast<uint64_t*>(p.ws) + 2ull * q.c;
            mask_reset(w);
        }
        finalize_uniform(p, q.c, q.stored, lo ^ q.V, t, scaled);
    }
}

// ---- counted form: xor -> wait -> ticket -> exchange -> reset ----
// One lane; n arrivals of `total` come with this call; done(raw) for the call
// completing the chunk, with the accumulated word.
// SETTLE: also wait for the exchange's return before going on.  The row
// kernels' wave 0 goes straight back to a loop of loads and stores: a register
// with a returning atomic still pending would make every later write to it
// wait for the wave's stores too, so the rare completing path consumes the
// value here.  The kernels whose lane 0 ends after the verdict do not need it
// and do not have it.
template <bool SETTLE = false, class Done>
__device__ __forceinline__ void arrive_count(uint32_t* accw, uint32_t V, uint32_t n, uint32_t total, Done done) {
    const uint32_t prev = __hip_atomic_fetch_xor(accw, V, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");  // the ordering rule
    const uint32_t tk = __hip_atomic_fetch_add(accw + 2, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk + n == total) {
        const uint32_t raw = __hip_atomic_exchange(accw, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (SETTLE) asm volatile("s_waitcnt vmcnt(0)" ::"v"(raw) : "memory");
        __hip_atomic_store(accw + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        done(raw);
    }
}

// ---- one publication for wave 0 of a row kernel ----
// The workgroup's reduced contribution V with its arrival bits (n of them, of
// `total` per chunk), wave-uniform: the mask form up to 32 arrivals per chunk
// (wstride 64-bit words between chunks' words: 2 packed, kPubLine / 2 for a
// line per chunk), else the counted form; the completing arrival compares
// with the trailer (V scaled by c_inv).
__device__ __forceinline__ void publish_bits(const DecodeParams& p, uint32_t c, uint64_t bits, uint32_t n,
                                             uint32_t total, uint32_t V, uint32_t stored, int t,
                                             uint32_t wstride = 2u) {
    if (total <= 32u) {  // the mask form from its halves: lane 0 at memory, the test on the broadcast word
        const uint64_t full = total >= 32u ? 0xFFFFFFFFull : ((1ull << total) - 1ull);  // (mask_of, spelled out)
        uint64_t prev = 0;
        uint64_t* const w = reinterpret_cast<uint64_t*>(p.ws) + (uint64_t)wstride * c;
        if (t == 0) prev = mask_issue(w, bits, V);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)prev);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(prev >> 32));
        if (mask_full_hi(hi, (uint32_t)bits, full)) {
            if (t == 0) mask_reset(w);
            finalize_uniform(p, c, stored, lo ^ V, t, true);
        }
    } else {  // counted, not the population of a mask: arrivals past 32 would set some bit twice.
        // arrive_count<true> spelled without its continuation (the closure reorders the two
        // registers of raw / last in the row kernels)
        uint32_t raw = 0, last = 0;
        if (t == 0) {
            uint32_t* accw = p.ws + 4ull * c;
            const uint32_t prev = __hip_atomic_fetch_xor(accw, V, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");
            const uint32_t tk = __hip_atomic_fetch_add(accw + 2, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tk + n == total) {
                raw = __hip_atomic_exchange(accw, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::"v"(raw) : "memory");
                __hip_atomic_store(accw + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        if (__builtin_amdgcn_readfirstlane(last))
            finalize_uniform(p, c, stored, __builtin_amdgcn_readfirstlane(raw), t, true);
    }
}

// ---- deferred CRC verdicts (zarrhip.h), for the decode kernels that publish
// without a returning atomic ----
// {word, stored} of chunk c in the OTHER bank (the previous launch's verdict),
// read by the chunk's first workgroup; one address for every lane (`zero`
// otherwise), so every path issues the same vector load.
__device__ __forceinline__ uint64_t dv_prev(const DecodeParams& p, uint32_t c, bool first, const void* zero) {
    return __hip_atomic_load(reinterpret_cast<const uint64_t*>(
                                 first ? p.ws + 4ull * c + 2u * (p.dv_bank ^ 1u) : static_cast<const uint32_t*>(zero)),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane: xor the workgroup's (chunk-referenced) contribution into this
// launch's bank word -- the first workgroup also folds in c3 ^ ~stored, so
// the word ends as computed ^ stored -- and record the trailer.  The atomic's
// result is unused: nobody waits for its round trip.
__device__ __forceinline__ void dv_publish(const DecodeParams& p, uint32_t c, bool first, uint32_t V,
                                           uint32_t stored) {
    uint32_t* w = p.ws + 4ull * c + 2u * p.dv_bank;
    __hip_atomic_fetch_xor(w, V ^ (first ? (p.c3 ^ ~stored) : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (first) __hip_atomic_store(w + 1, stored, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane of the first workgroup, after the chunk's own status: a nonzero
// previous verdict is the previous launch's mismatch (sticky status + error
// bit); its word is cleared for the launch after this one.
__device__ __forceinline__ void dv_settle(const DecodeParams& p, uint32_t c, uint64_t prev) {
    const uint32_t pw = (uint32_t)prev, ps = (uint32_t)(prev >> 32);
    if (pw != 0u) {
        report_mismatch(p.status, p.errflag, c, ps, pw);
        __hip_atomic_store(p.ws + 4ull * c + 2u * (p.dv_bank ^ 1u), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Arrival of one workgroup of a grouped tile kernel (k_decode_tileg /
// k_encode_tileg) with its CRC contribution v and non-empty bit: 64-bit words
// CRC (low 32) | arrival bits (32..47) | non-empty bits (48..63), one relaxed
// XOR per level.  Up to 16 groups per chunk the chunk word is the only level;
// up to 256 the groups first meet in words of 16 (the workspace tail after the
// 4 words per chunk), whose completing arrival carries the subgroup's XOR on
// to the chunk word.  True for the arrival completing the chunk, with the
// XOR of every contribution and whether any group was non-empty.
// SPR: every subword and the chunk's word on a 128-byte line of its own
// (chunk lines at ws + 32 c, subword lines after all chunk lines;
// zhip_plan_info sizes the workspace for it), so a chunk's arrivals do not
// meet on one line: production for k_decode_tilegw's two-tile form -- C3 in
// 128^3 chunks, 256 arrivals per chunk, 28.94 / 29.00 vs 29.57 / 29.28 us
// graph-timed (profiles/r05/aa/; tuning arm 48 keeps the packed words); in
// k_encode_tileg (128 arrivals per chunk) neutral, tuning arm 47.
template <bool SPR = false>
__device__ __forceinline__ bool tileg_arrive(uint32_t* ws, uint32_t n_chunks, uint32_t c, uint32_t grp,
                                             uint32_t gpc, uint32_t n_sub, uint32_t v, bool ne, uint32_t& raw,
                                             bool& any_ne) {
    if (n_sub) {
        const uint32_t sg = grp >> 4;
        const uint32_t in_sg = min(16u, gpc - (sg << 4));
        uint64_t* sw = SPR ? reinterpret_cast<uint64_t*>(ws + 32ull * n_chunks) + ((uint64_t)c * n_sub + sg) * 16u
                           : reinterpret_cast<uint64_t*>(ws + 4ull * n_chunks) + (uint64_t)c * n_sub + sg;
        const uint64_t b = 1ull << (grp & 15u);
        const uint64_t prev = __hip_atomic_fetch_xor(sw, (b << 32) | (ne ? b << 48 : 0ull) | v, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
        if ((((prev >> 32) & 0xFFFFull) ^ b) != (1ull << in_sg) - 1ull) return false;
        __hip_atomic_store(sw, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v ^= (uint32_t)prev;
        ne = ne || ((prev >> 48) & 0xFFFFull) != 0ull;
        grp = sg;
        gpc = n_sub;
    }
    uint64_t* cw = reinterpret_cast<uint64_t*>(ws) + (SPR ? 16ull : 2ull) * c;
    const uint64_t b = 1ull << grp;
    const uint64_t prev = __hip_atomic_fetch_xor(cw, (b << 32) | (ne ? b << 48 : 0ull) | v, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    if ((((prev >> 32) & 0xFFFFull) ^ b) != (1ull << gpc) - 1ull) return false;
    __hip_atomic_store(cw, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    raw = (uint32_t)prev ^ v;
    any_ne = ne || ((prev >> 48) & 0xFFFFull) != 0ull;
    return true;
}

// tileg_arrive with the look-back finalizer (round 6; tuning arms 62 / 63):
// the subwords of 16 arrivals on lines of their own (tileg_arrive SPR's
// layout; one word of up to 16 when n_sub is 0).  Every workgroup but the
// chunk's last (grp = gpc - 1) xors its bit | non-empty bit | v with a
// NON-returning atomic and returns false; the last one polls every subword
// (one lane, relaxed agent loads) until all the other arrivals are in, resets
// them and returns true with the chunk's raw sum and non-empty flag.  The
// caller takes it only while fewer chunks than CUs are in the launch (the
// finalizers then never hold every slot; publish_lb, decode_rows.hip).
__device__ __forceinline__ bool tileg_arrive_lb(uint32_t* ws, uint32_t n_chunks, uint32_t c, uint32_t grp,
                                                uint32_t gpc, uint32_t n_sub, uint32_t v, bool ne, uint32_t& raw,
                                                bool& any_ne) {
    const uint32_t nsw = n_sub ? n_sub : 1u;
    uint64_t* const base = n_sub ? reinterpret_cast<uint64_t*>(ws + 32ull * n_chunks) + (uint64_t)c * n_sub * 16u
                                 : reinterpret_cast<uint64_t*>(ws) + 16ull * c;
    const uint32_t sg = n_sub ? grp >> 4 : 0u;
    const uint64_t b = 1ull << (n_sub ? (grp & 15u) : grp);
    if (grp + 1u < gpc) {
        (void)__hip_atomic_fetch_xor(base + 16ull * sg, (b << 32) | (ne ? b << 48 : 0ull) | v, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
        return false;
    }
    uint32_t acc = v;
    bool nn = ne;
    for (uint32_t s = 0; s < nsw; ++s) {
        const uint32_t in_s = n_sub ? min(16u, gpc - 16u * s) : gpc;
        uint64_t expect = (1ull << in_s) - 1ull;
        if (s == sg) expect ^= b;
        uint64_t* const w = base + 16ull * s;
        uint64_t cur;
        for (;;) {
            cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (((cur >> 32) & 0xFFFFull) == expect) break;
            __builtin_amdgcn_s_sleep(1);
        }
        __hip_atomic_store(w, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc ^= (uint32_t)cur;
        nn = nn || ((cur >> 48) & 0xFFFFull) != 0ull;
    }
    raw = acc;
    any_ne = nn;
    return true;
}

}  // namespace zhip
