// Stand-alone host check of the fill-equality rule: drives zhip_emulate_fill_eq
// (the function the encode kernels share, csrc/zhip_fill_eq.h) over EVERY bit
// pattern of the 1- and 2-byte items and the edge patterns of the 4- and
// 8-byte ones as item -- and as fill every pattern of the 1-byte items, twelve
// patterns of the 2-byte ones (one per class of fill: zeros, subnormal, finite,
// the infinities, both NaN thresholds, all ones; 2^32 pairs are too many) and
// the edge patterns of the wider ones -- against a restatement of
// NDBuffer.all_equal through the host's own floating-point compare (float and
// double; float16 through its field layout).  Built with AddressSanitizer /
// UBSan on the host code (make -C zarr-python_amd check-fill-eq), it exits 0
// when every answer agrees and the argument checks hold.  CPU only: no HIP
// call is made.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/zarrhip.h"

static int g_fail = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (g_fail < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                \
        }                                                            \
    } while (0)

static bool half_nan(uint16_t x) { return ((x >> 10) & 0x1Fu) == 0x1Fu && (x & 0x3FFu) != 0; }
static float f32(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static double f64(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

enum Kind { kInt, kFloat, kCplx };

// all_equal for one item: integers compare bits; floats compare bits, and any
// NaN equals a NaN fill; complex64 compares components as values, and any item
// with a NaN component equals a fill with one
static bool want_eq(Kind kind, uint32_t item, uint64_t x, uint64_t f) {
    if (kind == kInt) return x == f;
    if (kind == kFloat) {
        if (x == f) return true;
        if (item == 2) return half_nan((uint16_t)x) && half_nan((uint16_t)f);
        if (item == 4) return std::isnan(f32((uint32_t)x)) && std::isnan(f32((uint32_t)f));
        return std::isnan(f64(x)) && std::isnan(f64(f));
    }
    const float xr = f32((uint32_t)x), xi = f32((uint32_t)(x >> 32)), fr = f32((uint32_t)f), fi = f32((uint32_t)(f >> 32));
    const bool xn = std::isnan(xr) || std::isnan(xi), fn = std::isnan(fr) || std::isnan(fi);
    if (xn || fn) return xn && fn;
    return xr == fr && xi == fi;
}

static std::vector<uint64_t> patterns(Kind kind, uint32_t item) {
    std::vector<uint64_t> v;
    if (item <= 2) {
        for (uint64_t x = 0; x < (1ull << (8 * item)); ++x) v.push_back(x);
        return v;
    }
    if (item == 4 || kind == kCplx) {
        const std::vector<uint32_t> w = {0x00000000u, 0x80000000u, 0x00000001u, 0x3F800000u, 0x3FC00000u, 0xC0200000u,
                                         0x7F7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7F800001u, 0xFF800001u, 0x7FC00000u,
                                         0xFFC00000u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0x7FBFFFFFu};
        if (item == 4) {
            for (uint32_t a : w) v.push_back(a);
        } else {
            for (uint32_t a : w)
                for (uint32_t b : w) v.push_back(((uint64_t)b << 32) | a);
        }
        return v;
    }
    return {0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x3FF8000000000000ull,
            0x7FEFFFFFFFFFFFFFull, 0x7FF0000000000000ull, 0xFFF0000000000000ull, 0x7FF0000000000001ull,
            0xFFF0000000000001ull, 0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FFFFFFFFFFFFFFFull,
            0xFFFFFFFFFFFFFFFFull, 0x7FF0000100000000ull, 0x7FF00000FFFFFFFFull, 0x7FF7FFFFFFFFFFFFull,
            // a NaN only by its low word, a NaN only by its high word
            0x7FF0000080000000ull, 0x7FF8000000000001ull};
}

static void sweep(Kind kind, uint32_t item) {
    const uint32_t lflags = kind == kFloat ? ZHIP_LF_FLOAT : kind == kCplx ? ZHIP_LF_COMPLEX : 0u;
    const std::vector<uint64_t> pats = patterns(kind, item);
    // the items as the kernels see them: native-order bytes, back to back
    std::vector<uint8_t> items(pats.size() * item);
    for (size_t i = 0; i < pats.size(); ++i) memcpy(items.data() + i * item, &pats[i], item);
    std::vector<uint8_t> eq(pats.size());
    // 2-byte items, integer and float alike: every fill would be 2^32 pairs; these cover each class of fill
    std::vector<uint64_t> fills = pats;
    if (item == 2) fills = {0x0000, 0x8000, 0x0001, 0x3C00, 0x3E00, 0x7BFF, 0x7C00, 0xFC00, 0x7C01, 0xFC01, 0x7E00, 0xFFFF};
    for (uint64_t f : fills) {
        uint8_t fb[8];
        memcpy(fb, &f, 8);
        uint32_t fnan = 99;
        CHECK(zhip_emulate_fill_eq(item, lflags, fb, items.data(), pats.size(), eq.data(), &fnan) == ZHIP_OK);
        bool f_nan = false;
        if (kind == kFloat) f_nan = item == 2 ? half_nan((uint16_t)f) : item == 4 ? std::isnan(f32((uint32_t)f)) : std::isnan(f64(f));
        if (kind == kCplx) f_nan = std::isnan(f32((uint32_t)f)) || std::isnan(f32((uint32_t)(f >> 32)));
        CHECK(fnan == (f_nan ? 1u : 0u));
        for (size_t i = 0; i < pats.size(); ++i) {
            const bool want = want_eq(kind, item, pats[i], f);
            if ((eq[i] != 0) != want && g_fail < 20)
                printf("kind %d item %u fill %016llx x %016llx: got %d want %d\n", (int)kind, item, (unsigned long long)f,
                       (unsigned long long)pats[i], (int)eq[i], (int)want);
            CHECK((eq[i] != 0) == want);
        }
    }
}

int main() {
    for (uint32_t item : {1u, 2u, 4u, 8u}) sweep(kInt, item);
    for (uint32_t item : {2u, 4u, 8u}) sweep(kFloat, item);
    sweep(kCplx, 8);
    // a 1-byte "float" layout has no NaN: bits only
    {
        const uint8_t fill = 0xFF, x[2] = {0xFF, 0x7F};
        uint8_t eq[2];
        uint32_t fnan = 9;
        CHECK(zhip_emulate_fill_eq(1, ZHIP_LF_FLOAT, &fill, x, 2, eq, &fnan) == ZHIP_OK);
        CHECK(fnan == 0 && eq[0] == 1 && eq[1] == 0);
    }
    // argument checks
    {
        const uint64_t z = 0;
        uint8_t eq[1];
        CHECK(zhip_emulate_fill_eq(3, 0, &z, &z, 1, eq, nullptr) == ZHIP_E_UNSUPPORTED);
        CHECK(zhip_emulate_fill_eq(16, 0, &z, &z, 1, eq, nullptr) == ZHIP_E_UNSUPPORTED);
        CHECK(zhip_emulate_fill_eq(4, ZHIP_LF_COMPLEX, &z, &z, 1, eq, nullptr) == ZHIP_E_INVALID);
        CHECK(zhip_emulate_fill_eq(8, ZHIP_LF_COMPLEX | ZHIP_LF_FLOAT, &z, &z, 1, eq, nullptr) == ZHIP_E_INVALID);
        CHECK(zhip_emulate_fill_eq(8, 0, nullptr, &z, 1, eq, nullptr) == ZHIP_E_INVALID);
        CHECK(zhip_emulate_fill_eq(8, 0, &z, nullptr, 1, eq, nullptr) == ZHIP_E_INVALID);
        CHECK(zhip_emulate_fill_eq(8, 0, &z, nullptr, 0, nullptr, nullptr) == ZHIP_OK);
    }
    if (g_fail) {
        printf("fill_eq_check: %d failures\n", g_fail);
        return 1;
    }
    printf("fill_eq_check ok\n");
    return 0;
}
