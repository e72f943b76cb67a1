// Stand-alone host check of the full-row form's tables and emulator
// (zhip_emulate_chunk_crc_ilx): creates the plans of tests/test_fullrow_tables.py,
// builds the row table image of each and runs the emulator for every span
// count against the host CRC-32C.  Built with AddressSanitizer / UBSan on the
// host code (make -C zarr-python_amd check-fullrow-tables), it exits 0 when
// the builders and the emulator stay inside their buffers and agree with the
// plain CRC.  CPU only: no HIP call is made.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/zarrhip.h"

static int check(int32_t n) {
    zhip_layout L{};
    L.ndim = 1;
    L.itemsize = 1;
    L.shape[0] = n;
    L.out_stride[0] = 1;
    L.nbytes = (uint64_t)n;
    L.flags = ZHIP_LF_CRC;
    zhip_plan* plan = nullptr;
    if (zhip_plan_create(&L, &plan) != ZHIP_OK) return std::printf("plan_create: %s\n", zhip_last_error()), 1;
    std::vector<uint32_t> image(zhip_plan_table_image(plan, 0, nullptr, 0));
    if (image.empty() || zhip_plan_table_image(plan, 0, image.data(), image.size()) != image.size()) return 1;
    // exact-size payload plus the 16 bytes of slack the emulators' block loads may touch
    std::vector<uint8_t> data((size_t)n + 16, 0);
    uint32_t x = 0x9E3779B9u ^ (uint32_t)n;
    for (int32_t i = 0; i < n; ++i) data[i] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    const uint32_t want = zhip_crc32c_host(data.data(), (uint64_t)n);
    int bad = 0;
    for (uint32_t P : {1u, 2u, 4u}) {
        const uint32_t got = zhip_emulate_chunk_crc_ilx(plan, data.data(), P);
        if (got != want) bad |= std::printf("n=%d P=%u: %08x != %08x\n", n, P, got, want), 1;
    }
    uint32_t units = 0, ws_words = 0;  // four 8 KiB spans per 32 KiB unit: three tile them or the form is declined
    if (zhip_plan_info(plan, &units, &ws_words) != ZHIP_OK) return 1;
    if (zhip_emulate_chunk_crc_ilx(plan, data.data(), 3) != ((4 * units) % 3 ? 0xFFFFFFFFu : want)) bad = 1;
    if (zhip_emulate_chunk_crc_ilx(plan, data.data(), 0) != 0xFFFFFFFFu) bad = 1;
    if (zhip_emulate_chunk_crc_ilx(plan, data.data(), 1) != zhip_emulate_chunk_crc_xw(plan, data.data())) bad = 1;
    return bad | zhip_plan_destroy(plan);
}

int main() {
    int bad = 0;
    for (int32_t n : {524288, 1048576, 1028096, 1024000, 262144 + 4100}) bad |= check(n);
    std::printf(bad ? "fullrow_tables_check: FAILED\n" : "fullrow_tables_check: ok\n");
    return bad;
}
