// Stand-alone host check of the plan table builders: creates the plans of
// tests/test_plan_tables.py's matrix and builds both images of each into
// exact-size buffers.  Built with AddressSanitizer / UBSan on the host code
// (make -C zarr-python_amd check-plan-tables), it exits 0 when the builders
// stay inside their regions.  CPU only: no HIP call is made.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/zarrhip.h"

static int check(std::vector<int32_t> shape, int itemsize, int tq, uint32_t flags, uint32_t n_inner = 0) {
    zhip_layout L{};
    L.ndim = (int32_t)shape.size();
    L.itemsize = itemsize;
    L.nbytes = (uint64_t)itemsize;
    for (int d = 0; d < L.ndim; ++d) L.nbytes *= (uint64_t)(L.shape[d] = shape[d]);
    int64_t stride = itemsize;  // out: dim tq contiguous, the others in stored order
    if (tq >= 0) L.out_stride[tq] = stride, stride *= shape[tq];
    for (int d = L.ndim - 1; d >= 0; --d)
        if (d != tq) L.out_stride[d] = stride, stride *= shape[d];
    L.flags = flags;
    L.n_inner = n_inner;
    L.index_size = n_inner ? 16 * n_inner + 4 : 0;
    zhip_plan* plan = nullptr;
    if (zhip_plan_create(&L, &plan) != ZHIP_OK) return std::printf("plan_create: %s\n", zhip_last_error()), 1;
    uint64_t regions[256];
    const uint32_t n_regions = zhip_plan_table_offsets(plan, regions, 256);
    for (int which = 0; which < 2; ++which) {
        std::vector<uint32_t> image(zhip_plan_table_image(plan, which, nullptr, 0));
        if (zhip_plan_table_image(plan, which, image.data(), image.size()) != image.size()) return 1;
        if (which == 0 && (image.empty() || n_regions == 0 || n_regions > 128)) return 1;
    }
    return zhip_plan_destroy(plan);
}

int main() {
    int bad = 0;
    for (int32_t n : {0, 16, 4096, 32768, 65536, 131072, 258048, 258041, 516096, 1024000, 1081344, 2097152, 8650752})
        bad |= check({n}, 1, -1, ZHIP_LF_CRC);
    for (int32_t n : {258048, 1024000}) {
        bad |= check({n}, 1, -1, 0);
        bad |= check({n}, 1, -1, ZHIP_LF_CRC | ZHIP_LF_NO_WRITE);
        bad |= check({n}, 1, -1, ZHIP_LF_CRC | ZHIP_LF_SHARDED, 8);
    }
    const uint32_t f32 = ZHIP_LF_CRC | ZHIP_LF_FLOAT;
    bad |= check({64, 64}, 4, 0, f32) | check({64, 256}, 4, 0, f32) | check({4, 64, 64}, 4, 1, f32);
    bad |= check({128, 128}, 4, 0, f32) | check({70, 40}, 4, 0, f32) | check({128, 64, 64}, 4, 1, f32);
    bad |= check({64, 256}, 4, 0, ZHIP_LF_FLOAT) | check({4, 64, 64}, 4, 1, ZHIP_LF_FLOAT);
    std::printf(bad ? "plan_tables_check: FAILED\n" : "plan_tables_check: ok\n");
    return bad;
}
