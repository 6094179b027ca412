// The context's memory owners (csrc/odo_ctx.h) and the one carver (Pack,
// csrc/odo_internal.h) under AddressSanitizer and UBSan, stand-alone and
// without a GPU: a grow-only block whose allocation fails, Pack's arithmetic,
// and the sizes of the two kernel-side layouts that are cut with Pack. Not part
// of the build or the suite; build and run it by hand on a CPU machine:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tests/cpp/ctx_memory_host_asan.cpp -o /tmp/ctx_memory_host_asan \
//       -Ladaptive-rgbd-localization-mappig_amd -lodo_hip -Wl,-rpath,$PWD/adaptive-rgbd-localization-mappig_amd
//   /tmp/ctx_memory_host_asan
//
// Without a device every hipMalloc and hipHostMalloc fails (hipErrorNoDevice,
// 100), which is the failure this program needs. What it cannot see is that
// reserve() clears HIP's last error: without a device hipGetLastError() reports
// error 100 for ever, cleared or not. That property rests on reading
// GrowBlock::reserve.
#include "../../adaptive-rgbd-localization-mappig_amd/csrc/odo_ctx.h"

#include <cstdio>

#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);      \
            return 1;                                                 \
        }                                                             \
    } while (0)

template <typename Block>
static int failed_allocation(const char* who) {
    Block b;
    EXPECT(b.reserve(0, 0, who) == ODO_OK && !b.p && b.cap == 0);  // nothing asked of an empty block
    for (int attempt = 0; attempt < 2; attempt++) {
        g_err.clear();
        EXPECT(b.reserve(4096, (size_t)1 << 20, who) == ODO_ERR_DEVICE);
        EXPECT(!b.p && b.cap == 0);
        const std::string msg = odo_last_error();
        EXPECT(!msg.empty() && msg.find(who) == 0);
    }
    b.release();
    EXPECT(!b.p && b.cap == 0);
    return 0;  // ~Block on an empty block
}

static int pack_arithmetic() {
    struct Case {
        std::vector<size_t> bytes, offs;
        size_t total;
    };
    const Case cases[] = {
        {{}, {}, 0},
        {{0}, {0}, 0},
        {{0, 0, 1, 0}, {0, 0, 0, 256}, 256},
        {{1, 255, 256, 257}, {0, 256, 512, 768}, 1280},
        {{511, 513, 0, 8}, {0, 512, 1280, 1280}, 1536},
        {{256 * 1000 - 1, 256 * 1000 + 1, 4}, {0, 256000, 512256}, 512512},
        {{((size_t)5 << 32) + 1, 3}, {0, ((size_t)5 << 32) + 256}, ((size_t)5 << 32) + 512},
    };
    for (const Case& c : cases) {
        Pack pk;
        for (size_t i = 0; i < c.bytes.size(); i++) EXPECT(pk.add(c.bytes[i]) == c.offs[i]);
        EXPECT(pk.off == c.total && pk.off % 256 == 0);
    }
    return 0;
}

// The constants are what the library of the commit before Pack cut these two
// layouts returned for the same shapes (k_ransac.hip's layout(), k_ba.hip's
// ba_al): the sizes, and with them every offset's upper bound, are unchanged.
static int layout_sizes() {
    odo_ransac_params p{200, 20, 3.0f, 4, 1};
    const RansacCfg c200 = ransac_cfg(p);
    p.iterations = 1000;
    const RansacCfg c1000 = ransac_cfg(p);
    EXPECT(ransac_scratch_bytes(1, 300, 10, c200) == 55296);  // one pair: no lanes slab
    EXPECT(ransac_scratch_bytes(64, 2000, 63, c200) == 59213056);
    EXPECT(ransac_scratch_bytes(3, 257, 9, c1000) == 7734016);
    EXPECT(ba_scratch_bytes(1, 1, 1, 1) == 7424);              // the smallest problem
    EXPECT(ba_scratch_bytes(5, 2048, 10240, 4) == 2105856);
    EXPECT(ba_scratch_bytes(5, 20000, 900, 3) == 3949312);     // 20 000 landmarks: BA_MAX_CHUNKS chunks of 313
    return 0;
}

int main() {
    using namespace odo;
    if (failed_allocation<DevBlock>("device block") || failed_allocation<PinnedBlock>("pinned block")) return 1;
    if (pack_arithmetic() || layout_sizes()) return 1;
    {   // a context that was never created on a device frees itself
        odo_ctx ctx;
        EXPECT(stage_reserve(&ctx, 100) == ODO_ERR_DEVICE && !ctx.stage.p && ctx.stage.cap == 0);
    }
    std::printf("ctx_memory_host_asan: failed allocations, Pack and the layout sizes passed\n");
    return 0;
}
