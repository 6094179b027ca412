// Frame::CreateCloud / Frame::VoxelGridFilterCloud of include/odo_frontend.hpp
// (Core/frame.h:48-49, :80) on one frame read from a file (BGR8 then depth16).
// Prints one line per step: the step, the cloud's point count and a position-
// weighted checksum of its 32-bit words; tests/test_cloud_frontend_cpp.py compares them with
// the Python binding on the same frame.
//
//   cloud_mirror frames.bin width height leaf
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "odo_frontend.hpp"

// sum of word[i] * (2 i + 1) modulo 2^64
static uint64_t checksum(const std::vector<odo_cloud_point>& c) {
    std::vector<uint32_t> w(c.size() * 4);
    if (!c.empty()) std::memcpy(w.data(), c.data(), w.size() * 4);
    uint64_t h = 0;
    for (size_t i = 0; i < w.size(); i++) h += (uint64_t)w[i] * (2 * (uint64_t)i + 1);
    return h;
}

static void report(const char* step, const odo_hip::Frame& f) {
    std::printf("%s %zu %016" PRIx64 "\n", step, f.mpCloud.size(), checksum(f.mpCloud));
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: cloud_mirror frames.bin width height leaf\n");
        return 2;
    }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    const float leaf = (float)std::atof(argv[4]);
    const size_t px = (size_t)w * h;
    std::vector<uint8_t> bgr(px * 3);
    std::vector<uint16_t> depth(px);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(bgr.data(), 1, bgr.size(), fp) != bgr.size() || std::fread(depth.data(), 2, px, fp) != px) {
        std::fprintf(stderr, "cloud_mirror: cannot read %s\n", argv[1]);
        return 2;
    }
    std::fclose(fp);
    try {
        odo_hip::Frame f(bgr.data(), depth.data(), w, h, 0.0);
        f.VoxelGridFilterCloud(leaf);  // no cloud yet: returns (frame.cpp:219)
        if (f.HasCloud() || !f.mpCloud.empty()) return 4;
        f.CreateCloud();
        report("create", f);
        f.CreateCloud();  // a frame keeps its cloud (frame.cpp:193)
        report("create", f);
        f.VoxelGridFilterCloud(leaf);
        report("filter", f);
    } catch (const odo_hip::Error& e) {
        std::fprintf(stderr, "cloud_mirror: %s\n", e.what());
        return 3;
    }
    return 0;
}
