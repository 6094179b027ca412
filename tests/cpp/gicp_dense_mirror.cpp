// GeneralizedICP::Compute(pF1, pF2, guess) of include/odo_frontend.hpp
// (Odometry/generalizedicp.cpp:41-53) on two frames read from a file (BGR8 then
// depth16, frame after frame). Prints "empty <0|1>" for a frame without a cloud
// on either side, then "gicp <converged>" and the 16 words of mT12 in hex;
// tests/test_gicp_dense_frontend_cpp.py compares them with the Python binding
// on the same frames.
//
//   gicp_dense_mirror frames.bin width height leaf iterations max_corr_dist
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "odo_frontend.hpp"

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: gicp_dense_mirror frames.bin width height leaf iterations max_corr_dist\n");
        return 2;
    }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    const float leaf = (float)std::atof(argv[4]);
    const size_t px = (size_t)w * h;
    std::vector<uint8_t> bgr(2 * px * 3);
    std::vector<uint16_t> depth(2 * px);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(bgr.data(), 1, bgr.size(), fp) != bgr.size() ||
        std::fread(depth.data(), 2, depth.size(), fp) != depth.size()) {
        std::fprintf(stderr, "gicp_dense_mirror: cannot read %s\n", argv[1]);
        return 2;
    }
    std::fclose(fp);
    try {
        odo_hip::Frame f1(bgr.data(), depth.data(), w, h, 0.0), f2(bgr.data() + px * 3, depth.data() + px, w, h, 1.0);
        odo_hip::GeneralizedICP gicp(std::atoi(argv[5]), std::atof(argv[6]));
        f1.CreateCloud();
        f1.VoxelGridFilterCloud(leaf);
        // f2 has no cloud yet: false without running (generalizedicp.cpp:43)
        std::printf("empty %d\n", (int)(gicp.Compute(&f1, &f2, odo_hip::Identity()) || gicp.Compute(&f2, &f1, odo_hip::Identity())));
        f2.CreateCloud();
        f2.VoxelGridFilterCloud(leaf);
        const bool ok = gicp.Compute(&f1, &f2, odo_hip::Identity());
        std::printf("gicp %d", (int)ok);
        for (int i = 0; i < 16; i++) {
            uint32_t u;
            std::memcpy(&u, &gicp.mT12[i], 4);
            std::printf(" %08" PRIx32, u);
        }
        std::printf("\n");
    } catch (const odo_hip::Error& e) {
        std::fprintf(stderr, "gicp_dense_mirror: %s\n", e.what());
        return 3;
    }
    return 0;
}
