// Frame::StatisticalOutlierRemovalFilterCloud and GeneralizedICP::mScore of
// include/odo_frontend.hpp (Core/frame.cpp:228-238, Odometry/generalizedicp.cpp:
// 82-87) on two frames read from a file (BGR8 then depth16, frame after frame).
// Prints, per frame, "voxel" and "sor" lines (point count and the position-
// weighted checksum of cloud_mirror.cpp), then "gicp <converged> <mScore as a
// hex float>" for Compute(pF1, pF2, identity) on the filtered clouds and
// "short <converged> <mScore>" for Compute(source, target, guess) on 19-point
// clouds; tests/test_sor_frontend_cpp.py compares them with the Python binding.
//
//   sor_mirror frames.bin width height leaf mean_k stddev iterations max_corr_dist
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
    if (argc != 9) {
        std::fprintf(stderr, "usage: sor_mirror frames.bin width height leaf mean_k stddev iterations max_corr_dist\n");
        return 2;
    }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    const float leaf = (float)std::atof(argv[4]);
    const int mean_k = std::atoi(argv[5]);
    const double stddev = std::atof(argv[6]);
    const size_t px = (size_t)w * h;
    std::vector<uint8_t> bgr(2 * px * 3);
    std::vector<uint16_t> depth(2 * px);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(bgr.data(), 1, bgr.size(), fp) != bgr.size() ||
        std::fread(depth.data(), 2, depth.size(), fp) != depth.size()) {
        std::fprintf(stderr, "sor_mirror: cannot read %s\n", argv[1]);
        return 2;
    }
    std::fclose(fp);
    try {
        odo_hip::Frame f1(bgr.data(), depth.data(), w, h, 0.0), f2(bgr.data() + px * 3, depth.data() + px, w, h, 1.0);
        f1.StatisticalOutlierRemovalFilterCloud(mean_k, stddev);  // no cloud yet: returns (frame.cpp:230)
        if (f1.HasCloud() || !f1.mpCloud.empty()) return 4;
        for (odo_hip::Frame* f : {&f1, &f2}) {
            f->CreateCloud();
            f->VoxelGridFilterCloud(leaf);
            report("voxel", *f);
            f->StatisticalOutlierRemovalFilterCloud(mean_k, stddev);
            report("sor", *f);
        }
        odo_hip::GeneralizedICP gicp(std::atoi(argv[7]), std::atof(argv[8]));
        const bool ok = gicp.Compute(&f1, &f2, odo_hip::Identity());
        std::printf("gicp %d %a\n", (int)ok, gicp.mScore);
        std::vector<float> a, b;
        for (int i = 0; i < 19; i++) {
            const odo_cloud_point &p = f1.mpCloud[(size_t)i], &q = f2.mpCloud[(size_t)i];
            a.insert(a.end(), {p.x, p.y, p.z});
            b.insert(b.end(), {q.x, q.y, q.z});
        }
        const bool short_ok = gicp.Compute(a, b, odo_hip::Identity());
        std::printf("short %d %a\n", (int)short_ok, gicp.mScore);
    } catch (const odo_hip::Error& e) {
        std::fprintf(stderr, "sor_mirror: %s\n", e.what());
        return 3;
    }
    return 0;
}
