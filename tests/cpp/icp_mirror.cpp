// IcpPointToPlane of include/odo_frontend.hpp (Odometry/icp/icpPointToPlane.h)
// on a template and a model read from a file (int32 template count, int32 model
// count, then the float32 x, y, z rows of either). Prints "dim <0|1>" (1: the
// constructor refused dimension 2), then "fit" with the 9 + 3 words of R, t and
// the residual's 64 bits in hex, the inlier count and the inlier ratio's bits;
// tests/test_icp_frontend_cpp.py compares them with the Python binding on the
// same clouds.
//
//   icp_mirror clouds.bin num_neighbors max_iterations min_delta indist
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "odo_frontend.hpp"

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: icp_mirror clouds.bin num_neighbors max_iterations min_delta indist\n");
        return 2;
    }
    int32_t n[2];
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(n, 4, 2, fp) != 2 || n[0] < 0 || n[1] < 0) {
        std::fprintf(stderr, "icp_mirror: cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<float> f(3 * ((size_t)n[0] + n[1]));
    if (std::fread(f.data(), 4, f.size(), fp) != f.size()) {
        std::fprintf(stderr, "icp_mirror: %s is short\n", argv[1]);
        return 2;
    }
    std::fclose(fp);
    std::vector<double> T(f.begin(), f.begin() + 3 * (size_t)n[0]), M(f.begin() + 3 * (size_t)n[0], f.end());
    try {
        bool refused = false;
        try {
            odo_hip::IcpPointToPlane two(M.data(), n[1] * 3 / 2, 2);
        } catch (const odo_hip::Error&) {
            refused = true;
        }
        std::printf("dim %d\n", (int)refused);
        odo_hip::IcpPointToPlane icp(M.data(), n[1], 3, std::atoi(argv[2]), 5.0);
        icp.setMaxIterations(std::atoi(argv[3]));
        icp.setMinDeltaParam(std::atof(argv[4]));
        float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
        const double residual = icp.fit(T.data(), n[0], R, t, std::atof(argv[5])), ratio = icp.getInlierRatio();
        std::printf("fit");
        for (int i = 0; i < 12; i++) {
            uint32_t u;
            std::memcpy(&u, i < 9 ? &R[i] : &t[i - 9], 4);
            std::printf(" %08" PRIx32, u);
        }
        uint64_t r, q;
        std::memcpy(&r, &residual, 8);
        std::memcpy(&q, &ratio, 8);
        std::printf(" %016" PRIx64 " %d %016" PRIx64 " %d %d\n", r, icp.getInlierCount(), q, icp.mLast.iterations,
                    icp.mLast.status);
    } catch (const odo_hip::Error& e) {
        std::fprintf(stderr, "icp_mirror: %s\n", e.what());
        return 3;
    }
    return 0;
}
