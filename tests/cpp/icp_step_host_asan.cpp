// The step header of the point-to-plane ICP (csrc/odo_icp_step.h: the 6 x 6
// Gauss-Jordan solve, the polar factor, the composition) under AddressSanitizer
// and UBSan, stand-alone and without a GPU: the text the device runs, compiled
// for the CPU. Not part of the build or the suite; build and run it by hand on
// a CPU machine:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/cpp/icp_step_host_asan.cpp -o /tmp/icp_step_host_asan && /tmp/icp_step_host_asan
#include "../../adaptive-rgbd-localization-mappig_amd/csrc/odo_icp_step.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #x);      \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    using namespace odo;
    // a solvable system: A = B^T B + I of a fixed B, b = A x
    float B[8][6], A[36], b[6];
    const float x[6] = {0.01f, -0.02f, 0.015f, 0.3f, -0.1f, 0.2f};
    unsigned s = 12345u;
    for (auto& r : B)
        for (float& v : r) {
            s = s * 1664525u + 1013904223u;
            v = (float)(s >> 8) / 16777216.0f - 0.5f;
        }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            float a = i == j ? 1.f : 0.f;
            for (auto& r : B) a += r[i] * r[j];
            A[6 * i + j] = a;
        }
    for (int i = 0; i < 6; i++) {
        b[i] = 0.f;
        for (int j = 0; j < 6; j++) b[i] += A[6 * i + j] * x[j];
    }
    float A1[36], b1[6];
    std::memcpy(A1, A, sizeof A);
    std::memcpy(b1, b, sizeof b);
    EXPECT(icp_solve6(A1, b1));
    for (int i = 0; i < 6; i++) EXPECT(std::fabs(b1[i] - x[i]) < 1e-5f);
    // exactly singular: columns and rows 2-4 zero (a model that is one exact
    // plane), then all zero (an empty active set)
    std::memcpy(A1, A, sizeof A);
    std::memcpy(b1, b, sizeof b);
    for (int i = 0; i < 6; i++)
        for (int j = 2; j < 5; j++) A1[6 * i + j] = A1[6 * j + i] = 0.f;
    EXPECT(!icp_solve6(A1, b1));
    std::memset(A1, 0, sizeof A1);
    std::memset(b1, 0, sizeof b1);
    EXPECT(!icp_solve6(A1, b1));
    // the polar factor: orthonormal, det +1, the rotation about x by atan |x|
    float R_[9];
    icp_polar(x, R_);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double d = 0;
            for (int k = 0; k < 3; k++) d += (double)R_[3 * i + k] * R_[3 * j + k];
            EXPECT(std::fabs(d - (i == j)) < 1e-6);
        }
    const double det = R_[0] * ((double)R_[4] * R_[8] - (double)R_[5] * R_[7]) -
                       R_[1] * ((double)R_[3] * R_[8] - (double)R_[5] * R_[6]) +
                       R_[2] * ((double)R_[3] * R_[7] - (double)R_[4] * R_[6]);
    EXPECT(std::fabs(det - 1.0) < 1e-6);
    const double th = std::sqrt((double)x[0] * x[0] + (double)x[1] * x[1] + (double)x[2] * x[2]);
    EXPECT(std::fabs((R_[0] + (double)R_[4] + R_[8] - 1.0) / 2.0 - std::cos(std::atan(th))) < 1e-6);
    EXPECT(std::fabs((R_[7] - (double)R_[5]) / 2.0 - x[0] / std::sqrt(1.0 + th * th)) < 1e-6);
    const float zero[6] = {0, 0, 0, 0, 0, 0};
    icp_polar(zero, R_);
    for (int i = 0; i < 9; i++) EXPECT(R_[i] == (i % 4 == 0 ? 1.f : 0.f));
    // a composition: a zero step leaves R, t alone with delta 0; a step onto
    // the identity gives R_ | t_ and their norms
    float R[9] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.f, 0.48f, 0.64f, 0.6f}, t[3] = {1.f, -2.f, 3.f};
    float R0[9], t0[3];
    std::memcpy(R0, R, sizeof R);
    std::memcpy(t0, t, sizeof t);
    EXPECT(icp_compose(zero, R, t) == 0.f);
    EXPECT(!std::memcmp(R, R0, sizeof R) && !std::memcmp(t, t0, sizeof t));
    float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tz[3] = {0, 0, 0};
    const float delta = icp_compose(x, I3, tz);
    icp_polar(x, R_);
    EXPECT(!std::memcmp(I3, R_, sizeof R_) && tz[0] == x[3] && tz[1] == x[4] && tz[2] == x[5]);
    EXPECT(std::fabs(delta - std::sqrt(0.3 * 0.3 + 0.1 * 0.1 + 0.2 * 0.2)) < 1e-6);
    std::printf("icp_step_host_asan: ok\n");
    return 0;
}
