// The small dense part of libicp's IcpPointToPlane::fitStep (Odometry/icp/
// icpPointToPlane.cpp:168-205, matrix.cpp:440-535) on floats in the reference's
// operation order, one text for the device (k_icp.hip) and the CPU
// (tests/cpp/icp_step_host_asan.cpp): the 6 x 6 Gauss-Jordan solve with full
// pivoting, the orthonormalised small rotation, the composition R|t = R_|t_ *
// R|t and the step's delta. Build with -ffp-contract=off: every product and
// sum below is rounded as written.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ODO_ICP_HD __host__ __device__
#else
#define ODO_ICP_HD
#endif

namespace odo {

// b_.solve(A_) (matrix.cpp:440-535, eps = 1e-20): A 6 x 6 row-major and b are
// overwritten; on success b holds the solution. The pivot search keeps the
// LAST largest |A[j][k]| (>=), so an all-zero remainder pivots on its last
// entry and fails the singularity test.
ODO_ICP_HD inline bool icp_solve6(float* A, float* b) {
    int ipiv[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 6; i++) {
        float big = 0.f;
        int irow = 0, icol = 0;
        for (int j = 0; j < 6; j++)
            if (ipiv[j] != 1)
                for (int k = 0; k < 6; k++)
                    if (ipiv[k] == 0)
                        if (fabsf(A[6 * j + k]) >= big) {
                            big = fabsf(A[6 * j + k]);
                            irow = j;
                            icol = k;
                        }
        ++ipiv[icol];
        if (irow != icol) {
            for (int l = 0; l < 6; l++) {
                const float s = A[6 * irow + l];
                A[6 * irow + l] = A[6 * icol + l];
                A[6 * icol + l] = s;
            }
            const float s = b[irow];
            b[irow] = b[icol];
            b[icol] = s;
        }
        if (fabsf(A[6 * icol + icol]) < 1e-20f) return false;
        const float pivinv = (float)(1.0 / (double)A[6 * icol + icol]);
        A[6 * icol + icol] = 1.f;
        for (int l = 0; l < 6; l++) A[6 * icol + l] *= pivinv;
        b[icol] *= pivinv;
        for (int ll = 0; ll < 6; ll++)
            if (ll != icol) {
                const float dum = A[6 * ll + icol];
                A[6 * ll + icol] = 0.f;
                for (int l = 0; l < 6; l++) A[6 * ll + l] -= A[6 * icol + l] * dum;
                b[ll] -= b[icol] * dum;
            }
    }
    // the reference unscrambles the columns of A here; b is already in order
    return true;
}

// R_ = U V^T of I + [x0, x1, x2]x (icpPointToPlane.cpp:176-187), the orthogonal
// polar factor, which no choice of SVD changes. For K = [w]x it has the closed
// form c I + c K + c^2 / (1 + c) w w^T with c = 1 / sqrt(1 + |w|^2) (the
// rotation about w by atan |w|; det = 1, so the reference's det < 0 branch is
// dead). Evaluated in double, rounded to float once.
ODO_ICP_HD inline void icp_polar(const float* x, float* R_) {
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double c = 1.0 / sqrt(1.0 + ((w0 * w0 + w1 * w1) + w2 * w2)), k = c * c / (1.0 + c);
    R_[0] = (float)(c + k * w0 * w0);
    R_[1] = (float)(k * w0 * w1 - c * w2);
    R_[2] = (float)(k * w0 * w2 + c * w1);
    R_[3] = (float)(k * w1 * w0 + c * w2);
    R_[4] = (float)(c + k * w1 * w1);
    R_[5] = (float)(k * w1 * w2 - c * w0);
    R_[6] = (float)(k * w2 * w0 - c * w1);
    R_[7] = (float)(k * w2 * w1 + c * w0);
    R_[8] = (float)(c + k * w2 * w2);
}

// a float Matrix product's running sum from 0 (matrix.cpp:284-288)
ODO_ICP_HD inline float icp_dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
    float s = 0.f;
    s += a0 * b0;
    s += a1 * b1;
    s += a2 * b2;
    return s;
}

// From the solution x: R = R_ R, t = R_ t + t_ (float products) and the return
// value max(|R_ - I|_F, |t_|) (Matrix::l2norm: a float running sum, its root)
ODO_ICP_HD inline float icp_compose(const float* x, float* R, float* t) {
    float R_[9], Rn[9], tn[3];
    icp_polar(x, R_);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            Rn[3 * i + j] = icp_dot3(R_[3 * i], R[j], R_[3 * i + 1], R[3 + j], R_[3 * i + 2], R[6 + j]);
    for (int i = 0; i < 3; i++)
        tn[i] = icp_dot3(R_[3 * i], t[0], R_[3 * i + 1], t[1], R_[3 * i + 2], t[2]) + x[3 + i];
    float nr = 0.f, nt = 0.f;
    for (int i = 0; i < 9; i++) {
        const float d = R_[i] - (i % 4 == 0 ? 1.f : 0.f);
        nr += d * d;
    }
    for (int i = 0; i < 3; i++) nt += x[3 + i] * x[3 + i];
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    for (int i = 0; i < 3; i++) t[i] = tn[i];
    const float a = sqrtf(nr), b = sqrtf(nt);
    return a > b ? a : b;
}

}  // namespace odo
