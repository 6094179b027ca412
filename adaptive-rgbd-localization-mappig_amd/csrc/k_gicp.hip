// GeneralizedICP::Compute(source, target, guess) (Odometry/generalizedicp.cpp:
// 30-39, 65-89; the ADAPTIVE_RICP fallback of odometry.cpp:46-78; SURVEY §8(f)
// rank 4): pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> on the GPU.
//   k_gicp_cov  one lane per point: the 20 nearest points of its own cloud
//               (brute force, float squared distances, ties to the lower
//               index), mean / covariance in double, eigenvalues replaced by
//               (1, 1, 1e-3) (computeCovariances);
//   k_gicp      one 4-wave workgroup runs computeTransformation: per ICP iteration the
//               nearest target point of every transformed source point
//               (lane-strided brute force), the Mahalanobis matrices
//               (R C1 R^T + C2)^-1 of the pairs within the distance threshold,
//               compaction in source order (ballot prefix), then
//               estimateRigidTransformationBFGS: BFGS2 + Fletcher's line search
//               with identical control flow on all lanes, the cost and gradient
//               as thread-strided partial sums, the four waves' partials of a
//               lane position added in order, an xor butterfly read on lane 0
//               (oracle/gicp_ref.cpp's sum256), and the convergence test.
// Whole clouds (GeneralizedICP::Compute(pF1, pF2, guess), generalizedicp.cpp:
// 41-53; odo_gicp_grid_batch, odo_gicp_dense) run the same code over a uniform
// grid per cloud instead of the two brute-force scans, with the scans' results
// bit for bit (DESIGN §4 "Dense GICP"):
//   k_gg_*           bounds, cell keys and a counting sort of every cloud into
//                    cell-ordered (x, y, z, index) rows plus cell starts;
//   k_gicp_cov_grid  the 20 neighbours by (distance, index) over Chebyshev rings
//                    of cells, stopped by gg_ring_bound; then cov_finish;
//   k_gicp_grid      k_gicp's body with the correspondence search over the cells
//                    within max_corr_dist of the query.
// The ring walk exists once (gg_walk, a template over a visitor) and also serves
// Frame::StatisticalOutlierRemovalFilterCloud (frame.cpp:228-238) and
// GeneralizedICP::mScore = getFitnessScore() (generalizedicp.cpp:82), DESIGN §4
// "SOR and fitness":
//   k_sor_dist       the mean_k + 1 nearest distances of every point in a per-lane
//                    LDS max-heap, PCL's distances[];
//   k_sor_stats / _mark / _scan / _pack  mean, stddev and threshold per cloud in a
//                    fixed order, the keep bytes, a stable compaction;
//   k_gicp_fit_nn / _sum  the nearest target distance of every transformed source
//                    point without a distance cap, and their mean per pair.
// The restatement, its pinned choices and the oracle are in oracle/gicp_ref.cpp
// (PCL is absent: parity with the library is unpinned).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>

#include "odo_gg_walk.h"
#include "odo_internal.h"
#include "odo_linalg.h"
#include "odo_wave.h"

namespace odo {
namespace {

constexpr int GI_K = 20;
constexpr int GI_LANES = 64;
constexpr int GI_THREADS = 256;  // the ICP / BFGS workgroup: 4 waves share every pass over the correspondences
constexpr int GI_WAVES = GI_THREADS / GI_LANES;
constexpr int GI_NV = 12;        // values reduced per gradient evaluation
constexpr int GI_STAGE = 4096;   // clouds up to this many points are staged in LDS (48 KB)

// computeCovariances from the ordered neighbour list nn[20] of point q on:
// mean and covariance in double, eigenvalues replaced by (1, 1, eps). One piece
// of code for the brute-force and the grid selection.
__device__ __forceinline__ void cov_finish(const float* __restrict__ P, const int* nn, int q, double eps,
                                           double* __restrict__ C) {
    double mean[3] = {0, 0, 0}, cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < GI_K; j++) {
        const float* pt = P + 3 * nn[j];
        const float x = pt[0], y = pt[1], z = pt[2];
        mean[0] += x;
        mean[1] += y;
        mean[2] += z;
        cov[0] += x * x;
        cov[3] += y * x;
        cov[4] += y * y;
        cov[6] += z * x;
        cov[7] += z * y;
        cov[8] += z * z;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) mean[a] /= (double)GI_K;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) {
            cov[a * 3 + b] /= (double)GI_K;
            cov[a * 3 + b] -= mean[a] * mean[b];
            cov[b * 3 + a] = cov[a * 3 + b];
        }
    double w[3], V[9];
    svdj<3, 3>(cov, w, nullptr, V);
    double out[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double v = c == 2 ? eps : 1.;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) out[a * 3 + b] += (v * V[a * 3 + c]) * V[b * 3 + c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) C[9 * q + k] = out[k];
}

// computeCovariances for point q of a cloud P of n points (LDS or global): the
// brute-force selection of the 20 neighbours, then cov_finish
__device__ __forceinline__ void cov_point(const float* __restrict__ P, int n, int q, double eps,
                                          double* __restrict__ C) {
    // the sorted top 20 in registers: +inf padding stands for "fewer than 20
    // so far", a candidate is inserted after equal distances (ties to the lower
    // index, as the scan is in index order)
    float nd[GI_K];
    int nn[GI_K];
#pragma unroll
    for (int j = 0; j < GI_K; j++) {
        nd[j] = __builtin_inff();
        nn[j] = 0;
    }
    const float pq[3] = {P[3 * q], P[3 * q + 1], P[3 * q + 2]};
    for (int i = 0; i < n; i++) {
        const float pi[3] = {P[3 * i], P[3 * i + 1], P[3 * i + 2]};
        const float d = dist2f(pq, pi);
        if (!(d < nd[GI_K - 1])) continue;
#pragma unroll
        for (int j = GI_K - 1; j > 0; j--) {
            const bool up = d < nd[j - 1];
            const bool here = !up && d < nd[j];
            nd[j] = up ? nd[j - 1] : (here ? d : nd[j]);
            nn[j] = up ? nn[j - 1] : (here ? i : nn[j]);
        }
        if (d < nd[0]) {
            nd[0] = d;
            nn[0] = i;
        }
    }
    cov_finish(P, nn, q, eps, C);
}

// grid (point blocks, problems, 2): z = 0 the target clouds, z = 1 the sources
__global__ __launch_bounds__(64) void k_gicp_cov(const float* __restrict__ src, const int* __restrict__ soffs,
                                                 double* __restrict__ Cs, const float* __restrict__ tgt,
                                                 const int* __restrict__ toffs, double* __restrict__ Ct, double eps) {
    const int pb = blockIdx.y;
    const int* offs = blockIdx.z ? soffs : toffs;
    const int n = offs[pb + 1] - offs[pb];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    // whole blocks leave together (the staging below needs every thread)
    if ((int)(blockIdx.x * blockDim.x) >= n || soffs[pb + 1] - soffs[pb] < 20 || toffs[pb + 1] - toffs[pb] < 20) return;
    const float* __restrict__ Pg = (blockIdx.z ? src : tgt) + 3 * (size_t)offs[pb];
    double* __restrict__ C = (blockIdx.z ? Cs : Ct) + 9 * (size_t)offs[pb];
    if (n <= GI_STAGE) {  // the whole cloud in LDS: the scan reads it with uniform addresses
        __shared__ float cst[3 * GI_STAGE];
        for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) cst[i] = Pg[i];
        __syncthreads();
        if (q < n) cov_point(cst, n, q, eps, C);
    } else if (q < n) {
        cov_point(Pg, n, q, eps, C);
    }
}

__device__ void inv3(const double* m, double* r) {
#define M_(i, j) m[(i) * 3 + (j)]
#define COF(i, j) (M_(((i) + 1) % 3, ((j) + 1) % 3) * M_(((i) + 2) % 3, ((j) + 2) % 3) - \
                   M_(((i) + 1) % 3, ((j) + 2) % 3) * M_(((i) + 2) % 3, ((j) + 1) % 3))
    const double c0 = COF(0, 0), c1 = COF(1, 0), c2 = COF(2, 0);
    const double det = sum3d(c0 * M_(0, 0), c1 * M_(1, 0), c2 * M_(2, 0));
    const double invdet = 1.0 / det;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) r[i * 3 + j] = COF(j, i) * invdet;
#undef COF
#undef M_
}

__device__ __forceinline__ void xform4f(const float* T, const float* p, float* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = ((T[4 * i] * p[0] + T[4 * i + 1] * p[1]) + T[4 * i + 2] * p[2]) + T[4 * i + 3];
}

// applyState on the identity base (AngleAxisf Z * Y * X via quaternions)
__device__ void apply_state(const double* x, float* T) {
    float q[3][4];
    const float a[3] = {(float)x[5], (float)x[4], (float)x[3]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float h = 0.5f * a[k];
        const float c = (float)cos((double)h), s = (float)sin((double)h);  // float trig via double (pinned)
        q[k][0] = c;
        q[k][1] = k == 2 ? s : 0.f;
        q[k][2] = k == 1 ? s : 0.f;
        q[k][3] = k == 0 ? s : 0.f;
    }
    auto mul = [](const float* A, const float* B, float* o) {
        o[0] = A[0] * B[0] - A[1] * B[1] - A[2] * B[2] - A[3] * B[3];
        o[1] = A[0] * B[1] + A[1] * B[0] + A[2] * B[3] - A[3] * B[2];
        o[2] = A[0] * B[2] + A[2] * B[0] + A[3] * B[1] - A[1] * B[3];
        o[3] = A[0] * B[3] + A[3] * B[0] + A[1] * B[2] - A[2] * B[1];
    };
    float zy[4], r[4];
    mul(q[0], q[1], zy);
    mul(zy, q[2], r);
    const float w = r[0], qx = r[1], qy = r[2], qz = r[3];
    const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz),
                        tyz - twx,         txz - twy, tyz + twx, 1.f - (txx + tyy)};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
        T[4 * i + 3] = 0.f + (float)x[i];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// oracle/gicp_ref.cpp's sum256: thread t's partial over k = t, t + 256, ...;
// lane l of wave 0 adds the four waves' partials of position l in wave order,
// then an xor butterfly read on lane 0; the NV results are broadcast via LDS.
template <int NV>
__device__ void block_sum256(double* v, double (*red)[GI_THREADS], double* out) {
#pragma unroll
    for (int k = 0; k < NV; k++) red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (threadIdx.x < GI_LANES) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            double z = ((red[k][threadIdx.x] + red[k][threadIdx.x + 64]) + red[k][threadIdx.x + 128]) +
                       red[k][threadIdx.x + 192];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) z += __shfl_xor(z, o, GI_LANES);
            if (threadIdx.x == 0) out[k] = z;
        }
    }
    __syncthreads();
}

struct GiProblem {
    const float* src;  // source after the guess
    const float* tgt;
    const int* is;
    const int* it;
    const double* M;
    int m;
    double (*red)[GI_THREADS];  // LDS [GI_NV][GI_THREADS]
    double* bc;                 // LDS [GI_NV]
};

__device__ double gi_cost(const GiProblem& P, const double* x) {
    float T[16];
    apply_state(x, T);
    double part = 0.0;
    for (int k = threadIdx.x; k < P.m; k += GI_THREADS) {
        const int si = P.is[k];
        const float ps[3] = {P.src[3 * si], P.src[3 * si + 1], P.src[3 * si + 2]};
        float pp[3];
        xform4f(T, ps, pp);
        const float* q = P.tgt + 3 * P.it[k];
        const double r[3] = {(double)(pp[0] - q[0]), (double)(pp[1] - q[1]), (double)(pp[2] - q[2])};
        const double* M = P.M + 9 * si;
        double t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = sum3d(M[3 * i] * r[0], M[3 * i + 1] * r[1], M[3 * i + 2] * r[2]);
        part += sum3d(r[0] * t[0], r[1] * t[1], r[2] * t[2]);
    }
    block_sum256<1>(&part, P.red, P.bc);
    return P.bc[0] / P.m;
}

__device__ void gi_grad(const GiProblem& P, const double* x, double* g) {
    float T[16];
    apply_state(x, T);
    double part[12];
#pragma unroll
    for (int i = 0; i < 12; i++) part[i] = 0.0;
    for (int k = threadIdx.x; k < P.m; k += GI_THREADS) {
        const int si = P.is[k];
        const float ps[3] = {P.src[3 * si], P.src[3 * si + 1], P.src[3 * si + 2]};
        float pp[3];
        xform4f(T, ps, pp);
        const float* q = P.tgt + 3 * P.it[k];
        const double r[3] = {(double)(pp[0] - q[0]), (double)(pp[1] - q[1]), (double)(pp[2] - q[2])};
        const double* M = P.M + 9 * si;
        double t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = sum3d(M[3 * i] * r[0], M[3 * i + 1] * r[1], M[3 * i + 2] * r[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) part[i] += t[i];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) part[3 + 3 * a + b] += (double)ps[a] * t[b];
    }
    double Rm[9];
    block_sum256<GI_NV>(part, P.red, P.bc);
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = P.bc[i] * (2.0 / P.m);
#pragma unroll
    for (int i = 0; i < 9; i++) Rm[i] = P.bc[3 + i] * (2.0 / P.m);
    const double phi = x[3], theta = x[4], psi = x[5];
    const double cphi = cos(phi), sphi = sin(phi), ctheta = cos(theta), stheta = sin(theta), cpsi = cos(psi),
                 spsi = sin(psi);
    const double d[3][9] = {{0., sphi * spsi + cphi * cpsi * stheta, cphi * spsi - cpsi * sphi * stheta,
                             0., -cpsi * sphi + cphi * spsi * stheta, -cphi * cpsi - sphi * spsi * stheta,
                             0., cphi * ctheta, -ctheta * sphi},
                            {-cpsi * stheta, cpsi * ctheta * sphi, cphi * cpsi * ctheta,
                             -spsi * stheta, ctheta * sphi * spsi, cphi * ctheta * spsi,
                             -ctheta, -sphi * stheta, -cphi * stheta},
                            {-ctheta * spsi, -cphi * cpsi - sphi * spsi * stheta, cpsi * sphi - cphi * spsi * stheta,
                             cpsi * ctheta, -cphi * spsi + cpsi * sphi * stheta, sphi * spsi + cphi * cpsi * stheta,
                             0., 0., 0.}};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double r = 0.;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) r += d[c][3 * j + i] * Rm[3 * i + j];
        g[3 + c] = r;
    }
}

enum { ST_NOT_STARTED = -2, ST_RUNNING = -1, ST_SUCCESS = 0, ST_NO_PROGRESS = 1 };

// bfgs.h on every lane of the wave (uniform control flow, wave-summed values)
struct GiBfgs {
    GiProblem P;
    double x0[6], p[6], g0[6], dx0[6], dg0[6], gradient[6];
    double f, fp0, g0norm, pnorm, delta_f;
    double x_alpha[6], g_alpha[6], f_alpha, df_alpha, f_key, g_key, df_key;

    __device__ static double dot6(const double* a, const double* b) {
        double s = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) s += a[i] * b[i];
        return s;
    }
    __device__ static double norm6(const double* a) { return sqrt(dot6(a, a)); }
    __device__ void moveTo(double alpha) {
#pragma unroll
        for (int i = 0; i < 6; i++) x_alpha[i] = x0[i] + alpha * p[i];
    }
    __device__ double slope() { return dot6(g_alpha, p); }
    __device__ double applyF(double alpha) {
        if (alpha == f_key) return f_alpha;
        moveTo(alpha);
        f_alpha = gi_cost(P, x_alpha);
        f_key = alpha;
        return f_alpha;
    }
    __device__ double applyDF(double alpha) {
        if (alpha == df_key) return df_alpha;
        moveTo(alpha);
        if (alpha != g_key) {
            gi_grad(P, x_alpha, g_alpha);
            g_key = alpha;
        }
        df_alpha = slope();
        df_key = alpha;
        return df_alpha;
    }
    __device__ static double cubic(double c0, double c1, double c2, double c3, double z) {
        return c0 + z * (c1 + z * (c2 + z * c3));
    }
    __device__ static void checkExtremum(double c0, double c1, double c2, double c3, double x, double& xmin,
                                         double& fmin) {
        const double y = cubic(c0, c1, c2, c3, x);
        if (y < fmin) {
            xmin = x;
            fmin = y;
        }
    }
    __device__ static int solve_quadratic(double a, double b, double c, double* x0, double* x1) {
        if (a == 0) {
            if (b == 0) return 0;
            *x0 = -c / b;
            return 1;
        }
        const double disc = b * b - 4 * a * c;
        if (disc > 0) {
            if (b == 0) {
                const double r = sqrt(-c / a);
                *x0 = -r;
                *x1 = r;
            } else {
                const double sgnb = (b > 0 ? 1 : -1);
                const double temp = -0.5 * (b + sgnb * sqrt(disc));
                const double r1 = temp / a, r2 = c / temp;
                if (r1 < r2) {
                    *x0 = r1;
                    *x1 = r2;
                } else {
                    *x0 = r2;
                    *x1 = r1;
                }
            }
            return 2;
        } else if (disc == 0) {
            *x0 = -0.5 * b / a;
            *x1 = -0.5 * b / a;
            return 2;
        }
        return 0;
    }
    __device__ static double cubicInterp(double f0, double fp0, double f1, double fp1, double zl, double zh) {
        const double eta = 3 * (f1 - f0) - 2 * fp0 - fp1;
        const double xi = fp0 + fp1 - 2 * (f1 - f0);
        const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
        double zmin = zl, fmin = cubic(c0, c1, c2, c3, zl);
        checkExtremum(c0, c1, c2, c3, zh, zmin, fmin);
        double z0 = 0, z1 = 0;
        const int n = solve_quadratic(3 * c3, 2 * c2, c1, &z0, &z1);
        if (n == 2) {
            if (z0 > zl && z0 < zh) checkExtremum(c0, c1, c2, c3, z0, zmin, fmin);
            if (z1 > zl && z1 < zh) checkExtremum(c0, c1, c2, c3, z1, zmin, fmin);
        } else if (n == 1) {
            if (z0 > zl && z0 < zh) checkExtremum(c0, c1, c2, c3, z0, zmin, fmin);
        }
        return zmin;
    }
    __device__ static double quadraticInterp(double f0, double fp0, double f1, double zl, double zh) {
        const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
        const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
        const double c = 2 * (f1 - f0 - fp0);
        double zmin = zl, fmin = fl;
        if (fh < fmin) {
            zmin = zh;
            fmin = fh;
        }
        if (c > 0) {
            const double z = -fp0 / c;
            if (z > zl && z < zh) {
                const double ff = f0 + z * (fp0 + z * (f1 - f0 - fp0));
                if (ff < fmin) {
                    zmin = z;
                    fmin = ff;
                }
            }
        }
        return zmin;
    }
    __device__ static double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin,
                                         double xmax) {
        double zmin = (xmin - a) / (b - a), zmax = (xmax - a) / (b - a);
        if (zmin > zmax) {
            const double t = zmin;
            zmin = zmax;
            zmax = t;
        }
        double z;
        if (!isnan(fpb))  // order 3
            z = cubicInterp(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax);
        else
            z = quadraticInterp(fa, fpa * (b - a), fb, zmin, zmax);
        return a + z * (b - a);
    }
    __device__ int lineSearch(double alpha1, double* alpha_new) {
        const double rho = 0.01, sigma = 0.01, tau1 = 9, tau2 = 0.05, tau3 = 0.5;
        double falpha, fpalpha, delta, alpha_next;
        double alpha = alpha1, alpha_prev = 0.0;
        int i = 0;
        const double f0 = applyF(0.0), fp0l = applyDF(0.0);
        double falpha_prev = f0, fpalpha_prev = fp0l;
        double a = 0.0, b = alpha, fa = f0, fb = 0.0, fpa = fp0l, fpb = 0.0;
        const double qnan = __builtin_nan("");
        while (i++ < 100) {
            falpha = applyF(alpha);
            if (falpha > f0 + alpha * rho * fp0l || falpha >= falpha_prev) {
                a = alpha_prev;
                fa = falpha_prev;
                fpa = fpalpha_prev;
                b = alpha;
                fb = falpha;
                fpb = qnan;
                break;
            }
            fpalpha = applyDF(alpha);
            if (fabs(fpalpha) <= -sigma * fp0l) {
                *alpha_new = alpha;
                return ST_SUCCESS;
            }
            if (fpalpha >= 0) {
                a = alpha;
                fa = falpha;
                fpa = fpalpha;
                b = alpha_prev;
                fb = falpha_prev;
                fpb = fpalpha_prev;
                break;
            }
            delta = alpha - alpha_prev;
            alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta,
                                     alpha + tau1 * delta);
            alpha_prev = alpha;
            falpha_prev = falpha;
            fpalpha_prev = fpalpha;
            alpha = alpha_next;
        }
        while (i++ < 100) {
            delta = b - a;
            alpha = interpolate(a, fa, fpa, b, fb, fpb, a + tau2 * delta, b - tau3 * delta);
            falpha = applyF(alpha);
            if ((a - alpha) * fpa <= DBL_EPSILON) return ST_NO_PROGRESS;
            if (falpha > f0 + rho * alpha * fp0l || falpha >= fa) {
                b = alpha;
                fb = falpha;
                fpb = qnan;
            } else {
                fpalpha = applyDF(alpha);
                if (fabs(fpalpha) <= -sigma * fp0l) {
                    *alpha_new = alpha;
                    return ST_SUCCESS;
                }
                if (((b - a) >= 0 && fpalpha >= 0) || ((b - a) <= 0 && fpalpha <= 0)) {
                    b = a;
                    fb = fa;
                    fpb = fpa;
                    a = alpha;
                    fa = falpha;
                    fpa = fpalpha;
                } else {
                    a = alpha;
                    fa = falpha;
                    fpa = fpalpha;
                }
            }
        }
        return ST_SUCCESS;
    }
    __device__ void minimizeInit(const double* x) {
        delta_f = 0;
        f = gi_cost(P, x);
        gi_grad(P, x, gradient);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            x0[i] = x[i];
            g0[i] = gradient[i];
        }
        g0norm = norm6(g0);
#pragma unroll
        for (int i = 0; i < 6; i++) p[i] = gradient[i] * (-1 / g0norm);
        pnorm = norm6(p);
        fp0 = -g0norm;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            x_alpha[i] = x0[i];
            g_alpha[i] = g0[i];
        }
        f_alpha = f;
        f_key = 0;
        g_key = 0;
        df_alpha = slope();
        df_key = 0;
    }
    __device__ int minimizeOneStep(double* x) {
        double alpha = 0.0, alpha1;
        const double f0 = f;
        if (pnorm == 0.0 || g0norm == 0.0 || fp0 == 0) return ST_NOT_STARTED;
        if (delta_f < 0) {
            const double del = fmax(-delta_f, 10 * DBL_EPSILON * fabs(f0));
            alpha1 = fmin(1.0, 2.0 * del / (-fp0));
        } else {
            alpha1 = 1.0;  // |step_size|
        }
        const int st = lineSearch(alpha1, &alpha);
        if (st != ST_SUCCESS) return st;
        applyF(alpha);  // updatePosition
        applyDF(alpha);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            x[i] = x_alpha[i];
            gradient[i] = g_alpha[i];
        }
        f = f_alpha;
        delta_f = f - f0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            dx0[i] = x[i] - x0[i];
            dg0[i] = gradient[i] - g0[i];
        }
        const double dxg = dot6(dx0, gradient), dgg = dot6(dg0, gradient), dxdg = dot6(dx0, dg0);
        const double dgnorm = norm6(dg0);
        double A, B;
        if (dxdg != 0) {
            B = dxg / dxdg;
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
        } else {
            B = 0;
            A = 0;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) p[i] = (gradient[i] + (-A) * dx0[i]) + (-B) * dg0[i];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            g0[i] = gradient[i];
            x0[i] = x[i];
        }
        g0norm = norm6(g0);
        pnorm = norm6(p);
        const double dir = (dot6(p, gradient) >= 0.0) ? -1.0 : +1.0;
#pragma unroll
        for (int i = 0; i < 6; i++) p[i] *= dir / pnorm;
        pnorm = norm6(p);
        fp0 = dot6(p, g0);
#pragma unroll
        for (int i = 0; i < 6; i++) {  // changeDirection
            x_alpha[i] = x0[i];
            g_alpha[i] = g0[i];
        }
        f_key = 0.0;
        g_key = 0.0;
        df_alpha = slope();
        df_key = 0.0;
        return ST_SUCCESS;
    }
};

// out[4]: converged, iterations, n_corr, (pad); T12[16]
// nearest point of T (n points, LDS or global) to q: strict <, ties to the lower index
__device__ __forceinline__ int nn_search(const float* __restrict__ T, int n, const float* q, float* bdo) {
    float bd = dist2f(q, T);
    int best = 0;
    for (int j = 1; j < n; j++) {
        const float tj[3] = {T[3 * j], T[3 * j + 1], T[3 * j + 2]};
        const float d = dist2f(q, tj);
        if (d < bd) {
            bd = d;
            best = j;
        }
    }
    *bdo = bd;
    return best;
}

struct BruteSearch {
    const float* tgt;
    int nt;
    __device__ __forceinline__ int operator()(const float* q, float* bd) const { return nn_search(tgt, nt, q, bd); }
};

// computeTransformation of one problem on its workgroup. Every pointer is the
// problem's own (source, target and their covariances; outp, Mah, is, it sized
// by the source). The correspondence search is the policy: search(q, &d)
// returns the target point nearest to q, the lowest index among equals, and
// its float squared distance (+inf when it looked at no point).
template <class Search>
__device__ __forceinline__ void gicp_body(const float* __restrict__ src, int ns, const float* __restrict__ tgt,
                                          int nt, const double* __restrict__ Cs, const double* __restrict__ Ct,
                                          float* __restrict__ outp, double* __restrict__ Mah, int* __restrict__ is,
                                          int* __restrict__ it, const float* __restrict__ guess,
                                          double max_corr_dist, int max_iterations, int max_inner,
                                          float* __restrict__ T12, int* __restrict__ outi, const Search& search) {
    __shared__ double red[GI_NV][GI_THREADS];
    __shared__ double bc[GI_NV];
    __shared__ int wcnt[GI_WAVES];
    const int lane = threadIdx.x & (GI_LANES - 1), wave = threadIdx.x / GI_LANES;
    if (ns < 20 || nt < 20) {  // generalizedicp.cpp:33
        if (threadIdx.x < 16) T12[threadIdx.x] = threadIdx.x % 5 == 0 ? 1.f : 0.f;
        if (threadIdx.x < 4) outi[threadIdx.x] = 0;
        return;
    }
    for (int i = threadIdx.x; i < ns; i += GI_THREADS) {  // transformPointCloud(output, output, guess)
        const float p0 = src[3 * i], p1 = src[3 * i + 1], p2 = src[3 * i + 2];
#pragma unroll
        for (int r = 0; r < 3; r++)
            outp[3 * i + r] = guess[4 * r] * p0 + guess[4 * r + 1] * p1 + guess[4 * r + 2] * p2 + guess[4 * r + 3];
    }
    __syncthreads();
    float Tcur[16], Tprev[16];
#pragma unroll
    for (int i = 0; i < 16; i++) Tcur[i] = Tprev[i] = i % 5 == 0 ? 1.f : 0.f;
    const double dist_threshold = max_corr_dist * max_corr_dist;
    int nr_iterations = 0, conv = 0, ncorr = 0;
    while (!conv) {
        double R[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) s += double(Tcur[4 * i + k]) * double(guess[4 * k + j]);
                R[3 * i + j] = s;
            }
        int base = 0;
        for (int i0 = 0; i0 < ns; i0 += GI_THREADS) {
            const int i = i0 + threadIdx.x;
            bool hit = false;
            int best = 0;
            if (i < ns) {
                const float pi[3] = {outp[3 * i], outp[3 * i + 1], outp[3 * i + 2]};
                float q[3];
                xform4f(Tcur, pi, q);
                float bd;
                best = search(q, &bd);  // (brute force: an LDS-staged target measured no faster)
                if ((double)bd < dist_threshold) {
                    hit = true;
                    const double* C1 = Cs + 9 * i;
                    const double* C2 = Ct + 9 * best;
                    double M[9], tmp[9];
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int b = 0; b < 3; b++)
                            M[3 * a + b] = sum3d(R[3 * a] * C1[b], R[3 * a + 1] * C1[3 + b], R[3 * a + 2] * C1[6 + b]);
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int b = 0; b < 3; b++) {
                            tmp[3 * a + b] = sum3d(M[3 * a] * R[3 * b], M[3 * a + 1] * R[3 * b + 1], M[3 * a + 2] * R[3 * b + 2]);
                            tmp[3 * a + b] += C2[3 * a + b];
                        }
                    double Mi[9];
                    inv3(tmp, Mi);
#pragma unroll
                    for (int k = 0; k < 9; k++) Mah[9 * i + k] = Mi[k];
                }
            }
            // compaction in source order: ballot within the wave, wave counts in order
            const uint64_t bal = __ballot(hit);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int pre = base, tot = 0;
#pragma unroll
            for (int w = 0; w < GI_WAVES; w++) {
                if (w < wave) pre += wcnt[w];
                tot += wcnt[w];
            }
            const int pos = pre + lane_rank(bal);
            if (hit) {
                is[pos] = i;
                it[pos] = best;
            }
            base += tot;
            __syncthreads();
        }
        __threadfence_block();
        __syncthreads();
        ncorr = base;
#pragma unroll
        for (int i = 0; i < 16; i++) Tprev[i] = Tcur[i];
        if (base < 4) break;  // NotEnoughPointsException: caught, not converged
        double x[6] = {Tcur[3], Tcur[7], Tcur[11], (double)(float)atan2((double)Tcur[9], (double)Tcur[10]), (double)(float)asin(-(double)Tcur[8]),
                       (double)(float)atan2((double)Tcur[4], (double)Tcur[0])};
        GiBfgs bf;
        bf.P = GiProblem{outp, tgt, is, it, Mah, base, red, bc};
        bf.minimizeInit(x);
        int inner = 0, result;
        do {
            inner++;
            result = bf.minimizeOneStep(x);
            if (result) break;
            double gn = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) gn += bf.gradient[k] * bf.gradient[k];
            result = sqrt(gn) < 1e-2 ? ST_SUCCESS : ST_RUNNING;
        } while (result == ST_RUNNING && inner < max_inner);
        if (!(result == ST_NO_PROGRESS || result == ST_SUCCESS || inner == max_inner)) break;
        apply_state(x, Tcur);
        double delta = 0.;
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int l = 0; l < 4; l++) {
                const double ratio = (k < 3 && l < 3) ? 1. / 2e-3 : 1. / 1e-9;
                const double c_delta = ratio * fabsf(Tprev[4 * k + l] - Tcur[4 * k + l]);
                if (c_delta > delta) delta = c_delta;
            }
        nr_iterations++;
        if (nr_iterations >= max_iterations || delta < 1) {
            conv = 1;
#pragma unroll
            for (int i = 0; i < 16; i++) Tprev[i] = Tcur[i];
        }
    }
    if (threadIdx.x == 0) {
        outi[0] = conv;
        outi[1] = nr_iterations;
        outi[2] = ncorr;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                T12[4 * i + j] = conv ? ((Tprev[4 * i] * guess[j] + Tprev[4 * i + 1] * guess[4 + j]) +
                                         Tprev[4 * i + 2] * guess[8 + j]) + Tprev[4 * i + 3] * guess[12 + j]
                                      : (i == j ? 1.f : 0.f);
    }
}

// one workgroup per problem of the batch
__global__ __launch_bounds__(GI_THREADS) void k_gicp(const float* __restrict__ src, const float* __restrict__ tgt,
                                                   const double* __restrict__ Cs, const double* __restrict__ Ct,
                                                   float* __restrict__ outp, double* __restrict__ Mah,
                                                   int* __restrict__ is, int* __restrict__ it, GicpArgs A,
                                                   float* __restrict__ T12, int* __restrict__ outi) {
    const int pb = blockIdx.x;
    const int s0 = A.soffs[pb], t0 = A.toffs[pb];
    const int ns = A.soffs[pb + 1] - s0, nt = A.toffs[pb + 1] - t0;
    tgt += 3 * (size_t)t0;
    gicp_body(src + 3 * (size_t)s0, ns, tgt, nt, Cs + 9 * (size_t)s0, Ct + 9 * (size_t)t0, outp + 3 * (size_t)s0,
              Mah + 9 * (size_t)s0, is + s0, it + s0, A.guess + 16 * pb, A.max_corr_dist, A.max_iterations,
              A.max_inner, T12 + 16 * pb, outi + 4 * pb, BruteSearch{tgt, nt});
}

// ------------------------------------------------------------------ the grid
// (DESIGN §4 "Dense GICP"; GgCloud in odo_internal.h)
constexpr int GG_CHUNK = 4096;  // cells per scan workgroup, points per bounds workgroup

// grid (point blocks, clouds)
__global__ __launch_bounds__(256) void k_gg_pack(const float* __restrict__ src, int stride,
                                                 const int* __restrict__ row0, const int* __restrict__ offs,
                                                 float* __restrict__ dst) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= offs[k + 1] - offs[k]) return;
    const float* s = src + (size_t)stride * ((size_t)row0[k] + i);
    float* d = dst + 3 * ((size_t)offs[k] + i);
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
}

// grid (GG_CHUNK-point blocks, clouds): min and max are exact in any order
__global__ __launch_bounds__(256) void k_gg_bounds(const float* __restrict__ P, const int* __restrict__ offs,
                                                   uint32_t* __restrict__ bounds) {
    const int k = blockIdx.y, n = offs[k + 1] - offs[k];
    const int i0 = blockIdx.x * GG_CHUNK;
    if (i0 >= n) return;
    const float* Pk = P + 3 * (size_t)offs[k];
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const int i1 = min(n, i0 + GG_CHUNK);
    for (int i = i0 + threadIdx.x; i < i1; i += 256)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = Pk[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, GI_LANES));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, GI_LANES));
        }
    if ((threadIdx.x & (GI_LANES - 1)) == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(&bounds[6 * k + a], f32_ordered(mn[a]));
            atomicMax(&bounds[6 * k + 3 + a], f32_ordered(mx[a]));
        }
}

// grid (point blocks, clouds): the cell of every point and the cells' counts
__global__ __launch_bounds__(256) void k_gg_count(const float* __restrict__ P, const GgCloud* __restrict__ cl,
                                                  int* __restrict__ key, int* __restrict__ cnt) {
    const GgCloud g = cl[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const size_t row = (size_t)g.p0 + i;
    const float p[3] = {P[3 * row], P[3 * row + 1], P[3 * row + 2]};
    int c[3];
    gg_cell3(g, p, c);
    const int cell = (c[2] * g.gy + c[1]) * g.gx + c[0];
    key[row] = cell;
    atomicAdd(&cnt[g.c0 + cell], 1);
}

// exclusive scan in place of this thread's items [begin, end) within the
// workgroup's; returns the workgroup's total
__device__ int gg_block_scan(int* __restrict__ a, int begin, int end) {
    __shared__ int ws[256];
    int s = 0;
    for (int i = begin; i < end; i++) s += a[i];
    ws[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = (int)threadIdx.x >= o ? ws[threadIdx.x - o] : 0;
        __syncthreads();
        ws[threadIdx.x] += v;
        __syncthreads();
    }
    int run = ws[threadIdx.x] - s;
    for (int i = begin; i < end; i++) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    return ws[255];
}

// the counting sort's scan over the m entries of all clouds: chunks, the chunk
// totals (one workgroup), and the totals added back
__global__ __launch_bounds__(256) void k_gg_scan_chunks(int* __restrict__ a, int m, int* __restrict__ bsum) {
    const int per = GG_CHUNK / 256;
    const int begin = min(m, (int)blockIdx.x * GG_CHUNK + (int)threadIdx.x * per), end = min(m, begin + per);
    const int tot = gg_block_scan(a, begin, end);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_gg_scan_tops(int* __restrict__ bsum, int nb) {
    const int per = (nb + 255) / 256;
    const int begin = min(nb, (int)threadIdx.x * per), end = min(nb, begin + per);
    (void)gg_block_scan(bsum, begin, end);
}
__global__ __launch_bounds__(256) void k_gg_scan_add(int* __restrict__ a, int m, const int* __restrict__ bsum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) a[i] += bsum[i / GG_CHUNK];
}

// grid (point blocks, clouds): the order within a cell is the atomics' (no
// result depends on it: every selection compares (distance, index))
__global__ __launch_bounds__(256) void k_gg_scatter(const float* __restrict__ P, const GgCloud* __restrict__ cl,
                                                    const int* __restrict__ key, const int* __restrict__ cstart,
                                                    int* __restrict__ fill, float4* __restrict__ sorted) {
    const GgCloud g = cl[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const size_t row = (size_t)g.p0 + i;
    const int cell = g.c0 + key[row];
    const int pos = cstart[cell] + atomicAdd(&fill[cell], 1);
    sorted[pos] = make_float4(P[3 * row], P[3 * row + 1], P[3 * row + 2], __int_as_float(i));
}

// (the ring walk gg_walk: odo_gg_walk.h)

// the covariance neighbours: the top 20 by (distance, index) in registers
// (an unrolled insertion list; as cov_point: +inf padding, whose index 0 no
// candidate goes below)
struct CovTop20 {
    float pq[3];
    float nd[GI_K];
    int nn[GI_K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < GI_K; j++) {
            nd[j] = __builtin_inff();
            nn[j] = 0;
        }
    }
    __device__ __forceinline__ void visit(const float4 t) {
        const float pi[3] = {t.x, t.y, t.z};
        const int idx = __float_as_int(t.w);
        const float d = dist2f(pq, pi);
#define GG_LT(j) (d < nd[j] || (d == nd[j] && idx < nn[j]))
        if (!GG_LT(GI_K - 1)) return;
#pragma unroll
        for (int j = GI_K - 1; j > 0; j--) {
            const bool up = GG_LT(j - 1);
            const bool here = !up && GG_LT(j);
            nd[j] = up ? nd[j - 1] : (here ? d : nd[j]);
            nn[j] = up ? nn[j - 1] : (here ? idx : nn[j]);
        }
        if (GG_LT(0)) {
            nd[0] = d;
            nn[0] = idx;
        }
#undef GG_LT
    }
    __device__ __forceinline__ float kth() const { return nd[GI_K - 1]; }
};

// grid (point blocks, clouds): one lane per point, in cell order, so that a
// wave walks the same cells. The top 20 by (distance, index) over the ring walk.
__global__ __launch_bounds__(64) void k_gicp_cov_grid(const float* __restrict__ P, const GgCloud* __restrict__ cl,
                                                      const int* __restrict__ cstart,
                                                      const float4* __restrict__ sorted, double* __restrict__ C,
                                                      double eps) {
    const GgCloud g = cl[blockIdx.y];
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (g.n < 20 || s >= g.n) return;
    const float4 me = sorted[(size_t)g.p0 + s];
    CovTop20 v;
    v.pq[0] = me.x;
    v.pq[1] = me.y;
    v.pq[2] = me.z;
    v.init();
    int c[3];
    gg_cell3(g, v.pq, c);
    gg_walk(g, cstart + g.c0, sorted, c, v);
    cov_finish(P + 3 * (size_t)g.p0, v.nn, __float_as_int(me.w), eps, C + 9 * (size_t)g.p0);
}

// ------------------------------------------------- SOR and the fitness score
// (DESIGN §4 "SOR and fitness") k nearest float squared distances, no indices:
// a max-heap of k floats per lane in LDS, entry j of lane l at h[j * 64 + l]
// (a lane's entries are a bank apart from its neighbours': no conflicts). The
// heap holds the k smallest distances seen whatever their order of arrival.
struct DistHeap {
    float pq[3];
    float* h;  // this lane's entry 0
    int k;
    __device__ __forceinline__ float& at(int j) const { return h[j * GI_LANES]; }
    // entry 0 replaced by d, sifted down within the first m entries
    __device__ __forceinline__ void sift(float d, int m) {
        int i = 0;
        for (;;) {
            const int l = 2 * i + 1;
            if (l >= m) break;
            const float hl = at(l), hr = l + 1 < m ? at(l + 1) : -1.f;  // distances are >= 0
            const float hm = fmaxf(hl, hr);
            if (!(hm > d)) break;
            at(i) = hm;
            i = hr > hl ? l + 1 : l;
        }
        at(i) = d;
    }
    __device__ __forceinline__ void visit(const float4 t) {
        const float pi[3] = {t.x, t.y, t.z};
        const float d = dist2f(pq, pi);
        if (d < at(0)) sift(d, k);
    }
    __device__ __forceinline__ float kth() const { return at(0); }
};

// grid (point blocks, clouds), LDS 64 * (mean_k + 1) floats: PCL's
// StatisticalOutlierRemoval distances[] of every cloud of more than mean_k
// points, in point order (include/odo.h odo_cloud_sor_batch)
__global__ __launch_bounds__(64) void k_sor_dist(const GgCloud* __restrict__ cl, const int* __restrict__ cstart,
                                                 const float4* __restrict__ sorted, int mean_k,
                                                 float* __restrict__ dist) {
    extern __shared__ float sor_heap[];
    const GgCloud g = cl[blockIdx.y];
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (g.n <= mean_k || s >= g.n) return;
    const float4 me = sorted[(size_t)g.p0 + s];
    DistHeap v;
    v.pq[0] = me.x;
    v.pq[1] = me.y;
    v.pq[2] = me.z;
    v.h = sor_heap + threadIdx.x;
    v.k = mean_k + 1;
    for (int j = 0; j < v.k; j++) v.at(j) = __builtin_inff();
    int c[3];
    gg_cell3(g, v.pq, c);
    gg_walk(g, cstart + g.c0, sorted, c, v);
    // heap sort: ascending in entries 0 ... k - 1
    for (int m = v.k - 1; m >= 1; m--) {
        const float last = v.at(m);
        v.at(m) = v.at(0);
        v.sift(last, m);
    }
    double sum = 0;  // entry 0 is dropped, as PCL drops nn_dists[0]
    // sqrtf is the correctly rounded root (hipcc's default); __fsqrt_rn is the native approximation here
    for (int j = 1; j < v.k; j++) sum += (double)sqrtf(v.at(j));
    dist[(size_t)g.p0 + __float_as_int(me.w)] = (float)(sum / (double)mean_k);
}

// one workgroup per cloud: sum and sq_sum over thread-strided partials and
// block_sum256's fixed order, then PCL's mean, variance, stddev, threshold
__global__ __launch_bounds__(GI_THREADS) void k_sor_stats(const GgCloud* __restrict__ cl,
                                                          const float* __restrict__ dist, int mean_k,
                                                          double stddev_mul, SorStats* __restrict__ st) {
    __shared__ double red[2][GI_THREADS];
    __shared__ double out[2];
    const GgCloud g = cl[blockIdx.x];
    if (g.n <= mean_k) return;  // skipped: the host preset st
    double v[2] = {0, 0};
    for (int i = threadIdx.x; i < g.n; i += GI_THREADS) {
        const float d = dist[(size_t)g.p0 + i];
        v[0] += (double)d;
        v[1] += (double)(d * d);  // the product in float, as PCL's vector<float> arithmetic
    }
    block_sum256<2>(v, red, out);
    if (threadIdx.x) return;
    const double n = (double)g.n, sum = out[0], sq = out[1];
    const double mean = sum / n, var = (sq - sum * sum / n) / (n - 1.0), sd = sqrt(var);
    SorStats r;
    r.sum = sum;
    r.sq_sum = sq;
    r.mean = mean;
    r.stddev = sd;
    r.threshold = mean + stddev_mul * sd;
    r.n_out = 0;
    r.pad = 0;
    st[blockIdx.x] = r;
}

// grid (256-point chunks, clouds): the keep byte of every point (a NaN
// threshold keeps all) and the chunk's kept count
__global__ __launch_bounds__(256) void k_sor_mark(const GgCloud* __restrict__ cl, const float* __restrict__ dist,
                                                  const SorStats* __restrict__ st, int mean_k, int nchunk,
                                                  uint8_t* __restrict__ keep, int* __restrict__ chunk_cnt) {
    const GgCloud g = cl[blockIdx.y];
    if ((int)blockIdx.x * 256 >= g.n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int k = 0;
    if (i < g.n) {
        k = g.n <= mean_k || !((double)dist[(size_t)g.p0 + i] > st[blockIdx.y].threshold);
        keep[(size_t)g.p0 + i] = (uint8_t)k;
    }
    const int tot = __syncthreads_count(k);
    if (threadIdx.x == 0) chunk_cnt[(size_t)blockIdx.y * nchunk + blockIdx.x] = tot;
}

// one workgroup per cloud: the chunk counts become the chunks' first kept
// ranks, their total is n_out
__global__ __launch_bounds__(256) void k_sor_scan(const GgCloud* __restrict__ cl, int nchunk,
                                                  int* __restrict__ chunk_cnt, SorStats* __restrict__ st) {
    const int m = (cl[blockIdx.x].n + 255) / 256;
    const int per = (m + 255) / 256;
    const int begin = min(m, (int)threadIdx.x * per), end = min(m, begin + per);
    const int tot = gg_block_scan(chunk_cnt + (size_t)blockIdx.x * nchunk, begin, end);
    if (threadIdx.x == 0) st[blockIdx.x].n_out = tot;
}

// grid (256-point chunks, clouds): the kept rows of cloud k (16-byte points at
// pts + row0[k], their counts alike) in order to rows new0[k] ... of the copies
__global__ __launch_bounds__(256) void k_sor_pack(const GgCloud* __restrict__ cl, const uint8_t* __restrict__ keep,
                                                  const int* __restrict__ chunk_cnt, int nchunk,
                                                  const int* __restrict__ row0, const int* __restrict__ new0,
                                                  const uint4* __restrict__ pts, const int* __restrict__ counts,
                                                  uint4* __restrict__ pts_out, int* __restrict__ counts_out) {
    __shared__ int wsum[4];
    const GgCloud g = cl[blockIdx.y];
    if ((int)blockIdx.x * 256 >= g.n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int k = i < g.n ? keep[(size_t)g.p0 + i] : 0;
    const uint64_t b = __ballot(k);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int rank = chunk_cnt[(size_t)blockIdx.y * nchunk + blockIdx.x] + lane_rank(b);
    for (int j = 0; j < w; j++) rank += wsum[j];
    if (!k) return;
    const size_t from = (size_t)row0[blockIdx.y] + i, to = (size_t)new0[blockIdx.y] + rank;
    pts_out[to] = pts[from];
    counts_out[to] = counts[from];
}

// the nearest target distance: one float
struct Nearest1 {
    float pq[3];
    float bd;
    __device__ __forceinline__ void visit(const float4 t) {
        const float pi[3] = {t.x, t.y, t.z};
        bd = fminf(bd, dist2f(pq, pi));
    }
    __device__ __forceinline__ float kth() const { return bd; }
};

// grid (source point blocks, pairs): getFitnessScore's nearest squared distance
// of every transformed source point over the whole target (no distance cap),
// the source in its cell order; nn in source point order at the pair's `work`
__global__ __launch_bounds__(64) void k_gicp_fit_nn(const GgCloud* __restrict__ cl, const GgPair* __restrict__ pairs,
                                                    const int* __restrict__ cstart,
                                                    const float4* __restrict__ sorted, const float* __restrict__ T,
                                                    float* __restrict__ nn) {
    const GgPair pr = pairs[blockIdx.y];
    const GgCloud S = cl[pr.s], G = cl[pr.t];
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S.n || G.n == 0) return;
    const float4 me = sorted[(size_t)S.p0 + s];
    const float p[3] = {me.x, me.y, me.z};
    Nearest1 v;
    xform4f(T + 16 * (size_t)blockIdx.y, p, v.pq);
    v.bd = __builtin_inff();
    int c[3];
    gg_cell3(G, v.pq, c);
    gg_walk(G, cstart + G.c0, sorted, c, v);
    nn[(size_t)pr.work + __float_as_int(me.w)] = v.bd;
}

// one workgroup per pair: score = (sum of nn in block_sum256's order) / ns;
// DBL_MAX for an empty source or target (PCL's nr == 0)
__global__ __launch_bounds__(GI_THREADS) void k_gicp_fit_sum(const GgCloud* __restrict__ cl,
                                                             const GgPair* __restrict__ pairs,
                                                             const float* __restrict__ nn,
                                                             double* __restrict__ score) {
    __shared__ double red[1][GI_THREADS];
    __shared__ double out[1];
    const GgPair pr = pairs[blockIdx.x];
    const int ns = cl[pr.s].n;
    if (ns == 0 || cl[pr.t].n == 0) {
        if (threadIdx.x == 0) score[blockIdx.x] = DBL_MAX;
        return;
    }
    double v[1] = {0};
    for (int i = threadIdx.x; i < ns; i += GI_THREADS) v[0] += (double)nn[(size_t)pr.work + i];
    block_sum256<1>(v, red, out);
    if (threadIdx.x == 0) score[blockIdx.x] = out[0] / (double)ns;
}

// the correspondence search over g.rings rings around the query's (clipped)
// cell: every target point closer than max_corr_dist lies in them (the host
// chose g.rings so), the selection is by (distance, index)
struct GridSearch {
    GgCloud g;
    const int* cs;
    const float4* sorted;
    __device__ __forceinline__ int operator()(const float* q, float* bdo) const {
        int c[3];
        gg_cell3(g, q, c);
        float bd = __builtin_inff();
        int best = 0;
        const int z0 = max(c[2] - g.rings, 0), z1 = min(c[2] + g.rings, g.gz - 1);
        const int y0 = max(c[1] - g.rings, 0), y1 = min(c[1] + g.rings, g.gy - 1);
        const int x0 = max(c[0] - g.rings, 0), x1 = min(c[0] + g.rings, g.gx - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                const int row = (z * g.gy + y) * g.gx;
                const int e = cs[row + x1 + 1];
                for (int i = cs[row + x0]; i < e; i++) {
                    const float4 t = sorted[i];
                    const float tj[3] = {t.x, t.y, t.z};
                    const float d = dist2f(q, tj);
                    const int idx = __float_as_int(t.w);
                    if (d < bd || (d == bd && idx < best)) {
                        bd = d;
                        best = idx;
                    }
                }
            }
        *bdo = bd;
        return best;
    }
};

// one workgroup per pair; the clouds of a pair by index, so that a cloud serves
// many pairs with one grid and one set of covariances
__global__ __launch_bounds__(GI_THREADS) void k_gicp_grid(
    const float* __restrict__ P, const GgCloud* __restrict__ cl, const GgPair* __restrict__ pairs,
    const int* __restrict__ cstart, const float4* __restrict__ sorted, const double* __restrict__ C,
    float* __restrict__ outp, double* __restrict__ Mah, int* __restrict__ is, int* __restrict__ it,
    const float* __restrict__ guess, double max_corr_dist, int max_iterations, int max_inner, float* __restrict__ T12,
    int* __restrict__ outi) {
    const int pb = blockIdx.x;
    const GgPair pr = pairs[pb];
    const GgCloud S = cl[pr.s], T = cl[pr.t];
    const size_t w = (size_t)pr.work;
    gicp_body(P + 3 * (size_t)S.p0, S.n, P + 3 * (size_t)T.p0, T.n, C + 9 * (size_t)S.p0, C + 9 * (size_t)T.p0,
              outp + 3 * w, Mah + 9 * w, is + w, it + w, guess + 16 * pb, max_corr_dist, max_iterations, max_inner,
              T12 + 16 * pb, outi + 4 * pb, GridSearch{T, cstart + T.c0, sorted});
}

}  // namespace

void launch_gg_pack(hipStream_t st, const float* src, int stride, const int* row0, const int* offs, int ncl,
                    int max_n, float* dst) {
    if (ncl == 0 || max_n == 0) return;
    hipLaunchKernelGGL(k_gg_pack, dim3((max_n + 255) / 256, ncl), dim3(256), 0, st, src, stride, row0, offs, dst);
}

void launch_gg_bounds(hipStream_t st, const float* P, const int* offs, int ncl, int max_n, uint32_t* bounds) {
    if (ncl == 0 || max_n == 0) return;
    hipLaunchKernelGGL(k_gg_bounds, dim3((max_n + GG_CHUNK - 1) / GG_CHUNK, ncl), dim3(256), 0, st, P, offs, bounds);
}

void launch_gg_build(hipStream_t st, const float* P, const GgCloud* cl, int ncl, int max_n, int64_t ncells_total,
                     int* key, int* cnt, int* fill, int* bsum, float4* sorted) {
    if (ncl == 0 || max_n == 0) return;
    const dim3 pts((max_n + 255) / 256, ncl);
    const int m = (int)ncells_total + 1, nb = (m + GG_CHUNK - 1) / GG_CHUNK;
    hipLaunchKernelGGL(k_gg_count, pts, dim3(256), 0, st, P, cl, key, cnt);
    hipLaunchKernelGGL(k_gg_scan_chunks, dim3(nb), dim3(256), 0, st, cnt, m, bsum);
    hipLaunchKernelGGL(k_gg_scan_tops, dim3(1), dim3(256), 0, st, bsum, nb);
    hipLaunchKernelGGL(k_gg_scan_add, dim3((m + 255) / 256), dim3(256), 0, st, cnt, m, bsum);
    hipLaunchKernelGGL(k_gg_scatter, pts, dim3(256), 0, st, P, cl, key, cnt, fill, sorted);
}

void launch_gg_cov(hipStream_t st, const float* P, const GgCloud* cl, int ncl, int max_n, const int* cstart,
                   const float4* sorted, double* C) {
    if (ncl == 0 || max_n < 20) return;
    hipLaunchKernelGGL(k_gicp_cov_grid, dim3((max_n + 63) / 64, ncl), dim3(64), 0, st, P, cl, cstart, sorted, C, 1e-3);
}

void launch_sor(hipStream_t st, const GgCloud* cl, int ncl, int max_n, const int* cstart, const float4* sorted,
                int mean_k, double stddev_mul, float* dist, SorStats* stats, uint8_t* keep, int* chunk_cnt) {
    if (ncl == 0 || max_n == 0) return;
    const int nchunk = (max_n + 255) / 256;
    if (max_n > mean_k) {
        hipLaunchKernelGGL(k_sor_dist, dim3((max_n + 63) / 64, ncl), dim3(64), (size_t)(mean_k + 1) * 64 * 4, st, cl,
                           cstart, sorted, mean_k, dist);
        hipLaunchKernelGGL(k_sor_stats, dim3(ncl), dim3(GI_THREADS), 0, st, cl, dist, mean_k, stddev_mul, stats);
    }
    hipLaunchKernelGGL(k_sor_mark, dim3(nchunk, ncl), dim3(256), 0, st, cl, dist, stats, mean_k, nchunk, keep,
                       chunk_cnt);
    hipLaunchKernelGGL(k_sor_scan, dim3(ncl), dim3(256), 0, st, cl, nchunk, chunk_cnt, stats);
}

void launch_sor_pack(hipStream_t st, const GgCloud* cl, int ncl, int max_n, const uint8_t* keep, const int* chunk_cnt,
                     const int* row0, const int* new0, const void* pts, const int* counts, void* pts_out,
                     int* counts_out) {
    if (ncl == 0 || max_n == 0) return;
    const int nchunk = (max_n + 255) / 256;
    hipLaunchKernelGGL(k_sor_pack, dim3(nchunk, ncl), dim3(256), 0, st, cl, keep, chunk_cnt, nchunk, row0, new0,
                       (const uint4*)pts, counts, (uint4*)pts_out, counts_out);
}

void launch_gg_fitness(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, int max_ns,
                       const int* cstart, const float4* sorted, const float* T, float* nn, double* score) {
    if (nprob == 0) return;
    if (max_ns)
        hipLaunchKernelGGL(k_gicp_fit_nn, dim3((max_ns + 63) / 64, nprob), dim3(64), 0, st, cl, pairs, cstart, sorted,
                           T, nn);
    hipLaunchKernelGGL(k_gicp_fit_sum, dim3(nprob), dim3(GI_THREADS), 0, st, cl, pairs, nn, score);
}

void launch_gg_icp(hipStream_t st, const float* P, const GgCloud* cl, const GgPair* pairs, int nprob,
                   const int* cstart, const float4* sorted, const double* C, float* outp, double* Mah, int* is,
                   int* it, const float* guess, double max_corr_dist, int max_iterations, int max_inner, float* T12,
                   int* outi) {
    if (nprob == 0) return;
    hipLaunchKernelGGL(k_gicp_grid, dim3(nprob), dim3(GI_THREADS), 0, st, P, cl, pairs, cstart, sorted, C, outp, Mah,
                       is, it, guess, max_corr_dist, max_iterations, max_inner, T12, outi);
}

void launch_gicp_cov(hipStream_t st, const float* src, const int* soffs, double* Cs, const float* tgt,
                     const int* toffs, double* Ct, int nprob, int max_n) {
    const int nbx = (max_n + 63) / 64;
    hipLaunchKernelGGL(k_gicp_cov, dim3(nbx, nprob, 2), dim3(64), 0, st, src, soffs, Cs, tgt, toffs, Ct, 1e-3);
}

void launch_gicp(hipStream_t st, const float* src, const float* tgt, int nprob, int max_ns, int max_nt, double* Cs,
                 double* Ct, float* outp, double* Mah, int* is, int* it, GicpArgs args, float* T12, int* outi) {
    launch_gicp_cov(st, src, args.soffs, Cs, tgt, args.toffs, Ct, nprob, std::max(max_ns, max_nt));
    hipLaunchKernelGGL(k_gicp, dim3(nprob), dim3(GI_THREADS), 0, st, src, tgt, Cs, Ct, outp, Mah, is, it, args, T12,
                       outi);
}

}  // namespace odo
