// LocalBundleAdjustment::Compute for gfx950 (Odometry/localbundleadjustment.cpp:65-315):
// g2o OptimizationAlgorithmLevenberg over SE3Expmap pose vertices and
// marginalised XYZ point vertices with mono / stereo reprojection edges,
// BlockSolver_6_3 (Schur complement on the poses, LDL^T without pivoting),
// two optimize() calls with the chi2 / depth classification between them.
// DESIGN.md §4 "Local BA" has the layout; in short:
//   - every per-edge, per-landmark and linear-algebra step is an FP64 kernel
//     on the context's stream; the host keeps only the Levenberg control flow
//     and reads three scalars per trial (chi2, scale, solver status);
//   - edges are grouped by landmark (a CSR built once per call): one thread
//     owns a landmark, forms Hll, bl and its W blocks in edge order, inverts
//     Hll + lambda I and back-substitutes its step;
//   - the landmarks' Schur products go to per-chunk partial reduced systems
//     (fixed chunks of BA_CHUNK landmarks, landmarks of a chunk in index
//     order), which are then added in chunk order: no floating-point atomics,
//     so a call is bit-identical run to run;
//   - the reduced system (at most 384 x 384) is factored in place in L2 by one
//     workgroup;
//   - the estimates are double-buffered: a trial writes the other buffer and
//     accept / reject is a pointer swap on the host.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "odo_device.h"
#include "odo_internal.h"

// parity with the float64 reference is a tolerance (as in k_pnp.hip)
#pragma clang fp contract(fast)

namespace odo {

#define BA_BLOCK 256
#define BA_CHUNK 128      // landmarks per partial reduced system ...
#define BA_MAX_CHUNKS 64  // ... until there would be more than 64 of them
#define BA_LDLT_THREADS 1024
#define BA_E_STEREO 1
#define BA_E_LEVEL1 2

struct BaCam {
    double fx, fy, cx, cy, bf;
};

// fixed-tree sum / max over a 256-thread workgroup, the result in every thread
ODO_INLINE double ba_block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = BA_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
ODO_INLINE double ba_block_max(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = BA_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = fmax(sh[t], sh[t + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// One edge at pose P (R row-major 9, t 3) and point X: camera-frame point,
// error obs - project (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError), chi2
struct BaEdgeEval {
    double Xc[3], e[3], chi2;
};
ODO_INLINE BaEdgeEval ba_edge_eval(const double* __restrict__ P, const double* __restrict__ X, const float* __restrict__ ob,
                                   bool st, double info, const BaCam& c) {
    BaEdgeEval r;
#pragma unroll
    for (int i = 0; i < 3; i++) r.Xc[i] = (P[3 * i] * X[0] + P[3 * i + 1] * X[1]) + (P[3 * i + 2] * X[2] + P[9 + i]);
    const double iz = 1.0 / r.Xc[2];
    const double pu = c.fx * r.Xc[0] * iz + c.cx, pv = c.fy * r.Xc[1] * iz + c.cy;
    r.e[0] = (double)ob[0] - pu;
    r.e[1] = (double)ob[1] - pv;
    r.e[2] = st ? (double)ob[2] - (pu - c.bf * iz) : 0.0;
    r.chi2 = info * ((r.e[0] * r.e[0] + r.e[1] * r.e[1]) + r.e[2] * r.e[2]);
    return r;
}
// RobustKernelHuber::robustify: rho and rho'
ODO_INLINE void ba_huber(double delta, double chi, double& rho0, double& rho1) {
    const double dsqr = delta * delta;
    if (chi <= dsqr) {
        rho0 = chi;
        rho1 = 1.0;
    } else {
        const double sq = sqrt(chi);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}
// d error / d (omega, upsilon) of the pose (update exp(dx) T; the Jacobian of
// k_pnp.hip / oracle/pose_ref.cpp:665-688) and d error / d X = -(d proj / d Xc) R
ODO_INLINE void ba_jacobians(const double* __restrict__ P, const double Xc[3], bool st, const BaCam& c, bool want_pose,
                             double Jp[3][6], double Jl[3][3]) {
    const double x = Xc[0], y = Xc[1], iz = 1.0 / Xc[2], iz2 = iz * iz;
    const double a0 = c.fx * iz, a2 = -c.fx * x * iz2, b1 = c.fy * iz, b2 = -c.fy * y * iz2, s2 = a2 + c.bf * iz2;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Jl[0][j] = -(a0 * P[j] + a2 * P[6 + j]);
        Jl[1][j] = -(b1 * P[3 + j] + b2 * P[6 + j]);
        Jl[2][j] = st ? -(a0 * P[j] + s2 * P[6 + j]) : 0.0;
    }
    if (!want_pose) return;
    Jp[0][0] = x * y * iz2 * c.fx;
    Jp[0][1] = -(1 + (x * x * iz2)) * c.fx;
    Jp[0][2] = y * iz * c.fx;
    Jp[0][3] = -iz * c.fx;
    Jp[0][4] = 0;
    Jp[0][5] = x * iz2 * c.fx;
    Jp[1][0] = (1 + y * y * iz2) * c.fy;
    Jp[1][1] = -x * y * iz2 * c.fy;
    Jp[1][2] = -x * iz * c.fy;
    Jp[1][3] = 0;
    Jp[1][4] = -iz * c.fy;
    Jp[1][5] = y * iz2 * c.fy;
    Jp[2][0] = st ? Jp[0][0] - c.bf * y * iz2 : 0.0;
    Jp[2][1] = st ? Jp[0][1] + c.bf * x * iz2 : 0.0;
    Jp[2][2] = st ? Jp[0][2] : 0.0;
    Jp[2][3] = st ? Jp[0][3] : 0.0;
    Jp[2][4] = 0;
    Jp[2][5] = st ? Jp[0][5] - c.bf * iz2 : 0.0;
}

struct BaGraph {  // the uploaded problem (device pointers)
    int nk, nl, ne, nf;
    const int32_t *ekf, *elm;
    const float* eobs;  // 3 per edge: u, v, uR
    const int32_t *lstart, *lorder, *kstart, *korder, *pidx;
};

// ---- initial estimates: SE3Quat from the float matrix (Converter::toSE3Quat:
// quaternion of R, normalised, w >= 0), points and the information weight
__global__ void __launch_bounds__(BA_BLOCK) k_ba_init(BaGraph g, const float* __restrict__ Tcw, const float* __restrict__ Xw,
                                                       double* __restrict__ P, double* __restrict__ X,
                                                       double* __restrict__ info, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i < g.nk) {
        const float* T = Tcw + 16 * (size_t)i;
        double m[3][3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) m[r][c] = (double)T[4 * r + c];
        double qx, qy, qz, qw;
        double t = m[0][0] + (m[1][1] + m[2][2]);
        if (t > 0) {  // Eigen quaternionbase_assign_impl<Matrix3>
            t = sqrt(t + 1.0);
            qw = 0.5 * t;
            t = 0.5 / t;
            qx = (m[2][1] - m[1][2]) * t;
            qy = (m[0][2] - m[2][0]) * t;
            qz = (m[1][0] - m[0][1]) * t;
        } else {
            int a = 0;
            if (m[1][1] > m[0][0]) a = 1;
            if (m[2][2] > m[a][a]) a = 2;
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            t = sqrt(m[a][a] - m[b][b] - m[c][c] + 1.0);
            double q[3];
            q[a] = 0.5 * t;
            t = 0.5 / t;
            qw = (m[c][b] - m[b][c]) * t;
            q[b] = (m[b][a] + m[a][b]) * t;
            q[c] = (m[c][a] + m[a][c]) * t;
            qx = q[0];
            qy = q[1];
            qz = q[2];
        }
        if (qw < 0) {
            qx = -qx;
            qy = -qy;
            qz = -qz;
            qw = -qw;
        }
        const double in = 1.0 / sqrt((qx * qx + qy * qy) + (qz * qz + qw * qw));
        qx *= in;
        qy *= in;
        qz *= in;
        qw *= in;
        double* o = P + 12 * (size_t)i;
        o[0] = 1 - 2 * (qy * qy + qz * qz);
        o[1] = 2 * (qx * qy - qw * qz);
        o[2] = 2 * (qx * qz + qw * qy);
        o[3] = 2 * (qx * qy + qw * qz);
        o[4] = 1 - 2 * (qx * qx + qz * qz);
        o[5] = 2 * (qy * qz - qw * qx);
        o[6] = 2 * (qx * qz - qw * qy);
        o[7] = 2 * (qy * qz + qw * qx);
        o[8] = 1 - 2 * (qx * qx + qy * qy);
        for (int r = 0; r < 3; r++) o[9 + r] = (double)T[4 * r + 3];
    }
    if (i < g.nl) {
        for (int r = 0; r < 3; r++) X[3 * (size_t)i + r] = (double)Xw[3 * (size_t)i + r];
        const float z = Xw[3 * (size_t)i + 2];
        info[i] = (double)(1.0f / (z * z));  // localbundleadjustment.cpp:158,185: float arithmetic
    }
    if (i < g.ne) flags[i] = g.eobs[3 * (size_t)i + 2] < 0.f ? 0 : BA_E_STEREO;
}

// ---- computeActiveErrors + activeRobustChi2 at (P, X): the chi2 of every
// level-0 edge is stored (what g2o keeps in the edge), the robust chi2 summed
// per workgroup in a fixed tree
__global__ void __launch_bounds__(BA_BLOCK) k_ba_error(BaGraph g, BaCam cam, const double* __restrict__ P,
                                                        const double* __restrict__ X, const double* __restrict__ info,
                                                        const uint8_t* __restrict__ flags, int robust, double dMono,
                                                        double dStereo, double* __restrict__ c2,
                                                        double* __restrict__ part) {
    __shared__ double sh[BA_BLOCK];
    const int e = blockIdx.x * BA_BLOCK + threadIdx.x;
    double v = 0;
    if (e < g.ne && !(flags[e] & BA_E_LEVEL1)) {
        const bool st = flags[e] & BA_E_STEREO;
        const int lm = g.elm[e];
        const BaEdgeEval r = ba_edge_eval(P + 12 * (size_t)g.ekf[e], X + 3 * (size_t)lm, g.eobs + 3 * (size_t)e, st, info[lm], cam);
        c2[e] = r.chi2;
        v = r.chi2;
        if (robust) {
            double r1;
            ba_huber(st ? dStereo : dMono, r.chi2, v, r1);
        }
    }
    v = ba_block_sum(v, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// sums of the per-workgroup partials in index order: scal[0] = chi2, scal[1] = the landmarks' share of the scale
__global__ void __launch_bounds__(BA_BLOCK) k_ba_final(const double* __restrict__ pchi, int nchi, const double* __restrict__ pscale,
                                                        int nscale, double* __restrict__ scal) {
    __shared__ double sh[BA_BLOCK];
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nchi; i += BA_BLOCK) a += pchi[i];
    for (int i = threadIdx.x; i < nscale; i += BA_BLOCK) b += pscale[i];
    a = ba_block_sum(a, sh);
    b = ba_block_sum(b, sh);
    if (threadIdx.x == 0) {
        scal[0] = a;
        scal[1] = b;
    }
}

// ---- linearisation grouped by landmark: one thread per landmark walks its
// level-0 edges in edge order: Hll (packed 00 01 02 11 12 22), bl, and for the
// edges of free keyframes W = Jp^T w Jl (6 x 3) and the compact list flist
// (edge, free-keyframe index; fcnt entries from lstart[l]) the Schur kernel
// walks. lact: the landmark is in the system.
__global__ void __launch_bounds__(BA_BLOCK) k_ba_linearize(BaGraph g, BaCam cam, const double* __restrict__ P,
                                                            const double* __restrict__ X, const double* __restrict__ info,
                                                            const uint8_t* __restrict__ flags, int robust, double dMono,
                                                            double dStereo, double* __restrict__ Hll, double* __restrict__ bl,
                                                            double* __restrict__ W, uint8_t* __restrict__ lact,
                                                            int2* __restrict__ flist, int* __restrict__ fcnt,
                                                            double* __restrict__ pmax) {
    __shared__ double sh[BA_BLOCK];
    const int l = blockIdx.x * BA_BLOCK + threadIdx.x;
    double mx = 0;
    if (l < g.nl) {
        double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
        bool act = false;
        int nfree = 0;
        const double inf = info[l];
        const double* Xl = X + 3 * (size_t)l;
        for (int q = g.lstart[l]; q < g.lstart[l + 1]; q++) {
            const int e = g.lorder[q];
            const uint8_t fl = flags[e];
            if (fl & BA_E_LEVEL1) continue;
            act = true;
            const bool st = fl & BA_E_STEREO;
            const int kf = g.ekf[e];
            const double* Pk = P + 12 * (size_t)kf;
            const BaEdgeEval r = ba_edge_eval(Pk, Xl, g.eobs + 3 * (size_t)e, st, inf, cam);
            double rho0, rho1 = 1.0;
            if (robust) ba_huber(st ? dStereo : dMono, r.chi2, rho0, rho1);
            const double w = rho1 * inf;
            const bool fr = g.pidx[kf] >= 0;
            double Jp[3][6], Jl[3][3];
            ba_jacobians(Pk, r.Xc, st, cam, fr, Jp, Jl);
            int h = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                b[a] -= (Jl[0][a] * (w * r.e[0]) + Jl[1][a] * (w * r.e[1])) + Jl[2][a] * (w * r.e[2]);
#pragma unroll
                for (int c = a; c < 3; c++) {
                    H[h] += (Jl[0][a] * w * Jl[0][c] + Jl[1][a] * w * Jl[1][c]) + Jl[2][a] * w * Jl[2][c];
                    h++;
                }
            }
            if (fr) {
                flist[g.lstart[l] + nfree++] = make_int2(e, g.pidx[kf]);
                double* We = W + 18 * (size_t)e;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        We[3 * a + c] = (Jp[0][a] * w * Jl[0][c] + Jp[1][a] * w * Jl[1][c]) + Jp[2][a] * w * Jl[2][c];
            }
        }
        for (int k = 0; k < 6; k++) Hll[6 * (size_t)l + k] = H[k];
        for (int k = 0; k < 3; k++) bl[3 * (size_t)l + k] = b[k];
        lact[l] = act ? 1 : 0;
        fcnt[l] = nfree;
        mx = fmax(fabs(H[0]), fmax(fabs(H[3]), fabs(H[5])));
    }
    mx = ba_block_max(mx, sh);
    if (threadIdx.x == 0) pmax[blockIdx.x] = mx;
}

// ---- the pose blocks: one wave per keyframe walks the keyframe's level-0
// edges (its own CSR, edge order), lanes striding, and sums Hpp (upper
// triangle) and bp over the lanes with a fixed xor butterfly
__global__ void __launch_bounds__(64) k_ba_pose(BaGraph g, BaCam cam, const double* __restrict__ P, const double* __restrict__ X,
                                                const double* __restrict__ info, const uint8_t* __restrict__ flags, int robust,
                                                double dMono, double dStereo, double* __restrict__ Hpp,
                                                double* __restrict__ bp, double* __restrict__ posemax,
                                                uint8_t* __restrict__ factive) {
    const int kf = blockIdx.x, lane = threadIdx.x;
    const int pi = g.pidx[kf];
    if (pi < 0) return;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0;
    const double* Pk = P + 12 * (size_t)kf;
    for (int q = g.kstart[kf] + lane; q < g.kstart[kf + 1]; q += 64) {
        const int e = g.korder[q];
        const uint8_t fl = flags[e];
        if (fl & BA_E_LEVEL1) continue;
        const bool st = fl & BA_E_STEREO;
        const int lm = g.elm[e];
        const double inf = info[lm];
        const BaEdgeEval r = ba_edge_eval(Pk, X + 3 * (size_t)lm, g.eobs + 3 * (size_t)e, st, inf, cam);
        double rho0, rho1 = 1.0;
        if (robust) ba_huber(st ? dStereo : dMono, r.chi2, rho0, rho1);
        const double w = rho1 * inf;
        double Jp[3][6], Jl[3][3];
        ba_jacobians(Pk, r.Xc, st, cam, true, Jp, Jl);
        int h = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            acc[21 + a] -= (Jp[0][a] * (w * r.e[0]) + Jp[1][a] * (w * r.e[1])) + Jp[2][a] * (w * r.e[2]);
#pragma unroll
            for (int c = a; c < 6; c++) {
                acc[h] += (Jp[0][a] * w * Jp[0][c] + Jp[1][a] * w * Jp[1][c]) + Jp[2][a] * w * Jp[2][c];
                h++;
            }
        }
        acc[27] += 1.0;  // level-0 edges of the keyframe
    }
#pragma unroll
    for (int k = 0; k < 28; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if (lane == 0) {
        double* Ho = Hpp + 36 * (size_t)pi;
        int h = 0;
        double mx = 0;
        for (int a = 0; a < 6; a++)
            for (int c = a; c < 6; c++) {
                Ho[6 * a + c] = acc[h];
                Ho[6 * c + a] = acc[h];
                if (a == c) mx = fmax(mx, fabs(acc[h]));
                h++;
            }
        for (int a = 0; a < 6; a++) bp[6 * (size_t)pi + a] = acc[21 + a];
        posemax[pi] = mx;
        factive[pi] = acc[27] > 0 ? 1 : 0;
    }
}

// scal[4] = max |diag H| over the pose and point blocks
__global__ void __launch_bounds__(BA_BLOCK) k_ba_maxdiag(const double* __restrict__ pmax, int npart, const double* __restrict__ posemax,
                                                          int nf, double* __restrict__ scal) {
    __shared__ double sh[BA_BLOCK];
    double m = 0;
    for (int i = threadIdx.x; i < npart; i += BA_BLOCK) m = fmax(m, pmax[i]);
    for (int i = threadIdx.x; i < nf; i += BA_BLOCK) m = fmax(m, posemax[i]);
    m = ba_block_max(m, sh);
    if (threadIdx.x == 0) scal[4] = m;
}

// ---- (Hll + lambda I)^-1 per landmark: cofactors over the determinant (Eigen's 3x3 inverse)
__global__ void __launch_bounds__(BA_BLOCK) k_ba_hinv(int nl, const double* __restrict__ Hll, const uint8_t* __restrict__ lact,
                                                       double lam, double* __restrict__ Hinv) {
    const int l = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (l >= nl || !lact[l]) return;
    const double* H = Hll + 6 * (size_t)l;
    const double a00 = H[0] + lam, a01 = H[1], a02 = H[2], a11 = H[3] + lam, a12 = H[4], a22 = H[5] + lam;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    double* o = Hinv + 6 * (size_t)l;
    o[0] = c00 / det;
    o[1] = c01 / det;
    o[2] = c02 / det;
    o[3] = c11 / det;
    o[4] = c12 / det;
    o[5] = c22 / det;
}

// ---- the Schur products of one chunk of landmarks into the chunk's partial
// reduced system Sp[chunk] ((n + 1) x n: n rows of -sum W Hll^-1 W^T, then the
// row of -sum W Hll^-1 bl). One workgroup per chunk takes its landmarks in
// index order; within a landmark every (edge pair, entry) is one thread's
// item, and a landmark has at most one edge per keyframe (checked by the
// host), so no two items of a landmark touch the same entry.
__global__ void __launch_bounds__(BA_BLOCK) k_ba_schur(BaGraph g, int n, int chunk, const uint8_t* __restrict__ lact,
                                                        const int2* __restrict__ flist, const int* __restrict__ fcnt,
                                                        const double* __restrict__ Hinv, const double* __restrict__ bl,
                                                        const double* __restrict__ W, double* __restrict__ Sp) {
    const int t = threadIdx.x;
    double* Pc = Sp + (size_t)blockIdx.x * (size_t)(n + 1) * n;
    for (int i = t; i < (n + 1) * n; i += BA_BLOCK) Pc[i] = 0;
    __syncthreads();
    const int l0 = blockIdx.x * chunk, l1 = min(g.nl, l0 + chunk);
    for (int l = l0; l < l1; l++) {
        const int m = fcnt[l];
        if (!lact[l] || m == 0) continue;
        const int2* fl = flist + g.lstart[l];
        const double* hi = Hinv + 6 * (size_t)l;
        const double h00 = hi[0], h01 = hi[1], h02 = hi[2], h11 = hi[3], h12 = hi[4], h22 = hi[5];
        const double b0 = bl[3 * (size_t)l], b1 = bl[3 * (size_t)l + 1], b2 = bl[3 * (size_t)l + 2];
        const int nblk = m * m * 36, items = nblk + m * 6;
        for (int it = t; it < items; it += BA_BLOCK) {
            if (it < nblk) {
                const int pr = it / 36, rc = it - pr * 36, r = rc / 6, c = rc - r * 6, a = pr / m, b = pr - a * m;
                const int2 ea = fl[a], eb = fl[b];
                const double* Wa = W + 18 * (size_t)ea.x + 3 * r;
                const double* Wb = W + 18 * (size_t)eb.x + 3 * c;
                const double t0 = (h00 * Wb[0] + h01 * Wb[1]) + h02 * Wb[2];
                const double t1 = (h01 * Wb[0] + h11 * Wb[1]) + h12 * Wb[2];
                const double t2 = (h02 * Wb[0] + h12 * Wb[1]) + h22 * Wb[2];
                Pc[(size_t)(6 * ea.y + r) * n + 6 * eb.y + c] -= (Wa[0] * t0 + Wa[1] * t1) + Wa[2] * t2;
            } else {
                const int j = it - nblk, a = j / 6, r = j - a * 6;
                const int2 ea = fl[a];
                const double* Wa = W + 18 * (size_t)ea.x + 3 * r;
                const double t0 = (h00 * b0 + h01 * b1) + h02 * b2;
                const double t1 = (h01 * b0 + h11 * b1) + h12 * b2;
                const double t2 = (h02 * b0 + h12 * b1) + h22 * b2;
                Pc[(size_t)n * n + 6 * ea.y + r] -= (Wa[0] * t0 + Wa[1] * t1) + Wa[2] * t2;
            }
        }
        __syncthreads();  // the next landmark's items may touch the same entries from other threads
    }
}

// ---- S = Hpp + lambda I + the chunks' partials in chunk order; row n the
// right-hand side bp + partials. A free pose without a level-0 edge is not in
// the system: its block is the identity and its right-hand side zero (dx = 0).
__global__ void __launch_bounds__(BA_BLOCK) k_ba_reduce(int n, int nchunks, const double* __restrict__ Sp,
                                                         const double* __restrict__ Hpp, const double* __restrict__ bp,
                                                         const uint8_t* __restrict__ factive, double lam,
                                                         double* __restrict__ S) {
    const int idx = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (idx >= (n + 1) * n) return;
    const int row = idx / n, col = idx - row * n;
    const size_t stride = (size_t)(n + 1) * n;
    double v = 0;
    if (row < n) {
        const int ib = row / 6, jb = col / 6;
        if (ib == jb) v = Hpp[36 * (size_t)ib + 6 * (row - 6 * ib) + (col - 6 * jb)] + (row == col ? lam : 0.0);
        for (int c = 0; c < nchunks; c++) v += Sp[c * stride + idx];
        if (!factive[ib] || !factive[jb]) v = row == col ? 1.0 : 0.0;
    } else {
        v = bp[col];
        for (int c = 0; c < nchunks; c++) v += Sp[c * stride + idx];
        if (!factive[col / 6]) v = 0.0;
    }
    S[idx] = v;
}

// ---- LinearSolverEigen (SimplicialLDLT) on the reduced system: LDL^T without
// pivoting, right-looking, in place in S (L2-resident: at most 1.2 MB), the
// right-hand side carried as row n so that the forward substitution and the
// division by D come out of the factorisation; then the backward
// substitution. One workgroup: the n pivots are a serial chain, and a
// workgroup barrier per pivot is cheaper than a launch. A zero pivot fails the
// solve (scal[2] = 1) and leaves dx = 0; no test reaches that branch (DESIGN.md
// §4 "Local BA").
__global__ void __launch_bounds__(BA_LDLT_THREADS) k_ba_ldlt(int n, double* __restrict__ S, double* __restrict__ dx,
                                                              double* __restrict__ scal) {
    __shared__ double colc[6 * 64 + 1], coll[6 * 64 + 1], xs[6 * 64];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    bool fail = false;
    for (int k = 0; k < n; k++) {
        const double d = S[(size_t)k * n + k];
        if (d == 0) {  // the same value in every thread
            fail = true;
            break;
        }
        for (int i = k + 1 + t; i <= n; i += BA_LDLT_THREADS) {
            const double c = S[(size_t)i * n + k], l = c / d;
            colc[i] = c;
            coll[i] = l;
            S[(size_t)i * n + k] = l;
        }
        __syncthreads();
        for (int i = k + 1 + ty; i <= n; i += 32) {
            const double li = coll[i];
            const int jmax = min(i, n - 1);
            for (int j = k + 1 + tx; j <= jmax; j += 32) S[(size_t)i * n + j] -= li * colc[j];
        }
        __syncthreads();
    }
    if (fail) {
        for (int i = t; i < n; i += BA_LDLT_THREADS) dx[i] = 0;
        if (t == 0) scal[2] = 1.0;
        return;
    }
    for (int i = t; i < n; i += BA_LDLT_THREADS) xs[i] = S[(size_t)n * n + i];
    __syncthreads();
    for (int k = n - 1; k > 0; k--) {
        const double xk = xs[k];
        for (int i = t; i < k; i += BA_LDLT_THREADS) xs[i] -= S[(size_t)k * n + i] * xk;
        __syncthreads();
    }
    for (int i = t; i < n; i += BA_LDLT_THREADS) dx[i] = xs[i];
    if (t == 0) scal[2] = 0.0;
}

// ---- VertexSE3Expmap::oplusImpl into the trial buffer: T <- exp(dx) T
// (SE3Quat::exp's Rodrigues R and V); poses outside the system are copied.
// scal[3] = the poses' share of the scale, sum dx (lambda dx + bp), in index order.
__global__ void __launch_bounds__(BA_BLOCK) k_ba_pose_update(BaGraph g, const double* __restrict__ P, double* __restrict__ Pt,
                                                              const double* __restrict__ dx, const uint8_t* __restrict__ factive,
                                                              const double* __restrict__ bp, double lam,
                                                              double* __restrict__ scal) {
    for (int k = threadIdx.x; k < g.nk; k += BA_BLOCK) {
        const double* T = P + 12 * (size_t)k;
        double* o = Pt + 12 * (size_t)k;
        const int pi = g.pidx[k];
        if (pi < 0 || !factive[pi]) {
            for (int q = 0; q < 12; q++) o[q] = T[q];
            continue;
        }
        const double* u = dx + 6 * (size_t)pi;
        const double w0 = u[0], w1 = u[1], w2 = u[2];
        const double theta = sqrt(w0 * w0 + (w1 * w1 + w2 * w2));
        const double O[3][3] = {{0, -w2, w1}, {w2, 0, -w0}, {-w1, w0, 0}};
        double O2[3][3], R[3][3], V[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + (O[i][1] * O[1][j] + O[i][2] * O[2][j]);
        double a = 1.0, b = 1.0, c = 1.0;  // g2o's branch below 1e-5: R = V = I + O + O^2
        double vb = 1.0, vc = 1.0;
        if (!(theta < 0.00001)) {
            const double sn = sin(theta), cs = cos(theta), th2 = theta * theta;
            a = sn / theta;
            b = (1 - cs) / th2;
            vb = b;
            vc = (theta - sn) / (theta * th2);
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double id = i == j ? 1.0 : 0.0;
                R[i][j] = (id + a * O[i][j]) + b * O2[i][j];
                V[i][j] = theta < 0.00001 ? R[i][j] : (id + vb * O[i][j]) + vc * O2[i][j];
            }
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o[3 * i + j] = R[i][0] * T[j] + (R[i][1] * T[3 + j] + R[i][2] * T[6 + j]);
            o[9 + i] = (R[i][0] * T[9] + (R[i][1] * T[10] + R[i][2] * T[11])) +
                       (V[i][0] * u[3] + (V[i][1] * u[4] + V[i][2] * u[5]));
        }
    }
    if (threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < g.nf; i++)
            if (factive[i])
                for (int j = 0; j < 6; j++) {
                    const double x = dx[6 * i + j];
                    s += x * (lam * x + bp[6 * i + j]);
                }
        scal[3] = s;
    }
}

// ---- back-substitution and VertexSBAPointXYZ::oplusImpl into the trial
// buffer: dl = (Hll + lambda I)^-1 (bl - sum W^T dx), X <- X + dl; the
// landmark's share of the scale summed per workgroup in a fixed tree
__global__ void __launch_bounds__(BA_BLOCK) k_ba_backsub(BaGraph g, const double* __restrict__ X, double* __restrict__ Xt,
                                                          const uint8_t* __restrict__ flags, const uint8_t* __restrict__ lact,
                                                          const double* __restrict__ Hinv, const double* __restrict__ bl,
                                                          const double* __restrict__ W, const double* __restrict__ dx,
                                                          double lam, const double* __restrict__ scal,
                                                          double* __restrict__ part) {
    __shared__ double sh[BA_BLOCK];
    const int l = blockIdx.x * BA_BLOCK + threadIdx.x;
    double v = 0;
    if (l < g.nl) {
        double x[3] = {X[3 * (size_t)l], X[3 * (size_t)l + 1], X[3 * (size_t)l + 2]};
        if (lact[l]) {
            const double b[3] = {bl[3 * (size_t)l], bl[3 * (size_t)l + 1], bl[3 * (size_t)l + 2]};
            double r[3] = {b[0], b[1], b[2]};
            for (int q = g.lstart[l]; q < g.lstart[l + 1]; q++) {
                const int e = g.lorder[q];
                if (flags[e] & BA_E_LEVEL1) continue;
                const int p = g.pidx[g.ekf[e]];
                if (p < 0) continue;
                const double* We = W + 18 * (size_t)e;
                const double* u = dx + 6 * (size_t)p;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    double s = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++) s += We[3 * a + c] * u[a];
                    r[c] -= s;
                }
            }
            const double* hi = Hinv + 6 * (size_t)l;
            double dl[3] = {(hi[0] * r[0] + hi[1] * r[1]) + hi[2] * r[2], (hi[1] * r[0] + hi[3] * r[1]) + hi[4] * r[2],
                            (hi[2] * r[0] + hi[4] * r[1]) + hi[5] * r[2]};
            if (scal[2] != 0.0) dl[0] = dl[1] = dl[2] = 0.0;  // failed solve: the step is zero
#pragma unroll
            for (int c = 0; c < 3; c++) {
                x[c] += dl[c];
                v += dl[c] * (lam * dl[c] + b[c]);
            }
        }
        for (int c = 0; c < 3; c++) Xt[3 * (size_t)l + c] = x[c];
    }
    v = ba_block_sum(v, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// ---- localbundleadjustment.cpp:223-254 (mode 0: level 1) and :261-285 (mode 1:
// the erase list): the edge's stored chi2 against its threshold, and
// isDepthPositive at the current estimates. cnt[mode] counts the marks.
__global__ void __launch_bounds__(BA_BLOCK) k_ba_classify(BaGraph g, const double* __restrict__ P, const double* __restrict__ X,
                                                           const double* __restrict__ c2, double thMono, double thStereo,
                                                           int mode, uint8_t* __restrict__ flags, uint8_t* __restrict__ erase,
                                                           int* __restrict__ cnt) {
    const int e = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (e >= g.ne) return;
    const uint8_t fl = flags[e];
    const double* Pk = P + 12 * (size_t)g.ekf[e];
    const double* Xl = X + 3 * (size_t)g.elm[e];
    const double z = (Pk[6] * Xl[0] + Pk[7] * Xl[1]) + (Pk[8] * Xl[2] + Pk[11]);
    const bool bad = c2[e] > ((fl & BA_E_STEREO) ? thStereo : thMono) || !(z > 0.0);
    if (mode == 0) {
        if (bad) flags[e] = fl | BA_E_LEVEL1;
    } else {
        erase[e] = bad ? 1 : 0;
    }
    if (bad) atomicAdd(cnt + mode, 1);
}

// ---- localbundleadjustment.cpp:302-315: estimates cast to float. Keyframes
// that were never in the system (fixed, or free without an edge) keep their input bits.
__global__ void __launch_bounds__(BA_BLOCK) k_ba_output(BaGraph g, const double* __restrict__ P, const double* __restrict__ X,
                                                         const float* __restrict__ Tcw, const uint8_t* __restrict__ insys,
                                                         float* __restrict__ oT, float* __restrict__ oX) {
    const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
    if (i < g.nk) {
        float* o = oT + 16 * (size_t)i;
        if (insys[i]) {
            const double* T = P + 12 * (size_t)i;
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) o[4 * r + c] = (float)T[3 * r + c];
                o[4 * r + 3] = (float)T[9 + r];
            }
            o[12] = o[13] = o[14] = 0.f;
            o[15] = 1.f;
        } else {
            for (int q = 0; q < 16; q++) o[q] = Tcw[16 * (size_t)i + q];
        }
    }
    if (i < g.nl)
        for (int c = 0; c < 3; c++) oX[3 * (size_t)i + c] = (float)X[3 * (size_t)i + c];
}

// ------------------------------------------------------------------ the host
static inline int ba_nchunks(int nl, int* chunk) {
    int ch = BA_CHUNK;
    if ((nl + ch - 1) / ch > BA_MAX_CHUNKS) ch = (nl + BA_MAX_CHUNKS - 1) / BA_MAX_CHUNKS;
    *chunk = ch;
    return std::max(1, (nl + ch - 1) / ch);
}

struct BaScratch {
    double *P[2], *X[2], *info, *c2, *W, *Hll, *bl, *Hinv, *Hpp, *bp, *posemax, *Sp, *S, *dx, *pchi, *pscale, *pmax, *scal;
    uint8_t *flags, *lact, *factive;
    int2* flist;
    int *fcnt, *cnt;
    size_t bytes;
};
static BaScratch ba_carve(uint8_t* base, int nk, int nl, int ne, int nf) {
    BaScratch s{};
    Pack pk;
    auto take = [&](size_t b) {
        const size_t o = pk.add(std::max<size_t>(b, 8));
        return base ? base + o : nullptr;
    };
    const size_t n = 6 * (size_t)nf;
    int chunk;
    const int nch = ba_nchunks(nl, &chunk);
    const size_t nbe = ((size_t)ne + BA_BLOCK - 1) / BA_BLOCK, nbl = ((size_t)nl + BA_BLOCK - 1) / BA_BLOCK;
    for (int k = 0; k < 2; k++) {
        s.P[k] = (double*)take((size_t)nk * 12 * 8);
        s.X[k] = (double*)take((size_t)nl * 3 * 8);
    }
    s.info = (double*)take((size_t)nl * 8);
    s.c2 = (double*)take((size_t)ne * 8);
    s.W = (double*)take((size_t)ne * 18 * 8);
    s.Hll = (double*)take((size_t)nl * 6 * 8);
    s.bl = (double*)take((size_t)nl * 3 * 8);
    s.Hinv = (double*)take((size_t)nl * 6 * 8);
    s.Hpp = (double*)take((size_t)nf * 36 * 8);
    s.bp = (double*)take((size_t)nf * 6 * 8);
    s.posemax = (double*)take((size_t)nf * 8);
    s.Sp = (double*)take((size_t)nch * (n + 1) * n * 8);
    s.S = (double*)take((n + 1) * n * 8);
    s.dx = (double*)take(n * 8);
    s.pchi = (double*)take(nbe * 8);
    s.pscale = (double*)take(nbl * 8);
    s.pmax = (double*)take(nbl * 8);
    s.scal = (double*)take(8 * 8);
    s.flags = (uint8_t*)take((size_t)ne);
    s.lact = (uint8_t*)take((size_t)nl);
    s.factive = (uint8_t*)take((size_t)nf);
    s.flist = (int2*)take((size_t)ne * sizeof(int2));
    s.fcnt = (int*)take((size_t)nl * sizeof(int));
    s.cnt = (int*)take(4 * sizeof(int));
    s.bytes = pk.off;
    return s;
}
size_t ba_scratch_bytes(int nk, int nl, int ne, int nf) { return ba_carve(nullptr, nk, nl, ne, nf).bytes; }

#define BA_HIP(x)                       \
    do {                                \
        const hipError_t e_ = (x);      \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// The two optimize() calls and the classifications. Everything is queued on
// `st`; the host waits only for the scalars of a trial (h_scal, pinned).
hipError_t ba_run(hipStream_t st, const BaArgs& a, const odo_ba_params& p, odo_ba_result* res) {
    const int nk = a.nk, nl = a.nl, ne = a.ne, nf = a.nf, n = 6 * nf;
    BaScratch s = ba_carve((uint8_t*)a.scratch, nk, nl, ne, nf);
    BaGraph g{nk, nl, ne, nf, a.ekf, a.elm, a.eobs, a.lstart, a.lorder, a.kstart, a.korder, a.pidx};
    const BaCam cam{a.fx, a.fy, a.cx, a.cy, a.bf};
    int chunk;
    const int nch = ba_nchunks(nl, &chunk);
    const int nbe = (ne + BA_BLOCK - 1) / BA_BLOCK, nbl = (nl + BA_BLOCK - 1) / BA_BLOCK;
    const int nball = (std::max(std::max(nk, nl), ne) + BA_BLOCK - 1) / BA_BLOCK;
    const double dMono = (double)p.huber_mono, dStereo = (double)p.huber_stereo;
    double* h = a.h_scal;
    int cur = 0;

    BA_HIP(hipMemsetAsync(s.cnt, 0, 4 * sizeof(int), st));
    BA_HIP(hipMemsetAsync(s.scal, 0, 8 * sizeof(double), st));
    hipLaunchKernelGGL(k_ba_init, dim3(nball), dim3(BA_BLOCK), 0, st, g, a.Tcw, a.Xw, s.P[0], s.X[0], s.info, s.flags);

    auto read_scal = [&]() -> hipError_t {
        BA_HIP(hipGetLastError());
        BA_HIP(hipMemcpyAsync(h, s.scal, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        return hipStreamSynchronize(st);
    };
    // SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg
    // (the schedule of oracle/pose_ref.cpp:804-851 over the joint system)
    auto optimize = [&](int iters, int robust, int32_t* n_iters, int32_t* n_trials, double* chi_first,
                        double* chi_last) -> hipError_t {
        hipLaunchKernelGGL(k_ba_error, dim3(nbe), dim3(BA_BLOCK), 0, st, g, cam, s.P[cur], s.X[cur], s.info, s.flags, robust,
                           dMono, dStereo, s.c2, s.pchi);
        hipLaunchKernelGGL(k_ba_final, dim3(1), dim3(BA_BLOCK), 0, st, s.pchi, nbe, s.pscale, 0, s.scal);
        BA_HIP(read_scal());
        double curChi = h[0], lambda = 0, ni = 2;
        *chi_first = curChi;
        for (int it = 0; it < iters; it++) {
            hipLaunchKernelGGL(k_ba_linearize, dim3(nbl), dim3(BA_BLOCK), 0, st, g, cam, s.P[cur], s.X[cur], s.info, s.flags,
                               robust, dMono, dStereo, s.Hll, s.bl, s.W, s.lact, s.flist, s.fcnt, s.pmax);
            if (nk)
                hipLaunchKernelGGL(k_ba_pose, dim3(nk), dim3(64), 0, st, g, cam, s.P[cur], s.X[cur], s.info, s.flags, robust,
                                   dMono, dStereo, s.Hpp, s.bp, s.posemax, s.factive);
            if (it == 0) {
                hipLaunchKernelGGL(k_ba_maxdiag, dim3(1), dim3(BA_BLOCK), 0, st, s.pmax, nbl, s.posemax, nf, s.scal);
                BA_HIP(read_scal());
                lambda = 1e-5 * h[4];
                ni = 2;
            }
            double rho = 0;
            int qmax = 0;
            do {
                const int tr = cur ^ 1;
                hipLaunchKernelGGL(k_ba_hinv, dim3(nbl), dim3(BA_BLOCK), 0, st, nl, s.Hll, s.lact, lambda, s.Hinv);
                if (n) {
                    hipLaunchKernelGGL(k_ba_schur, dim3(nch), dim3(BA_BLOCK), 0, st, g, n, chunk, s.lact, s.flist, s.fcnt, s.Hinv, s.bl,
                                       s.W, s.Sp);
                    hipLaunchKernelGGL(k_ba_reduce, dim3(((n + 1) * n + BA_BLOCK - 1) / BA_BLOCK), dim3(BA_BLOCK), 0, st, n, nch,
                                       s.Sp, s.Hpp, s.bp, s.factive, lambda, s.S);
                    hipLaunchKernelGGL(k_ba_ldlt, dim3(1), dim3(BA_LDLT_THREADS), 0, st, n, s.S, s.dx, s.scal);
                }
                hipLaunchKernelGGL(k_ba_pose_update, dim3(1), dim3(BA_BLOCK), 0, st, g, s.P[cur], s.P[tr], s.dx, s.factive, s.bp,
                                   lambda, s.scal);
                hipLaunchKernelGGL(k_ba_backsub, dim3(nbl), dim3(BA_BLOCK), 0, st, g, s.X[cur], s.X[tr], s.flags, s.lact, s.Hinv,
                                   s.bl, s.W, s.dx, lambda, s.scal, s.pscale);
                hipLaunchKernelGGL(k_ba_error, dim3(nbe), dim3(BA_BLOCK), 0, st, g, cam, s.P[tr], s.X[tr], s.info, s.flags,
                                   robust, dMono, dStereo, s.c2, s.pchi);
                hipLaunchKernelGGL(k_ba_final, dim3(1), dim3(BA_BLOCK), 0, st, s.pchi, nbe, s.pscale, nbl, s.scal);
                BA_HIP(read_scal());
                double tempChi = h[0];
                if (h[2] != 0.0) tempChi = 1.7976931348623157e308;
                const double scale = (h[3] + h[1]) + 1e-3;
                rho = (curChi - tempChi) / scale;
                if (rho > 0 && std::isfinite(tempChi)) {
                    double alpha = 1. - std::pow(2 * rho - 1, 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2;
                    curChi = tempChi;
                    cur = tr;  // accept: the trial buffer becomes the estimate
                } else {
                    lambda *= ni;
                    ni *= 2;  // reject: the estimate's buffer is untouched
                }
                qmax++;
                (*n_trials)++;
            } while (rho < 0 && qmax < 10);
            (*n_iters)++;
            if (qmax == 10 || rho == 0) break;
        }
        *chi_last = curChi;
        return hipSuccess;
    };

    res->iters1 = res->iters2 = res->trials1 = res->trials2 = 0;
    res->n_erase = res->n_level1 = 0;
    BA_HIP(optimize(p.iters_robust, p.robust ? 1 : 0, &res->iters1, &res->trials1, &res->chi2_initial, &res->chi2_stage1));
    res->chi2_final = res->chi2_stage1;
    const double thMono = (double)p.chi2_mono, thStereo = (double)p.chi2_stereo;
    if (p.iters_final > 0) {
        hipLaunchKernelGGL(k_ba_classify, dim3(nbe), dim3(BA_BLOCK), 0, st, g, s.P[cur], s.X[cur], s.c2, thMono, thStereo, 0,
                           s.flags, a.erase, s.cnt);
        BA_HIP(hipGetLastError());
        int cnt[4];
        BA_HIP(hipMemcpyAsync(h, s.cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
        BA_HIP(hipStreamSynchronize(st));
        memcpy(cnt, h, sizeof(cnt));
        res->n_level1 = cnt[0];
        if (cnt[0] < ne) {  // initializeOptimization(0) found active edges
            double first;
            BA_HIP(optimize(p.iters_final, 0, &res->iters2, &res->trials2, &first, &res->chi2_final));
        }
    }
    hipLaunchKernelGGL(k_ba_classify, dim3(nbe), dim3(BA_BLOCK), 0, st, g, s.P[cur], s.X[cur], s.c2, thMono, thStereo, 1, s.flags,
                       a.erase, s.cnt);
    hipLaunchKernelGGL(k_ba_output, dim3(nball), dim3(BA_BLOCK), 0, st, g, s.P[cur], s.X[cur], a.Tcw, a.insys, a.oT, a.oX);
    BA_HIP(hipGetLastError());
    BA_HIP(hipMemcpyAsync(a.counts, s.cnt, 4 * sizeof(int), hipMemcpyDeviceToDevice, st));
    return hipSuccess;
}

}  // namespace odo
