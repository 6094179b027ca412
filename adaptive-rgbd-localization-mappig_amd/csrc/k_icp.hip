// libicp's IcpPointToPlane (Odometry/icp/icp.cpp, icpPointToPlane.cpp,
// matrix.cpp; run by Tests/IcpPointToPlane.cpp:81-119), dimension 3, batched
// over the grids of k_gicp.hip (DESIGN §4 "Point-to-plane ICP"; the contract and
// the pinned choices are in include/odo.h at odo_icp_plane_batch):
//   k_icp_normals  one lane per model point in cell order: its num_neighbors
//                  nearest model points by (distance, index) over the ring walk,
//                  a sorted list per lane in LDS (k is a run-time value, 3..32);
//                  mu, Q, H in float in that order, the eigenvector of H's
//                  smallest eigenvalue from svdj<3,3>, libicp's sign rule;
//   k_icp_sweep    grid (template point blocks, pairs), one lane per template
//                  point in cell order: R T + t in double, the float query, its
//                  nearest model point without a distance cap (k_gicp_fit_nn's
//                  search, ties to the lower index), the gate and the row of
//                  [A | b], written to the point's own row. One search serves
//                  getInliers and fitStep: they query at the same R, t;
//   k_icp_step     one workgroup per pair: A^T A and A^T b in double over the
//                  rows in POINT order (thread-strided partials, a wave
//                  butterfly, the four waves in order), rounded to float once;
//                  then odo_icp_step.h on one lane: solve, polar factor,
//                  composition, delta, the loop test, and the "done" latch that
//                  makes the pair's later sweeps return at once.
// The rows go through memory in point order, not through a reduction inside
// the sweep, because the lanes of a sweep are in the cell order of the counting
// sort, whose order within a cell is the atomics': sums over lanes would differ
// from run to run.
// After the loop one more sweep and step in "residual" mode give getResidual
// over the last active set.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "odo_gg_walk.h"
#include "odo_icp_step.h"
#include "odo_internal.h"
#include "odo_linalg.h"

namespace odo {
namespace {

constexpr int IC_LANES = 64;
constexpr int IC_THREADS = 256;  // k_icp_step
constexpr int IC_NV = 28;        // 21 of A^T A's upper triangle, 6 of A^T b, the residual

// the k nearest by (distance, index), ascending, entry j of lane l at
// nd / nn[j * 64 + l] (a lane's entries are a bank apart from its neighbours').
// +inf padding stands for "fewer than k so far"; its index 0 no candidate goes
// below, as CovTop20.
struct TopK {
    float pq[3];
    float* nd;
    int* nn;
    int k;
    __device__ __forceinline__ bool lt(float d, int idx, int j) const {
        const float dj = nd[j * IC_LANES];
        return d < dj || (d == dj && idx < nn[j * IC_LANES]);
    }
    __device__ __forceinline__ void visit(const float4 t) {
        const float pi[3] = {t.x, t.y, t.z};
        const int idx = __float_as_int(t.w);
        const float d = dist2f(pq, pi);
        if (!lt(d, idx, k - 1)) return;
        int j = k - 1;
        while (j > 0 && lt(d, idx, j - 1)) {
            nd[j * IC_LANES] = nd[(j - 1) * IC_LANES];
            nn[j * IC_LANES] = nn[(j - 1) * IC_LANES];
            j--;
        }
        nd[j * IC_LANES] = d;
        nn[j * IC_LANES] = idx;
    }
    __device__ __forceinline__ float kth() const { return nd[(k - 1) * IC_LANES]; }
};

// grid (point blocks, clouds), LDS 64 * k * 8 bytes: computeNormals of every
// cloud with need[cloud] != 0 and at least 5 points; normals 3 per point in
// point order
__global__ __launch_bounds__(IC_LANES) void k_icp_normals(const float* __restrict__ P, const GgCloud* __restrict__ cl,
                                                          const int* __restrict__ need,
                                                          const int* __restrict__ cstart,
                                                          const float4* __restrict__ sorted, int num_neighbors,
                                                          float* __restrict__ normals) {
    extern __shared__ float icp_top[];
    const GgCloud g = cl[blockIdx.y];
    const int s = blockIdx.x * IC_LANES + threadIdx.x;
    if (!need[blockIdx.y] || g.n < 5 || s >= g.n) return;
    const float4 me = sorted[(size_t)g.p0 + s];
    TopK v;
    v.pq[0] = me.x;
    v.pq[1] = me.y;
    v.pq[2] = me.z;
    v.k = min(num_neighbors, g.n);
    v.nd = icp_top + threadIdx.x;
    v.nn = (int*)(icp_top + IC_LANES * num_neighbors) + threadIdx.x;
    for (int j = 0; j < v.k; j++) {
        v.nd[j * IC_LANES] = __builtin_inff();
        v.nn[j * IC_LANES] = 0;
    }
    int c[3];
    gg_cell3(g, v.pq, c);
    gg_walk(g, cstart + g.c0, sorted, c, v);
    // computeNormal (icpPointToPlane.cpp:341-368) on Matrix's floats
    const float* Pk = P + 3 * (size_t)g.p0;
    float mu[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < v.k; j++) {
        const float* p = Pk + 3 * (size_t)v.nn[j * IC_LANES];
        mu[0] += p[0];
        mu[1] += p[1];
        mu[2] += p[2];
    }
    const float kf = (float)v.k;
    mu[0] /= kf;
    mu[1] /= kf;
    mu[2] /= kf;
    float H[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < v.k; j++) {
        const float* p = Pk + 3 * (size_t)v.nn[j * IC_LANES];
        const float q[3] = {p[0] - mu[0], p[1] - mu[1], p[2] - mu[2]};
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) H[3 * a + b] += q[a] * q[b];
    }
    double Hd[9], w[3], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Hd[i] = (double)H[i];
    svdj<3, 3>(Hd, w, nullptr, V);
    float n[3] = {(float)V[2], (float)V[5], (float)V[8]};
    // Matrix::svd's sign rule (matrix.cpp:853-867) for U = V: more than half of
    // the column's six entries negative, i.e. two or three of the normal's
    if ((n[0] < 0.f) + (n[1] < 0.f) + (n[2] < 0.f) >= 2) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
    float* o = normals + 3 * ((size_t)g.p0 + __float_as_int(me.w));
    o[0] = n[0];
    o[1] = n[1];
    o[2] = n[2];
}

// the nearest model point by (distance, index)
struct NearestIdx {
    float pq[3];
    float bd;
    int best;
    float bp[3];
    __device__ __forceinline__ void visit(const float4 t) {
        const float pi[3] = {t.x, t.y, t.z};
        const int idx = __float_as_int(t.w);
        const float d = dist2f(pq, pi);
        if (d < bd || (d == bd && idx < best)) {
            bd = d;
            best = idx;
            bp[0] = t.x;
            bp[1] = t.y;
            bp[2] = t.z;
        }
    }
    __device__ __forceinline__ float kth() const { return bd; }
};

// grid (template point blocks, pairs). rows: 8 words per template point at the
// pair's `work`, in point order: the float row a[6], b, and the active flag;
// in residual mode words 0-1 become the double n . (m - t) of an active point.
__global__ __launch_bounds__(IC_LANES) void k_icp_sweep(const GgCloud* __restrict__ cl,
                                                        const GgPair* __restrict__ pairs,
                                                        const int* __restrict__ cstart,
                                                        const float4* __restrict__ sorted,
                                                        const float* __restrict__ normals,
                                                        const IcpState* __restrict__ state, int gate, double indist0,
                                                        int residual, float* __restrict__ rows) {
    const GgPair pr = pairs[blockIdx.y];
    const GgCloud S = cl[pr.s], G = cl[pr.t];
    const int s = blockIdx.x * IC_LANES + threadIdx.x;
    if (s >= S.n) return;
    const IcpState st = state[blockIdx.y];
    if (st.status == ODO_ICP_NO_MODEL || st.status == ODO_ICP_SHORT_TEMPLATE) return;
    if (!residual && st.done) return;
    const float4 me = sorted[(size_t)S.p0 + s];
    float* row = rows + 8 * ((size_t)pr.work + __float_as_int(me.w));
    int active = 1;
    if (residual) {
        // the last active set (6: none before the first iteration with a gate)
        if (indist0 > 0) active = st.iter > 0 ? __float_as_int(row[7]) : 0;
        if (!active) {
            row[7] = __int_as_float(0);
            return;
        }
    }
    const double Tx = me.x, Ty = me.y, Tz = me.z;
    const double sx = (double)st.R[0] * Tx + (double)st.R[1] * Ty + (double)st.R[2] * Tz + (double)st.t[0];
    const double sy = (double)st.R[3] * Tx + (double)st.R[4] * Ty + (double)st.R[5] * Tz + (double)st.t[1];
    const double sz = (double)st.R[6] * Tx + (double)st.R[7] * Ty + (double)st.R[8] * Tz + (double)st.t[2];
    NearestIdx v;
    v.pq[0] = (float)sx;
    v.pq[1] = (float)sy;
    v.pq[2] = (float)sz;
    v.bd = __builtin_inff();
    v.best = 0;
    v.bp[0] = v.bp[1] = v.bp[2] = 0.f;
    int c[3];
    gg_cell3(G, v.pq, c);
    gg_walk(G, cstart + G.c0, sorted, c, v);
    const float* nf = normals + 3 * ((size_t)G.p0 + v.best);
    const double nx = nf[0], ny = nf[1], nz = nf[2];
    const double dx = v.bp[0], dy = v.bp[1], dz = v.bp[2];
    if (residual) {
        // getResidual (icpPointToPlane.cpp:442-471): the unrounded R T + t
        *(double*)row = nx * (dx - sx) + ny * (dy - sy) + nz * (dz - sz);
        row[7] = __int_as_float(1);
        return;
    }
    if (st.indist > 0) {
        // fitIterate's decay (icp.cpp:84), then getInliers (icpPointToPlane.cpp:299)
        const double ind = fmax(st.indist * 0.9, 0.05);
        if (gate == ODO_ICP_GATE_PLANE)
            active = fabs((sx - dx) * nx + (sy - dy) * ny + (sz - dz) * nz) < ind;
        else
            active = fabs((sx - dx) * nx + (sy - dy) * ny + (sz - dz)) * nz < ind;
    }
    // fitStep (icpPointToPlane.cpp:153-165): s is the float query read back
    const double qx = v.pq[0], qy = v.pq[1], qz = v.pq[2];
    row[0] = (float)(nz * qy - ny * qz);
    row[1] = (float)(nx * qz - nz * qx);
    row[2] = (float)(ny * qx - nx * qy);
    row[3] = (float)nx;
    row[4] = (float)ny;
    row[5] = (float)nz;
    row[6] = (float)(nx * dx + ny * dy + nz * dz - nx * qx - ny * qy - nz * qz);
    row[7] = __int_as_float(active);
}

// one workgroup per pair
__global__ __launch_bounds__(IC_THREADS) void k_icp_step(const GgCloud* __restrict__ cl,
                                                         const GgPair* __restrict__ pairs,
                                                         const float* __restrict__ rows, IcpState* __restrict__ state,
                                                         int max_iterations, double min_delta, int residual,
                                                         int* __restrict__ unfinished) {
    __shared__ double red[IC_THREADS / IC_LANES][IC_NV];
    __shared__ int redn[IC_THREADS / IC_LANES];
    const GgPair pr = pairs[blockIdx.x];
    const int ns = cl[pr.s].n;
    const IcpState st0 = state[blockIdx.x];  // uniform over the workgroup
    if (st0.status == ODO_ICP_NO_MODEL || st0.status == ODO_ICP_SHORT_TEMPLATE) return;
    if (!residual && st0.done) return;
    double v[IC_NV];
#pragma unroll
    for (int k = 0; k < IC_NV; k++) v[k] = 0;
    int nact = 0;
    const float* R = rows + 8 * (size_t)pr.work;
    for (int i = threadIdx.x; i < ns; i += IC_THREADS) {
        const float4 lo = *(const float4*)(R + 8 * (size_t)i), hi = *(const float4*)(R + 8 * (size_t)i + 4);
        if (!__float_as_int(hi.w)) continue;
        nact++;
        if (residual) {
            v[27] += *(const double*)(R + 8 * (size_t)i);
            continue;
        }
        const double a[6] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y}, b = hi.z;
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) v[k++] += a[p] * a[q];
#pragma unroll
        for (int p = 0; p < 6; p++) v[21 + p] += a[p] * b;
    }
    // the lanes of a wave by an xor butterfly (every lane ends with the same
    // bits), then the four waves in order on thread 0
#pragma unroll
    for (int k = 0; k < IC_NV; k++)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, IC_LANES);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nact += __shfl_xor(nact, o, IC_LANES);
    const int lane = threadIdx.x & (IC_LANES - 1), wave = threadIdx.x / IC_LANES;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < IC_NV; k++) red[wave][k] = v[k];
        redn[wave] = nact;
    }
    __syncthreads();
    if (threadIdx.x) return;
    double sum[IC_NV];
    for (int k = 0; k < IC_NV; k++) sum[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    nact = redn[0] + redn[1] + redn[2] + redn[3];
    IcpState st = st0;
    st.n_active = nact;
    if (residual) {
        st.residual = nact ? sum[27] / (double)nact : 0.0;
        state[blockIdx.x] = st;
        return;
    }
    float A[36], b[6];
    int k = 0;
    for (int p = 0; p < 6; p++)
        for (int q = p; q < 6; q++) A[6 * p + q] = A[6 * q + p] = (float)sum[k++];
    for (int p = 0; p < 6; p++) b[p] = (float)sum[21 + p];
    if (icp_solve6(A, b)) {
        st.delta = icp_compose(b, st.R, st.t);
        st.status = ODO_ICP_OK;
    } else {
        st.delta = 0.f;  // fitStep's failure return; R, t stay
        st.status = ODO_ICP_SINGULAR;
    }
    if (st.indist > 0) st.indist = fmax(st.indist * 0.9, 0.05);
    st.iter++;
    st.done = !(st.iter < max_iterations && (double)st.delta > min_delta);
    state[blockIdx.x] = st;
    if (st.done) atomicSub(unfinished, 1);
}

}  // namespace

void launch_icp_normals(hipStream_t st, const float* P, const GgCloud* cl, const int* need, int ncl, int max_n,
                        const int* cstart, const float4* sorted, int num_neighbors, float* normals) {
    if (ncl == 0 || max_n < 5) return;
    hipLaunchKernelGGL(k_icp_normals, dim3((max_n + IC_LANES - 1) / IC_LANES, ncl), dim3(IC_LANES),
                       (size_t)num_neighbors * IC_LANES * 8, st, P, cl, need, cstart, sorted, num_neighbors, normals);
}

void launch_icp_sweep(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, int max_ns,
                      const int* cstart, const float4* sorted, const float* normals, const IcpState* state, int gate,
                      double indist, int residual, float* rows) {
    if (nprob == 0 || max_ns == 0) return;
    hipLaunchKernelGGL(k_icp_sweep, dim3((max_ns + IC_LANES - 1) / IC_LANES, nprob), dim3(IC_LANES), 0, st, cl, pairs,
                       cstart, sorted, normals, state, gate, indist, residual, rows);
}

void launch_icp_step(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, const float* rows,
                     IcpState* state, int max_iterations, double min_delta, int residual, int* unfinished) {
    if (nprob == 0) return;
    hipLaunchKernelGGL(k_icp_step, dim3(nprob), dim3(IC_THREADS), 0, st, cl, pairs, rows, state, max_iterations,
                       min_delta, residual, unfinished);
}

}  // namespace odo
