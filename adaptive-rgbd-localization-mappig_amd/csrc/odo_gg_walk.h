// The uniform-grid neighbour search shared by k_gicp.hip (GICP covariances,
// SOR, the fitness score) and k_icp.hip (point-to-plane ICP): the float squared
// distance, the cell of a point and the ring walk over a cloud's cell-ordered
// rows (GgCloud in odo_internal.h; DESIGN §4 "Dense GICP").
#pragma once

#include <hip/hip_runtime.h>

#include "odo_internal.h"

namespace odo {

__device__ __forceinline__ float dist2f(const float* a, const float* b) {
    float r = 0.f, d;
    d = a[0] - b[0];
    r += d * d;
    d = a[1] - b[1];
    r += d * d;
    d = a[2] - b[2];
    r += d * d;
    return r;
}

__device__ __forceinline__ void gg_cell3(const GgCloud& g, const float* p, int* c) {
    const int dim[3] = {g.gx, g.gy, g.gz};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float t = (p[a] - g.mn[a]) * g.inv;
        c[a] = (int)fminf(fmaxf(floorf(t), 0.f), (float)(dim[a] - 1));  // outside (a query): clipped
    }
}

// The ring walk, once: every point of the cells at Chebyshev distance 0, 1, 2
// ... from cell c goes to v.visit(row of `sorted`), and after ring r the walk
// stops when the k-th distance the visitor holds (v.kth(), +inf while it holds
// fewer) is STRICTLY below what any unseen point can have (gg_ring_bound), or
// when the rings have covered the grid. c is gg_cell3 of the query. For a query
// q outside the cloud's bounds that is also the cell of q', q clamped per axis
// into the bounds (the computed t is monotone in the coordinate and the
// bounds' own cells are 0 and dim - 1), and |p_a - q_a| >= |p_a - q'_a| for
// every point p of the cloud and every axis a, so the bound that holds for q'
// holds for any finite q (DESIGN §4 "SOR and fitness").
template <class V>
__device__ __forceinline__ void gg_walk(const GgCloud& g, const int* __restrict__ cs,
                                        const float4* __restrict__ sorted, const int* c, V& v) {
    const int rmax = max(max(max(c[0], g.gx - 1 - c[0]), max(c[1], g.gy - 1 - c[1])), max(c[2], g.gz - 1 - c[2]));
    for (int r = 0;; r++) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.gz - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.gy - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.gx - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                const int row = (z * g.gy + y) * g.gx;
                // a row on the shell's z or y faces is one run of cells, any
                // other row has the shell's two x faces
                const bool full = abs(z - c[2]) == r || abs(y - c[1]) == r;
                for (int k = 0; k < 2; k++) {
                    int xa = x0, xb = x1;
                    if (full) {
                        if (k) break;
                    } else {
                        xa = xb = k ? c[0] + r : c[0] - r;
                        if (xa < 0 || xa > g.gx - 1) continue;
                    }
                    const int e = cs[row + xb + 1];
                    for (int i = cs[row + xa]; i < e; i++) v.visit(sorted[i]);
                }
            }
        if (r >= rmax || (double)v.kth() < gg_ring_bound(g.w, g.slack, r)) break;
    }
}

}  // namespace odo
