// The pieces the window searches share (k_localmap.hip, k_fuse.hip): the
// projection of a landmark into a frame, the Hamming distance, and the
// uniform keypoint grid: a frame's undistorted keypoints are counting-sorted
// into row-major cells of LmGrid, so the cells a window covers in one cell
// row are one contiguous run of the sorted points. Device only.
#pragma once

#include "odo_device.h"
#include "odo_internal.h"
#include "odo_wave.h"

namespace odo {

// The projection include/odo.h pins. The camera-frame point is the folded gemm
// Rcw * X + tcw, accumulated in double in this order and rounded once; invz is
// 1 / z whatever z's sign (the callers test !(z < 0) first, and their bounds
// tests differ, so both stay with them). The pixel comes in two operation
// orders, each pinned for its caller: do not merge them.
struct LmkCam {
    float x, y, z, invz;
};
struct LmkPix {
    float u, v, ur;
};
ODO_INLINE LmkCam lmk_camera(const float* T, const float* X) {
    float Pc[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        Pc[k] = (float)((((double)T[4 * k] * X[0] + (double)T[4 * k + 1] * X[1]) + (double)T[4 * k + 2] * X[2]) +
                        (double)T[4 * k + 3]);
    return LmkCam{Pc[0], Pc[1], Pc[2], 1.0f / Pc[2]};
}
// Frame::isInFrustum (frame.cpp:100-133): (fx * x) * invz + cx
ODO_INLINE LmkPix lmk_pixel_frustum(const LmkCam& P, const LmCalib& C) {
    const float u = C.fx * P.x * P.invz + C.cx;
    const float v = C.fy * P.y * P.invz + C.cy;
    return LmkPix{u, v, u - C.mbf * P.invz};
}
// Matcher::Fuse (matcher.cpp:231-244): fx * (x * invz) + cx
ODO_INLINE LmkPix lmk_pixel_fuse(const LmkCam& P, const LmCalib& C) {
    const float x = P.x * P.invz, y = P.y * P.invz;
    const float u = C.fx * x + C.cx, v = C.fy * y + C.cy;
    return LmkPix{u, v, u - C.mbf * P.invz};
}

ODO_INLINE int lmk_hamming(const uint32_t* a, const uint8_t* b8) {
    const uint4* b = reinterpret_cast<const uint4*>(b8);
    const uint4 x = b[0], y = b[1];
    return __popc(a[0] ^ x.x) + __popc(a[1] ^ x.y) + __popc(a[2] ^ x.z) + __popc(a[3] ^ x.w) + __popc(a[4] ^ y.x) +
           __popc(a[5] ^ y.y) + __popc(a[6] ^ y.z) + __popc(a[7] ^ y.w);
}

// cell of coordinate t (relative to the grid origin), clamped: monotone in t,
// so a point inside [lo, hi] lies in a cell of [cell(lo), cell(hi)]
ODO_INLINE int lmk_cell(float t, float inv, int g) {
    return (int)fminf(fmaxf(floorf(t * inv), 0.0f), (float)(g - 1));
}
ODO_INLINE int lmk_cell_of(float x, float y, const LmGrid& G) {
    return lmk_cell(y - G.y0, G.inv, G.gy) * G.gx + lmk_cell(x - G.x0, G.inv, G.gx);
}

// The counting sort, by one workgroup: the n points K (x, y rows) into the
// cells of G. s_cnt is ncells + 1 LDS words; cs receives the ncells + 1 cell
// starts; emit(pos, j, x, y) stores point j at sorted position pos. The order
// inside a cell is whatever the atomics give: the searches decide by keys.
template <class Emit>
ODO_INLINE void lmk_bin(const float* __restrict__ K, int n, const LmGrid& G, int* s_cnt, int* __restrict__ cs,
                        Emit emit) {
    const int ncells = G.gx * G.gy;
    for (int c = threadIdx.x; c <= ncells; c += blockDim.x) s_cnt[c] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) atomicAdd(&s_cnt[lmk_cell_of(K[2 * j], K[2 * j + 1], G)], 1);
    __syncthreads();
    // exclusive scan by wave 0: a run of cells per lane, then the lanes' totals
    if (threadIdx.x < 64) {
        const int per = (ncells + 63) / 64, c0 = min((int)threadIdx.x * per, ncells), c1 = min(c0 + per, ncells);
        int sum = 0;
        for (int c = c0; c < c1; c++) sum += s_cnt[c];
        const int inc = wave_incl_scan_shfl(sum, (int)threadIdx.x);
        int run = inc - sum;
        for (int c = c0; c < c1; c++) {
            const int t = s_cnt[c];
            s_cnt[c] = run;
            run += t;
        }
        if (threadIdx.x == 63) s_cnt[ncells] = inc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= ncells; c += blockDim.x) cs[c] = s_cnt[c];
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const float x = K[2 * j], y = K[2 * j + 1];
        emit(atomicAdd(&s_cnt[lmk_cell_of(x, y, G)], 1), j, x, y);
    }
}

// the cells a +-th window around (u, v) can touch; one pixel of margin covers
// the rounding of u +- th against the window test's own fabsf(x - u) < th
struct LmkRange {
    int cx0, cx1, cy0, cy1;
};
ODO_INLINE LmkRange lmk_range(float u, float v, float th, const LmGrid& G) {
    LmkRange r;
    r.cx0 = lmk_cell((u - th - 1.0f) - G.x0, G.inv, G.gx);
    r.cx1 = lmk_cell((u + th + 1.0f) - G.x0, G.inv, G.gx);
    r.cy0 = lmk_cell((v - th - 1.0f) - G.y0, G.inv, G.gy);
    r.cy1 = lmk_cell((v + th + 1.0f) - G.y0, G.inv, G.gy);
    return r;
}
// GetFeaturesInArea's test (frame.cpp:258-274); false for a NaN u, v or th
ODO_INLINE bool lmk_in_window(float x, float y, float u, float v, float th) {
    const float dx = x - u, dy = y - v;
    return fabsf(dx) < th && fabsf(dy) < th;
}
// fn(k) for the sorted positions k of the range's cells that lie in
// [k_lo, k_hi): per cell row one run of the cell starts s_cs, walked from its
// first + first in steps of step
template <class Fn>
ODO_INLINE void lmk_for_window(const LmkRange& r, const int* s_cs, const LmGrid& G, int k_lo, int k_hi, int first,
                               int step, Fn fn) {
    for (int cy = r.cy0; cy <= r.cy1; cy++) {
        const int e = min(s_cs[cy * G.gx + r.cx1 + 1], k_hi);
        for (int k = max(s_cs[cy * G.gx + r.cx0], k_lo) + first; k < e; k += step) fn(k);
    }
}

}  // namespace odo
