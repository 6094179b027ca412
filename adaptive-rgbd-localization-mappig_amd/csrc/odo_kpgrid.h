// The uniform keypoint grid of the window searches (k_localmap.hip,
// k_fuse.hip): a frame's undistorted keypoints are counting-sorted into
// row-major cells of LmGrid, so the cells a window covers in one cell row are
// one contiguous run of the sorted points. Device only.
#pragma once

#include "odo_device.h"
#include "odo_internal.h"

namespace odo {

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

}  // namespace odo
