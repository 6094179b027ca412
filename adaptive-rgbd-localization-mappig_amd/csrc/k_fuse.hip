// The search of Matcher::Fuse (Features/matcher.cpp:212-291) for every Fuse
// call of LocalMapping::FuseLandmarks (System/localmapping.cpp:155-180) at
// once: call k projects the landmarks of its list into keyframe k, takes
// KeyFrame::GetFeaturesInArea's window (Core/frame.cpp:258-274), drops the
// keypoints beyond the reprojection gate (matcher.cpp:260-282) and keeps the
// Hamming minimum. What Fuse then does to the map (AddObservation, Replace)
// stays with the caller, who replays the calls in order; for that the gated
// set itself is returned (its size and its 8 lowest keypoint indices): a
// Replace in an earlier call changes a landmark's descriptor, never its
// projection, so only the minimum over that set has to be taken again
// (odo_fuse_best, DESIGN.md §4 Fuse).
//
//   k_fuse_bin     one workgroup per call: the keyframe's keypoints
//                  counting-sorted into the uniform grid (lmk_bin, odo_kpgrid.h),
//                  each sorted point with its right coordinate and its index
//   k_fuse_search  one thread per (call, list entry): the projection
//                  (lmk_camera, lmk_pixel_fuse, odo_kpgrid.h), then the grid
//                  cells under the window; the sorted points pass through
//                  LDS FZ_CHUNK at a time, a descriptor is read only for a
//                  gated keypoint. Grid order is not keypoint order: the best
//                  is the minimum of the key distance << 13 | index, the
//                  candidates the 8 smallest indices by a sorted insert
#include "odo_device.h"
#include "odo_internal.h"
#include "odo_kpgrid.h"

namespace odo {

#define FZ_CHUNK 2048  // sorted keypoints staged in LDS at a time (32 KiB)

__global__ void __launch_bounds__(256) k_fuse_bin(const odo_fuse_kf* __restrict__ kfs, const float* __restrict__ kun,
                                                  const float* __restrict__ ur, const int32_t* __restrict__ kp_off,
                                                  LmGrid G, float4* __restrict__ bpt, int* __restrict__ cstart) {
    extern __shared__ __attribute__((aligned(16))) int s_cnt[];  // ncells + 1
    const int c = blockIdx.x;
    const int k0 = kfs[c].kp_begin, n = kfs[c].kp_end - k0;
    const float* R = ur + k0;
    float4* out = bpt + kp_off[c];
    lmk_bin(kun + (size_t)k0 * 2, n, G, s_cnt, cstart + (size_t)c * (G.gx * G.gy + 1),
            [&](int pos, int j, float x, float y) { out[pos] = make_float4(x, y, R[j], __int_as_float(j)); });
}

__global__ void __launch_bounds__(256) k_fuse_search(const odo_fuse_kf* __restrict__ kfs,
                                                     const int32_t* __restrict__ kp_off,
                                                     const int32_t* __restrict__ rec_off,
                                                     const odo_landmark* __restrict__ lms, int n_lms,
                                                     const int32_t* __restrict__ lm_index,
                                                     const uint8_t* __restrict__ desc, const float4* __restrict__ bpt,
                                                     const int* __restrict__ cstart, LmGrid G, LmCalib C, float th,
                                                     odo_fuse_cand* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_fz[];
    float4* s_pt = reinterpret_cast<float4*>(s_fz);        // FZ_CHUNK
    int* s_cs = reinterpret_cast<int*>(s_pt + FZ_CHUNK);   // ncells + 1
    const int c = blockIdx.y, ncells = G.gx * G.gy;
    const int len = kfs[c].lm_end - kfs[c].lm_begin;
    if ((int)(blockIdx.x * blockDim.x) >= len) return;  // the whole workgroup: no barrier is left waiting
    const int k0 = kfs[c].kp_begin, n = kfs[c].kp_end - k0;
    for (int q = threadIdx.x; q <= ncells; q += blockDim.x) s_cs[q] = cstart[(size_t)c * (ncells + 1) + q];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = e < len;
    const float nan = __builtin_nanf("");
    float u = nan, v = nan, ur = nan;
    int nc = ODO_FUSE_NULL;
    uint32_t ld[8] = {};
    if (active) {
        const int li = lm_index[kfs[c].lm_begin + e];
        if (li >= 0 && li < n_lms) {
            const odo_landmark L = lms[li];
#pragma unroll
            for (int k = 0; k < 8; k++) ld[k] = reinterpret_cast<const uint32_t*>(L.desc)[k];
            const float* T = kfs[c].Tcw;
            nc = ODO_FUSE_BAD;
            if (!(L.flags & ODO_LM_BAD)) {
                // matcher.cpp:231-244: a NaN pixel fails these bounds, the upper ones are exclusive
                const LmkCam Pc = lmk_camera(T, L.X);
                nc = ODO_FUSE_BEHIND;
                if (!(Pc.z < 0.0f)) {
                    const LmkPix p = lmk_pixel_fuse(Pc, C);
                    nc = ODO_FUSE_OUTSIDE;
                    if (p.u >= C.minX && p.u < C.maxX && p.v >= C.minY && p.v < C.maxY) {
                        nc = 0;
                        u = p.u;
                        v = p.v;
                        ur = p.ur;
                    }
                }
            }
        }
    }
    const bool searched = active && nc == 0;
    LmkRange r{0, 0, 0, -1};
    if (searched) r = lmk_range(u, v, th, G);
    uint32_t best = 0xffffffffu;
    uint32_t cd[ODO_FUSE_CANDS];
#pragma unroll
    for (int k = 0; k < ODO_FUSE_CANDS; k++) cd[k] = 0xffffu;
    const uint8_t* D = desc + (size_t)k0 * 32;
    const float4* P = bpt + kp_off[c];
    for (int c0 = 0; c0 < n; c0 += FZ_CHUNK) {
        const int c1 = min(c0 + FZ_CHUNK, n);
        __syncthreads();  // the chunk before is read out (and s_cs is written, the first time round)
        for (int k = c0 + threadIdx.x; k < c1; k += blockDim.x) s_pt[k - c0] = P[k];
        __syncthreads();
        lmk_for_window(r, s_cs, G, c0, c1, 0, 1, [&](int k) {
            const float4 q = s_pt[k - c0];
            if (!lmk_in_window(q.x, q.y, u, v, th)) return;
            const float ex = u - q.x, ey = v - q.y;
            float e2 = ex * ex + ey * ey, lim = 5.99f;
            if (q.z >= 0.0f) {
                const float er = ur - q.z;
                e2 = e2 + er * er;
                lim = 7.8f;
            }
            if (e2 > lim) return;
            uint32_t j = (uint32_t)__float_as_int(q.w);
            best = min(best, ((uint32_t)lmk_hamming(ld, D + 32 * (size_t)j) << 13) | j);
            nc++;
            // sorted insert: cd stays the 8 smallest indices, ascending
#pragma unroll
            for (int k2 = 0; k2 < ODO_FUSE_CANDS; k2++) {
                const uint32_t lo = min(cd[k2], j);
                j = max(cd[k2], j);
                cd[k2] = lo;
            }
        });
    }
    if (!active) return;
    odo_fuse_cand o;
    o.u = u;
    o.v = v;
    o.ur = ur;
    o.n_cand = nc;
    o.best_idx = best == 0xffffffffu ? -1 : (int)(best & 0x1fff);
    o.best_dist = best == 0xffffffffu ? 0x7fffffff : (int)(best >> 13);
#pragma unroll
    for (int k = 0; k < ODO_FUSE_CANDS; k++) o.cand[k] = (uint16_t)cd[k];
    out[rec_off[c] + e] = o;
}

int launch_fuse_search(hipStream_t st, const FuseSearch& a) {
    if (a.max_kp > 8191) return -1;  // 13-bit keypoint index in a key
    if (a.n_kf <= 0) return 0;
    const int ncells = a.G.gx * a.G.gy;
    const size_t lds_bin = (size_t)(ncells + 1) * 4;
    const size_t lds_s = (size_t)FZ_CHUNK * sizeof(float4) + (size_t)(ncells + 1) * 4;
    hipLaunchKernelGGL(k_fuse_bin, dim3(a.n_kf), dim3(256), lds_bin, st, a.kfs, a.kun, a.ur, a.kp_off, a.G, a.bpt,
                       a.cstart);
    if (a.max_list > 0)
        hipLaunchKernelGGL(k_fuse_search, dim3((a.max_list + 255) / 256, a.n_kf), dim3(256), lds_s, st, a.kfs, a.kp_off,
                           a.rec_off, a.lms, a.n_lms, a.lm_index, a.desc, a.bpt, a.cstart, a.G, a.C, a.th, a.out);
    return 0;
}

}  // namespace odo
