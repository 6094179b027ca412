// Wave and workgroup building blocks shared by every kernel file: the wave
// prefix sum, a lane's rank under a ballot, the wave-scope LDS fence, the
// workgroup exclusive scans and ordered rank, the order-preserving float key
// and the border reflection. One definition of each; kernels add none.
#pragma once

#include "odo_device.h"

namespace odo {

// ------------------------------------------------------------------- waves
// inclusive prefix sum over the wave's 64 lanes (DPP: row shifts, then the row
// totals broadcast into the rows above). Every lane of the wave must be active.
ODO_INLINE int wave_incl_scan(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return x;
}
// the same sum as six dependent ds_bpermute round trips (lane: this lane's
// index in its wave)
ODO_INLINE int wave_incl_scan_shfl(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

// base + the lanes below this one among the set bits of a ballot
ODO_INLINE int lane_rank(uint64_t ballot, uint32_t base = 0u) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, base));
}

// LDS written by one lane of a wave, read by another lane of the same wave
ODO_INLINE void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// -------------------------------------------------------------- workgroups
// Exclusive scans in threadIdx order: the waves' scans, then the wave totals
// in one LDS step. Returns this thread's prefix and the workgroup's total.
// NT: the workgroup's threads (a multiple of 64) when the caller knows them at
// compile time, else 0 for blockDim.x. tmp: one int of LDS per wave and value.
// Every thread of the workgroup calls these.
template <int NT = 0, bool SHFL = false>
ODO_INLINE int block_exclusive_scan(int v, int* tmp, int* total) {
    const int nw = NT ? NT / 64 : ((int)blockDim.x + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = SHFL ? wave_incl_scan_shfl(v, lane) : wave_incl_scan(v);
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; w++) {
        const int sw = tmp[w];
        if (w < wave) base += sw;
        tot += sw;
    }
    *total = tot;
    __syncthreads();
    return base + x - v;
}
template <int NT = 0, bool SHFL = false>
ODO_INLINE int2 block_exclusive_scan2(int a, int b, int* tmp, int2* total) {
    const int nw = NT ? NT / 64 : ((int)blockDim.x + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xa = SHFL ? wave_incl_scan_shfl(a, lane) : wave_incl_scan(a);
    const int xb = SHFL ? wave_incl_scan_shfl(b, lane) : wave_incl_scan(b);
    if (lane == 63) tmp[wave] = xa, tmp[nw + wave] = xb;
    __syncthreads();
    int ba = 0, bb = 0, ta = 0, tb = 0;
    for (int w = 0; w < nw; w++) {
        const int sa = tmp[w], sb = tmp[nw + w];
        if (w < wave) ba += sa, bb += sb;
        ta += sa;
        tb += sb;
    }
    *total = int2{ta, tb};
    __syncthreads();
    return int2{ba + xa - a, bb + xb - b};
}

// ordered rank of `keep` among the workgroup's threads (thread order) and the
// total: a ballot per wave, not a scan of counts. ws: one int of LDS per wave
ODO_INLINE int block_rank(bool keep, int* ws, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const uint64_t b = __ballot(keep);
    if (lane == 0) ws[wv] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < nw; k++) {
        const int c = ws[k];
        if (k < wv) base += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + lane_rank(b);
}

// ------------------------------------------------------------------ scalars
// floats as uint32 whose unsigned order is the floats' order (-0 below +0):
// keys for integer sorts and for bounds kept by atomicMin / atomicMax
ODO_INLINE uint32_t f32_ordered(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ ODO_INLINE float f32_unordered(uint32_t u) {
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// BORDER_REFLECT_101 of index i into [0, n)
ODO_INLINE int reflect101(int i, int n) {
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}
// one reflection (|overshoot| < n): branch-free
ODO_INLINE int reflect101_1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

}  // namespace odo
