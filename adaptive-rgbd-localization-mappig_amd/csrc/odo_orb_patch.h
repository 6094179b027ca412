// The per-keypoint ORB patch code of the three finalize kernels
// (k_finalize_lds, k_oa_finalize, k_adapt_finalize): IC_Angle on a disc staged
// in LDS, the rBRIEF samples of a window staged in LDS, the ballot-to-descriptor
// store, and the two compile-time tables they read. Device code only.
// Lanes: 4 keypoints per wave, 16 lanes each (g = lane >> 4, sub = lane & 15),
// lane sub holding the tests w * 16 + sub. A kernel keeps its keypoint source,
// its global-to-LDS staging and its orb_kp; k_finalize_lds also a written-out
// copy of orb_ic_angle's and orb_brief_samples' bodies (k_finalize.hip: why).
#pragma once

#include "odo_device.h"
#include "../../include/odo_orb_pattern.h"

namespace odo {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 1.5 * 2^23: for |x| < 2^22, the float sum x + ORB_RND_MAGIC is x rounded half
// to even (cvRound) plus the magic, so its low mantissa bits are the integer.
constexpr float ORB_RND_MAGIC = 12582912.0f;
constexpr uint32_t ORB_RND_BITS = 0x4B400000u;
constexpr int ORB_KPW = 4;  // keypoints per wave

// Staged patches: the IC disc, rows y-15..y+15, 9 aligned dwords each; the
// rBRIEF window, rows y-18..y+18, 10 dwords each (rotated pattern points round
// into [-18, 18]).
constexpr int ORB_IC_W = 9, ORB_IC_N = 31 * ORB_IC_W;    // dwords per staged IC row, per disc (279)
constexpr int ORB_BR_W = 10, ORB_BR_N = 37 * ORB_BR_W;  // per staged rBRIEF row, per window (370)
// The rBRIEF window overwrites the IC disc once the angle is known, so a
// keypoint holds 370 dwords of LDS instead of 649 and more workgroups fit a CU.
// dwords of LDS per keypoint, padded to 16 mod 32: a wave's lanes 0-31 are two
// keypoints whose IC rows sit 9 dwords apart ({9s mod 32} for the 16 lanes:
// half the banks); the second keypoint 16 banks further takes exactly the
// other half ({16 + 9s}), where the unpadded 370 (18 mod 32) shared 14 of 16
// banks with the first (PMC: 35.7 M conflict cycles, 1.4x the kernel's LDS
// cycles)
constexpr int ORB_KP_DW = ((ORB_BR_N + 15) / 32) * 32 + 16;  // 400
// disc mask rows padded to 12 dwords: the 16 lanes of a ds_read_b128 group
// read 16 different rows, which at 8 dwords met on 2 banks each
constexpr int ORB_DISC_W = 12;

// ------------------------------------------------------------------ tables
// IC_Angle disc masks: row |v|'s dword i has byte bb set (0xff) where column
// u = 4 i + bb - 15 lies inside the disc, |u| <= umax[|v|].
struct DiscTab { uint32_t m[16 * 8]; };
constexpr DiscTab make_disc_tab() {
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    DiscTab T{};
    for (int av = 0; av < 16; av++)
        for (int i = 0; i < 8; i++) {
            uint32_t m = 0;
            for (int bb = 0; bb < 4; bb++) {
                const int u = 4 * i + bb - 15;
                if (u >= -umax[av] && u <= umax[av]) m |= 0xffu << (8 * bb);
            }
            T.m[av * 8 + i] = m;
        }
    return T;
}
static __constant__ DiscTab c_disc = make_disc_tab();

// ORB_SLAM2 pattern test t = (x0, y0, x1, y1) as signed bytes, lane-major:
// w[s * 16 + k] = test k * 16 + s (lane s's sixteen tests in 64 contiguous
// bytes)
struct alignas(16) PatTab { uint32_t w[256]; };
constexpr PatTab make_pat_tab() {
    PatTab T{};
    for (int s = 0; s < 16; s++)
        for (int k = 0; k < 16; k++) {
            const int t = k * 16 + s;
            uint32_t v = 0;
            for (int i = 0; i < 4; i++) v |= (uint32_t)(uint8_t)ODO_ORB_PATTERN[4 * t + i] << (8 * i);
            T.w[s * 16 + k] = v;
        }
    return T;
}
static __constant__ PatTab c_pat8 = make_pat_tab();

// The disc masks to LDS, one load per thread of a workgroup of nthreads
// (a barrier before the first orb_ic_angle is the caller's).
ODO_INLINE void orb_load_disc(uint32_t (*s_disc)[ORB_DISC_W], int nthreads) {
    for (int d = threadIdx.x; d < 128; d += nthreads) s_disc[d >> 3][d & 7] = c_disc.m[d];
}

// Lane sub's sixteen packed tests, and one of them as floats (exact).
ODO_INLINE void orb_lane_pattern(int sub, uint32_t (&pat8)[16]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint4 q = reinterpret_cast<const uint4*>(c_pat8.w)[sub * 4 + u];
        pat8[4 * u] = q.x, pat8[4 * u + 1] = q.y, pat8[4 * u + 2] = q.z, pat8[4 * u + 3] = q.w;
    }
}
ODO_INLINE float4 orb_test_points(uint32_t pw) {
    return {(float)(int8_t)(pw & 0xff), (float)(int8_t)((pw >> 8) & 0xff), (float)(int8_t)((pw >> 16) & 0xff),
            (float)(int8_t)(pw >> 24)};
}

// ---------------------------------------------------------------- IC angle
// IC_Angle of the keypoint whose disc its 16 lanes staged at P (ORB_IC_W
// dwords per row, the row's first byte sh bytes left of column -15): lane sub
// sums disc rows sub-15 and sub+1 - 9 aligned dwords per row realigned with
// alignbyte, bytes outside the disc masked, the moments by udot4 (exact
// integers) - then a 16-lane butterfly and fastAtan2. Every lane of the
// keypoint returns the angle in degrees.
ODO_INLINE float orb_ic_angle(const uint32_t* P, int sh, const uint32_t (*s_disc)[ORB_DISC_W], int sub) {
    int m10, m01;
    {
        const bool has1 = sub < 15;
        const int v0 = sub - 15, v1 = has1 ? sub + 1 : 0;
        const uint32_t* r0 = P + (v0 + 15) * ORB_IC_W;
        const uint32_t* r1 = P + (v1 + 15) * ORB_IC_W;
        uint32_t w0[9], w1[9];
#pragma unroll
        for (int i = 0; i < 9; i++) {
            w0[i] = r0[i];
            w1[i] = r1[i];
        }
        const uint4* M0 = reinterpret_cast<const uint4*>(s_disc[-v0]);
        const uint4* M1 = reinterpret_cast<const uint4*>(s_disc[v1]);
        const uint4 a0 = M0[0], a1 = M0[1], b0 = M1[0], b1 = M1[1];
        const uint32_t z = has1 ? 0xffffffffu : 0u;
        const uint32_t mk0[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const uint32_t mk1[8] = {b0.x & z, b0.y & z, b0.z & z, b0.w & z, b1.x & z, b1.y & z, b1.z & z, b1.w & z};
        uint32_t s0 = 0, s1 = 0, t = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t U = (uint32_t)(4 * i + 1) | ((uint32_t)(4 * i + 2) << 8) | ((uint32_t)(4 * i + 3) << 16) |
                               ((uint32_t)(4 * i + 4) << 24);
            const uint32_t d0 = __builtin_amdgcn_alignbyte(w0[i + 1], w0[i], sh) & mk0[i];
            const uint32_t d1 = __builtin_amdgcn_alignbyte(w1[i + 1], w1[i], sh) & mk1[i];
            s0 = __builtin_amdgcn_udot4(d0, 0x01010101u, s0, false);
            s1 = __builtin_amdgcn_udot4(d1, 0x01010101u, s1, false);
            t = __builtin_amdgcn_udot4(d0, U, t, false);
            t = __builtin_amdgcn_udot4(d1, U, t, false);
        }
        m10 = (int)t - 16 * (int)(s0 + s1);
        m01 = v0 * (int)s0 + v1 * (int)s1;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off);
        m01 += __shfl_xor(m01, off);
    }
    return fast_atan2((float)m01, (float)m10);
}

// ------------------------------------------------------------------ rBRIEF
// The descriptor's rotation: (cos, sin) of the angle (degrees) in the
// reference's arithmetic.
ODO_INLINE float2 orb_rotation(float angle) {
    const float factorPI = (float)(3.14159265358979323846 / 180.f);
    const float ang = angle * factorPI;
    double sd, cd;
    sincos((double)ang, &sd, &cd);
    return {(float)cd, (float)sd};
}

// Lane sub's 2 x 16 rBRIEF samples from the window staged at P (ORB_BR_W
// dwords per row, the row's first byte sh2 bytes left of column -18): the
// rotation in packed fp32, cvRound by the magic add. The staged byte of the
// rotated offset (iy, ix) is (iy + 18) * 40 + ix + 18 + sh2; the magic-rounded
// floats carry ORB_RND_BITS + offset in their bits.
ODO_INLINE void orb_brief_samples(const uint32_t* P, int sh2, float2 R, int sub, int (&tv0)[16], int (&tv1)[16]) {
    const f32x2 BA = {R.y, R.x}, AB = {R.x, R.y}, MAG = {ORB_RND_MAGIC, ORB_RND_MAGIC};
    const uint8_t* PB = reinterpret_cast<const uint8_t*>(P);
    // iy's low 24 bits are 0x400000 + dy (a 24-bit multiply: v_mad_u32_u24,
    // full rate, where the 32-bit product takes v_mad_u64_u32)
    const uint32_t cofs =
        (uint32_t)(18 * 4 * ORB_BR_W + 18 + sh2) - 0x400000u * (uint32_t)(4 * ORB_BR_W) - ORB_RND_BITS;  // mod 2^32
    uint32_t pat8[16];
    orb_lane_pattern(sub, pat8);
#pragma unroll
    for (int w = 0; w < 16; w++) {
        const float4 Pt = orb_test_points(pat8[w]);
        f32x2 q0 = (f32x2){Pt.x, Pt.x} * BA + (f32x2){Pt.y, -Pt.y} * AB;
        f32x2 q1 = (f32x2){Pt.z, Pt.z} * BA + (f32x2){Pt.w, -Pt.w} * AB;
        q0 = q0 + MAG;
        q1 = q1 + MAG;
        const uint32_t o0 = __umul24(__float_as_uint(q0.x), (uint32_t)(4 * ORB_BR_W)) + __float_as_uint(q0.y) + cofs;
        const uint32_t o1 = __umul24(__float_as_uint(q1.x), (uint32_t)(4 * ORB_BR_W)) + __float_as_uint(q1.y) + cofs;
        tv0[w] = PB[o0];
        tv1[w] = PB[o1];
    }
}

// -------------------------------------------------------------- descriptor
// The wave's four descriptors from its lanes' samples: bit w * 16 + sub of a
// keypoint is tv0[w] < tv1[w] of its lane sub. s_bal is the workgroup's
// [waves][16] 64-bit LDS words; the keypoint is slot o of frame f's kp_cap
// descriptors of 32 bytes, written if valid. CONTAINS A __syncthreads(): call
// it from control flow that is uniform over the workgroup.
// All sixteen ballots first (scalar registers), then lane 0 stores them in one
// block: a store after each ballot is sixteen exec-mask branch blocks that
// every wave enters. The empty asm keeps the stores 64 bits wide, one
// v_mov_b64 each: merged into 128-bit stores they take two 32-bit moves per
// ballot. The array and the indices are passed apart so that the LDS and
// descriptor addresses fold as they do written in the kernel.
ODO_INLINE void orb_store_desc(const int (&tv0)[16], const int (&tv1)[16], uint64_t (*s_bal)[16], int wave, int lane,
                               bool valid, uint8_t* __restrict__ desc, int f, int kp_cap, int o) {
    const int g = lane >> 4, sub = lane & 15;
    uint64_t bal[16];
#pragma unroll
    for (int w = 0; w < 16; w++) bal[w] = __ballot(tv0[w] < tv1[w]);
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < 16; w++) {
            s_bal[wave][w] = bal[w];
            asm volatile("" ::: "memory");
        }
    }
    __syncthreads();
    if (valid && sub < 8) {
        const uint32_t lo = (uint32_t)(s_bal[wave][2 * sub] >> (16 * g)) & 0xffffu;
        const uint32_t hi = (uint32_t)(s_bal[wave][2 * sub + 1] >> (16 * g)) & 0xffffu;
        reinterpret_cast<uint32_t*>(desc + ((size_t)f * kp_cap + o) * 32)[sub] = lo | (hi << 16);
    }
}

}  // namespace odo
