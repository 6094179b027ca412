// Keypoint finalisation for gfx950: ORBextractor::operator()'s tail
// (Features/orbextractor.cpp:756-815) — IC_Angle (:14-39), computeOrbDescriptor
// (:43-85) on the Gaussian-blurred level, the level-0 scaling of the
// coordinates (:805-811) — and Frame::ExtractFeatures' per-keypoint geometry
// (Core/frame.cpp:139-164 UndistortKeyPoints / depth back-projection,
// :286-313).
//
//   k_finalize_lds  16 lanes per keypoint, 4 keypoints per wave, both patches
//                   staged in LDS; IC angle, rBRIEF and the descriptor store
//                   as odo_orb_patch.h describes them
//   k_kp_geometry   one keypoint per lane: undistortion (5 double iterations)
//                   and the depth back-projection, shared with the ADAPTIVE
//                   extractor's finalisation (k_adaptive.hip)
#include "odo_device.h"
#include "odo_internal.h"
#include "odo_orb_patch.h"
#ifndef ODO_EXTRACT_PRIO
#define ODO_EXTRACT_PRIO 0
#endif

namespace odo {

// k_finalize_lds: each keypoint's two patches (the IC disc of the level, the
// rBRIEF window of the blurred level) are staged in LDS by its 16 lanes with
// row-contiguous loads. Per-lane global loads would put the 16 lanes of a
// keypoint on 16 different rows, 64 cache lines per wave instruction through
// the texture path; staged, a wave instruction touches about two rows per
// keypoint, and the 512 rBRIEF samples become LDS byte reads.
// The tables, strides, rotation and descriptor store are odo_orb_patch.h's.
// The IC moment block and the rBRIEF sample loop are written out here, the
// text (and comments) of orb_ic_angle and orb_brief_samples there: a helper's
// loops are unrolled before it is inlined, and the kernel then compiles to
// other device text (three VALU per sample address instead of v_mad_u32_u24 +
// v_add3_u32). A change to either copy belongs in both.
template <int NW>  // waves (of 4 keypoints) per workgroup: 2 ships (a plain kernel compiles to other device text)
__global__ void __launch_bounds__(64 * NW) k_finalize_lds(const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur,
                                                      size_t pyr_stride, const LevelDesc* __restrict__ lv, int nlevels,
                                                      const uint32_t* __restrict__ okp, const int* __restrict__ ocnt,
                                                      int okp_stride, orb_kp* __restrict__ kps, uint8_t* __restrict__ desc,
                                                      int* __restrict__ nkp, int kp_cap, uint32_t gx_rcp) {
    if (ODO_EXTRACT_PRIO) __builtin_amdgcn_s_setprio(ODO_EXTRACT_PRIO);
    __shared__ uint64_t s_bal[NW][16];
    __shared__ __attribute__((aligned(16))) uint32_t s_disc[16][ORB_DISC_W];
    __shared__ __attribute__((aligned(16))) uint32_t s_patch[NW * ORB_KPW][ORB_KP_DW];
    orb_load_disc(s_disc, 64 * NW);
    // XCD remap (workgroup h runs on XCD h & 7: the eight XCDs take eight
    // contiguous runs of the (frame, block) list). gx_rcp = ceil(2^32 /
    // gridDim.x) from the host, exact for lid * gridDim.x < 2^32 (0: no
    // remap): the whole index computation stays on the scalar unit
    int bx = blockIdx.x, f = blockIdx.y;
    {
        const uint32_t gx = gridDim.x, total = gx * gridDim.y;
        if ((total & 7) == 0 && gx_rcp != 0) {
            const uint32_t h = blockIdx.x + blockIdx.y * gx;
            const uint32_t lid = (h & 7) * (total >> 3) + (h >> 3);
            f = (int)__umulhi(lid, gx_rcp);
            bx = (int)(lid - (uint32_t)f * gx);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, sub = lane & 15;
    const int kslot = wave * ORB_KPW + g;  // keypoint slot in the workgroup
    const int idx = bx * (NW * ORB_KPW) + kslot;
    // The keypoint's level and its index in the level from the levels'
    // inclusive count prefixes P_i (scalar: ocnt is read at uniform addresses,
    // the first eight counts by independent loads): the prefixes are
    // non-decreasing, so lvl = #{i : P_i <= idx}, and k = idx - P_(lvl-1) is the
    // smallest of idx and the differences idx - P_i taken mod 2^32 (those with
    // P_i > idx wrap to huge values). Past the last level both are unused.
    int lvl = 0, acc = 0;
    uint32_t ku = (uint32_t)idx;
    {
        const int* const oc = ocnt + f * nlevels;
        int c8[8];
#pragma unroll
        for (int i = 0; i < 8; i++) c8[i] = oc[i < nlevels ? i : nlevels - 1];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            acc += i < nlevels ? c8[i] : 0;
            lvl += idx >= acc ? 1 : 0;
            ku = min(ku, (uint32_t)idx - (uint32_t)acc);
        }
        for (int i = 8; i < nlevels; i++) {
            acc += oc[i];
            lvl += idx >= acc ? 1 : 0;
            ku = min(ku, (uint32_t)idx - (uint32_t)acc);
        }
    }
    const int k = (int)ku;
    const int total = acc < kp_cap ? acc : kp_cap;
    if (bx == 0 && threadIdx.x == 0) nkp[f] = total;
    if (bx * (NW * ORB_KPW) >= total) return;  // uniform over the workgroup
    const bool valid = idx < acc && idx < kp_cap;
    if (!valid) lvl = 0;
    const LevelDesc L = lv[lvl];
    // an invalid slot stages and reads a dummy in-level patch and writes nothing
    const uint32_t key = valid ? okp[((size_t)f * nlevels + lvl) * okp_stride + k] : (16u | (16u << 12));
    const int kx = (int)(key & 0xfff) + 16, ky = (int)((key >> 12) & 0xfff) + 16;
    const float resp = (float)(key >> 24);
    // Lanes sub < 15 as a fixed grid over each window's chunks —
    // the IC disc's 31 rows of 3 chunks (12 bytes, global_load_dwordx3) as 5
    // rows x 3 chunks per step, the rBRIEF window's 37 rows of 5 chunks (8
    // bytes, dwordx2) as 3 rows x 5 chunks per step — so every step is one
    // uniform address increment (5 or 3 rows): 7 + 13 loads per wave, as
    // 32-bit byte offsets from the frame's base (uniform over the workgroup:
    // scalar base + vector offset). Lane 15 and the rows past a window's end
    // load an in-window dummy and store nothing. (Walking the chunks 16 at a
    // time took 6 + 12 loads but ≈130 more VALU per wave for its wrap
    // selects; single-dword loads, 42 per wave, kept the texture address /
    // data units 93 % / 94 % busy: profiles/r05_l/pmcx_tex.)
    constexpr int IC_STEPS = 7, BR_STEPS = 13;
    uint2 vbr[BR_STEPS];  // the rBRIEF window's dwords (in flight during the IC angle)
    uint32_t* P = s_patch[kslot];
    const int sh = (kx - 15) & 3, sh2 = (kx - 18) & 3;
    const bool glane = sub < 15;
    const int ir = sub / 3, ic = sub - 3 * ir;  // IC: row in the step, chunk
    const int br = sub / 5, bc = sub - 5 * br;  // rBRIEF
    {
        const uint8_t* fpyr = pyr + (size_t)f * pyr_stride;
        const uint8_t* fblur = blur + (size_t)f * pyr_stride;
        const uint32_t pitch = (uint32_t)L.pitch;
        uint3 v[IC_STEPS];
        {
            const uint32_t o0 = (uint32_t)L.off + (uint32_t)(ky - 15) * pitch + (uint32_t)(kx - 15 - sh);
            uint32_t o = o0 + (uint32_t)ir * pitch + 12u * (uint32_t)ic;
#pragma unroll
            for (int j = 0; j < IC_STEPS; j++) {
                // rows ir + 5 j <= 30 for every lane (ir <= 5) until the last
                // step, which holds row 30 only (ir == 0)
                const bool ok = j + 1 < IC_STEPS || ir == 0;
                v[j] = *reinterpret_cast<const uint3*>(fpyr + (ok ? o : o0));
                o += 5u * pitch;
            }
        }
        {
            const uint32_t o0 = (uint32_t)L.off + (uint32_t)(ky - 18) * pitch + (uint32_t)(kx - 18 - sh2);
            uint32_t o = o0 + (uint32_t)br * pitch + 8u * (uint32_t)bc;
#pragma unroll
            for (int j = 0; j < BR_STEPS; j++) {
                // rows br + 3 j <= 36 for every lane (br <= 3) until the last
                // step, which holds row 36 only (br == 0)
                const bool ok = j + 1 < BR_STEPS || br == 0;
                vbr[j] = *reinterpret_cast<const uint2*>(fblur + (ok ? o : o0));
                o += 3u * pitch;
            }
        }
        {
            uint32_t* d = P + ir * ORB_IC_W + 3 * ic;
#pragma unroll
            for (int j = 0; j < IC_STEPS; j++) {
                if (glane && (j + 1 < IC_STEPS || ir == 0)) {
                    d[0] = v[j].x;
                    d[1] = v[j].y;
                    d[2] = v[j].z;
                }
                d += 5 * ORB_IC_W;
            }
        }
    }
    __syncthreads();  // s_disc, the patches
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
    const float angle = fast_atan2((float)m01, (float)m10);
    const float2 R = orb_rotation(angle);  // (cos, sin)
    const f32x2 BA = {R.y, R.x}, AB = {R.x, R.y}, MAG = {ORB_RND_MAGIC, ORB_RND_MAGIC};
    __syncthreads();  // every IC disc read
    {
        uint32_t* d = P + br * ORB_BR_W + 2 * bc;
#pragma unroll
        for (int j = 0; j < BR_STEPS; j++) {
            if (glane && (j + 1 < BR_STEPS || br == 0)) *reinterpret_cast<uint2*>(d) = vbr[j];
            d += 3 * ORB_BR_W;
        }
    }
    __syncthreads();
    const uint8_t* PB = reinterpret_cast<const uint8_t*>(P);
    const uint32_t cofs = (uint32_t)(18 * 4 * ORB_BR_W + 18 + sh2) - 0x400000u * (uint32_t)(4 * ORB_BR_W) - ORB_RND_BITS;  // mod 2^32
    int tv0[16], tv1[16];
    uint32_t pat8[16];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint4 q = reinterpret_cast<const uint4*>(c_pat8.w)[sub * 4 + u];
        pat8[4 * u] = q.x, pat8[4 * u + 1] = q.y, pat8[4 * u + 2] = q.z, pat8[4 * u + 3] = q.w;
    }
#pragma unroll
    for (int w = 0; w < 16; w++) {
        const uint32_t pw = pat8[w];
        const float4 Pt = orb_test_points(pw);
        f32x2 q0 = (f32x2){Pt.x, Pt.x} * BA + (f32x2){Pt.y, -Pt.y} * AB;
        f32x2 q1 = (f32x2){Pt.z, Pt.z} * BA + (f32x2){Pt.w, -Pt.w} * AB;
        q0 = q0 + MAG;
        q1 = q1 + MAG;
        const uint32_t o0 = __umul24(__float_as_uint(q0.x), (uint32_t)(4 * ORB_BR_W)) + __float_as_uint(q0.y) + cofs;
        const uint32_t o1 = __umul24(__float_as_uint(q1.x), (uint32_t)(4 * ORB_BR_W)) + __float_as_uint(q1.y) + cofs;
        tv0[w] = PB[o0];
        tv1[w] = PB[o1];
    }
    orb_store_desc(tv0, tv1, s_bal, wave, lane, valid, desc, f, kp_cap, idx);
    if (valid && sub == 0) {
        orb_kp* kp = kps + (size_t)f * kp_cap + idx;
        float px = (float)kx, py = (float)ky;
        if (lvl != 0) {
            px *= L.scale;
            py *= L.scale;
        }
        kp->x = px;
        kp->y = py;
        kp->size = (float)(int)(31 * L.scale);
        kp->angle = angle;
        kp->response = resp;
        kp->octave = lvl;
        kp->class_id = -1;
    }
}

// UndistortKeyPoints + depth back-projection (frame.cpp:139-164, 286-313) of
// every finalised keypoint, one per lane.
__global__ void __launch_bounds__(256) k_kp_geometry(const orb_kp* __restrict__ kps, const int* __restrict__ nkp,
                                                     const uint16_t* __restrict__ depth, size_t depth_stride, int img_w,
                                                     FrameCalib cal, float* __restrict__ kun, float* __restrict__ xyz,
                                                     float* __restrict__ ur, int kp_cap) {
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nkp[f]) return;
    const size_t o = (size_t)f * kp_cap + i;
    const float2 p = *reinterpret_cast<const float2*>(&kps[o].x);
    kp_geometry(p.x, p.y, cal, depth + (size_t)f * depth_stride, img_w, kun + o * 2, xyz + o * 3, ur + o);
}

void launch_kp_geometry(hipStream_t st, const orb_kp* kps, const int* nkp, const uint16_t* depth, size_t depth_stride,
                        int img_w, FrameCalib cal, float* kun, float* xyz, float* ur, int kp_cap, int nframes) {
    dim3 g((kp_cap + 255) / 256, nframes);
    hipLaunchKernelGGL(k_kp_geometry, g, dim3(256), 0, st, kps, nkp, depth, depth_stride, img_w, cal, kun, xyz, ur,
                       kp_cap);
}

void launch_finalize(hipStream_t st, const uint8_t* pyr, const uint8_t* blur, size_t pyr_stride, const LevelDesc* lv,
                     int nlevels, const uint32_t* okp, const int* ocnt, int okp_stride, const uint16_t* depth,
                     size_t depth_stride, int img_w, FrameCalib cal, orb_kp* kps, uint8_t* desc, float* kun, float* xyz,
                     float* ur, int* nkp, int kp_cap, int nframes, bool geometry) {
    // 2 waves (8 keypoints, 21 KB of LDS) per workgroup: more workgroups
    // resident per CU than at 4 waves (42.5 KB)
    const uint32_t gx = (uint32_t)(kp_cap + 7) / 8;
    const uint64_t ntot = (uint64_t)gx * (uint64_t)nframes;
    // the kernel's XCD remap divides by gx with this reciprocal (0: no remap)
    const uint32_t gx_rcp = gx > 1 && ntot * gx < (1ull << 32) ? (uint32_t)(((1ull << 32) + gx - 1) / gx) : 0u;
    hipLaunchKernelGGL(k_finalize_lds<2>, dim3(gx, nframes), dim3(128), 0, st, pyr, blur, pyr_stride, lv, nlevels, okp,
                       ocnt, okp_stride, kps, desc, nkp, kp_cap, gx_rcp);
    if (geometry) launch_kp_geometry(st, kps, nkp, depth, depth_stride, img_w, cal, kun, xyz, ur, kp_cap, nframes);
}

}  // namespace odo
