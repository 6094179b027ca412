// Tracking::TrackLocalMap for every frame of a batch (System/tracking.cpp:
// 231-261, 368-405): SearchLocalLMs (Frame::isInFrustum, frame.cpp:100-133,
// then Matcher(0.8f)::ProjectionMatch, matcher.cpp:90-145, over
// GetFeaturesInArea's window, frame.cpp:258-274) against one shared landmark
// array, the merge with the slots KnnMatch carried over, and the edge gather
// for the second PnPSolver::Compute (k_pnp, unchanged). One launch chain for
// all frames of a search: odo_track_local_map searches the frames of a batch
// where they sit, odo_projection_match one frame of host inputs. The
// projection, the grid and the window walk are odo_kpgrid.h's.
//
//   k_lm_prior    per frame: prior slots holding a BAD landmark are released
//                 (UpdateLocalKFs, tracking.cpp:270-276), the rest mark their
//                 landmark SEEN in the frame's bitmask (tracking.cpp:371-382)
//                 and their slot taken iff the landmark has observations
//                 (matcher.cpp:114-117); without a prior the taken slots are
//                 the caller's, or none
//   k_lm_bin      per frame: the undistorted keypoints counting-sorted into a
//                 uniform grid (row-major cells, so the cells a window covers
//                 in one cell row are one contiguous run of the sorted points)
//   k_lm_cands    one thread per (frame, landmark): the projection
//                 (lmk_camera, lmk_pixel_frustum), then only the grid cells under
//                 the window (the frame's sorted points staged in LDS); a
//                 candidate is the key distance << 18 | keypoint << 5 | octave,
//                 so the reference's stable best / second best are the two
//                 smallest keys of the untaken candidates
//   k_lm_resolve  one workgroup per frame. The reference's landmark loop is
//                 serial only through the slots earlier landmarks with
//                 observations took; it equals the fixed point of a
//                 synchronous relaxation: every landmark i chooses at once
//                 with slot j taken iff it was taken at the start or
//                 owner[j] < i, owner[j] the smallest index of a landmark with
//                 observations that chose j in the round before. Landmark i's
//                 choice depends on landmarks below i only, so by induction it
//                 is final after round i + 1: the loop ends (no choice
//                 changed) at the reference's result for every input (5-23
//                 rounds on the frames of tools/local_map_bench.py; the count
//                 is reported in odo_local_map_result.pad[0]). Lists of up to LMK_CAP
//                 candidates: a thread per landmark; longer ones: a wave per
//                 landmark over the window's cell runs, distances recomputed.
//                 Then slot_lm[j] = the largest index that chose j
//                 (AddLandmark overwrites), the merge with the prior, and the
//                 PnP edges: Xg[j] = the landmark's X, f2_src[j] = j or -1
//   k_lm_stats    after k_pnp: n_map_inliers, the outlier flags, the record
#include "odo_device.h"
#include "odo_internal.h"
#include "odo_kpgrid.h"

namespace odo {

#define LMK_CAP 16  // candidates kept per (frame, landmark); longer lists take the wave path
#define LMK_NONE 0xffffffffu
#define LMK_OBS (1 << 30)  // in a candidate count: the landmark has observations
#define LMK_NT 1024  // k_lm_resolve threads
#define LMK_NW (LMK_NT / 64)

// key order = (distance, keypoint index): keypoint 13 bits, octave 5, distance 9
ODO_INLINE uint32_t lmk_key(int j, int oct, int d) {
    return ((uint32_t)d << 18) | ((uint32_t)j << 5) | (uint32_t)(oct & 31);
}
ODO_INLINE void lmk_insert(uint32_t k, uint32_t& a1, uint32_t& a2) {
    a2 = min(a2, max(a1, k));  // the two smallest, as selects (branches put a1 / a2 in scratch)
    a1 = min(a1, k);
}
// matcher.cpp:126-141: TH_HIGH = 100 (matcher.cpp:15-17), the ratio test only
// between candidates of one level; returns the slot or -1
ODO_INLINE int lmk_decide(uint32_t k1, uint32_t k2, float nnratio) {
    if (k1 == LMK_NONE) return -1;
    const double best1 = (double)(k1 >> 18);
    if (!(best1 <= 100.0)) return -1;
    if (k2 != LMK_NONE && (k1 & 31) == (k2 & 31) && best1 > (double)nnratio * (double)(k2 >> 18)) return -1;
    return (int)((k1 >> 5) & 0x1fff);
}

__global__ void __launch_bounds__(256) k_lm_prior(const int32_t* __restrict__ prior, const odo_landmark* __restrict__ lms,
                                                  int nL, const uint8_t* __restrict__ taken_in,
                                                  const int* __restrict__ nkp, int kp_cap,
                                                  uint32_t* __restrict__ seen, int seen_words,
                                                  int32_t* __restrict__ prior_eff, uint8_t* __restrict__ taken0) {
    const int f = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kp_cap) return;
    const int n = min(nkp[f], kp_cap);
    int k = (prior && j < n) ? prior[(size_t)f * kp_cap + j] : -1;
    uint8_t tk = (!prior && taken_in && j < n) ? taken_in[(size_t)f * kp_cap + j] : 0;
    if (k < 0 || k >= nL) {
        k = -1;
    } else {
        const int fl = lms[k].flags;
        if (fl & ODO_LM_BAD) {
            k = -1;
        } else {
            atomicOr(&seen[(size_t)f * seen_words + (k >> 5)], 1u << (k & 31));
            tk = (fl & ODO_LM_HAS_OBS) ? 1 : 0;
        }
    }
    prior_eff[(size_t)f * kp_cap + j] = k;
    taken0[(size_t)f * kp_cap + j] = tk;
}

__global__ void __launch_bounds__(256) k_lm_bin(const float* __restrict__ kun, const int32_t* __restrict__ oct,
                                                int oct_stride, const int* __restrict__ nkp, int kp_cap, LmGrid G,
                                                float2* __restrict__ bxy, uint32_t* __restrict__ bjo,
                                                int* __restrict__ cstart) {
    extern __shared__ int s_cnt[];  // ncells + 1
    const int f = blockIdx.x;
    const int32_t* O = oct + (size_t)f * kp_cap * oct_stride;
    float2* xy = bxy + (size_t)f * kp_cap;
    uint32_t* jo = bjo + (size_t)f * kp_cap;
    lmk_bin(kun + (size_t)f * kp_cap * 2, min(nkp[f], kp_cap), G, s_cnt, cstart + (size_t)f * (G.gx * G.gy + 1),
            [&](int pos, int j, float x, float y) {
                xy[pos] = make_float2(x, y);
                jo[pos] = (uint32_t)j | ((uint32_t)(O[(size_t)j * oct_stride] & 31) << 16);
            });
}

__global__ void __launch_bounds__(256) k_lm_cands(const float* __restrict__ Tcw, const odo_landmark* __restrict__ lms,
                                                  int nL, const uint32_t* __restrict__ seen, int seen_words,
                                                  const int* __restrict__ nkp, int kp_cap,
                                                  const uint8_t* __restrict__ desc, const float2* __restrict__ bxy,
                                                  const uint32_t* __restrict__ bjo, const int* __restrict__ cstart,
                                                  LmGrid G, LmCalib C, float th, float* __restrict__ proj,
                                                  int* __restrict__ ccount, uint32_t* __restrict__ cand) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_lm[];
    const int f = blockIdx.y, ncells = G.gx * G.gy;
    const int n = min(nkp[f], kp_cap);
    float2* s_xy = reinterpret_cast<float2*>(s_lm);                       // kp_cap
    uint32_t* s_jo = reinterpret_cast<uint32_t*>(s_xy + kp_cap);          // kp_cap
    int* s_cs = reinterpret_cast<int*>(s_jo + kp_cap);                    // ncells + 1
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        s_xy[k] = bxy[(size_t)f * kp_cap + k];
        s_jo[k] = bjo[(size_t)f * kp_cap + k];
    }
    for (int c = threadIdx.x; c <= ncells; c += blockDim.x) s_cs[c] = cstart[(size_t)f * (ncells + 1) + c];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nL) return;
    const odo_landmark L = lms[i];
    const float* T = Tcw + (size_t)f * 16;
    const bool was_seen = (seen[(size_t)f * seen_words + (i >> 5)] >> (i & 31)) & 1;
    const float nan = __builtin_nanf("");
    float u = nan, v = nan, ur = nan;
    bool in = false;
    // Frame::isInFrustum: a NaN pixel passes these bounds
    if (!(L.flags & (ODO_LM_BAD | ODO_LM_SEEN)) && !was_seen) {
        const LmkCam Pc = lmk_camera(T, L.X);
        if (!(Pc.z < 0.0f)) {
            const LmkPix p = lmk_pixel_frustum(Pc, C);
            if (!(p.u < C.minX || p.u > C.maxX) && !(p.v < C.minY || p.v > C.maxY)) {
                in = true;
                u = p.u;
                v = p.v;
                ur = p.ur;
            }
        }
    }
    const size_t fi = (size_t)f * nL + i;
    proj[3 * fi] = u;
    proj[3 * fi + 1] = v;
    proj[3 * fi + 2] = ur;
    int c = in ? 0 : -1;
    // a NaN projection (Pc.z == 0) passes the bounds and has an empty window
    if (in && u == u && v == v) {
        uint32_t ld[8];
#pragma unroll
        for (int k = 0; k < 8; k++) ld[k] = reinterpret_cast<const uint32_t*>(L.desc)[k];
        const uint8_t* D = desc + (size_t)f * kp_cap * 32;
        // candidate k of landmark i at [f][k][i]: a wave's k-th candidates share cache lines
        uint32_t* out = cand + (size_t)f * LMK_CAP * nL + i;
        lmk_for_window(lmk_range(u, v, th, G), s_cs, G, 0, n, 0, 1, [&](int k) {
            const float2 q = s_xy[k];
            if (!lmk_in_window(q.x, q.y, u, v, th)) return;
            if (c < LMK_CAP) {
                const uint32_t jo = s_jo[k];
                const int j = (int)(jo & 0xffff);
                out[(size_t)c * nL] = lmk_key(j, (int)(jo >> 16), lmk_hamming(ld, D + 32 * (size_t)j));
            }
            c++;
        });
    }
    // the count, with the landmark's HAS_OBS bit so the resolver reads one word per landmark
    ccount[fi] = c < 0 ? -1 : (c | ((L.flags & ODO_LM_HAS_OBS) ? LMK_OBS : 0));
}

ODO_INLINE uint32_t lmk_wave_min(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

__global__ void __launch_bounds__(LMK_NT) k_lm_resolve(const odo_landmark* __restrict__ lms, int nL,
                                                       const int* __restrict__ nkp, int kp_cap,
                                                       const uint8_t* __restrict__ desc,
                                                       const float2* __restrict__ bxy, const uint32_t* __restrict__ bjo,
                                                       const int* __restrict__ cstart, LmGrid G, float th, float nnratio,
                                                       const float* __restrict__ proj, const int* __restrict__ ccount,
                                                       const uint32_t* __restrict__ cand,
                                                       const int32_t* __restrict__ prior_eff,
                                                       const uint8_t* __restrict__ taken0, int32_t* __restrict__ choice,
                                                       int32_t* __restrict__ over, int32_t* __restrict__ slot_lm,
                                                       int32_t* __restrict__ f2_src, float* __restrict__ Xg,
                                                       odo_local_map_result* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) int s_res[];
    __shared__ int s_changed, s_nov, s_nin, s_nm, s_ne;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncells = G.gx * G.gy;
    const int n = min(nkp[f], kp_cap);
    int* own0 = s_res;             // kp_cap
    int* own1 = own0 + kp_cap;     // kp_cap
    int* s_cs = own1 + kp_cap;     // ncells + 1
    const int* cntf = ccount + (size_t)f * nL;
    const uint32_t* candf = cand + (size_t)f * nL * LMK_CAP;
    int32_t* chf = choice + (size_t)f * nL;
    int32_t* ovf = over + (size_t)f * nL;
    const uint8_t* tk = taken0 + (size_t)f * kp_cap;
    const uint8_t* D = desc + (size_t)f * kp_cap * 32;
    const float2* XY = bxy + (size_t)f * kp_cap;
    const uint32_t* JO = bjo + (size_t)f * kp_cap;
    if (tid == 0) s_nov = s_nin = s_nm = s_ne = 0;
    for (int c = tid; c <= ncells; c += LMK_NT) s_cs[c] = cstart[(size_t)f * (ncells + 1) + c];
    for (int j = tid; j < n; j += LMK_NT) own0[j] = tk[j] ? -1 : 0x7fffffff;
    __syncthreads();
    {
        int nin = 0;
        for (int i = tid; i < nL; i += LMK_NT) {
            const int c = cntf[i];  // -1: not in view
            chf[i] = -1;
            nin += c >= 0;
            if (c >= 0 && (c & ~LMK_OBS) > LMK_CAP) ovf[atomicAdd(&s_nov, 1)] = i;
        }
        if (nin) atomicAdd(&s_nin, nin);
    }
    __syncthreads();
    const int nov = s_nov;
    int cur = 0, rounds = 0;
    for (;;) {
        rounds++;
        const int* own = own0 + cur * kp_cap;  // the round before
        int* nxt = own0 + (cur ^ 1) * kp_cap;  // this round's owners
        for (int j = tid; j < n; j += LMK_NT) nxt[j] = tk[j] ? -1 : 0x7fffffff;
        if (tid == 0) s_changed = 0;
        __syncthreads();
        // lists of up to LMK_CAP candidates: a thread per landmark
        // (the next landmark's count and choice are loaded a trip ahead: the
        // loop is a chain of dependent L2 round trips, one workgroup per CU)
        int raw_n = tid < nL ? cntf[tid] : -1, old_n = tid < nL ? chf[tid] : -1;
        for (int i = tid; i < nL; i += LMK_NT) {
            const int raw = raw_n, old = old_n, c = raw & ~LMK_OBS;
            if (i + LMK_NT < nL) {
                raw_n = cntf[i + LMK_NT];
                old_n = chf[i + LMK_NT];
            }
            if (raw < 0 || c == 0 || c > LMK_CAP) continue;  // not in view, empty window, wave path
            uint32_t a1 = LMK_NONE, a2 = LMK_NONE;
            for (int k = 0; k < c; k++) {
                const uint32_t key = candf[(size_t)k * nL + i];
                if (own[(key >> 5) & 0x1fff] >= i) lmk_insert(key, a1, a2);  // taken: owner below i
            }
            const int j = lmk_decide(a1, a2, nnratio);
            if (j != old) {
                chf[i] = j;
                s_changed = 1;
            }
            if (j >= 0 && (raw & LMK_OBS)) atomicMin(&nxt[j], i);
        }
        // longer lists: a wave per landmark over the window's cell runs
        for (int q = wave; q < nov; q += LMK_NW) {
            const int i = ovf[q];
            const size_t fi = (size_t)f * nL + i;
            const float u = proj[3 * fi], v = proj[3 * fi + 1];
            uint32_t ld[8];
#pragma unroll
            for (int k = 0; k < 8; k++) ld[k] = reinterpret_cast<const uint32_t*>(lms[i].desc)[k];
            uint32_t a1 = LMK_NONE, a2 = LMK_NONE;
            lmk_for_window(lmk_range(u, v, th, G), s_cs, G, 0, n, lane, 64, [&](int k) {
                const float2 p = XY[k];
                if (!lmk_in_window(p.x, p.y, u, v, th)) return;
                const uint32_t jo = JO[k];
                const int j = (int)(jo & 0xffff);
                if (own[j] >= i) lmk_insert(lmk_key(j, (int)(jo >> 16), lmk_hamming(ld, D + 32 * (size_t)j)), a1, a2);
            });
            const uint32_t m1 = lmk_wave_min(a1);
            const uint32_t m2 = lmk_wave_min(a1 == m1 ? a2 : a1);  // keys are distinct: one lane holds m1
            if (lane == 0) {
                const int j = lmk_decide(m1, m2, nnratio);
                if (j != chf[i]) {
                    chf[i] = j;
                    s_changed = 1;
                }
                if (j >= 0 && (cntf[i] & LMK_OBS)) atomicMin(&nxt[j], i);
            }
        }
        __syncthreads();
        const int changed = s_changed;
        __syncthreads();
        if (!changed) break;
        cur ^= 1;
    }
    // Frame::AddLandmark in landmark order: the largest index that chose j stays
    int* sl = own0 + (cur ^ 1) * kp_cap;
    for (int j = tid; j < n; j += LMK_NT) sl[j] = -1;
    __threadfence_block();
    __syncthreads();
    {
        int nm = 0;
        for (int i = tid; i < nL; i += LMK_NT) {
            const int j = chf[i];
            if (j >= 0) {
                atomicMax(&sl[j], i);
                nm++;
            }
        }
        if (nm) atomicAdd(&s_nm, nm);
    }
    __syncthreads();
    // merged slots and the PnP edges (pnpsolver.cpp:57-135 reads them in slot order)
    {
        int ne = 0;
        for (int j = tid; j < kp_cap; j += LMK_NT) {
            const size_t fj = (size_t)f * kp_cap + j;
            int m = -1;
            if (j < n) m = sl[j] >= 0 ? sl[j] : prior_eff[fj];
            slot_lm[fj] = m;
            f2_src[fj] = m >= 0 ? j : -1;
            if (m >= 0) {
                Xg[3 * fj] = lms[m].X[0];
                Xg[3 * fj + 1] = lms[m].X[1];
                Xg[3 * fj + 2] = lms[m].X[2];
                ne++;
            }
        }
        if (ne) atomicAdd(&s_ne, ne);
    }
    __syncthreads();
    if (tid == 0) {
        res[f].n_in_view = s_nin;
        res[f].n_matches = s_nm;
        res[f].n_edges = s_ne;
        res[f].pad[0] = rounds;  // diagnostic: relaxation rounds, the confirming one included
    }
}

__global__ void __launch_bounds__(256) k_lm_stats(const odo_landmark* __restrict__ lms, const int* __restrict__ nkp,
                                                  int kp_cap, const int32_t* __restrict__ slot_lm,
                                                  const uint8_t* __restrict__ pnp_mask,
                                                  const odo_pair_result* __restrict__ pres,
                                                  uint8_t* __restrict__ outlier, odo_local_map_result* __restrict__ res) {
    __shared__ int s_n;
    const int f = blockIdx.x;
    const int n = min(nkp[f + 1], kp_cap);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int cnt = 0;
    for (int j = threadIdx.x; j < kp_cap; j += blockDim.x) {
        const size_t fj = (size_t)f * kp_cap + j;
        const int m = j < n ? slot_lm[fj] : -1;
        const bool inl = m >= 0 && pnp_mask[fj];
        outlier[fj] = (m >= 0 && !inl) ? 1 : 0;
        cnt += inl && (lms[m].flags & ODO_LM_HAS_OBS);  // tracking.cpp:247-255
    }
    if (cnt) atomicAdd(&s_n, cnt);
    __syncthreads();
    if (threadIdx.x < 16) res[f].Tcw[threadIdx.x] = pres[f].Tcw[threadIdx.x];
    if (threadIdx.x == 0) {
        res[f].pnp_inliers = pres[f].pnp_inliers;
        res[f].n_map_inliers = s_n;
        res[f].pad[1] = res[f].pad[2] = 0;
    }
}

int local_map_cand_cap() { return LMK_CAP; }

LmGrid local_map_grid(const float bounds[4]) {
    LmGrid G;
    G.x0 = bounds[0];
    G.y0 = bounds[2];
    float cell = 32.0f;
    for (;;) {
        const float w = fmaxf(bounds[1] - bounds[0], 0.0f), h = fmaxf(bounds[3] - bounds[2], 0.0f);
        const float gx = floorf(w / cell) + 1.0f, gy = floorf(h / cell) + 1.0f;
        if (gx * gy <= 2048.0f) {
            G.gx = (int)gx;
            G.gy = (int)gy;
            break;
        }
        cell *= 2.0f;
    }
    G.inv = 1.0f / cell;
    return G;
}

int launch_local_map_search(hipStream_t st, const LmSearch& a) {
    if (a.kp_cap > 8191) return -1;  // 13-bit keypoint index in a key
    const int ncells = a.G.gx * a.G.gy;
    const size_t lds_bin = (size_t)(ncells + 1) * 4;
    const size_t lds_c = (size_t)a.kp_cap * 12 + (size_t)(ncells + 1) * 4;
    const size_t lds_r = (size_t)a.kp_cap * 8 + (size_t)(ncells + 1) * 4;
    if (lds_c > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)k_lm_cands, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c);
    if (lds_r > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)k_lm_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r);
    hipLaunchKernelGGL(k_lm_prior, dim3((a.kp_cap + 255) / 256, a.nframes), dim3(256), 0, st, a.prior, a.lms, a.nL,
                       a.taken_in, a.nkp, a.kp_cap, a.seen, a.seen_words, a.prior_eff, a.taken0);
    hipLaunchKernelGGL(k_lm_bin, dim3(a.nframes), dim3(256), lds_bin, st, a.kun, a.oct, a.oct_stride, a.nkp, a.kp_cap,
                       a.G, a.bxy, a.bjo, a.cstart);
    if (a.nL > 0)
        hipLaunchKernelGGL(k_lm_cands, dim3((a.nL + 255) / 256, a.nframes), dim3(256), lds_c, st, a.Tcw, a.lms, a.nL,
                           a.seen, a.seen_words, a.nkp, a.kp_cap, a.desc, a.bxy, a.bjo, a.cstart, a.G, a.C, a.th,
                           a.proj, a.ccount, a.cand);
    hipLaunchKernelGGL(k_lm_resolve, dim3(a.nframes), dim3(LMK_NT), lds_r, st, a.lms, a.nL, a.nkp, a.kp_cap, a.desc,
                       a.bxy, a.bjo, a.cstart, a.G, a.th, a.nnratio, a.proj, a.ccount, a.cand, a.prior_eff, a.taken0,
                       a.choice, a.over, a.slot_lm, a.f2_src, a.Xg, a.res);
    return 0;
}

void launch_local_map_stats(hipStream_t st, const odo_landmark* lms, const int* nkp, int kp_cap, const int32_t* slot_lm,
                            const uint8_t* pnp_mask, const odo_pair_result* pres, uint8_t* outlier,
                            odo_local_map_result* res, int nframes) {
    hipLaunchKernelGGL(k_lm_stats, dim3(nframes), dim3(256), 0, st, lms, nkp, kp_cap, slot_lm, pnp_mask, pres, outlier,
                       res);
}

}  // namespace odo
