// Odometry::Compute's ADAPTIVE_RICP and RANSAC back-ends (odometry.cpp:46-92)
// for a batch of pairs, on the batch's pair stream after launch_ransac and in
// place of launch_pnp:
//   k_ricp_plan    per pair: the branch of odometry.cpp:52-53 from RANSAC's
//                  record, the GICP guess, the cloud length; the exclusive
//                  scan of the lengths
//   k_ricp_gather  Ransac::mpSourceCloud / mpTargetCloud (ransac.cpp:161-189)
//   launch_gicp    GeneralizedICP::Compute on the device-side offsets / guesses
//   k_ricp_apply   the odo_ricp_result record, Tcw (odometry.cpp:55-72) and
//                  the inlier flags (odometry.cpp:75-76, 90-91)
// RANSAC mode is k_ricp_apply alone with every pair on branch 0.
// Nothing here reads a count on the host: the grids are sized by the batch and
// match_cap, the kernels read n_matches / n_good / res / T12 on the device.
#include "odo_internal.h"
#include "odo_wave.h"

namespace odo {

namespace {

constexpr int RI_THREADS = 256;
constexpr int RI_WAVES = RI_THREADS / 64;

// matches of the batched contract's pair p that Ransac::Iterate walks: the pair
// has a predecessor and KnnMatch found enough of them (k_ransac_prep's `active`
// before the good-match count)
__device__ __forceinline__ bool pair_runs(const int* pair_valid, const int* n_matches, int p, int min_matches,
                                          int min_inlier_th) {
    const int nm = n_matches[p];
    return pair_valid[p] && nm >= min_matches && nm >= min_inlier_th;
}

// One workgroup for the whole batch. branch[p]: 0 keep RANSAC's mT12, 1 GICP
// from identity, 2 GICP from mT12. The decision is odometry.cpp:52-53 in float,
// operation by operation (the library is built with -ffp-contract=off).
// offs[0..n]: exclusive scan of the cloud lengths (source and target clouds
// have the same length: one offset array serves both).
__global__ void __launch_bounds__(RI_THREADS) k_ricp_plan(const odo_pair_result* __restrict__ res,
                                                          const float* __restrict__ T12,
                                                          const int* __restrict__ pair_valid,
                                                          const int* __restrict__ n_matches,
                                                          const int* __restrict__ n_good, int min_matches,
                                                          int min_inlier_th, int match_cap, RicpCfg cfg,
                                                          int* __restrict__ branch, float* __restrict__ guess,
                                                          int* __restrict__ offs, int n) {
    __shared__ int s_scan[RI_THREADS];
    const int t = threadIdx.x;
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += RI_THREADS) {
        const int p = p0 + t;
        int len = 0;
        if (p < n) {
            int br = 0;
            if (pair_valid[p]) {
                const float rmse = res[p].rmse;
                if (res[p].n_inliers < cfg.min_inliers || rmse * cfg.rmse_scale >= cfg.refine_at)
                    br = rmse * cfg.rmse_scale >= cfg.reset_at ? 1 : 2;
            }
            branch[p] = br;
            const float* T = T12 + (size_t)p * 16;
            float* g = guess + (size_t)p * 16;
            for (int i = 0; i < 16; i++) g[i] = br == 2 ? T[i] : (i % 5 == 0 ? 1.f : 0.f);
            if (br != 0 && pair_runs(pair_valid, n_matches, p, min_matches, min_inlier_th))
                len = min(max(n_good[p], 0), match_cap);
        }
        s_scan[t] = len;
        __syncthreads();
        for (int off = 1; off < RI_THREADS; off <<= 1) {
            const int a = t >= off ? s_scan[t - off] : 0;
            __syncthreads();
            s_scan[t] += a;
            __syncthreads();
        }
        if (p < n) offs[p] = base + s_scan[t] - len;
        base += s_scan[RI_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) offs[n] = base;
}

// One workgroup per pair: the depth-valid matches in m12 order
// (ransac.cpp:175-189), source = F1 xyz[queryIdx], target = F2 xyz[trainIdx],
// compacted in order: ballot within the wave, wave counts in order, a running
// tail across the chunks. The range [offs[p], offs[p+1]) is empty for a pair
// the plan did not select.
__global__ void __launch_bounds__(RI_THREADS) k_ricp_gather(const odo_dmatch* __restrict__ matches,
                                                            const int* __restrict__ n_matches,
                                                            const float* __restrict__ xyz, int kp_cap, int slot0,
                                                            int match_cap, int check_depth,
                                                            const int* __restrict__ offs, float* __restrict__ src,
                                                            float* __restrict__ tgt) {
    __shared__ int s_w[RI_WAVES];
    const int p = blockIdx.x;
    const int o0 = offs[p], len = offs[p + 1] - o0;
    if (len <= 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nm = min(n_matches[p], match_cap);
    const odo_dmatch* M = matches + (size_t)p * match_cap;
    const float* X1 = xyz + (size_t)(slot0 + p) * kp_cap * 3;
    const float* X2 = xyz + (size_t)(slot0 + p + 1) * kp_cap * 3;
    float* S = src + 3 * (size_t)o0;
    float* T = tgt + 3 * (size_t)o0;
    int tail = 0;
    for (int c0 = 0; c0 < nm; c0 += RI_THREADS) {
        const int i = c0 + t;
        bool keep = false;
        float s[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
        if (i < nm) {
            const odo_dmatch m = M[i];
            // indices come from k_pair_match (inside both frames); checked all the same
            if ((unsigned)m.queryIdx < (unsigned)kp_cap && (unsigned)m.trainIdx < (unsigned)kp_cap) {
                for (int k = 0; k < 3; k++) {
                    s[k] = X1[3 * m.queryIdx + k];
                    q[k] = X2[3 * m.trainIdx + k];
                }
                keep = true;
                if (check_depth) {
                    if (__builtin_isnan(s[2]) || __builtin_isnan(q[2])) keep = false;
                    if (s[2] <= 0 || q[2] <= 0) keep = false;
                }
            }
        }
        const uint64_t bal = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
        for (int w = 0; w < RI_WAVES; w++) {
            if (w < wave) before += s_w[w];
            tot += s_w[w];
        }
        __syncthreads();
        if (keep) {
            const int k = tail + before + lane_rank(bal);
            if (k < len) {  // len is k_pair_match's count of the same filter
                for (int j = 0; j < 3; j++) {
                    S[3 * k + j] = s[j];
                    T[3 * k + j] = q[j];
                }
            }
        }
        tail += tot;
    }
}

// One workgroup per pair. ricp / branch / gT / gio are null in RANSAC mode
// (every pair on branch 0). Tcw (the chosen T12 times F1's pose, the identity
// in the batched contract):
//   branch 0: RANSAC's T12 bits
//   branch 1: GICP's T12 if converged, else identity      (odometry.cpp:55-58)
//   branch 2: GICP's T12 if converged, else RANSAC's bits (odometry.cpp:61-64)
// inlier_mask: F2's flags, SetInlier(m.trainIdx) for every m of mvInliers (the
// set bits of RANSAC's mask over the sorted good matches); res.pnp_inliers the
// number of flags set. A pair without a predecessor gets what k_pnp gives it:
// Tcw = T12, no flags.
__global__ void __launch_bounds__(RI_THREADS) k_ricp_apply(const int* __restrict__ pair_valid,
                                                           const int* __restrict__ n_matches,
                                                           const int* __restrict__ n_good,
                                                           const odo_dmatch* __restrict__ matches,
                                                           const uint64_t* __restrict__ good,
                                                           const uint32_t* __restrict__ best_mask, int mask_words,
                                                           int match_cap, const int* __restrict__ nkp, int kp_cap,
                                                           int slot0, const float* __restrict__ T12,
                                                           const int* __restrict__ branch,
                                                           const int* __restrict__ offs, const float* __restrict__ gT,
                                                           const int* __restrict__ gio,
                                                           odo_pair_result* __restrict__ res,
                                                           odo_ricp_result* __restrict__ ricp,
                                                           uint8_t* __restrict__ inlier_mask) {
    __shared__ int s_cnt;
    const int p = blockIdx.x, t = threadIdx.x;
    odo_pair_result* R = res + p;
    const float* T0 = T12 + (size_t)p * 16;
    const int br = branch ? branch[p] : 0;
    const bool conv = br != 0 && gio[4 * p] != 0;
    if (t < 16) {
        const float id = t % 5 == 0 ? 1.f : 0.f;
        const float g = br != 0 ? gT[(size_t)p * 16 + t] : id;
        R->Tcw[t] = conv ? g : (br == 1 ? id : T0[t]);
        if (ricp) ricp[p].T12[t] = g;
    }
    if (ricp && t == 0) {
        odo_ricp_result* Q = ricp + p;
        Q->branch = br;
        Q->converged = br != 0 ? gio[4 * p] : 0;
        Q->iterations = br != 0 ? gio[4 * p + 1] : 0;
        Q->n_corr = br != 0 ? gio[4 * p + 2] : 0;
        Q->n_cloud = offs[p + 1] - offs[p];
        Q->pad[0] = Q->pad[1] = Q->pad[2] = 0;
    }
    // ---- inlier flags
    const int n2 = min(nkp[slot0 + p + 1], kp_cap);
    uint8_t* mask = inlier_mask + (size_t)p * kp_cap;
    for (int i = t; i < n2; i += RI_THREADS) mask[i] = 0;
    if (t == 0) s_cnt = 0;
    __syncthreads();
    const int nm = min(n_matches[p], match_cap);
    // best_mask is RANSAC's only where it accepted a hypothesis (n_inliers > 0)
    if (pair_valid[p] && R->n_inliers > 0) {
        const int ng = min(min(n_good[p], match_cap), mask_words * 32);
        const odo_dmatch* M = matches + (size_t)p * match_cap;
        const uint64_t* G = good + (size_t)p * match_cap;
        const uint32_t* BM = best_mask + (size_t)p * mask_words;
        for (int k = t; k < ng; k += RI_THREADS) {
            if (!((BM[k >> 5] >> (k & 31)) & 1)) continue;
            const uint32_t gi = (uint32_t)(G[k] >> 32);  // SortEl.val: position in the match list
            if (gi >= (uint32_t)nm) continue;
            const int ti = M[gi].trainIdx;
            if ((unsigned)ti < (unsigned)n2) mask[ti] = 1;  // same value from every writer
        }
    }
    __threadfence_block();
    __syncthreads();
    int c = 0;
    for (int i = t; i < n2; i += RI_THREADS) c += mask[i];
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if ((t & 63) == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (t == 0) R->pnp_inliers = s_cnt;
}

}  // namespace

void launch_ricp_plan(hipStream_t st, const odo_pair_result* res, const float* T12, const int* pair_valid,
                      const int* n_matches, const int* n_good, int min_matches, int min_inlier_th, int match_cap,
                      RicpCfg cfg, int* branch, float* guess, int* offs, int npairs) {
    hipLaunchKernelGGL(k_ricp_plan, dim3(1), dim3(RI_THREADS), 0, st, res, T12, pair_valid, n_matches, n_good,
                       min_matches, min_inlier_th, match_cap, cfg, branch, guess, offs, npairs);
}

void launch_ricp_gather(hipStream_t st, const odo_dmatch* matches, const int* n_matches, const float* xyz, int kp_cap,
                        int slot0, int match_cap, int check_depth, const int* offs, float* src, float* tgt,
                        int npairs) {
    hipLaunchKernelGGL(k_ricp_gather, dim3(npairs), dim3(RI_THREADS), 0, st, matches, n_matches, xyz, kp_cap, slot0,
                       match_cap, check_depth, offs, src, tgt);
}

void launch_ricp_apply(hipStream_t st, const int* pair_valid, const int* n_matches, const int* n_good,
                       const odo_dmatch* matches, const void* good, const uint32_t* best_mask, int mask_words,
                       int match_cap, const int* nkp, int kp_cap, int slot0, const float* T12, const int* branch,
                       const int* offs, const float* gT, const int* gio, odo_pair_result* res, odo_ricp_result* ricp,
                       uint8_t* inlier_mask, int npairs) {
    hipLaunchKernelGGL(k_ricp_apply, dim3(npairs), dim3(RI_THREADS), 0, st, pair_valid, n_matches, n_good, matches,
                       (const uint64_t*)good, best_mask, mask_words, match_cap, nkp, kp_cap, slot0, T12, branch, offs,
                       gT, gio, res, ricp, inlier_mask);
}

}  // namespace odo
