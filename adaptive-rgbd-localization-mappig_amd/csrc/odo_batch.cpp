// The pipelined batch path: extraction, the roll, kNN-2, the pair stages and
// the odo_track_batch* / host-input entry points.
//
// Batches are pipelined over an extraction stream, two pair streams and NSETS
// frame sets (each with its pair buffers and RANSAC scratch). Batch b uses set
// b % NSETS and pair stream b % 2:
//   extraction stream: pyramid, FAST, octree, blur, descriptors of the new
//     frames into slots 1..n of the set;
//   pair stream: RANSAC's rand() words (seed-only, ahead of the extraction's
//     end), then the roll (the previous batch's last frame into slot 0), the
//     keypoint geometry, kNN-2, matching, the DepthCovariance latch, RANSAC
//     and PnP (in the RANSAC / ADAPTIVE_RICP modes of odo_set_odometry the
//     chain of run_ricp in the PnP's place).
// So batch b+1's throughput-bound extraction overlaps batch b's latency-bound
// pair stages, and one batch's long RANSAC / PnP overlaps the next batch's
// pair stages on the other pair stream. One event per set ("PnP of this set
// done") orders the reuse: a set is rewritten only after the PnP of the batch
// that last used it, and the extraction of batch b waits for the PnP of batch
// b - PYR_WAIT. (The ADAPTIVE detectors, stage timing and host-input batches
// keep the roll and the geometry on the extraction stream.)
#include "odo_ctx.h"

// `st` waits until the PnP launch (and, async, the result copy) of the batch
// that last used frame set `set` is done. Every wait is a barrier packet the
// queue processes in order, so each is worth leaving out: one event per set is
// recorded after the batch's last pair-stream work, and the stream that
// recorded it needs no wait at all (it is ordered behind that work already).
static int wait_pnp_done(odo_ctx* c, hipStream_t st, int set) {
    if (st != c->pdone_st[set]) HIPCHK(hipStreamWaitEvent(st, c->ev_pnp_done[set], 0));
    return ODO_OK;
}

// The extraction stream's waits before the next batch: its frame set is free
// once the PnP of the batch that last used it is done, and the PnP of the
// batch PYR_WAIT before it is done.
static int queue_batch_waits(odo_ctx* c) {
    int e;
    const int s = next_set(c);
    if (c->pdone_rec[s] && (e = wait_pnp_done(c, c->stream, s))) return e;
    // batch b always uses set b % NSETS (seq_set and batch_counter only ever advance together)
    if (c->batch_counter >= (uint64_t)PYR_WAIT && (e = wait_pnp_done(c, c->stream, (s + NSETS - PYR_WAIT) % NSETS)))
        return e;
    return ODO_OK;
}

// gray (when d_bgr is given) and the pyramid levels of n frames
// (and, with blur given and c->blur_fused, the blurred levels in the same launch)
// Returns true when the blurred levels were written too.
constexpr int PYR_FUSED_MIN_FRAMES = 128;
static bool build_pyramid(odo_ctx* c, hipStream_t st, const uint8_t* d_bgr, uint8_t* pyr, int n, uint8_t* blur) {
    const size_t P = c->pyr_size;
    const bool fused = c->pyr_fusable && (c->pform == ODO_PYRAMID_FORM_FUSED || c->pform == ODO_PYRAMID_FORM_FUSED_NOBLUR ||
                                          (c->pform == ODO_PYRAMID_FORM_AUTO && n >= PYR_FUSED_MIN_FRAMES));
    if (fused) {
        if (c->pform == ODO_PYRAMID_FORM_FUSED_NOBLUR || !c->blur_fusable) blur = nullptr;
        launch_pyramid(st, d_bgr, pyr, (size_t)c->W * c->H * 3, P, c->lv, c->rx, c->ry, c->rx_off.data(),
                       c->ry_off.data(), c->nlevels, n, blur, c->lv_h.data(),
                       c->ry_h.data());
        return blur != nullptr;
    }
    if (d_bgr) launch_gray(st, d_bgr, pyr, c->W, c->H, c->lv_h[0].pitch, (size_t)c->W * c->H * 3, P, n);
    for (int l = 1; l < c->nlevels; l++) {
        const LevelDesc& S = c->lv_h[l - 1];
        const LevelDesc& D = c->lv_h[l];
        launch_resize(st, pyr, P, S.off, S.pitch, D.off, D.pitch, D.w, D.h, RZ_RB, c->rz_rows[l],
                      c->rx + c->rx_off[l], c->ry + c->ry_off[l], n);
    }
    return false;
}

// Extractor(FAST, ORB, ADAPTIVE) for frames slot0.. of `set` (k_adaptive.hip):
// threshold-free S map -> band survivors + S histograms -> the per-cell
// threshold chain over the batch in frame order -> keepStrongest ->
// retainBest + border filter -> rBRIEF / undistort / depth.
static int run_extract_adaptive(odo_ctx* c, int set, const uint8_t* d_bgr, const uint16_t* d_depth, int n,
                                int slot0) {
    hipStream_t st = c->stream;
    const size_t P = c->pyr_size;
    const size_t slot = fbase(c, set) + slot0;
    const LevelDesc& L0 = c->lv_h[0];
    uint8_t* pyr = c->pyr + slot * P;
    const size_t nc = (size_t)c->ad_ncells;
    if (d_bgr) launch_gray(st, d_bgr, pyr, c->W, c->H, L0.pitch, (size_t)c->W * c->H * 3, P, n);
    tmark(c, 1, st);
    launch_adapt_smap(st, pyr, P, c->W, c->H, L0.pitch, c->smap, c->smap_stride, n);
    HIPCHK(hipMemsetAsync(c->ahist, 0, (size_t)n * nc * 256 * sizeof(int), st));
    if (c->ad_nbands > 0)
        launch_adapt_cand(st, c->smap, c->smap_stride, L0.pitch, c->adb, c->ad_nbands, c->adc, c->ad_ncells, c->acand,
                          c->acand_stride, c->aband_cnt, c->ahist, n);
    tmark(c, 2, st);
    launch_adapt_chain(st, c->ahist, c->ad_ncells, n, c->cfg.adaptive, c->athresh, c->atsel, c->ansel);
    launch_adapt_select(st, c->acand, c->acand_stride, c->aband_cnt, c->ad_nbands, c->adb, c->adc, c->ad_ncells,
                        c->atsel, c->ansel, c->ad_mpc, c->abig, c->abig_stride, c->acell, c->acell_cnt, n);
    launch_adapt_assemble(st, c->acell, c->acell_cnt, c->ad_ncells, c->ad_mpc, c->cfg.adaptive.retain_best, c->W,
                          c->H, c->akp, c->kp_cap, c->nkp + slot, c->kp_cap, n);
    tmark(c, 3, st);
    launch_blur(st, pyr, c->blur + slot * P, P, c->lv, c->lv_h.data(), 1, n);
    tmark(c, 4, st);
    const FrameSlot f = frame_at(c, slot);
    launch_adapt_finalize(st, c->blur + slot * P, P, L0.pitch, c->akp, c->kp_cap, f.nkp, c->a_cos, c->a_sin, d_depth,
                          (size_t)c->W * c->H, c->W, c->cal, f.kps, f.desc, f.kun, f.xyz, f.ur, c->kp_cap, n);
    tmark(c, 5, st);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

// Extractor(ORB, ORB, ADAPTIVE) for frames slot0.. of `set`
// (k_adaptive_orb.hip): the frame pyramid + blur (cv::ORB::compute's levels)
// -> cell pyramids -> S maps -> band survivors + S histograms -> count tables
// -> the per-cell threshold chain -> per-cell select -> assemble ->
// IC angle / rBRIEF / undistort / depth.
static int run_extract_adaptive_orb(odo_ctx* c, int set, const uint8_t* d_bgr, const uint16_t* d_depth, int n,
                                    int slot0) {
    hipStream_t st = c->stream;
    const size_t P = c->pyr_size;
    const size_t slot = fbase(c, set) + slot0;
    uint8_t* pyr = c->pyr + slot * P;
    const int nc = c->ad_ncells, ni = (int)c->oai_h.size(), nb = (int)c->oab_h.size();
    build_pyramid(c, st, d_bgr, pyr, n, nullptr);
    tmark(c, 1, st);
    launch_oa_pyr(st, pyr, P, c->lv_h[0].pitch, c->oac, nc, c->oai, c->oa_buf0, c->oa_buf1, c->cpyr, c->cp_stride, n);
    HIPCHK(hipMemsetAsync(c->ohist, 0, (size_t)n * ni * 256 * sizeof(int), st));
    if (nb > 0)
        launch_oa_scand(st, c->cpyr, c->cp_stride, c->oai, ni, c->oab, nb, c->ocand, c->ocand_stride, c->oband_cnt,
                        c->ohist, c->oa_maxpitch, n);
    launch_oa_count(st, c->ohist, c->oac, c->oai, ni, nc, c->ophist, n);
    tmark(c, 2, st);
    launch_adapt_chain(st, c->ophist, nc, n, c->cfg.adaptive, c->athresh, c->atsel, c->ansel);
    launch_oa_select(st, c->ocand, c->ocand_stride, c->oband_cnt, nb, c->oab, c->oai, c->oac, nc, c->atsel, c->cpyr,
                     c->cp_stride, c->ad_mpc, c->oscr, c->oscr_stride, c->oa_ncap, c->ocell, c->acell_cnt, n);
    launch_oa_assemble(st, c->ocell, c->acell_cnt, c->oac, nc, c->ad_mpc, c->cfg.adaptive.retain_best, c->W, c->H,
                       c->osc, c->oakp, c->kp_cap, c->nkp + slot, c->kp_cap, n);
    tmark(c, 3, st);
    launch_blur(st, pyr, c->blur + slot * P, P, c->lv, c->lv_h.data(), OA_NLEV, n);
    tmark(c, 4, st);
    const FrameSlot f = frame_at(c, slot);
    launch_oa_finalize(st, pyr, c->blur + slot * P, P, c->lv, c->cpyr, c->cp_stride, c->oai, c->oac, c->osc, c->oakp,
                       c->kp_cap, f.nkp, d_depth, (size_t)c->W * c->H, c->W, c->cal, f.kps, f.desc, f.kun, f.xyz, f.ur,
                       c->kp_cap, n);
    tmark(c, 5, st);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

// `geometry`: the keypoint geometry (undistort, depth) in the finalize launch;
// a batch that runs it on its pair stream (track_batch) leaves it out there.
// The ADAPTIVE extractors always include it.
int odo::run_extract(odo_ctx* c, int set, const uint8_t* d_bgr, const uint16_t* d_depth, int n, int slot0, bool geometry) {
    if (c->adaptive_orb) return run_extract_adaptive_orb(c, set, d_bgr, d_depth, n, slot0);
    if (c->adaptive) return run_extract_adaptive(c, set, d_bgr, d_depth, n, slot0);
    hipStream_t st = c->stream;
    const size_t P = c->pyr_size;
    const size_t slot = fbase(c, set) + slot0;
    uint8_t* pyr = c->pyr + (size_t)slot * P;
    const bool blur_done = build_pyramid(c, st, d_bgr, pyr, n, c->blur + (size_t)slot * P);
    tmark(c, 1, st);
    launch_fast(st, pyr, P, c->fsegs, (int)c->fsegs_h.size(), c->lv, c->cand + (size_t)slot * c->ncells * c->cell_cap,
                c->cand_cnt + (size_t)slot * c->ncells, c->ncells, c->cell_cap, c->cfg.orb.ini_th_fast,
                c->cfg.orb.min_th_fast, c->fs_lds, n);
    tmark(c, 2, st);
    launch_octree(st, c->cand + (size_t)slot * c->ncells * c->cell_cap, c->cand_cnt + (size_t)slot * c->ncells, c->lv,
                  c->ncells, c->cell_cap, c->nlevels, c->keys + (size_t)slot * c->keys_per_frame,
                  c->knode + (size_t)slot * c->keys_per_frame, c->keys_per_frame, c->okp + (size_t)slot * c->nlevels * c->okp_stride,
                  c->ocnt + (size_t)slot * c->nlevels, c->okp_stride, c->node_cap, n);
    tmark(c, 3, st);
    if (!blur_done) launch_blur(st, pyr, c->blur + (size_t)slot * P, P, c->lv, c->lv_h.data(), c->nlevels, n);
    tmark(c, 4, st);
    const FrameSlot f = frame_at(c, slot);
    launch_finalize(st, pyr, c->blur + (size_t)slot * P, P, c->lv, c->nlevels,
                    c->okp + (size_t)slot * c->nlevels * c->okp_stride, c->ocnt + (size_t)slot * c->nlevels,
                    c->okp_stride, d_depth, (size_t)c->W * c->H, c->W, c->cal, f.kps, f.desc, f.kun, f.xyz, f.ur, f.nkp,
                    c->kp_cap, n, geometry);
    tmark(c, 5, st);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

// Odometry::Compute's RANSAC / ADAPTIVE_RICP tail (odometry.cpp:46-92) of one
// batch, on its pair stream after launch_ransac: plan (branch, guess, cloud
// offsets), gather (mpSourceCloud / mpTargetCloud), GICP, apply (record, Tcw,
// inlier flags); RANSAC mode is the apply step alone. Everything the chain
// reads (n_matches, n_good, res, T12) stays on the device: the host gives grid
// bounds only (the batch size and match_cap).
static void run_ricp(odo_ctx* c, hipStream_t st, int set, int n) {
    auto& P = c->pb[set];
    const FrameSlot f = frame_at(c, fbase(c, set));
    const int min_inl = c->cfg.ransac.min_inlier_th;
    if (c->odo_mode == ODO_ODOMETRY_RANSAC) {
        launch_ricp_apply(st, P.pair_valid, P.n_matches, P.n_good, P.matches, P.good, P.best_mask, c->mask_words,
                          c->match_cap, f.nkp, c->kp_cap, 0, P.T12, nullptr, nullptr, nullptr, nullptr, P.res, nullptr,
                          P.pnp_mask, n);
        return;
    }
    auto& R = c->rb[c->batch_counter & 1];  // the copy of this batch's pair stream
    const odo_ricp_params& rp = c->ricp;
    launch_ricp_plan(st, P.res, P.T12, P.pair_valid, P.n_matches, P.n_good, 20, min_inl, c->match_cap,
                     RicpCfg{rp.min_inliers, rp.rmse_scale, rp.refine_at, rp.reset_at}, R.branch, R.guess, R.offs, n);
    launch_ricp_gather(st, P.matches, P.n_matches, f.xyz, c->kp_cap, 0, c->match_cap, c->cfg.ransac.check_depth, R.offs,
                       R.src, R.tgt, n);
    GicpArgs args{R.guess, R.offs, R.offs, rp.gicp_max_corr_dist, rp.gicp_iterations, 20 /* PCL inner */};
    launch_gicp(st, R.src, R.tgt, n, c->match_cap, c->match_cap, R.Cs, R.Ct, R.outp, R.Mah, R.is, R.it, args, R.gT,
                R.gio);
    launch_ricp_apply(st, P.pair_valid, P.n_matches, P.n_good, P.matches, P.good, P.best_mask, c->mask_words,
                      c->match_cap, f.nkp, c->kp_cap, 0, P.T12, R.branch, R.offs, R.gT, R.gio, P.res, R.rec, P.pnp_mask,
                      n);
}

// The match stage of the n pairs of frame set `set` on stream `st`: the pair
// flags (pair 0 valid only with `first_valid`), k_pair_match and, unless
// `latched`, the DepthCovariance latch. Shared by run_pairs and
// odo_debug_match_features, so the two cannot drift apart.
int odo::run_pair_match(odo_ctx* c, hipStream_t st, int set, int n, bool first_valid, bool latched) {
    auto& P = c->pb[set];
    const size_t KC = (size_t)c->kp_cap;
    const FrameSlot f = frame_at(c, fbase(c, set));
    launch_pair_valid(st, P.pair_valid, n, first_valid ? 1 : 0);
    launch_pair_match(st, c->knn_idx[set], c->knn_dist[set], KC, f.xyz, f.nkp, c->kp_cap, 0, c->cfg.nn_ratio,
                      c->lm_bits[set], c->lm_words, c->knn_split, (size_t)c->maxb * KC, c->cfg.ransac.check_depth,
                      P.matches, P.n_matches, P.good, P.n_good, P.f2_src, c->sort_scratch, c->match_cap, n);
    // the DepthCovariance latch is taken from the first valid pair ever: with
    // two pair streams, a batch's latch kernel runs after the previous one's
    // (ev_latch). Once the latch holds a value (k_latch's host flag) and the
    // kernel that set it has completed, the latch kernel is a no-op: it and
    // its two ordering packets are left out
    if (!latched) {
        if (c->latch_rec) HIPCHK(hipStreamWaitEvent(st, c->ev_latch, 0));
        launch_latch(st, c->latch, P.good, P.n_good, P.n_matches, P.matches, f.xyz, c->kp_cap, 0, n, c->match_cap,
                     c->cfg.ransac.min_inlier_th, c->cfg.ransac.sample_size, c->cfg.ransac.iterations, P.pair_valid,
                     c->latch_set_h);
        HIPCHK(hipEventRecord(c->ev_latch, st));
        c->latch_rec = true;
    }
    return ODO_OK;
}

// Pair stages of one batch on its pair stream `st`, over frame set `set`:
// pair p is (slot p, slot p+1); pair 0 is valid only with a previous frame.
// `latched`: the DepthCovariance latch is known to hold its value (track_batch),
// so the latch kernel is left out. `defer_done`: the caller records the set's
// PnP-done event itself, after the result copy it queues behind the PnP.
static int run_pairs(odo_ctx* c, hipStream_t st, int set, int n, bool latched, bool defer_done) {
    auto& P = c->pb[set];
    const FrameSlot f = frame_at(c, fbase(c, set));
    int e;
    tmark(c, 6, st);
    if ((e = run_pair_match(c, st, set, n, c->has_prev, latched))) return e;
    tmark(c, 7, st);
    // RANSAC, then one PnP launch for the whole batch, back to back on the
    // batch's own pair stream: nothing else waits for RANSAC alone, so no
    // marker packet sits between the two launches
    if (!(c->skip & 16))
        launch_ransac(st, P.good, P.n_good, P.n_matches, P.matches, f.xyz, c->kp_cap, 0, c->match_cap, c->rcfg,
                      c->latch, P.pair_valid, 20, nullptr, c->rscr[set], P.best_mask, c->mask_words, P.res, P.T12, n,
                      c->h_open + set);
    tmark(c, 8, st);
    if (!(c->skip & 1)) {
        if (c->odo_mode == ODO_ODOMETRY_ADAPTIVE_RBA)
            launch_pnp(st, P.f2_src, f.xyz, f.kun, f.ur, f.nkp, c->kp_cap, 0, c->cal, P.T12, P.pair_valid, P.n_matches,
                       20, P.edges, P.res, P.pnp_mask, n);
        else
            run_ricp(c, st, set, n);  // Odometry(RANSAC) / Odometry(ADAPTIVE_RICP): in place of the PnP
    }
    tmark(c, 9, st);
    if (!defer_done) HIPCHK(hipEventRecord(c->ev_pnp_done[set], st));
    c->pdone_st[set] = st;
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

// n_matches / n_queries of the batch's result records (0 for a pair without a
// previous frame), on the device so the records can be copied out asynchronously
__global__ void k_res_patch(odo_pair_result* __restrict__ res, const int* __restrict__ n_matches,
                            const int* __restrict__ qcnt, int n, int first_valid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool v = i > 0 || first_valid;
    res[i].n_matches = v ? n_matches[i] : 0;
    res[i].n_queries = v ? qcnt[i] : 0;
}

static int finish_batch(odo_ctx* c, int set, int n, odo_pair_result* h_results) {
    if (!h_results) return ODO_OK;
    int e;
    if ((e = sync_all(c))) return e;
    auto& P = c->pb[set];
    HIPCHK(hipMemcpy(h_results, P.res, n * sizeof(odo_pair_result), hipMemcpyDeviceToHost));
    std::vector<int> nm(n);
    HIPCHK(hipMemcpy(nm.data(), P.n_matches, n * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> nq(n);
    HIPCHK(hipMemcpy(nq.data(), c->qcnt[set], n * sizeof(int), hipMemcpyDeviceToHost));
    // n_matches and the kNN-2 query counts into the result records
    for (int i = 0; i < n; i++) {
        h_results[i].n_matches = c->valid_h[i] ? nm[i] : 0;
        h_results[i].n_queries = c->valid_h[i] ? nq[i] : 0;
    }
    return ODO_OK;
}

// The previous batch's last frame into slot 0 of set `s`
// (Tracking::mLastFrame) on stream `st`, after that batch's geometry when it
// ran on its pair stream.
static int roll_last_frame(odo_ctx* c, hipStream_t st, int s) {
    if (c->geo_rec[c->seq_set]) HIPCHK(hipStreamWaitEvent(st, c->ev_geo[c->seq_set], 0));
    const FrameSlot src = frame_at(c, fbase(c, c->seq_set) + c->seq_n), dst = frame_at(c, fbase(c, s));
    launch_copy_frame(st, src.kps, src.desc, src.kun, src.xyz, src.ur, src.nkp, dst.kps, dst.desc, dst.kun, dst.xyz,
                      dst.ur, dst.nkp, c->kp_cap);
    return ODO_OK;
}

// The kNN-2 launch of the n pairs of set `s`, in the context's kernel form
void odo::launch_set_knn2(odo_ctx* c, hipStream_t st, int s, int n) {
    const size_t KC = (size_t)c->kp_cap;
    const FrameSlot f = frame_at(c, fbase(c, s));
    if (c->knn_mx)
        launch_knn2_f4(st, f.desc, f.nkp, KC * 32, f.desc + KC * 32, f.nkp + 1, KC * 32, c->knn_idx[s], c->knn_dist[s],
                       KC, c->kp_cap, n, c->qlist[s], c->qcnt[s], KC);
    else
        launch_knn2(st, f.desc, f.nkp, KC * 32, f.desc + KC * 32, f.nkp + 1, KC * 32, c->knn_idx[s], c->knn_dist[s],
                    KC, c->kp_cap, n, c->qlist[s], c->qcnt[s], KC, c->knn_split, (size_t)c->maxb * KC);
}

// kNN-2 of the batch's pairs on stream `st` (an event pair around it in timing mode 2)
int odo::run_knn(odo_ctx* c, hipStream_t st, int s, int n) {
    const FrameSlot f = frame_at(c, fbase(c, s));
    // the query frames' VO landmarks first: kNN-2 runs on their keypoints only
    const float mThDepth = c->cfg.calib.mbf * c->cfg.calib.th_depth / c->cfg.calib.fx;
    launch_vo_lm(st, f.xyz, f.nkp, c->kp_cap, 0, mThDepth, c->lm_bits[s], c->lm_words, c->qlist[s], c->qcnt[s], n);
    int kt = -1;
    if (c->ktiming) {
        kt = c->kt_next;
        if (c->kt_pending == odo_ctx::KT_RING) {  // slot reused: fold its time first
            int e;
            if ((e = kt_collect(c, kt))) return e;
            c->kt_pending--;
        }
        HIPCHK(hipEventRecord(c->kt0[kt], st));
    }
    c->last_knn_set = s;  // odo_knn_replay_time
    c->last_knn_n = n;
    if (!(c->skip & 8)) launch_set_knn2(c, st, s, n);
    if (kt >= 0) {
        HIPCHK(hipEventRecord(c->kt1[kt], st));
        c->kt_next = (kt + 1) % odo_ctx::KT_RING;
        c->kt_pending++;
    }
    tmark(c, 10, st);
    return ODO_OK;
}

// What differs between the callers of track_batch
struct BatchOpts {
    // a track_host batch: its depth reads must stay on the extraction stream
    // (ev_in_free, ev_depth_done)
    bool host_call = false;
    // the caller queues the result copy on the batch's pair stream
    // (*pair_stream) and records the set's PnP-done event after it
    bool defer_results = false;
};

// Queue one batch (arguments checked by the callers). No host sync.
static int track_batch(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n, const BatchOpts& opts,
                       hipStream_t* pair_stream = nullptr) {
    int e;
    // ---- 1. has the latch its value? Decided before this call queues
    // anything: a not-ready query leaves hipErrorNotReady as the thread's last
    // error, cleared here
    bool latched = false;
    if (c->latch_rec && __atomic_load_n(c->latch_set_h, __ATOMIC_ACQUIRE) != 0) {
        const hipError_t q = hipEventQuery(c->ev_latch);
        if (q == hipSuccess) latched = true;
        else if (q == hipErrorNotReady) (void)hipGetLastError();
        else return fail(ODO_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
    }
    const int s = next_set(c);
    // ---- 2. extraction stream: set s is free, batch b - PYR_WAIT is done
    if ((e = queue_batch_waits(c))) return e;
    tmark(c, 0, c->stream);
    // device inputs: the keypoint geometry (undistort, depth) and the slot-0
    // roll run at the head of the batch's pair stream instead of at the end of
    // the extraction stream, the step's critical path (round 6: 152.0-152.6 vs
    // 150.9-151.3 k frames/s, three alternations on one box, profiles/r06_d).
    // Not for the ADAPTIVE extractors (geometry inside their finalize), stage
    // timing (marks per stream) and host inputs.
    const bool geo_pair = !c->adaptive && !c->adaptive_orb && !c->timing && !opts.host_call;
    // ---- 3. the roll
    if (c->has_prev && !geo_pair && (e = roll_last_frame(c, c->stream, s))) return e;
    // ---- 4. extraction
    // (Round 6 measured ev_xdone completed by the last extraction kernel,
    // hipExtLaunchKernel's stop event, instead of a marker packet: with the
    // runtime's worker-thread dispatch the pair stream's wait on it did not
    // always hold (a batch's kNN-2 started before the previous batch's, seen
    // in the step marks), and the step was no faster. Not kept.)
    if ((e = run_extract(c, s, d_bgr, d_depth, n, 1, !geo_pair))) return e;
    // ---- 5. head of the batch's pair stream. The two pair streams take
    // alternate batches, so one batch's long RANSAC / PnP overlaps the next
    // batch's pair stages. RANSAC's rand() words depend on the pair seeds
    // only: they are queued ahead of the wait for the extraction, on the
    // stream that reads them (no marker in between).
    hipStream_t ps = (c->batch_counter & 1) ? c->pstream2 : c->pstream;
    if (pair_stream) *pair_stream = ps;
    if (c->pdone_rec[s] && (e = wait_pnp_done(c, ps, s))) return e;
    HIPCHK(hipEventRecord(c->ev_xdone[s], c->stream));
    launch_ransac_raw(ps, c->rscr[s], n, c->match_cap, c->mask_words, c->rcfg, (uint64_t)c->cfg.seed, c->pair_counter,
                      nullptr);
    HIPCHK(hipStreamWaitEvent(ps, c->ev_xdone[s], 0));
    if (geo_pair) {
        if (c->has_prev && (e = roll_last_frame(c, ps, s))) return e;
        const FrameSlot f = frame_at(c, fbase(c, s) + 1);
        launch_kp_geometry(ps, f.kps, f.nkp, d_depth, (size_t)c->W * c->H, c->W, c->cal, f.kun, f.xyz, f.ur, c->kp_cap,
                           n);
        HIPCHK(hipEventRecord(c->ev_geo[s], ps));
    }
    c->geo_rec[s] = geo_pair;
    // kNN-2 here and not on the extraction stream, the critical one, which
    // goes on to the next batch
    if ((e = run_knn(c, ps, s, n))) return e;
    // ---- 6. pair stages
    c->valid_h.assign(n, 1);
    c->valid_h[0] = c->has_prev ? 1 : 0;
    if (!(c->skip & 4) && (e = run_pairs(c, ps, s, n, latched, opts.defer_results))) return e;
    // ---- 7. bookkeeping
    c->pdone_rec[s] = true;
    c->seq_set = s;
    c->seq_n = n;
    c->view_set = s;
    c->last_n = n;
    c->lm_n = -1;
    c->view_mode = (c->skip & 5) ? -1 : c->odo_mode;
    c->view_rb = (int)(c->batch_counter & 1);
    c->has_prev = true;
    c->pair_counter += (uint64_t)n;
    c->batch_counter++;
    return ODO_OK;
}

// track_batch with the result records copied into page-locked host memory
// asynchronously (on the batch's pair stream, after its PnP): no host sync, so
// batches keep streaming; the records are valid after odo_synchronize().
static int track_batch_async(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n,
                             odo_pair_result* h_results, bool host_call) {
    const int first_valid = c->has_prev ? 1 : 0;
    BatchOpts opts;
    opts.host_call = host_call;
    opts.defer_results = true;
    hipStream_t st = nullptr;  // the batch's pair stream (its PnP ran there last)
    int e;
    if ((e = track_batch(c, d_bgr, d_depth, n, opts, &st))) return e;
    const int s = c->view_set;
    auto& P = c->pb[s];
    if ((e = wait_pnp_done(c, st, s))) return e;
    hipLaunchKernelGGL(k_res_patch, dim3((n + 255) / 256), dim3(256), 0, st, P.res, P.n_matches, c->qcnt[s], n,
                       first_valid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_results, P.res, (size_t)n * sizeof(odo_pair_result), hipMemcpyDeviceToHost, st));
    // the batch that next reuses set s waits for this event: include the copy
    HIPCHK(hipEventRecord(c->ev_pnp_done[s], st));
    c->pdone_st[s] = st;
    return ODO_OK;
}

// Host inputs (main.cpp:93-102 hands Track() images in host memory): the
// upload of this batch goes to staging buffer k on the copy stream and the
// extraction stream waits for it, so it overlaps the compute of the batches
// already queued. Buffer k is rewritten only after the extraction that last
// read it (two batches earlier) is done. The call returns once the host
// buffers have been consumed (the caller may refill them), on the error path
// too; with pinned buffers (odo_host_alloc, or hipHostRegister'ed) the DMA
// engines read them directly, pageable ones are staged by the runtime.
// sparse: only the BGR frames are uploaded and the extraction reads the
// keypoints' depth pixels in place through the mapped pointer (the depth
// buffer stays in use until ev_depth_done, odo_host_depth_query / _wait).
// async_res: the result records stream to page-locked memory as in
// odo_track_batch_async (no host sync).
static int track_host(odo_ctx* c, const uint8_t* bgr, const uint16_t* depth, int n, bool sparse,
                      odo_pair_result* h_results, odo_pair_result* async_res) {
    if (!c || !bgr || !depth || n <= 0 || n > c->maxb) return fail(ODO_ERR_ARG, "bad track args");
    void* dmap = nullptr;
    if (sparse) {
        // only HIP page-locked host memory may be read by a kernel (pageable
        // memory would fault): check the allocation type before taking its
        // device pointer
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, depth) != hipSuccess || attr.type != hipMemoryTypeHost ||
            hipHostGetDevicePointer(&dmap, (void*)depth, 0) != hipSuccess || !dmap) {
            (void)hipGetLastError();
            return fail(ODO_ERR_ARG, "sparse depth: depth must be page-locked host memory (odo_host_alloc)");
        }
    }
    const int k = c->in_next;
    c->in_next ^= 1;
    if (c->in_used[k]) HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_in_free[k], 0));
    const size_t px = (size_t)n * c->W * c->H;
    HIPCHK(hipMemcpyAsync(c->bgr_in[k], bgr, px * 3, hipMemcpyHostToDevice, c->cstream));
    if (!sparse) HIPCHK(hipMemcpyAsync(c->depth_in[k], depth, px * 2, hipMemcpyHostToDevice, c->cstream));
    HIPCHK(hipEventRecord(c->ev_in_copied[k], c->cstream));
    int e = ODO_OK;
    if (hipStreamWaitEvent(c->stream, c->ev_in_copied[k], 0) != hipSuccess) e = fail(ODO_ERR_DEVICE, "hipStreamWaitEvent");
    const uint16_t* dd = sparse ? (const uint16_t*)dmap : c->depth_in[k];
    BatchOpts opts;
    opts.host_call = true;
    if (!e) e = async_res ? track_batch_async(c, c->bgr_in[k], dd, n, async_res, true)
                          : track_batch(c, c->bgr_in[k], dd, n, opts);
    if (!e) {
        // everything that reads staging buffer k (and a sparse batch's depth
        // frames) is queued on the extraction stream
        if (hipEventRecord(c->ev_in_free[k], c->stream) != hipSuccess) e = fail(ODO_ERR_DEVICE, "hipEventRecord");
        c->in_used[k] = true;
        if (!e && sparse) {
            if (hipEventRecord(c->ev_depth_done, c->stream) != hipSuccess) e = fail(ODO_ERR_DEVICE, "hipEventRecord");
            c->depth_busy = true;
        }
    }
    // the host buffers are free once their copy has landed, whatever happened
    // after the copy was queued
    const hipError_t se = hipEventSynchronize(c->ev_in_copied[k]);
    if (e) return e;
    if (se != hipSuccess) return fail(ODO_ERR_DEVICE, std::string("hipEventSynchronize: ") + hipGetErrorString(se));
    return finish_batch(c, c->view_set, n, h_results);
}

extern "C" {

// Extraction only (no pairs, no roll): frames land in the set the next
// tracked batch will use, so the tracking sequence state is untouched.
int odo_extract_batch(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n) {
    if (!c || !d_bgr || !d_depth || n <= 0 || n > c->maxb) return fail(ODO_ERR_ARG, "bad extract args");
    int e;
    if ((e = sync_all(c))) return e;
    const int set = next_set(c);
    tmark(c, 0, c->stream);
    if ((e = run_extract(c, set, d_bgr, d_depth, n, 1))) return e;
    c->view_set = set;
    c->last_n = n;
    c->lm_n = -1;
    c->view_mode = -1;  // no pairs in view
    return ODO_OK;
}

int odo_track_batch(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n, odo_pair_result* h_results) {
    if (!c || !d_bgr || !d_depth || n <= 0 || n > c->maxb) return fail(ODO_ERR_ARG, "bad track args");
    int e;
    if ((e = track_batch(c, d_bgr, d_depth, n, BatchOpts{}))) return e;
    return finish_batch(c, c->view_set, n, h_results);
}

int odo_track_batch_async(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n, odo_pair_result* h_results) {
    if (!h_results) return fail(ODO_ERR_ARG, "null results");
    if (!c || !d_bgr || !d_depth || n <= 0 || n > c->maxb) return fail(ODO_ERR_ARG, "bad track args");
    return track_batch_async(c, d_bgr, d_depth, n, h_results, false);
}

// Position the sequence (SURVEY §8(e) frames mode): the next batch's pair p
// gets the global pair index pair_index + p (its per-pair RANSAC seed); with
// keep_prev = 0 the next batch's first frame starts a sequence segment (no
// pair with the previous call's last frame: a rank's halo frame). The latch
// and the ADAPTIVE thresholds are kept.
int odo_seek(odo_ctx* c, uint64_t pair_index, int keep_prev) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    c->pair_counter = pair_index;
    if (!keep_prev) c->has_prev = false;
    return ODO_OK;
}

int odo_track_batch_host(odo_ctx* c, const uint8_t* bgr, const uint16_t* depth, int n, odo_pair_result* h_results) {
    return track_host(c, bgr, depth, n, false, h_results, nullptr);
}

int odo_track_batch_host_async(odo_ctx* c, const uint8_t* bgr, const uint16_t* depth, int n,
                               odo_pair_result* h_results) {
    if (!h_results) return fail(ODO_ERR_ARG, "null results");
    return track_host(c, bgr, depth, n, false, nullptr, h_results);
}

int odo_track_batch_host_sparse_depth(odo_ctx* c, const uint8_t* bgr, const uint16_t* depth, int n,
                                      odo_pair_result* h_results) {
    return track_host(c, bgr, depth, n, true, h_results, nullptr);
}

int odo_host_depth_query(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    if (!c->depth_busy) return 0;
    const hipError_t q = hipEventQuery(c->ev_depth_done);
    if (q == hipSuccess) {
        c->depth_busy = false;
        return 0;
    }
    if (q == hipErrorNotReady) return 1;
    return fail(ODO_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
}

int odo_host_depth_wait(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    if (!c->depth_busy) return ODO_OK;
    HIPCHK(hipEventSynchronize(c->ev_depth_done));
    c->depth_busy = false;
    return ODO_OK;
}

void* odo_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        fail(ODO_ERR_DEVICE, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

int odo_host_free(void* p) {
    if (p) HIPCHK(hipHostFree(p));
    return ODO_OK;
}

}  // extern "C"
