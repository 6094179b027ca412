/*
 * odo.h — C-ABI of the MI355X-native per-frame odometry hot path
 * (ORB extraction + Hamming kNN matching + RANSAC-wrapped PnP), the drop-in
 * boundary for ttwang0303/Adaptive-RGBD-Localization-Mappig.
 *
 * Implemented by libodo_hip.so (hand-written HIP for gfx950). Plain pointers
 * and sizes only; every function returns an int status (ODO_OK = 0, < 0 on
 * error, message via odo_last_error()). The library never falls back to a CPU
 * implementation: without a usable gfx950 device odo_create() fails.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * the reference tree). INTEGRATION.md shows the reference-side bindings.
 */
#ifndef ODO_H
#define ODO_H

#include <stddef.h>
#include <stdint.h>

#include "odo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ODO_OK 0
#define ODO_ERR_ARG (-1)
#define ODO_ERR_DEVICE (-2)
#define ODO_ERR_CAPACITY (-3)
#define ODO_ERR_STATE (-4)

/* odo_config.detector: Extractor(detector, descriptor, mode) (extractor.cpp:14) */
#define ODO_DETECTOR_ORB_SLAM2 0      /* ORB_SLAM2 / ORB_SLAM2 / NORMAL (main.cpp:19-21, the reference default) */
#define ODO_DETECTOR_ADAPTIVE_FAST 1  /* FAST / ORB / ADAPTIVE: 3x3 grid-adapted FAST + cv::ORB descriptor */
#define ODO_DETECTOR_ADAPTIVE_ORB 2   /* ORB / ORB / ADAPTIVE: 3x3 grid-adapted cv::ORB detector (Harris,
                                         8 levels; detectoradjuster.cpp:29) + cv::ORB descriptor */

/* odo_config.forms: which of several bit-identical kernel forms runs (all
 * produce the same results; the parity tests run each). 0 everywhere = the
 * defaults. These are explicit per-context settings: the library reads no
 * environment variables (measurement knobs exist only in the separate
 * tuning build, make -C ... tuning). */
#define ODO_KNN_FORM_FP4 0   /* default: exact sign-vector products on the matrix cores (FP4 operands) */
#define ODO_KNN_FORM_VALU 1  /* xor + popcount on the VALUs (also taken for train sets above 8192) */
#define ODO_PYRAMID_FORM_AUTO 0   /* default: FUSED for batches of >= 128 frames, CHAIN below */
#define ODO_PYRAMID_FORM_CHAIN 1  /* k_gray + one k_resize launch per level, then the blur launch */
#define ODO_PYRAMID_FORM_FUSED_NOBLUR 2  /* one launch, a workgroup per frame builds every level;
                                            the blur as its own launch */
#define ODO_PYRAMID_FORM_FUSED 3  /* one launch: every level and its 7x7 blur (falls back to the
                                     chain / a separate blur launch where its host checks fail) */
typedef struct odo_kernel_forms {
    int32_t knn;                    /* ODO_KNN_FORM_* */
    int32_t knn_split;              /* VALU form: train splits per query block, 1..8 (0 = 2) */
    int32_t ransac_lanes_min_open;  /* open pairs from which the second RANSAC launch takes the
                                       lane-per-hypothesis kernel (0 = 32) */
    int32_t pyramid;                /* ODO_PYRAMID_FORM_*: gray + pyramid levels */
    int32_t ransac_first_hyps;      /* batched path: hypotheses per pair in the first RANSAC
                                       evaluation launch, 1..64 (0 = 2) */
} odo_kernel_forms;

/* Layout version of the structs below. odo_config starts with its own size,
 * which odo_default_config fills and odo_create checks, so a caller built
 * against a header with a different odo_config fails with ODO_ERR_ARG instead
 * of reading past its struct. */
#define ODO_ABI_VERSION 5
int odo_abi_version(void);  /* ODO_ABI_VERSION of the library */

typedef struct odo_config {
    uint32_t struct_size;       /* sizeof(odo_config): set by odo_default_config */
    int32_t width, height;      /* frame size (all frames of a context share it) */
    int32_t max_batch;          /* frames per odo_track_batch() call */
    odo_orb_params orb;         /* ORBextractor(nFeatures,1.2,8,20,7) extractor.cpp:86 */
    odo_calib calib;            /* Utils/common.h Calibration */
    float nn_ratio;             /* Matcher(0.9f) tracking.cpp:197 */
    odo_ransac_params ransac;   /* Ransac(200,20,3.0,4) odometry.cpp:28 */
    uint32_t seed;              /* per-pair RNG seed base (replaces srand(clock()), main.cpp:27) */
    int32_t detector;           /* ODO_DETECTOR_* */
    odo_adaptive_params adaptive; /* ADAPTIVE grid (Extractor::CreateAdaptiveDetector, extractor.cpp:55-77) */
    odo_kernel_forms forms;     /* bit-identical kernel alternatives (tests / A-B); zero = defaults */
} odo_config;

typedef struct odo_ctx odo_ctx;

/* Fill cfg with the reference's defaults (FR1 calibration, nfeatures=1000)
 * and its struct_size. */
void odo_default_config(odo_config* cfg, int width, int height, int max_batch);

/* Context: owns the HIP stream, HBM scratch and the cross-frame state the
 * reference keeps in globals or detector objects (previous frame,
 * DepthCovariance latch, the ADAPTIVE grid's per-cell FAST thresholds). */
odo_ctx* odo_create(const odo_config* cfg, int device);
void odo_destroy(odo_ctx* ctx);
const char* odo_last_error(void);
void* odo_stream(odo_ctx* ctx);               /* hipStream_t, for callers that share streams */
int odo_reset(odo_ctx* ctx);                  /* forget previous frame, latch, adaptive thresholds */
int odo_set_latch(odo_ctx* ctx, double cov);  /* NaN = unlatched */
double odo_get_latch(odo_ctx* ctx);

/* ---- Batched hot path: Tracking::Track for n frames (tracking.cpp:38-78 minus
 * map bookkeeping): Frame::Frame + ExtractFeatures (frame.cpp:18,135), then for
 * every frame t with a predecessor: UpdateLastFrame VO landmarks
 * (tracking.cpp:136), Matcher::KnnMatch (matcher.cpp:55), Odometry::Compute
 * ADAPTIVE_RBA = Ransac::Iterate + PnPSolver::Compute (odometry.cpp:105-116),
 * with F1 pose = identity (DESIGN.md §3 batched contract).
 * d_bgr: device [n][H][W][3] u8, d_depth: device [n][H][W] u16 (x5000).
 * results[n] (host): results[i] is the pair (frame i-1 -> frame i); frame -1
 * is the last frame of the previous call. When h_results is NULL the call is
 * asynchronous: the work runs on the library's streams (extraction =
 * odo_stream(), plus two pair streams), d_bgr is read by the
 * extraction stream and d_depth by the batch's pair stream (the keypoint
 * geometry), and odo_synchronize() waits for all of them. */
int odo_track_batch(odo_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_depth, int n,
                    odo_pair_result* h_results);
/* Same with host inputs, as Tracking::Track receives them (main.cpp:93-102).
 * The H2D upload runs on the context's copy stream into one of two device
 * staging buffers and overlaps the compute of the batches already queued; the
 * call returns once the host buffers have been consumed (the caller may refill
 * them) and the batch is queued. Pinned buffers (odo_host_alloc) are read by
 * the DMA engines directly; pageable ones are staged by the HIP runtime. With
 * h_results non-null it waits for the batch and fills the results. */
int odo_track_batch_host(odo_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, int n,
                         odo_pair_result* h_results);
/* odo_track_batch_host with the depth frames read in place: depth must be
 * page-locked host memory from odo_host_alloc (else ODO_ERR_ARG). Only the BGR
 * frames are uploaded; the keypoint geometry kernel reads each keypoint's depth
 * pixel through the mapped pointer, so about 2000 small reads per frame cross
 * PCIe instead of the 614 kB depth image. The BGR buffer is consumed when the
 * call returns; the DEPTH buffer must stay valid and unchanged until the batch
 * has read it: odo_host_depth_query() returns 0 / odo_host_depth_wait() returns
 * (or odo_synchronize(), or the call itself when h_results is set). */
int odo_track_batch_host_sparse_depth(odo_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, int n,
                                      odo_pair_result* h_results);
/* Whether the last odo_track_batch_host_sparse_depth batch may still read its
 * depth buffer: 1 = in use (do not refill it), 0 = released (< 0 on error).
 * odo_host_depth_wait blocks until it is released (odo_synchronize too). */
int odo_host_depth_query(odo_ctx* ctx);
int odo_host_depth_wait(odo_ctx* ctx);
/* odo_track_batch_host with the result records streamed to PAGE-LOCKED host
 * memory as odo_track_batch_async does (no host sync for the results; the host
 * input buffers are consumed when the call returns): the from-host form of the
 * SURVEY §8(e) frames mode, one PCIe upload per rank. */
int odo_track_batch_host_async(odo_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, int n,
                               odo_pair_result* h_results);
/* odo_track_batch with the n result records copied into PAGE-LOCKED host memory
 * (odo_host_alloc) asynchronously after the batch's PnP: no host sync, the
 * records are valid after odo_synchronize(). Used to stream results. */
int odo_track_batch_async(odo_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_depth, int n,
                          odo_pair_result* h_results);
/* Sequence position (SURVEY §8(e) frames mode, replaces the implicit global
 * frame counter of Tracking): the next batch's pair p uses global pair index
 * pair_index + p for its RANSAC seed; keep_prev = 0 makes the next batch's
 * first frame a segment start (a rank's halo frame: extracted, no pair with
 * the previous call). The DepthCovariance latch and ADAPTIVE thresholds stay. */
int odo_seek(odo_ctx* ctx, uint64_t pair_index, int keep_prev);
/* Page-locked host memory for input frames (decode straight into it so the
 * upload needs no extra host copy). NULL on failure; free with odo_host_free. */
void* odo_host_alloc(size_t bytes);
int odo_host_free(void* p);
/* Extraction only (frames land in the batch slots; no pairs). Device inputs. */
int odo_extract_batch(odo_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_depth, int n);
int odo_synchronize(odo_ctx* ctx);

/* ---- Odometry::Compute back-end of the batched path (odometry.cpp:43-117).
 * Every odo_track_batch* entry point (device, host, sparse-depth, async) runs
 * the context's mode:
 *   ADAPTIVE_RBA   Ransac::Iterate + PnPSolver::Compute (odometry.cpp:105-116),
 *                  the default.
 *   RANSAC         Ransac::Iterate alone (odometry.cpp:81-92).
 *   ADAPTIVE_RICP  Ransac::Iterate, then when mvInliers.size() < min_inliers or
 *                  rmse * rmse_scale >= refine_at (odometry.cpp:52, evaluated in
 *                  float as there) GeneralizedICP::Compute on Ransac's
 *                  mpSourceCloud / mpTargetCloud (ransac.cpp:161-189: the
 *                  depth-valid matches in KnnMatch order), from the identity
 *                  when rmse * rmse_scale >= reset_at (odometry.cpp:53-58;
 *                  T12 = identity if GICP does not converge), else from
 *                  Ransac::mT12 (odometry.cpp:60-65; Ransac::mT12 if it does
 *                  not). Decision, clouds, GICP and the pose stay on the
 *                  device: a batch gains no host synchronisation.
 * In RANSAC and ADAPTIVE_RICP odo_pair_result.T12, rmse, n_good, n_inliers,
 * ransac_ok, visited, n_sweeps and n_fit_points are what ADAPTIVE_RBA reports;
 * Tcw is the pose Odometry::Compute sets (the chosen T12 times F1's pose, the
 * identity in the batched contract; odometry.cpp:70-72, 85-87), so
 * odo_chain_poses and the trajectory writer apply unchanged; PnP does not
 * run; the mask odo_get_pair returns as pnp_inliers holds F2's inlier flags,
 * SetInlier(m.trainIdx) for every m of mvInliers (odometry.cpp:75-76, 90-91),
 * and odo_pair_result.pnp_inliers is the number of flags set. A pair without a
 * predecessor reports what ADAPTIVE_RBA reports for it. */
#define ODO_ODOMETRY_ADAPTIVE_RBA  0   /* default */
#define ODO_ODOMETRY_RANSAC        1   /* odometry.cpp:81-92 */
#define ODO_ODOMETRY_ADAPTIVE_RICP 2   /* odometry.cpp:46-78 */
/* The reference's constants: 20, 10.f, 7.f, 20.f, GeneralizedICP(10, 0.07)
 * (odometry.cpp:15, 52-53). */
void odo_default_ricp_params(odo_ricp_params* p);
/* Select the mode, from the next batch on; p: ADAPTIVE_RICP's constants (NULL =
 * the defaults; ignored by the other modes). Synchronises the context's
 * streams. ODO_ERR_ARG: unknown mode, gicp_iterations < 1, gicp_max_corr_dist
 * <= 0 (or not finite), a non-finite rmse_scale / refine_at / reset_at.
 * ODO_ERR_CAPACITY: ADAPTIVE_RICP on a context whose keypoint capacity exceeds
 * GICP's 16384 points per cloud. The sequence state (previous frame, latch,
 * pair counter, ADAPTIVE thresholds) is kept, and odo_reset keeps the mode. The
 * GICP scratch is allocated by the first switch to ADAPTIVE_RICP; a context
 * left in the default mode allocates and launches nothing for this. */
int odo_set_odometry(odo_ctx* ctx, int mode, const odo_ricp_params* p);
int odo_get_odometry(odo_ctx* ctx);   /* ODO_ODOMETRY_*, < 0 on error */
/* Pair i of the last batch when it ran in ADAPTIVE_RICP (else ODO_ERR_STATE):
 * the record and, optionally, the pair's mpSourceCloud / mpTargetCloud (src /
 * tgt: cap points of 3 floats each, r->n_cloud written; more than cap points:
 * ODO_ERR_CAPACITY after copying cap). The clouds of a pair on branch 0 are
 * not built (n_cloud = 0). Synchronises. */
int odo_get_ricp(odo_ctx* ctx, int i, odo_ricp_result* r, float* src, float* tgt, int cap);

/* Read back frame features of batch slot i (0 <= i < n of the last call). */
int odo_get_frame(odo_ctx* ctx, int i, orb_kp* kps, uint8_t* desc, float* kps_un, float* xyz,
                  float* u_right, int cap, int* n);
/* Read back pair i's matches (KnnMatch output), RANSAC inlier mask over the
 * sorted good matches, and PnP inlier mask over frame-i keypoints. */
int odo_get_pair(odo_ctx* ctx, int i, odo_dmatch* matches, int match_cap, int* n_matches,
                 odo_dmatch* good_sorted, int* n_good, uint8_t* ransac_inliers /* n_good */,
                 uint8_t* pnp_inliers /* frame kps */, int32_t* f2_src);

/* ---- Per-stage entry points (host buffers, synchronous) ---- */

/* Extractor::Extract + Frame::ExtractFeatures (extractor.cpp:39, frame.cpp:135):
 * BGR8 (or gray when channels==1) + optional depth16 -> keypoints,
 * 32-byte descriptors, undistorted points, camera xyz and right coordinate.
 * With ODO_DETECTOR_ADAPTIVE_FAST / _ORB every call advances the cell thresholds. */
int odo_extract(odo_ctx* ctx, const uint8_t* img, int channels, const uint16_t* depth,
                orb_kp* kps, uint8_t* desc, float* kps_un, float* xyz, float* u_right, int cap,
                int* n);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) as used by Matcher::KnnMatch
 * (matcher.cpp:60). idx/dist: nq x 2 (trainIdx -1 / INT_MAX when absent). */
int odo_knn2_hamming(odo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx,
                     int32_t* dist);

/* Ransac::Iterate(Frame*,Frame*,m12) (ransac.cpp:155). xyz1/xyz2: mvKeys3Dc of
 * both frames (n1/n2 points). rng: in/out glibc rand() state; latch: in/out
 * DepthCovariance static (NaN = unlatched). inliers: capacity n12. Returns the
 * bool result (1/0) in *ok. */
int odo_ransac(odo_ctx* ctx, const odo_dmatch* m12, int n12, const float* xyz1, int n1,
               const float* xyz2, int n2, const odo_ransac_params* p, odo_rng* rng, double* latch,
               float T12[16], float* rmse, odo_dmatch* inliers, int* n_inliers, int* ok);

/* ---- Hypotheses mode of Ransac::Iterate: the
 * hypotheses of one pair are sharded over ranks; each rank evaluates
 * [h0, h1) from the same rand() stream, the per-hypothesis summaries are
 * all-gathered (16..64 B each), every rank replays the ordered fold, and the
 * rank that owns the winner supplies T12 and the inlier list.
 * 1) odo_ransac_hyps: same inputs as odo_ransac (rng and latch are read, the
 *    latch is set if unlatched, rng is NOT advanced); writes summaries of
 *    [h0, h1) to out[0 .. h1-h0) and keeps the range's inlier masks in ctx. */
int odo_ransac_hyps(odo_ctx* ctx, const odo_dmatch* m12, int n12, const float* xyz1, int n1,
                    const float* xyz2, int n2, const odo_ransac_params* p, const odo_rng* rng,
                    double* latch, int h0, int h1, odo_hyp_summary* out, int* n_good);
/* 2) the ordered fold over all H = p->iterations summaries (host only, no
 *    device needed): identical on every rank. */
int odo_ransac_fold(const odo_hyp_summary* all, int H, int n_good, const odo_ransac_params* p,
                    odo_ransac_fold_result* r);
/* 3) outputs of the folded run from the last odo_ransac_hyps of this ctx:
 *    rng advanced by exactly the visited draws (every rank); T12, rmse,
 *    inliers and ok are valid when *owner = 1 (best_h in this rank's range,
 *    or no valid hypothesis: identity fallback), otherwise they come from the
 *    owner rank (broadcast). */
int odo_ransac_hyps_finish(odo_ctx* ctx, const odo_ransac_fold_result* r, odo_rng* rng, float T12[16],
                           float* rmse, odo_dmatch* inliers, int* n_inliers, int* ok, int* owner);

/* ---- The same hypotheses mode with the exchange in device memory (RCCL
 * collectives on device buffers, no host staging; ransac.cpp:233-249 is the
 * ordered fold it feeds). All work is queued on odo_stream(ctx); a caller
 * orders its collectives after it on that stream.
 * 1) odo_ransac_hyps_dev: as odo_ransac_hyps, the summaries of [h0, h1) into
 *    the DEVICE buffer d_block ((h1-h0) x 64 B, odo_hyp_summary layout); no
 *    host synchronisation. The gathered array must hold all H summaries in
 *    hypothesis order (contiguous rank ranges). When the pair never samples
 *    (Iterate returns before its loop: too few matches) the default summaries
 *    are copied on odo_stream(ctx) and this call synchronises that stream
 *    before it returns (step 4 does the same for its payload). */
int odo_ransac_hyps_dev(odo_ctx* ctx, const odo_dmatch* m12, int n12, const float* xyz1, int n1,
                        const float* xyz2, int n2, const odo_ransac_params* p, const odo_rng* rng,
                        double* latch, int h0, int h1, void* d_block, int* n_good);
/* 2) the ordered fold over the gathered device array d_all (H summaries) on
 *    the GPU; the odo_ransac_fold_result record is written to device memory
 *    d_fold (same values as odo_ransac_fold). */
int odo_ransac_fold_dev(odo_ctx* ctx, const void* d_all, int H, void* d_fold);
/* 3) size in int32 words of the payload buffer of step 4 (32 header words +
 *    4 per good match). */
int odo_ransac_hyps_payload_words(odo_ctx* ctx);
/* 4) the folded run's outputs: this rank's rand() state advanced on the
 *    device by exactly the visited draws; the owner of the winner (its range
 *    holds best_h; rank 0 when rank0 != 0 for the identity fallback or a pair
 *    that never sampled) writes the payload [T12 bits x16, rmse bits, ok,
 *    n_inliers, visited, 12 x 0, inliers as odo_dmatch...] to d_payload and
 *    every other rank writes zeros, so an int32 SUM all-reduce over the ranks
 *    leaves the owner's payload everywhere. */
int odo_ransac_hyps_finish_dev(odo_ctx* ctx, const void* d_fold, int rank0, void* d_payload, int payload_words);
/* 5) synchronise and unpack a (reduced) payload and this rank's rand() state. */
int odo_ransac_hyps_result(odo_ctx* ctx, const void* d_payload, odo_rng* rng, float T12[16], float* rmse,
                           odo_dmatch* inliers, int* n_inliers, int* ok, int* visited);

/* PnPSolver::Compute (pnpsolver.cpp:17): Xw n x 3 (world), obs n x 3 (u,v,uR;
 * uR<0 = mono edge). outlier: out, per edge. Returns inliers in *n_inliers. */
int odo_pnp_motion_ba(odo_ctx* ctx, const float* Xw, const float* obs, int n, const odo_calib* calib,
                      const float Tcw_init[16], float Tcw_out[16], uint8_t* outlier, int* n_inliers);

/* PnPRansac::Compute (pnpransac.cpp:11-51), the RANSAC
 * PnP back-end: cv::solvePnPRansac(v3D, v2D, mK, noDist, r, t, false,
 * iterations = 500, reproj_err = 3.0f, confidence = 0.85, inliers) over the
 * frame's landmark observations. Xw: n x 3 world points (Landmark::GetWorldPos),
 * uv: n x 2 undistorted keypoints (mvKeysUn), in index order. n < 10 returns
 * res->ok = 0 without running (pnpransac.cpp:30); no model with more than 4
 * inliers gives ok = 0; a best model with exactly 5 non-planar inliers gives
 * ok = ODO_PNP_RANSAC_THROW (-1: OpenCV's final solvePnP asserts count >= 6
 * in its DLT start and throws; Tcw and rvec/tvec are then zero, the model,
 * mask and n_inliers are set). Test ok == 1 for success, never truthiness. inlier_mask (n, optional):
 * the RANSAC inliers (Frame::SetInlier); good_counts (iterations, optional):
 * inliers of every hypothesis, of which the first res->iterations_visited are
 * the ones RANSAC visited. Hypotheses, EPnP, counts, the ordered fold and the
 * Levenberg-Marquardt refinement all run on the GPU (k_pnpransac.hip).
 * Arguments: iterations < 1 runs one hypothesis (ptsetreg.cpp: niters =
 * MAX(maxIters, 1)), so good_counts holds max(iterations, 1) entries.
 * Refused with ODO_ERR_ARG: a null ctx / res / Xw / uv (points may be null
 * when n = 0), n < 0, confidence not in (0, 1) (NaN included: run()'s
 * CV_Assert); with ODO_ERR_CAPACITY: more than 65536 points, or
 * max(iterations, 1) x points above 2^28. A refused call writes none of its
 * outputs. reproj_err and the points are NOT validated, as in OpenCV, whose
 * findInliers tests err <= (float)(reproj_err * reproj_err): a NaN
 * reproj_err accepts nothing (ok = 0 after all iterations), 0 accepts only
 * an exactly zero error, a negative value acts as its magnitude. A
 * non-finite landmark or observation is never an inlier, and a hypothesis
 * drawn on one counts no inliers; every device loop has a fixed trip count,
 * so such input costs time only. */
#define ODO_PNP_RANSAC_THROW (-1)
int odo_pnp_ransac(odo_ctx* ctx, const float* Xw, const float* uv, int n, const odo_calib* calib, int iterations,
                   float reproj_err, double confidence, odo_pnp_ransac_result* res, uint8_t* inlier_mask,
                   int32_t* good_counts);

/* PnPRansac::Compute for a batch of frames in one launch chain (the batched
 * contract of odo_track_batch): problem p = observations [offs[p], offs[p+1])
 * of Xw / uv (offs[0] = 0, nprob + 1 entries); res[p] as odo_pnp_ransac
 * (problems with fewer than 10 observations: ok = 0, best_iter = -1);
 * inlier_mask (optional) over all offs[nprob] observations. nprob = 0
 * returns ODO_OK and writes nothing. Refused with ODO_ERR_ARG, besides what
 * odo_pnp_ransac refuses: nprob < 0, a null offs, offs[0] != 0, decreasing
 * offsets; with ODO_ERR_CAPACITY: more than 65535 problems, a problem of more
 * than 65536 points, max(iterations, 1) x offs[nprob] above 2^28. A refused
 * call writes none of its outputs. */
int odo_pnp_ransac_batch(odo_ctx* ctx, const float* Xw, const float* uv, const int32_t* offs, int nprob,
                         const odo_calib* calib, int iterations, float reproj_err, double confidence,
                         odo_pnp_ransac_result* res, uint8_t* inlier_mask);

/* GeneralizedICP(max_iterations, max_corr_dist)::Compute(source, target, guess)
 * (generalizedicp.cpp:11-22, 30-39, 65-89): the PCL
 * GICP refinement Odometry::Compute's ADAPTIVE_RICP mode runs on RANSAC's
 * matched clouds (odometry.cpp:46-78; the reference builds it with 10
 * iterations and 0.07 m). src/tgt: n x 3 (Ransac::mpSourceCloud /
 * mpTargetCloud). Fewer than 20 points in either cloud: *converged = 0 without
 * running (generalizedicp.cpp:33). T12 = the final transformation when
 * converged, identity otherwise (generalizedicp.cpp:76-88); iterations = ICP
 * iterations run, n_corr = correspondences of the last one. Covariances,
 * correspondences and the BFGS all run on the GPU (k_gicp.hip); neighbour
 * searches are brute force, so clouds hold at most 16384 points
 * (ODO_ERR_CAPACITY; RANSAC's matched clouds are a few hundred; whole clouds
 * go through odo_gicp_grid_batch or odo_gicp_dense). */
int odo_gicp(odo_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float guess[16],
             int max_iterations, double max_corr_dist, float T12[16], int* converged, int* iterations, int* n_corr);

/* GeneralizedICP::Compute for a batch of pairs in one launch chain: pair p =
 * source points [soffs[p], soffs[p+1]) of src, target points [toffs[p],
 * toffs[p+1]) of tgt (offsets start at 0, nprob + 1 entries), guesses 16 per
 * pair (NULL: identity); T12 16 per pair, converged / iterations / n_corr one
 * per pair, as odo_gicp. */
int odo_gicp_batch(odo_ctx* ctx, const float* src, const int32_t* soffs, const float* tgt, const int32_t* toffs,
                   const float* guesses, int nprob, int max_iterations, double max_corr_dist, float* T12,
                   int32_t* converged, int32_t* iterations, int32_t* n_corr);

/* GICP's computeCovariances by itself (the first launch of odo_gicp /
 * odo_gicp_batch, k_gicp_cov), for tests and diagnosis: cloud p = points
 * [offs[p], offs[p+1]) of P (n x 3; offsets start at 0, nprob + 1 entries); C
 * receives 9 doubles per point, the row-major 3 x 3 covariance of the point's 20
 * nearest neighbours in its own cloud with the eigenvalues replaced by
 * (1, 1, 1e-3). A cloud under 20 points gets zeros (GICP does not run on it).
 * The kernel works on a source and a target set per call: the batch is given
 * to it in both roles, C is the source set, and ODO_ERR_DEVICE is returned if
 * the target set differs from it in any bit. At most 16384 points per cloud
 * (ODO_ERR_CAPACITY). */
int odo_gicp_covariances(odo_ctx* ctx, const float* P, const int32_t* offs, int nprob, double* C);

/* odo_gicp_batch with grid neighbour searches (DESIGN §4 "Dense GICP"): every
 * cloud is binned into a uniform grid, the 20 covariance neighbours are found
 * over Chebyshev rings of cells and the ICP correspondence in the cells within
 * max_corr_dist of the query, with the results of the brute-force scans bit for
 * bit (T12, converged, iterations, n_corr equal odo_gicp_batch's on any pair
 * that accepts). A cloud holds at most 1048576 points (a 640 x 480 cloud with
 * leaf 0 fits), a call 32767 pairs and 2^29 points (ODO_ERR_CAPACITY).
 * cell: edge of the grid's cells in metres. 0 = chosen per cloud by the
 * library: max(extent / cbrt(8 n), slightly above max_corr_dist), extent the
 * cloud's longest side, n its points; then the ICP search is the 27 cells
 * around the query. The cell is doubled until the cloud's table fits 2^24
 * cells; no result depends on the cell. cell > 0 = forced (tests): a table
 * above 2^24 cells, or above 2^28 cells over the clouds of a call, is
 * ODO_ERR_CAPACITY; a cell below max_corr_dist widens the ICP search to about
 * ceil(max_corr_dist / cell) rings. A cloud that spans more than FLT_MAX on
 * an axis is held in one cell (a forced cell: ODO_ERR_CAPACITY). A transformed
 * source point outside the
 * target's grid is searched from the nearest cell; beyond max_corr_dist it has
 * no correspondence, as in the brute-force search.
 * ODO_ERR_ARG (nothing written): null pointers with non-zero sizes, offsets
 * not starting at 0 or decreasing, max_iterations < 1, max_corr_dist or cell
 * negative or not finite, a non-finite guess entry or coordinate, nprob < 0. */
int odo_gicp_grid_batch(odo_ctx* ctx, const float* src, const int32_t* soffs, const float* tgt,
                        const int32_t* toffs, const float* guesses, int nprob, int max_iterations,
                        double max_corr_dist, float cell, float* T12, int32_t* converged, int32_t* iterations,
                        int32_t* n_corr);
/* odo_gicp_covariances with the grid search: C equals it bit for bit on any
 * cloud it accepts. Every cloud has one role, so there is no source / target
 * echo check. cell as above (0: max_corr_dist counts as 0); at most 65535
 * clouds of 1048576 points and 2^29 points per call (ODO_ERR_CAPACITY). */
int odo_gicp_grid_covariances(odo_ctx* ctx, const float* P, const int32_t* offs, int nprob, float cell, double* C);

/* ---- Trajectory (host only) ----
 * Relative-pose chain of the batched contract: results[i].Tcw is frame i's
 * pose in frame i-1's camera coordinates, so Tcw(i) = Tcw_rel(i) * Tcw(i-1)
 * (Odometry::Compute's Tcw2 = T12 * Tcw1, odometry.cpp:110-112), starting
 * from Tcw_prev (the last pose of the previous batch; identity for a new
 * sequence). Pairs without a predecessor (n_matches == 0 at i == 0 of a
 * sequence) keep Tcw_prev. 4x4 row-major floats; products in double. */
int odo_chain_poses(const odo_pair_result* results, int n, const float Tcw_prev[16], float* Tcw_out);
/* Tracking::SaveTrajectory's line format (tracking.cpp:544-582): "timestamp
 * tx ty tz qx qy qz qw" of the camera centre twc = -Rcw^T tcw and
 * Converter::toQuaternion(Rwc) (Eigen Quaterniond from the double matrix,
 * converter.cpp:149-161), std::fixed with 6 / 9 decimals. append: 0 = new
 * file. */
int odo_write_tum_trajectory(const char* path, const double* timestamps, const float* Tcw, int n, int append);

/* Frame::ComputeImageBounds (frame.cpp:315-349) for the context's calibration
 * and image size: undistorted corners -> minX, maxX, minY, maxY. Host only. */
int odo_image_bounds(odo_ctx* ctx, float bounds[4]);

/* Tracking::SearchLocalLMs (tracking.cpp:368-405): Frame::isInFrustum
 * (frame.cpp:100-133) for every landmark neither ODO_LM_BAD nor ODO_LM_SEEN,
 * then Matcher(nn_ratio)::ProjectionMatch(frame, landmarks, th)
 * (matcher.cpp:90-145; the reference passes 0.8f and 8.0f). Frame: n
 * undistorted keypoints (mvKeysUn), their octaves and descriptors;
 * slot_taken[j] = slot j holds a landmark with Observations() > 0. Outputs:
 * slot_lm[j] = index of the landmark AddLandmark put in slot j, or -1;
 * proj[3*i..] = (mTrackProjX, mTrackProjY, mTrackProjXR) of in-view
 * landmarks, NaN otherwise; *n_matches = ProjectionMatch's return. Then
 * TrackLocalMap's second PnPSolver::Compute is odo_pnp_motion_ba over every
 * slot holding a landmark. */
int odo_projection_match(odo_ctx* ctx, const float Tcw[16], const odo_landmark* lms, int n_lms,
                         const float* kps_un, const int32_t* octave, const uint8_t* desc, int n,
                         const uint8_t* slot_taken, float th, float nn_ratio, int32_t* slot_lm, float* proj,
                         int* n_matches);

/* ---- Batched Tracking::TrackLocalMap (tracking.cpp:231-261, 368-405): the
 * local-map search and the second PnPSolver::Compute for every frame of the
 * LAST BATCH, the n frames odo_get_frame(ctx, i, ...) reads (after any
 * odo_track_batch* or odo_extract_batch). The frames are read where they sit
 * in HBM: keypoints, octaves, descriptors and right coordinates are not
 * uploaded. One launch chain for all frames, on odo_stream().
 *
 * Frame i, pose Tcw[i] (world -> camera, 4x4 row-major; typically
 * odo_chain_poses output), against the one shared landmark array lms:
 *   prior   prior_slot_lm[i * kp_cap + j] = k >= 0: slot j already holds
 *           lms[k] when TrackLocalMap starts (a map landmark KnnMatch carried
 *           over); -1 (or an index outside [0, n_lms)): empty; NULL: every
 *           slot empty. kp_cap must be odo_kp_capacity(ctx). A prior slot
 *           whose landmark is ODO_LM_BAD is released first (UpdateLocalKFs,
 *           tracking.cpp:270-276); every remaining prior landmark counts as
 *           ODO_LM_SEEN for that frame only (tracking.cpp:371-382, 388); the
 *           slot is taken iff its landmark has ODO_LM_HAS_OBS
 *           (matcher.cpp:114-117). A landmark may appear in at most one prior
 *           slot of a frame (not checked).
 *   search  Frame::isInFrustum and Matcher(nn_ratio)::ProjectionMatch(th)
 *           exactly as odo_projection_match defines them, landmarks in index
 *           order (the reference passes 0.8f and 8.0f).
 *   slots   slot j holds the landmark the search put there, else its
 *           surviving prior, else -1.
 *   PnP     PnPSolver::Compute (pnpsolver.cpp:17) over every slot holding a
 *           landmark, in slot order, from Tcw[i]: Xw = the landmark's X, the
 *           observation (kps_un[j], u_right[j]) (mono when u_right < 0),
 *           information 1 / Xw.z^2 with the world z (pnpsolver.cpp:74,111).
 *           Fewer than 3 edges: pnp_inliers = 0 and the pose as given.
 * No carry between frames (the batched contract): frame i's
 * refined pose does not feed frame i + 1 inside the call; every frame starts
 * from the pose the caller passes.
 *
 * The call synchronises the context, uploads landmarks, poses and priors in
 * one transfer, and returns with results[0 .. n) filled (one download); slots,
 * projections and masks stay in HBM for odo_get_local_map. n_lms == 0 is valid
 * (zeros and the input poses). Scratch is allocated by the first call (and
 * grown when a later call brings more landmarks); a context that never calls
 * this allocates and launches nothing for it.
 * ODO_ERR_STATE: no batch yet. ODO_ERR_ARG: NULL ctx / Tcw / results (or lms
 * with n_lms > 0), kp_cap != odo_kp_capacity(ctx), th negative or not finite,
 * n_lms < 0. ODO_ERR_CAPACITY: more than 65536 landmarks, or a keypoint
 * capacity above 8191 (13-bit keypoint index in a candidate). */
int odo_track_local_map(odo_ctx* ctx, const odo_landmark* lms, int n_lms, const float* Tcw,
                        const int32_t* prior_slot_lm, int kp_cap, float th, float nn_ratio,
                        odo_local_map_result* results);
/* Frame i of the last odo_track_local_map (ODO_ERR_STATE when the last batch
 * has none): slot_lm[j] for the frame's keypoints (up to cap; more keypoints
 * than cap: ODO_ERR_CAPACITY after copying cap), proj (optional): n_lms x 3
 * (mTrackProjX, mTrackProjY, mTrackProjXR), NaN for landmarks not in view;
 * pnp_outlier (optional, cap): 1 for a slot whose landmark the second PnP
 * flagged as an outlier. Synchronises. */
int odo_get_local_map(odo_ctx* ctx, int i, int32_t* slot_lm, float* proj, uint8_t* pnp_outlier, int cap);
/* Keypoint slots per frame of the context: the row length of prior_slot_lm. */
int odo_kp_capacity(odo_ctx* ctx);

/* ---- LocalBundleAdjustment::Compute (localbundleadjustment.cpp:65-315) on
 * the device: g2o OptimizationAlgorithmLevenberg over SE3Expmap pose vertices
 * and marginalised XYZ point vertices, BlockSolver_6_3 + LinearSolverEigen,
 * optimize(iters_robust) with the Huber kernel, the chi2 / depth
 * classification (:223-254), optimize(iters_final) on the level-0 edges
 * without it, and the erase list (:261-285). The caller does the graph walk
 * of :21-63 (map bookkeeping) and passes flat arrays:
 *   Tcw      n_kf x 16, world -> camera, row-major, in / out (:85, :302-307)
 *   kf_fixed n_kf: 1 = the vertex is fixed (lFixedCameras and keyframe id 0, :87, :99)
 *   Xw       n_lm x 3 world positions, in / out (:133, :310-315)
 *   edges    n_edges observations (kf, lm, u, v, ur), ur < 0 monocular; a
 *            landmark holds at most one edge per keyframe (GetObservations
 *            is a map keyed by keyframe, :139)
 *   edge_erase[e] = 1: the reference would EraseLandmark / EraseObservation
 *            this pair (:290-297)
 * Semantics (DESIGN.md §2 lists the pinned choices):
 *   vertices  poses are SE3Quat from the float matrix (Converter::toSE3Quat),
 *            points double from float; update T <- exp(dx) T, X <- X + dl
 *   edges    error = obs - project(T X), third row u - bf / z for stereo; the
 *            pose Jacobian of odo_pnp_motion_ba, the point Jacobian
 *            -(d proj / d Xc) R; information 1.0f / (z * z) in float from the
 *            landmark's INITIAL world z (:158, :185), the same for all its
 *            edges, never updated
 *   optimize lambda0 = 1e-5 max |diag H| over all active pose and point blocks
 *            at the start of each optimize(); lambda on every diagonal; scale
 *            = sum x (lambda x + b) + 1e-3; a trial is rejected when rho <= 0,
 *            its chi2 is not finite or the solve failed; at most 10 trials;
 *            stop when the trials reach 10 or rho == 0
 *   solve    Hll^-1 per 3 x 3 block, S = Hpp - sum W Hll^-1 W^T, LDL^T without
 *            pivoting failing iff a pivot is exactly zero (the step of a
 *            failed solve is zero), points by back-substitution
 *   flags    after stage 1 an edge with chi2 > chi2_mono / chi2_stereo or
 *            (T X).z <= 0 goes to level 1; the chi2 is the one g2o has stored,
 *            of the LAST TRIAL EVALUATED (also a rejected one); the depth
 *            test uses the current estimates; a level-1 edge keeps its chi2.
 *            A landmark or free pose without a level-0 edge leaves the system
 *            and keeps its estimate. edge_erase: the same test after stage 2.
 *   outputs  cast to float; a fixed keyframe, a free keyframe without an edge
 *            and a landmark without an edge come back bit for bit
 * GlobalBundleAdjustment (globalbundleadjustment.cpp:151-152) is the same call
 * with iters_final = 0, iters_robust = nIterations and its Huber deltas
 * sqrt(5.99) / sqrt(7.815) in the params.
 * Not supported: the abort flag (pbStopFlag, :76, :208-219).
 * Deviations: a non-finite pose, point or observation, a landmark whose
 * 1.0f / (z * z) is infinite (z == 0, or z * z underflows in float; infinite
 * information in the reference), an edge index out of range or a
 * repeated (kf, lm) pair give ODO_ERR_ARG without a launch, the caller's
 * arrays untouched. n_edges == 0 (or no free keyframe and no landmark with an
 * edge) is valid: status = ODO_BA_NOTHING, inputs unchanged, nothing launched.
 * ODO_ERR_CAPACITY: more than 64 free keyframes, 256 keyframes, 65536
 * landmarks or 2^20 edges. One upload and one download; between them only
 * three scalars per Levenberg trial reach the host. Scratch is allocated by
 * the first call and grown by later ones; a context that never calls this
 * allocates and launches nothing for it. Bit-identical run to run. The call
 * synchronises the context first (like odo_track_local_map) and returns with
 * the outputs written; the last batch's results stay readable.
 * ODO_ERR_ARG also for iters_robust < 1, iters_final < 0 or a threshold <= 0.
 * calib NULL: the context's; params NULL: odo_default_ba_params. */
void odo_default_ba_params(odo_ba_params* p);
int odo_local_ba(odo_ctx* ctx, float* Tcw, const uint8_t* kf_fixed, int n_kf, float* Xw, int n_lm,
                 const odo_ba_edge* edges, int n_edges, const odo_calib* calib, const odo_ba_params* params,
                 uint8_t* edge_erase, odo_ba_result* result);

/* ---- Matcher::Fuse's search (matcher.cpp:212-291) for every Fuse call of
 * LocalMapping::FuseLandmarks (localmapping.cpp:155-180) in one launch chain.
 * Call k is Fuse(pKF, list, th): kfs[k] names pKF's pose, its rows of the
 * keypoint arrays and its list, entries [lm_begin, lm_end) of lm_index, each
 * an index into lms (< 0 or >= n_lms: a null pointer). Per (call, list entry)
 * one odo_fuse_cand record, in call order then list order:
 *   projection  p3Dc = Rcw X + tcw as odo_projection_match computes it (double
 *           accumulation, one rounding); z < 0.0f: ODO_FUSE_BEHIND; invz =
 *           1 / z, x = X * invz, u = fx * x + cx (v alike), ur = u - mbf * invz,
 *           all float; outside odo_image_bounds (u >= minX && u < maxX && v >=
 *           minY && v < maxY fails, also for NaN): ODO_FUSE_OUTSIDE
 *   window  KeyFrame::GetFeaturesInArea: fabsf(kp.x - u) < th && fabsf(kp.y - v)
 *           < th (the reference passes 4.0f)
 *   gate    u_right[j] >= 0: e2 = (ex * ex + ey * ey) + er * er, dropped when
 *           e2 > 7.8f; otherwise e2 = ex * ex + ey * ey, dropped when e2 > 5.99f
 *           (ex = u - kp.x, ey = v - kp.y, er = ur - u_right[j])
 *   best    the smallest Hamming distance to lms[].desc over the gated
 *           keypoints, the lowest keypoint index among equals (Fuse's strict
 *           <); bestDist <= TH_LOW (50) is the caller's test
 *   cand    the 8 lowest gated keypoint indices and n_cand, their number
 * Only ODO_LM_BAD of lms[].flags is read. The search of one Fuse call is a
 * function of the map at the start of the call; across the calls of
 * FuseLandmarks' first loop only a landmark's descriptor changes (Replace's
 * ComputeDistinctiveDescriptors), never the gated set: the caller replays the
 * calls in order with its own map and re-scores a changed landmark's record
 * with odo_fuse_best (DESIGN.md §4 Fuse).
 * The call synchronises the context first (like odo_track_local_map), uploads
 * once and downloads once; the last batch's results stay readable. n_kf == 0,
 * n_index == 0 and empty ranges are valid. Scratch is allocated by the first
 * call and grown by later ones; a context that never calls this allocates and
 * launches nothing for it.
 * ODO_ERR_ARG: a null pointer with a non-zero size, a range outside its array
 * (or reversed), th negative or not finite; nothing is written.
 * ODO_ERR_CAPACITY: a keyframe with more than 8191 keypoints, more than 256
 * calls, more than 65536 landmarks, more than 2^20 records. */
int odo_fuse_search(odo_ctx* ctx, const odo_fuse_kf* kfs, int n_kf, const float* kps_un, const float* u_right,
                    const uint8_t* desc, int n_kp, const odo_landmark* lms, int n_lms, const int32_t* lm_index,
                    int n_index, float th, odo_fuse_cand* out);
/* Host only, no device: Fuse's (bestIdx, bestDist) of one record under
 * another descriptor. kf_*: the keyframe's own kf_n rows (kp_begin is row 0).
 * rec->n_cand <= ODO_FUSE_CANDS: over rec->cand; more: the keyframe is scanned
 * again with the window and the gate from rec->u, v, ur. A record that was
 * not searched or has no candidate gives (-1, INT32_MAX). ODO_ERR_ARG: a null
 * pointer, kf_n < 0, a candidate index >= kf_n, th negative or not finite. */
int odo_fuse_best(const odo_fuse_cand* rec, const float* kf_kps_un, const float* kf_u_right, const uint8_t* kf_desc,
                  int kf_n, float th, const uint8_t new_desc[32], int32_t* best_idx, int32_t* best_dist);

/* ---- Dense clouds: Frame::CreateCloud (frame.cpp:191-215), then
 * Frame::VoxelGridFilterCloud(leaf) (frame.cpp:217-226, pcl::VoxelGrid
 * <PointXYZRGB>), then pcl::transformPointCloud(cloud, Twc) (Tests/
 * Draw_map_pose.cpp:72-73, 99-103; Tests/GICP_test.cpp:66-67), for n frames
 * already in HBM (laid out as odo_track_batch's) in one launch chain. PCL is
 * restated, not linked (DESIGN.md §2 Dense clouds):
 *   CreateCloud  z = (float)d16 * depth_factor; pixel (row i, column j) kept
 *           iff z > 0, raster order; x = ((float)j - cx) * z * invfx, y =
 *           ((float)i - cy) * z * invfy (invfx the float 1.0f / fx), b, g, r
 *           from the frame, a = 255. No undistortion, as in the reference.
 *   leaf == 0  CreateCloud alone: ODO_CLOUD_UNFILTERED, every count 1.
 *   VoxelGrid  inv = 1.0f / leaf; min_p / max_p the exact per-axis min / max;
 *           d[a] = (int64)((max_p[a] - min_p[a]) * inv) + 1; d0 * d1 * d2 >
 *           INT32_MAX (or a product / floor outside the integer's range, which
 *           PCL leaves undefined): the input cloud, ODO_CLOUD_UNFILTERED. Else
 *           min_b = (int)floorf(min_p * inv), max_b alike, div_b = max_b - min_b
 *           + 1; per point ijk[a] = (int)(floorf(p[a] * inv) - (float)min_b[a]),
 *           key = ijk0 + ijk1 * div_b[0] + ijk2 * (div_b[0] * div_b[1]) in
 *           wrapping 32-bit arithmetic read as unsigned; one output point per
 *           distinct key, ascending.
 *   centroid  count points; b, g, r, a each (uint8)(uint32)((float)sum /
 *           (float)count) with the exact integer sum; x, y, z a float sum in a
 *           fixed order (bit-identical run to run) divided by (float)count.
 *   Twc     row-major 4 x 4 per frame (the inverse of the caller's Tcw), or
 *           NULL; applied to the result: x' = ((m00 * x + m01 * y) + m02 * z) +
 *           m03 in float, rows 1 and 2 alike; colours untouched.
 *   n_valid == 0  n_points 0, ODO_CLOUD_OK, the info's bounds zero (PCL is
 *           undefined on an empty cloud).
 * The call synchronises the context first (like odo_track_local_map), runs on
 * odo_stream() and returns with info[0..n) filled; the points stay in HBM,
 * compact, frame after frame. The last batch's results stay readable. Scratch
 * is allocated by the first call and grown by later ones; a context that
 * never calls this allocates and launches nothing for it.
 * ODO_ERR_ARG: a null pointer, n outside 1..max_batch, leaf negative or not
 * finite, a non-finite Twc entry; nothing is written. */
int odo_dense_clouds(odo_ctx* ctx, const uint8_t* d_bgr, const uint16_t* d_depth, int n, float leaf, const float* Twc,
                     odo_cloud_info* info);
/* The same from host frames (frame.cpp:191-226 on the caller's images): one
 * upload through the context's input staging, then odo_dense_clouds. */
int odo_dense_clouds_host(odo_ctx* ctx, const uint8_t* bgr, const uint16_t* depth, int n, float leaf, const float* Twc,
                          odo_cloud_info* info);
/* Frame i of the last dense-cloud call (KeyFrame's mpCloud, keyframe.cpp:46-47):
 * up to cap points into pts and, when counts is not NULL, each point's voxel
 * population into counts; *n is the cloud's point count. A cloud of more than
 * cap points: ODO_ERR_CAPACITY after the first cap were copied.
 * ODO_ERR_STATE before any dense-cloud call; ODO_ERR_ARG: i outside the last
 * call's frames, cap < 0, a null pts with cap > 0, a null n. */
int odo_get_dense_cloud(odo_ctx* ctx, int i, odo_cloud_point* pts, int32_t* counts, int cap, int* n);
/* GeneralizedICP(max_iterations, max_corr_dist)::Compute(pF1, pF2, guess)
 * (generalizedicp.cpp:41-53, 65-89; the reference runs it as GeneralizedICP(15,
 * 0.05) on VoxelGridFilterCloud(0.03f) clouds) for nprob pairs of frames of the
 * last dense-cloud call, read where they lie in HBM (x, y, z at the 16-byte
 * stride of odo_cloud_point): pairs[2p] = source frame, pairs[2p+1] = target
 * frame; guesses 16 per pair or NULL (identity). It registers whatever the
 * buffers hold: with Twc == NULL in odo_dense_clouds that is the reference's
 * camera-frame registration, with a Twc the clouds in the map frame. The grid
 * and the covariances are built once per distinct frame named in pairs, so a
 * chain (i - 1, i), (i, i + 1) pays for frame i once. Results as
 * odo_gicp_grid_batch on the same points, bit for bit (automatic cell); an
 * empty cloud or one under 20 points: converged 0, identity. Synchronises the
 * context first; its scratch is allocated by the first call and regrown when a
 * call needs more (a context that never calls it allocates nothing for it).
 * ODO_ERR_STATE before any dense-cloud call; ODO_ERR_ARG (nothing written):
 * nprob < 0, null pointers with nprob > 0, a frame outside the last
 * dense-cloud call, max_iterations < 1, max_corr_dist negative or not finite,
 * a non-finite guess entry; ODO_ERR_CAPACITY: more than 65535 pairs or frames
 * in the dense-cloud call, or 2^29 points over the distinct frames;
 * ODO_ERR_DEVICE: a named cloud holds a non-finite coordinate (odo_dense_clouds
 * with finite Twc produces none). nprob == 0 is valid. */
int odo_gicp_dense(odo_ctx* ctx, const int32_t* pairs, int nprob, const float* guesses, int max_iterations,
                   double max_corr_dist, float* T12, int32_t* converged, int32_t* iterations, int32_t* n_corr);
/* The same buffers where they lie in HBM (what odo_gicp_dense, the device-side
 * GeneralizedICP::Compute(pF1, pF2, guess), generalizedicp.cpp:41-53, reads),
 * valid until the next dense-cloud call or odo_destroy. d_counts may be
 * NULL. Errors as odo_get_dense_cloud. */
int odo_dense_cloud_device(odo_ctx* ctx, int i, const odo_cloud_point** d_pts, const int32_t** d_counts, int* n);

/* ---- StatisticalOutlierRemoval and GICP's fitness score ----
 * Frame::StatisticalOutlierRemovalFilterCloud(meanK, stddev) (frame.cpp:228-238,
 * pcl::StatisticalOutlierRemoval<PointXYZRGB>) and GeneralizedICP::mScore =
 * getFitnessScore() (generalizedicp.cpp:82) over the grids of odo_gicp_grid_*
 * (DESIGN §4 "SOR and fitness"). PCL is restated from its source as recalled,
 * not linked: parity with the library is unpinned.
 *   d2(p, q)  the float squared distance of the GICP searches: ((dx * dx + dy *
 *           dy) + dz * dz) with float differences, no fused operations.
 *   SOR, a cloud of n points, mean_k >= 1, stddev_mul finite:
 *     point i: the mean_k + 1 smallest d2(p_i, p_j) over all j (i included),
 *           ascending, the first dropped (PCL's nn_dists[0]); only distances
 *           enter, so no result depends on a tie rule or on the points' order;
 *           dist_sum = the double sum, in ascending order, of (double)sqrtf(d2)
 *           (a correctly rounded float root); distances[i] = (float)(dist_sum /
 *           (double)mean_k).
 *     cloud: sum += (double)distances[i]; sq_sum += (double)(distances[i] *
 *           distances[i]), the product in float; mean = sum / n; variance =
 *           (sq_sum - sum * sum / n) / (n - 1); stddev = sqrt(variance);
 *           threshold = mean + stddev_mul * stddev. PCL sums in index order,
 *           the device in a fixed order of its own (bit-identical run to run).
 *     point i is removed iff (double)distances[i] > threshold: a NaN threshold
 *           (negative computed variance) keeps every point, as in PCL. Kept
 *           points keep their order; colours and voxel counts travel with them.
 *     n <= mean_k (PCL reads past the end of its result vectors): the cloud is
 *           left as it is, ODO_SOR_SKIPPED, mean = stddev = threshold = 0.
 *     mean_k > 64: ODO_ERR_CAPACITY (PCL's default is 50).
 *   fitness, source S (ns points), target T, transform M (row-major 4 x 4):
 *           s' = M s as x' = ((m00 * x + m01 * y) + m02 * z) + m03 in float; nn_i
 *           = min_j d2(s'_i, t_j) over the WHOLE target (PCL's max_range is
 *           DBL_MAX: no distance cap, however far s' lies outside the target's
 *           grid); score = (sum of (double)nn_i in a fixed order) / ns. An empty
 *           source or target: DBL_MAX (PCL's nr == 0). The reference's 1e6 for
 *           "not converged" is the caller's (include/odo_frontend.hpp does it).
 *
 * odo_dense_sor filters every cloud of the last dense-cloud call where it lies
 * in HBM: the kept points and counts are packed frame after frame again and the
 * context's offsets follow, so odo_get_dense_cloud, odo_dense_cloud_device and
 * odo_gicp_dense then see the filtered clouds. It counts as a dense-cloud call:
 * device pointers handed out before it are no longer valid. A second call
 * filters the filtered clouds, as calling the reference's method twice would.
 * info: one record per frame of that call. Synchronises the context first.
 * ODO_ERR_STATE before any dense-cloud call; ODO_ERR_ARG (nothing changed): a
 * null pointer, mean_k < 1, stddev_mul not finite; ODO_ERR_CAPACITY: mean_k >
 * 64, more than 1048576 points in a cloud. */
int odo_dense_sor(odo_ctx* ctx, int mean_k, double stddev_mul, odo_sor_info* info);
/* The same for ncl host clouds (P packed x, y, z; offs ncl + 1 first rows, as
 * odo_gicp_grid_covariances): keep[i] = 1 for a point that stays, distances
 * (may be NULL) PCL's distances[] (zeros for a skipped cloud), info per cloud.
 * cell as odo_gicp_grid_batch: 0 = chosen per cloud from n and mean_k, > 0
 * forced (tests); no result depends on it. Capacity limits as
 * odo_gicp_grid_covariances. ODO_ERR_ARG (nothing written): null pointers with
 * non-zero sizes, offsets not starting at 0 or decreasing, mean_k < 1,
 * stddev_mul or cell not finite, cell < 0, a non-finite coordinate, ncl < 0. */
int odo_cloud_sor_batch(odo_ctx* ctx, const float* P, const int32_t* offs, int ncl, int mean_k, double stddev_mul,
                        float cell, uint8_t* keep, float* distances, odo_sor_info* info);
/* getFitnessScore of nprob (source, target, T) problems on host clouds laid out
 * as odo_gicp_grid_batch's; T 16 floats per pair. score: one double per pair.
 * nn_d2 (may be NULL, for tests): nn_i of every source point, pair after pair
 * (zeros for a pair with an empty target). cell: 0 = chosen per cloud, > 0
 * forced. Limits and errors as odo_gicp_grid_batch; a non-finite T entry is
 * ODO_ERR_ARG. */
int odo_gicp_grid_fitness(odo_ctx* ctx, const float* src, const int32_t* soffs, const float* tgt,
                          const int32_t* toffs, const float* T, int nprob, float cell, double* score, float* nn_d2);
/* The same for pairs of frames of the last dense-cloud call (pairs as
 * odo_gicp_dense, T 16 floats per pair: the registration's result), on the
 * clouds where they lie in HBM; one grid per distinct frame named. Equals
 * odo_gicp_grid_fitness on the same points bit for bit. Errors as
 * odo_gicp_dense. */
int odo_gicp_dense_fitness(odo_ctx* ctx, const int32_t* pairs, int nprob, const float* T, double* score);

/* ---- Point-to-plane ICP: libicp's IcpPointToPlane, batched ----
 * Odometry/icp/ (icp.cpp, icpPointToPlane.cpp, matrix.cpp), dimension 3, as
 * Tests/IcpPointToPlane.cpp:81-119 runs it on RANSAC's inlier clouds, over the
 * grids of odo_gicp_grid_* (DESIGN §4 "Point-to-plane ICP"). The model is the
 * target (the cloud with the normals), the template is moved: model = R *
 * template + t. R, t are floats between iterations (matrix.h's FLOAT).
 *   normals   of model point i: its num_neighbors nearest model points, itself
 *           included, ascending by (d2, index) with d2 the float squared
 *           distance of the GICP searches; all of them when the model has fewer;
 *           mu (running float sums in that order, / (float)k), Q = P - mu, H = Q^T
 *           Q (running float sums in that order); the eigenvector of H's
 *           smallest eigenvalue from a double Jacobi SVD of (double)H, rounded
 *           to float, then Matrix::svd's sign rule (matrix.cpp:853-867), which for
 *           a symmetric H reads: negated when two or three components are
 *           negative. An exactly zero smallest singular value (an exact plane)
 *           is signed the same way.
 *   loop      delta = 1000; while (iterations < max_iterations && delta >
 *           min_delta): with indist > 0 first indist = max(indist * 0.9, 0.05)
 *           and the active set = getInliers, else every point is active; delta
 *           = fitStep.
 *   search    s = R * T + t in double from the floats; the query is (float)s; its
 *           nearest model point d by (d2, index), equal distances to the lower
 *           model index (the reference's kd-tree order is unknown), no distance
 *           cap; one search per iteration serves getInliers and fitStep.
 *   gate      ODO_ICP_GATE_AS_WRITTEN: abs((sx - dx) * nx + (sy - dy) * ny + (sz -
 *           dz)) * nz < indist, the reference's expression (a matched normal
 *           with nz <= 0 is always active); ODO_ICP_GATE_PLANE: abs(n . (s - d))
 *           < indist. s is the unrounded double here.
 *   fitStep   per active point, s the float query read back: the row [nz * sy -
 *           ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz] and b = n
 *           . d - n . s in double, stored as floats. A^T A and A^T b are summed in
 *           double in a fixed order of the device's own (bit-identical run to
 *           run, independent of the other pairs of the call) and rounded to
 *           float once; the reference's running float sums differ within the
 *           tolerance DESIGN §4 records. Then on floats in the reference's
 *           order: Gauss-Jordan with full pivoting (a pivot below 1e-20 fails:
 *           delta = 0, R and t unchanged, ODO_ICP_SINGULAR), R_ = the orthogonal
 *           polar factor of I + [x0 x1 x2]x, R = R_ * R, t = R_ * t + t_, delta =
 *           max(|R_ - I|_F, |t_|).
 *   residual  over the last active set at the final R, t, a fresh search each:
 *           the signed mean of n . (d - s), s unrounded; 0 for an empty set.
 *           max_iterations == 0 with indist > 0 (libicp would read a stale
 *           set): the set is empty.
 * Fewer than 5 model points: ODO_ICP_NO_MODEL; else fewer than 5 template
 * points: ODO_ICP_SHORT_TEMPLATE; both leave T = the guess, 0 iterations,
 * residual 0.
 *
 * odo_icp_normals: the normals alone of ncl host clouds (P packed x, y, z; offs
 * ncl + 1 first rows), 3 floats per point; zeros for a cloud under 5 points.
 * odo_icp_plane_batch: nprob problems, template p = rows toffs[p] .. toffs[p +
 * 1] of tmpl, model p = rows moffs[p] .. of model; guesses 16 floats per
 * problem (row-major 4 x 4, the rotation block taken as given) or NULL for
 * identity.
 * cell: 0 = chosen per cloud by the library, > 0 forced (tests); no result
 * depends on it. Limits as odo_gicp_grid_batch / odo_gicp_grid_covariances
 * (ODO_ERR_CAPACITY), and num_neighbors > 32. ODO_ERR_ARG (nothing written):
 * null pointers with non-zero sizes, offsets not starting at 0 or decreasing,
 * a non-finite coordinate, guess entry, min_delta or indist, cell negative or
 * not finite, num_neighbors < 3, max_iterations < 0, a gate other than 0 / 1,
 * a negative count. nprob == 0 (ncl == 0) is valid. Scratch comes from the
 * context's grow-only blocks at the first call. */
void odo_default_icp_params(odo_icp_params* p);
int odo_icp_normals(odo_ctx* ctx, const float* P, const int32_t* offs, int ncl, int num_neighbors, float cell,
                    float* normals);
int odo_icp_plane_batch(odo_ctx* ctx, const float* tmpl, const int32_t* toffs, const float* model,
                        const int32_t* moffs, const float* guesses, int nprob, const odo_icp_params* params,
                        float cell, odo_icp_result* out);
/* The same for pairs of frames of the last dense-cloud call, on the clouds
 * where they lie in HBM: pairs[2p] = the template (source frame), pairs[2p + 1]
 * = the model. The grid and the normals are built once per distinct model
 * frame. Results equal odo_icp_plane_batch on the same points bit for bit.
 * States and errors as odo_gicp_dense (ODO_ERR_STATE before any dense-cloud
 * call, ODO_ERR_DEVICE for a non-finite coordinate in a named cloud), the
 * parameters as above. */
int odo_icp_plane_dense(odo_ctx* ctx, const int32_t* pairs, int nprob, const float* guesses,
                        const odo_icp_params* params, odo_icp_result* out);

/* Kabsch::Compute (kabsch.cpp:14): one GPU workgroup (k_kabsch: centroids, A^T B
 * with a fixed-order block reduction, 3x3 Jacobi SVD). A,B: n x 3 host arrays.
 * R = W diag(1, 1, sgn(det V det W)) V^T is a rotation for every input (the
 * reference's sgn det M can give a reflection for rank-deficient sets); for
 * collinear or identical points its turn about the line is not determined by
 * the data. n = 0 returns the identity. */
int odo_kabsch(const float* A, const float* B, int n, float T[16]);

/* glibc rand() stream helpers (srand/rand of main.cpp:27, ransac.cpp:275). */
void odo_rng_seed(odo_rng* r, uint32_t seed);
int32_t odo_rng_next(odo_rng* r);

/* ---- Introspection for parity tests ---- */
int odo_debug_pyramid(odo_ctx* ctx, int i, uint8_t* out, size_t cap);
int odo_debug_fast(odo_ctx* ctx, int i, int level, orb_kp* out, int cap, int* n);
int odo_debug_octree(odo_ctx* ctx, int i, int level, orb_kp* out, int cap, int* n);
int odo_debug_blur(odo_ctx* ctx, int i, uint8_t* out, size_t cap);
/* std::sort(vGoodMatches) of Ransac::Iterate (ransac.cpp:199) as the pair
 * stage runs it on the GPU (workgroup-parallel introsort): in -> out sorted by
 * distance in libstdc++'s exact (unstable) order; distances must be >= 0. */
int odo_debug_sort(odo_ctx* ctx, const odo_dmatch* in, int n, odo_dmatch* out);

/* The pair-match stage on caller-supplied features: the batch path's own
 * launches with its own arguments (VO landmarks and query list, kNN-2 in the
 * context's form and split count, k_pair_match, the DepthCovariance latch) on
 * n host frames, without extraction, RANSAC or the pose stage.
 * counts[n]; desc [n][kp_cap][32] and xyz [n][kp_cap][3] with kp_cap =
 * odo_kp_capacity(ctx), of which the first counts[i] rows of frame i are read.
 * Frame i is placed in slot i of the frame set the next batch would use
 * (frame 0 where the roll puts the previous frame, the others where
 * extraction puts a batch's frames), so pair p is (frame p, frame p + 1):
 * n - 1 pairs, every one valid; 2 <= n <= max_batch + 1. Configuration is the
 * context's (nn_ratio, ransac.check_depth, ransac.min_inlier_th, calib for
 * mThDepth, forms.knn, forms.knn_split); the latch is read as odo_set_latch
 * left it, and *latch is its value after the batch. Every output array holds
 * n - 1 rows of kp_cap entries (qcnt, n_matches, n_good: n - 1 entries); only
 * the entries named are written:
 *   lm_flags   counts[p] flags of frame p's VO landmarks
 *   qlist      qcnt[p] landmark keypoint indices, ascending
 *   knn_idx/knn_dist  [kp_cap][2], the rows of landmark queries only: the
 *              train splits' lists merged (-1 / INT_MAX when absent)
 *   matches    n_matches[p] KnnMatch results in query order
 *   good       n_good[p] good matches in std::sort's order
 *   f2_src     counts[p + 1] entries: the frame-p keypoint whose landmark
 *              sits in this frame-(p + 1) slot, or -1
 * A null pointer or a negative count is ODO_ERR_ARG and a count above kp_cap
 * ODO_ERR_CAPACITY, both before anything else is read or written. The call
 * synchronises and ends with odo_reset: a later odo_track_batch* behaves as
 * it does after odo_reset (no previous frame, latch unset, pair counter 0). */
typedef struct odo_pair_stage_out {
    uint8_t* lm_flags;
    int32_t *qlist, *qcnt, *knn_idx, *knn_dist;
    odo_dmatch* matches;
    int32_t* n_matches;
    odo_dmatch* good;
    int32_t *n_good, *f2_src;
    double* latch;
} odo_pair_stage_out;
int odo_debug_match_features(odo_ctx* ctx, int n, const int32_t* counts, const uint8_t* desc, const float* xyz,
                             const odo_pair_stage_out* out);

/* Measurement only (no reference counterpart): re-runs the most recent
 * batch's kNN-2 launch `reps` times on an idle device and returns its mean
 * duration in ms (HIP events). The bench's roofline "alone" figure. */
int odo_knn_replay_time(odo_ctx* ctx, int reps, float* avg_ms);
/* ADAPTIVE detector state. The per-cell DetectorAdjuster thresholds persist
 * across frames and calls (detectoradjuster.cpp:52-65, App. B.13); they
 * advance with every extracted frame, in frame order within a batch.
 * odo_debug_adaptive: FAST threshold each cell used for frame i of the last
 * batch (t_used, grid cells; NULL skips) and the current thresholds (thresh;
 * NULL skips). Returns the number of grid cells (< 0 on error). */
int odo_debug_adaptive(odo_ctx* ctx, int i, int32_t* t_used, double* thresh);
int odo_set_adaptive_thresholds(odo_ctx* ctx, const double* thresh, int n);
/* std::nth_element(a, a + nth, a + n) by score (mode 0; keepStrongest,
 * videogridadaptedfeaturedetector.cpp:24-31) or KeyPointsFilter::retainBest
 * (mode 1) exactly as the ADAPTIVE stages run them on the GPU, over packed
 * keys (score << 24 | y << 12 | x). out: n keys, *n_out kept. */
int odo_debug_select(odo_ctx* ctx, const uint32_t* in, int n, int nth, int mode, uint32_t* out, int* n_out);
/* Timing (off by default; mode 0). Mode 1: odo_track_batch records HIP events
 * between stages and odo_last_timings reports the last batch (ms); these
 * events serialise the streams they sit on. Mode 2: an event pair brackets the
 * Hamming-match (kNN-2) launch of every batch on the extraction stream, and
 * odo_kernel_timing reports the mean launch duration since the mode was set. */
int odo_set_timing(odo_ctx* ctx, int mode);
int odo_kernel_timing(odo_ctx* ctx, double* avg_ms, long* launches);
/* Measurement only (mode 2): the start of every batch's kNN-2 launch since the
 * mode was set, in ms after odo_set_timing, batch order. A batch's kNN-2 starts
 * when its extraction has finished, so consecutive differences are the
 * pipeline's per-step times. Copies up to cap marks; returns how many exist. */
int odo_step_marks(odo_ctx* ctx, double* ms, int cap);
/* Per-stage device time of the last odo_track_batch (ms), via HIP events. */
int odo_last_timings(odo_ctx* ctx, float* ms, int cap, const char** names);

#ifdef __cplusplus
}
#endif

#endif /* ODO_H */
