/*
 * odo_types.h — plain-old-data types crossing the C-ABI of the MI355X
 * odometry hot path. Layouts mirror the OpenCV / reference types they
 * replace so a caller can memcpy between them.
 *
 *   orb_kp      <-> cv::KeyPoint  {pt.x, pt.y, size, angle, response, octave, class_id}
 *                   (produced by ORBextractor::operator(), Features/orbextractor.cpp:756)
 *   odo_dmatch  <-> cv::DMatch    {queryIdx, trainIdx, imgIdx, distance}
 *                   (Matcher::KnnMatch, Features/matcher.cpp:55)
 *   odo_calib   <-> Calibration namespace constants, Utils/common.h:32-74
 */
#ifndef ODO_TYPES_H
#define ODO_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orb_kp {
    float x, y;       /* pt (level-0 pixel coordinates after scaling, orbextractor.cpp:805-811) */
    float size;       /* PATCH_SIZE * scale, int-truncated (orbextractor.cpp:731) */
    float angle;      /* IC angle in degrees [0,360) (orbextractor.cpp:14-39) */
    float response;   /* FAST score (cornerScore<16>) */
    int32_t octave;   /* pyramid level */
    int32_t class_id; /* always -1 */
} orb_kp;

typedef struct odo_dmatch {
    int32_t queryIdx;
    int32_t trainIdx;
    int32_t imgIdx;
    float distance;
} odo_dmatch;

typedef struct odo_calib {
    float fx, fy, cx, cy;      /* common.h:35-38 (FR1 active) */
    float k1, k2, p1, p2, k3;  /* common.h:40-44; k1 == 0 disables undistortion (frame.cpp:288) */
    float depth_factor;        /* common.h:67, 1/5000 */
    float mbf;                 /* common.h:71, 40 */
    float th_depth;            /* common.h:72, 40 (mThDepth = mbf*thDepth/fx) */
} odo_calib;

typedef struct odo_orb_params {
    int32_t nfeatures;    /* ORBextractor(nFeatures=1000,...) extractor.cpp:86 */
    float scale_factor;   /* 1.2 */
    int32_t nlevels;      /* 8 */
    int32_t ini_th_fast;  /* 20 */
    int32_t min_th_fast;  /* 7 */
} odo_orb_params;

typedef struct odo_ransac_params {
    int32_t iterations;        /* Ransac(200,...) odometry.cpp:28 */
    int32_t min_inlier_th;     /* 20 */
    float max_mahalanobis;     /* 3.0 */
    int32_t sample_size;       /* 4 */
    int32_t check_depth;       /* mCheckDepth, true (ransac.cpp:20) */
} odo_ransac_params;

/* Grid-adapted detector (Extractor::ADAPTIVE with FAST inner detector),
 * extractor.cpp:52-77: DetectorAdjuster(FAST, 20, 2, 10000, 1.3, 0.7),
 * VideoDynamicAdaptedFeatureDetector(gridMin=67, gridMax=113, iters=5),
 * VideoGridAdaptedFeatureDetector(maxTotal=1020, 3x3, edge=31), then
 * retainBest(nFeatures=1000) and cv::ORB::compute (extractor.cpp:39-50). */
typedef struct odo_adaptive_params {
    int32_t grid_rows, grid_cols;
    int32_t edge_threshold;
    int32_t max_total_keypoints;
    int32_t cell_min, cell_max;
    int32_t escape_iters;
    double init_thresh, min_thresh, max_thresh;
    double increase_factor, decrease_factor;
    int32_t retain_best;       /* Extract: retainBest(nFeatures) extractor.cpp:45-46 */
} odo_adaptive_params;

/* glibc TYPE_3 additive-feedback generator state (random_r), the
 * process-global rand() stream used by Ransac::SampleMatches
 * (ransac.cpp:275-276) made explicit. */
typedef struct odo_rng {
    int32_t state[31];
    int32_t fpos;   /* index of fptr into state */
    int32_t rpos;   /* index of rptr into state */
} odo_rng;

/* Hypotheses mode: one evaluated RANSAC hypothesis (the
 * visited iteration of that index: its sample, refinement loop and refined
 * transform, ransac.cpp:201-231). cnt = |refined inliers| (0 = no valid
 * refinement); err = refinedError; T = refined T12 rows 0..2. 64 bytes. */
typedef struct odo_hyp_summary {
    double err;
    int32_t cnt;
    int32_t pad;
    float T[12];
} odo_hyp_summary;

/* Outcome of Ransac::Iterate's ordered running-best fold over all
 * hypotheses (ransac.cpp:233-249): best_h = index of the accepted hypothesis
 * (-1: none), visited = iterations run, valid = validIters. */
typedef struct odo_ransac_fold_result {
    int32_t best_h, visited, valid, n_inliers;
    float rmse;
    int32_t n_good;
    int32_t pad[2];
} odo_ransac_fold_result;

/* Result of PnPRansac::Compute's cv::solvePnPRansac (pnpransac.cpp:34-50):
 * (rvec, tvec) refined by solvePnP(ITERATIVE) on the RANSAC inliers, the best
 * RANSAC model, T = Converter::toHomogeneous(r, t) (row-major float), bOK,
 * inliers.rows, the index of the winning hypothesis and the RANSAC
 * iterations run (niters after RANSACUpdateNumIters). 176 bytes. */
typedef struct odo_pnp_ransac_result {
    double rvec[3], tvec[3];
    double model_rvec[3], model_tvec[3];
    float Tcw[16];
    int32_t ok, n_inliers, best_iter, iterations_visited;
} odo_pnp_ransac_result;

/* One local-map landmark for Matcher::ProjectionMatch (matcher.cpp:90-145):
 * world position (Landmark::GetWorldPos), distinctive descriptor
 * (GetDescriptor) and state flags. 48 bytes. */
#define ODO_LM_BAD 1       /* Landmark::isBad() */
#define ODO_LM_SEEN 2      /* mnLastFrameSeen == current frame (already matched; SearchLocalLMs skips it) */
#define ODO_LM_HAS_OBS 4   /* Observations() > 0 (a slot holding it is skipped by later landmarks) */
typedef struct odo_landmark {
    float X[3];
    int32_t flags;
    uint8_t desc[32];
} odo_landmark;

/* Per-frame-pair odometry result. */
typedef struct odo_pair_result {
    float T12[16];        /* RANSAC transform F1->F2 (row-major 4x4) */
    float Tcw[16];        /* PnP-refined pose of F2 (row-major 4x4) */
    float rmse;           /* Ransac::rmse */
    int32_t n_matches;    /* KnnMatch result size */
    int32_t n_good;       /* depth-valid matches entering RANSAC */
    int32_t n_inliers;    /* |Ransac::mvInliers| */
    int32_t ransac_ok;    /* Ransac::Iterate return */
    int32_t pnp_inliers;  /* PnPSolver::Compute return */
    int32_t visited;      /* RANSAC iterations actually run (realIters) */
    int32_t n_queries;    /* kNN-2 queries: F1 keypoints holding a VO landmark (the only ones KnnMatch keeps) */
    int32_t n_sweeps;     /* ComputeInliersAndError calls in the visited iterations (+1 for the identity
                             fallback): the RANSAC work E of SURVEY §8(d) is n_sweeps * n_good evaluations */
    int32_t n_fit_points; /* points added to TransformationFromCorrespondences fits (F of SURVEY §8(d)) */
} odo_pair_result;

/* The constants of Odometry::Compute's ADAPTIVE_RICP branch rule and of its
 * GeneralizedICP (odometry.cpp:15, 52-53) made explicit; odo_set_odometry. */
typedef struct odo_ricp_params {
    int32_t min_inliers;        /* 20   : mvInliers.size() < 20                     */
    float   rmse_scale;         /* 10.f : rmse * 10.0f                              */
    float   refine_at;          /* 7.f  : >= -> GICP                                */
    float   reset_at;           /* 20.f : >= -> GICP from identity, else from mT12  */
    int32_t gicp_iterations;    /* 10   : GeneralizedICP(10, 0.07)                  */
    double  gicp_max_corr_dist; /* 0.07                                             */
} odo_ricp_params;

/* What ADAPTIVE_RICP did for one pair of the last batch (odo_get_ricp). 96 bytes. */
typedef struct odo_ricp_result {
    float   T12[16];     /* GeneralizedICP::mT12 when GICP ran for the pair, identity otherwise */
    int32_t branch;      /* 0 keep RANSAC's mT12, 1 GICP from identity, 2 GICP from mT12 */
    int32_t converged, iterations, n_corr;   /* as odo_gicp; 0 when GICP did not run */
    int32_t n_cloud;     /* points in mpSourceCloud (= mpTargetCloud) */
    int32_t pad[3];
} odo_ricp_result;

/* Tracking::TrackLocalMap for one frame of the last batch (odo_track_local_map).
 * 96 bytes. */
typedef struct odo_local_map_result {
    float   Tcw[16];        /* pose after the second PnPSolver::Compute (the input pose when it does not run) */
    int32_t n_in_view;      /* landmarks isInFrustum accepted (nToMatch, tracking.cpp:394-397) */
    int32_t n_matches;      /* ProjectionMatch's return (0 when n_in_view == 0: it is not called) */
    int32_t n_edges;        /* slots holding a landmark when PnP starts */
    int32_t pnp_inliers;    /* PnPSolver::Compute's return */
    int32_t n_map_inliers;  /* inlier slots whose landmark has ODO_LM_HAS_OBS (TrackLocalMap's nInliers,
                               tracking.cpp:247-255) */
    int32_t pad[3];         /* pad[0]: diagnostic, the rounds the slot resolver ran for the frame; the rest 0 */
} odo_local_map_result;

/* One reprojection edge of odo_local_ba: keyframe kf observes landmark lm at
 * the undistorted keypoint (u, v) with right coordinate ur; ur < 0: a
 * monocular observation (localbundleadjustment.cpp:149). 20 bytes. */
typedef struct odo_ba_edge {
    int32_t kf, lm;
    float   u, v, ur;
} odo_ba_edge;

/* The constants of LocalBundleAdjustment::Compute made explicit
 * (odo_default_ba_params: localbundleadjustment.cpp:126-127, 213, 230, 244, 254). */
typedef struct odo_ba_params {
    int32_t iters_robust;   /* 5   first optimize(), Huber on                                        */
    int32_t iters_final;    /* 10  second optimize() on level-0 edges, Huber off; 0 = skip stage 2  */
    int32_t robust;         /* 1   Huber in stage 1                                                  */
    float   huber_mono, huber_stereo;   /* sqrtf(5.991), sqrtf(7.815) as floats                      */
    float   chi2_mono, chi2_stereo;     /* 5.991, 7.815                                              */
} odo_ba_params;

/* What odo_local_ba did. 64 bytes. */
#define ODO_BA_RAN 0       /* the optimiser ran */
#define ODO_BA_NOTHING 1   /* nothing to optimise: the inputs came back, nothing was launched */
typedef struct odo_ba_result {
    double  chi2_initial;   /* robust chi2 before the first iteration                  */
    double  chi2_stage1;    /* after the first optimize()                              */
    double  chi2_final;     /* after the second (= chi2_stage1 when it did not run)    */
    int32_t iters1, iters2;     /* iterations each optimize() ran                      */
    int32_t trials1, trials2;   /* Levenberg trials (linear solves) of each            */
    int32_t n_erase;        /* edges flagged in edge_erase                             */
    int32_t n_level1;       /* edges set aside after stage 1                           */
    int32_t status;         /* ODO_BA_*                                                */
    int32_t pad;
} odo_ba_result;

/* One Matcher::Fuse(pKF, vpLandmarks, th) call of odo_fuse_search
 * (matcher.cpp:212-313). 80 bytes. */
typedef struct odo_fuse_kf {
    float   Tcw[16];            /* pKF's pose, world -> camera, row-major */
    int32_t kp_begin, kp_end;   /* pKF's keypoints: rows [kp_begin, kp_end) of kps_un / u_right / desc */
    int32_t lm_begin, lm_end;   /* its list: entries [lm_begin, lm_end) of lm_index (ranges may repeat or overlap) */
} odo_fuse_kf;

#define ODO_FUSE_CANDS 8
/* n_cand < 0: the landmark was not searched */
#define ODO_FUSE_NULL    (-1)  /* lm_index entry < 0 or >= n_lms (a null pointer in vpLandmarks, matcher.cpp:223) */
#define ODO_FUSE_BAD     (-2)  /* ODO_LM_BAD (matcher.cpp:225; IsInKeyFrame is the caller's, at replay) */
#define ODO_FUSE_BEHIND  (-3)  /* p3Dc.z < 0.0f (matcher.cpp:231) */
#define ODO_FUSE_OUTSIDE (-4)  /* !IsInImage(u, v) (matcher.cpp:241, keyframe.cpp:424-427) */

/* The search of one (call, list entry) pair, in call order then list order.
 * 40 bytes. */
typedef struct odo_fuse_cand {
    float    u, v, ur;              /* the projection (matcher.cpp:238-244); NaN when n_cand < 0 */
    int32_t  n_cand;                /* keypoints inside the window that passed the gate (all of them), or ODO_FUSE_* */
    int32_t  best_idx;              /* Fuse's bestIdx under lms[].desc: first minimum in keypoint order; -1: none */
    int32_t  best_dist;             /* its Hamming distance; INT32_MAX: none */
    uint16_t cand[ODO_FUSE_CANDS];  /* the first min(n_cand, 8) candidates, ascending keypoint index (relative to
                                       kp_begin); unused entries 0xffff */
} odo_fuse_cand;

/* One point of a dense cloud (odo_dense_clouds): pcl::PointXYZRGB's payload,
 * camera frame (or the frame Twc maps to). 16 bytes. */
typedef struct odo_cloud_point {
    float   x, y, z;
    uint8_t b, g, r, a;         /* a = 255 for a CreateCloud point (PCL's default), the voxel's mean like b, g, r */
} odo_cloud_point;

#define ODO_CLOUD_OK         0  /* the voxel grid filter ran (or the cloud is empty) */
#define ODO_CLOUD_UNFILTERED 1  /* leaf == 0, or VoxelGrid's "leaf size is too small" return: CreateCloud's points */

/* One frame of odo_dense_clouds. 60 bytes. */
typedef struct odo_cloud_info {
    int32_t status;             /* ODO_CLOUD_* */
    int32_t n_valid;            /* CreateCloud's points: pixels with z > 0 */
    int32_t n_points;           /* points of the result */
    int32_t min_b[3], div_b[3]; /* VoxelGrid's min_b_ / div_b_ (zero when unfiltered or empty) */
    float   min_p[3], max_p[3]; /* getMinMax3D of CreateCloud's points, before Twc (zero when empty) */
} odo_cloud_info;

#define ODO_SOR_OK      0  /* the filter ran */
#define ODO_SOR_SKIPPED 1  /* n_in <= mean_k (the empty cloud too): the cloud is left as it is */

/* One cloud of odo_dense_sor / odo_cloud_sor_batch. 40 bytes. */
typedef struct odo_sor_info {
    int32_t status;             /* ODO_SOR_* */
    int32_t n_in, n_out;        /* points before and after */
    int32_t pad;
    double  mean, stddev, threshold;  /* of distances[]; zero when skipped; stddev and threshold NaN when the
                                         computed variance is negative (every point is then kept) */
} odo_sor_info;

/* libicp's IcpPointToPlane (odo_icp_plane_batch, odo_icp_plane_dense). */
#define ODO_ICP_GATE_AS_WRITTEN 0  /* getInliers as the reference has it (icpPointToPlane.cpp:299) */
#define ODO_ICP_GATE_PLANE      1  /* abs(n . (s - d)) < indist, the distance it meant */

#define ODO_ICP_OK             0
#define ODO_ICP_NO_MODEL       1  /* fewer than 5 model points: T is the guess */
#define ODO_ICP_SHORT_TEMPLATE 2  /* fewer than 5 template points: T is the guess */
#define ODO_ICP_SINGULAR       3  /* the last step's solve failed (a pivot below 1e-20): that step left R, t alone */

/* 32 bytes. odo_default_icp_params: 10, 200, AS_WRITTEN, 1e-4, -1 (libicp's defaults). */
typedef struct odo_icp_params {
    int32_t num_neighbors;   /* computeNormals' neighbours, the point itself included: 3 .. 32 */
    int32_t max_iterations;  /* setMaxIterations, >= 0 */
    int32_t gate;            /* ODO_ICP_GATE_* */
    int32_t pad;
    double  min_delta;       /* setMinDeltaParam */
    double  indist;          /* fit's indist: <= 0 every point is active */
} odo_icp_params;

/* One pair. 88 bytes. */
typedef struct odo_icp_result {
    float   T[16];       /* row-major 4 x 4 of the final R, t: model = R * template + t (icp.h:41) */
    double  residual;    /* fit's return value: getResidual over the last active set */
    float   delta;       /* the last step's max(|R_ - I|_F, |t_|); 1000 before any step, 0 after a failed solve */
    int32_t iterations;  /* steps run */
    int32_t n_active;    /* the last active set's size (getInlierCount) */
    int32_t status;      /* ODO_ICP_* */
} odo_icp_result;

#ifdef __cplusplus
}
#endif

#endif /* ODO_TYPES_H */
