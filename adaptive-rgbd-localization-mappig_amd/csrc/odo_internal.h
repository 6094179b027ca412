// Internal (non-ABI) structures shared by the HIP kernels and the host
// orchestration (odo_*.cpp, whose own shared header is odo_ctx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/odo_types.h"

namespace odo {

// Measurement / A-B knobs (serial streams, stage skipping, grid sizes, the
// choice among the kernel forms that ship). Only the tuning build (make tuning: -DODO_TUNING,
// build_tuning/libodo_hip.so, selected with ODO_LIB) reads them from the
// environment; the production library ignores the environment entirely, so a
// stray variable cannot change (or invalidate) a production context.
static inline const char* odo_knob(const char* name) {
#ifdef ODO_TUNING
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// The one carver: a block cut into 256-byte aligned sections. add() returns
// the section's offset; off is then the size of the block so far.
struct Pack {
    size_t off = 0;
    size_t add(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
};

#define FAST_ROI_MAX 72 // largest FAST cell ROI side (a level narrower than 2 cells: up to 65)

// One pyramid level of one frame (all frames share the geometry).
struct LevelDesc {
    int off;          // byte offset of the level inside a frame's pyramid buffer
    int w, h;
    int pitch;        // row stride in bytes (w rounded up to 16)
    float scale;      // mvScaleFactor[level] (float, orbextractor.cpp:358)
    int quota;        // mnFeaturesPerLevel[level]
    int cell_begin;   // range in the global cell table
    int cell_end;
    int key_off;      // offset of this level's key scratch inside a frame's key buffer
};

// One FAST cell ROI (orbextractor.cpp:688-711).
struct CellDesc {
    int16_t level;
    int16_t rows, cols;
    int16_t x0, y0;   // ROI origin in level pixels
    int16_t offx, offy;  // j*wCell, i*hCell (added to ROI coords, relative to the 16px border)
    int16_t pad;
};

// A FAST segment (k_fast_seg): cells [ja, ja + ncell) of one cell row of one
// level, whose ROIs (orbextractor.cpp:688-703) are staged in LDS as one union:
// rows [y0, y0 + rows), cols [x0, x0 + cols) of the level; cell jl of the
// segment is cells_h[ci0 + jl] (ROI x0 + jl*wcell).
#ifndef FS_SEGC
#define FS_SEGC 8  // cells per segment (at most; the host splits a cell row evenly)
#endif
#define FS_NCM FS_SEGC
// LDS row stride of a staged segment (bytes): a compile-time constant, so the
// kernel's neighbour offsets (the 16 circle pixels, the compass points, the
// NMS neighbours) are instruction immediates; the host sizes segments to fit
// it. 272 = 68 dwords, a 16-byte multiple (the staging stores) that moves each
// row 4 banks over: with 256 every row of a column fell in the same bank, and
// the segment test's scattered circle reads of candidates from different rows
// conflicted (profiles/r05_rs)
#ifndef FS_RS
#define FS_RS 272
#endif
struct FastSeg {
    int level, ci0;
    int16_t y0, x0, rows, cols, ncell, wcell;
    int16_t bw;  // kept-bitmap words per row
    // per-segment constants the kernel would otherwise divide for
    // (fast_seg_staging). The staging loop's thread grid: nw 16-byte columns
    // per staged row, rstep = FS_TH / nw rows per step, and rmag =
    // ceil(4096 / nw), with which t / nw = (t * rmag) >> 12 for every
    // t < FS_TH (nw <= 17: the error term t * 16 stays below 4096)
    int16_t nw, rstep, rmag;
    float inv_w;  // 1.0f / (float)wcell
};
// 32 bytes: the kernel reads its segment as two 16-byte scalar loads
static_assert(sizeof(FastSeg) == 32, "FastSeg is read as two uint4");
inline void fast_seg_staging(FastSeg& G) {
    const int nw = ((G.x0 & 15) + G.cols + 15) >> 4;
    G.nw = (int16_t)nw;
    G.rstep = (int16_t)(256 / nw);
    G.rmag = (int16_t)((4096 + nw - 1) / nw);
    G.inv_w = 1.0f / (float)G.wcell;
}
// k_fast_seg's dynamic LDS: byte offsets of its regions
struct FastLds {
    int img;  // bytes of the staged ROI union (the score map follows at img)
    int ring, clist, bits, cnt, qlist, misc, total;
};

// cv::resize INTER_LINEAR tables (per output column / row).
struct ResizeX {
    int sx0, sx1;
    int a0, a1;
};
struct ResizeY {
    int sy0, sy1;
    int b0, b1;
};

struct FrameCalib {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float depth_factor, mbf;
    float invfx, invfy;
};

// Frame::ExtractFeatures tail for one keypoint (frame.cpp:139-164, 286-313):
// cv::undistortPoints (5 iterations in double; skipped when k1 == 0,
// frame.cpp:288), then the depth at the truncated distorted pixel and the
// back-projection of the undistorted point.
__device__ inline void kp_geometry(float uu, float vv, const FrameCalib& cal, const uint16_t* depth, int img_w,
                                   float* ku, float* p3, float* urp) {
    float ux = uu, uy = vv;
    if (cal.k1 != 0.0f) {
        const double fx = cal.fx, fy = cal.fy, cx = cal.cx, cy = cal.cy;
        const double ifx = 1. / fx, ify = 1. / fy;
        const double k0 = cal.k1, k1 = cal.k2, k2 = cal.p1, k3 = cal.p2, k4 = cal.k3;
        double x = uu, y = vv;
        x = (x - cx) * ifx;
        y = (y - cy) * ify;
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; j++) {
            double r2 = x * x + y * y;
            double icdist = 1 / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
            double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x);
            double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        ux = (float)(fx * x + cx);
        uy = (float)(fy * y + cy);
    }
    ku[0] = ux;
    ku[1] = uy;
    float urv = -1.f, X = 0.f, Y = 0.f, Z = 0.f;
    const uint16_t d16 = depth[(size_t)((int)vv) * img_w + (int)uu];
    const float z = (float)d16 * cal.depth_factor + 0.0f;
    if (z > 0) {
        urv = ux - cal.mbf / z;
        X = (ux - cal.cx) * z * cal.invfx;
        Y = (uy - cal.cy) * z * cal.invfy;
        Z = z;
    }
    p3[0] = X;
    p3[1] = Y;
    p3[2] = Z;
    *urp = urv;
}

// ---- ADAPTIVE grid extractor (k_adaptive.hip)
#define AD_BH 16          // rows per candidate band
#define AD_MAXW 1024      // widest cell detection region (LDS staging)
#define AD_SEL_LDS 4096   // survivors a cell selects in LDS (more: global scratch)
using AdParams = odo_adaptive_params;

// One grid cell of VideoGridAdaptedFeatureDetector (videogridadaptedfeature
// detector.cpp:62-71): ROI [rs,re) x [cs,ce); FAST's detection region is the
// ROI minus 3 pixels on every side: rows [r0,r1), cols [c0,c1).
struct AdCell {
    int rs, re, cs, ce;
    int r0, r1, c0, c1;
    int band0, band1;  // its bands in the band table
    int cand_cap;      // survivor capacity over all its bands
    int pad;
};
// AD_BH rows [y0,y1) of one cell's detection region; its survivors land at
// cand_off of the frame's candidate buffer
struct AdBand {
    int cell, y0, y1, cand_off;
};

// ---- ADAPTIVE grid with the cv::ORB inner detector (k_adaptive_orb.hip):
// cv::ORB::create(10000, 1.2f, 8, 15, 0, 2, HARRIS_SCORE, 31, t) per grid
// cell (detectoradjuster.cpp:29)
#define OA_NLEV 8     // nlevels
#define OA_EDGE 15    // edgeThreshold (runByImageBorder of each level)
#define OA_PATCH 31   // patchSize
#ifndef OA_BH
#define OA_BH 64      // rows per candidate band of a cell level (k_oa_scand; 32: -1 %, profiles/r02_oa_bands_ab)
#endif
// one pyramid level of one grid cell, inside a frame's cell-pyramid buffer
struct OaImg {
    int off, w, h, pitch;
    int quota;         // nfeaturesPerLevel[level] of nfeatures 10000
    int band0, band1;  // its candidate bands (rows [15, h-15))
    int cand_cap;      // survivors over its bands
};
// one grid cell: ROI origin / size in the frame, its 8 level images
struct OaCell {
    int rs, cs, cw, ch;
    int img0;
    int pad[3];
};
struct OaBand {
    int img, y0, y1, cand_off;
};
struct OaScales {
    float s[OA_NLEV];  // getScale(level) = (float)pow((double)1.2f, level)
};

// RANSAC per-pair constants.
struct RansacCfg {
    int iterations;
    int min_inlier_th;
    float max_mahal;
    int sample_size;
    int check_depth;
    double raster_cov_x, raster_cov_y;
    int h0;     // hypotheses of the first eval launch ([0, h0)); set by launch_ransac
    int lanes_min_open;  // odo_kernel_forms.ransac_lanes_min_open (0 = default)
    int fold_wave;       // ordered fold by the whole wave (a lone pair); set by launch_ransac
    int first_hyps;      // odo_kernel_forms.ransac_first_hyps (0 = EV_H0)
};

// ---- launch wrappers (defined next to their kernels)
void launch_kp_geometry(hipStream_t st, const orb_kp* kps, const int* nkp, const uint16_t* depth, size_t depth_stride,
                        int img_w, FrameCalib cal, float* kun, float* xyz, float* ur, int kp_cap, int nframes);
void launch_gray(hipStream_t st, const uint8_t* bgr, uint8_t* pyr, int w, int h, int pitch, size_t in_stride,
                 size_t pyr_stride, int nframes);
size_t resize_lds_bytes(int spitch, int dw, int max_src_rows);
// gray + every pyramid level in one launch (one workgroup per frame); bgr may be
// null (level 0 already in place). pyramid_fusable: the host check of its
// assumptions (<= 16 levels, <= 4096 px wide, each quad's taps inside 8 bytes)
void launch_pyramid(hipStream_t st, const uint8_t* bgr, uint8_t* pyr, size_t in_stride, size_t pyr_stride,
                    const LevelDesc* lv, const ResizeX* rx, const ResizeY* ry, const int* rx_off, const int* ry_off,
                    int nlevels, int nframes, uint8_t* blur, const LevelDesc* lv_host,
                    const ResizeY* ry_h);
// blur: the blurred pyramid is written by the same launch (null: not);
// pyramid_blur_fusable: every level is large enough for the strip walks
bool pyramid_blur_fusable(const LevelDesc* lv_host, int nlevels);
bool pyramid_fusable(const LevelDesc* lv_host, const ResizeX* rx, const int* rx_off, int nlevels);
void launch_resize(hipStream_t st, uint8_t* pyr, size_t pyr_stride, int src_off, int spitch, int dst_off, int dpitch,
                   int dw, int dh, int rb, int max_src_rows, const ResizeX* xt, const ResizeY* yt, int nframes);
void launch_fast(hipStream_t st, const uint8_t* pyr, size_t pyr_stride, const FastSeg* segs, int nsegs,
                 const LevelDesc* lv, uint32_t* cand, int* cand_cnt, int ncells, int cell_cap, int ini_th, int min_th,
                 const FastLds& lds, int nframes);
// LDS layout of k_fast_seg for the context's largest segment (false: too large)
bool fast_lds_plan(const FastSeg* segs, int nsegs, FastLds& L);
size_t octree_lds_bytes(int node_cap);
void launch_octree(hipStream_t st, const uint32_t* cand, const int* cand_cnt, const LevelDesc* lv, int ncells,
                   int cell_cap, int nlevels, uint32_t* keys, int32_t* knode, size_t keys_stride,
                   uint32_t* okp, int* ocnt, int okp_stride, int node_cap, int nframes);
void launch_blur(hipStream_t st, const uint8_t* pyr, uint8_t* blur, size_t pyr_stride, const LevelDesc* lv,
                 const LevelDesc* lv_host, int nlevels, int nframes);
void launch_finalize(hipStream_t st, const uint8_t* pyr, const uint8_t* blur, size_t pyr_stride, const LevelDesc* lv,
                     int nlevels, const uint32_t* okp, const int* ocnt, int okp_stride, const uint16_t* depth,
                     size_t depth_stride, int img_w, FrameCalib cal, orb_kp* kps, uint8_t* desc, float* kun, float* xyz,
                     float* ur, int* nkp, int kp_cap, int nframes, bool geometry = true);
void launch_pair_valid(hipStream_t st, int* pv, int n, int first_valid);
void launch_copy_frame(hipStream_t st, const orb_kp* kps_s, const uint8_t* desc_s, const float* kun_s,
                       const float* xyz_s, const float* ur_s, const int* n_s, orb_kp* kps_d, uint8_t* desc_d,
                       float* kun_d, float* xyz_d, float* ur_d, int* n_d, int kp_cap);
void launch_knn2(hipStream_t st, const uint8_t* q, const int* qn, size_t q_stride, const uint8_t* t, const int* tn,
                 size_t t_stride, int2* idx, int2* dist, size_t out_stride, int max_q, int npairs,
                 const int32_t* qlist = nullptr, const int* qcnt = nullptr, size_t ql_stride = 0, int nsplit = 1,
                 size_t split_stride = 0);
// the same top-2 on the matrix cores (exact FP4 sign-vector formulation); one
// split slot, all trains, at most 8192 of them (k_knn2_f4)
void launch_knn2_f4(hipStream_t st, const uint8_t* q, const int* qn, size_t q_stride, const uint8_t* t, const int* tn,
                    size_t t_stride, int2* idx, int2* dist, size_t out_stride, int max_q, int npairs,
                    const int32_t* qlist = nullptr, const int* qcnt = nullptr, size_t ql_stride = 0);
void launch_vo_lm(hipStream_t st, const float* xyz, const int* nkp, int kp_cap, int slot0, float th_depth_m,
                  uint32_t* lm_bits, int lm_words, int32_t* qlist, int* qcnt, int npairs);
void launch_pair_match(hipStream_t st, const int2* knn_idx, const int2* knn_dist, size_t knn_stride, const float* xyz,
                       const int* nkp, int kp_cap, int slot0, float ratio, const uint32_t* lm_bits, int lm_words,
                       int nsplit, size_t split_stride, int check_depth,
                       odo_dmatch* matches, int* n_matches, void* good, int* n_good, int32_t* f2_src,
                       uint64_t* sort_scratch, int match_cap, int npairs);
int launch_sort_dbg(hipStream_t st, void* a, int n);
void launch_latch(hipStream_t st, double* latch, const void* good, const int* n_good, const int* n_matches,
                  const odo_dmatch* matches, const float* xyz, int kp_cap, int slot0, int npairs, int match_cap,
                  int min_inl, int sample_size, int iterations, const int* pair_valid, int* set_flag = nullptr);
size_t ransac_gpt_bytes();
// rand() words for every pair (data independent): launched ahead of
// launch_ransac on the same stream.
void launch_ransac_raw(hipStream_t st, void* scratch, int npairs, int match_cap, int mask_words, RansacCfg cfg,
                       uint64_t seed_base, uint64_t pair_base, odo_rng* rng_io);
void launch_ransac(hipStream_t st, const void* good, const int* n_good, const int* n_matches,
                   const odo_dmatch* matches, const float* xyz, int kp_cap, int slot0, int match_cap, RansacCfg cfg,
                   const double* latch, const int* pair_valid, int min_matches, odo_rng* rng_io, void* scratch,
                   uint32_t* best_mask, int mask_words, odo_pair_result* res, float* T12, int npairs,
                   int* open_hint = nullptr);
// hypotheses mode: samples of every hypothesis, evaluation of [h_lo, h_hi)
// only, no fold and no outputs
void launch_ransac_hyps(hipStream_t st, const void* good, const int* n_good, const int* n_matches,
                        const odo_dmatch* matches, const float* xyz, int kp_cap, int slot0, int match_cap,
                        RansacCfg cfg, const double* latch, const int* pair_valid, int min_matches, odo_rng* rng_io,
                        void* scratch, uint32_t* best_mask, int mask_words, odo_pair_result* res, float* T12,
                        int npairs, int h_lo, int h_hi);
size_t ransac_scratch_bytes(int npairs, int match_cap, int mask_words, const RansacCfg& cfg);
void ransac_read_hyps(hipStream_t st, void* scratch, int match_cap, int mask_words, RansacCfg cfg, int h0, int h1,
                      double* err, int* cnt, float* T);
void launch_ransac_finish(hipStream_t st, void* scratch, int match_cap, int mask_words, RansacCfg cfg,
                          const double* latch, odo_rng* rng_io, uint32_t* best_mask, odo_pair_result* res, float* T12,
                          int best_h, int visited, int valid, int best_cnt, float rmse);
// hypotheses mode with the exchange on the device (odo_ransac_hyps_dev ...)
void ransac_export_hyps(hipStream_t st, void* scratch, int match_cap, int mask_words, RansacCfg cfg, int h0, int h1,
                        void* d_block);
void launch_hyp_fold(hipStream_t st, const void* d_all, int H, int iterations, int ng, int min_inl, int sample_size,
                     odo_ransac_fold_result* d_out);
void launch_hyp_finish(hipStream_t st, void* scratch, int match_cap, int mask_words, RansacCfg cfg,
                       const double* latch, odo_rng* rng_io, uint32_t* best_mask, odo_pair_result* res, float* T12,
                       const odo_ransac_fold_result* d_fold, int h0, int h1, int rank0, const odo_dmatch* good, int ng,
                       int* payload, int words);
int hyp_payload_words(int ng);
size_t pnp_edge_bytes();
// sel / sel_val (only the pairs with sel[p] == sel_val): no caller passes them
// any more. Taking them out changed the register allocation of k_pnp<true>
// (324 -> 330 VGPRs) and measured ~0.3 % slower on the bench line, so the
// kernel keeps its signature (DESIGN §4 Pipelining).
void launch_pnp(hipStream_t st, const int32_t* f2_src, const float* xyz, const float* kun, const float* ur,
                const int* nkp, int kp_cap, int slot0, FrameCalib cal, const float* T12, const int* pair_valid,
                const int* n_matches, int min_matches, void* edges, odo_pair_result* res, uint8_t* inlier_mask,
                int npairs, const int* sel = nullptr, int sel_val = 0);
void launch_kabsch(hipStream_t st, const float* A, const float* B, int n, float* T);
// Local bundle adjustment (k_ba.hip). Device pointers unless noted: the
// uploaded problem (edges, their CSRs by landmark and by keyframe in edge
// order, pidx[k] = index of keyframe k among the free ones or -1, insys[k] =
// free and observed), the download block (oT nk x 16, oX nl x 3, erase ne,
// counts: level-1 marks, erase marks) and ba_scratch_bytes() of scratch.
// h_scal: 8 doubles of pinned host memory for the per-trial scalars.
struct BaArgs {
    int nk, nl, ne, nf;
    const float *Tcw, *Xw, *eobs;
    const int32_t *ekf, *elm, *lstart, *lorder, *kstart, *korder, *pidx;
    const uint8_t* insys;
    float *oT, *oX;
    uint8_t* erase;
    int32_t* counts;
    void* scratch;
    double* h_scal;
    double fx, fy, cx, cy, bf;
};
size_t ba_scratch_bytes(int nk, int nl, int ne, int nf);
hipError_t ba_run(hipStream_t st, const BaArgs& a, const odo_ba_params& p, odo_ba_result* res);
// GICP (k_gicp.hip), nprob problems: source p = points [soffs[p], soffs[p+1]) of
// src, target p = [toffs[p], toffs[p+1]) of tgt. Cs sum(ns)*9, Ct sum(nt)*9,
// outp sum(ns)*3, Mah sum(ns)*9, is / it sum(ns); T12 16 and outi 4 per problem.
struct GicpArgs {
    const float* guess;  // 16 per problem (device)
    const int* soffs;    // nprob + 1 (device)
    const int* toffs;
    double max_corr_dist;
    int max_iterations;
    int max_inner;
};
void launch_gicp(hipStream_t st, const float* src, const float* tgt, int nprob, int max_ns, int max_nt, double* Cs,
                 double* Ct, float* outp, double* Mah, int* is, int* it, GicpArgs args, float* T12, int* outi);
// launch_gicp's first launch by itself: k_gicp_cov on the source and target
// clouds of nprob problems (a problem with a cloud under 20 points is skipped,
// its rows of Cs / Ct are not written); max_n = the longest cloud of either side
void launch_gicp_cov(hipStream_t st, const float* src, const int* soffs, double* Cs, const float* tgt,
                     const int* toffs, double* Ct, int nprob, int max_n);
// Dense GICP (k_gicp.hip; DESIGN §4 "Dense GICP"): the neighbour searches over
// a uniform grid per cloud. The clouds of a call lie packed (x, y, z) one after
// the other in P; cloud k is points [p0, p0 + n). Its grid has gx * gy * gz
// cells (x fastest), cell (i, j, k) = floorf((p - mn) * inv) per axis, clamped;
// cstart[c0 + cell] is the first row of the cell in `sorted` (x, y, z, index
// within the cloud as int bits), rows of all clouds in one sequence, so
// cstart[c0 + ncells] is the cloud's end and the next cloud's first cell.
constexpr int GG_MAX_POINTS = 1 << 20;      // points per cloud
constexpr int64_t GG_MAX_CELLS = 1 << 24;   // cells per cloud (the table budget)
constexpr int64_t GG_MAX_TOTAL_CELLS = 1 << 28;  // cells of all clouds of a call
struct GgCloud {
    int p0, n, c0;
    int gx, gy, gz;
    float mn[3], inv;
    // the stop rule: after Chebyshev ring r every unseen point has a float
    // squared distance of at least gg_ring_bound(w, slack, r)
    double w, slack;
    int rings;  // ICP: rings searched around the query's cell
};
// the stop rule's bound; one definition for the host (rings) and the kernels
__host__ __device__ inline double gg_ring_bound(double w, double slack, int r) {
    const double g = r * w - slack;
    return g > 0 ? g * g * (1.0 - 0x1p-20) - 0x1p-140 : 0.0;
}
// a problem of the grid ICP: clouds by index, `work` the first row of its own
// outp / Mah / is / it (sized by the source)
struct GgPair {
    int s, t, work;
};
// cloud k: x, y, z of rows [row0[k], ...) of `stride` floats at src into the
// packed rows [offs[k], offs[k + 1]) of dst (row0, offs on the device)
void launch_gg_pack(hipStream_t st, const float* src, int stride, const int* row0, const int* offs, int ncl,
                    int max_n, float* dst);
// bounds[6 * k]: min x, y, z and max x, y, z of cloud k as ordered uint32
// (f32_ordered, odo_wave.h), preset to 0xffffffff / 0 by the caller; offs ncl + 1 (device)
void launch_gg_bounds(hipStream_t st, const float* P, const int* offs, int ncl, int max_n, uint32_t* bounds);
// counting sort of every cloud by cell: cnt and fill (ncells_total + 1 each) are
// preset to 0; cnt becomes cstart, bsum holds (ncells_total + 1 + 4095) / 4096 ints
void launch_gg_build(hipStream_t st, const float* P, const GgCloud* cl, int ncl, int max_n, int64_t ncells_total,
                     int* key, int* cnt, int* fill, int* bsum, float4* sorted);
// computeCovariances of every cloud of >= 20 points: C 9 per point, in point order
void launch_gg_cov(hipStream_t st, const float* P, const GgCloud* cl, int ncl, int max_n, const int* cstart,
                   const float4* sorted, double* C);
// k_gicp with the grid correspondence search, one workgroup per pair
void launch_gg_icp(hipStream_t st, const float* P, const GgCloud* cl, const GgPair* pairs, int nprob,
                   const int* cstart, const float4* sorted, const double* C, float* outp, double* Mah, int* is,
                   int* it, const float* guess, double max_corr_dist, int max_iterations, int max_inner, float* T12,
                   int* outi);
// StatisticalOutlierRemoval and getFitnessScore over the same grids (k_gicp.hip;
// DESIGN §4 "SOR and fitness"). One record per cloud:
constexpr int SOR_MAX_K = 64;  // mean_k: 65 floats per lane of LDS (PCL's default is 50)
struct SorStats {
    double sum, sq_sum, mean, stddev, threshold;
    int n_out, pad;
};
// dist (point order, preset to 0), stats (preset: zeros) and keep of every
// cloud; a cloud of at most mean_k points keeps all. chunk_cnt: ncl x
// ceil(max_n / 256) ints, on return the first kept rank of every 256-point chunk
void launch_sor(hipStream_t st, const GgCloud* cl, int ncl, int max_n, const int* cstart, const float4* sorted,
                int mean_k, double stddev_mul, float* dist, SorStats* stats, uint8_t* keep, int* chunk_cnt);
// the kept 16-byte rows pts[row0[k] + i] and their counts, in order, to rows
// new0[k] ... of pts_out / counts_out (row0, new0 on the device)
void launch_sor_pack(hipStream_t st, const GgCloud* cl, int ncl, int max_n, const uint8_t* keep, const int* chunk_cnt,
                     const int* row0, const int* new0, const void* pts, const int* counts, void* pts_out,
                     int* counts_out);
// nn[pair.work + i] = the nearest squared distance of T[pair] * source point i
// over the whole target; score[pair] = their mean, DBL_MAX for an empty side
void launch_gg_fitness(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, int max_ns,
                       const int* cstart, const float4* sorted, const float* T, float* nn, double* score);
// libicp's IcpPointToPlane over the same grids (k_icp.hip; DESIGN §4
// "Point-to-plane ICP"). One record per pair, kept on the device between the
// rounds of sweep + step:
constexpr int ICP_MAX_K = 32;  // num_neighbors: 8 bytes per neighbour and lane of LDS
struct IcpState {
    float R[9], t[3];
    float delta;
    int iter, n_active, status, done, pad;
    double indist, residual;
};
// computeNormals of every cloud k with need[k] != 0 and at least 5 points:
// normals 3 floats per point, in point order (preset by the caller)
void launch_icp_normals(hipStream_t st, const float* P, const GgCloud* cl, const int* need, int ncl, int max_n,
                        const int* cstart, const float4* sorted, int num_neighbors, float* normals);
// one search per template point at the pair's R, t: the gate and the row of
// [A | b] into rows (8 words per point at the pair's `work`, point order);
// residual != 0: getResidual's term of the last active set instead
void launch_icp_sweep(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, int max_ns,
                      const int* cstart, const float4* sorted, const float* normals, const IcpState* state, int gate,
                      double indist, int residual, float* rows);
// fitStep's solve and composition per pair from its rows, the loop test and
// the done latch (*unfinished counts the pairs still running); residual != 0:
// the mean of the residual terms
void launch_icp_step(hipStream_t st, const GgCloud* cl, const GgPair* pairs, int nprob, const float* rows,
                     IcpState* state, int max_iterations, double min_delta, int residual, int* unfinished);
// Batched ADAPTIVE_RICP / RANSAC back-ends (k_ricp.hip), on the pair stream
// after launch_ransac. The branch rule's constants (odometry.cpp:52-53):
struct RicpCfg {
    int min_inliers;
    float rmse_scale, refine_at, reset_at;
};
// branch npairs, guess 16 per pair, offs npairs + 1 (source and target clouds
// of a pair have one length: the offsets serve both)
void launch_ricp_plan(hipStream_t st, const odo_pair_result* res, const float* T12, const int* pair_valid,
                      const int* n_matches, const int* n_good, int min_matches, int min_inlier_th, int match_cap,
                      RicpCfg cfg, int* branch, float* guess, int* offs, int npairs);
// src / tgt: up to npairs * match_cap points
void launch_ricp_gather(hipStream_t st, const odo_dmatch* matches, const int* n_matches, const float* xyz, int kp_cap,
                        int slot0, int match_cap, int check_depth, const int* offs, float* src, float* tgt,
                        int npairs);
// RANSAC mode: branch, offs, gT, gio and ricp null (every pair keeps RANSAC's T12)
void launch_ricp_apply(hipStream_t st, const int* pair_valid, const int* n_matches, const int* n_good,
                       const odo_dmatch* matches, const void* good, const uint32_t* best_mask, int mask_words,
                       int match_cap, const int* nkp, int kp_cap, int slot0, const float* T12, const int* branch,
                       const int* offs, const float* gT, const int* gio, odo_pair_result* res, odo_ricp_result* ricp,
                       uint8_t* inlier_mask, int npairs);
// PnPRansac (k_pnpransac.hip), nprob problems, problem p = points [offs[p], offs[p+1]):
// idx P*H*5, model P*H*6, Rproj P*H*9, mask H*sum(n), good P*H, state P*4, res P, mask_out sum(n)
int pnp_ransac_max_points();
void launch_pnp_ransac(hipStream_t st, const float* Xw, const float* uv, const int* offs, int nprob,
                       const float K4[4], int H, float reproj_err, double confidence, int* idx, double* model,
                       double* Rproj, uint8_t* mask, int* good, int* state, odo_pnp_ransac_result* res,
                       uint8_t* mask_out);
// The local-map search (k_localmap.hip) over nframes frames of kp_cap keypoint
// rows each: kun / oct / desc / nkp point at the first frame searched. The
// octave of keypoint j of frame f is oct[(f * kp_cap + j) * oct_stride]
// (stride in 32-bit words: sizeof(orb_kp) / 4 over orb_kp rows, 1 over a
// plain array).
struct LmGrid {
    float x0, y0, inv;  // origin (minX, minY) and 1 / cell size of the keypoint grid
    int gx, gy;
};
struct LmCalib {
    float fx, fy, cx, cy, mbf;
    float minX, maxX, minY, maxY;
};
struct LmSearch {
    int nframes, nL, kp_cap, seen_words;
    const float* Tcw;            // nframes x 16
    const odo_landmark* lms;     // nL
    const int32_t* prior;        // nframes x kp_cap or null
    const uint8_t* taken_in;     // nframes x kp_cap or null: the taken slots of a search without a prior
    const float* kun;            // nframes x kp_cap x 2
    const int32_t* oct;
    int oct_stride;
    const uint8_t* desc;         // nframes x kp_cap x 32
    const int* nkp;              // nframes
    LmGrid G;
    LmCalib C;
    float th, nnratio;
    uint32_t* seen;              // nframes x seen_words, zeroed by the caller
    int32_t* prior_eff;          // nframes x kp_cap
    uint8_t* taken0;             // nframes x kp_cap
    float2* bxy;                 // nframes x kp_cap
    uint32_t* bjo;               // nframes x kp_cap
    int* cstart;                 // nframes x (gx * gy + 1)
    float* proj;                 // nframes x nL x 3
    int* ccount;                 // nframes x nL
    uint32_t* cand;              // nframes x local_map_cand_cap() x nL
    int32_t *choice, *over;      // nframes x nL each
    int32_t *slot_lm, *f2_src;   // nframes x kp_cap each
    float* Xg;                   // nframes x kp_cap x 3
    odo_local_map_result* res;   // nframes
};
int local_map_cand_cap();
LmGrid local_map_grid(const float bounds[4]);
// prior, bins, candidates, resolve, merge and edge gather; -1: kp_cap above 8191
int launch_local_map_search(hipStream_t st, const LmSearch& a);
// after the batch's k_pnp; nkp is the batch's slot-0 base, as launch_pnp takes it (frame f in slot f + 1)
void launch_local_map_stats(hipStream_t st, const odo_landmark* lms, const int* nkp, int kp_cap, const int32_t* slot_lm,
                            const uint8_t* pnp_mask, const odo_pair_result* pres, uint8_t* outlier,
                            odo_local_map_result* res, int nframes);
// Matcher::Fuse's search for n_kf calls (k_fuse.hip). Device pointers: the
// uploaded calls, keypoint rows, landmarks and index list; kp_off[k] = call
// k's first row of bpt (n_kf + 1 prefix sums of the calls' keypoint counts),
// rec_off[k] = its first record (prefix sums of the list lengths); bpt
// kp_off[n_kf] sorted points, cstart n_kf x (gx * gy + 1) cell starts.
// max_kp / max_list: the largest keypoint count / list length of a call.
struct FuseSearch {
    int n_kf, n_lms, max_kp, max_list;
    const odo_fuse_kf* kfs;
    const float *kun, *ur;
    const uint8_t* desc;
    const odo_landmark* lms;
    const int32_t *lm_index, *kp_off, *rec_off;
    LmGrid G;
    LmCalib C;
    float th;
    float4* bpt;
    int* cstart;
    odo_fuse_cand* out;
};
// bins and search; -1: a call with more than 8191 keypoints
int launch_fuse_search(hipStream_t st, const FuseSearch& a);
// Dense clouds (k_cloud.hip). A frame's elements (pixels, then its valid
// points) are cut into chunks of CLOUD_CHUNK, one wave each; nch chunks cover
// the W * H pixels of a frame.
constexpr int CLOUD_CHUNK = 1024;
// the plan of one frame, written by k_cloud_bounds / k_cloud_plan / k_cloud_voxels
struct CloudFrame {
    uint32_t lo[3], hi[3];  // min / max of x, y, z as order-preserving bits
    int32_t n_valid;        // pixels with z > 0
    int32_t filtered;       // the voxel grid applies (else the raster cloud is the result)
    int32_t npass;          // radix passes (key bytes that can be non-zero); the sorted keys lie in buffer npass & 1
    float inv;              // 1.0f / leaf
    int32_t min_b[3];
    uint32_t div0, div01;   // div_b[0], div_b[0] * div_b[1] (wrapping)
    int32_t n_points, out_off;  // voxels; the frame's first point in the output
    int32_t pad;
};
struct CloudArgs {
    int n, W, H, nch;
    FrameCalib cal;
    float leaf;
    const uint8_t* bgr;     // [n][H][W][3]
    const uint16_t* depth;  // [n][H][W]
    const float* Twc;       // [n][16] or nullptr
    CloudFrame* fr;         // [n]
    odo_cloud_info* info;   // [n]
    int32_t *chunk_off, *head_off;  // [n][nch]: valid pixels / voxel heads before each chunk
    int32_t* hist;          // [n][nch][256]
    uint32_t *key[2], *idx[2];  // [n][W * H] each: (key, pixel) ping-pong
    odo_cloud_point* out;
    int32_t* counts;
};
// bounds, plan, keys, the radix sort, the voxel heads and info[] (all but the points)
void launch_cloud_voxels(hipStream_t st, const CloudArgs& a);
// the voxel starts and the centroids into out / counts; max_points: the largest n_points of a frame
void launch_cloud_points(hipStream_t st, const CloudArgs& a, int max_points);
void launch_adapt_smap(hipStream_t st, const uint8_t* pyr, size_t pyr_stride, int w, int h, int pitch, uint8_t* smap,
                       size_t smap_stride, int nframes);
void launch_adapt_cand(hipStream_t st, const uint8_t* smap, size_t smap_stride, int pitch, const AdBand* bands,
                       int nbands, const AdCell* cells, int ncells, uint32_t* cand, size_t cand_stride, int* band_cnt,
                       int* hist, int nframes);
void launch_adapt_chain(hipStream_t st, const int* hist, int ncells, int nframes, AdParams P, double* thresh,
                        int* tsel, int* nsel);
size_t adapt_select_lds_bytes();
void launch_adapt_select(hipStream_t st, const uint32_t* cand, size_t cand_stride, const int* band_cnt, int nbands,
                         const AdBand* bands, const AdCell* cells, int ncells, const int* tsel, const int* nsel,
                         int max_per_cell, uint32_t* big, size_t big_stride, uint32_t* cell_out, int* cell_cnt,
                         int nframes);
size_t adapt_assemble_lds_bytes(int ncells, int max_per_cell);
void launch_adapt_assemble(hipStream_t st, const uint32_t* cell_out, const int* cell_cnt, int ncells, int max_per_cell,
                           int retain, int w, int h, uint32_t* akp, int akp_stride, int* nkp, int kp_cap,
                           int nframes);
void launch_adapt_finalize(hipStream_t st, const uint8_t* blur, size_t pyr_stride, int pitch, const uint32_t* akp,
                           int akp_stride, const int* nkp, float ca, float sb, const uint16_t* depth,
                           size_t depth_stride, int img_w, FrameCalib cal, orb_kp* kps, uint8_t* desc, float* kun,
                           float* xyz, float* ur, int kp_cap, int nframes);
void launch_oa_pyr(hipStream_t st, const uint8_t* pyr, size_t pyr_stride, int gpitch, const OaCell* cells, int ncells,
                   const OaImg* imgs, int buf0, int buf1, uint8_t* cpyr, size_t cp_stride, int nframes);
size_t oa_scand_lds_bytes(int maxpitch);
void launch_oa_scand(hipStream_t st, const uint8_t* cpyr, size_t cp_stride, const OaImg* imgs, int nimgs,
                     const OaBand* bands, int nbands, uint32_t* cand, size_t cand_stride, int* band_cnt, int* hist,
                     int maxpitch, int nframes);
void launch_oa_count(hipStream_t st, const int* hist, const OaCell* cells, const OaImg* imgs, int nimgs, int ncells,
                     int* phist, int nframes);
size_t oa_select_scratch_bytes(int ncap);
void launch_oa_select(hipStream_t st, const uint32_t* cand, size_t cand_stride, const int* band_cnt, int nbands,
                      const OaBand* bands, const OaImg* imgs, const OaCell* cells, int ncells, const int* tsel,
                      const uint8_t* cpyr, size_t cp_stride, int max_per_cell, uint8_t* scr, size_t scr_stride,
                      int ncap, uint64_t* cell_out, int* cell_cnt, int nframes);
size_t oa_assemble_lds_bytes(int ncells, int max_per_cell);
void launch_oa_assemble(hipStream_t st, const uint64_t* cell_out, const int* cell_cnt, const OaCell* cells,
                        int ncells, int max_per_cell, int retain, int w, int h, OaScales sc, uint64_t* akp,
                        int akp_stride, int* nkp, int kp_cap, int nframes);
void launch_oa_finalize(hipStream_t st, const uint8_t* pyr, const uint8_t* blur, size_t pyr_stride,
                        const LevelDesc* lv, const uint8_t* cpyr, size_t cp_stride, const OaImg* imgs,
                        const OaCell* cells, OaScales sc, const uint64_t* akp, int akp_stride, const int* nkp,
                        const uint16_t* depth, size_t depth_stride, int img_w, FrameCalib cal, orb_kp* kps,
                        uint8_t* desc, float* kun, float* xyz, float* ur, int kp_cap, int nframes);
void launch_adapt_select_dbg(hipStream_t st, uint32_t* a, int n, int nth, int mode, int* posL, int* posR,
                             int* n_out);

}  // namespace odo
