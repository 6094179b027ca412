// Host geometry tables of a context, built once per image size: pyramid
// levels, FAST cells and segments, resize coefficients (build_geometry) and
// the cell / band tables of the two ADAPTIVE detectors.
#include "odo_ctx.h"

inline int cvRoundH(float v) { return (int)lrintf(v); }
inline int cvFloorH(float v) {
    int i = (int)v;
    return i - (i > v);
}
inline int satShort(float v) {
    int r = cvRoundH(v);
    return std::min(std::max(r, -32768), 32767);
}

// ADAPTIVE with the cv::ORB inner detector: per grid cell the 8 levels of
// cv::ORB's pyramid of the cell sub-image (getScale sizes, orb.cpp), their
// candidate bands (rows [15, h-15) in OA_BH-row bands; strict 3x3 maxima are
// never 8-adjacent: <= ceil(r/2)ceil(c/2) survivors); the frame
// pyramid (pyr / blur, built by build_geometry) must have cv::ORB's level
// sizes, since cv::ORB::compute samples it.
static int build_adaptive_orb_geometry(odo_ctx* c) {
    const odo_adaptive_params& P = c->cfg.adaptive;
    float scale[OA_NLEV];
    int quota[OA_NLEV];
    {
        const double sf = (double)1.2f;
        const float factor = (float)(1.0 / sf);
        float nd = 10000 * (1 - factor) / (1 - (float)pow((double)factor, (double)OA_NLEV));
        int sum = 0;
        for (int l = 0; l < OA_NLEV; l++) {
            scale[l] = (float)pow(sf, (double)l);
            c->osc.s[l] = scale[l];
            if (l < OA_NLEV - 1) {
                quota[l] = cvRoundH(nd);
                sum += quota[l];
                nd *= factor;
            } else
                quota[l] = std::max(10000 - sum, 0);
        }
    }
    // the DetectorAdjuster chain runs on sum_l min(count_l, quota_l): exact
    // decisions need every quota above gridMax (k_adaptive_orb.hip)
    for (int l = 0; l < OA_NLEV; l++)
        if (quota[l] <= P.cell_max) return fail(ODO_ERR_ARG, "ADAPTIVE ORB: a level quota <= cell_max");
    if (c->nlevels < OA_NLEV) return fail(ODO_ERR_ARG, "ADAPTIVE ORB needs orb.nlevels >= 8 (frame pyramid)");
    for (int l = 0; l < OA_NLEV; l++) {
        const float inv = 1.0f / scale[l];
        if (cvRoundH((float)c->W * inv) != c->lv_h[l].w || cvRoundH((float)c->H * inv) != c->lv_h[l].h)
            return fail(ODO_ERR_ARG, "ADAPTIVE ORB: cv::ORB level size differs from the frame pyramid's");
    }
    c->oai_h.clear();
    c->oac_h.clear();
    c->oab_h.clear();
    int off = 0, coff = 0, buf0 = 0, buf1 = 0;
    c->oa_ncap = 1;
    for (const AdCell& A : c->adc_h) {
        OaCell C{};
        C.rs = A.rs;
        C.cs = A.cs;
        C.cw = A.ce - A.cs;
        C.ch = A.re - A.rs;
        C.img0 = (int)c->oai_h.size();
        int ncap = 0;
        for (int l = 0; l < OA_NLEV; l++) {
            OaImg I{};
            const float inv = 1.0f / scale[l];
            I.w = cvRoundH((float)C.cw * inv);
            I.h = cvRoundH((float)C.ch * inv);
            if (I.w > 1024 || I.h > 1024) return fail(ODO_ERR_ARG, "ADAPTIVE ORB: cell wider than 1024");
            if (I.w < 1 || I.h < 1) return fail(ODO_ERR_ARG, "ADAPTIVE ORB: empty cell level");
            I.pitch = (I.w + 15) & ~15;
            c->oa_maxpitch = std::max(c->oa_maxpitch, I.pitch);
            I.off = off;
            off += I.pitch * I.h;
            I.quota = quota[l];
            (l & 1 ? buf1 : buf0) = std::max(l & 1 ? buf1 : buf0, I.pitch * I.h);
            const int img = (int)c->oai_h.size();
            I.band0 = (int)c->oab_h.size();
            I.cand_cap = 0;
            const int cw = I.w - 2 * OA_EDGE;
            if (cw > 0)
                for (int y0 = OA_EDGE; y0 < I.h - OA_EDGE; y0 += OA_BH) {
                    OaBand B{img, y0, std::min(y0 + OA_BH, I.h - OA_EDGE), coff};
                    const int cap = ((B.y1 - B.y0 + 1) / 2) * ((cw + 1) / 2);
                    coff += (cap + 3) & ~3;
                    I.cand_cap += cap;
                    c->oab_h.push_back(B);
                }
            I.band1 = (int)c->oab_h.size();
            ncap += I.cand_cap;
            c->oai_h.push_back(I);
        }
        c->oa_ncap = std::max(c->oa_ncap, ncap);
        c->oac_h.push_back(C);
    }
    c->cp_stride = (size_t)off + 64;
    c->ocand_stride = (size_t)std::max(coff, 4);
    c->oa_buf0 = buf0;
    c->oa_buf1 = buf1;
    c->oscr_stride = (oa_select_scratch_bytes(c->oa_ncap) + 255) & ~(size_t)255;
    if (oa_scand_lds_bytes(c->oa_maxpitch) > 160 * 1024) return fail(ODO_ERR_ARG, "ADAPTIVE ORB: cell too wide for the S band");
    if (oa_assemble_lds_bytes(c->ad_ncells, c->ad_mpc) > 160 * 1024)
        return fail(ODO_ERR_ARG, "ADAPTIVE ORB grid keeps too many keypoints for one workgroup");
    if (c->ad_ncells > 15) return fail(ODO_ERR_ARG, "ADAPTIVE ORB: more than 15 grid cells");
    int e;
    if ((e = c->pool.alloc(&c->oai, c->oai_h.size()))) return e;
    if ((e = c->pool.alloc(&c->oac, c->oac_h.size()))) return e;
    if ((e = c->pool.alloc(&c->oab, std::max<size_t>(c->oab_h.size(), 1)))) return e;
    HIPCHK(hipMemcpy(c->oai, c->oai_h.data(), c->oai_h.size() * sizeof(OaImg), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->oac, c->oac_h.data(), c->oac_h.size() * sizeof(OaCell), hipMemcpyHostToDevice));
    if (!c->oab_h.empty())
        HIPCHK(hipMemcpy(c->oab, c->oab_h.data(), c->oab_h.size() * sizeof(OaBand), hipMemcpyHostToDevice));
    return ODO_OK;
}

// ADAPTIVE grid (videogridadaptedfeaturedetector.cpp:62-71): cell ROIs,
// FAST detection regions (ROI minus 3 px) and AD_BH-row bands with survivor
// capacities (strict 3x3 maxima are never 8-adjacent: <= ceil(r/2)ceil(c/2)).
static int build_adaptive_geometry(odo_ctx* c) {
    const odo_adaptive_params& P = c->cfg.adaptive;
    const int W = c->W, H = c->H, R = P.grid_rows, C = P.grid_cols, E = P.edge_threshold;
    if (R <= 0 || C <= 0 || R * C > 64 || E < 0 || P.escape_iters < 1 || P.max_total_keypoints < R * C ||
        !(P.min_thresh <= P.max_thresh))
        return fail(ODO_ERR_ARG, "invalid adaptive params");
    c->ad_ncells = R * C;
    c->ad_mpc = P.max_total_keypoints / (R * C);
    c->adc_h.clear();
    c->adb_h.clear();
    int off = 0, maxcap = 0;
    for (int i = 0; i < R; i++)
        for (int j = 0; j < C; j++) {
            AdCell A{};
            A.rs = std::max((i * H) / R - E, 0);
            A.re = std::min(H, ((i + 1) * H) / R + E);
            A.cs = std::max((j * W) / C - E, 0);
            A.ce = std::min(W, ((j + 1) * W) / C + E);
            A.r0 = A.rs + 3;
            A.r1 = std::max(A.r0, A.re - 3);
            A.c0 = A.cs + 3;
            A.c1 = std::max(A.c0, A.ce - 3);
            if (A.c1 - A.c0 > AD_MAXW) return fail(ODO_ERR_ARG, "adaptive cell wider than AD_MAXW");
            A.band0 = (int)c->adb_h.size();
            A.cand_cap = 0;
            const int cw2 = (A.c1 - A.c0 + 1) / 2;
            for (int y0 = A.r0; y0 < A.r1; y0 += AD_BH) {
                AdBand B{(int)c->adc_h.size(), y0, std::min(y0 + AD_BH, A.r1), off};
                const int cap = ((B.y1 - B.y0 + 1) / 2) * cw2;
                off += (cap + 3) & ~3;
                A.cand_cap += cap;
                c->adb_h.push_back(B);
            }
            A.band1 = (int)c->adb_h.size();
            maxcap = std::max(maxcap, A.cand_cap);
            c->adc_h.push_back(A);
        }
    c->ad_nbands = (int)c->adb_h.size();
    c->acand_stride = (size_t)std::max(off, 4);
    c->abig_stride = (size_t)3 * std::max(maxcap, 1);
    const int need = c->ad_ncells * c->ad_mpc;
    if (adapt_assemble_lds_bytes(c->ad_ncells, c->ad_mpc) > 160 * 1024)
        return fail(ODO_ERR_ARG, "adaptive grid keeps too many keypoints for one workgroup");
    c->kp_cap = std::max(c->kp_cap, (need + 63) & ~63);
    if (c->adaptive_orb) {
        int e;
        if ((e = build_adaptive_orb_geometry(c))) return e;
    }
    // ORB's rBRIEF at the FAST keypoints' angle -1 (orb.cpp computeOrbDescriptors)
    const float ang = -1.f * (float)(M_PI / 180.f);
    c->a_cos = (float)cos((double)ang);
    c->a_sin = (float)sin((double)ang);
    int e;
    if ((e = c->pool.alloc(&c->adc, c->adc_h.size()))) return e;
    if ((e = c->pool.alloc(&c->adb, std::max<size_t>(c->adb_h.size(), 1)))) return e;
    HIPCHK(hipMemcpy(c->adc, c->adc_h.data(), c->adc_h.size() * sizeof(AdCell), hipMemcpyHostToDevice));
    if (!c->adb_h.empty())
        HIPCHK(hipMemcpy(c->adb, c->adb_h.data(), c->adb_h.size() * sizeof(AdBand), hipMemcpyHostToDevice));
    return ODO_OK;
}

int odo::reset_adaptive(odo_ctx* c) {
    if (!c->adaptive) return ODO_OK;
    std::vector<double> t(c->ad_ncells, c->cfg.adaptive.init_thresh);
    HIPCHK(hipMemcpy(c->athresh, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return ODO_OK;
}

int odo::build_geometry(odo_ctx* c) {
    const odo_orb_params& p = c->cfg.orb;
    const int W = c->W, H = c->H;
    c->nlevels = p.nlevels;
    // ORBextractor tables (orbextractor.cpp:353-381); scaleFactor member is double
    std::vector<float> scale(p.nlevels), inv(p.nlevels);
    scale[0] = 1.0f;
    for (int i = 1; i < p.nlevels; i++) scale[i] = (float)((double)scale[i - 1] * (double)p.scale_factor);
    for (int i = 0; i < p.nlevels; i++) inv[i] = 1.0f / scale[i];
    std::vector<int> quota(p.nlevels);
    const double sf = (double)p.scale_factor;
    float factor = (float)(1.0f / sf);
    float nDesired = p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)p.nlevels));
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; l++) {
        quota[l] = cvRoundH(nDesired);
        sum += quota[l];
        nDesired *= factor;
    }
    quota[p.nlevels - 1] = std::max(p.nfeatures - sum, 0);

    c->lv_h.resize(p.nlevels);
    int off = 0, maxq = 0, max_nini = 1;
    size_t key_off = 0;
    c->cells_h.clear();
    c->fsegs_h.clear();
    int max_tiles = 0;
    for (int l = 0; l < p.nlevels; l++) {
        LevelDesc& L = c->lv_h[l];
        L.w = cvRoundH((float)W * inv[l]);
        L.h = cvRoundH((float)H * inv[l]);
        L.pitch = (L.w + 15) & ~15;
        L.off = off;
        L.scale = scale[l];
        L.quota = quota[l];
        off += L.pitch * L.h;
        maxq = std::max(maxq, quota[l]);
        if (L.w < 40 || L.h < 40) return fail(ODO_ERR_ARG, "pyramid level too small (< 40 px)");
        // FAST cells (orbextractor.cpp:669-703)
        const float Wc = 30;
        const int minBorderX = 16, minBorderY = 16;
        const int maxBorderX = L.w - 16, maxBorderY = L.h - 16;
        const float width = (float)(maxBorderX - minBorderX), height = (float)(maxBorderY - minBorderY);
        const int nCols = (int)(width / Wc), nRows = (int)(height / Wc);
        const int wCell = (int)ceil(width / nCols), hCell = (int)ceil(height / nRows);
        L.cell_begin = (int)c->cells_h.size();
        for (int i = 0; i < nRows; i++) {
            const float iniY = (float)(minBorderY + i * hCell);
            float maxY = iniY + hCell + 6;
            if (iniY >= maxBorderY - 3) continue;
            if (maxY > maxBorderY) maxY = (float)maxBorderY;
            for (int j = 0; j < nCols; j++) {
                const float iniX = (float)(minBorderX + j * wCell);
                float maxX = iniX + wCell + 6;
                if (iniX >= maxBorderX - 6) continue;
                if (maxX > maxBorderX) maxX = (float)maxBorderX;
                CellDesc C;
                C.level = (int16_t)l;
                C.y0 = (int16_t)(int)iniY;
                C.x0 = (int16_t)(int)iniX;
                C.rows = (int16_t)((int)maxY - (int)iniY);
                C.cols = (int16_t)((int)maxX - (int)iniX);
                C.offx = (int16_t)(j * wCell);
                C.offy = (int16_t)(i * hCell);
                C.pad = 0;
                if (C.rows > FAST_ROI_MAX || C.cols > FAST_ROI_MAX) return fail(ODO_ERR_ARG, "FAST cell exceeds ROI max");
                c->cells_h.push_back(C);
                c->fast_roi = std::max(c->fast_roi, (int)std::max(C.rows, C.cols));
                c->cell_cap = std::max(c->cell_cap, ((C.rows - 6 + 1) / 2) * ((C.cols - 6 + 1) / 2) + 1);
            }
        }
        L.cell_end = (int)c->cells_h.size();
        // FAST segments (k_fast_seg): each cell row's cells in runs of at most
        // FS_SEGC whose ROI union (plus up to 15 bytes of alignment) fits the
        // FS_RS-byte LDS row, split evenly; the segment's ROI union is
        // cells_h[ci0 .. ci0 + ncell) (pushed above in row-major order)
        {
            const int nct = L.cell_end - L.cell_begin;
            int ncj = 0;  // cells per row (the skipped columns are the last ones)
            for (int j = 0; j < nCols; j++)
                if ((float)(minBorderX + j * wCell) < (float)(maxBorderX - 6)) ncj++;
            if (ncj > 0 && nct % ncj == 0) {
                const int kmax = std::min(FS_SEGC, (FS_RS - 15 - 6) / wCell);
                if (kmax < 1) return fail(ODO_ERR_ARG, "FAST cell wider than a segment row");
                const int nrow = nct / ncj, nseg = (ncj + kmax - 1) / kmax;
                for (int ir = 0; ir < nrow; ir++)
                    for (int sg = 0; sg < nseg; sg++) {
                        const int ja = ncj * sg / nseg, jb = ncj * (sg + 1) / nseg;
                        const CellDesc& A = c->cells_h[L.cell_begin + ir * ncj + ja];
                        const CellDesc& B = c->cells_h[L.cell_begin + ir * ncj + jb - 1];
                        FastSeg G{};
                        G.level = l;
                        G.ci0 = L.cell_begin + ir * ncj + ja;
                        G.y0 = A.y0;
                        G.rows = A.rows;
                        G.x0 = A.x0;
                        G.cols = (int16_t)(B.x0 + B.cols - A.x0);
                        G.ncell = (int16_t)(jb - ja);
                        G.wcell = (int16_t)wCell;
                        G.bw = (int16_t)((G.cols + 31) >> 5);
                        if ((A.x0 & 15) + G.cols > FS_RS || G.ncell > FS_NCM || G.rows > 70 || (int)G.rows * FS_RS > 65536)
                            return fail(ODO_ERR_ARG, "FAST segment too large");
                        fast_seg_staging(G);
                        c->fsegs_h.push_back(G);
                    }
            } else if (nct > 0) {
                return fail(ODO_ERR_STATE, "FAST cells not a full grid");
            }
        }
        L.key_off = (int)key_off;
        const int nIni = (int)roundf((float)(maxBorderX - minBorderX) / (float)(maxBorderY - minBorderY));
        max_nini = std::max(max_nini, nIni);
        const int tiles = ((L.w + 63) / 64) * ((L.h + 15) / 16);
        max_tiles = std::max(max_tiles, tiles);
    }
    c->ncells = (int)c->cells_h.size();
    c->cell_cap = (c->cell_cap + 3) & ~3;
    for (int l = 0; l < p.nlevels; l++) {
        LevelDesc& L = c->lv_h[l];
        L.key_off = 0;
    }
    size_t koff = 0;
    for (int l = 0; l < p.nlevels; l++) {
        c->lv_h[l].key_off = (int)koff;
        koff += (size_t)(c->lv_h[l].cell_end - c->lv_h[l].cell_begin) * c->cell_cap;
    }
    c->keys_per_frame = koff;
    c->pyr_size = (size_t)off + 64;  // tail: 16-byte staging loads may run past the last row
    c->max_blur_tiles = max_tiles;
    c->okp_stride = maxq + 8;
    int nc = 64;
    while (nc < std::max(maxq + 8, 4 * max_nini + 8)) nc <<= 1;
    c->node_cap = nc;
    if (octree_lds_bytes(nc) > 160 * 1024) return fail(ODO_ERR_ARG, "octree node capacity exceeds LDS");
    c->kp_cap = ((p.nfeatures + 4 * p.nlevels + 8) + 63) & ~63;
    if (c->kp_cap > 8192) return fail(ODO_ERR_ARG, "nfeatures too large (kp cap 8192)");
    if (c->adaptive) {
        int e;
        if ((e = build_adaptive_geometry(c))) return e;
        // the ADAPTIVE keypoint capacity (cells x per-cell maximum) may exceed
        // the cap checked above: the LDS landmark bit sets of k_vo_lm /
        // k_pair_match and the 13-bit train index of the kNN-2 keys hold 8192
        if (c->kp_cap > 8192) return fail(ODO_ERR_ARG, "ADAPTIVE max_total_keypoints too large (kp cap 8192)");
    }
    c->match_cap = c->kp_cap;
    c->mask_words = (c->match_cap + 31) / 32;
    // resize tables (cv::resize generic INTER_LINEAR, App. A.2)
    std::vector<ResizeX> rx;
    std::vector<ResizeY> ry;
    c->rx_off.assign(p.nlevels, 0);
    c->ry_off.assign(p.nlevels, 0);
    c->rz_rows.assign(p.nlevels, 0);
    for (int l = 1; l < p.nlevels; l++) {
        const LevelDesc& S = c->lv_h[l - 1];
        const LevelDesc& D = c->lv_h[l];
        const double inv_sx = (double)D.w / S.w, inv_sy = (double)D.h / S.h;
        const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
        c->rx_off[l] = (int)rx.size();
        std::vector<int> xofs(D.w);
        std::vector<int> a0(D.w), a1(D.w);
        int xmax = D.w;
        for (int dx = 0; dx < D.w; dx++) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = cvFloorH(fx);
            fx -= sx;
            if (sx < 0) {
                fx = 0;
                sx = 0;
            }
            if (sx + 1 >= S.w) {
                xmax = std::min(xmax, dx);
                if (sx >= S.w - 1) {
                    fx = 0;
                    sx = S.w - 1;
                }
            }
            xofs[dx] = sx;
            a0[dx] = satShort((1.f - fx) * 2048);
            a1[dx] = satShort(fx * 2048);
        }
        for (int dx = 0; dx < D.w; dx++) {
            ResizeX X;
            X.sx0 = xofs[dx];
            if (dx < xmax) {
                X.sx1 = xofs[dx] + 1;
                X.a0 = a0[dx];
                X.a1 = a1[dx];
            } else {
                X.sx1 = xofs[dx];
                X.a0 = 2048;
                X.a1 = 0;
            }
            rx.push_back(X);
        }
        c->ry_off[l] = (int)ry.size();
        for (int dy = 0; dy < D.h; dy++) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = cvFloorH(fy);
            fy -= sy;
            ResizeY Y;
            Y.b0 = satShort((1.f - fy) * 2048);
            Y.b1 = satShort(fy * 2048);
            Y.sy0 = std::min(std::max(sy, 0), S.h - 1);
            Y.sy1 = std::min(std::max(sy + 1, 0), S.h - 1);
            ry.push_back(Y);
        }
        // source rows one band of RZ_RB output rows stages in LDS
        int mr = 1;
        for (int y0 = 0; y0 < D.h; y0 += RZ_RB) {
            const int y1 = std::min(y0 + RZ_RB, D.h) - 1;
            mr = std::max(mr, ry[c->ry_off[l] + y1].sy1 - ry[c->ry_off[l] + y0].sy0 + 1);
        }
        c->rz_rows[l] = mr;
        if (resize_lds_bytes(S.pitch, D.w, mr) > 64 * 1024) return fail(ODO_ERR_ARG, "image too wide for the resize band");
    }
    c->pform = c->cfg.forms.pyramid;
    if (const char* e = odo_knob("ODO_PYRAMID_FORM")) c->pform = atoi(e);  // tuning build: A/B without a config change
    c->pyr_fusable = pyramid_fusable(c->lv_h.data(), rx.data(), c->rx_off.data(), p.nlevels);
    c->blur_fusable = c->pyr_fusable && pyramid_blur_fusable(c->lv_h.data(), p.nlevels);
    int e;
    if ((e = c->pool.alloc(&c->lv, c->lv_h.size()))) return e;
    if ((e = c->pool.alloc(&c->cells, c->cells_h.size()))) return e;
    if ((e = c->pool.alloc(&c->rx, rx.size()))) return e;
    if ((e = c->pool.alloc(&c->ry, ry.size()))) return e;
    HIPCHK(hipMemcpy(c->lv, c->lv_h.data(), c->lv_h.size() * sizeof(LevelDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->cells, c->cells_h.data(), c->cells_h.size() * sizeof(CellDesc), hipMemcpyHostToDevice));
    if (!fast_lds_plan(c->fsegs_h.data(), (int)c->fsegs_h.size(), c->fs_lds))
        return fail(ODO_ERR_ARG, "FAST segments exceed LDS");
    if ((e = c->pool.alloc(&c->fsegs, std::max<size_t>(c->fsegs_h.size(), 1)))) return e;
    if (!c->fsegs_h.empty())
        HIPCHK(hipMemcpy(c->fsegs, c->fsegs_h.data(), c->fsegs_h.size() * sizeof(FastSeg), hipMemcpyHostToDevice));
    if (!rx.empty()) HIPCHK(hipMemcpy(c->rx, rx.data(), rx.size() * sizeof(ResizeX), hipMemcpyHostToDevice));
    if (!ry.empty()) HIPCHK(hipMemcpy(c->ry, ry.data(), ry.size() * sizeof(ResizeY), hipMemcpyHostToDevice));
    c->ry_h = ry;
    return ODO_OK;
}
