// C-ABI (include/odo.h) of the MI355X odometry path: the context's lifetime.
//
// A context owns all HBM scratch sized for max_batch frames, the per-image-size
// geometry tables (pyramid levels, FAST cells, resize coefficients) and the
// cross-frame state the reference keeps in globals: the previous frame
// (Tracking::mpLastFrame) and the DepthCovariance latch. Here: create /
// destroy / reset, buffer allocation, the mode and timing setters, the getters
// and odo_debug_*.
#include "odo_ctx.h"

thread_local std::string odo::g_err;

int odo::sync_all(odo_ctx* c) {
    for (hipStream_t st : c->owned) HIPCHK(hipStreamSynchronize(st));
    c->depth_busy = false;
    return ODO_OK;
}

int odo::stage_reserve(odo_ctx* c, size_t bytes) {
    // this buffer's own policy: at least doubled, at least 1 MiB
    return c->stage.reserve(bytes, std::max(c->stage.cap * 2, (size_t)1 << 20), "staging");
}

// ADAPTIVE_RICP scratch (odo_set_odometry): a pair's cloud has at most match_cap
// points; sizes as launch_gicp documents them
static int alloc_ricp(odo_ctx* c) {
    const size_t B = (size_t)c->maxb, N = B * c->match_cap;
    int e;
    for (auto& R : c->rb) {
        DevPool& P = R.pool;
        if ((e = P.alloc(&R.src, N * 3)) || (e = P.alloc(&R.tgt, N * 3)) || (e = P.alloc(&R.outp, N * 3))) return e;
        if ((e = P.alloc(&R.Cs, N * 9)) || (e = P.alloc(&R.Ct, N * 9)) || (e = P.alloc(&R.Mah, N * 9))) return e;
        if ((e = P.alloc(&R.is, N)) || (e = P.alloc(&R.it, N))) return e;
        if ((e = P.alloc(&R.guess, B * 16)) || (e = P.alloc(&R.gT, B * 16)) || (e = P.alloc(&R.gio, B * 4))) return e;
        if ((e = P.alloc(&R.offs, B + 1)) || (e = P.alloc(&R.branch, B)) || (e = P.alloc(&R.rec, B))) return e;
    }
    return ODO_OK;
}

static int alloc_buffers(odo_ctx* c) {
    const size_t S = NSETS * (size_t)c->slots, B = (size_t)c->maxb;
    const size_t KC = (size_t)c->kp_cap;
    DevPool& D = c->pool;
    int e;
    if ((e = D.alloc(&c->pyr, S * c->pyr_size)) || (e = D.alloc(&c->blur, S * c->pyr_size))) return e;
    if ((e = D.alloc(&c->cand, S * c->ncells * c->cell_cap)) || (e = D.alloc(&c->cand_cnt, S * c->ncells))) return e;
    if ((e = D.alloc(&c->keys, S * c->keys_per_frame)) || (e = D.alloc(&c->knode, S * c->keys_per_frame))) return e;
    if ((e = D.alloc(&c->okp, S * c->nlevels * c->okp_stride)) || (e = D.alloc(&c->ocnt, S * c->nlevels))) return e;
    if ((e = D.alloc(&c->kps, S * KC)) || (e = D.alloc(&c->desc, S * KC * 32)) || (e = D.alloc(&c->kun, S * KC * 2))) return e;
    if ((e = D.alloc(&c->xyz, S * KC * 3)) || (e = D.alloc(&c->ur, S * KC)) || (e = D.alloc(&c->nkp, S))) return e;
    for (int i = 0; i < 2; i++)
        if ((e = D.alloc(&c->bgr_in[i], B * c->W * c->H * 3)) || (e = D.alloc(&c->depth_in[i], B * c->W * c->H))) return e;
    c->lm_words = (c->kp_cap + 31) / 32;
    // kernel forms (odo_config.forms; all bit-identical)
    if (c->cfg.forms.knn_split > 0) c->knn_split = std::min(8, c->cfg.forms.knn_split);
    c->knn_mx = c->cfg.forms.knn != ODO_KNN_FORM_VALU;
    if (const char* ks = odo_knob("ODO_KNN_SPLIT")) c->knn_split = std::min(8, std::max(1, atoi(ks)));
    if (c->knn_mx) c->knn_split = 1;  // one top-2 slot per query
    for (int i = 0; i < NSETS; i++) {
        const size_t nk = (size_t)c->knn_split * B * KC;
        if ((e = D.alloc(&c->knn_idx[i], nk)) || (e = D.alloc(&c->knn_dist[i], nk))) return e;
        if ((e = D.alloc(&c->lm_bits[i], B * c->lm_words)) || (e = D.alloc(&c->qlist[i], B * KC))) return e;
        if ((e = D.alloc(&c->qcnt[i], B))) return e;
    }
    for (auto& P : c->pb) {
        if ((e = D.alloc(&P.matches, B * c->match_cap)) || (e = D.alloc(&P.n_matches, B))) return e;
        if ((e = D.alloc(&P.n_good, B)) || (e = D.alloc(&P.pair_valid, B))) return e;
        if ((e = D.alloc((uint64_t**)&P.good, B * c->match_cap)) || (e = D.alloc(&P.f2_src, B * KC))) return e;
        if ((e = D.alloc(&P.best_mask, B * c->mask_words)) || (e = D.alloc(&P.res, B)) || (e = D.alloc(&P.T12, B * 16))) return e;
        if ((e = D.alloc((uint8_t**)&P.edges, B * KC * pnp_edge_bytes())) || (e = D.alloc(&P.pnp_mask, B * KC))) return e;
    }
    int pw = 1;
    while (pw < c->kp_cap) pw <<= 1;
    if ((e = D.alloc(&c->sort_scratch, B * std::max(pw, c->kp_cap))) || (e = D.alloc(&c->latch, 1))) return e;
    for (int i = 0; i < NSETS; i++)
        if ((e = D.alloc((uint8_t**)&c->rscr[i], ransac_scratch_bytes((int)B, c->match_cap, c->mask_words, c->rcfg)))) return e;
    if (c->adaptive) {
        const size_t nc = (size_t)c->ad_ncells;
        if ((e = D.alloc(&c->atsel, B * nc)) || (e = D.alloc(&c->ansel, B * nc))) return e;
        if ((e = D.alloc(&c->acell_cnt, B * nc)) || (e = D.alloc(&c->athresh, nc))) return e;
        if (!c->adaptive_orb) {
            c->smap_stride = (size_t)c->lv_h[0].pitch * c->H;
            if ((e = D.alloc(&c->smap, B * c->smap_stride)) || (e = D.alloc(&c->acand, B * c->acand_stride))) return e;
            if ((e = D.alloc(&c->aband_cnt, B * std::max(c->ad_nbands, 1))) || (e = D.alloc(&c->ahist, B * nc * 256))) return e;
            if ((e = D.alloc(&c->abig, B * nc * c->abig_stride)) || (e = D.alloc(&c->acell, B * nc * c->ad_mpc))) return e;
            if ((e = D.alloc(&c->akp, B * KC))) return e;
        } else {
            const size_t ni = c->oai_h.size();
            if ((e = D.alloc(&c->cpyr, B * c->cp_stride)) || (e = D.alloc(&c->ocand, B * c->ocand_stride))) return e;
            if ((e = D.alloc(&c->oband_cnt, B * std::max<size_t>(c->oab_h.size(), 1)))) return e;
            if ((e = D.alloc(&c->ohist, B * ni * 256)) || (e = D.alloc(&c->ophist, B * nc * 256))) return e;
            if ((e = D.alloc(&c->oscr, B * nc * c->oscr_stride)) || (e = D.alloc(&c->ocell, B * nc * c->ad_mpc))) return e;
            if ((e = D.alloc(&c->oakp, B * KC))) return e;
        }
        if ((e = reset_adaptive(c))) return e;
    }
    HIPCHK(hipHostMalloc((void**)&c->h_open, NSETS * sizeof(int), hipHostMallocDefault));
    for (int i = 0; i < NSETS; i++) c->h_open[i] = -1;  // unknown: the first RANSAC launch runs both forms
    HIPCHK(hipHostMalloc((void**)&c->latch_set_h, sizeof(int), hipHostMallocCoherent));
    *c->latch_set_h = 0;
    HIPCHK(hipMemset(c->nkp, 0, S * sizeof(int)));
    const double nan = std::nan("");
    HIPCHK(hipMemcpy(c->latch, &nan, sizeof(double), hipMemcpyHostToDevice));
    return ODO_OK;
}

// fold the elapsed time of ring slot i into the running sum (waits for it)
int odo::kt_collect(odo_ctx* c, int i) {
    HIPCHK(hipEventSynchronize(c->kt1[i]));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, c->kt0[i], c->kt1[i]));
    c->kt_sum_ms += t;
    c->kt_count++;
    float m = 0;
    HIPCHK(hipEventElapsedTime(&m, c->kt_ref, c->kt0[i]));
    c->kt_marks.push_back(m);
    return ODO_OK;
}

extern "C" {

const char* odo_last_error(void) { return g_err.c_str(); }

int odo_abi_version(void) { return ODO_ABI_VERSION; }

void odo_default_config(odo_config* cfg, int width, int height, int max_batch) {
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(odo_config);
    cfg->width = width;
    cfg->height = height;
    cfg->max_batch = max_batch;
    cfg->orb = odo_orb_params{1000, 1.2f, 8, 20, 7};
    cfg->calib = odo_calib{517.3f, 516.5f, 318.6f, 255.3f, 0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f,
                           1.0f / 5000.0f, 40.0f, 40.0f};
    cfg->nn_ratio = 0.9f;
    cfg->ransac = odo_ransac_params{200, 20, 3.0f, 4, 1};
    cfg->seed = 0x5EED0000u;
    cfg->detector = ODO_DETECTOR_ORB_SLAM2;
    // Extractor::CreateAdaptiveDetector (extractor.cpp:55-77): minFeatures 600,
    // maxFeatures = 600 * 1.7 = 1020, 3x3 grid, gridMin = round(600/9.f) = 67,
    // gridMax = round(1020/9.f) = 113, 5 iterations, edge 31; FAST adjuster
    // (20, 2, 10000, 1.3, 0.7); Extract's retainBest(nFeatures = 1000)
    cfg->adaptive = odo_adaptive_params{3, 3, 31, 1020, 67, 113, 5, 20.0, 2.0, 10000.0, 1.3, 0.7, 1000};
}

odo_ctx* odo_create(const odo_config* cfg, int device) {
    if (cfg && cfg->struct_size != (uint32_t)sizeof(odo_config)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "odo_config.struct_size %u != %zu: the caller was built against another odo.h "
                 "(ODO_ABI_VERSION %d); fill it with odo_default_config", cfg->struct_size, sizeof(odo_config),
                 ODO_ABI_VERSION);
        fail(ODO_ERR_ARG, msg);
        return nullptr;
    }
    if (!cfg || cfg->width <= 0 || cfg->height <= 0 || cfg->max_batch <= 0 || cfg->orb.nlevels <= 0 ||
        cfg->orb.nlevels > 16) {
        fail(ODO_ERR_ARG, "invalid config");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
        fail(ODO_ERR_DEVICE, "no HIP device available (the MI355X path has no CPU fallback)");
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(ODO_ERR_DEVICE, std::string("device is not gfx950: ") + prop.gcnArchName);
        return nullptr;
    }
    hipSetDevice(device);
    const char* bad = nullptr;
    if (cfg->forms.knn != ODO_KNN_FORM_FP4 && cfg->forms.knn != ODO_KNN_FORM_VALU) bad = "unknown kNN-2 kernel form";
    else if (cfg->forms.pyramid < ODO_PYRAMID_FORM_AUTO || cfg->forms.pyramid > ODO_PYRAMID_FORM_FUSED)
        bad = "unknown pyramid kernel form";
    else if (cfg->forms.ransac_first_hyps < 0 || cfg->forms.ransac_first_hyps > 64)
        bad = "ransac_first_hyps: 0 (default) or 1..64";
    else if (cfg->detector != ODO_DETECTOR_ORB_SLAM2 && cfg->detector != ODO_DETECTOR_ADAPTIVE_FAST &&
             cfg->detector != ODO_DETECTOR_ADAPTIVE_ORB)
        bad = "unsupported detector";  // extractor.cpp:26-27 terminates here
    if (bad) {
        fail(ODO_ERR_ARG, bad);
        return nullptr;
    }
    odo_ctx* c = new odo_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->W = cfg->width;
    c->H = cfg->height;
    c->maxb = cfg->max_batch;
    c->slots = cfg->max_batch + 1;
    c->adaptive = cfg->detector == ODO_DETECTOR_ADAPTIVE_FAST || cfg->detector == ODO_DETECTOR_ADAPTIVE_ORB;
    c->adaptive_orb = cfg->detector == ODO_DETECTOR_ADAPTIVE_ORB;
    // ODO_SERIAL_STREAMS=1 (profiling): every stage on one stream, no overlap,
    // so per-kernel times are free of cross-stream contention
    const char* ser = odo_knob("ODO_SERIAL_STREAMS");
    c->serial = ser && ser[0] == '1';
    if (const char* sk = odo_knob("ODO_SKIP")) c->skip = atoi(sk);
    // Every stream runs at the default priority: measured on MI355X, giving
    // the pair streams the highest priority starves the extraction stream and
    // costs 17% throughput (1.63 vs 1.35 ms per 64-frame step).
    auto mk = [&](hipStream_t* s) {
        const bool r = hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess;
        if (r) c->owned.push_back(*s);
        return r;
    };
    bool ok = mk(&c->stream);
    if (ok && c->serial)
        c->pstream = c->pstream2 = c->stream;
    else if (ok)
        ok = mk(&c->pstream) && mk(&c->pstream2);
    auto mkev = [&](hipEvent_t* e) { return c->make_event(e, SYNC_EVENT_FLAGS) == hipSuccess; };
    for (int i = 0; i < NSETS && ok; i++) ok = mkev(&c->ev_pnp_done[i]) && mkev(&c->ev_xdone[i]) && mkev(&c->ev_geo[i]);
    if (ok) ok = mkev(&c->ev_latch);
    if (ok) ok = mkev(&c->ev_depth_done);
    // host-input uploads run on their own stream (the DMA engines), ordered
    // against the extraction stream by events only
    if (ok) ok = mk(&c->cstream);
    for (int i = 0; i < 2 && ok; i++) ok = mkev(&c->ev_in_copied[i]) && mkev(&c->ev_in_free[i]);
    if (!ok) {
        fail(ODO_ERR_DEVICE, "hipStreamCreate failed");
        delete c;
        return nullptr;
    }
    c->rcfg = ransac_cfg(cfg->ransac, cfg->forms);
    if (build_geometry(c) != ODO_OK || alloc_buffers(c) != ODO_OK) {
        delete c;
        return nullptr;
    }
    c->cal = frame_calib(cfg->calib);
    c->nev = 11;
    for (int i = 0; i < c->nev; i++) (void)c->make_event(&c->ev[i], hipEventDefault);
    return c;
}

void odo_destroy(odo_ctx* ctx) { delete ctx; }

void* odo_stream(odo_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int odo_reset(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    int e;
    if ((e = sync_all(c))) return e;
    c->has_prev = false;
    c->pair_counter = 0;
    const double nan = std::nan("");
    HIPCHK(hipMemcpy(c->latch, &nan, sizeof(double), hipMemcpyHostToDevice));
    if (c->latch_set_h) *c->latch_set_h = 0;
    return reset_adaptive(c);
}

void odo_default_ricp_params(odo_ricp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    // odometry.cpp:52-53 and GeneralizedICP(10, 0.07), odometry.cpp:15
    p->min_inliers = 20;
    p->rmse_scale = 10.0f;
    p->refine_at = 7.0f;
    p->reset_at = 20.0f;
    p->gicp_iterations = 10;
    p->gicp_max_corr_dist = 0.07;
}

int odo_set_odometry(odo_ctx* c, int mode, const odo_ricp_params* p) {
    // the argument checks come first and touch no device (nor the context)
    if (mode != ODO_ODOMETRY_ADAPTIVE_RBA && mode != ODO_ODOMETRY_RANSAC && mode != ODO_ODOMETRY_ADAPTIVE_RICP)
        return fail(ODO_ERR_ARG, "unknown odometry mode");
    odo_ricp_params rp;
    odo_default_ricp_params(&rp);
    if (p) rp = *p;
    if (rp.gicp_iterations < 1) return fail(ODO_ERR_ARG, "ricp: gicp_iterations < 1");
    if (!(rp.gicp_max_corr_dist > 0) || !std::isfinite(rp.gicp_max_corr_dist))
        return fail(ODO_ERR_ARG, "ricp: gicp_max_corr_dist must be positive and finite");
    if (!std::isfinite(rp.rmse_scale) || !std::isfinite(rp.refine_at) || !std::isfinite(rp.reset_at))
        return fail(ODO_ERR_ARG, "ricp: non-finite threshold");
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    // brute-force neighbour searches in one workgroup (gicp_run's limit)
    if (mode == ODO_ODOMETRY_ADAPTIVE_RICP && c->match_cap > 16384)
        return fail(ODO_ERR_CAPACITY, "ricp: more than 16384 points in a cloud");
    int e;
    if ((e = sync_all(c))) return e;
    if (mode == ODO_ODOMETRY_ADAPTIVE_RICP && c->rb[0].pool.slots.empty() && (e = alloc_ricp(c))) {
        // all or nothing: the mode stays as it was, a later switch allocates afresh
        for (auto& R : c->rb) R.pool.release();
        return e;
    }
    c->ricp = rp;
    c->odo_mode = mode;
    return ODO_OK;
}

int odo_get_odometry(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    return c->odo_mode;
}

int odo_get_ricp(odo_ctx* c, int i, odo_ricp_result* r, float* src, float* tgt, int cap) {
    if (!c || !r || cap < 0) return fail(ODO_ERR_ARG, "bad get_ricp args");
    if (c->view_mode != ODO_ODOMETRY_ADAPTIVE_RICP) return fail(ODO_ERR_STATE, "the last batch did not run in ADAPTIVE_RICP");
    if (i < 0 || i >= c->last_n) return fail(ODO_ERR_ARG, "bad pair index");
    int e;
    if ((e = sync_all(c))) return e;
    auto& R = c->rb[c->view_rb];
    int o[2] = {0, 0};
    HIPCHK(hipMemcpy(r, R.rec + i, sizeof(*r), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(o, R.offs + i, sizeof(o), hipMemcpyDeviceToHost));
    const int len = o[1] - o[0], m = std::min(len, cap);
    if (len < 0 || o[0] < 0 || (size_t)o[1] > (size_t)c->maxb * c->match_cap)
        return fail(ODO_ERR_STATE, "ricp: cloud offsets out of range");
    if (src && m > 0) HIPCHK(hipMemcpy(src, R.src + 3 * (size_t)o[0], (size_t)m * 12, hipMemcpyDeviceToHost));
    if (tgt && m > 0) HIPCHK(hipMemcpy(tgt, R.tgt + 3 * (size_t)o[0], (size_t)m * 12, hipMemcpyDeviceToHost));
    return (src || tgt) && len > cap ? fail(ODO_ERR_CAPACITY, "cap too small") : ODO_OK;
}

int odo_set_latch(odo_ctx* c, double cov) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    int e;
    if ((e = sync_all(c))) return e;
    HIPCHK(hipMemcpy(c->latch, &cov, sizeof(double), hipMemcpyHostToDevice));
    if (c->latch_set_h) *c->latch_set_h = std::isnan(cov) ? 0 : 1;
    return ODO_OK;
}

double odo_get_latch(odo_ctx* c) {
    double v = std::nan("");
    if (!c || sync_all(c)) return v;
    hipMemcpy(&v, c->latch, sizeof(double), hipMemcpyDeviceToHost);
    return v;
}

int odo_set_timing(odo_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return fail(ODO_ERR_ARG, "bad timing mode");
    int e;
    if ((e = sync_all(c))) return e;
    c->timing = mode == 1;
    c->ktiming = mode == 2;
    if (c->ktiming) {
        // timing only: no system-scope fence at the records (see SYNC_EVENT_FLAGS)
        const unsigned tf = hipEventDisableSystemFence;
        if (!c->kt0[0])
            for (int i = 0; i < odo_ctx::KT_RING; i++)
                if (c->make_event(&c->kt0[i], tf) != hipSuccess || c->make_event(&c->kt1[i], tf) != hipSuccess)
                    return fail(ODO_ERR_DEVICE, "hipEventCreate failed");
        c->kt_next = c->kt_pending = 0;
        c->kt_sum_ms = 0;
        c->kt_count = 0;
        if (!c->kt_ref && c->make_event(&c->kt_ref, tf) != hipSuccess)
            return fail(ODO_ERR_DEVICE, "hipEventCreate failed");
        HIPCHK(hipEventRecord(c->kt_ref, c->stream));  // every stream is idle (sync_all above)
        c->kt_marks.clear();
    }
    return ODO_OK;
}


int odo_kernel_timing(odo_ctx* c, double* avg_ms, long* launches) {
    if (!c || !avg_ms || !launches) return fail(ODO_ERR_ARG, "null arg");
    if (!c->ktiming) return fail(ODO_ERR_ARG, "kernel timing is off (odo_set_timing mode 2)");
    int e;
    if ((e = sync_all(c))) return e;
    const int n = c->kt_pending;
    for (int k = 0; k < n; k++) {
        const int i = (c->kt_next - n + k + odo_ctx::KT_RING) % odo_ctx::KT_RING;
        if ((e = kt_collect(c, i))) return e;
    }
    c->kt_pending = 0;
    *launches = c->kt_count;
    *avg_ms = c->kt_count ? c->kt_sum_ms / (double)c->kt_count : 0.0;
    return ODO_OK;
}

// The kNN-2 launch of batch b starts once b's extraction has finished (and
// its pair stream is free): the marks' differences are the pipeline's
// per-step times, read without adding any event to the extraction stream.
int odo_step_marks(odo_ctx* c, double* ms, int cap) {
    if (!c || cap < 0 || (cap > 0 && !ms)) return fail(ODO_ERR_ARG, "step_marks: bad arguments");
    double avg = 0;
    long n = 0;
    int e;
    if ((e = odo_kernel_timing(c, &avg, &n))) return e;  // collects the pending marks
    const int k = (int)c->kt_marks.size();
    for (int i = 0; i < k && i < cap; i++) ms[i] = c->kt_marks[i];
    return k;
}

int odo_synchronize(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    return sync_all(c);
}

int odo_get_frame(odo_ctx* c, int i, orb_kp* kps, uint8_t* desc, float* kps_un, float* xyz, float* u_right, int cap,
                  int* n) {
    if (!c || i < 0 || i >= c->last_n) return fail(ODO_ERR_ARG, "bad frame index");
    int e;
    if ((e = sync_all(c))) return e;
    // frame i of the last batch: slot i+1 of its frame set
    const FrameSlot f = frame_at(c, fbase(c, c->view_set) + i + 1);
    // every array at its full capacity (no round trip for the count first):
    // async copies into the pinned staging buffer, one sync, then the
    // caller's buffers
    const size_t KC = (size_t)c->kp_cap;
    Pack pk;
    const size_t o_n = pk.add(sizeof(int)), o_k = pk.add(KC * sizeof(orb_kp)), o_d = pk.add(KC * 32),
                 o_u = pk.add(KC * 8), o_x = pk.add(KC * 12), o_r = pk.add(KC * 4);
    if ((e = stage_reserve(c, pk.off))) return e;
    uint8_t* h = c->stage.p;
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(h + o_n, f.nkp, sizeof(int), hipMemcpyDeviceToHost, st));
    if (kps) HIPCHK(hipMemcpyAsync(h + o_k, f.kps, KC * sizeof(orb_kp), hipMemcpyDeviceToHost, st));
    if (desc) HIPCHK(hipMemcpyAsync(h + o_d, f.desc, KC * 32, hipMemcpyDeviceToHost, st));
    if (kps_un) HIPCHK(hipMemcpyAsync(h + o_u, f.kun, KC * 8, hipMemcpyDeviceToHost, st));
    if (xyz) HIPCHK(hipMemcpyAsync(h + o_x, f.xyz, KC * 12, hipMemcpyDeviceToHost, st));
    if (u_right) HIPCHK(hipMemcpyAsync(h + o_r, f.ur, KC * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int cnt = 0;
    memcpy(&cnt, h + o_n, sizeof(int));
    *n = cnt;
    const int m = std::max(0, std::min(cnt, cap));
    if (kps) memcpy(kps, h + o_k, (size_t)m * sizeof(orb_kp));
    if (desc) memcpy(desc, h + o_d, (size_t)m * 32);
    if (kps_un) memcpy(kps_un, h + o_u, (size_t)m * 8);
    if (xyz) memcpy(xyz, h + o_x, (size_t)m * 12);
    if (u_right) memcpy(u_right, h + o_r, (size_t)m * 4);
    return cnt > cap ? fail(ODO_ERR_CAPACITY, "cap too small") : ODO_OK;
}

int odo_get_pair(odo_ctx* c, int i, odo_dmatch* matches, int match_cap, int* n_matches, odo_dmatch* good_sorted,
                 int* n_good, uint8_t* ransac_inliers, uint8_t* pnp_inliers, int32_t* f2_src) {
    if (!c || i < 0 || i >= c->last_n) return fail(ODO_ERR_ARG, "bad pair index");
    int e;
    if ((e = sync_all(c))) return e;
    int nm = 0, ng = 0, n2 = 0;
    auto& P = c->pb[c->view_set];
    HIPCHK(hipMemcpy(&nm, P.n_matches + i, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ng, P.n_good + i, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&n2, frame_at(c, fbase(c, c->view_set) + i + 1).nkp, sizeof(int), hipMemcpyDeviceToHost));
    if (n_matches) *n_matches = nm;
    if (n_good) *n_good = ng;
    std::vector<odo_dmatch> M(std::max(nm, 1));
    HIPCHK(hipMemcpy(M.data(), P.matches + (size_t)i * c->match_cap, nm * sizeof(odo_dmatch), hipMemcpyDeviceToHost));
    if (matches) memcpy(matches, M.data(), std::min(nm, match_cap) * sizeof(odo_dmatch));
    if (good_sorted || ransac_inliers) {
        std::vector<uint64_t> G(std::max(ng, 1));
        HIPCHK(hipMemcpy(G.data(), (uint64_t*)P.good + (size_t)i * c->match_cap, ng * sizeof(uint64_t),
                         hipMemcpyDeviceToHost));
        if (good_sorted)
            for (int k = 0; k < ng && k < match_cap; k++) good_sorted[k] = M[(uint32_t)(G[k] >> 32)];
        if (ransac_inliers) {
            std::vector<uint32_t> bm(c->mask_words);
            HIPCHK(hipMemcpy(bm.data(), P.best_mask + (size_t)i * c->mask_words, c->mask_words * 4,
                             hipMemcpyDeviceToHost));
            for (int k = 0; k < ng && k < match_cap; k++) ransac_inliers[k] = (bm[k >> 5] >> (k & 31)) & 1;
        }
    }
    if (pnp_inliers) HIPCHK(hipMemcpy(pnp_inliers, P.pnp_mask + (size_t)i * c->kp_cap, n2, hipMemcpyDeviceToHost));
    if (f2_src) HIPCHK(hipMemcpy(f2_src, P.f2_src + (size_t)i * c->kp_cap, n2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ODO_OK;
}

// levels back to back, rows compacted (the device layout pitches rows to 16 bytes)
static int copy_levels(odo_ctx* c, const uint8_t* dev, uint8_t* out, size_t cap) {
    size_t total = 0;
    for (auto& L : c->lv_h) total += (size_t)L.w * L.h;
    if (cap < total) return fail(ODO_ERR_ARG, "output buffer too small");
    std::vector<uint8_t> buf(c->pyr_size);
    HIPCHK(hipMemcpy(buf.data(), dev, c->pyr_size, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (auto& L : c->lv_h)
        for (int y = 0; y < L.h; y++, o += L.w) memcpy(out + o, buf.data() + L.off + (size_t)y * L.pitch, L.w);
    return (int)o;
}

int odo_debug_pyramid(odo_ctx* c, int i, uint8_t* out, size_t cap) {
    if (!c || i < 0 || i >= c->last_n || !out) return fail(ODO_ERR_ARG, "bad args");
    int e;
    if ((e = sync_all(c))) return e;
    return copy_levels(c, c->pyr + (fbase(c, c->view_set) + i + 1) * c->pyr_size, out, cap);
}

int odo_debug_blur(odo_ctx* c, int i, uint8_t* out, size_t cap) {
    if (!c || i < 0 || i >= c->last_n || !out) return fail(ODO_ERR_ARG, "bad args");
    int e;
    if ((e = sync_all(c))) return e;
    return copy_levels(c, c->blur + (fbase(c, c->view_set) + i + 1) * c->pyr_size, out, cap);
}

int odo_debug_adaptive(odo_ctx* c, int i, int32_t* t_used, double* thresh) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    if (!c->adaptive) return fail(ODO_ERR_STATE, "context is not in ADAPTIVE mode");
    if (t_used && (i < 0 || i >= c->last_n)) return fail(ODO_ERR_ARG, "bad frame index");
    int e;
    if ((e = sync_all(c))) return e;
    if (t_used)
        HIPCHK(hipMemcpy(t_used, c->atsel + (size_t)i * c->ad_ncells, c->ad_ncells * sizeof(int),
                         hipMemcpyDeviceToHost));
    if (thresh) HIPCHK(hipMemcpy(thresh, c->athresh, c->ad_ncells * sizeof(double), hipMemcpyDeviceToHost));
    return c->ad_ncells;
}

int odo_set_adaptive_thresholds(odo_ctx* c, const double* thresh, int n) {
    if (!c || !thresh) return fail(ODO_ERR_ARG, "bad args");
    if (!c->adaptive) return fail(ODO_ERR_STATE, "context is not in ADAPTIVE mode");
    if (n != c->ad_ncells) return fail(ODO_ERR_ARG, "threshold count != grid cells");
    int e;
    if ((e = sync_all(c))) return e;
    HIPCHK(hipMemcpy(c->athresh, thresh, n * sizeof(double), hipMemcpyHostToDevice));
    return ODO_OK;
}

int odo_debug_select(odo_ctx* c, const uint32_t* in, int n, int nth, int mode, uint32_t* out, int* n_out) {
    if (!c || n < 0 || (n && (!in || !out)) || !n_out || nth < 0 || (mode != 0 && mode != 1) || (mode == 1 && nth < 1))
        return fail(ODO_ERR_ARG, "bad select args");
    int e;
    if ((e = sync_all(c))) return e;
    if (n == 0) {
        *n_out = 0;
        return ODO_OK;
    }
    if (nth > n) nth = n;
    c->arena.begin();
    DevBuf d(c->arena, (size_t)n * 12 + 16);
    ARENA_CHECK(c->arena);
    uint32_t* A = d.as<uint32_t>();
    int* posL = (int*)(A + n);
    int* posR = posL + n;
    int* dn = posR + n;
    HIPCHK(hipMemcpy(A, in, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_adapt_select_dbg(c->stream, A, n, nth, mode, posL, posR, dn);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, A, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, dn, sizeof(int), hipMemcpyDeviceToHost));
    return ODO_OK;
}

// Measurement: re-run the most recent batch's kNN-2 launch `reps` times on one
// stream of an otherwise idle device (all streams drained first; same inputs,
// same outputs rewritten) and return the mean launch time from HIP events.
int odo_knn_replay_time(odo_ctx* c, int reps, float* avg_ms) {
    if (!c || !avg_ms || reps <= 0) return fail(ODO_ERR_ARG, "knn_replay_time: bad arguments");
    if (c->last_knn_set < 0) return fail(ODO_ERR_ARG, "knn_replay_time: no batch tracked yet");
    int e;
    if ((e = sync_all(c))) return e;
    // hipGetLastError is sticky per thread: an error left by an earlier call
    // is reported as that, not as a failure of the replay
    const hipError_t pending = hipGetLastError();
    if (pending != hipSuccess)
        return fail(ODO_ERR_DEVICE, std::string("knn_replay_time: HIP error pending from an earlier call: ") +
                                        hipGetErrorString(pending));
    const int s = c->last_knn_set, n = c->last_knn_n;
    hipStream_t st = c->stream;
    auto launch = [&]() { launch_set_knn2(c, st, s, n); };
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    launch();  // warm
    HIPCHK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; r++) launch();
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    HIPCHK(hipEventDestroy(e0));
    HIPCHK(hipEventDestroy(e1));
    HIPCHK(hipGetLastError());
    *avg_ms = ms / (float)reps;
    return ODO_OK;
}

int odo_debug_sort(odo_ctx* c, const odo_dmatch* in, int n, odo_dmatch* out) {
    if (!c || n < 0 || (n && (!in || !out))) return fail(ODO_ERR_ARG, "bad sort args");
    if (n > 8192) return fail(ODO_ERR_CAPACITY, "debug sort: at most 8192 elements");
    if (n == 0) return ODO_OK;
    std::vector<uint64_t> el(n);
    for (int i = 0; i < n; i++) {
        if (!(in[i].distance >= 0.f)) return fail(ODO_ERR_ARG, "debug sort: negative/NaN distance");
        uint32_t bits;
        memcpy(&bits, &in[i].distance, 4);
        el[i] = ((uint64_t)(uint32_t)i << 32) | bits;  // SortEl{key = distance bits, val = index}
    }
    c->arena.begin();
    DevBuf d(c->arena, (size_t)n * 8);
    ARENA_CHECK(c->arena);
    HIPCHK(hipMemcpy(d.p, el.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    if (launch_sort_dbg(c->stream, d.p, n) != 0) return fail(ODO_ERR_DEVICE, "debug sort: the launch refused its arguments");
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(el.data(), d.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) out[i] = in[(uint32_t)(el[i] >> 32)];
    return ODO_OK;
}

static orb_kp unpack_key(uint32_t k) {
    orb_kp r;
    r.x = (float)(k & 0xfff);
    r.y = (float)((k >> 12) & 0xfff);
    r.size = 7.f;
    r.angle = -1.f;
    r.response = (float)(k >> 24);
    r.octave = 0;
    r.class_id = -1;
    return r;
}

int odo_debug_fast(odo_ctx* c, int i, int level, orb_kp* out, int cap, int* n) {
    if (!c || i < 0 || i >= c->last_n || level < 0 || level >= c->nlevels) return fail(ODO_ERR_ARG, "bad args");
    int e;
    if ((e = sync_all(c))) return e;
    const size_t slot = fbase(c, c->view_set) + i + 1;
    const LevelDesc& L = c->lv_h[level];
    const int nc = L.cell_end - L.cell_begin;
    std::vector<int> cnt(nc);
    std::vector<uint32_t> cand((size_t)nc * c->cell_cap);
    HIPCHK(hipMemcpy(cnt.data(), c->cand_cnt + (size_t)slot * c->ncells + L.cell_begin, nc * sizeof(int),
                     hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cand.data(), c->cand + ((size_t)slot * c->ncells + L.cell_begin) * c->cell_cap,
                     cand.size() * 4, hipMemcpyDeviceToHost));
    int m = 0;
    for (int ci = 0; ci < nc; ci++)
        for (int k = 0; k < cnt[ci]; k++) {
            if (m < cap) out[m] = unpack_key(cand[(size_t)ci * c->cell_cap + k]);
            m++;
        }
    *n = m;
    return ODO_OK;
}

int odo_debug_octree(odo_ctx* c, int i, int level, orb_kp* out, int cap, int* n) {
    if (!c || i < 0 || i >= c->last_n || level < 0 || level >= c->nlevels) return fail(ODO_ERR_ARG, "bad args");
    int e;
    if ((e = sync_all(c))) return e;
    const size_t slot = fbase(c, c->view_set) + i + 1;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, c->ocnt + (size_t)slot * c->nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<uint32_t> k(std::max(cnt, 1));
    HIPCHK(hipMemcpy(k.data(), c->okp + ((size_t)slot * c->nlevels + level) * c->okp_stride, cnt * 4,
                     hipMemcpyDeviceToHost));
    for (int j = 0; j < cnt && j < cap; j++) out[j] = unpack_key(k[j]);
    *n = cnt;
    return ODO_OK;
}

int odo_last_timings(odo_ctx* c, float* ms, int cap, const char** names) {
    static const char* kNamesOrb[] = {"gray+pyramid", "fast", "octree", "blur", "finalize", "knn2", "match+sort",
                                      "ransac", "pnp"};
    // ADAPTIVE marks: gray | S map + band survivors | chain + select + assemble | blur L0 | finalize
    static const char* kNamesAd[] = {"gray", "smap+cand", "chain+select", "blur", "finalize", "knn2", "match+sort",
                                     "ransac", "pnp"};
    const char* const* kNames = c && c->adaptive ? kNamesAd : kNamesOrb;
    // stage i spans events (a[i], b[i]): extraction stream 0..5; pair stream 10, 6..9
    static const int a[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8}, b[9] = {1, 2, 3, 4, 5, 10, 7, 8, 9};
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    if (!c->timing) return fail(ODO_ERR_ARG, "stage timing is off (odo_set_timing)");
    int e;
    if ((e = sync_all(c))) return e;
    int m = 0;
    for (int i = 0; i < 9 && i < cap; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, c->ev[a[i]], c->ev[b[i]]) != hipSuccess) t = -1;
        ms[i] = t;
        if (names) names[i] = kNames[i];
        m++;
    }
    return m;
}

int odo_kp_capacity(odo_ctx* c) {
    if (!c) return fail(ODO_ERR_ARG, "null ctx");
    return c->kp_cap;
}

}  // extern "C"
