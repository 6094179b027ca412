// Single-pair RANSAC (Ransac::Iterate over one frame pair): odo_ransac and
// hypotheses mode (odo_ransac_hyps* / odo_ransac_fold_dev), which splits the
// hypotheses of one pair over ranks. Both prepare and upload the pair with
// the same code, so they agree bit for bit.
#include "odo_ctx.h"

namespace {

// Ransac::Iterate's inputs after the depth filter, std::sort and the latch
// (ransac.cpp:164-199), uploaded for the single-pair RANSAC kernels.
struct PairRansacInput {
    std::vector<odo_dmatch> good;
    int ng = 0, words = 0, kc = 1, n1 = 0, n2 = 0;
    RansacCfg cfg{};
};

// < 0: an error (its message set); 0: RANSAC does not run (too few matches /
// good matches: Iterate returns before sampling); 1: run
int prepare_pair_ransac(const odo_dmatch* m12, int n12, const float* xyz1, int n1, const float* xyz2, int n2,
                        const odo_ransac_params* p, double* latch, PairRansacInput& in, int match_cap) {
    if (n12 < p->min_inlier_th) return 0;
    // depth filter (ransac.cpp:175-189) and std::sort by distance (ransac.cpp:199)
    in.good.clear();
    in.good.reserve(n12);
    for (int i = 0; i < n12; i++) {
        const odo_dmatch& m = m12[i];
        if (m.queryIdx < 0 || m.queryIdx >= n1 || m.trainIdx < 0 || m.trainIdx >= n2)
            return fail(ODO_ERR_ARG, "match index out of range");
        const float zs = xyz1[3 * m.queryIdx + 2], zt = xyz2[3 * m.trainIdx + 2];
        if (p->check_depth) {
            if (std::isnan(zs) || std::isnan(zt)) continue;
            if (zs <= 0 || zt <= 0) continue;
        }
        in.good.push_back(m);
    }
    if ((int)in.good.size() < p->min_inlier_th) return 0;
    std::sort(in.good.begin(), in.good.end(),
              [](const odo_dmatch& a, const odo_dmatch& b) { return a.distance < b.distance; });
    in.ng = (int)in.good.size();
    if (in.ng > match_cap * 64) return fail(ODO_ERR_CAPACITY, "too many matches");
    if (std::isnan(*latch)) {  // DepthCovariance first-call latch (ransac.cpp:416-421)
        for (const odo_dmatch& m : in.good) {
            const float* o = &xyz1[3 * m.queryIdx];
            const float* tg = &xyz2[3 * m.trainIdx];
            if (o[2] == 0.0f || tg[0] == 0.0f) continue;  // tg[0], not tg[2]: as the reference tests it
            if (std::isnan(o[2]) || std::isnan(tg[2])) continue;
            const double z = (double)o[2];
            const double sd = 0.01 * z * z;
            *latch = sd * sd;
            break;
        }
    }
    in.n1 = n1;
    in.n2 = n2;
    in.kc = std::max(std::max(n1, n2), 1);
    in.words = (in.ng + 31) / 32;
    in.cfg = ransac_cfg(*p);
    return 1;
}

// A prepared pair's inputs in a packed buffer: xyz (two slots of kc points),
// the good matches, their (index << 32 | distance bits) sort keys,
// {n_good, n_matches, pair_valid, 0}, the latch, the rand() state. The
// caller's output sections follow.
struct PairSections {
    size_t xyz = 0, m = 0, g = 0, ints = 0, latch = 0, rng = 0;
};
PairSections add_pair(Pack& pk, const PairRansacInput& in) {
    PairSections o;
    o.xyz = pk.add((size_t)2 * in.kc * 12);
    o.m = pk.add((size_t)in.ng * sizeof(odo_dmatch));
    o.g = pk.add((size_t)in.ng * 8);
    o.ints = pk.add(4 * sizeof(int));
    o.latch = pk.add(sizeof(double));
    o.rng = pk.add(sizeof(odo_rng));
    return o;
}
void fill_pair(uint8_t* h, const PairSections& o, const PairRansacInput& in, const float* xyz1, const float* xyz2,
               const double* latch, const odo_rng* rng) {
    memcpy(h + o.xyz, xyz1, (size_t)in.n1 * 12);
    memcpy(h + o.xyz + (size_t)in.kc * 12, xyz2, (size_t)in.n2 * 12);
    memcpy(h + o.m, in.good.data(), (size_t)in.ng * sizeof(odo_dmatch));
    uint64_t* gl = reinterpret_cast<uint64_t*>(h + o.g);
    for (int k = 0; k < in.ng; k++) {
        uint32_t bits;
        memcpy(&bits, &in.good[k].distance, 4);
        gl[k] = ((uint64_t)(uint32_t)k << 32) | bits;
    }
    const int ints[4] = {in.ng, in.ng, 1, 0};
    memcpy(h + o.ints, ints, sizeof(ints));
    memcpy(h + o.latch, latch, sizeof(double));
    memcpy(h + o.rng, rng, sizeof(odo_rng));
}

// Ransac::mvInliers from the best hypothesis' bit mask; returns their number
int gather_inliers(const uint32_t* bm, const std::vector<odo_dmatch>& good, odo_dmatch* inliers) {
    int k2 = 0;
    for (int k = 0; k < (int)good.size(); k++)
        if ((bm[k >> 5] >> (k & 31)) & 1) {
            if (inliers) inliers[k2] = good[k];
            k2++;
        }
    return k2;
}
}  // namespace

// One block of the context's hyp_arena (this session's until the next
// session): the pair's sections, then the result record, T, the RANSAC
// scratch and the inlier mask.
struct odo::HypSession {
    PairRansacInput in;
    int h0 = 0, h1 = 0, active = 0;
    uint8_t* d = nullptr;
    PairSections o;
    size_t o_res = 0, o_T = 0, o_scr = 0, o_bm = 0;
    template <typename T>
    T* at(size_t off) const {
        return reinterpret_cast<T*>(d + off);
    }
    double* latch() const { return at<double>(o.latch); }
    odo_rng* rng() const { return at<odo_rng>(o.rng); }
    odo_pair_result* res() const { return at<odo_pair_result>(o_res); }
    float* T() const { return at<float>(o_T); }
    void* scr() const { return d + o_scr; }
    uint32_t* bm() const { return at<uint32_t>(o_bm); }
};
void odo::free_hyp_session(HypSession* h) { delete h; }

// Hypotheses mode, shared by the host and the device exchange: a new session
// over the pair, its samples for all H hypotheses and the evaluation of
// [h0, h1) queued on the context's stream (no fold). *active = 0 when
// Iterate returns before sampling (too few matches).
static int hyps_launch(odo_ctx* c, const odo_dmatch* m12, int n12, const float* xyz1, int n1, const float* xyz2,
                       int n2, const odo_ransac_params* p, const odo_rng* rng, double* latch, int h0, int h1,
                       int* n_good, int* active) {
    free_hyp_session(c->hs);
    c->hs = new HypSession();
    HypSession& S = *c->hs;
    S.h0 = h0;
    S.h1 = h1;
    *n_good = 0;
    *active = 0;
    const int r = prepare_pair_ransac(m12, n12, xyz1, n1, xyz2, n2, p, latch, S.in, c->match_cap);
    if (r <= 0) return r;
    S.active = 1;
    *active = 1;
    PairRansacInput& in = S.in;
    const int ng = in.ng;
    *n_good = ng;
    hipStream_t st = c->stream;
    // the previous session's kernels (queued asynchronously by _dev / _finish)
    // may still read the arena that begin() may free and replace
    HIPCHK(hipStreamSynchronize(st));
    Pack pk;
    S.o = add_pair(pk, in);
    const size_t up = S.o.rng + sizeof(odo_rng);
    S.o_res = pk.add(sizeof(odo_pair_result));
    S.o_T = pk.add(16 * sizeof(float));
    S.o_scr = pk.add(ransac_scratch_bytes(1, ng, in.words, in.cfg));
    S.o_bm = pk.add((size_t)in.words * 4);
    c->hyp_arena.begin();
    S.d = (uint8_t*)c->hyp_arena.take(pk.off);
    ARENA_CHECK(c->hyp_arena);
    // the inputs packed in page-locked memory in their device order: one DMA.
    // The previous session's upload must have left the buffer before it is
    // refilled.
    if (c->hyp_up_rec) HIPCHK(hipEventSynchronize(c->hyp_up));
    if (const int e = c->hyp_stage.reserve(up, (size_t)1 << 20, "hypotheses staging")) return e;
    if (!c->hyp_up) {
        const hipError_t ee = c->make_event(&c->hyp_up, SYNC_EVENT_FLAGS);
        if (ee != hipSuccess)
            return fail(ODO_ERR_DEVICE, std::string("hipEventCreateWithFlags(&c->hyp_up, SYNC_EVENT_FLAGS): ") +
                                            hipGetErrorString(ee));
    }
    fill_pair(c->hyp_stage.p, S.o, in, xyz1, xyz2, latch, rng);
    HIPCHK(hipMemcpyAsync(S.d, c->hyp_stage.p, up, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->hyp_up, st));
    c->hyp_up_rec = true;
    int* ints = S.at<int>(S.o.ints);
    launch_ransac_raw(st, S.scr(), 1, ng, in.words, in.cfg, 0, 0, S.rng());
    launch_ransac_hyps(st, S.d + S.o.g, ints, ints + 1, S.at<odo_dmatch>(S.o.m), S.at<float>(S.o.xyz), in.kc, 0, ng,
                       in.cfg, S.latch(), ints + 2, 0, S.rng(), S.scr(), S.bm(), in.words, S.res(), S.T(), 1, h0, h1);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

extern "C" {

int odo_ransac(odo_ctx* c, const odo_dmatch* m12, int n12, const float* xyz1, int n1, const float* xyz2, int n2,
               const odo_ransac_params* p, odo_rng* rng, double* latch, float T12[16], float* rmse,
               odo_dmatch* inliers, int* n_inliers, int* ok) {
    if (!c || !p || !rng || !latch || !T12 || !rmse || !n_inliers || !ok || n12 < 0 || (n12 && !m12))
        return fail(ODO_ERR_ARG, "bad ransac args");
    // Iterate() resets its outputs first (ransac.cpp:157-159)
    for (int i = 0; i < 16; i++) T12[i] = (i % 5 == 0) ? 1.f : 0.f;
    *rmse = 1e6f;
    *n_inliers = 0;
    *ok = 0;
    PairRansacInput in;
    const int run = prepare_pair_ransac(m12, n12, xyz1, n1, xyz2, n2, p, latch, in, c->match_cap);
    if (run <= 0) return run;  // an error, or ODO_OK with the reset outputs
    hipStream_t st = c->stream;
    // inputs packed into the pinned staging buffer, one upload; the outputs
    // (rand() state, updated in place, result record, inlier mask) are
    // adjacent, one download
    Staged s;
    const PairSections o = add_pair(s.pk, in);
    s.out_begin = o.rng;
    s.mark_inputs_end();
    const size_t o_res = s.add(sizeof(odo_pair_result)), o_bm = s.add((size_t)in.words * 4);
    int e0;
    if ((e0 = s.reserve(c, c->arena))) return e0;
    DevBuf dT(c->arena, 16 * sizeof(float)), dgp(c->arena, ransac_scratch_bytes(1, in.ng, in.words, in.cfg));
    ARENA_CHECK(c->arena);
    fill_pair(s.h, o, in, xyz1, xyz2, latch, rng);
    HIPCHK(s.upload(st));
    int* dint = s.dev<int>(o.ints);
    launch_ransac_raw(st, dgp.p, 1, in.ng, in.words, in.cfg, 0, 0, s.dev<odo_rng>(o.rng));
    launch_ransac(st, s.d + o.g, dint, dint + 1, s.dev<odo_dmatch>(o.m), s.dev<float>(o.xyz), in.kc, 0, in.ng, in.cfg,
                  s.dev<double>(o.latch), dint + 2, 0, s.dev<odo_rng>(o.rng), dgp.p, s.dev<uint32_t>(o_bm), in.words,
                  s.dev<odo_pair_result>(o_res), dT.as<float>(), 1);
    HIPCHK(hipGetLastError());
    HIPCHK(s.download(st));
    HIPCHK(hipStreamSynchronize(st));
    odo_pair_result r;
    memcpy(&r, s.host<uint8_t>(o_res), sizeof(r));
    memcpy(rng, s.host<uint8_t>(o.rng), sizeof(odo_rng));
    memcpy(T12, r.T12, sizeof(r.T12));
    *rmse = r.rmse;
    *n_inliers = gather_inliers(s.host<uint32_t>(o_bm), in.good, inliers);
    *ok = r.ransac_ok;
    return ODO_OK;
}

int odo_ransac_hyps(odo_ctx* c, const odo_dmatch* m12, int n12, const float* xyz1, int n1, const float* xyz2, int n2,
                    const odo_ransac_params* p, const odo_rng* rng, double* latch, int h0, int h1,
                    odo_hyp_summary* out, int* n_good) {
    if (!c || !p || !rng || !latch || !n_good || n12 < 0 || (n12 && !m12) || h0 < 0 || h1 < h0 ||
        h1 > std::max(p->iterations, 0) || (h1 > h0 && !out))
        return fail(ODO_ERR_ARG, "bad ransac_hyps args");
    for (int h = 0; h < h1 - h0; h++) out[h] = odo_hyp_summary{1e6, 0, 0, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
    int active = 0;
    const int e = hyps_launch(c, m12, n12, xyz1, n1, xyz2, n2, p, rng, latch, h0, h1, n_good, &active);
    if (e || !active) return e;
    HypSession& S = *c->hs;
    PairRansacInput& in = S.in;
    hipStream_t st = c->stream;
    if (h1 > h0) {
        std::vector<double> err(h1 - h0);
        std::vector<int> cnt(h1 - h0);
        std::vector<float> T((size_t)(h1 - h0) * 12);
        ransac_read_hyps(st, S.scr(), in.ng, in.words, in.cfg, h0, h1, err.data(), cnt.data(), T.data());
        HIPCHK(hipGetLastError());
        for (int h = 0; h < h1 - h0; h++) {
            out[h].err = err[h];
            out[h].cnt = cnt[h];
            memcpy(out[h].T, &T[(size_t)h * 12], 48);
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return ODO_OK;
}

int odo_ransac_hyps_dev(odo_ctx* c, const odo_dmatch* m12, int n12, const float* xyz1, int n1, const float* xyz2,
                        int n2, const odo_ransac_params* p, const odo_rng* rng, double* latch, int h0, int h1,
                        void* d_block, int* n_good) {
    if (!c || !p || !rng || !latch || !n_good || n12 < 0 || (n12 && !m12) || h0 < 0 || h1 < h0 ||
        h1 > std::max(p->iterations, 0) || (h1 > h0 && !d_block))
        return fail(ODO_ERR_ARG, "bad ransac_hyps_dev args");
    int active = 0;
    const int e = hyps_launch(c, m12, n12, xyz1, n1, xyz2, n2, p, rng, latch, h0, h1, n_good, &active);
    if (e) return e;
    hipStream_t st = c->stream;
    if (!active) {
        // no sampling: the default summaries (the fold returns before them)
        if (h1 > h0) {
            // queued on the context's stream behind its earlier work; the
            // host vector dies at return, so this path synchronises (odo.h)
            std::vector<odo_hyp_summary> d(h1 - h0, odo_hyp_summary{1e6, 0, 0, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}});
            HIPCHK(hipMemcpyAsync(d_block, d.data(), d.size() * sizeof(odo_hyp_summary), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return ODO_OK;
    }
    HypSession& S = *c->hs;
    ransac_export_hyps(st, S.scr(), S.in.ng, S.in.words, S.in.cfg, h0, h1, d_block);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

int odo_ransac_hyps_finish(odo_ctx* c, const odo_ransac_fold_result* r, odo_rng* rng, float T12[16], float* rmse,
                           odo_dmatch* inliers, int* n_inliers, int* ok, int* owner) {
    if (!c || !r || !rng || !T12 || !rmse || !n_inliers || !ok || !owner) return fail(ODO_ERR_ARG, "bad finish args");
    if (!c->hs) return fail(ODO_ERR_STATE, "no odo_ransac_hyps call to finish");
    HypSession& S = *c->hs;
    for (int i = 0; i < 16; i++) T12[i] = (i % 5 == 0) ? 1.f : 0.f;
    *rmse = 1e6f;
    *n_inliers = 0;
    *ok = 0;
    *owner = 1;
    if (!S.active) return ODO_OK;  // Iterate returned before sampling: rng untouched
    PairRansacInput& in = S.in;
    *owner = (r->best_h < 0 || (r->best_h >= S.h0 && r->best_h < S.h1)) ? 1 : 0;
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(S.rng(), rng, sizeof(odo_rng), hipMemcpyHostToDevice, st));
    launch_ransac_finish(st, S.scr(), in.ng, in.words, in.cfg, S.latch(), S.rng(),
                         S.bm(), S.res(), S.T(), r->best_h, r->visited,
                         r->valid, r->n_inliers, r->rmse);
    HIPCHK(hipGetLastError());
    odo_pair_result pr;
    std::vector<uint32_t> bm(in.words);
    HIPCHK(hipMemcpyAsync(&pr, S.res(), sizeof(pr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bm.data(), S.bm(), (size_t)in.words * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rng, S.rng(), sizeof(odo_rng), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!*owner) return ODO_OK;
    memcpy(T12, pr.T12, sizeof(pr.T12));
    *rmse = pr.rmse;
    *n_inliers = gather_inliers(bm.data(), in.good, inliers);
    *ok = pr.ransac_ok;
    return ODO_OK;
}

int odo_ransac_fold_dev(odo_ctx* c, const void* d_all, int H, void* d_fold) {
    if (!c || !d_fold || H < 0 || (H && !d_all)) return fail(ODO_ERR_ARG, "bad fold_dev args");
    if (!c->hs) return fail(ODO_ERR_STATE, "no odo_ransac_hyps_dev call to fold");
    const HypSession& S = *c->hs;
    const int ng = S.active ? S.in.ng : 0;
    const RansacCfg& k = S.in.cfg;
    launch_hyp_fold(c->stream, d_all, H, S.active ? k.iterations : 0, ng, S.active ? k.min_inlier_th : 1,
                    S.active ? k.sample_size : 1, (odo_ransac_fold_result*)d_fold);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

int odo_ransac_hyps_payload_words(odo_ctx* c) {
    if (!c || !c->hs) return fail(ODO_ERR_STATE, "no odo_ransac_hyps_dev session");
    return hyp_payload_words(c->hs->active ? c->hs->in.ng : 0);
}

int odo_ransac_hyps_finish_dev(odo_ctx* c, const void* d_fold, int rank0, void* d_payload, int payload_words) {
    if (!c || !d_fold || !d_payload) return fail(ODO_ERR_ARG, "bad finish_dev args");
    if (!c->hs) return fail(ODO_ERR_STATE, "no odo_ransac_hyps_dev call to finish");
    HypSession& S = *c->hs;
    const int ng = S.active ? S.in.ng : 0;
    if (payload_words < hyp_payload_words(ng)) return fail(ODO_ERR_CAPACITY, "hyps payload too small");
    hipStream_t st = c->stream;
    if (!S.active) {
        // Iterate returned before sampling: rank 0 reports the reset outputs
        // (T = I, rmse 1e6, not ok), the rand() state is untouched
        std::vector<int> w(payload_words, 0);
        if (rank0) {
            for (int i = 0; i < 16; i++) {
                const float v = (i % 5 == 0) ? 1.f : 0.f;
                memcpy(&w[i], &v, 4);
            }
            const float r = 1e6f;
            memcpy(&w[16], &r, 4);
        }
        HIPCHK(hipMemcpyAsync(d_payload, w.data(), w.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));  // w dies at return (odo.h: this path synchronises)
        return ODO_OK;
    }
    launch_hyp_finish(st, S.scr(), S.in.ng, S.in.words, S.in.cfg, S.latch(), S.rng(),
                      S.bm(), S.res(), S.T(),
                      (const odo_ransac_fold_result*)d_fold, S.h0, S.h1, rank0, S.at<odo_dmatch>(S.o.m), ng,
                      (int*)d_payload, payload_words);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

int odo_ransac_hyps_result(odo_ctx* c, const void* d_payload, odo_rng* rng, float T12[16], float* rmse,
                           odo_dmatch* inliers, int* n_inliers, int* ok, int* visited) {
    if (!c || !d_payload || !rng || !T12 || !rmse || !n_inliers || !ok || !visited)
        return fail(ODO_ERR_ARG, "bad hyps_result args");
    if (!c->hs) return fail(ODO_ERR_STATE, "no odo_ransac_hyps_dev session");
    HypSession& S = *c->hs;
    const int ng = S.active ? S.in.ng : 0;
    const int words = hyp_payload_words(ng);
    std::vector<int> w(words);
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(w.data(), d_payload, (size_t)words * 4, hipMemcpyDeviceToHost, st));
    if (S.active) HIPCHK(hipMemcpyAsync(rng, S.rng(), sizeof(odo_rng), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(T12, w.data(), 64);
    memcpy(rmse, &w[16], 4);
    *ok = w[17];
    *n_inliers = w[18];
    *visited = w[19];
    if (*n_inliers < 0 || *n_inliers > ng) return fail(ODO_ERR_STATE, "hyps payload: bad inlier count");
    if (inliers && *n_inliers) memcpy(inliers, &w[32], (size_t)*n_inliers * sizeof(odo_dmatch));
    return ODO_OK;
}

}  // extern "C"
