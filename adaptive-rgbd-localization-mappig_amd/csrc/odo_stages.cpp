// The synchronous per-stage entry points (odo_extract ... odo_kabsch): each
// uploads its inputs, runs one stage's kernels on the extraction stream and
// returns the outputs. The ones that pack their inputs go through Staged;
// the rest copy array by array from the caller's (pageable) memory.
#include <mutex>

#include "odo_ctx.h"

// Batched TrackLocalMap scratch: max_batch frames, lm_cap landmarks
static void free_local_map(odo_ctx* c) {
    c->lm.pool.release();
    c->lm_cap = 0;
    c->lm_n = -1;
}
static int alloc_local_map(odo_ctx* c, int lm_cap) {
    const size_t B = (size_t)c->maxb, KC = (size_t)c->kp_cap, LC = (size_t)lm_cap;
    float bounds[4];
    odo_image_bounds(c, bounds);
    c->lm_grid = local_map_grid(bounds);
    const size_t ncells = (size_t)c->lm_grid.gx * c->lm_grid.gy;
    Pack pk;  // the largest upload: every section at its capacity
    pk.add(B * 64);
    pk.add(LC * sizeof(odo_landmark));
    pk.add(B * KC * 4);
    auto& L = c->lm;
    DevPool& P = L.pool;
    int e;
    if ((e = P.alloc(&L.up, pk.off)) || (e = P.alloc(&L.seen, B * ((LC + 31) / 32)))) return e;
    if ((e = P.alloc(&L.prior_eff, B * KC)) || (e = P.alloc(&L.taken0, B * KC)) || (e = P.alloc(&L.bxy, B * KC))) return e;
    if ((e = P.alloc(&L.bjo, B * KC)) || (e = P.alloc(&L.cstart, B * (ncells + 1)))) return e;
    if ((e = P.alloc(&L.proj, B * LC * 3)) || (e = P.alloc(&L.ccount, B * LC))) return e;
    if ((e = P.alloc(&L.cand, B * LC * local_map_cand_cap())) || (e = P.alloc(&L.choice, B * LC))) return e;
    if ((e = P.alloc(&L.over, B * LC)) || (e = P.alloc(&L.slot, B * KC)) || (e = P.alloc(&L.f2_src, B * KC))) return e;
    if ((e = P.alloc(&L.Xg, B * KC * 3)) || (e = P.alloc((uint8_t**)&L.edges, B * KC * pnp_edge_bytes()))) return e;
    if ((e = P.alloc(&L.pres, B)) || (e = P.alloc(&L.mask, B * KC)) || (e = P.alloc(&L.outl, B * KC))) return e;
    if ((e = P.alloc(&L.res, B)) || (e = P.alloc(&L.ints, 2 * B))) return e;
    // pair_valid = 1 and n_matches = 2^30 for every frame (launch_pnp's gates)
    std::vector<int> ints(2 * B, 1);
    std::fill(ints.begin() + B, ints.end(), 1 << 30);
    HIPCHK(hipMemcpy(L.ints, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
    c->lm_cap = lm_cap;
    return ODO_OK;
}

extern "C" {

int odo_extract(odo_ctx* c, const uint8_t* img, int channels, const uint16_t* depth, orb_kp* kps, uint8_t* desc,
                float* kps_un, float* xyz, float* u_right, int cap, int* n) {
    if (!c || !img || (channels != 1 && channels != 3) || !n) return fail(ODO_ERR_ARG, "bad extract args");
    int e0;
    if ((e0 = sync_all(c))) return e0;
    hipStream_t st = c->stream;
    const size_t npix = (size_t)c->W * c->H;
    const int set = next_set(c);
    const int slot = 1;
    if (depth) HIPCHK(hipMemcpyAsync(c->depth_in[0], depth, npix * 2, hipMemcpyHostToDevice, st));
    else HIPCHK(hipMemsetAsync(c->depth_in[0], 0, npix * 2, st));
    if (channels == 3) {
        HIPCHK(hipMemcpyAsync(c->bgr_in[0], img, npix * 3, hipMemcpyHostToDevice, st));
        tmark(c, 0, st);
        int e = run_extract(c, set, c->bgr_in[0], c->depth_in[0], 1, slot);
        if (e) return e;
    } else {
        // ORBextractor::operator() on a gray image: level 0 = the image itself
        HIPCHK(hipMemcpy2DAsync(c->pyr + (fbase(c, set) + slot) * c->pyr_size, c->lv_h[0].pitch, img, c->W, c->W, c->H,
                                hipMemcpyHostToDevice, st));
        tmark(c, 0, st);
        int e = run_extract(c, set, nullptr, c->depth_in[0], 1, slot);  // level 0 is in place
        if (e) return e;
    }
    c->view_set = set;
    c->last_n = 1;
    c->lm_n = -1;
    return odo_get_frame(c, 0, kps, desc, kps_un, xyz, u_right, cap, n);
}

int odo_knn2_hamming(odo_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist) {
    if (!c || nq < 0 || nt < 0 || (nq && !q) || (nt && !t) || !idx || !dist) return fail(ODO_ERR_ARG, "bad knn args");
    if (nq == 0) return ODO_OK;
    if (nq > (1 << 20) || nt > (1 << 20)) return fail(ODO_ERR_CAPACITY, "knn2: at most 2^20 descriptors");
    hipStream_t st = c->stream;
    // one packed upload (descriptors + counts) and one packed download
    Staged s;
    const size_t o_q = s.add((size_t)nq * 32), o_t = s.add((size_t)std::max(nt, 1) * 32), o_n = s.add(2 * sizeof(int));
    s.mark_inputs_end();
    s.mark_outputs_begin();
    const size_t o_i = s.add((size_t)nq * sizeof(int2)), o_d = s.add((size_t)nq * sizeof(int2));
    int e;
    if ((e = s.reserve(c, c->arena))) return e;
    memcpy(s.host<uint8_t>(o_q), q, (size_t)nq * 32);
    if (nt) memcpy(s.host<uint8_t>(o_t), t, (size_t)nt * 32);
    const int cnt[2] = {nq, nt};
    memcpy(s.host<int>(o_n), cnt, sizeof(cnt));
    HIPCHK(s.upload(st));
    int* dn = s.dev<int>(o_n);
    if (c->knn_mx && nt <= 8192)  // the packed key holds a 13-bit train index
        launch_knn2_f4(st, s.dev<uint8_t>(o_q), dn, 0, s.dev<uint8_t>(o_t), dn + 1, 0, s.dev<int2>(o_i), s.dev<int2>(o_d),
                       0, nq, 1, nullptr, nullptr, 0);
    else
        launch_knn2(st, s.dev<uint8_t>(o_q), dn, 0, s.dev<uint8_t>(o_t), dn + 1, 0, s.dev<int2>(o_i), s.dev<int2>(o_d), 0,
                    nq, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(s.download(st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(idx, s.host<uint8_t>(o_i), (size_t)nq * 8);
    memcpy(dist, s.host<uint8_t>(o_d), (size_t)nq * 8);
    return ODO_OK;
}

// The pair-match stage on caller-supplied features (tests). Frame i goes to
// slot i of the set the next batch would use: frame 0 where the roll puts the
// previous frame, the others where extraction puts a batch's frames. The
// launches are the batch path's own (run_knn, run_pair_match).
int odo_debug_match_features(odo_ctx* c, int n, const int32_t* counts, const uint8_t* desc, const float* xyz,
                             const odo_pair_stage_out* out) {
    if (!c || !counts || !desc || !xyz || !out) return fail(ODO_ERR_ARG, "match_features: null argument");
    if (n < 2 || n > c->maxb + 1) return fail(ODO_ERR_ARG, "match_features: 2 .. max_batch + 1 frames");
    if (!out->lm_flags || !out->qlist || !out->qcnt || !out->knn_idx || !out->knn_dist || !out->matches ||
        !out->n_matches || !out->good || !out->n_good || !out->f2_src || !out->latch)
        return fail(ODO_ERR_ARG, "match_features: null output");
    for (int i = 0; i < n; i++)
        if (counts[i] < 0) return fail(ODO_ERR_ARG, "match_features: negative count");
    for (int i = 0; i < n; i++)
        if (counts[i] > c->kp_cap) return fail(ODO_ERR_CAPACITY, "match_features: count above odo_kp_capacity");
    int e;
    if ((e = sync_all(c))) return e;
    const int set = next_set(c), np = n - 1, nsplit = c->knn_split;
    const size_t KC = (size_t)c->kp_cap, SS = (size_t)c->maxb * KC;
    const FrameSlot f = frame_at(c, fbase(c, set));
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpy(f.nkp, counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    for (int i = 0; i < n; i++) {
        if (counts[i] == 0) continue;
        HIPCHK(hipMemcpy(f.desc + i * KC * 32, desc + i * KC * 32, (size_t)counts[i] * 32, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.xyz + i * KC * 3, xyz + i * KC * 3, (size_t)counts[i] * 12, hipMemcpyHostToDevice));
    }
    if ((e = run_knn(c, st, set, np))) return e;
    if ((e = run_pair_match(c, st, set, np, true, false))) return e;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    auto& P = c->pb[set];
    std::vector<uint32_t> bits((size_t)np * c->lm_words);
    std::vector<int32_t> ql((size_t)np * KC), src((size_t)np * KC);
    std::vector<int> qc(np), nm(np), ng(np);
    std::vector<int2> ki((size_t)nsplit * SS), kd((size_t)nsplit * SS);
    std::vector<odo_dmatch> M((size_t)np * KC);
    std::vector<uint64_t> G((size_t)np * KC);
    HIPCHK(hipMemcpy(bits.data(), c->lm_bits[set], bits.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ql.data(), c->qlist[set], ql.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(qc.data(), c->qcnt[set], (size_t)np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ki.data(), c->knn_idx[set], ki.size() * sizeof(int2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kd.data(), c->knn_dist[set], kd.size() * sizeof(int2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(M.data(), P.matches, M.size() * sizeof(odo_dmatch), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(G.data(), P.good, G.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nm.data(), P.n_matches, (size_t)np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ng.data(), P.n_good, (size_t)np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(src.data(), P.f2_src, src.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->latch, c->latch, sizeof(double), hipMemcpyDeviceToHost));
    // the context as after odo_reset, whatever the counts below turn out to be
    c->view_mode = -1;
    c->last_n = 0;
    c->lm_n = -1;
    if ((e = odo_reset(c))) return e;
    for (int p = 0; p < np; p++) {
        const int n1 = counts[p], n2 = counts[p + 1];
        const size_t o = (size_t)p * KC;
        if (qc[p] < 0 || qc[p] > n1 || nm[p] < 0 || nm[p] > c->match_cap || ng[p] < 0 || ng[p] > nm[p])
            return fail(ODO_ERR_STATE, "match_features: a count the kernels wrote is out of range");
        out->qcnt[p] = qc[p];
        out->n_matches[p] = nm[p];
        out->n_good[p] = ng[p];
        memcpy(out->qlist + o, ql.data() + o, (size_t)qc[p] * 4);
        memcpy(out->matches + o, M.data() + o, (size_t)nm[p] * sizeof(odo_dmatch));
        memcpy(out->f2_src + o, src.data() + o, (size_t)n2 * 4);
        for (int i = 0; i < n1; i++) {
            const bool lm = (bits[(size_t)p * c->lm_words + (i >> 5)] >> (i & 31)) & 1u;
            out->lm_flags[o + i] = lm ? 1 : 0;
            if (!lm) continue;  // kNN-2 ran on the landmark queries only
            // the splits' top-2 lists as one: the two smallest (distance, index)
            std::pair<int, int> best[2] = {{0x7FFFFFFF, -1}, {0x7FFFFFFF, -1}};
            for (int h = 0; h < nsplit; h++) {
                const int2 I = ki[(size_t)h * SS + o + i], D = kd[(size_t)h * SS + o + i];
                const std::pair<int, int> cand[2] = {{D.x, I.x}, {D.y, I.y}};
                for (const auto& k : cand) {
                    if (k.second < 0) continue;
                    if (k < best[0]) {
                        best[1] = best[0];
                        best[0] = k;
                    } else if (k < best[1]) best[1] = k;
                }
            }
            for (int k = 0; k < 2; k++) {
                out->knn_idx[2 * (o + i) + k] = best[k].second;
                out->knn_dist[2 * (o + i) + k] = best[k].first;
            }
        }
        for (int k = 0; k < ng[p]; k++) {
            const uint32_t at = (uint32_t)(G[o + k] >> 32);  // SortEl.val: position in the match list
            if (at >= (uint32_t)nm[p]) return fail(ODO_ERR_STATE, "match_features: good match outside the match list");
            out->good[o + k] = M[o + at];
        }
    }
    return ODO_OK;
}

int odo_pnp_motion_ba(odo_ctx* c, const float* Xw, const float* obs, int n, const odo_calib* calib,
                      const float Tcw_init[16], float Tcw_out[16], uint8_t* outlier, int* n_inliers) {
    if (!c || n < 0 || (n && (!Xw || !obs)) || !Tcw_init || !Tcw_out || !n_inliers) return fail(ODO_ERR_ARG, "bad pnp args");
    hipStream_t st = c->stream;
    // the edge capacity, a multiple of 64 as k_pnp<true>'s LDS carve-up
    // requires (its float chi2 slots follow kp_cap flag bytes)
    if (n > (1 << 30)) return fail(ODO_ERR_CAPACITY, "pnp: too many edges");
    const int kc = (std::max(n, 1) + 63) & ~63;
    // inputs packed into the pinned staging buffer, one upload; the result
    // record and the inlier mask adjacent, one download
    Staged s;
    const size_t o_x = s.add((size_t)kc * 12), o_kun = s.add((size_t)2 * kc * 8), o_ur = s.add((size_t)2 * kc * 4),
                 o_src = s.add((size_t)kc * 4), o_int = s.add(4 * sizeof(int)), o_T = s.add(16 * 4);
    s.mark_inputs_end();
    s.mark_outputs_begin();
    const size_t o_res = s.add(sizeof(odo_pair_result)), o_mask = s.add((size_t)kc);
    int e0;
    if ((e0 = s.reserve(c, c->arena))) return e0;
    DevBuf dedges(c->arena, (size_t)kc * pnp_edge_bytes());
    ARENA_CHECK(c->arena);
    float* kun = s.host<float>(o_kun) + 2 * kc;  // slot 1 of the two-slot layout
    float* ur = s.host<float>(o_ur) + kc;
    int32_t* src = s.host<int32_t>(o_src);
    if (n) memcpy(s.host<float>(o_x), Xw, (size_t)n * 12);
    for (int i = 0; i < n; i++) {
        kun[2 * i] = obs[3 * i];
        kun[2 * i + 1] = obs[3 * i + 1];
        ur[i] = obs[3 * i + 2];
        src[i] = i;
    }
    const int ints[4] = {0, n, 1, 1 << 30};  // nkp[slot0], nkp[slot1], pair_valid, n_matches
    memcpy(s.host<int>(o_int), ints, sizeof(ints));
    memcpy(s.host<float>(o_T), Tcw_init, 64);
    HIPCHK(s.upload(st));
    int* dint = s.dev<int>(o_int);
    launch_pnp(st, s.dev<int32_t>(o_src), s.dev<float>(o_x), s.dev<float>(o_kun), s.dev<float>(o_ur), dint, kc, 0,
               frame_calib(calib ? *calib : c->cfg.calib), s.dev<float>(o_T), dint + 2, dint + 3, 0, dedges.p,
               s.dev<odo_pair_result>(o_res), s.dev<uint8_t>(o_mask), 1);
    HIPCHK(hipGetLastError());
    HIPCHK(s.download(st));
    HIPCHK(hipStreamSynchronize(st));
    odo_pair_result r;
    memcpy(&r, s.host<uint8_t>(o_res), sizeof(r));
    const uint8_t* mask = s.host<uint8_t>(o_mask);
    memcpy(Tcw_out, r.Tcw, 64);
    *n_inliers = r.pnp_inliers;
    if (outlier)
        for (int i = 0; i < n; i++) outlier[i] = mask[i] ? 0 : 1;
    return ODO_OK;
}

// PnPRansac::Compute over nprob problems (problem p = points [offs[p], offs[p+1])),
// one launch chain for the whole batch.
static int pnp_ransac_run(odo_ctx* c, const float* Xw, const float* uv, const int32_t* offs, int nprob,
                          const odo_calib* calib, int iterations, float reproj_err, double confidence,
                          odo_pnp_ransac_result* res, uint8_t* inlier_mask, int32_t* good_counts) {
    // ptsetreg.cpp run(): CV_Assert(confidence > 0 && confidence < 1); niters = MAX(maxIters, 1)
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(ODO_ERR_ARG, "confidence must be in (0, 1)");
    const int H = std::max(iterations, 1);
    if (offs[0] != 0) return fail(ODO_ERR_ARG, "pnp_ransac: offs[0] must be 0");
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "pnp_ransac: more than 65535 problems per call");
    for (int p = 0; p < nprob; p++) {
        const int n = offs[p + 1] - offs[p];
        if (n < 0) return fail(ODO_ERR_ARG, "pnp_ransac: offsets must not decrease");
        if (n > pnp_ransac_max_points()) return fail(ODO_ERR_CAPACITY, "pnp_ransac: too many points");
    }
    const int total = offs[nprob];
    if ((size_t)H * (size_t)std::max(total, 1) > ((size_t)1 << 28))
        return fail(ODO_ERR_CAPACITY, "pnp_ransac: iterations x points");
    hipStream_t st = c->stream;
    DevArena& A = c->arena;
    A.begin();
    const size_t tn = (size_t)std::max(total, 1), P = (size_t)nprob;
    DevBuf dx(A, tn * 12), duv(A, tn * 8), doffs(A, (P + 1) * 4), didx(A, P * H * 5 * 4), dmodel(A, P * H * 6 * 8),
        dR(A, P * H * 9 * 8), dmask(A, (size_t)H * tn), dgood(A, P * H * 4), dstate(A, P * 4 * 4),
        dres(A, P * sizeof(odo_pnp_ransac_result)), dmo(A, tn);
    ARENA_CHECK(A);
    if (total) {
        HIPCHK(hipMemcpyAsync(dx.p, Xw, (size_t)total * 12, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(duv.p, uv, (size_t)total * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(doffs.p, offs, (P + 1) * 4, hipMemcpyHostToDevice, st));
    const odo_calib& k = calib ? *calib : c->cfg.calib;
    const float K4[4] = {k.fx, k.fy, k.cx, k.cy};
    launch_pnp_ransac(st, dx.as<float>(), duv.as<float>(), doffs.as<int>(), nprob, K4, H, reproj_err, confidence,
                      didx.as<int>(), dmodel.as<double>(), dR.as<double>(), dmask.as<uint8_t>(), dgood.as<int>(),
                      dstate.as<int>(), dres.as<odo_pnp_ransac_result>(), dmo.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res, dres.p, P * sizeof(odo_pnp_ransac_result), hipMemcpyDeviceToHost, st));
    if (inlier_mask && total) HIPCHK(hipMemcpyAsync(inlier_mask, dmo.p, (size_t)total, hipMemcpyDeviceToHost, st));
    if (good_counts) HIPCHK(hipMemcpyAsync(good_counts, dgood.p, P * H * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ODO_OK;
}

int odo_pnp_ransac(odo_ctx* c, const float* Xw, const float* uv, int n, const odo_calib* calib, int iterations,
                   float reproj_err, double confidence, odo_pnp_ransac_result* res, uint8_t* inlier_mask,
                   int32_t* good_counts) {
    if (!c || n < 0 || (n && (!Xw || !uv)) || !res) return fail(ODO_ERR_ARG, "bad pnp_ransac args");
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(ODO_ERR_ARG, "confidence must be in (0, 1)");
    if (n < 10) {  // pnpransac.cpp:30: return 0 before solvePnPRansac
        memset(res, 0, sizeof(*res));
        res->best_iter = -1;
        if (inlier_mask && n) memset(inlier_mask, 0, (size_t)n);
        return ODO_OK;
    }
    const int32_t offs[2] = {0, n};
    return pnp_ransac_run(c, Xw, uv, offs, 1, calib, iterations, reproj_err, confidence, res, inlier_mask,
                          good_counts);
}

int odo_pnp_ransac_batch(odo_ctx* c, const float* Xw, const float* uv, const int32_t* offs, int nprob,
                         const odo_calib* calib, int iterations, float reproj_err, double confidence,
                         odo_pnp_ransac_result* res, uint8_t* inlier_mask) {
    if (!c || nprob < 0 || !offs || (nprob && !res)) return fail(ODO_ERR_ARG, "bad pnp_ransac_batch args");
    if (nprob == 0) return ODO_OK;
    if (offs[nprob] > 0 && (!Xw || !uv)) return fail(ODO_ERR_ARG, "bad pnp_ransac_batch args");
    return pnp_ransac_run(c, Xw, uv, offs, nprob, calib, iterations, reproj_err, confidence, res, inlier_mask,
                          nullptr);
}

static int gicp_run(odo_ctx* c, const float* src, const int32_t* soffs, const float* tgt, const int32_t* toffs,
                    const float* guesses, int nprob, int max_iterations, double max_corr_dist, float* T12,
                    int32_t* converged, int32_t* iterations, int32_t* n_corr) {
    if (soffs[0] != 0 || toffs[0] != 0) return fail(ODO_ERR_ARG, "gicp: offsets must start at 0");
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "gicp: more than 65535 pairs per call");
    int max_ns = 0, max_nt = 0;
    for (int p = 0; p < nprob; p++) {
        const int ns = soffs[p + 1] - soffs[p], nt = toffs[p + 1] - toffs[p];
        if (ns < 0 || nt < 0) return fail(ODO_ERR_ARG, "gicp: offsets must not decrease");
        // brute-force neighbour searches: O(ns * nt) per ICP iteration in one workgroup
        if (ns > 16384 || nt > 16384) return fail(ODO_ERR_CAPACITY, "gicp: more than 16384 points in a cloud");
        max_ns = std::max(max_ns, ns);
        max_nt = std::max(max_nt, nt);
    }
    const size_t S = (size_t)std::max(soffs[nprob], 1), T = (size_t)std::max(toffs[nprob], 1), P = (size_t)nprob;
    hipStream_t st = c->stream;
    DevArena& A = c->arena;
    A.begin();
    DevBuf ds(A, S * 12), dt(A, T * 12), dCs(A, S * 72), dCt(A, T * 72), dout(A, S * 12), dM(A, S * 72), dis(A, S * 4),
        dit(A, S * 4), dT(A, P * 64), dio(A, P * 16), dg(A, P * 64), dso(A, (P + 1) * 4), dto(A, (P + 1) * 4);
    ARENA_CHECK(A);
    if (soffs[nprob]) HIPCHK(hipMemcpyAsync(ds.p, src, (size_t)soffs[nprob] * 12, hipMemcpyHostToDevice, st));
    if (toffs[nprob]) HIPCHK(hipMemcpyAsync(dt.p, tgt, (size_t)toffs[nprob] * 12, hipMemcpyHostToDevice, st));
    std::vector<float> g(16 * P);
    for (size_t p = 0; p < P; p++)
        for (int i = 0; i < 16; i++) g[16 * p + i] = guesses ? guesses[16 * p + i] : (i % 5 == 0 ? 1.f : 0.f);
    HIPCHK(hipMemcpyAsync(dg.p, g.data(), P * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dso.p, soffs, (P + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dto.p, toffs, (P + 1) * 4, hipMemcpyHostToDevice, st));
    GicpArgs args{dg.as<float>(), dso.as<int>(), dto.as<int>(), max_corr_dist, max_iterations, 20 /* PCL inner */};
    launch_gicp(st, ds.as<float>(), dt.as<float>(), nprob, max_ns, max_nt, dCs.as<double>(), dCt.as<double>(),
                dout.as<float>(), dM.as<double>(), dis.as<int>(), dit.as<int>(), args, dT.as<float>(), dio.as<int>());
    HIPCHK(hipGetLastError());
    std::vector<int> io(4 * P);
    HIPCHK(hipMemcpyAsync(T12, dT.p, P * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(io.data(), dio.p, P * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++) {
        converged[p] = io[4 * p];
        iterations[p] = io[4 * p + 1];
        n_corr[p] = io[4 * p + 2];
    }
    return ODO_OK;
}

int odo_gicp(odo_ctx* c, const float* src, int ns, const float* tgt, int nt, const float guess[16], int max_iterations,
             double max_corr_dist, float T12[16], int* converged, int* iterations, int* n_corr) {
    if (!c || ns < 0 || nt < 0 || (ns && !src) || (nt && !tgt) || !T12 || !converged || !iterations || !n_corr)
        return fail(ODO_ERR_ARG, "bad gicp args");
    *converged = 0;
    *iterations = 0;
    *n_corr = 0;
    for (int i = 0; i < 16; i++) T12[i] = i % 5 == 0 ? 1.f : 0.f;
    if (ns < 20 || nt < 20) return ODO_OK;  // generalizedicp.cpp:33
    const int32_t so[2] = {0, ns}, to[2] = {0, nt};
    return gicp_run(c, src, so, tgt, to, guess, 1, max_iterations, max_corr_dist, T12, converged, iterations, n_corr);
}

int odo_gicp_batch(odo_ctx* c, const float* src, const int32_t* soffs, const float* tgt, const int32_t* toffs,
                   const float* guesses, int nprob, int max_iterations, double max_corr_dist, float* T12,
                   int32_t* converged, int32_t* iterations, int32_t* n_corr) {
    if (!c || nprob < 0 || !soffs || !toffs || (nprob && (!T12 || !converged || !iterations || !n_corr)))
        return fail(ODO_ERR_ARG, "bad gicp_batch args");
    if (nprob == 0) return ODO_OK;
    if ((soffs[nprob] > 0 && !src) || (toffs[nprob] > 0 && !tgt)) return fail(ODO_ERR_ARG, "bad gicp_batch args");
    return gicp_run(c, src, soffs, tgt, toffs, guesses, nprob, max_iterations, max_corr_dist, T12, converged,
                    iterations, n_corr);
}

int odo_gicp_covariances(odo_ctx* c, const float* P, const int32_t* offs, int nprob, double* C) {
    if (!c || nprob < 0 || !offs) return fail(ODO_ERR_ARG, "bad gicp_covariances args");
    if (nprob == 0) return ODO_OK;
    if (offs[0] != 0) return fail(ODO_ERR_ARG, "gicp_covariances: offsets must start at 0");
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "gicp_covariances: more than 65535 clouds per call");
    int max_n = 0;
    for (int p = 0; p < nprob; p++) {
        const int n = offs[p + 1] - offs[p];
        if (n < 0) return fail(ODO_ERR_ARG, "gicp_covariances: offsets must not decrease");
        if (n > 16384) return fail(ODO_ERR_CAPACITY, "gicp_covariances: more than 16384 points in a cloud");
        max_n = std::max(max_n, n);
    }
    const size_t N = (size_t)offs[nprob], np = (size_t)nprob;
    if (N == 0) return ODO_OK;
    if (!P || !C) return fail(ODO_ERR_ARG, "bad gicp_covariances args");
    memset(C, 0, N * 72);  // k_gicp_cov skips clouds under 20 points
    if (max_n < 20) return ODO_OK;
    hipStream_t st = c->stream;
    DevArena& A = c->arena;
    A.begin();
    DevBuf dp(A, N * 12), dCs(A, N * 72), dCt(A, N * 72), doff(A, (np + 1) * 4);
    ARENA_CHECK(A);
    HIPCHK(hipMemcpyAsync(dp.p, P, N * 12, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(doff.p, offs, (np + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dCs.p, 0, N * 72, st));
    HIPCHK(hipMemsetAsync(dCt.p, 0, N * 72, st));
    // the batch in both roles: the source set is returned, the target set must repeat it
    launch_gicp_cov(st, dp.as<float>(), doff.as<int>(), dCs.as<double>(), dp.as<float>(), doff.as<int>(),
                    dCt.as<double>(), nprob, max_n);
    HIPCHK(hipGetLastError());
    std::vector<double> Ct(N * 9);
    HIPCHK(hipMemcpyAsync(C, dCs.p, N * 72, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Ct.data(), dCt.p, N * 72, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (memcmp(C, Ct.data(), N * 72) != 0)
        return fail(ODO_ERR_DEVICE, "gicp_covariances: the source and the target set differ");
    return ODO_OK;
}

// Frame::ComputeImageBounds: cv::undistortPoints of the four corners (5
// iterations in double, App. A.10)
static void undistort_host(float u, float v, const odo_calib& c, float* uo, float* vo) {
    const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
    const double ifx = 1. / fx, ify = 1. / fy;
    const double k0 = c.k1, k1 = c.k2, k2 = c.p1, k3 = c.p2, k4 = c.k3;
    double x = u, y = v;
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
    *uo = (float)(fx * x + cx);
    *vo = (float)(fy * y + cy);
}

int odo_image_bounds(odo_ctx* c, float b[4]) {
    if (!c || !b) return fail(ODO_ERR_ARG, "bad bounds args");
    const odo_calib& k = c->cfg.calib;
    if (k.k1 != 0.0f) {
        const float cu[4] = {0.f, (float)c->W, 0.f, (float)c->W}, cv_[4] = {0.f, 0.f, (float)c->H, (float)c->H};
        float u[4], v[4];
        for (int i = 0; i < 4; i++) undistort_host(cu[i], cv_[i], k, &u[i], &v[i]);
        b[0] = std::min(u[0], u[2]);
        b[1] = std::max(u[1], u[3]);
        b[2] = std::min(v[0], v[1]);
        b[3] = std::max(v[2], v[3]);
    } else {
        b[0] = 0.f;
        b[1] = (float)c->W;
        b[2] = 0.f;
        b[3] = (float)c->H;
    }
    return ODO_OK;
}

int odo_projection_match(odo_ctx* c, const float Tcw[16], const odo_landmark* lms, int nL, const float* kun,
                         const int32_t* octave, const uint8_t* desc, int n, const uint8_t* slot_taken, float th,
                         float nn_ratio, int32_t* slot_lm, float* proj, int* n_matches) {
    if (!c || !Tcw || nL < 0 || n < 0 || (nL && (!lms || !proj)) || (n && (!kun || !octave || !desc || !slot_lm)) ||
        !n_matches)
        return fail(ODO_ERR_ARG, "bad projection_match args");
    if (n > 8191) return fail(ODO_ERR_CAPACITY, "more than 8191 keypoints");
    *n_matches = 0;
    hipStream_t st = c->stream;
    float b[4];
    odo_image_bounds(c, b);
    const odo_calib& k = c->cfg.calib;
    // one frame of the local-map search (k_localmap.hip): kp_cap = the frame's
    // own rows, no prior, the caller's taken slots; scratch from the arena
    LmSearch a{};
    a.nframes = 1;
    a.nL = nL;
    a.kp_cap = std::max(n, 1);
    a.seen_words = (nL + 31) / 32;
    a.oct_stride = 1;
    a.G = local_map_grid(b);
    a.C = LmCalib{k.fx, k.fy, k.cx, k.cy, k.mbf, b[0], b[1], b[2], b[3]};
    a.th = th;
    a.nnratio = nn_ratio;
    const size_t nl = std::max(nL, 1), nn = a.kp_cap, nw = std::max(a.seen_words, 1);
    const size_t ncells = (size_t)a.G.gx * a.G.gy;
    DevArena& A = c->arena;
    A.begin();
    DevBuf dT(A, 64), dl(A, nl * sizeof(odo_landmark)), dk(A, nn * 8), doc(A, nn * 4), dd(A, nn * 32), dtk(A, nn),
        dn(A, 4), dseen(A, nw * 4), dpe(A, nn * 4), dt0(A, nn), dbxy(A, nn * 8), dbjo(A, nn * 4),
        dcs(A, (ncells + 1) * 4), dproj(A, nl * 12), dcc(A, nl * 4), dcand(A, nl * local_map_cand_cap() * 4),
        dch(A, nl * 4), dov(A, nl * 4), dsl(A, nn * 4), df2(A, nn * 4), dXg(A, nn * 12),
        dres(A, sizeof(odo_local_map_result));
    ARENA_CHECK(A);
    HIPCHK(hipMemcpyAsync(dT.p, Tcw, 64, hipMemcpyHostToDevice, st));
    if (nL) HIPCHK(hipMemcpyAsync(dl.p, lms, (size_t)nL * sizeof(odo_landmark), hipMemcpyHostToDevice, st));
    if (n) {
        HIPCHK(hipMemcpyAsync(dk.p, kun, (size_t)n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(doc.p, octave, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dd.p, desc, (size_t)n * 32, hipMemcpyHostToDevice, st));
        if (slot_taken) HIPCHK(hipMemcpyAsync(dtk.p, slot_taken, (size_t)n, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dn.p, n, 1, st));
    HIPCHK(hipMemsetAsync(dseen.p, 0, nw * 4, st));
    a.Tcw = dT.as<float>();
    a.lms = dl.as<odo_landmark>();
    a.taken_in = slot_taken ? dtk.as<uint8_t>() : nullptr;
    a.kun = dk.as<float>();
    a.oct = doc.as<int32_t>();
    a.desc = dd.as<uint8_t>();
    a.nkp = dn.as<int>();
    a.seen = dseen.as<uint32_t>();
    a.prior_eff = dpe.as<int32_t>();
    a.taken0 = dt0.as<uint8_t>();
    a.bxy = dbxy.as<float2>();
    a.bjo = dbjo.as<uint32_t>();
    a.cstart = dcs.as<int>();
    a.proj = dproj.as<float>();
    a.ccount = dcc.as<int>();
    a.cand = dcand.as<uint32_t>();
    a.choice = dch.as<int32_t>();
    a.over = dov.as<int32_t>();
    a.slot_lm = dsl.as<int32_t>();
    a.f2_src = df2.as<int32_t>();
    a.Xg = dXg.as<float>();
    a.res = dres.as<odo_local_map_result>();
    if (launch_local_map_search(st, a) != 0) return fail(ODO_ERR_CAPACITY, "projection match capacity");
    HIPCHK(hipGetLastError());
    if (nL) HIPCHK(hipMemcpyAsync(proj, dproj.p, (size_t)nL * 12, hipMemcpyDeviceToHost, st));
    if (n) HIPCHK(hipMemcpyAsync(slot_lm, dsl.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(n_matches, &a.res->n_matches, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ODO_OK;
}

// Matcher::Fuse's search for every Fuse call of FuseLandmarks (k_fuse.hip):
// validation, one upload, the bins and the search, one download.
constexpr int FUSE_MAX_KF = 256, FUSE_MAX_KP = 8191, FUSE_MAX_LM = 65536, FUSE_MAX_REC = 1 << 20;
int odo_fuse_search(odo_ctx* c, const odo_fuse_kf* kfs, int n_kf, const float* kun, const float* ur, const uint8_t* desc,
                    int n_kp, const odo_landmark* lms, int n_lms, const int32_t* lm_index, int n_index, float th,
                    odo_fuse_cand* out) {
    if (!c || n_kf < 0 || n_kp < 0 || n_lms < 0 || n_index < 0 || (n_kf && !kfs) || (n_kp && (!kun || !ur || !desc)) ||
        (n_lms && !lms) || (n_index && !lm_index))
        return fail(ODO_ERR_ARG, "bad fuse_search args");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ODO_ERR_ARG, "fuse_search: th must be finite and >= 0");
    if (n_kf > FUSE_MAX_KF) return fail(ODO_ERR_CAPACITY, "fuse_search: more than 256 calls");
    if (n_lms > FUSE_MAX_LM) return fail(ODO_ERR_CAPACITY, "fuse_search: more than 65536 landmarks");
    std::vector<int32_t> kp_off((size_t)n_kf + 1, 0), rec_off((size_t)n_kf + 1, 0);
    int max_kp = 0, max_list = 0;
    for (int k = 0; k < n_kf; k++) {
        const odo_fuse_kf& F = kfs[k];
        if (F.kp_begin < 0 || F.kp_end < F.kp_begin || F.kp_end > n_kp)
            return fail(ODO_ERR_ARG, "fuse_search: a keypoint range outside [0, n_kp]");
        if (F.lm_begin < 0 || F.lm_end < F.lm_begin || F.lm_end > n_index)
            return fail(ODO_ERR_ARG, "fuse_search: a list range outside [0, n_index]");
        const int nk = F.kp_end - F.kp_begin, nl = F.lm_end - F.lm_begin;
        if (nk > FUSE_MAX_KP) return fail(ODO_ERR_CAPACITY, "fuse_search: a keyframe with more than 8191 keypoints");
        if (nl > FUSE_MAX_REC - rec_off[k]) return fail(ODO_ERR_CAPACITY, "fuse_search: more than 2^20 records");
        kp_off[(size_t)k + 1] = kp_off[k] + nk;  // at most 256 * 8191
        rec_off[(size_t)k + 1] = rec_off[k] + nl;
        max_kp = std::max(max_kp, nk);
        max_list = std::max(max_list, nl);
    }
    const size_t NK = (size_t)n_kf, NP = (size_t)n_kp, NR = (size_t)rec_off[NK];
    if (NR == 0) return ODO_OK;  // no record to write
    if (!out) return fail(ODO_ERR_ARG, "bad fuse_search args");
    int e;
    if ((e = sync_all(c))) return e;
    hipStream_t st = c->stream;
    float b[4];
    odo_image_bounds(c, b);
    const LmGrid G = local_map_grid(b);
    const size_t ncells = (size_t)G.gx * G.gy;
    Staged s;
    const size_t o_kf = s.add(NK * sizeof(odo_fuse_kf)), o_ko = s.add((NK + 1) * 4), o_ro = s.add((NK + 1) * 4),
                 o_kun = s.add(NP * 8), o_ur = s.add(NP * 4), o_desc = s.add(NP * 32),
                 o_lms = s.add((size_t)n_lms * sizeof(odo_landmark)), o_idx = s.add((size_t)n_index * 4);
    s.mark_inputs_end();
    s.mark_outputs_begin();
    const size_t o_out = s.add(NR * sizeof(odo_fuse_cand));
    // on the device the sorted points and the cell starts follow the pack
    Pack scr = s.pk;
    const size_t o_bpt = scr.add((size_t)kp_off[NK] * sizeof(float4)), o_cs = scr.add(NK * (ncells + 1) * 4);
    if ((e = c->fuse_dev.reserve(scr.off, (size_t)1 << 20, "fuse_search")) || (e = s.reserve(c, c->fuse_dev.p))) return e;
    memcpy(s.host<odo_fuse_kf>(o_kf), kfs, NK * sizeof(odo_fuse_kf));
    memcpy(s.host<int32_t>(o_ko), kp_off.data(), (NK + 1) * 4);
    memcpy(s.host<int32_t>(o_ro), rec_off.data(), (NK + 1) * 4);
    if (n_kp) {
        memcpy(s.host<float>(o_kun), kun, NP * 8);
        memcpy(s.host<float>(o_ur), ur, NP * 4);
        memcpy(s.host<uint8_t>(o_desc), desc, NP * 32);
    }
    if (n_lms) memcpy(s.host<odo_landmark>(o_lms), lms, (size_t)n_lms * sizeof(odo_landmark));
    memcpy(s.host<int32_t>(o_idx), lm_index, (size_t)n_index * 4);
    HIPCHK(s.upload(st));
    const odo_calib& k = c->cfg.calib;
    FuseSearch a{};
    a.n_kf = n_kf;
    a.n_lms = n_lms;
    a.max_kp = max_kp;
    a.max_list = max_list;
    a.kfs = s.dev<odo_fuse_kf>(o_kf);
    a.kun = s.dev<float>(o_kun);
    a.ur = s.dev<float>(o_ur);
    a.desc = s.dev<uint8_t>(o_desc);
    a.lms = s.dev<odo_landmark>(o_lms);
    a.lm_index = s.dev<int32_t>(o_idx);
    a.kp_off = s.dev<int32_t>(o_ko);
    a.rec_off = s.dev<int32_t>(o_ro);
    a.G = G;
    a.C = LmCalib{k.fx, k.fy, k.cx, k.cy, k.mbf, b[0], b[1], b[2], b[3]};
    a.th = th;
    a.bpt = s.dev<float4>(o_bpt);
    a.cstart = s.dev<int>(o_cs);
    a.out = s.dev<odo_fuse_cand>(o_out);
    if (launch_fuse_search(st, a) != 0) return fail(ODO_ERR_CAPACITY, "fuse_search capacity");
    HIPCHK(hipGetLastError());
    HIPCHK(s.download(st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, s.host<odo_fuse_cand>(o_out), NR * sizeof(odo_fuse_cand));
    return ODO_OK;
}

// Tracking::TrackLocalMap for the frames of the last batch, where they sit
// (k_localmap.hip, then the batch's k_pnp over the gathered edges).
constexpr int LM_MAX_LANDMARKS = 65536;
int odo_track_local_map(odo_ctx* c, const odo_landmark* lms, int nL, const float* Tcw, const int32_t* prior, int kp_cap,
                        float th, float nn_ratio, odo_local_map_result* results) {
    if (!c || !Tcw || !results || nL < 0 || (nL && !lms)) return fail(ODO_ERR_ARG, "bad track_local_map args");
    if (kp_cap != c->kp_cap) return fail(ODO_ERR_ARG, "track_local_map: kp_cap is not odo_kp_capacity()");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ODO_ERR_ARG, "track_local_map: th must be finite and >= 0");
    if (c->last_n <= 0) return fail(ODO_ERR_STATE, "track_local_map: no batch yet");
    if (nL > LM_MAX_LANDMARKS) return fail(ODO_ERR_CAPACITY, "track_local_map: more than 65536 landmarks");
    if (c->kp_cap > 8191) return fail(ODO_ERR_CAPACITY, "track_local_map: more than 8191 keypoints");
    int e;
    if ((e = sync_all(c))) return e;
    c->lm_n = -1;
    if (c->lm_cap == 0 || nL > c->lm_cap) {
        free_local_map(c);
        if ((e = alloc_local_map(c, std::max((nL + 1023) & ~1023, 4096)))) {  // all or nothing
            free_local_map(c);
            return e;
        }
    }
    const int n = c->last_n;
    const size_t KC = (size_t)c->kp_cap, fb = fbase(c, c->view_set);
    auto& L = c->lm;
    hipStream_t st = c->stream;
    // poses, priors and landmarks packed into the pinned staging buffer, one
    // upload into L.up; the result records come back over them (the staging
    // buffer grows before the pack is reserved: growing loses its contents)
    Staged s;
    const size_t o_T = s.add((size_t)n * 64), o_lms = s.add((size_t)nL * sizeof(odo_landmark)),
                 o_prior = s.add(prior ? (size_t)n * KC * 4 : 0);
    s.mark_inputs_end();
    if ((e = stage_reserve(c, std::max(s.in_end, (size_t)n * sizeof(odo_local_map_result)))) || (e = s.reserve(c, L.up)))
        return e;
    memcpy(s.host<float>(o_T), Tcw, (size_t)n * 64);
    if (nL) memcpy(s.host<odo_landmark>(o_lms), lms, (size_t)nL * sizeof(odo_landmark));
    if (prior) memcpy(s.host<int32_t>(o_prior), prior, (size_t)n * KC * 4);
    HIPCHK(s.upload(st));
    const int seen_words = (c->lm_cap + 31) / 32;
    HIPCHK(hipMemsetAsync(L.seen, 0, (size_t)n * seen_words * 4, st));
    float b[4];
    odo_image_bounds(c, b);
    const odo_calib& k = c->cfg.calib;
    LmSearch a{};
    a.nframes = n;
    a.nL = nL;
    a.kp_cap = c->kp_cap;
    a.seen_words = seen_words;
    a.Tcw = s.dev<float>(o_T);
    a.lms = s.dev<odo_landmark>(o_lms);
    a.prior = prior ? s.dev<int32_t>(o_prior) : nullptr;
    // slot 0 of the batch's frame set (k_pnp's and the statistics' base): frame i
    // sits in slot i + 1, the search starts at slot 1
    const float* kun0 = c->kun + fb * KC * 2;
    const int* nkp0 = c->nkp + fb;
    a.kun = kun0 + KC * 2;
    a.oct = &c->kps[(fb + 1) * KC].octave;
    a.oct_stride = sizeof(orb_kp) / 4;
    a.desc = c->desc + (fb + 1) * KC * 32;
    a.nkp = nkp0 + 1;
    a.G = c->lm_grid;
    a.C = LmCalib{k.fx, k.fy, k.cx, k.cy, k.mbf, b[0], b[1], b[2], b[3]};
    a.th = th;
    a.nnratio = nn_ratio;
    a.seen = L.seen;
    a.prior_eff = L.prior_eff;
    a.taken0 = L.taken0;
    a.bxy = L.bxy;
    a.bjo = L.bjo;
    a.cstart = L.cstart;
    a.proj = L.proj;
    a.ccount = L.ccount;
    a.cand = L.cand;
    a.choice = L.choice;
    a.over = L.over;
    a.slot_lm = L.slot;
    a.f2_src = L.f2_src;
    a.Xg = L.Xg;
    a.res = L.res;
    if (launch_local_map_search(st, a) != 0) return fail(ODO_ERR_CAPACITY, "track_local_map capacity");
    HIPCHK(hipGetLastError());
    // the second PnPSolver::Compute: k_pnp with pair p = frame p, its "F1
    // points" the gathered landmark positions (slot p of Xg), its F2 the
    // frame's slot p + 1, from the pose passed in
    launch_pnp(st, L.f2_src, L.Xg, kun0, c->ur + fb * KC, nkp0, c->kp_cap, 0, c->cal, a.Tcw, L.ints, L.ints + c->maxb,
               0, L.edges, L.pres, L.mask, n);
    HIPCHK(hipGetLastError());
    launch_local_map_stats(st, a.lms, nkp0, c->kp_cap, L.slot, L.mask, L.pres, L.outl, L.res, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h, L.res, (size_t)n * sizeof(odo_local_map_result), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(results, s.h, (size_t)n * sizeof(odo_local_map_result));
    c->lm_n = nL;
    return ODO_OK;
}

// LocalBundleAdjustment::Compute (k_ba.hip): validation, the two CSRs, one
// upload, the Levenberg loop (ba_run), one download.
void odo_default_ba_params(odo_ba_params* p) {
    if (!p) return;
    p->iters_robust = 5;
    p->iters_final = 10;
    p->robust = 1;
    p->huber_mono = sqrtf(5.991f);
    p->huber_stereo = sqrtf(7.815f);
    p->chi2_mono = 5.991f;
    p->chi2_stereo = 7.815f;
}

constexpr int BA_MAX_FREE = 64, BA_MAX_KF = 256, BA_MAX_LM = 65536, BA_MAX_EDGES = 1 << 20;
int odo_local_ba(odo_ctx* c, float* Tcw, const uint8_t* kf_fixed, int n_kf, float* Xw, int n_lm, const odo_ba_edge* edges,
                 int n_edges, const odo_calib* calib, const odo_ba_params* params, uint8_t* edge_erase,
                 odo_ba_result* result) {
    if (!c || !result || n_kf < 0 || n_lm < 0 || n_edges < 0 || (n_kf && (!Tcw || !kf_fixed)) || (n_lm && !Xw) ||
        (n_edges && (!edges || !edge_erase)))
        return fail(ODO_ERR_ARG, "bad local_ba args");
    odo_ba_params P;
    if (params) P = *params;
    else odo_default_ba_params(&P);
    if (P.iters_robust < 1 || P.iters_final < 0 || !(P.huber_mono > 0.f) || !(P.huber_stereo > 0.f) ||
        !std::isfinite(P.huber_mono) || !std::isfinite(P.huber_stereo) || !(P.chi2_mono > 0.f) || !(P.chi2_stereo > 0.f))
        return fail(ODO_ERR_ARG, "local_ba: bad params (iters_robust >= 1, iters_final >= 0, positive thresholds)");
    if (n_kf > BA_MAX_KF) return fail(ODO_ERR_CAPACITY, "local_ba: more than 256 keyframes");
    if (n_lm > BA_MAX_LM) return fail(ODO_ERR_CAPACITY, "local_ba: more than 65536 landmarks");
    if (n_edges > BA_MAX_EDGES) return fail(ODO_ERR_CAPACITY, "local_ba: more than 2^20 edges");
    std::vector<int32_t> pidx((size_t)std::max(n_kf, 1), -1);
    int nf = 0;
    for (int k = 0; k < n_kf; k++)
        if (!kf_fixed[k]) pidx[k] = nf++;
    if (nf > BA_MAX_FREE) return fail(ODO_ERR_CAPACITY, "local_ba: more than 64 free keyframes");
    for (size_t i = 0; i < (size_t)n_kf * 16; i++)
        if (!std::isfinite(Tcw[i])) return fail(ODO_ERR_ARG, "local_ba: non-finite pose");
    for (size_t i = 0; i < (size_t)n_lm * 3; i++)
        if (!std::isfinite(Xw[i])) return fail(ODO_ERR_ARG, "local_ba: non-finite landmark");
    for (int l = 0; l < n_lm; l++) {
        const float z = Xw[3 * (size_t)l + 2];
        if (!std::isfinite(1.0f / (z * z)))  // z == 0, or so small that z * z underflows
            return fail(ODO_ERR_ARG, "local_ba: a landmark with infinite information (z * z == 0 in float)");
    }
    // the CSRs by landmark and by keyframe, both in edge order (counting sorts)
    std::vector<int32_t> lstart((size_t)n_lm + 1, 0), kstart((size_t)n_kf + 1, 0), lorder((size_t)std::max(n_edges, 1)),
        korder((size_t)std::max(n_edges, 1));
    for (int e = 0; e < n_edges; e++) {
        const odo_ba_edge& E = edges[e];
        if (E.kf < 0 || E.kf >= n_kf || E.lm < 0 || E.lm >= n_lm) return fail(ODO_ERR_ARG, "local_ba: edge index out of range");
        if (!std::isfinite(E.u) || !std::isfinite(E.v) || !std::isfinite(E.ur))
            return fail(ODO_ERR_ARG, "local_ba: non-finite observation");
        lstart[(size_t)E.lm + 1]++;
        kstart[(size_t)E.kf + 1]++;
    }
    for (int l = 0; l < n_lm; l++) lstart[(size_t)l + 1] += lstart[l];
    for (int k = 0; k < n_kf; k++) kstart[(size_t)k + 1] += kstart[k];
    {
        std::vector<int32_t> lpos(lstart.begin(), lstart.end() - 1), kpos(kstart.begin(), kstart.end() - 1);
        for (int e = 0; e < n_edges; e++) {
            lorder[lpos[edges[e].lm]++] = e;
            korder[kpos[edges[e].kf]++] = e;
        }
        // at most one edge per (keyframe, landmark): the Schur kernel's items rely on it
        std::vector<int32_t> stamp((size_t)std::max(n_kf, 1), -1);
        for (int l = 0; l < n_lm; l++)
            for (int q = lstart[l]; q < lstart[(size_t)l + 1]; q++) {
                const int k = edges[lorder[q]].kf;
                if (stamp[k] == l) return fail(ODO_ERR_ARG, "local_ba: a (keyframe, landmark) pair appears in two edges");
                stamp[k] = l;
            }
    }
    memset(result, 0, sizeof(*result));
    if (n_edges == 0) {  // nothing to optimise: no vertex has an edge
        result->status = ODO_BA_NOTHING;
        return ODO_OK;
    }
    int e0;
    if ((e0 = sync_all(c))) return e0;
    hipStream_t st = c->stream;
    const size_t NK = (size_t)n_kf, NL = (size_t)n_lm, NE = (size_t)n_edges;
    Staged s;
    const size_t o_T = s.add(NK * 64), o_X = s.add(NL * 12), o_pidx = s.add(NK * 4), o_insys = s.add(NK),
                 o_ekf = s.add(NE * 4), o_elm = s.add(NE * 4), o_obs = s.add(NE * 12), o_ls = s.add((NL + 1) * 4),
                 o_lo = s.add(NE * 4), o_ks = s.add((NK + 1) * 4), o_ko = s.add(NE * 4);
    s.mark_inputs_end();
    s.mark_outputs_begin();
    const size_t o_oT = s.add(NK * 64), o_oX = s.add(NL * 12), o_er = s.add(NE), o_cnt = s.add(16);
    // on the device ba_run's scratch follows the pack; in the staging buffer
    // the per-trial scalars do (reserved first: growing loses the contents)
    const size_t io_bytes = s.pk.off, need = io_bytes + ba_scratch_bytes(n_kf, n_lm, n_edges, nf);
    if ((e0 = stage_reserve(c, io_bytes + 256))) return e0;
    if ((e0 = c->ba_dev.reserve(need, (size_t)1 << 20, "local_ba")) || (e0 = s.reserve(c, c->ba_dev.p))) return e0;
    memcpy(s.host<float>(o_T), Tcw, NK * 64);
    memcpy(s.host<float>(o_X), Xw, NL * 12);
    memcpy(s.host<int32_t>(o_pidx), pidx.data(), NK * 4);
    for (int k = 0; k < n_kf; k++) s.h[o_insys + k] = (pidx[k] >= 0 && kstart[(size_t)k + 1] > kstart[k]) ? 1 : 0;
    {
        int32_t *ekf = s.host<int32_t>(o_ekf), *elm = s.host<int32_t>(o_elm);
        float* ob = s.host<float>(o_obs);
        for (int e = 0; e < n_edges; e++) {
            ekf[e] = edges[e].kf;
            elm[e] = edges[e].lm;
            ob[3 * (size_t)e] = edges[e].u;
            ob[3 * (size_t)e + 1] = edges[e].v;
            ob[3 * (size_t)e + 2] = edges[e].ur;
        }
    }
    memcpy(s.host<int32_t>(o_ls), lstart.data(), (NL + 1) * 4);
    memcpy(s.host<int32_t>(o_lo), lorder.data(), NE * 4);
    memcpy(s.host<int32_t>(o_ks), kstart.data(), (NK + 1) * 4);
    memcpy(s.host<int32_t>(o_ko), korder.data(), NE * 4);
    HIPCHK(s.upload(st));
    const odo_calib& k = calib ? *calib : c->cfg.calib;
    BaArgs a{};
    a.nk = n_kf;
    a.nl = n_lm;
    a.ne = n_edges;
    a.nf = nf;
    a.Tcw = s.dev<float>(o_T);
    a.Xw = s.dev<float>(o_X);
    a.eobs = s.dev<float>(o_obs);
    a.ekf = s.dev<int32_t>(o_ekf);
    a.elm = s.dev<int32_t>(o_elm);
    a.lstart = s.dev<int32_t>(o_ls);
    a.lorder = s.dev<int32_t>(o_lo);
    a.kstart = s.dev<int32_t>(o_ks);
    a.korder = s.dev<int32_t>(o_ko);
    a.pidx = s.dev<int32_t>(o_pidx);
    a.insys = s.dev<uint8_t>(o_insys);
    a.oT = s.dev<float>(o_oT);
    a.oX = s.dev<float>(o_oX);
    a.erase = s.dev<uint8_t>(o_er);
    a.counts = s.dev<int32_t>(o_cnt);
    a.scratch = s.d + io_bytes;
    a.h_scal = s.host<double>(io_bytes);
    a.fx = (double)k.fx;
    a.fy = (double)k.fy;
    a.cx = (double)k.cx;
    a.cy = (double)k.cy;
    a.bf = (double)k.mbf;
    odo_ba_result r{};
    const hipError_t he = ba_run(st, a, P, &r);
    if (he != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(ODO_ERR_DEVICE, std::string("local_ba: ") + hipGetErrorString(he));
    }
    HIPCHK(s.download(st));
    HIPCHK(hipStreamSynchronize(st));
    int32_t cnt[4];
    memcpy(cnt, s.host<int32_t>(o_cnt), sizeof(cnt));
    r.n_level1 = cnt[0];
    r.n_erase = cnt[1];
    r.status = ODO_BA_RAN;
    memcpy(Tcw, s.host<float>(o_oT), NK * 64);
    memcpy(Xw, s.host<float>(o_oX), NL * 12);
    memcpy(edge_erase, s.host<uint8_t>(o_er), NE);
    *result = r;
    return ODO_OK;
}

int odo_get_local_map(odo_ctx* c, int i, int32_t* slot_lm, float* proj, uint8_t* pnp_outlier, int cap) {
    if (!c || !slot_lm || cap < 0) return fail(ODO_ERR_ARG, "bad get_local_map args");
    if (c->lm_n < 0) return fail(ODO_ERR_STATE, "get_local_map: the last batch has no local-map results");
    if (i < 0 || i >= c->last_n) return fail(ODO_ERR_ARG, "bad frame index");
    int e;
    if ((e = sync_all(c))) return e;
    const size_t KC = (size_t)c->kp_cap, nL = (size_t)c->lm_n;
    auto& L = c->lm;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, c->nkp + fbase(c, c->view_set) + i + 1, sizeof(int), hipMemcpyDeviceToHost));
    cnt = std::min(cnt, c->kp_cap);
    const size_t m = (size_t)std::max(0, std::min(cnt, cap));
    if (m) HIPCHK(hipMemcpy(slot_lm, L.slot + (size_t)i * KC, m * 4, hipMemcpyDeviceToHost));
    if (pnp_outlier && m) HIPCHK(hipMemcpy(pnp_outlier, L.outl + (size_t)i * KC, m, hipMemcpyDeviceToHost));
    if (proj && nL) HIPCHK(hipMemcpy(proj, L.proj + (size_t)i * nL * 3, nL * 12, hipMemcpyDeviceToHost));
    return cnt > cap ? fail(ODO_ERR_CAPACITY, "cap too small") : ODO_OK;
}

int odo_kabsch(const float* A, const float* B, int n, float T[16]) {
    if (n < 0 || (n && (!A || !B)) || !T) return fail(ODO_ERR_ARG, "bad kabsch args");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(ODO_ERR_DEVICE, "no HIP device");
    const int kc = std::max(n, 1);
    // Kabsch::Compute takes no context: one process-wide arena, one caller at a time
    static std::mutex mu;
    static DevArena KA;
    std::lock_guard<std::mutex> lock(mu);
    KA.begin();
    DevBuf da(KA, (size_t)kc * 12), db(KA, (size_t)kc * 12), dT(KA, 64);
    ARENA_CHECK(KA);
    if (n) {
        HIPCHK(hipMemcpy(da.p, A, (size_t)n * 12, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db.p, B, (size_t)n * 12, hipMemcpyHostToDevice));
    }
    launch_kabsch(0, da.as<float>(), db.as<float>(), n, dT.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(T, dT.p, 64, hipMemcpyDeviceToHost));
    return ODO_OK;
}

}  // extern "C"
