// GICP over whole clouds (include/odo.h: odo_gicp_grid_batch,
// odo_gicp_grid_covariances, odo_gicp_dense): the neighbour searches of
// k_gicp.hip over a uniform grid per cloud instead of the brute-force scans, with
// the same results bit for bit (DESIGN §4 "Dense GICP"). One launch chain serves
// the three entry points: the clouds of a call packed one after the other on the
// device, their bounds (one host round trip: the grids are sized from them),
// the counting sort, the covariances once per cloud, the ICP workgroups.
#include "odo_ctx.h"

namespace odo {

namespace {

// the ICP rings of a grid of cell width w: the first r whose bound reaches
// max_corr_dist^2 (every point beyond ring r is then too far to correspond)
int icp_rings(double w, double slack, double mcd, int max_dim) {
    double r = std::ceil((mcd * (1.0 + 0x1p-19) + slack) / w);
    if (!(r >= 1)) r = 1;
    if (r >= max_dim) return std::max(max_dim, 1);  // the whole grid
    int ri = (int)r;
    while (ri < max_dim && gg_ring_bound(w, slack, ri) < mcd * mcd) ri++;
    return ri;
}

// The grid of one cloud from its bounds (the cell rule). forced > 0:
// that cell or ODO_ERR_CAPACITY; else about 8 cells per point of a cubic cloud,
// not below max_corr_dist (plus the stop rule's slack, so that the ICP search
// is one ring), doubled until the table fits GG_MAX_CELLS.
int plan_grid(const float* mn, const float* mx, int n, float forced, double mcd, GgCloud* g, int64_t* ncells) {
    g->gx = g->gy = g->gz = 0;
    g->inv = 0.f;
    g->w = g->slack = 0;
    g->rings = 1;
    *ncells = 0;
    for (int a = 0; a < 3; a++) g->mn[a] = n ? mn[a] : 0.f;
    if (n == 0) return ODO_OK;
    double emax = 0;
    for (int a = 0; a < 3; a++) emax = std::max(emax, (double)mx[a] - (double)mn[a]);
    // a span beyond FLT_MAX: fl(x - min) overflows, so no cell edge bins such a
    // cloud; one cell holds it (the searches then see every point), and so does
    // a cell that the doubling below has taken out of the float range
    bool span_ok = true;
    for (int a = 0; a < 3; a++) span_ok = span_ok && std::isfinite(mx[a] - mn[a]);
    auto one_cell = [&]() {
        g->gx = g->gy = g->gz = 1;
        g->inv = 0.f;  // every t is 0 (or NaN, which the kernels clamp to 0)
        g->w = emax + 1.0;
        g->slack = 0;
        g->rings = 1;
        *ncells = 1;
        return ODO_OK;
    };
    if (!span_ok) {
        if (forced > 0) return fail(ODO_ERR_CAPACITY, "gicp_grid: the cloud spans more than FLT_MAX, no forced cell fits");
        return one_cell();
    }
    float cell = forced;
    if (!(forced > 0)) {
        double cd = std::max(emax / std::cbrt(8.0 * n), mcd * (1.0 + 0x1p-10) + 4.0 * (emax + mcd) * 0x1p-21);
        if (!(cd > 0)) cd = 1.0;  // coincident points and no correspondence distance: one cell
        cell = (float)cd;
        if (!(cell > 0) || !std::isfinite(cell)) cell = 1.f;
    }
    for (;;) {
        const float inv = 1.0f / cell;
        bool fits = std::isfinite(inv) && inv > 0;
        int dim[3] = {1, 1, 1};
        double prod = 1;
        for (int a = 0; a < 3 && fits; a++) {
            const float e = mx[a] - mn[a];
            const float t = floorf(e * inv);  // the kernels' cell of the largest coordinate
            if (!(t < (float)GG_MAX_CELLS)) fits = false;
            else dim[a] = (int)t + 1;
            prod *= dim[a];
        }
        if (fits && prod > (double)GG_MAX_CELLS) fits = false;
        const double w = fits ? 1.0 / (double)inv : 0, slack = (emax + w) * 0x1p-21;
        const int maxd = std::max(dim[0], std::max(dim[1], dim[2]));
        const int rings = fits ? icp_rings(w, slack, mcd, maxd) : 0;
        if (!fits || (!(forced > 0) && rings > 1 && maxd > 1)) {
            if (forced > 0) return fail(ODO_ERR_CAPACITY, "gicp_grid: the cell table of the forced cell exceeds 2^24 cells");
            cell *= fits ? 1.0009765625f : 2.0f;  // automatic: coarser never changes a result
            if (!std::isfinite(cell)) return one_cell();
            continue;
        }
        g->gx = dim[0];
        g->gy = dim[1];
        g->gz = dim[2];
        g->inv = inv;
        g->w = w;
        g->slack = slack;
        g->rings = rings;
        *ncells = (int64_t)prod;
        return ODO_OK;
    }
}

// where the points of a call come from
struct Source {
    const float* host[2] = {nullptr, nullptr};  // packed host rows, uploaded one after the other
    size_t host_rows[2] = {0, 0};
    const float* dev = nullptr;  // or device rows of `stride` floats: cloud k starts at row0[k]
    int stride = 0;
    std::vector<int32_t> row0;
};

// offs: ncl + 1 first rows of the clouds in the packed sequence. pairs / guesses /
// T12 ... (nprob) or C (covariances in point order), not both.
int run(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, std::vector<GgPair>& pairs,
        const float* guesses, int max_iterations, double mcd, float cell, float* T12, int32_t* converged,
        int32_t* iterations, int32_t* n_corr, double* C) {
    const int ncl = (int)offs.size() - 1, nprob = (int)pairs.size();
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl, NP = (size_t)nprob;
    int max_n = 0;
    for (int k = 0; k < ncl; k++) max_n = std::max(max_n, offs[k + 1] - offs[k]);
    size_t W = 0;
    for (auto& p : pairs) {
        if (W > ((size_t)1 << 30)) return fail(ODO_ERR_CAPACITY, "gicp_grid: more than 2^30 source points over the pairs");
        p.work = (int)W;
        W += (size_t)(offs[p.s + 1] - offs[p.s]);
    }
    Pack pk;
    const size_t o_P = pk.add(N * 12), o_offs = pk.add((NC + 1) * 4), o_row0 = pk.add(NC * 4),
                 o_bounds = pk.add(NC * 24), o_cl = pk.add(NC * sizeof(GgCloud)), o_pairs = pk.add(NP * sizeof(GgPair)),
                 o_guess = pk.add(NP * 64), o_key = pk.add(N * 4), o_sorted = pk.add(N * 16), o_C = pk.add(N * 72),
                 o_outp = pk.add(W * 12), o_Mah = pk.add(W * 72), o_is = pk.add(W * 4), o_it = pk.add(W * 4),
                 o_T = pk.add(NP * 64), o_io = pk.add(NP * 16);
    int e;
    if ((e = c->gg_pts.reserve(pk.off, 256, "gicp_grid"))) return e;
    uint8_t* d = c->gg_pts.p;
    hipStream_t st = c->stream;
    float* dP = (float*)(d + o_P);
    int* doffs = (int*)(d + o_offs);
    HIPCHK(hipMemcpyAsync(doffs, offs.data(), (NC + 1) * 4, hipMemcpyHostToDevice, st));
    if (src.dev) {
        if (ncl) HIPCHK(hipMemcpyAsync(d + o_row0, src.row0.data(), NC * 4, hipMemcpyHostToDevice, st));
        launch_gg_pack(st, src.dev, src.stride, (const int*)(d + o_row0), doffs, ncl, max_n, dP);
    } else {
        size_t at = 0;
        for (int k = 0; k < 2; k++) {
            if (src.host_rows[k])
                HIPCHK(hipMemcpyAsync(dP + 3 * at, src.host[k], src.host_rows[k] * 12, hipMemcpyHostToDevice, st));
            at += src.host_rows[k];
        }
    }
    std::vector<uint32_t> hb(6 * NC);
    for (size_t k = 0; k < NC; k++)
        for (int a = 0; a < 6; a++) hb[6 * k + a] = a < 3 ? 0xffffffffu : 0u;
    if (ncl) HIPCHK(hipMemcpyAsync(d + o_bounds, hb.data(), NC * 24, hipMemcpyHostToDevice, st));
    launch_gg_bounds(st, dP, doffs, ncl, max_n, (uint32_t*)(d + o_bounds));
    HIPCHK(hipGetLastError());
    if (ncl) HIPCHK(hipMemcpyAsync(hb.data(), d + o_bounds, NC * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the grids
    std::vector<GgCloud> cl(NC);
    int64_t total = 0;
    for (int k = 0; k < ncl; k++) {
        float mn[3], mx[3];
        const int n = offs[k + 1] - offs[k];
        for (int a = 0; a < 3; a++) {
            mn[a] = gg_decode(hb[6 * (size_t)k + a]);
            mx[a] = gg_decode(hb[6 * (size_t)k + 3 + a]);
            if (n && (!std::isfinite(mn[a]) || !std::isfinite(mx[a])))
                return fail(ODO_ERR_DEVICE, "gicp_grid: a cloud holds a non-finite coordinate");
        }
        int64_t nc;
        if ((e = plan_grid(mn, mx, n, cell, mcd, &cl[k], &nc))) return e;
        cl[k].p0 = offs[k];
        cl[k].n = n;
        cl[k].c0 = (int)total;
        total += nc;
        if (total > GG_MAX_TOTAL_CELLS) return fail(ODO_ERR_CAPACITY, "gicp_grid: more than 2^28 cells over the clouds of a call");
    }
    const size_t M = (size_t)total + 1, NB = (M + 4095) / 4096;
    Pack pc;
    const size_t o_cnt = pc.add(M * 4), o_fill = pc.add(M * 4), o_bsum = pc.add(NB * 4);
    if ((e = c->gg_cells.reserve(pc.off, 0, "gicp_grid"))) return e;
    uint8_t* dc = c->gg_cells.p;
    HIPCHK(hipMemsetAsync(dc, 0, o_bsum, st));  // cnt and fill
    if (ncl) HIPCHK(hipMemcpyAsync(d + o_cl, cl.data(), NC * sizeof(GgCloud), hipMemcpyHostToDevice, st));
    const GgCloud* dcl = (const GgCloud*)(d + o_cl);
    int* cstart = (int*)(dc + o_cnt);
    float4* sorted = (float4*)(d + o_sorted);
    double* dC = (double*)(d + o_C);
    launch_gg_build(st, dP, dcl, ncl, max_n, total, (int*)(d + o_key), cstart, (int*)(dc + o_fill),
                    (int*)(dc + o_bsum), sorted);
    if (C && N) HIPCHK(hipMemsetAsync(dC, 0, N * 72, st));  // clouds under 20 points: zeros
    launch_gg_cov(st, dP, dcl, ncl, max_n, cstart, sorted, dC);
    HIPCHK(hipGetLastError());
    if (C) {
        if (N) HIPCHK(hipMemcpyAsync(C, dC, N * 72, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return ODO_OK;
    }
    std::vector<float> g(16 * NP);
    for (size_t p = 0; p < NP; p++)
        for (int i = 0; i < 16; i++) g[16 * p + i] = guesses ? guesses[16 * p + i] : (i % 5 == 0 ? 1.f : 0.f);
    HIPCHK(hipMemcpyAsync(d + o_guess, g.data(), NP * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d + o_pairs, pairs.data(), NP * sizeof(GgPair), hipMemcpyHostToDevice, st));
    launch_gg_icp(st, dP, dcl, (const GgPair*)(d + o_pairs), nprob, cstart, sorted, dC, (float*)(d + o_outp),
                  (double*)(d + o_Mah), (int*)(d + o_is), (int*)(d + o_it), (const float*)(d + o_guess), mcd,
                  max_iterations, 20 /* PCL inner */, (float*)(d + o_T), (int*)(d + o_io));
    HIPCHK(hipGetLastError());
    std::vector<float> hT(16 * NP);
    std::vector<int> io(4 * NP);
    HIPCHK(hipMemcpyAsync(hT.data(), d + o_T, NP * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(io.data(), d + o_io, NP * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(T12, hT.data(), NP * 64);
    for (size_t p = 0; p < NP; p++) {
        converged[p] = io[4 * p];
        iterations[p] = io[4 * p + 1];
        n_corr[p] = io[4 * p + 2];
    }
    return ODO_OK;
}

bool all_finite(const float* v, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// offsets of one side: start at 0, do not decrease, clouds within the limit
int check_offs(const int32_t* offs, int nprob, const char* who) {
    if (offs[0] != 0) return fail(ODO_ERR_ARG, std::string(who) + ": offsets must start at 0");
    for (int p = 0; p < nprob; p++)
        if (offs[p + 1] < offs[p]) return fail(ODO_ERR_ARG, std::string(who) + ": offsets must not decrease");
    for (int p = 0; p < nprob; p++)
        if (offs[p + 1] - offs[p] > GG_MAX_POINTS)
            return fail(ODO_ERR_CAPACITY, std::string(who) + ": more than 1048576 points in a cloud");
    return ODO_OK;
}

int check_icp_params(int max_iterations, double mcd, const float* guesses, int nprob, const char* who) {
    if (max_iterations < 1) return fail(ODO_ERR_ARG, std::string(who) + ": max_iterations < 1");
    if (!(mcd >= 0) || !std::isfinite(mcd))
        return fail(ODO_ERR_ARG, std::string(who) + ": max_corr_dist must be finite and >= 0");
    if (guesses && !all_finite(guesses, 16 * (size_t)nprob)) return fail(ODO_ERR_ARG, std::string(who) + ": a guess is not finite");
    return ODO_OK;
}

}  // namespace
}  // namespace odo

extern "C" {

int odo_gicp_grid_batch(odo_ctx* c, const float* src, const int32_t* soffs, const float* tgt, const int32_t* toffs,
                        const float* guesses, int nprob, int max_iterations, double max_corr_dist, float cell,
                        float* T12, int32_t* converged, int32_t* iterations, int32_t* n_corr) {
    const char* who = "gicp_grid_batch";
    if (!c || nprob < 0 || !soffs || !toffs || (nprob && (!T12 || !converged || !iterations || !n_corr)))
        return fail(ODO_ERR_ARG, "bad gicp_grid_batch args");
    int e;
    if ((e = check_icp_params(max_iterations, max_corr_dist, guesses, nprob, who))) return e;
    if (!(cell >= 0) || !std::isfinite(cell)) return fail(ODO_ERR_ARG, "gicp_grid_batch: cell must be finite and >= 0");
    if (nprob == 0) return ODO_OK;
    // a cloud is a grid row (at most 65535 of them in a launch)
    if (nprob > 32767) return fail(ODO_ERR_CAPACITY, "gicp_grid_batch: more than 32767 pairs per call");
    if ((e = check_offs(soffs, nprob, who)) || (e = check_offs(toffs, nprob, who))) return e;
    const size_t S = (size_t)soffs[nprob], T = (size_t)toffs[nprob];
    if ((S && !src) || (T && !tgt)) return fail(ODO_ERR_ARG, "bad gicp_grid_batch args");
    if (S + T > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "gicp_grid_batch: more than 2^29 points per call");
    if (!all_finite(src, 3 * S) || !all_finite(tgt, 3 * T))
        return fail(ODO_ERR_ARG, "gicp_grid_batch: a coordinate is not finite");
    if ((e = sync_all(c))) return e;
    // clouds: the sources, then the targets
    std::vector<int32_t> offs(2 * (size_t)nprob + 1);
    std::vector<GgPair> pairs((size_t)nprob);
    for (int p = 0; p <= nprob; p++) offs[p] = soffs[p];
    for (int p = 1; p <= nprob; p++) offs[(size_t)nprob + p] = (int32_t)(S + (size_t)toffs[p]);
    for (int p = 0; p < nprob; p++) pairs[p] = GgPair{p, nprob + p, 0};
    Source s;
    s.host[0] = src;
    s.host_rows[0] = S;
    s.host[1] = tgt;
    s.host_rows[1] = T;
    return run(c, s, offs, pairs, guesses, max_iterations, max_corr_dist, cell, T12, converged, iterations, n_corr,
               nullptr);
}

int odo_gicp_grid_covariances(odo_ctx* c, const float* P, const int32_t* offs, int nprob, float cell, double* C) {
    const char* who = "gicp_grid_covariances";
    if (!c || nprob < 0 || !offs) return fail(ODO_ERR_ARG, "bad gicp_grid_covariances args");
    if (!(cell >= 0) || !std::isfinite(cell))
        return fail(ODO_ERR_ARG, "gicp_grid_covariances: cell must be finite and >= 0");
    if (nprob == 0) return ODO_OK;
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "gicp_grid_covariances: more than 65535 clouds per call");
    int e;
    if ((e = check_offs(offs, nprob, who))) return e;
    const size_t N = (size_t)offs[nprob];
    if (N == 0) return ODO_OK;
    if (!P || !C) return fail(ODO_ERR_ARG, "bad gicp_grid_covariances args");
    if (N > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "gicp_grid_covariances: more than 2^29 points per call");
    if (!all_finite(P, 3 * N)) return fail(ODO_ERR_ARG, "gicp_grid_covariances: a coordinate is not finite");
    if ((e = sync_all(c))) return e;
    std::vector<int32_t> o(offs, offs + nprob + 1);
    std::vector<GgPair> none;
    Source s;
    s.host[0] = P;
    s.host_rows[0] = N;
    return run(c, s, o, none, nullptr, 1, 0.0, cell, nullptr, nullptr, nullptr, nullptr, C);
}

int odo_gicp_dense(odo_ctx* c, const int32_t* pairs, int nprob, const float* guesses, int max_iterations,
                   double max_corr_dist, float* T12, int32_t* converged, int32_t* iterations, int32_t* n_corr) {
    const char* who = "gicp_dense";
    if (!c) return fail(ODO_ERR_ARG, "gicp_dense: null ctx");
    if (c->cloud_n < 0) return fail(ODO_ERR_STATE, "gicp_dense: no dense-cloud call yet");
    if (nprob < 0 || (nprob && (!pairs || !T12 || !converged || !iterations || !n_corr)))
        return fail(ODO_ERR_ARG, "bad gicp_dense args");
    int e;
    if ((e = check_icp_params(max_iterations, max_corr_dist, guesses, nprob, who))) return e;
    for (int k = 0; k < 2 * nprob; k++)
        if (pairs[k] < 0 || pairs[k] >= c->cloud_n)
            return fail(ODO_ERR_ARG, "gicp_dense: frame outside the last dense-cloud call");
    if (nprob == 0) return ODO_OK;
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "gicp_dense: more than 65535 pairs per call");
    if ((e = sync_all(c))) return e;
    // the distinct frames, in the order they are named: one grid and one set of
    // covariances each
    if (c->cloud_n > 65535) return fail(ODO_ERR_CAPACITY, "gicp_dense: more than 65535 frames in the dense-cloud call");
    std::vector<int> cloud_of((size_t)c->cloud_n, -1);
    std::vector<int32_t> offs(1, 0);
    std::vector<GgPair> pr((size_t)nprob);
    Source s;
    s.dev = (const float*)c->cloud_out.p;
    s.stride = (int)(sizeof(odo_cloud_point) / 4);
    for (int k = 0; k < 2 * nprob; k++) {
        const int f = pairs[k];
        if (cloud_of[f] < 0) {
            if (c->cloud_np[f] > GG_MAX_POINTS) return fail(ODO_ERR_CAPACITY, "gicp_dense: more than 1048576 points in a cloud");
            if ((size_t)offs.back() + (size_t)c->cloud_np[f] > (size_t)INT32_MAX / 4)
                return fail(ODO_ERR_CAPACITY, "gicp_dense: more than 2^29 points per call");
            cloud_of[f] = (int)offs.size() - 1;
            s.row0.push_back(c->cloud_off[f]);
            offs.push_back(offs.back() + c->cloud_np[f]);
        }
        (k & 1 ? pr[k / 2].t : pr[k / 2].s) = cloud_of[f];
    }
    return run(c, s, offs, pr, guesses, max_iterations, max_corr_dist, 0.f, T12, converged, iterations, n_corr,
               nullptr);
}

}  // extern "C"
