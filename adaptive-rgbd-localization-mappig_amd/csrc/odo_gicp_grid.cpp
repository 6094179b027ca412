// GICP over whole clouds (include/odo.h: odo_gicp_grid_batch,
// odo_gicp_grid_covariances, odo_gicp_dense): the neighbour searches of
// k_gicp.hip over a uniform grid per cloud instead of the brute-force scans, with
// the same results bit for bit (DESIGN §4 "Dense GICP"). One launch chain serves
// the three entry points: the clouds of a call packed one after the other on the
// device, their bounds (one host round trip: the grids are sized from them),
// the counting sort, the covariances once per cloud, the ICP workgroups.
#include "odo_ctx.h"
#include "odo_wave.h"

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
// that cell or ODO_ERR_CAPACITY; else about per_point cells per point of a cubic
// cloud (8 for GICP's 20 neighbours), not below max_corr_dist (plus the stop
// rule's slack, so that the ICP search is one ring), doubled until the table
// fits GG_MAX_CELLS.
int plan_grid(const float* mn, const float* mx, int n, float forced, double mcd, GgCloud* g, int64_t* ncells,
              double per_point = 8.0) {
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
        double cd = std::max(emax / std::cbrt(per_point * n), mcd * (1.0 + 0x1p-10) + 4.0 * (emax + mcd) * 0x1p-21);
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

// the sections of gg_pts that every call has; the caller adds its own after them
struct GridSections {
    size_t o_P, o_offs, o_row0, o_bounds, o_cl, o_key, o_sorted;
    GridSections(Pack& pk, size_t N, size_t NC)
        : o_P(pk.add(N * 12)), o_offs(pk.add((NC + 1) * 4)), o_row0(pk.add(NC * 4)), o_bounds(pk.add(NC * 24)),
          o_cl(pk.add(NC * sizeof(GgCloud))), o_key(pk.add(N * 4)), o_sorted(pk.add(N * 16)) {}
};
struct Grids {
    uint8_t* d = nullptr;  // gg_pts, reserved for `bytes`
    float* dP = nullptr;
    const GgCloud* dcl = nullptr;
    int* cstart = nullptr;
    float4* sorted = nullptr;
    int max_n = 0;
};

// The first half of every launch chain: the clouds of `offs` (ncl + 1 first rows
// in the packed sequence) packed on the device, their bounds (the host round
// trip), the grids by the cell rule (mcd, per_point) and the counting sort.
int build_grids(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, const GridSections& gs, size_t bytes,
                float cell, double mcd, double per_point, const char* who, Grids* G) {
    const int ncl = (int)offs.size() - 1;
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl;
    int max_n = 0;
    for (int k = 0; k < ncl; k++) max_n = std::max(max_n, offs[k + 1] - offs[k]);
    int e;
    if ((e = c->gg_pts.reserve(bytes, 256, who))) return e;
    uint8_t* d = c->gg_pts.p;
    hipStream_t st = c->stream;
    float* dP = (float*)(d + gs.o_P);
    int* doffs = (int*)(d + gs.o_offs);
    HIPCHK(hipMemcpyAsync(doffs, offs.data(), (NC + 1) * 4, hipMemcpyHostToDevice, st));
    if (src.dev) {
        if (ncl) HIPCHK(hipMemcpyAsync(d + gs.o_row0, src.row0.data(), NC * 4, hipMemcpyHostToDevice, st));
        launch_gg_pack(st, src.dev, src.stride, (const int*)(d + gs.o_row0), doffs, ncl, max_n, dP);
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
    if (ncl) HIPCHK(hipMemcpyAsync(d + gs.o_bounds, hb.data(), NC * 24, hipMemcpyHostToDevice, st));
    launch_gg_bounds(st, dP, doffs, ncl, max_n, (uint32_t*)(d + gs.o_bounds));
    HIPCHK(hipGetLastError());
    if (ncl) HIPCHK(hipMemcpyAsync(hb.data(), d + gs.o_bounds, NC * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the grids
    std::vector<GgCloud> cl(NC);
    int64_t total = 0;
    for (int k = 0; k < ncl; k++) {
        float mn[3], mx[3];
        const int n = offs[k + 1] - offs[k];
        for (int a = 0; a < 3; a++) {
            mn[a] = f32_unordered(hb[6 * (size_t)k + a]);
            mx[a] = f32_unordered(hb[6 * (size_t)k + 3 + a]);
            if (n && (!std::isfinite(mn[a]) || !std::isfinite(mx[a])))
                return fail(ODO_ERR_DEVICE, std::string(who) + ": a cloud holds a non-finite coordinate");
        }
        int64_t nc;
        if ((e = plan_grid(mn, mx, n, cell, mcd, &cl[k], &nc, per_point))) return e;
        cl[k].p0 = offs[k];
        cl[k].n = n;
        cl[k].c0 = (int)total;
        total += nc;
        if (total > GG_MAX_TOTAL_CELLS)
            return fail(ODO_ERR_CAPACITY, std::string(who) + ": more than 2^28 cells over the clouds of a call");
    }
    const size_t M = (size_t)total + 1, NB = (M + 4095) / 4096;
    Pack pc;
    const size_t o_cnt = pc.add(M * 4), o_fill = pc.add(M * 4), o_bsum = pc.add(NB * 4);
    if ((e = c->gg_cells.reserve(pc.off, 0, who))) return e;
    uint8_t* dc = c->gg_cells.p;
    HIPCHK(hipMemsetAsync(dc, 0, o_bsum, st));  // cnt and fill
    if (ncl) HIPCHK(hipMemcpyAsync(d + gs.o_cl, cl.data(), NC * sizeof(GgCloud), hipMemcpyHostToDevice, st));
    G->d = d;
    G->dP = dP;
    G->dcl = (const GgCloud*)(d + gs.o_cl);
    G->cstart = (int*)(dc + o_cnt);
    G->sorted = (float4*)(d + gs.o_sorted);
    G->max_n = max_n;
    launch_gg_build(st, dP, G->dcl, ncl, max_n, total, (int*)(d + gs.o_key), G->cstart, (int*)(dc + o_fill),
                    (int*)(dc + o_bsum), G->sorted);
    HIPCHK(hipGetLastError());
    return ODO_OK;
}

// the first row of every pair's own rows (sized by its source) in p.work; the total in *W
int pair_rows(const std::vector<int32_t>& offs, std::vector<GgPair>& pairs, const char* who, size_t* W) {
    *W = 0;
    for (auto& p : pairs) {
        if (*W > ((size_t)1 << 30)) return fail(ODO_ERR_CAPACITY, std::string(who) + ": more than 2^30 source points over the pairs");
        p.work = (int)*W;
        *W += (size_t)(offs[p.s + 1] - offs[p.s]);
    }
    return ODO_OK;
}

// GICP. pairs / guesses / T12 ... (nprob) or C (covariances in point order), not both.
int run(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, std::vector<GgPair>& pairs,
        const float* guesses, int max_iterations, double mcd, float cell, float* T12, int32_t* converged,
        int32_t* iterations, int32_t* n_corr, double* C) {
    const int ncl = (int)offs.size() - 1, nprob = (int)pairs.size();
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl, NP = (size_t)nprob;
    size_t W;
    int e;
    if ((e = pair_rows(offs, pairs, "gicp_grid", &W))) return e;
    Pack pk;
    const GridSections gs(pk, N, NC);
    const size_t o_pairs = pk.add(NP * sizeof(GgPair)), o_guess = pk.add(NP * 64), o_C = pk.add(N * 72),
                 o_outp = pk.add(W * 12), o_Mah = pk.add(W * 72), o_is = pk.add(W * 4), o_it = pk.add(W * 4),
                 o_T = pk.add(NP * 64), o_io = pk.add(NP * 16);
    Grids G;
    if ((e = build_grids(c, src, offs, gs, pk.off, cell, mcd, 8.0, "gicp_grid", &G))) return e;
    uint8_t* d = G.d;
    hipStream_t st = c->stream;
    float* dP = G.dP;
    const GgCloud* dcl = G.dcl;
    int* cstart = G.cstart;
    float4* sorted = G.sorted;
    const int max_n = G.max_n;
    double* dC = (double*)(d + o_C);
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

// The SOR cell rule (DESIGN §4 "SOR and fitness"): GICP's 8 cells per point
// serve 20 neighbours, so mean_k + 1 neighbours get 8 * 20 / (mean_k + 1), at
// most 16 (the table budget). A speed choice: no result depends on the cell.
double sor_cells_per_point(int mean_k) { return std::min(16.0, 160.0 / (mean_k + 1.0)); }
constexpr double FIT_CELLS_PER_POINT = 16.0;  // one neighbour

int check_sor_params(int mean_k, double stddev_mul, const char* who) {
    if (mean_k < 1) return fail(ODO_ERR_ARG, std::string(who) + ": mean_k < 1");
    if (!std::isfinite(stddev_mul)) return fail(ODO_ERR_ARG, std::string(who) + ": stddev_mul must be finite");
    if (mean_k > SOR_MAX_K) return fail(ODO_ERR_CAPACITY, std::string(who) + ": mean_k above 64");
    return ODO_OK;
}

// StatisticalOutlierRemoval of the clouds of `offs`. Host clouds: keep /
// distances (may be null) come back. Device clouds (dense): the kept rows of
// c->cloud_out are packed frame after frame and the context's offsets follow.
int run_sor(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, int mean_k, double stddev_mul, float cell,
            const char* who, uint8_t* keep, float* distances, odo_sor_info* info) {
    const int ncl = (int)offs.size() - 1;
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl;
    int max_n = 0;
    for (int k = 0; k < ncl; k++) max_n = std::max(max_n, offs[k + 1] - offs[k]);
    const size_t nchunk = ((size_t)max_n + 255) / 256;
    const bool dense = src.dev != nullptr;
    Pack pk;
    const GridSections gs(pk, N, NC);
    const size_t o_dist = pk.add(N * 4), o_keep = pk.add(N), o_stats = pk.add(NC * sizeof(SorStats)),
                 o_chunk = pk.add(NC * nchunk * 4), o_new0 = pk.add(NC * 4),
                 o_pts = pk.add(dense ? N * sizeof(odo_cloud_point) : 0), o_cnt = pk.add(dense ? N * 4 : 0);
    Grids G;
    int e;
    if ((e = build_grids(c, src, offs, gs, pk.off, cell, 0.0, sor_cells_per_point(mean_k), who, &G))) return e;
    uint8_t* d = G.d;
    hipStream_t st = c->stream;
    float* ddist = (float*)(d + o_dist);
    SorStats* dstats = (SorStats*)(d + o_stats);
    if (N) HIPCHK(hipMemsetAsync(ddist, 0, N * 4, st));  // skipped clouds: zeros
    HIPCHK(hipMemsetAsync(dstats, 0, NC * sizeof(SorStats), st));
    launch_sor(st, G.dcl, ncl, max_n, G.cstart, G.sorted, mean_k, stddev_mul, ddist, dstats, d + o_keep,
               (int*)(d + o_chunk));
    HIPCHK(hipGetLastError());
    std::vector<SorStats> hs(NC);
    HIPCHK(hipMemcpyAsync(hs.data(), dstats, NC * sizeof(SorStats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (dense) {
        std::vector<int32_t> off(NC + 1, 0), np(NC, 0);
        for (int k = 0; k < ncl; k++) {
            np[k] = hs[k].n_out;
            off[(size_t)k + 1] = off[k] + np[k];
        }
        const size_t kept = (size_t)off[NC];
        if (kept != N) {  // else nothing moves
            odo_cloud_point* pts = (odo_cloud_point*)c->cloud_out.p;
            int32_t* cnt = (int32_t*)(c->cloud_out.p + c->cloud_counts_at);
            HIPCHK(hipMemcpyAsync(d + o_new0, off.data(), NC * 4, hipMemcpyHostToDevice, st));
            // row0 (gs.o_row0) still holds the frames' first rows of cloud_out
            launch_sor_pack(st, G.dcl, ncl, max_n, d + o_keep, (const int*)(d + o_chunk), (const int*)(d + gs.o_row0),
                            (const int*)(d + o_new0), pts, cnt, d + o_pts, (int*)(d + o_cnt));
            HIPCHK(hipGetLastError());
            if (kept) {
                HIPCHK(hipMemcpyAsync(pts, d + o_pts, kept * sizeof(odo_cloud_point), hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(cnt, d + o_cnt, kept * 4, hipMemcpyDeviceToDevice, st));
            }
            HIPCHK(hipStreamSynchronize(st));
            c->cloud_off.swap(off);
            c->cloud_np.swap(np);
        }
    } else {
        if (N) HIPCHK(hipMemcpyAsync(keep, d + o_keep, N, hipMemcpyDeviceToHost, st));
        if (N && distances) HIPCHK(hipMemcpyAsync(distances, ddist, N * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    for (int k = 0; k < ncl; k++) {
        const int n = offs[k + 1] - offs[k];
        info[k].status = n <= mean_k ? ODO_SOR_SKIPPED : ODO_SOR_OK;
        info[k].n_in = n;
        info[k].n_out = hs[k].n_out;
        info[k].pad = 0;
        info[k].mean = hs[k].mean;
        info[k].stddev = hs[k].stddev;
        info[k].threshold = hs[k].threshold;
    }
    return ODO_OK;
}

// getFitnessScore of the pairs over the clouds of `offs`; nn_d2 (may be null)
// in pair order, sized by the sources
int run_fitness(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, std::vector<GgPair>& pairs,
                const float* T, float cell, const char* who, double* score, float* nn_d2) {
    const int ncl = (int)offs.size() - 1, nprob = (int)pairs.size();
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl, NP = (size_t)nprob;
    size_t W;
    int e;
    if ((e = pair_rows(offs, pairs, who, &W))) return e;
    int max_ns = 0;
    for (auto& p : pairs) max_ns = std::max(max_ns, offs[p.s + 1] - offs[p.s]);
    Pack pk;
    const GridSections gs(pk, N, NC);
    const size_t o_pairs = pk.add(NP * sizeof(GgPair)), o_T = pk.add(NP * 64), o_nn = pk.add(W * 4),
                 o_score = pk.add(NP * 8);
    Grids G;
    if ((e = build_grids(c, src, offs, gs, pk.off, cell, 0.0, FIT_CELLS_PER_POINT, who, &G))) return e;
    uint8_t* d = G.d;
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(d + o_pairs, pairs.data(), NP * sizeof(GgPair), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d + o_T, T, NP * 64, hipMemcpyHostToDevice, st));
    if (W) HIPCHK(hipMemsetAsync(d + o_nn, 0, W * 4, st));  // an empty target: no row is written
    launch_gg_fitness(st, G.dcl, (const GgPair*)(d + o_pairs), nprob, max_ns, G.cstart, G.sorted,
                      (const float*)(d + o_T), (float*)(d + o_nn), (double*)(d + o_score));
    HIPCHK(hipGetLastError());
    std::vector<double> hs(NP);
    HIPCHK(hipMemcpyAsync(hs.data(), d + o_score, NP * 8, hipMemcpyDeviceToHost, st));
    if (nn_d2 && W) HIPCHK(hipMemcpyAsync(nn_d2, d + o_nn, W * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(score, hs.data(), NP * 8);
    return ODO_OK;
}

// The ICP cell rule: the same table budget as SOR's for num_neighbors
// neighbours; the one-neighbour sweeps share the grid. A speed choice.
double icp_cells_per_point(int num_neighbors) { return std::min(16.0, 160.0 / num_neighbors); }

int check_icp_plane_params(const odo_icp_params* p, const float* guesses, int nprob, const char* who) {
    if (!p) return fail(ODO_ERR_ARG, std::string(who) + ": null params");
    if (p->num_neighbors < 3) return fail(ODO_ERR_ARG, std::string(who) + ": num_neighbors < 3");
    if (p->max_iterations < 0) return fail(ODO_ERR_ARG, std::string(who) + ": max_iterations < 0");
    if (!std::isfinite(p->min_delta) || !std::isfinite(p->indist))
        return fail(ODO_ERR_ARG, std::string(who) + ": min_delta and indist must be finite");
    if (p->gate != ODO_ICP_GATE_AS_WRITTEN && p->gate != ODO_ICP_GATE_PLANE)
        return fail(ODO_ERR_ARG, std::string(who) + ": unknown gate");
    if (guesses && !all_finite(guesses, 16 * (size_t)nprob)) return fail(ODO_ERR_ARG, std::string(who) + ": a guess is not finite");
    if (p->num_neighbors > ICP_MAX_K) return fail(ODO_ERR_CAPACITY, std::string(who) + ": num_neighbors above 32");
    return ODO_OK;
}

// IcpPointToPlane. pairs (s = template, t = model) / guesses / out (nprob), or
// normals (of every cloud, in point order), not both.
int run_icp(odo_ctx* c, const Source& src, const std::vector<int32_t>& offs, std::vector<GgPair>& pairs,
            const float* guesses, const odo_icp_params& prm, float cell, const char* who, odo_icp_result* out,
            float* normals) {
    const int ncl = (int)offs.size() - 1, nprob = (int)pairs.size();
    const size_t N = (size_t)offs[ncl], NC = (size_t)ncl, NP = (size_t)nprob;
    size_t W;
    int e;
    if ((e = pair_rows(offs, pairs, who, &W))) return e;
    int max_ns = 0;
    for (auto& p : pairs) max_ns = std::max(max_ns, offs[p.s + 1] - offs[p.s]);
    std::vector<int32_t> need(NC, normals ? 1 : 0);
    for (auto& p : pairs) need[p.t] = 1;
    Pack pk;
    const GridSections gs(pk, N, NC);
    const size_t o_need = pk.add(NC * 4), o_nrm = pk.add(N * 12), o_pairs = pk.add(NP * sizeof(GgPair)),
                 o_state = pk.add(NP * sizeof(IcpState)), o_left = pk.add(4), o_rows = pk.add(W * 32);
    Grids G;
    if ((e = build_grids(c, src, offs, gs, pk.off, cell, 0.0, icp_cells_per_point(prm.num_neighbors), who, &G))) return e;
    uint8_t* d = G.d;
    hipStream_t st = c->stream;
    float* dnrm = (float*)(d + o_nrm);
    if (ncl) HIPCHK(hipMemcpyAsync(d + o_need, need.data(), NC * 4, hipMemcpyHostToDevice, st));
    if (N) HIPCHK(hipMemsetAsync(dnrm, 0, N * 12, st));  // clouds under 5 points: zeros
    launch_icp_normals(st, G.dP, G.dcl, (const int*)(d + o_need), ncl, G.max_n, G.cstart, G.sorted, prm.num_neighbors,
                       dnrm);
    HIPCHK(hipGetLastError());
    if (normals) {
        if (N) HIPCHK(hipMemcpyAsync(normals, dnrm, N * 12, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return ODO_OK;
    }
    // fit's exits (icp.cpp:43-52) and fitIterate's start
    std::vector<IcpState> hs(NP);
    int left = 0;
    for (size_t p = 0; p < NP; p++) {
        IcpState& s = hs[p];
        memset(&s, 0, sizeof s);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) s.R[3 * i + j] = guesses ? guesses[16 * p + 4 * i + j] : (i == j ? 1.f : 0.f);
            s.t[i] = guesses ? guesses[16 * p + 4 * i + 3] : 0.f;
        }
        s.delta = 1000.f;
        s.indist = prm.indist;
        const int nm = offs[pairs[p].t + 1] - offs[pairs[p].t], nt = offs[pairs[p].s + 1] - offs[pairs[p].s];
        s.status = nm < 5 ? ODO_ICP_NO_MODEL : nt < 5 ? ODO_ICP_SHORT_TEMPLATE : ODO_ICP_OK;
        s.done = s.status != ODO_ICP_OK || !(0 < prm.max_iterations && 1000.0 > prm.min_delta);
        left += !s.done;
    }
    IcpState* dstate = (IcpState*)(d + o_state);
    int* dleft = (int*)(d + o_left);
    float* drows = (float*)(d + o_rows);
    const GgPair* dpairs = (const GgPair*)(d + o_pairs);
    HIPCHK(hipMemcpyAsync(dstate, hs.data(), NP * sizeof(IcpState), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dleft, &left, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d + o_pairs, pairs.data(), NP * sizeof(GgPair), hipMemcpyHostToDevice, st));
    // rounds of sweep + step with nothing read back; every 8th round the
    // counter of unfinished pairs, to stop early
    for (int r = 0; r < prm.max_iterations && left > 0; r++) {
        launch_icp_sweep(st, G.dcl, dpairs, nprob, max_ns, G.cstart, G.sorted, dnrm, dstate, prm.gate, prm.indist, 0,
                         drows);
        launch_icp_step(st, G.dcl, dpairs, nprob, drows, dstate, prm.max_iterations, prm.min_delta, 0, dleft);
        if (r % 8 == 7) {
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&left, dleft, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    launch_icp_sweep(st, G.dcl, dpairs, nprob, max_ns, G.cstart, G.sorted, dnrm, dstate, prm.gate, prm.indist, 1, drows);
    launch_icp_step(st, G.dcl, dpairs, nprob, drows, dstate, prm.max_iterations, prm.min_delta, 1, dleft);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs.data(), dstate, NP * sizeof(IcpState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t p = 0; p < NP; p++) {
        const IcpState& s = hs[p];
        odo_icp_result& o = out[p];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) o.T[4 * i + j] = s.R[3 * i + j];
            o.T[4 * i + 3] = s.t[i];
        }
        o.T[12] = o.T[13] = o.T[14] = 0.f;
        o.T[15] = 1.f;
        o.residual = s.residual;
        o.delta = s.delta;
        o.iterations = s.iter;
        o.n_active = s.n_active;
        o.status = s.status;
    }
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

int odo_cloud_sor_batch(odo_ctx* c, const float* P, const int32_t* offs, int ncl, int mean_k, double stddev_mul,
                        float cell, uint8_t* keep, float* distances, odo_sor_info* info) {
    const char* who = "cloud_sor_batch";
    if (!c || ncl < 0 || !offs || (ncl && !info)) return fail(ODO_ERR_ARG, "bad cloud_sor_batch args");
    int e;
    if ((e = check_sor_params(mean_k, stddev_mul, who))) return e;
    if (!(cell >= 0) || !std::isfinite(cell)) return fail(ODO_ERR_ARG, "cloud_sor_batch: cell must be finite and >= 0");
    if (ncl == 0) return ODO_OK;
    if (ncl > 65535) return fail(ODO_ERR_CAPACITY, "cloud_sor_batch: more than 65535 clouds per call");
    if ((e = check_offs(offs, ncl, who))) return e;
    const size_t N = (size_t)offs[ncl];
    if (N && (!P || !keep)) return fail(ODO_ERR_ARG, "bad cloud_sor_batch args");
    if (N > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "cloud_sor_batch: more than 2^29 points per call");
    if (!all_finite(P, 3 * N)) return fail(ODO_ERR_ARG, "cloud_sor_batch: a coordinate is not finite");
    if ((e = sync_all(c))) return e;
    std::vector<int32_t> o(offs, offs + ncl + 1);
    Source s;
    s.host[0] = P;
    s.host_rows[0] = N;
    return run_sor(c, s, o, mean_k, stddev_mul, cell, who, keep, distances, info);
}

int odo_dense_sor(odo_ctx* c, int mean_k, double stddev_mul, odo_sor_info* info) {
    const char* who = "dense_sor";
    if (!c) return fail(ODO_ERR_ARG, "dense_sor: null ctx");
    if (c->cloud_n < 0) return fail(ODO_ERR_STATE, "dense_sor: no dense-cloud call yet");
    if (!info) return fail(ODO_ERR_ARG, "bad dense_sor args");
    int e;
    if ((e = check_sor_params(mean_k, stddev_mul, who))) return e;
    if (c->cloud_n > 65535) return fail(ODO_ERR_CAPACITY, "dense_sor: more than 65535 frames in the dense-cloud call");
    if ((e = sync_all(c))) return e;
    std::vector<int32_t> offs(1, 0);
    Source s;
    s.dev = (const float*)c->cloud_out.p;
    s.stride = (int)(sizeof(odo_cloud_point) / 4);
    for (int f = 0; f < c->cloud_n; f++) {
        if (c->cloud_np[f] > GG_MAX_POINTS) return fail(ODO_ERR_CAPACITY, "dense_sor: more than 1048576 points in a cloud");
        if ((size_t)offs.back() + (size_t)c->cloud_np[f] > (size_t)INT32_MAX / 4)
            return fail(ODO_ERR_CAPACITY, "dense_sor: more than 2^29 points per call");
        s.row0.push_back(c->cloud_off[f]);
        offs.push_back(offs.back() + c->cloud_np[f]);
    }
    return run_sor(c, s, offs, mean_k, stddev_mul, 0.f, who, nullptr, nullptr, info);
}

int odo_gicp_grid_fitness(odo_ctx* c, const float* src, const int32_t* soffs, const float* tgt, const int32_t* toffs,
                          const float* T, int nprob, float cell, double* score, float* nn_d2) {
    const char* who = "gicp_grid_fitness";
    if (!c || nprob < 0 || !soffs || !toffs || (nprob && (!T || !score)))
        return fail(ODO_ERR_ARG, "bad gicp_grid_fitness args");
    if (!(cell >= 0) || !std::isfinite(cell)) return fail(ODO_ERR_ARG, "gicp_grid_fitness: cell must be finite and >= 0");
    if (nprob == 0) return ODO_OK;
    if (nprob > 32767) return fail(ODO_ERR_CAPACITY, "gicp_grid_fitness: more than 32767 pairs per call");
    int e;
    if ((e = check_offs(soffs, nprob, who)) || (e = check_offs(toffs, nprob, who))) return e;
    const size_t S = (size_t)soffs[nprob], Tn = (size_t)toffs[nprob];
    if ((S && !src) || (Tn && !tgt)) return fail(ODO_ERR_ARG, "bad gicp_grid_fitness args");
    if (S + Tn > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "gicp_grid_fitness: more than 2^29 points per call");
    if (!all_finite(src, 3 * S) || !all_finite(tgt, 3 * Tn))
        return fail(ODO_ERR_ARG, "gicp_grid_fitness: a coordinate is not finite");
    if (!all_finite(T, 16 * (size_t)nprob)) return fail(ODO_ERR_ARG, "gicp_grid_fitness: a transform is not finite");
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
    s.host_rows[1] = Tn;
    return run_fitness(c, s, offs, pairs, T, cell, who, score, nn_d2);
}

int odo_gicp_dense_fitness(odo_ctx* c, const int32_t* pairs, int nprob, const float* T, double* score) {
    const char* who = "gicp_dense_fitness";
    if (!c) return fail(ODO_ERR_ARG, "gicp_dense_fitness: null ctx");
    if (c->cloud_n < 0) return fail(ODO_ERR_STATE, "gicp_dense_fitness: no dense-cloud call yet");
    if (nprob < 0 || (nprob && (!pairs || !T || !score))) return fail(ODO_ERR_ARG, "bad gicp_dense_fitness args");
    for (int k = 0; k < 2 * nprob; k++)
        if (pairs[k] < 0 || pairs[k] >= c->cloud_n)
            return fail(ODO_ERR_ARG, "gicp_dense_fitness: frame outside the last dense-cloud call");
    if (nprob && !all_finite(T, 16 * (size_t)nprob))
        return fail(ODO_ERR_ARG, "gicp_dense_fitness: a transform is not finite");
    if (nprob == 0) return ODO_OK;
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "gicp_dense_fitness: more than 65535 pairs per call");
    if (c->cloud_n > 65535)
        return fail(ODO_ERR_CAPACITY, "gicp_dense_fitness: more than 65535 frames in the dense-cloud call");
    int e;
    if ((e = sync_all(c))) return e;
    // the distinct frames, in the order they are named: one grid each
    std::vector<int> cloud_of((size_t)c->cloud_n, -1);
    std::vector<int32_t> offs(1, 0);
    std::vector<GgPair> pr((size_t)nprob);
    Source s;
    s.dev = (const float*)c->cloud_out.p;
    s.stride = (int)(sizeof(odo_cloud_point) / 4);
    for (int k = 0; k < 2 * nprob; k++) {
        const int f = pairs[k];
        if (cloud_of[f] < 0) {
            if (c->cloud_np[f] > GG_MAX_POINTS)
                return fail(ODO_ERR_CAPACITY, "gicp_dense_fitness: more than 1048576 points in a cloud");
            if ((size_t)offs.back() + (size_t)c->cloud_np[f] > (size_t)INT32_MAX / 4)
                return fail(ODO_ERR_CAPACITY, "gicp_dense_fitness: more than 2^29 points per call");
            cloud_of[f] = (int)offs.size() - 1;
            s.row0.push_back(c->cloud_off[f]);
            offs.push_back(offs.back() + c->cloud_np[f]);
        }
        (k & 1 ? pr[k / 2].t : pr[k / 2].s) = cloud_of[f];
    }
    return run_fitness(c, s, offs, pr, T, 0.f, who, score, nullptr);
}

void odo_default_icp_params(odo_icp_params* p) {
    if (!p) return;
    p->num_neighbors = 10;  // icpPointToPlane.h
    p->max_iterations = 200;  // icp.cpp:7-8
    p->gate = ODO_ICP_GATE_AS_WRITTEN;
    p->pad = 0;
    p->min_delta = 1e-4;
    p->indist = -1;  // icp.h: fit's default
}

int odo_icp_normals(odo_ctx* c, const float* P, const int32_t* offs, int ncl, int num_neighbors, float cell,
                    float* normals) {
    const char* who = "icp_normals";
    if (!c || ncl < 0 || !offs) return fail(ODO_ERR_ARG, "bad icp_normals args");
    if (num_neighbors < 3) return fail(ODO_ERR_ARG, "icp_normals: num_neighbors < 3");
    if (!(cell >= 0) || !std::isfinite(cell)) return fail(ODO_ERR_ARG, "icp_normals: cell must be finite and >= 0");
    if (num_neighbors > odo::ICP_MAX_K) return fail(ODO_ERR_CAPACITY, "icp_normals: num_neighbors above 32");
    if (ncl == 0) return ODO_OK;
    if (ncl > 65535) return fail(ODO_ERR_CAPACITY, "icp_normals: more than 65535 clouds per call");
    int e;
    if ((e = check_offs(offs, ncl, who))) return e;
    const size_t N = (size_t)offs[ncl];
    if (N == 0) return ODO_OK;
    if (!P || !normals) return fail(ODO_ERR_ARG, "bad icp_normals args");
    if (N > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "icp_normals: more than 2^29 points per call");
    if (!all_finite(P, 3 * N)) return fail(ODO_ERR_ARG, "icp_normals: a coordinate is not finite");
    if ((e = sync_all(c))) return e;
    std::vector<int32_t> o(offs, offs + ncl + 1);
    std::vector<GgPair> none;
    Source s;
    s.host[0] = P;
    s.host_rows[0] = N;
    odo_icp_params prm;
    odo_default_icp_params(&prm);
    prm.num_neighbors = num_neighbors;
    return run_icp(c, s, o, none, nullptr, prm, cell, who, nullptr, normals);
}

int odo_icp_plane_batch(odo_ctx* c, const float* tmpl, const int32_t* toffs, const float* model, const int32_t* moffs,
                        const float* guesses, int nprob, const odo_icp_params* params, float cell,
                        odo_icp_result* out) {
    const char* who = "icp_plane_batch";
    if (!c || nprob < 0 || !toffs || !moffs || (nprob && !out)) return fail(ODO_ERR_ARG, "bad icp_plane_batch args");
    int e;
    if ((e = check_icp_plane_params(params, guesses, nprob, who))) return e;
    if (!(cell >= 0) || !std::isfinite(cell)) return fail(ODO_ERR_ARG, "icp_plane_batch: cell must be finite and >= 0");
    if (nprob == 0) return ODO_OK;
    if (nprob > 32767) return fail(ODO_ERR_CAPACITY, "icp_plane_batch: more than 32767 pairs per call");
    if ((e = check_offs(toffs, nprob, who)) || (e = check_offs(moffs, nprob, who))) return e;
    const size_t S = (size_t)toffs[nprob], T = (size_t)moffs[nprob];
    if ((S && !tmpl) || (T && !model)) return fail(ODO_ERR_ARG, "bad icp_plane_batch args");
    if (S + T > (size_t)INT32_MAX / 4) return fail(ODO_ERR_CAPACITY, "icp_plane_batch: more than 2^29 points per call");
    if (!all_finite(tmpl, 3 * S) || !all_finite(model, 3 * T))
        return fail(ODO_ERR_ARG, "icp_plane_batch: a coordinate is not finite");
    if ((e = sync_all(c))) return e;
    // clouds: the templates, then the models
    std::vector<int32_t> offs(2 * (size_t)nprob + 1);
    std::vector<GgPair> pairs((size_t)nprob);
    for (int p = 0; p <= nprob; p++) offs[p] = toffs[p];
    for (int p = 1; p <= nprob; p++) offs[(size_t)nprob + p] = (int32_t)(S + (size_t)moffs[p]);
    for (int p = 0; p < nprob; p++) pairs[p] = GgPair{p, nprob + p, 0};
    Source s;
    s.host[0] = tmpl;
    s.host_rows[0] = S;
    s.host[1] = model;
    s.host_rows[1] = T;
    return run_icp(c, s, offs, pairs, guesses, *params, cell, who, out, nullptr);
}

int odo_icp_plane_dense(odo_ctx* c, const int32_t* pairs, int nprob, const float* guesses,
                        const odo_icp_params* params, odo_icp_result* out) {
    const char* who = "icp_plane_dense";
    if (!c) return fail(ODO_ERR_ARG, "icp_plane_dense: null ctx");
    if (c->cloud_n < 0) return fail(ODO_ERR_STATE, "icp_plane_dense: no dense-cloud call yet");
    if (nprob < 0 || (nprob && (!pairs || !out))) return fail(ODO_ERR_ARG, "bad icp_plane_dense args");
    int e;
    if ((e = check_icp_plane_params(params, guesses, nprob, who))) return e;
    for (int k = 0; k < 2 * nprob; k++)
        if (pairs[k] < 0 || pairs[k] >= c->cloud_n)
            return fail(ODO_ERR_ARG, "icp_plane_dense: frame outside the last dense-cloud call");
    if (nprob == 0) return ODO_OK;
    if (nprob > 65535) return fail(ODO_ERR_CAPACITY, "icp_plane_dense: more than 65535 pairs per call");
    if (c->cloud_n > 65535) return fail(ODO_ERR_CAPACITY, "icp_plane_dense: more than 65535 frames in the dense-cloud call");
    if ((e = sync_all(c))) return e;
    // the distinct frames, in the order they are named: one grid each, normals
    // for those named as a model
    std::vector<int> cloud_of((size_t)c->cloud_n, -1);
    std::vector<int32_t> offs(1, 0);
    std::vector<GgPair> pr((size_t)nprob);
    Source s;
    s.dev = (const float*)c->cloud_out.p;
    s.stride = (int)(sizeof(odo_cloud_point) / 4);
    for (int k = 0; k < 2 * nprob; k++) {
        const int f = pairs[k];
        if (cloud_of[f] < 0) {
            if (c->cloud_np[f] > GG_MAX_POINTS)
                return fail(ODO_ERR_CAPACITY, "icp_plane_dense: more than 1048576 points in a cloud");
            if ((size_t)offs.back() + (size_t)c->cloud_np[f] > (size_t)INT32_MAX / 4)
                return fail(ODO_ERR_CAPACITY, "icp_plane_dense: more than 2^29 points per call");
            cloud_of[f] = (int)offs.size() - 1;
            s.row0.push_back(c->cloud_off[f]);
            offs.push_back(offs.back() + c->cloud_np[f]);
        }
        (k & 1 ? pr[k / 2].t : pr[k / 2].s) = cloud_of[f];
    }
    return run_icp(c, s, offs, pr, guesses, *params, 0.f, who, out, nullptr);
}

}  // extern "C"
