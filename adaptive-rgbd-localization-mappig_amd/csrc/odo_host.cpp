// The parts of the C-ABI that need no device: the glibc rand() restatement,
// the hypotheses fold, pose chaining, the TUM trajectory writer and the
// re-scoring of a Fuse record.
#include "odo_ctx.h"

static_assert(sizeof(odo_fuse_kf) == 80 && sizeof(odo_fuse_cand) == 40, "odo_fuse_* layout");

extern "C" {

// matcher.cpp:256-291 over the record's gated keypoints (k_fuse_search's
// window and gate, the same float operations in the same order)
int odo_fuse_best(const odo_fuse_cand* rec, const float* kun, const float* ur, const uint8_t* desc, int n, float th,
                  const uint8_t new_desc[32], int32_t* best_idx, int32_t* best_dist) {
    if (!rec || !new_desc || !best_idx || !best_dist || n < 0 || (n && (!kun || !ur || !desc)))
        return fail(ODO_ERR_ARG, "bad fuse_best args");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ODO_ERR_ARG, "fuse_best: th must be finite and >= 0");
    int bi = -1, bd = INT32_MAX;
    auto visit = [&](int j) {
        int d = 0;
        for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(new_desc[k] ^ desc[32 * (size_t)j + k]));
        if (d < bd) {
            bd = d;
            bi = j;
        }
    };
    if (rec->n_cand > ODO_FUSE_CANDS) {
        const float u = rec->u, v = rec->v, r = rec->ur;
        for (int j = 0; j < n; j++) {
            const float dx = kun[2 * j] - u, dy = kun[2 * j + 1] - v;
            if (!(fabsf(dx) < th && fabsf(dy) < th)) continue;
            const float ex = u - kun[2 * j], ey = v - kun[2 * j + 1];
            float e2 = ex * ex + ey * ey, lim = 5.99f;
            if (ur[j] >= 0.0f) {
                const float er = r - ur[j];
                e2 = e2 + er * er;
                lim = 7.8f;
            }
            if (e2 > lim) continue;
            visit(j);
        }
    } else {
        for (int k = 0; k < rec->n_cand; k++) {
            if (rec->cand[k] >= n) return fail(ODO_ERR_ARG, "fuse_best: a candidate outside the keyframe");
            visit(rec->cand[k]);
        }
    }
    *best_idx = bi;
    *best_dist = bd;
    return ODO_OK;
}

void odo_rng_seed(odo_rng* r, uint32_t seed) {
    // glibc __srandom_r (TYPE_3): Schrage LCG fill, fptr=3, rptr=0, 310 discards
    if (seed == 0) seed = 1;
    r->state[0] = (int32_t)seed;
    int32_t word = (int32_t)seed;
    for (int i = 1; i < 31; ++i) {
        long hi = word / 127773, lo = word % 127773;
        long w2 = 16807 * lo - 2836 * hi;
        if (w2 < 0) w2 += 2147483647;
        word = (int32_t)w2;
        r->state[i] = word;
    }
    r->fpos = 3;
    r->rpos = 0;
    for (int k = 0; k < 310; k++) odo_rng_next(r);
}

int32_t odo_rng_next(odo_rng* r) {
    uint32_t val = (uint32_t)r->state[r->fpos] + (uint32_t)r->state[r->rpos];
    r->state[r->fpos] = (int32_t)val;
    int32_t out = (int32_t)(val >> 1);
    if (++r->fpos >= 31) {
        r->fpos = 0;
        ++r->rpos;
    } else if (++r->rpos >= 31) r->rpos = 0;
    return out;
}

int odo_ransac_fold(const odo_hyp_summary* all, int H, int n_good, const odo_ransac_params* p,
                    odo_ransac_fold_result* r) {
    if (!p || !r || H < 0 || (H && !all)) return fail(ODO_ERR_ARG, "bad fold args");
    // ransac.cpp:201-249: hypothesis j is the j-th visited iteration; n += 10
    // skips do not consume samples, so the fold walks the summaries in order
    *r = odo_ransac_fold_result{-1, 0, 0, 0, 1e6f, n_good, {0, 0}};
    if (n_good < p->min_inlier_th || n_good < p->sample_size) return ODO_OK;
    const unsigned minInl = (unsigned)p->min_inlier_th;
    int n = 0, best = 0;
    float rmse = 1e6f;
    for (int pos = 0; pos < H && n < p->iterations; pos++) {
        const unsigned rc = (unsigned)all[pos].cnt;
        const double re = all[pos].err;
        r->visited++;
        bool brk = false;
        if (rc > 0) {
            r->valid++;
            if (re <= (double)rmse && rc >= (unsigned)best && rc >= minInl) {
                rmse = (float)re;
                best = (int)rc;
                r->best_h = pos;
                if (rc > n_good * 0.5) n += 10;
                if (rc > n_good * 0.75) n += 10;
                if (rc > n_good * 0.8) brk = true;
            }
        }
        n++;
        if (brk) break;
    }
    r->rmse = rmse;
    r->n_inliers = best;
    return ODO_OK;
}

int odo_chain_poses(const odo_pair_result* res, int n, const float Tcw_prev[16], float* out) {
    if (!res || n < 0 || !out) return fail(ODO_ERR_ARG, "bad chain args");
    double T[16];
    for (int k = 0; k < 16; k++) T[k] = Tcw_prev ? (double)Tcw_prev[k] : (k % 5 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < n; i++) {
        if (!(i == 0 && res[i].n_matches == 0)) {
            double R[16], M[16];
            for (int k = 0; k < 16; k++) R[k] = (double)res[i].Tcw[k];
            for (int r = 0; r < 4; r++)
                for (int c2 = 0; c2 < 4; c2++)
                    M[4 * r + c2] = ((R[4 * r] * T[c2] + R[4 * r + 1] * T[4 + c2]) + R[4 * r + 2] * T[8 + c2]) +
                                    R[4 * r + 3] * T[12 + c2];
            memcpy(T, M, sizeof(T));
        }
        for (int k = 0; k < 16; k++) out[16 * i + k] = (float)T[k];
    }
    return ODO_OK;
}

// Eigen::Quaterniond(Matrix3d) (quaternionbase_assign_impl), host restatement
static void quat_from_rot(const double m[3][3], double q[4] /* x y z w */) {
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
}

int odo_write_tum_trajectory(const char* path, const double* ts, const float* Tcw, int n, int append) {
    if (!path || n < 0 || (n && (!ts || !Tcw))) return fail(ODO_ERR_ARG, "bad trajectory args");
    FILE* f = fopen(path, append ? "a" : "w");
    if (!f) return fail(ODO_ERR_ARG, std::string("cannot open ") + path);
    for (int i = 0; i < n; i++) {
        const float* T = Tcw + 16 * i;
        // Rwc = Rcw^T; twc = -Rwc * tcw (cv::Mat float, double accumulation)
        float Rwc[3][3];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) Rwc[r][c2] = T[4 * c2 + r];
        float twc[3];
        for (int r = 0; r < 3; r++)
            twc[r] = (float)(((double)-Rwc[r][0] * T[3] + (double)-Rwc[r][1] * T[7]) + (double)-Rwc[r][2] * T[11]);
        double m[3][3], q[4];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) m[r][c2] = (double)Rwc[r][c2];
        quat_from_rot(m, q);
        fprintf(f, "%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", ts[i], twc[0], twc[1], twc[2], (float)q[0],
                (float)q[1], (float)q[2], (float)q[3]);
    }
    fclose(f);
    return ODO_OK;
}

}  // extern "C"
