// Dense clouds (include/odo.h): Frame::CreateCloud, VoxelGridFilterCloud and
// the map transform for the frames of a batch (k_cloud.hip). The launch chain
// has one host round trip in it: the infos come back once the voxels are
// counted, the output block is sized from them, and the points follow.
#include "odo_ctx.h"

static_assert(sizeof(odo_cloud_point) == 16 && sizeof(odo_cloud_info) == 60, "odo_cloud_* layout");

namespace odo {

static int check_args(odo_ctx* c, const void* a, const void* b, int n, float leaf, const float* Twc, odo_cloud_info* info) {
    if (!c || !a || !b || !info || n <= 0 || n > c->maxb) return fail(ODO_ERR_ARG, "bad dense_clouds args");
    if (!(leaf >= 0.0f) || !std::isfinite(leaf)) return fail(ODO_ERR_ARG, "dense_clouds: leaf must be finite and >= 0");
    if (Twc)
        for (int k = 0; k < 16 * n; k++)
            if (!std::isfinite(Twc[k])) return fail(ODO_ERR_ARG, "dense_clouds: Twc must be finite");
    return ODO_OK;
}

// the context is idle (sync_all) and the frames are in HBM, or queued on the stream
static int run_clouds(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n, float leaf, const float* Twc,
                      odo_cloud_info* info) {
    hipStream_t st = c->stream;
    const size_t N = (size_t)n, P = (size_t)c->W * c->H;
    const int nch = (int)((P + CLOUD_CHUNK - 1) / CLOUD_CHUNK);
    c->cloud_n = -1;  // until this call has its points
    Pack pk;
    const size_t o_twc = pk.add(N * 64), o_info = pk.add(N * sizeof(odo_cloud_info));
    const size_t host_bytes = pk.off;
    const size_t o_fr = pk.add(N * sizeof(CloudFrame)), o_co = pk.add(N * nch * 4), o_ho = pk.add(N * nch * 4),
                 o_hist = pk.add(N * nch * 256 * 4);
    size_t o_key[2], o_idx[2];
    for (int k = 0; k < 2; k++) {
        o_key[k] = pk.add(N * P * 4);
        o_idx[k] = pk.add(N * P * 4);
    }
    int e;
    if ((e = c->cloud_dev.reserve(pk.off, 0, "dense_clouds"))) return e;
    if ((e = stage_reserve(c, host_bytes))) return e;
    uint8_t *h = c->stage.p, *d = c->cloud_dev.p;
    if (Twc) {
        memcpy(h + o_twc, Twc, N * 64);
        HIPCHK(hipMemcpyAsync(d + o_twc, h + o_twc, N * 64, hipMemcpyHostToDevice, st));
    }
    CloudArgs a{};
    a.n = n;
    a.W = c->W;
    a.H = c->H;
    a.nch = nch;
    a.cal = c->cal;
    a.leaf = leaf;
    a.bgr = d_bgr;
    a.depth = d_depth;
    a.Twc = Twc ? (const float*)(d + o_twc) : nullptr;
    a.fr = (CloudFrame*)(d + o_fr);
    a.info = (odo_cloud_info*)(d + o_info);
    a.chunk_off = (int32_t*)(d + o_co);
    a.head_off = (int32_t*)(d + o_ho);
    a.hist = (int32_t*)(d + o_hist);
    for (int k = 0; k < 2; k++) {
        a.key[k] = (uint32_t*)(d + o_key[k]);
        a.idx[k] = (uint32_t*)(d + o_idx[k]);
    }
    launch_cloud_voxels(st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h + o_info, d + o_info, N * sizeof(odo_cloud_info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const odo_cloud_info* I = (const odo_cloud_info*)(h + o_info);
    std::vector<int32_t> off(N + 1, 0), np(N, 0);
    int max_points = 0;
    for (int f = 0; f < n; f++) {
        np[f] = I[f].n_points;
        off[(size_t)f + 1] = off[f] + np[f];  // at most max_batch * W * H
        max_points = std::max(max_points, np[f]);
    }
    // the points, then their counts
    const size_t total = (size_t)off[N];
    Pack po;
    po.add(total * sizeof(odo_cloud_point));
    const size_t cnt_at = po.off;
    // never empty: a call without a point still hands out a device address
    if ((e = c->cloud_out.reserve(std::max(cnt_at + total * 4, (size_t)256), 0, "dense_clouds"))) return e;
    a.out = (odo_cloud_point*)c->cloud_out.p;
    a.counts = (int32_t*)(c->cloud_out.p + cnt_at);
    launch_cloud_points(st, a, max_points);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    memcpy(info, I, N * sizeof(odo_cloud_info));
    c->cloud_off.swap(off);
    c->cloud_np.swap(np);
    c->cloud_counts_at = cnt_at;
    c->cloud_n = n;
    return ODO_OK;
}

static int cloud_at(odo_ctx* c, int i, const char* who) {
    if (!c) return fail(ODO_ERR_ARG, std::string(who) + ": null ctx");
    if (c->cloud_n < 0) return fail(ODO_ERR_STATE, std::string(who) + ": no dense-cloud call yet");
    if (i < 0 || i >= c->cloud_n) return fail(ODO_ERR_ARG, std::string(who) + ": frame outside the last dense-cloud call");
    return ODO_OK;
}

}  // namespace odo

extern "C" {

int odo_dense_clouds(odo_ctx* c, const uint8_t* d_bgr, const uint16_t* d_depth, int n, float leaf, const float* Twc,
                     odo_cloud_info* info) {
    int e;
    if ((e = check_args(c, d_bgr, d_depth, n, leaf, Twc, info))) return e;
    if ((e = sync_all(c))) return e;
    return run_clouds(c, d_bgr, d_depth, n, leaf, Twc, info);
}

int odo_dense_clouds_host(odo_ctx* c, const uint8_t* bgr, const uint16_t* depth, int n, float leaf, const float* Twc,
                          odo_cloud_info* info) {
    int e;
    if ((e = check_args(c, bgr, depth, n, leaf, Twc, info))) return e;
    if ((e = sync_all(c))) return e;
    // every stream is idle, so neither input staging buffer is in use; the call
    // below ends with the stream synchronised, so it is free again afterwards
    const size_t px = (size_t)n * c->W * c->H;
    HIPCHK(hipMemcpyAsync(c->bgr_in[0], bgr, px * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->depth_in[0], depth, px * 2, hipMemcpyHostToDevice, c->stream));
    return run_clouds(c, c->bgr_in[0], c->depth_in[0], n, leaf, Twc, info);
}

int odo_get_dense_cloud(odo_ctx* c, int i, odo_cloud_point* pts, int32_t* counts, int cap, int* n) {
    int e;
    if ((e = cloud_at(c, i, "get_dense_cloud"))) return e;
    if (!n || cap < 0 || (cap > 0 && !pts)) return fail(ODO_ERR_ARG, "bad get_dense_cloud args");
    if ((e = sync_all(c))) return e;
    const int np = c->cloud_np[i], m = std::min(np, cap);
    const size_t o = (size_t)c->cloud_off[i];
    if (m > 0) {
        HIPCHK(hipMemcpy(pts, (const odo_cloud_point*)c->cloud_out.p + o, (size_t)m * sizeof(odo_cloud_point),
                         hipMemcpyDeviceToHost));
        if (counts)
            HIPCHK(hipMemcpy(counts, (const int32_t*)(c->cloud_out.p + c->cloud_counts_at) + o, (size_t)m * 4,
                             hipMemcpyDeviceToHost));
    }
    *n = np;
    if (np > cap) return fail(ODO_ERR_CAPACITY, "get_dense_cloud: the cloud has more points than cap");
    return ODO_OK;
}

int odo_dense_cloud_device(odo_ctx* c, int i, const odo_cloud_point** d_pts, const int32_t** d_counts, int* n) {
    int e;
    if ((e = cloud_at(c, i, "dense_cloud_device"))) return e;
    if (!d_pts || !n) return fail(ODO_ERR_ARG, "bad dense_cloud_device args");
    const size_t o = (size_t)c->cloud_off[i];
    *d_pts = (const odo_cloud_point*)c->cloud_out.p + o;
    if (d_counts) *d_counts = (const int32_t*)(c->cloud_out.p + c->cloud_counts_at) + o;
    *n = c->cloud_np[i];
    return ODO_OK;
}

}  // extern "C"
