// The context behind the C-ABI (include/odo.h) and what its host translation
// units share: odo_capi.cpp (lifetime, setters, getters), odo_geometry.cpp
// (host tables), odo_batch.cpp (the pipelined path), odo_stages.cpp (the
// synchronous per-stage entry points), odo_cloud.cpp (dense clouds),
// odo_hyps.cpp (single-pair RANSAC) and odo_host.cpp (no device). Host only:
// no kernel file includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/odo.h"
#include "odo_device.h"
#include "odo_internal.h"

namespace odo {

// odo_last_error()'s message of the calling thread (defined in odo_capi.cpp)
extern thread_local std::string g_err;
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail(ODO_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Device scratch of the per-stage entry points (odo_extract ... odo_kabsch):
// owned by a context, bump-allocated per call, grown on demand and never freed
// per call. A call that outgrows the block takes an extra block; the next call
// replaces the blocks by one of their total size. Every allocation is checked
// (a failed one sets `failed`, which the entry point turns into
// ODO_ERR_DEVICE). begin() may hipFree the blocks: its callers first make sure
// that no kernel of an earlier call still uses them (the per-stage entry
// points are synchronous; hypotheses mode, whose _dev / _finish calls queue
// kernels asynchronously, synchronises its stream before begin()).
struct DevArena {
    std::vector<std::pair<uint8_t*, size_t>> blocks;
    size_t used = 0;
    bool failed = false;
    ~DevArena() { release(); }
    void release() {
        for (auto& b : blocks) (void)hipFree(b.first);
        blocks.clear();
        used = 0;
    }
    void begin() {
        failed = false;
        if (blocks.size() > 1) {
            size_t tot = 0;
            for (auto& b : blocks) tot += b.second;
            release();
            grow(tot);
        }
        used = 0;
    }
    bool grow(size_t bytes) {
        uint8_t* p = nullptr;
        if (hipMalloc((void**)&p, bytes) != hipSuccess) {
            failed = true;
            return false;
        }
        blocks.push_back({p, bytes});
        used = 0;
        return true;
    }
    void* take(size_t bytes) {
        bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
        if (blocks.empty() || used + bytes > blocks.back().second)
            if (!grow(std::max(bytes, blocks.empty() ? (size_t)16 << 20 : blocks.back().second))) return nullptr;
        void* r = blocks.back().first + used;
        used += bytes;
        return r;
    }
};

// Frame sets in flight (4): batch k extracts into set k%NSETS while the pair and
// PnP stages of batches k-1 and k-2 still read theirs, so the extraction
// stream never waits on the PnP latency of the batch just before it.
// measured: 4 sets 60.1k vs 3 sets 57.7k frames/s (256-frame batches).
// The extraction of batch b waits for the PnP of batch b - PYR_WAIT, so the
// pyramid does not share the CUs with a PnP / RANSAC evaluation still running
// from an earlier batch (measured: 3, 1.921-1.938 vs 1.933-1.989 ms per step,
// hard workload unchanged, profiles/r05_q).
constexpr int NSETS = 4, PYR_WAIT = 3;
// The next batch's roll reads this set's last frame on its pair stream, before
// its PnP: the batch that reuses this set waits for that PnP through PYR_WAIT,
// which therefore has to be at least 1. And batch b - PYR_WAIT must not share
// batch b's frame set: its PnP-done event is re-recorded by batch
// b - PYR_WAIT + NSETS.
static_assert(PYR_WAIT >= 1 && PYR_WAIT < NSETS, "PYR_WAIT must lie in [1, NSETS - 1]");
// The context's events only order its streams against each other (and tell
// the host that inputs were consumed): none needs the system-scope cache
// writeback + invalidate a default event record performs, which on this part
// also disturbs every kernel then running (round 5: ~10 records per batch;
// DESIGN §4 Pipelining)
constexpr unsigned SYNC_EVENT_FLAGS = hipEventDisableTiming | hipEventDisableSystemFence;
// output rows per resize workgroup
constexpr int RZ_RB = 16;

// Owner of hipMalloc'ed buffers whose pointers live in a context: alloc()
// records the slot it fills, release() frees every buffer and nulls the slots
// (so a partly built set is freed exactly, and a buffer cannot be forgotten).
struct DevPool {
    std::vector<void**> slots;
    ~DevPool() { release(); }
    template <typename T>
    int alloc(T** p, size_t count) {
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)p, count * sizeof(T));
        if (e != hipSuccess) return fail(ODO_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
        slots.push_back((void**)p);
        return ODO_OK;
    }
    void release() {
        for (void** s : slots) {
            (void)hipFree(*s);
            *s = nullptr;
        }
        slots.clear();
    }
};

// A grow-only block, device (hipMalloc) or page-locked (hipHostMalloc): one
// allocation that reserve() replaces by a larger one when a call needs more
// and that lives until release() or its owner's end. When it grows its
// contents are lost. The capacity policy is the caller's: reserve() allocates
// max(bytes, floor). A failed allocation leaves the block empty and HIP's last
// error cleared, so that no later call reports it.
template <bool PINNED>
struct GrowBlock {
    uint8_t* p = nullptr;
    size_t cap = 0;
    GrowBlock() = default;
    GrowBlock(const GrowBlock&) = delete;
    GrowBlock& operator=(const GrowBlock&) = delete;
    ~GrowBlock() { release(); }
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    int reserve(size_t bytes, size_t floor, const char* who) {
        if (bytes <= cap) return ODO_OK;
        release();
        const size_t want = std::max(bytes, floor);
        if ((PINNED ? hipHostMalloc((void**)&p, want, hipHostMallocDefault) : hipMalloc((void**)&p, want)) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(ODO_ERR_DEVICE, std::string(who) + (PINNED ? ": hipHostMalloc failed" : ": hipMalloc failed"));
        }
        cap = want;
        return ODO_OK;
    }
};
using DevBlock = GrowBlock<false>;
using PinnedBlock = GrowBlock<true>;

struct HypSession;  // hypotheses-mode RANSAC state (odo_hyps.cpp)
void free_hyp_session(HypSession* h);

}  // namespace odo

// The opaque handle of include/odo.h (a global name; its members' types are odo's)
using namespace odo;
struct odo_ctx {
    odo_config cfg{};
    HypSession* hs = nullptr;
    DevPool pool;  // the buffers that live as long as the context
    // every event of the context, destroyed with it
    std::vector<hipEvent_t> events;
    hipError_t make_event(hipEvent_t* e, unsigned flags) {
        const hipError_t r = hipEventCreateWithFlags(e, flags);
        if (r == hipSuccess) events.push_back(*e);
        return r;
    }
    int device = 0;
    hipStream_t stream = nullptr;   // extraction
    // pair stages of even / odd batches (kNN-2 at the head of the pair stream
    // instead of on the extraction stream: 88.2k vs 86.5k frames/s)
    hipStream_t pstream = nullptr, pstream2 = nullptr;
    std::vector<hipStream_t> owned;  // streams created (the rest alias them)
    hipEvent_t ev_latch = nullptr;   // after the last queued k_latch
    bool latch_rec = false;
    // ev_geo[set] follows the set's geometry kernel when it ran on the batch's
    // pair stream (geo_rec; the next batch's roll reads the last frame's
    // kun / xyz / uR)
    hipEvent_t ev_geo[NSETS] = {};
    bool geo_rec[NSETS] = {};
    uint64_t batch_counter = 0;  // batch b uses frame set b % NSETS and pair stream b % 2
    int W = 0, H = 0, maxb = 0, slots = 0, nlevels = 0;
    std::vector<LevelDesc> lv_h;
    std::vector<CellDesc> cells_h;
    std::vector<int> rx_off, ry_off, rz_rows;
    // k_pyramid (gray + levels, and the blurred levels) where its host checks
    // pass (pyramid_fusable, pyramid_blur_fusable) and odo_kernel_forms.pyramid
    // asks for it: ODO_PYRAMID_FORM_AUTO takes it for batches of at least
    // PYR_FUSED_MIN_FRAMES frames (a workgroup per frame: a small batch would
    // leave most CUs idle, one frame takes 0.45 vs 0.28 ms)
    int pform = ODO_PYRAMID_FORM_AUTO;
    bool pyr_fusable = false, blur_fusable = false;
    LevelDesc* lv = nullptr;
    CellDesc* cells = nullptr;
    ResizeX* rx = nullptr;
    ResizeY* ry = nullptr;
    std::vector<ResizeY> ry_h;  // host copy (k_pyramid's split plan)
    int ncells = 0, cell_cap = 0, kp_cap = 0, okp_stride = 0, node_cap = 0, match_cap = 0, mask_words = 0;
    int max_blur_tiles = 0;
    int fast_roi = 0;  // largest FAST cell ROI side
    std::vector<FastSeg> fsegs_h;  // k_fast_seg's segments (cell-row runs)
    FastSeg* fsegs = nullptr;
    FastLds fs_lds{};
    size_t pyr_size = 0, keys_per_frame = 0;
    FrameCalib cal{};
    RansacCfg rcfg{};
    // frame buffers ([NSETS][slots])
    uint8_t *pyr = nullptr, *blur = nullptr;
    uint32_t* cand = nullptr;
    int* cand_cnt = nullptr;
    uint32_t* keys = nullptr;
    int32_t* knode = nullptr;
    uint32_t* okp = nullptr;
    int* ocnt = nullptr;
    orb_kp* kps = nullptr;
    uint8_t* desc = nullptr;
    float *kun = nullptr, *xyz = nullptr, *ur = nullptr;
    int* nkp = nullptr;
    // staging for host inputs: two device buffers of max_batch frames each,
    // filled on the copy stream (odo_track_batch_host) while the extraction
    // stream reads the other one
    uint8_t* bgr_in[2] = {};
    uint16_t* depth_in[2] = {};
    hipStream_t cstream = nullptr;                      // H2D copies of host inputs
    hipEvent_t ev_in_copied[2] = {}, ev_in_free[2] = {};
    bool in_used[2] = {};
    // the last odo_track_batch_host_sparse_depth batch's depth reads (extraction
    // stream): the caller's depth buffer is in use until this event
    hipEvent_t ev_depth_done = nullptr;
    bool depth_busy = false;
    // page-locked staging of the per-stage (synchronous) entry points: their
    // inputs are packed here and uploaded with one DMA, their outputs come
    // back here with async copies into pinned memory and one sync
    PinnedBlock stage;
    // hypotheses mode (odo_ransac_hyps*): device scratch kept across sessions
    // (grow-only: a session per pair used to hipMalloc / hipFree its own,
    // 0.5 ms of the 1.2 ms per pair of round 4) and the session's packed
    // inputs in page-locked memory (one DMA), reused once hyp_up has passed
    DevArena hyp_arena;
    PinnedBlock hyp_stage;
    hipEvent_t hyp_up = nullptr;
    bool hyp_up_rec = false;
    int in_next = 0;
    // pair buffers ([maxb])
    int2 *knn_idx[NSETS] = {}, *knn_dist[NSETS] = {};  // per frame set
    // per frame set: the query frames' VO-landmark bits and kNN-2 query lists
    uint32_t* lm_bits[NSETS] = {};
    int32_t* qlist[NSETS] = {};
    int* qcnt[NSETS] = {};
    int lm_words = 0;
    int knn_split = 2;  // kNN-2 train splits per query block (ODO_KNN_SPLIT): more waves for short query lists
    // kNN-2 form (odo_kernel_forms.knn): true exact sign-vector products on the
    // matrix cores with FP4 (e2m1 +-1) operands (k_knn2_f4, the default), false
    // the VALU xor/popcount kernel k_knn2
    bool knn_mx = true;
    int last_knn_set = -1, last_knn_n = 0;  // the most recent batch's kNN-2 launch (odo_knn_replay_time)
    uint64_t* sort_scratch = nullptr;
    double* latch = nullptr;
    void* rscr[NSETS] = {};  // RANSAC scratch per frame set
    // per frame set: the pair stages of batch k write set k%NSETS while the
    // PnP launches of batches k-1, k-2 may still read their own sets
    struct PairBufs {
        odo_dmatch* matches = nullptr;
        int *n_matches = nullptr, *n_good = nullptr, *pair_valid = nullptr;
        void* good = nullptr;  // SortEl
        int32_t* f2_src = nullptr;
        uint32_t* best_mask = nullptr;
        odo_pair_result* res = nullptr;
        float* T12 = nullptr;
        void* edges = nullptr;
        uint8_t* pnp_mask = nullptr;
    } pb[NSETS];
    // Odometry::Compute back-end of the batched path (odo_set_odometry);
    // view_mode: the mode the last tracked batch ran in (-1: none / extraction only)
    int odo_mode = ODO_ODOMETRY_ADAPTIVE_RBA, view_mode = -1;
    odo_ricp_params ricp{};
    // ADAPTIVE_RICP scratch (allocated by the first switch to the mode, all or
    // nothing: rb[0].pool holds buffers exactly when it exists): one
    // copy per pair stream, batch b uses copy b & 1 on pair stream b & 1. The
    // batches of one stream run in order, so a copy is never shared by two
    // batches in flight and needs no event; odo_get_ricp reads view_rb, the
    // last batch's copy, after a full sync.
    struct RicpBufs {
        float *src = nullptr, *tgt = nullptr, *outp = nullptr, *guess = nullptr, *gT = nullptr;
        double *Cs = nullptr, *Ct = nullptr, *Mah = nullptr;
        int *is = nullptr, *it = nullptr, *offs = nullptr, *branch = nullptr, *gio = nullptr;
        odo_ricp_result* rec = nullptr;
        DevPool pool;
    } rb[2];
    int view_rb = 0;
    // Batched TrackLocalMap scratch (odo_track_local_map), allocated by its
    // first call: the per-frame arrays for max_batch frames, the per-landmark
    // ones for lm_cap landmarks (regrown when a call brings more). lm_n: the
    // landmarks of the last call while its batch is still the one in view
    // (-1: odo_get_local_map has nothing to read)
    struct LmBufs {
        uint8_t* up = nullptr;  // the packed upload: poses, priors, landmarks
        uint32_t* seen = nullptr;
        int32_t *prior_eff = nullptr, *choice = nullptr, *over = nullptr, *slot = nullptr, *f2_src = nullptr;
        uint8_t *taken0 = nullptr, *mask = nullptr, *outl = nullptr;
        float2* bxy = nullptr;
        uint32_t *bjo = nullptr, *cand = nullptr;
        int *cstart = nullptr, *ccount = nullptr, *ints = nullptr;
        float *proj = nullptr, *Xg = nullptr;
        void* edges = nullptr;
        odo_pair_result* pres = nullptr;
        odo_local_map_result* res = nullptr;
        DevPool pool;
    } lm;
    int lm_cap = 0, lm_n = -1;  // lm_cap 0: not allocated
    LmGrid lm_grid{};
    // odo_local_ba's device block (upload, download and kernel scratch)
    DevBlock ba_dev;
    // odo_fuse_search's device block (upload, records, sorted points and cell starts)
    DevBlock fuse_dev;
    // odo_dense_clouds: the scratch block (plans, histograms, the (key, pixel)
    // ping-pong of every frame of a call) and the output block (the points,
    // then their counts at cloud_counts_at). cloud_n: the frames of the last call
    // (-1: none), cloud_off / cloud_np their first point and point count
    DevBlock cloud_dev, cloud_out;
    size_t cloud_counts_at = 0;
    int cloud_n = -1;
    std::vector<int32_t> cloud_off, cloud_np;
    // the grid GICP entry points (odo_gicp_grid_batch, odo_gicp_grid_covariances,
    // odo_gicp_dense): the point-sized block and the cell-sized block
    DevBlock gg_pts, gg_cells;
    // sequence state: the last tracked batch sits in frame set seq_set (its
    // last frame at slot seq_n); getters read view_set / view_n
    bool has_prev = false;
    uint64_t pair_counter = 0;
    int seq_set = NSETS - 1, seq_n = 0;
    int view_set = 0, last_n = 0;
    std::vector<int> valid_h;
    hipEvent_t ev[16];
    int nev = 0;
    // per set: the extraction of the set's batch is done; the PnP of the
    // set's batch (and, async, its result copy) is done
    hipEvent_t ev_xdone[NSETS] = {}, ev_pnp_done[NSETS] = {};
    bool pdone_rec[NSETS] = {};
    hipStream_t pdone_st[NSETS] = {};  // the stream that last recorded ev_pnp_done of a set
    // ODO_SERIAL_STREAMS (tuning): every stream aliases the extraction stream.
    // (Four streams in all, the copy stream included: every stream beyond the
    // process's GPU_MAX_HW_QUEUES (4) hardware queues would share one with
    // another stream and serialise behind it.)
    bool serial = false;
    bool timing = false;
    // ODO_SKIP (measurement only; results are invalid when set): bit 0 skips
    // the PnP launch, bit 2 every pair stage, bit 3 kNN-2, bit 4 RANSAC
    int skip = 0;
    // ADAPTIVE grid extractor (ODO_DETECTOR_ADAPTIVE_FAST): cell / band
    // tables and per-batch scratch (extraction stream only), plus the
    // persistent per-cell DetectorAdjuster thresholds
    bool adaptive = false;
    int ad_ncells = 0, ad_nbands = 0, ad_mpc = 0;
    std::vector<AdCell> adc_h;
    std::vector<AdBand> adb_h;
    AdCell* adc = nullptr;
    AdBand* adb = nullptr;
    uint8_t* smap = nullptr;
    size_t smap_stride = 0, acand_stride = 0, abig_stride = 0;
    uint32_t *acand = nullptr, *abig = nullptr, *acell = nullptr, *akp = nullptr;
    int *aband_cnt = nullptr, *ahist = nullptr, *atsel = nullptr, *ansel = nullptr, *acell_cnt = nullptr;
    double* athresh = nullptr;
    float a_cos = 1.f, a_sin = 0.f;
    // ODO_DETECTOR_ADAPTIVE_ORB (k_adaptive_orb.hip): cell-level images, bands,
    // S-map tiles; per-batch cell pyramids / S maps / survivors / selection
    // scratch (extraction stream only); the frame pyramid and its blur come
    // from pyr / blur
    bool adaptive_orb = false;
    std::vector<OaImg> oai_h;
    std::vector<OaCell> oac_h;
    std::vector<OaBand> oab_h;
    OaImg* oai = nullptr;
    OaCell* oac = nullptr;
    OaBand* oab = nullptr;
    OaScales osc{};
    int oa_ncap = 0, oa_buf0 = 0, oa_buf1 = 0, oa_maxpitch = 16;
    size_t cp_stride = 0, ocand_stride = 0, oscr_stride = 0;
    uint8_t *cpyr = nullptr, *oscr = nullptr;
    uint32_t* ocand = nullptr;
    int *oband_cnt = nullptr, *ohist = nullptr, *ophist = nullptr;
    uint64_t *ocell = nullptr, *oakp = nullptr;
    DevArena arena;  // per-stage entry points' device scratch
    int* h_open = nullptr;  // page-locked [NSETS]: RANSAC open pairs of the last batch per set (launch hint)
    // page-locked, host-coherent: k_latch writes 1 once the latch holds a
    // value; with ev_latch complete the host then stops ordering (and
    // launching) the no-op latch kernels of later batches
    int* latch_set_h = nullptr;
    // Hamming-match kernel timing (odo_set_timing mode 2): an event pair
    // around the kNN-2 launch of every batch, read back and summed lazily
    static constexpr int KT_RING = 256;
    bool ktiming = false;
    hipEvent_t kt0[KT_RING] = {}, kt1[KT_RING] = {};
    int kt_next = 0, kt_pending = 0;
    double kt_sum_ms = 0;
    long kt_count = 0;
    // per-step marks (odo_step_marks): every collected kNN-2 start as ms after
    // kt_ref, an event recorded when mode 2 was set
    hipEvent_t kt_ref = nullptr;
    std::vector<double> kt_marks;

    // Frees exactly what exists (also a context whose creation failed
    // half-way). Every owner above frees itself; the body releases them by hand
    // only for the order, since members are destroyed after the body: device
    // memory goes while the streams whose work may still use it exist (hipFree
    // waits for that work), then the events, then the streams. An owner
    // missing here is still freed, by its own destructor, after the streams.
    ~odo_ctx() {
        lm.pool.release();
        for (DevBlock* b : {&ba_dev, &fuse_dev, &cloud_dev, &cloud_out, &gg_pts, &gg_cells}) b->release();
        free_hyp_session(hs);
        pool.release();
        for (auto& R : rb) R.pool.release();
        arena.release();
        hyp_arena.release();
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        stage.release();
        hyp_stage.release();
        for (hipStream_t st : owned) (void)hipStreamDestroy(st);
        if (h_open) (void)hipHostFree(h_open);
        if (latch_set_h) (void)hipHostFree(latch_set_h);
    }
};

namespace odo {

inline size_t fbase(const odo_ctx* c, int set) { return (size_t)set * c->slots; }
// the set the next batch extracts into
inline int next_set(const odo_ctx* c) { return (c->seq_set + 1) % NSETS; }

// The per-frame output arrays of frame slot `slot` (fbase(set) + slot in set)
struct FrameSlot {
    orb_kp* kps;
    uint8_t* desc;
    float *kun, *xyz, *ur;
    int* nkp;
};
inline FrameSlot frame_at(const odo_ctx* c, size_t slot) {
    const size_t KC = (size_t)c->kp_cap;
    return {c->kps + slot * KC,     c->desc + slot * KC * 32, c->kun + slot * KC * 2,
            c->xyz + slot * KC * 3, c->ur + slot * KC,        c->nkp + slot};
}

// Stage-timing marks (odo_last_timings) are recorded only when enabled with
// odo_set_timing: timing events serialise the queue they sit on, which costs
// tens of microseconds per mark once several streams are busy.
inline void tmark(odo_ctx* c, int i, hipStream_t st) {
    if (c->timing) (void)hipEventRecord(c->ev[i], st);
}

// a carve of the calling entry point's arena (no free: the arena owns it)
struct DevBuf {
    void* p = nullptr;
    DevBuf(DevArena& a, size_t bytes) : p(a.take(bytes)) {}
    template <typename T>
    T* as() {
        return (T*)p;
    }
};
#define ARENA_CHECK(a) \
    if ((a).failed) return fail(ODO_ERR_DEVICE, "device scratch allocation failed")

int sync_all(odo_ctx* c);                      // odo_capi.cpp
int stage_reserve(odo_ctx* c, size_t bytes);   // grows c->stage (its contents are lost)
int kt_collect(odo_ctx* c, int i);
int build_geometry(odo_ctx* c);                // odo_geometry.cpp
int reset_adaptive(odo_ctx* c);
int run_extract(odo_ctx* c, int set, const uint8_t* d_bgr, const uint16_t* d_depth, int n, int slot0,
                bool geometry = true);         // odo_batch.cpp
void launch_set_knn2(odo_ctx* c, hipStream_t st, int s, int n);
int run_knn(odo_ctx* c, hipStream_t st, int s, int n);  // k_vo_lm + launch_set_knn2
int run_pair_match(odo_ctx* c, hipStream_t st, int set, int n, bool first_valid, bool latched);

// One packed round trip of a synchronous entry point. The sections are laid
// out with add(), the inputs first; the host side is the context's pinned
// staging buffer, the device side one block with the same offsets. upload()
// is one copy of [0, inputs' end), download() one copy of [outputs' begin, end).
struct Staged {
    Pack pk;
    size_t in_end = 0, out_begin = 0;
    uint8_t *h = nullptr, *d = nullptr;
    size_t add(size_t bytes) { return pk.add(bytes); }
    void mark_inputs_end() { in_end = pk.off; }
    void mark_outputs_begin() { out_begin = pk.off; }
    // the caller's own device block (at least pk.off bytes) ...
    int reserve(odo_ctx* c, uint8_t* block) {
        const int e = stage_reserve(c, pk.off);
        h = c->stage.p;
        d = block;
        return e;
    }
    // ... or a carve of an arena, which this call begins
    int reserve(odo_ctx* c, DevArena& a) {
        a.begin();
        int e;
        if ((e = reserve(c, nullptr))) return e;
        d = (uint8_t*)a.take(pk.off);
        ARENA_CHECK(a);
        return ODO_OK;
    }
    template <typename T>
    T* host(size_t off) const {
        return reinterpret_cast<T*>(h + off);
    }
    template <typename T>
    T* dev(size_t off) const {
        return reinterpret_cast<T*>(d + off);
    }
    hipError_t upload(hipStream_t st) const { return hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, st); }
    hipError_t download(hipStream_t st) const {
        return hipMemcpyAsync(h + out_begin, d + out_begin, pk.off - out_begin, hipMemcpyDeviceToHost, st);
    }
};

// ErrorFunction2 statics (ransac.cpp:352-359) and a pair's RANSAC constants
inline RansacCfg ransac_cfg(const odo_ransac_params& p, const odo_kernel_forms& f = odo_kernel_forms{}) {
    const double cam_angle_x = 58.0 / 180.0 * M_PI, cam_angle_y = 45.0 / 180.0 * M_PI;
    const double rsx = 3 * tan(cam_angle_x / 640.0), rsy = 3 * tan(cam_angle_y / 480.0);
    return RansacCfg{p.iterations, p.min_inlier_th, p.max_mahalanobis, p.sample_size, p.check_depth, rsx * rsx,
                     rsy * rsy, 0, f.ransac_lanes_min_open, 0, f.ransac_first_hyps};
}
inline FrameCalib frame_calib(const odo_calib& k) {
    return FrameCalib{k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, k.k3, k.depth_factor, k.mbf, 1.0f / k.fx, 1.0f / k.fy};
}

}  // namespace odo
