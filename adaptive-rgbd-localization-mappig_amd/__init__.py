"""MI355X-native per-frame odometry hot path of Adaptive-RGBD-Localization-Mapping.

The compute path is libodo_hip.so (hand-written HIP for gfx950, C-ABI in
include/odo.h). This package is a thin Python binding used by tests and
bench.py; the reference-shaped C++ adapters (Extractor / Matcher / Ransac /
PnPSolver / Kabsch) are shown in INTEGRATION.md.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import (DETECTOR_ADAPTIVE_FAST, DETECTOR_ADAPTIVE_ORB, DETECTOR_ORB_SLAM2, KNN_FORM_FP4, KNN_FORM_VALU,
                   PYRAMID_FORM_AUTO, PYRAMID_FORM_CHAIN, PYRAMID_FORM_FUSED, PYRAMID_FORM_FUSED_NOBLUR,
                   AdaptiveParams, Calib, Config, DMatch, PnPRansacResult,
                   DMATCH_DTYPE, KP_DTYPE, LANDMARK_DTYPE, LOCAL_MAP_DTYPE, LM_BAD, LM_HAS_OBS, LM_SEEN, LocalMapResult,
                   OrbParams, PAIR_DTYPE, PairResult, RansacParams, Rng, check, load, ptr,
                   ODOMETRY_ADAPTIVE_RBA, ODOMETRY_ADAPTIVE_RICP, ODOMETRY_RANSAC, RicpParams, RicpResult,
                   BA_EDGE_DTYPE, BA_NOTHING, BA_RAN, BaParams, BaResult,
                   FUSE_BAD, FUSE_BEHIND, FUSE_CAND_DTYPE, FUSE_CANDS, FUSE_KF_DTYPE, FUSE_NULL, FUSE_OUTSIDE,
                   CLOUD_DTYPE, CLOUD_INFO_DTYPE, CLOUD_OK, CLOUD_UNFILTERED, ERR_CAPACITY, SOR_INFO_DTYPE,
                   SOR_OK, SOR_SKIPPED, SOR_MAX_K,
                   ICP_RESULT_DTYPE, ICP_GATE_AS_WRITTEN, ICP_GATE_PLANE, ICP_OK, ICP_NO_MODEL, ICP_SHORT_TEMPLATE,
                   ICP_SINGULAR, IcpParams)

__all__ = ["Odometry", "HostFrames", "PinnedResults", "default_config", "load", "KP_DTYPE", "DMATCH_DTYPE", "PAIR_DTYPE", "rng_stream",
           "kabsch", "Calib", "OrbParams", "RansacParams", "Config", "AdaptiveParams", "DETECTOR_ORB_SLAM2",
           "DETECTOR_ADAPTIVE_FAST", "DETECTOR_ADAPTIVE_ORB", "KNN_FORM_FP4", "KNN_FORM_VALU",
           "PYRAMID_FORM_AUTO", "PYRAMID_FORM_FUSED", "PYRAMID_FORM_CHAIN",
           "PYRAMID_FORM_FUSED_NOBLUR", "ODOMETRY_ADAPTIVE_RBA", "ODOMETRY_RANSAC", "ODOMETRY_ADAPTIVE_RICP",
           "RicpParams", "RicpResult", "default_ricp_params", "LANDMARK_DTYPE", "LOCAL_MAP_DTYPE", "LocalMapResult",
           "LM_BAD", "LM_SEEN", "LM_HAS_OBS", "BA_EDGE_DTYPE", "BaParams", "BaResult", "BA_RAN", "BA_NOTHING",
           "default_ba_params", "fuse_best", "FUSE_KF_DTYPE", "FUSE_CAND_DTYPE", "FUSE_CANDS", "FUSE_NULL", "FUSE_BAD",
           "FUSE_BEHIND", "FUSE_OUTSIDE", "CLOUD_DTYPE", "CLOUD_INFO_DTYPE", "CLOUD_OK", "CLOUD_UNFILTERED",
           "SOR_INFO_DTYPE", "SOR_OK", "SOR_SKIPPED", "SOR_MAX_K", "ICP_RESULT_DTYPE", "ICP_GATE_AS_WRITTEN",
           "ICP_GATE_PLANE", "ICP_OK", "ICP_NO_MODEL", "ICP_SHORT_TEMPLATE", "ICP_SINGULAR", "IcpParams", "icp_params"]


def default_config(width=640, height=480, max_batch=1, nfeatures=1000, iterations=200, seed=0x5EED0000,
                   calib=None, detector=_abi.DETECTOR_ORB_SLAM2, forms=None) -> Config:
    """Reference defaults (extractor.cpp:86, odometry.cpp:28, common.h FR1).
    detector: DETECTOR_ORB_SLAM2 (main.cpp:19-21), DETECTOR_ADAPTIVE_FAST
    (Extractor(FAST, ORB, ADAPTIVE), extractor.cpp:55-77) or
    DETECTOR_ADAPTIVE_ORB (Extractor(ORB, ORB, ADAPTIVE): the cv::ORB cell
    detector of detectoradjuster.cpp:29). forms: odo_kernel_forms fields
    (knn = KNN_FORM_FP4 / KNN_FORM_VALU, knn_split, ransac_lanes_min_open,
    pyramid = PYRAMID_FORM_AUTO / PYRAMID_FORM_FUSED / PYRAMID_FORM_CHAIN /
    PYRAMID_FORM_FUSED_NOBLUR, ransac_first_hyps)."""
    cfg = Config()
    load().odo_default_config(ptr(cfg), width, height, max_batch)
    cfg.detector = detector
    cfg.orb.nfeatures = nfeatures
    cfg.ransac.iterations = iterations
    cfg.seed = seed
    if calib is not None:
        for k, v in calib.items():
            setattr(cfg.calib, k, v)
    for k, v in (forms or {}).items():  # odo_kernel_forms: bit-identical kernel alternatives
        setattr(cfg.forms, k, v)
    return cfg


def default_ba_params() -> BaParams:
    """odo_default_ba_params: the constants of localbundleadjustment.cpp (5 robust
    iterations, 10 final ones, Huber sqrt(5.991) / sqrt(7.815), chi2 5.991 / 7.815)."""
    p = BaParams()
    load().odo_default_ba_params(ptr(p))
    return p


def default_ricp_params() -> RicpParams:
    """odo_default_ricp_params: the constants of odometry.cpp:15, 52-53."""
    p = RicpParams()
    load().odo_default_ricp_params(ptr(p))
    return p


class HostFrames:
    """Page-locked host buffers for n frames of BGR8 + depth16 (odo_host_alloc):
    decode into `bgr` / `depth` (numpy views) and pass the object to
    Odometry.track_batch_host; the DMA engines read it without a staging copy."""

    def __init__(self, n: int, width: int, height: int):
        self.lib = load()
        self.n, self.w, self.h = n, width, height
        nb, nd = n * height * width * 3, n * height * width * 2
        self._pb = self.lib.odo_host_alloc(nb)
        self._pd = self.lib.odo_host_alloc(nd)
        if not self._pb or not self._pd:
            self.close()
            raise MemoryError("odo_host_alloc failed: " + self.lib.odo_last_error().decode())
        self.bgr = np.ctypeslib.as_array(C.cast(self._pb, C.POINTER(C.c_uint8)), (n, height, width, 3))
        self.depth = np.ctypeslib.as_array(C.cast(self._pd, C.POINTER(C.c_uint16)), (n, height, width))

    def close(self):
        for a in ("_pb", "_pd"):
            p = getattr(self, a, None)
            if p:
                self.lib.odo_host_free(p)
                setattr(self, a, None)
        self.bgr = self.depth = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedResults:
    """Page-locked ring of result records for Odometry.track_batch_async:
    `rows` batches of `n` records each (a numpy PAIR_DTYPE view per row)."""

    def __init__(self, rows: int, n: int):
        self.lib = load()
        self.rows, self.n = rows, n
        self._p = self.lib.odo_host_alloc(rows * n * PAIR_DTYPE.itemsize)
        if not self._p:
            raise MemoryError("odo_host_alloc failed: " + self.lib.odo_last_error().decode())
        raw = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), (rows * n * PAIR_DTYPE.itemsize,))
        self.all = raw.view(PAIR_DTYPE).reshape(rows, n)

    def row_ptr(self, r: int) -> int:
        return self._p + (r % self.rows) * self.n * PAIR_DTYPE.itemsize

    def close(self):
        if getattr(self, "_p", None):
            self.lib.odo_host_free(self._p)
            self._p = None
        self.all = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Odometry:
    """One context = one HIP stream + HBM scratch + previous-frame/latch state."""

    def __init__(self, cfg: Config, device: int = 0):
        self.lib = load()
        self.cfg = cfg
        h = self.lib.odo_create(ptr(cfg), device)
        if not h:
            raise RuntimeError("odo_create failed: " + self.lib.odo_last_error().decode())
        self.h = h
        self.kp_cap = max(cfg.orb.nfeatures + 4 * cfg.orb.nlevels + 64,
                          cfg.adaptive.max_total_keypoints + 64)

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return self.lib.odo_stream(self.h) or 0

    def reset(self):
        check(self.lib.odo_reset(self.h))

    def set_latch(self, v: float):
        check(self.lib.odo_set_latch(self.h, v))

    @property
    def latch(self) -> float:
        return self.lib.odo_get_latch(self.h)

    def set_odometry(self, mode: int, **params):
        """odo_set_odometry: the Odometry::Compute back-end of every track_batch*
        call from the next batch on (ODOMETRY_ADAPTIVE_RBA, ODOMETRY_RANSAC,
        ODOMETRY_ADAPTIVE_RICP). params: odo_ricp_params fields that differ
        from the reference's constants (min_inliers, rmse_scale, refine_at,
        reset_at, gicp_iterations, gicp_max_corr_dist)."""
        p = default_ricp_params()
        for k, v in params.items():
            if k not in dict(RicpParams._fields_):
                raise TypeError(f"odo_ricp_params has no field {k!r}")
            setattr(p, k, v)
        check(self.lib.odo_set_odometry(self.h, int(mode), ptr(p)))

    def odometry_mode(self) -> int:
        r = self.lib.odo_get_odometry(self.h)
        if r < 0:
            check(r)
        return r

    def ricp(self, i: int):
        """odo_get_ricp: what ADAPTIVE_RICP did for pair i of the last batch.
        Returns dict(T12 4x4, branch, converged, iterations, n_corr, n_cloud,
        src n_cloud x 3, tgt n_cloud x 3): the record and Ransac's
        mpSourceCloud / mpTargetCloud."""
        r = RicpResult()
        src = np.zeros((self.kp_cap, 3), np.float32)
        tgt = np.zeros((self.kp_cap, 3), np.float32)
        check(self.lib.odo_get_ricp(self.h, i, ptr(r), ptr(src), ptr(tgt), self.kp_cap))
        n = r.n_cloud
        return dict(T12=np.array(r.T12, np.float32).reshape(4, 4), branch=r.branch, converged=r.converged,
                    iterations=r.iterations, n_corr=r.n_corr, n_cloud=n, src=src[:n].copy(), tgt=tgt[:n].copy())

    def track_batch(self, bgr_ptr: int, depth_ptr: int, n: int, want_results=True):
        """Device-resident inputs (e.g. torch tensor .data_ptr())."""
        out = np.zeros(n, PAIR_DTYPE) if want_results else None
        check(self.lib.odo_track_batch(self.h, C.c_void_p(bgr_ptr), C.c_void_p(depth_ptr), n,
                                       ptr(out) if want_results else None))
        return out

    def track_batch_async(self, bgr_ptr: int, depth_ptr: int, n: int, results: PinnedResults, row: int):
        """Device-resident inputs; the n result records land in results.all[row]
        after the next synchronize() (no host sync here)."""
        check(self.lib.odo_track_batch_async(self.h, C.c_void_p(bgr_ptr), C.c_void_p(depth_ptr), n,
                                             C.c_void_p(results.row_ptr(row))))

    def seek(self, pair_index: int, keep_prev: bool = False):
        """Next batch's pair p gets global pair index pair_index + p; without
        keep_prev its first frame starts a segment (a halo frame, no pair)."""
        check(self.lib.odo_seek(self.h, int(pair_index), 1 if keep_prev else 0))

    def _host_frames(self, hf: "HostFrames", n):
        """(n, bgr pointer, depth pointer) of a HostFrames after checking that it
        holds n frames of this context's size: the C-ABI trusts n * W * H."""
        n = hf.n if n is None else int(n)
        if not 0 < n <= hf.n:
            raise ValueError(f"n = {n} frames requested from a HostFrames of {hf.n}")
        if (hf.w, hf.h) != (self.cfg.width, self.cfg.height):
            raise ValueError(f"HostFrames are {hf.w}x{hf.h}, the context tracks "
                             f"{self.cfg.width}x{self.cfg.height}")
        if hf._pb is None:
            raise ValueError("HostFrames closed")
        return n, hf._pb, hf._pd

    def track_batch_host(self, bgr, depth=None, want_results=True, n=None):
        """Host inputs: numpy arrays (pageable) or a HostFrames (pinned; then
        `n` frames of it, default all). Without results the call returns once
        the host buffers are consumed and the batch is queued (the upload
        overlaps the compute of earlier batches; the batch runs asynchronously)."""
        if isinstance(bgr, HostFrames):
            n, pb, pd = self._host_frames(bgr, n)
        else:
            bgr = np.ascontiguousarray(bgr, np.uint8)
            depth = np.ascontiguousarray(depth, np.uint16)
            W, H = self.cfg.width, self.cfg.height
            n = bgr.shape[0]
            if bgr.shape != (n, H, W, 3) or depth.shape != (n, H, W):
                raise ValueError(f"frames must be (n, {H}, {W}, 3) u8 and (n, {H}, {W}) u16, got "
                                 f"{bgr.shape} and {depth.shape}")
            pb, pd = ptr(bgr), ptr(depth)
        out = np.zeros(n, PAIR_DTYPE) if want_results else None
        check(self.lib.odo_track_batch_host(self.h, pb, pd, n, ptr(out) if want_results else None))
        return out

    def track_batch_host_async(self, hf: "HostFrames", results: "PinnedResults", row: int, n=None, first: int = 0):
        """odo_track_batch_host_async: frames [first, first + n) of a HostFrames
        uploaded and tracked, the records streamed into results.all[row] (valid
        after synchronize(); the host frames are consumed on return)."""
        n = (hf.n - first) if n is None else int(n)
        if first < 0 or not 0 < n <= hf.n - first or n > results.n:
            raise ValueError(f"frames [{first}, {first + n}) of {hf.n}, result rows of {results.n}")
        self._host_frames(hf, first + n)
        fb, fd = hf.w * hf.h * 3, hf.w * hf.h * 2
        check(self.lib.odo_track_batch_host_async(self.h, C.c_void_p(hf._pb + first * fb),
                                                  C.c_void_p(hf._pd + first * fd), n,
                                                  C.c_void_p(results.row_ptr(row))))

    def track_batch_host_sparse_depth(self, hf: "HostFrames", want_results=True, n=None):
        """odo_track_batch_host_sparse_depth: BGR uploaded, depth read in place
        from the pinned HostFrames. Until the batch has read it the depth view
        is made read-only (numpy raises on a refill): depth_wait(),
        depth_busy() == False or synchronize() release it."""
        n, pb, pd = self._host_frames(hf, n)
        out = np.zeros(n, PAIR_DTYPE) if want_results else None
        check(self.lib.odo_track_batch_host_sparse_depth(self.h, pb, pd, n, ptr(out) if want_results else None))
        if not want_results:
            hf.depth.flags.writeable = False
            self._depth_hold = getattr(self, "_depth_hold", []) + [hf]
        return out

    def _release_depth(self):
        # the event covers the last sparse batch; earlier ones ran before it
        # on the same stream
        for hf in getattr(self, "_depth_hold", []):
            if hf.depth is not None:
                hf.depth.flags.writeable = True
        self._depth_hold = []

    def depth_busy(self) -> bool:
        """odo_host_depth_query: the last sparse-depth batch may still read its depth frames."""
        r = self.lib.odo_host_depth_query(self.h)
        if r < 0:
            check(r)
        if r == 0:
            self._release_depth()
        return r == 1

    def depth_wait(self):
        """odo_host_depth_wait: block until the sparse-depth frames are released."""
        check(self.lib.odo_host_depth_wait(self.h))
        self._release_depth()

    def set_timing(self, enable, mode: int = None):
        """Timing mode: 0 off, 1 per-stage HIP events in odo_track_batch
        (serialises the streams a little; see timings()), 2 an event pair around
        the Hamming-match launch of every batch (see kernel_timing())."""
        m = mode if mode is not None else (1 if enable else 0)
        check(self.lib.odo_set_timing(self.h, m))

    def knn_replay_ms(self, reps: int = 20) -> float:
        """Mean duration of the last batch's kNN-2 launch re-run alone (measurement)."""
        ms = C.c_float(0)
        check(self.lib.odo_knn_replay_time(self.h, reps, C.byref(ms)))
        return float(ms.value)

    def kernel_timing(self):
        """(mean Hamming-match launch duration in ms, launches) since mode 2 was set."""
        avg = C.c_double(0)
        n = C.c_long(0)
        check(self.lib.odo_kernel_timing(self.h, C.byref(avg), C.byref(n)))
        return avg.value, n.value

    def step_marks(self):
        """odo_step_marks: the start (ms after set_timing mode 2) of every batch's
        kNN-2 launch since then; np.diff gives the per-step times."""
        n = self.lib.odo_step_marks(self.h, None, 0)
        if n < 0:
            check(n)
        buf = (C.c_double * max(1, n))()
        k = self.lib.odo_step_marks(self.h, buf, n)
        if k < 0:
            check(k)
        return [float(buf[i]) for i in range(min(k, n))]

    def synchronize(self):
        check(self.lib.odo_synchronize(self.h))
        self._release_depth()

    def frame(self, i: int):
        cap = self.kp_cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        kun = np.zeros((cap, 2), np.float32)
        xyz = np.zeros((cap, 3), np.float32)
        ur = np.zeros(cap, np.float32)
        n = C.c_int(0)
        check(self.lib.odo_get_frame(self.h, i, ptr(kps), ptr(desc), ptr(kun), ptr(xyz), ptr(ur), cap, C.byref(n)))
        m = n.value
        return dict(kps=kps[:m], desc=desc[:m], kun=kun[:m], xyz=xyz[:m], ur=ur[:m])

    def pair(self, i: int):
        cap = self.kp_cap
        matches = np.zeros(cap, DMATCH_DTYPE)
        good = np.zeros(cap, DMATCH_DTYPE)
        rin = np.zeros(cap, np.uint8)
        pin = np.zeros(cap, np.uint8)
        src = np.zeros(cap, np.int32)
        nm, ng = C.c_int(0), C.c_int(0)
        check(self.lib.odo_get_pair(self.h, i, ptr(matches), cap, C.byref(nm), ptr(good), C.byref(ng), ptr(rin),
                                    ptr(pin), ptr(src)))
        return dict(matches=matches[:nm.value], good=good[:ng.value], ransac_inliers=rin[:ng.value],
                    pnp_inliers=pin, f2_src=src)

    def kp_capacity(self) -> int:
        """odo_kp_capacity: keypoint slots per frame (the row length of a prior)."""
        r = self.lib.odo_kp_capacity(self.h)
        if r < 0:
            check(r)
        return r

    def track_local_map(self, lms, Tcw, prior=None, th: float = 8.0, nn_ratio: float = 0.8):
        """odo_track_local_map: Tracking::TrackLocalMap (tracking.cpp:231-261) for
        every frame of the last batch, on the device. lms: LANDMARK_DTYPE array;
        Tcw: n x 4 x 4 poses (world -> camera), one per frame of the batch;
        prior: n rows of slot -> landmark index (-1 empty; rows shorter than the
        keypoint capacity are padded with -1) or None. Every frame starts from
        its own pose: a refined pose does not feed the next frame. Returns a
        LOCAL_MAP_DTYPE array of n records."""
        lms = np.ascontiguousarray(lms, LANDMARK_DTYPE)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        n, kc = T.shape[0], self.kp_capacity()
        pr = None
        if prior is not None:
            pr = np.full((n, kc), -1, np.int32)
            if len(prior) != n:
                raise ValueError(f"prior has {len(prior)} rows for {n} poses")
            for i, row in enumerate(prior):
                row = np.asarray(row, np.int32)
                if row.size > kc:
                    raise ValueError(f"prior row {i} has {row.size} slots, the context {kc}")
                pr[i, :row.size] = row
        out = np.zeros(n, LOCAL_MAP_DTYPE)
        self._lm_n = None
        check(self.lib.odo_track_local_map(self.h, ptr(lms), len(lms), ptr(T), ptr(pr), kc, th, nn_ratio, ptr(out)))
        self._lm_n = len(lms)
        return out

    def local_ba(self, Tcw, kf_fixed, Xw, edges, calib: Calib = None, params: BaParams = None):
        """odo_local_ba: LocalBundleAdjustment::Compute (localbundleadjustment.cpp:65-315)
        on the device. Tcw: n_kf x 4 x 4 poses (world -> camera); kf_fixed: n_kf
        (non-zero: the keyframe is fixed); Xw: n_lm x 3; edges: BA_EDGE_DTYPE
        array (ur < 0: monocular). With params.iters_final = 0 it is
        GlobalBundleAdjustment. The inputs are not modified. Returns
        (Tcw n_kf x 4 x 4, Xw n_lm x 3, erase uint8 per edge, BaResult)."""
        T = np.array(Tcw, np.float32, order="C").reshape(-1, 16)
        X = np.array(Xw, np.float32, order="C").reshape(-1, 3)
        fx = np.ascontiguousarray(np.asarray(kf_fixed) != 0, np.uint8).reshape(-1)
        if len(fx) != len(T):
            raise ValueError(f"kf_fixed has {len(fx)} entries for {len(T)} poses")
        E = np.ascontiguousarray(edges, BA_EDGE_DTYPE).reshape(-1)
        erase = np.zeros(len(E), np.uint8)
        res = BaResult()
        check(self.lib.odo_local_ba(self.h, ptr(T), ptr(fx), len(T), ptr(X), len(X), ptr(E), len(E),
                                    ptr(calib) if calib is not None else None,
                                    ptr(params) if params is not None else None, ptr(erase), ptr(res)))
        return T.reshape(-1, 4, 4), X, erase, res

    def fuse_search(self, kfs, lms, lm_index, th: float = 4.0):
        """odo_fuse_search: the search of Matcher::Fuse (matcher.cpp:212-291) for
        every Fuse call of LocalMapping::FuseLandmarks in one device call. kfs:
        one (Tcw 4 x 4, kps_un n x 2, u_right n, desc n x 32, (lm_begin, lm_end))
        per call, its list the entries [lm_begin, lm_end) of lm_index (indices
        into lms; < 0 or >= len(lms): a null pointer); lms: LANDMARK_DTYPE array.
        Returns a FUSE_CAND_DTYPE array, one record per (call, list entry) in
        call order then list order; candidate indices are the keyframe's own."""
        lms = np.ascontiguousarray(lms, LANDMARK_DTYPE).reshape(-1)
        idx = np.ascontiguousarray(lm_index, np.int32).reshape(-1)
        K = np.zeros(len(kfs), FUSE_KF_DTYPE)
        kun, ur, desc, row = [], [], [], 0
        for k, (T, p, r, d, (lo, hi)) in enumerate(kfs):
            p = np.asarray(p, np.float32).reshape(-1, 2)
            r = np.asarray(r, np.float32).reshape(-1)
            d = np.asarray(d, np.uint8).reshape(-1, 32)
            if not len(p) == len(r) == len(d):
                raise ValueError(f"keyframe {k}: {len(p)} keypoints, {len(r)} right coordinates, {len(d)} descriptors")
            K[k] = (np.asarray(T, np.float32).reshape(16), row, row + len(p), lo, hi)
            row += len(p)
            kun.append(p)
            ur.append(r)
            desc.append(d)
        kun = np.ascontiguousarray(np.concatenate(kun)) if kun else np.zeros((0, 2), np.float32)
        ur = np.ascontiguousarray(np.concatenate(ur)) if ur else np.zeros(0, np.float32)
        desc = np.ascontiguousarray(np.concatenate(desc)) if desc else np.zeros((0, 32), np.uint8)
        out = np.zeros(int(np.maximum(K["lm_end"] - K["lm_begin"], 0).sum()), FUSE_CAND_DTYPE)
        check(self.lib.odo_fuse_search(self.h, ptr(K), len(K), ptr(kun), ptr(ur), ptr(desc), row, ptr(lms), len(lms),
                                       ptr(idx), len(idx), th, ptr(out)))
        return out

    def _twc(self, Twc, n):
        if Twc is None:
            return None
        T = np.ascontiguousarray(Twc, np.float32).reshape(-1, 16)
        if len(T) != n:
            raise ValueError(f"Twc: {len(T)} matrices for {n} frames")
        return T

    def dense_clouds(self, bgr_ptr: int, depth_ptr: int, n: int, leaf: float = 0.03, Twc=None):
        """odo_dense_clouds: Frame::CreateCloud + VoxelGridFilterCloud(leaf)
        (frame.cpp:191-226; leaf 0: CreateCloud alone) and the optional map
        transform Twc (n x 4 x 4) for n device-resident frames laid out as
        track_batch's. Returns the CLOUD_INFO_DTYPE records; the points stay on
        the device (get_dense_cloud, dense_cloud_device)."""
        info = np.zeros(n, CLOUD_INFO_DTYPE)
        T = self._twc(Twc, n)
        check(self.lib.odo_dense_clouds(self.h, C.c_void_p(bgr_ptr), C.c_void_p(depth_ptr), n, leaf, ptr(T), ptr(info)))
        return info

    def dense_clouds_host(self, bgr, depth, leaf: float = 0.03, Twc=None):
        """odo_dense_clouds_host: dense_clouds on host frames (n x H x W x 3 u8,
        n x H x W u16). Returns the infos."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        W, H = self.cfg.width, self.cfg.height
        n = bgr.shape[0]
        if bgr.shape != (n, H, W, 3) or depth.shape != (n, H, W):
            raise ValueError(f"expected bgr {(n, H, W, 3)} and depth {(n, H, W)}, got {bgr.shape} and {depth.shape}")
        info = np.zeros(n, CLOUD_INFO_DTYPE)
        T = self._twc(Twc, n)
        check(self.lib.odo_dense_clouds_host(self.h, ptr(bgr), ptr(depth), n, leaf, ptr(T), ptr(info)))
        return info

    def get_dense_cloud(self, i: int, counts: bool = False):
        """odo_get_dense_cloud: frame i of the last dense_clouds call as a
        CLOUD_DTYPE array; with counts=True (points, voxel populations)."""
        n = C.c_int(0)
        rc = self.lib.odo_get_dense_cloud(self.h, i, None, None, 0, C.byref(n))
        if rc not in (0, ERR_CAPACITY):
            check(rc)
        pts = np.zeros(n.value, CLOUD_DTYPE)
        cnt = np.zeros(n.value, np.int32) if counts else None
        check(self.lib.odo_get_dense_cloud(self.h, i, ptr(pts), ptr(cnt), n.value, C.byref(n)))
        return (pts, cnt) if counts else pts

    def dense_cloud_device(self, i: int):
        """odo_dense_cloud_device: (points pointer, counts pointer, n) of frame
        i where it lies in HBM, valid until the next dense-cloud call."""
        dp, dc, n = C.c_void_p(0), C.c_void_p(0), C.c_int(0)
        check(self.lib.odo_dense_cloud_device(self.h, i, C.byref(dp), C.byref(dc), C.byref(n)))
        return dp.value or 0, dc.value or 0, n.value

    def local_map(self, i: int):
        """odo_get_local_map: frame i of the last track_local_map. Returns
        dict(slot_lm nkp, proj n_lms x 3 (NaN: not in view), pnp_outlier nkp)."""
        if getattr(self, "_lm_n", None) is None:
            raise RuntimeError("local_map: no track_local_map call on this context")
        kc = self.kp_capacity()
        sl = np.full(kc, -1, np.int32)
        out = np.zeros(kc, np.uint8)
        proj = np.zeros((self._lm_n, 3), np.float32)
        m = self.frame_count(i)
        check(self.lib.odo_get_local_map(self.h, i, ptr(sl), ptr(proj), ptr(out), kc))
        return dict(slot_lm=sl[:m], proj=proj, pnp_outlier=out[:m])

    def frame_count(self, i: int) -> int:
        """Keypoints of frame i of the last batch."""
        n = C.c_int(0)
        rc = self.lib.odo_get_frame(self.h, i, None, None, None, None, None, 0, C.byref(n))
        if rc != 0 and rc != _abi.ERR_CAPACITY:
            check(rc)
        return n.value

    def debug_pyramid(self, i: int, total: int):
        out = np.zeros(total + 4096, np.uint8)
        n = self.lib.odo_debug_pyramid(self.h, i, ptr(out), out.size)
        if n < 0:
            check(n)
        return out[:n]

    def debug_blur(self, i: int, total: int):
        out = np.zeros(total + 4096, np.uint8)
        n = self.lib.odo_debug_blur(self.h, i, ptr(out), out.size)
        if n < 0:
            check(n)
        return out[:n]

    def debug_fast(self, i: int, level: int, cap: int = 1 << 18):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int(0)
        check(self.lib.odo_debug_fast(self.h, i, level, ptr(out), cap, C.byref(n)))
        return out[:n.value]

    def debug_octree(self, i: int, level: int, cap: int = 1 << 14):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int(0)
        check(self.lib.odo_debug_octree(self.h, i, level, ptr(out), cap, C.byref(n)))
        return out[:n.value]

    def adaptive_state(self, i: int = None):
        """(FAST threshold per grid cell used for frame i of the last batch or
        None, current per-cell DetectorAdjuster thresholds)."""
        nc = self.cfg.adaptive.grid_rows * self.cfg.adaptive.grid_cols
        t = np.zeros(nc, np.int32)
        th = np.zeros(nc, np.float64)
        rc = self.lib.odo_debug_adaptive(self.h, -1 if i is None else i, None if i is None else ptr(t), ptr(th))
        if rc < 0:
            check(rc)
        return (None if i is None else t), th

    def set_adaptive_thresholds(self, th):
        th = np.ascontiguousarray(th, np.float64)
        check(self.lib.odo_set_adaptive_thresholds(self.h, ptr(th), th.size))

    def select(self, keys, nth: int, mode: int = 0):
        """GPU std::nth_element (mode 0) / retainBest (mode 1) on packed keys."""
        keys = np.ascontiguousarray(keys, np.uint32)
        out = np.zeros_like(keys)
        n = C.c_int(0)
        check(self.lib.odo_debug_select(self.h, ptr(keys), keys.size, nth, mode, ptr(out), C.byref(n)))
        return out, n.value

    def match_features_buffers(self, n: int, fill: int = 0x5A):
        """The output arrays of odo_debug_match_features for n frames, every
        byte `fill`, and the odo_pair_stage_out that points at them."""
        kc, m = self.kp_capacity(), n - 1
        out = dict(lm_flags=np.empty((m, kc), np.uint8), qlist=np.empty((m, kc), np.int32),
                   qcnt=np.empty(m, np.int32), knn_idx=np.empty((m, kc, 2), np.int32),
                   knn_dist=np.empty((m, kc, 2), np.int32), matches=np.empty((m, kc), DMATCH_DTYPE),
                   n_matches=np.empty(m, np.int32), good=np.empty((m, kc), DMATCH_DTYPE),
                   n_good=np.empty(m, np.int32), f2_src=np.empty((m, kc), np.int32), latch=np.empty(1, np.float64))
        for a in out.values():
            a.view(np.uint8).fill(fill)
        return out, _abi.PairStageOut(**{k: a.ctypes.data for k, a in out.items()})

    def match_features(self, frames, fill: int = 0x5A):
        """odo_debug_match_features: the pair-match stage (VO landmarks, kNN-2,
        k_pair_match, latch) on len(frames) frames of (desc [cnt, 32] u8,
        xyz [cnt, 3] f32); pair p is (frame p, frame p + 1). Returns the full
        output arrays: what the call did not write still holds `fill` bytes."""
        kc, n = self.kp_capacity(), len(frames)
        counts = np.array([len(d) for d, _ in frames], np.int32)
        desc = np.full((n, kc, 32), fill, np.uint8)
        xyz = np.full((n, kc, 3), np.nan, np.float32)
        for i, (d, x) in enumerate(frames):
            desc[i, :len(d)] = d
            xyz[i, :len(d)] = x
        out, st = self.match_features_buffers(n, fill)
        check(self.lib.odo_debug_match_features(self.h, n, ptr(counts), ptr(desc), ptr(xyz), C.byref(st)))
        return out

    def pnp_ransac(self, Xw, uv, calib=None, iterations: int = 500, reproj_err: float = 3.0,
                   confidence: float = 0.85):
        """PnPRansac::Compute (pnpransac.cpp:11-51) on the GPU: cv::solvePnPRansac
        over n landmark observations. Returns (result, inlier mask, per-hypothesis
        inlier counts)."""
        Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = Xw.shape[0]
        res = PnPRansacResult()
        mask = np.zeros(max(n, 1), np.uint8)
        good = np.zeros(max(iterations, 1), np.int32)
        cal = calib if calib is not None else self.cfg.calib
        check(self.lib.odo_pnp_ransac(self.h, ptr(Xw), ptr(uv), n, ptr(cal), iterations, reproj_err, confidence,
                                      ptr(res), ptr(mask), ptr(good)))
        return res, mask[:n].astype(bool), good

    def pnp_ransac_batch(self, problems, calib=None, iterations: int = 500, reproj_err: float = 3.0,
                         confidence: float = 0.85):
        """PnPRansac::Compute for a list of (Xw n x 3, uv n x 2) problems in one
        launch chain. Returns (results[nprob], list of inlier masks)."""
        sizes = [len(x) for x, _ in problems]
        offs = np.zeros(len(problems) + 1, np.int32)
        offs[1:] = np.cumsum(sizes)
        Xw = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x, _ in problems])
                                  if problems else np.zeros((0, 3), np.float32))
        uv = np.ascontiguousarray(np.concatenate([np.asarray(u, np.float32).reshape(-1, 2) for _, u in problems])
                                  if problems else np.zeros((0, 2), np.float32))
        res = (PnPRansacResult * max(len(problems), 1))()
        mask = np.zeros(max(int(offs[-1]), 1), np.uint8)
        cal = calib if calib is not None else self.cfg.calib
        check(self.lib.odo_pnp_ransac_batch(self.h, ptr(Xw), ptr(uv), ptr(offs), len(problems), ptr(cal), iterations,
                                            reproj_err, confidence, C.cast(res, C.c_void_p), ptr(mask)))
        return [res[i] for i in range(len(problems))], [mask[offs[i]:offs[i + 1]].astype(bool)
                                                         for i in range(len(problems))]

    def gicp(self, src, tgt, guess=None, max_iterations: int = 10, max_corr_dist: float = 0.07):
        """GeneralizedICP(max_iterations, max_corr_dist)::Compute(source, target,
        guess) (generalizedicp.cpp:30-39, 65-89) on the GPU. Returns
        (T12 4x4, converged, iterations, n_corr)."""
        src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        g = np.ascontiguousarray(np.eye(4, dtype=np.float32) if guess is None else guess, np.float32)
        T = np.zeros(16, np.float32)
        conv, it, nc = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.odo_gicp(self.h, ptr(src), src.shape[0], ptr(tgt), tgt.shape[0], ptr(g), max_iterations,
                                max_corr_dist, ptr(T), C.byref(conv), C.byref(it), C.byref(nc)))
        return T.reshape(4, 4), conv.value, it.value, nc.value

    def gicp_batch(self, pairs, max_iterations: int = 10, max_corr_dist: float = 0.07):
        """GeneralizedICP::Compute for a list of (src n x 3, tgt m x 3, guess 4x4 or
        None) in one launch chain. Returns a list of (T12, converged, iterations,
        n_corr)."""
        P = len(pairs)
        so = np.zeros(P + 1, np.int32)
        to = np.zeros(P + 1, np.int32)
        so[1:] = np.cumsum([len(s) for s, _, _ in pairs])
        to[1:] = np.cumsum([len(t) for _, t, _ in pairs])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xs])
                                              if xs else np.zeros((0, 3), np.float32))
        src, tgt = cat([s for s, _, _ in pairs]), cat([t for _, t, _ in pairs])
        g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                           for _, _, q in pairs]) if P else np.zeros((1, 4, 4), np.float32))
        T = np.zeros((max(P, 1), 16), np.float32)
        conv, it, nc = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        check(self.lib.odo_gicp_batch(self.h, ptr(src), ptr(so), ptr(tgt), ptr(to), ptr(g), P, max_iterations,
                                      max_corr_dist, ptr(T), ptr(conv), ptr(it), ptr(nc)))
        return [(T[p].reshape(4, 4), int(conv[p]), int(it[p]), int(nc[p])) for p in range(P)]

    def gicp_covariances(self, clouds):
        """GICP's computeCovariances (k_gicp_cov alone) for a list of n x 3 clouds
        in one launch. Returns a list of n x 3 x 3 float64 arrays (zeros for a
        cloud under 20 points). Raises if the kernel's source and target sets
        differ (odo_gicp_covariances)."""
        offs = np.zeros(len(clouds) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in clouds])
        P = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
                                 if clouds else np.zeros((0, 3), np.float32))
        Cv = np.full((max(int(offs[-1]), 1), 9), np.nan)
        check(self.lib.odo_gicp_covariances(self.h, ptr(P), ptr(offs), len(clouds), ptr(Cv)))
        return [Cv[offs[p]:offs[p + 1]].reshape(-1, 3, 3) for p in range(len(clouds))]

    def gicp_grid_batch(self, pairs, max_iterations: int = 10, max_corr_dist: float = 0.07, cell: float = 0.0):
        """gicp_batch with the grid neighbour searches (odo_gicp_grid_batch): the
        same results bit for bit, clouds of up to 1048576 points. cell: the grid's
        cell edge in metres, 0 = chosen by the library."""
        P = len(pairs)
        so = np.zeros(P + 1, np.int32)
        to = np.zeros(P + 1, np.int32)
        so[1:] = np.cumsum([len(s) for s, _, _ in pairs])
        to[1:] = np.cumsum([len(t) for _, t, _ in pairs])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xs])
                                              if xs else np.zeros((0, 3), np.float32))
        src, tgt = cat([s for s, _, _ in pairs]), cat([t for _, t, _ in pairs])
        g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                           for _, _, q in pairs]) if P else np.zeros((1, 4, 4), np.float32))
        T = np.zeros((max(P, 1), 16), np.float32)
        conv, it, nc = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        check(self.lib.odo_gicp_grid_batch(self.h, ptr(src), ptr(so), ptr(tgt), ptr(to), ptr(g), P, max_iterations,
                                           max_corr_dist, cell, ptr(T), ptr(conv), ptr(it), ptr(nc)))
        return [(T[p].reshape(4, 4), int(conv[p]), int(it[p]), int(nc[p])) for p in range(P)]

    def gicp_grid_covariances(self, clouds, cell: float = 0.0):
        """gicp_covariances with the grid search (odo_gicp_grid_covariances): the
        same arrays bit for bit."""
        offs = np.zeros(len(clouds) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in clouds])
        P = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
                                 if clouds else np.zeros((0, 3), np.float32))
        Cv = np.full((max(int(offs[-1]), 1), 9), np.nan)
        check(self.lib.odo_gicp_grid_covariances(self.h, ptr(P), ptr(offs), len(clouds), cell, ptr(Cv)))
        return [Cv[offs[p]:offs[p + 1]].reshape(-1, 3, 3) for p in range(len(clouds))]

    def gicp_dense(self, pairs, guesses=None, max_iterations: int = 15, max_corr_dist: float = 0.05):
        """GeneralizedICP::Compute(pF1, pF2, guess) (odo_gicp_dense) for a list of
        (source frame, target frame) of the last dense_clouds call, on the clouds
        where they lie in HBM. guesses: a list of 4x4 or None per pair, or None.
        Returns a list of (T12, converged, iterations, n_corr)."""
        P = len(pairs)
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2) if P else np.zeros((1, 2), np.int32))
        g = None
        if guesses is not None and P:
            g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                               for q in guesses]))
            assert g.shape == (P, 4, 4)
        T = np.zeros((max(P, 1), 16), np.float32)
        conv, it, nc = (np.zeros(max(P, 1), np.int32) for _ in range(3))
        check(self.lib.odo_gicp_dense(self.h, ptr(pr), P, None if g is None else ptr(g), max_iterations,
                                      max_corr_dist, ptr(T), ptr(conv), ptr(it), ptr(nc)))
        return [(T[p].reshape(4, 4), int(conv[p]), int(it[p]), int(nc[p])) for p in range(P)]

    def dense_sor(self, mean_k: int = 50, stddev_mul: float = 1.0):
        """odo_dense_sor: Frame::StatisticalOutlierRemovalFilterCloud(mean_k,
        stddev_mul) on every cloud of the last dense-cloud call, in HBM. Returns
        the SOR_INFO_DTYPE records, one per frame."""
        info = np.zeros(self.cfg.max_batch, SOR_INFO_DTYPE)  # a dense-cloud call has at most max_batch frames
        info["status"] = -1
        check(self.lib.odo_dense_sor(self.h, mean_k, stddev_mul, ptr(info)))
        return info[info["status"] >= 0].copy()

    def cloud_sor_batch(self, clouds, mean_k: int = 50, stddev_mul: float = 1.0, cell: float = 0.0):
        """odo_cloud_sor_batch: StatisticalOutlierRemoval of a list of n x 3
        clouds in one launch chain. Returns (keeps: list of bool arrays,
        distances: list of float32 arrays, SOR_INFO_DTYPE records)."""
        offs = np.zeros(len(clouds) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in clouds])
        P = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
                                 if clouds else np.zeros((0, 3), np.float32))
        N = max(int(offs[-1]), 1)
        keep, dist = np.zeros(N, np.uint8), np.full(N, np.nan, np.float32)
        info = np.zeros(max(len(clouds), 1), SOR_INFO_DTYPE)
        check(self.lib.odo_cloud_sor_batch(self.h, ptr(P), ptr(offs), len(clouds), mean_k, stddev_mul, cell, ptr(keep),
                                           ptr(dist), ptr(info)))
        cut = lambda a: [a[offs[k]:offs[k + 1]] for k in range(len(clouds))]
        return cut(keep.astype(bool)), cut(dist), info[:len(clouds)]

    def gicp_grid_fitness(self, pairs, cell: float = 0.0):
        """odo_gicp_grid_fitness: getFitnessScore for a list of (src n x 3, tgt m x
        3, T 4x4 or None). Returns (scores float64, list of per-source-point
        nearest squared distances)."""
        P = len(pairs)
        so = np.zeros(P + 1, np.int32)
        to = np.zeros(P + 1, np.int32)
        so[1:] = np.cumsum([len(s) for s, _, _ in pairs])
        to[1:] = np.cumsum([len(t) for _, t, _ in pairs])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xs])
                                              if xs else np.zeros((0, 3), np.float32))
        src, tgt = cat([s for s, _, _ in pairs]), cat([t for _, t, _ in pairs])
        T = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                           for _, _, q in pairs]) if P else np.zeros((1, 4, 4), np.float32))
        score = np.zeros(max(P, 1))
        nn = np.full(max(int(so[-1]), 1), np.nan, np.float32)
        check(self.lib.odo_gicp_grid_fitness(self.h, ptr(src), ptr(so), ptr(tgt), ptr(to), ptr(T), P, cell, ptr(score),
                                             ptr(nn)))
        return score[:P], [nn[so[p]:so[p + 1]] for p in range(P)]

    def gicp_dense_fitness(self, pairs, T=None):
        """odo_gicp_dense_fitness: getFitnessScore for a list of (source frame,
        target frame) of the last dense-cloud call under T (a list of 4x4 or
        None per pair, or None: identities). Returns the float64 scores."""
        P = len(pairs)
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2) if P else np.zeros((1, 2), np.int32))
        Ts = [None] * P if T is None else list(T)
        assert len(Ts) == P
        M = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                           for q in Ts]) if P else np.zeros((1, 4, 4), np.float32))
        score = np.zeros(max(P, 1))
        check(self.lib.odo_gicp_dense_fitness(self.h, ptr(pr), P, ptr(M), ptr(score)))
        return score[:P]

    def icp_normals(self, clouds, num_neighbors: int = 10, cell: float = 0.0):
        """odo_icp_normals: libicp's computeNormals of a list of n x 3 clouds in one
        launch chain. Returns a list of n x 3 float32 arrays (zeros for a cloud
        under 5 points)."""
        offs = np.zeros(len(clouds) + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in clouds])
        P = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
                                 if clouds else np.zeros((0, 3), np.float32))
        nrm = np.full((max(int(offs[-1]), 1), 3), np.nan, np.float32)
        check(self.lib.odo_icp_normals(self.h, ptr(P), ptr(offs), len(clouds), num_neighbors, cell, ptr(nrm)))
        return [nrm[offs[k]:offs[k + 1]] for k in range(len(clouds))]

    def icp_plane_batch(self, pairs, params=None, cell: float = 0.0):
        """libicp's IcpPointToPlane(model).fit(template, R, t, indist)
        (odo_icp_plane_batch) for a list of (template n x 3, model m x 3, guess 4x4
        or None). params: an IcpParams (icp_params()), None = libicp's defaults.
        Returns the ICP_RESULT_DTYPE records, one per pair."""
        P = len(pairs)
        to = np.zeros(P + 1, np.int32)
        mo = np.zeros(P + 1, np.int32)
        to[1:] = np.cumsum([len(t) for t, _, _ in pairs])
        mo[1:] = np.cumsum([len(m) for _, m, _ in pairs])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xs])
                                              if xs else np.zeros((0, 3), np.float32))
        tmpl, model = cat([t for t, _, _ in pairs]), cat([m for _, m, _ in pairs])
        g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                           for _, _, q in pairs]) if P else np.zeros((1, 4, 4), np.float32))
        prm = icp_params() if params is None else params
        out = np.zeros(max(P, 1), ICP_RESULT_DTYPE)
        check(self.lib.odo_icp_plane_batch(self.h, ptr(tmpl), ptr(to), ptr(model), ptr(mo), ptr(g), P, C.byref(prm), cell,
                                           ptr(out)))
        return out[:P]

    def icp_plane_dense(self, pairs, guesses=None, params=None):
        """odo_icp_plane_dense: the same for a list of (template frame, model
        frame) of the last dense-cloud call, on the clouds where they lie in HBM.
        guesses: a list of 4x4 or None per pair, or None."""
        P = len(pairs)
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2) if P else np.zeros((1, 2), np.int32))
        g = None
        if guesses is not None and P:
            g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32) if q is None else np.asarray(q, np.float32)
                                               for q in guesses]))
            assert g.shape == (P, 4, 4)
        prm = icp_params() if params is None else params
        out = np.zeros(max(P, 1), ICP_RESULT_DTYPE)
        check(self.lib.odo_icp_plane_dense(self.h, ptr(pr), P, None if g is None else ptr(g), C.byref(prm), ptr(out)))
        return out[:P]

    def timings(self):
        ms = np.zeros(16, np.float32)
        names = (C.c_char_p * 16)()
        n = self.lib.odo_last_timings(self.h, ptr(ms), 16, C.cast(names, C.c_void_p))
        return {names[i].decode(): float(ms[i]) for i in range(n)}


def icp_params(num_neighbors: int = None, max_iterations: int = None, min_delta: float = None, indist: float = None,
               gate: int = None) -> "IcpParams":
    """odo_default_icp_params (libicp's 10, 200, 1e-4, -1, the gate as written)
    with the given fields replaced."""
    p = IcpParams()
    load().odo_default_icp_params(C.byref(p))
    for k, v in (("num_neighbors", num_neighbors), ("max_iterations", max_iterations), ("min_delta", min_delta),
                 ("indist", indist), ("gate", gate)):
        if v is not None:
            setattr(p, k, v)
    return p


def rng_stream(seed: int, n: int) -> np.ndarray:
    """glibc rand() stream as restated by the library (host helper)."""
    r = Rng()
    L = load()
    L.odo_rng_seed(ptr(r), seed)
    return np.array([L.odo_rng_next(ptr(r)) for _ in range(n)], np.int32)


def fuse_best(rec, kps_un, u_right, desc, new_desc, th: float = 4.0):
    """odo_fuse_best (host only): Fuse's (bestIdx, bestDist) of one fuse_search
    record under another descriptor. kps_un / u_right / desc: the record's
    keyframe; over rec["cand"] when n_cand <= 8, else the keyframe is scanned
    again with the window and the gate from the record's projection. Returns
    (-1, INT32_MAX) when nothing is gated."""
    r = np.ascontiguousarray(rec, FUSE_CAND_DTYPE).reshape(-1)[:1]
    p = np.ascontiguousarray(kps_un, np.float32).reshape(-1, 2)
    u = np.ascontiguousarray(u_right, np.float32).reshape(-1)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    nd = np.ascontiguousarray(new_desc, np.uint8).reshape(32)
    bi, bd = C.c_int32(0), C.c_int32(0)
    check(load().odo_fuse_best(ptr(r), ptr(p), ptr(u), ptr(d), len(p), th, ptr(nd), C.cast(C.byref(bi), C.c_void_p),
                               C.cast(C.byref(bd), C.c_void_p)))
    return bi.value, bd.value


def pair_seed(base: int, pair: int) -> int:
    """Per-pair RANSAC seed of the batched contract: splitmix64(base ^ pair), low 32 bits."""
    m = (1 << 64) - 1
    z = ((base ^ pair) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z & 0xFFFFFFFF


def kabsch(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    T = np.zeros(16, np.float32)
    check(load().odo_kabsch(ptr(A), ptr(B), A.shape[0], ptr(T)))
    return T.reshape(4, 4)
