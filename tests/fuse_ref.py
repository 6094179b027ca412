"""Reference of LocalMapping::FuseLandmarks (localmapping.cpp:155-191) and of
the search inside Matcher::Fuse (matcher.cpp:212-291), with the problem
builders the fuse tests share. No GPU, no library.

search_np     the search of one Fuse call, vectorised over the keyframe's
              keypoints: numpy float32 / float64 in the order include/odo.h
              pins (odo_fuse_search)
search_py     the same call transcribed pair by pair from matcher.cpp:221-291
              with np.float32 scalars, written independently of search_np
Landmark / KeyFrame   the part of the map Fuse touches: observations, nObs
              (+2 for a stereo keypoint), Replace with its same-id return,
              ComputeDistinctiveDescriptors, keyframe slots
fuse_landmarks   localmapping.cpp:155-191 with the search step pluggable:
              RefSearch answers at replay time from the map as it then is (the
              reference's own order of events), RecordSearch from records made
              before the loop (the device's contract) plus a re-score
"""
import copy

import numpy as np

f32, f64 = np.float32, np.float64
TH_LOW = 50
INT32_MAX = 2**31 - 1
CANDS = 8
NULL, BAD_LM, BEHIND, OUTSIDE = -1, -2, -3, -4
LM_BAD = 1
LANDMARK_DTYPE = np.dtype([("X", "<f4", 3), ("flags", "<i4"), ("desc", "u1", 32)])
CAND_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("n_cand", "<i4"), ("best_idx", "<i4"),
                       ("best_dist", "<i4"), ("cand", "<u2", CANDS)])
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)

# FR1 intrinsics without distortion (the bounds are the image, 640 x 480) and a
# camera whose projection of (x, y, 1) under the identity pose is (x, y)
# exactly, for the cases that sit on a comparison's edge
CAM_FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, mbf=40.0)
CAM_UNIT = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, mbf=0.5)
NO_DISTORTION = dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)


def camera(cam, bounds=BOUNDS):
    c = {k: f32(v) for k, v in cam.items()}
    c["bounds"] = tuple(f32(b) for b in bounds)
    return c


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def empty_records(n):
    r = np.zeros(n, CAND_DTYPE)
    r["u"] = r["v"] = r["ur"] = np.nan
    r["n_cand"] = NULL
    r["best_idx"] = -1
    r["best_dist"] = INT32_MAX
    r["cand"] = 0xFFFF
    return r


# ------------------------------------------------------------------ searches
def search_np(kf, lms, index, th, cam):
    """One Fuse call. kf = (Tcw, kps_un, u_right, desc); index: the list as
    indices into lms. Returns CAND_DTYPE records, one per list entry."""
    T, kun, kur, kdesc = kf
    T = np.asarray(T, f32).reshape(4, 4).astype(f64)
    kun = np.asarray(kun, f32).reshape(-1, 2)
    kur = np.asarray(kur, f32).reshape(-1)
    kdesc = np.asarray(kdesc, np.uint8).reshape(-1, 32)
    index = np.asarray(index, np.int64).reshape(-1)
    th = f32(th)
    out = empty_records(len(index))
    valid = (index >= 0) & (index < len(lms))
    L = lms[np.where(valid, index, 0)] if len(lms) else np.zeros(len(index), LANDMARK_DTYPE)
    X = L["X"].astype(f64)
    with np.errstate(all="ignore"):
        Pc = [(((T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1]) + T[k, 2] * X[:, 2]) + T[k, 3]).astype(f32) for k in range(3)]
        invz = f32(1) / Pc[2]
        x, y = Pc[0] * invz, Pc[1] * invz
        u, v = cam["fx"] * x + cam["cx"], cam["fy"] * y + cam["cy"]
        ur = u - cam["mbf"] * invz
        b = cam["bounds"]
        inside = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        behind = Pc[2] < f32(0)
    bad = (L["flags"] & LM_BAD) != 0
    state = np.where(~valid, NULL, np.where(bad, BAD_LM, np.where(behind, BEHIND, np.where(~inside, OUTSIDE, 0))))
    out["n_cand"] = state
    stereo = kur >= 0
    for i in np.nonzero(state == 0)[0]:
        out["u"][i], out["v"][i], out["ur"][i] = u[i], v[i], ur[i]
        with np.errstate(all="ignore"):
            win = (np.abs(kun[:, 0] - u[i]) < th) & (np.abs(kun[:, 1] - v[i]) < th)
            ex, ey, er = u[i] - kun[:, 0], v[i] - kun[:, 1], ur[i] - kur
            e2m = ex * ex + ey * ey
            e2s = e2m + er * er
            drop = np.where(stereo, e2s > f32(7.8), e2m > f32(5.99))
        js = np.nonzero(win & ~drop)[0]
        out["n_cand"][i] = len(js)
        if len(js):
            d = _POP[kdesc[js] ^ L["desc"][i]].sum(1)
            k = int(np.argmin(d))  # the first minimum
            out["best_idx"][i], out["best_dist"][i] = js[k], d[k]
            out["cand"][i, :min(len(js), CANDS)] = js[:CANDS]
    return out


def search_pair_py(T, kun, kur, kdesc, X, ldesc, th, cam):
    """matcher.cpp:228-291 for one landmark: (state, u, v, ur, gated indices in
    keypoint order, bestIdx, bestDist)."""
    T = [[f64(T[r][c]) for c in range(4)] for r in range(3)]
    X = [f64(f32(t)) for t in X]
    nan = f32(np.nan)
    with np.errstate(all="ignore"):
        p = [f32(((T[r][0] * X[0] + T[r][1] * X[1]) + T[r][2] * X[2]) + T[r][3]) for r in range(3)]
        if p[2] < f32(0.0):
            return BEHIND, nan, nan, nan, [], -1, INT32_MAX
        invz = f32(1) / p[2]
        x = p[0] * invz
        y = p[1] * invz
        u = cam["fx"] * x + cam["cx"]
        v = cam["fy"] * y + cam["cy"]
        mnx, mxx, mny, mxy = cam["bounds"]
        if not (u >= mnx and u < mxx and v >= mny and v < mxy):
            return OUTSIDE, nan, nan, nan, [], -1, INT32_MAX
        ur = u - cam["mbf"] * invz
        gated, best_dist, best_idx = [], INT32_MAX, -1
        for j in range(len(kun)):
            kx, ky = f32(kun[j][0]), f32(kun[j][1])
            if not (abs(kx - u) < th and abs(ky - v) < th):
                continue
            ex = u - kx
            ey = v - ky
            if f32(kur[j]) >= 0:
                er = ur - f32(kur[j])
                e2 = ex * ex + ey * ey + er * er
                if e2 > f32(7.8):
                    continue
            else:
                e2 = ex * ex + ey * ey
                if e2 > f32(5.99):
                    continue
            gated.append(j)
            d = hamming(ldesc, kdesc[j])
            if d < best_dist:
                best_dist, best_idx = d, j
    return 0, u, v, ur, gated, best_idx, best_dist


def search_py(kf, lms, index, th, cam):
    """One Fuse call, pair by pair (matcher.cpp:221-291)."""
    T, kun, kur, kdesc = kf
    T = np.asarray(T, f32).reshape(4, 4)
    kun = np.asarray(kun, f32).reshape(-1, 2)
    kur = np.asarray(kur, f32).reshape(-1)
    kdesc = np.asarray(kdesc, np.uint8).reshape(-1, 32)
    out = empty_records(len(index))
    for i, li in enumerate(index):
        if li < 0 or li >= len(lms):
            continue
        if lms["flags"][li] & LM_BAD:
            out["n_cand"][i] = BAD_LM
            continue
        st, u, v, ur, gated, bi, bd = search_pair_py(T, kun, kur, kdesc, lms["X"][li], lms["desc"][li], f32(th), cam)
        out["n_cand"][i] = st if st < 0 else len(gated)
        if st == 0:
            out["u"][i], out["v"][i], out["ur"][i] = u, v, ur
            out["best_idx"][i], out["best_dist"][i] = bi, bd
            out["cand"][i, :min(len(gated), CANDS)] = gated[:CANDS]
    return out


def search_calls(calls, lms, lm_index, th, cam, one=search_np):
    """The records of odo_fuse_search: calls = [(Tcw, kps_un, u_right, desc,
    (lm_begin, lm_end))], in call order then list order."""
    lm_index = np.asarray(lm_index, np.int64).reshape(-1)
    parts = [one(c[:4], lms, lm_index[c[4][0]:c[4][1]], th, cam) for c in calls]
    return np.concatenate(parts) if parts else empty_records(0)


def records_equal(a, b):
    """Field by field, the floats by bit pattern; returns the first difference or None."""
    if len(a) != len(b):
        return f"{len(a)} records for {len(b)}"
    for name in CAND_DTYPE.names:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            i = int(np.nonzero((x != y).reshape(len(a), -1).any(1))[0][0])
            return f"record {i}, {name}: {a[name][i]} != {b[name][i]} ({a[i]} vs {b[i]})"
    return None


# ----------------------------------------------------------------- map model
class KeyFrame:
    def __init__(self, kid, Tcw, kun, ur, desc):
        self.id = kid
        self.Tcw = np.asarray(Tcw, f32).reshape(4, 4)
        self.kun = np.asarray(kun, f32).reshape(-1, 2)
        self.ur = np.asarray(ur, f32).reshape(-1)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.slots = [None] * len(self.kun)  # mvpLandmarks

    def arrays(self):
        return self.Tcw, self.kun, self.ur, self.desc


class Landmark:
    def __init__(self, lid, X, desc):
        self.id = lid
        self.X = np.asarray(X, f32).reshape(3)
        self.desc = np.asarray(desc, np.uint8).reshape(32).copy()
        self.obs = {}  # keyframe -> keypoint index (a std::map: iterated in keyframe order, here by id)
        self.nobs = 0
        self.bad = False
        self.fuse_cand_for = -1

    def in_keyframe(self, kf):
        return kf in self.obs

    def add_observation(self, kf, idx):  # landmark.cpp:69-80
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.nobs += 2 if kf.ur[idx] >= 0 else 1

    def replace(self, other):  # landmark.cpp:160-192: this landmark goes, `other` stays
        if other.id == self.id:
            return
        obs, self.obs, self.bad = self.obs, {}, True
        for kf in sorted(obs, key=lambda k: k.id):
            idx = obs[kf]
            if not other.in_keyframe(kf):
                kf.slots[idx] = other
                other.add_observation(kf, idx)
            else:
                kf.slots[idx] = None
        other.compute_distinctive_descriptors()

    def compute_distinctive_descriptors(self):  # landmark.cpp:219-273
        if self.bad or not self.obs:
            return
        ds = [kf.desc[self.obs[kf]] for kf in sorted(self.obs, key=lambda k: k.id)]
        n = len(ds)
        dist = [[hamming(ds[i], ds[j]) for j in range(n)] for i in range(n)]
        best_median, best = None, 0
        for i in range(n):
            median = sorted(dist[i])[int(0.5 * (n - 1))]
            if best_median is None or median < best_median:
                best_median, best = median, i
        self.desc = ds[best].copy()


def fuse_call(kf, lst, res, stats):
    """Matcher::Fuse's loop (matcher.cpp:221-310) with the search of entry i
    taken from res.best(i, landmark) -> (bestIdx, bestDist) or None."""
    for i, lm in enumerate(lst):
        if lm is None:
            continue
        if lm.bad or lm.in_keyframe(kf):
            continue
        r = res.best(i, lm)
        if r is None:
            continue
        best_idx, best_dist = r
        if best_dist <= TH_LOW:
            in_kf = kf.slots[best_idx]
            if in_kf is not None:
                if not in_kf.bad:
                    if in_kf.nobs > lm.nobs:
                        lm.replace(in_kf)
                        stats["replace_lm"] += 1
                    else:
                        in_kf.replace(lm)
                        stats["replace_in_kf"] += 1
            else:
                lm.add_observation(kf, best_idx)
                kf.slots[best_idx] = lm
                stats["add"] += 1
            stats["fused"] += 1


def fuse_landmarks(current, targets, search, th=4.0):
    """localmapping.cpp:155-191. search(calls, th) with calls = [(keyframe,
    list of landmarks)] is asked once for the first loop and once for the
    reverse call; it returns one object per call with best(i, landmark)."""
    stats = dict(add=0, replace_lm=0, replace_in_kf=0, fused=0)
    lms = list(current.slots)
    res = search([(kf, lms) for kf in targets], th)
    for kf, r in zip(targets, res):
        fuse_call(kf, lms, r, stats)
    cands = []
    for kf in targets:
        for lm in list(kf.slots):
            if lm is None:
                continue
            if lm.bad or lm.fuse_cand_for == current.id:
                continue
            lm.fuse_cand_for = current.id
            cands.append(lm)
    res = search([(current, cands)], th)
    fuse_call(current, cands, res[0], stats)
    for lm in list(current.slots):
        if lm is not None and not lm.bad:
            lm.compute_distinctive_descriptors()
    return stats


class RefSearch:
    """The reference's own search: asked at replay time, on the map as it is
    then. With track=True it also searches under the descriptor the landmark
    had when the loop began and counts what a frozen search would get wrong."""

    def __init__(self, cam, track=False):
        self.cam, self.track = cam, track
        self.changed = self.changed_best = self.changed_over = 0

    def __call__(self, calls, th):
        return [_RefCall(self, kf, {id(lm): lm.desc.copy() for lm in lst if lm is not None}, th) for kf, lst in calls]


class _RefCall:
    def __init__(self, owner, kf, snap, th):
        self.o, self.kf, self.snap, self.th = owner, kf, snap, f32(th)

    def best(self, i, lm):
        kf = self.kf
        st, _, _, _, gated, bi, bd = search_pair_py(kf.Tcw, kf.kun, kf.ur, kf.desc, lm.X, lm.desc, self.th, self.o.cam)
        if self.o.track and st == 0 and not np.array_equal(self.snap[id(lm)], lm.desc):
            old = search_pair_py(kf.Tcw, kf.kun, kf.ur, kf.desc, lm.X, self.snap[id(lm)], self.th, self.o.cam)
            self.o.changed += 1
            self.o.changed_best += old[5] != bi
            self.o.changed_over += len(gated) > CANDS
        return None if st < 0 or not gated else (bi, bd)


class RecordSearch:
    """The device's contract: every call of a loop searched at once, before
    the replay, from the landmarks as they are then (records(calls, lms,
    lm_index, th) -> CAND_DTYPE array, e.g. Odometry.fuse_search); at replay a
    landmark whose descriptor has changed since is re-scored with rescore(rec,
    kps_un, u_right, desc, new_desc, th) (fuse_best). rescore=None: the stale
    best is used, which the scenario must expose."""

    def __init__(self, records, rescore):
        self.records, self.rescore = records, rescore
        self.rescored = 0

    def __call__(self, calls, th):
        uniq, index = {}, []
        for _, lst in calls:
            for lm in lst:
                if lm is not None and id(lm) not in uniq:
                    uniq[id(lm)] = (len(uniq), lm)
        lms = np.zeros(len(uniq), LANDMARK_DTYPE)
        for k, lm in uniq.values():
            lms[k] = (lm.X, LM_BAD if lm.bad else 0, lm.desc)
        flat, spans = [], []
        for kf, lst in calls:
            spans.append((len(flat), len(flat) + len(lst)))
            flat += [-1 if lm is None else uniq[id(lm)][0] for lm in lst]
        rec = self.records([kf.arrays() + (s,) for (kf, _), s in zip(calls, spans)], lms, np.array(flat, np.int32), th)
        snap = {k: lm.desc.copy() for k, (_, lm) in uniq.items()}
        return [_RecordCall(self, kf, rec[s[0]:s[1]], snap, th) for (kf, _), s in zip(calls, spans)]


class _RecordCall:
    def __init__(self, owner, kf, rec, snap, th):
        self.o, self.kf, self.rec, self.snap, self.th = owner, kf, rec, snap, th

    def best(self, i, lm):
        r = self.rec[i]
        if r["n_cand"] <= 0:
            return None
        if self.o.rescore is not None and not np.array_equal(self.snap[id(lm)], lm.desc):
            self.o.rescored += 1
            return self.o.rescore(r, self.kf.kun, self.kf.ur, self.kf.desc, lm.desc, self.th)
        return int(r["best_idx"]), int(r["best_dist"])


def map_state(kfs, lms):
    """What FuseLandmarks may change, in comparable form."""
    return dict(slots=[[-1 if s is None else s.id for s in kf.slots] for kf in kfs],
                obs=[sorted((kf.id, idx) for kf, idx in lm.obs.items()) for lm in lms],
                nobs=[lm.nobs for lm in lms], bad=[lm.bad for lm in lms], desc=[lm.desc.tobytes() for lm in lms])


# ------------------------------------------------------------------ builders
def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(rng, d, k):
    """d with k distinct bits flipped (Hamming distance exactly k)."""
    bits = np.unpackbits(np.asarray(d, np.uint8).reshape(32))
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def pose(rng, rot=0.02, trans=0.05):
    w = rng.normal(0, rot, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / max(th, 1e-12) * K + (1 - np.cos(th)) / max(th * th, 1e-12) * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(0, trans, 3)
    return T.astype(f32)


def random_call(rng, n_kp, n_lm, cam=CAM_FR1):
    """A keyframe of n_kp keypoints in clusters (so windows hold several), 70 %
    stereo, some outside the image; n_lm landmarks: keypoints back-projected at
    their depth with a little noise, descriptors a few bits away. Returns
    (kf, lms)."""
    T = pose(rng)
    nb = max((n_kp + 2) // 3, 1)
    base = np.column_stack([rng.uniform(-6, 646, nb), rng.uniform(-6, 486, nb)])
    kun = (base[rng.integers(0, nb, n_kp)] + rng.normal(0, 0.8, (n_kp, 2))).astype(f32)
    if n_kp > 4:
        kun[:4, 0] = [32.0, 64.0, 96.0, 31.999998]  # on and just off cell borders of the 32-pixel grid
        kun[:4, 1] = [32.0, 95.99999, 64.0, 64.0]
    depth = rng.uniform(0.5, 4.0, n_kp)
    ur = np.where(rng.random(n_kp) < 0.7, kun[:, 0] - cam["mbf"] / depth + rng.normal(0, 0.3, n_kp), -1.0).astype(f32)
    desc = rand_desc(rng, n_kp)
    lms = np.zeros(n_lm, LANDMARK_DTYPE)
    if n_kp and n_lm:
        src = rng.integers(0, n_kp, n_lm)
        px = kun[src].astype(f64) + rng.normal(0, 0.7, (n_lm, 2))
        away = rng.random(n_lm) < 0.15  # some project where no keypoint may be
        px[away] = np.column_stack([rng.uniform(-20, 660, n_lm), rng.uniform(-20, 500, n_lm)])[away]
        d = depth[src]
        Xc = np.column_stack([(px[:, 0] - cam["cx"]) / cam["fx"] * d, (px[:, 1] - cam["cy"]) / cam["fy"] * d, d])
        Twc = np.linalg.inv(T.astype(f64))
        lms["X"] = (Xc @ Twc[:3, :3].T + Twc[:3, 3]).astype(f32)
        for i in range(n_lm):
            lms["desc"][i] = flip_bits(rng, desc[src[i]], int(rng.integers(0, 60)))
    elif n_lm:
        lms["X"] = rng.normal(0, 1, (n_lm, 3)).astype(f32) + f32([0, 0, 2])
        lms["desc"] = rand_desc(rng, n_lm)
    return (T, kun, ur, desc), lms


def unit_call(points, kps):
    """Identity pose under CAM_UNIT: landmark (x, y, z) projects to (x / z, y /
    z). points: [(x, y, z, desc)], kps: [(x, y, u_right, desc)]."""
    lms = np.zeros(len(points), LANDMARK_DTYPE)
    for i, (x, y, z, d) in enumerate(points):
        lms[i] = ((x, y, z), 0, d)
    kun = np.array([[k[0], k[1]] for k in kps], f32).reshape(-1, 2)
    ur = np.array([k[2] for k in kps], f32)
    desc = np.array([k[3] for k in kps], np.uint8).reshape(-1, 32)
    return (np.eye(4, dtype=f32), kun, ur, desc), lms


def gate_offset(target, fixed):
    """float32 t >= 0 with fl(fl(fixed) + fl(t * t)) == target exactly."""
    target, fixed = f32(target), f32(fixed)
    t = f32(np.sqrt(f64(target) - f64(fixed)))
    for _ in range(64):
        t = np.nextafter(t, f32(0))
    for _ in range(256):
        if fixed + t * t == target:
            return t
        t = np.nextafter(t, f32(np.inf))
    raise AssertionError(f"no float32 offset reaches {target!r} from {fixed!r}")


def edge_cases():
    """name -> (calls, lms, lm_index, th) under CAM_UNIT, each aimed at one
    comparison of the search."""
    rng = np.random.default_rng(0xF05E)
    D = rand_desc(rng, 8)
    inv = lambda d: np.bitwise_xor(d, 255).astype(np.uint8)  # noqa: E731
    up = lambda t: np.nextafter(f32(t), f32(np.inf))  # noqa: E731
    dn = lambda t: np.nextafter(f32(t), f32(-np.inf))  # noqa: E731
    C = {}

    def one(name, points, kps, th=4.0, index=None):
        kf, lms = unit_call(points, kps)
        idx = np.arange(len(lms), dtype=np.int32) if index is None else np.asarray(index, np.int32)
        C[name] = ([kf + ((0, len(idx)),)], lms, idx, th)

    # depth: z just below 0, -0, +0, the smallest normal, a denormal; x = 0 keeps u finite
    tiny, den = f32(1.17549435e-38), f32(1e-40)
    one("depth", [(0, 0, dn(0), D[0]), (0, 0, f32(-0.0), D[0]), (0, 0, f32(0.0), D[0]), (1, 1, f32(0.0), D[0]),
                  (0, 0, tiny, D[0]), (1, 1, tiny, D[0]), (0, 0, den, D[0]), (1, 1, den, D[0]), (5, 5, -1, D[0])],
        [(0, 0, -1, D[0]), (5, 5, -1, D[0])])
    # bounds: min kept, max dropped, one step to either side
    one("bounds", [(0, 0, 1, D[0]), (dn(0), 0, 1, D[0]), (0, dn(0), 1, D[0]), (dn(640), dn(480), 1, D[0]),
                   (640, 10, 1, D[0]), (10, 480, 1, D[0]), (up(640), 10, 1, D[0])],
        [(0, 0, -1, D[0]), (639.5, 479.5, -1, D[0])])
    # window: |dx| == th is outside, one step nearer is inside (the gate passes both)
    for th in (2.0, 0.5):
        one(f"window_{th}", [(100, 100, 1, D[0])],
            [(100 + th, 100, -1, D[0]), (dn(100 + th), 100, -1, D[1]), (100, 100 - th, -1, D[0]),
             (100, up(100 - th), -1, D[2]), (up(100 - th), dn(100 + th), -1, D[3])], th=th)
    # gate: e2 on the bound is kept, one ulp above is dropped; v = 0 makes ey = -kp.y exact
    kps = []
    for bound in (f32(5.99), up(5.99), dn(5.99)):
        kps.append((0, gate_offset(bound, 4.0), -1, D[0]))       # mono: ex = 2, ex * ex = 4
    for bound in (f32(7.8), up(7.8), dn(7.8)):
        kps.append((2, gate_offset(bound, 6.25), 4.0, D[0]))     # stereo: ex = 0, ur = 1.5, er = -2.5
    one("gate", [(2, 0, 1, D[1])], kps)
    # right coordinate: 0 and -0 are stereo, < 0 and NaN mono
    r58, r65 = f32(np.sqrt(5.8)), f32(np.sqrt(6.5))
    one("right", [(2, 0, 1, D[0])],
        [(2, r58, 0.0, D[0]), (2, r58, -0.5, D[1]), (2, r65, 1.5, D[2]), (2, r65, -1.0, D[3]), (2, r58, f32(-0.0), D[4]),
         (2, r58, np.nan, D[5])])
    # distances 0 and 256
    one("dist", [(50, 50, 1, D[0]), (90, 50, 1, D[1])], [(50, 50, -1, D[0]), (90, 50, -1, inv(D[1]))])
    # ties: the lower index wins, also when it lies in a later grid cell (the border is at 32)
    one("ties", [(32, 32, 1, D[0]), (200, 200, 1, D[0])],
        [(33, 33, -1, D[1]), (31, 31, -1, D[1]), (201, 200, -1, D[2]), (200, 200, -1, D[2]), (199, 200, -1, D[2])])
    # 8, 9 and 40 coincident candidates, their indices interleaved and in falling grid order
    pts, kps = [], []
    for n, x in ((8, 100.0), (9, 300.0), (40, 500.0)):
        pts.append((x, 96, 1, D[0]))
    order = [(x, k) for k in range(40) for n, x in ((8, 100.0), (9, 300.0), (40, 500.0)) if k < n]
    for x, k in order[::-1]:
        kps.append((x, 96.5 if k % 2 else 95.5, -1, flip_bits(rng, D[0], 3 + (7 * k) % 11)))
        kps.append((x + 3.5, 96, -1, D[0]))  # in the window, beyond the gate
    one("counts", pts, kps)
    # grid: keypoints on cell borders and outside the image, windows across borders
    kps = [(32, 32, -1, D[0]), (31.999998, 32, -1, D[1]), (32, 31.999998, -1, D[2]), (-1.5, -1, -1, D[3]),
           (641, 481, -1, D[4]), (-40, 200, -1, D[5]), (700, 500, 2.0, D[6]), (639.9, 479.9, -1, D[7]),
           (np.nan, 5, -1, D[0]), (5, np.inf, -1, D[0])]
    one("grid", [(32, 32, 1, D[0]), (0, 0, 1, D[3]), (639.5, 479.5, 1, D[4]), (31, 33, 1, D[1]), (0, 200, 1, D[5])], kps)
    # list entries: null, out of range, BAD
    kf, lms = unit_call([(50, 50, 1, D[0]), (50, 50, 1, D[1]), (51, 50, 1, D[2])], [(50, 50, -1, D[0])])
    lms["flags"][1] = LM_BAD
    lms["flags"][2] = 6  # SEEN | HAS_OBS: not read
    idx = np.array([0, -1, 1, 3, 2, -7, 2**31 - 1, 0], np.int32)
    C["entries"] = ([kf + ((0, len(idx)),)], lms, idx, 4.0)
    return C


def shape_cases():
    """name -> (calls, lms, lm_index, th) under CAM_FR1: keypoint counts, list
    lengths and call counts around the kernel's steps (64-lane waves,
    256-thread workgroups, the 2048-keypoint staging chunk)."""
    C = {}
    for n_kp in (0, 1, 63, 64, 65, 2049):
        rng = np.random.default_rng(1000 + n_kp)
        kf, lms = random_call(rng, n_kp, 40)
        C[f"kp_{n_kp}"] = ([kf + ((0, 40),)], lms, np.arange(40, dtype=np.int32), 4.0)
    for n_lm in (0, 1, 255, 256, 257):
        rng = np.random.default_rng(2000 + n_lm)
        kf, lms = random_call(rng, 300, n_lm)
        C[f"list_{n_lm}"] = ([kf + ((0, n_lm),)], lms, np.arange(n_lm, dtype=np.int32), 4.0)
    rng = np.random.default_rng(3000)
    kf, lms = random_call(rng, 400, 300)
    kf2, _ = random_call(rng, 350, 0)
    kf2 = (kf[0],) + kf2[1:]  # the same view, other keypoints
    idx = np.arange(300, dtype=np.int32)
    C["calls_2_shared"] = ([kf + ((0, 300),), kf2 + ((0, 300),)], lms, idx, 4.0)
    C["th_0.5"] = ([kf + ((0, 300),)], lms, idx, 0.5)
    rng = np.random.default_rng(3061)
    kf, lms = random_call(rng, 500, 400)
    lms["flags"][rng.random(400) < 0.05] |= LM_BAD
    idx = rng.integers(-2, 404, 900).astype(np.int32)
    calls = []
    for k in range(61):
        kk, _ = random_call(rng, int(rng.integers(0, 130)), 0)
        lo = int(rng.integers(0, 900))
        hi = lo + int(rng.integers(0, min(900 - lo, 300) + 1)) if k % 7 else lo
        calls.append(((kf[0],) + kk[1:] if k % 3 else kf) + ((lo, hi),))
    C["calls_61_mixed"] = (calls, lms, idx, 4.0)
    return C


def scenario():
    """The crafted FuseLandmarks problem: a current keyframe (id 0), five
    targets (1-5) and one keyframe that only holds observations (6), over 200
    world points. Landmark A_i of the current keyframe's slot i; some targets
    hold duplicates B of the same point. Points 0-2 are built for the stale
    best and the rescan (see tests/test_fuse_ref.py); the rest is a mixture.
    Returns (keyframes, landmarks, current, targets, camera)."""
    cam = camera(CAM_FR1)
    rng = np.random.default_rng(0x5CE7A)
    NP, NT = 200, 5
    P = np.column_stack([rng.uniform(-1.0, 1.0, NP), rng.uniform(-0.7, 0.7, NP), rng.uniform(1.5, 3.5, NP)])
    P[:3] = [(0.1, 0.05, 2.0), (-0.3, 0.2, 2.5), (0.4, -0.25, 3.0)]  # the crafted points: in every view
    base = rand_desc(rng, NP)
    kfs = []
    for k in range(NT + 2):
        T = pose(rng, 0.01, 0.03) if k else np.eye(4, dtype=f32)
        Xc = P @ T[:3, :3].astype(f64).T + T[:3, 3].astype(f64)
        uv = np.column_stack([CAM_FR1["fx"] * Xc[:, 0] / Xc[:, 2] + CAM_FR1["cx"],
                              CAM_FR1["fy"] * Xc[:, 1] / Xc[:, 2] + CAM_FR1["cy"]])
        kun = (uv + rng.uniform(-0.5, 0.5, (NP, 2))).astype(f32)
        ur = (kun[:, 0] - CAM_FR1["mbf"] / Xc[:, 2]).astype(f32)
        if k == NT + 1:
            ur[:] = -1.0  # the extra keyframe is monocular: its observations count 1
        else:
            ur[rng.random(NP) < 0.25] = -1.0
        desc = np.array([flip_bits(rng, base[i], int(rng.integers(0, 12))) for i in range(NP)], np.uint8)
        kfs.append([T, kun, ur, desc])
    # the crafted points: descriptors Da (landmark A as it starts) and Db (what it becomes), 40 bits apart
    extra = {k: [] for k in range(NT + 2)}  # keypoints appended to a keyframe: (x, y, ur, desc)
    crafted = {}
    for i in range(3):
        Da = base[i]
        Db = flip_bits(rng, Da, 40)
        crafted[i] = (Da, Db)
        kfs[0][3][i] = Da
        kfs[0][2][i] = abs(kfs[0][1][i, 0] - f32(20.0))  # stereo in the current keyframe: A starts with nObs = 2
        kfs[1][3][i] = Db                            # keyframe 1's keypoint holds B, observed there and in 6
        kfs[1][2][i] = -1.0
        kfs[NT + 1][3][i] = Db
        for k in (2, 3, 4, 5):
            kfs[k][2][i] = -1.0
        # keyframe 2: the point's own keypoint looks like Da; a second keypoint beside it like Db
        kfs[2][3][i] = flip_bits(rng, Da, 2)
        x, y = kfs[2][1][i]
        extra[2].append((x + 0.25, y - 0.25, -1.0, flip_bits(rng, Db, 2)))
        # keyframe 3: twelve keypoints at one place, the nearest to Da first, the nearest to Db last
        x, y = kfs[3][1][i]
        kfs[3][3][i] = flip_bits(rng, Da, 1)
        for q in range(11):
            extra[3].append((x, y, -1.0, flip_bits(rng, Db, 1) if q == 10 else flip_bits(rng, Da, 30 + q)))
    K = []
    for k, (T, kun, ur, desc) in enumerate(kfs):
        if extra[k]:
            e = extra[k]
            kun = np.concatenate([kun, np.array([[t[0], t[1]] for t in e], f32)])
            ur = np.concatenate([ur, np.array([t[2] for t in e], f32)])
            desc = np.concatenate([desc, np.array([t[3] for t in e], np.uint8)])
        K.append(KeyFrame(k, T, kun, ur, desc))
    cur, targets, side = K[0], K[1:NT + 1], K[NT + 1]
    lms = []

    def new_lm(i, d):
        lm = Landmark(len(lms), P[i].astype(f32), d)
        lms.append(lm)
        return lm

    def observe(lm, kf, idx):
        lm.add_observation(kf, idx)
        kf.slots[idx] = lm

    for i in range(NP):
        A = new_lm(i, cur.desc[i])
        observe(A, cur, i)
        if i < 3:
            B = new_lm(i, crafted[i][1])  # nObs 2 (two mono keypoints) is not more than A's 2: B is replaced by A
            observe(B, K[1], i)
            observe(B, side, i)
            continue
        for kf in targets:
            r = rng.random()
            if r < 0.25:
                observe(A, kf, i)                      # already in the keyframe: skipped
            elif r < 0.40:
                B = new_lm(i, kf.desc[i])              # a duplicate with one observation: replaced by A
                observe(B, kf, i)
            elif r < 0.55:
                B = new_lm(i, kf.desc[i])              # a duplicate seen more often: A is replaced
                observe(B, kf, i)
                observe(B, side, i)
            # else: the slot is empty
    for i in (50, 51, 52):
        cur.slots[i].bad = True  # bad landmarks in the list
    cur.slots[60] = None         # and a null
    return K, lms, cur, targets, cam


_SC = {}


def scenario_reference():
    """The scenario run on the reference alone: (problem, final state, stats, RefSearch)."""
    if not _SC:
        prob = scenario()
        K, lms, cur, targets, cam = copy.deepcopy(prob)
        rs = RefSearch(cam, track=True)
        stats = fuse_landmarks(cur, targets, rs)
        _SC["v"] = (prob, map_state(K, lms), stats, rs)
    return _SC["v"]


def run_scenario(records, rescore):
    prob = scenario_reference()[0]
    K, lms, cur, targets, cam = copy.deepcopy(prob)
    s = RecordSearch(records, rescore)
    stats = fuse_landmarks(cur, targets, s)
    return map_state(K, lms), stats, s
