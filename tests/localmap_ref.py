"""Reference composition of Tracking::TrackLocalMap for a batch of frames
(tracking.cpp:231-261, 368-405), out of the oracle's pieces, and the problem
builders the local-map tests share. No GPU.

Per frame (odo_track_local_map's contract, include/odo.h): release the prior
slots whose landmark is BAD (UpdateLocalKFs, tracking.cpp:270-276), flag the
remaining prior landmarks SEEN for this frame (tracking.cpp:371-382), a prior
slot is taken iff its landmark has observations (matcher.cpp:114-117); then
oracle_projection_match; slot j = the search's landmark, else the surviving
prior, else -1; oracle_pnp over every slot holding a landmark, in slot order,
from the pose given; nInliers as tracking.cpp:247-255 counts them.

relaxation_rounds() simulates, on the reference semantics alone, the
synchronous relaxation k_lm_resolve runs in place of the serial landmark loop.
"""
from collections import namedtuple

import numpy as np

import oracle_lib as O
from conftest import sequence

BAD, SEEN, HAS_OBS = 1, 2, 4
TH_HIGH = 100
SEQ_SEED = 0x5EED0007  # the frames test_projection.py uses
NF = 1000

_CACHE = {}


def oracle_frames():
    """The three frames of the sequence as the oracle extracts them (the
    device extracts the same features: tests/test_gpu_parity.py)."""
    if "fr" not in _CACHE:
        bgr, dep, poses = sequence(3, seed=SEQ_SEED)
        cal = O.fr1_calib()
        _CACHE["fr"] = ([O.extract_frame(bgr[i], dep[i], O.orb_params(NF), cal) for i in range(3)], poses)
    return _CACHE["fr"]


def image_bounds(cal, w=640, h=480):
    b = np.zeros(4, np.float32)
    O.lib().oracle_image_bounds(O.C.byref(cal), w, h, O.ptr(b))
    return b


# ---------------------------------------------------------------- builders
def base_landmarks(frames, poses):
    """Depth-valid keypoints of frame 1 in world coordinates: (Xw, desc)."""
    f1 = frames[1]
    ok = f1["xyz"][:, 2] > 0
    Xc = f1["xyz"][ok].astype(np.float64)
    Twc = poses[1]
    return (Xc @ Twc[:3, :3].T + Twc[:3, 3]).astype(np.float32), f1["desc"][ok]


def true_poses(poses, idx=(0, 1, 2)):
    return np.stack([np.linalg.inv(poses[i]).astype(np.float32) for i in idx])


def problem(frames, lms, Tcw, prior=None, th=8.0, nn_ratio=0.8):
    return dict(frames=list(frames), lms=np.ascontiguousarray(lms), Tcw=np.ascontiguousarray(Tcw, np.float32),
                prior=prior, th=float(th), nn_ratio=float(nn_ratio), cal=O.fr1_calib())


def landmark_mix(frames, poses, seed=1, dup=60):
    """test_projection.make_problem's landmark mix: the base landmarks plus
    `dup` near-duplicates, shuffled, 70 % HAS_OBS, 4 % BAD, 4 % SEEN."""
    Xw, d1 = base_landmarks(frames, poses)
    rng = np.random.default_rng(seed)
    nL = len(Xw) + dup
    lms = np.zeros(nL, O.LANDMARK_DTYPE)
    lms["X"][:len(Xw)] = Xw
    lms["desc"][:len(Xw)] = d1
    pick = rng.integers(0, len(Xw), dup)
    lms["X"][len(Xw):] = Xw[pick] + rng.normal(0, 0.002, (dup, 3)).astype(np.float32)
    lms["desc"][len(Xw):] = d1[pick] ^ (rng.random((dup, 32)) < 0.03).astype(np.uint8)
    lms = lms[rng.permutation(nL)]
    fl = np.where(rng.random(nL) < 0.7, HAS_OBS, 0)
    fl |= np.where(rng.random(nL) < 0.04, BAD, 0)
    fl |= np.where(rng.random(nL) < 0.04, SEEN, 0)
    lms["flags"] = fl
    return lms


def copies(frames, poses, k, sigma, flip, has_obs, seed):
    """Every base landmark k times (the landmark and k - 1 copies moved by
    N(0, sigma) with a share `flip` of descriptor bits flipped), a share
    `has_obs` with observations, shuffled."""
    Xw, d1 = base_landmarks(frames, poses)
    rng = np.random.default_rng(seed)
    n = len(Xw)
    lms = np.zeros(n * k, O.LANDMARK_DTYPE)
    for c in range(k):
        X, d = Xw, d1
        if c:
            X = Xw + rng.normal(0, sigma, (n, 3)).astype(np.float32)
            d = np.packbits(np.unpackbits(d1, axis=1) ^ (rng.random((n, 256)) < flip).astype(np.uint8), axis=1)
        lms["X"][c * n:(c + 1) * n] = X
        lms["desc"][c * n:(c + 1) * n] = d
    lms["flags"] = np.where(rng.random(n * k) < has_obs, HAS_OBS, 0)
    return lms[rng.permutation(n * k)]


def base_problem(frames, poses):
    return problem(frames, landmark_mix(frames, poses), true_poses(poses), th=8.0)


def contended_landmarks(frames, poses):
    return copies(frames, poses, 3, 0.002, 0.03, 1.0, seed=11)


def contended_problem(frames, poses, th=8.0):
    return problem(frames, contended_landmarks(frames, poses), true_poses(poses), th=th)


def wide_problem(frames, poses):
    return contended_problem(frames, poses, th=40.0)


def half_obs_problem(frames, poses):
    return problem(frames, copies(frames, poses, 6, 0.01, 0.10, 0.5, seed=12), true_poses(poses), th=40.0)


def prior_problem(frames, poses, seed=13):
    """Prior of frame i = 30 % of the reference's own no-prior slots of that
    frame; 5 % of the landmarks those hold are then flagged BAD."""
    P = base_problem(frames, poses)
    ref = compose(P)
    rng = np.random.default_rng(seed)
    prior, held = [], []
    for r in ref:
        pr = np.where((r["slot_lm"] >= 0) & (rng.random(len(r["slot_lm"])) < 0.3), r["slot_lm"], -1).astype(np.int32)
        prior.append(pr)
        held.append(pr[pr >= 0])
    held = np.unique(np.concatenate(held))
    lms = P["lms"].copy()
    lms["flags"][held[rng.random(len(held)) < 0.05]] |= BAD
    return problem(frames, lms, P["Tcw"], prior=prior, th=8.0)


# ------------------------------------------------------------- composition
def frame_state(P, i):
    """(per-frame flags, surviving prior, taken slots) of frame i."""
    lms, n = P["lms"], len(P["frames"][i]["kun"])
    flags = lms["flags"].copy()
    pr = np.full(n, -1, np.int32)
    if P["prior"] is not None:
        row = np.asarray(P["prior"][i], np.int32)[:n]
        pr[:len(row)] = row
        pr[(pr < 0) | (pr >= len(lms))] = -1
        h = pr >= 0
        pr[h] = np.where(lms["flags"][pr[h]] & BAD, -1, pr[h])
        h = pr >= 0
        flags[pr[h]] |= SEEN
    taken = np.zeros(n, np.uint8)
    h = pr >= 0
    taken[h] = (lms["flags"][pr[h]] & HAS_OBS) != 0
    return flags, pr, taken


def in_frustum(Tcw, lms, flags, cal, b):
    """Frame::isInFrustum (frame.cpp:100-133) as odo_projection_match defines
    it: double-accumulated Rcw P + tcw rounded once, float projection, a NaN
    projection (Pc.z == 0) passes the bounds."""
    f32 = np.float32
    T = Tcw.astype(np.float64).reshape(4, 4)
    X = lms["X"].astype(np.float64)
    Pc = [(((T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1]) + T[k, 2] * X[:, 2]) + T[k, 3]).astype(f32) for k in range(3)]
    with np.errstate(all="ignore"):
        invz = f32(1) / Pc[2]
        u = (f32(cal.fx) * Pc[0]) * invz + f32(cal.cx)
        v = (f32(cal.fy) * Pc[1]) * invz + f32(cal.cy)
        return ((flags & (BAD | SEEN)) == 0) & ~(Pc[2] < 0) & ~((u < b[0]) | (u > b[1])) & ~((v < b[2]) | (v > b[3]))


def search(P, i):
    """oracle_projection_match for frame i: (slot_lm, proj, n_matches, state)."""
    f, cal = P["frames"][i], P["cal"]
    flags, pr, taken = frame_state(P, i)
    lms = P["lms"].copy()
    lms["flags"] = flags
    n, nL = len(f["kun"]), len(lms)
    b = image_bounds(cal)
    sl = np.full(max(n, 1), -1, np.int32)
    proj = np.full((max(nL, 1), 3), np.nan, np.float32)
    kun = np.ascontiguousarray(f["kun"], np.float32) if n else np.zeros((1, 2), np.float32)
    octv = np.ascontiguousarray(f["kps"]["octave"], np.int32) if n else np.zeros(1, np.int32)
    desc = np.ascontiguousarray(f["desc"], np.uint8) if n else np.zeros((1, 32), np.uint8)
    tk = taken if n else np.zeros(1, np.uint8)
    lm_arg = lms if nL else np.zeros(1, O.LANDMARK_DTYPE)
    T = np.ascontiguousarray(P["Tcw"][i], np.float32).ravel()
    nm = O.lib().oracle_projection_match(O.ptr(T), O.ptr(lm_arg), nL, O.ptr(kun), O.ptr(octv), O.ptr(desc), n,
                                         O.ptr(tk), O.C.byref(cal), O.ptr(b), P["th"], P["nn_ratio"], O.ptr(sl),
                                         O.ptr(proj))
    n_in_view = int(in_frustum(T, lms, flags, cal, b).sum()) if nL else 0
    return sl[:n], proj[:nL], int(nm), dict(flags=flags, prior=pr, taken=taken, n_in_view=n_in_view)


def compose(P):
    """The reference TrackLocalMap of every frame: a list of dicts."""
    out = []
    for i, f in enumerate(P["frames"]):
        sl, proj, nm, st = search(P, i)
        slot = np.where(sl >= 0, sl, st["prior"]).astype(np.int32)
        idx = np.nonzero(slot >= 0)[0]
        ne = len(idx)
        Xw = np.ascontiguousarray(P["lms"]["X"][slot[idx]], np.float32).reshape(-1, 3)
        obs = np.ascontiguousarray(np.column_stack([f["kun"][idx, 0], f["kun"][idx, 1], f["ur"][idx]]),
                                   np.float32).reshape(-1, 3)
        T0 = np.ascontiguousarray(P["Tcw"][i], np.float32).ravel()
        T = np.zeros(16, np.float32)
        outl = np.zeros(max(ne, 1), np.uint8)
        Xa, oa = (Xw, obs) if ne else (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
        ninl = O.lib().oracle_pnp(O.ptr(Xa), O.ptr(oa), ne, O.C.byref(P["cal"]), O.ptr(T0), O.ptr(T), O.ptr(outl))
        outl = outl[:ne].astype(bool)
        has = (P["lms"]["flags"][slot[idx]] & HAS_OBS) != 0
        outlier = np.zeros(len(slot), np.uint8)
        outlier[idx] = outl
        out.append(dict(slot_lm=slot, search_slot=sl, proj=proj, n_in_view=st["n_in_view"], n_matches=nm, n_edges=ne,
                        Tcw=T.copy(), pnp_inliers=int(ninl), n_map_inliers=int((~outl & has).sum()),
                        pnp_outlier=outlier, prior=st["prior"]))
    return out


# -------------------------------------------------------------- relaxation
Relaxation = namedtuple("Relaxation", "rounds moved slot_lm n_matches over16 shared_slots")


def relaxation_rounds(P, i=2):
    """The synchronous relaxation on the reference semantics, frame i: every
    landmark chooses at once, slot j taken iff it was taken at the start or
    owner[j] < landmark index, owner[j] = the smallest index of a HAS_OBS
    landmark that chose j in the round before; until no choice changes. A
    landmark's choice: the two smallest (distance, keypoint) among its untaken
    window keypoints, TH_HIGH and the same-level ratio test
    (matcher.cpp:107-141). Returns Relaxation(rounds in which a choice
    changed, landmarks whose first-round choice differs from the final one,
    slot_lm = the largest index that chose each slot, landmarks with a choice,
    windows of more than 16 keypoints, slots chosen by two or more landmarks)."""
    f = P["frames"][i]
    _, proj, _, st = search(P, i)
    flags, taken0 = st["flags"], st["taken"].astype(bool)
    lms, th, ratio = P["lms"], np.float32(P["th"]), float(np.float32(P["nn_ratio"]))
    kun, octv = f["kun"].astype(np.float32), f["kps"]["octave"].astype(np.int64)
    bits = np.unpackbits(f["desc"], axis=1)
    n = len(kun)
    b = image_bounds(P["cal"])
    inview = in_frustum(np.ascontiguousarray(P["Tcw"][i], np.float32).ravel(), lms, flags, P["cal"], b)
    cands, over16 = {}, 0
    for k in np.nonzero(inview & ((flags & BAD) == 0))[0]:
        u, v = proj[k, 0], proj[k, 1]
        with np.errstate(invalid="ignore"):
            w = np.nonzero((np.abs(kun[:, 0] - u) < th) & (np.abs(kun[:, 1] - v) < th))[0]
        if len(w) == 0:
            continue
        over16 += len(w) > 16
        d = (bits[w] ^ np.unpackbits(lms["desc"][k])).sum(1)
        order = np.lexsort((w, d))
        cands[int(k)] = [(int(d[o]), int(w[o]), int(octv[w[o]])) for o in order]
    has = (flags & HAS_OBS) != 0
    big = 1 << 30
    owner = np.where(taken0, -1, big)
    choice, first, rounds = {}, None, 0
    while True:
        new = {}
        for k, lst in cands.items():
            two = [c for c in lst if not owner[c[1]] < k][:2]
            if not two or two[0][0] > TH_HIGH:
                continue
            if len(two) == 2 and two[0][2] == two[1][2] and two[0][0] > ratio * two[1][0]:
                continue
            new[k] = two[0][1]
        if first is None:
            first = dict(new)
        if new == choice:
            break
        rounds += 1
        choice = new
        owner = np.where(taken0, -1, big)
        for k, j in choice.items():
            if has[k]:
                owner[j] = min(owner[j], k)
    slot = np.full(n, -1, np.int32)
    count = np.zeros(n, np.int32)
    for k in sorted(choice):
        slot[choice[k]] = k
        count[choice[k]] += 1
    moved = sum(1 for k in cands if first.get(k, -1) != choice.get(k, -1))
    return Relaxation(rounds, moved, slot, len(choice), int(over16), int((count >= 2).sum()))
