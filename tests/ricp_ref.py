"""Reference composition of Odometry::Compute's ADAPTIVE_RICP / RANSAC modes
(odometry.cpp:46-92) from the unmodified CPU oracle — TEST INFRASTRUCTURE.

Per pair: O.track_pair for Ransac::Iterate (T12, rmse, mvInliers, the KnnMatch
list), Ransac::mpSourceCloud / mpTargetCloud rebuilt from the match list as
ransac.cpp:175-189 builds them, the branch rule of odometry.cpp:52-53 in
np.float32 arithmetic, O.gicp with the chosen guess, the fallbacks of
odometry.cpp:55-68 and F2's inlier flags (odometry.cpp:75-76).
"""
import numpy as np

import oracle_lib as O
from conftest import sequence

W, H, NFEAT = 640, 480, 1000
N_FRAMES = 12
DEFAULTS = dict(min_inliers=20, rmse_scale=10.0, refine_at=7.0, reset_at=20.0, gicp_iterations=10,
                gicp_max_corr_dist=0.07)


def crafted_sequence():
    """12 frames that drive Odometry::Compute(ADAPTIVE_RICP) through every
    branch under the reference's constants: a hard sequence with frame 4's
    depth zeroed (matches, none with depth), frame 7 replaced by a frame of
    another scene (RANSAC fails on real clouds) and frame 10 flat grey (no
    keypoints, no matches)."""
    bgr, dep, _ = sequence(N_FRAMES, W, H, seed=0x5EED0031, hard=True)
    other, odep, _ = sequence(3, W, H, seed=0x5EED0077)
    bgr, dep = bgr.copy(), dep.copy()  # the cached sequences stay as they are
    dep[4] = 0
    bgr[7], dep[7] = other[1], odep[1]
    bgr[10] = 128
    return bgr, dep


def extract_frames(bgr, dep, cal):
    return [O.extract_frame(bgr[i], dep[i], O.orb_params(NFEAT), cal) for i in range(len(bgr))]


def clouds(f1, f2, matches, rp):
    """mpSourceCloud / mpTargetCloud after Ransac::Iterate (ransac.cpp:161-189)."""
    empty = np.zeros((0, 3), np.float32)
    if len(matches) < rp.min_inlier_th:  # ransac.cpp:164
        return empty, empty
    s = f1["xyz"][matches["queryIdx"]]
    t = f2["xyz"][matches["trainIdx"]]
    if rp.check_depth:  # ransac.cpp:179-184
        keep = ~(np.isnan(s[:, 2]) | np.isnan(t[:, 2])) & ~((s[:, 2] <= 0) | (t[:, 2] <= 0))
        s, t = s[keep], t[keep]
    return np.ascontiguousarray(s, np.float32), np.ascontiguousarray(t, np.float32)


def decide(rmse, n_inliers, P):
    """odometry.cpp:52-53 in float: 0 keep RANSAC's mT12, 1 GICP from identity,
    2 GICP from mT12."""
    x = np.float32(rmse) * np.float32(P["rmse_scale"])
    if n_inliers < P["min_inliers"] or x >= np.float32(P["refine_at"]):
        return 1 if x >= np.float32(P["reset_at"]) else 2
    return 0


def ransac_pass(frames, cal, rp, seed_of):
    """Ransac::Iterate of every pair of the sequence (the DepthCovariance latch
    carried along). seed_of(i): RANSAC seed of pair i (frame i-1 -> frame i).
    Returns {i: (PairResult, KnnMatch list, latch after the pair)}."""
    out, latch = {}, float("nan")
    for i in range(1, len(frames)):
        r, _, matches, latch = O.track_pair(frames[i - 1], frames[i], cal, rp, seed_of(i), latch)
        out[i] = (r, matches, latch)
    return out


def compose(frames, passes, rp, mode="ricp", **params):
    """The sequence through Odometry(ADAPTIVE_RICP) (mode "ricp") or
    Odometry(RANSAC) (mode "ransac") on top of ransac_pass's results. Returns
    {i: dict} for i = 1 .. len(frames) - 1."""
    P = dict(DEFAULTS, **params)
    out = {}
    eye = np.eye(4, dtype=np.float32)
    for i in sorted(passes):
        f1, f2 = frames[i - 1], frames[i]
        r, matches, latch = passes[i]
        T_r = np.array(r.T12, np.float32).reshape(4, 4)
        src, tgt = clouds(f1, f2, matches, rp)
        br = decide(r.rmse, r.n_inliers, P) if mode == "ricp" else 0
        g = dict(T=eye.copy(), converged=0, iterations=0, n_corr=0)
        guess = None
        if br:
            guess = eye.copy() if br == 1 else T_r.copy()
            if len(src) >= 20 and len(tgt) >= 20:  # generalizedicp.cpp:33
                g = O.gicp(src, tgt, guess, P["gicp_iterations"], P["gicp_max_corr_dist"])
                if not g["converged"]:
                    g["T"] = eye.copy()  # generalizedicp.cpp:85
        if br == 0:
            Tcw = T_r
        elif g["converged"]:
            Tcw = np.array(g["T"], np.float32)
        else:
            Tcw = eye.copy() if br == 1 else T_r
        flags = np.zeros(len(f2["kps"]), np.uint8)
        flags[r.inliers["trainIdx"]] = 1  # odometry.cpp:75-76
        if br == 0:
            src = tgt = np.zeros((0, 3), np.float32)  # the batched path builds no cloud it does not use
        out[i] = dict(res=r, matches=matches, latch=latch, T_ransac=T_r, branch=br, src=src, tgt=tgt, guess=guess,
                      gicp_T=np.array(g["T"], np.float32).reshape(4, 4), converged=int(g["converged"]),
                      iterations=int(g["iterations"]), n_corr=int(g["n_corr"]), Tcw=Tcw, flags=flags)
    return out


def kind(e):
    """The four kinds of the crafted sequence's table."""
    if e["branch"] == 0:
        return "keep"
    if e["branch"] == 2:
        return "refine"
    return "reset_gicp" if len(e["src"]) >= 20 else "reset_empty"
