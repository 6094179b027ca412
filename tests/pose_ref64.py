"""Float64 references and input generators for the pose solvers -- TEST INFRASTRUCTURE.

Independent of the oracle (oracle/pose_ref.cpp restates the reference in its
float / double mix): plain numpy and scipy in float64, the same formulas
written once more. tests/test_pose_ref64.py checks these against closed-form
cases and the oracle against them on the CPU; tests/test_pose_solvers_gpu.py
checks the HIP kernels against both.
"""
from __future__ import annotations

import math

import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)


def bound_vs_ref64(oracle_dist: float, magnitude: float) -> float:
    """Bound on a kernel's distance from a float64 reference: 4 x the oracle's
    own distance from it on the same input (what the reference's float / double
    arithmetic costs; the factor covers another summation order and
    contracted FMAs), at least 4 float32 ulps of the case's largest magnitude."""
    return max(4.0 * float(oracle_dist), 4.0 * F32_EPS * max(float(magnitude), 1.0))


# ------------------------------------------------------------------ rotations
def rot(axis, deg):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    th = math.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def se3_exp(u):
    """exp of a twist (omega, upsilon) as a 4x4 matrix (g2o SE3Quat::exp's R and V)."""
    w, v = np.asarray(u[:3], np.float64), np.asarray(u[3:], np.float64)
    th = float(np.linalg.norm(w))
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O @ O
    if th < 1e-8:
        R = np.eye(3) + O + 0.5 * O2
        V = np.eye(3) + 0.5 * O + O2 / 6.0
    else:
        R = np.eye(3) + math.sin(th) / th * O + (1 - math.cos(th)) / th ** 2 * O2
        V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * O + (th - math.sin(th)) / th ** 3 * O2
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = V @ v
    return T


# --------------------------------------------------------------------- Kabsch
def kabsch64(A, B):
    """Kabsch::Compute (kabsch.cpp) in float64: centroids, M = sum (a - cA)(b - cB)^T,
    SVD, R = W diag(1, 1, sgn det M) V^T with det == 0 -> +1, t = cB - R cA.
    One deliberate departure from kabsch.cpp: for s2 <= 1e-9 s0 the sign is
    sgn det(W V^T), which makes R the proper rotation (see below).
    Returns (T 4x4, info) with info = dict(M, S (singular values), det, cA, cB)."""
    A = np.asarray(A, np.float64).reshape(-1, 3)
    B = np.asarray(B, np.float64).reshape(-1, 3)
    T = np.eye(4)
    if len(A) == 0:
        return T, dict(M=np.zeros((3, 3)), S=np.zeros(3), det=0.0, cA=np.zeros(3), cB=np.zeros(3))
    cA, cB = A.mean(0), B.mean(0)
    M = (A - cA).T @ (B - cB)
    V, S, Wt = np.linalg.svd(M)  # M = V S W^T
    det = float(np.linalg.det(M))
    sg = 1.0 if det == 0 else math.copysign(1.0, det)
    if S[2] <= 1e-9 * S[0]:
        # rank-deficient M (coplanar, collinear, identical points): det M is 0
        # or the LU's rounding noise, and the third singular vectors' signs
        # are LAPACK's choice, so the formula's R could be either of
        # W diag(1, 1, +-1) V^T. The proper rotation is the reference there
        # (det R = +1; for coplanar points it is the one rotation that maps
        # the plane as the data says)
        sg = 1.0 if np.linalg.det(Wt.T @ V.T) >= 0 else -1.0
    R = Wt.T @ np.diag([1.0, 1.0, sg]) @ V.T
    T[:3, :3] = R
    T[:3, 3] = cB - R @ cA
    return T, dict(M=M, S=S, det=det, cA=cA, cB=cB)


KABSCH_SIZES = (0, 1, 2, 3, 4, 255, 256, 257, 1025, 50000)
KABSCH_GEOMETRIES = ("exact", "noise", "rot170", "mirror", "coplanar", "collinear", "identical", "far",
                     "collinear_flip", "rod1", "rod2", "rod3", "far_small")
# sets whose data leave a rotation about a line, or all of it, open (also n < 3)
KABSCH_DEGENERATE = ("collinear", "collinear_flip", "identical")

KABSCH_GEOMETRY_SIZES = (257, 1025)


def kabsch_case(geometry: str, n: int):
    """(A, B) float32 point sets of one Kabsch case; deterministic per (geometry, n)."""
    rng = np.random.default_rng([KABSCH_GEOMETRIES.index(geometry), n, 0xCAB5])
    R = rot(rng.normal(size=3), 170.0 if geometry == "rot170" else 25.0)
    t = rng.normal(size=3) * 0.3
    A = rng.random((n, 3)) * 2 - 1
    if geometry == "coplanar":
        A[:, 2] = 0.5  # the plane z = 0.5: (A - cA)_z is exactly 0 in float and double
    elif geometry in ("collinear", "collinear_flip"):
        A = np.outer(rng.random(n) * 2 - 1, [0.6, -0.3, 0.74]) + [0.1, 0.2, 1.5]
    elif geometry == "identical":
        A = np.tile([0.3, -0.2, 1.7], (n, 1))
    elif geometry == "far":
        A = (rng.random((n, 3)) - 0.5) + [100.0, 0.0, 0.0]  # 1 m spread, 100 m out
    elif geometry == "far_small":
        A = (rng.random((n, 3)) - 0.5) * 1e-3 + [10.0, 0.0, 0.0]  # 1 mm spread, 10 m out
    elif geometry.startswith("rod"):
        # a 2 m rod 1, 2 or 3 % as thick as long: s1 / s0 of M about 1e-4 to 1e-3,
        # thin but three-dimensional, so the data fix the rotation. The rod
        # lies along x: M = C_A R^T then keeps the thin directions in rows of
        # their own size. (Turned to a generic direction, every entry of M is
        # of size s0 and rounding M to float, as kabsch.cpp does, costs
        # eps s0 / s1 = 1e-3 rad of roll before any solver runs.)
        thick = 0.01 * int(geometry[3:])
        A = A * [1.0, thick, thick] + [0.2, -0.1, 1.5]
    A = A.astype(np.float32)
    B = A.astype(np.float64) @ R.T + t
    if geometry == "noise":
        B = B + rng.normal(size=B.shape) * 1e-3
    elif geometry == "mirror":
        B = A.astype(np.float64) * [1.0, 1.0, -1.0] + t  # a reflection: det M < 0
    elif geometry == "collinear_flip":
        B = t - A.astype(np.float64)  # the line reversed: its direction in B is minus that in A
    return np.ascontiguousarray(A), np.ascontiguousarray(B.astype(np.float32))


def kabsch_is_unique(info) -> bool:
    """The rotation is determined when the second singular value of M is not
    negligible (two independent directions fix a rotation; the third then
    follows from the sign rule). s1 / s0 > 1e-3 is certainly enough; the
    cutoff here is 1e-5, between the thin rods (1e-4 to 1e-3), which are
    compared on all 16 elements too, and the collinear sets (1e-15). What
    float arithmetic can deliver on a determined case is measured by the
    oracle's own distance from the float64 result, which sets the bound."""
    S = info["S"]
    return bool(S[0] > 0 and S[1] / S[0] > 1e-5)


def kabsch_case_is_degenerate(geometry: str, n: int) -> bool:
    return geometry in KABSCH_DEGENERATE or n < 3


# ------------------------------------------------------------------------ PnP
class Cam:
    """fr1 intrinsics as the solvers see them: float32 values widened to double."""
    fx = float(np.float32(517.3))
    fy = float(np.float32(516.5))
    cx = float(np.float32(318.6))
    cy = float(np.float32(255.3))
    bf = float(np.float32(40.0))


CHI2_MONO, CHI2_STEREO = 5.991, 7.815

# k_pnp<true> keeps 45 B per edge slot in LDS (Xw 12, obs 12, info 4, flags 1,
# four float chi2 16), at most 96 KiB (pnp_lds_bytes, k_pnp.hip), and
# odo_pnp_motion_ba rounds the slot count up to a multiple of 64:
# 2176 slots = 97 920 B fit, the next multiple 2240 = 100 800 B does not. So
# n = 2176 is the last size on k_pnp<true> and n = 2177 (2240 slots) the first
# on k_pnp<false>; 2240 fills those slots.
PNP_LDS_LAST, PNP_HBM_FIRST = 2176, 2177
assert (PNP_LDS_LAST * 45 + 15) // 16 * 16 <= 96 * 1024 < ((PNP_LDS_LAST + 64) * 45 + 15) // 16 * 16
PNP_COUNTS = (0, 1, 2, 3, 9, 10, 11, 255, 256, 257, 301, 513, PNP_LDS_LAST, PNP_HBM_FIRST, 2240)
PNP_VARIANTS = ("mono", "stereo", "mixed", "noisefree_1cm", "init_exact", "init_far", "outliers30",
                "rot179_x", "rot179_y", "rot179_z", "rot179_111", "lost_mono", "lost_outliers30")
# an initial pose so far off (rotation in degrees, translation in metres) that
# the last round, which restarts there without the Huber kernel, has its
# trials rejected or diverges and every edge ends an outlier, while with the
# kernel still on it would converge: (data of, degrees, metres, seed)
PNP_LOST = {"lost_mono": ("mono", 30, 1.8, (30, 60, 2, 7)), "lost_outliers30": ("outliers30", 40, 0.8, (40, 80, 0, 7))}
PNP_VARIANT_N = 301
PNP_CASES = tuple(f"n{n}" for n in PNP_COUNTS) + PNP_VARIANTS
# seeds replaced where the oracle's own share of near-threshold edges exceeded
# the 1 % cap (tests/test_pose_ref64.py::test_pnp_cases_near_threshold_cap)
PNP_RESEED = {}


def pnp_case_n(name: str) -> int:
    """Edge count of a case (without generating it)."""
    return int(name[1:]) if name[0] == "n" and name[1:].isdigit() else PNP_VARIANT_N


def _project(Tcw, Xw):
    Xc = Xw @ Tcw[:3, :3].T + Tcw[:3, 3]
    iz = 1.0 / Xc[:, 2]
    u = Cam.fx * Xc[:, 0] * iz + Cam.cx
    v = Cam.fy * Xc[:, 1] * iz + Cam.cy
    return Xc, u, v, u - Cam.bf * iz


def pnp_case(name: str):
    """One motion-only PnP problem: dict(Xw (n,3) f32, obs (n,3) f32 with
    uR < 0 for mono edges, Tinit (4,4) f32, Ttrue (4,4) f64, n)."""
    if name in PNP_LOST:
        base, deg, metres, seed = PNP_LOST[name]
        c = pnp_case(base)
        rng = np.random.default_rng(list(seed))
        Tinit = se3_exp(np.r_[rot_vec(rng, deg), unit(rng) * metres]) @ c["Ttrue"]
        return dict(c, name=name, Tinit=np.ascontiguousarray(Tinit.astype(np.float32)))
    seed = PNP_RESEED.get(name, 0)
    rng = np.random.default_rng([PNP_CASES.index(name), seed, 0xB0A])
    n = pnp_case_n(name)
    variant = name if name in PNP_VARIANTS else "counts"
    Ttrue = np.eye(4)
    if variant.startswith("rot179"):
        axis = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "111": (1, 1, 1)}[variant.split("_")[1]]
        Ttrue[:3, :3] = rot(axis, 179.0)
    else:
        Ttrue[:3, :3] = rot(rng.normal(size=3), 3.0)
    Ttrue[:3, 3] = rng.normal(size=3) * 0.05
    # points in front of the camera, kept where the world depth (the
    # information weight is 1 / Xw.z^2) stays away from zero and the right
    # image coordinate is well inside the image
    Xw = np.zeros((0, 3), np.float32)
    while len(Xw) < n:
        Xc = rng.random((2 * n + 8, 3)) * [2, 1.5, 2] + [-1, -0.75, 1.0]
        W = ((Xc - Ttrue[:3, 3]) @ Ttrue[:3, :3]).astype(np.float32)
        keep = (np.abs(W[:, 2]) > 0.5) & (_project(Ttrue, W.astype(np.float64))[3] > 10.0)  # uR < 0 means mono
        Xw = np.concatenate([Xw, W[keep]])
    Xw = np.ascontiguousarray(Xw[:n])
    _, u, v, ur = _project(Ttrue, Xw.astype(np.float64))
    if variant == "mono":
        stereo = np.zeros(n, bool)
    elif variant == "stereo":
        stereo = np.ones(n, bool)
    else:
        stereo = rng.random(n) < 0.5
    obs = np.stack([u, v, np.where(stereo, ur, -1.0)], 1)
    exact = variant in ("noisefree_1cm", "init_exact")
    if not exact:
        obs[:, :2] += rng.normal(size=(n, 2)) * 0.3
        obs[:, 2] += np.where(stereo, rng.normal(size=n) * 0.3, 0.0)
        # gross outliers (10 %, or 30 %), and for n >= 20 some moderate ones on
        # both sides of the chi2 thresholds
        frac = 0.30 if variant == "outliers30" else 0.10
        g = rng.random(n) < frac
        obs[g, :2] += rng.choice([-1.0, 1.0], (int(g.sum()), 2)) * rng.uniform(20, 60, (int(g.sum()), 2))
        if n >= 20:
            m = (rng.random(n) < 0.08) & ~g
            obs[m, 0] += rng.choice([-1.0, 1.0], int(m.sum())) * rng.uniform(1.0, 8.0, int(m.sum()))
    obs[~stereo, 2] = -1.0
    if variant == "init_exact":
        Tinit = Ttrue.copy()
    elif variant == "init_far":
        Tinit = se3_exp(np.r_[rot_vec(rng, 10.0), unit(rng) * 0.20]) @ Ttrue
    else:
        Tinit = se3_exp(np.r_[rot_vec(rng, 0.2), unit(rng) * 0.01]) @ Ttrue  # 1 cm, 0.2 deg off
    return dict(name=name, n=n, Xw=Xw, obs=np.ascontiguousarray(obs.astype(np.float32)),
                Tinit=np.ascontiguousarray(Tinit.astype(np.float32)), Ttrue=Ttrue)


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def rot_vec(rng, deg):
    return unit(rng) * math.radians(deg)


def pnp_residuals(T, Xw, obs):
    """Information-weighted reprojection residuals in float64 (sqrt(info) * e,
    info = 1 / Xw.z^2 from the float32 z as the solvers compute it; mono edges
    2 rows, stereo edges 3), flattened, and the per-edge chi2."""
    Xw64 = np.asarray(Xw, np.float64)
    ob = np.asarray(obs, np.float64)
    z32 = np.asarray(Xw, np.float32)[:, 2]
    info = (np.float32(1.0) / (z32 * z32)).astype(np.float64)
    stereo = ~(np.asarray(obs)[:, 2] < 0)
    _, u, v, ur = _project(np.asarray(T, np.float64), Xw64)
    e = np.stack([ob[:, 0] - u, ob[:, 1] - v, np.where(stereo, ob[:, 2] - ur, 0.0)], 1)
    chi2 = info * (e * e).sum(1)
    return (np.sqrt(info)[:, None] * e).ravel(), chi2, stereo


def pnp_near_threshold(T, Xw, obs, margin=0.02):
    """Edges whose float64 chi2 at pose T lies within `margin` of its
    classification threshold (5.991 mono, 7.815 stereo)."""
    _, chi2, stereo = pnp_residuals(T, Xw, obs)
    th = np.where(stereo, CHI2_STEREO, CHI2_MONO)
    return np.abs(chi2 - th) <= margin * th


def pnp_polish(T, Xw, obs, inlier):
    """Least-squares optimum in float64 over the edges flagged `inlier`, started
    at T: scipy's trust-region solver on the info-weighted residuals, no robust
    kernel (the solver's rounds after the Huber kernel is dropped), the pose
    updated as exp(u) T. Returns (T_polished, max |T_polished - T|)."""
    from scipy.optimize import least_squares

    T0 = np.asarray(T, np.float64).reshape(4, 4)
    sel = np.asarray(inlier, bool)
    X, ob = np.asarray(Xw)[sel], np.asarray(obs)[sel]

    def fun(u):
        return pnp_residuals(se3_exp(u) @ T0, X, ob)[0]

    sol = least_squares(fun, np.zeros(6), method="trf", x_scale=1e-3, xtol=1e-15, ftol=1e-15, gtol=1e-15,
                        max_nfev=200)
    Tp = se3_exp(sol.x) @ T0
    return Tp, float(np.abs(Tp - T0).max())


# ----------------------------------------------------- RANSAC degenerate sets
RANSAC_GEOMETRIES = ("plane_z2", "z_levels", "shared_target_x", "duplicated", "collinear")


def ransac_case(geometry: str, corrupt: float, n: int = 300):
    """(xyz1, xyz2, matches as a dict of arrays) of one synthetic RANSAC input:
    match k pairs point k of F1 with point k of F2 (F2 = in-plane rigid motion
    of F1) unless corrupted, in which case its target is a random other point."""
    rng = np.random.default_rng([RANSAC_GEOMETRIES.index(geometry), int(corrupt * 100), n, 0x5AC])
    th = math.radians(4.0)
    R = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1.0]])
    t = np.array([0.05, -0.03, 0.0])
    P = rng.random((n, 3)) * [2, 1.5, 2] + [-1, -0.75, 1.0]
    if geometry == "plane_z2":
        P[:, 2] = 2.0
    elif geometry == "z_levels":
        P[:, 2] = 1.0 + 0.25 * rng.integers(0, 4, n)
    elif geometry == "collinear":
        P = np.outer(rng.random(n) * 2 - 1, [0.8, 0.5, 0.0]) + [0.0, 0.0, 1.5]
    Q = P @ R.T + t  # the motion keeps z: F2's z is F1's level exactly
    Q[:, 2] = P[:, 2]
    if geometry == "shared_target_x":
        Q[:, 0] = 0.25
    tr = np.arange(n)
    if geometry == "duplicated":  # match 2k + 1 repeats match 2k
        tr[1::2] = tr[0:n - 1:2][: len(tr[1::2])]
    qi = tr.copy()
    if corrupt > 0:
        sel = rng.random(n) < corrupt
        tr = np.where(sel, rng.integers(0, n, n), tr)
    dist = rng.integers(5, 60, n).astype(np.float32)
    return (np.ascontiguousarray(P.astype(np.float32)), np.ascontiguousarray(Q.astype(np.float32)),
            dict(queryIdx=qi.astype(np.int32), trainIdx=tr.astype(np.int32), distance=dist))
