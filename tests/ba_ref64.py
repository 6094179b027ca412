"""Float64 reference and case builders for local bundle adjustment -- TEST INFRASTRUCTURE.

A numpy restatement of odo_local_ba (include/odo.h): g2o's
OptimizationAlgorithmLevenberg over SE3 pose vertices and marginalised XYZ
point vertices with mono / stereo reprojection edges, as
LocalBundleAdjustment::Compute drives it (two optimize() calls with an
outlier classification between them). Written independently of
csrc/k_ba.hip: dense numpy, the active vertices compacted, `order` choosing
the sequence in which edges are accumulated and `solver` the factorisation
of the reduced system. tests/test_ba_ref64.py checks it against things it
cannot have been fitted to; tests/test_ba_gpu.py checks the kernels against it.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from pose_ref64 import Cam, unit

BA_EDGE_DTYPE = np.dtype([("kf", "<i4"), ("lm", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4")])
BA_EDGE_DTYPE64 = np.dtype([("kf", "<i4"), ("lm", "<i4"), ("u", "<f8"), ("v", "<f8"), ("ur", "<f8")])  # reference only
DBL_MAX = float(np.finfo(np.float64).max)


def default_params(**kw):
    """odo_default_ba_params(): the values of localbundleadjustment.cpp."""
    p = dict(iters_robust=5, iters_final=10, robust=1,
             huber_mono=float(np.float32(math.sqrt(5.991))), huber_stereo=float(np.float32(math.sqrt(7.815))),
             chi2_mono=float(np.float32(5.991)), chi2_stereo=float(np.float32(7.815)))
    p.update(kw)
    return p


# ------------------------------------------------------------------- geometry
def quat_roundtrip(R):
    """Rotation matrix -> unit quaternion (w >= 0) -> rotation matrix, as the
    SE3Quat constructor stores a pose (Converter::toSE3Quat)."""
    m = np.asarray(R, np.float64)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        x, y, z = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
    else:
        i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q = [0.0, 0.0, 0.0]
        q[i] = 0.5 * s
        s = 0.5 / s
        w = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
        x, y, z = q
    v = np.array([x, y, z, w])
    if w < 0:
        v = -v
    x, y, z, w = v / np.linalg.norm(v)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def se3_exp_g2o(u):
    """R, V of g2o's SE3Quat::exp (its small-angle branch is R = V = I + O + O^2 below 1e-5)."""
    w = np.asarray(u[:3], np.float64)
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O @ O
    if th < 0.00001:
        R = np.eye(3) + O + O2
        return R, R.copy()
    a, b, c = math.sin(th) / th, (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    return np.eye(3) + a * O + b * O2, np.eye(3) + b * O + c * O2


def skew(v):
    """(m, 3) -> (m, 3, 3) cross-product matrices."""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def edge_errors(R, t, X, kf, lm, obs, stereo, cam=Cam):
    """Errors obs - project(T X) (m, 3; third row 0 for mono edges) and camera-frame points."""
    Xc = np.einsum("mij,mj->mi", R[kf], X[lm]) + t[kf]
    iz = 1.0 / Xc[:, 2]
    pu = cam.fx * Xc[:, 0] * iz + cam.cx
    pv = cam.fy * Xc[:, 1] * iz + cam.cy
    e = np.stack([obs[:, 0] - pu, obs[:, 1] - pv, np.where(stereo, obs[:, 2] - (pu - cam.bf * iz), 0.0)], 1)
    return e, Xc


def edge_jacobians(R, Xc, kf, stereo, cam=Cam):
    """d error / d (omega, upsilon) of the pose (update exp(dx) T) and d error / d X."""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    iz = 1.0 / z
    iz2 = iz * iz
    m = len(x)
    P = np.zeros((m, 3, 3))  # d proj / d Xc
    P[:, 0, 0] = cam.fx * iz
    P[:, 0, 2] = -cam.fx * x * iz2
    P[:, 1, 1] = cam.fy * iz
    P[:, 1, 2] = -cam.fy * y * iz2
    P[:, 2, 0] = P[:, 0, 0]
    P[:, 2, 2] = P[:, 0, 2] + cam.bf * iz2
    P[~stereo, 2, :] = 0.0
    dX = np.concatenate([-skew(Xc), np.broadcast_to(np.eye(3), (m, 3, 3))], 2)  # d Xc / d (omega, upsilon)
    return -P @ dX, -P @ R[kf]


def huber(c2, delta):
    d2 = delta * delta
    big = c2 > d2
    sq = np.sqrt(np.where(big, c2, 1.0))
    return np.where(big, 2 * sq * delta - d2, c2), np.where(big, delta / sq, 1.0)


def ldlt_nopivot(A, b):
    """LDL^T without pivoting; (x, ok) with ok False iff a pivot is exactly zero."""
    n = len(b)
    if n == 0:
        return np.zeros(0), True
    L = np.array(A, np.float64)
    d = np.zeros(n)
    for k in range(n):
        d[k] = L[k, k]
        if d[k] == 0:
            return np.zeros(n), False
        c = L[k + 1:, k].copy()
        L[k + 1:, k] = c / d[k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], c)
    L = np.tril(L, -1) + np.eye(n)
    y = np.array(b, np.float64)
    for k in range(n):
        y[k + 1:] -= L[k + 1:, k] * y[k]
    y /= d
    for k in range(n - 1, -1, -1):
        y[:k] -= L[k, :k] * y[k]
    return y, True


# --------------------------------------------------------------------- system
class System:
    """The linearised joint system of one iteration over the active edges `act`
    (edge indices in accumulation order), active poses and landmarks compacted."""

    def __init__(self, R, t, X, E, act, robust, prm, cam):
        kf, lm = E["kf"][act], E["lm"][act]
        st = E["stereo"][act]
        e, Xc = edge_errors(R, t, X, kf, lm, E["obs"][act], st, cam)
        info = E["info"][lm]
        c2 = info * (e * e).sum(1)
        rho1 = huber(c2, np.where(st, prm["huber_stereo"], prm["huber_mono"]))[1] if robust else np.ones(len(act))
        Jp, Jl = edge_jacobians(R, Xc, kf, st, cam)
        w = rho1 * info
        self.lms = np.unique(lm)
        self.kfs = np.unique(kf[E["free"][kf]])
        lpos = np.full(len(X), -1)
        lpos[self.lms] = np.arange(len(self.lms))
        ppos = np.full(len(R), -1)
        ppos[self.kfs] = np.arange(len(self.kfs))
        self.li, self.pi = lpos[lm], ppos[kf]
        nl, nf = len(self.lms), len(self.kfs)
        self.Hll = np.zeros((nl, 3, 3))
        self.bl = np.zeros((nl, 3))
        np.add.at(self.Hll, self.li, np.einsum("mki,m,mkj->mij", Jl, w, Jl))
        np.add.at(self.bl, self.li, -np.einsum("mki,m,mk->mi", Jl, w, e))
        fr = self.pi >= 0
        self.fr = fr
        self.Hpp = np.zeros((nf, 6, 6))
        self.bp = np.zeros((nf, 6))
        np.add.at(self.Hpp, self.pi[fr], np.einsum("mki,m,mkj->mij", Jp[fr], w[fr], Jp[fr]))
        np.add.at(self.bp, self.pi[fr], -np.einsum("mki,m,mk->mi", Jp[fr], w[fr], e[fr]))
        self.W = np.einsum("mki,m,mkj->mij", Jp[fr], w[fr], Jl[fr])  # (free edges, 6, 3)

    def max_diag(self):
        d = [0.0]
        if len(self.Hpp):
            d.append(np.abs(np.einsum("nii->ni", self.Hpp)).max())
        if len(self.Hll):
            d.append(np.abs(np.einsum("nii->ni", self.Hll)).max())
        return max(d)

    def dense(self, lam):
        """The joint matrix and right-hand side, poses first."""
        nf, nl = len(self.kfs), len(self.lms)
        n = 6 * nf + 3 * nl
        H = np.zeros((n, n))
        for i in range(nf):
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = self.Hpp[i]
        for j in range(nl):
            o = 6 * nf + 3 * j
            H[o:o + 3, o:o + 3] = self.Hll[j]
        for W, i, j in zip(self.W, self.pi[self.fr], self.li[self.fr]):
            o = 6 * nf + 3 * j
            H[6 * i:6 * i + 6, o:o + 3] += W
            H[o:o + 3, 6 * i:6 * i + 6] += W.T
        H[np.arange(n), np.arange(n)] += lam
        return H, np.concatenate([self.bp.ravel(), self.bl.ravel()])

    def solve(self, lam, solver="ldlt"):
        """BlockSolver_6_3 with the points marginalised: (dx (nf, 6), dl (nl, 3), ok)."""
        nf, nl = len(self.kfs), len(self.lms)
        Hl = self.Hll + lam * np.eye(3)
        # Eigen's 3x3 inverse: cofactors over the determinant
        c = np.stack([np.cross(Hl[:, 1], Hl[:, 2]), np.cross(Hl[:, 2], Hl[:, 0]), np.cross(Hl[:, 0], Hl[:, 1])], 2)
        det = np.einsum("ni,ni->n", Hl[:, 0], c[:, :, 0])
        with np.errstate(all="ignore"):
            Hinv = c / det[:, None, None]
        pi, li = self.pi[self.fr], self.li[self.fr]
        S = np.zeros((nf, nf, 6, 6))
        S[np.arange(nf), np.arange(nf)] = self.Hpp + lam * np.eye(6)
        r = self.bp.copy()
        Y = np.einsum("mij,mjk->mik", self.W, Hinv[li])  # W Hll^-1 per free edge
        np.add.at(r, pi, -np.einsum("mik,mk->mi", Y, self.bl[li]))
        # every pair (a-th, b-th) of free edges of one landmark
        o = np.argsort(li, kind="stable")
        cnt = np.bincount(li, minlength=nl)
        start = np.concatenate([[0], np.cumsum(cnt)])
        K = int(cnt.max()) if len(cnt) else 0
        for a in range(K):
            for bb in range(K):
                sel = np.nonzero(cnt > max(a, bb))[0]
                ea, eb = o[start[sel] + a], o[start[sel] + bb]
                np.add.at(S, (pi[ea], pi[eb]), -np.einsum("mik,mjk->mij", Y[ea], self.W[eb]))
        S = S.transpose(0, 2, 1, 3).reshape(6 * nf, 6 * nf)
        ok = True
        with np.errstate(all="ignore"):
            if nf == 0:
                dx = np.zeros(0)
            elif solver == "ldlt":
                dx, ok = ldlt_nopivot(S, r.ravel())
            else:
                try:
                    dx = np.linalg.solve(S, r.ravel())
                except np.linalg.LinAlgError:
                    dx, ok = np.zeros(6 * nf), False
            dx = dx.reshape(nf, 6)
            rl = self.bl.copy()
            np.add.at(rl, li, -np.einsum("mik,mi->mk", self.W, dx[pi]))
            dl = np.einsum("nij,nj->ni", Hinv, rl)
        if not ok:
            dx, dl = np.zeros((nf, 6)), np.zeros((nl, 3))  # a failed solve leaves the step zero
        return dx, dl, ok


def _prepare(Tcw, fixed, Xw, edges):
    Tcw = np.asarray(Tcw, np.float32).reshape(-1, 4, 4)
    Xw32 = np.asarray(Xw, np.float32).reshape(-1, 3)
    R = np.stack([quat_roundtrip(T[:3, :3].astype(np.float64)) for T in Tcw]) if len(Tcw) else np.zeros((0, 3, 3))
    t = Tcw[:, :3, 3].astype(np.float64)
    z = Xw32[:, 2]
    with np.errstate(all="ignore"):
        info = (np.float32(1.0) / (z * z)).astype(np.float64)
    ur = edges["ur"].astype(np.float64)
    E = dict(kf=edges["kf"].astype(np.int64), lm=edges["lm"].astype(np.int64),
             obs=np.stack([edges["u"].astype(np.float64), edges["v"].astype(np.float64), ur], 1),
             stereo=~(edges["ur"] < 0), info=info, free=~np.asarray(fixed, bool))
    return Tcw, Xw32, R, t, Xw32.astype(np.float64), E


def local_ba_ref(Tcw, fixed, Xw, edges, params=None, order=None, solver="ldlt", cam=Cam):
    """odo_local_ba in float64. Returns a dict: Tcw, Xw (float32 outputs), Tcw64 /
    Xw64 (before the cast), erase, level1 (bool per edge), chi2 (the stored
    per-edge chi2 the flags were taken from; chi2_stage1_edges: the one the
    level-1 marks were taken from), iters / trials (per stage),
    trials_per_iter (a list per stage), chi2_initial / chi2_stage1 / chi2_final,
    Xw64_stage1 (the points after stage 1), status (0 ran, 1 nothing to do),
    min_decision (the smallest |chi2 - trial chi2| / chi2 any accept / reject
    decision rested on: near 1e-16 the decision was made by rounding)."""
    prm = params or default_params()
    Tcw, Xw32, R, t, X, E = _prepare(Tcw, fixed, Xw, edges)
    ne = len(edges)
    order = np.arange(ne) if order is None else np.asarray(order)
    stereo = E["stereo"]
    th = np.where(stereo, prm["chi2_stereo"], prm["chi2_mono"])
    out = dict(Tcw=Tcw.copy(), Xw=Xw32.copy(), erase=np.zeros(ne, np.uint8), level1=np.zeros(ne, bool),
               chi2=np.zeros(ne), chi2_stage1_edges=np.zeros(ne), iters=[0, 0], trials=[0, 0], trials_per_iter=[[], []], status=1,
               chi2_initial=0.0, chi2_stage1=0.0, chi2_final=0.0, min_decision=math.inf, Tcw64=None, Xw64=X.copy(), Xw64_stage1=X.copy())
    in_system = np.zeros(len(R), bool)
    if ne:
        in_system[np.unique(E["kf"])] = True
    in_system &= E["free"]
    if ne == 0:
        return out
    out["status"] = 0
    stored = np.zeros(ne)
    level1 = np.zeros(ne, bool)

    def chi_at(R_, t_, X_, act, robust):
        e, _ = edge_errors(R_, t_, X_, E["kf"][act], E["lm"][act], E["obs"][act], stereo[act], cam)
        c2 = E["info"][E["lm"][act]] * (e * e).sum(1)
        stored[act] = c2
        if robust:
            c2 = huber(c2, np.where(stereo[act], prm["huber_stereo"], prm["huber_mono"]))[0]
        return float(np.sum(c2))

    def optimize(R, t, X, act, iters, robust, stage):
        lam, ni = 0.0, 2.0
        with np.errstate(all="ignore"):
            cur = chi_at(R, t, X, act, robust)
        first = cur
        for it in range(iters):
            with np.errstate(all="ignore"):
                sysm = System(R, t, X, E, act, robust, prm, cam)
            if it == 0:
                lam, ni = 1e-5 * sysm.max_diag(), 2.0
            rho, q = 0.0, 0
            while True:
                dx, dl, ok = sysm.solve(lam, solver)
                R2, t2, X2 = R.copy(), t.copy(), X.copy()
                for i, k in enumerate(sysm.kfs):
                    Re, V = se3_exp_g2o(dx[i])
                    R2[k] = Re @ R[k]
                    t2[k] = Re @ t[k] + V @ dx[i, 3:]
                X2[sysm.lms] = X[sysm.lms] + dl
                with np.errstate(all="ignore"):
                    tmp = chi_at(R2, t2, X2, act, robust)
                    if not ok:
                        tmp = DBL_MAX
                    scale = float(np.sum(dx * (lam * dx + sysm.bp)) + np.sum(dl * (lam * dl + sysm.bl))) + 1e-3
                    rho = (cur - tmp) / scale
                if math.isfinite(tmp) and tmp != DBL_MAX:
                    out["min_decision"] = min(out["min_decision"], abs(cur - tmp) / max(cur, 1e-300))
                q += 1
                if rho > 0 and math.isfinite(tmp):
                    a = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, a)
                    ni = 2.0
                    cur = tmp
                    R, t, X = R2, t2, X2
                else:
                    lam *= ni
                    ni *= 2
                if not (rho < 0 and q < 10):
                    break
            out["iters"][stage] += 1
            out["trials"][stage] += q
            out["trials_per_iter"][stage].append(q)
            if q == 10 or rho == 0:
                break
        return R, t, X, first, cur

    def depth_bad(R, t, X):
        z = np.einsum("mj,mj->m", R[E["kf"], 2, :], X[E["lm"]]) + t[E["kf"], 2]
        return ~(z > 0)

    R, t, X, c0, c1 = optimize(R, t, X, order, prm["iters_robust"], bool(prm["robust"]), 0)
    out["chi2_initial"], out["chi2_stage1"], out["chi2_final"] = c0, c1, c1
    out["Xw64_stage1"] = X.copy()
    out["chi2_stage1_edges"] = stored.copy()
    if prm["iters_final"] > 0:
        level1 = (stored > th) | depth_bad(R, t, X)
        act = order[~level1[order]]
        if len(act):
            R, t, X, _, c2 = optimize(R, t, X, act, prm["iters_final"], False, 1)
            out["chi2_final"] = c2
    out["level1"] = level1
    out["chi2"] = stored.copy()
    out["erase"] = ((stored > th) | depth_bad(R, t, X)).astype(np.uint8)
    T64 = Tcw.astype(np.float64)
    T64[:, :3, :3], T64[:, :3, 3] = R, t
    out["Tcw64"], out["Xw64"] = T64, X
    T32 = T64.astype(np.float32)
    T32[~in_system] = Tcw[~in_system]
    out["Tcw"], out["Xw"] = T32, X.astype(np.float32)
    return out


# ---------------------------------------------------------------------- cases
def project(T, X, cam=Cam):
    Xc = X @ T[:3, :3].T + T[:3, 3]
    iz = 1.0 / Xc[:, 2]
    u = cam.fx * Xc[:, 0] * iz + cam.cx
    return u, cam.fy * Xc[:, 1] * iz + cam.cy, u - cam.bf * iz, Xc[:, 2]


def exp4(u):
    R, V = se3_exp_g2o(u)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ np.asarray(u[3:], np.float64)
    return T


def chunk_size(n_lm):
    """Landmarks per partial reduced system (ba_nchunks, csrc/k_ba.hip): BA_CHUNK,
    or ceil(n_lm / BA_MAX_CHUNKS) once BA_CHUNK would give more than BA_MAX_CHUNKS chunks."""
    return BA_CHUNK if -(-n_lm // BA_CHUNK) <= BA_MAX_CHUNKS else -(-n_lm // BA_MAX_CHUNKS)


def observed_landmarks(n_lm, count):
    """`count` landmark indices spread evenly over [0, n_lm), plus the first and
    last landmark and both sides of the chunk boundaries 1, 2, 33 and the last."""
    ch = chunk_size(n_lm)
    nch = -(-n_lm // ch)
    edge = [c * ch + d for c in (1, 2, 33, nch - 1) for d in (-1, 0) if 0 < c * ch < n_lm]
    return np.unique(np.r_[np.linspace(0, n_lm - 1, count).astype(np.int64), 0, n_lm - 1, edge].astype(np.int64))


def make_scene(seed, n_free, n_fixed, n_lm, obs="random", kinds="mixed", noise=0.5, outliers=0.10,
               pose_off=(1.0, 0.03), pt_off=0.02, mean_obs=4, first_free=False, exact_obs=False, observed=None, **params):
    """One synthetic problem: keyframes within a few degrees / decimetres of the
    origin looking down +z, landmarks 2 to 4 m in front of them (inside the image, right coordinate positive). obs: "random"
    (about mean_obs keyframes per landmark, at least 2), "once", "all",
    "fixed_only". pose_off = (degrees, metres) of the free poses' start.
    The true pose of a keyframe is what the solver makes of its float32
    matrix (quat_roundtrip), so a fixed keyframe sits exactly at its truth;
    exact_obs keeps the observations in float64 (a float64 edge table, for
    the reference only). observed: only about that many of the landmarks carry
    edges (observed_landmarks), the rest are valid landmarks without one."""
    rng = np.random.default_rng([int(x) for x in np.atleast_1d(seed)] + [n_free, n_fixed, n_lm, 0xBA])
    nk = n_free + n_fixed
    fixed = np.zeros(nk, np.uint8)
    fixed[rng.permutation(nk)[:n_fixed]] = 1
    if first_free and nk:
        fixed[:] = np.r_[np.zeros(n_free), np.ones(n_fixed)]
    T32 = np.stack([exp4(np.r_[unit(rng) * math.radians(rng.uniform(0, 4)), rng.uniform(-0.3, 0.3, 3) * [1, 1, 0.3]])
                    for _ in range(nk)]).astype(np.float32) if nk else np.zeros((0, 4, 4), np.float32)
    Ttrue = T32.astype(np.float64)
    for k in range(nk):
        Ttrue[k, :3, :3] = quat_roundtrip(Ttrue[k, :3, :3])
    Xtrue = (rng.random((n_lm, 3)) * [1.2, 1.0, 2] + [-0.6, -0.5, 2.0]).astype(np.float32).astype(np.float64)
    if obs == "once":
        pairs = [(int(rng.integers(nk)), l) for l in range(n_lm)]
    elif obs == "all":
        pairs = [(k, l) for l in range(n_lm) for k in range(nk)]
    else:
        pool = np.nonzero(fixed)[0] if obs == "fixed_only" else np.arange(nk)
        pairs = []
        for l in (range(n_lm) if observed is None else observed_landmarks(n_lm, observed)):
            m = min(len(pool), max(2, int(rng.poisson(mean_obs))))
            pairs += [(int(k), l) for k in sorted(rng.choice(pool, m, replace=False))]
    pairs = np.array(pairs, np.int64).reshape(-1, 2)
    pairs = pairs[rng.permutation(len(pairs))]  # edges in no particular order
    ne = len(pairs)
    E = np.zeros(ne, BA_EDGE_DTYPE64 if exact_obs else BA_EDGE_DTYPE)
    E["kf"], E["lm"] = pairs[:, 0], pairs[:, 1]
    stereo = {"stereo": np.ones(ne, bool), "mono": np.zeros(ne, bool)}.get(kinds)
    if stereo is None:
        stereo = rng.random(ne) < 0.5
    u, v, ur = np.zeros(ne), np.zeros(ne), np.zeros(ne)
    for k in range(nk):
        s = pairs[:, 0] == k
        u[s], v[s], ur[s], _ = project(Ttrue[k], Xtrue[pairs[s, 1]])
    u += rng.normal(size=ne) * noise
    v += rng.normal(size=ne) * noise
    ur += rng.normal(size=ne) * noise
    g = rng.random(ne) < outliers
    u[g] += rng.choice([-1.0, 1.0], int(g.sum())) * rng.uniform(15, 60, int(g.sum()))
    v[g] += rng.choice([-1.0, 1.0], int(g.sum())) * rng.uniform(15, 60, int(g.sum()))
    assert (ur[stereo] > 1.0).all()  # a negative right coordinate would read as a monocular edge
    E["u"], E["v"], E["ur"] = u, v, np.where(stereo, ur, -1.0)
    Tinit = T32.astype(np.float64)
    for k in range(nk):
        if not fixed[k]:
            Tinit[k] = exp4(np.r_[unit(rng) * math.radians(pose_off[0]), unit(rng) * pose_off[1]]) @ Ttrue[k]
    Xinit = Xtrue + rng.normal(size=Xtrue.shape) * pt_off
    return dict(Tcw=np.ascontiguousarray(Tinit.astype(np.float32)), fixed=fixed,
                Xw=np.ascontiguousarray(Xinit.astype(np.float32)), edges=E, params=default_params(**params),
                Ttrue=Ttrue, Xtrue=Xtrue)


# Widths the kernels use (csrc/k_ba.hip): landmarks are chunked by BA_CHUNK = 128
# for the per-chunk partial reduced systems, at most BA_MAX_CHUNKS = 64 of them
# (above 64 * 128 = 8192 landmarks a chunk holds ceil(n / 64)), per-edge and
# per-landmark kernels run 256 threads per workgroup, and the unblocked LDL^T
# walks the 6 * n_free rows with a 32 x 32 thread tile.
BA_CHUNK, BA_BLOCK, BA_TILE, BA_MAX_CHUNKS = 128, 256, 32, 64

# name -> make_scene arguments; SEEDS holds the seeds that are not 0. A seed was
# replaced (tests/test_ba_ref64.py::test_cases_stable holds the rule)
# where the reference alone -- natural order / LDL^T against reversed order /
# numpy.linalg.solve -- changed a flag or a trial count, or where one of its
# accept / reject decisions rested on a chi2 difference below MIN_DECISION of
# the chi2: there the last bits of a sum decide, and no summation order can be
# asked to reproduce the trial count. Cases that converge within a few
# iterations (only points move) run a shorter stage 2 for the same reason.
MIN_DECISION = 1e-9
_S = {}


def _add(name, *a, **kw):
    _S[name] = (a, kw)


for _nm, _a in (("s1_1_3", (1, 1, 3)), ("s2_1_16", (2, 1, 16)), ("s4_2_300", (4, 2, 300))):
    _add(_nm, *_a)
_add("s1_0_40_kf0_free", 1, 0, 40, kinds="stereo")
for _n in (63, 64, 65, 255, 256, 257, BA_CHUNK - 1, BA_CHUNK, BA_CHUNK + 1):
    _add(f"lm{_n}", 3, 2, _n, mean_obs=3)
for _n in (11, 32, 63, 64):
    _add(f"free{_n}", _n, 2, 96, mean_obs=6)
# 6 * n_free around the factorisation's 32-wide thread tile: 5 -> 30, 6 -> 36; 16 free -> 96 = 3 tiles
for _n in (5, 6, 16):
    _add(f"free{_n}", _n, 2, 96, mean_obs=4)
_add("once", 3, 2, 200, obs="once")
_add("all", 4, 3, 120, obs="all", iters_final=5)
_add("fixed_only", 2, 3, 150, obs="fixed_only", iters_final=4)
_add("all_fixed", 0, 4, 150, iters_final=4)
_add("stereo", 3, 2, 200, kinds="stereo")
_add("mono", 3, 2, 200, kinds="mono")
_add("outliers30", 4, 2, 300, outliers=0.30)
_add("global_robust", 3, 2, 200, iters_robust=10, iters_final=0, robust=1,
     huber_mono=float(np.float32(math.sqrt(5.99))))
_add("global_plain", 3, 2, 200, iters_robust=10, iters_final=0, robust=0)
_add("one_iter", 3, 2, 200, iters_robust=1)
_add("edges_gt_block", 4, 2, BA_BLOCK + 1, mean_obs=5)
_add("free_kf_no_edge", 3, 2, 120)
_add("lm_no_edge", 3, 2, 120)
_add("lm_all_level1", 3, 2, 120)
_add("behind", 3, 2, 120)
_add("rejected", 3, 2, 120, pose_off=(math.degrees(0.6), 1.0))
# (added after the cases above: a case's place in this list seeds its scene)
_add("ends_behind", 3, 2, 120, outliers=0.0)
# the 64-chunk limit: 8191 and 8192 landmarks are 64 chunks of 128, 8193 are 64 of 129,
# 20000 are 64 of 313; a few hundred of the landmarks carry edges, in every part of the range
for _n in (BA_MAX_CHUNKS * BA_CHUNK - 1, BA_MAX_CHUNKS * BA_CHUNK, BA_MAX_CHUNKS * BA_CHUNK + 1, 20000):
    _add(f"lm{_n}", 3, 2, _n, mean_obs=3, observed=300)
CASES = tuple(_S)
SEEDS = {'lm63': 2, 'lm64': 4, 'lm256': 1, 'lm127': 1, 'free11': 1, 'free32': 1, 'free5': 3, 'free6': 2, 'free16': 1,
         'free_kf_no_edge': 2, 'lm_all_level1': 1, 'behind': 1, 'rejected': 37, 'ends_behind': 1}


def build_case(name, seed):
    a, kw = _S[name]
    c = dict(make_scene([CASES.index(name), seed], *a, **kw))
    if name == "free_kf_no_edge":  # one more keyframe, free and unobserved
        T = np.concatenate([c["Tcw"], exp4(np.r_[0.1, -0.2, 0.05, 0.3, 0.1, -0.2]).astype(np.float32)[None]])
        c.update(Tcw=np.ascontiguousarray(T), fixed=np.r_[c["fixed"], 0].astype(np.uint8))
    elif name == "lm_no_edge":  # landmarks 0 and the last one have no edge
        E = c["edges"]
        c.update(edges=np.ascontiguousarray(E[(E["lm"] != 0) & (E["lm"] != 119)]))
    elif name == "lm_all_level1":  # every observation of landmark 5 is a gross outlier
        E = c["edges"].copy()
        s = E["lm"] == 5
        sg = np.where(np.arange(int(s.sum())) % 2, 1.0, -1.0)
        E["u"][s] += 40.0 * sg
        E["v"][s] -= 35.0 * sg
        c.update(edges=E)
    elif name == "ends_behind":
        # Landmark 7 starts in front of every camera and ends behind one: free
        # keyframe k truly stands 1 m further along z than the others, with the
        # landmark 0.3 m behind it, but starts 1 m back, where the landmark
        # is 0.7 m ahead. Its other edges pull k forward past the landmark.
        rng = np.random.default_rng([CASES.index(name), seed, 7])
        k = int(np.nonzero(c["fixed"] == 0)[0][0])
        Tt, Xt, E = c["Ttrue"].copy(), c["Xtrue"].copy(), c["edges"].copy()
        back = Tt[k].copy()
        Tt[k, 2, 3] -= 1.0
        Xt[7] = np.float32([0.1, 0.05, 0.7])
        E = E[(E["lm"] != 7) | (E["kf"] != k)]
        add = np.zeros(1, BA_EDGE_DTYPE)
        add["kf"], add["lm"], add["ur"] = k, 7, -1.0
        E = np.concatenate([E, add])
        for e in np.nonzero((E["kf"] == k) | (E["lm"] == 7))[0]:
            u, v, ur, _ = project(Tt[E["kf"][e]], Xt[E["lm"][e]][None])
            n3 = rng.normal(size=3) * 0.5
            E["u"][e], E["v"][e] = u[0] + n3[0], v[0] + n3[1]
            E["ur"][e] = ur[0] + n3[2] if (E["ur"][e] >= 0 and ur[0] > 1.0) else -1.0
        T0, X0 = c["Tcw"].copy(), c["Xw"].copy()
        T0[k] = back.astype(np.float32)
        X0[7] = (Xt[7] + rng.normal(size=3) * 0.01).astype(np.float32)
        c.update(Tcw=T0, Xw=X0, edges=np.ascontiguousarray(E), Ttrue=Tt, Xtrue=Xt, kf_moved=k)
    elif name == "behind":  # landmark 3 starts behind every camera
        X = c["Xw"].copy()
        X[3, 2] = -1.5
        c.update(Xw=X)
    return c


@functools.lru_cache(maxsize=None)
def ba_case(name):
    """dict(Tcw, fixed, Xw, edges, params, ...) of one case; deterministic per name."""
    c = build_case(name, SEEDS.get(name, 0))
    if name == "rejected":  # free poses start 0.6 rad and 1 m off: some trials are rejected
        r = local_ba_ref(c["Tcw"], c["fixed"], c["Xw"], c["edges"], c["params"])
        assert max(r["trials_per_iter"][0] + r["trials_per_iter"][1]) > 1, "the case no longer rejects a trial"
    return c


@functools.lru_cache(maxsize=None)
def ba_case_refs(name):
    """(natural order / LDL^T run, reversed order / numpy.linalg.solve run, d):
    d is the reference's own largest distance between the two on poses and
    points, what another summation order and factorisation cost."""
    c = ba_case(name)
    a = local_ba_ref(c["Tcw"], c["fixed"], c["Xw"], c["edges"], c["params"])
    b = local_ba_ref(c["Tcw"], c["fixed"], c["Xw"], c["edges"], c["params"],
                     order=np.arange(len(c["edges"]))[::-1], solver="solve")
    d = max(float(np.abs(a["Tcw64"] - b["Tcw64"]).max()) if len(c["Tcw"]) else 0.0,
            float(np.abs(a["Xw64"] - b["Xw64"]).max()) if len(c["Xw"]) else 0.0)
    return a, b, d


def near_threshold(ref, edges, params, margin=0.02, key="chi2"):
    th = np.where(edges["ur"] < 0, params["chi2_mono"], params["chi2_stereo"])
    return np.abs(ref[key] - th) <= margin * th


def flags_agree(got_erase, got_level1_count, ref, edges, params, tag=""):
    """The PnP tests' rule: flags equal except on edges whose reference chi2 is
    within 2 % of its threshold, and at most 1 % of the edges."""
    diff = np.asarray(got_erase, np.uint8) != ref["erase"]
    near = near_threshold(ref, edges, params)
    assert not (diff & ~near).any(), f"{tag}: erase flags differ away from the threshold at {np.nonzero(diff & ~near)[0][:8]}"
    cap = 0.01 * len(edges)
    assert diff.sum() <= cap, f"{tag}: {int(diff.sum())} erase flags differ (cap {cap:.1f})"
    dl = abs(int(got_level1_count) - int(ref["level1"].sum()))
    near1 = near_threshold(ref, edges, params, key="chi2_stage1_edges")
    assert dl <= min(int(near1.sum()), int(cap)), f"{tag}: level-1 count {got_level1_count} vs {int(ref['level1'].sum())}"
