"""Float64 reference and case builders for GICP -- TEST INFRASTRUCTURE.

Independent of the oracle (oracle/gicp_ref.cpp restates PCL's code path, the
insertion into a sorted top 20 included): numpy only, from the definitions.

* Neighbours: the float32 squared distances of the kernel (dx*dx, + dy*dy,
  + dz*dz, every step rounded to float32, which numpy's float32 arithmetic
  does), then the first 20 of a STABLE sort: equal distances keep index order,
  which is the "ties to the lower index" rule without any insertion code.
* Covariance: two-pass mean and covariance of those 20 points in float64,
  numpy.linalg.eigh, and with v the eigenvector of the smallest eigenvalue
  C = I - (1 - 1e-3) v v^T (eigenvalues (1, 1, 1e-3) on the eigenvectors; the
  two unit eigenvalues make the choice within their plane irrelevant). The
  relative eigen-gap (w1 - w0) / w2 says how well v is determined.
* First ICP iteration under the identity guess: per source point the float32
  argmin over the target (first minimum), a correspondence iff
  float64(d) < max_corr_dist^2.

tests/test_gicp_ref64.py checks the oracle against this on the CPU,
tests/test_gicp_edges_gpu.py the HIP kernels against both.
"""
from __future__ import annotations

import numpy as np

K = 20
EPS = 1e-3
GAP_MIN = 1e-2
F32_EPS = float(np.finfo(np.float32).eps)
SHIFT = np.float32([0.01, -0.005, 0.008])
SCENE_SIZES = (20, 21, 63, 64, 65, 300, 4096, 4097)


# ------------------------------------------------------------------ reference
def dist2_f32(q, P):
    """The kernel's dist2f of point q against every row of P, in float32."""
    q = np.asarray(q, np.float32)
    P = np.asarray(P, np.float32)
    d = q[0] - P[:, 0]
    r = d * d
    d = q[1] - P[:, 1]
    r = r + d * d
    d = q[2] - P[:, 2]
    r = r + d * d
    assert r.dtype == np.float32
    return r


def knn20_full(P):
    """n x 20 neighbour indices: the first 20 of a stable argsort, row by row."""
    P = np.asarray(P, np.float32)
    return np.stack([np.argsort(dist2_f32(p, P), kind="stable")[:K] for p in P])


def knn20(P):
    """knn20_full with a pre-filter: the first 20 of a stable sort all lie at or
    below the 20th smallest distance, so only those candidates are sorted (the
    4097-point clouds; tested equal to knn20_full)."""
    P = np.asarray(P, np.float32)
    out = np.empty((len(P), K), np.int64)
    for q, p in enumerate(P):
        d = dist2_f32(p, P)
        cand = np.flatnonzero(d <= np.partition(d, K - 1)[K - 1])  # ascending index
        out[q] = cand[np.argsort(d[cand], kind="stable")[:K]]
    return out


def covariances(P, nn=None):
    """(C n x 3 x 3, gap n, magnitude n, w2 n) in float64 for a cloud of >= 20
    points; gap = 0 where the largest eigenvalue is 0."""
    P = np.asarray(P, np.float32)
    assert len(P) >= K
    nn = knn20(P) if nn is None else nn
    X = P.astype(np.float64)[nn]                       # n x 20 x 3
    D = X - X.mean(axis=1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", D, D) / K
    w, V = np.linalg.eigh(cov)                         # ascending
    v = V[:, :, 0]
    C = np.eye(3)[None] - (1.0 - EPS) * v[:, :, None] * v[:, None, :]
    w2 = w[:, 2]
    gap = np.where(w2 > 0, (w[:, 1] - w[:, 0]) / np.where(w2 > 0, w2, 1.0), 0.0)
    return C, gap, np.abs(X).max(axis=(1, 2)), w2


def oracle_bound(gap, magnitude, w2):
    """Bound on |C_oracle - C_ref64| per point (max over the 9 entries).

    The oracle accumulates sum(x_a * x_b) / 20 - mean_a * mean_b in double, but
    every product x_a * x_b is a FLOAT product: relative error at most
    u = eps_f32 / 2, absolute at most u * m^2 with m the largest coordinate
    magnitude of the neighbourhood. The average of 20 such terms errs by at
    most u * m^2 per entry (the double operations add ~1e-16 m^2, nothing at
    this scale), so the symmetric perturbation E has ||E||_2 <= ||E||_F
    <= 3 u m^2 = 1.5 eps_f32 m^2. By the sin-theta theorem the eigenvector of
    the smallest eigenvalue turns by sin(theta) <= ||E||_2 / (delta - ||E||_2)
    with delta = w1 - w0 = gap * w2, which is <= 2 ||E||_2 / delta while
    ||E||_2 <= delta / 2 (beyond that the bound below exceeds 1, which no
    difference of two such matrices reaches). |C - C'| = (1 - 1e-3) |v v^T -
    v' v'^T| has 2-norm (1 - 1e-3) sin(theta), an upper bound of every entry:
        |dC| <= 2 * 1.5 * eps_f32 * m^2 / (gap * w2)        => c = 3
    plus 4 float32 ulps of 1 (C's scale) for the Jacobi SVD and the rest."""
    return 3.0 * F32_EPS * magnitude ** 2 / (gap * w2) + 4.0 * F32_EPS


def first_corr(src, tgt, max_corr_dist, last=False):
    """First-iteration correspondences under the identity guess: (source
    indices, target indices). last=True breaks equal distances to the HIGHER
    index (the rule the kernel must not have)."""
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32)
    thr = float(max_corr_dist) * float(max_corr_dist)
    si, ti = [], []
    for i, p in enumerate(src):
        d = dist2_f32(p, tgt)
        j = len(d) - 1 - int(np.argmin(d[::-1])) if last else int(np.argmin(d))
        if float(d[j]) < thr:
            si.append(i)
            ti.append(j)
    return np.asarray(si, np.int64), np.asarray(ti, np.int64)


def tied_sources(src, tgt):
    """Source points whose float32 minimum over the target is reached twice."""
    return np.asarray([i for i, p in enumerate(np.asarray(src, np.float32))
                       if (lambda d: np.count_nonzero(d == d.min()) > 1)(dist2_f32(p, tgt))], np.int64)


class FirstIterationCost:
    """GICP's first-iteration cost under the identity guess, in float64:
    f(x) = (1 / m) sum r^T (Cs_i + Ct_j)^-1 r over the m correspondences,
    r = R(x) s_i + t - t_j, x = (t, Euler angles about X, Y, Z composed as
    applyState does, Rz Ry Rx). BFGS stops where |grad f| < 1e-2."""

    def __init__(self, src, tgt, si, ti, Cs, Ct):
        self.S = np.asarray(src, np.float64)[si]
        self.Q = np.asarray(tgt, np.float64)[ti]
        self.M = np.linalg.inv(Cs[si] + Ct[ti])

    @staticmethod
    def pose(x):
        from scipy.spatial.transform import Rotation
        T = np.eye(4)
        T[:3, :3] = Rotation.from_euler("xyz", x[3:]).as_matrix()   # extrinsic x, y, z = Rz Ry Rx
        T[:3, 3] = x[:3]
        return T

    @staticmethod
    def state(T):
        from scipy.spatial.transform import Rotation
        T = np.asarray(T, np.float64)
        return np.r_[T[:3, 3], Rotation.from_matrix(T[:3, :3]).as_euler("xyz")]

    def __call__(self, x):
        T = self.pose(x)
        r = self.S @ T[:3, :3].T + T[:3, 3] - self.Q
        return np.einsum("na,nab,nb->", r, self.M, r) / len(self.S)

    def grad_norm(self, T, h=1e-6):
        x = self.state(T)
        e = np.eye(6) * h
        return float(np.linalg.norm([(self(x + e[k]) - self(x - e[k])) / (2 * h) for k in range(6)]))

    def optimum(self):
        from scipy.optimize import minimize
        return self.pose(minimize(self, np.zeros(6), method="BFGS", options=dict(gtol=1e-12)).x)


# ------------------------------------------------------------------ cases
_SCENE_SEED = 11
_SCENE = None


def scene(n):
    """The first n points of the three-plane scene of tests/test_gicp.py (4097
    points, noise 2 mm) under a fixed permutation, so that every prefix covers
    the three planes."""
    global _SCENE
    if _SCENE is None:
        from test_gicp import _scene
        P, _, _ = _scene(_SCENE_SEED, n=4097)
        _SCENE = np.ascontiguousarray(P[np.random.default_rng(_SCENE_SEED).permutation(len(P))])
        _SCENE.setflags(write=False)
    return _SCENE[:n]


def shifted(P):
    return (np.asarray(P, np.float32) + SHIFT).astype(np.float32)


def lattice(nx=6, ny=6, nz=2, h=0.25, origin=(0.0, 0.0, 2.0)):
    """nx x ny x nz points at spacing h (0.25: every coordinate, difference and
    squared distance is exact in float32), x fastest."""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (np.c_[x.ravel(), y.ravel(), z.ravel()] * h + np.asarray(origin)).astype(np.float32)


def lattice_perm(n=72):
    return np.random.default_rng(5).permutation(n)


def coincident(n=25):
    return np.tile(np.float32([0.5, -0.25, 2.0]), (n, 1))


def collinear_axis(n=25):
    """Along x at y = 0.5, z = 2: every float product is exact, the covariance is
    exactly diag(s, 0, 0)."""
    return np.c_[0.25 * np.arange(n), np.full(n, 0.5), np.full(n, 2.0)].astype(np.float32)


def collinear_diag(n=25):
    """Along (1, 1, 0): a rank-1 covariance that needs one Jacobi rotation."""
    return np.c_[0.25 * np.arange(n), 0.25 * np.arange(n), np.full(n, 2.0)].astype(np.float32)


def near_far_pair(k):
    """Source: the 6 x 6 x 2 lattice. Target: the same cloud 10 m away, except
    for k points (spread over the lattice, not coplanar) 0.01 m above their
    source points: exactly k correspondences at max_corr_dist 0.07."""
    S = lattice()
    T = S + np.float32([10.0, 0.0, 0.0])
    for j in [0, 5, 30, 71, 40, 14][:k]:
        T[j] = S[j] + np.float32([0.0, 0.0, 0.01])
    return S, T.astype(np.float32)


def threshold_pair():
    """27 source points at spacing 1 and max_corr_dist 0.25: the even target
    points sit at exactly 0.25 along x from their source points (float d^2 ==
    0.0625 == the threshold: no correspondence, the test is strict), the odd
    ones at the float below 0.25 (d^2 < 0.0625). Returns (src, tgt, dist,
    indices of the odd points)."""
    S = lattice(3, 3, 3, 1.0, (0.0, 0.0, 2.0))
    T = S.copy()
    T[:, 0] += np.float32(0.25)
    odd = np.arange(1, len(S), 2)
    T[odd, 0] = np.nextafter(T[odd, 0], np.float32(-np.inf))
    return S, T, 0.25, odd


def tie_pair():
    """Target: the 6 x 6 x 2 lattice. Source: 20 points 0.01 m above lattice
    points of the lower layer (unique nearest neighbours) and 5 points 0.01 m
    below midpoints of x-adjacent points on the lattice's boundary rows, whose two
    candidates are at equal float32 distance and have different covariances
    (one is a corner or next to one)."""
    T = lattice()
    up = np.float32([0.0, 0.0, 0.01])
    own = [7, 8, 9, 10, 13, 14, 15, 16, 19, 20, 21, 22, 25, 26, 27, 28, 1, 12, 23, 34]
    mids = [(0, 1), (4, 5), (30, 31), (34, 35), (6, 7)]
    S = [T[j] + up for j in own] + [(T[a] + T[b]) * np.float32(0.5) - up for a, b in mids]
    return np.asarray(S, np.float32), T


def plane_lattice():
    """Noise-free three-plane lattice: three mutually orthogonal 6 x 6 grids at
    spacing 0.25, 1.5 m and more apart, so that every neighbourhood lies in one
    plane."""
    g = 0.25 * np.arange(6)
    a, b = [m.ravel() for m in np.meshgrid(g, g, indexing="ij")]
    A = np.c_[a, b, np.full(36, 4.0)]                 # z = 4
    B = np.c_[np.full(36, -2.0), a, 1.0 + b]          # x = -2
    Cc = np.c_[2.0 + a, np.full(36, 3.0), 1.0 + b]    # y = 3
    return np.r_[A, B, Cc].astype(np.float32)


def known_motion():
    """(src, tgt, T_true): the plane lattice under a small rigid motion (every
    point moves less than the 0.07 m correspondence distance)."""
    from scipy.spatial.transform import Rotation
    S = plane_lattice()
    R = Rotation.from_rotvec([0.004, -0.006, 0.005]).as_matrix()
    t = np.array([0.01, -0.005, 0.008])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return S, (S.astype(np.float64) @ R.T + t).astype(np.float32), T


def cov_cases():
    """name -> cloud, for the covariance tests (every cloud >= 20 points)."""
    L = lattice()
    c = {f"scene{n}": scene(n) for n in SCENE_SIZES}
    c.update(lattice=L, lattice_perm=np.ascontiguousarray(L[lattice_perm()]), planes=plane_lattice(),
             coincident=coincident(), collinear_axis=collinear_axis(), collinear_diag=collinear_diag())
    return c


EXACT_CASES = ("lattice", "lattice_perm", "planes")        # nothing may fall below the gap
DEGENERATE_CASES = ("coincident", "collinear_axis", "collinear_diag")  # everything does, by construction


# ------------------------------------------------------------------ shared, computed once
_CACHE = {}


def cached(key, make):
    """Results shared by the tests of a session; the arrays are read-only."""
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def case(name):
    return cached(("case", name), lambda: np.ascontiguousarray(cov_cases()[name]))


def ref_cov(name):
    """(C, gap, magnitude, w2) of the reference on a covariance case."""
    return cached(("ref", name), lambda: covariances(case(name)))


def oracle_cov(name):
    import oracle_lib as O
    return cached(("oracle", name), lambda: O.gicp_covariances(case(name)))


COV_CASE_NAMES = tuple(f"scene{n}" for n in SCENE_SIZES) + EXACT_CASES + DEGENERATE_CASES
ICP_SIZES = ((20, 20), (20, 300), (300, 20), (21, 64), (255, 257), (256, 256), (257, 255), (4096, 4097), (4097, 64))


def icp_pair(ns, nt):
    """Source: the scene's first ns points; target: its first nt points, shifted."""
    return scene(ns), shifted(scene(nt))
