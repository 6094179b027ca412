"""References for the point-to-plane ICP (odo_icp_normals, odo_icp_plane_batch,
odo_icp_plane_dense): libicp's IcpPointToPlane, dimension 3 (the contract is in
include/odo.h; DESIGN §4 "Point-to-plane ICP").

  ref64   the algorithm in float64 numpy: exact rows from the unrounded R T + t,
          A^T A by a float64 product, numpy's solve. R, t stay float64.
  ref32   a transcription of libicp's float arithmetic in its own order: Matrix
          holds floats, so R, t, mu, Q, H, the rows, the RUNNING float sums of
          A^T A and A^T b over the active points, the Gauss-Jordan solve with full
          pivoting and the products R_ R, R_ t + t_ are float32, each operation
          rounded as the C++ rounds it.
Both share what the contract pins: the query is (float)(R T + t), the nearest
model point is the one of least float32 d2 = ((dx * dx + dy * dy) + dz * dz),
equal distances to the lower index, neighbours ascending by (d2, index), and
Matrix::svd's sign rule on a normal (negated when two or three components are
negative). Both take the eigenvector and the polar factor from numpy.linalg.

How far ref32 lies from ref64 on a case (e_ref) measures the reference's own
distance from exact arithmetic; the device, which sums A^T A in double in
another order, may differ from ref64 by 4 * max(e_ref over the stable cases,
1e-6) (tolerance()). A case is stable when the two references agree on the
iteration count and on every iteration's active set and correspondences.
"""
import numpy as np

f32, f64 = np.float32, np.float64
GATE_AS_WRITTEN, GATE_PLANE = 0, 1
OK, NO_MODEL, SHORT_TEMPLATE, SINGULAR = 0, 1, 2, 3
BRUTE_LIMIT = 1 << 20  # query x model pairs above which nearest() narrows the candidates with a k-d tree first


def d2_f32(q, P):
    """The float32 squared distance of the searches, q (3,) or (m, 1, 3) against P (n, 3)."""
    d = np.asarray(q, f32) - np.asarray(P, f32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(Q, M, brute=None):
    """Index of the nearest model point of every float32 query: least float32 d2,
    ties to the lower index. Brute force in chunks; for large products the 16
    nearest by float64 distance from a k-d tree are the candidates (the float32
    minimum lies among them unless more than 16 model points sit within float
    rounding of the same distance) and the same rule picks among them."""
    Q, M = np.ascontiguousarray(Q, f32), np.ascontiguousarray(M, f32)
    if brute is None:
        brute = len(Q) * len(M) <= BRUTE_LIMIT
    out = np.empty(len(Q), np.int64)
    if brute:
        step = max(1, (1 << 22) // max(len(M), 1))
        for a in range(0, len(Q), step):
            out[a:a + step] = np.argmin(d2_f32(Q[a:a + step, None, :], M[None]), axis=1)
        return out
    from scipy.spatial import cKDTree
    k = min(16, len(M))
    _, cand = cKDTree(M.astype(f64)).query(Q.astype(f64), k=k)
    cand = np.sort(cand.reshape(len(Q), k), axis=1)  # ascending index: argmin takes the lowest
    d = d2_f32(Q[:, None, :], M[cand])
    return cand[np.arange(len(Q)), np.argmin(d, axis=1)]


def knn(M, k):
    """n x min(k, n) neighbour indices, ascending by (d2, index), the point itself
    included. Clouds above 4096 points: the k + 16 nearest by float64 distance
    from a k-d tree are the candidates, ordered by the same rule (as nearest())."""
    M = np.asarray(M, f32)
    k = min(k, len(M))
    if len(M) <= 4096:
        return np.stack([np.argsort(d2_f32(p, M), kind="stable")[:k] for p in M])
    from scipy.spatial import cKDTree
    M64 = M.astype(f64)
    _, cand = cKDTree(M64).query(M64, k=min(k + 16, len(M)))
    d = d2_f32(M[:, None, :], M[cand])
    order = np.lexsort((cand, d), axis=1)[:, :k]
    return np.take_along_axis(cand, order, axis=1)


def sign_rule(n):
    """Matrix::svd's sign rule for the equal columns of U and V of a symmetric H."""
    return -n if np.count_nonzero(n < 0) >= 2 else n


def normals64(M, k):
    M64 = np.asarray(M, f32).astype(f64)
    P = M64[knn(M, k)]
    Q = P - P.mean(1, keepdims=True)
    _, V = np.linalg.eigh(np.einsum("nka,nkb->nab", Q, Q))
    n = V[:, :, 0]
    flip = np.count_nonzero(n < 0, axis=1) >= 2  # sign_rule, row by row
    return np.where(flip[:, None], -n, n)


def normals32(M, k):
    """computeNormal on Matrix's floats: running float sums in neighbour order."""
    M = np.asarray(M, f32)
    out = np.empty((len(M), 3), f32)
    for i, nn in enumerate(knn(M, k)):
        P = M[nn]
        mu = np.add.accumulate(P, axis=0, dtype=f32)[-1] / f32(len(nn))
        Q = P - mu
        H = np.empty((3, 3), f32)
        for a in range(3):
            for b in range(3):
                H[a, b] = np.add.accumulate(Q[:, a] * Q[:, b], dtype=f32)[-1]
        w, V = np.linalg.eigh(H.astype(f64))
        out[i] = sign_rule(V[:, 0].astype(f32))
    return out


def transform64(R, t, T):
    """R T + t in double in the written order, from whatever R, t hold."""
    R, t, T = np.asarray(R).astype(f64), np.asarray(t).astype(f64), np.asarray(T, f32).astype(f64)
    return np.stack([((R[i, 0] * T[:, 0] + R[i, 1] * T[:, 1]) + R[i, 2] * T[:, 2]) + t[i] for i in range(3)], 1)


def gate_mask(s, d, n, indist, gate):
    if gate == GATE_PLANE:
        return np.abs(((s[:, 0] - d[:, 0]) * n[:, 0] + (s[:, 1] - d[:, 1]) * n[:, 1]) + (s[:, 2] - d[:, 2]) * n[:, 2]) < indist
    return np.abs(((s[:, 0] - d[:, 0]) * n[:, 0] + (s[:, 1] - d[:, 1]) * n[:, 1]) + (s[:, 2] - d[:, 2])) * n[:, 2] < indist


def rows(s, d, n):
    """fitStep's [A | b] in double from the points s it is given."""
    sx, sy, sz = s.T
    dx, dy, dz = d.T
    nx, ny, nz = n.T
    A = np.stack([nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz], 1)
    b = ((((nx * dx + ny * dy) + nz * dz) - nx * sx) - ny * sy) - nz * sz
    return A, b


def polar(x):
    """U V^T of I + [x0 x1 x2]x by numpy's SVD, float64."""
    x = np.asarray(x, f64)
    K = np.array([[1, -x[2], x[1]], [x[2], 1, -x[0]], [-x[1], x[0], 1]], f64)
    U, _, Vt = np.linalg.svd(K)
    return U @ Vt


def solve32(A, b):
    """Matrix::solve (matrix.cpp:440-535) on float32 scalars; None when a pivot is below 1e-20."""
    A, b = np.array(A, f32), np.array(b, f32)
    m = len(b)
    ipiv = [0] * m
    for _ in range(m):
        big, irow, icol = f32(0), 0, 0
        for j in range(m):
            if ipiv[j] != 1:
                for k in range(m):
                    if ipiv[k] == 0 and abs(A[j, k]) >= big:
                        big, irow, icol = abs(A[j, k]), j, k
        ipiv[icol] += 1
        if irow != icol:
            A[[irow, icol]] = A[[icol, irow]]
            b[[irow, icol]] = b[[icol, irow]]
        if abs(A[icol, icol]) < f32(1e-20):
            return None
        pivinv = f32(1.0 / f64(A[icol, icol]))
        A[icol, icol] = f32(1)
        A[icol] = A[icol] * pivinv
        b[icol] = b[icol] * pivinv
        for ll in range(m):
            if ll != icol:
                dum = A[ll, icol]
                A[ll, icol] = f32(0)
                A[ll] = A[ll] - A[icol] * dum
                b[ll] = b[ll] - b[icol] * dum
    return b


def _dot3_32(a, b):
    s = f32(0)
    for k in range(3):
        s = f32(s + f32(a[k] * b[k]))
    return s


def _l2_32(v):
    s = f32(0)
    for x in np.asarray(v, f32).reshape(-1):
        s = f32(s + f32(x * x))
    return np.sqrt(s, dtype=f32)


def fit(T, M, guess=None, num_neighbors=10, max_iterations=200, min_delta=1e-4, indist=-1.0, gate=GATE_AS_WRITTEN,
        single=False):
    """IcpPointToPlane(M, num_neighbors).fit(T, R, t, indist): ref32 with
    single=True, else ref64. Returns a dict: T (4 x 4), iterations, n_active,
    residual, delta, status and trace, one (active mask, model index of every
    template point) per iteration."""
    T, M = np.ascontiguousarray(T, f32).reshape(-1, 3), np.ascontiguousarray(M, f32).reshape(-1, 3)
    ft = f32 if single else f64
    g = np.eye(4) if guess is None else np.asarray(guess, f32).astype(f64)
    R, t = g[:3, :3].astype(ft), g[:3, 3].astype(ft)
    out = dict(iterations=0, n_active=0, residual=0.0, delta=1000.0, status=OK, trace=[])

    def done():
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, t
        out["T"] = P
        return out

    if len(M) < 5 or len(T) < 5:
        out["status"] = NO_MODEL if len(M) < 5 else SHORT_TEMPLATE
        return done()
    N = (normals32 if single else normals64)(M, num_neighbors).astype(f64)
    M64 = M.astype(f64)
    active = np.ones(len(T), bool) if indist <= 0 else np.zeros(len(T), bool)
    delta, it = 1000.0, 0
    while it < max_iterations and delta > min_delta:
        s = transform64(R, t, T)
        q = s.astype(f32)
        idx = nearest(q, M)
        d, n = M64[idx], N[idx]
        if indist > 0:
            indist = max(indist * 0.9, 0.05)
            active = gate_mask(s, d, n, indist, gate)
        out["trace"].append((active.copy(), idx))
        A, b = rows((q.astype(f64) if single else s)[active], d[active], n[active])
        if single:
            A, b = A.astype(f32), b.astype(f32)
            A_, b_ = np.zeros((6, 6), f32), np.zeros(6, f32)
            if len(b):
                for i in range(6):
                    for j in range(6):
                        A_[i, j] = np.add.accumulate(A[:, i] * A[:, j], dtype=f32)[-1]
                    b_[i] = np.add.accumulate(A[:, i] * b, dtype=f32)[-1]
            x = solve32(A_, b_)
        else:
            A_, b_ = A.T @ A, A.T @ b
            # the reference's test is a pivot below 1e-20; in float64 a system
            # whose smallest singular value is rounding noise stands for it
            sv = np.linalg.svd(A_, compute_uv=False) if len(b) else np.zeros(6)
            x = None if sv[-1] <= 1e-13 * max(sv[0], 1e-300) else np.linalg.solve(A_, b_)
        it += 1
        if x is None:
            delta, out["status"] = 0.0, SINGULAR
            continue
        out["status"] = OK
        R_ = polar(x[:3]).astype(ft)
        t_ = np.asarray(x[3:], ft)
        if single:
            Rn = np.array([[_dot3_32(R_[i], R[:, j]) for j in range(3)] for i in range(3)], f32)
            t = np.array([f32(_dot3_32(R_[i], t) + t_[i]) for i in range(3)], f32)
            R = Rn
            delta = float(max(_l2_32(R_ - np.eye(3, dtype=f32)), _l2_32(t_)))
        else:
            R, t = R_ @ R, R_ @ t + t_
            delta = float(max(np.linalg.norm(R_ - np.eye(3)), np.linalg.norm(t_)))
    out["iterations"], out["delta"] = it, delta
    if it == 0 and indist > 0:
        active[:] = False  # pinned: libicp would read a stale set
    out["n_active"] = int(active.sum())
    if active.any():
        s = transform64(R, t, T)[active]
        idx = nearest(s.astype(f32), M)
        d, n = M64[idx], N[idx]
        terms = (n[:, 0] * (d[:, 0] - s[:, 0]) + n[:, 1] * (d[:, 1] - s[:, 1])) + n[:, 2] * (d[:, 2] - s[:, 2])
        out["residual"] = float(np.add.accumulate(terms)[-1] / len(terms))
    return done()


def ref64(T, M, guess=None, **kw):
    return fit(T, M, guess, single=False, **kw)


def ref32(T, M, guess=None, **kw):
    return fit(T, M, guess, single=True, **kw)


def same_trace(a, b):
    return (a["iterations"] == b["iterations"] and a["status"] == b["status"] and len(a["trace"]) == len(b["trace"])
            and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1][x[0]], y[1][y[0]])
                    for x, y in zip(a["trace"], b["trace"])))


# ------------------------------------------------------------------ the scenes
def corner(n, seed, noise=0.002):
    """n points on three mutually orthogonal walls meeting at (1, 1, 3) (a room
    corner seen from inside, coordinates 1-4 m), jittered by `noise` along the
    wall normals, in random order."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 3, n)
    uv = rng.uniform(0.0, 1.0, (n, 2))
    P = np.empty((n, 3))
    for a in range(3):
        m = w == a
        P[m] = np.insert(uv[m], a, 0.0, axis=1)
    P[np.arange(n), w] += noise * rng.standard_normal(n)
    P = P @ rotation([0.3, -0.2, 0.4]).T + [1.0, 1.0, 3.0]  # no wall along an axis
    return np.ascontiguousarray(P, f32)


def rotation(rv):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(rv).as_matrix()


def motion(deg=1.0, shift=0.02, seed=0):
    """A rigid motion of `deg` degrees about a random axis and `shift` metres."""
    rng = np.random.default_rng(1000 + seed)
    ax, tr = rng.standard_normal(3), rng.standard_normal(3)
    P = np.eye(4)
    P[:3, :3] = rotation(np.radians(deg) * ax / np.linalg.norm(ax))
    P[:3, 3] = shift * tr / np.linalg.norm(tr)
    return P


def moved(P, Tm):
    """The cloud whose points Tm carries onto P's surface: inv(Tm) applied to P."""
    Ti = np.linalg.inv(Tm)
    return np.ascontiguousarray(np.asarray(P, f64) @ Ti[:3, :3].T + Ti[:3, 3], f32)


def pair(n_t, n_m, seed):
    """(template, model): two samplings of the corner, the template displaced by
    a 2 cm / 1 degree motion that ICP has to find."""
    return moved(corner(n_t, 2 * seed + 1), motion(seed=seed)), corner(n_m, 2 * seed)


def tilted_wall(nz_sign):
    """(template, model): a 12 x 12 wall whose signed normal has nz of the given
    sign, and a template 0.2 m off it along the normal: far outside a 0.05 gate."""
    g = np.stack(np.meshgrid(np.arange(12) * 0.05, np.arange(12) * 0.05, indexing="ij"), -1).reshape(-1, 2)
    rng = np.random.default_rng(11)
    # (+, +, -) keeps its sign under the rule and its negation (-, -, +) is turned into it
    n = np.array([0.6, 0.48, -0.64]) if nz_sign < 0 else np.array([0.48, 0.6, 0.64])
    e1 = np.cross(n, [0.0, 1.0, 0.3])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    M = g[:, :1] * e1 + g[:, 1:] * e2 + [1.0, 1.0, 2.0] + 1e-4 * rng.standard_normal((144, 1)) * n
    return f32(M[20:120] + 0.2 * n), f32(M)


def exact_plane(n=8, h=0.25, z=2.0):
    """n x n points at spacing h on z = const: H's third row and column are exactly 0."""
    g = np.stack(np.meshgrid(np.arange(n) * h, np.arange(n) * h, indexing="ij"), -1).reshape(-1, 2)
    return f32(np.c_[g, np.full(len(g), z)])


def tie_scene(a_first):
    """(template, model, index of q in the template): two horizontal sheets of
    points at spacing 4 g, g = 1/128, heights quantised to 2^-12: A at z about 2
    and C at z about 2 + 16 g, C only from x = q_x + 8 g on. Template point q = a
    + (0, 0, 10 g) stands over a on A and 10 g from b = q + (8 g, 0, 6 g), C's
    nearest point, in float32 d2 too (100 g^2 both, exactly); every other model
    point is at 116 g^2 or more, and the ten neighbours of a and of b lie on
    their own sheet. Under ODO_ICP_GATE_PLANE at the 0.05 floor a is outside (10
    g = 0.078) and b inside (6 g = 0.047), whichever sign the normals take, so
    which of the two the search takes shows in n_active (and in T). a_first: a
    has the lower index."""
    rng = np.random.default_rng(21)
    g = 1.0 / 128
    q12 = lambda m: np.round(m * 4096) / 4096
    i, j = [x.reshape(-1) for x in np.meshgrid(np.arange(12), np.arange(12), indexing="ij")]
    A = np.c_[1.0 + 4 * g * i, 1.0 + 4 * g * j, 2.0 + q12(2e-4 * rng.standard_normal(144))]
    C = np.c_[1.0 + 4 * g * (i + 6), 1.0 + 4 * g * j, 2.0 + 16 * g + q12(2e-4 * rng.standard_normal(144))]
    ia, ib = 4 * 12 + 5, 0 * 12 + 5
    A[ia, 2], C[ib, 2] = 2.0, 2.0 + 16 * g
    q = A[ia] + [0, 0, 10 * g]
    assert np.array_equal(C[ib], q + [8 * g, 0, 6 * g])
    # the other template points: 0.01 over points of A away from q
    others = A[(i >= 8) & (j % 2 == 0)] + [0, 0, 0.01]
    # a corner 2 m away, sampled twice, conditions the six unknowns
    far = [2.0, 0.0, 0.0]
    T = np.r_[others[:17], [q], others[17:], moved(corner(60, 6), motion(0.2, 0.004, 9)) + far]
    M = np.r_[A, C, corner(200, 5) + far] if a_first else np.r_[C, A, corner(200, 5) + far]
    return f32(T), f32(M), 17


# The loop cases: name -> (template, model, keyword arguments). The all-active
# cases stop at 8 iterations (at libicp's 1e-4 a float32 run can keep stepping
# by its own rounding noise long after float64 has stopped).
LOOP_SIZES = ((64, 96, 1), (300, 300, 2), (2000, 2000, 3))
LOOP_INDIST = (-1.0, 0.01, 1.0)


def loop_cases():
    c = {}
    for nt, nm, seed in LOOP_SIZES:
        T, M = pair(nt, nm, seed)
        for ind in LOOP_INDIST:
            for gate in (GATE_AS_WRITTEN, GATE_PLANE):
                kw = dict(num_neighbors=10, max_iterations=8 if ind <= 0 else 50, min_delta=1e-4, indist=ind, gate=gate)
                c[f"corner{nt}_indist{ind:g}_gate{gate}"] = (T, M, kw)
    # the test program's setting (Tests/IcpPointToPlane.cpp: 15 neighbours, 50 iterations, 1e-8, 0.01)
    T, M = pair(300, 300, 4)
    c["corner300_test_program"] = (T, M, dict(num_neighbors=15, max_iterations=50, min_delta=1e-8, indist=0.01,
                                              gate=GATE_AS_WRITTEN))
    return c


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def loop_refs(name):
    """(ref64, ref32, stable) of a loop case, once per session."""
    def make():
        T, M, kw = loop_cases()[name]
        a, b = ref64(T, M, **kw), ref32(T, M, **kw)
        return a, b, same_trace(a, b)
    return cached(("loop", name), make)


def e_ref(name):
    a, b, _ = loop_refs(name)
    return float(np.abs(a["T"] - b["T"]).max())


def tolerance():
    """4 * max(e_ref over the stable loop cases, 1e-6): the device against ref64."""
    def make():
        es = [e_ref(n) for n in loop_cases() if loop_refs(n)[2]]
        return 4.0 * max(es + [1e-6])
    return cached("tolerance", make)


def residual_rtol():
    """The same construction for the residual, on relative differences."""
    def make():
        rel = [abs(a["residual"] - b["residual"]) / abs(a["residual"])
               for a, b, st in (loop_refs(n) for n in loop_cases()) if st and a["residual"] != 0]
        return 4.0 * max(rel + [1e-6])
    return cached("residual_rtol", make)
