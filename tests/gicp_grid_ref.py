"""The grid neighbour searches of dense GICP, restated in numpy -- TEST INFRASTRUCTURE.

k_gicp.hip's grid path (DESIGN §4 "Dense GICP") from its definitions: the cell
rule (plan), the cell of a point (cells_of: floorf((p - min) * inv) per axis in
float32, clamped), the cell-ordered points (build: a sort by cell key, the
order within a cell optionally shuffled, since no result may depend on it), the
Chebyshev ring search for the 20 covariance neighbours with the stop rule
(knn20) and the correspondence search over a fixed number of rings
(first_corr). Selections compare (distance, index).

The stop rule. After every cell within Chebyshev ring r of the query's cell has
been examined, an unseen point p differs from the query q by at least r + 1
cells on some axis a, so the COMPUTED t = fl(fl(x - min) * inv) differ by more
than r. Each t carries two roundings, |t - (x - min) inv| <= (2u + u^2) (x -
min) inv with u = 2^-24 and 0 <= x - min <= E (the extent; E + w for a query
that lies outside the bounds in the border cell), so in real numbers
    |p_a - q_a| > r w - 2 (2u + u^2) (E + w)  >=  r w - slack,
w = 1 / inv the cell edge, slack = (E + w) 2^-21 (twice what is needed). dist2f
rounds five times on the way (difference, square, two sums, each relative u)
and its three products may underflow (absolute 2^-150 each), so the float
distance of an unseen point is at least
    bound(r) = (r w - slack)^2 (1 - 2^-20) - 2^-140        (0 where r w <= slack)
and the search stops only when the 20th distance held is STRICTLY below it:
an unseen point can then neither beat nor tie a held one. A search that runs
out of rings has seen the whole cloud.

tests/test_gicp_grid_ref.py holds this against gicp_ref64's brute force on the
CPU; tests/test_gicp_grid_gpu.py the kernels against the oracle and against the
brute-force kernels.
"""
from __future__ import annotations

import math

import numpy as np

import gicp_ref64 as G

f32 = np.float32
K = 20
MAX_CELLS = 1 << 24
COV_CELLS = (0.0, 0.0625, 0.25, 1000.0)


# ------------------------------------------------------------------ the rule
def ring_bound(w, slack, r):
    g = r * w - slack
    return g * g * (1.0 - 2.0 ** -20) - 2.0 ** -140 if g > 0 else 0.0


def icp_rings(w, slack, mcd, max_dim):
    r = math.ceil((mcd * (1.0 + 2.0 ** -19) + slack) / w)
    r = max(r, 1)
    if r >= max_dim:
        return max(max_dim, 1)
    while r < max_dim and ring_bound(w, slack, r) < mcd * mcd:
        r += 1
    return r


def plan(P, cell=0.0, mcd=0.0):
    """The grid of a cloud of >= 1 points: dict(mn, inv, dims, w, slack, rings),
    or None where a forced cell needs more than 2^24 cells."""
    P = np.asarray(P, f32)
    mn, mx = P.min(axis=0), P.max(axis=0)
    emax = float((mx.astype(np.float64) - mn.astype(np.float64)).max())
    forced = cell > 0
    with np.errstate(over="ignore"):
        span_ok = bool(np.all(np.isfinite(mx - mn)))
    one_cell = dict(mn=mn, inv=f32(0.0), dims=[1, 1, 1], w=emax + 1.0, slack=0.0, rings=1)
    if not span_ok:  # fl(x - min) overflows: one cell (a forced cell does not fit)
        return None if forced else one_cell
    if forced:
        c = f32(cell)
    else:
        cd = max(emax / (8.0 * len(P)) ** (1.0 / 3.0), mcd * (1.0 + 2.0 ** -10) + 4.0 * (emax + mcd) * 2.0 ** -21)
        c = f32(cd if cd > 0 else 1.0)
        if not (c > 0 and np.isfinite(c)):
            c = f32(1.0)
    while True:
        with np.errstate(over="ignore", divide="ignore"):
            inv = f32(1.0) / c
        fits = bool(np.isfinite(inv) and inv > 0)
        dims = [1, 1, 1]
        if fits:
            with np.errstate(over="ignore"):
                t = np.floor((mx - mn) * inv)
            if not np.all(t < f32(MAX_CELLS)):
                fits = False
            else:
                dims = [int(v) + 1 for v in t]
        if fits and dims[0] * dims[1] * dims[2] > MAX_CELLS:
            fits = False
        w = 1.0 / float(inv) if fits else 0.0
        slack = (emax + w) * 2.0 ** -21
        rings = icp_rings(w, slack, mcd, max(dims)) if fits else 0
        if not fits or (not forced and rings > 1 and max(dims) > 1):
            if forced:
                return None
            with np.errstate(over="ignore"):
                c = c * (f32(1.0009765625) if fits else f32(2.0))
            if not np.isfinite(c):
                return one_cell
            continue
        return dict(mn=mn, inv=inv, dims=dims, w=w, slack=slack, rings=rings)


def cells_of(g, Q):
    """n x 3 integer cells of the rows of Q (points of the cloud or queries)."""
    Q = np.asarray(Q, f32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor((Q - g["mn"]) * g["inv"])
    assert t.dtype == f32
    return np.clip(np.nan_to_num(t, nan=0.0), 0, np.asarray(g["dims"], f32) - 1).astype(np.int64)


def build(P, cell=0.0, mcd=0.0, shuffle=None):
    """The grid with its cell-ordered points: keys (sorted), order (point index
    of every row). shuffle: a Generator that permutes the rows within a cell."""
    P = np.asarray(P, f32)
    g = plan(P, cell, mcd)
    assert g is not None
    c = cells_of(g, P)
    gx, gy, _ = g["dims"]
    key = (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0]
    tie = shuffle.permutation(len(P)) if shuffle is not None else np.arange(len(P))
    order = np.lexsort((tie, key))
    g.update(P=P, cells=c, keys=key[order], order=order)
    return g


def _run(g, first, last):
    """Rows of the cells first ... last (one run: x is the fastest axis)."""
    a, b = np.searchsorted(g["keys"], first, "left"), np.searchsorted(g["keys"], last, "right")
    return g["order"][a:b]


def ring_points(g, c, r):
    """Point indices of the cells at Chebyshev distance exactly r from cell c
    (from the definition; the kernel walks the shell's rows of cells)."""
    return np.flatnonzero(np.abs(g["cells"] - c).max(axis=1) == r)


def knn20(g, stop=ring_bound):
    """(n x 20 neighbour lists ordered by (distance, index), rings examined per
    point) of the cloud of grid g. stop: the bound of the stop rule."""
    P, n = g["P"], len(g["P"])
    assert n >= K
    nn, rings = np.empty((n, K), np.int64), np.empty(n, np.int64)
    dims = np.asarray(g["dims"])
    for q in range(n):
        c = g["cells"][q]
        rmax = int(np.maximum(c, dims - 1 - c).max())
        hd, hi = np.zeros(0, f32), np.zeros(0, np.int64)
        r = 0
        while True:
            idx = ring_points(g, c, r)
            d = np.r_[hd, G.dist2_f32(P[q], P[idx])] if len(idx) else hd
            i = np.r_[hi, idx]
            keep = np.lexsort((i, d))[:K]
            hd, hi = d[keep], i[keep]
            if r >= rmax or (len(hd) == K and float(hd[K - 1]) < stop(g["w"], g["slack"], r)):
                break
            r += 1
        assert len(hi) == K
        nn[q], rings[q] = hi, r
    return nn, rings


def apply_guess(S, guess):
    """transformPointCloud as k_gicp's first loop: float32, left to right."""
    S = np.asarray(S, f32)
    M = np.asarray(np.eye(4) if guess is None else guess, f32)
    x, y, z = S[:, 0], S[:, 1], S[:, 2]
    return np.stack([M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)], 1).astype(f32)


def first_corr(src, tgt, max_corr_dist, cell=0.0, shuffle=None):
    """gicp_ref64.first_corr through the grid of the target: the cells within
    g["rings"] of each source point's clipped cell, the best by (distance, index)."""
    src = np.asarray(src, f32)
    g = build(tgt, cell, max_corr_dist, shuffle)
    gx, gy, gz = g["dims"]
    R = g["rings"]
    thr = float(max_corr_dist) * float(max_corr_dist)
    si, ti = [], []
    for i, (p, c) in enumerate(zip(src, cells_of(g, src))):
        cand = [_run(g, (z * gy + y) * gx + max(c[0] - R, 0), (z * gy + y) * gx + min(c[0] + R, gx - 1))
                for z in range(max(c[2] - R, 0), min(c[2] + R, gz - 1) + 1)
                for y in range(max(c[1] - R, 0), min(c[1] + R, gy - 1) + 1)]
        idx = np.concatenate(cand)
        if not len(idx):
            continue
        d = G.dist2_f32(p, g["P"][idx])
        j = np.lexsort((idx, d))[0]
        if float(d[j]) < thr:
            si.append(i)
            ti.append(int(idx[j]))
    return np.asarray(si, np.int64), np.asarray(ti, np.int64), g


# ------------------------------------------------------------------ cases
def two_clusters():
    """10 + 15 points in two 0.1 m cubes 3 m apart: the 20 neighbours of every
    point reach into the other cluster, across about 60 empty rings at cell 0.05."""
    rng = np.random.default_rng(0x2C)
    a = rng.uniform(0.0, 0.1, (10, 3)) + [0.0, 0.0, 2.0]
    b = rng.uniform(0.0, 0.1, (15, 3)) + [3.0, 0.0, 2.0]
    return np.r_[a, b].astype(f32)


def face_lattice():
    """gicp_ref64.lattice(), spacing 0.25 from the cloud's minimum: at cells 0.25,
    0.125 and 0.0625 every point lies on cell faces, and equal distances tie
    across cells."""
    return G.lattice()


def far():
    """200 points, one axis 100 times the others (1 x 1 x 100 m)."""
    rng = np.random.default_rng(0xFA)
    return (rng.uniform(0.0, 1.0, (200, 3)) * [1.0, 1.0, 100.0]).astype(f32)


def translation(t):
    T = np.eye(4, dtype=f32)
    T[:3, 3] = t
    return T


def outside():
    """(src, tgt, guess): the guess moves the source 10 m beyond the target's bounds."""
    return G.scene(300), G.shifted(G.scene(300)), translation([10.0, 0.0, 0.0])


def half_outside():
    """(src, tgt, guess): the source is the scene 1 m to the left, the guess brings
    it back, the target is the part x <= -0.3 of the shifted scene: about half of
    the moved source lies beyond the target's bounds by more than 0.07 m."""
    S = G.scene(300)
    T = G.shifted(S)
    return (S - f32([1.0, 0.0, 0.0])).astype(f32), np.ascontiguousarray(T[T[:, 0] <= -0.3]), translation([1.0, 0.0, 0.0])


def outside_fraction(src, tgt, guess, margin=0.0):
    """Share of the moved source points outside the target's bounds by more than margin."""
    m = apply_guess(src, guess)
    lo, hi = tgt.min(axis=0) - margin, tgt.max(axis=0) + margin
    return float(np.mean(np.any((m < lo) | (m > hi), axis=1)))


NEW_CLOUDS = dict(two_clusters=two_clusters, face_lattice=face_lattice, far=far)
NEW_PAIRS = dict(outside=outside, half_outside=half_outside)


def cloud(name):
    if name in NEW_CLOUDS:
        return G.cached(("grid_case", name), lambda: np.ascontiguousarray(NEW_CLOUDS[name]()))
    return G.case(name)


def pair(name):
    return G.cached(("grid_pair", name), NEW_PAIRS[name])
