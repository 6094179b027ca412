"""StatisticalOutlierRemoval and GICP's fitness score, restated in numpy -- TEST
INFRASTRUCTURE.

Brute-force restatements of the semantics include/odo.h pins for
odo_cloud_sor_batch / odo_dense_sor and odo_gicp_grid_fitness /
odo_gicp_dense_fitness (PCL's StatisticalOutlierRemoval::applyFilterIndices and
Registration::getFitnessScore from their source as recalled; PCL is absent, so
parity with the library is unpinned). float32 elementwise arithmetic for the
squared distance (gicp_ref64.dist2_f32, the kernels' dist2f), the float
product distances[i] * distances[i] and sqrtf; the sums are float64 in PCL's
index order (np.cumsum is sequential).

What the device may differ by. It adds the same non-negative terms in a fixed
order of its own. A recursive float64 sum of n non-negative terms in ANY order
is within (n - 1) u S of the exact sum S (u = 2^-53, to first order; E = 1.01
(n - 1) u covers the higher orders for n <= 2^20), so two orders differ by at
most 2 E S: with r = 2 E,
    |d sum| <= r sum,   |d sq_sum| <= r sq_sum.
Every later operation is one correctly rounded double operation on each side
(4 u covers both sides and a device sqrt / division one ulp off):
    mean = sum / n                     |d mean| <= (r + 4u) mean
    B = sum * sum / n                  |d B|    <= (2r + 8u) B
    var = (sq_sum - B) / (n - 1)       |d var|  <= (r sq_sum + (2r + 8u) B) / (n - 1) + 4u |var|
which is the cancellation: the error is relative to sq_sum and B, not to their
difference. Three cases:
    var - |d var| > 0    both sides take a root: |d stddev| <= |d var| / stddev + 4u stddev
                         (sqrt(a) - sqrt(b) = (a - b) / (sqrt(a) + sqrt(b)), one root is the reference's)
    var + |d var| < 0    both sides get NaN: stddev and threshold NaN, every point kept
    otherwise            the sign is not determined: no bound (inf), such a cloud is no test case
    threshold = mean + mul stddev      |d thr| <= |d mean| + |mul| |d stddev| + 4u (|mean| + |mul| stddev)
threshold_bound(ref) returns these. The keep mask is required exactly on a case
none of whose distances lies within the threshold's bound of the threshold
(margin_ok; tests/test_sor_ref.py checks it for every case, a condition on the
inputs, not a tolerance on the kernel). distances[] holds no reordered sum: each
is a sequential sum over an ascending list, so it is compared bit for bit.

The fitness score is one such sum divided by ns: |d score| <= (r + 4u) score
with n = ns (fitness_bound).

The ring walk's stop rule for a query outside the grid (the fitness search has no
distance cap, and a transformed source point may lie anywhere).
tests/gicp_grid_ref.py's argument covers a query up to one cell outside the
bounds. For any finite query q let q' be q clamped per axis into the cloud's
bounds [mn, mx]. (1) The walk starts from the cell of q': the computed t =
fl(fl(x - mn) * inv) is monotone in x, the cell of mn is 0 and the cell of mx is
dim - 1 (the grid was sized so), so clamping the cell of q to [0, dim - 1] gives
the cell of q' on every axis (an overflowing x - mn gives +-inf, clamped alike;
the one-cell grid has inv = 0 and every cell 0). (2) q' lies within the bounds,
so the argument holds for it with 0 <= x - mn <= E and no allowance at all:
after ring r an unseen point p has |p_a - q'_a| > r w - slack on some axis a.
(3) p lies within the bounds, and q'_a is the point of [mn_a, mx_a] nearest to
q_a, so |p_a - q_a| >= |p_a - q'_a| > r w - slack. dist2f's rounding argument
does not depend on where q lies (an overflow gives +inf, which is above every
bound), so bound(r) holds for every finite q and the slack needs no widening.
"""
from __future__ import annotations

import sys

import numpy as np

import gicp_grid_ref as R
import gicp_ref64 as G

f32 = np.float32
U = 2.0 ** -53
DBL_MAX = sys.float_info.max
SOR_OK, SOR_SKIPPED = 0, 1
MAX_K = 64  # the kernel's cap on mean_k (include/odo.h)
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -3, -4


# ------------------------------------------------------------------ reference
def seq_sum(x):
    """Sequential float64 sum, first to last."""
    x = np.asarray(x, np.float64)
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def sor_distances(P, mean_k):
    """PCL's distances[] of a cloud of more than mean_k points, float32."""
    P = np.asarray(P, f32)
    n = len(P)
    assert n > mean_k >= 1
    out = np.empty(n, f32)
    for i in range(n):
        d2 = np.sort(G.dist2_f32(P[i], P))[: mean_k + 1]
        assert d2.dtype == f32
        root = np.sqrt(d2[1:])  # float32, correctly rounded; the first is dropped
        assert root.dtype == f32
        out[i] = f32(seq_sum(root) / float(mean_k))
    return out


def sor_stats(dist, mul):
    """sum, sq_sum, mean, var, stddev, threshold of distances[] in PCL's order."""
    dist = np.asarray(dist, f32)
    n = len(dist)
    sq = dist * dist
    assert sq.dtype == f32
    s, q = seq_sum(dist), seq_sum(sq)
    mean = s / n
    var = (q - s * s / n) / (n - 1)
    sd = float(np.sqrt(var)) if var >= 0 else float("nan")
    return dict(n=n, mul=float(mul), sum=s, sq_sum=q, mean=mean, var=var, stddev=sd, threshold=mean + mul * sd)


def sor(P, mean_k, mul):
    """The whole filter on one cloud: dict(status, n_in, n_out, keep, distances,
    mean, stddev, threshold, ...)."""
    P = np.asarray(P, f32).reshape(-1, 3)
    n = len(P)
    if n <= mean_k:
        return dict(status=SOR_SKIPPED, n_in=n, n_out=n, keep=np.ones(n, bool), distances=np.zeros(n, f32), n=n,
                    mul=float(mul), sum=0.0, sq_sum=0.0, mean=0.0, var=0.0, stddev=0.0, threshold=0.0)
    dist = sor_distances(P, mean_k)
    r = sor_stats(dist, mul)
    keep = ~(dist.astype(np.float64) > r["threshold"])  # NaN: all kept
    r.update(status=SOR_OK, n_in=n, n_out=int(keep.sum()), keep=keep, distances=dist)
    return r


def threshold_bound(r):
    """dict(mean, stddev, threshold): what a fixed-order device sum may differ by
    (the module docstring); nan_expected: both sides get a NaN stddev. inf where
    the variance's sign is not determined."""
    n = r["n"]
    if r.get("status") == SOR_SKIPPED or n < 2:
        return dict(mean=0.0, stddev=0.0, threshold=0.0, var=0.0, nan_expected=False)
    rr = 2 * 1.01 * (n - 1) * U
    B = r["sum"] * r["sum"] / n
    dmean = (rr + 4 * U) * abs(r["mean"])
    dvar = (rr * r["sq_sum"] + (2 * rr + 8 * U) * B) / (n - 1) + 4 * U * abs(r["var"])
    if r["var"] + dvar < 0:
        return dict(mean=dmean, stddev=0.0, threshold=0.0, var=dvar, nan_expected=True)
    if r["var"] - dvar <= 0:
        if r["var"] == 0 and dvar == 0:  # all distances zero: exact on both sides
            return dict(mean=0.0, stddev=0.0, threshold=0.0, var=0.0, nan_expected=False)
        return dict(mean=dmean, stddev=float("inf"), threshold=float("inf"), var=dvar, nan_expected=False)
    dsd = dvar / r["stddev"] + 4 * U * r["stddev"]
    dthr = dmean + abs(r["mul"]) * dsd + 4 * U * (abs(r["mean"]) + abs(r["mul"]) * r["stddev"])
    return dict(mean=dmean, stddev=dsd, threshold=dthr, var=dvar, nan_expected=False)


def margin_ok(r):
    """No distance lies within the threshold's bound of the threshold (or the
    threshold is NaN on both sides): the keep mask is then determined."""
    b = threshold_bound(r)
    if r["status"] == SOR_SKIPPED or b["nan_expected"]:
        return True
    if not np.isfinite(b["threshold"]) or np.isnan(r["threshold"]):
        return False
    if b["threshold"] == 0.0:  # all distances zero: both sides compute the same threshold, 0 > 0 is false
        return True
    return bool(np.all(np.abs(r["distances"].astype(np.float64) - r["threshold"]) > b["threshold"]))


def fitness(S, T, M=None):
    """(score, nn_d2 float32 per source point); DBL_MAX for an empty side (nn zeros)."""
    S, T = np.asarray(S, f32).reshape(-1, 3), np.asarray(T, f32).reshape(-1, 3)
    if len(S) == 0 or len(T) == 0:
        return DBL_MAX, np.zeros(len(S), f32)
    m = R.apply_guess(S, M)
    nn = np.array([G.dist2_f32(p, T).min() for p in m], f32)
    return seq_sum(nn) / len(S), nn


def fitness_bound(score, ns):
    return (2 * 1.01 * max(ns - 1, 0) * U + 4 * U) * abs(score)


# ------------------------------------------------------------------ the cases
def blob_outlier():
    """200 points in a 0.2 m cube and one point 50 m away on every axis: the
    outlier stretches the bounds, so at any cell that fits the table the blob
    shares a few cells."""
    rng = np.random.default_rng(0x50)
    return np.r_[rng.uniform(0.0, 0.2, (200, 3)) + [0.0, 0.0, 1.0], [[50.0, 50.0, 51.0]]].astype(f32)


def two_sites(na, nb):
    """na + nb points, coincident within each of two sites 3 m apart along x."""
    return np.r_[np.tile([0.5, -0.25, 2.0], (na, 1)), np.tile([3.5, -0.25, 2.0], (nb, 1))].astype(f32)


def plane(n=100):
    rng = np.random.default_rng(0x91)
    return np.c_[rng.uniform(0.0, 1.0, (n, 2)), np.full(n, 2.0)].astype(f32)


def cube_negative_variance():
    """The 8 corners of a cube of edge h, mean_k 3: every distances[i] is the same
    float g = sqrtf(fl(h * h)), so the exact variance is 0 and the computed one is
    8 (fl32(g * g) - g * g) / 7; h is the first edge for which the float product
    rounds DOWN, which makes it negative by about 2^-25 g^2, far beyond the
    bound."""
    for i in range(1, 1000):
        h = f32(0.3) + f32(i) * f32(2.0 ** -10)
        g = np.sqrt(f32(h * h))
        if float(f32(g * g)) < float(g) * float(g):
            z, y, x = np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")
            return (np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(f32) * h).astype(f32)
    raise AssertionError("no edge found")


def cases():
    """name -> (cloud, mean_k, stddev_mul), one cloud each."""
    c = {}
    c["n_eq_k_skipped"] = (G.scene(20), 20, 1.0)
    c["n_eq_k_plus_1"] = (G.scene(21), 20, 1.0)  # every search is the whole cloud
    for k in (1, 8, 20, 50, MAX_K):
        c[f"scene300_k{k}"] = (G.scene(300), k, 1.0)
    c["coincident"] = (G.coincident(70), 50, 1.0)
    c["two_sites_large"] = (two_sites(12, 15), 8, 1.0)  # each site > mean_k: all distances zero
    c["two_sites_small"] = (two_sites(5, 6), 8, 1.0)    # each site < mean_k + 1: neighbours at the other site
    c["lattice"] = (G.lattice(), 8, 1.0)
    c["line"] = (G.collinear_axis(25), 8, 1.0)
    c["plane"] = (plane(), 8, 1.0)
    c["blob_outlier"] = (blob_outlier(), 20, 1.0)
    for n in (63, 64, 65, 257):
        c[f"scene{n}"] = (G.scene(n), 8, 1.0)
    c["mul_zero"] = (G.scene(300), 8, 0.0)
    c["mul_negative"] = (G.scene(300), 8, -1.0)
    c["mul_large"] = (G.scene(300), 8, 100.0)
    c["negative_variance"] = (cube_negative_variance(), 3, 1.0)
    return c


def mixed_batch():
    """(clouds, mean_k, mul): mixed sizes with an empty and a skipped cloud between filtered ones."""
    return [G.scene(100), np.zeros((0, 3), f32), G.scene(5), G.scene(257), G.coincident(30), blob_outlier()], 8, 1.0


TINY_DIV = {"two_sites_large": 300, "two_sites_small": 300}  # these clouds span one axis only


def cells_for(P, name=None):
    """The automatic cell, a tiny one (1 / 64 of the longest side: up to 2^18 cells,
    which a search that runs out of rings walks in full; 1 / 300 where the case
    asks for hundreds of empty cells), one in between, and one cell for the cloud."""
    P = np.asarray(P, f32)
    E = float((P.max(0).astype(np.float64) - P.min(0)).max()) if len(P) else 0.0
    return (0.0, E / TINY_DIV.get(name, 64) if E > 0 else 0.01, E / 8 if E > 0 else 0.5, 2 * E + 1.0)


def case(name):
    return G.cached(("sor_case", name), lambda: cases()[name])


def ref(name):
    """The reference of a case, computed once per session."""
    P, k, mul = case(name)
    return G.cached(("sor_ref", name), lambda: sor(P, k, mul))


def fitness_cases():
    """name -> (source, target, T)."""
    S, Tg = G.scene(300), G.shifted(G.scene(300))
    c = {"scene": (S, Tg, None), "coincident": (S, S.copy(), None)}
    for a in range(3):
        for sgn in (-1.0, 1.0):
            t = [0.0, 0.0, 0.0]
            t[a] = sgn * 25.0
            c[f"outside_{'xyz'[a]}{'+' if sgn > 0 else '-'}"] = (G.scene(65), Tg, R.translation(t))
    c["outside_corner"] = (G.scene(65), Tg, R.translation([40.0, -30.0, 20.0]))
    c["half_outside"] = R.pair("half_outside")
    c["target_1"] = (G.scene(65), Tg[:1], None)
    c["target_64"] = (G.scene(65), Tg[:64], None)
    c["target_65"] = (G.scene(64), Tg[:65], None)
    c["empty_source"] = (np.zeros((0, 3), f32), Tg, None)
    c["empty_target"] = (S[:10], np.zeros((0, 3), f32), None)
    return c
