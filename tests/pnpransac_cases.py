"""Crafted PnPRansac problems at the widths of k_pnpransac.hip, and the pieces
of cv::solvePnPRansac that can be restated independently of the oracle.

The builders return a Case: (Xw, uv, iterations, reproj, conf) plus `prop`,
the property the case exists for, stated on the builder's own labels or as a
figure the reference side must reproduce (tests/test_pnpransac_cases.py
asserts every one of them on the oracle; the device never enters a claim).

The independent pieces are numpy / scipy only (no oracle code):
  subsets_py   cv::RNG(-1) + getSubset's retry rule -> every hypothesis' indices
  fold_py      RANSACPointSetRegistrator::run's loop over the inlier counts
  count64      float64 reprojection errors -> inlier mask + "on the edge" flags
  minimum64    scipy least_squares on the reprojection residuals, float64
"""
import math
from dataclasses import dataclass, field

import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

import oracle_lib as O

FLT_EPSILON = float(np.finfo(np.float32).eps)


# ------------------------------------------------- helpers shared with test_pnpransac.py
def _problem(seed, n, outlier_frac, noise=0.5, planar=False):
    rng = np.random.default_rng(seed)
    cal = O.fr1_calib()
    Xc = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1, 5, n)]
    if planar:
        Xc[:, 2] = 3.0 + 0.2 * Xc[:, 0]
    rv = rng.normal(0, 0.2, 3)
    t = rng.normal(0, 0.3, 3)
    R = Rotation.from_rotvec(rv).as_matrix()
    Xw = (Xc - t) @ R  # Xc = R Xw + t
    uv = np.c_[cal.fx * Xc[:, 0] / Xc[:, 2] + cal.cx, cal.fy * Xc[:, 1] / Xc[:, 2] + cal.cy]
    uv += rng.normal(0, noise, uv.shape)
    out = rng.random(n) < outlier_frac
    uv[out] += rng.uniform(-80, 80, (out.sum(), 2))
    return Xw.astype(np.float32), uv.astype(np.float32), cal, rv, t, out


def _five_inliers(seed):
    """12 observations, 5 exact and 7 moved 40-120 px: the best RANSAC model
    has exactly 5 inliers (goodCount > modelPoints - 1 accepts it)."""
    Xw, uv, cal, *_ = _problem(seed, 12, 0.0, noise=0.0)
    rng = np.random.default_rng(seed + 1000)
    ang = rng.uniform(0, 2 * np.pi, 7)
    uv[5:] += (np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(40, 120, (7, 1))).astype(np.float32)
    return Xw, uv, cal


def _cvrng_py(state, a, b, n):
    out = []
    for _ in range(n):
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
        out.append(a + (state & 0xFFFFFFFF) % (b - a))
    return out


def _update_py(p, ep, m, maxit):
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    denom = 1.0 - (1.0 - ep) ** m
    if denom < 2.2250738585072014e-308:
        return 0
    num, denom = math.log(num), math.log(denom)
    return maxit if denom >= 0 or -num >= maxit * (-denom) else int(round(num / denom))


def update_quotient(p, ep, m=5):
    """num / denom of RANSACUpdateNumIters before it is rounded (_update_py's formula)."""
    return math.log(max(1.0 - p, 2.2250738585072014e-308)) / math.log(1.0 - (1.0 - ep) ** m)


# ------------------------------------------------------------ independent pieces
def subsets_py(n, H):
    """Every hypothesis' 5 indices: RNG rng((uint64)-1), rng.uniform(0, n) per
    draw, a draw equal to an earlier index of the same subset drawn again
    (ptsetreg.cpp getSubset). Returns (idx H x 5, redraws) with redraws a list
    of (h, i, j): while filling slot i of hypothesis h a draw equalled slot j."""
    need = 8 * H + 64
    stream = _cvrng_py((1 << 64) - 1, 0, n, need)
    pos = 0
    idx = np.zeros((H, 5), np.int64)
    redraws = []
    for h in range(H):
        sub = []
        for i in range(5):
            while True:
                if pos == len(stream):  # the stream is sequential: a longer one has the same head
                    need *= 2
                    stream = _cvrng_py((1 << 64) - 1, 0, n, need)
                v = stream[pos]
                pos += 1
                if v in sub:
                    redraws.append((h, i, sub.index(v)))
                    continue
                break
            sub.append(v)
        idx[h] = sub
    return idx, redraws


def fold_py(good, n, H, conf):
    """run()'s loop: a hypothesis wins when its count exceeds max(maxGood, 4),
    and then shrinks niters. good needs the visited entries only.
    Returns (best, visited, maxGood)."""
    niters, max_good, best, it = max(H, 1), 0, -1, 0
    while it < niters:
        g = int(good[it])
        if g > max(max_good, 4):
            best, max_good = it, g
            niters = _update_py(conf, (n - g) / n, 5, niters)
        it += 1
    return best, it, max_good


def project64(rt, Xw, cal):
    R = Rotation.from_rotvec(np.asarray(rt[:3], np.float64)).as_matrix()
    Xc = np.asarray(Xw, np.float64) @ R.T + np.asarray(rt[3:], np.float64)
    return np.c_[cal.fx * Xc[:, 0] / Xc[:, 2] + cal.cx, cal.fy * Xc[:, 1] / Xc[:, 2] + cal.cy]


def count64(model, Xw, uv, thr, cal=None):
    """Inlier mask of `model` from float64 reprojection errors (e2 <= thr, thr
    the squared pixel error) and, per point, whether |e2 - thr| <= 1e-3 thr:
    there float32 rounding of the projection may decide either way."""
    cal = cal or O.fr1_calib()
    with np.errstate(all="ignore"):
        e2 = ((project64(model, Xw, cal) - np.asarray(uv, np.float64)) ** 2).sum(1)
    return e2 <= thr, np.abs(e2 - thr) <= 1e-3 * thr


def minimum64(rt0, Xw, uv, cal=None):
    """The float64 minimum of the reprojection residuals over (rvec, tvec),
    started at rt0, tolerances 1e-15."""
    cal = cal or O.fr1_calib()
    X, u = np.asarray(Xw, np.float64), np.asarray(uv, np.float64)

    def resid(p):
        return (project64(p, X, cal) - u).ravel()

    s = least_squares(resid, np.asarray(rt0, np.float64), xtol=1e-15, ftol=1e-15, gtol=1e-15, method="lm")
    return s.x


def scatter_ratio64(Xw):
    """w[2] / w[1] of the points' 3 x 3 scatter matrix (cvFindExtrinsicCameraParams2's planarity figure)."""
    X = np.asarray(Xw, np.float64)
    d = X - X.mean(0)
    w = np.linalg.svd(d.T @ d, compute_uv=False)
    return w[2] / w[1]


# ------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    Xw: np.ndarray
    uv: np.ndarray
    iterations: int = 500
    reproj: float = 3.0
    conf: float = 0.85
    prop: dict = field(default_factory=dict)

    def args(self):
        return self.Xw, self.uv, self.iterations, self.reproj, self.conf


def _gross(uv, where, rng):
    """Move the observations `where` by 40-120 px in a random direction."""
    k = int(np.count_nonzero(where)) if np.asarray(where).dtype == bool else len(where)
    ang = rng.uniform(0, 2 * np.pi, k)
    uv[where] += (np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(40, 120, (k, 1))).astype(np.float32)


def crafted(n, g, seed, noise=0.0):
    """n observations of one pose, g of them inliers (exact, or with `noise` px)
    and n - g moved 40-120 px, permuted. Returns (Xw, uv, labels)."""
    Xw, uv, *_ = _problem(seed, n, 0.0, noise=noise)
    rng = np.random.default_rng(seed + 7)
    ang = rng.uniform(0, 2 * np.pi, n - g)
    uv[g:] += (np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(40, 120, (n - g, 1))).astype(np.float32)
    p = rng.permutation(n)
    lab = np.arange(n) < g
    return Xw[p], uv[p], lab[p]


POINT_WIDTHS = (10, 11, 63, 64, 65, 255, 256, 257, 513)


def point_width(n):
    """n at a width of k_pr_count (256-thread stride, 4-wave tail) or of the
    64-lane loops: 30 % gross outliers; the last index is an inlier and the
    last full wave / block before it holds inliers (asserted on the labels)."""
    Xw, uv, *_ = _problem(500 + n, n, 0.0, noise=0.5)
    rng = np.random.default_rng(900 + n)
    lab = np.ones(n, bool)
    lab[rng.permutation(n - 1)[:int(round(0.3 * n))]] = False  # never the last index
    _gross(uv, ~lab, rng)
    assert lab[-1]
    spans = []
    if n >= 64:
        spans.append((64 * (n // 64) - 64, 64 * (n // 64)))  # the last full wave
    if n >= 256:
        spans.append((256 * (n // 256) - 64, 256 * (n // 256)))  # the last wave of the last full block
    for lo, hi in spans:
        assert lab[lo:hi].any()
    return Case(f"points_{n}", Xw, uv, prop=dict(kind="points", labels=lab, spans=spans))


# inlier count -> seed at which the oracle's best model keeps exactly the labelled inliers
INLIER_WIDTHS = {6: 0, 7: 0, 63: 1, 64: 4, 65: 1, 129: 1}


def inlier_width(count):
    """`count` inliers (0.5 px noise) of n = count + 8 at a width of the
    one-wave refine kernel; 6 is the smallest count the DLT accepts."""
    Xw, uv, lab = crafted(count + 8, count, 700 + 16 * count + INLIER_WIDTHS[count], noise=0.5)
    return Case(f"inliers_{count}", Xw, uv, prop=dict(kind="inliers", labels=lab, n_inliers=count))


# visited -> (n, exact inliers, seed): RANSACUpdateNumIters(0.85, (n - g) / n, 5, .) = visited
FOLD_STOPS = {63: (85, 42, 100), 64: (67, 33, 100), 65: (57, 28, 101), 127: (58, 25, 100), 128: (79, 34, 102),
              129: (128, 55, 100), 1: (16, 15, 100), 2: (10, 9, 100)}
# (n, g, seed): num / denom with a fractional part >= 0.5 (rounds up) and < 0.5 (rounds down)
FOLD_ROUND = {"up": (13, 8, 101), "down": (12, 8, 100)}


def fold_stop(visited):
    n, g, seed = FOLD_STOPS[visited]
    Xw, uv, lab = crafted(n, g, seed)
    assert _update_py(0.85, (n - g) / n, 5, 500) == visited
    return Case(f"fold_stop_{visited}", Xw, uv, prop=dict(kind="fold", labels=lab, visited=visited, n_inliers=g,
                                                           ties=visited > 2))


def fold_round(which):
    n, g, seed = FOLD_ROUND[which]
    Xw, uv, lab = crafted(n, g, seed)
    q = update_quotient(0.85, (n - g) / n)
    frac = q - math.floor(q)
    assert (frac >= 0.5) == (which == "up") and frac != 0.5
    visited = _update_py(0.85, (n - g) / n, 5, 500)
    assert visited == (math.ceil(q) if which == "up" else math.floor(q))
    return Case(f"fold_round_{which}", Xw, uv, prop=dict(kind="fold", labels=lab, visited=visited, n_inliers=g,
                                                         ties=False, quotient=q))


ITERATION_WIDTHS = (0, 1, 63, 64, 65, 129)


def iteration_width(iterations):
    """One 700-point problem, half gross outliers, confidence 0.999: the
    estimate of RANSACUpdateNumIters stays above 129 (log 0.001 / log(1 - 2^-5)
    = 218 when every true point is counted), so `iterations` is what ends the
    loop. Hypothesis 0 draws five true points, so 0 and 1 iterations give a pose too."""
    Xw, uv, *_ = _problem(17, 700, 0.5)
    return Case(f"iterations_{iterations}", Xw, uv, iterations, 3.0, 0.999,
                prop=dict(kind="iterations", visited=max(iterations, 1)))


SMALL_N = {10: (6, 100), 12: (7, 100)}  # n -> (exact inliers, seed)


def small_n(n):
    """n = 10 / 12 at 4096 iterations: subsets of 5 out of so few redraw often,
    also against an index that is not the one drawn just before."""
    g, seed = SMALL_N[n]
    Xw, uv, lab = crafted(n, g, seed)
    return Case(f"small_{n}", Xw, uv, 4096, prop=dict(kind="small", labels=lab, n_inliers=g))


def _planar_points(seed, g, s):
    """g camera-frame points on the plane z = 3 + 0.2 x, moved off it by s * dz."""
    rng = np.random.default_rng(seed)
    Xc = np.c_[rng.uniform(-1.5, 1.5, g), rng.uniform(-1, 1, g), np.zeros(g)]
    Xc[:, 2] = 3.0 + 0.2 * Xc[:, 0] + s * rng.standard_normal(g)
    return Xc


def planar_edge(g, side, seed=71):
    """g exact near-planar inliers + 7 gross outliers whose scatter ratio
    w[2] / w[1] (float64, of the float32 landmarks) lies 0.5 % below ("planar")
    or above ("dlt") cvFindExtrinsicCameraParams2's 1e-3: the thickness is
    bisected on that ratio, so the two sides' thicknesses differ by < 1 %."""
    target = 1e-3 * (0.995 if side == "planar" else 1.005)
    Xo, uvo, cal, rv, t, _ = _problem(seed, g + 7, 0.0, noise=0.0)
    R = Rotation.from_rotvec(rv).as_matrix()

    def world(s):
        return ((_planar_points(seed + 1, g, s) - t) @ R).astype(np.float32)

    lo, hi = 0.0, 1.0
    for _ in range(60):
        s = 0.5 * (lo + hi)
        if scatter_ratio64(world(s)) < target:
            lo = s
        else:
            hi = s
    s = hi if side == "dlt" else lo
    Xw, uv = Xo.copy(), uvo.copy()
    Xw[:g] = world(s)
    uv[:g] = project64(np.r_[rv, t], Xw[:g], cal).astype(np.float32)
    _gross(uv, np.arange(g, g + 7), np.random.default_rng(seed + 2))
    lab = np.arange(g + 7) < g
    return Case(f"planar{g}_{side}", Xw, uv, 4096, prop=dict(kind="planar", labels=lab, n_inliers=g, side=side,
                                                             thickness=s, ok=(-1 if g == 5 and side == "dlt" else 1)))


def degenerate(which):
    cal = O.fr1_calib()
    if which == "identical":  # 40 times one observation: no 5-point model exists
        Xw = np.tile(np.float32([[0.1, 0.2, 3.0]]), (40, 1))
        uv = np.tile(np.float32([[320, 240]]), (40, 1))
        return Case("identical_40", Xw, uv, prop=dict(kind="degenerate", ok=0, visited=500))
    if which == "duplicates":  # 30 copies of one point among 40
        Xw, uv, *_ = _problem(9, 40, 0.0)
        Xw[:30] = Xw[0]
        uv[:30] = uv[0]
        return Case("duplicates_30_of_40", Xw, uv, prop=dict(kind="degenerate"))
    if which == "collinear":
        Xw, uv, *_ = _problem(9, 40, 0.0)
        Xw[:, 1] = 0
        Xw[:, 2] = 3
        return Case("collinear_40", Xw, uv, prop=dict(kind="degenerate"))
    if which == "behind":  # 10 of 60 landmarks 50 m behind the camera
        Xw, uv, *_ = _problem(10, 60, 0.0, noise=0.0)
        Xw[50:, 2] -= 50
        return Case("behind_10_of_60", Xw, uv, prop=dict(kind="degenerate"))
    if which == "four":  # the largest count is 4: nothing is accepted
        Xw, uv, lab = crafted(12, 4, 300)
        return Case("four_exact", Xw, uv, 4096, prop=dict(kind="degenerate", ok=0, best_iter=-1, max_good=4))
    raise KeyError(which)


def five_exact(seed):
    Xw, uv, _ = _five_inliers(seed)
    return Case(f"five_{seed}", Xw, uv, 4096, prop=dict(kind="five", n_inliers=5, ok=(1 if seed == 61 else -1)))


def reproj_case(which):
    """reproj_err is not validated (ptsetreg.cpp squares it into a float
    threshold and tests err <= t): NaN accepts nothing, 0 only an exact zero
    error, a negative value acts as its magnitude."""
    Xw, uv, lab = crafted(40, 30, 130, noise=0.5)
    val = {"nan": float("nan"), "zero": 0.0, "negative": -3.0}[which]
    return Case(f"reproj_{which}", Xw, uv, 500, val, 0.85, prop=dict(kind="reproj", which=which))


def nonfinite_case(which):
    """One non-finite landmark or observation among 40 (nothing checks the
    points): it is never an inlier and a hypothesis drawn on it counts nothing."""
    Xw, uv, lab = crafted(40, 30, 131, noise=0.5)
    Xw, uv = Xw.copy(), uv.copy()
    bad = int(subsets_py(40, 1)[0][0, 0])  # a member of the first hypothesis
    if which == "nan_xw":
        Xw[bad, 1] = np.nan
    elif which == "inf_xw":
        Xw[bad, 2] = np.inf
    elif which == "nan_uv":
        uv[bad, 0] = np.nan
    else:
        raise KeyError(which)
    return Case(f"nonfinite_{which}", Xw, uv, prop=dict(kind="nonfinite", bad=bad, labels=lab))


def single_cases():
    """Every single-problem case, by name."""
    cs = [point_width(n) for n in POINT_WIDTHS]
    cs += [inlier_width(c) for c in INLIER_WIDTHS]
    cs += [fold_stop(v) for v in FOLD_STOPS]
    cs += [fold_round(w) for w in FOLD_ROUND]
    cs += [iteration_width(i) for i in ITERATION_WIDTHS]
    cs += [small_n(n) for n in SMALL_N]
    cs += [planar_edge(g, side) for g in (5, 40) for side in ("planar", "dlt")]
    cs += [degenerate(w) for w in ("identical", "duplicates", "collinear", "behind", "four")]
    cs += [five_exact(s) for s in (60, 61, 62)]
    cs += [reproj_case(w) for w in ("nan", "zero", "negative")]
    cs += [nonfinite_case(w) for w in ("nan_xw", "inf_xw", "nan_uv")]
    return {c.name: c for c in cs}


# ---------------------------------------------------------------------- batches
def batch_many(nprob):
    """nprob problems of 12-20 points (500 iterations) with skipped (< 10
    points) problems at positions 0, 62, 63, 64 and last; position 0 is empty."""
    probs = []
    short = {0: 0, 62: 9, 63: 5, 64: 1, nprob - 1: 9 if nprob - 1 not in (63, 64) else (5 if nprob - 1 == 63 else 1)}
    for p in range(nprob):
        if p in short:
            Xw, uv, *_ = _problem(4000 + p, 9, 0.0)
            probs.append((Xw[:short[p]], uv[:short[p]]))
        else:
            n = 12 + p % 9
            Xw, uv, _ = crafted(n, n - 3 - p % 3, 4000 + p, noise=0.3)
            probs.append((Xw, uv))
    return probs, sorted(k for k in short if k < nprob)


# --------------------------------------------------------------- reference side
_REF = {}


def reference(case):
    """The oracle's result for a case (computed once per process), and for
    ok = 1 the float64 minimum on the oracle's inlier set with d = max |oracle
    rt - minimum|: the oracle's own distance, the only one a bound is built from."""
    if case.name not in _REF:
        cal = O.fr1_calib()
        r = O.pnp_ransac(case.Xw, case.uv, cal, case.iterations, case.reproj, case.conf)
        if r["ok"] == 1:
            m = r["mask"]
            r["rt64"] = minimum64(r["rt"], case.Xw[m], case.uv[m], cal)
            r["d"] = float(np.abs(r["rt64"] - r["rt"]).max())
        _REF[case.name] = r
    return _REF[case.name]


def bound64(ref):
    """4 d (the margin of pose_ref64.bound_vs_ref64) + CvLevMarq's own stop
    rule: a correct run may end once a step is below FLT_EPSILON relative."""
    return 4.0 * ref["d"] + FLT_EPSILON * float(np.abs(ref["rt64"]).max())
