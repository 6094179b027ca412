"""The pose solvers against independent float64 references at edge shapes.

k_kabsch, k_pnp (through odo_kabsch / odo_pnp_motion_ba) and the RANSAC refit
on degenerate geometry (odo_ransac, and k_ransac_lanes through the batched
path). References: tests/pose_ref64.py (float64 numpy / scipy), checked on the
CPU by tests/test_pose_ref64.py, and the oracle.

Tolerances against a float64 reference are set per case inside the test
(pose_ref64.bound_vs_ref64): 4 x the oracle's own distance from the same
reference on the same input, at least 4 float32 ulps of the case's largest
magnitude; the 1e-4 bars against the oracle stay as absolute caps. RANSAC
results are compared by bit pattern, so a zero's sign counts.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import pose_ref64 as P
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

KABSCH_CASES = [("exact", n) for n in P.KABSCH_SIZES if n not in P.KABSCH_GEOMETRY_SIZES] + \
    [(g, n) for g in P.KABSCH_GEOMETRIES for n in P.KABSCH_GEOMETRY_SIZES]


@pytest.fixture(scope="module")
def ctx():
    """One context for the per-stage entry points of this module."""
    pkg = load_pkg()
    cfg = pkg.default_config(640, 480, 1, nfeatures=1000, iterations=200)
    odo = pkg.Odometry(cfg)
    yield pkg, odo, cfg
    odo.close()


# --------------------------------------------------------------------- Kabsch
@functools.lru_cache(maxsize=None)
def _kabsch_refs(geometry, n):
    A, B = P.kabsch_case(geometry, n)
    T64, info = P.kabsch64(A, B)
    K = np.zeros(16, np.float32)
    O.lib().oracle_kabsch(O.ptr(A), O.ptr(B), n, O.ptr(K))
    return A, B, T64, info, K.reshape(4, 4)


@pytest.mark.parametrize("geometry,n", KABSCH_CASES)
def test_kabsch_against_float64(geometry, n):
    """Where two singular values of the float64 M are significant the answer
    is unique: all 16 elements against the float64 result. Otherwise
    (collinear, identical, n < 3) any rotation about the remaining axis fits:
    the last row, orthonormality, det R = +1 and R cA + t = cB."""
    A, B, T64, info, K = _kabsch_refs(geometry, n)
    T = load_pkg().kabsch(A, B)
    assert T.dtype == np.float32 and T.shape == (4, 4)
    assert P.kabsch_is_unique(info) == (not P.kabsch_case_is_degenerate(geometry, n))
    if n == 0:
        assert T.tobytes() == np.eye(4, dtype=np.float32).tobytes()
        return
    T, K = T.astype(np.float64), K.astype(np.float64)
    assert np.array_equal(T[3], [0, 0, 0, 1])
    mag = max(np.abs(A).max(), np.abs(B).max(), np.abs(T64).max())
    R = T[:3, :3]
    cen = lambda X: np.abs(X[:3, :3] @ info["cA"] + X[:3, 3] - info["cB"]).max()
    if P.kabsch_is_unique(info):
        d_gpu, d_or = np.abs(T - T64).max(), np.abs(K - T64).max()
        bound = P.bound_vs_ref64(d_or, mag)
        print(f"kabsch {geometry} n={n}: |gpu - f64| {d_gpu:.3e} |oracle - f64| {d_or:.3e} bound {bound:.3e}")
        assert d_gpu <= bound
    else:
        # the oracle's R may be a reflection here; its centroid residual is still
        # what the reference's float arithmetic costs
        bound = P.bound_vs_ref64(cen(K), mag)
        print(f"kabsch {geometry} n={n}: centroid residual gpu {cen(T):.3e} oracle {cen(K):.3e} bound {bound:.3e}")
        # orthonormal to float32 rounding: R multiplies two factors, each the
        # product of up to ~10 Jacobi rotations that add an ulp or so apiece
        assert np.abs(R @ R.T - np.eye(3)).max() <= 32 * P.F32_EPS
        assert abs(np.linalg.det(R) - 1.0) <= 32 * P.F32_EPS, "a reflection"
        assert cen(T) <= bound


@pytest.mark.parametrize("geometry,n", [c for c in KABSCH_CASES if not P.kabsch_case_is_degenerate(*c)])
def test_kabsch_against_oracle(geometry, n):
    """The 1e-4 bar of test_kabsch_entry_point on every case whose data fix
    the answer. For collinear or identical points and n < 3 a rotation about
    the line stays open and each implementation returns what rounding left in
    its M (the oracle, restating kabsch.cpp, possibly a reflection): those
    cases are held to the properties in test_kabsch_against_float64 only."""
    A, B, T64, _, K = _kabsch_refs(geometry, n)
    T = load_pkg().kabsch(A, B)
    d, d_or = np.abs(T - K).max(), np.abs(K - T64).max()
    print(f"kabsch {geometry} n={n}: |gpu - oracle| {d:.3e} |oracle - f64| {d_or:.3e}")
    if d_or < 1e-4:
        assert d < 1e-4
    else:
        # the oracle's float running sums put its own centroids further than
        # the bar from the float64 result (a small cloud far out): a kernel
        # within the bar of it would be wrong by as much, so the kernel has to
        # be the closer of the two to float64 instead
        assert np.abs(T - T64).max() < d_or


# ------------------------------------------------------------------------ PnP
@functools.lru_cache(maxsize=None)
def _pnp_refs(name):
    c = P.pnp_case(name)
    n = c["n"]
    T = np.zeros(16, np.float32)
    out = np.zeros(max(n, 1), np.uint8)
    ni = O.lib().oracle_pnp(O.ptr(c["Xw"]), O.ptr(c["obs"]), n, C.byref(O.fr1_calib()), O.ptr(c["Tinit"].ravel()),
                            O.ptr(T), O.ptr(out))
    return c, T.reshape(4, 4), out[:n].astype(bool), ni


_PNP_GPU = {}


def _pnp_gpu(ctx, name):
    if name not in _PNP_GPU:
        pkg, odo, cfg = ctx
        c = _pnp_refs(name)[0]
        n = c["n"]
        T = np.zeros(16, np.float32)
        out = np.full(max(n, 1), 255, np.uint8)
        ni = C.c_int(-1)
        pkg.check(pkg.load().odo_pnp_motion_ba(odo.h, pkg.ptr(c["Xw"]), pkg.ptr(c["obs"]), n, pkg.ptr(cfg.calib),
                                               pkg.ptr(c["Tinit"].ravel()), pkg.ptr(T), pkg.ptr(out), C.byref(ni)))
        assert n == 0 or set(np.unique(out[:n])) <= {0, 1}
        _PNP_GPU[name] = (T.reshape(4, 4), out[:n].astype(bool), ni.value)
    return _PNP_GPU[name]


@pytest.mark.parametrize("name", P.PNP_CASES)
def test_pnp_against_oracle(ctx, name):
    """Pose within 1e-4 of the oracle's; flags equal except on edges whose
    float64 chi2 at the oracle's pose is within 2 % of 5.991 / 7.815, at most
    1 % of the case's edges; the inlier count is the flags'. With fewer than
    3 edges the pose is the initial pose bit for bit and every edge an inlier."""
    c, T_or, out_or, n_or = _pnp_refs(name)
    T, out, ni = _pnp_gpu(ctx, name)
    n = c["n"]
    if n < 3:
        # pnpsolver.cpp returns before optimising when it has fewer than 3
        # edges: the slots keep the inlier flag set at edge creation, while
        # the returned count is the early return's 0
        assert T.tobytes() == c["Tinit"].tobytes(), "pose differs from the initial pose"
        assert not out.any() and ni == n_or == 0
        return
    d = np.abs(T - T_or).max()
    diff = out != out_or
    print(f"pnp {name}: |gpu - oracle| {d:.3e}, inliers {ni} vs {n_or}, {diff.sum()} flags differ")
    assert d < 1e-4
    assert np.array_equal(T[3], [0, 0, 0, 1])
    assert ni == n - out.sum()
    if diff.any():
        near = P.pnp_near_threshold(T_or, c["Xw"], c["obs"])
        assert not (diff & ~near).any(), f"flags differ away from a threshold at edges {np.nonzero(diff & ~near)[0][:8]}"
        assert diff.sum() <= n // 100, f"{diff.sum()} flags differ, more than 1 % of {n}"
    else:
        assert ni == n_or


@pytest.mark.parametrize("name", [x for x in P.PNP_CASES if P.pnp_case_n(x) >= 10])
def test_pnp_against_float64_polish(ctx, name):
    """Independent of the oracle: scipy's float64 least squares over the
    returned inlier set, started at the returned pose, must not move it
    further than 4 x what it moves the oracle's pose over the oracle's set."""
    c, T_or, out_or, n_or = _pnp_refs(name)
    T, out, ni = _pnp_gpu(ctx, name)
    if n_or < 3:  # nothing to fit (the lost cases): the kernel has to say so too
        assert ni == n_or
        return
    assert ni >= 3
    mv_or = P.pnp_polish(T_or, c["Xw"], c["obs"], ~out_or)[1]
    mv = P.pnp_polish(T, c["Xw"], c["obs"], ~out)[1]
    bound = P.bound_vs_ref64(mv_or, np.abs(T_or).max())
    print(f"pnp {name}: polish moves gpu {mv:.3e} oracle {mv_or:.3e} bound {bound:.3e}")
    assert mv <= bound


# ------------------------------------------------- RANSAC, degenerate geometry
def _matches(m, keep=None):
    n = len(m["queryIdx"]) if keep is None else keep
    a = np.zeros(n, O.DMATCH_DTYPE)
    for f in ("queryIdx", "trainIdx", "distance"):
        a[f] = m[f][:n]
    return a


def _ransac_both(ctx, x1, x2, m, iters=200):
    """Two calls in a row through both implementations (the first sets the
    latch, the second starts from it and from the advanced rand() state)."""
    pkg, odo, _ = ctx
    r_ref, r_gpu = O.Rng(), pkg.Rng()
    O.lib().oracle_rng_seed(C.byref(r_ref), 4242)
    pkg.load().odo_rng_seed(pkg.ptr(r_gpu), 4242)
    lat_ref, lat_gpu = C.c_double(float("nan")), C.c_double(float("nan"))
    rp, rpg = O.ransac_params(iters), pkg.RansacParams(iters, 20, 3.0, 4, 1)
    gpu = functools.partial(pkg.load().odo_ransac, odo.h)
    res = []
    for call in range(2):
        ref = O.ransac_pair(O.lib().oracle_ransac, True, m, x1, x2, rp, r_ref, lat_ref)
        got = O.ransac_pair(gpu, False, m, x1, x2, rpg, r_gpu, lat_gpu)
        res.append((got, ref))
    return res


@pytest.mark.parametrize("corrupt", [0.0, 0.5])
@pytest.mark.parametrize("geometry", P.RANSAC_GEOMETRIES)
def test_ransac_degenerate_geometry_bits(ctx, geometry, corrupt):
    """odo_ransac == Ransac::Iterate by bit pattern on planar, depth-quantised,
    shared-coordinate, duplicated and collinear sets."""
    x1, x2, m = P.ransac_case(geometry, corrupt)
    for call, (got, ref) in enumerate(_ransac_both(ctx, x1, x2, _matches(m))):
        print(f"ransac {geometry} corrupt {corrupt} call {call}: ok {ref['ok']} visited {ref['visited']} "
              f"good {ref['n_good']} inliers {len(ref['inliers'])} rmse {ref['rmse']}")
        O.assert_ransac_bits(got, ref, f"{geometry} corrupt {corrupt} call {call}")


@pytest.mark.parametrize("n", [20, 19])
def test_ransac_at_min_inlier_th(ctx, n):
    """Exactly min_inlier_th (20) good matches, and one fewer (no sampling:
    identity, rmse 1e6, rand() state untouched)."""
    x1, x2, m = P.ransac_case("z_levels", 0.0)
    for call, (got, ref) in enumerate(_ransac_both(ctx, x1, x2, _matches(m, n))):
        O.assert_ransac_bits(got, ref, f"{n} matches call {call}")
        if n == 19:
            assert ref["ok"] == 0 and ref["visited"] == 0 and len(ref["inliers"]) == 0
        else:
            assert ref["visited"] >= 1


# scene, depth: the largest visited count the oracle reports among the 7 pairs
# (200 iterations, 1000 features, seed 0x5EED0040). The plain sequence with one
# depth closes every pair within the first launch's two hypotheses, so the hard
# sequence (noise, movers, repeated texture) runs as well: there every pair
# visits all 200 and refits with non-members on the lanes kernel.
LANES_CASES = {("plain", "const"): 2, ("plain", "levels"): 140, ("hard", "const"): 200, ("hard", "levels"): 200}


@pytest.mark.parametrize("scene,depth", list(LANES_CASES))
def test_ransac_lanes_degenerate_depth_bits(scene, depth):
    """k_ransac_lanes (the only caller of add_sel<true>) on a batch of 8
    frames at 320x240 whose depth images are one value (10 000: a
    fronto-parallel plane at 2 m) or multiples of 1250 (0.25 m levels): every
    pair against oracle_track_pair by bit pattern."""
    pkg = load_pkg()
    iters, nf = 200, 1000
    bgr, dep, _ = sequence(8, 320, 240, seed=0x5EED0040, hard=scene == "hard")
    d = np.full_like(dep, 10000) if depth == "const" else ((dep // 1250) * 1250).astype(dep.dtype)
    cal = O.fr1_calib()
    fr = [O.extract_frame(bgr[i], d[i], O.orb_params(nf), cal) for i in range(8)]
    cfg = pkg.default_config(320, 240, 8, nfeatures=nf, iterations=iters, forms={"ransac_lanes_min_open": 1})
    odo = pkg.Odometry(cfg)
    try:
        res = odo.track_batch_host(bgr, d)
        latch = float("nan")
        visited = []
        for p in range(1, 8):
            r, _, matches, latch = O.track_pair(fr[p - 1], fr[p], cal, O.ransac_params(iters),
                                                pkg.pair_seed(cfg.seed, p), latch)
            tag = f"{scene} {depth} pair {p}"
            g = odo.pair(p)
            assert np.array_equal(g["matches"], matches), f"{tag}: match list"
            assert (res[p]["n_matches"], res[p]["n_good"], res[p]["visited"], res[p]["n_inliers"],
                    res[p]["ransac_ok"]) == (r.n_matches, r.n_good, r.visited, r.n_inliers, r.ransac_ok), \
                f"{tag}: counts"
            assert (res[p]["n_sweeps"], res[p]["n_fit_points"]) == (r.n_sweeps, r.n_fit_points), f"{tag}: work counts"
            O.assert_same_bits(res[p]["T12"], r.T12, f"{tag}: T12")
            O.assert_same_bits(res[p]["rmse"], r.rmse, f"{tag}: rmse")
            O.check_ransac_inliers(g, r, tag)
            visited.append(r.visited)
        assert odo.latch == latch
        print(f"lanes {scene} {depth}: visited {visited}")
        assert max(visited) > 1 and max(visited) >= LANES_CASES[scene, depth]
    finally:
        odo.close()
