"""The float64 GICP reference (tests/gicp_ref64.py) against itself and the oracle
(oracle/gicp_ref.cpp), on the CPU. The cases are the ones
tests/test_gicp_edges_gpu.py runs on the device, so this file also shows that
each case sees the property it is there for: the lattice sees the tie rule of
the 20-nearest search, the midpoint pair sees the tie rule of the
correspondence search, the threshold pair sees the strict comparison, and the
share of points whose covariance the reference cannot pin (relative eigen-gap
under 1e-2) stays within its limits.
"""
import numpy as np
import pytest

import gicp_ref64 as G
import oracle_lib as O

SCENE_CASES = tuple(f"scene{n}" for n in G.SCENE_SIZES)


# ------------------------------------------------------------------ the reference alone
def test_prefiltered_knn_is_the_stable_sort():
    for name in ("lattice", "lattice_perm", "collinear_axis", "coincident", "scene65", "scene300"):
        P = G.case(name)
        assert np.array_equal(G.knn20(P), G.knn20_full(P)), name


def test_knn_ties_go_to_the_lower_index():
    assert np.array_equal(G.knn20(G.coincident()), np.tile(np.arange(20), (25, 1)))
    nn = G.knn20(G.collinear_axis())
    assert list(nn[12][:5]) == [12, 11, 13, 10, 14]      # equidistant pairs: left (lower) first
    assert list(nn[24][:3]) == [24, 23, 22] and list(nn[0][:3]) == [0, 1, 2]


@pytest.mark.parametrize("name", SCENE_CASES + G.EXACT_CASES)
def test_reference_spectrum_and_left_out_share(name):
    """C is symmetric with spectrum (1e-3, 1, 1); at most 5 % of a scene's points
    fall under the eigen-gap, none of a lattice's."""
    C, gap, _, _ = G.ref_cov(name)
    np.testing.assert_allclose(C, C.transpose(0, 2, 1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.linalg.eigvalsh(C), np.tile([1e-3, 1.0, 1.0], (len(C), 1)), rtol=0, atol=1e-12)
    out = np.mean(gap < G.GAP_MIN)
    print(f"{name}: {out:.4f} left out, smallest gap {gap.min():.4f}")
    assert out <= (0.0 if name in G.EXACT_CASES else 0.05)


@pytest.mark.parametrize("name", G.DEGENERATE_CASES)
def test_degenerate_cases_have_no_gap(name):
    assert np.all(G.ref_cov(name)[1] < G.GAP_MIN)


def test_neighbourhoods_of_a_20_point_cloud_are_the_cloud():
    C = G.ref_cov("scene20")[0]
    assert np.abs(C - C[0]).max() < 1e-12


def test_plane_lattice_normals():
    """Every neighbourhood of the three-plane lattice lies in its plane: C is
    diag with 1e-3 on the plane's normal, exactly."""
    C = G.ref_cov("planes")[0]
    for k, axis in enumerate((2, 0, 1)):
        d = np.ones(3)
        d[axis] = 1e-3
        np.testing.assert_allclose(C[36 * k:36 * (k + 1)], np.tile(np.diag(d), (36, 1, 1)), rtol=0, atol=1e-12)


def test_permuted_lattice_sees_the_tie_rule():
    """The same points in another order get other neighbourhoods where distances
    tie: rows differ by more than 1e-2 (a search without the lower-index rule
    cannot match both orders)."""
    p = G.lattice_perm()
    C0, C1 = G.ref_cov("lattice")[0], G.ref_cov("lattice_perm")[0]
    assert np.array_equal(G.case("lattice_perm"), G.case("lattice")[p])
    d = np.abs(C1 - C0[p]).max(axis=(1, 2))
    print(f"permuted lattice: {np.count_nonzero(d > 1e-2)} of {len(d)} rows differ, max {d.max():.3f}")
    assert np.count_nonzero(d > 1e-2) >= 1


# ------------------------------------------------------------------ the oracle's covariances
@pytest.mark.parametrize("name", G.COV_CASE_NAMES)
def test_oracle_covariances_against_float64(name):
    """Symmetry and spectrum as tests/test_gicp.py checks them, on every point;
    against float64 within gicp_ref64.oracle_bound wherever the gap is >= 1e-2."""
    Co = G.oracle_cov(name)
    C, gap, mag, w2 = G.ref_cov(name)
    assert np.all(np.isfinite(Co))
    np.testing.assert_allclose(Co, Co.transpose(0, 2, 1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.linalg.eigvalsh(Co), np.tile([1e-3, 1.0, 1.0], (len(Co), 1)), rtol=0, atol=1e-9)
    ok = gap >= G.GAP_MIN
    if name in G.DEGENERATE_CASES:
        assert not ok.any()
        return
    d = np.abs(Co - C).max(axis=(1, 2))[ok]
    b = G.oracle_bound(gap[ok], mag[ok], w2[ok])
    print(f"{name}: oracle - float64 max {d.max():.3e}, largest share of the bound {np.max(d / b):.3e}, "
          f"min gap {gap[ok].min():.4f}")
    assert np.all(d <= b)


def test_oracle_covariances_of_degenerate_clouds():
    """Zero and axis-aligned rank-1 covariances need no Jacobi rotation: V = I,
    C = diag(1, 1, 1e-3) exactly."""
    for name in ("coincident", "collinear_axis"):
        assert np.array_equal(G.oracle_cov(name), np.tile(np.diag([1.0, 1.0, 1e-3]), (25, 1, 1))), name


# ------------------------------------------------------------------ the oracle's first iteration
@pytest.mark.parametrize("ns,nt", G.ICP_SIZES)
def test_oracle_converges_on_the_size_pairs(ns, nt):
    S, T = G.icp_pair(ns, nt)
    r = O.gicp(S, T)
    assert r["converged"] == 1 and 1 <= r["iterations"] <= 10
    r1 = O.gicp(S, T, None, 1)
    assert r1["n_corr"] == len(G.first_corr(S, T, 0.07)[0]) >= 4


@pytest.mark.parametrize("ns,nt", [(19, 300), (300, 19)])
def test_oracle_early_exit_on_one_side(ns, nt):
    r = O.gicp(*G.icp_pair(ns, nt))
    assert (r["converged"], r["iterations"], r["n_corr"]) == (0, 0, 0)
    assert np.array_equal(r["T"], np.eye(4, dtype=np.float32))


def test_oracle_three_and_four_correspondences():
    S, T = G.near_far_pair(3)
    assert len(G.first_corr(S, T, 0.07)[0]) == 3
    r = O.gicp(S, T, None, 1)
    assert (r["converged"], r["iterations"], r["n_corr"]) == (0, 0, 3)
    assert np.array_equal(r["T"], np.eye(4, dtype=np.float32))
    S, T = G.near_far_pair(4)
    assert len(G.first_corr(S, T, 0.07)[0]) == 4
    r = O.gicp(S, T, None, 1)
    assert (r["converged"], r["iterations"], r["n_corr"]) == (1, 1, 4)


def test_oracle_threshold_is_strict():
    S, T, dist, odd = G.threshold_pair()
    d2 = np.array([G.dist2_f32(s, T)[i] for i, s in enumerate(S)])
    even = np.arange(0, len(S), 2)
    assert np.all(d2[even].astype(np.float64) == dist * dist) and np.all(d2[odd].astype(np.float64) < dist * dist)
    si, ti = G.first_corr(S, T, dist)
    assert np.array_equal(si, odd) and np.array_equal(ti, odd)
    r = O.gicp(S, T, None, 1, dist)
    assert (r["converged"], r["iterations"], r["n_corr"]) == (1, 1, len(odd))


def test_midpoint_pair_sees_the_correspondence_tie_rule():
    """Five source points have two nearest target points at equal float32
    distance, with covariances more than 1e-2 apart. The float64 minimisers of
    the first iteration's cost under the two tie rules differ by far more than
    the 1e-5 the pose is compared at, and the pose the oracle returns after one
    iteration is a stationary point of the lower-index cost only: BFGS stops at
    a gradient norm near 1e-2, and under the higher-index correspondences the
    gradient there is more than ten times that."""
    S, T = G.tie_pair()
    tied = G.tied_sources(S, T)
    assert list(tied) == [20, 21, 22, 23, 24]
    lo, hi = G.first_corr(S, T, 0.2), G.first_corr(S, T, 0.2, last=True)
    assert len(lo[0]) == len(hi[0]) == len(S)
    assert np.array_equal(np.flatnonzero(lo[1] != hi[1]), tied) and np.all(lo[1][tied] < hi[1][tied])
    Cs = G.covariances(S)
    Ct = G.ref_cov("lattice")
    assert Cs[1].min() >= G.GAP_MIN and Ct[1].min() >= G.GAP_MIN
    assert np.all(np.abs(Ct[0][lo[1]] - Ct[0][hi[1]]).max(axis=(1, 2))[tied] > 1e-2)
    f_lo = G.FirstIterationCost(S, T, *lo, Cs[0], Ct[0])
    f_hi = G.FirstIterationCost(S, T, *hi, Cs[0], Ct[0])
    assert np.abs(f_lo.optimum() - f_hi.optimum()).max() > 1e-3
    r = O.gicp(S, T, None, 1, 0.2)
    assert (r["converged"], r["iterations"], r["n_corr"]) == (1, 1, len(S))
    g_lo, g_hi = f_lo.grad_norm(r["T"]), f_hi.grad_norm(r["T"])
    print(f"gradient norm at the oracle's pose: {g_lo:.4f} (lower index), {g_hi:.4f} (higher index)")
    assert g_hi > 10 * 1e-2 and g_lo < g_hi / 10


def test_oracle_recovers_the_known_motion():
    S, T, Tt = G.known_motion()
    assert np.linalg.norm(T - S, axis=1).max() < 0.07
    r = O.gicp(S, T)
    assert r["converged"] == 1 and r["n_corr"] == len(S)
    print(f"known motion: |T_oracle - T_true| = {np.abs(r['T'] - Tt).max():.3e}")
    np.testing.assert_allclose(r["T"], Tt, rtol=0, atol=2e-3)   # as test_gicp.test_oracle_recovers_motion


def test_covariance_entry_point_rejects_a_null_context():
    """odo_gicp_covariances checks its arguments before any device call
    (ODO_ERR_ARG = -1), so this runs without a GPU."""
    from conftest import load_pkg
    lib = load_pkg().load()
    offs = np.int32([0, 20])
    assert lib.odo_gicp_covariances(None, None, offs.ctypes.data, 1, None) == -1
    assert lib.odo_last_error()
