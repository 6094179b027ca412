"""tests/sor_ref.py on the CPU: the float32 restatement against an independent
float64 brute force, and every crafted case against the property it is named
for. In particular no point of any case lies within threshold_bound of the
threshold, so tests/test_sor_gpu.py may require the keep mask exactly: that is
a condition on the inputs, checked here, not a tolerance on the kernel.
"""
import numpy as np
import pytest

import gicp_grid_ref as R
import sor_ref as S

F32_EPS = 2.0 ** -24


def brute64(P, mean_k, mul):
    """All in float64 and from the definition: full sort, np.sum."""
    P = np.asarray(P, np.float64)
    D = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    D.sort(axis=1)
    dist = D[:, 1:mean_k + 1].mean(axis=1)
    mean, sd = dist.mean(), dist.std(ddof=1)
    return dist, mean, sd, mean + mul * sd


@pytest.mark.parametrize("name", list(S.cases()))
def test_reference_against_float64(name):
    P, k, mul = S.case(name)
    r = S.ref(name)
    assert r["n_in"] == len(P) and r["n_out"] == int(r["keep"].sum())
    if len(P) <= k:
        assert r["status"] == S.SOR_SKIPPED and r["keep"].all() and not r["distances"].any()
        return
    dist, mean, sd, thr = brute64(P, k, mul)
    # a float squared distance: 5 roundings on coordinates of magnitude <= M; its root, the mean's cast
    M = float(np.abs(P).max()) * 2
    err = 16 * F32_EPS * np.maximum(dist, np.sqrt(F32_EPS) * M) + 1e-30
    assert np.all(np.abs(r["distances"] - dist) <= err), name
    e = float(err.max())
    assert abs(r["mean"] - mean) <= e
    if name != "negative_variance":
        assert abs(r["stddev"] - sd) <= 4 * np.sqrt(e * max(sd, e)) + 4 * e
        # the mask agrees wherever float64 puts the point clear of the threshold
        clear = np.abs(dist - thr) > 8 * np.sqrt(e * max(sd, e)) + 8 * e
        assert np.array_equal(r["keep"][clear], ~(dist > thr)[clear])
        assert clear.mean() > 0.9 or not dist.any()


@pytest.mark.parametrize("name", list(S.cases()))
def test_no_point_within_the_bound_of_the_threshold(name):
    r = S.ref(name)
    b = S.threshold_bound(r)
    assert S.margin_ok(r), (name, r["threshold"], b)
    assert b["nan_expected"] == (name == "negative_variance")
    if r["status"] == S.SOR_OK and not b["nan_expected"] and r["threshold"] != 0:
        assert b["threshold"] <= 1e-9 * abs(r["threshold"]), "the bound is about n 2^-52, relative"


def test_batch_margin():
    clouds, k, mul = S.mixed_batch()
    refs = [S.sor(P, k, mul) for P in clouds]
    assert [r["status"] for r in refs] == [0, 1, 1, 0, 0, 0]
    assert all(S.margin_ok(r) for r in refs)
    assert refs[-1]["n_out"] < refs[-1]["n_in"]


def test_named_properties():
    c = S.cases()
    assert S.ref("n_eq_k_skipped")["status"] == S.SOR_SKIPPED
    P, k, _ = c["n_eq_k_plus_1"]
    assert len(P) == k + 1 and S.ref("n_eq_k_plus_1")["status"] == S.SOR_OK
    assert S.MAX_K >= 64 and c[f"scene300_k{S.MAX_K}"][1] == S.MAX_K
    for name in ("coincident", "two_sites_large"):
        r = S.ref(name)
        assert not r["distances"].any() and r["threshold"] == 0.0 and r["keep"].all(), name
    r = S.ref("two_sites_small")
    P, k, _ = c["two_sites_small"]
    assert np.all(r["distances"] > 1.0) and 0 < r["n_out"] < len(P)
    # at the tiny forced cell the two sites are hundreds of cells apart, all of them empty
    g = R.build(P, S.cells_for(P, "two_sites_small")[1])
    assert g["dims"][0] >= 200 and len(np.unique(g["keys"])) == 2
    # the lattice: many distances equal to the (mean_k + 1)-th
    P, k, _ = c["lattice"]
    import gicp_ref64 as G
    ties = [np.count_nonzero(np.sort(G.dist2_f32(p, P))[k] == G.dist2_f32(p, P)) for p in P]
    assert min(ties) >= 2
    for name, ones in (("line", 2), ("plane", 1)):
        P = c[name][0]
        assert sorted(R.build(P, S.cells_for(P)[2])["dims"]).count(1) == ones, name
    r = S.ref("blob_outlier")
    assert r["n_out"] == r["n_in"] - 1 and not r["keep"][-1] and r["keep"][:-1].all()
    P = c["blob_outlier"][0]
    assert len(np.unique(R.build(P, S.cells_for(P)[1])["keys"])) <= 9
    assert S.ref("mul_zero")["n_out"] < S.ref("mul_large")["n_out"] == 300
    assert S.ref("mul_negative")["n_out"] < S.ref("mul_zero")["n_out"]
    r = S.ref("negative_variance")
    b = S.threshold_bound(r)
    assert r["var"] < -b["var"] < 0 and np.isnan(r["threshold"]) and r["keep"].all()
    assert len(set(r["distances"].tolist())) == 1


@pytest.mark.parametrize("name", list(S.fitness_cases()))
def test_fitness_reference(name):
    src, tgt, T = S.fitness_cases()[name]
    score, nn = S.fitness(src, tgt, T)
    if name.startswith("empty"):
        assert score == S.DBL_MAX
        return
    m = R.apply_guess(src, T).astype(np.float64)
    d = ((m[:, None, :] - np.asarray(tgt, np.float64)[None]) ** 2).sum(-1).min(1)
    Mx = max(float(np.abs(m).max()), float(np.abs(tgt).max())) * 2
    assert np.all(np.abs(nn - d) <= 16 * F32_EPS * np.maximum(d, F32_EPS * Mx * Mx))
    assert abs(score - d.mean()) <= 16 * F32_EPS * max(d.mean(), F32_EPS * Mx * Mx)
    if name == "coincident":
        assert score == 0.0
    if name.startswith("outside"):
        assert R.outside_fraction(src, tgt, T, margin=10.0) == 1.0
    if name == "half_outside":
        assert 0.3 < R.outside_fraction(src, tgt, T, margin=0.07) < 0.7
