"""tests/gicp_grid_ref.py (the grid neighbour searches of dense GICP, restated)
against the brute force of tests/gicp_ref64.py, on the CPU: the stop rule of the
ring search is proven here before a GPU sees it.

Every cloud at every cell (the new clouds and gicp_ref64's covariance cases,
but not scene4096 / scene4097, whose numpy ring search would take minutes: the
GPU test runs those against the brute-force kernel and the oracle): the ordered
20-neighbour lists are identical to gicp_ref64.knn20's. The 1-NN search is
held on the pairs in which the grid can differ from a scan (outside, half
outside, threshold, ties, a known motion, four correspondences), not on every
size of ICP_SIZES, which differ only in length. Every pair at every cell: the first-iteration
correspondences are identical to gicp_ref64.first_corr's on the source moved by
the guess, with the rows of a cell in sorted and in shuffled order. Each new
case is checked for the property it is named for, and a search that stops as
soon as it holds 20 points is shown to fail, so the cases can tell a wrong stop
rule from a right one.
"""
import numpy as np
import pytest

import gicp_grid_ref as R
import gicp_ref64 as G

CLOUDS = ["two_clusters", "face_lattice", "far"] + [n for n in G.COV_CASE_NAMES if n not in ("scene4096", "scene4097")]
EXTRA_CELLS = dict(two_clusters=(0.05,), face_lattice=(0.125,))


def cells_for(name):
    return R.COV_CELLS + EXTRA_CELLS.get(name, ())


def brute(name):
    return G.cached(("grid_knn", name), lambda: G.knn20(R.cloud(name)))


# ------------------------------------------------------------------ the cases
def test_two_clusters_cross_empty_rings():
    P = R.cloud("two_clusters")
    assert len(P) == 25 and P[10:, 0].min() - P[:10, 0].max() > 2.8
    nn = brute("two_clusters")
    assert all((nn[q] >= 10).any() for q in range(10)) and all((nn[q] < 10).any() for q in range(10, 25))
    g = R.build(P, 0.05)
    _, rings = R.knn20(g)
    assert rings.min() >= 55 and g["dims"][0] >= 60


def test_face_lattice_lies_on_faces_and_ties():
    P = R.cloud("face_lattice")
    for cell in (0.25, 0.125, 0.0625):
        g = R.plan(P, cell)
        t = (P - g["mn"]) * g["inv"]
        assert np.array_equal(t, np.floor(t))  # every coordinate on a face
    d = G.dist2_f32(P[0], P)
    assert np.count_nonzero(d == d[1]) >= 2 and not np.array_equal(R.cells_of(R.plan(P, 0.25), P[1:2]),
                                                                 R.cells_of(R.plan(P, 0.25), P[6:7]))


def test_far_is_long_and_its_fine_table_does_not_fit():
    P = R.cloud("far")
    e = P.max(axis=0) - P.min(axis=0)
    assert len(P) == 200 and e[2] > 90 * max(e[0], e[1])
    assert R.plan(P, 0.001) is None and R.plan(P, 0.0) is not None


def test_outside_pairs():
    S, T, g = R.pair("outside")
    assert R.outside_fraction(S, T, g, margin=0.07) == 1.0
    assert len(G.first_corr(R.apply_guess(S, g), T, 0.07)[0]) == 0
    S, T, g = R.pair("half_outside")
    assert 0.3 < R.outside_fraction(S, T, g, margin=0.07) < 0.7
    assert 20 <= len(G.first_corr(R.apply_guess(S, g), T, 0.07)[0]) < len(S)


def test_automatic_cell_rule():
    """Never below max_corr_dist, one ICP ring, and the table within its budget."""
    for name in CLOUDS:
        for mcd in (0.0, 0.05, 0.07, 0.25):
            g = R.plan(R.cloud(name), 0.0, mcd)
            assert g["w"] > mcd or max(g["dims"]) == 1
            assert g["rings"] == 1 and np.prod(g["dims"]) <= R.MAX_CELLS
    assert R.plan(G.lattice(), 0.05 / 3, 0.05)["rings"] == 4  # ceil(3 + slack)


def test_a_span_beyond_float_range_is_one_cell():
    """Finite coordinates whose difference overflows float32: the plan ends (one
    cell, every point in it), and a forced cell does not fit."""
    P = np.r_[R.cloud("two_clusters")[:13] - np.float32([3e38, 0, 0]),
              R.cloud("two_clusters")[13:] + np.float32([3e38, 0, 0])].astype(np.float32)
    assert np.all(np.isfinite(P))
    for mcd in (0.0, 0.05):
        g = R.plan(P, 0.0, mcd)
        assert g["dims"] == [1, 1, 1] and g["rings"] == 1
    assert R.plan(P, 0.25) is None and R.plan(P, 1e30) is None
    assert not R.cells_of(R.plan(P), P).any()
    # a huge but representable span still gets a grid
    Q = (R.cloud("two_clusters") * np.float32(1e37)).astype(np.float32)
    assert max(R.plan(Q)["dims"]) > 1
    with np.errstate(over="ignore"):
        assert np.array_equal(R.knn20(R.build(P))[0], G.knn20(P))


# ------------------------------------------------------------------ 20 neighbours
@pytest.mark.parametrize("name", CLOUDS)
def test_ring_search_equals_brute_force(name):
    P = R.cloud(name)
    want = brute(name)
    for cell in cells_for(name):
        nn, rings = R.knn20(R.build(P, cell))
        assert np.array_equal(nn, want), (name, cell)
    print(f"{name}: {len(P)} points, cells {cells_for(name)}")


def test_stopping_at_twenty_held_fails():
    """The cases can tell a wrong stop rule: without the bound the lists differ."""
    naive = lambda w, slack, r: np.inf
    bad = [name for name in ("scene300", "two_clusters", "face_lattice")
           if not np.array_equal(R.knn20(R.build(R.cloud(name), 0.0625), stop=naive)[0], brute(name))]
    assert "scene300" in bad


# ------------------------------------------------------------------ 1-NN
def icp_pairs():
    S, T, dist, _ = G.threshold_pair()
    return dict(outside=(*R.pair("outside"), 0.07), half_outside=(*R.pair("half_outside"), 0.07),
                threshold=(S, T, None, dist), tie=(*G.tie_pair(), None, 0.2),
                known=(*G.known_motion()[:2], None, 0.07), near4=(*G.near_far_pair(4), None, 0.07))


@pytest.mark.parametrize("name", sorted(icp_pairs()))
def test_correspondence_search_equals_brute_force(name):
    S, T, guess, mcd = icp_pairs()[name]
    moved = R.apply_guess(S, guess)
    si, ti = G.first_corr(moved, T, mcd)
    for cell in (0.0, mcd / 3, 10 * mcd):
        for shuffle in (None, np.random.default_rng(4)):
            gi, gt, g = R.first_corr(moved, T, mcd, cell, shuffle)
            assert np.array_equal(gi, si) and np.array_equal(gt, ti), (name, cell)
        assert g["rings"] == (1 if cell != mcd / 3 else 4) or max(g["dims"]) <= g["rings"], (name, cell, g["rings"])
