"""k_gicp_cov and k_gicp (k_gicp.hip) at the shapes where they can break.

Covariances, through odo_gicp_covariances (k_gicp_cov alone; the entry point
feeds every batch to the kernel as source AND as target and fails unless the
two sets come back bit-equal, so every call below also checks the kernel's
soffs / toffs and Cs / Ct selection): clouds at the edges of the 64-point
blocks, at GI_STAGE = 4096 (LDS-staged) and 4097 (the global-memory branch),
of exactly 20 points, lattices whose equal distances exercise "ties to the
lower index", and zero / rank-1 neighbourhoods. Each is checked
  (a) for symmetry (1e-15) and the spectrum (1e-3, 1, 1) (1e-9),
  (b) against the float64 reference of tests/gicp_ref64.py where the relative
      eigen-gap is >= 1e-2, within pose_ref64.bound_vs_ref64 of the oracle's own
      distance on that point,
  (c) against the oracle on every point, bit for bit: both sides are IEEE
      double with one operation order and the same Jacobi rotations.

The ICP loop, through odo_gicp / odo_gicp_batch against the oracle with
tests/test_gicp.py's assertions (converged, iterations, n_corr exact, T12
within 1e-5): source and target clouds of different lengths on both sides of
the 256-thread compaction chunks and of GI_STAGE, 19 points on one side only,
exactly 3 and 4 correspondences, a neighbour at exactly the distance
threshold, equal distances in the correspondence search, a known motion, and
ragged batches in which soffs != toffs from the first pair on.
"""
import numpy as np
import pytest

import gicp_ref64 as G
import oracle_lib as O
from conftest import load_pkg
from pose_ref64 import bound_vs_ref64

I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def odo():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(640, 480, 1))
    yield o
    o.close()


# ================================================================= covariances
def gpu_cov(odo, name):
    return G.cached(("gpu_cov", name), lambda: odo.gicp_covariances([G.case(name)])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.COV_CASE_NAMES)
def test_covariances(odo, name):
    Cg = gpu_cov(odo, name)
    Co = G.oracle_cov(name)
    C, gap, _, _ = G.ref_cov(name)
    assert Cg.shape == Co.shape and np.all(np.isfinite(Cg))
    # (a)
    np.testing.assert_allclose(Cg, Cg.transpose(0, 2, 1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.linalg.eigvalsh(Cg), np.tile([1e-3, 1.0, 1.0], (len(Cg), 1)), rtol=0, atol=1e-9)
    # (b)
    ok = gap >= G.GAP_MIN
    d_gpu = np.abs(Cg - C).max(axis=(1, 2))
    d_or = np.abs(Co - C).max(axis=(1, 2))
    bound = np.array([bound_vs_ref64(d, 1.0) for d in d_or])
    exact = np.array_equal(Cg, Co)
    print(f"{name}: n={len(Cg)} compared with float64: {ok.sum()} max |gpu - f64| "
          f"{d_gpu[ok].max() if ok.any() else 0:.3e} (oracle {d_or[ok].max() if ok.any() else 0:.3e}); "
          f"max |gpu - oracle| {np.abs(Cg - Co).max():.3e}; bit-equal to the oracle: {exact}")
    assert np.all(d_gpu[ok] <= bound[ok])
    # (c)
    assert exact


@pytest.mark.gpu
def test_covariances_ragged_batch(odo):
    """Every cloud under 1000 points, a 19-point and an empty cloud in one launch:
    rows equal the single calls bit for bit, the 19-point cloud gets zeros."""
    names = [n for n in G.COV_CASE_NAMES if len(G.case(n)) < 1000]
    assert len(names) == len(G.COV_CASE_NAMES) - 2
    clouds = [G.case(n) for n in names]
    clouds[2:2] = [G.scene(19), np.zeros((0, 3), np.float32)]
    out = odo.gicp_covariances(clouds)
    assert np.array_equal(out[2], np.zeros((19, 3, 3))) and out[3].shape == (0, 3, 3)
    for n, c in zip(names, out[:2] + out[4:]):
        assert np.array_equal(c, gpu_cov(odo, n)), n


@pytest.mark.gpu
def test_covariances_short_clouds_only(odo):
    """No cloud reaches 20 points: nothing is launched, the output is zeroed."""
    out = odo.gicp_covariances([G.scene(19), np.zeros((0, 3), np.float32), G.scene(1)])
    assert [o.shape[0] for o in out] == [19, 0, 1] and all(not o.any() for o in out)
    assert odo.gicp_covariances([]) == []


@pytest.mark.gpu
def test_covariances_argument_errors(odo):
    """Offsets are checked on the host before anything is queued (ODO_ERR_ARG = -1,
    ODO_ERR_CAPACITY = -3)."""
    lib, h = odo.lib, odo.h
    P = np.zeros((16385, 3), np.float32)
    Cv = np.zeros((16385, 9))

    def call(offs, n, cloud=P):
        o = np.asarray(offs, np.int32)      # kept alive across the call
        return lib.odo_gicp_covariances(h, None if cloud is None else cloud.ctypes.data, o.ctypes.data, n,
                                        Cv.ctypes.data)

    assert call([1, 30], 1) == -1          # does not start at 0
    assert call([0, 30, 25], 2) == -1      # decreases
    assert call([0, 16385], 1) == -3       # more than 16384 points in a cloud
    assert call([0, 30], 1, cloud=None) == -1   # points without a cloud
    assert call([0, 0], 1) == 0 and call([0], 0) == 0


# ================================================================= ICP loop
def single(odo, S, T, iters=10, dist=0.07, key=None):
    """odo_gicp on a pair against the oracle (tests/test_gicp.py's _check);
    returns (gpu result, oracle result), kept for the batch tests under key."""
    def run():
        ref = O.gicp(S, T, None, iters, dist)
        Tg, conv, it, nc = odo.gicp(S, T, None, iters, dist)
        return (Tg, conv, it, nc), ref
    (Tg, conv, it, nc), ref = G.cached(("icp", key, iters, dist), run) if key is not None else run()
    assert conv == ref["converged"]
    assert it == ref["iterations"]
    assert nc == ref["n_corr"]
    np.testing.assert_allclose(Tg, ref["T"], rtol=0, atol=1e-5)
    return (Tg, conv, it, nc), ref


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nt", G.ICP_SIZES)
def test_icp_unequal_sizes(odo, ns, nt):
    S, T = G.icp_pair(ns, nt)
    _, ref = single(odo, S, T, key=(ns, nt))
    assert ref["converged"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nt", [(19, 300), (300, 19), (0, 0)])
def test_icp_short_cloud_on_one_side(odo, ns, nt):
    S, T = G.icp_pair(ns, nt)
    (Tg, conv, it, nc), _ = single(odo, S, T, key=(ns, nt))
    assert (conv, it, nc) == (0, 0, 0) and np.array_equal(Tg, I4)


@pytest.mark.gpu
def test_icp_three_and_four_correspondences(odo):
    S, T = G.near_far_pair(3)
    (Tg, conv, it, nc), _ = single(odo, S, T, iters=1, key="near3")
    assert (conv, it, nc) == (0, 0, 3) and nc == len(G.first_corr(S, T, 0.07)[0])
    assert np.array_equal(Tg, I4)
    S, T = G.near_far_pair(4)
    (Tg, conv, it, nc), _ = single(odo, S, T, iters=1, key="near4")
    assert (conv, it, nc) == (1, 1, 4) and nc == len(G.first_corr(S, T, 0.07)[0])


@pytest.mark.gpu
def test_icp_threshold_is_strict(odo):
    S, T, dist, odd = G.threshold_pair()
    (_, conv, it, nc), _ = single(odo, S, T, iters=1, dist=dist, key="threshold")
    assert (conv, it) == (1, 1) and nc == len(G.first_corr(S, T, dist)[0]) == len(odd)


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 10])
def test_icp_equal_distances_go_to_the_lower_index(odo, iters):
    """tests/test_gicp_ref64.py shows that the pose of this pair depends on which
    of two equidistant target points a source point takes."""
    S, T = G.tie_pair()
    (_, conv, _, nc), _ = single(odo, S, T, iters=iters, dist=0.2, key="tie")
    assert conv == 1
    if iters == 1:
        assert nc == len(G.first_corr(S, T, 0.2)[0]) == len(S)


@pytest.mark.gpu
def test_icp_known_motion(odo):
    """Against the motion itself, not the oracle's pose: the device may be as far
    from it as bound_vs_ref64 allows given the oracle's own distance."""
    S, T, Tt = G.known_motion()
    (Tg, conv, _, nc), ref = single(odo, S, T, key="known")
    assert conv == 1 and nc == len(S)
    d_or = np.abs(ref["T"] - Tt).max()
    d_gpu = np.abs(Tg - Tt).max()
    print(f"known motion: |T_gpu - T_true| {d_gpu:.3e}, |T_oracle - T_true| {d_or:.3e}")
    assert d_gpu <= bound_vs_ref64(d_or, 1.0)


def batch_pairs():
    """(key, source, target): a long source with a short target first, then an
    early exit with ns < 20 <= nt, then an empty pair, then the rest: soffs and
    toffs differ from the first pair on."""
    sizes = [(300, 20), (19, 300), (0, 0)] + [s for s in G.ICP_SIZES if max(s) < 1000 and s != (300, 20)] + [(300, 19)]
    pairs = [(s, *G.icp_pair(*s)) for s in sizes]
    pairs += [("near3", *G.near_far_pair(3)), ("near4", *G.near_far_pair(4)), ("threshold", *G.threshold_pair()[:2]),
              ("tie", *G.tie_pair()), ("known", *G.known_motion()[:2])]
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [False, True], ids=["as_built", "roles_swapped"])
@pytest.mark.parametrize("iters,dist", [(10, 0.07), (1, 0.25)])
def test_icp_ragged_batch(odo, iters, dist, swap):
    """One odo_gicp_batch call over every pair under 1000 points (at (1, 0.25) the
    threshold pair and the equal distances are live): every pair equals its
    single call bit for bit, and the oracle as the single calls do."""
    pairs = [(("swapped", k), T, S) if swap else (k, S, T) for k, S, T in batch_pairs()]
    so = np.cumsum([len(S) for _, S, _ in pairs])
    to = np.cumsum([len(T) for _, _, T in pairs])
    assert so[0] != to[0] and np.count_nonzero(so != to) >= len(pairs) - 2
    out = odo.gicp_batch([(S, T, None) for _, S, T in pairs], iters, dist)
    assert len(out) == len(pairs)
    for (k, S, T), (Tb, conv, it, nc) in zip(pairs, out):
        (T1, conv1, it1, nc1), _ = single(odo, S, T, iters=iters, dist=dist, key=k)
        assert (conv, it, nc) == (conv1, it1, nc1), k
        assert np.array_equal(Tb, T1), k
