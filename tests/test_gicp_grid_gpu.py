"""The grid neighbour searches of k_gicp.hip (odo_gicp_grid_covariances,
odo_gicp_grid_batch) against the brute-force kernels and the oracle.

The grid search must return exactly what the brute-force scans return, so
everything is compared bit for bit: covariances with odo_gicp_covariances AND
the oracle, ICP results (T12, converged, iterations, n_corr) with
odo_gicp_batch, plus tests/test_gicp.py's assertions against the oracle
(flags, iterations, n_corr exact, T12 within 1e-5). Cells: the automatic one, and
forced ones below the point spacing, at it, far above it and one cell for the
whole cloud; for the ICP search a third of max_corr_dist (4 rings) and ten
times it. The clouds are tests/test_gicp_edges_gpu.py's plus those of
tests/gicp_grid_ref.py (tests/test_gicp_grid_ref.py checks on the CPU what each
is named for), and one pair above the brute-force path's 16384 points, which
only the oracle can judge.
"""
import ctypes as C

import numpy as np
import pytest

import gicp_grid_ref as R
import gicp_ref64 as G
import oracle_lib as O
from conftest import load_pkg
from pose_ref64 import bound_vs_ref64
from test_gicp_edges_gpu import batch_pairs

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
ERR_ARG, ERR_CAPACITY = -1, -3
COV_NAMES = G.COV_CASE_NAMES + tuple(R.NEW_CLOUDS)
BIG = ("scene4096", "scene4097")


@pytest.fixture(scope="module")
def odo():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(640, 480, 1))
    yield o
    o.close()


# ================================================================= covariances
def brute_cov(odo, name):
    return G.cached(("gpu_cov", name), lambda: odo.gicp_covariances([R.cloud(name)])[0])


def oracle_cov(name):
    return G.cached(("oracle", name), lambda: O.gicp_covariances(R.cloud(name)))


@pytest.mark.parametrize("name", COV_NAMES)
def test_covariances(odo, name):
    P = R.cloud(name)
    for cell in ((0.0, 0.25) if name in BIG else R.COV_CELLS):
        Cg = odo.gicp_grid_covariances([P], cell)[0]
        assert Cg.shape == (len(P), 3, 3) and np.all(np.isfinite(Cg))
        assert np.array_equal(Cg, oracle_cov(name)), (name, cell, "oracle")
        assert np.array_equal(Cg, brute_cov(odo, name)), (name, cell, "brute force")


def test_covariances_ragged_batch(odo):
    names = [n for n in COV_NAMES if n not in BIG]
    clouds = [R.cloud(n) for n in names]
    clouds[2:2] = [G.scene(19), np.zeros((0, 3), np.float32)]
    for cell in (0.0, 0.25):
        out = odo.gicp_grid_covariances(clouds, cell)
        assert np.array_equal(out[2], np.zeros((19, 3, 3))) and out[3].shape == (0, 3, 3)
        for n, c in zip(names, out[:2] + out[4:]):
            assert np.array_equal(c, odo.gicp_grid_covariances([R.cloud(n)], cell)[0]), (n, cell)
            assert np.array_equal(c, brute_cov(odo, n)), (n, cell)


def test_covariances_short_clouds_only(odo):
    out = odo.gicp_grid_covariances([G.scene(19), np.zeros((0, 3), np.float32), G.scene(1)])
    assert [o.shape[0] for o in out] == [19, 0, 1] and all(not o.any() for o in out)
    assert odo.gicp_grid_covariances([]) == []


# ================================================================= ICP loop
def icp_cases():
    """key -> (source, target, guess, iterations, max_corr_dist)."""
    c = {s: (*G.icp_pair(*s), None, 10, 0.07) for s in G.ICP_SIZES + ((19, 300), (300, 19), (0, 0))}
    S, T, dist, _ = G.threshold_pair()
    c["threshold"] = (S, T, None, 1, dist)
    c["tie1"] = (*G.tie_pair(), None, 1, 0.2)
    c["tie10"] = (*G.tie_pair(), None, 10, 0.2)
    c["near3"] = (*G.near_far_pair(3), None, 1, 0.07)
    c["near4"] = (*G.near_far_pair(4), None, 1, 0.07)
    c["known"] = (*G.known_motion()[:2], None, 10, 0.07)
    c["outside"] = (*R.pair("outside"), 10, 0.07)
    c["half_outside"] = (*R.pair("half_outside"), 10, 0.07)
    return c


ICP = icp_cases()


def brute_and_oracle(odo, key):
    S, T, g, iters, dist = ICP[key]
    return G.cached(("grid_icp", key), lambda: (odo.gicp(S, T, g, iters, dist), O.gicp(S, T, g, iters, dist)))


def check(res, brute, ref, what):
    Tg, conv, it, nc = res
    assert (conv, it, nc) == brute[1:], what
    assert np.array_equal(Tg, brute[0]), what
    assert (conv, it, nc) == (ref["converged"], ref["iterations"], ref["n_corr"]), what
    np.testing.assert_allclose(Tg, ref["T"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("key", list(ICP), ids=[str(k) for k in ICP])
def test_icp(odo, key):
    S, T, g, iters, dist = ICP[key]
    brute, ref = brute_and_oracle(odo, key)
    for cell in (0.0, dist / 3, 10 * dist):
        res = odo.gicp_grid_batch([(S, T, g)], iters, dist, cell)[0]
        check(res, brute, ref, (key, cell))
    Tg, conv, it, nc = res
    if key in ((19, 300), (300, 19), (0, 0)):
        assert (conv, it, nc) == (0, 0, 0) and np.array_equal(Tg, I4)
    elif key == "outside":
        assert (conv, it, nc) == (0, 0, 0) and np.array_equal(Tg, I4)
    elif key == "near3":
        assert (conv, it, nc) == (0, 0, 3) and np.array_equal(Tg, I4)
    elif key == "near4":
        assert (conv, it, nc) == (1, 1, 4)
    elif key == "threshold":
        assert (conv, it) == (1, 1) and nc == len(G.first_corr(S, T, dist)[0]) == len(G.threshold_pair()[3])
    elif key == "tie1":
        assert conv == 1 and nc == len(G.first_corr(S, T, dist)[0]) == len(S)
    elif key == "half_outside":
        assert conv == 1 and 20 <= nc < len(S)
    elif key == "known":
        Tt = G.known_motion()[2]
        d_or, d_gpu = np.abs(ref["T"] - Tt).max(), np.abs(Tg - Tt).max()
        print(f"known motion: |T_gpu - T_true| {d_gpu:.3e}, |T_oracle - T_true| {d_or:.3e}")
        assert conv == 1 and nc == len(S) and d_gpu <= bound_vs_ref64(d_or, 1.0)
    else:
        assert conv == 1


@pytest.mark.parametrize("swap", [False, True], ids=["as_built", "roles_swapped"])
@pytest.mark.parametrize("iters,dist", [(10, 0.07), (1, 0.25)])
def test_icp_ragged_batch(odo, iters, dist, swap):
    """tests/test_gicp_edges_gpu.py's ragged batch in one odo_gicp_grid_batch call:
    every pair equals its single grid call and its brute-force call bit for bit."""
    pairs = [(T, S) if swap else (S, T) for _, S, T in batch_pairs()]
    pairs += [R.pair("half_outside")[:2], R.pair("outside")[:2]]
    guesses = [None] * (len(pairs) - 2) + [R.pair("half_outside")[2], R.pair("outside")[2]]
    batch = [(S, T, g) for (S, T), g in zip(pairs, guesses)]
    out = odo.gicp_grid_batch(batch, iters, dist)
    brute = odo.gicp_batch(batch, iters, dist)
    assert len(out) == len(batch)
    for k, (b, res, br) in enumerate(zip(batch, out, brute)):
        one = odo.gicp_grid_batch([b], iters, dist)[0]
        assert res[1:] == one[1:] == br[1:], k
        assert np.array_equal(res[0], one[0]) and np.array_equal(res[0], br[0]), k


def test_above_the_brute_force_capacity(odo):
    """16385 points on both sides: odo_gicp_batch refuses them, the oracle judges."""
    from test_gicp import _scene
    P, Q, _ = _scene(41, n=16385)
    with pytest.raises(Exception):
        odo.gicp_batch([(P, Q, None)], 2, 0.07)
    ref = G.cached(("grid_icp", "big"), lambda: O.gicp(P, Q, None, 2, 0.07))
    Tg, conv, it, nc = odo.gicp_grid_batch([(P, Q, None)], 2, 0.07)[0]
    print(f"16385 points: converged {conv}, iterations {it}, n_corr {nc}")
    assert (conv, it, nc) == (ref["converged"], ref["iterations"], ref["n_corr"]) and it == 2 and nc > 1000
    np.testing.assert_allclose(Tg, ref["T"], rtol=0, atol=1e-5)


def test_blocks_regrow_and_results_repeat():
    """A fresh context: a pair of 20-point clouds, a pair of 300-point clouds
    three times as wide, the 20-point pair again, all at one forced cell of
    0.25. The point-sized block is sized by the points of a call (40, then 600),
    the cell-sized block by its cells: the wide clouds hold the small ones'
    points scaled by 3, so no axis of theirs has fewer cells and the table is
    larger. Both blocks regrow. The small results are identical, and the large
    one equals the same call on another fresh context."""
    pkg = load_pkg()
    small = (*G.icp_pair(20, 20), None)
    wide = np.ascontiguousarray(G.scene(300) * np.float32(3))
    large = (wide, G.shifted(wide), None)
    ext = lambda P: P.max(0) - P.min(0)
    assert np.all(np.floor(ext(wide) / 0.25) > np.floor(ext(small[0]) / 0.25))

    def call(o, pair):
        T, conv, it, nc = o.gicp_grid_batch([pair], 10, 0.07, 0.25)[0]
        return T.tobytes(), conv, it, nc

    one, two = (pkg.Odometry(pkg.default_config(640, 480, 1)) for _ in range(2))
    try:
        a = call(one, small)
        b = call(one, large)
        assert call(one, small) == a
        assert call(two, large) == b
        assert a[1] == 1 and b[3] > 0
    finally:
        one.close()
        two.close()


# ================================================================= arguments
def test_far_cloud_and_the_table_budget(odo):
    P = R.cloud("far")
    offs = np.array([0, len(P)], np.int32)
    Cv = np.full((len(P), 9), 7.0)
    lib = odo.lib
    assert lib.odo_gicp_grid_covariances(odo.h, P.ctypes.data, offs.ctypes.data, 1, 0.001, Cv.ctypes.data) == ERR_CAPACITY
    assert np.all(Cv == 7.0)
    assert np.array_equal(odo.gicp_grid_covariances([P], 0.0)[0], oracle_cov("far"))
    T, io = np.full(16, 7.0, np.float32), np.full(3, 7, np.int32)
    g = I4.copy()
    rc = lib.odo_gicp_grid_batch(odo.h, P.ctypes.data, offs.ctypes.data, P.ctypes.data, offs.ctypes.data, g.ctypes.data,
                                 1, 5, 0.07, 0.001, T.ctypes.data, io[0:].ctypes.data, io[1:].ctypes.data,
                                 io[2:].ctypes.data)
    assert rc == ERR_CAPACITY and np.all(T == 7.0) and np.all(io == 7)


def test_argument_errors_write_nothing(odo):
    lib, h = odo.lib, odo.h
    S, Tt = np.ascontiguousarray(G.scene(30)), np.ascontiguousarray(G.shifted(G.scene(40)))
    T, io = np.full(16, 7.0, np.float32), np.full(3, 7, np.int32)
    Cv = np.full((40, 9), 7.0)
    ok = dict(src=S, so=[0, 30], tgt=Tt, to=[0, 40], g=I4.copy(), n=1, it=5, dist=0.07, cell=0.0, T=T)

    def batch(**kw):
        a = {**ok, **kw}
        so, to = np.asarray(a["so"], np.int32), np.asarray(a["to"], np.int32)   # kept alive across the call
        p = lambda x: None if x is None else x.ctypes.data
        return lib.odo_gicp_grid_batch(h, p(a["src"]), so.ctypes.data, p(a["tgt"]), to.ctypes.data, p(a["g"]), a["n"],
                                       a["it"], a["dist"], a["cell"], p(a["T"]), io[0:].ctypes.data, io[1:].ctypes.data,
                                       io[2:].ctypes.data)

    def cov(offs, n, cloud=Tt, cell=0.0, out=Cv):
        o = np.asarray(offs, np.int32)
        return lib.odo_gicp_grid_covariances(h, None if cloud is None else cloud.ctypes.data, o.ctypes.data, n, cell,
                                             None if out is None else out.ctypes.data)

    nan_g = I4.copy()
    nan_g[1, 3] = np.nan
    nan_s = S.copy()
    nan_s[7, 2] = np.inf
    big = np.zeros((1048577, 3), np.float32)
    for kw in (dict(src=None), dict(tgt=None), dict(T=None), dict(so=[1, 30]), dict(to=[0, 40, 30], so=[0, 30, 30], n=2),
               dict(it=0), dict(dist=-0.07), dict(dist=float("nan")), dict(dist=float("inf")), dict(cell=-1.0),
               dict(cell=float("nan")), dict(cell=float("inf")), dict(g=nan_g), dict(src=nan_s), dict(n=-1)):
        assert batch(**kw) == ERR_ARG, kw
        assert lib.odo_last_error()
    assert batch(src=big, so=[0, 1048577]) == ERR_CAPACITY
    assert np.all(T == 7.0) and np.all(io == 7)
    assert batch(n=0) == 0 and np.all(T == 7.0)
    assert batch() == 0 and io[0] == 1 and T[15] == 1.0
    nan_t = Tt.copy()
    nan_t[3, 0] = np.nan
    assert cov([1, 40], 1) == ERR_ARG and cov([0, 40, 30], 2) == ERR_ARG and cov([0, 40], 1, cloud=None) == ERR_ARG
    assert cov([0, 40], 1, out=None) == ERR_ARG and cov([0, 40], -1) == ERR_ARG and cov([0, 40], 1, cloud=nan_t) == ERR_ARG
    assert cov([0, 40], 1, cell=-0.5) == ERR_ARG and cov([0, 40], 1, cell=float("nan")) == ERR_ARG
    assert cov([0, 1048577], 1, cloud=big) == ERR_CAPACITY
    assert np.all(Cv == 7.0)
    assert cov([0, 0], 1) == 0 and cov([0], 0) == 0 and np.all(Cv == 7.0)
    assert cov([0, 40], 1) == 0 and np.array_equal(Cv.reshape(-1, 3, 3), odo.gicp_covariances([Tt])[0])
