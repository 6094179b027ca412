"""odo_ransac and hypotheses mode share one set-up of the pair (depth filter,
sort, capacity check, DepthCovariance latch). At the gates where that set-up
branches, odo_ransac and odo_ransac_hyps over [0, iterations) + the fold +
odo_ransac_hyps_finish must agree bit for bit: T12, rmse, ok, the inlier list,
the rand() state and the latch.

min_inlier_th = 20, 64 iterations, check_depth on. Match counts 0 / 19 / 20 /
21 around the first gate; 40 matches of which 21 (20) fail the depth filter,
which leaves 19 (20) around the second. Each with the latch passed in as NaN,
preset, and NaN with every source z == 0 (nothing to latch from: it stays NaN).
"""
import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg
from test_hyp_shard import _problem

pytestmark = pytest.mark.gpu

ITERS, MIN_INL = 64, 20
PRESET = 1.5e-3


@pytest.fixture(scope="module")
def base():
    """40 matches with a valid depth on both sides, every keypoint in one match only."""
    pkg = load_pkg()
    m, x1, x2, _ = _problem(0.0, ITERS)
    x1, x2 = np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)
    z1, z2 = x1[m["queryIdx"], 2], x2[m["trainIdx"], 2]
    keep = (z1 > 0) & (z2 > 0)
    _, first_q = np.unique(m["queryIdx"], return_index=True)
    _, first_t = np.unique(m["trainIdx"], return_index=True)
    once = np.zeros(m.size, bool)
    once[np.intersect1d(first_q, first_t)] = True
    m = np.ascontiguousarray(m[keep & once][:40])
    assert m.size == 40
    odo = pkg.Odometry(pkg.default_config(640, 480, 1, nfeatures=1000, iterations=ITERS))
    yield pkg, odo, m, x1, x2
    odo.close()


def _spoil(m, x1, x2, k):
    """The first k matches fail the depth filter: NaN or non-positive z on one side."""
    x1, x2 = x1.copy(), x2.copy()
    bad = [np.nan, 0.0, -1.0]
    for i in range(k):
        side, idx = (x1, m["queryIdx"][i]) if i % 2 == 0 else (x2, m["trainIdx"][i])
        side[idx, 2] = bad[i % 3]
    return x1, x2


def _case(name, m, x1, x2):
    """-> matches, xyz1, xyz2, good matches after the filter"""
    if name.startswith("n"):
        k = int(name[1:])
        return np.ascontiguousarray(m[:k]), x1, x2, k
    k = {"filter_leaves_19": 21, "filter_leaves_20": 20}[name]
    return (m,) + _spoil(m, x1, x2, k) + (40 - k,)


def _iterate(pkg, odo, m, x1, x2, latch):
    lib = pkg.load()
    rng = pkg.Rng()
    lib.odo_rng_seed(pkg.ptr(rng), 99)
    lat = O.C.c_double(latch)
    T = np.zeros(16, np.float32)
    rmse, ni, ok = O.C.c_float(0), O.C.c_int(0), O.C.c_int(0)
    inl = np.zeros(max(m.size, 1), pkg.DMATCH_DTYPE)
    rc = lib.odo_ransac(odo.h, pkg.ptr(m), m.size, pkg.ptr(x1), x1.shape[0], pkg.ptr(x2), x2.shape[0],
                        pkg.ptr(pkg.RansacParams(ITERS, MIN_INL, 3.0, 4, 1)), pkg.ptr(rng), O.C.byref(lat), pkg.ptr(T),
                        O.C.byref(rmse), pkg.ptr(inl), O.C.byref(ni), O.C.byref(ok))
    return rc, dict(T=T.tobytes(), rmse=np.float32(rmse.value).tobytes(), ok=ok.value, inliers=inl[:ni.value].tobytes(),
                    rng=bytes(rng), latch=np.float64(lat.value).tobytes())


def _hypotheses(pkg, odo, m, x1, x2, latch):
    from arlm_amd import hyp_shard
    lib = pkg.load()
    params = pkg.RansacParams(ITERS, MIN_INL, 3.0, 4, 1)
    rng = pkg.Rng()
    lib.odo_rng_seed(pkg.ptr(rng), 99)
    lat = O.C.c_double(latch)
    allh = np.zeros(ITERS, pkg._abi.HYP_DTYPE)
    ng = O.C.c_int(-1)
    rc = lib.odo_ransac_hyps(odo.h, pkg.ptr(m), m.size, pkg.ptr(x1), x1.shape[0], pkg.ptr(x2), x2.shape[0],
                             pkg.ptr(params), pkg.ptr(rng), O.C.byref(lat), 0, ITERS, pkg.ptr(allh), O.C.byref(ng))
    if rc:
        return rc, None, ng.value
    fr = hyp_shard.fold(allh, ng.value, params)
    T = np.zeros(16, np.float32)
    rmse, ni, ok, own = O.C.c_float(0), O.C.c_int(0), O.C.c_int(0), O.C.c_int(0)
    inl = np.zeros(max(m.size, 1), pkg.DMATCH_DTYPE)
    pkg.check(lib.odo_ransac_hyps_finish(odo.h, pkg.ptr(fr), pkg.ptr(rng), pkg.ptr(T), O.C.byref(rmse), pkg.ptr(inl),
                                         O.C.byref(ni), O.C.byref(ok), O.C.byref(own)))
    assert own.value == 1, "the only rank owns the result"
    return 0, dict(T=T.tobytes(), rmse=np.float32(rmse.value).tobytes(), ok=ok.value, inliers=inl[:ni.value].tobytes(),
                   rng=bytes(rng), latch=np.float64(lat.value).tobytes()), ng.value


@pytest.mark.parametrize("latch", ["nan", "preset", "nan_source_z0"])
@pytest.mark.parametrize("name", ["n0", "n19", "n20", "n21", "filter_leaves_19", "filter_leaves_20"])
def test_iterate_and_hypotheses_agree_at_the_gates(base, name, latch):
    pkg, odo, m0, x1, x2 = base
    m, x1, x2, good = _case(name, m0, x1, x2)
    if latch == "nan_source_z0":
        x1 = x1.copy()
        x1[:, 2] = 0.0  # check_depth then filters every match
        good = 0
    lat_in = PRESET if latch == "preset" else float("nan")
    rc_a, a = _iterate(pkg, odo, m, x1, x2, lat_in)
    rc_b, b, ng = _hypotheses(pkg, odo, m, x1, x2, lat_in)
    assert rc_a == 0 and rc_b == 0
    runs = m.size >= MIN_INL and good >= MIN_INL
    assert ng == (good if runs else 0), "good matches after the depth filter"
    for k in a:
        assert a[k] == b[k], f"{name}/{latch}: {k} differs between odo_ransac and hypotheses mode"
    lat_out = np.frombuffer(a["latch"], np.float64)[0]
    if latch == "preset":
        assert lat_out == PRESET, "a latch that holds a value is kept"
    elif runs:
        z = x1[m["queryIdx"][_best_good(m, x1, x2)], 2].astype(np.float64)
        assert lat_out in ((0.01 * z * z) ** 2).tolist(), "DepthCovariance of the best good match"
    else:
        assert np.isnan(lat_out), "RANSAC did not run (or had no depth to latch from): the latch stays NaN"
    if not runs:
        ident = np.eye(4, dtype=np.float32).tobytes()
        assert a["T"] == ident and a["ok"] == 0 and a["inliers"] == b"" and a["rmse"] == np.float32(1e6).tobytes()


def _best_good(m, x1, x2):
    """The good matches the latch may be taken from: those of the smallest
    distance (the first in std::sort's order; ties in any order)."""
    ok = np.flatnonzero((x1[m["queryIdx"], 2] > 0) & (x2[m["trainIdx"], 2] > 0))
    return ok[m["distance"][ok] == m["distance"][ok].min()]


def test_match_index_out_of_range(base):
    pkg, odo, m0, x1, x2 = base
    lib = pkg.load()
    m = m0.copy()
    m["queryIdx"][3] = x1.shape[0]
    rc_a, _ = _iterate(pkg, odo, m, x1, x2, float("nan"))
    msg_a = lib.odo_last_error().decode()
    rc_b, _, _ = _hypotheses(pkg, odo, m, x1, x2, float("nan"))
    msg_b = lib.odo_last_error().decode()
    assert rc_a == pkg._abi.ERR_ARG and rc_b == pkg._abi.ERR_ARG
    assert "match index out of range" in msg_a and "match index out of range" in msg_b
