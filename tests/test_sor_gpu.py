"""odo_cloud_sor_batch / odo_dense_sor (k_gicp.hip: k_sor_*) against tests/sor_ref.py.

distances[] bit for bit; mean, stddev and threshold within the bound derived in
sor_ref's docstring for a sum in another fixed order; the keep mask, n_out and
the status exactly (tests/test_sor_ref.py checks on the CPU that no distance of
a case lies within the bound of its threshold). Every cloud runs with the
automatic cell and with three forced ones (tiny, in between, one cell for the
whole cloud), with bit-equal results across cells. The cases are sor_ref's.
"""
import numpy as np
import pytest

import cloud_ref as CR
import fuse_ref as F
import sor_ref as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_STATE = S.ERR_ARG, S.ERR_CAPACITY, S.ERR_STATE


@pytest.fixture(scope="module")
def odo():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(640, 480, 1))
    yield o
    o.close()


def check(got, r, what):
    keep, dist, info = got
    b = S.threshold_bound(r)
    print(f"{what}: n {r['n_in']} -> {int(info['n_out'])}, mean {float(info['mean']):.17g} (ref {r['mean']:.17g}, bound "
          f"{b['mean']:.3g}), threshold {float(info['threshold']):.17g} (ref {r['threshold']:.17g}, bound "
          f"{b['threshold']:.3g})")
    assert int(info["status"]) == r["status"] and int(info["n_in"]) == r["n_in"], what
    assert dist.tobytes() == r["distances"].tobytes(), what
    assert abs(float(info["mean"]) - r["mean"]) <= b["mean"], what
    if b["nan_expected"]:
        assert np.isnan(info["stddev"]) and np.isnan(info["threshold"]), what
    else:
        assert abs(float(info["stddev"]) - r["stddev"]) <= b["stddev"], what
        assert abs(float(info["threshold"]) - r["threshold"]) <= b["threshold"], what
    assert np.array_equal(keep, r["keep"]), what
    assert int(info["n_out"]) == r["n_out"], what


@pytest.mark.parametrize("name", list(S.cases()))
def test_case(odo, name):
    P, k, mul = S.case(name)
    r = S.ref(name)
    first = None
    for cell in S.cells_for(P, name):
        keeps, dists, info = odo.cloud_sor_batch([P], k, mul, cell)
        check((keeps[0], dists[0], info[0]), r, (name, cell))
        got = (keeps[0].tobytes(), dists[0].tobytes(), info.tobytes())
        first = first or got
        assert got == first, (name, cell, "differs from the automatic cell")


def test_lattice_does_not_depend_on_the_order_of_points(odo):
    P, k, mul = S.case("lattice")
    rng = np.random.default_rng(0x5E)
    base = odo.cloud_sor_batch([P], k, mul)
    for _ in range(3):
        perm = rng.permutation(len(P))
        for cell in S.cells_for(P):
            keeps, dists, info = odo.cloud_sor_batch([np.ascontiguousarray(P[perm])], k, mul, cell)
            back = np.empty_like(dists[0])
            back[perm] = dists[0]
            assert back.tobytes() == base[1][0].tobytes()
            kb = np.empty_like(keeps[0])
            kb[perm] = keeps[0]
            assert np.array_equal(kb, base[0][0]) and int(info[0]["n_out"]) == int(base[2][0]["n_out"])


def test_mixed_batch(odo):
    clouds, k, mul = S.mixed_batch()
    refs = [S.sor(P, k, mul) for P in clouds]
    for cell in (0.0, 0.5):
        keeps, dists, info = odo.cloud_sor_batch(clouds, k, mul, cell)
        for i, r in enumerate(refs):
            check((keeps[i], dists[i], info[i]), r, ("batch", cell, i))
            one = odo.cloud_sor_batch([clouds[i]], k, mul, cell)
            assert one[1][0].tobytes() == dists[i].tobytes() and one[2][0].tobytes() == info[i].tobytes()
    assert odo.cloud_sor_batch([], k, mul)[2].shape == (0,)


def test_results_repeat(odo):
    P, k, mul = S.case("scene300_k50")
    a = odo.cloud_sor_batch([P], k, mul)
    b = odo.cloud_sor_batch([P], k, mul)
    assert a[1][0].tobytes() == b[1][0].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_argument_errors_write_nothing(odo):
    lib, h = odo.lib, odo.h
    P = np.ascontiguousarray(S.case("scene300_k8")[0])
    keep, dist = np.full(300, 7, np.uint8), np.full(300, 7.0, np.float32)
    info = np.full(5, 7, np.int64)  # 40 bytes
    ok = dict(P=P, offs=[0, 300], n=1, k=8, mul=1.0, cell=0.0, keep=keep, info=info)

    def call(**kw):
        a = {**ok, **kw}
        o = np.asarray(a["offs"], np.int32)
        p = lambda x: None if x is None else x.ctypes.data
        return lib.odo_cloud_sor_batch(h, p(a["P"]), o.ctypes.data, a["n"], a["k"], a["mul"], a["cell"], p(a["keep"]),
                                       dist.ctypes.data, p(a["info"]))

    nan_p = P.copy()
    nan_p[7, 1] = np.nan
    inf_p = P.copy()
    inf_p[299, 0] = np.inf
    for kw in (dict(P=None), dict(keep=None), dict(info=None), dict(offs=[1, 300]), dict(offs=[0, 200, 100], n=2),
               dict(k=0), dict(k=-3), dict(mul=float("nan")), dict(mul=float("inf")), dict(cell=-1.0),
               dict(cell=float("nan")), dict(cell=float("inf")), dict(P=nan_p), dict(P=inf_p), dict(n=-1)):
        assert call(**kw) == ERR_ARG, kw
        assert lib.odo_last_error()
    assert call(k=S.MAX_K + 1) == ERR_CAPACITY
    big = np.zeros((1048577, 3), np.float32)
    assert call(P=big, offs=[0, 1048577]) == ERR_CAPACITY
    assert call(cell=1e-4) == ERR_CAPACITY  # the forced cell's table
    assert np.all(keep == 7) and np.all(dist == 7.0) and np.all(info == 7)
    assert call(n=0) == 0 and np.all(keep == 7)
    assert call(k=S.MAX_K) == 0 and call() == 0
    assert np.array_equal(keep.astype(bool), S.ref("scene300_k8")["keep"])
    assert dist.tobytes() == S.ref("scene300_k8")["distances"].tobytes()


# ================================================================= odo_dense_sor
def dense_frames():
    """(bgr 4 x H x W x 3, depth 4 x H x W): three crafted frames of cloud_ref.cases()
    (257, 65 and 255 scattered valid pixels) and a synthetic one: a 300 x 200 pixel
    wall at 2 m with millimetre noise and six lone pixels far in front of it."""
    c = CR.cases()
    rng = np.random.default_rng(0xD5)
    d = np.zeros((CR.H, CR.W), np.uint16)
    d[100:300, 150:450] = (10000 + rng.integers(-10, 11, (200, 300))).astype(np.uint16)
    for i, j in ((20, 30), (50, 600), (400, 100), (450, 500), (240, 20), (30, 320)):
        d[i, j] = 2500 + 100 * (i % 7)
    names = ("valid_257", "valid_65", "valid_255")
    bgr = np.concatenate([c[n][1] for n in names] + [CR.colours(rng)])
    depth = np.concatenate([c[n][2] for n in names] + [d[None]])
    return np.ascontiguousarray(bgr), np.ascontiguousarray(depth)


def xyz(pts):
    return np.ascontiguousarray(np.stack([pts["x"], pts["y"], pts["z"]], 1))


def test_dense_sor():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(CR.W, CR.H, 4, nfeatures=500, iterations=50,
                                        calib={**CR.CAMS["fr1"], **F.NO_DISTORTION}))
    try:
        with pytest.raises(RuntimeError, match=f"odo error {ERR_STATE}"):
            o.dense_sor(8, 1.0)
        with pytest.raises(RuntimeError, match=f"odo error {ERR_STATE}"):
            o.gicp_dense_fitness([(0, 1)])
        bgr, depth = dense_frames()
        k, mul = 8, 1.0
        o.dense_clouds_host(bgr, depth, 0.03)
        cur = [o.get_dense_cloud(i, counts=True) for i in range(4)]
        assert all(3 * k < len(p) <= v for (p, _), v in zip(cur, (257, 65, 255))) and len(cur[3][0]) > 500
        for rnd in range(2):  # a second call filters the filtered clouds
            refs = [S.sor(xyz(p), k, mul) for p, _ in cur]
            assert all(S.margin_ok(r) for r in refs), "a condition on the inputs"
            info = o.dense_sor(k, mul)
            assert len(info) == 4
            after = [o.get_dense_cloud(i, counts=True) for i in range(4)]
            for i, (r, (p0, c0), (p1, c1)) in enumerate(zip(refs, cur, after)):
                print(f"round {rnd} frame {i}: {r['n_in']} -> {r['n_out']}")
                assert (int(info[i]["status"]), int(info[i]["n_in"]), int(info[i]["n_out"])) == (r["status"], r["n_in"], r["n_out"])
                b = S.threshold_bound(r)
                assert abs(float(info[i]["threshold"]) - r["threshold"]) <= b["threshold"]
                assert p1.tobytes() == p0[r["keep"]].tobytes() and c1.tobytes() == c0[r["keep"]].tobytes(), (rnd, i)
            if rnd == 0:
                assert refs[3]["n_out"] < refs[3]["n_in"], "the lone pixels go"
            # the device views: packed frame after frame, the filtered sizes
            dev = [o.dense_cloud_device(i) for i in range(4)]
            assert [d[2] for d in dev] == [len(p) for p, _ in after]
            for a, b_ in zip(dev, dev[1:]):
                assert b_[0] - a[0] == 16 * a[2] and b_[1] - a[1] == 4 * a[2]
            cur = after
        # GICP and the fitness score see the filtered clouds
        pairs = [(3, 3), (0, 2), (2, 3)]
        pts = [xyz(p) for p, _ in cur]
        got = o.gicp_dense(pairs, None, 5, 0.05)
        want = o.gicp_grid_batch([(pts[s], pts[t], None) for s, t in pairs], 5, 0.05)
        for g, w in zip(got, want):
            assert g[1:] == w[1:] and g[0].tobytes() == w[0].tobytes()
        assert got[0][3] == len(pts[3]), "a cloud against itself: every point corresponds"
        Ts = [g[0] for g in got]
        fit = o.gicp_dense_fitness(pairs, Ts)
        host, _ = o.gicp_grid_fitness([(pts[s], pts[t], T) for (s, t), T in zip(pairs, Ts)])
        assert fit.tobytes() == host.tobytes()
        for (s, t), T, f in zip(pairs, Ts, fit):
            ref = S.fitness(pts[s], pts[t], T)[0]
            assert abs(f - ref) <= S.fitness_bound(ref, len(pts[s]))
    finally:
        o.close()
