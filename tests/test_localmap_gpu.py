"""Batched TrackLocalMap on the device (odo_track_local_map, k_localmap.hip)
against the reference composition of tests/localmap_ref.py.

The frames are extracted on the device and read back with odo.frame(i), so the
reference runs on the features the device holds. Slots, projections (bit
patterns, NaNs included), n_in_view, n_matches and n_edges must be identical;
the pose and the inlier counts take the tolerances of the GPU PnP against
oracle_pnp (test_projection.py: pose 1e-4 max-abs, inlier counts within 2).
"""
import numpy as np
import pytest

import localmap_ref as R
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu


class Device:
    """A context with a batch in view and the frames it holds."""

    def __init__(self, bgr, dep):
        self.pkg = load_pkg()
        self.odo = self.pkg.Odometry(self.pkg.default_config(640, 480, len(bgr), nfeatures=R.NF))
        self.track(bgr, dep)

    def track(self, bgr, dep):
        self.odo.track_batch_host(np.ascontiguousarray(bgr), np.ascontiguousarray(dep))
        self.frames = [self.odo.frame(i) for i in range(len(bgr))]

    def run(self, P):
        res = self.odo.track_local_map(P["lms"], P["Tcw"], prior=P["prior"], th=P["th"], nn_ratio=P["nn_ratio"])
        return res, [self.odo.local_map(i) for i in range(len(P["frames"]))]


@pytest.fixture(scope="module")
def seq():
    return sequence(3, seed=R.SEQ_SEED)


@pytest.fixture(scope="module")
def dev(seq):
    bgr, dep, _ = seq
    d = Device(bgr, dep)
    yield d
    d.odo.close()


@pytest.fixture(scope="module")
def dev2(seq):
    """A batch of two frames: frames 1 and 2."""
    bgr, dep, _ = seq
    d = Device(bgr[1:3], dep[1:3])
    yield d
    d.odo.close()


def check(res, maps, ref, tag=""):
    assert len(res) == len(ref) == len(maps)
    for i, (g, m, r) in enumerate(zip(res, maps, ref)):
        t = f"{tag} frame {i}"
        print(f"{t}: in view {r['n_in_view']} matches {r['n_matches']} edges {r['n_edges']} "
              f"pnp {g['pnp_inliers']}/{r['pnp_inliers']} map {g['n_map_inliers']}/{r['n_map_inliers']} "
              f"pose err {np.abs(g['Tcw'] - r['Tcw']).max():.2e}")
        assert np.array_equal(m["slot_lm"], r["slot_lm"]), f"{t}: slots differ at {np.nonzero(m['slot_lm'] != r['slot_lm'])[0][:10]}"
        assert np.array_equal(m["proj"].view(np.uint32), r["proj"].view(np.uint32)), f"{t}: projections differ"
        assert g["n_in_view"] == r["n_in_view"], t
        assert g["n_matches"] == r["n_matches"], t
        assert g["n_edges"] == r["n_edges"], t
        assert np.abs(g["Tcw"] - r["Tcw"]).max() < 1e-4, t
        assert abs(int(g["pnp_inliers"]) - r["pnp_inliers"]) <= 2, t
        assert abs(int(g["n_map_inliers"]) - r["n_map_inliers"]) <= 2, t
        # flags only of slots that hold a landmark
        assert not m["pnp_outlier"][m["slot_lm"] < 0].any(), t


BUILDERS = dict(base=R.base_problem, contended=R.contended_problem, wide=R.wide_problem, half_obs=R.half_obs_problem,
                prior=R.prior_problem)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_local_map(dev, seq, name):
    """base: batch indexing, per-frame keypoint counts; contended: the order
    dependence; wide: lists beyond the candidate cap, long cascades; half_obs:
    overwrites of untaken slots; prior: per-frame SEEN / taken sets, release of
    BAD priors, prior edges in the PnP."""
    P = BUILDERS[name](dev.frames, seq[2])
    ref = R.compose(P)
    if name == "base":
        assert all(r["n_matches"] > 50 for r in ref)
    res, maps = dev.run(P)
    check(res, maps, ref, name)
    if name == "prior":
        # surviving prior slots are PnP edges
        for m, r in zip(maps, ref):
            keep = r["prior"] >= 0
            assert keep.sum() >= 100 and (m["slot_lm"][keep] >= 0).all()


@pytest.mark.parametrize("n_lms", [0, 1, 63, 64, 65, 255, 256, 257])
def test_chunk_edges(dev2, seq, n_lms):
    """Block and wave tails of both kernels: the first n_lms landmarks of the
    contended set, a batch of two frames."""
    poses = seq[2]
    lms = R.contended_landmarks([None, dev2.frames[0]], [None, poses[1]])  # the landmarks come from frame 1
    P = R.problem(dev2.frames, lms[:n_lms], R.true_poses(poses, (1, 2)), th=8.0)
    res, maps = dev2.run(P)
    ref = R.compose(P)
    check(res, maps, ref, f"n_lms {n_lms}")
    if n_lms == 0:
        for g, T in zip(res, P["Tcw"]):
            assert g["n_in_view"] == g["n_matches"] == g["n_edges"] == g["pnp_inliers"] == g["n_map_inliers"] == 0
            assert np.array_equal(g["Tcw"], T.ravel())


def _mix(dev, seq):
    return R.landmark_mix(dev.frames, seq[2])


@pytest.mark.parametrize("case", ["all_bad", "all_seen", "behind", "camera_plane"])
def test_flags_and_early_outs(dev, seq, case):
    poses = seq[2]
    lms = _mix(dev, seq)
    Tcw = R.true_poses(poses)
    if case == "all_bad":
        lms["flags"] |= R.BAD
    elif case == "all_seen":
        lms["flags"] |= R.SEEN
    elif case == "behind":
        Ry = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)  # a turn by pi about y
        Tcw = np.stack([Ry @ T for T in Tcw])
    else:
        # frame 0 at a pose of exact numbers, and one world point on its camera
        # plane: Pc.z = ((0 x + 0 y) + 1 (-2)) + 2 == 0, 1 / Pc.z = inf
        Tcw[0] = np.eye(4, dtype=np.float32)
        Tcw[0, 2, 3] = 2.0
        lms["X"][5] = (0.5, 0.25, -2.0)
        lms["flags"][5] = R.HAS_OBS
    P = R.problem(dev.frames, lms, Tcw, th=8.0)
    ref = R.compose(P)
    if case != "camera_plane":
        assert all(r["n_in_view"] == r["n_matches"] == r["n_edges"] == 0 for r in ref)
    res, maps = dev.run(P)
    check(res, maps, ref, case)
    if case != "camera_plane":
        for g, T in zip(res, Tcw):
            assert np.array_equal(g["Tcw"], T.ravel()) and g["pnp_inliers"] == 0


def test_camera_centre_landmark(dev, seq):
    """A landmark at the camera centre: Pc = 0, u = fx 0 inf + cx is NaN, which
    passes isInFrustum's bounds and has an empty window. The NaN is the result
    of an invalid operation, whose sign the hardware chooses (x86 SSE: the
    negative 'indefinite' NaN), so this one row is compared as NaN, not by bit
    pattern; everything else as everywhere."""
    poses = seq[2]
    lms = _mix(dev, seq)
    Tcw = R.true_poses(poses)
    Tcw[0] = np.eye(4, dtype=np.float32)
    Tcw[0, 2, 3] = 2.0
    lms["X"][5] = (0.0, 0.0, -2.0)
    lms["flags"][5] = R.HAS_OBS
    P = R.problem(dev.frames, lms, Tcw, th=8.0)
    ref = R.compose(P)
    res, maps = dev.run(P)
    assert np.isnan(maps[0]["proj"][5]).all() and np.isnan(ref[0]["proj"][5]).all()
    for m, r in zip(maps, ref):
        m["proj"][5] = r["proj"][5]
    check(res, maps, ref, "camera centre")
    in_view_without = R.compose(R.problem(dev.frames, np.delete(lms, 5), Tcw, th=8.0))[0]["n_in_view"]
    assert ref[0]["n_in_view"] == in_view_without + 1  # the NaN projection counts as in view


def test_empty_frame_in_the_middle(seq):
    """nkp == 0 inside a batch: nothing matched, the input pose, neighbours unaffected."""
    bgr, dep, poses = seq
    b = np.stack([bgr[1], np.zeros_like(bgr[1]), bgr[2]])
    d = np.stack([dep[1], dep[1], dep[2]])
    dv = Device(b, d)
    assert [len(f["kun"]) > 0 for f in dv.frames] == [True, False, True]
    lms = R.landmark_mix([None, dv.frames[0]], [None, poses[1]])
    P = R.problem(dv.frames, lms, R.true_poses(poses, (1, 1, 2)), th=8.0)
    ref = R.compose(P)
    res, maps = dv.run(P)
    check(res, maps, ref, "empty")
    assert res[1]["n_matches"] == res[1]["n_edges"] == res[1]["pnp_inliers"] == res[1]["n_map_inliers"] == 0
    assert np.array_equal(res[1]["Tcw"], P["Tcw"][1].ravel()) and len(maps[1]["slot_lm"]) == 0
    assert res[0]["n_matches"] > 50 and res[2]["n_matches"] > 50
    dv.odo.close()


def test_few_edges(dev, seq):
    """Two landmarks in view: PnPSolver::Compute returns 0 below 3 edges and the pose stays."""
    Xw, d1 = R.base_landmarks(dev.frames, seq[2])
    lms = np.zeros(2, R.O.LANDMARK_DTYPE)
    lms["X"], lms["desc"], lms["flags"] = Xw[:2], d1[:2], R.HAS_OBS
    P = R.problem(dev.frames, lms, R.true_poses(seq[2]), th=8.0)
    ref = R.compose(P)
    assert max(r["n_edges"] for r in ref) == 2
    res, maps = dev.run(P)
    check(res, maps, ref, "few")
    for g, T in zip(res, P["Tcw"]):
        assert g["pnp_inliers"] == 0 and np.array_equal(g["Tcw"], T.ravel())


def test_repeat_and_new_batch(seq):
    """Scratch reuse: the contended case twice on one context, a smaller case
    in between, then again after a new batch: no stale owner, slots or counts."""
    bgr, dep, poses = seq
    dv = Device(bgr, dep)
    P = R.contended_problem(dv.frames, poses)
    ref = R.compose(P)
    check(*dv.run(P), ref, "first")
    small = R.problem(dv.frames, P["lms"][:100], P["Tcw"], th=40.0)
    check(*dv.run(small), R.compose(small), "small")
    check(*dv.run(P), ref, "second")
    dv.track(bgr, dep)
    with pytest.raises(RuntimeError):  # the new batch has no local-map results yet
        dv.pkg.check(dv.odo.lib.odo_get_local_map(dv.odo.h, 0, dv.pkg.ptr(np.zeros(4096, np.int32)), None, None, 4096))
    check(*dv.run(P), ref, "after a new batch")
    dv.odo.close()


def test_errors():
    pkg = load_pkg()
    lib = pkg.load()
    A = pkg._abi
    odo = pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=R.NF))
    kc = odo.kp_capacity()
    lms = np.zeros(4, A.LANDMARK_DTYPE)
    T = np.tile(np.eye(4, dtype=np.float32).ravel(), (2, 1))
    out = np.zeros(2, A.LOCAL_MAP_DTYPE)
    call = lambda **k: lib.odo_track_local_map(odo.h, pkg.ptr(lms), k.get("n", 4), pkg.ptr(T), None, k.get("kc", kc),
                                               k.get("th", 8.0), 0.8, k.get("out", pkg.ptr(out)))
    assert call() == A.ERR_STATE  # no batch yet
    assert lib.odo_get_local_map(odo.h, 0, pkg.ptr(np.zeros(kc, np.int32)), None, None, kc) == A.ERR_STATE
    bgr, dep, _ = sequence(3, seed=R.SEQ_SEED)
    odo.track_batch_host(bgr[:2], dep[:2])
    assert call(kc=kc + 64) == A.ERR_ARG
    assert call(out=None) == A.ERR_ARG
    assert call(n=-1) == A.ERR_ARG
    assert call(th=-1.0) == A.ERR_ARG and call(th=float("nan")) == A.ERR_ARG and call(th=float("inf")) == A.ERR_ARG
    assert lib.odo_track_local_map(None, pkg.ptr(lms), 4, pkg.ptr(T), None, kc, 8.0, 0.8, pkg.ptr(out)) == A.ERR_ARG
    assert call(n=65537) == A.ERR_CAPACITY
    # none of the refused calls left results behind
    assert lib.odo_get_local_map(odo.h, 0, pkg.ptr(np.zeros(kc, np.int32)), None, None, kc) == A.ERR_STATE
    assert call() == 0
    odo.close()
