"""odo_gicp_dense: GeneralizedICP::Compute(pF1, pF2, guess) on the clouds that
odo_dense_clouds left in HBM.

The call reads the frames' points where they lie, so it must equal
odo_gicp_grid_batch on the same points copied out through odo_get_dense_cloud,
bit for bit: with and without a Twc, on voxel-filtered clouds and on a leaf 0
(CreateCloud only) cloud. The room pair (48 k points a side at leaf 0.03: the
5 cm depth noise of cloud_ref.room_depth spreads the surfaces over many voxels)
is held against the oracle with tests/test_gicp.py's assertions; the oracle's
brute-force searches over that pair take about 12 s of CPU, once per session. Frames with 0, 19, 20 and 257 valid pixels
give the early exits and the smallest cloud that runs.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as R
import fuse_ref as F
import gicp_ref64 as G
import oracle_lib as O
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
EMPTY, N19, N20, N257, ROOM_A, ROOM_B = range(6)
PAIRS = [(ROOM_A, ROOM_B), (ROOM_B, ROOM_A), (N20, N257), (N257, N20), (N257, ROOM_A), (ROOM_A, N257), (N20, N20),
         (EMPTY, ROOM_A), (ROOM_A, EMPTY), (N19, ROOM_A), (ROOM_A, N19), (EMPTY, EMPTY), (N19, N20), (N20, N19)]
SHORT = (EMPTY, N19)


def frames():
    def make():
        rng = np.random.default_rng(0xD3)
        depth = np.concatenate([R.scattered(rng, k) for k in (0, 19, 20, 257)] + [R.room_depth(rng), R.room_depth(rng)])
        return R.colours(rng, 6), np.ascontiguousarray(depth)
    return G.cached("dense_frames", make)


@pytest.fixture(scope="module")
def ctx():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(R.W, R.H, 6, nfeatures=500, iterations=50,
                                        calib={**R.CAMS["fr1"], **F.NO_DISTORTION}))
    yield pkg, o
    o.close()


def xyz(pts):
    return np.ascontiguousarray(np.stack([pts["x"], pts["y"], pts["z"]], 1))


def same(a, b):
    return len(a) == len(b) and all(x[1:] == y[1:] and x[0].tobytes() == y[0].tobytes() for x, y in zip(a, b))


def poses(n):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0x7D)
    T = np.tile(I4, (n, 1, 1))
    for k in range(n):
        T[k, :3, :3] = Rotation.from_rotvec(rng.uniform(-0.5, 0.5, 3)).as_matrix()
        T[k, :3, 3] = rng.uniform(-2, 2, 3)
    return T


@pytest.mark.parametrize("twc", [False, True], ids=["camera_frame", "map_frame"])
def test_equals_the_host_path(ctx, twc):
    _, odo = ctx
    bgr, depth = frames()
    # a pose per frame; the two room frames share one, so that they still overlap in the map frame
    Twc = poses(6)
    Twc[ROOM_B] = Twc[ROOM_A]
    info = odo.dense_clouds_host(bgr, depth, 0.03, Twc if twc else None)
    assert [int(v) for v in info["n_valid"][:4]] == [0, 19, 20, 257] and info["n_points"][N20] == 20
    assert info["n_points"][N19] == 19 and min(info["n_points"][4:]) > 10000
    clouds = [xyz(odo.get_dense_cloud(i)) for i in range(6)]
    got = odo.gicp_dense(PAIRS, None, 3, 0.05)
    want = odo.gicp_grid_batch([(clouds[s], clouds[t], None) for s, t in PAIRS], 3, 0.05)
    assert same(got, want)
    for (s, t), (T, conv, it, nc) in zip(PAIRS, got):
        if s in SHORT or t in SHORT:
            assert (conv, it, nc) == (0, 0, 0) and np.array_equal(T, I4), (s, t)
    assert got[0][1] == 1 and got[0][3] > 1000 and got[2][3] >= 0
    # one pair per call, and a guess per pair
    for k in (0, 2, 7):
        assert same(odo.gicp_dense([PAIRS[k]], None, 3, 0.05), got[k:k + 1]), k
    g = I4.copy()
    g[:3, 3] = [0.01, -0.02, 0.005]
    two = odo.gicp_dense([PAIRS[0], PAIRS[1]], [g, None], 3, 0.05)
    assert same(two, odo.gicp_grid_batch([(clouds[4], clouds[5], g), (clouds[5], clouds[4], None)], 3, 0.05))
    assert same(two[1:], got[1:2]) and not np.array_equal(two[0][0], got[0][0])
    # the clouds are still there
    assert all(np.array_equal(xyz(odo.get_dense_cloud(i)), clouds[i]) for i in range(6))


def test_unfiltered_cloud(ctx):
    _, odo = ctx
    bgr, depth = frames()
    info = odo.dense_clouds_host(bgr[N20:N257 + 1], depth[N20:N257 + 1], 0.0)
    assert list(info["n_points"]) == [20, 257] and info["status"][1] == R.CLOUD_UNFILTERED
    a, b = xyz(odo.get_dense_cloud(0)), xyz(odo.get_dense_cloud(1))
    got = odo.gicp_dense([(1, 1), (0, 1), (1, 0)], None, 2, 0.05)
    assert same(got, odo.gicp_grid_batch([(b, b, None), (a, b, None), (b, a, None)], 2, 0.05)) and got[0][3] == 257


def test_room_pair_against_the_oracle(ctx):
    _, odo = ctx
    bgr, depth = frames()
    odo.dense_clouds_host(bgr, depth, 0.03)
    S, T = xyz(odo.get_dense_cloud(ROOM_A)), xyz(odo.get_dense_cloud(ROOM_B))
    ref = G.cached("dense_room_oracle", lambda: O.gicp(S, T, None, 3, 0.05))
    Tg, conv, it, nc = odo.gicp_dense([(ROOM_A, ROOM_B)], None, 3, 0.05)[0]
    print(f"room pair: {len(S)} and {len(T)} points, converged {conv}, iterations {it}, n_corr {nc}")
    assert (conv, it, nc) == (ref["converged"], ref["iterations"], ref["n_corr"]) and conv == 1
    np.testing.assert_allclose(Tg, ref["T"], rtol=0, atol=1e-5)


def test_state_and_argument_errors(ctx):
    pkg, _ = ctx
    lib, E = pkg.load(), pkg._abi
    bgr, depth = frames()
    fresh = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50))
    try:
        T, io = np.full(32, 7.0, np.float32), np.full(6, 7, np.int32)
        nan_g = np.tile(I4, (2, 1, 1))
        nan_g[1, 2, 3] = np.nan

        def call(pairs, n, g=None, iters=3, dist=0.05, out=T):
            p = np.asarray(pairs, np.int32)
            return lib.odo_gicp_dense(fresh.h, p.ctypes.data if p.size else None, n, None if g is None else g.ctypes.data,
                                      iters, dist, None if out is None else out.ctypes.data, io[0:].ctypes.data,
                                      io[2:].ctypes.data, io[4:].ctypes.data)

        assert call([0, 1], 1) == E.ERR_STATE and call([], 0) == E.ERR_STATE
        fresh.dense_clouds_host(bgr[3:6], depth[3:6], 0.03)
        for args in (([0, 3], 1), ([-1, 0], 1), ([0, 1], -1), ([0, 1], 1, None, 0), ([0, 1], 1, None, 3, -0.05),
                     ([0, 1], 1, None, 3, float("nan")), ([0, 1, 1, 2], 2, nan_g), ([0, 1], 1, None, 3, 0.05, None),
                     ([], 1)):
            assert call(*args) == E.ERR_ARG, args
            assert lib.odo_last_error()
        assert np.all(T == 7.0) and np.all(io == 7)
        assert call([], 0) == 0 and np.all(T == 7.0)
        assert call([1, 2, 2, 1], 2) == 0 and io[0] == 1 and io[1] == 1 and T[31] == 1.0
    finally:
        fresh.close()


def test_tracking_is_undisturbed(ctx):
    """The pair records of two tracked batches are the same with dense clouds and
    a dense GICP between them as without."""
    pkg, _ = ctx
    bgr, dep, _ = sequence(4)
    bgr, dep = np.ascontiguousarray(bgr), np.ascontiguousarray(dep)

    def track(dense):
        odo = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50))
        try:
            out = []
            for a in (0, 2):
                out.append(odo.track_batch_host(bgr[a:a + 2], dep[a:a + 2]).copy())
                if dense:
                    odo.dense_clouds_host(bgr[a:a + 2], dep[a:a + 2], 0.03)
                    r = odo.gicp_dense([(0, 1)], None, 2, 0.05)
                    assert r[0][3] > 1000 and len(odo.frame(1)["kps"]) > 0  # the tracked batch is still readable
            return np.concatenate(out)
        finally:
            odo.close()

    a, b = track(False), track(True)
    assert a.tobytes() == b.tobytes() and a["n_matches"][1:].min() > 0
