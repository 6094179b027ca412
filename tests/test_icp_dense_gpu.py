"""odo_icp_plane_dense: libicp's IcpPointToPlane on the clouds that
odo_dense_clouds left in HBM. It reads the frames' points where they lie, so it
must equal odo_icp_plane_batch on the same points copied out through
odo_get_dense_cloud, bit for bit: with and without a Twc, and with a guess.
Frames with 0, 4, 5 and 257 valid pixels give the exits and the smallest
clouds that run; the room pair (48 k points a side at leaf 0.03) is held
against ref64 (tests/icp_ref.py), run once per session.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as R
import fuse_ref as F
import icp_ref as I
from conftest import load_pkg

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
EMPTY, N4, N5, N257, ROOM_A, ROOM_B = range(6)
PAIRS = [(ROOM_A, ROOM_B), (ROOM_B, ROOM_A), (N5, N257), (N257, N5), (N257, ROOM_A), (ROOM_A, N257), (N5, N5),
         (N4, ROOM_A), (ROOM_A, N4), (EMPTY, ROOM_A), (ROOM_A, EMPTY), (EMPTY, EMPTY), (N4, N5), (N5, N4)]
ROOM_KW = dict(num_neighbors=10, max_iterations=20, min_delta=1e-4, indist=0.01, gate=I.GATE_AS_WRITTEN)


def frames():
    def make():
        rng = np.random.default_rng(0x1C9)
        depth = np.concatenate([R.scattered(rng, k) for k in (0, 4, 5, 257)] + [R.room_depth(rng), R.room_depth(rng)])
        return R.colours(rng, 6), np.ascontiguousarray(depth)
    return I.cached("dense_frames", make)


@pytest.fixture(scope="module")
def ctx():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(R.W, R.H, 6, nfeatures=500, iterations=50,
                                        calib={**R.CAMS["fr1"], **F.NO_DISTORTION}))
    yield pkg, o
    o.close()


def xyz(pts):
    return np.ascontiguousarray(np.stack([pts["x"], pts["y"], pts["z"]], 1))


def poses(n):
    rng = np.random.default_rng(0x7D)
    T = np.tile(I4, (n, 1, 1))
    for k in range(n):
        T[k, :3, :3] = I.rotation(rng.uniform(-0.5, 0.5, 3))
        T[k, :3, 3] = rng.uniform(-2, 2, 3)
    return T


def expected_status(clouds, s, t):
    return I.NO_MODEL if len(clouds[t]) < 5 else I.SHORT_TEMPLATE if len(clouds[s]) < 5 else None


@pytest.mark.parametrize("twc", [False, True], ids=["camera_frame", "map_frame"])
def test_equals_the_host_path(ctx, twc):
    pkg, odo = ctx
    bgr, depth = frames()
    Twc = poses(6)
    Twc[ROOM_B] = Twc[ROOM_A]  # the two room frames still overlap in the map frame
    info = odo.dense_clouds_host(bgr, depth, 0.03, Twc if twc else None)
    assert [int(v) for v in info["n_valid"][:4]] == [0, 4, 5, 257] and min(info["n_points"][4:]) > 10000
    assert [int(v) for v in info["n_points"][:3]] == [0, 4, 5]
    clouds = [xyz(odo.get_dense_cloud(i)) for i in range(6)]
    prm = pkg.icp_params(max_iterations=4, indist=0.01)
    got = odo.icp_plane_dense(PAIRS, None, prm)
    want = odo.icp_plane_batch([(clouds[s], clouds[t], None) for s, t in PAIRS], prm)
    assert got.tobytes() == want.tobytes()
    for (s, t), rec in zip(PAIRS, got):
        st = expected_status(clouds, s, t)
        if st is not None:
            assert rec["status"] == st and rec["iterations"] == 0 and np.array_equal(rec["T"].reshape(4, 4), I4), (s, t)
        else:
            assert rec["iterations"] >= 1, (s, t)
    assert got[0]["status"] == I.OK and got[0]["n_active"] > 10000
    # one pair per call, and a guess per pair
    for k in (0, 2, 7):
        assert odo.icp_plane_dense([PAIRS[k]], None, prm).tobytes() == got[k:k + 1].tobytes(), k
    g = I4.copy()
    g[:3, 3] = [0.01, -0.02, 0.005]
    two = odo.icp_plane_dense([PAIRS[0], PAIRS[1]], [g, None], prm)
    assert two.tobytes() == odo.icp_plane_batch([(clouds[4], clouds[5], g), (clouds[5], clouds[4], None)], prm).tobytes()
    assert two[1].tobytes() == got[1].tobytes() and two[0].tobytes() != got[0].tobytes()
    assert all(np.array_equal(xyz(odo.get_dense_cloud(i)), clouds[i]) for i in range(6))  # the clouds are still there


def test_room_pair_against_ref64(ctx):
    pkg, odo = ctx
    bgr, depth = frames()
    odo.dense_clouds_host(bgr, depth, 0.03)
    S, M = xyz(odo.get_dense_cloud(ROOM_A)), xyz(odo.get_dense_cloud(ROOM_B))
    ref = I.cached("dense_room_ref64", lambda: I.ref64(S, M, **ROOM_KW))
    r32 = I.cached("dense_room_ref32", lambda: I.ref32(S, M, **ROOM_KW))
    rec = odo.icp_plane_dense([(ROOM_A, ROOM_B)], None, pkg.icp_params(**ROOM_KW))[0]
    share = lambda r: r["n_active"] / len(S)
    e_share = 4 * max(abs(share(r32) - share(ref)), 1.0 / len(S))
    err = np.abs(rec["T"].reshape(4, 4) - ref["T"]).max()
    print(f"room pair: {len(S)} and {len(M)} points, iterations {rec['iterations']} / {ref['iterations']}, n_active "
          f"{rec['n_active']} / {ref['n_active']} / ref32 {r32['n_active']}, residual {rec['residual']:.9e} / "
          f"{ref['residual']:.9e}, |T - ref64| {err:.3e}, delta {rec['delta']:.3e}")
    assert ref["iterations"] < ROOM_KW["max_iterations"] and ref["delta"] <= ROOM_KW["min_delta"]  # it converges
    assert rec["status"] == I.OK and rec["iterations"] == ref["iterations"] and rec["delta"] <= ROOM_KW["min_delta"]
    assert abs(share(rec) - share(ref)) <= e_share
    assert abs(rec["residual"] - ref["residual"]) <= I.residual_rtol() * abs(ref["residual"])
    assert err <= I.tolerance()


def test_state_and_argument_errors(ctx):
    pkg, _ = ctx
    lib, E = pkg.load(), pkg._abi
    bgr, depth = frames()
    fresh = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50))
    try:
        out = np.zeros(2, pkg.ICP_RESULT_DTYPE)
        out["T"], out["status"] = 7.0, 7
        before = out.tobytes()
        nan_g = np.tile(I4, (2, 1, 1))
        nan_g[1, 2, 3] = np.nan

        def call(pairs, n, g=None, prm=None, o=out):
            p = np.asarray(pairs, np.int32)
            q = pkg.icp_params(max_iterations=2) if prm is None else prm
            return lib.odo_icp_plane_dense(fresh.h, p.ctypes.data if p.size else None, n,
                                           None if g is None else g.ctypes.data, None if prm is False else C.byref(q),
                                           None if o is None else o.ctypes.data)

        assert call([0, 1], 1) == E.ERR_STATE and call([], 0) == E.ERR_STATE
        fresh.dense_clouds_host(bgr[3:6], depth[3:6], 0.03)
        P = pkg.icp_params
        for args in (([0, 3], 1), ([-1, 0], 1), ([0, 1], -1), ([0, 1], 1, None, P(max_iterations=-1)),
                     ([0, 1], 1, None, P(num_neighbors=2)), ([0, 1], 1, None, P(indist=float("nan"))),
                     ([0, 1], 1, None, P(gate=3)), ([0, 1, 1, 2], 2, nan_g), ([0, 1], 1, None, None, None), ([], 1),
                     ([0, 1], 1, None, False)):
            assert call(*args) == E.ERR_ARG, args
            assert lib.odo_last_error()
        assert call([0, 1], 1, None, P(num_neighbors=33)) == E.ERR_CAPACITY
        assert out.tobytes() == before
        assert call([], 0) == 0 and out.tobytes() == before
        assert call([1, 2, 2, 1], 2) == 0 and out["status"][0] == I.OK and out["iterations"][1] == 2
    finally:
        fresh.close()
