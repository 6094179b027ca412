"""odo_dense_clouds (k_cloud.hip) against the reference of tests/cloud_ref.py.

Infos, order, counts and colours are exact (min_p / max_p by bit pattern); x, y,
z lie within the derived bound of a float32 sum in any order (cloud_ref's
docstring), and a voxel of one point equals that point bit for bit. The cases
are the reference's own (tests/test_cloud_ref.py checks on the CPU that each has
the property it is named for) plus two frames of the synthetic sequence.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as R
import fuse_ref as F
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

CASES = R.cases()
NAMES = sorted(CASES) + ["sequence"]
_ODO = {}
_REFS = {}


def case(name):
    if name == "sequence":
        bgr, dep, _ = sequence(2)
        return "fr1", np.ascontiguousarray(bgr), np.ascontiguousarray(dep), 0.03
    return CASES[name]


def ref(name, leaf=None):
    cam, bgr, depth, lf = case(name)
    lf = lf if leaf is None else leaf
    if (name, lf) not in _REFS:
        _REFS[name, lf] = R.dense_ref(bgr, depth, R.CAMS[cam], lf)
    return _REFS[name, lf]


@pytest.fixture(scope="module")
def ctx():
    """camera name -> a 640 x 480 context with max_batch 3, made on first use."""
    pkg = load_pkg()

    def get(cam):
        if cam not in _ODO:
            _ODO[cam] = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50,
                                                        calib={**R.CAMS[cam], **F.NO_DISTORTION}))
        return pkg, _ODO[cam]

    yield get
    for o in _ODO.values():
        o.close()
    _ODO.clear()


def run(odo, bgr, depth, leaf, Twc=None):
    info = odo.dense_clouds_host(bgr, depth, leaf, Twc)
    return info, [odo.get_dense_cloud(i, counts=True) for i in range(len(depth))]


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(p.tobytes() == q.tobytes() and c.tobytes() == d.tobytes()
                                                   for (p, c), (q, d) in zip(a[1], b[1]))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_frame(info, pts, counts, r, what):
    for k in ("status", "n_valid", "n_points"):
        assert int(info[k]) == int(r[k]), (what, k, int(info[k]), int(r[k]))
    assert np.array_equal(info["min_b"], r["min_b"]) and np.array_equal(info["div_b"], r["div_b"]), what
    assert np.array_equal(bits(info["min_p"]), bits(r["min_p"])) and np.array_equal(bits(info["max_p"]), bits(r["max_p"])), what
    assert len(pts) == len(counts) == r["n_points"], what
    assert np.array_equal(counts, r["counts"]), what
    assert np.array_equal(np.stack([pts[a] for a in "bgra"], 1), r["bgra"]), what
    got = np.stack([pts[a] for a in "xyz"], 1)
    err = np.abs(got.astype(np.float64) - r["xyz64"])
    bound = R.centroid_bound(r)
    if len(got):
        print(f"{what}: {len(got)} points, largest count {int(counts.max())}, worst |err| / bound "
              f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound), what
    one = r["counts"] == 1
    assert np.array_equal(bits(got[one]), bits(r["first"][one])), what


@pytest.mark.parametrize("name", NAMES)
def test_case(ctx, name):
    cam, bgr, depth, leaf = case(name)
    pkg, odo = ctx(cam)
    a = run(odo, bgr, depth, leaf)
    assert a[0].dtype == pkg.CLOUD_INFO_DTYPE and a[1][0][0].dtype == pkg.CLOUD_DTYPE
    for f, r in enumerate(ref(name)):
        check_frame(a[0][f], a[1][f][0], a[1][f][1], r, f"{name}[{f}]")
    assert same(a, run(odo, bgr, depth, leaf)), "a second call differs"


@pytest.mark.parametrize("name", ["leaf_zero", "random_overflow"])
def test_unfiltered_is_the_raster_cloud(ctx, name):
    cam, bgr, depth, leaf = case(name)
    _, odo = ctx(cam)
    info, clouds = run(odo, bgr, depth, leaf)
    for f in range(len(depth)):
        want = R.create_cloud(bgr[f], depth[f], R.CAMS[cam])
        assert info[f]["status"] == R.CLOUD_UNFILTERED
        assert clouds[f][0].tobytes() == want.tobytes() and np.all(clouds[f][1] == 1)


def some_poses(n):
    rng = np.random.default_rng(0x7C)
    T = np.zeros((n, 4, 4), np.float32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        T[k, :3, :3] = q * rng.uniform(0.5, 2.0)  # not only rigid: the call takes any finite matrix
        T[k, :3, 3] = rng.uniform(-3, 3, 3)
        T[k, 3] = rng.standard_normal(4)  # the last row is not read
    return T


@pytest.mark.parametrize("name", ["room", "ragged_batch", "leaf_zero", "sequence", "heavy_four_voxels"])
def test_twc_is_applied_to_the_result(ctx, name):
    cam, bgr, depth, leaf = case(name)
    _, odo = ctx(cam)
    T = some_poses(len(depth))
    moved = run(odo, bgr, depth, leaf, T)
    plain = run(odo, bgr, depth, leaf)
    assert moved[0].tobytes() == plain[0].tobytes()  # the info is the camera frame's
    for f in range(len(depth)):
        assert moved[1][f][0].tobytes() == R.transform(plain[1][f][0], T[f]).tobytes()
        assert np.array_equal(moved[1][f][1], plain[1][f][1])
    if len(depth) and len(plain[1][-1][0]):
        assert moved[1][-1][0].tobytes() != plain[1][-1][0].tobytes()


class DeviceBytes:
    """A device range for torch.as_tensor."""

    def __init__(self, p, nbytes):
        self.__cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(p, False), version=2)


def test_device_frames_and_device_results(ctx):
    import torch
    cam, bgr, depth, leaf = case("ragged_batch")
    pkg, odo = ctx(cam)
    host = run(odo, bgr, depth, leaf)
    tb, td = torch.from_numpy(bgr).cuda(), torch.from_numpy(depth.view(np.int16)).cuda()
    torch.cuda.synchronize()
    info = odo.dense_clouds(tb.data_ptr(), td.data_ptr(), len(depth), leaf)
    dev = (info, [odo.get_dense_cloud(i, counts=True) for i in range(len(depth))])
    assert same(host, dev)
    for f in range(len(depth)):
        dp, dc, n = odo.dense_cloud_device(f)
        assert n == info[f]["n_points"]
        if n == 0:
            continue
        assert dp and dc
        p = torch.as_tensor(DeviceBytes(dp, 16 * n), device="cuda").cpu().numpy()
        c = torch.as_tensor(DeviceBytes(dc, 4 * n), device="cuda").cpu().numpy()
        assert p.tobytes() == dev[1][f][0].tobytes() and c.tobytes() == dev[1][f][1].tobytes()
    # the frames lie one after the other
    p0, _, n0 = odo.dense_cloud_device(0)
    p1, _, n1 = odo.dense_cloud_device(1)
    p2, _, _ = odo.dense_cloud_device(2)
    assert p1 == p0 + 16 * n0 and p2 == p1 + 16 * n1


def test_small_cap(ctx):
    cam, bgr, depth, leaf = case("room")
    pkg, odo = ctx(cam)
    info, clouds = run(odo, bgr, depth, leaf)
    full, cnt = clouds[0]
    cap = 100
    pts, c, n = np.zeros(cap + 1, pkg.CLOUD_DTYPE), np.full(cap + 1, -7, np.int32), C.c_int(-1)
    rc = odo.lib.odo_get_dense_cloud(odo.h, 0, pkg.ptr(pts), pkg.ptr(c), cap, C.byref(n))
    assert rc == pkg._abi.ERR_CAPACITY and n.value == len(full) > cap
    assert pts[:cap].tobytes() == full[:cap].tobytes() and np.array_equal(c[:cap], cnt[:cap])
    assert not pts[cap:].tobytes().strip(b"\0") and c[cap] == -7
    # counts are optional, and an exact cap is no error
    pts2, n2 = np.zeros(len(full), pkg.CLOUD_DTYPE), C.c_int(-1)
    assert odo.lib.odo_get_dense_cloud(odo.h, 0, pkg.ptr(pts2), None, len(full), C.byref(n2)) == 0
    assert pts2.tobytes() == full.tobytes() and n2.value == len(full)


def test_argument_errors_write_nothing(ctx):
    cam, bgr, depth, leaf = case("room")
    pkg, _ = ctx(cam)
    lib, E = pkg.load(), pkg._abi
    fresh = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50))
    try:
        info = np.full(3, -9, np.int32).repeat(15).view(pkg.CLOUD_INFO_DTYPE)
        keep = info.tobytes()
        b3, d3 = np.repeat(bgr, 3, 0), np.repeat(depth, 3, 0)
        pts, n = np.zeros(4, pkg.CLOUD_DTYPE), C.c_int(-5)
        dp, dn = C.c_void_p(77), C.c_int(-5)
        # the getters before any dense-cloud call
        assert lib.odo_get_dense_cloud(fresh.h, 0, pkg.ptr(pts), None, 4, C.byref(n)) == E.ERR_STATE
        assert lib.odo_dense_cloud_device(fresh.h, 0, C.byref(dp), None, C.byref(dn)) == E.ERR_STATE
        assert n.value == -5 and dn.value == -5 and dp.value == 77 and not pts.tobytes().strip(b"\0")
        nan = np.eye(4, dtype=np.float32)[None].repeat(3, 0)
        nan[2, 1, 3] = np.nan
        inf = nan.copy()
        inf[2, 1, 3] = -np.inf
        host = lib.odo_dense_clouds_host
        for args in ((None, pkg.ptr(d3), 3, 0.03, None, pkg.ptr(info)), (pkg.ptr(b3), None, 3, 0.03, None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, 0.03, None, None), (pkg.ptr(b3), pkg.ptr(d3), 0, 0.03, None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), -1, 0.03, None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 4, 0.03, None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, -0.03, None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, float("nan"), None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, float("inf"), None, pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, 0.03, pkg.ptr(nan), pkg.ptr(info)),
                     (pkg.ptr(b3), pkg.ptr(d3), 3, 0.03, pkg.ptr(inf), pkg.ptr(info))):
            assert host(fresh.h, *args) == E.ERR_ARG, args[2:5]
            assert lib.odo_dense_clouds(fresh.h, *args) == E.ERR_ARG, args[2:5]
            assert lib.odo_last_error()
        assert info.tobytes() == keep
        # still no result to read, then one, and the getters' own checks
        assert lib.odo_get_dense_cloud(fresh.h, 0, pkg.ptr(pts), None, 4, C.byref(n)) == E.ERR_STATE
        got = fresh.dense_clouds_host(b3[:2], d3[:2], 0.03)
        assert got[0]["n_points"] == ref("room")[0]["n_points"]
        for i in (-1, 2):
            assert lib.odo_get_dense_cloud(fresh.h, i, pkg.ptr(pts), None, 4, C.byref(n)) == E.ERR_ARG
            assert lib.odo_dense_cloud_device(fresh.h, i, C.byref(dp), None, C.byref(dn)) == E.ERR_ARG
        assert lib.odo_get_dense_cloud(fresh.h, 0, None, None, 4, C.byref(n)) == E.ERR_ARG
        assert lib.odo_get_dense_cloud(fresh.h, 0, pkg.ptr(pts), None, -1, C.byref(n)) == E.ERR_ARG
        assert lib.odo_get_dense_cloud(fresh.h, 0, pkg.ptr(pts), None, 4, None) == E.ERR_ARG
        assert lib.odo_dense_cloud_device(fresh.h, 0, None, None, C.byref(dn)) == E.ERR_ARG
        assert n.value == -5 and dn.value == -5 and dp.value == 77 and not pts.tobytes().strip(b"\0")
        # a failed call keeps the last result readable
        assert host(fresh.h, pkg.ptr(b3), pkg.ptr(d3), 3, -1.0, None, pkg.ptr(info)) == E.ERR_ARG
        assert len(fresh.get_dense_cloud(1)) == got[1]["n_points"]
    finally:
        fresh.close()


def test_blocks_regrow_and_results_repeat():
    """A fresh context: one frame, then two (both blocks are sized exactly, so
    the scratch block and the output block regrow), then the one frame again.
    The one-frame results are byte-identical, frame 0 is still readable after
    the last call, and the two-frame result equals the same call on another
    fresh context."""
    pkg = load_pkg()
    bgr, dep, _ = sequence(2)
    bgr, dep = np.ascontiguousarray(bgr), np.ascontiguousarray(dep)
    one, two = (pkg.Odometry(pkg.default_config(R.W, R.H, 2, nfeatures=500, iterations=50)) for _ in range(2))
    try:
        a = run(one, bgr[:1], dep[:1], 0.03)
        b = run(one, bgr, dep, 0.03)
        assert b[0]["n_points"].sum() > a[0]["n_points"].sum() > 0
        again = run(one, bgr[:1], dep[:1], 0.03)
        assert same(a, again) and len(again[1]) == 1
        assert one.get_dense_cloud(0, counts=True)[0].tobytes() == a[1][0][0].tobytes()
        assert same(b, run(two, bgr, dep, 0.03)) and len(b[1]) == 2
    finally:
        one.close()
        two.close()


def test_more_than_64_frames():
    """66 frames in one call: the frames' output offsets are scanned 64 at a
    time by one wave, so frames 64 and 65 start at the carry of the first
    round. A few scattered points per frame (none in some, also at the round's
    edges), every frame compared with the reference like the single cases."""
    pkg = load_pkg()
    rng = np.random.default_rng(0x66F)
    n = 66
    counts = [int(k) for k in rng.integers(0, 70, n)]
    counts[0], counts[63], counts[64], counts[65] = 3, 0, 65, 2
    depth = np.concatenate([R.scattered(rng, k) for k in counts])
    bgr = np.ascontiguousarray(np.broadcast_to(R.colours(rng), (n, R.H, R.W, 3)))
    odo = pkg.Odometry(pkg.default_config(R.W, R.H, n, nfeatures=500, iterations=50,
                                          calib={**R.CAMS["fr1"], **F.NO_DISTORTION}))
    try:
        info, clouds = run(odo, bgr, depth, 0.03)
        assert [int(v) for v in info["n_valid"]] == counts
        for f, r in enumerate(R.dense_ref(bgr, depth, R.CAMS["fr1"], 0.03)):
            check_frame(info[f], clouds[f][0], clouds[f][1], r, f"frame {f} of {n}")
    finally:
        odo.close()


def test_tracking_is_undisturbed(ctx):
    """The pair records of two tracked batches are the same with a dense-cloud
    call between them (and one before and after) as without."""
    pkg = load_pkg()
    bgr, dep, _ = sequence(4)
    bgr, dep = np.ascontiguousarray(bgr), np.ascontiguousarray(dep)

    def track(clouds):
        odo = pkg.Odometry(pkg.default_config(R.W, R.H, 3, nfeatures=500, iterations=50))
        try:
            out = []
            for a in (0, 2):
                if clouds:
                    odo.dense_clouds_host(bgr[a:a + 2], dep[a:a + 2], 0.03)
                out.append(odo.track_batch_host(bgr[a:a + 2], dep[a:a + 2]).copy())
                if clouds:
                    info = odo.dense_clouds_host(bgr[a:a + 1], dep[a:a + 1], 0.03)
                    assert info[0]["n_points"] == len(odo.get_dense_cloud(0)) > 0
                    assert len(odo.frame(1)["kps"]) > 0  # the tracked batch is still readable
            return np.concatenate(out)
        finally:
            odo.close()

    a, b = track(False), track(True)
    assert a.tobytes() == b.tobytes() and a["n_matches"][1:].min() > 0
