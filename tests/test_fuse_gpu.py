"""odo_fuse_search (k_fuse.hip) against the reference of tests/fuse_ref.py.

Every comparison is exact: u, v, ur by bit pattern, the integers equal. The
cases are the reference's own (tests/test_fuse_ref.py checks them on the CPU):
the comparisons' edges under a camera that projects (x, y, 1) to (x, y), the
shapes around the kernel's steps (64 lanes, 256 threads, the 2048-keypoint
staging chunk) under the FR1 intrinsics, and the crafted FuseLandmarks
scenario end to end, where a replay that keeps a stale best fails.
"""
import numpy as np
import pytest

import fuse_ref as F
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

EDGE = F.edge_cases()
SHAPE = F.shape_cases()


def make(pkg, cam):
    return pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=500, iterations=50, calib={**cam, **F.NO_DISTORTION}))


@pytest.fixture(scope="module")
def unit():
    pkg = load_pkg()
    odo = make(pkg, F.CAM_UNIT)
    yield pkg, odo, F.camera(F.CAM_UNIT)
    odo.close()


@pytest.fixture(scope="module")
def fr1():
    pkg = load_pkg()
    odo = make(pkg, F.CAM_FR1)
    yield pkg, odo, F.camera(F.CAM_FR1)
    odo.close()


def check(ctx, case):
    pkg, odo, cam = ctx
    calls, lms, idx, th = case
    got = odo.fuse_search(calls, lms, idx, th)
    assert got.dtype == F.CAND_DTYPE
    assert F.records_equal(got, F.search_calls(calls, lms, idx, th, cam)) is None
    return got


def test_bounds_are_the_image(unit, fr1):
    for pkg, odo, cam in (unit, fr1):
        b = np.zeros(4, np.float32)
        pkg.check(odo.lib.odo_image_bounds(odo.h, pkg.ptr(b)))
        assert tuple(b) == cam["bounds"]


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edges(unit, name):
    check(unit, EDGE[name])


@pytest.mark.parametrize("name", sorted(SHAPE))
def test_shapes(fr1, name):
    check(fr1, SHAPE[name])


def test_scenario_end_to_end(fr1):
    """fuse_landmarks with the device search and fuse_best: the final slots,
    observations, bad flags and descriptors of the reference."""
    pkg, odo, _ = fr1
    _, want, stats, _ = F.scenario_reference()
    got, gstats, s = F.run_scenario(odo.fuse_search, pkg.fuse_best)
    assert got == want and gstats == stats
    assert s.rescored > 0
    stale, _, _ = F.run_scenario(odo.fuse_search, None)
    assert stale != want


def raw(ctx, K, kun, ur, desc, lms, idx, th=4.0, n_kp=None, n_lms=None, n_index=None, out=None, n_kf=None):
    pkg, odo, _ = ctx
    p = pkg.ptr
    return odo.lib.odo_fuse_search(odo.h, p(K), len(K) if n_kf is None else n_kf, p(kun), p(ur), p(desc),
                                   len(kun) if n_kp is None else n_kp, p(lms), len(lms) if n_lms is None else n_lms,
                                   p(idx), len(idx) if n_index is None else n_index, th, p(out))


def test_errors_and_capacities(fr1):
    pkg, odo, _ = fr1
    A, CAP = pkg._abi.ERR_ARG, pkg._abi.ERR_CAPACITY
    kun, ur, desc = np.zeros((10, 2), np.float32), np.zeros(10, np.float32), np.zeros((10, 32), np.uint8)
    lms, idx = np.zeros(4, pkg.LANDMARK_DTYPE), np.arange(4, dtype=np.int32)
    K = np.zeros(1, pkg.FUSE_KF_DTYPE)
    K[0] = (np.eye(4, dtype=np.float32).ravel(), 0, 10, 0, 4)
    out = np.full(8 * 40, 0x5A, np.uint8).view(pkg.FUSE_CAND_DTYPE)
    before = out.tobytes()
    inputs = [a.copy() for a in (K, kun, ur, desc, lms, idx)]

    def bad(code, **kw):
        a = dict(K=K, kun=kun, ur=ur, desc=desc, lms=lms, idx=idx, out=out)
        a.update(kw)
        assert raw(fr1, a.pop("K"), a.pop("kun"), a.pop("ur"), a.pop("desc"), a.pop("lms"), a.pop("idx"), **a) == code, kw
        assert odo.lib.odo_last_error()
        assert out.tobytes() == before, kw

    def with_kf(**f):
        k = K.copy()
        for name, v in f.items():
            k[name] = v
        return k

    assert odo.lib.odo_fuse_search(None, None, 0, None, None, None, 0, None, 0, None, 0, 4.0, None) == A
    bad(A, K=None, n_kf=1)
    bad(A, kun=None, n_kp=10)
    bad(A, ur=None, n_kp=10)
    bad(A, desc=None, n_kp=10)
    bad(A, lms=None, n_lms=4)
    bad(A, idx=None, n_index=4)
    bad(A, out=None)
    bad(A, n_kp=-1)
    for th in (-1.0, float("nan"), float("inf")):
        bad(A, th=th)
    bad(A, K=with_kf(kp_end=11))
    bad(A, K=with_kf(kp_begin=-1))
    bad(A, K=with_kf(kp_begin=6, kp_end=5))
    bad(A, K=with_kf(lm_end=5))
    bad(A, K=with_kf(lm_begin=-1))
    bad(A, K=with_kf(lm_begin=3, lm_end=2))
    bad(CAP, K=np.repeat(K, 257))
    bad(CAP, lms=np.zeros(65537, pkg.LANDMARK_DTYPE))
    big = 8192
    bad(CAP, K=with_kf(kp_end=big), kun=np.zeros((big, 2), np.float32), ur=np.zeros(big, np.float32),
        desc=np.zeros((big, 32), np.uint8))
    long_idx = np.zeros(4097, np.int32)
    bad(CAP, K=np.repeat(with_kf(lm_end=4097), 256), idx=long_idx)  # 256 * 4097 > 2^20
    for a, b in zip(inputs, (K, kun, ur, desc, lms, idx)):
        assert a.tobytes() == b.tobytes()
    # the limits themselves are inside the capacity; empty ranges and an empty list are valid
    assert raw(fr1, np.repeat(with_kf(lm_end=0), 256), kun, ur, desc, lms, idx, out=None) == 0
    assert raw(fr1, K[:0], kun[:0], ur[:0], desc[:0], lms[:0], idx[:0], out=None) == 0
    k8191 = 8191
    one = np.zeros(1, pkg.FUSE_CAND_DTYPE)
    assert raw(fr1, with_kf(kp_end=k8191, lm_end=1), np.zeros((k8191, 2), np.float32), np.zeros(k8191, np.float32),
               np.zeros((k8191, 32), np.uint8), lms, idx, out=one) == 0
    assert out.tobytes() == before


def test_scratch_grows_and_results_repeat(fr1):
    """A fresh context: a small call, a larger one that regrows the scratch, the small one again."""
    pkg, _, cam = fr1
    odo = make(pkg, F.CAM_FR1)
    try:
        ctx = (pkg, odo, cam)
        small = check(ctx, SHAPE["kp_63"])
        rng = np.random.default_rng(9)
        kf, lms = F.random_call(rng, 8191, 200)  # the most keypoints a keyframe may have
        calls = [kf + ((0, 200),)] * 12  # 98 292 sorted points: past the first block of 1 MiB
        check(ctx, (calls, lms, np.arange(200, dtype=np.int32), 4.0))
        again = check(ctx, SHAPE["kp_63"])
        assert small.tobytes() == again.tobytes()
    finally:
        odo.close()


def test_last_batch_stays_readable_and_tracking_is_unchanged():
    """A call after a batch leaves the batch's frames readable, and a call
    between two batches leaves both batches' results as without it."""
    pkg = load_pkg()
    bgr, dep, _ = sequence(4)
    case = SHAPE["list_257"]
    outs = []
    for with_fuse in (False, True):
        odo = pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=500, iterations=50))
        try:
            r1 = odo.track_batch_host(bgr[:2], dep[:2])
            f0, m0 = odo.frame(1), odo.pair(1)["matches"]
            if with_fuse:
                odo.fuse_search(*case)
                f1 = odo.frame(1)
                assert all(np.array_equal(f0[k], f1[k]) for k in f0)
                assert np.array_equal(m0, odo.pair(1)["matches"])
            r2 = odo.track_batch_host(bgr[2:4], dep[2:4])
            outs.append((r1.tobytes(), r2.tobytes()))
        finally:
            odo.close()
    assert outs[0] == outs[1]
