"""CPU checks of the dense-cloud reference (tests/cloud_ref.py): the numpy
restatement against the pass-by-pass transcription on tiny clouds, every
crafted case against the property it is named for, and the library's four
dense-cloud symbols against the binding.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as R
from conftest import load_pkg

TINY = R.tiny_clouds()
_CASES = {}
_REFS = {}


def case(name):
    if not _CASES:
        _CASES.update(R.cases())
    return _CASES[name]


def ref(name):
    if name not in _REFS:
        cam, bgr, depth, leaf = case(name)
        _REFS[name] = R.dense_ref(bgr, depth, R.CAMS[cam], leaf)
    return _REFS[name]


@pytest.mark.parametrize("name", sorted(TINY))
def test_numpy_equals_transcription(name):
    cloud, leaf = TINY[name]
    r = R.voxel_grid(cloud, leaf)
    keys, counts, pts = R.voxel_grid_py(cloud, leaf)
    assert r["status"] == R.CLOUD_OK and r["n_valid"] == len(cloud)
    assert np.array_equal(keys, r["keys"]) and np.all(np.diff(keys.astype(np.int64)) > 0)
    assert np.array_equal(counts, r["counts"]) and counts.sum() == len(cloud)
    assert np.array_equal(np.stack([pts[a] for a in "bgra"], 1), r["bgra"])
    got = np.stack([pts[a] for a in "xyz"], 1).astype(np.float64)
    assert np.all(np.abs(got - r["xyz64"]) <= R.centroid_bound(r))
    one = r["counts"] == 1
    assert np.array_equal(got[one].astype(np.float32).view(np.uint32), r["first"][one].view(np.uint32))


def test_tiny_clouds_cover_their_names():
    assert R.voxel_grid(*TINY["one_voxel"])["n_points"] == 1
    assert int(R.voxel_grid(*TINY["far"])["keys"].max()) >= 2**24
    cloud, leaf = TINY["lattice"]
    t = cloud["x"] * (np.float32(1) / np.float32(leaf))
    assert np.array_equal(t, np.floor(t)) and t.min() < 0 < t.max()
    assert R.voxel_grid(cloud, leaf)["n_points"] == len(cloud)  # every lattice point its own voxel


def test_transform_is_the_written_order():
    pts = np.zeros(1, R.CLOUD_DTYPE)
    pts["x"], pts["y"], pts["z"] = 1.0, 2.0**-24, -1.0
    T = np.eye(4, dtype=np.float32)
    T[0] = [1.0, 1.0, 1.0, 0.0]  # (1 + 2^-24) rounds to 1 first, so the sum is 0, not 2^-24
    assert R.transform(pts, T)["x"][0] == 0.0
    assert R.transform(pts, np.eye(4)).tobytes() == pts.tobytes()


def grid(name, frame=0):
    cam, bgr, depth, leaf = case(name)
    return R.grid_of(R.create_cloud(bgr[frame], depth[frame], R.CAMS[cam]), leaf)


def test_overflow_case_overflows():
    g = grid("random_overflow")
    assert g["d"][0] * g["d"][1] * g["d"][2] > R.INT32_MAX and not g["filtered"]
    r = ref("random_overflow")[0]
    assert r["status"] == R.CLOUD_UNFILTERED and r["n_points"] == r["n_valid"] == R.P
    g = grid("random_no_overflow")
    assert g["d"][0] * g["d"][1] * g["d"][2] <= R.INT32_MAX and g["filtered"]
    assert ref("random_no_overflow")[0]["status"] == R.CLOUD_OK


def test_all_key_bytes_case():
    assert int(ref("ramp_all_key_bytes")[0]["keys"].max()) == 806527978
    r = ref("ramp")[0]
    assert tuple(r["div_b"]) == (540, 219, 437) and int(r["keys"].max()) == 51679619
    assert int(ref("random_no_overflow")[0]["keys"].max()) >= 2**24


def test_heavy_voxel_cases():
    r = ref("heavy_four_voxels")[0]
    assert r["n_points"] == 4 and np.all(255 * r["counts"].astype(np.int64) >= 2**24)
    assert r["counts"].sum() == R.P
    r = ref("heavy_one_voxel")[0]
    assert r["n_points"] == 1 and r["counts"][0] == R.P and 255 * R.P >= 2**24


@pytest.mark.parametrize("name", ["boundary_unit_half", "boundary_unit_one", "boundary_centred_half", "boundary_centred_four"])
def test_boundary_cases(name):
    cam, bgr, depth, leaf = case(name)
    cloud = R.create_cloud(bgr[0], depth[0], R.CAMS[cam])
    inv = np.float32(1) / np.float32(leaf)
    assert np.all(cloud["z"] == cloud["z"][0])  # a depth plane
    for a in "xyz":
        t = cloud[a] * inv
        on = t == np.floor(t)  # on a voxel boundary: every point, or every fourth at leaf 4
        assert on.all() if leaf <= 1 else (np.any(on & (t < 0)) and np.any(on & (t > 0))) or a == "z"
    if cam == "centred":
        assert (cloud["x"] * inv).min() < 0 < (cloud["x"] * inv).max() and np.any(cloud["x"] == 0)
        assert (cloud["y"] * inv).min() < 0 < (cloud["y"] * inv).max()
    else:
        assert (cloud["x"] * inv).min() == 0 == (cloud["y"] * inv).min()
    r = ref(name)[0]
    per = max(1, int(leaf)) ** 2
    assert r["n_points"] * per == R.P and np.all(r["counts"] == per)


@pytest.mark.parametrize("k", R.VALID_COUNTS)
def test_valid_count_cases(k):
    _, _, depth, _ = case(f"valid_{k}")
    assert int((depth > 0).sum()) == k
    r = ref(f"valid_{k}")[0]
    assert r["n_valid"] == k and r["counts"].sum() == k
    if 1 < k < R.P:
        assert len(np.unique(np.nonzero(depth[0])[0])) > 1  # over more than one row


def test_ragged_batch_case():
    r = ref("ragged_batch")
    assert [q["n_valid"] > 0 for q in r] == [False, True, True] and r[2]["n_valid"] == 1
    assert r[0]["n_points"] == 0 and r[0]["status"] == R.CLOUD_OK and not r[0]["min_p"].any()
    assert r[1]["n_valid"] > R.P // 2


def test_leaf_zero_is_create_cloud():
    cam, bgr, depth, leaf = case("leaf_zero")
    for f, r in enumerate(ref("leaf_zero")):
        cloud = R.create_cloud(bgr[f], depth[f], R.CAMS[cam])
        assert r["status"] == R.CLOUD_UNFILTERED and r["n_points"] == len(cloud) and np.all(r["counts"] == 1)
        assert np.array_equal(r["first"], np.stack([cloud[a] for a in "xyz"], 1))


def test_library_exports_the_dense_cloud_calls():
    """Fails on a library without the feature."""
    pkg = load_pkg()
    lib = pkg.load()
    sig = pkg._abi.SIGNATURES
    P = C.c_void_p
    want = {"odo_dense_clouds": (C.c_int, [P, P, P, C.c_int, C.c_float, P, P]),
            "odo_dense_clouds_host": (C.c_int, [P, P, P, C.c_int, C.c_float, P, P]),
            "odo_get_dense_cloud": (C.c_int, [P, C.c_int, P, P, C.c_int, P]),
            "odo_dense_cloud_device": (C.c_int, [P, C.c_int, P, P, P])}
    for name, s in want.items():
        assert hasattr(lib, name), f"libodo_hip.so does not export {name}"
        assert sig[name] == s
        fn = getattr(lib, name)
        assert fn.restype is s[0] and list(fn.argtypes) == s[1]
    for m in ("dense_clouds", "dense_clouds_host", "get_dense_cloud", "dense_cloud_device"):
        assert callable(getattr(pkg.Odometry, m))
    assert pkg.CLOUD_DTYPE == R.CLOUD_DTYPE and pkg.CLOUD_DTYPE.itemsize == 16
    assert pkg.CLOUD_INFO_DTYPE.itemsize == C.sizeof(pkg._abi.CloudInfo) == 60
    assert (pkg.CLOUD_OK, pkg.CLOUD_UNFILTERED) == (R.CLOUD_OK, R.CLOUD_UNFILTERED)
    # the argument checks come before any device call
    buf = (C.c_uint8 * 64)()
    assert lib.odo_dense_clouds(None, buf, buf, 1, 0.03, None, buf) == -1
    assert lib.odo_dense_clouds_host(None, buf, buf, 1, 0.03, None, buf) == -1
    assert lib.odo_get_dense_cloud(None, 0, buf, None, 1, buf) == -1
    assert lib.odo_dense_cloud_device(None, 0, buf, None, buf) == -1
