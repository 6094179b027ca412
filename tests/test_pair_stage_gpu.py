"""The pair-match stage on crafted features against tests/pair_ref.py.

odo_debug_match_features runs the batch path's own launches (k_vo_lm, kNN-2
over the landmark query list in the context's form and split count,
k_pair_match, k_latch) on host features. Every case of pair_ref.CASES runs in
the FP4 form and in the VALU form with 1, 2, 3 and 8 train splits; what each
case is for is asserted on the CPU by tests/test_pair_ref.py. Every comparison
is exact (np.array_equal; the latch by its bits), and every output starts as a
canary, so a slot the stage should have left alone, or failed to write, fails.

The depth filter's query side and k_latch's "source z == 0" skip cannot be
reached here or in the batch path: a query is a VO landmark, whose depth is a
positive number by selection (test_pair_ref.py asserts it on the filter cases).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pair_ref as R
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

FILL = 0x5A
FORMS = {"fp4": dict(knn=0), "valu1": dict(knn=1, knn_split=1), "valu2": dict(knn=1, knn_split=2),
         "valu3": dict(knn=1, knn_split=3), "valu8": dict(knn=1, knn_split=8)}
_CTX = {}


def ctx_for(form, cfg):
    """One 640x480, nfeatures = 1000 context per form and configuration, kept for the module."""
    key = (form, cfg["ratio"], cfg["check_depth"], cfg["min_inl"], cfg["max_batch"])
    if key not in _CTX:
        pkg = load_pkg()
        c = pkg.default_config(640, 480, cfg["max_batch"], nfeatures=1000, forms=FORMS[form])
        c.nn_ratio = cfg["ratio"]
        c.ransac.check_depth = cfg["check_depth"]
        c.ransac.min_inlier_th = cfg["min_inl"]
        _CTX[key] = pkg.Odometry(c)
        assert _CTX[key].kp_capacity() == R.KP_CAP
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for odo in _CTX.values():
        odo.close()
    _CTX.clear()


def canary(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def check_outputs(case, out, tag):
    """Every output of every pair against the reference; the rest still canary."""
    frames = case["frames"]
    for p, r in enumerate(case["pairs"]):
        n1, n2 = len(frames[p][0]), len(frames[p + 1][0])
        t = f"{tag} pair {p}"
        assert np.array_equal(out["lm_flags"][p, :n1], r["flags"]), f"{t}: landmark flags"
        assert canary(out["lm_flags"][p, n1:]), f"{t}: flags written past the frame"
        nq = len(r["qlist"])
        assert out["qcnt"][p] == nq, f"{t}: {out['qcnt'][p]} landmark queries, reference {nq}"
        assert np.array_equal(out["qlist"][p, :nq], r["qlist"]), f"{t}: query list"
        assert canary(out["qlist"][p, nq:]), f"{t}: query list written past its count"
        bad = R.knn_ref.first_mismatch(out["knn_idx"][p][r["qlist"]], out["knn_dist"][p][r["qlist"]],
                                       r["knn_idx"], r["knn_dist"], f"{t}: kNN-2 at the keypoint index")
        assert bad is None, bad
        rest = np.ones(R.KP_CAP, bool)
        rest[r["qlist"]] = False
        assert canary(out["knn_idx"][p][rest]) and canary(out["knn_dist"][p][rest]), \
            f"{t}: kNN-2 output at a keypoint that is no landmark"
        for name, cnt in (("matches", "n_matches"), ("good", "n_good")):
            n = len(r[name])
            assert out[cnt][p] == n, f"{t}: {cnt} {out[cnt][p]}, reference {n}"
            got, ref = out[name][p, :n], r[name].astype(out[name].dtype)
            assert np.array_equal(got, ref), f"{t}: {name} differ first at {np.nonzero(got != ref)[0][:4]}"
            assert canary(out[name][p, n:]), f"{t}: {name} written past the count"
        assert np.array_equal(out["f2_src"][p, :n2], r["f2_src"]), \
            f"{t}: f2_src differs at trains {np.nonzero(out['f2_src'][p, :n2] != r['f2_src'])[0][:8]}"
        assert canary(out["f2_src"][p, n2:]), f"{t}: f2_src written past the frame"
    got = float(out["latch"][0])
    if np.isnan(case["latch"]):
        assert np.isnan(got), f"{tag}: latch {got!r}, reference NaN"
    else:
        O.assert_same_bits(got, case["latch"], f"{tag}: latch", np.float64)


def run_case(form, name):
    case = R.pair_case(name)
    odo = ctx_for(form, case["cfg"])
    assert np.isnan(odo.latch), "the context does not start unlatched"
    if not np.isnan(case["cfg"]["latch"]):
        odo.set_latch(case["cfg"]["latch"])
    out = odo.match_features(case["frames"], FILL)
    check_outputs(case, out, f"{name} ({form})")
    return odo, out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", R.CASES)
def test_case(form, name):
    """Landmark selection (lm-*), the query list (ql-*), train counts and
    splits (nt-*, split-*), the ratio boundary, train slots, the two scans
    (nm-*, ng-*), the depth filter, the sort inside the stage with the heap
    branch (sort-killer-*), and the latch (latch-*)."""
    run_case(form, name)


def test_runs_of_items_in_one_workgroup():
    """63 pairs x 5 query blocks x 8 splits = 2520 kNN-2 items on a
    max_batch = 64 context, more than a round of 8 workgroups on each of 256
    CUs: workgroups carry runs of consecutive splits of one query block and
    flush() writes empties into the splits after the first. (A frame is the
    train of one pair and the query of the next, so both sides have 1025
    keypoints.)"""
    run_case("valu8", R.RUNS_CASE)


def test_context_is_reset_after_the_call(pkg):
    """A preset latch is read by the call and gone after it, and a tracked
    batch then gives what it gives on a fresh context."""
    case = R.pair_case("latch-preset")
    odo, out = run_case("fp4", "latch-preset")
    assert out["latch"][0] == 0.125 and np.isnan(odo.latch)
    bgr, dep, _ = sequence(2)
    got = odo.track_batch_host(bgr, dep)
    fresh = pkg.Odometry(pkg.default_config(640, 480, case["cfg"]["max_batch"], nfeatures=1000))
    ref = fresh.track_batch_host(bgr, dep)
    assert got.tobytes() == ref.tobytes()
    assert got[0]["n_matches"] == 0 and got[1]["n_matches"] >= 20
    O.assert_same_bits(odo.latch, fresh.latch, "latch after a tracked batch", np.float64)
    fresh.close()
    odo.reset()


def test_bad_arguments_are_refused_with_the_outputs_untouched(pkg):
    """A count above the capacity (ODO_ERR_CAPACITY) and null pointers
    (ODO_ERR_ARG) return before anything is written; the context then answers a
    small case as before."""
    name = "nm-20"
    case = R.pair_case(name)
    odo = ctx_for("valu2", case["cfg"])
    lib, kc = pkg.load(), odo.kp_capacity()
    desc = np.zeros((2, kc, 32), np.uint8)
    xyz = np.ones((2, kc, 3), np.float32)

    def call(counts, d=desc, x=xyz, n=2, null_out=None, no_out=False):
        out, st = odo.match_features_buffers(n, FILL)
        if null_out:
            setattr(st, null_out, None)
        counts = np.asarray(counts, np.int32)
        rc = lib.odo_debug_match_features(odo.h, n, pkg.ptr(counts), None if d is None else pkg.ptr(d),
                                          None if x is None else pkg.ptr(x), None if no_out else C.byref(st))
        assert all(canary(a) for a in out.values()), "an output was written by a refused call"
        return rc

    assert call([10, kc + 1]) == pkg._abi.ERR_CAPACITY
    assert call([kc + 1, 10]) == pkg._abi.ERR_CAPACITY
    assert call([10, -1]) == pkg._abi.ERR_ARG
    assert call([10, 10], d=None) == pkg._abi.ERR_ARG
    assert call([10, 10], x=None) == pkg._abi.ERR_ARG
    assert call([10, 10], no_out=True) == pkg._abi.ERR_ARG
    assert call([10, 10], null_out="f2_src") == pkg._abi.ERR_ARG
    assert call([10, 10], null_out="latch") == pkg._abi.ERR_ARG
    assert call([10], n=1) == pkg._abi.ERR_ARG
    assert call([10] * 4, n=4) == pkg._abi.ERR_ARG  # max_batch + 1 = 3 frames at most
    assert lib.odo_debug_match_features(None, 2, None, None, None, None) == pkg._abi.ERR_ARG
    run_case("valu2", name)


@pytest.mark.parametrize("name,keys", R.SORT_ALONE, ids=[n for n, _ in R.SORT_ALONE])
def test_sort_alone_at_the_depth_limit(pkg, name, keys):
    """odo_debug_sort on McIlroy's adversary inputs: ranges reach depth 0 and
    block_gnu_sort heap-sorts them (gnu_heap_select + gnu_sort_heap over
    gnu_adjust_heap, odo_select.h). The
    reference is pair_ref.std_sort, which test_pair_ref.py holds against the
    real std::sort on these very inputs."""
    keys = np.array(keys(), np.float32)
    n = len(keys)
    perm, heaps = R.std_sort(keys.tolist())
    assert heaps
    m = np.zeros(n, O.DMATCH_DTYPE)
    m["queryIdx"] = np.arange(n)
    m["distance"] = keys
    got = np.full(n, FILL, O.DMATCH_DTYPE)
    odo = ctx_for("fp4", R.pair_case("nm-20")["cfg"])
    pkg.check(pkg.load().odo_debug_sort(odo.h, pkg.ptr(m), n, pkg.ptr(got)))
    assert np.array_equal(got["queryIdx"], perm), "permutation differs from std::sort"
    assert np.array_equal(got["distance"], keys[perm])
