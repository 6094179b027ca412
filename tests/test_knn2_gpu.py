"""The kNN-2 Hamming kernels against the bit-matmul reference at edge shapes.

k_knn2_f4 (FP4 matrix cores, the default form) and k_knn2 (VALU:
forms={"knn": 1}, and the entry point's choice for train sets above 8192),
both through odo_knn2_hamming, against tests/knn_ref.py's knn2_ref. The cases
and the conditions that make them worth running are checked on the CPU by
tests/test_knn_ref.py. Indices and distances are integers: every comparison
is np.array_equal, and the outputs start as a canary so an unwritten slot
fails.
"""
import numpy as np
import pytest

import knn_ref as K
from conftest import load_pkg

pytestmark = pytest.mark.gpu

ODO_ERR_CAPACITY = -3  # include/odo.h
ids = lambda cases: [K.case_name(*c) for c in cases]


@pytest.fixture(scope="module", params=["fp4", "valu"])
def ctx(request):
    """One 640x480, max_batch = 1 context per kernel form."""
    pkg = load_pkg()
    forms = {"knn": pkg.KNN_FORM_VALU} if request.param == "valu" else None
    odo = pkg.Odometry(pkg.default_config(640, 480, 1, forms=forms))
    yield pkg, odo, request.param
    odo.close()


def _knn2(ctx, q, t, nq=None, nt=None):
    pkg, odo, _ = ctx
    nq = len(q) if nq is None else nq
    nt = len(t) if nt is None else nt
    gi = np.full((len(q), 2), K.CANARY, np.int32)
    gd = np.full((len(q), 2), K.CANARY, np.int32)
    rc = pkg.load().odo_knn2_hamming(odo.h, pkg.ptr(q), nq, pkg.ptr(t), nt, pkg.ptr(gi), pkg.ptr(gd))
    return rc, gi, gd


def _check(ctx, family, nq, nt):
    q, t, ri, rd = K.case(family, nq, nt)
    rc, gi, gd = _knn2(ctx, q, t)
    assert rc == 0, f"odo_knn2_hamming returned {rc}"
    bad = K.first_mismatch(gi, gd, ri, rd, f"{K.case_name(family, nq, nt)} ({ctx[2]})")
    assert bad is None, bad


@pytest.mark.parametrize("family,nq,nt", K.NT_CASES, ids=ids(K.NT_CASES))
def test_train_count_edges(ctx, family, nq, nt):
    """nt around the lane group (4), tile (16), chunk (128 FP4, 256 VALU) and
    the 8192 form switch, 65 queries (a full wave and one query of the next):
    full and tail chunks, pad rows against the largest real key (all_far, H =
    256), ties on the index in every comparison (all_equal, few_values) and
    across each boundary in both orders (planted), H = 0 at the last index
    (extremes). On the FP4 context nt > 8192 runs the VALU kernel."""
    _check(ctx, family, nq, nt)


@pytest.mark.parametrize("family,nq,nt", K.NQ_CASES, ids=ids(K.NQ_CASES))
def test_query_count_edges(ctx, family, nq, nt):
    """nq around the query tile (16), wave (64) and item (256) against 129
    trains (a full chunk and a one-train tail); 1793, 2049 and 2305 queries
    are 8, 9 and 10 items: the FP4 kernel's per-XCD item order, equal and
    unequal ranges."""
    _check(ctx, family, nq, nt)


@pytest.mark.parametrize("family,nq,nt", K.CORNER_CASES, ids=ids(K.CORNER_CASES))
def test_form_switch_corner(ctx, family, nq, nt):
    """257 queries against 8192 and 8193 trains. 8192 is the last size of the
    FP4 form: the copy at index 8191 (extremes) is the largest index its key
    holds. At 8193 the FP4 context falls back to the VALU kernel on its own
    and has to return index 8192."""
    _check(ctx, family, nq, nt)
    if family == "extremes":
        assert (K.case(family, nq, nt)[2][::2, 0] == nt - 1).all()


@pytest.mark.parametrize("family,nq,nt", K.ONE_HOT_CASES, ids=ids(K.ONE_HOT_CASES))
def test_one_hot_bit_permutation(ctx, family, nq, nt):
    """Each of the 256 bit positions counted exactly once and by the same
    permutation on both operands: H is 0 / 2 (256 / 254 complemented)."""
    _check(ctx, family, nq, nt)


def test_grid_stride_over_items(ctx):
    """2^20 - 3 queries (the entry point takes 2^20) are 4096 items, more
    than one round of resident workgroups whatever the occupancy (at most 8
    on each of 256 CUs), so workgroups loop over several items, the last one
    partial; 130 trains with planted pairs. The queries repeat a pool of 509."""
    nq, nt = (1 << 20) - 3, 130
    pool, t, ri, rd = K.case("planted", K.POOL, nt)
    q, sel = K.pooled(nq, pool)
    rc, gi, gd = _knn2(ctx, q, t)
    assert rc == 0, f"odo_knn2_hamming returned {rc}"
    bad = K.first_mismatch(gi, gd, ri[sel], rd[sel], f"pooled planted {nq}x{nt} ({ctx[2]})")
    assert bad is None, bad


def test_capacity_then_a_small_case(ctx):
    """2^20 + 1 queries or trains are refused with ODO_ERR_CAPACITY before
    any buffer is read or written, and the context then answers as before."""
    q, t, _, _ = K.case("random", 65, 129)
    for nq, nt in (((1 << 20) + 1, 129), (65, (1 << 20) + 1)):
        rc, gi, gd = _knn2(ctx, q, t, nq, nt)
        assert rc == ODO_ERR_CAPACITY, (nq, nt, rc)
        assert (gi == K.CANARY).all() and (gd == K.CANARY).all()
    _check(ctx, "random", 65, 129)
