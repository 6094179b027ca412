"""tests/knn_ref.py on the CPU: the bit-matmul reference against the oracle's
C loop and test_golden's numpy brute force on every case of
tests/test_knn2_gpu.py, and each descriptor family's defining condition on
the reference, so the GPU tests cannot go quietly vacuous."""
import numpy as np
import pytest

import knn_ref as K
import oracle_lib as O
from test_golden import _knn2_numpy

ALL_CASES = K.NT_CASES + K.NQ_CASES + K.CORNER_CASES + K.ONE_HOT_CASES + [("planted", K.POOL, 130)]
NUMPY_BYTES = 64 << 20  # _knn2_numpy's nq * nt * 32-byte intermediate
ids = lambda cases: [K.case_name(*c) for c in cases]


def _of(family, cases=ALL_CASES):
    return [c for c in cases if c[0] == family]


@pytest.mark.parametrize("family,nq,nt", ALL_CASES, ids=ids(ALL_CASES))
def test_reference_equals_oracle_and_numpy(family, nq, nt):
    """knn2_ref == oracle_knn2, and == _knn2_numpy where that fits in memory
    and has two neighbours to sort."""
    q, t, ri, rd = K.case(family, nq, nt)
    oi, od = O.knn2(q, t)
    assert K.first_mismatch(oi, od, ri, rd, K.case_name(family, nq, nt)) is None
    if nt >= 2 and nq * nt * 32 <= NUMPY_BYTES:
        ni, nd = _knn2_numpy(q, t)
        assert np.array_equal(ni, ri) and np.array_equal(nd, rd)


def test_reference_equals_oracle_large():
    """2305 x 8192: several query blocks of the reference against the largest
    FP4 train set, about 19 M comparisons."""
    q, t = K.random(2305, 8192, 1)
    ri, rd = K.knn2_ref(q, t)
    oi, od = O.knn2(q, t)
    assert np.array_equal(oi, ri) and np.array_equal(od, rd)


@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (3, 1), (1, 2)])
def test_reference_missing_neighbours(nq, nt):
    """nt < 2 leaves (-1, INT32_MAX) in the slots without a train."""
    q, t = K.random(nq, nt, 5)
    ri, rd = K.knn2_ref(q, t)
    assert ri.shape == rd.shape == (nq, 2) and ri.dtype == rd.dtype == np.int32
    assert (ri[:, min(nt, 2):] == -1).all() and (rd[:, min(nt, 2):] == K.INT32_MAX).all()
    assert (ri[:, :min(nt, 2)] >= 0).all() and (rd[:, :min(nt, 2)] <= 256).all()
    if nq:
        oi, od = O.knn2(q, t)
        assert np.array_equal(oi, ri) and np.array_equal(od, rd)


def test_shape_lists_straddle_the_constants():
    """Each step of both kernels has its value, one below and one above."""
    for step in (4, 16, 64, 128, 256, 384, 8192):
        assert {step - 1, step, step + 1} <= set(K.NT_EDGES), step
    for step in (16, 64, 256):
        assert {step - 1, step, step + 1} <= set(K.NQ_EDGES), step
    items = lambda nq: (nq + 255) // 256
    assert (items(1793), items(2049), items(2305)) == (8, 9, 10)  # the XCD branch from 8 items on
    for n in (9, 10):  # unequal per-XCD ranges
        assert len({n * (x + 1) // 8 - n * x // 8 for x in range(8)}) > 1
    assert all(any(c == (f, K.NQ_FOR_NT, nt) for c in K.NT_CASES) for f in K.FAMILIES for nt in K.NT_EDGES if nt >= 2)


@pytest.mark.parametrize("family,nq,nt", _of("all_far"), ids=ids(_of("all_far")))
def test_all_far_is_all_256(family, nq, nt):
    _, _, ri, rd = K.case(family, nq, nt)
    if nt == 1:
        assert (ri == [0, -1]).all() and (rd == [256, K.INT32_MAX]).all()
    else:
        assert (ri == [0, 1]).all() and (rd == 256).all()


@pytest.mark.parametrize("family,nq,nt", _of("all_equal"), ids=ids(_of("all_equal")))
def test_all_equal_is_all_ties(family, nq, nt):
    q, _, ri, rd = K.case(family, nq, nt)
    if nt == 1:
        assert (ri == [0, -1]).all() and (rd[:, 1] == K.INT32_MAX).all()
    else:
        assert (ri == [0, 1]).all() and (rd[:, 0] == rd[:, 1]).all()
    assert nq < 16 or len(np.unique(rd[:, 0])) > 4  # the queries do differ


@pytest.mark.parametrize("family,nq,nt", _of("planted"), ids=ids(_of("planted")))
def test_planted_top2_is_the_planted_pair(family, nq, nt):
    """Query i's top-2 is {a, b} of its group at distances (e, e) or
    (e, e + 1); a tie is ordered by index. At least a third of the queries
    are ties, and every group the shape has room for occurs."""
    _, _, ri, rd = K.case(family, nq, nt)
    plan, first = K.planted_plan(nt, K.case_seed(family, nq, nt))
    assert len(plan) == len(K.planted_pairs(nt)) >= 2
    ties = 0
    for i in range(nq):
        a, b, e, tie = plan[(first + i) % len(plan)]
        assert 1 <= e <= 8
        if tie:
            assert ri[i].tolist() == [min(a, b), max(a, b)] and rd[i].tolist() == [e, e], (i, a, b, e, tie)
            ties += 1
        else:
            assert ri[i].tolist() == [a, b] and rd[i].tolist() == [e, e + 1], (i, a, b, e, tie)
    assert 3 * ties >= nq
    if nq >= len(plan) >= 4:
        assert ties < nq, "no pair decided by distance"


def test_planted_pairs_cover_the_boundaries():
    assert K.planted_pairs(2) == [(0, 1), (1, 0)]
    assert K.planted_pairs(5) == [(3, 4), (4, 3), (0, 4), (4, 0)]
    assert K.planted_pairs(129) == [(3, 4), (4, 3), (15, 16), (16, 15), (127, 128), (128, 127), (0, 128), (128, 0)]
    assert K.planted_pairs(8449) == [(3, 4), (4, 3), (15, 16), (16, 15), (127, 128), (128, 127), (255, 256),
                                     (8447, 8448), (0, 8448), (8448, 0)]


@pytest.mark.parametrize("family,nq,nt", _of("extremes"), ids=ids(_of("extremes")))
def test_extremes_reach_0_and_the_last_index(family, nq, nt):
    """Every query has its exact copy among the trains, the even ones only at
    nt - 1; every query's complement (H = 256) is there too."""
    q, t, ri, rd = K.case(family, nq, nt)
    assert (rd[:, 0] == 0).all()
    assert (ri[::2, 0] == nt - 1).all() and nq >= 1
    pop = np.unpackbits(q, axis=1).sum(1)
    assert set(np.unique(pop)) <= {0, 1, 255, 256}
    tset = {x.tobytes() for x in t}
    assert all((~x).tobytes() in tset and x.tobytes() in tset for x in q)
    if nt == 2:
        assert (rd[:, 1] == 256).all()


def test_one_hot_counts_every_bit_once():
    _, _, ri, rd = K.case("one_hot", 256, 256)
    assert (ri[:, 0] == np.arange(256)).all() and (rd == [0, 2]).all()
    assert (ri[1:, 1] == 0).all() and ri[0, 1] == 1
    _, _, ri, rd = K.case("one_hot_complement", 256, 256)
    assert (rd == [254, 254]).all() and (ri[2:] == [0, 1]).all()
    assert ri[0].tolist() == [1, 2] and ri[1].tolist() == [0, 2]


@pytest.mark.parametrize("family,nq,nt", _of("few_values"), ids=ids(_of("few_values")))
def test_few_values_has_ties_at_several_distances(family, nq, nt):
    """From 16 trains on, nearly every query's two nearest are tied, at more
    than one distance, and neither 0 nor one value only."""
    _, _, ri, rd = K.case(family, nq, nt)
    tied = rd[:, 0] == rd[:, 1]
    assert (ri[tied, 0] < ri[tied, 1]).all()
    if nt >= 16:
        assert (rd[:, 0] == rd[:, 1]).mean() > 0.9 and len(np.unique(rd[:, 0])) >= 2 and rd.max() <= 14


def test_pooled_indexes_the_pool():
    pool = K.random(K.POOL, 1, 3)[0]
    q, sel = K.pooled(2 * K.POOL + 7, pool)
    assert q.shape == (2 * K.POOL + 7, 32) and np.array_equal(q[K.POOL + 5], pool[5]) and sel[K.POOL + 5] == 5
    # 4096 items of 256 queries: more than the 8 x 256 workgroups that can be resident
    assert ((1 << 20) - 3 + 255) // 256 == 4096 > 8 * 256
