"""Independent kNN-2 Hamming reference and the edge cases of the matcher tests.

knn2_ref shares no code or method with the oracle's xor-and-popcount loop or
with test_golden._knn2_numpy: descriptors are unpacked to 0/1 matrices and
H = pop(q) + pop(t) - 2 Q T^T comes out of a float64 matmul (values <= 256,
exact). The two smallest (H, index) keys per query, the lower train index
first on a tie (cv::BFMatcher's order), a missing neighbour (-1, INT32_MAX) as
at the C-ABI (include/odo.h).

Shapes are named after the kernel constants they straddle; descriptor
families are functions of (nq, nt, seed) returning (q, t). The conditions
that make each family worth running are asserted on the reference by
tests/test_knn_ref.py (CPU); tests/test_knn2_gpu.py runs the kernels.
"""
import functools
import zlib

import numpy as np

INT32_MAX = 0x7FFFFFFF
CANARY = 0x5A5A5A5A  # pre-fill of the output arrays: an unwritten slot fails

# FP4 form (k_knn2_f4): 4 trains per lane group, 16 per tile, 128 per LDS
# chunk. VALU form (k_knn2): 4 trains interleaved, 256 per chunk. 8192 is the
# switch between the forms at the entry point (13-bit index in the FP4 key);
# 8449 = 8192 + 257. Run at nq = NQ_FOR_NT.
NT_EDGES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385,
            8191, 8192, 8193, 8449]
NQ_FOR_NT = 65
# 16 queries per tile, 64 per wave, 256 per item. 1793 = 8 items, the first
# grid that takes the per-XCD item order; 2049 and 2305 = 9 and 10 items,
# unequal per-XCD ranges (one, then two XCDs with two items). Run at
# nt = NT_FOR_NQ.
NQ_EDGES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1793, 2049, 2305]
NT_FOR_NQ = 129
CORNERS = [(257, 8192), (257, 8193)]  # more than one item on both sides of the switch
POOL = 509  # distinct queries of the grid-stride case (a prime: no item holds the same 256)


# --------------------------------------------------------------- the reference
def knn2_ref(q, t, block=512):
    """Brute-force top-2 by bit matmul. Returns int32 idx[nq, 2], dist[nq, 2]."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), INT32_MAX, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    assert nt <= 1 << 21
    tb = np.unpackbits(t, axis=1).astype(np.float64)
    pt = tb.sum(1)
    k = min(2, nt)
    j = np.arange(nt, dtype=np.int64)
    for b in range(0, nq, block):
        qb = np.unpackbits(q[b:b + block], axis=1).astype(np.float64)
        h = qb.sum(1)[:, None] + pt[None, :] - 2.0 * (qb @ tb.T)
        key = h.astype(np.int64) * (1 << 21) + j[None, :]  # ordered as (H, index)
        best = np.partition(key, tuple(range(k)), axis=1)[:, :k]
        idx[b:b + block, :k] = best & ((1 << 21) - 1)
        dist[b:b + block, :k] = best >> 21
    return idx, dist


def first_mismatch(gi, gd, ri, rd, name):
    """None if (gi, gd) == (ri, rd), else a line naming the first differing
    query with its reference and returned (idx, dist)."""
    gi, gd, ri, rd = (np.asarray(a).reshape(-1, 2) for a in (gi, gd, ri, rd))
    if gi.shape != ri.shape or gd.shape != rd.shape:
        return f"{name}: shapes {gi.shape} {gd.shape} vs reference {ri.shape} {rd.shape}"
    bad = np.nonzero((gi != ri).any(1) | (gd != rd).any(1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (f"{name}: {bad.size} of {len(ri)} queries differ, first query {i}: reference idx {ri[i].tolist()} "
            f"dist {rd[i].tolist()}, returned idx {gi[i].tolist()} dist {gd[i].tolist()}")


# ------------------------------------------------------------------- families
def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def random(nq, nt, seed):
    rng = np.random.default_rng(seed)
    return _rand(rng, nq), _rand(rng, nt)


def extremes_pool(nt, seed):
    """All-zero, all-ones and one-bit neighbours, closed under complement; as
    many one-bit pairs (up to 3) as nt has room for."""
    rng = np.random.default_rng(seed)
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    pool = [z, o]
    for b in rng.choice(256, min(3, (nt - 2) // 2), replace=False):
        pool += [_flip(z, [b]), _flip(o, [b])]
    return np.stack(pool)


def extremes(nq, nt, seed):
    """Queries from extremes_pool; most trains random; every pool member (so
    every query's exact copy, H = 0, and complement, H = 256) among the trains,
    one member's only copy at index nt - 1: the even queries are that member."""
    assert nt >= 2
    rng = np.random.default_rng(seed + 1)
    pool = extremes_pool(nt, seed)
    n = len(pool)
    last = seed % n
    t = _rand(rng, nt)
    others = [m for m in range(n) if m != last]
    t[rng.choice(nt - 1, n - 1, replace=False)] = pool[others]
    t[nt - 1] = pool[last]
    i = np.arange(nq)
    q = pool[np.where(i % 2 == 0, last, np.asarray(others + [last])[(i // 2) % n])]
    return q, t


def all_far(nq, nt, seed):
    """Every query one descriptor, every train its complement: every distance
    is 256, the largest real key, and the answer (0, 1)."""
    d = _rand(np.random.default_rng(seed), 1)
    return np.repeat(d, nq, 0), np.repeat(~d, nt, 0)


def all_equal(nq, nt, seed):
    """Identical trains, random queries: every comparison is a tie."""
    rng = np.random.default_rng(seed)
    return _rand(rng, nq), np.repeat(_rand(rng, 1), nt, 0)


def few_values(nq, nt, seed):
    """Descriptors drawn from 4 values a few bits apart, the trains from 3 of
    them: massive ties at several distances, a quarter of the queries with no
    exact copy."""
    rng = np.random.default_rng(seed)
    base = _rand(rng, 1)[0]
    v = np.stack([_flip(base, rng.choice(256, k, replace=False)) for k in (0, 3, 5, 9)])
    return v[rng.integers(0, 4, nq)], v[(seed + 1 + rng.integers(0, 3, nt)) % 4]


def planted_pairs(nt):
    """The ordered boundary pairs (a, b) that fit in nt: across a lane group
    (3|4), a tile (15|16), an FP4 chunk (127|128), a VALU chunk (255|256), the
    tail (nt-2|nt-1) and the whole range, in both orders where both exist."""
    cand = [(3, 4), (4, 3), (15, 16), (16, 15), (127, 128), (128, 127), (255, 256), (nt - 2, nt - 1),
            (0, nt - 1), (nt - 1, 0)]
    out = []
    for a, b in cand:
        if 0 <= a < nt and 0 <= b < nt and a != b and (a, b) not in out:
            out.append((a, b))
    return out


def planted_plan(nt, seed):
    """(plan, first): per group g (a, b, e, tie), and the group of query 0
    (query i belongs to group (first + i) % len(plan)). The nearest train is a
    at distance e, the second b at e (tie: the order is the index's) or e + 1.
    A pair and its reverse share e and tie. Two thirds of the position pairs
    tie, one of them (by seed) always, and query 0 is one of its queries; one
    pair at least, where there are two, is decided by distance."""
    pairs = planted_pairs(nt)
    classes = []
    for a, b in pairs:
        if (min(a, b), max(a, b)) not in classes:
            classes.append((min(a, b), max(a, b)))
    n = len(classes)
    always = seed % n
    by_dist = {c for c in range(n) if (c + seed) % 3 == 0 and c != always}
    if not by_dist and n > 1:
        by_dist = {(always + 1) % n}
    plan = []
    for a, b in pairs:
        c = classes.index((min(a, b), max(a, b)))
        plan.append((a, b, 1 + (c + seed) % 8, c not in by_dist))
    first = [min(a, b) for a, b, _, _ in plan].index(classes[always][0])
    return plan, first


def planted(nq, nt, seed):
    """Random trains; the queries of group g are one descriptor whose copy with
    e bits flipped sits at a_g and one with e (or e + 1) bits flipped at b_g.
    Each group flips bits of its own 24-bit range, so a train planted for
    another group that shares a position stays further away than both."""
    assert nt >= 2
    rng = np.random.default_rng(seed)
    t = _rand(rng, nt)
    plan, first = planted_plan(nt, seed)
    fixed, fwd, gq = set(), {}, []
    for g, (a, b, e, tie) in enumerate(plan):
        if (b, a) in fwd:
            # the reverse of an earlier group, which left t_b = q0 ^ A and
            # t_a = q0 ^ B (|A| = e <= |B|, disjoint): q0 ^ A ^ B is e from t_a
            # and |B| from t_b
            gq.append(_flip(t[a], fwd[b, a]))
            continue
        assert not (a in fixed and b in fixed), "both positions planted by unrelated groups"
        A = list(range(24 * g, 24 * g + e))
        B = list(range(24 * g + 12, 24 * g + 12 + e + (0 if tie else 1)))
        if a in fixed:
            qd = _flip(t[a], A)
            t[b] = _flip(qd, B)
        elif b in fixed:
            qd = _flip(t[b], B)
            t[a] = _flip(qd, A)
        else:
            qd = _rand(rng, 1)[0]
            t[a], t[b] = _flip(qd, A), _flip(qd, B)
        fixed |= {a, b}
        fwd[a, b] = A
        gq.append(qd)
    q = np.stack(gq)[(first + np.arange(nq)) % len(plan)]
    return q, t


def one_hot(complement=False):
    """q[i] has only bit i set, t[j] only bit j (256 x 256): H = 0 on the
    diagonal, else 2. Every bit position counts exactly once, by the same
    permutation on both operands. complement: ~t, H = 256 / 254."""
    q = np.zeros((256, 32), np.uint8)
    i = np.arange(256)
    q[i, i >> 3] = (1 << (i & 7)).astype(np.uint8)
    return q, (~q if complement else q.copy())


FAMILIES = {"random": random, "extremes": extremes, "all_far": all_far, "all_equal": all_equal,
            "planted": planted, "few_values": few_values}
MIN_NT = {"extremes": 2, "planted": 2}  # a copy and a complement / two planted trains


def fits(family, nq, nt):
    return nt >= MIN_NT.get(family, 1)


def case_name(family, nq, nt):
    return f"{family}-{nq}x{nt}"


def case_seed(family, nq, nt):
    return zlib.crc32(case_name(family, nq, nt).encode()) & 0xFFFF


@functools.lru_cache(maxsize=None)
def case(family, nq, nt):
    """(q, t, ref_idx, ref_dist) of one case, computed once and shared; the
    arrays are read-only."""
    seed = case_seed(family, nq, nt)
    if family.startswith("one_hot"):
        assert (nq, nt) == (256, 256)
        q, t = one_hot(family == "one_hot_complement")
    else:
        q, t = FAMILIES[family](nq, nt, seed)
    assert q.shape == (nq, 32) and t.shape == (nt, 32) and q.dtype == t.dtype == np.uint8
    q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
    ri, rd = knn2_ref(q, t)
    for a in (q, t, ri, rd):
        a.setflags(write=False)
    return q, t, ri, rd


NT_CASES = [(f, NQ_FOR_NT, nt) for f in FAMILIES for nt in NT_EDGES if fits(f, NQ_FOR_NT, nt)]
NQ_CASES = [(f, nq, NT_FOR_NQ) for f in ("random", "planted") for nq in NQ_EDGES]
CORNER_CASES = [(f, nq, nt) for nq, nt in CORNERS for f in ("random", "extremes", "all_equal")]
ONE_HOT_CASES = [("one_hot", 256, 256), ("one_hot_complement", 256, 256)]


def pooled(nq, pool):
    """pool[i % len(pool)] for i < nq, and the index to take a reference
    computed on the pool through: a million queries cost the CPU nothing."""
    sel = np.arange(nq) % len(pool)
    return np.ascontiguousarray(pool[sel]), sel
