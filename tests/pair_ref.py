"""Independent reference of the pair-match stage and the cases its tests run.

The stage (k_vo_lm, kNN-2 over the landmark query list, k_pair_match, k_latch;
reached through odo_debug_match_features) restated in numpy and plain Python:
no GPU and no oracle calls. tests/test_pair_ref.py checks every piece against
the oracle and every case for what it is named after; tests/test_pair_stage_gpu.py
runs the kernels on the cases.

  vo_landmarks   Tracking::UpdateLastFrame (tracking.cpp:146-190): the K
                 smallest (z, index) among z > 0, K = min(valid, max(#(z <= th) + 1, 101))
  ratio_match    Matcher::KnnMatch (matcher.cpp:62-85) on knn_ref.knn2_ref, the
                 ratio test in float32, the last accepting query owns a train
  depth_filter   ransac.cpp:175-189, order preserved
  std_sort       libstdc++'s std::sort, sequentially: __introsort_loop
                 (threshold 16, median of three to first, unguarded Hoare
                 partition, depth limit 2 floor(log2 n)), __partial_sort's
                 __heap_select + __sort_heap at depth 0, __final_insertion_sort
  killer         McIlroy's adversary ("A Killer Adversary for Quicksort", 1999)
                 run against std_sort: inputs that reach the depth limit
  latch          Ransac::DepthCovariance's first-call latch (ransac.cpp:416-421)

Exact Hamming distances come from a code with pairwise distance 128: the rows
of the 256-bit Sylvester Hadamard matrix and their complements (CODE). Row j
with its first d <= 63 bits flipped is at distance d from row j and at least
65 from every other code word.
"""
import functools

import numpy as np

import knn_ref

INT32_MAX = knn_ref.INT32_MAX
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
# odo_default_config's FR1 calibration: mThDepth = mbf * th_depth / fx in float
TH_DEPTH = np.float32(40.0) * np.float32(40.0) / np.float32(517.3)
KP_CAP = 1088  # odo_kp_capacity at nfeatures = 1000
SPLITS = (1, 2, 3, 8)  # the VALU form's knn_split values the GPU test runs


# ------------------------------------------------------------- VO landmarks
def vo_landmarks(xyz, th=TH_DEPTH):
    """(flags uint8[n], qlist int32[K] ascending)."""
    z = np.asarray(xyz, np.float32).reshape(-1, 3)[:, 2]
    order = sorted((float(v), i) for i, v in enumerate(z) if v > 0)
    within = sum(1 for v, _ in order if np.float32(v) <= np.float32(th))
    k = min(len(order), max(within + 1, 101))
    flags = np.zeros(len(z), np.uint8)
    for _, i in order[:k]:
        flags[i] = 1
    return flags, np.nonzero(flags)[0].astype(np.int32)


# ------------------------------------------------------- ratio test, slots
def ratio_match(ki, kd, qlist, ratio, n2):
    """(matches in query order, f2_src). ki / kd: kNN-2 rows of the queries of
    qlist; an absent neighbour is (-1, INT32_MAX)."""
    m, src = [], np.full(n2, -1, np.int32)
    r = np.float32(ratio)
    for row, q in enumerate(qlist):
        if ki[row, 0] < 0:
            continue
        d0, d1 = np.float32(kd[row, 0]), np.float32(kd[row, 1])
        if d0 < np.float32(r * d1):
            m.append((int(q), int(ki[row, 0]), 0, d0))
            src[ki[row, 0]] = q  # queries ascend: the largest accepting one stays
    return np.array(m, DMATCH_DTYPE), src


def depth_filter(matches, xyz1, xyz2, check_depth):
    """Indices into matches of the good ones (ransac.cpp:175-189)."""
    keep = []
    for k, m in enumerate(matches):
        zs, zt = xyz1[m["queryIdx"], 2], xyz2[m["trainIdx"], 2]
        if check_depth and (np.isnan(zs) or np.isnan(zt) or zs <= 0 or zt <= 0):
            continue
        keep.append(k)
    return np.array(keep, np.int64)


# ------------------------------------------------------------ std::sort
def _std_sort_items(a, lt, depth=None):
    """libstdc++ std::sort of list a in place under lt(x, y); returns the sizes
    of the ranges that took the heap branch (__partial_sort at depth 0).
    depth: the depth limit in place of 2 floor(log2 n)."""
    n, heaps = len(a), []

    def adjust_heap(first, hole, length, value):
        top, child = hole, hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if lt(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if length % 2 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        while hole > top and lt(a[first + (hole - 1) // 2], value):  # __push_heap
            a[first + hole] = a[first + (hole - 1) // 2]
            hole = (hole - 1) // 2
        a[first + hole] = value

    def partial_sort(first, middle, last):
        length = middle - first
        if length >= 2:  # __make_heap
            for parent in range((length - 2) // 2, -1, -1):
                adjust_heap(first, parent, length, a[first + parent])
        for i in range(middle, last):  # __heap_select
            if lt(a[i], a[first]):
                v, a[i] = a[i], a[first]
                adjust_heap(first, 0, length, v)
        while middle - first > 1:  # __sort_heap
            middle -= 1
            v, a[middle] = a[middle], a[first]
            adjust_heap(first, 0, middle - first, v)

    def median_to_first(res, x, y, z):
        if lt(a[x], a[y]):
            pick = y if lt(a[y], a[z]) else (z if lt(a[x], a[z]) else x)
        elif lt(a[x], a[z]):
            pick = x
        else:
            pick = z if lt(a[y], a[z]) else y
        a[res], a[pick] = a[pick], a[res]

    def partition(first, last, pivot):
        while True:
            while lt(a[first], a[pivot]):
                first += 1
            last -= 1
            while lt(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            a[first], a[last] = a[last], a[first]
            first += 1

    def introsort_loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                partial_sort(first, last, last)
                heaps.append(last - first)
                return
            depth -= 1
            median_to_first(first, first + 1, first + (last - first) // 2, last - 1)
            cut = partition(first + 1, last, first)
            introsort_loop(cut, last, depth)
            last = cut

    def linear_insert(i):  # __unguarded_linear_insert
        v = a[i]
        while lt(v, a[i - 1]):
            a[i] = a[i - 1]
            i -= 1
        a[i] = v

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if lt(a[i], a[first]):
                v = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = v
            else:
                linear_insert(i)

    if n:
        introsort_loop(0, n, 2 * (n.bit_length() - 1) if depth is None else depth)
        if n > 16:
            insertion_sort(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion_sort(0, n)
    return heaps


def std_sort(keys):
    """(permutation, heap range sizes): out[k] = input position of the element
    std::sort leaves at k, elements compared by key only."""
    a = [(k, i) for i, k in enumerate(keys)]
    heaps = _std_sort_items(a, lambda x, y: x[0] < y[0])
    return [i for _, i in a], heaps


def heap_sort(keys):
    """The permutation std::__partial_sort(first, last, last) leaves (the
    introsort's depth-0 branch on a whole range)."""
    a = [(k, i) for i, k in enumerate(keys)]
    _std_sort_items(a, lambda x, y: x[0] < y[0], depth=0)
    return [i for _, i in a]


@functools.lru_cache(maxsize=None)
def killer(n):
    """McIlroy's adversary against std_sort: a permutation of 0..n-1 (tuple)
    on which the introsort spends its depth."""
    gas = float("inf")
    val, state = [gas] * n, {"solid": 0, "cand": 0}

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            f = x if x == state["cand"] else y
            val[f] = state["solid"]
            state["solid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    _std_sort_items(list(range(n)), lt)
    for i in range(n):
        if val[i] == gas:
            val[i] = state["solid"]
            state["solid"] += 1
    assert sorted(val) == list(range(n))
    return tuple(val)


def killer_few(n, k):
    """killer(n) // k: the same shape with n / k distinct values."""
    return tuple(v // k for v in killer(n))


# ------------------------------------------------------------------ latch
def latch_ref(pairs, xyz, min_inl, preset=float("nan")):
    """pairs: per pair dict(matches, good); xyz[i]: frame i's points. The
    first sorted good match with z1 != 0 and x2 != 0 of the first pair past
    the gates whose depths are both numbers; a latch that holds a value is kept."""
    if not np.isnan(preset):
        return float(preset)
    for p, r in enumerate(pairs):
        if len(r["matches"]) < 20 or len(r["matches"]) < min_inl or len(r["good"]) < min_inl:
            continue
        for m in r["good"]:
            z1, x2 = xyz[p][m["queryIdx"], 2], xyz[p + 1][m["trainIdx"], 0]
            if z1 == 0 or x2 == 0:  # ComputeInliersAndError, ransac.cpp:326 (sic: target.x)
                continue
            if np.isnan(z1) or np.isnan(xyz[p + 1][m["trainIdx"], 2]):
                continue  # ErrorFunction2 returns before DepthCovariance (ransac.cpp:362-365)
            sd = 0.01 * float(z1) * float(z1)
            return sd * sd
    return float("nan")


# ------------------------------------------------------------- the stage
def stage_ref(frames, cfg):
    """frames: [(desc, xyz)]; returns (per-pair dicts, latch)."""
    pairs = []
    for p in range(len(frames) - 1):
        (d1, x1), (d2, x2) = frames[p], frames[p + 1]
        flags, ql = vo_landmarks(x1)
        ki, kd = knn_ref.knn2_ref(d1[ql], d2)
        matches, src = ratio_match(ki, kd, ql, cfg["ratio"], len(d2))
        keep = depth_filter(matches, x1, x2, cfg["check_depth"])
        perm, heaps = std_sort([float(matches["distance"][k]) for k in keep])
        pairs.append(dict(flags=flags, qlist=ql, knn_idx=ki, knn_dist=kd, matches=matches,
                          good_keys=matches["distance"][keep], good=matches[keep[perm]] if len(keep) else matches[:0],
                          f2_src=src, heaps=heaps))
    return pairs, latch_ref(pairs, [x for _, x in frames], cfg["min_inl"], cfg["latch"])


# ------------------------------------------------------------------ the code
def _code():
    h = np.array([[1]])
    for _ in range(8):
        h = np.block([[h, h], [h, -h]])
    rows = np.packbits((h < 0).astype(np.uint8), axis=1)
    return np.concatenate([rows, ~rows])


CODE = _code()  # 512 x 32 bytes, pairwise Hamming distance 128 (256 for a row and its complement)
CODE.setflags(write=False)
REJECT = CODE[255]  # 128 from every train of a case (cases use neither row 255 nor its complement as a train)


def flip(w, d, start=0):
    """w with bits start .. start + d - 1 flipped (bit b = byte b >> 3, mask 0x80 >> (b & 7))."""
    w = w.copy()
    for b in range(start, start + d):
        w[b >> 3] ^= np.uint8(0x80 >> (b & 7))
    return w


def near(j, d, start=0):
    """Code word j with d bits flipped."""
    return flip(CODE[j], d, start)


def trains(n, first=0):
    """n distinct code words, none of them REJECT or its complement."""
    ids = [j for j in range(512) if j % 256 != 255][first:first + n]
    assert len(ids) == n
    return CODE[ids].copy(), ids


def _xyz(z, x=None):
    z = np.asarray(z, np.float32)
    out = np.empty((len(z), 3), np.float32)
    out[:, 0] = 0.25 + 0.001 * np.arange(len(z)) if x is None else x
    out[:, 1] = -0.5
    out[:, 2] = z
    return out


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _cfg(**kw):
    c = dict(ratio=0.9, check_depth=1, min_inl=20, latch=float("nan"), max_batch=2)
    c.update(kw)
    return c


WITHIN, BEYOND = 1.5, 4.0  # z on either side of TH_DEPTH (3.09)


# --------------------------------------------------------------- the cases
# A builder returns (frames, cfg, meta); meta names what the case claims.
def _lm_case(z, seed=1, meta=None):
    """Landmark selection: frame 0 with the z given, 8 trains, queries that
    are near copies of a train (so landmarks match and nothing else does)."""
    rng = np.random.default_rng(seed)
    t, ids = trains(8)
    q = np.stack([near(ids[i % 8], i % 5) for i in range(len(z))]) if len(z) else np.zeros((0, 32), np.uint8)
    return [(q, _xyz(z)), (t, _xyz(rng.uniform(0.5, 6.0, 8)))], _cfg(), meta or {}


def _lm_n1(n1):
    rng = np.random.default_rng(100 + n1)
    z = rng.uniform(0.5, 6.0, n1).astype(np.float32)
    z[rng.random(n1) < 0.1] = 0.0
    return _lm_case(z, n1)


def _lm_counts(within, beyond, invalid=5, seed=0):
    rng = np.random.default_rng(1000 * within + 10 * beyond + seed)
    z = np.concatenate([rng.uniform(0.5, 3.0, within), rng.uniform(3.2, 9.0, beyond), np.zeros(invalid)])
    return _lm_case(rng.permutation(z).astype(np.float32), seed, dict(within=within, beyond=beyond))


def _lm_tie(within, beyond_below):
    """Equal z at the K-th and (K+1)-th place of the sorted list: within
    points inside, beyond_below smaller points beyond, then two equal ones
    (the lower index wins) and three larger ones."""
    rng = np.random.default_rng(7 + within)
    z = np.concatenate([rng.uniform(0.5, 3.0, within), rng.uniform(3.2, 4.0, beyond_below), [5.0, 9.0, 5.0, 8.0, 7.0],
                        np.zeros(3)]).astype(np.float32)
    perm = rng.permutation(len(z))
    z = z[perm]
    tie = sorted(int(i) for i in np.nonzero(z == np.float32(5.0))[0])
    return _lm_case(z, 3, dict(tie=tie, place=within + beyond_below))


def _lm_at_th():
    rng = np.random.default_rng(11)
    z = np.concatenate([rng.uniform(0.5, 3.0, 99), np.full(6, TH_DEPTH), rng.uniform(3.2, 9.0, 3), np.zeros(4)])
    return _lm_case(rng.permutation(z).astype(np.float32), 4, dict(at_th=6, within=105))


def _lm_special(within):
    rng = np.random.default_rng(13 + within)
    special = np.array([np.nan, 0.0, -0.0, -1.5, -np.inf, 1e-45, np.inf], np.float32)
    z = np.concatenate([rng.uniform(0.5, 3.0, within).astype(np.float32), special])
    return _lm_case(rng.permutation(z), 5, dict(within=within + 1))


def _ql(count, layout):
    """count landmarks out of 600 keypoints, at the low indices, the high
    ones or alternating; every other keypoint (z = 0) is an exact copy of a
    train, whose match would pass the ratio test."""
    n1 = 600
    sel = {"low": np.arange(count), "high": np.arange(n1 - count, n1), "alt": 2 * np.arange(count)}[layout]
    z = np.zeros(n1, np.float32)
    z[sel] = WITHIN + 0.001 * np.arange(count)
    t, ids = trains(40)
    q = np.stack([near(ids[i % 40], 0 if z[i] == 0 else i % 4) for i in range(n1)])
    return [(q, _xyz(z)), (t, _xyz(np.full(40, 2.0)))], _cfg(), dict(landmarks=count)


def _nt(n2):
    """300 landmark queries against n2 trains; query i is train i % n2 with
    i % 7 bits flipped: the best sits at 0 and at n2 - 1 among others."""
    n1 = 300
    t, ids = trains(n2)
    q = np.stack([near(ids[i % n2], i % 7) if n2 else REJECT for i in range(n1)])
    return [(q, _xyz(np.full(n1, WITHIN))), (t, _xyz(np.full(n2, 2.0)))], _cfg(), {}


def split_bounds(nt, nsplit):
    return [nt * h // nsplit for h in range(nsplit + 1)]


def _split_copies(n2=257):
    """Identical trains at b - 1 and b for every split boundary b of 2, 3 and
    8 splits: the two copies tie, the lower index comes first, and the ratio
    test rejects every query (d0 = d1) unless the merge loses the second."""
    t, ids = trains(n2)
    bs = sorted({b for s in SPLITS for b in split_bounds(n2, s)[1:-1]})
    for b in bs:
        t[b - 1] = t[b]
    q = np.stack([near(ids[b], k) for b in bs for k in (1, 3)])
    n1 = len(q)
    return [(q, _xyz(np.full(n1, WITHIN))), (t, _xyz(np.full(n2, 2.0)))], _cfg(), dict(copies=[(b - 1, b) for b in bs])


def _split_order(n2=257):
    """Best and second best one bit apart at adjacent trains (k, k + 1), in
    both orders: boundary pairs lie in different splits, the interior ones
    in one split. Distances (0, 1) pass the ratio test; (18, 19) fail it, and
    would pass against the third neighbour, 100 or more away."""
    t, ids = trains(n2)
    bs = sorted({b for s in SPLITS for b in split_bounds(n2, s)[1:-1]})
    pos = [(b - 1, b) for b in bs] + [(10, 11), (140, 141), (240, 241), (0, n2 - 1)]
    q = []
    for a, b in pos:
        t[a] = near(ids[b], 1, start=200)  # one bit from t[b]
        q += [t[b].copy(), t[a].copy(), flip(t[b], 18), flip(t[a], 18)]
    q = np.stack(q)
    return [(q, _xyz(np.full(len(q), WITHIN))), (t, _xyz(np.full(n2, 2.0)))], _cfg(), dict(adjacent=pos)


RATIO_PAIRS = [(0, 0), (0, 1), (9, 10), (18, 20), (27, 30), (45, 50), (63, 70), (40, 40), (8, 10), (26, 30), (62, 70)]


def _ratio():
    """Query k is code word k; its two nearest trains are that word with d0
    and with d1 other bits flipped."""
    t, q = [], []
    for k, (d0, d1) in enumerate(RATIO_PAIRS):
        q.append(CODE[k].copy())
        t += [near(k, d0), near(k, d1, start=128)]
    t, q = np.stack(t), np.stack(q)
    return [(q, _xyz(np.full(len(q), WITHIN))), (t, _xyz(np.full(len(t), 2.0)))], _cfg(), dict(dists=RATIO_PAIRS)


def _slots():
    """Several accepting queries per train, on both sides of the 256-query
    scan chunk and at the end; every other query is rejected."""
    n1 = 600
    t, ids = trains(12)
    owners = {0: [3, 255, 256, 599], 1: [100, 254], 2: [257, 20], 5: [511, 512, 513]}
    q = np.repeat(REJECT[None], n1, 0)
    for tr, qs in owners.items():
        for k, i in enumerate(qs):
            q[i] = near(ids[tr], k + 1)
    return ([(q, _xyz(np.full(n1, WITHIN))), (t, _xyz(np.full(12, 2.0)))], _cfg(),
            dict(owners={tr: max(qs) for tr, qs in owners.items()}))


SIZES = [0, 1, 19, 20, 255, 256, 257]
BAD_Z = [np.nan, 0.0, -0.0, -2.0, -np.inf]


def _matches_case(k, removed, check_depth, seed=0, n1=400):
    """k accepting queries with good depth, plus one per BAD_Z train depth
    when removed; the other queries are rejected (128 from every train)."""
    rng = np.random.default_rng(50 + k + seed)
    extra = len(BAD_Z) if removed else 0
    m = k + extra
    n2 = max(m, 2)  # a lone train would accept every query: its second neighbour is absent
    t, ids = trains(n2)
    must = [255, 256, 0, n1 - 1][:m]  # either side of the 256-wide scan chunk, the first and the last query
    rest = rng.choice([i for i in range(n1) if i not in must], m - len(must), replace=False)
    acc = np.sort(np.concatenate([must, rest]).astype(np.int64))
    tr = rng.permutation(m)
    q = np.repeat(REJECT[None], n1, 0)
    for j, i in enumerate(acc):
        q[i] = near(ids[tr[j]], int(rng.integers(0, 40)))
    zt = np.full(n2, 2.0, np.float32)
    if removed:
        zt[rng.choice(n2, extra, replace=False)] = BAD_Z
    return ([(q, _xyz(np.full(n1, WITHIN))), (t, _xyz(zt))], _cfg(check_depth=check_depth),
            dict(n_matches=k + extra, n_good=k + extra if not check_depth else k))


def _sort_case(keys, ratio=100.0):
    """len(keys) good matches whose distances, in match order, are keys
    (<= 63): query i is train i with keys[i] bits flipped."""
    n = len(keys)
    t, ids = trains(n)
    q = np.stack([near(ids[i], int(d)) for i, d in enumerate(keys)])
    return ([(q, _xyz(np.full(n, WITHIN))), (t, _xyz(np.full(n, 2.0)))], _cfg(ratio=ratio),
            dict(keys=[float(d) for d in keys]))


def _latch_case(kind):
    n = 30
    t, ids = trains(n)
    q = np.stack([near(ids[i], i) for i in range(n)])  # distances 0, 1, 2, ...: the sorted order is the index
    z1 = (1.0 + 0.03125 * np.arange(n)).astype(np.float32)
    x2 = np.full(n, 0.5, np.float32)
    zt = np.full(n, 2.0, np.float32)
    cfg = _cfg()
    if kind == "x0":  # the first sorted good match has target x +0, the second -0
        x2[0], x2[1] = 0.0, -0.0
    elif kind == "nocheck":  # kept by the filter despite the train depth; x +-0 still skipped
        cfg = _cfg(check_depth=0)
        zt[:3] = [np.nan, 0.0, -1.0]  # the first: no number, skipped; the third latches
        x2[1] = -0.0
    elif kind == "preset":
        cfg = _cfg(latch=0.125)
    elif kind == "filtered":  # the first sorted matches fall to the depth filter
        zt[:4] = [0.0, np.nan, -1.0, -0.0]
    f0, f1 = (q, _xyz(z1)), (t, _xyz(zt, x2))
    if kind == "second":  # pair 0 has 19 matches, pair 1 latches
        q0 = q[:19].copy()
        q0[:, 31] ^= np.uint8(1)  # one bit from its train, frame 1's keypoint of the same index
        return [(q0, _xyz(np.full(19, 1.25))), f0, f1], cfg, dict(first_pair_matches=19)
    if kind == "none":  # 30 matches, every target x zero
        f1 = (t, _xyz(zt, np.zeros(n, np.float32)))
    return [f0, f1], cfg, {}


def _runs():
    """64 frames of 1025 landmarks on a max_batch = 64 context: 63 pairs x 5
    query blocks x 8 splits = 2520 kNN-2 items. Three distinct frames in
    turn, so neighbouring pairs differ."""
    base = [_rand_desc(np.random.default_rng(900 + k), 1025) for k in range(3)]
    fr = []
    for k in range(3):
        d = base[k].copy()
        for i in range(700):  # two bits from one of the next frame's keypoints 700 .. 1024, which stay as drawn
            d[i] = base[(k + 1) % 3][700 + (i * 7 + k) % 325]
            d[i, i % 32] ^= np.uint8(0x11)
        fr.append((d, _xyz(np.random.default_rng(910 + k).uniform(0.5, 3.0, 1025))))
    return [fr[i % 3] for i in range(64)], _cfg(max_batch=64), {}


def _builders():
    b = {}
    for n1 in (0, 1, 63, 64, 65, 100, 101, 102, 255, 256, 257, 1087, 1088):
        b[f"lm-n1-{n1}"] = functools.partial(_lm_n1, n1)
    for w in (0, 99, 100, 101):
        for y in (0, 1, 2):
            b[f"lm-within-{w}-beyond-{y}"] = functools.partial(_lm_counts, w, y)
    b["lm-all-within-150"] = functools.partial(_lm_counts, 150, 0)
    b["lm-all-within-1088"] = functools.partial(_lm_counts, 1088, 0, 0)
    b["lm-few-valid"] = functools.partial(_lm_counts, 30, 30, 240)
    b["lm-tie-sort-path"] = functools.partial(_lm_tie, 50, 50)   # K = 101: places 101 | 102 tie
    b["lm-tie-min-path"] = functools.partial(_lm_tie, 120, 0)    # K = 121: the nearest beyond ties
    b["lm-z-at-th"] = _lm_at_th
    b["lm-special-sort-path"] = functools.partial(_lm_special, 40)
    b["lm-special-min-path"] = functools.partial(_lm_special, 130)
    for count in (0, 1, 255, 256, 257):
        for layout in ("low", "high", "alt"):
            b[f"ql-{count}-{layout}"] = functools.partial(_ql, count, layout)
    for n2 in (0, 1, 2, 3, 7, 8, 9, 255, 256, 257):
        b[f"nt-{n2}"] = functools.partial(_nt, n2)
    b["split-copies"] = _split_copies
    b["split-order"] = _split_order
    b["ratio"] = _ratio
    b["slots"] = _slots
    for k in SIZES:
        b[f"nm-{k}"] = functools.partial(_matches_case, k, False, 1)
        b[f"ng-{k}"] = functools.partial(_matches_case, k, True, 1)
        b[f"ng-{k}-nocheck"] = functools.partial(_matches_case, k, True, 0)
    rng = np.random.default_rng(5)
    b["sort-16"] = functools.partial(_sort_case, tuple(rng.integers(0, 12, 16)))
    b["sort-17"] = functools.partial(_sort_case, tuple(rng.integers(0, 12, 17)))
    b["sort-two-values-300"] = functools.partial(_sort_case, tuple(np.where(rng.random(300) < 0.5, 5, 9)))
    for n in (40, 48, 64):
        b[f"sort-killer-{n}"] = functools.partial(lambda n: _sort_case(killer(n)), n)
    for kind in ("x0", "nocheck", "preset", "filtered", "second", "none"):
        b[f"latch-{kind}"] = functools.partial(_latch_case, kind)
    b["runs-64"] = _runs
    return b


_BUILDERS = _builders()
CASES = [n for n in _BUILDERS if n != "runs-64"]  # the cases of a max_batch = 2 context
RUNS_CASE = "runs-64"
KILLER_CASES = [n for n in CASES if n.startswith("sort-killer-")]
# odo_debug_sort alone: (name, keys)
SORT_ALONE = [(f"killer-{n}", functools.partial(killer, n)) for n in (40, 100, 257, 777, 8192)] + \
             [(f"killer-{n}-few", functools.partial(killer_few, n, k)) for n, k in ((777, 2), (8192, 8))]


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """dict(frames, cfg, meta, pairs, latch): the features, the context's
    configuration, what the case claims, and the expected outputs. Computed
    once and shared: the arrays are read-only."""
    frames, cfg, meta = _BUILDERS[name]()
    frames = [(np.ascontiguousarray(d, np.uint8).reshape(-1, 32), np.ascontiguousarray(x, np.float32).reshape(-1, 3))
              for d, x in frames]
    assert all(len(d) == len(x) <= KP_CAP for d, x in frames) and 2 <= len(frames) <= cfg["max_batch"] + 1
    if name == RUNS_CASE:  # three distinct pairs in turn: the reference of each once
        first, latch = stage_ref(frames[:4], cfg)
        pairs = [first[p % 3] for p in range(len(frames) - 1)]
    else:
        pairs, latch = stage_ref(frames, cfg)
    for d, x in frames:
        d.setflags(write=False)
        x.setflags(write=False)
    return dict(frames=frames, cfg=cfg, meta=meta, pairs=pairs, latch=latch)
