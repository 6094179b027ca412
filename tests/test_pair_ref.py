"""CPU checks of tests/pair_ref.py: every piece of the pair-stage reference
against the oracle (oracle_vo_landmarks, oracle_knn_match, oracle_sort_dmatch,
the real std::sort; whole cases against oracle_track_pair where it runs
RANSAC), and every case for what it is named after."""
import numpy as np
import pytest

import oracle_lib as O
import pair_ref as R

ALL_CASES = R.CASES + [R.RUNS_CASE]


def oracle_landmarks(xyz):
    flags = np.zeros(max(len(xyz), 1), np.uint8)
    n = O.lib().oracle_vo_landmarks(O.ptr(np.ascontiguousarray(xyz)), len(xyz), float(R.TH_DEPTH), O.ptr(flags))
    return flags[:len(xyz)], n


def oracle_std_sort(keys):
    m = np.zeros(len(keys), O.DMATCH_DTYPE)
    m["queryIdx"] = np.arange(len(keys))
    m["distance"] = keys
    O.lib().oracle_sort_dmatch(O.ptr(m), len(keys))
    return list(m["queryIdx"])


def distinct_pairs(case):
    """The pairs of a case that differ (the runs case repeats three)."""
    return range(3 if case == R.RUNS_CASE else len(R.pair_case(case)["pairs"]))


@pytest.mark.parametrize("case", ALL_CASES)
def test_landmarks_match_the_oracle(case):
    c = R.pair_case(case)
    for p in distinct_pairs(case):
        flags, n = oracle_landmarks(c["frames"][p][1])
        assert np.array_equal(c["pairs"][p]["flags"], flags)
        assert len(c["pairs"][p]["qlist"]) == n


@pytest.mark.parametrize("seed", range(6))
def test_landmarks_match_the_oracle_on_random_depths(seed):
    rng = np.random.default_rng(seed)
    for _ in range(20):
        n = int(rng.integers(0, 400))
        z = rng.choice([0.0, 1.0, 2.5, float(R.TH_DEPTH), 3.5, 3.5, 7.0, np.nan, -1.0, np.inf], n).astype(np.float32)
        z += (rng.random(n) < 0.5) * rng.integers(0, 3, n).astype(np.float32) * np.float32(0.25)
        xyz = np.zeros((n, 3), np.float32)
        xyz[:, 2] = z
        flags, cnt = oracle_landmarks(xyz)
        got, ql = R.vo_landmarks(xyz)
        assert np.array_equal(got, flags) and len(ql) == cnt


@pytest.mark.parametrize("case", ALL_CASES)
def test_matches_and_slots_match_the_oracle(case):
    """Matcher::KnnMatch on the reference's landmark flags: the match list in
    order and the owner of every train slot."""
    c = R.pair_case(case)
    for p in distinct_pairs(case):
        (d1, _), (d2, _) = c["frames"][p], c["frames"][p + 1]
        r = c["pairs"][p]
        n1, n2 = len(d1), len(d2)
        zeros8, zeros32 = np.zeros(max(n1, 1), np.uint8), np.zeros(max(n1, 1), np.int32)
        obs2, src2 = np.full(max(n2, 1), -1, np.int32), np.full(max(n2, 1), -1, np.int32)
        out2 = np.zeros(max(n2, 1), np.uint8)
        m = np.zeros(max(n1, 1), O.DMATCH_DTYPE)
        flags = np.ascontiguousarray(np.concatenate([r["flags"], np.zeros(1, np.uint8)]))
        nm = O.lib().oracle_knn_match(O.ptr(np.ascontiguousarray(d1)), n1, O.ptr(np.ascontiguousarray(d2)), n2,
                                      c["cfg"]["ratio"], O.ptr(flags), O.ptr(zeros8), O.ptr(zeros32), O.ptr(obs2),
                                      O.ptr(src2), O.ptr(out2), O.ptr(m), max(n1, 1))
        assert nm == len(r["matches"])
        assert np.array_equal(m[:nm], r["matches"].astype(O.DMATCH_DTYPE))
        assert np.array_equal(src2[:n2], r["f2_src"])
        ki, kd = O.knn2(d1, d2) if n1 else (np.zeros((0, 2), np.int32),) * 2
        assert np.array_equal(ki[r["qlist"]], r["knn_idx"]) and np.array_equal(kd[r["qlist"]], r["knn_dist"])


@pytest.mark.parametrize("case", ALL_CASES)
def test_good_matches_are_std_sorted(case):
    c = R.pair_case(case)
    for p in distinct_pairs(case):
        r = c["pairs"][p]
        keys = [float(k) for k in r["good_keys"]]
        perm = oracle_std_sort(keys)
        ref = R.std_sort(keys)[0]
        assert perm == ref
        assert [float(k) for k in r["good"]["distance"]] == [keys[i] for i in perm]


SORT_INPUTS = [(name, fn) for name, fn in R.SORT_ALONE] + \
              [(f"killer-{n}", lambda n=n: R.killer(n)) for n in (33, 48, 61, 64)]


@pytest.mark.parametrize("name,keys", SORT_INPUTS, ids=[n for n, _ in SORT_INPUTS])
def test_std_sort_is_std_sort_on_killer_inputs(name, keys):
    keys = [float(k) for k in keys()]
    perm, heaps = R.std_sort(keys)
    assert perm == oracle_std_sort(keys)
    if name != "killer-33":
        print(f"{name}: heap branch on ranges of {heaps}")
        assert heaps and all(h > 16 for h in heaps), "the input does not reach the depth limit"
    else:
        assert not heaps  # 2 floor(log2 33) = 10 levels are enough for 33 elements


@pytest.mark.parametrize("seed", range(8))
def test_std_sort_is_std_sort_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    for _ in range(6):
        n = int(rng.integers(0, 700))
        keys = rng.integers(0, int(rng.integers(1, 80)), n).astype(np.float32)
        if seed % 2:
            keys[:n // 2] = np.sort(keys[:n // 2])[::-1]
        assert R.std_sort(keys.tolist())[0] == oracle_std_sort(keys)


@pytest.mark.parametrize("case", R.KILLER_CASES)
def test_killer_cases_take_the_heap_branch(case):
    c = R.pair_case(case)
    r = c["pairs"][0]
    assert [float(k) for k in r["good_keys"]] == c["meta"]["keys"], "the good list is not the killer input"
    assert max(c["meta"]["keys"]) <= 63
    print(f"{case}: heap branch on ranges of {r['heaps']}")
    assert r["heaps"], "the case does not reach the depth limit in the reference"


@pytest.mark.parametrize("case", [n for n in ALL_CASES if len(R.pair_case(n)["pairs"][0]["matches"]) >= 20
                                  or len(R.pair_case(n)["frames"]) > 2])
def test_whole_cases_match_the_oracle_track(case):
    """oracle_track_pair (UpdateLastFrame, KnnMatch, Ransac::Iterate) pair by
    pair, the latch carried along: the match list and the latch."""
    c = R.pair_case(case)
    cfg = c["cfg"]
    cal = O.fr1_calib()
    rp = O.ransac_params(iters=3, min_inl=cfg["min_inl"], check_depth=cfg["check_depth"])
    latch = cfg["latch"]
    ran = False
    for p in distinct_pairs(case):
        fr = []
        for d, x in c["frames"][p:p + 2]:
            n = len(d)
            fr.append(dict(kps=np.zeros(max(n, 1), O.KP_DTYPE)[:n], desc=np.ascontiguousarray(d),
                           kun=np.zeros((n, 2), np.float32), xyz=np.ascontiguousarray(x), ur=np.full(n, -1, np.float32)))
        _, _, m, latch = O.track_pair(fr[0], fr[1], cal, rp, 1234 + p, latch=latch, ratio=cfg["ratio"])
        assert np.array_equal(m, c["pairs"][p]["matches"].astype(O.DMATCH_DTYPE))
        ran = ran or len(m) >= 20
        if case == R.RUNS_CASE:
            break  # the latch is the first pair's
    assert ran
    O.assert_same_bits(latch, c["latch"], f"{case}: latch", np.float64)


# ------------------------------------------------ what the cases are named after
def test_counts_of_the_selection_cases():
    for w in (0, 99, 100, 101):
        for y in (0, 1, 2):
            c = R.pair_case(f"lm-within-{w}-beyond-{y}")
            z = c["frames"][0][1][:, 2]
            assert ((z > 0) & (z <= R.TH_DEPTH)).sum() == w and (z > R.TH_DEPTH).sum() == y
            assert len(c["pairs"][0]["qlist"]) == min(w + y, max(w + 1, 101))
    for name, n in (("lm-all-within-150", 150), ("lm-all-within-1088", 1088)):
        z = R.pair_case(name)["frames"][0][1][:, 2]
        assert ((z > 0) & (z <= R.TH_DEPTH)).sum() == n and not (z > R.TH_DEPTH).any()
        assert len(R.pair_case(name)["pairs"][0]["qlist"]) == n
    c = R.pair_case("lm-few-valid")
    assert (c["frames"][0][1][:, 2] > 0).sum() == 60 == len(c["pairs"][0]["qlist"])
    for n1 in (0, 1, 63, 64, 65, 100, 101, 102, 255, 256, 257, 1087, 1088):
        assert len(R.pair_case(f"lm-n1-{n1}")["frames"][0][0]) == n1
    c = R.pair_case("lm-z-at-th")
    z = c["frames"][0][1][:, 2]
    assert (z == R.TH_DEPTH).sum() == 6 and (z < R.TH_DEPTH).sum() - (z <= 0).sum() == 99
    assert c["pairs"][0]["flags"][z == R.TH_DEPTH].all() and len(c["pairs"][0]["qlist"]) == 106


@pytest.mark.parametrize("case,k,path", [("lm-tie-sort-path", 101, "sort"), ("lm-tie-min-path", 121, "min")])
def test_tie_cases_tie_at_the_kth_place(case, k, path):
    c = R.pair_case(case)
    z = c["frames"][0][1][:, 2]
    order = sorted((float(v), i) for i, v in enumerate(z) if v > 0)
    assert order[k - 1][0] == order[k][0], "no equal z at the K-th / (K+1)-th place"
    lo, hi = c["meta"]["tie"]
    assert (order[k - 1][1], order[k][1]) == (lo, hi)
    f = c["pairs"][0]["flags"]
    assert f[lo] == 1 and f[hi] == 0 and f.sum() == k
    within = int(((z > 0) & (z <= R.TH_DEPTH)).sum())
    assert (within >= 100) == (path == "min")


@pytest.mark.parametrize("case", ["lm-special-sort-path", "lm-special-min-path"])
def test_special_depths(case):
    c = R.pair_case(case)
    z, f = c["frames"][0][1][:, 2], c["pairs"][0]["flags"]
    bits = z.view(np.uint32)
    assert f[bits == 1].all(), "the smallest subnormal is a valid depth"
    assert f[np.isposinf(z)].all(), "+inf is valid: the only point beyond / among the first 101"
    assert not f[np.isnan(z) | (z <= 0)].any()
    assert np.isnan(z).any() and (bits == 0x80000000).any() and np.isneginf(z).any()


def test_query_list_cases():
    for count in (0, 1, 255, 256, 257):
        for layout in ("low", "high", "alt"):
            c = R.pair_case(f"ql-{count}-{layout}")
            r = c["pairs"][0]
            assert len(r["qlist"]) == count and len(c["frames"][0][0]) == 600
            # every keypoint that is no landmark would match: an exact copy of a train, the next train 128 away
            ki, kd = R.knn_ref.knn2_ref(c["frames"][0][0], c["frames"][1][0])
            rest = r["flags"] == 0
            assert (kd[rest, 0] == 0).all() and (kd[rest, 1] == 128).all()
            assert set(r["matches"]["queryIdx"]) <= set(r["qlist"].tolist())
            assert len(r["matches"]) == count


@pytest.mark.parametrize("case", ["split-copies", "split-order"])
def test_split_cases_straddle_every_boundary(case):
    c = R.pair_case(case)
    nt = len(c["frames"][1][0])
    r = c["pairs"][0]
    top = {(int(a), int(b)) for a, b in r["knn_idx"]}
    pairs = c["meta"]["copies"] if case == "split-copies" else c["meta"]["adjacent"]
    for s in (2, 3, 8):
        for b in R.split_bounds(nt, s)[1:-1]:
            assert (b - 1, b) in pairs, f"no planted pair across the boundary {b} of {s} splits"
    if case == "split-copies":
        t = c["frames"][1][0]
        for a, b in pairs:
            assert np.array_equal(t[a], t[b]) and (a, b) in top
        assert (r["knn_dist"][:, 0] == r["knn_dist"][:, 1]).all() and len(r["matches"]) == 0
    else:
        for a, b in pairs:
            assert (a, b) in top and (b, a) in top, "both orders of best / second best"
        for s in (2, 3, 8):
            bounds = R.split_bounds(nt, s)
            same = [np.searchsorted(bounds, a, "right") == np.searchsorted(bounds, b, "right") for a, b in pairs]
            assert any(same) and not all(same)
        assert (0, nt - 1) in top and (nt - 1, 0) in top, "the best at index 0 and at n2 - 1"
        # half the queries pass the ratio test; the others fail it by the second neighbour alone
        d = r["knn_dist"].tolist()
        assert d.count([0, 1]) == d.count([18, 19]) == 2 * len(pairs) == len(d) // 2
        assert len(r["matches"]) == 2 * len(pairs)
        q, t = c["frames"][0][0], c["frames"][1][0]
        third = np.sort(np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2), axis=1)[:, 2]
        assert (18 < np.float32(0.9) * third.astype(np.float32)).all()


def test_train_count_cases():
    for n2 in (0, 1, 2, 3, 7, 8, 9, 255, 256, 257):
        c = R.pair_case(f"nt-{n2}")
        r = c["pairs"][0]
        assert len(c["frames"][1][0]) == n2
        if n2:
            assert {0, n2 - 1} <= set(r["knn_idx"][:, 0].tolist()), "the best at index 0 and at n2 - 1"
        if n2 < 2:
            assert (r["knn_idx"][:, 1] == -1).all() and (r["knn_dist"][:, 1] == R.INT32_MAX).all()
        assert len(r["matches"]) == (300 if n2 else 0)


def test_ratio_case_has_the_distances_it_names():
    c = R.pair_case("ratio")
    r = c["pairs"][0]
    assert [tuple(d) for d in r["knn_dist"].tolist()] == [tuple(p) for p in R.RATIO_PAIRS]
    accepted = set(r["matches"]["queryIdx"].tolist())
    f32 = {k for k, (d0, d1) in enumerate(R.RATIO_PAIRS) if np.float32(d0) < np.float32(0.9) * np.float32(d1)}
    assert accepted == f32 == {1, 8, 9, 10}


def test_slot_case_has_several_queries_per_train():
    c = R.pair_case("slots")
    r = c["pairs"][0]
    for tr, owner in c["meta"]["owners"].items():
        qs = r["matches"]["queryIdx"][r["matches"]["trainIdx"] == tr]
        assert len(qs) >= 2 and r["f2_src"][tr] == owner == qs.max()
    assert {255, 256, 599} <= set(r["matches"]["queryIdx"].tolist())


def test_size_cases_have_the_sizes_they_name():
    for k in R.SIZES:
        for name in (f"nm-{k}", f"ng-{k}", f"ng-{k}-nocheck"):
            c = R.pair_case(name)
            r = c["pairs"][0]
            assert (len(r["matches"]), len(r["good"])) == (c["meta"]["n_matches"], c["meta"]["n_good"]), name
        assert len(R.pair_case(f"nm-{k}")["pairs"][0]["matches"]) == k
        c = R.pair_case(f"ng-{k}")
        r = c["pairs"][0]
        assert len(r["good"]) == k
        gone = np.setdiff1d(r["matches"]["trainIdx"], r["good"]["trainIdx"])
        zt = c["frames"][1][1][gone, 2]
        assert len(zt) == 5 and np.isnan(zt).sum() == 1 and (zt == 0).sum() == 2 and (zt < 0).sum() == 2
        # a query is a landmark, so its depth is a positive number: the filter's query side cannot fire
        assert (c["frames"][0][1][r["matches"]["queryIdx"], 2] > 0).all()


def test_sort_cases():
    assert len(R.pair_case("sort-16")["pairs"][0]["good"]) == 16
    assert len(R.pair_case("sort-17")["pairs"][0]["good"]) == 17
    r = R.pair_case("sort-two-values-300")["pairs"][0]
    assert len(r["good"]) == 300 and sorted(set(r["good_keys"].tolist())) == [5.0, 9.0]


def test_latch_cases():
    def lat(z):
        sd = 0.01 * float(z) * float(z)
        return sd * sd

    def first_good(name, p=0):
        c = R.pair_case(name)
        return c, c["pairs"][p]["good"]

    c, g = first_good("latch-x0")
    x2 = c["frames"][1][1][g["trainIdx"][:3], 0]
    assert x2[0] == 0 and not np.signbit(x2[0]) and x2[1] == 0 and np.signbit(x2[1]) and x2[2] != 0
    assert c["latch"] == lat(c["frames"][0][1][g["queryIdx"][2], 2])
    c, g = first_good("latch-nocheck")
    assert c["cfg"]["check_depth"] == 0 and len(g) == 30
    assert np.isnan(c["frames"][1][1][g["trainIdx"][0], 2]) and c["frames"][1][1][g["trainIdx"][0], 0] != 0
    assert c["latch"] == lat(c["frames"][0][1][g["queryIdx"][2], 2])
    c, g = first_good("latch-filtered")
    assert len(g) == 26 and c["latch"] == lat(c["frames"][0][1][4, 2])
    c = R.pair_case("latch-second")
    assert [len(r["matches"]) for r in c["pairs"]] == [19, 30] and c["latch"] == lat(1.0)
    assert R.pair_case("latch-preset")["latch"] == 0.125
    assert np.isnan(R.pair_case("latch-none")["latch"]) and np.isnan(R.pair_case("ng-19")["latch"])
    assert np.isnan(R.pair_case("nm-19")["latch"]) and not np.isnan(R.pair_case("nm-20")["latch"])


def test_runs_case_has_more_items_than_a_round_of_workgroups():
    c = R.pair_case(R.RUNS_CASE)
    items = sum(-(-len(r["qlist"]) // 256) * 8 for r in c["pairs"])
    assert len(c["pairs"]) == 63 and items == 2520 > 8 * 256
    assert all(len(r["matches"]) > 256 for r in c["pairs"][:3])
