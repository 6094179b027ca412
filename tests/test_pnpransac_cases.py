"""The crafted PnPRansac cases (pnpransac_cases.py) are what they are named
for: every property is asserted on the reference side (the builder's labels,
the independent numpy / scipy pieces and the oracle), never on the device.

Also here: subsets_py + fold_py against the oracle's own run for every case
(the winning hypothesis' model from subsets_py's indices is the oracle's model,
so the draw streams agree up to it), count64 against the oracle's mask, and
d = max |oracle rt - float64 minimum| for every ok = 1 case (printed; the GPU
file's bound is built from it).
"""
import math

import numpy as np
import pytest

import oracle_lib as O
import pnpransac_cases as PC

CASES = PC.single_cases()
NAMES = list(CASES)


def _non_adjacent(redraws, visited):
    return [x for x in redraws if x[2] < x[1] - 1 and x[0] < visited]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_is_named_for(name):
    c = CASES[name]
    r = PC.reference(c)
    p, n, kind = c.prop, len(c.Xw), c.prop["kind"]
    lab = p.get("labels")
    if "ok" in p:
        assert r["ok"] == p["ok"]
    if "visited" in p:
        assert r["niters"] == p["visited"]
    if "n_inliers" in p:
        assert r["n_inliers"] == p["n_inliers"]
        if lab is not None:
            np.testing.assert_array_equal(r["mask"], lab)  # no outlier fits by chance
    if kind == "points":
        assert lab[-1] and abs((~lab).sum() - 0.3 * n) <= 0.5
        for lo, hi in p["spans"]:
            assert lab[lo:hi].any() and r["mask"][lo:hi].any()
        assert r["ok"] != 0 and r["mask"][-1]  # the tail index counts on the reference too
    if kind == "inliers":
        assert r["ok"] == 1 and n == p["n_inliers"] + 8
    if kind == "fold":
        assert r["ok"] == 1
        mg = r["good"].max()
        assert mg == p["n_inliers"] and r["best_iter"] == int(np.argmax(r["good"] == mg))
        if p["ties"]:
            assert (r["good"] == mg).sum() >= 2  # the first of equal counts wins
        if "quotient" in p:
            q = p["quotient"]
            assert r["niters"] == (math.ceil(q) if name.endswith("up") else math.floor(q))
    if kind == "iterations":
        assert c.iterations in PC.ITERATION_WIDTHS and n == 700 and r["ok"] == 1
        if c.iterations == 0:  # MAX(maxIters, 1): the same run as one iteration, its count recorded too
            one = PC.reference(CASES["iterations_1"])
            for k in ("ok", "niters", "best_iter", "n_inliers"):
                assert r[k] == one[k]
            assert np.array_equal(r["good"], one["good"]) and np.array_equal(r["rt"], one["rt"])
    if kind == "small":
        assert c.iterations == 4096
        _, redraws = PC.subsets_py(n, r["niters"])
        assert _non_adjacent(redraws, r["niters"])
    if kind == "planar":
        ratio = PC.scatter_ratio64(c.Xw[r["mask"]])
        assert (ratio < 1e-3) == (p["side"] == "planar") and abs(ratio / 1e-3 - 1) < 0.01
    if kind == "degenerate" and "max_good" in p:
        assert r["good"].max() <= p["max_good"] and r["best_iter"] == p["best_iter"]
    if kind == "reproj":
        if p["which"] == "negative":
            pos = O.pnp_ransac(c.Xw, c.uv, O.fr1_calib(), c.iterations, -c.reproj, c.conf)
            assert r["ok"] == 1 and np.array_equal(r["mask"], pos["mask"]) and np.array_equal(r["rt"], pos["rt"])
        else:
            assert r["ok"] == 0 and r["niters"] == 500 and not r["good"].any()
    if kind == "nonfinite":
        idx, _ = PC.subsets_py(n, r["niters"])
        hit = [h for h in range(r["niters"]) if p["bad"] in idx[h]]
        assert 0 in hit and not r["good"][hit].any()  # a hypothesis drawn on it counts nothing
        assert r["ok"] == 1 and not r["mask"][p["bad"]] and np.isfinite(r["rt"]).all()


def test_planar_pairs_are_within_one_percent():
    for g in (5, 40):
        a, b = CASES[f"planar{g}_planar"].prop["thickness"], CASES[f"planar{g}_dlt"].prop["thickness"]
        assert 0 < a < b < 1.01 * a
    assert PC.reference(CASES["planar5_planar"])["ok"] == 1 and PC.reference(CASES["planar5_dlt"])["ok"] == -1
    assert PC.reference(CASES["planar40_planar"])["ok"] == 1 and PC.reference(CASES["planar40_dlt"])["ok"] == 1


def test_fold_cases_cover_the_stops_and_both_roundings():
    assert sorted(PC.FOLD_STOPS) == [1, 2, 63, 64, 65, 127, 128, 129]
    for w, (n, g, _) in PC.FOLD_ROUND.items():
        q = PC.update_quotient(0.85, (n - g) / n)
        assert (q - math.floor(q) >= 0.5) == (w == "up")
        assert PC._update_py(0.85, (n - g) / n, 5, 500) == math.floor(q) + (w == "up")


@pytest.mark.parametrize("name", NAMES)
def test_subsets_and_fold_reproduce_the_oracle(name):
    c = CASES[name]
    r = PC.reference(c)
    n = len(c.Xw)
    best, visited, max_good = PC.fold_py(r["good"], n, c.iterations, c.conf)
    assert (best, visited) == (r["best_iter"], r["niters"])
    if r["ok"] == 0:
        return
    assert max_good == r["n_inliers"]
    # the winner's minimal set, drawn independently, gives the oracle's model
    idx, _ = PC.subsets_py(n, best + 1)
    cal = O.fr1_calib()
    K = np.array([cal.fx, cal.fy, cal.cx, cal.cy], np.float64)
    pw = np.ascontiguousarray(c.Xw[idx[best]], np.float64)
    us = np.ascontiguousarray(c.uv[idx[best]], np.float64)
    model = np.zeros(6)
    O.lib().oracle_epnp(O.ptr(pw), O.ptr(us), 5, O.ptr(K), O.ptr(model))
    np.testing.assert_array_equal(model, r["model"])


@pytest.mark.parametrize("name", NAMES)
def test_count64_agrees_off_the_edge(name):
    c = CASES[name]
    r = PC.reference(c)
    if r["ok"] == 0 or c.prop["kind"] == "reproj":
        return
    mask, edge = PC.count64(r["model"], c.Xw, c.uv, c.reproj ** 2)
    assert edge.sum() <= 0.01 * len(c.Xw)
    np.testing.assert_array_equal(mask[~edge], r["mask"][~edge])


def test_oracle_distance_from_the_float64_minimum():
    """d per ok = 1 case, printed (pytest -s). The refinement stops on a
    relative step below FLT_EPSILON, so d far below that says the oracle's
    DLT / homography start and CvLevMarq land on the minimum."""
    ds = {}
    for name, c in CASES.items():
        r = PC.reference(c)
        if r["ok"] == 1:
            ds[name] = r["d"]
            print(f"{name:24s} d = {r['d']:.3e}  bound = {PC.bound64(r):.3e}")
    assert len(ds) >= 40
    print(f"d range: {min(ds.values()):.3e} .. {max(ds.values()):.3e}")
    assert max(ds.values()) < PC.FLT_EPSILON  # below the LM's own stop rule on every case
