"""The Fuse reference against itself (tests/fuse_ref.py), the host-only
odo_fuse_best against it, and the conditions the crafted FuseLandmarks
scenario has to meet so that the device test cannot pass vacuously. No GPU."""
import numpy as np
import pytest

import fuse_ref as F
from conftest import load_pkg

EDGE = F.edge_cases()
SHAPE = F.shape_cases()
UNIT, FR1 = F.camera(F.CAM_UNIT), F.camera(F.CAM_FR1)


@pytest.mark.parametrize("name", sorted(EDGE))
def test_numpy_search_equals_transcription_on_edges(name):
    calls, lms, idx, th = EDGE[name]
    assert F.records_equal(F.search_calls(calls, lms, idx, th, UNIT), F.search_calls(calls, lms, idx, th, UNIT,
                                                                                     one=F.search_py)) is None


@pytest.mark.parametrize("name", sorted(SHAPE))
def test_numpy_search_equals_transcription_on_shapes(name):
    calls, lms, idx, th = SHAPE[name]
    a = F.search_calls(calls, lms, idx, th, FR1)
    assert F.records_equal(a, F.search_calls(calls, lms, idx, th, FR1, one=F.search_py)) is None
    if name.startswith(("kp_6", "kp_2", "list_2", "calls")):
        assert (a["n_cand"] > 1).any() and (a["n_cand"] == 0).any(), "the case exercises nothing"


def test_edge_cases_sit_on_their_edges():
    """What each edge case is built to show, stated on the reference's output."""
    rec = {k: F.search_calls(*v, UNIT) for k, v in EDGE.items()}
    r = rec["depth"]
    assert list(r["n_cand"]) == [F.BEHIND, F.OUTSIDE, F.OUTSIDE, F.OUTSIDE, 1, F.OUTSIDE, F.OUTSIDE, F.OUTSIDE, F.BEHIND]
    assert r["u"][4] == 0 and r["ur"][4] < -1e37 and np.isnan(r["u"][0])
    assert list(rec["bounds"]["n_cand"]) == [1, F.OUTSIDE, F.OUTSIDE, 1, F.OUTSIDE, F.OUTSIDE, F.OUTSIDE]
    # keypoint 4 sits inside both windows' corners; only th = 0.5's corner is inside the gate
    assert rec["window_2.0"][0]["n_cand"] == 2 and list(rec["window_2.0"][0]["cand"][:3]) == [1, 3, 0xFFFF]
    assert rec["window_0.5"][0]["n_cand"] == 3 and list(rec["window_0.5"][0]["cand"][:3]) == [1, 3, 4]
    assert rec["gate"][0]["n_cand"] == 4 and list(rec["gate"][0]["cand"][:4]) == [0, 2, 3, 5]
    assert rec["right"][0]["n_cand"] == 3 and list(rec["right"][0]["cand"][:3]) == [1, 2, 5]
    assert list(rec["dist"]["best_dist"]) == [0, 256] and list(rec["dist"]["best_idx"]) == [0, 1]
    assert list(rec["ties"]["best_idx"]) == [0, 2] and list(rec["ties"]["n_cand"]) == [2, 3]
    assert list(rec["counts"]["n_cand"]) == [8, 9, 40]
    assert all(np.all(np.diff(r["cand"].astype(int)) > 0) for r in rec["counts"])
    assert list(rec["grid"]["n_cand"]) == [3, 1, 2, 3, 0]
    assert list(rec["entries"]["n_cand"]) == [1, F.NULL, F.BAD_LM, F.NULL, 1, F.NULL, F.NULL, 1]


def test_fuse_best_equals_transcription():
    """odo_fuse_best over the candidate list (n_cand <= 8) and over the rescan
    (n_cand > 8), under descriptors the records were not made with."""
    pkg = load_pkg()
    rng = np.random.default_rng(77)
    seen = {"list": 0, "rescan": 0, "none": 0}
    for cases, cam in ((EDGE, UNIT), (SHAPE, FR1)):
        for name in ("counts", "gate", "ties", "depth", "kp_2049", "list_257", "th_0.5"):
            if name not in cases:
                continue
            calls, lms, idx, th = cases[name]
            rec = F.search_calls(calls, lms, idx, th, cam)
            T, kun, kur, kdesc = calls[0][:4]
            for i in range(min(len(rec), 60)):
                r = rec[i]
                for nd in (F.rand_desc(rng, 1)[0], kdesc[int(rng.integers(len(kdesc)))] if len(kdesc) else lms["desc"][0]):
                    got = pkg.fuse_best(r, kun, kur, kdesc, nd, th)
                    if r["n_cand"] < 0:
                        assert got == (-1, F.INT32_MAX)
                        seen["none"] += 1
                        continue
                    ref = F.search_pair_py(np.asarray(T).reshape(4, 4), kun, kur, kdesc, lms["X"][idx[i]], nd, F.f32(th), cam)
                    assert got == (ref[5], ref[6]), (name, i)
                    seen["rescan" if r["n_cand"] > F.CANDS else "list"] += 1
    assert min(seen.values()) > 0, seen
    lib = pkg.load()
    r = F.empty_records(1)
    r["n_cand"], r["cand"][0, 0] = 1, 5
    out = np.zeros(2, np.int32)
    args = (pkg.ptr(r), pkg.ptr(np.zeros((2, 2), np.float32)), pkg.ptr(np.zeros(2, np.float32)),
            pkg.ptr(np.zeros((2, 32), np.uint8)), 2)
    tail = (pkg.ptr(np.zeros(32, np.uint8)), pkg.ptr(out[:1]), pkg.ptr(out[1:]))
    assert lib.odo_fuse_best(*args, 4.0, *tail) == pkg._abi.ERR_ARG  # candidate 5 of 2 keypoints
    assert lib.odo_fuse_best(*args, -1.0, *tail) == pkg._abi.ERR_ARG
    assert lib.odo_fuse_best(*args, float("nan"), *tail) == pkg._abi.ERR_ARG
    assert lib.odo_fuse_best(None, *args[1:], 4.0, *tail) == pkg._abi.ERR_ARG


def test_scenario_meets_its_conditions():
    """On the reference alone: every branch of Fuse, a landmark whose changed
    descriptor moves its best match, and one with more than 8 candidates."""
    _, _, stats, rs = F.scenario_reference()
    assert stats["add"] > 0 and stats["replace_lm"] > 0 and stats["replace_in_kf"] > 0, stats
    assert rs.changed_best > 0, "no landmark whose later bestIdx differs under its old descriptor"
    assert rs.changed_over > 0, "no changed landmark with more than 8 candidates"


def test_scenario_replay_from_records():
    """The device's contract on the reference search: records made before each
    loop plus odo_fuse_best reproduce the reference; the stale best does not."""
    pkg = load_pkg()
    _, want, stats, _ = F.scenario_reference()
    cam = F.scenario_reference()[0][4]
    records = lambda calls, lms, idx, th: F.search_calls(calls, lms, idx, th, cam)  # noqa: E731
    got, gstats, s = F.run_scenario(records, pkg.fuse_best)
    assert got == want and gstats == stats
    assert s.rescored > 0
    stale, _, _ = F.run_scenario(records, None)
    assert stale != want, "a replay that keeps the stale best must fail on this scenario"
