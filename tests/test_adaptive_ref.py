"""CPU checks of the independent ADAPTIVE model (tests/adaptive_ref.py)
against the oracle, on the crafted cases the GPU edge tests run
(tests/test_adaptive_edges_gpu.py): keypoint coordinates, responses and order,
the threshold every cell used, and the persistent thresholds, all exact.

The conditions the crafted cases exist for are asserted here from the model
alone: every chain branch runs somewhere, every "killer" selection input
exhausts introselect's depth, and the wide one-column grids put survivors
past the 32nd pixel of a candidate thread's run.
"""
import numpy as np
import pytest

import adaptive_ref as R
import oracle_lib as O


def oracle_params(case):
    return case.apply(O.adaptive_params())


def run_model(case):
    p = oracle_params(case)
    m = R.AdaptiveModel(p, case.start)
    return [m.extract_gray(g) for g in case.frames]


_MODEL = {}


def model_of(case):
    if case.name not in _MODEL:
        _MODEL[case.name] = run_model(case)
    return _MODEL[case.name]


def test_dot_image_facts():
    """The facts the crafted inputs rest on."""
    pts = [(40, 40, 7), (48, 40, 255), (40, 48, 1), (56, 56, 2), (72, 40, 50), (73, 40, 50), (88, 40, 50), (89, 40, 51)]
    for inv in (False, True):
        img = R.dots(128, 96, pts, inverted=inv)
        S = R.s_map(img)
        exp = np.zeros_like(S)
        for x, y, v in pts:
            exp[y, x] = v
        assert np.array_equal(S, exp)
        assert np.array_equal(O.gray(R.to_bgr(img)), img)
    xs, ys, resp = R.model_fast(R.s_map(R.dots(128, 96, pts)), 0)
    got = sorted(zip(xs.tolist(), ys.tolist(), resp.tolist()))
    # S = 1 scores 0; the equal pair keeps neither; of (50, 51) only the larger
    assert got == sorted([(40, 40, 6), (48, 40, 254), (56, 56, 1), (89, 40, 50)])


@pytest.mark.parametrize("case", R.cases(), ids=repr)
def test_model_matches_oracle(case):
    ex = O.AdaptiveExtractor(oracle_params(case))
    if case.start is not None:
        ex.thresh[:] = case.start
    res = model_of(case)
    seen = set()
    for f, (g, m) in enumerate(zip(case.frames, res)):
        kps, _, t_ref = ex.extract_gray(g, cap=4096)
        tag = f"{case.name} frame {f}"
        assert np.array_equal(m["t_used"], t_ref), f"{tag}: thresholds used {m['t_used']} vs {t_ref}"
        assert len(kps) == len(m["x"]), f"{tag}: {len(m['x'])} keypoints vs {len(kps)}"
        assert np.array_equal(kps["x"], m["x"].astype(np.float32)), f"{tag}: x"
        assert np.array_equal(kps["y"], m["y"].astype(np.float32)), f"{tag}: y"
        assert np.array_equal(kps["response"], m["response"].astype(np.float32)), f"{tag}: response"
        assert np.array_equal(m["thresh"], ex.thresh), f"{tag}: persistent thresholds"
        for tr in m["trace"]:
            seen |= tr
    assert set(case.expect) <= seen, f"{case.name}: branches {set(case.expect) - seen} did not run"


def test_every_chain_branch_runs():
    seen = set()
    for case in R.cases():
        for m in model_of(case):
            for tr in m["trace"]:
                seen |= tr
    assert seen == set(R.BRANCHES)


@pytest.mark.parametrize("name", ["wide_520", "wide_640"])
def test_wide_runs_have_survivors_past_32(name):
    case = next(c for c in R.cases() if c.name == name)
    m = model_of(case)[0]
    offs = R.run_offsets(m["survivors"], case.w, case.h, oracle_params(case))
    assert max(offs) >= 32
    if name == "wide_640":
        assert len(m["cells"][0]) > 4096  # beyond the LDS selection capacity, one cell


def test_crafted_cases_reach_what_they_name():
    by = {c.name: c for c in R.cases()}
    for n in ("narrow_62", "low_62"):
        m = model_of(by[n])[0]
        assert len(m["x"]) == 0 and sum(len(c) for c in m["cells"]) > 0
    m = model_of(by["thresh_above_255"])
    assert m[0]["thresh"][0] == 325.0 and m[1]["t_used"][0] == 227
    t = np.array([m["t_used"][0] for m in model_of(by["min_thresh_0"])])
    assert {0, 1} <= set(t.tolist())
    # a dot in the overlap of n cells appears n times; with edge 0 the 3 px
    # FAST margins of neighbouring cells leave (120, 120) in no detection region
    for e in (0, 60):
        m = model_of(by[f"overlap_edge{e}"])[0]
        n_mid = int(np.sum((m["x"] == 120) & (m["y"] == 120)))
        n_two = int(np.sum((m["x"] == 112) & (m["y"] == 40)))
        assert (n_mid, n_two) == ((0, 1) if e == 0 else (4, 2))
    for nf in (17, 33):  # the chain moves inside the first chunk and across its boundary
        t = np.array([m["t_used"] for m in model_of(by[f"alternating_{nf}"])])
        assert (np.diff(t[:16], axis=0) != 0).any() and (t[16] != t[15]).any()
    m = model_of(by["grid_8x8_edge0"])[0]
    assert len(m["t_used"]) == 64


@pytest.mark.parametrize("name,keys,nth,must_hit", [pytest.param(*c, id=c[0]) for c in R.killer_cases()])
def test_selection_model_matches_nth_element(name, keys, nth, must_hit):
    n = len(keys)
    info = {}
    got = R.nth_element_packed(keys, nth, info)
    assert bool(info.get("depth_limit")) == must_hit
    ref = keys.copy()
    O.lib().oracle_nth_element_score(O.ptr(ref), n, nth)
    assert np.array_equal(got, ref), "nth_element permutation differs"
    info = {}
    got = R.retain_best_packed(keys, nth, info)
    assert bool(info.get("depth_limit")) == (must_hit and n > nth)
    ref = keys.copy()
    m = O.lib().oracle_retain_best_score(O.ptr(ref), n, nth)
    assert len(got) == m and np.array_equal(got, ref[:m]), "retainBest differs"


@pytest.mark.parametrize("seed", range(8))
def test_retain_best_model_with_ties(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.choice([5, 12, 113, 1017, 3000]))
    score = rng.integers(3, 3 + int(rng.choice([2, 5, 40])), n).astype(np.uint32)
    keys = ((score << 24) | np.arange(n, dtype=np.uint32)).astype(np.uint32)
    for n_points in (0, 1, n // 2, n - 1, n, n + 1):
        got = R.retain_best_packed(keys, n_points)
        ref = keys.copy()
        m = O.lib().oracle_retain_best_score(O.ptr(ref), n, n_points)
        assert len(got) == m and np.array_equal(got, ref[:m]), (n, n_points)
