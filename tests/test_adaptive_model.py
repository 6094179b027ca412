"""CPU checks of the decomposition the GPU ADAPTIVE extractor is built on
(DESIGN.md §4 "ADAPTIVE grid"), against the oracle's literal restatement of
the reference (videogridadaptedfeaturedetector.cpp, videodynamicadapted…,
detectoradjuster.cpp, extractor.cpp:39-77):

* cv::FAST(roi, t, nonmax) == {p in the ROI's detection region : S(p) > t and
  S(p) >= 2 and S(p) > S(q) for every 8-neighbour q inside the region},
  response S(p) - 1,
  where S(p) = max(0, best 9-arc contrast) is threshold-free. So one S map per
  frame gives every threshold's keypoint set and count.
* the per-cell threshold chain (tooFew / tooMany / good) replayed on the
  per-cell count-above-threshold tables reproduces the oracle's thresholds
  frame after frame.
* the single-range parallel Hoare partition model of libstdc++'s introselect
  (what the GPU runs for keepStrongest / retainBest) returns exactly
  std::nth_element's permutation.

The model itself lives in tests/adaptive_ref.py, which also carries the
heap-select fallback these inputs do not reach (tests/test_adaptive_ref.py
reaches it with adversarial inputs).
"""
import numpy as np
import pytest

import oracle_lib as O
from adaptive_ref import cell_geometry, chain_step, introselect_model, model_fast, s_map
from conftest import sequence


def oracle_fast(img, y0, x0, rows, cols, t):
    w = img.shape[1]
    out = np.zeros(1 << 16, O.KP_DTYPE)
    sub = np.ascontiguousarray(img)
    n = O.lib().oracle_fast_roi(O.C.c_void_p(sub.ctypes.data + y0 * w + x0), w, rows, cols, t, O.ptr(out), out.size)
    return out[:n]


@pytest.mark.parametrize("t", [0, 2, 5, 7, 13, 20, 41, 254, 255])
def test_fast_is_thresholded_s_map(t):
    bgr, _, _ = sequence(2)
    img = O.gray(bgr[1])
    S = s_map(img)
    rng = np.random.default_rng(t)
    for _ in range(3):
        rows, cols = int(rng.integers(20, 230)), int(rng.integers(20, 280))
        y0, x0 = int(rng.integers(0, 480 - rows)), int(rng.integers(0, 640 - cols))
        ref = oracle_fast(img, y0, x0, rows, cols, t)
        # S of the full image equals S of the ROI inside the ROI's own detection region
        xs, ys, resp = model_fast(S[y0:y0 + rows, x0:x0 + cols], t)
        assert len(ref) == len(xs), (t, rows, cols)
        assert np.array_equal(ref["x"], xs.astype(np.float32)) and np.array_equal(ref["y"], ys.astype(np.float32))
        assert np.array_equal(ref["response"], resp.astype(np.float32))


def test_threshold_chain_matches_oracle():
    bgr, _, _ = sequence(6)
    ex = O.AdaptiveExtractor()
    p = ex.p
    assert (p.grid_rows, p.grid_cols, p.cell_min, p.cell_max, p.max_total_keypoints) == (3, 3, 67, 113, 1020)
    thresh = np.full(9, p.init_thresh)
    cells = cell_geometry(640, 480, p)
    for f in range(6):
        img = O.gray(bgr[f])
        S = s_map(img)
        _, _, t_ref = ex.extract_gray(img)
        for c, (rs, re, cs, ce) in enumerate(cells):
            xs, ys, resp = model_fast(S[rs:re, cs:ce], 0)
            hist = np.bincount(resp + 1, minlength=257)
            count_above = hist[::-1].cumsum()[::-1]  # count_above[t] = #{S >= t}; need S > t
            above = np.append(count_above[1:], 0)
            thresh[c], t_used = chain_step(thresh[c], above, p)
            assert t_used == t_ref[c], (f, c)
        assert np.array_equal(thresh, ex.thresh), f"frame {f}"


@pytest.mark.parametrize("seed", range(12))
def test_introselect_model_matches_nth_element(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([4, 5, 17, 114, 200, 1017, 3000]))
    levels = int(rng.choice([2, 5, 30, 250]))
    score = rng.integers(3, 3 + levels, n)
    a = ((score.astype(np.uint32) << 24) | np.arange(n, dtype=np.uint32)).astype(np.uint32)
    nth = int(rng.integers(0, n))
    ref = a.copy()
    O.lib().oracle_nth_element_score(O.ptr(ref), n, nth)
    got = introselect_model(a, nth, key=lambda e: 255 - (int(e) >> 24))
    assert np.array_equal(np.array(got, np.uint32), ref)
