"""GPU parity of the two ADAPTIVE extractors off their default parameters and
on crafted S maps (tests/adaptive_ref.py): every frame bit-exact against the
oracle as in test_adaptive_gpu.py (keypoints, descriptors, undistorted
points, xyz, uR), the threshold every cell used on every frame and the
persistent thresholds. No tolerances.

tests/test_adaptive_ref.py holds the CPU half: the independent model equals
the oracle on the same cases, and the conditions the cases exist for (chain
branches, depth-limit fallback, runs past 32 px) hold by the model alone.
"""
import numpy as np
import pytest

import adaptive_ref as R
import oracle_lib as O
from conftest import load_pkg, sequence
from test_adaptive_gpu import assert_frame, cal_of

pytestmark = pytest.mark.gpu

DEPTH = 7500  # any constant valid plane (1.5 m): the geometry stage is covered elsewhere


def config(pkg, w, h, n, params, inner="fast", nlevels=8):
    det = pkg.DETECTOR_ADAPTIVE_ORB if inner == "orb" else pkg.DETECTOR_ADAPTIVE_FAST
    cfg = pkg.default_config(w, h, n, nfeatures=1000, iterations=64, seed=0x5EED0016, detector=det)
    cfg.orb.nlevels = nlevels
    for k, v in params.items():
        setattr(cfg.adaptive, k, v)
    return cfg


def oracle_params(params):
    p = O.adaptive_params()
    for k, v in params.items():
        setattr(p, k, v)
    return p


def check_batch(pkg, params, bgr, dep, start=None, inner="fast", nlevels=8, tag="", nonempty=False):
    """One batch of len(bgr) frames through the GPU and the oracle."""
    n, h, w = bgr.shape[:3]
    cfg = config(pkg, w, h, n, params, inner, nlevels)
    odo = pkg.Odometry(cfg)
    try:
        cal = cal_of(cfg)
        ex = O.AdaptiveExtractor(oracle_params(params), inner=inner)
        if start is not None:
            ex.thresh[:] = start
            odo.set_adaptive_thresholds(np.asarray(start, np.float64))
        frames, t_ref = [], []
        for i in range(n):
            before = ex.thresh.copy()
            _, _, t = ex.extract_gray(O.gray(bgr[i]), cap=1100)
            ex.thresh[:] = before
            frames.append(ex.extract_frame(bgr[i], dep[i], cal))
            t_ref.append(t)
        odo.track_batch_host(bgr, dep)
        for i in range(n):
            t_used, _ = odo.adaptive_state(i)
            assert np.array_equal(t_used, t_ref[i]), f"{tag} frame {i}: cell thresholds {t_used} vs {t_ref[i]}"
            assert_frame(odo.frame(i), frames[i], f"{tag} frame {i}")
            if nonempty:
                assert len(frames[i]["kps"]) > 0, f"{tag} frame {i}: the oracle found nothing"
        _, th = odo.adaptive_state()
        assert np.array_equal(th, ex.thresh), f"{tag}: persistent thresholds {th} vs {ex.thresh}"
    finally:
        odo.close()
    return frames


# ---------------------------------------------------------------- selection
@pytest.fixture(scope="module")
def select_ctx():
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(320, 240, 1, detector=pkg.DETECTOR_ADAPTIVE_FAST))
    yield odo
    odo.close()


@pytest.mark.parametrize("name,keys,nth,must_hit", [pytest.param(*c, id=c[0]) for c in R.killer_cases()])
def test_select_at_the_depth_limit_and_tiny(select_ctx, name, keys, nth, must_hit):
    """std::nth_element / retainBest through odo_debug_select on adversary
    inputs that exhaust introselect's depth (asserted from the model alone),
    on such a block in front of 2750 tied elements, and on 1..4 equal
    elements up to nth = n."""
    n = len(keys)
    info = {}
    R.nth_element_packed(keys, nth, info)
    assert bool(info.get("depth_limit")) == must_hit, "the model does not reach the depth limit on this input"
    ref = keys.copy()
    O.lib().oracle_nth_element_score(O.ptr(ref), n, nth)
    got, m = select_ctx.select(keys, nth, 0)
    assert m == n and np.array_equal(got, ref), "nth_element permutation differs"
    ref2 = keys.copy()
    m2 = O.lib().oracle_retain_best_score(O.ptr(ref2), n, nth)
    got2, g2 = select_ctx.select(keys, nth, 1)
    assert g2 == m2 and np.array_equal(got2[:g2], ref2[:m2]), "retainBest differs"


# ---------------------------------------------------------------- FAST inner
@pytest.mark.parametrize("case", R.cases(), ids=repr)
def test_fast_inner_case(case):
    pkg = load_pkg()
    bgr = np.stack([R.to_bgr(g) for g in case.frames])
    dep = np.full((case.n, case.h, case.w), DEPTH, np.uint16)
    frames = check_batch(pkg, case.params, bgr, dep, case.start, "fast", case.nlevels(), case.name)
    if case.name in ("narrow_62", "low_62"):
        assert all(len(f["kps"]) == 0 for f in frames)


# ---------------------------------------------------------------- ORB inner
def orb_cases():
    return [
        # one cell = the whole frame: the cell pyramid exceeds the LDS level buffers
        ("orb_1x1", 640, 480, dict(grid_rows=1, grid_cols=1, cell_min=200, cell_max=400, retain_best=500), None),
        ("orb_2x5", 320, 240, dict(grid_rows=2, grid_cols=5, max_total_keypoints=600, cell_min=20, cell_max=60,
                                   escape_iters=1, retain_best=-1), None),
        ("orb_3x5_edge0", 320, 240, dict(grid_rows=3, grid_cols=5, edge_threshold=0, max_total_keypoints=450,
                                         cell_min=5, cell_max=40, retain_best=100), np.linspace(3.0, 45.0, 15)),
    ]


@pytest.mark.parametrize("name,w,h,params,start", [pytest.param(*c, id=c[0]) for c in orb_cases()])
def test_orb_inner_case(name, w, h, params, start):
    """Noise frames and one rendered frame in one batch; the oracle finds
    keypoints on every one."""
    pkg = load_pkg()
    rng = np.random.default_rng(len(name))
    rb, rd, _ = sequence(1, w=w, h=h, seed=0x5EED0016)
    nz = 1 if w == 640 else 2
    bgr = np.concatenate([rng.integers(0, 256, (nz, h, w, 3), dtype=np.uint8), np.asarray(rb)[:1]])
    dep = np.concatenate([rng.integers(2000, 20000, (nz, h, w)).astype(np.uint16), np.asarray(rd)[:1]])
    check_batch(pkg, params, np.ascontiguousarray(bgr), np.ascontiguousarray(dep), start, "orb", 8, name,
                nonempty=True)


def windows_past_level_edges(frames, w, h):
    """Per level edge (left, top, right, bottom): how many oracle keypoints
    have an rBRIEF window, 18 px around the centre cvRound(pt / scale) of
    their octave's level of the frame pyramid, that crosses it."""
    lw, lh = np.zeros(8, np.int32), np.zeros(8, np.int32)
    sc, q = np.zeros(8, np.float32), np.zeros(8, np.int32)
    O.lib().oracle_orbcv_levels(w, h, O.ptr(lw), O.ptr(lh), O.ptr(sc), O.ptr(q))
    hits = np.zeros(4, np.int64)
    for f in frames:
        k = f["kps"]
        o = k["octave"]
        inv = np.float32(1) / sc[o]
        cx, cy = np.rint(k["x"] * inv).astype(np.int64), np.rint(k["y"] * inv).astype(np.int64)
        hits += [np.sum(cx < 18), np.sum(cy < 18), np.sum(cx + 18 >= lw[o]), np.sum(cy + 18 >= lh[o])]
    return hits


def test_orb_inner_windows_leave_the_level():
    """rBRIEF windows that cross each of the four edges of their level (the
    byte-by-byte REFLECT_101 staging of k_oa_finalize), in workgroups that also
    hold in-level keypoints and, at a frame's end, invalid slots.

    orb_3x5_edge0's grid, overlap, totals and start thresholds with
    retain_best off, on noise in 6 x 6 px blocks: white noise has FAST corners
    on level 0 only, whose windows runByImageBorder(31) keeps inside; blocks
    give the cell pyramids corners up to octave 4, and a cell at the frame's
    border then puts a centre within 18 px of its level's edge. Seed chosen
    with the oracle: 4 / 2 / 5 / 3 such keypoints, 245 and 301 per frame."""
    pkg = load_pkg()
    w, h, b = 320, 240, 6
    rng = np.random.default_rng(3)
    blocks = rng.integers(0, 256, (2, h // b, -(-w // b), 3), dtype=np.uint8)
    bgr = np.ascontiguousarray(np.repeat(np.repeat(blocks, b, 1), b, 2)[:, :h, :w])
    dep = rng.integers(2000, 20000, (2, h, w)).astype(np.uint16)
    params = dict(grid_rows=3, grid_cols=5, edge_threshold=0, max_total_keypoints=450, cell_min=5, cell_max=40,
                  retain_best=-1)
    frames = check_batch(pkg, params, bgr, dep, np.linspace(3.0, 45.0, 15), "orb", 8, "orb_3x5_edge0_blocks",
                         nonempty=True)
    hits = windows_past_level_edges(frames, w, h)
    assert hits.min() >= 1, f"windows past the (left, top, right, bottom) level edges: {hits}"
    assert any(len(f["kps"]) % 8 for f in frames), "no frame ends inside a finalize workgroup"


# ---------------------------------------------------------------- refusals
def orb_min_quota():
    lw, lh = np.zeros(8, np.int32), np.zeros(8, np.int32)
    sc, q = np.zeros(8, np.float32), np.zeros(8, np.int32)
    O.lib().oracle_orbcv_levels(640, 480, O.ptr(lw), O.ptr(lh), O.ptr(sc), O.ptr(q))
    return int(q.min())


def refusals():
    both = ("fast", "orb")
    return [
        ("cells_65", 640, 480, dict(grid_rows=5, grid_cols=13), both, "invalid adaptive params"),
        ("cells_16_orb", 640, 480, dict(grid_rows=4, grid_cols=4), ("orb",), "more than 15 grid cells"),
        ("escape_0", 640, 480, dict(escape_iters=0), both, "invalid adaptive params"),
        ("min_above_max", 640, 480, dict(min_thresh=30.0, max_thresh=20.0), both, "invalid adaptive params"),
        ("total_below_cells", 640, 480, dict(max_total_keypoints=8), both, "invalid adaptive params"),
        ("cell_too_wide", 1100, 240, dict(grid_rows=1, grid_cols=1), both, "wider than AD_MAXW"),
        ("cell_max_at_quota", 640, 480, dict(cell_max=orb_min_quota()), ("orb",), "level quota <= cell_max"),
        ("cell_max_above_quota", 640, 480, dict(cell_max=orb_min_quota() + 1), ("orb",), "level quota <= cell_max"),
    ]


def refuse_all(pkg):
    for name, w, h, params, inners, msg in refusals():
        for inner in inners:
            with pytest.raises(RuntimeError, match=msg):
                pkg.Odometry(config(pkg, w, h, 1, params, inner))


def test_bad_parameters_are_refused_and_leave_nothing_behind():
    """odo_create fails with the argument error; a second round of refusals
    takes no device memory beyond the first (which absorbs the runtime's
    one-time allocations); a default context created afterwards works."""
    import torch
    pkg = load_pkg()
    free = []
    for _ in range(2):
        refuse_all(pkg)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[1] >= free[0], f"refused contexts kept {free[0] - free[1]} bytes of device memory"
    # one quota below the refusal: the ORB-inner context is accepted
    pkg.Odometry(config(pkg, 640, 480, 1, dict(cell_max=orb_min_quota() - 1), "orb")).close()
    rng = np.random.default_rng(7)
    bgr = rng.integers(0, 256, (1, 240, 320, 3), dtype=np.uint8)
    dep = np.full((1, 240, 320), DEPTH, np.uint16)
    for inner in ("fast", "orb"):
        check_batch(pkg, {}, bgr, dep, None, inner, 8, f"default {inner}", nonempty=True)
