"""odo_projection_match at the shapes where its search can go wrong: the entry
point runs the local-map search (k_localmap.hip: keypoint grid, candidate
lists of 16, a wave per longer list, the relaxation resolver) over one frame of
host inputs.

Every case compares the device with oracle_projection_match as
test_projection.test_gpu_projection_match does: slot_lm, the proj bit patterns
(NaNs included) and n_matches, all identical. One exception, as in
test_localmap_gpu.test_camera_centre_landmark: the projection of a landmark
with Pc == 0 is the NaN of an invalid operation, whose sign the hardware
chooses, so that row is compared as NaN.

The inputs come from test_projection.make_problem, the builders of
localmap_ref.py and, where a case needs keypoints at chosen pixels, landmarks
placed in front of an identity pose. Each case states how many landmarks must
be in view and matched in the reference, so none passes vacuously. th = +inf is
defined by the reference loop (every keypoint is in the window) and is kept.
"""
import ctypes as C

import numpy as np
import pytest

import localmap_ref as R
import oracle_lib as O
import test_projection as TP
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

NL_EDGES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
NAMES = (["n0", "nL0", "n1"] + [f"nL{k}" for k in NL_EDGES] +
         ["taken_half", "taken_null", "taken_all", "th0", "th1000", "thinf", "bounds", "dup", "onecell", "pcz0", "n8191"])


# ------------------------------------------------------------------ builders
def flip(desc, share, rng):
    """desc (m x 32 bytes) with a share of its bits flipped."""
    return np.packbits(np.unpackbits(desc, axis=1) ^ (rng.random((len(desc), 256)) < share).astype(np.uint8), axis=1)


def pixel_landmarks(px, py, desc, cal, flags, z=2.0):
    """Landmarks that an identity pose projects to about (px, py)."""
    lms = np.zeros(len(px), O.LANDMARK_DTYPE)
    zz = np.float64(z)
    lms["X"] = np.stack([(px - cal.cx) / cal.fx * zz, (py - cal.cy) / cal.fy * zz, np.full(len(px), zz)], 1).astype(np.float32)
    lms["desc"] = desc
    lms["flags"] = flags
    return lms


def pixel_problem(kun, octave, desc, pick, cal, rng, th, share=0.03, jitter=1.5, taken=None):
    """Identity pose; one landmark per keypoint of `pick`, a jitter away from
    it, with the keypoint's descriptor (a share of bits flipped); 70 % HAS_OBS."""
    px = kun[pick, 0].astype(np.float64) + rng.uniform(-jitter, jitter, len(pick))
    py = kun[pick, 1].astype(np.float64) + rng.uniform(-jitter, jitter, len(pick))
    d = flip(desc[pick], share, rng) if share else desc[pick].copy()
    fl = np.where(rng.random(len(pick)) < 0.7, R.HAS_OBS, 0)
    return dict(lms=pixel_landmarks(px, py, d, cal, fl), Tcw=np.eye(4, dtype=np.float32),
                kun=np.ascontiguousarray(kun, np.float32), octave=np.ascontiguousarray(octave, np.int32),
                desc=np.ascontiguousarray(desc, np.uint8),
                taken=np.zeros(len(kun), np.uint8) if taken is None else taken, cal=cal, th=th)


def build_problems():
    """name -> (problem, landmarks that must be in view, matches that must exist)."""
    base = TP.make_problem(1)
    cal = base["cal"]
    frames, poses = R.oracle_frames()
    big = R.contended_landmarks(frames, poses)  # three copies of every landmark, all with observations
    b = R.image_bounds(cal)
    n = len(base["kun"])
    sl0 = oracle(base)[0]
    out = {}

    def derive(**kw):
        P = dict(base)
        P.update(kw)
        return P

    out["n0"] = derive(kun=np.zeros((0, 2), np.float32), octave=np.zeros(0, np.int32), desc=np.zeros((0, 32), np.uint8),
                       taken=np.zeros(0, np.uint8)), 1, 0
    out["nL0"] = derive(lms=base["lms"][:0]), 0, 0
    j = int(np.nonzero(sl0 >= 0)[0][0])  # a keypoint the base problem matches
    out["n1"] = derive(kun=base["kun"][j:j + 1].copy(), octave=base["octave"][j:j + 1].copy(),
                       desc=base["desc"][j:j + 1].copy(), taken=np.zeros(1, np.uint8)), 1, 1
    for k in NL_EDGES:
        out[f"nL{k}"] = derive(lms=np.ascontiguousarray(big[:k])), 1, (10 if k >= 63 else 0)
    rng = np.random.default_rng(17)
    out["taken_half"] = derive(taken=(rng.random(n) < 0.5).astype(np.uint8)), 1, 10
    out["taken_null"] = derive(taken=None), 1, 10
    out["taken_all"] = derive(taken=np.ones(n, np.uint8)), 1, 0
    out["th0"] = derive(th=0.0), 1, 0
    out["th1000"] = derive(th=1000.0), 1, 1
    out["thinf"] = derive(th=float("inf")), 1, 1

    # keypoints exactly on the image bounds, and outside them (clamped cells)
    kun = base["kun"].copy()
    moved = rng.choice(n, 18, replace=False)
    x, y = kun[moved, 0].copy(), kun[moved, 1].copy()
    at = [(b[0], y[0]), (b[1], y[1]), (x[2], b[2]), (x[3], b[3]), (b[0], b[2]), (b[1], b[3]), (b[0], b[3]), (b[1], b[2]),
          (b[0] - 5, y[8]), (b[1] + 7.5, y[9]), (x[10], b[2] - 3), (x[11], b[3] + 20), (b[0] - 40, b[2] - 40),
          (b[1] + 100, b[3] + 100), (-1e6, y[14]), (1e6, y[15]), (x[16], -1e6), (x[17], 1e6)]
    kun[moved] = np.array(at, np.float32)
    pick = np.concatenate([moved, rng.choice(n, 200, replace=False)])
    P = pixel_problem(kun, base["octave"], base["desc"], pick, cal, rng, th=8.0, jitter=3.0)
    # landmarks aimed at keypoints off the image land outside the bounds: aim them at the nearest pixel inside
    X = P["lms"]["X"]
    lo = ((np.array([b[0], b[2]]) + 0.5 - [cal.cx, cal.cy]) / [cal.fx, cal.fy] * 2.0).astype(np.float32)
    hi = ((np.array([b[1], b[3]]) - 0.5 - [cal.cx, cal.cy]) / [cal.fx, cal.fy] * 2.0).astype(np.float32)
    X[:, 0], X[:, 1] = np.clip(X[:, 0], lo[0], hi[0]), np.clip(X[:, 1], lo[1], hi[1])
    P["moved"] = moved
    out["bounds"] = P, 100, 10

    # two keypoints with the same coordinates and descriptor, the landmark's own: distance 0 twice, the index decides
    kun, octv, desc = base["kun"].copy(), base["octave"].copy(), base["desc"].copy()
    src = rng.choice(np.arange(50, n - 50), 20, replace=False)
    dst = src + np.where(np.arange(20) % 2, 37, -37)
    dst = np.where(np.isin(dst, src), dst + 1, dst)
    kun[dst], octv[dst], desc[dst] = kun[src], octv[src], desc[src]
    P = pixel_problem(kun, octv, desc, np.concatenate([src, rng.choice(n, 100, replace=False)]), cal, rng, th=8.0, share=0)
    P["lms"]["flags"] = 0  # no observations: no slot is ever taken, every landmark sees both keypoints
    P["dup"] = (src, dst)
    out["dup"] = P, 100, 10

    # every keypoint in one cell of the grid: one long run, a long cascade
    m = 300
    kun = np.stack([b[0] + 320.25 + 31.5 * rng.random(m), b[2] + 224.25 + 31.5 * rng.random(m)], 1).astype(np.float32)
    pick = np.arange(m) % 100
    P = pixel_problem(kun, base["octave"][:m], base["desc"][:m], pick, cal, rng, th=6.0, jitter=0.5)
    P["lms"]["flags"] = R.HAS_OBS
    out["onecell"] = P, 300, 10

    # Pc == 0: a NaN projection, in view, no match; Pc.z == 0 beside the axis: infinite, out of view
    P = pixel_problem(base["kun"], base["octave"], base["desc"], rng.choice(n, 100, replace=False), cal, rng, th=8.0)
    P["lms"]["X"][7] = (0.0, 0.0, 0.0)
    P["lms"]["X"][9] = (0.3, 0.0, 0.0)
    P["lms"]["flags"][[7, 9]] = R.HAS_OBS
    P["nan_rows"] = [7]
    out["pcz0"] = P, 50, 10

    # the most keypoints the entry point takes, uniformly placed
    m = 8191
    kun = np.stack([b[0] + (b[1] - b[0]) * rng.random(m), b[2] + (b[3] - b[2]) * rng.random(m)], 1).astype(np.float32)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    octv = rng.integers(0, 8, m).astype(np.int32)
    out["n8191"] = pixel_problem(kun, octv, desc, rng.choice(m, 600, replace=False), cal, rng, th=8.0,
                                 taken=(rng.random(m) < 0.1).astype(np.uint8)), 300, 10
    assert sorted(out) == sorted(NAMES)
    return out


def oracle(P):
    """(slot_lm, proj, n_matches) of the reference; empty inputs as one unused row."""
    n, nL = len(P["kun"]), len(P["lms"])
    b = R.image_bounds(P["cal"])
    sl = np.full(max(n, 1), -1, np.int32)
    proj = np.full((max(nL, 1), 3), np.nan, np.float32)
    kun = P["kun"] if n else np.zeros((1, 2), np.float32)
    octv = P["octave"] if n else np.zeros(1, np.int32)
    desc = P["desc"] if n else np.zeros((1, 32), np.uint8)
    taken = P["taken"] if P["taken"] is not None and n else np.zeros(max(n, 1), np.uint8)
    lms = P["lms"] if nL else np.zeros(1, O.LANDMARK_DTYPE)
    T = np.ascontiguousarray(P["Tcw"], np.float32).ravel()
    nm = O.lib().oracle_projection_match(O.ptr(T), O.ptr(lms), nL, O.ptr(kun), O.ptr(octv), O.ptr(desc), n, O.ptr(taken),
                                         C.byref(P["cal"]), O.ptr(b), P["th"], 0.8, O.ptr(sl), O.ptr(proj))
    return sl[:n], proj[:nL], int(nm)


def device(ctx, P):
    """odo_projection_match; null pointers for empty inputs and for no taken slots."""
    pkg, odo = ctx
    n, nL = len(P["kun"]), len(P["lms"])
    sl = np.full(n, -7, np.int32)
    proj = np.full((nL, 3), 7.0, np.float32)
    nm = C.c_int(-7)
    arr = lambda a, m: pkg.ptr(np.ascontiguousarray(a)) if m else None
    T = np.ascontiguousarray(P["Tcw"], np.float32).ravel()
    rc = odo.lib.odo_projection_match(odo.h, pkg.ptr(T), arr(P["lms"], nL), nL, arr(P["kun"], n), arr(P["octave"], n),
                                      arr(P["desc"], n), n, arr(P["taken"], n and P["taken"] is not None), P["th"], 0.8,
                                      pkg.ptr(sl) if n else None, pkg.ptr(proj) if nL else None, C.byref(nm))
    return rc, sl, proj, nm.value


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def problems():
    return {name: (P, nv, nm, oracle(P)) for name, (P, nv, nm) in build_problems().items()}


@pytest.fixture(scope="module")
def ctx():
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=R.NF))
    yield pkg, odo
    odo.close()


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", NAMES)
def test_edge(ctx, problems, name):
    P, min_view, min_matches, (sl_ref, proj_ref, nm_ref) = problems[name]
    in_view = int((~np.isnan(proj_ref[:, 0])).sum()) if len(proj_ref) else 0
    print(f"{name}: n {len(P['kun'])} landmarks {len(P['lms'])} th {P['th']} in view {in_view} matches {nm_ref}")
    assert in_view >= min_view and nm_ref >= min_matches, "the case does not exercise what it is for"
    if name in ("taken_all", "th0", "n0", "nL0"):
        assert nm_ref == 0
    if name == "bounds":
        assert (sl_ref[P["moved"]] >= 0).sum() >= 8  # keypoints on and beyond the bounds hold landmarks
    if name == "dup":
        # the lower index of each pair holds a landmark, the higher never does
        src, dst = P["dup"]
        assert (sl_ref[np.minimum(src, dst)] >= 0).sum() >= 10 and (sl_ref[np.maximum(src, dst)] < 0).all()
    rc, sl, proj, nm = device(ctx, P)
    assert rc == 0
    assert nm == nm_ref
    assert np.array_equal(sl, sl_ref), f"slot assignments differ at {np.nonzero(sl != sl_ref)[0][:10]}"
    for r in P.get("nan_rows", []):
        assert np.isnan(proj[r]).all() and np.isnan(proj_ref[r]).all()
        proj[r] = proj_ref[r]
    assert np.array_equal(proj.view(np.uint32), proj_ref.view(np.uint32)), "projections differ"


def test_capacity(ctx, problems):
    """8192 keypoints do not fit the 13-bit keypoint index of a candidate."""
    pkg, odo = ctx
    P = dict(problems["n8191"][0])
    for k in ("kun", "octave", "desc", "taken"):
        P[k] = np.concatenate([P[k], P[k][:1]])
    rc, _, _, nm = device(ctx, P)
    assert rc == pkg._abi.ERR_CAPACITY


def test_local_map_results_survive(ctx, problems):
    """The call uses scratch of its own: odo_get_local_map still returns the
    last odo_track_local_map's results, for every frame of the batch."""
    pkg, odo = ctx
    bgr, dep, poses = sequence(3, seed=R.SEQ_SEED)
    odo.track_batch_host(np.ascontiguousarray(bgr[1:3]), np.ascontiguousarray(dep[1:3]))
    frames = [odo.frame(i) for i in range(2)]
    lms = R.landmark_mix([None, frames[0]], [None, poses[1]])
    res = odo.track_local_map(lms, R.true_poses(poses, (1, 2)), th=8.0)
    assert all(r["n_matches"] > 50 for r in res)
    before = [odo.local_map(i) for i in range(2)]
    for name in ("taken_half", "nL1025"):  # fewer and more landmarks than the batch call had
        P, _, _, (sl_ref, _, nm_ref) = problems[name]
        rc, sl, _, nm = device(ctx, P)
        assert rc == 0 and nm == nm_ref and np.array_equal(sl, sl_ref)
    after = [odo.local_map(i) for i in range(2)]
    for x, y in zip(before, after):
        assert np.array_equal(x["slot_lm"], y["slot_lm"]) and np.array_equal(x["pnp_outlier"], y["pnp_outlier"])
        assert np.array_equal(x["proj"].view(np.uint32), y["proj"].view(np.uint32))
