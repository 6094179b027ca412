"""CPU tests of the batched ADAPTIVE_RICP / RANSAC odometry modes: the crafted
sequence drives the reference composition (ricp_ref, built on the CPU oracle)
through every branch of odometry.cpp:52-68, the decision is inclusive at
equality, and the library's device-free entry points (the default constants,
the argument checks) answer without a GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import ricp_ref as RR
from conftest import load_pkg


@pytest.fixture(scope="module")
def crafted():
    cal = O.fr1_calib()
    bgr, dep = RR.crafted_sequence()
    frames = RR.extract_frames(bgr, dep, cal)
    passes = RR.ransac_pass(frames, cal, O.ransac_params(), lambda i: 1234 + i)
    return frames, passes, RR.compose(frames, passes, O.ransac_params())


def test_crafted_sequence_takes_every_branch(crafted):
    """A condition on the inputs: under the reference's constants the sequence
    yields branch 0, branch 2, branch 1 with a real GICP and branch 1 with an
    empty cloud (with and without matches)."""
    _, _, ref = crafted
    for i, e in ref.items():
        r = e["res"]
        print(f"pair {i}: {RR.kind(e)} matches {r.n_matches} good {r.n_good} inliers {r.n_inliers} "
              f"rmse {r.rmse:.4f} cloud {len(e['src'])} conv {e['converged']} it {e['iterations']} "
              f"corr {e['n_corr']}")
    kinds = {i: RR.kind(e) for i, e in ref.items()}
    assert kinds[1] == "keep" and ref[1]["res"].n_inliers >= 20
    for i in (2, 3, 6, 9):
        assert kinds[i] == "refine" and ref[i]["converged"] and ref[i]["n_corr"] >= 4, f"pair {i}"
    for i in (7, 8):
        assert kinds[i] == "reset_gicp" and not ref[i]["res"].ransac_ok, f"pair {i}"
        assert np.float32(ref[i]["res"].rmse) == np.float32(1e6) and ref[i]["converged"], f"pair {i}"
    assert kinds[4] == "reset_empty" and ref[4]["res"].n_matches >= 20 and ref[4]["res"].n_good == 0
    for i in (5, 10, 11):
        assert kinds[i] == "reset_empty" and ref[i]["res"].n_matches == 0, f"pair {i}"
    # the fallbacks of a GICP that does not run: identity on branch 1
    for i in (4, 5, 10, 11):
        assert np.array_equal(ref[i]["Tcw"], np.eye(4, dtype=np.float32))
    assert np.array_equal(ref[1]["Tcw"], ref[1]["T_ransac"])


def test_decision_is_inclusive_at_equality(crafted):
    """rmse * 10.0f >= refine_at (odometry.cpp:52): a refine_at of exactly
    float(rmse) * float(10) of pair 1 sends it to GICP, the next float up
    keeps RANSAC's pose."""
    frames, passes, ref = crafted
    r = ref[1]["res"]
    at = np.float32(r.rmse) * np.float32(10)
    assert RR.decide(r.rmse, r.n_inliers, dict(RR.DEFAULTS, refine_at=at)) == 2
    assert RR.decide(r.rmse, r.n_inliers, dict(RR.DEFAULTS, refine_at=np.nextafter(at, np.float32(np.inf)))) == 0
    got = RR.compose(frames, {1: passes[1]}, O.ransac_params(), refine_at=float(at))
    assert got[1]["branch"] == 2 and len(got[1]["src"]) == r.n_good


def test_default_ricp_params_are_the_reference_constants():
    """odometry.cpp:15 (GeneralizedICP(10, 0.07)) and 52-53 (20, 10.0f, 7.0f, 20)."""
    pkg = load_pkg()
    p = pkg.default_ricp_params()
    assert C.sizeof(pkg.RicpParams) == 32 and C.sizeof(pkg.RicpResult) == 96
    assert (p.min_inliers, p.rmse_scale, p.refine_at, p.reset_at, p.gicp_iterations, p.gicp_max_corr_dist) == \
        (20, 10.0, 7.0, 20.0, 10, 0.07)
    assert {k: getattr(p, k) for k in RR.DEFAULTS} == RR.DEFAULTS


def test_odometry_entry_points_check_their_arguments():
    """Device-free checks (ODO_ERR_ARG = -1, with a message): a NULL context, an
    unknown mode and bad ADAPTIVE_RICP constants."""
    pkg = load_pkg()
    lib = pkg.load()
    buf = (C.c_uint8 * 128)()
    assert lib.odo_set_odometry(None, pkg.ODOMETRY_ADAPTIVE_RICP, None) == -1
    assert b"null ctx" in lib.odo_last_error()
    assert lib.odo_get_odometry(None) == -1 and lib.odo_last_error()
    assert lib.odo_get_ricp(None, 0, buf, None, None, 0) == -1 and lib.odo_last_error()
    for mode in (-1, 3, 7):
        assert lib.odo_set_odometry(None, mode, None) == -1, mode
        assert b"unknown odometry mode" in lib.odo_last_error()
    for field, bad in (("gicp_iterations", 0), ("gicp_max_corr_dist", 0.0), ("gicp_max_corr_dist", float("nan")),
                       ("refine_at", float("inf")), ("reset_at", float("nan")), ("rmse_scale", float("-inf"))):
        p = pkg.default_ricp_params()
        setattr(p, field, bad)
        assert lib.odo_set_odometry(None, pkg.ODOMETRY_ADAPTIVE_RICP, C.byref(p)) == -1, field
        assert b"ricp" in lib.odo_last_error(), field
