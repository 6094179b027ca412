"""The reference composition of the batched TrackLocalMap (tests/localmap_ref.py)
and the property its GPU kernel rests on, on the CPU: the serial landmark loop
of Matcher::ProjectionMatch (matcher.cpp:90-145) equals the fixed point of a
synchronous relaxation. Also the conditions that keep the GPU cases of
tests/test_localmap_gpu.py from passing by being easy, asserted from the
reference alone."""
import numpy as np
import pytest

import localmap_ref as R
import oracle_lib as O


@pytest.fixture(scope="module")
def seq():
    return R.oracle_frames()


@pytest.fixture(scope="module")
def problems(seq):
    fr, poses = seq
    return dict(base=R.base_problem(fr, poses), contended=R.contended_problem(fr, poses),
                wide=R.wide_problem(fr, poses), half_obs=R.half_obs_problem(fr, poses),
                prior=R.prior_problem(fr, poses))


@pytest.fixture(scope="module")
def relax(problems):
    return {k: R.relaxation_rounds(P, 2) for k, P in problems.items()}


def test_composition_without_prior_is_projection_match_then_pnp(seq, problems):
    """prior=None: exactly oracle_projection_match with no slot taken, then
    oracle_pnp over the matched slots from the pose given."""
    fr, poses = seq
    P = problems["base"]
    ref = R.compose(P)
    cal = P["cal"]
    b = R.image_bounds(cal)
    for i, f in enumerate(fr):
        n, nL = len(f["kun"]), len(P["lms"])
        sl = np.zeros(n, np.int32)
        proj = np.zeros((nL, 3), np.float32)
        T0 = np.ascontiguousarray(P["Tcw"][i]).ravel()
        nm = O.lib().oracle_projection_match(O.ptr(T0), O.ptr(P["lms"]), nL, O.ptr(np.ascontiguousarray(f["kun"])),
                                             O.ptr(np.ascontiguousarray(f["kps"]["octave"])),
                                             O.ptr(np.ascontiguousarray(f["desc"])), n, O.ptr(np.zeros(n, np.uint8)),
                                             O.C.byref(cal), O.ptr(b), 8.0, 0.8, O.ptr(sl), O.ptr(proj))
        r = ref[i]
        assert nm == r["n_matches"] and np.array_equal(sl, r["slot_lm"])
        assert np.array_equal(proj.view(np.uint32), r["proj"].view(np.uint32))
        assert r["n_in_view"] == int((~np.isnan(proj[:, 0])).sum())
        idx = np.nonzero(sl >= 0)[0]
        assert r["n_edges"] == len(idx) <= nm  # an untaken slot may be overwritten: fewer slots than matches
        Xw = np.ascontiguousarray(P["lms"]["X"][sl[idx]])
        obs = np.ascontiguousarray(np.column_stack([f["kun"][idx], f["ur"][idx]]), np.float32)
        T = np.zeros(16, np.float32)
        out = np.zeros(len(idx), np.uint8)
        ninl = O.lib().oracle_pnp(O.ptr(Xw), O.ptr(obs), len(idx), O.C.byref(cal), O.ptr(T0), O.ptr(T), O.ptr(out))
        assert ninl == r["pnp_inliers"] and np.array_equal(T, r["Tcw"])
        assert np.array_equal(out, r["pnp_outlier"][idx])


@pytest.mark.parametrize("name", ["base", "contended", "wide", "half_obs", "prior"])
def test_relaxation_reaches_the_serial_result(problems, relax, name):
    """The fixed point of the synchronous relaxation is the serial loop's
    result: same slots, same match count, on every builder and frame 2."""
    P = problems[name]
    sl, _, nm, _ = R.search(P, 2)
    x = relax[name]
    print(f"{name}: rounds {x.rounds} moved {x.moved} matches {x.n_matches} over16 {x.over16} shared {x.shared_slots}")
    assert x.n_matches == nm
    assert np.array_equal(x.slot_lm, sl)


def test_relaxation_every_frame_of_the_contended_case(problems):
    P = problems["contended"]
    for i in (0, 1):
        sl, _, nm, _ = R.search(P, i)
        x = R.relaxation_rounds(P, i)
        assert x.n_matches == nm and np.array_equal(x.slot_lm, sl)


def test_conditions_on_the_inputs(problems, relax):
    """The cases are hard where they claim to be."""
    c, w, h = relax["contended"], relax["wide"], relax["half_obs"]
    assert c.rounds >= 5 and c.moved >= 500, c[:2]
    assert w.rounds >= 8 and w.over16 >= 1000, (w.rounds, w.over16)
    assert h.n_matches >= 1000 and h.shared_slots >= 1, (h.n_matches, h.shared_slots)
    for r in R.compose(problems["base"]):
        assert r["n_matches"] > 50
    P = problems["prior"]
    for i in range(3):
        _, pr, taken = R.frame_state(P, i)
        assert (pr >= 0).sum() >= 100, (i, int((pr >= 0).sum()))
    # the prior case releases something, and holds taken and untaken slots
    raw = np.concatenate([p[p >= 0] for p in P["prior"]])
    assert (P["lms"]["flags"][raw] & R.BAD).any()
    _, pr, taken = R.frame_state(P, 2)
    assert taken.any() and (~taken.astype(bool) & (pr >= 0)).any()


def test_prior_landmarks_are_seen_for_their_frame_only(problems):
    P = problems["prior"]
    ref = R.compose(P)
    for i, r in enumerate(ref):
        pr = r["prior"]
        held = pr[pr >= 0]
        assert np.isnan(r["proj"][held, 0]).all()          # SEEN: not projected
        assert not np.isin(r["search_slot"], held).any()   # nor matched again
        tk = (P["lms"]["flags"][held] & R.HAS_OBS) != 0
        assert np.array_equal(r["slot_lm"][pr >= 0][tk], held[tk])  # taken priors stay
