"""odo_local_ba (csrc/k_ba.hip) against the float64 reference at edge shapes.

Reference: tests/ba_ref64.py, checked on the CPU by tests/test_ba_ref64.py.
Per case:
  poses, points   within pose_ref64.bound_vs_ref64(d, magnitude), d the
                  reference's own largest distance between its natural-order /
                  LDL^T run and its reversed-order / numpy.linalg.solve run
                  (what another summation order and factorisation cost,
                  measured on the reference, never on the kernel); 4 x that,
                  at least 4 float32 ulps of the case's largest magnitude
  erase, level 1  equal, except on edges whose reference chi2 is within 2 % of
                  its threshold, and at most 1 % of the case's edges
  iterations and trials of both stages equal to the reference's
Widths the cases sit around (ba_ref64.BA_CHUNK, BA_BLOCK, BA_TILE): the
landmark chunk of the partial reduced systems (127 / 128 / 129 landmarks), the
256-thread workgroups of the per-landmark and per-edge kernels (255 / 256 / 257
landmarks, more than 256 edges), the 64-lane wave (63 / 64 / 65), the 32-wide
tile of the factorisation's trailing update (5, 6, 16 free keyframes: 30, 36,
96 rows) and its 384-row limit (63, 64 free keyframes), and the limit of 64
chunks (BA_MAX_CHUNKS): 8191 / 8192 landmarks are 64 chunks of 128, 8193 are
64 of 129 and 20 000 are 64 of 313; in those cases about 300 landmarks carry
edges, in the first and last chunk, across chunk boundaries and in more than
half the chunks (tests/test_ba_ref64.py::test_case_shapes), the others none.
Three cases run a shortened second stage: `all` (5 iterations), `fixed_only`
and `all_fixed` (4). Where only points move, or every keyframe sees every
landmark, the reference converges to rounding within a few iterations, and its
own trial counts then change with the edge order (ba_ref64.MIN_DECISION), so
the default 10-iteration second stage is not compared on those structures.
The failed-solve path (a pivot exactly zero) is not reached by any case.
"""
import numpy as np
import pytest

import ba_ref64 as B
from pose_ref64 import Cam, bound_vs_ref64
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=500, iterations=50))
    yield pkg, odo
    odo.close()


def calib(pkg):
    c = pkg.Calib()
    c.fx, c.fy, c.cx, c.cy, c.mbf = Cam.fx, Cam.fy, Cam.cx, Cam.cy, Cam.bf
    return c


def params(pkg, d):
    p = pkg.BaParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def run(ctx, c):
    pkg, odo = ctx
    return odo.local_ba(c["Tcw"], c["fixed"], c["Xw"], c["edges"], calib(pkg), params(pkg, c["params"]))


@pytest.mark.parametrize("name", B.CASES)
def test_against_float64(ctx, name):
    c = B.ba_case(name)
    ref, _, d = B.ba_case_refs(name)
    T, X, erase, res = run(ctx, c)
    assert T.dtype == np.float32 and X.dtype == np.float32 and erase.dtype == np.uint8
    mag = max(float(np.abs(ref["Tcw64"]).max()), float(np.abs(ref["Xw64"]).max()))
    bound = bound_vs_ref64(d, mag)
    dT = float(np.abs(T.astype(np.float64) - ref["Tcw64"]).max())
    dX = float(np.abs(X.astype(np.float64) - ref["Xw64"]).max())
    print(f"{name}: d {d:.3e} gpu poses {dT:.3e} points {dX:.3e} bound {bound:.3e} iters {res.iters1}/{res.iters2} "
          f"trials {res.trials1}/{res.trials2} ref {ref['iters']} {ref['trials']} level1 {res.n_level1} erase {res.n_erase}")
    assert res.status == pkg_of(ctx).BA_RAN
    assert (res.iters1, res.iters2) == tuple(ref["iters"]), f"iterations {res.iters1}, {res.iters2} vs {ref['iters']}"
    assert (res.trials1, res.trials2) == tuple(ref["trials"]), f"trials {res.trials1}, {res.trials2} vs {ref['trials']}"
    assert dT <= bound and dX <= bound
    assert res.n_erase == int(erase.sum())
    B.flags_agree(erase, res.n_level1, ref, c["edges"], c["params"], name)
    # the reported chi2: the same rule, on the reference's own two values
    ref_b = B.ba_case_refs(name)[1]
    for key, got in (("chi2_initial", res.chi2_initial), ("chi2_stage1", res.chi2_stage1), ("chi2_final", res.chi2_final)):
        cb = max(4.0 * abs(ref[key] - ref_b[key]), 4.0 * float(np.finfo(np.float32).eps) * abs(ref[key]))
        assert abs(got - ref[key]) <= cb, (key, got, ref[key], cb)
    # vertices outside the system come back bit for bit
    E = c["edges"]
    out_kf = np.ones(len(c["Tcw"]), bool)
    out_kf[np.unique(E["kf"])] = False
    out_kf |= c["fixed"].astype(bool)
    assert T[out_kf].tobytes() == c["Tcw"][out_kf].tobytes()
    out_lm = np.ones(len(c["Xw"]), bool)
    out_lm[np.unique(E["lm"])] = False
    assert X[out_lm].tobytes() == c["Xw"][out_lm].tobytes()
    assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(T), 1)))


def pkg_of(ctx):
    return ctx[0]


def test_case_properties(ctx):
    """The stage-logic cases cover what they are named for (on the reference),
    and the device agrees on it."""
    c = B.ba_case("lm_all_level1")
    ref = B.ba_case_refs("lm_all_level1")[0]
    s = c["edges"]["lm"] == 5
    assert ref["level1"][s].all() and s.sum() >= 2
    T, X, erase, res = run(ctx, c)
    # out of the system in stage 2: the landmark keeps its stage-1 estimate
    assert np.abs(X[5].astype(np.float64) - ref["Xw64_stage1"][5]).max() <= bound_vs_ref64(0.0, np.abs(ref["Xw64"]).max())
    assert erase[s].all()
    c = B.ba_case("behind")
    ref = B.ba_case_refs("behind")[0]
    s = c["edges"]["lm"] == 3
    assert ref["erase"][s].all()
    assert run(ctx, c)[2][s].all()
    c = B.ba_case("ends_behind")  # in front at the start, behind keyframe kf_moved at the end: the depth test alone
    ref = B.ba_case_refs("ends_behind")[0]
    e = int(np.nonzero((c["edges"]["kf"] == c["kf_moved"]) & (c["edges"]["lm"] == 7))[0][0])
    assert ref["erase"][e] and ref["chi2"][e] < c["params"]["chi2_mono"]
    T, X, erase, res = run(ctx, c)
    assert erase[e] == 1
    assert (T[c["kf_moved"]].astype(np.float64)[2, :3] @ X[7] + T[c["kf_moved"]][2, 3]) < 0
    c = B.ba_case("free_kf_no_edge")
    assert not c["fixed"][-1] and not (c["edges"]["kf"] == len(c["fixed"]) - 1).any()
    c = B.ba_case("fixed_only")
    assert c["fixed"][np.unique(c["edges"]["kf"])].all() and not c["fixed"].all()
    T = run(ctx, c)[0]
    assert T.tobytes() == c["Tcw"].tobytes()  # only points move
    ref = B.ba_case_refs("rejected")[0]
    assert max(ref["trials_per_iter"][0] + ref["trials_per_iter"][1]) > 1
    assert any(max(B.ba_case_refs(n)[0]["trials_per_iter"][0]) > 1 for n in ("s1_0_40_kf0_free", "once"))


def test_repeatable_and_scratch_growth(ctx):
    """Two calls on the same input give identical bytes, also after a larger
    problem has grown the scratch in between."""
    small, big = B.ba_case("s2_1_16"), B.ba_case("s4_2_300")
    pkg = pkg_of(ctx)
    odo = pkg.Odometry(pkg.default_config(640, 480, 1, nfeatures=500, iterations=50))
    try:
        loc = (pkg, odo)
        a = run(loc, small)
        b = run(loc, small)
        run(loc, big)
        c = run(loc, small)
        for r in (b, c):
            assert r[0].tobytes() == a[0].tobytes() and r[1].tobytes() == a[1].tobytes() and r[2].tobytes() == a[2].tobytes()
            assert bytes(r[3]) == bytes(a[3])
        for other in (big, B.ba_case("lm20000")):  # the second: 64 chunks of 313 landmarks
            b1, b2 = run(loc, other), run(loc, other)
            assert b1[0].tobytes() == b2[0].tobytes() and b1[1].tobytes() == b2[1].tobytes()
            assert b1[2].tobytes() == b2[2].tobytes() and bytes(b1[3]) == bytes(b2[3])
    finally:
        odo.close()


def test_block_regrows_past_its_floor_and_results_repeat(ctx):
    """A fresh context: a small call, one that outgrows the device block, the
    small one again. The block starts at its floor of 1 MiB and holds the packed
    inputs and outputs plus ba_scratch_bytes. The large problem is 4 free and 1
    fixed keyframe that each see all 2048 landmarks: 5 * 2048 = 10 240 edges.
    The per-edge scratch sections alone (c2 8, W 144, flags 1, flist 8 = 161
    bytes an edge) take 10 240 * 161 = 1 648 640 bytes > 1 048 576. The small
    results are byte-identical, and the large one equals the same call on
    another fresh context."""
    pkg = pkg_of(ctx)
    small = B.ba_case("s2_1_16")
    big = B.make_scene([0xB16, 0], 4, 1, 2048, obs="all", iters_robust=2, iters_final=2)
    assert len(big["edges"]) == 10240

    def fresh():
        return pkg, pkg.Odometry(pkg.default_config(640, 480, 1, nfeatures=500, iterations=50))

    def as_bytes(r):
        return r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), bytes(r[3])

    one, two = fresh(), fresh()
    try:
        a = as_bytes(run(one, small))
        b = as_bytes(run(one, big))
        assert as_bytes(run(one, small)) == a
        assert as_bytes(run(two, big)) == b
        assert run(two, big)[3].status == pkg.BA_RAN
    finally:
        one[1].close()
        two[1].close()


def test_nothing_to_do(ctx):
    pkg, odo = ctx
    c = B.ba_case("s2_1_16")
    T, X, erase, res = odo.local_ba(c["Tcw"], c["fixed"], c["Xw"], c["edges"][:0], calib(pkg))
    assert res.status == pkg.BA_NOTHING and len(erase) == 0
    assert T.tobytes() == c["Tcw"].tobytes() and X.tobytes() == c["Xw"].tobytes()
    T, X, erase, res = odo.local_ba(c["Tcw"][:0], c["fixed"][:0], c["Xw"][:0], c["edges"][:0])
    assert res.status == pkg.BA_NOTHING and T.shape == (0, 4, 4)


def _raw(ctx, Tcw, fixed, Xw, E, prm=None):
    """The C entry point on copies; returns (rc, the arrays after the call)."""
    pkg, odo = ctx
    A = pkg._abi
    T, X = np.array(Tcw, np.float32), np.array(Xw, np.float32)
    fx, E = np.array(fixed, np.uint8), np.array(E, A.BA_EDGE_DTYPE)
    er = np.full(len(E), 7, np.uint8)
    res = A.BaResult()
    rc = odo.lib.odo_local_ba(odo.h, A.ptr(T), A.ptr(fx), len(T), A.ptr(X), len(X), A.ptr(E), len(E), None,
                              A.ptr(prm) if prm is not None else None, A.ptr(er), A.ptr(res))
    return rc, T, X, er


def test_errors_leave_the_arrays_untouched(ctx):
    pkg, odo = ctx
    A = pkg._abi
    c = B.ba_case("s2_1_16")
    T0, X0, E0, f0 = c["Tcw"], c["Xw"], c["edges"], c["fixed"]

    def expect(code, T=T0, f=f0, X=X0, E=E0, prm=None):
        rc, T1, X1, er = _raw(ctx, T, f, X, E, prm)
        assert rc == code, (rc, code)
        assert T1.tobytes() == np.asarray(T, np.float32).tobytes() and X1.tobytes() == np.asarray(X, np.float32).tobytes()
        assert (er == 7).all()

    for bad in (np.nan, np.inf):
        T = T0.copy()
        T[1, 0, 3] = bad
        expect(A.ERR_ARG, T=T)
        X = X0.copy()
        X[2, 1] = bad
        expect(A.ERR_ARG, X=X)
        E = E0.copy()
        E["v"][3] = bad
        expect(A.ERR_ARG, E=E)
    for z in (0.0, -0.0, 1e-30, -1e-25):  # 1.0f / (z * z) is infinite: z * z underflows in float
        X = X0.copy()
        X[4, 2] = z
        expect(A.ERR_ARG, X=X)
    for field, val in (("kf", -1), ("kf", len(T0)), ("lm", -1), ("lm", len(X0))):
        E = E0.copy()
        E[field][5] = val
        expect(A.ERR_ARG, E=E)
    expect(A.ERR_ARG, E=np.concatenate([E0, E0[:1]]))  # a (keyframe, landmark) pair twice
    p = pkg.default_ba_params()
    p.iters_robust = 0
    expect(A.ERR_ARG, prm=p)
    # capacity: 65 free keyframes, 257 keyframes, 65537 landmarks, 2^20 + 1 edges
    eye = np.tile(np.eye(4, dtype=np.float32), (257, 1, 1))
    expect(A.ERR_CAPACITY, T=eye[:65], f=np.zeros(65, np.uint8))
    expect(A.ERR_CAPACITY, T=eye, f=np.ones(257, np.uint8))
    expect(A.ERR_CAPACITY, X=np.ones((65537, 3), np.float32))
    big = np.zeros((1 << 20) + 1, A.BA_EDGE_DTYPE)
    expect(A.ERR_CAPACITY, E=big)
    assert odo.lib.odo_local_ba(None, None, None, 0, None, 0, None, 0, None, None, None, None) == A.ERR_ARG
    # 64 free keyframes of 256 are within capacity
    rc, _, _, _ = _raw(ctx, eye[:256], np.r_[np.zeros(64), np.ones(192)], X0, E0[:0])
    assert rc == 0


def test_between_two_batches():
    """A call between two odo_track_batch calls leaves their results equal to a run without it."""
    pkg = load_pkg()
    bgr, dep, _ = sequence(4)
    c = B.ba_case("s2_1_16")
    outs = []
    for with_ba in (False, True):
        odo = pkg.Odometry(pkg.default_config(640, 480, 2, nfeatures=500, iterations=50))
        try:
            r1 = odo.track_batch_host(bgr[:2], dep[:2])
            if with_ba:
                odo.local_ba(c["Tcw"], c["fixed"], c["Xw"], c["edges"], calib(pkg))
            r2 = odo.track_batch_host(bgr[2:4], dep[2:4])
            outs.append((r1.tobytes(), r2.tobytes()))
        finally:
            odo.close()
    assert outs[0] == outs[1]
