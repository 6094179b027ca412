"""odo_pnp_ransac / odo_pnp_ransac_batch on the crafted cases of
pnpransac_cases.py: point counts at the widths of k_pr_count and of the
one-wave refine kernel, fold stops at the chunk edges of the batch path,
`iterations` and problem counts at 63 / 64 / 65, the comparisons that decide a
branch (planar or DLT, ni < 6, first of equal counts, rint, the redraw), and
degenerate or unvalidated input.

Two references. The oracle, exactly as test_pnpransac._check_gpu holds it
(integers and mask equal, model 1e-9, refined pose 1e-7). And, for every
ok = 1 case, the float64 least-squares minimum on the inlier set, which shares
nothing with the kernel or the oracle: the device pose lies within
4 d + FLT_EPSILON max|rt64| of it, d being the ORACLE's distance from that
minimum (test_pnpransac_cases.py prints it; 0 .. 1.6e-9 on these cases), 4 the
margin of pose_ref64.bound_vs_ref64, and the second term CvLevMarq's own stop
rule (a correct run may end once a step is below FLT_EPSILON relative).
PNPRANSAC_EDGES_RECORD=<file> appends "case d device bound" lines to a file
(profiles/pnpransac_edges/bounds.txt is such a record).
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import pnpransac_cases as PC
from conftest import load_pkg
from test_pnpransac import _check_gpu

pytestmark = pytest.mark.gpu

CASES = PC.single_cases()
ODO_ERR_ARG, ODO_ERR_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def odo():
    pkg = load_pkg()
    cfg = pkg.default_config(640, 480, 1, nfeatures=1000, iterations=200)
    o = pkg.Odometry(cfg)
    yield o
    o.close()


def _record(line):
    path = os.environ.get("PNPRANSAC_EDGES_RECORD")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", list(CASES))
def test_single_case(odo, name):
    c = CASES[name]
    ref, res = _check_gpu(odo, c.Xw, c.uv, O.fr1_calib(), c.iterations, c.reproj, c.conf)
    if "ok" in c.prop:
        assert res.ok == c.prop["ok"]
    if "n_inliers" in c.prop:
        assert res.n_inliers == c.prop["n_inliers"]
    if ref["ok"] != 1:
        return
    ref = PC.reference(c)  # + the float64 minimum on the (equal) inlier set
    rt = np.r_[res.rvec[:], res.tvec[:]]
    dist, bound = float(np.abs(rt - ref["rt64"]).max()), PC.bound64(ref)
    _record(f"{name:24s} d {ref['d']:.3e}  device {dist:.3e}  bound {bound:.3e}")
    assert dist <= bound


# ---------------------------------------------------------------------- batches
def _result_bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _check_batch(odo, probs, iterations=500, reproj=3.0, conf=0.85):
    """Every problem of the batch against the oracle and the one-problem call."""
    cal = O.fr1_calib()
    res, masks = odo.pnp_ransac_batch(probs, None, iterations, reproj, conf)
    assert len(res) == len(probs)
    for p, ((Xw, uv), r, m) in enumerate(zip(probs, res, masks)):
        ref = O.pnp_ransac(Xw, uv, cal, iterations, reproj, conf)
        one, mask1, _ = odo.pnp_ransac(Xw, uv, None, iterations, reproj, conf)
        assert r.ok == ref["ok"] == one.ok, p
        if len(Xw) < 10:  # skipped: pnpransac.cpp:30
            assert (r.ok, r.best_iter, r.n_inliers, r.iterations_visited) == (0, -1, 0, 0), p
            assert not m.any() and len(m) == len(Xw), p
            assert _result_bytes(r) == _result_bytes(one), p
            continue
        assert r.iterations_visited == ref["niters"] == one.iterations_visited, p
        assert r.best_iter == ref["best_iter"] == one.best_iter, p
        assert r.n_inliers == (ref["n_inliers"] if ref["ok"] else 0) == one.n_inliers, p
        np.testing.assert_array_equal(m, mask1)
        assert _result_bytes(r) == _result_bytes(one), p  # Tcw, poses and model, bit for bit
        if not ref["ok"]:
            assert not m.any(), p
            continue
        np.testing.assert_array_equal(m, ref["mask"])
        np.testing.assert_allclose(np.r_[r.model_rvec[:], r.model_tvec[:]], ref["model"], rtol=0, atol=1e-9)
        if ref["ok"] == 1:
            np.testing.assert_allclose(np.r_[r.rvec[:], r.tvec[:]], ref["rt"], rtol=0, atol=1e-7)
    return res, masks


def _fold_probs():
    names = [f"fold_stop_{v}" for v in PC.FOLD_STOPS] + ["fold_round_up", "fold_round_down"]
    return [(CASES[k].Xw, CASES[k].uv) for k in names]


def test_batch_fold_edges(odo):
    """All fold-edge cases in one call: the chunked path (64 hypotheses per
    chunk) stops each problem's fold at 63, 64, 65, 127, 128, 129, 1, 2 ..."""
    res, _ = _check_batch(odo, _fold_probs())
    assert [r.iterations_visited for r in res[:8]] == list(PC.FOLD_STOPS)


@pytest.mark.parametrize("iterations", [1, 63, 64, 65, 129])
def test_batch_iteration_widths(odo, iterations):
    """Three problems whose loops are ended by `iterations`, not by the estimate."""
    big = CASES[f"iterations_{iterations}"]
    probs = [(big.Xw, big.uv), (CASES["points_65"].Xw, CASES["points_65"].uv),
             (CASES["points_257"].Xw, CASES["points_257"].uv)]
    res, _ = _check_batch(odo, probs, iterations, 3.0, 0.999)
    assert res[0].iterations_visited == iterations


@pytest.mark.parametrize("nprob", [63, 64, 65])
def test_batch_problem_count_widths(odo, nprob):
    """One lane per problem in k_pr_subsets / k_pr_fold, 64 lanes per block:
    skipped problems sit at lanes 0, 62, 63, at lane 0 of the second block and last."""
    probs, short = PC.batch_many(nprob)
    assert {0, 62, nprob - 1} <= set(short) and len(probs[0][0]) == 0
    _check_batch(odo, probs)


def test_batch_early_stop_beside_a_full_run(odo):
    """A fold that ends in the first chunk between two that run all 500."""
    names = ["identical_40", "fold_stop_2", "collinear_40", "fold_stop_63", "fold_stop_65"]
    res, _ = _check_batch(odo, [(CASES[k].Xw, CASES[k].uv) for k in names])
    assert [r.iterations_visited for r in res] == [500, 2, 500, 63, 65]


def test_batch_of_nothing(odo):
    res, masks = odo.pnp_ransac_batch([])
    assert res == [] and masks == []


def _batch_bytes(odo, probs):
    res, masks = odo.pnp_ransac_batch(probs)
    return b"".join(_result_bytes(r) for r in res), [m.copy() for m in masks]


def test_batch_is_deterministic_and_the_arena_is_reused(odo):
    small = _fold_probs()[:3]
    large, _ = PC.batch_many(65)
    large = large + _fold_probs()
    s0, sm0 = _batch_bytes(odo, small)
    l0, lm0 = _batch_bytes(odo, large)
    l1, lm1 = _batch_bytes(odo, large)  # twice on one context: identical bytes
    assert l0 == l1 and all(np.array_equal(a, b) for a, b in zip(lm0, lm1))
    s1, sm1 = _batch_bytes(odo, small)  # a small batch after a large one: its own results
    assert s0 == s1 and all(np.array_equal(a, b) for a, b in zip(sm0, sm1))
    _check_batch(odo, small)


# --------------------------------------------------------------------- refusals
class _Raw:
    """The C entry points with pre-filled outputs, to see what a refusal touches."""

    def __init__(self, odo, n, nprob=1):
        self.pkg = load_pkg()
        self.lib, self.h, self.ptr = odo.lib, odo.h, self.pkg._abi.ptr
        self.Xw = np.ones((max(n, 1), 3), np.float32)
        self.uv = np.ones((max(n, 1), 2), np.float32)
        self.res = (self.pkg.PnPRansacResult * max(nprob, 1))()
        C.memset(self.res, 0xA5, C.sizeof(self.res))
        self.mask = np.full(max(n, 1), 0xA5, np.uint8)
        self.good = np.full(8, 0x5A5A5A5A, np.int32)
        self.cal = odo.cfg.calib

    def untouched(self):
        return (C.string_at(self.res, C.sizeof(self.res)) == b"\xa5" * C.sizeof(self.res)
                and (self.mask == 0xA5).all() and (self.good == 0x5A5A5A5A).all())

    def single(self, n, iterations=4, reproj=3.0, conf=0.85, ctx=True, Xw=True, uv=True, res=True):
        p = self.ptr
        return self.lib.odo_pnp_ransac(self.h if ctx else None, p(self.Xw) if Xw else None, p(self.uv) if uv else None,
                                       n, p(self.cal), iterations, reproj, conf,
                                       C.cast(self.res, C.c_void_p) if res else None, p(self.mask),
                                       p(self.good) if iterations <= len(self.good) else None)

    def batch(self, offs, nprob, iterations=4, conf=0.85, ctx=True, Xw=True, res=True, offs_null=False):
        p = self.ptr
        offs = np.ascontiguousarray(offs, np.int32)
        return self.lib.odo_pnp_ransac_batch(self.h if ctx else None, p(self.Xw) if Xw else None, p(self.uv),
                                             None if offs_null else p(offs), nprob, p(self.cal), iterations, 3.0, conf,
                                             C.cast(self.res, C.c_void_p) if res else None, p(self.mask))


@pytest.mark.parametrize("conf", [0.0, 1.0, float("nan"), -0.5, 1.5])
def test_refuses_bad_confidence(odo, conf):
    r = _Raw(odo, 20, 2)
    assert r.single(20, conf=conf) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], 2, conf=conf) == ODO_ERR_ARG and r.untouched()


def test_refuses_bad_sizes_offsets_and_pointers(odo):
    r = _Raw(odo, 20, 2)
    assert r.single(-1) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], -1) == ODO_ERR_ARG and r.untouched()
    assert r.batch([1, 10, 20], 2) == ODO_ERR_ARG and r.untouched()  # offs[0] != 0
    assert r.batch([0, 15, 12], 2) == ODO_ERR_ARG and r.untouched()  # decreasing
    assert r.batch([0, -3, 12], 2) == ODO_ERR_ARG and r.untouched()
    # null pointers
    assert r.single(20, ctx=False) == ODO_ERR_ARG and r.untouched()
    assert r.single(20, Xw=False) == ODO_ERR_ARG and r.untouched()
    assert r.single(20, uv=False) == ODO_ERR_ARG and r.untouched()
    assert r.single(20, res=False) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], 2, ctx=False) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], 2, Xw=False) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], 2, res=False) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0, 10, 20], 2, offs_null=True) == ODO_ERR_ARG and r.untouched()
    assert r.batch([0], 0) == 0 and r.untouched()  # nprob = 0: nothing to do, nothing written
    # the calls above left the context usable
    c = CASES["fold_stop_2"]
    _check_gpu(odo, c.Xw, c.uv, O.fr1_calib())


def test_refuses_what_exceeds_the_capacity(odo):
    r = _Raw(odo, 65600, 65536)  # buffers as large as the calls claim, were one not refused
    assert r.single(65537) == ODO_ERR_CAPACITY and r.untouched()
    assert r.batch([0, 65537], 1) == ODO_ERR_CAPACITY and r.untouched()
    assert r.batch([0, 10, 65547], 2) == ODO_ERR_CAPACITY and r.untouched()
    # iterations x points > 2^28
    assert r.single(257, iterations=1 << 20) == ODO_ERR_CAPACITY and r.untouched()
    assert r.batch([0, 128, 257], 2, iterations=1 << 20) == ODO_ERR_CAPACITY and r.untouched()
    # 65536 problems (empty ones: the count alone is refused)
    assert r.batch(np.zeros(65537, np.int32), 65536) == ODO_ERR_CAPACITY and r.untouched()


def test_python_wrapper_raises_on_refusal(odo):
    c = CASES["fold_stop_2"]
    for conf in (0.0, 1.0, float("nan")):
        with pytest.raises(RuntimeError):
            odo.pnp_ransac(c.Xw, c.uv, None, 500, 3.0, conf)
        with pytest.raises(RuntimeError):
            odo.pnp_ransac_batch([(c.Xw, c.uv)] * 2, None, 500, 3.0, conf)
