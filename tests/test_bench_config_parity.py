"""GPU parity of the configuration bench.py measures.

The bench runs 256-frame batches back to back on device-resident inputs with
the default schedule (two pair streams taking alternate batches, four frame
sets in flight, the occupancy-sized kNN-2 grid whose workgroups take several
(pair, query block, train split) items, the RANSAC work list). Here the same
setup runs six consecutive batches, so every frame set is reused and both pair
streams alternate, and all pairs of the last batch are compared with the CPU
oracle (Tracking::Track order: tracking.cpp:193-208; Ransac::Iterate
ransac.cpp:155-267; PnPSolver::Compute pnpsolver.cpp:17-214):

* every frame's keypoints, descriptors, kun, xyz, uR: bit-exact;
* every pair's match list, n_queries, n_good, visited, n_inliers, ok, T12, rmse,
  RANSAC inlier list (Ransac::mvInliers entry for entry), RANSAC work (sweeps, fit points): bit-exact; the
  DepthCovariance latch: exact;
* PnP pose within 1e-4; PnP inlier flags equal except on edges whose chi2 at
  the oracle's pose lies within 2 % of the threshold (5.991 mono, 7.815 stereo).

cfg2_hard_b64 runs the hard workload (synth.make_sequence(hard=True): image and
depth noise, two moving cuboids, repeated texture, twice the motion), where
the inlier ratio is ~64 % and RANSAC visits ~450 of its 500 hypotheses.

cfg2 also runs with both kNN-2 kernel forms and VALU train splits 1, 2 and 8 (match lists and query counts
bit-exact each time): 256 pairs give more active kNN-2 items than resident
workgroups, so runs covering several items, split flushes and query-block
switches inside one workgroup are all exercised. cfg4 (ICL, fy < 0) runs at
B = 256 and cfg5 (1280x960, 8000 kp, H = 8192) at B = 32.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
from conftest import load_pkg, sequence

pytestmark = pytest.mark.gpu

FR1 = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)
ICL = dict(fx=481.2, fy=-480.0, cx=319.5, cy=239.5)
NODIST = dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
BATCHES = 6
THREADS = 16  # the box's CPU share; ctypes releases the GIL inside the oracle

CONFIGS = {
    # bench.py defaults: cfg2, 64-frame closed loop cycled through 256-frame batches
    "cfg2_bench": dict(w=640, h=480, nf=2000, iters=500, B=256, L=64, intr=None, calib=None,
                       scene=0x5EED0002, seed=0x5EED0000),
    "cfg4_icl_b256": dict(w=640, h=480, nf=2000, iters=500, B=256, L=64, intr=ICL, calib=dict(ICL, **NODIST),
                          scene=0x5EED0004, seed=0x5EED0004),
    "cfg5_1280_b32": dict(w=1280, h=960, nf=8000, iters=8192, B=32, L=32, intr=FR1,
                          calib=dict(fx=2 * FR1["fx"], fy=2 * FR1["fy"], cx=2 * FR1["cx"], cy=2 * FR1["cy"],
                                     **NODIST), scene=0x5EED0005, seed=0x5EED0005),
    # the hard workload (bench.py's hard_workload leg): noise, movers, repeated
    # texture, 2x motion; RANSAC visits ~450 of 500 hypotheses per pair
    "cfg2_hard_b64": dict(w=640, h=480, nf=2000, iters=500, B=64, L=64, intr=None, calib=None,
                          scene=0x5EED0002, seed=0x5EED0000, hard=True),
}


def _oracle_calib(cfg):
    k = cfg.calib
    return O.Calib(k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, k.k3, k.depth_factor, k.mbf, k.th_depth)


def _pos(c, b, i):
    """Loop position of frame i of batch b: batch b starts b (B + 1) frames
    into the cycled loop, so no two of the BATCHES batches hold the same frames
    (a batch reading a frame set's data from before its own extraction -- a
    broken cross-stream dependency -- would read other frames), and pair 0 of
    batch b pairs positions b (B + 1) - 2 and b (B + 1)."""
    return (b * (c["B"] + 1) + i) % c["L"]


def _nb(c):
    return c.get("batches", BATCHES)


def _run_gpu(pkg, c, bgr, dep, forms=None):
    """bench.py's timed loop: device-resident batches, _nb(c) back-to-back
    calls without a host sync (batch b's frames at _pos(c, b, .)), except
    one after batch c["sync_after"] when the config names it.
    forms: odo_kernel_forms fields (bit-identical kernel alternatives)."""
    import torch
    B, L, NB = c["B"], c["L"], _nb(c)
    idx = torch.from_numpy(np.arange(NB * (B + 1)) % L).to("cuda")
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr)).to("cuda")[idx].contiguous()
    d_dep = torch.from_numpy(np.ascontiguousarray(dep).view(np.int16)).to("cuda")[idx].contiguous()
    fb, fd = d_bgr[0].numel(), 2 * d_dep[0].numel()  # bytes per frame
    cfg = pkg.default_config(c["w"], c["h"], B, nfeatures=c["nf"], iterations=c["iters"], seed=c["seed"],
                             calib=c["calib"], forms=forms)
    odo = pkg.Odometry(cfg)
    torch.cuda.synchronize()
    for b in range(NB):
        o = b * (B + 1)
        last = b == NB - 1
        res = odo.track_batch(d_bgr.data_ptr() + o * fb, d_dep.data_ptr() + o * fd, B, want_results=last)
        if b == c.get("sync_after", -1):
            odo.synchronize()
    odo.synchronize()
    del d_bgr, d_dep
    return odo, cfg, res


def _pair_frames(c, frames, p):
    """(F1, F2) of pair p of the last batch."""
    b = _nb(c) - 1
    f2 = frames[_pos(c, b, p)]
    f1 = frames[_pos(c, b, p - 1)] if p > 0 else frames[(b * (c["B"] + 1) - 2) % c["L"]]
    return f1, f2


def _oracle_run(pkg, c, cfg, bgr, dep):
    cal = _oracle_calib(cfg)
    op = O.orb_params(c["nf"])
    L, B = c["L"], c["B"]
    with ThreadPoolExecutor(THREADS) as ex:
        frames = list(ex.map(lambda i: O.extract_frame(bgr[i], dep[i], op, cal), range(L)))
    rp = O.ransac_params(c["iters"])
    # the latch comes from the first valid pair ever: global pair 1 (frames 0, 1)
    latch = float("nan")
    g = 1
    while np.isnan(latch):
        _, _, _, latch = O.track_pair(frames[(g - 1) % L], frames[g % L], cal, rp, pkg.pair_seed(cfg.seed, g), latch)
        g += 1
    g0 = (_nb(c) - 1) * B

    def pair(p):
        f1, f2 = _pair_frames(c, frames, p)
        return O.track_pair(f1, f2, cal, rp, pkg.pair_seed(cfg.seed, g0 + p), latch)

    with ThreadPoolExecutor(THREADS) as ex:
        pairs = list(ex.map(pair, range(B)))
    return cal, frames, pairs, latch


_ORACLE = {}


def _oracle_cached(name, pkg, c, cfg, bgr, dep):
    if name not in _ORACLE:
        _ORACLE[name] = _oracle_run(pkg, c, cfg, bgr, dep)
    return _ORACLE[name]


def _compare(name, c, odo, res, oracle, full=True, pnp=True):
    cal, frames, pairs, latch = oracle
    B, L = c["B"], c["L"]
    g0 = (_nb(c) - 1) * B
    if full:
        for i in range(B):
            got, ref = odo.frame(i), frames[_pos(c, _nb(c) - 1, i)]
            assert len(got["kps"]) == len(ref["kps"]), f"{name} frame {i}: N"
            assert np.array_equal(got["kps"], ref["kps"]), f"{name} frame {i}: keypoints"
            assert np.array_equal(got["desc"], ref["desc"]), f"{name} frame {i}: descriptors"
            for f in ("kun", "xyz", "ur"):
                assert np.array_equal(got[f], ref[f]), f"{name} frame {i}: {f}"
    for p in range(B):
        r, mask, matches, _ = pairs[p]
        g = odo.pair(p)
        tag = f"{name} pair {p} (global {g0 + p})"
        assert np.array_equal(g["matches"], matches), f"{tag}: match list"
        assert res[p]["n_queries"] == r.n_queries, f"{tag}: kNN-2 query count"
        if not full:
            continue
        assert (res[p]["n_matches"], res[p]["n_good"], res[p]["visited"], res[p]["n_inliers"],
                res[p]["ransac_ok"]) == (r.n_matches, r.n_good, r.visited, r.n_inliers, r.ransac_ok), \
            f"{tag}: RANSAC counts"
        assert (res[p]["n_sweeps"], res[p]["n_fit_points"]) == (r.n_sweeps, r.n_fit_points), \
            f"{tag}: RANSAC work counts (sweeps, fit points)"
        assert np.array_equal(res[p]["T12"], np.array(r.T12, np.float32)), f"{tag}: T12"
        assert res[p]["rmse"] == np.float32(r.rmse), f"{tag}: rmse"
        O.assert_same_bits(res[p]["T12"], r.T12, f"{tag}: T12")  # a zero's sign included
        O.assert_same_bits(res[p]["rmse"], r.rmse, f"{tag}: rmse")
        O.check_ransac_inliers(g, r, tag)
        if not pnp:
            continue
        Tref = np.array(r.Tcw, np.float32).reshape(4, 4)
        dT = np.abs(res[p]["Tcw"].reshape(4, 4) - Tref).max()
        assert dT < 1e-4, f"{tag}: PnP pose differs by {dT}"
        f1, f2 = _pair_frames(c, frames, p)
        n2 = len(f2["kps"])
        O.check_pnp_flags(g["pnp_inliers"][:n2], mask, f1, f2, g["f2_src"][:n2], Tref, cal, tag)
    assert odo.latch == latch, f"{name}: latch {odo.latch} vs {latch}"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bench_configuration_full_batch(name):
    c = CONFIGS[name]
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True,
                           hard=c.get("hard", False))
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep)
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    r = oracle[2]
    print(f"{name}: B={c['B']} visited mean {np.mean([x[0].visited for x in r]):.1f} max "
          f"{max(x[0].visited for x in r)}, inliers mean {np.mean([x[0].n_inliers for x in r]):.1f}")
    try:
        _compare(name, c, odo, res, oracle)
    finally:
        odo.close()


@pytest.mark.parametrize("form,split", [(1, 1), (1, 2), (1, 8), (0, 0)])
def test_bench_configuration_knn_forms(form, split):
    """Every kNN-2 kernel form (odo_kernel_forms.knn): the VALU xor/popcount
    kernel with train splits 1 / 2 / 8 and more active items than resident
    workgroups, and the FP4 MFMA kernel (the default; its XCD-ordered items and
    min3 / med3 top-2): match lists and query counts of all 256 pairs
    bit-exact."""
    name = "cfg2_bench"
    c = CONFIGS[name]
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True)
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep, forms={"knn": form, "knn_split": split})
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    try:
        _compare(name + f" kNN form {form} split {split}", c, odo, res, oracle, full=False)
    finally:
        odo.close()


@pytest.mark.parametrize("name", ["cfg2_bench", "cfg4_icl_b256"])
def test_bench_configuration_ransac_lanes(name):
    """The second RANSAC launch on the lane-per-hypothesis kernel
    (k_ransac_lanes) whatever the open-pair count (ransac_lanes_min_open = 1: from
    the fifth batch on, a set whose previous batch left a pair open takes it):
    every pair of the last batch bit-exact against the oracle."""
    c = CONFIGS[name]
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True)
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep, forms={"ransac_lanes_min_open": 1})
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    try:
        _compare(name + " lanes", c, odo, res, oracle)
    finally:
        odo.close()


@pytest.mark.parametrize("h0", [1, 3, 5, 8])
def test_bench_configuration_first_ransac_launch(h0):
    """The first RANSAC evaluation launch at other widths
    (odo_kernel_forms.ransac_first_hyps): h0 hypotheses per pair,
    fewer waves per workgroup than rows of four when h0 < 4 and a partly
    filled second row at 5: every pair of the last batch bit-exact (visited
    counts, T12, inlier lists, work counts)."""
    name = "cfg2_bench"
    c = CONFIGS[name]
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True)
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep, forms={"ransac_first_hyps": h0})
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    try:
        _compare(name + f" first launch h0 {h0}", c, odo, res, oracle)
    finally:
        odo.close()


def test_bench_configuration_latched():
    """Two batches, a host sync, then six more without one: from the third
    batch on the DepthCovariance latch is known to be set (k_latch's host flag
    after its event completed) and the batches leave the latch kernel and its
    ordering packets out (odo_batch.cpp run_pairs). Every pair of the last
    batch bit-exact, the latch included."""
    name = "cfg2_latched"
    c = dict(CONFIGS["cfg2_bench"], batches=8, sync_after=1)
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True)
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep)
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    try:
        _compare(name, c, odo, res, oracle)
    finally:
        odo.close()


def test_bench_configuration_ransac_lanes_ieee_form():
    """k_ransac_lanes in its IEEE ErrorFunction2 form. The fast square-root /
    reciprocal form (EF_FAST=2, the default) is chosen per launch only when
    every open pair's points have depths in [2^-20, 2^20] (k_ransac_prep's
    guard); with depth_factor 1e-10 (z = raw * depth_factor; TUM's is
    1 / 5000) the bench scene's depths (raw 4614-17886) become
    4.6e-7-1.8e-6 m, partly below it, so the launch takes the IEEE form.
    Forced onto the lanes kernel as in test_bench_configuration_ransac_lanes:
    every pair's RANSAC result bit-exact (counts, work counts, T12, rmse,
    inlier lists) and the latch exact. PnP is not compared: at these depths
    its stereo terms (u - mbf / z ~ -4e7) leave float resolution, which the
    pose tolerance does not cover, and this test is about RANSAC."""
    name = "cfg2_tiny_depth"
    c = dict(CONFIGS["cfg2_bench"], calib=dict(depth_factor=1e-10))
    pkg = load_pkg()
    bgr, dep, _ = sequence(c["L"], c["w"], c["h"], intrinsics=c["intr"], seed=c["scene"], closed_loop=True)
    odo, cfg, res = _run_gpu(pkg, c, bgr, dep, forms={"ransac_lanes_min_open": 1})
    oracle = _oracle_cached(name, pkg, c, cfg, bgr, dep)
    try:
        for i in range(c["B"]):
            z = odo.frame(i)["xyz"].reshape(-1, 3)[:, 2]
            z = z[np.isfinite(z) & (z > 0)]
            assert z.size and (z < 2.0 ** -20).mean() > 0.05, f"frame {i}: depths not below the fast-form guard"
        _compare(name + " lanes IEEE form", c, odo, res, oracle, pnp=False)
    finally:
        odo.close()
