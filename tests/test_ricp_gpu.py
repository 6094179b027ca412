"""GPU parity of the batched ADAPTIVE_RICP / RANSAC odometry modes
(odo_set_odometry) against the reference composition of ricp_ref (CPU oracle):
stage by stage on a crafted sequence that takes every branch of
odometry.cpp:52-68, across batch splits, entry points, parameters and mode
switches.

Tolerances: RANSAC, the decision, the clouds, the GICP counters, the fallback
poses and the inlier flags are exact (bit patterns / integers). A converged
GICP pose is held to 1e-5 of the oracle's, the bar tests/test_gicp.py holds
odo_gicp to against the same oracle on the same kind of cloud; the clouds fed
to it here are bit-equal to the oracle's, so nothing else enters. Against
odo_gicp on the read-back clouds the batched GICP is bit-equal (same kernels).
"""
import numpy as np
import pytest

import oracle_lib as O
import ricp_ref as RR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

# The seed base under which the batched contract's per-pair seeds
# (pair_seed(SEED, i)) give the crafted sequence the outcome table that the CPU
# test asserts for the oracle seeds 1234 + i (checked on the reference below).
SEED = 0x5EED0031
PAIRS2 = [(a, a + 2) for a in range(0, RR.N_FRAMES, 2)]
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def world():
    """Frames, the oracle's RANSAC pass and the default-constant reference:
    computed once, read-only."""
    pkg = load_pkg()
    cal = O.fr1_calib()
    bgr, dep = RR.crafted_sequence()
    frames = RR.extract_frames(bgr, dep, cal)
    rp = O.ransac_params()
    passes = RR.ransac_pass(frames, cal, rp, lambda i: pkg.pair_seed(SEED, i))
    ref = RR.compose(frames, passes, rp)
    kinds = {i: RR.kind(e) for i, e in ref.items()}
    assert kinds == {1: "keep", 2: "refine", 3: "refine", 4: "reset_empty", 5: "reset_empty", 6: "refine",
                     7: "reset_gicp", 8: "reset_gicp", 9: "refine", 10: "reset_empty", 11: "reset_empty"}, kinds
    return dict(pkg=pkg, cal=cal, bgr=bgr, dep=dep, frames=frames, rp=rp, passes=passes, ref=ref)


def make_odo(pkg, max_batch):
    cfg = pkg.default_config(RR.W, RR.H, max_batch, nfeatures=RR.NFEAT, iterations=200, seed=SEED)
    return pkg.Odometry(cfg)


def collect(odo, res, a, mode):
    """Everything the last batch (frames a ..) reports, keyed by frame index."""
    out = {}
    for k in range(len(res)):
        e = dict(res=res[k].copy(), pair=odo.pair(k))
        if mode == 2:
            e["ricp"] = odo.ricp(k)
        out[a + k] = e
    return out


def run(w, cuts, mode, odo=None, how="device", **params):
    """The 12 frames in the given batches through one context in `mode`
    (a list: one mode per batch). Returns ({frame: report}, [latch per batch])."""
    import torch
    pkg = w["pkg"]
    modes = mode if isinstance(mode, list) else [mode] * len(cuts)
    own = odo is None
    if own:
        odo = make_odo(pkg, max(b - a for a, b in cuts))
    got, latches = {}, []
    cur = None
    for (a, b), m in zip(cuts, modes):
        if m != cur:
            odo.set_odometry(m, **(params if m == 2 else {}))
            cur = m
        assert odo.odometry_mode() == m
        if how == "host":
            res = odo.track_batch_host(w["bgr"][a:b], w["dep"][a:b])
        else:
            tb = torch.from_numpy(w["bgr"][a:b]).to("cuda")
            td = torch.from_numpy(w["dep"][a:b].view(np.int16)).to("cuda")
            torch.cuda.synchronize()
            res = odo.track_batch(tb.data_ptr(), td.data_ptr(), b - a)
        got.update(collect(odo, res, a, m))
        latches.append(odo.latch)
    if own:
        odo.close()
    return got, latches


def check_ransac(g, e, n2, tag):
    """The RANSAC fields and the inlier flags of one pair against the oracle."""
    r, res, pair = e["res"], g["res"], g["pair"]
    assert np.array_equal(pair["matches"], e["matches"]), f"{tag}: match list differs"
    got = dict(T12=res["T12"], rmse=res["rmse"], ok=res["ransac_ok"],
               inliers=pair["good"][pair["ransac_inliers"].astype(bool)])
    O.assert_ransac_bits(got, dict(T12=r.T12, rmse=r.rmse, ok=r.ransac_ok, inliers=r.inliers), tag)
    O.check_ransac_inliers(pair, r, tag)
    assert (res["n_matches"], res["n_good"], res["n_inliers"], res["visited"], res["n_sweeps"],
            res["n_fit_points"]) == (r.n_matches, r.n_good, r.n_inliers, r.visited, r.n_sweeps, r.n_fit_points), tag
    flags = pair["pnp_inliers"]
    assert np.array_equal(flags[:n2], e["flags"]), f"{tag}: inlier flags differ"
    assert not flags[n2:].any() and int(res["pnp_inliers"]) == int(e["flags"].sum()), f"{tag}: flag count"


def check_ricp(g, e, tag):
    """Decision, clouds, GICP counters and Tcw of one pair against the reference."""
    q, res = g["ricp"], g["res"]
    print(f"{tag}: branch {q['branch']} cloud {q['n_cloud']} conv {q['converged']} it {q['iterations']} "
          f"corr {q['n_corr']} | ref {e['branch']} {len(e['src'])} {e['converged']} {e['iterations']} {e['n_corr']}")
    assert q["branch"] == e["branch"], f"{tag}: branch {q['branch']} vs {e['branch']}"
    assert q["n_cloud"] == len(e["src"]) == len(e["tgt"]), f"{tag}: n_cloud {q['n_cloud']} vs {len(e['src'])}"
    O.assert_same_bits(q["src"], e["src"], f"{tag}: source cloud")
    O.assert_same_bits(q["tgt"], e["tgt"], f"{tag}: target cloud")
    assert (q["converged"], q["iterations"], q["n_corr"]) == (e["converged"], e["iterations"], e["n_corr"]), \
        f"{tag}: GICP converged / iterations / n_corr"
    Tcw = res["Tcw"].reshape(4, 4)
    if e["branch"] == 0 or (e["branch"] == 2 and not e["converged"]):
        O.assert_same_bits(Tcw, res["T12"], f"{tag}: Tcw is RANSAC's T12")
        O.assert_same_bits(Tcw, e["T_ransac"], f"{tag}: Tcw is the oracle's RANSAC T12")
    elif e["branch"] == 1 and not e["converged"]:
        O.assert_same_bits(Tcw, EYE, f"{tag}: Tcw is the identity")
    else:
        d = float(np.abs(Tcw - e["Tcw"]).max())
        print(f"{tag}: |Tcw - reference| max {d:.3g}")
        assert d < 1e-5, f"{tag}: Tcw differs from the reference composition by {d}"
        O.assert_same_bits(Tcw, q["T12"], f"{tag}: Tcw is the record's GICP T12")
    if not e["converged"]:
        O.assert_same_bits(q["T12"], EYE, f"{tag}: GICP T12 of a pair it did not converge on")


def check_all(w, got, ref, tag):
    assert sorted(got) == list(range(RR.N_FRAMES))
    for i in range(1, RR.N_FRAMES):
        check_ransac(got[i], ref[i], len(w["frames"][i]["kps"]), f"{tag} pair {i}")
        check_ricp(got[i], ref[i], f"{tag} pair {i}")


def same_reports(a, b, tag, ricp=True):
    """Two runs' reports of the same frames, bit for bit."""
    for i in sorted(a):
        assert a[i]["res"].tobytes() == b[i]["res"].tobytes(), f"{tag}: pair {i} record differs"
        for k in ("matches", "good", "ransac_inliers", "pnp_inliers", "f2_src"):
            assert np.array_equal(a[i]["pair"][k], b[i]["pair"][k]), f"{tag}: pair {i} {k} differs"
        if ricp:
            for k, v in a[i]["ricp"].items():
                O.assert_same_bits(v, b[i]["ricp"][k], f"{tag}: pair {i} ricp {k}",
                                   np.float32 if isinstance(v, np.ndarray) else np.int32)


@pytest.fixture(scope="module")
def case1(world):
    """max_batch = 2, six batches: every frame set is reused, both pair
    streams (and both copies of the GICP scratch) alternate."""
    return run(world, PAIRS2, 2)


def test_parity_stage_by_stage(world, case1):
    w = world
    got, latches = case1
    check_all(w, got, w["ref"], "b2")
    assert latches[-1] == w["passes"][RR.N_FRAMES - 1][2]
    # a pair without a predecessor reports what the default mode reports
    first = got[0]
    assert first["res"]["n_matches"] == 0 and first["res"]["pnp_inliers"] == 0 and first["ricp"]["n_cloud"] == 0
    O.assert_same_bits(first["res"]["Tcw"], EYE, "frame 0: Tcw")
    assert not first["pair"]["pnp_inliers"].any()
    # wherever GICP ran: bit-equal to odo_gicp on the read-back clouds
    odo = make_odo(w["pkg"], 1)
    ran = 0
    for i in range(1, RR.N_FRAMES):
        q = got[i]["ricp"]
        if q["branch"] == 0 or q["n_cloud"] < 20:
            continue
        guess = EYE if q["branch"] == 1 else got[i]["res"]["T12"].reshape(4, 4)
        T, conv, it, nc = odo.gicp(q["src"], q["tgt"], guess)
        O.assert_same_bits(q["T12"], T, f"pair {i}: batched GICP T12 vs odo_gicp")
        assert (q["converged"], q["iterations"], q["n_corr"]) == (conv, it, nc), f"pair {i}: vs odo_gicp"
        ran += 1
    odo.close()
    assert ran == 6


def test_batching_independence(world, case1):
    w = world
    one, _ = run(w, [(0, 12)], 2)
    same_reports(case1[0], one, "one batch of 12 vs batches of 2")
    split, _ = run(w, [(0, 5), (5, 10), (10, 12)], 2)
    same_reports(case1[0], split, "5 + 5 + 2 vs batches of 2")
    host, _ = run(w, PAIRS2, 2, how="host")
    same_reports(case1[0], host, "track_batch_host vs device inputs")


def test_pipelined_async_batches(world, case1):
    """Six batches queued without a host sync, the records streamed to pinned
    memory: two batches in flight share nothing of the new scratch."""
    import torch
    w = world
    pkg = w["pkg"]
    odo = make_odo(pkg, 2)
    odo.set_odometry(pkg.ODOMETRY_ADAPTIVE_RICP)
    ring = pkg.PinnedResults(len(PAIRS2), 2)
    dev = [(torch.from_numpy(w["bgr"][a:b]).to("cuda"), torch.from_numpy(w["dep"][a:b].view(np.int16)).to("cuda"))
           for a, b in PAIRS2]
    torch.cuda.synchronize()
    for k, (tb, td) in enumerate(dev):
        odo.track_batch_async(tb.data_ptr(), td.data_ptr(), 2, ring, k)
    odo.synchronize()
    for k, (a, b) in enumerate(PAIRS2):
        for j in range(2):
            assert ring.all[k][j].tobytes() == case1[0][a + j]["res"].tobytes(), f"async record of frame {a + j}"
    last = collect(odo, ring.all[len(PAIRS2) - 1], PAIRS2[-1][0], 2)
    same_reports(last, case1[0], "async last batch")
    ring.close()
    odo.close()


def test_parameters(world):
    w = world
    pkg = w["pkg"]
    r1 = w["passes"][1][0]
    at = float(np.float32(r1.rmse) * np.float32(10))
    odo = make_odo(pkg, 2)
    for params in (dict(reset_at=8.0), dict(refine_at=at), dict(min_inliers=60), dict(gicp_max_corr_dist=1e-4),
                   dict(gicp_iterations=1)):
        ref = RR.compose(w["frames"], w["passes"], w["rp"], **params)
        # conditions on the inputs: each variant moves what it is meant to move
        if "reset_at" in params:
            assert all(ref[i]["branch"] == 1 and len(ref[i]["src"]) >= 20 for i in (2, 3, 9)) and ref[6]["branch"] == 2
        if "refine_at" in params:
            assert w["ref"][1]["branch"] == 0 and ref[1]["branch"] == 2
        if "min_inliers" in params:
            assert ref[1]["branch"] == 2 and ref[1]["res"].n_inliers >= 20
        if "gicp_max_corr_dist" in params:
            assert not any(e["converged"] for e in ref.values())
            assert {e["branch"] for e in ref.values() if len(e["src"]) >= 20} == {1, 2}
        if "gicp_iterations" in params:
            assert all(e["iterations"] == 1 for e in ref.values() if e["converged"])
        odo.reset()
        got, _ = run(w, PAIRS2, 2, odo=odo, **params)
        check_all(w, got, ref, str(params))
    odo.close()


def test_ransac_mode(world):
    w = world
    pkg = w["pkg"]
    ref = RR.compose(w["frames"], w["passes"], w["rp"], mode="ransac")
    odo = make_odo(pkg, 2)
    got, _ = run(w, PAIRS2, pkg.ODOMETRY_RANSAC, odo=odo)
    for i in range(1, RR.N_FRAMES):
        check_ransac(got[i], ref[i], len(w["frames"][i]["kps"]), f"ransac pair {i}")
        O.assert_same_bits(got[i]["res"]["Tcw"], got[i]["res"]["T12"], f"ransac pair {i}: Tcw")
    r = pkg.RicpResult()
    assert odo.lib.odo_get_ricp(odo.h, 0, pkg.ptr(r), None, None, 0) == pkg._abi.ERR_STATE
    assert odo.lib.odo_last_error()
    odo.close()


def test_mode_switches_keep_the_sequence(world, case1):
    w = world
    rba, lat_rba = run(w, PAIRS2, 0)
    modes = [0, 2, 0, 2, 0, 0]
    mixed, lat_mixed = run(w, PAIRS2, modes)
    for (a, b), m in zip(PAIRS2, modes):
        sub = {i: mixed[i] for i in range(a, b)}
        if m == 0:
            same_reports(sub, rba, f"RBA batch {a}", ricp=False)
        else:
            same_reports(sub, case1[0], f"RICP batch {a}")
    for k in range(len(PAIRS2)):
        O.assert_same_bits(lat_mixed[k], lat_rba[k], f"latch after batch {k} (vs all RBA)", np.float64)
        O.assert_same_bits(lat_mixed[k], case1[1][k], f"latch after batch {k} (vs all RICP)", np.float64)


def test_default_mode_is_untouched(world):
    w = world
    pkg = w["pkg"]
    odo = make_odo(pkg, 2)
    assert odo.odometry_mode() == pkg.ODOMETRY_ADAPTIVE_RBA == 0
    r = pkg.RicpResult()
    assert odo.lib.odo_get_ricp(odo.h, 0, pkg.ptr(r), None, None, 0) == pkg._abi.ERR_STATE
    odo.track_batch_host(w["bgr"][:2], w["dep"][:2])
    assert odo.lib.odo_get_ricp(odo.h, 0, pkg.ptr(r), None, None, 0) == pkg._abi.ERR_STATE
    assert odo.odometry_mode() == 0
    # the argument checks that need a context
    assert odo.lib.odo_set_odometry(odo.h, 5, None) == pkg._abi.ERR_ARG
    p = pkg.default_ricp_params()
    p.gicp_iterations = 0
    assert odo.lib.odo_set_odometry(odo.h, pkg.ODOMETRY_ADAPTIVE_RICP, pkg.ptr(p)) == pkg._abi.ERR_ARG
    assert odo.odometry_mode() == 0
    odo.close()
