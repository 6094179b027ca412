"""Throughput of the batched path's three Odometry::Compute back-ends
(odo_set_odometry: ADAPTIVE_RBA, RANSAC, ADAPTIVE_RICP) on the same frames.

Batches of 256 frames at 640x480 / 2000 keypoints with the inputs in HBM, the
bench's default workload and its hard one; one context per workload, the modes
measured in turn and the turn repeated (--reps), each measurement a warm-up,
then --steps queued batches and one synchronise. One JSON line per
measurement (stdout, and appended to --out): frames/s, ms per step, and for
ADAPTIVE_RICP the share of pairs per branch and the cloud sizes.

    python tools/ricp_bench.py --out profiles/r08_ricp/bench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/ricp_bench.py --workloads hard --modes ricp --reps 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MODES = {"rba": 0, "ransac": 1, "ricp": 2}


def branch_shares(odo, n):
    q = [odo.ricp(i) for i in range(n)]
    br = np.array([x["branch"] for x in q])
    nc = np.array([x["n_cloud"] for x in q])
    ran = (br != 0) & (nc >= 20)
    return {"branch0": round(float((br == 0).mean()), 4), "branch1": round(float((br == 1).mean()), 4),
            "branch2": round(float((br == 2).mean()), 4), "gicp_ran": round(float(ran.mean()), 4),
            "gicp_converged": round(float(np.mean([x["converged"] for x in q])), 4),
            "mean_cloud_of_ran": round(float(nc[ran].mean()), 1) if ran.any() else 0.0,
            "max_cloud": int(nc.max()),
            "mean_gicp_iterations_of_ran": round(float(np.mean([x["iterations"] for x, r in zip(q, ran) if r])), 2)
            if ran.any() else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--seq-len", type=int, default=64)
    ap.add_argument("--workloads", default="default,hard")
    ap.add_argument("--modes", default="rba,ransac,ricp")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    pkg, synth = bench.load_pkg(), bench.load_synth()
    W, H, B = 640, 480, args.batch
    out = open(args.out, "a") if args.out else None
    for wl in args.workloads.split(","):
        L = min(args.seq_len, B)
        bgr, dep, _ = synth.make_sequence(L, W, H, seed=bench.shard_seed(0), closed_loop=True, hard=wl == "hard")
        idx = np.arange(B) % L
        d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[idx])).to("cuda")
        d_dep = torch.from_numpy(np.ascontiguousarray(dep[idx]).view(np.int16)).to("cuda")
        cfg = pkg.default_config(W, H, B, nfeatures=args.nfeatures, iterations=args.iters, seed=bench.rank_seeds(0)[1])
        odo = pkg.Odometry(cfg, device=0)
        torch.cuda.synchronize()
        step = lambda want=False: odo.track_batch(d_bgr.data_ptr(), d_dep.data_ptr(), B, want_results=want)
        for rep in range(args.reps):
            for name in args.modes.split(","):
                odo.set_odometry(MODES[name])
                for _ in range(args.warmup):
                    step()
                res = step(True)
                shares = branch_shares(odo, B) if name == "ricp" else None
                odo.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                odo.synchronize()
                dt = time.perf_counter() - t0
                line = {"workload": wl, "mode": name, "rep": rep, "batch": B, "steps": args.steps,
                        "frames_per_s": round(B * args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 4),
                        "mean_matches": round(float(np.mean(res["n_matches"])), 1),
                        "mean_inliers": round(float(np.mean(res["n_inliers"])), 1),
                        "mean_flags": round(float(np.mean(res["pnp_inliers"])), 1)}
                if shares:
                    line["ricp"] = shares
                s = json.dumps(line)
                print(s, flush=True)
                if out:
                    out.write(s + "\n")
                    out.flush()
        odo.close()
        del d_bgr, d_dep


if __name__ == "__main__":
    main()
