"""Time of StatisticalOutlierRemoval and of GICP's fitness score over a batch
(odo_dense_sor, odo_gicp_dense_fitness on the clouds odo_dense_clouds left in
HBM), one JSON line.

--batch frames of the closed-loop synthetic sequence (--seq-len distinct
frames, repeated) lie in HBM as odo_track_batch's inputs do, as in
tools/cloud_bench.py; odo_dense_clouds filters them at --leaf.

sor50_ms / sor20_ms   one odo_dense_sor(50, 1.0) / odo_dense_sor(20, 1.0) call on
             fresh clouds (odo_dense_clouds runs again before every call, untimed)
fitness_ms   odo_gicp_dense_fitness on the batch - 1 consecutive pairs, identity
cov_host_ms  the yardstick: odo_gicp_grid_covariances (the same ring walk for 20
             neighbours with indices) on the same clouds copied to the host, and
sor20_host_ms  odo_cloud_sor_batch(20, 1.0) on those host clouds in the same
             process: both include their transfers (the covariances download
             72 bytes per point, SOR 5), so sor20_host_over_cov_host bounds the
             searches' ratio from below; the kernels' own ratio is in the
             kernel trace (k_sor_dist against k_gicp_cov_grid)

Each form gets a warm-up (the first call allocates the scratch), then --reps
calls timed with a host clock; every call returns with its results downloaded
and the stream idle. No GPU: it fails.

    python tools/sor_bench.py --out profiles/dense_sor/bench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/sor_bench.py --reps 1
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


def timed(fn, reps, before=None):
    """Mean seconds of fn over reps calls after one warm-up; before() runs untimed ahead of every call."""
    total, out = 0.0, None
    for r in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        if r:
            total += time.perf_counter() - t0
    return total / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=64)
    ap.add_argument("--leaf", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sor_bench: no GPU (there is no CPU fallback)")
    pkg, synth = bench.load_pkg(), bench.load_synth()
    W, H, B = 640, 480, args.batch
    L = min(args.seq_len, B)
    bgr, dep, _ = synth.make_sequence(L, W, H, seed=bench.shard_seed(0), closed_loop=True)
    idx = np.arange(B) % L
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[idx])).to("cuda")
    d_dep = torch.from_numpy(np.ascontiguousarray(dep[idx]).view(np.int16)).to("cuda")
    odo = pkg.Odometry(pkg.default_config(W, H, B, nfeatures=2000, iterations=50), device=0)
    torch.cuda.synchronize()
    fresh = lambda: odo.dense_clouds(d_bgr.data_ptr(), d_dep.data_ptr(), B, args.leaf)
    info = fresh()
    pairs = [(i, i + 1) for i in range(B - 1)]
    out = {"tool": "sor_bench", "batch": B, "seq_len": L, "leaf": args.leaf, "reps": args.reps,
           "n_points_mean": round(float(info["n_points"].mean()), 1), "n_points_max": int(info["n_points"].max())}
    dt, fit = timed(lambda: odo.gicp_dense_fitness(pairs), args.reps)
    out.update(fitness_ms=round(dt * 1e3, 3), fitness_pairs=len(pairs), fitness_mean=float(np.mean(fit)))
    clouds = [odo.get_dense_cloud(i) for i in range(B)]
    xyz = [np.ascontiguousarray(np.stack([c["x"], c["y"], c["z"]], 1)) for c in clouds]
    dt_c, _ = timed(lambda: odo.gicp_grid_covariances(xyz), args.reps)
    dt_h, host = timed(lambda: odo.cloud_sor_batch(xyz, 20, 1.0), args.reps)
    out.update(cov_host_ms=round(dt_c * 1e3, 3), sor20_host_ms=round(dt_h * 1e3, 3),
               sor20_host_over_cov_host=round(dt_h / dt_c, 2))
    for k in (50, 20):
        dt, si = timed(lambda: odo.dense_sor(k, 1.0), args.reps, before=fresh)
        out[f"sor{k}_ms"] = round(dt * 1e3, 3)
        out[f"sor{k}_removed_share"] = round(1.0 - float(si["n_out"].sum()) / float(si["n_in"].sum()), 4)
        if k == 20:
            out["dense_equals_host"] = bool(np.array_equal(si["n_out"], host[2]["n_out"]))
    out["sor20_over_cov_host"] = round(out["sor20_ms"] / out["cov_host_ms"], 2)
    s = json.dumps(out)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")
    odo.close()


if __name__ == "__main__":
    main()
