"""Time of the point-to-plane ICP over a batch (odo_icp_plane_dense and
odo_icp_plane_batch: libicp's IcpPointToPlane), one JSON line per form, in one
job with odo_gicp_dense on the same pairs.

--batch frames of the closed-loop synthetic sequence (--seq-len distinct
frames, repeated) lie in HBM as odo_track_batch's inputs do; odo_dense_clouds
filters them at --leaf once (tools/gicp_dense_bench.py's clouds).

dense_reference  odo_icp_plane_dense on the batch - 1 consecutive pairs at the
                 reference's settings (Tests/IcpPointToPlane.cpp: 15 neighbours,
                 50 iterations, min_delta 1e-8, indist 0.01)
dense_defaults   the same at libicp's defaults (10, 200, 1e-4, every point active)
gicp_dense       odo_gicp_dense(15, 0.05) on the same pairs
sparse           odo_icp_plane_batch on --batch pairs of --sparse-points points
                 (RANSAC's inlier clouds are a few hundred points) sampled from
                 consecutive clouds, at the reference's settings, next to
                 odo_gicp_batch(10, 0.07) on the same pairs (sparse_gicp)

Each form gets a warm-up (the first call allocates the scratch), then --reps
calls timed with a host clock; every call returns with its results downloaded
and the stream idle. No GPU: it fails.

    python tools/icp_bench.py --out profiles/icp_dense/bench.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/icp_bench.py --reps 2 --only dense_reference
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


def timed(fn, reps):
    fn()  # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=64)
    ap.add_argument("--leaf", type=float, default=0.03)
    ap.add_argument("--sparse-points", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one form alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: no GPU (there is no CPU fallback)")
    pkg, synth = bench.load_pkg(), bench.load_synth()
    W, H, B = 640, 480, args.batch
    L = min(args.seq_len, B)
    bgr, dep, _ = synth.make_sequence(L, W, H, seed=bench.shard_seed(0), closed_loop=True)
    idx = np.arange(B) % L
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[idx])).to("cuda")
    d_dep = torch.from_numpy(np.ascontiguousarray(dep[idx]).view(np.int16)).to("cuda")
    odo = pkg.Odometry(pkg.default_config(W, H, B, nfeatures=2000, iterations=50), device=0)
    torch.cuda.synchronize()
    info = odo.dense_clouds(d_bgr.data_ptr(), d_dep.data_ptr(), B, args.leaf)
    pairs = [(i, i + 1) for i in range(B - 1)]
    reference = pkg.icp_params(num_neighbors=15, max_iterations=50, min_delta=1e-8, indist=0.01)
    base = {"tool": "icp_bench", "batch": B, "seq_len": L, "leaf": args.leaf, "reps": args.reps,
            "n_points_mean": round(float(info["n_points"].mean()), 1), "n_points_max": int(info["n_points"].max())}
    lines = []

    def icp_line(form, dt, res, n, prm):
        return {**base, "form": form, "pairs": n, "call_ms": round(dt * 1e3, 3), "pairs_per_s": round(n / dt, 1),
                "num_neighbors": prm.num_neighbors, "max_iterations": prm.max_iterations, "min_delta": prm.min_delta,
                "indist": prm.indist, "iterations_mean": round(float(res["iterations"].mean()), 2),
                "iterations_max": int(res["iterations"].max()), "n_active_mean": round(float(res["n_active"].mean()), 1),
                "singular": int((res["status"] == pkg.ICP_SINGULAR).sum())}

    want = lambda form: args.only in (None, form)
    if want("dense_reference"):
        dt, res = timed(lambda: odo.icp_plane_dense(pairs, None, reference), args.reps)
        lines.append(icp_line("dense_reference", dt, res, len(pairs), reference))
    if want("dense_defaults"):
        prm = pkg.icp_params()
        dt, res = timed(lambda: odo.icp_plane_dense(pairs, None, prm), args.reps)
        lines.append(icp_line("dense_defaults", dt, res, len(pairs), prm))
    if want("gicp_dense"):
        dt, res = timed(lambda: odo.gicp_dense(pairs, None, 15, 0.05), args.reps)
        lines.append({**base, "form": "gicp_dense", "pairs": len(pairs), "call_ms": round(dt * 1e3, 3),
                      "pairs_per_s": round(len(pairs) / dt, 1), "converged": int(sum(r[1] for r in res)),
                      "iterations_mean": round(float(np.mean([r[2] for r in res])), 2)})
    if want("sparse") or want("sparse_gicp"):
        rng = np.random.default_rng(7)
        xyz = []
        for i in range(min(B, L + 1)):
            c = odo.get_dense_cloud(i)
            p = np.stack([c["x"], c["y"], c["z"]], 1)
            xyz.append(np.ascontiguousarray(p[rng.choice(len(p), min(args.sparse_points, len(p)), replace=False)]))
        host = [(xyz[i % L], xyz[i % L + 1] if i % L + 1 < len(xyz) else xyz[0], None) for i in range(B)]
        if want("sparse"):
            dt, res = timed(lambda: odo.icp_plane_batch(host, reference), args.reps)
            lines.append({**icp_line("sparse", dt, res, B, reference), "points": args.sparse_points})
        if want("sparse_gicp"):
            dt, res = timed(lambda: odo.gicp_batch(host, 10, 0.07), args.reps)
            lines.append({**base, "form": "sparse_gicp", "pairs": B, "points": args.sparse_points,
                          "call_ms": round(dt * 1e3, 3), "pairs_per_s": round(B / dt, 1),
                          "converged": int(sum(r[1] for r in res))})
    for ln in lines:
        s = json.dumps(ln)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")
    odo.close()


if __name__ == "__main__":
    main()
