"""Time of dense GICP over a batch (odo_gicp_dense: GeneralizedICP(15, 0.05)::
Compute(pF1, pF2, guess) on the clouds odo_dense_clouds left in HBM), one JSON
line per form.

--batch frames of the closed-loop synthetic sequence (--seq-len distinct
frames, repeated) lie in HBM as odo_track_batch's inputs do; odo_dense_clouds
filters them at --leaf once.

dense        odo_gicp_dense on the batch - 1 consecutive pairs, guess identity:
             grids and covariances once per frame, one ICP workgroup per pair
grid_first   odo_gicp_dense on the first --brute-pairs pairs alone
brute_first  the same clouds copied out and given to odo_gicp_batch (the
             brute-force searches) for those pairs, in the same process; the
             results must equal the grid form's bit for bit

Each form gets a warm-up (the first call allocates the scratch), then --reps
calls timed with a host clock; every call returns with its results downloaded
and the stream idle. No GPU: it fails.

    python tools/gicp_dense_bench.py --out profiles/gicp_dense/bench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/gicp_dense_bench.py --reps 2 --only-dense
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
    ap.add_argument("--iterations", type=int, default=15)
    ap.add_argument("--max-corr-dist", type=float, default=0.05)
    ap.add_argument("--brute-pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-dense", action="store_true", help="the whole-batch form alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gicp_dense_bench: no GPU (there is no CPU fallback)")
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
    it, dist, nb = args.iterations, args.max_corr_dist, min(args.brute_pairs, B - 1)
    base = {"tool": "gicp_dense_bench", "batch": B, "seq_len": L, "leaf": args.leaf, "iterations": it,
            "max_corr_dist": dist, "reps": args.reps, "n_points_mean": round(float(info["n_points"].mean()), 1),
            "n_points_max": int(info["n_points"].max())}
    lines = []
    dt, res = timed(lambda: odo.gicp_dense(pairs, None, it, dist), args.reps)
    lines.append({**base, "form": "dense", "pairs": len(pairs), "call_ms": round(dt * 1e3, 3),
                  "pairs_per_s": round(len(pairs) / dt, 1), "converged": int(sum(r[1] for r in res)),
                  "iterations_mean": round(float(np.mean([r[2] for r in res])), 2),
                  "n_corr_mean": round(float(np.mean([r[3] for r in res])), 1)})
    if not args.only_dense:
        dt_g, first = timed(lambda: odo.gicp_dense(pairs[:nb], None, it, dist), args.reps)
        clouds = [odo.get_dense_cloud(i) for i in range(nb + 1)]
        xyz = [np.ascontiguousarray(np.stack([c["x"], c["y"], c["z"]], 1)) for c in clouds]
        host = [(xyz[i], xyz[i + 1], None) for i in range(nb)]
        dt_b, brute = timed(lambda: odo.gicp_batch(host, it, dist), args.reps)
        same = all(a[1:] == b[1:] and a[0].tobytes() == b[0].tobytes() for a, b in zip(first, brute)) and \
            all(a[1:] == b[1:] and a[0].tobytes() == b[0].tobytes() for a, b in zip(first, res))
        lines.append({**base, "form": "grid_first", "pairs": nb, "call_ms": round(dt_g * 1e3, 3)})
        lines.append({**base, "form": "brute_first", "pairs": nb, "call_ms": round(dt_b * 1e3, 3),
                      "brute_over_grid": round(dt_b / dt_g, 2), "results_equal": bool(same)})
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
