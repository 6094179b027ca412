"""Time of the dense clouds of a batch (odo_dense_clouds: Frame::CreateCloud +
VoxelGridFilterCloud on the device), one JSON line.

--batch frames of the closed-loop synthetic sequence (--seq-len distinct
frames, repeated) lie in HBM as odo_track_batch's inputs do.

one call     every frame's cloud at --leaf in ONE call
per frame    the same frames as one call per frame, in the same process

Each form gets a warm-up (the first call allocates the scratch), then --reps
calls (an eighth as many of the per-frame form) timed with a host clock; every
call returns with the infos downloaded and the stream idle. No GPU: it fails.

    python tools/cloud_bench.py --out profiles/cloud/bench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/cloud_bench.py --reps 8 --only-batch

--only-batch times the one-call form alone, so that a kernel trace of the run
holds the launches of whole-batch calls only.
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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--only-batch", action="store_true", help="the one-call form alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cloud_bench: no GPU (there is no CPU fallback)")
    pkg, synth = bench.load_pkg(), bench.load_synth()
    W, H, B = 640, 480, args.batch
    L = min(args.seq_len, B)
    bgr, dep, _ = synth.make_sequence(L, W, H, seed=bench.shard_seed(0), closed_loop=True)
    idx = np.arange(B) % L
    d_bgr = torch.from_numpy(np.ascontiguousarray(bgr[idx])).to("cuda")
    d_dep = torch.from_numpy(np.ascontiguousarray(dep[idx]).view(np.int16)).to("cuda")
    odo = pkg.Odometry(pkg.default_config(W, H, B, nfeatures=2000, iterations=50), device=0)
    torch.cuda.synchronize()
    pb, pd, fb, fd = d_bgr.data_ptr(), d_dep.data_ptr(), W * H * 3, W * H * 2

    dt_one, info = timed(lambda: odo.dense_clouds(pb, pd, B, args.leaf), args.reps)
    line = {"tool": "cloud_bench", "batch": B, "seq_len": L, "leaf": args.leaf, "reps": args.reps,
            "n_valid_mean": round(float(info["n_valid"].mean()), 1), "n_points_mean": round(float(info["n_points"].mean()), 1),
            "n_points_max": int(info["n_points"].max()), "filtered": int((info["status"] == pkg.CLOUD_OK).sum()),
            "one_call_ms": round(dt_one * 1e3, 3), "clouds_per_s": round(B / dt_one, 1),
            "gpixels_per_s": round(B * W * H / dt_one / 1e9, 3)}
    if not args.only_batch:
        first = odo.get_dense_cloud(0)
        last = odo.get_dense_cloud(B - 1)
        dt_each, parts = timed(lambda: [odo.dense_clouds(pb + i * fb, pd + i * fd, 1, args.leaf)[0] for i in range(B)],
                               max(args.reps // 8, 1))
        same = bool(np.array(parts, info.dtype).tobytes() == info.tobytes() and
                    odo.get_dense_cloud(0).tobytes() == last.tobytes())
        dt_raw, raw = timed(lambda: odo.dense_clouds(pb, pd, B, 0.0), max(args.reps // 4, 1))
        line.update({"per_frame_calls_ms": round(dt_each * 1e3, 3), "per_frame_clouds_per_s": round(B / dt_each, 1),
                     "one_call_over_per_frame": round(dt_each / dt_one, 2), "results_equal": same,
                     "create_cloud_only_ms": round(dt_raw * 1e3, 3), "create_cloud_points": int(raw["n_points"].sum()),
                     "first_cloud_points": int(len(first))})
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")
    odo.close()


if __name__ == "__main__":
    main()
