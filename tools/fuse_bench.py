"""Time of the Fuse search of LocalMapping::FuseLandmarks (odo_fuse_search) at
the workload's shape, one JSON line.

A closed-loop synthetic sequence of 1 + --targets frames at 640x480 / 2000
keypoints is extracted once; frame 0 is the current keyframe, the others the
target keyframes, all at their ground-truth poses.

first loop   the current keyframe's landmarks (its depth-valid keypoints in
             world coordinates, about 1900) against every target in ONE call,
             and the same searches as one call per target, in the same process
reverse      the targets' landmarks (their depth-valid keypoints, thinned to
             --reverse-landmarks) against the current keyframe in one call

Each form gets a warm-up, then --reps calls (a quarter as many of the
per-target form) timed with a host clock; every call ends in a synchronise.
No GPU: it fails.

    python tools/fuse_bench.py --out profiles/fuse/bench.jsonl
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


def landmarks_of(pkg, f, Twc):
    ok = f["xyz"][:, 2] > 0
    lms = np.zeros(int(ok.sum()), pkg.LANDMARK_DTYPE)
    lms["X"] = (f["xyz"][ok].astype(np.float64) @ Twc[:3, :3].T + Twc[:3, 3]).astype(np.float32)
    lms["desc"], lms["flags"] = f["desc"][ok], pkg.LM_HAS_OBS
    return lms


def timed(fn, reps):
    fn()  # warm-up (the first call allocates the scratch)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=30)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--reverse-landmarks", type=int, default=31000)
    ap.add_argument("--th", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fuse_bench: no GPU (there is no CPU fallback)")
    pkg, synth = bench.load_pkg(), bench.load_synth()
    W, H, B = 640, 480, args.targets + 1
    bgr, dep, poses = synth.make_sequence(B, W, H, seed=bench.shard_seed(0), closed_loop=True)
    odo = pkg.Odometry(pkg.default_config(W, H, B, nfeatures=args.nfeatures, iterations=50), device=0)
    odo.track_batch_host(np.ascontiguousarray(bgr), np.ascontiguousarray(dep))
    frames = [odo.frame(i) for i in range(B)]
    Tcw = [np.linalg.inv(p).astype(np.float32) for p in poses]
    kf = [(Tcw[i], frames[i]["kun"], frames[i]["ur"], frames[i]["desc"]) for i in range(B)]

    cur = landmarks_of(pkg, frames[0], poses[0])
    idx = np.arange(len(cur), dtype=np.int32)
    span = (0, len(cur))
    calls = [kf[i] + (span,) for i in range(1, B)]
    dt_one, rec = timed(lambda: odo.fuse_search(calls, cur, idx, args.th), args.reps)
    dt_each, parts = timed(lambda: [odo.fuse_search([c], cur, idx, args.th) for c in calls], max(args.reps // 4, 1))
    same = bool(np.concatenate(parts).tobytes() == rec.tobytes())

    rev = np.concatenate([landmarks_of(pkg, frames[i], poses[i]) for i in range(1, B)])
    rev = np.ascontiguousarray(rev[::max(-(-len(rev) // args.reverse_landmarks), 1)])
    ridx = np.arange(len(rev), dtype=np.int32)
    dt_rev, rrec = timed(lambda: odo.fuse_search([kf[0] + ((0, len(rev)),)], rev, ridx, args.th), args.reps)

    def stats(r):
        s = r["n_cand"] >= 0
        return {"searched": int(s.sum()), "with_candidates": int((r["n_cand"] > 0).sum()),
                "mean_candidates": round(float(r["n_cand"][s].mean()), 2) if s.any() else 0.0,
                "over_8": int((r["n_cand"] > 8).sum()), "best_le_50": int((r["best_dist"] <= 50).sum())}

    line = {"tool": "fuse_bench", "targets": args.targets, "nfeatures": args.nfeatures, "th": args.th, "reps": args.reps,
            "keypoints_mean": round(float(np.mean([len(f["kun"]) for f in frames])), 1),
            "first_loop": {"landmarks": int(len(cur)), "records": int(len(rec)),
                           "one_call_ms": round(dt_one * 1e3, 3), "per_target_calls_ms": round(dt_each * 1e3, 3),
                           "one_call_over_per_target": round(dt_each / dt_one, 2), "records_equal": same, **stats(rec)},
            "reverse": {"landmarks": int(len(rev)), "one_call_ms": round(dt_rev * 1e3, 3), **stats(rrec)}}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")
    odo.close()


if __name__ == "__main__":
    main()
