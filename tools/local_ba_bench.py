"""Time of one local bundle adjustment (odo_local_ba) at the workload's own shape.

One synthetic problem: 20 free and 20 fixed keyframes within a few degrees /
decimetres of each other, 8192 landmarks 2 to 4 m in front of them, about 6
observations each (half stereo, half monocular), 0.5 px noise, 10 % gross
outliers; free poses start 1 degree / 3 cm off, points 2 cm. After a warm-up
(which allocates the scratch) the same call is repeated --reps times, each
timed with a host clock (the call ends in a synchronise).

One JSON line (stdout, and appended to --out): the median ms per call,
iterations and Levenberg trials of both stages, edges and edges per second
(edges x linear solves / time). No GPU: it fails.

    python tools/local_ba_bench.py --out profiles/local_ba/bench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/local_ba_bench.py --reps 1
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def make_problem(pkg, n_free, n_fixed, n_lm, mean_obs, noise, outliers, seed, calib):
    rng = np.random.default_rng(seed)
    nk = n_free + n_fixed
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
    T = np.tile(np.eye(4), (nk, 1, 1))
    for k in range(nk):
        T[k, :3, :3] = rodrigues(unit() * math.radians(rng.uniform(0, 4)))
        T[k, :3, 3] = rng.uniform(-0.3, 0.3, 3) * [1, 1, 0.3]
    X = rng.random((n_lm, 3)) * [1.2, 1.0, 2] + [-0.6, -0.5, 2.0]
    fixed = np.zeros(nk, np.uint8)
    fixed[rng.permutation(nk)[:n_fixed]] = 1
    cnt = np.clip(rng.poisson(mean_obs, n_lm), 2, nk)
    lm = np.repeat(np.arange(n_lm), cnt)
    kf = np.concatenate([rng.choice(nk, m, replace=False) for m in cnt])
    p = rng.permutation(len(lm))
    lm, kf = lm[p], kf[p]
    Xc = np.einsum("mij,mj->mi", T[kf, :3, :3], X[lm]) + T[kf, :3, 3]
    iz = 1.0 / Xc[:, 2]
    u = calib.fx * Xc[:, 0] * iz + calib.cx + rng.normal(size=len(lm)) * noise
    v = calib.fy * Xc[:, 1] * iz + calib.cy + rng.normal(size=len(lm)) * noise
    ur = u - calib.mbf * iz + rng.normal(size=len(lm)) * noise
    g = rng.random(len(lm)) < outliers
    u[g] += rng.choice([-1.0, 1.0], int(g.sum())) * rng.uniform(15, 60, int(g.sum()))
    v[g] += rng.choice([-1.0, 1.0], int(g.sum())) * rng.uniform(15, 60, int(g.sum()))
    E = np.zeros(len(lm), pkg.BA_EDGE_DTYPE)
    E["kf"], E["lm"], E["u"], E["v"] = kf, lm, u, v
    E["ur"] = np.where(rng.random(len(lm)) < 0.5, np.maximum(ur, 0.0), -1.0)
    T0 = T.copy()
    for k in np.nonzero(fixed == 0)[0]:
        D = np.eye(4)
        D[:3, :3] = rodrigues(unit() * math.radians(1.0))
        D[:3, 3] = unit() * 0.03
        T0[k] = D @ T[k]
    X0 = X + rng.normal(size=X.shape) * 0.02
    return T0.astype(np.float32), fixed, X0.astype(np.float32), E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--free", type=int, default=20)
    ap.add_argument("--fixed", type=int, default=20)
    ap.add_argument("--landmarks", type=int, default=8192)
    ap.add_argument("--obs", type=float, default=6.0, help="mean observations per landmark")
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--outliers", type=float, default=0.10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0xBA)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("local_ba_bench: no GPU (there is no CPU fallback)")
    pkg = bench.load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 1, nfeatures=500), device=0)
    cal = odo.cfg.calib
    T0, fixed, X0, E = make_problem(pkg, args.free, args.fixed, args.landmarks, args.obs, args.noise, args.outliers,
                                    args.seed, cal)
    for _ in range(max(1, args.warmup)):
        T, X, erase, res = odo.local_ba(T0, fixed, X0, E)
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        T, X, erase, res = odo.local_ba(T0, fixed, X0, E)
        ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    trials = res.trials1 + res.trials2
    line = {"tool": "local_ba_bench", "free": args.free, "fixed": args.fixed, "landmarks": args.landmarks,
            "edges": int(len(E)), "reps": args.reps, "ms_per_call": round(med, 3),
            "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
            "iters": [res.iters1, res.iters2], "trials": [res.trials1, res.trials2],
            "ms_per_trial": round(med / max(trials, 1), 3),
            "edges_per_s": round(len(E) * trials / (med * 1e-3), 1),
            "chi2": [res.chi2_initial, res.chi2_stage1, res.chi2_final], "n_level1": res.n_level1,
            "n_erase": res.n_erase}
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")
    odo.close()


if __name__ == "__main__":
    main()
