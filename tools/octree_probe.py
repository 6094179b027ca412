"""Stage times of k_octree's first- and last-level workgroups of frame 0 on one
bench batch (256 frames of the synthetic loop at 640x480, 2000 features). A
-DODO_OCTREE_PROFILE build named by ODO_LIB prints, per launch, one line per
stamp: the 10 ns ticks since the previous stamp (S start, G gather, H the
classify pass into the histogram, I initial nodes, 1 / 2 an iteration of that
phase, L the lookup pass, R retention). Usage: ODO_LIB=... python
tools/octree_probe.py > stamps.txt; the summary goes to stderr."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg, load_synth  # noqa: E402


def summarise(path):
    """Per level, the stamps of the last launch in `path`: tag and microseconds."""
    runs = {}
    for line in open(path):
        m = re.match(r"OTP level (\d+) keys (\d+) stamp (\d+) (\S) (\d+)", line)
        if m:
            l, n, i, tag, dt = int(m[1]), int(m[2]), int(m[3]), m[4], int(m[5])
            if i == 1:
                runs[l] = (n, [])
            runs[l][1].append((tag, dt / 100.0))
    for l, (n, st) in sorted(runs.items()):
        total = sum(d for _, d in st)
        print(f"level {l}: {n} keys, {total:.1f} us: " + " ".join(f"{t}:{d:.1f}" for t, d in st), file=sys.stderr)


def main():
    if len(sys.argv) > 1:
        return summarise(sys.argv[1])
    pkg = load_pkg()
    synth = load_synth()
    B = int(os.environ.get("OCTREE_PROBE_FRAMES", "256"))
    bgr, dep, _ = synth.make_sequence(64, 640, 480, seed=0x5EED0002, closed_loop=True)
    reps = (B + 63) // 64
    bgr, dep = np.concatenate([bgr] * reps)[:B], np.concatenate([dep] * reps)[:B]
    odo = pkg.Odometry(pkg.default_config(640, 480, B, nfeatures=2000, iterations=500))
    for _ in range(3):
        odo.track_batch_host(bgr, dep)
        odo.synchronize()
    odo.close()


if __name__ == "__main__":
    main()
