"""GPU: k_octree's phase 1 from the key histogram, on every way out of it.

Written in the manner of test_octree_resident_gpu.py: one Odometry per (size,
nfeatures), the crafted images as the frames of its one batch. At 320x240 (one
root node, D = 3 or 4 by nfeatures) the dot images of test_octree_key_counts.py
end the restated iterations at depths 1 to 5, by the quota, by the switch to
phase 2 and by running past D (dots(100) at 800 features divides down to single
keys); 2049 keys take the HBM-scratch tier. 532x232 has three root nodes: D = 3
at 800 features, and a sorted list of more than 512 nodes at 4000
(test_octree_hist_model.py asserts which of these ways its inputs reach, on the
CPU). Every (frame, level) of odo_debug_octree, read into canary-filled buffers,
must equal octree_ref and the oracle's octree fed the GPU's own FAST output.
"""
import ctypes as C

import numpy as np
import pytest

import extract_ref as R
from conftest import load_pkg
from test_extract_ref import assert_keys, keys_of, oracle_octree
from test_octree_key_counts import dots, dots_random

pytestmark = pytest.mark.gpu

CANARY = 0xA5
DOT_FRAMES = [(f"dots{k}", (lambda k=k: dots(k))) for k in (2, 100, 255, 600, 2047, 2049)] + \
    [("random2049", lambda: dots_random(2049))]
WIDE_FRAMES = [(name, (lambda name=name: R.FAMILIES[name](532, 232, 7))) for name in ("noise", "dots_varied")]
RUNS = [(320, 240, nf, DOT_FRAMES) for nf in (60, 800, 1500)] + [(532, 232, nf, WIDE_FRAMES) for nf in (800, 4000)]
_RUN = {}


def run(w, h, nf, frames):
    """FAST and octree output of every frame and level of one batch, read back once."""
    if (w, h, nf) in _RUN:
        return _RUN[(w, h, nf)]
    pkg = load_pkg()
    gray = [make() for _, make in frames]
    bgr = np.stack([np.stack([g, g, g], 2) for g in gray])
    dep = np.stack([R.depth_one(w, h) for _ in gray])
    odo = pkg.Odometry(pkg.default_config(w, h, len(gray), nfeatures=nf, iterations=50))
    odo.track_batch_host(bgr, dep)
    lw, lh, _, quota = R.level_tables(w, h, nf)
    out = {"tables": (lw, lh, quota)}
    for i, (name, _) in enumerate(frames):
        d = {"fast": [], "oct": []}
        for l in range(8):
            for what, fn, cap in (("fast", odo.lib.odo_debug_fast, (lw[l] * lh[l]) // 4 + 8),
                                  ("oct", odo.lib.odo_debug_octree, max(quota) + 72)):
                buf = np.empty(cap, pkg.KP_DTYPE)
                buf.view(np.uint8)[...] = CANARY
                n = C.c_int(-1)
                pkg.check(fn(odo.h, i, l, pkg.ptr(buf), cap, C.byref(n)))
                assert 0 <= n.value <= cap, f"{name} {what} level {l}: count {n.value}"
                tail = np.ascontiguousarray(buf[n.value:]).view(np.uint8)
                assert (tail == CANARY).all(), f"{name} {what} level {l}: written past its {n.value} entries"
                d[what].append(buf[:n.value].copy())
        out[name] = d
    odo.close()
    _RUN[(w, h, nf)] = out
    return out


CASES = [(w, h, nf, frames, name) for w, h, nf, frames in RUNS for name, _ in frames]


@pytest.mark.parametrize("w,h,nf,frames,name", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[4]}" for c in CASES])
def test_octree(w, h, nf, frames, name):
    out = run(w, h, nf, frames)
    lw, lh, quota = out["tables"]
    d = out[name]
    if name[4:].isdigit():  # dots<k>: built for k keys at level 0
        assert len(d["fast"][0]) == int(name[4:]), f"level 0 has {len(d['fast'][0])} keys"
    for l in range(8):
        g = d["fast"][l]
        x, y, r = g["x"].astype(np.int64), g["y"].astype(np.int64), g["response"].astype(np.int64)
        keep = R.octree_ref(x, y, r, 16, lw[l] - 16, 16, lh[l] - 16, quota[l])
        assert_keys(d["oct"][l], x[keep], y[keep], r[keep], f"level {l} ({len(x)} keys) vs octree_ref")
        o = oracle_octree(keys_of(x, y, r), lw[l], lh[l], quota[l])
        assert_keys(d["oct"][l], o["x"], o["y"], o["response"], f"level {l} ({len(x)} keys) vs oracle_octree")
