"""GPU: k_octree on both sides of its register-resident / HBM-scratch edge.

One Odometry at 320x240, nfeatures 800; the frames of its one batch are the dot
images of test_octree_key_counts.py (K keys at level 0: the empty level, a node
that never divides, the newSize == S exit, the 256-thread stride, the resident
capacity, each -1 / +0 / +1; equal values, so every retention is a tie that the
first candidate wins), the same at K = cap + 1 with varied responses, and a
noise image (5923 keys at level 0: the scratch path and the rank / sort switch).
Every (frame, level) of odo_debug_octree, read into canary-filled buffers, must
equal octree_ref and the oracle's octree fed the GPU's own FAST output.
"""
import ctypes as C

import numpy as np
import pytest

import extract_ref as R
from conftest import load_pkg
from test_extract_ref import assert_keys, keys_of, oracle_octree
from test_octree_key_counts import H, KS, RESIDENT_CAP, W, dots, dots_random

pytestmark = pytest.mark.gpu

NF = 800
CANARY = 0xA5
FRAMES = [(f"dots{k}", k) for k in KS] + [("random", RESIDENT_CAP + 1), ("noise", None)]
_RUN = {}


def image(name, k):
    if name == "noise":
        return R.noise(W, H, 7)
    return dots_random(k) if name == "random" else dots(k)


def run():
    """FAST and octree output of every frame and level, read back once."""
    if _RUN:
        return _RUN
    pkg = load_pkg()
    gray = [image(name, k) for name, k in FRAMES]
    bgr = np.stack([np.stack([g, g, g], 2) for g in gray])
    dep = np.stack([R.depth_one(W, H) for _ in gray])
    odo = pkg.Odometry(pkg.default_config(W, H, len(gray), nfeatures=NF, iterations=50))
    odo.track_batch_host(bgr, dep)
    lw, lh, _, quota = R.level_tables(W, H, NF)
    for i, (name, _) in enumerate(FRAMES):
        d = {"fast": [], "oct": []}
        for l in range(8):
            for what, fn, cap in (("fast", odo.lib.odo_debug_fast, (lw[l] * lh[l]) // 4 + 8),
                                  ("oct", odo.lib.odo_debug_octree, NF + 72)):
                buf = np.empty(cap, pkg.KP_DTYPE)
                buf.view(np.uint8)[...] = CANARY
                n = C.c_int(-1)
                pkg.check(fn(odo.h, i, l, pkg.ptr(buf), cap, C.byref(n)))
                assert 0 <= n.value <= cap, f"{name} {what} level {l}: count {n.value}"
                tail = np.ascontiguousarray(buf[n.value:]).view(np.uint8)
                assert (tail == CANARY).all(), f"{name} {what} level {l}: written past its {n.value} entries"
                d[what].append(buf[:n.value].copy())
        _RUN[name] = d
    odo.close()
    _RUN["tables"] = (lw, lh, quota)
    return _RUN


@pytest.mark.parametrize("name,k", FRAMES, ids=[f[0] for f in FRAMES])
def test_octree(name, k):
    out = run()
    lw, lh, quota = out["tables"]
    d = out[name]
    n0 = len(d["fast"][0])
    if k is not None:
        assert n0 == k, f"level 0 has {n0} keys, the image was built for {k}"
    else:
        assert n0 > 2 * RESIDENT_CAP
    for l in range(8):
        g = d["fast"][l]
        x, y, r = g["x"].astype(np.int64), g["y"].astype(np.int64), g["response"].astype(np.int64)
        keep = R.octree_ref(x, y, r, 16, lw[l] - 16, 16, lh[l] - 16, quota[l])
        assert_keys(d["oct"][l], x[keep], y[keep], r[keep], f"level {l} ({len(x)} keys) vs octree_ref")
        o = oracle_octree(keys_of(x, y, r), lw[l], lh[l], quota[l])
        assert_keys(d["oct"][l], o["x"], o["y"], o["response"], f"level {l} ({len(x)} keys) vs oracle_octree")
