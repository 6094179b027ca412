"""GPU: every extraction stage on crafted images at edge shapes, each stage fed
the GPU's own previous stage so a failure names its stage.

k_pyramid / k_blur against the oracle; k_fast_seg and k_octree against the
numpy / Python references of extract_ref.py AND the oracle (count, x, y,
response, order); k_finalize_lds against ic_angle_ref (bit-exact) and brief_ref
(outside its ambiguity mask) and the oracle (everywhere); k_kp_geometry against
the float64 geometry_ref within float32 bounds and the oracle bit for bit.
Which kernel paths the images reach (the FAST overflow form, retry cells in
mixed segments, all-tie cells, several root nodes, the rank / sort switch ...)
is asserted on the CPU by test_extract_ref.py.

One Odometry per run, all families as the frames of one batch.
"""
import ctypes as C

import numpy as np
import pytest

import extract_ref as R
import oracle_lib as O
from conftest import load_pkg
from test_extract_ref import (BIG, BIG_FAMILIES, NFEATURES, SEED, SIZES, assert_frame, assert_keys, keys_of,
                              oracle_blur, oracle_fast, oracle_octree, oracle_pyramid, reference_frame, split_levels)

pytestmark = pytest.mark.gpu

RUNS = [(w, h, nf) for (w, h) in SIZES for nf in NFEATURES.get((w, h), (800,))] + [BIG + (800,)]
CASES = [(w, h, nf, f) for (w, h, nf) in RUNS for f in (R.FAMILIES if (w, h) != BIG else BIG_FAMILIES)]
IDS = [f"{w}x{h}-{nf}-{f}" for w, h, nf, f in CASES]
CANARY = 0xA5
_RUNS = {}
_FAST = {}


def families_of(w, h):
    return list(R.FAMILIES if (w, h) != BIG else BIG_FAMILIES)


def depth_of(w, h, i):
    """Frame i's depth family: rotates with the size, so a family meets
    different depths at different sizes."""
    names = list(R.DEPTHS)
    return names[(i + SIZES.index((w, h)) if (w, h) in SIZES else i) % len(names)]


def canary(n, dtype):
    a = np.empty(n, dtype)
    a.view(np.uint8)[...] = CANARY
    return a


def untouched(a, n, what):
    tail = np.ascontiguousarray(a[n:]).view(np.uint8)
    assert (tail == CANARY).all(), f"{what}: written past its {n} entries"


def run(w, h, nf):
    """The batch of all families at one size: every stage's output read back
    once, into canary-filled arrays (nothing past a count may change)."""
    key = (w, h, nf)
    if key in _RUNS:
        return _RUNS[key]
    pkg = load_pkg()
    fams = families_of(w, h)
    gray = [R.FAMILIES[f](w, h, SEED) for f in fams]
    bgr = np.stack([np.stack([g, g, g], 2) for g in gray])
    dep = np.stack([R.DEPTHS[depth_of(w, h, i)](w, h) for i in range(len(fams))])
    cfg = pkg.default_config(w, h, len(fams), nfeatures=nf, iterations=50)
    odo = pkg.Odometry(cfg)
    odo.track_batch_host(bgr, dep)
    lw, lh, scale, quota = R.level_tables(w, h, nf)
    total = sum(a * b for a, b in zip(lw, lh))
    L = odo.lib
    out = {}
    for i, f in enumerate(fams):
        d = {"gray": gray[i], "depth": dep[i]}
        for name, fn in (("pyr", L.odo_debug_pyramid), ("blur", L.odo_debug_blur)):
            buf = canary(total + 4096, np.uint8)
            n = fn(odo.h, i, pkg.ptr(buf), buf.size)
            assert n == total, f"{name}: {n} bytes vs {total}"
            untouched(buf, n, name)
            d[name] = split_levels(buf[:n].copy(), lw, lh)
        d["fast"], d["oct"] = [], []
        for l in range(8):
            for name, fn, cap in (("fast", L.odo_debug_fast, (lw[l] * lh[l]) // 4 + 8),
                                  ("oct", L.odo_debug_octree, nf + 72)):
                buf = canary(cap, pkg.KP_DTYPE)
                n = C.c_int(-1)
                pkg.check(fn(odo.h, i, l, pkg.ptr(buf), cap, C.byref(n)))
                assert 0 <= n.value <= cap, f"{name} level {l}: count {n.value}"
                untouched(buf, n.value, f"{name} level {l}")
                d[name].append(buf[:n.value].copy())
        cap = odo.kp_cap
        fr = dict(kps=canary(cap, pkg.KP_DTYPE), desc=canary(cap * 32, np.uint8), kun=canary(cap * 2, np.float32),
                  xyz=canary(cap * 3, np.float32), ur=canary(cap, np.float32))
        n = C.c_int(-1)
        pkg.check(L.odo_get_frame(odo.h, i, pkg.ptr(fr["kps"]), pkg.ptr(fr["desc"]), pkg.ptr(fr["kun"]),
                                  pkg.ptr(fr["xyz"]), pkg.ptr(fr["ur"]), cap, C.byref(n)))
        n = n.value
        assert 0 <= n <= cap
        for k, per in (("kps", 1), ("desc", 32), ("kun", 2), ("xyz", 3), ("ur", 1)):
            untouched(fr[k], n * per, f"frame {k}")
        d["frame"] = dict(kps=fr["kps"][:n].copy(), desc=fr["desc"][:n * 32].reshape(n, 32).copy(),
                          kun=fr["kun"][:n * 2].reshape(n, 2).copy(), xyz=fr["xyz"][:n * 3].reshape(n, 3).copy(),
                          ur=fr["ur"][:n].copy())
        out[f] = d
    odo.close()
    _RUNS[key] = (out, (lw, lh, scale, quota), cfg)
    return _RUNS[key]


def fast_ref(level):
    """fast_level_ref, computed once per distinct level (the runs of one size
    share their images)."""
    key = (level.shape, level.tobytes())
    if key not in _FAST:
        _FAST[key] = R.fast_level_ref(level)
    return _FAST[key]


@pytest.mark.parametrize("w,h,nf,family", CASES, ids=IDS)
def test_pyramid_and_blur(w, h, nf, family):
    d = run(w, h, nf)[0][family]
    ref = oracle_pyramid(d["gray"], nf)
    for l in range(8):
        bad = np.argwhere(d["pyr"][l] != ref[l])
        assert bad.size == 0, f"pyramid level {l}: {len(bad)} px differ, first (y, x) {bad[0]}"
        bad = np.argwhere(d["blur"][l] != oracle_blur(d["pyr"][l]))
        assert bad.size == 0, f"blur level {l}: {len(bad)} px differ, first (y, x) {bad[0]}"


@pytest.mark.parametrize("w,h,nf,family", CASES, ids=IDS)
def test_fast(w, h, nf, family):
    d = run(w, h, nf)[0][family]
    for l in range(8):
        x, y, r, _ = fast_ref(d["pyr"][l])
        assert_keys(d["fast"][l], x, y, r, f"level {l} vs fast_level_ref")
        o = oracle_fast(d["pyr"][l])
        assert_keys(d["fast"][l], o["x"], o["y"], o["response"], f"level {l} vs oracle_fast_level")


@pytest.mark.parametrize("w,h,nf,family", CASES, ids=IDS)
def test_octree(w, h, nf, family):
    out, (lw, lh, _, quota), _ = run(w, h, nf)
    d = out[family]
    for l in range(8):
        g = d["fast"][l]
        x, y, r = g["x"].astype(np.int64), g["y"].astype(np.int64), g["response"].astype(np.int64)
        keep = R.octree_ref(x, y, r, 16, lw[l] - 16, 16, lh[l] - 16, quota[l])
        assert_keys(d["oct"][l], x[keep], y[keep], r[keep], f"level {l} (quota {quota[l]}) vs octree_ref")
        o = oracle_octree(keys_of(x, y, r), lw[l], lh[l], quota[l])
        assert_keys(d["oct"][l], o["x"], o["y"], o["response"], f"level {l} (quota {quota[l]}) vs oracle_octree")


@pytest.mark.parametrize("w,h,nf,family", CASES, ids=IDS)
def test_keypoints_angles_descriptors(w, h, nf, family):
    out, (lw, lh, scale, quota), cfg = run(w, h, nf)
    d = out[family]
    kept = [(k["x"].astype(np.int64), k["y"].astype(np.int64), k["response"]) for k in d["oct"]]
    ref_kps, ref_desc, mask = reference_frame(d["pyr"], d["blur"], kept, scale)
    fr = d["frame"]
    assert_frame(fr["kps"], fr["desc"], ref_kps, ref_desc, mask, "frame vs references")
    ref = O.extract_frame(np.stack([d["gray"]] * 3, 2), d["depth"], O.orb_params(nf), O.fr1_calib())
    assert len(fr["kps"]) == len(ref["kps"]), f"N {len(fr['kps'])} vs the oracle's {len(ref['kps'])}"
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(fr["kps"][f], ref["kps"][f]), f"kp.{f} vs oracle"
    O.assert_same_bits(fr["kps"]["angle"], ref["kps"]["angle"], "angle vs oracle")
    bad = np.nonzero((fr["desc"] != ref["desc"]).any(1))[0]
    assert bad.size == 0, f"descriptors differ from the oracle's at {bad[:8]}"


@pytest.mark.parametrize("w,h,nf,family", CASES, ids=IDS)
def test_geometry(w, h, nf, family):
    out, _, cfg = run(w, h, nf)
    d = out[family]
    fr = d["frame"]
    c = cfg.calib
    assert c.k1 != 0  # FR1 distortion
    R.assert_geometry(fr["kun"], fr["xyz"], fr["ur"], fr["kps"]["x"], fr["kps"]["y"], d["depth"], c, "frame")
    ref = O.extract_frame(np.stack([d["gray"]] * 3, 2), d["depth"], O.orb_params(nf), O.fr1_calib())
    for k in ("kun", "xyz", "ur"):
        O.assert_same_bits(fr[k], ref[k], f"{k} vs oracle")
