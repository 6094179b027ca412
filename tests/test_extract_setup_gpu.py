"""GPU: the per-workgroup set-up paths of k_fast_seg and k_finalize_lds.

Small frames whose geometry and content reach every case of the kernels'
set-up code: the staging grid (one to seventeen 16-byte columns, x0 & 15 from
0 to 15, a staged row that fills the LDS row), one-cell and eight-cell
segments, the retry bookkeeping (no, some and all cells of a segment redone at
minThFAST, cells that stay empty), the corner-list overflow, and in the
finalisation the level search (levels without keypoints, all keypoints on one
level, totals of 0, not a multiple of 8, above kp_cap) and the workgroup remap.
Which cases the sizes and images reach is asserted here on the CPU, from the
cell arithmetic of extract_ref.py (fast_cells / segments restate
build_geometry) and the reference FAST's per-cell counts, so a geometry change
cannot silently un-cover one. Every frame's FAST candidates, octree order,
keypoints and descriptors are compared bit for bit with the CPU oracle.

Two cases of the kernels cannot be produced by any configuration and are
asserted as such: kp_cap is a multiple of 64, so the finalisation grid
(kp_cap / 8 workgroups per frame) is always a multiple of 8 and the remap is
always taken (1 and 8 frames both run); and no staged row ends closer than
three bytes to FS_RS (269 of 272: eight cells of 31 at x0 & 15 = 15; the
fullest row here is 268, inside the last quad).
"""
import functools

import numpy as np
import pytest

import extract_ref as R
import oracle_lib as O
from conftest import load_pkg
from test_extract_ref import assert_keys, keys_of, oracle_fast, oracle_octree, oracle_pyramid

pytestmark = pytest.mark.gpu

SEED = 7
FS_RS, FS_SEGC, FS_CL = 272, 8, 1024


# ------------------------------------------------------------------ images
def flat(w, h, seed):
    return np.full((h, w), 100, np.uint8)


def one_level(w, h, seed):
    """Single pixels 8 above a flat 100, far apart: corners at minThFAST on
    level 0 only (the first resize already spreads them below the threshold)."""
    img = np.full((h, w), 100, np.uint8)
    img[30:h - 30:37, 30:w - 30:41] = 108
    return img


IMAGES = dict(R.FAMILIES, flat=flat, one_level=one_level)

# (w, h, nfeatures, images). 1804 x 144: a row of 59 cells of 31 (level 0), the
# only kind that fills the staged row; level 7 is 40 rows high, the minimum.
# 532 x 232 at 24 features: three root nodes keep 12 keys per level, 88 in all
# above kp_cap = 64. 300 x 224: level 7 (84 x 63) is one cell; eight frames.
WIDE = (1804, 144, 800, ("noise", "dots_low", "flat", "one_level"))
CAPPED = (532, 232, 24, ("dots_varied",))
SMALL = (300, 224, 60, ("patchwork", "dots_low", "discs", "noise", "flat", "one_level", "blank_but_one",
                         "checker_sat"))
RUNS = {"wide": WIDE, "capped": CAPPED, "small": SMALL}
CASES = [(name, i) for name, r in RUNS.items() for i in range(len(r[3]))]
IDS = [f"{name}-{RUNS[name][3][i]}" for name, i in CASES]


def kp_cap_of(nf):
    return ((nf + 4 * 8 + 8) + 63) & ~63


# ------------------------------------------------------------------ CPU side
@functools.lru_cache(maxsize=None)
def segment_table(w, h, nf):
    """Every level's segments as (level, x0 & 15, cols, ncell, wcell, cell indices)."""
    lw, lh, _, _ = R.level_tables(w, h, nf)
    out = []
    for l in range(8):
        cells, (_, _, wcell, _) = R.fast_cells(lw[l], lh[l])
        for s in R.segments(cells, wcell, FS_SEGC, FS_RS):
            a, b = cells[s[0]], cells[s[-1]]
            out.append((l, int(a["x0"]) & 15, int(b["x0"] + b["cols"] - a["x0"]), len(s), wcell, s))
    return out


@functools.lru_cache(maxsize=None)
def analysis(name, i):
    """The oracle's pyramid of frame i of a run and the reference FAST (with
    its per-cell counts) of every level."""
    w, h, nf, fams = RUNS[name]
    img = IMAGES[fams[i]](w, h, SEED)
    levels = oracle_pyramid(img, nf)
    return img, levels, [R.fast_level_ref(lv) for lv in levels]


@functools.lru_cache(maxsize=None)
def oracle_frame(name, i):
    w, h, nf, fams = RUNS[name]
    img = analysis(name, i)[0]
    return O.extract_frame(np.stack([img] * 3, 2), R.DEPTHS["ramp"](w, h), O.orb_params(nf), O.fr1_calib(), cap=4096)


def test_segment_shapes_reached():
    segs = [s for r in RUNS.values() for s in segment_table(*r[:3])]
    assert any(n == 1 for _, _, _, n, _, _ in segs), "no one-cell segment"
    assert any(n == FS_SEGC for _, _, _, n, _, _ in segs), "no segment of FS_SEGC cells"
    shs = {sh for _, sh, _, _, _, _ in segs}
    assert {0, 15} <= shs and len(shs) >= 8, f"x0 & 15 reaches only {sorted(shs)}"
    nws = {(sh + cols + 15) >> 4 for _, sh, cols, _, _, _ in segs}
    assert 17 in nws and min(nws) <= 4, f"16-byte columns per staged row: {sorted(nws)}"
    fill = max(sh + cols for _, sh, cols, _, _, _ in segs)
    assert all(sh + cols <= FS_RS for _, sh, cols, _, _, _ in segs)
    # within a quad of FS_RS; no geometry passes 269 (test_fullest_row_is_269)
    assert fill >= FS_RS - 4, f"fullest staged row {fill} of {FS_RS}"


def test_fullest_row_is_269():
    """Over every level width an 8-level pyramid of up to 4000 columns can hold,
    no segment's staged row passes 269 bytes."""
    best = 0
    for w in range(72, 4001):
        cells, (_, _, wcell, _) = R.fast_cells(w, 100)
        for s in R.segments(cells, wcell, FS_SEGC, FS_RS):
            a, b = cells[s[0]], cells[s[-1]]
            best = max(best, (int(a["x0"]) & 15) + int(b["x0"] + b["cols"] - a["x0"]))
    assert best == 269


def test_levels_reached():
    for w, h, nf, _ in RUNS.values():
        lw, lh, _, _ = R.level_tables(w, h, nf)
        assert any(a % 4 for a in lw), f"{w}x{h}: every level width is a multiple of 4"
    # 40 rows, the least build_geometry takes (such a level has no cell row)
    assert R.level_tables(*WIDE[:3])[1][7] == 40, "level 7 above the minimum height"


def test_retry_cases_reached():
    seen = set()
    for name, i in CASES:
        w, h, nf, fams = RUNS[name]
        fast = analysis(name, i)[2]
        segs = segment_table(w, h, nf)
        for l, _, _, _, _, s in segs:
            cells = fast[l][3]
            rt = cells["retried"][s]
            seen |= {"some"} if rt.any() and not rt.all() and len(s) > 1 else set()
            seen |= {"all"} if rt.all() and len(s) > 1 else set()
            seen |= {"none"} if not rt.any() else set()
            seen |= {"empty after retry"} if (rt & (cells["n_kept"][s] == 0)).any() else set()
            seen |= {"kept after retry"} if (rt & (cells["n_kept"][s] > 0)).any() else set()
        if fams[i] == "flat":
            for x, _, _, cells in fast:
                assert cells["retried"].all() and (cells["n_kept"] == 0).all() and len(x) == 0
    assert seen == {"some", "all", "none", "empty after retry", "kept after retry"}, seen


def test_corner_list_overflow_reached():
    """A level-0 segment of the noise frames holds more corners at iniThFAST
    than the corner list (the score-map scan), another level's segment fewer."""
    for name in ("wide", "small"):
        w, h, nf, fams = RUNS[name]
        fast = analysis(name, fams.index("noise"))[2]
        per = [(l, int(fast[l][3]["n_ini"][s].sum())) for l, _, _, _, _, s in segment_table(w, h, nf)]
        assert max(n for l, n in per if l == 0) > FS_CL, f"{name}: {max(per)}"
        assert min(n for _, n in per) < FS_CL


def test_finalize_cases_reached():
    totals = {(name, i): len(oracle_frame(name, i)["kps"]) for name, i in CASES}
    caps = {name: kp_cap_of(r[2]) for name, r in RUNS.items()}
    assert any(n % 8 for n in totals.values()), "every total is a multiple of 8"
    assert any(n == 0 for n in totals.values()), "no frame without keypoints"
    assert any(n > caps[name] for (name, _), n in totals.items()), "no total above kp_cap"
    assert any(0 < n < caps[name] for (name, _), n in totals.items())
    one = [set(oracle_frame(name, i)["kps"]["octave"].tolist()) for name, i in CASES]
    assert {0} in one, "no frame with all keypoints on level 0"
    assert any(len(o) == 8 for o in one), "no frame with keypoints on every level"
    # both frame counts of the remap; the grid is a multiple of 8 in both
    # (module docstring)
    assert {len(r[3]) for r in RUNS.values()} >= {1, 8}
    assert all((c // 8) % 8 == 0 for c in caps.values())


# ------------------------------------------------------------------ GPU side
_RUNS = {}


def run(name):
    if name in _RUNS:
        return _RUNS[name]
    pkg = load_pkg()
    w, h, nf, fams = RUNS[name]
    gray = [analysis(name, i)[0] for i in range(len(fams))]
    bgr = np.stack([np.stack([g, g, g], 2) for g in gray])
    dep = np.stack([R.DEPTHS["ramp"](w, h)] * len(fams))
    odo = pkg.Odometry(pkg.default_config(w, h, len(fams), nfeatures=nf, iterations=50))
    assert odo.kp_capacity() == kp_cap_of(nf)
    odo.track_batch_host(bgr, dep)
    out = []
    for i in range(len(fams)):
        out.append(dict(fast=[odo.debug_fast(i, l) for l in range(8)], oct=[odo.debug_octree(i, l) for l in range(8)],
                        frame=odo.frame(i)))
    odo.close()
    _RUNS[name] = out
    return out


@pytest.mark.parametrize("name,i", CASES, ids=IDS)
def test_candidates_and_octree(name, i):
    w, h, nf, _ = RUNS[name]
    g = run(name)[i]
    lw, lh, _, quota = R.level_tables(w, h, nf)
    levels = analysis(name, i)[1]
    for l in range(8):
        o = oracle_fast(levels[l])
        assert_keys(g["fast"][l], o["x"], o["y"], o["response"], f"level {l} vs oracle_fast_level")
        k = oracle_octree(keys_of(o["x"], o["y"], o["response"]), lw[l], lh[l], quota[l])
        assert_keys(g["oct"][l], k["x"], k["y"], k["response"], f"level {l} (quota {quota[l]}) vs oracle_octree")


@pytest.mark.parametrize("name,i", CASES, ids=IDS)
def test_keypoints_and_descriptors(name, i):
    nf = RUNS[name][2]
    fr = run(name)[i]["frame"]
    ref = oracle_frame(name, i)
    n = min(len(ref["kps"]), kp_cap_of(nf))  # the first kp_cap of the oracle's, in its order
    assert len(fr["kps"]) == n, f"N {len(fr['kps'])} vs the oracle's {len(ref['kps'])} (kp_cap {kp_cap_of(nf)})"
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(fr["kps"][f], ref["kps"][f][:n]), f"kp.{f} vs oracle"
    O.assert_same_bits(fr["kps"]["angle"], ref["kps"]["angle"][:n], "angle vs oracle")
    bad = np.nonzero((fr["desc"] != ref["desc"][:n]).any(1))[0]
    assert bad.size == 0, f"descriptors differ from the oracle's at {bad[:8]}"
    for k in ("kun", "xyz", "ur"):
        O.assert_same_bits(fr[k], ref[k][:n], f"{k} vs oracle")
