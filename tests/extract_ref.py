"""Independent references for the ORB-SLAM2 extractor, and adversarial images.

Written from the reference's Features/orbextractor.cpp and Core/frame.cpp (and
the published definitions of FAST-9/16, cv::fastAtan2 and cv::undistortPoints),
not from oracle/orb_ref.cpp: test_extract_ref.py holds the oracle against these
and test_extract_stages_gpu.py holds the HIP kernels against both. Plain numpy
and Python, no GPU, no oracle import.

  level_tables     ORBextractor ctor (orbextractor.cpp:346-381) + level sizes (:837-838)
  fast_level_ref   the FAST part of ComputeKeyPointsOctTree (:669-723)
  octree_ref       DistributeOctTree / DivideNode (:412-663)
  ic_angle_ref     IC_Angle (:14-39), the umax table (:389-403), cv::fastAtan2
  brief_ref        computeOrbDescriptor (:43-85) with the rotated pattern evaluated exactly
  geometry_ref     Frame::UndistortKeyPoints + ExtractFeatures (frame.cpp:139-164, 286-313) in float64
  FAMILIES / DEPTHS  crafted images and depth maps
"""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EDGE_THRESHOLD = 19
BORDER = EDGE_THRESHOLD - 3   # minBorderX / minBorderY (orbextractor.cpp:672)
HALF_PATCH = 15


def cv_round(v):
    """cvRound: round half to even."""
    return int(np.rint(v))


# ------------------------------------------------------------------ tables
def level_tables(w, h, nfeatures, scale_factor=1.2, nlevels=8):
    """(widths, heights, float32 scales, quotas) of the pyramid levels. The
    scaleFactor member is a double holding the float argument."""
    sf = float(F32(scale_factor))
    scale = [F32(1.0)]
    for _ in range(1, nlevels):
        scale.append(F32(float(scale[-1]) * sf))
    inv = [F32(1.0) / s for s in scale]
    factor = F32(1.0 / sf)
    nd = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(math.pow(float(factor), float(nlevels))))
    quota, total = [], 0
    for _ in range(nlevels - 1):
        quota.append(cv_round(nd))
        total += quota[-1]
        nd = nd * factor
    quota.append(max(nfeatures - total, 0))
    lw = [cv_round(F32(w) * s) for s in inv]
    lh = [cv_round(F32(h) * s) for s in inv]
    return lw, lh, scale, quota


def umax_table():
    """End of each row of the circular patch (orbextractor.cpp:389-403)."""
    umax = [0] * (HALF_PATCH + 1)
    vmax = int(math.floor(float(F32(HALF_PATCH) * np.sqrt(F32(2.0)) / F32(2) + F32(1))))
    vmin = int(math.ceil(float(F32(HALF_PATCH) * np.sqrt(F32(2.0)) / F32(2))))
    hp2 = float(HALF_PATCH * HALF_PATCH)
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(hp2 - v * v))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


def orb_pattern():
    """The 256 rBRIEF tests (x0, y0, x1, y1): OpenCV's published bit_pattern_31,
    kept as data in include/odo_orb_pattern.h."""
    txt = open(os.path.join(ROOT, "include", "odo_orb_pattern.h")).read()
    body = txt[txt.index("{") + 1:txt.index("}")]
    v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024
    return v.reshape(256, 4)


# ------------------------------------------------------------------ FAST
# the Bresenham circle of radius 3, (dx, dy), in FAST's order
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
          (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_strength(img):
    """Per pixel, the FAST-9/16 strength m by definition: the largest t such
    that 9 contiguous circle pixels are all darker than v - t + 1 or all
    brighter than v + t - 1, i.e. the maximum over the 16 arcs of the minimum
    of the 9 differences (and of their negatives). A pixel is a corner at
    threshold th iff m > th; its score is m - 1 (0 in the 3-pixel frame)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    m = np.zeros((h, w), np.int16)
    if h < 7 or w < 7:
        return m
    v = img[3:h - 3, 3:w - 3].astype(np.int16)
    d = np.stack([v - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int16) for dx, dy in CIRCLE])
    dd = np.concatenate([d, d[:8]])                    # cyclic: 24 planes
    best = None
    for sign in (1, -1):
        s = dd if sign == 1 else -dd
        m2 = np.minimum(s[:-1], s[1:])                 # 23: runs of 2
        m4 = np.minimum(m2[:-2], m2[2:])               # 21: runs of 4
        m8 = np.minimum(m4[:-4], m4[4:])               # 17: runs of 8
        m9 = np.minimum(m8[:16], s[8:24])              # 16: runs of 9
        arc = m9.max(0)
        best = arc if best is None else np.maximum(best, arc)
    m[3:h - 3, 3:w - 3] = best
    return m


def _fast_roi(ms, th):
    """cv::FAST(roi, th, nonmaxSuppression=true) given the ROI's strength map:
    corners in the ROI minus its 3-pixel frame, kept iff the score is strictly
    greater than all eight neighbours, neighbours outside that area counting 0.
    Returns (x, y, score) in row-major order and the corner count before NMS."""
    rows, cols = ms.shape
    if rows < 7 or cols < 7:
        z = np.zeros(0, np.int64)
        return z, z, z, 0
    inner = ms[3:rows - 3, 3:cols - 3].astype(np.int32)
    corner = inner > th
    s = np.zeros((rows - 4, cols - 4), np.int32)
    s[1:-1, 1:-1] = np.where(corner, inner - 1, 0)
    c = s[1:-1, 1:-1]
    nb = np.zeros_like(c)
    H, W = c.shape
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nb = np.maximum(nb, s[dy:dy + H, dx:dx + W])
    keep = corner & (c > nb)
    ys, xs = np.nonzero(keep)
    return xs + 3, ys + 3, c[ys, xs], int(corner.sum())


CELL_DTYPE = np.dtype([("i", "i4"), ("j", "i4"), ("x0", "i4"), ("y0", "i4"), ("cols", "i4"), ("rows", "i4"),
                       ("n_ini", "i4"), ("retried", "?"), ("n_kept", "i4")])


def fast_cells(w, h):
    """The cell grid of one level (orbextractor.cpp:669-703): a CELL_DTYPE
    array (counts zero) in the loops' order and (nCols, nRows, wCell, hCell)."""
    min_bx = min_by = BORDER
    max_bx, max_by = w - EDGE_THRESHOLD + 3, h - EDGE_THRESHOLD + 3
    width, height = F32(max_bx - min_bx), F32(max_by - min_by)
    ncols, nrows = int(width / F32(30)), int(height / F32(30))
    cells = []
    if ncols <= 0 or nrows <= 0:  # the reference's loops do not run (wCell / hCell are never used)
        return np.zeros(0, CELL_DTYPE), (ncols, nrows, 0, 0)
    wcell, hcell = int(math.ceil(width / F32(ncols))), int(math.ceil(height / F32(nrows)))
    for i in range(nrows):
        ini_y = min_by + i * hcell
        max_y = ini_y + hcell + 6
        if ini_y >= max_by - 3:
            continue
        max_y = min(max_y, max_by)
        for j in range(ncols):
            ini_x = min_bx + j * wcell
            max_x = ini_x + wcell + 6
            if ini_x >= max_bx - 6:
                continue
            max_x = min(max_x, max_bx)
            cells.append((i, j, ini_x, ini_y, max_x - ini_x, max_y - ini_y, 0, False, 0))
    return np.array(cells, CELL_DTYPE), (ncols, nrows, wcell, hcell)


def fast_level_ref(level, ini_th=20, min_th=7):
    """vToDistributeKeys of one level: (x, y, response) int arrays relative to
    the 16-pixel border, in the order of the reference's loops (cells row-major,
    each cell's corners row-major), and the per-cell CELL_DTYPE record: n_ini =
    corners at ini_th before NMS, retried = the cell kept nothing at ini_th and
    was redone at min_th, n_kept = corners it contributes."""
    level = np.ascontiguousarray(level, np.uint8)
    h, w = level.shape
    cells, (ncols, nrows, wcell, hcell) = fast_cells(w, h)
    m = fast_strength(level)
    X, Y, R = [], [], []
    for c in cells:
        roi = m[c["y0"]:c["y0"] + c["rows"], c["x0"]:c["x0"] + c["cols"]]
        x, y, r, n_ini = _fast_roi(roi, ini_th)
        c["n_ini"] = n_ini
        if x.size == 0:
            c["retried"] = True
            x, y, r, _ = _fast_roi(roi, min_th)
        c["n_kept"] = x.size
        X.append(x + c["j"] * wcell)
        Y.append(y + c["i"] * hcell)
        R.append(r)
    cat = lambda a: np.concatenate(a).astype(np.int64) if a else np.zeros(0, np.int64)
    return cat(X), cat(Y), cat(R), cells


# ------------------------------------------------------------------ octree
class _Node:
    __slots__ = ("ulx", "uly", "urx", "bry", "keys", "no_more", "seq")

    def __init__(self, ulx, uly, urx, bry, keys):
        self.ulx, self.uly, self.urx, self.bry, self.keys = ulx, uly, urx, bry, keys
        self.no_more = False
        self.seq = -1


def _c_round(v):
    """C round(): half away from zero."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def octree_ref(x, y, resp, min_x, max_x, min_y, max_y, n_want, stats=None):
    """DistributeOctTree: the indices of the retained keys, in vResultKeys'
    order. x, y, resp: the level's candidates (relative to the border), in
    vToDistributeKeys order. The std::list is a Python list (push_front =
    insert at 0). The std::sort of (size, pointer) pairs compares pointers for
    equal sizes, which the reference leaves to the allocator: pinned to creation
    order (a node made later compares greater, so is divided first), DESIGN.md
    §4 k_octree. `stats`, if a dict, receives the lengths of the lists sorted."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    resp = np.asarray(resp, np.float32)
    n_ini = _c_round(float(F32(max_x - min_x) / F32(max_y - min_y)))
    hx = F32(max_x - min_x) / F32(n_ini)
    seq = [0]

    def stamp(nd):
        nd.seq = seq[0]
        seq[0] += 1
        return nd

    roots = []
    for i in range(n_ini):
        ulx, urx = int(hx * F32(i)), int(hx * F32(i + 1))
        roots.append(stamp(_Node(ulx, 0, urx, max_y - min_y, None)))
    which = (x / hx).astype(np.int64)       # float32 division, truncated
    for i, nd in enumerate(roots):
        nd.keys = np.nonzero(which == i)[0]
    nodes = []
    for nd in roots:
        if nd.keys.size == 1:
            nd.no_more = True
            nodes.append(nd)
        elif nd.keys.size > 1:
            nodes.append(nd)

    def divide(nd):
        half_x = int(math.ceil(float(F32(nd.urx - nd.ulx) / F32(2))))
        half_y = int(math.ceil(float(F32(nd.bry - nd.uly) / F32(2))))
        mx, my = nd.ulx + half_x, nd.uly + half_y
        k = nd.keys
        left, top = x[k] < mx, y[k] < my
        ch = [_Node(nd.ulx, nd.uly, mx, my, k[left & top]), _Node(mx, nd.uly, nd.urx, my, k[~left & top]),
              _Node(nd.ulx, my, mx, nd.bry, k[left & ~top]), _Node(mx, my, nd.urx, nd.bry, k[~left & ~top])]
        for c in ch:
            c.no_more = c.keys.size == 1
        return ch

    finish = False
    while not finish:
        prev = len(nodes)
        pushed, kept, to_sort, n_expand = [], [], [], 0
        for nd in nodes:                       # children go to the front: not visited in this pass
            if nd.no_more:
                kept.append(nd)
                continue
            for c in divide(nd):
                if c.keys.size > 0:
                    pushed.append(stamp(c))
                    if c.keys.size > 1:
                        n_expand += 1
                        to_sort.append(c)
        nodes = pushed[::-1] + kept
        if len(nodes) >= n_want or len(nodes) == prev:
            finish = True
        elif len(nodes) + n_expand * 3 > n_want:
            while not finish:
                prev = len(nodes)
                order = sorted(to_sort, key=lambda c: (c.keys.size, c.seq))
                if stats is not None:
                    stats.setdefault("sorted", []).append(len(order))
                to_sort = []
                for nd in reversed(order):
                    for c in divide(nd):
                        if c.keys.size > 0:
                            nodes.insert(0, stamp(c))
                            if c.keys.size > 1:
                                to_sort.append(c)
                    nodes.remove(nd)           # identity: _Node defines no __eq__
                    if len(nodes) >= n_want:
                        break
                if len(nodes) >= n_want or len(nodes) == prev:
                    finish = True
    out = []
    for nd in nodes:
        r = resp[nd.keys]
        best, best_r = 0, r[0]
        for k in range(1, r.size):             # strictly greater: the first maximum wins
            if r[k] > best_r:
                best, best_r = k, r[k]
        out.append(int(nd.keys[best]))
    return np.array(out, np.int64)


# ------------------------------------------------------------------ IC angle
def fast_atan2_f32(yv, xv):
    """cv::fastAtan2 (degrees) restated in float32 operations."""
    yv = np.asarray(yv, F32)
    xv = np.asarray(xv, F32)
    scale = F32(180 / math.pi)
    p1, p3 = F32(0.9997878412794807) * scale, F32(-0.3258083974640975) * scale
    p5, p7 = F32(0.1555786518463281) * scale, F32(-0.04432655554792128) * scale
    eps = F32(2.220446049250313e-16)
    ax, ay = np.abs(xv), np.abs(yv)
    with np.errstate(invalid="ignore", divide="ignore"):
        swap = ~(ax >= ay)
        num, den = np.where(swap, ax, ay), np.where(swap, ay, ax)
        c = (num / (den + eps)).astype(F32)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
        a = np.where(swap, F32(90) - a, a).astype(F32)
        a = np.where(xv < 0, F32(180) - a, a).astype(F32)
        a = np.where(yv < 0, F32(360) - a, a).astype(F32)
    return a


def ic_moments(level, x, y):
    """Exact integer (m01, m10) over the umax disc around (x, y)."""
    level = np.asarray(level)
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    um = umax_table()
    off = np.arange(-HALF_PATCH, HALF_PATCH + 1)
    disc = np.array([[abs(u) <= um[abs(v)] for u in off] for v in off])
    patch = level[(y[:, None] + off[None, :])[:, :, None], (x[:, None] + off[None, :])[:, None, :]].astype(np.int64)
    patch = patch * disc[None]
    m10 = (patch * off[None, None, :]).sum((1, 2))
    m01 = (patch * off[None, :, None]).sum((1, 2))
    return m01, m10


def ic_angle_ref(level, x, y):
    """IC_Angle at integer level coordinates (x, y): float32 degrees."""
    m01, m10 = ic_moments(level, x, y)
    return fast_atan2_f32(m01.astype(F32), m10.astype(F32))


# ------------------------------------------------------------------ rBRIEF
AMBIGUITY = 2.0 ** -17


def brief_ref(blurred, x, y, angle):
    """computeOrbDescriptor at integer level coordinates: (desc, mask), both
    (n, 32) uint8. a, b are the float32 of the double cos / sin of
    float32(angle) * float32(pi / 180). Each rotated coordinate p.x * b + p.y * a,
    p.x * a - p.y * b is evaluated in float64 from those float32 values: the
    products are exact (24 bits by 4) and the sum is rounded at 2^-49 or
    better, far inside the band below. A coordinate within 2^-17 of a
    half-integer is ambiguous (a fused and an unfused float32 evaluation differ
    by at most about four float32 ulps of a value below 32 and can round to
    different sides only there); mask has the bit of every test that touches
    one. Every other coordinate rounds the one possible way."""
    blurred = np.asarray(blurred)
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    ang = np.asarray(angle, F32) * F32(math.pi / F32(180))
    a = np.cos(ang.astype(np.float64)).astype(F32).astype(np.float64)[:, None]
    b = np.sin(ang.astype(np.float64)).astype(F32).astype(np.float64)[:, None]
    pat = orb_pattern().astype(np.float64)
    val, amb = [], []
    for px, py in ((pat[:, 0], pat[:, 1]), (pat[:, 2], pat[:, 3])):
        fy = px[None, :] * b + py[None, :] * a
        fx = px[None, :] * a - py[None, :] * b
        bad = np.zeros(fy.shape, bool)
        for f in (fx, fy):
            bad |= np.abs(f - np.floor(f) - 0.5) < AMBIGUITY
        iy, ix = np.rint(fy).astype(np.int64), np.rint(fx).astype(np.int64)
        val.append(blurred[y[:, None] + iy, x[:, None] + ix].astype(np.int64))
        amb.append(bad)
    bits = (val[0] < val[1]).astype(np.uint8)
    desc = np.packbits(bits, axis=1, bitorder="little")
    mask = np.packbits((amb[0] | amb[1]).astype(np.uint8), axis=1, bitorder="little")
    return desc, mask


# ------------------------------------------------------------------ geometry
def geometry_ref(kx, ky, depth, calib):
    """Float64 UndistortKeyPoints (cv::undistortPoints with P = K: five
    fixed-point iterations) and the depth lookup / back-projection of
    ExtractFeatures. kx, ky: float32 keypoint coordinates; depth: uint16 (h, w);
    calib: an object with fx fy cx cy k1 k2 p1 p2 k3 depth_factor mbf (the
    float32 values). Returns float64 (kun (n, 2), z, X, Y, ur) with the
    reference's 0 / -1 where the depth is not positive."""
    kx = np.asarray(kx, F32)
    ky = np.asarray(ky, F32)
    c = {k: float(F32(getattr(calib, k))) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3",
                                                    "depth_factor", "mbf")}
    u, v = kx.astype(np.float64), ky.astype(np.float64)
    if c["k1"] == 0.0:
        un = np.stack([u, v], 1)
    else:
        x0, y0 = (u - c["cx"]) / c["fx"], (v - c["cy"]) / c["fy"]
        px, py = x0.copy(), y0.copy()
        for _ in range(5):
            r2 = px * px + py * py
            icd = 1.0 / (1.0 + ((c["k3"] * r2 + c["k2"]) * r2 + c["k1"]) * r2)
            dx = 2 * c["p1"] * px * py + c["p2"] * (r2 + 2 * px * px)
            dy = c["p1"] * (r2 + 2 * py * py) + 2 * c["p2"] * px * py
            px, py = (x0 - dx) * icd, (y0 - dy) * icd
        un = np.stack([px * c["fx"] + c["cx"], py * c["fy"] + c["cy"]], 1)
    d = np.asarray(depth)[ky.astype(np.int64), kx.astype(np.int64)].astype(np.float64)  # at<float>(v, u): truncation
    z = d * c["depth_factor"]
    has = z > 0
    zs = np.where(has, z, 1.0)
    X = np.where(has, (un[:, 0] - c["cx"]) * z / c["fx"], 0.0)
    Y = np.where(has, (un[:, 1] - c["cy"]) * z / c["fy"], 0.0)
    ur = np.where(has, un[:, 0] - c["mbf"] / zs, -1.0)
    return un, np.where(has, z, 0.0), X, Y, ur


# ------------------------------------------------------------------ images
def _rng(w, h, seed, salt):
    return np.random.default_rng([seed, w, h, salt])


def noise(w, h, seed):
    """Uniform white noise 0..255: a quarter of the pixels are corners."""
    return _rng(w, h, seed, 1).integers(0, 256, (h, w), dtype=np.uint8)


def discs(w, h, seed):
    """Bright discs of radius 2, period 7, on 10, one intensity per disc:
    plateaus whose corners tie with a neighbour."""
    rng = _rng(w, h, seed, 2)
    img = np.full((h, w), 10, np.uint8)
    ny, nx = (h + 6) // 7, (w + 6) // 7
    val = rng.integers(150, 255, (ny, nx), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    dy, dx = yy % 7 - 3, xx % 7 - 3
    on = dx * dx + dy * dy <= 4
    img[on] = val[yy // 7, xx // 7][on]
    return img


def dots_equal(w, h, seed):
    """Single pixels, period 4, all 255 on 0: every response equal and at the top of the range."""
    img = np.zeros((h, w), np.uint8)
    img[1::4, 1::4] = 255
    return img


def dots_varied(w, h, seed):
    """Single pixels, period 4, 30..255 on 0."""
    img = np.zeros((h, w), np.uint8)
    img[1::4, 1::4] = _rng(w, h, seed, 4).integers(30, 256, img[1::4, 1::4].shape, dtype=np.uint8)
    return img


def dots_low(w, h, seed):
    """Single pixels 8..27 above 100, period 6; in about half of the 37-pixel
    blocks the dots stay at 8..20, below iniThFAST: cells found at iniThFAST
    next to cells found only at minThFAST."""
    rng = _rng(w, h, seed, 5)
    img = np.full((h, w), 100, np.uint8)
    ys, xs = np.mgrid[2:h:6, 2:w:6]
    low = rng.integers(0, 2, ((h + 36) // 37, (w + 36) // 37)).astype(bool)[ys // 37, xs // 37]
    hi = rng.integers(8, 28, ys.shape)
    lo = rng.integers(8, 21, ys.shape)
    img[ys, xs] = 100 + np.where(low, lo, hi)
    return img


def blank_but_one(w, h, seed):
    """One 255 dot on 0."""
    img = np.zeros((h, w), np.uint8)
    img[h // 2 + 1, w // 2 + 3] = 255
    return img


def quadrant(w, h, seed):
    """Corners in the bottom-right quarter only."""
    img = np.zeros((h, w), np.uint8)
    src = dots_varied(w, h, seed + 1)
    img[h // 2:, w // 2:] = src[h // 2:, w // 2:]
    return img


# The extreme keypoint positions of level 0: a cell ROI starts at the 16-pixel
# border and FAST leaves a 3-pixel frame inside it, so x runs over
# [19, w - 20] and y over [19, h - 20].
RING_LO = BORDER + 3


def ring_positions(w, h):
    lo, xh, yh = RING_LO, w - 1 - RING_LO, h - 1 - RING_LO
    return [(lo, lo), (w // 2, lo), (xh, lo), (lo, h // 2), (xh, h // 2), (lo, yh), (w // 2, yh), (xh, yh)]


def ring_dots(w, h, seed):
    """255 dots on 0 at the four corners and the four edge midpoints of the
    rectangle of extreme keypoint positions, and four weaker interior dots:
    two of 128, and two of 8, found only at minThFAST, which the blur rounds
    away (56 * 56 * 8 / 65536 < 0.5): a flat blurred patch, every rBRIEF test
    comparing equal values."""
    img = np.zeros((h, w), np.uint8)
    for x, y in ring_positions(w, h):
        img[y, x] = 255
    for (fx, fy), v in zip(((0.3, 0.3), (0.7, 0.35), (0.35, 0.7), (0.72, 0.68)), (128, 8, 8, 128)):
        img[int(fy * h), int(fx * w)] = v
    return img


def checker_sat(w, h, seed):
    """0 / 255 blocks of 5 pixels."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // 5) + (xx // 5)) & 1) * 255).astype(np.uint8)


def patchwork(w, h, seed):
    """Tiles of noise, dots_low, discs and blank in bands 67 pixels high, cut
    at widths that are no multiple of a cell: every other band holds one noise
    tile 0.62 w wide (alternately at the left and the right end), the rest are
    narrow tiles of all four kinds."""
    src = [noise(w, h, seed + 11), dots_low(w, h, seed + 12), discs(w, h, seed + 13), np.zeros((h, w), np.uint8)]
    widths = [29, 47, 31, 53, 37, 43]
    img = np.zeros((h, w), np.uint8)
    big = int(0.62 * w) + 3
    for b, y0 in enumerate(range(0, h, 67)):
        y1 = min(y0 + 67, h)
        cuts, kinds, x, k = [], [], 0, b
        while x < w:
            cuts.append(x)
            kinds.append(k % 4)
            x += widths[k % len(widths)]
            k += 1
        cuts.append(w)
        if b % 2 == 0:
            lo, hi = (0, big) if b % 4 == 0 else (w - big, w)
        for i, kind in enumerate(kinds):
            img[y0:y1, cuts[i]:cuts[i + 1]] = src[kind][y0:y1, cuts[i]:cuts[i + 1]]
        if b % 2 == 0:
            img[y0:y1, lo:hi] = src[0][y0:y1, lo:hi]
    return img


FAMILIES = {"noise": noise, "discs": discs, "dots_equal": dots_equal, "dots_varied": dots_varied,
            "dots_low": dots_low, "blank_but_one": blank_but_one, "quadrant": quadrant, "ring_dots": ring_dots,
            "checker_sat": checker_sat, "patchwork": patchwork}


def depth_zeros(w, h):
    return np.zeros((h, w), np.uint16)


def depth_max(w, h):
    return np.full((h, w), 65535, np.uint16)


def depth_one(w, h):
    return np.ones((h, w), np.uint16)


def depth_ramp(w, h):
    return (np.arange(w * h, dtype=np.int64) % 65536).astype(np.uint16).reshape(h, w)


DEPTHS = {"zeros": depth_zeros, "max": depth_max, "one": depth_one, "ramp": depth_ramp}


def ulp32(v):
    """The float32 spacing at |v| (v float64)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F32)).astype(np.float64)


def assert_geometry(kun, xyz, ur, kx, ky, depth, calib, what):
    """Float32 keypoint geometry against geometry_ref:
    kun within 1 float32 ulp (a double computation rounded once); Z within
    1 ulp; X, Y within 5 * 2^-24 relative of the float64 value computed from the
    given kun and Z (three float32 operations and the rounded 1 / f); ur within
    2^-24 (2 |mbf / z| + |ur|); xyz = 0 and ur = -1 exactly where the depth is 0."""
    kun = np.asarray(kun, F32)
    xyz = np.asarray(xyz, F32)
    ur = np.asarray(ur, F32)
    un, z, _, _, _ = geometry_ref(kx, ky, depth, calib)
    assert kun.shape == un.shape, f"{what}: {kun.shape} undistorted keypoints vs {un.shape}"
    if kun.shape[0] == 0:
        return
    err = np.abs(kun.astype(np.float64) - un)
    assert (err <= ulp32(un)).all(), f"{what}: kun off by {(err / ulp32(un)).max():.2f} ulp"
    has = z > 0
    assert (xyz[~has] == 0).all() and (ur[~has] == -1).all(), f"{what}: keypoints without depth"
    if not has.any():
        return
    g = xyz[has].astype(np.float64)
    zz = z[has]
    ez = np.abs(g[:, 2] - zz)
    assert (ez <= ulp32(zz)).all(), f"{what}: Z off by {(ez / ulp32(zz)).max():.2f} ulp"
    cx, cy, fx, fy, mbf = (float(F32(getattr(calib, k))) for k in ("cx", "cy", "fx", "fy", "mbf"))
    ku = kun[has].astype(np.float64)
    for i, (cc, ff, name) in enumerate(((cx, fx, "X"), (cy, fy, "Y"))):
        ref = (ku[:, i] - cc) * g[:, 2] / ff
        e = np.abs(g[:, i] - ref)
        assert (e <= 5 * 2.0 ** -24 * np.abs(ref)).all(), \
            f"{what}: {name} off by {(e / np.maximum(np.abs(ref), 1e-300)).max() * 2 ** 24:.2f} x 2^-24 relative"
    q = mbf / g[:, 2]
    ref = ku[:, 0] - q
    e = np.abs(ur[has].astype(np.float64) - ref)
    assert (e <= 2.0 ** -24 * (2 * np.abs(q) + np.abs(ref))).all(), f"{what}: ur error {e.max()}"


def scaled_keypoints(level, x, y, scale):
    """operator()'s keypoint of a retained key (x, y relative to the border) on
    `level`: (float32 x, float32 y, size) (orbextractor.cpp:731-740, 805-811)."""
    px = (np.asarray(x, np.int64) + BORDER).astype(F32)
    py = (np.asarray(y, np.int64) + BORDER).astype(F32)
    if level != 0:
        px, py = px * F32(scale), py * F32(scale)
    return px, py, float(int(F32(31) * F32(scale)))


def segments(cells, wcell, seg_cells=8, row_bytes=272):
    """k_fast_seg's segments of one level, restating odo_geometry.cpp build_geometry: each
    cell row's ncj cells in nseg = ceil(ncj / kmax) even runs, kmax = min(8,
    (272 - 15 - 6) / wCell), run sg = cells [ncj sg / nseg, ncj (sg + 1) / nseg)
    of the row. Returns a list of index arrays into `cells`."""
    out = []
    if cells.size == 0:
        return out
    kmax = min(seg_cells, (row_bytes - 15 - 6) // wcell)
    for i in np.unique(cells["i"]):
        row = np.nonzero(cells["i"] == i)[0]
        ncj = row.size
        nseg = (ncj + kmax - 1) // kmax
        for sg in range(nseg):
            out.append(row[ncj * sg // nseg:ncj * (sg + 1) // nseg])
    return out
