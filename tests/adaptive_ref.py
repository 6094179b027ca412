"""Independent model of Extractor(FAST, ORB, ADAPTIVE)'s detection stage in
plain numpy / Python, and the crafted inputs of the ADAPTIVE edge tests.

Nothing here is derived from oracle/orb_ref.cpp: the pieces are written from
the documented behaviour of what the reference calls.

* cv::FAST(roi, t, nonmax) as a thresholded, threshold-free S map (s_map,
  model_fast);
* VideoGridAdaptedFeatureDetector's cell ROIs (cell_geometry), keepStrongest
  and the aggregation in grid order;
* VideoDynamicAdaptedFeatureDetector::detect over DetectorAdjuster
  (chain_step), with a trace of the branches that ran;
* libstdc++'s std::nth_element: __introselect with its depth-limit fallback
  (__heap_select(first, nth + 1, last), then iter_swap(first, nth)) and the
  final __insertion_sort (introselect_model);
* cv::KeyPointsFilter::retainBest: nth_element, then the bidirectional
  std::partition of the tail on response >= ambiguous (retain_best_model);
* cv::ORB::compute's runByImageBorder(31).

AdaptiveModel strings them together: (gray, params, thresholds) -> keypoints
(x, y, response, in order), the threshold every cell used, the new persistent
thresholds, the chain trace and whether any selection hit introselect's depth
limit.

The crafted inputs are dot images: one pixel of value v on a zero background
has S = v exactly and S = 0 everywhere else (the same inverted on 255), dots
8 px apart do not interact, so every cell's survivor list and its count above
every threshold are set by hand. cases() lists the FAST-inner cases shared by
tests/test_adaptive_ref.py (model == oracle, CPU) and
tests/test_adaptive_edges_gpu.py (GPU == oracle).
"""
import numpy as np

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

BRANCHES = ("tooFew", "tooMany", "good", "clamp_min", "clamp_max", "escape_iters", "t_clamp_255")


def s_map(img):
    """S(p) for p in [3,h-3)x[3,w-3), 0 elsewhere (int32)."""
    h, w = img.shape
    S = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return S
    v = img[3:h - 3, 3:w - 3].astype(np.int32)
    d = np.stack([v - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) for dx, dy in CIRCLE])
    best = np.zeros_like(v)
    for k in range(16):
        arc = d[[(k + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    S[3:h - 3, 3:w - 3] = best
    return S


def model_fast(S_roi, t):
    """Keypoints of cv::FAST(roi, t, nonmax) from the ROI's S map (row-major)."""
    rows, cols = S_roi.shape
    R = np.zeros_like(S_roi)
    R[3:rows - 3, 3:cols - 3] = S_roi[3:rows - 3, 3:cols - 3]  # detection region only
    P = np.pad(R, 1)
    nb = np.stack([P[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                   if dy or dx]).max(0)
    keep = (R > t) & (R >= 2) & (R > nb)  # score S-1 >= 1: a 0 score never passes the NMS
    ys, xs = np.nonzero(keep)
    return xs, ys, R[ys, xs] - 1


def cell_geometry(w, h, p):
    cells = []
    for i in range(p.grid_rows):
        rs, re = max(i * h // p.grid_rows - p.edge_threshold, 0), min(h, (i + 1) * h // p.grid_rows + p.edge_threshold)
        for j in range(p.grid_cols):
            cs, ce = max(j * w // p.grid_cols - p.edge_threshold, 0), min(w, (j + 1) * w // p.grid_cols + p.edge_threshold)
            cells.append((rs, re, cs, ce))
    return cells


def chain_step(thresh, count_above, p, trace=None):
    """VideoDynamicAdaptedFeatureDetector::detect replayed on count_above[t].
    trace: a set that receives the names (BRANCHES) of the branches that ran."""
    tr = trace if trace is not None else set()
    it = p.escape_iters
    while True:
        if int(thresh) > 255:
            tr.add("t_clamp_255")
        t = min(max(int(thresh), 0), 255)
        n = int(count_above[t])
        if n < p.cell_min:
            tr.add("tooFew")
            if thresh * p.decrease_factor < p.min_thresh:
                tr.add("clamp_min")
            thresh = max(thresh * p.decrease_factor, p.min_thresh)
        elif n > p.cell_max:
            tr.add("tooMany")
            if thresh * p.increase_factor > p.max_thresh:
                tr.add("clamp_max")
            thresh = min(thresh * p.increase_factor, p.max_thresh)
            break
        else:
            tr.add("good")
            break
        it -= 1
        if not (it > 0 and p.min_thresh < thresh < p.max_thresh):
            if it <= 0 and p.min_thresh < thresh < p.max_thresh:
                tr.add("escape_iters")
            break
    return thresh, t


# ---- std::nth_element (libstdc++): introselect, single range per level,
# parallel Hoare partition; heap select at the depth limit
def _adjust_heap(a, first, hole, length, value, key):
    """std::__adjust_heap followed by its __push_heap."""
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if key(a[first + child]) < key(a[first + child - 1]):
            child -= 1
        a[first + hole] = a[first + child]
        hole = child
    if length % 2 == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        a[first + hole] = a[first + child - 1]
        hole = child - 1
    while hole > top:
        parent = (hole - 1) // 2
        if not key(a[first + parent]) < key(value):
            break
        a[first + hole] = a[first + parent]
        hole = parent
    a[first + hole] = value


def heap_select(a, first, middle, last, key):
    """std::__heap_select: a max-heap of [first, middle); every later element
    smaller than the top replaces it (__pop_heap(first, middle, i))."""
    length = middle - first
    if length >= 2:
        for parent in range((length - 2) // 2, -1, -1):
            _adjust_heap(a, first, parent, length, a[first + parent], key)
    for i in range(middle, last):
        if key(a[i]) < key(a[first]):
            v = a[i]
            a[i] = a[first]
            _adjust_heap(a, first, 0, length, v, key)


def introselect_model(a, nth, key, info=None):
    """std::nth_element(a, a + nth, end) with comp(x, y) = key(x) < key(y).
    info: a dict whose "depth_limit" is set when the fallback ran; with
    "stop_at_limit" set the call returns there, before the fallback."""
    a = list(a)
    n = len(a)
    if n == 0 or nth == n:
        return a
    first, last = 0, n
    depth = 2 * (n.bit_length() - 1)
    while last - first > 3:
        if depth == 0:
            if info is not None and info.get("stop_at_limit"):
                info["depth_limit"] = True
                return a
            heap_select(a, first, nth + 1, last, key)
            a[first], a[nth] = a[nth], a[first]
            if info is not None:
                info["depth_limit"] = True
            return a
        depth -= 1
        mid = first + (last - first) // 2
        x, y, z = first + 1, mid, last - 1
        kx, ky, kz = key(a[x]), key(a[y]), key(a[z])
        if kx < ky:
            m = y if ky < kz else (z if kx < kz else x)
        else:
            m = x if kx < kz else (z if ky < kz else y)
        a[first], a[m] = a[m], a[first]
        pk = key(a[first])
        L = [j for j in range(first + 1, last) if key(a[j]) >= pk]
        R = [j for j in range(last - 1, first, -1) if key(a[j]) <= pk]
        ks = sum(1 for k in range(min(len(L), len(R))) if L[k] < R[k])
        for k in range(ks):
            a[L[k]], a[R[k]] = a[R[k]], a[L[k]]
        cut = L[ks] if ks < len(L) else last
        if ks > 0:
            cut = min(cut, R[ks - 1])
        if cut <= nth:
            first = cut
        else:
            last = cut
    for i in range(first + 1, last):  # __insertion_sort
        v = a[i]
        if key(v) < key(a[first]):
            a[first + 1:i + 1] = a[first:i]
            a[first] = v
        else:
            j = i
            while key(v) < key(a[j - 1]):
                a[j] = a[j - 1]
                j -= 1
            a[j] = v
    return a


def partition_model(a, first, last, pred):
    """libstdc++'s bidirectional std::__partition on a[first:last], in place."""
    while True:
        while True:
            if first == last:
                return first
            if pred(a[first]):
                first += 1
            else:
                break
        last -= 1
        while True:
            if first == last:
                return first
            if not pred(a[last]):
                last -= 1
            else:
                break
        a[first], a[last] = a[last], a[first]
        first += 1


def retain_best_model(a, n_points, resp, info=None):
    """cv::KeyPointsFilter::retainBest(a, n_points) on a list; resp(e) is the
    response."""
    a = list(a)
    if n_points >= 0 and len(a) > n_points:
        if n_points == 0:
            return []
        a = introselect_model(a, n_points, key=lambda e: -resp(e), info=info)
        amb = resp(a[n_points - 1])
        end = partition_model(a, n_points, len(a), lambda e: resp(e) >= amb)
        a = a[:end]
    return a


def run_by_image_border(kps, w, h, b=31):
    """KeyPointsFilter::runByImageBorder: Rect(b, b, w - 2b, h - 2b).contains."""
    if h <= 2 * b or w <= 2 * b:
        return []
    return [k for k in kps if b <= k[0] < w - b and b <= k[1] < h - b]


# packed (score << 24 | y << 12 | x) keys of the GPU selection's debug entry
def score_key(e):
    return 255 - (int(e) >> 24)


def nth_element_packed(keys, nth, info=None):
    return np.array(introselect_model([int(k) for k in keys], nth, score_key, info), np.uint32)


def retain_best_packed(keys, n_points, info=None):
    return np.array(retain_best_model([int(k) for k in keys], n_points, lambda e: e >> 24, info), np.uint32)


class AdaptiveModel:
    """The FAST-inner ADAPTIVE detector with its persistent cell thresholds.
    extract_gray returns a dict: x, y, response (int arrays, in output order),
    t_used (per cell), thresh (the new persistent thresholds, also kept),
    trace (per cell, the set of chain branches that ran), depth_limit (any
    selection of this frame ran the heap-select fallback) and cells (per cell,
    the survivors above the used threshold before keepStrongest, as (x, y,
    response) in image coordinates) and survivors (per cell, every survivor of
    the threshold-free NMS)."""

    def __init__(self, params, thresh=None):
        self.p = params
        nc = params.grid_rows * params.grid_cols
        self.thresh = np.full(nc, params.init_thresh, np.float64) if thresh is None else np.array(thresh, np.float64)

    def extract_gray(self, gray):
        p = self.p
        h, w = gray.shape
        S = s_map(gray)
        max_per_cell = p.max_total_keypoints // (p.grid_rows * p.grid_cols)
        out, t_used, trace, cells_dbg, survivors = [], [], [], [], []
        info = {}
        for c, (rs, re, cs, ce) in enumerate(cell_geometry(w, h, p)):
            xs, ys, resp = model_fast(S[rs:re, cs:ce], 0)
            hist = np.bincount(resp + 1, minlength=257)
            at_least = hist[::-1].cumsum()[::-1]
            above = np.append(at_least[1:], 0)  # above[t] = #{S > t}
            tr = set()
            self.thresh[c], t = chain_step(self.thresh[c], above, p, tr)
            allk = [(int(x) + cs, int(y) + rs, int(r)) for x, y, r in zip(xs, ys, resp)]
            survivors.append(allk)
            kps = [k for k in allk if k[2] + 1 > t]
            cells_dbg.append(list(kps))
            if len(kps) > max_per_cell:  # keepStrongest
                kps = introselect_model(kps, max_per_cell, key=lambda e: -abs(e[2]), info=info)[:max_per_cell]
            out += kps
            t_used.append(t)
            trace.append(tr)
        if len(out) > p.retain_best:  # Extractor::Extract
            out = retain_best_model(out, p.retain_best, lambda e: e[2], info)
        out = run_by_image_border(out, w, h, 31)
        a = np.array(out, np.int64).reshape(-1, 3)
        return dict(x=a[:, 0], y=a[:, 1], response=a[:, 2], t_used=np.array(t_used, np.int32),
                    thresh=self.thresh.copy(), trace=trace, depth_limit=bool(info.get("depth_limit")),
                    cells=cells_dbg, survivors=survivors)


# ---- McIlroy's adversary ("A killer adversary for quicksort", 1999) run
# against introselect_model: values are decided only when a comparison needs
# them, so every partition peels off a constant number of elements.
class _Adversary:
    def __init__(self, ngas, solid):
        self.gas = ngas + len(solid) + 1000  # compares above every solid value
        self.val = [self.gas] * ngas + list(solid)
        self.nsolid = 0
        self.base = (max(solid) + 1) if solid else 0
        self.candidate = 0

    def freeze(self, i):
        self.val[i] = self.base + self.nsolid
        self.nsolid += 1

    def cmp(self, x, y):
        v = self.val
        if v[x] == self.gas and v[y] == self.gas:
            self.freeze(x if x == self.candidate else y)
        if v[x] == self.gas:
            self.candidate = x
        elif v[y] == self.gas:
            self.candidate = y
        return v[x] - v[y]


class _AdvKey:
    __slots__ = ("adv", "i")

    def __init__(self, adv, i):
        self.adv, self.i = adv, i

    def __lt__(self, o):
        return self.adv.cmp(self.i, o.i) < 0

    def __le__(self, o):
        return self.adv.cmp(self.i, o.i) <= 0

    def __ge__(self, o):
        return self.adv.cmp(self.i, o.i) >= 0


def adversary_keys(n, nth, tail_keys=(), ties=False):
    """Packed keys (score << 24 | index) whose first n elements are decided by
    the adversary against introselect_model(., nth): distinct key values
    above every tail key. tail_keys: key values (255 - score) of fixed elements
    that follow the block. nth counts within the whole array.
    ties: the adversary stops at the depth limit and the elements still
    undecided there (never compared with one another, above every decided
    value) share three values, so the heap-select fallback runs on ties."""
    adv = _Adversary(n, list(tail_keys))
    total = n + len(tail_keys)
    info = {"stop_at_limit": True} if ties else None
    introselect_model(range(total), nth, key=lambda i: _AdvKey(adv, i), info=info)
    top = adv.base + adv.nsolid
    for i in range(n):
        if adv.val[i] == adv.gas:
            if ties:
                adv.val[i] = top + i % 3
            else:
                adv.freeze(i)
    kv = np.array(adv.val, np.int64)
    assert kv.max() <= 255 and (ties or len(set(kv[:n].tolist())) == n)
    return (((255 - kv).astype(np.uint32) << 24) | np.arange(total, dtype=np.uint32)).astype(np.uint32)


# ---- dot images
def dots(w, h, pts, inverted=False):
    """A gray image with S = v at every (x, y, v) of pts and S = 0 elsewhere
    (dots at least 8 px apart, or adjacent on purpose)."""
    img = np.zeros((h, w), np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return (255 - img) if inverted else img


def dot_grid(x0, y0, x1, y1, values, step=8):
    """len(values) dots on a step-px lattice filling [x0, x1) x [y0, y1) row
    by row."""
    pts = []
    x, y = x0, y0
    for v in values:
        assert y < y1, "dot_grid: the box is too small"
        pts.append((x, y, int(v)))
        x += step
        if x >= x1:
            x, y = x0, y + step
    return pts


def to_bgr(gray):
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=-1))


def noise(w, h, seed, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def run_offsets(cells, w, h, p, band_rows=16, threads=256):
    """Offsets, within its thread's run, of every survivor of a frame, as
    k_adapt_cand assigns them: a band is band_rows rows of a cell's detection
    region and each thread takes ceil(rows * cw / threads) row-major pixels.
    cells: AdaptiveModel's per-cell `survivors` lists."""
    offs = []
    for (rs, re, cs, ce), kps in zip(cell_geometry(w, h, p), cells):
        r0, r1, c0, c1 = rs + 3, re - 3, cs + 3, ce - 3
        cw = c1 - c0
        for x, y, _ in kps:
            y0 = r0 + (y - r0) // band_rows * band_rows
            rows = min(band_rows, r1 - y0)
            chunk = -(-rows * cw // threads)
            offs.append(((y - y0) * cw + (x - c0)) % chunk)
    return offs


# ---- the crafted FAST-inner cases
class Case:
    """name; params: AdaptiveParams fields off their defaults; frames: gray
    images (n, h, w); start: start thresholds per cell or None; expect: chain
    branches this case is built to run (checked against the model's trace)."""

    def __init__(self, name, params, frames, start=None, expect=()):
        self.name, self.params, self.start, self.expect = name, params, start, tuple(expect)
        self.frames = np.ascontiguousarray(np.asarray(frames, np.uint8))
        self.n, self.h, self.w = self.frames.shape

    def __repr__(self):
        return self.name

    def apply(self, p):
        for k, v in self.params.items():
            setattr(p, k, v)
        return p

    def nlevels(self):
        """ORB pyramid levels to configure: the default 8 where the image
        carries them, else 1 (the FAST-inner ADAPTIVE extractor reads level 0
        only)."""
        return 8 if min(self.w, self.h) >= 240 else 1


def _chain_cases():
    cs = []
    # one cell (1x1, edge 0) of 160x96; dots of value 100 (S > 20) and 10
    # (2 < S <= 20): exact counts at the start threshold 20 and below it
    base = dict(grid_rows=1, grid_cols=1, edge_threshold=0, max_total_keypoints=400, cell_min=6, cell_max=9,
                retain_best=-1)

    def img(n_hi, n_lo=0):
        return dots(160, 96, dot_grid(34, 34, 126, 62, [100] * n_hi + [10] * n_lo))

    # n = cell_min-1, cell_min, cell_max, cell_max+1 at the used threshold
    cs.append(Case("count_min_minus_1", base, [img(5, 1)], expect=("tooFew", "good")))
    cs.append(Case("count_min", base, [img(6, 3)], expect=("good",)))
    cs.append(Case("count_max", base, [img(9, 3)], expect=("good",)))
    cs.append(Case("count_max_plus_1", base, [img(10)], expect=("tooMany",)))
    cs.append(Case("min_eq_max_cells", dict(base, cell_min=7, cell_max=7), [img(6, 1), img(7, 5), img(8)],
                   expect=("tooFew", "good", "tooMany")))
    cs.append(Case("escape_1", dict(base, escape_iters=1), [img(2, 2), img(2, 2), img(7)],
                   expect=("tooFew", "escape_iters", "good")))
    cs.append(Case("escape_5_exhausted", base, [img(1), img(1)], expect=("tooFew", "escape_iters")))
    cs.append(Case("clamp_min_first_step", base, [img(1), img(7)], start=[2.5], expect=("tooFew", "clamp_min")))
    cs.append(Case("min_eq_max_thresh", dict(base, min_thresh=10.0, max_thresh=10.0, init_thresh=10.0),
                   [img(1), img(12), img(7)], expect=("tooFew", "clamp_min", "tooMany", "clamp_max", "good")))
    # min_thresh 0: thresholds 1 and 0 in use (dots of S = 2 count at t = 1
    # and t = 0; S = 1 never survives the NMS)
    lo5, lo6 = (dots(160, 96, dot_grid(34, 34, 126, 62, [2] * k + [1] * 4)) for k in (5, 6))
    cs.append(Case("min_thresh_0", dict(base, min_thresh=0.0), [lo6, lo5, lo6], start=[1.2],
                   expect=("good", "tooFew", "escape_iters")))
    # 250 -> tooMany -> 325: the next frame uses t = 255 and finds nothing
    hi = dots(160, 96, dot_grid(34, 34, 126, 62, [255] * 6 + [252] * 6))
    cs.append(Case("thresh_above_255", base, [hi, hi], start=[250.0], expect=("tooMany", "t_clamp_255", "tooFew")))
    # 17 and 33 small frames alternating dense / sparse over a 2x2 grid: the
    # chain moves on both sides of the 16-frame chunk boundary
    g = dict(grid_rows=2, grid_cols=2, edge_threshold=0, max_total_keypoints=400, cell_min=4, cell_max=6,
             retain_best=-1)

    def quad(vals):
        pts = []
        for (x0, y0), v in zip(((8, 8), (72, 8), (8, 72), (72, 72)), vals):
            pts += dot_grid(x0, y0, x0 + 48, y0 + 48, v)
        return dots(128, 128, pts)

    # 16 dots per cell with a spread of values: a dense frame has 4..6 dots
    # above t for t around 100..130 (times 1 + 0.15 k in cell k), a sparse one
    # for t around 31..39, so no threshold suits both and the chain moves on
    # every frame
    dense = [[int((10 + 10 * i) * (1 + 0.15 * k)) for i in range(16)] for k in range(4)]
    sparse = [[int((4 + 3 * i) * (1 + 0.15 * k)) for i in range(16)] for k in range(4)]
    for nf in (17, 33):
        fr = [quad(dense if f % 2 == 0 else sparse) for f in range(nf)]
        cs.append(Case(f"alternating_{nf}", g, fr, expect=("tooFew", "tooMany", "good")))
    return cs


def _geometry_cases():
    cs = []
    # 1x1 grid, runs longer than 32 px (520 and 640 wide); 640x480: more than
    # 4096 survivors above the used threshold (global-scratch selection)
    one = dict(grid_rows=1, grid_cols=1)
    cs.append(Case("wide_520", one, noise(520, 70, 11), start=[40.0]))
    cs.append(Case("wide_640", one, noise(640, 480, 12), start=[2.0]))
    # grid shapes on noise (every cell tooMany, keepStrongest binds) and dots
    for r, c, w, h in ((1, 4, 322, 96), (4, 1, 96, 322), (2, 5, 323, 131)):
        cs.append(Case(f"grid_{r}x{c}_noise", dict(grid_rows=r, grid_cols=c, max_total_keypoints=40 * r * c,
                                                   cell_min=10, cell_max=30, retain_best=35 * r * c),
                       noise(w, h, 20 + r * c, 2)))
    # 8x8 = 64 cells of 20..21 x 9..10 px (164x76 is no multiple of the grid),
    # edge 0: detection regions 14..15 x 3..4 px; edge 2: overlapping
    for e in (0, 2):
        cs.append(Case(f"grid_8x8_edge{e}", dict(grid_rows=8, grid_cols=8, edge_threshold=e, max_total_keypoints=128,
                                                 cell_min=1, cell_max=2, retain_best=-1, min_thresh=0.0),
                       noise(164, 76, 30 + e, 2), start=np.linspace(0.5, 60, 64)))
    # edges 0 and 60 on a 2x2 grid of 240x240: dots in the overlap of two and
    # of four cells appear once per cell that sees them; dots on the first /
    # last row / column of a detection region and one pixel outside
    for e in (0, 60):
        p = dict(grid_rows=2, grid_cols=2, edge_threshold=e, max_total_keypoints=400, cell_min=1, cell_max=50,
                 retain_best=-1)
        pts = [(120, 120, 90), (112, 40, 80), (128, 200, 70), (40, 120, 60), (200, 112, 50)]
        # cell (0, 0) = [0, 120 + e)^2: last row / column of its detection region
        r1 = c1 = 120 + e - 3
        pts += [(c1 - 1, 64, 101), (c1, 72, 102), (64, r1 - 1, 103), (72, r1, 104), (c1 - 1, r1 - 1, 105)]
        # a larger neighbour one pixel outside the region must not suppress
        pts += [(88, r1 - 1, 80), (88, r1, 81), (c1 - 1, 96, 82), (c1, 96, 83)]
        # cell (1, 1) = [120 - e, 240)^2: first row / column
        r0 = c0 = 120 - e + 3
        pts += [(c0, 160, 111), (c0 - 1, 168, 112), (160, r0, 113), (168, r0 - 1, 114), (c0, r0, 115)]
        pts += [(184, r0, 84), (184, r0 - 1, 85), (c0, 192, 86), (c0 - 1, 192, 87)]
        # the image's own 3 px margin
        pts += [(3, 48, 120), (2, 56, 121), (48, 3, 122), (56, 2, 123), (236, 80, 124), (237, 88, 125),
                (80, 236, 126), (88, 237, 127)]
        assert len({(x, y) for x, y, _ in pts}) == len(pts)
        cs.append(Case(f"overlap_edge{e}", p, [dots(240, 240, pts), dots(240, 240, pts, inverted=True)]))
    # equal-value neighbours (the strict maximum keeps neither), v / v+1 pairs,
    # the values 1, 2, 254, 255, and the image-border filter at 30 / 31 and
    # w-32 / w-31 (likewise h) on 160x128
    p = dict(grid_rows=1, grid_cols=2, edge_threshold=31, max_total_keypoints=400, cell_min=1, cell_max=100,
             retain_best=-1, min_thresh=0.0, init_thresh=0.5)
    pts = [(40, 40, 50), (41, 40, 50), (56, 40, 50), (56, 41, 50), (72, 40, 50), (73, 41, 50), (88, 40, 50),
           (87, 41, 50), (104, 40, 50), (105, 40, 51), (120, 40, 51), (120, 41, 50),
           (40, 56, 1), (48, 56, 2), (56, 56, 254), (64, 56, 255), (72, 56, 3)]
    w, h = 160, 128
    pts += [(30, 64, 90), (31, 72, 91), (w - 32, 64, 92), (w - 31, 72, 93), (64, 30, 94), (72, 31, 95),
            (64, h - 32, 96), (72, h - 31, 97)]
    frames = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):  # one corner combination per frame: the dots stay apart
        q = pts + [(30 + dx, 30 + dy, 61), (w - 32 + dx, 30 + dy, 62), (30 + dx, h - 32 + dy, 63),
                   (w - 32 + dx, h - 32 + dy, 64)]
        assert len({(x, y) for x, y, _ in q}) == len(q)
        frames.append(dots(w, h, q))
    frames.append(255 - frames[0])
    cs.append(Case("ties_values_border", p, frames))
    # w or h <= 62: runByImageBorder(31) leaves nothing
    small = dict(grid_rows=1, grid_cols=1, edge_threshold=0, max_total_keypoints=50, cell_min=1, cell_max=40,
                 retain_best=-1)
    cs.append(Case("narrow_62", small, [dots(62, 100, dot_grid(8, 8, 54, 92, [90] * 20))]))
    cs.append(Case("low_62", small, [dots(100, 62, dot_grid(8, 8, 92, 54, [90] * 20))]))
    # max_per_cell 1 and 2: keepStrongest on a 2x2 grid with ties at the top
    for mpc in (1, 2):
        p = dict(grid_rows=2, grid_cols=2, edge_threshold=0, max_total_keypoints=4 * mpc + 3, cell_min=1, cell_max=100,
                 retain_best=-1)
        pts = []
        for k, (x0, y0) in enumerate(((34, 34), (130, 34), (34, 130), (130, 130))):
            pts += dot_grid(x0, y0, x0 + 56, y0 + 56, [60, 80, 80, 70, 80, 30, 90 if k == 3 else 80][:4 + k])
        cs.append(Case(f"max_per_cell_{mpc}", p, [dots(240, 240, pts)]))
    # retain_best around the assembled count (12 = 4 cells x 3), ties at the
    # boundary score
    pts = []
    for k, (x0, y0) in enumerate(((34, 34), (130, 34), (34, 130), (130, 130))):
        pts += dot_grid(x0, y0, x0 + 56, y0 + 56, [70, 50 + k, 70 - k, 40, 90])
    for rb in (-1, 0, 1, 11, 12, 13, 5, 9):
        p = dict(grid_rows=2, grid_cols=2, edge_threshold=0, max_total_keypoints=12, cell_min=1, cell_max=100,
                 retain_best=rb)
        cs.append(Case(f"retain_best_{rb}", p, [dots(240, 240, pts)]))
    return cs


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _chain_cases() + _geometry_cases()
    return _CASES


def killer_cases():
    """(name, keys, nth, must_hit): selection inputs; must_hit: the model must
    report the depth-limit fallback."""
    out = []
    for n in (40, 64, 250):
        for nth in (n - 1, n // 2):
            out.append((f"killer_{n}_{nth}", adversary_keys(n, nth), nth, True))
    for n in (64, 250):  # the fallback itself on heavy ties
        for nth in (n - 1, n // 2):
            out.append((f"killer_ties_{n}_{nth}", adversary_keys(n, nth, ties=True), nth, True))
    rng = np.random.default_rng(16)
    tail = rng.integers(0, 3, 2750)  # heavy ties: three scores above the block's
    for nth in (2999, 2750 + 125):
        out.append((f"embedded_{nth}", adversary_keys(250, nth, tail), nth, True))
    for n in (1, 2, 3, 4):
        eq = ((np.uint32(77) << 24) | np.arange(n, dtype=np.uint32)).astype(np.uint32)
        for nth in range(1, n + 1):
            out.append((f"equal_{n}_{nth}", eq, nth, False))
    return out
