"""CPU: a model of k_octree's phase 1 restated over one key histogram.

While every node with more than one key is divided (DistributeOctTree's first
loop), a child's box depends on its parent's box alone, so a key's quadrant
path through the first D levels is a function of its own coordinates and the
count of every node down to depth D is a sum over one histogram of depth-D
path codes. hist_octree() restates the first D iterations that way, as the
kernel does: path codes, the histogram pyramid, the list bookkeeping of each
depth from the counts (push-front order, creation seq, the sorted-list
entries, the two exits), a table of list positions by path prefix, one lookup
per key, and then the reference's loops from the state reached. It must return
extract_ref.octree_ref's indices, in order, for D = 0..4, and the inputs must
reach every way out of the restated part.
"""
import math

import numpy as np
import pytest

import extract_ref as R
from test_extract_ref import CASES, IDS, analysis, nfeatures_of, octree_of
from test_octree_key_counts import H, W, dots

F32 = np.float32
DS = (0, 1, 2, 3, 4)


class _Node:
    __slots__ = ("x0", "y0", "x1", "y1", "cnt", "seq", "depth", "path", "keys")

    def __init__(self, x0, y0, x1, y1, cnt, seq, depth=-1, path=-1, keys=None):
        self.x0, self.y0, self.x1, self.y1, self.cnt, self.seq = x0, y0, x1, y1, cnt, seq
        self.depth, self.path, self.keys = depth, path, keys


def _children_boxes(nd):
    hx, hy = (nd.x1 - nd.x0 + 1) >> 1, (nd.y1 - nd.y0 + 1) >> 1  # ceil(half), as DivideNode
    mx, my = nd.x0 + hx, nd.y0 + hy
    return [(nd.x0, nd.y0, mx, my), (mx, nd.y0, nd.x1, my), (nd.x0, my, mx, nd.y1), (mx, my, nd.x1, nd.y1)]


def hist_octree(x, y, resp, min_x, max_x, min_y, max_y, n_want, D, trace=None):
    """octree_ref's result with the first D phase-1 iterations taken from the
    histogram. trace, if a dict, receives how the restated part ended."""
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    resp = np.asarray(resp, F32)
    tr = {} if trace is None else trace
    n_ini = R._c_round(float(F32(max_x - min_x) / F32(max_y - min_y)))
    hx = F32(max_x - min_x) / F32(n_ini)
    bx0 = np.array([int(hx * F32(i)) for i in range(n_ini)], np.int64)
    bx1 = np.array([int(hx * F32(i + 1)) for i in range(n_ini)], np.int64)
    # ---- path codes: the root, then D descents of the key's own box
    root = (x.astype(F32) / hx).astype(np.int64)
    X0, X1 = bx0[root], bx1[root]
    Y0, Y1 = np.zeros_like(x), np.full_like(x, max_y - min_y)
    code = root.copy()
    for _ in range(D):
        mx, my = X0 + ((X1 - X0 + 1) >> 1), Y0 + ((Y1 - Y0 + 1) >> 1)
        right, low = x >= mx, y >= my
        X0, X1 = np.where(right, mx, X0), np.where(right, X1, mx)
        Y0, Y1 = np.where(low, my, Y0), np.where(low, Y1, my)
        code = code * 4 + right + 2 * low
    # ---- the pyramid: counts of depth d are sums of four of depth d + 1
    hist = [None] * (D + 1)
    hist[D] = np.bincount(code, minlength=n_ini * 4 ** D)
    for d in range(D - 1, -1, -1):
        hist[d] = hist[d + 1].reshape(-1, 4).sum(1)
    # ---- list bookkeeping per depth, from the counts alone
    nodes = [_Node(bx0[i], 0, bx1[i], max_y - min_y, int(hist[0][i]), i, 0, i) for i in range(n_ini)
             if hist[0][i] > 0]
    tr["n_ini"], tr["root_counts"] = n_ini, [int(c) for c in hist[0]]
    seq, d, finish, phase, to_sort = n_ini, 0, False, 1, []
    while d < D and not finish and phase == 1:
        S = len(nodes)
        pushed, kept, to_sort = [], [], []
        for nd in nodes:
            if nd.cnt <= 1:
                kept.append(nd)
                continue
            for q, box in enumerate(_children_boxes(nd)):
                c = int(hist[d + 1][nd.path * 4 + q])
                if c > 0:
                    ch = _Node(*box, c, seq, d + 1, nd.path * 4 + q)
                    seq += 1
                    pushed.append(ch)
                    if c > 1:
                        to_sort.append(ch)
        nodes = pushed[::-1] + kept
        if len(nodes) >= n_want or len(nodes) == S:
            finish = True
            tr["finish"] = "quota" if len(nodes) >= n_want else "same size"
        elif len(nodes) + 3 * len(to_sort) > n_want:
            phase = 2
        d += 1
    tr["dstar"], tr["hist_exit"] = d, "finish" if finish else "phase 2" if phase == 2 else "D"
    # ---- positions by path prefix, and each key's node
    postab = [np.full(len(h), -1, np.int64) for h in hist]
    for pos, nd in enumerate(nodes):
        postab[nd.depth][nd.path] = pos
    node = np.full(len(x), -1, np.int64)
    for dd in range(d + 1):
        prefix = code >> (2 * (D - dd))
        here = (node < 0) & ((hist[dd][prefix] == 1) | (dd == d))
        node[here] = postab[dd][prefix[here]]
    assert (node >= 0).all()
    for pos, nd in enumerate(nodes):
        nd.keys = np.nonzero(node == pos)[0]
        assert nd.keys.size == nd.cnt
    # ---- the reference's loops from here
    state = {"seq": seq}

    def divide(nd):
        boxes = _children_boxes(nd)
        k = nd.keys
        quad = (x[k] >= boxes[3][0]) + 2 * (y[k] >= boxes[3][1])
        return [_Node(*box, int((quad == q).sum()), -1, keys=k[quad == q]) for q, box in enumerate(boxes)]

    def stamp(nd):
        nd.seq = state["seq"]
        state["seq"] += 1
        return nd

    tr["p1_iters"], tr["p2_iters"] = d, 0
    while not finish and phase == 1:
        S = len(nodes)
        pushed, kept, to_sort = [], [], []
        for nd in nodes:
            if nd.cnt <= 1:
                kept.append(nd)
                continue
            for c in divide(nd):
                if c.cnt > 0:
                    pushed.append(stamp(c))
                    if c.cnt > 1:
                        to_sort.append(c)
        nodes = pushed[::-1] + kept
        tr["p1_iters"] += 1
        if len(nodes) >= n_want or len(nodes) == S:
            finish = True
            tr["finish"] = "quota" if len(nodes) >= n_want else "same size"
        elif len(nodes) + 3 * len(to_sort) > n_want:
            phase = 2
    tr["switched"] = phase == 2
    while not finish:
        S = len(nodes)
        order = sorted(to_sort, key=lambda c: (c.cnt, c.seq))
        to_sort = []
        for nd in reversed(order):
            for c in divide(nd):
                if c.cnt > 0:
                    nodes.insert(0, stamp(c))
                    if c.cnt > 1:
                        to_sort.append(c)
            nodes.remove(nd)
            if len(nodes) >= n_want:
                break
        tr["p2_iters"] += 1
        if len(nodes) >= n_want or len(nodes) == S:
            finish = True
            tr["finish"] = "quota" if len(nodes) >= n_want else "same size"
    out = []
    for nd in nodes:
        r = resp[nd.keys]
        out.append(int(nd.keys[int(np.argmax(r))]))  # argmax: the first maximum
    return np.array(out, np.int64)


_SEEN = set()


def note(tr, D):
    """The ways out of the restated part that a run took."""
    if D == 0:
        return
    ex, ds = tr["hist_exit"], tr["dstar"]
    if ex == "finish" and ds < D:
        _SEEN.add("finish below D")
    if ex == "phase 2" and ds < D:
        _SEEN.add("phase 2 below D")
    if ex == "phase 2" and ds == D:
        _SEEN.add("phase 2 at D")
    if ex == "D" and tr["switched"]:
        _SEEN.add("past D, then phase 2")
    if ex == "D" and not tr["switched"] and tr["finish"] == "same size":
        _SEEN.add("past D, then same size")
    if tr["p2_iters"] > 1:
        _SEEN.add("phase 2 twice")
    if tr["n_ini"] >= 2 and D < 4 and ds > 0:
        _SEEN.add("nIni >= 2, D < 4")
    rc = tr["root_counts"]
    if 1 in rc and max(rc) > 1 and ds > 0:
        _SEEN.add("single-key root beside a dividing root")


def check(x, y, r, lw, lh, quota, want, what):
    for D in DS:
        tr = {}
        got = hist_octree(x, y, r, 16, lw - 16, 16, lh - 16, quota, D, tr)
        assert np.array_equal(got, want), f"{what} D {D}: {len(got)} vs {len(want)} keys, or their order"
        note(tr, D)


@pytest.mark.parametrize("family,w,h", CASES, ids=IDS)
def test_model_equals_octree_ref(family, w, h):
    _, levels, fast = analysis(family, w, h)
    for nf in nfeatures_of(w, h):
        quota = R.level_tables(w, h, nf)[3]
        for l, (lv, (x, y, r, _)) in enumerate(zip(levels, fast)):
            if len(x):
                check(x, y, r, lv.shape[1], lv.shape[0], quota[l], octree_of(family, w, h, nf)[l][0],
                      f"nfeatures {nf} level {l}")


# dot images at level 0 (their pyramids are not needed: the octree of one level)
DOTS = [(k, nf) for k in (2, 255, 600, 2047) for nf in (60, 800, 1500)] + [(100, 800)]


@pytest.mark.parametrize("k,nf", DOTS)
def test_model_on_dots(k, nf):
    x, y, r, _ = R.fast_level_ref(dots(k))
    assert len(x) == k
    q = R.level_tables(W, H, nf)[3][0]
    check(x, y, r, W, H, q, R.octree_ref(x, y, r, 16, W - 16, 16, H - 16, q), f"dots({k}) nfeatures {nf}")


def test_sparse_dots_divide_to_single_keys():
    """dots(100) at 800 features stays below the quota: phase 1 runs until
    every node holds one key and ends with newSize == S, past D."""
    x, y, r, _ = R.fast_level_ref(dots(100))
    q = R.level_tables(W, H, 800)[3][0]
    tr = {}
    keep = hist_octree(x, y, r, 16, W - 16, 16, H - 16, q, 4, tr)
    assert len(keep) == 100 < q and tr["hist_exit"] == "D" and tr["finish"] == "same size" and tr["p1_iters"] > 4


def three_roots(n, lone):
    """Distinct uniform keys on 532x232 (three root nodes); with `lone`, the
    first root node holds exactly one of them."""
    rng = np.random.default_rng(11)
    x, y = rng.integers(170 if lone else 3, 497, n), rng.integers(3, 197, n)
    if lone:
        x[0], y[0] = 40, 100
    _, i = np.unique(x * 4096 + y, return_index=True)
    i = np.sort(i)
    return x[i], y[i], rng.integers(20, 255, len(i))


WIDE = [(n, lone, nf) for n, lone in ((300, True), (3000, False)) for nf in (800, 4000)]


@pytest.mark.parametrize("n,lone,nf", WIDE)
def test_model_on_three_roots(n, lone, nf):
    x, y, r = three_roots(n, lone)
    q = R.level_tables(532, 232, nf)[3][0]
    check(x, y, r, 532, 232, q, R.octree_ref(x, y, r, 16, 516, 16, 216, q), f"{n} keys nfeatures {nf}")


def test_every_way_out_reached():
    """A condition on the dot images and the three-root keys, not a
    measurement: together they leave the restated iterations every way."""
    _SEEN.clear()
    for k, nf in DOTS:
        test_model_on_dots(k, nf)
    for n, lone, nf in WIDE:
        test_model_on_three_roots(n, lone, nf)
    want = {"finish below D", "phase 2 below D", "phase 2 at D", "past D, then phase 2", "past D, then same size",
            "phase 2 twice", "nIni >= 2, D < 4", "single-key root beside a dividing root"}
    assert _SEEN >= want, f"not reached: {want - _SEEN}"
