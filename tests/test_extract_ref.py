"""CPU: the oracle's extractor stages against the independent references of
extract_ref.py on crafted images, and the conditions that make
test_extract_stages_gpu.py mean something (which kernel paths the images
reach), asserted from the references alone.

FAST and the octree bit-exact (count, x, y, response, order); IC angles
bit-exact; descriptor bits equal outside brief_ref's ambiguity mask; the
keypoint geometry within the float32 bounds of extract_ref.assert_geometry.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import extract_ref as R
import oracle_lib as O

SEED = 7
SIZES = [(320, 240), (330, 250), (480, 240), (640, 200), (532, 232)]
BIG = (640, 480)                       # with the two dense families only
BIG_FAMILIES = ("noise", "patchwork")
# (w, h) -> nfeatures of its runs. 320x240: single-digit quotas at 60, quotas
# above the candidates of the sparse families at 1500. 532x232 at 4000: the
# only way to a sorted list of more than 512 nodes, see test_octree_paths.
NFEATURES = {(320, 240): (60, 800, 1500), (532, 232): (800, 4000)}
CASES = [(f, w, h) for (w, h) in SIZES for f in R.FAMILIES] + [(f,) + BIG for f in BIG_FAMILIES]
IDS = [f"{f}-{w}x{h}" for f, w, h in CASES]


def nfeatures_of(w, h):
    return NFEATURES.get((w, h), (800,))


def split_levels(flat, lw, lh):
    out, off = [], 0
    for a, b in zip(lw, lh):
        out.append(np.ascontiguousarray(flat[off:off + a * b]).reshape(b, a))
        off += a * b
    return out


def oracle_pyramid(gray, nf=800):
    h, w = gray.shape
    lw, lh, _, _ = R.level_tables(w, h, nf)
    flat = np.zeros(sum(a * b for a, b in zip(lw, lh)), np.uint8)
    n = O.lib().oracle_pyramid(O.ptr(np.ascontiguousarray(gray)), w, h, C.byref(O.orb_params(nf)), O.ptr(flat))
    assert n == flat.size
    return split_levels(flat, lw, lh)


def oracle_fast(level, ini=20, mn=7):
    h, w = level.shape
    out = np.zeros(max((w * h) // 4, 1), O.KP_DTYPE)
    n = O.lib().oracle_fast_level(O.ptr(np.ascontiguousarray(level)), w, h, ini, mn, O.ptr(out), out.size)
    assert n <= out.size
    return out[:n]


def oracle_octree(keys, lw, lh, quota):
    out = np.zeros(max(len(keys), 1), O.KP_DTYPE)
    n = O.lib().oracle_octree(O.ptr(np.ascontiguousarray(keys)), len(keys), 16, lw - 16, 16, lh - 16, quota,
                              O.ptr(out), out.size)
    assert n <= out.size
    return out[:n]


def oracle_blur(level):
    out = np.zeros_like(level)
    O.lib().oracle_blur(O.ptr(np.ascontiguousarray(level)), level.shape[1], level.shape[0], O.ptr(out))
    return out


def keys_of(x, y, r):
    """(x, y, response) as the orb_kp records the FAST stages emit."""
    k = np.zeros(len(x), O.KP_DTYPE)
    k["x"], k["y"], k["response"] = x, y, r
    k["size"], k["angle"], k["class_id"] = 7, -1, -1
    return k


def assert_keys(got, x, y, r, what):
    assert len(got) == len(x), f"{what}: {len(got)} keys vs {len(x)}"
    for f, ref in (("x", x), ("y", y), ("response", r)):
        bad = np.nonzero(got[f] != ref)[0]
        assert bad.size == 0, f"{what}: {f} differs at {bad[:8]}: {got[f][bad[:8]]} vs {np.asarray(ref)[bad[:8]]}"


@functools.lru_cache(maxsize=None)
def analysis(family, w, h):
    """The oracle's pyramid of one image and the reference FAST of every level."""
    img = R.FAMILIES[family](w, h, SEED)
    assert img.shape == (h, w) and img.dtype == np.uint8
    levels = oracle_pyramid(img)
    fast = [R.fast_level_ref(lv) for lv in levels]
    return img, levels, fast


@functools.lru_cache(maxsize=None)
def octree_of(family, w, h, nf):
    """Per level (kept indices, lengths of the lists sorted) at nf features."""
    _, levels, fast = analysis(family, w, h)
    quota = R.level_tables(w, h, nf)[3]
    out = []
    for lv, (x, y, r, _), q in zip(levels, fast, quota):
        st = {}
        keep = R.octree_ref(x, y, r, 16, lv.shape[1] - 16, 16, lv.shape[0] - 16, q, st)
        out.append((keep, st.get("sorted", [])))
    return out


def test_equal_channels_are_the_gray_value():
    """The tests feed the gray images as B = G = R: cvtColor's weights sum to
    2^14, so the gray byte is the common value."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(O.gray(np.stack([v, v, v], 2)), v)


@pytest.mark.parametrize("w,h", SIZES + [BIG])
def test_level_tables_equal_oracle(w, h):
    for nf in (60, 800, 1500, 2000, 4000):
        lw, lh, sc, q = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_float * 8)(), (C.c_int * 8)()
        O.lib().oracle_level_sizes(C.byref(O.orb_params(nf)), w, h, lw, lh, sc, q)
        rw, rh, rs, rq = R.level_tables(w, h, nf)
        assert (list(lw), list(lh), list(q)) == (rw, rh, rq)
        O.assert_same_bits(list(sc), rs, "level scales")
    u = (C.c_int * 16)()
    O.lib().oracle_umax(u)
    assert list(u) == R.umax_table()


@pytest.mark.parametrize("family,w,h", CASES, ids=IDS)
def test_oracle_fast_equals_ref(family, w, h):
    _, levels, fast = analysis(family, w, h)
    for l, (lv, (x, y, r, _)) in enumerate(zip(levels, fast)):
        assert_keys(oracle_fast(lv), x, y, r, f"level {l}")


@pytest.mark.parametrize("family,w,h", CASES, ids=IDS)
def test_oracle_octree_equals_ref(family, w, h):
    _, levels, fast = analysis(family, w, h)
    for nf in nfeatures_of(w, h):
        quota = R.level_tables(w, h, nf)[3]
        for l, (lv, (x, y, r, _)) in enumerate(zip(levels, fast)):
            keep = octree_of(family, w, h, nf)[l][0]
            got = oracle_octree(keys_of(x, y, r), lv.shape[1], lv.shape[0], quota[l])
            assert_keys(got, x[keep], y[keep], r[keep], f"nfeatures {nf} level {l}")


def reference_frame(levels, blurred, kept, scale):
    """The frame's keypoints and descriptors from per-level retained keys
    [(x, y, response)] (relative to the border): KP_DTYPE array, desc, mask."""
    kps, desc, mask = [], [], []
    for l, (x, y, r) in enumerate(kept):
        k = np.zeros(len(x), O.KP_DTYPE)
        k["x"], k["y"], size = R.scaled_keypoints(l, x, y, scale[l])
        k["size"], k["response"], k["octave"], k["class_id"] = size, r, l, -1
        ix, iy = np.asarray(x, np.int64) + R.BORDER, np.asarray(y, np.int64) + R.BORDER
        k["angle"] = R.ic_angle_ref(levels[l], ix, iy)
        d, m = R.brief_ref(blurred[l], ix, iy, k["angle"])
        kps.append(k)
        desc.append(d)
        mask.append(m)
    return np.concatenate(kps), np.concatenate(desc), np.concatenate(mask)


def assert_frame(kps, desc, ref_kps, ref_desc, mask, what):
    """Keypoints field by field (the angle by bit pattern), descriptor bits
    outside the ambiguity mask, and the cap on the mask's share of the bits."""
    assert len(kps) == len(ref_kps), f"{what}: N {len(kps)} vs {len(ref_kps)}"
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        bad = np.nonzero(kps[f] != ref_kps[f])[0]
        assert bad.size == 0, f"{what}: kp.{f} differs at {bad[:8]}: {kps[f][bad[:8]]} vs {ref_kps[f][bad[:8]]}"
    O.assert_same_bits(kps["angle"], ref_kps["angle"], f"{what}: IC angle")
    diff = (desc ^ ref_desc) & ~mask
    bad = np.nonzero(diff.any(1))[0]
    assert bad.size == 0, f"{what}: descriptor bits differ outside the ambiguity mask at keypoints {bad[:8]}"
    if len(kps):
        share = np.unpackbits(mask).sum() / (256.0 * len(kps))
        # a cap, not a measurement: the expected share is about 4 * 2^-16
        assert share <= 1e-3, f"{what}: {share:.2e} of the descriptor bits are ambiguous"


@functools.lru_cache(maxsize=None)
def oracle_extract(family, w, h, nf=800):
    img = analysis(family, w, h)[0]
    cap = nf + 64
    kps = np.zeros(cap, O.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = O.lib().oracle_orb_extract(O.ptr(img), w, h, C.byref(O.orb_params(nf)), O.ptr(kps), O.ptr(desc), cap)
    assert n <= cap
    return kps[:n], desc[:n]


@pytest.mark.parametrize("family,w,h", CASES, ids=IDS)
def test_oracle_angles_and_descriptors_equal_ref(family, w, h):
    _, levels, fast = analysis(family, w, h)
    kept = [(x[k], y[k], r[k]) for (x, y, r, _), (k, _) in zip(fast, octree_of(family, w, h, 800))]
    ref_kps, ref_desc, mask = reference_frame(levels, [oracle_blur(lv) for lv in levels], kept,
                                              R.level_tables(w, h, 800)[2])
    kps, desc = oracle_extract(family, w, h)
    assert_frame(kps, desc, ref_kps, ref_desc, mask, "oracle_orb_extract")


@pytest.mark.parametrize("family,w,h", CASES, ids=IDS)
def test_oracle_geometry_within_bounds(family, w, h):
    kps, _ = oracle_extract(family, w, h)
    cal = O.fr1_calib()
    for name, fn in R.DEPTHS.items():
        dep = fn(w, h)
        z = np.zeros(w * h, np.float32)
        O.lib().oracle_depth_to_f32(O.ptr(dep), w * h, cal.depth_factor, O.ptr(z))
        n = len(kps)
        kun, xyz, ur = np.zeros((max(n, 1), 2), np.float32), np.zeros((max(n, 1), 3), np.float32), \
            np.zeros(max(n, 1), np.float32)
        O.lib().oracle_frame_geometry(O.ptr(np.ascontiguousarray(kps)), n, O.ptr(z), w, h, C.byref(cal), O.ptr(kun),
                                      O.ptr(xyz), O.ptr(ur))
        R.assert_geometry(kun[:n], xyz[:n], ur[:n], kps["x"], kps["y"], dep, cal, f"depth {name}")
        if name == "zeros":
            assert (xyz[:n] == 0).all() and (ur[:n] == -1).all()
        elif n:
            assert (xyz[:n, 2] > 0).sum() >= n - 1  # the ramp holds one zero


def test_fast_vectorised_equals_bruteforce():
    """fast_strength against the per-pixel definition (as test_oracle._fast_numpy)."""
    from test_oracle import _fast_numpy
    rng = np.random.default_rng(3)
    img = (rng.random((40, 52)) * 60 + 90).astype(np.uint8)
    img[10:25, 12:30] = 230
    img[28:33, 5:9] = 10
    img[5::4, 33::4] = 255
    m = R.fast_strength(img)
    for th in (7, 20):
        x, y, s, _ = R._fast_roi(m, th)
        assert list(zip(x.tolist(), y.tolist(), s.tolist())) == _fast_numpy(img, th) and len(x) > 0


# ---------------------------------------------------------------- conditions
def level0_segments(family, w, h):
    cells = analysis(family, w, h)[2][0][3]
    wcell = R.fast_cells(w, h)[1][2]
    return cells, R.segments(cells, wcell)


def test_fast_overflow_reached():
    """k_fast_seg's corner list holds 1024 entries per segment: noise and
    patchwork put more corners than that into a level-0 segment at every
    size, and fewer into another at 320x240 (and, for patchwork, at every size)."""
    for family in BIG_FAMILIES:
        for w, h in SIZES + [BIG]:
            cells, segs = level0_segments(family, w, h)
            per = [int(cells["n_ini"][s].sum()) for s in segs]
            assert max(per) > 1024, f"{family} {w}x{h}: largest segment has {max(per)} corners"
            if family == "patchwork" or (w, h) == (320, 240):
                assert min(per) < 1024, f"{family} {w}x{h}: smallest segment has {min(per)} corners"


def test_retry_cells_share_segments():
    """A segment with both a retried cell and a cell that kept corners at
    iniThFAST; over the sizes, a retried cell first, last and inside its segment."""
    for family in ("patchwork", "dots_low"):
        places = set()
        for w, h in SIZES:
            cells, segs = level0_segments(family, w, h)
            mixed = [s for s in segs if cells["retried"][s].any() and (~cells["retried"][s] & (cells["n_kept"][s] > 0)).any()]
            assert mixed, f"{family} {w}x{h}: no segment mixes retried and kept cells"
            for s in mixed:
                rt = np.nonzero(cells["retried"][s])[0]
                places |= {"first"} if 0 in rt else set()
                places |= {"last"} if len(s) - 1 in rt else set()
                places |= {"inside"} if ((rt > 0) & (rt < len(s) - 1)).any() else set()
        assert places == {"first", "last", "inside"}, f"{family}: retried cells only {places} of their segments"


def test_all_tie_cells_reached():
    """discs: a cell with corners at iniThFAST that lost all of them to NMS
    ties and was redone at minThFAST, as the reference does."""
    for w, h in SIZES:
        cells = analysis("discs", w, h)[2][0][3]
        assert ((cells["n_ini"] > 0) & cells["retried"]).any(), f"discs {w}x{h}"


def test_nms_reaches_cell_boundaries_ties_and_top_score():
    """A corner whose stronger neighbour lies one pixel across a cell
    boundary (so it is kept where a frame-wide NMS drops it), equal neighbouring
    scores, and the top score 254."""
    x, y, r, cells = analysis("noise", 320, 240)[2][0]
    lv = analysis("noise", 320, 240)[1][0]
    m = R.fast_strength(lv)
    s = np.where(m > 20, m - 1, 0)
    nb = np.zeros_like(s)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                nb = np.maximum(nb, np.roll(np.roll(s, dy, 0), dx, 1))
    kept_global = s[y + 16, x + 16] > nb[y + 16, x + 16]
    assert (~kept_global).sum() > 0, "no kept corner has a stronger or equal neighbour across a cell boundary"
    assert ((s > 0) & (s == nb)).any(), "no equal neighbouring scores"
    assert analysis("dots_equal", 320, 240)[2][0][2].max() == 254


def test_octree_paths_reached():
    """Levels with 0 and 1 candidates, fewer than the quota, more than 20 000;
    all responses equal with more candidates than the quota; more than one
    root node; the (size, pointer) sort on lists of at most and of more than
    512 nodes (k_octree counts ranks up to OT_RANK_MAX = 512 and sorts beyond).
    The sorted list is shorter than the quota, so it passes 512 only above
    about 2400 features: 532x232 (three root nodes: 768 nodes after four
    divisions) at 4000 features."""
    seen = set()
    for family, w, h in CASES:
        _, levels, fast = analysis(family, w, h)
        for nf in nfeatures_of(w, h):
            quota = R.level_tables(w, h, nf)[3]
            for l, ((x, y, r, _), (keep, srt)) in enumerate(zip(fast, octree_of(family, w, h, nf))):
                n = len(x)
                seen |= {"none"} if n == 0 else set()
                seen |= {"one"} if n == 1 else set()
                seen |= {"below quota"} if 1 < n < quota[l] else set()
                seen |= {"above 20000"} if n > 20000 else set()
                seen |= {"all equal"} if n > quota[l] and np.unique(r).size == 1 else set()
                seen |= {"sort <= 512"} if any(0 < c <= 512 for c in srt) else set()
                seen |= {"sort > 512"} if any(c > 512 for c in srt) else set()
                seen |= {"single digit quota"} if quota[l] < 10 and n > quota[l] else set()
                lw, lh = levels[l].shape[1], levels[l].shape[0]
                n_ini = R._c_round(float(np.float32(lw - 32) / np.float32(lh - 32)))
                seen |= {f"nIni {min(n_ini, 4)}"} if n > 1 else set()
    want = {"none", "one", "below quota", "above 20000", "all equal", "sort <= 512", "sort > 512",
            "single digit quota", "nIni 1", "nIni 2", "nIni 3", "nIni 4"}
    assert seen == want, f"not reached: {want - seen}"


def test_root_node_tie_rounds_away_from_zero():
    """532x232: (532 - 32) / (232 - 32) = 2.5, and round() gives three root nodes."""
    assert np.float32(500) / np.float32(200) == 2.5 and R._c_round(2.5) == 3


def test_cell_capacity_bound():
    """No cell keeps more than ceil((rows - 6) / 2) * ceil((cols - 6) / 2)
    corners (kept corners are never 8-neighbours): what cell_cap rests on."""
    for family, w, h in CASES:
        for (_, _, _, cells) in analysis(family, w, h)[2]:
            if cells.size:
                cap = ((cells["rows"] - 6 + 1) // 2) * ((cells["cols"] - 6 + 1) // 2)
                assert (cells["n_kept"] <= cap).all(), f"{family} {w}x{h}"


def test_ring_keypoints_survive_the_octree():
    """ring_dots: level-0 keypoints at the eight extreme positions (x = 19,
    w - 20, y = 19, h - 20: the border plus FAST's own frame), and no family
    puts a candidate outside them."""
    for w, h in SIZES:
        x, y, _, _ = analysis("ring_dots", w, h)[2][0]
        for nf in nfeatures_of(w, h):
            keep = octree_of("ring_dots", w, h, nf)[0][0]
            got = set(zip((x[keep] + 16).tolist(), (y[keep] + 16).tolist()))
            assert set(R.ring_positions(w, h)) <= got, f"{w}x{h} nfeatures {nf}"
    for family, w, h in CASES:
        for lv, (x, y, _, _) in zip(*analysis(family, w, h)[1:]):
            if len(x):
                assert x.min() >= 3 and y.min() >= 3 and x.max() <= lv.shape[1] - 36 and y.max() <= lv.shape[0] - 36


def test_degenerate_patches_reached():
    """IC moments m10 = m01 = 0 (fastAtan2(0, 0)), angles on the axes, and flat
    blurred patches (every rBRIEF test compares equal values)."""
    seen = set()
    for family in ("blank_but_one", "ring_dots", "dots_equal", "checker_sat"):
        for w, h in SIZES:
            _, levels, fast = analysis(family, w, h)
            for l, ((x, y, r, _), (keep, _)) in enumerate(zip(fast, octree_of(family, w, h, 800))):
                if not len(keep):
                    continue
                ix, iy = x[keep] + 16, y[keep] + 16
                m01, m10 = R.ic_moments(levels[l], ix, iy)
                seen |= {"zero moments"} if ((m01 == 0) & (m10 == 0)).any() else set()
                seen |= {"axis"} if (((m01 == 0) ^ (m10 == 0))).any() else set()
                d, _ = R.brief_ref(oracle_blur(levels[l]), ix, iy, R.ic_angle_ref(levels[l], ix, iy))
                seen |= {"zero descriptor"} if (~d.any(1)).any() else set()
    assert seen == {"zero moments", "axis", "zero descriptor"}, seen
