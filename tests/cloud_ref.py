"""Reference of the dense clouds (odo_dense_clouds, include/odo.h): numpy
restatements of Frame::CreateCloud (frame.cpp:191-215), of PCL 1.8's
VoxelGrid<PointXYZRGB> as the header pins it, and of the map transform; a
plain-Python transcription of VoxelGrid's four passes (index vector, sort,
count, centroid) for tiny clouds; and the builders of the crafted cases.

The numpy form is written exactly as the header states the semantics: float32
arithmetic left to right, a stable argsort on the unsigned key, exact integer
colour sums. Its x, y, z centroid is a float64 mean (`xyz64`), with the mean
absolute coordinate of the voxel beside it (`mabs`): the device sums in float32
in an order of its own, so the comparison is the worst-case bound of such a sum,
    |got - ref64| <= 1.01 * count * 2^-24 * mean|p_i| + 2^-24 * |ref64|
(count terms in any order, plus the division's rounding); a voxel of one point
must equal that point bit for bit.
"""
import numpy as np

import fuse_ref

f32 = np.float32
W, H = 640, 480
P = W * H
INT32_MAX = 2**31 - 1
CLOUD_OK, CLOUD_UNFILTERED = 0, 1
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])

# cameras (the calib fields a context is created with; no distortion is applied to a cloud)
DF = 1.0 / 5000.0
CAM_FR1 = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, depth_factor=DF)
CAM_FR1_CORNER = dict(fx=517.3, fy=516.5, cx=0.0, cy=0.0, depth_factor=DF)  # x, y >= 0: one voxel at a large leaf
# fuse_ref.CAM_UNIT with a power-of-two depth factor: depth 1024 is z = 1, x = j, y = i, all exact
CAM_UNIT = dict(fx=fuse_ref.CAM_UNIT["fx"], fy=fuse_ref.CAM_UNIT["fy"], cx=fuse_ref.CAM_UNIT["cx"],
                cy=fuse_ref.CAM_UNIT["cy"], depth_factor=2.0**-10)
CAM_UNIT_CENTRED = dict(CAM_UNIT, cx=320.0, cy=240.0)  # x = j - 320, y = i - 240: both sides of zero
CAMS = dict(fr1=CAM_FR1, corner=CAM_FR1_CORNER, unit=CAM_UNIT, centred=CAM_UNIT_CENTRED)


def ordered(a):
    """float32 -> uint32 with the same order, -0 below +0 (the exact min / max)."""
    b = np.ascontiguousarray(a, f32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def create_cloud(bgr, depth, cam):
    """frame.cpp:191-215 on one frame (H x W x 3 u8, H x W u16)."""
    z = depth.astype(f32) * f32(cam["depth_factor"])
    invfx, invfy = f32(1.0) / f32(cam["fx"]), f32(1.0) / f32(cam["fy"])
    i, j = np.meshgrid(np.arange(depth.shape[0]), np.arange(depth.shape[1]), indexing="ij")
    x = (j.astype(f32) - f32(cam["cx"])) * z * invfx
    y = (i.astype(f32) - f32(cam["cy"])) * z * invfy
    keep = z > 0
    c = np.zeros(int(keep.sum()), CLOUD_DTYPE)
    c["x"], c["y"], c["z"] = x[keep], y[keep], z[keep]
    c["b"], c["g"], c["r"] = bgr[..., 0][keep], bgr[..., 1][keep], bgr[..., 2][keep]
    c["a"] = 255
    return c


def grid_of(cloud, leaf):
    """VoxelGrid's set-up: dict(min_p, max_p, d, filtered, min_b, div_b, inv)."""
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    g = dict(min_p=np.zeros(3, f32), max_p=np.zeros(3, f32), d=None, filtered=False, min_b=np.zeros(3, np.int32),
             div_b=np.zeros(3, np.int32), inv=f32(0))
    if len(cloud) == 0:
        return g
    o = ordered(xyz)
    g["min_p"] = xyz[np.argmin(o, 0), np.arange(3)]
    g["max_p"] = xyz[np.argmax(o, 0), np.arange(3)]
    if not leaf > 0:
        return g
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(leaf)
        t = (g["max_p"] - g["min_p"]) * inv
        if not np.all(t < f32(2.0**31)):  # also NaN; no int64 holds the product
            return g
        d = [int(v) + 1 for v in t]
        g["d"] = d
        if d[0] * d[1] * d[2] > INT32_MAX:
            return g
        fl, fh = np.floor(g["min_p"] * inv), np.floor(g["max_p"] * inv)
    if not (np.all(fl >= f32(-2.0**31)) and np.all(fh < f32(2.0**31))):
        return g
    min_b = [int(v) for v in fl]
    div_b = [int(v) - m + 1 for v, m in zip(fh, min_b)]
    if max(div_b) > INT32_MAX:
        return g
    g.update(filtered=True, min_b=np.array(min_b, np.int32), div_b=np.array(div_b, np.int32), inv=inv)
    return g


def keys_of(cloud, g):
    """The unsigned 32-bit voxel key of every point (applyFilter's index vector)."""
    inv, mb, dv = g["inv"], g["min_b"], [int(v) for v in g["div_b"]]
    # uint64 arithmetic wraps modulo 2^64, so its low 32 bits are the wrapping int32 sum
    ijk = [(np.floor(cloud[a] * inv) - f32(mb[k])).astype(np.int32).astype(np.int64).astype(np.uint64)
           for k, a in enumerate("xyz")]
    key = ijk[0] + ijk[1] * np.uint64(dv[0]) + ijk[2] * np.uint64(dv[0] * dv[1] % 2**32)
    return (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def voxel_grid(cloud, leaf):
    """The whole filter. dict(status, n_valid, n_points, min_b, div_b, min_p,
    max_p, keys, counts, bgra n x 4, xyz64 n x 3, mabs n x 3, first n x 3 f32: the
    first point of each voxel (the result itself where count is 1))."""
    g = grid_of(cloud, leaf)
    n = len(cloud)
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    col = np.stack([cloud["b"], cloud["g"], cloud["r"], cloud["a"]], 1)
    out = dict(n_valid=n, min_p=g["min_p"], max_p=g["max_p"], min_b=g["min_b"], div_b=g["div_b"])
    if n == 0 or not g["filtered"]:
        out.update(status=CLOUD_OK if n == 0 else CLOUD_UNFILTERED, n_points=n, keys=np.arange(n, dtype=np.uint32),
                   counts=np.ones(n, np.int32), bgra=col, xyz64=xyz.astype(np.float64), mabs=np.abs(xyz).astype(np.float64),
                   first=xyz, min_b=np.zeros(3, np.int32), div_b=np.zeros(3, np.int32))
        return out
    key = keys_of(cloud, g)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    counts = np.diff(np.concatenate([head, [n]])).astype(np.int32)
    x64 = xyz[order].astype(np.float64)
    s64 = np.add.reduceat(x64, head, 0)
    a64 = np.add.reduceat(np.abs(x64), head, 0)
    csum = np.add.reduceat(col[order].astype(np.uint64), head, 0)
    fc = counts.astype(f32)[:, None]
    bgra = (csum.astype(f32) / fc).astype(np.uint32).astype(np.uint8)
    out.update(status=CLOUD_OK, n_points=len(head), keys=ks[head], counts=counts, bgra=bgra,
               xyz64=s64 / counts[:, None], mabs=a64 / counts[:, None], first=xyz[order][head])
    return out


def transform(pts, T):
    """pcl::transformPointCloud on CLOUD_DTYPE points: x' = ((m00 x + m01 y) + m02 z) + m03 in float32."""
    M = np.asarray(T, f32).reshape(4, 4)
    x, y, z = pts["x"], pts["y"], pts["z"]
    out = pts.copy()
    for k, a in enumerate("xyz"):
        out[a] = ((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3]
    return out


def voxel_grid_py(cloud, leaf):
    """PCL's passes one after the other in plain Python (tiny clouds): the index
    vector, its sort, the count of each run, the centroid of each run with
    float32 accumulators in sorted order. Returns (keys, counts, points) or
    None for the overflow return."""
    g = grid_of(cloud, leaf)
    if not g["filtered"]:
        return None
    inv, mb, dv = g["inv"], g["min_b"], [int(v) for v in g["div_b"]]
    index = []
    for i, p in enumerate(cloud):
        ijk = [int(f32(np.floor(f32(p[a]) * inv)) - f32(mb[k])) for k, a in enumerate("xyz")]
        index.append(((ijk[0] + ijk[1] * dv[0] + ijk[2] * (dv[0] * dv[1])) % 2**32, i))
    index.sort(key=lambda t: t[0])
    runs, first = [], 0
    while first < len(index):
        last = first + 1
        while last < len(index) and index[last][0] == index[first][0]:
            last += 1
        runs.append((first, last))
        first = last
    keys, counts, pts = [], [], np.zeros(len(runs), CLOUD_DTYPE)
    for v, (lo, hi) in enumerate(runs):
        acc = [f32(0)] * 7
        for _, i in index[lo:hi]:
            for k, a in enumerate("xyzbgra"):
                acc[k] = f32(acc[k] + f32(cloud[i][a]))
        nf = f32(hi - lo)
        for k, a in enumerate("xyz"):
            pts[v][a] = f32(acc[k] / nf)
        for k, a in enumerate("bgra"):
            pts[v][a] = int(f32(acc[3 + k] / nf)) & 255
        keys.append(index[lo][0])
        counts.append(hi - lo)
    return np.array(keys, np.uint32), np.array(counts, np.int32), pts


def centroid_bound(ref):
    """The per-coordinate bound of the module docstring, n x 3."""
    return 1.01 * ref["counts"][:, None] * 2.0**-24 * ref["mabs"] + 2.0**-24 * np.abs(ref["xyz64"])


def dense_ref(bgr, depth, cam, leaf):
    """One reference per frame of a batch."""
    return [voxel_grid(create_cloud(bgr[i], depth[i], cam), leaf) for i in range(len(depth))]


# ------------------------------------------------------------------ the cases
def colours(rng, n=1):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def ramp_depth():
    """1 ... 65535 over the frame in raster order."""
    return (1 + (np.arange(P, dtype=np.int64) * 65534) // (P - 1)).astype(np.uint16).reshape(1, H, W)


def random_depth(rng, n=1):
    return rng.integers(1, 65536, (n, H, W), dtype=np.uint16)


def room_depth(rng):
    """A box seen from inside: smooth depth between 1 and 4 m with a few objects and holes."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 2.5 + 1.2 * np.cos(j / W * 3.0) - 0.8 * (i / H) + 0.05 * rng.standard_normal((H, W))
    z[100:220, 150:300] = 1.2
    z[300:420, 400:560] = 1.7
    z[rng.random((H, W)) < 0.02] = 0.0
    return np.clip(z * 5000.0, 0, 65535).astype(np.uint16).reshape(1, H, W)


def scattered(rng, k):
    """k valid pixels scattered over the rows (all of them for k = P)."""
    d = np.zeros(P, np.uint16)
    at = np.arange(P) if k == P else np.sort(rng.choice(P, k, replace=False))
    d[at] = rng.integers(2000, 20000, len(at), dtype=np.uint16)
    return d.reshape(1, H, W)


VALID_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, P)


def cases():
    """name -> (camera name, bgr n x H x W x 3, depth n x H x W, leaf); one to three frames each."""
    rng = np.random.default_rng(0xC10D)
    c = {}
    c["room"] = ("fr1", colours(rng), room_depth(rng), 0.03)
    c["random_overflow"] = ("fr1", colours(rng), random_depth(rng), 0.01)
    c["random_no_overflow"] = ("fr1", colours(rng), random_depth(rng), 0.012)
    c["ramp"] = ("fr1", colours(rng), ramp_depth(), 0.03)
    c["ramp_all_key_bytes"] = ("fr1", colours(rng), ramp_depth(), 0.012)
    c["heavy_four_voxels"] = ("fr1", colours(rng), random_depth(rng), 100.0)
    c["heavy_one_voxel"] = ("corner", colours(rng), random_depth(rng), 100.0)
    plane = np.full((1, H, W), 1024, np.uint16)
    c["boundary_unit_half"] = ("unit", colours(rng), plane, 0.5)
    c["boundary_unit_one"] = ("unit", colours(rng), plane, 1.0)
    c["boundary_centred_half"] = ("centred", colours(rng), plane, 0.5)
    c["boundary_centred_four"] = ("centred", colours(rng), plane, 4.0)
    for k in VALID_COUNTS:
        c[f"valid_{k}"] = ("fr1", colours(rng), scattered(rng, k), 0.03)
    c["ragged_batch"] = ("fr1", colours(rng, 3), np.concatenate([scattered(rng, 0), room_depth(rng), scattered(rng, 1)]), 0.03)
    c["leaf_zero"] = ("fr1", colours(rng, 2), np.concatenate([room_depth(rng), scattered(rng, 257)]), 0.0)
    return c


def tiny_clouds():
    """name -> (cloud, leaf) for the transcription: a few hundred points."""
    rng = np.random.default_rng(0x717)
    out = {}

    def cloud(xyz):
        c = np.zeros(len(xyz), CLOUD_DTYPE)
        c["x"], c["y"], c["z"] = np.asarray(xyz, f32).T
        for a in "bgr":
            c[a] = rng.integers(0, 256, len(xyz))
        c["a"] = 255
        return c

    out["cube"] = (cloud(rng.uniform(-1, 1, (300, 3))), 0.3)
    out["dense"] = (cloud(rng.uniform(-1, 1, (400, 3))), 1.5)
    out["one_voxel"] = (cloud(rng.uniform(0.1, 0.9, (100, 3))), 1.0)
    out["one_point"] = (cloud([[0.3, -0.2, 1.0]]), 0.03)
    g = np.arange(-4, 5) * 0.25  # p * inv an exact integer on both sides of zero
    out["lattice"] = (cloud(np.stack(np.meshgrid(g, g, [1.0, 1.25]), -1).reshape(-1, 3)), 0.25)
    out["far"] = (cloud(rng.uniform(-1, 1, (200, 3)) * [100.0, 1.0, 0.1]), 0.01)  # a long axis: keys above 2^24
    return out
