"""Helpers shared by test_aligner_calibrate.py (CPU) and test_gpu_aligner_calibrate.py: the small clouds, removeFarPointCloud and
pcl::VoxelGrid<PointXYZI> in numpy float32, in the order oracle/estimate.cpp:mmlo_voxel_downsample sums in."""
import numpy as np
from scipy.spatial.transform import Rotation as Rsc

F = np.float32


# ---- the clouds of tests/test_gpu_gicp_batch.py (copied: test files are not imported) --------------------------------------
def corner_cloud(rng, n):
    """n points on the planes x = 0, y = 0, z = 0 of a 4 m room corner, 5 mm noise across each plane."""
    p = rng.uniform(0.0, 4.0, (n, 3))
    p[np.arange(n), rng.integers(0, 3, n)] = rng.normal(0.0, 0.005, n)
    return p


def pair(seed, n_src, n_tgt, scale=1.0, with_motion=False):
    """(src, tgt) float32: one pool of points, the target its first n_tgt, the source n_src of them in another order, moved by
    scale x (a few cm, a few mrad).  with_motion: also (R, t) with tgt-frame point = R src + t."""
    rng = np.random.default_rng(seed)
    pool = corner_cloud(rng, max(n_src, n_tgt, 1))
    tgt = pool[:n_tgt]
    src = pool[rng.permutation(len(pool))[:n_src]]
    R = Rsc.from_euler("xyz", scale * rng.uniform(-4e-3, 4e-3, 3)).as_matrix()
    t = scale * rng.uniform(-0.04, 0.04, 3)
    out = ((src - t) @ R).astype(np.float32), tgt.astype(np.float32)
    return out + (R, t) if with_motion else out


def start_matrix(i):
    """A distinct, recognisable T0: an alignment that does not run must hand it back untouched."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.25 + i, -0.5 * i, 0.125]
    T[3, :3] = [i, 2.0, -3.0]                                                # (not a rigid motion: nobody may "repair" it)
    return T


def key(res):
    """(converged, T, info) as bytes."""
    ok, T, info = res
    return (bool(ok), np.ascontiguousarray(T, np.float32).tobytes(), bytes(info))


def with_intensity(xyz, seed=0):
    """n x 4 float32: the points with a reflectivity-like fourth field (0 .. 255, not integral)."""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, rng.uniform(0.0, 255.0, (len(xyz), 1)).astype(np.float32)], axis=1)


# ---- removeFarPointCloud (lidars_extrinsic_cali.h:398-422) ----------------------------------------------------------------
def crop_far(xyzi, far_th):
    """Float arithmetic, left to right, strict comparison; order kept.  n x 4 float32 in, m x 4 float32 (C order) out."""
    p = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r2 = (x * x + y * y) + z * z
    assert r2.dtype == np.float32
    return np.ascontiguousarray(p[~(r2 > F(far_th) * F(far_th))])


# ---- pcl::VoxelGrid<PointXYZI>::applyFilter (PCL 1.8.1) in float32 -------------------------------------------------------
def voxel_overflows(xyz, leaf):
    inv = F(1.0) / F(leaf)
    d = ((xyz.max(0) - xyz.min(0)) * inv).astype(np.int64) + 1
    return int(d[0]) * int(d[1]) * int(d[2]) > 2147483647


def voxel_mean4(xyzi, leaf):
    """All four fields averaged per voxel: voxel index i + j dx + k dx dy on the floor of the bounding box, output ascending by
    index, a voxel's points summed in input order in float32 (from 0) and divided by their number.  Returns (m x 4, unfiltered)."""
    p = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    if len(p) == 0:
        return p.copy(), False
    xyz = p[:, :3]
    if voxel_overflows(xyz, leaf):
        return p.copy(), True
    inv = F(1.0) / F(leaf)
    min_b = np.floor(xyz.min(0) * inv).astype(np.int32)
    max_b = np.floor(xyz.max(0) * inv).astype(np.int32)
    div = (max_b - min_b + 1).astype(np.int64)
    cell = np.floor(xyz * inv) - min_b.astype(np.float32)
    assert cell.dtype == np.float32
    ijk = cell.astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    out = []
    first = 0
    while first < len(p):
        last = first + 1
        while last < len(p) and idx[order[last]] == idx[order[first]]:
            last += 1
        s = np.zeros(4, np.float32)
        for k in order[first:last]:
            s = s + p[k]
        out.append(s / F(last - first))
        first = last
    return np.asarray(out, np.float32).reshape(-1, 4), False


def host_crop_voxel(O, xyzi, far_th, leaf):
    """The reference of mml_cloud_crop_voxel: numpy crop, then oracle.voxel_downsample for x, y, z and voxel_mean4 for the
    intensity.  Returns (m x 4 float32, unfiltered); asserts that voxel_mean4's x, y, z are the oracle's bits, so that its
    intensity column is the mean over the oracle's own groups in the oracle's own order."""
    c = crop_far(xyzi, far_th)
    if len(c) == 0:
        return c, False
    ref3 = O.voxel_downsample(c[:, :3], leaf)
    ref4, unf = voxel_mean4(c, leaf)
    assert ref3.shape == ref4[:, :3].shape and ref3.tobytes() == np.ascontiguousarray(ref4[:, :3]).tobytes()
    return ref4, unf


def pose_errors(T, R, t):
    """(translation error in metres, rotation error in radians) of the 4 x 4 estimate T against the motion (R, t)."""
    T = np.asarray(T, np.float64)
    dR = T[:3, :3] @ R.T
    return float(np.linalg.norm(T[:3, 3] - t)), float(np.linalg.norm(Rsc.from_matrix(dR).as_rotvec()))
