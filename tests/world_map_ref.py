"""A plain numpy / Python restatement of the world map's arithmetic (csrc/world_map_key.h, include/mmloam_hip.h "The world
map"), independent of the library: a dict key -> [float32 sums x, y, z, intensity added one by one, count] per map set.

    world point   pout = R * pin + t in float64, (R0 x + R1 y) + R2 z, then + t, one rounding to float32 -- the transform written
                  out in the header comment of mml_cloud_download_registered_batch
    voxel index   i = floor(float64(x * inv)) with inv = float32(1) / float32(leaf) and the product in float32; a point is skipped
                  when its label is not in the mask, else when a coordinate or the intensity is not finite, else when an index
                  is outside [-2^17, 2^17) (the voxel (2^17-1)^3 of map 1023, whose key is the empty marker, counts as outside)
    key           map << 54 | (k + 2^17) << 36 | (j + 2^17) << 18 | (i + 2^17)
    accumulate    float32 adds, one point after the other, from the stored sum; centroid = sum / float32(count)
"""
import numpy as np

HALF = 1 << 17
EMPTY = (1 << 64) - 1
F32 = np.float32


def world_points(xyz, T):
    """(n, 3) float32 points at the row-major 4 x 4 pose T -> (n, 3) float32 world points."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros((len(p), 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(np.float32)
    return out


def inv_leaf(leaf):
    return F32(1.0) / F32(leaf)


def axis_index(v, inv):
    """The voxel index of one float32 coordinate, or None outside [-2^17, 2^17)."""
    with np.errstate(all="ignore"):
        f = np.floor(np.float64(F32(v) * F32(inv)))
    if not (f >= -HALF and f < HALF):
        return None
    return int(f)


def pack(map, i, j, k):
    return (map << 54) | ((k + HALF) << 36) | ((j + HALF) << 18) | (i + HALF)


def unpack(key):
    m = (1 << 18) - 1
    return key >> 54, (key & m) - HALF, ((key >> 18) & m) - HALF, ((key >> 36) & m) - HALF


def hash_position(key, slots):
    """csrc/world_map_key.h mml_wm_hash: the first table position a key is tried at (splitmix64's finaliser, masked)."""
    m = (1 << 64) - 1
    key ^= key >> 30
    key = (key * 0xbf58476d1ce4e5b9) & m
    key ^= key >> 27
    key = (key * 0x94d049bb133111eb) & m
    key ^= key >> 31
    return key & (slots - 1)


def table_slots(capacity):
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


class WorldMapRef:
    def __init__(self, leaf):
        self.inv = inv_leaf(leaf)
        self.vox = {}   # key -> [np.float32 x 4, count]
        self.info = dict(n_points=0, n_kept=0, n_nonfinite=0, n_out_of_range=0, n_masked=0, n_new_voxels=0)

    def add_world(self, map, xyzi, labels=None, label_mask=7):
        """World points (n, 4) float32 x, y, z, intensity into `map`, in the order given."""
        xyzi = np.asarray(xyzi, np.float32).reshape(-1, 4)
        labels = np.zeros(len(xyzi), np.int64) if labels is None else np.asarray(labels).astype(np.int64)
        # which points take part, in the order of the rules: mask, not finite, out of range (whole arrays, the rules of axis_index)
        masked = ~np.isin(labels, [l for l in (0, 1, 2) if (label_mask >> l) & 1])
        nonfinite = ~masked & ~np.isfinite(xyzi).all(axis=1)
        with np.errstate(all="ignore"):
            f = np.floor((xyzi[:, :3] * self.inv).astype(np.float64))     # the product in float32, floor of its double
        inside = ((f >= -HALF) & (f < HALF)).all(axis=1)
        ijk = np.where(inside[:, None], f, 0).astype(np.int64)
        keys = [pack(map, int(i), int(j), int(k)) for i, j, k in ijk]    # Python integers: all 64 bits
        out = ~masked & ~nonfinite & ~(inside & np.array([k != EMPTY for k in keys], bool))
        kept = ~masked & ~nonfinite & ~out
        for name, sel in (("n_points", np.ones(len(xyzi), bool)), ("n_masked", masked), ("n_nonfinite", nonfinite), ("n_out_of_range", out),
                          ("n_kept", kept)):
            self.info[name] += int(sel.sum())
        # a voxel's points one after the other in float32, from the stored sum: cumsum adds sequentially, in the order given
        rows = {}
        for r in np.flatnonzero(kept):
            rows.setdefault(keys[r], []).append(r)
        for key, rr in rows.items():
            if key not in self.vox:
                self.vox[key] = [np.zeros(4, np.float32), 0]
                self.info["n_new_voxels"] += 1
            a = self.vox[key]
            a[0] = np.cumsum(np.concatenate([a[0][None], xyzi[rr]]), axis=0, dtype=np.float32)[-1]
            a[1] += len(rr)

    def add(self, map, xyz, intensity, T, labels=None, label_mask=7):
        """Sensor-frame points through the pose, then add_world."""
        w = world_points(xyz, T)
        self.add_world(map, np.concatenate([w, np.asarray(intensity, np.float32).reshape(-1, 1)], axis=1), labels, label_mask)

    def add_records(self, map, rec, label_mask=7):
        """(n, 12) float32 registered-cloud records (x y z 1 | 0 0 label 0 | intensity 0 0 0), already in the world frame."""
        rec = np.asarray(rec, np.float32).reshape(-1, 12)
        self.add_world(map, rec[:, [0, 1, 2, 8]], rec[:, 6].astype(np.int64), label_mask)

    def reset(self, map=-1):
        self.vox = {k: v for k, v in self.vox.items() if map >= 0 and (k >> 54) != map}

    def size(self, map=-1):
        return sum(1 for k in self.vox if map < 0 or (k >> 54) == map)

    def download(self, map):
        """((n, 4) float32 centroids, (n,) int32 counts) of one map in ascending key order."""
        keys = sorted(k for k in self.vox if (k >> 54) == map)
        out = np.zeros((len(keys), 4), np.float32)
        cnt = np.zeros(len(keys), np.int32)
        for r, k in enumerate(keys):
            s, n = self.vox[k]
            out[r] = s / F32(n)
            cnt[r] = n
        return out, cnt
