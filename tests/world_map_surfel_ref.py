"""A numpy restatement of a surfel map's arithmetic (csrc/world_map_key.h, include/mmloam_hip.h "Surfel maps"), independent of
the library and built on tests/world_map_ref.py, whose world point, voxel index, key and order of the points it uses.

    voxel centre   c = (float32(i) + float32(0.5)) * float32(leaf) per axis, i the voxel index; offset d = w - c in float32
    view vector    v = o - w in float32, o = float32 of the pose's translation (T[3], T[7], T[11])
    moments        12 float32 per voxel: sdx sdy sdz vx | sxx sxy sxz vy | syy syz szz vz.  One point: sd += d; the six products
                   dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz each rounded to float32, then added; v += v_point.  Every add starts
                   from the stored value, the points in the order given (add_point: np.float32 scalars, operation for operation;
                   add_world runs the same adds per voxel as one float32 cumsum, which adds one element after the other)
    covariance     float64: nd = float64(n), m_a = float64(sd_a) / nd, C_ab = float64(s_ab) / nd - m_a * m_b
    surfel         n >= 3: the oracle's eig3 (O.model_fit5(0, ...), bit for bit the device's eig3_sym) on Cxx Cxy Cyy Cxz Cyz Czz;
                   normal = float32(eigenvector of ev[0]), negated when (n.x*V.x + n.y*V.y) + n.z*V.z < 0 in float64 (V the view
                   sum); l0 l1 l2 = float32(ev); planarity = float32((ev1 - ev0) / ev2), linearity = float32((ev2 - ev1) / ev2),
                   both 0 when ev2 <= 0.  n < 3: eight zeros.
"""
import numpy as np

import world_map_ref as R

F32 = np.float32
SD, VIEW, PROD = [0, 1, 2], [3, 7, 11], [4, 5, 6, 8, 9, 10]     # where the sums sit among the 12 floats


def origin(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.array([T[0, 3], T[1, 3], T[2, 3]], np.float64).astype(np.float32)


def centre(i, leaf):
    return (F32(i) + F32(0.5)) * F32(leaf)


def add_point(m, w, c, o):
    """One point into the 12 float32 of m, np.float32 scalars in the order of mml_wm_add_moments.  w, c, o: world point, voxel
    centre, sensor origin (3 float32 each)."""
    dx, dy, dz = F32(w[0]) - F32(c[0]), F32(w[1]) - F32(c[1]), F32(w[2]) - F32(c[2])
    m[0] = m[0] + dx
    m[1] = m[1] + dy
    m[2] = m[2] + dz
    for at, p in zip(PROD, (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
        m[at] = m[at] + F32(p)
    for at, r in zip(VIEW, range(3)):
        m[at] = m[at] + (F32(o[r]) - F32(w[r]))
    return m


def point_rows(w, c, o):
    """(n, 12) float32: what each of n points of ONE voxel adds, in the layout of the accumulator."""
    w = np.asarray(w, np.float32).reshape(-1, 3)
    d = w - np.asarray(c, np.float32)[None]
    rows = np.zeros((len(w), 12), np.float32)
    rows[:, SD] = d
    rows[:, PROD] = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    rows[:, VIEW] = np.asarray(o, np.float32).reshape(-1, 3) - w
    return rows


def covariance(mom, n):
    """(m, 12) float32 moments, (m,) counts >= 1 -> (m, 6) float64: Cxx Cxy Cyy Cxz Cyz Czz, the solver's m00 m10 m11 m20 m21 m22."""
    mom = np.asarray(mom, np.float32).reshape(-1, 12).astype(np.float64)
    nd = np.asarray(n).astype(np.float64)
    mx, my, mz = mom[:, 0] / nd, mom[:, 1] / nd, mom[:, 2] / nd
    return np.stack([mom[:, 4] / nd - mx * mx, mom[:, 5] / nd - mx * my, mom[:, 8] / nd - my * my, mom[:, 6] / nd - mx * mz,
                     mom[:, 9] / nd - my * mz, mom[:, 10] / nd - mz * mz], 1)


def surfels(O, mom, n):
    """(m, 8) float32 surfel records of m voxels; O: the oracle module (its eig3 is the device's, bit for bit)."""
    mom = np.asarray(mom, np.float32).reshape(-1, 12)
    n = np.asarray(n).reshape(-1)
    out = np.zeros((len(mom), 8), np.float32)
    sel = np.flatnonzero(n >= 3)
    if len(sel) == 0:
        return out
    e = O.model_fit5(0, covariance(mom[sel], n[sel]))
    ev, v0 = e[:, :3], e[:, 3:6].copy()
    V = mom[sel][:, VIEW].astype(np.float64)
    dot = (v0[:, 0] * V[:, 0] + v0[:, 1] * V[:, 1]) + v0[:, 2] * V[:, 2]
    v0[dot < 0] = -v0[dot < 0]
    with np.errstate(all="ignore"):
        flat = ev[:, 2] <= 0
        den = np.where(flat, 1.0, ev[:, 2])
        planarity = np.where(flat, 0.0, (ev[:, 1] - ev[:, 0]) / den)
        linearity = np.where(flat, 0.0, (ev[:, 2] - ev[:, 1]) / den)
        out[sel, :3] = v0.astype(np.float32)
        out[sel, 3:6] = ev.astype(np.float32)
        out[sel, 6] = planarity.astype(np.float32)
        out[sel, 7] = linearity.astype(np.float32)
    return out


class SurfelMapRef(R.WorldMapRef):
    """WorldMapRef with the moments beside the sums: self.mom, key -> 12 float32."""

    def __init__(self, leaf):
        super().__init__(leaf)
        self.leaf = F32(leaf)
        self.mom = {}

    def add_world(self, map, xyzi, labels=None, label_mask=7, o=(0.0, 0.0, 0.0)):
        """World points (n, 4) of `map` seen from the sensor origin(s) o -- (3,) for all or (n, 3) --, in the order given."""
        xyzi = np.asarray(xyzi, np.float32).reshape(-1, 4)
        o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), (len(xyzi), 3))
        before = set(self.vox)
        super().add_world(map, xyzi, labels, label_mask)
        # the points the base class kept, by its rules (mask, finite, range, the empty marker's voxel), and their keys
        labels = np.zeros(len(xyzi), np.int64) if labels is None else np.asarray(labels).astype(np.int64)
        ok = np.isin(labels, [l for l in (0, 1, 2) if (label_mask >> l) & 1]) & np.isfinite(xyzi).all(axis=1)
        with np.errstate(all="ignore"):
            f = np.floor((xyzi[:, :3] * self.inv).astype(np.float64))     # (R.axis_index on whole arrays)
        ok &= ((f >= -R.HALF) & (f < R.HALF)).all(axis=1)
        rows = {}
        for r in np.flatnonzero(ok):
            key = R.pack(map, int(f[r, 0]), int(f[r, 1]), int(f[r, 2]))
            if key != R.EMPTY:
                rows.setdefault(key, []).append(r)
        assert set(rows) - before == set(self.vox) - before and set(rows) <= set(self.vox)
        for key, rr in rows.items():
            _, i, j, k = R.unpack(key)
            c = np.array([centre(i, self.leaf), centre(j, self.leaf), centre(k, self.leaf)], np.float32)
            start = self.mom.get(key, np.zeros(12, np.float32))
            self.mom[key] = np.cumsum(np.concatenate([start[None], point_rows(xyzi[rr, :3], c, o[rr])]), axis=0, dtype=np.float32)[-1]

    def add(self, map, xyz, intensity, T, labels=None, label_mask=7):
        w = R.world_points(xyz, T)
        self.add_world(map, np.concatenate([w, np.asarray(intensity, np.float32).reshape(-1, 1)], axis=1), labels, label_mask, origin(T))

    def add_records(self, map, rec, T, label_mask=7):
        """(n, 12) float32 registered-cloud records, already in the world frame at the pose T (whose translation is the origin)."""
        rec = np.asarray(rec, np.float32).reshape(-1, 12)
        self.add_world(map, rec[:, [0, 1, 2, 8]], rec[:, 6].astype(np.int64), label_mask, origin(T))

    def reset(self, map=-1):
        super().reset(map)
        self.mom = {k: v for k, v in self.mom.items() if k in self.vox}

    def moments(self, map):
        """((n, 12) float32, (n,) int32 counts) of one map in ascending key order."""
        keys = sorted(k for k in self.vox if (k >> 54) == map)
        out = np.zeros((len(keys), 12), np.float32)
        for r, k in enumerate(keys):
            out[r] = self.mom[k]
        return out, np.array([self.vox[k][1] for k in keys], np.int32)

    def surfels(self, O, map):
        return surfels(O, *self.moments(map))
