"""A numpy restatement of the pose score and the relocalisation search (csrc/world_map_score.h, include/mmloam_hip.h
"relocalisation in a surfel world map"), independent of the library and built on tests/world_map_assoc_ref.py: the table of a map
is A.surfel_table's (centroid, count, surfel record per key), the steps of a feature are A.associate's up to the gates, restated
over whole arrays so that a few ten thousand feature-hypothesis pairs take a second.

    features      0, stride, 2 stride, ... of the stack
    status        0 skipped (no voxel: not counted), 1 no candidate, 2 planarity, 3 distance, 4 match -- A.associate's reasons
    match         q = trunc((1.0 - |d| / max_plane_dist) * 65536.0) in float64 (0 when d is not a number)
    result        score_q = sum q, n_match, n_scored = the features not skipped: integers
    ranking       the larger score_q, then the larger n_match, then the smaller index
    search        level 0: the grid around the seed; the `keep` best; each further level: steps / refine, the grids of +-1
                  previous step around the kept hypotheses in their order; the best of the last level is T_start
The hypotheses of a grid come from the caller (`grid`: the C function through ctypes in the device tests, whose poses
tests/test_world_map_pose_grid.py holds to 1e-15 of pose_grid below)."""
import math

import numpy as np

import world_map_assoc_ref as A
import world_map_ref as R

SCORE_DT = np.dtype([("score_q", np.uint64), ("n_match", np.int32), ("n_scored", np.int32)])
SKIPPED, NONE, PLANARITY, DISTANCE, MATCH = range(5)


def options(leaf, stride=1, **over):
    return dict(A.options(leaf, **over), stride=stride)


class Table:
    """one map's voxels as arrays in key order: keys (uint64), float32 centroids, counts, float32 surfel records"""

    def __init__(self, table, map):
        keys = sorted(table)
        self.map = map
        self.keys = np.array(keys, np.uint64)
        self.cen = np.array([table[k][0] for k in keys], np.float32).reshape(-1, 3)
        self.cnt = np.array([table[k][1] for k in keys], np.int64)
        self.sur = np.array([table[k][2] for k in keys], np.float32).reshape(-1, 8)


def table_of(ref, O, map):
    return Table(A.surfel_table(ref, O, map), map)


def statuses(tab, inv, feats, T, o):
    """(H, m) status and (H, m) uint64 q of the strided features of `feats` at the poses T (H, 4, 4)"""
    feats = np.asarray(feats, np.float32).reshape(-1, 3)[::o["stride"]]
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    H, m = len(T), len(feats)
    W = np.stack([R.world_points(feats, t) for t in T]).reshape(H * m, 3) if m else np.zeros((0, 3), np.float32)
    with np.errstate(all="ignore"):
        f = np.floor((W * R.F32(inv)).astype(np.float64))                 # the product in float32, floor of its double
        ok = np.isfinite(W).all(axis=1) & ((f >= -R.HALF) & (f < R.HALF)).all(axis=1)
    ijk = np.where(ok[:, None], f, 0).astype(np.int64)
    n = len(W)
    best_r2, best_key, best_at = np.zeros(n), np.zeros(n, np.uint64), np.full(n, -1, np.int64)
    rng = (-1, 0, 1) if o["neighbourhood"] else (0,)
    Wd = W.astype(np.float64)
    for dk in rng:
        for dj in rng:
            for di in rng:
                c = ijk + np.array([di, dj, dk])
                inr = ok & ((c >= -R.HALF) & (c < R.HALF)).all(axis=1)
                u = (np.where(inr[:, None], c, 0) + R.HALF).astype(np.uint64)
                key = (np.uint64(tab.map) << np.uint64(54)) | (u[:, 2] << np.uint64(36)) | (u[:, 1] << np.uint64(18)) | u[:, 0]
                at = np.searchsorted(tab.keys, key)
                at = np.where(at < len(tab.keys), at, 0)
                held = inr & (key != np.uint64(R.EMPTY)) & (len(tab.keys) > 0)
                if len(tab.keys):
                    held &= (tab.keys[at] == key) & (tab.cnt[at] >= o["min_points"])
                else:
                    continue
                d = Wd - tab.cen[at].astype(np.float64)
                r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                take = held & ((best_at < 0) | (r2 < best_r2) | ((r2 == best_r2) & (key < best_key)))
                best_r2, best_key, best_at = np.where(take, r2, best_r2), np.where(take, key, best_key), np.where(take, at, best_at)
    status = np.where(ok, NONE, SKIPPED)
    q = np.zeros(n, np.uint64)
    has = best_at >= 0
    if has.any():
        at = np.where(has, best_at, 0)
        plan = tab.sur[at, 6]
        nrm = tab.sur[at, :3].astype(np.float64)
        dw = Wd - tab.cen[at].astype(np.float64)
        with np.errstate(all="ignore"):
            d = (nrm[:, 0] * dw[:, 0] + nrm[:, 1] * dw[:, 1]) + nrm[:, 2] * dw[:, 2]
            low = plan < o["min_planarity"]
            far = np.abs(d) > o["max_plane_dist"]
            v = (1.0 - np.abs(d) / o["max_plane_dist"]) * 65536.0
        status = np.where(has, np.where(low, PLANARITY, np.where(far, DISTANCE, MATCH)), status)
        q = np.where((status == MATCH) & (v >= 0.0), np.trunc(np.where(v >= 0.0, v, 0.0)), 0.0).astype(np.uint64)
    return status.reshape(H, m), q.reshape(H, m)


def score(tab, inv, feats, T, o):
    """(H,) SCORE_DT of the stack `feats` at the poses T"""
    st, q = statuses(tab, inv, feats, T, o)
    out = np.zeros(len(st), SCORE_DT)
    out["score_q"] = q.sum(axis=1, dtype=np.uint64)
    out["n_match"] = (st == MATCH).sum(axis=1)
    out["n_scored"] = (st != SKIPPED).sum(axis=1)
    return out


def ranking(s):
    """the indices of the results s, best first"""
    return sorted(range(len(s)), key=lambda h: (-int(s["score_q"][h]), -int(s["n_match"][h]), h))


# ---- the grid ----
def cells(half, step):
    return 0 if half == 0.0 else int(math.floor(half / step + 1e-9))


def shape(half_xy, step_xy, half_z, step_z, half_yaw, step_yaw):
    """(kx, kz, kw, nx, nz, nw, cyclic)"""
    kx, kz, kw = cells(half_xy, step_xy), cells(half_z, step_z), cells(half_yaw, step_yaw)
    cyclic = kw > 0 and abs(2.0 * kw * step_yaw - 2.0 * math.pi) <= 1e-9
    return kx, kz, kw, 2 * kx + 1, 2 * kz + 1, 2 * kw + 1 - (1 if cyclic else 0), cyclic


def pose_grid(seed, half_xy, step_xy, half_z, step_z, half_yaw, step_yaw):
    """(H, 4, 4): Trans(t_seed + delta) Rz(yaw) R_seed, index ((iyaw nz + iz) ny + iy) nx + ix"""
    seed = np.asarray(seed, np.float64).reshape(4, 4)
    kx, kz, kw, nx, nz, nw, _ = shape(half_xy, step_xy, half_z, step_z, half_yaw, step_yaw)
    out = np.zeros((nw, nz, nx, nx, 4, 4))
    for iw in range(nw):
        yaw = (iw - kw) * step_yaw
        c, s = math.cos(yaw), math.sin(yaw)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        for iz in range(nz):
            for iy in range(nx):
                for ix in range(nx):
                    T = np.eye(4)
                    T[:3, :3] = Rz @ seed[:3, :3]
                    T[:3, 3] = seed[:3, 3] + [(ix - kx) * step_xy, (iy - kx) * step_xy, (iz - kz) * step_z]
                    out[iw, iz, iy, ix] = T
    return out.reshape(-1, 4, 4)


def search(tab, inv, feats, seed, g, o, grid):
    """The levels of mml_world_map_relocalize for one slot.  g: dict(half_xy, step_xy, half_z, step_z, half_yaw, step_yaw, levels,
    refine, keep); grid(seed, half_xy, step_xy, half_z, step_z, half_yaw, step_yaw) -> (H, 4, 4).  Returns dict(best, second,
    n_hyp_scored, T_start, level0=(poses, scores, order))."""
    step = [g["step_xy"], g["step_z"], g["step_yaw"]]
    half = [g["half_xy"], g["half_z"], g["half_yaw"]]
    seeds, total, out = [np.asarray(seed, np.float64).reshape(4, 4)], 0, {}
    for level in range(g["levels"]):
        T = np.concatenate([grid(s, half[0], step[0], half[1], step[1], half[2], step[2]) for s in seeds])
        s = score(tab, inv, feats, T, o)
        order = ranking(s)
        total += len(T)
        if level == 0:
            kx, kz, kw, nx, nz, nw, cyclic = shape(half[0], step[0], half[1], step[1], half[2], step[2])
            b = order[0]
            at = lambda h: (h % nx, (h // nx) % nx, (h // (nx * nx)) % nz, h // (nx * nx * nz))
            second = np.zeros((), SCORE_DT)
            for h in order:
                d = [abs(p - q) for p, q in zip(at(h), at(b))]
                if cyclic:
                    d[3] = min(d[3], nw - d[3])
                if max(d) > 1:
                    second = s[h]
                    break
            out.update(best=s[b], second=second, level0=(T, s, order))
        seeds = [T[h] for h in order[:g["keep"]]]
        ks = shape(half[0], step[0], half[1], step[1], half[2], step[2])[:3]
        half = [step[a] if ks[a] else 0.0 for a in range(3)]          # (an axis of one cell stays one cell)
        step = [v / g["refine"] for v in step]
    out.update(n_hyp_scored=total, T_start=seeds[0])
    return out
