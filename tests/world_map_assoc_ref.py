"""A numpy restatement of localisation in a surfel map (csrc/world_map_assoc.h, include/mmloam_hip.h "localisation in a surfel
world map"), independent of the library: built on tests/world_map_surfel_ref.py (SurfelMapRef: sums, counts, moments, surfels)
and, for the loop, on the oracle's solve.

    world point   w = float32 world point of feature f at the pose T (world_map_ref.world_points); the feature is skipped when a
                  coordinate is not finite or an index floor(float64(w * inv)) leaves [-2^17, 2^17)
    candidates    the voxel of w, or the 27 around it that lie in range (the packed key of the free marker excluded), held by the
                  map with count >= min_points; c = sum.xyz / float32(count); r2 = ((wx-cx)^2 + (wy-cy)^2) + (wz-cz)^2 in
                  float64; the smallest r2 wins, ties to the smaller packed key
    gates         the winner's surfel (nx ny nz planarity as float32): planarity < min_planarity -> none; d = (nx (wx-cx) +
                  ny (wy-cy)) + nz (wz-cz) in float64; |d| > max_plane_dist -> none
    record        ori = f, proj = w - d n, omega = n, error = |T f - proj| with T f in float64 from the float32 f
    loop          mml_estimate's: x = [P, log Q], associate at the pose, solve (the oracle's), deltaR < 0.05 deg and deltaT < 0.05
"""
import numpy as np

import world_map_ref as R
import world_map_surfel_ref as S

DEFAULTS = dict(neighbourhood=1, min_points=5, min_planarity=np.float32(0.5))


def options(leaf, **over):
    o = dict(DEFAULTS, max_plane_dist=float(np.float32(leaf)))
    o.update(over)
    o["min_planarity"] = np.float32(o["min_planarity"])
    return o


def tf_points(T, f):
    """T f in float64 from float32 points, ((T0 x + T1 y) + T2 z) + T3"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(f, np.float32).reshape(-1, 3).astype(np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def surfel_table(ref, O, map):
    """key -> (float32 centroid xyz, count, float32 surfel record) of one map"""
    keys = sorted(k for k in ref.vox if (k >> 54) == map)
    sur = ref.surfels(O, map)
    return {k: (ref.vox[k][0][:3] / R.F32(ref.vox[k][1]), ref.vox[k][1], sur[r]) for r, k in enumerate(keys)}


def choose(table, map, w, inv, o):
    """The winner of one world point: (key, centroid, surfel) or None; and why not ('skipped', 'none')."""
    if not np.isfinite(w).all():
        return None, "skipped"
    ijk = [R.axis_index(v, inv) for v in w]
    if any(i is None for i in ijk):
        return None, "skipped"
    best = None
    rng = (-1, 0, 1) if o["neighbourhood"] else (0,)
    for dk in rng:
        for dj in rng:
            for di in rng:
                i, j, k = ijk[0] + di, ijk[1] + dj, ijk[2] + dk
                if not all(-R.HALF <= v < R.HALF for v in (i, j, k)):
                    continue
                key = R.pack(map, i, j, k)
                if key == R.EMPTY or key not in table or table[key][1] < o["min_points"]:
                    continue
                c = table[key][0]
                d = w.astype(np.float64) - c.astype(np.float64)
                r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if best is None or r2 < best[0] or (r2 == best[0] and key < best[1]):
                    best = (r2, key)
    if best is None:
        return None, "none"
    return (best[1],) + table[best[1]][::2], "ok"


def associate(ref, O, map, feats, T, o, table=None):
    """(m, 10) float64 plane records (ori, proj, omega, error) and (m,) int32 src of the surf stack `feats` at the pose T."""
    feats = np.asarray(feats, np.float32).reshape(-1, 3)
    table = surfel_table(ref, O, map) if table is None else table
    with np.errstate(all="ignore"):
        W = R.world_points(feats, T)
        P = tf_points(T, feats)
    rec, src, why = [], [], []
    for s in range(len(feats)):
        w = W[s]
        win, reason = choose(table, map, w, ref.inv, o)
        if win is None:
            why.append(reason)
            continue
        _, c, sur = win
        if sur[6] < o["min_planarity"]:
            why.append("planarity")
            continue
        n = sur[:3].astype(np.float64)
        dw = w.astype(np.float64) - c.astype(np.float64)
        d = (n[0] * dw[0] + n[1] * dw[1]) + n[2] * dw[2]
        if abs(d) > o["max_plane_dist"]:
            why.append("distance")
            continue
        proj = w.astype(np.float64) - d * n
        e = P[s] - proj
        rec.append(np.concatenate([feats[s].astype(np.float64), proj, n, [np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])]]))
        src.append(s)
        why.append("factor")
    return np.array(rec, np.float64).reshape(-1, 10), np.array(src, np.int32), why


def stats(O, rec):
    """n_plane, n_plane_used, the normal Gram matrix (9,), min_singular and is_degenerate of a slot's plane records"""
    om = rec[:, 6:9]
    gram = (om[:, :, None] * om[:, None, :]).sum(axis=0).reshape(9) if len(rec) else np.zeros(9)
    ms = -1.0
    if len(rec) > 10:
        ms = float(np.sqrt(max(np.linalg.eigvalsh(gram.reshape(3, 3))[0], 0.0)))
    return dict(n_line=0, n_plane=len(rec), n_line_used=0, n_plane_used=int((np.abs(rec[:, 9]) > 1e-5).sum()), gram=gram, min_singular=ms,
                is_degenerate=int(ms < 3.0))


def plane_factors(O, rec):
    pf = np.zeros(len(rec), O.PLANE_DT)
    pf["point_ori"], pf["point_proj"], pf["omega"], pf["error"] = rec[:, :3], rec[:, 3:6], rec[:, 6:9], rec[:, 9]
    return pf


def pose_matrix(O, P, Q, T_bl):
    from scipy.spatial.transform import Rotation as Rsc
    T = np.eye(4)
    T[:3, :3] = Rsc.from_quat(Q).as_matrix()
    T[:3, 3] = P
    return T @ T_bl


def localize(ref, O, map, feats, exTlb, P, Q, leaf, by_outer, max_outer=5, inner_iters=10, **over):
    """mml_world_map_localize for one slot: (P, Q, outer iterations, the factor count of every outer iteration, degenerate)."""
    P, Q = np.asarray(P, np.float64).copy(), np.asarray(Q, np.float64).copy()
    T_bl = np.linalg.inv(np.asarray(exTlb, np.float64).reshape(4, 4))
    table = surfel_table(ref, O, map)
    counts, degenerate, it = [], 0, 0
    for it in range(max_outer):
        x = np.concatenate([P, O.so3_log(Q)])
        o = options(leaf, max_plane_dist=by_outer[min(it, 2)], **over)
        rec, _, _ = associate(ref, O, map, feats, pose_matrix(O, P, Q, T_bl), o, table)
        counts.append(len(rec))
        degenerate |= stats(O, rec)["is_degenerate"]
        xs, _, _ = O.solve_window([np.zeros(0, O.LINE_DT)], [plane_factors(O, rec)], x[None], T_bl, inner_iters)
        qa = O.so3_exp(xs[0, 3:])
        from scipy.spatial.transform import Rotation as Rsc
        dR = np.degrees((Rsc.from_quat(Q) * Rsc.from_quat(qa).inv()).magnitude())
        dT = np.linalg.norm(P - xs[0, :3])
        P, Q = xs[0, :3].copy(), qa
        if dR < 0.05 and dT < 0.05:
            break
    return P, Q, it + 1, counts, degenerate
