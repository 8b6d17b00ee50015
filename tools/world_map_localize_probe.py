"""Localising n scans in a finished surfel map, two ways, alternated in one run on one context:
  (host)   what a caller does without mml_world_map_localize: the centroids, counts and surfels of the map downloaded once
           (world_map_download, world_map_surfels), then per outer iteration the association in numpy (27 voxels per feature,
           vectorised, float64), mml_factors_upload per slot (an empty line list and the plane records), ONE mml_solve for all
           slots, and mml_estimate's convergence test on the host;
  (device) one mml_world_map_localize for the n slots.
    python tools/world_map_localize_probe.py [--out <table>] [--isa <file>] [--resources <file>] [n ...]
Defaults: n = 1, 8, 64 slots; order host, device, host, device, the stacks uploaded again before every run.  Written per size: the
wall time of each run (host clock around the whole localisation), the outer iterations, and the largest difference between the
final poses of the two ways over all slots (the host way sums in float64 and takes the voxel of a centroid from the centroid, so
the two are close, not equal).  --isa / --resources: files whose lines are copied into the table (tools/isa_compare.py against
the parent commit for world_map.hip; the kernel-resource-usage remarks of k_wm_associate).  No speed-up is claimed or gated: the
values are one run on one box.

Scene: the inside of a 4 x 3 x 2 m room, leaf 0.5 m, the map from two scans of 9000 points, every slot a scan of 2000 surf
features of its own from a pose a few centimetres and about a degree off."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation as Rsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEAF = 0.5
HALF = 1 << 17
BOX = np.array([2.0, 1.5, 1.0])
BY_OUTER = [2 * LEAF, LEAF, 0.5 * LEAF]


def shift(t, rotvec=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = Rsc.from_rotvec(rotvec).as_matrix()
    T[:3, 3] = t
    return T


def box_points(rng, n, noise):
    p = rng.uniform(-1, 1, (n, 3)) * BOX
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = rng.choice([-1.0, 1.0], n) * BOX[axis] + rng.normal(0, noise, n)
    return p + [0.3, -0.2, 0.1]


def sensor_frame(world, T):
    return ((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def records(xyz):
    rec = np.zeros((len(xyz), 12), np.float32)
    rec[:, :3], rec[:, 3], rec[:, 8] = xyz, 1.0, 1.0
    return rec


def pack(ijk):
    v = ijk.astype(np.int64) + HALF
    return (v[..., 2] << 36) | (v[..., 1] << 18) | v[..., 0]


class HostMap:
    """the map as the downloads hand it out: keys (ascending, as the rows are), centroids, counts, normals, planarity"""

    def __init__(self, ctx, map):
        cen, cnt = ctx.world_map_download(map, counts=True)
        sur = ctx.world_map_surfels(map)
        self.keys = pack(np.floor(cen[:, :3] * (np.float32(1.0) / np.float32(LEAF))))
        order = np.argsort(self.keys)
        self.keys, self.cen, self.cnt = self.keys[order], cen[order, :3].astype(np.float64), cnt[order]
        self.nrm, self.planarity = sur[order, :3].astype(np.float64), sur[order, 6]
        self.bytes = cen.nbytes + cnt.nbytes + sur.nbytes

    def associate(self, feats, T, max_dist, min_points=5, min_planarity=0.5):
        """(m, 10) plane records of one slot's surf stack at the pose T"""
        f = feats.astype(np.float64)
        w = (f @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        ijk = np.floor(w * (np.float32(1.0) / np.float32(LEAF))).astype(np.int64)
        w = w.astype(np.float64)
        best_r2, best = np.full(len(f), np.inf), np.full(len(f), -1)
        for dk in (-1, 0, 1):
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    key = pack(ijk + [di, dj, dk])
                    at = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
                    ok = (self.keys[at] == key) & (self.cnt[at] >= min_points)
                    r2 = ((w - self.cen[at]) ** 2).sum(axis=1)
                    take = ok & (r2 < best_r2)
                    best_r2[take], best[take] = r2[take], at[take]
        sel = np.flatnonzero(best >= 0)
        at = best[sel]
        sel, at = sel[self.planarity[at] >= min_planarity], at[self.planarity[at] >= min_planarity]
        d = ((w[sel] - self.cen[at]) * self.nrm[at]).sum(axis=1)
        keep = np.abs(d) <= max_dist
        sel, at, d = sel[keep], at[keep], d[keep]
        proj = w[sel] - d[:, None] * self.nrm[at]
        err = np.linalg.norm(f[sel] @ T[:3, :3].T + T[:3, 3] - proj, axis=1)
        return np.concatenate([f[sel], proj, self.nrm[at], err[:, None]], axis=1)


def host_localize(ctx, hm, feats, P, Q, max_outer=5, inner_iters=10):
    n = len(feats)
    P, Q = P.copy(), Q.copy()
    done, outer = np.zeros(n, bool), np.zeros(n, int)
    for it in range(max_outer):
        if done.all():
            break
        x = np.concatenate([P, Rsc.from_quat(Q).as_rotvec()], axis=1)
        for s in range(n):
            T = shift(P[s])
            T[:3, :3] = Rsc.from_quat(Q[s]).as_matrix()
            ctx.factors_upload(s, 0, np.zeros((0, 10)))
            ctx.factors_upload(s, 1, hm.associate(feats[s], T, BY_OUTER[min(it, 2)]))
        xs, _, _ = ctx.solve(0, n, x, np.eye(4), max_iters=inner_iters)
        for s in np.flatnonzero(~done):
            qa = Rsc.from_rotvec(xs[s, 3:])
            dR = np.degrees((Rsc.from_quat(Q[s]) * qa.inv()).magnitude())
            dT = np.linalg.norm(P[s] - xs[s, :3])
            P[s], Q[s], outer[s] = xs[s, :3], qa.as_quat(), it + 1
            done[s] = (dR < 0.05 and dT < 0.05) or it + 1 == max_outer
    return P, Q, outer


def run_size(M, n, out):
    rng = np.random.default_rng(100 + n)
    ctx = M.Context(max_scans=max(n, 2), max_velo_points=8192, max_livox_points=8192, max_features=2048)
    try:
        ctx.world_map_create(1, LEAF, 2048, surfels=True)
        for s, T in enumerate((shift([0.2, 0.1, 0.0]), shift([-0.5, 0.3, 0.2], [0.0, 0.0, 0.4]))):
            ctx.cloud_upload(s, records(sensor_frame(box_points(rng, 9000, 0.003), T)), 4500)
            ctx.world_map_add(s, [0], T)
        feats, P0, Q0 = [], np.zeros((n, 3)), np.zeros((n, 4))
        for s in range(n):
            truth = shift(rng.uniform(-0.3, 0.3, 3), [0.0, 0.0, rng.uniform(-0.3, 0.3)])
            feats.append(sensor_frame(box_points(rng, 2000, 0.002), truth))
            P0[s] = truth[:3, 3] + rng.uniform(-0.03, 0.03, 3)
            Q0[s] = (Rsc.from_matrix(truth[:3, :3]) * Rsc.from_rotvec(rng.uniform(-0.012, 0.012, 3))).as_quat()
        opts = M.wm_localize_opts(LEAF)
        results = {}
        for rep in range(2):
            for way in ("host", "device"):
                for s in range(n):
                    ctx.features_upload(s, 0, np.zeros((0, 3), np.float32))
                    ctx.features_upload(s, 1, feats[s])
                t0 = time.perf_counter()
                if way == "host":
                    hm = HostMap(ctx, 0)
                    P, Q, outer = host_localize(ctx, hm, feats, P0, Q0)
                else:
                    P, Q, info = ctx.world_map_localize(0, [0] * n, np.eye(4), P0, Q0, opts)
                    outer = np.array([i.outer_iterations for i in info])
                dt = time.perf_counter() - t0
                results[way] = (P, Q)
                out.append("n = %3d  run %d  %-6s  %9.2f ms  outer iterations %d .. %d%s" % (
                    n, rep, way, 1e3 * dt, outer.min(), outer.max(), "  (map read back once: %d bytes)" % hm.bytes if way == "host" else ""))
        dP = np.abs(results["host"][0] - results["device"][0]).max()
        dQ = min(np.abs(results["host"][1] - results["device"][1]).max(), np.abs(results["host"][1] + results["device"][1]).max())
        out.append("n = %3d  final poses, host against device over all slots: max |dP| = %.3e m, max |dQ| = %.3e" % (n, dP, dQ))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_localize_probe.txt"))
    ap.add_argument("--isa")
    ap.add_argument("--resources")
    ap.add_argument("sizes", nargs="*", type=int, default=[1, 8, 64])
    a = ap.parse_args()
    M = importlib.import_module("multi-modal-loam_amd")
    import torch
    out = ["world_map_localize_probe: %s, one run, nothing gated and no speed-up claimed" % torch.cuda.get_device_name(0),
           "host = downloads once + numpy association + mml_factors_upload per slot + one mml_solve per outer iteration; device = one mml_world_map_localize",
           ""]
    for n in a.sizes:
        run_size(M, n, out)
        out.append("")
    for title, path in (("k_wm_associate, -Rpass-analysis=kernel-resource-usage:", a.resources),
                        ("tools/isa_compare.py, world_map.hip of the parent commit against this one:", a.isa)):
        if path:
            out += [title] + ["  " + l.rstrip() for l in open(path)] + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
