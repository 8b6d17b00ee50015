"""Scoring H pose hypotheses per slot against a finished surfel map, two ways, alternated in one run on one context:
  (associate) the way open before mml_world_map_score: one mml_world_map_associate with `stats` per hypothesis, all n slots per
              call, n_plane taken as the score -- one launch, one eigen-solve per feature and host synchronisations per hypothesis;
  (score)     one mml_world_map_score for the n slots and their H hypotheses.
    python tools/world_map_score_probe.py [--out <table>] [--isa <file>] [--resources <file>]
For n = 1, 8 slots and H = 64, 1 024, 8 192 hypotheses per slot; order associate, score, associate, score.  Written per size: the
wall time of each run (host clock around the calls), and how many of the n x H n_match differ from the n_plane of the other way
(none may).  Then the surfel cache on its own: a score call of one hypothesis right after the map was exported, reset and imported
again (the cache is stale and is rebuilt in front of the score) against the same call repeated (the cache is valid), for a table
of 4 096 and of 524 288 positions.  --isa / --resources: files whose lines are copied into the table (tools/isa_compare.py against
the parent commit for world_map.hip and world_map_assoc.hip; the kernel-resource-usage remarks of k_wm_score and
k_wm_surfel_cache).  No speed-up is claimed or gated: the values are one run on one box.

Scene: the inside of a 4 x 3 x 2 m room, leaf 0.5 m, the map from two scans of 9000 points, every slot a scan of 2000 surf
features of its own; the hypotheses are mml_wm_pose_grid's around the slot's pose (x, y and yaw), the first H of a grid that holds
at least H."""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation as Rsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEAF = 0.5
BOX = np.array([2.0, 1.5, 1.0])


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


def hypotheses(M, T, H):
    """the first H cells of a grid around T: 9 x 9 in x and y, as many yaw cells as H needs"""
    yaw = max(1, math.ceil(H / 81.0))
    k = yaw // 2 + 1
    g = M.wm_pose_grid(T, 0.4, 0.1, 0.0, 1.0, 0.02 * k, 0.02)
    assert len(g) >= H
    return g[:H]


def make_map(M, ctx, rng, capacity):
    ctx.world_map_create(1, LEAF, capacity, surfels=True)
    for s, T in enumerate((shift([0.2, 0.1, 0.0]), shift([-0.5, 0.3, 0.2], [0.0, 0.0, 0.4]))):
        ctx.cloud_upload(s, records(sensor_frame(box_points(rng, 9000, 0.003), T)), 4500)
        ctx.world_map_add(s, [0], T)


def run_size(M, n, sizes, out):
    rng = np.random.default_rng(200 + n)
    ctx = M.Context(max_scans=max(n, 2), max_velo_points=8192, max_livox_points=8192, max_features=2048)
    try:
        make_map(M, ctx, rng, 2048)
        poses, feats = [], []
        for s in range(n):
            truth = shift(rng.uniform(-0.3, 0.3, 3), [0.0, 0.0, rng.uniform(-0.3, 0.3)])
            poses.append(truth)
            feats.append(sensor_frame(box_points(rng, 2000, 0.002), truth))
            ctx.features_upload(s, 0, np.zeros((0, 3), np.float32))
            ctx.features_upload(s, 1, feats[s])
        ao, so = M.wm_assoc_opts(LEAF), M.wm_score_opts(LEAF)
        ctx.world_map_score(0, [0] * n, np.stack(poses)[:, None], so)          # (the cache is built before anything is timed)
        for H in sizes:
            T = np.stack([hypotheses(M, poses[s], H) for s in range(n)])       # (n, H, 4, 4)
            res = {}
            for rep in range(2):
                for way in ("associate", "score"):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    if way == "associate":
                        planes = np.zeros((n, H), np.int64)
                        for h in range(H):
                            st = ctx.world_map_associate(0, [0] * n, T[:, h], ao)
                            planes[:, h] = [x.n_plane for x in st]
                        res[way] = planes
                    else:
                        res[way] = ctx.world_map_score(0, [0] * n, T, so)["n_match"].astype(np.int64)
                    dt = time.perf_counter() - t0
                    out.append("n = %d  H = %5d  run %d  %-9s  %10.2f ms  (%8.2f us per slot and hypothesis)" % (n, H, rep, way, 1e3 * dt, 1e6 * dt / (n * H)))
            out.append("n = %d  H = %5d  n_match against n_plane: %d of %d differ; matches per hypothesis %d .. %d" % (
                n, H, int((res["associate"] != res["score"]).sum()), n * H, res["score"].min(), res["score"].max()))
    finally:
        ctx.close()


def cache_alone(M, capacity, out):
    rng = np.random.default_rng(7)
    ctx = M.Context(max_scans=2, max_velo_points=8192, max_livox_points=8192, max_features=2048)
    try:
        make_map(M, ctx, rng, capacity)
        T = shift([0.1, -0.1, 0.05])
        ctx.features_upload(0, 0, np.zeros((0, 3), np.float32))
        ctx.features_upload(0, 1, sensor_frame(box_points(rng, 2000, 0.002), T))
        so = M.wm_score_opts(LEAF)
        ctx.world_map_score(0, [0], T[None, None], so)                         # (allocates the cache)
        for rep in range(3):
            ex = ctx.world_map_export(0)
            ctx.world_map_reset(0)
            ctx.world_map_import(0, **ex)
            times = []
            for state in ("stale", "valid"):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.world_map_score(0, [0], T[None, None], so)
                times.append(time.perf_counter() - t0)
            out.append("table of %7d positions (%d voxels held)  run %d  score of one hypothesis: cache stale %8.1f us, valid %8.1f us, difference %8.1f us" % (
                2 * capacity, ctx.world_map_size(0), rep, 1e6 * times[0], 1e6 * times[1], 1e6 * (times[0] - times[1])))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_score_probe.txt"))
    ap.add_argument("--isa")
    ap.add_argument("--resources")
    a = ap.parse_args()
    M = importlib.import_module("multi-modal-loam_amd")
    import torch
    out = ["world_map_score_probe: %s, one run, nothing gated and no speed-up claimed" % torch.cuda.get_device_name(0),
           "associate = one mml_world_map_associate with stats per hypothesis, n_plane as the score; score = one mml_world_map_score", ""]
    for n in (1, 8):
        run_size(M, n, (64, 1024, 8192), out)
        out.append("")
    out += ["the surfel cache on its own (k_wm_surfel_cache, one lane per table position, in front of the score):"]
    for capacity in (2048, 262144):
        cache_alone(M, capacity, out)
    out.append("")
    for title, path in (("k_wm_score and k_wm_surfel_cache, -Rpass-analysis=kernel-resource-usage:", a.resources),
                        ("tools/isa_compare.py, world_map.hip and world_map_assoc.hip of the parent commit against this one:", a.isa)):
        if path:
            out += [title] + ["  " + l.rstrip() for l in open(path)] + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
