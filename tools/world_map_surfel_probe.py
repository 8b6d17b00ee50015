"""What per-voxel normals cost: n sequences replayed through BatchLidarOdometry, three ways, alternated in one run:
  (a) world_map=(leaf, capacity): a plain world map, the yardstick;
  (b) world_map=(leaf, capacity, "surfels"): a surfel map, world_map_surfels(seq) of every sequence read at the end;
  (c) the only way to normals without the feature: no device map, Context.cloud_download_registered for the published scans each
      round, per-voxel moments summed on the host (numpy, float64, vectorised) and numpy.linalg.eigh over the voxels at the end.
    python tools/world_map_surfel_probe.py [--out <table>] [--rounds R] [--parent-lib <libmmloam_hip.so of the parent commit>]
                                           [--isa <file with the ISA comparison's lines>] [n ...]
Defaults: n = 1, 8, 64 sequences, 4 rounds.  Every size runs in a process of its own under its own time limit; inside it the
order is (a) (b) (c) (a) (b) (c) on fresh contexts.  With --parent-lib, (a) runs once more per size in a further process on that
library (through $MML_LIB_PATH): the plain map's speed before this feature.  Written per size: scans/s of each (host clock around
the whole replay loop: upload, extract, undistort, estimate, map, and for (b) / (c) the normals at the end), the bytes read back
per round for the map, and how far (c)'s normals lie from (b)'s (the largest angle over the voxels of at least 10 points whose
planarity exceeds 0.5; (c) sums in float64 about the origin, so the two are close, not equal).  No speed-up is claimed or gated;
the values are one run on one box.

Inputs: synth scans (16 rings x 450 azimuths + 6000 Livox points with sweep motion), sequence w on its own stretch of the
trajectory; leaf 0.2 m."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LEAF = 0.2
ADD_READBACK_BYTES = 32      # seven counters and the table's total, 4 bytes each (world_map.hip)


class HostNormals:
    """(c): float64 sums of 1, p, p p^T and of the view vector per voxel key, over the registered clouds of one sequence"""

    def __init__(self):
        self.keys = np.zeros(0, np.int64)
        self.sums = np.zeros((0, 13))

    def add(self, rec, T):
        p = rec[:, :3].astype(np.float64)
        ijk = np.floor(rec[:, :3] * (np.float32(1.0) / np.float32(LEAF))).astype(np.int64) + (1 << 17)
        key = (ijk[:, 2] << 36) | (ijk[:, 1] << 18) | ijk[:, 0]
        rows = np.concatenate([np.ones((len(p), 1)), p, p[:, [0, 0, 0, 1, 1, 2]] * p[:, [0, 1, 2, 1, 2, 2]], T[:3, 3][None] - p], 1)
        keys, inv = np.unique(np.concatenate([self.keys, key]), return_inverse=True)
        sums = np.zeros((len(keys), 13))
        np.add.at(sums, inv, np.concatenate([self.sums, rows]))
        self.keys, self.sums = keys, sums

    def normals(self):
        """(keys, counts, (n, 3) normals towards the view sum, planarity) in ascending key order"""
        n = self.sums[:, 0]
        m = self.sums[:, 1:4] / n[:, None]
        s = self.sums[:, 4:10] / n[:, None]
        C = np.zeros((len(n), 3, 3))
        for (a, b), col in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
            C[:, a, b] = C[:, b, a] = s[:, col] - m[:, a] * m[:, b]
        ev, vec = np.linalg.eigh(C)
        nrm = vec[:, :, 0]
        nrm = np.where(((nrm * self.sums[:, 10:13]).sum(1) < 0)[:, None], -nrm, nrm)
        with np.errstate(all="ignore"):
            planarity = np.where(ev[:, 2] > 0, (ev[:, 1] - ev[:, 0]) / ev[:, 2], 0.0)
        return self.keys, n, nrm, planarity


def replay(M, odometry, inp, n, rounds, variant, capacity):
    ctx = M.Context(max_scans=n, max_map_points=1 << 17)
    try:
        wm = {"a": (LEAF, capacity), "b": (LEAF, capacity, "surfels"), "c": None}[variant]
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2, increment="segmented", world_map=wm)
        host, back = [HostNormals() for _ in range(n)], 0
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(rounds):
            for w in range(n):
                ctx.scan_upload(w, inp[w][i][0], inp[w][i][1])
            ctx.extract(0, n)
            ctx.undistort(0, n, np.stack([inp[w][i][2].reshape(9) for w in range(n)]), np.stack([inp[w][i][3] for w in range(n)]))
            bat.estimate_lidar_pose(list(range(n)), np.stack([inp[w][i][4] for w in range(n)]), np.stack([inp[w][i][5] for w in range(n)]))
            pub = [w for w in range(n) if not bat.seq[w].fail_detected]
            for run in odometry._adjacent_runs(pub, lambda w: w):
                if variant != "c":
                    back += ADD_READBACK_BYTES
                    continue
                clouds = ctx.cloud_download_registered(run[0], len(run), np.stack([bat.seq[w].last_T for w in run]))
                for w, c in zip(run, clouds):
                    host[w].add(c, bat.seq[w].last_T)
                    back += 48 * len(c) + 4
        out = dict(voxels=0)
        if variant == "b":
            sur = [bat.world_map_surfels(w) for w in range(n)]
            out["voxels"] = int(sum(len(s) for s in sur))
            out["final_bytes"] = int(sum(s.nbytes for s in sur))
            out["first"] = (sur[0], ctx.world_map_download(0, counts=True)[1])
        elif variant == "c":
            nrm = [h.normals() for h in host]
            out["voxels"] = int(sum(len(k[0]) for k in nrm))
            out["first"] = nrm[0]
        ctx.synchronize()
        dt = time.perf_counter() - t0
        out.update(scans_per_s=n * rounds / dt, bytes_per_round=back / rounds)
        return out
    finally:
        ctx.close()


def worker(n, rounds, variants):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    from world_map_probe import inputs
    inp = inputs(synth, n, rounds)
    capacity = max(1 << 16, n * rounds * 13200)      # (every point its own voxel at the worst)
    runs = [(v, replay(M, odometry, inp, n, rounds, v, capacity)) for v in variants]
    r = dict(n=n, rounds=rounds, variants=variants)
    for v in set(variants):
        mine = [x for name, x in runs if name == v]
        r[v] = [x["scans_per_s"] for x in mine]
        r[v + "_bytes"] = mine[0]["bytes_per_round"]
        r[v + "_voxels"] = mine[0]["voxels"]
        if v == "b":
            r["b_final_bytes"] = mine[0]["final_bytes"]
    if "b" in variants and "c" in variants:
        (sur, cnt), (keys, hn, nrm, plan) = [x for name, x in runs if name == "b"][0]["first"], [x for name, x in runs if name == "c"][0]["first"]
        r["same_voxels"] = bool(len(sur) == len(keys) and (cnt == hn).all())
        if r["same_voxels"]:
            sel = (cnt >= 10) & (sur[:, 6] > 0.5)
            cos = np.clip((sur[sel, :3].astype(np.float64) * nrm[sel]).sum(1), -1, 1)
            r["compared"] = int(sel.sum())
            r["max_angle_deg"] = float(np.degrees(np.arccos(cos)).max()) if sel.any() else 0.0
    print("PROBE " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_surfel_probe.txt"))
    ap.add_argument("--worker", type=int, default=None)
    ap.add_argument("--variants", default="abcabc")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds the process of one size may take")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--isa", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker is not None:
        return worker(a.worker, a.rounds, list(a.variants))
    rows, parent = [], {}

    def child(n, variants, env=None):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n), "--rounds", str(a.rounds), "--variants", variants],
                             capture_output=True, text=True, timeout=a.limit, env=env)
        if out.returncode != 0:   # (nothing more is started on the device after a failure)
            sys.exit("the process of n = %d (%s) failed (%d): %s" % (n, variants, out.returncode, out.stderr[-2000:]))
        return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")][0]

    for n in a.sizes or [1, 8, 64]:
        rows.append(child(n, "abcabc"))
        if a.parent_lib:
            parent[n] = child(n, "aa", dict(os.environ, MML_LIB_PATH=os.path.abspath(a.parent_lib)))["a"]
    two = lambda v: " | ".join("%.1f" % x for x in v)
    lines = ["per-voxel normals of n sequences replayed through BatchLidarOdometry (synth scans of 13 200 points, leaf %.1f m), three ways," % LEAF,
             "alternated (a) (b) (c) (a) (b) (c) on fresh contexts; scans/s over the whole replay loop, both repetitions (the first",
             "repetition of a process carries its warm-up).  THE VALUES ARE ONE RUN ON ONE BOX; no speed-up is claimed or gated.",
             "(a) world_map=(leaf, capacity): a plain map, 28 bytes per table position -- the yardstick; no normals",
             "(b) world_map=(leaf, capacity, \"surfels\"): 76 bytes per table position, k_wm_insert<true>; world_map_surfels of every",
             "    sequence read once at the end (inside the clock)",
             "(c) no device map: cloud_download_registered per round, per-voxel float64 moments in numpy, numpy.linalg.eigh at the end",
             "(a) parent: (a) on the parent commit's library, a process of its own, two repetitions",
             "B/round back: bytes read back per round for the map ((a), (b): 32 per add call); (b) final: the surfel download at the end",
             "angle: the largest angle between (b)'s and (c)'s normal of sequence 0 over the compared voxels (n >= 10, planarity > 0.5);",
             "(c) sums in float64 about the origin, (b) as defined in include/mmloam_hip.h: close, not equal",
             "",
             "%4s %6s %8s %18s %18s %18s %18s %10s %10s %12s %9s %7s" % ("n", "rounds", "voxels", "(a) scans/s", "(b) scans/s", "(c) scans/s", "(a) parent",
                                                                      "(b) B/rnd", "(c) B/rnd", "(b) final B", "compared", "angle")]
    for r in rows:
        lines.append("%4d %6d %8d %18s %18s %18s %18s %10.0f %10.0f %12d %9s %7s" % (
            r["n"], r["rounds"], r["b_voxels"], two(r["a"]), two(r["b"]), two(r["c"]), two(parent[r["n"]]) if r["n"] in parent else "-",
            r["b_bytes"], r["c_bytes"], r["b_final_bytes"], r.get("compared", "-") if r.get("same_voxels") else "differ",
            "%.3f" % r["max_angle_deg"] if r.get("same_voxels") else "-"))
    if a.isa and os.path.exists(a.isa):
        lines += ["", "ISA of the world map's kernels (world_map.hip) against the parent commit's, tools/isa_compare.py <old .s> <new .s> k_wm:",
                  "k_wm_insert in the first column is k_wm_insert<false>, the plain map's insert; k_wm_gather and k_wm_put (the rows of a rebuild,",
                  "reset of one map among several) carry the moments behind one launch-uniform branch; \"(banked form)\" is the tool's word for the",
                  "<true> instantiations, which it lists and does not compare (k_wm_insert<true> is the surfel map's insert)"] + open(a.isa).read().rstrip().splitlines()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
