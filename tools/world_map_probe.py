"""The world map of n sequences replayed through BatchLidarOdometry, two ways, alternated in one run:
  (a) the way a caller has on the parent commit: per round Context.cloud_download_registered for the published scans, then the
      numpy restatement of the map's arithmetic on the host (tests/world_map_ref.py);
  (b) BatchLidarOdometry(world_map=(leaf, capacity)): one mml_world_map_add per run of adjacent slots, the map stays on the device.
    python tools/world_map_probe.py [--out <table>] [--rounds R] [--isa <file with the ISA comparison's lines>] [n ...]
Defaults: n = 1, 8, 64 sequences, 4 rounds.  Every size runs in a process of its own under its own time limit; inside it the
order is (a) (b) (a) (b) on fresh contexts.  Every sequence's final map of (b) is compared bitwise with (a)'s.  Written per
size: scans/s of both (host clock around the whole replay loop: upload, extract, undistort, estimate, map), the bytes read back
for the map per round of both, and what one add call costs in launches and synchronisations (by construction: see
csrc/world_map.hip's header comment).  No speed-up is claimed; the values are one run on one box.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
LEAF = 0.2
ADD_READBACK_BYTES = 32      # seven counters and the table's total, 4 bytes each (world_map.hip)


def inputs(synth, n, rounds):
    from scipy.spatial.transform import Rotation as Rsc
    out = []
    for w in range(n):
        seq = []
        for i in range(rounds):
            k = 20 + 3 * (w % 16) + 4 * i
            v, l = synth.velo_scan(k, n_az=450, motion=True), synth.livox_scan(k, n=6000, motion=True)
            dR, dt = synth.sweep_motion(k)
            T = synth.pose_matrix(k).copy()
            T[:3, 3] += [0.02, -0.015, 0.01]
            seq.append((v, l, dR, dt, T[:3, 3].copy(), Rsc.from_matrix(T[:3, :3]).as_quat()))
        out.append(seq)
    return out


def replay(M, odometry, R, inp, n, rounds, device_map, capacity):
    ctx = M.Context(max_scans=n, max_map_points=1 << 17)
    try:
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2, increment="segmented", world_map=(LEAF, capacity) if device_map else None)
        ref, back = R.WorldMapRef(LEAF), 0
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(rounds):
            for w in range(n):
                ctx.scan_upload(w, inp[w][i][0], inp[w][i][1])
            ctx.extract(0, n)
            ctx.undistort(0, n, np.stack([inp[w][i][2].reshape(9) for w in range(n)]), np.stack([inp[w][i][3] for w in range(n)]))
            bat.estimate_lidar_pose(list(range(n)), np.stack([inp[w][i][4] for w in range(n)]), np.stack([inp[w][i][5] for w in range(n)]))
            pub = [w for w in range(n) if not bat.seq[w].fail_detected]
            if device_map:
                back += ADD_READBACK_BYTES * len(odometry._adjacent_runs(pub, lambda w: w))
            else:
                for run in odometry._adjacent_runs(pub, lambda w: w):
                    clouds = ctx.cloud_download_registered(run[0], len(run), np.stack([bat.seq[w].last_T for w in run]))
                    for w, c in zip(run, clouds):
                        ref.add_records(w, c)
                        back += 48 * len(c) + 4
        ctx.synchronize()
        dt = time.perf_counter() - t0
        maps = [bat.world_map(w) if device_map else ref.download(w)[0] for w in range(n)]
        return dict(scans_per_s=n * rounds / dt, bytes_per_round=back / rounds, maps=maps)
    finally:
        ctx.close()


def worker(n, rounds):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    import world_map_ref as R
    inp = inputs(synth, n, rounds)
    capacity = max(1 << 16, n * rounds * 13200)      # (every point its own voxel at the worst)
    runs = [replay(M, odometry, R, inp, n, rounds, dev, capacity) for dev in (False, True, False, True)]
    differing = sum(0 if (a.shape == b.shape and a.tobytes() == b.tobytes()) else 1 for a, b in zip(runs[0]["maps"], runs[1]["maps"]))
    differing += sum(0 if a.tobytes() == b.tobytes() else 1 for a, b in zip(runs[1]["maps"], runs[3]["maps"]))
    r = dict(n=n, rounds=rounds, voxels=int(sum(len(m) for m in runs[1]["maps"])), differing_maps=differing,
             host=[runs[0]["scans_per_s"], runs[2]["scans_per_s"]], device=[runs[1]["scans_per_s"], runs[3]["scans_per_s"]],
             host_bytes=runs[0]["bytes_per_round"], device_bytes=runs[1]["bytes_per_round"])
    print("PROBE " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_probe.txt"))
    ap.add_argument("--worker", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds the process of one size may take")
    ap.add_argument("--isa", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker is not None:
        return worker(a.worker, a.rounds)
    rows = []
    for n in a.sizes or [1, 8, 64]:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n), "--rounds", str(a.rounds)], capture_output=True, text=True,
                             timeout=a.limit)
        if out.returncode != 0:   # (nothing more is started on the device after a failure)
            sys.exit("the process of n = %d failed (%d): %s" % (n, out.returncode, out.stderr[-2000:]))
        rows += [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]
    lines = ["the world map of n sequences replayed through BatchLidarOdometry (synth scans of 13 200 points, leaf %.1f m), two ways," % LEAF,
             "alternated (a) (b) (a) (b) on fresh contexts; scans/s over the whole replay loop, both repetitions; one run on one box",
             "(a) parent commit's way: cloud_download_registered per round + the numpy restatement on the host",
             "(b) world_map=: one mml_world_map_add per run of adjacent slots",
             "equal = every sequence's final map of (b) holds the bytes of (a)'s, and the two (b) runs hold the same bytes",
             "one add call: 4 kernel launches of its own (keys, run heads, lookup, insert) + 2 memsets + one rocPRIM radix sort + one",
             "rocPRIM scan; 1 host synchronisation (32 bytes read back), whatever the number of slots",
             "",
             "%4s %7s %9s %24s %24s %16s %16s %6s" % ("n", "rounds", "voxels", "(a) scans/s", "(b) scans/s", "(a) B/round back", "(b) B/round back", "equal")]
    ok = True
    for r in rows:
        ok &= r["differing_maps"] == 0
        lines.append("%4d %7d %9d %24s %24s %16.0f %16.0f %6s" % (r["n"], r["rounds"], r["voxels"], "%.1f | %.1f" % tuple(r["host"]),
                                                               "%.1f | %.1f" % tuple(r["device"]), r["host_bytes"], r["device_bytes"],
                                                               r["differing_maps"] == 0))
    if a.isa and os.path.exists(a.isa):
        lines += ["", "ISA of the registered-cloud kernels (capi.hip) and the association kernels (map_assoc.hip) against the parent commit's,",
                  "tools/isa_compare.py:"] + open(a.isa).read().rstrip().splitlines()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a device map differs from the host restatement's")


if __name__ == "__main__":
    main()
