"""The replay of tools/map_banks_probe.py -- n synthetic sequences in lockstep through ONE BatchLidarOdometry over n slots and n map
banks (upload, extract, undistort, EstimateLidarPose with map upkeep) -- with the banks' local maps grown two ways:
  (a) on a build of the PARENT commit: increment="loop", mml_map_bank_increment works the growing banks through one by one;
  (b) on this build: increment="segmented", mml_map_bank_increment_segmented works them in one chain of launches.
    python tools/bank_increment_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 8, 64 sequences of 6 scans (16 rings x 1800 azimuths + 24 000 Livox points), the inputs of map_banks_probe.py.

(a) runs on the parent build ($MML_LIB_PATH):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
in a process of its own; (b) runs on this build in a second process, started only after the first succeeded, each under a time
limit of its own.  EVERY pose is compared: P and Q of every scan of every sequence must be bit-equal across the two, and the
key-scan lists equal.  Times are host clock around the whole replay.  Per size: a warm-up replay, then 3 timed ones; the median,
and the fastest / slowest beside it.  No ratio is gated: the table says what was measured."""
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
from map_banks_probe import REPS, ROUNDS, TRAJ, make_inputs  # noqa: E402

SYNCS = [
    "host synchronisations of the increment per round, from the code (after the entry drain; g = the banks that grow this round):",
    "  loop       per bank, the chain below with that one bank: 1 (the two stack sizes) + 1 (the two filtered sizes and boxes) + 1 per",
    "             cell-refinement round of the bank's slower kind (1 to 5)  =  (2 + R) g.  (On a build from before the chains were merged:",
    "             a chain of its own, per kind a size, a box and the rounds, at least 7 g.)",
    "  segmented  1 (all stack sizes) + per chunk of banks: 1 (all filtered sizes and boxes) + 1 per cell-refinement round of the",
    "             chunk's slowest (bank, kind)  =  2 + R whatever g is, while the banks' rings fit one chunk (2^22 points)",
    "             (csrc/map_upkeep.hip mml_map_upkeep_increment_segmented, csrc/map_assoc.hip mml_build_grids)",
]


def grid_times(M, synth, sizes, reps=5):
    """Host clock, ending in a synchronise, of map_set_local(1, cloud) at each size and of one map_global_increment: every repetition's
    milliseconds.  The clouds: uniform points in a 40 x 40 x 6 m box (seeded); the increment: one 4 000 + 8 000 point key scan appended."""
    rng = np.random.default_rng(11)
    out = {}
    ctx = M.Context(max_scans=1, max_map_points=max(1 << 19, max(sizes)))
    for m in sizes:
        cloud = (rng.random((m, 3)) * np.array([40.0, 40.0, 6.0])).astype(np.float32)
        t = []
        for rep in range(1 + reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.map_set_local(1, cloud)
            ctx.synchronize()
            if rep:
                t.append(1e3 * (time.perf_counter() - t0))
        out["map_set_local_%d_ms" % m] = t
    t = []
    for rep in range(1 + reps):
        ctx.map_global_reset()
        for kind, m in ((0, 4000), (1, 8000)):
            ctx.features_upload(0, kind, (rng.random((m, 3)) * np.array([40.0, 40.0, 6.0])).astype(np.float32))
        ctx.map_global_append(0, np.eye(4))
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.map_global_increment(np.eye(4))
        ctx.synchronize()
        if rep:
            t.append(1e3 * (time.perf_counter() - t0))
    out["map_global_increment_ms"] = t
    ctx.close()
    return out


def worker(ns, mode, dump, how=None, grid_sizes=()):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    nmax = max(ns)
    scans, pred = make_inputs(synth, nmax)
    ctx = M.Context(max_scans=nmax, max_map_points=1 << 19)
    how = how or ("loop" if mode == "prev" else "segmented")

    def replay(n):
        poses = np.zeros((n, ROUNDS, 7))
        ctx.map_banks(0)
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2, increment=how)
        for i in range(ROUNDS):
            for w in range(n):
                ctx.scan_upload(w, scans[(w % TRAJ, i)][0], scans[(w % TRAJ, i)][1])
            ctx.extract(0, n)
            ctx.undistort(0, n, np.stack([scans[(w % TRAJ, i)][2][0].reshape(9) for w in range(n)]),
                          np.stack([scans[(w % TRAJ, i)][2][1] for w in range(n)]))
            P, Q, _ = bat.estimate_lidar_pose(list(range(n)), np.stack([pred[(w, i)][0] for w in range(n)]),
                                              np.stack([pred[(w, i)][1] for w in range(n)]))
            poses[:, i] = np.concatenate([P, Q], axis=1)
        return poses, bat.key_scans

    out, arrays = {}, {}
    for n in ns:
        t, res = [], None
        for rep in range(1 + REPS):
            t0 = time.perf_counter()
            res = replay(n)
            ctx.synchronize()
            if rep:
                t.append(time.perf_counter() - t0)
        t = sorted(t)
        out[str(n)] = dict(s=t[len(t) // 2], lo=t[0], hi=t[-1], t=t, scans=n * ROUNDS, keys=[int(k) for k in res[1]])
        arrays["poses_%d" % n] = res[0]
    ctx.close()
    if grid_sizes:  # (--grid: the one-map grid build and the cube store's increment, for an A/B of two builds)
        out["grid"] = grid_times(M, synth, grid_sizes)
    np.savez(dump, **arrays)
    print("RESULT " + json.dumps(out), flush=True)


def run(mode, ns, dump, lib, limit):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--dump", dump] + [str(n) for n in ns], env=env, timeout=limit,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("the %s replay failed (exit %d):\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_increment_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--how", default=None, choices=["loop", "segmented"], help="--worker: the increment to run whatever the mode")
    ap.add_argument("--grid", default="", help="--worker: also time map_set_local at these sizes (comma-separated) and one map_global_increment")
    ap.add_argument("ns", nargs="*", type=int)
    a = ap.parse_args()
    ns = a.ns or [1, 8, 64]
    if a.worker:
        return worker(ns, a.worker, a.dump, a.how, [int(m) for m in a.grid.split(",") if m])
    if not os.path.exists(a.prev):
        raise SystemExit("no parent build at %s (see the docstring)" % a.prev)
    tmp = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(tmp, exist_ok=True)
    dumps = [os.path.join(tmp, "bank_increment_probe_%s.npz" % m) for m in ("prev", "new")]
    prev = run("prev", ns, dumps[0], a.prev, a.limit)
    new = run("new", ns, dumps[1], None, a.limit)
    A, B = np.load(dumps[0]), np.load(dumps[1])
    lines = ["bank increment: n sequences x %d scans (16 x 1800 + 24 000 points) in lockstep, one BatchLidarOdometry, n slots, n banks" % ROUNDS,
             '(a) parent build, increment="loop"   (b) this build, increment="segmented"',
             "median of %d replays after a warm-up (fastest .. slowest); compared: P, Q of every scan of every sequence bitwise, the key-scan lists" % REPS,
             "", "%5s %7s | %28s %10s | %28s %10s | %6s | %s" % ("n", "scans", "(a) s", "scans/s", "(b) s", "scans/s", "b / a", "poses that differ / key scans")]
    bad = 0
    for n in ns:
        p, q = prev[str(n)], new[str(n)]
        pa, pb = A["poses_%d" % n], B["poses_%d" % n]
        diff = int(np.sum(np.any(pa.view(np.uint64) != pb.view(np.uint64), axis=2)))
        keys = "equal" if p["keys"] == q["keys"] else "DIFFERENT"
        bad += diff + (keys != "equal")
        fmt = lambda r: "%.4f (%.4f .. %.4f)" % (r["s"], r["lo"], r["hi"])
        lines.append("%5d %7d | %28s %10.0f | %28s %10.0f | %6.2f | %d of %d / %s" % (n, p["scans"], fmt(p), p["scans"] / p["s"], fmt(q), q["scans"] / q["s"],
                                                                                     (q["scans"] / q["s"]) / (p["scans"] / p["s"]), diff, pa.shape[0] * pa.shape[1], keys))
    lines += [""] + SYNCS
    for d in dumps:
        os.remove(d)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
