"""n synthetic sequences replayed through the live 1-frame loop (upload, extract, undistort, EstimateLidarPose with map upkeep),
two ways:
  (a) on a build of the PARENT commit: n sequential LidarOdometry loops in one context of one slot, one sequence after the
      other -- all a context with a single local map offers;
  (b) on this build: ONE BatchLidarOdometry over n slots and n map banks, the sequences in lockstep.
    python tools/map_banks_probe.py [--prev <parent .so>] [--isa-report <file>] [--out <table>] [n ...]
Defaults: n = 1, 8, 64 sequences of 6 scans of the BASELINE configs[1] shape (16 rings x 1800 azimuths + 24 000 Livox points).
Four trajectories of synth scans are generated once per process and shared round robin; every sequence has its own predicted
poses, so no two sequences see the same problem.

(a) runs on the parent build ($MML_LIB_PATH, as tools/pose_ingest_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
in a process of its own; (b) runs on this build in a second process, started only after the first succeeded, each under a time
limit of its own.  EVERY pose is compared: P and Q of every scan of every sequence must be bit-equal across the two, and the
key-scan counts equal.  Times are host clock around the whole replay (every call in it ends in a synchronisation).  Per size: a
warm-up replay, then 3 timed ones; the median, and the fastest / slowest beside it.
--isa-report: the output of tools/isa_compare.py on the two builds' map_assoc assembly, carried into the table as it is."""
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
TRAJ, ROUNDS, REPS = 4, 6, 3


def make_inputs(synth, n):
    from scipy.spatial.transform import Rotation as Rsc
    scans = {}
    for t in range(TRAJ):
        for i in range(ROUNDS):
            k = 20 + 37 * t + (4 + t) * i
            scans[(t, i)] = (synth.velo_scan(k, motion=True), synth.livox_scan(k, motion=True), synth.sweep_motion(k), synth.pose_matrix(k))
    pred = {}
    for w in range(n):
        rng = np.random.default_rng(1000 + w)
        for i in range(ROUNDS):
            T = scans[(w % TRAJ, i)][3].copy()
            T[:3, :3] = T[:3, :3] @ Rsc.from_rotvec(rng.uniform(-0.004, 0.004, 3)).as_matrix()
            T[:3, 3] += rng.uniform(-0.03, 0.03, 3)
            pred[(w, i)] = (T[:3, 3].copy(), Rsc.from_matrix(T[:3, :3]).as_quat())
    return scans, pred


def worker(ns, mode, dump):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    nmax = max(ns)
    scans, pred = make_inputs(synth, nmax)
    out = {}
    ctx = M.Context(max_scans=1 if mode == "prev" else nmax, max_map_points=1 << 19)

    def replay_sequential(n):
        poses, keys = np.zeros((n, ROUNDS, 7)), []
        for w in range(n):
            odo = odometry.LidarOdometry(ctx, lidar_mode=2)
            for i in range(ROUNDS):
                v, l, (dR, dt), _ = scans[(w % TRAJ, i)]
                ctx.scan_upload(0, v, l)
                ctx.extract(0, 1)
                ctx.undistort(0, 1, dR.reshape(1, 9), dt.reshape(1, 3))
                P, Q, _ = odo.estimate_lidar_pose(0, *pred[(w, i)])
                poses[w, i] = np.concatenate([P, Q])
            keys.append(odo.key_scans)
        return poses, keys

    def replay_batch(n):
        poses = np.zeros((n, ROUNDS, 7))
        ctx.map_banks(0)
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2)
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

    replay = replay_sequential if mode == "prev" else replay_batch
    arrays = {}
    for n in ns:
        t, res = [], None
        for rep in range(1 + REPS):
            t0 = time.perf_counter()
            res = replay(n)
            ctx.synchronize()
            if rep:
                t.append(time.perf_counter() - t0)
        t = sorted(t)
        out[str(n)] = dict(s=t[len(t) // 2], lo=t[0], hi=t[-1], scans=n * ROUNDS, keys=[int(k) for k in res[1]])
        arrays["poses_%d" % n] = res[0]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_banks_probe.txt"))
    ap.add_argument("--isa-report", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("ns", nargs="*", type=int)
    a = ap.parse_args()
    ns = a.ns or [1, 8, 64]
    if a.worker:
        return worker(ns, a.worker, a.dump)
    if not os.path.exists(a.prev):
        raise SystemExit("no parent build at %s (see the docstring)" % a.prev)
    tmp = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(tmp, exist_ok=True)
    dumps = [os.path.join(tmp, "map_banks_probe_%s.npz" % m) for m in ("prev", "new")]
    prev = run("prev", ns, dumps[0], a.prev, a.limit)
    new = run("new", ns, dumps[1], None, a.limit)
    A, B = np.load(dumps[0]), np.load(dumps[1])
    lines = ["map banks: n sequences x %d scans (16 x 1800 + 24 000 points), the live 1-frame loop with map upkeep" % ROUNDS,
             "(a) parent build: n sequential LidarOdometry loops, one slot, one map   (b) this build: one BatchLidarOdometry, n slots, n banks",
             "median of %d replays after a warm-up (fastest .. slowest); poses compared: P, Q of every scan of every sequence, bitwise" % REPS, "",
             "%5s %7s | %28s %10s | %28s %10s | %6s | %s" % ("n", "scans", "(a) s", "scans/s", "(b) s", "scans/s", "b / a", "poses that differ / key scans")]
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
    lines += ["", "ISA of the association kernels, parent build against this build (tools/isa_compare.py on the -save-temps assembly of",
              "csrc/map_assoc.hip, the Makefile's flags; the unbanked instantiations are what a launch without a bound slot runs):"]
    lines += open(a.isa_report).read().rstrip().splitlines() if a.isa_report else ["(not supplied: --isa-report)"]
    for d in dumps:
        os.remove(d)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
