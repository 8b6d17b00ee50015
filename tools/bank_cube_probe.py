"""n synthetic sequences replayed through the live 1-frame loop WITH the map thread's cube schedule (odometry.py: append after
every non-degenerate scan, MapIncrement on every second one, Estimate against the cube first), two ways:
  (a) on a build of the PARENT commit: n sequential LidarOdometry(global_map=True) loops, each on a context of its own with one
      slot, through the C-ABI the parent has (mml_map_global_append / _increment);
  (b) on this build: ONE BatchLidarOdometry(global_map=True) over n slots and n map banks, the sequences in lockstep
      (mml_map_bank_global_append / _increment, the banked association kernels with the cube stage).
    python tools/bank_cube_probe.py [--prev <parent .so>] [--isa-report <file>] [--isa-parent <file>] [--out <table>] [n ...]
Defaults: n = 1, 8, 64 sequences of 7 scans (16 rings x 450 azimuths + 6 000 Livox points, the shape of the GPU tests).  Four
trajectories of synth scans are generated once per process and shared round robin; every sequence has its own predicted poses.

(a) runs on the parent build ($MML_LIB_PATH, as tools/map_banks_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
in a process of its own; (b) runs in a second process, started only after the first succeeded, each under a time limit of its
own.  EVERY pose is compared: P and Q of every scan of every sequence must be bit-equal across the two, the key-scan counts and
the cube store sizes equal.  Times are host clock around the replay alone (contexts are created before the clock starts; every
call in the replay ends in a synchronisation).  Per size: a warm-up replay, then 3 timed ones; the median, and the fastest /
slowest beside it.  No speed-up is claimed: (b) works n banks' increments through one after the other, and each increment
synchronises the host several times (counted below from the calls the replay issued).
--isa-report: the output of tools/isa_compare.py on the two builds' map_assoc assembly; --isa-parent: the "(banked form)" lines
of the same tool run on the parent's assembly alone.  Both are carried into the table as they are."""
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
TRAJ, ROUNDS, REPS = 4, 7, 3


def make_inputs(synth, n):
    from scipy.spatial.transform import Rotation as Rsc
    scans = {}
    for t in range(TRAJ):
        for i in range(ROUNDS):
            k = 20 + 37 * t + (4 + t) * i
            scans[(t, i)] = (synth.velo_scan(k, n_az=450, motion=True), synth.livox_scan(k, n=6000, motion=True), synth.sweep_motion(k),
                             synth.pose_matrix(k))
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
    out, arrays = {}, {}

    def replay_sequential(n, ctxs):
        poses, keys, sizes, t = np.zeros((n, ROUNDS, 7)), [], [], 0.0
        for w in range(n):
            ctx = ctxs[w]
            t0 = time.perf_counter()
            odo = odometry.LidarOdometry(ctx, lidar_mode=2, global_map=True)
            for i in range(ROUNDS):
                v, l, (dR, dt), _ = scans[(w % TRAJ, i)]
                ctx.scan_upload(0, v, l)
                ctx.extract(0, 1)
                ctx.undistort(0, 1, dR.reshape(1, 9), dt.reshape(1, 3))
                P, Q, _ = odo.estimate_lidar_pose(0, *pred[(w, i)])
                poses[w, i] = np.concatenate([P, Q])
            ctx.synchronize()
            t += time.perf_counter() - t0
            keys.append(odo.key_scans)
            sizes.append([odo.n_corner_global, odo.n_surf_global])
        return poses, keys, sizes, t, None

    def replay_batch(n, ctxs):
        ctx = ctxs[0]
        poses = np.zeros((n, ROUNDS, 7))
        ctx.map_banks(0)
        per_round = []
        inner = ctx.bank_global_increment

        def counted(banks, T):
            per_round.append(len(banks))
            return inner(banks, T)

        ctx.bank_global_increment = counted
        t0 = time.perf_counter()
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2, global_map=True)
        for i in range(ROUNDS):
            for w in range(n):
                ctx.scan_upload(w, scans[(w % TRAJ, i)][0], scans[(w % TRAJ, i)][1])
            ctx.extract(0, n)
            ctx.undistort(0, n, np.stack([scans[(w % TRAJ, i)][2][0].reshape(9) for w in range(n)]),
                          np.stack([scans[(w % TRAJ, i)][2][1] for w in range(n)]))
            P, Q, _ = bat.estimate_lidar_pose(list(range(n)), np.stack([pred[(w, i)][0] for w in range(n)]),
                                              np.stack([pred[(w, i)][1] for w in range(n)]))
            poses[:, i] = np.concatenate([P, Q], axis=1)
        ctx.synchronize()
        t = time.perf_counter() - t0
        del ctx.bank_global_increment
        return poses, bat.key_scans, [[st.n_corner_global, st.n_surf_global] for st in bat.seq], t, per_round

    for n in ns:
        t, res = [], None
        for rep in range(1 + REPS):
            if mode == "prev":
                ctxs = [M.Context(max_scans=1, max_map_points=1 << 19) for _ in range(n)]
            else:
                ctxs = [M.Context(max_scans=n, max_map_points=1 << 19)]
            try:
                res = (replay_sequential if mode == "prev" else replay_batch)(n, ctxs)
            finally:
                for c in ctxs:
                    c.close()
            if rep:
                t.append(res[3])
        t = sorted(t)
        out[str(n)] = dict(s=t[len(t) // 2], lo=t[0], hi=t[-1], scans=n * ROUNDS, keys=[int(k) for k in res[1]],
                           sizes=[[int(a), int(b)] for a, b in res[2]], increments=res[4])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_cube_probe.txt"))
    ap.add_argument("--isa-report", default=None)
    ap.add_argument("--isa-parent", default=None)
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
    dumps = [os.path.join(tmp, "bank_cube_probe_%s.npz" % m) for m in ("prev", "new")]
    prev = run("prev", ns, dumps[0], a.prev, a.limit)
    new = run("new", ns, dumps[1], None, a.limit)
    A, B = np.load(dumps[0]), np.load(dumps[1])
    lines = ["bank cube maps: n sequences x %d scans (16 x 450 + 6 000 points), the live 1-frame loop with local-map upkeep AND the cube schedule" % ROUNDS,
             "(a) parent build: n sequential LidarOdometry(global_map=True) loops, a context of one slot each, own cube store",
             "(b) this build: one BatchLidarOdometry(global_map=True), n slots, n banks, every bank its own cube store and match copy",
             "median of %d replays after a warm-up (fastest .. slowest); poses compared: P, Q of every scan of every sequence, bitwise" % REPS,
             "no speed-up is claimed or gated: (b) works the banks' increments through one after the other", "",
             "%5s %7s | %28s %10s | %28s %10s | %6s | %s" % ("n", "scans", "(a) s", "scans/s", "(b) s", "scans/s", "b / a",
                                                          "poses that differ / key scans / cube store sizes")]
    bad = 0
    for n in ns:
        p, q = prev[str(n)], new[str(n)]
        pa, pb = A["poses_%d" % n], B["poses_%d" % n]
        diff = int(np.sum(np.any(pa.view(np.uint64) != pb.view(np.uint64), axis=2)))
        keys = "equal" if p["keys"] == q["keys"] else "DIFFERENT"
        sizes = "equal" if p["sizes"] == q["sizes"] else "DIFFERENT"
        bad += diff + (keys != "equal") + (sizes != "equal")
        fmt = lambda r: "%.4f (%.4f .. %.4f)" % (r["s"], r["lo"], r["hi"])
        lines.append("%5d %7d | %28s %10.0f | %28s %10.0f | %6.2f | %d of %d / %s / %s" % (
            n, p["scans"], fmt(p), p["scans"] / p["s"], fmt(q), q["scans"] / q["s"], (q["scans"] / q["s"]) / (p["scans"] / p["s"]), diff,
            pa.shape[0] * pa.shape[1], keys, sizes))
    lines += ["", "cube stores that pass the gate at the end (corner > 0 and surf > 100, Estimator.cpp:1032): " +
              ", ".join("n = %s: %d of %d" % (n, sum(1 for c, s in new[str(n)]["sizes"] if c > 0 and s > 100), int(n)) for n in map(str, ns)),
              "", "host synchronisations of a round of increments in (b).  From the code, per bank and increment (map_global.hip, the n-store",
              "chain with n = 1): 1 kept / selected totals of both kinds (the capacity decision) + 1 filtered sizes (none when no cube is",
              "over 300) + at most 1 when the match copy grows + 1 bounding boxes of both kinds + R, the cell-refinement rounds of the slower",
              "kind (map_assoc.hip mml_build_grids): 3 + R, 4 + R on growth.  Banks per mml_map_bank_global_increment call:"]
    for n in ns:
        inc = new[str(n)]["increments"] or []
        lines.append("  n = %3d: %s banks in the %d calls of a replay -> about %d .. %d synchronisations in the largest round" % (
            n, inc, len(inc), 4 * max(inc + [0]), 8 * max(inc + [0])))
    lines += ["", "ISA of the association kernels, parent build against this build (tools/isa_compare.py on the -save-temps assembly of",
              "csrc/map_assoc.hip, the Makefile's flags; the unbanked instantiations are what a launch without a bound slot runs):"]
    lines += open(a.isa_report).read().rstrip().splitlines() if a.isa_report else ["(not supplied: --isa-report)"]
    lines += ["", "the banked forms at the PARENT (no cube stage reachable: have_g was 0 in every banked launch):"]
    lines += open(a.isa_parent).read().rstrip().splitlines() if a.isa_parent else ["(not supplied: --isa-parent)"]
    lines += ["", "Occupancy (MML_AW_SEARCH / _FIT / _HARD = 8 / 4 / 1 wavefronts per SIMD, csrc/map_assoc.hip): every banked form has the VGPR count",
              "of its parent banked form (64 / 128 / 128 / 117-121) and no more than its unbanked twin (64 / 128 / 132 / 123-127): no banked form",
              "drops an occupancy step.  Scratch: k_associate<true> 32 bytes and k_associate_fit_all<true> 20 bytes, as at the parent (their",
              "unbanked twins: 36 and 20 bytes, the price of holding them to 64 / 128 registers); the far-query forms and k_associate_fit<true> 0."]
    for d in dumps:
        os.remove(d)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
