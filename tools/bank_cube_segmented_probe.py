"""The replay of tools/bank_cube_probe.py -- n synthetic sequences through ONE BatchLidarOdometry(global_map=True) over n slots and
n map banks, the live 1-frame loop with the map thread's cube schedule -- with the banks' cube stores grown two ways:
  (a) on a build of the PARENT commit: global_increment="loop", mml_map_bank_global_append / _increment work the banks of a call
      through one after the other;
  (b) on this build: global_increment="segmented", mml_map_bank_global_append_segmented / _increment_segmented work them in one
      chain of launches (csrc/map_global.hip).
    python tools/bank_cube_segmented_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 8, 64 sequences of 7 scans (16 rings x 450 azimuths + 6 000 Livox points).  The inputs are those of
tools/bank_cube_probe.py (make_inputs, imported).

(a) runs on the parent build ($MML_LIB_PATH):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
Each replay set runs in a process of its own under a time limit of its own, the two builds ALTERNATED: (a), (b), (a), (b), ... --
REPS pairs, every process replaying each n once as a warm-up and once timed; a process starts only after the one before it
succeeded.  Per n the median of the REPS timed replays, the fastest / slowest beside it.  EVERY pose (P and Q of every scan of every
sequence), every key-scan list and every final cube-store size is compared bitwise between (a) and (b), in every pair.  Times are
host clock around the replay alone (the context exists before the clock starts; the replay ends in a synchronisation).
No speed-up is gated: the table records what one MI355X gave."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bank_cube_probe import ROUNDS, TRAJ, make_inputs  # noqa: E402

REPS = 3
SYNCS = [
    "host synchronisations of a round's cube upkeep after each call's entry drain, from the code:",
    "  (a) loop      on a parent from before the chains were merged -- append: 1 (all stack sizes) + 1 per bank; increment, per bank:",
    "                the match copy 2 + one per cell-refinement round per kind with points (+1 when its buffers grow); the store 1 per",
    "                kind with points + 1 per kind with a cube over 300 points: 4 to 6 and more per bank.  On this build the loop's",
    "                append is (b)'s, and its increment is (b)'s chain once per bank: 3 + R per bank, 4 + R on growth",
    "  (b) segmented append: 1 (all stack sizes), one launch for all banks",
    "                increment, whatever n: 1 kept / selected totals of all segments (the capacity decision) + 1 filtered sizes (none",
    "                when no cube is filtered) + at most 1 when a match copy grows + 1 bounding boxes of all match copies + R, the",
    "                cell-refinement rounds of the slowest match copy: 3 + R, 4 + R on growth",
    "                (csrc/map_global.hip chain_chunk / match_chunk, csrc/map_assoc.hip mml_build_grids); per chunk when the call's",
    "                banks hold more than MML_BANK_GLOBAL_INCREMENT_BUDGET points or number more than MML_BANK_GLOBAL_CHUNK_BANKS",
]


def worker(ns, mode, dump):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    scans, pred = make_inputs(synth, max(ns))
    how = dict(global_increment="segmented") if mode == "new" else {}     # (the parent's BatchLidarOdometry has no such argument)
    out, arrays = {}, {}

    def replay(n, ctx):
        poses = np.zeros((n, ROUNDS, 7))
        per_round = []
        inner = ctx.bank_global_increment

        def counted(banks, T, **kw):
            per_round.append(len(banks))
            return inner(banks, T, **kw)

        ctx.bank_global_increment = counted
        t0 = time.perf_counter()
        bat = odometry.BatchLidarOdometry(ctx, n, lidar_mode=2, global_map=True, **how)
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
        res = None
        for rep in range(2):                               # a warm-up, then the timed replay, each on a fresh context
            ctx = M.Context(max_scans=n, max_map_points=1 << 19)
            try:
                res = replay(n, ctx)
            finally:
                ctx.close()
        out[str(n)] = dict(s=res[3], scans=n * ROUNDS, keys=[int(k) for k in res[1]],
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_cube_segmented_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("ns", nargs="*", type=int)
    a = ap.parse_args()
    ns = a.ns or [1, 8, 64]
    if a.worker:
        return worker(ns, a.worker, a.dump)
    if not os.path.exists(a.prev):
        raise SystemExit("no parent build at %s (see the docstring)" % a.prev)
    tmp = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(tmp, exist_ok=True)
    dumps = [os.path.join(tmp, "bank_cube_segmented_probe_%s.npz" % m) for m in ("prev", "new")]
    times = {m: {n: [] for n in ns} for m in ("prev", "new")}
    diff = {n: 0 for n in ns}
    keys = {n: True for n in ns}
    sizes = {n: True for n in ns}
    last = None
    for rep in range(REPS):                                # alternated: (a), (b), (a), (b), ...
        prev = run("prev", ns, dumps[0], a.prev, a.limit)
        new = run("new", ns, dumps[1], None, a.limit)
        A, B = np.load(dumps[0]), np.load(dumps[1])
        for n in ns:
            p, q = prev[str(n)], new[str(n)]
            times["prev"][n].append(p["s"])
            times["new"][n].append(q["s"])
            diff[n] += int(np.sum(np.any(A["poses_%d" % n].view(np.uint64) != B["poses_%d" % n].view(np.uint64), axis=2)))
            keys[n] = keys[n] and p["keys"] == q["keys"]
            sizes[n] = sizes[n] and p["sizes"] == q["sizes"]
        last = new
    lines = ["bank cube maps, the cube upkeep of a round: n sequences x %d scans (16 x 450 + 6 000 points) through ONE BatchLidarOdometry(global_map=True)," % ROUNDS,
             "n slots, n banks, every bank its own cube store and match copy",
             "(a) parent build, global_increment=\"loop\": mml_map_bank_global_append / _increment, the banks of a call one after the other",
             "(b) this build, global_increment=\"segmented\": mml_map_bank_global_append_segmented / _increment_segmented, one chain of launches",
             "median of %d timed replays, each after a warm-up in its own process, (a) and (b) alternated (fastest .. slowest); compared in" % REPS,
             "every pair: P, Q of every scan of every sequence, every key-scan list, every final cube-store size, bitwise",
             "no speed-up is gated; this is what one MI355X gave; the default stays \"loop\"", "",
             "%5s %7s | %28s %10s | %28s %10s | %6s | %s" % ("n", "scans", "(a) s", "scans/s", "(b) s", "scans/s", "b / a",
                                                          "poses that differ / key scans / cube store sizes")]
    bad = 0
    for n in ns:
        ta, tb = sorted(times["prev"][n]), sorted(times["new"][n])
        ma, mb = ta[len(ta) // 2], tb[len(tb) // 2]
        sc = n * ROUNDS
        bad += diff[n] + (not keys[n]) + (not sizes[n])
        fmt = lambda t, m: "%.4f (%.4f .. %.4f)" % (m, t[0], t[-1])
        lines.append("%5d %7d | %28s %10.0f | %28s %10.0f | %6.2f | %d of %d / %s / %s" % (
            n, sc, fmt(ta, ma), sc / ma, fmt(tb, mb), sc / mb, ma / mb, diff[n], REPS * sc, "equal" if keys[n] else "DIFFERENT",
            "equal" if sizes[n] else "DIFFERENT"))
    slower = [n for n in ns if sorted(times["new"][n])[REPS // 2] > sorted(times["prev"][n])[REPS // 2]]
    lines += ["", "the segmented form is slower than the loop at n = %s" % ", ".join(map(str, slower)) if slower else
              "the segmented form is not slower than the loop at any n measured"]
    lines += ["", "banks per increment call of a replay in (b):"]
    for n in ns:
        inc = last[str(n)]["increments"] or []
        lines.append("  n = %3d: %s" % (n, inc))
    lines += [""] + SYNCS
    lines += ["", "the association kernels are not touched: csrc/map_assoc.hip is byte for byte the parent's"]
    for d in dumps:
        os.remove(d)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
