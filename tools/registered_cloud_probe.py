"""The registered (world-frame) clouds of n resident slots, three ways:
  (a) the way a caller does it on the PARENT commit: n x mml_scan_download_pointxyzinormal, then per slot the reference's
      double transform and the repack into the published record in numpy (row by row in the reference's order of operations,
      so that the result is the reference's bit for bit);
  (b) n x mml_cloud_download_registered;
  (c) one mml_cloud_download_registered_batch.
    python tools/registered_cloud_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 16, 64, 512 slots.

(a) runs on a build of the parent commit ($MML_LIB_PATH, as tools/gicp_refresh_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
in a process of its own; (b) and (c) run on this build in a second process, started only after the first succeeded, each
under a time limit of its own.  All three write into one preallocated host buffer of the total size and none makes a
sizing call (the counts are known from the setup), so the difference is the host loop and the per-slot synchronisations.
Every record of (b) and (c) is compared with (a) recomputed in the second process, and a SHA-256 of the whole output ties
that to the parent build's (a).

Inputs: the bench scan shape (16 rings x 1800 azimuths + 24 000 Livox points with sweep motion), synth scans 14 .. 29 reused
round robin, extracted and undistorted; every slot has its own pose.  Times are host clock around the calls, which end in a
stream synchronise.  Per size: a warm-up, then at least 20 repetitions; median and the 10th / 90th percentile."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = 16          # distinct synth scans


def timed(fn, min_reps=20, warm=1):
    t = []
    for rep in range(warm + min_reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def slot_pose(synth, s):
    """A pose of its own for every slot: the trajectory pose of scan s, a few hundred metres out."""
    T = synth.pose_matrix(s).copy()
    T[:3, 3] += [250.0 + 0.37 * s, -120.0 - 0.11 * s, 3.0]
    return T


def host_registered(rec, T, out):
    """pointAssociateToMap over one downloaded cloud (rec: n x 12 float32) into out (n x 12 float32, zeroed)."""
    x, y, z = (rec[:, c].astype(np.float64) for c in range(3))
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    out[:, 3] = 1.0
    out[:, 6] = rec[:, 6]
    out[:, 8] = rec[:, 8]


def worker(ns, mode):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    L = M.lib()
    nmax = max(ns)
    ctx = M.Context(max_scans=nmax)
    base = [(synth.velo_scan(14 + k, motion=True), synth.livox_scan(14 + k, motion=True), synth.sweep_motion(14 + k))
            for k in range(min(BASE, nmax))]
    for s in range(nmax):
        ctx.scan_upload(s, base[s % BASE][0], base[s % BASE][1])
    ctx.extract(0, nmax)
    ctx.undistort(0, nmax, np.stack([base[s % BASE][2][0].reshape(9) for s in range(nmax)]),
                  np.stack([base[s % BASE][2][1] for s in range(nmax)]))
    counts = np.array([ctx.scan_info(s).n_points for s in range(nmax)], np.int64)
    T = np.ascontiguousarray(np.stack([slot_pose(synth, s) for s in range(nmax)]).reshape(nmax, 16))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    at = lambda a, i: C.c_void_p(a.ctypes.data + a.strides[0] * i)

    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.mml_last_error(ctx._h).decode())

    scratch = np.zeros((int(counts.max()), 12), np.float32)
    nn = np.zeros(nmax, np.int32)

    def host(k, out):
        off = 0
        out[:] = 0
        for s in range(k):
            ck(L.mml_scan_download_pointxyzinormal(ctx._h, s, p(scratch), len(scratch), at(nn, s)))
            host_registered(scratch[:nn[s]], T[s].reshape(4, 4), out[off:off + nn[s]])
            off += int(nn[s])

    def single(k, out):
        off = 0
        for s in range(k):
            ck(L.mml_cloud_download_registered(ctx._h, s, at(T, s), at(out, off), len(out) - off, at(nn, s)))
            off += int(nn[s])

    def batch(k, out):
        ck(L.mml_cloud_download_registered_batch(ctx._h, 0, k, p(T), p(out), len(out), p(nn)))

    for k in ns:
        total = int(counts[:k].sum())
        out = np.zeros((total, 12), np.float32)
        r = dict(n=k, mode=mode, points=total, lib=os.environ.get("MML_LIB_PATH", "default"))
        if mode == "prev":
            r["host"] = timed(lambda: host(k, out))
            r["sha"] = hashlib.sha256(out.tobytes()).hexdigest()
        else:
            ref = np.zeros_like(out)
            host(k, ref)
            r["sha"] = hashlib.sha256(ref.tobytes()).hexdigest()
            for name, fn in (("single", single), ("batch", batch)):
                out[:] = 0
                r[name] = timed(lambda: fn(k, out))
                r[name + "_differing_records"] = int((out.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum())
        print("PROBE " + json.dumps(r), flush=True)
    ctx.close()


def run_worker(lib, ns, mode, limit):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode] + [str(n) for n in ns], env=env,
                         capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registered_cloud_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker)
    ns = a.sizes or [1, 16, 64, 512]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    prev = run_worker(a.prev, ns, "prev", a.limit)
    new = run_worker(None, ns, "new", a.limit)   # started only after the first succeeded
    f = lambda t: "%.2f [%.2f .. %.2f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["the registered clouds of n resident slots (bench scan shape, undistorted, one pose per slot), into one host buffer;",
             "ms, median [p10 .. p90] of >= 20 repetitions, host clock around the calls",
             "(a) parent build: n x mml_scan_download_pointxyzinormal + numpy double transform and repack per slot",
             "(b) n x mml_cloud_download_registered    (c) one mml_cloud_download_registered_batch",
             "equal = every record of (b) and of (c) holds the bytes of (a), and (a) is the same on both builds (SHA-256)",
             "",
             "%5s %10s %28s %28s %28s %8s %8s %6s" % ("n", "points", "(a) host loop ms", "(b) single calls ms", "(c) batch call ms", "(a)/(c)",
                                                     "(b)/(c)", "equal")]
    ok = True
    for rp, rn in zip(prev, new):
        eq = rp["sha"] == rn["sha"] and rn["single_differing_records"] == 0 and rn["batch_differing_records"] == 0
        ok &= eq
        lines.append("%5d %10d %28s %28s %28s %8.2f %8.2f %6s" % (rn["n"], rn["points"], f(rp["host"]), f(rn["single"]), f(rn["batch"]),
                                                               rp["host"]["ms"] / rn["batch"]["ms"], rn["single"]["ms"] / rn["batch"]["ms"], eq))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a record of the device calls differs from the host loop's")


if __name__ == "__main__":
    main()
