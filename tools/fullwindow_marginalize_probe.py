"""Marginalizing frame 0 of n solved windows: the host path of the parent commit against one
mml_fullwindow_marginalize_batch call.
    python tools/fullwindow_marginalize_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: W = 5 (the reference's SLIDEWINDOWSIZE); n = 1, 16, 64, 300, 1024.

The host path runs on a build of the PARENT commit ($MML_LIB_PATH, as tools/fullwindow_batch_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
It is what BatchWindowEstimator(marginalize="host") pays per outer iteration that closes windows: the frame-0 records of the
batch solve (records0: one more launch and read-back, timed as the difference of the batch solve with and without them) plus
n mml_fullwindow_marginalize calls from a tight ctypes loop.  The device path on the new build is one
mml_fullwindow_marginalize_batch call, which needs no records.  Each library runs in a process of its own.

A problem: as in tools/fullwindow_batch_probe.py -- W frames in slots 0 .. W - 1, IMU factors, a prior marginalized from a
first solve, window w solved from its own perturbation of the poses; every window is marginalized at its own solution.  Times
are host clock around the C-ABI calls, which end in a stream synchronise; arguments are marshalled before the clock starts.
Per n: warm-up, then at least 20 repetitions and at least 0.5 s of timed work; median and the 10th / 90th percentile."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K0 = 40
W = 5


def timed(fn, min_reps=20, min_s=0.5, warm=3):
    for _ in range(warm):
        fn()
    t, total = [], 0.0
    while len(t) < min_reps or total < min_s:
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        total += t[-1]
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def worker(ns, mode):
    from scipy.spatial.transform import Rotation as Rsc
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    L = M.lib()
    c = M.Context(max_scans=8)
    cm, sm = [], []
    for k in range(K0 - 8, K0):
        c.scan_upload(0, synth.velo_scan(k), synth.livox_scan(k))
        c.extract(0, 1)
        c.undistort(0, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
        c.downsample(0, 1)
        T = synth.pose_matrix(k)
        cm.append(synth.transform(T, c.features_download(0, 0).astype(np.float64)).astype(np.float32))
        sm.append(synth.transform(T, c.features_download(0, 1).astype(np.float64)).astype(np.float32))
    c.map_set_local(0, synth.voxel_filter(np.concatenate(cm), c.cfg.leaf_corner))
    c.map_set_local(1, synth.voxel_filter(np.concatenate(sm), c.cfg.leaf_surf))
    west = odometry.WindowEstimator(c, gravity=synth.GRAVITY)
    T_bl = np.ascontiguousarray(west.T_bl.reshape(16))
    rng = np.random.default_rng(11)
    x0, pres = [], [None]
    for f in range(W):
        k = K0 + f
        c.scan_upload(f, synth.velo_scan(k), synth.livox_scan(k))
        c.extract(f, 1)
        c.undistort(f, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
        c.downsample(f, 1)
        T = synth.pose_matrix(k).copy()
        T[:3, :3] = T[:3, :3] @ Rsc.from_rotvec(rng.normal(0, 0.003, 3)).as_matrix()
        T[:3, 3] += rng.normal(0, 0.02, 3)
        x0.append(np.concatenate([T[:3, 3], Rsc.from_matrix(T[:3, :3]).as_rotvec(), synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                  np.zeros(3), np.zeros(3)]))
        if f > 0:
            pres.append(M.imu_preintegrate(synth.imu_samples(k - 1, k), np.zeros(3), np.zeros(3)))
        c.associate(f, 1, west._T_wl(x0[f])[None], 1.0)
    x0 = np.stack(x0)

    def make(prior):
        fw = M.FullWindowSolver(W, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4)
        for f in range(1, W):
            fw.set_imu(f, pres[f], synth.GRAVITY)
        if prior is not None:
            fw.set_prior(prior)
        return fw

    fw = make(None)
    xs, _, _ = fw.solve_device(c, 0, west.T_bl, x0)
    prior = fw.marginalize(c.linearize_window(0, 1, xs[:1], west.T_bl, 3e-4, 0.0)[0], xs)
    nmax = max(ns)
    fws = [make(prior) for _ in range(nmax)]
    start = np.zeros((nmax, M.FW_X_STRIDE))
    for w in range(nmax):
        xw = x0.copy()
        xw[:, :3] += rng.normal(0, 0.01, (W, 3))
        xw[:, 3:6] += rng.normal(0, 0.002, (W, 3))
        start[w, :15 * W] = xw.reshape(-1)
    handles = (C.c_void_p * nmax)(*[f._h.value for f in fws])
    hs = [C.c_void_p(handles[w]) for w in range(nmax)]
    first = np.zeros(nmax, np.int32)
    x = start.copy()
    rec = np.zeros((nmax, 32))
    out = (M.Prior * nmax)()
    pT, px, pf, pr = (a.ctypes.data_as(C.c_void_p) for a in (T_bl, x, first, rec))
    rows = [C.c_void_p(x.ctypes.data + 8 * M.FW_X_STRIDE * w) for w in range(nmax)]
    recs = [C.c_void_p(rec.ctypes.data + 8 * 32 * w) for w in range(nmax)]
    outs = [C.byref(out[w]) for w in range(nmax)]

    def solve(n, records):
        x[:n] = start[:n]
        if L.mml_fullwindow_solve_batch(c._h, n, handles, pf, pT, px, None, None, pr if records else None) != 0:
            raise RuntimeError(L.mml_last_error(c._h).decode())

    def host_loop(n):
        for w in range(n):
            if L.mml_fullwindow_marginalize(hs[w], recs[w], rows[w], outs[w]) != 0:
                raise RuntimeError("mml_fullwindow_marginalize failed")

    def device(n):
        if L.mml_fullwindow_marginalize_batch(c._h, n, handles, pf, pT, px, out) != 0:
            raise RuntimeError(L.mml_last_error(c._h).decode())

    for n in ns:
        r = dict(n=n, lib=os.environ.get("MML_LIB_PATH", "default"))
        r["solve"] = timed(lambda: solve(n, False))
        r["solve_rec"] = timed(lambda: solve(n, True))     # leaves x and rec at the solution
        if mode == "host":
            r["loop"] = timed(lambda: host_loop(n))
        else:
            host_loop(n)
            ref = bytes(out)[:C.sizeof(M.Prior) * n]
            r["device"] = timed(lambda: device(n))
            r["equal"] = bytes(out)[:C.sizeof(M.Prior) * n] == ref
        print("PROBE " + json.dumps(r), flush=True)
    c.close()


def run_worker(lib, ns, mode):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode] + [str(n) for n in ns], env=env,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullwindow_marginalize_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker)
    ns = a.sizes or [1, 16, 64, 300, 1024]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    prev = run_worker(a.prev, ns, "host")
    new = run_worker(None, ns, "device")
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["marginalizing frame 0 of n solved windows (W = %d, with prior); ms, median [p10 .. p90] of >= 20 repetitions / >= 0.5 s" % W,
             "host path (parent build): records0 = batch solve with the frame-0 records minus the same solve without, plus n",
             "mml_fullwindow_marginalize calls; device path (new build): one mml_fullwindow_marginalize_batch call",
             "",
             "%6s %26s %26s %26s %26s %12s %12s %9s %6s" % ("n", "solve ms (parent)", "solve + records0 ms", "host loop ms", "device call ms",
                                                            "host us/win", "dev us/win", "speed-up", "equal")]
    ok = True
    for rp, rn in zip(prev, new):
        n = rn["n"]
        host = rp["loop"]["ms"] + max(0.0, rp["solve_rec"]["ms"] - rp["solve"]["ms"])
        dev = rn["device"]["ms"]
        lines.append("%6d %26s %26s %26s %26s %12.1f %12.1f %9.1f %6s" % (n, f(rp["solve"]), f(rp["solve_rec"]), f(rp["loop"]), f(rn["device"]),
                                                                      1e3 * host / n, 1e3 * dev / n, host / dev, rn["equal"]))
        ok &= rn["equal"]
        if n == 64:
            ok &= dev < host
    lines.append("")
    lines.append("batch solve on the new build, ms: " + ", ".join("n = %d: %.3f" % (r["n"], r["solve"]["ms"]) for r in new))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a device prior differs from the host's, or the device call at n = 64 is not faster per window than the parent's host path")


if __name__ == "__main__":
    main()
