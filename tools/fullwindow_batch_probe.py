"""n sequential mml_fullwindow_solve calls against one mml_fullwindow_solve_batch call on the same n problems.
    python tools/fullwindow_batch_probe.py [--prev <parent .so>] [--out <table>] [W] [n ...]
Defaults: W = 5 (the reference's SLIDEWINDOWSIZE) and W = 8; n = 1, 8, 64, 256, 1024.

The sequential baseline comes from a build of the PARENT commit ($MML_LIB_PATH, as tools/ab_bench.sh does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
which also shows whether the single call changed.  Every library runs in a process of its own, in the order parent (single
call only) / new / parent, so the two parent figures for the single call bracket the new one: their difference is the run-to-run
spread the parent / new ratio has to be read against.

A problem: W frames in slots 0 .. W - 1 (synthetic scans, extracted, down-sampled and associated at perturbed poses against a
map of the eight scans before them), IMU factors, a prior marginalized from a first solve; window w starts from its own
perturbation of the poses, so that iteration counts differ inside a batch.  Times are host clock around the C-ABI call, which
ends in a stream synchronise; arguments are marshalled before the clock starts.  Per (W, n): warm-up, then at least 20
repetitions and at least 1 s of timed work; median and the 10th / 90th percentile."""
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


def timed(fn, min_reps=20, min_s=1.0, warm=3):
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


def worker(W, ns, modes):
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
    prior = fw.marginalize(c.linearize_window(0, 1, xs[:1], west.T_bl, 3e-4, 0.0)[0], xs) if W >= 2 else None
    nmax = max(ns)
    fws = [make(prior) for _ in range(nmax)]
    start = np.zeros((nmax, M.FW_X_STRIDE))
    for w in range(nmax):
        xw = x0.copy()
        xw[:, :3] += rng.normal(0, 0.01, (W, 3))
        xw[:, 3:6] += rng.normal(0, 0.002, (W, 3))
        start[w, :15 * W] = xw.reshape(-1)
    handles = (C.c_void_p * nmax)(*[f._h.value for f in fws])
    first = np.zeros(nmax, np.int32)
    summ = (M.SolveSummary * nmax)()
    ev = np.zeros(nmax, np.int32)
    x = start.copy()
    pT, px, pf, pe = T_bl.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p)
    rows = [C.c_void_p(x.ctypes.data + 8 * M.FW_X_STRIDE * w) for w in range(nmax)]
    hs = [C.c_void_p(handles[w]) for w in range(nmax)]
    for n in ns:
        r = dict(W=W, n=n, lib=os.environ.get("MML_LIB_PATH", "default"))

        def seq():
            x[:n] = start[:n]
            for w in range(n):
                if L.mml_fullwindow_solve(c._h, hs[w], 0, pT, rows[w], None, None) != 0:
                    raise RuntimeError("mml_fullwindow_solve failed")

        def batch():
            x[:n] = start[:n]
            if L.mml_fullwindow_solve_batch(c._h, n, handles, pf, pT, px, summ, pe, None) != 0:
                raise RuntimeError(L.mml_last_error(c._h).decode())

        if "seq" in modes:
            r["seq"] = timed(seq)
            x_seq = x[:n].copy()
        if "batch" in modes:
            r["batch"] = timed(batch)
            r["iterations"] = [int(min(s.iterations for s in summ[:n])), int(max(s.iterations for s in summ[:n]))]
            r["evaluations"] = float(np.mean(ev[:n]))
            if "seq" in modes:
                r["equal"] = bool(np.array_equal(x_seq, x[:n]))
        print("PROBE " + json.dumps(r), flush=True)
    c.close()


def run_worker(lib, W, ns, modes):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", modes, str(W)] + [str(n) for n in ns], env=env,
                         capture_output=True, text=True, timeout=1500)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullwindow_batch_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes[0], a.sizes[1:], a.worker.split("+"))
    Ws = [a.sizes[0]] if a.sizes else [5, 8]
    ns = a.sizes[1:] or [1, 8, 64, 256, 1024]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    lines = ["full-window solve: n sequential mml_fullwindow_solve calls (parent build, new build) against one",
             "mml_fullwindow_solve_batch call on the same problems; ms per call sequence, median [p10 .. p90] of >= 20 repetitions / >= 1 s",
             ""]
    ok = True
    for W in Ws:
        p0 = run_worker(a.prev, W, [1], "seq")[0]
        new = run_worker(None, W, ns, "seq+batch")
        prev = run_worker(a.prev, W, ns, "seq")
        lines.append("W = %d   (iterations per window %s, mean evaluations %.1f)" % (W, new[-1]["iterations"], new[-1]["evaluations"]))
        lines.append("%6s %28s %28s %28s %12s %12s %12s %9s %6s" % ("n", "sequential parent ms", "sequential new ms", "batch ms", "seq us/win", "batch us/win",
                                                                "batch win/s", "speed-up", "equal"))
        for rn, rp in zip(new, prev):
            f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
            n = rn["n"]
            lines.append("%6d %28s %28s %28s %12.1f %12.1f %12.0f %9.1f %6s" % (
                n, f(rp["seq"]), f(rn["seq"]), f(rn["batch"]), 1e3 * rn["seq"]["ms"] / n, 1e3 * rn["batch"]["ms"] / n, 1e3 * n / rn["batch"]["ms"],
                rn["seq"]["ms"] / rn["batch"]["ms"], rn["equal"]))
            ok &= rn["equal"]
            if n == 64:
                ok &= rn["batch"]["ms"] < rn["seq"]["ms"]
        one = [r for r in new if r["n"] == 1]
        if one:
            lines.append("single call: parent before %.4f ms, new %.4f ms, parent after %.4f ms -> parent / new %.3f and %.3f (parent run-to-run %.3f)" % (
                p0["seq"]["ms"], one[0]["seq"]["ms"], prev[0]["seq"]["ms"], p0["seq"]["ms"] / one[0]["seq"]["ms"],
                prev[0]["seq"]["ms"] / one[0]["seq"]["ms"], p0["seq"]["ms"] / prev[0]["seq"]["ms"]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    if not ok:
        sys.exit("FINDING: a batch differs from the sequential results, or the batch at n = 64 is not faster per window than the sequential calls")


if __name__ == "__main__":
    main()
