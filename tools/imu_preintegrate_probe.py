"""Pre-integrating n IMU intervals: n mml_imu_preintegrate calls (the parent commit's host routine) against the host loop
and the device call of mml_imu_preintegrate_batch.
    python tools/imu_preintegrate_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 4, 64, 1024, 7168 intervals of 20 and of 40 samples (synth.imu_samples has 20 per interval at 200 Hz, a Livox
IMU gives 20 - 40).

The single calls run on a build of the PARENT commit ($MML_LIB_PATH, as tools/fullwindow_marginalize_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
from a tight ctypes loop, one call per interval, in a process of their own.  The new build runs the same intervals through
mml_imu_preintegrate_batch with a NULL context (the host loop of csrc/imu_preint.h) and with a context (one upload, one launch of
k_imu_preintegrate, one read-back), and compares the bytes of the two.

Inputs: the family of tests/test_imu.py from a fixed seed, a bias pair per interval.  Times are host clock around the C-ABI
calls -- the device call ends in a stream synchronise -- with the arguments marshalled before the clock starts.  Per size:
a warm-up, then at least 5 repetitions and at least 0.5 s of timed work; median and the 10th / 90th percentile."""
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
LENGTHS = (20, 40)


def timed(fn, min_reps=5, min_s=0.5, warm=2):
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
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    ctx = M.Context(max_scans=1) if mode == "new" else None
    nmax = max(ns)
    for k in LENGTHS:
        rng = np.random.default_rng(100 + k)
        smp = np.concatenate([rng.normal(0, 0.3, (nmax * k, 3)), rng.normal(0, 0.2, (nmax * k, 3)) + [0, 0, 1.0],
                              rng.uniform(0.004, 0.006, (nmax * k, 1))], axis=1)
        bg, ba = rng.normal(0, 0.01, (nmax, 3)), rng.normal(0, 0.03, (nmax, 3))
        offsets = (k * np.arange(nmax + 1)).astype(np.int32)
        out = (M.ImuPreint * nmax)()
        ps, po, pg, pa = (a.ctypes.data_as(C.c_void_p) for a in (smp, offsets, bg, ba))
        rows = [C.c_void_p(smp.ctypes.data + 56 * k * i) for i in range(nmax)]
        gs = [C.c_void_p(bg.ctypes.data + 24 * i) for i in range(nmax)]
        as_ = [C.c_void_p(ba.ctypes.data + 24 * i) for i in range(nmax)]
        outs = [C.byref(out[i]) for i in range(nmax)]
        kk = C.c_int(k)

        def single(n):
            for i in range(n):
                if L.mml_imu_preintegrate(rows[i], kk, gs[i], as_[i], outs[i]) != 0:
                    raise RuntimeError("mml_imu_preintegrate failed")

        def batch(n, h):
            if L.mml_imu_preintegrate_batch(h, n, ps, po, pg, pa, out) != 0:
                raise RuntimeError(L.mml_last_error(h).decode() if h else "mml_imu_preintegrate_batch failed")

        for n in ns:
            r = dict(n=n, k=k, lib=os.environ.get("MML_LIB_PATH", "default"))
            if mode == "prev":
                r["single"] = timed(lambda: single(n))
            else:
                r["host"] = timed(lambda: batch(n, None))
                ref = bytes(out)[:C.sizeof(M.ImuPreint) * n]
                r["device"] = timed(lambda: batch(n, ctx._h))
                r["equal"] = bytes(out)[:C.sizeof(M.ImuPreint) * n] == ref
            print("PROBE " + json.dumps(r), flush=True)
    if ctx is not None:
        ctx.close()


def run_worker(lib, ns, mode):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode] + [str(n) for n in ns], env=env,
                         capture_output=True, text=True, timeout=420)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_preintegrate_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker)
    ns = a.sizes or [1, 4, 64, 1024, 7168]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    prev = run_worker(a.prev, ns, "prev")
    new = run_worker(None, ns, "new")
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["pre-integrating n IMU intervals of k samples; ms, median [p10 .. p90] of >= 5 repetitions / >= 0.5 s",
             "single calls (parent build): n mml_imu_preintegrate calls; host loop / device call (new build):",
             "mml_imu_preintegrate_batch with a NULL context / with a context",
             "",
             "%4s %6s %26s %26s %26s %11s %11s %11s %9s %6s" % ("k", "n", "single calls ms", "host loop ms", "device call ms", "single us/i",
                                                              "host us/i", "dev us/i", "speed-up", "equal")]
    ok = True
    for rp, rn in zip(prev, new):
        n = rn["n"]
        s, h, d = rp["single"]["ms"], rn["host"]["ms"], rn["device"]["ms"]
        lines.append("%4d %6d %26s %26s %26s %11.2f %11.2f %11.2f %9.2f %6s" % (rn["k"], n, f(rp["single"]), f(rn["host"]), f(rn["device"]),
                                                                           1e3 * s / n, 1e3 * h / n, 1e3 * d / n, s / d, rn["equal"]))
        ok &= rn["equal"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a device pre-integration differs from the host build's")


if __name__ == "__main__":
    main()
