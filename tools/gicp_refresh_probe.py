"""Refreshing the extrinsic on n extracted slots: n sequential mml_gicp_refresh calls on a build of the PARENT commit against one
chained mml_gicp_refresh_batch call of this build.
    python tools/gicp_refresh_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 16, 64, 256, 1024 slots.

The single calls run on a build of the parent commit ($MML_LIB_PATH, as tools/lio_init_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
from a tight ctypes loop over one persistent matrix, in a process of their own; the new build runs the same slots through one
mml_gicp_refresh_batch(chain = 1, apply = 1) in a second process.  Each process opens the device and runs under a time limit of
its own, the second only after the first succeeded.  Every output matrix (the matrix held after each frame) and every
refreshed flag of the two runs are compared.

Inputs: distinct synthetic scans -- synth scans 14 .. 29, each turned about z by a multiple of 1.5 mrad per reuse, so no two slots
hold the same points -- extracted without an extrinsic.  apply = 1 moves a slot's Livox part, so every repetition starts from a
fresh mml_extract of the range, which only enqueues work: the setup waits for it (mml_synchronize) before the clock starts, so
neither arm pays for the extraction.  Times are host clock around the C-ABI calls, which end in a stream synchronise.  Per size: a warm-up, then at least 20 repetitions; median and the 10th / 90th percentile."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = 16          # distinct synth scans
T0 = np.eye(4, dtype=np.float32)
T0[:3, 3] = [0.02, -0.01, 0.03]


def timed(fn, setup, min_reps=20, warm=1):
    t = []
    for rep in range(warm + min_reps):
        setup()
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def scans(n):
    """n distinct (velo xyzi, livox records): base scan s % BASE turned about z by 1.5 mrad x (s // BASE)."""
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    base = [(synth.velo_scan(14 + k), synth.livox_scan(14 + k)) for k in range(min(BASE, n))]
    for s in range(n):
        v, l = base[s % BASE]
        a = 1.5e-3 * (s // BASE)
        if a == 0.0:
            yield v, l
            continue
        c, sn = np.float32(np.cos(a)), np.float32(np.sin(a))
        v2, l2 = v.copy(), l.copy()
        v2[:, 0], v2[:, 1] = c * v[:, 0] - sn * v[:, 1], sn * v[:, 0] + c * v[:, 1]
        l2["x"], l2["y"] = c * l["x"] - sn * l["y"], sn * l["x"] + c * l["y"]
        yield v2, l2


def worker(ns, mode, tmp):
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    nmax = max(ns)
    ctx = M.Context(max_scans=nmax)
    for s, (v, l) in enumerate(scans(nmax)):
        ctx.scan_upload(s, v, l)
    ctx.synchronize()
    T = np.zeros((nmax, 16), np.float32)
    ref = np.zeros(nmax, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    row = lambda a, i: C.c_void_p(a.ctypes.data + a.strides[0] * i)

    def single(k):
        cur = T0.reshape(16).copy()
        for s in range(k):
            if L.mml_gicp_refresh(ctx._h, s, p(cur), 1, row(ref, s), None) != 0:
                raise RuntimeError(L.mml_last_error(ctx._h).decode())
            T[s] = cur

    def batch(k):
        T[0] = T0.reshape(16)
        if L.mml_gicp_refresh_batch(ctx._h, 0, k, p(T), 1, 1, p(ref), None) != 0:
            raise RuntimeError(L.mml_last_error(ctx._h).decode())

    for k in ns:
        fn = single if mode == "prev" else batch
        r = dict(n=k, mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"))
        r["t"] = timed(lambda: fn(k), lambda: (ctx.extract(0, k), ctx.synchronize()))
        r["refreshed"] = int(ref[:k].sum())
        np.save(os.path.join(tmp, "%s_%d.npy" % (mode, k)), np.concatenate([T[:k], ref[:k, None].astype(np.float32)], axis=1))
        print("PROBE " + json.dumps(r), flush=True)
    ctx.close()


def run_worker(lib, ns, mode, tmp, limit):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--tmp", tmp] + [str(n) for n in ns], env=env,
                         capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_refresh_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker, a.tmp)
    ns = a.sizes or [1, 16, 64, 256, 1024]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    with tempfile.TemporaryDirectory() as tmp:
        prev = run_worker(a.prev, ns, "prev", tmp, a.limit)
        new = run_worker(None, ns, "new", tmp, a.limit)   # started only after the first succeeded
        diff = []
        for n in ns:
            x, y = np.load(os.path.join(tmp, "prev_%d.npy" % n)), np.load(os.path.join(tmp, "new_%d.npy" % n))
            diff.append((x.tobytes() == y.tobytes(), float(np.abs(x - y).max())))
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["refreshing the extrinsic on n extracted slots (distinct synthetic scans), one persistent matrix, apply = 1;",
             "ms, median [p10 .. p90] of >= 20 repetitions, host clock around the C-ABI calls",
             "single calls (parent build): n mml_gicp_refresh calls; batch call (new build): one mml_gicp_refresh_batch(chain = 1)",
             "refreshed = frames whose alignment converged; equal = all n matrices and flags of the two runs hold the same bytes",
             "",
             "%6s %10s %30s %30s %12s %12s %10s %6s %10s" % ("n", "refreshed", "single calls ms", "batch call ms", "single us/slot",
                                                             "batch us/slot", "speed-up", "equal", "max |dT|")]
    ok = True
    wins = None
    for rp, rn, (eq, dmax) in zip(prev, new, diff):
        n = rn["n"]
        s, b = rp["t"]["ms"], rn["t"]["ms"]
        lines.append("%6d %10d %30s %30s %12.1f %12.1f %10.2f %6s %10.3g" % (n, rn["refreshed"], f(rp["t"]), f(rn["t"]), 1e3 * s / n, 1e3 * b / n,
                                                                        s / b, eq, dmax))
        ok &= eq and rp["refreshed"] == rn["refreshed"]
        if b < s and wins is None:
            wins = n
        if b >= s:
            wins = None
    lines += ["", "the batch call is faster than the single calls from n = %s on" % wins if wins is not None else
              "the batch call is not faster than the single calls at the largest n measured"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a matrix of the batch call differs from the single calls'")


if __name__ == "__main__":
    main()
