"""The feature node's six clouds of n extracted slots (mml_feature_clouds_download_batch), timed three ways:
  (a) YARDSTICK, on a build of the PARENT commit: n x mml_scan_download_pointxyzinormal -- the only cloud the parent can deliver.
      It covers the two combine clouds alone, so it is a yardstick for that shared part, not an equivalent;
  (b) n x mml_feature_clouds_download;
  (c) one mml_feature_clouds_download_batch.
    python tools/feature_clouds_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 64, 512 slots of the BASELINE configs[1] scan (16 rings x 1800 azimuths + 24 000 Livox points), synth scans
14 .. 29 reused round robin, extracted.

(a) runs on the parent build ($MML_LIB_PATH, as tools/registered_cloud_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
in a process of its own; (b) and (c) run on this build in a second process, started only after the first succeeded, each under
a time limit of its own.  All write into one preallocated host buffer and none makes a sizing call (the counts are known from the
setup).  Every byte of (c) is compared with (b); the combine clouds inside them are compared with (a)'s clouds through a SHA-256
over both builds.  Times are host clock around the calls, which end in a stream synchronise.  Per size: a warm-up, then at least
20 repetitions; median and the 10th / 90th percentile.  The table also sets the n = 1 time next to one B = 1 mml_step (0.33 ms,
BASELINE.md)."""
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
STEP_MS = 0.33     # one B = 1 mml_step


def timed(fn, min_reps=20, warm=1):
    t = []
    for rep in range(warm + min_reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def worker(ns, mode):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    L = M.lib()
    nmax = max(ns)
    ctx = M.Context(max_scans=nmax)
    base = [(synth.velo_scan(14 + k), synth.livox_scan(14 + k)) for k in range(min(BASE, nmax))]
    for s in range(nmax):
        ctx.scan_upload(s, *base[s % BASE])
    ctx.extract(0, nmax)
    infos = [ctx.scan_info(s) for s in range(nmax)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    at = lambda a, i: C.c_void_p(a.ctypes.data + a.strides[0] * i)

    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.mml_last_error(ctx._h).decode())

    def fused(k, out, nn):
        off = 0
        for s in range(k):
            ck(L.mml_scan_download_pointxyzinormal(ctx._h, s, at(out, off), len(out) - off, at(nn, s)))
            off += int(nn[s])

    def single(k, out, nn):
        off = 0
        for s in range(k):
            ck(L.mml_feature_clouds_download(ctx._h, s, at(out, off), len(out) - off, at(nn, 6 * s)))
            off += int(nn[6 * s:6 * s + 6].sum())

    def batch(k, out, nn):
        ck(L.mml_feature_clouds_download_batch(ctx._h, 0, k, p(out), len(out), p(nn)))

    for k in ns:
        r = dict(n=k, mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"))
        n_fused = sum(i.n_points for i in infos[:k])
        fo, fn_ = np.zeros((n_fused, 12), np.float32), np.zeros(k, np.int32)
        if mode == "prev":
            r["fused"] = timed(lambda: fused(k, fo, fn_))
            r["sha"] = hashlib.sha256(fo.tobytes()).hexdigest()
        else:
            total = sum(i.n_points + i.velo_corner_num + i.velo_surf_num + i.livox_corner_num + i.livox_surf_num for i in infos[:k])
            a, b = np.zeros((total, 12), np.float32), np.zeros((total, 12), np.float32)
            na, nb = np.zeros(6 * k, np.int32), np.zeros(6 * k, np.int32)
            r["single"] = timed(lambda: single(k, a, na))
            r["batch"] = timed(lambda: batch(k, b, nb))
            r["points"] = total
            r["differing_bytes"] = int((a.view(np.uint8) != b.view(np.uint8)).sum()) + int((na != nb).sum())
            ends = np.cumsum(nb)
            comb = [b[ends[6 * s + c] - nb[6 * s + c]:ends[6 * s + c]] for s in range(k) for c in (2, 5)]
            r["sha"] = hashlib.sha256(np.concatenate(comb).tobytes()).hexdigest()
        r["fused_points"] = n_fused
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_clouds_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker)
    ns = a.sizes or [1, 64, 512]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    prev = run_worker(a.prev, ns, "prev", a.limit)
    new = run_worker(None, ns, "new", a.limit)   # started only after the first succeeded
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["tools/feature_clouds_probe.py: the six union_cloud clouds of n extracted slots (16 x 1800 + 24 000 points each), into one host buffer;",
             "ms, median [p10 .. p90] of >= 20 repetitions, host clock around the calls",
             "(a) yardstick, parent build: n x mml_scan_download_pointxyzinormal (the two combine clouds only -- not an equivalent)",
             "(b) n x mml_feature_clouds_download    (c) one mml_feature_clouds_download_batch",
             "equal = every byte of (c) is (b)'s, and the combine clouds inside them are (a)'s on the parent build (SHA-256)",
             "",
             "%5s %10s %10s %28s %28s %28s %8s %6s" % ("n", "points", "fused", "(a) parent, fused only ms", "(b) single calls ms", "(c) batch call ms",
                                                      "(b)/(c)", "equal")]
    ok = slower = True
    for rp, rn in zip(prev, new):
        eq = rp["sha"] == rn["sha"] and rn["differing_bytes"] == 0
        ok &= eq
        lines.append("%5d %10d %10d %28s %28s %28s %8.2f %6s" % (rn["n"], rn["points"], rn["fused_points"], f(rp["fused"]), f(rn["single"]), f(rn["batch"]),
                                                               rn["single"]["ms"] / rn["batch"]["ms"], eq))
    one = [r for r in new if r["n"] == 1]
    if one:
        lines += ["", "n = 1: %.3f ms for the message against %.2f ms for one B = 1 mml_step (%.2f steps)" % (one[0]["batch"]["ms"], STEP_MS,
                                                                                                        one[0]["batch"]["ms"] / STEP_MS)]
    last = new[-1]
    slower = last["batch"]["ms"] > last["single"]["ms"]
    lines.append("n = %d: the batch call is %s than the %d single calls" % (last["n"], "SLOWER" if slower else "not slower", last["n"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: the batch call, the single calls and the parent's fused cloud do not hold the same bytes")
    if slower:
        sys.exit("FINDING: the batch call is slower than the single calls at n = %d" % last["n"])


if __name__ == "__main__":
    main()
