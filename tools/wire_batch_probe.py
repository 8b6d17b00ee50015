"""n union_cloud messages in wire form into n scan slots, the feature node's way in, measured two ways.
    python tools/wire_batch_probe.py [--prev <parent .so>] [--staged <LDS-staged .so>] [--out <table>] [n ...]

1. THE CALLS, host clock.  n = 1, 16, 64 frames of 28 800 Velodyne records (22 bytes: x y z intensity float32, ring uint16, time
   float32) and 24 000 Livox records (19 bytes), random bytes, laid out in one buffer per sensor with 64-byte gaps (message headers):
     (a) on a build of the PARENT commit ($MML_LIB_PATH): n mml_scan_upload_wire calls, then mml_synchronize;
     (b) on this build: one mml_scan_upload_wire_batch call, then mml_synchronize.
   A warm-up, then at least 10 repetitions; median and the 10th / 90th percentile.  EVERY slot is compared: the bytes
   mml_scan_raw_download returns for all n slots must be the same on both builds.
2. THE KERNELS, `rocprofv3 --kernel-trace --stats`, each in a run of its own (tracing slows the host: no call time is taken there).
   One frame of 28 800 x 22-byte, one of 28 800 x 32-byte and one of 24 000 x 19-byte records, each alone in its call, through
     parent  k_decode_pointcloud2 / k_decode_custompoints (mml_scan_upload_wire on the parent build),
     batch   k_wire_decode_batch of this build (256 records per workgroup, per-lane byte loads),
     staged  k_wire_decode_batch compiled with -DMML_WIRE_STAGED=16384 (a tile of at most 16 KB parked in LDS by 16-byte loads,
             fields assembled from LDS), when --staged names such a build:
             make -C multi-modal-loam_amd/csrc BUILD=build_staged OUT=<.so> EXTRA=-DMML_WIRE_STAGED=16384
   Every build is profiled twice, alternating, so that the run-to-run spread stands beside the difference.  Per kernel and case:
   median us of the dispatches after the first three, [min .. max], and payload bytes over that time.
The parent build:  make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so   (at the parent commit).
Every device process runs under a time limit of its own and the next one starts only after it succeeded."""
import argparse
import csv
import ctypes as C
import glob
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NV, NL, STEP, GAP = 28800, 24000, 22, 64
KERNEL_CASES = [("28800 x 22 B", 0, NV, 22), ("28800 x 32 B", 0, NV, 32), ("24000 x 19 B", 1, NL, 19)]   # name, sensor, records, bytes
KERNEL_REPS, KERNEL_SKIP = 23, 3
KERNELS = ("k_decode_pointcloud2", "k_decode_custompoints", "k_wire_decode_batch")


def timed(fn, min_reps=10, warm=1):
    t = []
    for rep in range(warm + min_reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def lay_out(rng, n, records, rec_bytes):
    """n payloads of random bytes in one buffer, a GAP of 0xA5 in front of each; (buffer, int64 offsets)."""
    stride = GAP + records * rec_bytes
    buf = np.full(n * stride, 0xA5, np.uint8)
    at = GAP + stride * np.arange(n, dtype=np.int64)
    for a in at:
        buf[a:a + records * rec_bytes] = rng.integers(0, 256, records * rec_bytes, dtype=np.uint8)
    return buf, at


def p(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def worker_calls(ns, mode):
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    nmax = max(ns)
    ctx = M.Context(max_scans=nmax, max_velo_points=NV, max_livox_points=NL)
    rng = np.random.default_rng(1)
    vd, va = lay_out(rng, nmax, NV, STEP)
    ld, la = lay_out(rng, nmax, NL, 19)

    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.mml_last_error(ctx._h).decode())

    def single(k):
        for i in range(k):
            ck(L.mml_scan_upload_wire(ctx._h, i, p(vd[va[i]:]), NV, STEP, 0, 4, 8, 12, p(ld[la[i]:]), NL))
        ck(L.mml_synchronize(ctx._h))

    def batch(k):
        nv, nl = np.full(k, NV, np.int32), np.full(k, NL, np.int32)
        ck(L.mml_scan_upload_wire_batch(ctx._h, 0, k, p(vd), p(va), p(nv), STEP, 0, 4, 8, 12, p(ld), p(la), p(nl), 19))
        ck(L.mml_synchronize(ctx._h))

    for k in ns:
        r = dict(n=k, mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"), mbytes=k * (NV * STEP + NL * 19) / 1e6)
        r["t"] = timed(lambda: single(k) if mode == "prev" else batch(k))
        h = hashlib.sha256()
        for s in range(k):
            v, l = ctx.scan_raw_download(s)
            assert len(v) == NV and len(l) == NL
            h.update(v.tobytes())
            h.update(l.tobytes())
        r["raw"] = h.hexdigest()
        print("PROBE " + json.dumps(r), flush=True)
    ctx.close()


def worker_kernels(mode):
    """KERNEL_REPS rounds over the three cases, one frame per call (dispatch i of the decode kernels is case i mod 3)."""
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    ctx = M.Context(max_scans=1, max_velo_points=NV, max_livox_points=NL)
    rng = np.random.default_rng(2)
    data = [lay_out(rng, 1, n, rec) for _, _, n, rec in KERNEL_CASES]
    one, zero, at0 = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64)
    for _ in range(KERNEL_REPS):
        for (name, sensor, n, rec), (buf, at) in zip(KERNEL_CASES, data):
            one[0] = n
            if mode == "prev":
                rc = L.mml_scan_upload_wire(ctx._h, 0, p(buf[at[0]:]), n, rec, 0, 4, 8, 12, None, 0) if sensor == 0 else \
                    L.mml_scan_upload_wire(ctx._h, 0, None, 0, 22, 0, 4, 8, 12, p(buf[at[0]:]), n)
            elif sensor == 0:
                rc = L.mml_scan_upload_wire_batch(ctx._h, 0, 1, p(buf), p(at), p(one), rec, 0, 4, 8, 12, None, p(at0), p(zero), 19)
            else:
                rc = L.mml_scan_upload_wire_batch(ctx._h, 0, 1, None, p(at0), p(zero), 22, 0, 4, 8, 12, p(buf), p(at), p(one), rec)
            if rc != 0 or L.mml_synchronize(ctx._h) != 0:
                raise RuntimeError(L.mml_last_error(ctx._h).decode())
    ctx.close()
    print("KERNELS_DONE", flush=True)


def run_worker(lib, args, limit, prof_dir=None):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if prof_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "wire", "--"] + cmd
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, (out.stdout + out.stderr)[-2000:]))
    return out.stdout


def kernel_times(prof_dir):
    """Per case the durations (us) of the decode kernels' dispatches, in dispatch order, from the kernel trace."""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise RuntimeError("expected one kernel trace under %s, found %r" % (prof_dir, files))
    rows = [r for r in csv.DictReader(open(files[0])) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != KERNEL_REPS * len(KERNEL_CASES):
        raise RuntimeError("%d decode dispatches in the trace, %d expected" % (len(rows), KERNEL_REPS * len(KERNEL_CASES)))
    us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]).reshape(KERNEL_REPS, len(KERNEL_CASES))
    names = [next(k for k in KERNELS if k in rows[c]["Kernel_Name"]) for c in range(len(KERNEL_CASES))]
    return names, us[KERNEL_SKIP:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--staged", default=None, help="a build with -DMML_WIRE_STAGED=16384, for the kernel comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_batch_probe.txt"))
    ap.add_argument("--prof", default=os.path.join(ROOT, "tools_tmp", "wire_batch_prof"), help="directory for the profiler's files")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker in ("prev", "new"):
        return worker_calls(a.sizes, a.worker)
    if a.worker:
        return worker_kernels(a.worker.split(":")[1])
    ns = a.sizes or [1, 16, 64]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    sizes = [str(n) for n in ns]
    parse = lambda text: [json.loads(ln[6:]) for ln in text.splitlines() if ln.startswith("PROBE ")]
    prev = parse(run_worker(a.prev, ["--worker", "prev"] + sizes, a.limit))
    new = parse(run_worker(None, ["--worker", "new"] + sizes, a.limit))   # started only after the first succeeded
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["tools/wire_batch_probe.py: n union_cloud messages in wire form (28 800 x 22-byte PointCloud2 records + 24 000 x 19-byte",
             "CustomPoint records each, 64-byte gaps between the payloads) into n scan slots",
             "",
             "1. the calls: ms, median [p10 .. p90] of >= 10 repetitions, host clock, both ending in mml_synchronize",
             "(a) parent build: n mml_scan_upload_wire calls     (b) this build: one mml_scan_upload_wire_batch call",
             "equal = mml_scan_raw_download of every one of the n slots returns the same bytes on both builds",
             "",
             "%5s %10s %28s %28s %8s %10s %6s" % ("n", "wire MB", "(a) n single calls ms", "(b) one batch call ms", "(a)/(b)", "(b) GB/s", "equal")]
    ok = True
    for rp, rn in zip(prev, new):
        eq = rp["raw"] == rn["raw"]
        ok &= eq
        lines.append("%5d %10.2f %28s %28s %8.2f %10.2f %6s" % (rn["n"], rn["mbytes"], f(rp["t"]), f(rn["t"]), rp["t"]["ms"] / rn["t"]["ms"],
                                                            rn["mbytes"] / rn["t"]["ms"], eq))
    lines += ["", "2. the decode kernels: rocprofv3 --kernel-trace --stats, one frame per call, us per dispatch, median [min .. max] of %d"
              % (KERNEL_REPS - KERNEL_SKIP),
              "dispatches, and payload bytes (records x record size) over the median; every build profiled twice, alternating",
              "",
              "%-14s %-8s %-24s %26s %10s" % ("case", "build", "kernel", "us", "GB/s")]
    builds = [("parent", a.prev, "prev"), ("batch", None, "new")] + ([("staged", a.staged, "new")] if a.staged else [])
    for rnd in range(2):
        for label, lib, mode in builds:
            d = os.path.join(a.prof, "%s_%d" % (label, rnd))
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d)
            run_worker(lib, ["--worker", "kernels:" + mode], a.limit, prof_dir=d)
            names, us = kernel_times(d)
            for c, (case, _, n, rec) in enumerate(KERNEL_CASES):
                med = float(np.median(us[:, c]))
                lines.append("%-14s %-8s %-24s %26s %10.1f" % (case, "%s #%d" % (label, rnd + 1), names[c],
                                                             "%.2f [%.2f .. %.2f]" % (med, us[:, c].min(), us[:, c].max()), n * rec / med / 1e3))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: the batch call and the parent's single calls do not leave the same slots")


if __name__ == "__main__":
    main()
