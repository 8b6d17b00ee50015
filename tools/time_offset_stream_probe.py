"""The aligner's time-offset estimation, hand-composed on a build of the PARENT commit against one
mml_time_offset_estimate_stream call of this build.
    python tools/time_offset_stream_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1 and 8 Velodyne frames of 28 800 points against 192 000 stream points (eight Livox messages of 24 000),
search_resolution 30, 12 000 sliced points.

The yardstick runs on a build of the parent commit ($MML_LIB_PATH, as tools/time_offset_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
and is what a caller of that build has to do: mml_velo_fov_select_batch (sizing call and filling call), the host merge of the
last eight messages it kept beside the stream into an n x 3 array, mml_time_offset_search_batch with that array given once per
frame, then the stamp of the best window from its own offsets -- the host hand-over included.  The new build makes one
mml_time_offset_estimate_stream call on the resident stream.  In both processes the messages are pushed to a stream before the
clock starts (both callers hold one), the clock is the host's around the calls, and the context is synchronised at both ends.
Each process opens the device and runs under a time limit of its own, the second only after the first succeeded.  Every
output is compared: n_kept, n_windows, best_window, lowest_error, optim_start, all window errors, all distances."""
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
RES, SLICED, MSGS, MSG_PTS = 30, 12000, 8, 24000
T0 = 1600000000 * 10 ** 9
REPS = 20


def timed(ctx, fn):
    t = []
    for rep in range(1 + REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if rep >= 1:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def worker(ns, mode, tmp):
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    ctx = M.Context(max_scans=1)
    msgs = [synth.livox_scan(40 + j, motion=True) for j in range(MSGS)]
    tbs = [T0 + j * 100000000 for j in range(MSGS)]
    for m in msgs:
        m["offset_time"] = (np.arange(len(m), dtype=np.uint64) * 4000).astype(np.uint32)
    frames = [np.ascontiguousarray(synth.velo_scan(40 + k)) for k in range(max(ns))]
    stamps = [T0 + 5 * 10 ** 8 + 1000 * k for k in range(max(ns))]
    st = ctx.livox_stream(MSGS * MSG_PTS)
    for tb, m in zip(tbs, msgs):
        st.push(tb, m)
    offs = np.concatenate([np.uint64(tb) + m["offset_time"].astype(np.uint64) for tb, m in zip(tbs, msgs)])
    for k in ns:
        res = {}

        def hand():
            sel = ctx.velo_fov_select(frames[:k])
            livox = np.concatenate([np.stack([m["x"], m["y"], m["z"]], 1) for m in msgs]).astype(np.float32)   # the caller's second copy
            vo = sel["offsets"]
            out = ctx.time_offset_search_batch([sel["xyz"][vo[i]:vo[i + 1]] for i in range(k)], [livox] * k, RES, SLICED)
            res["rows"] = [dict(r, n_kept=int(sel["n_kept"][i]), n_windows=len(r["window_error"]),
                                optim_start=int(offs[r["best_window"] * RES]) if r["best_window"] >= 0 else 0) for i, r in enumerate(out)]

        def stream():
            res["rows"] = ctx.time_offset_estimate_stream(st, 0, MSGS * MSG_PTS, frames[:k], stamps[:k], None, RES, SLICED)

        r = dict(n=k, mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"), t=timed(ctx, hand if mode == "prev" else stream))
        rows = res["rows"]
        np.savez(os.path.join(tmp, "%s_%d.npz" % (mode, k)), nn=np.concatenate([x["nn_d2"] for x in rows]),
                 err=np.concatenate([x["window_error"] for x in rows]), low=np.array([x["lowest_error"] for x in rows]),
                 ints=np.array([[x["n_kept"], x["n_windows"], x["best_window"], x["optim_start"]] for x in rows], np.uint64))
        r["found"] = int(sum(x["best_window"] >= 0 for x in rows))
        print("PROBE " + json.dumps(r), flush=True)
    st.close()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_offset_stream_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker, a.tmp)
    ns = a.sizes or [1, 8]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    with tempfile.TemporaryDirectory() as tmp:
        prev = run_worker(a.prev, ns, "prev", tmp, a.limit)
        new = run_worker(None, ns, "new", tmp, a.limit)   # started only after the first succeeded
        same = []
        for rn in new:
            x, y = np.load(os.path.join(tmp, "prev_%d.npz" % rn["n"])), np.load(os.path.join(tmp, "new_%d.npz" % rn["n"]))
            same.append(all(x[k].tobytes() == y[k].tobytes() for k in ("nn", "err", "low", "ints")))
    f = lambda t: "%.2f [%.2f .. %.2f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["time-offset estimation of n Velodyne frames (28 800 points) against 192 000 stream points, resolution %d, %d sliced points;" % (RES, SLICED),
             "ms, median [p10 .. p90] of %d repetitions after a warm-up, host clock, the context synchronised at both ends" % REPS,
             "hand-composed (parent build): mml_velo_fov_select_batch + host merge + mml_time_offset_search_batch + the stamp on the host",
             "stream call (new build): one mml_time_offset_estimate_stream on the resident stream",
             "equal = n_kept, n_windows, best_window, lowest_error, optim_start, every window error and every distance hold the same bytes",
             "", "%4s %6s %28s %28s %8s %6s" % ("n", "found", "hand-composed ms", "stream call ms", "ratio", "equal")]
    for rp, rn, eq in zip(prev, new, same):
        lines.append("%4d %6d %28s %28s %8.2f %6s" % (rn["n"], rn["found"], f(rp["t"]), f(rn["t"]), rp["t"]["ms"] / rn["t"]["ms"], eq))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not all(same):
        sys.exit("FINDING: an output of the stream call differs from the hand-composed path's")


if __name__ == "__main__":
    main()
