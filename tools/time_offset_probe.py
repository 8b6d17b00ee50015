"""The aligner's time-offset search on n cloud pairs: n sequential mml_time_offset_search calls on a build of the PARENT commit
against one mml_time_offset_search_batch call of this build.
    python tools/time_offset_probe.py [--prev <parent .so>] [--out <table>] [n ...]
Defaults: n = 1, 8, 64, 256 problems of about 20 k Velodyne and 190 k Livox points, search_resolution 30, 12 000 sliced points
(5 934 windows per problem), every problem with its own transform.

The single calls run on a build of the parent commit ($MML_LIB_PATH, as tools/gicp_refresh_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
from a tight ctypes loop, in a process of their own; the new build runs the same problems through one batch call in a second
process.  Each process opens the device and runs under a time limit of its own, the second only after the first succeeded.
Every output of the two runs is compared: n_windows, best_window, lowest_error, all window errors, all nearest-neighbour
distances (those through a SHA-256 of their bytes).

Inputs: BASE distinct synthetic pairs -- a VLP-16 scan thinned to 20 000 points, eight Livox scans merged to 192 000 --, each
reused turned about z by a multiple of 1.5 mrad, so no two problems hold the same points.  Times are host clock around the
C-ABI calls, which include the upload of the clouds and end in a stream synchronise.  Per size: a warm-up, then 20 repetitions
(5 from n = 64 on); median and the 10th / 90th percentile."""
import argparse
import ctypes as C
import hashlib
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
BASE = 2           # distinct synthetic cloud pairs
RES, SLICED = 30, 12000


def timed(fn, reps, warm=1):
    t = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def make_base(path):
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    out = {}
    for k in range(BASE):
        v = synth.velo_scan(40 + k)[:, :3]
        out["v%d" % k] = np.ascontiguousarray(v[np.arange(len(v)) % 36 < 25][:20000])
        parts = [synth.livox_scan(40 + 8 * k + j, motion=True) for j in range(8)]
        out["l%d" % k] = np.concatenate([np.stack([p["x"], p["y"], p["z"]], 1) for p in parts]).astype(np.float32)
    np.savez(path, **out)


def problems(path, n):
    """n distinct (velo, livox, tf): base pair s % BASE turned about z by 1.5 mrad x (s // BASE)."""
    base = np.load(path)
    vs, ls, tfs = [], [], []
    for s in range(n):
        v, l = base["v%d" % (s % BASE)], base["l%d" % (s % BASE)]
        a = 1.5e-3 * (s // BASE)
        if a != 0.0:
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
            v, l = v @ R.T, l @ R.T
        th = 0.01 + 1e-4 * s
        tfs.append(np.array([[np.cos(th), -np.sin(th), 0, 0.05], [np.sin(th), np.cos(th), 0, -0.1], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float32))
        vs.append(np.ascontiguousarray(v, np.float32))
        ls.append(np.ascontiguousarray(l, np.float32))
    return vs, ls, np.stack(tfs)


def worker(ns, mode, tmp):
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    at = lambda a, i: C.c_void_p(a.ctypes.data + a.strides[0] * int(i))
    ctx = M.Context(max_scans=1)
    vs, ls, tfs = problems(os.path.join(tmp, "base.npz"), max(ns))
    for k in ns:
        nv, nl = [len(v) for v in vs[:k]], [len(l) for l in ls[:k]]
        vo = np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)
        lo = np.concatenate([[0], np.cumsum(nl)]).astype(np.int32)
        nwin = [(m - SLICED - 1) // RES + 1 if m > SLICED else 0 for m in nl]
        wo = np.concatenate([[0], np.cumsum(nwin)]).astype(np.int64)
        velo, livox = np.ascontiguousarray(np.concatenate(vs[:k])), np.ascontiguousarray(np.concatenate(ls[:k]))
        tf = np.ascontiguousarray(tfs[:k].reshape(k, 16))
        nn, err = np.zeros(len(livox), np.float32), np.zeros(int(wo[-1]))
        nw, best, low = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k)

        def single():
            for i in range(k):
                rc = L.mml_time_offset_search(ctx._h, at(velo, vo[i]), nv[i], at(tf, i), at(livox, lo[i]), nl[i], RES, SLICED, at(nn, lo[i]),
                                              at(err, wo[i]), nwin[i], at(nw, i), at(best, i), at(low, i))
                if rc != 0:
                    raise RuntimeError(L.mml_last_error(ctx._h).decode())

        def batch():
            rc = L.mml_time_offset_search_batch(ctx._h, k, p(velo), p(vo), p(tf), p(livox), p(lo), RES, SLICED, p(nn), p(err), p(wo), p(nw), p(best),
                                                p(low))
            if rc != 0:
                raise RuntimeError(L.mml_last_error(ctx._h).decode())

        r = dict(n=k, mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"), n_velo=int(np.mean(nv)), n_livox=int(np.mean(nl)))
        r["t"] = timed(single if mode == "prev" else batch, 20 if k < 64 else 5)
        r["nn_sha256"] = hashlib.sha256(nn.tobytes()).hexdigest()
        r["found"] = int((best >= 0).sum())
        np.savez(os.path.join(tmp, "%s_%d.npz" % (mode, k)), err=err, nw=nw, best=best, low=low)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_offset_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds each device process may take")
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker, a.tmp)
    ns = a.sizes or [1, 8, 64, 256]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    with tempfile.TemporaryDirectory() as tmp:
        make_base(os.path.join(tmp, "base.npz"))
        prev = run_worker(a.prev, ns, "prev", tmp, a.limit)
        new = run_worker(None, ns, "new", tmp, a.limit)   # started only after the first succeeded
        same = []
        for rp, rn in zip(prev, new):
            x, y = np.load(os.path.join(tmp, "prev_%d.npz" % rn["n"])), np.load(os.path.join(tmp, "new_%d.npz" % rn["n"]))
            same.append(rp["nn_sha256"] == rn["nn_sha256"] and all(x[k].tobytes() == y[k].tobytes() for k in ("err", "nw", "best", "low")))
    f = lambda t: "%.2f [%.2f .. %.2f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["time-offset search on n cloud pairs (%d Velodyne, %d Livox points each, distinct), resolution %d, %d sliced points, a transform per problem;"
             % (new[0]["n_velo"], new[0]["n_livox"], RES, SLICED),
             "ms, median [p10 .. p90] of 20 repetitions (5 from n = 64 on), host clock around the C-ABI calls (upload and read-back included)",
             "single calls (parent build): n mml_time_offset_search calls; batch call (new build): one mml_time_offset_search_batch",
             "found = problems with a best window; equal = n_windows, best_window, lowest_error, every window error and every distance hold the same bytes",
             "",
             "%6s %8s %28s %28s %14s %14s %10s %6s" % ("n", "found", "single calls ms", "batch call ms", "single ms/prob", "batch ms/prob", "speed-up",
                                                    "equal")]
    ok = True
    wins = None
    for rp, rn, eq in zip(prev, new, same):
        n = rn["n"]
        s, b = rp["t"]["ms"], rn["t"]["ms"]
        lines.append("%6d %8d %28s %28s %14.3f %14.3f %10.2f %6s" % (n, rn["found"], f(rp["t"]), f(rn["t"]), s / n, b / n, s / b, eq))
        ok &= eq
        if b < s and wins is None:
            wins = n
        if b >= s:
            wins = None
    lines += ["", "break-even: the batch call is faster than the single calls from n = %s on (of the sizes measured)" % wins if wins is not None else
              "break-even: none -- the batch call is not faster than the single calls at the largest n measured"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: an output of the batch call differs from the single calls'")


if __name__ == "__main__":
    main()
