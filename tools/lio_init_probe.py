"""Initialising n segments: n mml_lio_initialize calls (the parent commit's host routine) against the host loop and the device
call of mml_lio_initialize_batch.
    python tools/lio_init_probe.py [--prev <parent .so>] [--out <table>] [n_seg ...]
Defaults: n_seg = 1, 16, 64, 300, 1024 segments of 3 and of 8 frames, 20 IMU messages per frame at 200 Hz.

The single calls run on a build of the PARENT commit ($MML_LIB_PATH, as tools/imu_preintegrate_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
from a tight ctypes loop, one call per segment, in a process of their own.  The new build runs the same segments through
mml_lio_initialize_batch with a NULL context (the host loop of csrc/lio_init_core.h) and with a context (one upload, three
launches, one read-back), and compares every output byte of the two.  The process that opens the device runs under a time
limit of its own, after the one that does not; a failure of either ends the probe.

Inputs: a smooth motion (constant body rate and world acceleration) in a world whose gravity is tilted, a tilt, a bias pair and
an extrinsic per segment, from a fixed seed.  The state arrays are in/out, so every repetition starts from a copy of the
inputs (inside the clock: a memcpy of 16 doubles per frame).  Times are host clock around the C-ABI calls -- the device call
ends in a stream synchronise -- with the arguments marshalled before the clock starts.  Per size: a warm-up, then at least 20
repetitions; median and the 10th / 90th percentile."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
from scipy.spatial.transform import Rotation as Rsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = (3, 8)
PER, H, GN = 20, 0.005, 9.805
KEYS = ("P", "Q", "V", "bg", "ba")


def timed(fn, min_reps=20, warm=2):
    for _ in range(warm):
        fn()
    t = []
    while len(t) < min_reps:
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), reps=len(t))


def segments(n_seg, n, seed):
    """The concatenated arguments of n_seg segments of n frames."""
    rng = np.random.default_rng(seed)
    F = n_seg * n
    a = dict(t=np.zeros(F), P=np.zeros((F, 3)), Q=np.zeros((F, 4)), V=np.zeros((F, 3)), bg=np.zeros((F, 3)), ba=np.zeros((F, 3)),
             smp=np.zeros((F * PER, 7)), ex=np.zeros((n_seg, 16)))
    w_body, a_world = np.array([0.05, -0.03, 0.2]), np.array([0.3, -0.2, 0.05])
    P0, V0, R0 = np.array([1.0, 2.0, 0.5]), np.array([0.5, 0.1, -0.05]), Rsc.from_rotvec([0.0, 0.0, 0.3])
    T = PER * H
    ts = (T * np.arange(n)[:, None] + H * np.arange(PER)[None, :]).reshape(-1)     # sample k of frame f holds from T f + k H
    tf = T * (np.arange(n) + 1.0)
    for s in range(n_seg):
        gw = Rsc.from_rotvec(rng.normal(0, 0.04, 3) * [1, 1, 0]).as_matrix() @ np.array([0.0, 0.0, -GN])
        bg, ba = rng.normal(0, 0.003, 3), rng.normal(0, 0.03, 3)
        ex = np.eye(4)
        ex[:3, :3] = Rsc.from_rotvec(rng.normal(0, 0.03, 3)).as_matrix()
        ex[:3, 3] = rng.normal(0, 0.08, 3)
        Rk = (R0 * Rsc.from_rotvec(w_body[None, :] * ts[:, None])).as_matrix()
        acc = (np.einsum("kji,j->ki", Rk, a_world - gw) + ba) / GN
        f0 = s * n
        a["smp"][f0 * PER:(f0 + n) * PER] = np.concatenate([np.tile(w_body + bg, (n * PER, 1)), acc, np.full((n * PER, 1), H)], axis=1)
        Rf = (R0 * Rsc.from_rotvec(w_body[None, :] * tf[:, None])).as_matrix()
        Pf = P0 + V0 * tf[:, None] + 0.5 * a_world * tf[:, None] ** 2
        exi = np.linalg.inv(ex)
        Rl = Rf @ exi[:3, :3]
        a["t"][f0:f0 + n] = tf
        a["P"][f0:f0 + n] = Pf + Rf @ exi[:3, 3]
        a["Q"][f0:f0 + n] = Rsc.from_matrix(Rl).as_quat()
        a["ex"][s] = ex.reshape(16)
    a["fo"] = (n * np.arange(n_seg + 1)).astype(np.int32)
    a["so"] = (PER * np.arange(F + 1)).astype(np.int32)
    return a


def worker(ns, mode):
    M = importlib.import_module("multi-modal-loam_amd")
    L = M.lib()
    ctx = M.Context(max_scans=1) if mode == "new" else None
    nmax = max(ns)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for n in FRAMES:
        a = segments(nmax, n, 200 + n)
        st = {k: a[k].copy() for k in KEYS}
        out = (M.LioInitResult * nmax)()
        pre = (M.ImuPreint * (nmax * n))()
        off1 = (PER * np.arange(n + 1)).astype(np.int32)

        def reset(k):
            for key in KEYS:
                st[key][:k * n] = a[key][:k * n]

        at = lambda arr, row, width: C.c_void_p(arr.ctypes.data + 8 * width * row)
        single_args = [(C.c_int(n), at(a["t"], s * n, 1), at(st["P"], s * n, 3), at(st["Q"], s * n, 4), at(st["V"], s * n, 3),
                        at(st["bg"], s * n, 3), at(st["ba"], s * n, 3), at(a["smp"], s * n * PER, 7), p(off1), at(a["ex"], s, 16), None,
                        C.byref(pre, C.sizeof(M.ImuPreint) * s * n), C.byref(out[s])) for s in range(nmax)]

        def single(k):
            reset(k)
            for s in range(k):
                if L.mml_lio_initialize(*single_args[s]) != 0:
                    raise RuntimeError("mml_lio_initialize failed")

        def batch(k, h):
            reset(k)
            if L.mml_lio_initialize_batch(h, k, p(a["fo"]), p(a["t"]), p(st["P"]), p(st["Q"]), p(st["V"]), p(st["bg"]), p(st["ba"]), p(a["smp"]),
                                          p(a["so"]), p(a["ex"]), None, pre, out) != 0:
                raise RuntimeError(L.mml_last_error(h).decode() if h else "mml_lio_initialize_batch failed")

        def everything(k):
            return b"".join(st[key][:k * n].tobytes() for key in KEYS) + bytes(out)[:C.sizeof(M.LioInitResult) * k] + \
                bytes(pre)[:C.sizeof(M.ImuPreint) * k * n]

        for k in ns:
            r = dict(n_seg=k, frames=n, lib=os.environ.get("MML_LIB_PATH", "default"))
            if mode == "prev":
                r["single"] = timed(lambda: single(k))
            else:
                C.memset(pre, 0, C.sizeof(pre))                  # (entry 0 of a segment is never written)
                r["host"] = timed(lambda: batch(k, None))
                ref = everything(k)
                r["device"] = timed(lambda: batch(k, ctx._h))
                r["equal"] = everything(k) == ref
            r["ok"] = int(sum(out[s].status == 0 for s in range(k)))
            print("PROBE " + json.dumps(r), flush=True)
    if ctx is not None:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lio_init_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    if a.worker:
        return worker(a.sizes, a.worker)
    ns = a.sizes or [1, 16, 64, 300, 1024]
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    prev = run_worker(a.prev, ns, "prev", 400)      # host code only
    new = run_worker(None, ns, "new", 500)          # opens the device: its own limit, started only after the first succeeded
    f = lambda t: "%.3f [%.3f .. %.3f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["initialising n_seg segments of `frames` frames, %d IMU messages per frame; ms, median [p10 .. p90] of >= 20 repetitions" % PER,
             "single calls (parent build): n_seg mml_lio_initialize calls; host loop / device call (new build):",
             "mml_lio_initialize_batch with a NULL context / with a context; ok = segments with status 0",
             "",
             "%6s %6s %5s %28s %28s %28s %11s %11s %11s %9s %6s" % ("frames", "n_seg", "ok", "single calls ms", "host loop ms", "device call ms",
                                                                  "single us/s", "host us/s", "dev us/s", "speed-up", "equal")]
    ok = True
    for rp, rn in zip(prev, new):
        n = rn["n_seg"]
        s, h, d = rp["single"]["ms"], rn["host"]["ms"], rn["device"]["ms"]
        lines.append("%6d %6d %5d %28s %28s %28s %11.1f %11.1f %11.1f %9.2f %6s" % (rn["frames"], n, rn["ok"], f(rp["single"]), f(rn["host"]),
                                                                              f(rn["device"]), 1e3 * s / n, 1e3 * h / n, 1e3 * d / n, s / d, rn["equal"]))
        ok &= rn["equal"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    if not ok:
        sys.exit("FINDING: a device initialisation differs from the host build's")


if __name__ == "__main__":
    main()
