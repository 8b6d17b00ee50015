"""The aligner's Velodyne FOV selection (unionLidarsAligner.cpp:437-490) for n frames of 28 800 points, three ways on this build:
    python tools/velo_fov_probe.py [--out <table>] [n ...]
  host:   mml_velo_fov_select_batch with a NULL context -- the reference's loop, csrc/velo_fov.h compiled for the host;
  numpy:  a vectorised restatement (numpy.arctan2 and the parallel resolution of halfPassed; its last bits are numpy's, not
          glibc's, so only its counts are compared, within 0.1 %);
  device: mml_velo_fov_select_batch with a context, the filling call alone (rows, counts and info into arrays sized beforehand),
          timed on the host clock with the context synchronised before and after.
Defaults: n = 1, 16, 64.  The device rows are compared with the host rows to the byte before anything is timed.  A warm-up, then
10 repetitions; median [p10 .. p90] milliseconds.  The table goes to profiles/velo_fov_probe.txt.  No speed is a pass criterion."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NV = 28800
PI = np.pi


def timed(fn, reps=10, warm=1):
    t = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return "%.2f [%.2f .. %.2f]" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90)), float(np.median(t))


def numpy_select(f):
    """One frame, vectorised: first-branch ori of every point, h = the first index that sets the flag, second branch after it."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        A = -np.arctan2(f[:, 1], f[:, 0])
        s = A[0]
        e = f32(np.float64(A[-1]) + 2 * PI)
        if np.float64(e - s) > 3 * PI:
            e = f32(np.float64(e) - 2 * PI)
        elif np.float64(e - s) < PI:
            e = f32(np.float64(e) + 2 * PI)
        a64 = A.astype(np.float64)
        o1 = np.where(a64 < np.float64(s) - PI / 2, (a64 + 2 * PI).astype(f32), np.where(a64 > np.float64(s) + PI * 3 / 2, (a64 - 2 * PI).astype(f32), A))
        sets = (o1 - s).astype(np.float64) > PI
        h = int(np.argmax(sets)) if sets.any() else len(A)
        b = (a64 + 2 * PI).astype(f32)
        b64 = b.astype(np.float64)
        o2 = np.where(b64 < np.float64(e) - PI * 3 / 2, (b64 + 2 * PI).astype(f32), np.where(b64 > np.float64(e) + PI / 2, (b64 - 2 * PI).astype(f32), b))
        ori = np.where(np.arange(len(A)) <= h, o1, o2)
        rel = (ori - s) / (e - s)
        o = ori.astype(np.float64)
        keep = ((o > -0.7608) & (o < 0.7158)) | ((o > -0.7608 + 2 * PI) & (o < 0.7158 + 2 * PI))
    return np.concatenate([f[keep, :3], rel[keep, None]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "velo_fov_probe.txt"))
    ap.add_argument("sizes", nargs="*", type=int)
    a = ap.parse_args()
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    sizes = a.sizes or [1, 16, 64]
    base = [synth.velo_scan(40 + k) for k in range(4)]
    assert all(len(b) == NV for b in base)
    ctx = M.Context(max_scans=1, max_velo_points=NV, max_livox_points=64)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    lines = ["velo_fov_probe: n frames of %d points, packed x, y, z, intensity; milliseconds, median [p10 .. p90] of 10" % NV,
             "device: %s" % (ctx.device_info(),),
             "%6s %10s | %24s | %24s | %24s | %s" % ("n", "kept", "host (NULL ctx)", "numpy restatement", "device", "host / device")]
    for n in sizes:
        frames = [np.roll(base[i % 4], 977 * i, axis=0) for i in range(n)]     # (the sweep starts somewhere else in every frame)
        data, bo, npts, step = M.velo_fov_pack(frames)
        host = M.velo_fov_select_raw(data, bo, npts, step)
        dev = M.velo_fov_select_raw(data, bo, npts, step, ctx=ctx)
        for k in ("xyzt", "xyz", "n_kept", "info"):
            assert dev[k].tobytes() == host[k].tobytes(), (n, k)
        total = len(host["xyzt"])
        counts = [len(numpy_select(f)) for f in frames]
        assert abs(sum(counts) - total) <= max(1e-3 * total, 2), (sum(counts), total)
        xyzt, xyz = np.zeros((total, 4), np.float32), np.zeros((total, 3), np.float32)
        kept, info = np.zeros(n, np.int32), np.zeros(n, M.VELO_FOV_INFO_DTYPE)

        def call(h):
            rc = M.lib().mml_velo_fov_select_batch(h, n, p(data), p(bo), p(npts), step, 0, 4, 8, p(xyzt), p(xyz), total, p(kept), p(info))
            assert rc == M.MML_OK, rc

        def device():
            ctx.synchronize()
            call(ctx._h)
            ctx.synchronize()

        th, mh = timed(lambda: call(None))
        tn, _ = timed(lambda: [numpy_select(f) for f in frames])
        td, md = timed(device)
        assert xyzt.tobytes() == host["xyzt"].tobytes()
        lines.append("%6d %10d | %24s | %24s | %24s | %.2f" % (n, total, th, tn, td, mh / md))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
