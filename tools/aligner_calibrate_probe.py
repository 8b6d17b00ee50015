"""The aligner's start-up calibration on one integrated Livox frame and one Velodyne frame: the host route a user has without
mml_aligner_calibrate, on a build of the PARENT commit, against the one device call of this build.
    python tools/aligner_calibrate_probe.py [--prev <parent .so>] [--out <table>] [--reps n]

Host route (parent build, $MML_LIB_PATH as tools/gicp_refresh_probe.py does):
    make -C multi-modal-loam_amd/csrc BUILD=build_prev OUT=../libmmloam_hip_prev.so      (at the parent commit)
numpy crop at 50 m, a numpy restatement of the CPU voxel filter (PCL's voxel index, stable sort, float32 means; the tools do not
load the test oracle) with leaf 0.05 on both clouds, then mml_gicp_align -- ten outer iterations, epsilon 1e-6, no
correspondence gate: the only settings the parent has.  Device call (this build): mml_aligner_calibrate --
crop, voxel filter and the GICP with {500, 1e-3, 2 m} on the device.  The two routes do not run the same settings, so their
matrices are compared, not expected to be equal; both are also compared with the motion the pair was built with.  Each route
runs in a process of its own under a time limit of its own, the second only after the first succeeded.

Inputs: synth.livox_scan(14) (24 000 points, intensity = reflectivity) moved by a known small motion, and synth.velo_scan(14)
(28 800 points); both see the same room from the same pose, so the motion is the extrinsic to find.  Times are host clock
around the calls, which end synchronised; a warm-up, then --reps repetitions; median and the 10th / 90th percentile."""
import argparse
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
FAR, LEAF = 50.0, 0.05
EULER, TRANS = (0.004, -0.006, 0.008), (0.05, -0.03, 0.02)


def clouds():
    """(hori n x 4, velo n x 4, R, t) with Velodyne-frame point = R hori + t."""
    from scipy.spatial.transform import Rotation as Rsc
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    l = synth.livox_scan(14)
    v = synth.velo_scan(14)
    R, t = Rsc.from_euler("xyz", EULER).as_matrix(), np.array(TRANS)
    xyz = np.stack([l["x"], l["y"], l["z"]], 1).astype(np.float64)
    h = np.concatenate([(xyz - t) @ R, l["reflectivity"].astype(np.float64)[:, None]], axis=1).astype(np.float32)
    return h, v, R, t


def errors(T, R, t):
    from scipy.spatial.transform import Rotation as Rsc
    T = np.asarray(T, np.float64)
    return float(np.linalg.norm(T[:3, 3] - t)), float(np.linalg.norm(Rsc.from_matrix(T[:3, :3] @ R.T).as_rotvec()))


def timed(fn, reps, warm=1):
    ts, out = [], None
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        out = fn()
        if rep >= warm:
            ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return dict(ms=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)), reps=len(ts)), out


def crop(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return p[~((x * x + y * y) + z * z > np.float32(FAR) * np.float32(FAR))]


def voxel(xyz, leaf):
    """pcl::VoxelGrid on the host: voxel index i + j dx + k dx dy on the floor of the bounding box, stable sort, float32 means."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    min_b = np.floor(xyz.min(0) * inv).astype(np.int64)
    div = np.floor(xyz.max(0) * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(xyz * inv) - min_b.astype(np.float32)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    heads = np.flatnonzero(np.concatenate([[True], idx[order][1:] != idx[order][:-1]]))
    cnt = np.diff(np.concatenate([heads, [len(idx)]])).astype(np.float32)
    return (np.add.reduceat(xyz[order], heads, axis=0) / cnt[:, None]).astype(np.float32)


def worker(mode, tmp, reps):
    M = importlib.import_module("multi-modal-loam_amd")
    h, v, R, t = clouds()
    ctx = M.Context(max_scans=1)
    r = dict(mode=mode, lib=os.environ.get("MML_LIB_PATH", "default"), n_hori=len(h), n_velo=len(v))
    if mode == "prev":
        filt = lambda: (voxel(crop(h)[:, :3], LEAF), voxel(crop(v)[:, :3], LEAF))
        r["t_filter"], (hd, vd) = timed(filt, reps)
        r["t_gicp"], (ok, T, info) = timed(lambda: ctx.gicp_align(hd, vd), reps)
        r["t"], _ = timed(lambda: ctx.gicp_align(*filt()), reps)
        r.update(n_hori_ds=len(hd), n_velo_ds=len(vd))
    else:
        r["t_filter"], ((hd, _), (vd, _)) = timed(lambda: (ctx.cloud_crop_voxel(h, FAR, LEAF), ctx.cloud_crop_voxel(v, FAR, LEAF)), reps)
        r["t_gicp"], _ = timed(lambda: ctx.gicp_align_opts(hd[:, :3], vd[:, :3], 500, 1e-3, 2.0), reps)
        r["t"], (ok, T, _, ci) = timed(lambda: ctx.aligner_calibrate(h, v), reps)
        info = ci.gicp
        r.update(n_hori_ds=ci.n_hori_ds, n_velo_ds=ci.n_velo_ds, unfiltered=(ci.hori_unfiltered, ci.velo_unfiltered))
    ctx.close()
    r.update(converged=bool(ok), outer=info.outer_iterations, evals=info.objective_evaluations, objective=info.objective, err=errors(T, R, t))
    np.save(os.path.join(tmp, mode + ".npy"), np.asarray(T, np.float32))
    print("PROBE " + json.dumps(r), flush=True)


def run_worker(lib, mode, tmp, reps, limit):
    env = dict(os.environ)
    if lib:
        env["MML_LIB_PATH"] = lib
    else:
        env.pop("MML_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--tmp", tmp, "--reps", str(reps)], env=env,
                         capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise RuntimeError("worker failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    return [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("PROBE ")][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", default=os.path.join(ROOT, "multi-modal-loam_amd", "libmmloam_hip_prev.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_calibrate_probe.txt"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each device process may take")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.tmp, a.reps)
    if not os.path.exists(a.prev):
        sys.exit("no parent build at %s (see the module docstring)" % a.prev)
    with tempfile.TemporaryDirectory() as tmp:
        prev = run_worker(a.prev, "prev", tmp, a.reps, a.limit)
        new = run_worker(None, "new", tmp, a.reps, a.limit)   # started only after the first succeeded
        dT = float(np.abs(np.load(os.path.join(tmp, "prev.npy")) - np.load(os.path.join(tmp, "new.npy"))).max())
    f = lambda t: "%.2f [%.2f .. %.2f]" % (t["ms"], t["p10"], t["p90"])
    lines = ["the aligner's start-up calibration: one Livox frame of %d points onto one Velodyne frame of %d points" % (new["n_hori"], new["n_velo"]),
             "ms, median [p10 .. p90] of %d repetitions after a warm-up, host clock around calls that end synchronised" % new["t"]["reps"],
             "host route (parent build): numpy crop 50 m + numpy voxel filter 0.05 on the CPU, then mml_gicp_align {10, 1e-6, no gate}",
             "device call (this build):  mml_aligner_calibrate = crop + voxel filter + GICP {500, 1e-3, 2 m} on the device",
             "filter / gicp: the two stages timed on their own (device: mml_cloud_crop_voxel x 2, mml_gicp_align_opts)",
             "",
             "%-12s %9s %9s %10s %6s %6s %24s %24s %24s %12s %12s" % ("route", "hori kept", "velo kept", "converged", "outer", "evals", "whole ms", "filter ms",
                                                                     "gicp ms", "t error m", "rot error rad")]
    for name, r in (("host route", prev), ("device call", new)):
        lines.append("%-12s %9d %9d %10s %6d %6d %24s %24s %24s %12.3g %12.3g" % (name, r["n_hori_ds"], r["n_velo_ds"], r["converged"], r["outer"],
                                                                              r["evals"], f(r["t"]), f(r["t_filter"]), f(r["t_gicp"]),
                                                                              r["err"][0], r["err"][1]))
    lines += ["", "max |hori_tf(device call) - T(host route)| = %.3g   (different settings: not expected to be equal)" % dT,
              "device call / host route, whole: %.2f" % (new["t"]["ms"] / prev["t"]["ms"])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
