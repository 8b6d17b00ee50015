#!/usr/bin/env python3
"""bench.py -- scans/s of the mm-loam scan-registration hot path on MI355X.

Default workload (BASELINE.json configs[1], the configuration the metric is quoted on): fused VLP-16 (16 x 1800) + Livox
Horizon (24 000) scans = 52 800 points, local map of 200 000 points; one STEP = feature extraction + undistortion +
down-sampling + one 5-NN association pass + 10 trust-region (GN / dogleg) iterations for a batch of scans whose raw
points are already resident in HBM.  value = whole-job scans/s.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 1|2|3|4] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps, writes its outputs (--dump-outputs) and prints the JSON line: metric, value,
ms_per_step (one timed step), config.  Everything else it can measure or check is behind --full (see "Added to the JSON line").

  --dump-outputs DIR  after the timed steps: what the timed path computed in its last step, as DIR/<name>.npy (float32 /
              float64, at most 64 MB in all; ranks r > 0 add _rank<r> to the name).  The inputs are seeded: the same
              arguments give the same inputs on every run, so two builds can be compared output for output.
              configs 1, 3, 4: poses (slots x 6: translation | rotation vector, what mml_step returned for every resident
              slot), corner_features / surf_features (the down-sampled stacks of the first distinct slots, concatenated)
              and feature_counts (corner, surf per dumped slot); config 2: poses (scans x 4 x 4) of the last replay pass
  --config 1  BASELINE configs[1] (default; the driver's line)
  --config 2  BASELINE configs[2]: replay, one scan at a time through the WHOLE odometry loop (upload, extract, undistort,
              down-sample, Estimate 5 outer x 10 inner, key-scan rule + map upkeep on the device) plus the joint solve of
              the 8-scan sliding window; value = sustained scans/s next to the 10 Hz bag rate, with per-scan latency
              percentiles and the B = 1 latency of the configs[1] step
  --config 3  BASELINE configs[3]: 128 x 2048 scans (262 144 points), 2 M-point map, 10 GN iterations
  --config 4  BASELINE configs[4]: 240 k-point fused scans, 10 M-point map, 20 GN iterations

One process per GPU.  `--gpus N` with N > 1 spawns the N ranks itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*) unless
a launcher (python -m torch.distributed.run ...) already did; torch.distributed (RCCL) carries the barrier and the
max-over-ranks clock.  The path shards by scan with no data-path collective ("scaling": "weak"); the one real exchange of
the path -- the joint window solve -- runs through the C-ABI's own RCCL calls (mml_window_solve_allgather) and is
reported in "window_solve".

Added to the JSON line with --full (configs 1, 3, 4: replica check of the timed region's slots, value_by_slots,
value_with_upload, window_solve, rccl; config 2: the B = 1 step latency, full_window_imu, the C++ adapter leg):
  roofline     -- dominant kernel: algorithmic bytes per launch / its mean launch time (HIP events on the library's own
                  stream around every launch of a single-stream pass) against 8 TB/s HBM
  cpu_baseline -- oracle/bench_cpu (the CPU restatement, pure C++, -O3 -ffp-contract=off; the reference binary cannot be
                  built here) on this box's host cores over a bounded sample of the same scans: single thread, the
                  reference's own threading, and one scan per core
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6.3 TB/s achievable
BAG_RATE_HZ = 10.0      # mm_lio_full.launch:21 (10 Hz Velodyne, one union message per sweep)
VALU_CLOCK_HZ = 2.4e9   # MI355X peak engine clock (MI355X_MICROARCH.md): the VALU issue peak is CUs x 4 SIMDs x clock / 4

# Algorithmic bytes per unit for every stage (DESIGN.md section "Kernels"): N fused points, F features per scan.
# The SURVEY 8(d) figures: extraction 20 B/pt in total, undistort 28 B/pt, association 112 B/feature,
# linearisation 72 B/factor/iteration.  The extraction chain is split over its kernels by what each must move.
STAGE_BYTES = {
    "assign_count":     lambda n_v, n_l, nf, it: 16 * n_v + 20 * n_l,  # k_assign_a: read the raw records, ring id / crop test
    "assign_scan":      lambda n_v, n_l, nf, it: 0,                    # k_assign_b: block records only
    "assign_scatter":   lambda n_v, n_l, nf, it: 16 * n_v + 20 * n_l + 20 * (n_v + n_l),  # k_assign_c: read again, write xyzi + label slot
    # one-pass bucketing (ring layouts up to 32 rings): every raw record read once, the bucketed point (16 B) and its (fused index,
    # in-sweep time) record (8 B) written once
    "assign_ends":      lambda n_v, n_l, nf, it: 0,
    "assign_onepass":   lambda n_v, n_l, nf, it: 16 * n_v + 20 * n_l + 24 * (n_v + n_l),
    "assign_tables":    lambda n_v, n_l, nf, it: 0,
    "stencil":          lambda n_v, n_l, nf, it: 16 * (n_v + n_l),     # read xyzi of every bucketed point
    "select":           lambda n_v, n_l, nf, it: 11 * (n_v + n_l),     # attr 2 B + 2 order keys 8 B + label 1 B (+ 4 B per labelled point)
    "crop_compact":     lambda n_v, n_l, nf, it: 4 * (n_v + n_l),      # (k_crop: behind mml_cloud_upload only since round 5)
    "undistort":        lambda n_v, n_l, nf, it: 28 * (n_v + n_l),
    # list entry 4 B + point 16 B + fused index 4 B per labelled point (~7 % of the points: taken as 0.07 N) + 16 B per feature out
    "voxel_downsample": lambda n_v, n_l, nf, it: 24 * 0.07 * (n_v + n_l) + 16 * nf,
    "associate":        lambda n_v, n_l, nf, it: 112 * nf,
    "associate_far":    lambda n_v, n_l, nf, it: 0,                    # queue of the few far queries (bytes counted in associate)
    "associate_fit":    lambda n_v, n_l, nf, it: 0,                    # model fit of the searched features (bytes counted in associate)
    "assoc_stats":      lambda n_v, n_l, nf, it: 0,
    "solve":            lambda n_v, n_l, nf, it: 72 * nf * (it + 1),   # it iterations + the initial linearisation
}

# BASELINE.json configs[i] -> shapes.  slots = resident scan slots per GPU; scans_per_step = the batch one step processes
# (the resident slots are passed over scans_per_step / slots times: every pass recomputes everything from the raw points).
# The slots are sized for the 288 GB of the device (61 GB at configs[1], ~180 GB at the dense layouts): one mml_step call per pass,
# i.e. one host synchronisation and one ramp-up / drain of the two stream lanes per 8192 (4096) scans -- 2048 / 1024 / 512 slots
# measured 345 k / 71.0 k / 66.7 k scans/s where these sizes give 353 k / 75.6 k / 76.7 k on the same boxes.
CONFIGS = {
    1: dict(name="BASELINE configs[1]: fused VLP-16 16x1800 + Livox Horizon 24000 scan (52800 pts)", n_rings=16, n_az=1800,
            pitch0=-15.0, pitch_step=2.0, livox=24000, map_points=200000, gn_iters=10, slots=8192, scans_per_step=32768,
            max_features=0, distinct=64),
    3: dict(name="BASELINE configs[3]: 128-ring x 2048 dense scan (262144 pts)", n_rings=128, n_az=2048, pitch0=-25.0,
            pitch_step=40.0 / 127.0, livox=0, map_points=2000000, gn_iters=10, slots=4096, scans_per_step=8192,
            max_features=1 << 16, distinct=8),
    4: dict(name="BASELINE configs[4]: 240k-pt fused scan (128 x 1687 + Livox 24000)", n_rings=128, n_az=1687, pitch0=-25.0,
            pitch_step=40.0 / 127.0, livox=24000, map_points=10000000, gn_iters=20, slots=4096, scans_per_step=8192,
            max_features=1 << 16, distinct=8),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3, 4], help="index into BASELINE.json configs")
    ap.add_argument("--full", action="store_true", help="every section besides the headline: checks, roofline, CPU baseline, "
                    "other batch sizes, uploads, window solve (the options below that tune a section act only with --full)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last step "
                    "to DIR/<name>.npy")
    ap.add_argument("--slots", type=int, default=0, help="resident scan slots per GPU (0: the config's default)")
    ap.add_argument("--batch", type=int, default=0, help="scans per step per GPU (0: the config's default; rounded up to whole passes over the slots)")
    ap.add_argument("--map-points", type=int, default=0)
    ap.add_argument("--gn-iters", type=int, default=0)
    ap.add_argument("--distinct", type=int, default=0, help="distinct synthetic scans cycled through the slots")
    ap.add_argument("--no-spread", action="store_true", help="keep every scan on the map's original tile (the round-1 layout)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed even with one rank (exercises the N > 1 code path)")
    ap.add_argument("--window-demo", action="store_true", help="run the C-ABI / RCCL joint window solve section on one GPU as well")
    ap.add_argument("--kernel-steps", type=int, default=4, help="single-stream steps after the timed region (per-kernel timing)")
    ap.add_argument("--cpu-seconds", type=float, default=6.0, help="time budget of each CPU-baseline variant (0: skip the CPU leg)")
    ap.add_argument("--cell-corner", type=float, default=0.0, help="kNN grid cell edge for the corner map (0: library default)")
    ap.add_argument("--cell-surf", type=float, default=0.0, help="kNN grid cell edge for the surf map (0: library default)")
    ap.add_argument("--replay-scans", type=int, default=240, help="--config 2: scans replayed through the odometry loop")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (gloo: CPU plumbing test only)")
    ap.add_argument("--skip-cpp-loop", action="store_true", help="--config 2: skip the C++ adapter leg (tools/live_loop.cpp)")
    ap.add_argument("--skip-by-slots", action="store_true", help="skip the value_by_slots section (counter passes: only launches of one size)")
    ap.add_argument("--skip-upload", action="store_true", help="skip the PCIe-inclusive section (counter passes: only launches of one size)")
    ap.add_argument("--stub-step", action="store_true", help="CPU plumbing test: no device, a step is a short sleep")
    ap.add_argument("--strict", action="store_true", help="exit non-zero when any section of the run reported an error (the JSON line's "
                    "\"errors\" list is not empty); tools/profile_round.sh passes it")
    return ap.parse_args()


# ---- launcher ---------------------------------------------------------------------------------------------------------
def spawn_ranks(args):
    """`bench.py --gpus N` started bare: become the launcher of N ranks on this node (one process per GPU)."""
    n = args.gpus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):  # one rank died: do not leave the others in a collective
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
            rc = rc or (p.returncode or 0)
    return rc


def pctl(a, q):
    return float(np.percentile(np.asarray(a, dtype=np.float64), q)) if len(a) else None


# ---- CPU plumbing test (tests/test_host.py): the launcher, the rendezvous, the max-over-ranks clock, the JSON line ----
def run_stub(args, rank, world, dist):
    import torch
    B = args.batch or 64

    def barrier():
        if dist is not None:
            dist.barrier()

    for _ in range(args.warmup):
        time.sleep(0.001)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))  # ranks deliberately unequal: the slowest one sets the clock
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        print(json.dumps({"metric": "scans/s (stub step, CPU plumbing test)", "value": world * B * args.steps / elapsed,
                          "unit": "scans/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "none", "data": "none", "config": {"workload": "stub"}}), flush=True)


# ---- workload ---------------------------------------------------------------------------------------------------------
def lib_sha16(M):
    """First 16 hex digits of the sha256 of the loaded libmmloam_hip.so: the PMC summaries under profiles/ carry the hash of the
    build they were counted on (tools/profile_round.sh), so that a count from another build is reported as stale."""
    import hashlib
    try:
        path = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "libmmloam_hip.so")
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    except Exception:
        return None


def rccl_report(M):
    """Which RCCL the process runs on: every librccl mapped (there must be ONE: the package maps PyTorch's copy before its own
    library asks for `librccl.so.1`, see multi-modal-loam_amd/__init__.py), the version behind the C-ABI's collectives and the
    version torch.distributed's "nccl" backend reports."""
    try:
        r = M.rccl_libraries()
        try:
            import torch
            tv = torch.cuda.nccl.version()
            r["torch_version"] = int(tv[0]) * 10000 + int(tv[1]) * 100 + int(tv[2]) if isinstance(tv, tuple) else int(tv)
        except Exception:
            r["torch_version"] = None
        r["single_copy"] = len(r["loaded"]) == 1
        return r
    except Exception as e:
        return {"error": repr(e)[:200]}


def replica_check(digests, x, keys):
    """Groups of slots with equal `keys` (same scan, same map tile, same initial pose) must have equal digest rows and equal
    poses.  Returns the JSON object of the bench line."""
    groups = {}
    for s, k in enumerate(keys):
        groups.setdefault(k, []).append(s)
    mism, examples, replicated = 0, [], 0
    for k, slots in groups.items():
        f = slots[0]
        replicated += len(slots) - 1
        for s in slots[1:]:
            bad = [int(w) for w in np.nonzero(digests[s] != digests[f])[0]]
            if bad or not np.array_equal(x[s], x[f]):
                mism += 1
                if len(examples) < 8:
                    examples.append({"slot": int(s), "first_slot_of_group": int(f), "digest_words": bad})
    out = {"slots": int(len(keys)), "groups": len(groups), "replica_slots_compared": int(replicated), "digest_words": int(digests.shape[1]),
           "mismatches": int(mism)}
    if examples:
        out["examples"] = examples
    return out


def make_scan(synth, cfg, k, motion=True):
    v = synth.velo_scan(k, n_rings=cfg["n_rings"], n_az=cfg["n_az"], pitch0=cfg["pitch0"], pitch_step=cfg["pitch_step"], motion=motion)
    l = synth.livox_scan(k, n=cfg["livox"], motion=motion) if cfg["livox"] else np.zeros(0, synth.LIVOX_DTYPE)
    return v, l


def make_context(M, cfg, slots, device, args, map_points):
    nv = cfg["n_rings"] * cfg["n_az"]
    kw = dict(max_scans=slots, max_velo_points=nv, max_livox_points=cfg["livox"], n_rings=cfg["n_rings"],
              pitch0_deg=cfg["pitch0"], pitch_step_deg=cfg["pitch_step"], max_map_points=max(int(map_points * 1.05), 1 << 16),
              cell_corner=args.cell_corner, cell_surf=args.cell_surf)
    if cfg["max_features"]:
        kw["max_features"] = cfg["max_features"]
    return M.Context(M.default_config(**kw), device=device)


def build_maps(ctx, synth, cfg, base, map_points):
    """Features of the 8 scans preceding the batch (the role of the 50-keyframe local map, Estimator.cpp:1585-1643),
    extracted with the product path itself, moved to the world frame with the generating poses, voxel-filtered as the
    reference filters the merged local map on every update (:1630-1637), then grown to `map_points` by tiled
    replication (synth.grow_map)."""
    cm, sm = [], []
    for k in range(base - 8, base):
        v, l = make_scan(synth, cfg, k, motion=False)
        ctx.scan_upload(0, v, l)
        ctx.extract(0, 1)
        ctx.undistort(0, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
        ctx.downsample(0, 1)
        T = synth.pose_matrix(k)
        cm.append(synth.transform(T, ctx.features_download(0, 0).astype(np.float64)).astype(np.float32))
        sm.append(synth.transform(T, ctx.features_download(0, 1).astype(np.float64)).astype(np.float32))
    cm = synth.voxel_filter(np.concatenate(cm), ctx.cfg.leaf_corner)
    sm = synth.voxel_filter(np.concatenate(sm), ctx.cfg.leaf_surf)
    n_corner_map = max(64, map_points // 10)
    corner_map = synth.grow_map(cm, n_corner_map, seed=7)
    surf_map = synth.grow_map(sm, map_points - n_corner_map, seed=8)
    full_tiles = max(1, min(n_corner_map // max(len(cm), 1), (map_points - n_corner_map) // max(len(sm), 1)))
    return corner_map, surf_map, full_tiles


def pinned(a):
    """Host copy in page-locked memory (the staging a real feeder would use)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return a
    t = torch.from_numpy(a.view(np.uint8).reshape(-1)).pin_memory()
    return t.numpy().view(a.dtype).reshape(a.shape)


# ---- --dump-outputs ---------------------------------------------------------------------------------------------------
DUMP_BYTES = 64 << 20   # all arrays of one rank together


def throughput_outputs(ctx, x, n_slots, max_slots=64):
    """What the last timed step computed: the poses mml_step returned for every resident slot, and the down-sampled corner /
    surf features of the first min(n_slots, max_slots) slots (the distinct scans), as many whole slots as fit DUMP_BYTES."""
    out = {"poses": np.ascontiguousarray(x, np.float64)}
    budget = DUMP_BYTES - out["poses"].nbytes
    corner, surf, counts = [], [], []
    for s in range(min(n_slots, max_slots)):
        cf = np.ascontiguousarray(ctx.features_download(s, 0), np.float32).reshape(-1, 3)
        sf = np.ascontiguousarray(ctx.features_download(s, 1), np.float32).reshape(-1, 3)
        nbytes = cf.nbytes + sf.nbytes + 16
        if nbytes > budget:
            break
        budget -= nbytes
        corner.append(cf)
        surf.append(sf)
        counts.append((len(cf), len(sf)))
    out["corner_features"] = np.concatenate(corner) if corner else np.zeros((0, 3), np.float32)
    out["surf_features"] = np.concatenate(surf) if surf else np.zeros((0, 3), np.float32)
    out["feature_counts"] = np.array(counts, np.float64).reshape(-1, 2)
    return out


def dump_outputs(path, rank, arrays):
    """DIR/<name>.npy for every array (DIR/<name>_rank<r>.npy on rank r > 0)."""
    arrays = {name: np.asarray(a) for name, a in arrays.items()}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_BYTES
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ("_rank%d" % rank if rank else "") + ".npy"), a)


# >>> cpu_baseline leg (the only code that may name the oracle)
def write_cpu_workload(path, ctx, cfg, scans, dR, dt, x0, corner_map, surf_map, gn_iters, thres):
    import struct
    c = ctx.cfg
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", 0x424c4d4d, len(scans), c.n_rings))
        f.write(struct.pack("<ffff", c.pitch0_deg, c.pitch_step_deg, c.near_th, c.far_th))
        f.write(struct.pack("<i", c.n_livox_lines))
        f.write(struct.pack("<ff", c.leaf_corner, c.leaf_surf))
        f.write(struct.pack("<i", gn_iters))
        f.write(struct.pack("<d", thres))
        for k, (v, l) in enumerate(scans):
            v = np.ascontiguousarray(v, np.float32).reshape(-1, 4)
            f.write(struct.pack("<i", len(v)))
            f.write(v.tobytes())
            f.write(struct.pack("<i", len(l)))
            f.write(np.ascontiguousarray(l).tobytes())
            f.write(np.ascontiguousarray(dR[k], np.float64).tobytes())
            f.write(np.ascontiguousarray(dt[k], np.float64).tobytes())
            f.write(np.ascontiguousarray(x0[k], np.float64).tobytes())
        for m in (corner_map, surf_map):
            m = np.ascontiguousarray(m, np.float32).reshape(-1, 3)
            f.write(struct.pack("<i", len(m)))
            f.write(m.tobytes())


def cpu_baseline_cpp(ctx, cfg, scans, dR, dt, x0, corner_map, surf_map, gn_iters, thres, seconds, x_gpu):
    """oracle/bench_cpu on this box's host cores.  The oracle is the checker / reported baseline, never the product."""
    import tempfile
    exe = os.path.join(ROOT, "oracle", "build", "bench_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    n_cpu = min(len(scans), 8)  # kd-tree queries dominate: 8 distinct scans keep the workload file small
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "workload.bin")
        write_cpu_workload(path, ctx, cfg, scans[:n_cpu], dR, dt, x0, corner_map, surf_map, gn_iters, thres)
        out = subprocess.run([exe, path, "--single-seconds", str(seconds), "--shaped-seconds", str(seconds), "--parallel-seconds",
                              str(seconds * 1.5)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        return {"error": (out.stderr or out.stdout)[-300:]}
    r = json.loads(out.stdout.strip().splitlines()[-1])
    poses = np.array(r.pop("poses"))
    sp = r["scan_parallel"]
    return {"value": sp["scans_per_s"], "unit": "scans/s", "cores": sp["cores"], "kind": "port",
            "sample": "%d scans (cycled over %d distinct), one worker process per pinned core for %.0f s; same map / poses / %d fixed "
                      "iterations as the GPU step, kd-tree build excluded; oracle/bench_cpu, g++ -O3 -ffp-contract=off"
                      % (sp["scans"], n_cpu, seconds * 1.5, gn_iters),
            "cpu_model": r["cpu_model"], "host_cores": r["host_cores"], "cgroup_cpu_quota": r.get("cgroup_cpu_quota"),
            "single_thread": r["single"],
            "reference_shaped": dict(r["reference_shaped"], layout="6 threads over the Livox lines, rings serial, corner || surf "
                                                                     "association, 6-thread solve (unionFeatureExtract.cpp:1008-1015,1228-1230; "
                                                                     "Estimator.cpp:1271-1297,1430)"),
            "kdtree_build_s": r["kdtree_build_s"], "pose_diff_vs_gpu": float(np.abs(poses - x_gpu[:len(poses)]).max())}


# <<< cpu_baseline leg


# ---- throughput (configs 1, 3, 4) ---------------------------------------------------------------------------------------
def run_throughput(args, rank, local_rank, world, dist):
    import torch
    from scipy.spatial.transform import Rotation as Rsc
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    cfg = dict(CONFIGS[args.config])
    B = args.slots or cfg["slots"]
    batch = args.batch or cfg["scans_per_step"]
    passes = max(1, (batch + B - 1) // B)
    batch = passes * B
    map_points = args.map_points or cfg["map_points"]
    gn_iters = args.gn_iters or cfg["gn_iters"]
    ctx = make_context(M, cfg, B, local_rank, args, map_points)
    dev_name, cus, hbm = ctx.device_info()
    # stream lanes of mml_step: with passes of 8192 (4096) scans two lanes of 4096 (2048) give the best rate -- 2 / 3 / 4 / 6 lanes:
    # 360 / 360 / 351 / 340 k scans/s at configs[1], 76.4 / 75.7 k at configs[3] -- which is the library's default (capi.hip:
    # n_lanes = 2), so without $MML_LANES the bench runs the library as it comes and never calls mml_set_lanes before the timed region
    n_lanes = int(os.environ.get("MML_LANES", "0")) or 2
    if "MML_LANES" in os.environ:
        ctx.set_lanes(n_lanes)

    # ---- synthetic inputs (same on every rank except the seed offset) ---------------------------------------
    base = 100 + 1000 * rank
    nd = max(1, min(args.distinct or cfg["distinct"], B))
    scans = [make_scan(synth, cfg, base + k) for k in range(nd)]
    corner_map, surf_map, full_tiles = build_maps(ctx, synth, cfg, base, map_points)
    ctx.map_set_local(0, corner_map)
    ctx.map_set_local(1, surf_map)
    # The map is the scene tiled on a lattice: unless --no-spread, consecutive groups of slots sit on different tiles
    # (their initial poses are shifted by the tile offset, the sensor-frame points are what they are), so the
    # association of a batch touches the whole map, not the one tile around the origin.
    # (at most B / (2 nd) tiles, so that every (scan, tile) pair occurs in at least two slots: the replica check below compares them)
    tiles = synth.tile_offsets(1 if args.no_spread else max(1, min(full_tiles, B // (2 * nd))))
    dR = np.zeros((B, 9))
    dt = np.zeros((B, 3))
    x0 = np.zeros((B, 6))
    gt = np.zeros((B, 3))
    for s in range(B):
        k = s % nd
        ctx.scan_upload(s, scans[k][0], scans[k][1])
        # true motion over the sweep (the scans are simulated with it) and a perturbed initial pose
        mR, mt = synth.sweep_motion(base + k)
        dR[s], dt[s] = mR.reshape(9), mt
        off = tiles[(s // nd) % len(tiles)]
        Tp = synth.pose_matrix(base + k).copy()
        gt[s] = Tp[:3, 3] + off
        Tp[:3, 3] += np.array([0.03, -0.02, 0.01]) + off
        Tp[:3, :3] = Tp[:3, :3] @ Rsc.from_rotvec([0.002, -0.001, 0.004]).as_matrix()
        x0[s] = np.concatenate([Tp[:3, 3], Rsc.from_matrix(Tp[:3, :3]).as_rotvec()])
    ctx.synchronize()
    exTlb = np.eye(4)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def one_step():
        x = None
        for _ in range(passes):
            x = ctx.step(0, B, dR, dt, exTlb, 25.0, gn_iters, x0)
        return x

    for _ in range(args.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        x = one_step()
    barrier()
    elapsed = time.perf_counter() - t0
    errors = []
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, throughput_outputs(ctx, x, nd))

    # pose sanity: the step must actually have registered the scans.  Only the slots on tile 0 count -- the original,
    # un-jittered copy of the scene, where the generating pose IS the registration optimum up to the range noise; on the
    # jittered copies of grow_map the optimum sits wherever the jitter put it -- and the number is asserted, not just printed.
    on_tile0 = np.array([(s // nd) % len(tiles) == 0 for s in range(B)])
    gt_err = float(np.abs(x[on_tile0, :3] - gt[on_tile0]).max())

    def headline(elapsed):
        return {
            "metric": "scans/s (feature-extract+kNN+%d GN iters) on %s" % (gn_iters, "16-ring x1800 + Livox 24k fused cloud" if args.config == 1 else cfg["name"].split(": ")[1]),
            "value": world * batch * args.steps / elapsed, "unit": "scans/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32/f64", "data": "synthetic",
            "config": {"workload": "%s, local map %d pts, 1 association pass (thres_dist 25), %d GN iterations, W=1"
                                   % (cfg["name"], map_points, gn_iters),
                       "scans_per_step_per_gpu": batch, "resident_slots": B, "passes_per_step": passes, "stream_lanes": n_lanes, "distinct_scans": nd,
                       "map_tiles_touched": len(tiles), "map_tiles_complete": full_tiles, "parallelism": "scan-sharded x%d" % world,
                       "device": dev_name, "cus": cus, "max_pose_err_vs_gt_m_tile0": gt_err, "timed_region_s": elapsed}}

    if not args.full:   # the plain run: the headline and nothing else
        bad = 0.0 if gt_err < 0.05 else 1.0
        if dist is not None:
            t = torch.tensor([elapsed, bad], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed, bad = float(t[0].item()), float(t[1].item())
        if bad:
            raise RuntimeError("bench: the step did not register the scans (pose error %.3f m on the un-jittered tile)" % gt_err)
        return (json.dumps(dict(headline(elapsed), errors=errors)) if rank == 0 else None), False, errors

    # ---- --full from here on: every section below runs outside the timed region -----------------------------------------
    # ---- replica check (outside the timed region): slots that were given the same scan on the same map tile with the same initial
    # pose must hold bit-identical results -- labels, rings, undistorted cloud, times, both stacks, both factor lists, pose
    # (mml_slot_digest, ten words per slot) -- at the launch shapes of the timed region.  tests/test_gpu_shapes.py ties the
    # first slot of such a group to the oracle; here the equality is checked on the run that is being reported.
    dg_timed = ctx.slot_digest(0, B)
    replica = replica_check(dg_timed, x, [(s % nd, (s // nd) % len(tiles)) for s in range(B)])
    # (every rank learns of a mismatch on any rank BEFORE anyone raises: a rank that raised alone would leave the others waiting
    #  in the next collective)
    any_mismatch = replica["mismatches"]
    if dist is not None:
        t = torch.tensor([float(any_mismatch)], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        any_mismatch = int(t.item())
    if any_mismatch:
        raise RuntimeError("bench: replica check failed (this rank: %s)" % json.dumps(replica))
    # Per-kernel durations for the roofline object: the timed region overlaps sub-batches on the stream lanes, so kernel
    # time there is shared between concurrent kernels.  The same step is therefore repeated on ONE stream (every
    # kernel covers the whole batch and owns the device) with HIP events around each stage on that stream; these
    # are the launches of grid size `KB scans` in the rocprofv3 summary under profiles/ (KB = min(B, 1024): distinct,
    # in that summary, from the timed region's per-lane launches of B / lanes scans).
    KB = min(B, 1024)
    ctx.set_lanes(1)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.kernel_steps):
        ctx.step(0, KB, dR[:KB], dt[:KB], exTlb, 25.0, gn_iters, x0[:KB])
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    # ... and the one-lane pass over the first KB slots must leave exactly what the timed region's lanes left there
    dg_one = ctx.slot_digest(0, KB)
    replica["one_lane_vs_timed_region_slots"] = KB
    replica["one_lane_vs_timed_region_mismatches"] = int(np.any(dg_one != dg_timed[:KB], axis=1).sum())
    ctx.set_lanes(n_lanes)
    if dist is not None:
        t = torch.tensor([elapsed, float(replica["one_lane_vs_timed_region_mismatches"])], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0].item())
        if t[1].item() > 0 and not replica["one_lane_vs_timed_region_mismatches"]:
            raise RuntimeError("bench: the single-lane pass differs from the timed region on another rank")
    if replica["one_lane_vs_timed_region_mismatches"]:
        raise RuntimeError("bench: the single-lane pass differs from the timed region: %s" % json.dumps(replica))

    # ---- where the headline comes from: the same step at other batch sizes (outside the timed region; rank 0) -----------------
    # `value` needs thousands of resident slots; the reference registers ONE scan at a time.  Scans/s of mml_step over the first S
    # slots, the library's lanes as in the timed region, every size run for >= 0.3 s.
    value_by_slots = None
    if rank == 0 and not args.skip_by_slots:
        value_by_slots = {}
        try:
            for S in (1, 8, 64, 512, 4096, 8192):
                if S > B:
                    continue
                ctx.step(0, S, dR[:S], dt[:S], exTlb, 25.0, gn_iters, x0[:S])
                n_it, t1 = 0, time.perf_counter()
                while True:
                    ctx.step(0, S, dR[:S], dt[:S], exTlb, 25.0, gn_iters, x0[:S])
                    n_it += 1
                    el = time.perf_counter() - t1
                    if el >= 0.3:
                        break
                value_by_slots[str(S)] = {"scans_per_s": S * n_it / el, "ms_per_call": el / n_it * 1e3}
        except Exception as e:
            errors.append("value_by_slots: " + repr(e)[:200])

    if not gt_err < 0.05:
        raise RuntimeError("bench: the step did not register the scans (pose error %.3f m on the un-jittered tile)" % gt_err)

    # ---- roofline for the dominant kernel ---------------------------------------------------------------------
    info = [ctx.scan_info(s) for s in range(min(B, nd))]
    n_v = float(np.mean([i.n_velo for i in info])) * KB
    n_l = float(np.mean([i.n_points - i.n_velo for i in info])) * KB
    nf = float(np.mean([len(ctx.features_download(s, 0)) + len(ctx.features_download(s, 1)) for s in range(min(B, nd))])) * KB
    # a stage's brackets of one step cover all its kernels over the KB scans: time per step = time per "launch of KB scans"
    stage_ms = {k: v[0] / max(args.kernel_steps, 1) for k, v in prof.items() if v[1] > 0}
    dom = max(stage_ms, key=stage_ms.get)
    alg_bytes = STAGE_BYTES.get(dom, lambda *a: 0)(n_v, n_l, nf, gn_iters)
    achieved = alg_bytes / (stage_ms[dom] * 1e-3) / 1e9 if stage_ms[dom] > 0 else 0.0
    # PMC evidence of the same command, committed under profiles/ by tools/profile_round.sh (separate rocprofv3 passes):
    # HBM traffic per launch (FETCH_SIZE / WRITE_SIZE) and VALU wave-instructions per launch (SQ_INSTS_VALU)
    suffix = "" if args.config == 1 else "_config%d" % args.config
    # (both files carry the hash of the library they were measured on; numbers from another build are reported as stale)
    lib_sha = lib_sha16(M)
    traffic, traffic_file, traffic_stale = None, None, None
    for tag in ("r06", "r05", "r04", "r03", "r02"):
        tr_file = os.path.join(ROOT, "profiles", "traffic_%s%s.json" % (tag, suffix))
        if os.path.exists(tr_file):
            try:
                tr = json.load(open(tr_file))
                if tr.get(dom) is not None:
                    traffic = tr[dom] * KB / float(tr.get("scans_per_launch", KB))
                    traffic_file = os.path.relpath(tr_file, ROOT)
                    traffic_stale = tr.get("lib_sha16") != lib_sha
                    break
            except Exception:
                pass
    # Issue-bound kernels.  The VALU issue peak is MEASURED on the box (mml_issue_rate; tools/issue_probe.hip has every class,
    # profiles/r06_issue_probe.txt): a wave64 float / VOP3 / DPP instruction holds a SIMD for 4 cycles (v_fma_f32, v_mul_f32,
    # v_pk_fma_f32, v_fma_f64: 6.0e11 wave-instructions/s on 256 CUs), a simple 32-bit integer VOP2 instruction for 2.2
    # (v_add_u32: 1.12e12), v_rcp_f32 for 8.  `peak` is the v_fma_f32 rate -- the roof of a kernel made of float arithmetic --,
    # `peak_int` the v_add_u32 rate; the fraction of `peak` the dominant stage reaches says how much of its time is instruction
    # issue -- for such a kernel THIS is the roof, not HBM.
    issue = None
    try:
        issue_peak, issue_peak_int, peak_source = float(ctx.issue_rate(0)), float(ctx.issue_rate(1)), "measured"
    except Exception as e:
        issue_peak, issue_peak_int, peak_source = cus * 4 * VALU_CLOCK_HZ / 4.0, None, "assumed"
        errors.append("issue_rate: " + repr(e)[:200])
    sq_file = next((f for f in (os.path.join(ROOT, "profiles", "sq_%s%s.json" % (tag, suffix)) for tag in ("r06", "r05", "r04", "r03"))
                    if os.path.exists(f)), None)
    if sq_file is not None:
        try:
            sq = json.load(open(sq_file))
            if dom in sq and stage_ms[dom] > 0:
                wi = sq[dom]["valu_wave_instr"] * KB / float(sq.get("scans_per_launch", KB))
                peak = issue_peak
                issue = {"valu_wave_instr_per_launch": wi, "achieved": wi / (stage_ms[dom] * 1e-3), "peak": peak,
                         "peak_int": issue_peak_int, "peak_source": peak_source,
                         "unit": "wave-instructions/s", "frac": wi / (stage_ms[dom] * 1e-3) / peak,
                         "source": os.path.relpath(sq_file, ROOT), "stale": sq.get("lib_sha16") != lib_sha}
        except Exception:
            issue = None
    # counter traffic / algorithmic bytes for every stage the counter file has (the file is per KB scans): wasted re-reads show here
    traffic_ratio = None
    if traffic_file is not None:
        try:
            tr = json.load(open(os.path.join(ROOT, traffic_file)))
            scale = KB / float(tr.get("scans_per_launch", KB))
            traffic_ratio = {"stale": traffic_stale}
            tot_t = tot_a = 0.0
            for st in stage_ms:
                ab = STAGE_BYTES.get(st, lambda *a: 0)(n_v, n_l, nf, gn_iters)
                if tr.get(st) is not None:
                    tot_t += tr[st] * scale
                    tot_a += ab
                    if ab > 0:
                        traffic_ratio[st] = tr[st] * scale / ab
            traffic_ratio["step"] = tot_t / tot_a if tot_a > 0 else None          # against the per-kernel budgets of STAGE_BYTES
            traffic_ratio["step_traffic_bytes_per_launch"] = tot_t
            # ... and against SURVEY 8(d)'s per-scan figure (48 N + 112 F + 72 F I), which counts no intermediate array at all
            traffic_ratio["step_vs_survey_8d"] = tot_t / ((48 * (n_v + n_l) + 112 * nf + 72 * nf * gn_iters) or 1.0)
        except Exception as e:
            errors.append("traffic_ratio: " + repr(e)[:200])
    hbm_frac = achieved / HBM_PEAK_GBPS
    # (a stale instruction count -- taken on another build of the library -- does not decide the bound)
    bound = "valu-issue" if issue is not None and not issue["stale"] and issue["frac"] > max(hbm_frac, 0.5) else "hbm"
    # the practical HBM roof of THIS box: a device-to-device copy (read + write counted), next to the 8 TB/s of the data sheet
    try:
        copy_gbps = float(ctx.copy_bandwidth(1 << 30, 10))
    except Exception as e:
        copy_gbps = None
        errors.append("copy_bandwidth: " + repr(e)[:200])
    bytes_per_scan = 48 * (n_v + n_l) / KB + 112 * nf / KB + 72 * nf / KB * gn_iters
    total_scans = world * batch * args.steps
    value = total_scans / elapsed

    # ---- PCIe-inclusive rate: the boundary hands over host buffers (mml_scan_upload) --------------------------------
    # one pass with every scan of the batch copied in from pinned host memory in front of the step (serial: upload, then
    # compute); never `value`
    with_upload = None
    B_all = B
    try:
        if args.skip_upload:
            raise RuntimeError("skipped (--skip-upload)")
        B = min(B_all, 2048)  # (this section on at most 2048 slots: its pinned staging arrays are slots x scan size)
        ps = [(pinned(v), pinned(l)) for v, l in scans]
        ctx.synchronize()
        t1 = time.perf_counter()
        for s in range(B):
            ctx.scan_upload(s, ps[s % nd][0], ps[s % nd][1])
        ctx.synchronize()
        t_up = time.perf_counter() - t1
        t1 = time.perf_counter()
        ctx.step(0, B, dR[:B], dt[:B], exTlb, 25.0, gn_iters, x0[:B])
        t_st = time.perf_counter() - t1
        up_bytes = sum(scans[s % nd][0].nbytes + scans[s % nd][1].nbytes for s in range(B))
        with_upload = {"slots": B, "scans_per_s": B / (t_up + t_st) * world, "upload_GBps": up_bytes / t_up / 1e9,
                       "upload_ms_per_scan": t_up / B * 1e3, "note": "uploads (pinned host memory, one hipMemcpyAsync per "
                       "sensor per scan) serialised in front of the step; with uploads overlapped the bound is min(upload, compute)"}
        # the same batch staged in two slot-strided pinned arrays and copied with mml_scan_upload_batch (two copies in all)
        c = ctx.cfg
        if c.max_velo_points % 64 == 0 and c.max_livox_points % 64 == 0:
            vb = torch.zeros((B, c.max_velo_points, 4), dtype=torch.float32).pin_memory().numpy()
            lb = torch.zeros((B, c.max_livox_points * 20), dtype=torch.uint8).pin_memory().numpy().view(synth.LIVOX_DTYPE).reshape(B, c.max_livox_points)
            nvs, nls = np.zeros(B, np.int32), np.zeros(B, np.int32)
            for s in range(B):
                v, l = scans[s % nd]
                nvs[s], nls[s] = len(v), len(l)
                vb[s, :len(v)] = v
                lb[s, :len(l)] = l
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.scan_upload_batch(0, vb, nvs, lb, nls)
            ctx.synchronize()
            t_upb = time.perf_counter() - t1
            with_upload["batched"] = {"scans_per_s": B / (t_upb + t_st) * world, "upload_GBps": (vb.nbytes + lb.nbytes) / t_upb / 1e9,
                                      "note": "mml_scan_upload_batch: the whole batch in two host-to-device copies, then the step"}
            # the feeder a deployment would run: two slot ranges, the copy of one under the kernels of the other
            h = B // 2
            xa = xb = None
            ctx.scan_upload_batch(0, vb[:h], nvs[:h], lb[:h], nls[:h])
            ctx.synchronize()
            rounds = 4
            t1 = time.perf_counter()
            for _ in range(rounds):
                ctx.scan_upload_batch(h, vb[h:2 * h], nvs[h:2 * h], lb[h:2 * h], nls[h:2 * h])
                xa = ctx.step(0, h, dR[:h], dt[:h], exTlb, 25.0, gn_iters, x0[:h])
                ctx.scan_upload_batch(0, vb[:h], nvs[:h], lb[:h], nls[:h])
                xb = ctx.step(h, h, dR[h:2 * h], dt[h:2 * h], exTlb, 25.0, gn_iters, x0[h:2 * h])
            ctx.synchronize()
            t_pipe = time.perf_counter() - t1
            with_upload["overlapped"] = {"scans_per_s": rounds * 2 * h / t_pipe * world,
                                         "pose_diff_vs_resident": float(max(np.abs(xa - x[:h]).max(), np.abs(xb - x[h:2 * h]).max())),
                                         "note": "two slot ranges alternate: mml_scan_upload_batch of one range (own copy stream) runs "
                                                 "under mml_step of the other; every scan crosses PCIe once per step"}
    except Exception as e:
        with_upload = {"error": repr(e)[:200]}
        if not args.skip_upload:
            errors.append("value_with_upload: " + repr(e)[:200])
    B = B_all

    # ---- joint window solve across ranks through the C-ABI: one frame per GPU, ncclAllGather of the
    # 32-double normal-equation record per evaluation, the dogleg state machine resident on every device.  Outside the
    # timed region; reported next to the sharded throughput because the live path never exchanges data.
    window = None
    window_timed_out = False
    if dist is not None or args.window_demo:
        def window_section():
            W = world
            if dist is not None:
                # every rank takes the same decision before any of them enters ncclCommInitRank: a rank that refused alone
                # (two RCCL copies mapped, Context.comm_init) would leave the others waiting in the rendezvous
                two = torch.tensor([1.0 if len(M.rccl_libraries()["loaded"]) > 1 else 0.0], device="cuda")
                dist.all_reduce(two, op=dist.ReduceOp.MAX)
                if two.item() > 0:
                    raise RuntimeError("two RCCL copies are mapped on at least one rank: window section skipped on all ranks")
                idt = torch.zeros(M.COMM_ID_BYTES, dtype=torch.uint8, device="cuda")
                if rank == 0:
                    idt = torch.frombuffer(bytearray(M.comm_unique_id()), dtype=torch.uint8).to("cuda")
                dist.broadcast(idt, src=0)
                comm_id = bytes(idt.cpu().numpy().tobytes())
            else:
                comm_id = M.comm_unique_id()
            ctx.comm_init(W, rank, comm_id)
            # replicate rank 0's map (what a fleet of pose nodes sharing one map would do), then every rank associates its
            # own frame (slot 0 still holds the features of the last step) against it
            t1 = time.perf_counter()
            ctx.comm_broadcast_local_map(0)
            t_map = time.perf_counter() - t1
            xm = x0[0].copy()
            xm[:3] -= tiles[0]
            Tw = np.eye(4)
            Tw[:3, :3] = Rsc.from_rotvec(xm[3:]).as_matrix()
            Tw[:3, 3] = xm[:3]
            ctx.associate(0, 1, Tw[None], 1.0)
            res = None
            lat = []
            for rep in range(6):
                res = ctx.window_solve_allgather(0, 1, xm[None], np.eye(4), max_iters=gn_iters, fixed=False, huber=0.0, w_tan=3e-4)
                lat.append(res[3].device_ms)
            xl, xw, sm, tim = res
            agree = True
            if dist is not None:
                chk = torch.from_numpy(xw.reshape(-1).copy()).to("cuda")
                ref = chk.clone()
                dist.broadcast(ref, src=0)
                ag = torch.tensor([1.0 if torch.equal(ref, chk) else 0.0], device="cuda")
                dist.all_reduce(ag, op=dist.ReduceOp.MIN)
                agree = bool(ag.item() == 1.0)
            # map-update exchange: rank 0's key scan to every replica
            t1 = time.perf_counter()
            ctx.comm_broadcast_features(0, 0)
            ctx.synchronize()
            t_feat = time.perf_counter() - t1
            result = {"frames": W, "path": "C-ABI mml_window_solve_allgather (ncclAllGather on the ctx stream, device-resident dogleg)",
                      "iterations": sm.iterations, "termination": sm.termination, "evaluations": tim.evaluations,
                      "rounds": tim.rounds, "device_ms": float(np.median(lat)), "ms_per_evaluation": float(np.median(lat)) / max(tim.rounds, 1),
                      "ranks_agree_bitwise": agree, "map_broadcast_ms": t_map * 1e3, "feature_broadcast_ms": t_feat * 1e3,
                      "own_frame_err_vs_gt_m": float(np.abs(xl[0][:3] - synth.pose_matrix(base)[:3, 3]).max())}
            ctx.comm_destroy()
            return result

        # The section talks to the other ranks through collectives that nothing in this container could exercise at N > 1
        # (one GPU here): it runs under a watchdog so that a fault in it can cost the window report, never the bench line.
        import threading
        box = {}

        def guarded():
            try:
                torch.cuda.set_device(local_rank)  # the current device is per thread
                box["window"] = window_section()
            except Exception as e:
                box["window"] = {"error": repr(e)[:300]}
        th = threading.Thread(target=guarded, daemon=True)
        th.start()
        th.join(180.0)
        if th.is_alive():
            window, window_timed_out = {"error": "window section timed out after 180 s"}, True
        else:
            window = box.get("window")
        if isinstance(window, dict) and "error" in window:
            errors.append("window_solve: " + str(window["error"])[:200])

    # ---- CPU baseline: the oracle on this box's host cores (rank 0, N = 1 only) ----------------------------------
    cpu = None
    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        try:
            xs = x0.copy()
            xs[:, :3] -= np.array([tiles[(s // nd) % len(tiles)] for s in range(B)])
            xg = x.copy()
            xg[:, :3] -= np.array([tiles[(s // nd) % len(tiles)] for s in range(B)])
            cpu = cpu_baseline_cpp(ctx, cfg, scans, dR, dt, xs, corner_map, surf_map, gn_iters, 25.0, args.cpu_seconds, xg)
        except Exception as e:
            cpu = {"error": repr(e)[:300]}
        if isinstance(cpu, dict) and "error" in cpu:
            errors.append("cpu_baseline: " + str(cpu["error"])[:200])

    if rank == 0:
        out = headline(elapsed)
        out["config"].update(features_per_scan=nf / KB, points_per_scan=(n_v + n_l) / KB, algorithmic_bytes_per_scan=bytes_per_scan)
        out.update({
            "value_with_upload": with_upload,
            "roofline": {"bound": bound, "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": hbm_frac, "traffic": traffic, "traffic_source": traffic_file, "traffic_stale": traffic_stale,
                         "lib_sha16": lib_sha, "issue": issue,
                         "measured_copy_GBps": copy_gbps,
                         "frac_of_measured_copy": (achieved / copy_gbps) if copy_gbps else None,
                         "avg_launch_ms": stage_ms[dom], "algorithmic_bytes_per_launch": alg_bytes,
                         "scans_per_launch": KB, "timing": "HIP events, %d single-stream steps after the timed region" % args.kernel_steps,
                         "whole_path_frac": bytes_per_scan * value / world / 1e9 / HBM_PEAK_GBPS,
                         "stage_ms_per_launch": stage_ms, "traffic_ratio": traffic_ratio},
            "cpu_baseline": cpu,
            "window_solve": window,
            "rccl": rccl_report(M),
            "replica_check": replica,
            "value_by_slots": value_by_slots,
            "errors": errors,
        })
        return json.dumps(out), window_timed_out, errors
    return None, window_timed_out, errors


# ---- pose conversions of the replay loop (module level: tests/test_host.py exercises them without a device) -------------
# Plain numpy on 3 x 3 arrays.  scipy's Rotation.from_matrix costs ~50 us a call (it
# orthogonalises through an SVD); the loop converts ten poses per scan, which was a fifth of the per-scan time this harness
# reported for the device path it is there to measure.  (Checked against scipy below, once, outside the timed region.)
def quat_from_matrix(R):   # (x, y, z, w), Shepperd's method
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R[0, 0], R[0, 1], R[0, 2], R[1, 0], R[1, 1], R[1, 2], R[2, 0], R[2, 1], R[2, 2]
    tr = m00 + m11 + m22
    if tr > 0.0:
        r = np.sqrt(1.0 + tr)
        q = np.array([(m21 - m12) / (2 * r), (m02 - m20) / (2 * r), (m10 - m01) / (2 * r), 0.5 * r])
    elif m00 >= m11 and m00 >= m22:
        r = np.sqrt(1.0 + m00 - m11 - m22)
        q = np.array([0.5 * r, (m01 + m10) / (2 * r), (m02 + m20) / (2 * r), (m21 - m12) / (2 * r)])
    elif m11 >= m22:
        r = np.sqrt(1.0 - m00 + m11 - m22)
        q = np.array([(m01 + m10) / (2 * r), 0.5 * r, (m12 + m21) / (2 * r), (m02 - m20) / (2 * r)])
    else:
        r = np.sqrt(1.0 - m00 - m11 + m22)
        q = np.array([(m02 + m20) / (2 * r), (m12 + m21) / (2 * r), 0.5 * r, (m10 - m01) / (2 * r)])
    q /= np.sqrt(q @ q)
    return q if q[3] >= 0 else -q


def matrix_from_quat(q):
    x, y, z, w = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rotvec_from_matrix(R):
    q = quat_from_matrix(R)
    nv = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    k = 2.0 if nv < 1e-12 else 2.0 * np.arctan2(nv, q[3]) / nv
    return k * q[:3]


def matrix_from_rotvec(v):
    th = np.sqrt(v @ v)
    im, re = (0.5, 1.0) if th < 1e-12 else (np.sin(0.5 * th) / th, np.cos(0.5 * th))
    return matrix_from_quat(np.array([im * v[0], im * v[1], im * v[2], re]))


def rotvec_from_quat(q):
    nv = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    w = q[3] if q[3] >= 0 else -q[3]
    sg = 1.0 if q[3] >= 0 else -1.0
    k = 2.0 if nv < 1e-12 else 2.0 * np.arctan2(nv, w) / nv
    return (sg * k) * np.asarray(q[:3], dtype=np.float64)


def matrices_from_x(x):    # (W, 6) poses (translation | rotation vector) -> (W, 4, 4), Rodrigues, all frames at once
    v = x[:, 3:]
    th = np.sqrt((v * v).sum(1))
    k = v / np.maximum(th, 1e-300)[:, None]
    c, sn = np.cos(th), np.sin(th)
    T = np.zeros((len(x), 4, 4))
    T[:, :3, :3] = (1 - c)[:, None, None] * k[:, :, None] * k[:, None, :]
    T[:, 0, 0] += c
    T[:, 1, 1] += c
    T[:, 2, 2] += c
    T[:, 0, 1] -= sn * k[:, 2]
    T[:, 1, 0] += sn * k[:, 2]
    T[:, 0, 2] += sn * k[:, 1]
    T[:, 2, 0] -= sn * k[:, 1]
    T[:, 1, 2] -= sn * k[:, 0]
    T[:, 2, 1] += sn * k[:, 0]
    T[:, :3, 3] = x[:, :3]
    T[:, 3, 3] = 1.0
    return T


def pose_helpers_selfcheck():
    """The plain-numpy conversions against scipy (run once per replay, outside the timed region; also tests/test_host.py)."""
    from scipy.spatial.transform import Rotation as Rsc
    _rng = np.random.default_rng(5)
    _xs = np.concatenate([_rng.normal(0, 3, (16, 3)), _rng.normal(0, 1.2, (16, 3))], axis=1)
    _xs[0, 3:] = 0.0
    assert np.abs(matrices_from_x(_xs)[:, :3, :3] - Rsc.from_rotvec(_xs[:, 3:]).as_matrix()).max() < 1e-12
    for _ in range(64):
        _R = Rsc.from_rotvec(_rng.normal(0, 1.5, 3)).as_matrix()
        assert np.abs(rotvec_from_matrix(_R) - Rsc.from_matrix(_R).as_rotvec()).max() < 1e-12
        assert np.abs(matrix_from_rotvec(rotvec_from_matrix(_R)) - _R).max() < 1e-12
        _q = Rsc.from_matrix(_R).as_quat()
        assert min(np.abs(quat_from_matrix(_R) - _q).max(), np.abs(quat_from_matrix(_R) + _q).max()) < 1e-12
        assert np.abs(matrix_from_quat(_q) - _R).max() < 1e-12
        assert np.abs(rotvec_from_quat(_q) - Rsc.from_matrix(_R).as_rotvec()).max() < 1e-12
        assert np.abs(rotvec_from_quat(-_q) - Rsc.from_matrix(_R).as_rotvec()).max() < 1e-12


R_PERT = matrix_from_rotvec(np.array((0.002, -0.001, 0.003)))   # the IMU-sized rotation error of the replay's predictions


def perturbed(T, dt_=(0.02, -0.015, 0.01), rv=None):
    """T with a translation error dt_ added and a rotation error exp(rv) (default: R_PERT) multiplied on the right."""
    T2 = T.copy()
    T2[:3, :3] = T[:3, :3] @ (R_PERT if rv is None else matrix_from_rotvec(np.asarray(rv, dtype=np.float64)))
    T2[:3, 3] = T[:3, 3] + np.asarray(dt_)
    return T2


def cpp_live_loop(scans, motions, predicted, reps=3):
    """Builds tools/live_loop.cpp (g++, against the in-tree library) and runs it on a scene file of the replay's scans: the
    odometry loop driven through the C++ adapter, timed with std::chrono inside the process.  -> its JSON object."""
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp(prefix="mml_live_")   # (the scene file is ~0.9 MB per scan: removed again below)
    try:
        return _cpp_live_loop_in(tmp, scans, motions, predicted, reps)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _cpp_live_loop_in(tmp, scans, motions, predicted, reps):
    import struct
    import subprocess
    from scipy.spatial.transform import Rotation as Rsc
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    exe, scene = os.path.join(tmp, "live_loop"), os.path.join(tmp, "scene.bin")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
           os.path.join(ROOT, "tools", "live_loop.cpp"), "-o", exe, "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("g++ tools/live_loop.cpp: " + out.stderr[-300:])
    with open(scene, "wb") as f:   # (the scene format of tests/cpp/adapter_gpu_probe.cpp, mode 0)
        f.write(struct.pack("<iii", 0x4d4d4c31, 0, len(scans)))
        for (v, l), (mR, mt), Tp in zip(scans, motions, predicted):
            v = np.ascontiguousarray(v, np.float32).reshape(-1, 4)
            f.write(struct.pack("<i", len(v)))
            f.write(v.tobytes())
            f.write(struct.pack("<i", len(l)))
            f.write(np.ascontiguousarray(l).tobytes())
            q = Rsc.from_matrix(Tp[:3, :3]).as_quat()
            for a in (mR.reshape(9), mt, Tp[:3, 3], q, np.zeros(3)):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
            f.write(struct.pack("<i", 0))
        f.write(struct.pack("<i", 0))
        f.write(struct.pack("<i", 0))
    run = subprocess.run([exe, scene, str(reps)], capture_output=True, text=True, timeout=600)
    if run.returncode != 0:
        raise RuntimeError("live_loop rc %d: %s" % (run.returncode, (run.stderr or run.stdout)[-300:]))
    return json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])


# ---- configs[2]: replay through the whole odometry loop ----------------------------------------------------------------
def run_replay(args, rank, local_rank, world, dist):
    import torch
    from scipy.spatial.transform import Rotation as Rsc
    M = importlib.import_module("multi-modal-loam_amd")
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    cfg = dict(CONFIGS[1])
    W = 8
    ctx = make_context(M, cfg, W, local_rank, args, 1 << 20)
    dev_name, cus, hbm = ctx.device_info()
    n = args.replay_scans
    k0 = 20 + 2000 * rank
    scans = [tuple(pinned(a) for a in make_scan(synth, cfg, k0 + i)) for i in range(n)]
    motions = [synth.sweep_motion(k0 + i) for i in range(n)]
    T_bl = np.eye(4)

    if args.full:
        pose_helpers_selfcheck()

    def replay(timed):
        odo = odometry.LidarOdometry(ctx, lidar_mode=2)
        poses_x = np.zeros((W, 6))   # the window's poses as (translation | rotation vector), the form the solver takes and returns
        lat, lat_win, poses = [], [], []
        T_prev = T_prev_gt = None
        worst_gt = 0.0
        t_all = time.perf_counter()
        for i in range(n):
            k = k0 + i
            T_gt = synth.pose_matrix(k)
            # prediction: previous estimate advanced by the true relative motion plus an IMU-sized error
            Tp = T_gt.copy() if T_prev is None else perturbed(T_prev @ np.linalg.inv(T_prev_gt) @ T_gt)
            slot = i % W
            t1 = time.perf_counter()
            ctx.scan_upload(slot, scans[i][0], scans[i][1])
            ctx.extract(slot, 1)
            ctx.undistort(slot, 1, motions[i][0].reshape(1, 9), motions[i][1].reshape(1, 3))
            P, Q, grew = odo.estimate_lidar_pose(slot, Tp[:3, 3], quat_from_matrix(Tp[:3, :3]))
            poses_x[slot, :3] = P
            poses_x[slot, 3:] = rotvec_from_quat(np.asarray(Q, dtype=np.float64))
            t2 = time.perf_counter()
            if i + 1 >= W and odo.n_surf_local > 100:
                # the 8-scan sliding window: every frame re-associated at its current pose (thres_dist 1, full-window
                # weights, Estimator.cpp:1203-1204) and solved jointly on the device
                ctx.associate(0, W, matrices_from_x(poses_x), 1.0, stats=False)  # enqueue only: the joint solve follows on the same stream
                xs, _, _ = ctx.solve(0, W, poses_x, T_bl, window=W, max_iters=10, huber=0.0, w_tan=3e-4)
                poses_x[:] = xs
            T = matrices_from_x(poses_x[slot:slot + 1])[0]
            t3 = time.perf_counter()
            lat.append((t3 - t1) * 1e3)
            lat_win.append((t3 - t2) * 1e3)
            poses.append(T)
            if i > 0:
                worst_gt = max(worst_gt, float(np.abs(T[:3, 3] - T_gt[:3, 3]).max()))
            T_prev, T_prev_gt = T, T_gt
        total = time.perf_counter() - t_all
        return dict(total=total, lat=lat, lat_win=lat_win, worst_gt=worst_gt, key_scans=odo.key_scans,
                    map=(odo.n_corner_local, odo.n_surf_local), poses=np.array(poses))

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    replay(False)  # warm-up pass (allocations of the map upkeep, code objects)
    # the timed region: the replay `reps` times over (every pass starts from an empty map and a fresh odometry object),
    # sized so that the default run times about 2 s
    reps = max(1, (2 * args.steps) // 5)
    barrier()
    runs = [replay(True) for _ in range(reps)]
    barrier()
    r = dict(total=sum(q["total"] for q in runs), lat=[v for q in runs for v in q["lat"]],
             lat_win=[v for q in runs for v in q["lat_win"][W:]], worst_gt=max(q["worst_gt"] for q in runs),
             key_scans=runs[-1]["key_scans"], map=runs[-1]["map"])
    elapsed = r["total"]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    hz = world * n * reps / elapsed
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, {"poses": runs[-1]["poses"]})

    def headline():
        return {
            "metric": "scans/s sustained (full odometry loop incl. upload + 8-scan window solve), one scan at a time",
            "value": hz, "unit": "scans/s", "n_gpus": world, "steps": n * reps, "warmup": n,
            "ms_per_step": elapsed / (n * reps) * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32/f64", "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: replay of %d fused 52.8k-pt scans (synthetic room, the office bag is not "
                                   "available offline) through EstimateLidarPose (5 outer x 10 inner) with the local map grown on the "
                                   "device, plus the joint solve of the 8-scan sliding window after every scan" % n,
                       "window": W, "replay_passes": reps, "device": dev_name, "cus": cus, "bag_rate_hz": BAG_RATE_HZ,
                       "headroom_vs_bag_rate": hz / world / BAG_RATE_HZ, "key_scans": r["key_scans"], "local_map_points": list(r["map"]),
                       "max_pose_err_vs_gt_m": r["worst_gt"], "timed_region_s": elapsed},
            "latency_ms": {"per_scan_p50": pctl(r["lat"], 50), "per_scan_p99": pctl(r["lat"], 99), "per_scan_max": float(np.max(r["lat"])),
                           "window8_part_p50": pctl(r["lat_win"], 50), "window8_part_p99": pctl(r["lat_win"], 99)}}

    if not args.full:   # the plain run: the headline and nothing else
        return (json.dumps(dict(headline(), errors=[])) if rank == 0 else None), []

    # ---- --full from here on ----------------------------------------------------------------------------------------------
    # B = 1 latency of the configs[1] step against the replay's final map, and of the W = 8 joint solve alone
    dR1, dt1 = motions[-1][0].reshape(1, 9), motions[-1][1].reshape(1, 3)
    x1 = np.concatenate([synth.pose_matrix(k0 + n - 1)[:3, 3] + [0.03, -0.02, 0.01],
                         Rsc.from_matrix(synth.pose_matrix(k0 + n - 1)[:3, :3]).as_rotvec()])[None]
    lat1 = []
    for it in range(220):
        t1 = time.perf_counter()
        ctx.step((n - 1) % W, 1, dR1, dt1, np.eye(4), 25.0, 10, x1)
        if it >= 20:
            lat1.append((time.perf_counter() - t1) * 1e3)
    # IMU_Mode = 2: the full 15 W-parameter window (IMU factors, prior carried from a first call).  "host": the lidar frames
    # are linearised on the device in one launch per trust-region evaluation and the dense iteration runs on the host
    # (mml_fullwindow_step); "device": the whole iteration is one kernel launch per ceres::Solve (mml_fullwindow_solve)
    fullwin = {}
    errors = []
    for solver, Wf in (("host", 5), ("device", 5), ("host", 8), ("device", 8)):
        try:
            west = odometry.WindowEstimator(ctx, gravity=synth.GRAVITY, solver=solver)
            rng = np.random.default_rng(3)
            t_calls, k_ms = [], []
            for call in range(4):
                frames, pres = [], [None]
                for f in range(Wf):
                    k = k0 + 40 + call + f
                    v, l = make_scan(synth, cfg, k, motion=False)
                    ctx.scan_upload(f, v, l)
                    ctx.extract(f, 1)
                    ctx.downsample(f, 1)
                    Tk = perturbed(synth.pose_matrix(k), dt_=rng.normal(0, 0.02, 3), rv=rng.normal(0, 0.003, 3))
                    q = Rsc.from_matrix(Tk[:3, :3]).as_quat()
                    frames.append(dict(P=Tk[:3, 3].copy(), Q=q if q[3] >= 0 else -q, V=synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                       bg=np.zeros(3), ba=np.zeros(3)))
                    if f > 0:
                        pres.append(M.imu_preintegrate(synth.imu_samples(k - 1, k), np.zeros(3), np.zeros(3)))
                ctx.synchronize()
                timed_kernel = solver == "device" and call == 3      # last call: HIP events around the solve kernel
                if timed_kernel:
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                t1 = time.perf_counter()
                info_w = west.estimate(list(range(Wf)), frames, pres)
                if timed_kernel:
                    ctx.synchronize()
                    fwp = ctx.profile_get().get("fullwindow", (0.0, 0))
                    ctx.profile_enable(False)
                    k_ms = [fwp[0], fwp[1]]
                else:
                    t_calls.append((time.perf_counter() - t1) * 1e3)
            evals = info_w["evaluations"]
            est = float(np.median(t_calls[1:]))
            fullwin["%s_w%d" % (solver, Wf)] = {
                "frames": Wf, "estimate_ms": est, "outer_iterations": info_w["outer"], "evaluations": evals,
                "ms_per_evaluation": est / max(evals, 1),
                "max_pose_err_vs_gt_m": float(max(np.abs(frames[f]["P"] - synth.pose_matrix(k0 + 43 + f)[:3, 3]).max() for f in range(Wf)))}
            if k_ms:
                fullwin["%s_w%d" % (solver, Wf)].update(solve_launches=int(k_ms[1]), solve_device_ms_total=float(k_ms[0]),
                                                        solve_device_ms_per_evaluation=float(k_ms[0]) / max(evals, 1))
        except Exception as e:
            fullwin["%s_w%d" % (solver, Wf)] = {"error": repr(e)[:200]}
            errors.append("full_window_imu %s_w%d: %s" % (solver, Wf, repr(e)[:200]))

    # stage times of the same B = 1 step (HIP events)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(20):
        ctx.step((n - 1) % W, 1, dR1, dt1, np.eye(4), 25.0, 10, x1)
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    stage_ms = {k: v[0] / 20.0 for k, v in prof.items() if v[1] > 0}
    dom = max(stage_ms, key=stage_ms.get)
    info = ctx.scan_info((n - 1) % W)
    nf = len(ctx.features_download((n - 1) % W, 0)) + len(ctx.features_download((n - 1) % W, 1))
    alg = STAGE_BYTES.get(dom, lambda *a: 0)(info.n_velo, info.n_points - info.n_velo, nf, 10)

    # >>> cpu_baseline leg: the same loop through the oracle on one host core, bounded sample
    cpu = None
    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import mml_oracle as O
            O.build()
            lm = O.LocalMap(window=50, leaf_corner=ctx.cfg.leaf_corner, leaf_surf=ctx.cfg.leaf_surf)
            last_update = np.array([-1.0, -1.0, -1.0])
            T_prev = T_prev_gt = None
            t1 = time.perf_counter()
            done = 0
            for i in range(n):
                k = k0 + i
                T_gt = synth.pose_matrix(k)
                Tp = T_gt.copy() if T_prev is None else perturbed(T_prev @ np.linalg.inv(T_prev_gt) @ T_gt)
                ev, el = O.extract_velo(scans[i][0]), O.extract_livox(scans[i][1])
                xyz = np.concatenate([ev["xyzi"][:, :3], el["xyzi"][:, :3]])
                rel = np.concatenate([ev["reltime"], el["reltime"]])
                lab = np.concatenate([ev["label"], el["label"]])
                und = O.undistort(xyz, rel, motions[i][0], motions[i][1])
                cf, sf = O.voxel_downsample(und[lab == 1], 0.4), O.voxel_downsample(und[lab == 2], 0.2)
                Po, Qo = Tp[:3, 3].copy(), Rsc.from_matrix(Tp[:3, :3]).as_quat()
                cmap, smap = lm.get(0), lm.get(1)
                deg = False
                if len(cmap) > 0 and len(smap) > 100:
                    Po, Qo, _, deg, _ = O.estimate_single(cf, sf, cmap, smap, np.eye(4), Po, Qo, 5, 10)
                T = np.eye(4)
                T[:3, :3] = Rsc.from_quat(Qo).as_matrix()
                T[:3, 3] = Po
                if not deg:
                    d = last_update - T[:3, 3]
                    if float(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) >= 0.5:
                        lm.increment(cf, sf, T)
                        last_update = T[:3, 3].copy()
                T_prev, T_prev_gt = T, T_gt
                done += 1
                if time.perf_counter() - t1 > 3 * args.cpu_seconds:
                    break
            t_cpu = time.perf_counter() - t1
            cpu = {"value": done / t_cpu, "unit": "scans/s", "cores": 1, "kind": "port",
                   "sample": "first %d scans of the same replay through the oracle (extract, undistort, down-sample, "
                             "Estimate 5 x 10 incl. the kd-tree rebuilds the reference does on every call, key-scan rule, "
                             "MapIncrementLocal), one host thread of %d, Python glue between the C++ calls; no 8-scan window"
                             % (done, os.cpu_count())}
        except Exception as e:
            cpu = {"error": repr(e)[:300]}
            errors.append("cpu_baseline: " + repr(e)[:200])
    # <<< cpu_baseline leg

    # ---- the same replay from the reference's host language: tools/live_loop.cpp drives the C++ adapter (no Python in the loop) ----
    cpp = None
    if rank == 0 and not args.skip_cpp_loop:
        try:
            cpp = cpp_live_loop(scans, motions, [perturbed(synth.pose_matrix(k0 + i)) for i in range(n)])
        except Exception as e:
            cpp = {"error": repr(e)[:300]}
            errors.append("cpp_adapter_loop: " + repr(e)[:200])

    if rank == 0:
        out = headline()
        out["latency_ms"].update(configs1_step_B1_p50=pctl(lat1, 50), configs1_step_B1_p99=pctl(lat1, 99))
        out.update({
            "latency_ms_cpp_adapter": cpp,
            "full_window_imu": fullwin,
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": alg / (stage_ms[dom] * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": alg / (stage_ms[dom] * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                         "avg_launch_ms": stage_ms[dom], "algorithmic_bytes_per_launch": alg, "scans_per_launch": 1,
                         "timing": "HIP events, 20 one-scan steps", "stage_ms_per_launch": stage_ms,
                         "note": "one scan per launch cannot fill 256 CUs: this mode is bound by launch latency and the serial "
                                 "dependency chain, not by HBM"},
            "cpu_baseline": cpu,
            "errors": errors,
        })
        return json.dumps(out), errors
    return None, errors


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        if args.backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    line, stuck, errors = None, False, []
    try:
        if args.stub_step:
            run_stub(args, rank, world, dist)
        else:
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
            if args.config == 2:
                line, errors = run_replay(args, rank, local_rank, world, dist)
            else:
                line, stuck, errors = run_throughput(args, rank, local_rank, world, dist)
    finally:
        if dist is not None and not stuck:   # (a rank stuck in a collective cannot be torn down cleanly: just leave)
            dist.destroy_process_group()
    if rank == 0 and line is not None:
        # the one JSON line goes LAST: RCCL prints a version banner through C stdio, which sits in that buffer until the
        # process exits when stdout is a file or a pipe -- push it out first
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(line, flush=True)
    if errors and rank == 0:
        print("bench.py: %d section(s) reported an error: %s" % (len(errors), "; ".join(errors)), file=sys.stderr, flush=True)
    if stuck:
        os._exit(3 if (args.strict and errors) else 0)
    if args.strict and errors:
        sys.exit(3)


if __name__ == "__main__":
    main()
