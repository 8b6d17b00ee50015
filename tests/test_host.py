"""CPU suite, product side: the C-ABI library loads and exports what include/mmloam_hip.h declares, refuses to
run without a device (no CPU fallback), and the host-only joint window solver (the multi-GPU exchange step)
agrees with the oracle -- single process and across 2 gloo ranks."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, perturbed, pose_to_x


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(mml_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol(M):
    lib = M.lib()
    names = _declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libmmloam_hip.so does not export %s" % n
    assert lib.mml_abi_version() == 1


def test_struct_layouts_match_header(M):
    # sizes the ctypes mirrors must agree with (checked against the C compiler)
    code = textwrap.dedent("""
        #include <stdio.h>
        #include "mmloam_hip.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mml_config), sizeof(mml_scan_info), sizeof(mml_assoc_stats),
                 sizeof(mml_solve_opts), sizeof(mml_solve_summary), sizeof(mml_estimate_info), sizeof(mml_profile),
                 sizeof(mml_livox_point), sizeof(mml_window_timing), sizeof(mml_gicp_info), sizeof(mml_imu_preint), sizeof(mml_prior));
          return 0; }""")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    mine = [C.sizeof(M.Config), C.sizeof(M.ScanInfo), C.sizeof(M.AssocStats), C.sizeof(M.SolveOpts),
            C.sizeof(M.SolveSummary), C.sizeof(M.EstimateInfo), C.sizeof(M.Profile), M.LIVOX_DTYPE.itemsize,
            C.sizeof(M.WindowTiming), C.sizeof(M.GicpInfo), C.sizeof(M.ImuPreint), C.sizeof(M.Prior)]
    assert sizes == mine


def test_no_device_is_a_loud_error(M, has_gpu):
    if has_gpu:
        pytest.skip("a GPU is present")
    with pytest.raises(M.MmlError) as e:
        M.Context(max_scans=1)
    assert e.value.code == M.MML_ERR_NO_DEVICE


def test_phase_clock_reader_of_a_default_build(M):
    # The shipped library carries no phase clocks (csrc/phase_clock.h): the reader knows the seven families by name, says of each that
    # it was not built in, and says so -- as for a name that is no family -- before any HIP call and without touching out.
    families = ["op", "st", "sel", "sp", "vx", "sv", "svw"]
    assert M.PHASE_CLOCKS_UNKNOWN < 0 and M.PHASE_CLOCKS_NOT_BUILT < 0 and M.PHASE_CLOCKS_UNKNOWN != M.PHASE_CLOCKS_NOT_BUILT
    out = (C.c_ulonglong * 64)(*range(1000, 1064))
    for fam in families:
        for reset in (False, True):
            assert M.phase_clocks(fam, out, reset) == M.PHASE_CLOCKS_NOT_BUILT, fam
    for name in ("", "fw", "OP", "svww", "o"):
        for reset in (False, True):
            assert M.phase_clocks(name, out, reset) == M.PHASE_CLOCKS_UNKNOWN, name
    assert M.lib().mml_debug_phase_clocks(None, out, 64, 0) == M.PHASE_CLOCKS_UNKNOWN
    assert list(out) == list(range(1000, 1064))


def test_cpp_adapter_compiles_links_and_runs_host_side(M, tmp_path):
    """multi-modal-loam_amd/host/mmloam_adapter.hpp (the reference-language mirror of feature_extraction / Estimator)
    builds against include/mmloam_hip.h and the shared library; the IMU pre-integration it forwards to needs no
    device, and creating a context without one is the documented loud error."""
    src = tmp_path / "adapter_probe.cpp"
    src.write_text(textwrap.dedent(r"""
        #include <cstdio>
        #include "mmloam_adapter.hpp"
        int main() {
            double smp[7 * 20];
            for (int i = 0; i < 20; ++i) { double* m = smp + 7 * i; m[0] = 0; m[1] = 0; m[2] = 0.2; m[3] = 0; m[4] = 0.01; m[5] = 1.0; m[6] = 0.005; }
            const double z[3] = {0, 0, 0};
            mml_imu_preint pre;
            if (mml_imu_preintegrate(smp, 20, z, z, &pre) != MML_OK) return 2;
            std::printf("dtime %.3f dv_z %.4f\n", pre.dtime, pre.dv[2]);
            try {
                mml::Context ctx(1, 0);
                mml::Estimator est(ctx, 0.4f, 0.2f);
                const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, l[12] = {0.1f, 0, 0, 0.9f, 0, 0, 0, 0.8f, 0, 1, 1, 0};
                mml::TimeOffsetResult r = mml::EstimateTimeOffsetCore(ctx, v, 3, nullptr, l, 4, 1, 2);
                std::printf("context ok, %d windows, best %d\n", r.n_windows, r.best_window);
            } catch (const std::exception& e) {
                std::printf("no device: %s\n", e.what());
            }
            return 0;
        }"""))
    exe = tmp_path / "adapter_probe"
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"), str(src), "-o", str(exe),
           "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dtime 0.100" in run.stdout and ("no device" in run.stdout or "context ok" in run.stdout)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "multi-modal-loam_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "mml_oracle" not in txt and "oracle/" not in txt.replace("oracle/linalg.h", "").replace(
                    "oracle/estimate.cpp", ""), "%s references the oracle" % f
    # the developer tools measure and summarise the product only
    for f in os.listdir(os.path.join(ROOT, "tools")):
        if f.endswith(".py"):
            assert "mml_oracle" not in open(os.path.join(ROOT, "tools", f)).read(), "tools/%s imports the oracle" % f
    # bench.py: code that names the oracle (a string with the directory / library name, the module name) lives only inside
    # the regions marked as the cpu_baseline leg; doc strings and comments may talk about it
    import ast
    import io
    import tokenize
    src = open(os.path.join(ROOT, "bench.py")).read()
    lines = src.split("\n")
    regions, start = [], None
    for k, ln in enumerate(lines, 1):
        if ln.strip().startswith("# >>> cpu_baseline leg"):
            start = k
        elif ln.strip().startswith("# <<< cpu_baseline leg"):
            regions.append((start, k))
            start = None
    assert regions and start is None
    doc_lines = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.FunctionDef, ast.ClassDef)) and ast.get_docstring(node, clean=False) is not None:
            d = node.body[0]
            doc_lines.update(range(d.lineno, d.end_lineno + 1))
    hits = 0
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        named = (tok.type == tokenize.NAME and tok.string == "mml_oracle") or \
                (tok.type == tokenize.STRING and ("oracle" in tok.string) and tok.start[0] not in doc_lines)
        if named:
            hits += 1
            assert any(a <= tok.start[0] <= b for a, b in regions), "bench.py line %d names the oracle outside the cpu_baseline leg" % tok.start[0]
    assert hits >= 2


def test_bench_spawns_ranks_itself(tmp_path):
    """`python bench.py --gpus 2` started bare launches two ranks (RANK / WORLD_SIZE / MASTER_*), they rendezvous (gloo
    here, no device: --stub-step), the slowest rank sets the clock and rank 0 prints ONE line with n_gpus = 2."""
    import json
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1",
                          "--backend", "gloo", "--stub-step"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1, out.stdout
    r = json.loads(js[0])
    assert r["n_gpus"] == 2 and r["steps"] == 5 and r["scaling"] == "weak"
    assert r["ms_per_step"] >= 4.0          # rank 1 sleeps 4 ms per step: max over ranks, not rank 0's own 2 ms
    # the same entry point under an external launcher (the driver's way) must not spawn again
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--backend", "gloo", "--stub-step"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1 and json.loads(js[0])["n_gpus"] == 2


def _frame_problem(O, scene, k, thres=1.0):
    fr = scene["frames"][k]
    T = perturbed(fr["T_gt"])
    tc, ts = O.KdTree(scene["corner_map"]), O.KdTree(scene["surf_map"])
    lf, _ = O.associate_lines(fr["corner"], tc, T, thres)
    pf, _ = O.associate_planes(fr["surf"], ts, T, thres)
    return lf, pf, pose_to_x(T)


def _run_window(M, O, lfs, pfs, x0, w_tan, huber, max_iters=10, fixed=False):
    W = len(lfs)
    ws = M.WindowSolver(W, max_iters=max_iters, fixed=fixed, huber=huber, w_tan=w_tan)
    x = np.array(x0, dtype=np.float64).reshape(W, 6)
    n_lin = 0
    while True:
        recs = []
        for f in range(W):
            H, g, c = O.linearize(lfs[f], pfs[f], x[f], np.eye(4), w_tan, huber)
            recs.append(M.pack_record(H, g, c))
        n_lin += 1
        done, x = ws.step(np.stack(recs), x)
        if done:
            break
        assert n_lin < 200
    return x, ws.summary(), n_lin


@pytest.mark.parametrize("W,w_tan,huber", [(1, 0.0, 0.1 / 1.5e-3), (2, 3e-4, 0.0), (4, 3e-4, 0.0)])
def test_window_solver_matches_oracle(M, O, scene, W, w_tan, huber):
    probs = [_frame_problem(O, scene, k) for k in range(W)]
    lfs, pfs = [p[0] for p in probs], [p[1] for p in probs]
    x0 = np.stack([p[2] for p in probs])
    xo, so, _ = O.solve_window(lfs, pfs, x0, np.eye(4), 10, huber=huber, w_tan=w_tan)
    xw, sw, n_lin = _run_window(M, O, lfs, pfs, x0, w_tan, huber)
    assert sw.iterations == so["iterations"] and sw.successful == so["successful"] and sw.termination == so["termination"]
    assert np.abs(xw - xo).max() < 1e-9  # pose bar is 1e-4 m / 1e-4 rad
    assert np.isclose(sw.final_cost, so["final_cost"], rtol=1e-9)
    assert n_lin == so["iterations"] + 1 or so["termination"] != 0


def test_window_solver_fixed_iterations(M, O, scene):
    lf, pf, x0 = _frame_problem(O, scene, 0)
    xo, so, _ = O.solve_window([lf], [pf], x0[None], np.eye(4), 10, fixed=True)
    xw, sw, _ = _run_window(M, O, [lf], [pf], x0[None], 0.0, 0.1 / 1.5e-3, fixed=True)
    assert sw.iterations == 10 == so["iterations"]
    assert np.abs(xw - xo).max() < 1e-9


_GLOO_WORKER = r'''
import importlib, os, sys
import numpy as np
import torch
import torch.distributed as dist
ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import mml_oracle as O
from conftest import perturbed, pose_to_x
M = importlib.import_module("multi-modal-loam_amd")
synth = importlib.import_module("multi-modal-loam_amd.synth")
dist.init_process_group("gloo")
rank, W = dist.get_rank(), dist.get_world_size()
# every rank builds the same (small) replicated map, then owns ONE frame of the window
cm, sm = [], []
for k in range(3):
    ev, el = O.extract_velo(synth.velo_scan(k, n_az=450)), O.extract_livox(synth.livox_scan(k, n=6000))
    p = np.concatenate([ev["xyzi"][:, :3], el["xyzi"][:, :3]]); lb = np.concatenate([ev["label"], el["label"]])
    T = synth.pose_matrix(k)
    cm.append(synth.transform(T, O.voxel_downsample(p[lb == 1], 0.4).astype(np.float64)).astype(np.float32))
    sm.append(synth.transform(T, O.voxel_downsample(p[lb == 2], 0.2).astype(np.float64)).astype(np.float32))
cm = O.voxel_downsample(np.concatenate(cm), 0.4); sm = O.voxel_downsample(np.concatenate(sm), 0.2)
tc, ts = O.KdTree(cm), O.KdTree(sm)
def frame(k):
    ev, el = O.extract_velo(synth.velo_scan(k, n_az=450)), O.extract_livox(synth.livox_scan(k, n=6000))
    p = np.concatenate([ev["xyzi"][:, :3], el["xyzi"][:, :3]]); lb = np.concatenate([ev["label"], el["label"]])
    T = perturbed(synth.pose_matrix(k))
    lf, _ = O.associate_lines(O.voxel_downsample(p[lb == 1], 0.4), tc, T, 1.0)
    pf, _ = O.associate_planes(O.voxel_downsample(p[lb == 2], 0.2), ts, T, 1.0)
    return lf, pf, pose_to_x(T)
lf, pf, x_mine = frame(4 + rank)
xs = [torch.zeros(6, dtype=torch.float64) for _ in range(W)]
dist.all_gather(xs, torch.from_numpy(x_mine))
x = np.stack([t.numpy() for t in xs])
ws = M.WindowSolver(W, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4)
while True:
    H, g, c = O.linearize(lf, pf, x[rank], np.eye(4), 3e-4, 0.0)      # per-frame normal equations on "this GPU"
    rec = torch.from_numpy(M.pack_record(H, g, c))
    out = [torch.zeros(32, dtype=torch.float64) for _ in range(W)]
    dist.all_gather(out, rec)                                          # the 32-double-per-frame exchange step
    done, x = ws.step(np.stack([t.numpy() for t in out]), x)           # every rank solves the joint system redundantly
    if done:
        break
# all ranks agree bit for bit, and rank 0 checks against the oracle's joint solve
chk = [torch.zeros(6 * W, dtype=torch.float64) for _ in range(W)]
dist.all_gather(chk, torch.from_numpy(x.reshape(-1).copy()))
assert all(torch.equal(chk[0], c) for c in chk)
if rank == 0:
    fr = [frame(4 + r) for r in range(W)]
    xo, so, _ = O.solve_window([f[0] for f in fr], [f[1] for f in fr], np.stack([f[2] for f in fr]), np.eye(4), 10, huber=0.0, w_tan=3e-4)
    s = ws.summary()
    assert np.abs(xo - x).max() < 1e-9, np.abs(xo - x).max()
    assert s.iterations == so["iterations"] and s.termination == so["termination"]
    print("GLOO_WINDOW_OK", s.iterations)
dist.destroy_process_group()
'''


def test_window_solve_two_ranks_gloo(tmp_path):
    """world_size 2, gloo: one frame per rank, all-gather of the 32-double records every iteration."""
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29541", str(script), ROOT],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "GLOO_WINDOW_OK" in out.stdout


_ORDER_PROBE = r'''
import importlib, sys
sys.path.insert(0, sys.argv[1])
if sys.argv[2] == "torch_first":
    import torch
M = importlib.import_module("multi-modal-loam_amd")
M.lib()
if sys.argv[2] == "package_first":
    import torch
r = M.rccl_libraries()
hip = sorted(set(l.split()[5] for l in open("/proc/self/maps") if len(l.split()) >= 6 and "libamdhip64" in l.split()[5]))
print("PROBE", len(r["loaded"]), len(hip), r["version"])
'''


@pytest.mark.parametrize("order", ["torch_first", "package_first"])
def test_one_hip_runtime_and_one_rccl_whatever_the_import_order(tmp_path, order):
    """libmmloam_hip.so (RCCL inside the C-ABI) and torch.distributed must drive the SAME RCCL on the SAME HIP runtime; the
    package maps the PyTorch wheel's copies before its own library whichever is imported first (and the process must still exit
    cleanly: RCCL's symbols in the global scope ahead of torch's libraries end in a double free at exit)."""
    script = tmp_path / "probe.py"
    script.write_text(_ORDER_PROBE)
    out = subprocess.run([sys.executable, str(script), ROOT, order], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    probe = [ln for ln in out.stdout.splitlines() if ln.startswith("PROBE")][0].split()
    assert probe[1] == "1" and probe[2] == "1", out.stdout
    assert int(probe[3]) >= 20000


def _libm_check(tmp_path, include_dir, ns, f1, f2, pairs=400_000_000):
    """Compile tests/cpp/libm_f32_check.cpp around one libm_f32.h and run it: atanf on all 2^32 arguments and atan2f on `pairs`
    pairs against this machine's libm, bit for bit."""
    exe = tmp_path / "libm_f32_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", '-DIMPL_HEADER="libm_f32.h"', "-DIMPL_NS=" + ns, "-DIMPL_ATAN=" + f1,
                    "-DIMPL_ATAN2=" + f2, "-I", include_dir, os.path.join(ROOT, "tests", "cpp", "libm_f32_check.cpp"), "-o", str(exe), "-lpthread"],
                   check=True)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    out = subprocess.run([str(exe), str(pairs), str(threads)], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "atanf 0" in out.stdout and "atan2f 0" in out.stdout, out.stdout[-2000:]


def test_libm_f32_equals_glibc(tmp_path):
    """csrc/libm_f32.h (host and device source; the bucketing kernels' azimuth and ring pitch) computes the bits of glibc's atanf /
    atan2f -- the float overloads unionFeatureExtract.cpp:1136-1139,1159,1168 resolve to (convention 4).
    Compiled for the host and compared with THIS image's libm (2.35: the same fdlibm float routines as melodic's 2.27) on all 2^32
    arguments of atanf and 4e8 pairs of atan2f (random patterns, lidar-like coordinates, ratios on the reduction thresholds,
    zeros / denormals / infinities)."""
    _libm_check(tmp_path, os.path.join(ROOT, "multi-modal-loam_amd", "csrc"), "mml_libm", "atanf_fd", "atan2f_fd")


def test_live_loop_builds_against_the_library(tmp_path):
    """tools/live_loop.cpp (the configs[2] replay driven through the C++ adapter: bench.py --config 2 builds and runs it on the GPU
    box) compiles and links against the in-tree library and the adapter header as they are now; without a scene file it exits 2."""
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    exe = tmp_path / "live_loop"
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                          os.path.join(ROOT, "tools", "live_loop.cpp"), "-o", str(exe), "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir,
                          "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "warning" not in out.stderr, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2
