"""CPU suite for surfel maps (mml_world_map_create_opts, _download_moments, _download_surfels): the stand-alone program over
csrc/world_map_key.h against the numpy restatement tests/world_map_surfel_ref.py, bit for bit; the restatement against cases
whose every operation is exact (dyadic coordinates, leaf 0.25), with no tolerance; the C-ABI surface of the three new calls.
The device side is tests/test_gpu_world_map_surfel.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

import world_map_ref as R
import world_map_surfel_ref as S
from conftest import ROOT

CALLS = ("mml_world_map_create_opts", "mml_world_map_download_moments", "mml_world_map_download_surfels")
LEAF = 0.25
I4 = np.eye(4)


@pytest.fixture(autouse=True)
def surfel_build(M):
    """every test of this file is about a library that has surfel maps"""
    assert all(hasattr(M.lib(), name) for name in CALLS)


def _slots():
    """(map, pose, (n, 4) float32 x y z intensity): a few thousand random points, tens per voxel, under the identity and under a
    rotation with a translation that is no float; negative indices, and the indices -2^17 and 2^17 - 1 on every axis"""
    rng = np.random.default_rng(21)
    f = np.float32
    G = np.eye(4)
    G[:3, :3] = Rsc.from_rotvec([0.3, -0.2, 0.9]).as_matrix()
    G[:3, 3] = [12.5000001, -7.25, 3.1]
    lo, hi = f(-R.HALF * LEAF), f((R.HALF - 1) * LEAF)
    edge = []
    for axis in range(3):
        for v in (lo, lo + f(0.01), hi, hi + f(0.2), f(-0.01), f(-LEAF)):
            for rep in range(4):
                p = [f(0.3) + f(0.01) * rep, f(-0.3), f(0.1)]
                p[axis] = v + f(0.003) * rep
                edge.append(p + [f(1.0) + rep])
    cloud = lambda n, span: np.concatenate([(rng.random((n, 3), np.float32) - f(0.5)) * f(span), rng.random((n, 1), np.float32) * f(100)], 1)
    return [(0, I4, cloud(1500, 0.7)), (1, G, cloud(1200, 0.6)), (0, G, cloud(800, 0.6)), (0, I4, np.array(edge, np.float32)),
            (1, I4, cloud(700, 0.7))]


def test_moments_arithmetic_stand_alone(has_gpu, tmp_path):
    """tests/cpp/world_map_moments_check.cpp includes only world_map_key.h; a host program of its own, under AddressSanitizer and
    UndefinedBehaviorSanitizer where no device is visible, plain otherwise.  Its accumulators (float bits) and the six covariance
    inputs (hexadecimal doubles) of every voxel equal the numpy restatement's bit for bit."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "world_map_moments_check"
    san = [] if has_gpu else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + san +
                         ["-I", os.path.join(ROOT, "multi-modal-loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "world_map_moments_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    slots = _slots()
    ref = S.SurfelMapRef(LEAF)
    words = [float(np.float32(LEAF)).hex(), str(len(slots))]
    for m, T, pts in slots:
        words += [str(m), str(len(pts))] + [float(v).hex() for v in np.asarray(T, np.float64).reshape(16)] + [float(v).hex() for v in pts.reshape(-1)]
        ref.add(m, pts[:, :3], pts[:, 3], T)
    inp = tmp_path / "points.txt"
    inp.write_text("\n".join(words) + "\n")
    run = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    got = [ln.split() for ln in run.stdout.splitlines()]
    keys = sorted(ref.vox)
    assert [int(g[0]) for g in got] == keys and len(keys) > 100
    idx = {v for k in keys for v in R.unpack(k)[1:]}
    assert -R.HALF in idx and R.HALF - 1 in idx and -1 in idx and ref.info["n_out_of_range"] == 0
    assert max(ref.vox[k][1] for k in keys) >= 20
    mom = np.stack([ref.mom[k] for k in keys])
    cnt = np.array([ref.vox[k][1] for k in keys])
    cov = S.covariance(mom, cnt)
    for r, g in enumerate(got):
        assert int(g[1]) == cnt[r]
        assert [int(w, 16) for w in g[2:14]] == mom[r].view(np.uint32).tolist(), (r, g)
        assert [float.fromhex(w).hex() for w in g[14:20]] == [float(c).hex() for c in cov[r]], (r, g)


def test_restatement_cumsum_equals_scalar_adds():
    """add_world adds a voxel's points with one float32 cumsum; add_point is the same adds with np.float32 scalars, one operation
    after the other.  Order-sensitive values: both give the same bits, the reversed order does not."""
    rng = np.random.default_rng(4)
    w = (np.float32(3.0) + rng.random((200, 3), np.float32) * np.float32(0.24)).astype(np.float32)
    o = np.array([1.0e4, -2.0e4, 30.0], np.float32)
    ref = S.SurfelMapRef(LEAF)
    ref.add_world(0, np.concatenate([w, np.ones((200, 1), np.float32)], 1), o=o)
    (key, m), = ref.mom.items()
    c = [S.centre(i, LEAF) for i in R.unpack(key)[1:]]
    assert c == [np.float32(3.125)] * 3
    a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
    for p in w:
        S.add_point(a, p, c, o)
    for p in w[::-1]:
        S.add_point(b, p, c, o)
    assert a.tobytes() == m.tobytes() and b.tobytes() != m.tobytes()


def _plane_points(z):
    """four points of voxel (2, 3, 4) at leaf 0.25 (centre 0.625, 0.875, 1.125) on the plane z: every operation exact"""
    return np.array([[0.625 + 0.0625, 0.875, z, 1], [0.625 - 0.0625, 0.875, z, 1], [0.625, 0.875 + 0.0625, z, 1], [0.625, 0.875 - 0.0625, z, 1]], np.float32)


def test_exact_plane_normal_sign_and_zero_dot(O):
    z = 1.0625
    rows = {}
    for name, oz in (("above", 5.0), ("below", -5.0), ("inside", z)):
        ref = S.SurfelMapRef(LEAF)
        ref.add_world(0, _plane_points(z), o=(0.625, 0.875, oz))
        mom, cnt = ref.moments(0)
        assert cnt.tolist() == [4]
        # sd = (0, 0, 4 * -1/16), sxx = syy = 2/256, szz = 4/256, no mixed product; the view sum is 4 * (oz - z) along z alone
        assert mom[0].tolist() == [0.0, 0.0, -0.25, 0.0, 2 / 256, 0.0, 0.0, 0.0, 2 / 256, 0.0, 4 / 256, 4 * (oz - z)]
        assert S.covariance(mom, cnt)[0].tolist() == [1 / 512, 0.0, 1 / 512, 0.0, 0.0, 0.0]
        rows[name] = ref.surfels(O, 0)[0]
    assert rows["above"].tolist() == [0.0, 0.0, 1.0, 0.0, 1 / 512, 1 / 512, 1.0, 0.0]                 # l0 == 0 exactly, planarity 1
    assert rows["below"][:3].tolist() == [0.0, 0.0, -1.0] and rows["below"][3:].tolist() == rows["above"][3:].tolist()
    # a dot of exactly 0 keeps the solver's vector, signs of the zeros included
    assert rows["inside"].tobytes() == rows["above"].tobytes()
    assert np.signbit(rows["below"][:2]).all() and not np.signbit(rows["above"][:3]).any()


def test_exact_two_points_and_coincident_points(O):
    ref = S.SurfelMapRef(LEAF)
    ref.add_world(0, _plane_points(1.0625)[:2], o=(0, 0, 9))
    ref.add_world(1, np.repeat(np.array([[0.6875, 0.875, 1.0625, 1]], np.float32), 3, axis=0), o=(0, 0, 9))
    assert ref.moments(0)[1].tolist() == [2] and ref.moments(0)[0].any()
    assert ref.surfels(O, 0).tolist() == [[0.0] * 8]                                                     # n = 2: eight zeros
    mom, cnt = ref.moments(1)
    assert cnt.tolist() == [3] and S.covariance(mom, cnt)[0].tolist() == [0.0] * 6                       # 3 d^2 / 3 - d^2, exact
    s = ref.surfels(O, 1)[0]
    assert s[3:].tolist() == [0.0] * 5 and np.abs(s[:3]).tolist() == [1.0, 0.0, 0.0]                      # ev2 == 0: both ratios 0


def _header():
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_library_and_ctypes_view_agree(M):
    src = _header()
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = M.lib()
    assert set(M.WORLD_MAP_SURFEL_ARGTYPES) == set(CALLS)
    for name in CALLS:
        decl = re.findall(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert len(decl) == 1, name
        n_args = len([a for a in decl[0].split(",") if a.strip()])
        assert name in exported, name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args == len(M.WORLD_MAP_SURFEL_ARGTYPES[name]) == 5, name
    assert re.search(r"#define\s+MML_WM_SURFELS\s+1u\b", src) and M.MML_WM_SURFELS == 1
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", src) and L.mml_abi_version() == 1
    for name in ("world_map_moments", "world_map_surfels"):
        assert callable(getattr(M.Context, name)), name
    odometry = __import__("importlib").import_module("multi-modal-loam_amd.odometry")
    assert callable(odometry.LidarOdometry.world_map_surfels) and callable(odometry.BatchLidarOdometry.world_map_surfels)


def test_null_context_is_invalid(M):
    L = M.lib()
    n = C.c_long(-7)
    out = np.zeros(12, np.float32)
    assert L.mml_world_map_create_opts(None, 1, 0.2, 16, M.MML_WM_SURFELS) == M.MML_ERR_INVALID
    assert L.mml_world_map_create_opts(None, 1, 0.2, 16, 0) == M.MML_ERR_INVALID
    assert L.mml_world_map_download_moments(None, 0, None, 0, C.byref(n)) == M.MML_ERR_INVALID
    assert L.mml_world_map_download_surfels(None, 0, out.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == M.MML_ERR_INVALID
    assert n.value == -7 and not out.any()
