"""CPU suite for the world map (mml_world_map_*): the stand-alone check of csrc/world_map_key.h, the C-ABI surface -- header,
library and ctypes view carry the same entry points with the same argument counts --, the NULL-context refusals, and the numpy
restatement tests/world_map_ref.py against hand-computed cases.  The device side is tests/test_gpu_world_map.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import world_map_ref as R
from conftest import ROOT

# the six calls of the issue's block; the seventh declaration of that block is the info struct, checked field for field below
CALLS = ("mml_world_map_create", "mml_world_map_destroy", "mml_world_map_reset", "mml_world_map_add", "mml_world_map_size",
         "mml_world_map_download")
INFO_FIELDS = ["n_points", "n_kept", "n_nonfinite", "n_out_of_range", "n_masked", "n_new_voxels", "n_voxels_total"]


def test_key_arithmetic_stand_alone(has_gpu, tmp_path):
    """tests/cpp/world_map_key_check.cpp includes only world_map_key.h; a host program of its own, under AddressSanitizer and
    UndefinedBehaviorSanitizer where no device is visible (sanitizer builds stay on the CPU machines), plain otherwise."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "world_map_key_check"
    san = [] if has_gpu else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + san +
                         ["-I", os.path.join(ROOT, "multi-modal-loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "world_map_key_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert run.stdout == "world_map_key_check ok\n"


def _header():
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_library_and_ctypes_view_agree(M):
    src = _header()
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = M.lib()
    assert set(M.WORLD_MAP_ARGTYPES) == set(CALLS)
    for name in CALLS:
        decl = re.findall(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert len(decl) == 1, name
        n_args = len([a for a in decl[0].split(",") if a.strip()])
        assert name in exported, name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args == len(M.WORLD_MAP_ARGTYPES[name]), name
    assert [len(M.WORLD_MAP_ARGTYPES[n]) for n in CALLS] == [4, 1, 2, 7, 3, 6]
    # the info struct: seven longs, in the header's order
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mml_world_map_info\s*;", src).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "long " + ", ".join(INFO_FIELDS) + ";"
    assert [f[0] for f in M.WorldMapInfo._fields_] == INFO_FIELDS and C.sizeof(M.WorldMapInfo) == 7 * C.sizeof(C.c_long)
    for name in ("world_map_create", "world_map_add", "world_map_download", "world_map_size", "world_map_reset"):
        assert callable(getattr(M.Context, name)), name


def test_null_context_is_invalid(M):
    L = M.lib()
    n = C.c_long(-7)
    T = np.eye(4).reshape(1, 16)
    m = np.zeros(1, np.int32)
    assert L.mml_world_map_create(None, 1, 0.2, 16) == M.MML_ERR_INVALID
    assert L.mml_world_map_destroy(None) == M.MML_ERR_INVALID
    assert L.mml_world_map_reset(None, -1) == M.MML_ERR_INVALID
    assert L.mml_world_map_add(None, 0, 1, m.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p), 7, None) == M.MML_ERR_INVALID
    assert L.mml_world_map_size(None, 0, C.byref(n)) == M.MML_ERR_INVALID
    assert L.mml_world_map_download(None, 0, None, None, 0, C.byref(n)) == M.MML_ERR_INVALID
    assert n.value == -7


def test_restatement_two_points_in_one_voxel_both_orders():
    """Float32 steps are 8 wide at 1e8, so the order in which a voxel's points reach its STORED sum decides the result (all
    points share voxel (0, 0, 0); the arithmetic is shown on the intensity sum, which takes any sign).  Hand-computed:
      case 1  stored 1e8, then 5 and -1e8:  (1e8 + 5 = 100000008) - 1e8 = 8   against   (1e8 - 1e8 = 0) + 5 = 5
      case 2  from zero, 1e8, 5, 5:  100000008, then + 5 = 100000013 -> 100000016   against   5, 5, 1e8:  10 + 1e8 -> 100000008
      case 3  two points from an EMPTY voxel: 0 + a is exact and a + b = b + a, the same sum in both orders."""
    f = np.float32
    leaf = 4.0
    key = R.pack(0, 0, 0, 0)
    big, five, neg = [1.0, 1.0, 1.0, 1.0e8], [1.0, 1.0, 1.0, 5.0], [1.0, 1.0, 1.0, -1.0e8]
    r1, r2 = R.WorldMapRef(leaf), R.WorldMapRef(leaf)
    for r, order in ((r1, [five, neg]), (r2, [neg, five])):
        r.add_world(0, [big])          # one call stores the sum ...
        r.add_world(0, order)          # ... the next adds two points to it, one after the other
    assert r1.vox[key][0].tolist() == [3.0, 3.0, 3.0, 8.0] and r2.vox[key][0].tolist() == [3.0, 3.0, 3.0, 5.0]
    assert r1.vox[key][1] == r2.vox[key][1] == 3
    assert r1.download(0)[0][0, 3] == f(8.0) / f(3.0) and r2.download(0)[0][0, 3] == f(5.0) / f(3.0)
    r3, r4 = R.WorldMapRef(leaf), R.WorldMapRef(leaf)
    r3.add_world(0, [big, five, five])
    r4.add_world(0, [five, five, big])
    assert r3.vox[key][0][3] == f(100000016.0) and r4.vox[key][0][3] == f(100000008.0)
    r5, r6 = R.WorldMapRef(leaf), R.WorldMapRef(leaf)
    r5.add_world(0, [big, five])
    r6.add_world(0, [five, big])
    assert r5.vox[key][0][3] == r6.vox[key][0][3] == f(100000008.0)
    assert r5.info == dict(n_points=2, n_kept=2, n_nonfinite=0, n_out_of_range=0, n_masked=0, n_new_voxels=1)


def test_restatement_voxel_edges_and_key():
    f = np.float32
    inv = R.inv_leaf(0.25)
    assert inv == f(4.0)
    assert R.axis_index(f(-0.0), inv) == 0 and R.axis_index(f(-0.25), inv) == -1
    assert R.axis_index(np.nextafter(f(0), f(-1)), inv) == -1
    assert R.axis_index(f(32767.75), inv) == R.HALF - 1 and R.axis_index(f(32768.0), inv) is None
    assert R.axis_index(f(-32768.0), inv) == -R.HALF and R.axis_index(np.nextafter(f(-32768.0), f(-1e9)), inv) is None
    assert R.pack(0, -R.HALF, -R.HALF, -R.HALF) == 0 and R.pack(1023, R.HALF - 1, R.HALF - 1, R.HALF - 1) == R.EMPTY
    assert R.unpack(R.pack(5, -3, 7, -11)) == (5, -3, 7, -11)
    assert R.pack(2, 1 - R.HALF, 2 - R.HALF, 3 - R.HALF) == (2 << 54) | (3 << 36) | (2 << 18) | 1
    r = R.WorldMapRef(0.25)
    hi = 32767.75
    pts = [[0, 0, 0, 1], [np.nan, 0, 0, 1], [0, 0, 0, np.inf], [32768.0, 0, 0, 1], [0.1, 0.1, 0.1, 3]]
    r.add_world(1, pts, labels=[0, 1, 2, 0, 1], label_mask=7)
    r.add_world(1, [[0.2, 0.2, 0.2, 5]], labels=[2], label_mask=3)      # masked
    r.add_world(1023, [[hi, hi, hi, 1]])                                 # the empty marker's voxel: out of range
    assert r.info == dict(n_points=7, n_kept=2, n_nonfinite=2, n_out_of_range=2, n_masked=1, n_new_voxels=1)
    c, n = r.download(1)
    assert n.tolist() == [2] and c[0].tolist() == [f(0.1) / f(2), f(0.1) / f(2), f(0.1) / f(2), f(2.0)]
    assert r.size(0) == 0 and r.size(1) == 1 and r.size() == 1


def test_restatement_world_point_and_hash():
    T = np.array([[1.5, 0.25, -0.125, 4.0], [0.0, -0.75, 2.0, -3.0], [0.3, 0.3, 0.3, 0.1], [9, 9, 9, 9]])
    w = R.world_points([[1.0, 2.0, 4.0]], T)
    assert w.tolist() == [[np.float32(1.5 + 0.5 - 0.5 + 4.0), np.float32(-1.5 + 8.0 - 3.0), np.float32(((0.3 * 1.0 + 0.3 * 2.0) + 0.3 * 4.0) + 0.1)]]
    assert R.table_slots(1) == 2 and R.table_slots(4) == 8 and R.table_slots(64) == 128
    assert all(R.hash_position(k, 2) < 2 and R.hash_position(k, 1 << 20) < (1 << 20) for k in (0, 1, R.EMPTY - 1, 12345678901234567))
