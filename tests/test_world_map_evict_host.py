"""csrc/world_map_evict.h on the host: tests/cpp/world_map_evict_check.cpp, a program of its own, is built with AddressSanitizer
and UndefinedBehaviorSanitizer where no device is visible (as tests/test_world_map_assoc_host.py builds its program), runs
mml_wme_goes and mml_wme_index_box on scripted cases -- indices at lo, lo - 1, hi - 1, hi per axis, boxes at the ends of the
index range, empty boxes, NOBOX, the count rule at and below min_count, metric boxes on voxel faces, with negative coordinates
and past the range -- and prints every case with its inputs.  Every line is compared with tests/world_map_evict_ref.py.  The
library's mml_wm_index_box, which needs no context, is held against the same restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import world_map_evict_ref as E
from conftest import ROOT


@pytest.fixture(scope="module")
def lines(has_gpu, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("world_map_evict") / "world_map_evict_check"
    san = [] if has_gpu else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + san +
                         ["-I", os.path.join(ROOT, "multi-modal-loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "world_map_evict_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    return run.stdout.splitlines()


def _box_case(line):
    words, res = line[2:].split("=")
    f = np.array([int(w, 16) for w in words.split()], np.uint32).view(np.float32)
    return f[0], f[1:4], f[4:7], [int(v) for v in res.split()]


def test_goes_against_the_restatement(lines):
    n, seen = 0, set()
    for line in lines:
        if line[0] != "G":
            continue
        words, res = line[2:].split("=")
        v = [int(w) for w in words.split()]
        r = E.rule(0, v[0], v[1:4], v[4:7], v[7])
        want = bool(E.goes(r, [v[8:11]], [v[11]])[0])
        assert int(res) == int(want), line
        seen.add((v[0], int(res)))
        n += 1
    assert lines[-1].split()[:2] == ["S", str(n)] and n >= 200
    assert seen == {(m, g) for m in (0, 1, 2) for g in (0, 1)}      # every mode both evicts and keeps somewhere


def test_index_box_against_the_restatement(M, lines):
    import ctypes as C
    n, refused, clamped = 0, 0, 0
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for line in lines:
        if line[0] != "B":
            continue
        leaf, lo_xyz, hi_xyz, got = _box_case(line)
        want = E.index_box(leaf, lo_xyz, hi_xyz)
        lo, hi = np.full(3, 7, np.int32), np.full(3, 7, np.int32)
        rc = M.lib().mml_wm_index_box(float(leaf), p(np.ascontiguousarray(lo_xyz)), p(np.ascontiguousarray(hi_xyz)), p(lo), p(hi))
        if want is None:
            assert got == [-1] + [7] * 6, line                 # refused, nothing written
            assert rc == M.MML_ERR_INVALID and lo.tolist() + hi.tolist() == [7] * 6, line
            refused += 1
        else:
            assert got == [0] + want[0].tolist() + want[1].tolist(), (line, want)
            assert rc == M.MML_OK and lo.tolist() + hi.tolist() == got[1:], line
            clamped += max(abs(v) for v in got[1:]) == E.HALF
        n += 1
    assert lines[-1].split()[2] == str(n) and n >= 40 and refused >= 7 and clamped >= 8
    # by hand: a corner on a voxel face belongs to the voxel above it, and hi is one past the corner's voxel
    assert [a.tolist() for a in E.index_box(0.5, (0.0, -0.5, -0.25), (1.0, 0.0, 0.25))] == [[0, -1, -1], [3, 1, 1]]
    lo, hi = M.wm_index_box(0.5, (0.0, -0.5, -0.25), (1.0, 0.0, 0.25))
    assert lo.tolist() == [0, -1, -1] and hi.tolist() == [3, 1, 1]
    with pytest.raises(M.MmlError):
        M.wm_index_box(0.5, (0.0, np.nan, 0.0), (1.0, 1.0, 1.0))
    assert M.lib().mml_wm_index_box(0.5, None, None, None, None) == M.MML_ERR_INVALID


def test_restatement_evict_by_hand():
    ijk = np.array([[0, 0, -1], [1, 0, 0], [5, 0, 0], [0, 0, 1]], np.int32)
    e = dict(ijk=ijk, sums=np.arange(16, dtype=np.float32).reshape(4, 4), counts=np.array([1, 2, 3, 4], np.int32), moments=None)
    other = dict(ijk=ijk[:1], sums=np.zeros((1, 4), np.float32), counts=np.ones(1, np.int32), moments=None)
    left, gone, info = E.evict({0: other, 1: e}, [E.rule(1, E.OUTSIDE, (0, 0, 0), (2, 1, 2), 3)])
    assert left[0] is other and left[1]["counts"].tolist() == [4] and gone[1]["counts"].tolist() == [1, 2, 3]
    assert info == [dict(n_before=4, n_evicted=3, n_kept=1, first_row=0)]
    left, gone, info = E.evict({0: e, 1: e}, [E.rule(1, E.INSIDE, (0, 0, 0), (2, 1, 2)), E.rule(0, E.NOBOX, min_count=2)])
    assert [i["first_row"] for i in info] == [1, 0] and gone[0]["counts"].tolist() == [1] and gone[1]["counts"].tolist() == [2, 4]
    assert E.same(left[0], E.take(e, np.array([1, 2, 3]))) and not E.same(left[0], left[1])
