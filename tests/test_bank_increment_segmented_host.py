"""The segmented bank increment without a device: mml_map_bank_increment_segmented and mml_debug_bank_increment_budget are declared
and exported and refuse a NULL context and null arrays; BatchLidarOdometry hands the choice on; and csrc/grid_cell_rule.h -- the
cell-size decisions that build_grid_into and the segmented grid build both call -- compiled into a stand-alone host program
(tests/cpp/grid_cell_rule_check.cpp) decides what a numpy restatement of build_grid_into's loop decides, on random boxes, on boxes
that exceed the cell budget (the 1.26 growth) and on clouds that stay dense through round 4 (the stop)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["mml_map_bank_increment_segmented", "mml_debug_bank_increment_budget"]


def test_names_declared_and_exported(M):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmloam_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mml_map_bank_increment_segmented\s*\(\s*mml_ctx\s*\*\s*ctx,\s*int n,\s*const int\s*\*\s*banks,\s*const int\s*\*\s*slots,"
                     r"\s*const double\s*\*\s*T_wl,\s*int\s*\*\s*n_corner,\s*int\s*\*\s*n_surf\)", src)
    assert re.search(r"\bint\s+mml_debug_bank_increment_budget\s*\(\s*mml_ctx\s*\*\s*ctx,\s*long points\)", src)
    assert re.search(r"#define\s+MML_BANK_INCREMENT_BUDGET\s+\(1 << 22\)", src)
    for n in NAMES:
        assert hasattr(M.lib(), n), "libmmloam_hip.so does not export %s" % n


def test_null_context_and_null_arrays_are_argument_errors(M):
    L, p = M.lib(), M._p
    one = np.zeros(1, np.int32)
    T = np.eye(4).reshape(1, 16)
    assert L.mml_map_bank_increment_segmented(None, 1, p(one), p(one), p(T), None, None) == M.MML_ERR_INVALID
    assert L.mml_map_bank_increment_segmented(None, 0, None, None, None, None, None) == M.MML_ERR_INVALID
    assert L.mml_map_bank_increment_segmented(None, 2, p(np.zeros(2, np.int32)), None, p(np.tile(T, (2, 1))), None, None) == M.MML_ERR_INVALID
    import ctypes as C
    assert L.mml_debug_bank_increment_budget(None, C.c_long(100)) == M.MML_ERR_INVALID


class _Stub:
    """Records how bank_increment was called; everything else BatchLidarOdometry needs for a first round (empty maps: no Estimate)."""

    def __init__(self):
        self.calls = []

    def map_banks(self, n):
        pass

    def bind_banks(self, first, banks):
        pass

    def scan_info(self, slot):
        import types
        return types.SimpleNamespace(fused_corner_num=200)

    def downsample(self, first, count):
        pass

    def bank_increment(self, *a, **kw):
        self.calls.append((len(a), dict(kw)))
        return np.full(len(a[0]), 100, np.int32), np.full(len(a[0]), 1000, np.int32)


def test_batch_odometry_hands_the_choice_on(M):
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    P, Q = np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    for how, want in (({}, {}), (dict(increment="loop"), {}), (dict(increment="segmented"), dict(segmented=True))):
        ctx = _Stub()
        bat = odometry.BatchLidarOdometry(ctx, 2, **how)
        _, _, grew = bat.estimate_lidar_pose([0, 1], P, Q)
        assert list(grew) == [True, True]
        assert ctx.calls == [(3, want)]               # "loop": the three positional arguments of before and nothing else
    with pytest.raises(ValueError):
        odometry.BatchLidarOdometry(_Stub(), 2, increment="both")


# ---- grid_cell_rule.h against build_grid_into's loop, restated ---------------------------------------------------------------------

F = np.float32


def _loop(bbox, cell, max_cells, m, occ):
    """build_grid_into's `for (int round = 0;; ++round)` on the host values it reads: float arithmetic in float32, as the C code."""
    out = []
    cell = F(cell)
    for rnd in range(6):
        while True:
            dim, total = [], 1
            for c in range(3):
                d = int(np.floor(F(F(bbox[3 + c]) - F(bbox[c])) / cell)) + 1
                d = max(d, 1)
                dim.append(d)
                total *= d
            if total <= max_cells:
                break
            cell = F(cell * F(1.26))
        ncell = dim[0] * dim[1] * dim[2]
        per_cell = float(m) / (occ[rnd] if occ[rnd] > 0 else 1)
        stop = per_cell <= 12.0 or rnd >= 4 or ncell * 8 > max_cells
        out.append("%d %08x %d %d %d %d %d" % (rnd, cell.view(np.uint32), dim[0], dim[1], dim[2], ncell, 0 if stop else 1))
        if stop:
            break
        cell = F(cell * F(0.5))
    out.append("end")
    return out


def _cases():
    rng = np.random.default_rng(11)
    cases = []
    for i in range(400):
        lo = rng.uniform(-80, 80, 3).astype(F)
        ext = (rng.uniform(0, 1, 3) ** 2 * [120, 120, 30]).astype(F)
        if i % 9 == 0:
            ext[rng.integers(3)] = 0                                   # a flat box: one cell along that axis
        hi = (lo + ext).astype(F)
        cell = F(rng.choice([0.05, 0.2, 1.0, 1.6, 2.0, 3.2]))
        max_cells = int(rng.choice([4 * (1 << 10) + 4096, 4 * (1 << 16) + 4096, 4 * (1 << 21) + 4096]))
        m = int(rng.integers(1, 60000))
        kind = i % 4
        if kind == 0:
            occ = [m] * 5                                              # one point per cell: done in round 0
        elif kind == 1:
            occ = [1] * 5                                              # dense for ever: the round-4 stop or the cell budget
        else:
            occ = sorted(int(x) for x in rng.integers(0, m + 1, 5))    # (0: the guard against a division by zero)
        cases.append((np.concatenate([lo, hi]), cell, max_cells, m, occ))
    return cases


def test_cell_rule_equals_the_loop_it_was_factored_from(tmp_path):
    exe = tmp_path / "grid_cell_rule_check"
    csrc = os.path.join(ROOT, "multi-modal-loam_amd", "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", csrc,
                          os.path.join(ROOT, "tests", "cpp", "grid_cell_rule_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    cases = _cases()
    text = "".join("%s %08x %d %d %s\n" % (" ".join("%08x" % v for v in bbox.view(np.uint32)), cell.view(np.uint32), mc, m,
                                          " ".join(str(o) for o in occ)) for bbox, cell, mc, m, occ in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    want = [line for bbox, cell, mc, m, occ in cases for line in _loop(bbox, cell, mc, m, occ)]
    got = run.stdout.split("\n")[:-1]
    assert got == want
    rounds = [len(_loop(*c)) - 1 for c in cases]
    grown = sum(1 for bbox, cell, mc, m, occ in cases if _loop(bbox, cell, mc, m, occ)[0].split()[1] != "%08x" % cell.view(np.uint32))
    assert max(rounds) == 5 and min(rounds) == 1 and grown >= 10      # the round-4 stop and the `total > max_cells` growth were reached
