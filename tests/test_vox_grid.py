"""csrc/voxel_sort_dev.h, the one definition of the voxel filters' arithmetic: a stand-alone host program
(tests/cpp/vox_grid_check.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own.  The
order-preserving float key is strictly monotone from -inf over -0.f / +0.f to +inf and its inverse returns every bit;
MML_BBOX_EMPTY decodes to +inf / -inf; MmlVoxGrid::make / index agree with PCL 1.8.1's rules, worked out in the program in plain
integer and double code, on a single point, on either side of a voxel face at negative coordinates, around the int32 overflow
rule (2^31 - 2 voxels, one voxel more along x, 2^31), on a box with max == min and on scattered clouds.  The header's arithmetic
needs no device; like the parameter block's program this one runs where none is visible, so that sanitizer builds stay on the CPU
machines."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vox_grid_arithmetic_under_sanitizers(has_gpu, tmp_path):
    if has_gpu:
        pytest.skip("a device is visible: sanitizer builds run on the CPU machines")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "vox_grid_check"
    csrc = os.path.join(ROOT, "multi-modal-loam_amd", "csrc")
    out = subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "vox_grid_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert run.stdout == "vox_grid_check ok\n"
