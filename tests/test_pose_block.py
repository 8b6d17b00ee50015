"""csrc/pose_block.h, the parameter block behind mml_step and mml_estimate: a stand-alone host program
(tests/cpp/pose_block_check.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own.  For
1, 2, 16, 17, 33 and 4096 slots the fields do not overlap, the block ends inside the 64 doubles per slot that d_pose_in gives its
slots and reports the extent of its last field as its size; the pieces of a call cut the way mml_step cuts it (3 + 65 slots over 2
lanes, 4096 over 8) are pairwise disjoint and lie inside the call's range.  The header needs no device; like the memory owners'
program this one runs where none is visible, so that sanitizer builds stay on the CPU machines."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_block_layout_under_sanitizers(has_gpu, tmp_path):
    if has_gpu:
        pytest.skip("a device is visible: sanitizer builds run on the CPU machines")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "pose_block_check"
    csrc = os.path.join(ROOT, "multi-modal-loam_amd", "csrc")
    out = subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                          "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "pose_block_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert run.stdout == "pose_block_check ok\n"
