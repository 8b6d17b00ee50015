"""csrc/mml_mem.h, the owner of the library's device and pinned memory, on its failure paths: a stand-alone host program
(tests/cpp/mem_owner_replay.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  Without a device every allocation
fails and leaves its pointer null, which is what the program needs; where a device is visible the test skips, so that no device is
ever opened under a sanitizer.  The same program checks the header's two device-free helpers: the block layouts of MmlCarve and
the side calls' registry MmlSides (created once, empty after a failed reserve, released any number of times, nothing leaked)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memory_owners_survive_failed_allocations_under_sanitizers(M, has_gpu, tmp_path):
    if has_gpu:
        pytest.skip("a device is visible: the allocations would succeed")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "mem_owner_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                          "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                          os.path.join(ROOT, "tests", "cpp", "mem_owner_replay.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-1000:], run.stderr[-3000:])
    assert run.stdout == "mem_owner_replay ok\n"
