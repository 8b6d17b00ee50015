"""The upper layers of the union-frame assembly without a device: the C++ adapter's LivoxPointQueue compiles with the host
compiler, the C-ABI and Python names exist, and csrc/union_plan.h -- the recurrence the device kernel runs -- replays the fixed
cases in a stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer, against tests/union_ref.py."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import union_cases as UC  # noqa: E402
import union_ref as UR  # noqa: E402


def test_adapter_header_compiles_with_the_host_compiler(M, tmp_path):
    src = tmp_path / "queue_probe.cpp"
    src.write_text(textwrap.dedent(r"""
        #include "mmloam_adapter.hpp"
        bool one(mml::Context& c, const std::vector<mml::LivoxMsg>& msgs, const float* velo, int n, const float* tf) {
            mml::LivoxPointQueue q(c, 100000);
            q.transform_hori_timestamp(msgs);
            const bool ok = q.pub_horipoints_given_stamp(10, 20, velo, n, tf, 0);
            const std::vector<bool> many = q.pub_horipoints_given_stamp(std::vector<uint64_t>{20, 30, 40}, velo, std::vector<int>{0, n, n}, tf, 0);
            q.reset();
            return ok && many[1] && q.last_frame().status == 0 && q.state().disorder == 0 && q.last_frames().size() == 2;
        }
        """))
    libdir = os.path.dirname(M.LIB_PATH)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                          str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_names_exist(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    for name in ("mml_livox_stream_create", "mml_livox_stream_destroy", "mml_livox_stream_reset", "mml_livox_stream_push",
                 "mml_livox_stream_push_wire", "mml_livox_stream_state_get", "mml_union_assemble", "mml_union_plan", "mml_scan_raw_download"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_UNION_BATCH_MAX\s+%d\b" % M.UNION_BATCH_MAX, header) and M.UNION_BATCH_MAX == 65535
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    for name in ("livox_stream", "union_assemble", "scan_raw_download"):
        assert callable(getattr(M.Context, name)), name
    for name in ("push", "push_wire", "state", "reset"):
        assert callable(getattr(M.LivoxStream, name)), name
    assert callable(M.union_plan) and M.UNION_FRAME_DTYPE.itemsize == 32
    assert (M.UNION_OK, M.UNION_EMPTY, M.UNION_NOT_REACHED, M.UNION_NO_POINTS, M.UNION_OVERFLOW) == (0, 1, 2, 3, 4)
    # a NULL context or stream is refused
    assert M.lib().mml_union_assemble(None, None, 0, 1, None, None, None, None, None) == M.MML_ERR_INVALID
    assert M.lib().mml_livox_stream_push(None, 0, None, 0) == M.MML_ERR_INVALID


def test_union_plan_header_replays_the_fixed_cases_under_sanitizers(M, tmp_path):
    exe = tmp_path / "union_plan_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "cpp", "union_plan_replay.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    cases = UC.fixed_cases()
    text, wants = [], []
    for name in sorted(cases):
        msgs, bounds, maxl, _ = cases[name]
        hs, S = UC.stamps_of(msgs)
        text.append("%d 0 %d %d %d\n%s\n%s\n" % (hs, len(S), maxl, len(bounds) - 1, " ".join(str(int(v)) for v in S),
                                                " ".join(str(v % 2 ** 64) for v in bounds)))
        wants.append(UR.replay(msgs, bounds, maxl)[0])
    run = subprocess.run([str(exe)], input="".join(text), capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], np.int64)
    want = np.concatenate(wants)
    assert len(got) == len(want)
    for k, name in enumerate(want.dtype.names):
        assert np.array_equal(got[:, k], want[name]), name
