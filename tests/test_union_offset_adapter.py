"""The upper layers of the time-offset mode without a device: the C++ adapter's one-stamp overloads and time_offset_ns compile
with the host compiler and resolve as intended, and csrc/union_plan.h's mml_union_resolve_offset -- the recurrence the device
kernel runs -- replays the fixed cases in a stand-alone host program (its own main) built with AddressSanitizer and
UndefinedBehaviorSanitizer, against tests/union_offset_ref.py.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import union_cases as UC  # noqa: E402
import union_offset_cases as OC  # noqa: E402
import union_offset_ref as OR  # noqa: E402


def test_adapter_overloads_compile_with_the_host_compiler(M, tmp_path):
    src = tmp_path / "offset_queue_probe.cpp"
    src.write_text(textwrap.dedent(r"""
        #include <type_traits>
        #include "mmloam_adapter.hpp"
        // search -> offset -> assembly as one path (unionLidarsAligner.cpp:1146, :1161, :520, :872-1009)
        bool one(mml::Context& c, const std::vector<mml::LivoxMsg>& msgs, const float* velo, int n, const float* tf, uint64_t velo_stamp,
                 uint64_t livox_timebase, uint64_t best_offset) {
            mml::LivoxPointQueue q(c, 100000);
            q.transform_hori_timestamp(msgs);
            const uint64_t time_offset = mml::time_offset_ns(velo_stamp, livox_timebase, best_offset);
            const int sliced_points = 12000;
            const bool ok = q.pub_horipoints_given_stamp(velo_stamp - time_offset, sliced_points, velo, n, tf, 0);
            const std::vector<bool> many = q.pub_horipoints_given_stamp(std::vector<uint64_t>{20, 30, 40}, sliced_points, velo,
                                                                        std::vector<int>{0, n, n, n}, tf, 0);
            // the interval overload is still reached with two uint64_t stamps
            const uint64_t a = 10, b = 20;
            const bool interval = q.pub_horipoints_given_stamp(a, b, velo, n, tf, 0);
            return ok && many[2] && interval && q.last_frames().size() == 1;
        }
        static_assert(std::is_same<decltype(mml::time_offset_ns(0, 0, 0)), uint64_t>::value, "uint64 arithmetic");
        """))
    libdir = os.path.dirname(M.LIB_PATH)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
                          str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_time_offset_ns_restates_the_reference(M, tmp_path):
    """:1146 / :1161 in uint64, wrapping when the Livox clock is ahead, and :520 undoing it: a stand-alone program."""
    src = tmp_path / "time_offset_ns.cpp"
    exe = tmp_path / "time_offset_ns"
    src.write_text(textwrap.dedent(r"""
        #include <cstdio>
        #include "mmloam_adapter.hpp"
        int main() {
            const uint64_t velo = 1600000000123456789ull, tb = 1600000000000000000ull, off = 37000000ull;
            const uint64_t d = mml::time_offset_ns(velo, tb, off);
            if (d != 86456789ull) return 1;
            if (velo - d != tb + off) return 2;                  // :520: the frame starts at the best window's first point
            const uint64_t ahead = mml::time_offset_ns(tb, velo, off);   // Livox ahead of the Velodyne: the difference wraps ...
            if (ahead != 0ull - 123456789ull - off) return 3;
            if (tb - ahead != velo + off) return 4;              // ... and :520 still lands on the point
            std::puts("ok");
            return 0;
        }
        """))
    libdir = os.path.dirname(M.LIB_PATH)
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"), str(src), "-o", str(exe)],
                         capture_output=True, text=True)   # (no library: nothing but the inline function is used)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stderr[-2000:])


def test_union_plan_header_replays_the_fixed_cases_under_sanitizers(M, tmp_path):
    exe = tmp_path / "union_offset_plan_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "cpp", "union_offset_plan_replay.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    cases = OC.fixed_cases()
    text, wants = [], []
    for name in sorted(cases):
        msgs, starts, c, _ = cases[name]
        hs, S = UC.stamps_of(msgs)
        text.append("%d 0 %d %d %d\n%s\n%s\n" % (hs, len(S), c, len(starts), " ".join(str(int(v)) for v in S),
                                                " ".join(str(v % 2 ** 64) for v in starts)))
        wants.append(OR.replay(msgs, starts, c)[0])
    run = subprocess.run([str(exe)], input="".join(text), capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    got = np.array([[int(v) for v in line.split()] for line in run.stdout.splitlines()], np.int64)
    want = np.concatenate(wants)
    assert len(got) == len(want)
    for k, name in enumerate(want.dtype.names):
        assert np.array_equal(got[:, k], want[name]), name
