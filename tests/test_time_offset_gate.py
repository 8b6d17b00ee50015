"""mml_time_offset_gate (csrc/time_offset_gate.h), host only: the frame estimate_timeoffset runs on, held to a sequential
restatement of unionLidarsAligner.cpp:1026-1051 written here -- and the refusals of mml_time_offset_estimate_stream that are
reachable without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

S = 1000000000          # ns per second
T0 = 1600000000 * S     # a stamp of the year 2020: the doubles involved carry about 2.4e-7 s


def to_sec(ns):
    """ros::Time::toSec(): (double)sec + 1e-9 * (double)nsec"""
    return float(ns // S) + 1e-9 * float(ns % S)


def gate_ref(velo, hori, n_msgs):
    """:1026-1051 as the reference walks them, on lists; the two reads it leaves undefined are the two refusals."""
    velo = list(velo)
    if not velo:
        return -1, 1                                   # :1026 back() of an empty vector
    v, h = to_sec(velo[-1]), to_sec(hori)              # :1026-1027
    while v > h or abs(v - h) < 0.2:                   # :1034 (abs on doubles: DESIGN.md convention 15)
        velo.pop()                                     # :1037-1038
        if not velo:
            return -1, 1                               # :1039 back() of an empty vector: GATE_EMPTY
        v = to_sec(velo[-1])                           # :1039
    if n_msgs < 8:
        return -1, 2                                   # :1051 hori_vec[msg_size - 8]: TOO_FEW_MESSAGES
    return len(velo) - 1, 0                            # :1044


HAND = [
    ("a velo stamp newer than hori", [T0 - 2 * S, T0 + S // 2], T0, 8, (0, 0)),
    ("within 0.2 s, velo older", [T0 - S, T0 - S // 10], T0, 8, (0, 0)),
    ("within 0.2 s, velo newer", [T0 - S, T0 + S // 10], T0, 8, (0, 0)),
    ("0.3 s older: kept", [T0 - S, T0 - 3 * S // 10], T0, 8, (1, 0)),
    ("several pops", [T0 - 3 * S, T0 - S, T0 - S // 10, T0 + S // 100, T0 + S], T0, 9, (1, 0)),
    ("all frames popped", [T0 - S // 10, T0, T0 + S], T0, 8, (-1, 1)),
    ("one frame, popped", [T0], T0, 8, (-1, 1)),
    ("no frame", [], T0, 8, (-1, 1)),
    ("7 messages", [T0 - S], T0, 7, (-1, 2)),
    ("8 messages", [T0 - S], T0, 8, (0, 0)),
    ("7 messages and every frame popped: the loop comes first", [T0], T0, 7, (-1, 1)),
    ("a second boundary in between", [999999999, 2 * S + 5], 3 * S, 8, (1, 0)),
]


def test_hand_made_lists(M):
    for what, velo, hori, n_msgs, want in HAND:
        assert gate_ref(velo, hori, n_msgs) == want, what
        assert M.time_offset_gate(velo, hori, n_msgs) == want, what


def test_exactly_0p2_s_apart_follows_the_doubles(M):
    """Exactly 0.2 s in nanoseconds is not exactly 0.2 in toSec() doubles: whether the frame is popped is what the reference's
    comparison of the two doubles gives, on either side -- the restatement decides, the library follows it, and both outcomes occur."""
    seen = set()
    for k in range(400):
        hori = T0 + k * 7919 * 1000 + 123456789
        velo = [hori - 5 * S, hori - S // 5]
        want = gate_ref(velo, hori, 8)
        assert M.time_offset_gate(velo, hori, 8) == want, k
        seen.add(want[0])
    assert seen == {0, 1}
    # small stamps, where the doubles can be written down: 1.0 - 0.8 = 0.19999999999999996 < 0.2 pops; toSec() of 0.3 s is
    # 1e-9 * 3e8 = 0.30000000000000004 and of 0.1 s 0.1, whose difference 0.20000000000000004 stays
    assert M.time_offset_gate([1, 8 * S // 10], S, 8) == gate_ref([1, 8 * S // 10], S, 8) == (0, 0)
    assert to_sec(S) - to_sec(8 * S // 10) < 0.2 < to_sec(3 * S // 10) - to_sec(S // 10)
    assert M.time_offset_gate([1, S // 10], 3 * S // 10, 8) == gate_ref([1, S // 10], 3 * S // 10, 8) == (1, 0)


def random_cases(n, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        hori = T0 + int(rng.integers(0, 50 * S))
        m = int(rng.integers(0, 9))
        # frames every ~0.1 s ending around hori: older, near and newer stamps, sometimes out of order, sometimes exactly 0.2 s off
        end = hori + int(rng.integers(-12, 6)) * (S // 10) + int(rng.integers(-3, 4)) * int(rng.integers(0, 2))
        velo = sorted(end - int(rng.integers(0, 20)) * (S // 10) - int(rng.integers(0, 1000)) for _ in range(m))
        if m and rng.random() < 0.2:
            velo[int(rng.integers(0, m))] = hori - S // 5
        if m > 1 and rng.random() < 0.1:
            rng.shuffle(velo)
        out.append((velo, hori, int(rng.integers(5, 11))))
    return out


def test_random_lists(M):
    statuses = set()
    for velo, hori, n_msgs in random_cases(4000):
        want = gate_ref(velo, hori, n_msgs)
        assert M.time_offset_gate(velo, hori, n_msgs) == want, (velo, hori, n_msgs)
        statuses.add(want[1])
    assert statuses == {0, 1, 2}


def test_argument_rules(M):
    L = M.lib()
    sel, st = C.c_int(-7), C.c_int(-7)
    v = np.array([T0], np.uint64)
    p = v.ctypes.data_as(C.c_void_p)
    assert L.mml_time_offset_gate(-1, p, T0, 8, C.byref(sel), C.byref(st)) == M.MML_ERR_INVALID
    assert L.mml_time_offset_gate(1, None, T0, 8, C.byref(sel), C.byref(st)) == M.MML_ERR_INVALID
    assert L.mml_time_offset_gate(1, p, T0, -1, C.byref(sel), C.byref(st)) == M.MML_ERR_INVALID
    assert L.mml_time_offset_gate(1, p, T0, 8, None, C.byref(st)) == M.MML_ERR_INVALID
    assert L.mml_time_offset_gate(1, p, T0, 8, C.byref(sel), None) == M.MML_ERR_INVALID
    assert (sel.value, st.value) == (-7, -7)            # a refusal writes nothing
    assert L.mml_time_offset_gate(0, None, T0, 8, C.byref(sel), C.byref(st)) == M.MML_OK and (sel.value, st.value) == (-1, M.TOFS_GATE_EMPTY)


def test_declared_in_the_header_exported_and_row_layout(M, tmp_path):
    header = open(M.HEADER_PATH).read()
    for name in ("mml_time_offset_estimate_stream", "mml_time_offset_gate"):
        assert name + "(" in header and hasattr(M.lib(), name)
    for name, val in (("MML_TOFS_GATE_OK", M.TOFS_GATE_OK), ("MML_TOFS_GATE_EMPTY", M.TOFS_GATE_EMPTY),
                      ("MML_TOFS_GATE_TOO_FEW_MESSAGES", M.TOFS_GATE_TOO_FEW_MESSAGES), ("MML_TOFS_ROW_OK", M.TOFS_ROW_OK),
                      ("MML_TOFS_ROW_NO_VELO_IN_FOV", M.TOFS_ROW_NO_VELO_IN_FOV)):
        assert "#define %s %d" % (name, val) in header
    src = tmp_path / "row.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mmloam_hip.h"\nint main(void) { typedef mml_time_offset_estimate_row R;\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(R), offsetof(R, status), offsetof(R, n_kept), offsetof(R, n_windows),\n'
                   'offsetof(R, best_window), offsetof(R, lowest_error), offsetof(R, optim_start), offsetof(R, time_offset), offsetof(R, accepted));\n'
                   'return 0; }\n')
    exe = tmp_path / "row"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = M.TOFS_ROW_DTYPE
    assert got == [d.itemsize] + [d.fields[k][1] for k in ("status", "n_kept", "n_windows", "best_window", "lowest_error", "optim_start",
                                                          "time_offset", "accepted")]


def test_stream_call_without_a_context_is_refused(M):
    """The one refusal of the device call that is reachable without a device: a NULL context (every other rule needs the stream's
    context to carry the message; tests/test_gpu_time_offset_stream.py holds them with sentinels)."""
    rows = np.full(1, -9, M.TOFS_ROW_DTYPE)
    bo, npts, vs = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = M.lib().mml_time_offset_estimate_stream(None, None, 0, 0, 1, None, p(bo), p(npts), 16, 0, 4, 8, p(vs), None, 30, 512, 1e6, None, None,
                                                 None, p(rows))
    assert rc == M.MML_ERR_INVALID
    assert np.all(rows["status"] == -9) and np.all(rows["best_window"] == -9)


def test_gate_header_under_sanitizers(M, tmp_path):
    """csrc/time_offset_gate.h compiled by the host compiler into a stand-alone program with AddressSanitizer and
    UndefinedBehaviorSanitizer: the hand-made lists and the random ones, answers against the restatement."""
    exe = tmp_path / "time_offset_gate_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "cpp", "time_offset_gate_replay.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    cases = [(v, h, m) for _, v, h, m, _ in HAND] + random_cases(1500, seed=12)
    text = "%d\n" % len(cases) + "".join("%d %d %d\n%s\n" % (len(v), h, m, " ".join(str(int(x)) for x in v)) for v, h, m in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    got = [tuple(int(x) for x in ln.split()) for ln in run.stdout.splitlines()]
    assert got == [(0,) + gate_ref(v, h, m) for v, h, m in cases]
