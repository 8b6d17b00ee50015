"""mml::ImuQueue of the C++ adapter without a device: the header compiles, and a program that pushes the messages one by one
and calls fetchImuMsgs (single and batch form) and the trim gives what tests/imu_fetch_ref.py gives, to the byte."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imu_fetch_cases as IC  # noqa: E402
import imu_fetch_ref as IR  # noqa: E402


def test_imu_queue_replays_the_edge_cases(M, tmp_path):
    exe = tmp_path / "imu_queue_replay"
    libdir = os.path.dirname(M.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
           os.path.join(ROOT, "tests", "cpp", "imu_queue_replay.cpp"), "-o", str(exe), "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    msgs = IC.stream()
    T = msgs[:, 0]
    cases = IC.edge_intervals(T)
    ts, te = [c[1] for c in cases], [c[2] for c in cases]
    text = "%d %d\n" % (len(msgs), len(ts)) + "\n".join(" ".join(float(v).hex() for v in m) for m in msgs) + "\n" + \
        "\n".join("%s %s" % (float(a).hex(), float(b).hex()) for a, b in zip(ts, te)) + "\n%s %d\n" % (float(T[450]).hex(), 200)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows, offsets, samples = IR.fetch_batch(msgs, ts, te)
    lines = run.stdout.splitlines()
    k = 0
    for i in range(len(ts)):
        ok, status, n = (int(v) for v in lines[k].split())
        assert (ok, status, n) == (int(rows["status"][i] == 0), rows["status"][i], rows["n"][i]), cases[i][0]
        got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[k + 1:k + 1 + n]]).reshape(-1, 7)
        assert got.tobytes() == samples[offsets[i]:offsets[i + 1]].tobytes(), cases[i][0]
        k += 1 + n
    assert lines[k] == "batch same"
    assert lines[k + 1] == "size %d" % (len(T) - IR.drop_before(list(T), 0, T[450], 200))
