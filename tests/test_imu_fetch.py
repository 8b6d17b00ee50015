"""mml_imu_fetch_host (csrc/imu_fetch.h on the host: two binary searches per interval) against the yardstick
tests/imu_fetch_ref.py (fetchImuMsgs as the sequential walk of unionPoseEstimation.cpp:307-395).  Status, n, first,
interpolated, the gyro z operands, offsets and every sample double must have the same BYTES: the arithmetic is a fixed sequence of
IEEE double operations with contraction off.  No device is needed; what the device does with the same header is
tests/test_gpu_imu_fetch.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imu_fetch_cases as IC  # noqa: E402
import imu_fetch_ref as IR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_cut_equal(got, want, what):
    rows, offsets, samples = want
    assert got["rows"].dtype == rows.dtype
    for name in rows.dtype.names:
        assert got["rows"][name].tobytes() == rows[name].tobytes(), "%s: %s differs\n got %s\nwant %s" % (what, name, got["rows"], rows)
    assert np.array_equal(got["offsets"], offsets), what
    if "samples" in got:
        assert got["samples"].shape == samples.shape and got["samples"].tobytes() == samples.tobytes(), what


def host_cut(M, msgs, ts, te, **kw):
    return M.imu_fetch_batch(np.asarray(msgs, dtype=np.float64).reshape(-1, 7), ts, te, **kw)


def test_names_exist(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    for name in ("mml_imu_stream_create", "mml_imu_stream_destroy", "mml_imu_stream_reset", "mml_imu_stream_push", "mml_imu_stream_drop_before",
                 "mml_imu_stream_state_get", "mml_imu_fetch_batch", "mml_imu_fetch_host", "mml_imu_predict_batch"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_IMU_FETCH_BATCH_MAX\s+%d\b" % M.IMU_FETCH_BATCH_MAX, header) and M.IMU_FETCH_BATCH_MAX == M.PREINT_BATCH_MAX
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    assert M.IMU_INTERVAL_DTYPE == IR.INTERVAL_DTYPE and M.IMU_INTERVAL_DTYPE.itemsize == 40
    assert (M.IMU_FETCH_OK, M.IMU_FETCH_EMPTY, M.IMU_FETCH_NOT_REACHED, M.IMU_FETCH_TOO_OLD, M.IMU_FETCH_REVERSED, M.IMU_FETCH_NO_SAMPLE) == \
        (IR.OK, IR.EMPTY, IR.NOT_REACHED, IR.TOO_OLD, IR.REVERSED, IR.NO_SAMPLE)
    for name in ("push", "drop_before", "state", "reset"):
        assert callable(getattr(M.ImuStream, name)), name
    assert callable(M.Context.imu_stream)
    # the struct sizes the ctypes / numpy views must agree with
    code = '#include <stdio.h>\n#include "mmloam_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(mml_imu_interval), sizeof(mml_imu_stream_state)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert sizes == [M.IMU_INTERVAL_DTYPE.itemsize, C.sizeof(M.ImuStreamState)]
    # a NULL context or stream is refused
    assert M.lib().mml_imu_fetch_batch(None, None, 1, None, None, None, None, None, None, None, 0, None, None) == M.MML_ERR_INVALID
    assert M.lib().mml_imu_stream_push(None, None, 0) == M.MML_ERR_INVALID


def test_edge_intervals_one_by_one_and_in_one_call(M):
    msgs = IC.stream()
    cases = IC.edge_intervals(msgs[:, 0])
    seen = set()
    for name, s, e, status, n, interp in cases:
        want = IR.fetch_batch(msgs, [s], [e])
        # the yardstick itself gives what the case was built to give (worked out by hand from the reference's lines)
        assert (int(want[0]["status"][0]), int(want[0]["n"][0]), int(want[0]["interpolated"][0])) == (status, n, interp), (name, want[0])
        assert_cut_equal(host_cut(M, msgs, [s], [e], want=("samples",)), want, name)
        seen.add(status)
    assert seen == {0, 2, 3, 4, 5}
    ts, te = [c[1] for c in cases], [c[2] for c in cases]
    assert_cut_equal(host_cut(M, msgs, ts, te, want=("samples",)), IR.fetch_batch(msgs, ts, te), "all in one call")


def test_first_names_the_first_message(M):
    msgs = IC.stream()
    T = msgs[:, 0]
    got = host_cut(M, msgs, [T[30], T[IC.DUP_A]], [IC.mid(T, 33), IC.mid(T, 13)], want=())
    assert list(got["rows"]["first"]) == [31, 12]


def test_one_message_stream_and_empty_array(M):
    one = IC.stream()[:1]
    t = one[0, 0]
    ts = [t - 1, t - 1, t - 1, t + 1, t, t - 1]
    te = [t + 1, t, t - 0.5, t, t, np.nextafter(t, np.inf)]
    want = IR.fetch_batch(one, ts, te)
    assert list(want[0]["status"]) == [IR.NOT_REACHED, IR.TOO_OLD, IR.TOO_OLD, IR.REVERSED, IR.TOO_OLD, IR.NOT_REACHED]
    assert_cut_equal(host_cut(M, one, ts, te, want=("samples",)), want, "one message")
    want = IR.fetch_batch(np.zeros((0, 7)), [1.0, 2.0], [2.0, 1.0])
    assert list(want[0]["status"]) == [IR.EMPTY, IR.EMPTY]                  # (:309 comes before :325)
    got = host_cut(M, np.zeros((0, 7)), [1.0, 2.0], [2.0, 1.0], bg=np.zeros(3), ba=np.zeros(3))
    assert_cut_equal(got, want, "empty array")
    assert np.array_equal(got["dq"], [[0, 0, 0, 1]] * 2) and got["pre"][1].dtime == 0.0 and got["pre"][1].jacobian[16] == 1.0


def test_consecutive_frames_with_preintegration_and_gyro(M):
    msgs = IC.stream()
    ts, te = IC.consecutive(30)
    bg, ba = IC.biases(30)
    want = IR.fetch_batch(msgs, ts, te)
    got = host_cut(M, msgs, ts, te, bg=bg, ba=ba)
    assert_cut_equal(got, want, "30 frames")
    assert np.all(want[0]["status"] == IR.OK) and set(want[0]["n"]) <= {20, 21} and np.all(want[0]["interpolated"] == 1)
    # row 0's dt counts from the previous frame's stamp: every interval's dt column sums to its length (to rounding)
    o = want[1]
    for i in range(30):
        assert abs(want[2][o[i]:o[i + 1], 6].sum() - (te[i] - ts[i])) < 1e-6 and np.all(want[2][o[i]:o[i + 1], 6] > 0)
    per = [got["samples"][o[i]:o[i + 1]] for i in range(30)]
    pre = M.imu_preintegrate_batch(per, bg, ba)
    assert bytes(got["pre"]) == b"".join(bytes(p) for p in pre)
    # dq: the chain of mml_imu_gyro_integrate.  The two may differ in whose sin / cos they call (an ulp) over at most 21
    # chained unit-quaternion products: 21 x a few x 2.2e-16, bound 1e-12 with two orders of margin
    ref = np.stack([M.imu_gyro_integrate(p) for p in per])
    d = np.abs(got["dq"] - ref).max()
    print("max |dq - mml_imu_gyro_integrate| = %.3e" % d)
    assert d <= 1e-12
    # outputs do not depend on what else is asked for, and samples may stay inside
    only = host_cut(M, msgs, ts, te, bg=bg, ba=ba, want=("pre", "dq"))
    assert bytes(only["pre"]) == bytes(got["pre"]) and only["dq"].tobytes() == got["dq"].tobytes() and "samples" not in only


def test_prediction_against_numpy(M):
    from scipy.spatial.transform import Rotation
    msgs = IC.stream()
    n = 12
    ts, te = IC.consecutive(n)
    bg, ba = IC.biases(n)
    got = host_cut(M, msgs, ts, te, bg=bg, ba=ba)
    rng = np.random.default_rng(3)
    prev = np.concatenate([rng.normal(0, 30, (n, 3)), Rotation.random(n, random_state=4).as_quat(), rng.normal(0, 2, (n, 3))], axis=1)
    ex = np.eye(4)
    ex[:3, :3] = Rotation.from_rotvec([0.02, -0.4, 1.1]).as_matrix()
    ex[:3, 3] = [0.1, -0.05, 0.3]
    out = M.imu_predict_batch(ex, prev=prev, pre=got["pre"], dq=got["dq"])
    worst = 0.0
    for i in range(n):
        p = got["pre"][i]
        st, dR, dt = IR.predict_lio(prev[i], np.array(p.dq), np.array(p.dp), np.array(p.dv), ex)
        Rb, Rl = IR.predict_gyro(got["dq"][i], ex)
        scale = max(1.0, np.abs(st[:3]).max())
        for a, b in ((out["state"][i], st), (out["delta_Rl"][i], dR), (out["delta_tl"][i], dt), (out["gyro_Rb"][i], Rb), (out["gyro_Rl"][i], Rl)):
            worst = max(worst, np.abs(a - b).max() / scale)
    print("max |prediction - numpy| / max(1, |P|) = %.3e" % worst)
    assert worst <= 1e-12
    # the groups are independent, and a group given in part is refused
    lio = M.imu_predict_batch(ex, prev=prev, pre=got["pre"])
    assert lio["state"].tobytes() == out["state"].tobytes() and "gyro_Rb" not in lio
    gy = M.imu_predict_batch(ex, dq=got["dq"])
    assert gy["gyro_Rl"].tobytes() == out["gyro_Rl"].tobytes()
    z = np.zeros((1, 10))
    assert M.lib().mml_imu_predict_batch(None, 1, M._p(ex), M._p(z), None, None, None, None, None, None, None) == M.MML_ERR_INVALID
    assert M.lib().mml_imu_predict_batch(None, 1, M._p(ex), *([None] * 8)) == M.MML_ERR_INVALID
    assert M.lib().mml_imu_predict_batch(None, 0, M._p(ex), *([None] * 5), M._p(z), M._p(z), M._p(z)) == M.MML_ERR_INVALID


def test_refusals_write_nothing_and_the_next_call_is_right(M):
    msgs = IC.stream()
    ts, te = IC.consecutive(4)
    good = host_cut(M, msgs, ts, te, bg=np.zeros(3), ba=np.zeros(3))
    L = M.lib()
    rows = np.full(4, 7, M.IMU_INTERVAL_DTYPE)
    off = np.full(5, 7, np.int32)
    smp = np.full((200, 7), 7.0)
    dq = np.full((4, 4), 7.0)
    pre = (M.ImuPreint * 4)()
    z = np.zeros((4, 3))
    p = M._p

    def call(n=4, msgs_=msgs, ts_=ts, te_=te, bg=z, ba=z, rows_=rows, off_=off, cap=200, pre_=pre, n_msgs=None):
        return L.mml_imu_fetch_host(p(msgs_), len(msgs_) if n_msgs is None else n_msgs, n, p(ts_), p(te_), p(bg), p(ba), p(rows_), p(off_), p(smp), cap, pre_, p(dq))

    bad_t = ts.copy()
    bad_t[2] = np.inf
    nan_t = te.copy()
    nan_t[1] = np.nan
    unordered = msgs.copy()
    unordered[[100, 101]] = unordered[[101, 100]]
    for what, rc, want in (("n = 0", call(n=0), M.MML_ERR_INVALID), ("n too large", call(n=M.IMU_FETCH_BATCH_MAX + 1), M.MML_ERR_INVALID),
                           ("null t_start", call(ts_=None), M.MML_ERR_INVALID), ("null t_end", call(te_=None), M.MML_ERR_INVALID),
                           ("null rows", call(rows_=None), M.MML_ERR_INVALID), ("null offsets", call(off_=None), M.MML_ERR_INVALID),
                           ("bg without ba", call(ba=None), M.MML_ERR_INVALID), ("ba without bg", call(bg=None), M.MML_ERR_INVALID),
                           ("pre without biases", call(bg=None, ba=None), M.MML_ERR_INVALID), ("infinite time", call(ts_=bad_t), M.MML_ERR_INVALID),
                           ("NaN time", call(te_=nan_t), M.MML_ERR_INVALID), ("negative capacity", call(cap=-1), M.MML_ERR_INVALID),
                           ("negative n_msgs", call(n_msgs=-1), M.MML_ERR_INVALID), ("unordered stamps", call(msgs_=unordered), M.MML_ERR_STATE)):
        assert rc == want, what
        assert np.all(rows["status"] == 7) and np.all(off == 7) and np.all(smp == 7.0) and np.all(dq == 7.0), what
    # one row short: rows and offsets are written, so the caller learns the size; samples, pre and dq are not
    total = int(good["offsets"][4])
    assert call(cap=total - 1) == M.MML_ERR_CAPACITY
    assert rows.tobytes() == good["rows"].tobytes() and np.array_equal(off, good["offsets"]) and np.all(smp == 7.0) and np.all(dq == 7.0)
    assert call(cap=total) == M.MML_OK
    assert smp[:total].tobytes() == good["samples"].tobytes() and dq.tobytes() == good["dq"].tobytes() and bytes(pre) == bytes(good["pre"])


def test_drop_before_rule():
    """The sequential trim the device tests hold ImuStream.drop_before to (tests/test_gpu_imu_fetch.py)."""
    T = list(IC.stream(50)[:, 0])
    assert IR.drop_before(T, 0, T[20], 10) == 20
    assert IR.drop_before(T, 0, T[45], 10) == 40            # keep_min stops it
    assert IR.drop_before(T, 5, T[45], 100) == 5            # keep_min larger than the live count
    assert IR.drop_before(T, 5, T[0] - 1.0, 0) == 5         # t before the front
    assert IR.drop_before(T, 0, T[49] + 1.0, 0) == 50
    assert IR.drop_before(T, 0, T[IC.DUP_A + 1], 0) == IC.DUP_A     # equal stamps: neither is older than t


def test_host_headers_under_sanitizers(M, tmp_path):
    """csrc/imu_fetch.h compiled by the host compiler into a stand-alone program with AddressSanitizer and
    UndefinedBehaviorSanitizer: the edge intervals and the consecutive frames, rows against the yardstick."""
    exe = tmp_path / "imu_fetch_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-D__host__=", "-D__device__=", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                          os.path.join(ROOT, "tests", "cpp", "imu_fetch_replay.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    msgs = IC.stream()
    cases = IC.edge_intervals(msgs[:, 0])
    c_ts, c_te = IC.consecutive(30)
    ts = np.array([c[1] for c in cases] + list(c_ts))
    te = np.array([c[2] for c in cases] + list(c_te))
    text = "%d %d\n" % (len(msgs), len(ts)) + "\n".join(" ".join(float(v).hex() for v in m) for m in msgs) + "\n" + \
        "\n".join("%s %s" % (float(a).hex(), float(b).hex()) for a, b in zip(ts, te)) + "\n"
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    rows, offsets, samples = IR.fetch_batch(msgs, ts, te)
    lines = run.stdout.splitlines()
    head = np.array([[int(v) for v in ln.split()[:4]] for ln in lines[:len(ts)]], np.int64)
    assert np.array_equal(head[:, 0], rows["status"]) and np.array_equal(head[:, 1], rows["n"]) and np.array_equal(head[:, 2], rows["first"])
    assert np.array_equal(head[:, 3], rows["interpolated"])
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[len(ts):len(ts) + len(samples)]])
    assert got.tobytes() == samples.tobytes()
    # the last line: the gyro chain and the prediction ran on every interval without a report; a checksum keeps them alive
    assert lines[-1].startswith("checksum ")
