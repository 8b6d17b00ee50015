"""CPU suite for the pose node's batched way in (mml_pose_ingest_plan; mml_pose_ingest_batch runs the same routine,
csrc/pose_ingest.h): the decisions of unionPoseEstimation.cpp:719-773 against a restatement written here, the counts, the
argument errors and the C-ABI surface.  The device half is tests/test_gpu_pose_ingest.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mml_pose_ingest_plan", "mml_pose_ingest_batch")
FILL = 0x5A


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the rules, restated ------------------------------------------------------------------------------------------------
def expected_row(M, np6, row, first, hth, vth, velo_only):
    """(decision, reason, fast_rotation, n_points, n_velo, 0) for one frame.  row: None or (status, n, front, back)."""
    if row is not None and row[1] == 0:                                   # :719-730: nothing fetched, the message is popped
        return (M.INGEST_DROPPED, M.INGEST_WHY_FETCH + row[0], 0, 0, 0, 0)
    nv, corners, nl = int(np6[2]), int(np6[3]), int(np6[5])
    if row is None:                                                       # IMU_Mode 0: vimuMsg.empty() at :741
        return (M.INGEST_VELO_ONLY, M.INGEST_WHY_NO_IMU, 0, nv, nv, 0)
    if first:                                                             # first_velo_frame at :741
        return (M.INGEST_VELO_ONLY, M.INGEST_WHY_FIRST_FRAME, 0, nv, nv, 0)
    f, b = abs(float(row[2])), abs(float(row[3]))                         # NaN stays NaN: every comparison below is False
    fast = int(f > vth or b > vth)                                        # :771
    if velo_only:                                                         # :746, :767
        return (M.INGEST_VELO_ONLY, M.INGEST_WHY_VELO_ONLY_MODE, fast, nv, nv, 0)
    if not (f < hth or b < hth):                                          # :747
        return (M.INGEST_VELO_ONLY, M.INGEST_WHY_FAST_ROTATION, fast, nv, nv, 0)
    if not corners > 100:                                                 # :748
        return (M.INGEST_VELO_ONLY, M.INGEST_WHY_FEW_CORNERS, fast, nv, nv, 0)
    return (M.INGEST_MERGED, M.INGEST_WHY_MERGED, fast, nv + nl, nv, 0)   # :756


def _table(M, hth, vth):
    """frames covering every gyro pair of the value list x livox_corner_num in {0, 100, 101}, plus the rows with n == 0 for every
    fetch status: (n_points (F, 6), rows (F))"""
    up, dn = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    mags = [0.0, 0.1, dn(hth), hth, up(hth), 1.0, dn(vth), vth, up(vth), 2.0]       # below / exactly at / above each threshold
    vals = sorted(set(mags + [-m for m in mags])) + [float("nan")]                  # both signs (mixed in the pairs), NaN
    rng = np.random.default_rng(3)
    n6, rows = [], []
    for corners, (f, b) in itertools.product((0, 100, 101), itertools.product(vals, vals)):
        c = rng.integers(0, 400, 6)
        c[3] = corners
        n6.append(c)
        rows.append((0, int(rng.integers(1, 30)), 0, 0, 0, f, b))
    for status, corners in itertools.product((1, 2, 3, 4, 5), (0, 101)):             # nothing fetched: n == 0, gyro 0 as the fetch leaves it
        c = rng.integers(0, 400, 6)
        c[3] = corners
        n6.append(c)
        rows.append((status, 0, 7, 0, 0, 0.0, 0.0))
    return np.array(n6, np.int32), np.array(rows, M.IMU_INTERVAL_DTYPE)


def _rows_tuple(rows, i):
    return (int(rows["status"][i]), int(rows["n"][i]), float(rows["front_gyro_z"][i]), float(rows["back_gyro_z"][i]))


def _as_array(M, tuples):
    return np.array(tuples, dtype=M.POSE_INGEST_ROW_DTYPE)


@pytest.mark.parametrize("velo_only", [0, 1])
@pytest.mark.parametrize("thresholds", [(0.3, 1.5), (0.5, 1.25)])
def test_truth_table_against_the_restated_rules(M, velo_only, thresholds):
    hth, vth = thresholds
    n6, rows = _table(M, hth, vth)
    F = len(n6)
    assert F > 1200 and np.isnan(rows["front_gyro_z"]).sum() >= 60 and (rows["n"] == 0).sum() == 10
    opts = dict(hori_rotate_th=hth, velo_rotate_th=vth, velo_only_mode=velo_only)
    # rows given, no first frame
    base = [expected_row(M, n6[i], _rows_tuple(rows, i), False, hth, vth, velo_only) for i in range(F)]
    got = M.pose_ingest_plan(n6, rows, **opts)
    assert got.tobytes() == _as_array(M, base).tobytes()
    dec = got["decision"]
    assert set(dec) == ({0, 2} if velo_only else {0, 1, 2})
    want_reasons = {M.INGEST_WHY_VELO_ONLY_MODE} if velo_only else {M.INGEST_WHY_MERGED, M.INGEST_WHY_FAST_ROTATION, M.INGEST_WHY_FEW_CORNERS}
    assert set(got["reason"][dec != 2]) == want_reasons and set(got["reason"][dec == 2]) == {M.INGEST_WHY_FETCH + s for s in range(1, 6)}
    assert set(got["fast_rotation"]) == {0, 1}
    # exactly at a threshold the strict comparisons are both false
    at = (np.abs(rows["front_gyro_z"]) == hth) & (np.abs(rows["back_gyro_z"]) == hth) & (rows["n"] > 0)
    assert at.sum() == 12 and (got["decision"][at] == 0).all() and (got["fast_rotation"][at] == 0).all()
    atv = (np.abs(rows["front_gyro_z"]) == vth) & (np.abs(rows["back_gyro_z"]) == vth)
    assert atv.sum() == 12 and (got["fast_rotation"][atv] == 0).all()
    # every frame in turn as the first frame: only its own row changes (a dropped frame stays dropped)
    base_rows = _as_array(M, base)
    for i in range(F):
        want = base_rows.copy()
        want[i] = expected_row(M, n6[i], _rows_tuple(rows, i), True, hth, vth, velo_only)
        g = M.pose_ingest_plan(n6, rows, first_frame=i, **opts)
        assert g.tobytes() == want.tobytes(), i
    # rows == NULL: no gate at all, first frame or not
    none = [expected_row(M, n6[i], None, False, hth, vth, velo_only) for i in range(F)]
    for first in (-1, 0, F - 1):
        g = M.pose_ingest_plan(n6, None, first_frame=first, **opts)
        assert g.tobytes() == _as_array(M, none).tobytes()
        assert (g["decision"] == 0).all() and (g["reason"] == M.INGEST_WHY_NO_IMU).all() and (g["fast_rotation"] == 0).all()


def test_counts_follow_the_input_table(M):
    n6, rows = _table(M, 0.3, 1.5)
    got = M.pose_ingest_plan(n6, rows)
    merged, dropped = got["decision"] == M.INGEST_MERGED, got["decision"] == M.INGEST_DROPPED
    only = got["decision"] == M.INGEST_VELO_ONLY
    assert merged.sum() > 100 and only.sum() > 100 and dropped.sum() == 10
    assert np.array_equal(got["n_velo"][merged], n6[merged, 2]) and np.array_equal(got["n_points"][merged], n6[merged, 2] + n6[merged, 5])
    assert np.array_equal(got["n_velo"][only], n6[only, 2]) and np.array_equal(got["n_points"][only], n6[only, 2])
    assert (got["n_points"][dropped] == 0).all() and (got["n_velo"][dropped] == 0).all()
    assert (got["_pad"] == 0).all()
    # the four feature clouds count for nothing but livox_corner_num
    n2 = n6.copy()
    n2[:, [0, 1, 4]] += 1000
    assert M.pose_ingest_plan(n2, rows).tobytes() == got.tobytes()


def test_argument_errors_leave_out_untouched(M):
    L = M.lib()
    n6 = np.array([[1, 2, 30, 150, 5, 60], [0, 0, 10, 0, 0, 20], [3, 3, 3, 3, 3, 3]], np.int32)
    rows = np.zeros(3, M.IMU_INTERVAL_DTYPE)
    rows["n"] = 4
    o = M.pose_ingest_opts()

    def call(count, n, r, opts, out=True):
        buf = np.full(4 * M.POSE_INGEST_ROW_DTYPE.itemsize, FILL, np.uint8)
        rc = L.mml_pose_ingest_plan(C.c_int(count), _p(n), _p(r), C.byref(opts) if opts is not None else None, _p(buf) if out else None)
        return rc, buf
    rc, buf = call(3, n6, rows, o)
    assert rc == M.MML_OK and (buf[:72] != FILL).any() and (buf[72:] == FILL).all()     # three rows written, not a byte more
    for count in (0, -1, M.POSE_INGEST_MAX + 1):
        rc, buf = call(count, n6, rows, o)
        assert rc == M.MML_ERR_INVALID and (buf == FILL).all(), count
    for n, opts in ((None, o), (n6, None)):
        rc, buf = call(3, n, rows, opts)
        assert rc == M.MML_ERR_INVALID and (buf == FILL).all()
    assert call(3, n6, rows, o, out=False)[0] == M.MML_ERR_INVALID
    for frame, k in ((0, 0), (1, 2), (2, 5), (2, 3)):                                    # a negative count anywhere in the table
        bad = n6.copy()
        bad[frame, k] = -1
        rc, buf = call(3, bad, rows, o)
        assert rc == M.MML_ERR_INVALID and (buf == FILL).all(), (frame, k)
    for first in (-2, 3, 100):
        rc, buf = call(3, n6, rows, M.pose_ingest_opts(first_frame=first))
        assert rc == M.MML_ERR_INVALID and (buf == FILL).all(), first
    for first in (-1, 0, 2):
        assert call(3, n6, rows, M.pose_ingest_opts(first_frame=first))[0] == M.MML_OK
    badrows = rows.copy()
    badrows["n"][1] = -1
    rc, buf = call(3, n6, badrows, o)
    assert rc == M.MML_ERR_INVALID and (buf == FILL).all()
    # the device call without a context
    assert L.mml_pose_ingest_batch(None, 0, 3, None, _p(n6), _p(rows), C.byref(o), _p(np.zeros(3, M.POSE_INGEST_ROW_DTYPE))) == M.MML_ERR_INVALID
    # the wrapper raises what the library returns
    with pytest.raises(M.MmlError) as ei:
        M.pose_ingest_plan(n6, rows, first_frame=3)
    assert ei.value.code == M.MML_ERR_INVALID
    with pytest.raises(ValueError):
        M.pose_ingest_plan(n6, rows[:2])
    with pytest.raises(TypeError):
        M.pose_ingest_plan(n6, rows, hori_rotate=0.2)


def test_declared_in_the_header_exported_and_defaults(M):
    text = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"\bint\s+(mml_[a-z0-9_]+)\s*\(", src)
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert declared.count(name) == 1, name
        assert name in exported, name
    assert len(re.findall(r"\bvoid\s+mml_pose_ingest_opts_default\s*\(", src)) == 1 and "mml_pose_ingest_opts_default" in exported
    assert "k_pose_ingest_decode" in subprocess.run(["strings", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    o = M.pose_ingest_opts()
    assert (o.hori_rotate_th, o.velo_rotate_th, o.velo_only_mode, o.first_frame) == (0.3, 1.5, 0, -1)
    assert C.sizeof(M.PoseIngestOpts) == 24 and M.POSE_INGEST_ROW_DTYPE.itemsize == 24
    # the enums of the header are the wrapper's constants
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(MML_INGEST_[A-Z_]+)\s*=\s*(\d+)", src))
    for name, value in enum.items():
        assert getattr(M, name[4:]) == value, name
    assert len(enum) == 10
    assert re.search(r"typedef struct \{ int decision, reason, fast_rotation, n_points, n_velo, _pad; \} mml_pose_ingest_row;", src)
    assert callable(M.Context.pose_ingest) and callable(M.pose_ingest_plan)
    odo = __import__("importlib").import_module("multi-modal-loam_amd.odometry")
    assert callable(odo.ingest_union_clouds)
    internal = open(os.path.join(os.path.dirname(M.LIB_PATH), "csrc", "pose_ingest.h")).read()
    assert re.search(r"#define\s+MML_POSE_INGEST_MAX\s+%d\b" % M.POSE_INGEST_MAX, internal)


def test_abs_is_the_double_overload(M, tmp_path):
    """Which `abs` do unionPoseEstimation.cpp:747, :771 call?  Written without std:: on a double.  With <cstdlib> alone only the C
    library's abs(int) is in the global namespace (0.9 becomes 0: every rotation would pass the gate); the TU includes
    Estimator/Estimator.h -> <tf/tf.h> -> tf/LinearMath/Scalar.h -> <math.h>, and libstdc++'s <math.h> (gcc >= 6; melodic has
    7.5) adds `using std::abs;` -- the double overload wins.  Compiled here both ways; the library follows the second."""
    src = tmp_path / "ov.cpp"
    src.write_text("#include <cstdlib>\n#ifdef WITH_MATH_H\n#include <math.h>\n#endif\n#include <type_traits>\n"
                   "static_assert(std::is_same<decltype(abs(-0.9)), EXPECT>::value, \"abs\");\nint main() {}\n")

    def compiles(*flags):
        return subprocess.run(["g++", "-std=c++14", "-fsyntax-only", *flags, str(src)], capture_output=True).returncode == 0
    assert compiles("-DEXPECT=int") and not compiles("-DEXPECT=double")                                  # <cstdlib> alone
    assert compiles("-DWITH_MATH_H", "-DEXPECT=double") and not compiles("-DWITH_MATH_H", "-DEXPECT=int")  # the reference's TU
    n6 = np.array([[0, 0, 10, 500, 0, 10]], np.int32)
    rows = np.zeros(1, M.IMU_INTERVAL_DTYPE)
    rows["n"], rows["front_gyro_z"], rows["back_gyro_z"] = 5, -0.9, 0.9
    got = M.pose_ingest_plan(n6, rows, hori_rotate_th=0.5, velo_rotate_th=0.95)
    assert (got["decision"][0], got["reason"][0], got["fast_rotation"][0]) == (M.INGEST_VELO_ONLY, M.INGEST_WHY_FAST_ROTATION, 0)
    got = M.pose_ingest_plan(n6, rows, hori_rotate_th=0.95, velo_rotate_th=0.5)
    assert (got["decision"][0], got["fast_rotation"][0]) == (M.INGEST_MERGED, 1)
