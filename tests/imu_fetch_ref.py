"""The yardstick of the IMU queue tests: fetchImuMsgs (unionPoseEstimation.cpp:307-395) restated as the sequential walk it is,
over a Python list of messages, with its trim (:383-390) and the frame prediction of process() (:779-780, :805-828) in numpy.
Written from the reference's lines, not from the library's searches: `imu_idx` walks from 0 and every comparison is the one
the line makes.  Python floats are IEEE doubles and nothing here is fused, so the rows are the reference's to the byte."""
import numpy as np

OK, EMPTY, NOT_REACHED, TOO_OLD, REVERSED, NO_SAMPLE = 0, 1, 2, 3, 4, 5

INTERVAL_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("first", "<i8"), ("interpolated", "<i4"), ("_pad", "<i4"),
                           ("front_gyro_z", "<f8"), ("back_gyro_z", "<f8")])


def fetch(msgs, start, end):
    """msgs: list of (stamp, gx, gy, gz, ax, ay, az).  Returns (status, first, interpolated, rows) with rows = the messages of
    vimuMsg as [gx, gy, gz, ax, ay, az, dt], dt as PreIntegration / GyroIntegration subtract it with lastTime = start
    (IMUIntegrator.cpp:122, :97).  Where the reference reads back() of an empty vector, or walks past the end of the vector
    (end == start == the last stamp), the status is NO_SAMPLE."""
    if len(msgs) == 0:                                   # :309
        return EMPTY, 0, 0, []
    out = []                                             # vimuMsg as (stamp, six values)
    first = 0
    interpolated = 0
    current_time = 0.0
    imu_idx = 0
    status = OK
    while True:
        if end < start:                                  # :325
            status = REVERSED
            break
        if float(msgs[-1][0]) < end:                     # :332
            status = NOT_REACHED
            break
        if float(msgs[0][0]) >= end:                     # :338
            status = TOO_OLD
            break
        if imu_idx >= len(msgs):                         # _imuMsgVector[imu_idx] past the end: undefined in the reference
            status = NO_SAMPLE
            break
        m = msgs[imu_idx]
        time = float(m[0])
        if time <= end and time > start:                 # :348
            if not out:
                first = imu_idx
            out.append((time, [float(v) for v in m[1:7]]))
            current_time = time
            if time == end:                              # :353
                break
        elif time <= start:                              # :355
            pass
        else:
            if not out:                                  # vimuMsg.back() of an empty vector: undefined in the reference
                status = NO_SAMPLE
                break
            dt_1 = end - current_time                    # :359
            dt_2 = time - end
            w1 = dt_2 / (dt_1 + dt_2)
            w2 = dt_1 / (dt_1 + dt_2)
            back = out[-1][1]
            out.append((end, [w1 * back[c] + w2 * float(m[1 + c]) for c in range(6)]))   # stamp: fromSec(end), see the header
            interpolated = 1
            break
        imu_idx += 1
    if status != OK:
        return status, 0, 0, []
    rows = []
    last = start
    for t, v in out:
        rows.append(v + [t - last])
        last = t
    return OK, first, interpolated, rows


def fetch_batch(msgs, t_start, t_end):
    """What mml_imu_fetch_host returns for the same arguments: rows (INTERVAL_DTYPE), offsets, samples."""
    msgs = [tuple(float(v) for v in m) for m in np.asarray(msgs, dtype=np.float64).reshape(-1, 7)]
    n = len(t_start)
    rows = np.zeros(n, INTERVAL_DTYPE)
    offsets = np.zeros(n + 1, np.int32)
    samples = []
    for i in range(n):
        status, first, interp, r = fetch(msgs, float(t_start[i]), float(t_end[i]))
        rows[i] = (status, len(r), first, interp, 0, r[0][2] if r else 0.0, r[-1][2] if r else 0.0)
        offsets[i + 1] = offsets[i] + len(r)
        samples += r
    return rows, offsets, np.array(samples, dtype=np.float64).reshape(-1, 7)


def drop_before(stamps, front, t, keep_min):
    """:383-390 on the live stamps stamps[front:]: the new front."""
    tail = len(stamps)
    while tail - front > keep_min and stamps[front] < t:
        front += 1
    return front


# ---- the prediction, :805-828 and :779-780, in numpy (quaternions x, y, z, w) -------------------------------------------------
def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _qmul(a, b):
    av, bv = np.asarray(a[:3]), np.asarray(b[:3])
    v = a[3] * bv + b[3] * av + np.cross(av, bv)
    return np.array([v[0], v[1], v[2], a[3] * b[3] - av @ bv])


def _quat_from_matrix(R):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    return q if q[3] >= 0 else -q


def predict_lio(prev, dq, dp, dv, exTlb):
    """state (P, Q, V), velo_delta_Rl, velo_delta_tl.  Rotations of vectors go through the rotation matrix, products through
    the Hamilton formula with numpy's cross / dot: another operation order than the library's."""
    P0, Q0, V0 = np.asarray(prev[:3]), np.asarray(prev[3:7]), np.asarray(prev[7:10])
    R0 = _qmat(Q0)
    exRbl = exTlb[:3, :3].T
    exPbl = -exRbl @ exTlb[:3, 3]
    qbl = _quat_from_matrix(exRbl)
    Q = _qmul(Q0, dq)
    P = P0 + R0 @ np.asarray(dp)
    V = V0 + R0 @ np.asarray(dv)
    Qwlpre = _qmul(Q0, qbl)
    Pwlpre = R0 @ exPbl + P0
    Qwl = _qmul(Q, qbl)
    Pwl = _qmat(Q) @ exPbl + P
    Rpre = _qmat(Qwlpre)
    return np.concatenate([P, Q, V]), Rpre.T @ _qmat(Qwl), Rpre.T @ (Pwl - Pwlpre)


def predict_gyro(dq, exTlb):
    Rb = _qmat(dq)
    Rlb = exTlb[:3, :3]
    return Rb, Rlb @ Rb @ Rlb.T
