"""Test infrastructure only: numpy restatement of the reference's LIO initialisation, written from the reference and
Ceres 2.1.0 (not from multi-modal-loam_amd/csrc/lio_init.hip) so that the two can check each other.
  * gyro_integrate     IMUIntegrator::GyroIntegration            mm-loam/src/lio/IMUIntegrator.cpp:90-106
  * average_acc        -IMUIntegrator::GetAverageAcc, rescaled   IMUIntegrator.cpp:168-181, unionPoseEstimation.cpp:428-432
  * gravity_residual   Cost_Initial_G                            mm-loam/include/utils/ceresfunc.h:626-652
  * init_imu_residual  Cost_Initialization_IMU                   ceresfunc.h:654-741
  * levenberg_marquardt  ceres::Solve with default options (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
                       local_parameterization.cc QuaternionParameterization)
  * try_map_initialization  TryMAPInitialization              unionPoseEstimation.cpp:425-625
The Jacobians are analytic (derived here from the functors); tests/test_lio_init.py checks them against central
differences.  Quaternions are (x, y, z, w) except the gravity solve's parameter block, which is Ceres's (w, x, y, z)."""
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation as Rsc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import imu_oracle as IO  # noqa: E402

GNORM = 9.805
G_I = np.array([0.0, 0.0, -GNORM])


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    return Rsc.from_rotvec(np.asarray(w, dtype=np.float64)).as_matrix()


def log_so3(R):
    return Rsc.from_matrix(R).as_rotvec()


def Jr(w):
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-6:
        return np.eye(3) - 0.5 * K + K @ K / 6.0
    return np.eye(3) - (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K


def Jr_inv(w):
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-6:
        return np.eye(3) + 0.5 * K + K @ K / 12.0
    return np.eye(3) + 0.5 * K + (1.0 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))) * K @ K


def quat_matrix(q):
    """Eigen::Quaterniond::toRotationMatrix, q = (x, y, z, w)."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_quat(m):
    """Eigen's Matrix3d -> Quaterniond (quaternionbase_assign_impl), (x, y, z, w)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def sophus_exp(w):
    """Sophus::SO3d::exp(w).matrix(): the unit quaternion (sin(th/2)/th w, cos(th/2)), then toRotationMatrix."""
    th2 = float(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th2 < 1e-20:
        im, re = 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, 1.0 - th2 / 8.0 + th2 * th2 / 384.0
    else:
        th = np.sqrt(th2)
        im, re = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    return quat_matrix([im * w[0], im * w[1], im * w[2], re])


def _mul3(A, B):
    """3 x 3 product with Eigen's lazy-product order of the sums, (a0 b0 + a1 b1) + a2 b2."""
    C = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
    return C


def gyro_integrate(samples, dq):
    """GyroIntegration: dq (x, y, z, w) advanced by every message, dq = normalized(Quaterniond(dq.matrix() * exp(gyr dt)))
    with the sign of w made non-negative.  dt < 0 is the ROS_ASSERT: ValueError."""
    samples = np.asarray(samples, dtype=np.float64).reshape(-1, 7)
    if np.any(samples[:, 6] < 0):
        raise ValueError("dt < 0")
    q = np.asarray(dq, dtype=np.float64).copy()
    for m in samples:
        qr = matrix_quat(_mul3(quat_matrix(q), sophus_exp(m[0:3] * m[6])))
        if qr[3] < 0:
            qr = -qr
        q = qr / np.linalg.norm(qr)
    return q


def average_acc(samples0):
    s = np.asarray(samples0, dtype=np.float64).reshape(-1, 7)[:31]
    a = -(s[:, 3:6] * GNORM).sum(0) / len(s)
    return a * GNORM / np.linalg.norm(a)


def gravity_residual(q, acc, jac=False):
    """Cost_Initial_G for q = (w, x, y, z), not normalised: v + 2 w (u x v) + 2 u x (u x v) - acc.  Jacobian 3 x 4."""
    w, u, v = q[0], np.asarray(q[1:4]), G_I
    r = v + 2 * w * np.cross(u, v) + 2 * np.cross(u, np.cross(u, v)) - acc
    if not jac:
        return r
    J = np.zeros((3, 4))
    J[:, 0] = 2 * np.cross(u, v)
    J[:, 1:] = -2 * w * hat(v) + 2 * ((u @ v) * np.eye(3) + np.outer(u, v) - 2 * np.outer(v, u))
    return r, J


def quat_plus(x, d):
    """QuaternionParameterization::Plus on (w, x, y, z)."""
    nd = np.linalg.norm(d)
    if nd == 0:
        return np.array(x, dtype=np.float64)
    z = np.concatenate([[np.cos(nd)], np.sin(nd) / nd * np.asarray(d)])
    w0, x0, y0, z0 = z
    w1, x1, y1, z1 = x
    return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                     w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])


def quat_plus_jacobian(x):
    w, a, b, c = x
    return np.array([[-a, -b, -c], [w, c, -b], [-c, w, a], [b, -a, w]])


def sqrt_info9(pre_cov):
    return np.linalg.cholesky(np.linalg.inv(np.asarray(pre_cov)[:9, :9])).T


def _pre(p):
    """ctypes ImuPreint or imu_oracle.preintegrate dict -> dict."""
    if isinstance(p, dict):
        return p
    from scipy.spatial.transform import Rotation
    return dict(dp=np.array(p.dp), dv=np.array(p.dv), dR=Rotation.from_quat(np.array(p.dq)).as_matrix(), dtime=p.dtime,
                bg=np.array(p.bg), ba=np.array(p.ba), jacobian=np.array(p.jacobian).reshape(15, 15),
                covariance=np.array(p.covariance).reshape(15, 15))


def init_imu_residual(pre, ri, rj, dp, rwg, vi, vj, ba, bg, jac=False):
    """Cost_Initialization_IMU with its sqrt information; Jacobian 9 x 15 [rwg | vi | vj | ba | bg]."""
    pre = _pre(pre)
    dt = pre["dtime"]
    J15 = pre["jacobian"]
    dbg, dba = np.asarray(bg) - pre["bg"], np.asarray(ba) - pre["ba"]
    Ri, Rj, Rwg = exp_so3(ri), exp_so3(rj), exp_so3(rwg)
    gw = Rwg @ G_I
    rP = Ri.T @ (dp - vi * dt - gw * dt * dt * 0.5) - (pre["dp"] + J15[0:3, 9:12] @ dbg + J15[0:3, 12:15] @ dba)
    phi = J15[3:6, 9:12] @ dbg
    E = (pre["dR"] @ exp_so3(phi)).T @ Ri.T @ Rj
    rPhi = log_so3(E)
    rV = Ri.T @ (vj - vi - gw * dt) - (pre["dv"] + J15[6:9, 9:12] @ dbg + J15[6:9, 12:15] @ dba)
    U = sqrt_info9(pre["covariance"])
    r = U @ np.concatenate([rP, rPhi, rV])
    if not jac:
        return r
    J = np.zeros((9, 15))
    dgw = -Rwg @ hat(G_I) @ Jr(rwg)           # d (exp(rwg) G_I) / d rwg
    J[0:3, 0:3] = -0.5 * dt * dt * Ri.T @ dgw
    J[6:9, 0:3] = -dt * Ri.T @ dgw
    J[0:3, 3:6] = -dt * Ri.T
    J[6:9, 3:6] = -Ri.T
    J[6:9, 6:9] = Ri.T
    J[0:3, 9:12] = -J15[0:3, 12:15]
    J[6:9, 9:12] = -J15[6:9, 12:15]
    J[0:3, 12:15] = -J15[0:3, 9:12]
    J[6:9, 12:15] = -J15[6:9, 9:12]
    J[3:6, 12:15] = -Jr_inv(rPhi) @ E.T @ Jr(phi) @ J15[3:6, 9:12]
    return r, U @ J


def levenberg_marquardt(fun, x0, quat=False):
    """ceres::Solve, default Solver::Options (LEVENBERG_MARQUARDT, 50 iterations, tolerances 1e-6 / 1e-10 / 1e-8,
    radius 1e4 (max 1e16), LM diagonal in [1e-6, 1e32], min relative decrease 1e-3, Jacobi scaling), the normal
    equations solved by Cholesky.  fun(x) -> (r, J ambient).  quat: x = (w, x, y, z) on the QuaternionParameterization.
    Returns (x, dict(iterations, successful, initial_cost, final_cost, termination))."""
    x0 = np.array(x0, dtype=np.float64)
    x = x0.copy()
    plus = quat_plus if quat else (lambda a, d: a + d)

    def full(z):
        r, Ja = fun(z)
        J = Ja @ quat_plus_jacobian(z) if quat else Ja
        g = J.T @ r
        return r, J, g, 0.5 * r @ r, np.abs(z - plus(z, -g)).max()

    r, J, g, cost, gmax = full(x)
    info = dict(iterations=0, successful=0, initial_cost=cost, termination=0)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    radius, decrease, reuse, invalid = 1e4, 2.0, False, 0
    diag = None
    while True:
        if info["iterations"] >= 50:
            break
        if gmax <= 1e-10:
            info["termination"] = 1
            break
        if radius < 1e-32:
            break
        info["iterations"] += 1
        Js = J * scale
        if not reuse:
            diag = np.clip((Js * Js).sum(0), 1e-6, 1e32)
        reuse = True
        try:
            L = np.linalg.cholesky(Js.T @ Js + np.diag(diag / radius))
            step = -np.linalg.solve(L.T, np.linalg.solve(L, Js.T @ r))
            valid = bool(np.all(np.isfinite(step)))
        except np.linalg.LinAlgError:
            valid = False
        if valid:
            mr = Js @ step
            mcc = -(mr @ (r + mr / 2.0))
            valid = mcc > 0
        if not valid:
            invalid += 1
            if invalid >= 5:
                x, info["termination"] = x0.copy(), 4
                break
            radius /= decrease
            decrease *= 2
            continue
        invalid = 0
        xc = plus(x, step * scale)
        rc = fun(xc)[0]
        cc = 0.5 * rc @ rc
        if np.linalg.norm(x - xc) <= 1e-8 * (np.linalg.norm(x) + 1e-8):
            info["termination"] = 2
            break
        if abs(cost - cc) <= 1e-6 * cost:
            info["termination"] = 3
            break
        rho = (cost - cc) / mcc
        if rho > 1e-3:
            x = xc
            r, J, g, cost, gmax = full(x)
            info["successful"] += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2 * rho - 1) ** 3))
            decrease, reuse = 2.0, False
        else:
            radius /= decrease
            decrease *= 2
    info["final_cost"] = cost
    return x, info


def joint_problem(frames, pres, prior_r, prior_v, exTlb):
    """Residuals and Jacobian of the joint problem over z = [r_wg | b_a | b_g | v_0 .. v_{n-1}] (:498-566)."""
    n = len(frames)
    exR, exP = exTlb[:3, :3], exTlb[:3, 3]
    pb = [fr["P"] + quat_matrix(fr["Q"]) @ exP for fr in frames]
    rb = [log_so3(quat_matrix(fr["Q"]) @ exR) for fr in frames]
    nx = 9 + 3 * n

    def fun(z):
        rs, Js = [], []
        E = exp_so3(z[:3]).T @ exp_so3(prior_r)
        e = log_so3(E)
        rs.append(2000.0 * e)
        Jrow = np.zeros((3, nx))
        Jrow[:, 0:3] = -2000.0 * Jr_inv(e) @ E.T @ Jr(z[:3])
        Js.append(Jrow)
        for off, s, prior in ((3, 1000.0, np.zeros(3)), (6, 4000.0, np.zeros(3))) + tuple(
                (9 + 3 * i, 4000.0, prior_v[i]) for i in range(n)):
            rs.append(s * (z[off:off + 3] - prior))
            Jrow = np.zeros((3, nx))
            Jrow[:, off:off + 3] = s * np.eye(3)
            Js.append(Jrow)
        for i in range(1, n):
            vi, vj = z[9 + 3 * (i - 1):12 + 3 * (i - 1)], z[9 + 3 * i:12 + 3 * i]
            r, J = init_imu_residual(pres[i], rb[i - 1], rb[i], pb[i] - pb[i - 1], z[:3], vi, vj, z[3:6], z[6:9], jac=True)
            rs.append(r)
            Jrow = np.zeros((9, nx))
            for b, col in enumerate((0, 9 + 3 * (i - 1), 9 + 3 * i, 3, 6)):
                Jrow[:, col:col + 3] += J[:, 3 * b:3 * b + 3]
            Js.append(Jrow)
        return np.concatenate(rs), np.vstack(Js)

    return fun, pb


def try_map_initialization(frames, samples, exTlb, pres=None):
    """TryMAPInitialization on a list of frame dicts (t, P, Q x y z w, V, bg, ba), changed in place like the reference's
    list; samples: list of the frames' IMU message arrays; pres: list of the frames' pre-integrations (imu_oracle dicts,
    entry 0 unused) or None (frame i pre-integrated with frame i-1's biases).  Returns a dict with ok, status,
    fail_frame, gravity, q_wg (x y z w), r_wg, ba, bg, the two solves' infos, pres (after the redo) and keep_from."""
    n = len(frames)
    exTlb = np.asarray(exTlb, dtype=np.float64)
    if pres is None:
        pres = [None] + [IO.preintegrate(samples[i], frames[i - 1]["bg"], frames[i - 1]["ba"]) for i in range(1, n)]
    pres = list(pres)
    acc = average_acc(samples[0])
    qx, ginfo = levenberg_marquardt(lambda q: gravity_residual(q, acc, jac=True), [1.0, 0.0, 0.0, 0.0], quat=True)
    q_wg = np.array([qx[1], qx[2], qx[3], qx[0]])
    prior_r = log_so3(quat_matrix(q_wg))
    exP = exTlb[:3, 3]
    prior_v = [None] * n
    for i in range(1, n):
        prior_v[i] = (frames[i]["P"] - frames[i - 1]["P"] + quat_matrix(frames[i]["Q"]) @ exP
                      - quat_matrix(frames[i - 1]["Q"]) @ exP) / (frames[i]["t"] - frames[i - 1]["t"])
    prior_v[0] = prior_v[1]
    fun, _ = joint_problem(frames, pres, prior_r, prior_v, exTlb)
    z0 = np.concatenate([np.zeros(9)] + list(prior_v))
    z, jinfo = levenberg_marquardt(fun, z0)
    out = dict(ok=False, status=0, fail_frame=-1, gravity=exp_so3(z[:3]) @ G_I, q_wg=q_wg, r_wg=z[:3].copy(), ba=z[3:6].copy(),
               bg=z[6:9].copy(), average_acc=acc, gravity_info=ginfo, joint_info=jinfo, pres=pres, keep_from=0, prior_v=prior_v)
    if np.linalg.norm(z[3:6]) > 0.5 or np.linalg.norm(z[6:9]) > 0.5:
        out["status"] = 1
        return out
    for i in range(n):
        frames[i]["ba"], frames[i]["bg"] = z[3:6].copy(), z[6:9].copy()
        v = z[9 + 3 * i:12 + 3 * i].copy()
        if np.linalg.norm(v - prior_v[i]) > 2.0:
            out["status"], out["fail_frame"] = 2, i
            return out
        frames[i]["V"] = v
    for i in range(n - 1):
        pres[i + 1] = IO.preintegrate(samples[i + 1], frames[i]["bg"], frames[i]["ba"])
    keep = max(0, n - 5)
    del frames[:keep]
    R = quat_matrix(frames[-1]["Q"])
    frames[-1]["P"] = frames[-1]["P"] + R @ exP
    frames[-1]["Q"] = matrix_quat(R @ exTlb[:3, :3])
    out.update(ok=True, keep_from=keep, pres=[None] + pres[1 + keep:])
    return out
