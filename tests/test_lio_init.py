"""CPU suite for the LIO initialisation that opens full-window mode (TryMAPInitialization, GyroIntegration,
GetAverageAcc, Cost_Initialization_IMU): the C-ABI against the independent numpy restatement in tests/lio_init_ref.py,
central differences and scipy's least-squares solver."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation as Rsc

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import imu_oracle as IO  # noqa: E402
import lio_init_ref as LR  # noqa: E402

GN = 9.805
KEYS = ("P", "Q", "V", "bg", "ba")


def _exTlb():
    T = np.eye(4)
    T[:3, :3] = Rsc.from_rotvec([0.01, 0.02, -0.03]).as_matrix()
    T[:3, 3] = [0.05, -0.02, 0.1]
    return T


def _window(n=3, tilt=(0.03, -0.04, 0.0), bg=(0.002, -0.003, 0.001), ba=(0.03, -0.02, 0.04), per=60, h=0.005,
            exTlb=np.eye(4)):
    """n frames of a smooth motion (constant body rate and world acceleration, as tests/test_imu.py::_trajectory) in a
    world whose gravity is `tilt` away from -z; frame f holds the `per` IMU samples before its time stamp, measured
    with constant biases.  P, Q are the lidar poses (world <- lidar) for the extrinsic exTlb."""
    gw = Rsc.from_rotvec(tilt).as_matrix() @ np.array([0.0, 0.0, -GN])
    w_body, a_world = np.array([0.05, -0.03, 0.2]), np.array([0.3, -0.2, 0.05])
    P0, V0 = np.array([1.0, 2.0, 0.5]), np.array([0.5, 0.1, -0.05])
    R0 = Rsc.from_rotvec([0.0, 0.0, 0.3]).as_matrix()

    def body(t):
        return P0 + V0 * t + 0.5 * a_world * t * t, V0 + a_world * t, R0 @ Rsc.from_rotvec(w_body * t).as_matrix()

    T = per * h
    frames, samples = [], []
    for f in range(n):
        t = T * (f + 1)
        P, V, R = body(t)
        smp = []
        for k in range(per):       # forward Euler: the sample holds over the following dt
            Rk = body(t - T + k * h)[2]
            smp.append(np.concatenate([w_body + bg, (Rk.T @ (a_world - gw) + ba) / GN, [h]]))
        Tb = np.eye(4)
        Tb[:3, :3], Tb[:3, 3] = R, P
        Tl = Tb @ np.linalg.inv(exTlb)
        frames.append(dict(t=t, P=Tl[:3, 3].copy(), Q=Rsc.from_matrix(Tl[:3, :3]).as_quat(), V=np.zeros(3), bg=np.zeros(3),
                           ba=np.zeros(3), V_true=V))
        samples.append(np.array(smp))
    return frames, samples, gw


def _copy(frames):
    return [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()} for f in frames]


def _run_c(M, frames, samples, exTlb, pre=None):
    return M.lio_initialize([f["t"] for f in frames], *[[f[k] for f in frames] for k in KEYS], samples, exTlb, pre)


def test_gyro_integration_matches_numpy_restatement(M):
    rng = np.random.default_rng(0)
    for trial in range(20):
        n = int(rng.integers(1, 60))
        smp = np.concatenate([rng.normal(0, 0.8, (n, 3)), rng.normal(0, 1, (n, 3)), rng.uniform(0.0, 0.01, (n, 1))], axis=1)
        dq0 = np.array([0.0, 0.0, 0.0, 1.0]) if trial == 0 else Rsc.random(random_state=trial).as_quat()
        if dq0[3] < 0:
            dq0 = -dq0
        got, ref = M.imu_gyro_integrate(smp, dq0), LR.gyro_integrate(smp, dq0)
        # an ulp or two per message (libm's sin / cos in numpy, fdlibm's in imu_math.h) accumulates over up to 60
        # messages: observed at most 3.1e-15 over 200 such runs, hence 4e-15 rather than 1e-15
        assert np.abs(got - ref).max() <= 4e-15, (trial, np.abs(got - ref).max())
        assert got[3] >= 0 and abs(np.linalg.norm(got) - 1) < 1e-15
    # accumulation: two calls equal one over the concatenation (dq is not reset)
    smp = np.concatenate([rng.normal(0, 0.5, (30, 3)), np.zeros((30, 3)), np.full((30, 1), 0.005)], axis=1)
    two = M.imu_gyro_integrate(smp[15:], M.imu_gyro_integrate(smp[:15]))
    assert np.array_equal(two, M.imu_gyro_integrate(smp))
    # a rotation past pi: Quaterniond(dq * dR) comes out with w < 0 and is flipped
    big = np.array([[0.0, 0.0, 20.0, 0, 0, 1, 0.1], [0.0, 0.0, 20.0, 0, 0, 1, 0.1]])
    got = M.imu_gyro_integrate(big)
    q = LR.matrix_quat(LR.quat_matrix([0.0, 0.0, 0.0, 1.0]) @ LR.exp_so3([0, 0, 2.0]))
    assert LR.matrix_quat(LR.quat_matrix(q) @ LR.exp_so3([0, 0, 2.0]))[3] < 0     # the flip is exercised
    assert np.abs(got - LR.gyro_integrate(big, [0, 0, 0, 1.0])).max() <= 4e-15 and got[3] >= 0
    assert np.allclose(Rsc.from_quat(got).as_rotvec(), Rsc.from_rotvec([0, 0, 4.0]).as_rotvec(), atol=1e-12)
    # dt < 0 is refused (the reference's ROS_ASSERT) and leaves dq alone
    bad = smp.copy()
    bad[7, 6] = -1e-4
    dq = np.array([0.1, 0.2, 0.3, 0.9])
    with pytest.raises(M.MmlError) as e:
        M.imu_gyro_integrate(bad, dq)
    assert e.value.code == M.MML_ERR_INVALID
    with pytest.raises(ValueError):
        LR.gyro_integrate(bad, dq)


def test_init_factor_residual_and_analytic_jacobian(M):
    rng = np.random.default_rng(4)
    frames, samples, _ = _window(2)
    for trial in range(5):
        lin_bg, lin_ba = rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)
        pre = M.imu_preintegrate(samples[1], lin_bg, lin_ba)
        ri, rj = rng.normal(0, 0.5, 3), rng.normal(0, 0.5, 3)
        dp, rwg = rng.normal(0, 0.3, 3), rng.normal(0, 0.1, 3)
        vi, vj, ba, bg = rng.normal(0, 1, 3), rng.normal(0, 1, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)
        r, J = M.imu_init_factor(pre, ri, rj, dp, rwg, vi, vj, ba, bg)
        r_ref, J_ref = LR.init_imu_residual(pre, ri, rj, dp, rwg, vi, vj, ba, bg, jac=True)
        assert np.abs(r - r_ref).max() <= 1e-12 * np.abs(r_ref).max(), np.abs(r - r_ref).max()

        def f(z):
            return M.imu_init_factor(pre, ri, rj, dp, z[0:3], z[3:6], z[6:9], z[9:12], z[12:15], jac=False)[0]

        z0 = np.concatenate([rwg, vi, vj, ba, bg])
        Jn = IO.numeric_jacobian(f, z0, h=1e-6)
        assert np.abs(J - Jn).max() <= 1e-6 * np.abs(Jn).max(), np.abs(J - Jn).max() / np.abs(Jn).max()
        assert np.abs(J - J_ref).max() <= 1e-9 * np.abs(J_ref).max()


@pytest.mark.parametrize("tilt_deg", [0.0, 2.5, 7.5, 15.0, 40.0, 60.0, 179.0])
def test_gravity_solve(M, tilt_deg):
    """Cost_Initial_G on the quaternion manifold from para_quat = (1, 0, 0, 0): q_wg rotates (0, 0, -9.805) onto the
    average acceleration to within what the solver's tolerances leave, and q_wg / the iteration counts equal the numpy
    LM restatement.  Observed over tilts 0-60 deg (3 axes, 2.5 deg steps): the solve stops on the parameter tolerance
    with |q_wg g - average_acc| up to 1.6e-7 (1.7e-8 of |g|), and q_wg within 3.3e-13 of the restatement; 175-179.5 deg
    away from the start the problem is near its antipodal saddle and the two agree to 6.7e-9."""
    axis = np.array([0.6, -0.8, 0.0]) if tilt_deg < 100 else np.array([0.3, 0.9, 0.1]) / np.linalg.norm([0.3, 0.9, 0.1])
    g_dir = Rsc.from_rotvec(np.radians(tilt_deg) * axis).as_matrix() @ np.array([0, 0, -1.0])
    rng = np.random.default_rng(int(tilt_deg * 10))
    # frame 0's messages: specific force = -gravity (at rest) plus noise; 40 messages (GetAverageAcc reads the first 31)
    acc = np.tile(-g_dir, (40, 1)) + rng.normal(0, 0.01, (40, 3))
    smp0 = np.concatenate([np.zeros((40, 3)), acc, np.full((40, 1), 0.005)], axis=1)
    frames, samples, _ = _window(3)
    samples[0] = smp0
    res, _, _ = _run_c(M, frames, samples, np.eye(4))
    avg = LR.average_acc(smp0)
    assert np.abs(np.array(res.average_acc) - avg).max() <= 1e-13
    qx = np.array([res.q_wg[3], res.q_wg[0], res.q_wg[1], res.q_wg[2]])
    assert np.linalg.norm(LR.gravity_residual(qx, avg)) <= 5e-7
    q_ref, info = LR.levenberg_marquardt(lambda q: LR.gravity_residual(q, avg, jac=True), [1.0, 0, 0, 0], quat=True)
    assert np.abs(qx - q_ref).max() <= (1e-12 if tilt_deg <= 60 else 1e-8), np.abs(qx - q_ref).max()
    gs = res.gravity_solve
    assert (gs.iterations, gs.successful, gs.termination) == (info["iterations"], info["successful"], info["termination"])
    assert gs.termination in (1, 2, 3)
    cz = 1.0 - 2.0 * (qx[1] ** 2 + qx[2] ** 2)        # (R_wg e_z)_z: the tilt q_wg found ...
    assert abs(cz - (-avg[2] / GN)) < 1e-7              # ... is the tilt of the average acceleration


def _scipy_joint(frames, samples, exTlb, res):
    """The same joint problem minimised to convergence by scipy (xtol / ftol 1e-15)."""
    n = len(frames)
    pres = [None] + [IO.preintegrate(samples[i], np.zeros(3), np.zeros(3)) for i in range(1, n)]
    q = np.array(res.q_wg)
    prior_r = LR.log_so3(LR.quat_matrix(q))
    exP = exTlb[:3, 3]
    prior_v = [None] * n
    for i in range(1, n):
        prior_v[i] = (frames[i]["P"] - frames[i - 1]["P"] + LR.quat_matrix(frames[i]["Q"]) @ exP
                      - LR.quat_matrix(frames[i - 1]["Q"]) @ exP) / (frames[i]["t"] - frames[i - 1]["t"])
    prior_v[0] = prior_v[1]
    fun, _ = LR.joint_problem(frames, pres, prior_r, prior_v, exTlb)
    z0 = np.concatenate([np.zeros(9)] + prior_v)
    sol = least_squares(lambda z: fun(z)[0], z0, jac=lambda z: fun(z)[1], xtol=1e-15, ftol=1e-15, gtol=1e-15, method="lm")
    return sol.x, 0.5 * sol.fun @ sol.fun


@pytest.mark.parametrize("n,tilt,ex", [(3, (0.03, -0.04, 0.0), False), (3, (0.0, 0.05, 0.01), True), (5, (-0.02, 0.03, 0.0), True)])
def test_joint_solve_matches_numpy_lm_and_scipy(M, n, tilt, ex):
    exTlb = _exTlb() if ex else np.eye(4)
    frames, samples, gw = _window(n, tilt=tilt, exTlb=exTlb)
    res, st, _ = _run_c(M, _copy(frames), samples, exTlb)
    ref = LR.try_map_initialization(_copy(frames), samples, exTlb)
    assert res.status == 0 and ref["ok"]
    js, ji = res.joint_solve, ref["joint_info"]
    assert (js.iterations, js.successful, js.termination) == (ji["iterations"], ji["successful"], ji["termination"])
    for a, b in ((res.r_wg, ref["r_wg"]), (res.ba, ref["ba"]), (res.bg, ref["bg"]), (res.gravity, ref["gravity"])):
        assert np.abs(np.array(a) - b).max() <= 1e-9, np.abs(np.array(a) - b).max()
    fr_ref = _copy(frames)
    LR.try_map_initialization(fr_ref, samples, exTlb)
    assert np.abs(st["V"] - np.array([f["V"] for f in fr_ref])).max() <= 1e-9
    # against the converged minimiser: Ceres's function tolerance stops when the cost changes by <= 1e-6 of itself
    z, cost = _scipy_joint(frames, samples, exTlb, res)
    zc = np.concatenate([res.r_wg, res.ba, res.bg, st["V"].reshape(-1)])
    assert js.final_cost >= cost * (1 - 1e-12) and js.final_cost - cost <= 1e-6 * js.final_cost
    # observed on these three windows: |z - z_scipy| 1.5e-7 / 1.4e-6 / 1.8e-6, cost above the minimum by 3.6e-11 / 2.2e-9 /
    # 2.3e-9 of itself (the solve stops on the function tolerance after 3 iterations)
    assert np.abs(zc - z).max() <= 1e-5, np.abs(zc - z).max()
    # the recovered gravity is close to the tilted truth (the prior on r is the first frame's body-frame acceleration)
    ang = np.degrees(np.arccos(np.clip(np.dot(res.gravity, gw) / (GN * np.linalg.norm(res.gravity)), -1, 1)))
    assert ang < 3.0, ang


def test_bias_failure_writes_nothing(M):
    frames, samples, _ = _window(3)
    samples = [s.copy() for s in samples]
    for s in samples[1:]:
        s[:, 3:6] += 30.0 / GN        # a specific force the lidar motion cannot explain: b_a absorbs it
    fr = _copy(frames)
    for f in fr:
        f["V"] = np.array([0.1, 0.2, 0.3])
    before = _copy(fr)
    res, st, _ = _run_c(M, fr, samples, np.eye(4))
    ref = LR.try_map_initialization(_copy(fr), samples, np.eye(4))
    assert res.status == 1 and ref["status"] == 1 and res.fail_frame == -1
    assert np.linalg.norm(res.ba) > 0.5 or np.linalg.norm(res.bg) > 0.5
    for k in KEYS:
        assert np.array_equal(st[k], np.array([f[k] for f in before]))
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    fl, sl = _copy(fr), list(samples)
    ok, g, _ = odometry.try_map_initialization(fl, sl, np.eye(4))
    assert not ok and len(fl) == 3 and len(sl) == 3
    for a, b in zip(fl, before):
        for k in KEYS + ("t",):
            assert np.array_equal(a[k], b[k])


def test_velocity_failure_leaves_the_partial_state(M):
    frames, samples, _ = _window(3)
    samples = list(samples)
    # the back frame's IMU covers 15 ms of the 0.3 s between the lidar time stamps: its tight pre-integration forces
    # v_1 = lidar displacement / 15 ms, far from the prior dp / dt (frame 0 keeps a velocity near its own prior)
    samples[2] = samples[2][-3:]
    fr = _copy(frames)
    for f in fr:
        f["V"] = np.array([9.0, 9.0, 9.0])
    res, st, _ = _run_c(M, fr, samples, np.eye(4))
    ref_fr = _copy(fr)
    ref = LR.try_map_initialization(ref_fr, samples, np.eye(4))
    assert res.status == 2 and ref["status"] == 2 and res.fail_frame == ref["fail_frame"] == 1
    assert np.linalg.norm(res.ba) <= 0.5 and np.linalg.norm(res.bg) <= 0.5
    k = res.fail_frame
    for i in range(3):
        new_b = i <= k
        assert np.array_equal(st["ba"][i], np.array(res.ba) if new_b else np.zeros(3))
        assert np.array_equal(st["bg"][i], np.array(res.bg) if new_b else np.zeros(3))
        if i < k:
            assert not np.array_equal(st["V"][i], [9.0, 9.0, 9.0])
            assert np.abs(st["V"][i] - ref_fr[i]["V"]).max() <= 1e-9
        else:
            assert np.array_equal(st["V"][i], [9.0, 9.0, 9.0])
        assert np.array_equal(st["P"][i], fr[i]["P"]) and np.array_equal(st["Q"][i], fr[i]["Q"])
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    fl = _copy(fr)
    ok, _, _ = odometry.try_map_initialization(fl, list(samples), np.eye(4))
    assert not ok
    for i in range(3):
        for key in KEYS:
            assert np.array_equal(fl[i][key], st[key][i]), (i, key)


@pytest.mark.parametrize("n", [3, 7])
def test_success_state(M, n):
    """Step 7: every frame's V / biases, the pre-integrations redone with the new biases, the list trimmed to 5, only the
    back frame moved from lidar to body -- through the C-ABI, odometry.try_map_initialization and the restatement."""
    exTlb = _exTlb()
    frames, samples, _ = _window(n, exTlb=exTlb)
    res, st, pres = _run_c(M, _copy(frames), samples, exTlb)
    assert res.status == 0 and res.keep_from == max(0, n - 5)
    for i in range(n - 1):
        want = M.imu_preintegrate(samples[i + 1], st["bg"][i], st["ba"][i])
        assert bytes(pres[i + 1]) == bytes(want)
        assert np.array_equal(st["bg"][i], np.array(res.bg)) and np.array_equal(st["ba"][i], np.array(res.ba))
    for i in range(n - 1):
        assert np.array_equal(st["P"][i], frames[i]["P"]) and np.array_equal(st["Q"][i], frames[i]["Q"])
    Rl = Rsc.from_quat(frames[-1]["Q"]).as_matrix()
    assert np.allclose(st["P"][-1], frames[-1]["P"] + Rl @ exTlb[:3, 3], atol=1e-14)
    assert np.allclose(Rsc.from_quat(st["Q"][-1]).as_matrix(), Rl @ exTlb[:3, :3], atol=1e-14)
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    fl, sl = _copy(frames), list(samples)
    ok, g, pl = odometry.try_map_initialization(fl, sl, exTlb)
    keep = max(0, n - 5)
    assert ok and len(fl) == min(n, 5) and len(sl) == min(n, 5) and len(pl) == len(fl)
    assert np.array_equal(g, np.array(res.gravity))
    for j, f in enumerate(fl):
        i = j + keep
        assert f["t"] == frames[i]["t"]
        for k in KEYS:
            assert np.array_equal(f[k], st[k][i]), (i, k)
        if j >= 1:
            assert bytes(pl[j]) == bytes(pres[i]) and bytes(f["pre"]) == bytes(pres[i])
    ref_fr = _copy(frames)
    ref = LR.try_map_initialization(ref_fr, samples, exTlb)
    assert ref["ok"] and len(ref_fr) == len(fl)
    for a, b in zip(fl, ref_fr):
        for k in KEYS:
            assert np.abs(a[k] - b[k]).max() <= 1e-9, k
    for j in range(1, len(fl)):
        assert np.abs(np.array(pl[j].dp) - ref["pres"][j]["dp"]).max() <= 1e-9


def test_given_preintegrations_are_used(M):
    """A frame list that carries its own pre-integrations (the reference's IMUIntegrator state, linearised at the biases
    its predecessor had when it was pushed) is solved with those, not with ones recomputed from the current biases."""
    frames, samples, _ = _window(3)
    fr = _copy(frames)
    for f in fr:
        f["bg"], f["ba"] = np.array([0.001, 0.0, -0.001]), np.array([0.01, 0.02, 0.0])
    held = [None] + [M.imu_preintegrate(samples[i], np.zeros(3), np.zeros(3)) for i in range(1, 3)]
    r_held, _, p_held = _run_c(M, _copy(fr), samples, np.eye(4), held)
    r_own, _, p_own = _run_c(M, _copy(fr), samples, np.eye(4))
    assert bytes(p_own[1]) != bytes(M.imu_preintegrate(samples[1], np.zeros(3), np.zeros(3)))
    r_ref = LR.try_map_initialization(_copy(fr), samples, np.eye(4),
                                      [None] + [IO.preintegrate(samples[i], np.zeros(3), np.zeros(3)) for i in range(1, 3)])
    assert np.abs(np.array(r_held.ba) - r_ref["ba"]).max() <= 1e-9
    assert np.abs(np.array(r_held.ba) - np.array(r_own.ba)).max() > 1e-9


def test_lio_init_result_layout_matches_header(M, tmp_path):
    code = textwrap.dedent("""
        #include <stdio.h>
        #include <stddef.h>
        #include "mmloam_hip.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mml_lio_init_result), offsetof(mml_lio_init_result, gravity),
                 offsetof(mml_lio_init_result, q_wg), offsetof(mml_lio_init_result, average_acc), offsetof(mml_lio_init_result, ba),
                 offsetof(mml_lio_init_result, bg), offsetof(mml_lio_init_result, gravity_solve), offsetof(mml_lio_init_result, joint_solve));
          return 0; }""")
    (tmp_path / "t.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    R = M.LioInitResult
    mine = [C.sizeof(R), R.gravity.offset, R.q_wg.offset, R.average_acc.offset, R.ba.offset, R.bg.offset,
            R.gravity_solve.offset, R.joint_solve.offset]
    assert got == mine


def test_cpp_adapter_try_map_initialization_matches_python(M, tmp_path):
    """mml::TryMAPInitialization (host/mmloam_adapter.hpp) on a std::list<LidarFrame> built host-side, no device."""
    exTlb = _exTlb()
    frames, samples, _ = _window(3, exTlb=exTlb)
    data = tmp_path / "frames.txt"
    with open(data, "w") as f:
        f.write(" ".join("%.17g" % v for v in exTlb.reshape(-1)) + "\n")
        for fr, s in zip(frames, samples):
            f.write("%.17g %s %s %d\n" % (fr["t"], " ".join("%.17g" % v for v in fr["P"]), " ".join("%.17g" % v for v in fr["Q"]), len(s)))
            for row in s:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    src = tmp_path / "init_probe.cpp"
    src.write_text(textwrap.dedent(r"""
        #include <cstdio>
        #include <list>
        #include <vector>
        #include "mmloam_adapter.hpp"
        int main(int argc, char** argv) {
            FILE* f = std::fopen(argv[1], "r");
            mml::Matrix4d exTlb;
            for (int i = 0; i < 16; ++i) if (std::fscanf(f, "%lf", &exTlb.m[i]) != 1) return 2;
            std::list<mml::Estimator::LidarFrame> frames;
            std::vector<mml::IMUIntegrator> imu;
            for (int k = 0; k < 3; ++k) {
                mml::Estimator::LidarFrame fr;
                int n = 0;
                if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %d", &fr.timeStamp, &fr.P.v[0], &fr.P.v[1], &fr.P.v[2],
                                &fr.Q.x, &fr.Q.y, &fr.Q.z, &fr.Q.w, &n) != 9) return 3;
                mml::IMUIntegrator it;
                for (int i = 0; i < n; ++i) {
                    double m[7];
                    for (int j = 0; j < 7; ++j) if (std::fscanf(f, "%lf", &m[j]) != 1) return 4;
                    it.PushIMUMsg(m);
                }
                frames.push_back(fr);
                imu.push_back(it);
            }
            mml::Vector3d g;
            mml::IMUIntegrator probe = imu[1];
            probe.GyroIntegration();
            mml::Vector3d acc = imu[0].GetAverageAcc();
            bool ok = mml::TryMAPInitialization(frames, imu, exTlb, g);
            std::printf("ok %d n %zu g %.17g %.17g %.17g\n", ok ? 1 : 0, frames.size(), g.v[0], g.v[1], g.v[2]);
            std::printf("dq %.17g %.17g %.17g %.17g acc %.17g %.17g %.17g\n", probe.dq.x, probe.dq.y, probe.dq.z, probe.dq.w,
                        acc.v[0], acc.v[1], acc.v[2]);
            for (const auto& fr : frames)
                std::printf("frame %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n",
                            fr.P.v[0], fr.P.v[1], fr.P.v[2], fr.Q.x, fr.Q.y, fr.Q.z, fr.Q.w, fr.V.v[0], fr.V.v[1], fr.V.v[2],
                            fr.bg.v[0], fr.bg.v[1], fr.bg.v[2], fr.ba.v[0], fr.ba.v[1], fr.ba.v[2]);
            std::printf("pre_dp %.17g %.17g %.17g\n", imu[2].pre.dp[0], imu[2].pre.dp[1], imu[2].pre.dp[2]);
            return 0;
        }"""))
    exe = tmp_path / "init_probe"
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"), str(src), "-o", str(exe),
           "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    fl, sl = _copy(frames), list(samples)
    ok, g, pl = odometry.try_map_initialization(fl, sl, exTlb)
    head = lines[0].split()
    assert head[:4] == ["ok", "1", "n", "3"] and ok
    assert np.array_equal(np.array([float(v) for v in head[5:8]]), g)
    vals = lines[1].split()
    assert np.array_equal(np.array([float(v) for v in vals[1:5]]), M.imu_gyro_integrate(samples[1]))
    acc = -(samples[0][:31, 3:6] * GN).sum(0) / 31
    assert np.allclose(np.array([float(v) for v in vals[6:9]]), -acc, rtol=1e-15, atol=0)
    for line, fr in zip(lines[2:5], fl):
        v = np.array([float(x) for x in line.split()[1:]])
        assert np.array_equal(v, np.concatenate([fr["P"], fr["Q"], fr["V"], fr["bg"], fr["ba"]]))
    assert np.array_equal(np.array([float(v) for v in lines[5].split()[1:]]), np.array(pl[2].dp))
