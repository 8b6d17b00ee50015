"""GPU suite for the LIO initialisation: a cold start from an empty map on the device, the way the reference's pose node
brings up IMU_Mode 2 (unionPoseEstimation.cpp:774-794, 881-888, 939-985): gyro-predicted 1-frame lidar odometry, a frame
pushed every third scan, TryMAPInitialization when veloPushCount / veloStartTime allow it, then full-window estimates
with the initialisation's gravity, velocities, biases and redone pre-integrations.  The same control flow is driven by
the CPU oracle (C++ lidar restatement, numpy IMU / initialisation / window restatements) and the two must agree."""
import importlib
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import imu_oracle as IO  # noqa: E402
import lio_init_ref as LR  # noqa: E402

GN = 9.805
K0 = 0
N_SCANS = 15                     # scans K0 .. K0 + 14: initialisation at the 12th, full-window estimates at the 14th and 15th
G_MAP = Rsc.from_rotvec([0.03, -0.035, 0.0]).as_matrix() @ np.array([0.0, 0.0, -GN])   # 2.64 deg from the map's -z
BG_TRUE, BA_TRUE = np.array([0.003, -0.002, 0.004]), np.array([0.04, -0.03, 0.05])


def _imu(synth, k, rate=200, v=0.5, w=0.2):
    """The IMU messages of sweep k (scan time k - 1 to k) for synth.pose_at's motion in a map frame whose gravity is
    G_MAP, with constant biases; each message holds over the following dt (IMUIntegrator's forward Euler)."""
    n = int(round(0.1 * rate))
    h = 0.1 / n
    out = np.zeros((n, 7))
    for i in range(n):
        R, _ = synth.pose_at(k - 1 + i / n)
        f = np.array([0.0, v * w, 0.0]) - R.T @ G_MAP        # centripetal acceleration minus gravity, body frame
        out[i] = np.concatenate([[0.0, 0.0, w] + BG_TRUE, (f + BA_TRUE) / GN, [h]])
    return out


def _clouds(synth, k):
    """Scan k swept while moving, except the first (the node starts at rest: the first map is undistorted by identity)."""
    return synth.velo_scan(k, motion=k != K0), synth.livox_scan(k, motion=k != K0)


def _quat(R):
    q = Rsc.from_matrix(R).as_quat()
    return -q if q[3] < 0 else q


def _run(backend, synth):
    """The bring-up state machine over N_SCANS scans on one backend.  Returns the trace of every frame list state."""
    B = backend
    frames, samples = [], []
    push_count, start_time, inited, gravity = 0, 0.0, False, None
    R_aft, t_aft = synth.pose_matrix(K0)[:3, :3].copy(), synth.pose_matrix(K0)[:3, 3].copy()   # the map frame's origin
    dRb, dtb, dRl, dtl = np.eye(3), np.zeros(3), np.eye(3), np.zeros(3)
    trace = dict(init_scan=None, gravity=None, states=[], windows=0)
    for s in range(N_SCANS):
        k = K0 + s
        t = 0.1 * k
        imu = _imu(synth, k) if s > 0 else np.zeros((0, 7))
        if not inited:
            if s > 0:                                       # :774-788: GyroIntegration from identity -> delta_Rb, prediction
                dRb = Rsc.from_quat(B.gyro(imu)).as_matrix()
                dRl = dRb                                   # exTlb = I
            P, R = R_aft @ dtb + t_aft, R_aft @ dRb
            Pn, Qn = B.scan(k, dRl, dtl, P, _quat(R))       # undistort with (delta_Rl, delta_tl), EstimateLidarPose
            Rn = Rsc.from_quat(Qn).as_matrix()
            dRb, dtb = R_aft.T @ Rn, R_aft.T @ (Pn - t_aft)  # :838-846
            dRl, dtl = dRb, dtb
            R_aft, t_aft = Rn, Pn
            if push_count == 0:                             # :944-955
                frames.append(dict(t=t, P=Pn.copy(), Q=Qn.copy(), V=np.zeros(3), bg=np.zeros(3), ba=np.zeros(3), scan=(k, dRl, dtl)))
                samples.append(imu.copy())
                if len(frames) > 3:
                    frames.pop(0)
                    samples.pop(0)
            else:
                fr = frames[-1]
                samples[-1] = np.concatenate([samples[-1], imu])
                fr.update(t=t, P=Pn.copy(), Q=Qn.copy(), scan=(k, dRl, dtl))
            push_count += 1
            if push_count >= 3:                             # :957-983
                push_count = 0
                if len(frames) > 1:
                    frames[-1]["pre"] = B.preint(samples[-1], frames[-2]["bg"], frames[-2]["ba"])
                if len(frames) == int(3 / 1.5):
                    start_time = frames[-1]["t"]
                if len(frames) == 3 and frames[0]["t"] >= start_time:
                    ok, gravity = B.init(frames, samples)
                    if ok:
                        inited, trace["init_scan"], trace["gravity"] = True, s, gravity
        else:                                               # :796-829: pre-integration from the back frame, prediction
            back = frames[-1]
            pre = B.preint(imu, back["bg"], back["ba"])
            dQ, dP, dV = B.deltas(pre)
            Rb = Rsc.from_quat(back["Q"]).as_matrix()
            fr = dict(t=t, P=back["P"] + Rb @ dP, Q=_quat(Rb @ dQ), V=back["V"] + Rb @ dV, bg=back["bg"].copy(),
                      ba=back["ba"].copy(), pre=pre, scan=(k, dQ, dP))
            frames.append(fr)
            samples.append(imu)
            if len(frames) > 5:
                frames.pop(0)
                samples.pop(0)
            if len(frames) == 5:                            # full-window mode (windowSize == SLIDEWINDOWSIZE)
                B.window(frames, gravity)
                trace["windows"] += 1
            else:                                           # (a 4-frame list: the 1-frame lidar estimate of the new scan)
                fr["P"], fr["Q"] = B.scan(k, dQ, dP, fr["P"], fr["Q"])
        trace["states"].append([{key: np.array(f[key]) for key in ("P", "Q", "V", "bg", "ba")} for f in frames])
    trace["final"] = [(f["scan"][0], f["P"].copy(), f["Q"].copy()) for f in frames]
    return trace


class _Device:
    def __init__(self, M, synth, ctx):
        self.M, self.synth, self.ctx = M, synth, ctx
        self.odometry = importlib.import_module("multi-modal-loam_amd.odometry")
        self.odo = self.odometry.LidarOdometry(ctx, lidar_mode=2)
        self.west = None

    def gyro(self, imu):
        return self.M.imu_gyro_integrate(imu)

    def preint(self, smp, bg, ba):
        return self.M.imu_preintegrate(smp, bg, ba)

    def deltas(self, pre):
        return Rsc.from_quat(np.array(pre.dq)).as_matrix(), np.array(pre.dp), np.array(pre.dv)

    def _load(self, slot, k, dR, dt):
        c = self.ctx
        c.scan_upload(slot, *_clouds(self.synth, k))
        c.extract(slot, 1)
        c.undistort(slot, 1, np.asarray(dR).reshape(1, 9), np.asarray(dt).reshape(1, 3))

    def scan(self, k, dR, dt, P, Q):
        self._load(5, k, dR, dt)
        Pn, Qn, _ = self.odo.estimate_lidar_pose(5, P, Q)
        return Pn, Qn

    def init(self, frames, samples):
        ok, g, _ = self.odometry.try_map_initialization(frames, samples, np.eye(4))
        return ok, g

    def window(self, frames, gravity):
        if self.west is None:
            self.west = self.odometry.WindowEstimator(self.ctx, gravity=gravity, solver="device")
        for f, fr in enumerate(frames):
            self._load(f, *fr["scan"])
            self.ctx.downsample(f, 1)
        self.west.estimate(list(range(5)), frames, [None] + [fr["pre"] for fr in frames[1:]])


class _Oracle:
    def __init__(self, O, synth, leaf_corner, leaf_surf):
        self.O, self.synth = O, synth
        self.lm = O.LocalMap(window=50, leaf_corner=leaf_corner, leaf_surf=leaf_surf)
        self.last_update = np.array([-1.0, -1.0, -1.0])
        self.prior = None

    def gyro(self, imu):
        return LR.gyro_integrate(imu, [0.0, 0.0, 0.0, 1.0])

    def preint(self, smp, bg, ba):
        return IO.preintegrate(smp, bg, ba)

    def deltas(self, pre):
        return pre["dR"], pre["dp"], pre["dv"]

    def _features(self, k, dR, dt):
        O = self.O
        v, l = _clouds(self.synth, k)
        ev, el = O.extract_velo(v), O.extract_livox(l)
        xyz = np.concatenate([ev["xyzi"][:, :3], el["xyzi"][:, :3]])
        rel = np.concatenate([ev["reltime"], el["reltime"]])
        lab = np.concatenate([ev["label"], el["label"]])
        und = O.undistort(xyz, rel, np.asarray(dR), np.asarray(dt))
        return O.voxel_downsample(und[lab == 1], 0.4), O.voxel_downsample(und[lab == 2], 0.2), int((lab == 1).sum())

    def scan(self, k, dR, dt, P, Q):
        """LidarOdometry.estimate_lidar_pose on the CPU (odometry.py / Estimator.cpp:967-1140, lidar_mode 2, exTlb = I)."""
        O = self.O
        cf, sf, n_corner = self._features(k, dR, dt)
        P, Q = np.array(P, dtype=np.float64), np.array(Q, dtype=np.float64)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rsc.from_quat(Q).as_matrix(), P
        cm, sm = self.lm.get(0), self.lm.get(1)
        deg = False
        if len(cm) > 0 and len(sm) > 100:
            P, Q, _, deg, _ = O.estimate_single(cf, sf, cm, sm, np.eye(4), P, Q, 5, 10)
        if n_corner > 50:
            T[:3, :3], T[:3, 3] = Rsc.from_quat(Q).as_matrix(), P
        else:
            T[:3, 3] = [P[0], P[1], T[2, 3]]
        if not deg:
            d = self.last_update - T[:3, 3]
            if float(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) >= 0.5:
                self.lm.increment(cf, sf, T)
                self.last_update = T[:3, 3].copy()
        return P, Q

    def init(self, frames, samples):
        pres = [None] + [fr["pre"] for fr in frames[1:]]
        out = LR.try_map_initialization(frames, samples, np.eye(4), pres)
        if out["ok"]:
            for i in range(1, len(frames)):
                frames[i]["pre"] = out["pres"][i]
            del samples[:out["keep_from"]]
        return out["ok"], out["gravity"]

    def window(self, frames, G):
        """Estimator::Estimate in full-window mode on the CPU: the oracle loop of
        test_gpu_parity.py::test_full_window_estimate_with_imu_matches_oracle_loop."""
        O, W = self.O, len(frames)
        tc, ts = O.KdTree(self.lm.get(0)), O.KdTree(self.lm.get(1))
        feats = [self._features(*fr["scan"])[:2] for fr in frames]
        pres = [None] + [fr["pre"] for fr in frames[1:]]
        x = np.stack([np.concatenate([fr["P"], Rsc.from_quat(fr["Q"]).as_rotvec(), fr["V"], fr["bg"], fr["ba"]]) for fr in frames])
        facs = []
        for f in range(W):
            Twl = np.eye(4)
            Twl[:3, :3], Twl[:3, 3] = Rsc.from_rotvec(x[f][3:6]).as_matrix(), x[f][:3]
            facs.append((O.associate_lines(feats[f][0], tc, Twl, 1.0)[0], O.associate_planes(feats[f][1], ts, Twl, 1.0)[0]))
        prior = self.prior
        for it in range(5):
            back_before = x[-1].copy()

            def evaluate(z):
                xx = z.reshape(W, 15)
                n = 15 * W
                H, g, cost = np.zeros((n, n)), np.zeros(n), 0.0
                for f in range(W):
                    Hf, gf, cf = O.linearize(facs[f][0], facs[f][1], xx[f][:6], np.eye(4), 3e-4, 0.0)
                    H[15 * f:15 * f + 6, 15 * f:15 * f + 6] += Hf
                    g[15 * f:15 * f + 6] += gf
                    cost += cf
                for f in range(1, W):
                    fun = lambda q, f=f: IO.imu_residual(pres[f], G, q[:6], q[6:15], q[15:21], q[21:30])
                    q = np.concatenate([xx[f - 1], xx[f]])
                    r = fun(q)
                    J = IO.numeric_jacobian(fun, q, h=1e-6)
                    sl = slice(15 * (f - 1), 15 * (f + 1))
                    H[sl, sl] += J.T @ J
                    g[sl] += J.T @ r
                    cost += 0.5 * r @ r
                if prior is not None:
                    r = IO.prior_residual(prior, xx[0])
                    H[:15, :15] += prior["J"].T @ prior["J"]
                    g[:15] += prior["J"].T @ r
                    cost += 0.5 * r @ r
                return H, g, cost

            z, _, _, _ = IO.dense_trust_region(evaluate, x, max_iters=10, fixed=False)
            x = z.reshape(W, 15)
            Rb = Rsc.from_rotvec(back_before[3:6]).inv() * Rsc.from_rotvec(x[-1][3:6])
            deltaR = np.degrees(np.linalg.norm(Rb.as_rotvec()))
            deltaT = np.linalg.norm(back_before[:3] - x[-1][:3])
            if (deltaR < 0.05 and deltaT < 0.05) or it == 4:
                A, b = np.zeros((30, 30)), np.zeros(30)
                if prior is not None:
                    r = IO.prior_residual(prior, x[0])
                    A[:15, :15] += prior["J"].T @ prior["J"]
                    b[:15] += prior["J"].T @ r
                fun = lambda q: IO.imu_residual(pres[1], G, q[:6], q[6:15], q[15:21], q[21:30])
                q = np.concatenate([x[0], x[1]])
                J = IO.numeric_jacobian(fun, q, h=1e-6)
                A += J.T @ J
                b += J.T @ fun(q)
                H0, g0, _ = O.linearize(facs[0][0], facs[0][1], x[0][:6], np.eye(4), 3e-4, 0.0)
                A[:6, :6] += H0
                b[:6] += g0
                Jn, rn, _, _ = IO.marginalize(A, b, 15)
                self.prior = dict(J=Jn, r0=rn, x0=x[1].copy())
                break
        for f, fr in enumerate(frames):
            q = Rsc.from_rotvec(x[f][3:6]).as_quat()
            fr["P"], fr["Q"] = x[f][0:3].copy(), -q if q[3] < 0 else q
            fr["V"], fr["bg"], fr["ba"] = x[f][6:9].copy(), x[f][9:12].copy(), x[f][12:15].copy()


@pytest.mark.gpu
def test_cold_start_initialisation_then_full_window_matches_oracle(M, O, synth):
    c = M.Context(max_scans=6)
    try:
        dev = _run(_Device(M, synth, c), synth)
        ora = _run(_Oracle(O, synth, c.cfg.leaf_corner, c.cfg.leaf_surf), synth)
    finally:
        c.close()
    # frames pushed at scans 0, 3, 6, 9; veloStartTime = scan 5; the first list whose front is not older: scan 11
    assert dev["init_scan"] == ora["init_scan"] == 11
    assert dev["windows"] == ora["windows"] == 2
    ang = np.degrees(np.arccos(np.clip(np.dot(dev["gravity"], G_MAP) / (np.linalg.norm(dev["gravity"]) * GN), -1, 1)))
    assert ang < 1.0, ang
    assert np.abs(dev["gravity"] - ora["gravity"]).max() < 1e-6
    worst = 0.0
    for s, (a, b) in enumerate(zip(dev["states"], ora["states"])):
        assert len(a) == len(b)
        for fa, fb in zip(a, b):
            for key in ("P", "V", "bg", "ba"):
                d = np.abs(fa[key] - fb[key]).max()
                worst = max(worst, d)
                assert d < 1e-6, (s, key, d)
            d = np.abs((Rsc.from_quat(fa["Q"]).inv() * Rsc.from_quat(fb["Q"])).as_rotvec()).max()
            worst = max(worst, d)
            assert d < 1e-6, (s, "Q", d)
    for k, P, Q in dev["final"]:
        T = synth.pose_matrix(k)
        assert np.abs(P - T[:3, 3]).max() < 0.05, (k, P - T[:3, 3])
        assert np.degrees(np.linalg.norm((Rsc.from_matrix(T[:3, :3]).inv() * Rsc.from_quat(Q)).as_rotvec())) < 0.5
    print("cold start: init at scan %d, gravity %.3f deg from the truth, worst device / oracle difference %.2e"
          % (dev["init_scan"], ang, worst))
