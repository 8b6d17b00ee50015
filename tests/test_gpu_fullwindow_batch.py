"""mml_fullwindow_solve_batch (n full-window solves in one device call) and odometry.BatchWindowEstimator against
mml_fullwindow_solve / WindowEstimator(solver="device") called window by window.  A window's arithmetic must not depend on
its neighbours in the batch, so every comparison is bit-equality."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from conftest import perturbed

pytestmark = pytest.mark.gpu

SLOTS = 12
K0 = 20
W_TAN = 3e-4


def summary_tuple(s):
    return (s.iterations, s.successful, s.termination, s.initial_cost, s.final_cost)


def prior_fields(p):
    return [np.array(p.J), np.array(p.r0), np.array(p.x0)]


class Problems:
    """12 slots of synthetic scans K0 .. K0 + 11, extracted, undistorted, down-sampled and associated at perturbed poses (as
    test_fullwindow_device_solve_matches_host_loop builds its 8), pre-integrations between consecutive scans, and a prior
    produced by marginalizing a first solve of the 8-frame window."""

    def __init__(self, M, synth, scene):
        odometry = importlib.import_module("multi-modal-loam_amd.odometry")
        self.M, self.G = M, synth.GRAVITY
        self.c = c = M.Context(max_scans=SLOTS)
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        west = odometry.WindowEstimator(c, gravity=self.G)
        self.T_bl = west.T_bl
        rng = np.random.default_rng(5)
        x0, self.pres = [], [None]
        for f in range(SLOTS):
            k = K0 + f
            c.scan_upload(f, synth.velo_scan(k), synth.livox_scan(k))
            c.extract(f, 1)
            c.undistort(f, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
            c.downsample(f, 1)
            T = perturbed(synth.pose_matrix(k), dt=rng.normal(0, 0.02, 3), rotvec=rng.normal(0, 0.003, 3))
            x0.append(np.concatenate([T[:3, 3], Rsc.from_matrix(T[:3, :3]).as_rotvec(), synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                      rng.normal(0, 1e-4, 3), rng.normal(0, 1e-3, 3)]))
            if f > 0:
                self.pres.append(M.imu_preintegrate(synth.imu_samples(k - 1, k), np.zeros(3), np.zeros(3)))
            c.associate(f, 1, west._T_wl(x0[f])[None], 1.0)
        self.x0 = np.stack(x0)
        self.prior = None
        fw = self.make(dict(W=8, first=0))
        xs, _, _ = fw.solve_device(c, 0, self.T_bl, self.x0[:8])
        self.prior = fw.marginalize(c.linearize_window(0, 1, xs[:1], self.T_bl, W_TAN, 0.0)[0], xs)
        # the distinct problems of the mixed batch, all on first_slot = 0, and their single solves (computed once)
        self.A = dict(W=8, first=0, prior=True)
        self.B = dict(W=3, first=0, skip=(2,))
        self.C = dict(W=1, first=0)
        self.refs = {}
        self.D = dict(W=8, first=0, prior=True, x=self.single(self.A)["x"])

    def make(self, spec):
        fw = self.M.FullWindowSolver(spec["W"], max_iters=spec.get("max_iters", 10), fixed=False, huber=0.0, w_tan=W_TAN)
        for f in range(1, spec["W"]):
            if f not in spec.get("skip", ()):
                fw.set_imu(f, self.pres[spec["first"] + f], self.G)
        if spec.get("prior"):
            fw.set_prior(self.prior)
        return fw

    def start(self, spec):
        return spec["x"] if "x" in spec else self.x0[spec["first"]:spec["first"] + spec["W"]]

    def single(self, spec):
        """mml_fullwindow_solve alone on a fresh handle with this set-up."""
        key = (spec["W"], spec["first"], tuple(spec.get("skip", ())), bool(spec.get("prior")), spec["x"].tobytes() if "x" in spec else None)
        if key not in self.refs:
            fw = self.make(spec)
            x, s, ev = fw.solve_device(self.c, spec["first"], self.T_bl, self.start(spec))
            self.refs[key] = dict(x=x, summary=summary_tuple(s), evaluations=ev, handle=fw, spec=spec)
        return self.refs[key]

    def batch(self, specs, records0=False):
        fws = [self.make(s) for s in specs]
        out = self.M.fullwindow_solve_batch(self.c, fws, [s["first"] for s in specs], self.T_bl, [self.start(s) for s in specs],
                                            records0=records0)
        return fws, out

    def assert_equal_single(self, spec, fw, x, s, ev):
        ref = self.single(spec)
        assert np.array_equal(x, ref["x"]), np.abs(x - ref["x"]).max(0)
        assert summary_tuple(s) == ref["summary"]
        assert ev == ref["evaluations"]
        assert summary_tuple(fw.summary()) == ref["summary"]       # the handle reports the solve as after the single call


@pytest.fixture(scope="module")
def prob(M, synth, scene):
    p = Problems(M, synth, scene)
    yield p
    p.c.close()


def test_batch_of_one_equals_the_single_solve(prob):
    fws, (xs, ss, evs) = prob.batch([prob.A])
    assert len(xs) == len(ss) == len(evs) == 1 and xs[0].shape == (8, 15)
    prob.assert_equal_single(prob.A, fws[0], xs[0], ss[0], evs[0])


def test_mixed_batch_on_overlapping_slots(prob):
    """W = 8 with prior, W = 3 with an IMU gap and no prior, W = 1, and a W = 8 that starts from the first one's solution
    and finishes in its first rounds while the others run on: all on first_slot = 0."""
    M, c = prob.M, prob.c
    specs = [prob.A, prob.B, prob.C, prob.D]
    fws, (xs, ss, evs, rec0) = prob.batch(specs, records0=True)
    for spec, fw, x, s, ev in zip(specs, fws, xs, ss, evs):
        prob.assert_equal_single(spec, fw, x, s, ev)
    assert len({s.iterations for s in ss}) >= 2
    assert any(s.successful >= 1 and np.abs(x - prob.start(spec)).max() > 1e-4 for spec, x, s in zip(specs, xs, ss))
    assert rec0.shape == (4, 32)
    for spec, fw, x, r in zip(specs, fws, xs, rec0):
        assert np.array_equal(r, c.linearize_window(spec["first"], 1, x[:1], prob.T_bl, W_TAN, 0.0)[0])
        if spec["W"] >= 2:
            pb, ps = fw.marginalize(r, x), prob.single(spec)["handle"].marginalize(r, x)
            for a, b in zip(prior_fields(pb), prior_fields(ps)):
                assert np.array_equal(a, b)


def test_distinct_slot_ranges_in_either_order(prob):
    specs = [dict(W=3, first=f) for f in (0, 3, 6, 9)]
    for order in (specs, specs[::-1]):
        fws, (xs, ss, evs) = prob.batch(order)
        for spec, fw, x, s, ev in zip(order, fws, xs, ss, evs):
            prob.assert_equal_single(spec, fw, x, s, ev)
    # the four windows see different scans: four different answers
    assert len({prob.single(s)["x"].tobytes() for s in specs}) == 4


def test_more_windows_than_compute_units(prob):
    """n = 300: one launch runs in several waves of workgroups."""
    specs = [prob.A, prob.B, prob.C] * 100
    fws, (xs, ss, evs) = prob.batch(specs)
    assert len(xs) == 300
    for w, (spec, fw, x, s, ev) in enumerate(zip(specs, fws, xs, ss, evs)):
        assert np.array_equal(x, xs[w % 3]) and summary_tuple(s) == summary_tuple(ss[w % 3]) and ev == evs[w % 3], w
        prob.assert_equal_single(spec, fw, x, s, ev)


def test_refusals_leave_the_context_usable(prob):
    M, c = prob.M, prob.c
    fw = prob.make(prob.A)
    with pytest.raises(M.MmlError) as e:
        M.fullwindow_solve_batch(c, [fw, fw], [0, 0], prob.T_bl, [prob.x0[:8], prob.x0[:8]])
    assert e.value.code == M.MML_ERR_INVALID and "window 1" in str(e.value)
    with pytest.raises(M.MmlError) as e:
        M.fullwindow_solve_batch(c, [prob.make(prob.C), fw], [0, SLOTS - 7], prob.T_bl, [prob.x0[:1], prob.x0[:8]])
    assert e.value.code == M.MML_ERR_INVALID and "window 1" in str(e.value)
    with pytest.raises(M.MmlError) as e:
        M.fullwindow_solve_batch(c, [], [], prob.T_bl, [])
    assert e.value.code == M.MML_ERR_INVALID
    fws, (xs, ss, evs) = prob.batch([prob.A])
    prob.assert_equal_single(prob.A, fws[0], xs[0], ss[0], evs[0])


def test_batch_window_estimator_equals_three_window_estimators(M, synth, scene):
    """Two consecutive calls (the second consumes the priors of the first) on 3 windows of W = 3 in slots 0-2, 3-5, 6-8, each
    with its own gravity vector, against one WindowEstimator(solver="device") per window on the same inputs."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    n, W = 3, 3
    G = np.stack([synth.GRAVITY, synth.GRAVITY * (1.0 + 1e-3), synth.GRAVITY])
    c = M.Context(max_scans=n * W)
    try:
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        refs = [odometry.WindowEstimator(c, gravity=G[w], solver="device") for w in range(n)]
        best = odometry.BatchWindowEstimator(c, n, gravity=G)
        rng = np.random.default_rng(23)
        slots = [list(range(W * w, W * w + W)) for w in range(n)]
        for k0 in (20, 21):
            frames, pres = [], []
            for w in range(n):
                frames.append([])
                pres.append([None])
                for f in range(W):
                    k, slot = k0 + W * w + f, W * w + f
                    c.scan_upload(slot, synth.velo_scan(k), synth.livox_scan(k))
                    c.extract(slot, 1)
                    c.undistort(slot, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
                    c.downsample(slot, 1)
                    T = perturbed(synth.pose_matrix(k), dt=rng.normal(0, 0.02, 3), rotvec=rng.normal(0, 0.003, 3))
                    q = Rsc.from_matrix(T[:3, :3]).as_quat()
                    frames[w].append(dict(P=T[:3, 3].copy(), Q=-q if q[3] < 0 else q, V=synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                          bg=np.zeros(3), ba=np.zeros(3)))
                    if f > 0:
                        pres[w].append(M.imu_preintegrate(synth.imu_samples(k - 1, k), np.zeros(3), np.zeros(3)))
            copy = lambda fl: [{kk: vv.copy() for kk, vv in fr.items()} for fr in fl]
            frames_r, frames_b = [copy(fl) for fl in frames], [copy(fl) for fl in frames]
            infos_r = [refs[w].estimate(slots[w], frames_r[w], pres[w]) for w in range(n)]
            infos_b = best.estimate(slots, frames_b, pres)
            for w in range(n):
                for fr, fb in zip(frames_r[w], frames_b[w]):
                    for key in ("P", "Q", "V", "bg", "ba"):
                        assert np.array_equal(fr[key], fb[key]), (w, key)
                assert infos_b[w]["outer"] == infos_r[w]["outer"]
                assert infos_b[w]["evaluations"] == infos_r[w]["evaluations"]
                assert [summary_tuple(s) for s in infos_b[w]["summaries"]] == [summary_tuple(s) for s in infos_r[w]["summaries"]]
                for a, b in zip(prior_fields(best.priors[w]), prior_fields(refs[w].prior)):
                    assert np.array_equal(a, b), w
        with pytest.raises(ValueError):
            best.estimate([[0, 2, 1], [3, 4, 5], [6, 7, 8]], frames_b, pres)
    finally:
        c.close()
