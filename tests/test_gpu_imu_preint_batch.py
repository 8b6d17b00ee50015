"""mml_imu_preintegrate_batch on the device (k_imu_preintegrate, one wavefront per interval) against the host build of the same
routine (a NULL context): csrc/imu_preint.h runs the host's operations in the host's order on both sides, so every comparison
is bytes(device) == bytes(host).  The inputs are those of tests/test_imu_preint_batch.py; every one is finite and in range."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from conftest import perturbed
from test_imu_preint_batch import BA, BG, byte_cases, check_refusals, family, large_rotation, mixed_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1)
    yield c
    c.close()


def assert_device_equals_host(M, ctx, smp, bg, ba):
    dev = M.imu_preintegrate_batch(smp, bg, ba, ctx)
    host = M.imu_preintegrate_batch(smp, bg, ba)
    assert len(dev) == len(host) == len(smp)
    for i, (d, h) in enumerate(zip(dev, host)):
        assert bytes(d) == bytes(h), (i, len(smp[i]), np.abs(np.frombuffer(bytes(d)) - np.frombuffer(bytes(h))).max())
    return dev


def test_one_interval_of_zero_one_and_two_samples(M, ctx):
    rng = np.random.default_rng(10)
    for n in (0, 1, 2):
        (pre,) = assert_device_equals_host(M, ctx, [family(rng, n)], BG, BA)
        assert pre.dq[3] > 0 and np.array_equal(np.array(pre.bg), BG) and np.array_equal(np.array(pre.ba), BA)
    (pre,) = M.imu_preintegrate_batch([np.zeros((0, 7))], BG, BA, ctx)     # the reset state
    assert np.array_equal(np.array(pre.jacobian).reshape(15, 15), np.eye(15)) and not np.any(np.array(pre.covariance))


def test_lengths_at_the_chunk_edges(M, ctx):
    """The loader takes 32 samples at a time with 64 lanes: one short of, at and one past one, two and four chunks."""
    rng = np.random.default_rng(11)
    lengths = (31, 32, 33, 63, 64, 65, 128, 129)
    dev = assert_device_equals_host(M, ctx, [family(rng, n, 0.001, 0.003) for n in lengths], BG, BA)
    assert all(np.isfinite(np.frombuffer(bytes(p))).all() for p in dev)


def test_mixed_batch_and_the_cases_without_sin_or_cos(M, ctx, synth):
    assert_device_equals_host(M, ctx, *mixed_batch(synth))
    for name, s, bg, ba in byte_cases():
        (pre,) = assert_device_equals_host(M, ctx, [s], bg, ba)
        assert bytes(pre) == bytes(M.imu_preintegrate(s, bg, ba)), name   # and through it the single call


def test_rotation_through_180_degrees(M, ctx):
    s = large_rotation(np.random.default_rng(12))
    (pre,) = assert_device_equals_host(M, ctx, [s], BG, BA)
    R = Rsc.from_quat(np.array(pre.dq)).as_matrix()
    assert np.trace(R) < 0 and pre.dq[3] >= 0


def test_more_intervals_than_one_wave_of_workgroups(M, ctx):
    """n = 300 intervals of 3 .. 20 samples, a bias pair each; every result lands in its own entry."""
    rng = np.random.default_rng(13)
    smp = [family(rng, int(k)) for k in rng.integers(3, 21, 300)]
    dev = assert_device_equals_host(M, ctx, smp, rng.normal(0, 0.01, (300, 3)), rng.normal(0, 0.03, (300, 3)))
    assert len({bytes(p) for p in dev}) == 300


def test_smaller_call_after_a_larger_one_reuses_the_buffers(M, synth):
    rng = np.random.default_rng(14)
    c = M.Context(max_scans=1)
    try:
        big = [family(rng, 40) for _ in range(64)]
        assert_device_equals_host(M, c, big, BG, BA)
        assert_device_equals_host(M, c, [family(rng, 5), family(rng, 0), family(rng, 17)], BG, BA)
        assert_device_equals_host(M, c, big[:3], BG, BA)
    finally:
        c.close()


def test_refusals_leave_the_context_usable(M, ctx):
    check_refusals(M, ctx)
    with pytest.raises(M.MmlError) as e:
        M.imu_preintegrate_batch([], BG, BA, ctx)
    assert e.value.code == M.MML_ERR_INVALID and "mml_imu_preintegrate_batch" in str(e.value)
    assert_device_equals_host(M, ctx, [family(np.random.default_rng(15), 9)], BG, BA)


def test_batch_window_estimator_on_device_and_host_preintegrations(M, synth, scene):
    """Two windows of W = 3 (the set-up of tests/test_gpu_fullwindow_batch.py): BatchWindowEstimator fed by
    preintegrate_windows through the device call and through the host routine gives the same frames and priors."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    n, W, k0 = 2, 3, 20
    c = M.Context(max_scans=n * W)
    try:
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        rng = np.random.default_rng(23)
        frames, samples = [], []
        for w in range(n):
            frames.append([])
            samples.append([None])
            for f in range(W):
                k, slot = k0 + W * w + f, W * w + f
                c.scan_upload(slot, synth.velo_scan(k), synth.livox_scan(k))
                c.extract(slot, 1)
                c.undistort(slot, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
                c.downsample(slot, 1)
                T = perturbed(synth.pose_matrix(k), dt=rng.normal(0, 0.02, 3), rotvec=rng.normal(0, 0.003, 3))
                q = Rsc.from_matrix(T[:3, :3]).as_quat()
                frames[w].append(dict(P=T[:3, 3].copy(), Q=-q if q[3] < 0 else q, V=synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                      bg=rng.normal(0, 1e-4, 3), ba=rng.normal(0, 1e-3, 3)))
                if f > 0:
                    samples[w].append(synth.imu_samples(k - 1, k))
        slots = [list(range(W * w, W * w + W)) for w in range(n)]
        copy = lambda fl: [{kk: vv.copy() for kk, vv in fr.items()} for fr in fl]
        result = {}
        for side, cc in (("host", None), ("device", c)):
            pres = odometry.preintegrate_windows(samples, frames, cc)
            est = odometry.BatchWindowEstimator(c, n, gravity=synth.GRAVITY)
            fr = [copy(fl) for fl in frames]
            infos = est.estimate(slots, fr, pres)
            result[side] = (pres, fr, est.priors, [i["outer"] for i in infos])
        for w in range(n):
            for f in range(1, W):
                assert bytes(result["device"][0][w][f]) == bytes(result["host"][0][w][f]), (w, f)
            for fh, fd in zip(result["host"][1][w], result["device"][1][w]):
                for key in ("P", "Q", "V", "bg", "ba"):
                    assert np.array_equal(fh[key], fd[key]), (w, key)
            ph, pd = result["host"][2][w], result["device"][2][w]
            for name in ("J", "r0", "x0"):
                assert np.array_equal(np.array(getattr(ph, name)), np.array(getattr(pd, name))), (w, name)
            assert not np.array_equal(result["host"][1][w][-1]["P"], frames[w][-1]["P"])    # the estimate moved the frames
        assert result["host"][3] == result["device"][3]
    finally:
        c.close()
