"""The batch solve's three-wavefront form (solve.hip k_solve_batch1: launches of more one-frame problems than the device has CUs,
plan_weight_tan = 0, no trace) against the other forms of the solve, bit for bit.

One context of just more slots than CUs (264 on a 256-CU part; a multiple of 8 for the windowed call), tiny scans (16 rings x 256
azimuths + 2 048 Livox points, four distinct ones) taken through the product path -- extract, undistort, down-sample, associate --
against the scene's map, and planted among them the slots the form has a branch for:
  no corner feature | no feature of either kind | a surf stack with the overflow mark (a full-size scan in a context whose
  max_features holds only the tiny ones) | more than 128 valid line factors (the loop behind the hoisted first factor) | every
  line factor invalid (the slot associated from 500 m away: no neighbour, src < 0) | exactly one plane factor.
The batch call must equal one-slot calls (k_solve_wide) of the first, the last and every planted slot in pose and summary, for
max_num_iterations 0, 1, 10 with fixed iterations (the cost-only last pass) and without (where no pass may be cost-only); and the
calls that must stay on the general form -- plan_weight_tan != 0, window = 8, a trace requested -- must still agree with their
one-at-a-time / windowed counterparts."""
import numpy as np
import pytest

from conftest import perturbed, pose_to_x

pytestmark = pytest.mark.gpu

HUBER = 0.1 / 1.5e-3
MF = 640  # holds a tiny scan's stacks (<= 460 surf features), not a full one's (~1 050)
NO_CORNER, NOTHING, OVERFLOW, LONG_LINES, ALL_INVALID, ONE_PLANE = 3, 4, 5, 6, 7, 9
KEY = lambda q: (q.iterations, q.successful, q.termination, q.initial_cost, q.final_cost)


@pytest.fixture(scope="module")
def batch(M, synth, scene):
    probe = M.Context(max_scans=1)
    cus = probe.device_info()[1]
    probe.close()
    B = (cus // 8 + 1) * 8
    c = M.Context(max_scans=B, max_features=MF)
    try:
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        ks = [10 + s % 4 for s in range(B)]
        tiny = {k: (synth.velo_scan(k, n_az=256), synth.livox_scan(k, n=2048)) for k in set(ks)}
        for s in range(B):
            if s == OVERFLOW:
                c.scan_upload(s, synth.velo_scan(ks[s]), synth.livox_scan(ks[s]))
            elif s % 16 == 1:
                c.scan_upload(s, tiny[ks[s]][0], None)  # (no Livox points)
            else:
                c.scan_upload(s, *tiny[ks[s]])
        c.extract(0, B)
        c.undistort(0, B, np.tile(np.eye(3).reshape(1, 9), (B, 1)), np.zeros((B, 3)))
        try:
            c.downsample(0, B)
        except M.MmlError as e:  # (the call may report the overflowing slot; its mark stays either way)
            assert e.code == M.MML_ERR_CAPACITY
        with pytest.raises(M.MmlError) as e:
            c.features_download(OVERFLOW, 1)
        assert e.value.code == M.MML_ERR_CAPACITY, "the full-size scan's surf stack does not carry the overflow mark"
        T = np.stack([perturbed(synth.pose_matrix(k)) for k in ks])
        T[ALL_INVALID, :3, 3] += 500.0
        c.associate(0, B, T, 25.0, stats=False)
        x0 = np.stack([pose_to_x(t) for t in T])
        # the planted lists
        lines, src_l = c.factors_download(0, 0)
        planes, src_p = c.factors_download(0, 1)
        lines, planes = lines[src_l >= 0], planes[src_p >= 0]
        assert len(lines) > 50 and len(planes) > 128
        rng = np.random.default_rng(5)
        long_lines = np.resize(lines, (300, 10)).copy()
        long_lines[:, :3] += rng.normal(0, 0.02, (300, 3))
        long_lines[:, 9] = 0.25
        long_lines[rng.integers(128, 300, 30), 9] = 0.0  # skipped records behind the first 128
        long_lines[[0, 5, 64, 127], 9] = [0.0, 1e-5, 0.0, -1e-6]  # ... and among a thread's first (hoisted) factor: |error| <= 1e-5, src >= 0
        c.factors_upload(NO_CORNER, 0, lines[:0])
        c.factors_upload(NOTHING, 0, lines[:0])
        c.factors_upload(NOTHING, 1, planes[:0])
        c.factors_upload(LONG_LINES, 0, long_lines)
        c.factors_upload(ONE_PLANE, 1, planes[:1])
        x0[[NO_CORNER, NOTHING, LONG_LINES, ONE_PLANE]] = x0[0]
        _, src = c.factors_download(ALL_INVALID, 0)  # (the valid records only)
        assert len(c.features_download(ALL_INVALID, 0)) > 100 and len(src) == 0, "the far slot's line factors are not all invalid"
        assert (np.abs(long_lines[:, 9]) > 1e-5).sum() > 128
        yield dict(c=c, B=B, x0=x0, sample=sorted({0, B - 1, NO_CORNER, NOTHING, OVERFLOW, LONG_LINES, ALL_INVALID, ONE_PLANE}))
    finally:
        c.close()


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("max_iters", [0, 1, 10])
def test_batch_form_equals_one_slot_calls(batch, max_iters, fixed):
    c, B, x0 = batch["c"], batch["B"], batch["x0"]
    xb, sb, _ = c.solve(0, B, x0, np.eye(4), max_iters=max_iters, fixed=fixed, huber=HUBER)
    assert np.isfinite(xb).all()
    moved = 0
    for s in batch["sample"]:
        x1, s1, _ = c.solve(s, 1, x0[s:s + 1], np.eye(4), max_iters=max_iters, fixed=fixed, huber=HUBER)
        assert np.array_equal(x1[0], xb[s]) and KEY(s1[0]) == KEY(sb[s]), (s, max_iters, fixed, x1[0] - xb[s], KEY(s1[0]), KEY(sb[s]))
        moved += not np.array_equal(xb[s], x0[s])
    assert np.array_equal(xb[NOTHING], x0[NOTHING])
    if max_iters == 0:
        assert np.array_equal(xb, x0)
    elif max_iters == 10:
        assert moved >= len(batch["sample"]) - 2 and sb[0].iterations >= 1  # (the check is not blind: the solves move their poses)
        if fixed:
            assert sb[0].iterations == max_iters


def test_general_form_still_takes_the_other_batches(batch):
    c, B, x0 = batch["c"], batch["B"], batch["x0"]
    kw = dict(max_iters=10, fixed=True, huber=HUBER)
    # plan_weight_tan != 0: three residual rows per plane factor
    xb, sb, _ = c.solve(0, B, x0, np.eye(4), w_tan=3e-4, **kw)
    x0t, s0t, _ = c.solve(0, B, x0, np.eye(4), **kw)
    assert not np.array_equal(xb[0], x0t[0]), "plan_weight_tan did not reach the solve"
    for s in batch["sample"]:
        x1, s1, _ = c.solve(s, 1, x0[s:s + 1], np.eye(4), w_tan=3e-4, **kw)
        assert np.array_equal(x1[0], xb[s]) and KEY(s1[0]) == KEY(sb[s]), ("w_tan", s)
    # a trace requested: the traced batch equals the untraced one (the new form) and the one-slot traces
    xt, st, tt = c.solve(0, B, x0, np.eye(4), trace=True, **kw)
    assert np.array_equal(xt, x0t) and [KEY(q) for q in st] == [KEY(q) for q in s0t]
    for s in batch["sample"]:
        x1, s1, t1 = c.solve(s, 1, x0[s:s + 1], np.eye(4), trace=True, **kw)
        n = st[s].iterations  # (the rows of the iterations that ran, as tests/test_gpu_lidar_eval.py compares them)
        assert s1[0].iterations == n and np.array_equal(x1[0], xt[s]), ("trace", s)
        if st[s].termination != 4:  # (a solve that ends on invalid steps -- the slots without factors -- leaves no rows for them)
            assert np.array_equal(t1[0][:n], tt[s][:n]), ("trace", s)
    assert np.array_equal(tt[0][st[0].iterations - 1], xt[0])
    # windows of eight frames: the frame-parallel rounds against the sequential, traced window solve
    kw8 = dict(window=8, max_iters=10, fixed=True, huber=0.0, w_tan=3e-4)
    xw, sw, _ = c.solve(0, B, x0, np.eye(4), **kw8)
    xs, ss, _ = c.solve(0, B, x0, np.eye(4), trace=True, **kw8)
    assert np.array_equal(xw, xs) and [KEY(q) for q in sw] == [KEY(q) for q in ss]
    assert not np.array_equal(xw[:8], x0t[:8])
