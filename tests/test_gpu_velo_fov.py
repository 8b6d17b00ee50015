"""mml_velo_fov_select[_batch] on the device against the NULL-context host path of the same call, to the byte: rows, counts, info.
The host path itself is held to an independent restatement of the reference's loop in tests/test_velo_fov.py; the end-to-end
case here feeds that restatement's cloud to the time-offset search directly.  Frame sizes straddle the kernel's boundaries: a
wavefront (64), one workgroup pass (M.FOV_TILE_POINTS) and the largest frame that stays in registers (M.FOV_REG_POINTS)."""
import importlib
import math

import numpy as np
import pytest

from test_velo_fov import RawCall, _p, restate, ring, rotated_scan

pytestmark = pytest.mark.gpu

PI = math.pi
START = -0.3


def sweep(n, h, seed):
    """n points of one revolution from -atan2 = START on whose point h is the first more than pi past the start (h >= n: none is);
    FOV points at both ends."""
    k = min(h, n)
    o = np.concatenate([np.linspace(START, START + 2.9, k), np.linspace(START + 3.25, START + 2 * PI - 0.01, n - k)])
    return ring(o, seed)


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1, max_velo_points=8192, max_livox_points=64)
    yield c
    c.close()


def assert_equal(dev, host, what=""):
    for k in ("n_kept", "info", "xyzt", "xyz", "offsets"):
        assert dev[k].tobytes() == host[k].tobytes(), (what, k)


def test_sizes_around_every_boundary_and_h_in_every_place(M, ctx):
    T, R = M.FOV_TILE_POINTS, M.FOV_REG_POINTS
    assert (T, R) == (256, 4096)
    shapes = [(1, 9), (2, 1), (63, 5), (64, 63), (65, 64), (T - 1, 5), (T, T - 6), (T + 1, T), (T + 1, 9999), (R - 1, 5), (R, T - 3), (R, 2 * T + 188),
              (R + 1, 5), (R + 1, T - 1), (R + 1, R), (R + 1, 3 * T + 17), (8192, 6000)]
    frames = [sweep(n, h, 100 + i) for i, (n, h) in enumerate(shapes)]
    host = M.velo_fov_select(frames)
    # the frames are what they claim: h where it was put (first wave, last wave of a pass, a later tile, the last point, never)
    assert host["info"]["half_index"].tolist() == [h if h < n else -1 for n, h in shapes]
    assert np.all(host["n_kept"][2:] > 0) and host["n_kept"][0] == 1
    dev = ctx.velo_fov_select(frames)
    assert_equal(dev, host, "batch")
    for i in (0, 3, 7, 11, 15):                                  # single calls: the n = 1 case of the same kernels
        assert_equal(ctx.velo_fov_select([frames[i]]), M.velo_fov_select([frames[i]]), shapes[i])


def test_batch_of_five_with_an_empty_frame_equals_the_single_calls(M, ctx, synth):
    frames = [rotated_scan(synth, 20, 0.0), sweep(300, 120, 1), np.zeros((0, 4), np.float32), rotated_scan(synth, 23, PI / 2), sweep(4500, 4400, 2)]
    frames[1][150, :3] = np.nan                                   # a NaN point in the middle: never kept, never sets the flag
    batch = ctx.velo_fov_select(frames)
    assert_equal(batch, M.velo_fov_select(frames), "host")
    singles = [ctx.velo_fov_select([f]) for f in frames]
    assert batch["n_kept"][2] == 0 and batch["info"][2].tolist() == (0.0, 0.0, -1, 0)
    for k in ("xyzt", "xyz", "info"):
        assert batch[k].tobytes() == b"".join(s[k].tobytes() for s in singles), k
    assert batch["n_kept"].tolist() == [int(s["n_kept"][0]) for s in singles]


def test_nan_first_and_last_points_give_the_same_nan_bits(M, ctx):
    """startOri / endOri NaN: every relTime is NaN and points are still kept by their unadjusted azimuth (tests/test_velo_fov.py);
    the NaN written is the one the reference's machine writes, on both paths."""
    first, last = ring(np.linspace(-0.5, 5.6, 400), 6), ring(np.linspace(-0.5, 5.6, 400), 5)
    first[0, 0] = np.nan
    last[-1, 1] = np.nan
    dev, host = ctx.velo_fov_select([first, last]), M.velo_fov_select([first, last])
    assert np.all(host["n_kept"] > 50) and np.all(np.isnan(host["xyzt"][:, 3]))
    assert_equal(dev, host, "nan")


def test_strided_and_unaligned_records(M, ctx):
    f = sweep(1000, 400, 3)
    want = M.velo_fov_select([f])
    for step, off, lead in ((32, (4, 12, 20), 5), (22, (0, 4, 8), 3), (12, (0, 4, 8), 0)):
        rec = np.full((len(f), step), 0x5a, np.uint8)
        for c in range(3):
            rec[:, off[c]:off[c] + 4] = np.ascontiguousarray(f[:, c]).view(np.uint8).reshape(-1, 4)
        raw = np.concatenate([np.full(lead, 9, np.uint8), rec.reshape(-1)])
        dev = M.velo_fov_select_raw(raw, [lead], [len(f)], step, *off, ctx=ctx)
        host = M.velo_fov_select_raw(raw, [lead], [len(f)], step, *off)
        assert_equal(dev, host, step)
        assert dev["xyzt"].tobytes() == want["xyzt"].tobytes(), step


def test_frame_above_max_velo_points_is_refused_and_nothing_is_written(M, ctx):
    c = RawCall(M, [sweep(100, 50, 4), sweep(8193, 4000, 5)])
    assert c.run(ctx=ctx._h) == M.MML_ERR_CAPACITY and c.untouched()
    msg = M.lib().mml_last_error(ctx._h).decode()
    assert "mml_velo_fov_select_batch" in msg and "frame 1" in msg and "8193" in msg
    c = RawCall(M, [sweep(100, 50, 4)], cap=3)                  # fewer rows than are kept: refused after the count, nothing written
    assert c.run(ctx=ctx._h) == M.MML_ERR_CAPACITY and c.untouched()
    c = RawCall(M, [sweep(100, 50, 4)])
    assert c.run(ctx=ctx._h, step=11) == M.MML_ERR_INVALID and c.untouched()


def test_scratch_grows_with_the_call_and_profiling_names_the_stage(M):
    c = M.Context(max_scans=1, max_velo_points=8192, max_livox_points=64)
    try:
        small = [sweep(200, 90, 6)]
        assert_equal(c.velo_fov_select(small), M.velo_fov_select(small), "small")
        big = [sweep(5000, 2500, 7), sweep(8192, 100, 8), sweep(777, 776, 9)]
        c.profile_enable(True)
        c.profile_reset()
        out = c.velo_fov_select(big)                              # sizing call (one synchronisation) + filling call (two)
        prof = c.profile_get()
        c.profile_enable(False)
        assert_equal(out, M.velo_fov_select(big), "grown")
        assert_equal(c.velo_fov_select(small), M.velo_fov_select(small), "small again")
        assert "velo_fov" in prof and prof["velo_fov"][1] == 3, prof
    finally:
        c.close()


def test_selection_feeds_the_time_offset_search(M, synth):
    """Raw frames -> FOV selection -> time_offset_search_batch in two device calls equals the same search fed with the clouds the
    restatement selects."""
    odo = importlib.import_module("multi-modal-loam_amd.odometry")
    frames = [rotated_scan(synth, 20, 0.0), rotated_scan(synth, 22, -0.7)]
    lv = synth.livox_scan(31)
    livox = np.stack([lv["x"], lv["y"], lv["z"]], 1).astype(np.float32)[:3000]
    th = 0.03
    tf = np.array([[np.cos(th), -np.sin(th), 0, 0.05], [np.sin(th), np.cos(th), 0, -0.1], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float32)
    c = M.Context(max_scans=1, max_velo_points=4096, max_livox_points=64)
    try:
        got, sel = odo.time_offset_from_frames(c, frames, livox, tf, 30, 500)
        clouds = [restate(f)[0][:, :3] for f in frames]
        assert [len(x) for x in clouds] == sel["n_kept"].tolist() and min(len(x) for x in clouds) > 100
        want = c.time_offset_search_batch(clouds, [livox, livox], 30, 500, tfs=tf)
    finally:
        c.close()
    for g, w in zip(got, want):
        assert np.array_equal(g["nn_d2"], w["nn_d2"]) and np.array_equal(g["window_error"], w["window_error"])
        assert g["best_window"] == w["best_window"] and g["lowest_error"] == w["lowest_error"] and len(g["window_error"]) > 0
