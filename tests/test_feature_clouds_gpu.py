"""GPU suite for the feature node's message: mml_feature_clouds_download_batch / mml_feature_clouds_download against the
oracle's extraction in raw order (tests/feature_clouds_expect.py).  Byte equality throughout: k = 0, 1, 3, 4 against the oracle,
k = 2, 5 against mml_scan_download_pointxyzinormal on the same slot."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from feature_clouds_expect import NAMES, cached, expected

pytestmark = pytest.mark.gpu

FULL = (14, 1800, 24000, False)     # the scan of test_gicp_refresh_on_a_slot: livox_corner_num > 100
# (seed, azimuths, Livox points, messy): raw counts that are no multiple of 64 or 1024
ONE_BLOCK = (5, 101, 1501, True)    # 1616 + 1501 raw points: one bucketing block per sensor, two rounds of the walk
TWO_BLOCKS = (6, 301, 5003, True)   # 4816 + 5003: two blocks per sensor, a block boundary inside the walk


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 12)


def _same(a, b):
    return a.shape[0] == b.shape[0] and np.array_equal(_u32(a), _u32(b))


def _raw(M, ctx, first, count, capacity=None, fill=0xA5, out=True):
    """the batch entry point as it is: (rc, n_points (count, 6), buffer of `capacity` records prefilled with `fill`)"""
    n = np.full(6 * max(count, 1), -7, np.int32)
    buf = np.full((max(capacity or 0, 1), 48), fill, np.uint8) if out else None
    rc = M.lib().mml_feature_clouds_download_batch(ctx._h, first, count, _p(buf), capacity or 0, _p(n))
    return rc, n.reshape(-1, 6), buf


def _check_slot(M, c, slot, e, far_transformed=None):
    """slot's six clouds against the expectation `e`; returns them"""
    clouds = c.feature_clouds(slot, 1)[0]
    info = c.scan_info(slot)
    fused = c.scan_download_pointxyzinormal(slot)
    for k in (0, 1, 3, 4):
        assert _same(clouds[k], e[NAMES[k]]), (slot, NAMES[k], len(clouds[k]), len(e[NAMES[k]]))
    assert _same(clouds[2], fused[:info.n_velo]) and _same(clouds[5], fused[info.n_velo:])
    assert [len(clouds[k]) for k in (0, 1, 3, 4)] == [info.velo_corner_num, info.velo_surf_num, info.livox_corner_num, info.livox_surf_num]
    assert tuple(len(clouds[k]) for k in (0, 1, 3, 4)) == e["counts"]
    assert _same(clouds[2], e["velo_fused"])
    return clouds


@pytest.mark.parametrize("onepass", [True, False])
@pytest.mark.parametrize("shape", [ONE_BLOCK, TWO_BLOCKS])
def test_raw_order_clouds_match_the_oracle(M, O, monkeypatch, shape, onepass):
    """Scans of one and of two bucketing blocks with dropped raw records mixed in (Livox line > 5 and x < 0.01, Velodyne NaN and
    out-of-table pitch), through both bucketing forms (the three-pass one stores a scan as ONE block)."""
    if not onepass:
        monkeypatch.setenv("MML_ASSIGN_ONEPASS", "0")
    v, l, e = cached(*shape, 50.0)
    blk = M.ASSIGN_BLOCK_POINTS
    assert (len(v) > blk and len(l) > blk) == (shape is TWO_BLOCKS) and len(v) % 64 and len(l) % 64
    assert (l["line"] > 5).sum() > 10 and (l["x"] < 0.01).sum() > 10 and np.isnan(v[:, 0]).sum() > 10
    assert len(e["velo_corner"]) and len(e["velo_surface"]) and len(e["livox_corner"]) and len(e["livox_surface"])
    c = M.Context(max_scans=1)
    try:
        c.scan_upload(0, v, l)
        c.extract(0, 1)
        clouds = _check_slot(M, c, 0, e)
        assert _same(clouds[5], e["livox_fused"])
        assert (clouds[0]["intensity"] != 0).any() and (clouds[2]["intensity"] == 0).all()
    finally:
        c.close()


def test_livox_points_beyond_far_th_and_the_counters(M, O):
    """far_th = 8 m: labelled Livox points beyond the fused cloud are in k = 3, 4 and in livox_*_num, and nowhere else."""
    v, l, e = cached(*FULL, 8.0)
    assert e["far_labelled"] >= 10
    c = M.Context(max_scans=1, far_th=8.0)
    try:
        c.scan_upload(0, v, l)
        c.extract(0, 1)
        clouds = _check_slot(M, c, 0, e)
        n_fused_labelled = int((clouds[5]["normal_z"] > 0).sum())
        assert len(clouds[3]) + len(clouds[4]) == n_fused_labelled + e["far_labelled"]
    finally:
        c.close()


def test_extrinsic_reaches_livox_combine_only(M, O):
    """mml_extract with an extrinsic: applied when livox_corner_num > 100 (slot 0), to livox_combine alone; not at all otherwise
    (slot 1, a short Livox frame)."""
    v, l, e0 = cached(*FULL, 50.0)
    l1 = l[:3000]
    e1 = expected(O, v, l1)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0.9998, -0.02, 0.0], [0.02, 0.9998, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.05, -0.02, 0.1]
    c = M.Context(max_scans=2)
    try:
        c.scan_upload(0, v, l)
        c.scan_upload(1, v, l1)
        c.extract(0, 2, T)
        assert c.scan_info(0).livox_corner_num > 100 and c.scan_info(1).livox_corner_num <= 100
        a = _check_slot(M, c, 0, e0)
        b = _check_slot(M, c, 1, e1)
        p = e0["livox_fused"][:, :3]
        moved = np.stack([T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1] + T[r, 2] * p[:, 2] + T[r, 3] for r in range(3)], 1).astype(np.float32)
        got = np.stack([a[5]["x"], a[5]["y"], a[5]["z"]], 1)
        assert len(got) == len(p) and not np.array_equal(got, p) and np.abs(got - moved).max() < 1e-4
        assert _same(b[5], e1["livox_fused"])
    finally:
        c.close()


def test_batch_with_empty_sensors_equals_the_single_calls(M, O):
    """three slots of different sizes, one without a Velodyne part and one without a Livox part: the batch is the three single
    calls back to back, and every cloud starts where the counts before it end"""
    v0, l0, e0 = cached(*ONE_BLOCK, 50.0)
    v1, l1, e1 = cached(7, 0, 2001, False, 50.0)
    v2, l2, e2 = cached(8, 150, 0, False, 50.0)
    c = M.Context(max_scans=4)
    try:
        for s, (v, l) in enumerate(((v0, l0), (v1, l1), (v2, l2))):
            c.scan_upload(1 + s, v, l)
        c.extract(1, 3)
        rc, n, _ = _raw(M, c, 1, 3, out=False)
        assert rc == M.MML_OK and (n >= 0).all()
        assert (n[1, :3] == 0).all() and n[1, 3:].sum() > 0 and (n[2, 3:] == 0).all() and n[2, :3].sum() > 0
        total = int(n.sum())
        rc, n2, buf = _raw(M, c, 1, 3, capacity=total + 3)
        assert rc == M.MML_OK and np.array_equal(n, n2) and (buf[total:] == 0xA5).all()
        singles = []
        for s in range(3):
            rc, ns, bs = _raw(M, c, 1 + s, 1, capacity=int(n[s].sum()))
            assert rc == M.MML_OK and np.array_equal(ns[0], n[s])
            singles.append(bs[:int(n[s].sum())])
        assert np.array_equal(buf[:total], np.concatenate(singles))
        # the offsets follow from n_points: cut the buffer there and compare with the expectation
        rec = buf[:total].view(np.float32).reshape(-1, 12)
        ends = np.cumsum(n.reshape(-1))
        for s, e in enumerate((e0, e1, e2)):
            for k in (0, 1, 3, 4):
                hi = ends[6 * s + k]
                assert _same(rec[hi - n[s, k]:hi], e[NAMES[k]]), (s, k)
        # ... and the wrapper cuts it the same way
        for s, six in enumerate(c.feature_clouds(1, 3)):
            assert [len(x) for x in six] == list(n[s])
    finally:
        c.close()


def test_sizing_capacity_state_and_argument_errors(M, O, synth):
    v, l, e = cached(*ONE_BLOCK, 50.0)
    c = M.Context(max_scans=3)
    L = M.lib()
    try:
        for s in range(3):
            c.scan_upload(s, v, l)
        # never extracted
        rc, _, _ = _raw(M, c, 0, 1, out=False)
        assert rc == M.MML_ERR_STATE
        c.extract(0, 3)
        rc, n, _ = _raw(M, c, 0, 3, out=False)            # the sizing call
        assert rc == M.MML_OK and (n == n[0]).all() and n[0].sum() > 0
        total = int(n.sum())
        rc, n2, buf = _raw(M, c, 0, 3, capacity=total - 1)  # too small: nothing written, the counts still are
        assert rc == M.MML_ERR_CAPACITY and (buf == 0xA5).all() and np.array_equal(n, n2)
        one = np.zeros(6, np.int32)
        rec = np.full((int(n[0].sum()), 48), 0x5A, np.uint8)
        assert L.mml_feature_clouds_download(c._h, 1, _p(rec), len(rec) - 1, _p(one)) == M.MML_ERR_CAPACITY and (rec == 0x5A).all()
        assert L.mml_feature_clouds_download(c._h, 1, _p(rec), len(rec), _p(one)) == M.MML_OK and np.array_equal(one, n[1])
        # bad ranges and arguments
        for first, count in ((-1, 1), (3, 1), (0, 4), (2, 2), (0, 0), (0, -1)):
            assert _raw(M, c, first, count, capacity=total)[0] == M.MML_ERR_INVALID, (first, count)
        assert L.mml_feature_clouds_download_batch(c._h, 0, 1, None, 0, None) == M.MML_ERR_INVALID
        assert L.mml_feature_clouds_download(c._h, 3, None, 0, _p(one)) == M.MML_ERR_INVALID
        # the call belongs between mml_extract and mml_undistort
        c.undistort(0, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
        assert _raw(M, c, 0, 1, out=False)[0] == M.MML_ERR_STATE
        assert _raw(M, c, 0, 3, out=False)[0] == M.MML_ERR_STATE and _raw(M, c, 1, 2, out=False)[0] == M.MML_OK
        # an uploaded cloud has no raw order
        c.cloud_upload(1, c.scan_download_pointxyzinormal(1), c.scan_info(1).n_velo)
        assert _raw(M, c, 1, 1, out=False)[0] == M.MML_ERR_STATE
        # the raw scan uploaded again since the extraction (the next scan staged early)
        c.scan_upload(2, v, l)
        assert _raw(M, c, 2, 1, out=False)[0] == M.MML_ERR_STATE
        c.extract(2, 1)
        assert _raw(M, c, 2, 1, out=False)[0] == M.MML_OK
        with pytest.raises(M.MmlError) as ei:
            c.feature_clouds(0, 1)
        assert ei.value.code == M.MML_ERR_STATE
    finally:
        c.close()


def test_the_call_leaves_the_slots_as_they_were(M, O):
    """digests equal before and after the call, and the stages that follow give what they give without it"""
    v, l, _ = cached(*TWO_BLOCKS, 50.0)
    a, b = M.Context(max_scans=2), M.Context(max_scans=2)
    try:
        for c in (a, b):
            c.scan_upload(0, v, l)
            c.scan_upload(1, v[:1000], l[:700])
            c.extract(0, 2)
        before = a.slot_digest(0, 2)
        a.feature_clouds(0, 2)
        a.feature_clouds(1, 1)
        assert np.array_equal(a.slot_digest(0, 2), before) and np.array_equal(b.slot_digest(0, 2), before)
        dR, dt = np.tile(np.eye(3).reshape(1, 9), (2, 1)), np.full((2, 3), 0.01)
        for c in (a, b):
            c.undistort(0, 2, dR, dt)
            c.downsample(0, 2)
        assert np.array_equal(a.slot_digest(0, 2), b.slot_digest(0, 2))
    finally:
        a.close()
        b.close()


def test_cpp_adapter_fills_the_same_messages(M, O, tmp_path):
    """unionCloudMessage and the reference-signature overloads of getVeloFeature / getHoriFeatureExtract, compiled against
    mmloam_adapter.hpp, against the ctypes result"""
    exe = tmp_path / "feature_clouds_probe"
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
           os.path.join(ROOT, "tests", "cpp", "feature_clouds_probe.cpp"), "-o", str(exe), "-L", libdir, "-lmmloam_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    scans = [cached(*ONE_BLOCK, 50.0)[:2], cached(*TWO_BLOCKS, 50.0)[:2]]
    far = 9.0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(scans)).tobytes() + np.float32(far).tobytes())
        for v, l in scans:
            f.write(np.int32(len(v)).tobytes() + np.ascontiguousarray(v, np.float32).tobytes())
            f.write(np.int32(len(l)).tobytes() + np.ascontiguousarray(l).tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FEATURE_CLOUDS_PROBE_DONE" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    msgs, at = [], 0
    while at < len(raw):
        head = np.frombuffer(raw, np.int32, 10, at)
        at += 40
        six = []
        for k in range(6):
            six.append(np.frombuffer(raw, np.float32, 12 * head[k], at).reshape(-1, 12))
            at += 48 * int(head[k])
        msgs.append((head, six))
    assert len(msgs) == len(scans) + 2 and at == len(raw)
    c = M.Context(max_scans=4, far_th=far)
    try:
        (v0, l0) = scans[0]
        for s, (v, l) in enumerate(scans):
            c.scan_upload(s, v, l)
        c.scan_upload(2, v0, None)
        c.scan_upload(3, None, l0)
        c.extract(0, 4)
        for s, (six, (head, got)) in enumerate(zip(c.feature_clouds(0, 4), msgs)):
            info = c.scan_info(s)
            assert list(head[:6]) == [len(x) for x in six], s
            assert list(head[6:]) == [info.velo_corner_num, info.velo_surf_num, info.livox_corner_num, info.livox_surf_num], s
            for k in range(6):
                assert np.array_equal(got[k].view(np.uint32), six[k].view(np.uint32).reshape(-1, 12)), (s, k)
        assert msgs[2][0][0] > 0 and msgs[3][0][3] > 0
    finally:
        c.close()
