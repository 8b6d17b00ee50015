"""GPU suite: the device's undistortion (csrc/undistort_dev.h: fast form, float_round_safe guard, undistort_exact) against the exact
references of tests/golden/undistort_kat.npz (tests/undistort_checks.py), BIT FOR BIT on every point: 14 sweep motions -- every
branch of the matrix -> quaternion assignment, the linear slerp branch and its edge, both sides of theta = 0.5, w < 0, 179.99
degrees and pi, a matrix that is not orthonormal -- with 768 random points and 256 guard points each, the guard points being those
the device may not answer with its fast form.

One motion per slot, the slot's 1 024 points uploaded as a labelled cloud (mml_cloud_upload): 517 in the Velodyne region and 507 in
the Livox region of slots of 2 048 + 2 048, so both regions end inside a 256-lane block of k_undistort.

  1. the whole-cloud kernel: one mml_undistort over the 14 slots;
  2. a sub-range, mml_undistort(3, 5): parameters are indexed from 0, slots from `first`; the slots outside keep their bytes;
  3. k_undistort_listed.  mml_step is the only caller of that kernel and it extracts the slot's RAW scan first, which replaces an
     uploaded cloud: caller-chosen points and times cannot reach the listed kernel through the C-ABI, so the fixture's floats
     cannot be asserted there.  What can be: mml_step with the fixture's 14 motions on synthetic scans leaves, labelled points
     (k_undistort_listed) and the rest (k_undistort<SETTLE>) alike, the bytes the whole-cloud kernel of (1) leaves for the same
     scans and motions -- the listed kernel's parameter indexing and its call of undistort_point on every branch of the fixture."""
import numpy as np
import pytest

import undistort_checks as K

pytestmark = pytest.mark.gpu

N_VELO = 517
NV = NL = 2048


@pytest.fixture(scope="module")
def kat():
    return K.load()


def _records(f, i, label=None):
    """48-byte PointXYZINormal records of the points i: x y z _ | normal_x = s, normal_y = line, normal_z = label _ | intensity"""
    rec = np.zeros((len(i), 12), np.float32)
    rec[:, :3] = f["xyz"][i]
    rec[:, 4] = f["s"][i]
    rec[:, 5] = np.arange(len(i)) % 6
    if label is not None:
        rec[:, 6] = label
    rec[:, 8] = 1.0 + np.arange(len(i), dtype=np.float32)
    return rec


@pytest.fixture(scope="module")
def ctx(M, kat):
    c = M.Context(max_scans=len(kat["names"]), max_velo_points=NV, max_livox_points=NL)
    yield c
    c.close()


def _upload_all(c, f):
    for m in range(len(f["names"])):
        i = K.of_motion(f, m)
        assert len(i) > 2 * N_VELO - 256 and N_VELO % 256 and (len(i) - N_VELO) % 256
        c.cloud_upload(m, _records(f, i), N_VELO)


def _check_slot(c, f, m, undistorted):
    i = K.of_motion(f, m)
    d = c.scan_download(m)
    assert d["info"].n_points == len(i) and d["info"].n_velo == N_VELO
    assert np.array_equal(d["xyzi"][:, 3], _records(f, i)[:, 8])
    if undistorted:
        K.assert_bits(f, d["xyzi"][:, :3], i, "slot %d" % m)
        assert np.all(d["reltime"] == 1.0)
    else:
        assert d["xyzi"][:, :3].tobytes() == f["xyz"][i].tobytes() and d["reltime"].tobytes() == f["s"][i].tobytes(), m


def test_whole_cloud_kernel_equals_exact_floats(ctx, kat):
    f = kat
    nm = len(f["names"])
    _upload_all(ctx, f)
    ctx.undistort(0, nm, f["dR"], f["dt"])
    got = np.concatenate([ctx.scan_download(m)["xyzi"][:, :3] for m in range(nm)])
    idx = np.concatenate([K.of_motion(f, m) for m in range(nm)])
    bad = K.differing(f, got, idx)
    print("whole cloud: %d of %d points differ (%d of the %d guard points)" % (len(bad), len(idx), int(f["guard"][bad].sum()), int(f["guard"].sum())))
    for m in range(nm):
        _check_slot(ctx, f, m, True)


def test_sub_range_equals_exact_floats(ctx, kat):
    f = kat
    _upload_all(ctx, f)
    ctx.undistort(3, 5, f["dR"][3:8], f["dt"][3:8])
    for m in range(len(f["names"])):
        _check_slot(ctx, f, m, 3 <= m < 8)


def test_listed_kernel_equals_whole_cloud_kernel_on_every_branch(M, synth, kat):
    """(3) of the module's docstring.  16 rings x 512 azimuths + 2 000 Livox points a slot, four distinct scans over the 14 slots; a
    small local map made of the first scan's own down-sampled features.  Down-sampled stacks and poses are not asserted."""
    f = kat
    nm = len(f["names"])
    c = M.Context(max_scans=nm, max_velo_points=16 * 512, max_livox_points=2048)
    try:
        for s in range(nm):
            k = 30 + s % 4
            c.scan_upload(s, synth.velo_scan(k, n_az=512, motion=True), synth.livox_scan(k, n=2000, motion=True))
        c.extract(0, nm)
        c.undistort(0, nm, f["dR"], f["dt"])
        c.downsample(0, nm)
        want = [c.scan_download(s) for s in range(nm)]
        listed = [int((w["label"] != 0).sum()) for w in want]
        assert min(listed) > 256 and min(w["info"].n_points - n for w, n in zip(want, listed)) > 4096   # both kernels have work
        c.map_set_local(0, c.features_download(0, 0))       # (slot 0: the identity motion)
        c.map_set_local(1, c.features_download(0, 1))
        c.step(0, nm, f["dR"], f["dt"], np.eye(4), 25.0, 1, np.zeros((nm, 6)))
        for s in range(nm):
            d = c.scan_download(s)                           # the first reader: settles the rest of the cloud
            lab = want[s]["label"] != 0
            assert np.array_equal(d["label"], want[s]["label"]) and np.all(d["reltime"] == 1.0)
            assert d["xyzi"][lab].tobytes() == want[s]["xyzi"][lab].tobytes(), "slot %d (%s): listed points" % (s, f["names"][s])
            assert d["xyzi"][~lab].tobytes() == want[s]["xyzi"][~lab].tobytes(), "slot %d (%s): settled points" % (s, f["names"][s])
    finally:
        c.close()
