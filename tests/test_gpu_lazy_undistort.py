"""mml_step undistorts only the points on the slot's label lists; the rest of the cloud is finished by the first entry point that
reads it (mml_cloud_settle, csrc/undistort_voxel.hip).  Nothing a caller can see may differ from the step that undistorted the
whole cloud itself.

Reference of every cloud comparison: the eager chain `extract -> undistort -> downsample` through the public entry points on the
same context and slots, run first, its downloads kept.  Where a reader also returns what association and solve leave (the factor
and pose words of mml_slot_digest, the poses of the step) the reference is the same step on a context created with
$MML_LAZY_UNDISTORT=0, the library's switch back to the whole-cloud undistortion: the step's association pose is built on the
host inside mml_step and cannot be handed to mml_associate bit for bit from here.  Every comparison is byte equality.

Shapes: 16 rings x 512 azimuths + 2 000 Livox points (10 048 valid points in slots of 10 240: 40 blocks of k_undistort, a ragged
last block in both sensor regions, ~700 listed points a slot: every lane of k_undistort_listed's 8 workgroups strides or idles)."""
import os

import numpy as np
import pytest

from conftest import perturbed, pose_to_x

pytestmark = pytest.mark.gpu

N_AZ, N_LIVOX = 512, 2000
NV, NL = 16 * N_AZ, 2048
KS = (30, 31, 32, 33)
GN = 4


def _ctx(M, B, lazy=True, **over):
    """A context of B small slots; lazy=False: created under $MML_LAZY_UNDISTORT=0 (the switch is read once per context)."""
    old = os.environ.get("MML_LAZY_UNDISTORT")
    if not lazy:
        os.environ["MML_LAZY_UNDISTORT"] = "0"
    try:
        kw = dict(max_scans=B, max_velo_points=NV, max_livox_points=NL)
        kw.update(over)
        return M.Context(**kw)
    finally:
        if not lazy:
            if old is None:
                del os.environ["MML_LAZY_UNDISTORT"]
            else:
                os.environ["MML_LAZY_UNDISTORT"] = old


def _eager_chain(c, first, count, dR, dt):
    c.extract(first, count)
    c.undistort(first, count, dR, dt)
    c.downsample(first, count)


def _cloud(c, s):
    d = c.scan_download(s)
    return (d["xyzi"].tobytes(), d["reltime"].tobytes(), d["ring"].tobytes(), d["label"].tobytes())


def _feats(c, s):
    return (c.features_download(s, 0).tobytes(), c.features_download(s, 1).tobytes())


@pytest.fixture(scope="module")
def setup(M, synth):
    """Four distinct moving scans, their sweep motions and start poses, a small map made of their own down-sampled features, and
    the results of the step that undistorts the whole cloud itself (4 slots): digests, poses."""
    cases = []
    for k in KS:
        dR, dt = synth.sweep_motion(k)
        T0 = perturbed(synth.pose_matrix(k))
        cases.append(dict(velo=synth.velo_scan(k, n_az=N_AZ, motion=True), livox=synth.livox_scan(k, n=N_LIVOX, motion=True),
                          dR=dR.reshape(9), dt=dt, T0=T0, x0=pose_to_x(T0), k=k))
    dR = np.stack([cs["dR"] for cs in cases])
    dt = np.stack([cs["dt"] for cs in cases])
    x0 = np.stack([cs["x0"] for cs in cases])
    c = _ctx(M, 4, lazy=False)
    try:
        for s, cs in enumerate(cases):
            c.scan_upload(s, cs["velo"], cs["livox"])
        _eager_chain(c, 0, 4, dR, dt)
        maps = [[], []]
        for s, cs in enumerate(cases):
            T = synth.pose_matrix(cs["k"])
            for kind in (0, 1):
                maps[kind].append(synth.transform(T, c.features_download(s, kind).astype(np.float64)).astype(np.float32))
        maps = [np.concatenate(m) for m in maps]
        assert len(maps[0]) > 20 and len(maps[1]) > 100
        c.map_set_local(0, maps[0])
        c.map_set_local(1, maps[1])
        x = c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
        ref = dict(x=x, digest=c.slot_digest(0, 4), cloud=[_cloud(c, s) for s in range(4)], feats=[_feats(c, s) for s in range(4)])
    finally:
        c.close()
    return dict(cases=cases, dR=dR, dt=dt, x0=x0, maps=maps, eager_step=ref)


def _filled(M, setup, B, **kw):
    """A context of B slots, slot s holding scan s % 4, the maps set; with the per-slot arguments of a step over all of them."""
    c = _ctx(M, B, **kw)
    c.map_set_local(0, setup["maps"][0])
    c.map_set_local(1, setup["maps"][1])
    for s in range(B):
        cs = setup["cases"][s % 4]
        c.scan_upload(s, cs["velo"], cs["livox"])
    rep = lambda a: np.stack([a[s % 4] for s in range(B)])
    return c, rep(setup["dR"]), rep(setup["dt"]), rep(setup["x0"])


@pytest.fixture(scope="module")
def four(M, setup):
    """The 4-slot context the reader tests share, with what every reader returns after the eager chain."""
    c, dR, dt, x0 = _filled(M, setup, 4)
    try:
        yield c, dR, dt, x0
    finally:
        c.close()


def _gicp(c):
    try:
        c.gicp_refresh(0, np.eye(4))
        return "ran"
    except Exception as e:   # (an undistorted slot is refused: the same refusal either way)
        return (type(e).__name__, getattr(e, "code", None), str(e))


def _readers(T):
    blob = lambda arrs: [a.tobytes() for a in arrs]
    return {
        "scan_download": lambda c: [_cloud(c, s) for s in range(4)],
        "scan_download_pointxyzinormal": lambda c: [c.scan_download_pointxyzinormal(s).tobytes() for s in range(4)],
        "cloud_download_registered": lambda c: [blob(c.cloud_download_registered(s, 1, T[s])) for s in range(4)],
        "cloud_download_registered_batch": lambda c: blob(c.cloud_download_registered(0, 4, T)),
        "slot_digest": lambda c: c.slot_digest(0, 4)[:, :7].tobytes(),   # counts, labels, lines, points, times, both stacks
        "gicp_refresh": lambda c: (_gicp(c), _cloud(c, 0)),
    }


@pytest.mark.parametrize("reader", ["scan_download", "scan_download_pointxyzinormal", "cloud_download_registered",
                                    "cloud_download_registered_batch", "slot_digest", "gicp_refresh"])
def test_step_then_each_reader_first(four, setup, reader):
    """(1) a fresh step, then `reader` as the first reader of the slots: what it returns after the eager chain."""
    c, dR, dt, x0 = four
    read = _readers(np.stack([cs["T0"] for cs in setup["cases"]]))[reader]
    _eager_chain(c, 0, 4, dR, dt)
    want = read(c)
    want_feats = [_feats(c, s) for s in range(4)]
    want_cloud = [_cloud(c, s) for s in range(4)]
    x = c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
    got = read(c)
    assert got == want
    assert [_feats(c, s) for s in range(4)] == want_feats
    assert [_cloud(c, s) for s in range(4)] == want_cloud     # ... and the whole cloud is finished behind it
    # against the step that undistorts everything itself: poses, and every digest word (factor lists and pose included)
    es = setup["eager_step"]
    assert x.tobytes() == es["x"].tobytes()
    assert c.slot_digest(0, 4).tobytes() == es["digest"].tobytes()
    assert want_cloud == es["cloud"] and want_feats == es["feats"]


def test_undistort_again(four, setup, synth):
    """(2) step, then mml_undistort with a second motion: the eager undistortion twice (the second reads the time as 1)."""
    c, dR, dt, x0 = four
    m2 = [synth.sweep_motion(k + 7) for k in KS]
    dR2 = np.stack([m[0].reshape(9) for m in m2])
    dt2 = np.stack([m[1] for m in m2])
    c.extract(0, 4)
    c.undistort(0, 4, dR, dt)
    c.undistort(0, 4, dR2, dt2)
    want = [_cloud(c, s) for s in range(4)]
    c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
    c.undistort(0, 4, dR2, dt2)
    assert [_cloud(c, s) for s in range(4)] == want
    assert all(np.all(c.scan_download(s)["reltime"] == 1.0) for s in range(4))


def test_back_to_back_steps(four, setup):
    """(3) two steps with nothing read in between: the second extraction drops the pending state of the first."""
    c, dR, dt, x0 = four
    _eager_chain(c, 0, 4, dR, dt)
    want = [_cloud(c, s) + _feats(c, s) for s in range(4)]
    x1 = c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
    x2 = c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
    assert x1.tobytes() == x2.tobytes()
    assert [_cloud(c, s) + _feats(c, s) for s in range(4)] == want


def test_partial_range(M, setup):
    """(4) eager chain on 8 slots, step on [2, 5): a slot below, inside and above the range."""
    c, dR, dt, x0 = _filled(M, setup, 8)
    try:
        _eager_chain(c, 0, 8, dR, dt)
        want = {s: _cloud(c, s) + _feats(c, s) for s in (1, 3, 6)}
        c.step(2, 3, dR[2:5], dt[2:5], np.eye(4), 25.0, GN, x0[2:5])
        for s in (1, 3, 6):
            assert _cloud(c, s) + _feats(c, s) == want[s], s
        # settling a range that is pending only in part ([2, 5) of [0, 8)), after another step
        c.step(2, 3, dR[2:5], dt[2:5], np.eye(4), 25.0, GN, x0[2:5])
        dg = c.slot_digest(0, 8)
        for s in range(8):
            assert dg[s, 1:7].tobytes() == dg[s % 4 + (4 if s < 4 else 0), 1:7].tobytes(), s   # cloud and stacks of the replica
    finally:
        c.close()


def test_two_lanes(M, setup):
    """(5) 80 slots over 4 scans (count >= 64: the step runs on the lanes): replica slots digest alike, and like a one-lane run."""
    B = 80
    c, dR, dt, x0 = _filled(M, setup, B)
    try:
        x2 = c.step(0, B, dR, dt, np.eye(4), 25.0, GN, x0)
        d2 = c.slot_digest(0, B)
        for s in range(4, B):
            assert d2[s].tobytes() == d2[s % 4].tobytes(), s
        c.set_lanes(1)
        x1 = c.step(0, B, dR, dt, np.eye(4), 25.0, GN, x0)
        assert x1.tobytes() == x2.tobytes()
        assert c.slot_digest(0, B).tobytes() == d2.tobytes()
        # (the batch kernels of 80 slots and the small-call kernels of 4 leave the same cloud)
        assert [_cloud(c, s) for s in range(4)] == setup["eager_step"]["cloud"]
    finally:
        c.close()


def test_far_threshold(M, setup, synth):
    """(6) a small far_th: labelled Livox points beyond it are counted, carry 0x81 / 0x82 and are on no list."""
    c, dR, dt, x0 = _filled(M, setup, 4, far_th=6.0)
    try:
        _eager_chain(c, 0, 4, dR, dt)
        far_labelled = 0
        for s in range(4):
            d = c.scan_download(s)
            i = d["info"]
            far_labelled += i.livox_corner_num + i.livox_surf_num - int((d["label"][i.n_velo:] != 0).sum())
        assert far_labelled > 0
        want = [_cloud(c, s) + _feats(c, s) for s in range(4)]
        c.step(0, 4, dR, dt, np.eye(4), 25.0, GN, x0)
        assert [_cloud(c, s) + _feats(c, s) for s in range(4)] == want
    finally:
        c.close()


@pytest.mark.parametrize("count", [1, 16])
def test_packed_path(M, setup, count):
    """(7) calls of up to 16 slots move their parameters in one block (the live path)."""
    c, dR, dt, x0 = _filled(M, setup, 16)
    try:
        _eager_chain(c, 0, 16, dR, dt)
        want = [_cloud(c, s) + _feats(c, s) for s in range(16)]
        x = c.step(0, count, dR[:count], dt[:count], np.eye(4), 25.0, GN, x0[:count])
        assert [_cloud(c, s) + _feats(c, s) for s in range(16)] == want
        if count == 16:
            for s in range(16):
                assert x[s].tobytes() == x[s % 4].tobytes(), s
    finally:
        c.close()
