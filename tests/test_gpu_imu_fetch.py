"""mml_imu_stream / mml_imu_fetch_batch / mml_imu_predict_batch on the device against mml_imu_fetch_host / the host build on the
same messages: EVERY output byte must be equal (rows, offsets, samples, pre, dq, prediction).  The host side is held to the
reference's walk in tests/test_imu_fetch.py."""
import importlib
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imu_fetch_cases as IC  # noqa: E402
import imu_fetch_ref as IR  # noqa: E402
from conftest import perturbed  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def msgs():
    return IC.stream()


@pytest.fixture(scope="module")
def resident(ctx, msgs):
    s = ctx.imu_stream(1024)
    s.push(msgs)
    yield s
    s.close()


def assert_same(dev, host, what):
    assert set(dev) == set(host), what
    for k in host:
        a, b = (bytes(dev[k]), bytes(host[k])) if k == "pre" else (dev[k].tobytes(), host[k].tobytes())
        assert a == b, "%s: %s differs" % (what, k)


def both(M, stream, live_msgs, ts, te, **kw):
    """The device call and the host call on the same messages.  `first` counts absolutely on the stream, from 0 on the array."""
    dev = M.imu_fetch_batch(stream, ts, te, **kw)
    host = M.imu_fetch_batch(live_msgs, ts, te, **kw)
    host["rows"] = host["rows"].copy()
    host["rows"]["first"] += stream.state()["front"]
    assert_same(dev, host, "n = %d" % len(ts))
    return dev


def test_every_edge_case_in_one_call(M, resident, msgs):
    cases = IC.edge_intervals(msgs[:, 0])
    ts, te = [c[1] for c in cases], [c[2] for c in cases]
    bg, ba = IC.biases(len(ts))
    dev = both(M, resident, msgs, ts, te, bg=bg, ba=ba)
    assert [(int(r["status"]), int(r["n"]), int(r["interpolated"])) for r in dev["rows"]] == [c[3:] for c in cases]
    st = resident.state()
    assert (st["front"], st["tail"], st["disorder"], st["first_stamp"], st["last_stamp"]) == (0, len(msgs), 0, msgs[0, 0], msgs[-1, 0])


@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_wavefront_and_workgroup_edges(M, resident, msgs, n):
    # intervals of 35 ms every 3.3 ms: they overlap, repeat messages and run off the stream's end (NOT_REACHED) for the large n
    ts = np.array([IC.SEC + 0.2525 + 0.0033 * k for k in range(n)])
    dev = both(M, resident, msgs, ts, ts + 0.035, bg=np.zeros(3), ba=np.full(3, 0.01))
    if n == 1025:
        assert set(dev["rows"]["status"]) == {IR.OK, IR.NOT_REACHED}


def test_a_smaller_call_after_a_larger_one_and_each_output_alone(M, resident, msgs):
    ts, te = IC.consecutive(5)
    full = both(M, resident, msgs, ts, te, bg=np.zeros(3), ba=np.zeros(3))
    for want in (("samples",), ("pre",), ("dq",), ()):
        part = both(M, resident, msgs, ts, te, bg=np.zeros(3), ba=np.zeros(3), want=want)
        for k in want:
            assert (bytes(part[k]) if k == "pre" else part[k].tobytes()) == (bytes(full[k]) if k == "pre" else full[k].tobytes())


def test_all_statuses_nonzero_without_samples(M, ctx, resident, msgs):
    T = msgs[:, 0]
    ts = np.array([T[5], T[-1], T[0] - 2.0, T[20] + 0.001])
    te = np.array([T[3], T[-1] + 1.0, T[0] - 1.0, T[20] + 0.002])
    rows = np.zeros(4, M.IMU_INTERVAL_DTYPE)
    off = np.full(5, -1, np.int32)
    dq = np.full((4, 4), 7.0)
    pre = (M.ImuPreint * 4)()
    z = np.zeros((4, 3))
    p = M._p
    ctx._ck(M.lib().mml_imu_fetch_batch(ctx._h, resident._h, 4, p(ts), p(te), p(z), p(z), p(rows), p(off), None, 0, pre, p(dq)))
    assert list(rows["status"]) == [IR.REVERSED, IR.NOT_REACHED, IR.TOO_OLD, IR.NO_SAMPLE] and np.all(rows["n"] == 0) and np.all(off == 0)
    assert np.array_equal(dq, [[0, 0, 0, 1]] * 4)
    reset = M.imu_preintegrate_batch([np.zeros((0, 7))] * 4, z, z)
    assert bytes(pre) == b"".join(bytes(r) for r in reset)


def test_capacity_one_row_short(M, ctx, resident, msgs):
    ts, te = IC.consecutive(6)
    good = M.imu_fetch_batch(resident, ts, te, bg=np.zeros(3), ba=np.zeros(3))
    total = int(good["offsets"][-1])
    rc, out = M.imu_fetch_raw(resident, ts, te, np.zeros(3), np.zeros(3), sample_capacity=total - 1)
    assert rc == M.MML_ERR_CAPACITY and "sample_capacity" in M.lib().mml_last_error(ctx._h).decode()
    assert out["rows"].tobytes() == good["rows"].tobytes() and np.array_equal(out["offsets"], good["offsets"]) and "samples" not in out
    rc, out = M.imu_fetch_raw(resident, ts, te, np.zeros(3), np.zeros(3), sample_capacity=total)
    assert rc == M.MML_OK
    assert_same(out, good, "after the refusal")


def test_refusals_leave_the_context_usable(M, ctx, resident, msgs):
    ts, te = IC.consecutive(3)
    L, p = M.lib(), M._p
    rows, off, z = np.full(3, 7, M.IMU_INTERVAL_DTYPE), np.full(4, 7, np.int32), np.zeros((3, 3))
    pre = (M.ImuPreint * 3)()
    inf = ts.copy()
    inf[1] = np.inf
    other = M.Context(max_scans=1)
    try:
        for what, rc in (("n = 0", L.mml_imu_fetch_batch(ctx._h, resident._h, 0, p(ts), p(te), None, None, p(rows), p(off), None, 0, None, None)),
                         ("n too large", L.mml_imu_fetch_batch(ctx._h, resident._h, 8193, p(ts), p(te), None, None, p(rows), p(off), None, 0, None, None)),
                         ("null stream", L.mml_imu_fetch_batch(ctx._h, None, 3, p(ts), p(te), None, None, p(rows), p(off), None, 0, None, None)),
                         ("null t_end", L.mml_imu_fetch_batch(ctx._h, resident._h, 3, p(ts), None, None, None, p(rows), p(off), None, 0, None, None)),
                         ("null rows", L.mml_imu_fetch_batch(ctx._h, resident._h, 3, p(ts), p(te), None, None, None, p(off), None, 0, None, None)),
                         ("another context", L.mml_imu_fetch_batch(other._h, resident._h, 3, p(ts), p(te), None, None, p(rows), p(off), None, 0, None, None)),
                         ("bg alone", L.mml_imu_fetch_batch(ctx._h, resident._h, 3, p(ts), p(te), p(z), None, p(rows), p(off), None, 0, None, None)),
                         ("pre without biases", L.mml_imu_fetch_batch(ctx._h, resident._h, 3, p(ts), p(te), None, None, p(rows), p(off), None, 0, pre, None)),
                         ("infinite time", L.mml_imu_fetch_batch(ctx._h, resident._h, 3, p(inf), p(te), None, None, p(rows), p(off), None, 0, None, None))):
            assert rc == M.MML_ERR_INVALID, what
            assert np.all(rows["status"] == 7) and np.all(off == 7), what
        assert "interval 1" in L.mml_last_error(ctx._h).decode()
    finally:
        other.close()
    both(M, resident, msgs, ts, te, bg=z, ba=z)


def test_pushes_trim_and_move_to_front(M, ctx):
    """A 256-message stream fed 40 messages at a time with a trim after every push: the live part moves to the front of the other
    array several times.  State, trim and cuts equal the sequential rule / the host call on the surviving messages."""
    msgs = IC.stream(1200, seed=5)
    T = list(msgs[:, 0])
    s = ctx.imu_stream(256)
    try:
        front, moves, base = 0, 0, 0
        for k in range(0, 1200, 40):
            if k + 40 - base > 256:       # the stream's own rule: the live part moves when the array's end would be passed
                moves, base = moves + 1, front
            s.push(msgs[k:k + 40])
            keep = 100 if k % 400 else 300     # (300: more than the live count, nothing is dropped)
            t = T[k] - 0.4 if k % 280 else T[0] - 1.0   # (every seventh: a time before the front)
            s.drop_before(t, keep)
            front = IR.drop_before(T[:k + 40], front, t, keep)
            st = s.state()
            assert (st["front"], st["tail"], st["disorder"], st["first_stamp"], st["last_stamp"]) == (front, k + 40, 0, T[front], T[k + 39])
            if k % 200 == 0 or k == 1160:
                ts = np.array([T[front] - 0.01, T[front + 3], 0.5 * (T[k + 20] + T[k + 21]), T[k + 39]])
                te = np.array([T[front + 5], 0.5 * (T[front + 70] + T[front + 71]), T[k + 39], T[k + 39] + 0.01])
                both(M, s, msgs[front:k + 40], ts, te, bg=np.zeros(3), ba=np.zeros(3))
        assert moves >= 2 and front > 900
        with pytest.raises(M.MmlError) as e:
            s.push(IC.stream(300, seed=6))
        assert e.value.code == M.MML_ERR_CAPACITY and s.state()["tail"] == 1200
    finally:
        s.close()


def test_disorder_is_refused_then_reset(M, ctx, msgs):
    s, s2 = ctx.imu_stream(1024), ctx.imu_stream(64)      # (two more streams on the context, beside `resident`)
    try:
        s.push(msgs[:300])
        s.push(msgs[290:400])           # its first message is older than the message before it
        s2.push(msgs[:1])
        ts, te = IC.consecutive(2)
        rc, _ = M.imu_fetch_raw(s, ts, te, want=())
        assert rc == M.MML_ERR_STATE and s.state()["disorder"] == 1
        one = both(M, s2, msgs[:1], [msgs[0, 0] - 1.0, msgs[0, 0] - 1.0], [msgs[0, 0] + 1.0, msgs[0, 0]])
        assert list(one["rows"]["status"]) == [IR.NOT_REACHED, IR.TOO_OLD]
        s2.reset()
        empty = both(M, s2, np.zeros((0, 7)), [1.0], [2.0], bg=np.zeros(3), ba=np.zeros(3))
        assert list(empty["rows"]["status"]) == [IR.EMPTY]
        s.reset()
        assert s.state() == dict(front=0, tail=0, disorder=0, first_stamp=0.0, last_stamp=0.0)
        s.push(msgs[:400])
        both(M, s, msgs[:400], ts, te, bg=np.zeros(3), ba=np.zeros(3))
    finally:
        s.close()
        s2.close()


def test_prediction_equals_the_host_build(M, ctx, resident, msgs):
    n = 70
    ts = np.array([IC.SEC + 0.2525 + 0.03 * k for k in range(n)])
    got = M.imu_fetch_batch(resident, ts, ts + 0.1, bg=np.zeros(3), ba=np.zeros(3), want=("pre", "dq"))
    rng = np.random.default_rng(3)
    prev = np.concatenate([rng.normal(0, 30, (n, 3)), Rsc.random(n, random_state=4).as_quat(), rng.normal(0, 2, (n, 3))], axis=1)
    ex = np.eye(4)
    ex[:3, :3] = Rsc.from_rotvec([0.02, -0.4, 1.1]).as_matrix()
    ex[:3, 3] = [0.1, -0.05, 0.3]
    for kw in (dict(prev=prev, pre=got["pre"], dq=got["dq"]), dict(prev=prev[:3], pre=list(got["pre"])[:3]), dict(dq=got["dq"][:1])):
        assert_same(M.imu_predict_batch(ex, ctx=ctx, **kw), M.imu_predict_batch(ex, **kw), sorted(kw))


def test_fetch_imu_windows_feeds_the_batch_calls(M, synth, scene):
    """odometry.fetch_imu_windows on a resident stream and on the host array give the same samples and pre-integrations, and
    try_map_initialization_batch and BatchWindowEstimator give the same results from either."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    n, W, k0 = 2, 3, 20
    ks = list(range(k0 - 1, k0 + n * W))                      # one scan before the first frame: frame 0's messages
    rows = np.concatenate([synth.imu_samples(k - 1, k) for k in ks[1:]])
    stamp = IC.SEC + 0.1 * ks[0] + np.cumsum(rows[:, 6])
    msgs = np.concatenate([stamp[:, None], rows[:, :6]], axis=1)
    stamps = [[IC.SEC + 0.1 * (k0 + W * w + f - 1) for f in range(W + 1)] for w in range(n)]
    rng = np.random.default_rng(23)
    c = M.Context(max_scans=n * W)
    try:
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        frames = []
        for w in range(n):
            frames.append([])
            for f in range(W):
                k, slot = k0 + W * w + f, W * w + f
                c.scan_upload(slot, synth.velo_scan(k), synth.livox_scan(k))
                c.extract(slot, 1)
                c.undistort(slot, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))
                c.downsample(slot, 1)
                T = perturbed(synth.pose_matrix(k), dt=rng.normal(0, 0.02, 3), rotvec=rng.normal(0, 0.003, 3))
                q = Rsc.from_matrix(T[:3, :3]).as_quat()
                frames[w].append(dict(t=stamps[w][f + 1], P=T[:3, 3].copy(), Q=-q if q[3] < 0 else q, V=synth.velocity_at(k) + rng.normal(0, 0.02, 3),
                                      bg=np.zeros(3), ba=np.zeros(3)))
        s = c.imu_stream(4096)
        s.push(msgs[:100])
        s.push(msgs[100:])
        copy = lambda fl: [{kk: (vv.copy() if hasattr(vv, "copy") else vv) for kk, vv in fr.items()} for fr in fl]
        results = {}
        for name, src in (("stream", s), ("host", msgs)):
            smp, pres = odometry.fetch_imu_windows(src, stamps, frames)
            fl, sl = [copy(f) for f in frames], [list(x) for x in smp]
            init = odometry.try_map_initialization_batch(fl, sl, None, c)
            fb = [copy(f) for f in frames]
            best = odometry.BatchWindowEstimator(c, n, gravity=synth.GRAVITY)
            infos = best.estimate([list(range(W * w, W * w + W)) for w in range(n)], fb, pres)
            results[name] = (smp, pres, fl, init, fb, infos)
        a, b = results["stream"], results["host"]
        for w in range(n):
            assert all(19 <= len(x) <= 22 for x in a[0][w])       # (100 ms at 200 Hz; a boundary may fall an ulp beside a message)
            assert [x.tobytes() for x in a[0][w]] == [x.tobytes() for x in b[0][w]]
            assert [None if p is None else bytes(p) for p in a[1][w]] == [None if p is None else bytes(p) for p in b[1][w]]
            assert a[3][w][0] == b[3][w][0] and a[3][w][1].tobytes() == b[3][w][1].tobytes()
            for fa, fbb in zip(a[2][w] + a[4][w], b[2][w] + b[4][w]):
                for key in ("P", "Q", "V", "bg", "ba"):
                    assert np.array_equal(fa[key], fbb[key]), (w, key)
            assert a[5][w]["outer"] == b[5][w]["outer"] and a[5][w]["evaluations"] == b[5][w]["evaluations"]
        s.close()
    finally:
        c.close()
