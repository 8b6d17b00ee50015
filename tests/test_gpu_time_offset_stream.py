"""mml_time_offset_estimate_stream on the device: estimate_timeoffset (unionLidarsAligner.cpp:1021-1166) on a resident Livox
stream.  The yardstick is the oracle (O.time_offset_search) on the FOV rows of the HOST selection (mml_velo_fov_select_batch with
a NULL context) and the x, y, z that were pushed, bit for bit; the stamps are computed here from what was pushed."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

RES, SLICED = 30, 512
N_MSG, MSG_PTS, LAST = 10, 700, 8
T0 = 1600000000 * 10 ** 9
U64 = 1 << 64


def tf_matrix():
    th = 0.03
    return np.array([[np.cos(th), -np.sin(th), 0, 0.05], [np.sin(th), np.cos(th), 0, -0.1], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def data(M, O, synth):
    """Velodyne frames of 300, 4096 and 4097 points (x, y, z, intensity) and one that keeps nothing; ten Livox messages of 700
    points with distinct time bases; the host selection of every frame and, per (frame, tf), the oracle's search against the last
    eight messages -- computed once and left unchanged."""
    frames = [np.ascontiguousarray(synth.velo_scan(31)[::96][:300]), np.ascontiguousarray(synth.velo_scan(32)[::7][:4096]),
              np.ascontiguousarray(synth.velo_scan(33)[::7][:4097])]
    assert [len(f) for f in frames] == [300, 4096, 4097]
    behind = np.zeros((50, 4), np.float32)
    behind[:, 0], behind[:, 1], behind[:, 2] = -5.0, np.linspace(-0.5, 0.5, 50), 0.2
    pts = synth.livox_scan(31, motion=True)[:N_MSG * MSG_PTS].copy()
    msgs, tbs = [], []
    for j in range(N_MSG):
        p = pts[j * MSG_PTS:(j + 1) * MSG_PTS].copy()
        p["offset_time"] = np.arange(MSG_PTS, dtype=np.uint32) * 9000 + 17 * j
        p["_pad"] = 0
        if j == N_MSG - LAST:        # the first of the eight is far away: the best window starts in a later message
            p["x"] += np.float32(200.0)
        msgs.append(p)
        tbs.append(T0 + j * 7000000 + 3 * j * j)
    lxyz = np.concatenate([np.stack([p["x"], p["y"], p["z"]], 1) for p in msgs]).astype(np.float32)
    stamp = np.concatenate([np.uint64(tb) + p["offset_time"].astype(np.uint64) for tb, p in zip(tbs, msgs)])
    sel = [M.velo_fov_select([f]) for f in frames + [behind]]          # ctx None: the host routine
    assert [len(s["xyz"]) for s in sel] == [70, 948, 949, 0]
    begin, end = (N_MSG - LAST) * MSG_PTS, N_MSG * MSG_PTS
    want = {}
    for i in range(3):
        for with_tf in (False, True):
            want[(i, with_tf)] = O.time_offset_search(sel[i]["xyz"], lxyz[begin:end], RES, SLICED, tf_matrix() if with_tf else None)
    return dict(frames=frames, behind=behind, msgs=msgs, tbs=tbs, lxyz=lxyz, stamp=stamp, sel=sel, begin=begin, end=end, want=want)


def push_all(st, d, wire=False, upto=N_MSG):
    from union_cases import to_wire
    for j in range(upto):
        if wire:
            st.push_wire(d["tbs"][j], to_wire(d["msgs"][j]), MSG_PTS)
        else:
            st.push(d["tbs"][j], d["msgs"][j])


def assert_row(got, want, what):
    assert got.get("status", 0) == 0, what                      # (`got` may be the dict of time_offset_search, which has no status)
    assert np.array_equal(got["nn_d2"], want["nn_d2"]), what
    assert got.get("n_windows", len(got["window_error"])) == len(want["window_error"]) == len(got["window_error"]), what
    assert np.array_equal(got["window_error"], want["window_error"]), what
    assert got["best_window"] == want["best_window"] and got["lowest_error"] == want["lowest_error"], what


def same_rows(a, b):
    keys = ("status", "n_kept", "n_windows", "best_window", "lowest_error", "optim_start", "time_offset", "accepted")
    return (all(a[k] == b[k] for k in keys) and np.array_equal(a["nn_d2"], b["nn_d2"]) and np.array_equal(a["window_error"], b["window_error"]))


@pytest.mark.parametrize("with_tf", [False, True])
def test_rows_match_the_oracle_bit_for_bit(M, data, with_tf):
    """Every row against the oracle on the host selection's rows and the pushed coordinates.  Beside it, equality with the
    hand-composed device calls of the same build (velo_fov_select + time_offset_search); that second comparison alone would prove
    nothing, both sides go through the same kernels."""
    d = data
    tf = tf_matrix() if with_tf else None
    c = M.Context(max_scans=1)
    try:
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        rows = c.time_offset_estimate_stream(st, d["begin"], d["end"], d["frames"], [T0 + 10 ** 9] * 3, tf, RES, SLICED)
        hand = []
        for f in d["frames"]:
            s = c.velo_fov_select([f])
            hand.append((s, c.time_offset_search(s["xyz"], d["lxyz"][d["begin"]:d["end"]], RES, SLICED, tf)))
        st.close()
    finally:
        c.close()
    for i in range(3):
        w = d["want"][(i, with_tf)]
        assert len(w["window_error"]) == (LAST * MSG_PTS - SLICED - 1) // RES + 1 and w["best_window"] >= 0
        assert rows[i]["n_kept"] == len(d["sel"][i]["xyz"]) == hand[i][0]["n_kept"][0]
        assert_row(rows[i], w, ("oracle", i))
        assert_row(rows[i], hand[i][1], ("hand-composed", i))


def test_stamps_offset_and_threshold(M, data):
    d = data
    w = d["want"][(1, False)]
    k = d["begin"] + w["best_window"] * RES
    assert w["best_window"] * RES >= MSG_PTS                       # the best window starts beyond the first of the eight messages
    msg, pt = divmod(k, MSG_PTS)
    optim = d["tbs"][msg] + int(d["msgs"][msg]["offset_time"][pt])  # timebase of its message + offset_time
    assert optim == int(d["stamp"][k])
    low = w["lowest_error"]
    later, earlier = optim + 123456789, optim - 5                   # the second wraps in uint64
    c = M.Context(max_scans=1)
    try:
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        f = d["frames"][1]
        at = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f, f], [later, earlier], None, RES, SLICED, error_th=low)
        above = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f], [later], None, RES, SLICED, error_th=np.nextafter(low, np.inf))
        below = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f], [later], None, RES, SLICED, error_th=np.nextafter(low, -np.inf))
        st.close()
    finally:
        c.close()
    for r in at + above + below:
        assert r["best_window"] == w["best_window"] and r["lowest_error"] == low and r["optim_start"] == optim
    assert at[0]["time_offset"] == later - optim == 123456789
    assert at[1]["time_offset"] == (earlier - optim) % U64 == U64 - 5
    assert [at[0]["accepted"], at[1]["accepted"], above[0]["accepted"], below[0]["accepted"]] == [0, 0, 1, 0]   # :1159 is a strict <


def test_stream_geometry(M, data):
    """begin > front after mml_union_assemble_offset moved the front; a stream whose live part has moved to its second array; a
    push_wire stream: the same rows every time."""
    d = data
    w = d["want"][(0, False)]
    f = d["frames"][0]
    vs = [int(d["stamp"][d["begin"]]) + 10 ** 8]
    velo4 = np.ascontiguousarray(d["frames"][0][:40])
    c = M.Context(max_scans=1)
    try:
        # the front moves to 300
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        rows = c.union_assemble_offset(st, 0, [int(d["stamp"][100])], 200, [velo4])
        assert rows["status"][0] == M.UNION_OK and st.state()["front"] == 300
        moved = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f], vs, None, RES, SLICED)[0]
        st.close()
        # capacity 6400: nine messages, the front to 700, the tenth message does not fit behind the ninth: the live part moves
        st = c.livox_stream(6400)
        push_all(st, d, upto=9)
        rows = c.union_assemble_offset(st, 0, [int(d["stamp"][690])], 10, [velo4])
        assert rows["status"][0] == M.UNION_OK and st.state()["front"] == 700
        st.push(d["tbs"][9], d["msgs"][9])
        assert st.state() == {"start_stamp": d["tbs"][0], "front": 700, "tail": 7000, "disorder": 0}
        second = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f], vs, None, RES, SLICED)[0]
        st.close()
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d, wire=True)
        wire = c.time_offset_estimate_stream(st, d["begin"], d["end"], [f], vs, None, RES, SLICED)[0]
        st.close()
    finally:
        c.close()
    k = d["begin"] + w["best_window"] * RES
    for what, r in (("front moved", moved), ("second array", second), ("push_wire", wire)):
        assert_row(r, w, what)
        assert r["optim_start"] == int(d["stamp"][k]) and r["time_offset"] == (vs[0] - int(d["stamp"][k])) % U64, what


def test_range_sizes(M, O, data):
    """An empty range; a range of exactly sliced_points points (no window, the distances filled); one point more (one window)."""
    d = data
    f, xyz = d["frames"][0], d["sel"][0]["xyz"]
    end = d["end"]
    c = M.Context(max_scans=1)
    try:
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        empty = c.time_offset_estimate_stream(st, end, end, [f], [T0], None, RES, SLICED)[0]
        exact = c.time_offset_estimate_stream(st, end - SLICED, end, [f], [T0], None, RES, SLICED)[0]
        one = c.time_offset_estimate_stream(st, end - SLICED - 1, end, [f], [T0], None, RES, SLICED)[0]
        st.close()
    finally:
        c.close()
    assert (empty["status"], empty["n_kept"], empty["n_windows"], empty["best_window"], empty["lowest_error"]) == (0, len(xyz), 0, -1, 1e6)
    assert (empty["optim_start"], empty["time_offset"], empty["accepted"]) == (0, 0, 0) and len(empty["nn_d2"]) == 0
    w = O.time_offset_search(xyz, d["lxyz"][end - SLICED:end], RES, SLICED)
    assert len(w["window_error"]) == 0
    assert_row(exact, w, "exactly sliced_points")
    assert exact["best_window"] == -1 and len(exact["nn_d2"]) == SLICED and (exact["optim_start"], exact["accepted"]) == (0, 0)
    w = O.time_offset_search(xyz, d["lxyz"][end - SLICED - 1:end], RES, SLICED)
    assert len(w["window_error"]) == 1
    assert_row(one, w, "sliced_points + 1")
    assert one["best_window"] == 0 and one["optim_start"] == int(d["stamp"][end - SLICED - 1]) and one["accepted"] == 1


def test_frames_in_one_call(M, data):
    """n = 1 and 5; the same frame twice; a frame that keeps nothing between two that do; five frames in one call equal five calls."""
    d = data
    fr = [d["frames"][0], d["behind"], d["frames"][2], d["frames"][0], d["frames"][1]]
    vs = [T0 + 10 ** 9 + 1000 * i for i in range(5)]
    tf = tf_matrix()
    c = M.Context(max_scans=1)
    try:
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        five = c.time_offset_estimate_stream(st, d["begin"], d["end"], fr, vs, tf, RES, SLICED)
        solo = [c.time_offset_estimate_stream(st, d["begin"], d["end"], [fr[i]], [vs[i]], tf, RES, SLICED)[0] for i in range(5)]
        st.close()
    finally:
        c.close()
    for i, which in ((0, 0), (2, 2), (3, 0), (4, 1)):
        assert_row(five[i], d["want"][(which, True)], i)
    for i in range(5):
        assert same_rows(five[i], solo[i]), i
    r = five[1]
    assert (r["status"], r["n_kept"], r["n_windows"], r["best_window"], r["lowest_error"]) == (M.TOFS_ROW_NO_VELO_IN_FOV, 0, 0, -1, 1e6)
    assert (r["optim_start"], r["time_offset"], r["accepted"]) == (0, 0, 0)
    assert five[0]["time_offset"] + 3000 == five[3]["time_offset"] and np.array_equal(five[0]["nn_d2"], five[3]["nn_d2"])


def test_the_stream_is_only_read(M, data):
    """mml_livox_stream_state_get before and after is equal, and a following mml_union_assemble_offset fills its slot with the
    same digest as on a twin stream that never saw the estimate."""
    d = data
    velo4 = np.ascontiguousarray(d["frames"][0])
    start = int(d["stamp"][d["begin"] + 40])
    digs, fronts = [], []
    for estimate in (True, False):
        c = M.Context(max_scans=1)
        try:
            st = c.livox_stream(N_MSG * MSG_PTS)
            push_all(st, d)
            if estimate:
                before = st.state()
                c.time_offset_estimate_stream(st, d["begin"], d["end"], d["frames"], [T0] * 3, tf_matrix(), RES, SLICED)
                assert st.state() == before
            rows = c.union_assemble_offset(st, 0, [start], SLICED, [velo4], tf_matrix())
            assert rows["status"][0] == M.UNION_OK and rows["n_livox"][0] == SLICED
            fronts.append(st.state())
            c.extract(0, 1)
            digs.append(c.slot_digest(0, 1))
            st.close()
        finally:
            c.close()
    assert fronts[0] == fronts[1] and np.array_equal(digs[0], digs[1])


def raw_call(M, c, st, begin, end, n, data, bo, npts, step, offs, vs, res, sliced, nn, err, wo, rows):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = M.lib().mml_time_offset_estimate_stream(c._h, None if st is None else st._h, begin, end, n, p(data), p(bo), p(npts), step, offs[0], offs[1],
                                                 offs[2], p(vs), None, res, sliced, 1e6, p(nn), p(err), p(wo), p(rows))
    return rc, M.lib().mml_last_error(c._h).decode()


def test_refusals_write_nothing_and_name_the_frame(M, data):
    d = data
    fr = [d["frames"][0], d["frames"][1]]
    raw, bo, npts, step = M.velo_fov_pack(fr)
    vs = np.array([T0, T0], np.uint64)
    L = d["end"] - d["begin"]
    each = (L - SLICED - 1) // RES + 1
    wo = np.array([0, each, 2 * each], np.int64)
    big_n = M.FOV_BATCH_MAX + 1
    inv, cap = M.MML_ERR_INVALID, M.MML_ERR_CAPACITY
    c, other = M.Context(max_scans=1), M.Context(max_scans=1)
    small_velo = M.Context(max_scans=1, max_velo_points=4000)
    small_map = M.Context(max_scans=1, max_map_points=4000)
    try:
        streams = {x: x.livox_stream(N_MSG * MSG_PTS) for x in (c, other, small_velo, small_map)}
        for s in streams.values():
            push_all(s, d)
        st = streams[c]
        neg = npts.copy()
        neg[1] = -1
        dec = wo.copy()
        dec[2] = dec[1] - 1
        K = dict(ctx=c, st=st, begin=d["begin"], end=d["end"], n=2, data=raw, bo=bo, npts=npts, step=step, offs=(0, 4, 8), vs=vs, res=RES,
                 sliced=SLICED, wo=wo, with_out=True)
        cases = [("n = 0", dict(n=0), inv, "n = 0"), ("n above the maximum", dict(n=big_n, bo=np.zeros(big_n, np.int64), npts=np.zeros(big_n, np.int32)),
                                                      inv, "n = %d" % big_n),
                 ("NULL n_points", dict(npts=None), inv, "null"), ("point_step", dict(step=8), inv, "point_step"),
                 ("field offset", dict(offs=(0, 4, 14)), inv, "offset 14"), ("negative count", dict(npts=neg), inv, "frame 1"),
                 ("NULL data", dict(data=None), inv, "data is null"), ("NULL stream", dict(st=None), inv, "null"),
                 ("NULL stamps", dict(vs=None), inv, "null"), ("NULL out", dict(with_out=False), inv, "null"),
                 ("NULL window_offsets", dict(wo=None), inv, "null"), ("decreasing window offsets", dict(wo=dec), inv, "frame 1"),
                 ("foreign stream", dict(st=streams[other]), inv, "another context"), ("resolution", dict(res=0), inv, "search_resolution"),
                 ("sliced", dict(sliced=0), inv, "sliced_points"), ("begin before the front", dict(begin=-1), inv, "range"),
                 ("end beyond the tail", dict(end=d["end"] + 1), inv, "range"), ("reversed range", dict(begin=d["end"], end=d["begin"]), inv, "range"),
                 ("above max_velo_points", dict(ctx=small_velo, st=streams[small_velo]), cap, "frame 1"),
                 ("above max_map_points", dict(ctx=small_map, st=streams[small_map]), cap, "frame 1")]
        for what, change, code, text in cases:
            k = dict(K, **change)
            nn, err = np.full(2 * L, -7.5, np.float32), np.full(2 * each, -7.5)
            rows = np.full(2, -9, M.TOFS_ROW_DTYPE)
            rc, msg = raw_call(M, k["ctx"], k["st"], k["begin"], k["end"], k["n"], k["data"], k["bo"], k["npts"], k["step"], k["offs"], k["vs"], k["res"],
                               k["sliced"], nn, err, k["wo"], rows if k["with_out"] else None)
            assert rc == code, (what, rc, msg)
            assert "mml_time_offset_estimate_stream" in msg and text in msg, (what, msg)
            assert np.all(nn == -7.5) and np.all(err == -7.5) and np.all(rows["status"] == -9) and np.all(rows["n_kept"] == -9), what
        # the context and the stream are as good as before
        good = c.time_offset_estimate_stream(st, d["begin"], d["end"], fr, [T0, T0], None, RES, SLICED)
        assert_row(good[0], d["want"][(0, False)], "after the refusals")
        assert_row(good[1], d["want"][(1, False)], "after the refusals")
        for s in streams.values():
            s.close()
    finally:
        for x in (c, other, small_velo, small_map):
            x.close()


def test_synchronisations_launches_and_scratch_life_cycle(M, data):
    """With profiling on every call shows ONE launch of each of its three phases -- the three host synchronisations -- for n = 1
    and n = 5 alike (an empty range: the counts alone).  A large call, a small one, the hand-composed calls in between, on two
    contexts: the blocks only grow and every result stays what the oracle says.  The stream is destroyed before its context."""
    d = data
    five = [d["frames"][i % 3] for i in range(5)]
    ctxs = [M.Context(max_scans=1), M.Context(max_scans=1)]
    try:
        for c in ctxs:
            st = c.livox_stream(N_MSG * MSG_PTS)
            push_all(st, d)
            c.profile_enable(True)
            c.profile_reset()
            one = c.time_offset_estimate_stream(st, d["begin"], d["end"], five[:1], [T0], None, RES, SLICED)
            p1 = c.profile_get()
            c.profile_reset()
            many = c.time_offset_estimate_stream(st, d["begin"], d["end"], five, [T0] * 5, None, RES, SLICED)
            p5 = c.profile_get()
            c.profile_reset()
            c.time_offset_estimate_stream(st, d["end"], d["end"], five, [T0] * 5, None, RES, SLICED)
            p0 = c.profile_get()
            stages = ("velo_fov", "tofs_box", "tofs_search")
            assert [p1[s][1] for s in stages] == [1, 1, 1] == [p5[s][1] for s in stages], (p1, p5)
            assert p0["velo_fov"][1] == 1 and all(p0.get(s, (0, 0))[1] == 0 for s in stages[1:]), p0
            c.profile_enable(False)
            sel = c.velo_fov_select([d["frames"][2]])
            hand = c.time_offset_search(sel["xyz"], d["lxyz"][d["begin"]:d["end"]], RES, SLICED)
            again = c.time_offset_estimate_stream(st, d["begin"], d["end"], five[:1], [T0], None, RES, SLICED)
            assert_row(one[0], d["want"][(0, False)], "one")
            for i in range(5):
                assert_row(many[i], d["want"][(i % 3, False)], ("five", i))
            assert_row(hand, d["want"][(2, False)], "the hand-composed calls after the stream call")
            assert same_rows(again[0], one[0])
            st.close()
    finally:
        for c in ctxs:
            c.close()


def test_odometry_time_offset_from_stream(M, data):
    """odometry.time_offset_from_stream: the gate's frame, then its row; all_frames=True: every queued frame."""
    d = data
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    hori = d["tbs"][-1]
    sec = 10 ** 9
    vs = [hori - 2 * sec, hori - sec, hori - sec // 10, hori + sec]         # the gate pops the last two: frame 1 is selected
    fr = [d["frames"][0], d["frames"][1], d["frames"][2], d["frames"][0]]
    marks = [j * MSG_PTS for j in range(N_MSG + 1)]
    assert M.time_offset_gate(vs, hori, N_MSG) == (1, M.TOFS_GATE_OK)
    c = M.Context(max_scans=1)
    try:
        st = c.livox_stream(N_MSG * MSG_PTS)
        push_all(st, d)
        row, selected, status = odometry.time_offset_from_stream(c, st, marks, fr, vs, hori, None, RES, SLICED)
        rows, _, _ = odometry.time_offset_from_stream(c, st, marks, fr, vs, hori, None, RES, SLICED, all_frames=True)
        none = odometry.time_offset_from_stream(c, st, marks[:8], fr, vs, hori, None, RES, SLICED)
        st.close()
    finally:
        c.close()
    w = d["want"][(1, False)]
    assert (selected, status) == (1, M.TOFS_GATE_OK)
    assert_row(row, w, "selected frame")
    k = d["begin"] + w["best_window"] * RES
    assert row["optim_start"] == int(d["stamp"][k]) and row["time_offset"] == (vs[1] - int(d["stamp"][k])) % U64 and row["accepted"] == 1
    assert len(rows) == 4 and same_rows(rows[1], row) and rows[3]["time_offset"] == (vs[3] - rows[3]["optim_start"]) % U64
    assert none == (None, -1, M.TOFS_GATE_TOO_FEW_MESSAGES)


def test_cpp_adapter_estimate_timeoffset(M, data, tmp_path):
    """mml::LivoxPointQueue's marks and mml::estimate_timeoffset through tests/cpp/time_offset_stream_probe.cpp: the selected
    frame's row as the Python path gives it."""
    d = data
    exe = tmp_path / "time_offset_stream_probe"
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
           os.path.join(ROOT, "tests", "cpp", "time_offset_stream_probe.cpp"), "-o", str(exe), "-L", libdir, "-lmmloam_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    hori = d["tbs"][-1]
    sec = 10 ** 9
    vs = [hori - 2 * sec, hori - sec, hori + sec]
    fr = [d["frames"][0], d["frames"][1], d["frames"][2]]
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as f:
        f.write(np.array([N_MSG, len(fr), RES, SLICED], np.int32).tobytes())
        f.write(np.array([hori], np.uint64).tobytes())
        for tb, m in zip(d["tbs"], d["msgs"]):
            f.write(np.array([tb], np.uint64).tobytes() + np.array([len(m)], np.int32).tobytes() + m.tobytes())
        for s, v in zip(vs, fr):
            f.write(np.array([s], np.uint64).tobytes() + np.array([len(v)], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes())
    run = subprocess.run([str(exe), str(scene)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    marks = [ln for ln in lines if ln and ln[0] == "mark"]
    assert [(int(m[1]), int(m[2]), int(m[3])) for m in marks] == [(d["tbs"][j], j * MSG_PTS, MSG_PTS) for j in range(N_MSG)]
    r = [ln for ln in lines if ln and ln[0] == "row"][0]
    w = d["want"][(1, False)]
    k = d["begin"] + w["best_window"] * RES
    assert [int(x) for x in r[1:7]] == [0, 1, 0, len(d["sel"][1]["xyz"]), len(w["window_error"]), w["best_window"]]
    assert float.fromhex(r[7]) == w["lowest_error"]
    assert int(r[8]) == int(d["stamp"][k]) and int(r[9]) == (vs[1] - int(d["stamp"][k])) % U64 and int(r[10]) == 1
    few = [ln for ln in lines if ln and ln[0] == "few"][0]
    assert [int(x) for x in few[1:3]] == [M.TOFS_GATE_TOO_FEW_MESSAGES, -1]
    assert "TIME_OFFSET_STREAM_PROBE_DONE" in run.stdout
