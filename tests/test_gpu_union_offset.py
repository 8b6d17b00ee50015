"""mml_union_assemble_offset on the device: the aligner's time-offset mode, a fixed count of Livox points per Velodyne frame cut
out of the device stream into scan slots.  The yardstick is tests/union_offset_ref.py -- the reference's one-stamp overload
walking and erasing list-backed queues (unionLidarsAligner.cpp:872-1009), which shares no code with csrc/union_plan.h -- for the
rows, the stream's front and the Livox records, to the byte; union_ref.transform_velo (a float32 numpy evaluation of the kernel's
expression) for the Velodyne rows.  A test is a script of pushes and assemble calls that runs once on the yardstick and once on
the device.  Small shapes on purpose: 8 slots of 512 + 256 points, streams of about 900 points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import union_cases as UC  # noqa: E402
import union_offset_ref as OR  # noqa: E402
import union_ref as UR  # noqa: E402

pytestmark = pytest.mark.gpu

HS = UC.HS
MAXL = 256
GAP = 5 * 10 ** 9   # the last message starts 5 s late: stamps and in-frame offsets above 2^32 ns
TH = 0.3
TF = np.array([[np.cos(TH), -np.sin(TH), 0.01, 0.25], [np.sin(TH), np.cos(TH), -0.02, -1.5], [0.015, 0.02, 1, 0.125], [0, 0, 0, 1]], np.float32)


def context(M):
    return M.Context(max_scans=8, max_velo_points=512, max_livox_points=MAXL)


def ordered_offsets(rng, n, span=10 ** 8):
    return np.sort(rng.integers(0, span, n))


def velo_clouds(rng, sizes):
    return [rng.uniform(-30, 30, (n, 4)).astype(np.float32) for n in sizes]


# ---- a script: ("push", msg) | ("offset", first_slot, starts, c, velo_list) | ("interval", first_slot, bounds, velo_list) ----
def run_yardstick(script, tf, maxl=MAXL):
    """Per assemble call (rows FRAME_DTYPE, [(velo rows, livox records) per frame]); then (front, tail)."""
    a = OR.OffsetAligner()
    out, tail = [], 0
    for op in script:
        if op[0] == "push":
            a.transform_hori_timestamp([op[1]])
            tail += len(op[1][1])
            continue
        rows, frames = [], []
        if op[0] == "offset":
            _, first, starts, c, velo = op
            for t, v in zip(starts, velo):
                r, p = a.pub_horipoints_given_stamp_1(int(t), c)
                rows.append(r)
                frames.append((UR.transform_velo(v, tf), p))
        else:
            _, first, bounds, velo = op
            for i, v in enumerate(velo):
                r, p = a.pub_horipoints_given_stamp(int(bounds[i]), int(bounds[i + 1]), maxl)
                rows.append(r)
                frames.append((UR.transform_velo(v, tf), p))
        out.append((np.array(rows, dtype=UR.FRAME_DTYPE), frames))
    return out, (a.erased, tail)


def run_device(c, st, script, tf, wire=False, singles=False):
    """The same from the device; singles: every assemble call of k frames as k calls of one frame."""
    out = []
    for op in script:
        if op[0] == "push":
            tb, p = op[1]
            if wire:
                st.push_wire(tb, UC.to_wire(p), len(p))
            else:
                st.push(tb, p)
            continue
        first, velo = op[1], op[-1]
        k = len(velo)
        if op[0] == "offset":
            starts, n = op[2], op[3]
            if singles:
                rows = np.concatenate([c.union_assemble_offset(st, first + i, starts[i:i + 1], n, velo[i:i + 1], tf) for i in range(k)])
            else:
                rows = c.union_assemble_offset(st, first, starts, n, velo, tf)
        else:
            bounds = op[2]
            if singles:
                rows = np.concatenate([c.union_assemble(st, first + i, bounds[i:i + 2], velo[i:i + 1], tf) for i in range(k)])
            else:
                rows = c.union_assemble(st, first, bounds, velo, tf)
        out.append((rows, [c.scan_raw_download(first + i) for i in range(k)]))
    state = st.state()
    return out, state


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, ((gr, gf), (wr, wf)) in enumerate(zip(got, want)):
        assert gr.dtype == wr.dtype
        for name in wr.dtype.names:
            assert np.array_equal(gr[name], wr[name]), "%s: call %d: %s differs\n got %s\nwant %s" % (what, k, name, gr, wr)
        for i, ((gv, gl), (wv, wl)) in enumerate(zip(gf, wf)):
            assert gv.shape == wv.shape and gv.tobytes() == wv.tobytes(), "%s: call %d: Velodyne rows of frame %d" % (what, k, i)
            assert len(gl) == len(wl) and gl.tobytes() == wl.tobytes(), "%s: call %d: Livox records of frame %d" % (what, k, i)


def fill_slots(c, n_slots, seed=5):
    """Something else in every slot first, so that what a call leaves there is the call's."""
    rng = np.random.default_rng(seed)
    for s in range(n_slots):
        c.scan_upload(s, rng.uniform(-1, 1, (40 + s, 4)).astype(np.float32), UC.message(0, np.arange(30 + s), 9)[1])
    c.synchronize()


@pytest.fixture(scope="module")
def script4():
    """Four messages of 220, 300, 100 and 280 points at 10 Hz, the last one 5 s late (900 points), and three calls:
      c = 1: one point; c = 103 (515 dwords: no multiple of 256, more than one block of the gather): a frame after a walk, then a
      start past the last stamp -- NOT_REACHED, which leaves point 619; after the last message c = 103 again: 103 points that
      span the 5 s (offsets above 2^32, truncated), the remainder of 50 points, then EMPTY twice.
    Velodyne clouds of 300, 512 (full), 0, 77, 1, 257 (256 + 1) and 5 rows."""
    rng = np.random.default_rng(11)
    late = HS + 2 * 10 ** 8 + GAP
    msgs = [UC.message(HS, ordered_offsets(rng, 220), 1), UC.message(HS + 10 ** 8, ordered_offsets(rng, 300), 2),
            UC.message(HS + 2 * 10 ** 8, ordered_offsets(rng, 100), 3), UC.message(late, ordered_offsets(rng, 280), 4)]
    hs, S = UC.stamps_of(msgs)
    velo = velo_clouds(rng, (300, 512, 0, 77, 1, 257, 5))
    script = [("push", msgs[0]), ("push", msgs[1]), ("push", msgs[2]),
              ("offset", 0, [HS - 10 ** 7], 1, velo[0:1]),
              ("offset", 1, [HS + 12 * 10 ** 7, HS + 4 * 10 ** 8], 103, velo[1:3]),
              ("push", msgs[3]),
              ("offset", 3, [HS + 10 ** 8, hs + int(S[850]), hs + int(S[850]), late + 10 ** 9], 103, velo[3:7])]
    want, ends = run_yardstick(script, TF)
    assert [list(r["status"]) for r, _ in want] == [[0], [0, 2], [0, 0, 1, 1]]
    assert [list(r["n_livox"]) for r, _ in want] == [[1], [103, 0], [103, 900 - int(want[2][0][1]["begin"]), 0, 0]]
    assert want[1][0][0]["begin"] > 1 and want[1][0][1]["front_after"] == 619      # a walk; NOT_REACHED drained to the last point
    assert 0 < want[2][0][1]["n_livox"] < 103 and ends == (900, 900)
    k = int(want[2][0][0]["end"]) - 1   # the frame across the 5 s: an in-frame offset above 2^32, truncated
    assert hs + int(S[k]) - (HS + 10 ** 8) > 2 ** 32 and int(S.max()) > 2 ** 32
    return dict(script=script, want=want, ends=ends)


def test_slots_rows_and_stream_equal_the_yardstick(M, script4):
    d = script4
    c = context(M)
    try:
        fill_slots(c, 8)
        keep = c.scan_raw_download(7)
        st = c.livox_stream(2000)
        got, state = run_device(c, st, d["script"], TF)
        untouched = c.scan_raw_download(7)
        st.close()
    finally:
        c.close()
    assert_same(got, d["want"], "script4")
    assert all(np.all(l["_pad"] == 0) for _, frames in got for _, l in frames)
    assert state == {"start_stamp": HS, "front": d["ends"][0], "tail": d["ends"][1], "disorder": 0}
    assert untouched[0].tobytes() == keep[0].tobytes() and untouched[1].tobytes() == keep[1].tobytes()
    # the rows are also what the host-only plan gives for the same stream (held to the yardstick by test_union_offset_plan.py)
    msgs = [op[1] for op in d["script"] if op[0] == "push"]
    hs, S = UC.stamps_of(msgs)
    rc, plan = M.union_plan_offset(S, 619, 900, hs, d["script"][-1][2], 103)
    assert rc == M.MML_OK and plan.tobytes() == got[2][0].tobytes()


def test_batch_equals_singles(M, script4):
    d = script4
    out = []
    for singles in (False, True):
        c = context(M)
        try:
            st = c.livox_stream(2000)
            out.append(run_device(c, st, d["script"], None, singles=singles))
            st.close()
        finally:
            c.close()
    (ga, sa), (gb, sb) = out
    assert sa == sb
    for (ra, _), (rb, _) in zip(ga, gb):
        assert ra.tobytes() == rb.tobytes()
    assert_same(ga, gb, "batch against singles")
    assert_same(ga, run_yardstick(d["script"], None)[0], "batch, no transform")


def test_push_forms(M, script4):
    d = script4
    out = []
    for wire in (False, True):
        c = context(M)
        try:
            st = c.livox_stream(2000)
            out.append(run_device(c, st, d["script"], TF, wire=wire))
            st.close()
        finally:
            c.close()
    assert out[0][1] == out[1][1]
    assert_same(out[1][0], out[0][0], "wire against struct")
    assert_same(out[1][0], d["want"], "wire")


def test_compaction(M):
    """capacity_points = 700: eight messages of 220 points with a 150-point frame cut after each; the live part has to move to the
    front of the other array more than once (modelled below by the rule the header states).  Same results as with ample capacity."""
    rng = np.random.default_rng(8)
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, 220), 40 + m) for m in range(8)]
    velo = velo_clouds(rng, [9 + m for m in range(8)])
    script = []
    for m in range(8):
        script += [("push", msgs[m]), ("offset", m % 4, [HS + m * 10 ** 8 + 10 ** 7], 150, velo[m:m + 1])]
    want, ends = run_yardstick(script, None)
    assert all(r["status"][0] == UR.OK and r["n_livox"][0] == 150 for r, _ in want)
    base = front = tail = moves = 0
    for m in range(8):
        if tail - base + 220 > 700:
            base, moves = front, moves + 1
        tail += 220
        front = int(want[m][0][0]["front_after"])
    assert moves >= 2 and tail - front <= 700
    c = context(M)
    try:
        small, ample = c.livox_stream(700), c.livox_stream(4000)
        got_small, state_small = run_device(c, small, script, None)
        got_ample, state_ample = run_device(c, ample, script, None)
        small.close()
        ample.close()
    finally:
        c.close()
    assert_same(got_small, want, "capacity 700")
    assert_same(got_ample, want, "capacity 4000")
    assert state_small == state_ample == {"start_stamp": HS, "front": ends[0], "tail": 1760, "disorder": 0}


def test_not_reached_drains_to_one_point_and_a_later_push_continues(M):
    rng = np.random.default_rng(14)
    msgs = [UC.message(HS, ordered_offsets(rng, 50, 10 ** 6), 1), UC.message(HS + 10 ** 8, ordered_offsets(rng, 60, 10 ** 6), 2)]
    velo = velo_clouds(rng, (3, 4, 5))
    script = [("push", msgs[0]), ("offset", 0, [HS + 10 ** 7, HS + 2 * 10 ** 7], 20, velo[0:2]), ("push", msgs[1]),
              ("offset", 2, [HS + 3 * 10 ** 7], 20, velo[2:3])]
    want, ends = run_yardstick(script, TF)
    assert [tuple(r) for r in want[0][0]] == [(UR.NOT_REACHED, 0, 49, 49, 49)] * 2
    assert tuple(want[1][0][0]) == (UR.OK, 20, 50, 70, 70)   # the point that was left is behind the new stamp: erased, not emitted
    c = context(M)
    try:
        fill_slots(c, 3)
        st = c.livox_stream(200)
        got, state = run_device(c, st, script[:2], TF)
        assert state == {"start_stamp": HS, "front": 49, "tail": 50, "disorder": 0}
        more, state = run_device(c, st, script[2:], TF)
        st.close()
    finally:
        c.close()
    assert_same(got + more, want, "drain, push, continue")
    assert len(got[0][1][0][1]) == 0 and len(got[0][1][0][0]) == 3   # a NOT_REACHED frame: its Velodyne part, no Livox point
    assert state == {"start_stamp": HS, "front": ends[0], "tail": 110, "disorder": 0}


def test_interleaved_with_the_interval_mode(M):
    """mml_union_assemble and mml_union_assemble_offset on ONE stream equal the reference's two overloads on one queue."""
    rng = np.random.default_rng(17)
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, 240), 60 + m) for m in range(4)]
    velo = velo_clouds(rng, (10, 20, 30, 40, 50, 60, 70))
    e8 = 10 ** 8
    script = [("push", msgs[0]), ("push", msgs[1]),
              ("interval", 0, [HS + 10 ** 7, HS + 4 * 10 ** 7, HS + 7 * 10 ** 7], velo[0:2]),       # leaves 100 points before its end
              ("offset", 2, [HS + 6 * 10 ** 7, HS + e8], 103, velo[2:4]),                             # starts inside them
              ("push", msgs[2]), ("push", msgs[3]),
              ("interval", 4, [HS + 2 * e8, HS + 2 * e8 + 5 * 10 ** 7], velo[4:5]),
              ("offset", 5, [HS + 3 * e8, HS + 5 * e8], 200, velo[5:7]),                              # 200 of 240; then NOT_REACHED
              ("interval", 7, [HS + 3 * e8, HS + 6 * e8], velo[0:1])]                                 # the one point that was left
    want, ends = run_yardstick(script, TF)
    assert [list(r["status"]) for r, _ in want] == [[0, 0], [0, 0], [0], [0, 2], [0]]
    assert want[1][0][0]["begin"] < want[0][0][1]["end"] and want[3][0][0]["n_livox"] == 200
    assert tuple(want[3][0][1]) == (UR.NOT_REACHED, 0, 959, 959, 959) and tuple(want[4][0][0]) == (UR.OK, 1, 959, 960, 959)
    c = context(M)
    try:
        st = c.livox_stream(1000)
        got, state = run_device(c, st, script, TF)
        st.close()
    finally:
        c.close()
    assert_same(got, want, "interleaved")
    assert state == {"start_stamp": HS, "front": ends[0], "tail": 960, "disorder": 0}


def test_a_batch_across_the_plan_kernels_round(M):
    """1 030 frames in one call (the plan kernel resolves 1 024 per round) of c = 3 points out of a 5 000-point stream, on a
    context of 1 088 slots of 64 + 64 points; the last five starts lie past the stream."""
    rng = np.random.default_rng(23)
    n, count = 5000, 1030
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, n // 4), 80 + m) for m in range(4)]
    hs, S = UC.stamps_of(msgs)
    starts = [hs + int(S[(23 * i) // 5]) for i in range(count - 5)] + [hs + int(S[-1]) + 1 + i for i in range(5)]
    velo = velo_clouds(rng, [i % 5 for i in range(count)])
    script = [("push", m) for m in msgs] + [("offset", 50, starts, 3, velo)]
    want, ends = run_yardstick(script, TF)
    status = want[0][0]["status"]
    assert np.all(status[:count - 5] == UR.OK) and np.all(status[count - 5:] == UR.NOT_REACHED) and ends == (n - 1, n)
    assert np.any(want[0][0]["begin"][1:] > want[0][0]["end"][:-1])   # (walks between the frames)
    c = M.Context(max_scans=1088, max_velo_points=64, max_livox_points=64, max_features=256, max_map_points=4096)
    try:
        st = c.livox_stream(n)
        got, state = run_device(c, st, script, TF)
        st.close()
    finally:
        c.close()
    assert_same(got, want, "1 030 frames")
    assert state == {"start_stamp": HS, "front": n - 1, "tail": n, "disorder": 0}


def test_downstream_extract_sees_the_same_slot(M, synth):
    """The assembled slot is in the state mml_scan_upload leaves: extraction of both gives the same digest."""
    lv = synth.livox_scan(3, n=240)
    lv["_pad"] = 0x5A
    velo = synth.velo_scan(3, n_az=32)   # 512 rows
    tf = np.eye(4, dtype=np.float32)
    tf[:3, 3] = [0.1, -0.05, 0.02]
    script = [("push", (HS, lv)), ("offset", 0, [HS + 10 ** 6], 200, [velo])]
    want, _ = run_yardstick(script, tf)
    assert want[0][0][0]["status"] == UR.OK and want[0][0][0]["n_livox"] > 150
    c = context(M)
    try:
        st = c.livox_stream(500)
        run_device(c, st, script, tf)
        c.scan_upload(1, want[0][1][0][0], want[0][1][0][1])
        c.extract(0, 2)
        dig = c.slot_digest(0, 2)
        info = c.scan_info(0)
        st.close()
    finally:
        c.close()
    assert info.n_points > 0
    assert np.array_equal(dig[0], dig[1])


def test_refusals_leave_slots_counts_and_stream_untouched(M):
    rng = np.random.default_rng(21)
    c, other = context(M), M.Context(max_scans=1, max_velo_points=64, max_livox_points=64)
    try:
        fill_slots(c, 8)
        was = [c.scan_raw_download(s) for s in range(8)]
        st = c.livox_stream(600)
        st.push(*UC.message(HS, ordered_offsets(rng, 200), 1))
        foreign = other.livox_stream(10)
        before = st.state()
        velo = [np.ones((3, 4), np.float32)] * 2
        ok = [HS, HS + 10]
        refused = [
            (M.MML_ERR_INVALID, dict(first=0, starts=[], n=3, velo=[])),                                  # count 0
            (M.MML_ERR_INVALID, dict(first=0, starts=[HS + 10, HS], n=3, velo=velo)),                     # decreasing starts
            (M.MML_ERR_INVALID, dict(first=7, starts=ok, n=3, velo=velo)),                                # slot range
            (M.MML_ERR_INVALID, dict(first=-1, starts=ok, n=3, velo=velo)),
            (M.MML_ERR_INVALID, dict(first=0, starts=ok, n=0, velo=velo)),                                # sliced_points < 1
            (M.MML_ERR_INVALID, dict(first=0, starts=ok, n=-5, velo=velo)),
            (M.MML_ERR_CAPACITY, dict(first=0, starts=ok, n=MAXL + 1, velo=velo)),                        # sliced_points > max_livox_points
            (M.MML_ERR_CAPACITY, dict(first=0, starts=ok, n=3, velo=[np.ones((513, 4), np.float32), velo[0]])),   # > max_velo_points
            (M.MML_ERR_INVALID, dict(first=0, starts=ok, n=3, velo=velo, stream=foreign)),                # a stream of another context
        ]
        for code, a in refused:
            with pytest.raises(M.MmlError) as e:
                c.union_assemble_offset(a.get("stream", st), a["first"], a["starts"], a["n"], a["velo"])
            assert e.value.code == code, a
        # NULL arguments, through the C-ABI itself
        L = M.lib()
        starts, vo, rows = np.array(ok, np.uint64), np.array([0, 3, 6], np.int32), np.zeros(2, M.UNION_FRAME_DTYPE)
        cloud = np.ones((6, 4), np.float32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        for args in ((None, starts, cloud, vo, rows), (st._h, None, cloud, vo, rows), (st._h, starts, None, vo, rows),
                     (st._h, starts, cloud, None, rows), (st._h, starts, cloud, vo, None)):
            s_, t_, v_, o_, r_ = args
            assert L.mml_union_assemble_offset(c._h, s_, 0, 2, p(t_), 3, p(v_), p(o_), None, p(r_)) == M.MML_ERR_INVALID
        assert not rows.tobytes().strip(b"\0")
        assert st.state() == before == {"start_stamp": HS, "front": 0, "tail": 200, "disorder": 0}
        # a message whose first stamp lies below the previous tail: counted at the push, refused by the next assemble
        st.push(*UC.message(HS + 10 ** 6, ordered_offsets(rng, 100), 4))   # its own stamps ordered, its first one early
        assert st.state()["disorder"] == 1
        with pytest.raises(M.MmlError) as e:
            c.union_assemble_offset(st, 0, ok, 3, velo)
        assert e.value.code == M.MML_ERR_STATE
        assert st.state() == {"start_stamp": HS, "front": 0, "tail": 300, "disorder": 1}
        now = [c.scan_raw_download(s) for s in range(8)]
        for (v0, l0), (v1, l1) in zip(was, now):
            assert v0.tobytes() == v1.tobytes() and l0.tobytes() == l1.tobytes()
        foreign.close()
        st.close()
    finally:
        other.close()
        c.close()


@pytest.mark.parametrize("count", [1, 6])
def test_one_plan_and_one_gather_launch_per_call(M, count):
    rng = np.random.default_rng(31)
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, 200), m) for m in range(4)]
    starts = [HS + 5 * 10 ** 7 + i * 6 * 10 ** 7 for i in range(count)]
    velo = velo_clouds(rng, [100 + i for i in range(count)])
    c = context(M)
    try:
        st = c.livox_stream(2000)
        for m in msgs:
            st.push(*m)
        c.synchronize()
        c.profile_enable(True)
        c.profile_reset()
        rows = c.union_assemble_offset(st, 0, starts, 103, velo, TF)
        prof = c.profile_get()
        st.close()
    finally:
        c.close()
    assert len(rows) == count and np.all(rows["status"] == UR.OK)
    assert prof["union_offset_plan"][1] == 1 and prof["union_gather"][1] == 1
    assert prof.get("union_plan", (0.0, 0))[1] == 0
