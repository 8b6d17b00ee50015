"""mml_union_assemble on the device: a Livox stream pushed message by message and cut into scan slots.  The yardstick is
tests/union_ref.py -- the reference's walks over list-backed queues (unionLidarsAligner.cpp:736-868), which shares no code with
csrc/union_plan.h -- for the Livox records, to the byte; a float32 numpy evaluation of k_tofs_tf's expression for the Velodyne
rows; mml_union_plan (itself held to the yardstick by tests/test_union_plan.py) for the rows.  Small shapes on purpose: 8
slots of 512 + 256 points, streams of 3-5 messages of 100-300 points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import union_cases as UC  # noqa: E402
import union_ref as UR  # noqa: E402

pytestmark = pytest.mark.gpu

HS = UC.HS
MAXL = 256
GAP = 5 * 10 ** 9   # the last message starts 5 s late: stamps and in-frame offsets above 2^32 ns


def context(M):
    return M.Context(max_scans=8, max_velo_points=512, max_livox_points=MAXL)


def ordered_offsets(rng, n, span=10 ** 8):
    return np.sort(rng.integers(0, span, n))


@pytest.fixture(scope="module")
def stream4():
    """Four messages of 220, 300, 100 and 180 points at 10 Hz (the last one 5 s late) and six frames that do not line up with
    them: one starts before the stream, one is empty (start == end), one spans the 5 s.  Every frame holds at most 256 points."""
    rng = np.random.default_rng(11)
    msgs = [UC.message(HS, ordered_offsets(rng, 220), 1), UC.message(HS + 10 ** 8, ordered_offsets(rng, 300), 2),
            UC.message(HS + 2 * 10 ** 8, ordered_offsets(rng, 100), 3), UC.message(HS + 2 * 10 ** 8 + GAP, ordered_offsets(rng, 180), 4)]
    late = HS + 2 * 10 ** 8 + GAP
    bounds = [HS - 10 ** 7, HS + 5 * 10 ** 7, HS + 12 * 10 ** 7, HS + 12 * 10 ** 7, HS + 19 * 10 ** 7, late + 3 * 10 ** 7, late + 8 * 10 ** 7]
    velo = [rng.uniform(-30, 30, (n, 4)).astype(np.float32) for n in (300, 512, 0, 77, 1, 257)]   # full, none, one, 256 + 1
    th = 0.3
    tf = np.array([[np.cos(th), -np.sin(th), 0.01, 0.25], [np.sin(th), np.cos(th), -0.02, -1.5], [0.015, 0.02, 1, 0.125], [0, 0, 0, 1]], np.float32)
    want_rows, want_pts = UR.replay(msgs, bounds, MAXL)
    assert list(want_rows["status"]) == [0, 0, 3, 0, 0, 0] and want_rows["n_livox"].max() <= MAXL
    hs, S = UC.stamps_of(msgs)
    k = int(want_rows[4]["end"]) - 1   # the frame across the 5 s: an in-frame offset above 2^32, truncated
    assert hs + int(S[k]) - bounds[4] > 2 ** 32 and int(S.max()) > 2 ** 32
    return dict(msgs=msgs, bounds=bounds, velo=velo, tf=tf, rows=want_rows, pts=want_pts)


def push_all(stream, msgs, wire=False):
    for tb, p in msgs:
        if wire:
            stream.push_wire(tb, UC.to_wire(p), len(p))
        else:
            stream.push(tb, p)


def fill_slots(c, n_slots, seed=5):
    """Something else in every slot first, so that what the call leaves there is the call's."""
    rng = np.random.default_rng(seed)
    for s in range(n_slots):
        c.scan_upload(s, rng.uniform(-1, 1, (40 + s, 4)).astype(np.float32), UC.message(0, np.arange(30 + s), 9)[1])
    c.synchronize()


def slots(c, first, count):
    return [c.scan_raw_download(first + i) for i in range(count)]


def assert_slots(got, want_velo, want_pts, what):
    for i, (v, l) in enumerate(got):
        assert v.shape == want_velo[i].shape and v.tobytes() == want_velo[i].tobytes(), "%s: Velodyne rows of frame %d" % (what, i)
        assert len(l) == len(want_pts[i]) and l.tobytes() == want_pts[i].tobytes(), "%s: Livox records of frame %d" % (what, i)


def test_slots_equal_the_yardstick(M, stream4):
    d = stream4
    c = context(M)
    try:
        fill_slots(c, 8)
        st = c.livox_stream(2000)
        push_all(st, d["msgs"])
        rows = c.union_assemble(st, 1, d["bounds"], d["velo"], d["tf"])
        got = slots(c, 1, 6)
        state = st.state()
        st.close()
    finally:
        c.close()
    hs, S = UC.stamps_of(d["msgs"])
    rc, plan = M.union_plan(S, 0, len(S), hs, d["bounds"], MAXL)
    assert rc == M.MML_OK
    for name in plan.dtype.names:
        assert np.array_equal(rows[name], plan[name]) and np.array_equal(rows[name], d["rows"][name]), name
    assert_slots(got, [UR.transform_velo(v, d["tf"]) for v in d["velo"]], d["pts"], "6 frames")
    assert all(np.all(l["_pad"] == 0) for _, l in got) and len(got[2][1]) == 0 and len(got[2][0]) == 0
    assert state == {"start_stamp": HS, "front": int(d["rows"][-1]["front_after"]), "tail": 800, "disorder": 0}


def test_batch_equals_singles(M, stream4):
    d = stream4
    out = []
    for batch in (True, False):
        c = context(M)
        try:
            st = c.livox_stream(2000)
            push_all(st, d["msgs"])
            if batch:
                rows = c.union_assemble(st, 0, d["bounds"], d["velo"], None)
            else:
                rows = np.concatenate([c.union_assemble(st, i, d["bounds"][i:i + 2], d["velo"][i:i + 1], None) for i in range(6)])
            out.append((rows, slots(c, 0, 6), st.state()))
            st.close()
        finally:
            c.close()
    (ra, sa, ta), (rb, sb, tb) = out
    assert ra.tobytes() == rb.tobytes() and ta == tb
    assert_slots(sa, [v for v, _ in sb], [l for _, l in sb], "batch against singles")
    assert_slots(sa, [UR.transform_velo(v, None) for v in d["velo"]], d["pts"], "batch, no transform")


def test_push_forms(M):
    rng = np.random.default_rng(3)
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, n), 20 + m) for m, n in enumerate((100, 101, 55))]   # 256 points
    bounds = [HS - 1, HS + 10 ** 9]
    c = context(M)
    try:
        got = []
        for wire in (False, True):
            st = c.livox_stream(300)
            push_all(st, msgs, wire)
            rows = c.union_assemble(st, int(wire), bounds, [np.zeros((0, 4), np.float32)])
            got.append((rows, c.scan_raw_download(int(wire))[1], st.state()))
            st.close()
    finally:
        c.close()
    want_rows, want_pts = UR.replay(msgs, bounds, MAXL)
    assert got[0][0].tobytes() == got[1][0].tobytes() == want_rows.tobytes() and got[0][2] == got[1][2]
    assert len(want_pts[0]) == 256
    assert got[0][1].tobytes() == got[1][1].tobytes() == want_pts[0].tobytes()


def test_downstream_extract_sees_the_same_slot(M, synth):
    """The assembled slot is in the state mml_scan_upload leaves: extraction of both gives the same digest."""
    lv = synth.livox_scan(3, n=240)
    lv["_pad"] = 0x5A
    velo = synth.velo_scan(3, n_az=32)   # 512 rows
    msgs, bounds = [(HS, lv)], [HS + 10 ** 6, HS + 9 * 10 ** 7]
    tf = np.eye(4, dtype=np.float32)
    tf[:3, 3] = [0.1, -0.05, 0.02]
    want_rows, want_pts = UR.replay(msgs, bounds, MAXL)
    assert want_rows[0]["status"] == UR.OK and want_rows[0]["n_livox"] > 150
    c = context(M)
    try:
        st = c.livox_stream(500)
        push_all(st, msgs)
        c.union_assemble(st, 0, bounds, [velo], tf)
        c.scan_upload(1, UR.transform_velo(velo, tf), want_pts[0])
        c.extract(0, 2)
        dig = c.slot_digest(0, 2)
        info = c.scan_info(0)
        st.close()
    finally:
        c.close()
    assert info.n_points > 0
    assert np.array_equal(dig[0], dig[1])


def test_compaction(M):
    """capacity_points = 700: eight messages of 220 points with a frame cut after each; the live part has to move to the front
    of the array more than once (modelled below by the rule the header states).  Same results as with ample capacity."""
    rng = np.random.default_rng(8)
    msgs = [UC.message(HS + m * 10 ** 8, ordered_offsets(rng, 220), 40 + m) for m in range(8)]
    bounds = [HS + m * 10 ** 8 + 2 * 10 ** 7 for m in range(9)]   # frame m lies inside what has been pushed after message m
    velo = [rng.uniform(-5, 5, (9 + m, 4)).astype(np.float32) for m in range(8)]
    ref = UR.Aligner()
    c = context(M)
    try:
        small, ample = c.livox_stream(700), c.livox_stream(4000)
        base = front = tail = moves = 0
        for m in range(8):
            if tail - base + 220 > 700:
                base, moves = front, moves + 1
            tail += 220
            ref.transform_hori_timestamp([msgs[m]])
            want_row, want_pts = ref.pub_horipoints_given_stamp(bounds[m] - 10 ** 8, bounds[m], MAXL)
            got = []
            for k, st in enumerate((small, ample)):
                st.push(*msgs[m])
                rows = c.union_assemble(st, k, [bounds[m] - 10 ** 8, bounds[m]], [velo[m]])
                got.append((rows, c.scan_raw_download(k)))
            assert tuple(got[0][0][0]) == tuple(got[1][0][0]) == want_row, m
            assert want_row[0] == UR.OK
            for rows, (v, l) in got:
                assert v.tobytes() == velo[m].tobytes() and l.tobytes() == want_pts.tobytes(), m
            front = want_row[4]
        assert moves >= 2
        assert small.state() == ample.state() == {"start_stamp": HS, "front": front, "tail": 1760, "disorder": 0}
        small.close()
        ample.close()
    finally:
        c.close()


def test_refusals(M):
    rng = np.random.default_rng(21)
    c = context(M)
    try:
        # a push over capacity changes nothing
        st = c.livox_stream(300)
        st.push(*UC.message(HS, ordered_offsets(rng, 200), 1))
        before = st.state()
        with pytest.raises(M.MmlError) as e:
            st.push(*UC.message(HS + 10 ** 8, ordered_offsets(rng, 101), 2))
        assert e.value.code == M.MML_ERR_CAPACITY and st.state() == before == {"start_stamp": HS, "front": 0, "tail": 200, "disorder": 0}
        st.push(*UC.message(HS + 10 ** 8, ordered_offsets(rng, 100), 2))   # (exactly full is accepted)
        assert st.state()["tail"] == 300
        # decreasing stamps, a slot range out of bounds: refused before anything is written
        fill_slots(c, 8)
        was = slots(c, 0, 8)
        velo = [np.ones((3, 4), np.float32)] * 2
        for first, bounds in ((0, [HS, HS + 10, HS + 5]), (7, [HS, HS + 10, HS + 20]), (-1, [HS, HS + 10, HS + 20])):
            with pytest.raises(M.MmlError) as e:
                c.union_assemble(st, first, bounds, velo)
            assert e.value.code == M.MML_ERR_INVALID, (first, bounds)
        assert st.state()["front"] == 0
        # a message whose first stamp lies below the previous tail: counted at the push, refused by the next assemble
        st.reset()
        assert st.state() == {"start_stamp": 0, "front": 0, "tail": 0, "disorder": 0}
        st.push(*UC.message(HS, ordered_offsets(rng, 120), 3))
        st.push(*UC.message(HS + 10 ** 6, ordered_offsets(rng, 100), 4))   # its own stamps ordered, its first one early
        assert st.state()["disorder"] == 1
        with pytest.raises(M.MmlError) as e:
            c.union_assemble(st, 0, [HS, HS + 10 ** 7, HS + 10 ** 9], velo)
        assert e.value.code == M.MML_ERR_STATE
        assert st.state()["front"] == 0
        now = slots(c, 0, 8)
        for (v0, l0), (v1, l1) in zip(was, now):
            assert v0.tobytes() == v1.tobytes() and l0.tobytes() == l1.tobytes()
        st.close()
        # a frame of more than 256 points: OVERFLOW, no Livox point in its slot, the frame after it as the yardstick has it
        msgs = [UC.message(HS, ordered_offsets(rng, 300), 5), UC.message(HS + 10 ** 8, ordered_offsets(rng, 150), 6)]
        bounds = [HS, HS + 95 * 10 ** 6, HS + 2 * 10 ** 8]
        want_rows, want_pts = UR.replay(msgs, bounds, MAXL)
        assert list(want_rows["status"]) == [UR.OVERFLOW, UR.OK] and want_rows[0]["n_livox"] > MAXL
        st = c.livox_stream(600)
        push_all(st, msgs)
        rows = c.union_assemble(st, 2, bounds, velo)
        assert rows.tobytes() == want_rows.tobytes()
        got = slots(c, 2, 2)
        assert len(got[0][1]) == 0 and got[0][0].tobytes() == velo[0].tobytes()
        assert got[1][1].tobytes() == want_pts[1].tobytes()
        st.close()
    finally:
        c.close()


@pytest.mark.parametrize("count", [1, 6])
def test_one_plan_and_one_gather_launch_per_call(M, stream4, count):
    d = stream4
    c = context(M)
    try:
        st = c.livox_stream(2000)
        push_all(st, d["msgs"])
        c.synchronize()
        c.profile_enable(True)
        c.profile_reset()
        rows = c.union_assemble(st, 0, d["bounds"][:count + 1], d["velo"][:count], d["tf"])
        prof = c.profile_get()
        st.close()
    finally:
        c.close()
    assert len(rows) == count
    assert prof["union_plan"][1] == 1 and prof["union_gather"][1] == 1
