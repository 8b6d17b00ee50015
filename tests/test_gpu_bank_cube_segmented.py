"""mml_map_bank_global_increment_segmented / mml_map_bank_global_append_segmented (include/mmloam_hip.h, "map banks"): n banks'
cube stores grown by ONE chain of launches.

There is ONE chain (csrc/map_global.hip): the loop calls (mml_map_bank_global_increment / _append) and the context's own store
(mml_map_global_increment / _append) run it with n = 1, so "segmented equals loop" compares the chain with itself.  It is therefore
anchored outside the code under test, twice.  tests/golden/cube_increment_parent.npz (make_cube_increment_parent.py) holds what the
loop forms and the own store of the commit before the merge -- a separate one-store implementation -- returned on a MI355X for the
run functions below: sizes, centres and SHA-256 digests of every downloaded byte string and of the association records.  Both call
forms and both chunk budgets must reproduce it exactly.  The CPU oracle's CubeStore is held against the same histories per cube,
and the claims a case rests on (a cube at exactly 300 points is kept, one at 301 is filtered, a pose move drops one layer and keeps
another, "gone" empties a store) are asserted on the oracle alone before the device is compared.  Every comparison is on bytes, with
no tolerance -- sizes, live stores with their cube tags and the order inside every cube, centres, and (through the factor records
of bound slots) the match copies.  A refused call, of either form or on the own store, leaves its store exactly as it was.

STEPS' "far" pose: on the oracle it moves the centre by two layers and drops NO point (1028 corner points before and after in bank
0's order) -- every stored tag changes, none dies.  The test asserts that move; the layer that leaves the grid is covered by
test_move_drops_one_layer on a cloud built for it."""
import hashlib
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, perturbed, shifted
from test_gpu_bank_cube import (BIND, MM, SH, STEPS, _alone, _banked_ctx, _load_features, _poses, _records, _sequence_inputs,
                                _step_inputs, maps)  # noqa: F401  (maps: a fixture)

pytestmark = pytest.mark.gpu

E3 = np.zeros((0, 3), np.float32)
ORDER = {0: STEPS, 2: STEPS[3:] + STEPS[:3]}
FEED = {0: 0, 2: 1, 3: 4}                  # the slot whose stacks feed the bank
BANKS = (0, 1, 2, 3)


def digest(name, obj, out=None):
    """The fixture form of a run: its nested tuples / lists / dicts flattened to path -> SHA-256 of a byte string (32 uint8) or an
    integer array."""
    out = {} if out is None else out
    if isinstance(obj, bytes):
        out[name] = np.frombuffer(hashlib.sha256(obj).digest(), np.uint8)
    elif isinstance(obj, dict):
        for k in obj:
            digest("%s/%s" % (name, ".".join(str(i) for i in k) if isinstance(k, tuple) else k), obj[k], out)
    elif isinstance(obj, (list, tuple)) and any(isinstance(x, (bytes, dict, list, tuple)) for x in obj):
        for i, x in enumerate(obj):
            digest("%s/%d" % (name, i), x, out)
    else:
        a = np.asarray(obj)
        assert a.size == 0 or a.dtype.kind in "iub", (name, a.dtype)
        out[name] = a.astype(np.int64)
    return out


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(GOLDEN, "cube_increment_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def assert_parent(parent, name, run):
    """Every entry of the run equals the fixture's, and the fixture has no entry under `name` that the run lacks."""
    got = digest(name, run)
    assert sorted(got) == sorted(k for k in parent if k == name or k.startswith(name + "/")), name
    for k, v in got.items():
        w = parent[k]
        assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), "%s differs from the parent commit's one-store chain" % k


def _world(f, T):
    x, y, z = (f[:, i].astype(np.float64) for i in range(3))
    return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32) for r in range(3)], 1)


def _dl(c, banks):
    return {(b, k): tuple(a.tobytes() for a in c.bank_global_download(b, k)) for b in banks for k in (0, 1)}


def _history_inputs(scene, step):
    """bank -> (T of the increment, [(corner, surf, T) of every append before it]).  Banks 0 and 2: the step list in two orders;
    bank 1: in every increment, nothing pending, nothing stored (the empty segment); bank 3: appends from step 4 on, one per step."""
    inp = {b: _step_inputs(scene, step, *ORDER[b][step]) for b in (0, 2)}
    inp[1] = (np.eye(4), [])
    if step >= 4:
        fr = scene["frames"][step % 4]
        T3 = shifted(perturbed(fr["T_gt"], dt=(0.02 * step, 0.01, 0.0)), SH)
        inp[3] = (T3, [(fr["corner"], fr["surf"], T3)])
    return inp


def _run_history(M, scene, segmented, budget=None):
    """The history on one context; what every round left: the sizes returned, every bank's downloads, the records of the two
    bound slots at steps 2, 5 and 7."""
    kw = dict(segmented=True) if segmented else {}
    c = M.Context(max_scans=5, max_map_points=MM)
    rec = []
    loc = (scene["corner_map"] + SH.astype(np.float32), scene["surf_map"] + SH.astype(np.float32))
    try:
        c.map_banks(4)
        if budget is not None:
            c.bank_global_increment_budget(budget)
        for b in (0, 2):
            for kind in (0, 1):
                c.bank_set_local(b, kind, loc[kind])
        c.bind_banks(2, [0, 2])
        frq = scene["frames"][1]
        Tq = shifted(perturbed(frq["T_gt"]), SH)
        for s in (2, 3):
            c.features_upload(s, 0, frq["corner"])
            c.features_upload(s, 1, frq["surf"])
        for step in range(len(STEPS)):
            inp = _history_inputs(scene, step)
            for r in range(2):                            # the r-th append of every bank that has one: ONE call
                who = [b for b in (0, 2, 3) if b in inp and len(inp[b][1]) > r]
                for b in who:
                    c.features_upload(FEED[b], 0, inp[b][1][r][0])
                    c.features_upload(FEED[b], 1, inp[b][1][r][1])
                if who:
                    c.bank_global_append(who, [FEED[b] for b in who], np.stack([inp[b][1][r][2] for b in who]), **kw)
            call = [2, 1, 0] + ([3] if 3 in inp else [])
            nc, ns = c.bank_global_increment(call, np.stack([inp[b][0] for b in call]), **kw)
            out = dict(sizes=(call, nc.tolist(), ns.tolist()), dl=_dl(c, BANKS))
            if step in (2, 5, 7):
                c.associate(2, 2, np.stack([Tq, Tq]), 1.0)
                out["assoc"] = (_records(c, 2), _records(c, 3))
            rec.append(out)
    finally:
        c.close()
    return rec


@pytest.fixture(scope="module")
def loop_record(M, scene):
    return _run_history(M, scene, False)


@pytest.fixture(scope="module")
def seg_record(M, scene):
    return _run_history(M, scene, True)


def _per_cube(xyz, cube):
    order = np.argsort(cube, kind="stable")
    return xyz[order], cube[order]


def _same_as_oracle(dl, cs, what):
    for kind in (0, 1):
        gx = np.frombuffer(dl[kind][0], np.float32).reshape(-1, 3)
        gc = np.frombuffer(dl[kind][1], np.int32)
        gcen = np.frombuffer(dl[kind][2], np.int32)
        ox, oc, ocen = cs.get(kind)
        assert len(gx) == len(ox) and np.array_equal(gcen, ocen), (what, kind)
        gxs, gcs = _per_cube(gx, gc)
        assert np.array_equal(gcs, oc) and gxs.tobytes() == ox.tobytes(), (what, kind)


def test_history_equals_loop_and_oracle(O, scene, parent, loop_record, seg_record):
    """Test 1."""
    assert len(seg_record) == len(loop_record) == len(STEPS)
    assert_parent(parent, "history", loop_record)
    assert_parent(parent, "history", seg_record)
    used = False
    for step, (got, want) in enumerate(zip(seg_record, loop_record)):
        assert got["sizes"] == want["sizes"], step
        for key in want["dl"]:
            assert got["dl"][key] == want["dl"][key], (step, key)
        assert ("assoc" in got) == (step in (2, 5, 7))
        if "assoc" in got:
            assert got["assoc"] == want["assoc"], step                   # the match copy lags one increment, as the loop's
            used = used or got["assoc"][0] != got["assoc"][1]
        assert all(len(got["dl"][(1, k)][0]) == 0 for k in (0, 1))       # bank 1: the empty segment
        if step < 4:
            assert all(len(got["dl"][(3, k)][0]) == 0 for k in (0, 1))
    assert used, "the two banks' match copies never made a difference"
    assert len(seg_record[4]["dl"][(3, 1)][0]) > 0                       # bank 3's first increment (n0 = 0) stored its scan
    # the same history through the oracle, per bank and cube with order
    for b in (0, 2, 3):
        cs = O.CubeStore()
        before = ((0, 0), None)
        for step in range(len(STEPS)):
            inp = _history_inputs(scene, step)
            if b not in inp:
                continue
            T, feats = inp[b]
            cs.increment(np.concatenate([E3] + [_world(cf, Tr) for cf, sf, Tr in feats]),
                         np.concatenate([E3] + [_world(sf, Tr) for cf, sf, Tr in feats]), T)
            cen_before = before[1]
            now = (tuple(len(cs.get(k)[0]) for k in (0, 1)), cs.get(0)[2].copy())
            if b != 3 and ORDER[b][step][0] == "far":                    # the layers shift under a store that holds points
                assert min(before[0]) > 0 and now[0] == before[0] and not np.array_equal(now[1], cen_before)
            if b != 3 and ORDER[b][step][0] == "gone":                   # every layer leaves the grid
                assert min(before[0]) > 0 and now[0] == (0, 0)
            before = now
            _same_as_oracle({k: seg_record[step]["dl"][(b, k)] for k in (0, 1)}, cs, (b, step))


def _lattice(first, count, origin, pitch=0.1, row=20):
    """Points first .. first + count - 1 of a planar lattice at `pitch` metres, `row` points per row: distinct, one cube."""
    k = np.arange(first, first + count)
    return (np.asarray(origin, np.float32) + np.stack([pitch * (k % row), pitch * (k // row), 0 * k], 1).astype(np.float32)).astype(np.float32)


EDGE = {0: (150, 150), 1: (150, 151), 2: (128, 128), 3: (128, 129)}   # bank -> (stored, new): 300, 301, and 256 / 257 rows
CORNER_AT, SURF_AT = (5.0, 5.0, 1.0), (5.0, 55.0, 1.0)                 # well inside one 50 m cube each (two different cubes)


def _edge_clouds(b, part):
    first, count = (0, EDGE[b][0]) if part == 0 else (EDGE[b][0], EDGE[b][1])
    return _lattice(first, count, CORNER_AT), _lattice(first, count, SURF_AT)


def _edge_run(M, banks, segmented):
    kw = dict(segmented=True) if segmented else {}
    I = np.eye(4)
    c = M.Context(max_scans=4, max_map_points=MM)
    try:
        c.map_banks(4)
        sizes = []
        for part in (0, 1):
            for i, b in enumerate(banks):
                cf, sf = _edge_clouds(b, part)
                c.features_upload(i, 0, cf)
                c.features_upload(i, 1, sf)
            c.bank_global_append(banks, list(range(len(banks))), np.stack([I] * len(banks)), **kw)
            nc, ns = c.bank_global_increment(banks, np.stack([I] * len(banks)), **kw)   # the second: all four edges in ONE call
            sizes.append((nc.tolist(), ns.tolist()))
        return sizes, _dl(c, banks)
    finally:
        c.close()


def _edge_oracle(O):
    stores = {}
    for b in EDGE:
        cs = O.CubeStore()
        for part in (0, 1):
            cs.increment(*_edge_clouds(b, part), np.eye(4))
        stores[b] = cs
    for k in (0, 1):                                       # on the oracle alone: 300 is kept whole, 301 is filtered
        assert len(stores[0].get(k)[0]) == 300 and len(stores[1].get(k)[0]) < 301
        assert len(stores[2].get(k)[0]) == 256 and len(stores[3].get(k)[0]) == 257
        assert len(np.unique(stores[1].get(k)[1])) == 1    # one cube
    return stores


def test_the_300_point_edge_and_block_edges(M, O, parent):
    """Test 2."""
    stores = _edge_oracle(O)
    banks = [0, 1, 2, 3]
    seg, loop = _edge_run(M, banks, True), _edge_run(M, banks, False)
    assert seg == loop
    assert_parent(parent, "edge", loop)
    for b in banks:
        _same_as_oracle({k: seg[1][(b, k)] for k in (0, 1)}, stores[b], b)
    # n = 1: the 301 bank alone equals mml_map_global_increment on a context of its own
    one = _edge_run(M, [1], True)
    assert one[1] == {(1, k): seg[1][(1, k)] for k in (0, 1)}
    r = M.Context(max_scans=1, max_map_points=MM)
    try:
        for part in (0, 1):
            cf, sf = _edge_clouds(1, part)
            r.features_upload(0, 0, cf)
            r.features_upload(0, 1, sf)
            r.map_global_append(0, np.eye(4))
            want = r.map_global_increment(np.eye(4))
            assert want == (one[0][part][0][0], one[0][part][1][0])
        for k in (0, 1):
            assert tuple(a.tobytes() for a in r.map_global_download(k)) == one[1][(1, k)]
    finally:
        r.close()


def _move_inputs():
    near, far = _lattice(0, 200, (1.0, 2.0, 0.5)), _lattice(0, 180, (-400.0, 2.0, 0.5))
    few = _lattice(0, 40, (1.0, 60.0, 0.5))
    Ta, Tb = np.eye(4), np.eye(4)
    Ta[0, 3], Tb[0, 3] = -200.0, 300.0
    return near, far, few, Ta, Tb


def _move_run(M, segmented):
    kw = dict(segmented=True) if segmented else {}
    near, far, few, Ta, Tb = _move_inputs()
    c = M.Context(max_scans=2, max_map_points=MM)
    try:
        c.map_banks(2)
        c.features_upload(0, 0, near)
        c.features_upload(0, 1, few)
        c.features_upload(1, 0, far)
        c.features_upload(1, 1, E3)
        c.bank_global_append([1], [0], np.eye(4)[None], **kw)
        c.bank_global_append([1], [1], np.eye(4)[None], **kw)
        s1 = c.bank_global_increment([0, 1], np.stack([np.eye(4), Ta]), **kw)
        s2 = c.bank_global_increment([1, 0], np.stack([Tb, Tb]), **kw)
        return (s1[0].tolist(), s1[1].tolist(), s2[0].tolist(), s2[1].tolist(), _dl(c, (0, 1)))
    finally:
        c.close()


def test_move_drops_one_layer(M, O, parent):
    """MapMove under a store of two layers: the pose at x = -200 m shifts the grid up, a cloud at x = -400 m lands in layer 4; the
    pose at x = +300 m shifts it down by six: layer 4 leaves the grid, the cloud around the origin (layer 12 -> 6) stays."""
    near, far, few, Ta, Tb = _move_inputs()
    cs = O.CubeStore()
    cs.increment(np.concatenate([near, far]), few, Ta)
    n1 = len(cs.get(0)[0])
    cs.increment(E3, E3, Tb)
    assert n1 == 380 and len(cs.get(0)[0]) == 200 and len(cs.get(1)[0]) == 40          # on the oracle: one layer of two is gone
    out = [_move_run(M, True), _move_run(M, False)]
    assert out[0] == out[1] and out[0][2] == [200, 0]
    assert_parent(parent, "move", out[1])
    _same_as_oracle({k: out[0][4][(1, k)] for k in (0, 1)}, cs, "after the move")


def _own_dl(c):
    return {k: tuple(a.tobytes() for a in c.map_global_download(k)) for k in (0, 1)}


ONE_POINT = np.array([[3.0, -2.0, 0.5]], np.float32)
# MapMove ALWAYS ends with the sensor's cube in height layer 2 (Map_Manager.cpp:491 shifts up to 8, :536 down below 11 - 8 = 3), so
# at the identity pose the centre goes from (10, 5, 10) to (10, 2, 10).  The pose whose centre ends where it started lies three
# layers down: z = -140 m -> six shifts up, six down, twelve in all.
BELOW = np.eye(4)
BELOW[2, 3] = -140.0


def _own_run(M, scene):
    """The context's OWN store through map_global_append / map_global_increment.  "edge<b>": the four EDGE cases, a context each.
    "empty": an increment with nothing stored and nothing pending at the pose BELOW, between two associations of a slot against
    the local maps; "one": then one pending corner point and no surf point, at the identity pose."""
    out = {}
    for b in EDGE:
        c = M.Context(max_scans=1, max_map_points=MM)
        try:
            sizes = []
            for part in (0, 1):
                cf, sf = _edge_clouds(b, part)
                c.features_upload(0, 0, cf)
                c.features_upload(0, 1, sf)
                c.map_global_append(0, np.eye(4))
                sizes.append(c.map_global_increment(np.eye(4)))
            out["edge%d" % b] = (sizes, _own_dl(c))
        finally:
            c.close()
    c = M.Context(max_scans=2, max_map_points=MM)
    try:
        frq = scene["frames"][1]
        Tq = shifted(perturbed(frq["T_gt"]), SH)
        for kind, name in ((0, "corner"), (1, "surf")):
            c.map_set_local(kind, scene[name + "_map"] + SH.astype(np.float32))
            c.features_upload(1, kind, frq[name])
        c.associate(1, 1, Tq[None], 1.0)
        before = _records(c, 1)
        sizes = c.map_global_increment(BELOW)
        c.associate(1, 1, Tq[None], 1.0)
        out["empty"] = (sizes, _own_dl(c), before, _records(c, 1))
        c.features_upload(0, 0, ONE_POINT)
        c.features_upload(0, 1, E3)
        c.map_global_append(0, np.eye(4))
        out["one"] = (c.map_global_increment(np.eye(4)), _own_dl(c))
    finally:
        c.close()
    return out


def test_own_store_through_the_chain(M, O, scene, parent):
    """The own store is the chain with n = 1 and no bank: the 300 / 301 and 256 / 257 edges, the empty increment, one point."""
    stores = _edge_oracle(O)
    own = _own_run(M, scene)
    assert_parent(parent, "own", own)
    for b in EDGE:
        sizes, dl = own["edge%d" % b]
        assert sizes[0] == (EDGE[b][0], EDGE[b][0])
        assert sizes[1] == tuple(len(stores[b].get(k)[0]) for k in (0, 1))
        _same_as_oracle(dl, stores[b], b)
    sizes, dl, before, after = own["empty"]
    assert sizes == (0, 0) and all(len(dl[k][0]) == 0 and len(dl[k][1]) == 0 for k in (0, 1))
    assert all(np.frombuffer(dl[k][2], np.int32).tolist() == [10, 5, 10] for k in (0, 1))
    assert after == before and len(before[0]) > 0 and len(before[2]) > 0     # the local maps are matched as before the call
    sizes, dl = own["one"]
    cs = O.CubeStore()
    cs.increment(E3, E3, BELOW)
    assert cs.get(0)[2].tolist() == [10, 5, 10]                              # on the oracle: twelve shifts, the centre where it was
    cs.increment(ONE_POINT, E3, np.eye(4))
    assert sizes == (1, 0) and dl[0][0] == ONE_POINT.tobytes() and cs.get(0)[2].tolist() == [10, 2, 10]
    _same_as_oracle(dl, cs, "one point")


@pytest.mark.parametrize("budget", [1, 3000])
def test_chunks_give_the_same_bytes(M, scene, parent, seg_record, budget):
    """Test 3: every bank a chunk of its own (budget 1: any bank with points is over it); a budget the first round's banks share
    (2 x 1274 + 16 points or so) and later rounds' do not; against the default's record."""
    pending = sum(len(cf) + len(sf) for T, feats in _history_inputs(scene, 0).values() for cf, sf, Tr in feats)
    assert 0 < pending <= 3000 < sum(seg_record[5]["sizes"][1]) + sum(seg_record[5]["sizes"][2])   # (stored alone, before round 6)
    got = _run_history(M, scene, True, budget=budget)
    assert got == seg_record
    assert_parent(parent, "history", got)


def _state(c, banks, n, slot):
    return (c.slot_digest(0, n).tobytes(), c.slot_banks(0, n).tobytes(), _dl(c, banks))


def _refused(M, c, code, call, state):
    before = state()
    with pytest.raises(M.MmlError) as e:
        call()
    assert e.value.code == code and len(M.lib().mml_last_error(c._h)) > 0
    assert state() == before


def test_refusals_change_nothing(M, cube_scene, maps):
    """Test 4, on a context with maps, bindings and a history: argument refusals and the pose outside the grid."""
    n = 6
    c, twin = _banked_ctx(M, maps, n, BIND), _banked_ctx(M, maps, n, BIND)
    try:
        T = _poses(cube_scene, n)
        for x, kw in ((c, dict(segmented=True)), (twin, {})):           # the accepted history, on both
            _load_features(x, cube_scene, n)
            x.bank_global_append([0, 2], [0, 1], T[:2], **kw)
            x.bank_global_increment([0, 2], T[:2], **kw)
            x.bank_global_append([0, 1], [2, 3], T[2:4], **kw)          # (pending points too)

        def state():
            c.associate(0, n, T, 25.0)                                  # a fresh association: the match copies are what they were
            return _state(c, (0, 1, 2), n, 2) + (_records(c, 2), _records(c, 5))

        T2, T3 = T[:2], T[:3]
        far = T3.copy()
        far[1, 0, 3] = 5000.0                                           # 64 or more layer shifts, the SECOND bank of three
        S = dict(segmented=True)
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_append([1, 1], [0, 1], T2, **S), state)      # a bank twice
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_increment([2, 2], T2, **S), state)
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_append([0, 3], [0, 1], T2, **S), state)      # a bank out of range
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_increment([0, -1], T2, **S), state)
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_append([0, 1], [0, n], T2, **S), state)      # a slot out of range
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_increment([], np.zeros((0, 16)), **S), state)  # no banks
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.bank_global_increment([0, 1, 2], far, **S), state)       # the pose at x = 5000 m
        # the next valid call equals the loop's on the twin
        got = c.bank_global_increment([2, 0, 1], T3, **S)
        want = twin.bank_global_increment([2, 0, 1], T3)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
        assert _dl(c, (0, 1, 2)) == _dl(twin, (0, 1, 2))
        c.associate(0, n, T, 25.0)
        twin.associate(0, n, T, 25.0)
        assert all(_records(c, s) == _records(twin, s) for s in range(n))
    finally:
        c.close()
        twin.close()


def test_refusals_without_banks_and_without_a_stack(M, synth, cube_scene):
    """Test 4, the two STATE cases: a context without banks; an append with a slot whose down-sampling overflowed, in the MIDDLE of
    the list -- the banks before and after it are not fed either."""
    c = M.Context(max_scans=3, max_map_points=MM, max_features=64)
    try:
        T = _poses(cube_scene, 3)
        S = dict(segmented=True)
        for call in (lambda: c.bank_global_increment([0], T[:1], **S), lambda: c.bank_global_append([0], [0], T[:1], **S)):
            with pytest.raises(M.MmlError) as e:
                call()
            assert e.value.code == M.MML_ERR_STATE and len(M.lib().mml_last_error(c._h)) > 0
        c.map_banks(3)
        for s in (0, 2):
            c.features_upload(s, 0, cube_scene["frames"][0]["corner"][:50])
            c.features_upload(s, 1, cube_scene["frames"][0]["surf"][:60])
        c.scan_upload(1, synth.velo_scan(3, n_az=450), synth.livox_scan(3, n=6000))
        c.extract(1, 1)
        c.downsample(1, 1)                                              # far more than 64 features: the overflow mark, not a stack
        with pytest.raises(M.MmlError):
            c.features_count(1, 1)
        c.bank_global_append([1], [0], T[:1], **S)                      # bank 1 holds pending points already
        c.bind_banks(0, [2])
        _refused(M, c, M.MML_ERR_STATE, lambda: c.bank_global_append([0, 1, 2], [0, 1, 2], T, **S), lambda: _state(c, (0, 1, 2), 3, 0))
        nc, ns = c.bank_global_increment([0, 1, 2], T, **S)
        assert nc.tolist() == [0, 50, 0] and ns.tolist() == [0, 60, 0]  # what was pending before the refused call, and nothing else
    finally:
        c.close()


CAP_MM = 1 << 14
BIG = [_lattice(8000 * j, 8000, (-20.0, -20.0, 0.5), pitch=0.05, row=400) for j in range(3)]   # 24000 points, one cube, > CAP_MM


def _capacity_ctx(M, scene, kw):
    """max_map_points = 2^14; banks 0 and 2: two scans stored, a third pending; slot 3 bound to bank 0."""
    loc = (scene["corner_map"][:8000] + SH.astype(np.float32), scene["surf_map"][:8000] + SH.astype(np.float32))
    fr = scene["frames"]
    x = M.Context(max_scans=4, max_map_points=CAP_MM)
    x.map_banks(3)
    for b in (0, 2):
        for kind in (0, 1):
            x.bank_set_local(b, kind, loc[kind])
    x.bind_banks(3, [0])
    x.features_upload(3, 0, fr[1]["corner"])
    x.features_upload(3, 1, fr[1]["surf"])
    for rnd in range(2):
        for i, b in enumerate((0, 2)):
            x.features_upload(i, 0, fr[rnd + i]["corner"])
            x.features_upload(i, 1, fr[rnd + i]["surf"])
        Tr = np.stack([shifted(perturbed(fr[rnd + i]["T_gt"]), SH) for i in range(2)])
        x.bank_global_append([0, 2], [0, 1], Tr, **kw)
        x.bank_global_increment([0, 2], Tr, **kw)
    x.bank_global_append([0, 2], [0, 1], Tr, **kw)
    return x


def _overfill_bank_1(c, kw):
    c.features_upload(2, 1, _lattice(0, 10, (3.0, 3.0, 0.5)))
    for j in range(3):                                                  # bank 1: 24000 pending corner points
        c.features_upload(2, 0, BIG[j])
        c.bank_global_append([1], [2], np.eye(4)[None], **kw)


def test_capacity_refusal_leaves_all_banks(M, scene):
    """Test 4, the case the loop cannot pass: max_map_points so small that the SECOND bank of a three-bank call overflows.  The
    poses move the grid, so the loop would have shifted the first bank's tags and moved its centre; here the first and the third
    bank, and the second, are exactly as before."""
    fr = scene["frames"]
    Tq = shifted(perturbed(fr[1]["T_gt"]), SH)
    S = dict(segmented=True)
    c, twin = _capacity_ctx(M, scene, S), _capacity_ctx(M, scene, {})
    try:
        _overfill_bank_1(c, S)
        Tm = np.stack([np.eye(4)] * 3)
        Tm[:, 0, 3] = 260.0                                             # MapMove: three layers down for every bank

        def state():
            c.associate(3, 1, Tq[None], 1.0)
            return _state(c, (0, 1, 2), 4, 3) + (_records(c, 3),)

        _refused(M, c, M.MML_ERR_CAPACITY, lambda: c.bank_global_increment([0, 1, 2], Tm, **S), state)
        # bank 1's pending points are still there: alone it is refused again; the others' next call equals the loop's on the twin
        _refused(M, c, M.MML_ERR_CAPACITY, lambda: c.bank_global_increment([1], Tm[:1], **S), state)
        got = c.bank_global_increment([0, 2], Tm[:2], **S)
        want = twin.bank_global_increment([0, 2], Tm[:2])
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and min(got[1]) > 0
        assert _dl(c, (0, 2)) == _dl(twin, (0, 2))
        assert np.frombuffer(_dl(c, (0,))[(0, 0)][2], np.int32)[2] == 7                              # the centre moved with the accepted call
        c.associate(3, 1, Tq[None], 1.0)
        twin.associate(3, 1, Tq[None], 1.0)
        assert _records(c, 3) == _records(twin, 3)
    finally:
        c.close()
        twin.close()


def test_loop_refusal_leaves_the_refused_bank_and_those_after_it(M, scene):
    """The loop form of the call above: bank 0 is incremented (as the twin's [0] call does it), bank 1 is refused and is, with
    bank 2 behind it, byte for byte as before -- stores, tags, centres, and through bank 0's slot the match copy of the twin."""
    c, twin = _capacity_ctx(M, scene, {}), _capacity_ctx(M, scene, {})
    try:
        _overfill_bank_1(c, {})
        Tm = np.stack([np.eye(4)] * 3)
        Tm[:, 0, 3] = 260.0
        Tq = shifted(perturbed(scene["frames"][1]["T_gt"]), SH)
        before = _dl(c, (1, 2))
        with pytest.raises(M.MmlError) as e:
            c.bank_global_increment([0, 1, 2], Tm)
        assert e.value.code == M.MML_ERR_CAPACITY and len(M.lib().mml_last_error(c._h)) > 0
        assert _dl(c, (1, 2)) == before
        assert np.frombuffer(before[(2, 0)][2], np.int32)[2] == 10                     # (not moved: the accepted call moves it to 7)
        twin.bank_global_increment([0], Tm[:1])
        assert _dl(c, (0,)) == _dl(twin, (0,))
        for x in (c, twin):
            x.associate(3, 1, Tq[None], 1.0)
        assert _records(c, 3) == _records(twin, 3)
        # bank 1's pending points are still there (refused again), bank 2's too: its next increment equals the twin's
        with pytest.raises(M.MmlError) as e:
            c.bank_global_increment([1], Tm[:1])
        assert e.value.code == M.MML_ERR_CAPACITY and _dl(c, (1, 2)) == before
        got, want = c.bank_global_increment([2], Tm[:1]), twin.bank_global_increment([2], Tm[:1])
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and min(got[1]) > 0
        assert _dl(c, (2,)) == _dl(twin, (2,))
    finally:
        c.close()
        twin.close()


def _own_history_ctx(M, scene):
    """A context of its own with max_map_points = 2^14: local maps, a query stack in slot 1, two scans stored, a third pending."""
    fr = scene["frames"]
    c = M.Context(max_scans=2, max_map_points=CAP_MM)
    for kind, name in ((0, "corner"), (1, "surf")):
        c.map_set_local(kind, scene[name + "_map"][:8000] + SH.astype(np.float32))
        c.features_upload(1, kind, fr[1][name])
    for rnd in range(3):
        c.features_upload(0, 0, fr[rnd]["corner"])
        c.features_upload(0, 1, fr[rnd]["surf"])
        Tr = shifted(perturbed(fr[rnd]["T_gt"]), SH)
        c.map_global_append(0, Tr)
        if rnd < 2:
            c.map_global_increment(Tr)
    return c


def test_own_store_refusals_change_nothing(M, scene):
    """mml_map_global_increment refused -- the pose that needs more than 64 layer shifts, the store over max_map_points, both with
    a pose that moves the grid -- leaves downloads, centre, match copy (a fresh association) and pending clouds as they were."""
    c, twin = _own_history_ctx(M, scene), _own_history_ctx(M, scene)
    try:
        Tq = shifted(perturbed(scene["frames"][1]["T_gt"]), SH)
        Tm = np.eye(4)
        Tm[0, 3] = 260.0
        far = np.eye(4)
        far[0, 3] = 5000.0

        def state():
            c.associate(1, 1, Tq[None], 1.0)
            return _own_dl(c), _records(c, 1)

        assert all(len(state()[0][k][0]) > 0 for k in (0, 1)) and len(state()[1][2]) > 0
        _refused(M, c, M.MML_ERR_INVALID, lambda: c.map_global_increment(far), state)
        # the pending clouds too: the next accepted call equals the twin's, which saw no refusal
        assert c.map_global_increment(Tm) == twin.map_global_increment(Tm)
        assert _own_dl(c) == _own_dl(twin) and np.frombuffer(_own_dl(c)[0][2], np.int32)[2] == 7
        twin.associate(1, 1, Tq[None], 1.0)
        assert state()[1] == _records(twin, 1)
        c.features_upload(0, 1, _lattice(0, 10, (3.0, 3.0, 0.5)))
        for j in range(3):                                              # 24000 pending corner points
            c.features_upload(0, 0, BIG[j])
            c.map_global_append(0, np.eye(4))
        back = np.eye(4)
        back[0, 3] = 10.0                                               # (moves the grid again: three layers up)
        _refused(M, c, M.MML_ERR_CAPACITY, lambda: c.map_global_increment(back), state)
        _refused(M, c, M.MML_ERR_CAPACITY, lambda: c.map_global_increment(back), state)   # (the pending points are still there)
    finally:
        c.close()
        twin.close()


@pytest.mark.parametrize("bad", [0, 1])
def test_own_append_without_a_stack_changes_nothing(M, synth, cube_scene, bad):
    """mml_map_global_append of a slot whose stack of kind `bad` carries the overflow mark while the other kind's is valid: refused
    before either pending cloud grows."""
    c = M.Context(max_scans=2, max_map_points=MM, max_features=64)
    try:
        T = _poses(cube_scene, 2)
        c.features_upload(0, 0, cube_scene["frames"][0]["corner"][:50])
        c.features_upload(0, 1, cube_scene["frames"][0]["surf"][:60])
        c.map_global_append(0, T[0])                                    # pending: 50 corner, 60 surf points
        c.scan_upload(1, synth.velo_scan(3, n_az=450), synth.livox_scan(3, n=6000))
        c.extract(1, 1)
        c.downsample(1, 1)                                              # far more than 64 features of either kind
        c.features_upload(1, 1 - bad, cube_scene["frames"][1][("corner", "surf")[1 - bad]][:40])
        assert c.features_count(1, 1 - bad) == 40
        with pytest.raises(M.MmlError):
            c.features_count(1, bad)                                    # the overflow mark, not a stack
        _refused(M, c, M.MML_ERR_STATE, lambda: c.map_global_append(1, T[1]), lambda: _own_dl(c))
        assert c.map_global_increment(T[0]) == (50, 60)                 # what was pending before the refused call, and nothing else
    finally:
        c.close()


@pytest.fixture(scope="module")
def replay(M, synth):
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    inputs = [_sequence_inputs(synth, w, 7) for w in range(3)]
    return inputs, [_alone(M, odometry, inputs[w], True) for w in range(3)]


@pytest.mark.parametrize("increment", ["loop", "segmented"])
def test_lockstep_replay_segmented(M, parent, replay, increment):
    """Test 5: test_lockstep_replay_with_cube_schedule's three sequences x seven rounds with both cube calls of a round through the
    segmented entry points -- and, with increment="segmented", the local-map increment too: a round's whole upkeep in two chains."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    inputs, alone = replay
    assert_parent(parent, "alone", alone)                  # the own store through the chain, against the one-store chain's record
    W, rounds = 3, 7
    c = M.Context(max_scans=W, max_map_points=MM)
    try:
        bat = odometry.BatchLidarOdometry(c, W, lidar_mode=2, global_map=True, global_increment="segmented", increment=increment)
        for i in range(rounds):
            for w in range(W):
                c.scan_upload(w, inputs[w][i][0], inputs[w][i][1])
            c.extract(0, W)
            c.undistort(0, W, np.stack([inputs[w][i][2].reshape(9) for w in range(W)]), np.stack([inputs[w][i][3] for w in range(W)]))
            P, Q, grew = bat.estimate_lidar_pose(list(range(W)), np.stack([inputs[w][i][4] for w in range(W)]),
                                                 np.stack([inputs[w][i][5] for w in range(W)]))
            for w in range(W):
                assert (P[w].tobytes(), Q[w].tobytes(), grew[w]) == alone[w][0][i], "sequence %d, scan %d" % (w, i)
                assert (bat.seq[w].n_corner_global, bat.seq[w].n_surf_global) == alone[w][1][i]
        assert bat.key_scans == [a[2] for a in alone]
        assert [st.last_T.tobytes() for st in bat.seq] == [a[3] for a in alone]
    finally:
        c.close()
