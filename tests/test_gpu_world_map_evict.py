"""GPU suite for mml_world_map_evict against tests/world_map_evict_ref.py.  Maps are built with world_map_import from hand-made
rows (distinct random indices, random sums, counts 1 .. 9, random moments on a surfel map) with capacity_voxels equal to the
voxels held, so that the table is as full as it may be and probe chains are long; every comparison is bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import world_map_evict_ref as E
from test_gpu_world_map import I4, _sequence_inputs, records, upload
from test_gpu_world_map_score import LEAF as ROOM_LEAF
from test_gpu_world_map_score import equal, scan, scene_points, sensor_frame, shift, stack

pytestmark = pytest.mark.gpu
LEAF = 0.25
SPAN = 12            # indices in [-SPAN, SPAN): 13 824 voxels to draw from
BIG = ((-SPAN,) * 3, (SPAN,) * 3)
HALF = ((-SPAN,) * 3, (0, SPAN, SPAN))          # i < 0
EMPTY = ((0, 0, 0), (0, 0, 0))


def make_rows(rng, n, surfels, span=SPAN):
    """n voxels as world_map_export would hand them out: ascending packed key (k, then j, then i)"""
    flat = rng.choice((2 * span) ** 3, n, replace=False)
    ijk = np.stack([flat % (2 * span), flat // (2 * span) % (2 * span), flat // (2 * span) ** 2], 1).astype(np.int32) - span
    ijk = ijk[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))]
    return dict(ijk=np.ascontiguousarray(ijk), sums=rng.normal(0, 50, (n, 4)).astype(np.float32), counts=rng.integers(1, 10, n).astype(np.int32),
                moments=rng.normal(0, 1, (n, 12)).astype(np.float32) if surfels else None)


def context(M, rows, surfels, capacity=None, **kw):
    """a context whose world map holds rows[m] in map m; capacity_voxels = the voxels held unless given"""
    c = M.Context(max_scans=1, max_velo_points=1024, max_livox_points=1024, **kw)
    c.world_map_create(len(rows), LEAF, capacity or max(1, sum(len(r["ijk"]) for r in rows)), surfels=surfels)
    for m, r in enumerate(rows):
        c.world_map_import(m, **r)
    return c


def exports(c, n_maps):
    return {m: c.world_map_export(m) for m in range(n_maps)}


def api_rules(M, rules):
    return [M.wm_evict_rule(**r) for r in rules]


def check_call(M, c, n_maps, rules):
    """one world_map_evict against the restatement; returns (what the maps held before, the rows handed back)"""
    before = exports(c, n_maps)
    left, gone, infos = E.evict(before, rules)
    info, rows = c.world_map_evict(api_rules(M, rules))
    for m in range(n_maps):
        assert E.same(c.world_map_export(m), left[m]), (m, rules)
        assert c.world_map_size(m) == len(left[m]["ijk"])
    assert c.world_map_size(-1) == sum(len(v["ijk"]) for v in left.values())
    for r, i, want in zip(rules, info, infos):
        assert {k: getattr(i, k) for k in want} == want, (r, want)
        assert E.same(rows[r["map"]], gone[r["map"]]), r
    return before, rows


CASES = [E.rule(1, mode, *box, min_count=mc) for mode in (E.OUTSIDE, E.INSIDE, E.NOBOX) for box in (BIG, HALF, EMPTY) for mc in (0, 3)] + \
        [E.rule(1, E.NOBOX, *BIG, min_count=10), E.rule(1, E.INSIDE, *HALF, min_count=1)]


@pytest.mark.parametrize("surfels", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_against_the_restatement(M, n, surfels):
    """two maps of n voxels in a full table; a rule for map 1 under every mode, min_count 0 and 3, on boxes that evict none, some
    and all; the rows come back in key order, and importing them again restores the map"""
    rng = np.random.default_rng(100 + n)
    rows = [make_rows(rng, n, surfels), make_rows(rng, n, surfels)]
    c = context(M, rows, surfels)
    try:
        seen = set()
        for r in CASES:
            before, back = check_call(M, c, 2, [r])
            assert E.same(before[0], rows[0]) and E.same(before[1], rows[1])
            seen.add(0 if len(back[1]["ijk"]) == 0 else 2 if len(back[1]["ijk"]) == n else 1)
            c.world_map_import(1, **back[1])                                    # evict, then import: every export is what it was
            assert E.same(c.world_map_export(1), rows[1]) and E.same(c.world_map_export(0), rows[0])
        assert n < 63 or seen == {0, 1, 2}                                      # none, some and all went somewhere
    finally:
        c.close()


def test_one_map_in_a_table_of_exactly_its_capacity(M):
    rng = np.random.default_rng(7)
    rows = [make_rows(rng, 1000, True)]
    c = context(M, rows, True, capacity=1000)
    try:
        for r in (E.rule(0, E.OUTSIDE, *HALF, min_count=3), E.rule(0, E.INSIDE, *BIG), E.rule(0, E.NOBOX, min_count=5)):
            _, back = check_call(M, c, 1, [r])
            c.world_map_import(0, **back[0])
            assert E.same(c.world_map_export(0), rows[0])
    finally:
        c.close()


def raw_evict(M, c, rules, capacity, surfels, flags=0):
    """mml_world_map_evict itself: (rc, infos, n_evicted, out_map, ijk, sums, counts, moments)"""
    arr = (M.WmEvictRule * len(rules))(*api_rules(M, rules))
    info = (M.WmEvictInfo * len(rules))()
    n = C.c_long(-1)
    cap = max(capacity, 1)
    omap, ijk, sums, counts = np.full(cap, -7, np.int32), np.zeros((cap, 3), np.int32), np.zeros((cap, 4), np.float32), np.zeros(cap, np.int32)
    mom = np.zeros((cap, 12), np.float32) if surfels else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = M.lib().mml_world_map_evict(c._h, len(rules), arr, flags, info, capacity, p(omap), p(ijk), p(sums), p(counts), p(mom), C.byref(n))
    return rc, list(info), n.value, omap, ijk, sums, counts, mom


def test_several_maps_in_one_call(M):
    rng = np.random.default_rng(11)
    rows = [make_rows(rng, n, True) for n in (300, 200, 257)]
    rules = [E.rule(2, E.INSIDE, *HALF, min_count=2), E.rule(0, E.OUTSIDE, *HALF, min_count=0)]      # map 2 first, then map 0
    left, gone, infos = E.evict(dict(enumerate(rows)), rules)
    c, d = context(M, rows, True), context(M, rows, True)
    try:
        n0, n2 = len(gone[0]["ijk"]), len(gone[2]["ijk"])
        assert min(n0, n2) > 50
        rc, info, n, omap, ijk, sums, counts, mom = raw_evict(M, c, rules, n0 + n2 + 5, True)
        assert rc == M.MML_OK and n == n0 + n2
        assert omap[:n].tolist() == [0] * n0 + [2] * n2 and (omap[n:] == -7).all()              # map 0's run, then map 2's
        assert [i.first_row for i in info] == [n0, 0] and [i.n_evicted for i in info] == [n2, n0]
        assert [(i.n_before, i.n_kept) for i in info] == [(257, 257 - n2), (300, 300 - n0)]
        for m, a in ((0, 0), (2, n0)):
            b = a + len(gone[m]["ijk"])
            assert E.same(dict(ijk=ijk[a:b], sums=sums[a:b], counts=counts[a:b], moments=mom[a:b]), gone[m])
        assert E.same(c.world_map_export(1), rows[1])                                           # the map not named keeps every bit
        # ... and two calls with one rule each leave the same bytes
        back = {}
        for r in rules:
            back.update(d.world_map_evict(api_rules(M, [r]))[1])
        for m in range(3):
            assert E.same(c.world_map_export(m), left[m]) and E.same(d.world_map_export(m), left[m])
            assert c.world_map_size(m) == d.world_map_size(m) == len(left[m]["ijk"])
        assert E.same(back[0], gone[0]) and E.same(back[2], gone[2])
    finally:
        c.close()
        d.close()


@pytest.mark.parametrize("surfels", [False, True])
def test_the_table_is_still_a_table(M, surfels):
    rng = np.random.default_rng(5)
    rows = make_rows(rng, 1000, surfels)
    rule = E.rule(0, E.INSIDE, *HALF)
    left, gone, _ = E.evict({0: rows}, [rule])
    left, gone = left[0], gone[0]
    assert 400 < len(gone["ijk"]) < 600
    c = context(M, [rows], surfels)
    d = context(M, [left], surfels, capacity=1000)                              # a map that never held the evicted voxels
    try:
        _, back = c.world_map_evict(api_rules(M, [rule]))
        assert E.same(back[0], gone)
        # (a) every survivor is found: importing it again is refused
        with pytest.raises(M.MmlError) as e:
            c.world_map_import(0, **left)
        assert e.value.code == M.MML_ERR_STATE
        for r in rng.choice(len(left["ijk"]), 64, replace=False):
            with pytest.raises(M.MmlError) as e:
                c.world_map_import(0, **E.take(left, [r]))
            assert e.value.code == M.MML_ERR_STATE
        assert E.same(c.world_map_export(0), left)
        # (b) no evicted voxel is found: importing them all succeeds, and the map is the original one
        c.world_map_import(0, **back[0])
        assert E.same(c.world_map_export(0), rows)
        # (c) an add sees survivors and free places alike: points into 20 survivors, 20 evicted voxels and 5 voxels never held
        c.world_map_evict(api_rules(M, [rule]), rows=False)
        assert E.same(c.world_map_export(0), left)
        fresh = np.array([[SPAN + 1, a, -a] for a in range(5)], np.int32)
        into = np.concatenate([left["ijk"][:20], gone["ijk"][:20], fresh, gone["ijk"][:3]])
        rec = records((into.astype(np.float32) + np.float32(0.5)) * np.float32(LEAF))
        out = []
        for x in (c, d):
            upload(x, 0, rec)
            info = x.world_map_add(0, [0], I4)
            assert (info.n_kept, info.n_new_voxels) == (48, 25)
            out.append(x.world_map_export(0))
        assert E.same(out[0], out[1])
        ijk = out[0]["ijk"]
        assert len(np.unique(ijk, axis=0)) == len(ijk) == len(left["ijk"]) + 25
        count_of = {tuple(v): n for v, n in zip(ijk.tolist(), out[0]["counts"].tolist())}
        assert [count_of[tuple(v)] for v in gone["ijk"][:20].tolist()] == [2] * 3 + [1] * 17      # from zero
        assert [count_of[tuple(v)] for v in left["ijk"][:20].tolist()] == (left["counts"][:20] + 1).tolist()   # from the stored sum
    finally:
        c.close()
        d.close()


def test_dry_run_capacity_refusal_and_nothing_to_evict(M):
    rng = np.random.default_rng(9)
    rows = [make_rows(rng, 257, False), make_rows(rng, 65, False)]
    c = context(M, rows, False)
    try:
        rule = E.rule(0, E.OUTSIDE, *HALF, min_count=3)
        _, gone, infos = E.evict(dict(enumerate(rows)), [rule])
        n_ev = infos[0]["n_evicted"]
        assert 100 < n_ev < 257
        same_as_before = lambda: all(E.same(c.world_map_export(m), rows[m]) and c.world_map_size(m) == len(rows[m]["ijk"]) for m in (0, 1))
        info = c.world_map_evict(api_rules(M, [rule]), dry=True)                # a dry run: the counts, nothing else
        assert {k: getattr(info[0], k) for k in infos[0]} == infos[0] and same_as_before()
        rc, info, n, omap, *_ = raw_evict(M, c, [rule], 300, False, flags=M.MML_WM_EVICT_DRY)
        assert rc == M.MML_OK and n == n_ev and (omap == -7).all() and same_as_before()
        rc, info, n, omap, *_ = raw_evict(M, c, [rule], n_ev - 1, False)         # one row too few
        assert rc == M.MML_ERR_CAPACITY and n == n_ev and {k: getattr(info[0], k) for k in infos[0]} == infos[0]
        msg = M.lib().mml_last_error(c._h).decode()
        assert str(n_ev) in msg and str(n_ev - 1) in msg, msg
        assert (omap == -7).all() and same_as_before()
        for nothing in (E.rule(0, E.OUTSIDE, *BIG), E.rule(1, E.INSIDE, *EMPTY, min_count=1), E.rule(1, E.NOBOX)):
            info, back = c.world_map_evict(api_rules(M, [nothing]))
            assert info[0].n_evicted == 0 and info[0].n_kept == info[0].n_before == len(rows[nothing["map"]]["ijk"])
            assert len(back[nothing["map"]]["ijk"]) == 0 and same_as_before()
        rc, info, n, *_ = raw_evict(M, c, [rule], n_ev, False)                   # exactly enough
        assert rc == M.MML_OK and n == n_ev and c.world_map_size(0) == 257 - n_ev and c.world_map_size(-1) == 257 + 65 - n_ev
    finally:
        c.close()


def test_surfel_cache_follows_an_eviction(M):
    """a real eviction makes the next score call rebuild the surfel cache; a dry run, a refusal and a call that evicts nothing do not"""
    rng = np.random.default_rng(31)
    c = M.Context(max_scans=2, max_velo_points=4096, max_livox_points=4096, max_features=512)
    d = M.Context(max_scans=2, max_velo_points=4096, max_livox_points=4096, max_features=512)
    try:
        c.world_map_create(1, ROOM_LEAF, 1024, surfels=True)
        d.world_map_create(1, ROOM_LEAF, 1024, surfels=True)
        Ta = shift([0.2, 0.1, 0.0])
        rec = records(sensor_frame(scene_points(rng, 2500), Ta))
        upload(c, 0, rec)
        c.world_map_add(0, [0], Ta)
        Tf = shift([0.1, -0.1, 0.05])
        feats = scan(rng, 300, Tf)
        stack(c, 1, feats)
        stack(d, 1, feats)
        T = Tf[None, None]
        o = M.wm_score_opts(ROOM_LEAF, max_plane_dist=0.25)
        c.profile_enable(True)
        builds = lambda: c.profile_get().get("wm_surfel_cache", (0.0, 0))[1]
        first = c.world_map_score(1, [0], T, o)[0]
        assert first["n_match"][0] > 50 and builds() == 1
        full = c.world_map_export(0)
        lo, hi = c.world_map_index_box((-50.0, -50.0, -50.0), (0.3, 50.0, 50.0))               # the half of the room with x below its centre
        rule = E.rule(0, E.INSIDE, lo, hi)
        left, gone, _ = E.evict({0: full}, [rule])
        assert len(gone[0]["ijk"]) > 100 and len(left[0]["ijk"]) > 100
        c.world_map_evict(api_rules(M, [rule]), dry=True)
        assert equal(c.world_map_score(1, [0], T, o)[0], first) and builds() == 1                # a dry run: the cache stands
        c.world_map_evict(api_rules(M, [E.rule(0, E.NOBOX)]))
        rc = raw_evict(M, c, [rule], 1, True)[0]
        assert rc == M.MML_ERR_CAPACITY
        assert equal(c.world_map_score(1, [0], T, o)[0], first) and builds() == 1                # nothing evicted, refused: it stands
        c.world_map_evict(api_rules(M, [rule]), rows=False)
        after = c.world_map_score(1, [0], T, o)[0]
        assert builds() == 2 and not equal(after, first) and after["n_match"][0] < first["n_match"][0]
        d.world_map_import(0, **left[0])                                                       # a map that never held them
        assert equal(d.world_map_score(1, [0], T, o)[0], after) and after["n_match"][0] > 10
    finally:
        c.close()
        d.close()


def test_refusals(M):
    rng = np.random.default_rng(13)
    rows = [make_rows(rng, 65, False), make_rows(rng, 64, False)]
    c, s = context(M, rows, False), context(M, [make_rows(rng, 10, True)], True)
    try:
        L, h = M.lib(), c._h
        ok = E.rule(0, E.INSIDE, *BIG)
        arr = lambda rules: (M.WmEvictRule * len(rules))(*api_rules(M, rules))
        a = [np.zeros(200, np.int32), np.zeros((200, 3), np.int32), np.zeros((200, 4), np.float32), np.zeros(200, np.int32), np.zeros((200, 12), np.float32)]
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        full = [p(x) for x in a[:4]] + [None]
        call = lambda rules, n=None, flags=0, cap=200, out=full, handle=h: L.mml_world_map_evict(
            handle, len(rules) if n is None else n, arr(rules) if rules else None, flags, None, cap, *out, None)
        refusals = [
            call(None, n=1),                                                  # NULL rules
            call([ok], n=0), call([ok, E.rule(1), ok], n=3),                  # n_rules outside 1 .. n_maps
            call([E.rule(2)]), call([E.rule(-1)]),                            # a map outside [0, n_maps)
            call([ok, E.rule(0, E.NOBOX)]),                                   # a map named twice
            call([E.rule(0, 3)]), call([E.rule(0, -1)]),                      # an unknown mode
            call([E.rule(0, E.NOBOX, min_count=-1)]),
            call([ok], flags=2), call([ok], flags=3),                         # unknown flag bits
            call([ok], cap=-1),
            call([ok], out=[None] + full[1:]), call([ok], out=full[:1] + [None] + full[2:]),      # out arrays partly NULL
            call([ok], out=full[:2] + [None] + full[3:]), call([ok], out=full[:3] + [None, None]),
            call([ok], out=[None] * 5),                                       # (a capacity without arrays)
            call([ok], out=full[:4] + [p(a[4])]),                             # moments on a plain map
            call([ok], out=full, handle=s._h),                                # ... and none on a surfel map
        ]
        assert refusals == [M.MML_ERR_INVALID] * len(refusals)
        assert "rule 1" in (call([ok, E.rule(0, E.NOBOX)]), L.mml_last_error(h).decode())[1]    # the message names the rule
        assert all(E.same(c.world_map_export(m), rows[m]) for m in (0, 1)) and c.world_map_size(-1) == 129
        assert s.world_map_size(0) == 10
        c.world_map_destroy()
        assert call([ok]) == M.MML_ERR_STATE
    finally:
        c.close()
        s.close()


def test_rolling_world_map(M, synth):
    """BatchLidarOdometry(world_map_roll=...) with an on_evict that collects rows: per sequence the survivors and the collected
    rows together are the voxels of the same run without rolling, bit for bit wherever a voxel was not created again after an
    eviction.  Those are counted, printed, and must be less than a tenth: the half extent cuts off only the ceiling, which the
    sensors see from afar -- the voxel arithmetic of tests/world_map_ref.py on the raw scans at the room's ground-truth poses
    leaves out 121 of 10 044 and 137 of 8 729 voxels, the device run on the labelled points 176 of 8 443 and 234 of 7 080.  The
    poses do not change."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    W_, rounds = 2, 3
    inputs = [_sequence_inputs(synth, w, rounds) for w in range(W_)]
    runs = {}
    for roll in (False, True):
        c = M.Context(max_scans=W_, max_map_points=1 << 19)
        try:
            collected = {w: [] for w in range(W_)}
            kw = dict(world_map_roll=((30.0, 30.0, 1.9), 1), on_evict=lambda w, rows: collected[w].append(rows)) if roll else {}
            bat = odometry.BatchLidarOdometry(c, W_, lidar_mode=2, world_map=(0.2, 1 << 16), **kw)
            poses_out = []
            for i in range(rounds):
                for w in range(W_):
                    c.scan_upload(w, inputs[w][i][0], inputs[w][i][1])
                c.extract(0, W_)
                c.undistort(0, W_, np.stack([inputs[w][i][2].reshape(9) for w in range(W_)]), np.stack([inputs[w][i][3] for w in range(W_)]))
                P, Q, grew = bat.estimate_lidar_pose(list(range(W_)), np.stack([inputs[w][i][4] for w in range(W_)]),
                                                     np.stack([inputs[w][i][5] for w in range(W_)]))
                poses_out.append((P.tobytes(), Q.tobytes(), tuple(grew)))
            runs[roll] = (poses_out, exports(c, W_), collected)
        finally:
            c.close()
    assert runs[True][0] == runs[False][0]
    for w in range(W_):
        whole, left, parts = runs[False][1][w], runs[True][1][w], runs[True][2][w]
        assert len(parts) == rounds and sum(len(p["ijk"]) for p in parts) > 200
        ijk = np.concatenate([left["ijk"]] + [p["ijk"] for p in parts])
        sums = np.concatenate([left["sums"]] + [p["sums"] for p in parts])
        counts = np.concatenate([left["counts"]] + [p["counts"] for p in parts])
        uniq, first, times = np.unique(ijk, axis=0, return_index=True, return_counts=True)
        want = {tuple(v): r for r, v in enumerate(whole["ijk"].tolist())}
        assert set(want) == set(map(tuple, uniq.tolist()))                      # the same voxel set
        again = int((times > 1).sum())
        print("sequence %d: %d voxels, %d created again after an eviction and left out" % (w, len(want), again))
        assert again <= len(want) // 10
        once = first[times == 1]
        at = np.array([want[tuple(v)] for v in ijk[once].tolist()])
        assert sums[once].tobytes() == whole["sums"][at].tobytes() and counts[once].tobytes() == whole["counts"][at].tobytes()
