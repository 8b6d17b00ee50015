"""The local-map increment chain of csrc/map_upkeep.hip (k_inc_to_world, k_inc_concat_bbox, k_inc_voxel_keys, the sort, heads and
scan, k_inc_centroid, k_inc_bbox_out, mml_build_grids) at its ring, voxel and count edges, against the CPU oracle.

The cases are tests/local_map_cases.py; tests/test_local_map_cases_census.py shows on the oracle alone that each reaches its edge.
The yardstick is one O.LocalMap per map with the context's leaves.  After every checked increment the returned (n_corner, n_surf)
and the downloaded cloud of each kind are compared as bytes, order included: the chain is compiled with -ffp-contract=off and no
tolerance is used anywhere.  Every case goes through all three entry points -- the own map (mml_map_increment_local), a bank
through mml_map_bank_increment, a bank through mml_map_bank_increment_segmented -- and each is compared with the oracle, not with
the others."""
import numpy as np
import pytest

import local_map_cases as L

pytestmark = pytest.mark.gpu

MM = 1 << 17   # above 65 537: the rings of family B fit


@pytest.fixture(scope="module")
def cases(O):
    return L.build_cases(O)


@pytest.fixture(scope="module")
def want(O, cases):
    """name -> the oracle's maps after every increment, computed once per case and never changed."""
    memo = {}

    def get(name, bank=None):
        key = (name, bank)
        if key not in memo:
            memo[key] = L.oracle_history(O, cases[name] if bank is None else L.bank_case(cases[name], bank))
        return memo[key]
    return get


@pytest.fixture(scope="module")
def three(M):
    """One slot, the own map and two banks; a case starts from reset rings whose memory still holds the case before."""
    c = M.Context(max_scans=1, max_map_points=MM)
    assert (c.cfg.leaf_corner, c.cfg.leaf_surf) == (np.float32(L.LEAF[0]), np.float32(L.LEAF[1]))
    c.map_banks(2)
    yield c
    c.close()


FORMS = ("own map", "bank, loop", "bank, segmented")


def _increment(c, form, T):
    if form == 0:
        return c.map_increment_local(0, T)
    nc, ns = c.bank_increment([form - 1], [0], T[None], segmented=(form == 2))
    return int(nc[0]), int(ns[0])


def _download(c, form, kind):
    return c.map_local_download(kind) if form == 0 else c.bank_download(form - 1, kind)


def _same(got_n, got, want_maps, what):
    assert got_n == (len(want_maps[0]), len(want_maps[1])), what
    for kind in range(2):
        assert got[kind].shape == want_maps[kind].shape and got[kind].tobytes() == want_maps[kind].tobytes(), (what, "kind %d" % kind)


# A: k_inc_concat_bbox's slot lookup (the binary search over s_off and its tie rule for empty slots; the early return of a workgroup
#    past `total`), increment_chunk's ring_off table, `if (max_feat)` / `if (total)` with nothing to launch.
# B: blocks_for's cap of 256 workgroups and the stride of all five kernels above 65 536 rows; k_inc_centroid's `s == off` lane and
#    pos[end - 1] + flag[end - 1]; mml_voxel_run_sum's order for runs of 1, 2, 63, 64, 65 and 65 537 points; k_run_heads at row 0.
# C: MmlVoxGrid::make / index on exact multiples of the leaf, their float neighbours and negative coordinates; k_inc_to_world's
#    double-to-float cast.
# D: mml_voxel_grid_overflows and `G.overflows ? (unsigned)i : idx` in k_inc_voxel_keys, one float either side of INT_MAX voxels,
#    and the way back once the wrap replaced the far points.
@pytest.mark.parametrize("name", L.SINGLE)
def test_single_map(three, cases, want, name):
    c, case, maps = three, cases[name], want(name)
    c.map_local_reset()
    c.bank_reset(0)
    c.bank_reset(1)
    for i, (corner, surf, T) in enumerate(case["incs"]):
        c.features_upload(0, 0, corner)
        c.features_upload(0, 1, surf)
        got_n = [_increment(c, form, T) for form in range(3)]
        if i < case["check_from"]:
            continue
        for form in range(3):
            _same(got_n[form], [_download(c, form, k) for k in range(2)], maps[i], "%s, %s, increment %d" % (name, FORMS[form], i))


# mml_build_grids behind the chain (the jobs of increment_chunk: h_back sizes and k_inc_bbox_out's boxes, its `m < cap` clamp and
# its early return for a one-point and an empty segment): the grid of a one-point map, of the 257-point mixed map, of the unfiltered
# overflow map with its far points, of a 65 537-point map.
@pytest.mark.parametrize("name", L.KNN)
def test_rebuilt_grid(M, O, cases, want, name):
    case, maps = cases[name], want(name)
    c = M.Context(max_scans=1, max_map_points=MM)
    try:
        for i, (corner, surf, T) in enumerate(case["incs"][:case["knn_at"] + 1]):
            c.features_upload(0, 0, corner)
            c.features_upload(0, 1, surf)
            got_n = c.map_increment_local(0, T)
        _same(got_n, [c.map_local_download(k) for k in range(2)], maps[i], name)
        for kind in range(2):
            cloud = maps[i][kind]
            q = L.knn_queries(cloud, 7 + kind)
            if len(cloud) < 5:                                   # no neighbour sets (test_gpu_grid_build_edges.py::test_tiny_maps)
                gi, _ = c.knn5(kind, q, max_d2=25.0)
                assert np.all(gi == -1), (name, kind)
                continue
            gi, gd = c.knn5(kind, q)
            oi, od = O.KdTree(cloud).knn5(q)
            assert np.array_equal(gi, oi) and gd.tobytes() == od.tobytes(), (name, kind)
    finally:
        c.close()


def _refused(M, c, call, names):
    with pytest.raises(M.MmlError) as e:
        call()
    msg = M.lib().mml_last_error(c._h).decode()
    assert e.value.code == M.MML_ERR_CAPACITY and names in msg, (e.value.code, msg)


# E: the capacity check of mml_map_upkeep_increment_segmented (`t > ctx->MM`, before increment_chunk writes ring_n, the ring or
#    localMapID) and `dst >= cap` of k_inc_centroid at dst = cap - 1.
def test_capacity_own_map(M, cases, want):
    case, maps = cases["E.capacity"], want("E.capacity")
    c = M.Context(max_scans=1, max_map_points=case["max_map_points"])
    try:
        for i, (corner, surf, T) in enumerate(case["incs"]):
            c.features_upload(0, 0, corner)
            c.features_upload(0, 1, surf)
            if i in case["refused"]:
                before = [c.map_local_download(k).tobytes() for k in range(2)]
                _refused(M, c, lambda: c.map_increment_local(0, T), "the context's own local map")
                assert [c.map_local_download(k).tobytes() for k in range(2)] == before == [m.tobytes() for m in maps[i]]
                continue
            # (after a refusal: the same ring slot and localMapID as an oracle that never saw the refused stacks)
            _same(c.map_increment_local(0, T), [c.map_local_download(k) for k in range(2)], maps[i], "own map, increment %d" % i)
        assert max(len(maps[i][0]) for i in range(len(maps))) == case["max_map_points"]
    finally:
        c.close()


def test_capacity_second_of_three_banks(M, O, cases, want):
    """The case on bank 1 of a three-bank segmented call; banks 0 and 2 grow by small stacks of their own.  A refused call leaves
    all three as they were, and the next round equals three oracles that never saw it."""
    case, maps = cases["E.capacity"], want("E.capacity")
    rng = np.random.default_rng(61)
    side = [[(rng.uniform(-4, 4, (3 + i, 3)).astype(np.float32), rng.uniform(-4, 4, (2 * i, 3)).astype(np.float32), L.pose(5.0 * i, (0.1 * i, 0.2, 0.3)))
             for i in range(len(case["incs"]))] for _ in range(2)]
    others = [dict(name="side", incs=s, refused=case["refused"]) for s in side]
    side_maps = [L.oracle_history(O, o) for o in others]
    c = M.Context(max_scans=3, max_map_points=case["max_map_points"])
    try:
        c.map_banks(3)
        for i, (corner, surf, T) in enumerate(case["incs"]):
            stacks = [side[0][i], (corner, surf, T), side[1][i]]
            for s, (a, b, _) in enumerate(stacks):
                c.features_upload(s, 0, a)
                c.features_upload(s, 1, b)
            Ts = np.stack([t for _, _, t in stacks])
            wanted = [side_maps[0][i], maps[i], side_maps[1][i]]
            if i in case["refused"]:
                before = [c.bank_download(b, k).tobytes() for b in range(3) for k in range(2)]
                _refused(M, c, lambda: c.bank_increment([0, 1, 2], [0, 1, 2], Ts, segmented=True), "map bank 1")
                assert [c.bank_download(b, k).tobytes() for b in range(3) for k in range(2)] == before
                assert before == [m.tobytes() for w in wanted for m in w]
                continue
            nc, ns = c.bank_increment([0, 1, 2], [0, 1, 2], Ts, segmented=True)
            for b in range(3):
                _same((int(nc[b]), int(ns[b])), [c.bank_download(b, k) for k in range(2)], wanted[b], "bank %d, increment %d" % (b, i))
    finally:
        c.close()


def _ring_points(fcase):
    """[call][bank] -> the bank's ring points of both kinds after the write (fewer calls than ring slots: the running sum)."""
    run = np.zeros(len(fcase["banks"]), int)
    out = []
    for row in fcase["calls"]:
        run = run + np.array([len(a) + len(b) for a, b, _ in row])
        out.append(run.copy())
    return out


def _budgets(fcase):
    """Chunkings of the segmented call, as budgets per call: None (the library's own), every bank alone, and with the 65 537-point
    bank a cut before it and a cut after it."""
    pts, big = _ring_points(fcase), fcase["big"]
    out = {"unchunked": [None] * len(pts), "alone": [1] * len(pts)}
    if big is not None:
        out["before"] = [int(max(p[big], p[:big].sum(), 1)) for p in pts]
        out["after"] = [int(max(p[:big + 1].sum(), 1)) for p in pts]
        last = pts[-2]
        assert big in L.chunks(last, out["before"][-2]) and big > 0
        if big + 1 < len(last) and last[big + 1:].sum() > 0:
            assert big not in L.chunks(last, out["after"][-2]) and len(L.chunks(last, out["after"][-2])) == 2
        assert len(L.chunks(last, 1)) >= int((last > 1).sum())
    return out


# F: the segment index above the voxel index -- `blockIdx.y << 32` in k_inc_voxel_keys, the sort's width 32 + seg_bits with 2 n
#    crossing 2, 4, 8, 16 -- with identical low key words in adjacent segments; cat_off of a segment without rows; max_total of a call
#    whose segments differ by five orders of magnitude (workgroups past a small segment's total return early); the greedy chunks of
#    mml_map_upkeep_increment_segmented around the large bank.
@pytest.mark.parametrize("name", L.BANKS)
def test_many_maps(M, cases, want, name):
    fcase = cases[name]
    n = len(fcase["banks"])
    banks = list(range(n))
    forms = [("loop", False, None)] + [("segmented, " + k, True, b) for k, b in _budgets(fcase).items()]
    for what, segmented, budget in forms:
        c = M.Context(max_scans=n, max_map_points=MM)
        try:
            c.map_banks(n)
            for k, row in enumerate(fcase["calls"]):
                for s, (corner, surf, _) in enumerate(row):
                    c.features_upload(s, 0, corner)
                    c.features_upload(s, 1, surf)
                if budget is not None and budget[k] is not None:
                    c.debug_bank_increment_budget(budget[k])
                nc, ns = c.bank_increment(banks, banks, np.stack([T for _, _, T in row]), segmented=segmented)
                for b in banks:                                  # every bank against its own oracle, every round
                    _same((int(nc[b]), int(ns[b])), [c.bank_download(b, kind) for kind in range(2)], want(name, b)[k],
                          "%s, %s, call %d, bank %d (%s)" % (name, what, k, b, fcase["banks"][b]))
        finally:
            c.close()
