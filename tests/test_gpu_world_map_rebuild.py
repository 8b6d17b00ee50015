"""GPU suite for the world map's rebuild -- gather the survivors, clear the keys, put them back -- which mml_world_map_reset(map)
and mml_world_map_evict share: reset(map) at the survivor counts where the gather and the put have a launch with nothing to do, a
partial wave and an exact workgroup, and the two callers against each other.  Maps are built as in test_gpu_world_map_evict.py
(hand-made rows through world_map_import, capacity_voxels equal to the voxels held, so probe chains are long); every comparison
is bit for bit."""
import numpy as np
import pytest

import world_map_evict_ref as E
from test_gpu_world_map import I4, records, upload
from test_gpu_world_map_evict import EMPTY, LEAF, SPAN, api_rules, context, exports, make_rows

pytestmark = pytest.mark.gpu


def sizes(c, n_maps):
    return [c.world_map_size(m) for m in range(n_maps)] + [c.world_map_size(-1)]


@pytest.mark.parametrize("surfels", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_reset_of_one_map_at_the_survivor_count_edges(M, n, surfels):
    """map 0 holds the n survivors, map 1 five rows (reset returns early on an empty map); reset(1) leaves map 0 bit for bit, an
    import restores map 1, and reset(0) -- five survivors -- leaves map 1"""
    rng = np.random.default_rng(300 + n)
    rows = [make_rows(rng, n, surfels), make_rows(rng, 5, surfels)]
    none = E.take(rows[1], np.zeros(5, bool))
    c = context(M, rows, surfels)
    try:
        assert sizes(c, 2) == [n, 5, n + 5]
        c.world_map_reset(1)
        assert E.same(c.world_map_export(0), rows[0])
        assert len(c.world_map_export(1)["ijk"]) == 0 and E.same(c.world_map_export(1), none)
        assert sizes(c, 2) == [n, 0, n]
        c.world_map_import(1, **rows[1])
        assert E.same(c.world_map_export(0), rows[0]) and E.same(c.world_map_export(1), rows[1])
        assert sizes(c, 2) == [n, 5, n + 5]
        c.world_map_reset(0)
        assert E.same(c.world_map_export(1), rows[1]) and len(c.world_map_export(0)["ijk"]) == 0
        assert sizes(c, 2) == [0, 5, 5]
    finally:
        c.close()


def test_reset_and_evict_rebuild_alike(M):
    """three surfel maps of 257 voxels in two identical contexts: reset(1) in one, an eviction of the whole of map 1 (an empty box
    under OUTSIDE), rows dropped, in the other -- the same exports and sizes; then one add of four points, two into survivors and two
    into voxels never held, finds and claims alike in both"""
    rng = np.random.default_rng(41)
    rows = [make_rows(rng, 257, True) for _ in range(3)]
    rule = E.rule(1, E.OUTSIDE, *EMPTY)
    left, gone, infos = E.evict(dict(enumerate(rows)), [rule])
    assert len(gone[1]["ijk"]) == 257 and len(left[1]["ijk"]) == 0
    c, d = context(M, rows, True), context(M, rows, True)
    try:
        c.world_map_reset(1)
        info = d.world_map_evict(api_rules(M, [rule]), rows=False)
        assert {k: getattr(info[0], k) for k in infos[0]} == infos[0]
        for m in range(3):
            assert E.same(c.world_map_export(m), left[m]) and E.same(d.world_map_export(m), left[m]), m
        assert sizes(c, 3) == sizes(d, 3) == [257, 0, 257, 514]
        # the rebuilt table is still a table
        fresh = np.array([[SPAN + 1, 0, 0], [SPAN + 1, 1, -1]], np.int32)
        into = np.concatenate([rows[0]["ijk"][[3, 200]], fresh])
        rec = records((into.astype(np.float32) + np.float32(0.5)) * np.float32(LEAF))
        out = []
        for x in (c, d):
            upload(x, 0, rec)
            got = x.world_map_add(0, [0], I4)
            assert (got.n_kept, got.n_new_voxels, got.n_voxels_total) == (4, 2, 516)
            out.append(exports(x, 3))
        for m in range(3):
            assert E.same(out[0][m], out[1][m]), m
        assert E.same(out[0][1], left[1]) and E.same(out[0][2], rows[2])
        count_of = {tuple(v): k for v, k in zip(out[0][0]["ijk"].tolist(), out[0][0]["counts"].tolist())}
        assert len(count_of) == 259
        assert [count_of[tuple(v)] for v in into.tolist()] == (rows[0]["counts"][[3, 200]] + 1).tolist() + [1, 1]
        assert sizes(c, 3) == sizes(d, 3) == [259, 0, 257, 516]
    finally:
        c.close()
        d.close()
