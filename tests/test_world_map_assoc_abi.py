"""Localisation in a surfel map, what needs no device: the C-ABI of the six entry points, the option defaults, the refusals that
are decided before a context is touched, and the restatement's own candidate choice (tests/world_map_assoc_ref.py) on scripted
cases -- ties in r2 broken by the key, a point on a voxel face, the index-range edges, a winner that fails each gate."""
import ctypes as C

import numpy as np

import world_map_assoc_ref as A
import world_map_ref as R

LEAF = 0.5


def test_symbols_structs_and_defaults(M):
    L = M.lib()
    for name in list(M.WORLD_MAP_LOCALIZE_ARGTYPES) + ["mml_wm_assoc_opts_default", "mml_wm_localize_opts_default"]:
        assert hasattr(L, name), name
    assert C.sizeof(M.WmAssocOpts) == 24 and C.sizeof(M.WmLocalizeOpts) == 24 + 24 + 8
    o = M.wm_assoc_opts(LEAF)
    assert (o.neighbourhood, o.min_points, o.min_planarity, o.max_plane_dist) == (1, 5, 0.5, 0.5)
    o = M.wm_assoc_opts(0.2)
    assert o.max_plane_dist == float(np.float32(0.2))
    lo = M.wm_localize_opts(LEAF)
    assert list(lo.max_plane_dist_by_outer) == [1.0, 0.5, 0.25] and (lo.max_outer, lo.inner_iters) == (5, 10) and lo.assoc.min_points == 5
    L.mml_wm_assoc_opts_default(None, C.c_float(1.0))      # a NULL is ignored


def test_null_context_is_refused_before_anything_else(M):
    L = M.lib()
    ijk, sums, cnt = np.zeros((1, 3), np.int32), np.zeros((1, 4), np.float32), np.ones(1, np.int32)
    n = C.c_long(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mml_world_map_export(None, 0, None, None, None, None, 0, C.byref(n)) == M.MML_ERR_INVALID and n.value == -7
    assert L.mml_world_map_import(None, 0, 1, p(ijk), p(sums), p(cnt), None) == M.MML_ERR_INVALID
    o, lo = M.wm_assoc_opts(LEAF), M.wm_localize_opts(LEAF)
    m, T = np.zeros(1, np.int32), np.eye(4)
    P, Q = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    assert L.mml_world_map_associate(None, 0, 1, p(m), p(T), C.byref(o), None) == M.MML_ERR_INVALID
    assert L.mml_world_map_localize(None, 0, 1, p(m), p(T), p(P), p(Q), C.byref(lo), None) == M.MML_ERR_INVALID


def _table(entries):
    """(i, j, k) -> (centroid, count, planarity, normal) as the restatement's table of map 0"""
    out = {}
    for ijk, (c, n, planarity, normal) in entries.items():
        sur = np.zeros(8, np.float32)
        sur[:3], sur[6] = normal, planarity
        out[R.pack(0, *ijk)] = (np.asarray(c, np.float32), n, sur)
    return out


def test_restatement_choice_on_scripted_cases():
    inv, o = R.inv_leaf(LEAF), A.options(LEAF)
    up = (0.0, 0.0, 1.0)
    w = np.array([0.5, 0.25, 0.25], np.float32)                       # on the face x = 0.5: its voxel is (1, 0, 0)
    tab = _table({(0, 0, 0): ((0.25, 0.25, 0.25), 9, 0.9, up), (1, 0, 0): ((0.75, 0.25, 0.25), 9, 0.9, up)})
    win, why = A.choose(tab, 0, w, inv, o)
    assert why == "ok" and win[0] == R.pack(0, 0, 0, 0)                # a tie in r2: the smaller key
    assert A.choose(tab, 0, w, inv, A.options(LEAF, neighbourhood=0))[0][0] == R.pack(0, 1, 0, 0)
    tab = _table({(0, 0, 0): ((0.3, 0.25, 0.25), 4, 0.9, up), (1, 0, 0): ((0.9, 0.25, 0.25), 5, 0.9, up)})
    assert A.choose(tab, 0, w, inv, o)[0][0] == R.pack(0, 1, 0, 0)     # the nearer voxel has min_points - 1 points
    assert A.choose({}, 0, w, inv, o) == (None, "none")
    assert A.choose(tab, 0, np.array([np.nan, 0, 0], np.float32), inv, o) == (None, "skipped")
    assert A.choose(tab, 0, np.array([R.HALF * LEAF, 0, 0], np.float32), inv, o) == (None, "skipped")
    for i in (R.HALF - 1, -R.HALF):                                     # the neighbours beyond the range are not looked up
        e = _table({(i, 0, 0): (((i + 0.5) * LEAF, 0.25, 0.25), 7, 0.9, up)})
        assert A.choose(e, 0, np.array([(i + 0.5) * LEAF, 0.25, 0.25], np.float32), inv, o)[0][0] == R.pack(0, i, 0, 0)
    m = R.HALF - 1                                                      # the one voxel whose key is the free marker
    assert R.pack(1023, m, m, m) == R.EMPTY
    e = {R.EMPTY: (np.full(3, (m + 0.5) * LEAF, np.float32), 9, np.zeros(8, np.float32))}
    assert A.choose(e, 1023, np.full(3, (m + 0.5) * LEAF, np.float32), inv, o) == (None, "none")
