"""Relocalisation in a surfel map, what needs no device: the C-ABI of the new entry points, the struct sizes, the option defaults,
the refusals that are decided before a context is touched, and the restatement's own score (tests/world_map_score_ref.py) on
scripted cases against the one-feature restatement of the association (tests/world_map_assoc_ref.py)."""
import ctypes as C

import numpy as np

import world_map_assoc_ref as A
import world_map_ref as R
import world_map_score_ref as W

LEAF = 0.5


def test_symbols_structs_and_defaults(M):
    L = M.lib()
    for name in list(M.WORLD_MAP_SCORE_ARGTYPES) + ["mml_wm_score_opts_default", "mml_wm_reloc_opts_default"]:
        assert hasattr(L, name), name
    assert C.sizeof(M.WmScore) == 16 and M.WM_SCORE_DT.itemsize == 16 and C.sizeof(M.WmScoreOpts) == 32
    assert C.sizeof(M.WmRelocOpts) == 48 + 16 + 32 + 56 and C.sizeof(M.WmRelocInfo) == 48 + 8 + 128 + 16
    assert (M.WmScore.score_q.offset, M.WmScore.n_match.offset, M.WmScore.n_scored.offset) == (0, 8, 12)
    assert [M.WM_SCORE_DT.fields[n][1] for n in ("score_q", "n_match", "n_scored")] == [0, 8, 12]
    o = M.wm_score_opts(LEAF)
    assert (o.stride, o.assoc.neighbourhood, o.assoc.min_points, o.assoc.min_planarity, o.assoc.max_plane_dist) == (1, 1, 5, 0.5, 0.5)
    assert M.wm_score_opts(0.2).assoc.max_plane_dist == float(np.float32(0.2))
    o = M.wm_score_opts(LEAF, stride=3, max_plane_dist=0.25, neighbourhood=0)
    assert (o.stride, o.assoc.max_plane_dist, o.assoc.neighbourhood) == (3, 0.25, 0)
    r = M.wm_reloc_opts(LEAF)
    assert (r.half_xy, r.step_xy, r.half_z, r.half_yaw, r.step_yaw) == (2.0, 0.5, 0.0, np.pi, np.pi / 16)
    assert (r.levels, r.refine, r.keep, r.score.stride, r.score.assoc.max_plane_dist) == (2, 2, 4, 1, 0.5)
    assert list(r.localize.max_plane_dist_by_outer) == [1.0, 0.5, 0.25] and (r.localize.max_outer, r.localize.inner_iters) == (5, 10)
    L.mml_wm_score_opts_default(None, C.c_float(1.0))      # a NULL is ignored
    L.mml_wm_reloc_opts_default(None, C.c_float(1.0))


def test_null_arguments_are_refused_before_anything_else(M):
    L = M.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o, r = M.wm_score_opts(LEAF), M.wm_reloc_opts(LEAF)
    m, T = np.zeros(1, np.int32), np.eye(4)
    P, Q = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    out = np.zeros(1, M.WM_SCORE_DT)
    assert L.mml_world_map_score(None, 0, 1, p(m), 1, p(T), C.byref(o), p(out)) == M.MML_ERR_INVALID
    assert L.mml_world_map_relocalize(None, 0, 1, p(m), p(T), p(P), p(Q), C.byref(r), None) == M.MML_ERR_INVALID
    assert L.mml_wm_body_pose(None, p(T), p(P), p(Q)) == M.MML_ERR_INVALID
    assert L.mml_wm_body_pose(p(T), p(T), p(P), None) == M.MML_ERR_INVALID


def test_body_pose_inverts_the_composition(M):
    from scipy.spatial.transform import Rotation as Rsc
    rng = np.random.default_rng(2)
    for _ in range(20):
        ex, Twb = np.eye(4), np.eye(4)
        ex[:3, :3], ex[:3, 3] = Rsc.from_rotvec(rng.normal(0, 0.5, 3)).as_matrix(), rng.normal(0, 0.3, 3)
        Twb[:3, :3], Twb[:3, 3] = Rsc.from_rotvec(rng.normal(0, 1.5, 3)).as_matrix(), rng.normal(0, 3.0, 3)
        P, Q = M.wm_body_pose(Twb @ np.linalg.inv(ex), ex)
        assert np.abs(P - Twb[:3, 3]).max() < 1e-12 and np.abs(Rsc.from_quat(Q).as_matrix() - Twb[:3, :3]).max() < 1e-12
        assert abs(np.linalg.norm(Q) - 1.0) < 1e-15
        assert np.abs(M.wm_lidar_pose(P, Q, ex) - Twb @ np.linalg.inv(ex)).max() < 1e-12


def _table(entries):
    out = {}
    for ijk, (c, n, planarity, normal) in entries.items():
        sur = np.zeros(8, np.float32)
        sur[:3], sur[6] = normal, planarity
        out[R.pack(0, *ijk)] = (np.asarray(c, np.float32), n, sur)
    return out


def test_restatement_score_agrees_with_the_one_feature_restatement():
    """W.statuses restates A.associate over whole arrays: on random stacks around a few voxels every status is A.associate's
    reason and a match is a record of A.associate; the quantum is 65536 at d = 0 and 0 at the gate."""
    rng = np.random.default_rng(11)
    inv = R.inv_leaf(LEAF)
    ref = type("Ref", (), dict(inv=inv))()
    names = {"skipped": W.SKIPPED, "none": W.NONE, "planarity": W.PLANARITY, "distance": W.DISTANCE, "factor": W.MATCH}
    seen = set()
    for case in range(40):
        entries = {}
        for _ in range(12):
            ijk = tuple(int(v) for v in rng.integers(-2, 2, 3))
            n = rng.normal(0, 1, 3)
            entries[ijk] = ((np.array(ijk) + rng.random(3)) * LEAF, int(rng.integers(2, 9)), float(rng.choice([0.2, 0.5, 0.9])), n / np.linalg.norm(n))
        table = _table(entries)
        feats = rng.uniform(-1.2, 1.2, (30, 3)).astype(np.float32)
        feats[0, 0] = np.nan
        feats[1, 1] = (R.HALF + 2) * LEAF
        T = np.eye(4)
        T[:3, 3] = rng.normal(0, 0.05, 3)
        for nb in (0, 1):
            for stride in (1, 3):
                o = W.options(LEAF, stride=stride, neighbourhood=nb, max_plane_dist=0.125, min_points=4)
                st, q = W.statuses(W.Table(table, 0), inv, feats, T[None], o)
                rec, src, why = A.associate(ref, None, 0, feats[::stride], T, {k: v for k, v in o.items() if k != "stride"}, table)
                assert st[0].tolist() == [names[w] for w in why]
                assert np.flatnonzero(st[0] == W.MATCH).tolist() == src.tolist()
                s = W.score(W.Table(table, 0), inv, feats, T[None], o)[0]
                assert s["n_match"] == len(src) and s["n_scored"] == len(why) - why.count("skipped") and s["score_q"] == q.sum()
                assert (q[0][st[0] != W.MATCH] == 0).all() and (q <= 65536).all()
                seen |= set(why)
    assert seen == set(names)
    tab = W.Table(_table({(0, 0, 0): ((0.25, 0.25, 0.25), 9, 0.9, (0.0, 0.0, 1.0))}), 0)
    f = np.array([[0.25, 0.25, 0.25], [0.1, 0.4, 0.375], [0.1, 0.4, 0.125]], np.float32)
    st, q = W.statuses(tab, inv, f, np.eye(4)[None], W.options(LEAF, max_plane_dist=0.125))
    assert st.tolist() == [[4, 4, 4]] and q.tolist() == [[65536, 0, 0]]
    s = np.zeros(4, W.SCORE_DT)
    s["score_q"], s["n_match"] = [5, 9, 9, 9], [1, 2, 3, 3]
    assert W.ranking(s) == [2, 3, 1, 0]
