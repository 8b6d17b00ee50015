"""GPU suite for relocalisation in a surfel map: mml_world_map_score and mml_world_map_relocalize against
tests/world_map_score_ref.py.  The scene is the room of tests/test_gpu_world_map_assoc.py (leaf 0.5 m, two maps in a table of
2 048 voxels of capacity, the sparse voxels, the blob and the edge patches outside it) with two interior wall panels of different
length, so that the room does not map onto itself under a half turn.  Scores are integers and compared exactly; the poses of the
loop to 1e-9, the bound tests/test_gpu_world_map_assoc.py test_localize holds."""
import ctypes as C
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

import world_map_assoc_ref as A
import world_map_ref as R
import world_map_score_ref as W
import world_map_surfel_ref as S
from test_gpu_world_map import I4, records, ref_add, same, upload

pytestmark = pytest.mark.gpu
LEAF = 0.5
BOX = np.array([2.0, 1.5, 1.0])
CENTRE = np.array([0.3, -0.2, 0.1])


def shift(t, rotvec=None):
    T = np.eye(4)
    T[:3, 3] = t
    if rotvec is not None:
        T[:3, :3] = Rsc.from_rotvec(rotvec).as_matrix()
    return T


def scene_points(rng, n, noise=0.003):
    """n world points: three quarters on the inside of the box's six walls, the rest on two interior panels -- x = 0.9 over
    y in [-1.5, 0.1] and y = 0.6 over x in [-2, -1.1] (relative to the centre), full height"""
    p = rng.uniform(-1, 1, (n, 3)) * BOX
    axis = rng.integers(0, 3, n)
    side = rng.choice([-1.0, 1.0], n)
    p[np.arange(n), axis] = side * BOX[axis] + rng.normal(0, noise, n)
    kind = rng.integers(0, 8, n)
    a, b = kind == 0, kind == 1
    p[a, 0], p[a, 1] = 0.9 + rng.normal(0, noise, a.sum()), rng.uniform(-1.5, 0.1, a.sum())
    p[b, 1], p[b, 0] = 0.6 + rng.normal(0, noise, b.sum()), rng.uniform(-2.0, -1.1, b.sum())
    return p + CENTRE


def sensor_frame(world, T):
    with np.errstate(invalid="ignore"):
        return ((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def scan(rng, n, T):
    return sensor_frame(scene_points(rng, n, noise=0.002), T)


def stack(ctx, slot, feats, corners=3):
    ctx.features_upload(slot, 0, np.full((corners, 3), 0.25, np.float32))
    ctx.features_upload(slot, 1, np.asarray(feats, np.float32).reshape(-1, 3))


def downloads(ctx, maps):
    out = []
    for m in maps:
        out += [a.tobytes() for a in ctx.world_map_download(m, counts=True)]
        out += [ctx.world_map_moments(m).tobytes(), ctx.world_map_surfels(m).tobytes()]
    return out + [ctx.world_map_size(-1)]


def scene():
    """the clouds of the scene and the poses they are added at: [(records, [(map, T), ...]), ...] -- what the device and the
    restatement are both built from"""
    rng = np.random.default_rng(21)
    poses = [shift([0.2, 0.1, 0.0]), shift([-0.5, 0.3, 0.2], [0.0, 0.0, 0.4])]
    tilt = shift([0.0, 0.0, 0.0], [0.02, -0.03, 0.01])
    out = []
    for T in poses:
        rec = records(sensor_frame(scene_points(rng, 9000), T))
        out.append((rec, [(0, T), (1, tilt @ T)]))
    # voxels of 1, 2 and min_points - 1 points, and a blob of low planarity, outside the room; patches at the index-range edges
    sparse = np.concatenate([np.repeat([[5.2, 0.2, 0.2]], 1, 0), np.repeat([[5.2, 1.2, 0.2]], 2, 0), np.repeat([[5.2, 2.2, 0.2]], 4, 0)]) + rng.normal(0, 0.01, (7, 3))
    blob = np.array([7.25, 0.25, 0.25]) + rng.uniform(-0.2, 0.2, (60, 3))
    ring = np.array([[0, a, b] for a in (-0.1, 0.0, 0.1) for b in (-0.1, 0.0, 0.1) if a or b])
    edge = np.array([[(R.HALF - 1 + 0.5) * LEAF, 0.2, 0.2], [(-R.HALF + 0.5) * LEAF, 0.2, 0.2]]).repeat(8, 0) + np.tile(ring, (2, 1))
    out.append((records(np.concatenate([sparse, blob, edge]).astype(np.float32)), [(0, I4)]))
    return out, tilt


def scene_ref(O):
    clouds, tilt = scene()
    ref = S.SurfelMapRef(LEAF)
    for rec, adds in clouds:
        for m, T in adds:
            ref_add(ref, m, rec, T)
    return ref, [W.table_of(ref, O, m) for m in (0, 1)], tilt


@pytest.fixture(scope="module")
def room(M, O):
    """two surfel maps in one context -- the scene, and the same clouds with the scene turned a little (other planes) -- and the
    restatement's tables of both, computed once and left unchanged"""
    c = M.Context(max_scans=4, max_velo_points=8192, max_livox_points=8192, max_features=4096)
    c.world_map_create(2, LEAF, 2048, surfels=True)
    clouds, _ = scene()
    for s, (rec, adds) in enumerate(clouds):
        upload(c, s, rec)
        for m, T in adds:
            c.world_map_add(s, [m], T)
    ref, tabs, tilt = scene_ref(O)
    yield c, ref, tabs
    c.close()


def expected(tabs, ref, map, feats, T, o):
    if map < 0:
        return np.zeros(len(T), W.SCORE_DT)
    return W.score(tabs[map], ref.inv, feats, T, o)


def equal(got, exp):
    return all(np.array_equal(got[k], exp[k]) for k in ("score_q", "n_match", "n_scored"))


def placed_features():
    """the placed features of tests/test_gpu_world_map_assoc.py, world coordinates"""
    wall_x = CENTRE[0] + BOX[0]
    return np.array([
        [wall_x - 0.004, 0.0, 0.3],                                         # on the voxel face y = 0: the winner may be a neighbour
        [wall_x + 0.001, 0.5, 0.5], [wall_x, -0.5, 0.0],                    # faces in two and three axes
        [5.2, 0.2, 0.3], [5.2, 1.2, 0.3], [5.2, 2.2, 0.3],                  # next to voxels of 1, 2 and min_points - 1 points
        [7.25, 0.25, 0.3],                                                  # next to a voxel of low planarity
        [wall_x - 0.24, 0.3, 0.3], [wall_x - 0.26, 0.3, 0.3],               # |d| just inside and just outside the gate of 0.25
        [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],                             # not finite
        [(R.HALF - 1 + 0.5) * LEAF, 0.2, 0.2], [(-R.HALF + 0.5) * LEAF, 0.2, 0.2],   # neighbours leave the range
        [(R.HALF + 3) * LEAF, 0.0, 0.0],                                    # the feature itself is out of range
    ], np.float64)


def main_stack(rng, T):
    placed = placed_features()
    feats = sensor_frame(np.concatenate([scene_points(rng, 700, noise=0.002), placed]), T)
    feats[-len(placed):][9:11] = placed[9:11].astype(np.float32)             # (the non-finite ones as they are)
    return feats


def hypothesis_pool(T):
    """around the pose T a stack was made at: the identity, T, shifts of a few centimetres and of 9 m, a small rotation, a pose
    with a NaN, a pose that moves the points beyond the index range"""
    nan = T.copy()
    nan[1, 2] = np.nan
    return [I4.copy(), T.copy(), shift([0.03, -0.02, 0.04]) @ T, shift([9.0, 9.0, 9.0]) @ T, shift([0.01, 0.0, -0.02], [0.01, -0.02, 0.03]) @ T,
            nan, shift([1.0e5, 0.0, 0.0]) @ T]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("nb", [0, 1])
def test_score_matches_restatement(M, O, room, nb, stride):
    c, ref, tabs = room
    rng = np.random.default_rng(5 + nb)
    Ts = [shift([0.1, -0.1, 0.05]), shift([9.0, 9.0, 9.0]), shift([-0.2, 0.15, 0.0], [0.01, 0.0, -0.02])]
    o = M.wm_score_opts(LEAF, neighbourhood=nb, max_plane_dist=0.25, stride=stride)
    ro = W.options(LEAF, neighbourhood=nb, max_plane_dist=0.25, stride=stride)
    maps = [1, -1, 0]
    # (stack sizes of slots 0 and 2, hypotheses per slot): the wave's edges 0, 1, 63, 64, 65, 257; one workgroup, exactly one, one over
    calls = [(None, 257, 5), (0, 1, 1), (63, 64, 4), (65, 257, 5)]
    seen = set()
    for call, (n0, n2, H) in enumerate(calls):
        feats = [main_stack(rng, Ts[0]) if n0 is None else scan(rng, n0, Ts[0]), scan(rng, 7, Ts[1]), scan(rng, n2, Ts[2])]
        for s in range(3):
            stack(c, s, feats[s], corners=s)
        T = np.stack([[hypothesis_pool(Ts[s])[(call + 2 * s + h) % 7] for h in range(H)] for s in range(3)])
        got = c.world_map_score(0, maps, T, o)
        assert got.shape == (3, H) and got.dtype == M.WM_SCORE_DT
        for s in range(3):
            exp = expected(tabs, ref, maps[s], feats[s], T[s], ro)
            assert equal(got[s], exp), (call, s, got[s], exp)
            n_looked = 0 if len(feats[s]) == 0 else (len(feats[s]) - 1) // stride + 1
            assert (got[s]["n_scored"] <= n_looked).all() and (got[s]["n_match"] <= got[s]["n_scored"]).all()
        assert not got[1].view(np.uint8).any()                                # the skipped slot's rows are zeros
        if n0 is None:                                                      # the placed features did what they were placed for
            st, q = W.statuses(tabs[1], ref.inv, feats[0], T[0], ro)
            seen |= set(st.ravel().tolist())
            h = [(call + h) % 7 for h in range(H)].index(1)                 # the hypothesis at the pose the stack was made at
            assert got[0]["n_match"][h] > (700 // stride) // 2
            for k in range(H):
                kind = (call + k) % 7
                if kind in (3, 5, 6):       # 9 m off: nothing matches; NaN: nothing is looked at; 10^5 m off: at most the patch of the far edge is
                    assert got[0]["n_match"][k] == 0 and (kind == 3 or got[0]["n_scored"][k] <= (0 if kind == 5 else 2))
    assert seen == {W.SKIPPED, W.NONE, W.PLANARITY, W.DISTANCE, W.MATCH} or nb == 0 or stride != 1


def test_restatement_counts_the_factors_of_associate(M, O, room):
    """on the first GPU test's inputs the restatement's n_match is the number of src >= 0 records of A.associate"""
    c, ref, tabs = room
    rng = np.random.default_rng(5 + 1)
    T0 = shift([0.1, -0.1, 0.05])
    feats = main_stack(rng, T0)
    for nb in (0, 1):
        for T in (T0, hypothesis_pool(T0)[2]):
            ao = A.options(LEAF, neighbourhood=nb, max_plane_dist=0.25)
            _, src, why = A.associate(ref, O, 1, feats, T, ao)
            s = W.score(tabs[1], ref.inv, feats, T[None], dict(ao, stride=1))[0]
            assert s["n_match"] == len(src) and s["n_scored"] == len(why) - why.count("skipped") and len(src) > 300


def test_score_equals_associate(M, O, room):
    c, ref, tabs = room
    rng = np.random.default_rng(9)
    T0 = shift([0.1, -0.1, 0.05])
    feats = main_stack(rng, T0)
    stack(c, 0, feats)
    pool = hypothesis_pool(T0)
    T = np.stack([pool[k] for k in (1, 2, 4, 3, 0)])
    for nb in (0, 1):
        got = c.world_map_score(0, [0], T[None], M.wm_score_opts(LEAF, neighbourhood=nb, max_plane_dist=0.25))[0]
        planes = [c.world_map_associate(0, [0], T[h], M.wm_assoc_opts(LEAF, neighbourhood=nb, max_plane_dist=0.25))[0].n_plane for h in range(5)]
        assert got["n_match"].tolist() == planes and planes[0] > 300 and planes[3] == 0, (got, planes)


def test_score_is_read_only_and_batch_invariant(M, O, room):
    c, ref, tabs = room
    rng = np.random.default_rng(13)
    Ts = [shift([0.1, -0.1, 0.05]), shift([-0.2, 0.15, 0.0], [0.01, 0.0, -0.02])]
    feats = [scan(rng, 300, Ts[0]), scan(rng, 131, Ts[1])]
    for s in range(2):
        stack(c, s, feats[s])
    c.world_map_associate(0, [0, 1], np.stack(Ts), M.wm_assoc_opts(LEAF))     # factors and statistics to be left alone
    before = (downloads(c, [0, 1]), [c.slot_digest(s, 1).tobytes() for s in range(2)], [[a.tobytes() for a in c.factors_download(s, 1)] for s in range(2)])
    T = np.stack([[hypothesis_pool(Ts[s])[k] for k in (1, 2, 4, 3, 5)] for s in range(2)])
    o = M.wm_score_opts(LEAF, stride=2)
    both = c.world_map_score(0, [0, 1], T, o)
    after = (downloads(c, [0, 1]), [c.slot_digest(s, 1).tobytes() for s in range(2)], [[a.tobytes() for a in c.factors_download(s, 1)] for s in range(2)])
    assert before == after
    for s in range(2):
        for h in range(5):
            one = c.world_map_score(s, [s], T[s, h][None, None], o)
            assert one.shape == (1, 1) and one[0, 0] == both[s, h], (s, h, one, both[s, h])
    assert both["n_match"][0, 0] > 100 and both["n_match"][1, 0] > 30 and len(set(both["score_q"].ravel().tolist())) > 4


def test_cache_follows_the_map(M, O):
    rng = np.random.default_rng(31)
    c = M.Context(max_scans=3, max_velo_points=4096, max_livox_points=4096, max_features=512)
    try:
        c.world_map_create(2, LEAF, 1024, surfels=True)
        ref = S.SurfelMapRef(LEAF)
        Ta, Tb = shift([0.2, 0.1, 0.0]), shift([-0.5, 0.3, 0.2], [0.0, 0.0, 0.4])
        rec = [records(sensor_frame(scene_points(rng, 2500), Ta)), records(sensor_frame(scene_points(rng, 2500), Tb))]
        upload(c, 0, rec[0])
        upload(c, 1, rec[1])
        c.world_map_add(0, [0], Ta)
        ref_add(ref, 0, rec[0], Ta)
        c.world_map_add(1, [1], Tb)
        ref_add(ref, 1, rec[1], Tb)
        Tf = shift([0.1, -0.1, 0.05])
        feats = scan(rng, 300, Tf)
        stack(c, 2, feats)
        T = np.stack([Tf, shift([0.03, -0.02, 0.04]) @ Tf, shift([0.0, 0.0, 0.0], [0.0, 0.0, 0.03]) @ Tf])[None]
        o, ro = M.wm_score_opts(LEAF, max_plane_dist=0.25), W.options(LEAF, max_plane_dist=0.25)
        exp = lambda m: W.score(W.table_of(ref, O, m), ref.inv, feats, T[0], ro)
        first = c.world_map_score(2, [0], T, o)[0]
        assert equal(first, exp(0)) and first["n_match"][0] > 50
        c.world_map_add(1, [0], Tb)                                          # the map grows: the cache is rebuilt
        ref_add(ref, 0, rec[1], Tb)
        grown = c.world_map_score(2, [0], T, o)[0]
        assert equal(grown, exp(0)) and not equal(grown, first)
        ex = c.world_map_export(0)                                           # the same voxels at other table positions
        c.world_map_reset(0)
        assert not c.world_map_score(2, [0], T, o)[0]["n_match"].any()       # (an empty map: everything is looked at, nothing matches)
        c.world_map_import(0, **ex)
        assert equal(c.world_map_score(2, [0], T, o)[0], grown)
        second = c.world_map_score(2, [1], T, o)[0]
        assert equal(second, exp(1)) and second["n_match"][0] > 50
        c.world_map_reset(0)                                                 # map 1's voxels are taken out and put back
        assert equal(c.world_map_score(2, [1], T, o)[0], second)
        c.world_map_reset(-1)
        assert not c.world_map_score(2, [1], T, o)[0]["n_match"].any()
    finally:
        c.close()


def test_score_refusals(M, O, room, synth):
    c, ref, tabs = room
    feats = scan(np.random.default_rng(3), 100, I4)
    stack(c, 0, feats)
    c.world_map_associate(0, [0], I4, M.wm_assoc_opts(LEAF))
    before = (downloads(c, [0, 1]), c.slot_digest(0, 2).tobytes())
    T = I4[None, None]
    cases = [dict(maps=[2]), dict(maps=[-2]), dict(min_points=2), dict(max_plane_dist=np.nan), dict(max_plane_dist=0.0), dict(max_plane_dist=-0.1),
             dict(max_plane_dist=np.inf), dict(min_planarity=np.inf), dict(neighbourhood=2), dict(stride=0), dict(stride=-3)]
    for over in cases:
        over = dict(over)
        maps = over.pop("maps", [0])
        with pytest.raises(M.MmlError) as e:
            c.world_map_score(0, maps, T, M.wm_score_opts(LEAF, **over))
        assert e.value.code == M.MML_ERR_INVALID, over
    L = M.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m, out, o = np.zeros(1, np.int32), np.zeros(1, M.WM_SCORE_DT), M.wm_score_opts(LEAF)
    for n_hyp in (0, -1, 65537):
        assert L.mml_world_map_score(c._h, 0, 1, p(m), n_hyp, p(I4), C.byref(o), p(out)) == M.MML_ERR_INVALID and "n_hyp" in L.mml_last_error(c._h).decode()
    assert L.mml_world_map_score(c._h, 0, 1, p(m), 1, None, C.byref(o), p(out)) == M.MML_ERR_INVALID
    assert L.mml_world_map_score(c._h, 0, 1, p(m), 1, p(I4), C.byref(o), None) == M.MML_ERR_INVALID
    assert L.mml_world_map_score(c._h, 0, 1, p(m), 1, p(I4), None, p(out)) == M.MML_ERR_INVALID
    assert L.mml_world_map_score(c._h, 0, 1, None, 1, p(I4), C.byref(o), p(out)) == M.MML_ERR_INVALID
    assert L.mml_world_map_score(c._h, 3, 2, p(m), 1, p(I4), C.byref(o), p(out)) == M.MML_ERR_INVALID      # the slot range
    assert not out.view(np.uint8).any() and (downloads(c, [0, 1]), c.slot_digest(0, 2).tobytes()) == before
    big = M.Context(max_scans=65, max_velo_points=256, max_livox_points=256, max_features=64)            # count x n_hyp above 2^22
    try:
        m65 = np.zeros(65, np.int32)
        assert L.mml_world_map_score(big._h, 0, 65, p(m65), 65536, p(I4), C.byref(o), p(out)) == M.MML_ERR_INVALID and "2^22" in L.mml_last_error(big._h).decode()
    finally:
        big.close()
    for kind in ("none", "plain"):               # no world map; a plain one
        x = M.Context(max_scans=1, max_velo_points=256, max_livox_points=256)
        try:
            stack(x, 0, feats)
            if kind == "plain":
                x.world_map_create(1, LEAF, 64)
            d = x.slot_digest(0, 1).tobytes()
            with pytest.raises(M.MmlError) as e:
                x.world_map_score(0, [0], T, M.wm_score_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and x.slot_digest(0, 1).tobytes() == d
            with pytest.raises(M.MmlError) as e:
                x.world_map_relocalize(0, [0], np.eye(4), np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]), M.wm_reloc_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and x.slot_digest(0, 1).tobytes() == d
        finally:
            x.close()
    x = M.Context(max_scans=2, max_features=64)  # a slot whose down-sampling overflowed holds no stack
    try:
        x.world_map_create(1, LEAF, 64, surfels=True)
        stack(x, 0, feats[:40])
        x.scan_upload(1, synth.velo_scan(3, n_az=450), synth.livox_scan(3, n=6000))
        x.extract(1, 1)
        x.downsample(1, 1)
        r = x.world_map_score(0, [0, -1], np.stack([I4, I4])[:, None], M.wm_score_opts(LEAF))   # an empty map; the skipped slot's stack is not looked at
        assert (r["n_scored"][0, 0], r["n_match"][0, 0], r["score_q"][0, 0]) == (40, 0, 0) and not r[1].view(np.uint8).any()
        digest = x.slot_digest(0, 2).tobytes()
        for first, maps in ((0, [0, 0]), (1, [0])):
            with pytest.raises(M.MmlError) as e:
                x.world_map_score(first, maps, np.stack([I4] * len(maps))[:, None], M.wm_score_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and "slot 1" in str(e.value)
        assert x.slot_digest(0, 2).tobytes() == digest
    finally:
        x.close()
    # the search's own refusals
    P0, Q0 = np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]])
    for over in (dict(levels=0), dict(levels=4), dict(refine=1), dict(refine=5), dict(keep=0), dict(keep=17), dict(step_xy=0.0), dict(half_yaw=4.0),
                 dict(half_xy=np.nan), dict(half_xy=40.0, step_xy=0.1), dict(score=M.wm_score_opts(LEAF, stride=0)), dict(score=M.wm_score_opts(LEAF, max_plane_dist=0.0)),
                 dict(localize=M.wm_localize_opts(LEAF, max_outer=0)), dict(localize=M.wm_localize_opts(LEAF, max_plane_dist_by_outer=[1.0, np.nan, 1.0]))):
        with pytest.raises(M.MmlError) as e:
            c.world_map_relocalize(0, [0], np.eye(4), P0, Q0, M.wm_reloc_opts(LEAF, **over))
        assert e.value.code == M.MML_ERR_INVALID, over
    for maps, P in (([-1], P0), ([2], P0), ([0], np.array([[np.nan, 0.0, 0.0]]))):
        with pytest.raises(M.MmlError) as e:
            c.world_map_relocalize(0, maps, np.eye(4), P, Q0, M.wm_reloc_opts(LEAF))
        assert e.value.code == M.MML_ERR_INVALID
    assert (downloads(c, [0, 1]), c.slot_digest(0, 2).tobytes()) == before


# ---- the search ----
GRID = dict(half_xy=0.6, step_xy=0.3, half_z=0.0, step_z=1.0, half_yaw=np.radians(30.0), step_yaw=np.radians(10.0), levels=2, refine=2, keep=2)
BY_OUTER = [2 * LEAF, LEAF, 0.5 * LEAF]


def reloc_cases(tilt):
    """two slots: (map, truth, seed, features) -- about 150 features each, a seed about 0.6 m and 25 degrees off"""
    rng = np.random.default_rng(77)
    def off(truth, dt, yaw_deg):
        seed = truth.copy()
        seed[:3, :3] = Rsc.from_rotvec([0.0, 0.0, np.radians(yaw_deg)]).as_matrix() @ truth[:3, :3]
        seed[:3, 3] += dt
        return seed
    truth0 = shift([0.15, -0.1, 0.05], [0.0, 0.0, 0.1])
    truth1 = tilt @ shift([-0.25, 0.2, -0.05], [0.0, 0.0, -0.2])
    world1 = scene_points(rng, 140, noise=0.002) @ tilt[:3, :3].T             # map 1 holds the scene turned by `tilt`
    return [(0, truth0, off(truth0, [0.55, -0.25, 0.02], 24.0), scan(rng, 150, truth0)),
            (1, truth1, off(truth1, [-0.35, 0.5, -0.01], -17.0), sensor_frame(world1, truth1))]


def yaw_between(Ra, Rb):
    return (Rsc.from_matrix(Ra) * Rsc.from_matrix(Rb).inv()).magnitude()


def restated_search(M, O, ref, tabs, case):
    map, truth, seed, feats = case
    grid = lambda s, *a: M.wm_pose_grid(s, *a)
    r = W.search(tabs[map], ref.inv, feats, seed, GRID, W.options(LEAF), grid)
    T, s, order = r["level0"]
    dist = [np.linalg.norm(t[:3, 3] - truth[:3, 3]) / GRID["step_xy"] + yaw_between(t[:3, :3], truth[:3, :3]) / GRID["step_yaw"] for t in T]
    P, Q = M.wm_body_pose(r["T_start"], np.eye(4))
    Pr, Qr, outer, counts, degenerate = A.localize(ref, O, map, feats, np.eye(4), P, Q, LEAF, BY_OUTER)
    err_t = np.linalg.norm(Pr - truth[:3, 3])
    err_r = yaw_between(Rsc.from_quat(Qr).as_matrix(), truth[:3, :3])
    fine_t, fine_r = GRID["step_xy"] / GRID["refine"], GRID["step_yaw"] / GRID["refine"]
    print("map %d: level-0 best %d (nearest the truth: %d), best %s second %s, %d hypotheses; the loop ends %.4f m and %.4f rad from the truth (half the finest step: %.4f m, %.4f rad)"
          % (map, order[0], int(np.argmin(dist)), r["best"], r["second"], r["n_hyp_scored"], err_t, err_r, fine_t / 2, fine_r / 2))
    # the conditions on the scene, on the restatement alone
    assert order[0] == int(np.argmin(dist))
    assert int(r["second"]["score_q"]) < int(r["best"]["score_q"]) and int(r["second"]["score_q"]) > 0
    assert err_t < fine_t / 2 and err_r < fine_r / 2 and degenerate == 0
    assert len(feats) * len(T) <= 40000 and len(feats) * (r["n_hyp_scored"] - len(T)) <= 40000
    return r, (P, Q), (Pr, Qr, outer)


def test_relocalize(M, O, room):
    c, ref, tabs = room
    cases = reloc_cases(scene()[1])
    seeds = [M.wm_body_pose(case[2], np.eye(4)) for case in cases]           # what the call is given, and the lidar pose it makes of it
    cases = [case[:2] + (M.wm_lidar_pose(P, Q, np.eye(4)),) + case[3:] for case, (P, Q) in zip(cases, seeds)]
    restated = [restated_search(M, O, ref, tabs, case) for case in cases]
    before = downloads(c, [0, 1])
    for s, case in enumerate(cases):
        stack(c, s, case[3], corners=2 + 3 * s)
    opts = M.wm_reloc_opts(LEAF, **GRID)
    singles = []
    for s, (case, (r, start, loop)) in enumerate(zip(cases, restated)):
        P, Q, info = c.world_map_relocalize(s, [case[0]], np.eye(4), seeds[s][0][None], seeds[s][1][None], opts)
        i = info[0]
        for name in ("best", "second"):
            got = getattr(i, name)
            assert (got.score_q, got.n_match, got.n_scored) == tuple(int(r[name][k]) for k in ("score_q", "n_match", "n_scored")), (s, name)
        assert i.n_hyp_scored == r["n_hyp_scored"] and same(np.array(i.T_start).reshape(4, 4), r["T_start"])
        # the loop: bit for bit a direct world_map_localize from T_start, and the restatement's to 1e-9
        Pd, Qd, est = c.world_map_localize(s, [case[0]], np.eye(4), start[0][None], start[1][None], opts.localize)
        assert same(P, Pd) and same(Q, Qd) and i.est.outer_iterations == est[0].outer_iterations == loop[2]
        assert i.est.n_surf_feat == len(case[3]) and i.est.n_corner_feat == 2 + 3 * s
        print("slot %d: device - restatement %.3e %.3e" % (s, np.abs(P[0] - loop[0]).max(), np.abs(Q[0] - loop[1]).max()))
        assert np.abs(P[0] - loop[0]).max() < 1e-9 and np.abs(Q[0] - loop[1]).max() < 1e-9
        T_end = M.wm_lidar_pose(P[0], Q[0], np.eye(4))
        final = c.world_map_score(s, [case[0]], T_end[None, None], opts.score)[0, 0]
        assert (i.final.score_q, i.final.n_match, i.final.n_scored) == (int(final["score_q"]), int(final["n_match"]), int(final["n_scored"]))
        assert i.final.n_match > len(case[3]) // 2
        singles.append((P, Q, i))
    # count = 2 in one call against one call per slot: the search and the poses, bit for bit
    P2, Q2, info2 = c.world_map_relocalize(0, [cases[0][0], cases[1][0]], np.eye(4), np.stack([seeds[0][0], seeds[1][0]]), np.stack([seeds[0][1], seeds[1][1]]), opts)
    for s in range(2):
        P, Q, i = singles[s]
        assert same(P2[s], P[0]) and same(Q2[s], Q[0])
        assert bytes(info2[s].best) == bytes(i.best) and bytes(info2[s].second) == bytes(i.second) and bytes(info2[s].final) == bytes(i.final)
        assert info2[s].n_hyp_scored == i.n_hyp_scored and list(info2[s].T_start) == list(i.T_start)
        assert info2[s].est.outer_iterations == i.est.outer_iterations
    Pm, Qm, infom = importlib.import_module("multi-modal-loam_amd.odometry").MapLocalizer(c, [cases[0][0], cases[1][0]]).relocalize(
        [0, 1], np.stack([seeds[0][0], seeds[1][0]]), np.stack([seeds[0][1], seeds[1][1]]), opts)
    assert same(Pm, P2) and same(Qm, Q2) and [bytes(a) for a in infom] == [bytes(a) for a in info2]
    assert downloads(c, [0, 1]) == before
