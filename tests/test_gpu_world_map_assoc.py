"""GPU suite for localisation in a surfel map: mml_world_map_export / _import, mml_world_map_associate, mml_world_map_localize
against tests/world_map_assoc_ref.py.  Slots are filled as in tests/test_gpu_world_map_surfel.py (mml_cloud_upload with hand-made
records), the surf stacks through mml_features_upload; leaf 0.5 m, tables of at most a few thousand positions.  Records, src
arrays and counts are compared exactly; the Gram matrix and the smallest singular value to 1e-9 relative (the bound the
association tests of tests/test_gpu_parity.py hold min_singular to), the poses of the loop to 1e-9 (the bound of the mml_estimate
parity test there)."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

import world_map_assoc_ref as A
import world_map_ref as R
import world_map_surfel_ref as S
from test_gpu_world_map import I4, records, ref_add, same, upload

pytestmark = pytest.mark.gpu
LEAF = 0.5
BOX = np.array([2.0, 1.5, 1.0])      # half extents of the room: three pairs of walls


def shift(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def downloads(ctx, maps, surfels=True):
    out = []
    for m in maps:
        out += [a.tobytes() for a in ctx.world_map_download(m, counts=True)]
        if surfels:
            out += [ctx.world_map_moments(m).tobytes(), ctx.world_map_surfels(m).tobytes()]
    return out + [ctx.world_map_size(-1)]


def box_points(rng, n, noise=0.003, centre=(0.3, -0.2, 0.1)):
    """n world points on the inside of the box's six walls"""
    p = rng.uniform(-1, 1, (n, 3)) * BOX
    axis = rng.integers(0, 3, n)
    side = rng.choice([-1.0, 1.0], n)
    p[np.arange(n), axis] = side * BOX[axis] + rng.normal(0, noise, n)
    return p + np.asarray(centre)


def sensor_frame(world, T):
    return ((world - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def wraps(keys, slots):
    """linear probing of the restatement's hash: does a key land below its first position?"""
    tab, wrapped = {}, False
    for k in sorted(keys):
        h = R.hash_position(k, slots)
        p = h
        while p in tab:
            p = (p + 1) & (slots - 1)
        tab[p] = k
        wrapped |= p < h
    return wrapped


def stack(ctx, slot, feats, corners=3):
    ctx.features_upload(slot, 0, np.full((corners, 3), 0.25, np.float32))
    ctx.features_upload(slot, 1, np.asarray(feats, np.float32).reshape(-1, 3))


def check_slot(ctx, O, ref, slot, map, feats, T, o, st):
    exp, esrc, why = A.associate(ref, O, map, feats, T, o)
    got, src = ctx.factors_download(slot, 1)
    assert same(src, esrc), (src[:8], esrc[:8])
    assert same(got, exp), np.argwhere(got.view(np.uint64) != exp.view(np.uint64))[:4]
    assert len(ctx.factors_download(slot, 0)[1]) == 0
    e = A.stats(O, exp)
    assert (st.n_line, st.n_plane, st.n_line_used, st.n_plane_used) == (0, e["n_plane"], 0, e["n_plane_used"])
    assert np.allclose(np.array(st.normal_gram), e["gram"], rtol=1e-9, atol=1e-9)
    assert abs(st.min_singular - e["min_singular"]) < 1e-9 * max(1.0, abs(e["min_singular"])) and st.is_degenerate == e["is_degenerate"]
    return why


@pytest.mark.parametrize("surfels", [True, False])
def test_export_import_round_trip(M, O, surfels):
    f = np.float32
    for seed in range(64):       # voxels chosen so that a probe chain of the restatement's hash wraps at the table's end
        rng = np.random.default_rng(seed)
        ijk = {tuple(int(v) for v in rng.integers(-6, 6, 3)) for _ in range(40)}
        keys = [R.pack(m, *v) for m in (0, 1) for v in ijk]
        if len(keys) <= 96 and wraps(keys, R.table_slots(96)):
            break
    assert wraps(keys, R.table_slots(96)) and R.table_slots(96) == 256
    cen = (np.array(sorted(ijk), f) + f(0.5)) * f(LEAF)
    rec = [records(np.repeat(cen, 6, axis=0) + (rng.random((6 * len(cen), 3), f) - f(0.5)) * f(0.4)) for _ in range(2)]
    more = records(np.concatenate([cen[:10], cen[:5] + f(20.0)]) + f(0.05))
    ctxs = [M.Context(max_scans=3, max_velo_points=512, max_livox_points=512) for _ in range(2)]
    try:
        for c in ctxs:
            for s in range(2):
                upload(c, s, rec[s])
            upload(c, 2, more)
            c.world_map_create(2, LEAF, 96, surfels=surfels)
            c.world_map_add(0, [0, 1], np.stack([I4, shift([0.01, 0.02, 0.03])]))
        c, twin = ctxs
        before = downloads(c, [0, 1], surfels)
        ex = c.world_map_export(0)
        assert (ex["moments"] is not None) == surfels and len(ex["ijk"]) == len(cen) and same(ex["counts"], c.world_map_download(0, counts=True)[1])
        assert sorted(R.pack(0, *v) for v in ex["ijk"].tolist()) == sorted(k for k in keys if k >> 54 == 0)
        # refusals: a voxel that is present; over capacity -- the table stays as it was
        for n, code in ((3, M.MML_ERR_STATE),):
            with pytest.raises(M.MmlError) as e:
                c.world_map_import(0, ex["ijk"][:n], ex["sums"][:n], ex["counts"][:n], None if not surfels else ex["moments"][:n])
            assert e.value.code == code and downloads(c, [0, 1], surfels) == before
        far = np.arange(3 * 60, dtype=np.int32).reshape(60, 3) + 1000
        with pytest.raises(M.MmlError) as e:
            c.world_map_import(1, far, np.ones((60, 4), f), np.ones(60, np.int32), np.ones((60, 12), f) if surfels else None)
        assert e.value.code == M.MML_ERR_CAPACITY and downloads(c, [0, 1], surfels) == before
        for bad in (dict(ijk=[[1 << 17, 0, 0]]), dict(ijk=[[0, -(1 << 17) - 1, 0]]), dict(counts=[0]), dict(ijk=[[5, 5, 5], [5, 5, 5]], rows=2)):
            n = bad.get("rows", 1)
            with pytest.raises(M.MmlError) as e:
                c.world_map_import(0, bad.get("ijk", [[900, 0, 0]]), np.ones((n, 4), f), bad.get("counts", [1] * n), np.ones((n, 12), f) if surfels else None)
            assert e.value.code == M.MML_ERR_INVALID
        with pytest.raises(M.MmlError) as e:     # moments on a plain map, none on a surfel map
            c.world_map_import(0, [[900, 0, 0]], np.ones((1, 4), f), [1], None if surfels else np.ones((1, 12), f))
        assert e.value.code == M.MML_ERR_INVALID and downloads(c, [0, 1], surfels) == before
        c.world_map_reset(0)
        assert c.world_map_size(0) == 0 and c.world_map_size(1) == len(cen)
        c.world_map_import(0, **ex)
        assert downloads(c, [0, 1], surfels) == before
        for x in ctxs:                           # the sums continue from the stored value
            x.world_map_add(2, [0], shift([0.02, 0.0, -0.01]))
        assert downloads(c, [0, 1], surfels) == downloads(twin, [0, 1], surfels) != before
    finally:
        for c in ctxs:
            c.close()


@pytest.fixture(scope="module")
def room(M, O):
    """two surfel maps in one context: the room, and the same voxels with the room turned a little (other planes)"""
    rng = np.random.default_rng(21)
    c = M.Context(max_scans=4, max_velo_points=8192, max_livox_points=8192, max_features=4096)
    ref = S.SurfelMapRef(LEAF)
    c.world_map_create(2, LEAF, 2048, surfels=True)
    poses = [shift([0.2, 0.1, 0.0]), shift([-0.5, 0.3, 0.2])]
    poses[1][:3, :3] = Rsc.from_rotvec([0.0, 0.0, 0.4]).as_matrix()
    tilt = np.eye(4)
    tilt[:3, :3] = Rsc.from_rotvec([0.02, -0.03, 0.01]).as_matrix()
    for s, T in enumerate(poses):
        world = box_points(rng, 9000)
        rec = records(sensor_frame(world, T))
        upload(c, s, rec)
        c.world_map_add(s, [0], T)
        ref_add(ref, 0, rec, T)
        c.world_map_add(s, [1], tilt @ T)
        ref_add(ref, 1, rec, tilt @ T)
    # voxels of 1, 2 and min_points - 1 points, and a blob of low planarity, outside the room
    sparse = np.concatenate([np.repeat([[5.2, 0.2, 0.2]], 1, 0), np.repeat([[5.2, 1.2, 0.2]], 2, 0), np.repeat([[5.2, 2.2, 0.2]], 4, 0)]) + rng.normal(0, 0.01, (7, 3))
    blob = np.array([7.25, 0.25, 0.25]) + rng.uniform(-0.2, 0.2, (60, 3))
    ring = np.array([[0, a, b] for a in (-0.1, 0.0, 0.1) for b in (-0.1, 0.0, 0.1) if a or b])           # 8 points of a flat patch: planarity 1
    edge = np.array([[(R.HALF - 1 + 0.5) * LEAF, 0.2, 0.2], [(-R.HALF + 0.5) * LEAF, 0.2, 0.2]]).repeat(8, 0) + np.tile(ring, (2, 1))
    rec = records(np.concatenate([sparse, blob, edge]).astype(np.float32))
    upload(c, 2, rec)
    c.world_map_add(2, [0], I4)
    ref_add(ref, 0, rec, I4)
    yield c, ref, rng
    c.close()


def scan(rng, n, T):
    return sensor_frame(box_points(rng, n, noise=0.002), T)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_stack_sizes(M, O, room, n):
    c, ref, rng = room
    T = shift([0.1, -0.1, 0.05])
    feats = scan(np.random.default_rng(n), n, T)
    stack(c, 3, feats)
    o = M.wm_assoc_opts(LEAF)
    st = c.world_map_associate(3, [0], T, o)
    why = check_slot(c, O, ref, 3, 0, feats, T, A.options(LEAF), st[0])
    assert n < 63 or why.count("factor") > n // 2


@pytest.mark.parametrize("nb", [0, 1])
def test_three_slots_two_maps_and_the_placed_features(M, O, room, nb):
    c, ref, rng = room
    rng = np.random.default_rng(5 + nb)
    f = np.float32
    before = downloads(c, [0, 1])
    T = np.stack([shift([0.1, -0.1, 0.05]), shift([9.0, 9.0, 9.0]), shift([-0.2, 0.15, 0.0])])
    T[2][:3, :3] = Rsc.from_rotvec([0.01, 0.0, -0.02]).as_matrix()
    wall_x = 0.3 + BOX[0]                                                   # the wall x = 2.3
    placed = np.array([
        [wall_x - 0.004, 0.0, 0.3],                                         # on the voxel face y = 0: the winner may be a neighbour
        [wall_x + 0.001, 0.5, 0.5], [wall_x, -0.5, 0.0],                    # faces in two and three axes
        [5.2, 0.2, 0.3], [5.2, 1.2, 0.3], [5.2, 2.2, 0.3],                  # next to voxels of 1, 2 and min_points - 1 points
        [7.25, 0.25, 0.3],                                                  # next to a voxel of low planarity
        [wall_x - 0.24, 0.3, 0.3], [wall_x - 0.26, 0.3, 0.3],               # |d| just inside and just outside the gate of 0.25
        [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],                             # not finite
        [(R.HALF - 1 + 0.5) * LEAF, 0.2, 0.2], [(-R.HALF + 0.5) * LEAF, 0.2, 0.2],   # neighbours leave the range
        [(R.HALF + 3) * LEAF, 0.0, 0.0],                                    # the feature itself is out of range
    ], np.float64)
    main = np.concatenate([box_points(rng, 700, noise=0.002), placed])
    feats = [sensor_frame(main, T[0]), scan(rng, 100, T[1]), sensor_frame(box_points(rng, 300, noise=0.002), T[2])]
    feats[0][-len(placed):][9:11] = placed[9:11].astype(f)                  # (the non-finite ones as they are)
    for s in range(3):
        stack(c, s, feats[s], corners=s)
    keep = c.factors_download(1, 1)
    o = M.wm_assoc_opts(LEAF, neighbourhood=nb, max_plane_dist=0.25)
    ro = A.options(LEAF, neighbourhood=nb, max_plane_dist=0.25)
    st = c.world_map_associate(0, [1, -1, 0], T, o)
    why0 = check_slot(c, O, ref, 0, 1, feats[0], T[0], ro, st[0])
    check_slot(c, O, ref, 2, 0, feats[2], T[2], ro, st[2])
    got = c.factors_download(1, 1)
    assert same(got[0], keep[0]) and same(got[1], keep[1])                  # the skipped slot is as it was
    assert downloads(c, [0, 1]) == before                                   # the table is only read
    # the same slot against the other map: same voxel indices, other planes
    st = c.world_map_associate(0, [0], T[0], o)
    why = check_slot(c, O, ref, 0, 0, feats[0], T[0], ro, st[0])
    assert why.count("factor") >= len(main) // 2
    tail = why[-len(placed):]
    assert tail[9:11] == ["skipped"] * 2 and tail[13] == "skipped" and tail[7] == "factor" and tail[8] == "distance"
    if nb:
        assert tail[3:6] == ["none"] * 3 and tail[6] == "planarity" and tail[11:13] == ["factor"] * 2
    a, b = A.associate(ref, O, 0, feats[0], T[0], ro)[0], A.associate(ref, O, 1, feats[0], T[0], ro)[0]
    assert len(a) and len(b) and not same(a, b)


def test_localize(M, O, room):
    c, ref, _ = room
    rng = np.random.default_rng(77)
    before = downloads(c, [0, 1])
    truth = shift([0.15, -0.1, 0.05])
    truth[:3, :3] = Rsc.from_rotvec([0.0, 0.0, 0.1]).as_matrix()
    feats = scan(rng, 2000, truth)
    dt, drot = np.array([0.03, -0.02, 0.025]), np.array([0.01, -0.008, 0.012])       # a few centimetres, about a degree
    start = truth.copy()
    start[:3, :3] = truth[:3, :3] @ Rsc.from_rotvec(drot).as_matrix()
    start[:3, 3] += dt
    P0, Q0 = start[:3, 3], Rsc.from_matrix(start[:3, :3]).as_quat()
    by_outer = [2 * LEAF, LEAF, 0.5 * LEAF]
    Pr, Qr, outer, counts, degenerate = A.localize(ref, O, 0, feats, np.eye(4), P0, Q0, LEAF, by_outer)
    assert degenerate == 0 and counts[0] > 1000
    err_t = np.linalg.norm(Pr - truth[:3, 3])
    err_r = (Rsc.from_quat(Qr) * Rsc.from_matrix(truth[:3, :3]).inv()).magnitude()
    assert err_t < 0.1 * np.linalg.norm(dt) and err_r < 0.1 * np.linalg.norm(drot), (err_t, err_r)
    # a second, different scan for slot 1: another pose, another start, the other map
    truth1 = shift([-0.25, 0.2, -0.05])
    truth1[:3, :3] = Rsc.from_rotvec([0.02, -0.03, -0.2]).as_matrix()
    feats1 = scan(rng, 1500, truth1)
    P1, Q1 = truth1[:3, 3] + [-0.02, 0.03, 0.01], (Rsc.from_matrix(truth1[:3, :3]) * Rsc.from_rotvec([-0.01, 0.005, 0.01])).as_quat()
    stack(c, 0, feats, corners=2)
    stack(c, 1, feats1, corners=5)
    opts = M.wm_localize_opts(LEAF)
    P, Q, info = c.world_map_localize(0, [0], np.eye(4), P0[None], Q0[None], opts)
    print("device - restatement:", np.abs(P[0] - Pr).max(), np.abs(Q[0] - Qr).max(), "outer", info[0].outer_iterations, outer, "restatement error", err_t, err_r)
    assert info[0].outer_iterations == outer and info[0].is_degenerate == 0 and info[0].n_surf_feat == len(feats)
    assert len(c.factors_download(0, 1)[1]) == counts[-1]
    assert np.abs(P[0] - Pr).max() < 1e-9 and np.abs(Q[0] - Qr).max() < 1e-9
    import importlib
    Pm, Qm, _ = importlib.import_module("multi-modal-loam_amd.odometry").MapLocalizer(c, 0).localize([0], P0[None], Q0[None])
    assert same(Pm, P) and same(Qm, Q)
    # count = 2 in one call against one call per slot, bit for bit: poses, iteration counts and the factors left in the slots
    Ps, Qs, infos = c.world_map_localize(1, [1], np.eye(4), P1[None], Q1[None], opts)
    single = [c.factors_download(s, 1) for s in (0, 1)]
    assert not same(Ps[0], P[0]) and len(single[1][1]) > 500 and not same(single[0][0], single[1][0])
    P2, Q2, info2 = c.world_map_localize(0, [0, 1], np.eye(4), np.stack([P0, P1]), np.stack([Q0, Q1]), opts)
    assert same(P2[0], P[0]) and same(Q2[0], Q[0]) and same(P2[1], Ps[0]) and same(Q2[1], Qs[0])
    assert [i.outer_iterations for i in info2] == [outer, infos[0].outer_iterations]
    assert [i.n_surf_feat for i in info2] == [len(feats), len(feats1)] and [i.n_corner_feat for i in info2] == [2, 5]
    # (as in mml_estimate, a slot that has converged is associated again, at its final pose, while another slot of the call
    #  iterates on: the factors LEFT in a slot equal the single call's only where the slot ran as long as the call did)
    last = max(i.outer_iterations for i in info2)
    assert any(i.outer_iterations == last for i in info2)
    for s in (0, 1):
        if info2[s].outer_iterations == last:
            both = c.factors_download(s, 1)
            assert same(both[0], single[s][0]) and same(both[1], single[s][1])
    assert downloads(c, [0, 1]) == before


def test_refusals_leave_the_slots_as_they_were(M, O, room):
    c, ref, _ = room
    feats = scan(np.random.default_rng(3), 100, I4)
    stack(c, 0, feats)
    c.world_map_associate(0, [0], I4, M.wm_assoc_opts(LEAF))
    digest = c.slot_digest(0, 2).tobytes()
    P0, Q0 = np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]])
    cases = [(dict(maps=[2]), M.MML_ERR_INVALID), (dict(maps=[-2]), M.MML_ERR_INVALID), (dict(min_points=2), M.MML_ERR_INVALID),
             (dict(max_plane_dist=np.nan), M.MML_ERR_INVALID), (dict(min_planarity=np.inf), M.MML_ERR_INVALID), (dict(neighbourhood=2), M.MML_ERR_INVALID)]
    for over, code in cases:
        maps = over.pop("maps", [0])
        with pytest.raises(M.MmlError) as e:
            c.world_map_associate(0, maps, I4, M.wm_assoc_opts(LEAF, **over))
        assert e.value.code == code, over
        with pytest.raises(M.MmlError) as e:
            c.world_map_localize(0, maps, np.eye(4), P0, Q0, M.wm_localize_opts(LEAF, assoc=M.wm_assoc_opts(LEAF, **{k: v for k, v in over.items() if k != "max_plane_dist"}),
                                                                                   **({"max_plane_dist_by_outer": [1.0, np.nan, 1.0]} if "max_plane_dist" in over else {})))
        assert e.value.code == code, over
    with pytest.raises(M.MmlError) as e:         # the loop takes no skipped slot
        c.world_map_localize(0, [-1], np.eye(4), P0, Q0, M.wm_localize_opts(LEAF))
    assert e.value.code == M.MML_ERR_INVALID
    L = M.lib()
    m = np.zeros(1, np.int32)
    assert L.mml_world_map_associate(c._h, 0, 1, m.ctypes.data, None, None, None) == M.MML_ERR_INVALID
    assert L.mml_world_map_associate(c._h, 0, 1, None, I4.ctypes.data, None, None) == M.MML_ERR_INVALID
    assert c.slot_digest(0, 2).tobytes() == digest
    for kind in ("none", "plain"):               # no world map; a plain one
        x = M.Context(max_scans=1, max_velo_points=256, max_livox_points=256)
        try:
            stack(x, 0, feats)
            if kind == "plain":
                x.world_map_create(1, LEAF, 64)
            d = x.slot_digest(0, 1).tobytes()
            with pytest.raises(M.MmlError) as e:
                x.world_map_associate(0, [0], I4, M.wm_assoc_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE
            with pytest.raises(M.MmlError) as e:
                x.world_map_localize(0, [0], np.eye(4), P0, Q0, M.wm_localize_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and x.slot_digest(0, 1).tobytes() == d
        finally:
            x.close()


def test_slot_without_a_stack_is_refused(M, O, synth):
    """A slot whose down-sampling overflowed max_features holds no stack (its size is the overflow mark): MML_ERR_STATE from the
    call's read-back of the stack sizes, for the whole call, naming the slot; the other slot of the call keeps its factors."""
    c = M.Context(max_scans=2, max_features=64)
    try:
        c.world_map_create(1, LEAF, 64, surfels=True)
        feats = scan(np.random.default_rng(4), 40, I4)
        stack(c, 0, feats)
        c.scan_upload(1, synth.velo_scan(3, n_az=450), synth.livox_scan(3, n=6000))
        c.extract(1, 1)
        c.downsample(1, 1)                                   # far more than 64 features ...
        with pytest.raises(M.MmlError):
            c.features_count(1, 1)                           # ... the overflow mark, not a stack
        c.world_map_associate(0, [0], I4, M.wm_assoc_opts(LEAF))          # slot 0 alone works (an empty map: no factor)
        c.world_map_associate(0, [0, -1], np.stack([I4, I4]), M.wm_assoc_opts(LEAF))   # a skipped slot's stack is not looked at
        digest = c.slot_digest(0, 2).tobytes()
        P, Q = np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
        for first, maps in ((0, [0, 0]), (1, [0])):
            with pytest.raises(M.MmlError) as e:
                c.world_map_associate(first, maps, np.stack([I4] * len(maps)), M.wm_assoc_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and "slot 1" in str(e.value)
            with pytest.raises(M.MmlError) as e:
                c.world_map_localize(first, maps, np.eye(4), P[:len(maps)], Q[:len(maps)], M.wm_localize_opts(LEAF))
            assert e.value.code == M.MML_ERR_STATE and "slot 1" in str(e.value)
            assert c.slot_digest(0, 2).tobytes() == digest
    finally:
        c.close()
