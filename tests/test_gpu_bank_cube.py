"""A map bank's global cube map (include/mmloam_hip.h, "map banks", CUBE STAGE): its own MAP_MANAGER store, its own match copy,
and the cube stage of the association for bound slots.

Everything here is bit-equality against a context without banks whose OWN maps hold the same clouds.  The banked kernels run the
arithmetic of the unbanked ones in the same order (one template, csrc/map_assoc.hip) and the banks' upkeep is the own store's
code on the bank's state (MmlMapState), so no tolerance is needed and none is used.

Slot counts 6 and 12 lie on either side of `fresh_all = count <= 8` (csrc/map_assoc.hip): both launch forms run."""
import importlib
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from conftest import perturbed, shifted

pytestmark = pytest.mark.gpu

BIND = [1, -1, 0, 2, 1, 0]   # interleaved as in test_gpu_map_banks.py; -1 is the context's own map
MM = 1 << 19
EMPTY = np.zeros((0, 3), np.float32)
NOCUBE = np.zeros(0, np.int32)
GATE = (100, 50)             # a cube is used when it holds more corner / surf points (Estimator.cpp:198, :627)


def _thin_one_cube(xyz, cube, gate):
    """The cloud with one cube that passes the gate cut down to half the gate: that cube falls back to the local map."""
    ids, cnt = np.unique(cube, return_counts=True)
    big = ids[cnt > gate]
    assert len(big) > 0
    victim = big[np.argmax(cnt[cnt > gate])]
    keep = np.ones(len(cube), bool)
    keep[np.flatnonzero(cube == victim)[gate // 2:]] = False
    assert 0 < int(np.sum(cube[keep] == victim)) <= gate
    return xyz[keep], cube[keep]


@pytest.fixture(scope="module")
def maps(cube_scene):
    """map id -> (corner local, surf local, (corner cube cloud, its cube indices) or None, the same for surf): bank 0 the cube
    scene, bank 1 a thinned cube map, bank 2 the local map only, -1 the context's own (a different local cloud, no cube map)."""
    cs = cube_scene
    cl, sl = cs["corner_local"], cs["surf_local"]
    g0 = ((cs["corner_global"], cs["corner_cube"]), (cs["surf_global"], cs["surf_cube"]))
    g1 = (_thin_one_cube(*g0[0], GATE[0]), _thin_one_cube(*g0[1], GATE[1]))
    return {0: (cl, sl, g0), 1: (cl, sl, g1), 2: (cl, sl, None), -1: (cl[1::3] + np.float32(0.03), sl[::3] - np.float32(0.02), None)}


def _poses(cs, n, outside=True):
    """Slots 0 .. 3: the poses of test_two_level_association_matches_oracle (slot 3 moved 600 m out of the cube grid when
    `outside`); further slots: the same frames from other perturbed poses."""
    T = []
    for s in range(n):
        fr = cs["frames"][s % 4]
        P = perturbed(fr["T_gt"]) if s < 4 else perturbed(fr["T_gt"], dt=(0.03 - 0.01 * s, -0.02, 0.01 * (s % 3)), rotvec=(0.002, -0.001 * s, 0.004))
        T.append(shifted(P, cs["shift"]))
    T = np.stack(T)
    if outside and n > 3:
        T[3, :3, 3] += [0.0, 600.0, 0.0]
    return T


def _load_features(c, cs, n, first=0):
    for s in range(n):
        fr = cs["frames"][s % 4]
        c.features_upload(first + s, 0, fr["corner"])
        c.features_upload(first + s, 1, fr["surf"])


def _records(c, s):
    gl, glsrc = c.factors_download(s, 0)
    gp, gpsrc = c.factors_download(s, 1)
    return gl.tobytes(), glsrc.tobytes(), gp.tobytes(), gpsrc.tobytes()


def _set_own(c, m):
    """The context's own maps := map `m` of `maps`."""
    c.map_set_local(0, m[0])
    c.map_set_local(1, m[1])
    for kind in (0, 1):
        if m[2] is None:
            c.map_set_global(kind, EMPTY, NOCUBE)
        else:
            c.map_set_global(kind, m[2][kind][0], m[2][kind][1])


def _banked_ctx(M, maps, n_slots, bind):
    c = M.Context(max_scans=n_slots, max_map_points=MM)
    c.map_banks(3)
    for b in (0, 1, 2):
        c.bank_set_local(b, 0, maps[b][0])
        c.bank_set_local(b, 1, maps[b][1])
        if maps[b][2] is not None:
            for kind in (0, 1):
                c.bank_set_global(b, kind, maps[b][2][kind][0], maps[b][2][kind][1])
    c.map_set_local(0, maps[-1][0])
    c.map_set_local(1, maps[-1][1])
    c.bind_banks(0, bind)
    return c


@pytest.fixture(scope="module")
def reference(M, cube_scene, maps):
    """For 6 and 12 slots: every slot's factor records against every map, from a context without banks whose own maps are set to
    that map's clouds.  Computed once, read by the tests, never changed."""
    out = {}
    c = M.Context(max_scans=12, max_map_points=MM)
    try:
        for n in (6, 12):
            _load_features(c, cube_scene, n)
            T = _poses(cube_scene, n)
            for mid, m in maps.items():
                _set_own(c, m)
                c.associate(0, n, T, 25.0)
                for s in range(n):
                    out[(n, mid, s)] = _records(c, s)
    finally:
        c.close()
    return out


def test_inputs_exercise_both_stages(O, cube_scene, maps):
    """What keeps test 1 honest, on the CPU oracle: over the four frames at these poses more than 100 factors come from the cube
    stage and more than 50 from the local map (the condition test_two_level_association_matches_oracle asserts for them)."""
    cs = cube_scene
    g = maps[0][2]
    gm = [O.CubeMap(g[0][0], g[0][1]), O.CubeMap(g[1][0], g[1][1])]
    tr = [O.KdTree(cs["corner_local"]), O.KdTree(cs["surf_local"])]
    T = _poses(cs, 4)
    tot_g = tot_l = 0
    for k, fr in enumerate(cs["frames"]):
        _, _, lfg = O.associate_lines2(fr["corner"], gm[0], tr[0], T[k], 25.0)
        _, _, pfg = O.associate_planes2(fr["surf"], gm[1], tr[1], T[k], 25.0)
        tot_g += int(lfg.sum() + pfg.sum())
        tot_l += int((1 - lfg).sum() + (1 - pfg).sum())
    assert tot_g > 100 and tot_l > 50


@pytest.mark.parametrize("n", [6, 12])
def test_association_bit_identical_per_bank(M, cube_scene, maps, reference, n):
    """Test 1: both launch forms; a bank with the cube map, one with a cube below the gate, one without, one unbound slot."""
    for kind in (0, 2):   # (records: 0 the line factors, 2 the plane factors) the cube map changes what a slot is matched against
        assert any(reference[(n, 0, s)][kind] != reference[(n, 2, s)][kind] for s in range(n)), "the cube stage changes nothing here"
    assert any(reference[(n, 0, s)] != reference[(n, 1, s)] for s in range(n)), "the thinned cube changes nothing here"
    bind = BIND * (n // 6)
    c = _banked_ctx(M, maps, n, bind)
    try:
        _load_features(c, cube_scene, n)
        T = _poses(cube_scene, n)
        c.associate(0, n, T, 25.0)
        if n == 12:
            assert c.associate_far_count() > 0
        for s in range(n):
            assert _records(c, s) == reference[(n, bind[s], s)], "slot %d (bank %d) of %d" % (s, bind[s], n)
        assert len(c.factors_download(3, 0)[1]) == 0 and len(c.factors_download(3, 1)[1]) == 0   # outside the cube grid
        # the bindings and the cube maps persist: a second call over a sub-range that starts at a bound slot
        c.associate(2, 3, T[2:5], 25.0)
        for s in (2, 3, 4):
            assert _records(c, s) == reference[(n, bind[s], s)]
        # a bank's cube map removed again: that bank is matched against its local map alone
        for kind in (0, 1):
            c.bank_set_global(0, kind, EMPTY, NOCUBE)
        c.associate(0, n, T, 25.0)
        for s in range(n):
            assert _records(c, s) == reference[(n, 2 if bind[s] == 0 else bind[s], s)], "slot %d after the removal" % s
    finally:
        c.close()


def _estimate_case(M, cs, maps):
    n = 6
    T = _poses(cs, n, outside=False)
    P = np.stack([t[:3, 3] for t in T])
    Q = np.stack([Rsc.from_matrix(t[:3, :3]).as_quat() for t in T])
    bind = [1, 2, 0, 2, 1, 0]                             # six bound slots
    c = _banked_ctx(M, maps, n, bind)
    r = M.Context(max_scans=n, max_map_points=MM)
    try:
        _load_features(c, cs, n)
        _load_features(r, cs, n)
        Pb, Qb, ib = c.estimate(0, n, np.eye(4), P, Q)
        for s in range(n):
            _set_own(r, maps[bind[s]])
            Pr, Qr, ir = r.estimate(s, 1, np.eye(4), P[s][None], Q[s][None])
            assert Pr[0].tobytes() == Pb[s].tobytes() and Qr[0].tobytes() == Qb[s].tobytes(), "slot %d (bank %d)" % (s, bind[s])
            assert (ir[0].outer_iterations, ir[0].is_degenerate, ir[0].n_corner_feat, ir[0].n_surf_feat) == \
                (ib[s].outer_iterations, ib[s].is_degenerate, ib[s].n_corner_feat, ib[s].n_surf_feat)
        assert any(i.outer_iterations > 1 for i in ib)
    finally:
        c.close()
        r.close()


def test_estimate_bit_identical(M, cube_scene, maps):
    """Test 2: mml_estimate over six bound slots against six single-context runs."""
    _estimate_case(M, cube_scene, maps)


def test_estimate_bit_identical_narrow_solve(M, cube_scene, maps):
    """The same in contexts created with MML_SOLVE_WIDE=0."""
    old = os.environ.get("MML_SOLVE_WIDE")
    os.environ["MML_SOLVE_WIDE"] = "0"
    try:
        _estimate_case(M, cube_scene, maps)
    finally:
        if old is None:
            del os.environ["MML_SOLVE_WIDE"]
        else:
            os.environ["MML_SOLVE_WIDE"] = old


STEPS = [(k, 1) for k in range(4)] + [(0, 2), (1, 2), ("far", 0), (2, 1), ("gone", 0), (3, 1)]   # test_global_cube_store_matches_oracle
SH = np.array([22.0, 24.0, 0.0])


def _step_inputs(scene, step, k, reps):
    """(T of the increment, [(corner, surf, T) of every append before it]) of one entry of STEPS at position `step`."""
    if k in ("far", "gone"):
        T = np.eye(4)
        T[:3, 3] = [182.0, 24.0, 1.0] if k == "far" else [900.0, -500.0, 1.0]
        return T, []
    fr = scene["frames"][k]
    feats = [(fr["corner"], fr["surf"],
              shifted(perturbed(fr["T_gt"], dt=(0.13 * step + 0.05 * r, -0.07 * step, 0.0), rotvec=(0.0, 0.0, 0.01 * step)), SH)) for r in range(reps)]
    return feats[-1][2], feats


def test_cube_store_upkeep_per_bank(M, scene):
    """Test 3: the step list of test_global_cube_store_matches_oracle into banks 0 and 2, in different orders, against one
    single context per bank with the same history; an association of a bound slot at steps 2, 5 and 7 (the match copy lags one
    increment); bank 1 stays empty."""
    order = {0: STEPS, 2: STEPS[3:] + STEPS[:3]}
    slot = {0: 0, 2: 1}                                   # the slot whose stacks feed the bank
    c = M.Context(max_scans=4, max_map_points=MM)
    ref = {b: M.Context(max_scans=2, max_map_points=MM) for b in (0, 2)}
    loc = (scene["corner_map"] + SH.astype(np.float32), scene["surf_map"] + SH.astype(np.float32))
    try:
        c.map_banks(3)
        for b in (0, 2):
            for kind in (0, 1):
                c.bank_set_local(b, kind, loc[kind])
                ref[b].map_set_local(kind, loc[kind])
        c.bind_banks(2, [0, 2])
        frq = scene["frames"][1]
        Tq = shifted(perturbed(frq["T_gt"]), SH)
        for x, s in ((c, 2), (c, 3), (ref[0], 1), (ref[2], 1)):
            x.features_upload(s, 0, frq["corner"])
            x.features_upload(s, 1, frq["surf"])
        used = False
        for step in range(len(STEPS)):
            inp = {b: _step_inputs(scene, step, *order[b][step]) for b in (0, 2)}
            for r in range(2):                            # the r-th append of every bank that has one: ONE call
                who = [b for b in (0, 2) if len(inp[b][1]) > r]
                for b in who:
                    cf, sf, Tr = inp[b][1][r]
                    for x, s in ((c, slot[b]), (ref[b], 0)):
                        x.features_upload(s, 0, cf)
                        x.features_upload(s, 1, sf)
                    ref[b].map_global_append(0, Tr)
                if who:
                    c.bank_global_append(who, [slot[b] for b in who], np.stack([inp[b][1][r][2] for b in who]))
            nc, ns = c.bank_global_increment([2, 0], np.stack([inp[2][0], inp[0][0]]))
            for i, b in enumerate((2, 0)):
                assert (int(nc[i]), int(ns[i])) == ref[b].map_global_increment(inp[b][0])
                for kind in (0, 1):
                    got, want = c.bank_global_download(b, kind), ref[b].map_global_download(kind)
                    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (step, b, kind)
            for kind in (0, 1):
                assert len(c.bank_global_download(1, kind)[0]) == 0
            if step in (2, 5, 7):
                c.associate(2, 2, np.stack([Tq, Tq]), 1.0)
                for b, s in ((0, 2), (2, 3)):
                    ref[b].associate(1, 1, Tq[None], 1.0)
                    assert _records(c, s) == _records(ref[b], 1), (step, b)
                used = used or _records(c, 2) != _records(c, 3)
        assert used, "the two banks' match copies never made a difference"
        assert len(c.bank_global_download(0, 1)[0]) > 0
        c.bank_global_reset(0)
        assert len(c.bank_global_download(0, 1)[0]) == 0 and len(c.bank_global_download(2, 1)[0]) > 0
    finally:
        c.close()
        for x in ref.values():
            x.close()


def _sequence_inputs(synth, w, rounds):
    """The inputs of test_lockstep_replay_bit_identical (test_gpu_map_banks.py): sequence 2 starts with two tiny scans."""
    out = []
    for i in range(rounds):
        k = (20, 60, 35)[w] + (4, 5, 6)[w] * i
        v, l = synth.velo_scan(k, n_az=450, motion=True), synth.livox_scan(k, n=6000, motion=True)
        if w == 2 and i < 2:
            v, l = v[:16 * 3], l[:600]
        dR, dt = synth.sweep_motion(k)
        Tp = perturbed(synth.pose_matrix(k), dt=(0.02, -0.015, 0.01), rotvec=(0.002, -0.001, 0.003))
        out.append((v, l, dR, dt, Tp[:3, 3].copy(), Rsc.from_matrix(Tp[:3, :3]).as_quat()))
    return out


def _alone(M, odometry, inputs, global_map):
    c = M.Context(max_scans=1, max_map_points=MM)
    try:
        odo = odometry.LidarOdometry(c, lidar_mode=2, global_map=global_map)
        poses, sizes = [], []
        for v, l, dR, dt, P, Q in inputs:
            c.scan_upload(0, v, l)
            c.extract(0, 1)
            c.undistort(0, 1, dR.reshape(1, 9), dt.reshape(1, 3))
            Pg, Qg, grew = odo.estimate_lidar_pose(0, P, Q)
            poses.append((Pg.tobytes(), Qg.tobytes(), grew))
            sizes.append((odo.n_corner_global, odo.n_surf_global))
        return poses, sizes, odo.key_scans, odo.last_T.tobytes()
    finally:
        c.close()


def test_lockstep_replay_with_cube_schedule(M, synth):
    """Test 4: three sequences through BatchLidarOdometry(global_map=True) against a LidarOdometry(global_map=True) alone on a
    fresh context each.  Seven rounds: the increment of round 3 copies a store of two scans into the match copy, so from round 4
    on Estimate has a cube above its gate."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    W, rounds = 3, 7
    inputs = [_sequence_inputs(synth, w, rounds) for w in range(W)]
    alone = [_alone(M, odometry, inputs[w], True) for w in range(W)]
    # some increment before the last round leaves more surf points than the gate asks of ONE cube ...
    assert any(ns > GATE[1] and nc > 0 for a in alone for nc, ns in a[1][:-2])
    # ... and the cube stage is used: sequence 0's poses differ from the loop that drives the local map alone
    local_only = _alone(M, odometry, inputs[0], False)
    assert local_only[0] != alone[0][0] and local_only[0][:2] == alone[0][0][:2]
    c = M.Context(max_scans=W, max_map_points=MM)
    try:
        bat = odometry.BatchLidarOdometry(c, W, lidar_mode=2, global_map=True)
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


def test_errors_change_nothing(M, scene, cube_scene, maps):
    """Test 5: every refusal leaves the banks' stores, the bindings and a bound slot's records as they were."""
    n = 6
    c = _banked_ctx(M, maps, n, BIND)
    try:
        _load_features(c, cube_scene, n)
        T = _poses(cube_scene, n)
        c.bank_global_append([0, 2], [0, 1], T[:2])
        c.bank_global_increment([0, 2], T[:2])
        c.bank_global_append([0], [2], T[2:3])             # (pending points too)
        c.associate(0, n, T, 25.0)

        def state():
            dl = [a.tobytes() for b in (0, 1, 2) for kind in (0, 1) for a in c.bank_global_download(b, kind)]
            return (c.slot_digest(0, n).tobytes(), c.slot_banks(0, n).tobytes(), tuple(dl), _records(c, 2))

        def refused(code, call):
            before = state()
            with pytest.raises(M.MmlError) as e:
                call()
            assert e.value.code == code and len(M.lib().mml_last_error(c._h)) > 0
            assert state() == before

        T2 = T[:2]
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_append([1, 1], [0, 1], T2))            # a bank twice in an append
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_increment([2, 2], T2))                 # a bank twice in an increment
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_append([0, 3], [0, 1], T2))            # a bank out of range
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_increment([0, -1], T2))
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_download(3, 0))
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_reset(3))
        refused(M.MML_ERR_INVALID, lambda: c.bank_set_global(3, 0, maps[0][2][0][0], maps[0][2][0][1]))
        refused(M.MML_ERR_INVALID, lambda: c.bank_global_append([0, 1], [0, n], T2))            # a slot out of range, bank 0 not fed either
        # the context's OWN cube map: no slot can be bound, bound slots cannot be associated
        for kind, name in ((0, "corner"), (1, "surf")):
            c.map_set_global(kind, cube_scene[name + "_global"], cube_scene[name + "_cube"])
        refused(M.MML_ERR_STATE, lambda: c.bind_banks(1, [2]))
        refused(M.MML_ERR_STATE, lambda: c.associate(0, n, T, 25.0))
        for kind in (0, 1):
            c.map_set_global(kind, EMPTY, NOCUBE)
        # the pending clouds are what they were: bank 0's next increment equals that of a context with the accepted history
        r = M.Context(max_scans=n, max_map_points=MM)
        try:
            _load_features(r, cube_scene, n)
            r.map_global_append(0, T[0])
            r.map_global_increment(T[0])
            r.map_global_append(2, T[2])
            want = r.map_global_increment(T[2])
            nc, ns = c.bank_global_increment([0], T[2:3])
            assert (int(nc[0]), int(ns[0])) == want
            for kind in (0, 1):
                assert all(g.tobytes() == w.tobytes() for g, w in zip(c.bank_global_download(0, kind), r.map_global_download(kind)))
        finally:
            r.close()
    finally:
        c.close()


def test_append_without_a_stack_is_refused(M, synth, cube_scene):
    """Test 5, the two STATE cases.  A slot whose down-sampling overflowed max_features holds no stack: the whole append is
    refused and the other bank of the call is not fed.  A context without banks refuses every call."""
    c = M.Context(max_scans=2, max_map_points=MM, max_features=64)
    try:
        T = _poses(cube_scene, 2)
        with pytest.raises(M.MmlError) as e:                                                    # no banks
            c.bank_global_increment([0], T[:1])
        assert e.value.code == M.MML_ERR_STATE
        with pytest.raises(M.MmlError) as e:
            c.bank_global_download(0, 0)
        assert e.value.code == M.MML_ERR_STATE
        c.map_banks(2)
        c.features_upload(0, 0, cube_scene["frames"][0]["corner"][:50])
        c.features_upload(0, 1, cube_scene["frames"][0]["surf"][:60])
        c.scan_upload(1, synth.velo_scan(3, n_az=450), synth.livox_scan(3, n=6000))
        c.extract(1, 1)
        c.downsample(1, 1)                                                                      # far more than 64 features ...
        with pytest.raises(M.MmlError):
            c.features_count(1, 1)                                                              # ... the overflow mark, not a stack
        with pytest.raises(M.MmlError) as e:
            c.bank_global_append([0, 1], [0, 1], T)
        assert e.value.code == M.MML_ERR_STATE and len(M.lib().mml_last_error(c._h)) > 0
        nc, ns = c.bank_global_increment([0, 1], T)
        assert list(nc) == [0, 0] and list(ns) == [0, 0]                                        # nothing was pending in either bank
        c.bank_global_append([0], [0], T[:1])
        nc, ns = c.bank_global_increment([0], T[:1])
        assert (int(nc[0]), int(ns[0])) == (50, 60)
    finally:
        c.close()


def _cube_ctx(M, cs, max_map_points, bank):
    """Two slots, one bank, the cube scene's local map in the own map and in bank 0; slot 0 bound to `bank` (-1: unbound)."""
    c = M.Context(max_scans=2, max_map_points=max_map_points)
    c.map_banks(1)
    for kind, name in ((0, "corner"), (1, "surf")):
        c.map_set_local(kind, cs[name + "_local"])
        c.bank_set_local(0, kind, cs[name + "_local"])
    c.bind_banks(0, [bank])
    _load_features(c, cs, 1)
    return c


def _set_global(c, bank, kind, xyz, cube, cen=None):
    if bank < 0:
        c.map_set_global(kind, xyz, cube, cen)
    else:
        c.bank_set_global(bank, kind, xyz, cube, cen)


def test_own_cube_map_and_bank_are_the_same_code(M, cube_scene):
    """The same cube map in the context's own and in bank 0: equal factor records of a slot matched against either; then one
    append + increment of both stores from the same slot and pose: equal sizes, points, cube indices and centre."""
    cs = cube_scene
    T = _poses(cs, 1)
    c = _cube_ctx(M, cs, MM, -1)
    try:
        rec = {}
        for bank in (-1, 0):
            for kind, name in ((0, "corner"), (1, "surf")):
                _set_global(c, bank, kind, cs[name + "_global"], cs[name + "_cube"], [10, 5, 10])
            c.bind_banks(0, [bank])
            c.associate(0, 1, T, 1.0)
            rec[bank] = _records(c, 0)
            if bank < 0:                                  # the own cube map and a bound slot exclude each other
                for kind in (0, 1):
                    c.map_set_global(kind, EMPTY, NOCUBE)
        assert rec[-1] == rec[0] and len(c.factors_download(0, 1)[1]) > 0
        c.map_global_append(0, T[0])
        c.bank_global_append([0], [0], T)
        n_own = c.map_global_increment(T[0])
        nb = c.bank_global_increment([0], T)
        assert n_own == (int(nb[0][0]), int(nb[1][0])) and min(n_own) > 0
        for kind in (0, 1):
            own, bnk = c.map_global_download(kind), c.bank_global_download(0, kind)
            assert len(own[0]) == n_own[kind] and all(a.tobytes() == b.tobytes() for a, b in zip(own, bnk)), kind
    finally:
        c.close()


@pytest.mark.parametrize("bank", [-1, 0])
def test_refused_set_global_changes_nothing(M, cube_scene, bank):
    """A set_global that is refused -- a cube index of 4851, one point more than max_map_points -- leaves the cube map as it was: a
    slot matched against it gets the factor records it got before.  Cube index 4850 and max_map_points points are accepted."""
    cs = cube_scene
    mm = 1 << 15                                          # max_map_points here: the accepted full-size call stays small
    assert max(len(cs["surf_local"]), len(cs["corner_local"])) <= mm
    T = _poses(cs, 1)
    c = _cube_ctx(M, cs, mm, bank)
    try:
        for kind, name in ((0, "corner"), (1, "surf")):
            _set_global(c, bank, kind, cs[name + "_global"], cs[name + "_cube"])
        c.associate(0, 1, T, 1.0)
        before = _records(c, 0)
        bad = cs["surf_cube"].copy()
        bad[len(bad) // 2] = 4851
        for kind in (0, 1):
            with pytest.raises(M.MmlError) as e:
                _set_global(c, bank, kind, cs["surf_global"], bad, [3, 3, 3])
            assert e.value.code == M.MML_ERR_INVALID
            with pytest.raises(M.MmlError) as e:
                _set_global(c, bank, kind, np.zeros((mm + 1, 3), np.float32), np.zeros(mm + 1, np.int32), [3, 3, 3])
            assert e.value.code == M.MML_ERR_CAPACITY
        c.associate(0, 1, T, 1.0)
        assert _records(c, 0) == before
        xyz = np.random.default_rng(11).uniform(-20.0, 20.0, (mm, 3)).astype(np.float32)
        _set_global(c, bank, 1, xyz, np.full(mm, 4850, np.int32))
        c.associate(0, 1, T, 1.0)
        assert _records(c, 0) != before                   # the records do depend on the cube map
        c.synchronize()
    finally:
        c.close()
