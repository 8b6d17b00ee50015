"""Map banks (include/mmloam_hip.h, "map banks"): N further local maps per context, every slot matched against its own.

Everything here is bit-equality: a bound slot's factor records, poses and maps against the same call on a context whose OWN map
holds the bank's cloud and that has no binding.  The banked kernels run the arithmetic of the unbanked ones in the same order
(one template, csrc/map_assoc.hip), so no tolerance is needed and none is used.

Small-batch threshold: mml_launch_associate takes the small-batch form (`fresh_all`: every feature goes straight to the 64- /
32-lane far-query kernel) for count <= 8 (csrc/map_assoc.hip, `P.fresh_all = count <= 8`; the entry points in capi.hip pass
their count through); 6 slots are below it, 12 above."""
import importlib
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from conftest import perturbed, pose_to_x

pytestmark = pytest.mark.gpu

BIND = [1, -1, 0, 2, 1, 0]   # the interleaved bindings of the issue: bank 2 stays empty, -1 is the context's own map
MM = 1 << 19                 # max_map_points of the contexts here: the maps hold a few thousand points, a full ring 50 stacks
EMPTY = np.zeros((0, 3), np.float32)


def _maps(scene):
    """map id -> (corner cloud, surf cloud): banks 0, 1, 2 (empty) and the context's own (-1), all different in size and extent."""
    cm, sm = scene["corner_map"], scene["surf_map"]
    half_c, half_s = cm[cm[:, 0] < np.median(cm[:, 0]) + 2.0][::2], sm[sm[:, 0] < np.median(sm[:, 0]) + 2.0][::2]
    own_c, own_s = cm[1::3] + np.float32(0.03), sm[::3] - np.float32(0.02)
    maps = {0: (cm, sm), 1: (half_c, half_s), 2: (EMPTY, EMPTY), -1: (own_c, own_s)}
    sizes = [len(m[0]) for m in maps.values()]
    assert len(set(sizes)) == 4 and len(half_c) > 20 and len(half_s) > 100
    return maps


def _poses(scene, n):
    fr = scene["frames"]
    return [perturbed(fr[i % 4]["T_gt"], dt=(0.03 - 0.01 * i, -0.02, 0.01 * (i % 3)), rotvec=(0.002, -0.001 * i, 0.004)) for i in range(n)]


def _load_features(c, scene, n):
    for s in range(n):
        fr = scene["frames"][s % 4]
        c.features_upload(s, 0, fr["corner"])
        c.features_upload(s, 1, fr["surf"])


def _records(c, s):
    gl, glsrc = c.factors_download(s, 0)
    gp, gpsrc = c.factors_download(s, 1)
    return gl.tobytes(), glsrc.tobytes(), gp.tobytes(), gpsrc.tobytes()


def _banked_ctx(M, maps, n_slots, bind):
    c = M.Context(max_scans=n_slots, max_map_points=MM)
    c.map_banks(3)
    for b in (0, 1):
        c.bank_set_local(b, 0, maps[b][0])
        c.bank_set_local(b, 1, maps[b][1])
    c.map_set_local(0, maps[-1][0])
    c.map_set_local(1, maps[-1][1])
    c.bind_banks(0, bind)
    assert list(c.slot_banks(0, n_slots)) == list(bind)
    return c


@pytest.fixture(scope="module")
def maps(scene):
    return _maps(scene)


@pytest.fixture(scope="module")
def reference(M, scene, maps):
    """For 6 and 12 slots: the factor records and far-query counts of every slot against every map, from a context without banks
    whose own map is set to that cloud.  Computed once, read by the tests, never changed."""
    out = {}
    c = M.Context(max_scans=12, max_map_points=MM)
    try:
        for n in (6, 12):
            _load_features(c, scene, n)
            T = np.stack(_poses(scene, n))
            for mid, (cm, sm) in maps.items():
                c.map_set_local(0, cm)
                c.map_set_local(1, sm)
                c.associate(0, n, T, 25.0)
                out[(n, mid, "far")] = c.associate_far_count()
                for s in range(n):
                    out[(n, mid, s)] = _records(c, s)
    finally:
        c.close()
    return out


@pytest.mark.parametrize("n", [6, 12])
def test_association_bit_identical_per_bank(M, scene, maps, reference, n):
    """Test 1: both launch forms (6 slots: small-batch; 12: pass 1 + far queue), interleaved bindings, one empty bank."""
    assert reference[(12, 0, "far")] > 0, "the large map alone sends no query to the far queue at 12 slots"
    bind = BIND * (n // 6)
    c = _banked_ctx(M, maps, n, bind)
    try:
        _load_features(c, scene, n)
        c.associate(0, n, np.stack(_poses(scene, n)), 25.0)
        assert c.associate_far_count() > 0
        for s in range(n):
            assert _records(c, s) == reference[(n, bind[s], s)], "slot %d (bank %d) of %d" % (s, bind[s], n)
        empty = [s for s in range(n) if bind[s] == 2]
        for s in empty:                                   # an empty bank: no feature gets a factor
            assert len(c.factors_download(s, 0)[1]) == 0 and len(c.factors_download(s, 1)[1]) == 0
        # the bindings persist: a second call, now over a sub-range that starts at a bound slot
        c.associate(2, 3, np.stack(_poses(scene, n))[2:5], 25.0)
        for s in (2, 3, 4):
            assert _records(c, s) == reference[(n, bind[s], s)]
    finally:
        c.close()


def _estimate_case(M, scene, maps):
    """Test 2 on the current environment: mml_estimate over the six bound slots against six single-map runs."""
    n = 6
    T = _poses(scene, n)
    P = np.stack([t[:3, 3] for t in T])
    Q = np.stack([Rsc.from_matrix(t[:3, :3]).as_quat() for t in T])
    c = _banked_ctx(M, maps, n, BIND)
    r = M.Context(max_scans=n, max_map_points=MM)
    try:
        assert n <= c.device_info()[1]                    # count <= CU count: the packed call (k_solve_wide unless MML_SOLVE_WIDE=0)
        _load_features(c, scene, n)
        _load_features(r, scene, n)
        Pb, Qb, ib = c.estimate(0, n, np.eye(4), P, Q)
        Tb = np.stack([np.eye(4)] * n)
        for s in range(n):
            Tb[s, :3, :3], Tb[s, :3, 3] = Rsc.from_quat(Qb[s]).as_matrix(), Pb[s]
        sb = c.associate(0, n, Tb, 1.0)
        for s in range(n):
            r.map_set_local(0, maps[BIND[s]][0])
            r.map_set_local(1, maps[BIND[s]][1])
            Pr, Qr, ir = r.estimate(s, 1, np.eye(4), P[s][None], Q[s][None])
            assert Pr[0].tobytes() == Pb[s].tobytes() and Qr[0].tobytes() == Qb[s].tobytes(), "slot %d (bank %d)" % (s, BIND[s])
            assert (ir[0].outer_iterations, ir[0].is_degenerate, ir[0].n_corner_feat, ir[0].n_surf_feat) == \
                (ib[s].outer_iterations, ib[s].is_degenerate, ib[s].n_corner_feat, ib[s].n_surf_feat)
            sr = r.associate(s, 1, Tb[s][None], 1.0)[0]
            assert np.float64(sr.min_singular).tobytes() == np.float64(sb[s].min_singular).tobytes()
            assert (sr.n_line, sr.n_plane, sr.is_degenerate) == (sb[s].n_line, sb[s].n_plane, sb[s].is_degenerate)
        assert any(i.outer_iterations > 1 for i in ib)
    finally:
        c.close()
        r.close()


def test_estimate_bit_identical(M, scene, maps):
    _estimate_case(M, scene, maps)


def test_estimate_bit_identical_narrow_solve(M, scene, maps):
    """The same in contexts created with MML_SOLVE_WIDE=0 (the one-frame solve through k_solve<true>)."""
    old = os.environ.get("MML_SOLVE_WIDE")
    os.environ["MML_SOLVE_WIDE"] = "0"
    try:
        _estimate_case(M, scene, maps)
    finally:
        if old is None:
            del os.environ["MML_SOLVE_WIDE"]
        else:
            os.environ["MML_SOLVE_WIDE"] = old


def test_upkeep_ring_wrap_bit_identical(M, scene, synth, maps):
    """Test 3: 52 increments on bank 0 (the ring wraps at 50) against mml_map_increment_local; bank 1 untouched."""
    c = M.Context(max_scans=4, max_map_points=MM)
    r = M.Context(max_scans=4, max_map_points=MM)
    try:
        c.map_banks(2)
        c.bank_set_local(1, 0, maps[1][0])
        c.bank_set_local(1, 1, maps[1][1])
        before = (c.bank_download(1, 0).tobytes(), c.bank_download(1, 1).tobytes())
        for x in (c, r):
            _load_features(x, scene, 4)
        for i in range(1, 53):
            T = synth.pose_matrix(3 * i)
            s = i % 4
            nb = c.bank_increment([0], [s], T[None])
            nr = r.map_increment_local(s, T)
            assert (int(nb[0][0]), int(nb[1][0])) == nr
            if i in (1, 2, 50, 51, 52):
                for kind in (0, 1):
                    got, want = c.bank_download(0, kind), r.map_local_download(kind)
                    assert len(want) > 0 and got.tobytes() == want.tobytes(), "increment %d, kind %d" % (i, kind)
        assert (c.bank_download(1, 0).tobytes(), c.bank_download(1, 1).tobytes()) == before
        # the bank is what a bound slot is matched against
        c.bind_banks(0, [0])
        r.map_set_local(0, r.map_local_download(0))
        r.map_set_local(1, r.map_local_download(1))
        T = synth.pose_matrix(150)[None]
        c.associate(0, 1, T, 25.0)
        r.associate(0, 1, T, 25.0)
        assert _records(c, 0) == _records(r, 0)
        # reset empties the ring, not the map; two banks from two slots in one call
        c.bank_reset(0)
        r.map_local_reset()
        nb = c.bank_increment([1, 0], [2, 3], np.stack([synth.pose_matrix(1), synth.pose_matrix(2)]))
        nr = r.map_increment_local(3, synth.pose_matrix(2))
        assert (int(nb[0][1]), int(nb[1][1])) == nr
        assert c.bank_download(0, 1).tobytes() == r.map_local_download(1).tobytes()
    finally:
        c.close()
        r.close()


def test_unbound_slots_are_isolated(M, scene, synth):
    """Test 4: bindings set and cleared again: mml_step on unbound slots leaves the digests of a context that never had banks."""
    n = 3
    fr = scene["frames"]
    x0 = np.stack([pose_to_x(perturbed(fr[s]["T_gt"])) for s in range(n)])
    dR, dt = np.tile(np.eye(3).reshape(1, 9), (n, 1)), np.zeros((n, 3))
    dig = []
    for banked in (True, False):
        c = M.Context(max_scans=n, max_map_points=MM)
        try:
            c.map_set_local(0, scene["corner_map"])
            c.map_set_local(1, scene["surf_map"])
            if banked:
                c.map_banks(2)
                c.bank_set_local(0, 0, scene["corner_map"][::2])
                c.bank_set_local(0, 1, scene["surf_map"][::2])
                c.bind_banks(0, [0, 1, 0])
                c.bind_banks(0, [-1, -1, -1])
                assert list(c.slot_banks(0, n)) == [-1] * n
            for s in range(n):
                c.scan_upload(s, fr[s]["velo"], fr[s]["livox"])
            x = c.step(0, n, dR, dt, np.eye(4), 25.0, 4, x0)
            dig.append((c.slot_digest(0, n).tobytes(), x.tobytes()))
        finally:
            c.close()
    assert dig[0] == dig[1]


def _sequence_inputs(synth, w, rounds):
    """Scans, sweep motions and predicted poses of sequence w: its own trajectory; sequence 2 starts with two tiny scans, whose
    local map stays below the gate of Estimator.cpp:1032-1035."""
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


def test_lockstep_replay_bit_identical(M, synth):
    """Test 5: three sequences of six scans through BatchLidarOdometry against a LidarOdometry alone on a fresh context each."""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    W, rounds = 3, 6
    inputs = [_sequence_inputs(synth, w, rounds) for w in range(W)]
    alone, gated = [], []
    for w in range(W):
        c = M.Context(max_scans=1, max_map_points=MM)
        try:
            odo = odometry.LidarOdometry(c, lidar_mode=2)
            poses, skipped = [], 0
            for v, l, dR, dt, P, Q in inputs[w]:
                c.scan_upload(0, v, l)
                c.extract(0, 1)
                c.undistort(0, 1, dR.reshape(1, 9), dt.reshape(1, 3))
                skipped += 0 if (odo.n_corner_local > 0 and odo.n_surf_local > 100) else 1
                Pg, Qg, grew = odo.estimate_lidar_pose(0, P, Q)
                poses.append((Pg.tobytes(), Qg.tobytes(), grew))
            alone.append((poses, odo.key_scans, odo.last_T.tobytes()))
            gated.append(skipped)
        finally:
            c.close()
    assert gated[0] == 1 and gated[1] == 1 and gated[2] >= 2, gated     # sequence 2: its first scans fail the local-map gate
    assert all(a[1] >= 2 for a in alone)
    c = M.Context(max_scans=W, max_map_points=MM)
    try:
        bat = odometry.BatchLidarOdometry(c, W, lidar_mode=2)
        for i in range(rounds):
            for w in range(W):
                c.scan_upload(w, inputs[w][i][0], inputs[w][i][1])
            c.extract(0, W)
            c.undistort(0, W, np.stack([inputs[w][i][2].reshape(9) for w in range(W)]), np.stack([inputs[w][i][3] for w in range(W)]))
            P, Q, grew = bat.estimate_lidar_pose(list(range(W)), np.stack([inputs[w][i][4] for w in range(W)]),
                                                 np.stack([inputs[w][i][5] for w in range(W)]))
            for w in range(W):
                assert (P[w].tobytes(), Q[w].tobytes(), grew[w]) == alone[w][0][i], "sequence %d, scan %d" % (w, i)
        assert bat.key_scans == [a[1] for a in alone]
        assert [st.last_T.tobytes() for st in bat.seq] == [a[2] for a in alone]
    finally:
        c.close()


def test_errors_change_nothing(M, scene, cube_scene, maps):
    """Test 6: binding under a global cube map, a bank out of range, a bank twice in one increment: an error code, a message,
    and nothing changed."""
    n = 6
    c = _banked_ctx(M, maps, n, BIND)
    try:
        _load_features(c, scene, n)
        c.associate(0, n, np.stack(_poses(scene, n)), 25.0)

        def state():
            return (c.slot_digest(0, n).tobytes(), c.slot_banks(0, n).tobytes(), c.bank_download(0, 0).tobytes(), c.bank_download(0, 1).tobytes(),
                    c.bank_download(1, 1).tobytes())

        def refused(code, call):
            before = state()
            with pytest.raises(M.MmlError) as e:
                call()
            assert e.value.code == code and len(M.lib().mml_last_error(c._h)) > 0
            assert state() == before

        refused(M.MML_ERR_INVALID, lambda: c.bind_banks(0, [0, 3]))                    # banks 0 .. 2 exist
        refused(M.MML_ERR_INVALID, lambda: c.bind_banks(0, [-2]))
        refused(M.MML_ERR_INVALID, lambda: c.bank_set_local(3, 0, maps[0][0]))
        T2 = np.stack([np.eye(4)] * 2)
        refused(M.MML_ERR_INVALID, lambda: c.bank_increment([1, 1], [0, 1], T2))       # a bank twice
        refused(M.MML_ERR_INVALID, lambda: c.bank_increment([0, 5], [0, 1], T2))
        refused(M.MML_ERR_INVALID, lambda: c.bank_increment([0, 1], [0, n], T2))       # slot out of range, bank 0 not grown either
        # a global cube map: bound slots cannot be associated, no slot can be bound; unbound slots go on as before
        for kind, name in ((0, "corner"), (1, "surf")):
            c.map_set_global(kind, cube_scene[name + "_global"], cube_scene[name + "_cube"])
        refused(M.MML_ERR_STATE, lambda: c.associate(0, n, np.stack(_poses(scene, n)), 25.0))
        refused(M.MML_ERR_STATE, lambda: c.estimate(0, 1, np.eye(4), np.zeros((1, 3)), np.array([[0.0, 0, 0, 1]])))
        refused(M.MML_ERR_STATE, lambda: c.bind_banks(1, [2]))
        c.associate(1, 1, np.stack(_poses(scene, n))[1:2], 25.0)                       # slot 1 is unbound
        c.bind_banks(0, [-1])                                                          # unbinding is always possible
        assert list(c.slot_banks(0, 2)) == [-1, -1]
        for kind in (0, 1):
            c.map_set_global(kind, EMPTY, np.zeros(0, np.int32))
        c.bind_banks(0, [1])
        c.associate(0, n, np.stack(_poses(scene, n)), 25.0)
    finally:
        c.close()


WINDOW = 50                  # MML_LOCAL_WINDOW (csrc/mml_internal.h): the ring wraps at the 51st increment


def _code(M, call):
    with pytest.raises(M.MmlError) as e:
        call()
    return e.value.code


def test_own_map_and_bank_are_the_same_code(M, scene, synth, maps):
    """The context's own map and bank 0 from the same inputs: equal bytes after set_local, and equal sizes and bytes after every
    one of WINDOW + 1 increments from the same slot and pose (the ring wraps at the last)."""
    cm, sm = maps[1][0][:400], maps[1][1][:900]
    fr = scene["frames"][0]
    c = M.Context(max_scans=2, max_map_points=MM)
    try:
        c.map_banks(1)
        for kind, xyz in ((0, cm), (1, sm)):
            c.map_set_local(kind, xyz)
            c.bank_set_local(0, kind, xyz)
            own = c.map_local_download(kind)
            assert len(own) == len(xyz) and own.tobytes() == c.bank_download(0, kind).tobytes()
        c.features_upload(1, 0, fr["corner"][:300])
        c.features_upload(1, 1, fr["surf"][:700])
        for i in range(WINDOW + 1):
            T = synth.pose_matrix(3 * i + 1)
            n_own = c.map_increment_local(1, T)
            nb = c.bank_increment([0], [1], T[None])
            assert n_own == (int(nb[0][0]), int(nb[1][0])) and min(n_own) > 0, i
            for kind in (0, 1):
                own = c.map_local_download(kind)
                assert len(own) == n_own[kind] and own.tobytes() == c.bank_download(0, kind).tobytes(), (i, kind)
    finally:
        c.close()


def test_fresh_own_map_is_unset_and_fresh_bank_is_empty(M, scene):
    """The two defaults: a context's own map refuses until both kinds are set; a bank that was never set is an empty map."""
    c = M.Context(max_scans=2, max_map_points=MM)
    try:
        _load_features(c, scene, 2)
        T = np.stack(_poses(scene, 2))
        for own_call in (lambda: c.associate(0, 1, T[:1], 25.0), lambda: c.knn5(0, np.zeros((1, 3))), lambda: c.knn5(1, np.zeros((1, 3))),
                         lambda: c.map_local_download(0), lambda: c.map_local_download(1)):
            assert _code(M, own_call) == M.MML_ERR_STATE
        c.map_banks(1)
        for kind in (0, 1):
            assert c.bank_download(0, kind).shape == (0, 3)
        c.bind_banks(0, [0])
        c.associate(0, 1, T[:1], 25.0)
        assert len(c.factors_download(0, 0)[1]) == 0 and len(c.factors_download(0, 1)[1]) == 0
        assert _code(M, lambda: c.associate(1, 1, T[1:], 25.0)) == M.MML_ERR_STATE      # slot 1 is unbound: the own map is still unset
        assert _code(M, lambda: c.map_local_download(0)) == M.MML_ERR_STATE
    finally:
        c.close()


def test_context_with_banks_twice_in_one_process(M, scene, synth):
    """Create, use and close a context with banks, twice: one increment of the own map and one of bank 0 (the rings' first
    allocation), a refused call on each, and a clean synchronize."""
    T = synth.pose_matrix(3)
    for _ in range(2):
        c = M.Context(max_scans=2, max_map_points=MM)
        try:
            c.map_banks(1)
            _load_features(c, scene, 2)
            n_own = c.map_increment_local(0, T)
            nb = c.bank_increment([0], [0], T[None])
            assert n_own == (int(nb[0][0]), int(nb[1][0])) and min(n_own) > 0
            assert _code(M, lambda: c.map_increment_local(2, T)) == M.MML_ERR_INVALID          # slots 0, 1 exist
            assert _code(M, lambda: c.bank_increment([1], [0], T[None])) == M.MML_ERR_INVALID  # bank 0 exists
            c.synchronize()
            assert c.map_local_download(1).tobytes() == c.bank_download(0, 1).tobytes()
        finally:
            c.close()
