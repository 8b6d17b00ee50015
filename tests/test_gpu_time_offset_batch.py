"""mml_time_offset_search_batch on the device.  The yardstick is the oracle (O.time_offset_search, a kd-tree search and the
reference's loops on the host), per problem and bit for bit -- np.array_equal on nn_d2 and window_error, equal best_window and
lowest_error, the rule of test_time_offset_search_matches_oracle.  Equality with the single call of the same build is asserted
next to it; on its own it would prove nothing, both go through the same kernels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES, SLICED = 30, 500


@pytest.fixture(scope="module")
def clouds(synth):
    """Three Velodyne scans (x, y, z; 28 800 points each) and three Livox clouds (two scans each, 48 000 points), to be cut down."""
    velo = [np.ascontiguousarray(synth.velo_scan(31 + k)[:, :3]) for k in range(3)]
    livox = []
    for k in range(3):
        parts = [synth.livox_scan(31 + 2 * k + j, motion=True) for j in range(2)]
        livox.append(np.concatenate([np.stack([p["x"], p["y"], p["z"]], 1) for p in parts]).astype(np.float32))
    return velo, livox


def tf_matrix(i):
    th = 0.02 * (i + 1)
    return np.array([[np.cos(th), -np.sin(th), 0, 0.05 * i], [np.sin(th), np.cos(th), 0, -0.1], [0, 0, 1, 0.02 * i], [0, 0, 0, 1]], np.float32)


def three_pairs(clouds):
    velo, livox = clouds
    vs = [velo[0][::15], velo[1][3::17], velo[2][5::29]]                      # 1920, 1694, 993 points
    ls = [livox[0][:3000], livox[1][1000:3777], livox[2][::19][:1501]]
    return vs, ls


def same(a, b):
    return (np.array_equal(a["nn_d2"], b["nn_d2"]) and np.array_equal(a["window_error"], b["window_error"]) and
            a["best_window"] == b["best_window"] and a["lowest_error"] == b["lowest_error"])


def assert_same(got, want, what):
    assert np.array_equal(got["nn_d2"], want["nn_d2"]), what
    assert len(got["window_error"]) == len(want["window_error"]), what
    assert np.array_equal(got["window_error"], want["window_error"]), what
    assert got["best_window"] == want["best_window"] and got["lowest_error"] == want["lowest_error"], what


def raw(M, c, n, velo, vo, tf, livox, lo, res, sliced, nn, err, wo, nw, best, low):
    """The C call on the caller's own arrays (None = NULL); returns (code, message)."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = M.lib().mml_time_offset_search_batch(c._h, n, p(velo), p(vo), p(tf), p(livox), p(lo), res, sliced, p(nn), p(err), p(wo), p(nw), p(best), p(low))
    return rc, M.lib().mml_last_error(c._h).decode()


@pytest.mark.parametrize("with_tf", [True, False])
def test_three_problems_match_the_oracle_bit_for_bit(M, O, clouds, with_tf):
    vs, ls = three_pairs(clouds)
    tfs = np.stack([tf_matrix(i) for i in range(3)]) if with_tf else None
    c = M.Context(max_scans=1)
    try:
        batch = c.time_offset_search_batch(vs, ls, RES, SLICED, tfs)
        single = [c.time_offset_search(vs[i], ls[i], RES, SLICED, None if tfs is None else tfs[i]) for i in range(3)]
    finally:
        c.close()
    assert len(batch) == 3
    for i in range(3):
        o = O.time_offset_search(vs[i], ls[i], RES, SLICED, None if tfs is None else tfs[i])
        assert len(o["window_error"]) == (len(ls[i]) - SLICED - 1) // RES + 1 > 0 and o["best_window"] >= 0
        assert_same(batch[i], o, ("oracle", i))
        assert_same(batch[i], single[i], ("single call", i))


def test_edge_problems_inside_one_batch(M, O, clouds):
    velo, livox = clouds
    rng = np.random.default_rng(5)
    dup = velo[1][::113][:200]
    dup = np.concatenate([dup, dup[rng.integers(0, 200, 57)]])               # 257 points, 57 of them duplicates: one 256-lane block and a bit
    assert len(dup) == 257
    far = (livox[0][:1000] + np.float32(500.0)).astype(np.float32)
    vs = [velo[0][:100], velo[0][::15], velo[1][::15], velo[2][777:778], velo[0][:3], dup, velo[2][::15]]
    ls = [np.zeros((0, 3), np.float32), livox[0][:SLICED], livox[1][:SLICED + 1], livox[2][:700], far, livox[1][2000:3000], livox[2][:3000]]
    c = M.Context(max_scans=1)
    try:
        batch = c.time_offset_search_batch(vs, ls, RES, SLICED)
    finally:
        c.close()
    assert len(batch) == 7
    # no Livox point: 0 windows, -1, 1e6
    assert len(batch[0]["nn_d2"]) == 0 and len(batch[0]["window_error"]) == 0 and batch[0]["best_window"] == -1 and batch[0]["lowest_error"] == 1e6
    want = [None] + [O.time_offset_search(vs[i], ls[i], RES, SLICED) for i in range(1, 7)]
    for i in range(1, 7):
        assert_same(batch[i], want[i], i)
    # n_livox == sliced_points: no window, the distances still filled; one point more: exactly one window
    assert len(batch[1]["window_error"]) == 0 and batch[1]["best_window"] == -1 and len(batch[1]["nn_d2"]) == SLICED and np.all(batch[1]["nn_d2"] > 0)
    assert len(batch[2]["window_error"]) == 1 and batch[2]["best_window"] == 0 and batch[2]["lowest_error"] == batch[2]["window_error"][0]
    assert len(batch[3]["window_error"]) == (700 - SLICED - 1) // RES + 1
    # every window of the far problem is above the 1e6 start value
    assert len(batch[4]["window_error"]) == (1000 - SLICED - 1) // RES + 1 and np.all(batch[4]["window_error"] > 1e6)
    assert batch[4]["best_window"] == -1 and batch[4]["lowest_error"] == 1e6
    assert batch[6]["best_window"] >= 0 and len(batch[6]["window_error"]) == (3000 - SLICED - 1) // RES + 1


def test_problems_are_independent_of_their_place_in_the_batch(M, O, clouds):
    velo, livox = clouds
    vs, ls = [], []
    for i in range(70):                                                      # 70 distinct cuts: more problems than a wavefront has lanes
        v = velo[i % 3][i % 11::15 + (i % 7)]
        l = livox[(i + 1) % 3][37 * i:37 * i + 600 + 31 * (i % 9)]
        vs.append(v[:2000])
        ls.append(l)
    tfs = np.stack([tf_matrix(i % 5) for i in range(70)])
    c = M.Context(max_scans=1)
    try:
        batch = c.time_offset_search_batch(vs, ls, RES, SLICED, tfs)
        rev = c.time_offset_search_batch(vs[::-1], ls[::-1], RES, SLICED, tfs[::-1])[::-1]
        alone = [c.time_offset_search_batch([vs[i]], [ls[i]], RES, SLICED, tfs[i:i + 1])[0] for i in range(70)]
    finally:
        c.close()
    assert len(batch) == 70 and len(set(r["nn_d2"].tobytes() for r in batch)) == 70
    for i in range(70):
        assert len(batch[i]["window_error"]) == (len(ls[i]) - SLICED - 1) // RES + 1 > 0
        assert_same(rev[i], batch[i], ("reversed", i))
        assert_same(alone[i], batch[i], ("alone", i))
    for i in (0, 33, 64, 69):                                                # (the yardstick, on a few of them: lanes 0, 33 and beyond 63)
        assert_same(batch[i], O.time_offset_search(vs[i], ls[i], RES, SLICED, tfs[i]), ("oracle", i))


def test_window_error_capacity_is_per_problem(M, O, clouds):
    vs, ls = three_pairs(clouds)
    velo, vo, livox, lo, _ = M.time_offset_pack(vs, ls)
    nwin = M.time_offset_plan(vo, lo, RES, SLICED)[2]
    room = nwin.copy()
    room[1:] -= 2                                                            # problems 1 and 2 get room for two windows fewer than they have
    wo = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    err = np.full(int(wo[-1]) + 4, -7.5)
    nn = np.zeros(len(livox), np.float32)
    nw, best, low = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3)
    c = M.Context(max_scans=1)
    try:
        rc, msg = raw(M, c, 3, velo, vo, None, livox, lo, RES, SLICED, nn, err, wo, nw, best, low)
    finally:
        c.close()
    assert rc == M.MML_OK, msg
    assert np.all(err[wo[-1]:] == -7.5)                                      # problem 2's surplus: nothing behind its room
    for i in range(3):
        o = O.time_offset_search(vs[i], ls[i], RES, SLICED)
        assert nw[i] == nwin[i] == len(o["window_error"])                    # all windows counted and searched ...
        assert best[i] == o["best_window"] and low[i] == o["lowest_error"]
        assert np.array_equal(err[wo[i]:wo[i + 1]], o["window_error"][:room[i]])   # ... problem 1's surplus not written: problem 2 starts right behind
        assert np.array_equal(nn[lo[i]:lo[i + 1]], o["nn_d2"])


def test_refusals_write_nothing(M, clouds):
    vs, ls = three_pairs(clouds)
    velo, vo, livox, lo, _ = M.time_offset_pack(vs, ls)
    wo = np.concatenate([[0], np.cumsum(M.time_offset_plan(vo, lo, RES, SLICED)[2])]).astype(np.int64)
    big = np.zeros(M.TOFS_BATCH_MAX + 2, np.int32)
    bigw = np.zeros(M.TOFS_BATCH_MAX + 2, np.int64)
    dec = vo.copy()
    dec[2] = dec[1] - 1
    no_velo = vo.copy()
    no_velo[2] = no_velo[1]                                                  # problem 1: Livox points, no Velodyne point
    inv, cap = M.MML_ERR_INVALID, M.MML_ERR_CAPACITY
    cases = [("n = 0", 0, vo, lo, wo, True, inv, "n = 0"), ("n above the maximum", M.TOFS_BATCH_MAX + 1, big, big, bigw, True, inv, "n = 65536"),
             ("decreasing offsets", 3, dec, lo, wo, True, inv, "problem 1"), ("NULL n_windows", 3, vo, lo, wo, False, inv, "null"),
             ("no Velodyne point", 3, no_velo, lo, wo, True, inv, "problem 1")]
    c = M.Context(max_scans=1)
    small = M.Context(max_scans=1, max_map_points=len(vs[0]) - 1)            # problem 0's cloud is one point too large for it
    try:
        for what, n, v_off, l_off, w_off, with_nw, code, text in cases + [("above max_map_points", 3, vo, lo, wo, True, cap, "problem 0")]:
            ctx = small if code == cap else c
            nn, err = np.full(len(livox), -7.5, np.float32), np.full(int(wo[-1]), -7.5)
            nw, best, low = np.full(3, -9, np.int32), np.full(3, -9, np.int32), np.full(3, -7.5)
            rc, msg = raw(M, ctx, n, velo, v_off, None, livox, l_off, RES, SLICED, nn, err, w_off, nw if with_nw else None, best, low)
            assert rc == code, (what, rc, msg)
            assert "mml_time_offset_search_batch" in msg and text in msg, (what, msg)
            assert np.all(nn == -7.5) and np.all(err == -7.5) and np.all(nw == -9) and np.all(best == -9) and np.all(low == -7.5), what
        # the context is as good as before
        assert len(c.time_offset_search_batch(vs, ls, RES, SLICED)) == 3
    finally:
        c.close()
        small.close()


def test_scratch_life_cycle_and_host_synchronisations(M, O, clouds):
    """A large batch, a small one, the single call, on two contexts: the block only grows and every result stays what the oracle
    says.  With profiling on, each call shows ONE launch of each of its two phases -- the two host synchronisations -- whatever n."""
    velo, livox = clouds
    vs, ls = three_pairs(clouds)
    many_v = [velo[i % 3][i::40][:700] for i in range(24)]
    many_l = [livox[i % 3][50 * i:50 * i + 900] for i in range(24)]
    want = [O.time_offset_search(vs[i], ls[i], RES, SLICED) for i in range(3)]
    want_many = {i: O.time_offset_search(many_v[i], many_l[i], RES, SLICED) for i in (0, 23)}
    ctxs = [M.Context(max_scans=1), M.Context(max_scans=1)]
    try:
        for c in ctxs:
            c.profile_enable(True)
            c.profile_reset()
            large = c.time_offset_search_batch(many_v, many_l, RES, SLICED)
            prof = c.profile_get()
            assert prof["tofs_box"][1] == 1 and prof["tofs_search"][1] == 1, prof
            small = c.time_offset_search_batch(vs[:2], ls[:2], RES, SLICED)
            single = c.time_offset_search(vs[2], ls[2], RES, SLICED)
            prof = c.profile_get()
            assert prof["tofs_box"][1] == 3 and prof["tofs_search"][1] == 3, prof   # 24, 2 and 1 problems: one of each per call
            for i in (0, 23):
                assert_same(large[i], want_many[i], ("large", i))
            assert_same(small[0], want[0], "small 0")
            assert_same(small[1], want[1], "small 1")
            assert_same(single, want[2], "the single call after a batch")
            again = c.time_offset_search_batch(many_v, many_l, RES, SLICED)
            assert all(same(a, b) for a, b in zip(again, large))
    finally:
        for c in ctxs:
            c.close()
