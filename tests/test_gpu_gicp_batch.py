"""mml_gicp_align_batch / mml_gicp_refresh_batch on the device.  The reference of every comparison but the oracle test is the
single call (mml_gicp_align / mml_gicp_refresh) on the same problem, and the comparison is on BYTES -- converged, the 16 floats of T,
the whole mml_gicp_info, the downloaded slots: both sides run the same kernels on the same numbers, so no tolerance is needed
whatever the conditioning of a problem, and none is allowed."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

pytestmark = pytest.mark.gpu


# ---- small synthetic clouds: three perpendicular planes with noise, the source a moved subset ----------------------------
def corner_cloud(rng, n):
    """n points on the planes x = 0, y = 0, z = 0 of a 4 m room corner, 5 mm noise across each plane."""
    p = rng.uniform(0.0, 4.0, (n, 3))
    p[np.arange(n), rng.integers(0, 3, n)] = rng.normal(0.0, 0.005, n)
    return p


def pair(seed, n_src, n_tgt, scale=1.0):
    """(src, tgt) float32: one pool of points, the target its first n_tgt, the source n_src of them in another order, moved by
    scale x (a few cm, a few mrad)."""
    rng = np.random.default_rng(seed)
    pool = corner_cloud(rng, max(n_src, n_tgt, 1))
    tgt = pool[:n_tgt]
    src = pool[rng.permutation(len(pool))[:n_src]]
    R = Rsc.from_euler("xyz", scale * rng.uniform(-4e-3, 4e-3, 3)).as_matrix()
    t = scale * rng.uniform(-0.04, 0.04, 3)
    return ((src - t) @ R).astype(np.float32), tgt.astype(np.float32)


def start_matrix(i):
    """A distinct, recognisable T0 per problem: an alignment that does not run must hand it back untouched."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.25 + i, -0.5 * i, 0.125]
    T[3, :3] = [i, 2.0, -3.0]                                                # (not a rigid motion: nobody may "repair" it)
    return T


def key(res):
    """(converged, T, info) as bytes."""
    ok, T, info = res
    return (bool(ok), np.ascontiguousarray(T, np.float32).tobytes(), bytes(info))


def info_tuple(info):
    return (info.outer_iterations, info.objective_evaluations, info.objective, info.n_source, info.n_target)


EDGE_SIZES = [(20, 20), (19, 40), (40, 19), (0, 40), (21, 257), (257, 256), (513, 300), (300, 1025), (1025, 1025)]


def test_sizes_at_the_kernels_edges_in_one_call(M):
    """k_correspondences = 20 on either side (below it: no alignment, matrix untouched, info zeroed), an empty source, a block
    boundary (256 / 257), EV_CH = 512 (a second chunk of the objective's term table), TILE = 1024 (a second LDS tile of the searches),
    all in one call -- so grid.x is sized by the largest cloud and most problems have blocks that leave at once."""
    pairs = [pair(100 + i, a, b) for i, (a, b) in enumerate(EDGE_SIZES)]
    T0 = np.stack([start_matrix(i) for i in range(len(pairs))])
    c = M.Context(max_scans=1)
    try:
        single = [c.gicp_align(s, t, T0[i]) for i, (s, t) in enumerate(pairs)]
        batch = c.gicp_align_batch(pairs, T0)
        rev = c.gicp_align_batch(pairs[::-1], T0[::-1])[::-1]
    finally:
        c.close()
    for i, (a, b) in enumerate(EDGE_SIZES):
        print(EDGE_SIZES[i], single[i][0], info_tuple(single[i][2]), info_tuple(batch[i][2]))
        assert key(batch[i]) == key(single[i]), EDGE_SIZES[i]
        assert key(rev[i]) == key(batch[i]), EDGE_SIZES[i]
        if a < 20 or b < 20:                                                 # not aligned: as gicp_run leaves it
            assert not batch[i][0] and np.array_equal(batch[i][1], T0[i]) and bytes(batch[i][2]) == bytes(24), EDGE_SIZES[i]
        else:
            assert info_tuple(batch[i][2])[3:] == (a, b) and batch[i][2].outer_iterations >= 1, EDGE_SIZES[i]
    assert sum(r[0] for r in batch) >= 4                                     # the call is not a collection of failures
    assert len({key(r) for r in batch}) == len(batch)


# ---- 300 tiny problems: more workgroups than compute units; shared by the life-cycle test ---------------------------------
@pytest.fixture(scope="module")
def tiny300(M):
    """300 problems of 24 .. 64 points (seeded sizes), displacements from nothing to ten times the usual one so that the
    alignments end after different numbers of outer iterations, and what the single call returns for each."""
    rng = np.random.default_rng(7)
    sizes = rng.integers(24, 65, (300, 2))
    pairs = [pair(1000 + i, int(a), int(b), scale=(0.0, 1.0, 3.0, 10.0)[i % 4]) for i, (a, b) in enumerate(sizes)]
    c = M.Context(max_scans=1)
    try:
        single = [key(c.gicp_align(s, t)) for s, t in pairs]
    finally:
        c.close()
    return dict(pairs=pairs, single=single)


def test_more_problems_than_compute_units(M, tiny300):
    pairs, single = tiny300["pairs"], tiny300["single"]
    assert len({(len(s), len(t)) for s, t in pairs}) > 100
    c = M.Context(max_scans=1)
    try:
        batch = c.gicp_align_batch(pairs)
    finally:
        c.close()
    assert len(batch) == 300
    bad = [i for i in range(300) if key(batch[i]) != single[i]]
    assert not bad, bad[:10]
    iters = sorted({r[2].outer_iterations for r in batch})
    print("outer_iterations in the batch:", iters, " converged:", sum(r[0] for r in batch))
    assert len(iters) >= 2                                                   # finished states skip rounds others still run


def test_batch_of_two_against_the_oracle(M, O, synth):
    """The two well-conditioned pairs of test_gicp_align_matches_oracle (tests/test_gpu_parity.py), built the same way, as one
    batch of two, held to that test's bounds."""
    ev = O.extract_velo(synth.velo_scan(12))
    vs = ev["xyzi"][ev["label"] == 2][:, :3].copy()
    Tt = np.eye(4)
    Tt[:3, :3] = Rsc.from_euler("xyz", [0.01, -0.015, 0.02]).as_matrix()
    Tt[:3, 3] = [0.05, -0.03, 0.02]
    rng = np.random.default_rng(0)
    sub = vs[rng.random(len(vs)) < 0.8]
    src = ((sub.astype(np.float64) - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)
    pairs = [(src, vs), (sub, vs)]
    c = M.Context(max_scans=1)
    try:
        batch = c.gicp_align_batch(pairs)
    finally:
        c.close()
    for (s_, t_), (okg, Tg, info) in zip(pairs, batch):
        oko, To, ito, evo, fo = O.gicp_align(s_, t_)
        print(len(s_), len(t_), np.abs(Tg - To).max(), info_tuple(info), (ito, evo, fo))
        assert okg and oko
        assert np.abs(Tg - To).max() <= 1e-6, np.abs(Tg - To).max()
        assert info.outer_iterations == ito and info.objective_evaluations == evo
        assert abs(info.objective - fo) <= 1e-9 * max(fo, 1e-9) + 1e-15
        assert (info.n_source, info.n_target) == (len(s_), len(t_))


# ---- the refresh of a range of slots --------------------------------------------------------------------------------------
T_START = np.eye(4, dtype=np.float32)
T_START[:3, :3] = Rsc.from_euler("xyz", [0.002, -0.003, 0.004]).as_matrix().astype(np.float32)
T_START[:3, 3] = [0.02, -0.01, 0.03]


@pytest.fixture(scope="module")
def four_scans(synth):
    """slot 0: scan 14; slot 1: the same with 3000 Livox points (livox_corner_num <= 100: skipped); slot 2: scan 15; slot 3:
    Velodyne scan 16 without a Livox part (skipped)."""
    return [(synth.velo_scan(14), synth.livox_scan(14)), (synth.velo_scan(14), synth.livox_scan(14)[:3000]),
            (synth.velo_scan(15), synth.livox_scan(15)), (synth.velo_scan(16), None)]


def extracted_context(M, four_scans):
    c = M.Context(max_scans=4)
    for s, (v, l) in enumerate(four_scans):
        c.scan_upload(s, v, l)
    c.extract(0, 4)                                                           # without an extrinsic
    return c


def slot_bytes(c, slot):
    d = c.scan_download(slot)
    return (d["xyzi"].tobytes(), d["label"].tobytes(), d["reltime"].tobytes(), d["ring"].tobytes())


@pytest.fixture(scope="module")
def chained_reference(M, four_scans):
    """The loop the batch call replaces: gicp_refresh(s, T, apply=True) over one persistent matrix, on its own context."""
    c = extracted_context(M, four_scans)
    try:
        before = [slot_bytes(c, s) for s in range(4)]
        T = T_START.copy()
        refreshed, rows, infos = [], [], []
        for s in range(4):
            ok, T, info = c.gicp_refresh(s, T, apply=True)
            refreshed.append(ok)
            rows.append(T.copy())
            infos.append(bytes(info))
        after = [slot_bytes(c, s) for s in range(4)]
    finally:
        c.close()
    return dict(before=before, refreshed=refreshed, rows=rows, infos=infos, after=after)


def check_against_chain(ref, out, slots_after):
    refreshed, T, infos = out
    assert refreshed.tolist() == ref["refreshed"]
    for s in range(4):
        assert T[s].tobytes() == ref["rows"][s].tobytes(), s
        assert bytes(infos[s]) == ref["infos"][s], s
        assert slots_after[s] == ref["after"][s], s


def test_refresh_batch_chained_and_per_slot(M, four_scans, chained_reference):
    ref = chained_reference
    assert ref["refreshed"] == [True, False, True, False]                    # slots 0 and 2 refreshed; 1 and 3 are skipped
    assert ref["after"][1] == ref["before"][1] and ref["after"][3] == ref["before"][3] and ref["after"][0] != ref["before"][0]
    b = extracted_context(M, four_scans)
    try:
        assert [slot_bytes(b, s) for s in range(4)] == ref["before"]
        out = b.gicp_refresh_batch(0, 4, T_START, chain=True, apply=True)
        check_against_chain(ref, out, [slot_bytes(b, s) for s in range(4)])
        T = out[1]
        assert np.array_equal(T[1], T[0]) and np.array_equal(T[3], T[2])    # a skipped frame keeps the matrix of the frame before it
        assert not np.array_equal(T[0], T_START) and not np.array_equal(T[2], T[0])
    finally:
        b.close()
    # chain = False: a matrix per slot (several robots), against per-slot single calls on a context of their own
    Ts = np.stack([T_START, start_matrix(1), np.eye(4, dtype=np.float32), start_matrix(3)])
    a, b = extracted_context(M, four_scans), extracted_context(M, four_scans)
    try:
        single = [a.gicp_refresh(s, Ts[s], apply=True) for s in range(4)]
        refreshed, T, infos = b.gicp_refresh_batch(0, 4, Ts, chain=False, apply=True)
        for s in range(4):
            assert (bool(refreshed[s]), T[s].tobytes(), bytes(infos[s])) == key(single[s]), s
            assert slot_bytes(b, s) == slot_bytes(a, s), s
        assert np.array_equal(T[1], Ts[1]) and np.array_equal(T[3], Ts[3]) and refreshed.tolist() == [True, False, True, False]
    finally:
        a.close()
        b.close()


def test_apply_false_returns_the_matrices_and_leaves_the_slots(M, four_scans, chained_reference):
    ref = chained_reference
    c = extracted_context(M, four_scans)
    try:
        refreshed, T, infos = c.gicp_refresh_batch(0, 4, T_START, chain=True, apply=False)
        assert [slot_bytes(c, s) for s in range(4)] == ref["before"]
        assert refreshed.tolist() == ref["refreshed"]
        for s in range(4):
            assert T[s].tobytes() == ref["rows"][s].tobytes() and bytes(infos[s]) == ref["infos"][s], s
    finally:
        c.close()


def raw_refresh_batch(M, c, first, count, T, chain=1, apply=1):
    """The C call on the caller's own arrays: (rc, message)."""
    rc = M.lib().mml_gicp_refresh_batch(c._h, first, count, T.ctypes.data_as(C.c_void_p), chain, apply, None, None)
    return rc, M.lib().mml_last_error(c._h).decode()


def test_refusals_change_nothing_and_leave_the_context_usable(M, synth, four_scans, chained_reference):
    c = extracted_context(M, four_scans)
    try:
        T = np.stack([T_START, start_matrix(1), start_matrix(2), start_matrix(3)])
        T_before = T.tobytes()

        def refused(first, count, code, *words):
            before = [slot_bytes(c, s) for s in range(4)]
            rc, msg = raw_refresh_batch(M, c, first, count, T)
            assert rc == code, (rc, msg)
            assert "mml_gicp_refresh_batch" in msg and all(w in msg for w in words), msg
            assert T.tobytes() == T_before
            assert [slot_bytes(c, s) for s in range(4)] == before

        refused(0, 0, M.MML_ERR_INVALID, "count = 0")
        refused(2, 3, M.MML_ERR_INVALID, "slot 4")                           # a range past max_scans
        refused(4, 1, M.MML_ERR_INVALID, "slot 4")
        c.undistort(1, 1, np.eye(3).reshape(1, 9), np.zeros((1, 3)))        # an undistorted slot in the middle of the range
        refused(0, 4, M.MML_ERR_STATE, "slot 1 ", "undistorted")
        with pytest.raises(M.MmlError) as e:                                 # the single call's code
            c.gicp_refresh(1, T_START)
        assert e.value.code == M.MML_ERR_STATE
        c.extract(1, 1)
        v, l = four_scans[2]
        c.scan_upload(2, v, l)                                               # the raw scan staged again after the extraction
        refused(0, 4, M.MML_ERR_STATE, "slot 2's raw scan")
        c.extract(2, 1)
        # ... and the same context completes the valid call
        out = c.gicp_refresh_batch(0, 4, T_START, chain=True, apply=True)
        check_against_chain(chained_reference, out, [slot_bytes(c, s) for s in range(4)])
    finally:
        c.close()


def test_scratch_grows_shrinks_and_grows_again(M, tiny300):
    """300 problems, then 1, then 300 on one context (its block grows once and is then reused, also by the single call between
    them); a second context that starts with the small call and grows afterwards.  Same bytes every time."""
    pairs, single = tiny300["pairs"], tiny300["single"]
    big = pair(5, 700, 900)
    a, b = M.Context(max_scans=1), M.Context(max_scans=1)
    try:
        a300 = [key(r) for r in a.gicp_align_batch(pairs)]
        a1 = [key(r) for r in a.gicp_align_batch(pairs[17:18])]
        abig = key(a.gicp_align(*big))
        a300_again = [key(r) for r in a.gicp_align_batch(pairs)]
        b1 = [key(r) for r in b.gicp_align_batch(pairs[17:18])]
        bbig = key(b.gicp_align(*big))
        b300 = [key(r) for r in b.gicp_align_batch(pairs)]
        b1_again = [key(r) for r in b.gicp_align_batch(pairs[17:18])]
    finally:
        a.close()
        b.close()
    assert a300 == single and a300_again == single and b300 == single
    assert a1 == [single[17]] and b1 == a1 and b1_again == a1
    assert abig == bbig and abig[0]
