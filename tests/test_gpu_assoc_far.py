"""The far-query search of the association (k_associate_hard: shells >= 2, clipped by the gate, rows four at a time) on
hand-built maps of a few dozen points, against the oracle's associate_lines / associate_planes.

Every case runs at 2, 6 and 12 slots -- 64, 32 and 4 lanes per far query -- with the same features in every slot; all slots
must match the oracle (same features accepted, records within 1e-9, as tests/test_gpu_parity.py::test_association_matches_oracle
asks) and the three runs must leave byte-identical records.

Geometry: coordinates are multiples of the kind's grid cell c (5 x leaf, a power of two times 0.1 ... exact in float for the
dyadic offsets used where exactness matters).  "Anchor" points on the corners and edge midpoints of [0, 20 c]^3 fix the grid:
origin 0, 21 cells per axis; they lie farther than the gate from every query.  T = identity, so a feature is its own query."""
import numpy as np
import pytest

from assoc_cases import _anchors, _cells, _centre, _dummy, _five
from conftest import pose_to_x

pytestmark = pytest.mark.gpu

SLOTS = (2, 6, 12)


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=12)
    yield c
    c.close()


def _run(ctx, O, maps, feats, thres):
    """Associates feats against maps at 2, 6 and 12 slots; checks every slot against the oracle and the three runs against each
    other.  Returns ((line records, src), (plane records, src)) of slot 0."""
    maps = [np.ascontiguousarray(m, np.float32) for m in maps]
    feats = [np.ascontiguousarray(f, np.float32).reshape(-1, 3) for f in feats]
    assert len(maps[0]) > 20 and len(maps[1]) > 20
    ctx.map_set_local(0, maps[0])
    ctx.map_set_local(1, maps[1])
    trees = [O.KdTree(maps[0]), O.KdTree(maps[1])]
    T = np.eye(4)
    lf, lsrc = O.associate_lines(feats[0], trees[0], T, thres)
    pf, psrc = O.associate_planes(feats[1], trees[1], T, thres)
    ol = np.concatenate([lf["point_ori"], lf["p1"], lf["p2"], lf["error"][:, None]], axis=1)
    op = np.concatenate([pf["point_ori"], pf["point_proj"], pf["omega"], pf["error"][:, None]], axis=1)
    first = None
    for n in SLOTS:
        for s in range(n):
            ctx.features_upload(s, 0, feats[0])
            ctx.features_upload(s, 1, feats[1])
        ctx.associate(0, n, np.stack([T] * n), thres)
        for s in range(n):
            gl, glsrc = ctx.factors_download(s, 0)
            gp, gpsrc = ctx.factors_download(s, 1)
            assert np.array_equal(glsrc, lsrc) and np.array_equal(gpsrc, psrc), (n, s, glsrc, lsrc, gpsrc, psrc)
            assert np.allclose(gl, ol, rtol=0, atol=1e-9) and np.allclose(gp, op, rtol=0, atol=1e-9), (n, s)
            got = (gl.tobytes(), glsrc.tobytes(), gp.tobytes(), gpsrc.tobytes())
            if first is None:
                first = got
            assert got == first, "slot %d of %d differs from slot 0 of %d" % (s, n, SLOTS[0])
    return (ol, lsrc), (op, psrc)


def _run_kind(ctx, O, kind, cmap, feats, thres):
    """One kind under test, the other kind idle; returns (records, src) of the kind."""
    c = _cells(ctx)
    dm, df = _dummy(c[1 - kind])
    maps, fts = [dm, dm], [df, df]
    maps[kind], fts[kind] = cmap, feats
    return _run(ctx, O, maps, fts, thres)[kind]


@pytest.mark.parametrize("kind", [0, 1])
def test_four_inside_fifth_beyond_gate(ctx, O, kind):
    """Case 1: four map points within the gate, the fifth just beyond it: no factor."""
    c = _cells(ctx)[kind]
    q = _centre(c)
    R = 5.0 * c
    ex, ey = np.eye(3)[0], np.eye(3)[1]
    five = _five(kind, q - np.array([1.01 * R, 0, 0]), 0.3 * c, ex, ey)  # the base point is the farthest of the five
    m = np.concatenate([five, _anchors(c, q, 1.5 * R)])
    d = np.sort(np.linalg.norm(m - q, axis=1))
    assert d[3] < 0.99 * R and d[4] > 1.005 * R
    rec, src = _run_kind(ctx, O, kind, m, q[None], R * R)
    assert len(src) == 0


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("frac, factor", [(0.25, True), (-0.25, False), (-0.75, False)])
def test_fifth_neighbour_one_float_from_gate(ctx, O, kind, frac, factor):
    """Case 2: d2 of the fifth neighbour is exactly 25 (offset 5 m along x from a query with exact coordinates); thres_dist is
    no float: 25 + 0.25 ulp (d2 is the float below it, the search bound is the float above: factor), 25 - 0.25 ulp and
    25 - 0.75 ulp (d2 is the float above thres_dist and equals the search bound, reached with and without the round-up: none)."""
    c = _cells(ctx)[kind]
    q = _centre(c)
    ulp = float(np.spacing(np.float32(25.0)))
    below = float(np.float32(25.0) - np.nextafter(np.float32(25.0), np.float32(0)))
    thres = 25.0 + (frac * ulp if frac > 0 else frac * below)
    assert float(np.float32(thres)) != thres
    ex, ey = np.eye(3)[0], np.eye(3)[1]
    five = _five(kind, q - np.array([5.0, 0, 0]), 0.125, ex, ey)
    m = np.concatenate([five, _anchors(c, q, 7.5)])
    f32 = five.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), five)
    d2 = np.sort(((f32 - q.astype(np.float32)) ** 2).sum(1, dtype=np.float32))
    assert d2[4] == np.float32(25.0) and d2[3] < 25.0
    rec, src = _run_kind(ctx, O, kind, m, q[None], thres)
    assert len(src) == (1 if factor else 0)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("where", ["xface", "face", "edge", "corner"])
def test_five_in_one_far_shell(ctx, O, kind, where):
    """Case 3: all five neighbours in one shell >= 3 (shell 3 and shell 4), rings 0-2 empty: on an x-face row (end cells only),
    on a face row (whole x span), on an edge and on a corner of the shell."""
    c = _cells(ctx)[kind]
    q = _centre(c)
    for shell, sign in ((3, 1.0), (3, -1.0), (4, 1.0)):
        near = shell - 0.4  # offset (cells) of the cluster from the query: cell `shell` away, near its inner side
        off = {"xface": (near, 0.1, -0.1), "face": (0.1, -0.1, near), "edge": (0.1, near, near), "corner": (near, near, near)}[where]
        if where == "corner" and shell == 4:
            continue  # beyond the gate radius of 5 cells used here
        base = q + sign * np.array(off) * c
        axes = np.eye(3)
        a, b = (axes[1], axes[2]) if where == "xface" else (axes[0], axes[1])
        five = _five(kind, base, 0.05 * c, sign * a, sign * b)
        cellidx = np.floor(five / c).astype(int) - 10
        assert np.all(np.abs(cellidx).max(1) == shell)
        m = np.concatenate([five, _anchors(c, q, 7.5 * c)])
        rec, src = _run_kind(ctx, O, kind, m, q[None], (6.0 * c) ** 2 if shell == 4 else (5.0 * c) ** 2)
        assert len(src) == 1, (where, shell, sign)


@pytest.mark.parametrize("kind", [0, 1])
def test_tie_across_lanes_and_groups(ctx, O, kind):
    """Case 4: two candidates for the fifth place at equal d2, in rows y = hy - 3 and y = hy + 3 of z = hz - 1 in shell 3 (row
    numbers 14 and 20 of its 7 x 7 rows: lanes 2 and 0, groups 0 and 1 at four lanes a query): the lower index wins, whichever
    of the two it is."""
    c = _cells(ctx)[kind]
    q = _centre(c)
    A = q + np.array([0.125, 2.75, -0.875]) * c
    B = q + np.array([0.125, -2.75, -0.875]) * c
    if kind == 0:
        four = np.array([q + np.array([0.125, t, -0.875]) * c for t in (2.25, 1.75, 1.25, 0.75)])
    else:
        four = np.array([q + np.array([0.125, y, z]) * c for y, z in ((2.0, -0.5), (2.0, -1.0), (1.5, -0.25), (1.5, -1.25))])
    qf = q.astype(np.float32)
    dA = ((A.astype(np.float32) - qf) ** 2).sum(dtype=np.float32)
    dB = ((B.astype(np.float32) - qf) ** 2).sum(dtype=np.float32)
    assert dA == dB and np.all(((four.astype(np.float32) - qf) ** 2).sum(1) < dA)
    anchors = _anchors(c, q, 7.5 * c)
    out = []
    for pair in ((A, B), (B, A)):
        m = np.concatenate([four, np.array(pair), anchors])
        out.append(_run_kind(ctx, O, kind, m, q[None], (5.0 * c) ** 2))
    assert len(out[0][1]) == 1  # A first: the line / the plane through A and the four
    if len(out[1][1]) == 1:
        assert not np.array_equal(out[0][0], out[1][0])  # B first: another model (or none)


@pytest.mark.parametrize("kind", [0, 1])
def test_queries_outside_the_grid(ctx, O, kind):
    """Case 5: a query outside the map's bounding box beyond each of its six sides, five points within the gate."""
    c = _cells(ctx)[kind]
    qs, clusters = [], []
    for ax in range(3):
        for side in (0, 1):
            q = _centre(c)
            q[ax] = -2.2 * c if side == 0 else 22.2 * c
            inward = np.zeros(3)
            inward[ax] = 1.0 if side == 0 else -1.0
            base = q + inward * 2.6 * c
            a, b = np.eye(3)[(ax + 1) % 3], np.eye(3)[(ax + 2) % 3]
            clusters.append(_five(kind, base, 0.05 * c, a, b))
            qs.append(q)
    qs = np.array(qs)
    m = np.concatenate(clusters + [_anchors(c, qs, 7.5 * c)])
    assert np.all(m.min(0) == 0) and np.all(m.max(0) == 20 * c)  # the queries lie outside the grid
    rec, src = _run_kind(ctx, O, kind, m, qs, (5.0 * c) ** 2)
    assert len(src) == 6


@pytest.mark.parametrize("kind", [0, 1])
def test_shells_of_1_4_5_9_rows(ctx, O, kind):
    """Case 6: queries on a grid edge (hy = hz = 0: shell r has (r + 1)^2 in-grid rows: 1, 4, 9, 16) with their five points in
    the LAST row of shell 0, 1, 2 and 3; and a grid 21 x 5 x 1 cells (shells of 1, 2, 3, 4, 5, 5 rows), five points in row 5."""
    c = _cells(ctx)[kind]
    ex, ey, ez = np.eye(3)
    qs, clusters = [], []
    for r, x in zip((0, 1, 2, 3), (0.5, 6.5, 13.5, 19.5)):
        q = np.array([x, 0.5, 0.5]) * c
        d = (r + 0.3) if r else 0.6
        clusters.append(_five(kind, np.array([x * c, d * c, d * c]), 0.05 * c, ex, ey))
        qs.append(q)
    qs = np.array(qs)
    m = np.concatenate(clusters + [_anchors(c, qs, 7.5 * c)])
    rec, src = _run_kind(ctx, O, kind, m, qs, (5.0 * c) ** 2)
    assert len(src) == 4
    # the thin grid
    q = np.array([10.5, 0.5, 0.25]) * c
    five = _five(kind, np.array([10.4 * c, 4.3 * c, 0.25 * c]), 0.05 * c, ex, ey if kind == 0 else ez * 0.5)
    anchors = np.array([[x * c, y * c, z * c] for x in (0, 1, 2, 18, 19, 20) for y in (0, 4.0) for z in (0, 0.5)])
    m = np.concatenate([five, anchors])
    assert np.array_equal(np.floor(m.max(0) / c).astype(int) + 1, [21, 5, 1]) and np.all(np.floor(five[:, 1] / c) == 4)
    rec, src = _run_kind(ctx, O, kind, m, q[None], (5.0 * c) ** 2)
    assert len(src) == 1


def test_both_kinds_far_in_one_call(ctx, O):
    """Case 7: a corner-kind and a surf-kind far query in the same call at thres_dist 25: cells of 5 x leaf each, so the two
    walk to different last shells.  Each kind has a query whose five points lie 3.2 .. 3.6 m away and one that has none."""
    cells = _cells(ctx)
    assert cells[0] != cells[1]
    maps, feats, expect = [], [], []
    for kind in (0, 1):
        c = cells[kind]
        q = _centre(c)
        q2 = q + np.array([0, 0, 9.0])  # nothing within 5 m: walks every shell to the gate
        five = _five(kind, q + np.array([3.2, 0.1, -0.1]), 0.1, np.eye(3)[1], np.eye(3)[2])
        m = np.concatenate([five, _anchors(c, np.array([q, q2]), 7.5)])
        assert np.sort(np.linalg.norm(m - q2, axis=1))[0] > 5.1
        maps.append(m)
        feats.append(np.array([q, q2]))
    (lrec, lsrc), (prec, psrc) = _run(ctx, O, maps, feats, 25.0)
    assert list(lsrc) == [0] and list(psrc) == [0]


def test_far_count_is_the_last_calls_own(M, synth, scene):
    """mml_associate_far_count after a two-lane step over 64 slots and then a one-slot associate: the one-slot call queues every
    feature of its slot (<= 8 slots: all queries go to the far kernels), and that is the count -- not that plus what lane 1 of the
    step left in its counter."""
    B = 64
    c = M.Context(max_scans=B)
    try:
        c.map_set_local(0, scene["corner_map"])
        c.map_set_local(1, scene["surf_map"])
        v, l = synth.velo_scan(10, n_az=450), synth.livox_scan(10, n=6000)
        for s in range(B):
            c.scan_upload(s, v, l)
        T = synth.pose_matrix(10)
        x0 = np.stack([pose_to_x(T)] * B)
        c.step(0, B, np.stack([np.eye(3).reshape(9)] * B), np.zeros((B, 3)), np.eye(4), 25.0, 2, x0)
        far_step = c.associate_far_count()
        nf = len(c.features_download(0, 0)) + len(c.features_download(0, 1))
        assert 0 < far_step <= B * nf
        c.associate(0, 1, T[None], 25.0)
        assert c.associate_far_count() == nf
        # slot 0 alone saw the same features in the step: lane 1's 32 slots had far queries of their own
        c.associate(0, 32, np.stack([T] * 32), 25.0)
        far_half = c.associate_far_count()
        assert 0 < far_half < far_step
    finally:
        c.close()
