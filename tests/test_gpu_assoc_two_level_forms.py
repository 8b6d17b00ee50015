"""The two-level association -- the cube cloud of the feature's own cube first, the local map as fall-back -- in every launch form,
on the hand-built cases of tests/assoc_cases.py, against the oracle's associate_lines2 / associate_planes2.

Own maps: the case's maps in the context's own (map_set_local / map_set_global), the same features in every slot, at 2, 6 and 12
slots: the fresh form at 64 and at 32 lanes a query, and the lane-per-feature form with k_associate_hard<4> and its second round.
Banked: 12 slots over three banks -- two hold the case's maps, the third its local maps without the cube clouds -- and one unbound
slot that reads the context's own maps (the local maps moved by 0.125 m, no cube map).  Every slot is checked against the
oracle's answer for the map it is bound to: the same features accepted, records within 1e-9 (the rule of
tests/test_gpu_parity.py::test_association_matches_oracle); the slots of one map leave byte-identical records.

tests/test_assoc_two_level_census.py shows, without a device, that the oracle takes the branch each case is named for."""
import numpy as np
import pytest

import assoc_cases as A

pytestmark = pytest.mark.gpu

SLOTS = (2, 6, 12)
BIND = [0, 1, 2, 0, 1, -1, 2, 0, 1, 0, 2, 1]   # slot -> bank, -1 the context's own maps
MAP_OF = {0: "cube", 1: "cube", 2: "local", -1: "own"}
MM = 1 << 16
EMPTY = np.zeros((0, 3), np.float32)
NOCUBE = np.zeros(0, np.int32)
OWN_SHIFT = np.array([0.0, 0.0, 0.125], np.float32)


@pytest.fixture(scope="module")
def cases(M):
    return A.all_cases(M, M.default_config())


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=12, max_map_points=MM, max_features=512)
    assert A._cells(c) == A._cells(M.default_config())
    yield c
    c.close()


@pytest.fixture(scope="module")
def bctx(M):
    c = M.Context(max_scans=12, max_map_points=MM, max_features=512)
    c.map_banks(3)
    c.bind_banks(0, BIND)
    yield c
    c.close()


@pytest.fixture(scope="module")
def both(M, O):
    """Case F and the oracle's answer for its whole pool, against each of the three maps of the banked variant."""
    case = A.case_both_kinds(M, M.default_config())
    return case, _answers(O, case)


def _own_local(case):
    return [m + OWN_SHIFT for m in case["local"]]


def _answers(O, case, feats=None):
    return {"cube": A.oracle_answer(O, case, feats), "local": A.oracle_answer(O, case, feats, cube=False),
            "own": A.oracle_answer(O, case, feats, local=_own_local(case), cube=False)}


def _prefix(ans, n):
    """The answer for the first n[kind] features of the pool `ans` is the answer of."""
    out = []
    for kind in (0, 1):
        rec, src, fg = ans[kind]
        keep = src < n[kind]
        out.append((rec[keep], src[keep], fg[keep]))
    return out


def _set_own(c, case, local=None, cube=True):
    for kind in (0, 1):
        c.map_set_local(kind, (local or case["local"])[kind])
        g = case["glob"][kind] if cube else None
        c.map_set_global(kind, *(g if g is not None else (EMPTY, NOCUBE)), case["cen"])


def _set_banks(c, case):
    for b in (0, 1, 2):
        for kind in (0, 1):
            c.bank_set_local(b, kind, case["local"][kind])
            g = case["glob"][kind] if b < 2 else None
            c.bank_set_global(b, kind, *(g if g is not None else (EMPTY, NOCUBE)), case["cen"])
    _set_own(c, case, _own_local(case), cube=False)


def _check_slot(c, s, want, stats=None):
    """Slot s holds the oracle's answer `want`; returns its records as bytes."""
    gl, glsrc = c.factors_download(s, 0)
    gp, gpsrc = c.factors_download(s, 1)
    (ol, lsrc, _), (op, psrc, _) = want
    assert np.array_equal(glsrc, lsrc) and np.array_equal(gpsrc, psrc), (s, glsrc, lsrc, gpsrc, psrc)
    assert np.allclose(gl, ol, rtol=0, atol=1e-9) and np.allclose(gp, op, rtol=0, atol=1e-9), s
    if stats is not None:
        assert (stats.n_line, stats.n_plane) == (len(lsrc), len(psrc))
    return gl.tobytes(), glsrc.tobytes(), gp.tobytes(), gpsrc.tobytes()


def _upload(c, case, slots):
    for s in slots:
        for kind in (0, 1):
            c.features_upload(s, kind, case["feats"][kind])


@pytest.mark.parametrize("name", A.case_names())
def test_own_maps(ctx, O, cases, name):
    case = cases[name]
    want = A.oracle_answer(O, case)
    _set_own(ctx, case)
    _upload(ctx, case, range(12))
    first = None
    for n in SLOTS:
        st = ctx.associate(0, n, np.stack([case["T"]] * n), case["thres"])
        if n == 12 and case["far"]:
            assert ctx.associate_far_count() > 0
        for s in range(n):
            got = _check_slot(ctx, s, want, st[s])
            first = first or got
            assert got == first, "slot %d of %d differs from slot 0 of %d" % (s, n, SLOTS[0])


@pytest.mark.parametrize("name", A.case_names())
def test_banked(bctx, O, cases, name):
    case = cases[name]
    want = _answers(O, case)
    _set_banks(bctx, case)
    _upload(bctx, case, range(12))
    st = bctx.associate(0, 12, np.stack([case["T"]] * 12), case["thres"])
    if case["far"]:
        assert bctx.associate_far_count() > 0
    first = {}
    for s in range(12):
        m = MAP_OF[BIND[s]]
        got = _check_slot(bctx, s, want[m], st[s])
        assert got == first.setdefault(m, got), "slot %d differs from the first slot of map '%s'" % (s, m)


# ---- F: chunk and prefix edges of the lane-per-feature pass ----------------------------------------------------------------------

COUNTS = ([0, 1, 127, 128, 129, 257, 0, 257, 1, 0, 128, 129],   # corner features of slot s
          [129, 0, 257, 1, 0, 127, 128, 0, 257, 129, 0, 1])     # surf features: a (kind, slot) item without features between filled ones


def _upload_counts(c, case):
    for s in range(12):
        for kind in (0, 1):
            c.features_upload(s, kind, case["feats"][kind][:COUNTS[kind][s]])


def test_chunk_edges(ctx, both):
    """0, 1, 127, 128, 129 and 257 features per (slot, kind) -- none, one lane, one short of a chunk, a chunk, a chunk and a lane,
    two chunks and a lane -- in one 12-slot call; then slots 3 .. 11 again as associate(3, 9, ...): first > 0."""
    case, ans = both
    assert all(sorted(set(k)) == [0, 1, 127, 128, 129, 257] for k in COUNTS)
    _set_own(ctx, case)
    _upload_counts(ctx, case)
    T = np.stack([case["T"]] * 12)
    st = ctx.associate(0, 12, T, case["thres"])
    assert ctx.associate_far_count() > 0
    recs = [_check_slot(ctx, s, _prefix(ans["cube"], (COUNTS[0][s], COUNTS[1][s])), st[s]) for s in range(12)]
    assert sum(st[s].n_line + st[s].n_plane for s in range(12)) > 500
    # the same records again from a call that starts at slot 3; to see that it wrote them, slots 3 .. 11 first get other poses
    Tm = T.copy()
    Tm[:, 2, 3] = 0.03
    ctx.associate(0, 12, Tm, case["thres"])
    assert any(_records(ctx, s) != recs[s] for s in range(3, 12))
    moved = [_records(ctx, s) for s in range(3)]
    st = ctx.associate(3, 9, T[3:], case["thres"])
    for s in range(3, 12):
        assert _check_slot(ctx, s, _prefix(ans["cube"], (COUNTS[0][s], COUNTS[1][s])), st[s - 3]) == recs[s]
    assert [_records(ctx, s) for s in range(3)] == moved   # slots 0 .. 2 are not the call's


def _records(c, s):
    gl, glsrc = c.factors_download(s, 0)
    gp, gpsrc = c.factors_download(s, 1)
    return gl.tobytes(), glsrc.tobytes(), gp.tobytes(), gpsrc.tobytes()


def test_chunk_edges_banked(bctx, both):
    """The feature counts of test_chunk_edges over the three banks and the unbound slot."""
    case, ans = both
    _set_banks(bctx, case)
    _upload_counts(bctx, case)
    st = bctx.associate(0, 12, np.stack([case["T"]] * 12), case["thres"])
    assert bctx.associate_far_count() > 0
    for s in range(12):
        _check_slot(bctx, s, _prefix(ans[MAP_OF[BIND[s]]], (COUNTS[0][s], COUNTS[1][s])), st[s])


def test_few_features_after_many(ctx, O, both):
    """257 features a slot and kind, then three in the same slots, two of them without a factor: the second call's records and src
    lists hold nothing of the first (a feature's record bytes park the search result of pass 1 before they hold a factor)."""
    case, ans = both
    _set_own(ctx, case)
    T = np.stack([case["T"]] * 12)
    for s in range(12):
        for kind in (0, 1):
            ctx.features_upload(s, kind, case["feats"][kind])
    st = ctx.associate(0, 12, T, case["thres"])
    assert all(st[s].n_line + st[s].n_plane > 300 for s in range(12))
    few = [case["feats"][0][[3, 1, 7]], case["feats"][1][[2, 3, 5]]]
    want = A.oracle_answer(O, case, few)
    assert len(want[0][1]) < 3 and len(want[0][1]) + len(want[1][1]) > 0
    for s in range(12):
        for kind in (0, 1):
            ctx.features_upload(s, kind, few[kind])
    st = ctx.associate(0, 12, T, case["thres"])
    first = None
    for s in range(12):
        got = _check_slot(ctx, s, want, st[s])
        first = first or got
        assert got == first


@pytest.mark.parametrize("count", [513, 600])
def test_prefix_carries_across_tiles(M, O, both, count):
    """2 * count > 1024 (kind, slot) items: k_assoc_prefix walks more than one tile of 1024 and carries its running sum into the
    next.  One to three features per slot and kind, cycled from six small sets; every slot against the oracle's answer for its set."""
    case, _ = both
    sets = [[case["feats"][0][4 * j:4 * j + 1 + j % 3], case["feats"][1][4 * j + 1:4 * j + 2 + (j + 1) % 3]] for j in range(6)]
    want = [A.oracle_answer(O, case, f) for f in sets]
    assert sum(len(w[0][1]) + len(w[1][1]) for w in want) > 6
    c = M.Context(max_scans=count, max_velo_points=0, max_livox_points=64, max_features=64, max_map_points=1 << 15)
    try:
        _set_own(c, case)
        for s in range(count):
            for kind in (0, 1):
                c.features_upload(s, kind, sets[s % 6][kind])
        st = c.associate(0, count, np.stack([case["T"]] * count), case["thres"])
        first = {}
        for s in range(count):
            got = _check_slot(c, s, want[s % 6], st[s])
            assert got == first.setdefault(s % 6, got), s
    finally:
        c.close()
