"""tests/local_map_cases.py on the oracle alone: every case is what its name claims, so that the device test
(tests/test_gpu_local_map_edges.py) cannot pass because a case quietly stopped reaching its edge.  No GPU."""
import numpy as np
import pytest

import local_map_cases as L


@pytest.fixture(scope="module")
def cases(O):
    return L.build_cases(O)


def test_every_case_is_built(cases):
    assert sorted(cases) == sorted(L.SINGLE + ["E.capacity"] + L.BANKS)
    for name in L.SINGLE:
        assert any(len(c) != len(s) for c, s, _ in cases[name]["incs"]), name      # the two kinds of an increment differ in shape


def _ring(O, case, upto):
    """The ring's concatenation after increment `upto`, from the oracle: at a leaf of 1e-5 every point is its own voxel or the
    index overflows, and both give the cloud back."""
    sub = dict(case, incs=case["incs"][:upto + 1])
    return L.oracle_history(O, sub, leaf=(1e-5, 1e-5))[-1]


@pytest.mark.parametrize("name", [n for n in L.SINGLE if n.startswith("A.")])
def test_ring_occupancy(O, cases, name):
    case = cases[name]
    sc, ss = case["expect"]["sizes"]
    tot = L.ring_totals(case)
    seen_empty_lead = False
    for i in range(len(case["incs"])):
        lo = max(0, i + 1 - L.WINDOW)
        want = (sum(sc[lo:i + 1]), sum(ss[lo:i + 1]))
        assert tot[i][0] == want
        ring = _ring(O, case, i)
        assert (len(ring[0]), len(ring[1])) == want, (name, i)
        seen_empty_lead |= 0 in tot[i][1][0] and want[0] > 0
    assert seen_empty_lead                                   # a ring with points that starts with an empty slot
    assert min(min(sc), min(ss)) == 0 and sc != ss
    empties = [tot[i][1] for i in range(len(case["incs"]))]
    if name == "A.i.empty-first":
        assert tot[0][0] == (0, 0) and tot[1][0] == (0, 0) and tot[2][0] == (2, 3) and case["check_from"] == 0
    if name == "A.ii.runs":
        assert [t[0][0] for t in tot] == [0, 0, 3, 3, 4, 4, 4, 261, 261] and [t[0][1] for t in tot] == [0, 257, 257, 257, 258, 258, 261, 261, 261]
    if name == "A.iii.wrap-empties":
        assert empties[49] == ((), ()) and empties[53][0] == (0, 2) and empties[53][1] == (1, 3) and case["check_from"] == 50
    if name == "A.iv.last-slot":
        assert empties[49][0] == tuple(range(49)) and tot[48][0] == (0, 0) and tot[49][0] == (3, 1)
        assert empties[50][0] == tuple(range(1, 49)) and empties[51][0] == tuple(range(1, 49))


@pytest.mark.parametrize("name", [n for n in L.SINGLE if n.startswith("B.")])
def test_count_edges(O, cases, name):
    case = cases[name]
    hist = L.oracle_history(O, case)
    assert L.ring_totals(case)[-1][0] == case["expect"]["total"]
    assert (len(hist[-1][0]), len(hist[-1][1])) == case["expect"]["filtered"]
    assert case["check_from"] <= len(hist) - 1
    for kind in range(2):
        if case["expect"]["filtered"][kind] != 1 or case["expect"]["total"][kind] < 3:
            continue
        # the one-voxel cloud: the reversed order sums to other bits, so an order error cannot hide
        cat = np.concatenate([inc[kind] for inc in case["incs"]])
        assert np.array_equal(O.voxel_downsample(cat, L.LEAF[kind]), hist[-1][kind])
        rev = O.voxel_downsample(cat[::-1].copy(), L.LEAF[kind])
        assert len(rev) == 1 and rev.tobytes() != hist[-1][kind].tobytes(), name
    if name.endswith("mixed"):
        cat = np.concatenate([inc[0] for inc in case["incs"]])
        _, counts = np.unique(L.voxel_of(cat, L.LEAF[0]), axis=0, return_counts=True)
        assert set(counts) >= set(L.RUNS[:4]) and (len(cat) < 1000 or set(counts) >= set(L.RUNS))
        ring_order = np.unique(L.voxel_of(cat, L.LEAF[0]), axis=0, return_inverse=True)[1].reshape(-1)
        assert (np.diff(ring_order[:64]) != 0).sum() > 30              # shuffled: a voxel's points are not adjacent in the ring


def _pair_merges(O, a, b, T, kind):
    lm = O.LocalMap(window=L.WINDOW, leaf_corner=L.LEAF[0], leaf_surf=L.LEAF[1])
    pair = np.stack([a, b])
    lm.increment(pair if kind == 0 else L.EMPTY, pair if kind == 1 else L.EMPTY, T)
    return len(lm.get(kind)) == 1


def test_voxel_edges(O, cases):
    part = {}
    for pname in L.C_POSES:
        case = cases["C." + pname]
        (corner, surf, T), = case["incs"]
        hist = L.oracle_history(O, case)
        for kind, pts in enumerate((corner, surf)):
            vox = L.voxel_of(L.to_world(T, pts), L.LEAF[kind])
            groups = np.unique(vox, axis=0, return_inverse=True)[1].reshape(-1)
            assert len(np.unique(groups)) == len(hist[0][kind]) < len(pts)       # the restatement counts what the oracle counts
            merged, split = case["expect"]["merged"][kind], case["expect"]["split"][kind]
            assert merged and split
            for a, b in merged:
                assert _pair_merges(O, pts[a], pts[b], T, kind), (pname, kind, a, b)
            for a, b in split:
                assert not _pair_merges(O, pts[a], pts[b], T, kind), (pname, kind, a, b)
            n = case["expect"]["common"][kind]
            g = groups[:n]
            part[pname, kind] = g[:, None] == g[None, :]                         # which points of the common cloud share a voxel
    for kind in range(2):
        a, b, c = (part[p, kind] for p in L.C_POSES)
        assert (a != b).any() and (a != c).any() and (b != c).any()
    # the values that the float product lifts onto the integer are in the cloud, and the pose at 1e4 m makes the cast round
    for leaf in L.LEAF:
        vals, below = L.edge_values(leaf)
        inv = np.float32(1.0) / np.float32(leaf)
        assert all(np.float32(x * inv) == np.round(np.float64(x) / leaf) and np.float64(x) * np.float64(inv) < np.round(np.float64(x) / leaf) for x in below)
    (corner, _, T), = cases["C.far"]["incs"]
    exact = corner.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert (L.to_world(T, corner).astype(np.float64) != exact).any()
    (corner, surf, T), = cases["C.negative"]["incs"]
    assert (L.to_world(T, corner) < 0).all() and (L.to_world(T, surf) < 0).all()


@pytest.mark.parametrize("side", ["below", "above"])
def test_index_overflow(O, cases, side):
    case = cases["D." + side]
    hist = L.oracle_history(O, case)
    for kind in range(2):
        went_in = np.concatenate([case["incs"][0][kind], case["incs"][1][kind]])
        got = hist[1][kind]
        if side == "below":
            assert len(got) < len(went_in)
        else:
            assert got.tobytes() == went_in.tobytes()                              # unfiltered, in ring order
            assert len(O.voxel_downsample(went_in[2:], L.LEAF[kind])) < len(went_in) - 2   # with duplicates a filter would merge
        assert hist[L.WINDOW - 1][kind].tobytes() == got.tobytes()
        after = hist[L.WINDOW][kind]                                                # the wrap replaced the far points
        assert len(after) < len(case["incs"][1][kind]) + len(case["incs"][L.WINDOW][kind])
    lo, hi = cases["D.below"]["expect"]["extent"], cases["D.above"]["expect"]["extent"]
    assert all(np.nextafter(np.float32(a), np.float32(np.inf)) == np.float32(b) for a, b in zip(lo, hi))


def test_capacity(O, cases):
    case = cases["E.capacity"]
    mm = case["max_map_points"]
    hist, tot = L.oracle_history(O, case), L.ring_totals(case)
    at_c, at_s = case["expect"]["full_at"]
    assert tot[at_c][0][0] == mm == len(hist[at_c][0]) and tot[at_s][0][1] == mm == len(hist[at_s][1])
    for i in case["refused"]:
        before = tot[i - 1][0]
        would = (before[0] + len(case["incs"][i][0]), before[1] + len(case["incs"][i][1]))
        assert max(would) == mm + 1 and tot[i] == tot[i - 1]
    assert max(max(t[0]) for t in tot) == mm


def test_bank_cases(O, cases):
    sizes = {"empty": (0, 0), "one": (1, 0), "mixed": (8, 8), "mixed2": (8, 8), "above": (302, 202), "big": (1, 300)}
    assert [len(cases[n]["banks"]) for n in L.BANKS] == [1, 2, 3, 5, 9, 6, 6]
    for name in L.BANKS:
        f = cases[name]
        assert f["banks"][-1] == "empty" or "last" not in name
        for j, b in enumerate(f["banks"]):
            hist = L.oracle_history(O, L.bank_case(f, j))
            assert (len(hist[L.F_CALLS - 2][0]), len(hist[L.F_CALLS - 2][1])) == sizes[b], (name, j, b)
            if b != "empty":
                assert hist[-1][0].tobytes() != hist[-2][0].tobytes()
            if b == "mixed2":                                                       # the twin: the same map from another ring slot
                twin = L.oracle_history(O, L.bank_case(f, j - 1))
                assert f["banks"][j - 1] == "mixed" and twin[-2][0].tobytes() == hist[-2][0].tobytes()
            if b == "big":
                assert L.ring_totals(L.bank_case(f, j))[L.F_CALLS - 2][0] == (65537, 300) and f["big"] == j
    # 2 n crosses 2, 4, 8 and 16
    assert [int(np.ceil(np.log2(2 * len(cases[n]["banks"])))) for n in L.BANKS[:5]] == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("name", L.KNN)
def test_knn_queries_have_no_ties(O, cases, name):
    """The grid check compares indices: the six nearest map points of every query are at six distinct distances."""
    case = cases[name]
    hist = L.oracle_history(O, case)[case["knn_at"]]
    for kind in range(2):
        cloud = hist[kind]
        if len(cloud) < 6:
            continue
        q = L.knn_queries(cloud, 7 + kind)
        assert 60 <= len(q) <= 70
        d2 = np.sort(((q[:, None, :].astype(np.float64) - cloud[None].astype(np.float64)) ** 2).sum(axis=2), axis=1)[:, :6]
        assert (np.diff(d2, axis=1) > 2e-6 * d2[:, 1:]).all(), name
