"""The cases of tests/assoc_cases.py on the oracle alone: every case takes the branch it is named for -- so many factors, so many
of them from the cube stage, these features without one --, with the cube map and, where a case has none, through the local-only
entry points as well; O.find_used_map and M.cube_index agree on every feature and on every map point.  A case that was meant for
the fall-back and is accepted in the cube, or the other way round, fails here, without a device."""
import numpy as np
import pytest

import assoc_cases as A


@pytest.fixture(scope="module")
def cases(M):
    return A.all_cases(M, M.default_config())


def test_case_names(cases):
    assert list(cases) == A.case_names() and len(set(A.case_names())) == len(A.case_names())


def _world(case, feats):
    """The features in the map frame as the association sees them: the pose applied in double, stored to float."""
    T = case["T"]
    with np.errstate(invalid="ignore"):
        return (feats.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


@pytest.mark.parametrize("name", A.case_names())
def test_oracle_takes_the_named_branch(M, O, cases, name):
    case = cases[name]
    ans = A.oracle_answer(O, case)
    for kind in (0, 1):
        rec, src, fg = ans[kind]
        e = case["expect"][kind]
        n = len(case["feats"][kind])
        assert (len(src), int(fg.sum())) == (e["n"], e["n_cube"]), (kind, src, fg)
        assert sorted(set(range(n)) - set(src.tolist())) == e["none"]
        # the cube of every feature, both ways
        w = _world(case, case["feats"][kind])
        ids = M.cube_index(w, case["cen"])
        for p, cid in zip(w, ids):
            if np.all(np.isfinite(p)):
                assert O.find_used_map(p, case["cen"]) == cid
        if case["glob"][kind] is not None:
            xyz, cube = case["glob"][kind]
            assert np.array_equal(cube, M.cube_index(xyz, case["cen"]))
            assert all(O.find_used_map(p, case["cen"]) == cid for p, cid in zip(xyz[::7], cube[::7]))
    print("%s: %d factor(s) from the cube stage, %d from the fall-back, none for %s" % (
        name, sum(e["n_cube"] for e in case["expect"]), sum(e["n"] - e["n_cube"] for e in case["expect"]),
        [e["none"] for e in case["expect"]]))


@pytest.mark.parametrize("name", [n for n in A.case_names() if "cubenone" in n])
def test_local_only_entry_points(O, cases, name):
    """A case without a cube map (default cen): associate_lines / associate_planes give what the two-level entry points give."""
    case = cases[name]
    assert case["glob"] == [None, None] and case["cen"] == A.DEFAULT_CEN
    ans = A.oracle_answer(O, case)
    lf, lsrc = O.associate_lines(case["feats"][0], O.KdTree(case["local"][0]), case["T"], case["thres"])
    pf, psrc = O.associate_planes(case["feats"][1], O.KdTree(case["local"][1]), case["T"], case["thres"])
    ol, op = A.factor_arrays(lf, pf)
    assert np.array_equal(lsrc, ans[0][1]) and np.array_equal(psrc, ans[1][1])
    assert np.array_equal(ol, ans[0][0]) and np.array_equal(op, ans[1][0])


@pytest.mark.parametrize("name", [n for n in A.case_names() if n[0] in "BCD"])
def test_cube_stage_decides(O, cases, name):
    """B, C, D: without the cube clouds the same features get the local map's model -- another record, or a factor where the cube
    stage gives none -- so a device that skipped or mis-tagged the cube stage cannot match the oracle by accident."""
    case = cases[name]
    kind = case["kind"]
    with_cube, without = A.oracle_answer(O, case)[kind], A.oracle_answer(O, case, cube=False)[kind]
    assert int(without[2].sum()) == 0
    if case["expect"][kind]["n_cube"]:
        assert not (np.array_equal(with_cube[1], without[1]) and np.array_equal(with_cube[0], without[0]))
    else:
        assert np.array_equal(with_cube[1], without[1]) and np.array_equal(with_cube[0], without[0])


@pytest.mark.parametrize("cen", [(10, 5, 10), (3, 3, 3)])
def test_cube_index_edges(M, O, cen):
    """Case E: on every edge point of every axis M.cube_index and O.find_used_map agree; the points are inside / outside the cube
    grid as edge_points says, and the two sides of a face are different cubes."""
    for ax in (0, 1, 2):
        edges = A.edge_points(ax, cen)
        ids = []
        for x, inside in edges:
            p = np.zeros(3, np.float32)
            p[ax] = x
            cid = O.find_used_map(p, cen)
            assert cid == int(M.cube_index(p[None], cen)[0]) and (cid != 5000) == inside, (ax, x, cid)
            ids.append(cid)
        assert ids[0] != ids[1] and ids[2] != ids[3] and ids[1] == ids[2] and len(set(ids[:5] + ids[6:7])) == 5
        step = (1, 21, 441)[ax]
        assert ids[0] - ids[1] == step and ids[2] - ids[3] == step


def test_both_kinds_case(M, O):
    """Case F: every prefix of the pool is a feature set (a feature's factor does not depend on the others); both stages occur
    for both kinds, features without a factor for the corner kind."""
    case = A.case_both_kinds(M, M.default_config())
    full = A.oracle_answer(O, case)
    for kind in (0, 1):
        rec, src, fg = full[kind]
        assert 0 < int(fg.sum()) < len(src) <= len(case["feats"][kind])
    assert len(full[0][1]) < len(case["feats"][0])   # (25 m^2 is 2.5 corner cells: the models three cells out are beyond it)
    for n in (1, 127, 129):
        part = A.oracle_answer(O, case, feats=[f[:n] for f in case["feats"]])
        for kind in (0, 1):
            keep = full[kind][1] < n
            assert np.array_equal(part[kind][1], full[kind][1][keep]) and np.array_equal(part[kind][0], full[kind][0][keep])
