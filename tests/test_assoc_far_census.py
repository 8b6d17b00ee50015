"""tools/assoc_far_census.py: its restatement of the grid mapping, the stop rule and the row rule of the 5-NN shell search, on
a 3 x 3 x 3 grid with answers worked out by hand."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

INF = float("inf")


@pytest.fixture(scope="module")
def C():
    spec = importlib.util.spec_from_file_location("assoc_far_census", os.path.join(ROOT, "tools", "assoc_far_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _occ():
    occ = np.zeros((3, 3, 3), np.int32)  # [x, y, z]
    occ[0, 1, 1] = 1
    occ[1, 0, 1] = 2
    occ[2, 2, 2] = 1
    return occ


def test_grid_mapping(C):
    pts = np.array([[0, 0, 0], [2.9, 2.9, 2.9], [1.0, 1.99, 2.0]], np.float32)
    g = C.grid_of(pts, 1.0)
    assert list(g["dims"]) == [3, 3, 3] and np.all(g["origin"] == 0)
    assert C.cell_coords(g, pts).tolist() == [[0, 0, 0], [2, 2, 2], [1, 1, 2]]
    assert C.cell_coords(g, [[-0.5, 3.5, 1.0]]).tolist() == [[0, 2, 1]]  # clamped
    h, f, inset = C.query_cell(g, [-0.5, 1.25, 3.5])  # the home cell of a query is not clamped
    assert list(h) == [-1, 1, 3] and inset == 0.25
    assert C.rmax_of(dict(cell=2.0), 25.0) == 4 and C.rmax_of(dict(cell=1.0), 25.0) == 6


def test_stop_rule(C):
    g = dict(cell=2.0)
    # after shell 1 with inset 0.5: rho = 1.5 * 2 - 0.002 = 2.998, rho^2 = 8.988
    assert C.knn_done(g, 0.5, 1, 8.9, 25.0)
    assert not C.knn_done(g, 0.5, 1, 9.0, 25.0)
    assert C.knn_done(g, 0.5, 1, INF, 8.9)      # the visited radius has reached the gate
    assert not C.knn_done(g, 0.0, 0, 0.0, 25.0)  # no radius yet


def test_rows_of_a_shell(C):
    dims = (3, 3, 3)
    mid, corner = (1, 1, 1), (0, 0, 0)
    assert C.shell_rows(dims, mid, 0) == [(1, 1)]
    assert len(C.shell_rows(dims, mid, 1)) == 9 and len(C.shell_rows(dims, mid, 2)) == 9
    assert [len(C.shell_rows(dims, corner, r)) for r in (0, 1, 2, 3)] == [1, 4, 9, 9]
    assert C.shell_rows(dims, corner, 1) == [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_cells_of_a_row(C):
    dims, h, f = (3, 3, 3), (1, 1, 1), (1.5, 1.5, 1.5)
    assert C.row_cells(dims, h, f, 1, 0, 0, INF) == [0, 1, 2]   # face row: the whole span
    assert C.row_cells(dims, h, f, 1, 1, 1, INF) == [0, 2]      # the two end cells
    assert C.row_cells(dims, h, f, 2, 1, 1, INF) == []          # shell 2: its end cells lie outside the grid
    # bound 0.6 cells: reach 0.604; the row at gap 0.5 keeps w = sqrt(0.3648 - 0.25) = 0.339 -> x in [1.16, 1.84]: cell 1
    assert C.row_cells(dims, h, f, 1, 0, 1, 0.6) == [1]
    assert C.row_cells(dims, h, f, 1, 0, 0, 0.6) is None        # gap^2 = 0.5 > 0.365
    assert C.row_cells(dims, h, f, 1, 1, 1, 0.6) == [0, 2]      # x in [0.90, 2.10] reaches both end cells
    assert C.row_cells(dims, h, f, 1, 1, 1, 0.4) == []          # x in [1.10, 1.90] reaches neither


def test_row_counts(C):
    occ = _occ()
    h, f = (1, 1, 1), (1.5, 1.5, 1.5)
    assert C.count_rows(occ, h, f, 1, INF) == (9, 6)   # points in rows (1, 1), (0, 1) and (2, 2)
    assert C.count_rows(occ, h, f, 1, 0.6) == (5, 3)   # the four corner rows fall outside; (1, 1) and (0, 1) hold points
    assert C.count_rows(occ, h, f, 1, 0.4) == (1, 1)   # gap 0.5 > reach 0.404: the centre row alone, and it reads no cell
    # home cell at the grid corner: shell 2 has nine rows, only the face row (2, 2) reaches the point at (2, 2, 2)
    assert C.count_rows(occ, (0, 0, 0), (0.5, 0.5, 0.5), 2, INF) == (9, 8)
    assert C.count_rows(occ, (0, 0, 0), (0.5, 0.5, 0.5), 1, INF) == (4, 2)  # rows (0, 1) and (1, 1) hold points
