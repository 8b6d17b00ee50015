"""The grid build (csrc/map_assoc.hip mml_build_grids) on its one-cloud path -- map_set_local and the cube map's map_set_global, 32-bit
keys holding the cell alone -- at the smallest inputs at which the shared builder can go wrong.  Every case is checked through knn5
or associate against the oracle's kd-tree, indices exact."""
import numpy as np
import pytest

from conftest import perturbed
from test_gpu_bank_increment_segmented import _per_cell, refinement_clouds

pytestmark = pytest.mark.gpu

MM = 1 << 16
EMPTY = np.zeros((0, 3), np.float32)


@pytest.fixture
def c(M):
    ctx = M.Context(max_scans=1, max_map_points=MM)
    yield ctx
    ctx.close()


def _knn_exact(c, O, kind, cloud, q):
    gi, gd = c.knn5(kind, q)
    oi, od = O.KdTree(cloud).knn5(q)
    assert np.array_equal(gi, oi) and gd.tobytes() == od.tobytes()
    assert (gi >= 0).all() and (gi < len(cloud)).all()


@pytest.mark.parametrize("m", [0, 1])
def test_tiny_maps(c, O, scene, m):
    """m = 0 (the empty grid: 1 x 1 x 1, two zero ints in cell_start) and m = 1: no neighbour sets, no factors, as on the oracle."""
    rng = np.random.default_rng(m)
    cloud = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    q = rng.uniform(-2, 2, (70, 3)).astype(np.float32)
    fr = scene["frames"][0]
    for kind in range(2):
        c.map_set_local(kind, cloud)
        assert len(c.map_local_download(kind)) == m
        gi, _ = c.knn5(kind, q, max_d2=25.0)
        assert np.all(gi == -1)
    c.features_upload(0, 0, fr["corner"][:100])
    c.features_upload(0, 1, fr["surf"][:100])
    c.associate(0, 1, fr["T_gt"][None], 25.0)
    tree = O.KdTree(cloud)
    assert len(O.associate_lines(fr["corner"][:100], tree, fr["T_gt"], 25.0)[1]) == 0
    assert len(O.associate_planes(fr["surf"][:100], tree, fr["T_gt"], 25.0)[1]) == 0
    assert len(c.factors_download(0, 0)[1]) == 0 and len(c.factors_download(0, 1)[1]) == 0
    # a map after the empty one: the builder's state does not stick
    cloud = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    c.map_set_local(1, cloud)
    _knn_exact(c, O, 1, cloud, q)


@pytest.mark.parametrize("m", [256, 257])
def test_workgroup_edge(c, O, m):
    """One point each side of a 256-thread workgroup."""
    rng = np.random.default_rng(m)
    cloud = rng.uniform(-6, 6, (m, 3)).astype(np.float32)
    q = np.concatenate([rng.uniform(-7, 7, (200, 3)).astype(np.float32), cloud[-3:]])
    for kind in range(2):
        c.map_set_local(kind, cloud)
        _knn_exact(c, O, kind, cloud, q)


def test_one_cell(M, O):
    """All points in one cell and ncell = 1: 12 points (the densest cell the rule leaves alone) inside a twentieth of a cell edge."""
    rng = np.random.default_rng(3)
    edge = 1.0
    cloud = (np.float32(4.0) + rng.uniform(0, edge / 20, (12, 3))).astype(np.float32)
    assert _per_cell(cloud, edge) == 12.0
    q = np.concatenate([cloud[:4], rng.uniform(3, 5, (60, 3)).astype(np.float32)])
    ctx = M.Context(max_scans=1, max_map_points=MM, cell_corner=edge, cell_surf=edge)
    try:
        for kind in range(2):
            ctx.map_set_local(kind, cloud)
            _knn_exact(ctx, O, kind, cloud, q)
    finally:
        ctx.close()


def test_refinement_rounds(M, O):
    """The dense plane of test_refinement as a set map at cell = 8 x leaf: ~58 points per occupied cell, then ~15 at half the edge --
    two refinement rounds for one cloud."""
    _, dense, _ = refinement_clouds()
    cell = 8 * 0.2
    assert _per_cell(dense, cell) > 12.0 and _per_cell(dense, cell / 2) > 12.0 and _per_cell(dense, cell / 4) <= 12.0
    rng = np.random.default_rng(4)
    q = np.concatenate([dense[::97], (dense[rng.integers(0, len(dense), 300)] + rng.normal(0, 0.2, (300, 3))).astype(np.float32)])
    ctx = M.Context(max_scans=1, max_map_points=MM, cell_corner=cell, cell_surf=cell)
    try:
        for kind in range(2):
            ctx.map_set_local(kind, dense)
            _knn_exact(ctx, O, kind, dense, q)
    finally:
        ctx.close()


def test_tagged_cube_map(c, M, O):
    """A tagged cube map of 243 surf points over the 3 cubes that meet at x = y = 25 (the fourth is left empty): the cube stage must
    search the points of the feature's own cube only -- the tags travel with the sort -- and fall back to the local map, a copy
    lifted by 5 cm, where the cube holds too few: the source indices the oracle's two-level association returns, records within
    1e-9."""
    g = np.float32(22.45) + np.float32(0.3) * np.arange(18, dtype=np.float32)
    xx, yy = np.meshgrid(g, g)
    plane = np.stack([xx.ravel(), yy.ravel(), np.float32(60.0) + np.float32(0.02) * np.sin(xx.ravel())], axis=1).astype(np.float32)
    glob = plane[~((plane[:, 0] > 25) & (plane[:, 1] > 25))]
    rng = np.random.default_rng(6)
    glob = glob[rng.permutation(len(glob))]          # the cubes interleaved: the sort has to carry every tag
    cube = M.cube_index(glob)
    assert len(glob) == 243 and len(np.unique(cube)) == 3 and min(np.bincount(cube)[np.unique(cube)]) > 50
    local = (plane + np.array([0, 0, 0.05], np.float32)).astype(np.float32)
    line = np.stack([g, g, np.full(18, 61.0, np.float32)], axis=1).astype(np.float32).repeat(2, axis=0)
    T = perturbed(np.eye(4), dt=(0.01, -0.01, 0.005), rotvec=(0.0005, -0.0005, 0.001))
    feat = plane[rng.integers(0, len(plane), 200)] + np.concatenate([rng.uniform(-0.1, 0.1, (200, 2)), np.zeros((200, 1))], axis=1)
    feat = feat.astype(np.float32)
    c.map_set_local(0, line)
    c.map_set_local(1, local)
    c.map_set_global(1, glob, cube)
    c.features_upload(0, 0, EMPTY)
    c.features_upload(0, 1, feat)
    c.associate(0, 1, T[None], 25.0)
    pf, psrc, pfg = O.associate_planes2(feat, O.CubeMap(glob, cube), O.KdTree(local), T, 25.0)
    gp, gpsrc = c.factors_download(0, 1)
    assert pfg.sum() > 50 and (1 - pfg).sum() > 10                  # both stages
    assert len(np.unique(M.cube_index(feat[psrc[pfg == 1]]))) == 3  # factors from all three cubes
    assert np.array_equal(gpsrc, psrc)
    op = np.concatenate([pf["point_ori"], pf["point_proj"], pf["omega"], pf["error"][:, None]], axis=1)
    assert np.allclose(gp, op, rtol=0, atol=1e-9)
