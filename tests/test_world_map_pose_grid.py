"""mml_wm_pose_grid through ctypes, no context: cell counts, index order, the sizing call, MML_ERR_CAPACITY, the dropped duplicate
at half_yaw = pi, the single cell of a zero half extent and the refusals.  The poses are held to 1e-15 absolute of
tests/world_map_score_ref.py pose_grid (math.sin / math.cos); nothing downstream depends on more, because the device tests score
the poses the C function returned."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

import world_map_score_ref as W


def seed_pose():
    T = np.eye(4)
    T[:3, :3] = Rsc.from_rotvec([0.3, -0.2, 0.7]).as_matrix()
    T[:3, 3] = [1.5, -2.25, 0.4]
    return T


def raw(M, seed, a, out, capacity):
    n = C.c_long(-5)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    rc = M.lib().mml_wm_pose_grid(p(seed), *[C.c_double(v) for v in a], p(out), capacity, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("a", [
    (0.6, 0.2, 0.0, 1.0, 0.0, 1.0),                      # 0.6 / 0.2 counts three steps: 7 x 7 cells
    (0.5, 0.2, 0.3, 0.3, 0.5, 0.2),                      # 5 x 5 x 3 x 5
    (1.0, 0.5, 0.0, 0.0, math.pi, math.pi / 8),          # the whole circle: 16 yaw cells, not 17
    (0.0, 0.0, 0.25, 0.1, math.pi, 1.0),                 # pi / 1.0: 3 steps a side, 7 cells, no duplicate
    (0.0, 7.0, 0.0, -1.0, 0.0, 0.0),                     # one cell: the steps of a zero half are not read
    (0.19, 0.2, 0.0, 1.0, 0.1, 0.2),                     # halves below one step: one cell each
])
def test_cells_order_and_poses(M, a):
    seed = seed_pose()
    got = M.wm_pose_grid(seed, *a)
    exp = W.pose_grid(seed, *a)
    kx, kz, kw, nx, nz, nw, cyclic = W.shape(*a)
    assert got.shape == exp.shape == (nx * nx * nz * nw, 4, 4)
    assert nx == 2 * int(math.floor(a[0] / a[1] + 1e-9)) + 1 if a[0] else nx == 1
    assert np.abs(got - exp).max() <= 1e-15
    assert (got[:, 3] == [0.0, 0.0, 0.0, 1.0]).all()
    # the index order: x fastest, then y, then z, then yaw; the centre cell is the seed
    g = got.reshape(nw, nz, nx, nx, 4, 4)
    for iw, iz, iy, ix in [(0, 0, 0, 0), (nw - 1, nz - 1, nx - 1, 0), (kw, kz, kx, kx), (nw // 2, 0, nx - 1, nx // 2)]:
        t = g[iw, iz, iy, ix][:3, 3] - seed[:3, 3]
        assert np.abs(t - [(ix - kx) * a[1], (iy - kx) * a[1], (iz - kz) * a[3]]).max() <= 1e-15
        yaw = (iw - kw) * a[5]
        Rz = np.array([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        assert np.abs(g[iw, iz, iy, ix][:3, :3] - Rz @ seed[:3, :3]).max() <= 1e-15
    assert np.array_equal(g[kw, kz, kx, kx], seed)
    assert (g[..., 2, :3] == seed[2, :3]).all()         # a turn about the world z axis leaves the third row


def test_the_duplicate_at_pi_is_dropped(M):
    seed = seed_pose()
    full = M.wm_pose_grid(seed, 0.0, 1.0, 0.0, 1.0, math.pi, math.pi / 4)
    assert len(full) == 8                                # -pi, -3 pi / 4, ..., 3 pi / 4
    part = M.wm_pose_grid(seed, 0.0, 1.0, 0.0, 1.0, math.pi - 0.01, math.pi / 4)
    assert len(part) == 7                                # three steps a side: the circle is not covered, nothing is dropped
    first, last = full[0][:3, :3], np.diag([math.cos(math.pi), math.cos(math.pi), 1.0]) @ seed[:3, :3]
    assert np.abs(first - last).max() < 1e-15            # the cell that went would have repeated the first
    assert W.shape(0.0, 1.0, 0.0, 1.0, math.pi, math.pi / 4)[6] and not W.shape(0.0, 1.0, 0.0, 1.0, math.pi - 0.01, math.pi / 4)[6]


def test_sizing_capacity_and_refusals(M):
    seed = seed_pose()
    a = (0.5, 0.25, 0.0, 1.0, 0.2, 0.1)                  # 5 x 5 x 1 x 5
    assert raw(M, seed, a, None, 0) == (M.MML_OK, 125)
    out = np.full((125, 16), 7.0)
    assert raw(M, seed, a, out, 124) == (M.MML_ERR_CAPACITY, 125) and (out == 7.0).all()
    assert raw(M, seed, a, out, 125) == (M.MML_OK, 125) and not (out == 7.0).any()
    for bad in [(0.5, 0.0, 0, 1, 0, 1), (0.5, -0.1, 0, 1, 0, 1), (0, 1, 0.5, 0.0, 0, 1), (0, 1, 0, 1, 0.5, -1.0),      # step <= 0
                (math.nan, 0.1, 0, 1, 0, 1), (0.5, math.inf, 0, 1, 0, 1), (0, 1, math.inf, 1, 0, 1), (0, 1, 0, 1, 0, math.nan),
                (-0.5, 0.1, 0, 1, 0, 1), (0, 1, 0, 1, math.pi + 1e-6, 0.1),                                           # half < 0, half_yaw > pi
                (100.0, 0.01, 0, 1, 0, 1)]:                                                                            # 2001^2 cells
        assert raw(M, seed, bad, None, 0) == (M.MML_ERR_INVALID, -5), bad
    for at in (0, 7, 11):
        s = seed.copy()
        s.reshape(16)[at] = math.nan
        assert raw(M, s, a, None, 0) == (M.MML_ERR_INVALID, -5)
    assert raw(M, None, a, None, 0)[0] == M.MML_ERR_INVALID
    assert M.lib().mml_wm_pose_grid(seed.ctypes.data_as(C.c_void_p), *[C.c_double(v) for v in a], None, 0, None) == M.MML_ERR_INVALID
    with pytest.raises(M.MmlError):
        M.wm_pose_grid(seed, 0.5, 0.0)
