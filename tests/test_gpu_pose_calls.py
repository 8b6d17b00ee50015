"""mml_estimate and mml_step around the boundary between their two forms (csrc/pose_block.h, mml_pose_packed): up to 16 slots a
call moves its parameter block in one copy and reads k_solve's result records, above that the poses come back from d_x and the
stack sizes from ft_n, and a step of 64 slots or more is cut into one block per lane.  Scans are independent, so a slot's result
may depend neither on the form nor on the call's size, its first slot or its lanes.  Every comparison is byte equality.

Shapes: test_gpu_lazy_undistort.py's four small scans (10 048 points a slot) and their map, replicated over the slots.
17 slots: the first count of the unpacked form.  step(3, 65) on two lanes: pieces of 33 and 32 slots at a first slot that is not 0,
the smallest shape at which a piece's offset into d_pose_in or a short last piece can go wrong."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

from test_gpu_lazy_undistort import GN, _eager_chain, _filled, setup  # noqa: F401  (setup: the module's fixture)

pytestmark = pytest.mark.gpu


def _same(a, b):
    """poses and info of two estimate results, as bytes"""
    return (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            and [bytes(i) for i in a[2]] == [bytes(i) for i in b[2]])


def _rows(r, sl):
    return r[0][sl], r[1][sl], r[2][sl]


@pytest.fixture(scope="module")
def est17(M, setup):
    """A context of 17 slots (slot s holds scan s % 4) after extract, undistort, downsample; start poses; estimate(0, 17)."""
    c, dR, dt, _ = _filled(M, setup, 17)
    try:
        _eager_chain(c, 0, 17, dR, dt)
        T0 = [setup["cases"][s % 4]["T0"] for s in range(17)]
        P0 = np.stack([T[:3, 3] for T in T0])
        Q0 = np.stack([Rsc.from_matrix(T[:3, :3]).as_quat() for T in T0])
        yield c, P0, Q0, c.estimate(0, 17, np.eye(4), P0, Q0)
    finally:
        c.close()


def test_estimate_17_slots_replicas_and_one_at_a_time(est17):
    c, P0, Q0, r17 = est17
    assert all(i.outer_iterations >= 1 and i.n_corner_feat > 0 and i.n_surf_feat > 0 for i in r17[2])
    for s in range(4, 17):
        assert _same(_rows(r17, slice(s, s + 1)), _rows(r17, slice(s % 4, s % 4 + 1))), s
    for s in range(17):
        one = c.estimate(s, 1, np.eye(4), P0[s:s + 1], Q0[s:s + 1])
        assert _same(one, _rows(r17, slice(s, s + 1))), s


def test_estimate_16_and_17_slots_in_one_context(est17):
    c, P0, Q0, r17 = est17
    r16 = c.estimate(0, 16, np.eye(4), P0[:16], Q0[:16])
    assert _same(r16, _rows(r17, slice(0, 16)))


def test_step_65_slots_from_slot_3_on_two_lanes(M, setup):
    B, first, count = 68, 3, 65
    c, dR, dt, x0 = _filled(M, setup, B)
    try:
        sl = slice(first, first + count)
        x2 = c.step(first, count, dR[sl], dt[sl], np.eye(4), 25.0, GN, x0[sl])
        d2 = c.slot_digest(first, count)
        for i in range(4, count):
            assert x2[i].tobytes() == x2[i % 4].tobytes(), i
            assert d2[i].tobytes() == d2[i % 4].tobytes(), i
        assert not np.array_equal(x2, x0[sl])
        c.set_lanes(1)
        x1 = c.step(first, count, dR[sl], dt[sl], np.eye(4), 25.0, GN, x0[sl])
        assert x1.tobytes() == x2.tobytes()
        assert c.slot_digest(first, count).tobytes() == d2.tobytes()
    finally:
        c.close()
