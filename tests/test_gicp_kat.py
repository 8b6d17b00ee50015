"""CPU suite: the oracle's GICP pieces (oracle/gicp.cpp: Problem::eval with computeRDerivative, solve_quadratic, interpolate,
apply_state and the state recovery, one inner BFGS round) against the exact references of tests/golden/gicp_kat.npz
(tests/golden/make_gicp_kat.py: the definitions at 80 digits, the gradient by central differences, no derivative-of-rotation
formula).  tests/test_gpu_gicp_kat.py runs the same checks on the device with the same bounds.

Bounds.  A ratio is an error over its first-order rounding unit (tests/gicp_checks.py, every term commented).  Each bound is
8 x the ORACLE's worst ratio over the whole fixture (gicp_checks.MEASURED, measured here on the CPU, never on the device):

    quantity                                                   worst    bound
    f        objective                                         %(f)s
    g_t      gradient, translation                             %(g_t)s
    g_r      gradient, roll / pitch / yaw                      %(g_r)s
    quad     solve_quadratic, a root                           %(quad)s
    interp   interpolate, the step                             %(interp)s
    state_R  apply_state, an entry of R                        %(state_R)s
    state_x  the angles recovered from the matrix              %(state_x)s
    round_f  fobj of a round against the exact f of its T      %(round_f)s
    cov      covariance I - (1 - 1e-3) u0 u0'                  %(cov)s
    maha     (R C1 R' + C2)^-1                                 %(maha)s

The generator asserts that at the O(1)-angle states every entry of dPhi, dTh, dPsi that is not identically zero (6 + 9 + 6: the
first column of dPhi and the last row of dPsi are zero by definition) moves a gradient component by more than 100 units; with any
single entry negated in a scratch copy of the oracle, test_oracle_objective_against_exact fails (g_r between 8e3 and 2e5 units against a bound of 0.14).

Discrete: the 20 neighbours are the exact set (in the exact order on the lattice, ties by index), the correspondence is the exact
1-NN, a distance equal to the gate is rejected; undecidable items (inside the float rounding band, at most 1 %% per family) may
take either side.
"""
import numpy as np
import pytest

import gicp_checks as K

__doc__ = __doc__ % {k: "%6.3f   %6.2f" % (v, K.BOUNDS[k]) for k, v in K.MEASURED.items()}


@pytest.fixture(scope="module")
def kat():
    return K.load()


@pytest.fixture(scope="module")
def measured(O, kat):
    impl = K.oracle_impl(O)
    r = {}
    K.nn_checks(kat, impl, "oracle")
    r.update(K.cov_ratios(kat, impl, "oracle"))
    r.update(K.corr_ratios(kat, impl, "oracle"))
    r.update(K.eval_ratios(kat, impl, "oracle"))
    r.update(K.quad_ratios(kat, impl, "oracle"))
    r.update(K.interp_ratios(kat, impl, "oracle"))
    r.update(K.state_ratios(kat, impl, "oracle"))
    r.update(K.round_checks(kat, impl, O, "oracle"))
    return r


def test_fixture_covers_what_it_names(kat):
    lists = K.eval_lists()
    assert [n for n, h in lists if len(h) == 0] == list(K.EVAL_M) and len(lists) == 2 * len(K.EVAL_M) + 1
    for n, h in lists[len(K.EVAL_M):-1]:
        assert h[0] == 0 and h[-1] == n - 1 and (n < 600 or {511, 512, 513} <= set(h)) and (n < 1100 or {1023, 1024, 1025} <= set(h))
    assert len(lists[-1][1]) == K.EVAL_N // 2
    assert kat["ev_f"].shape == (len(lists), len(K.EVAL_STATES)) and kat["ev_src"].shape == (K.EVAL_N, 3)
    live = np.ones((3, 3, 3), bool)
    live[0, :, 0] = False
    live[2, 2, :] = False
    assert (kat["ev_seen"][live] > 100).all() and live.sum() == 21
    assert set(kat["q_names"]) == {"q_two_roots", "q_no_root", "q_disc_zero", "q_linear", "q_both_zero", "q_b_zero"}
    assert (kat["q_count"][kat["q_fam"] == kat["q_names"].index("q_disc_zero")] == 2).all()
    mag = np.abs(kat["q_abc"][:, 0][kat["q_abc"][:, 0] != 0])
    assert mag.min() < 1e-11 and mag.max() > 1e5
    assert len(kat["i_names"]) == 14 and np.isnan(kat["i_items"][:, 5]).sum() >= 72
    for k, n in enumerate(kat["i_names"]):
        if n != "i_flat":
            assert kat["i_undecidable"][kat["i_fam"] == k].mean() <= 0.01, n
    x = kat["s_x"]
    assert (np.abs(x[:, 4]) <= 1.5).all() and (np.abs(x[:, 4]) == 1.5).sum() >= 2 and np.signbit(x[1, 3:]).all()
    assert {(a, b, c) for a, b, c in np.sign(x[8:, 3:])} == {(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)}


def test_oracle_neighbours_covariances_correspondences_against_exact(measured):
    """the discrete parts (neighbour sets, tie order on the lattice, correspondences, the gate with d == gate^2 rejected) are
    asserted while `measured` is gathered"""
    K.check_bounds("oracle", {k: measured[k] for k in ("cov", "maha")})


def test_oracle_objective_against_exact(measured):
    K.check_bounds("oracle", {k: measured[k] for k in ("f", "g_t", "g_r")})


def test_oracle_line_search_pieces_against_exact(measured):
    K.check_bounds("oracle", {k: measured[k] for k in ("quad", "interp")})


def test_oracle_state_against_exact(measured):
    K.check_bounds("oracle", {k: measured[k] for k in ("state_R", "state_x")})


def test_oracle_round_properties(measured):
    K.check_bounds("oracle", {"round_f": measured["round_f"]})


def test_oracle_measured_ratios_are_current(measured):
    """the table: no figure of the oracle on this fixture exceeds the measured one the bounds are derived from, and none has fallen
    to less than half of it"""
    print("\n".join("%-8s %8.3f" % kv for kv in measured.items()))
    assert set(measured) == set(K.MEASURED)
    for name, worst in measured.items():
        assert 0.5 * K.MEASURED[name] <= worst <= K.MEASURED[name], (name, worst)
