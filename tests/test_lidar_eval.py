"""CPU suite: the oracle's lidar factor evaluation (oracle/estimate.cpp: make_pose / left_jacobian, line_eval, plane_core,
plane_basis, huber, linearize -- through O.line_residual, O.plane_residual and O.linearize on ONE-factor lists) against the
exact references of tests/golden/lidar_eval_kat.npz (tests/golden/make_lidar_eval_kat.py: the factor's definition at 80
digits, Jacobians by central differences there, no left-Jacobian formula), family by family.

Bounds.  A ratio is an error over its first-order rounding unit (tests/lidar_eval_checks.py units(): eps = 2^-52 times exact
operand magnitudes; no negative power of the rotation angle).  Each bound is 8 x the ORACLE's worst ratio over the whole
fixture (lidar_eval_checks.MEASURED, measured here on the CPU, never on the device; 8 rather than the model fit's 4: the device
forms root and inverse root by sqrt_pair at about 1 ulp each, chains four of them, and contracts to FMA):

    quantity                                              worst   family             bound   seed 7
    c_r    residual rows                                  0.944   huber_near_above     7.6   1.065
    c_jt   dr / dt                                        0.677   line_generic         5.4   1.041
    c_jr   dr / dphi                                      0.619   line_near_1e-9       5.0   0.885
    c_htt  H = rho' J'J, translation block                0.892   huber_near_above     7.2   1.041
    c_htr  H, translation x rotation                      0.881   huber_near_above     7.1   0.854
    c_hrr  H, rotation block                              0.870   huber_near_above     7.0   0.885
    c_gt   g = rho' J'r, translation                      0.757   plane_basis_ties     6.1   0.870
    c_gr   g, rotation                                    0.750   plane_basis_ties     6.1   0.870
    c_c    cost = rho / 2                                 0.941   huber_near_above     7.6   0.907

Seed 7 of the generator: every figure within 2 x of the table's (the largest gap is c_jt, 1.54 x), so the fixture's size stands
(a first fixture of 1280 items had c_jt 2.6 x apart between the seeds; the near and generic families grew for it).

The small-angle condition: for c_jt, c_jr, c_htt, c_htr, c_hrr the worst ratio over the rotation families with theta in
[1e-10, 1e-4] is at most 4 x the worst over theta in [1e-2, 1] -- the error must not grow as theta shrinks.  The oracle gives
0.33 / 0.26 (c_jt), 0.23 / 0.15 (c_jr), 0.33 / 0.26, 0.25 / 0.16, 0.23 / 0.15 (H).  With a = (1 - cos theta) / theta^2 in
left_jacobian, as it was, the rotational figures are 7.3e4 / 0.16 (c_jr), 4.7e4 / 0.16 (c_htr) and 5.7e4 / 0.16 (c_hrr), worst at
theta = 1e-9 where a came out as 0, and the bounds of c_jr, c_htr, c_hrr fail in every family from 1e-9 to 1e-4: the finding this
suite was written for.

A second finding: linearize formed a plane factor's H and g from M = S'S = a^2 w w' + b^2 (I - w w'), which holds for a unit
omega; omega is a float vector, and against the rows of plane_residual (the deterministic basis, the definition) H was off by up
to 3600 units (plane_basis_ties).  linearize now sums the rows.

Decisions.  An excluded record (!(|error| > 1e-5), NaN included) contributes exactly nothing; a point exactly on its line has
zero rows and one exactly on its line or plane a zero residual, g and cost -- zeros, not small numbers (on its plane the row
itself is S dP/dx: |d| d is differentiable at 0); the Huber branch equals the exact one on every item whose exact |s - delta^2|
is outside the band stored in the fixture, which is wider than the bound on s reaches (checked below).
"""
import numpy as np
import pytest

import lidar_eval_checks as K


@pytest.fixture(scope="module")
def kat():
    return K.load()


def test_fixture_covers_what_it_names(kat):
    names = kat["families"]
    count = lambda n: int((kat["fam"] == names.index(n)).sum())
    small, large = K.theta_classes(kat)
    assert len(small) == 7 and len(large) == 3
    assert 1400 <= len(kat["kind"]) <= 1800
    assert kat["zero"].sum() == count("line_on") == 12 and (kat["dist"] == 0).sum() == 24
    g = kat["fam"] == names.index("gate")
    err = kat["rec"][g, 9]
    assert set(np.unique(err[~np.isnan(err)])) == {-1e-5, 0.0, 1e-5, np.nextafter(1e-5, 1.0)} and np.isnan(err).any()
    assert np.array_equal(kat["excluded"][g], ~(np.abs(err) > 1e-5)) and not kat["excluded"][~g].any()
    rel = kat["margin"] / kat["delta"] ** 2
    for n, lo, hi in (("huber_far_below", -1.0, -0.99), ("huber_near_below", -2e-3, -5e-10), ("huber_near_above", 5e-10, 2e-3),
                      ("huber_10x", 8.9, 9.1), ("huber_1e6x", 0.99e6, 1.01e6)):
        r = rel[kat["fam"] == names.index(n)]
        assert (r > lo).all() and (r < hi).all(), (n, r.min(), r.max())
    assert (kat["delta"][kat["fam"] == names.index("huber_off")] == 0).all()
    w = kat["rec"][kat["fam"] == names.index("plane_basis_ties"), 6:9]
    a = np.abs(w)
    branch = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
    assert set(branch) == {0, 1, 2} and ((a[:, 0] == a[:, 1]) | (a[:, 1] == a[:, 2]) | (a[:, 0] == a[:, 2])).sum() >= 12
    one = kat["fam"] == names.index("one_pose")
    assert one.sum() == 260 and (kat["x"][one] == kat["x"][one][0]).all() and (kat["tbl"][one] == 1).all() and (kat["w_tan"][one] == 0).all()
    weight = 1 - 0.9 * kat["dist"] / np.sqrt(np.linalg.norm(kat["P"], axis=1))
    assert (weight[kat["fam"] == names.index("line_small_range")] < 0).any() and np.linalg.norm(kat["P"], axis=1).min() < 2e-2


def test_bands_cover_the_bounds(kat):
    """s = sum r^2 is off by at most the rows' bound in its own unit (u_s is the first-order image of u_r), the branch compares it
    with delta^2 rounded once; the undecidable band is wider, and at most 1 % of the Huber families is inside it"""
    assert K.BOUNDS["c_r"] + 1 <= kat["band"]
    hub = np.array([kat["families"][i].startswith("huber_") and kat["families"][i] != "huber_off" for i in kat["fam"]])   # (delta > 0)
    assert hub.sum() == 192 and (kat["delta"][hub] > 0).all()
    assert kat["undecidable"][hub].mean() <= 0.01


def test_oracle_rows_against_exact(O, kat):
    ratios, flags = K.row_summary(kat, K.oracle_rows(O, kat))
    bad = K.report("oracle", ratios)
    K.check_flags("oracle", flags)
    K.check_small_angles("oracle", kat, ratios)
    assert not bad, "oracle outside the bound: %s" % bad


def test_oracle_linearize_against_exact(O, kat):
    K.check_against_exact(kat, K.oracle_evaluate(O, kat), "oracle")


def test_oracle_measured_ratios_are_current(O, kat):
    """the docstring's table: no figure of the oracle on this fixture exceeds the measured one the bounds are derived from, and
    none has fallen to less than half of it (the table would then claim more room than the oracle needs)"""
    ratios, _ = K.row_summary(kat, K.oracle_rows(O, kat))
    ratios.update(K.summary(kat, K.oracle_evaluate(O, kat))[0])
    assert set(ratios) == set(K.MEASURED)
    for name, per_family in ratios.items():
        worst = np.nanmax(list(per_family.values()))
        assert 0.5 * K.MEASURED[name] <= worst <= K.MEASURED[name], (name, worst)


def test_units_hold_no_negative_power_of_theta(kat):
    """the rotation families repeat the same geometries at every theta: between the families from 1e-10 to 1e-4 the units of the
    Jacobian and of H differ by the translation's rounding alone"""
    small, _ = K.theta_classes(kat)
    worst = []
    for key in ("u_J", "u_H"):
        u = np.stack([kat[key][kat["fam"] == kat["families"].index(n)].reshape(36, -1) for n in small])
        live = (u > 0).all(0)
        worst.append((u.max(0)[live] / u.min(0)[live]).max())
    print("units across the small-angle families: max / min", worst)
    assert max(worst) < 4.0
