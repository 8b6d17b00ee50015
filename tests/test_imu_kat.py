"""CPU suite: the IMU side of the full-window estimator (csrc/imu_math.h, csrc/imu_preint.h through M.imu_factor,
M.imu_preintegrate, M.imu_preintegrate_batch(ctx=None) and FullWindowSolver.normal_equations) and the numpy oracle
(oracle/imu_oracle.py) against the exact references of tests/golden/imu_kat.npz (tests/golden/make_imu_kat.py: the definitions at
80 digits, Jacobians by central differences there, no Jr or Jr^-1 formula), family by family.

Bounds.  A ratio is an error over its first-order rounding unit (tests/imu_checks.py: eps = 2^-52 times exact operand magnitudes,
no negative power of an angle; the pre-integration's units are its recurrence run on absolute values, times n eps).  Each bound is
8 x the numpy ORACLE's worst ratio over the whole fixture (imu_checks.MEASURED, measured on the CPU, never on the library or the
device; the factor of the lidar suite: the device contracts nothing here, but it chains more operations).  A bound of 0 asks for
the exact value: copies of the record's blocks, +-1, structural zeros.

    quantity                                               worst   family         bound   seed 7
    f_rp    raw residual, position rows                    0.125   thi_3           1.00   0.091
    f_rr    raw residual, rotation rows                    0.020   rpi_1e-9        0.16   0.032
    f_rr_tr   the same at pi - 1e-11 (|qw| < 1e-10)        0.996   rpi_1e-11       7.97   0.995
    f_rv    raw residual, velocity rows                    0.127   thi_3           1.02   0.116
    f_rb    raw residual, bias rows                        0       -               0      0
    f_jp    raw Jacobian, position rows                    0.438   thi_3           3.50   0.500
    f_jr    raw Jacobian, rotation rows                    0.014   thr_0.99e-10    0.11   0.012
    f_jv    raw Jacobian, velocity rows                    0.438   thi_3           3.50   0.500
    f_jb    raw Jacobian, bias rows                        0       -               0      0
    w_r_n   whitened residual, covariance of n samples     0.041 (2), 0.056 (10), 0.042 (200), 0.058 (2000); seed 7 0.036, 0.055, 0.071, 0.052
    w_j_n   whitened Jacobian                              0.085 (2), 0.173 (10), 0.122 (200), 0.052 (2000); seed 7 0.119, 0.114, 0.113, 0.091
    c_n     cost |U r|^2 / 2, all factor items under cov n 0.028 (2), 0.028 (10), 0.012 (200), 0.011 (2000); seed 7 0.040, 0.019, 0.014, 0.014
    c_tr      the same at pi - 1e-11                       0.990   rpi_1e-11       7.92   0.990
    p_dp    pre-integration dp                             0.972   rot_1e-3        7.78   0.984
    p_dv    dv                                             0.910   rot_1e-7        7.28   0.933
    p_dq    dq                                             0.500   rot_1e-3        4.00   0.500
    p_dt    dtime                                          0.079   rot_1.01e-5     0.63   0.078
    p_jbg   jacobian, the gyro-bias columns (carry Jr)     0.955   rot_0.99e-5     7.64   0.834
    p_jac   jacobian, the other columns                    0.972   rot_1e-3        7.78   0.984
    p_cov   covariance                                     1.038   cov             8.30   0.995
    d_g     prior: g = dx                                  0.050   d_pi-1e-3       0.40   0.035
    d_c     prior: cost = |dx|^2 / 2                       0.101   d_3e-4          0.81   0.078
    d_g_tr, d_c_tr  the same at pi - 1e-11                 0.999, 0.998           7.99   0.998, 0.997

Seed 7 of the generator: every figure within 2 x of the table's (the largest gap is w_j_2000, 1.77 x), so the fixture's size stands.
The whitening states its bound per covariance; the condition numbers of the four covariances scaled to a unit diagonal are 17.9,
13.6, 15.4 and 90.2 (1.6e7 to 2.0e9 in the 2-norm, which is scaling, not conditioning) and stand in the units.

The small-angle condition: for the Jacobian rows that carry Jr or Jr^-1 (f_jp, f_jr, f_jv) the worst ratio over the ladder in
(1e-12, 1e-2] is at most 4 x the worst over [0.1, 1], for theta_i = theta_j and for the rotation residual on the ladder; the same
for p_jbg and p_cov over |gyr dt| in (1e-5, 1e-3] against 0.1.  THE FINDING: with a = (1 - cos theta) / theta^2 in so3_Jr and
(1 - cos n) / n in preint_sample_terms, as they were (oracle and library alike), the figures were
    f_jp 22.0 / 0.156, f_jv 21.1 / 0.125, f_jr 4.77 / 1.64 (theta_i ladder, worst at 1.01e-4, just past the series' switch),
    p_jbg 6782 / 1.49, p_cov 3404 / 1.02 (worst at |gyr dt| = 1.01e-5, just past the Jr = I decision),
and the bounds of f_jp, f_jv, f_jr, p_jbg, p_cov failed in the families from 1.01e-4 (1.01e-5) to 1e-2 (1e-3).  With the
coefficient formed as 2 (sin(theta / 2) / theta)^2, resp. 2 sin^2(n / 2) / n, they are 0.156 / 0.156, 0.125 / 0.125,
0.0098 / 0.0056, 0.78 / 0.45, 0.91 / 1.02 (oracle) and 0.156 / 0.156, 0.022 / 0.125, 0.0063 / 0.0044, 0.78 / 0.90, 1.07 / 1.43
(library).  (theta - sin theta) / theta^3 and 1 - sin n / n stay as they are: they multiply [w]x^2 resp. K^2, so their
cancellation is an absolute error of about eps, inside the unit.

Transcribed behaviour, stated and bounded rather than changed: so3_log_q's |qw| < 1e-10 branch (Sophus) returns pi / n and so
drops 2 atan(|qw| / n) of the angle -- 1e-11 rad at pi - 1e-11, where qw = sin(5e-12); at pi - 1e-9 qw = 5e-10 and the branch is
not taken.  The units of the *_tr quantities add this derived truncation, the oracle's log takes the same branch, and their
ratios of 0.99 say that the truncation is all there is.  Likewise the reference's decision Jr = I for |gyr dt| <= 1e-5 is part of
the exact recurrence.

A covariance of ONE sample has rank 12 in exact arithmetic (position and velocity noise are proportional), so it has no
square-root information: the whitening uses 2, 10, 200 and 2000 samples, and the empty interval (covariance 0) must give
MML_ERR_STATE.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import imu_oracle as IO  # noqa: E402
import imu_checks as K  # noqa: E402


@pytest.fixture(scope="module")
def kat():
    return K.load()


def oracle_ratios(kat):
    R = K.factor_summary(kat, K.oracle_raw(IO))
    R.update(K.whiten_summary(kat, K.oracle_whitened(IO)))
    R.update(K.preint_summary(kat, K.oracle_preint(IO, kat)))
    R.update(K.prior_summary(kat, K.oracle_prior(IO)))
    R.update(K.cost_summary(kat, K.oracle_costs(IO, kat)))
    return R


@pytest.fixture(scope="module")
def oracle(kat):
    return oracle_ratios(kat)


def library_ratios(M, kat, batch):
    R = K.factor_summary(kat, K.library_raw(M))
    R.update(K.whiten_summary(kat, K.library_whitened(M)))
    R.update(K.preint_summary(kat, K.library_results(library_preint(M, kat, batch))))
    R.update(K.prior_summary(kat, K.library_prior(M)))
    R.update(K.cost_summary(kat, K.library_costs(M, kat)))
    return R


def library_preint(M, kat, batch, ctx=None):
    P = kat["p"]
    if batch:
        return M.imu_preintegrate_batch([p["samples"] for p in P], np.stack([p["bg"] for p in P]), np.stack([p["ba"] for p in P]), ctx=ctx)
    return [M.imu_preintegrate(p["samples"], p["bg"], p["ba"]) for p in P]


def test_fixture_covers_what_it_names(kat):
    names = kat["f_families"]
    count = lambda n: sum(it["fam"] == n for it in kat["f"])
    assert all(count(n) == K.N_GEOM for n in names) and len(kat["f"]) == K.N_GEOM * (len(K.LADDER_I) + len(K.LADDER_R) + len(K.NEAR_PI) + len(K.DBG) + 3)
    assert {it["pre"]["dt"] for it in kat["f"]} == set(K.DTS)
    norm = lambda v: float(np.sqrt((v * v).sum()))
    for it, qw, qn, br in zip(kat["f"], kat["f_qw"], kat["f_qn"], kat["f_branch"]):
        fam, val = it["fam"].split("_", 1)
        thi, thj, thr = norm(it["x"][3:6]), norm(it["x"][18:21]), norm(it["r"][3:6])
        assert it["has_J"] == (fam != "rpi")
        if fam == "thi":                                       # theta_i = theta_j on the ladder: so3_exp_q's and so3_Jr's switches
            t = float(val)
            assert abs(thi / t - 1) < 1e-6 and abs(thj / t - 1) < 1e-6
            assert (thi * thi < 1e-20) == (t < 1e-10) and (thi * thi < 1e-8) == (t < 1e-4)
        elif fam == "thr":                                     # the rotation residual on the ladder: so3_log_q's and so3_Jr_inv's
            t = float(val)
            assert abs(thr - t) < 1e-15 + 1e-6 * t, (it["fam"], thr)
            assert (qn * qn < 1e-20) == (t < 2e-10) and (thr * thr < 1e-8) == (t < 1e-4)
        elif fam == "rpi":
            assert abs((np.pi - thr) / float(val) - 1) < 1e-3 and (abs(qw) < 1e-10) == (float(val) < 2e-10)
        elif fam == "dbg":
            assert abs(norm(it["x"][9:12] - it["pre"]["bg"]) - float(val)) <= 1e-6 * float(val)
        elif fam == "quat":                                    # m3_to_quat's three branches without the trace
            assert br == 1 + "xyz".index(val)
    assert (kat["f_branch"][[it["fam"].startswith("thi") for it in kat["f"]]] == 0).any()
    # the intervals: lengths, the side of the Jr = I decision for every sample, an interval that turns through more than 180 degrees
    P = kat["p"]
    assert sorted({p["spec"]["n"] for p in P if p["spec"]["fam"] != "cov"}) == list(K.LENGTHS)
    for p, above in zip(P, kat["p_above"]):
        s = p["spec"]
        nrm = np.sqrt((((p["samples"][:, 0:3] - p["bg"]) * p["samples"][:, 6:7]) ** 2).sum(1))
        assert (np.abs(nrm / s["rot"] - 1) < 1e-9).all()
        assert above == (s["n"] if s["rot"] > 1e-5 else 0) and ((nrm > 1e-5) == (s["rot"] > 1e-5)).all()
        assert (p["exact"]["dq"][3] >= 0)
    assert {(p["spec"]["bias"], p["spec"]["jitter"]) for p in P if p["spec"]["n"] >= 31} == {(a, b) for a in (False, True) for b in (False, True)}
    assert max(len(p["samples"]) * p["spec"]["rot"] for p in P) > np.pi and kat["p_angle"].max() <= np.pi
    # the whitening: real covariances, their condition numbers recorded
    assert [P[i]["spec"]["n"] for i in kat["w_interval"]] == list(K.COV_LENGTHS) and (kat["w_cond"] >= 1).all() and (kat["w_cond2"] >= kat["w_cond"]).all()
    # the prior: the ladder and the four angles near pi; |qw| < 1e-10 at pi - 1e-11 alone (qw = sin(delta / 2))
    for it, qw in zip(kat["d"], kat["d_qw"]):
        val = it["fam"][2:]
        thr = norm(it["dx"][3:6])
        if val.startswith("pi-"):
            assert abs((np.pi - thr) / float(val[3:]) - 1) < 1e-3 and (abs(qw) < 1e-10) == (float(val[3:]) < 2e-10)
        else:
            assert abs(thr - float(val)) < 1e-15 + 1e-6 * float(val)


def test_units_hold_no_negative_power_of_theta(kat):
    """the ladder families repeat the same geometries at every angle: up to 1e-2 their units differ by operand rounding alone"""
    worst = []
    for lad in ("thi_", "thr_"):
        fams = [n for n in kat["f_families"] if n.startswith(lad) and float(n[4:]) <= 1e-2]
        assert len(fams) >= 9
        for key in ("u_r", "u_J"):
            u = np.stack([np.stack([it[key].reshape(-1) for it in kat["f"] if it["fam"] == n]) for n in fams])
            live = (u > 0).all(0)
            assert ((u > 0).any(0) == live).all()
            worst.append(float((u.max(0)[live] / u.min(0)[live]).max()))
    print("units across the small-angle families: max / min", worst)
    assert max(worst) < 4.0


def test_oracle_against_exact(oracle):
    K.check("oracle", oracle)


def test_oracle_measured_ratios_are_current(oracle):
    """the docstring's table: no figure of the oracle on this fixture exceeds the measured one the bounds are derived from, and
    none has fallen to less than half of it"""
    assert set(oracle) == set(K.MEASURED)
    for name, per_family in oracle.items():
        w = K.worst(per_family)
        assert 0.5 * K.MEASURED[name] <= w <= K.MEASURED[name], (name, w)


def test_library_single_calls_against_exact(M, kat):
    """M.imu_factor, M.imu_preintegrate (libm's sin / cos in the right Jacobian), FullWindowSolver.normal_equations"""
    K.check("library", library_ratios(M, kat, batch=False))


def test_library_batch_call_against_exact(M, kat):
    """M.imu_preintegrate_batch(ctx=None): the project's own sin / cos; its difference from the single call is reported"""
    R = K.preint_summary(kat, K.library_results(library_preint(M, kat, batch=True)))
    K.check("library batch", R)
    one, many = library_preint(M, kat, batch=False), library_preint(M, kat, batch=True)
    d = [max(np.abs(np.array(a.jacobian) - np.array(b.jacobian)).max(), np.abs(np.array(a.covariance) - np.array(b.covariance)).max()) for a, b in zip(one, many)]
    print("single against batch call, worst |difference| of jacobian and covariance: %.3g on %s" % (max(d), kat["p"][int(np.argmax(d))]["spec"]["name"]))
    for a, b in zip(one, many):
        assert bytes(a)[:8 * 17] == bytes(b)[:8 * 17]          # dp, dv, dq, dtime, bg, ba do not meet the right Jacobian


def test_covariance_that_is_not_positive_definite_is_an_error(M, kat):
    """an empty interval has a zero covariance: the documented error (MML_ERR_STATE), not numbers"""
    p = next(p for p in kat["p"] if p["spec"]["n"] == 0)
    pre = M.imu_preintegrate(p["samples"], p["bg"], p["ba"])
    assert not np.any(np.array(pre.covariance))
    x = kat["w"][0]["x"]
    with pytest.raises(M.MmlError) as e:
        M.imu_factor(pre, K.GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
    assert e.value.code == M.MML_ERR_STATE
