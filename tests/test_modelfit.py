"""CPU suite: the oracle's line / plane model fit (oracle/linalg.h eig3_sym and plane_fit5, fit_line / fit_plane of
oracle/estimate.cpp, through mmlo_model_fit5) against the exact references of tests/golden/modelfit_kat.npz
(tests/golden/make_modelfit_kat.py: rational least squares, 50-digit eigenvalues), family by family.

Bounds.  eps = 2^-52, epsf = 2^-23, |A| = max |entry|, |p| = max |coordinate|, kappa from the exact Gram matrix.  Each
constant is 4 x the oracle's worst ratio over the whole fixture (modelfit_checks.MEASURED, measured here on the CPU,
never on the device):

    quantity                                                        unit of the ratio                    worst   bound
    c_e  eigenvalues |l - l_exact|                                  eps |A|                               10.04   40.2
    c_v  residual ||A v - l v||                                     eps |A|                                9.43   37.7
    c_o  orthonormality ||V'V - I||_F                               eps                                   10.07   40.3
    c_q  QR, full rank: ||X - X_exact||                             eps kappa^2 ||X_exact||                2.30    9.2
    c_r  QR residual | ||A X + 1|| - exact |                        eps sqrt5 (1 + ||A|| ||X||) kappa      0.365   1.5
    c_f  plane pa pb pc (absolute), pd (relative)                   epsf + 4 c_q eps kappa^2               1.25    5.0
    c_p  plane proj                                                 (the same) (|sel| + |pd| + 1)          0.57    2.3
    c_c  line centroid                                              epsf |p|                               1.20    4.8
    c_l  line eigenvalues (float covariance about a float centroid) u = epsf (|A| + |p| sqrt|A|) + (epsf |p|)^2   0.378   1.5
    c_d  sine of the angle between p1 - p2 and the exact direction  u / (ev2 - ev1) + epsf |p| / 0.2 + epsf   0.83   3.3
    c_t  tripod: centre - centroid, | |p1 - p2| - 0.2 |             epsf (|p| + 0.2)                       1.35    5.4

A second seed of the generator (7) gave 8.54 / 8.31 / 9.29 / 2.36 / 0.249 / 1.36 / 0.61 / 1.32 / 0.64 / 0.87 / 0.87 in the same
order: every figure within 2 x of the table's, so the fixture's size stands.

Decisions (line gate, 0.2 gate, rank) must equal the exact ones except on items the generator marked undecidable: exact
margin inside the bands stored in the fixture, which are wider than the bounds above reach (checked below).
"""
import numpy as np
import pytest

import modelfit_checks as K


@pytest.fixture(scope="module")
def kat():
    return K.load()


def check_against_exact(kat, fit, who):
    ratios, flags = K.summary(kat, fit)
    for name, per_family in ratios.items():
        for fam, r in per_family.items():
            print("%s %s %-20s %s" % (who, name, fam, "%8.3f (bound %.1f)" % (r, K.BOUNDS[name]) if r == r else
                                        "no item with an exact value: compared with the oracle only"))
    for name, ok in flags.items():
        assert ok.all(), "%s: %s wrong on items %s" % (who, name, np.flatnonzero(~ok)[:10])
    bad = [(n, f, r) for n, pf in ratios.items() for f, r in pf.items() if r == r and not r <= K.BOUNDS[n]]
    assert all(any(r == r for r in pf.values()) for pf in ratios.values())
    assert not bad, "%s outside the bound: %s" % (who, bad)


def test_bands_cover_the_bounds(kat):
    line_band, plane_band, qr_band, rank_band = kat["bands"]
    assert 4 * K.BOUNDS["c_l"] <= line_band          # ev2 and 3 ev1 each off by the bound
    assert 4 * K.BOUNDS["c_f"] <= plane_band         # three coefficients times a coordinate, plus pd
    assert 3 * K.BOUNDS["c_q"] <= qr_band
    assert rank_band >= 4


def test_oracle_model_fit_against_exact(O, kat):
    check_against_exact(kat, O.model_fit5, "oracle")


def test_oracle_measured_ratios_are_current(O, kat):
    """the docstring's table: no figure of the oracle on this fixture exceeds the measured one the bounds are derived from"""
    ratios, _ = K.summary(kat, O.model_fit5)
    for name, per_family in ratios.items():
        worst = np.nanmax(list(per_family.values()))
        assert worst <= K.MEASURED[name], (name, worst)


def test_batched_entry_equals_the_single_calls(O, kat):
    for m in kat["eig3_in"][::97]:
        A = np.array([[m[0], m[1], m[3]], [m[1], m[2], m[4]], [m[3], m[4], m[5]]])
        ev, V = O.eig3_sym(A)
        o = O.model_fit5(K.EIG3, m[None])[0]
        assert np.array_equal(o[:3], ev) and np.array_equal(o[3:].reshape(3, 3).T, V)
    for a in kat["qr_in"][::97]:
        x, o = O.plane_fit5(a), O.model_fit5(K.QR, a[None])[0]
        assert np.array_equal(o[:3], x, equal_nan=True)


def test_degenerate_conventions(O):
    """What the reference's arithmetic gives on the degenerate neighbourhoods (convention 13)."""
    zero = np.zeros((1, 18), np.float32)
    o = O.model_fit5(K.QR, np.zeros((1, 15)))[0]
    assert o[3] == 3 and not np.isfinite(o[:3]).any()  # 0 < 0 is false: Eigen keeps rank 3 and divides by 0
    p = O.model_fit5(K.PLANE, zero)[0]
    assert p[0] == 1 and np.isnan(p[4:8]).all() and np.isnan(p[8:]).all()   # |NaN| > 0.2 is false: accepted
    same = np.tile(np.float32([3, -2, 1]), 6)[None]
    p = O.model_fit5(K.PLANE, same)[0]
    assert np.isfinite(p[1:4]).all()
    l = O.model_fit5(K.LINE, zero[:, :15])[0]
    assert l[0] == 0 and np.all(l[4:7] == 0)         # 0 > 3 * 0 is false: no line
    with np.errstate(all="ignore"):
        ops = O.model_fit5(K.OPS64, np.array([[2.0, 3.0], [-1.0, 0.0]]))
    assert ops[0, 0] == np.sqrt(2.0) and ops[0, 1] == 2.0 / 3.0 and np.isnan(ops[1, 0]) and ops[1, 1] == -np.inf


def test_gate_families_sit_on_their_gates(O, kat):
    """The threshold families are compared with the oracle alone (device == oracle bit for bit, on the GPU); here: they really
    sit on the gates, and the oracle takes the reference's side of an exact tie."""
    g = kat["qr_fam"] == list(kat["qr_families"]).index("gate_0p2")
    acc = O.model_fit5(K.PLANE, kat["plane_in"][g])[:, 0]
    assert np.abs(kat["plane_margin"][g]).max() < 1e-6 and kat["plane_undecidable"][g].all()
    assert 0.25 * g.sum() < acc.sum() < 0.75 * g.sum()              # a few float ulps either side of 0.2 m
    t = kat["line_fam"] == list(kat["line_families"]).index("gate3_tie")
    o = O.model_fit5(K.LINE, kat["line_in"][t])
    tie = o[:, 6] == 3 * o[:, 5]
    assert tie.sum() >= 20 and not o[tie, 0].any()                  # ev2 > 3 ev1 is strict (Estimator.cpp:253)
    assert o[~tie, 0].any() and not o[~tie, 0].all()
