"""CPU suite: tests/golden/undistort_kat.npz is what tests/undistort_checks.py says it is, and the oracle's mmlo_undistort agrees
with it bit for bit.
  1. every motion family and branch is there, the guard margins are inside [8 B, 5e-14], no coordinate is under 8 B;
  2. mpmath at 50 digits on 32 points per motion (16 of the random set, 16 of the guard set) reproduces the stored floats and margins;
  3. O.undistort equals the stored floats bit for bit on every point, and its double expression restated in numpy
     (undistort_checks.oracle_double) rounds to the same floats;
  4. the oracle's double error re-measured on the points of (2) is <= the stored B (B is the maximum over the generator's 117.6
     million candidates, so a larger value here means the fixture or the oracle changed)."""
import numpy as np
import pytest

import undistort_checks as K


@pytest.fixture(scope="module")
def kat():
    return K.load()


def test_fixture_is_what_it_claims(kat):
    f = kat
    nm = len(f["names"])
    assert nm == 14 and f["dR"].shape == (nm, 9) and f["dt"].shape == (nm, 3)
    th, br, lin, wneg = f["theta"], f["quat_branch"], f["linear"], f["w_negative"]
    assert lin[0] and th[0] == 0 and np.array_equal(f["dR"][0], np.eye(3).reshape(9))            # identity: the linear branch
    assert not lin[1:].any()
    assert 4e-8 < th[1] < 6e-8                                                                    # 1e-7 rad: 1 / sinTheta = 2e7
    assert abs(th[2] - 0.01) < 1e-4 and abs(th[13] - 0.01) < 1e-4                                 # the workload
    assert 0.499 < th[3] < 0.5 < th[4] < 0.501                                                    # either side of theta = 0.5
    assert abs(th[5] - 1.0) < 1e-6
    assert {K.DIAG0, K.DIAG1, K.DIAG2} <= set(br[th > 1.04].tolist()) and (br[th < 1.04] == K.TRACE_POS).all()
    assert any(wneg[m] and abs(th[m] - np.deg2rad(85)) < 1e-6 for m in range(nm))                 # 170 degrees with w < 0
    assert abs(th[11] - np.deg2rad(179.99 / 2)) < 1e-9 and abs(th[12] - np.pi / 2) < 1e-12        # 179.99 degrees and pi
    R = f["dR"].reshape(nm, 3, 3)
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max((1, 2))
    assert (orth[:13] < 1e-15).all() and orth[13] > 1e-9                                          # one float-rounded matrix
    assert np.array_equal(R[13], R[13].astype(np.float32).astype(np.float64))
    B = f["B"]
    assert 1e-16 < B < 3e-15 and K.DECIDABLE * B < K.GUARD_HI / 4
    assert f["margin"].min() >= K.DECIDABLE * B                                                   # every coordinate is decidable
    assert f["xyz"].dtype == f["s"].dtype == f["ref"].dtype == np.float32 and np.isfinite(f["ref"]).all()
    for m in range(nm):
        i = K.of_motion(f, m)
        g = f["guard"][i]
        assert (~g).sum() == 768 and 128 <= g.sum() <= 256 and not g[:768].any()
        lo = f["margin"][i[g]].min(1)
        assert (lo >= K.DECIDABLE * B).all() and (lo <= K.GUARD_HI).all()
        h = np.histogram(np.log(lo), bins=4, range=(np.log(K.DECIDABLE * B), np.log(K.GUARD_HI)))[0]
        assert h.min() >= g.sum() // 8, h                                                         # spread in log, roughly evenly
        xyz, s = f["xyz"][i[~g]], f["s"][i[~g]]
        for v in (0.0, 1.0, 0.5, 1e-6, np.nextafter(np.float32(1), np.float32(0))):
            assert (s == np.float32(v)).any()
        assert (s < 0).any() and (s > 1).any() and s.min() >= -0.05 and s.max() <= 1.05
        rng = np.linalg.norm(xyz, axis=1)
        assert (rng < 1e-3).sum() >= 3 and ((xyz == 0).sum(1) == 1).sum() >= 3
        assert (rng < 1).any() and ((rng > 2) & (rng < 10)).any() and (rng > 12).any()
    assert len(f["xyz"]) * 40 < 800 * 1024


@pytest.fixture(scope="module")
def recomputed(kat):
    """32 points per motion with mpmath: indices, exact values (as doubles hi + lo), floats, margins"""
    f = kat
    A = K.MP(50)
    idx, hi, lo, flt, mg = [], [], [], [], []
    for m in range(len(f["names"])):
        i = K.of_motion(f, m)
        g = f["guard"][i]
        for p in np.concatenate([i[~g][::48], i[g][::max(g.sum() // 16, 1)][:16]]):
            e, info = K.exact_mp(A, f["dR"][m], f["dt"][m], f["xyz"][p], f["s"][p])
            assert (info["quat_branch"], info["linear"], info["w_negative"]) == (f["quat_branch"][m], f["linear"][m], f["w_negative"][m])
            sc = float(K.scale_of(f["xyz"][p], f["dt"][m]))
            fm = [K.margin_mp(A, c, sc) for c in e]
            idx.append(p)
            hi.append([float(c) for c in e])
            lo.append([float(c - A.num(float(c))) for c in e])
            flt.append([r[0] for r in fm])
            mg.append([float(r[1]) for r in fm])
    return np.array(idx), np.array(hi), np.array(lo), np.array(flt, np.float32), np.array(mg)


def test_mpmath_reproduces_floats_and_margins(kat, recomputed):
    idx, _, _, flt, mg = recomputed
    assert len(idx) == 32 * 14
    assert np.array_equal(flt.view(np.uint32), kat["ref"][idx].view(np.uint32))
    assert (np.abs(mg - kat["margin"][idx]) <= 1e-18 + 2.0 ** -24 * mg).all()       # (stored as float32)


def test_oracle_equals_fixture_bit_for_bit(kat, O):
    f = kat
    for m in range(len(f["names"])):
        i = K.of_motion(f, m)
        got = O.undistort(f["xyz"][i], f["s"][i], f["dR"][m], f["dt"][m])
        K.assert_bits(f, got, i, "mmlo_undistort, motion %d" % m)
        K.assert_bits(f, K.oracle_double(f["dR"][m], f["dt"][m], f["xyz"][i], f["s"][i]).astype(np.float32), i, "oracle_double, motion %d" % m)


def test_oracle_error_is_within_the_stored_bound(kat, recomputed):
    f = kat
    idx, hi, lo, _, _ = recomputed
    worst = 0.0
    for m in range(len(f["names"])):
        k = f["motion"][idx] == m
        p = idx[k]
        dbl = K.oracle_double(f["dR"][m], f["dt"][m], f["xyz"][p], f["s"][p])
        err = np.abs((dbl - hi[k]) - lo[k]) / K.scale_of(f["xyz"][p], f["dt"][m])[:, None]
        worst = max(worst, float(err.max()))
    print("oracle double error on %d points: %.3g * scale (B = %.3g)" % (len(idx), worst, f["B"]))
    assert 0 < worst <= f["B"]
