"""GPU suite: the device's IMU arithmetic (csrc/imu_preint.h in k_imu_preintegrate; csrc/imu_math.h's imu_raw, imu_whiten and
prior_residual in the device-resident full-window solve) against the exact references of tests/golden/imu_kat.npz, with the
checks and the BOUNDS of tests/test_imu_kat.py -- 8 x the numpy oracle's worst ratios, never the device's.
  a. pre-integration: every interval of the fixture through M.imu_preintegrate_batch(..., ctx) in ONE call; the ratios, the
     bounds and the small-angle condition as on the host.  A direct statement about k_imu_preintegrate, not one inherited from
     the byte equality with the host.
  b. cost: windows of W = 2 on two slots with empty factor lists, solved by mml_fullwindow_solve_batch at
     max_num_iterations = 0 in one call: every raw factor item under one of the fixture's real covariances and every whitening
     item (initial_cost = |U r|^2 / 2 exactly, quantities c_*), and every prior item with J = I, r0 = 0 and no IMU factor
     (initial_cost = |dx|^2 / 2, quantities d_c, d_c_tr).  x comes back bit-equal and everything is finite.
For the record (not a bound), the device's worst ratios on the MI355X: p_dp 0.971, p_dv 0.909,
p_dq 0.314, p_dt 0.079, p_jbg 0.915, p_jac 1.230, p_cov 1.428 (small angles against 0.1: p_jbg 0.781 / 0.902, p_cov 1.07 / 1.43);
c_2 0.038, c_10 0.023, c_200 0.012, c_2000 0.018, c_tr 0.989, d_c 0.100, d_c_tr 0.997.
"""
import numpy as np
import pytest

import imu_checks as K

pytestmark = pytest.mark.gpu
NONE = np.zeros((0, 10))


@pytest.fixture(scope="module")
def kat():
    return K.load()


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=2, max_features=512, device=0)
    yield c
    c.close()


def test_device_preintegration_against_exact(M, ctx, kat):
    P = kat["p"]
    pres = M.imu_preintegrate_batch([p["samples"] for p in P], np.stack([p["bg"] for p in P]), np.stack([p["ba"] for p in P]), ctx=ctx)
    R = K.check("device", K.preint_summary(kat, K.library_results(pres)))
    print("device worst ratios:", {k: "%.3f" % K.worst(v) for k, v in R.items()})


def test_device_cost_against_exact(M, ctx, kat):
    for slot in (0, 1):
        for kind in (0, 1):
            ctx.factors_upload(slot, kind, NONE)
    items = K.cost_items(kat)
    solvers, xs = [], []
    for x, p, cov, jac, c, _, _, _ in items:
        fw = M.FullWindowSolver(2, max_iters=0)
        fw.set_imu(1, K.library_record(M, p, cov, jac), K.GRAV)
        solvers.append(fw)
        xs.append(x.reshape(2, 15))
    for it in kat["d"]:
        fw = M.FullWindowSolver(2, max_iters=0)
        pr = M.Prior()
        pr.J[:], pr.r0[:], pr.x0[:] = list(np.eye(15).reshape(-1)), [0.0] * 15, list(it["x0"])
        fw.set_prior(pr)
        solvers.append(fw)
        xs.append(np.stack([it["x"], it["x"]]))
    assert len(solvers) <= 1024
    xo, summ, _ = M.fullwindow_solve_batch(ctx, solvers, [0] * len(solvers), np.eye(4), xs)
    for a, b in zip(xs, xo):
        assert np.array_equal(a, b)
    cost = np.array([s.initial_cost for s in summ])
    assert np.isfinite(cost).all() and np.isfinite([s.final_cost for s in summ]).all()
    R = K.cost_summary(kat, cost[:len(items)])
    for it, got in zip(kat["d"], cost[len(items):]):
        K._worst(R, "d_c" + ("_tr" if it["truncated"] else ""), it["fam"], K.ratio(got - it["cost"], it["u_c"]))
    K.check("device", R, small_angles=False)
    print("device worst ratios:", {k: "%.3f" % K.worst(v) for k, v in R.items()})
