"""CPU suite: the trust-region step of the lidar solves (csrc/solve.hip: tr_propose / tr_decide, the host build that
mml_window_solver_step runs) driven through EVERY branch by records given in advance (M.tr_replay variant 0, tests/tr_cases.py) and
held to the float64 transcription of the definition in tests/tr_checks.py (np.linalg.solve, no code or expression of solve.hip).

Bounds: tr_checks.BOUND, 8 x the worst ratio of the numpy transcription against the fixture, per branch class and quantity; the
transcription, the host and (test_gpu_tr_kat.py) every device copy are held to them, and their branch sequences to the exact one.

Census: every branch code, every decision and every termination occurs at least 5 times for every W in 1, 2, 3, 8.  An
invalid step followed by a valid one (num_invalid back to 0) is reached by the family "recover" and counted too.
"""
import collections

import numpy as np
import pytest

import tr_cases as C
import tr_checks as K

import os

from conftest import GOLDEN


@pytest.fixture(scope="module")
def scripts():
    return C.make_scripts()


@pytest.fixture(scope="module")
def host(M, scripts):
    return M.tr_replay(None, 0, scripts)


@pytest.fixture(scope="module")
def logs(scripts):
    """the exact logs of tests/golden/tr_kat.npz (None for a script the fixture does not cover)"""
    fix = np.load(os.path.join(GOLDEN, "tr_kat.npz"), allow_pickle=False)
    out = K.fixture_logs(fix, scripts)
    assert sum(l is not None for l in out) >= 550
    return out


def codes_of(di, k, r):
    return [int(c) for c in di[k, r, 9:9 + min(int(di[k, r, 8]), 5)]]


def check_against_transcription(scripts, logs, out, what, bound=None):
    """branch sequences equal, candidates / dogleg_norm / model_change within UNITS units; returns the worst ratios by class"""
    xc, dg, di = out
    worst = collections.defaultdict(float)
    for k, (s, lg) in enumerate(zip(scripts, logs)):
        if lg is None:
            continue
        n = 6 * s["W"]
        u_x = u_step = u_dn = u_rad = 0.0  # x carries the units of every step accepted so far, the radius those of 3 dogleg_norm
        for r, l in enumerate(lg):
            if l["decide"] in (K.D_SHRINK, K.D_KEEP, K.D_GROW, K.D_GRAD):
                u_x += u_step
            if l["decide"] == K.D_GROW:
                u_rad = max(u_rad, 3.0 * u_dn)
            if l["decide"] in (K.D_SHRINK, K.D_REJECT):
                u_rad *= 0.5
            assert codes_of(di, k, r) == l["codes"] and int(di[k, r, 7]) == l["decide"], (what, s["name"], r, codes_of(di, k, r), l["codes"])
            assert [int(v) for v in di[k, r, :7]] == [l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"],
                                                     l["evaluate"]], (what, s["name"], r)
            if not (l["go"] and l["evaluate"]):
                continue
            x, xe = np.array(l["x"], float), np.array(l["xc"], float)
            cond = l["cond"]
            u_step = K.EPS * (cond * max(np.max(np.abs(xe - x)), 1e-300) + np.max(np.abs(x)))
            rr = u_rad / float(l["radius"])  # relative unit of the radius: it scales the Cauchy and the interpolated step
            u_xc = u_x + u_step + rr * np.max(np.abs(xe - x))
            u_dn = K.EPS * cond * l["dogleg_norm"] + u_rad
            ratios = {"xc": np.max(np.abs(xc[k, r, :n] - xe)) / u_xc,
                      "dogleg_norm": abs(dg[k, r, 4] - l["dogleg_norm"]) / u_dn,
                      "model_change": abs(dg[k, r, 5] - l["model_change"]) / (K.EPS * cond * l["u_mc"] + 2.0 * rr * l["u_mc"])}
            for q, v in ratios.items():
                key = (K.CLASS[l["branch"]], q)
                worst[key] = max(worst[key], float(v))
                assert bound is None or v <= bound[key], (what, s["name"], r, q, v, bound[key])
    return dict(worst)


def test_numpy_transcription_within_its_bounds(scripts, logs):
    worst = check_against_transcription(scripts, logs, K.replay_np(scripts), "numpy", K.BOUND)
    print("numpy, worst ratios:", sorted(worst.items()))
    for key, v in worst.items():  # the table is the measurement: neither stale nor padded
        assert 0.5 * K.MEASURED[key] <= v <= 1.01 * K.MEASURED[key], (key, v, K.MEASURED[key])


def test_host_follows_the_definition(scripts, logs, host):
    worst = check_against_transcription(scripts, logs, host, "host", K.BOUND)
    print("worst ratios (units of tr_checks):", sorted(worst.items()))
    assert len(worst) == 9  # three quantities in each of the three classes were compared


def test_census(scripts, host):
    _, _, di = host
    for W in C.WS:
        code, decide, term = collections.Counter(), collections.Counter(), collections.Counter()
        retried_valid = failed = reuse = 0
        for k, s in enumerate(scripts):
            if s["W"] != W:
                continue
            R = len(s["records"])
            for r in range(R):
                for c in codes_of(di, k, r):
                    code[c & 15] += 1
                    retried_valid += (c & 15) <= 4 and (c >> 4) & 15 > 0
                    failed += bool(c & K.FAILED)
                decide[int(di[k, r, 7])] += 1
                # a proposal after a rejection reuses gn, grad and alpha
                reuse += r > 0 and int(di[k, r - 1, 3]) == 1 and int(di[k, r, 7]) == K.D_REJECT and int(di[k, r, 8]) == 1 and int(di[k, r, 6]) == 1
            term[int(di[k, R - 1, 4])] += 1
        for c in (K.GN, K.CAUCHY, K.INTERP_NEG, K.INTERP_POS, K.SOLVE_FAILED, K.MODEL_INVALID, K.STOP_ITER, K.STOP_RADIUS):
            assert code[c] >= 5, (W, K.CODE_NAMES[c], code)
        for d in (K.D_PARAM, K.D_FUNC, K.D_GRAD, K.D_REJECT, K.D_SHRINK, K.D_KEEP, K.D_GROW):
            assert decide[d] >= 5, (W, "decision", d, decide)
        for t in (0, 1, 2, 3, 4):
            assert term[t] >= 5, (W, "termination", t, term)
        recovered = sum(int(di[k, r, 8]) > 1 and int(di[k, r, 6]) == 1 and int(di[k, r, 2]) == 0 for k, s in enumerate(scripts) if s["W"] == W
                        for r in range(len(s["records"])))
        assert retried_valid >= 5 and failed >= 5 and reuse >= 5 and recovered >= 5, (W, retried_valid, failed, reuse, recovered)


def test_clamps_and_mu_are_exercised(scripts, host):
    """the [1e-6, 1e32] clamps: scripts whose scaled diagonal is outside on either side ran a valid step; mu left its floor"""
    _, dg, di = host
    seen = collections.Counter()
    for k, s in enumerate(scripts):
        if s["family"] in ("edge_diag0", "edge_diag_small", "edge_diag_huge"):
            seen[(s["W"], s["family"])] += int(np.any(di[k, 1:len(s["records"]), 6] == 1))
        seen[(s["W"], "mu")] += int(np.any(dg[k, :len(s["records"]), 2] > 1e-8) and di[k, len(s["records"]) - 1, 4] != 4)
    for W in C.WS:
        for f in ("edge_diag0", "edge_diag_small", "edge_diag_huge", "mu"):
            assert seen[(W, f)] >= 2, (W, f, seen)


def test_nonfinite_records_end_defined(scripts, host):
    xc, dg, di = host
    n = 0
    for k, s in enumerate(scripts):
        if s["finite"]:
            continue
        n += 1
        R, W = len(s["records"]), s["W"]
        last = di[k, R - 1]
        assert 0 <= last[0] <= s["max_iters"] and last[4] in (0, 1, 2, 3, 4), (s["name"], last)
        assert np.all(np.isfinite(dg[k, :R, 8:8 + 6 * W])), s["name"]  # x is never poisoned
        if last[4] == 4:
            assert last[5] == 0 and np.array_equal(dg[k, R - 1, 8:8 + 6 * W], s["x0"]), s["name"]
    assert n >= 16 * len(C.WS)


def test_failure_restores_x_init_bit_for_bit(scripts, host):
    _, dg, di = host
    n = 0
    for k, s in enumerate(scripts):
        R, W = len(s["records"]), s["W"]
        if di[k, R - 1, 4] == 4:
            n += 1
            assert np.array_equal(dg[k, R - 1, 8:8 + 6 * W], s["x0"]) and di[k, R - 1, 2] == 5, s["name"]
            assert np.array_equal(dg[k, R - 1, 8 + 6 * W:], np.zeros(48 - 6 * W))
    assert n >= 20


def test_window_solver_step_runs_the_same_machine(M, scripts, host):
    """mml_window_solver_step fed the same records round by round returns the hook's candidates bit for bit"""
    xc, _, di = host
    for k, s in enumerate(scripts):
        W = s["W"]
        ws = M.WindowSolver(W, max_iters=s["max_iters"], fixed=bool(s["fixed"]))
        x = np.array(s["x0"], float)
        for r, rec in enumerate(s["records"]):
            rec32 = np.zeros((W, 32))
            rec32[:, :28] = rec
            done, x = ws.step(rec32, x)
            assert np.array_equal(np.asarray(x).reshape(-1), xc[k, r, :6 * W], equal_nan=True), (s["name"], r)
            assert bool(done) == (di[k, r, 5] == 0), (s["name"], r)
            if done:
                break
        summ = ws.summary()
        assert (summ.iterations, summ.successful, summ.termination) == tuple(int(v) for v in di[k, r, [0, 1, 4]]), s["name"]
