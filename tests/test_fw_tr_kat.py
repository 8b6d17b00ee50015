"""CPU suite: the trust-region step of the full-window solve on the host (csrc/window_imu.hip: propose / decide with the dense
cholesky and chol_solve_rcp) driven through every branch by normal equations given in advance (M.fw_replay variant 0,
tests/fw_tr_cases.py), held to the 80-digit fixture tests/golden/fw_tr_kat.npz within fw_tr_checks.BOUND (8 x the worst ratio of
the numpy transcription against the fixture) and to its branch and decision codes exactly.

Census (test_census prints it): per W in 1, 2, 3, 5, 8 every proposal code (Gauss-Newton, Cauchy, both interpolations, solve
failed, model invalid, stop-iter, FAILED; stop-radius for W 1 and 2, where the radius family runs), every decision code, a
proposal with reuse = 1 straight after a rejection; the family pivot reports exactly the aimed number of mu raises, with the
first non-positive pivot of a plain Cholesky (fw_tr_cases.first_bad_pivot) in the aimed column at every mu below.
"""
import collections
import os

import numpy as np
import pytest

import fw_tr_cases as C
import fw_tr_checks as K
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def scripts():
    return C.make_scripts()


@pytest.fixture(scope="module")
def host(M, scripts):
    return M.fw_replay(None, 0, scripts)


@pytest.fixture(scope="module")
def logs(scripts):
    """the exact logs of tests/golden/fw_tr_kat.npz (None for a script the fixture does not cover)"""
    fix = np.load(os.path.join(GOLDEN, "fw_tr_kat.npz"), allow_pickle=False)
    out = K.fixture_logs(fix, scripts)
    n_small = sum(s["W"] <= 3 and s["finite"] and s["family"] != "radius" for s in scripts)
    assert sum(l is not None for l in out) >= 0.9 * n_small
    return out


def codes_of(di, k, r):
    return [int(c) for c in di[k, r, 9:9 + min(int(di[k, r, 8]), 5)]]


def test_numpy_transcription_within_its_bounds(scripts, logs):
    worst = K.check_against_fixture(scripts, logs, K.replay_np(scripts), "numpy", K.BOUND)
    print("numpy, worst ratios:", sorted(worst.items()))
    assert len(worst) == 9
    for key, v in worst.items():  # the table is the measurement: neither stale nor padded
        assert 0.5 * K.MEASURED[key] <= v <= 1.01 * K.MEASURED[key], (key, v, K.MEASURED[key])


def test_host_follows_the_definition(scripts, logs, host):
    worst = K.check_against_fixture(scripts, logs, host, "host", K.BOUND)
    print("host, worst ratios (units of tr_checks):", sorted(worst.items()))
    assert len(worst) == 9  # three quantities in each of the three classes were compared


def test_host_branches_equal_the_transcription_on_every_finite_script(scripts, host):
    """the scripts the fixture does not reach (W = 5, 8 beyond their prefix, the radius family): the float64 transcription's int
    digest -- counters, termination, decision and branch codes -- equals the host's"""
    _, _, ni = K.replay_np(scripts)
    _, _, di = host
    for k, s in enumerate(scripts):
        if s["finite"]:
            R = len(s["records"])
            assert np.array_equal(di[k, :R, :14], ni[k, :R, :14]), s["name"]


def test_census(scripts, host):
    _, dg, di = host
    for W in C.WS:
        code, decide = collections.Counter(), collections.Counter()
        failed = reuse = 0
        pivots = {}
        for k, s in enumerate(scripts):
            if s["W"] != W:
                continue
            R = len(s["records"])
            for r in range(R):
                for c in codes_of(di, k, r):
                    code[c & 15] += 1
                    failed += bool(c & K.FAILED)
                decide[int(di[k, r, 7])] += 1
                # a proposal straight after a rejection reuses gn, grad and alpha
                reuse += r > 0 and int(di[k, r - 1, 3]) == 1 and int(di[k, r, 7]) == K.D_REJECT and int(di[k, r, 8]) == 1 and int(di[k, r, 6]) == 1
            if "aim" in s:
                j, raises = s["aim"]
                c = codes_of(di, k, 1)
                assert len(c) == 1 and (c[0] & 15) <= 4 and (c[0] >> 4) & 15 == raises, (s["name"], c)
                scale = K.scale_np(s["records"][0])
                H = K.dense(s["records"][1][0])
                assert [C.first_bad_pivot(C.damped(H, scale, 1e-8 * 10.0 ** i)) for i in range(raises + 1)] == [j] * raises + [-1], s["name"]
                pivots[j] = pivots.get(j, ()) + (raises,)
        want = [K.GN, K.CAUCHY, K.INTERP_NEG, K.INTERP_POS, K.SOLVE_FAILED, K.MODEL_INVALID, K.STOP_ITER] + ([K.STOP_RADIUS] if W <= 2 else [])
        print("W = %d  proposals %s FAILED %d  decisions %s  reuse-after-reject %d  pivot columns (raises) %s" % (
            W, {K.CODE_NAMES[c]: code[c] for c in want}, failed, {d: decide[d] for d in range(1, 8)}, reuse, sorted(pivots.items())))
        for c in want:
            assert code[c] >= 1, (W, K.CODE_NAMES[c], code)
        for d in (K.D_PARAM, K.D_FUNC, K.D_GRAD, K.D_REJECT, K.D_SHRINK, K.D_KEEP, K.D_GROW):
            assert decide[d] >= 1, (W, "decision", d, decide)
        assert failed >= 1 and reuse >= 5, (W, failed, reuse)
        assert sorted(pivots) == [j for j in C.PIVOT_COLUMNS if j < 15 * W - 1] + [15 * W - 1] and all(v == (1, 3) for v in pivots.values())


def test_uncovered_scripts_end_defined(scripts, host):
    """radius, nonfinite, overflow (and the scripts whose scale is NaN): x is never poisoned, every other value the host returns is
    finite unless the script carries a NaN / Inf, and the nonfinite and overflow scripts whose bad value reaches a solve end in the
    mu ladder: solve failed, then FAILED with x = x0"""
    xc, dg, di = host
    n = collections.Counter()
    for k, s in enumerate(scripts):
        if s["finite"] and s["family"] != "radius":
            continue
        R, m = len(s["records"]), 15 * s["W"]
        fam = s["family"].split("_")[0]
        n[fam] += 1
        last = di[k, R - 1]
        assert 0 <= last[0] <= s["max_iters"] and last[4] in (0, 1, 2, 3, 4), (s["name"], last)
        assert np.all(np.isfinite(dg[k, :R, 8:8 + m])) and np.all(np.isfinite(xc[k, :R, :m])), s["name"]  # x and what is handed back
        assert np.all(dg[k, :R, 8 + m:] == 0.0) and np.all(xc[k, :R, m:] == 0.0), s["name"]
        if s["family"] == "radius":
            assert np.all(np.isfinite(dg[k, :R, :8])) and last[4] == 0 and last[5] == 0, s["name"]
            assert [c for r in range(R) for c in codes_of(di, k, r)][-1] == K.STOP_RADIUS and dg[k, R - 1, 1] < 1e-32, s["name"]
        if last[4] == 4:
            assert last[5] == 0 and np.array_equal(dg[k, R - 1, 8:8 + m], s["x0"]), s["name"]
        bad_at_solve = fam == "overflow" or any(t in s["family"] for t in ("nan_H", "inf_H", "nan_g", "inf_g")) and "later" not in s["family"]
        if bad_at_solve and fam == "nonfinite":  # the bad value sits in the round at x0: no step is ever valid
            assert last[4] == 4 and last[1] == 0 and all((c & 15) in (K.SOLVE_FAILED, K.MODEL_INVALID) for c in codes_of(di, k, 0)), (s["name"], di[k, 0])
        if fam == "overflow":  # the ladder is climbed by a solution that is not finite
            r = 0 if di[k, 0, 4] == 4 else 1
            assert (codes_of(di, k, r)[0] & 15) == K.SOLVE_FAILED and di[k, R - 1, 4] == 4, (s["name"], di[k, :R, :14])
    assert n["nonfinite"] == len(C.NONFINITE) * len(C.WS) and n["overflow"] >= 4 * len(C.WS) and n["radius"] == 4, n


def test_failure_restores_x_init_bit_for_bit(scripts, host):
    _, dg, di = host
    n = 0
    for k, s in enumerate(scripts):
        R, m = len(s["records"]), 15 * s["W"]
        if di[k, R - 1, 4] == 4:
            n += 1
            assert np.array_equal(dg[k, R - 1, 8:8 + m], s["x0"]) and di[k, R - 1, 2] == 5, s["name"]
    assert n >= 20


def test_fullwindow_step_runs_the_same_machine(M, scripts, host):
    """the hook's initialisation and call order are mml_fullwindow_step's: a solver without factors, fed lidar records whose 6 x 6
    blocks and costs make up a script, hands back the hook's candidates bit for bit"""
    rng = np.random.default_rng(7)
    for W in (1, 3):
        recs = []
        for r in range(4):
            rec = np.zeros((W, 32))
            for f in range(W):
                Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
                H = (Q * np.logspace(0, -3, 6)) @ Q.T
                H = 0.5 * (H + H.T)
                rec[f, :21] = H[np.triu_indices(6)]
                rec[f, 21:27] = rng.standard_normal(6) * 0.1
                rec[f, 27] = 1.0 / (r + 1.0)
            recs.append(rec)
        fw = M.FullWindowSolver(W, max_iters=10, fixed=True, huber=0.0, w_tan=3e-4)
        x0 = rng.standard_normal((W, 15))
        rounds = []
        for rec in recs:
            H, g, cost = fw.normal_equations(rec, x0)
            rounds.append((K.band(H), g, cost))
        xc, dg, di = M.fw_replay(None, 0, [dict(W=W, fixed=1, max_iters=10, x0=x0.reshape(-1), records=rounds)])
        x = x0.copy()
        for r, rec in enumerate(recs):
            done, x = fw.step(rec, x)
            assert np.array_equal(np.asarray(x).reshape(-1), xc[0, r, :15 * W]) and bool(done) == (di[0, r, 5] == 0), (W, r)
        s = fw.summary()
        assert (s.iterations, s.successful, s.termination, s.final_cost) == (di[0, 3, 0], di[0, 3, 1], di[0, 3, 4], dg[0, 3, 0])
        assert s.successful >= 1


def test_argument_refusals(M, scripts):
    import ctypes as ct
    lib = M.lib()
    s = scripts[0]
    m = 15 * s["W"]

    def call(hdr, n=1, off=0, length=None, null=None, variant=0):
        hdr = np.array(hdr, np.int32)
        R = max(int(hdr[3]), 1)
        x0, offs = np.zeros(120), np.array([off], np.int64)
        rounds = np.ones(R * (46 * 15 * max(min(int(hdr[0]), 8), 1) + 1))
        xc, dg, di = np.zeros((R, 120)), np.zeros((R, 128)), np.zeros((R, 16), np.int32)
        args = [hdr, x0, offs, rounds, xc, dg, di]
        p = [None if i == null else a.ctypes.data_as(ct.c_void_p) for i, a in enumerate(args)]
        return lib.mml_debug_fw_replay(None, variant, n, p[0], p[1], p[2], p[3], ct.c_longlong(len(rounds) if length is None else length), p[4], p[5], p[6])

    good = [s["W"], 0, 10, 2]
    assert call(good) == M.MML_OK
    for hdr in ([0, 0, 10, 2], [9, 0, 10, 2], [1, 2, 10, 2], [1, 0, -1, 2], [1, 0, 1001, 2], [1, 0, 10, 0], [1, 0, 10, 257]):
        assert call(hdr) == M.MML_ERR_INVALID, hdr
    for null in range(7):
        assert call(good, null=null) == M.MML_ERR_INVALID, null
    assert call(good, off=1) == M.MML_ERR_INVALID and call(good, off=-1) == M.MML_ERR_INVALID  # the script leaves the array
    assert call(good, length=(64 << 20) // 8 + 1) == M.MML_ERR_INVALID                           # more than 64 MB of rounds
    assert call(good, n=-1) == M.MML_ERR_INVALID and call(good, n=1025) == M.MML_ERR_INVALID
    assert call(good, variant=1) == M.MML_ERR_INVALID and call(good, variant=2) == M.MML_ERR_INVALID  # the device needs a context
    with pytest.raises(ValueError):
        M.fw_replay(None, 0, [dict(s, records=[(np.zeros((m, 44)), np.zeros(m), 1.0)])])


def test_header_declares_and_library_exports_the_hook(M):
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    assert "int mml_debug_fw_replay(mml_ctx* ctx, int variant, int n, const int* hdr" in src and "#define MML_FW_DIGEST_DOUBLES 128" in src
    assert hasattr(M.lib(), "mml_debug_fw_replay") and M.FW_DIGEST_DOUBLES == 128
