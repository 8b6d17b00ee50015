"""The four device copies of the trust-region step (csrc/solve.hip: tr_propose / tr_decide on one lane, tr_propose_w1_wave,
tr_propose_w1_regs / tr_decide_w1_regs, tr_propose_wave / tr_decide_wave) replayed on the scripts of tests/tr_cases.py, every
branch of every copy (test_tr_kat.py asserts the census on the host, and the branch codes are compared here): candidates and the
whole digest equal the host's bit for bit -- a NaN where the host has one, of whatever payload, since a NaN's sign and payload
are the processor's choice and nothing ever reads them -- and within the bounds of test_tr_kat.py of the definition.
W = 1 runs the variants 1 to 4, W > 1 the variants 1 and 4; one launch per variant."""
import numpy as np
import pytest

import tr_cases as C
import tr_checks as K
from test_tr_kat import check_against_transcription, logs, scripts, host  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(M):
    return M.Context(max_scans=1)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def assert_equal_to_host(names, h, d, what):
    for q, u, v in zip(("xc", "digest", "digest_i"), h, d):
        if not same(u, v):
            k = int(np.argwhere([not same(u[i], v[i]) for i in range(len(u))])[0][0])
            r = int(np.argwhere([not same(u[k, j], v[k, j]) for j in range(u.shape[1])])[0][0])
            raise AssertionError((what, q, names[k], "round", r, u[k, r], v[k, r]))


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_device_copies_equal_the_host(M, ctx, scripts, host, logs, variant):
    idx = [k for k, s in enumerate(scripts) if s["W"] == 1 or variant in (1, 4)]
    sub = [scripts[k] for k in idx]
    h = tuple(a[idx] for a in host)
    d = M.tr_replay(ctx, variant, sub)
    assert_equal_to_host([s["name"] for s in sub], h, d, "variant %d" % variant)
    check_against_transcription(sub, [logs[k] for k in idx], d, "variant %d" % variant, K.BOUND)


def test_more_scripts_than_compute_units(M, ctx):
    many = C.many_scripts(300)
    h = M.tr_replay(None, 0, many)
    names = [s["name"] for s in many]
    for variant in (1, 4):
        assert_equal_to_host(names, h, M.tr_replay(ctx, variant, many), "variant %d" % variant)
    one = [k for k, s in enumerate(many) if s["W"] == 1]
    for variant in (2, 3):
        assert_equal_to_host([names[k] for k in one], tuple(a[one] for a in h), M.tr_replay(ctx, variant, [many[k] for k in one]),
                             "variant %d" % variant)


def test_one_frame_copies_refuse_windows(M, ctx, scripts):
    w2 = [s for s in scripts if s["W"] == 2][:1]
    for variant in (2, 3):
        with pytest.raises(M.MmlError):
            M.tr_replay(ctx, variant, w2)


# ---- the production kernels against a replay of their own records ------------------------------------------------------------------
def replay_closed_loop(M, c, first, W, x0, T_bl, max_iters, fixed, huber):
    """the solve of slots first .. first + W - 1 as a script: round r's records are mml_linearize_window at the candidate the host
    replay of the rounds before it proposes"""
    recs, x = [], np.asarray(x0, float).reshape(W, 6)
    for _ in range(max_iters + 1):
        recs.append(c.linearize_window(first, W, x, T_bl, w_tan=0.0, huber=huber)[:, :28].copy())
        s = dict(W=W, fixed=int(fixed), max_iters=max_iters, x0=np.asarray(x0, float).reshape(-1), records=np.array(recs))
        xc, dg, di = M.tr_replay(None, 0, [s])
        if not di[0, len(recs) - 1, 5]:
            break
        x = xc[0, len(recs) - 1, :6 * W].reshape(W, 6)
    return s, dg[0], di[0]


def test_solve_kernels_equal_a_replay_of_their_records(M, O, scene):
    """k_solve_wide, k_solve<true> (one-frame problems), k_solve (W = 4, the traced form) and the frame-parallel window solve on
    the scene's slots: the trace and the summary equal the replay of the records mml_linearize_window returns at the traced poses
    -- which ties tr_init and the order of the hook's calls to the kernels' own initialisation and loops -- and the device copy
    that the kernel runs gives the same on that script."""
    import os
    from conftest import perturbed, pose_to_x
    from test_gpu_parity import _setup_estimation
    HUBER = 0.1 / 1.5e-3
    T = np.stack([perturbed(fr["T_gt"]) for fr in scene["frames"]])
    x0 = np.stack([pose_to_x(T[k]) for k in range(4)])
    T_bl = np.eye(4)
    before = os.environ.pop("MML_SOLVE_WIDE", None)
    try:
        for wide in ("1", "0"):
            if wide == "0":
                os.environ["MML_SOLVE_WIDE"] = "0"
            c = M.Context(max_scans=4)
            os.environ.pop("MML_SOLVE_WIDE", None)
            try:
                _setup_estimation(c, O, scene)
                c.associate(0, 4, T, 1.0)
                for fixed in (False, True):
                    # one-frame problems: k_solve_wide (wide) or k_solve<true>
                    s, dg, di = replay_closed_loop(M, c, 1, 1, x0[1], T_bl, 10, fixed, HUBER)
                    xg, sg, tg = c.solve(1, 1, x0[1:2], T_bl, window=1, max_iters=10, fixed=fixed, huber=HUBER, trace=True)
                    R = len(s["records"])
                    assert (sg[0].iterations, sg[0].successful, sg[0].termination) == tuple(int(v) for v in di[R - 1, [0, 1, 4]]), (wide, fixed)
                    assert sg[0].iterations >= 2 and sg[0].final_cost == dg[R - 1, 0] and np.array_equal(xg[0], dg[R - 1, 8:14]), (wide, fixed)
                    for it in range(sg[0].iterations):
                        assert np.array_equal(tg[0, it], dg[min(it + 1, R - 1), 8:14]), (wide, fixed, it)
                    for variant in (3, 2) if wide == "1" else (2,):
                        d = M.tr_replay(c, variant, [s])
                        assert same(d[1][0], dg) and same(d[2][0], di), (variant, fixed)
                    if wide == "0":
                        continue
                    # a window of four frames: k_solve with the trace, the frame-parallel rounds without
                    s, dg, di = replay_closed_loop(M, c, 0, 4, x0, T_bl, 10, fixed, HUBER)
                    R = len(s["records"])
                    xg, sg, tg = c.solve(0, 4, x0, T_bl, window=4, max_iters=10, fixed=fixed, huber=HUBER, trace=True)
                    xp, sp, _ = c.solve(0, 4, x0, T_bl, window=4, max_iters=10, fixed=fixed, huber=HUBER)
                    for who, xs, ss in (("k_solve", xg, sg), ("frame-parallel", xp, sp)):
                        assert (ss[0].iterations, ss[0].successful, ss[0].termination) == tuple(int(v) for v in di[R - 1, [0, 1, 4]]), (who, fixed)
                        assert ss[0].final_cost == dg[R - 1, 0] and np.array_equal(xs.reshape(-1), dg[R - 1, 8:32]), (who, fixed)
                    for it in range(sg[0].iterations):
                        assert np.array_equal(tg[0, it], dg[min(it + 1, R - 1), 8:32]), (fixed, it)
                    for variant in (1, 4):
                        d = M.tr_replay(c, variant, [s])
                        assert same(d[1][0], dg) and same(d[2][0], di), (variant, fixed)
            finally:
                c.close()
    finally:
        os.environ.pop("MML_SOLVE_WIDE", None)
        if before is not None:
            os.environ["MML_SOLVE_WIDE"] = before
