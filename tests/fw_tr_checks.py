"""The trust-region step of the full-window (IMU_Mode 2) solve -- csrc/window_imu.hip: propose / decide on the host,
csrc/fullwindow_dev.hip: fw_propose / fw_decide / fw_factor_solve on the device -- restated from its DEFINITION on the dense
n x n system, n = 15 W, for tests/test_fw_tr_kat.py, tests/test_gpu_fw_tr_kat.py, tests/fw_tr_cases.py and
tests/golden/make_fw_tr_kat.py.  Nothing here is shared with either copy: the damped system is solved by np.linalg.solve (LU
with pivoting, neither the dense nor the band Cholesky), positive definiteness is np.linalg.cholesky used as a test only, the
quadratic forms are matrix products, the dogleg crossing is the textbook root.  The definition and the units are those of
tr_checks' docstring with A = S H S of the WHOLE window and cond = cond_2(A + mu D^2) of the whole 15 W system; the loop around
the proposal is tr_checks.Machine (comparisons and copies only), told where a round keeps its cost and its gradient.

A round is (band, g, cost): the band of H as k_fw_step holds it, (n, 45), row a, band column c standing for column
15 (a // 15 - 1) + c; dense() / band() convert.  MEASURED / BOUND at the end of this module.
"""
import numpy as np

import tr_checks as K
from tr_checks import (CAUCHY, CLASS, CODE_NAMES, D_FUNC, D_GRAD, D_GROW, D_KEEP, D_PARAM, D_REJECT, D_SHRINK, EPS, FAILED, GN,  # noqa: F401
                       INTERP_NEG, INTERP_POS, MODEL_INVALID, SOLVE_FAILED, STOP_ITER, STOP_RADIUS)


def band_columns(n):
    """(n, 45) column index of every band entry, and the mask of those inside 0 .. n - 1"""
    col = 15 * (np.arange(n)[:, None] // 15 - 1) + np.arange(45)[None, :]
    return col, (col >= 0) & (col < n)


def band(H):
    H = np.asarray(H, float)
    n = len(H)
    col, ok = band_columns(n)
    out = np.zeros((n, 45))
    out[ok] = H[np.nonzero(ok)[0], col[ok]]
    return out


def dense(b):
    b = np.asarray(b, float)
    n = len(b)
    col, ok = band_columns(n)
    H = np.zeros((n, n))
    H[np.nonzero(ok)[0], col[ok]] = b[ok]
    return H


def scale_np(rec):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.sqrt(np.diag(dense(rec[0]))))


def propose_np(rec, scale, mu, radius):
    """One proposal in float64 on the dense system; the dict of tr_checks.propose_np (delta has n entries)."""
    H, g = dense(rec[0]), np.asarray(rec[1], float)
    n = len(g)
    retries, y = 0, None
    with np.errstate(all="ignore"):
        A = H * scale[:, None] * scale[None, :]
        b = g * scale
        d = np.sqrt(np.minimum(np.maximum(np.diag(A), 1e-6), 1e32))
        while mu < 1.0:
            M = A + mu * np.diag(d ** 2)
            good = bool(np.all(np.isfinite(M)) and np.all(np.isfinite(b)))
            if good:
                try:
                    np.linalg.cholesky(M)  # (the test of positive definiteness only)
                    y = np.linalg.solve(M, -b)
                    good = bool(np.all(np.isfinite(y)))
                except np.linalg.LinAlgError:
                    good = False
            if good:
                break
            y = None
            mu *= 10.0
            retries += 1
        out = dict(ok=False, mu=mu, retries=retries, valid=False)
        if y is None:
            return out
        cond = np.linalg.cond(A + mu * np.diag(d ** 2))
        z_gn = d * y
        grad = b / d
        gd = grad / d
        alpha = (grad @ grad) / (gd @ A @ gd)
        gn_norm, g_norm = np.sqrt(z_gn @ z_gn), np.sqrt(grad @ grad)
        if gn_norm <= radius:
            z, branch = z_gn, GN
        elif g_norm * alpha >= radius:
            z, branch = -(radius / g_norm) * grad, CAUCHY
        else:
            a = -alpha * grad
            v = z_gn - a
            aa, av, vv = a @ a, a @ v, v @ v
            disc = np.sqrt(av * av + vv * (radius * radius - aa))
            beta = (disc - av) / vv if av <= 0 else (radius * radius - aa) / (disc + av)
            z, branch = a + beta * v, (INTERP_NEG if av <= 0 else INTERP_POS)
        yy = z / d
        mc = -(yy @ b + 0.5 * (yy @ A @ yy))
        delta = yy * scale
        out.update(ok=True, branch=branch, delta=delta, dogleg_norm=float(np.sqrt(z @ z)), model_change=float(mc), valid=bool(mc > 0.0),
                   cond=float(cond), gn_norm=float(gn_norm), cauchy_norm=float(g_norm * alpha),
                   u_mc=float(np.abs(yy) @ np.abs(b) + 0.5 * np.abs(yy) @ np.abs(A) @ np.abs(yy)), step_norm=float(np.sqrt(delta @ delta)))
    return out


def cost_terms(rec):
    return [rec[2]]


def gradient_max(rec):
    return np.max(np.abs(np.asarray(rec[1], float)))


def machine(W, fixed, max_iters, x0, propose=propose_np, scale_of=scale_np, **kw):
    return K.Machine(W, fixed, max_iters, x0, propose, scale_of, cost_terms=cost_terms, gradient_max=gradient_max, **kw)


def run_np(script):
    m = machine(script["W"], script["fixed"], script["max_iters"], script["x0"])
    return [m.feed(r) for r in script["records"]]


def replay_np(scripts):
    """run_np in the layout of M.fw_replay: (xc, digest, digest_i); scripts that are not finite stay zero"""
    rmax = max(len(s["records"]) for s in scripts)
    xc, dg, di = np.zeros((len(scripts), rmax, 120)), np.zeros((len(scripts), rmax, 128)), np.zeros((len(scripts), rmax, 16), np.int32)
    for k, s in enumerate(scripts):
        if not s["finite"]:
            continue
        n = 15 * s["W"]
        for r, l in enumerate(run_np(s)):
            xc[k, r, :n], dg[k, r, 8:8 + n] = l["xc"], l["x"]
            dg[k, r, :8] = [l["cost"], l["radius"], l["mu"], 0.0, l["dogleg_norm"], l["model_change"], l["step_norm"], l["x_norm"]]
            di[k, r, :9] = [l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"], l["evaluate"], l["decide"],
                            len(l["codes"])]
            di[k, r, 9:9 + min(5, len(l["codes"]))] = l["codes"][:5]
    return xc, dg, di


def fixture_logs(fix, scripts):
    """the rows of tests/golden/fw_tr_kat.npz (ragged: one row per round, n values of x and xc per round) as the logs
    Machine.feed returns, per script (None: not covered by the fixture)"""
    out = [None] * len(scripts)
    row = pos = 0
    for i, k in enumerate(fix["index"]):
        s = scripts[int(k)]
        assert s["name"] == str(fix["name"][i]), (s["name"], fix["name"][i])
        n, logs = 15 * s["W"], []
        for r in range(int(fix["rounds"][i])):
            st = [int(v) for v in fix["state"][row]]
            logs.append(dict(xc=fix["xc"][pos:pos + n], x=fix["x"][pos:pos + n], dogleg_norm=float(fix["dogleg_norm"][row]),
                             model_change=float(fix["model_change"][row]), cond=float(fix["cond"][row]), u_mc=float(fix["u_mc"][row]),
                             radius=float(fix["radius"][row]), branch=int(fix["branch"][row]), decide=int(fix["decide"][row]),
                             codes=[int(c) for c in fix["codes"][row, :int(fix["nprop"][row])]], iter=st[0], successful=st[1],
                             num_invalid=st[2], reuse=st[3], termination=st[4], go=st[5], evaluate=st[6]))
            row += 1
            pos += n
        out[int(k)] = logs
    return out


def check_against_fixture(scripts, logs, out, what, bound=None):
    """branch sequences and the int digest equal the fixture's; candidates, dogleg_norm and model_change within `bound` units of it
    (the units and their carrying forward are tests/test_tr_kat.py's).  Returns the worst ratios by (class, quantity)."""
    import collections
    xc, dg, di = out
    worst = collections.defaultdict(float)
    for k, (s, lg) in enumerate(zip(scripts, logs)):
        if lg is None:
            continue
        n = 15 * s["W"]
        u_x = u_step = u_dn = u_rad = 0.0  # x carries the units of every step accepted so far, the radius those of 3 dogleg_norm
        for r, l in enumerate(lg):
            if l["decide"] in (D_SHRINK, D_KEEP, D_GROW, D_GRAD):
                u_x += u_step
            if l["decide"] == D_GROW:
                u_rad = max(u_rad, 3.0 * u_dn)
            if l["decide"] in (D_SHRINK, D_REJECT):
                u_rad *= 0.5
            got = [int(c) for c in di[k, r, 9:9 + min(int(di[k, r, 8]), 5)]]
            assert got == l["codes"][:5] and int(di[k, r, 8]) == len(l["codes"]) and int(di[k, r, 7]) == l["decide"], (what, s["name"], r, got, l["codes"], int(di[k, r, 7]), l["decide"])
            assert [int(v) for v in di[k, r, :7]] == [l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"],
                                                     l["evaluate"]], (what, s["name"], r)
            if not (l["go"] and l["evaluate"]):
                continue
            x, xe = np.array(l["x"], float), np.array(l["xc"], float)
            cond = l["cond"]
            u_step = EPS * (cond * max(np.max(np.abs(xe - x)), 1e-300) + np.max(np.abs(x)))
            rr = u_rad / float(l["radius"])  # relative unit of the radius: it scales the Cauchy and the interpolated step
            u_xc = u_x + u_step + rr * np.max(np.abs(xe - x))
            u_dn = EPS * cond * l["dogleg_norm"] + u_rad
            ratios = {"xc": np.max(np.abs(xc[k, r, :n] - xe)) / u_xc,
                      "dogleg_norm": abs(dg[k, r, 4] - l["dogleg_norm"]) / u_dn,
                      "model_change": abs(dg[k, r, 5] - l["model_change"]) / (EPS * cond * l["u_mc"] + 2.0 * rr * l["u_mc"])}
            for q, v in ratios.items():
                key = (CLASS[l["branch"]], q)
                worst[key] = max(worst[key], float(v))
                assert bound is None or v <= bound[key], (what, s["name"], r, q, v, bound[key])
    return dict(worst)


# Worst ratios of the float64 transcription (replay_np) against tests/golden/fw_tr_kat.npz, by the class of the proposal's branch
# and by quantity (tests/test_fw_tr_kat.py::test_numpy_transcription_within_its_bounds prints them); BOUND is 8 x, the factor of
# the other known-answer suites.  Measured on numpy alone, never on the library or the device.
MEASURED = {
    ('cauchy', 'dogleg_norm'): 7560,
    ('cauchy', 'model_change'): 4704,
    ('cauchy', 'xc'): 1.267e+04,
    ('gn', 'dogleg_norm'): 1.421,
    ('gn', 'model_change'): 0.5631,
    ('gn', 'xc'): 7016,
    ('interp', 'dogleg_norm'): 1.324e+04,
    ('interp', 'model_change'): 2554,
    ('interp', 'xc'): 1.275e+04,
}
BOUND = {k: 8.0 * v for k, v in MEASURED.items()}
