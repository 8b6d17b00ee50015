"""Known answers for the trust-region step of the lidar solves, from the DEFINITION at 80 digits (mpmath), never from the project's
expressions: tests/tr_checks.py states the definition, and its loop (Machine: comparisons and copies only) is run here around an
exact proposal:

    scale   1 / (1 + sqrt(H_ii)) of the records at x0,  A = S H S,  b = S g,  D = sqrt(clamp(A_ii, 1e-6, 1e32))
    gn      the exact solution of (A + mu D^2) y = -b (LU at 80 digits); positive definiteness by the exact Cholesky factorisation
    Cauchy  the exact alpha = |grad|^2 / (grad' D^-1 A D^-1 grad)
    dogleg  the exact root in beta of |a + beta (b - a)|^2 = radius^2 (a negative discriminant: no crossing, the step is invalid)
    model   the exact -(y'b + y'A y / 2)
mu and the radius are doubles by definition (x 10, / 5, x 0.5, max(radius, 3 dogleg_norm) rounded once); x, the cost and every
other value are carried exactly and rounded to double once when stored.

A script of tests/tr_cases.py is REJECTED when one of its decisions is not taken with a margin: |gn| against the radius, alpha |grad|
against the radius, the sign of c and of the discriminant, rel against 1e-3, 0.25 and 0.75, the three tolerances
(relative distance at most 1e3 cond 2^-53), the sign of model_change (1e3 2^-53 of its summed terms) and the smallest eigenvalue
of a damped matrix scaled to a unit diagonal against 0 (1e3 2^-53 of the largest: the guard of the pivot's sign).  At most 10 % may be rejected (asserted).  The radius family (125 exact rounds per script) and the
scripts with NaN / Inf or a NaN scale are not covered.  Data only: tests/golden/tr_kat.npz.

    python tests/golden/make_tr_kat.py [path]          python tests/golden/make_tr_kat.py --measure
"""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tr_cases as C  # noqa: E402
import tr_checks as K  # noqa: E402

mp.mp.dps = 80
RMAX = 12
GUARD = 1e3 * 2.0 ** -53


def scale_mp(rec):
    H, _, _ = K.unpack_H(rec)
    return [[1 / (1 + mp.sqrt(mp.mpf(float(H[f, i, i])))) for i in range(6)] for f in range(len(H))]


def propose_mp(rec, scale, mu, radius):
    H, g, _ = K.unpack_H(rec)
    W = len(H)
    A = [mp.matrix(6, 6) for _ in range(W)]
    b, d = [], []
    for f in range(W):
        for i in range(6):
            for j in range(6):
                A[f][i, j] = mp.mpf(float(H[f, i, j])) * scale[f][i] * scale[f][j]
        b.append([mp.mpf(float(g[f, i])) * scale[f][i] for i in range(6)])
        d.append([mp.sqrt(min(max(A[f][i, i], mp.mpf(1e-6)), mp.mpf(1e32))) for i in range(6)])
    margins, retries, y = [], 0, None
    while mu < 1.0:
        good, ys, cond = True, [], 1.0
        for f in range(W):
            Mx = A[f].copy()
            for i in range(6):
                Mx[i, i] += mp.mpf(mu) * d[f][i] ** 2
            Mf = np.array(Mx.tolist(), float)
            ev = np.linalg.eigvalsh(Mf)
            dj = np.sqrt(np.abs(np.diag(Mf)))  # (Cholesky's pivots are as safe as the matrix scaled to a unit diagonal is definite)
            evs = np.linalg.eigvalsh(Mf / dj[:, None] / dj[None, :])
            margins.append(("pivot", float(evs[0] / max(abs(evs[-1]), 1e-300)) + 1.0, 1.0, 1.0))
            try:
                mp.cholesky(Mx)
            except (ValueError, ZeroDivisionError):
                good = False
                break
            ys.append(mp.lu_solve(Mx, -mp.matrix(b[f])))
            cond = max(cond, float(ev[-1] / ev[0]))
        if good:
            y = ys
            break
        mu *= 10.0
        retries += 1
    out = dict(ok=False, mu=mu, retries=retries, valid=False, margins=margins)
    if y is None:
        return out
    z_gn = [d[f][i] * y[f][i] for f in range(W) for i in range(6)]
    grad = [b[f][i] / d[f][i] for f in range(W) for i in range(6)]
    dd = [d[f][i] for f in range(W) for i in range(6)]

    def quad(v):  # v' blockdiag(A) v
        return sum((mp.matrix(v[6 * f:6 * f + 6]).T * A[f] * mp.matrix(v[6 * f:6 * f + 6]))[0] for f in range(W))

    def dot(u, v):
        return sum(s * t for s, t in zip(u, v))

    gg = dot(grad, grad)
    q = quad([s / t for s, t in zip(grad, dd)])
    if q == 0:
        out.update(ok=True, branch=0, delta=[mp.nan] * (6 * W), dogleg_norm=mp.nan, model_change=mp.nan, cond=cond, u_mc=0.0)
        return out
    alpha = gg / q
    gn_norm, g_norm = mp.sqrt(dot(z_gn, z_gn)), mp.sqrt(gg)
    margins.append(("gn_radius", float(gn_norm), radius, cond))
    z = None
    if gn_norm <= radius:
        z, branch = z_gn, K.GN
    else:
        margins.append(("cauchy_radius", float(g_norm * alpha), radius, cond))
        if g_norm * alpha >= radius:
            z, branch = [-(mp.mpf(radius) / g_norm) * t for t in grad], K.CAUCHY
        else:
            a = [-alpha * t for t in grad]
            v = [s - t for s, t in zip(z_gn, a)]
            aa, av, vv = dot(a, a), dot(a, v), dot(v, v)
            disc = av * av + vv * (mp.mpf(radius) ** 2 - aa)
            margins.append(("c_sign", float(av / mp.sqrt(aa * vv)) + 1.0, 1.0, cond))
            margins.append(("discriminant", float(disc / (av * av + vv * (mp.mpf(radius) ** 2 + aa))) + 1.0, 1.0, cond))
            branch = K.INTERP_NEG if av <= 0 else K.INTERP_POS
            if disc >= 0:
                beta = (-av + mp.sqrt(disc)) / vv
                z = [s + beta * t for s, t in zip(a, v)]
    if z is None:  # the segment passes the sphere by: no step
        out.update(ok=True, branch=branch, cond=cond, u_mc=0.0)
        return out
    yy = [s / t for s, t in zip(z, dd)]
    bb = [b[f][i] for f in range(W) for i in range(6)]
    ss = [scale[f][i] for f in range(W) for i in range(6)]
    mc = -(dot(yy, bb) + quad(yy) / 2)
    u_mc = float(dot([abs(t) for t in yy], [abs(t) for t in bb]) +
                 sum((mp.matrix([abs(t) for t in yy[6 * f:6 * f + 6]]).T * A[f].apply(abs) * mp.matrix([abs(t) for t in yy[6 * f:6 * f + 6]]))[0]
                     for f in range(W)) / 2)
    margins.append(("model_change", float(mc) / u_mc + 1.0, 1.0, 1.0))  # (its sign: rounding of the sums, 1e3 2^-53 of their terms)
    out.update(ok=True, branch=branch, delta=[s * t for s, t in zip(yy, ss)], dogleg_norm=mp.sqrt(dot(z, z)), model_change=mc,
               valid=bool(mc > 0), cond=cond, u_mc=u_mc)
    return out


def decided(margins):
    for name, v, t, cond in margins:
        v, t = float(v), float(t)
        if abs(v - t) <= GUARD * cond * max(abs(v), abs(t)):
            return False, (name, v, t, cond)
    return True, None


def covered(s):
    return s["finite"] and s["family"] != "radius"


def run_exact(s):
    m = K.Machine(s["W"], s["fixed"], s["max_iters"], s["x0"], propose_mp, scale_mp, sqrt=mp.sqrt, num=mp.mpf)
    logs = [m.feed(r) for r in s["records"]]
    ok, why = decided([t for l in logs for t in l["margins"]])
    return logs, ok, why


def pack(scripts, results):
    n = len(results)
    arr = dict(index=np.zeros(n, np.int64), W=np.zeros(n, np.int64), rounds=np.zeros(n, np.int64),
               xc=np.zeros((n, RMAX, 48)), x=np.zeros((n, RMAX, 48)), dogleg_norm=np.zeros((n, RMAX)), model_change=np.zeros((n, RMAX)),
               rel=np.full((n, RMAX), np.nan), cond=np.ones((n, RMAX)), u_mc=np.zeros((n, RMAX)), radius=np.zeros((n, RMAX)),
               state=np.zeros((n, RMAX, 8), np.int64), codes=np.zeros((n, RMAX, 5), np.int64), nprop=np.zeros((n, RMAX), np.int64),
               decide=np.zeros((n, RMAX), np.int64), branch=np.zeros((n, RMAX), np.int64))
    for i, (k, logs) in enumerate(results):
        s = scripts[k]
        arr["index"][i], arr["W"][i], arr["rounds"][i] = k, s["W"], len(logs)
        for r, l in enumerate(logs):
            w6 = 6 * s["W"]
            arr["xc"][i, r, :w6] = [float(t) for t in l["xc"]]
            arr["x"][i, r, :w6] = [float(t) for t in l["x"]]
            arr["dogleg_norm"][i, r], arr["model_change"][i, r] = float(l["dogleg_norm"]), float(l["model_change"])
            if l["rel"] is not None:
                arr["rel"][i, r] = float(l["rel"])
            arr["cond"][i, r], arr["u_mc"][i, r], arr["radius"][i, r], arr["branch"][i, r] = l["cond"], l["u_mc"], l["radius"], l["branch"]
            arr["state"][i, r] = [l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"], l["evaluate"], 0]
            arr["nprop"][i, r], arr["decide"][i, r] = len(l["codes"]), l["decide"]
            arr["codes"][i, r, :min(5, len(l["codes"]))] = l["codes"][:5]
    return arr


def main(path):
    scripts = C.make_scripts()
    results, rejected, total = [], [], 0
    for k, s in enumerate(scripts):
        if not covered(s):
            continue
        total += 1
        logs, ok, why = run_exact(s)
        if ok:
            results.append((k, logs))
        else:
            rejected.append((s["name"], why))
    print("covered %d, rejected %d (%.1f %%)" % (total, len(rejected), 100.0 * len(rejected) / total))
    for r in rejected:
        print("  rejected", r)
    assert len(rejected) <= 0.1 * total, "more than 10 % rejected: change the inputs, not the margin"
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in pack(scripts, results).items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    if "--measure" in sys.argv:
        fix = np.load(os.path.join(here, "tr_kat.npz"))
        scripts = C.make_scripts()
        print(K.measure(fix, scripts, lambda sub: K.replay_np(sub)))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "tr_kat.npz"))
