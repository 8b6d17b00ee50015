"""Known answers for the trust-region step of the full-window solve, from the DEFINITION at 80 digits (mpmath) on the dense 15 W
system, never from the project's expressions: tests/fw_tr_checks.py states the definition, and tr_checks.Machine (comparisons and
copies only) is run here around an exact proposal, as tests/golden/make_tr_kat.py does for the lidar solves:

    scale   1 / (1 + sqrt(H_ii)) of the round at x0,  A = S H S,  b = S g,  D = sqrt(clamp(A_ii, 1e-6, 1e32))
    gn      the exact solution of (A + mu D^2) y = -b (LU at 80 digits); positive definiteness by the exact Cholesky factorisation
    Cauchy, dogleg, model   as in make_tr_kat.py, on the whole window
mu and the radius are doubles by definition; x, the cost and every other value are carried exactly and rounded once when stored.

Margin rule (make_tr_kat.py's): a script is REJECTED when one of its decisions is taken without a margin of 1e3 cond 2^-53 (|gn|
and alpha |grad| against the radius, the sign of c and of the discriminant, rel against 1e-3 / 0.25 / 0.75, the tolerances), of
1e3 2^-53 of its summed terms (the sign of model_change) or of 1e3 2^-53 of the largest eigenvalue of the damped matrix scaled to
a unit diagonal (the smallest one against 0: the pivots' sign).  At most 10 % of the covered scripts may be rejected (asserted).

Coverage: every finite script of W <= 3 outside the radius family; for W = 5 and W = 8 the first at most 4 rounds of one script
per proposal class (gn / cauchy / interp) and per decision (an 80-digit LU of n = 120 takes seconds).  Results only, ragged (one
row per round, n values of x and xc per round), compressed: tests/golden/fw_tr_kat.npz; the scripts are regenerated from the seed.

Generation time, measured on the 8 cores it was written on (8 worker processes): see GENERATION_SECONDS below.

    python tests/golden/make_fw_tr_kat.py [path]          python tests/golden/make_fw_tr_kat.py --measure
"""
import multiprocessing
import os
import sys
import time
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fw_tr_cases as C  # noqa: E402
import fw_tr_checks as K  # noqa: E402

GENERATION_SECONDS = 69  # wall time of the last full generation (8 worker processes)
mp.mp.dps = 80
GUARD = 1e3 * 2.0 ** -53
PREFIX = 4  # rounds covered of a W = 5 / W = 8 script


def scale_mp(rec):
    d = np.diag(K.dense(rec[0]))
    return [1 / (1 + mp.sqrt(mp.mpf(float(v)))) for v in d]


def propose_mp(rec, scale, mu, radius):
    H, g = K.dense(rec[0]), np.asarray(rec[1], float)
    n = len(g)
    A = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            if H[i, j] != 0.0:
                A[i, j] = mp.mpf(float(H[i, j])) * scale[i] * scale[j]
    b = [mp.mpf(float(g[i])) * scale[i] for i in range(n)]
    d = [mp.sqrt(min(max(A[i, i], mp.mpf(1e-6)), mp.mpf(1e32))) for i in range(n)]
    margins, retries, y, cond = [], 0, None, 1.0
    while mu < 1.0:
        Mx = A.copy()
        for i in range(n):
            Mx[i, i] += mp.mpf(mu) * d[i] ** 2
        Mf = np.array(Mx.tolist(), float)
        ev = np.linalg.eigvalsh(Mf)
        dj = np.sqrt(np.abs(np.diag(Mf)))  # (Cholesky's pivots are as safe as the matrix scaled to a unit diagonal is definite)
        evs = np.linalg.eigvalsh(Mf / dj[:, None] / dj[None, :])
        margins.append(("pivot", float(evs[0] / max(abs(evs[-1]), 1e-300)) + 1.0, 1.0, 1.0))
        try:
            mp.cholesky(Mx)
            y = mp.lu_solve(Mx, -mp.matrix(b))
            cond = float(ev[-1] / ev[0])
            break
        except (ValueError, ZeroDivisionError):
            mu *= 10.0
            retries += 1
    out = dict(ok=False, mu=mu, retries=retries, valid=False, margins=margins)
    if y is None:
        return out
    y = list(y)

    def quad(v):
        return (mp.matrix(v).T * A * mp.matrix(v))[0]

    def dot(u, v):
        return sum(s * t for s, t in zip(u, v))

    z_gn = [s * t for s, t in zip(d, y)]
    grad = [s / t for s, t in zip(b, d)]
    gg = dot(grad, grad)
    q = quad([s / t for s, t in zip(grad, d)])
    if q == 0:
        out.update(ok=True, branch=0, delta=[mp.nan] * n, dogleg_norm=mp.nan, model_change=mp.nan, cond=cond, u_mc=0.0)
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
    yy = [s / t for s, t in zip(z, d)]
    mc = -(dot(yy, b) + quad(yy) / 2)
    ya = [abs(t) for t in yy]
    u_mc = float(dot(ya, [abs(t) for t in b]) + (mp.matrix(ya).T * A.apply(abs) * mp.matrix(ya))[0] / 2)
    margins.append(("model_change", float(mc) / u_mc + 1.0, 1.0, 1.0))  # (its sign: rounding of the sums, 1e3 2^-53 of their terms)
    out.update(ok=True, branch=branch, delta=[s * t for s, t in zip(yy, scale)], dogleg_norm=mp.sqrt(dot(z, z)), model_change=mc,
               valid=bool(mc > 0), cond=cond, u_mc=u_mc)
    return out


def decided(margins):
    for name, v, t, cond in margins:
        v, t = float(v), float(t)
        if abs(v - t) <= GUARD * cond * max(abs(v), abs(t)):
            return False, (name, v, t, cond)
    return True, None


def coverage(scripts):
    """[(script index, rounds covered)]: all of W <= 3 that is finite and not the radius family; for W = 5, 8 one script per proposal
    class and per decision, chosen with the float64 transcription among the first PREFIX rounds"""
    out = []
    for W in (5, 8):
        want = ["gn", "cauchy", "interp"] + [K.D_PARAM, K.D_FUNC, K.D_GRAD, K.D_REJECT, K.D_SHRINK, K.D_KEEP, K.D_GROW]
        for k, s in enumerate(scripts):
            if s["W"] != W or not s["finite"] or s["family"] == "radius" or not want:
                continue
            logs = K.run_np({**s, "records": s["records"][:PREFIX]})
            have = {K.CLASS[l["branch"]] for l in logs if l["go"] and l["evaluate"]} | {l["decide"] for l in logs}
            if have & set(want):
                want = [w for w in want if w not in have]
                out.append((k, min(PREFIX, len(s["records"]))))
        assert not want, (W, want)
    out += [(k, len(s["records"])) for k, s in enumerate(scripts) if s["W"] <= 3 and s["finite"] and s["family"] != "radius"]
    return sorted(out)


def run_exact(job):
    s, rounds = job
    m = K.machine(s["W"], s["fixed"], s["max_iters"], s["x0"], propose_mp, scale_mp, sqrt=mp.sqrt, num=mp.mpf)
    logs = [m.feed(r) for r in s["records"][:rounds]]
    ok, why = decided([t for l in logs for t in l["margins"]])
    keep = ("xc", "x", "dogleg_norm", "model_change", "rel", "cond", "u_mc", "radius", "branch", "iter", "successful", "num_invalid", "reuse",
            "termination", "go", "evaluate", "codes", "decide")
    slim = []
    for l in logs:
        e = {q: l[q] for q in keep}
        for q in ("xc", "x"):
            e[q] = [float(t) for t in e[q]]
        for q in ("dogleg_norm", "model_change"):
            e[q] = float(e[q])
        e["rel"] = float(e["rel"]) if e["rel"] is not None else float("nan")
        slim.append(e)
    return slim, ok, why


def pack(scripts, results):
    rows = [(k, l) for k, logs in results for l in logs]
    arr = dict(index=np.array([k for k, _ in results], np.int64), name=np.array([scripts[k]["name"] for k, _ in results]),
               rounds=np.array([len(logs) for _, logs in results], np.int64),
               xc=np.concatenate([np.array(l["xc"], float) for _, l in rows]), x=np.concatenate([np.array(l["x"], float) for _, l in rows]),
               dogleg_norm=np.array([l["dogleg_norm"] for _, l in rows]), model_change=np.array([l["model_change"] for _, l in rows]),
               rel=np.array([l["rel"] for _, l in rows]), cond=np.array([float(l["cond"]) for _, l in rows]),
               u_mc=np.array([float(l["u_mc"]) for _, l in rows]), radius=np.array([float(l["radius"]) for _, l in rows]),
               branch=np.array([l["branch"] for _, l in rows], np.int64), decide=np.array([l["decide"] for _, l in rows], np.int64),
               nprop=np.array([len(l["codes"]) for _, l in rows], np.int64),
               state=np.array([[l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"], l["evaluate"], 0]
                               for _, l in rows], np.int64),
               codes=np.array([(l["codes"][:5] + [0] * 5)[:5] for _, l in rows], np.int64))
    return arr


def main(path):
    t0 = time.time()
    scripts = C.make_scripts()
    cover = coverage(scripts)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(run_exact, [(scripts[k], r) for k, r in cover], chunksize=1)
    results, rejected = [], []
    for (k, _), (logs, ok, why) in zip(cover, done):
        if ok:
            results.append((k, logs))
        else:
            rejected.append((scripts[k]["name"], why))
    print("covered %d, rejected %d (%.1f %%)" % (len(cover), len(rejected), 100.0 * len(rejected) / len(cover)))
    for r in rejected:
        print("  rejected", r)
    assert len(rejected) <= 0.1 * len(cover), "more than 10 % rejected: change the inputs, not the margin"
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in pack(scripts, results).items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes, %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    if "--measure" in sys.argv:
        fix = np.load(os.path.join(here, "fw_tr_kat.npz"), allow_pickle=False)
        scripts = C.make_scripts()
        worst = K.check_against_fixture(scripts, K.fixture_logs(fix, scripts), K.replay_np(scripts), "numpy")
        for key, v in sorted(worst.items()):
            print("    %r: %.4g," % (key, v))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "fw_tr_kat.npz"))
