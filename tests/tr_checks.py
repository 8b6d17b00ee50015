"""The trust-region step of the lidar solves (csrc/solve.hip: Ceres' loop with TRADITIONAL_DOGLEG and Jacobi scaling) restated from
its DEFINITION, for tests/test_tr_kat.py, tests/test_gpu_tr_kat.py, tests/tr_cases.py and tests/golden/make_tr_kat.py.  Nothing
here is shared with solve.hip: the damped system is solved by np.linalg.solve (LU with pivoting, not the code's Cholesky), the
quadratic forms are matrix products, the dogleg crossing is the root of |a + beta (b - a)|^2 = radius^2 by the textbook formula.

    scale   s_i = 1 / (1 + sqrt(H_ii)) of the records at x0 (fixed for the solve),  A = S H S,  b = S g
    D       d_i = sqrt(min(max(A_ii, 1e-6), 1e32))
    gn      in the coordinates z = D y:  z_gn = D y,  (A + mu D^2) y = -b;  mu is raised by 10 while the matrix is not positive
            definite (or the solve is not finite), up to mu >= 1: the solve has failed
    grad    D^-1 b;  the Cauchy point is -alpha grad,  alpha = |grad|^2 / (grad' D^-1 A D^-1 grad)
    dogleg  z_gn if |z_gn| <= radius;  -radius grad / |grad| if alpha |grad| >= radius;  otherwise the point of the segment from the
            Cauchy point to z_gn on the sphere
    step    delta = S D^-1 z,  model_change = -(y' b + y' A y / 2) for y = D^-1 z,  step_norm = |delta|

The loop around it (Machine) is shared by the float64 transcription (propose_np) and the 80-digit one of make_tr_kat.py: it only
compares and copies.  mu and the radius' halving are part of the algorithm's definition and are formed in doubles everywhere.

Units (first order in eps = 2^-53, from the data, per proposal; cond = cond_2(A + mu D^2)):
    u_xc     eps (cond max|delta| + max|x|) + the same of every step accepted before: x carries their errors
    u_dn     eps cond dogleg_norm
    u_mc     eps cond (|y|'|b| + |y|'|A||y| / 2)
(rel = (cost - cand) / model_change is logged; the decisions it leads to are compared as branch codes.)
A ratio is an error over its unit; tests/test_tr_kat.py carries the units of the accepted steps and of the radius forward (x and
the radius inherit them).  MEASURED / BOUND at the end of this module.
"""
import numpy as np

EPS = 2.0 ** -53
IU = np.triu_indices(6)

# branch codes of include/mmloam_hip.h
GN, CAUCHY, INTERP_NEG, INTERP_POS, SOLVE_FAILED, MODEL_INVALID, STOP_ITER, STOP_RADIUS, FAILED = 1, 2, 3, 4, 5, 6, 8, 9, 256
D_PARAM, D_FUNC, D_GRAD, D_REJECT, D_SHRINK, D_KEEP, D_GROW = 1, 2, 3, 4, 5, 6, 7
CODE_NAMES = {GN: "gauss_newton", CAUCHY: "cauchy", INTERP_NEG: "interp_c<=0", INTERP_POS: "interp_c>0", SOLVE_FAILED: "solve_failed",
              MODEL_INVALID: "model_invalid", STOP_ITER: "stop_iter", STOP_RADIUS: "stop_radius"}


def unpack_H(rec):
    """(W, 28) records -> (W, 6, 6) symmetric H, (W, 6) g, (W,) cost"""
    rec = np.asarray(rec, float)
    H = np.zeros((len(rec), 6, 6))
    H[:, IU[0], IU[1]] = rec[:, :21]
    H[:, IU[1], IU[0]] = rec[:, :21]
    return H, rec[:, 21:27].copy(), rec[:, 27].copy()


def pack_record(H, g, cost):
    r = np.zeros(28)
    r[:21] = np.asarray(H)[IU]
    r[21:27] = g
    r[27] = cost
    return r


def scale_np(rec):
    H, _, _ = unpack_H(rec)
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.sqrt(np.einsum("fii->fi", H)))


def propose_np(rec, scale, mu, radius):
    """One proposal in float64.  Returns a dict: ok, mu (after the ladder), retries, and for ok: branch, delta (W, 6), dogleg_norm,
    model_change, step quantities for the units."""
    H, g, _ = unpack_H(rec)
    W = len(H)
    with np.errstate(all="ignore"):
        A = H * scale[:, :, None] * scale[:, None, :]
        b = g * scale
        d = np.sqrt(np.minimum(np.maximum(np.einsum("fii->fi", A), 1e-6), 1e32))
    retries = 0
    y = None
    with np.errstate(all="ignore"):
        while mu < 1.0:
            good = True
            ys = []
            for f in range(W):
                M = A[f] + mu * np.diag(d[f] ** 2)
                if not np.all(np.isfinite(M)) or not np.all(np.isfinite(b[f])):
                    good = False
                    break
                try:
                    np.linalg.cholesky(M)  # (the test of positive definiteness only)
                    ys.append(np.linalg.solve(M, -b[f]))
                except np.linalg.LinAlgError:
                    good = False
                    break
                if not np.all(np.isfinite(ys[-1])):
                    good = False
                    break
            if good:
                y = np.array(ys)
                break
            mu *= 10.0
            retries += 1
        out = dict(ok=False, mu=mu, retries=retries, valid=False)
        if y is None:
            return out
        cond = max(np.linalg.cond(A[f] + mu * np.diag(d[f] ** 2)) for f in range(W))
        z_gn = d * y
        grad = b / d
        gd = grad / d
        q = sum(gd[f] @ A[f] @ gd[f] for f in range(W))
        alpha = np.sum(grad * grad) / q
        gn_norm, g_norm = np.sqrt(np.sum(z_gn * z_gn)), np.sqrt(np.sum(grad * grad))
        if gn_norm <= radius:
            z, branch = z_gn, GN
        elif g_norm * alpha >= radius:
            z, branch = -(radius / g_norm) * grad, CAUCHY
        else:
            a = -alpha * grad
            v = z_gn - a
            aa, av, vv = np.sum(a * a), np.sum(a * v), np.sum(v * v)
            disc = np.sqrt(av * av + vv * (radius * radius - aa))
            beta = (disc - av) / vv if av <= 0 else (radius * radius - aa) / (disc + av)
            z, branch = a + beta * v, (INTERP_NEG if av <= 0 else INTERP_POS)
        yy = z / d
        lin = sum(yy[f] @ b[f] for f in range(W))
        quad = sum(yy[f] @ A[f] @ yy[f] for f in range(W))
        mc = -(lin + 0.5 * quad)
        delta = yy * scale
        out.update(ok=True, branch=branch, delta=delta, dogleg_norm=float(np.sqrt(np.sum(z * z))), model_change=float(mc),
                   valid=bool(mc > 0.0), cond=float(cond), gn_norm=float(gn_norm), cauchy_norm=float(g_norm * alpha), gn_ratio=float(gn_norm / radius), cauchy_ratio=float(g_norm * alpha / radius),
                   u_mc=float(sum(np.abs(yy[f]) @ np.abs(b[f]) + 0.5 * np.abs(yy[f]) @ np.abs(A[f]) @ np.abs(yy[f]) for f in range(W))),
                   step_norm=float(np.sqrt(np.sum(delta * delta))))
    return out


class Machine:
    """Ceres' trust-region loop around a proposal function, round by round as the replay hook runs it.  Values are whatever the
    proposal returns (floats, or mpmath numbers in make_tr_kat.py); feed() returns the round's log."""

    def __init__(self, W, fixed, max_iters, x0, propose, scale_of, sqrt=np.sqrt, num=float, cost_terms=None, gradient_max=None):
        self.W, self.fixed, self.max_iters, self.propose, self.scale_of, self.sqrt, self.num = W, fixed, max_iters, propose, scale_of, sqrt, num
        # how the cost's terms and the largest gradient entry are read out of a round's record (the default: W 28-double records;
        # fw_tr_checks.py passes its own for the full-window rounds)
        self.cost_terms = cost_terms if cost_terms is not None else (lambda rec: np.asarray(rec, float)[:, 27])
        self.gradient_max = gradient_max if gradient_max is not None else (lambda rec: np.max(np.abs(np.asarray(rec, float)[:, 21:27])))
        self.x = [num(v) for v in np.asarray(x0, float).reshape(-1)]
        self.x_init = list(self.x)
        self.round = -1

    def _norm(self, v):
        return self.sqrt(sum((t * t for t in v), self.num(0)))

    def feed(self, rec):
        self.round += 1
        log = dict(decide=0, codes=[], rel=None, margins=[])
        if self.round == 0:
            self.rec, self.scale = rec, self.scale_of(rec)
            self.cost = sum((self.num(c) for c in self.cost_terms(rec)), self.num(0))
            self.x_norm = self._norm(self.x)
            self.radius, self.mu = 1e4, 1e-8
            self.num_invalid = self.iter = self.successful = self.termination = 0
            self.go, self.evaluate, self.reuse = 1, 0, 0
            self.dogleg_norm = self.model_change = self.step_norm = self.num(0)
            self.xc = list(self.x)
            if not self.fixed:
                gm = self.gradient_max(rec)
                log["margins"].append(("gradient_tol", gm, 1e-10, 1.0))
                if gm <= 1e-10:
                    self.termination, self.go = 1, 0
        elif self.go:
            self._decide(rec, log)
        while self.go:
            self._propose(log)
            if not self.go or self.evaluate:
                break
        log.update(xc=list(self.xc if self.go and self.evaluate else self.x), x=list(self.x), cost=self.cost, radius=self.radius, mu=self.mu,
                   dogleg_norm=self.dogleg_norm, model_change=self.model_change, step_norm=self.step_norm, x_norm=self.x_norm,
                   iter=self.iter, successful=self.successful, num_invalid=self.num_invalid, termination=self.termination, go=self.go,
                   evaluate=self.evaluate, reuse=self.reuse, cond=getattr(self, "cond", 1.0), u_mc=getattr(self, "u_mc", 0.0),
                   branch=getattr(self, "branch", 0))
        return log

    def _decide(self, rec, log):
        cand = sum((self.num(c) for c in self.cost_terms(rec)), self.num(0))
        cond = self.cond
        if not self.fixed:
            thr = 1e-8 * (self.x_norm + 1e-8)
            log["margins"].append(("parameter_tol", self.step_norm, thr, cond))
            if self.step_norm <= thr:
                self.termination, self.go, log["decide"] = 2, 0, D_PARAM
                return
            log["margins"].append(("function_tol", abs(self.cost - cand), 1e-6 * self.cost, 1.0))
            if abs(self.cost - cand) <= 1e-6 * self.cost:
                self.termination, self.go, log["decide"] = 3, 0, D_FUNC
                return
        rel = (self.cost - cand) / self.model_change
        log["rel"] = rel
        log["u_rel_num"] = abs(float(self.cost)) + abs(float(cand))
        for t in (1e-3, 0.25, 0.75):
            log["margins"].append(("rel_%g" % t, rel, t, cond))
            # (and the cancellation in cost - cand, both sums of W doubles: the distance in units of |cost| + |cand|)
            tt = abs(self.cost) + abs(cand)
            log["margins"].append(("rel_sum_%g" % t, self.cost - cand - t * self.model_change + tt, tt, 1.0))
        if rel > 1e-3:
            self.x = list(self.xc)
            self.x_norm = self._norm(self.x)
            self.rec, self.cost = rec, cand
            self.successful += 1
            if not self.fixed:
                gm = self.gradient_max(rec)
                log["margins"].append(("gradient_tol", gm, 1e-10, 1.0))
                if gm <= 1e-10:
                    self.termination, self.go, log["decide"] = 1, 0, D_GRAD
                    return
            log["decide"] = D_SHRINK if rel < 0.25 else D_GROW if rel > 0.75 else D_KEEP
            if rel < 0.25:
                self.radius = self.radius * 0.5
            if rel > 0.75:
                self.radius = max(self.radius, float(3.0 * self.dogleg_norm))  # (the radius is a double: rounded once)
            self.mu = max(1e-8, 2.0 * self.mu / 10.0)
            self.reuse = 0
        else:
            self.radius = self.radius * 0.5
            self.reuse = 1
            log["decide"] = D_REJECT

    def _propose(self, log):
        self.evaluate = 0
        if self.iter >= self.max_iters or self.radius < 1e-32:
            log["codes"].append(STOP_ITER if self.iter >= self.max_iters else STOP_RADIUS)
            self.go = 0
            return
        self.iter += 1
        log["reused"] = log.get("reused", 0) + self.reuse  # (a proposal that keeps gn, grad and alpha)
        self.reuse = 1
        p = self.propose(self.rec, self.scale, self.mu, self.radius)
        self.mu = p["mu"]
        log["margins"] += p.get("margins", [])
        if not (p["ok"] and p["valid"]):
            self.num_invalid += 1
            code = (MODEL_INVALID if p["ok"] else SOLVE_FAILED) + 16 * p["retries"]
            if self.num_invalid >= 5:
                self.x = list(self.x_init)
                self.termination, self.go = 4, 0
                code += FAILED
            else:
                self.mu *= 10.0
                self.reuse = 0
            log["codes"].append(code)
            return
        log["codes"].append(p["branch"] + 16 * p["retries"])
        self.num_invalid = 0
        delta = [self.num(v) if not isinstance(v, self.num) else v for v in np.asarray(p["delta"], dtype=object).reshape(-1)]
        self.xc = [a + b for a, b in zip(self.x, delta)]
        self.delta = delta
        self.step_norm = self._norm(delta)
        self.dogleg_norm, self.model_change = p["dogleg_norm"], p["model_change"]
        self.cond, self.u_mc, self.branch = p["cond"], p["u_mc"], p["branch"]
        self.evaluate = 1


def machine_np(script):
    return Machine(script["W"], script["fixed"], script["max_iters"], script["x0"], propose_np, scale_np)


def run_np(script):
    m = machine_np(script)
    return [m.feed(r) for r in script["records"]]


CLASS = {GN: "gn", CAUCHY: "cauchy", INTERP_NEG: "interp", INTERP_POS: "interp"}


def fixture_logs(fix, scripts):
    """the rows of tests/golden/tr_kat.npz as the logs Machine.feed returns, per script (None: not covered by the fixture)"""
    out = [None] * len(scripts)
    for i, k in enumerate(fix["index"]):
        n, logs = 6 * int(fix["W"][i]), []
        for r in range(int(fix["rounds"][i])):
            st = [int(v) for v in fix["state"][i, r]]
            logs.append(dict(xc=fix["xc"][i, r, :n], x=fix["x"][i, r, :n], dogleg_norm=float(fix["dogleg_norm"][i, r]),
                             model_change=float(fix["model_change"][i, r]), cond=float(fix["cond"][i, r]), u_mc=float(fix["u_mc"][i, r]),
                             radius=float(fix["radius"][i, r]), branch=int(fix["branch"][i, r]), decide=int(fix["decide"][i, r]),
                             codes=[int(c) for c in fix["codes"][i, r, :int(fix["nprop"][i, r])]], iter=st[0], successful=st[1],
                             num_invalid=st[2], reuse=st[3], termination=st[4], go=st[5], evaluate=st[6]))
        out[int(k)] = logs
    return out


def replay_np(scripts):
    """run_np in the layout of M.tr_replay: (xc, digest, digest_i)"""
    rmax = max(len(s["records"]) for s in scripts)
    xc, dg, di = np.zeros((len(scripts), rmax, 48)), np.zeros((len(scripts), rmax, 56)), np.zeros((len(scripts), rmax, 16), np.int32)
    for k, s in enumerate(scripts):
        if not s["finite"]:
            continue
        n = 6 * s["W"]
        for r, l in enumerate(run_np(s)):
            xc[k, r, :n], dg[k, r, 8:8 + n] = l["xc"], l["x"]
            dg[k, r, :8] = [l["cost"], l["radius"], l["mu"], 0.0, l["dogleg_norm"], l["model_change"], l["step_norm"], l["x_norm"]]
            di[k, r, :9] = [l["iter"], l["successful"], l["num_invalid"], l["reuse"], l["termination"], l["go"], l["evaluate"], l["decide"],
                            len(l["codes"])]
            di[k, r, 9:9 + min(5, len(l["codes"]))] = l["codes"][:5]
    return xc, dg, di


# Worst ratios of the float64 transcription (replay_np) against tests/golden/tr_kat.npz, by the class of the proposal's branch and
# by quantity (tests/test_tr_kat.py::test_numpy_transcription_within_its_bounds prints them); BOUND is 8 x, the factor of the
# other known-answer suites.  Measured on numpy alone, never on the library or the device.
MEASURED = {
    ('cauchy', 'dogleg_norm'): 7345,  # host 7.34e+03
    ('cauchy', 'model_change'): 4344,  # host 4.34e+03
    ('cauchy', 'xc'): 6846,  # host 6.85e+03
    ('gn', 'dogleg_norm'): 1.069,  # host 1.07
    ('gn', 'model_change'): 0.8952,  # host 1.46
    ('gn', 'xc'): 914.3,  # host 153
    ('interp', 'dogleg_norm'): 1.269e+04,  # host 1.14e+04
    ('interp', 'model_change'): 2386,  # host 2.15e+03
    ('interp', 'xc'): 1.178e+04,  # host 1.11e+04
}
BOUND = {k: 8.0 * v for k, v in MEASURED.items()}
