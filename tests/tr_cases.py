"""Scripts for the trust-region replay hook (M.tr_replay): deterministic, seeded, numpy only.  A script is W, fixed, max_iters, x0
and R rounds of W 28-double records given in advance; the candidate costs and the gradients' lengths are CHOSEN with the float64
transcription of the definition (tr_checks.Machine around tr_checks.propose_np) so that the state machine takes the branch the
family is about -- the records stay data.

Families (per W in 1, 2, 3, 8; H = Q diag(lambda) Q' per frame, condition 1 .. 1e12, scale 1e-4 .. 1e8):
    walk        12 rounds of a random plan of accepted (rel 0.1 / 0.5 / 0.9) and rejected candidates; the gradient of every accepted
                record is scaled so that |gn| / radius is 0.3 .. 300: Gauss-Newton, Cauchy and interpolated steps, rejections in a
                row that take a Gauss-Newton step down to the other two, re-proposals with reuse = 1
    tol         parameter, function and gradient tolerance (at the start and after an accepted step), each also with fixed = 1
    cap         max_iters = 3 with more rounds than that
    radius      fixed = 1 and 125 rejections: the radius falls below 1e-32
    edge        a zero diagonal entry, diagonals under 1e-6 and (after an accepted step) over 1e32 for the clamps, an all-zero frame,
                an all-zero window, a negative-definite and an indefinite H, a candidate cost equal to the cost, a candidate cost 0
    interp_neg  the interpolation's formula for c <= 0 (below)
    recover     invalid steps followed by a valid one, which resets the counter
    nonfinite   NaN / Inf in H, in g and in a candidate cost  (finite = False: no transcription is run on them)

The two beta formulas.  In the coordinates z = D y let B = D^-1 A D^-1, g = grad, a = -alpha g the Cauchy point and
b = -(B + mu I)^-1 g the Gauss-Newton point; c = a.(b - a) = alpha (g'(B + mu I)^-1 g - (g'g)^2 / (g'B g)).  For mu = 0 this is
>= 0 by Cauchy-Schwarz ((g'B g)(g'B^-1 g) >= (g'g)^2), with equality only for an eigenvector, where a = b and the interpolation
is not reached: at the floor mu = 1e-8 the formula for c <= 0 is out of reach of anything but rounding.  It IS reachable by
finite records once mu is large: an indefinite H raises mu (ladder), the step is accepted (mu / 5), and the next record has
B = [[1, 1 - e], [1 - e, 1]] (+) I with e = mu / 200 and a gradient that is the strong eigenvector (eigenvalue 2 - e) plus a share
p of the weak one (eigenvalue e): c < 0 needs p < mu (e + mu) / 4, |b| > |a| needs p > mu (e + mu)^2 / 4; the family interp_neg
takes p = mu (e + mu) / 8 and puts the radius at sqrt(|a| |b|).  Both formulas are therefore in the census.

An invalid step followed by a valid one: a Gauss-Newton step of a system that factors has model_change = y'(A / 2 + mu D^2) y > 0,
a Cauchy step with alpha > 0 is shorter than the minimiser along the gradient, a failed solve leaves mu >= 1 for good and a zero
gradient is invalid at every mu -- it is the interpolation with alpha < 0 that reaches it (family recover, see there).
"""
import numpy as np

import tr_checks as K

WS = (1, 2, 3, 8)
SEED = 20261019


def spd(rng, cond, scale):
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    lam = scale * np.logspace(0, -np.log10(cond), 6)
    H = (Q * lam) @ Q.T
    return 0.5 * (H + H.T)


def records(rng, W, g_len=1.0, cost=1.0, cond=None, scale=None, Hs=None):
    out = np.zeros((W, 28))
    for f in range(W):
        c = cond if cond is not None else 10.0 ** rng.uniform(0, 12)
        s = scale if scale is not None else 10.0 ** rng.uniform(-4, 8)
        H = Hs[f] if Hs is not None else spd(rng, c, s)
        g = rng.standard_normal(6)
        out[f] = K.pack_record(H, g_len * g * np.sqrt(np.abs(np.diag(H)) + 1e-300), cost / W)
    return out


class Builder:
    def __init__(self, W, fixed, max_iters, x0, family, finite=True):
        self.s = dict(W=W, fixed=fixed, max_iters=max_iters, x0=np.asarray(x0, float), family=family, finite=finite, records=[])
        self.m = K.Machine(W, fixed, max_iters, x0, K.propose_np, K.scale_np)
        self.log = None

    def push(self, rec):
        self.s["records"].append(np.array(rec, float))
        self.log = self.m.feed(rec)
        return self.log

    def aim(self, rng, rec, t, mu=None, radius=None):
        """scale the gradients of rec so that the next proposal's |gn| is t x the radius it will meet"""
        m = self.m
        scale = m.scale if m.round >= 0 else K.scale_np(rec)
        p = K.propose_np(rec, scale, 1e-8 if mu is None else mu, 1e300)
        if p["ok"] and p["gn_norm"] > 0:
            rec = rec.copy()
            rec[:, 21:27] *= t * (1e4 if radius is None else radius) / p["gn_norm"]
        return rec

    def set_cost(self, rec, total):
        rec = rec.copy()
        rec[:, 27] = total / len(rec)
        return rec

    def candidate(self, rng, action, t=None):
        """the records of the current candidate for an action: 'grow' / 'keep' / 'shrink' / 'reject'"""
        m = self.m
        rel = {"grow": 0.9, "keep": 0.5, "shrink": 0.1, "reject": -0.5, "reject0": 4e-4}[action]
        cand = float(m.cost) - rel * float(m.model_change)
        rec = records(rng, m.W)
        if rel > 1e-3:
            radius = m.radius * 0.5 if rel < 0.25 else max(m.radius, 3.0 * float(m.dogleg_norm)) if rel > 0.75 else m.radius
            rec = self.aim(rng, rec, t if t is not None else rng.choice([0.3, 0.35, 0.6, 3.0, 30.0, 300.0]), max(1e-8, m.mu / 5.0), radius)
        return self.set_cost(rec, cand)

    def done(self):
        self.s["records"] = np.array(self.s["records"])
        return self.s


def x_start(rng, W):
    return rng.standard_normal(6 * W) * rng.choice([1e-3, 1.0, 50.0])


def walk(rng, W, k):
    b = Builder(W, int(k % 6 == 5), 50, x_start(rng, W), "walk")
    t0 = [0.3, 0.35, 0.6, 3.0, 30.0, 300.0][k % 6]
    rec0 = records(rng, W)
    b.push(b.set_cost(b.aim(rng, rec0, t0), 1.0))
    # cost: a few model changes above zero, as a least-squares cost is
    b.s["records"][0][:, 27] = 20.0 * max(float(b.m.model_change), 1e-300) / W
    b = _rebuild(b)
    plans = (["reject"] * 3 + ["grow", "keep", "reject", "shrink", "reject0", "reject", "grow", "grow"],
             ["grow", "reject", "reject", "reject", "keep", "shrink", "shrink", "reject", "keep", "grow", "reject"],
             ["keep", "shrink", "reject", "grow", "reject", "reject", "reject", "reject", "grow", "keep", "shrink"],
             ["reject"] * 6 + ["keep", "grow", "reject0", "shrink", "keep"])
    for a in plans[(k // 6) % 4]:
        if not b.m.go:
            break
        b.push(b.candidate(rng, a))
    return b.done()


def _rebuild(b):
    n = Builder(b.s["W"], b.s["fixed"], b.s["max_iters"], b.s["x0"], b.s["family"], b.s["finite"])
    for r in b.s["records"]:
        n.push(r)
    return n


def tol(rng, W, k):
    kind, fixed = ("param", "func", "grad0", "grad1")[k % 4], (k // 4) % 2
    b = Builder(W, fixed, 50, rng.standard_normal(6 * W) * (1e6 if kind == "param" else 1.0), "tol_%s_fixed%d" % (kind, fixed))
    rec0 = b.set_cost(records(rng, W, cond=10.0 ** rng.uniform(0, 6)), 1.0)
    if kind == "param":  # a step of 1e-10 |x| (a Gauss-Newton step: its length is linear in g), |x| large so that g stays above 1e-10
        rec0 = b.aim(rng, rec0, 1e-3)
        b.push(rec0)
        rec0[:, 21:27] *= 1e-10 * float(b.m.x_norm) / float(b.m.step_norm)
        b = Builder(W, fixed, 50, b.s["x0"], b.s["family"])
    elif kind == "grad0":
        rec0[:, 21:27] *= 1e-12 / np.max(np.abs(rec0[:, 21:27]))
    else:
        rec0 = b.aim(rng, rec0, 0.3)
    b.push(rec0)
    for r in range(4):
        if not b.m.go:
            # the rounds after a stop change nothing: two more, so that the hook's idle rounds are compared too
            b.s["records"] += [records(rng, W), records(rng, W)]
            break
        rec = b.candidate(rng, "keep", 0.3)
        if kind == "func" and r == 0:
            rec = b.set_cost(rec, float(b.m.cost) * (1.0 - 1e-9))
        if kind == "grad1" and r == 0:
            rec[:, 21:27] *= 1e-13 / np.max(np.abs(rec[:, 21:27]))
        if fixed and (kind in ("grad0", "param") or (kind == "grad1" and r >= 1)):
            # the model change of a gradient this small is far under an ulp of the cost: a candidate rejected beyond doubt
            rec = b.set_cost(rec, 2.0 * float(b.m.cost))
        b.push(rec)
    return b.done()


def cap(rng, W, k):
    b = Builder(W, k % 2, 3, x_start(rng, W), "cap")
    b.push(b.set_cost(b.aim(rng, records(rng, W), [0.3, 3.0, 30.0][k % 3]), 1.0))
    for a in (["grow", "reject", "keep", "keep", "keep"], ["reject", "reject", "reject", "keep", "keep"])[(k // 2) % 2]:
        if not b.m.go:
            b.s["records"].append(records(rng, W))
            continue
        b.push(b.candidate(rng, a))
    return b.done()


def radius(rng, W, k):
    b = Builder(W, 1, 1000, x_start(rng, W), "radius")
    b.push(b.set_cost(b.aim(rng, records(rng, W, cond=10.0 ** (2 * k)), 0.3), 1.0))
    for r in range(127):
        if not b.m.go:
            b.s["records"].append(records(rng, W))
            continue
        b.push(b.candidate(rng, "reject"))
    return b.done()


EDGES = ("diag0", "diag_small", "diag_huge", "zero_frame", "zero_window", "negdef", "indef", "indef_mu", "cost_equal", "cost_zero")


def edge(rng, W, k):
    kind = EDGES[k % len(EDGES)]
    fixed = 1 if kind in ("zero_window",) else (k // len(EDGES)) % 2
    b = Builder(W, fixed, 50, x_start(rng, W), "edge_" + kind)
    c = 10.0 ** rng.uniform(0, 4)
    Hs = [spd(rng, c, 10.0 ** rng.uniform(-2, 4)) for _ in range(W)]
    rec0 = records(rng, W, Hs=Hs)
    f = rng.integers(W)
    if kind == "diag0":  # parameter 2 of one frame is unobserved: row, column and gradient exactly 0
        Hs[f][2, :] = Hs[f][:, 2] = 0.0
        rec0 = records(rng, W, Hs=Hs)
        rec0[f, 21 + 2] = 0.0
    elif kind == "diag_small":
        Hs[f] = spd(rng, 10.0, 1e-9)
        rec0 = records(rng, W, Hs=Hs)
    elif kind == "zero_frame" and W > 1:
        rec0[f] = 0.0
    elif kind == "zero_window":
        rec0[:] = 0.0
    elif kind in ("indef", "indef_mu"):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = np.array([1.0, 0.8, 0.6, 0.5, 0.3, -10.0 ** rng.uniform(-6, -1)])
        Hs[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T) * 10.0 ** rng.uniform(-2, 4)
        rec0 = records(rng, W, Hs=Hs)
    if np.any(K.unpack_H(rec0)[0][:, range(6), range(6)] < 0):
        b.s["finite"] = False  # (a negative diagonal at x0: the scale is NaN)
    rec0 = b.set_cost(b.aim(rng, rec0, [0.3, 3.0][k % 2]) if kind not in ("zero_window",) else rec0, 1.0)
    b.push(rec0)
    for r in range(5):
        if not b.m.go:
            b.s["records"].append(records(rng, W))
            continue
        rec = b.candidate(rng, ("grow", "keep", "reject", "keep", "shrink")[r])
        if kind == "diag_huge" and r == 0:  # accepted, and its diagonal scaled by the x0 scale is over 1e32
            Hh = [spd(rng, 10.0, 1.0) for _ in range(W)]
            Hh[f] = spd(rng, 10.0, 1e40)
            rec = b.set_cost(b.aim(rng, records(rng, W, Hs=Hh), 0.3, max(1e-8, b.m.mu / 5.0), max(b.m.radius, 3.0 * float(b.m.dogleg_norm))), rec[:, 27].sum())
        if kind == "indef_mu" and r == 0:  # mu is high now: a nearly isotropic model, grad nearly an eigenvector
            Hi = [h * (np.eye(6) + 1e-6 * spd(rng, 10.0, 1.0)) for h in 10.0 ** rng.uniform(-2, 2, W)]
            rec = b.set_cost(b.aim(rng, records(rng, W, Hs=Hi), 3.0, max(1e-8, b.m.mu / 5.0), max(b.m.radius, 3.0 * float(b.m.dogleg_norm))), rec[:, 27].sum())
        if kind == "negdef" and r == 0:  # accepted, and one frame's H is negative definite (at x0 its square roots would be NaN)
            rec[:, :27] = records(rng, W, Hs=[(-h if i == f else h) for i, h in enumerate(Hs)])[:, :27]
        if kind == "cost_equal" and r == 1:
            rec = b.set_cost(rec, 1.0)
            rec[:, 27] = b.m.rec[:, 27]
        if kind == "cost_zero" and r == 1:
            rec[:, 27] = 0.0
        b.push(rec)
    return b.done()


def interp_neg(rng, W, k):
    """c <= 0 in the interpolation (see the module's text): an indefinite record raises mu, the step is accepted, and the next
    record has one frame with B = [[1, 1 - e], [1 - e, 1]] (+) I, e = mu / 200, and a gradient that is the strong eigenvector plus
    a share p = mu (e + mu) / 8 of the weak one; the other frames have no gradient."""
    b = Builder(W, k % 2, 50, x_start(rng, W), "interp_neg")
    f = rng.integers(W)
    Hs = [spd(rng, 10.0, 10.0 ** rng.uniform(-2, 4)) for _ in range(W)]
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    lam = np.array([1.0, 0.8, 0.6, 0.5, 0.3, -[0.3, 0.03, 0.003, 0.0003][k % 4]])
    Hs[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T) * 10.0 ** rng.uniform(-2, 4)
    rec0 = records(rng, W, Hs=Hs)
    if np.any(K.unpack_H(rec0)[0][:, range(6), range(6)] < 0):
        b.s["finite"] = False
    b.push(b.set_cost(b.aim(rng, rec0, 0.3, 1.0 - 1e-9), 1.0))
    if not (b.m.go and b.m.evaluate):
        return b.done()
    mu = max(1e-8, b.m.mu / 5.0)
    radius = max(b.m.radius, 3.0 * float(b.m.dogleg_norm))
    e = mu / 200.0
    pw = mu * (e + mu) / 8.0
    h = 10.0 ** rng.uniform(-2, 2, W)
    Hc = [hh * np.eye(6) for hh in h]
    Hc[f][0, 1] = Hc[f][1, 0] = h[f] * (1.0 - e)
    rec = np.array([K.pack_record(Hc[i], np.zeros(6), 0.0) for i in range(W)])
    rec[f, 21:23] = np.sqrt(1.0 - pw) * np.array([1.0, 1.0]) + np.sqrt(pw) * np.array([1.0, -1.0])
    p = K.propose_np(rec, b.m.scale, mu, 1e300)
    rec[:, 21:27] *= radius / np.sqrt(p["gn_norm"] * p["cauchy_norm"])
    b.push(b.set_cost(rec, float(b.m.cost) - 0.9 * float(b.m.model_change)))
    for a in ("reject", "keep", "grow"):
        if b.m.go:
            b.push(b.candidate(rng, a))
    return b.done()


def recover(rng, W, k):
    """invalid steps followed by a valid one: one frame's H has a small negative eigenvalue l and, in the scaled coordinates, the
    gradient is its eigenvector v plus a share e < sqrt(|l|) of another one, so g'B g < 0 and alpha < 0: the 'Cauchy point' a lies far
    uphill, and the segment from a to the Gauss-Newton point b passes the sphere by when the radius is under |b| sin(a, b): the
    discriminant is negative, the step NaN, model_change NaN -- invalid.  Every invalid step raises mu by 10, which shortens b,
    until the segment crosses the sphere or b is inside.  The share and the radius are searched on a small fixed grid with the
    float64 transcription; the first pair that gives an invalid step followed by a valid one is kept."""
    f = rng.integers(W)
    Hs = [spd(rng, 10.0, 1.0) for _ in range(W)]
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    neg = [1e-4, 1e-5, 1e-6][k % 3]
    lam = np.array([1.0, 0.8, 0.6, 0.5, 0.3, -neg])
    Hs[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T)
    x0 = x_start(rng, W)
    base = np.array([K.pack_record(Hs[i], np.zeros(6), 0.0) for i in range(W)])
    sc = K.scale_np(base)[f]
    A = Hs[f] * sc[:, None] * sc[None, :]
    d2 = np.maximum(np.diag(A), 1e-6)
    Bm = A / np.sqrt(d2[:, None] * d2[None, :])
    ev, V = np.linalg.eigh(Bm)
    for share in (0.2, 0.5, 0.8):
        for t in (1.5, 3.0, 10.0, 30.0, 100.0, 300.0):
            b = Builder(W, k % 2, 50, x0, "recover", finite=bool(np.all(np.diag(Hs[f]) > 0)))
            rec0 = base.copy()
            grad = V[:, 0] + share * np.sqrt(-ev[0]) * V[:, 5]
            rec0[f, 21:27] = np.sqrt(d2) * grad / sc
            p = K.propose_np(rec0, K.scale_np(rec0), 1e-8, 1e300)
            rec0[:, 21:27] *= t * 1e4 / p["gn_norm"]
            log = b.push(b.set_cost(rec0, 1.0))
            if len(log["codes"]) >= 2 and (log["codes"][-1] & 15) <= 4:
                for a in ("grow", "reject", "keep"):
                    if b.m.go and b.m.evaluate:
                        b.push(b.candidate(rng, a))
                return b.done()
    return b.done()


NONFINITE = ("nan_H", "inf_H", "nan_g", "inf_g", "nan_cost", "inf_cost", "nan_H_later", "nan_g_later")


def nonfinite(rng, W, k):
    kind = NONFINITE[k % len(NONFINITE)]
    b = Builder(W, (k // len(NONFINITE)) % 2, 8, x_start(rng, W), "nonfinite_" + kind, finite=False)
    rec0 = b.set_cost(b.aim(rng, records(rng, W, cond=100.0), 0.3), 1.0)
    f, bad = rng.integers(W), (np.nan if kind.startswith("nan") else np.inf)
    if kind in ("nan_H", "inf_H"):
        rec0[f, rng.integers(21)] = bad
    if kind in ("nan_g", "inf_g"):
        rec0[f, 21 + rng.integers(6)] = bad
    b.push(rec0)
    for r in range(5):
        rec = b.candidate(rng, ("grow", "keep", "reject", "keep", "shrink")[r]) if b.m.go and np.isfinite(float(b.m.model_change)) else records(rng, W)
        rec = np.where(np.isfinite(rec), rec, 1.0)
        if r == 0 and kind in ("nan_cost", "inf_cost"):
            rec[f, 27] = bad
        if r == 0 and kind == "nan_H_later":
            rec[f, 3] = bad
        if r == 0 and kind == "nan_g_later":
            rec[f, 22] = bad
        if b.m.go:
            b.push(rec)
        else:
            b.s["records"].append(rec)
    return b.done()


FAMILIES = ((walk, 24), (tol, 48), (cap, 8), (radius, 5), (edge, 40), (interp_neg, 12), (recover, 12), (nonfinite, 16))


def make_scripts(seed=SEED, families=FAMILIES, ws=WS):
    scripts = []
    for W in ws:
        for fi, (fn, n) in enumerate(families):
            for k in range(n):
                rng = np.random.default_rng([seed, W, fi, k])
                s = fn(rng, W, k)
                s["name"] = "%s/W%d/%d" % (s["family"], W, k)
                scripts.append(s)
    return scripts


def many_scripts(n=300, seed=SEED + 1):
    """more scripts than the device has compute units: n one-frame-to-eight-frame scripts of 3 rounds"""
    out = []
    for k in range(n):
        rng = np.random.default_rng([seed, k])
        W = WS[k % 4]
        b = Builder(W, 0, 50, x_start(rng, W), "many")
        b.push(b.set_cost(b.aim(rng, records(rng, W), [0.3, 3.0, 30.0][k % 3]), 1.0))
        for a in (("grow", "reject"), ("reject", "keep"), ("shrink", "grow"))[(k // 3) % 3]:
            b.push(b.candidate(rng, a)) if b.m.go else b.s["records"].append(records(rng, W))
        s = b.done()
        s["name"] = "many/%d" % k
        out.append(s)
    return out
