"""Scripts for the full-window replay hook (M.fw_replay): deterministic, seeded, numpy only.  A script is W, fixed, max_iters, x0
and R rounds (band of H, g, cost) given in advance; candidate costs and gradient lengths are CHOSEN with the float64
transcription of the definition (tr_checks.Machine around fw_tr_checks.propose_np), as tr_cases.Builder does -- the rounds stay
data.

Sizes: W in 1, 2, 3, 5, 8 -- n = 15 has no off-diagonal block, n = 30 a band that is the whole matrix, n = 45 the first true
out-of-band zeros, n = 75 the first rows >= 64 (the second register of the substitutions), n = 120 the maximum.

H is block tridiagonal and symmetric bit for bit, built as the assembly builds it: a 15 x 15 block Q diag(lambda) Q' per frame
(condition 1 .. 1e12, scale 1e-4 .. 1e8; see make_H) plus J'J of a 15 x 30 factor block for every pair of consecutive frames.

Families: those of tr_cases.py (walk, tol, cap, radius -- W 1 and 2 only --, edge, interp_neg, recover, nonfinite; see there
for the reasoning behind interp_neg and recover, which is used unchanged on one frame's block) and the band's own:
    decoupled   an exactly zero off-diagonal block at one frame boundary (an IMU gap), and at all of them
    pivot       round 1 (after an accepted step, the scale being fixed by round 0) has its first non-positive pivot at column j, for
                j in 0, 14, 15, 29, 30, 44, 63, 64, 65, n - 1 as far as n has them, and becomes definite after exactly k in 1, 3 raises
                of mu: the columns 0 .. j are decoupled from the rest (exact zeros), their leading j x j block is definite, and
                H_jj is lowered by bisection until the pivot of column j of S H S + mu* D^2 is zero at mu* = 1e-8 10^(k - 1/2).
                A pivot grows with mu, so the ladder fails k times at column j and then passes.
    overflow    a system that factors but whose solution overflows: g near the largest double against a small H
                (finite = False: the transcription is not run on it; host and device must agree and end defined)
    nonfinite   a NaN and an Inf in H at an in-band position of the first, a middle and the last block row, in g, and in a
                candidate cost  (finite = False)
"""
import numpy as np

import fw_tr_checks as K

WS = (1, 2, 3, 5, 8)
SEED = 20261020
PIVOT_COLUMNS = (0, 14, 15, 29, 30, 44, 63, 64, 65)


def spd(rng, cond, scale, m=15):
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = scale * np.logspace(0, -np.log10(cond), m)
    H = (Q * lam) @ Q.T
    return 0.5 * (H + H.T)


def make_H(rng, W, cond=None, scale=None, gaps=(), blocks=None):
    """frame blocks + J'J of a factor between frames f - 1 and f for every f not in gaps"""
    n = 15 * W
    H = np.zeros((n, n))
    sc = []
    # one H in twelve spans the whole range (condition to 1e12, scale 1e-4 .. 1e8); the others stay where cond_2 of the WHOLE damped
    # window -- which also sees the frames' scales against each other -- leaves the exact fixture's margin rule room to decide
    wide = rng.random() < 0.08
    for f in range(W):
        c = cond if cond is not None else 10.0 ** rng.uniform(0, 12 if wide else 5)
        s = (scale[f] if np.ndim(scale) else scale) if scale is not None else 10.0 ** (rng.uniform(-4, 8) if wide else rng.uniform(0, 8))
        sc.append(s)
        H[15 * f:15 * f + 15, 15 * f:15 * f + 15] = blocks[f] if blocks is not None else spd(rng, c, s)
    for f in range(1, W):
        J = rng.standard_normal((15, 30)) * np.sqrt(min(sc[f - 1], sc[f]) * 10.0 ** rng.uniform(-3, 0))
        if f not in gaps:
            H[15 * f - 15:15 * f + 15, 15 * f - 15:15 * f + 15] += J.T @ J
    return 0.5 * (H + H.T)


def records(rng, W, g_len=1.0, cost=1.0, cond=None, scale=None, H=None, gaps=()):
    H = make_H(rng, W, cond, scale, gaps) if H is None else H
    g = rng.standard_normal(15 * W)
    return (K.band(H), g_len * g * np.sqrt(np.abs(np.diag(H)) + 1e-300), float(cost))


def with_g(rec, g):
    return (rec[0], np.asarray(g, float), rec[2])


class Builder:
    def __init__(self, W, fixed, max_iters, x0, family, finite=True):
        self.s = dict(W=W, fixed=fixed, max_iters=max_iters, x0=np.asarray(x0, float), family=family, finite=finite, records=[])
        self.m = K.machine(W, fixed, max_iters, x0)
        self.log = None
        self.scales = None

    def fresh(self, rng, gaps=(), cond=None):
        """a random round whose frames keep the scales this script drew first: the Jacobi scaling is fixed by round 0, so frames
        that changed scale from round to round would leave S H S, and with it cond_2 of the window, anywhere (edge_diag_huge does that
        on purpose)"""
        if self.scales is None:
            self.scales = 10.0 ** (rng.uniform(-4, 8, self.s["W"]) if rng.random() < 0.08 else rng.uniform(0, 8, self.s["W"]))
        return records(rng, self.s["W"], cond=cond, scale=self.scales, gaps=gaps)

    def push(self, rec):
        self.s["records"].append(rec)
        self.log = self.m.feed(rec)
        return self.log

    def aim(self, rec, t, mu=None, radius=None):
        """scale the gradient of rec so that the next proposal's |gn| is t x the radius it will meet"""
        m = self.m
        scale = m.scale if m.round >= 0 else K.scale_np(rec)
        p = K.propose_np(rec, scale, 1e-8 if mu is None else mu, 1e300)
        if p["ok"] and p["gn_norm"] > 0:
            rec = with_g(rec, rec[1] * (t * (1e4 if radius is None else radius) / p["gn_norm"]))
        return rec

    @staticmethod
    def set_cost(rec, total):
        return (rec[0], rec[1], float(total))

    def next_radius(self, rel):
        m = self.m
        return m.radius * 0.5 if rel < 0.25 else max(m.radius, 3.0 * float(m.dogleg_norm)) if rel > 0.75 else m.radius

    def candidate(self, rng, action, t=None, rec=None, gaps=()):
        """the round of the current candidate for an action: 'grow' / 'keep' / 'shrink' / 'reject' / 'reject0'"""
        m = self.m
        rel = {"grow": 0.9, "keep": 0.5, "shrink": 0.1, "reject": -0.5, "reject0": 4e-4}[action]
        cand = float(m.cost) - rel * float(m.model_change)
        rec = self.fresh(rng, gaps=gaps) if rec is None else rec
        if rel > 1e-3:
            rec = self.aim(rec, t if t is not None else rng.choice([0.3, 0.35, 0.6, 3.0, 30.0, 300.0]), max(1e-8, m.mu / 5.0), self.next_radius(rel))
        return self.set_cost(rec, cand)

    def done(self):
        return self.s


def x_start(rng, W):
    return rng.standard_normal(15 * W) * rng.choice([1e-3, 1.0, 50.0])


PLANS = (["reject"] * 3 + ["grow", "keep", "reject", "shrink", "reject0", "reject", "grow", "grow"],
         ["grow", "shrink", "reject", "reject", "reject", "keep", "shrink", "reject", "keep", "grow", "reject"],
         # reject -> reject -> accept -> reject: both slots of the device's band copy are restored from
         ["keep", "shrink", "reject", "reject", "grow", "reject", "reject", "reject", "grow", "keep", "shrink"],
         ["reject"] * 6 + ["keep", "grow", "reject0", "shrink", "keep"])


def walk(rng, W, k, gaps=(), family="walk", rounds=11):
    x0 = x_start(rng, W)
    t0 = [0.3, 0.35, 0.6, 3.0, 30.0, 300.0][k % 6]
    b = Builder(W, int(k % 6 == 5), 50, x0, family)
    rec0 = b.aim(b.fresh(rng, gaps=gaps), t0)
    b.push(b.set_cost(rec0, 1.0))
    # cost: a few model changes above zero, as a least-squares cost is
    rec0 = b.set_cost(rec0, 20.0 * max(float(b.m.model_change), 1e-300))
    b, old = Builder(W, int(k % 6 == 5), 50, x0, family), b
    b.scales = old.scales
    b.push(rec0)
    for a in PLANS[(k // 6) % 4][:rounds]:
        if not b.m.go:
            break
        b.push(b.candidate(rng, a, gaps=gaps))
    return b.done()


def tol(rng, W, k):
    kind, fixed = ("param", "func", "grad0", "grad1")[k % 4], (k // 4) % 2
    x0 = rng.standard_normal(15 * W) * (1e6 if kind == "param" else 1.0)
    b = Builder(W, fixed, 50, x0, "tol_%s_fixed%d" % (kind, fixed))
    rec0 = b.set_cost(b.fresh(rng, cond=10.0 ** rng.uniform(0, 6)), 1.0)
    if kind == "param":  # a step of 1e-10 |x| (a Gauss-Newton step: its length is linear in g), |x| large so that g stays above 1e-10
        rec0 = b.aim(rec0, 1e-3)
        b.push(rec0)
        rec0 = with_g(rec0, rec0[1] * (1e-10 * float(b.m.x_norm) / float(b.m.step_norm)))
        b, old = Builder(W, fixed, 50, x0, b.s["family"]), b
        b.scales = old.scales
    elif kind == "grad0":
        rec0 = with_g(rec0, rec0[1] * (1e-12 / np.max(np.abs(rec0[1]))))
    else:
        rec0 = b.aim(rec0, 0.3)
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
            rec = with_g(rec, rec[1] * (1e-13 / np.max(np.abs(rec[1]))))
        if fixed and (kind in ("grad0", "param") or (kind == "grad1" and r >= 1)):
            # the model change of a gradient this small is far under an ulp of the cost: a candidate rejected beyond doubt
            rec = b.set_cost(rec, 2.0 * float(b.m.cost))
        b.push(rec)
    return b.done()


def cap(rng, W, k):
    b = Builder(W, k % 2, 3, x_start(rng, W), "cap")
    b.push(b.set_cost(b.aim(b.fresh(rng), [0.3, 3.0, 30.0][k % 3]), 1.0))
    for a in (["grow", "reject", "keep", "keep", "keep"], ["reject", "reject", "reject", "keep", "keep"])[(k // 2) % 2]:
        if not b.m.go:
            b.s["records"].append(records(rng, W))
            continue
        b.push(b.candidate(rng, a))
    return b.done()


def radius(rng, W, k):
    b = Builder(W, 1, 1000, x_start(rng, W), "radius")
    b.push(b.set_cost(b.aim(records(rng, W, cond=10.0 ** (2 * k)), 0.3), 1.0))
    H = make_H(rng, W)
    for r in range(125):  # (the same H in every rejected round: only its cost is read)
        if not b.m.go:
            b.s["records"].append(records(rng, W, H=H))
            continue
        b.push(b.candidate(rng, "reject", rec=records(rng, W, H=H)))
    return b.done()


EDGES = ("diag0", "diag_small", "diag_huge", "zero_frame", "zero_window", "negdef", "indef", "indef_mu", "cost_equal", "cost_zero")


def edge(rng, W, k):
    kind = EDGES[k % len(EDGES)]
    fixed = 1 if kind in ("zero_window",) else (k // len(EDGES)) % 2
    b = Builder(W, fixed, 50, x_start(rng, W), "edge_" + kind)
    c = 10.0 ** rng.uniform(0, 4)
    blocks = [spd(rng, c, 10.0 ** rng.uniform(-2, 4)) for _ in range(W)]
    f = int(rng.integers(W))
    gaps = ()
    g_zero = None
    if kind == "diag0":  # one parameter of one frame is unobserved: row, column and gradient exactly 0
        H = make_H(rng, W, scale=1.0, blocks=blocks)
        a = 15 * f + 2
        H[a, :] = H[:, a] = 0.0
        g_zero = a
    elif kind == "diag_small":
        blocks[f] = spd(rng, 10.0, 1e-9)
        H = make_H(rng, W, scale=1e-9, blocks=blocks, gaps=range(W))
        gaps = range(W)
    elif kind == "zero_frame" and W > 1:
        H = make_H(rng, W, scale=1.0, blocks=blocks, gaps=(f, f + 1))
        H[15 * f:15 * f + 15, :] = H[:, 15 * f:15 * f + 15] = 0.0
    elif kind == "zero_window":
        H = np.zeros((15 * W, 15 * W))
    elif kind in ("indef", "indef_mu"):
        Q, _ = np.linalg.qr(rng.standard_normal((15, 15)))
        lam = np.concatenate([np.linspace(1.0, 0.3, 14), [-10.0 ** rng.uniform(-6, -1)]])
        blocks[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T) * 10.0 ** rng.uniform(-2, 4)
        H = make_H(rng, W, scale=1.0, blocks=blocks, gaps=range(W))
    else:
        H = make_H(rng, W, scale=1.0, blocks=blocks)
    rec0 = records(rng, W, H=H)
    if g_zero is not None:
        rec0[1][g_zero] = 0.0
    if kind == "zero_frame" and W > 1:
        rec0[1][15 * f:15 * f + 15] = 0.0
    if kind == "zero_window":
        rec0 = with_g(rec0, np.zeros(15 * W))
    if np.any(np.diag(H) < 0):
        b.s["finite"] = False  # (a negative diagonal at x0: the scale is NaN)
    rec0 = b.set_cost(b.aim(rec0, [0.3, 3.0][k % 2]) if kind != "zero_window" else rec0, 1.0)
    b.push(rec0)
    for r in range(5):
        if not b.m.go:
            b.s["records"].append(records(rng, W))
            continue
        action = ("grow", "keep", "reject", "keep", "shrink")[r]
        rec = b.candidate(rng, action)
        if kind == "diag_huge" and r == 0:  # accepted, and its diagonal scaled by the x0 scale is over 1e32
            bl = [spd(rng, 10.0, 1.0) for _ in range(W)]
            bl[f] = spd(rng, 10.0, 1e40)
            rec = b.set_cost(b.aim(records(rng, W, H=make_H(rng, W, scale=1.0, blocks=bl)), 0.3, max(1e-8, b.m.mu / 5.0), b.next_radius(0.9)), rec[2])
        if kind == "indef_mu" and r == 0:  # mu is high now: a nearly isotropic model, grad nearly an eigenvector
            bl = [h * (np.eye(15) + 1e-6 * spd(rng, 10.0, 1.0)) for h in 10.0 ** rng.uniform(-2, 2, W)]
            rec = b.set_cost(b.aim(records(rng, W, H=make_H(rng, W, blocks=bl, gaps=range(W))), 3.0, max(1e-8, b.m.mu / 5.0), b.next_radius(0.9)), rec[2])
        if kind == "negdef" and r == 0:  # accepted, and one frame's H is negative definite (at x0 its square roots would be NaN)
            bl = [(-h if i == f else h) for i, h in enumerate(blocks)]
            rec = (K.band(make_H(rng, W, blocks=bl, gaps=range(W))), rec[1], rec[2])
        if kind == "cost_equal" and r == 1:
            rec = b.set_cost(rec, float(b.m.cost))
        if kind == "cost_zero" and r == 1:
            rec = b.set_cost(rec, 0.0)
        b.push(rec)
    return b.done()


def interp_neg(rng, W, k):
    """c <= 0 in the interpolation (tr_cases' text): an indefinite round raises mu, the step is accepted, and the next round has
    B = [[1, 1 - e], [1 - e, 1]] (+) I in one frame, e = mu / 200, and a gradient that is the strong eigenvector plus a share
    p = mu (e + mu) / 8 of the weak one; the other entries of the gradient are zero."""
    b = Builder(W, k % 2, 50, x_start(rng, W), "interp_neg")
    f = int(rng.integers(W))
    blocks = [spd(rng, 10.0, 10.0 ** rng.uniform(-2, 4)) for _ in range(W)]
    Q, _ = np.linalg.qr(rng.standard_normal((15, 15)))
    lam = np.concatenate([np.linspace(1.0, 0.3, 14), [-[0.3, 0.03, 0.003, 0.0003][k % 4]]])
    blocks[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T) * 10.0 ** rng.uniform(-2, 4)
    H = make_H(rng, W, blocks=blocks, gaps=range(W))
    if np.any(np.diag(H) < 0):
        b.s["finite"] = False
    b.push(b.set_cost(b.aim(records(rng, W, H=H), 0.3, 1.0 - 1e-9), 1.0))
    if not (b.m.go and b.m.evaluate):
        return b.done()
    mu = max(1e-8, b.m.mu / 5.0)
    rad = b.next_radius(0.9)
    e = mu / 200.0
    pw = mu * (e + mu) / 8.0
    h = np.repeat(10.0 ** rng.uniform(-2, 2, W), 15)
    Hc = np.diag(h)
    Hc[15 * f, 15 * f + 1] = Hc[15 * f + 1, 15 * f] = h[15 * f] * (1.0 - e)
    g = np.zeros(15 * W)
    g[15 * f:15 * f + 2] = np.sqrt(1.0 - pw) * np.array([1.0, 1.0]) + np.sqrt(pw) * np.array([1.0, -1.0])
    rec = (K.band(Hc), g, 0.0)
    p = K.propose_np(rec, b.m.scale, mu, 1e300)
    rec = with_g(rec, g * (rad / np.sqrt(p["gn_norm"] * p["cauchy_norm"])))
    b.push(b.set_cost(rec, float(b.m.cost) - 0.9 * float(b.m.model_change)))
    for a in ("reject", "keep", "grow"):
        if b.m.go:
            b.push(b.candidate(rng, a))
    return b.done()


def recover(rng, W, k):
    """invalid steps followed by a valid one (tr_cases.recover on one frame's 15 x 15 block): the block has a small negative eigenvalue
    and the gradient is its eigenvector plus a share of another one, so alpha < 0 and the segment from the Cauchy point to the
    Gauss-Newton point passes the sphere by (a NaN step, invalid) until mu, raised by every invalid step, has shortened it."""
    f = int(rng.integers(W))
    blocks = [spd(rng, 10.0, 1.0) for _ in range(W)]
    Q, _ = np.linalg.qr(rng.standard_normal((15, 15)))
    neg = [1e-4, 1e-5, 1e-6][k % 3]
    lam = np.concatenate([np.linspace(1.0, 0.3, 14), [-neg]])
    blocks[f] = 0.5 * ((Q * lam) @ Q.T + ((Q * lam) @ Q.T).T)
    H = make_H(rng, W, scale=1.0, blocks=blocks, gaps=range(W))
    x0 = x_start(rng, W)
    base = (K.band(H), np.zeros(15 * W), 0.0)
    sc = K.scale_np(base)[15 * f:15 * f + 15]
    A = blocks[f] * sc[:, None] * sc[None, :]
    d2 = np.maximum(np.diag(A), 1e-6)
    ev, V = np.linalg.eigh(A / np.sqrt(d2[:, None] * d2[None, :]))
    b = None
    for share in (0.2, 0.5, 0.8):
        for t in (1.5, 3.0, 10.0, 30.0, 100.0, 300.0):
            b = Builder(W, k % 2, 50, x0, "recover", finite=bool(np.all(np.diag(H) > 0)))
            g = np.zeros(15 * W)
            g[15 * f:15 * f + 15] = np.sqrt(d2) * (V[:, 0] + share * np.sqrt(-ev[0]) * V[:, 14]) / sc
            rec0 = with_g(base, g)
            p = K.propose_np(rec0, K.scale_np(rec0), 1e-8, 1e300)
            rec0 = with_g(rec0, g * (t * 1e4 / p["gn_norm"]))
            log = b.push(b.set_cost(rec0, 1.0))
            if len(log["codes"]) >= 2 and (log["codes"][-1] & 15) <= 4:
                for a in ("grow", "reject", "keep"):
                    if b.m.go and b.m.evaluate:
                        b.push(b.candidate(rng, a))
                return b.done()
    return b.done()


def block_rows(W):
    """the first, a middle and the last block row"""
    return sorted({0, W // 2, W - 1})


# (kind, which of block_rows): H at every block row, g and the cost once
NONFINITE = tuple((kind, i) for kind in ("nan_H", "inf_H", "nan_H_later", "inf_H_later") for i in range(3)) + \
    (("nan_g", 0), ("inf_g", 2), ("nan_g_later", 1), ("nan_cost", 0), ("inf_cost", 1))


def nonfinite(rng, W, k):
    kind, i = NONFINITE[k % len(NONFINITE)]
    rows = block_rows(W)
    F = rows[i % len(rows)]
    b = Builder(W, k % 2, 8, x_start(rng, W), "nonfinite_%s_row%d" % (kind, F), finite=False)
    rec0 = b.set_cost(b.aim(records(rng, W, cond=100.0), 0.3), 1.0)
    bad = np.nan if kind.startswith("nan") else np.inf
    a = 15 * F + int(rng.integers(15))
    cols = [c for c in range(max(0, 15 * F - 15), min(15 * W, 15 * F + 30)) if c != a or k % 2]  # in-band, on or off the diagonal
    c = int(rng.choice(cols))

    def poison_H(rec):
        H = K.dense(rec[0])
        H[a, c] = H[c, a] = bad
        return (K.band(H), rec[1], rec[2])

    def poison_g(rec):
        g = rec[1].copy()
        g[a] = bad
        return with_g(rec, g)

    if kind in ("nan_H", "inf_H"):
        rec0 = poison_H(rec0)
    if kind in ("nan_g", "inf_g"):
        rec0 = poison_g(rec0)
    b.push(rec0)
    for r in range(3):
        ok = b.m.go and np.isfinite(float(b.m.model_change)) and np.isfinite(float(b.m.cost))
        rec = b.candidate(rng, ("grow", "reject", "keep")[r]) if ok else records(rng, W)
        rec = (rec[0], np.where(np.isfinite(rec[1]), rec[1], 1.0), rec[2] if np.isfinite(rec[2]) else 1.0)
        if r == 0 and kind in ("nan_cost", "inf_cost"):
            rec = b.set_cost(rec, bad)
        if r == 0 and kind in ("nan_H_later", "inf_H_later"):
            rec = poison_H(rec)
        if r == 0 and kind == "nan_g_later":
            rec = poison_g(rec)
        if b.m.go:
            b.push(rec)
        else:
            b.s["records"].append(rec)
    return b.done()


def decoupled(rng, W, k):
    """an IMU gap: the off-diagonal block at one boundary (k even) or at every boundary (k odd) is exactly zero"""
    gaps = tuple(range(1, W)) if k % 2 else ((1 + (k // 2) % max(W - 1, 1)),)
    return walk(rng, W, k // 2, gaps=gaps, family="decoupled_" + ("all" if k % 2 else "one"), rounds=6)


def first_bad_pivot(M):
    """column of the first non-positive (or non-finite) pivot of a plain Cholesky of M, or -1"""
    L = np.array(M, float)
    n = len(L)
    for j in range(n):
        d = L[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0.0) or not np.isfinite(d):
            return j
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return -1


def damped(H, scale, mu):
    A = H * scale[:, None] * scale[None, :]
    return A + mu * np.diag(np.minimum(np.maximum(np.diag(A), 1e-6), 1e32))


def pivot(rng, W, k):
    n = 15 * W
    cols = [j for j in PIVOT_COLUMNS if j < n - 1] + [n - 1]
    j, raises = cols[(k // 2) % len(cols)], (1, 3)[k % 2]
    b = Builder(W, k % 2, 50, x_start(rng, W), "pivot_col%d_k%d" % (j, raises))
    b.s["aim"] = (j, raises)
    b.push(b.set_cost(b.aim(records(rng, W, cond=100.0, scale=1.0), 0.3), 1.0))
    assert b.m.go and b.m.evaluate and b.m.mu == 1e-8
    # round 1: accepted (mu stays at its floor), H definite but for column j, columns 0 .. j cut off from the rest
    H = make_H(rng, W, cond=100.0, scale=1.0)
    H[:j + 1, j + 1:] = 0.0
    H[j + 1:, :j + 1] = 0.0
    mu_star = 1e-8 * 10.0 ** (raises - 0.5)
    scale = b.m.scale

    def piv(t):
        Ht = H.copy()
        Ht[j, j] -= t
        M = damped(Ht, scale, mu_star)[:j + 1, :j + 1]
        return M[j, j] - (M[j, :j] @ np.linalg.solve(M[:j, :j], M[j, :j]) if j else 0.0)

    lo, hi = 0.0, 2.0 * H[j, j] + 1.0
    assert piv(lo) > 0 > piv(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if piv(mid) > 0 else (lo, mid)
    H[j, j] -= 0.5 * (lo + hi)
    rec = b.candidate(rng, "keep", 3.0, rec=records(rng, W, H=H))
    b.push(rec)
    for a in ("reject", "keep"):
        if b.m.go and b.m.evaluate:
            b.push(b.candidate(rng, a))
    return b.done()


def overflow(rng, W, k):
    """the solve factors, the solution is not finite: |g| near the largest double over an H of scale 1e-3, at x0 (k even) or in
    the round of an accepted candidate (k odd)"""
    b = Builder(W, k % 2, 8, x_start(rng, W), "overflow", finite=False)
    big = records(rng, W, cond=10.0, scale=1e-3)
    big = with_g(big, big[1] * (1e306 / np.max(np.abs(big[1]))))
    if k % 2 == 0:
        b.push(b.set_cost(big, 1.0))
    else:
        b.push(b.set_cost(b.aim(records(rng, W, cond=100.0), 0.3), 1.0))
        b.push(b.set_cost(big, float(b.m.cost) - 0.5 * float(b.m.model_change)))
    for r in range(3):
        rec = b.set_cost(records(rng, W), 0.5)
        if b.m.go:
            b.push(rec)
        else:
            b.s["records"].append(rec)
    return b.done()


FAMILIES = ((walk, 12), (tol, 8), (cap, 4), (radius, 2), (edge, 20), (interp_neg, 6), (recover, 6), (nonfinite, len(NONFINITE)), (decoupled, 6),
            (pivot, 20), (overflow, 4))


def make_scripts(seed=SEED, families=FAMILIES, ws=WS):
    scripts = []
    for W in ws:
        for fi, (fn, cnt) in enumerate(families):
            if fn is radius and W > 2:
                continue
            if fn is decoupled and W == 1:
                continue
            if fn is pivot:
                cnt = 2 * (len([j for j in PIVOT_COLUMNS if j < 15 * W - 1]) + 1)
            for k in range(cnt):
                rng = np.random.default_rng([seed, W, fi, k])
                s = fn(rng, W, k)
                s["name"] = "%s/W%d/%d" % (s["family"], W, k)
                scripts.append(s)
    return scripts


def many_scripts(n=300, seed=SEED + 1):
    """more scripts than the device has compute units: n scripts of 3 rounds over all five sizes"""
    out = []
    for k in range(n):
        rng = np.random.default_rng([seed, k])
        W = WS[k % 5]
        b = Builder(W, 0, 50, x_start(rng, W), "many")
        b.push(b.set_cost(b.aim(b.fresh(rng), [0.3, 3.0, 30.0][k % 3]), 1.0))
        for a in (("grow", "reject"), ("reject", "keep"), ("shrink", "grow"))[(k // 3) % 3]:
            b.push(b.candidate(rng, a)) if b.m.go else b.s["records"].append(records(rng, W))
        s = b.done()
        s["name"] = "many/%d" % k
        out.append(s)
    return out
