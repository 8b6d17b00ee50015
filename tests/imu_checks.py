"""Shared by tests/test_imu_kat.py (the numpy oracle and the library on the host) and tests/test_gpu_imu_kat.py (the device):
worst ratios of an implementation's IMU factor (raw and whitened), pre-integration and prior residual against the exact references
of tests/golden/imu_kat.npz (tests/golden/make_imu_kat.py), family by family.

A ratio is an error divided by a first-order rounding unit: eps = 2^-52 times exact operand magnitudes (factor_units,
preint_units, prior_units below, every term commented).  Nothing in a unit is measured on an implementation, and no unit holds a
negative power of an angle: |Jr| enters as 1 + theta / 2 + theta^2 / 6, |Jr^-1| as 1 + theta / 2 + theta^2 / 10 (theta <= 3; the
families nearer to pi carry no Jacobian rows: Jr^-1 is ill-conditioned there, its pole is at 2 pi).  A unit of zero says that the
value is an exact copy, an exact constant or a structural zero: any error there is a ratio of infinity.

The samples of the pre-integrated intervals are a formula (interval_samples: integer residues, one division, IEEE operations
only), not data, so the fixture stores the results alone."""
import os

import numpy as np

EPS = 2.0 ** -52
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_kat.npz")
GRAV = np.array([0.0, 0.0, -9.805])
GNORM = 9.805
ACC_N, GYR_N, ACC_W, GYR_W = 0.08, 0.004, 2.0e-4, 2.0e-5
DTS = (0.005, 0.1, 1.0)
N_GEOM = 6
_f = lambda names: [(s, float(s)) for s in names]
# theta_i = theta_j; 1e-10 is so3_exp_q's switch (one value on each side), 1e-4 that of so3_Jr / so3_Jr_inv
LADDER_I = _f(("1e-12", "0.99e-10", "1.01e-10", "1e-7", "9.9e-5", "1.01e-4", "3e-4", "1e-3", "1e-2", "0.1", "1", "3"))
# the rotation residual; so3_log_q's series switch is |imag q| = sin(theta / 2) = 1e-10: theta = 2e-10, one value on each side
LADDER_R = LADDER_I[:3] + _f(("1.98e-10", "2.02e-10")) + LADDER_I[3:]
NEAR_PI = _f(("1e-3", "1e-6", "1e-9", "1e-11"))
DBG = _f(("0", "1e-8", "1e-3", "0.3"))
ROTS = _f(("1e-7", "0.99e-5", "1.01e-5", "3e-5", "1e-4", "1e-3", "0.1"))
LENGTHS = (0, 1, 2, 31, 32, 33, 200)
COV_LENGTHS = (2, 10, 200, 2000)          # one sample gives a covariance of rank 12 (position and velocity noise proportional)


def _intervals():
    out = [dict(name="empty_a", fam="empty", n=0, rot=1e-3, bias=False, jitter=False), dict(name="empty_b", fam="empty", n=0, rot=1e-3, bias=True, jitter=False)]
    for ir, (rn, rot) in enumerate(ROTS):
        for il, n in enumerate(LENGTHS[1:]):
            out.append(dict(name="rot_%s_%d" % (rn, n), fam="rot_" + rn, n=n, rot=rot, bias=(ir + il) % 2 == 1, jitter=(ir + 2 * il) % 3 == 0))
    for k, n in enumerate(COV_LENGTHS):
        out.append(dict(name="cov_%d" % n, fam="cov", n=n, rot=2e-3, bias=k % 2 == 0, jitter=k % 2 == 1))
    for k, s in enumerate(out):
        s["k"] = k
    return out


INTERVALS = _intervals()


def interval_samples(spec, seed):
    """-> (samples (n, 7), bg, ba): |(gyro - bg) dt| = spec["rot"] to rounding for every sample, a slowly turning axis, dt 5 ms
    constant or jittered by +-20 %, acceleration near (0, 0, 1) g"""
    n, k = spec["n"], spec["k"] + int(seed) % 1000
    i = np.arange(n, dtype=np.int64)
    u = lambda p, q, m: ((i * p + q + 7 * k) % m) / float(m) - 0.5
    dt = 0.005 * (1.0 + 0.4 * u(37, 11, 101)) if spec["jitter"] else np.full(n, 0.005)
    d = np.stack([0.6 + 0.3 * u(13, 5, 89), -0.48 + 0.3 * u(29, 3, 97), 0.64 + 0.3 * u(31, 17, 83)], 1)
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    bg = np.array([0.011, -0.007, 0.004]) if spec["bias"] else np.zeros(3)
    ba = np.array([0.05, 0.02, -0.03]) if spec["bias"] else np.zeros(3)
    gyro = bg[None, :] + d * (spec["rot"] / dt)[:, None]
    acc = np.stack([0.2 * u(41, 2, 103), 0.2 * u(43, 19, 107), 1.0 + 0.2 * u(47, 23, 109)], 1)
    return np.concatenate([gyro, acc, dt[:, None]], 1).reshape(n, 7), bg, ba


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _rot(w):
    from scipy.spatial.transform import Rotation as Rsc
    return Rsc.from_rotvec(w).as_matrix()


def jl(t):
    return 1 + 0.5 * t + t * t / 6


def jinv(t):
    return 1 + 0.5 * t + 0.1 * t * t


# ---- units ------------------------------------------------------------------------------------------------------------------
U_R = 4 * EPS          # an entry of exp(w) for a w given in doubles: sin, cos, the quaternion's products


def factor_units(x, p, r, qw, qn):
    """x (30), p: the record's fields, r: the exact residual (15), qw / qn: cos / sin of half the exact rotation residual
    -> (u_r (15), u_J (15, 30))"""
    Pi, wi, Vi, bgi, bai, Pj, wj, Vj = x[0:3], x[3:6], x[6:9], x[9:12], x[12:15], x[15:18], x[18:21], x[21:24]
    dt, g = p["dt"], GRAV
    RiT = np.abs(_rot(wi).T)                                   # magnitudes only
    dbg, dba = np.abs(bgi - p["bg"]), np.abs(bai - p["ba"])
    a = Pj - Pi - Vi * dt - 0.5 * g * dt * dt
    b = Vj - Vi - g * dt
    u_a = EPS * (np.abs(Pj) + np.abs(Pi) + 2 * np.abs(Vi) * dt + np.abs(g) * dt * dt + np.abs(a))     # the sum, term by term
    u_b = EPS * (np.abs(Vj) + np.abs(Vi) + 2 * np.abs(g) * dt + np.abs(b))
    # Ri' a: the rounded a through |Ri'|, the dot product, the entries of Ri
    u_Ra = RiT @ (u_a + 3 * EPS * np.abs(a)) + U_R * np.abs(a).sum()
    u_Rb = RiT @ (u_b + 3 * EPS * np.abs(b)) + U_R * np.abs(b).sum()
    cp = np.abs(p["Jpbg"]) @ dbg + np.abs(p["Jpba"]) @ dba
    cv = np.abs(p["Jvbg"]) @ dbg + np.abs(p["Jvba"]) @ dba
    u_r = np.zeros(15)
    u_r[0:3] = u_Ra + EPS * (2 * np.abs(p["dp"]) + 5 * cp + np.abs(r[0:3]))
    u_r[6:9] = u_Rb + EPS * (2 * np.abs(p["dv"]) + 5 * cv + np.abs(r[6:9]))
    u_r[9:15] = EPS * np.abs(r[9:15])
    # E = (dR exp(jd))' Ri' Rj: dq stored in doubles and its matrix (8 eps), exp(jd) with jd = Jrbg dbg rounded, Ri, Rj, three products
    jd = np.abs(p["Jrbg"]) @ dbg
    u_E = 8 * EPS + 3 * U_R + 9 * EPS + 4 * EPS * jd.sum()
    thr = _norm(r[3:6])
    # log: |d log / dE| <= |Jr^-1|, two entries per component; the reference's branch |qw| < 1e-10 returns pi / n and so drops
    # 2 atan(|qw| / n) of the angle -- transcribed behaviour, derived from the exact qw, not measured
    trunc = 2 * np.arctan(abs(qw) / qn) * np.abs(r[3:6]) / thr if abs(qw) < 1e-10 else 0.0
    u_rR = 2 * jinv(thr) * u_E + EPS * np.abs(r[3:6])
    u_r[3:6] = u_rR + trunc
    u_J = np.zeros((15, 30))
    thi, thj, thd = _norm(wi), _norm(wj), _norm(p["Jrbg"] @ (bgi - p["bg"]))
    u_Jr = lambda t: 6 * EPS * jl(t)                            # an entry of Jr(w)
    # rows of Ri' (a) and Ri' (b): +-Ri', -dt Ri', [Ri' a]x Jr(theta_i); -Jpbg, -Jpba, -Jvbg, -Jvba are exact copies
    Ri_T = _rot(wi).T
    for r0, Rv, u_Rv in ((0, np.abs(Ri_T @ a), u_Ra), (6, np.abs(Ri_T @ b), u_Rb)):
        u_J[r0:r0 + 3, r0:r0 + 3] = U_R                        # -Ri': the columns of P_i (position rows), of V_i (velocity rows)
        u_J[r0:r0 + 3, 15 + r0:18 + r0] = U_R                  # +Ri': P_j, V_j
        u_J[r0:r0 + 3, 3:6] = u_Rv.sum() * jl(thi) + Rv.sum() * (u_Jr(thi) + 3 * EPS * jl(thi))
    u_J[0:3, 6:9] = dt * (U_R + EPS)
    # rotation rows: Jr^-1(rR) (Rj' Ri) Jr(theta_i); Jr^-1(rR) E' Jr(jd) Jrbg; Jr^-1(rR) Jr(theta_j).  Jr^-1 is evaluated at the
    # computed rR: |d Jr^-1 / dw| <= 0.5 + 0.2 theta
    u_Ji = 6 * EPS * jinv(thr) + (0.5 + 0.2 * thr) * u_rR.max()
    common = 3 * u_Ji + 40 * EPS * jinv(thr)
    u_J[3:6, 3:6] = jl(thi) * common
    u_J[3:6, 18:21] = jl(thj) * common
    u_J[3:6, 9:12] = (np.abs(p["Jrbg"]).sum(0) * jl(thd) * (common + 3 * jinv(thr) * u_E))[None, :]
    return u_r, u_J


def preint_units(samples, bg, ba):
    """the recurrence of the pre-integration run on absolute values, times n eps: an error of eps relative made at any of the n
    steps reaches the result through the |A| of the later ones"""
    n = len(samples)
    Jh, Ch, dph, dvh, R, dth = np.eye(15), np.zeros((15, 15)), np.zeros(3), np.zeros(3), np.eye(3), 0.0
    noise = np.diag([GYR_N ** 2] * 3 + [ACC_N ** 2] * 3 + [GYR_W ** 2] * 3 + [ACC_W ** 2] * 3)
    for m in samples:
        acc, dt = np.abs(m[3:6] * GNORM) + np.abs(ba), m[6]
        gdt = (m[0:3] - bg) * dt
        t = _norm(gdt)
        aR = np.abs(R)
        hacc = np.array([[0, acc[2], acc[1]], [acc[2], 0, acc[0]], [acc[1], acc[0], 0]])
        Jr = jl(t) * np.ones((3, 3)) if t > 1e-5 else np.eye(3)
        A = np.eye(15)
        A[0:3, 3:6], A[0:3, 6:9], A[0:3, 12:15] = 0.5 * dt * dt * aR @ hacc, np.eye(3) * dt, 0.5 * dt * dt * aR
        A[3:6, 3:6], A[3:6, 9:12] = np.abs(_rot(gdt).T), Jr * dt
        A[6:9, 3:6], A[6:9, 12:15] = dt * aR @ hacc, dt * aR
        B = np.zeros((15, 12))
        B[0:3, 3:6], B[3:6, 0:3], B[6:9, 3:6], B[9:12, 6:9], B[12:15, 9:12] = 0.5 * dt * dt * aR, Jr * dt, dt * aR, np.eye(3) * dt, np.eye(3) * dt
        Jh, Ch = A @ Jh, A @ Ch @ A.T + B @ noise @ B.T
        dph = dph + dvh * dt + 0.5 * dt * dt * aR @ acc
        dvh = dvh + dt * aR @ acc
        R = R @ _rot(gdt)
        dth += dt
    s = EPS * n
    return dict(dp=s * dph, dv=s * dvh, dq=s * np.ones(4), dtime=s * dth, jacobian=s * Jh, covariance=s * Ch)


def prior_units(x, x0, dx, cost, qw, qn):
    u = EPS * np.abs(dx)
    thr = _norm(dx[3:6])
    u_E = 2 * U_R + 3 * EPS
    trunc = 2 * np.arctan(abs(qw) / qn) * np.abs(dx[3:6]) / thr if abs(qw) < 1e-10 else 0.0
    u[3:6] = 2 * jinv(thr) * u_E + EPS * np.abs(dx[3:6]) + trunc
    return u, (np.abs(dx) * u).sum() + 16 * EPS * cost


def whitened_units(f, c, r, u_r, J=None, u_J=None):
    """units of U r and U J for covariance c of the fixture.  U = chol(cov^-1)': what cov^-1 amplifies is inherent to the
    operation -- the condition number of the covariance scaled to a unit diagonal (the one an inverse through a Cholesky factor
    sees) times eps.  A perturbation of cov^-1 = U'U of that relative size, d_i d_k with d_k = (cov^-1)_kk^1/2 = |U[:, k]|, moves
    U[i, k] by about d_k whether or not the entry is zero"""
    U, cond = np.abs(f["w_U"][c]), f["w_cond"][c]
    Uh = np.triu(np.tile(np.sqrt((U * U).sum(0))[None, :], (15, 1)))
    u_rw = U @ u_r + EPS * cond * (Uh @ np.abs(r))
    return u_rw, None if J is None else U @ u_J + EPS * cond * (Uh @ np.abs(J))


def cost_of(r):
    r = np.asarray(r, np.longdouble)
    return float(0.5 * (r * r).sum())


def cost_unit(r, u_r):
    return float((np.abs(r) * u_r).sum() + 32 * EPS * cost_of(r))


def whitened_factor_cost(f, it, c):
    """a raw factor item under covariance c of the fixture: the exact cost |U r|^2 / 2 (U and r each rounded once, their product
    in extended precision) and its unit"""
    rw = (f["w_U"][c].astype(np.longdouble) @ it["r"].astype(np.longdouble)).astype(np.float64)
    u_rw, _ = whitened_units(f, c, it["r"], it["u_r"])
    return cost_of(rw), cost_unit(rw, u_rw)


# ---- loading ----------------------------------------------------------------------------------------------------------------
PRE_KEYS = ("dp", "dv", "dq", "dt", "bg", "ba", "Jpbg", "Jpba", "Jrbg", "Jvbg", "Jvba")


def load(path=KAT):
    z = np.load(path)
    f = {k: z[k] for k in z.files}
    seed = int(f["seed"])
    for key in ("f_families", "d_families"):
        f[key] = [str(s) for s in f[key]]
    # (c) the intervals: samples from the formula, exact results, units
    iu = np.triu_indices(15)
    f["p"] = []
    for k, spec in enumerate(INTERVALS):
        smp, bg, ba = interval_samples(spec, seed)
        cov = np.zeros((15, 15))
        cov[iu] = f["p_cov"][k]
        cov = cov + np.triu(cov, 1).T
        f["p"].append(dict(spec=spec, samples=smp, bg=bg, ba=ba, units=preint_units(smp, bg, ba),
                           exact=dict(dp=f["p_dp"][k], dv=f["p_dv"][k], dq=f["p_dq"][k], dtime=f["p_dtime"][k], jacobian=f["p_jacobian"][k], covariance=cov)))
    # (a) raw factor items
    f["f"] = []
    for i in range(len(f["f_x"])):
        p = {k: f["f_" + k][i] for k in PRE_KEYS}
        u_r, u_J = factor_units(f["f_x"][i], p, f["f_r"][i], f["f_qw"][i], f["f_qn"][i])
        f["f"].append(dict(x=f["f_x"][i], pre=p, r=f["f_r"][i], J=f["f_J"][i], has_J=bool(f["f_has_J"][i]), u_r=u_r, u_J=u_J, fam=f["f_families"][f["f_fam"][i]],
                           truncated=abs(f["f_qw"][i]) < 1e-10))
    # (b) whitening items: the record is an interval's exact result as doubles
    f["w"] = []
    for i in range(len(f["w_x"])):
        c = int(f["w_cov"][i])
        e = f["p"][int(f["w_interval"][c])]["exact"]
        Jm = e["jacobian"]
        p = dict(dp=e["dp"], dv=e["dv"], dq=e["dq"], dt=e["dtime"], bg=f["p"][int(f["w_interval"][c])]["bg"], ba=f["p"][int(f["w_interval"][c])]["ba"],
                 Jpbg=Jm[0:3, 9:12], Jpba=Jm[0:3, 12:15], Jrbg=Jm[3:6, 9:12], Jvbg=Jm[6:9, 9:12], Jvba=Jm[6:9, 12:15])
        u_r, u_J = factor_units(f["w_x"][i], p, f["w_r"][i], f["w_qw"][i], f["w_qn"][i])
        u_rw, u_Jw = whitened_units(f, c, f["w_r"][i], u_r, f["w_J"][i], u_J)
        f["w"].append(dict(x=f["w_x"][i], pre=p, cov=e["covariance"], jacobian=Jm, c=c, rw=f["w_rw"][i], Jw=f["w_Jw"][i], u_rw=u_rw, u_Jw=u_Jw,
                           cost=cost_of(f["w_rw"][i]), u_c=cost_unit(f["w_rw"][i], u_rw)))
    # (d) prior items
    f["d"] = []
    for i in range(len(f["d_x"])):
        u_dx, u_c = prior_units(f["d_x"][i], f["d_x0"][i], f["d_dx"][i], f["d_cost"][i], f["d_qw"][i], f["d_qn"][i])
        f["d"].append(dict(x=f["d_x"][i], x0=f["d_x0"][i], dx=f["d_dx"][i], cost=f["d_cost"][i], u_dx=u_dx, u_c=u_c, fam=f["d_families"][f["d_fam"][i]],
                           truncated=abs(f["d_qw"][i]) < 1e-10))
    return f


# ---- ratios -----------------------------------------------------------------------------------------------------------------
def ratio(err, unit):
    """worst |err| / unit; a zero unit admits a zero error alone"""
    err, unit = np.abs(np.asarray(err, float)).reshape(-1), np.broadcast_to(np.asarray(unit, float), np.shape(err)).reshape(-1)
    with np.errstate(all="ignore"):
        q = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if len(q) else 0.0


def _worst(d, name, fam, v):
    d.setdefault(name, {})
    d[name][fam] = max(d[name].get(fam, 0.0), v)


def factor_summary(f, raw):
    """raw(x, pre) -> (r (15), J (15, 30)) before the square-root information.  {quantity: {family: worst ratio}}"""
    out = {}
    for it in f["f"]:
        r, J = raw(it["x"], it["pre"])
        assert np.isfinite(r).all() and np.isfinite(J).all(), it["fam"]
        for name, rows in (("f_rp", slice(0, 3)), ("f_rr_tr" if it["truncated"] else "f_rr", slice(3, 6)), ("f_rv", slice(6, 9)), ("f_rb", slice(9, 15))):
            _worst(out, name, it["fam"], ratio(r[rows] - it["r"][rows], it["u_r"][rows]))
        if it["has_J"]:
            for name, rows in (("f_jp", slice(0, 3)), ("f_jr", slice(3, 6)), ("f_jv", slice(6, 9)), ("f_jb", slice(9, 15))):
                _worst(out, name, it["fam"], ratio(J[rows] - it["J"][rows], it["u_J"][rows]))
    return out


def whiten_summary(f, whitened):
    """whitened(x, pre, cov, jacobian) -> (r, J) with the square-root information applied; one quantity per covariance"""
    out = {}
    for it in f["w"]:
        r, J = whitened(it["x"], it["pre"], it["cov"], it["jacobian"])
        n = COV_LENGTHS[it["c"]]
        _worst(out, "w_r_%d" % n, "cov", ratio(r - it["rw"], it["u_rw"]))
        _worst(out, "w_j_%d" % n, "cov", ratio(J - it["Jw"], it["u_Jw"]))
    return out


def cost_items(f):
    """-> [(x, record fields, covariance, the record's jacobian or None, c, exact cost, unit, family)]: every raw factor item under one
    of the fixture's real covariances (item i under covariance i mod 4), and the whitening items under their own"""
    out = []
    for i, it in enumerate(f["f"]):
        c = i % len(COV_LENGTHS)
        cost, u = whitened_factor_cost(f, it, c)
        out.append((it["x"], it["pre"], f["p"][int(f["w_interval"][c])]["exact"]["covariance"], None, c, cost, u, it["fam"] + ("!" if it["truncated"] else "")))
    for it in f["w"]:
        out.append((it["x"], it["pre"], it["cov"], it["jacobian"], it["c"], it["cost"], it["u_c"], "cov"))
    return out


def cost_summary(f, costs):
    """costs: |U r|^2 / 2 of every entry of cost_items(f); one quantity per covariance"""
    out = {}
    for (x, p, cov, jac, c, cost, u, fam), got in zip(cost_items(f), costs):
        assert np.isfinite(got)
        # (the items of the reference's |qw| < 1e-10 branch, marked "!", are not pooled with the rest)
        _worst(out, "c_tr" if fam.endswith("!") else "c_%d" % COV_LENGTHS[c], fam.rstrip("!"), ratio(got - cost, u))
    return out


def preint_summary(f, results):
    """results: one dict (dp, dv, dq, dtime, jacobian (15, 15), covariance (15, 15)) per interval of INTERVALS"""
    out = {}
    for p, got in zip(f["p"], results):
        e, u, fam = p["exact"], p["units"], p["spec"]["fam"]
        for name, key in (("p_dp", "dp"), ("p_dv", "dv"), ("p_dt", "dtime"), ("p_cov", "covariance")):
            _worst(out, name, fam, ratio(np.asarray(got[key]) - e[key], u[key]))
        q = np.asarray(got["dq"])
        assert q[3] >= 0
        dq = q - e["dq"] if abs(e["dq"][3]) > 1e-6 else np.minimum(np.abs(q - e["dq"]), np.abs(q + e["dq"]))
        _worst(out, "p_dq", fam, ratio(dq, u["dq"]))
        dJ = np.asarray(got["jacobian"]) - e["jacobian"]
        bgc = np.zeros((15, 15), bool)
        bgc[:, 9:12] = True                                    # the columns of the gyro bias: every entry there went through Jr
        _worst(out, "p_jbg", fam, ratio(dJ[bgc], u["jacobian"][bgc]))
        _worst(out, "p_jac", fam, ratio(dJ[~bgc], u["jacobian"][~bgc]))
    return out


def prior_summary(f, evaluate):
    """evaluate(x, x0) -> (g (15), cost) of a one-frame problem with the prior J = I, r0 = 0 alone"""
    out = {}
    for it in f["d"]:
        g, c = evaluate(it["x"], it["x0"])
        assert np.isfinite(g).all() and np.isfinite(c)
        tr = "_tr" if it["truncated"] else ""                  # the items of the reference's |qw| < 1e-10 branch are not pooled with the rest
        _worst(out, "d_g" + tr, it["fam"], ratio(g - it["dx"], it["u_dx"]))
        _worst(out, "d_c" + tr, it["fam"], ratio(c - it["cost"], it["u_c"]))
    return out


# ---- the oracle's worst ratios over the whole fixture (measured on the CPU, tabulated in tests/test_imu_kat.py); the bounds are
# 8 x these for the oracle, the library on the host and the device alike
MEASURED = {"f_rp": 0.125, "f_rr": 0.02, "f_rv": 0.127, "f_rb": 0.0, "f_jp": 0.438, "f_jr": 0.014, "f_jv": 0.438, "f_jb": 0.0, "f_rr_tr": 0.996,
            "w_r_2": 0.041, "w_j_2": 0.085, "w_r_10": 0.056, "w_j_10": 0.173, "w_r_200": 0.042, "w_j_200": 0.122, "w_r_2000": 0.058, "w_j_2000": 0.052,
            "p_dp": 0.972, "p_dv": 0.91, "p_dt": 0.079, "p_cov": 1.038, "p_dq": 0.5, "p_jbg": 0.955, "p_jac": 0.972,
            "d_g": 0.05, "d_c": 0.101, "d_g_tr": 0.999, "d_c_tr": 0.998, "c_2": 0.028, "c_10": 0.028, "c_200": 0.012, "c_2000": 0.011, "c_tr": 0.99}
BOUNDS = {k: 8 * v for k, v in MEASURED.items()}
SMALL_ANGLE_FACTOR = 4.0


def worst(per_family):
    return max(per_family.values())


def report(who, ratios):
    """prints every family's ratio; -> the (quantity, family, ratio) outside the bounds"""
    for name, per_family in ratios.items():
        for fam, r in per_family.items():
            print("%s %-8s %-14s %10.3f (bound %.2f)" % (who, name, fam, r, BOUNDS.get(name, float("nan"))))
    return [(n, fam, r) for n, pf in ratios.items() for fam, r in pf.items() if not r <= BOUNDS[n]]


def _ladder(fam):
    return float(fam.split("_", 1)[1])


def small_angle_condition(ratios):
    """{(quantity, ladder): (worst small, worst large)}: the Jacobian blocks that carry Jr or Jr^-1 over theta in (1e-12, 1e-2]
    against [0.1, 1], per ladder; the pre-integration's gyro-bias Jacobian and covariance over |gyr dt| in (1e-5, 1e-3] against 0.1"""
    out = {}
    for name in ("f_jp", "f_jr", "f_jv"):
        for lad in ("thi_", "thr_"):
            pf = {k: v for k, v in ratios.get(name, {}).items() if k.startswith(lad)}
            if pf:
                small = [v for k, v in pf.items() if 1e-12 < _ladder(k) <= 1e-2]
                large = [v for k, v in pf.items() if 0.1 <= _ladder(k) <= 1]
                assert len(small) >= 8 and len(large) == 2
                out[name, lad] = (max(small), max(large))
    for name in ("p_jbg", "p_cov"):
        pf = {k: v for k, v in ratios.get(name, {}).items() if k.startswith("rot_")}
        if pf:
            small = [v for k, v in pf.items() if 1e-5 < _ladder(k) <= 1e-3]
            assert len(small) == 4
            out[name, "rot_"] = (max(small), pf["rot_0.1"])
    return out


def check_small_angles(who, ratios):
    cond = small_angle_condition(ratios)
    for (name, lad), (small, large) in cond.items():
        print("%s %s %s small angles %.3g, large %.3g" % (who, name, lad, small, large))
    bad = {k: v for k, v in cond.items() if not v[0] <= SMALL_ANGLE_FACTOR * v[1]}
    assert not bad, "%s: the error grows as the angle shrinks: %s" % (who, bad)


def check(who, ratios, small_angles=True):
    bad = report(who, ratios)
    if small_angles:
        check_small_angles(who, ratios)
    assert not bad, "%s outside the bound: %s" % (who, bad)
    return ratios


# ---- the implementations ----------------------------------------------------------------------------------------------------
def oracle_pre(IO, p, cov=None, jacobian=None):
    from scipy.spatial.transform import Rotation as Rsc
    J = np.eye(15) if jacobian is None else np.array(jacobian)
    if jacobian is None:
        J[0:3, 9:12], J[0:3, 12:15], J[3:6, 9:12], J[6:9, 9:12], J[6:9, 12:15] = p["Jpbg"], p["Jpba"], p["Jrbg"], p["Jvbg"], p["Jvba"]
    return dict(dp=p["dp"], dv=p["dv"], dR=Rsc.from_quat(p["dq"]).as_matrix(), dtime=float(p["dt"]), bg=p["bg"], ba=p["ba"], jacobian=J,
                covariance=np.eye(15) if cov is None else cov)


def oracle_raw(IO):
    def raw(x, p):
        pre = oracle_pre(IO, p)
        return IO.imu_residual_raw(pre, GRAV, x[0:6], x[6:15], x[15:21], x[21:30]), IO.imu_jacobian_raw(pre, GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
    return raw


def oracle_whitened(IO):
    def whitened(x, p, cov, jacobian):
        pre = oracle_pre(IO, p, cov, jacobian)
        U = IO.sqrt_info(cov)
        return U @ IO.imu_residual_raw(pre, GRAV, x[0:6], x[6:15], x[15:21], x[21:30]), U @ IO.imu_jacobian_raw(pre, GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
    return whitened


def oracle_costs(IO, f):
    out = []
    for x, p, cov, jac, c, _, _, _ in cost_items(f):
        r = IO.sqrt_info(cov) @ IO.imu_residual_raw(oracle_pre(IO, p, cov, jac), GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
        out.append(0.5 * float(r @ r))
    return out


def library_costs(M, f):
    out = []
    for x, p, cov, jac, c, _, _, _ in cost_items(f):
        r, _ = M.imu_factor(library_record(M, p, cov, jac), GRAV, x[0:6], x[6:15], x[15:21], x[21:30], jac=False)
        out.append(0.5 * float(r @ r))
    return out


def oracle_preint(IO, f):
    from scipy.spatial.transform import Rotation as Rsc
    out = []
    for p in f["p"]:
        o = IO.preintegrate(p["samples"], p["bg"], p["ba"])
        q = Rsc.from_matrix(o["dR"]).as_quat()
        o["dq"] = -q if q[3] < 0 else q
        out.append(o)
    return out


def oracle_prior(IO):
    def evaluate(x, x0):
        dx = IO.prior_residual(dict(x0=x0, r0=np.zeros(15), J=np.eye(15)), x)
        return dx, 0.5 * float(dx @ dx)
    return evaluate


def library_record(M, p, cov=None, jacobian=None):
    pre = M.ImuPreint()
    J = oracle_pre(None, p, cov, jacobian)["jacobian"]
    pre.dp[:], pre.dv[:], pre.dq[:], pre.dtime = list(p["dp"]), list(p["dv"]), list(p["dq"]), float(p["dt"])
    pre.bg[:], pre.ba[:] = list(p["bg"]), list(p["ba"])
    pre.jacobian[:] = list(J.reshape(-1))
    pre.covariance[:] = list((np.eye(15) if cov is None else np.asarray(cov)).reshape(-1))
    return pre


def library_raw(M):
    def raw(x, p):
        return M.imu_factor(library_record(M, p), GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
    return raw


def library_whitened(M):
    def whitened(x, p, cov, jacobian):
        return M.imu_factor(library_record(M, p, cov, jacobian), GRAV, x[0:6], x[6:15], x[15:21], x[21:30])
    return whitened


def library_results(pres):
    return [dict(dp=np.array(p.dp), dv=np.array(p.dv), dq=np.array(p.dq), dtime=p.dtime, jacobian=np.array(p.jacobian).reshape(15, 15),
                 covariance=np.array(p.covariance).reshape(15, 15)) for p in pres]


def library_prior(M):
    fw = M.FullWindowSolver(1)

    def evaluate(x, x0):
        pr = M.Prior()
        pr.J[:], pr.r0[:], pr.x0[:] = list(np.eye(15).reshape(-1)), [0.0] * 15, list(x0)
        fw.set_prior(pr)
        _, g, c = fw.normal_equations(np.zeros((1, 32)), x[None])
        return g, c
    return evaluate
