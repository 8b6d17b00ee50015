"""Known answers for RemoveLidarDistortion (csrc/undistort_dev.h, oracle/estimate.cpp:mmlo_undistort), computed with neither
implementation: tests/undistort_checks.py:sequence in numpy.longdouble, every stored point confirmed with mpmath at 50 digits.
Data only: tests/golden/undistort_kat.npz.  Deterministic, CPU only, run by no test (a few minutes on 8 cores).

    python tests/golden/make_undistort_kat.py [seed]

Per motion (one sweep motion dR, dt each; `names`, `quat_branch`, `linear`, `w_negative`, `theta` say which branches it takes):
  * a random set of N_RANDOM points: ranges 1, 10 and 60 m mixed, s uniform in [0, 1] plus the special values, a few points with
    one coordinate exactly 0 and a few closer than 1 mm;
  * a guard set of 128 .. 256 points mined from N_MINE random candidates: at least one coordinate whose exact value lies within
    [8 B, 5e-14] * scale of a float rounding boundary, the margins spread over that interval as evenly in log as the candidates
    allow (they are uniform, not log-uniform: the low end is thin).
B is measured here: the largest |oracle's double result - exact| / scale over every candidate evaluated.  Points with a coordinate
closer than 8 B to a boundary are redrawn (random set) or not taken (guard set), so every stored coordinate is decidable.
"""
import math
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import undistort_checks as K  # noqa: E402

N_RANDOM = 768
N_MINE = 8400000            # candidates per motion
CHUNK = 200000
GUARD_MIN, GUARD_MAX, GUARD_BINS = 128, 256, 8
S_SPECIAL = np.array([0.0, 1.0, 0.5, 1e-6, np.nextafter(np.float32(1), np.float32(0))], np.float32)
DEG = np.pi / 180


def rodrigues(rotvec):
    v = np.asarray(rotvec, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    n = v / a
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def about(angle, axis):
    a = np.asarray(axis, np.float64)
    return angle * a / np.linalg.norm(a)


# name, rotation vector, float32-rounded matrix?, what the generator asserts of it: (quat_branch, linear, w_negative, theta range)
MOTIONS = [
    ("identity", (0, 0, 0), False, (K.TRACE_POS, True, False, (0, 0))),
    ("1e-7 rad", about(1e-7, (0.3, -0.5, 0.8)), False, (K.TRACE_POS, False, False, (4e-8, 6e-8))),
    ("0.02 rad", about(0.02, (0.1, -0.2, 0.97)), False, (K.TRACE_POS, False, False, (0.0099, 0.0101))),
    ("0.999 rad", about(0.999, (0.5, 0.4, -0.7)), False, (K.TRACE_POS, False, False, (0.499, 0.5))),
    ("1.001 rad", about(1.001, (0.5, 0.4, -0.7)), False, (K.TRACE_POS, False, False, (0.5, 0.501))),
    ("2 rad", about(2.0, (-0.6, 0.7, 0.4)), False, (K.TRACE_POS, False, False, (0.99, 1.01))),
    ("120.5 deg, x", about(120.5 * DEG, (1, 0.3, 0.2)), False, (K.DIAG0, False, False, (1.05, 1.06))),
    ("170 deg, y", about(170 * DEG, (0.2, 1, 0.3)), False, (K.DIAG1, False, False, (1.48, 1.49))),
    ("120.5 deg, z", about(120.5 * DEG, (0.3, 0.2, 1)), False, (K.DIAG2, False, False, (1.05, 1.06))),
    ("170 deg, z", about(170 * DEG, (-0.2, 0.3, 1)), False, (K.DIAG2, False, False, (1.48, 1.49))),
    ("170 deg, -x: w < 0", about(170 * DEG, (-1, 0, 0.01)), False, (K.DIAG0, False, True, (1.48, 1.49))),
    ("179.99 deg", about(179.99 * DEG, (0.4, -0.8, 0.45)), False, (K.DIAG1, False, None, (1.5707, 1.5708))),
    ("pi", about(np.pi, (0.6, 0.3, 0.74)), False, (K.DIAG2, False, None, (1.5707, 1.5708))),
    ("0.02 rad, float matrix", about(0.02, (-0.3, 0.9, 0.3)), True, (K.TRACE_POS, False, False, (0.0099, 0.0101))),
]


class Double:
    num, sqrt = staticmethod(float), staticmethod(math.sqrt)


def directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def random_points(rng, n):
    """ranges 1, 10 and 60 m mixed (0.2 .. 1 of each), s uniform in [0, 1]"""
    r = rng.choice([1.0, 10.0, 60.0], n) * rng.uniform(0.2, 1.0, n)
    return (directions(rng, n) * r[:, None]).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)


def random_set(rng):
    xyz, s = random_points(rng, N_RANDOM)
    k = len(S_SPECIAL)
    s[:k] = S_SPECIAL
    s[k:k + 8] = np.concatenate([rng.uniform(-0.05, 0, 4), rng.uniform(1, 1.05, 4)]).astype(np.float32)
    for i in range(12):                                   # one coordinate exactly 0
        xyz[k + 8 + i, i % 3] = 0.0
    xyz[k + 20:k + 32] = (directions(rng, 12) * rng.uniform(1e-5, 1e-3, (12, 1))).astype(np.float32)   # closer than 1 mm
    s[k + 20] = 1.0
    s[k + 21] = 0.0
    return xyz, s


def evaluate(dR, dt, xyz, s, O):
    """exact values, their floats and margins, the oracle's double error (/ scale) and whether its float is the exact value's"""
    scale = K.scale_of(xyz, dt)
    v, _ = K.exact_ld(dR, dt, xyz, s)
    ref, mg = K.margins_ld(v, scale)
    dbl = K.oracle_double(dR, dt, xyz, s)
    got = O.undistort(xyz, s, dR, dt)
    assert np.array_equal(dbl.astype(np.float32).view(np.uint32), got.view(np.uint32)), "oracle_double is not mmlo_undistort"
    err = (np.abs(K.LD.num(dbl) - v) / K.LD.num(scale)[:, None]).astype(np.float64)
    return v, ref, mg, err, got.view(np.uint32) != ref.view(np.uint32)


def mine(job):
    """one chunk of one motion's candidates -> worst oracle error, the mismatching coordinates, the candidates near a boundary"""
    m, c, dR, dt, seed = job
    import mml_oracle as O
    rng = np.random.default_rng([seed, 1000 + m, c])
    xyz, s = random_points(rng, CHUNK)
    v, ref, mg, err, mism = evaluate(dR, dt, xyz, s, O)
    near = mg.min(1) <= K.GUARD_HI
    return m, float(err.max()), np.stack([mg[mism], err[mism]], 1), xyz[near], s[near], ref[near], mg[near], v[near]


def confirm(job):
    """mpmath at 50 digits on stored points: |longdouble - mpmath| / scale, and the floats agree"""
    dR, dt, xyz, s, v, ref = job
    A = K.MP(50)
    worst = 0.0
    for p, t, vl, r in zip(xyz, s, v, ref):
        e, _ = K.exact_mp(A, dR, dt, p, t)
        sc = float(K.scale_of(p, dt))
        for c in range(3):
            f, _ = K.margin_mp(A, e[c], sc)
            assert f.view(np.uint32) == r[c].view(np.uint32), (p, t, c, f, r[c])
            worst = max(worst, float(abs(e[c] - _mpf_of_ld(vl[c])) / sc))
    return worst


def _mpf_of_ld(x):
    """a longdouble as an mpf, exactly: split into two doubles"""
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def pick_guard(mg_min, lo):
    """indices of up to GUARD_MAX candidates with lo <= mg_min <= GUARD_HI, as even in log as the supply allows: equal quotas per
    log bin, what a thin bin leaves goes to the others"""
    edges = np.geomspace(lo, K.GUARD_HI, GUARD_BINS + 1)
    bins = [list(np.flatnonzero((mg_min >= edges[b]) & (mg_min <= edges[b + 1] if b == GUARD_BINS - 1 else mg_min < edges[b + 1])))
            for b in range(GUARD_BINS)]
    take = [[] for _ in bins]
    left = GUARD_MAX
    while left > 0 and any(bins):
        live = [b for b in range(GUARD_BINS) if bins[b]]
        quota = max(left // len(live), 1)
        for b in live:
            k = min(quota, len(bins[b]), left)
            take[b] += bins[b][:k]
            bins[b] = bins[b][k:]
            left -= k
    return np.sort(np.concatenate([np.asarray(t, np.int64) for t in take]))


def main(seed=20250611):
    import mml_oracle as O
    O.build()
    rng = np.random.default_rng(seed)
    dRs, dts, infos = [], [], []
    for name, rv, as_float, want in MOTIONS:
        dR = rodrigues(rv)
        if as_float:
            dR = dR.astype(np.float32).astype(np.float64)
            assert np.abs(dR.T @ dR - np.eye(3)).max() > 1e-9          # not orthonormal
        dt = rng.normal(0, 0.3, 3)
        _, info = K.exact_ld(dR, dt, np.ones((1, 3), np.float32), np.ones(1, np.float32))
        br, lin, wneg, (t0, t1) = want
        assert info["quat_branch"] == br and info["linear"] == lin and t0 <= info["theta"] <= t1, (name, info)
        assert wneg is None or info["w_negative"] == wneg, (name, info)
        assert K.motion_quat(Double, dR)[1] == br              # (the double evaluation takes the same rule)
        dRs.append(dR.reshape(9))
        dts.append(dt)
        infos.append(info)
    assert {i["quat_branch"] for i in infos} == {0, 1, 2, 3} and any(i["w_negative"] for i in infos) and any(i["linear"] for i in infos)
    assert any(i["theta"] < 0.5 for i in infos[3:4]) and any(i["theta"] >= 0.5 for i in infos[4:5])
    nm = len(MOTIONS)

    # -- candidates: B, the mismatches, the points near a boundary
    jobs = [(m, c, dRs[m], dts[m], seed) for m in range(nm) for c in range(N_MINE // CHUNK)]
    B, mism, near = 0.0, [], [[] for _ in range(nm)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for m, e, mm, *cand in pool.imap(mine, jobs, chunksize=1):
            B = max(B, e)
            mism.append(mm)
            near[m].append(cand)
    mism = np.concatenate(mism)
    n_cand = nm * N_MINE

    # -- random sets, redrawn until every coordinate is decidable (B can only grow while doing so)
    sets = []
    for m in range(nm):
        xyz, s = random_set(rng)
        while True:
            v, ref, mg, err, mm = evaluate(dRs[m], dts[m], xyz, s, O)
            B = max(B, float(err.max()))
            bad = mg.astype(np.float32).min(1) < K.DECIDABLE * B
            if not bad.any():
                break
            print("motion %d: %d random points redrawn" % (m, bad.sum()))
            xyz[bad] = random_points(rng, int(bad.sum()))[0]
        n_cand += len(xyz)
        sets.append([xyz, s, ref, mg, v])
    for m in range(nm):      # (B is final now)
        assert sets[m][3].astype(np.float32).min() >= K.DECIDABLE * B

    # -- guard sets
    sizes = []
    for m in range(nm):
        xyz, s, ref, mg, v = [np.concatenate([c[k] for c in near[m]]) for k in range(5)]
        mgf = mg.astype(np.float32).astype(np.float64)
        ok = mgf.min(1) >= K.DECIDABLE * B
        pick = np.flatnonzero(ok)[pick_guard(mgf.min(1)[ok], K.DECIDABLE * B)]
        assert GUARD_MIN <= len(pick) <= GUARD_MAX, (m, len(pick), int(ok.sum()))
        sizes.append(len(pick))
        g = [a[pick] for a in (xyz, s, ref, mg, v)]
        sets[m] = [np.concatenate([a, b]) for a, b in zip(sets[m], g)]

    # -- every stored point again with mpmath
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        agree = max(pool.map(confirm, [(dRs[m], dts[m], sets[m][0], sets[m][1], sets[m][4], sets[m][2]) for m in range(nm)]))
    assert agree <= 1e-18, agree

    motion = np.concatenate([np.full(len(sets[m][0]), m, np.uint8) for m in range(nm)])
    guard = np.concatenate([np.arange(len(sets[m][0])) >= N_RANDOM for m in range(nm)])
    out = dict(B=np.float64(B), n_candidates=np.int64(n_cand), names=np.array([m[0] for m in MOTIONS]),
               rotvec=np.array([m[1] for m in MOTIONS], np.float64), dR=np.array(dRs), dt=np.array(dts),
               quat_branch=np.array([i["quat_branch"] for i in infos], np.uint8), linear=np.array([i["linear"] for i in infos]),
               w_negative=np.array([i["w_negative"] for i in infos]), theta=np.array([i["theta"] for i in infos]),
               motion=motion, guard=guard, xyz=np.concatenate([t[0] for t in sets]), s=np.concatenate([t[1] for t in sets]),
               ref=np.concatenate([t[2] for t in sets]), margin=np.concatenate([t[3] for t in sets]).astype(np.float32))
    path = os.path.join(HERE, "undistort_kat.npz")
    np.savez(path, **out)
    print("B = %.4g  (8 B = %.4g)" % (B, 8 * B))
    print("candidates evaluated: %d (%d coordinates)" % (n_cand, 3 * n_cand))
    print("oracle float != exact float at %d coordinates; their margins %s, the oracle's errors there %s"
          % (len(mism), np.array2string(mism[:, 0], precision=3), np.array2string(mism[:, 1], precision=3)))
    print("longdouble against mpmath: %.3g * scale" % agree)
    print("guard-set sizes:", sizes)
    for m in range(nm):
        i = infos[m]
        print("  %-24s quat branch %d linear %d w<0 %d theta %.9g" % (MOTIONS[m][0], i["quat_branch"], i["linear"], i["w_negative"], i["theta"]))
    print("%s: %d points, %d bytes" % (path, len(motion), os.path.getsize(path)))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
