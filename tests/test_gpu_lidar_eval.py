"""GPU suite: the device's lidar factor evaluation (csrc/lidar_eval.h: make_pose, the line and plane rows with their Jacobians,
sqrt_pair, huber, accum, block_reduce28) through the existing entry points, against the exact references of
tests/golden/lidar_eval_kat.npz.
  a. device against exact, one factor at a time: every item alone in a slot (factors_upload), evaluated by linearize_window
     (k_linearize; eight slots a launch, the call's limit), with the summary, the small-angle condition and the BOUNDS of
     tests/test_lidar_eval.py -- 8 x the oracle's worst ratios, never the device's.
     For the record (not a bound), the device's worst ratios on the MI355X: c_htt 0.350, c_htr 0.361,
     c_hrr 0.375, c_gt 0.347, c_gr 0.346, c_c 0.408; small angles against theta in [1e-2, 1]: 0.342 / 0.234, 0.335 / 0.229, 0.277 / 0.223.
  b. the reduction: lists of 0 + 0, 1 + 0, 0 + 1, 127, 128, 129, 257 factors of the one-pose family, lines only and planes only
     included, through linearize against the exactly rounded sum (math.fsum) of the stored exact records; unit
     eps log2(n) sum |term| plus the per-factor bounds (device: at most 0.006 of it).  No factor: exact zeros.
  c. the three solve kernels on the edge families: slots of generic factors (which fix the pose) mixed with the near-line and
     near-plane, exact-zero, gate, both-sides-of-Huber and negative-weight families, 127 / 128 / 129 and 1535 / 1536 / 1537
     planes (one round of twelve slots x 128 virtual threads of eval_frame_wide, and one more), start poses from the
     small-angle families and theta = 3; each slot solved alone in a default context (k_solve_wide), alone in a context
     created with MML_SOLVE_WIDE=0 (k_solve<true>) and in one launch of more slots than the device has CUs (k_solve<false>):
     identical bits of x, summary and trace, everything finite.  The factors are the fixture's identity-extrinsic items moved
     rigidly to the slot's pose; the float ends of a rotated line round, so the moved line families are near to 1e-5 m only.
     The distances that matter come from the exact-zero families instead (coordinates in multiples of 1/8, moved by their
     translation alone and exactly): three slots start with their 12 lines and 12 planes, at start rotations of 0 (exactly
     on: line_row's path through sqrt_pair's clamp), 2e-9 rad (about 1e-9 m off) and 3e-7 rad (about 1e-6 m off) and no
     translation; solve_cases asserts these distances.
"""
import math
import os

import numpy as np
import pytest

import lidar_eval_checks as K

pytestmark = pytest.mark.gpu
NONE = np.zeros((0, 10))
HUBER = 0.1 / 1.5e-3


@pytest.fixture(scope="module")
def kat():
    return K.load()


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=64, max_features=512, device=0)
    yield c
    c.close()


def device_evaluate(c, f):
    def evaluate(idx):
        H, g, cost = np.zeros((len(idx), 21)), np.zeros((len(idx), 6)), np.zeros(len(idx))
        key = np.stack([f["tbl"][idx], f["w_tan"][idx], f["delta"][idx]], 1)
        launches = 0
        for k in np.unique(key, axis=0):
            grp = idx[(key == k).all(1)]
            for at in range(0, len(grp), 8):
                part = grp[at:at + 8]
                first = at % 64                                  # walk through the context's 64 slots
                for j, i in enumerate(part):
                    one = f["rec"][i:i + 1]
                    c.factors_upload(first + j, 0, one if f["kind"][i] == 0 else NONE)
                    c.factors_upload(first + j, 1, one if f["kind"][i] == 1 else NONE)
                rec = c.linearize_window(first, len(part), f["x"][part], f["T_bl"][int(k[0])], w_tan=k[1], huber=k[2])
                H[np.searchsorted(idx, part)], g[np.searchsorted(idx, part)], cost[np.searchsorted(idx, part)] = rec[:, :21], rec[:, 21:27], rec[:, 27]
                launches += 1
        print("k_linearize launches:", launches)
        return H, g, cost
    return evaluate


def test_device_single_factors_against_exact(ctx, kat):
    ratios = K.check_against_exact(kat, device_evaluate(ctx, kat), "device")
    print("device worst ratios:", {k: "%.3f" % np.nanmax(list(v.values())) for k, v in ratios.items()})


# ---- b. the reduction ------------------------------------------------------------------------------------------------------
REDUCTION_LISTS = [(0, 0), (1, 0), (0, 1), (64, 63), (127, 0), (0, 127), (64, 64), (128, 0), (0, 128), (65, 64), (129, 0), (0, 129), (128, 129)]


def test_reduction_against_the_exact_sum(ctx, kat):
    one = np.flatnonzero(kat["fam"] == kat["families"].index("one_pose"))
    lines, planes = one[kat["kind"][one] == 0], one[kat["kind"][one] == 1]
    x, T = kat["x"][one[0]], kat["T_bl"][kat["tbl"][one[0]]]
    worst = 0.0
    for nl, npl in REDUCTION_LISTS:
        sel = np.concatenate([lines[:nl], planes[:npl]]).astype(int)
        ctx.factors_upload(0, 0, kat["rec"][lines[:nl]] if nl else NONE)
        ctx.factors_upload(0, 1, kat["rec"][planes[:npl]] if npl else NONE)
        Hm, g, c = ctx.linearize(0, x, T, w_tan=0.0, huber=HUBER)
        got = np.concatenate([[Hm[a, b] for a, b in K.TRI], g, [c]])
        if len(sel) == 0:
            assert (got == 0).all()
            continue
        terms = np.concatenate([kat["H"][sel], kat["g"][sel], kat["cost"][sel, None]], 1)
        units = np.concatenate([kat["u_H"][sel] * np.where(K.TT, K.BOUNDS["c_htt"], np.where(K.RR, K.BOUNDS["c_hrr"], K.BOUNDS["c_htr"])),
                                kat["u_g"][sel] * np.repeat([K.BOUNDS["c_gt"], K.BOUNDS["c_gr"]], 3), kat["u_c"][sel, None] * K.BOUNDS["c_c"]], 1)
        want = np.array([math.fsum(t) for t in terms.T])
        unit = K.EPS * max(1.0, math.log2(len(sel))) * np.abs(terms).sum(0) + units.sum(0)
        ratio = np.abs(got - want) / unit
        print("reduction %3d lines + %3d planes: worst |sum - exact| / unit %.3f" % (nl, npl, ratio.max()))
        worst = max(worst, ratio.max())
        assert np.isfinite(got).all() and ratio.max() <= 1.0, (nl, npl, ratio)
    print("reduction worst", worst)


# ---- c. the three solve kernels ---------------------------------------------------------------------------------------------
def rotation(phi):
    from scipy.spatial.transform import Rotation as Rsc
    return Rsc.from_rotvec(phi).as_matrix() if np.any(phi) else np.eye(3)


def moved(kat, i, phi):
    """item i (identity extrinsic) moved rigidly so that it sits at the pose x = [0, phi] as it sat at its own"""
    x, rec = kat["x"][i], kat["rec"][i].copy()
    G = rotation(phi) @ rotation(x[3:]).T
    mv = lambda v: G @ (v - x[:3])
    if kat["kind"][i] == 0:
        rec[3:6], rec[6:9] = np.float32(mv(rec[3:6])), np.float32(mv(rec[6:9]))
    else:
        rec[3:6], rec[6:9] = mv(rec[3:6]), np.float32(G @ rec[6:9])
    return rec


def distance(rec, kind, x0):
    """of the record's point from its line / plane at the pose x0 (identity extrinsic), in doubles"""
    P = rotation(x0[3:]) @ rec[:3] + x0[:3]
    if kind == 0:
        return np.linalg.norm(np.cross(P - rec[3:6], P - rec[6:9])) / np.linalg.norm(rec[3:6] - rec[6:9])
    return np.linalg.norm(P - rec[3:6])


def solve_cases(kat):
    """-> [(lines, planes, x0)].  Slots 0, 1, 2 begin with the exact-zero families (poses with no rotation), moved by their own
    translation alone: under the slot's start rotation of 2e-9, 0 and 3e-7 rad and no translation they lie about 1e-9 m from,
    exactly on, and about 1e-6 m from their lines and planes -- distances the float ends of a rotated line cannot keep."""
    names = kat["families"]
    ident = kat["tbl"] == 0                                      # (w_tan is the call's, not the record's: every plane item serves)
    fam = lambda *ns: np.flatnonzero(ident & np.isin(kat["fam"], [names.index(n) for n in ns]))
    generic = fam("line_generic", "plane_generic", "line_seg_0.2", "line_seg_10", "plane_axis", *[n for n in names if n.startswith("theta_")])
    edge = fam("line_near_1e-3", "line_near_1e-6", "line_near_1e-9", "plane_near_1e-3", "plane_near_1e-6", "plane_near_1e-9", "gate",
               "huber_near_below", "huber_near_above", "huber_10x", "line_small_range", "plane_small_range")
    on = fam("line_on", "plane_on")
    assert len(on) == 24 and kat["zero"][on].sum() == 12 and (kat["kind"][edge] == 0).sum() > 40 and (kat["kind"][edge] == 1).sum() > 40
    starts = [(np.array([1e-9, -2e-9, 5e-10]), 0.0), (np.array([0.0, 0.0, 0.0]), 0.0), (np.array([3e-7, 1e-7, -2e-7]), 0.0),
              (np.array([2.0, -1.0, 2.0]), 1.0), (np.array([4e-5, -8e-5, 1e-5]), 1.0), (np.array([-1.0, 2.0, 2.0]), 1.0)]
    cases = []
    for k, ((phi, kick), n_plane, n_line) in enumerate(zip(starts, (127, 128, 129, 1535, 1536, 1537), (40, 24, 129, 5, 128, 1))):
        x0 = np.concatenate([kick * np.array([0.02, -0.01, 0.015]), phi])         # (the start rotation is the family's angle itself)
        rest = np.concatenate([edge, generic])
        recs = {0: [], 1: []}
        if k < 3:
            for i in on:
                recs[kat["kind"][i]].append(moved(kat, i, np.zeros(3)))
        for kind, n in ((0, n_line), (1, n_plane)):
            pool = rest[kat["kind"][rest] == kind]
            assert len(recs[kind]) <= n
            recs[kind] += [moved(kat, i, phi) for i in np.resize(pool, n - len(recs[kind]))]
        lines, planes = (np.stack(recs[q]) if recs[q] else NONE for q in (0, 1))
        if k < 3:                                                # what the slot's first evaluation meets, kernel by kernel
            for kind, part in ((0, lines[:12]), (1, planes[:12])):
                d = np.array([distance(r, kind, x0) for r in part])
                lo, hi = ((1e-10, 1e-7), (0.0, 0.0), (1e-8, 1e-5))[k]
                assert len(d) == 12 and (d >= lo).all() and (d <= hi).all() and (k == 1 or (d < hi / 5).any()), (k, kind, d)
        cases.append((lines, planes, x0))
    return cases


def test_three_solve_kernels_agree_on_the_edge_families(M, kat):
    cases = solve_cases(kat)
    B = 320                                                      # more slots than the device has CUs: k_solve<false>
    out = {}
    before = os.environ.pop("MML_SOLVE_WIDE", None)              # the default context: the variable unset
    for wide in ("1", "0"):
        try:
            if wide == "0":
                os.environ["MML_SOLVE_WIDE"] = "0"
            c = M.Context(max_scans=B if wide == "1" else len(cases), max_features=1600)
        finally:
            os.environ.pop("MML_SOLVE_WIDE", None)
            if wide == "0" and before is not None:
                os.environ["MML_SOLVE_WIDE"] = before
        try:
            for s in range(B if wide == "1" else len(cases)):
                lines, planes, _ = cases[s % len(cases)]
                c.factors_upload(s, 0, lines)
                c.factors_upload(s, 1, planes)
            x0 = np.stack([cases[s % len(cases)][2] for s in range(B)])
            key = lambda q: (q.iterations, q.successful, q.termination, q.initial_cost, q.final_cost)
            for huber, fixed in ((HUBER, True), (HUBER, False), (0.0, False)):
                alone = [c.solve(s, 1, x0[s:s + 1], np.eye(4), max_iters=10, fixed=fixed, huber=huber, trace=True) for s in range(len(cases))]
                out[wide, huber, fixed] = [(x[0], key(q[0]), t[0][:q[0].iterations]) for x, q, t in alone]
                if wide == "1":
                    xb, sb, tb = c.solve(0, B, x0, np.eye(4), max_iters=10, fixed=fixed, huber=huber, trace=True)
                    out["batch", huber, fixed] = [(xb[s], key(sb[s]), tb[s][:sb[s].iterations]) for s in range(B)]
        finally:
            c.close()
    for huber, fixed in ((HUBER, True), (HUBER, False), (0.0, False)):
        w, p, b = out["1", huber, fixed], out["0", huber, fixed], out["batch", huber, fixed]
        for s in range(B):
            xa, ka, ta = w[s % len(cases)]
            assert np.isfinite(xa).all() and np.isfinite(ta).all() and np.isfinite(ka[3:]).all(), (s, huber, fixed)
            for who, (xo, ko, to) in (("k_solve<true>", p[s % len(cases)]), ("k_solve<false>", b[s])):
                assert np.array_equal(xa, xo) and ka == ko and np.array_equal(ta, to), (who, s, huber, fixed, xa - xo, ka, ko)
        print("huber %g fixed %d: iterations %s, |x - start| %s" % (huber, fixed, [k[0] for _, k, _ in w],
                                                                  ["%.2g" % np.abs(x - cs[2]).max() for (x, _, _), cs in zip(w, cases)]))
