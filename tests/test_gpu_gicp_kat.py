"""GPU suite: the device's GICP pieces (csrc/gicp.hip) through the test hook mml_debug_gicp -- the kernels and __device__ functions
the alignments run -- against the exact references of tests/golden/gicp_kat.npz, with the checks and the BOUNDS of
tests/gicp_checks.py (8 x the oracle's worst ratios, tests/test_gicp_kat.py; never the device's).
  EVAL    gicp_eval in one workgroup of BF_THREADS: f and the gradient at eleven states over correspondence lists of 4 .. 1537 entries
          either side of the 512-term chunks, with and without holes; lane 0's copy and the last lane's are bit-identical
  QUAD / INTERP / STATE   solve_quadratic, interpolate, apply_state and the state recovery, one lane per item
  ROUND   one launch of k_gicp_bfgs: properties against the exact objective (rational arithmetic on the returned float matrix)
  COV     k_gicp_cov: the neighbour ids against the exact 20-NN (random clouds at the block and tile seams, a lattice of true ties, exact
          duplicates, a cloud 60 m out), the covariances of 20-point patches against I - (1 - 1e-3) u0 u0'
  CORR    k_gicp_corr: the exact 1-NN under a float T, the gate (either side, and d == gate^2 rejected), M against the exact inverse
  batch independence and the hook's refusals
For the record (not a bound), the device's worst ratios on the MI355X: f 0.021, g_t 0.045, g_r 0.017, quad 0.995, interp 0.127,
state_R 0.465, state_x 0.226, round_f 0.005, cov 0.037, maha 0.993 -- the oracle's own figures to the digits shown; the rounds took the oracle's 72, 91 and
74 evaluations.
"""
import numpy as np
import pytest

import gicp_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kat():
    return K.load()


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def impl(M, ctx):
    def ev(src, tgt, corr, maha, xs, gated):
        f, g = ctx.debug_gicp(M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=corr, maha=maha, x=xs, gate2=4.0 if gated else 0.0)
        assert np.array_equal(f[:, 0], f[:, 1]) and np.array_equal(g[:, 0], g[:, 1]), "lane 0 and the last lane hold different values"
        f0, _ = ctx.debug_gicp(M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=corr, maha=maha, x=xs[:2], gate2=4.0 if gated else 0.0, grad=False)
        assert np.array_equal(f0[:, 0], f[:2, 0]) and np.array_equal(f0[:, 0], f0[:, 1])      # the value-only pass: the same f
        return f[:, 0], g[:, 0]
    return dict(neigh=lambda p: ctx.debug_gicp(M.GICP_DBG_COV, tgt=p)[1], cov=lambda p: ctx.debug_gicp(M.GICP_DBG_COV, tgt=p)[0],
                corr=lambda s, t, c1, c2, T, g2: ctx.debug_gicp(M.GICP_DBG_CORR, src=s, tgt=t, cov_src=c1, cov_tgt=c2, T=T, gate2=g2),
                eval=ev, quad=lambda a: ctx.debug_gicp(M.GICP_DBG_QUAD, x=a), interp=lambda a: ctx.debug_gicp(M.GICP_DBG_INTERP, x=a),
                state=lambda x: ctx.debug_gicp(M.GICP_DBG_STATE, x=x),
                round=lambda s, t, c, m, T, g2, mi, te: ctx.debug_gicp(M.GICP_DBG_ROUND, src=s, tgt=t, corr=c, maha=m, T=T, gate2=g2,
                                                                       max_iterations=mi, transformation_epsilon=te))


def test_device_objective_against_exact(kat, impl):
    K.check_bounds("device", K.eval_ratios(kat, impl, "device"))


def test_device_line_search_pieces_against_exact(kat, impl):
    r = K.quad_ratios(kat, impl, "device")
    r.update(K.interp_ratios(kat, impl, "device"))
    K.check_bounds("device", r)


def test_device_state_against_exact(kat, impl):
    K.check_bounds("device", K.state_ratios(kat, impl, "device"))


def test_device_round_properties(kat, impl, O):
    K.check_bounds("device", K.round_checks(kat, impl, O, "device"))


def test_device_neighbours_covariances_correspondences_against_exact(kat, impl):
    """MML_GICP_DBG_COV / _CORR: the discrete decisions (neighbour sets, tie order, correspondences, d == gate^2 rejected) are
    asserted inside; the covariances and Mahalanobis matrices against the same BOUNDS as the oracle"""
    K.nn_checks(kat, impl, "device")
    r = K.cov_ratios(kat, impl, "device")
    r.update(K.corr_ratios(kat, impl, "device"))
    K.check_bounds("device", r)


def test_batch_independence(M, ctx):
    """the same cloud pair at positions 0 and 2 of a three-problem call, between two different problems: identical bits"""
    from test_gpu_gicp_batch import key, pair
    a, b, c = pair(7, 300, 513), pair(8, 1025, 257), pair(9, 40, 64)
    r1 = ctx.gicp_align_batch([a, b, a])
    r2 = ctx.gicp_align_batch([c, a, b])
    assert key(r1[0]) == key(r1[2]) == key(r2[1]) and key(r1[1]) == key(r2[2]) and r1[0][0]


def test_refusals_leave_the_context_usable(M, kat, ctx):
    src, tgt, maha = kat["ev_src"][:8], kat["ev_tgt"][:8], kat["ev_maha"][:8]
    corr = np.arange(8, dtype=np.int32)
    x = K.EVAL_STATES[:1]
    hole, past, below = corr.copy(), corr.copy(), corr.copy()
    hole[3], past[7], below[0] = -1, 8, -2
    calls = [dict(op=M.GICP_DBG_COV, tgt=kat["ev_src"][:19]), dict(op=M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=corr, maha=maha, x=np.zeros((0, 6))),
             dict(op=M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=past, maha=maha, x=x), dict(op=M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=hole, maha=maha, x=x),
             dict(op=M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=below, maha=maha, x=x, gate2=4.0),
             dict(op=M.GICP_DBG_ROUND, src=src, tgt=tgt, corr=past, maha=maha, T=np.eye(4)), dict(op=M.GICP_DBG_QUAD, x=np.zeros((0, 3))),
             dict(op=M.GICP_DBG_EVAL, src=src, tgt=tgt, corr=np.full(8, -1, np.int32), maha=maha, x=x, gate2=4.0), dict(op=7, x=x), dict(op=M.GICP_DBG_CORR, src=src, tgt=tgt, T=np.eye(4))]
    for kw in calls:
        with pytest.raises(M.MmlError) as e:
            ctx.debug_gicp(**kw)
        assert e.value.code == M.MML_ERR_INVALID, kw["op"]
    cnt, roots = ctx.debug_gicp(M.GICP_DBG_QUAD, x=np.array([[1.0, -3.0, 2.0]]))
    assert cnt[0] == 2 and np.array_equal(roots[0], [1.0, 2.0])
