"""mml_time_offset_search_batch without a device: the entry point is declared and exported, the ABI version is unchanged, a NULL
context is refused, the host-only checks of the call (mml_time_offset_plan: offset validation, window counts) are right on plain
arrays, and the Python wrapper turns ragged lists of clouds into the offset form of the C-ABI.  What the call computes is
tests/test_gpu_time_offset_batch.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest


def test_header_declares_and_library_exports_the_entry_points(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    assert re.search(r"\bint\s+mml_time_offset_search_batch\s*\(\s*mml_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,", header)
    assert re.search(r"\bint\s+mml_time_offset_plan\s*\(\s*int\s+n\s*,", header)
    for name in ("mml_time_offset_search_batch", "mml_time_offset_plan", "mml_time_offset_search"):   # the single call stays
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_TOFS_BATCH_MAX\s+%d\b" % M.TOFS_BATCH_MAX, header) and M.TOFS_BATCH_MAX == 65535
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    assert callable(M.Context.time_offset_search_batch) and callable(M.time_offset_pack) and callable(M.time_offset_plan)


def test_null_context_is_refused_and_nothing_is_written(M):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    velo, livox = np.zeros((40, 3), np.float32), np.zeros((60, 3), np.float32)
    vo, lo, wo = np.array([0, 40], np.int32), np.array([0, 60], np.int32), np.array([0, 8], np.int64)
    nn, err = np.full(60, 7.0, np.float32), np.full(8, 7.0)
    nw, best, low = np.full(1, -3, np.int32), np.full(1, -3, np.int32), np.full(1, 7.0)
    rc = M.lib().mml_time_offset_search_batch(None, 1, p(velo), p(vo), None, p(livox), p(lo), 3, 10, p(nn), p(err), p(wo), p(nw), p(best), p(low))
    assert rc == M.MML_ERR_INVALID
    assert np.all(nn == 7.0) and np.all(err == 7.0) and nw[0] == -3 and best[0] == -3 and low[0] == 7.0


def test_window_counts(M):
    """(n_livox - sliced - 1) / res + 1 when n_livox > sliced, else 0 -- against the reference's loop `for cnt = 0; cnt * res +
    sliced < n_livox; ++cnt`, at the sizes around every boundary."""
    cases = [(nl, res, sliced) for res in (1, 2, 30, 997) for sliced in (1, 5, 500) for nl in
             (0, 1, sliced - 1, sliced, sliced + 1, sliced + 2, sliced + res - 1, sliced + res, sliced + res + 1, sliced + 7 * res + 3)]
    for res in (1, 2, 30, 997):
        for sliced in (1, 5, 500):
            sizes = [nl for nl, r, s in cases if r == res and s == sliced and nl >= 0]
            lo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            vo = np.arange(len(sizes) + 1, dtype=np.int32)                   # one Velodyne point each
            rc, bad, nwin = M.time_offset_plan(vo, lo, res, sliced)
            assert rc == M.MML_OK and bad == -1
            for nl, got in zip(sizes, nwin):
                want = 0
                while want * res + sliced < nl:
                    want += 1
                assert got == want, (nl, res, sliced)
    # the reference's defaults on the merged cloud of eight Livox messages
    assert M.time_offset_plan([0, 20000], [0, 190000])[2].tolist() == [(190000 - 12000 - 1) // 30 + 1]


def test_offsets_are_validated_on_the_host(M):
    ok, inv, cap = M.MML_OK, M.MML_ERR_INVALID, M.MML_ERR_CAPACITY
    plan = M.time_offset_plan
    assert plan([0, 5, 5, 9], [0, 100, 100, 120], 30, 50)[:2] == (ok, -1)    # an empty problem in the middle is no refusal
    assert plan([3, 5], [7, 9], 1, 1)[:2] == (ok, -1)                        # offsets need not start at 0
    assert plan([0, 5, 5, 9], [0, 100, 100, 120], 30, 50, max_map_points=5)[:2] == (ok, -1)
    assert plan([-1, 5], [0, 9])[:2] == (inv, 0)                             # negative
    assert plan([0, 5], [-2, 9])[:2] == (inv, 0)
    assert plan([0, 5, 4, 9], [0, 1, 2, 3])[:2] == (inv, 1)                  # decreasing: the problem whose cloud ends before it starts
    assert plan([0, 5, 6, 9], [0, 4, 3, 3])[:2] == (inv, 1)
    assert plan([0, 5, 5, 9], [0, 4, 6, 7])[:2] == (inv, 1)                  # Livox points, no Velodyne point
    assert plan([0, 5, 11, 12], [0, 4, 6, 7], max_map_points=5)[:2] == (cap, 1)
    assert plan([0, 5], [0, 9], 0, 10)[:2] == (inv, -1) and plan([0, 5], [0, 9], 30, 0)[:2] == (inv, -1)
    # n outside 1 .. MML_TOFS_BATCH_MAX, NULL offsets; a refusal leaves n_windows alone
    L, p = M.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    big = np.zeros(M.TOFS_BATCH_MAX + 2, np.int32)
    nwin, bad = np.full(M.TOFS_BATCH_MAX + 1, -9, np.int32), C.c_int(5)
    assert L.mml_time_offset_plan(0, p(big), p(big), 30, 10, -1, p(nwin), C.byref(bad)) == inv and bad.value == -1
    assert L.mml_time_offset_plan(M.TOFS_BATCH_MAX + 1, p(big), p(big), 30, 10, -1, p(nwin), C.byref(bad)) == inv
    assert L.mml_time_offset_plan(1, None, p(big), 30, 10, -1, p(nwin), C.byref(bad)) == inv
    assert L.mml_time_offset_plan(2, p(np.array([0, 5, 4], np.int32)), p(big), 30, 10, -1, p(nwin), None) == inv
    assert np.all(nwin == -9)
    assert L.mml_time_offset_plan(M.TOFS_BATCH_MAX, p(big), p(big), 30, 10, -1, p(nwin), None) == ok and np.all(nwin[:-1] == 0)


def test_ragged_lists_are_packed_into_the_offset_form(M):
    rng = np.random.default_rng(0)
    sizes = [(5, 7), (3, 0), (0, 0), (11, 2)]
    velos = [rng.normal(size=(a, 3)) for a, _ in sizes]
    livoxs = [rng.normal(size=(b, 3)).astype(np.float32) for _, b in sizes]
    velos[0] = velos[0].reshape(-1).tolist()                                 # a flat list is taken as n x 3 too
    velo, vo, livox, lo, tf = M.time_offset_pack(velos, livoxs)
    assert vo.dtype == np.int32 and lo.dtype == np.int32 and velo.dtype == np.float32 and livox.dtype == np.float32 and tf is None
    assert vo.tolist() == [0, 5, 8, 8, 19] and lo.tolist() == [0, 7, 7, 7, 9]
    assert velo.shape == (19, 3) and livox.shape == (9, 3) and velo.flags.c_contiguous and livox.flags.c_contiguous
    for i in range(len(sizes)):
        assert np.array_equal(velo[vo[i]:vo[i + 1]], np.asarray(velos[i], np.float32).reshape(-1, 3)), i
        assert np.array_equal(livox[lo[i]:lo[i + 1]], livoxs[i]), i
    # one matrix for every problem, or one per problem; the caller's array is never aliased
    T1 = np.eye(4)
    T1[1, 3] = -0.5
    tf = M.time_offset_pack(velos, livoxs, T1)[4]
    assert tf.shape == (4, 16) and tf.dtype == np.float32 and all(np.array_equal(tf[i], T1.astype(np.float32).reshape(16)) for i in range(4))
    Tn = rng.normal(size=(4, 4, 4)).astype(np.float32)
    tf = M.time_offset_pack(velos, livoxs, Tn)[4]
    assert np.array_equal(tf, Tn.reshape(4, 16)) and not np.shares_memory(tf, Tn) and tf.flags.c_contiguous
    # nothing at all: empty clouds, offsets of n + 1 zeros; lists of different lengths are refused
    velo, vo, livox, lo, tf = M.time_offset_pack([np.zeros((0, 3))], [np.zeros((0, 3))])
    assert velo.shape == (0, 3) and livox.shape == (0, 3) and vo.tolist() == [0, 0] and lo.tolist() == [0, 0]
    with pytest.raises(ValueError):
        M.time_offset_pack(velos, livoxs[:-1])
