"""mml_gicp_align_batch / mml_gicp_refresh_batch without a device: the two entry points are declared and exported, the ABI
version is unchanged, a NULL context is refused, and the Python wrappers turn a ragged list of cloud pairs into the offset form
of the C-ABI (checked on the arrays they build).  What the calls compute is tests/test_gpu_gicp_batch.py."""
import ctypes as C
import re
import subprocess

import numpy as np


def test_header_declares_and_library_exports_both_entry_points(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    for name in ("mml_gicp_align_batch", "mml_gicp_refresh_batch"):
        assert re.search(r"\bint\s+%s\s*\(\s*mml_ctx\s*\*\s*ctx\s*,\s*int\s" % name, header), name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    for name in ("mml_gicp_align", "mml_gicp_refresh"):                      # the single calls stay
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_GICP_BATCH_MAX\s+%d\b" % M.GICP_BATCH_MAX, header) and M.GICP_BATCH_MAX == 65535
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    assert callable(M.Context.gicp_align_batch) and callable(M.Context.gicp_refresh_batch)
    assert C.sizeof(M.GicpInfo) == 24                                        # compared as bytes by the GPU tests: no padding


def test_null_context_is_refused_and_nothing_is_written(M):
    L = M.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    src, tgt = np.zeros((40, 3), np.float32), np.zeros((40, 3), np.float32)
    off = np.array([0, 40], np.int32)
    T = np.full((1, 16), 7.0, np.float32)
    conv = np.full(1, -3, np.int32)
    info = (M.GicpInfo * 1)()
    C.memset(info, 0xAB, C.sizeof(info))
    before = bytes(info)
    assert L.mml_gicp_align_batch(None, 1, p(src), p(off), p(tgt), p(off), p(T), p(conv), C.cast(info, C.c_void_p)) == M.MML_ERR_INVALID
    assert np.all(T == 7.0) and conv[0] == -3 and bytes(info) == before
    ref = np.full(1, -3, np.int32)
    assert L.mml_gicp_refresh_batch(None, 0, 1, p(T), 1, 1, p(ref), C.cast(info, C.c_void_p)) == M.MML_ERR_INVALID
    assert np.all(T == 7.0) and ref[0] == -3 and bytes(info) == before


def test_pairs_are_marshalled_into_the_offset_form(M):
    rng = np.random.default_rng(0)
    sizes = [(5, 7), (0, 3), (4, 0), (0, 0), (11, 2)]
    pairs = [(rng.normal(size=(a, 3)), rng.normal(size=(b, 3)).astype(np.float32)) for a, b in sizes]
    pairs[0] = (pairs[0][0].reshape(-1).tolist(), pairs[0][1])               # a flat list is taken as n x 3 too
    src, so, tgt, to, T = M.gicp_pack_pairs(pairs)
    assert so.dtype == np.int32 and to.dtype == np.int32 and src.dtype == np.float32 and tgt.dtype == np.float32 and T.dtype == np.float32
    assert so.tolist() == [0, 5, 5, 9, 9, 20] and to.tolist() == [0, 7, 10, 10, 10, 12]
    assert src.shape == (20, 3) and tgt.shape == (12, 3) and src.flags.c_contiguous and tgt.flags.c_contiguous and T.flags.c_contiguous
    for i, (s, t) in enumerate(pairs):
        assert np.array_equal(src[so[i]:so[i + 1]], np.asarray(s, np.float32).reshape(-1, 3)), i
        assert np.array_equal(tgt[to[i]:to[i + 1]], np.asarray(t, np.float32).reshape(-1, 3)), i
    assert T.shape == (5, 4, 4) and all(np.array_equal(T[i], np.eye(4, dtype=np.float32)) for i in range(5))
    # one initial matrix for every problem, or one per problem; the caller's arrays are never aliased
    T1 = np.eye(4)
    T1[1, 3] = -0.5
    T = M.gicp_pack_pairs(pairs, T1)[4]
    assert T.shape == (5, 4, 4) and all(np.array_equal(T[i], T1.astype(np.float32)) for i in range(5))
    Tn = rng.normal(size=(5, 4, 4)).astype(np.float32)
    T = M.gicp_pack_pairs(pairs, Tn)[4]
    assert np.array_equal(T, Tn) and not np.shares_memory(T, Tn)
    # nothing at all: empty clouds, offsets of n + 1 zeros
    src, so, tgt, to, T = M.gicp_pack_pairs([(np.zeros((0, 3)), np.zeros((0, 3)))])
    assert src.shape == (0, 3) and tgt.shape == (0, 3) and so.tolist() == [0, 0] and to.tolist() == [0, 0] and T.shape == (1, 4, 4)
