"""mml_union_plan_offset (csrc/union_plan.h on the host: one lower bound per frame and the clamp-add recurrence of
mml_union_resolve_offset) against the yardstick tests/union_offset_ref.py (the reference's one-stamp overload walking and erasing
list-backed queues, unionLidarsAligner.cpp:872-1009).  Every field of every row must be equal.  No device is needed; what the
device does with the same header is tests/test_gpu_union_offset.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import union_cases as UC  # noqa: E402
import union_offset_cases as OC  # noqa: E402
import union_offset_ref as OR  # noqa: E402
import union_ref as UR  # noqa: E402

N_RANDOM = 2400


def plan_rows(M, msgs, starts, c, split=None):
    """The rows of mml_union_plan_offset for the whole stream pushed first; split: in two calls, the second starting from the front
    the first one left."""
    hs, S = UC.stamps_of(msgs)
    if split is None or split <= 0 or split >= len(starts):
        rc, rows = M.union_plan_offset(S, 0, len(S), hs, starts, c)
        assert rc == M.MML_OK
        return rows
    rc, a = M.union_plan_offset(S, 0, len(S), hs, starts[:split], c)
    assert rc == M.MML_OK
    rc, b = M.union_plan_offset(S, int(a[-1]["front_after"]), len(S), hs, starts[split:], c)
    assert rc == M.MML_OK
    return np.concatenate([a, b])


def assert_rows_equal(got, want, what):
    assert got.dtype == want.dtype == UR.FRAME_DTYPE
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), "%s: %s differs\n got %s\nwant %s" % (what, name, got, want)


@pytest.mark.parametrize("name", sorted(OC.fixed_cases()))
def test_fixed_case(M, name):
    msgs, starts, c, expected = OC.fixed_cases()[name]
    want, pts = OR.replay(msgs, starts, c)
    # the yardstick itself gives what the case was built to give (worked out by hand from the reference's lines)
    assert [(int(r["status"]), int(r["begin"]), int(r["end"]), int(r["front_after"])) for r in want] == expected, (name, want)
    assert [len(p) for p in pts] == [int(r["n_livox"]) for r in want] == [e[2] - e[1] for e in expected]
    assert_rows_equal(plan_rows(M, msgs, starts, c), want, name)
    for split in range(1, len(starts)):
        assert_rows_equal(plan_rows(M, msgs, starts, c, split), want, "%s split at %d" % (name, split))


def test_fixed_cases_are_what_they_claim():
    """The properties the cases are named after, checked on the inputs and on what the yardstick emits."""
    cases = OC.fixed_cases()
    msgs, starts, c, _ = cases["hs_above_timebase"]
    hs, S = UC.stamps_of(msgs)
    assert hs > msgs[1][0] and [(hs + int(v)) % 2 ** 64 - hs for v in S] == [1000, 1010, 1100, 1200]
    _, pts = OR.replay(msgs, starts, c)
    assert list(pts[0]["offset_time"]) == [50, 150]
    msgs, starts, c, _ = cases["offset_truncated"]
    hs, S = UC.stamps_of(msgs)
    _, pts = OR.replay(msgs, starts, c)
    full = [hs + int(v) - starts[0] for v in S[1:]]
    assert max(full) > 2 ** 32 and list(pts[0]["offset_time"]) == [v % 2 ** 32 for v in full]
    assert np.all(pts[0]["_pad"] == 0) and np.all(msgs[0][1]["_pad"] != 0)
    # the other fields leave as they came
    src = np.concatenate([p for _, p in msgs])[1:6]
    for name in ("x", "y", "z", "reflectivity", "tag", "line"):
        assert np.array_equal(pts[0][name], src[name]), name


def test_random_cases(M):
    rng = np.random.default_rng(20261019)
    cases = [OC.random_case(rng) for _ in range(N_RANDOM)]
    wants = [OR.replay(*c)[0] for c in cases]
    status = np.concatenate([w["status"] for w in wants])
    share = np.bincount(status, minlength=3) / len(status)
    print("frames %d, share per status OK/EMPTY/NOT_REACHED: %s" % (len(status), np.round(share, 3)))
    # the generator reaches every branch in strength: no status is all but left out of the comparison below
    assert len(share) == 3 and share[OR.OK] >= 0.40 and share[OR.EMPTY] >= 0.05 and share[OR.NOT_REACHED] >= 0.05, share
    assert any(w["status"][-1] == OR.NOT_REACHED and w["front_after"][-1] > 0 for w in wants)   # (a walk that drained the queue)
    for k, (c, want) in enumerate(zip(cases, wants)):
        msgs, starts, n = c
        assert_rows_equal(plan_rows(M, msgs, starts, n), want, "case %d" % k)
        assert_rows_equal(plan_rows(M, msgs, starts, n, split=k % len(starts)), want, "case %d split" % k)


def test_refusals(M):
    S = np.array([0, 10, 20, 15, 30], np.uint64)
    ok = [UC.HS, UC.HS + 10]
    assert M.union_plan_offset(S, 0, 5, UC.HS, ok, 3)[0] == M.MML_ERR_STATE          # 15 after 20
    assert M.union_plan_offset(S, 0, 3, UC.HS, ok, 3)[0] == M.MML_OK                 # (outside [front, tail): not read)
    assert M.union_plan_offset(S, 3, 5, UC.HS, ok, 3)[0] == M.MML_OK
    assert M.union_plan_offset(S, 0, 3, UC.HS, [UC.HS + 10, UC.HS], 3)[0] == M.MML_ERR_INVALID   # decreasing starts
    assert M.union_plan_offset(S, 0, 3, UC.HS, [UC.HS, UC.HS], 3)[0] == M.MML_OK                 # (equal starts are fine)
    assert M.union_plan_offset(S, 2, 1, UC.HS, ok, 3)[0] == M.MML_ERR_INVALID
    assert M.union_plan_offset(S, -1, 3, UC.HS, ok, 3)[0] == M.MML_ERR_INVALID
    assert M.union_plan_offset(S, 0, 3, UC.HS, [], 3)[0] == M.MML_ERR_INVALID          # count = 0
    assert M.union_plan_offset(S, 0, 3, UC.HS, ok, 0)[0] == M.MML_ERR_INVALID          # sliced_points = 0
    assert M.union_plan_offset(S, 0, 3, UC.HS, ok, -4)[0] == M.MML_ERR_INVALID
    # NULL pointers, through the C-ABI itself
    L, C = M.lib(), __import__("ctypes")
    st = np.array(ok, np.uint64)
    rows = np.zeros(2, M.UNION_FRAME_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.mml_union_plan_offset(p(S), 0, 3, C.c_uint64(UC.HS), 2, p(st), 3, p(rows)) == M.MML_OK
    assert L.mml_union_plan_offset(None, 0, 3, C.c_uint64(UC.HS), 2, p(st), 3, p(rows)) == M.MML_ERR_INVALID
    assert L.mml_union_plan_offset(p(S), 0, 3, C.c_uint64(UC.HS), 2, None, 3, p(rows)) == M.MML_ERR_INVALID
    assert L.mml_union_plan_offset(p(S), 0, 3, C.c_uint64(UC.HS), 2, p(st), 3, None) == M.MML_ERR_INVALID
    assert L.mml_union_plan_offset(None, 0, 0, C.c_uint64(UC.HS), 2, p(st), 3, p(rows)) == M.MML_OK   # (an empty stream needs no S)
    assert list(rows["status"]) == [OR.EMPTY, OR.EMPTY]


def test_names_exist(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    for name in ("mml_union_assemble_offset", "mml_union_plan_offset"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    assert callable(M.Context.union_assemble_offset) and callable(M.union_plan_offset)
    assert (M.UNION_OK, M.UNION_EMPTY, M.UNION_NOT_REACHED) == (OR.OK, OR.EMPTY, OR.NOT_REACHED) == (0, 1, 2)
    # a NULL context is refused
    assert M.lib().mml_union_assemble_offset(None, None, 0, 1, None, 1, None, None, None, None) == M.MML_ERR_INVALID


def test_interval_plan_rows_are_unchanged(M):
    """mml_union_plan on the fixed cases of union_cases.py: still the rows of its own yardstick."""
    for name, (msgs, bounds, maxl, _) in sorted(UC.fixed_cases().items()):
        hs, S = UC.stamps_of(msgs)
        rc, rows = M.union_plan(S, 0, len(S), hs, bounds, maxl)
        assert rc == M.MML_OK
        assert_rows_equal(rows, UR.replay(msgs, bounds, maxl)[0], name)
