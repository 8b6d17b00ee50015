"""mml_union_plan (csrc/union_plan.h on the host: two lower bounds per frame and an integer recurrence) against the yardstick
tests/union_ref.py (the reference's walks over list-backed queues, unionLidarsAligner.cpp:736-868).  Every field of every row
must be equal.  No device is needed; what the device does with the same header is tests/test_gpu_union.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import union_cases as UC  # noqa: E402
import union_ref as UR  # noqa: E402

N_RANDOM = 2400


def plan_rows(M, msgs, bounds, maxl, split=None):
    """The rows of mml_union_plan for the whole stream pushed first; split: in two calls, the second starting from the front the
    first one left (what mml_union_assemble's caller does from call to call)."""
    hs, S = UC.stamps_of(msgs)
    if split is None or split <= 0 or split >= len(bounds) - 1:
        rc, rows = M.union_plan(S, 0, len(S), hs, bounds, maxl)
        assert rc == M.MML_OK
        return rows
    rc, a = M.union_plan(S, 0, len(S), hs, bounds[:split + 1], maxl)
    assert rc == M.MML_OK
    rc, b = M.union_plan(S, int(a[-1]["front_after"]), len(S), hs, bounds[split:], maxl)
    assert rc == M.MML_OK
    return np.concatenate([a, b])


def assert_rows_equal(got, want, what):
    assert got.dtype == want.dtype == M_FRAME
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), "%s: %s differs\n got %s\nwant %s" % (what, name, got, want)


M_FRAME = UR.FRAME_DTYPE


@pytest.mark.parametrize("name", sorted(UC.fixed_cases()))
def test_fixed_case(M, name):
    msgs, bounds, maxl, expected = UC.fixed_cases()[name]
    assert M.UNION_FRAME_DTYPE == UR.FRAME_DTYPE
    want, _ = UR.replay(msgs, bounds, maxl)
    # the yardstick itself gives what the case was built to give (worked out by hand from the reference's lines)
    assert [(int(r["status"]), int(r["begin"]), int(r["end"])) for r in want] == expected, (name, want)
    assert_rows_equal(plan_rows(M, msgs, bounds, maxl), want, name)
    for split in range(1, len(bounds) - 1):
        assert_rows_equal(plan_rows(M, msgs, bounds, maxl, split), want, "%s split at %d" % (name, split))


def test_fixed_cases_are_what_they_claim():
    """The properties the cases are named after, checked on the inputs themselves."""
    c = UC.fixed_cases()
    _, S = UC.stamps_of(c["stamps_above_2_32"][0])
    assert UC.HS != 0 and int(S.max()) > 2 ** 32
    msgs, bounds, maxl, _ = c["offset_truncated"]
    hs, S = UC.stamps_of(msgs)
    rows, pts = UR.replay(msgs, bounds, maxl)
    full = hs + S.astype(object) - bounds[0]
    assert max(full) > 2 ** 32 and np.array_equal(pts[0]["offset_time"], np.array([v % 2 ** 32 for v in full], np.uint32))
    assert np.all(pts[0]["_pad"] == 0) and np.all(msgs[0][1]["_pad"] != 0)
    rows, _ = UR.replay(*c["erase_below_and_above_100"][:3])
    assert [int(v) for v in rows["front_after"]] == [0, 100, 140]


def test_random_cases(M):
    rng = np.random.default_rng(20261018)
    cases = [UC.random_case(rng) for _ in range(N_RANDOM)]
    wants = [UR.replay(*c)[0] for c in cases]
    status = np.concatenate([w["status"] for w in wants])
    share = np.bincount(status, minlength=5) / len(status)
    print("frames %d, share per status OK/EMPTY/NOT_REACHED/NO_POINTS/OVERFLOW: %s" % (len(status), np.round(share, 3)))
    # the generator reaches every branch: no status is silently left out of the comparison below
    for s in (UR.OK, UR.EMPTY, UR.NOT_REACHED, UR.NO_POINTS):
        assert share[s] >= 0.05, (s, share)
    assert np.count_nonzero(status == UR.OVERFLOW) >= 1
    assert any(np.any(w["front_after"] > 0) for w in wants)   # (and the queue is erased in some)
    for k, (c, want) in enumerate(zip(cases, wants)):
        msgs, bounds, maxl = c
        assert_rows_equal(plan_rows(M, msgs, bounds, maxl), want, "case %d" % k)
        assert_rows_equal(plan_rows(M, msgs, bounds, maxl, split=(k % (len(bounds) - 1))), want, "case %d split" % k)


def test_refusals(M):
    S = np.array([0, 10, 20, 15, 30], np.uint64)
    ok = [UC.HS, UC.HS + 10]
    assert M.union_plan(S, 0, 5, UC.HS, ok, 256)[0] == M.MML_ERR_STATE          # 15 after 20
    assert M.union_plan(S, 0, 3, UC.HS, ok, 256)[0] == M.MML_OK                 # (outside [front, tail): not read)
    assert M.union_plan(S, 3, 5, UC.HS, ok, 256)[0] == M.MML_OK
    assert M.union_plan(S, 0, 3, UC.HS, [UC.HS + 10, UC.HS], 256)[0] == M.MML_ERR_INVALID
    assert M.union_plan(S, 2, 1, UC.HS, ok, 256)[0] == M.MML_ERR_INVALID
    assert M.union_plan(S, 0, 3, UC.HS, [UC.HS], 256)[0] == M.MML_ERR_INVALID   # count = 0
