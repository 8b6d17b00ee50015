"""Inputs of the time-offset-mode tests (test_union_offset_plan.py, test_union_offset_adapter.py, test_gpu_union_offset.py):
Livox messages, one start stamp per frame and the point count `c` (sliced_points).  Messages and stamps S are built by
tests/union_cases.py (message, stamps_of)."""
import numpy as np

from union_cases import HS, message

OK, EMPTY, NOT_REACHED = 0, 1, 2


def fixed_cases():
    """name -> (msgs, starts, c, expected (status, begin, end, front_after) per frame, worked out by hand from
    unionLidarsAligner.cpp:872-1009)."""
    h = HS
    c = {}
    c["empty"] = ([], [h, h + 10], 3, [(EMPTY, 0, 0, 0), (EMPTY, 0, 0, 0)])
    # one point: behind t it cannot be erased (:897 size() > 1), the walk gives up and the front stays; at or after t it goes out
    c["one_point_before_t"] = ([message(h, [10])], [h + 20], 3, [(NOT_REACHED, 0, 0, 0)])
    c["one_point_at_t"] = ([message(h, [10])], [h + 10], 3, [(OK, 0, 1, 1)])
    c["one_point_after_t"] = ([message(h, [10])], [h + 5], 3, [(OK, 0, 1, 1)])
    # a run of stamps equal to t: the walk stops at the FIRST of them (<), and the next frame with the same t starts where this ended
    c["ties_at_t"] = ([message(h, [0, 10, 10, 10, 20, 30])], [h + 10, h + 10], 2, [(OK, 1, 3, 3), (OK, 3, 5, 5)])
    # t before the first point: nothing is erased by the walk
    c["t_before_first"] = ([message(h, [50, 60, 70])], [h + 40], 2, [(OK, 0, 2, 2)])
    # t after the last point: the walk erases all but one point and returns false; a second such frame finds that one point
    c["t_after_last_twice"] = ([message(h, [0, 10, 20, 30])], [h + 100, h + 200], 2, [(NOT_REACHED, 3, 3, 3), (NOT_REACHED, 3, 3, 3)])
    # c larger than what is left after the walk: what is left goes out
    c["c_larger_than_left"] = ([message(h, 10 * np.arange(5))], [h + 25], 1000, [(OK, 3, 5, 5)])
    # the frames consume the stream exactly: the next one finds it empty
    c["exact_then_empty"] = ([message(h, 10 * np.arange(6))], [h, h + 30, h + 30], 3, [(OK, 0, 3, 3), (OK, 3, 6, 6), (EMPTY, 6, 6, 6)])
    # the walk and the count from fronts that are not 0; the last frame takes the last point
    c["walk_then_slices"] = ([message(h, 10 * np.arange(20))], [h + 35, h + 35, h + 185], 4, [(OK, 4, 8, 8), (OK, 8, 12, 12), (OK, 19, 20, 20)])
    # hs (the first message's time base) larger than the second message's time base: timebase - hs wraps, hs + S is still the
    # point's own time (absolute times h + 1000, 1010, 1100, 1200)
    c["hs_above_timebase"] = ([message(h, [1000, 1010]), message(h - 500, [1600, 1700])], [h + 1050], 3, [(OK, 2, 4, 4)])
    # A[k] - t above 2^32 (the second message starts 5 s late): offset_time is truncated to 32 bits
    c["offset_truncated"] = ([message(h, [0, 10]), message(h + 5 * 10 ** 9, [0, 10, 20, 30])], [h + 5], 10, [(OK, 1, 6, 6)])
    return c


def random_case(rng):
    """(msgs, starts, c): a time-ordered stream of 0 .. 400 points in 1-3 messages whose stamps grow by 0, 1, 1 000 or 10^6 ns, 1-8
    frames whose starts lie inside the stream (a quarter of them on a point's stamp) -- in half of the cases the last one or two
    past the last stamp -- and c in {1, 3, 20, 1 000}."""
    n = int(rng.choice([0, 1, 3, 8, 40, 400], p=[0.06, 0.06, 0.08, 0.10, 0.35, 0.35]))
    t0 = HS + int(rng.integers(0, 10 ** 6))
    rel = np.cumsum(rng.choice([0, 1, 1000, 10 ** 6], n)).astype(np.int64) if n else np.zeros(0, np.int64)
    msgs = []
    if n:
        n_msgs = int(rng.integers(1, 4))
        cuts = np.unique(np.concatenate([[0], rng.integers(0, n, n_msgs - 1), [n]]))
        for m in range(len(cuts) - 1):
            a, b = int(cuts[m]), int(cuts[m + 1])
            lead = int(rng.integers(0, 1000))   # the message's time base lies this far before its first point
            msgs.append(message(t0 + int(rel[a]) - lead, rel[a:b] - rel[a] + lead, seed=m))
    lo, hi = (t0 + int(rel[0]), t0 + int(rel[-1])) if n else (t0, t0 + 1000)
    count = int(rng.integers(1, 9))
    starts = lo - 2 + (rng.random(count) * (hi - lo + 4)).astype(np.int64)
    if n:
        on = rng.random(count) < 0.25
        starts[on] = t0 + rel[rng.integers(0, n, int(on.sum()))]
    starts = np.sort(starts)
    if rng.random() < 0.5:
        k = min(count, int(rng.integers(1, 3)))
        starts[count - k:] = hi + 1 + np.sort(rng.integers(0, 1000, k))
    return msgs, [int(v) for v in starts], int(rng.choice([1, 3, 20, 1000]))
