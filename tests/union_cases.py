"""Inputs of the union-frame tests (test_union_plan.py, test_gpu_union.py): Livox messages, frame boundaries, and the stamps
S = (timebase - hs) + offset_time as the header defines them (computed here with numpy, for mml_union_plan's argument; the
yardstick tests/union_ref.py computes its own)."""
import numpy as np

from union_ref import LIVOX_DTYPE

HS = 1_600_000_000_000_000_123   # a 2020 ROS time in ns: far above 2^32, not a round number
M64 = (1 << 64) - 1


def message(timebase, offsets, seed=0):
    """(timebase, points): the given offset_times, coordinates and bytes that identify the point, _pad set to garbage on purpose
    (roscpp leaves it unset; the assembled record must carry 0)."""
    offsets = np.asarray(offsets, np.uint64)
    n = len(offsets)
    rng = np.random.default_rng(seed * 7919 + n)
    p = np.zeros(n, LIVOX_DTYPE)
    p["offset_time"] = offsets.astype(np.uint32)
    p["x"] = rng.uniform(1, 40, n).astype(np.float32)
    p["y"] = rng.uniform(-20, 20, n).astype(np.float32)
    p["z"] = rng.uniform(-3, 6, n).astype(np.float32)
    p["reflectivity"] = rng.integers(0, 256, n)
    p["tag"] = rng.integers(0, 256, n)
    p["line"] = rng.integers(0, 6, n)
    p["_pad"] = 0xA5
    return int(timebase), p


def stamps_of(msgs):
    """(hs, S uint64[n]) for the messages pushed in order into an empty stream."""
    if not msgs:
        return 0, np.zeros(0, np.uint64)
    hs = msgs[0][0]
    S = [((tb - hs) & M64) + int(o) & M64 for tb, p in msgs for o in p["offset_time"]]
    return hs, np.array(S, dtype=np.uint64)


def to_wire(points):
    """The serialised CustomPoint array: 19 bytes per point (the 20-byte struct without _pad)."""
    raw = np.ascontiguousarray(points).view(np.uint8).reshape(-1, 20)
    return np.ascontiguousarray(raw[:, :19]).reshape(-1)


def fixed_cases():
    """name -> (msgs, frame boundaries, max_livox_points, expected (status, begin, end) per frame, worked out by hand from
    unionLidarsAligner.cpp:766-868)."""
    OK, EMPTY, NOT_REACHED, NO_POINTS, OVERFLOW = 0, 1, 2, 3, 4
    h = HS
    c = {}
    # a stamp equal to `start` ends the walk (>=) and is the skipped point j; a stamp equal to `end` is not emitted (<)
    c["stamp_equal_start_and_end"] = ([message(h, [0, 10, 20, 30, 40])], [h + 10, h + 30], 256, [(OK, 2, 3)])
    # runs of equal stamps on both boundaries: the walk stops at the FIRST 10, the emission at the FIRST 20
    c["equal_runs_straddle"] = ([message(h, [0, 10, 10, 10, 20, 20, 20, 30])], [h + 10, h + 20], 256, [(OK, 2, 4)])
    # S[q] >= start on entry: no walk, nothing skipped
    c["front_already_inside"] = ([message(h, [50, 60, 70])], [h + 40, h + 65], 256, [(OK, 0, 2)])
    # the walk skips its first match: point 1 (stamp 10) lies in [5, 100) and is not emitted
    c["skipped_point_j"] = ([message(h, [0, 10, 20, 30])], [h + 5, h + 100], 256, [(OK, 2, 4)])
    # the gate (S[j] = 100) is at or after `end`: nothing emitted; second frame: the same without a walk (S[q] = 0 >= start, >= end)
    c["gate_after_end"] = ([message(h, [0, 100, 200])], [h + 10, h + 50], 256, [(NO_POINTS, 2, 2)])
    c["gate_after_end_no_walk"] = ([message(h + 7, [0, 100, 200])], [h, h + 7], 256, [(NO_POINTS, 0, 0)])
    # a one-point queue: behind the frame it cannot be walked (:791 size() > 1); inside it is emitted; at `end` it is not
    c["one_point_not_reached"] = ([message(h, [10])], [h + 20, h + 30], 256, [(NOT_REACHED, 0, 0)])
    c["one_point_emitted"] = ([message(h, [10])], [h + 5, h + 30], 256, [(OK, 0, 1)])
    c["one_point_at_end"] = ([message(h, [10])], [h + 5, h + 10], 256, [(NO_POINTS, 0, 0)])
    # the match is the last point: begin == tail, nothing to emit
    c["match_is_last_point"] = ([message(h, [0, 10, 20])], [h + 15, h + 90], 256, [(NO_POINTS, 3, 3)])
    # `end` beyond the tail: the loop ends at the last point
    c["end_beyond_tail"] = ([message(h, 10 * np.arange(10))], [h, h + 10 ** 6], 256, [(OK, 0, 10)])
    # e - q = 50 < 100: nothing erased; then e - q = 200 > 100: front 100; then from a front that is not 0
    c["erase_below_and_above_100"] = ([message(h, 10 * np.arange(250))], [h, h + 500, h + 2000, h + 2400], 256,
                                      [(OK, 0, 50), (OK, 51, 200), (OK, 201, 240)])
    # failing frames followed by good ones: NO_POINTS, then OK; OVERFLOW (5 points, room for 3), then OK
    c["no_points_then_good"] = ([message(h, 100 + 10 * np.arange(8))], [h, h + 50, h + 130, h + 400], 256,
                                [(NO_POINTS, 0, 0), (OK, 0, 3), (OK, 4, 8)])
    c["overflow_then_good"] = ([message(h, 10 * np.arange(12))], [h, h + 50, h + 90, h + 200], 3,
                               [(OVERFLOW, 0, 5), (OK, 6, 9), (OK, 10, 12)])
    # an empty stream
    c["empty"] = ([], [h, h + 10, h + 20], 256, [(EMPTY, 0, 0), (EMPTY, 0, 0)])
    # stamps above 2^32 ns (the second message starts 5 s after the first) with the non-zero hs
    c["stamps_above_2_32"] = ([message(h, [0, 10]), message(h + 5 * 10 ** 9, [0, 10, 20, 30])],
                              [h + 5 * 10 ** 9 - 5, h + 5 * 10 ** 9 + 25], 256, [(OK, 3, 5)])
    # S[k] - s above 2^32: the frame spans the 5 s, the offset_time of the late points is truncated to 32 bits
    c["offset_truncated"] = ([message(h, [0, 10]), message(h + 5 * 10 ** 9, [0, 10, 20, 30])], [h, h + 6 * 10 ** 9], 256, [(OK, 0, 6)])
    # a message older than hs cannot be in order (its points lie before the ones already there): see the GPU refusal test
    return c


def random_case(rng):
    """(msgs, boundaries, max_livox_points): 0 or about 50-600 time-ordered points in 1-4 messages, 1-12 frames whose boundaries lie
    from before the first point to after the last, some on point stamps, some repeated."""
    msgs = []
    if rng.random() >= 0.10:
        total = int(rng.integers(50, 601))
        n_msgs = int(rng.integers(1, 5))
        cuts = np.sort(rng.integers(1, total, n_msgs - 1)) if n_msgs > 1 else np.zeros(0, int)
        sizes = np.diff(np.concatenate([[0], cuts, [total]]))
        t = HS + int(rng.integers(0, 10 ** 6))
        for m, n in enumerate(sizes):
            if n == 0:
                continue
            span = int(rng.choice([n // 4 + 1, 40 * n, 10 ** 8]))   # many equal stamps | dense | a 100 ms message
            offs = np.sort(rng.integers(0, span + 1, n))
            msgs.append(message(t, offs, seed=m))
            t = t + int(offs[-1]) + int(rng.choice([0, 1, 1000, 5 * 10 ** 9]))
    count = int(rng.integers(1, 13))
    if msgs:
        hs, S = stamps_of(msgs)
        lo, hi = hs + int(S[0]), hs + int(S[-1])
    else:
        hs, S, lo, hi = HS, np.zeros(0, np.uint64), HS, HS + 1000
    width = hi - lo + 10
    b = lo - width // 4 + (rng.random(count + 1) * (width * 3 // 2)).astype(np.int64)
    if len(S):
        on = rng.random(count + 1) < 0.25
        b[on] = hs + S[rng.integers(0, len(S), int(on.sum()))].astype(np.int64)
    rep = rng.random(count + 1) < 0.15
    b[1:][rep[1:]] = b[:-1][rep[1:]]
    bounds = [int(v) for v in np.sort(b)]
    return msgs, bounds, int(rng.choice([8, 40, 256, 1000]))
