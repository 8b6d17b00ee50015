"""The inputs the IMU queue tests share: one 200 Hz message stream at epoch-scale stamps (sec + 1e-9 * nsec, where the dt
subtractions are hardest) with two pairs of equal stamps, and the edge intervals over it, each named after what it is for."""
import numpy as np

SEC = 1600000000
N_MSGS = 700
DUP_A, DUP_B = 10, 40          # T[10] == T[11], T[40] == T[41]


def stream(n=N_MSGS, seed=20261020):
    """(n, 7) messages: stamp, gyro xyz, accel xyz (in g).  200 Hz with +-0.2 ms of jitter; message DUP + 1 repeats DUP's stamp."""
    rng = np.random.default_rng(seed)
    nsec = np.arange(n, dtype=np.int64) * 5000000 + rng.integers(-200000, 200001, n)
    if n > DUP_B + 1:
        nsec[DUP_A + 1] = nsec[DUP_A]
        nsec[DUP_B + 1] = nsec[DUP_B]
    sec, nsec = SEC + nsec // 1000000000, nsec % 1000000000
    m = np.zeros((n, 7))
    m[:, 0] = [float(s) + 1e-9 * float(ns) for s, ns in zip(sec, nsec)]    # ros::Time::toSec
    m[:, 1:4] = rng.normal(0.0, 0.3, (n, 3))
    m[:, 4:7] = rng.normal(0.0, 0.2, (n, 3)) + [0.0, 0.0, 1.0]
    assert np.all(np.diff(m[:, 0]) >= 0)
    return m


def mid(T, i):
    """A time strictly between T[i] and T[i + 1]."""
    t = 0.5 * (T[i] + T[i + 1])
    assert T[i] < t < T[i + 1]
    return t


def edge_intervals(T):
    """[(name, start, end, expected status, expected n, expected interpolated)] over the stamps of stream()."""
    last = len(T) - 1
    c = [
        ("one_message_at_end", mid(T, 19), T[20], 0, 1, 0),
        ("one_inside_plus_interpolation", mid(T, 19), mid(T, 20), 0, 2, 1),
        ("nothing_inside", T[20] + 0.001, T[20] + 0.002, 5, 0, 0),
        ("end_equals_start_between", T[20] + 0.001, T[20] + 0.001, 5, 0, 0),
        ("end_equals_start_on_a_stamp", T[20], T[20], 5, 0, 0),
        ("end_equals_start_on_the_last_stamp", T[last], T[last], 5, 0, 0),
        ("start_equals_a_stamp", T[30], mid(T, 33), 0, 4, 1),                  # message 30 is out: 31, 32, 33 + synthesised
        ("end_equals_a_stamp", mid(T, 29), T[35], 0, 6, 0),
        ("equal_stamps_straddle_start", T[DUP_A], mid(T, 13), 0, 3, 1),        # 10 and 11 are out: 12, 13 + synthesised
        ("equal_stamps_straddle_end", mid(T, 37), T[DUP_B], 0, 3, 0),          # 38, 39, 40; 41 (the same stamp) is not reached
        ("end_equals_the_last_stamp", mid(T, last - 4), T[last], 0, 4, 0),
        ("end_one_ulp_past_the_last_stamp", mid(T, last - 4), np.nextafter(T[last], np.inf), 2, 0, 0),
        ("end_equals_the_first_stamp", T[0] - 1.0, T[0], 3, 0, 0),
        ("end_before_the_first_stamp", T[0] - 1.0, T[0] - 0.5, 3, 0, 0),
        ("end_before_start", T[50], T[45], 4, 0, 0),
        ("start_before_the_first_stamp", T[0] - 1.0, mid(T, 2), 0, 4, 1),
    ]
    for L in (1, 63, 64, 65, 130):      # the write kernel's lane stride
        c.append(("rows_%d_exact" % L, mid(T, 99), T[100 + L - 1], 0, L, 0))
        if L > 1:
            c.append(("rows_%d_interpolated" % L, mid(T, 99), mid(T, 100 + L - 2), 0, L, 1))
    return c


def consecutive(n, t0=SEC + 0.2525, step=0.1):
    """n consecutive intervals of `step` seconds: t_start[i] = t_end[i - 1].  The boundaries lie mid-way between two 200 Hz ticks,
    farther from both than the jitter, so every 0.1 s interval holds 20 messages and the synthesised one."""
    t = np.array([t0 + step * k for k in range(n + 1)])
    return t[:-1].copy(), t[1:].copy()


def biases(n, seed=7):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.01, (n, 3)), rng.normal(0, 0.05, (n, 3))
