"""The yardstick of the aligner frame assembly: a literal Python transcription of the reference's
transform_hori_timestamp (unionLidarsAligner.cpp:736-763) and pub_horipoints_given_stamp (:766-868) on list-backed
queues, statement by statement, with the reference's line numbers.  It shares no code with csrc/union_plan.h: it walks
the queues as the reference does and knows nothing of lower bounds.

uint64 arithmetic is spelled out with & M64.  ros::Time().fromNSec(t).toNSec() (:756, :814/:823) is the identity for every
t below 2^32 seconds, which is all the callers produce.

Where the reference is undefined, the definitions of include/mmloam_hip.h (mml_union_assemble) are used, each marked
DEFINED below:
  * :837 reads the stamp one past the last point after emitting it: the loop ends there;
  * :842 reads front() of an empty vector when nothing was emitted: status NO_POINTS, nothing published, nothing erased;
  * :862-863 erase a negative count when idx < 100: nothing is erased;
  * more than max_livox_points points (no such limit in the reference): OVERFLOW, no points for the slot, the needed count
    reported, the queue erased as for OK.
Rows: (status, n_livox, begin, end, front_after) with absolute point indices (counted over everything ever pushed);
frames that emit nothing have begin = end = the index the emission would have started at where the walk got that far
(NO_POINTS), else the front.
"""
import numpy as np

M64 = (1 << 64) - 1
OK, EMPTY, NOT_REACHED, NO_POINTS, OVERFLOW = 0, 1, 2, 3, 4

LIVOX_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                        ("reflectivity", "u1"), ("tag", "u1"), ("line", "u1"), ("_pad", "u1")])
FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_livox", "<i4"), ("begin", "<i8"), ("end", "<i8"), ("front_after", "<i8")])


class Aligner:
    def __init__(self):
        self._first_hori = True
        self._hori_start_stamp = 0
        self._hori_points_queue = []        # CustomPoint as (offset_time, x, y, z, reflectivity, tag, line)
        self._hori_points_stamp_queue = []  # uint64
        self.erased = 0                     # bookkeeping of this transcription: points erased so far = absolute index of the front

    def transform_hori_timestamp(self, hori_msg_vec):
        """hori_msg_vec: list of (timebase, points) with points a LIVOX_DTYPE array."""
        for timebase, points in hori_msg_vec:
            if self._first_hori:                                              # :203
                self._hori_start_stamp = int(timebase)                        # :204
                self._first_hori = False                                      # :206
        for timebase, points in hori_msg_vec:                                 # :749
            delta_t = (int(timebase) - self._hori_start_stamp) & M64          # :751
            for j in range(len(points)):                                      # :754
                p = points[j]
                stamp = (delta_t + int(p["offset_time"])) & M64               # :756
                self._hori_points_stamp_queue.append(stamp)                   # :758
                self._hori_points_queue.append((int(p["offset_time"]), p["x"], p["y"], p["z"], int(p["reflectivity"]),
                                                int(p["tag"]), int(p["line"])))  # :759

    def pub_horipoints_given_stamp(self, velo_start_stamp, velo_end_stamp, max_livox_points):
        """Returns (row, points): row as documented above, points the LIVOX_DTYPE array the slot receives."""
        none = np.zeros(0, LIVOX_DTYPE)
        q = self.erased
        if len(self._hori_points_stamp_queue) == 0:                           # :769
            return (EMPTY, 0, q, q, q), none                                  # :772
        hs = self._hori_start_stamp
        hori_pts_front_stamp = (hs + self._hori_points_stamp_queue[0]) & M64  # :777
        idx = 0                                                               # :787
        while hori_pts_front_stamp < velo_start_stamp:                        # :789
            if len(self._hori_points_queue) > 1 and idx < len(self._hori_points_stamp_queue):  # :791
                hori_pts_front_stamp = (hs + self._hori_points_stamp_queue[idx]) & M64         # :794
                idx += 1                                                      # :795
            else:
                return (NOT_REACHED, 0, q, q, q), none                        # :798
        begin = idx
        out = []
        while hori_pts_front_stamp < velo_end_stamp and idx < len(self._hori_points_queue):   # :811
            stamp = (self._hori_points_stamp_queue[idx] + hs - velo_start_stamp) & M64         # :814
            src = self._hori_points_queue[idx]
            offset_time = stamp & 0xFFFFFFFF                                  # :823 (uint32 = uint64)
            out.append((offset_time, src[1], src[2], src[3], src[4], src[5], src[6], 0))       # :819-827
            idx += 1                                                          # :835
            if idx == len(self._hori_points_stamp_queue):                     # DEFINED: :837 would read one past the last stamp
                break
            hori_pts_front_stamp = (hs + self._hori_points_stamp_queue[idx]) & M64             # :837
        if len(out) == 0:                                                     # DEFINED: :842 front() of an empty vector
            return (NO_POINTS, 0, q + begin, q + begin, q), none
        n_erase = idx - 100                                                   # :862
        if n_erase > 0:                                                       # DEFINED: a negative count erases nothing
            del self._hori_points_queue[:n_erase]                             # :862
            del self._hori_points_stamp_queue[:n_erase]                       # :863
            self.erased += n_erase
        row_tail = (q + begin, q + idx, self.erased)
        if len(out) > max_livox_points:                                       # DEFINED: the slot's capacity
            return (OVERFLOW, len(out)) + row_tail, none
        return (OK, len(out)) + row_tail, np.array(out, dtype=LIVOX_DTYPE)    # :866


def replay(msgs, stamps, max_livox_points):
    """All messages pushed, then frames [stamps[i], stamps[i+1]) one after the other.  (rows FRAME_DTYPE, list of points)."""
    a = Aligner()
    a.transform_hori_timestamp(msgs)
    rows, pts = [], []
    for i in range(len(stamps) - 1):
        r, p = a.pub_horipoints_given_stamp(int(stamps[i]), int(stamps[i + 1]), max_livox_points)
        rows.append(r)
        pts.append(p)
    return np.array(rows, dtype=FRAME_DTYPE), pts


def transform_velo(xyzi, tf):
    """pcl::transformPointCloud as csrc/time_offset.hip's k_tofs_tf states it: float32, t0 * x + t1 * y + t2 * z + t3 summed
    left to right, every product and sum rounded to float32; the intensity carried; tf None: a copy."""
    v = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    if tf is None:
        return v.copy()
    t = np.asarray(tf, np.float32).reshape(16)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    o = v.copy()
    for r in range(3):
        o[:, r] = ((t[4 * r] * x + t[4 * r + 1] * y).astype(np.float32) + t[4 * r + 2] * z).astype(np.float32) + t[4 * r + 3]
    return o
