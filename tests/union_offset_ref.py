"""The yardstick of the aligner's time-offset mode: a literal Python transcription of the ONE-STAMP overload
pub_horipoints_given_stamp(start_stamp, msg) (unionLidarsAligner.cpp:872-1009), which velo_cloud_handler calls at :520 once
the time offset is known, on the list-backed queues of tests/union_ref.py -- statement by statement, with the reference's line
numbers.  It really erases from the lists, shares no code with csrc/union_plan.h and knows nothing of lower bounds.

uint64 arithmetic is spelled out with & M64; ros::Time().fromNSec(t).toNSec() (:955/:964) is the identity for every t below
2^32 seconds, which is all the callers produce.  Nothing in this overload is undefined: the front() reads at :912 and :984 always
have an element (the walk erases only while more than one point is queued; at least one point is emitted).  The statements that
only build messages nobody reads (livox_interpolate_msg :898-908, the pcl cloud :970-974, the publishers) are left out; the erase
of _velo_queue at :1005 concerns the caller's Velodyne queue, which is not modelled.

Rows: (status, n_livox, begin, end, front_after) with absolute point indices, as tests/union_ref.py has them.  A frame that
emits nothing has begin = end = front_after = the front it leaves: the walk may have erased points before it gave up (:916).
"""
import numpy as np

from union_ref import FRAME_DTYPE, LIVOX_DTYPE, Aligner

M64 = (1 << 64) - 1
OK, EMPTY, NOT_REACHED = 0, 1, 2


class OffsetAligner(Aligner):
    """union_ref.Aligner (queues, transform_hori_timestamp, the interval overload) plus the one-stamp overload."""

    def pub_horipoints_given_stamp_1(self, start_stamp, offset_search_sliced_points):
        """Returns (row, points): points the LIVOX_DTYPE array livox_aligned_msg.points holds at :993."""
        none = np.zeros(0, LIVOX_DTYPE)
        if len(self._hori_points_stamp_queue) == 0:                               # :874
            q = self.erased
            return (EMPTY, 0, q, q, q), none                                      # :877
        hs = self._hori_start_stamp
        hori_pts_front_stamp = (hs + self._hori_points_stamp_queue[0]) & M64      # :881
        while hori_pts_front_stamp < start_stamp:                                 # :896
            if len(self._hori_points_queue) > 1:                                  # :897
                del self._hori_points_queue[0]                                    # :910
                del self._hori_points_stamp_queue[0]                              # :911
                self.erased += 1
                hori_pts_front_stamp = (hs + self._hori_points_stamp_queue[0]) & M64  # :912
            else:
                q = self.erased
                return (NOT_REACHED, 0, q, q, q), none                            # :916
        begin = self.erased
        points_num = -1                                                           # :946
        if offset_search_sliced_points < len(self._hori_points_queue):            # :947
            points_num = offset_search_sliced_points                              # :948
        else:
            points_num = len(self._hori_points_queue)                             # :950
        out = []
        for i in range(points_num):                                               # :952
            stamp = (self._hori_points_stamp_queue[0] + hs - start_stamp) & M64   # :955
            src = self._hori_points_queue[0]
            offset_time = stamp & 0xFFFFFFFF                                      # :964 (uint32 = uint64)
            out.append((offset_time, src[1], src[2], src[3], src[4], src[5], src[6], 0))  # :960-968
            del self._hori_points_queue[0]                                        # :977
            del self._hori_points_stamp_queue[0]                                  # :978
            self.erased += 1
        return (OK, len(out), begin, self.erased, self.erased), np.array(out, dtype=LIVOX_DTYPE)  # :1008


def replay(msgs, starts, sliced_points):
    """All messages pushed, then one frame per start stamp, one after the other.  (rows FRAME_DTYPE, list of points)."""
    a = OffsetAligner()
    a.transform_hori_timestamp(msgs)
    rows, pts = [], []
    for t in starts:
        r, p = a.pub_horipoints_given_stamp_1(int(t), sliced_points)
        rows.append(r)
        pts.append(p)
    return np.array(rows, dtype=FRAME_DTYPE), pts
