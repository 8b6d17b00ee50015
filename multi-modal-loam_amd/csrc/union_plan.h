// union_plan.h -- the frame recurrence of the aligner's pub_horipoints_given_stamp (unionLidarsAligner.cpp:766-868), shared by
// the host (mml_union_plan) and the device (k_union_plan, livox_stream.hip): the pattern of imu_preint.h and marg_dense.h.
// At the end of the file: the same for the one-stamp overload (:872-1009), mml_union_plan_offset and k_union_plan_offset.
//
// The stream is a queue of points with 64-bit stamps S[i] (nanoseconds after hs, the first message's time base), indexed
// ABSOLUTELY: i counts every point ever pushed, q is the queue's front, tail one past its last point.  The reference compares
// absolute times, hs + S[i], with the frame's stamps (:777, :794, :837), and so does this file: in unsigned 64-bit arithmetic
// hs + S[i] is the point's own time (time base + offset_time) even for a message that is older than hs.
//
// On a time-ordered stream (hs + S[i] never decreases) the two walks of the reference are lower bounds:
//   lbs = first i in [q0, tail) with hs + S[i] >= start, else tail          (q0: any front at or before q)
//   lbe = the same for end
// and one frame follows from (q, tail, lbs, lbe) alone -- no stamp is read again:
//   :769-773  q == tail                                   EMPTY
//   :789      hs + S[q] >= start  <=>  lbs <= q           no walk: b = q, the gate is point q's stamp
//   :789-800  otherwise the walk ends ONE PAST its first match j = lbs: b = j + 1, the gate is S[j]; no match (lbs == tail, which
//             is also what a one-point queue gives): NOT_REACHED
//   :811      the gate decides whether point b goes out, not b's own stamp: gate >= end  <=>  lbe <= max(q, lbs).  Then, or when
//             b == tail, the loop emits nothing and :842 reads front() of an empty vector: NO_POINTS (defined here)
//   :811-838  b goes out, then k = b + 1 ... while k < tail and hs + S[k] < end: e = max(b + 1, lbe)   (the read of S[tail] at :837
//             after the last point is defined here as the end of the loop)
//   :862-863  the queue drops its first (e - q) - 100 points: q' = max(q, e - 100) (a negative count erases nothing, defined here)
//   more than max_livox_points points: OVERFLOW -- the slot gets none, n_livox reports e - b, the queue advances as for OK
// Rows of frames that emit nothing: begin = end = b where b exists (NO_POINTS), else q; n_livox = 0; front_after = q.
#ifndef MML_UNION_PLAN_H
#define MML_UNION_PLAN_H

#include <stdint.h>

#include "mmloam_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MML_UNION_HD __host__ __device__
#else
#define MML_UNION_HD
#endif

enum { MML_UNION_OK = 0, MML_UNION_EMPTY = 1, MML_UNION_NOT_REACHED = 2, MML_UNION_NO_POINTS = 3, MML_UNION_OVERFLOW = 4 };
#define MML_UNION_KEEP 100  // points the reference leaves in front of a frame's end (:862)

// First i in [lo, hi) with hs + S[i] >= t (unsigned, as the reference adds them), else hi.  `S` is indexed by i - origin.
MML_UNION_HD inline long mml_union_lower_bound(const uint64_t* S, long origin, long lo, long hi, uint64_t hs, uint64_t t) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (hs + S[mid - origin] < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One frame; returns the front the next frame starts from.
MML_UNION_HD inline long mml_union_resolve(long q, long tail, long lbs, long lbe, int max_livox_points, mml_union_frame* f) {
    f->n_livox = 0;
    f->begin = f->end = q;
    f->front_after = q;
    if (q == tail) {
        f->status = MML_UNION_EMPTY;
        return q;
    }
    long b = q, gate = q;  // gate: the point whose stamp decides whether b goes out
    if (lbs > q) {
        if (lbs >= tail) {
            f->status = MML_UNION_NOT_REACHED;
            return q;
        }
        gate = lbs;
        b = lbs + 1;
    }
    if (b == tail || lbe <= gate) {
        f->status = MML_UNION_NO_POINTS;
        f->begin = f->end = b;
        return q;
    }
    const long e = lbe > b + 1 ? lbe : b + 1;
    const long after = e - MML_UNION_KEEP > q ? e - MML_UNION_KEEP : q;
    const long n = e - b;
    f->begin = b;
    f->end = e;
    f->front_after = after;
    f->n_livox = n > 2147483647L ? 2147483647 : (int)n;
    f->status = n > (long)max_livox_points ? MML_UNION_OVERFLOW : MML_UNION_OK;
    return after;
}

// The ONE-STAMP overload of pub_horipoints_given_stamp (:872-1009), which the aligner runs once the time offset is known
// (:513-551): a fixed count of points from the first one at or after t.  With lb the lower bound of t over [q0, tail) for any
// front q0 at or before q, the first live point at or after t is L = max(q, lb) (the stream is time-ordered), and:
//   :874-878  q == tail                                   EMPTY, the front stays
//   :896-918  the walk erases front points while hs + S[front] < t and more than one point is queued: the front becomes L; with
//             no point at or after t (L == tail) it stops at the last point and returns false: NOT_REACHED, and the queue HAS
//             changed, front = tail - 1
//   :946-980  n = min(sliced, tail - L) points go out and all of them are erased: front = L + n (no keep-100 here)
// Every front() the overload reads (:912, :984) has an element, so nothing needs a definition: there is no NO_POINTS and, as
// the caller refuses sliced > max_livox_points up front, no OVERFLOW.  Rows that emit nothing: begin = end = front_after.
MML_UNION_HD inline long mml_union_resolve_offset(long q, long tail, long lb, int sliced, mml_union_frame* f) {
    f->n_livox = 0;
    f->begin = f->end = q;
    f->front_after = q;
    if (q == tail) {
        f->status = MML_UNION_EMPTY;
        return q;
    }
    const long L = lb > q ? lb : q;
    if (L >= tail) {
        f->status = MML_UNION_NOT_REACHED;
        f->begin = f->end = f->front_after = tail - 1;
        return tail - 1;
    }
    const long n = tail - L < (long)sliced ? tail - L : (long)sliced;
    f->status = MML_UNION_OK;
    f->begin = L;
    f->end = f->front_after = L + n;
    f->n_livox = (int)n;
    return L + n;
}

#endif
