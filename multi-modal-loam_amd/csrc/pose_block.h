// pose_block.h -- the parameter block of a pose call (mml_step, mml_estimate): the part of d_pose_in that one call, or one
// lane's piece of a call, owns, and where its four arrays lie in it.  d_pose_in gives every slot kPoseSlotDoubles doubles, so the
// ranges of disjoint slot ranges are disjoint.  The pinned twin that is filled on the host has the same layout at another base.
// No HIP: a host program can include it (tests/cpp/pose_block_check.cpp).
#ifndef MML_POSE_BLOCK_H
#define MML_POSE_BLOCK_H

#include <stddef.h>

constexpr int kPoseSlotDoubles = 64;
constexpr int kPackMaxSlots = 16;
// The packed form of a pose call: its start poses go to k_solve inside the block and everything read back comes up as one
// result record per slot, so one copy each way.  k_solve takes both only from a launch of at most one problem per CU.
inline bool mml_pose_packed(int count, int cus) { return count <= kPackMaxSlots && count <= cus; }

struct PoseBlock {
    int first = 0, count = 0;  // the slots
    double* base = nullptr;    // of the slots' range in d_pose_in, or of the pinned twin
    // und: sweep motion dR | dt, 12 per slot.  T_wl: association pose, 16 per slot.  x: start pose, 6 per slot.  T_bl: 16, once.
    // (mml_estimate has no sweep motions: the field keeps its place and the copy starts behind it)
    static constexpr size_t kUnd = 12, kTwl = 16, kX = 6, kTbl = 16;
    // n (kUnd + kTwl + kX) + kTbl <= n (kUnd + kTwl + kX + kTbl) for every n >= 1
    static_assert(kUnd + kTwl + kX + kTbl <= kPoseSlotDoubles, "a block of any count fits its slots' range of d_pose_in");
    size_t o_und() const { return 0; }
    size_t o_Twl() const { return o_und() + kUnd * (size_t)count; }
    size_t o_x() const { return o_Twl() + kTwl * (size_t)count; }
    size_t o_Tbl() const { return o_x() + kX * (size_t)count; }
    size_t size() const { return o_Tbl() + kTbl; }  // in doubles
    double* und() const { return base + o_und(); }
    double* T_wl() const { return base + o_Twl(); }
    double* x() const { return base + o_x(); }
    double* T_bl() const { return base + o_Tbl(); }

    static PoseBlock of(double* d_pose_in, int first, int count) { return {first, count, d_pose_in + kPoseSlotDoubles * (size_t)first}; }
    PoseBlock at(double* other_base) const { return {first, count, other_base}; }
    // piece p of this call cut into pieces of `chunk` slots (mml_step's lanes); count <= 0 behind the last one
    PoseBlock piece(int p, int chunk) const {
        const int f = first + p * chunk, left = first + count - f;
        return {f, left < chunk ? left : chunk, base + kPoseSlotDoubles * (size_t)(f - first)};
    }
};

#endif
