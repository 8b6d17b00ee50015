// The layout of csrc/pose_block.h, the parameter block of mml_step and mml_estimate, checked on the host: built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_pose_block.py and run as a process of its own.  The fields are
// written through the accessors into a buffer of exactly the slots' range, so a field that left it would be reported too.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "pose_block.h"

static int fails = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("line %d: %s\n", __LINE__, #cond);             \
            ++fails;                                              \
        }                                                         \
    } while (0)

struct Span {
    size_t a, b;  // [a, b) in doubles from the call's base
};
static bool disjoint(const Span& p, const Span& q) { return p.b <= q.a || q.b <= p.a; }

static void check_block(int first, int count) {
    std::vector<double> pool(kPoseSlotDoubles * (size_t)(first + count), 0.0);  // d_pose_in up to the end of the block's slots
    const PoseBlock b = PoseBlock::of(pool.data(), first, count);
    const size_t n = (size_t)count;
    CHECK(b.first == first && b.count == count && b.base == pool.data() + kPoseSlotDoubles * (size_t)first);
    const Span f[4] = {{b.o_und(), b.o_und() + PoseBlock::kUnd * n},
                       {b.o_Twl(), b.o_Twl() + PoseBlock::kTwl * n},
                       {b.o_x(), b.o_x() + PoseBlock::kX * n},
                       {b.o_Tbl(), b.o_Tbl() + PoseBlock::kTbl}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) CHECK(disjoint(f[i], f[j]));
    size_t end = 0;
    for (const Span& s : f) end = std::max(end, s.b);
    CHECK(b.size() == f[3].b && b.size() == end);  // the size is the extent of the last field
    CHECK(b.size() <= kPoseSlotDoubles * n);      // inside the slots' range
    CHECK(b.und() == b.base + f[0].a && b.T_wl() == b.base + f[1].a && b.x() == b.base + f[2].a && b.T_bl() == b.base + f[3].a);
    // what a motion, an association pose, a start pose and the extrinsic take per slot (mml_step's arguments, k_solve's reads)
    CHECK(PoseBlock::kUnd == 9 + 3 && PoseBlock::kTwl == 16 && PoseBlock::kX == 6 && PoseBlock::kTbl == 16);
    // every field written whole, each with its own value, then read back: nothing overlaps, nothing leaves the pool (ASan)
    double* p[4] = {b.und(), b.T_wl(), b.x(), b.T_bl()};
    for (int i = 0; i < 4; ++i)
        for (size_t k = 0; k < f[i].b - f[i].a; ++k) p[i][k] = i + 1;
    for (int i = 0; i < 4; ++i)
        for (size_t k = 0; k < f[i].b - f[i].a; ++k) CHECK(p[i][k] == i + 1);
    // the pinned twin: the same layout at another base
    std::vector<double> twin(b.size());
    const PoseBlock h = b.at(twin.data());
    CHECK(h.first == first && h.count == count && h.size() == b.size() && h.base == twin.data());
    CHECK(h.T_bl() + PoseBlock::kTbl == twin.data() + twin.size());
}

// a call cut the way mml_step cuts it: `lanes` pieces of ceil(count / lanes) slots, the last one shorter
static void check_pieces(int first, int count, int lanes) {
    std::vector<double> pool(kPoseSlotDoubles * (size_t)(first + count), 0.0);
    const PoseBlock call = PoseBlock::of(pool.data(), first, count);
    const int chunk = (count + lanes - 1) / lanes;
    std::vector<Span> spans;
    int slots = 0, next = first;
    for (int p = 0; p < lanes; ++p) {
        const PoseBlock b = call.piece(p, chunk);
        if (b.count <= 0) break;
        CHECK(b.first == next && b.count <= chunk);
        next += b.count;
        slots += b.count;
        CHECK(b.base >= call.base && b.base + b.size() <= call.base + kPoseSlotDoubles * (size_t)count);  // inside the call's range
        CHECK(b.base == pool.data() + kPoseSlotDoubles * (size_t)b.first);                              // at its own slots
        spans.push_back({(size_t)(b.base - call.base), (size_t)(b.base - call.base) + b.size()});
        for (size_t k = 0; k < b.size(); ++k) b.base[k] += 1.0;
    }
    CHECK(slots == count && call.piece(lanes, chunk).count <= 0);
    for (size_t i = 0; i < spans.size(); ++i)
        for (size_t j = i + 1; j < spans.size(); ++j) CHECK(disjoint(spans[i], spans[j]));
    for (double v : pool) CHECK(v == 0.0 || v == 1.0);  // no double belongs to two pieces
}

int main() {
    for (int count : {1, 2, 16, 17, 33, 4096}) {
        check_block(0, count);
        check_block(3, count);
    }
    check_pieces(3, 65, 2);  // pieces of 33 and 32 at a first slot that is not 0
    check_pieces(0, 4096, 8);
    check_pieces(0, 64, 8);
    check_pieces(5, 67, 8);  // a last piece of 4 behind seven of 9
    // one predicate for the packed form: at most kPackMaxSlots slots, and at most one problem per CU
    CHECK(kPackMaxSlots == 16);
    CHECK(mml_pose_packed(1, 256) && mml_pose_packed(16, 256) && !mml_pose_packed(17, 256));
    CHECK(mml_pose_packed(8, 8) && !mml_pose_packed(9, 8) && !mml_pose_packed(16, 8));
    if (fails) return 1;
    printf("pose_block_check ok\n");
    return 0;
}
