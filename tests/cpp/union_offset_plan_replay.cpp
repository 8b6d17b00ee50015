// Stand-alone replay of the one-stamp recurrence of csrc/union_plan.h on the host (tests/test_union_offset_adapter.py builds it
// with -fsanitize=address,undefined): reads cases from stdin and prints the frame rows.  One case:
//   hs front tail sliced_points count
//   S[0] .. S[tail-1]
//   starts[0] .. starts[count-1]
// Output per frame: status n_livox begin end front_after.  The stamp array is allocated at exactly tail entries and the starts at
// exactly count, so a read past either would be reported.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "union_plan.h"

int main() {
    uint64_t hs;
    long front, tail;
    int sliced, count;
    while (std::scanf("%" SCNu64 " %ld %ld %d %d", &hs, &front, &tail, &sliced, &count) == 5) {
        if (front < 0 || tail < front || count < 1 || sliced < 1) return 2;
        std::vector<uint64_t> S((size_t)tail), starts((size_t)count);
        for (auto& v : S)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        for (auto& v : starts)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        long q = front;
        for (int i = 0; i < count; ++i) {
            mml_union_frame f;
            q = mml_union_resolve_offset(q, tail, mml_union_lower_bound(S.data(), 0, front, tail, hs, starts[(size_t)i]), sliced, &f);
            std::printf("%d %d %ld %ld %ld\n", f.status, f.n_livox, f.begin, f.end, f.front_after);
        }
    }
    return 0;
}
