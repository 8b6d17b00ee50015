// Stand-alone replay of csrc/union_plan.h on the host (tests/test_union_adapter.py builds it with -fsanitize=address,undefined):
// reads cases from stdin and prints the frame rows.  One case:
//   hs front tail max_livox_points count
//   S[0] .. S[tail-1]
//   stamps[0] .. stamps[count]
// Output per frame: status n_livox begin end front_after.  The stamp array is allocated at exactly tail entries, so a read one
// past the last point -- the reference's own out-of-bounds read at unionLidarsAligner.cpp:837 -- would be reported.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "union_plan.h"

int main() {
    uint64_t hs;
    long front, tail;
    int maxl, count;
    while (std::scanf("%" SCNu64 " %ld %ld %d %d", &hs, &front, &tail, &maxl, &count) == 5) {
        if (front < 0 || tail < front || count < 1) return 2;
        std::vector<uint64_t> S((size_t)tail), stamps((size_t)count + 1);
        for (auto& v : S)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        for (auto& v : stamps)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        long q = front;
        long lbs = mml_union_lower_bound(S.data(), 0, front, tail, hs, stamps[0]);
        for (int i = 0; i < count; ++i) {
            const long lbe = mml_union_lower_bound(S.data(), 0, front, tail, hs, stamps[(size_t)i + 1]);
            mml_union_frame f;
            q = mml_union_resolve(q, tail, lbs, lbe, maxl, &f);
            std::printf("%d %d %ld %ld %ld\n", f.status, f.n_livox, f.begin, f.end, f.front_after);
            lbs = lbe;
        }
    }
    return 0;
}
