// Replays csrc/time_offset_gate.h on the host, stand-alone (tests/test_time_offset_gate.py builds it with
// -fsanitize=address,undefined, so the header is compiled by the plain host compiler).
// stdin:  the number of cases, then per case "n_velo hori_stamp n_hori_msgs" and n_velo stamps (unsigned decimal nanoseconds).
// stdout: per case "rc selected status".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "time_offset_gate.h"

int main() {
    int cases = 0;
    if (std::scanf("%d", &cases) != 1 || cases < 0) return 2;
    for (int c = 0; c < cases; ++c) {
        int n_velo = 0, n_msgs = 0;
        uint64_t hori = 0;
        if (std::scanf("%d %" SCNu64 " %d", &n_velo, &hori, &n_msgs) != 3 || n_velo < 0) return 2;
        std::vector<uint64_t> stamps((size_t)n_velo);  // exactly as large as the data: a read past either end is a sanitizer report
        for (uint64_t& v : stamps)
            if (std::scanf("%" SCNu64, &v) != 1) return 2;
        int selected = -7, status = -7;
        const int rc = time_offset_gate(n_velo, n_velo ? stamps.data() : nullptr, hori, n_msgs, &selected, &status);
        std::printf("%d %d %d\n", rc, selected, status);
    }
    return 0;
}
