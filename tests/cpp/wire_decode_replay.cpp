// Replays csrc/wire_decode.h on the host, stand-alone (tests/test_wire_batch_host.py builds it with -fsanitize=address,undefined,
// so the header is compiled by the plain host compiler and every byte it reads is checked).
// argv[1]: a case file -- int32 number of cases, then per case
//   int32 count, point_step, off_x, off_y, off_z, off_intensity, livox_record_bytes, max_velo_points, max_livox_points;
//   int64 velo_bytes, livox_bytes; int64 velo_at[count]; int32 n_velo[count]; int64 livox_at[count]; int32 n_livox[count];
//   velo_bytes bytes; livox_bytes bytes.
// stdout: per case "rc bad_frame span0 span1 span2 span3" and, with rc 0, one line of the Velodyne words (4 a point) and one of
// the Livox words (5 a point), hexadecimal.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "wire_decode.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
    return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t cases = 0;
    if (fread(&cases, 4, 1, f) != 1 || cases < 0) return 2;
    for (int c = 0; c < cases; ++c) {
        int32_t h[9];
        int64_t len[2];
        if (fread(h, 4, 9, f) != 9 || fread(len, 8, 2, f) != 2 || h[0] < 0 || len[0] < 0 || len[1] < 0) return 2;
        const size_t n = (size_t)h[0];
        std::vector<int64_t> vat(n), lat(n);
        std::vector<int32_t> nv(n), nl(n);
        if (!rd(f, vat) || !rd(f, nv) || !rd(f, lat) || !rd(f, nl)) return 2;
        std::vector<uint8_t> vd((size_t)len[0]), ld((size_t)len[1]);  // exactly as large as the data: a read past either end is a sanitizer report
        if (!rd(f, vd) || !rd(f, ld)) return 2;
        const WireCall call{h[0], vat.data(), nv.data(), h[1], h[2], h[3], h[4], h[5], lat.data(), nl.data(), h[6]};
        int64_t span[4] = {0, 0, 0, 0};
        int bad = -7;
        char msg[192];
        const int rc = wire_plan(call, h[7], h[8], span, &bad, msg, sizeof(msg));
        std::printf("%d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", rc, bad, span[0], span[1], span[2], span[3]);
        if (rc != MML_OK) continue;
        if (span[1] > (int64_t)vd.size() || span[3] > (int64_t)ld.size()) return 3;  // (the case file is wrong, not the header)
        size_t tv = 0, tl = 0;
        for (size_t i = 0; i < n; ++i) tv += nv[i], tl += nl[i];
        std::vector<uint32_t> vo(4 * tv), lo(5 * tl);
        wire_decode_host(call, vd.data(), ld.data(), vo.data(), lo.data());
        for (uint32_t w : vo) std::printf("%08x ", w);
        std::printf("\n");
        for (uint32_t w : lo) std::printf("%08x ", w);
        std::printf("\n");
    }
    fclose(f);
    return 0;
}
