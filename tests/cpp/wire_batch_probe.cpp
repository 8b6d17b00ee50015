// wire_batch_probe.cpp -- the adapter's side of tests/test_gpu_wire_batch.py: union_cloud messages in wire form in, digests out.
// in:  int32 count, first_slot, max_scans, max_velo_points, max_livox_points, point_step, off_x, off_y, off_z, off_intensity,
//      livox_record_bytes; int64 velo_bytes, livox_bytes; int64 velo_at[count]; int32 n_velo[count]; int64 livox_at[count];
//      int32 n_livox[count]; the two buffers
// out: the mml_scan_info counters' n_points of the count slots (int32), then the ten mml_slot_digest words of each, after ONE
//      feature_extraction::unionCloudWire call
#include <cstdio>
#include <vector>

#include "mmloam_adapter.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
    return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t h[11];
    int64_t len[2];
    if (fread(h, 4, 11, in) != 11 || fread(len, 8, 2, in) != 2 || h[0] < 1 || len[0] < 0 || len[1] < 0) return 2;
    const int n = h[0], first_slot = h[1];
    std::vector<int64_t> vat(n), lat(n);
    std::vector<int32_t> nv(n), nl(n);
    std::vector<uint8_t> vd((size_t)len[0]), ld((size_t)len[1]);
    if (!rd(in, vat) || !rd(in, nv) || !rd(in, lat) || !rd(in, nl) || !rd(in, vd) || !rd(in, ld)) return 2;
    fclose(in);
    try {
        mml_config cfg;
        mml_config_default(&cfg, h[2]);
        cfg.max_velo_points = h[3];
        cfg.max_livox_points = h[4];
        mml::Context ctx(h[2], 0, &cfg);
        mml::feature_extraction fe(ctx);
        std::vector<mml_scan_info> infos;
        fe.unionCloudWire(first_slot, n, vd.empty() ? nullptr : vd.data(), vat.data(), nv.data(), h[5], h[6], h[7], h[8], h[9],
                          ld.empty() ? nullptr : ld.data(), lat.data(), nl.data(), h[10], nullptr, &infos);
        if ((int)infos.size() != n) return 3;
        std::vector<int32_t> np(n);
        for (int i = 0; i < n; ++i) np[i] = infos[i].n_points;
        std::vector<uint64_t> dg(MML_DIGEST_WORDS * (size_t)n);
        mml::check(ctx.get(), mml_slot_digest(ctx.get(), first_slot, n, dg.data()), "mml_slot_digest");
        FILE* f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(np.data(), sizeof(int32_t), n, f);
        fwrite(dg.data(), sizeof(uint64_t), dg.size(), f);
        fclose(f);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("WIRE_BATCH_PROBE_DONE\n");
    return 0;
}
