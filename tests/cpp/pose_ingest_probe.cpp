// pose_ingest_probe.cpp -- the adapter's side of tests/test_gpu_pose_ingest.py: union_cloud messages in, rows and digests out.
// in:  int n, first_slot, max_scans, max_velo_points, max_livox_points, has_rows; mml_pose_ingest_opts; then per message six
//      counts and the six clouds' 48-byte records; then (has_rows) n mml_imu_interval rows
// out: n mml_pose_ingest_row of ONE Estimator::IngestUnionClouds call, then the ten mml_slot_digest words of the n slots
#include <cstdio>
#include <vector>

#include "mmloam_adapter.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int head[6];
    mml_pose_ingest_opts opts;
    if (fread(head, sizeof(int), 6, in) != 6 || fread(&opts, sizeof(opts), 1, in) != 1) return 2;
    const int n = head[0], first_slot = head[1];
    if (n < 1) return 2;
    std::vector<mml::UnionFeatureClouds> msgs(n);
    for (auto& m : msgs) {
        int np[6];
        if (fread(np, sizeof(int), 6, in) != 6) return 2;
        mml::PointCloud* c[6] = {&m.velo_corner, &m.velo_surface, &m.velo_combine, &m.livox_corner, &m.livox_surface, &m.livox_combine};
        for (int k = 0; k < 6; ++k) {
            c[k]->resize(np[k]);
            if (np[k] && fread(c[k]->data(), sizeof(mml::PointXYZINormal), np[k], in) != (size_t)np[k]) return 2;
        }
        m.livox_corner_num = np[3];
    }
    std::vector<mml_imu_interval> rows(head[5] ? n : 0);
    if (head[5] && fread(rows.data(), sizeof(mml_imu_interval), n, in) != (size_t)n) return 2;
    fclose(in);
    try {
        mml_config cfg;
        mml_config_default(&cfg, head[2]);
        cfg.max_velo_points = head[3];
        cfg.max_livox_points = head[4];
        mml::Context ctx(head[2], 0, &cfg);
        mml::Estimator est(ctx, cfg.leaf_corner, cfg.leaf_surf);
        const std::vector<mml_pose_ingest_row> out = est.IngestUnionClouds(first_slot, msgs, head[5] ? rows.data() : nullptr, opts);
        if ((int)out.size() != n) return 3;
        std::vector<uint64_t> dg(MML_DIGEST_WORDS * (size_t)n);
        mml::check(ctx.get(), mml_slot_digest(ctx.get(), first_slot, n, dg.data()), "mml_slot_digest");
        FILE* f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(out.data(), sizeof(mml_pose_ingest_row), n, f);
        fwrite(dg.data(), sizeof(uint64_t), dg.size(), f);
        fclose(f);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("POSE_INGEST_PROBE_DONE\n");
    return 0;
}
