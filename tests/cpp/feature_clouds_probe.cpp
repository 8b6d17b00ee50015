// feature_clouds_probe.cpp -- the adapter's side of tests/test_feature_clouds_gpu.py: scans in, union_cloud messages out.
// in:  int n, float far_th, then per scan: int n_velo, n_velo x 4 floats, int n_livox, n_livox x 20-byte CustomPoint records
// out: per message 6 cloud sizes, 4 counters, the six clouds' records -- first the n messages of ONE unionCloudMessage over
//      the slots 0 .. n-1, then scan 0's Velodyne part through getVeloFeature(normal, corner, surf) and its Livox part through
//      getHoriFeatureExtract(cloud, corner, surf), each written as a message whose other sensor is empty.
#include <cstdio>
#include <vector>

#include "mmloam_adapter.hpp"

static void put(FILE* f, const mml::UnionFeatureClouds& m) {
    const mml::PointCloud* c[6] = {&m.velo_corner, &m.velo_surface, &m.velo_combine, &m.livox_corner, &m.livox_surface, &m.livox_combine};
    int head[10];
    for (int k = 0; k < 6; ++k) head[k] = (int)c[k]->size();
    head[6] = m.velo_corner_num, head[7] = m.velo_surf_num, head[8] = m.livox_corner_num, head[9] = m.livox_surf_num;
    fwrite(head, sizeof(int), 10, f);
    for (int k = 0; k < 6; ++k)
        if (!c[k]->empty()) fwrite(c[k]->data(), sizeof(mml::PointXYZINormal), c[k]->size(), f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int n = 0;
    float far_th = 0;
    if (fread(&n, 4, 1, in) != 1 || fread(&far_th, 4, 1, in) != 1 || n < 1) return 2;
    std::vector<std::vector<float>> velo(n);
    std::vector<std::vector<mml_livox_point>> livox(n);
    for (int i = 0; i < n; ++i) {
        int nv = 0, nl = 0;
        if (fread(&nv, 4, 1, in) != 1) return 2;
        velo[i].resize(4 * (size_t)nv);
        if (nv && fread(velo[i].data(), 16, nv, in) != (size_t)nv) return 2;
        if (fread(&nl, 4, 1, in) != 1) return 2;
        livox[i].resize(nl);
        if (nl && fread(livox[i].data(), sizeof(mml_livox_point), nl, in) != (size_t)nl) return 2;
    }
    fclose(in);
    try {
        mml_config cfg;
        mml_config_default(&cfg, n + 2);
        cfg.far_th = far_th;
        mml::Context ctx(n + 2, 0, &cfg);
        mml::feature_extraction fe(ctx);
        for (int i = 0; i < n; ++i)
            mml::check(ctx.get(), mml_scan_upload(ctx.get(), i, velo[i].data(), (int)velo[i].size() / 4, livox[i].data(), (int)livox[i].size()),
                       "scan_upload");
        mml::check(ctx.get(), mml_extract(ctx.get(), 0, n, nullptr), "extract");
        std::vector<mml::UnionFeatureClouds> msgs;
        fe.unionCloudMessage(0, n, msgs);
        FILE* out = fopen(argv[2], "wb");
        if (!out) return 2;
        for (const auto& m : msgs) put(out, m);
        mml_scan_info info;
        mml::UnionFeatureClouds a, b;
        fe.getVeloFeature(velo[0].data(), (int)velo[0].size() / 4, a.velo_combine, a.velo_corner, a.velo_surface, info, n);
        a.velo_corner_num = info.velo_corner_num, a.velo_surf_num = info.velo_surf_num;
        put(out, a);
        fe.getHoriFeatureExtract(livox[0].data(), (int)livox[0].size(), b.livox_combine, b.livox_corner, b.livox_surface, info, n + 1);
        b.livox_corner_num = info.livox_corner_num, b.livox_surf_num = info.livox_surf_num;
        put(out, b);
        fclose(out);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("FEATURE_CLOUDS_PROBE_DONE\n");
    return 0;
}
