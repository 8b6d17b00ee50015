// mmloam_adapter.hpp -- host-side mirror of the reference's C++ surface on top of the C-ABI (include/mmloam_hip.h).
//
// The reference exposes the hot path through two classes (there is no plugin / FFI layer):
//   feature_extraction          mm-loam/src/unionFeatureExtract.cpp:143     detectFeaturePoints :341, getVeloFeature :1113,
//                                                                            getHoriFeatureExtract :952
//   Estimator                   mm-loam/include/Estimator/Estimator.h:25     EstimateLidarPose :211, Estimate :216,
//                                                                            failureDetected :278
//   RemoveLidarDistortion       mm-loam/src/unionPoseEstimation.cpp:402
// This header re-creates those names, argument meanings and error behaviour (no exceptions on the data path, status
// through flags; out-of-grid / NaN points are skipped silently exactly like the reference) over plain buffers.
// PCL / Eigen / ROS are not available in the build image, so clouds are passed as mml::PointXYZINormal arrays with
// pcl::PointXYZINormal's 48-byte layout and field reuse (normal_x = in-scan time, normal_y = ring / line,
// normal_z = label, Estimator.cpp:992-1011); inside a catkin workspace the same struct aliases the PCL type, so the
// adapter works on `cloud->points.data()` without copies of the caller's cloud.
//
// Header-only; link with -lmmloam_hip.  One adapter object per caller thread (the reference's Estimator is not
// re-entrant either, Estimator.h:284-318).
#ifndef MMLOAM_ADAPTER_HPP
#define MMLOAM_ADAPTER_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <stdexcept>
#include <string>
#include <vector>

#include "mmloam_hip.h"

namespace mml {

// pcl::PointXYZINormal memory layout (48 bytes, 16-byte aligned): x,y,z,pad | normal_x,normal_y,normal_z,pad |
// intensity, curvature, pad, pad
struct alignas(16) PointXYZINormal {
    float x, y, z, data_pad;
    float normal_x, normal_y, normal_z, normal_pad;
    float intensity, curvature, pad0, pad1;
};
static_assert(sizeof(PointXYZINormal) == 48, "must match pcl::PointXYZINormal");
using PointCloud = std::vector<PointXYZINormal>;

// union-cloud/msg/union_cloud.msg:4-19 without its header: the six clouds and the four counters of the feature node's message
struct UnionFeatureClouds {
    PointCloud velo_corner, velo_surface, velo_combine;
    PointCloud livox_corner, livox_surface, livox_combine;
    int velo_corner_num = 0, velo_surf_num = 0, livox_corner_num = 0, livox_surf_num = 0;
};

struct Matrix3d {  // row-major
    double m[9];
};
struct Vector3d {
    double v[3];
};
struct Matrix4d {  // row-major
    double m[16];
};
struct Quaterniond {  // x, y, z, w
    double x = 0, y = 0, z = 0, w = 1;
};

inline void check(mml_ctx* ctx, int rc, const char* what) {
    if (rc != MML_OK) throw std::runtime_error(std::string(what) + ": " + (ctx ? mml_last_error(ctx) : "no context"));
}

// RAII owner of one mml_ctx, shared by the two adapter classes of a node pair living in one process
class Context {
   public:
    explicit Context(int max_scans = 1, int device = 0, const mml_config* cfg = nullptr) {
        mml_config c;
        if (cfg)
            c = *cfg;
        else
            mml_config_default(&c, max_scans);
        int rc = mml_create(&c, device, &ctx_);
        if (rc != MML_OK) throw std::runtime_error("mml_create failed (no HIP device? there is no CPU fallback)");
        cfg_ = c;
    }
    ~Context() { mml_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    mml_ctx* get() const { return ctx_; }
    const mml_config& config() const { return cfg_; }

    // Map banks (include/mmloam_hip.h, "map banks"), for a host that replays several sequences in this context: n further local
    // maps, the bank of every slot (-1: the context's own map, the one the Estimator below uses), and MapIncrementLocal for n
    // distinct banks in one call (T_wl: n x 16, row-major; the sizes may be null).  A bank has its own global cube map, which a
    // bound slot is matched against first: set it, or feed its MAP_MANAGER store (featureAssociateToMap / MapIncrement) for n
    // distinct banks in one call each.  bank_increment, segmented = true: mml_map_bank_increment_segmented -- the same banks bit
    // for bit from one chain of launches (2 + R host synchronisations whatever n is); a slot without a stack is refused before
    // any bank changes.
    void map_banks(int n) { check(ctx_, mml_map_banks_create(ctx_, n), "map_banks"); }
    void bind_banks(int first_slot, int count, const int* banks) { check(ctx_, mml_slot_bind_bank(ctx_, first_slot, count, banks), "bind_banks"); }
    void bank_increment(int n, const int* banks, const int* slots, const double* T_wl, int* n_corner = nullptr, int* n_surf = nullptr,
                        bool segmented = false) {
        check(ctx_, (segmented ? mml_map_bank_increment_segmented : mml_map_bank_increment)(ctx_, n, banks, slots, T_wl, n_corner, n_surf),
              "bank_increment");
    }
    void bank_set_global(int bank, int kind, const float* xyz, const int* cube, int m, const int* cen = nullptr) {
        check(ctx_, mml_map_bank_set_global(ctx_, bank, kind, xyz, cube, m, cen), "bank_set_global");
    }
    // segmented = true: mml_map_bank_global_append_segmented / _increment_segmented -- the same stores and match copies bit for
    // bit from one chain of launches (3 + R host synchronisations whatever n is); every refusal leaves every bank as it was.
    void bank_global_append(int n, const int* banks, const int* slots, const double* T_wl, bool segmented = false) {
        check(ctx_, (segmented ? mml_map_bank_global_append_segmented : mml_map_bank_global_append)(ctx_, n, banks, slots, T_wl),
              "bank_global_append");
    }
    void bank_global_increment(int n, const int* banks, const double* T_wl, int* n_corner = nullptr, int* n_surf = nullptr,
                               bool segmented = false) {
        check(ctx_, (segmented ? mml_map_bank_global_increment_segmented : mml_map_bank_global_increment)(ctx_, n, banks, T_wl, n_corner, n_surf),
              "bank_global_increment");
    }

   private:
    mml_ctx* ctx_ = nullptr;
    mml_config cfg_;
};

// The world map of a context (include/mmloam_hip.h, "The world map"): what a replay keeps of /velo_full_cloud_mapped, the
// registered clouds of n sequences voxel-merged on the device.  Created with the object and destroyed with it; the context must
// outlive it.  add: slot first_slot + i into map map_of_slot[i] (-1: skipped) at T_wl[16 i ...] (transformTobeMapped, row-major),
// one device call and one host synchronisation for all slots.  download: the voxels of one map in ascending key order as points
// x, y, z, intensity = the centroid, curvature = the voxel's point count, everything else as in a default-constructed point.
class WorldMap {
   public:
    // surfels = true: a surfel map (MML_WM_SURFELS), 76 bytes per table position instead of 28; moments() and surfels() read it
    WorldMap(Context& ctx, int n_maps, float leaf, long capacity_voxels, bool surfels = false) : ctx_(ctx) {
        check(ctx_.get(), mml_world_map_create_opts(ctx_.get(), n_maps, leaf, capacity_voxels, surfels ? MML_WM_SURFELS : 0u),
              "mml_world_map_create_opts");
    }
    ~WorldMap() { mml_world_map_destroy(ctx_.get()); }
    WorldMap(const WorldMap&) = delete;
    WorldMap& operator=(const WorldMap&) = delete;
    mml_world_map_info add(int first_slot, int count, const int* map_of_slot, const double* T_wl, unsigned label_mask = 7) {
        mml_world_map_info info;
        check(ctx_.get(), mml_world_map_add(ctx_.get(), first_slot, count, map_of_slot, T_wl, label_mask, &info), "mml_world_map_add");
        return info;
    }
    void reset(int map = -1) { check(ctx_.get(), mml_world_map_reset(ctx_.get(), map), "mml_world_map_reset"); }
    long size(int map = -1) {
        long n = 0;
        check(ctx_.get(), mml_world_map_size(ctx_.get(), map, &n), "mml_world_map_size");
        return n;
    }
    long download(int map, PointCloud& cloud) {
        long n = 0;
        check(ctx_.get(), mml_world_map_download(ctx_.get(), map, nullptr, nullptr, 0, &n), "mml_world_map_download");
        std::vector<float> xyzi(4 * (size_t)(n ? n : 1));
        std::vector<int> cnt((size_t)(n ? n : 1));
        if (n) check(ctx_.get(), mml_world_map_download(ctx_.get(), map, xyzi.data(), cnt.data(), n, &n), "mml_world_map_download");
        cloud.assign((size_t)n, PointXYZINormal{0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
        for (long i = 0; i < n; ++i) {
            cloud[i].x = xyzi[4 * i];
            cloud[i].y = xyzi[4 * i + 1];
            cloud[i].z = xyzi[4 * i + 2];
            cloud[i].intensity = xyzi[4 * i + 3];
            cloud[i].curvature = (float)cnt[i];
        }
        return n;
    }
    // a surfel map's voxels in the order of download(): 12 floats each (sdx sdy sdz vx | sxx sxy sxz vy | syy syz szz vz) ...
    std::vector<float> moments(int map) { return rows(map, 12, mml_world_map_download_moments, "mml_world_map_download_moments"); }
    // ... and 8 floats each: nx ny nz | l0 l1 l2 | planarity linearity (eight zeros for a voxel of fewer than 3 points)
    std::vector<float> surfels(int map) { return rows(map, 8, mml_world_map_download_surfels, "mml_world_map_download_surfels"); }

    // One map as it is stored, in the order of download(): what import_voxels takes back bit for bit (into a map that does not hold
    // the voxels yet).  moments stays empty on a plain map.
    struct Voxels {
        std::vector<int> ijk;        // n x 3 voxel indices
        std::vector<float> sums;     // n x 4: the sums x, y, z, intensity (not the centroids)
        std::vector<int> counts;     // n
        std::vector<float> moments;  // n x 12 on a surfel map
    };
    Voxels export_voxels(int map, bool surfels) {
        long n = 0;
        check(ctx_.get(), mml_world_map_export(ctx_.get(), map, nullptr, nullptr, nullptr, nullptr, 0, &n), "mml_world_map_export");
        Voxels v;
        v.ijk.resize(3 * (size_t)n);
        v.sums.resize(4 * (size_t)n);
        v.counts.resize((size_t)n);
        if (surfels) v.moments.resize(12 * (size_t)n);
        if (n)
            check(ctx_.get(), mml_world_map_export(ctx_.get(), map, v.ijk.data(), v.sums.data(), v.counts.data(), surfels ? v.moments.data() : nullptr, n, &n),
                  "mml_world_map_export");
        return v;
    }
    void import_voxels(int map, const Voxels& v) {
        check(ctx_.get(), mml_world_map_import(ctx_.get(), map, (long)v.counts.size(), v.ijk.data(), v.sums.data(), v.counts.data(),
                                               v.moments.empty() ? nullptr : v.moments.data()),
              "mml_world_map_import");
    }
    // Plane factors for the surf stacks of slots first_slot + i from the surfels of map map_of_slot[i] (-1: skipped), one launch;
    // stats: count entries, or nullptr to enqueue only.  The slots are then ready for mml_solve / mml_linearize.
    void associate(int first_slot, int count, const int* map_of_slot, const double* T_wl, const mml_wm_assoc_opts& opts,
                   mml_assoc_stats* stats = nullptr) {
        check(ctx_.get(), mml_world_map_associate(ctx_.get(), first_slot, count, map_of_slot, T_wl, &opts, stats), "mml_world_map_associate");
    }
    // Estimator::Estimate's loop against the map: P (count x 3), Q (count x 4) in and out; the map is only read
    void localize(int first_slot, int count, const int* map_of_slot, const double* exTlb, double* P, double* Q, const mml_wm_localize_opts& opts,
                  mml_estimate_info* info = nullptr) {
        check(ctx_.get(), mml_world_map_localize(ctx_.get(), first_slot, count, map_of_slot, exTlb, P, Q, &opts, info), "mml_world_map_localize");
    }
    // n_hyp pose hypotheses per slot (T_wl: count x n_hyp x 16) scored against the maps in one launch: count x n_hyp results,
    // integers, zeros for a slot with map -1; the map and the slots are only read
    std::vector<mml_wm_score> score(int first_slot, int count, const int* map_of_slot, int n_hyp, const double* T_wl, const mml_wm_score_opts& opts) {
        std::vector<mml_wm_score> out((size_t)(count > 0 ? count : 0) * (size_t)(n_hyp > 0 ? n_hyp : 0));
        check(ctx_.get(), mml_world_map_score(ctx_.get(), first_slot, count, map_of_slot, n_hyp, T_wl, &opts, out.data()), "mml_world_map_score");
        return out;
    }
    // the coarse-to-fine search around the seed poses P, Q, ending in localize: P, Q in and out
    void relocalize(int first_slot, int count, const int* map_of_slot, const double* exTlb, double* P, double* Q, const mml_wm_reloc_opts& opts,
                    mml_wm_reloc_info* info = nullptr) {
        check(ctx_.get(), mml_world_map_relocalize(ctx_.get(), first_slot, count, map_of_slot, exTlb, P, Q, &opts, info), "mml_world_map_relocalize");
    }
    // The index box of a metric one in a map of leaf size `leaf`: lo = index(lo_xyz), hi = index(hi_xyz) + 1 (no context needed)
    static void index_box(float leaf, const float lo_xyz[3], const float hi_xyz[3], int lo[3], int hi[3]) {
        if (mml_wm_index_box(leaf, lo_xyz, hi_xyz, lo, hi) != MML_OK) throw std::runtime_error("mml_wm_index_box: leaf or a coordinate not finite");
    }
    // What one evict call took out: the rows of all named maps in ascending key order (map, then k, j, i), as import_voxels takes
    // them map by map -- info[r].first_row is where the rows of rules[r].map begin -- and one info per rule
    struct Evicted {
        std::vector<int> map;   // n: the map of every row
        Voxels rows;
        std::vector<mml_wm_evict_info> info;
    };
    // At most one rule per map, all in one device chain.  rows = false drops the evicted voxels; dry = true only counts (info).
    Evicted evict(const std::vector<mml_wm_evict_rule>& rules, bool surfels, bool rows = true, bool dry = false) {
        Evicted e;
        e.info.resize(rules.size());
        long n = 0;
        const bool sized = rows && !dry;   // the arrays are sized by a dry run first
        check(ctx_.get(), mml_world_map_evict(ctx_.get(), (int)rules.size(), rules.data(), sized || dry ? MML_WM_EVICT_DRY : 0u, e.info.data(), 0, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, &n),
              "mml_world_map_evict");
        if (!sized) return e;
        const size_t cap = n > 0 ? (size_t)n : 1;
        e.map.resize(cap);
        e.rows.ijk.resize(3 * cap);
        e.rows.sums.resize(4 * cap);
        e.rows.counts.resize(cap);
        if (surfels) e.rows.moments.resize(12 * cap);
        check(ctx_.get(), mml_world_map_evict(ctx_.get(), (int)rules.size(), rules.data(), 0u, e.info.data(), (long)cap, e.map.data(), e.rows.ijk.data(),
                                              e.rows.sums.data(), e.rows.counts.data(), surfels ? e.rows.moments.data() : nullptr, &n),
              "mml_world_map_evict");
        e.map.resize((size_t)n);
        e.rows.ijk.resize(3 * (size_t)n);
        e.rows.sums.resize(4 * (size_t)n);
        e.rows.counts.resize((size_t)n);
        if (surfels) e.rows.moments.resize(12 * (size_t)n);
        return e;
    }

   private:
    std::vector<float> rows(int map, int width, int (*call)(mml_ctx*, int, float*, long, long*), const char* who) {
        long n = 0;
        check(ctx_.get(), call(ctx_.get(), map, nullptr, 0, &n), who);
        std::vector<float> out((size_t)width * (size_t)n);
        if (n) check(ctx_.get(), call(ctx_.get(), map, out.data(), n, &n), who);
        return out;
    }
    Context& ctx_;
};

// ---- feature_extraction (unionFeatureExtract.cpp:143-1320), hot-path members only -----------------------------------
class feature_extraction {
   public:
    explicit feature_extraction(Context& ctx) : ctx_(ctx) {}

    // unionFeatureExtract.cpp:341-343.  `cloud` is one scan line; indices refer to it.
    void detectFeaturePoints(const PointCloud& cloud, std::vector<int>& pointsLessSharp, std::vector<int>& pointsLessFlat) {
        const int n = (int)cloud.size();
        std::vector<float> pts(4 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            pts[4 * i] = cloud[i].x;
            pts[4 * i + 1] = cloud[i].y;
            pts[4 * i + 2] = cloud[i].z;
            pts[4 * i + 3] = cloud[i].intensity;
        }
        std::vector<int> sharp(n ? n : 1), flat(n ? n : 1);
        int ns = 0, nf = 0;
        check(ctx_.get(), mml_detect_line(ctx_.get(), pts.data(), n, sharp.data(), &ns, flat.data(), &nf, nullptr),
              "detectFeaturePoints");
        pointsLessSharp.insert(pointsLessSharp.end(), sharp.begin(), sharp.begin() + ns);
        pointsLessFlat.insert(pointsLessFlat.end(), flat.begin(), flat.begin() + nf);
    }

    // unionCloudHandler (:266-321) minus ROS (de)serialisation and the PCL GICP refresh: one union_cloud message in,
    // the labelled fused cloud [velo_combine ; livox_combine] out, plus the four counters of union_cloud.msg:16-19.
    // velo_xyzi: n_velo x (x,y,z,intensity); livox: msg->livox_time_aligned.points.data().
    void unionCloud(const float* velo_xyzi, int n_velo, const mml_livox_point* livox, int n_livox,
                    const float* livox_extrinsic /*row-major 4x4 or nullptr*/, PointCloud& fused, mml_scan_info& info,
                    int slot = 0) {
        mml_ctx* c = ctx_.get();
        check(c, mml_scan_upload(c, slot, velo_xyzi, n_velo, livox, n_livox), "scan_upload");
        check(c, mml_extract(c, slot, 1, livox_extrinsic), "extract");
        check(c, mml_scan_info_get(c, slot, &info), "scan_info");
        download(slot, info.n_points, fused);
    }

    // unionCloudHandler including its GICP refresh (:302-318): features without an extrinsic, then -- when
    // livox_corner_num > 100 -- extri_mtx re-estimated from the Livox surf cloud against the Velodyne surf cloud (every frame,
    // as the reference does) and applied to the Livox part; extri_mtx (row-major) persists across frames in the caller.
    bool unionCloudRefresh(const float* velo_xyzi, int n_velo, const mml_livox_point* livox, int n_livox, float extri_mtx[16],
                           PointCloud& fused, mml_scan_info& info, int slot = 0) {
        mml_ctx* c = ctx_.get();
        check(c, mml_scan_upload(c, slot, velo_xyzi, n_velo, livox, n_livox), "scan_upload");
        check(c, mml_extract(c, slot, 1, nullptr), "extract");
        int refreshed = 0;
        check(c, mml_gicp_refresh(c, slot, extri_mtx, 1, &refreshed, nullptr), "gicp_refresh");
        check(c, mml_scan_info_get(c, slot, &info), "scan_info");
        download(slot, info.n_points, fused);
        return refreshed != 0;
    }

    // The refresh of unionCloudRefresh for `count` scans already uploaded to the slots first_slot .. (offline replay): ONE persistent
    // extri_mtx carried through the frames -- a frame whose alignment converged replaces it, every other frame (not converged, or
    // livox_corner_num <= 100) keeps it -- exactly the loop of unionCloudRefresh over the slots, in one mml_extract and one
    // mml_gicp_refresh_batch.  fused_out[i]: frame i's fused cloud, its Livox part under the matrix held after frame i;
    // infos (may be null): the frames' counters.  Returns the number of frames that refreshed; extri_mtx is the last frame's matrix.
    int unionCloudRefreshBatch(int first_slot, int count, float extri_mtx[16], std::vector<PointCloud>& fused_out,
                               std::vector<mml_scan_info>* infos = nullptr) {
        mml_ctx* c = ctx_.get();
        check(c, mml_extract(c, first_slot, count, nullptr), "extract");
        std::vector<float> T(16 * (size_t)(count > 0 ? count : 1));
        std::vector<int> refreshed(count > 0 ? count : 1, 0);
        for (int k = 0; k < 16; ++k) T[k] = extri_mtx[k];
        check(c, mml_gicp_refresh_batch(c, first_slot, count, T.data(), 1, 1, refreshed.data(), nullptr), "gicp_refresh_batch");
        for (int k = 0; k < 16; ++k) extri_mtx[k] = T[16 * (size_t)(count - 1) + k];
        fused_out.resize(count);
        if (infos) infos->resize(count);
        int n_refreshed = 0;
        for (int i = 0; i < count; ++i) {
            mml_scan_info info;
            check(c, mml_scan_info_get(c, first_slot + i, &info), "scan_info");
            download(first_slot + i, info.n_points, fused_out[i]);
            if (infos) (*infos)[i] = info;
            n_refreshed += refreshed[i] != 0;
        }
        return n_refreshed;
    }

    // getVeloFeature (:1113-1117) and getHoriFeatureExtract (:952-956) on their own
    void getVeloFeature(const float* velo_xyzi, int n, PointCloud& points_normal, mml_scan_info& info, int slot = 0) {
        unionCloud(velo_xyzi, n, nullptr, 0, nullptr, points_normal, info, slot);
    }
    void getHoriFeatureExtract(const mml_livox_point* pts, int n, PointCloud& laserCloud, mml_scan_info& info, int slot = 0) {
        unionCloud(nullptr, 0, pts, n, nullptr, laserCloud, info, slot);
    }

    // The reference's own signatures: getVeloFeature(msg, normal, corner, surf) (:1113-1117) and getHoriFeatureExtract(msg,
    // cloud, corner, surf) (:952-956).  corner / surf are the sensor's labelled points in RAW order -- the Velodyne ones with the
    // sensor's intensity, cropped near + far (:1244-1252, :1287-1295), the Livox ones cropped near only (:925, :933) --, normal /
    // cloud the combine cloud; all three from one mml_feature_clouds_download.
    void getVeloFeature(const float* velo_xyzi, int n, PointCloud& points_normal, PointCloud& points_corner, PointCloud& points_surf,
                        mml_scan_info& info, int slot = 0) {
        extractOnly(velo_xyzi, n, nullptr, 0, info, slot);
        std::vector<UnionFeatureClouds> m;
        unionCloudMessage(slot, 1, m);
        points_normal.swap(m[0].velo_combine);
        points_corner.swap(m[0].velo_corner);
        points_surf.swap(m[0].velo_surface);
    }
    void getHoriFeatureExtract(const mml_livox_point* pts, int n, PointCloud& laserCloud, PointCloud& laserConerCloud,
                               PointCloud& laserSurfCloud, mml_scan_info& info, int slot = 0) {
        extractOnly(nullptr, 0, pts, n, info, slot);
        std::vector<UnionFeatureClouds> m;
        unionCloudMessage(slot, 1, m);
        laserCloud.swap(m[0].livox_combine);
        laserConerCloud.swap(m[0].livox_corner);
        laserSurfCloud.swap(m[0].livox_surface);
    }

    // The union_cloud messages of `count` extracted slots (what unionCloudHandler fills at :287-293 and publishes at :942-947,
    // :1302-1306), from ONE mml_feature_clouds_download_batch behind its sizing call.  Stamps and frame ids are the caller's.
    void unionCloudMessage(int first_slot, int count, std::vector<UnionFeatureClouds>& out) {
        mml_ctx* c = ctx_.get();
        std::vector<int> n(6 * (size_t)(count > 0 ? count : 1), 0);
        check(c, mml_feature_clouds_download_batch(c, first_slot, count, nullptr, 0, n.data()), "mml_feature_clouds_download_batch");
        long total = 0;
        for (int i = 0; i < 6 * count; ++i) total += n[i];
        PointCloud data((size_t)total);
        if (total > 0)
            check(c, mml_feature_clouds_download_batch(c, first_slot, count, reinterpret_cast<uint8_t*>(data.data()), total, n.data()),
                  "mml_feature_clouds_download_batch");
        out.assign(count, UnionFeatureClouds{});
        const PointXYZINormal* p = data.data();
        for (int i = 0; i < count; ++i) {
            UnionFeatureClouds& m = out[i];
            PointCloud* clouds[6] = {&m.velo_corner, &m.velo_surface, &m.velo_combine, &m.livox_corner, &m.livox_surface, &m.livox_combine};
            for (int k = 0; k < 6; ++k) {
                clouds[k]->assign(p, p + n[6 * i + k]);
                p += n[6 * i + k];
            }
            m.velo_corner_num = n[6 * i];
            m.velo_surf_num = n[6 * i + 1];
            m.livox_corner_num = n[6 * i + 3];
            m.livox_surf_num = n[6 * i + 4];
        }
    }

    // The way in of unionCloudHandler (:266-293) for `count` union_cloud messages held as raw bytes (a bag reader, a feature node
    // in a process of its own): pcl::fromROSMsg (:1119-1121) and the CustomPoint field reads (:985-997) for all of them in ONE
    // mml_scan_upload_wire_batch, then one mml_extract over the slots.  Frame i's velo_time_aligned payload is n_velo[i] records
    // of point_step bytes at velo_data + velo_at[i] (field offsets as in msg.fields), its livox_time_aligned.points n_livox[i]
    // serialised records of livox_record_bytes (19, or 20 for in-memory structs) at livox_data + livox_at[i]; the offsets may
    // point into one mapped chunk with the message headers between the payloads.  infos (may be null): the frames' counters.
    void unionCloudWire(int first_slot, int count, const uint8_t* velo_data, const int64_t* velo_at, const int* n_velo, int point_step,
                        int off_x, int off_y, int off_z, int off_intensity, const uint8_t* livox_data, const int64_t* livox_at,
                        const int* n_livox, int livox_record_bytes = 19, const float* livox_extrinsic = nullptr,
                        std::vector<mml_scan_info>* infos = nullptr) {
        mml_ctx* c = ctx_.get();
        check(c, mml_scan_upload_wire_batch(c, first_slot, count, velo_data, velo_at, n_velo, point_step, off_x, off_y, off_z, off_intensity,
                                            livox_data, livox_at, n_livox, livox_record_bytes), "mml_scan_upload_wire_batch");
        check(c, mml_extract(c, first_slot, count, livox_extrinsic), "extract");
        if (!infos) return;
        infos->resize(count);
        for (int i = 0; i < count; ++i) check(c, mml_scan_info_get(c, first_slot + i, &(*infos)[i]), "scan_info");
    }

    // upload + extract without an extrinsic + counters: the slot is left for the download the caller chooses
    void extractOnly(const float* velo_xyzi, int n_velo, const mml_livox_point* livox, int n_livox, mml_scan_info& info, int slot) {
        mml_ctx* c = ctx_.get();
        check(c, mml_scan_upload(c, slot, velo_xyzi, n_velo, livox, n_livox), "scan_upload");
        check(c, mml_extract(c, slot, 1, nullptr), "extract");
        check(c, mml_scan_info_get(c, slot, &info), "scan_info");
    }

    void download(int slot, int n, PointCloud& out) {
        std::vector<float> xyzi(4 * (size_t)(n ? n : 1)), rel(n ? n : 1);
        std::vector<uint8_t> line(n ? n : 1), label(n ? n : 1);
        check(ctx_.get(), mml_scan_download(ctx_.get(), slot, xyzi.data(), rel.data(), line.data(), label.data(), n ? n : 1),
              "scan_download");
        out.assign(n, PointXYZINormal{});
        for (int i = 0; i < n; ++i) {
            out[i].x = xyzi[4 * i];
            out[i].y = xyzi[4 * i + 1];
            out[i].z = xyzi[4 * i + 2];
            out[i].data_pad = 1.f;
            out[i].intensity = xyzi[4 * i + 3];
            out[i].normal_x = rel[i];
            out[i].normal_y = (float)line[i];
            out[i].normal_z = (float)label[i];
        }
    }

   private:
    Context& ctx_;
};

// ---- icp_ext_matching (unionFeatureExtract.cpp:74-123): the GICP behind the per-frame extrinsic refresh --------------------
// bool icp_ext_matching(cloud_src, cloud_tgt, cloud_aligned, icp_mtx, en_viewer): icp_mtx (row-major here) is assigned and
// cloud_aligned filled only when the alignment converged.
inline bool icp_ext_matching(Context& ctx, const PointCloud& cloud_src, const PointCloud& cloud_tgt, PointCloud& cloud_aligned,
                             float icp_mtx[16]) {
    std::vector<float> s(3 * cloud_src.size() + 3), t(3 * cloud_tgt.size() + 3);
    for (size_t i = 0; i < cloud_src.size(); ++i) {
        s[3 * i] = cloud_src[i].x;
        s[3 * i + 1] = cloud_src[i].y;
        s[3 * i + 2] = cloud_src[i].z;
    }
    for (size_t i = 0; i < cloud_tgt.size(); ++i) {
        t[3 * i] = cloud_tgt[i].x;
        t[3 * i + 1] = cloud_tgt[i].y;
        t[3 * i + 2] = cloud_tgt[i].z;
    }
    int converged = 0;
    check(ctx.get(), mml_gicp_align(ctx.get(), s.data(), (int)cloud_src.size(), t.data(), (int)cloud_tgt.size(), icp_mtx, &converged, nullptr),
          "icp_ext_matching");
    if (!converged) return false;
    cloud_aligned = cloud_src;  // icp.align(*cloud_aligned): the source under the final transformation
    for (auto& p : cloud_aligned) {
        const float x = icp_mtx[0] * p.x + icp_mtx[1] * p.y + icp_mtx[2] * p.z + icp_mtx[3];
        const float y = icp_mtx[4] * p.x + icp_mtx[5] * p.y + icp_mtx[6] * p.z + icp_mtx[7];
        const float z = icp_mtx[8] * p.x + icp_mtx[9] * p.y + icp_mtx[10] * p.z + icp_mtx[11];
        p.x = x;
        p.y = y;
        p.z = z;
    }
    return true;
}

// icp_ext_matching for a list of cloud pairs in one device call (mml_gicp_align_batch): pair i's result is what icp_ext_matching
// returns for it alone.  icp_mtx: 16 floats per pair, in/out; cloud_aligned[i] is filled, and converged[i] set, only when pair i
// converged.  Returns the number of pairs that converged.
inline int icp_ext_matching_batch(Context& ctx, const std::vector<PointCloud>& cloud_src, const std::vector<PointCloud>& cloud_tgt,
                                  std::vector<PointCloud>& cloud_aligned, std::vector<float>& icp_mtx, std::vector<char>& converged) {
    if (cloud_src.size() != cloud_tgt.size() || icp_mtx.size() != 16 * cloud_src.size())
        throw std::runtime_error("icp_ext_matching_batch: one target and 16 matrix entries per source cloud");
    const int n = (int)cloud_src.size();
    std::vector<int> so(n + 1, 0), to(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        so[i + 1] = so[i] + (int)cloud_src[i].size();
        to[i + 1] = to[i] + (int)cloud_tgt[i].size();
    }
    std::vector<float> s(3 * (size_t)so[n] + 3), t(3 * (size_t)to[n] + 3);
    for (int i = 0; i < n; ++i) {
        for (size_t k = 0; k < cloud_src[i].size(); ++k) {
            float* o = &s[3 * ((size_t)so[i] + k)];
            o[0] = cloud_src[i][k].x, o[1] = cloud_src[i][k].y, o[2] = cloud_src[i][k].z;
        }
        for (size_t k = 0; k < cloud_tgt[i].size(); ++k) {
            float* o = &t[3 * ((size_t)to[i] + k)];
            o[0] = cloud_tgt[i][k].x, o[1] = cloud_tgt[i][k].y, o[2] = cloud_tgt[i][k].z;
        }
    }
    std::vector<int> conv(n ? n : 1, 0);
    check(ctx.get(), mml_gicp_align_batch(ctx.get(), n, s.data(), so.data(), t.data(), to.data(), icp_mtx.data(), conv.data(), nullptr),
          "icp_ext_matching_batch");
    cloud_aligned.resize(n);
    converged.assign(n, 0);
    int n_conv = 0;
    for (int i = 0; i < n; ++i) {
        if (!conv[i]) continue;
        converged[i] = 1;
        ++n_conv;
        const float* m = &icp_mtx[16 * (size_t)i];
        cloud_aligned[i] = cloud_src[i];
        for (auto& p : cloud_aligned[i]) {
            const float x = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
            const float y = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
            const float z = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
            p.x = x;
            p.y = y;
            p.z = z;
        }
    }
    return n_conv;
}

// ---- RemoveLidarDistortion (unionPoseEstimation.cpp:402-403): in place on the slot's device-resident fused cloud ----
inline void RemoveLidarDistortion(Context& ctx, int slot, const Matrix3d& dRlc, const Vector3d& dtlc) {
    check(ctx.get(), mml_undistort(ctx.get(), slot, 1, dRlc.m, dtlc.v), "RemoveLidarDistortion");
}

// A labelled cloud that arrived over /union_feature_cloud (velo_combine followed by livox_combine, the merge of
// unionPoseEstimation.cpp:746-757) -> scan slot: pcl::fromROSMsg on the device.  n_velo = velo_combine's size.
// n_velo = -1 (the caller does not know the split, as the reference's RemoveLidarDistortion does not): the cloud fills the
// Velodyne region first and spills the rest into the Livox region, so a merged cloud of up to max_velo_points +
// max_livox_points is accepted; the velo_* / livox_* label counts and mml_gicp_refresh are then not meaningful for the slot
// (undistortion, down-sampling and the estimator do not depend on the split).
inline void uploadCloud(Context& ctx, int slot, const PointCloud& cloud, int n_velo = -1) {
    const int n = (int)cloud.size();
    if (n_velo < 0) n_velo = n < ctx.config().max_velo_points ? n : ctx.config().max_velo_points;
    check(ctx.get(), mml_cloud_upload(ctx.get(), slot, reinterpret_cast<const uint8_t*>(cloud.data()), n, n_velo),
          "mml_cloud_upload");
}

// void RemoveLidarDistortion(pcl::PointCloud<PointType>::Ptr& cloud, const Eigen::Matrix3d& dRlc, const Eigen::Vector3d& dtlc)
// exactly as the pose node calls it (unionPoseEstimation.cpp:862): the CALLER's cloud is undistorted in place (x, y, z
// rewritten, normal_x = 1, :416-419).  The cloud stays resident in `slot` as well, so a LidarFrame built from it can
// name the slot instead of carrying the points back (LidarFrame::resident).
inline void RemoveLidarDistortion(Context& ctx, PointCloud& cloud, const Matrix3d& dRlc, const Vector3d& dtlc, int slot = 0,
                                  int n_velo = -1) {
    const int n = (int)cloud.size();
    if (n == 0) return;
    uploadCloud(ctx, slot, cloud, n_velo);
    check(ctx.get(), mml_undistort(ctx.get(), slot, 1, dRlc.m, dtlc.v), "RemoveLidarDistortion");
    std::vector<float> xyzi(4 * (size_t)n), rel(n);
    check(ctx.get(), mml_scan_download(ctx.get(), slot, xyzi.data(), rel.data(), nullptr, nullptr, n), "scan_download");
    for (int i = 0; i < n; ++i) {
        cloud[i].x = xyzi[4 * i];
        cloud[i].y = xyzi[4 * i + 1];
        cloud[i].z = xyzi[4 * i + 2];
        cloud[i].normal_x = rel[i];
    }
}

// ---- Estimator (Estimator.h:25-343), hot-path members only ------------------------------------------------------------
class Estimator {
   public:
    static const int SLIDEWINDOWSIZE = 5;  // Estimator.h:30

    struct LidarFrame {  // Estimator.h:33-56
        // laserCloud (Estimator.h:35): the caller's labelled, undistorted cloud.  When set (and not `resident`) it is
        // uploaded into scan slot `slot` at the start of EstimateLidarPose / EstimateFullWindow; a cloud that is already
        // in the slot (extracted there, or left there by RemoveLidarDistortion(ctx, cloud, ...)) is named by slot alone.
        PointCloud* laserCloud = nullptr;
        int n_velo = -1;        // velo_combine's share of laserCloud (-1: all of it)
        bool resident = false;  // the slot already holds this cloud
        int slot = 0;
        Vector3d P{{0, 0, 0}};
        Vector3d V{{0, 0, 0}};
        Quaterniond Q;
        Vector3d bg{{0, 0, 0}};
        Vector3d ba{{0, 0, 0}};
        double timeStamp = 0;
        int lidarType = 0;
    };

    // FeatureLine / FeaturePlanVec (Estimator.h:59-84, 105-122) as the association leaves them.  sqrt_info of the plane
    // factor is carried as the plane normal omega: sqrt_info^T sqrt_info = a^2 w w^T + b^2 (I - w w^T) does not depend on the
    // basis the reference's SVD happens to pick (a = 1 / lidar_m, b = plan_weight_tan / lidar_m, Estimator.cpp:675-682).
    struct FeatureLine {
        Vector3d pointOri, lineP1, lineP2;
        double error = 0;
        bool valid = false;
    };
    struct FeaturePlanVec {
        Vector3d pointOri, pointProj, omega;
        double error = 0;
        bool valid = false;
    };
    double thres_dist = 25.0;  // Estimator.h:332, set by Estimate() (25 -> 10 -> 1, Estimator.cpp:1207,1377-1381)
    // EstimateFullWindow: true = the joint ceres::Solve is one device-resident iteration (mml_fullwindow_solve, needs the
    // window in consecutive slots); false = host iteration with one device evaluation per trust-region step
    bool device_window_solve = true;
    // EstimateFullWindow: true = frame 0 is marginalized by one device call (mml_fullwindow_marginalize_batch, n = 1) without
    // fetching its lidar record; false = record read-back + mml_fullwindow_marginalize on the host.  The priors are bit-identical.
    bool device_marginalize = false;

    // processPointToLine / processPointToPlanVec (Estimator.h:159-186, Estimator.cpp:148-365, 573-777) for the down-sampled
    // stacks of `slot` at lidar pose m4d = transformTobeMapped: kNN + model fit on the device (both kinds in one launch),
    // the surviving features appended to the vector with their ComputeError() value; `valid` = |error| > 1e-5, i.e.
    // the factor enters the problem (:1313,1325).  The cost functions themselves stay on the device (mml_solve).
    void processPointToLine(std::vector<FeatureLine>& vLineFeatures, int slot, const Matrix4d& m4d) {
        associate(slot, m4d);
        std::vector<double> f;
        const int n = factors(slot, 0, f);
        for (int i = 0; i < n; ++i) {
            FeatureLine l;
            for (int c = 0; c < 3; ++c) {
                l.pointOri.v[c] = f[10 * i + c];
                l.lineP1.v[c] = f[10 * i + 3 + c];
                l.lineP2.v[c] = f[10 * i + 6 + c];
            }
            l.error = f[10 * i + 9];
            l.valid = std::fabs(l.error) > 1e-5;
            vLineFeatures.push_back(l);
        }
    }
    void processPointToPlanVec(std::vector<FeaturePlanVec>& vPlanFeatures, int slot, const Matrix4d& m4d, bool& is_degenerate) {
        mml_assoc_stats st = associate(slot, m4d);
        if (st.is_degenerate) is_degenerate = true;  // only ever set, never cleared (:771-775)
        std::vector<double> f;
        const int n = factors(slot, 1, f);
        for (int i = 0; i < n; ++i) {
            FeaturePlanVec pl;
            for (int c = 0; c < 3; ++c) {
                pl.pointOri.v[c] = f[10 * i + c];
                pl.pointProj.v[c] = f[10 * i + 3 + c];
                pl.omega.v[c] = f[10 * i + 6 + c];
            }
            pl.error = f[10 * i + 9];
            pl.valid = std::fabs(pl.error) > 1e-5;
            vPlanFeatures.push_back(pl);
        }
    }

    // Estimate(lidarFrameList, exTlb, gravity, is_degenerate) (Estimator.h:216-219) in the live 1-frame mode (windowSize !=
    // SLIDEWINDOWSIZE, Estimator.cpp:1143-1581): every frame registered against the maps, poses updated in place.
    void Estimate(std::list<LidarFrame>& lidarFrameList, const Matrix4d& exTlb, const Vector3d& gravity, bool& is_degenerate) {
        (void)gravity;
        for (auto& f : lidarFrameList) {
            double Q[4] = {f.Q.x, f.Q.y, f.Q.z, f.Q.w};
            mml_estimate_info info;
            check(ctx_.get(), mml_estimate(ctx_.get(), f.slot, 1, exTlb.m, f.P.v, Q, 5, 10, &info), "Estimate");
            f.Q.x = Q[0];
            f.Q.y = Q[1];
            f.Q.z = Q[2];
            f.Q.w = Q[3];
            if (info.is_degenerate) is_degenerate = true;
        }
    }

    int keyScans() const { return key_scans_; }
    int localMapCorners() const { return n_corner_map_; }
    int localMapSurfs() const { return n_surf_map_; }

    // get_corner_map() / get_surf_map() (Estimator.h:221-226): the MAP_MANAGER cube store, concatenated
    PointCloud get_corner_map() { return global_map(0); }
    PointCloud get_surf_map() { return global_map(1); }

    // Estimator(const float& filter_corner, const float& filter_surf) (Estimator.h:147): the leaf sizes are part of
    // mml_config (leaf_corner / leaf_surf) and must match the context's.
    Estimator(Context& ctx, float filter_corner, float filter_surf) : ctx_(ctx) {
        mml_config c;
        check(ctx.get(), mml_config_get(ctx.get(), &c), "mml_config_get");
        if (c.leaf_corner != filter_corner || c.leaf_surf != filter_surf)
            throw std::invalid_argument("Estimator: filter_corner / filter_surf differ from the context's leaf_corner / leaf_surf");
    }

    // pcl::fromROSMsg + the LidarFrame hand-over: bring every frame's cloud into its slot
    void residentClouds(std::list<LidarFrame>& frames) {
        for (auto& f : frames) stage(f);
    }

    // laserCloud{Corner,Surf}FromLocal (Estimator.cpp:1159-1167): replaces kdtree->setInputCloud
    void setLocalMap(const float* corner_xyz, int n_corner, const float* surf_xyz, int n_surf) {
        check(ctx_.get(), mml_map_set_local(ctx_.get(), 0, corner_xyz, n_corner), "map corner");
        check(ctx_.get(), mml_map_set_local(ctx_.get(), 1, surf_xyz, n_surf), "map surf");
        n_corner_map_ = n_corner;
        n_surf_map_ = n_surf;
    }

    // laserCloud{Corner,Surf}FromMap[4851] + kdtree{Corner,Surf}FromMap[4851] (Estimator.cpp:1170-1184): the cube
    // clouds concatenated, cube[i] = index of point i's cube in the MAP_MANAGER arrays; cen = laserCloudCen*_last.
    void setGlobalMap(const float* corner_xyz, const int* corner_cube, int n_corner, const float* surf_xyz,
                      const int* surf_cube, int n_surf, const int cen[3]) {
        check(ctx_.get(), mml_map_set_global(ctx_.get(), 0, corner_xyz, corner_cube, n_corner, cen), "global corner");
        check(ctx_.get(), mml_map_set_global(ctx_.get(), 1, surf_xyz, surf_cube, n_surf, cen), "global surf");
    }

    // Estimator::threadMapIncrement (Estimator.cpp:92-145) with the MAP_MANAGER cube stores on the device:
    // featureAssociateToMap -> mml_map_global_append, MapIncrement (+ MapMove) -> mml_map_global_increment.
    void appendToGlobalMap(const LidarFrame& f, const Matrix4d& transformForMap) {
        check(ctx_.get(), mml_map_global_append(ctx_.get(), f.slot, transformForMap.m), "featureAssociateToMap");
    }
    void incrementGlobalMap(const Matrix4d& transform) {
        check(ctx_.get(), mml_map_global_increment(ctx_.get(), transform.m, nullptr, nullptr), "MapIncrement");
    }

    // EstimateLidarPose(std::list<LidarFrame>&, exTlb, gravity, lidarMode) (Estimator.h:211-214, Estimator.cpp:967-1140).
    // Live 1-frame mode: the list holds one frame; it is registered against the local map, the
    // pose is updated in place, and the key-scan rule (:1121-1135) grows the local map ON THE DEVICE
    // (mml_map_increment_local replaces MapIncrementLocal + the two kd-tree rebuilds of the next Estimate call).
    // failureDetected() reports the degeneracy flag (:1139).
    void EstimateLidarPose(std::list<LidarFrame>& lidarFrameList, const Matrix4d& exTlb, const Vector3d& gravity,
                           int lidarMode) {
        (void)gravity;
        if (lidarFrameList.empty()) return;
        // exRbl = exTlb.R^T, exPbl = -exRbl * exTlb.t (:973-974)
        double exRbl[9], exPbl[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) exRbl[3 * r + c] = exTlb.m[4 * c + r];
        for (int r = 0; r < 3; ++r)
            exPbl[r] = -1.0 * ((exRbl[3 * r] * exTlb.m[3] + exRbl[3 * r + 1] * exTlb.m[7]) + exRbl[3 * r + 2] * exTlb.m[11]);
        auto to_be_mapped = [&](const LidarFrame& f, double* T) {
            const double x = f.Q.x, y = f.Q.y, z = f.Q.z, w = f.Q.w;
            const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                                 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                                 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c)
                    T[4 * r + c] = (R[3 * r] * exRbl[c] + R[3 * r + 1] * exRbl[3 + c]) + R[3 * r + 2] * exRbl[6 + c];
                T[4 * r + 3] = ((R[3 * r] * exPbl[0] + R[3 * r + 1] * exPbl[1]) + R[3 * r + 2] * exPbl[2]) + f.P.v[r];
            }
            T[12] = T[13] = T[14] = 0;
            T[15] = 1;
        };
        double T[16];
        to_be_mapped(lidarFrameList.back(), T);  // :975-977
        int corner_cnt = 0;
        for (auto& f : lidarFrameList) {
            stage(f);
            mml_scan_info si;
            check(ctx_.get(), mml_scan_info_get(ctx_.get(), f.slot, &si), "scan info");
            corner_cnt += si.fused_corner_num;  // :990-996
            check(ctx_.get(), mml_downsample(ctx_.get(), f.slot, 1), "downsample");  // :1013-1024
        }
        bool is_degenerate = false;
        if (n_corner_map_ > 0 && n_surf_map_ > 100) Estimate(lidarFrameList, exTlb, gravity, is_degenerate);  // :1032-1035
        LidarFrame& front = lidarFrameList.front();
        if ((lidarMode == 1 && !is_degenerate && corner_cnt > 100) || (lidarMode == 2 && corner_cnt > 50)) {
            to_be_mapped(front, T);  // :1041-1049
        } else {                     // :1050-1066
            T[3] = front.P.v[0];
            T[7] = front.P.v[1];
        }
        if (!is_degenerate) {  // :1070-1136
            // Both modes COMPARE with last_velo_update_pose (:1082, :1119); mode 1 WRITES last_hori_update_pose (:1115), which
            // nothing ever reads: a Horizon-mode estimator that never sees a mode-2 call keeps comparing with (-1, -1, -1) and
            // grows its map on every scan farther than sqrt(0.5) m from there.  Preserved as it is.
            const double dx = last_velo_update_pose_[0] - T[3], dy = last_velo_update_pose_[1] - T[7], dz = last_velo_update_pose_[2] - T[11];
            const double d2 = lidarMode == 2 ? (double)(float)(dx * dx + dy * dy + dz * dz) : (dx * dx + dy * dy + dz * dz);
            if (d2 >= 0.5 && (lidarMode == 1 || lidarMode == 2)) {
                check(ctx_.get(), mml_map_increment_local(ctx_.get(), front.slot, T, &n_corner_map_, &n_surf_map_),
                      "MapIncrementLocal");
                ++key_scans_;
                double* last = lidarMode == 2 ? last_velo_update_pose_ : last_hori_update_pose_;
                last[0] = T[3];
                last[1] = T[7];
                last[2] = T[11];
            }
        }
        _fail_detected = is_degenerate;  // :1139
    }

    // Estimate(lidarFrameList, exTlb, gravity, is_degenerate) in full-window mode (windowSize == SLIDEWINDOWSIZE,
    // Estimator.cpp:1143-1581, IMU_Mode = 2): lidar factors of every frame associated once (thres_dist 1,
    // plan_weight_tan 3e-4, no loss) and linearised on the device, IMU factors (LidarFrame::imu) between consecutive
    // frames, the marginalization prior of the previous call; 5 outer x 10 inner iterations, then frame 0 is
    // marginalized (:1448-1567).  imu[f] (f >= 1) = the pre-integration between frames f-1 and f
    // (mml_imu_preintegrate replaces IMUIntegrator::PreIntegration).
    void EstimateFullWindow(std::vector<LidarFrame*>& frames, const std::vector<mml_imu_preint>& imu, const Matrix4d& exTlb,
                            const Vector3d& gravity) {
        const int W = (int)frames.size();
        if (W < 1 || W > 8 || (int)imu.size() < W) throw std::runtime_error("EstimateFullWindow: bad window");
        for (auto* f : frames) {
            if (f->laserCloud && !f->resident) {
                stage(*f);
                check(ctx_.get(), mml_downsample(ctx_.get(), f->slot, 1), "downsample");  // Estimator.cpp:1013-1024
            }
        }
        double T_bl[16];  // inverse of exTlb
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) T_bl[4 * r + c] = exTlb.m[4 * c + r];
            T_bl[4 * r + 3] = -((exTlb.m[r] * exTlb.m[3] + exTlb.m[4 + r] * exTlb.m[7]) + exTlb.m[8 + r] * exTlb.m[11]);
        }
        T_bl[12] = T_bl[13] = T_bl[14] = 0;
        T_bl[15] = 1;
        const double w_tan = 0.0003, thres_dist = 1.0;  // :1203-1204
        std::vector<double> x(15 * (size_t)W), rec(32 * (size_t)W);
        for (int it = 0; it < 5; ++it) {
            for (int f = 0; f < W; ++f) {  // vector2double (:937-950)
                const LidarFrame& l = *frames[f];
                double* xf = &x[15 * (size_t)f];
                for (int k = 0; k < 3; ++k) {
                    xf[k] = l.P.v[k];
                    xf[6 + k] = l.V.v[k];
                    xf[9 + k] = l.bg.v[k];
                    xf[12 + k] = l.ba.v[k];
                }
                quat_log(l.Q, xf + 3);
            }
            if (it == 0)
                for (int f = 0; f < W; ++f) {
                    double T_wl[16];
                    body_to_lidar_world(*frames[f], exTlb, T_wl);
                    check(ctx_.get(), mml_associate(ctx_.get(), frames[f]->slot, 1, T_wl, thres_dist, nullptr), "associate");
                }
            const Quaterniond q_before = frames[W - 1]->Q;
            const Vector3d t_before = frames[W - 1]->P;
            mml_solve_opts so{10, 0, 0.0, w_tan};
            mml_fullwindow* fw = mml_fullwindow_create(W, &so);
            if (!fw) throw std::runtime_error("mml_fullwindow_create");
            for (int f = 1; f < W; ++f) mml_fullwindow_set_imu(fw, f, &imu[f], gravity.v);
            if (have_prior_) mml_fullwindow_set_prior(fw, &prior_);
            bool consecutive = true;
            for (int f = 1; f < W; ++f) consecutive = consecutive && frames[f]->slot == frames[0]->slot + f;
            auto lidar_records = [&]() {
                if (consecutive) {  // one launch + one read-back for the whole window
                    check(ctx_.get(), mml_linearize_window(ctx_.get(), frames[0]->slot, W, 15, x.data(), T_bl, w_tan, 0.0, rec.data()),
                          "linearize_window");
                    return;
                }
                for (int f = 0; f < W; ++f) {
                    double H[36], g[6], c;
                    check(ctx_.get(), mml_linearize(ctx_.get(), frames[f]->slot, &x[15 * (size_t)f], T_bl, w_tan, 0.0, H, g, &c),
                          "linearize");
                    double* r = &rec[32 * (size_t)f];
                    int k = 0;
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b) r[k++] = H[6 * a + b];
                    for (int a = 0; a < 6; ++a) r[21 + a] = g[a];
                    r[27] = c;
                    r[28] = r[29] = r[30] = r[31] = 0;
                }
            };
            if (consecutive && device_window_solve) {  // ceres::Solve as one device-resident iteration
                const int rc = mml_fullwindow_solve(ctx_.get(), fw, frames[0]->slot, T_bl, x.data(), nullptr, nullptr);
                if (rc != MML_OK) {
                    mml_fullwindow_destroy(fw);
                    check(ctx_.get(), rc, "mml_fullwindow_solve");
                }
            } else {
                for (int guard = 0; guard < 200; ++guard) {  // host iteration, one device evaluation per step
                    lidar_records();
                    const int rc = mml_fullwindow_step(fw, rec.data(), x.data());
                    if (rc < 0) {
                        mml_fullwindow_destroy(fw);
                        throw std::runtime_error("mml_fullwindow_step");
                    }
                    if (rc == 1) break;
                }
            }
            for (int f = 0; f < W; ++f) {  // double2vector (:952-964)
                LidarFrame& l = *frames[f];
                const double* xf = &x[15 * (size_t)f];
                for (int k = 0; k < 3; ++k) {
                    l.P.v[k] = xf[k];
                    l.V.v[k] = xf[6 + k];
                    l.bg.v[k] = xf[9 + k];
                    l.ba.v[k] = xf[12 + k];
                }
                quat_exp(xf + 3, l.Q);
            }
            const Quaterniond& qa = frames[W - 1]->Q;
            const double dot = std::fabs(q_before.x * qa.x + q_before.y * qa.y + q_before.z * qa.z + q_before.w * qa.w);
            const double deltaR = 2.0 * std::acos(dot > 1.0 ? 1.0 : dot) * 180.0 / M_PI;
            double dT = 0;
            for (int k = 0; k < 3; ++k) dT += (t_before.v[k] - frames[W - 1]->P.v[k]) * (t_before.v[k] - frames[W - 1]->P.v[k]);
            const bool last = (deltaR < 0.05 && std::sqrt(dT) < 0.05) || it == 4;
            if (last && W >= 2) {  // :1453-1546
                if (device_marginalize) {
                    std::vector<double> xw(MML_FW_X_STRIDE, 0.0);
                    std::memcpy(xw.data(), x.data(), sizeof(double) * x.size());
                    const int first = frames[0]->slot;
                    have_prior_ = mml_fullwindow_marginalize_batch(ctx_.get(), 1, &fw, &first, T_bl, xw.data(), &prior_) == MML_OK;
                } else {
                    lidar_records();
                    have_prior_ = mml_fullwindow_marginalize(fw, rec.data(), x.data(), &prior_) == MML_OK;
                }
            }
            mml_fullwindow_destroy(fw);
            if (last) break;
        }
    }

    bool failureDetected() const { return _fail_detected; }  // Estimator.h:278

    // The pose node's loop after EstimateLidarPose (unionPoseEstimation.cpp:896-903: pointAssociateToMap over the front
    // frame's cloud) and pcl::toROSMsg (:907): `data` becomes laserCloudMsg.data, 48-byte PointXYZINormal records of the
    // cloud in `slot` at T = transformTobeMapped (row-major 4x4, :876-880), transformed and packed on the device.  Returns
    // the number of points.
    int RegisteredCloud(int slot, const double T[16], std::vector<uint8_t>& data) {
        std::vector<int> n;
        return (int)RegisteredCloud(slot, 1, T, data, n);
    }
    // The same for `count` resident slots in one device call (a replay): slot first_slot + i at T[16 i ...]; the records of
    // slot i start at record n_points[0] + ... + n_points[i-1] of `data`.  Returns the total number of points.
    long RegisteredCloud(int first_slot, int count, const double* T, std::vector<uint8_t>& data, std::vector<int>& n_points) {
        n_points.assign(count > 0 ? count : 1, 0);
        check(ctx_.get(), mml_cloud_download_registered_batch(ctx_.get(), first_slot, count, T, nullptr, 0, n_points.data()),
              "mml_cloud_download_registered_batch");
        long total = 0;
        for (int i = 0; i < count; ++i) total += n_points[i];
        data.assign(48 * (size_t)total, 0);
        if (total)
            check(ctx_.get(), mml_cloud_download_registered_batch(ctx_.get(), first_slot, count, T, data.data(), total, n_points.data()),
                  "mml_cloud_download_registered_batch");
        n_points.resize(count > 0 ? count : 0);
        return total;
    }

    // The pose node's way in for a replay (unionPoseEstimation.cpp:679-688, :719-773): the messages of `msgs.size()` frames
    // into slots first_slot ..., packed into one block and handed over in ONE mml_pose_ingest_batch call, which also takes
    // the node's decision per message -- merge livox_combine or not, detected_fast_rotation, the frame dropped because
    // fetchImuMsgs returned nothing.  rows: what ImuQueue's fetch wrote for the frames' intervals, or nullptr (IMU_Mode 0).
    // A frame's livox_corner_num is the size of its livox_corner cloud, as in the feature node's message.  Returns one row per
    // frame; the slots of the frames that were not dropped are ready for RemoveLidarDistortion / EstimateLidarPose.
    std::vector<mml_pose_ingest_row> IngestUnionClouds(int first_slot, const std::vector<UnionFeatureClouds>& msgs, const mml_imu_interval* rows,
                                                       const mml_pose_ingest_opts& opts) {
        const size_t n = msgs.size();
        std::vector<int> np(6 * (n ? n : 1), 0);
        size_t total = 0;
        for (size_t i = 0; i < n; ++i) {
            const PointCloud* c[6] = {&msgs[i].velo_corner,  &msgs[i].velo_surface,  &msgs[i].velo_combine,
                                      &msgs[i].livox_corner, &msgs[i].livox_surface, &msgs[i].livox_combine};
            for (int k = 0; k < 6; ++k) total += (size_t)(np[6 * i + k] = (int)c[k]->size());
        }
        PointCloud block;
        block.reserve(total);
        for (const UnionFeatureClouds& m : msgs)
            for (const PointCloud* c : {&m.velo_corner, &m.velo_surface, &m.velo_combine, &m.livox_corner, &m.livox_surface, &m.livox_combine})
                block.insert(block.end(), c->begin(), c->end());
        std::vector<mml_pose_ingest_row> out(n ? n : 1);
        check(ctx_.get(),
              mml_pose_ingest_batch(ctx_.get(), first_slot, (int)n, total ? reinterpret_cast<const uint8_t*>(block.data()) : nullptr, np.data(), rows,
                                    &opts, out.data()),
              "mml_pose_ingest_batch");
        out.resize(n);
        return out;
    }

   private:
    mml_assoc_stats associate(int slot, const Matrix4d& m4d) {
        mml_assoc_stats st;
        check(ctx_.get(), mml_associate(ctx_.get(), slot, 1, m4d.m, thres_dist, &st), "mml_associate");
        return st;
    }
    int factors(int slot, int kind, std::vector<double>& f) {
        int n = 0;
        check(ctx_.get(), mml_factors_download(ctx_.get(), slot, kind, nullptr, nullptr, 0, &n), "mml_factors_download");
        f.assign(10 * (size_t)(n > 0 ? n : 1), 0.0);
        check(ctx_.get(), mml_factors_download(ctx_.get(), slot, kind, f.data(), nullptr, n > 0 ? n : 1, &n), "mml_factors_download");
        return n;
    }
    PointCloud global_map(int kind) {
        int n = 0, cen[3];
        check(ctx_.get(), mml_map_global_download(ctx_.get(), kind, nullptr, nullptr, 0, &n, cen), "mml_map_global_download");
        std::vector<float> xyz(3 * (size_t)(n > 0 ? n : 1));
        check(ctx_.get(), mml_map_global_download(ctx_.get(), kind, xyz.data(), nullptr, n, &n, cen), "mml_map_global_download");
        PointCloud out(n, PointXYZINormal{});
        for (int i = 0; i < n; ++i) {
            out[i].x = xyz[3 * i];
            out[i].y = xyz[3 * i + 1];
            out[i].z = xyz[3 * i + 2];
            out[i].data_pad = 1.f;
        }
        return out;
    }
    void stage(LidarFrame& f) {
        if (f.laserCloud && !f.resident) {
            uploadCloud(ctx_, f.slot, *f.laserCloud, f.n_velo);
            f.resident = true;
        }
    }
    // Sophus::SO3d(Q).log() / SO3d::exp(phi).unit_quaternion()
    static void quat_log(const Quaterniond& q, double* w) {
        const double n2 = q.x * q.x + q.y * q.y + q.z * q.z, n = std::sqrt(n2);
        double k;
        if (n2 < 1e-20)
            k = 2.0 / q.w - (2.0 / 3.0) * n2 / (q.w * q.w * q.w);
        else if (std::fabs(q.w) < 1e-10)
            k = (q.w > 0 ? M_PI : -M_PI) / n;
        else
            k = 2.0 * std::atan(n / q.w) / n;
        w[0] = k * q.x;
        w[1] = k * q.y;
        w[2] = k * q.z;
    }
    static void quat_exp(const double* w, Quaterniond& q) {
        const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        double im, re;
        if (th2 < 1e-20) {
            im = 0.5 - th2 / 48.0;
            re = 1.0 - th2 / 8.0;
        } else {
            const double th = std::sqrt(th2);
            im = std::sin(0.5 * th) / th;
            re = std::cos(0.5 * th);
        }
        q.x = im * w[0];
        q.y = im * w[1];
        q.z = im * w[2];
        q.w = re;
    }
    // transformTobeMapped = [Q exRbl | Q exPbl + P] (:1266-1268)
    static void body_to_lidar_world(const LidarFrame& f, const Matrix4d& exTlb, double* T) {
        const double x = f.Q.x, y = f.Q.y, z = f.Q.z, w = f.Q.w;
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                             2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        double exRbl[9], exPbl[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) exRbl[3 * r + c] = exTlb.m[4 * c + r];
        for (int r = 0; r < 3; ++r)
            exPbl[r] = -1.0 * ((exRbl[3 * r] * exTlb.m[3] + exRbl[3 * r + 1] * exTlb.m[7]) + exRbl[3 * r + 2] * exTlb.m[11]);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                T[4 * r + c] = (R[3 * r] * exRbl[c] + R[3 * r + 1] * exRbl[3 + c]) + R[3 * r + 2] * exRbl[6 + c];
            T[4 * r + 3] = ((R[3 * r] * exPbl[0] + R[3 * r + 1] * exPbl[1]) + R[3 * r + 2] * exPbl[2]) + f.P.v[r];
        }
        T[12] = T[13] = T[14] = 0;
        T[15] = 1;
    }
    Context& ctx_;
    mml_prior prior_;
    bool have_prior_ = false;
    int n_corner_map_ = 0, n_surf_map_ = 0;
    int key_scans_ = 0;  // scans that entered the local map (the key-scan rule of :1121-1135)
    double last_velo_update_pose_[3] = {-1.0, -1.0, -1.0};  // Estimator.h:339-340
    double last_hori_update_pose_[3] = {-1.0, -1.0, -1.0};
    bool _fail_detected = false;
};

// ---- LidarsParamEstimator (unionLidarsAligner.cpp): the start-up calibration of hori_cloud_handler (:221-270) --------------
// calibratePCLICP (lidars_extrinsic_cali.h:493-618) on the device (mml_aligner_calibrate): source_cloud = _hori_igcloud, target_cloud =
// _velo_new_cloud, both packed x, y, z, intensity floats.  On convergence tf_matrix (row-major 4 x 4) receives
// getFinalTransformation() and, when velo_hori_tf is given, that receives _velo_hori_tf_matrix as :251-253 build it ([R^T | -t],
// not the rigid inverse); otherwise both stay as they were.  Returns hasConverged().  (save_pcd has no counterpart.)
inline bool calibratePCLICP(Context& ctx, const float* source_cloud, int n_source, const float* target_cloud, int n_target, float* tf_matrix,
                            float* velo_hori_tf = nullptr, mml_calib_info* info = nullptr) {
    float unused[16];
    int converged = 0;
    check(ctx.get(), mml_aligner_calibrate(ctx.get(), source_cloud, n_source, target_cloud, n_target, tf_matrix,
                                           velo_hori_tf ? velo_hori_tf : unused, &converged, info),
          "mml_aligner_calibrate");
    return converged != 0;
}

// ---- LidarsParamEstimator (unionLidarsAligner.cpp): the numeric core of estimate_timeoffset (:1077-1153) ----------------
// velo_fov / livox: packed x, y, z floats (the FOV-cropped Velodyne cloud of :1080 and the merged Livox points of
// :1053-1068); velo_hori_tf: _velo_hori_tf_matrix, row-major.  Returns the start index of the best window in the merged
// Livox array (cnt * resolution, the argument of livox_msg_offset_vec at :1143), or -1 when no window beats the 1e6
// start value; *lowest_error is what :1155 compares with _time_esti_error_th.
struct TimeOffsetResult {
    int n_windows = 0, best_window = -1;
    double lowest_error = 1000000.0;
};
inline TimeOffsetResult EstimateTimeOffsetCore(Context& ctx, const float* velo_fov, int n_velo, const float* velo_hori_tf,
                                               const float* livox, int n_livox, int offset_search_resolution = 30,
                                               int offset_search_sliced_points = 12000) {
    TimeOffsetResult r;
    check(ctx.get(), mml_time_offset_search(ctx.get(), velo_fov, n_velo, velo_hori_tf, livox, n_livox, offset_search_resolution,
                                            offset_search_sliced_points, nullptr, nullptr, 0, &r.n_windows, &r.best_window,
                                            &r.lowest_error),
          "mml_time_offset_search");
    return r;
}
// What the search ends in (:1146, :1161): _time_offset = velo_stamp - (livox_msg.timebase + livox_msg_offset_vec[best_window]), in
// uint64 nanoseconds as the reference holds it (it wraps when the Livox clock is ahead; :520 subtracts it again in uint64).
// offset_of_best_window_point: the merged array's entry at TimeOffsetResult::best_window, offset_time + (timebase - livox_timebase)
// (:1062-1068).  The frames of the time-offset mode then start at velo_stamp - time_offset_ns(...):
// LivoxPointQueue::pub_horipoints_given_stamp(start_stamp, sliced_points, ...) below.
inline uint64_t time_offset_ns(uint64_t velo_stamp, uint64_t livox_timebase, uint64_t offset_of_best_window_point) {
    return velo_stamp - (livox_timebase + offset_of_best_window_point);
}
// EstimateTimeOffsetCore for a list of (Velodyne FOV cloud, merged Livox cloud) pairs in one device call
// (mml_time_offset_search_batch): every queued velo_fov_vec entry against the merged Livox points, or the searches of a bag's
// fast-rotation events replayed at once.  velo_fov[i] / livox[i]: packed x, y, z floats; velo_hori_tf: 16 floats used for every
// pair, 16 per pair, or empty (no transform).  Result i is what EstimateTimeOffsetCore returns for pair i alone.
inline std::vector<TimeOffsetResult> estimate_timeoffset_batch(Context& ctx, const std::vector<std::vector<float>>& velo_fov,
                                                               const std::vector<std::vector<float>>& livox,
                                                               const std::vector<float>& velo_hori_tf, int offset_search_resolution = 30,
                                                               int offset_search_sliced_points = 12000) {
    const size_t n = velo_fov.size();
    if (livox.size() != n || !(velo_hori_tf.empty() || velo_hori_tf.size() == 16 || velo_hori_tf.size() == 16 * n))
        throw std::runtime_error("estimate_timeoffset_batch: one Livox cloud per Velodyne cloud; 0, 16 or 16 n matrix entries");
    std::vector<int> vo(n + 1, 0), lo(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        if (velo_fov[i].size() % 3 || livox[i].size() % 3) throw std::runtime_error("estimate_timeoffset_batch: clouds are packed x, y, z");
        vo[i + 1] = vo[i] + (int)(velo_fov[i].size() / 3);
        lo[i + 1] = lo[i] + (int)(livox[i].size() / 3);
    }
    std::vector<float> v(3 * (size_t)vo[n] + 3), l(3 * (size_t)lo[n] + 3), tf;
    for (size_t i = 0; i < n; ++i) {
        std::copy(velo_fov[i].begin(), velo_fov[i].end(), v.begin() + 3 * (size_t)vo[i]);
        std::copy(livox[i].begin(), livox[i].end(), l.begin() + 3 * (size_t)lo[i]);
    }
    if (velo_hori_tf.size() == 16 && n != 1)
        for (size_t i = 0; i < n; ++i) tf.insert(tf.end(), velo_hori_tf.begin(), velo_hori_tf.end());
    else
        tf = velo_hori_tf;
    std::vector<int> nwin(n ? n : 1, 0), best(n ? n : 1, -1);
    std::vector<double> lowest(n ? n : 1, 1000000.0);
    check(ctx.get(), mml_time_offset_search_batch(ctx.get(), (int)n, v.data(), vo.data(), tf.empty() ? nullptr : tf.data(), l.data(), lo.data(),
                                                  offset_search_resolution, offset_search_sliced_points, nullptr, nullptr, nullptr, nwin.data(),
                                                  best.data(), lowest.data()),
          "mml_time_offset_search_batch");
    std::vector<TimeOffsetResult> r(n);
    for (size_t i = 0; i < n; ++i) {
        r[i].n_windows = nwin[i];
        r[i].best_window = best[i];
        r[i].lowest_error = lowest[i];
    }
    return r;
}

// ---- velo_cloud_handler's FOV selection (unionLidarsAligner.cpp:437-490): velo_fovs_cloud from the PointCloud2 payload -----------
// data / n_points / point_step / off_*: pointCloudIn->data.data(), width * height, point_step and the offsets of the float32
// fields x, y, z in pointCloudIn->fields -- no pcl::fromROSMsg loop.  ctx == nullptr runs the same routine on the host.
// VeloFovCloud is velo_fovs_cloud for one or many frames: xyzi holds the kept points as x, y, z, intensity = relTime (the
// pcl::PointXYZI fields the reference fills), xyz the same points packed x, y, z, offsets[i] .. offsets[i+1] the rows of frame i
// (n + 1 entries); info[i] = startOri, endOri, the point that set halfPassed, the count.
struct VeloFovCloud {
    std::vector<float> xyzi, xyz;
    std::vector<int> offsets;
    std::vector<mml_velo_fov_info> info;
    size_t size() const { return xyz.size() / 3; }
};
struct VeloFrame {  // what the selection needs of a sensor_msgs/PointCloud2: msg.data.data(), msg.width * msg.height
    const uint8_t* data = nullptr;
    int n_points = 0;
};
inline VeloFovCloud select_velo_fov_batch(Context* ctx, const std::vector<VeloFrame>& frames, int point_step, int off_x, int off_y, int off_z) {
    VeloFovCloud c;
    const size_t n = frames.size();
    c.offsets.assign(n + 1, 0);
    c.info.resize(n);
    if (n == 0) return c;
    mml_ctx* h = ctx ? ctx->get() : nullptr;
    // the frames lie anywhere in memory: offsets are taken from the lowest address among them
    const uint8_t* base = nullptr;
    for (const VeloFrame& f : frames)
        if (f.n_points > 0 && (!base || f.data < base)) base = f.data;
    std::vector<long> at(n, 0);
    std::vector<int> np(n, 0), kept(n, 0);
    for (size_t i = 0; i < n; ++i) {
        np[i] = frames[i].n_points;
        at[i] = frames[i].n_points > 0 ? (long)(frames[i].data - base) : 0;
    }
    check(h, mml_velo_fov_select_batch(h, (int)n, base, at.data(), np.data(), point_step, off_x, off_y, off_z, nullptr, nullptr, 0, kept.data(),
                                       nullptr),
          "mml_velo_fov_select_batch");
    for (size_t i = 0; i < n; ++i) c.offsets[i + 1] = c.offsets[i] + kept[i];
    const long total = c.offsets[n];
    c.xyzi.resize(4 * (size_t)total + 4);
    c.xyz.resize(3 * (size_t)total + 3);
    check(h, mml_velo_fov_select_batch(h, (int)n, base, at.data(), np.data(), point_step, off_x, off_y, off_z, c.xyzi.data(), c.xyz.data(), total,
                                       kept.data(), c.info.data()),
          "mml_velo_fov_select_batch");
    c.xyzi.resize(4 * (size_t)total);
    c.xyz.resize(3 * (size_t)total);
    return c;
}
inline VeloFovCloud select_velo_fov(Context* ctx, const uint8_t* data, int n_points, int point_step, int off_x, int off_y, int off_z) {
    return select_velo_fov_batch(ctx, std::vector<VeloFrame>{VeloFrame{data, n_points}}, point_step, off_x, off_y, off_z);
}
// estimate_timeoffset_batch on a selection as it stands: cloud i of `velo_fov` against livox[i] -- no repacking of the Velodyne side.
inline std::vector<TimeOffsetResult> estimate_timeoffset_batch(Context& ctx, const VeloFovCloud& velo_fov, const std::vector<std::vector<float>>& livox,
                                                               const std::vector<float>& velo_hori_tf, int offset_search_resolution = 30,
                                                               int offset_search_sliced_points = 12000) {
    const size_t n = velo_fov.offsets.empty() ? 0 : velo_fov.offsets.size() - 1;
    if (livox.size() != n || !(velo_hori_tf.empty() || velo_hori_tf.size() == 16 || velo_hori_tf.size() == 16 * n))
        throw std::runtime_error("estimate_timeoffset_batch: one Livox cloud per Velodyne cloud; 0, 16 or 16 n matrix entries");
    std::vector<int> lo(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        if (livox[i].size() % 3) throw std::runtime_error("estimate_timeoffset_batch: clouds are packed x, y, z");
        lo[i + 1] = lo[i] + (int)(livox[i].size() / 3);
    }
    std::vector<float> l(3 * (size_t)lo[n] + 3), tf;
    for (size_t i = 0; i < n; ++i) std::copy(livox[i].begin(), livox[i].end(), l.begin() + 3 * (size_t)lo[i]);
    if (velo_hori_tf.size() == 16 && n != 1)
        for (size_t i = 0; i < n; ++i) tf.insert(tf.end(), velo_hori_tf.begin(), velo_hori_tf.end());
    else
        tf = velo_hori_tf;
    std::vector<int> nwin(n ? n : 1, 0), best(n ? n : 1, -1);
    std::vector<double> lowest(n ? n : 1, 1000000.0);
    check(ctx.get(), mml_time_offset_search_batch(ctx.get(), (int)n, velo_fov.xyz.data(), velo_fov.offsets.data(), tf.empty() ? nullptr : tf.data(),
                                                  l.data(), lo.data(), offset_search_resolution, offset_search_sliced_points, nullptr, nullptr,
                                                  nullptr, nwin.data(), best.data(), lowest.data()),
          "mml_time_offset_search_batch");
    std::vector<TimeOffsetResult> r(n);
    for (size_t i = 0; i < n; ++i) {
        r[i].n_windows = nwin[i];
        r[i].best_window = best[i];
        r[i].lowest_error = lowest[i];
    }
    return r;
}

// ---- the aligner node's point queue (unionLidarsAligner.cpp: _hori_points_queue / _hori_points_stamp_queue) on the device -------
// transform_hori_timestamp (:736-763) pushes the queued messages; pub_horipoints_given_stamp (:766-868) cuts one Velodyne frame
// interval out of the queue and, where the reference publishes a union_cloud (:343-364), fills a scan slot: the Livox points with
// their rewritten offset_time and the Velodyne cloud transformed by _velo_hori_tf_matrix.  The return value is the reference's
// bool; last_frame() tells why a frame came back false (mml_union_frame.status; the cases the reference leaves undefined are
// defined in include/mmloam_hip.h).  mml_extract on the slot follows, as after mml_scan_upload.  Destroy before the Context.
struct LivoxMsg {  // what the queue needs of a livox_ros_driver/CustomMsg: msg.timebase, msg.points.data(), msg.points.size()
    uint64_t timebase = 0;
    const mml_livox_point* points = nullptr;
    int point_num = 0;
};
class LivoxPointQueue {
   public:
    LivoxPointQueue(Context& ctx, long capacity_points) : ctx_(ctx) {
        check(ctx.get(), mml_livox_stream_create(ctx.get(), capacity_points, &s_), "mml_livox_stream_create");
    }
    ~LivoxPointQueue() { mml_livox_stream_destroy(s_); }
    LivoxPointQueue(const LivoxPointQueue&) = delete;
    LivoxPointQueue& operator=(const LivoxPointQueue&) = delete;
    mml_livox_stream* get() const { return s_; }

    // :736-763.  The points must stay valid until the next synchronising call (pub_horipoints_given_stamp is one).
    void transform_hori_timestamp(const std::vector<LivoxMsg>& hori_msg_vec) {
        for (const LivoxMsg& m : hori_msg_vec) {
            check(ctx_.get(), mml_livox_stream_push(s_, m.timebase, m.points, m.point_num), "mml_livox_stream_push");
            marks_.push_back(Mark{m.timebase, pushed_, m.point_num});
            pushed_ += m.point_num;
        }
    }
    // What the queue knows from its pushes: per message its time base, its first point's absolute index and its point count
    // (hori_vec's boundaries for estimate_timeoffset below, :1049-1074).  drop_marks_before forgets the messages that end at or
    // before `front` (what the assemble calls have erased).
    struct Mark {
        uint64_t timebase;
        long first;
        int count;
    };
    const std::vector<Mark>& marks() const { return marks_; }
    void drop_marks_before(long front) {
        size_t k = 0;
        while (k < marks_.size() && marks_[k].first + marks_[k].count <= front) ++k;
        marks_.erase(marks_.begin(), marks_.begin() + (long)k);
    }
    // :766-868 with :350-352: one frame into `slot`.  velo_xyzi: n_velo x (x, y, z, intensity); velo_hori_tf: 16 floats or nullptr.
    bool pub_horipoints_given_stamp(uint64_t velo_start_stamp, uint64_t velo_end_stamp, const float* velo_xyzi, int n_velo,
                                    const float* velo_hori_tf, int slot) {
        const uint64_t stamps[2] = {velo_start_stamp, velo_end_stamp};
        const int vo[2] = {0, n_velo};
        frames_.resize(1);
        check(ctx_.get(), mml_union_assemble(ctx_.get(), s_, slot, 1, stamps, velo_xyzi, vo, velo_hori_tf, frames_.data()), "mml_union_assemble");
        return frames_[0].status == 0;
    }
    // count frames in one device call: frame i = [stamps[i], stamps[i + 1]) with rows velo_offsets[i] .. velo_offsets[i + 1] - 1 of
    // velo_xyzi into slot first_slot + i.  Returns the reference's bool per frame.
    std::vector<bool> pub_horipoints_given_stamp(const std::vector<uint64_t>& stamps, const float* velo_xyzi, const std::vector<int>& velo_offsets,
                                                 const float* velo_hori_tf, int first_slot) {
        if (stamps.size() < 2 || velo_offsets.size() != stamps.size())
            throw std::runtime_error("pub_horipoints_given_stamp: count + 1 stamps and count + 1 offsets");
        const int count = (int)stamps.size() - 1;
        frames_.resize((size_t)count);
        check(ctx_.get(), mml_union_assemble(ctx_.get(), s_, first_slot, count, stamps.data(), velo_xyzi, velo_offsets.data(), velo_hori_tf,
                                             frames_.data()),
              "mml_union_assemble");
        std::vector<bool> ok((size_t)count);
        for (int i = 0; i < count; ++i) ok[(size_t)i] = frames_[(size_t)i].status == 0;
        return ok;
    }
    // :872-1009 with :513-551, the one-stamp overload the aligner runs once the time offset is known: up to sliced_points
    // (_offset_search_sliced_points) points from the first one at or after start_stamp (= Velodyne stamp - time offset, :520;
    // time_offset_ns above) into `slot`, with the Velodyne cloud.  A false return may have erased points (NOT_REACHED leaves one).
    // The overloads are told apart as the reference's are: by the second argument, uint64_t end stamp or int point count.
    bool pub_horipoints_given_stamp(uint64_t start_stamp, int sliced_points, const float* velo_xyzi, int n_velo, const float* velo_hori_tf,
                                    int slot) {
        const int vo[2] = {0, n_velo};
        frames_.resize(1);
        check(ctx_.get(), mml_union_assemble_offset(ctx_.get(), s_, slot, 1, &start_stamp, sliced_points, velo_xyzi, vo, velo_hori_tf, frames_.data()),
              "mml_union_assemble_offset");
        return frames_[0].status == 0;
    }
    // count such frames in one device call: starts[i] with rows velo_offsets[i] .. velo_offsets[i + 1] - 1 into slot first_slot + i.
    std::vector<bool> pub_horipoints_given_stamp(const std::vector<uint64_t>& starts, int sliced_points, const float* velo_xyzi,
                                                 const std::vector<int>& velo_offsets, const float* velo_hori_tf, int first_slot) {
        if (starts.empty() || velo_offsets.size() != starts.size() + 1)
            throw std::runtime_error("pub_horipoints_given_stamp: count starts and count + 1 offsets");
        const int count = (int)starts.size();
        frames_.resize((size_t)count);
        check(ctx_.get(), mml_union_assemble_offset(ctx_.get(), s_, first_slot, count, starts.data(), sliced_points, velo_xyzi, velo_offsets.data(),
                                                    velo_hori_tf, frames_.data()),
              "mml_union_assemble_offset");
        std::vector<bool> ok((size_t)count);
        for (int i = 0; i < count; ++i) ok[(size_t)i] = frames_[(size_t)i].status == 0;
        return ok;
    }
    const std::vector<mml_union_frame>& last_frames() const { return frames_; }
    const mml_union_frame& last_frame() const { return frames_.back(); }
    mml_livox_stream_state state() {
        mml_livox_stream_state st;
        check(ctx_.get(), mml_livox_stream_state_get(s_, &st), "mml_livox_stream_state_get");
        return st;
    }
    void reset() {
        check(ctx_.get(), mml_livox_stream_reset(s_), "mml_livox_stream_reset");
        marks_.clear();
        pushed_ = 0;
    }

   private:
    Context& ctx_;
    mml_livox_stream* s_ = nullptr;
    std::vector<mml_union_frame> frames_;
    std::vector<Mark> marks_;
    long pushed_ = 0;
};

// LidarsParamEstimator::estimate_timeoffset (:1021-1166) on the queue: the gate of :1026-1043 (mml_time_offset_gate) over the queued
// Velodyne frames, then ONE mml_time_offset_estimate_stream call for the frame it selects against the queue's last eight messages
// -- FOV selection, search and stamps on the device, nothing handed over through host memory.  velo_msgs / velo_stamps: velo_vec,
// oldest first, as payloads (point_step / off_*: the PointCloud2 layout) and header stamps in ns; hori_stamp: hori_vec.back()'s
// header stamp.  The result is the selected frame's row, `accepted` being _time_offset_initd and `time_offset` _time_offset;
// `selected` is the frame's index, -1 with gate_status EMPTY / TOO_FEW_MESSAGES (defined refusals, include/mmloam_hip.h), in which
// case no device call is made.
struct TimeOffsetEstimate {
    int gate_status = MML_TOFS_GATE_EMPTY, selected = -1;
    mml_time_offset_estimate_row row = {0, 0, 0, -1, 1000000.0, 0, 0, 0, 0};
};
inline TimeOffsetEstimate estimate_timeoffset(Context& ctx, LivoxPointQueue& queue, const std::vector<VeloFrame>& velo_msgs,
                                              const std::vector<uint64_t>& velo_stamps, uint64_t hori_stamp, const float* velo_hori_tf,
                                              int offset_search_resolution, int offset_search_sliced_points, double time_esti_error_th,
                                              int point_step = 16, int off_x = 0, int off_y = 4, int off_z = 8) {
    if (velo_msgs.size() != velo_stamps.size()) throw std::runtime_error("estimate_timeoffset: one stamp per Velodyne frame");
    TimeOffsetEstimate r;
    const std::vector<LivoxPointQueue::Mark>& marks = queue.marks();
    check(ctx.get(), mml_time_offset_gate((int)velo_stamps.size(), velo_stamps.data(), hori_stamp, (int)marks.size(), &r.selected, &r.gate_status),
          "mml_time_offset_gate");
    if (r.selected < 0) return r;
    const LivoxPointQueue::Mark &first = marks[marks.size() - 8], &last = marks.back();
    const VeloFrame& f = velo_msgs[(size_t)r.selected];
    const long at = 0;
    check(ctx.get(), mml_time_offset_estimate_stream(ctx.get(), queue.get(), first.first, last.first + last.count, 1, f.data, &at, &f.n_points,
                                                     point_step, off_x, off_y, off_z, &velo_stamps[(size_t)r.selected], velo_hori_tf,
                                                     offset_search_resolution, offset_search_sliced_points, time_esti_error_th, nullptr, nullptr,
                                                     nullptr, &r.row),
          "mml_time_offset_estimate_stream");
    return r;
}

// ---- the pose node's IMU queue (unionPoseEstimation.cpp: _imuMsgVector) --------------------------------------------------------
// push is imuHandler's push_back (:296); fetchImuMsgs (:307-395) cuts (startTime, endTime] out of the queue, the message
// synthesised at endTime included, and returns the reference's bool (true iff the status is 0, as :394).  A message is 7
// doubles: header.stamp.toSec(), angular_velocity xyz, linear_acceleration xyz; vimuMsg comes back as rows of 7 doubles in the
// shape IMUIntegrator below takes (gyro xyz, accel xyz, dt with lastTime = startTime).  last_interval() tells why a call came
// back false (mml_imu_interval.status; NO_SAMPLE, which the reference leaves undefined, is defined in include/mmloam_hip.h).
// With a Context the queue is a mml_imu_stream in device memory and the batch form is ONE mml_imu_fetch_batch call; without one
// it is a host vector and the calls run mml_imu_fetch_host, bit-identical to it.  Unlike the reference's, fetchImuMsgs does
// not trim the queue: drop_before is :383-390 (t = min(_time_last_hori, _time_last_velo), keep_min = 200).
class ImuQueue {
   public:
    ImuQueue() = default;
    ImuQueue(Context& ctx, long capacity_msgs) : ctx_(&ctx) {
        check(ctx.get(), mml_imu_stream_create(ctx.get(), capacity_msgs, &s_), "mml_imu_stream_create");
    }
    ~ImuQueue() { mml_imu_stream_destroy(s_); }
    ImuQueue(const ImuQueue&) = delete;
    ImuQueue& operator=(const ImuQueue&) = delete;
    mml_imu_stream* get() const { return s_; }

    // one message (7 doubles) or n of them.  On a device queue the buffer must stay valid until the next synchronising call.
    void push(const double* msg, int n = 1) {
        if (s_)
            check(ctx_->get(), mml_imu_stream_push(s_, msg, n), "mml_imu_stream_push");
        else
            host_.insert(host_.end(), msg, msg + 7 * (size_t)n);
    }
    bool fetchImuMsgs(double startTime, double endTime, std::vector<double>& vimuMsg) {
        const std::vector<bool> ok = fetchImuMsgs(std::vector<double>{startTime}, std::vector<double>{endTime});
        vimuMsg = samples_;
        return ok[0];
    }
    // n intervals in one call: interval i's rows are last_samples() rows last_offsets()[i] .. last_offsets()[i + 1] - 1.
    std::vector<bool> fetchImuMsgs(const std::vector<double>& startTimes, const std::vector<double>& endTimes) {
        if (startTimes.empty() || startTimes.size() != endTimes.size()) throw std::runtime_error("fetchImuMsgs: one start and one end per interval");
        const int n = (int)startTimes.size();
        rows_.resize((size_t)n);
        offsets_.assign((size_t)n + 1, 0);
        samples_.clear();
        call(n, startTimes.data(), endTimes.data(), nullptr, 0);   // the sizing call
        samples_.resize(7 * (size_t)offsets_[(size_t)n]);
        if (!samples_.empty()) call(n, startTimes.data(), endTimes.data(), samples_.data(), offsets_[(size_t)n]);
        std::vector<bool> ok((size_t)n);
        for (int i = 0; i < n; ++i) ok[(size_t)i] = rows_[(size_t)i].status == 0;
        return ok;
    }
    void drop_before(double t, long keep_min = 200) {
        if (s_) {
            check(ctx_->get(), mml_imu_stream_drop_before(s_, t, keep_min), "mml_imu_stream_drop_before");
            return;
        }
        size_t front = 0;
        while ((long)(host_.size() / 7 - front) > keep_min && host_[7 * front] < t) ++front;
        host_.erase(host_.begin(), host_.begin() + (std::ptrdiff_t)(7 * front));
    }
    long size() {
        if (!s_) return (long)(host_.size() / 7);
        mml_imu_stream_state st;
        check(ctx_->get(), mml_imu_stream_state_get(s_, &st), "mml_imu_stream_state_get");
        return st.tail - st.front;
    }
    const std::vector<mml_imu_interval>& last_intervals() const { return rows_; }
    const mml_imu_interval& last_interval() const { return rows_.back(); }
    const std::vector<double>& last_samples() const { return samples_; }
    const std::vector<int>& last_offsets() const { return offsets_; }

   private:
    void call(int n, const double* ts, const double* te, double* samples, long cap) {
        if (s_)
            check(ctx_->get(), mml_imu_fetch_batch(ctx_->get(), s_, n, ts, te, nullptr, nullptr, rows_.data(), offsets_.data(), samples, cap, nullptr, nullptr),
                  "mml_imu_fetch_batch");
        else
            check(nullptr, mml_imu_fetch_host(host_.data(), (long)(host_.size() / 7), n, ts, te, nullptr, nullptr, rows_.data(), offsets_.data(), samples,
                                              cap, nullptr, nullptr),
                  "mml_imu_fetch_host");
    }
    Context* ctx_ = nullptr;
    mml_imu_stream* s_ = nullptr;
    std::vector<double> host_;
    std::vector<mml_imu_interval> rows_;
    std::vector<double> samples_;
    std::vector<int> offsets_;
};

// ---- IMUIntegrator (IMUIntegrator.h / IMUIntegrator.cpp) over the caller's messages ----------------------------------------
// A message is 7 doubles: angular_velocity xyz, linear_acceleration xyz (units of g, as the Livox IMU reports them), dt to the
// previous message (the stamp difference the reference forms from lastTime, :95-97, :122).  Reset() keeps the messages, as
// the reference's Reset (:49-58) does.
class IMUIntegrator {
   public:
    void PushIMUMsg(const double* msg) { msgs.insert(msgs.end(), msg, msg + 7); }
    void PushIMUMsg(const std::vector<double>& msg7n) { msgs.insert(msgs.end(), msg7n.begin(), msg7n.end()); }
    int size() const { return (int)(msgs.size() / 7); }
    void Reset() {
        dq = Quaterniond();
        has_pre = false;
    }
    // GyroIntegration (:90-106): accumulates onto dq (not reset); throws on a dt < 0 (the reference's ROS_ASSERT)
    void GyroIntegration() {
        double q[4] = {dq.x, dq.y, dq.z, dq.w};
        check(nullptr, mml_imu_gyro_integrate(msgs.data(), size(), q), "mml_imu_gyro_integrate");
        dq.x = q[0], dq.y = q[1], dq.z = q[2], dq.w = q[3];
    }
    // PreIntegration (:108-166) with the linearisation biases bg / ba; `pre` holds the result
    void PreIntegration(const Vector3d& bg, const Vector3d& ba) {
        check(nullptr, mml_imu_preintegrate(msgs.data(), size(), bg.v, ba.v, &pre), "mml_imu_preintegrate");
        dq.x = pre.dq[0], dq.y = pre.dq[1], dq.z = pre.dq[2], dq.w = pre.dq[3];
        has_pre = true;
    }
    // PreIntegration() of many integrators in one mml_imu_preintegrate_batch call: integrators[i] with the biases bg[i] / ba[i].
    // ctx null: the host routine; otherwise one device call, bit-identical to it.  Every integrator is left as PreIntegration
    // leaves it; `out` (may be null) also receives the results in order.
    static void PreIntegrationBatch(mml_ctx* ctx, const std::vector<IMUIntegrator*>& integrators, const std::vector<Vector3d>& bg,
                                    const std::vector<Vector3d>& ba, std::vector<mml_imu_preint>* out = nullptr) {
        const size_t n = integrators.size();
        if (bg.size() != n || ba.size() != n) throw std::runtime_error("PreIntegrationBatch: one bg and one ba per integrator");
        std::vector<double> smp, b(6 * n);
        std::vector<int> offsets(1, 0);
        for (size_t i = 0; i < n; ++i) {
            smp.insert(smp.end(), integrators[i]->msgs.begin(), integrators[i]->msgs.end());
            offsets.push_back(offsets.back() + integrators[i]->size());
            for (int k = 0; k < 3; ++k) b[3 * i + k] = bg[i].v[k], b[3 * (n + i) + k] = ba[i].v[k];
        }
        std::vector<mml_imu_preint> pre(n);
        check(ctx, mml_imu_preintegrate_batch(ctx, (int)n, smp.data(), offsets.data(), b.data(), b.data() + 3 * n, pre.data()),
              "mml_imu_preintegrate_batch");
        for (size_t i = 0; i < n; ++i) {
            IMUIntegrator& it = *integrators[i];
            it.pre = pre[i];
            it.dq.x = pre[i].dq[0], it.dq.y = pre[i].dq[1], it.dq.z = pre[i].dq[2], it.dq.w = pre[i].dq[3];
            it.has_pre = true;
        }
        if (out) *out = pre;
    }
    // GetAverageAcc (:168-181): the mean of the first 31 messages' linear_acceleration * gnorm
    Vector3d GetAverageAcc() const {
        Vector3d s{{0, 0, 0}};
        int i = 0;
        for (int k = 0; k < size(); ++k) {
            for (int c = 0; c < 3; ++c) s.v[c] += msgs[7 * (size_t)k + 3 + c] * 9.805;
            i++;
            if (i > 30) break;
        }
        for (int c = 0; c < 3; ++c) s.v[c] /= i;
        return s;
    }
    const Quaterniond& GetDeltaQ() const { return dq; }

    std::vector<double> msgs;  // size() x 7
    Quaterniond dq;            // GyroIntegration's accumulator / the last pre-integration's dq
    mml_imu_preint pre{};      // the last PreIntegration
    bool has_pre = false;
};

// TryMAPInitialization (unionPoseEstimation.cpp:425-625) through mml_lio_initialize.  frameList: the reference's list
// (lidar poses P / Q, V, bg, ba, timeStamp); imu[i]: frame i's integrator (its messages; its `pre` when every frame after
// the first has one, else frame i's messages are pre-integrated with frame i-1's biases).  Both are changed the way the
// reference changes its list: on success the new V / biases, the pre-integrations redone with them, the list trimmed to
// SLIDEWINDOWSIZE and the back frame moved from lidar to body; nothing when the biases are too large; the partial writes
// of :589-598 when a velocity is.  GravityVector is written in every case, as the reference writes it before its checks.
inline bool TryMAPInitialization(std::list<Estimator::LidarFrame>& frameList, std::vector<IMUIntegrator>& imu,
                                 const Matrix4d& exTlb, Vector3d& GravityVector) {
    const int n = (int)frameList.size();
    if (n < 2 || (int)imu.size() != n) throw std::runtime_error("TryMAPInitialization: one IMUIntegrator per frame, >= 2 frames");
    std::vector<double> t(n), P(3 * (size_t)n), Q(4 * (size_t)n), V(3 * (size_t)n), bg(3 * (size_t)n), ba(3 * (size_t)n), smp;
    std::vector<int> offsets(1, 0);
    std::vector<mml_imu_preint> pre_in(n), pre_out(n);
    bool given = true;
    int i = 0;
    for (const auto& f : frameList) {
        t[i] = f.timeStamp;
        const double q[4] = {f.Q.x, f.Q.y, f.Q.z, f.Q.w};
        for (int k = 0; k < 3; ++k) {
            P[3 * i + k] = f.P.v[k];
            V[3 * i + k] = f.V.v[k];
            bg[3 * i + k] = f.bg.v[k];
            ba[3 * i + k] = f.ba.v[k];
        }
        for (int k = 0; k < 4; ++k) Q[4 * i + k] = q[k];
        smp.insert(smp.end(), imu[i].msgs.begin(), imu[i].msgs.end());
        offsets.push_back(offsets.back() + imu[i].size());
        if (i >= 1) {
            given = given && imu[i].has_pre;
            pre_in[i] = imu[i].pre;
        }
        ++i;
    }
    mml_lio_init_result res;
    check(nullptr,
          mml_lio_initialize(n, t.data(), P.data(), Q.data(), V.data(), bg.data(), ba.data(), smp.data(), offsets.data(), exTlb.m,
                             given ? pre_in.data() : nullptr, pre_out.data(), &res),
          "mml_lio_initialize");
    for (int k = 0; k < 3; ++k) GravityVector.v[k] = res.gravity[k];
    if (res.status == 1) return false;
    i = 0;
    for (auto& f : frameList) {  // V / bg / ba as written (all of them, or the partial state)
        for (int k = 0; k < 3; ++k) {
            f.V.v[k] = V[3 * i + k];
            f.bg.v[k] = bg[3 * i + k];
            f.ba.v[k] = ba[3 * i + k];
        }
        ++i;
    }
    if (res.status != 0) return false;
    for (int j = 1; j < n; ++j) {
        imu[j].pre = pre_out[j];
        imu[j].dq.x = pre_out[j].dq[0], imu[j].dq.y = pre_out[j].dq[1], imu[j].dq.z = pre_out[j].dq[2], imu[j].dq.w = pre_out[j].dq[3];
        imu[j].has_pre = true;
    }
    Estimator::LidarFrame& back = frameList.back();
    for (int k = 0; k < 3; ++k) back.P.v[k] = P[3 * (n - 1) + k];
    back.Q.x = Q[4 * (n - 1)], back.Q.y = Q[4 * (n - 1) + 1], back.Q.z = Q[4 * (n - 1) + 2], back.Q.w = Q[4 * (n - 1) + 3];
    for (int j = 0; j < res.keep_from; ++j) frameList.pop_front();  // WINDOWSIZE = SLIDEWINDOWSIZE (:611-614)
    imu.erase(imu.begin(), imu.begin() + res.keep_from);
    return true;
}

// TryMAPInitialization for many frame lists through ONE mml_lio_initialize_batch call: frameLists[s] / imus[s] / exTlbs[s] are
// one segment's arguments of the function above (2 .. MML_LIO_BATCH_MAX_FRAMES frames), each changed exactly as that function
// changes them; GravityVectors[s] is written in every case but status 3.  The call takes pre-integrations for all segments or
// for none: they are handed over when every frame after the first of EVERY segment has one.  ctx null: the host routine;
// otherwise one device call, bit-identical to it.  Returns per segment whether it initialised; a segment whose pre-integration
// covariance is not positive definite (status 3, e.g. an empty interval) is left untouched and does not throw.
inline std::vector<bool> TryMAPInitializationBatch(mml_ctx* ctx, std::vector<std::list<Estimator::LidarFrame>*>& frameLists,
                                                   std::vector<std::vector<IMUIntegrator>*>& imus, const std::vector<Matrix4d>& exTlbs,
                                                   std::vector<Vector3d>& GravityVectors) {
    const size_t ns = frameLists.size();
    if (imus.size() != ns || exTlbs.size() != ns) throw std::runtime_error("TryMAPInitializationBatch: one imu vector and one exTlb per frame list");
    std::vector<int> fo(1, 0), so(1, 0);
    std::vector<double> t, P, Q, V, bg, ba, smp, ex;
    std::vector<mml_imu_preint> pre_in;
    bool given = true;
    for (size_t s = 0; s < ns; ++s) {
        const int n = (int)frameLists[s]->size();
        if ((int)imus[s]->size() != n) throw std::runtime_error("TryMAPInitializationBatch: one IMUIntegrator per frame");
        int i = 0;
        for (const auto& f : *frameLists[s]) {
            const IMUIntegrator& it = (*imus[s])[i];
            t.push_back(f.timeStamp);
            for (int k = 0; k < 3; ++k) P.push_back(f.P.v[k]), V.push_back(f.V.v[k]), bg.push_back(f.bg.v[k]), ba.push_back(f.ba.v[k]);
            Q.push_back(f.Q.x), Q.push_back(f.Q.y), Q.push_back(f.Q.z), Q.push_back(f.Q.w);
            smp.insert(smp.end(), it.msgs.begin(), it.msgs.end());
            so.push_back(so.back() + it.size());
            if (i >= 1) given = given && it.has_pre;
            pre_in.push_back(it.pre);
            ++i;
        }
        fo.push_back(fo.back() + n);
        ex.insert(ex.end(), exTlbs[s].m, exTlbs[s].m + 16);
    }
    if (smp.empty()) smp.resize(7);
    std::vector<mml_imu_preint> pre_out(pre_in.size());
    std::vector<mml_lio_init_result> res(ns);
    check(ctx,
          mml_lio_initialize_batch(ctx, (int)ns, fo.data(), t.data(), P.data(), Q.data(), V.data(), bg.data(), ba.data(), smp.data(), so.data(),
                                   ex.data(), given ? pre_in.data() : nullptr, pre_out.data(), res.data()),
          "mml_lio_initialize_batch");
    GravityVectors.resize(ns);
    std::vector<bool> ok(ns, false);
    for (size_t s = 0; s < ns; ++s) {
        const mml_lio_init_result& r = res[s];
        if (r.status == 3) continue;
        for (int k = 0; k < 3; ++k) GravityVectors[s].v[k] = r.gravity[k];
        if (r.status == 1) continue;
        const int f0 = fo[s], n = fo[s + 1] - f0;
        int i = f0;
        for (auto& f : *frameLists[s]) {  // V / bg / ba as written (all of them, or the partial state)
            for (int k = 0; k < 3; ++k) f.V.v[k] = V[3 * i + k], f.bg.v[k] = bg[3 * i + k], f.ba.v[k] = ba[3 * i + k];
            ++i;
        }
        if (r.status != 0) continue;
        std::vector<IMUIntegrator>& imu = *imus[s];
        for (int j = 1; j < n; ++j) {
            const mml_imu_preint& p = pre_out[f0 + j];
            imu[j].pre = p;
            imu[j].dq.x = p.dq[0], imu[j].dq.y = p.dq[1], imu[j].dq.z = p.dq[2], imu[j].dq.w = p.dq[3];
            imu[j].has_pre = true;
        }
        Estimator::LidarFrame& back = frameLists[s]->back();
        const int b = f0 + n - 1;
        for (int k = 0; k < 3; ++k) back.P.v[k] = P[3 * b + k];
        back.Q.x = Q[4 * b], back.Q.y = Q[4 * b + 1], back.Q.z = Q[4 * b + 2], back.Q.w = Q[4 * b + 3];
        for (int j = 0; j < r.keep_from; ++j) frameLists[s]->pop_front();
        imu.erase(imu.begin(), imu.begin() + r.keep_from);
        ok[s] = true;
    }
    return ok;
}

}  // namespace mml
#endif
