// mml_internal.h -- private definitions shared by the HIP translation units of libmmloam_hip.so.
// gfx950 (MI355X) only.  All device code is compiled with -ffp-contract=off: the reference arithmetic
// is x86-64 SSE2 without FMA and the parity tests are bit-exact on float paths.
#ifndef MML_INTERNAL_H
#define MML_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mml_mem.h"
#include "pose_block.h"
#include "mmloam_hip.h"

#define MML_WAVE 64

namespace mml_und {
// A double literal as a scalar-register operand.  gfx950 has no 64-bit literal in VOP3: left alone the compiler materialises
// each constant of a polynomial with two v_mov_b32 next to its FMA (three vector instructions per term in kernels that are
// bound by vector issue); from an SGPR pair the term is ONE v_fma_f64 and the two s_mov_b32 go to the scalar unit.
__device__ __forceinline__ double sconst(double v) {
    asm("" : "+s"(v));
    return v;
}
}  // namespace mml_und
// One-pass bucketing (feature.hip k_assign_onepass): a scan line is stored as up to MML_SEG_MAX segments, one per MML_OP_BLK-point
// block of the raw scan; MML_SEG_FLAT bounds (blocks x lines) of one sensor.
#define MML_SEG_MAX 16
#define MML_OP_BLK 4096
#define MML_SEG_FLAT 512
#define MML_VOXEL_LDS_CAP 8192  // labelled points per (slot, kind) that k_voxel sorts in LDS; more go the global-sort way

// ---- factor records kept on the device (SoA would save little: every field is read once per GN pass) ----
struct MmlLineFactor {   // Estimator.h:59-84 FeatureLine (values are floats in the reference, :256-271)
    float ori[3];
    float p1[3];
    float p2[3];
    int src;             // feature index, -1 = no factor for this feature
    double error;        // FeatureLine::ComputeError
};
struct MmlPlaneFactor {  // Estimator.h:105-122 FeaturePlanVec with sqrt_info replaced by omega
    float ori[3];
    float omega[3];
    double proj[3];
    double error;
    int src;
    int _pad;
};

struct MmlGrid {         // radix-sorted uniform grid over one map cloud (replaces pcl::KdTreeFLANN)
    float4* pts = nullptr;      // sorted by cell key: x, y, z, original index (bit pattern)
    int* cell_start = nullptr;  // ncell + 1
    uint16_t* tags = nullptr;   // optional: cube index of every sorted point (global map), else nullptr
    int m = 0;
    float origin[3] = {0.f, 0.f, 0.f};
    float cell = 1.f;
    float inv_cell = 1.f;
    int dim[3] = {1, 1, 1};
    int ncell = 1;
};

// The global cube map of one Estimator (a12 + map_global.hip), in two parts, both held by the Estimator's MmlMapState below; the
// scratch the upkeep works in (bank_cube, the sort buffers) is the context's.
// The MATCH COPY: what Estimate() matches against -- tagged grids over the concatenated cube clouds, the unsorted clouds with
// their tags, the 4851 cube counts, laserCloudCen*_last.  Sized by need (mml_cube_match_ensure).
struct MmlCubeMatch {
    MmlGrid ggrid[2];
    bool have_gmap[2] = {false, false};
    float4* gmap_orig[2] = {nullptr, nullptr};
    uint16_t* gtag_orig[2] = {nullptr, nullptr};
    int* cube_cnt[2] = {nullptr, nullptr};  // 4851 ints each
    MmlGroup ggrid_mem[2];                  // owns ggrid[k].pts / cell_start / tags, gmap_orig[k], gtag_orig[k], cube_cnt[k]
    int gmap_cap[2] = {0, 0};               // points the group of a kind is sized for
    int cen[3] = {10, 5, 10};               // laserCloudCen{Width,Height,Depth}_last (Map_Manager.h:113-115)
    void release() {
        for (auto& g : ggrid_mem) g.release();
        for (int k = 0; k < 2; ++k) {
            ggrid[k] = MmlGrid();
            have_gmap[k] = false;
            gmap_orig[k] = nullptr;
            gtag_orig[k] = nullptr;
            cube_cnt[k] = nullptr;
            gmap_cap[k] = 0;
        }
    }
};
// The LIVE STORE (MAP_MANAGER's cubes): points + cube tags, the ping-pong pair of the compaction, the pending world-frame
// features (laserCloud{Corner,Surf}_to_map), the live centre.  72 bytes per point of max_map_points plus 2 x 16 x max_features x
// 16 bytes of pending clouds, allocated by the first append / increment.
struct MmlCubeLive {
    float4* gs_pts[2] = {nullptr, nullptr};
    uint16_t* gs_tag[2] = {nullptr, nullptr};
    float4* gs_pts2[2] = {nullptr, nullptr};   // ping-pong for compaction
    uint16_t* gs_tag2[2] = {nullptr, nullptr};
    int gs_n[2] = {0, 0};
    float4* gp_pts[2] = {nullptr, nullptr};    // laserCloud{Corner,Surf}_to_map
    int gp_n[2] = {0, 0};
    int gp_cap = 0;
    int gs_cen[3] = {10, 5, 10};               // laserCloudCen{Width,Height,Depth} of the live store
    MmlGroup mem;                              // owns gs_pts .. gp_pts
};

// The maps of one Estimator: the local map -- the two grids with their unsorted clouds, the key-scan ring with its counts,
// localMapID, the two map sizes -- and the global cube map (cmatch / clive).  The context holds one of its own (mml_ctx::own) and
// every map bank one more (mml_map_banks_create); all code that works on "a map" takes this struct (mml_map_at).  Only the grids'
// arrays exist from the start (mml_map_local_alloc): the ring comes with the first increment, the live store with the first
// append / increment, the match copy is sized by need.  As defined here a state is the context's own, whose two kinds are unset
// until mml_map_set_local; a bank is created set and empty.
#define MML_LOCAL_WINDOW 50  // localMapWindowSize, Estimator.h:326
struct MmlMapState {
    int name = -1;                           // what a message calls it: the bank, -1 the context's own
    MmlCubeMatch cmatch;
    MmlCubeLive clive;
    MmlGrid grid[2];
    bool have_map[2] = {false, false};
    float4* map_tmp = nullptr;               // 2 x MM: the unsorted clouds
    MmlGroup grid_mem;                       // owns grid[k].pts / cell_start and map_tmp
    float4* ring[2] = {nullptr, nullptr};    // MML_LOCAL_WINDOW x MF each
    MmlGroup ring_mem;                       // owns ring[2]
    int ring_n[2][MML_LOCAL_WINDOW] = {};
    long local_map_id = 0;                   // localMapID
    int local_map_n[2] = {0, 0};
    void release() {
        grid_mem.release();
        ring_mem.release();
        cmatch.release();
        clive.mem.release();
    }
};
// What the association kernels read of one local map of one kind: a row of the device-resident table of a context with banks.
struct alignas(16) MmlMapDesc {
    MmlGrid g;
    const float4* orig;  // the unsorted cloud (index = original index)
};
static_assert(sizeof(MmlMapDesc) % 16 == 0 && sizeof(MmlMapDesc) / 4 <= 32, "a descriptor is read as dwords, at most 32");
// What they read of one global cube map of one kind: a row of the second table, beside the first.  The grid comes first, as in
// MmlMapDesc: a far query picks the row of its stage and reads the grid from either.  Entry 0 (the context's own map) always has
// have_g = 0: a bound slot and the context's own cube map exclude each other, so a banked launch never reads it.
struct alignas(16) MmlCubeDesc {
    MmlGrid g;            // the tagged grid
    const float4* orig;   // the unsorted cloud
    const int* cube_cnt;  // 4851 counts
    int have_g;
    int cen[3];           // the ENTRY's centre (the same in both rows of an entry)
};
static_assert(sizeof(MmlCubeDesc) % 16 == 0 && sizeof(MmlCubeDesc) / 4 <= 32, "a descriptor is read as dwords, at most 32");
static_assert(offsetof(MmlCubeDesc, g) == 0 && offsetof(MmlMapDesc, g) == 0, "the grid leads both rows");
struct MmlBanks {
    std::vector<MmlMapState> bank;    // sized once by mml_map_banks_create: pointers into it hold until mml_map_banks_destroy
    std::vector<int> slot_bank;       // B: bank of every slot, -1 = the context's own map
    int n_bound = 0;                  // slots with a bank
    MmlMapDesc* d_table = nullptr;    // (banks + 1) x 2 kinds; row 0: the context's own map
    MmlCubeDesc* d_cube_table = nullptr;  // the same rows for the cube maps
    int* d_slot_bank = nullptr;       // B
    MmlGroup tab_mem;                 // owns the three
    bool dirty = true;                // a grid, a match copy or a binding changed since the device copies were written (mml_assoc_ready)
    void release() {
        for (MmlMapState& b : bank) b.release();
        bank.clear();
        slot_bank.clear();
        tab_mem.release();
        d_table = nullptr;
        d_cube_table = nullptr;
        d_slot_bank = nullptr;
        n_bound = 0;
        dirty = true;
    }
};

struct MmlStageTimer {
    std::string name;
    double total_ms = 0;
    long launches = 0;
};

struct MmlComm;   // comm.hip: RCCL communicator + window-solve buffers
// the side calls' scratch structs, each defined in its own file and kept in mml_ctx::side (mml_side below); mml_destroy releases
// them in this order
enum MmlSideId {
    MML_SIDE_FULLWINDOW,   // fullwindow_dev.hip MmlFwDev: parameter / scratch buffers of the device-resident full-window solve
    MML_SIDE_PREINT,       // imu_preint.hip MmlPreintDev: buffers of mml_imu_preintegrate_batch
    MML_SIDE_LIO,          // lio_init_batch.hip MmlLioDev: the block of mml_lio_initialize_batch
    MML_SIDE_GICP,         // gicp.hip MmlGicpDev: the blocks of the GICP alignments (single and batch calls)
    MML_SIDE_TIME_OFFSET,  // time_offset.hip MmlTofsDev: the blocks of the time-offset searches (single and batch calls)
    MML_SIDE_UNION,        // livox_stream.hip MmlUnionDev: the staging blocks of mml_union_assemble
    MML_SIDE_VELO_FOV,     // velo_fov.hip MmlVfovDev: the blocks of the Velodyne FOV selection (single and batch calls)
    MML_SIDE_CALIB,        // calibrate.hip MmlCalibDev: the blocks of mml_cloud_crop_voxel / mml_aligner_calibrate
    MML_SIDE_FEATURE_CLOUDS,  // capi.hip MmlFeatCloudsDev: the table block of mml_feature_clouds_download_batch
    MML_SIDE_IMU_FETCH,    // imu_stream.hip MmlImuFetchDev: the block of mml_imu_fetch_batch / mml_imu_predict_batch
    MML_SIDE_POSE_INGEST,  // pose_ingest.hip MmlPoseIngestDev: the table block of mml_pose_ingest_batch
    MML_SIDE_WM_SCORE,     // world_map_score.hip MmlWmScoreDev: the hypotheses and results of mml_world_map_score
    MML_SIDE_COUNT
};

struct mml_ctx {
    mml_config cfg;
    MmlComm* comm = nullptr;
    MmlSides<MML_SIDE_COUNT> side;
    // frame-parallel window solve (solve.hip): one state machine copy, 4 counters and two record buffers per slot
    void* wstate = nullptr;
    double* wrec = nullptr;
    double* waux = nullptr;
    MmlGroup win_state;  // owns the three, allocated by the first such solve
    struct WinGraph {  // captured launch chain of one frame-parallel window solve
        int first, count, W, max_iters, fixed;
        double huber, w_tan;
        hipStream_t stream;
        const double* Tbl;
        bool second;
        hipGraphExec_t exec;
    };
    std::vector<WinGraph> win_graphs;
    int device = 0;
    // launch settings, read once by mml_create (capi.hip read_settings): the device's CU count and the environment switches
    int cus = 0;                 // multiProcessorCount of `device`
    bool onepass_wanted = true;  // $MML_ASSIGN_ONEPASS=0: false (mml_feature_init still decides `onepass` from the layout)
    bool solve_wide = true;      // $MML_SOLVE_WIDE=0: false, the live path's one-frame solve through k_solve<true>
    bool use_graph = true;       // $MML_NO_GRAPH: false, the window solve's chain launched kernel by kernel
    bool lazy_undistort = true;  // $MML_LAZY_UNDISTORT=0: false, mml_step undistorts the whole cloud itself (see und_pending)
    // `lanes`: independent HIP streams.  Entry points enqueue on lane `cur` (0 unless mml_step is pipelining
    // sub-batches); per-call scratch is sliced by slot index so lanes never share a byte.
    static constexpr int MAX_LANES = 8;
    hipStream_t streams[MAX_LANES] = {};
    // mml_scan_upload_batch copies on its own stream, so that the copy of one slot range runs under the kernels of
    // another; an entry point that touches a slot range first makes the lanes wait for the uploads still in flight on it
    hipStream_t copy_stream = nullptr;
    hipEvent_t lane_mark[MAX_LANES] = {};
    struct Upload {
        int first, count;
        hipEvent_t done;
    };
    std::vector<Upload> uploads;
    std::vector<hipEvent_t> upload_event_pool;
    int n_lanes = 1;
    int cur = 0;
    int far_lanes = 1;  // lanes whose far-query counters the last top-level association wrote (mml_associate_far_count)
    std::string err;
    MmlFixed fixed;  // owns every buffer below that mml_create allocates (the plain pointers without an owner named beside them)

    int B = 0, NV = 0, NL = 0, NT = 0, L = 0, MF = 0;

    // inputs
    float4* velo_in = nullptr;            // B * NV
    mml_livox_point* livox_in = nullptr;  // B * NL
    int* d_n_in = nullptr;                // B * 2 (velo, livox)
    std::vector<int> h_n_in;
    std::vector<char> stats_stale;        // B: 1 while assoc_stats of the slot do not describe its current factors (mml_ensure_assoc_stats)
    std::vector<char> raw_extracted;      // B: 1 while the slot's raw buffers are the ones its extracted state was made from

    // per raw point scratch
    uint8_t* raw_line = nullptr;  // B * NT   line id or 255
    float* raw_ori = nullptr;     // B * NV   -atan2(y,x) as float

    // line-bucketed points
    float4* ln_pts = nullptr;   // B * NT
    int* ln_gidx = nullptr;     // B * NT  fused index of the point: >= 0 kept, -1 dropped, -2 Livox beyond far_th
    int* ln_rel = nullptr;      // B * NT  bits of its in-sweep time, normal_x (two 4-byte arrays: the undistortion reads the time only, the
                                //         label pass the index only; as one 8-byte record each of them fetched both)
    int* line_start = nullptr;  // B * L   start of the line in LINE ORDER (the index space of ln_curv / ln_refl / ln_attr)
    int* line_len = nullptr;    // B * L
    // where the points of a line are STORED (ln_pts / ln_gidx / ln_rel / ln_label): segment s of a line covers its line indices
    // [seg_cum[s], seg_cum[s + 1]) at storage positions seg_pos[s] ...  (three-pass bucketing: one segment, = line_start)
    int* seg_cum = nullptr;     // B * L * (MML_SEG_MAX + 1)
    int* seg_pos = nullptr;     // B * L * MML_SEG_MAX
    int* seg_n = nullptr;       // B * L
    int* seg_flat = nullptr;    // B * 2 * MML_SEG_FLAT: the segment starts of a sensor's region in storage order (block-major)
    int* seg_flat_n = nullptr;  // B * 2 * 2: entries | lines per block
    // per 64 line indices the one segment boundary they may cross and the storage offsets on either side (k_seg_records):
    // seg_rs for the rounds of k_stencil's tiles (indices 64 r - 5 ...), seg_rw for aligned windows (64 w ...); record
    // (line, r) sits at  slot * seg_rstride + (line_start[line] >> 6) + 6 * line + r
    int4* seg_rs = nullptr;
    int4* seg_rw = nullptr;
    int seg_rstride = 0;
    unsigned long long* op_agg = nullptr;  // B * 2 * MML_SEG_MAX: block aggregates of the one-pass bucketing (epoch-tagged)
    unsigned op_epoch = 0;
    bool onepass = false;       // the ring layout takes the one-pass bucketing
    float* ln_curv = nullptr;
    float* ln_refl = nullptr;
    uint16_t* ln_attr = nullptr;
    int* crop_cnt = nullptr;     // crop pass block counts (8 ints per block)
    int* blk_cnt = nullptr;      // assign pass histograms
    int* assign_aux = nullptr;   // 8 ints per slot
    unsigned* sel_scratch = nullptr;  // 4 x B*NT unsigned: k_select scratch for lines beyond the LDS budget
    int sel_cap = 0;
    int sel_cap_velo = 0;
    unsigned* brk_queue = nullptr;  // B * NT: queued break-point candidates of k_stencil
    int* brk_cnt = nullptr;         // 2 B: break-point queue sizes, then redo queue sizes
    int* queue_off = nullptr;       // 2 (B + MAX_LANES + 1): per launch the offsets of the slots' redo / break-point queues in their concatenation
    unsigned* redo_queue = nullptr; // B * NT: points k_stencil left to k_stencil_redo
    uint8_t* sel_done = nullptr;       // B * L: lines finished by k_select_part
    int* sel_list = nullptr;           // 2 * B * L * 2 ints: (slot, line) lists of the lines left to k_select (rings | Livox lines)
    int* sel_list_cnt = nullptr;       // 2 B ints
    unsigned char* st_exit = nullptr;  // B * (NT / 256 + L + 8): k_stencil segment mode, exit offsets of the stride walk per tile
    int* vx_big = nullptr;             // 2 B: per launch (indexed by its first slot) the slots k_voxel<512> left to the large form: count | list

    // combined (pre-crop) cloud, velo part at [0, NV), livox part at [NV, NT)
    int* cb_n = nullptr;  // B * 2

    // The fused cropped cloud [velo_combine ; livox_combine] has no storage of its own: a kept point lives at its
    // line-bucketed position (ln_pts, undistorted in place) and ln_gidx says where it sits in the fused order; that order
    // is materialised only at the API boundary (downloads) and as the tie-break of the voxel sort.
    uint8_t* ln_line = nullptr;   // B * NT  ring / Livox line (normal_y) of an UPLOADED cloud (an extracted one has its line table)
    int* slot_flags = nullptr;    // B * 2   [0] bit 0: filled by mml_cloud_upload, bit 1: undistorted (in-sweep time reads 1);
                                  //         [1] bit 1 as it was when the current mml_undistort started
    // INVARIANT (partly undistorted slots).  mml_step undistorts only the points on the slot's two label lists -- all its
    // down-sampler reads -- and sets und_pending[slot] = 1.  While that byte is set: slot_flags, d_und and d_und_par describe the
    // sweep motion as after a whole mml_undistort, the LISTED points of ln_pts are final, every other point of ln_pts still holds its
    // raw coordinates, and the label lists (vx_keys, fu_info[6..7]) are those of the cloud.  mml_cloud_settle(first, count) finishes
    // the other points and clears the byte; every entry point that reads or rewrites ln_pts / ln_rel / ln_label outside the step
    // calls it first.  What replaces the cloud (mml_launch_extract, mml_cloud_upload) just clears the byte.
    std::vector<char> und_pending;  // B
    uint8_t* ln_label = nullptr;  // B * NT  0 none / 1 corner / 2 surf (normal_z) for kept points; 0x81 / 0x82 for labelled Livox
                                  //         points beyond far_th (counted in livox_*_num and aligned by the GICP refresh, not fused)
                                  //         (bit 6, MML_LABEL_SETTLED, lives only inside mml_cloud_settle: "this point is done")
    int* fu_info = nullptr;  // B * 8: n_points, n_velo, vc, vs, lc, ls, fused corner, fused surf

    // down-sampled feature stacks: kind 0 corner, 1 surf
    float4* ft_xyz[2] = {nullptr, nullptr};  // B * MF
    int* ft_n = nullptr;                     // 2 * B
    unsigned long long* vx_keys = nullptr;   // voxel sort scratch: B * 2 * VX_CAP
    int* vx_gidx = nullptr;                  // B * 2 * VX_CAP: the fused index of every listed point (label_append), parallel to the lists in vx_keys
    // batched global-sort down-sampler (map_upkeep.hip mml_downsample_big), allocated on first use
    unsigned long long* seg_keys = nullptr;
    unsigned* seg_vals = nullptr;
    float4* seg_cat = nullptr;
    int* seg_flag = nullptr;
    int* seg_meta = nullptr;
    MmlGroup seg_scratch;                    // owns the five
    MmlStaging<char, false> seg_tmp[8];      // rocPRIM temporary storage per stream lane (lanes run concurrently: no sharing)
    int VX_CAP = 0;                          // label-list stride per (slot, kind) = NT: every labelled point is listed

    // factors
    MmlLineFactor* lf = nullptr;   // B * MF
    MmlPlaneFactor* pf = nullptr;  // B * MF
    int* work_off = nullptr;       // 2 * B + 1 chunk offsets for k_associate
    float* hard_knn = nullptr;     // 10 floats per queued feature
    int4* hard_list = nullptr;     // B * MF * 2 queued (slot, kind, feature) triples
    double* assoc_stats = nullptr; // B * 16: n_line, n_plane, n_line_used, n_plane_used, gram[9], ...

    // maps: the context's own (what an unbound slot is matched against) and the banks'
    MmlMapState own;
    static constexpr int LOCAL_WINDOW = MML_LOCAL_WINDOW;
    MmlStaging<char, false> wire_stage;      // raw message bytes on their way in / out (one call at a time; grows to the largest)
    MmlBanks banks;                    // map banks (map_banks.hip): further maps, and which slot is matched against which
    // scratch of the local-map increment (map_upkeep.hip mml_map_upkeep_increment_segmented), of the own map's as of the banks':
    // sized by the ring points of the largest chunk of maps a call has worked on, 48 bytes per point
    struct BankInc {
        float4* cat = nullptr;               // the chunk's rings, concatenated
        unsigned long long* keys = nullptr;  // 2 x cap: sort keys in / out
        unsigned* vals = nullptr;            // 2 x cap
        int* flag = nullptr;                 // 2 x (cap + 1): run heads, positions
        size_t cap = 0;                      // points
        MmlGroup mem;                        // owns the four
        MmlStaging<char> tab;                // a chunk's tables and read-backs: device block and pinned twin
        long budget = MML_BANK_INCREMENT_BUDGET;  // ring points per chunk (mml_debug_bank_increment_budget)
    } bank_inc;
    // scratch of the cube stores' upkeep (map_global.hip), of the own store's as of the banks' (one increment runs at a time), a group
    // of its own: sized by the points (store + pending, both kinds) and the segments of the largest chunk of stores a call has
    // worked on -- 60 bytes per point, 8 x 4851 ints per segment
    struct BankCube {
        int* work = nullptr;                 // seg_cap x (cnt | changed | six box keys per cube)
        int* flags = nullptr;                // 4 x (cap + 1): keep, keep_pos, sel, sel_pos (run heads and positions after the scatter)
        unsigned long long* keys = nullptr;  // 2 x cap: sort keys in / out
        unsigned* vals = nullptr;            // 2 x cap
        float4* sel_pts = nullptr;           // cap: the selected rows
        uint16_t* tags = nullptr;            // 2 x cap: every row's cube | the selected rows' cubes
        size_t cap = 0;                      // points
        int seg_cap = 0;                     // segments
        MmlGroup mem;                        // owns the six
        MmlStaging<char> tab;                // a chunk's tables and read-backs: device block and pinned twin
        long budget = MML_BANK_GLOBAL_INCREMENT_BUDGET;  // points per chunk (mml_debug_bank_global_increment_budget)
    } bank_cube;
    // the world map (world_map.hip, mml_world_map_*): one open-addressing table of voxels for n maps, a group of its own.
    // 28 bytes per table position (key, float4 sum, count), 2 .. 4 positions per voxel of capacity; a surfel map (MML_WM_SURFELS)
    // holds three float4 of moments per position more, 76 bytes.  The add chain's scratch is 52 bytes per point of the call's bound
    // (count x NT), grow-only, for both kinds, beside rocPRIM's temporary storage and the call's table block (a surfel map: 16
    // bytes per slot more, the sensor origins)
    struct WorldMap {
        int n_maps = 0;                      // 0: no world map
        bool surfels = false;                // MML_WM_SURFELS: mom[] allocated
        float4* mom[3] = {nullptr, nullptr, nullptr};  // slots each: (sdx sdy sdz vx) (sxx sxy sxz vy) (syy syz szz vz), world_map_key.h
        float leaf = 0.f;
        long capacity = 0;                   // voxels, all maps together
        unsigned long long slots = 0;        // table positions: the next power of two >= 2 x capacity
        unsigned long long* keys = nullptr;  // slots: world_map_key.h keys, MML_WM_EMPTY where free
        float4* sum = nullptr;               // slots: x, y, z, intensity
        int* count = nullptr;                // slots
        int* map_n = nullptr;                // n_maps + 1: voxels per map, then the total
        MmlGroup mem;                        // owns the four, mom[] of a surfel map and, once a call has scored, the cache
        float4* cache = nullptr;             // slots: (nx, ny, nz, planarity) of every position's surfel, 16 bytes per position more;
                                             //        allocated by the first mml_world_map_score (world_map.hip mml_wm_cache_ready)
        unsigned long long version = 0;      // advanced on the host by every call that writes the table (world_map.hip wm_touch)
        unsigned long long cache_version = 0;  // the version the cache was filled from; behind `version`: stale
        MmlStaging<char, false> scratch;     // the calls' scratch (one call at a time)
        MmlStaging<char, false> tmp;         // rocPRIM temporary storage
        MmlStaging<char> tab;                // a call's slot rows and counters: device block and pinned twin
        MmlStaging<int, false> assoc_maps;   // B: the map of every slot of the last association against the map (world_map_assoc.hip)
        void release() {
            mem.release();
            scratch.release();
            tmp.release();
            tab.release();
            assoc_maps.release();
            keys = nullptr;
            sum = nullptr;
            count = nullptr;
            map_n = nullptr;
            mom[0] = mom[1] = mom[2] = nullptr;
            cache = nullptr;
            ++version;
            surfels = false;
            n_maps = 0;
        }
    } world;
    unsigned* map_keys = nullptr;
    unsigned* map_keys2 = nullptr;
    unsigned* map_vals = nullptr;
    unsigned* map_vals2 = nullptr;
    MmlStaging<char> grid_tab;         // the one-cloud grid build's table (mml_grid_table_bytes(1)): device block and pinned twin
    MmlStaging<char, false> sort_tmp;  // rocPRIM temporary storage of the map builds and filters (voxel_sort_dev.h)
    int MM = 0;

    // solver state
    double* d_x = nullptr;        // B * 6
    double* d_pose_in = nullptr;  // B * kPoseSlotDoubles: the calls' parameter blocks, a call owning its slots' range (pose calls: PoseBlock)
    double* d_result = nullptr;      // B * MML_SOLVE_RESULT: k_solve's result records (pose, stack sizes, association statistics) for small calls
    double* d_summ = nullptr;     // B * 8
    double* d_trace = nullptr;    // B * 6 * MAX_ITERS
    double* d_und = nullptr;      // B * 8 per-scan undistortion constants
    double* d_und_par = nullptr;  // B * 12 the sweep motion (dR, dt) of the slot's last undistortion: k_undistort_prep's copy of the call's
                                  //        parameters, which live in d_pose_in only until the next stage overwrites them
    double* d_rec = nullptr;      // B * 32
    float* d_extr = nullptr;      // 16 floats
    int* d_misc = nullptr;        // misc ints

    // pinned host staging
    double* h_stage = nullptr;
    size_t h_stage_doubles = 0;
    size_t stage_cursor = 0;

    // profiling
    bool profiling = false;
    std::vector<MmlStageTimer> stages;
    struct Pending {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;

    // every owner declared above, for mml_destroy: a new one is added here, next to its declaration
    void release_memory() {
        win_state.release();
        seg_scratch.release();
        for (auto& t : seg_tmp) t.release();
        own.release();
        banks.release();
        bank_inc.mem.release();
        bank_inc.tab.release();
        bank_cube.mem.release();
        bank_cube.tab.release();
        world.release();
        wire_stage.release();
        grid_tab.release();
        sort_tmp.release();
        fixed.release();
    }
};

#define MML_STREAM(ctx) ((ctx)->streams[(ctx)->cur])
int mml_sync_all(mml_ctx* ctx);
// For a call that reads no slot and wants an idle device: selects the context's device, ends everything the context has in
// flight -- every lane of a pipelined mml_step and the upload stream -- and makes lane 0 the current one.  capi.hip.
int mml_enter_idle(mml_ctx* ctx);
// the scratch struct D of side call `id`, created on first use
template <class D>
D* mml_side(mml_ctx* ctx, MmlSideId id) {
    return ctx->side.get<D>(id);
}
double* mml_stage_alloc(mml_ctx* ctx, size_t doubles);  // pinned staging ring (capi.hip): small read-backs land here
int mml_uploads_wait(mml_ctx* ctx, int first, int count);

#define MML_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return MML_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define MML_REQUIRE(cond, code, msg) \
    do {                             \
        if (!(cond)) {               \
            ctx->err = (msg);        \
            return (code);           \
        }                            \
    } while (0)

// A refusal with a formatted message: the text goes to ctx->err when there is a context to carry it (at most 191 characters),
// `code` comes back.  capi.hip.
int mml_refuse(mml_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

// profiling bracket (no-op unless enabled)
int mml_stage_begin(mml_ctx* ctx, const char* name);
void mml_stage_end(mml_ctx* ctx, int token);
struct MmlStageScope {
    mml_ctx* c;
    int t;
    MmlStageScope(mml_ctx* ctx, const char* name) : c(ctx), t(mml_stage_begin(ctx, name)) {}
    ~MmlStageScope() { mml_stage_end(c, t); }
};

// launchers implemented in the .hip files (all asynchronous on ctx->stream)
int mml_launch_extract(mml_ctx* ctx, int first, int count, bool have_extrinsic);
int mml_launch_cloud_decode(mml_ctx* ctx, int slot, const float* d_raw, int n, int n_velo);
// the second half of mml_launch_cloud_decode for `count` slots that a decode kernel has filled: ONE k_crop launch, a workgroup per slot
int mml_launch_cloud_lists(mml_ctx* ctx, int first, int count);
// where the two point counts k_crop reads sit in a slot's 8 ints of assign_aux (feature.hip AssignAux, asserted there)
#define MML_AUX_INTS 8
#define MML_AUX_KEPT_VELO 3
#define MML_AUX_KEPT_LIVOX 6
int mml_launch_undistort(mml_ctx* ctx, int first, int count, const double* d_params);
// mml_step's form: the points on the slots' label lists only; the slots become partly undistorted (mml_ctx::und_pending)
int mml_launch_undistort_listed(mml_ctx* ctx, int first, int count, const double* d_params);
// finishes the partly undistorted slots of [first, first + count) on the current stream (a host loop over B bytes when none is)
int mml_cloud_settle(mml_ctx* ctx, int first, int count);
#define MML_LABEL_SETTLED 0x40  // no label value uses it: 0, 1, 2, 0x81, 0x82
int mml_launch_downsample(mml_ctx* ctx, int first, int count);
// labelled corner points per (slot, kind) that the LDS sort of k_voxel takes (surf: MML_VOXEL_LDS_CAP)
inline int mml_voxel_cap_corner(const mml_ctx* ctx) { return (ctx->NT > 65536 || MML_VOXEL_LDS_CAP < 2048) ? MML_VOXEL_LDS_CAP : 2048; }
// The maps of bank `bank`, -1: the context's own.
inline MmlMapState& mml_map_at(mml_ctx* ctx, int bank) { return bank < 0 ? ctx->own : ctx->banks.bank[(size_t)bank]; }
// map_banks.hip: the arrays every local map has from the start -- grid[k].pts, grid[k].cell_start, map_tmp -- for the own map
// (mml_create) as for a bank
int mml_map_local_alloc(mml_ctx* ctx, MmlMapState& map);
// map_assoc.hip, the one-cloud grid build: kind `kind` of the map's local map from m host points (null: the cloud is in the map's
// map_tmp + kind * MM already, the map broadcast of comm.hip).  The scratch it uses (the sort buffers) is the context's.
int mml_build_grid(mml_ctx* ctx, MmlMapState& map, int kind, const float* h_xyz, int m);
// map_banks.hip.  mml_assoc_ready: the state checks of a call that associates slots [first, first + count) -- an unbound slot needs
// the context's two maps (`who` before both maps were set), a bound one that the context's OWN global cube map is unset -- and the
// device copies of the two descriptor tables and the bindings brought up to date (a drained context and small copies, only after
// a change).
int mml_assoc_ready(mml_ctx* ctx, int first, int count, const char* who);
inline bool mml_any_bound(const mml_ctx* ctx, int first, int count) {
    if (!ctx->banks.n_bound) return false;
    for (int i = 0; i < count; ++i)
        if (ctx->banks.slot_bank[(size_t)first + i] >= 0) return true;
    return false;
}
// gicp.hip: mml_gicp_align_opts on clouds that are on the device already, for a caller that has made the context idle
int mml_gicp_align_device(mml_ctx* ctx, const char* who, const float4* d_src, int n_src, const float4* d_tgt, int n_tgt,
                          const mml_gicp_opts* opts, float* T_inout, int* converged, mml_gicp_info* info);
int mml_downsample_big(mml_ctx* ctx, int first, int count);
int mml_downsample_redo_overflow(mml_ctx* ctx, int first, int count, std::vector<int>* redone);
// Estimator::MapIncrementLocal (map_upkeep.hip): map `map` grows by the two stacks of `slot` at T_wl (16 doubles, row-major).
struct MmlMapIncrement {
    MmlMapState* map;
    int slot;
    const double* T_wl;
};
// n distinct maps in one chain of launches (one map: n = 1, its two kinds two segments); the caller has checked the arguments
// and drained the context.  Checks every slot's stack before a map changes: all or nothing.
int mml_map_upkeep_increment_segmented(mml_ctx* ctx, int n, const MmlMapIncrement* inc, int* n_corner, int* n_surf);
// map_assoc.hip, the grid build: nseg clouds that are on the device, one sort and one read-back per refinement round for all of
// them.  A job: the grid to fill (its pts / cell_start / tags are the destination), the unsorted cloud, the configured cell edge,
// the cloud's size, its bounding box as six keys (MML_BBOX_EMPTY where m = 0), and the points' tags in the cloud's order (null: the
// cloud has none).  Key: unsigned long long (segment << 32 | cell) for any nseg, unsigned (the cell alone) for nseg = 1.
struct MmlGridJob {
    MmlGrid* g;
    const float4* orig;
    float cell;
    int m;
    const int* bbox_keys;
    const uint16_t* tag_orig;
};
template <class Key>
struct MmlGridScratch {
    Key *keys, *keys2;    // cap each
    unsigned *vals, *vals2;
    size_t cap;           // points
    void *tab_d, *tab_h;  // mml_grid_table_bytes(nseg) on the device and pinned
};
size_t mml_grid_table_bytes(int nseg);
template <class Key>
int mml_build_grids(mml_ctx* ctx, int nseg, const MmlGridJob* jobs, const MmlGridScratch<Key>& W, int* rounds);
// the match copy of the map's cube map set from host points (map_assoc.hip); the caller has checked the arguments -- the cube indices
// too -- and drained the context
int mml_build_global_grid(mml_ctx* ctx, MmlMapState& map, int kind, const float* h_xyz, const int* h_cube, int m, const int* cen);
// The one capacity rule of a match copy: room for m points of `kind` (at least 1024; the cube counts move with the rest, every
// builder rewrites them).  A copy that has to grow is replaced, so the caller waits for work in flight first -- once per call,
// when mml_cube_match_fits says no.
inline bool mml_cube_match_fits(const MmlCubeMatch& G, int kind, int m) { return m <= G.gmap_cap[kind] && G.ggrid_mem[kind].present(); }
int mml_cube_match_ensure(mml_ctx* ctx, MmlCubeMatch& G, int kind, int m);
int mml_cube_store_download(mml_ctx* ctx, const MmlMapState& map, int kind, float* xyz, int* cube_idx, int capacity, int* n, int* cen);
int mml_cube_store_reset(mml_ctx* ctx, MmlMapState& map);
int mml_cube_store_ensure(mml_ctx* ctx, MmlMapState& map);  // the store's own memory, on first use
// The upkeep (map_global.hip): the stores of n DISTINCT maps in one chain of launches; the caller has checked the arguments and
// drained the context.  A message names a bank's store by the map's name, the context's own by no prefix.  Every refusal leaves
// all n stores -- live arrays, tags, centres, pending clouds, match copies -- as they were.
int mml_cube_store_increment_segmented(mml_ctx* ctx, int n, MmlMapState* const* maps, const double* T_wl, int* n_corner, int* n_surf);
int mml_cube_store_append_segmented(mml_ctx* ctx, int n, MmlMapState* const* maps, const int* slots, const double* T_wl);
// The chunks of such a call: chunk c = stores [cut[c], cut[c + 1]) -- greedy, in call order, at most `budget` points (pts[i]: store +
// pending, both kinds) and at most max_stores stores per chunk, a store over the budget a chunk of its own.
std::vector<int> mml_cube_chunks(int n, const long long* pts, long long budget, int max_stores);
// The sort key of the cube filter: segment << 53 | cube << 40 | PCL voxel index.  4851 cubes take 13 bits, the index 40: up to 2048
// segments in 64 bits.
__host__ __device__ inline unsigned long long mml_cube_key(unsigned seg, unsigned cube, unsigned long long vox) {
    return ((unsigned long long)seg << 53) | ((unsigned long long)cube << 40) | vox;
}
__host__ __device__ inline unsigned mml_cube_key_cube(unsigned long long key) { return (unsigned)(key >> 40) & 0x1fffu; }
inline int mml_cube_key_bits(int nseg) {  // the sort's end_bit
    int b = 1;
    while ((1 << b) < nseg) ++b;
    return 53 + b;
}
int mml_launch_knn5(mml_ctx* ctx, int kind, const float* d_q, int nq, float max_d2, int* d_idx, float* d_d2);
// with_stats = false (mml_step, which reads none of them): the per-slot statistics (counts, normal Gram matrix) are left stale and
// computed by mml_ensure_assoc_stats when a consumer asks (mml_linearize*, the next mml_associate with statistics)
int mml_launch_associate(mml_ctx* ctx, int first, int count, const double* d_Twl, double thres_dist, bool with_stats = true);
int mml_ensure_assoc_stats(mml_ctx* ctx, int first, int count);
// world_map_assoc.hip: association against a surfel world map.  mml_wm_assoc_ready: the refusals of a call over slots
// [first, first + count) -- before any device work but ONE read-back of the stack sizes -- and the call's map numbers sent down;
// mml_launch_wm_associate: k_wm_associate for those slots at the poses d_Twl (16 doubles per slot, on the device), enqueue only.
int mml_wm_assoc_ready(mml_ctx* ctx, const char* who, int first, int count, const int* map_of_slot, const mml_wm_assoc_opts* o, bool need_all);
int mml_wm_assoc_opts_ok(mml_ctx* ctx, const char* who, const mml_wm_assoc_opts* o);  // the option refusals alone, host only
int mml_launch_wm_associate(mml_ctx* ctx, int first, int count, const double* d_Twl, const mml_wm_assoc_opts& o);
// world_map.hip: the surfel cache of a surfel map made valid for the table as it is (allocated on first use, rebuilt when stale),
// enqueue only.  world_map_score.hip: mml_world_map_score behind its argument checks; ready = false: the caller has run
// mml_wm_assoc_ready for these slots and maps itself (mml_world_map_relocalize, once for all its levels).
int mml_wm_cache_ready(mml_ctx* ctx);
int mml_wm_score_run(mml_ctx* ctx, const char* who, int first, int count, const int* map_of_slot, int n_hyp, const double* T_wl,
                     const mml_wm_score_opts* o, mml_wm_score* out, bool ready);
#define MML_SOLVE_RESULT 24  // doubles per problem of k_solve's result record: x (6), stack sizes (2), association statistics (16)
// d_x_in / d_result (a PoseBlock's start poses, the result records): packed pose calls only, mml_pose_packed(count, ctx->cus)
int mml_launch_solve(mml_ctx* ctx, int first, int count, int window, const double* d_Tbl, mml_solve_opts opts,
                     bool want_trace, const double* d_x_in = nullptr, double* d_result = nullptr);
int mml_window_solve_continue(mml_ctx* ctx, int first, int count, int window, const double* d_Tbl, mml_solve_opts opts);
int mml_feature_init(mml_ctx* ctx);
// mml_union_assemble (livox_stream.hip): the host-only checks, then -- after the entry point's slot checks -- the device part
int mml_union_check(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* stamps, const float* velo_xyzi,
                    const int* velo_offsets, mml_union_frame* out);
int mml_union_run(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* stamps, const float* velo_xyzi,
                  const int* velo_offsets, const float* tf, mml_union_frame* out);
// the same pair for mml_union_assemble_offset
int mml_union_offset_check(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* starts, int sliced_points,
                           const float* velo_xyzi, const int* velo_offsets, mml_union_frame* out);
int mml_union_offset_run(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* starts, int sliced_points,
                         const float* velo_xyzi, const int* velo_offsets, const float* tf, mml_union_frame* out);
// What mml_time_offset_estimate_stream (time_offset.hip) reads of a stream: the live part's arrays (point i sits at element
// i - base of rec, 5 dwords each, and of stamp) and the host's counters.  livox_stream.hip; nothing is enqueued or changed.
struct MmlLivoxView {
    mml_ctx* ctx;
    const uint32_t* rec;
    const uint64_t* stamp;
    long base, front, tail;
    uint64_t hs;
};
MmlLivoxView mml_livox_stream_view(const mml_livox_stream* s);
// velo_fov.hip, for the same caller, which keeps the selection on the device: the argument rules of the FOV calls (n_max: the
// caller's bound on n); the selection itself -- records down, k_vfov_select, counts and info back in ONE host synchronisation, *info
// being n rows of pinned memory that stay valid until the context's next selection --; and the packing pass of that selection,
// enqueued on the current stream: frame i's kept rows as packed x, y, z from row dst[i] of the device array d_xyz.
int mml_vfov_check(mml_ctx* ctx, const char* who, int n, int n_max, const uint8_t* data, const long* byte_offsets, const int* n_points, int step,
                   int ox, int oy, int oz);
int mml_vfov_select_device(mml_ctx* ctx, const char* who, int n, const uint8_t* data, const long* byte_offsets, const int* n_points, int step,
                           int ox, int oy, int oz, const mml_velo_fov_info** info);
int mml_vfov_pack_device(mml_ctx* ctx, int n, const long long* dst, int max_kept, float* d_xyz);
// imu_preint.hip: k_imu_preintegrate on device arrays (bias: n x (bg | ba)), asynchronous on the current stream
int mml_launch_imu_preintegrate(mml_ctx* ctx, int n, const double* d_samples, const int* d_offsets, const double* d_bias, mml_imu_preint* d_out);
int mml_launch_detect_line(mml_ctx* ctx, int n, uint16_t* d_final);
int mml_launch_raw_lines(mml_ctx* ctx, int first, int count);  // raw_line[] of the slots (ring / line id per raw point), for the GICP refresh
int mml_launch_linearize(mml_ctx* ctx, int slot, const double* d_x, const double* d_Tbl, double w_tan,
                         double huber, double* d_record, int frames = 1);

#endif
