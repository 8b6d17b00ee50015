// Drives mml::LivoxPointQueue's marks and mml::estimate_timeoffset (host/mmloam_adapter.hpp) on a device the way the aligner node
// would: the queued Livox messages are pushed, the queued Velodyne frames go in as PointCloud2-style payloads
// (tests/test_gpu_time_offset_stream.py builds and runs it).
// argv[1]: a file of  int32 n_msgs, n_frames, resolution, sliced | uint64 hori_stamp |
//          per message uint64 timebase, int32 n, n records of 20 bytes | per frame uint64 stamp, int32 n, n rows of 4 floats.
// stdout: "mark timebase first count" per message, "row gate_status selected status n_kept n_windows best_window lowest_error(hex)
//          optim_start time_offset accepted", "few gate_status selected" for the same call on a queue of seven messages.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "mmloam_adapter.hpp"

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
    return std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    uint64_t hori = 0;
    if (!rd(f, head, 4) || !rd(f, &hori, 1)) return 2;
    const int n_msgs = head[0], n_frames = head[1], res = head[2], sliced = head[3];
    std::vector<std::vector<mml_livox_point>> pts((size_t)n_msgs);
    std::vector<mml::LivoxMsg> msgs((size_t)n_msgs);
    for (int j = 0; j < n_msgs; ++j) {
        int32_t n = 0;
        if (!rd(f, &msgs[(size_t)j].timebase, 1) || !rd(f, &n, 1)) return 2;
        pts[(size_t)j].resize((size_t)n);
        if (!rd(f, pts[(size_t)j].data(), (size_t)n)) return 2;
        msgs[(size_t)j].points = pts[(size_t)j].data();
        msgs[(size_t)j].point_num = n;
    }
    std::vector<std::vector<float>> rows((size_t)n_frames);
    std::vector<mml::VeloFrame> frames((size_t)n_frames);
    std::vector<uint64_t> stamps((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i) {
        int32_t n = 0;
        if (!rd(f, &stamps[(size_t)i], 1) || !rd(f, &n, 1)) return 2;
        rows[(size_t)i].resize(4 * (size_t)n);
        if (!rd(f, rows[(size_t)i].data(), 4 * (size_t)n)) return 2;
        frames[(size_t)i].data = reinterpret_cast<const uint8_t*>(rows[(size_t)i].data());
        frames[(size_t)i].n_points = n;
    }
    std::fclose(f);
    try {
        mml::Context ctx(1);
        {
            mml::LivoxPointQueue queue(ctx, 16384);
            queue.transform_hori_timestamp(msgs);
            for (const auto& m : queue.marks()) std::printf("mark %" PRIu64 " %ld %d\n", m.timebase, m.first, m.count);
            const mml::TimeOffsetEstimate e = mml::estimate_timeoffset(ctx, queue, frames, stamps, hori, nullptr, res, sliced, 1e6);
            std::printf("row %d %d %d %d %d %d %a %" PRIu64 " %" PRIu64 " %d\n", e.gate_status, e.selected, e.row.status, e.row.n_kept,
                        e.row.n_windows, e.row.best_window, e.row.lowest_error, e.row.optim_start, e.row.time_offset, e.row.accepted);
        }
        {
            mml::LivoxPointQueue queue(ctx, 16384);
            queue.transform_hori_timestamp(std::vector<mml::LivoxMsg>(msgs.begin(), msgs.begin() + 7));
            const mml::TimeOffsetEstimate e = mml::estimate_timeoffset(ctx, queue, frames, stamps, hori, nullptr, res, sliced, 1e6);
            std::printf("few %d %d\n", e.gate_status, e.selected);
        }
    } catch (const std::exception& ex) {
        std::printf("exception %s\n", ex.what());
        return 1;
    }
    std::printf("TIME_OFFSET_STREAM_PROBE_DONE\n");
    return 0;
}
