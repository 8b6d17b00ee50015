// Replays mml::ImuQueue (host/mmloam_adapter.hpp) without a device: push message by message, fetchImuMsgs interval by interval
// and then all intervals in one call, and the trim.  tests/test_imu_queue_adapter.py builds and runs it against tests/imu_fetch_ref.py.
// stdin:  n_msgs n, then n_msgs lines of 7 doubles (stamp, gyro xyz, accel xyz), then n lines "start end"; doubles as hex floats;
//         then "t keep_min" for the trim.
// stdout: per interval "ok status n" and its rows (7 hex floats each), from the single calls; "batch same|differs"; "size k".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmloam_adapter.hpp"

static double read_double() {
    char buf[64];
    if (std::scanf("%63s", buf) != 1) std::exit(2);
    return std::strtod(buf, nullptr);
}

int main() {
    long n_msgs = 0;
    int n = 0;
    if (std::scanf("%ld %d", &n_msgs, &n) != 2 || n_msgs < 0 || n < 1) return 2;
    mml::ImuQueue q;
    for (long i = 0; i < n_msgs; ++i) {
        double m[7];
        for (double& v : m) v = read_double();
        q.push(m);
    }
    std::vector<double> ts((size_t)n), te((size_t)n), all;
    std::vector<int> counts;
    for (int i = 0; i < n; ++i) {
        ts[(size_t)i] = read_double();
        te[(size_t)i] = read_double();
        std::vector<double> vimuMsg;
        const bool ok = q.fetchImuMsgs(ts[(size_t)i], te[(size_t)i], vimuMsg);
        std::printf("%d %d %d\n", ok ? 1 : 0, q.last_interval().status, q.last_interval().n);
        for (size_t k = 0; k < vimuMsg.size(); ++k) std::printf("%a%c", vimuMsg[k], k % 7 == 6 ? '\n' : ' ');
        all.insert(all.end(), vimuMsg.begin(), vimuMsg.end());
        counts.push_back((int)(vimuMsg.size() / 7));
    }
    const std::vector<bool> ok = q.fetchImuMsgs(ts, te);
    bool same = q.last_samples() == all && (int)ok.size() == n;
    for (int i = 0; i < n && same; ++i)
        same = q.last_offsets()[(size_t)i + 1] - q.last_offsets()[(size_t)i] == counts[(size_t)i] && ok[(size_t)i] == (q.last_intervals()[(size_t)i].status == 0);
    std::printf("batch %s\n", same ? "same" : "differs");
    const double t = read_double();
    const long keep = (long)read_double();
    q.drop_before(t, keep);
    std::printf("size %ld\n", q.size());
    return 0;
}
