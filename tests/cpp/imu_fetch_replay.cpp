// Replays csrc/imu_fetch.h on the host, stand-alone (tests/test_imu_fetch.py builds it with -fsanitize=address,undefined and
// -D__host__= -D__device__=, so the header is compiled by the plain host compiler).
// stdin:  n_msgs n, then n_msgs lines of 7 doubles (stamp, gyro xyz, accel xyz), then n lines "start end"; doubles as hex floats.
// stdout: n lines "status n first interpolated", then every row of every interval (7 hex floats), then a checksum line over
//         the gyro chain and the prediction, which run on every interval too.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "imu_fetch.h"

static double read_double() {
    char buf[64];
    if (std::scanf("%63s", buf) != 1) std::exit(2);
    return std::strtod(buf, nullptr);
}

int main() {
    long n_msgs = 0;
    int n = 0;
    if (std::scanf("%ld %d", &n_msgs, &n) != 2 || n_msgs < 0 || n < 0) return 2;
    // exactly as large as the data: a read past either end is an AddressSanitizer report
    std::vector<double> msgs(7 * (size_t)n_msgs), ts((size_t)n), te((size_t)n);
    for (double& v : msgs) v = read_double();
    for (int i = 0; i < n; ++i) {
        ts[(size_t)i] = read_double();
        te[(size_t)i] = read_double();
    }
    std::vector<mml_imu_interval> rows((size_t)n);
    for (int i = 0; i < n; ++i) {
        imu_fetch_plan(msgs.data(), 0, 0, n_msgs, ts[(size_t)i], te[(size_t)i], &rows[(size_t)i]);
        std::printf("%d %d %ld %d\n", rows[(size_t)i].status, rows[(size_t)i].n, rows[(size_t)i].first, rows[(size_t)i].interpolated);
    }
    double ex[16] = {0, -1, 0, 0.1, 1, 0, 0, -0.2, 0, 0, 1, 0.3, 0, 0, 0, 1};
    const ImuExtrinsic e = imu_extrinsic(ex);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const mml_imu_interval& r = rows[(size_t)i];
        std::vector<double> packed(7 * (size_t)r.n);
        for (int k = 0; k < r.n; ++k) {
            imu_fetch_row(msgs.data(), 0, r.first, r.n, r.interpolated, ts[(size_t)i], te[(size_t)i], k, packed.data() + 7 * (size_t)k);
            for (int c = 0; c < 7; ++c) std::printf("%a%c", packed[7 * (size_t)k + c], c == 6 ? '\n' : ' ');
        }
        double q[4], Rb[9], Rl[9], state[10], dR[9], dt[3];
        imu_fetch_gyro(packed.data(), r.n, q);
        imu_predict_gyro(q, e, Rb, Rl);
        const double prev[10] = {1, 2, 3, 0, 0, 0, 1, 0.1, 0.2, 0.3}, dp[3] = {0.01, 0.02, 0.03}, dv[3] = {0.1, 0.0, -0.1};
        imu_predict_lio(prev, q, dp, dv, e, state, dR, dt);
        for (int k = 0; k < 9; ++k) sum += Rl[k] + dR[k];
        sum += state[0] + dt[0];
    }
    std::printf("checksum %a\n", sum);
    return 0;
}
