// csrc/velo_fov.h -- the Velodyne field-of-view selection of velo_cloud_handler (unionLidarsAligner.cpp:437-490), host and device
// source.  Per frame of n points, with A(i) = -atan2(y_i, x_i) as float:
//   :439-447  startOri = A(0), endOri = A(n-1) + 2 pi, folded into (startOri + pi, startOri + 3 pi)       vfov_sweep
//   :461-470  while halfPassed is false: ori folded into [startOri - pi/2, startOri + 3 pi/2]             vfov_first_branch
//             ori - startOri > pi sets halfPassed                                                         vfov_sets_half
//   :471-477  afterwards: ori + 2 pi folded into [endOri - 3 pi/2, endOri + pi/2]                         vfov_second_branch
//   :479      relTime = (ori - startOri) / (endOri - startOri)                                            vfov_rel_time
//   :482-483  kept iff ori lies in (-0.7608, 0.7158) or in that interval + 2 pi                           vfov_in_fov
// Arithmetic (convention 4): the translation unit includes the PCL headers, so atan2(float, float) is the float
// overload = glibc's atan2f = mml_libm::atan2f_fd.  ori, startOri, endOri are floats; every M_PI expression is a double, so each
// comparison promotes the float side, each `ori +- 2 * M_PI` is a double sum rounded to float by the assignment, and
// `ori - startOri`, `endOri - startOri` and the division are float operations (the build has -ffp-contract=off and correctly
// rounded float division on the device).  NaN / Inf coordinates need no case of their own: every comparison with a NaN is false.
// vfov_frame_host is the reference's loop as written, flag and all; the device (velo_fov.hip) resolves the flag in parallel from
// the same pieces: h = the first i whose first-branch ori sets the flag, points i <= h take the first branch, the others the second.
#pragma once
#include <stdint.h>
#include <string.h>

#include "libm_f32.h"
#include "mmloam_hip.h"

#if defined(__HIPCC__)
#define MML_VFOV_HD __host__ __device__ inline
#else
#define MML_VFOV_HD inline
#endif

namespace mml_vfov {

constexpr double PI = 3.14159265358979323846;  // M_PI

MML_VFOV_HD float vfov_azimuth(float x, float y) { return -mml_libm::atan2f_fd(y, x); }

MML_VFOV_HD void vfov_sweep(float a_first, float a_last, float& startOri, float& endOri) {
    startOri = a_first;
    endOri = (float)((double)a_last + 2 * PI);
    if ((double)(endOri - startOri) > 3 * PI)
        endOri = (float)((double)endOri - 2 * PI);
    else if ((double)(endOri - startOri) < PI)
        endOri = (float)((double)endOri + 2 * PI);
}

MML_VFOV_HD float vfov_first_branch(float ori, float startOri) {
    if ((double)ori < (double)startOri - PI / 2)
        ori = (float)((double)ori + 2 * PI);
    else if ((double)ori > (double)startOri + PI * 3 / 2)
        ori = (float)((double)ori - 2 * PI);
    return ori;
}

MML_VFOV_HD bool vfov_sets_half(float ori, float startOri) { return (double)(ori - startOri) > PI; }

MML_VFOV_HD float vfov_second_branch(float ori, float endOri) {
    ori = (float)((double)ori + 2 * PI);
    if ((double)ori < (double)endOri - PI * 3 / 2)
        ori = (float)((double)ori + 2 * PI);
    else if ((double)ori > (double)endOri + PI / 2)
        ori = (float)((double)ori - 2 * PI);
    return ori;
}

// The one place where a NaN reaches an output: with a NaN first (last) point startOri (endOri) is NaN and so is every relTime.
// Which NaN is a matter of the machine: SSE returns its first NaN operand, quieted, else the second; the device's a - b negates b
// by a source modifier, sign of a NaN included.  vfov_nan_rule applies the SSE rule on top of a result, so both builds write the
// reference's bits; for operands that are numbers it returns r unchanged.
MML_VFOV_HD float vfov_nan_rule(float a, float b, float r) {
    if (a != a) return mml_libm::i2f(mml_libm::f2i(a) | 0x00400000);
    if (b != b) return mml_libm::i2f(mml_libm::f2i(b) | 0x00400000);
    return r;
}
MML_VFOV_HD float vfov_rel_time(float ori, float startOri, float endOri) {
    const float num = vfov_nan_rule(ori, startOri, ori - startOri), den = vfov_nan_rule(endOri, startOri, endOri - startOri);
    return vfov_nan_rule(num, den, num / den);
}

MML_VFOV_HD bool vfov_in_fov(float ori) {
    const double o = ori;
    return (o > -0.7608 && o < 0.7158) || (o > -0.7608 + 2 * PI && o < 0.7158 + 2 * PI);
}

// One frame on the host: n records of `step` bytes, float32 fields at ox / oy / oz.  rows (x, y, z, relTime per kept point, in input
// order) may be null: the frame is then only counted.  n == 0 (where the reference reads points[0]) yields nothing.
inline void vfov_frame_host(const uint8_t* rec, int n, int step, int ox, int oy, int oz, float* rows, mml_velo_fov_info* info) {
    info->start_ori = info->end_ori = 0.f;
    info->half_index = -1;
    info->n_kept = 0;
    if (n <= 0) return;
    const auto field = [&](int i, int off) {
        float v;
        memcpy(&v, rec + (size_t)i * step + off, 4);
        return v;
    };
    float startOri, endOri;
    vfov_sweep(vfov_azimuth(field(0, ox), field(0, oy)), vfov_azimuth(field(n - 1, ox), field(n - 1, oy)), startOri, endOri);
    bool halfPassed = false;
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const float x = field(i, ox), y = field(i, oy), z = field(i, oz);
        float ori = vfov_azimuth(x, y);
        if (!halfPassed) {
            ori = vfov_first_branch(ori, startOri);
            if (vfov_sets_half(ori, startOri)) {
                halfPassed = true;
                info->half_index = i;
            }
        } else {
            ori = vfov_second_branch(ori, endOri);
        }
        const float relTime = vfov_rel_time(ori, startOri, endOri);
        if (vfov_in_fov(ori)) {
            if (rows) {
                float* r = rows + 4 * (size_t)kept;
                r[0] = x;
                r[1] = y;
                r[2] = z;
                r[3] = relTime;
            }
            ++kept;
        }
    }
    info->start_ori = startOri;
    info->end_ori = endOri;
    info->n_kept = kept;
}

}  // namespace mml_vfov
