// wire_decode.h -- the two record layouts a union_cloud message arrives in, ONE definition for every reader:
//   k_wire_decode_batch (wire_ingest.hip, the byte source is LDS or the staged bytes in global memory),
//   mml_wire_decode_host (the byte source is the caller's buffer) and tests/cpp/wire_decode_replay.cpp (the plain host compiler).
// A reader hands in a byte source `S` with one member, `uint32_t le32(int64_t pos) const`: the four bytes at pos .. pos + 3 as a
// little-endian word, whatever pos mod 4 is.  Everything below asks for words that lie INSIDE the record it decodes, so a source
// that serves exactly the payload's bytes is never asked for one outside them.
//   Velodyne  sensor_msgs/PointCloud2 payload: records of point_step bytes, float32 fields x, y, z, intensity at byte offsets
//             listed in msg.fields (pcl::fromROSMsg<PointXYZI>, unionFeatureExtract.cpp:1119-1121) -> x, y, z, intensity
//   Livox 19  serialised livox_ros_driver/CustomPoint: uint32 offset_time, float32 x, y, z, uint8 reflectivity, tag, line
//             (the fields read at unionFeatureExtract.cpp:985-997) -> the five dwords of mml_livox_point, _pad = 0
//   Livox 20  mml_livox_point as it stands, pad byte included
// Integer bit assembly only: a float travels as its bit pattern and never through an arithmetic instruction or a float register
// of the host, so signalling NaNs, NaN payloads, -0 and denormals arrive unchanged.
// The argument rules of mml_scan_upload_wire_plan / mml_scan_upload_wire_batch / mml_wire_decode_host live here too (wire_plan).
#ifndef MML_WIRE_DECODE_H
#define MML_WIRE_DECODE_H

#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mmloam_hip.h"

#if defined(__HIPCC__)
#define MML_WIRE_HD __host__ __device__
#else
#define MML_WIRE_HD
#endif

#define MML_WIRE_BATCH_MAX 65535  // frames per call: the decode kernel's second grid dimension

// The plain byte source: memory the caller can address byte by byte (host buffers; on the device, global memory).
struct WireBytes {
    const uint8_t* p;
    MML_WIRE_HD uint32_t le32(int64_t pos) const {
        const uint8_t* q = p + pos;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
};

// One Velodyne record at byte `rec` of the source -> the bit patterns of x, y, z, intensity (oi < 0: no such field, +0.0f).
template <class S>
MML_WIRE_HD inline void wire_velo_record(const S& s, int64_t rec, int ox, int oy, int oz, int oi, uint32_t out[4]) {
    out[0] = s.le32(rec + ox);
    out[1] = s.le32(rec + oy);
    out[2] = s.le32(rec + oz);
    out[3] = oi >= 0 ? s.le32(rec + oi) : 0u;
}

// One Livox record of record_bytes (19 or 20) at byte `rec` -> the five dwords of mml_livox_point: offset_time, x, y, z,
// reflectivity | tag << 8 | line << 16 | _pad << 24.  The 19-byte form takes its last three bytes from the word at +15 (bytes
// 15 .. 18, the last of the record), which leaves _pad 0.
template <class S>
MML_WIRE_HD inline void wire_livox_record(const S& s, int64_t rec, int record_bytes, uint32_t out[5]) {
    out[0] = s.le32(rec);
    out[1] = s.le32(rec + 4);
    out[2] = s.le32(rec + 8);
    out[3] = s.le32(rec + 12);
    out[4] = record_bytes == 19 ? s.le32(rec + 15) >> 8 : s.le32(rec + 16);
}

// ---- host only from here: the call's arguments, their rules, the host decode ----------------------------------------------------
struct WireCall {
    int count;
    const int64_t* velo_at;
    const int* n_velo;
    int point_step, off_x, off_y, off_z, off_intensity;
    const int64_t* livox_at;
    const int* n_livox;
    int livox_record_bytes;
};

// One sensor's frames: offsets never decrease, payloads do not overlap (frame i starts at or behind the end of frame i - 1, an
// empty frame's offset included), counts within `cap` (cap < 0: not checked).  span: first byte of the first payload, one past the
// last byte of the last one; 0, 0 when the sensor has no point.  `at` may be NULL when every count is 0.
inline int wire_plan_sensor(const char* name, const char* cap_name, int count, const int64_t* at, const int* n, int rec_bytes, int cap,
                            int64_t span[2], int* bad_frame, char* msg, size_t msg_len) {
    span[0] = span[1] = 0;
    bool any = false;
    int64_t prev_end = 0;
    for (int i = 0; i < count; ++i) {
        *bad_frame = i;
        if (n[i] < 0) {
            snprintf(msg, msg_len, "frame %d: negative %s count (%d)", i, name, n[i]);
            return MML_ERR_INVALID;
        }
        if (!at) {
            if (n[i] == 0) continue;
            snprintf(msg, msg_len, "frame %d: %d %s points and NULL offsets", i, n[i], name);
            return MML_ERR_INVALID;
        }
        const int64_t bytes = (int64_t)n[i] * rec_bytes;
        if (at[i] < 0 || at[i] > INT64_MAX - bytes) {
            snprintf(msg, msg_len, "frame %d: %s offset %lld is negative or overflows with its %lld bytes", i, name, (long long)at[i],
                     (long long)bytes);
            return MML_ERR_INVALID;
        }
        if (i > 0 && at[i] < prev_end) {
            snprintf(msg, msg_len, "frame %d: %s offset %lld lies before byte %lld where frame %d ends (offsets never decrease, payloads never overlap)",
                     i, name, (long long)at[i], (long long)prev_end, i - 1);
            return MML_ERR_INVALID;
        }
        prev_end = at[i] + bytes;
        if (cap >= 0 && n[i] > cap) {
            snprintf(msg, msg_len, "frame %d: %d %s points, %s is %d", i, n[i], name, cap_name, cap);
            return MML_ERR_CAPACITY;
        }
        if (n[i] > 0) {
            if (!any) span[0] = at[i];
            span[1] = prev_end;
            any = true;
        }
    }
    *bad_frame = -1;
    return MML_OK;
}

// Every rule that needs no context.  MML_OK, or MML_ERR_INVALID / MML_ERR_CAPACITY with the text in msg (at least 192 characters)
// and the frame in *bad_frame (-1: the refusal is about the call, not about one frame).  span[4] is written only with MML_OK.
inline int wire_plan(const WireCall& c, int max_velo_points, int max_livox_points, int64_t span[4], int* bad_frame, char* msg, size_t msg_len) {
    int bad = -1;
    if (bad_frame) *bad_frame = -1;
    if (c.count < 1 || c.count > MML_WIRE_BATCH_MAX) {
        snprintf(msg, msg_len, "count %d outside 1 .. %d", c.count, MML_WIRE_BATCH_MAX);
        return MML_ERR_INVALID;
    }
    if (!c.n_velo || !c.n_livox || !span) {
        snprintf(msg, msg_len, "NULL n_velo, n_livox or span");
        return MML_ERR_INVALID;
    }
    if (c.point_step < 12 || c.point_step > 256) {
        snprintf(msg, msg_len, "point_step %d outside 12 .. 256", c.point_step);
        return MML_ERR_INVALID;
    }
    const int offs[4] = {c.off_x, c.off_y, c.off_z, c.off_intensity};
    for (int k = 0; k < 4; ++k)
        if (!((k == 3 && offs[k] < 0) || (offs[k] >= 0 && offs[k] + 4 <= c.point_step))) {
            snprintf(msg, msg_len, "field offset %d (%c) outside the %d-byte point record", offs[k], "xyzi"[k], c.point_step);
            return MML_ERR_INVALID;
        }
    if (c.livox_record_bytes != 19 && c.livox_record_bytes != 20) {
        snprintf(msg, msg_len, "livox_record_bytes %d is neither 19 (wire form) nor 20 (mml_livox_point)", c.livox_record_bytes);
        return MML_ERR_INVALID;
    }
    int64_t sp[4];
    int rc = wire_plan_sensor("Velodyne", "max_velo_points", c.count, c.velo_at, c.n_velo, c.point_step, max_velo_points, sp, &bad, msg, msg_len);
    if (rc == MML_OK)
        rc = wire_plan_sensor("Livox", "max_livox_points", c.count, c.livox_at, c.n_livox, c.livox_record_bytes, max_livox_points, sp + 2, &bad, msg,
                              msg_len);
    if (bad_frame) *bad_frame = bad;
    if (rc != MML_OK) return rc;
    memcpy(span, sp, sizeof(sp));
    return MML_OK;
}

// The decode of a whole call on the host: frame i's Velodyne points from row sum(n_velo[0 .. i)) of velo_xyzi (4 words a row), its
// Livox points from row sum(n_livox[0 .. i)) of livox (5 words a row).  The arguments have passed wire_plan.  The outputs are
// written as words (memcpy), never as floats.
inline void wire_decode_host(const WireCall& c, const uint8_t* velo_data, const uint8_t* livox_data, void* velo_xyzi, void* livox) {
    const WireBytes vs{velo_data}, ls{livox_data};
    char* vo = static_cast<char*>(velo_xyzi);
    char* lo = static_cast<char*>(livox);
    for (int i = 0; i < c.count; ++i) {
        for (int k = 0; k < c.n_velo[i]; ++k, vo += 16) {
            uint32_t w[4];
            wire_velo_record(vs, c.velo_at[i] + (int64_t)k * c.point_step, c.off_x, c.off_y, c.off_z, c.off_intensity, w);
            memcpy(vo, w, 16);
        }
        for (int k = 0; k < c.n_livox[i]; ++k, lo += 20) {
            uint32_t w[5];
            wire_livox_record(ls, c.livox_at[i] + (int64_t)k * c.livox_record_bytes, c.livox_record_bytes, w);
            memcpy(lo, w, 20);
        }
    }
}

#endif
