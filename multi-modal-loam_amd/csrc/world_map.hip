// world_map.hip -- the world map: the registered clouds of n sequences voxel-merged on the device (mml_world_map_*).
// One open-addressing hash table per context (mml_ctx::world): key (world_map_key.h: map << 54 | three 18-bit voxel indices),
// float4 sum (x, y, z, intensity) and count per position, linear probing, MML_WM_EMPTY where free; n maps share the table, the
// map number is part of the key.  A voxel is never moved or removed by an add, so the work of a call does not depend on the size
// of the map.  The arithmetic -- world point, voxel index, key, hash, accumulator -- is world_map_key.h's and nowhere else.
//
// mml_world_map_add, one chain for the `count` slots of the call (B = the call's bound: NT points for every slot that takes part):
//   k_wm_keys      grid (NT / 256, count): the slot's row (pose, map, offset) is wave-uniform; every fused point of the slot through
//                  mml_world_point and mml_wm_classify, label_mask applied, the skipped points counted; kept point g of slot i
//                  writes its world point, key and ordinal at index off_i + g (the keys were preset to MML_WM_EMPTY, so every
//                  other index sorts behind the kept points)
//   sort           one stable mml_sort_pairs<unsigned long long> over the B pairs: equal keys stay in ordinal order = slot order,
//                  then fused point order; k_run_heads (the empty marker starts no run) and one exclusive scan
//   k_wm_lookup    one lane per distinct voxel of the call: probes the table read-only, records the position or a miss; the launch
//                  counts the distinct voxels and the misses
//   read-back      the call's ONLY host synchronisation: the seven counters and the table's total.  total + misses > capacity:
//                  MML_ERR_CAPACITY -- only scratch has been written up to here
//   k_wm_insert    one lane per distinct voxel: a miss claims a position with a 64-bit atomicCAS on the key array; then the run of
//                  the voxel's points is added in order to the stored accumulator (zero for a new voxel) and stored with plain
//                  stores -- keys inside a call are distinct, one lane owns a voxel; the per-map counts and the total follow
// Scratch per point of B: 16 (world point) + 2 x 8 (keys in / out) + 2 x 4 (ordinals in / out) + 3 x 4 (run head, scan, hit) = 52
// bytes, grow-only, and rocPRIM's temporary storage beside it.
//
// A SURFEL MAP (mml_world_map_create_opts, MML_WM_SURFELS) holds three float4 of moments per position beside the sum and the
// count (world_map_key.h, MmlWmMoments: the offsets from the voxel's centre, their six products, the view vectors), 76 bytes per
// position instead of 28.  Its add runs the same chain with k_wm_insert<true>: the lane carries the moments beside the sums --
// loaded on a hit, zero on a claim, plain stores at the end -- with the voxel's centre from the key it holds and the point's
// sensor origin from the call's origin table: a point's ordinal is off_i + g and every slot that takes part owns NT ordinals, so
// ordinal / NT is the slot's place among them.  NEW SCRATCH PER POINT: 0 bytes (52 as for a plain map); the call's table block
// grows by one float4 origin per slot, written by the host from the pose (mml_wm_origin).  The moments of a position are read
// only after its key is claimed and its accumulators are stored, so neither reset(-1) nor create clears them.
// mml_world_map_download, _download_moments and _download_surfels share one collect, sort and gather chain (wm_download); the
// surfel gather is one lane per voxel: the covariance in double (mml_wm_covariance), eig3_sym register-only, the normal turned
// towards the view sum (wm_surfel, world_map_dev.h: the association against the map, world_map_assoc.hip, runs it too).
//
// ROWS OUT OF THE TABLE AND BACK.  Outside the table a voxel is a row of a WmRows: its key, its stored sum and count and, on a
// surfel map, its moments as three float4 per row (the export's layout; there is no other).  Rows leave the table through ONE
// gather (k_wm_gather: row i is position vals[i], sorted or not) and enter it through ONE put (k_wm_put: claim, then plain
// stores; a by-value WmCounts says what the launch writes into the per-map counts and the total).  On the host wm_rebuild is
// "gather these survivors, clear the keys, put them back, write the counts" -- a position inside a probe chain cannot be freed, so
// whatever removes voxels rebuilds -- and wm_rows_up is "these rows to the caller's arrays, the keys as voxel indices".  Behind them:
//   mml_world_map_export           a fourth gather of the download chain (k_wm_gather over the sorted positions), then wm_rows_up;
//                                  mml_world_map_download_moments is the same gather with the moments alone
//   mml_world_map_import           checks its rows on the host, looks all of them up in one launch (k_wm_import_find), refuses at the
//                                  add's refusal point -- one read-back, only scratch written -- and then puts them, the map's count
//                                  and the total growing by one add per wave
//   mml_world_map_reset(map >= 0)  collects the other maps' positions (k_wm_collect<true>) and rebuilds from them, the map's count
//                                  zeroed; scratch by the survivors it has counted
//   mml_world_map_evict            removes voxels by rule (world_map_evict.h: an index box and a minimum count per map named):
//                                  k_wm_evict_mark walks the table once and splits the occupied positions into an evicted and a
//                                  survivor list; one read-back of the counters, the refusal point; then the evicted rows are sorted
//                                  and gathered when they are wanted, the table is rebuilt from the survivors, every ruled map's count
//                                  set to n_before - n_evicted from the device's counters, and the evicted rows go up behind a second
//                                  synchronisation (wm_rows_up); scratch by capacity_voxels
//
// THE SURFEL CACHE (mml_wm_cache_ready, for mml_world_map_score): one float4 per table position, (nx, ny, nz, planarity) of the
// position's surfel, 16 bytes per position more (92 instead of 76), allocated in the map's memory group by the first call that
// scores and filled by k_wm_surfel_cache, one lane per position, register-only, wm_surfel as everywhere.  It is valid for the
// table version it was built from: every call that writes the table -- add past its refusal point, import, reset, create, destroy
// -- advances WorldMap::version on the host (wm_touch; no kernel of theirs knows of the cache), and a score call rebuilds a
// cache whose version is behind.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mml_internal.h"
#include "fused_view_dev.h"
#include "voxel_sort_dev.h"
#include "world_map_assoc.h"
#include "world_map_evict.h"

namespace {
#include "eig3_dev.h"
#include "world_map_dev.h"

// one slot of the call, read through scalar loads (blockIdx.y)
struct WmRow {
    double T[16];  // T_wl, row-major
    int map;       // -1: the slot is skipped
    int off;       // the slot's first index in the call's arrays
    int pad[2];
};
enum { WM_POINTS, WM_KEPT, WM_NONFINITE, WM_RANGE, WM_MASKED, WM_DISTINCT, WM_MISSES, WM_COUNTERS };

__global__ __launch_bounds__(256) void k_wm_keys(SlotArrays A, const WmRow* __restrict__ rows, float inv, unsigned label_mask,
                                                 float4* __restrict__ pts, unsigned long long* __restrict__ keys,
                                                 unsigned* __restrict__ vals, int* __restrict__ counters) {
    const WmRow& R = rows[blockIdx.y];
    if (R.map < 0) return;  // (the whole workgroup)
    const int slot = A.first + blockIdx.y;
    const FusedView V = slot_view(A, slot);
    const int b0 = blockIdx.x * blockDim.x, cv = V.cb_n[0], cl = V.cb_n[1];
    if (b0 >= V.NV + cl || (b0 >= cv && b0 + (int)blockDim.x <= V.NV)) return;  // (as k_encode_registered: no valid position here)
    int g = 0, line;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    float rel;
    bool valid = fused_at(V, b0 + threadIdx.x, g, p, rel, line);
    valid = valid && g < A.fu_info[8 * (size_t)slot] && g < A.NT;  // (the slot's points end at its count; an index stays inside the slot's NT)
    int what = -1;  // -1: masked (or no point)
    unsigned long long key = MML_WM_EMPTY;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    if (valid) {
        const unsigned label = V.label[b0 + threadIdx.x];
        if (label < 3 && ((label_mask >> label) & 1u)) {
            mml_world_point(R.T, p.x, p.y, p.z, wx, wy, wz);
            what = mml_wm_classify(R.map, wx, wy, wz, p.w, inv, key);
        }
    }
    wm_count(counters + WM_POINTS, valid);
    wm_count(counters + WM_MASKED, valid && what < 0);
    wm_count(counters + WM_NONFINITE, what == MML_WM_NONFINITE);
    wm_count(counters + WM_RANGE, what == MML_WM_OUT_OF_RANGE);
    wm_count(counters + WM_KEPT, what == MML_WM_KEPT);
    if (what == MML_WM_KEPT) {
        const size_t at = (size_t)R.off + g;
        pts[at] = make_float4(wx, wy, wz, p.w);
        keys[at] = key;
        vals[at] = (unsigned)at;
    }
}

// claims a free position for `key` (which is not in the table, and which no other lane inserts); -1 only from a full table
__device__ __forceinline__ long long wm_claim(unsigned long long* __restrict__ tab, unsigned long long slots, unsigned long long key) {
    unsigned long long h = mml_wm_hash(key, slots);
    for (unsigned long long step = 0; step < slots; ++step) {
        if (atomicCAS(tab + h, MML_WM_EMPTY, key) == MML_WM_EMPTY) return (long long)h;
        h = (h + 1) & (slots - 1);
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_wm_lookup(const unsigned long long* __restrict__ keys, const int* __restrict__ flag, int n,
                                                   const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                   int* __restrict__ hit, int* __restrict__ counters) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = s < n && flag[s];
    long long at = 0;
    if (head) {
        at = wm_find(tab, slots, keys[s]);
        hit[s] = (int)at;
    }
    wm_count(counters + WM_DISTINCT, head);
    wm_count(counters + WM_MISSES, head && at < 0);
}

// what k_wm_insert<true> takes beside the arguments of a plain map's insert; <false> takes nothing
template <bool Surfels>
struct WmMomentArgs {};
template <>
struct WmMomentArgs<true> {
    float4 *m0, *m1, *m2;   // the table's three moment arrays
    const float4* origin;   // the sensor origin of the call's i-th slot that takes part
    float leaf;
    int nt;                 // ordinals per slot that takes part (the context's NT)
};

template <bool Surfels>
__global__ __launch_bounds__(256) void k_wm_insert(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                   const int* __restrict__ flag, const int* __restrict__ hit, int n,
                                                   const float4* __restrict__ pts, unsigned long long* __restrict__ tab,
                                                   unsigned long long slots, float4* __restrict__ sum, int* __restrict__ count,
                                                   int* __restrict__ map_n, int n_maps, WmMomentArgs<Surfels> S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = s < n && flag[s];
    bool fresh = false;
    if (head) {
        const unsigned long long key = keys[s];
        long long at = hit[s];
        MmlWmAcc a = {0.f, 0.f, 0.f, 0.f, 0};
        MmlWmMoments m = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (at < 0) {
            fresh = true;
            at = wm_claim(tab, slots, key);
            atomicAdd(map_n + (int)(key >> MML_WM_MAP_SHIFT), 1);
        } else {
            const float4 v = sum[at];
            a.x = v.x;
            a.y = v.y;
            a.z = v.z;
            a.w = v.w;
            a.n = count[at];
            if constexpr (Surfels) m = wm_moments(S.m0[at], S.m1[at], S.m2[at]);
        }
        if (at >= 0) {  // (always: the host refused the call that would have filled the table)
            if constexpr (Surfels) {
                int map, i, j, k;
                mml_wm_unkey(key, map, i, j, k);
                const float cx = mml_wm_centre(i, S.leaf), cy = mml_wm_centre(j, S.leaf), cz = mml_wm_centre(k, S.leaf);
                for (int e = s; e < n && keys[e] == key; ++e) {
                    const unsigned v = vals[e];
                    const float4 p = pts[v];
                    const float4 o = S.origin[v / (unsigned)S.nt];
                    mml_wm_add(a, p.x, p.y, p.z, p.w);
                    mml_wm_add_moments(m, p.x, p.y, p.z, cx, cy, cz, o.x, o.y, o.z);
                }
                S.m0[at] = make_float4(m.sdx, m.sdy, m.sdz, m.vx);
                S.m1[at] = make_float4(m.sxx, m.sxy, m.sxz, m.vy);
                S.m2[at] = make_float4(m.syy, m.syz, m.szz, m.vz);
            } else {
                for (int e = s; e < n && keys[e] == key; ++e) {
                    const float4 p = pts[vals[e]];
                    mml_wm_add(a, p.x, p.y, p.z, p.w);
                }
            }
            sum[at] = make_float4(a.x, a.y, a.z, a.w);
            count[at] = a.n;
        }
    }
    wm_count(map_n + n_maps, fresh);
}

// download / reset: the occupied positions of one map (or of every map but one) appended to a list in any order
template <bool Others>
__global__ __launch_bounds__(256) void k_wm_collect(const unsigned long long* __restrict__ tab, unsigned long long slots, int map, int cap,
                                                    int* __restrict__ cursor, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    for (unsigned long long h = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; h < slots; h += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long k = tab[h];
        if (k == MML_WM_EMPTY || ((int)(k >> MML_WM_MAP_SHIFT) == map) == Others) continue;
        const int at = atomicAdd(cursor, 1);
        if (at < cap) {
            keys[at] = k;
            vals[at] = (unsigned)h;
        }
    }
}
// download: the centroids of the sorted positions
__global__ __launch_bounds__(256) void k_wm_centroids(const unsigned* __restrict__ vals, int n, const float4* __restrict__ sum,
                                                      const int* __restrict__ count, float4* __restrict__ out, int* __restrict__ out_n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned at = vals[i];
    const float4 v = sum[at];
    const MmlWmAcc a = {v.x, v.y, v.z, v.w, count[at]};
    float c[4];
    mml_wm_centroid(a, c);
    out[i] = make_float4(c[0], c[1], c[2], c[3]);
    out_n[i] = a.n;
}
// download_surfels: one lane per sorted position, 8 floats (wm_surfel, world_map_dev.h)
__global__ __launch_bounds__(256) void k_wm_surfels(const unsigned* __restrict__ vals, int n, WmMom M, const int* __restrict__ count,
                                                    float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned at = vals[i];
    const int np = count[at];
    float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0;
    if (np >= 3) {
        const MmlWmMoments m = wm_moments(M.m0[at], M.m1[at], M.m2[at]);
        wm_surfel(m, np, o0, o1);
    }
    out[2 * (size_t)i] = o0;
    out[2 * (size_t)i + 1] = o1;
}
// the surfel cache: every position's entry (wm_cache_entry, world_map_dev.h); a free position holds zeros
__global__ __launch_bounds__(256) void k_wm_surfel_cache(const unsigned long long* __restrict__ tab, unsigned long long slots, WmMom M,
                                                         const int* __restrict__ count, float4* __restrict__ cache) {
    const unsigned long long h = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= slots) return;
    float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tab[h] != MML_WM_EMPTY) e = wm_cache_entry(wm_moments(M.m0[h], M.m1[h], M.m2[h]), count[h]);
    cache[h] = e;
}
// ROWS OUTSIDE THE TABLE, in scratch -- the survivors of a rebuild, the rows of an export, an import or an eviction: row i is the key,
// the stored float4 sum and the count of one voxel and, on a surfel map, its moments as three float4 at mom[3 i ..] (the layout of
// mml_world_map_export); mom is null on a plain map.  There is no other layout outside the table.
struct WmRows {
    unsigned long long* keys;
    float4* sum;
    int* n;
    float4* mom;
};
// rows out of the table: row i is position vals[i] (sorted or not), one lane per row, plain loads and stores; the keys are in R
// already (the walk that made vals wrote them).  download_moments gathers the moments alone (R.sum null); both branches are
// launch-uniform
__global__ __launch_bounds__(256) void k_wm_gather(const unsigned* __restrict__ vals, int n, const float4* __restrict__ sum,
                                                   const int* __restrict__ count, WmMom M, WmRows R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned at = vals[i];
    if (R.sum) {
        R.sum[i] = sum[at];
        R.n[i] = count[at];
    }
    if (R.mom) {
        R.mom[3 * (size_t)i] = M.m0[at];
        R.mom[3 * (size_t)i + 1] = M.m1[at];
        R.mom[3 * (size_t)i + 2] = M.m2[at];
    }
}
// import: which of the call's n distinct keys the table holds already -- counted, nothing is written to the table
__global__ __launch_bounds__(256) void k_wm_import_find(const unsigned long long* __restrict__ keys, int n, const unsigned long long* __restrict__ tab,
                                                        unsigned long long slots, int* __restrict__ hits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool held = false;
    if (i < n) held = wm_find(tab, slots, keys[i]) >= 0;
    wm_count(hits, held);
}
// What a put writes into map_n beside its rows, by value; every branch on it is launch-uniform.  reset(map): zero_map and total;
// evict: the rules with their (n_before, n_evicted) counter pairs, and total; import: add_map.
struct WmCounts {
    const mml_wm_evict_rule* rules;  // map_n[rules[r].map] = per_rule[2 r] - per_rule[2 r + 1] for r < n_rules
    const int* per_rule;
    int n_rules;
    int zero_map;  // the map whose count becomes 0, or -1
    int total;     // what the total becomes, or -1
    int add_map;   // the map whose count, and with it the total, grows by the rows put (one add per wave), or -1
};
// rows into the table: k_wm_insert's claim path with the accumulators as given -- one lane per row, the keys distinct and none of
// them in the table, plain stores behind the claim; the first workgroup writes the counts that are set
__global__ __launch_bounds__(256) void k_wm_put(WmRows R, int n, unsigned long long* __restrict__ tab, unsigned long long slots,
                                                float4* __restrict__ sum, int* __restrict__ count, WmMom M, int* __restrict__ map_n, int n_maps,
                                                WmCounts C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0) {
        for (int r = threadIdx.x; r < C.n_rules; r += blockDim.x) map_n[C.rules[r].map] = C.per_rule[2 * r] - C.per_rule[2 * r + 1];
        if (threadIdx.x == 0 && C.zero_map >= 0) map_n[C.zero_map] = 0;
        if (threadIdx.x == 0 && C.total >= 0) map_n[n_maps] = C.total;
    }
    long long at = -1;
    if (i < n) at = wm_claim(tab, slots, R.keys[i]);
    if (at >= 0) {  // (always for i < n: a table that held these rows, or whose host refused the call that would have filled it)
        sum[at] = R.sum[i];
        count[at] = R.n[i];
        if (R.mom) {  // (a surfel map: the whole launch)
            M.m0[at] = R.mom[3 * (size_t)i];
            M.m1[at] = R.mom[3 * (size_t)i + 1];
            M.m2[at] = R.mom[3 * (size_t)i + 2];
        }
    }
    if (C.add_map >= 0) {
        wm_count(map_n + C.add_map, at >= 0);
        wm_count(map_n + n_maps, at >= 0);
    }
}

// evict: every table position once.  An occupied position goes, with its key, to the evicted list (the front of keys / vals, from
// index 0 up) when its map is named by a rule and mml_wme_goes says so (world_map_evict.h), else to the survivor list (the back of
// the same arrays, from index cap - 1 down: the two lists together hold at most `cap` = capacity_voxels entries).  One wave takes
// 64 consecutive positions per pass, 512 contiguous bytes of keys; the count is loaded only under a rule with min_count > 1.  One
// atomic per wave and list (wm_count's ballot), one per wave and rule met for n_before / n_evicted.  The order inside both lists
// depends on scheduling.  counters: WME_EVICTED, WME_KEPT, then (n_before, n_evicted) per rule.
enum { WME_EVICTED, WME_KEPT, WME_RULES };
__global__ __launch_bounds__(256) void k_wm_evict_mark(const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                       const int* __restrict__ count, const int* __restrict__ rule_of, int n_maps,
                                                       const mml_wm_evict_rule* __restrict__ rules, int cap, int* __restrict__ counters,
                                                       unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1;
    // (the loop is wave-uniform: all 64 lanes stay in it, a lane past the table's end holds the free marker)
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < slots;
         base += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long h = base + lane;
        const unsigned long long key = h < slots ? tab[h] : MML_WM_EMPTY;
        const bool held = key != MML_WM_EMPTY;
        int rule = -1;
        bool goes = false;
        if (held) {
            int map, i, j, k;
            mml_wm_unkey(key, map, i, j, k);
            if (map < n_maps) rule = rule_of[map];
            if (rule >= 0) {
                const mml_wm_evict_rule R = rules[rule];
                goes = mml_wme_goes(R, i, j, k, R.min_count > 1 ? count[h] : 1);
            }
        }
        const unsigned long long ev = __ballot(goes), kp = __ballot(held && !goes);
        int b_ev = 0, b_kp = 0;
        if (lane == 0) {
            if (ev) b_ev = atomicAdd(counters + WME_EVICTED, __popcll(ev));
            if (kp) b_kp = atomicAdd(counters + WME_KEPT, __popcll(kp));
        }
        b_ev = __shfl(b_ev, 0);
        b_kp = __shfl(b_kp, 0);
        if (goes) {
            const int at = b_ev + __popcll(ev & below);
            if (at < cap) {
                keys[at] = key;
                vals[at] = (unsigned)h;
            }
        } else if (held) {
            const int at = b_kp + __popcll(kp & below);
            if (at < cap) {
                keys[cap - 1 - at] = key;
                vals[cap - 1 - at] = (unsigned)h;
            }
        }
        unsigned long long todo = __ballot(rule >= 0);  // the named maps' voxels of this pass, rule by rule
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int r = __shfl(rule, lead);
            const unsigned long long same = __ballot(rule == r), gone = __ballot(rule == r && goes);
            if ((int)lane == lead) {
                atomicAdd(counters + WME_RULES + 2 * r, __popcll(same));
                if (gone) atomicAdd(counters + WME_RULES + 2 * r + 1, __popcll(gone));
            }
            todo &= ~same;
        }
    }
}
int wm_enter(mml_ctx* ctx, const char* who) {
    if (!ctx) return MML_ERR_INVALID;
    if (ctx->world.n_maps == 0) return mml_refuse(ctx, MML_ERR_STATE, "%s: the context has no world map (mml_world_map_create)", who);
    MML_HIP(hipSetDevice(ctx->device));
    return MML_OK;
}
int wm_clear(mml_ctx* ctx, hipStream_t s) {
    mml_ctx::WorldMap& W = ctx->world;
    MML_HIP(hipMemsetAsync(W.keys, 0xff, sizeof(unsigned long long) * W.slots, s));
    MML_HIP(hipMemsetAsync(W.map_n, 0, sizeof(int) * ((size_t)W.n_maps + 1), s));
    return MML_OK;
}
unsigned wm_blocks(size_t n) { return (unsigned)((n + 255) / 256); }
// the grid of a grid-stride walk over the table's positions: at most 1 024 workgroups
unsigned wm_walk_blocks(const mml_ctx::WorldMap& W) { return std::min(wm_blocks((size_t)W.slots), 1024u); }
// where a sort of the table's keys may stop: above the map numbers in use, and `marker_bit` = 1 bit higher where the empty marker
// is among the keys and has to sort behind every one of them (with more than 512 maps all 64 bits are then compared, and no kept
// key equals the marker)
int wm_end_bit(const mml_ctx::WorldMap& W, int marker_bit) {
    int map_bits = 1;
    while ((1 << map_bits) < W.n_maps) ++map_bits;
    return std::min(MML_WM_MAP_SHIFT + map_bits + marker_bit, 64);
}
// the table is about to be written: whatever was derived from it (the surfel cache) is stale from here on
void wm_touch(mml_ctx::WorldMap& W) { ++W.version; }
WmMom wm_mom(const mml_ctx::WorldMap& W) { return WmMom{W.mom[0], W.mom[1], W.mom[2]}; }
// a moments array is given on a surfel map and on no other
int wm_moments_arg(mml_ctx* ctx, const char* who, const char* name, const void* moments) {
    const bool surfels = ctx->world.surfels;
    if ((moments != nullptr) == surfels) return MML_OK;
    return mml_refuse(ctx, MML_ERR_INVALID, "%s: %s must be %s", who, name, surfels ? "given: the map holds surfels" : "NULL: the map is a plain one");
}

// THE REBUILD.  An open-addressing table has no way to free a position inside a probe chain (every key value is in use, there is
// no tombstone), so a call that removes voxels takes the `n` survivors out -- the positions vals[0..n), whose keys are in R.keys
// already, gathered into R --, clears the keys and puts the rows back by claim; the put writes the total and what C says of the
// maps' counts.  Enqueue only.
int wm_rebuild(mml_ctx* ctx, const unsigned* vals, WmRows R, size_t n, WmCounts C, hipStream_t s) {
    mml_ctx::WorldMap& W = ctx->world;
    if (n) hipLaunchKernelGGL(k_wm_gather, dim3(wm_blocks(n)), dim3(256), 0, s, vals, (int)n, W.sum, W.count, wm_mom(W), R);
    MML_HIP(hipMemsetAsync(W.keys, 0xff, sizeof(unsigned long long) * W.slots, s));
    C.total = (int)n;
    hipLaunchKernelGGL(k_wm_put, dim3(n ? wm_blocks(n) : 1), dim3(256), 0, s, R, (int)n, W.keys, W.slots, W.sum, W.count, wm_mom(W), W.map_n, W.n_maps, C);
    MML_HIP(hipGetLastError());
    return MML_OK;
}
// the `n` rows R up to the caller's arrays (moments on a surfel map), one synchronisation, the keys unpacked on the host into
// voxel indices and, where wanted, map numbers
int wm_rows_up(mml_ctx* ctx, WmRows R, size_t n, int* out_map, int* ijk, float* sums, int* counts, float* moments, hipStream_t s) {
    std::vector<unsigned long long> h_keys(n);
    MML_HIP(hipMemcpyAsync(sums, R.sum, sizeof(float4) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(counts, R.n, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    if (R.mom) MML_HIP(hipMemcpyAsync(moments, R.mom, sizeof(float4) * 3 * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(h_keys.data(), R.keys, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (size_t r = 0; r < n; ++r) {
        int map;
        mml_wm_unkey(h_keys[r], map, ijk[3 * r], ijk[3 * r + 1], ijk[3 * r + 2]);
        if (out_map) out_map[r] = map;
    }
    return MML_OK;
}

// mml_world_map_create and _create_opts
int wm_create(mml_ctx* ctx, int n_maps, float leaf, long capacity_voxels, unsigned flags) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_maps >= 1 && n_maps <= MML_WM_MAPS_MAX, MML_ERR_INVALID, "mml_world_map_create: n_maps outside 1..1024");
    MML_REQUIRE(isfinite(leaf) && leaf > 0.f, MML_ERR_INVALID, "mml_world_map_create: leaf must be finite and positive");
    MML_REQUIRE(capacity_voxels >= 1 && capacity_voxels <= (1L << 29), MML_ERR_INVALID, "mml_world_map_create: capacity_voxels outside 1..2^29");
    if (flags & ~MML_WM_SURFELS) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_create_opts: unknown flag bits 0x%x (MML_WM_SURFELS is 0x%x)", flags & ~MML_WM_SURFELS, MML_WM_SURFELS);
    mml_ctx::WorldMap& W = ctx->world;
    if (W.n_maps) return mml_refuse(ctx, MML_ERR_STATE, "mml_world_map_create: the context has a world map of %d maps already", W.n_maps);
    MML_HIP(hipSetDevice(ctx->device));
    const unsigned long long slots = mml_wm_table_slots(capacity_voxels);
    const bool surfels = (flags & MML_WM_SURFELS) != 0;
    // (a plain map allocates what it always did)
    int rc = surfels ? W.mem.reserve(ctx, {mml_part(W.keys, (size_t)slots), mml_part(W.sum, (size_t)slots), mml_part(W.count, (size_t)slots),
                                           mml_part(W.map_n, (size_t)n_maps + 1), mml_part(W.mom[0], (size_t)slots),
                                           mml_part(W.mom[1], (size_t)slots), mml_part(W.mom[2], (size_t)slots)})
                     : W.mem.reserve(ctx, {mml_part(W.keys, (size_t)slots), mml_part(W.sum, (size_t)slots), mml_part(W.count, (size_t)slots),
                                           mml_part(W.map_n, (size_t)n_maps + 1)});
    if (rc != MML_OK) return rc;
    W.surfels = surfels;
    W.n_maps = n_maps;
    W.leaf = leaf;
    W.capacity = capacity_voxels;
    W.slots = slots;
    wm_touch(W);
    hipStream_t s = MML_STREAM(ctx);
    rc = wm_clear(ctx, s);
    if (rc == MML_OK && hipStreamSynchronize(s) != hipSuccess) rc = mml_refuse(ctx, MML_ERR_HIP, "mml_world_map_create: hipStreamSynchronize failed");
    if (rc != MML_OK) W.release();
    return rc;
}
}  // namespace

int mml_world_map_create(mml_ctx* ctx, int n_maps, float leaf, long capacity_voxels) { return wm_create(ctx, n_maps, leaf, capacity_voxels, 0u); }
int mml_world_map_create_opts(mml_ctx* ctx, int n_maps, float leaf, long capacity_voxels, unsigned flags) {
    return wm_create(ctx, n_maps, leaf, capacity_voxels, flags);
}

int mml_world_map_destroy(mml_ctx* ctx) {
    int rc = wm_enter(ctx, "mml_world_map_destroy");
    if (rc != MML_OK) return rc;
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    ctx->world.release();
    return MML_OK;
}

int mml_world_map_size(mml_ctx* ctx, int map, long* n_voxels) {
    int rc = wm_enter(ctx, "mml_world_map_size");
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    MML_REQUIRE(n_voxels != nullptr, MML_ERR_INVALID, "mml_world_map_size: null n_voxels");
    if (map < -1 || map >= W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_size: map %d outside [-1, %d)", map, W.n_maps);
    int* h = reinterpret_cast<int*>(mml_stage_alloc(ctx, 1));
    MML_HIP(hipMemcpyAsync(h, W.map_n + (map < 0 ? W.n_maps : map), sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    *n_voxels = h[0];
    return MML_OK;
}

int mml_world_map_reset(mml_ctx* ctx, int map) {
    int rc = wm_enter(ctx, "mml_world_map_reset");
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    if (map < -1 || map >= W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_reset: map %d outside [-1, %d)", map, W.n_maps);
    hipStream_t s = MML_STREAM(ctx);
    wm_touch(W);
    if (map < 0) return wm_clear(ctx, s);
    // One map of several: the other maps' voxels are the survivors of a rebuild (wm_rebuild), sized by their number.
    int* h = reinterpret_cast<int*>(mml_stage_alloc(ctx, 1));
    MML_HIP(hipMemcpyAsync(h, W.map_n + map, sizeof(int), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(h + 1, W.map_n + W.n_maps, sizeof(int), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    if (h[0] == 0) return MML_OK;
    const size_t m = (size_t)(h[1] - h[0]);
    MmlCarve<16> c;
    const MmlField<unsigned long long> f_keys = c.take<unsigned long long>(m);
    const MmlField<unsigned> f_vals = c.take<unsigned>(m);
    const MmlField<float4> f_sum = c.take<float4>(m);
    const MmlField<int> f_n = c.take<int>(m);
    const MmlField<int> f_cur = c.take<int>(1);
    const MmlField<float4> f_mom = c.take<float4>(W.surfels ? 3 * m : 0);
    rc = W.scratch.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    char* d = W.scratch.d;
    MML_HIP(hipMemsetAsync(f_cur.in(d), 0, sizeof(int), s));
    if (m) {
        MML_HIP(hipMemsetAsync(f_vals.in(d), 0, f_vals.bytes(), s));  // (every entry a table position, whatever the walk finds)
        hipLaunchKernelGGL(k_wm_collect<true>, dim3(wm_walk_blocks(W)), dim3(256), 0, s, W.keys, W.slots, map, (int)m, f_cur.in(d), f_keys.in(d),
                           f_vals.in(d));
    }
    return wm_rebuild(ctx, f_vals.in(d), WmRows{f_keys.in(d), f_sum.in(d), f_n.in(d), W.surfels ? f_mom.in(d) : nullptr}, m,
                      WmCounts{nullptr, nullptr, 0, map, -1, -1}, s);
}

int mml_world_map_add(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* T_wl, unsigned label_mask,
                      mml_world_map_info* info) {
    int rc = wm_enter(ctx, "mml_world_map_add");
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    MML_REQUIRE(count >= 1 && count <= 65535, MML_ERR_INVALID, "mml_world_map_add: count outside 1..65535 (the grid's second dimension)");
    MML_REQUIRE(first_slot >= 0 && first_slot + count <= ctx->B, MML_ERR_INVALID, "mml_world_map_add: slot range out of bounds");
    MML_REQUIRE(map_of_slot != nullptr && T_wl != nullptr, MML_ERR_INVALID, "mml_world_map_add: null map_of_slot / T_wl");
    MML_REQUIRE((label_mask & 7u) != 0, MML_ERR_INVALID, "mml_world_map_add: label_mask selects no label");
    int live = 0;
    for (int i = 0; i < count; ++i) {
        if (map_of_slot[i] < -1 || map_of_slot[i] >= W.n_maps)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_add: map %d of slot %d outside [-1, %d)", map_of_slot[i], first_slot + i, W.n_maps);
        live += map_of_slot[i] >= 0;
    }
    if (!ctx->uploads.empty() && (rc = mml_uploads_wait(ctx, first_slot, count)) != MML_OK) return rc;
    if (info) memset(info, 0, sizeof(*info));
    hipStream_t s = MML_STREAM(ctx);
    if (live == 0) {
        if (info) return mml_world_map_size(ctx, -1, &info->n_voxels_total);
        return MML_OK;
    }
    rc = mml_cloud_settle(ctx, first_slot, count);  // (as every reader of the cloud outside the step: mml_internal.h, und_pending)
    if (rc != MML_OK) return rc;
    const long long bound = (long long)live * ctx->NT;
    if (bound > INT_MAX) return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_world_map_add: %d slots of %d points exceed 2^31 - 1 points per call", live, ctx->NT);
    const size_t n = (size_t)bound;
    // scratch and tables, all before the first launch
    MmlCarve<16> c;
    const MmlField<float4> f_pts = c.take<float4>(n);
    const MmlField<unsigned long long> f_keys = c.take<unsigned long long>(2 * n);
    const MmlField<unsigned> f_vals = c.take<unsigned>(2 * n);
    const MmlField<int> f_flag = c.take<int>(n), f_pos = c.take<int>(n), f_hit = c.take<int>(n);
    rc = W.scratch.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    const int end_bit = wm_end_bit(W, 1);  // (the keys were preset to the empty marker)
    rc = W.tmp.reserve(ctx, mml_sort_pairs_bytes<unsigned long long>(n, end_bit, s), s);
    if (rc != MML_OK) return rc;
    MmlCarve<16> t;
    const MmlField<WmRow> f_rows = t.take<WmRow>((size_t)count);
    const MmlField<int> f_cnt = t.take<int>(WM_COUNTERS + 1);  // the counters, and behind them (read-back only) the table's total
    const MmlField<float4> f_org = t.take<float4>(W.surfels ? (size_t)live : 0);  // a surfel map: the origin of every slot that takes part
    rc = W.tab.reserve(ctx, t.bytes(), s);
    if (rc != MML_OK) return rc;
    // (the pinned twin is free: the last call that used it waited for its read-back, which ran behind its copy down)
    WmRow* h_rows = f_rows.in(W.tab.h);
    int off = 0;
    for (int i = 0; i < count; ++i) {
        memset(static_cast<void*>(&h_rows[i]), 0, sizeof(WmRow));
        memcpy(h_rows[i].T, T_wl + 16 * (size_t)i, sizeof(double) * 16);
        h_rows[i].map = map_of_slot[i];
        h_rows[i].off = off;
        if (map_of_slot[i] < 0) continue;
        if (W.surfels) {  // (off = NT x the slot's place among those that take part: k_wm_insert<true> divides an ordinal by NT)
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            mml_wm_origin(h_rows[i].T, o.x, o.y, o.z);
            f_org.in(W.tab.h)[off / ctx->NT] = o;
        }
        off += ctx->NT;
    }
    int* h_cnt = f_cnt.in(W.tab.h);
    memset(h_cnt, 0, f_cnt.bytes());
    MML_HIP(hipMemcpyAsync(W.tab.d, W.tab.h, t.bytes(), hipMemcpyHostToDevice, s));
    char* d = W.scratch.d;
    unsigned long long *keys = f_keys.in(d), *keys2 = keys + n;
    unsigned *vals = f_vals.in(d), *vals2 = vals + n;
    int* d_cnt = f_cnt.in(W.tab.d);
    MML_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * n, s));
    MML_HIP(hipMemsetAsync(vals, 0, sizeof(unsigned) * n, s));
    hipLaunchKernelGGL(k_wm_keys, dim3(wm_blocks((size_t)ctx->NT), count), dim3(256), 0, s, slot_arrays(ctx, first_slot), f_rows.in(W.tab.d),
                       mml_wm_inv_leaf(W.leaf), label_mask & 7u, f_pts.in(d), keys, vals, d_cnt);
    rc = mml_sort_pairs(ctx, W.tmp, keys, keys2, vals, vals2, n, end_bit, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_run_heads<unsigned long long>, dim3(wm_blocks(n)), dim3(256), 0, s, keys2, (int)n, 0, MML_WM_EMPTY, f_flag.in(d));
    rc = mml_exclusive_scan(ctx, W.tmp, f_flag.in(d), f_pos.in(d), n, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_wm_lookup, dim3(wm_blocks(n)), dim3(256), 0, s, keys2, f_flag.in(d), (int)n, W.keys, W.slots, f_hit.in(d), d_cnt);
    MML_HIP(hipGetLastError());
    // the call's one read-back
    MML_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(int) * WM_COUNTERS, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(h_cnt + WM_COUNTERS, W.map_n + W.n_maps, sizeof(int), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    const long total = h_cnt[WM_COUNTERS], misses = h_cnt[WM_MISSES];
    if (total + misses > W.capacity)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_world_map_add: %ld voxels held + %ld new ones exceed capacity_voxels %ld; nothing was added", total,
                          misses, W.capacity);
    wm_touch(W);
    if (h_cnt[WM_DISTINCT] && W.surfels)
        hipLaunchKernelGGL(k_wm_insert<true>, dim3(wm_blocks(n)), dim3(256), 0, s, keys2, vals2, f_flag.in(d), f_hit.in(d), (int)n, f_pts.in(d), W.keys,
                           W.slots, W.sum, W.count, W.map_n, W.n_maps,
                           WmMomentArgs<true>{W.mom[0], W.mom[1], W.mom[2], f_org.in(W.tab.d), W.leaf, ctx->NT});
    else if (h_cnt[WM_DISTINCT])
        hipLaunchKernelGGL(k_wm_insert<false>, dim3(wm_blocks(n)), dim3(256), 0, s, keys2, vals2, f_flag.in(d), f_hit.in(d), (int)n, f_pts.in(d), W.keys,
                           W.slots, W.sum, W.count, W.map_n, W.n_maps, WmMomentArgs<false>{});
    MML_HIP(hipGetLastError());
    if (info) {
        info->n_points = h_cnt[WM_POINTS];
        info->n_kept = h_cnt[WM_KEPT];
        info->n_nonfinite = h_cnt[WM_NONFINITE];
        info->n_out_of_range = h_cnt[WM_RANGE];
        info->n_masked = h_cnt[WM_MASKED];
        info->n_new_voxels = misses;
        info->n_voxels_total = total + misses;
    }
    return MML_OK;
}

namespace {
// The three downloads and the export: the occupied positions of the map collected, sorted by key and gathered -- the chain is this
// function's and nobody else's; `what` chooses the gather kernel and the floats per voxel.  The export (WM_RAW) hands up whole rows
// (wm_rows_up): the stored sums into `out`, the counts, the sorted keys as voxel indices into `ijk` and, on a surfel map, the
// moments into `moments`.
enum WmWhat { WM_CENTROIDS = 4, WM_MOMENTS = 12, WM_SURFELS = 8, WM_RAW = 16 };  // (the value: floats per voxel; WM_RAW: 4, or 16 with moments)
int wm_download(mml_ctx* ctx, const char* who, WmWhat what, int map, float* out, int* out_count, long capacity, long* n_voxels,
                int* ijk = nullptr, float* moments = nullptr) {
    int rc = wm_enter(ctx, who);
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    if (what != WM_CENTROIDS && what != WM_RAW && !W.surfels)
        return mml_refuse(ctx, MML_ERR_STATE, "%s: the world map was created without MML_WM_SURFELS (mml_world_map_create_opts)", who);
    if (!n_voxels) return mml_refuse(ctx, MML_ERR_INVALID, "%s: null n_voxels", who);
    if (map < 0 || map >= W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "%s: map %d outside [0, %d)", who, map, W.n_maps);
    if (what == WM_RAW && (out || out_count || ijk || moments)) {  // (all NULL: the sizing call)
        if (!out || !out_count || !ijk) return mml_refuse(ctx, MML_ERR_INVALID, "%s: ijk, sums and counts are given together or not at all", who);
        if ((rc = wm_moments_arg(ctx, who, "moments", moments)) != MML_OK) return rc;
    }
    rc = mml_world_map_size(ctx, map, n_voxels);
    if (rc != MML_OK || !out || *n_voxels == 0) return rc;
    if (capacity < *n_voxels) return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: map %d holds %ld voxels, capacity is %ld", who, map, *n_voxels, capacity);
    hipStream_t s = MML_STREAM(ctx);
    const size_t n = (size_t)*n_voxels;
    MmlCarve<16> c;
    const MmlField<unsigned long long> f_keys = c.take<unsigned long long>(2 * n);
    const MmlField<unsigned> f_vals = c.take<unsigned>(2 * n);
    const MmlField<float4> f_out = c.take<float4>((what == WM_RAW ? 1 : (size_t)what / 4) * n);
    const MmlField<float4> f_mom = c.take<float4>(what == WM_RAW && W.surfels ? 3 * n : 0);
    const MmlField<int> f_n = c.take<int>(n);
    const MmlField<int> f_cur = c.take<int>(1);
    rc = W.scratch.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    rc = W.tmp.reserve(ctx, mml_sort_pairs_bytes<unsigned long long>(n, MML_WM_MAP_SHIFT, s), s);
    if (rc != MML_OK) return rc;
    char* d = W.scratch.d;
    unsigned long long* keys = f_keys.in(d);
    unsigned* vals = f_vals.in(d);
    MML_HIP(hipMemsetAsync(f_cur.in(d), 0, sizeof(int), s));
    MML_HIP(hipMemsetAsync(vals, 0, sizeof(unsigned) * n, s));  // (every entry a table position, whatever the walk finds)
    hipLaunchKernelGGL(k_wm_collect<false>, dim3(wm_walk_blocks(W)), dim3(256), 0, s, W.keys, W.slots, map, (int)n, f_cur.in(d), keys, vals);
    rc = mml_sort_pairs(ctx, W.tmp, keys, keys + n, vals, vals + n, n, MML_WM_MAP_SHIFT, s);  // (the map number is the same in all)
    if (rc != MML_OK) return rc;
    const WmRows R = what == WM_RAW ? WmRows{keys + n, f_out.in(d), f_n.in(d), W.surfels ? f_mom.in(d) : nullptr}
                                    : WmRows{nullptr, nullptr, nullptr, f_out.in(d)};
    if (what == WM_CENTROIDS)
        hipLaunchKernelGGL(k_wm_centroids, dim3(wm_blocks(n)), dim3(256), 0, s, vals + n, (int)n, W.sum, W.count, f_out.in(d), f_n.in(d));
    else if (what == WM_SURFELS)
        hipLaunchKernelGGL(k_wm_surfels, dim3(wm_blocks(n)), dim3(256), 0, s, vals + n, (int)n, wm_mom(W), W.count, f_out.in(d));
    else  // the stored accumulators as they are: the moments alone, or the export's rows
        hipLaunchKernelGGL(k_wm_gather, dim3(wm_blocks(n)), dim3(256), 0, s, vals + n, (int)n, W.sum, W.count, wm_mom(W), R);
    MML_HIP(hipGetLastError());
    if (what == WM_RAW) return wm_rows_up(ctx, R, n, nullptr, ijk, out, out_count, moments, s);
    MML_HIP(hipMemcpyAsync(out, f_out.in(d), f_out.bytes(), hipMemcpyDeviceToHost, s));
    if (out_count) MML_HIP(hipMemcpyAsync(out_count, f_n.in(d), sizeof(int) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    return MML_OK;
}
}  // namespace

int mml_world_map_download(mml_ctx* ctx, int map, float* out_xyzi, int* out_count, long capacity, long* n_voxels) {
    return wm_download(ctx, "mml_world_map_download", WM_CENTROIDS, map, out_xyzi, out_count, capacity, n_voxels);
}
int mml_world_map_download_moments(mml_ctx* ctx, int map, float* out, long capacity, long* n_voxels) {
    return wm_download(ctx, "mml_world_map_download_moments", WM_MOMENTS, map, out, nullptr, capacity, n_voxels);
}
int mml_world_map_download_surfels(mml_ctx* ctx, int map, float* out, long capacity, long* n_voxels) {
    return wm_download(ctx, "mml_world_map_download_surfels", WM_SURFELS, map, out, nullptr, capacity, n_voxels);
}
int mml_world_map_export(mml_ctx* ctx, int map, int* ijk, float* sums, int* counts, float* moments, long capacity, long* n_voxels) {
    return wm_download(ctx, "mml_world_map_export", WM_RAW, map, sums, counts, capacity, n_voxels, ijk, moments);
}

int mml_world_map_import(mml_ctx* ctx, int map, long n, const int* ijk, const float* sums, const int* counts, const float* moments) {
    int rc = wm_enter(ctx, "mml_world_map_import");
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    // the arguments, on the host, before any device work
    if (map < 0 || map >= W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_import: map %d outside [0, %d)", map, W.n_maps);
    MML_REQUIRE(n >= 0 && n <= (1L << 29), MML_ERR_INVALID, "mml_world_map_import: n outside 0..2^29");
    MML_REQUIRE(n == 0 || (ijk && sums && counts), MML_ERR_INVALID, "mml_world_map_import: null ijk / sums / counts");
    if (n > 0 && (rc = wm_moments_arg(ctx, "mml_world_map_import", "moments", moments)) != MML_OK) return rc;
    if (n == 0) return MML_OK;
    std::vector<unsigned long long> h_keys((size_t)n);
    for (long r = 0; r < n; ++r) {
        const int i = ijk[3 * r], j = ijk[3 * r + 1], k = ijk[3 * r + 2];
        const bool in = i >= -MML_WM_HALF && i < MML_WM_HALF && j >= -MML_WM_HALF && j < MML_WM_HALF && k >= -MML_WM_HALF && k < MML_WM_HALF;
        if (!in || mml_wm_key(map, i, j, k) == MML_WM_EMPTY)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_import: row %ld: voxel (%d, %d, %d) %s", r, i, j, k,
                              in ? "of this map packs to the free marker" : "outside [-2^17, 2^17)");
        if (counts[r] < 1) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_import: row %ld: count %d < 1", r, counts[r]);
        h_keys[(size_t)r] = mml_wm_key(map, i, j, k);
    }
    {
        std::vector<unsigned long long> sorted(h_keys);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) {
            int m, i, j, k;
            mml_wm_unkey(*dup, m, i, j, k);
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_import: voxel (%d, %d, %d) is given twice", i, j, k);
        }
    }
    hipStream_t s = MML_STREAM(ctx);
    const size_t m = (size_t)n;
    MmlCarve<16> c;
    const MmlField<unsigned long long> f_keys = c.take<unsigned long long>(m);
    const MmlField<float4> f_sum = c.take<float4>(m);
    const MmlField<int> f_n = c.take<int>(m);
    const MmlField<float4> f_mom = c.take<float4>(W.surfels ? 3 * m : 0);
    const MmlField<int> f_cnt = c.take<int>(2);  // the hits, and behind them (read-back only) the table's total
    rc = W.scratch.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    char* d = W.scratch.d;
    MML_HIP(hipMemsetAsync(f_cnt.in(d), 0, sizeof(int) * 2, s));
    MML_HIP(hipMemcpyAsync(f_keys.in(d), h_keys.data(), f_keys.bytes(), hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(f_sum.in(d), sums, f_sum.bytes(), hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(f_n.in(d), counts, f_n.bytes(), hipMemcpyHostToDevice, s));
    if (W.surfels) MML_HIP(hipMemcpyAsync(f_mom.in(d), moments, f_mom.bytes(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_wm_import_find, dim3(wm_blocks(m)), dim3(256), 0, s, f_keys.in(d), (int)m, W.keys, W.slots, f_cnt.in(d));
    MML_HIP(hipGetLastError());
    // the read-back: the refusal point of mml_world_map_add -- only scratch has been written up to here
    int h_cnt[2] = {0, 0};
    MML_HIP(hipMemcpyAsync(h_cnt, f_cnt.in(d), sizeof(int), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(h_cnt + 1, W.map_n + W.n_maps, sizeof(int), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    if (h_cnt[0] > 0)
        return mml_refuse(ctx, MML_ERR_STATE, "mml_world_map_import: %d of the %ld voxels are present in map %d already; nothing was imported", h_cnt[0], n, map);
    if ((long)h_cnt[1] + n > W.capacity)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_world_map_import: %d voxels held + %ld imported exceed capacity_voxels %ld; nothing was imported",
                          h_cnt[1], n, W.capacity);
    wm_touch(W);
    hipLaunchKernelGGL(k_wm_put, dim3(wm_blocks(m)), dim3(256), 0, s, WmRows{f_keys.in(d), f_sum.in(d), f_n.in(d), W.surfels ? f_mom.in(d) : nullptr}, (int)m,
                       W.keys, W.slots, W.sum, W.count, wm_mom(W), W.map_n, W.n_maps, WmCounts{nullptr, nullptr, 0, -1, -1, map});
    MML_HIP(hipGetLastError());
    MML_HIP(hipStreamSynchronize(s));  // (the caller's arrays and the key vector were the copies' sources)
    return MML_OK;
}

int mml_wm_index_box(float leaf, const float* lo_xyz, const float* hi_xyz, int* lo, int* hi) {
    if (!lo_xyz || !hi_xyz || !lo || !hi) return MML_ERR_INVALID;
    return mml_wme_index_box(leaf, lo_xyz, hi_xyz, lo, hi) == 0 ? MML_OK : MML_ERR_INVALID;
}

// Scratch per voxel of capacity_voxels (the lists are sized before the walk has counted): 8 + 4 for the two lists, which share
// one pair of arrays; past a dry run 16 + 4 for the rows taken out (the evicted ones in front, the survivors behind them) and,
// on a surfel map, 48 for their moments; 8 + 4 more for the sorted pairs when rows are handed back.
int mml_world_map_evict(mml_ctx* ctx, int n_rules, const mml_wm_evict_rule* rules, unsigned flags, mml_wm_evict_info* info, long capacity,
                        int* out_map, int* out_ijk, float* out_sums, int* out_counts, float* out_moments, long* n_evicted) {
    int rc = wm_enter(ctx, "mml_world_map_evict");
    if (rc != MML_OK) return rc;
    mml_ctx::WorldMap& W = ctx->world;
    MML_REQUIRE(rules != nullptr, MML_ERR_INVALID, "mml_world_map_evict: null rules");
    if (n_rules < 1 || n_rules > W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: n_rules %d outside 1..%d (n_maps)", n_rules, W.n_maps);
    if (flags & ~MML_WM_EVICT_DRY)
        return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: unknown flag bits 0x%x (MML_WM_EVICT_DRY is 0x%x)", flags & ~MML_WM_EVICT_DRY, MML_WM_EVICT_DRY);
    if (capacity < 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: capacity %ld < 0", capacity);
    std::vector<int> rule_of((size_t)W.n_maps, -1);
    for (int r = 0; r < n_rules; ++r) {
        const mml_wm_evict_rule& R = rules[r];
        if (R.map < 0 || R.map >= W.n_maps) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: rule %d: map %d outside [0, %d)", r, R.map, W.n_maps);
        if (rule_of[(size_t)R.map] >= 0)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: rule %d: map %d is named by rule %d already", r, R.map, rule_of[(size_t)R.map]);
        if (R.mode != MML_WM_EVICT_OUTSIDE && R.mode != MML_WM_EVICT_INSIDE && R.mode != MML_WM_EVICT_NOBOX)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: rule %d: unknown mode %d", r, R.mode);
        if (R.min_count < 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: rule %d: min_count %d < 0", r, R.min_count);
        rule_of[(size_t)R.map] = r;
    }
    const bool rows = out_ijk != nullptr, dry = (flags & MML_WM_EVICT_DRY) != 0;
    if (rows) {
        if (!out_map || !out_sums || !out_counts)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: out_map, out_ijk, out_sums and out_counts are given together or not at all");
        if ((rc = wm_moments_arg(ctx, "mml_world_map_evict", "out_moments", out_moments)) != MML_OK) return rc;
    } else {
        if (out_map || out_sums || out_counts || out_moments)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: out_map, out_ijk, out_sums and out_counts are given together or not at all");
        if (capacity != 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_evict: capacity %ld without out arrays (0 drops the rows)", capacity);
    }
    hipStream_t s = MML_STREAM(ctx);
    // scratch and tables, all before the first launch
    const size_t cap = (size_t)W.capacity;
    const bool sorted = rows && !dry;
    MmlCarve<16> c;
    const MmlField<unsigned long long> f_keys = c.take<unsigned long long>(cap);
    const MmlField<unsigned> f_vals = c.take<unsigned>(cap);
    const MmlField<unsigned long long> f_keys2 = c.take<unsigned long long>(sorted ? cap : 0);
    const MmlField<unsigned> f_vals2 = c.take<unsigned>(sorted ? cap : 0);
    const MmlField<float4> f_sum = c.take<float4>(dry ? 0 : cap);
    const MmlField<int> f_n = c.take<int>(dry ? 0 : cap);
    const MmlField<float4> f_mom = c.take<float4>(!dry && W.surfels ? 3 * cap : 0);
    rc = W.scratch.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    const int end_bit = wm_end_bit(W, 0);  // (no entry of the evicted list is the free marker)
    if (sorted && (rc = W.tmp.reserve(ctx, mml_sort_pairs_bytes<unsigned long long>(cap, end_bit, s), s)) != MML_OK) return rc;
    MmlCarve<16> t;
    const MmlField<int> f_of = t.take<int>((size_t)W.n_maps);
    const MmlField<mml_wm_evict_rule> f_rules = t.take<mml_wm_evict_rule>((size_t)n_rules);
    const MmlField<int> f_cnt = t.take<int>(WME_RULES + 2 * (size_t)n_rules);
    rc = W.tab.reserve(ctx, t.bytes(), s);
    if (rc != MML_OK) return rc;
    // (the pinned twin is free: the last call that used it waited for its read-back, which ran behind its copy down)
    memcpy(f_of.in(W.tab.h), rule_of.data(), sizeof(int) * rule_of.size());
    memcpy(static_cast<void*>(f_rules.in(W.tab.h)), rules, sizeof(mml_wm_evict_rule) * (size_t)n_rules);
    int* h_cnt = f_cnt.in(W.tab.h);
    memset(h_cnt, 0, f_cnt.bytes());
    MML_HIP(hipMemcpyAsync(W.tab.d, W.tab.h, t.bytes(), hipMemcpyHostToDevice, s));
    char* d = W.scratch.d;
    int* d_cnt = f_cnt.in(W.tab.d);
    const mml_wm_evict_rule* d_rules = f_rules.in(W.tab.d);
    hipLaunchKernelGGL(k_wm_evict_mark, dim3(wm_walk_blocks(W)), dim3(256), 0, s, W.keys, W.slots, W.count, f_of.in(W.tab.d), W.n_maps, d_rules, (int)cap,
                       d_cnt, f_keys.in(d), f_vals.in(d));
    MML_HIP(hipGetLastError());
    // the call's first read-back and its refusal point: only scratch has been written up to here
    MML_HIP(hipMemcpyAsync(h_cnt, d_cnt, f_cnt.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    const size_t n_ev = (size_t)h_cnt[WME_EVICTED], n_sv = (size_t)h_cnt[WME_KEPT];
    if (n_evicted) *n_evicted = (long)n_ev;
    if (info)
        for (int r = 0; r < n_rules; ++r) {
            info[r].n_before = h_cnt[WME_RULES + 2 * r];
            info[r].n_evicted = h_cnt[WME_RULES + 2 * r + 1];
            info[r].n_kept = info[r].n_before - info[r].n_evicted;
            info[r].first_row = 0;  // the evicted rows of the rules that name a smaller map come first
            for (int q = 0; q < n_rules; ++q)
                if (rules[q].map < rules[r].map) info[r].first_row += h_cnt[WME_RULES + 2 * q + 1];
        }
    if (n_ev + n_sv > cap)
        return mml_refuse(ctx, MML_ERR_STATE, "mml_world_map_evict: the table holds %zu voxels, more than capacity_voxels %zu; nothing was evicted", n_ev + n_sv, cap);
    if (dry) return MML_OK;
    if (rows && capacity < (long)n_ev)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_world_map_evict: %zu voxels to evict, capacity is %ld rows; nothing was evicted", n_ev, capacity);
    if (n_ev == 0) return MML_OK;
    wm_touch(W);
    // the rows taken out, in one set of arrays: the evicted ones in front (in key order, when they are handed back), the survivors
    // behind them
    float4* mom = W.surfels ? f_mom.in(d) : nullptr;
    const WmRows ev = {f_keys2.in(d), f_sum.in(d), f_n.in(d), mom};
    const WmRows sv = {f_keys.in(d) + (cap - n_sv), ev.sum + n_ev, ev.n + n_ev, mom ? mom + 3 * n_ev : nullptr};
    if (rows) {
        rc = mml_sort_pairs(ctx, W.tmp, f_keys.in(d), f_keys2.in(d), f_vals.in(d), f_vals2.in(d), n_ev, end_bit, s);
        if (rc != MML_OK) return rc;
        hipLaunchKernelGGL(k_wm_gather, dim3(wm_blocks(n_ev)), dim3(256), 0, s, f_vals2.in(d), (int)n_ev, W.sum, W.count, wm_mom(W), ev);
    }
    // every ruled map's count becomes n_before - n_evicted of its rule, from the device's counters
    rc = wm_rebuild(ctx, f_vals.in(d) + (cap - n_sv), sv, n_sv, WmCounts{d_rules, d_cnt + WME_RULES, n_rules, -1, -1, -1}, s);
    if (rc != MML_OK || !rows) return rc;
    return wm_rows_up(ctx, ev, n_ev, out_map, out_ijk, out_sums, out_counts, out_moments, s);  // the call's second synchronisation
}

// The surfel cache of a surfel map, valid for the table as it is: allocated on first use, rebuilt when a call has written the table
// since it was filled.  Enqueue only; a failed allocation is reported before any launch.
int mml_wm_cache_ready(mml_ctx* ctx) {
    mml_ctx::WorldMap& W = ctx->world;
    if (!W.cache) {
        const hipError_t e = W.mem.alloc(&W.cache, (size_t)W.slots);
        if (e != hipSuccess) return mml_mem_fail(ctx, "mml_world_map_score: the surfel cache (16 bytes per table position), hipMalloc", e);
        W.cache_version = 0;
    }
    if (W.cache_version == W.version) return MML_OK;
    MmlStageScope t(ctx, "wm_surfel_cache");
    hipLaunchKernelGGL(k_wm_surfel_cache, dim3(wm_blocks((size_t)W.slots)), dim3(256), 0, MML_STREAM(ctx), W.keys, W.slots, wm_mom(W), W.count, W.cache);
    MML_HIP(hipGetLastError());
    W.cache_version = W.version;
    return MML_OK;
}
