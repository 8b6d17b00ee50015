// map_banks.hip -- map banks: N further local maps per context, and which scan slot is matched against which.
//   A bank holds what the context's own local map holds (MmlMapBank, mml_internal.h); set, increment, reset and download run
//   the code of the single-map calls on the bank's state (MmlMapRef).  The association kernels of a launch with a bound slot read
//   the maps' grid descriptors from two device-resident tables, (banks + 1) rows x 2 kinds each -- the local maps and the global
//   cube maps --, through the per-slot bank array (map_assoc.hip, the BANKED forms); this file keeps the three device arrays
//   equal to the host's state.
//   A bank has its own global cube map (MmlCubeMatch / MmlCubeLive, mml_internal.h): the mml_map_bank_global_* calls run the code
//   of the own-map calls on it (MmlCubeRef): one chain of launches for n stores (map_global.hip), which the *_segmented forms
//   and both appends run once for all n banks and the loop increment once per bank.  The context's OWN cube map and a bound
//   slot exclude each other.
#include <string.h>

#include <algorithm>

#include "mml_internal.h"

namespace {

int enter(mml_ctx* ctx) {
    MML_HIP(hipSetDevice(ctx->device));
    return mml_sync_all(ctx);
}

int check_bank(mml_ctx* ctx, int bank) {
    const int n = (int)ctx->banks.bank.size();
    if (n == 0) return mml_refuse(ctx, MML_ERR_STATE, "the context has no map banks (mml_map_banks_create)");
    if (bank < 0 || bank >= n) return mml_refuse(ctx, MML_ERR_INVALID, "map bank %d outside [0, %d)", bank, n);
    return MML_OK;
}

int check_slot_range(mml_ctx* ctx, int first, int count) {
    if (count < 1 || first < 0 || (long)first + count > ctx->B)
        return mml_refuse(ctx, MML_ERR_INVALID, "slots [%d, %d + %d) outside [0, %d)", first, first, count, ctx->B);
    return MML_OK;
}

// n banks (and, where given, n slots) in range, no bank twice: the argument checks of the calls that work n banks through
int check_distinct_banks(mml_ctx* ctx, int n, const int* banks, const int* slots, const char* who) {
    for (int i = 0; i < n; ++i) {
        int rc = check_bank(ctx, banks[i]);
        if (rc == MML_OK && slots) rc = check_slot_range(ctx, slots[i], 1);
        if (rc != MML_OK) return rc;
    }
    std::vector<int> seen(banks, banks + n);
    std::sort(seen.begin(), seen.end());
    const auto dup = std::adjacent_find(seen.begin(), seen.end());
    if (dup != seen.end()) return mml_refuse(ctx, MML_ERR_INVALID, "map bank %d appears twice in one %s", *dup, who);
    return MML_OK;
}

}  // namespace

int mml_assoc_ready(mml_ctx* ctx, int first, int count, const char* who) {
    MmlBanks& K = ctx->banks;
    bool bound = false;
    for (int i = 0; i < count; ++i) {
        const int bank = K.n_bound ? K.slot_bank[(size_t)first + i] : -1;
        if (bank < 0) {
            if (!(ctx->have_map[0] && ctx->have_map[1])) return mml_refuse(ctx, MML_ERR_STATE, "%s before both maps were set", who);
            continue;
        }
        if (ctx->cmatch.have_gmap[0] || ctx->cmatch.have_gmap[1])
            return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d is bound to map bank %d and the context's own global cube map is set (a bank has its own)",
                              who, first + i, bank);
        bound = true;
    }
    if (!bound || !K.dirty) return MML_OK;
    // the device copies, rewritten on the launch stream of an idle context (other lanes may still read the old ones otherwise)
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    const size_t rows = 2 * (K.bank.size() + 1);
    std::vector<MmlMapDesc> t(rows);
    std::vector<MmlCubeDesc> tc(rows);
    for (size_t e = 0; e <= K.bank.size(); ++e)
        for (int k = 0; k < 2; ++k) {
            const MmlCubeMatch& G = e == 0 ? ctx->cmatch : K.bank[e - 1].cmatch;
            MmlCubeDesc& c = tc[2 * e + k];
            memset(static_cast<void*>(&c), 0, sizeof(c));
            c.g = G.ggrid[k];
            c.orig = G.gmap_orig[k];
            c.cube_cnt = G.cube_cnt[k];
            c.have_g = (e > 0 && G.have_gmap[k]) ? 1 : 0;  // (entry 0: never, the exclusion rule above)
            for (int a = 0; a < 3; ++a) c.cen[a] = G.cen[a];
            MmlMapDesc& d = t[2 * e + k];
            memset(static_cast<void*>(&d), 0, sizeof(d));  // (the padding too: the rows are compared and copied as bytes)
            d.g = e == 0 ? ctx->grid[k] : K.bank[e - 1].grid[k];
            d.orig = (e == 0 ? ctx->map_tmp : K.bank[e - 1].map_tmp) + (size_t)k * ctx->MM;
            if (e == 0 && !ctx->have_map[k]) d.g.m = 0;  // (an unset own map: only bound slots are in the launch)
        }
    hipStream_t s = ctx->streams[0];
    MML_HIP(hipMemcpyAsync(K.d_table, t.data(), sizeof(MmlMapDesc) * rows, hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(K.d_cube_table, tc.data(), sizeof(MmlCubeDesc) * rows, hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(K.d_slot_bank, K.slot_bank.data(), sizeof(int) * (size_t)ctx->B, hipMemcpyHostToDevice, s));
    MML_HIP(hipStreamSynchronize(s));  // (`t` and `tc` go out of scope)
    K.dirty = false;
    return MML_OK;
}

extern "C" {

int mml_map_banks_create(mml_ctx* ctx, int n_banks) {
    if (!ctx) return MML_ERR_INVALID;
    if (n_banks < 1 || n_banks > MML_MAP_BANKS_MAX)
        return mml_refuse(ctx, MML_ERR_INVALID, "n_banks must be in [1, %d]", MML_MAP_BANKS_MAX);
    MML_REQUIRE(ctx->banks.bank.empty(), MML_ERR_STATE, "the context has map banks already (mml_map_banks_destroy first)");
    int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    MmlBanks& K = ctx->banks;
    K.bank.resize((size_t)n_banks);
    K.slot_bank.assign((size_t)ctx->B, -1);
    K.n_bound = 0;
    K.dirty = true;
    const size_t MM = (size_t)ctx->MM;
    rc = K.tab_mem.reserve(ctx, {mml_part(K.d_table, 2 * ((size_t)n_banks + 1)), mml_part(K.d_cube_table, 2 * ((size_t)n_banks + 1)),
                                 mml_part(K.d_slot_bank, (size_t)ctx->B)});
    for (int b = 0; b < n_banks && rc == MML_OK; ++b) {
        MmlMapBank& m = K.bank[(size_t)b];
        rc = m.grid_mem.reserve(ctx, {mml_part(m.grid[0].pts, MM), mml_part(m.grid[0].cell_start, 4 * MM + 4096 + 2), mml_part(m.grid[1].pts, MM),
                                      mml_part(m.grid[1].cell_start, 4 * MM + 4096 + 2), mml_part(m.map_tmp, 2 * MM)});
    }
    if (rc != MML_OK) K.release();
    return rc;
}

int mml_map_banks_destroy(mml_ctx* ctx) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    ctx->banks.release();
    return MML_OK;
}

int mml_map_bank_set_local(mml_ctx* ctx, int bank, int kind, const float* xyz, int m) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    MML_REQUIRE(m >= 0 && (m == 0 || xyz), MML_ERR_INVALID, "bad map arguments");
    MML_HIP(hipSetDevice(ctx->device));
    return mml_build_grid(ctx, mml_map_bank(ctx, bank), kind, xyz, m);
}

int mml_map_bank_reset(mml_ctx* ctx, int bank) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    MmlMapBank& b = ctx->banks.bank[(size_t)bank];
    memset(b.ring_n, 0, sizeof(b.ring_n));
    b.local_map_id = 0;
    return MML_OK;
}

int mml_map_bank_download(mml_ctx* ctx, int bank, int kind, float* xyz, int capacity, int* n) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad arguments");
    const MmlMapBank& b = ctx->banks.bank[(size_t)bank];
    MML_REQUIRE(b.have_map[kind], MML_ERR_STATE, "the bank's last map build failed");
    MML_HIP(hipSetDevice(ctx->device));
    const int m = b.grid[kind].m;
    *n = m;
    if (!xyz || m == 0) return MML_OK;
    MML_REQUIRE(capacity >= m, MML_ERR_CAPACITY, "capacity below the map size");
    std::vector<float4> tmp((size_t)m);
    MML_HIP(hipMemcpyAsync(tmp.data(), b.map_tmp + (size_t)kind * ctx->MM, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    for (int i = 0; i < m; ++i) {
        xyz[3 * i] = tmp[i].x;
        xyz[3 * i + 1] = tmp[i].y;
        xyz[3 * i + 2] = tmp[i].z;
    }
    return MML_OK;
}

int mml_slot_bind_bank(mml_ctx* ctx, int first_slot, int count, const int* banks) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(banks != nullptr, MML_ERR_INVALID, "null banks");
    int rc = check_slot_range(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    MmlBanks& K = ctx->banks;
    const int n = (int)K.bank.size();
    bool any = false;
    for (int i = 0; i < count; ++i) {  // every entry is checked before a binding changes
        if (banks[i] < -1 || banks[i] >= n)
            return mml_refuse(ctx, MML_ERR_INVALID, "slot %d: map bank %d outside [-1, %d)", first_slot + i, banks[i], n);
        any = any || banks[i] >= 0;
    }
    if (any && (ctx->cmatch.have_gmap[0] || ctx->cmatch.have_gmap[1]))
        return mml_refuse(ctx, MML_ERR_STATE, "the context's own global cube map is set: a bound slot is matched against its bank's");
    if (n == 0) return MML_OK;  // (all -1 on a context without banks: nothing to record)
    for (int i = 0; i < count; ++i) {
        int& cur = K.slot_bank[(size_t)first_slot + i];
        if (cur == banks[i]) continue;
        K.n_bound += (banks[i] >= 0) - (cur >= 0);
        cur = banks[i];
        K.dirty = true;
    }
    return MML_OK;
}

int mml_slot_bank_get(mml_ctx* ctx, int first_slot, int count, int* banks) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(banks != nullptr, MML_ERR_INVALID, "null banks");
    const int rc = check_slot_range(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    for (int i = 0; i < count; ++i) banks[i] = ctx->banks.bank.empty() ? -1 : ctx->banks.slot_bank[(size_t)first_slot + i];
    return MML_OK;
}

int mml_map_bank_increment(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && banks && slots && T_wl, MML_ERR_INVALID, "bad arguments");
    // all arguments are checked before the device is touched or a bank changes
    int rc = check_distinct_banks(ctx, n, banks, slots, "mml_map_bank_increment");
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    if (!ctx->uploads.empty()) return mml_refuse(ctx, MML_ERR_STATE, "uploads in flight after a drained context");
    for (int i = 0; i < n; ++i) {
        int m[2] = {0, 0};
        rc = mml_map_upkeep_increment(ctx, mml_map_bank(ctx, banks[i]), slots[i], T_wl + 16 * (size_t)i, m);
        if (n_corner) n_corner[i] = m[0];
        if (n_surf) n_surf[i] = m[1];
        if (rc != MML_OK) return rc;
    }
    return MML_OK;
}

int mml_map_bank_increment_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && banks && slots && T_wl, MML_ERR_INVALID, "bad arguments");
    // all arguments are checked before the device is touched or a bank changes
    int rc = check_distinct_banks(ctx, n, banks, slots, "mml_map_bank_increment_segmented");
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    if (!ctx->uploads.empty()) return mml_refuse(ctx, MML_ERR_STATE, "uploads in flight after a drained context");
    std::vector<MmlMapIncrement> inc;
    for (int i = 0; i < n; ++i) inc.push_back(MmlMapIncrement{mml_map_bank(ctx, banks[i]), slots[i], T_wl + 16 * (size_t)i});
    return mml_map_upkeep_increment_segmented(ctx, n, inc.data(), n_corner, n_surf);
}

int mml_debug_bank_increment_budget(mml_ctx* ctx, long points) {
    if (!ctx) return MML_ERR_INVALID;
    if (points < 1 || points >= (1l << 31)) return mml_refuse(ctx, MML_ERR_INVALID, "the chunk budget must be in [1, 2^31) points");
    ctx->bank_inc.budget = points;
    return MML_OK;
}

// ---- a bank's global cube map: the own-map calls of capi.hip on mml_cube_bank(ctx, bank) ----

int mml_map_bank_set_global(mml_ctx* ctx, int bank, int kind, const float* xyz, const int* cube, int m, const int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    MML_REQUIRE(kind == 0 || kind == 1, MML_ERR_INVALID, "map kind must be 0 (corner) or 1 (surf)");
    MML_REQUIRE(m >= 0 && (m == 0 || (xyz && cube)), MML_ERR_INVALID, "bad global map arguments");
    MML_REQUIRE(m <= ctx->MM, MML_ERR_CAPACITY, "global map larger than max_map_points");
    for (int i = 0; i < m; ++i) MML_REQUIRE(cube[i] >= 0 && cube[i] < 4851, MML_ERR_INVALID, "cube index outside [0, 4851)");
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    return mml_build_global_grid(ctx, mml_cube_bank(ctx, bank), kind, xyz, cube, m, cen);
}

// a call's arguments checked and the context drained, then ONE append chain for all n banks (map_global.hip): every slot's stacks
// are checked before a bank's pending clouds change
static int global_append(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, const char* who) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && banks && slots && T_wl, MML_ERR_INVALID, "bad arguments");
    int rc = check_distinct_banks(ctx, n, banks, slots, who);
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    if (!ctx->uploads.empty()) return mml_refuse(ctx, MML_ERR_STATE, "uploads in flight after a drained context");
    std::vector<MmlCubeRef> cubes;
    for (int i = 0; i < n; ++i) cubes.push_back(mml_cube_bank(ctx, banks[i]));
    return mml_cube_store_append_segmented(ctx, n, cubes.data(), banks, slots, T_wl);
}

int mml_map_bank_global_append(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl) {
    return global_append(ctx, n, banks, slots, T_wl, "mml_map_bank_global_append");
}

int mml_map_bank_global_append_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl) {
    return global_append(ctx, n, banks, slots, T_wl, "mml_map_bank_global_append_segmented");
}

// the loop: one n = 1 chain per bank, in call order; a refusal leaves bank i as it was and banks 0 .. i-1 incremented
int mml_map_bank_global_increment(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && banks && T_wl, MML_ERR_INVALID, "bad arguments");
    int rc = check_distinct_banks(ctx, n, banks, nullptr, "mml_map_bank_global_increment");
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    for (int i = 0; i < n; ++i) {
        int m[2] = {0, 0};
        rc = mml_cube_store_increment(ctx, mml_cube_bank(ctx, banks[i]), banks[i], T_wl + 16 * (size_t)i, m);
        if (n_corner) n_corner[i] = m[0];
        if (n_surf) n_surf[i] = m[1];
        if (rc != MML_OK) return rc;
    }
    return MML_OK;
}

// ONE chain for all n banks
int mml_map_bank_global_increment_segmented(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && banks && T_wl, MML_ERR_INVALID, "bad arguments");
    int rc = check_distinct_banks(ctx, n, banks, nullptr, "mml_map_bank_global_increment_segmented");
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    std::vector<MmlCubeRef> cubes;
    for (int i = 0; i < n; ++i) cubes.push_back(mml_cube_bank(ctx, banks[i]));
    return mml_cube_store_increment_segmented(ctx, n, cubes.data(), banks, T_wl, n_corner, n_surf);
}

int mml_debug_bank_global_increment_budget(mml_ctx* ctx, long points) {
    if (!ctx) return MML_ERR_INVALID;
    if (points < 1 || points >= (1l << 31)) return mml_refuse(ctx, MML_ERR_INVALID, "the chunk budget must be in [1, 2^31) points");
    ctx->bank_cube.budget = points;
    return MML_OK;
}

int mml_map_bank_global_download(mml_ctx* ctx, int bank, int kind, float* xyz, int* cube, int capacity, int* n, int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad arguments");
    MML_HIP(hipSetDevice(ctx->device));
    return mml_cube_store_download(ctx, mml_cube_bank(ctx, bank), kind, xyz, cube, capacity, n, cen);
}

int mml_map_bank_global_reset(mml_ctx* ctx, int bank) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = check_bank(ctx, bank);
    if (rc != MML_OK) return rc;
    rc = enter(ctx);
    if (rc != MML_OK) return rc;
    return mml_cube_store_reset(ctx, mml_cube_bank(ctx, bank));
}

}  // extern "C"
