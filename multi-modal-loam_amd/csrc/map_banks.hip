// map_banks.hip -- the map entry points, and the map banks: N further Estimators' maps per context, and which scan slot is matched
//   against which.
//   The context's own maps and every bank's are one struct (MmlMapState, mml_internal.h; mml_map_at).  Each map call exists twice
//   in the C API -- mml_map_* for the own maps, mml_map_bank_* for a bank's -- and once here: the public function checks what only
//   it can check (a slot range; check_bank / check_distinct_banks) and calls the shared body with the state.
//   The association kernels of a launch with a bound slot read the maps' grid descriptors from two device-resident tables,
//   (banks + 1) rows x 2 kinds each -- the local maps and the global cube maps --, through the per-slot bank array (map_assoc.hip,
//   the BANKED forms); mml_assoc_ready keeps the three device arrays equal to the host's state.
//   The cube stores' upkeep is one chain of launches for n stores (map_global.hip), which the *_segmented forms and the appends run
//   once for all n banks and the loop increment once per bank.  The context's OWN cube map and a bound slot exclude each other.
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

// the slot of an own-map call
int check_own_slot(mml_ctx* ctx, int slot) {
    MML_REQUIRE(slot >= 0 && slot < ctx->B, MML_ERR_INVALID, "slot range out of bounds");
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

const int kOwn = -1;  // the own maps in a list of banks

std::vector<MmlMapState*> maps_at(mml_ctx* ctx, int n, const int* banks) {
    std::vector<MmlMapState*> maps;
    for (int i = 0; i < n; ++i) maps.push_back(&mml_map_at(ctx, banks[i]));
    return maps;
}

// ---- the shared bodies: the caller has checked ctx and whatever names the map ----

int set_local(mml_ctx* ctx, MmlMapState& map, int kind, const float* xyz, int m) {
    MML_REQUIRE(m >= 0 && (m == 0 || xyz), MML_ERR_INVALID, "bad map arguments");
    MML_HIP(hipSetDevice(ctx->device));
    return mml_build_grid(ctx, map, kind, xyz, m);
}

int local_reset(mml_ctx* ctx, MmlMapState& map) {
    const int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    memset(map.ring_n, 0, sizeof(map.ring_n));
    map.local_map_id = 0;
    return MML_OK;
}

int local_download(mml_ctx* ctx, const MmlMapState& map, int kind, float* xyz, int capacity, int* n) {
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad arguments");
    MML_REQUIRE(map.have_map[kind], MML_ERR_STATE, map.name < 0 ? "no local map" : "the bank's last map build failed");
    MML_HIP(hipSetDevice(ctx->device));
    const int m = map.grid[kind].m;
    *n = m;
    if (!xyz || m == 0) return MML_OK;
    MML_REQUIRE(capacity >= m, MML_ERR_CAPACITY, "capacity below the map size");
    std::vector<float4> tmp((size_t)m);
    MML_HIP(hipMemcpyAsync(tmp.data(), map.map_tmp + (size_t)kind * ctx->MM, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    for (int i = 0; i < m; ++i) {
        xyz[3 * i] = tmp[i].x;
        xyz[3 * i + 1] = tmp[i].y;
        xyz[3 * i + 2] = tmp[i].z;
    }
    return MML_OK;
}

// Estimator::MapIncrementLocal for the n maps `banks`: the context drained, then ONE chain for all of them (one_chain: all or
// nothing) or one n = 1 chain per map in call order (a refusal leaves map i as it was, its two sizes 0, and maps 0 .. i-1 incremented)
int local_increment(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf, bool one_chain) {
    int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    std::vector<MmlMapIncrement> inc;
    for (int i = 0; i < n; ++i) inc.push_back(MmlMapIncrement{&mml_map_at(ctx, banks[i]), slots[i], T_wl + 16 * (size_t)i});
    if (one_chain) return mml_map_upkeep_increment_segmented(ctx, n, inc.data(), n_corner, n_surf);
    for (int i = 0; i < n && rc == MML_OK; ++i) {
        if (n_corner) n_corner[i] = 0;
        if (n_surf) n_surf[i] = 0;
        rc = mml_map_upkeep_increment_segmented(ctx, 1, &inc[(size_t)i], n_corner ? n_corner + i : nullptr, n_surf ? n_surf + i : nullptr);
    }
    return rc;
}

// Validates everything and drains the context before the map changes: a refused call leaves the match copy as it was.
int set_global(mml_ctx* ctx, MmlMapState& map, int kind, const float* xyz, const int* cube, int m, const int* cen) {
    MML_REQUIRE(kind == 0 || kind == 1, MML_ERR_INVALID, "map kind must be 0 (corner) or 1 (surf)");
    MML_REQUIRE(m >= 0 && (m == 0 || (xyz && cube)), MML_ERR_INVALID, "bad global map arguments");
    MML_REQUIRE(m <= ctx->MM, MML_ERR_CAPACITY, "global map larger than max_map_points");
    for (int i = 0; i < m; ++i) MML_REQUIRE(cube[i] >= 0 && cube[i] < 4851, MML_ERR_INVALID, "cube index outside [0, 4851)");
    const int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    return mml_build_global_grid(ctx, map, kind, xyz, cube, m, cen);
}

// the context drained, then ONE append chain for all n stores (map_global.hip): every slot's stacks are checked before a store's
// pending clouds change
int global_append(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl) {
    const int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    return mml_cube_store_append_segmented(ctx, n, maps_at(ctx, n, banks).data(), slots, T_wl);
}

// the context drained, then ONE increment chain for all n stores or one n = 1 chain per store, as local_increment
int global_increment(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf, bool one_chain) {
    int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    const std::vector<MmlMapState*> maps = maps_at(ctx, n, banks);
    if (one_chain) return mml_cube_store_increment_segmented(ctx, n, maps.data(), T_wl, n_corner, n_surf);
    for (int i = 0; i < n && rc == MML_OK; ++i) {
        if (n_corner) n_corner[i] = 0;
        if (n_surf) n_surf[i] = 0;
        rc = mml_cube_store_increment_segmented(ctx, 1, &maps[(size_t)i], T_wl + 16 * (size_t)i, n_corner ? n_corner + i : nullptr,
                                                n_surf ? n_surf + i : nullptr);
    }
    return rc;
}

int global_download(mml_ctx* ctx, const MmlMapState& map, int kind, float* xyz, int* cube, int capacity, int* n, int* cen) {
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad arguments");
    MML_HIP(hipSetDevice(ctx->device));
    return mml_cube_store_download(ctx, map, kind, xyz, cube, capacity, n, cen);
}

int global_reset(mml_ctx* ctx, MmlMapState& map) {
    const int rc = enter(ctx);
    if (rc != MML_OK) return rc;
    return mml_cube_store_reset(ctx, map);
}

// the checks of the bank calls that work n banks through
int check_bank_call(mml_ctx* ctx, int n, const int* banks, const int* slots, bool need_slots, const double* T_wl, const char* who) {
    MML_REQUIRE(n >= 1 && banks && (slots || !need_slots) && T_wl, MML_ERR_INVALID, "bad arguments");
    return check_distinct_banks(ctx, n, banks, slots, who);
}

}  // namespace

int mml_map_local_alloc(mml_ctx* ctx, MmlMapState& map) {
    const size_t MM = (size_t)ctx->MM;
    return map.grid_mem.reserve(ctx, {mml_part(map.grid[0].pts, MM), mml_part(map.grid[0].cell_start, 4 * MM + 4096 + 2), mml_part(map.grid[1].pts, MM),
                                      mml_part(map.grid[1].cell_start, 4 * MM + 4096 + 2), mml_part(map.map_tmp, 2 * MM)});
}

int mml_assoc_ready(mml_ctx* ctx, int first, int count, const char* who) {
    MmlBanks& K = ctx->banks;
    const MmlMapState& own = ctx->own;
    bool bound = false;
    for (int i = 0; i < count; ++i) {
        const int bank = K.n_bound ? K.slot_bank[(size_t)first + i] : -1;
        if (bank < 0) {
            if (!(own.have_map[0] && own.have_map[1])) return mml_refuse(ctx, MML_ERR_STATE, "%s before both maps were set", who);
            continue;
        }
        if (own.cmatch.have_gmap[0] || own.cmatch.have_gmap[1])
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
    for (size_t e = 0; e <= K.bank.size(); ++e) {
        const MmlMapState& M = mml_map_at(ctx, (int)e - 1);
        for (int k = 0; k < 2; ++k) {
            const MmlCubeMatch& G = M.cmatch;
            MmlCubeDesc& c = tc[2 * e + k];
            memset(static_cast<void*>(&c), 0, sizeof(c));
            c.g = G.ggrid[k];
            c.orig = G.gmap_orig[k];
            c.cube_cnt = G.cube_cnt[k];
            c.have_g = (e > 0 && G.have_gmap[k]) ? 1 : 0;  // (entry 0: never, the exclusion rule above)
            for (int a = 0; a < 3; ++a) c.cen[a] = G.cen[a];
            MmlMapDesc& d = t[2 * e + k];
            memset(static_cast<void*>(&d), 0, sizeof(d));  // (the padding too: the rows are compared and copied as bytes)
            d.g = M.grid[k];
            d.orig = M.map_tmp + (size_t)k * ctx->MM;
            if (e == 0 && !M.have_map[k]) d.g.m = 0;  // (an unset own map: only bound slots are in the launch)
        }
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
    rc = K.tab_mem.reserve(ctx, {mml_part(K.d_table, 2 * ((size_t)n_banks + 1)), mml_part(K.d_cube_table, 2 * ((size_t)n_banks + 1)),
                                 mml_part(K.d_slot_bank, (size_t)ctx->B)});
    for (int b = 0; b < n_banks && rc == MML_OK; ++b) {
        MmlMapState& m = K.bank[(size_t)b];
        m.name = b;
        m.have_map[0] = m.have_map[1] = true;  // a bank that was never set is an empty map
        rc = mml_map_local_alloc(ctx, m);
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
    if (any && (ctx->own.cmatch.have_gmap[0] || ctx->own.cmatch.have_gmap[1]))
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

int mml_debug_bank_increment_budget(mml_ctx* ctx, long points) {
    if (!ctx) return MML_ERR_INVALID;
    if (points < 1 || points >= (1l << 31)) return mml_refuse(ctx, MML_ERR_INVALID, "the chunk budget must be in [1, 2^31) points");
    ctx->bank_inc.budget = points;
    return MML_OK;
}

int mml_debug_bank_global_increment_budget(mml_ctx* ctx, long points) {
    if (!ctx) return MML_ERR_INVALID;
    if (points < 1 || points >= (1l << 31)) return mml_refuse(ctx, MML_ERR_INVALID, "the chunk budget must be in [1, 2^31) points");
    ctx->bank_cube.budget = points;
    return MML_OK;
}

// ---- the map calls: the own maps', then the banks' ----

int mml_map_set_local(mml_ctx* ctx, int kind, const float* xyz, int m) {
    if (!ctx) return MML_ERR_INVALID;
    return set_local(ctx, ctx->own, kind, xyz, m);
}

int mml_map_local_reset(mml_ctx* ctx) {
    if (!ctx) return MML_ERR_INVALID;
    return local_reset(ctx, ctx->own);
}

int mml_map_local_download(mml_ctx* ctx, int kind, float* xyz, int capacity, int* n) {
    if (!ctx) return MML_ERR_INVALID;
    return local_download(ctx, ctx->own, kind, xyz, capacity, n);
}

int mml_map_increment_local(mml_ctx* ctx, int slot, const double* T_wl, int* n_corner_map, int* n_surf_map) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_own_slot(ctx, slot);
    if (rc != MML_OK) return rc;
    MML_REQUIRE(T_wl, MML_ERR_INVALID, "null transform");
    return local_increment(ctx, 1, &kOwn, &slot, T_wl, n_corner_map, n_surf_map, false);
}

int mml_map_set_global(mml_ctx* ctx, int kind, const float* xyz, const int* cube, int m, const int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    return set_global(ctx, ctx->own, kind, xyz, cube, m, cen);
}

int mml_map_global_append(mml_ctx* ctx, int slot, const double* T_wl) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_own_slot(ctx, slot);
    if (rc != MML_OK) return rc;
    MML_REQUIRE(T_wl, MML_ERR_INVALID, "null transform");
    return global_append(ctx, 1, &kOwn, &slot, T_wl);
}

int mml_map_global_increment(mml_ctx* ctx, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(T_wl, MML_ERR_INVALID, "null transform");
    return global_increment(ctx, 1, &kOwn, T_wl, n_corner, n_surf, false);
}

int mml_map_global_download(mml_ctx* ctx, int kind, float* xyz, int* cube, int capacity, int* n, int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    return global_download(ctx, ctx->own, kind, xyz, cube, capacity, n, cen);
}

int mml_map_global_reset(mml_ctx* ctx) {
    if (!ctx) return MML_ERR_INVALID;
    return global_reset(ctx, ctx->own);
}

int mml_map_bank_set_local(mml_ctx* ctx, int bank, int kind, const float* xyz, int m) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : set_local(ctx, mml_map_at(ctx, bank), kind, xyz, m);
}

int mml_map_bank_reset(mml_ctx* ctx, int bank) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : local_reset(ctx, mml_map_at(ctx, bank));
}

int mml_map_bank_download(mml_ctx* ctx, int bank, int kind, float* xyz, int capacity, int* n) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : local_download(ctx, mml_map_at(ctx, bank), kind, xyz, capacity, n);
}

// all arguments are checked before the device is touched or a bank changes
int mml_map_bank_increment(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, slots, true, T_wl, "mml_map_bank_increment");
    return rc != MML_OK ? rc : local_increment(ctx, n, banks, slots, T_wl, n_corner, n_surf, false);
}

int mml_map_bank_increment_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, slots, true, T_wl, "mml_map_bank_increment_segmented");
    return rc != MML_OK ? rc : local_increment(ctx, n, banks, slots, T_wl, n_corner, n_surf, true);
}

int mml_map_bank_set_global(mml_ctx* ctx, int bank, int kind, const float* xyz, const int* cube, int m, const int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : set_global(ctx, mml_map_at(ctx, bank), kind, xyz, cube, m, cen);
}

int mml_map_bank_global_append(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, slots, true, T_wl, "mml_map_bank_global_append");
    return rc != MML_OK ? rc : global_append(ctx, n, banks, slots, T_wl);
}

int mml_map_bank_global_append_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, slots, true, T_wl, "mml_map_bank_global_append_segmented");
    return rc != MML_OK ? rc : global_append(ctx, n, banks, slots, T_wl);
}

int mml_map_bank_global_increment(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, nullptr, false, T_wl, "mml_map_bank_global_increment");
    return rc != MML_OK ? rc : global_increment(ctx, n, banks, T_wl, n_corner, n_surf, false);
}

int mml_map_bank_global_increment_segmented(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank_call(ctx, n, banks, nullptr, false, T_wl, "mml_map_bank_global_increment_segmented");
    return rc != MML_OK ? rc : global_increment(ctx, n, banks, T_wl, n_corner, n_surf, true);
}

int mml_map_bank_global_download(mml_ctx* ctx, int bank, int kind, float* xyz, int* cube, int capacity, int* n, int* cen) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : global_download(ctx, mml_map_at(ctx, bank), kind, xyz, cube, capacity, n, cen);
}

int mml_map_bank_global_reset(mml_ctx* ctx, int bank) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = check_bank(ctx, bank);
    return rc != MML_OK ? rc : global_reset(ctx, mml_map_at(ctx, bank));
}

}  // extern "C"
