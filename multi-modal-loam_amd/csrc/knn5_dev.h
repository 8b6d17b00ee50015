// knn5_dev.h -- the exact 5-NN ring search over a radix-sorted uniform grid (MmlGrid), shared by map_assoc.hip (association,
// mml_knn5) and time_offset.hip (the aligner's time-offset search).  Device code only; included inside the including file's
// anonymous namespace, after mml_internal.h.  Compiled with -ffp-contract=off.

// cell of a coordinate along one axis (clamped: rounding may put a point of the bounding box one cell outside)
__device__ __forceinline__ int cell_coord(float v, float o, float inv, int dim) {
    int c = (int)floorf((v - o) * inv);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

// ---------------------------------------------------------------------------------------------------
// exact 5-NN
// The list is five 64-bit keys, (bits of d2) << 32 | index: d2 is a non-negative float, so its bit pattern orders like
// its value and one unsigned compare is the reference's order "(d, index) ascending" (ties by lower index).  A NaN d2
// has a pattern above +inf and never enters, as with the float compare.
struct Knn5 {
    unsigned long long key[5];
};
constexpr unsigned long long KNN_EMPTY = (0x7f800000ull << 32) | 0x7fffffffull;  // (INFINITY, INT_MAX)
__device__ __forceinline__ unsigned long long knn_key(float d, int id) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)id;
}
__device__ __forceinline__ float knn_d(const Knn5& k, int j) { return __uint_as_float((unsigned)(k.key[j] >> 32)); }
__device__ __forceinline__ int knn_id(const Knn5& k, int j) { return (int)(unsigned)k.key[j]; }
__device__ __forceinline__ void knn_init(Knn5& k) {
#pragma unroll
    for (int i = 0; i < 5; ++i) k.key[i] = KNN_EMPTY;
}
// Sorted insert by rank: lt_s = (x < key[s]) is monotone in s for a sorted list, so the new list is
//   key[s] = lt_s ? (lt_{s-1} ? key[s-1] : x) : key[s]
// -- five compares and two selects per word, 23 vector instructions and no dependent chain.  A wavefront runs the insert as
// soon as ONE of its lanes has a candidate below its fifth key, which is the case for nearly every candidate of the first rings
// (a lane takes ~5 (1 + ln(n / 5)) of n candidates), so the insert is most of what a candidate costs; the sinking form
// (compare, two selects, compare, two selects per stage) compiled to 38.
__device__ __forceinline__ unsigned long long sel64(bool c, unsigned long long a, unsigned long long b) {
    // (two v_cndmask; written on the halves and marked unpredictable so that no pass turns a select of a select into branches)
    const unsigned lo = __builtin_unpredictable(c) ? (unsigned)a : (unsigned)b;
    const unsigned hi = __builtin_unpredictable(c) ? (unsigned)(a >> 32) : (unsigned)(b >> 32);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void knn_insert_key(Knn5& k, unsigned long long x) {
    const bool lt0 = x < k.key[0], lt1 = x < k.key[1], lt2 = x < k.key[2], lt3 = x < k.key[3], lt4 = x < k.key[4];
    const unsigned long long c1 = sel64(lt0, k.key[0], x), c2 = sel64(lt1, k.key[1], x), c3 = sel64(lt2, k.key[2], x),
                             c4 = sel64(lt3, k.key[3], x);
    k.key[4] = sel64(lt4, c4, k.key[4]);
    k.key[3] = sel64(lt3, c3, k.key[3]);
    k.key[2] = sel64(lt2, c2, k.key[2]);
    k.key[1] = sel64(lt1, c1, k.key[1]);
    k.key[0] = sel64(lt0, x, k.key[0]);
}
__device__ __forceinline__ void knn_insert(Knn5& k, float dd, int ii) {
    const unsigned long long x = knn_key(dd, ii);
    if (!(x < k.key[4])) return;
    knn_insert_key(k, x);
}

// tags / mytag: when the grid carries cube tags (global map, a12) only points of the query's cube take part: the
// reference searches the kd-tree of ONE cube (Estimator.cpp:199,630).  Every point inside the visited radius is still
// looked at, so the exactness bound of the ring search is unchanged.
__device__ __forceinline__ void scan_range(const float4* __restrict__ pts, const uint16_t* __restrict__ tags, int mytag,
                                           int s, int e, float qx, float qy, float qz, Knn5& k) {
    // four candidates per round, their loads issued together (one load per round leaves its whole latency exposed)
    for (int i0 = s; i0 < e; i0 += 4) {
        float4 p[4];
        int tg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = (unsigned)min(i0 + u, e - 1);  // (unsigned: a 32-bit offset from the scalar base, no 64-bit address arithmetic)
            p[u] = pts[i];
            tg[u] = tags ? (int)tags[i] : mytag;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
            float r = 0;
            r += dx * dx;
            r += dy * dy;
            r += dz * dz;
            // a candidate that does not take part carries a key that never enters
            const unsigned long long x = (i0 + u >= e || tg[u] != mytag) ? ~0ull : knn_key(r, (int)__float_as_uint(p[u].w));
            if (x < k.key[4]) knn_insert_key(k, x);
        }
    }
}

// Ring-expanding search.  After ring r every map point with Chebyshev cell distance <= r from the query's home
// cell has been visited, which includes every point within Euclidean distance
// rho_r = (r + inset) * cell - margin  (inset = distance from the query to the nearest face of its home cell).
// A query is finished when its 5th best squared distance is below rho_r^2 (exact 5-NN), or when rho_r^2 >= max_d2
// (the caller rejects anything with d5 >= max_d2, Estimator.cpp:285,705).
//
// Two-level schedule: every lane walks rings 0 and 1 of its own query (27 cells, the common case for a
// voxel-filtered map); queries that are still open are then finished one at a time by the WHOLE wavefront, the 64
// lanes splitting the rows of each further shell and merging their private top-5 lists with shuffles.  That bounds
// the cost of the rare far query (hundreds of mostly empty cells) by ~1/64 of a private walk.
struct KnnQuery {
    float qx, qy, qz, inset;
    float fx, fy, fz;  // the query in cell units
    int hx, hy, hz;
};

__device__ __forceinline__ KnnQuery knn_query(const MmlGrid& g, float qx, float qy, float qz) {
    KnnQuery q;
    q.qx = qx;
    q.qy = qy;
    q.qz = qz;
    const float fx = (qx - g.origin[0]) * g.inv_cell, fy = (qy - g.origin[1]) * g.inv_cell,
                fz = (qz - g.origin[2]) * g.inv_cell;
    q.fx = fx;
    q.fy = fy;
    q.fz = fz;
    q.hx = (int)floorf(fx);
    q.hy = (int)floorf(fy);
    q.hz = (int)floorf(fz);
    float inset = fminf(fminf(fminf(fx - q.hx, q.hx + 1 - fx), fminf(fy - q.hy, q.hy + 1 - fy)),
                        fminf(fz - q.hz, q.hz + 1 - fz));
    q.inset = (inset > 0.f) ? inset : 0.f;
    return q;
}

// true when the search may stop after shell r
__device__ __forceinline__ bool knn_done(const MmlGrid& g, float inset, int r, float d5, float max_d2) {
    float rho = ((float)r + inset) * g.cell;
    rho = rho - 1e-3f * g.cell;  // margin dominating the float rounding of d2 and of the cell mapping
    if (!(rho > 0.f)) return false;
    const float rho2 = rho * rho;
    return d5 < rho2 || rho2 >= max_d2;
}

// one row (fixed y,z) of shell r: the whole x-span on a face, the two end cells otherwise.
// `bound` is any upper bound of the query's final 5th squared distance (INFINITY when none is known).  Cells that
// cannot hold a point closer than that are skipped: a point stored in cell (cx, y, z) lies, per axis, within 2e-3 cells
// of the cell's slab (float rounding of the cell mapping at build and query time, the same allowance knn_done makes),
// so its distance to the query is at least cell * (|gap vector| - 4e-3); a skipped point has d2 > bound * (1 + 1e-5) in
// exact arithmetic and therefore a float d2 > bound: it could not have entered the list.
__device__ __forceinline__ void scan_shell_row(const MmlGrid& g, const KnnQuery& q, int r, int y, int z, Knn5& k,
                                               int mytag = -1, float bound = INFINITY) {
    const int DX = g.dim[0], DY = g.dim[1], DZ = g.dim[2];
    if (y < 0 || y >= DY || z < 0 || z >= DZ) return;
    int xlo = -1, xhi = DX;  // no bound yet (a far query still looking for its first five points): nothing to work out
    if (bound < INFINITY) {
        const float gy = y > q.hy ? (float)y - q.fy : (y < q.hy ? q.fy - (float)(y + 1) : 0.f);
        const float gz = z > q.hz ? (float)z - q.fz : (z < q.hz ? q.fz - (float)(z + 1) : 0.f);
        const float reach = sqrtf(bound * 1.00001f) * g.inv_cell + 4e-3f;  // cells
        const float w2 = reach * reach - (gy * gy + gz * gz);
        if (w2 < 0.f) return;
        const float w = sqrtf(w2);
        // cells of this row whose slab comes within w cells of the query along x
        xlo = (int)floorf(fmaxf(q.fx - w, -1.f));
        xhi = (int)floorf(fminf(q.fx + w, (float)DX));
    }
    const int x0 = q.hx - r, x1 = q.hx + r;
    const bool face = (z == q.hz - r || z == q.hz + r || y == q.hy - r || y == q.hy + r);
    const int rowbase = DX * (y + DY * z);
    if (face) {
        const int xa = max(max(x0, 0), xlo), xb = min(min(x1, DX - 1), xhi);
        if (xa <= xb)
            scan_range(g.pts, g.tags, mytag, g.cell_start[rowbase + xa], g.cell_start[rowbase + xb + 1], q.qx, q.qy, q.qz, k);
    } else {
        if (x0 >= 0 && x0 < DX && x0 >= xlo)
            scan_range(g.pts, g.tags, mytag, g.cell_start[rowbase + x0], g.cell_start[rowbase + x0 + 1], q.qx, q.qy, q.qz, k);
        if (x1 >= 0 && x1 < DX && x1 != x0 && x1 <= xhi)
            scan_range(g.pts, g.tags, mytag, g.cell_start[rowbase + x1], g.cell_start[rowbase + x1 + 1], q.qx, q.qy, q.qz, k);
    }
}

// Four rows of shell r at once: rows t, t + STRIDE, t + 2 STRIDE, t + 3 STRIDE of the shell's in-grid rectangle
// (row t is y = ylo + t % wy, z = zlo + t / wy; rows at or beyond nrows do not exist).  scan_shell_row is a dependent chain per
// row -- extent, two cell_start loads, points -- and a far query's rows are mostly empty, so a lane that walks them one by
// one waits a full load latency for every "nothing here".  Here the extents of all four rows are worked out first, every
// cell_start load of the group is issued together (a face row is one span of cells, two loads; any other row is its two end
// cells, four loads; a piece that does not exist or lies outside `bound` reads cell_start[0] twice and comes out empty), and only
// the pieces that hold points go on to scan_range: an empty row costs no further memory access.
// `bound` as in scan_shell_row, finite or not, fixed for the group: it may be stale by the group's own finds, and a looser
// bound only reads more.  The cells visited are those scan_shell_row visits for the same bound, and the top-5 list is a set
// ordered by (d2, index) keys, so the order of the visits does not matter.
template <int STRIDE>
__device__ __forceinline__ void scan_shell_rows4(const MmlGrid& g, const KnnQuery& q, int r, int ylo, int wy, int zlo, int nrows,
                                                 int t, Knn5& k, int mytag, float bound) {
    const int DX = g.dim[0], DY = g.dim[1];
    const float reach = sqrtf(bound * 1.00001f) * g.inv_cell + 4e-3f;  // cells
    const float reach2 = reach * reach;
    const int x0 = q.hx - r, x1 = q.hx + r;
    unsigned ia[8], ib[8];  // piece v = cells [ia, ib) of cell_start's index space; constant indices only: registers
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int tu = t + u * STRIDE;
        const int y = ylo + tu % wy, z = zlo + tu / wy;
        const float gy = y > q.hy ? (float)y - q.fy : (y < q.hy ? q.fy - (float)(y + 1) : 0.f);
        const float gz = z > q.hz ? (float)z - q.fz : (z < q.hz ? q.fz - (float)(z + 1) : 0.f);
        const float w2 = reach2 - (gy * gy + gz * gz);
        const bool in = tu < nrows && !(w2 < 0.f);
        const float w = sqrtf(fmaxf(w2, 0.f));
        const int xlo = (int)floorf(fmaxf(q.fx - w, -1.f)), xhi = (int)floorf(fminf(q.fx + w, (float)DX));
        const bool face = (z == q.hz - r || z == q.hz + r || y == q.hy - r || y == q.hy + r);
        const int rowbase = DX * (y + DY * z);
        const int xa = max(max(x0, 0), xlo), xb = min(min(x1, DX - 1), xhi);
        const bool va = in && (face ? xa <= xb : (x0 >= 0 && x0 < DX && x0 >= xlo));
        const bool vb = in && !face && x1 >= 0 && x1 < DX && x1 != x0 && x1 <= xhi;
        ia[2 * u] = va ? (unsigned)(rowbase + (face ? xa : x0)) : 0u;
        ib[2 * u] = va ? (unsigned)(rowbase + (face ? xb : x0) + 1) : 0u;
        ia[2 * u + 1] = vb ? (unsigned)(rowbase + x1) : 0u;
        ib[2 * u + 1] = vb ? (unsigned)(rowbase + x1 + 1) : 0u;
    }
    int s[8], e[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        s[v] = g.cell_start[ia[v]];
        e[v] = g.cell_start[ib[v]];
    }
    unsigned todo = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) todo |= (s[v] < e[v] ? 1u : 0u) << v;
    // every lane takes its own next non-empty piece, so the lanes of a wavefront scan side by side whichever rows theirs are
#pragma unroll 1
    while (todo) {
        const int v = __ffs((int)todo) - 1;
        todo &= todo - 1;
        int ss = s[0], ee = e[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            ss = v == j ? s[j] : ss;
            ee = v == j ? e[j] : ee;
        }
        scan_range(g.pts, g.tags, mytag, ss, ee, q.qx, q.qy, q.qz, k);
    }
}

// ring 1 rows, nearest first, so that the bound has tightened before the edge and corner rows are reached
__device__ __constant__ const signed char kRing1Row[9][2] = {{0, 0}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}};

// rings 0 and 1 of one query, private to the lane; true when the search may stop there
__device__ __forceinline__ bool scan_rings01(const MmlGrid& g, const KnnQuery& q, int rmax, float max_d2, Knn5& k, int mytag) {
    scan_shell_row(g, q, 0, q.hy, q.hz, k, mytag);
    if (knn_done(g, q.inset, 0, knn_d(k, 4), max_d2)) return true;
    if (rmax < 1) return false;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) scan_shell_row(g, q, 1, q.hy + kRing1Row[t][0], q.hz + kRing1Row[t][1], k, mytag, knn_d(k, 4));
    return knn_done(g, q.inset, 1, knn_d(k, 4), max_d2);
}

__device__ __forceinline__ unsigned long long knn_head(const Knn5& k, int head) {
    unsigned long long key = KNN_EMPTY;
#pragma unroll
    for (int s = 0; s < 5; ++s)
        if (head == s) key = k.key[s];
    return key;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}
// merge of the private sorted lists (disjoint point sets) of the lanes whose ids differ in the bits below `span` into
// their common top-5, same in all of them
template <int SPAN>
__device__ __forceinline__ void lanes_merge5(const Knn5& local, Knn5& out) {
    int head = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const unsigned long long mine = knn_head(local, head);
        unsigned long long m = mine;
#pragma unroll
        for (int o = SPAN / 2; o > 0; o >>= 1) {
            const unsigned long long other = shfl_xor_u64(m, o);
            m = other < m ? other : m;
        }
        out.key[r] = m;
        if (mine == m && (unsigned)(m >> 32) < 0x7f800000u) head++;
    }
}

// Must be called by ALL 64 lanes of the wavefront (inactive queries pass valid = false and only help).
__device__ void knn5_search(const MmlGrid& g, bool valid, float qx, float qy, float qz, float max_d2, Knn5& k) {
    knn_init(k);
    const KnnQuery q = knn_query(g, qx, qy, qz);
    // no shell beyond the grid's far side holds a cell (keeps an unbounded search, max_d2 = inf, finite)
    const int rgrid = max(max(max(q.hx, g.dim[0] - 1 - q.hx), max(q.hy, g.dim[1] - 1 - q.hy)), max(q.hz, g.dim[2] - 1 - q.hz));
    const float rf = ceilf(sqrtf(max_d2) * g.inv_cell) + 1.f;
    const int rmax = rf < (float)rgrid ? (int)rf : max(rgrid, 0);
    bool pending = false;
    if (valid) {
        pending = !scan_rings01(g, q, rmax, max_d2, k, -1);
        if (rmax < 2) pending = false;
    }
    unsigned long long todo = __ballot(pending);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        KnnQuery s;
        s.qx = __shfl(q.qx, src);
        s.qy = __shfl(q.qy, src);
        s.qz = __shfl(q.qz, src);
        s.inset = __shfl(q.inset, src);
        s.fx = __shfl(q.fx, src);
        s.fy = __shfl(q.fy, src);
        s.fz = __shfl(q.fz, src);
        s.hx = __shfl(q.hx, src);
        s.hy = __shfl(q.hy, src);
        s.hz = __shfl(q.hz, src);
        Knn5 loc;
        if (lane == src)
            loc = k;
        else
            knn_init(loc);
        Knn5 best;
        knn_init(best);
        const int rmax_s = __shfl(rmax, src);  // (the bound of the query being served, not of the serving lane's own)
        // a query outside the grid: the shells before the grid's near side hold no cell
        const int rnear = max(max(max(-s.hx, s.hx - (g.dim[0] - 1)), max(-s.hy, s.hy - (g.dim[1] - 1))),
                              max(-s.hz, s.hz - (g.dim[2] - 1)));
        for (int r = max(2, rnear); r <= rmax_s; ++r) {
            const float bnd = fminf(knn_d(best, 4), __shfl(knn_d(k, 4), src));  // both bound the final 5th distance from above
            // the rows of the shell that lie inside the grid
            const int ylo = max(s.hy - r, 0), yhi = min(s.hy + r, g.dim[1] - 1), zlo = max(s.hz - r, 0), zhi = min(s.hz + r, g.dim[2] - 1);
            const int wy = yhi - ylo + 1, wz = zhi - zlo + 1;
            if (wy > 0 && wz > 0)
                for (int t = lane; t < wy * wz; t += 64)
                    scan_shell_row(g, s, r, ylo + (t % wy), zlo + (t / wy), loc, -1, fminf(bnd, knn_d(loc, 4)));
            lanes_merge5<64>(loc, best);
            if (knn_done(g, s.inset, r, knn_d(best, 4), max_d2)) break;
        }
        if (lane == src) k = best;
    }
}
