// mml_mem.h -- the one place of libmmloam_hip.so that allocates and frees device and pinned memory.  Four owners, one per
// lifetime: MmlFixed (allocated by a create call, freed by its destroy), MmlStaging (grow-only), MmlGroup (several buffers that
// exist together or not at all) and MmlTemp (one call).  Beside them the two things every batched side call builds on them:
// MmlCarve, which lays typed arrays out in one block and is the only code that casts block memory, and MmlSides, which holds the
// side calls' scratch structs for the context and deletes them in one loop.  Host code only: a program without kernels can include it.
// `Ctx` in the calls below is whatever carries the error text in a std::string `err` (mml_ctx in the library).
#ifndef MML_MEM_H
#define MML_MEM_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "mmloam_hip.h"

template <class Ctx>
int mml_mem_fail(Ctx* ctx, const char* what, hipError_t e) {
    (void)hipGetLastError();  // (reported here: a later launch check must not find it)
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return MML_ERR_HIP;
}

// Buffers of a fixed size: alloc() hands out the pointer and records it, release() frees whatever was recorded.  The owner keeps
// the typed pointers under their own names; after a failed alloc() the pointer is null and nothing is recorded for it.
struct MmlFixed {
    std::vector<void*> dev, pinned;
    template <class T>
    hipError_t alloc(T** p, size_t n) {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (n ? n : 1));
        if (e == hipSuccess) dev.push_back(*p);
        else *p = nullptr;
        return e;
    }
    template <class T>
    hipError_t alloc_pinned(T** p, size_t n) {
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(p), sizeof(T) * (n ? n : 1), hipHostMallocDefault);
        if (e == hipSuccess) pinned.push_back(*p);
        else *p = nullptr;
        return e;
    }
    void release() {
        for (void* p : dev)
            if (p) (void)hipFree(p);
        for (void* p : pinned)
            if (p) (void)hipHostFree(p);
        dev.clear();
        pinned.clear();
    }
};

// A device array and (Pinned) its pinned host twin, sized for the largest request so far: it only grows, to exactly the size
// asked for.  reserve(ctx, n) is for buffers whose users drain their stream before they return, so that nothing is in flight when
// the buffers are replaced; reserve(ctx, n, stream) synchronises `stream` first and is for the others.  A failure midway leaves
// cap == 0 and each pointer valid or null, which the next reserve() or release() cleans up.
template <class T, bool Pinned = true>
struct MmlStaging {
    T* d = nullptr;
    T* h = nullptr;  // stays null without Pinned
    size_t cap = 0;  // elements
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
    }
    template <class Ctx>
    int reserve(Ctx* ctx, size_t n) {
        if (n <= cap) return MML_OK;
        release();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(T) * n);
        if (e != hipSuccess) return d = nullptr, mml_mem_fail(ctx, "hipMalloc", e);
        if (Pinned && (e = hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(T) * n, hipHostMallocDefault)) != hipSuccess)
            return h = nullptr, mml_mem_fail(ctx, "hipHostMalloc", e);
        cap = n;
        return MML_OK;
    }
    template <class Ctx>
    int reserve(Ctx* ctx, size_t n, hipStream_t live) {
        if (n <= cap) return MML_OK;
        const hipError_t e = hipStreamSynchronize(live);
        if (e != hipSuccess) return mml_mem_fail(ctx, "hipStreamSynchronize", e);
        return reserve(ctx, n);
    }
};

// Several device buffers that exist together or not at all, each read by its owner through a typed view pointer: reserve()
// replaces what the group held and fills every view or, when one allocation fails, frees the ones it made and leaves every view
// null and the group absent, so the next call tries again.
struct MmlPart {
    void** view;
    size_t bytes;
};
template <class T>
MmlPart mml_part(T*& view, size_t n) {
    return MmlPart{reinterpret_cast<void**>(&view), sizeof(T) * n};
}
struct MmlGroup : MmlFixed {
    bool present() const { return !dev.empty(); }
    template <class Ctx>
    int reserve(Ctx* ctx, std::initializer_list<MmlPart> parts) {
        release();
        hipError_t e = hipSuccess;
        for (const MmlPart& p : parts)
            if (e == hipSuccess && (e = hipMalloc(p.view, p.bytes)) == hipSuccess) dev.push_back(*p.view);
        if (e == hipSuccess) return MML_OK;
        release();
        for (const MmlPart& p : parts) *p.view = nullptr;
        return mml_mem_fail(ctx, "hipMalloc", e);
    }
};

// A device array that lives for one call: freed on every return path.
template <class T>
struct MmlTemp {
    T* d = nullptr;
    MmlTemp() = default;
    MmlTemp(const MmlTemp&) = delete;
    MmlTemp& operator=(const MmlTemp&) = delete;
    ~MmlTemp() {
        if (d) (void)hipFree(d);
    }
    hipError_t alloc(size_t n) {
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(T) * n);
        if (e != hipSuccess) d = nullptr;
        return e;
    }
};

// One block carved into typed arrays.  A field knows where it lies and how many elements it has, so that an array's type and
// count are written once: in(base) is the array inside the pinned twin or the device block alike, bytes() its size for a copy.
template <class T>
struct MmlField {
    size_t off = 0, n = 0;  // bytes from the block's start | elements
    size_t bytes() const { return sizeof(T) * n; }
    size_t end() const { return off + bytes(); }
    T* in(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};
// The cursor that hands the fields out, front to back.  take() starts a field on the next multiple of Align (a power of two),
// pack() directly behind the field before it; a field of no elements takes no room.  bytes(): the block, a multiple of Align.
template <size_t Align>
struct MmlCarve {
    size_t last = 0;  // end of the last field
    static size_t up(size_t b) { return (b + (Align - 1)) & ~(Align - 1); }
    template <class T>
    MmlField<T> take(size_t n) {
        const MmlField<T> f{up(last), n};
        last = f.end();
        return f;
    }
    template <class T>
    MmlField<T> pack(size_t n) {
        const MmlField<T> f{last, n};
        last = f.end();
        return f;
    }
    size_t bytes() const { return up(last); }
};

// The scratch structs of the side calls (the batched calls beside the scan pipeline), one slot per call family.  get<D>(i)
// creates slot i's struct on first use; release() deletes them all, and a struct's destructor releases its own buffers.
template <int N>
struct MmlSides {
    struct Slot {
        void* p = nullptr;
        void (*drop)(void*) = nullptr;
    } slot[N];
    template <class D>
    static void drop_as(void* p) {
        delete static_cast<D*>(p);
    }
    template <class D>
    D* get(int i) {
        if (!slot[i].p) slot[i] = Slot{new D(), &drop_as<D>};
        return static_cast<D*>(slot[i].p);
    }
    void release() {
        for (Slot& s : slot) {
            if (s.p) s.drop(s.p);
            s = Slot{};
        }
    }
};

#endif
