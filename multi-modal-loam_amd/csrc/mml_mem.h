// mml_mem.h -- the one place of libmmloam_hip.so that allocates and frees device and pinned memory.  Four owners, one per
// lifetime: MmlFixed (allocated by a create call, freed by its destroy), MmlStaging (grow-only), MmlGroup (several buffers that
// exist together or not at all) and MmlTemp (one call).  Host code only: a program without kernels can include it.
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

#endif
