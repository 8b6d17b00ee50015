// The failure paths of csrc/mml_mem.h on a machine without a device, where every hipMalloc and hipHostMalloc fails and leaves its
// pointer null: each owner must read as empty afterwards, fail the same way again, and release any number of times.  Built
// with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_mem_owner.py; exits 0 when every check holds.
#include <stdio.h>

#include "mml_mem.h"

struct Ctx {
    std::string err;
};

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                             \
        }                                                           \
    } while (0)

template <bool Pinned>
static void staging(bool with_stream) {
    Ctx ctx;
    MmlStaging<double, Pinned> b;
    for (int round = 0; round < 2; ++round) {
        ctx.err.clear();
        const int rc = with_stream ? b.reserve(&ctx, 1000, nullptr) : b.reserve(&ctx, 1000);
        CHECK(rc == MML_ERR_HIP);
        CHECK(b.cap == 0 && b.d == nullptr && b.h == nullptr);
        CHECK(!ctx.err.empty());
    }
    CHECK(b.reserve(&ctx, 0) == MML_OK && b.cap == 0);  // nothing asked for: nothing to do
    b.release();
    b.release();
    CHECK(b.cap == 0 && b.d == nullptr && b.h == nullptr);
}

static void group() {
    Ctx ctx;
    float* a = reinterpret_cast<float*>(8);  // stale values: a failed reserve() must null them
    int* b = reinterpret_cast<int*>(8);
    void* c = reinterpret_cast<void*>(8);
    MmlGroup g;
    CHECK(!g.present());
    for (int round = 0; round < 2; ++round) {
        ctx.err.clear();
        const int rc = g.reserve(&ctx, {mml_part(a, 100), mml_part(b, 7), MmlPart{&c, 64}});
        CHECK(rc == MML_ERR_HIP);
        CHECK(!g.present() && g.dev.empty());
        CHECK(a == nullptr && b == nullptr && c == nullptr);
        CHECK(!ctx.err.empty());
    }
    g.release();
    g.release();
    CHECK(!g.present());
}

static void temp() {
    {
        MmlTemp<int> t;  // never allocated
    }
    MmlTemp<float> t;
    CHECK(t.alloc(256) != hipSuccess);
    CHECK(t.d == nullptr);
    CHECK(t.alloc(256) != hipSuccess && t.d == nullptr);
}

static void fixed() {
    MmlFixed f;
    f.release();  // empty
    double* p = reinterpret_cast<double*>(8);
    unsigned long long* q = reinterpret_cast<unsigned long long*>(8);
    CHECK(f.alloc(&p, 16) != hipSuccess && p == nullptr);
    CHECK(f.alloc(&p, 0) != hipSuccess && p == nullptr);
    CHECK(f.alloc_pinned(&q, 1) != hipSuccess && q == nullptr);
    CHECK(f.dev.empty() && f.pinned.empty());  // a failed allocation is not recorded
    f.dev.assign(3, nullptr);                  // and nulls that were are passed over
    f.pinned.assign(2, nullptr);
    f.release();
    CHECK(f.dev.empty() && f.pinned.empty());
    f.release();
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        fprintf(stderr, "a device is visible: this program replays the paths of a machine without one\n");
        return 2;
    }
    staging<true>(false);
    staging<true>(true);
    staging<false>(false);
    staging<false>(true);
    group();
    temp();
    fixed();
    if (failures) return 1;
    printf("mem_owner_replay ok\n");
    return 0;
}
