// The failure paths of csrc/mml_mem.h on a machine without a device, where every hipMalloc and hipHostMalloc fails and leaves its
// pointer null: each owner must read as empty afterwards, fail the same way again, and release any number of times.  Also the
// two helpers that need no device at all: MmlCarve on a host block, and MmlSides with stand-in scratch structs.  Built
// with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_mem_owner.py; exits 0 when every check holds.
#include <stdint.h>
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

struct Rec24 {  // a record whose size is no multiple of any alignment below
    double a, b;
    float c;
    int d;
};

// MmlCarve<A>: where the fields lie, and a block carved by it written and read back end to end (every byte of every field, and
// nothing outside the block, or AddressSanitizer stops the program)
template <size_t A>
static void carve() {
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)255, (size_t)256, (size_t)257}) {
        MmlCarve<A> c;
        CHECK(c.bytes() == 0);
        const auto ints = c.template take<int>(n + 1);
        const auto recs = c.template take<Rec24>(n);
        const auto none = c.template take<double>(0);  // no elements: no room, and the next field starts where it would have
        const auto dbl = c.template take<double>(7 * n);
        const auto raw = c.template take<char>(2 * n);
        const auto tail = c.template pack<uint16_t>(3);  // directly behind `raw`, wherever that ends
        const size_t off[] = {ints.off, recs.off, none.off, dbl.off, raw.off}, end[] = {ints.end(), recs.end(), none.end(), dbl.end(), raw.end()};
        CHECK(ints.off == 0);
        for (int i = 0; i < 5; ++i) {
            CHECK(off[i] % A == 0);
            CHECK(i == 0 || (off[i] >= end[i - 1] && off[i] - end[i - 1] < A));  // in order, disjoint, padded by less than A
        }
        CHECK(ints.n == n + 1 && ints.bytes() == sizeof(int) * (n + 1) && recs.bytes() == sizeof(Rec24) * n);
        CHECK(none.n == 0 && none.bytes() == 0 && none.end() == none.off && dbl.off == none.off);
        CHECK(tail.off == raw.end() && tail.bytes() == 6);
        CHECK(c.bytes() % A == 0 && c.bytes() >= tail.end() && c.bytes() - tail.end() < A);  // the last field's end, rounded up

        std::vector<char> blk(c.bytes());
        blk[c.bytes() - 1] = 7;  // (padding, or the last field's last byte: rewritten below)
        int* pi = ints.in(blk.data());
        Rec24* pr = recs.in(blk.data());
        double* pd = dbl.in(blk.data());
        char* pc = raw.in(blk.data());
        CHECK((char*)pi == blk.data() + ints.off && (char*)pr == blk.data() + recs.off && (char*)pd == blk.data() + dbl.off);
        for (size_t i = 0; i < ints.n; ++i) pi[i] = (int)i;
        for (size_t i = 0; i < recs.n; ++i) pr[i] = Rec24{(double)i, -(double)i, (float)i, (int)i};
        for (size_t i = 0; i < dbl.n; ++i) pd[i] = 0.5 * (double)i;
        for (size_t i = 0; i < raw.n; ++i) pc[i] = (char)(i & 127);
        uint16_t* pt = tail.in(blk.data());  // (2-byte aligned: `raw` has an even number of bytes)
        for (size_t i = 0; i < tail.n; ++i) pt[i] = (uint16_t)(1000 + i);
        size_t wrong = 0;  // the fields did not overwrite each other
        for (size_t i = 0; i < ints.n; ++i) wrong += pi[i] != (int)i;
        for (size_t i = 0; i < recs.n; ++i) wrong += !(pr[i].a == (double)i && pr[i].b == -(double)i && pr[i].c == (float)i && pr[i].d == (int)i);
        for (size_t i = 0; i < dbl.n; ++i) wrong += pd[i] != 0.5 * (double)i;
        for (size_t i = 0; i < raw.n; ++i) wrong += pc[i] != (char)(i & 127);
        for (size_t i = 0; i < tail.n; ++i) wrong += pt[i] != (uint16_t)(1000 + i);
        CHECK(wrong == 0);
    }
    MmlCarve<A> empty;  // a block of nothing but empty fields
    CHECK(empty.template take<float>(0).off == 0 && empty.template take<int>(0).off == 0 && empty.bytes() == 0);
}

// stand-ins for the side calls' scratch structs: buffers released by the destructor, which counts
static int side_alive = 0;
struct SideA {
    MmlStaging<char> io;
    MmlStaging<double, false> big;
    SideA() { ++side_alive; }
    ~SideA() {
        io.release();
        big.release();
        --side_alive;
    }
};
struct SideB {
    MmlStaging<int> tab;
    std::vector<int> kept = std::vector<int>(100, 1);  // heap of its own: LeakSanitizer reports it unless the destructor ran
    SideB() { ++side_alive; }
    ~SideB() {
        tab.release();
        --side_alive;
    }
};

static void sides() {
    Ctx ctx;
    MmlSides<3> s;  // slot 1 stays unused
    s.release();    // nothing created yet
    for (int round = 0; round < 2; ++round) {
        SideA* a = s.get<SideA>(0);
        CHECK(a != nullptr && side_alive == 1);
        CHECK(s.get<SideA>(0) == a && side_alive == 1);  // created once
        CHECK(a->io.reserve(&ctx, 4096) == MML_ERR_HIP && !ctx.err.empty());
        CHECK(a->io.cap == 0 && a->io.d == nullptr && a->io.h == nullptr);
        CHECK(a->big.reserve(&ctx, 10) == MML_ERR_HIP && a->big.cap == 0 && a->big.d == nullptr);
        CHECK(s.get<SideA>(0) == a);  // and still there for the next call to try again
        SideB* b = s.get<SideB>(2);
        CHECK((void*)b != (void*)a && side_alive == 2 && s.get<SideB>(2) == b);
        CHECK(b->tab.reserve(&ctx, 1) == MML_ERR_HIP && b->tab.cap == 0);
        CHECK(s.slot[1].p == nullptr);
        s.release();
        CHECK(side_alive == 0 && s.slot[0].p == nullptr && s.slot[2].p == nullptr);
        s.release();  // again: nothing left to delete
        CHECK(side_alive == 0);
    }
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
    carve<8>();
    carve<16>();
    carve<256>();
    sides();
    if (failures) return 1;
    printf("mem_owner_replay ok\n");
    return 0;
}
