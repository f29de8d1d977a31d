// The owners of copra_amd/csrc/device_mem.hpp against a counting allocator: what they release, when, and what a failed attempt leaves.
// Stand-alone (g++ -std=c++17 -fsanitize=address,undefined, no HIP): tests/test_device_mem.py builds and runs it.
#include "../../copra_amd/csrc/device_mem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>

struct Fake { // live blocks and bytes; the fail_at-th alloc from now on fails (1-based; 0: none)
    static std::map<void*, size_t> live;
    static size_t bytes;
    static int allocs, releases, fail_at, copies;
    static int alloc(void** p, size_t n)
    {
        ++allocs;
        if (fail_at > 0 && --fail_at == 0) return 2;
        *p = std::malloc(n ? n : 1);
        live[*p] = n, bytes += n;
        return 0;
    }
    static void release(void* p)
    {
        ++releases;
        auto it = live.find(p);
        if (it == live.end()) {
            std::fprintf(stderr, "release of a block that is not live\n");
            std::abort();
        }
        bytes -= it->second;
        live.erase(it);
        std::free(p);
    }
    static int copy_in(void* dst, const void* src, size_t n)
    {
        ++copies;
        auto it = live.find(dst);
        if (it == live.end() || it->second < n) return 7;
        std::memcpy(dst, src, n);
        return 0;
    }
};
std::map<void*, size_t> Fake::live;
size_t Fake::bytes = 0;
int Fake::allocs = 0, Fake::releases = 0, Fake::fail_at = 0, Fake::copies = 0;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

template <class T>
using Buf = DevBuf<T, Fake>;
static_assert(!std::is_copy_constructible<Buf<int>>::value && !std::is_copy_assignable<Buf<int>>::value, "move-only");
static_assert(!std::is_copy_constructible<DevBag<Fake>>::value && !std::is_copy_assignable<DevBag<Fake>>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<Buf<int>>::value && std::is_nothrow_move_assignable<Buf<int>>::value, "cheap moves");

static size_t nlive() { return Fake::live.size(); }

static void test_empty()
{
    const int r0 = Fake::releases;
    {
        Buf<double> b;
        CHECK(!b && b.get() == nullptr && b.count() == 0);
        double* p = b; // reads as the pointer
        CHECK(p == nullptr);
        b.reset();
    }
    CHECK(Fake::releases == r0 && nlive() == 0);
}

static void test_alloc_and_grow()
{
    Buf<double> b;
    CHECK(b.alloc(10) == 0 && b && b.count() == 10 && nlive() == 1 && Fake::bytes == 10 * sizeof(double));
    b[9] = 3.0;
    CHECK(*(b + 9) == 3.0);
    double* first = b;
    const int r0 = Fake::releases;
    CHECK(b.alloc(4) == 0 && Fake::releases == r0 + 1 && nlive() == 1 && b.count() == 4 && Fake::bytes == 4 * sizeof(double)); // released first
    first = b;
    CHECK(b.grow(3) == 0 && b.get() == first && b.count() == 4 && Fake::releases == r0 + 1); // large enough: kept
    CHECK(b.grow(4) == 0 && b.get() == first);
    CHECK(b.grow(5) == 0 && b.count() == 5 && Fake::releases == r0 + 2 && nlive() == 1); // too small: replaced
    Fake::fail_at = 1;
    CHECK(b.alloc(6) == 2 && !b && b.count() == 0 && nlive() == 0); // a failed attempt leaves it empty (the old block went first)
    Fake::fail_at = 1;
    CHECK(b.grow(1) == 2 && !b);
    CHECK(b.grow(1) == 0 && b.count() == 1);
    b.reset();
    CHECK(!b && nlive() == 0);
    Buf<int> e;
    CHECK(e.grow(0) == 0 && nlive() == 1); // (an empty buffer grows even to nothing: `if (!x) alloc`)
}

static void test_moves()
{
    Buf<int> a, b;
    CHECK(a.alloc(3) == 0 && b.alloc(5) == 0 && nlive() == 2);
    int* pa = a;
    const int r0 = Fake::releases;
    b = std::move(a); // the target's block goes, exactly once
    CHECK(Fake::releases == r0 + 1 && nlive() == 1 && !a && a.count() == 0 && b.get() == pa && b.count() == 3);
    Buf<int> c(std::move(b));
    CHECK(!b && b.count() == 0 && c.get() == pa && c.count() == 3 && Fake::releases == r0 + 1);
    Buf<int>& self = c;
    c = std::move(self); // self-move: harmless
    CHECK(c.get() == pa && c.count() == 3 && nlive() == 1 && Fake::releases == r0 + 1);
    c = Buf<int>(); // an empty one moved in: releases
    CHECK(!c && nlive() == 0 && Fake::releases == r0 + 2);
}

static void test_bag()
{
    const int r0 = Fake::releases;
    {
        DevBag<Fake> bag;
        std::vector<double> v = { 1.0, 2.0, 3.0 };
        std::vector<int> none;
        double* d = bag.add(v.size(), &v);
        CHECK(d && d[0] == 1.0 && d[2] == 3.0 && Fake::copies == 1);
        int* z = bag.add(none.size(), &none); // an empty table still has an address; nothing to copy
        CHECK(z && Fake::copies == 1 && Fake::bytes == 3 * sizeof(double) + sizeof(int));
        CHECK(bag.add<long long>(7) != nullptr && bag.size() == 3 && bag.error() == 0);
        Fake::fail_at = 1;
        CHECK(bag.add<int>(2) == nullptr && bag.error() == 2 && bag.size() == 3);
        CHECK(bag.add<int>(2) != nullptr && bag.error() == 2 && bag.size() == 4); // the FIRST error stays
        DevBag<Fake> other(std::move(bag));
        CHECK(bag.size() == 0 && bag.error() == 0 && other.size() == 4 && other.error() == 2 && nlive() == 4);
        bag.add<int>(1);
        bag = std::move(other); // the target's block goes
        CHECK(nlive() == 4 && bag.size() == 4 && other.size() == 0 && Fake::releases == r0 + 1);
        DevBag<Fake>& self = bag;
        bag = std::move(self);
        CHECK(bag.size() == 4 && nlive() == 4);
    }
    CHECK(nlive() == 0 && Fake::releases == r0 + 5); // every block once
    DevBag<Fake> bag;
    bag.add<int>(1), bag.add<int>(1);
    bag.reset();
    CHECK(nlive() == 0 && bag.size() == 0 && bag.error() == 0);
}

// The all-or-none group as the engine writes it: five buffers built in locals, moved into the handle once every one succeeded.
struct Handle {
    Buf<int> count, list, hist;
    Buf<double> ws, ws2;
};
static int ensure_group(Handle& h, size_t n)
{
    Buf<int> count, list, hist;
    Buf<double> ws, ws2;
    int e = count.alloc(4);
    if (e == 0) e = list.alloc(n);
    if (e == 0) e = hist.alloc(16);
    if (e == 0) e = ws.alloc(3 * n);
    if (e == 0) e = ws2.alloc(5 * n);
    if (e != 0) return e;
    h.count = std::move(count), h.list = std::move(list), h.hist = std::move(hist), h.ws = std::move(ws), h.ws2 = std::move(ws2);
    return 0;
}
static void test_group()
{
    for (int held = 0; held < 2; ++held) {
        for (int k = 1; k <= 5; ++k) {
            Handle h;
            if (held) CHECK(ensure_group(h, 8) == 0 && nlive() == 5);
            void* const before[5] = { h.count.get(), h.list.get(), h.hist.get(), h.ws.get(), h.ws2.get() };
            const size_t counts[5] = { h.count.count(), h.list.count(), h.hist.count(), h.ws.count(), h.ws2.count() };
            const size_t live0 = nlive(), bytes0 = Fake::bytes;
            Fake::fail_at = k;
            CHECK(ensure_group(h, 32) == 2);
            CHECK(Fake::fail_at == 0);
            void* const after[5] = { h.count.get(), h.list.get(), h.hist.get(), h.ws.get(), h.ws2.get() };
            const size_t counts1[5] = { h.count.count(), h.list.count(), h.hist.count(), h.ws.count(), h.ws2.count() };
            for (int i = 0; i < 5; ++i) CHECK(after[i] == before[i] && counts1[i] == counts[i]); // the handle exactly as it was
            CHECK(nlive() == live0 && Fake::bytes == bytes0 && live0 == (held ? 5u : 0u)); // nothing live beyond it
            CHECK(ensure_group(h, 32) == 0 && nlive() == 5 && h.list.count() == 32); // ... and the next attempt replaces the whole group
        }
        CHECK(nlive() == 0);
    }
}

int main()
{
    test_empty();
    test_alloc_and_grow();
    CHECK(nlive() == 0);
    test_moves();
    test_bag();
    test_group();
    CHECK(nlive() == 0 && Fake::bytes == 0 && Fake::allocs > 0);
    std::printf("device_mem ok: %d allocations, %d releases, none live\n", Fake::allocs, Fake::releases);
    return 0;
}
