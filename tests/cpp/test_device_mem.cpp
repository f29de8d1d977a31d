// The owners of copra_amd/csrc/device_mem.hpp against a counting allocator: what they release, when, and what a failed attempt leaves;
// and DevArg, the borrowed-or-owned input array: which pointer is in force, when its copy grows, what a failed allocation or copy leaves.
// Stand-alone (g++ -std=c++17 -fsanitize=address,undefined, no HIP): tests/test_device_mem.py builds and runs it.
#include "../../copra_amd/csrc/device_mem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>

struct Fake { // live blocks and bytes; the fail_at-th alloc from now on fails (1-based; 0: none), and so does the copy_fail_at-th copy_in
    static std::map<void*, size_t> live;
    static size_t bytes;
    static int allocs, releases, fail_at, copies, copy_fail_at;
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
        if (copy_fail_at > 0 && --copy_fail_at == 0) return 9;
        auto it = live.find(dst);
        if (it == live.end() || it->second < n) return 7;
        std::memcpy(dst, src, n);
        return 0;
    }
};
std::map<void*, size_t> Fake::live;
size_t Fake::bytes = 0;
int Fake::allocs = 0, Fake::releases = 0, Fake::fail_at = 0, Fake::copies = 0, Fake::copy_fail_at = 0;

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
template <class T>
using Arg = DevArg<T, Fake>;
static_assert(!std::is_copy_constructible<Arg<int>>::value && !std::is_copy_assignable<Arg<int>>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<Arg<int>>::value && std::is_nothrow_move_assignable<Arg<int>>::value, "cheap moves");

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

// A borrowed-or-owned input array: the view in force and the copy behind it
static void test_arg_borrow_and_copy()
{
    const int r0 = Fake::releases;
    {
        Arg<double> a;
        const double* p = a; // reads as the pointer in force
        CHECK(!a && p == nullptr && a.get() == nullptr && !a.copy() && nlive() == 0); // default: unset, nothing held
        a.unset(), a.reset();
        CHECK(Fake::releases == r0);
        const double host[6] = { 1.0, 2.0, 3.0, 4.0, 5.0, 6.0 };
        const int a0 = Fake::allocs, c0 = Fake::copies;
        CHECK(a.copy_in(host, 4) == 0 && a && a.get() == a.copy().get() && a.copy().count() == 4 && nlive() == 1);
        CHECK(Fake::allocs == a0 + 1 && Fake::copies == c0 + 1 && a[0] == 1.0 && a[3] == 4.0);
        const double* const block = a.copy().get();
        double theirs[2] = { 7.0, 8.0 };
        a.borrow(theirs); // the caller's array: the copy is kept for the next time
        CHECK(a.get() == theirs && a[1] == 8.0 && a.copy().get() == block && a.copy().count() == 4 && nlive() == 1 && Fake::releases == r0);
        CHECK(a.copy_in(host + 1, 3) == 0 && Fake::allocs == a0 + 1 && a.get() == block && a[0] == 2.0); // no larger: no allocation
        CHECK(a.copy_in(host, 4) == 0 && Fake::allocs == a0 + 1 && a.get() == block);
        CHECK(a.copy_in(host, 5) == 0 && Fake::allocs == a0 + 2 && Fake::releases == r0 + 1 && nlive() == 1); // too small: replaced
        CHECK(a.get() == a.copy().get() && a.copy().count() == 5 && a[4] == 5.0 && Fake::bytes == 5 * sizeof(double));
        a.borrow(nullptr); // (a null array borrowed is an array unset)
        CHECK(!a && a.copy().count() == 5 && nlive() == 1);
    }
    CHECK(nlive() == 0 && Fake::releases == r0 + 2);
}

static void test_arg_empty_copy()
{
    Arg<double> a;
    const int c0 = Fake::copies;
    CHECK(a.copy_in(nullptr, 0) == 0 && a && a.copy().count() == 1 && nlive() == 1 && Fake::copies == c0); // an address, no copy call
    const double* const block = a.get();
    const int a0 = Fake::allocs;
    CHECK(a.copy_in(nullptr, 0) == 0 && a.get() == block && Fake::allocs == a0 && Fake::copies == c0);
    const double one = 4.0;
    CHECK(a.copy_in(&one, 1) == 0 && a.get() == block && Fake::allocs == a0 && Fake::copies == c0 + 1 && a[0] == 4.0); // max(count, 1) is held
}

static void test_arg_failures()
{
    const double host[8] = { 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0 };
    double theirs[1] = { 0.0 };
    for (int held = 0; held < 2; ++held) { // from nothing held, and from a copy in force that has to grow
        Arg<double> a;
        if (held) CHECK(a.copy_in(host, 2) == 0 && a && nlive() == 1);
        Fake::fail_at = 1;
        CHECK(a.copy_in(host, 8) == 2 && Fake::fail_at == 0); // the allocation fails: the view is null, the old block went first
        CHECK(!a && a.get() == nullptr && !a.copy() && a.copy().count() == 0 && nlive() == 0 && Fake::bytes == 0);
        CHECK(a.copy_in(host, 8) == 0 && a && a.get() == a.copy().get() && a[7] == 8.0 && nlive() == 1); // ... and the next attempt succeeds
        a.borrow(theirs);
        Fake::copy_fail_at = 1;
        CHECK(a.copy_in(host, 8) == 9 && Fake::copy_fail_at == 0); // the copy fails: the view is null -- not the caller's array, not the
        CHECK(!a && a.copy().count() == 8 && nlive() == 1 && Fake::bytes == 8 * sizeof(double)); // block half written --, the block is held
        CHECK(a.copy_in(host, 3) == 0 && a.get() == a.copy().get() && a[2] == 3.0 && nlive() == 1);
    }
    CHECK(nlive() == 0);
}

static void test_arg_unset_and_reset()
{
    const double host[3] = { 1.0, 2.0, 3.0 };
    Arg<double> a;
    CHECK(a.copy_in(host, 3) == 0);
    const double* const block = a.get();
    const int r0 = Fake::releases, a0 = Fake::allocs;
    a.unset(); // off: the copy stays
    CHECK(!a && a.copy().get() == block && nlive() == 1 && Fake::releases == r0);
    CHECK(a.copy_in(host, 3) == 0 && a.get() == block && Fake::allocs == a0);
    a.reset(); // off: the copy goes
    CHECK(!a && !a.copy() && nlive() == 0 && Fake::releases == r0 + 1);
    a.reset();
    CHECK(Fake::releases == r0 + 1);
    CHECK(a.copy_in(host, 1) == 0 && a && Fake::allocs == a0 + 1);
}

// An entry of a list dropped as the engine drops a driven cost (target_drop_cost): the entries behind it move down by one, each view with
// its own copy
static void test_arg_moves()
{
    const double h0[2] = { 10.0, 11.0 }, h1[3] = { 20.0, 21.0, 22.0 }, h2[1] = { 30.0 };
    double theirs[1] = { 40.0 };
    {
        Arg<double> m[3];
        CHECK(m[0].copy_in(h0, 2) == 0 && m[1].copy_in(h1, 3) == 0 && m[2].copy_in(h2, 1) == 0 && nlive() == 3);
        const double *const b1 = m[1].get(), *const b2 = m[2].get();
        const int r0 = Fake::releases;
        m[0] = std::move(m[1]); // by assignment: the target's copy goes, exactly once
        CHECK(Fake::releases == r0 + 1 && nlive() == 2);
        CHECK(m[0].get() == b1 && m[0].get() == m[0].copy().get() && m[0].copy().count() == 3 && m[0][2] == 22.0);
        CHECK(!m[1] && !m[1].copy() && m[1].copy().count() == 0); // what was moved from is unset and holds nothing
        m[1] = std::move(m[2]);
        CHECK(Fake::releases == r0 + 1 && m[1].get() == b2 && m[1].get() == m[1].copy().get() && !m[2] && !m[2].copy());
        Arg<double>& self = m[1];
        m[1] = std::move(self); // self-move: harmless
        CHECK(m[1].get() == b2 && m[1].copy().get() == b2 && nlive() == 2);
        Arg<double> c(std::move(m[0]));
        CHECK(c.get() == b1 && c.copy().get() == b1 && !m[0] && !m[0].copy() && nlive() == 2 && Fake::releases == r0 + 1);
    }
    CHECK(nlive() == 0);
    {
        Arg<double> m[3]; // ... and by swaps, as the engine does it: the dropped entry's copy ends up behind the list, kept
        CHECK(m[0].copy_in(h0, 2) == 0 && m[1].copy_in(h1, 3) == 0 && m[2].copy_in(h2, 1) == 0);
        const double *const b0 = m[0].get(), *const b1 = m[1].get();
        m[2].borrow(theirs); // (a borrowed view travels too, with the copy it bypasses)
        const double* const b2 = m[2].copy().get();
        const int r0 = Fake::releases;
        m[0].unset();
        std::swap(m[0], m[1]), std::swap(m[1], m[2]);
        CHECK(Fake::releases == r0 && nlive() == 3);
        CHECK(m[0].get() == b1 && m[0].copy().get() == b1 && m[1].get() == theirs && m[1].copy().get() == b2 && !m[2] && m[2].copy().get() == b0);
    }
    CHECK(nlive() == 0); // every block once: a second release aborts in Fake::release
}

int main()
{
    test_empty();
    test_alloc_and_grow();
    CHECK(nlive() == 0);
    test_moves();
    test_bag();
    test_group();
    test_arg_borrow_and_copy();
    test_arg_empty_copy();
    CHECK(nlive() == 0);
    test_arg_failures();
    test_arg_unset_and_reset();
    CHECK(nlive() == 0);
    test_arg_moves();
    CHECK(nlive() == 0 && Fake::bytes == 0 && Fake::allocs > 0);
    std::printf("device_mem ok: %d allocations, %d releases, none live\n", Fake::allocs, Fake::releases);
    return 0;
}
