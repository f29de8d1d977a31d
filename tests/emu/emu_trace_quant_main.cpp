// emu_trace_quant_main.cpp -- tests/emu/emu_trace_quant.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_trace_quant_abi.py builds and runs it): (6, 3) and (1, 1) at batches around a wave, the workgroup and its second round, every
// non-empty `what`, with and without limits, with and without an estimate, one level and eight, three walk orders; ages 0, 2, FALLBACK and
// HELD with NaN controls in the held rows; rows built to break a radix select -- all equal, two values, the lowest byte alone, signed zeros,
// denormals, +-1e308, non-finite entries, nothing finite --; then a buffer of 3 slots driven over 10 ticks with every = 2.  Every array has
// exactly the elements the kernel may touch, the output exactly its doubles.  The x and u rows are checked against a sort of the finite
// values by the key, written here a second time.  Exit status 0: every walk ran, the walk orders agree byte for byte and the sort agrees.
#include "emu_trace_quant.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Lcg {
    unsigned long long s;
    unsigned long long word()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return s;
    }
    double next() { return (double)(word() >> 11) / 9007199254740992.0 - 0.5; }
};

std::vector<double> rnd(Lcg& g, size_t n, double scale = 1.0, double shift = 0.0)
{
    std::vector<double> v(n);
    for (double& x : v) x = shift + scale * g.next();
    return v;
}

const double kLevels[8] = { 0.0, 1.0, 0.5, 1.0 / 3.0, 1e-9, 0.999, 0.5, 0.05 };

unsigned long long bits_of(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// the rule, by sorting: the finite values of `v` by their key, rank k of level p
unsigned long long by_sort(const std::vector<double>& v, double p)
{
    std::vector<unsigned long long> keys;
    for (double x : v)
        if (std::isfinite(x)) {
            const unsigned long long b = bits_of(x);
            keys.push_back(b ^ ((b >> 63) ? ~0ull : 1ull << 63));
        }
    if (keys.empty()) return 0x7FF8000000000000ull;
    std::sort(keys.begin(), keys.end());
    const long long n = (long long)keys.size(), c = (long long)std::ceil(p * (double)n);
    const long long k = std::min(n - 1, std::max(0ll, c - 1));
    const unsigned long long key = keys[(size_t)k];
    return key ^ ((key >> 63) ? 1ull << 63 : ~0ull);
}

int run_shape(int nx, int nu)
{
    int bad = 0;
    Lcg g { (unsigned long long)(1000 * nx + nu) };
    const int pattern[4] = { 0, 2, -1, -2 };
    for (int batch : { 1, 63, 65, 257, 1025, 2049 }) {
        const size_t b = (size_t)batch;
        auto x = rnd(g, b * nx, 4.0), u = rnd(g, b * nu, 4.0), est = rnd(g, b * nx, 4.0);
        auto xlo = rnd(g, nx, 0.5, -1.0), xhi = rnd(g, nx, 0.5, 1.0), ulo = rnd(g, nu, 0.5, -1.0), uhi = rnd(g, nu, 0.5, 1.0);
        std::vector<int> age(b);
        for (size_t i = 0; i < b; ++i) {
            age[i] = pattern[(i * 7 + 3) % 4];
            if (age[i] == -2)
                for (int c = 0; c < nu; ++c) u[i * nu + c] = NAN; // (held: its control is never used)
        }
        x[(b / 2) * nx] = NAN;
        for (int what = 1; what < 8; ++what)
            for (int limits = 0; limits < 2; ++limits)
                for (int live = 0; live < 2; ++live)
                    for (int nq : { 1, 8 }) {
                        const int rows = ((what & 1) ? nx : 0) + ((what & 2) ? nu : 0) + ((what & 4) ? nx : 0) + limits;
                        std::vector<double> first;
                        for (int order = 0; order < 3; ++order) {
                            std::vector<double> out((size_t)rows * nq); // (exactly the slot's doubles)
                            EmuQuantTick t;
                            std::memset(&t, 0, sizeof t);
                            t.batch = batch, t.nx = nx, t.nu = nu, t.what = what, t.order = order, t.nq = nq, t.seed = 7;
                            t.x = x.data(), t.u = u.data(), t.est = live ? est.data() : nullptr, t.age = age.data();
                            if (limits) t.x_lo = xlo.data(), t.x_hi = xhi.data(), t.u_lo = ulo.data(), t.u_hi = uhi.data();
                            for (int q = 0; q < nq; ++q) t.level[q] = kLevels[(q + what) % 8];
                            t.out = out.data();
                            if (emu_trace_quant_tick(&t) != 0 || t.rows != rows) return 1;
                            if (first.empty()) first = out;
                            if (std::memcmp(first.data(), out.data(), out.size() * sizeof(double)) != 0) {
                                std::printf("nx %d nu %d batch %d what %d limits %d live %d nq %d: order %d disagrees\n", nx, nu, batch, what, limits, live, nq, order);
                                ++bad;
                            }
                        }
                        if (what & 1) // the x rows against the sort
                            for (int r = 0; r < nx; ++r) {
                                std::vector<double> col(b);
                                for (size_t i = 0; i < b; ++i) col[i] = x[i * nx + r];
                                for (int q = 0; q < nq; ++q)
                                    if (bits_of(first[(size_t)r * nq + q]) != by_sort(col, kLevels[(q + what) % 8])) {
                                        std::printf("nx %d nu %d batch %d what %d nq %d: x row %d level %d is not the sort's\n", nx, nu, batch, what, nq, r, q);
                                        ++bad;
                                    }
                            }
                    }
    }
    return bad;
}

int run_column(const char* name, const std::vector<double>& v)
{
    int bad = 0;
    const int batch = (int)v.size();
    std::vector<double> u((size_t)batch, 0.0);
    std::vector<int> age((size_t)batch, 0);
    for (int order = 0; order < 3; ++order) {
        std::vector<double> out(8);
        EmuQuantTick t;
        std::memset(&t, 0, sizeof t);
        t.batch = batch, t.nx = 1, t.nu = 1, t.what = 1, t.order = order, t.nq = 8, t.seed = 5;
        t.x = v.data(), t.u = u.data(), t.age = age.data();
        for (int q = 0; q < 8; ++q) t.level[q] = kLevels[q];
        t.out = out.data();
        if (emu_trace_quant_tick(&t) != 0 || t.rows != 1) return 1;
        for (int q = 0; q < 8; ++q)
            if (bits_of(out[(size_t)q]) != by_sort(v, kLevels[q])) {
                std::printf("%s: order %d level %d is not the sort's\n", name, order, q);
                ++bad;
            }
    }
    return bad;
}

int run_edges()
{
    Lcg g { 99 };
    int bad = 0;
    bad += run_column("all equal", std::vector<double>(300, 0.7));
    std::vector<double> two(301), low(700), zeros(200), den(300), huge(129), mixed(1500), none(90);
    for (double& x : two) x = g.next() < -0.2 ? -2.5 : 4.0;
    for (double& x : low) {
        const unsigned long long b = (bits_of(1.2345678) & ~0xFFull) | (g.word() >> 56);
        std::memcpy(&x, &b, sizeof x);
    }
    for (double& x : zeros) x = g.next() < 0.0 ? -0.0 : 0.0;
    for (size_t i = 0; i < den.size(); ++i) {
        const unsigned long long b = ((g.word() >> 24) | 1ull) | (i % 2 ? 1ull << 63 : 0ull);
        std::memcpy(&den[i], &b, sizeof(double));
    }
    for (double& x : huge) x = (g.next() < 0.0 ? -1e308 : 1e308) * (0.95 + 0.1 * g.next());
    for (size_t i = 0; i < mixed.size(); ++i) {
        mixed[i] = std::ldexp(g.next(), (int)(g.word() >> 55) - 256);
        if (i % 7 == 3) mixed[i] = NAN;
        if (i % 31 == 5) mixed[i] = INFINITY;
        if (i % 37 == 6) mixed[i] = -INFINITY;
    }
    for (size_t i = 0; i < none.size(); ++i) none[i] = i % 3 == 0 ? NAN : i % 3 == 1 ? INFINITY : -INFINITY;
    bad += run_column("two values", two) + run_column("lowest byte", low) + run_column("signed zeros", zeros) + run_column("denormals", den);
    bad += run_column("huge", huge) + run_column("mixed", mixed) + run_column("nothing finite", none) + run_column("one", { -3.5 });
    return bad;
}

int run_clock()
{
    const int nx = 3, nu = 1, batch = 70, what = 3, nq = 3, rows = 4;
    Lcg g { 11 };
    auto x = rnd(g, (size_t)batch * nx), u = rnd(g, (size_t)batch * nu);
    std::vector<int> age((size_t)batch, 0);
    std::vector<double> buffer((size_t)3 * rows * nq, -7.25); // (exactly the buffer's slots)
    EmuQuantClock clock { 0, 0, 0, 3, 2 };
    for (int tick = 0; tick < 10; ++tick) {
        EmuQuantTick t;
        std::memset(&t, 0, sizeof t);
        t.batch = batch, t.nx = nx, t.nu = nu, t.what = what, t.nq = nq;
        t.x = x.data(), t.u = u.data(), t.age = age.data();
        t.level[0] = 0.05, t.level[1] = 0.5, t.level[2] = 0.95;
        const long long slot = emu_trace_quant_record(&t, &clock, buffer.data());
        if (slot < -1) return 1;
    }
    int untouched = 0;
    for (double v : buffer) untouched += v == -7.25;
    return !(clock.tick == 10 && clock.recorded == 3 && clock.missed == 2 && untouched == 0);
}

} // namespace

int main()
{
    int levels = 0, threads = 0, lds = 0;
    emu_trace_quant_sizes(&levels, &threads, &lds);
    int bad = (levels != 8) + (threads % 64 != 0);
    bad += run_shape(6, 3) + run_shape(1, 1) + run_edges() + run_clock();
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
