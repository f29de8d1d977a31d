// emu_trace_main.cpp -- tests/emu/emu_trace.cpp as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_trace_abi.py builds and runs it): (6, 3) and (3, 1) at instance counts around a wave, a thread count and a chunk, every
// non-empty `what`, with and without limits, with and without an estimate, through the image and through direct loads, three walk orders;
// ages 0, 2, FALLBACK and HELD with NaN controls in the held rows; then a trace of 3 slots driven over 10 ticks with every = 2.  Every array
// has exactly the elements the kernel may touch, the slot exactly its bytes.  Exit status 0: every walk ran, the walk orders and the two ways
// to the data agree byte for byte and the head counts are what the ages say.
#include "emu_trace.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Lcg {
    unsigned long long s;
    double next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0 - 0.5;
    }
};

std::vector<double> rnd(Lcg& g, size_t n, double scale = 1.0, double shift = 0.0)
{
    std::vector<double> v(n);
    for (double& x : v) x = shift + scale * g.next();
    return v;
}

int run_shape(int nx, int nu)
{
    int bad = 0;
    Lcg g { (unsigned long long)(1000 * nx + nu) };
    const int pattern[4] = { 0, 2, -1, -2 };
    for (int batch : { 1, 63, 65, 257, 1025 }) {
        const size_t b = (size_t)batch;
        auto x = rnd(g, b * nx, 4.0), u = rnd(g, b * nu, 4.0), est = rnd(g, b * nx, 4.0);
        auto xlo = rnd(g, nx, 0.5, -1.0), xhi = rnd(g, nx, 0.5, 1.0), ulo = rnd(g, nu, 0.5, -1.0), uhi = rnd(g, nu, 0.5, 1.0);
        std::vector<int> age(b);
        long long want[4] = { 0, 0, 0, 0 }; // solved, replayed, fallback, held
        for (size_t i = 0; i < b; ++i) {
            age[i] = pattern[(i * 7 + 3) % 4];
            want[age[i] == 0 ? 0 : age[i] >= 1 ? 1 : age[i] == -1 ? 2 : 3] += 1;
            if (age[i] == -2)
                for (int c = 0; c < nu; ++c) u[i * nu + c] = NAN; // (held: its control is never used)
        }
        x[(b / 2) * nx] = NAN;
        for (int what = 1; what < 8; ++what)
            for (int limits = 0; limits < 2; ++limits)
                for (int live = 0; live < 2; ++live) {
                    const int rows = emu_trace_rows(what, nx, nu, limits);
                    const size_t bytes = (size_t)emu_trace_slot_bytes(rows);
                    std::vector<unsigned char> first;
                    for (int lds = 0; lds < 2; ++lds)
                        for (int order = 0; order < 3; ++order) {
                            std::vector<unsigned char> slot(bytes);
                            EmuTraceTick t;
                            std::memset(&t, 0, sizeof t);
                            t.batch = batch, t.nx = nx, t.nu = nu, t.what = what, t.order = order, t.lds_mode = lds, t.vec2_mode = -1, t.seed = 7;
                            t.x = x.data(), t.u = u.data(), t.est = live ? est.data() : nullptr, t.age = age.data();
                            if (limits) t.x_lo = xlo.data(), t.x_hi = xhi.data(), t.u_lo = ulo.data(), t.u_hi = uhi.data();
                            t.tol = 0.25, t.tick = 5, t.tau = 6, t.slot = slot.data();
                            if (emu_trace_tick(&t) != 0 || t.rows != rows) return 1;
                            if (first.empty()) first = slot;
                            if (std::memcmp(first.data(), slot.data(), bytes) != 0) {
                                std::printf("nx %d nu %d batch %d what %d limits %d live %d: lds %d order %d disagrees\n", nx, nu, batch, what, limits, live, lds, order);
                                ++bad;
                            }
                        }
                    long long head[8];
                    std::memcpy(head, first.data(), sizeof head);
                    if (head[0] != 5 || head[1] != 6 || head[2] != want[0] || head[3] != want[1] || head[4] != want[2] || head[5] != want[3] || (!limits && head[6] != 0)
                        || head[7] != 0) {
                        std::printf("nx %d nu %d batch %d what %d limits %d: wrong head\n", nx, nu, batch, what, limits);
                        ++bad;
                    }
                }
    }
    return bad;
}

int run_clock()
{
    const int nx = 3, nu = 1, batch = 70, what = 3;
    const size_t bytes = (size_t)emu_trace_slot_bytes(emu_trace_rows(what, nx, nu, 0));
    Lcg g { 11 };
    auto x = rnd(g, (size_t)batch * nx), u = rnd(g, (size_t)batch * nu);
    std::vector<int> age((size_t)batch, 0);
    std::vector<unsigned char> buffer(3 * bytes); // (exactly the trace's slots)
    EmuTraceClock clock { 0, 0, 0, 3, 2 };
    for (int tick = 0; tick < 10; ++tick) {
        EmuTraceTick t;
        std::memset(&t, 0, sizeof t);
        t.batch = batch, t.nx = nx, t.nu = nu, t.what = what, t.lds_mode = -1, t.vec2_mode = -1;
        t.x = x.data(), t.u = u.data(), t.age = age.data(), t.tau = tick + 1;
        const long long slot = emu_trace_record(&t, &clock, buffer.data());
        if (slot < -1) return 1;
    }
    long long tick2 = 0;
    std::memcpy(&tick2, buffer.data() + 2 * bytes, sizeof tick2);
    return !(clock.tick == 10 && clock.recorded == 3 && clock.missed == 2 && tick2 == 4);
}

} // namespace

int main()
{
    int head = 0, stat = 0;
    emu_trace_sizes(&head, &stat);
    int bad = (head != 64) + (stat != 56) + (emu_trace_slot_bytes(16) != 64 + 56 * 16);
    bad += run_shape(6, 3) + run_shape(3, 1) + run_clock();
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
